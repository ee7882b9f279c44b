"""The float64 references of tests/shim_kernels.py, validated on the CPU before any kernel is compared with them: chained into the three PCG schedules the
library runs they must solve a small SPD system and agree with each other; chained into the LM loop they must reproduce the float64 LM loop that
tests/test_gpu_double.py writes out (test_double_precision_levenberg_marquardt_against_float64, its inner `for k in range(L)` loop, restated here line by line).
No device, no library."""
import numpy as np
import pytest

import shim_kernels as sk


def _spd_system(n=37, width=7, seed=5):
    """5-point Laplacian of a `width`-wide row-major grid cut off after n nodes, plus a random positive diagonal"""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for i in range(n):
        for j in (i - 1, i + 1):
            if 0 <= j < n and j // width == i // width: A[i, j] = -1.0
        for j in (i - width, i + width):
            if 0 <= j < n: A[i, j] = -1.0
    A += np.diag(-A.sum(axis=1) + rng.uniform(0.5, 2.0, n))
    return A, rng.standard_normal(n)


def _schedule_step2_step3(A, b, pre, K):
    """PCGStep1 (A p), thallo_hip_pcg_step2_full, thallo_hip_pcg_step3: the reference-shaped loop"""
    r = b.copy(); z = pre * r; p = z.copy(); delta = np.zeros_like(b); aN = r @ z
    for _ in range(K):
        Ap = A @ p; aD = p @ Ap
        alpha = aN / aD if aD != 0 else 0.0
        delta, r, z, bn, _q = sk.ref_step2_full(delta, p, r, Ap, pre, None, alpha)
        bN = bn.sum()
        beta = bN / aN if aN != 0 else 0.0
        p = sk.ref_step3(p, z, beta); aN = bN
    return delta


def _schedule_pupdate_step2(A, b, pre, K):
    """thallo_hip_pcg_pupdate (PCGStep3 of k-1 + the delta update of k-1), A p, thallo_hip_pcg_step2; thallo_hip_linear_update's pending term at the end"""
    r = b.copy(); z = pre * r; p = np.zeros_like(b); delta = np.zeros_like(b); aN = r @ z
    alpha = beta = 0.0
    for k in range(K):
        p, delta = sk.ref_pupdate(z, p, delta, alpha, beta, first=(k == 0))
        Ap = A @ p; aD = p @ Ap
        alpha = aN / aD if aD != 0 else 0.0
        r, z, bn = sk.ref_step2(r, Ap, pre, alpha)
        bN = bn.sum()
        beta = bN / aN if aN != 0 else 0.0
        aN = bN
    _, delta = sk.ref_linear_update_n(None, delta, [p], [alpha])
    return delta


def _schedule_update_scalars(A, b, pre, K):
    """thallo_hip_pcg_update, A p with the sums alphaD / N, S1, S2 (thallo_hip_block_sums' terms), thallo_hip_pcg_scalars_finish's betaN = N - 2 alpha S1 + alpha^2 S2"""
    r = b.copy(); p = np.zeros_like(b); delta = np.zeros_like(b); aN = r @ (pre * r)
    alpha = beta = 0.0; Ap = None
    for k in range(K):
        r, p, delta = sk.ref_pcg_update(r, Ap, pre, p, delta, alpha, beta, first=1 if k == 0 else 0)
        Ap = A @ p
        ad, n_, s1, s2 = sk.ref_block_sums(p, Ap, r, pre)
        aD = ad.sum()
        alpha = aN / aD if aD != 0 else 0.0
        bN, _mag = sk.beta_n_f64(n_.sum(), s1.sum(), s2.sum(), alpha)
        beta = bN / aN if aN != 0 else 0.0
        aN = bN
    _, delta = sk.ref_linear_update_n(None, delta, [p], [alpha])
    return delta


def test_the_three_pcg_schedules_of_the_references_solve_an_spd_system():
    """The per-kernel references chained into (a) step2_full + step3, (b) pupdate + step2, (c) pcg_update + the N, S1, S2 scalars: the same iterates to 1e-12 after 10
    iterations, and after K = 30 the solution of numpy.linalg.solve within the CG bound 2 sqrt(kappa) rho^K, rho = (sqrt(kappa) - 1) / (sqrt(kappa) + 1), kappa the condition
    number of the Jacobi-preconditioned matrix (the energy-norm bound times sqrt(kappa) for the 2-norm), plus 1e-12 for the float64 arithmetic."""
    A, b = _spd_system()
    assert np.linalg.eigvalsh(A).min() > 0
    pre = 1.0 / np.diag(A)
    sched = (_schedule_step2_step3, _schedule_pupdate_step2, _schedule_update_scalars)
    d10 = [f(A, b, pre, 10) for f in sched]
    scale = np.abs(d10[0]).max()
    for d in d10[1:]:
        assert np.abs(d - d10[0]).max() <= 1e-12 * scale
    x = np.linalg.solve(A, b)
    ev = np.linalg.eigvalsh(np.sqrt(pre)[:, None] * A * np.sqrt(pre)[None, :])
    kappa = ev.max() / ev.min()
    K = 30
    rho = (np.sqrt(kappa) - 1) / (np.sqrt(kappa) + 1)
    bound = 2 * np.sqrt(kappa) * rho ** K + 1e-12
    assert bound < 1e-6                                  # (the bound says something)
    for f in sched:
        assert np.abs(f(A, b, pre, K) - x).max() <= bound * np.abs(x).max()


def _lm_problem(seed=9):
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((60, 37)) * (rng.uniform(0, 1, (60, 37)) < 0.2)
    J[:37] += np.diag(rng.uniform(0.5, 1.5, 37))
    return J, rng.standard_normal(60)


def _lm_loop_written_out(J, F, radius, L, period, q_tolerance, min_lm, max_lm):
    """tests/test_gpu_double.py, test_double_precision_levenberg_marquardt_against_float64: one LM step's PCG loop (first GN iteration: SSq is saved)"""
    f32 = lambda v: float(np.float32(v))
    r = -(J.T @ F); d = (J * J).sum(axis=0)
    SSq = 1.0 / (1.0 + np.sqrt(d)) ** 2
    unclamped = d / radius; cm = (1.0 / SSq) / radius
    CtC = np.minimum(np.maximum(unclamped, min_lm * cm), max_lm * cm)
    M = 1.0 / (CtC + radius * unclamped)
    b = r.copy(); z = M * r; aN = r @ z; delta = np.zeros_like(r); Q0 = 0.0; pvec = None; done = L
    for k in range(L):
        pvec = z.copy() if k == 0 else z + (bN / aN_prev) * pvec
        if k: aN = bN
        Ap = J.T @ (J @ pvec) + CtC * pvec; aD = pvec @ Ap
        alpha = aN / aD
        delta = delta + alpha * pvec
        if (k + 1) % period == 0: r = b - (J.T @ (J @ delta) + CtC * delta)
        else: r = r - alpha * Ap
        z = M * r; bN = z @ r; aN_prev = aN
        Q1 = 0.5 * delta @ (r + b)
        zeta = (k + 1) * (Q1 - Q0) / Q1
        if not np.isfinite(Q1) or not np.isfinite(zeta) or zeta < f32(q_tolerance): done = k + 1; break
        Q0 = Q1
    return delta, r, done, Q0


def _lm_loop_of_references(J, F, radius, L, period, q_tolerance, min_lm, max_lm):
    """the same loop from thallo_hip_lm_finalize_diagonal, pcg_pupdate (delta == NULL: the LM p update), lm_step1_finish, pcg_step2_full with b, lm_zeta and, every
    `period` iterations, lm_step2_first_half / second_half"""
    r = -(J.T @ F); d = (J * J).sum(axis=0)
    SSq, CtC, M, b, z, an = sk.ref_lm_finalize(d, None, r, radius, min_lm, max_lm, save_ssq=1, use_preconditioner=1)
    aN = an.sum(); delta = np.zeros_like(r); p = np.zeros_like(r); state = (0.0, 0, 0); beta = 0.0
    for k in range(L):
        if state[1]:
            break                                          # (the gate: later launches do nothing)
        p, _ = sk.ref_pupdate(z, p, None, 0.0, beta, first=(k == 0))
        Ap, adt = sk.ref_lm_step1_finish(J.T @ (J @ p), CtC, p)
        alpha = aN / adt.sum()
        if (k + 1) % period == 0:
            delta = sk.ref_lm_step2_first(delta, p, alpha)
            Ad, _ = sk.ref_lm_step1_finish(J.T @ (J @ delta), CtC, delta)
            r, z, bnt, qt = sk.ref_lm_step2_second(b, Ad, M, delta)
        else:
            delta, r, z, bnt, qt = sk.ref_step2_full(delta, p, r, Ap, M, b, alpha)
        bN = bnt.sum(); beta = bN / aN; aN = bN
        state = sk.ref_lm_zeta(state, qt.sum(), k, q_tolerance)
    return delta, r, state[2] if state[1] else L, state[0]


@pytest.mark.parametrize("q_tolerance", [0.0, 0.05])
def test_the_lm_chain_of_the_references_is_the_written_out_float64_loop(q_tolerance):
    """delta, r and Q0 to 1e-11 (relative to the largest entry), the same number of iterations; with q_tolerance = 0.05 the zeta test ends the loop early."""
    J, F = _lm_problem()
    f32 = lambda v: float(np.float32(v))
    args = (J, F, f32(30.0), 25, 10, q_tolerance, f32(1e-6), f32(1e32))
    d0, r0, done0, Q0 = _lm_loop_written_out(*args)
    d1, r1, done1, Q1 = _lm_loop_of_references(*args)
    assert done0 == done1 and (done0 < 25) == (q_tolerance > 0), (done0, done1)
    assert np.abs(d1 - d0).max() <= 1e-11 * np.abs(d0).max()
    assert np.abs(r1 - r0).max() <= 1e-11 * max(np.abs(r0).max(), np.abs(J.T @ F).max())
    assert abs(Q1 - Q0) <= 1e-11 * abs(Q0)


def test_lm_zeta_reference_cases():
    """continue; stop by tolerance; Q1 = 0 (0 / 0: a stop); Q1 = inf; already frozen"""
    assert sk.ref_lm_zeta((-1.0, 0, 0), -3.0, 2, 0.5) == (-3.0, 0, 0)             # zeta = 3 * (-2) / (-3) = 2
    assert sk.ref_lm_zeta((-2.0, 0, 0), -2.5, 1, 0.5) == (-2.0, 1, 2)             # zeta = 2 * (-0.5) / (-2.5) = 0.4 < 0.5
    assert sk.ref_lm_zeta((0.0, 0, 0), 0.0, 4, 0.0) == (0.0, 1, 5)
    assert sk.ref_lm_zeta((1.0, 0, 0), np.inf, 0, 0.0) == (1.0, 1, 1)
    assert sk.ref_lm_zeta((1.0, 1, 3), 5.0, 7, 0.0) == (1.0, 1, 3)


def test_float32_scalar_helpers():
    """the documented order against an independent evaluation on data where every order gives the same float; the guards; the (hi, lo) words; flat_grid's cap"""
    rng = np.random.default_rng(0)
    for nb in (1, 5, 64, 65, 1024):
        part = rng.integers(-100, 101, nb).astype(np.float32)
        assert float(sk.sum_partials(part)) == float(part.astype(np.float64).sum()) == sk.sum_partials_f64(part)
    assert sk.sum_partials(np.array([-0.0], np.float32)).tobytes() == np.float32(-0.0).tobytes()
    assert sk.div32(3, 0, True) == 0 and np.isinf(sk.div32(3, 0, False)) and np.isnan(sk.div32(0, 0, False)) and sk.div32(3, 4, True) == np.float32(0.75)
    for x in (-1.5, 5e-324, 1e300, 0.1):
        hi, lo = sk.hi_lo_words(x)
        assert sk.from_hi_lo(hi, lo) == x
    assert sk.flat_grid(1, 256) == 1 and sk.flat_grid(256 * 31, 256) == 31 and sk.flat_grid(10 ** 9, 256) == 1024 and sk.flat_grid(10 ** 9, 30) == 120
    assert sk.flat_grid(10 ** 9, 1) == 4 and sk.flat_grid(10 ** 9, 3) == 8 and sk.flat_grid(0, 256) == 1
    assert sk.ulp_apart(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1 and sk.ulp_apart(np.float32(0.0), np.float32(-0.0)) == 0
