"""tests/ba_reference.py validated on the CPU before any kernel is compared with it: the dual-number Jacobian against difference quotients, the sparse operators against a
dense matrix, the index lists against a brute-force restatement, and the references chained into three PCG / LM iterations (the pattern of tests/test_shim_references.py).
No device, no library."""
import numpy as np
import pytest

import ba_reference as br
import shim_kernels as sk

def tiny(plan_order=False, seed=3, **kw):
    inc = br.incidence([3, 0, 4, 2, 5, 3], [2, 3, 1, 0, 4, 2, 5, 0], seed=seed, plan_order=plan_order)
    return inc, br.scene(inc, seed=seed, **kw)


H_STEP = 1e-4


@pytest.mark.parametrize("distortion", [1.0, 8.0])
def test_the_dual_number_jacobian_against_central_differences(distortion):
    """J against (F(x + h e_k) - F(x - h e_k)) / 2h of the float64 residual, h = 1e-4, the rotation branch held (a step of 1e-4 from |w| ~ 1e-4 or 0 would cross the cut;
    the reference's AD differentiates the branch taken).  Cameras 0..4 have |w|^2 = 2e-8, 2e-8, 0.5e-8, 0.5e-8, 0: both branches and no rotation; distortion 8: l1 ~ 0.4,
    l2 ~ 0.08 at r2 up to ~0.2.
    Bar per entry: 50 eps S / h + (h^2 / 6) T G.  First term: a residual is ~50 float64 operations on quantities bounded by S = |observed| + |predicted|, so each of the two
    evaluations is off by at most 50 eps S / 2 ... and their difference, divided by 2h, by 50 eps S / h = 2.2e-7 at S = 2e3.  Second term: the quotient's truncation error
    h^2 |F'''| / 6; G is the observation's largest |J| entry and T = 100 bounds |F'''| / G: at unit length scale (|X| <= 1.8, depth >= 3.7, |c| <= 0.5) every further
    derivative multiplies by a small constant over the depth, well below 100^(1/2).  At G ~ 1e3 the bar is ~2e-4, seven digits below the entry; a wrong partial is off
    by its own size."""
    inc, (cams, pts, obs) = tiny(distortion=distortion)
    cams, pts, obs = (a.astype(np.float64) for a in (cams, pts, obs))
    branch = br.check_rotation_branches(cams)
    assert list(branch[:5]) == [True, True, False, False, False] and branch[5]
    oc, op = inc.oToC, inc.oToP
    F, J = br.residual_and_jacobian(cams, pts, obs, oc, op)
    assert F.shape == (inc.O, 2) and J.shape == (inc.O, 2, 12)
    S = (np.abs(obs) + np.abs(obs - F))[:, :, None]
    G = np.abs(J).max(axis=(1, 2))[:, None, None]
    bar = 50 * np.finfo(np.float64).eps * S / H_STEP + H_STEP ** 2 / 6 * 100 * G
    fd = np.zeros_like(J)
    for k in range(12):
        out = []
        for s in (+1, -1):
            c2, p2 = cams.copy(), pts.copy()
            if k < 9: c2[:, k] += s * H_STEP
            else: p2[:, k - 9] += s * H_STEP
            out.append(br.residual_and_jacobian(c2, p2, obs, oc, op, branch=branch)[0])
        fd[:, :, k] = (out[0] - out[1]) / (2 * H_STEP)
    ratio = np.abs(J - fd) / bar
    print("largest |J - fd| / bar", ratio.max(), "largest bar / G", (bar / G).max())
    assert (ratio <= 1).all()
    assert (bar / G).max() < 1e-5                    # (the bar says something)
    assert (np.abs(J).max(axis=(0, 1)) > 0).all()     # no column is trivially zero


def test_the_float32_restatement_is_the_same_function_in_float32():
    inc, (cams, pts, obs) = tiny()
    F64, J64 = br.residual_and_jacobian(cams, pts, obs, inc.oToC, inc.oToP)
    F32, J32 = br.residual_and_jacobian(cams, pts, obs, inc.oToC, inc.oToP, dtype=np.float32)
    assert F32.dtype == np.float32 and J32.dtype == np.float32 and np.isfinite(J32).all()
    assert 0 < np.abs(J32 - J64).max() <= 1e-4 * np.abs(J64).max()
    assert np.abs(F32 - F64).max() <= 1e-5 * (np.abs(obs) + np.abs(obs - F64)).max()


def test_a_camera_near_the_branch_cut_is_refused():
    cams = np.zeros((2, 9)); cams[1, 0] = np.sqrt(1.005e-8)
    with pytest.raises(AssertionError):
        br.check_rotation_branches(cams)
    cams[1, 0] = np.sqrt(1.02e-8)
    assert list(br.check_rotation_branches(cams)) == [False, True]


def dense(Jb, inc):
    J = np.zeros((2 * inc.O, inc.n))
    b = np.asarray(Jb, np.float64).reshape(inc.O, 2, 12)
    for q in range(inc.O):
        for r in range(2):
            for k in range(9): J[2 * q + r, 9 * inc.q_cam[q] + k] += b[q, r, k]
            for k in range(3): J[2 * q + r, 9 * inc.C + 3 * inc.q_pt[q] + k] += b[q, r, 9 + k]
    return J


@pytest.mark.parametrize("plan_order", [False, True])
def test_the_sparse_operators_against_a_dense_matrix(plan_order):
    inc, _ = tiny(plan_order)
    rng = np.random.default_rng(1)
    Jb, F, p, ctc = rng.standard_normal((inc.O, 24)), rng.standard_normal((inc.O, 2)), rng.standard_normal(inc.n), rng.uniform(0.5, 2.0, inc.n)
    J = dense(Jb, inc)
    g, mag = br.jt_f(Jb, F, inc)
    assert np.allclose(g, J.T @ F.ravel(), rtol=0, atol=1e-13 * mag.max()) and np.allclose(mag, np.abs(J).T @ np.abs(F.ravel()), rtol=1e-13)
    assert np.allclose(br.jtj_diag(Jb, inc), (J * J).sum(axis=0), rtol=1e-13)
    for c in (None, ctc):
        Ap, M, cnt = br.apply(Jb, inc, p, c)
        want = J.T @ (J @ p) + (0 if c is None else c * p)
        wantM = np.abs(J).T @ (np.abs(J) @ np.abs(p)) + (0 if c is None else np.abs(c * p))
        assert np.abs(Ap - want).max() <= 1e-13 * M.max() and np.allclose(M, wantM, rtol=1e-13) and (np.abs(Ap) <= M * (1 + 1e-13)).all()
        assert list(cnt) == list(np.repeat([3, 0, 4, 2, 5, 3], 9)) + list(np.repeat(np.diff(inc.pt_ptr), 3))
    assert (br.apply(Jb, inc, p)[0][9:18] == 0).all()                     # the camera nothing observes


def check_lists(inc, cam_counts, pt_counts, plan_order):
    """the lists restated observation by observation"""
    O_ = inc.O
    assert list(np.diff(inc.cam_ptr)) == list(cam_counts)
    assert sorted(np.diff(inc.pt_ptr)) == sorted(pt_counts)
    if not plan_order: assert list(np.diff(inc.pt_ptr)) == list(pt_counts)
    assert sorted(inc.cam_obs) == list(range(O_)) and sorted(inc.pt_pos) == list(range(O_))
    assert not (np.diff(inc.oToC) >= 0).all()        # the caller's order is no camera order
    for c in range(inc.C):
        qs = range(inc.cam_ptr[c], inc.cam_ptr[c + 1])
        ids = [int(inc.cam_obs[q]) for q in qs]
        assert sorted(ids) == [o for o in range(O_) if inc.oToC[o] == c]
        key = [(int(inc.oToP[o]), o) for o in ids] if plan_order else ids
        assert key == sorted(key)
    for q in range(O_):
        assert inc.q_cam[q] == inc.oToC[inc.cam_obs[q]] and inc.q_pt[q] == inc.oToP[inc.cam_obs[q]]
    for j in range(inc.P):
        qs = [int(q) for q in inc.pt_pos[inc.pt_ptr[j]:inc.pt_ptr[j + 1]]]
        assert sorted(qs) == [q for q in range(O_) if inc.q_pt[q] == j]
        key = qs if plan_order else [int(inc.cam_obs[q]) for q in qs]
        assert key == sorted(key)
    if plan_order:
        first = [min([int(inc.q_cam[q]) for q in range(O_) if inc.q_pt[q] == j], default=inc.C) for j in range(inc.P)]
        assert first == sorted(first)
        assert sorted(inc.pt_new2old) == list(range(inc.P)) and list(np.diff(inc.pt_ptr)) == list(np.asarray(pt_counts)[inc.pt_new2old])


@pytest.mark.parametrize("plan_order", [False, True])
def test_the_index_lists_against_a_brute_force_restatement(plan_order):
    cc, pc = [3, 0, 4, 2, 5, 3], [2, 3, 1, 0, 4, 2, 5, 0]
    check_lists(br.incidence(cc, pc, seed=3, plan_order=plan_order), cc, pc, plan_order)
    pc = br.edge_pt_counts(sum(br.EDGE_CAMS))
    inc = br.incidence(br.EDGE_CAMS, pc, seed=1, plan_order=plan_order)
    check_lists(inc, br.EDGE_CAMS, pc, plan_order)
    assert set(np.diff(inc.pt_ptr)) >= {0, 1, 2, 3, 4, 5, 7, 8, 9} and np.diff(inc.pt_ptr)[-1] == 0 and inc.C % 4 != 0
    # a camera may see a point twice (incidence()'s docstring; EDGE must: 193 observations over 192 observed points): counted by hand here
    pairs = [(int(c), int(j)) for c, j in zip(inc.oToC, inc.oToP)]
    assert br.duplicate_pairs(inc) == len(pairs) - len(set(pairs)) and 0 < br.duplicate_pairs(inc) < inc.O // 10


def test_the_references_chained_into_three_pcg_iterations():
    """thallo_hip_ba_pcg_init, then three iterations of thallo_hip_pcg_update_lm + thallo_hip_ba_pcg_apply_lm as the header states them, from this module's references:
    r_0 = b = -J^T F, M^-1 = 1 / (CtC + diag), p_k = M^-1 r_k + beta_{k-1} p_{k-1}, A p_k = (J^T J + CtC) p_k, alpha_k = alphaN_k / alphaD_k,
    betaN_k = N - 2 alpha S1 + alpha^2 S2, q_{k+1} = 0.5 [U + alpha (T1 - T2) - alpha^2 alphaD].  Every iteration: betaN_k equals r_{k+1} . M^-1 r_{k+1} of the updated
    vectors, q_{k+1} equals 0.5 delta_{k+1} . (r_{k+1} + b), the recurred r equals b - A delta_{k+1} applied afresh, the model q falls (what CG guarantees) -- and on this
    instance the preconditioned residual norm r . M^-1 r falls too."""
    inc, (cams, pts, obs) = tiny()
    F, J = br.residual_and_jacobian(cams, pts, obs[inc.cam_obs], inc.q_cam, inc.q_pt)
    Jb = J.reshape(inc.O, 24)
    g, _ = br.jt_f(Jb, F, inc)
    b = -g
    diag = br.jtj_diag(Jb, inc)
    ctc = 1e-3 * diag + 1e-6
    pre = 1.0 / (ctc + diag)
    r, delta, p = b.copy(), np.zeros(inc.n), np.zeros(inc.n)
    aN = float(r @ (pre * r)); alpha = beta = 0.0; Ap = None; q = 0.0
    norms, qs = [aN], [q]
    for k in range(3):
        r, p, delta = sk.ref_pcg_update(r, Ap, pre, p, delta, alpha, beta, first=1 if k == 0 else 0)
        Ap, M, _ = br.apply(Jb, inc, p, ctc)
        aD = float(p @ Ap)
        N, S1, S2 = br.sums3(pre, r, Ap).sum(axis=0)
        U, T1, T2 = br.sumsq(delta, r, b, p, Ap).sum(axis=0)
        alpha = aN / aD
        bN, _ = sk.beta_n_f64(N, S1, S2, alpha)
        q, _ = br.lm_q1(U, T1, T2, alpha, aD)
        r1, d1 = r - alpha * Ap, delta + alpha * p
        assert abs(bN - r1 @ (pre * r1)) <= 1e-9 * N
        assert abs(q - 0.5 * d1 @ (r1 + b)) <= 1e-12 * abs(q)
        fresh = b - br.apply(Jb, inc, d1, ctc)[0]
        assert np.abs(fresh - r1).max() <= 1e-11 * np.abs(b).max()
        beta = bN / aN; aN = bN
        norms.append(bN); qs.append(q)
    print("r . M^-1 r", norms, "q", qs)
    assert all(b1 < a1 for a1, b1 in zip(norms, norms[1:]))
    assert all(b1 > a1 for a1, b1 in zip(qs, qs[1:]))          # q = 0.5 delta . (r + b) = b . delta - 0.5 delta . A delta: CG raises it monotonically
