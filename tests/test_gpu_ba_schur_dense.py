"""Bundle adjustment's dense Cholesky Schur solve (csrc/ba_schur_dense.hip, ThalloX_PlanSetLinearSolver kind 3): the kernels through their exported symbols on random
symmetric positive definite matrices and on the device's own assembled S, then the C call -- one step, trajectories, compositions, the failed factor, the covariance
through the factor, unchanged plans, refusals and the budget.

Kernel bars are derived, not measured.  u = 2^-24, gamma_k = k u / (1 - k u), both sides evaluated in float64:
  factor    |T - L L^T| <= 2 gamma_{n+1} |L||L|^T componentwise                                    (Higham, Accuracy and Stability, theorem 10.3)
  sweeps    |B - L Y| <= 2 gamma_n |L||Y| and |Y - L^T X| <= 2 gamma_n |L^T||X| componentwise      (theorem 8.5)
They hold for any order of summation and for fused multiply-adds; the factor 2 covers a division or a square root that is not correctly rounded.  The expansion:
d within 2 u of S_ii^-1/2 (a square root and a division) and every stored entry equal to float32(float32(d_i S_ij) d_j) bit for bit.
Matrices: T = M^T M / n + I scaled to a unit diagonal, n = 1, 9, 31, 32, 33, 45, 64, 216, 288 and 2313.  The one grid cap of the kernels is the panel solve's
(32 workgroups of 64 rows: 2048 rows per pass); at n = 2313 the first panels have 2281 rows below them, so its workgroups stride.  The trailing update's grid grows with n
(19 x 19 tiles there), the sweeps' does not depend on n.

Through the C ABI a step and a covariance are held to 4 x the float32 LAPACK mirror's own error (tests/ba_schur_dense_mirror.py) on the same instance against the same
float64 reference, computed in the same run -- tests/test_gpu_ba_covariance.py's rule, for its reason: two correct float32 evaluations in different association orders;
costs per step to that mirror's within tests/test_gpu_ba_schur_explicit.py's bar max(1e-5, 3 err_jacobi).  Every figure is printed before it is asserted.

Measured on an MI355X (also in profiles/ba_schur_dense/README.md): largest multiples of the derived bounds 0.088 (factor, n = 33), 0.139 / 0.109 (panel sweeps, n = 9) and
0.147 (one-column sweeps, n = 9), falling to 0.0018 / 0.0015 / 0.0010 at n = 2313; d within 1.02 - 1.44 u; one GN step 0.41 - 1.26 x the mirror's error (1.2e-5 ... 4.8e-5),
kernels and C call alike, and the kernels' delta applied to the cameras gives the C call's bytes in all six cases; trajectories: largest cost difference from the mirror 1.0e-6
(err_jacobi 4.6e-7 ... 1.1e-6); the covariance 0.44 - 2.15 x the mirror's error under the squared loss and 0.95 - 3.63 under Huber -- THE LARGEST MULTIPLE IS 3.63
((5, 72, 330) with its extras, LM, Huber, cameras; mirror 4.4e-5); (200, 6000, 26000): 1.02 x the mirror's 2.9e-2."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import shim_kernels as sk
import test_gpu_block_precond as bp
import thallo_amd
from shim_kernels import EPS, F32
from thallo_amd import api, synthetic as syn

import ba_covariance_mirror as cm
import ba_schur_dense_mirror as dm
import test_gpu_ba_schur as base
from ba_block_mirror import BaBlockMirror
from ba_robust_mirror import robust
from ba_schur_dense_mirror import BaSchurDenseMirror
from ba_schur_mirror import with_extras
from helpers import copy_params, set_ab, to_device, to_host
from test_gpu_ba_covariance import CovDevice, InfoT, SysT, plan, problem
from test_gpu_ba_schur import dev, host, rel, run, torch      # noqa: F401  (torch: the module fixture)

pytestmark = pytest.mark.gpu

K = cm.K
NB = 32
NS = [1, 9, 31, 32, 33, 45, 64, 216, 288, 2313]
BOTH, FORWARD, BACKWARD = 0, 1, 2
SHAPES = [((5, 72, 330), 5, True), ((3, 160, 480), 3, True), ((24, 300, 1200), 12, False)]
GN = dict(nIterations=3, lIterations=10)
LM = dict(nIterations=3, lIterations=7, q_tolerance=0.1, function_tolerance=0.0)


def gamma(k): return k * EPS / (1 - k * EPS)


@pytest.fixture(scope="module")
def L(torch):
    lib = C.CDLL(thallo_amd.lib()._name)
    vp, it, lg, fl = C.c_void_p, C.c_int, C.c_long, C.c_float
    R, spt = bp.RegionsT, C.POINTER(SysT)
    sig = {
        "vector_elems": [lg],
        "ba_compute_j": [it] + [vp] * 9, "ba_point_order": [it, vp, vp, vp], "ba_pack_point_blocks": [it, vp, vp, vp, vp],
        "ba_pcg_init": [it, it] + [vp] * 15,
        "lm_finalize_diagonal": [vp] * 7 + [lg, fl, fl, fl, it, it, vp, vp],
        "ba_block_diag": [it, it] + [vp] * 6,
        "ba_schur_factor": [it, vp, vp, vp, vp, vp],
        "ba_schur_rhs": [it, it] + [vp] * 12,
        "block_factor": [R] + [vp] * 6, "block_hold": [R, vp, vp, vp], "block_hold_factor": [R, vp, vp, vp],
        "ba_schur_w": [it, it] + [vp] * 5,
        "ba_schur_assemble": [it, it, lg] + [vp] * 8,
        "ba_cov_work_bytes": [it],
        "ba_cov_rhs": [spt, it, vp, it, vp, vp],
        "ba_cov_out": [spt, it, vp, it, vp, vp, vp, vp],
        "dense_ld": [lg],
        "ba_schur_dense_expand": [it, lg, vp, vp, vp, vp, lg, vp, vp, vp, vp],
        "dense_potrf": [lg, lg, vp, vp, vp],
        "dense_potrs_cols": [lg, lg, vp, vp, vp, it, it, vp],
        "dense_potrs_vec": [lg, lg, vp, vp, vp, vp, it, vp],
    }
    for name, args in sig.items():
        f = getattr(lib, "thallo_hip_" + name)
        f.argtypes = args
        f.restype = lg if name in ("vector_elems", "ba_cov_work_bytes", "dense_ld") else it
    return lib


# ------------------------------------------------------------------ 1. factor and sweeps on random matrices
def spd(n, seed):
    """T = M^T M / n + I scaled to a unit diagonal -> float32 [n, n] (symmetric)"""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    A = M.T @ M / n + np.eye(n)
    s = 1.0 / np.sqrt(np.diag(A))
    T = (A * s[:, None] * s[None, :]).astype(F32)
    return np.tril(T) + np.tril(T, -1).T


def pack(T, ld):
    """the lower triangle in a [n, ld] buffer whose upper triangle and padding are the canary"""
    n = len(T)
    buf = np.full((n, ld), sk.CANARY, np.uint32)
    i, j = np.tril_indices(n)
    buf[i, j] = np.ascontiguousarray(T, F32).view(np.uint32)[i, j]
    return buf


def unpack(buf, n, ld):
    """-> the lower triangle as float32 [n, n] (zeros above); the canaries must be where they were"""
    buf = np.asarray(buf).view(np.uint32).reshape(n, ld)
    up = np.triu_indices(n, 1)
    assert (buf[up] == sk.CANARY).all() and (buf[:, n:] == sk.CANARY).all(), "the upper triangle or the padding changed"
    return np.tril(buf[:, :n].view(F32))


class Factor:
    """one n: the matrix, the device's factor of it (two runs), the info word -- computed once, shared, never changed"""

    def __init__(self, torch, L, n):
        self.n, self.ld = n, int(L.thallo_hip_dense_ld(n))
        assert self.ld % NB == 0 and n <= self.ld < n + NB
        self.T = spd(n, 100 + n)
        self.runs = []
        for _ in range(2):
            t, info = dev(torch, pack(self.T, self.ld), np.uint32), dev(torch, np.array([77], np.int32), np.int32)
            assert L.thallo_hip_dense_potrf(n, self.ld, t.data_ptr(), info.data_ptr(), None) == 0
            torch.cuda.synchronize()
            self.runs.append((t, int(host(info, 1, np.int32)[0])))
        self.Ld = self.runs[0][0]
        self.L = unpack(host(self.Ld, n * self.ld, np.uint32), n, self.ld)


@pytest.fixture(scope="module")
def factors(torch, L):
    cache = {}

    def get(n):
        if n not in cache: cache[n] = Factor(torch, L, n)
        return cache[n]
    return get


@pytest.mark.parametrize("n", NS)
def test_factor_within_highams_bound(torch, L, factors, n):
    """T = L L^T: |T - L L^T| <= 2 gamma_{n+1} |L||L|^T componentwise in float64; info 0; the upper triangle and the padding untouched; two runs the same bits"""
    Fz = factors(n)
    assert Fz.runs[0][1] == 0 and Fz.runs[1][1] == 0
    assert sk.same_bytes(host(Fz.runs[0][0], n * Fz.ld, np.uint32), host(Fz.runs[1][0], n * Fz.ld, np.uint32))
    L64 = Fz.L.astype(np.float64)
    assert np.isfinite(L64).all() and (np.diag(L64) > 0).all()
    res = np.abs(np.tril(Fz.T.astype(np.float64) - L64 @ L64.T))
    bound = 2 * gamma(n + 1) * (np.abs(L64) @ np.abs(L64).T)
    worst = float((res / bound)[np.tril_indices(n)].max())
    print("dense factor n", n, "largest multiple of 2 gamma_{n+1} |L||L|^T:", worst)
    assert worst <= 1.0


def _sweep_bounds(n, Lf, B, Y, X, what):
    L64, B, Y, X = (a.astype(np.float64) for a in (Lf, B, Y, X))
    aL = np.abs(L64)
    f = np.abs(B - L64 @ Y) / (2 * gamma(n) * (aL @ np.abs(Y)) + 1e-300)
    b = np.abs(Y - L64.T @ X) / (2 * gamma(n) * (aL.T @ np.abs(X)) + 1e-300)
    print("dense sweeps", what, "n", n, "largest multiples of 2 gamma_n |L||Y|: forward", float(f.max()), "backward", float(b.max()))
    assert f.max() <= 1.0 and b.max() <= 1.0


@pytest.mark.parametrize("n", NS)
def test_panel_sweeps_within_the_substitution_bound(torch, L, factors, n):
    """64 right-hand sides: each sweep alone within its bound, the two in a row the bits of the one-launch form, two runs the same bits; a column solved alone (the other 63
    zero) is the column of the full panel bit for bit and the unused columns stay zero; two panels in one launch are each panel alone; L untouched"""
    Fz = factors(n)
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, K)).astype(F32)
    lp = Fz.Ld.data_ptr()

    def sweep(b, mode, groups=1):
        x = dev(torch, b)
        assert L.thallo_hip_dense_potrs_cols(n, Fz.ld, lp, None, x.data_ptr(), groups, mode, None) == 0
        torch.cuda.synchronize()
        return host(x, b.size).reshape(b.shape)
    Y = sweep(B, FORWARD); X = sweep(Y, BACKWARD)
    _sweep_bounds(n, Fz.L, B, Y, X, "panel")
    X2 = sweep(B, BOTH)
    assert sk.same_bytes(X, X2) and sk.same_bytes(X2, sweep(B, BOTH))
    for k in (0, 37):
        B1 = np.zeros_like(B); B1[:, k] = B[:, k]
        X1 = sweep(B1, BOTH)
        assert sk.same_bytes(X1[:, k], X2[:, k]) and not np.delete(X1, k, 1).any()
    Bb = rng.standard_normal((n, K)).astype(F32)
    two = sweep(np.stack([B, Bb]), BOTH, groups=2)
    assert sk.same_bytes(two[0], X2) and sk.same_bytes(two[1], sweep(Bb, BOTH))
    assert sk.same_bytes(unpack(host(Fz.Ld, n * Fz.ld, np.uint32), n, Fz.ld), Fz.L)


@pytest.mark.parametrize("n", NS)
def test_one_column_sweeps_within_the_substitution_bound(torch, L, factors, n):
    """the one-right-hand-side form: each sweep within its bound, the two in a row the bits of the one-launch form, two runs the same bits; with d: D L^-T L^-1 D b, the
    scalings exact products around the same sweeps, zeros of d giving exact zeros"""
    Fz = factors(n)
    rng = np.random.default_rng(1000 + n)
    b = rng.standard_normal(n).astype(F32)
    lp = Fz.Ld.data_ptr()

    def sweep(v, mode, d=None):
        vd, x = dev(torch, v), dev(torch, np.full(n, np.nan))
        dd = None if d is None else dev(torch, d)
        assert L.thallo_hip_dense_potrs_vec(n, Fz.ld, lp, None if d is None else dd.data_ptr(), vd.data_ptr(), x.data_ptr(), mode, None) == 0
        torch.cuda.synchronize()
        return host(x, n)
    y = sweep(b, FORWARD); x = sweep(y, BACKWARD)
    _sweep_bounds(n, Fz.L, b[:, None], y[:, None], x[:, None], "one column")
    x2 = sweep(b, BOTH)
    assert sk.same_bytes(x, x2) and sk.same_bytes(x2, sweep(b, BOTH))
    d = rng.uniform(0.5, 2.0, n).astype(F32)
    xd = sweep(b, BOTH, d)
    assert sk.same_bytes(xd, (sweep((d * b).astype(F32), BOTH) * d).astype(F32))


@pytest.mark.parametrize("n,k", [(45, 5), (45, 40), (64, 33), (216, 215)])
def test_a_pivot_that_is_not_positive_sets_the_info_word_and_leaves_no_nan(torch, L, n, k):
    """T with T_kk = -1: the leading k x k block is positive definite, pivot k is not positive -- info = k + 1, the factor goes on with 1.0 there, nothing is NaN or inf"""
    T = spd(n, 7 + n + k)
    T[k, k] = -1.0
    ld = int(L.thallo_hip_dense_ld(n))
    t, info = dev(torch, pack(T, ld), np.uint32), dev(torch, np.array([77], np.int32), np.int32)
    assert L.thallo_hip_dense_potrf(n, ld, t.data_ptr(), info.data_ptr(), None) == 0
    torch.cuda.synchronize()
    Lf = unpack(host(t, n * ld, np.uint32), n, ld)
    assert int(host(info, 1, np.int32)[0]) == k + 1
    assert np.isfinite(Lf).all() and Lf[k, k] == 1.0
    L64 = Lf[:k, :k].astype(np.float64)
    assert (np.abs(np.tril(T[:k, :k].astype(np.float64) - L64 @ L64.T)) <= 2 * gamma(n + 1) * (np.abs(L64) @ np.abs(L64).T) + 1e-300).all()


def test_the_entry_points_refuse_bad_arguments(torch, L):
    t = dev(torch, np.zeros(64 * 64)); w = dev(torch, np.zeros(4), np.int32)
    assert L.thallo_hip_dense_ld(0) == -1 and L.thallo_hip_dense_ld(1) == 32 and L.thallo_hip_dense_ld(33) == 64
    assert L.thallo_hip_dense_potrf(40, 40, t.data_ptr(), w.data_ptr(), None) < 0                 # a leading dimension that is no multiple of the panel width
    assert L.thallo_hip_dense_potrf(40, 32, t.data_ptr(), w.data_ptr(), None) < 0
    assert L.thallo_hip_dense_potrf(0, 32, t.data_ptr(), w.data_ptr(), None) < 0
    assert L.thallo_hip_dense_potrs_cols(40, 64, t.data_ptr(), None, t.data_ptr(), 0, BOTH, None) < 0
    assert L.thallo_hip_dense_potrs_cols(40, 64, t.data_ptr(), None, t.data_ptr(), 1, 3, None) < 0
    assert L.thallo_hip_dense_potrs_vec(40, 64, t.data_ptr(), None, w.data_ptr(), w.data_ptr(), BOTH, None) < 0      # x == b


# ------------------------------------------------------------------ 2. the expansion, and the three kernels in a row, on the device's own S
@pytest.fixture(scope="module")
def instances(torch, L):
    cache = {}

    def get(dims, band, renumber):
        key = (dims, renumber)
        if key not in cache: cache[key] = CovDevice(torch, L, dims, band, renumber)
        return cache[key]
    return get


def expand(torch, L, A, masked):
    """-> (T float32 [n, ld] as stored, d, non-positive diagonals, the device buffers)"""
    n = 9 * A.C; ld = int(L.thallo_hip_dense_ld(n))
    t, d, w = dev(torch, np.full(n * ld, np.nan)), dev(torch, np.full(n, np.nan)), dev(torch, np.array([77, 78], np.uint32), np.uint32)
    P = lambda k: A.d[k].data_ptr()
    assert L.thallo_hip_ba_schur_dense_expand(A.C, A.st.nblk, P("row_ptr"), P("col"), P("S"), P("mask") if masked else None, ld, t.data_ptr(), d.data_ptr(), w.data_ptr(), None) == 0
    torch.cuda.synchronize()
    words = host(w, 2, np.uint32)
    assert int(words[1]) == 78
    return host(t, n * ld).reshape(n, ld), host(d, n), int(words[0]), (t, d, ld)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dims,band,renumber", [(d, b, r) for d, b, _ in SHAPES for r in (False, True)])
def test_the_expansion_against_float64_from_the_devices_own_s(torch, L, instances, dims, band, renumber, masked):
    """d = S_ii^-1/2 within 2 u, 0 at the held scalars and at the scalars whose diagonal is not positive (the nine of the camera nothing observes), which are counted; every stored entry of the lower triangle
    is float32(float32(d_i S_ij) d_j) bit for bit -- 0 where the cameras are not co-visible --, the dead scalars have the identity's rows and columns exactly; the upper
    triangle and the padding are the zeros of the clear"""
    A = instances(dims, band, renumber)
    n = 9 * A.C
    T, d, nonpos, _ = expand(torch, L, A, masked)
    S = A.S64.astype(F32)
    assert sk.same_bytes(S.astype(np.float64), A.S64)
    hold = A.mask[:n] if masked else np.zeros(n, bool)
    diag = S.diagonal()
    dead = hold | ~(diag > 0)
    # (this S was assembled under the gauge: a held scalar's diagonal is the identity's minus its coupling terms and may be negative -- counted when the expansion is
    #  not given the mask)
    assert nonpos == int((~hold & ~(diag > 0)).sum()) >= 9 and (nonpos == 9 or not masked) and not d[dead].any()
    ref = 1.0 / np.sqrt(diag[~dead].astype(np.float64))
    e = np.abs(d[~dead] - ref) / ref
    print("dense expansion", dims, renumber, masked, "d: largest relative error", float(e.max()), "=", float(e.max() / EPS), "u")
    assert e.max() <= 2 * EPS
    want = ((d[:, None] * S).astype(F32) * d[None, :]).astype(F32)
    want[dead, :] = 0; want[:, dead] = 0; want[dead, dead] = 1
    assert sk.same_bytes(np.tril(T[:, :n]), np.tril(want))
    assert not np.triu(T[:, :n], 1).any() and not T[:, n:].any()
    live = np.nonzero(~dead)[0]
    # (a unit diagonal: d carries at most 2 u, twice, and the two products a rounding each)
    assert (np.abs(T[live, live] - 1) <= 6.01 * EPS).all() and (np.tril(T[:, :n]) != 0).sum() > n


def device_g(torch, L, A):
    """g = b_c - E Cp^-1 b_p of the instance's GN step from the held elimination factor, on the device -> float32 [9 C]"""
    B = A.B
    y, U, g, r_out = (dev(torch, np.full(k, np.nan)) for k in (3 * B.P, 2 * B.O, B.nc, B.nc))
    assert L.thallo_hip_ba_schur_rhs(*B.lists_args(), A.d["Ge"].data_ptr(), B.ptr("b"), y.data_ptr(), U.data_ptr(), g.data_ptr(), r_out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return host(g, B.nc)


def kernels_delta(torch, L, A):
    """expand, factor, one-column solve on the instance's S and g -> (delta_c, info, g)"""
    n = 9 * A.C
    g = device_g(torch, L, A)
    _, d, _, (t, dd, ld) = expand(torch, L, A, True)
    info, gd, x = dev(torch, np.array([77], np.int32), np.int32), dev(torch, g), dev(torch, np.full(n, np.nan))
    assert L.thallo_hip_dense_potrf(n, ld, t.data_ptr(), info.data_ptr(), None) == 0
    assert L.thallo_hip_dense_potrs_vec(n, ld, t.data_ptr(), dd.data_ptr(), gd.data_ptr(), x.data_ptr(), BOTH, None) == 0
    torch.cuda.synchronize()
    return host(x, n), int(host(info, 1, np.int32)[0]), g


@pytest.mark.parametrize("renumber", [False, True])
@pytest.mark.parametrize("dims,band,extras", SHAPES)
def test_one_gn_step_against_float64_on_the_devices_own_s(torch, L, monkeypatch, instances, dims, band, extras, renumber):
    """delta_c of one GN step with the gauge held -- the three kernels in a row on the device's own S and g, and the C call (the cameras' change over the step) --
    against np.linalg.solve in float64 on S_FF of that S, within 4 x the float32 LAPACK mirror's own error on the same S and g, each in max |err| / max |delta|.  The
    C call's figure carries the rounding of x + delta, so its mirror does too.  delta is exactly 0 at the held scalars and at the camera nothing observes (every
    instance here carries its extras: the device's own S is tests/test_gpu_ba_covariance.py's CovDevice)"""
    A = instances(dims, band, renumber)
    n = 9 * A.C
    free = A.free_c
    dk, info, g = kernels_delta(torch, L, A)
    ref = np.zeros(n); ref[free] = np.linalg.solve(A.S64[np.ix_(free, free)], g.astype(np.float64)[free])
    Tm, dmir, nonpos = dm.expand32(A.S64.astype(F32), A.mask[:n])
    mir = dm.sweeps32(dm.factor32(Tm), dmir, g)
    top = np.abs(ref).max()
    e_mir, e_k = np.abs(mir - ref).max() / top, np.abs(dk - ref).max() / top
    name = (A.B.C, A.B.P, A.B.O, "renumbered" if renumber else "caller's order")
    print("dense step", name, "kernels: mirror error", e_mir, "device", e_k, "= %.2f x" % (e_k / e_mir))
    assert info == 0 and nonpos == 9 and not dk[~free].any() and not mir[~free].any()
    assert e_mir > 0 and e_k <= 4 * e_mir
    # the C call on the same instance
    p, d3 = with_extras(syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band))
    set_ab(monkeypatch, ba_renumber="1" if renumber else "0")
    s, params, d = plan(d3, p, False, None, cm.gauge_mask(d3[0], d3[1]), solver="schur_dense", nIterations=1, lIterations=10)
    assert s.step(params), api.last_error()
    assert s.schur_dense_nonpositive() == 9 and len(s.alpha_beta_trace()) == 0
    cams = to_host(d[0]).reshape(-1).copy()
    s.close()
    x0 = p[0].reshape(-1)
    step = cams.astype(np.float64) - x0
    step_mir = (x0 + mir).astype(F32).astype(np.float64) - x0
    e_c, e_cm = np.abs(step - ref).max() / top, np.abs(step_mir - ref).max() / top
    print("dense step", name, "C call: mirror error", e_cm, "device", e_c, "= %.2f x" % (e_c / e_cm), "| the kernels' delta applied gives the call's bits:", sk.same_bytes((x0 + dk).astype(F32), cams))
    assert sk.same_bytes(cams[~free], x0[~free]) and (cams[free] != x0[free]).any()
    assert e_cm > 0 and e_c <= 4 * e_cm


# ------------------------------------------------------------------ 3. through the C ABI
def dense_run(d3, p, lm, mask, loss=None, **sp):
    """-> (costs, linear iterations per step, cameras, points, schedule name, non-positive diagonals per step)"""
    s, params, d = plan(d3, p, lm, loss, mask, solver="schur_dense", **sp)
    costs, iters, nonpos = [s.current_cost()], [], []
    while s.step(params):
        costs.append(s.current_cost()); iters.append(len(s.alpha_beta_trace())); nonpos.append(s.schur_dense_nonpositive())
    name = s.schedule_name
    s.close()
    return np.array(costs), iters, to_host(d[0]).copy(), to_host(d[1]).copy(), name, nonpos


def err_jacobi(orc, d3, p, lm, sp):
    """the default plan's distance from the oracle's solve on the same instance: what two float32 evaluations of one trajectory differ by"""
    co, _ = orc.Problem(orc.BUNDLE_ADJUST, d3, copy_params(p)).solve(use_lm=1 if lm else 0, **sp)
    cj, *_ = run(d3, p, lm, **sp)
    return float(rel(cj, co).max())


@pytest.mark.parametrize("renumber", ["0", "1"])
@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("dims,band,extras", SHAPES)
def test_trajectories_through_the_c_abi(torch, orc, monkeypatch, dims, band, extras, lm, renumber):
    """GN 3 and LM 3 x 7 (lIterations is ignored) with the gauge held: costs per step the dense mirror's within max(1e-5, 3 err_jacobi); no linear iteration is reported;
    the held scalars keep their bits; the schedule name carries the kind and n"""
    p, d3 = problem(dims, band, extras)
    mask = cm.gauge_mask(d3[0], d3[1])
    sp_ = LM if lm else GN
    m = BaSchurDenseMirror(d3, p, mask)
    cmir = m.lm_solve(3, q_tolerance=0.1, function_tolerance=0.0)[0] if lm else m.gn_solve(3)
    ej = err_jacobi(orc, d3, p, lm, sp_)
    set_ab(monkeypatch, ba_renumber=renumber)
    cs, its, cams, pts, name, nonpos = dense_run(d3, p, lm, mask, **sp_)
    err = float(rel(cs, cmir).max())
    print("dense", "LM" if lm else "GN", d3, "renumbered" if renumber == "1" else "caller's order", list(cs), "mirror", cmir, "err_jacobi", ej, "err", err, name)
    assert m.pivot is None and len(cs) == len(cmir) == 4 and its == [0] * 3
    assert nonpos == m.nonpos == [9 if extras and not lm else 0] * 3      # (LM's diagonal makes the camera nothing observes a live scalar with g = 0: delta is 0 there all the same)
    assert err <= max(1e-5, 3 * ej)
    assert "assembled (" in name and "dense Cholesky of S (n = %d)" % (9 * d3[0]) in name and "block-Jacobi on S" not in name
    hold_c = mask[:9 * d3[0]]
    assert sk.same_bytes(cams.reshape(-1)[hold_c], p[0].reshape(-1)[hold_c]) and (cams.reshape(-1)[~hold_c][:9] != p[0].reshape(-1)[~hold_c][:9]).any()
    if extras: assert sk.same_bytes(cams[-1], p[0][-1]) and sk.same_bytes(pts[-2], p[1][-2])      # the camera and the point nothing observes


@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("what", ["huber", "intrinsics"])
def test_it_composes_with_a_robust_loss_and_with_held_intrinsics(torch, orc, what, lm):
    """(24, 300, 1200): Huber(2) with the gauge held, and every camera's intrinsics held (in GN next to the gauge): costs per step the dense mirror's under the same loss
    and mask, the held scalars' bits unchanged"""
    dims, band, _ = SHAPES[2]
    p, d3 = problem(dims, band, False)
    mask = cm.gauge_mask(d3[0], d3[1])
    if what == "intrinsics":
        if lm: mask[:] = False
        mask[:9 * d3[0]].reshape(-1, 9)[:, 6:9] = True
    loss = "huber" if what == "huber" else None
    sp_ = LM if lm else GN
    m = robust(BaSchurDenseMirror)(loss, 2.0, d3, p, mask) if loss else BaSchurDenseMirror(d3, p, mask)
    cmir = m.lm_solve(3, q_tolerance=0.1, function_tolerance=0.0)[0] if lm else m.gn_solve(3)
    ej = err_jacobi(orc, d3, p, lm, sp_)
    cs, its, cams, pts, name, nonpos = dense_run(d3, p, lm, mask, loss, **sp_)
    err = float(rel(cs, cmir).max())
    print("dense", what, "LM" if lm else "GN", list(cs), "mirror", cmir, "err_jacobi", ej, "err", err, name)
    assert m.pivot is None and len(cs) == len(cmir) == 4 and its == [0] * 3 and cs[-1] < cs[0]
    assert err <= max(1e-5, 3 * ej)
    hold_c = mask[:9 * d3[0]]
    assert sk.same_bytes(cams.reshape(-1)[hold_c], p[0].reshape(-1)[hold_c]) and "%d unknowns held" % int(mask.sum()) in name
    if loss: assert "huber loss, scale 2" in name


@pytest.mark.parametrize("dims,band,extras", SHAPES)
def test_gn_without_a_gauge_fails_the_step_and_names_the_pivot(torch, dims, band, extras):
    """the factor of the singular system meets a pivot that is not positive: the step returns 0, last_error() names a camera and a scalar and says what to do, the
    unknowns are byte-equal to before; the same plan under LM steps"""
    p, d3 = problem(dims, band, extras)
    s, params, d = plan(d3, p, False, None, None, solver="schur_dense", **GN)
    c0 = s.current_cost()
    assert not s.step(params)
    msg = api.last_error()
    print("dense GN without a gauge", d3, msg)
    mt = re.search(r"camera (\d+), scalar (\d+) \(index (\d+) of (\d+)\)", msg)
    assert mt and "bundle_adjustment" in msg and "pivot" in msg and "hold" in msg and "Levenberg-Marquardt" in msg
    cam, sc, idx, n = (int(x) for x in mt.groups())
    assert 0 <= cam < d3[0] and 0 <= sc < 9 and idx == 9 * cam + sc and n == 9 * d3[0]
    assert sk.same_bytes(to_host(d[0]), p[0]) and sk.same_bytes(to_host(d[1]), p[1]) and s.current_cost() == c0
    s.close()
    cs, its, *_ = dense_run(d3, p, True, None, **LM)
    assert len(cs) == 4 and cs[-1] < cs[0]


def cov_reference(m, mask, C_):
    """the float64 (A_FF)^-1 of a mirror's J, dense -> (Sigma, free)"""
    J, sys = dm.gn_system(m, mask)
    A = (J.T @ J).toarray()
    free = ~mask & ~cm.undetermined(A, C_)
    return cm.dense_cov64(A, free), free, sys


COV_CASES = [(d, b, e, lm, ren, None) for d, b, e in SHAPES for lm in (False, True) for ren in ("0", "1")] + [(d, b, e, True, "0", "huber") for d, b, e in SHAPES]


@pytest.mark.parametrize("dims,band,extras,lm,renumber,loss", COV_CASES)
def test_covariance_through_the_factor_against_float64(torch, monkeypatch, dims, band, extras, lm, renumber, loss):
    """after 3 steps of a kind-3 plan: camera and point blocks against the float64 (A_FF)^-1 of the oracle's J at the device's unknowns within 4 x the dense mirror's error
    against the same reference; held rows and columns exactly zero; with the extras the camera nothing observes is asked for too: its nine columns are the call's
    not_converged and its block stays zero, the two undetermined points are NaN blocks; nothing iterates; every block symmetric bit for bit.  GN and LM, both point
    orders; under Huber(2) on the LM plans in the caller's order"""
    p, d3 = problem(dims, band, extras)
    C_, P_, _ = d3
    mask = cm.gauge_mask(C_, P_)
    set_ab(monkeypatch, ba_renumber=renumber)
    s, params, d = plan(d3, p, lm, loss, mask, solver="schur_dense", **(LM if lm else GN))
    while s.step(params): pass
    cams = list(range(C_ if extras else 9))
    pts = list(range(0, P_ - 2, max(1, P_ // 25)))[:23] + ([P_ - 2, P_ - 1] if extras else [3, 4])
    out = s.covariance(params, cameras=cams, points=pts, rel_tol=float("nan"), max_iterations=-3)      # (accepted and ignored)
    nonpos = s.schur_dense_nonpositive()
    here = [to_host(d[0]).copy(), to_host(d[1]).copy()] + [a.copy() for a in p[2:]]
    s.close()
    m = (robust(BaBlockMirror)(loss, 2.0, d3, here) if loss else BaBlockMirror(d3, here))
    Sig, free, sys = cov_reference(m, mask, C_)
    cov = dm.DenseCovariance(sys, mask)
    name = (d3, "LM" if lm else "GN", "renumbered" if renumber == "1" else "caller's order", loss or "squared")
    for mode, ids, key, dd, off in ((0, cams, "cameras", 9, 0), (1, pts, "points", 3, 9 * C_)):
        got = out[key]
        Bm, im = cov.solve(mode, ids)
        ok = ~np.isnan(Bm[:, 0, 0])
        ref = cm.blocks_of(Sig, ids, dd, off)
        fr = free[off:off + dd * (C_ if mode == 0 else P_)].reshape(-1, dd)[ids]
        assert (np.isnan(got[:, 0, 0]) == ~ok).all() and np.isnan(got[~ok]).all() and int((~ok).sum()) == (2 if extras and mode else 0)
        e_dev, e_mir = cm.cov_error(got[ok], ref[ok], fr[ok]), cm.cov_error(Bm[ok], ref[ok], fr[ok])
        print("dense covariance", name, key, "mirror error", e_mir, "device", e_dev, "= %.2f x" % (e_dev / e_mir))
        assert sk.same_bytes(got[ok], np.transpose(got[ok], (0, 2, 1)))
        assert e_mir > 0 and e_dev <= 4 * e_mir, (name, key, e_dev, e_mir)
    info = out["info"]
    print("dense covariance", name, "info", info)
    assert not out["cameras"][0].any() and not out["cameras"][1][3].any() and out["cameras"][1][0, 0] > 0
    assert info["iterations"] == 0 and info["worst_residual"] == 0.0 and info["nan_blocks"] == (2 if extras else 0)
    assert info["not_converged"] == (9 if extras else 0) == nonpos
    assert info["columns"] == int(free[:9 * C_].reshape(-1, 9)[cams].sum()) + 3 * len(pts) - 3 * info["nan_blocks"]
    if extras: assert not out["cameras"][-1].any()


@pytest.mark.parametrize("lm", [False, True])
def test_the_covariance_call_leaves_the_solve_as_it_was(torch, lm):
    """step, covariance, step against step, step on a kind-3 plan: the same unknown bytes, costs and launch counts by name"""
    dims, band, _ = SHAPES[2]
    p, d3 = problem(dims, band, False)
    mask = cm.gauge_mask(d3[0], d3[1])
    sp_ = dict(LM, nIterations=4) if lm else dict(GN, nIterations=4)
    runs = []
    for call in (False, True):
        s, params, d = plan(d3, p, lm, None, mask, solver="schur_dense", **sp_)
        costs = [s.current_cost()]
        for k in range(4):
            assert s.step(params)
            costs.append(s.current_cost())
            if call and k in (0, 2):
                out = s.covariance(params, cameras=[1, 2], points=[0, 1, 2])
                assert np.isfinite(out["cameras"]).all() and out["info"]["not_converged"] == 0
        stats = {k: v["launches"] for k, v in s.kernel_stats().items() if v["launches"]}
        runs.append((costs, stats, to_host(d[0]).copy(), to_host(d[1]).copy()))
        s.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and {"SchurDenseExpand", "SchurDenseFactor", "SchurDenseSolve"} <= set(a[1])
    assert sk.same_bytes(a[2], b[2]) and sk.same_bytes(a[3], b[3]) and (a[2] != p[0]).any()


def test_a_chain_of_two_hundred_cameras_solves_every_column(torch):
    """(200, 6000, 26000), LM 3 steps, the gauge held: seven cameras' covariance returns 0 with all 63 columns solved and nothing iterated -- where the column PCG of
    kind 2 takes 344 iterations on the device and leaves columns open within its default 500 on the CPU mirror.  The error against the float64 Schur route (S assembled
    from the oracle's sparse J at the device's unknowns) is held to 4 x the dense mirror's against the same reference"""
    dims = (200, 6000, 26000)
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2])
    C_, P_, _ = dims
    nc = 9 * C_
    mask = cm.gauge_mask(C_, P_)
    s, params, d = plan(dims, p, True, None, mask, solver="schur_dense", nIterations=3, lIterations=5, q_tolerance=0.1, function_tolerance=0.0)
    while s.step(params): pass
    cams = list(range(2, 9))
    out = s.covariance(params, cameras=cams)
    here = [to_host(d[0]).copy(), to_host(d[1]).copy()] + [a.copy() for a in p[2:]]
    name = s.schedule_name
    s.close()
    assert out["info"] == dict(iterations=0, columns=63, not_converged=0, nan_blocks=0, worst_residual=0.0) and "n = 1800" in name
    m = BaBlockMirror(dims, here)
    J, sys = dm.gn_system(m, mask)
    J = sp.csc_matrix(J)
    Jc, Jp = sp.csr_matrix(J[:, :nc]), sp.csr_matrix(J[:, nc:])
    Hp = sp.bsr_matrix((Jp.T @ Jp).tocsr(), blocksize=(3, 3))      # (block diagonal: a residual sees one point)
    assert Hp.data.shape[0] == P_ and (Hp.indices == np.arange(P_)).all()
    Ci = sp.bsr_matrix((np.linalg.inv(Hp.data), Hp.indices, Hp.indptr), shape=Hp.shape)
    E = (Jc.T @ Jp).tocsr()
    S64 = (Jc.T @ Jc).toarray() - (E @ Ci @ E.T).toarray()
    free_c = ~mask[:nc]
    ref = cm.blocks_of(cm.inv_s_ff64(S64, free_c), cams, 9)
    Bm, im = dm.DenseCovariance(sys, mask).solve(0, cams)
    fr = free_c.reshape(-1, 9)[cams]
    e_dev, e_mir = cm.cov_error(out["cameras"], ref, fr), cm.cov_error(Bm, ref, fr)
    print("dense covariance", dims, "7 cameras: mirror error", e_mir, "device", e_dev, "= %.2f x" % (e_dev / e_mir))
    assert e_mir > 0 and e_dev <= 4 * e_mir


@pytest.mark.parametrize("lm", [False, True])
def test_dense_then_pcg_before_init_is_the_never_called_plan_bit_for_bit(torch, lm):
    dims, band, _ = SHAPES[2]
    p, d3 = problem(dims, band, False)
    sp_ = dict(nIterations=3, lIterations=25, q_tolerance=0.02) if lm else dict(nIterations=3, lIterations=10)
    a = run(d3, p, lm, **sp_)
    b = run(d3, p, lm, solver="schur_dense", back=True, **sp_)
    assert list(a[0]) == list(b[0]) and a[1] == b[1] and a[6] == b[6] and "dense" not in b[6]
    assert sk.same_bytes(a[4], b[4]) and sk.same_bytes(a[5], b[5])


def test_a_kind_2_plan_launches_what_it_launched(torch):
    """the kernel names of a kind-2 plan's steps and covariance call: none of the dense form's, and the set the assembled form has had"""
    dims, band, _ = SHAPES[2]
    p, d3 = problem(dims, band, False)
    s, params, d = plan(d3, p, True, None, cm.gauge_mask(d3[0], d3[1]), solver="schur_explicit_pcg", **LM)
    while s.step(params): pass
    s.covariance(params, cameras=[1])
    names = {k for k, v in s.kernel_stats().items() if v["launches"]}
    assert s.schur_dense_nonpositive() == -1 and "dense" not in s.schedule_name and "block-Jacobi on S" in s.schedule_name
    s.close()
    assert not any(k.startswith("SchurDense") for k in names)
    assert {"SchurW", "SchurAssemble", "SchurApplyS", "SchurFactor", "SchurReduce", "SchurBack", "BlockFactor", "BlockApply", "BlockStep2LM", "PCGStep3", "PCGZeta"} <= names


def test_a_reinit_with_another_kind_frees_and_switches(torch):
    """kind 3, Init, steps; kind 2, re-Init: the PCG loop runs again (iterations reported, no dense launches' getter); kind 3 again: the first solve's bits; kind 0: the
    getters answer -1"""
    dims, band, _ = SHAPES[2]
    p, d3 = problem(dims, band, False)
    mask = cm.gauge_mask(d3[0], d3[1])
    d = to_device(copy_params(p))
    s = api.ThalloSolver(d3, thallo_amd.energy_file("bundle_adjustment"))
    s.hold(0, mask[:9 * d3[0]])
    s.set_solver_parameters(nIterations=2, lIterations=10)
    params = s.make_params(d)
    costs = []
    for kind in ("schur_dense", "schur_explicit_pcg", "schur_dense", "pcg"):
        for t, a in zip(d[:2], p[:2]): t.copy_(torch.from_numpy(a.copy()))
        s.set_linear_solver(kind)
        s.init(params)
        assert s.ready(), api.last_error()
        dense = kind == "schur_dense"
        assert ("dense Cholesky" in s.schedule_name) == dense and (s.schur_blocks() > 0) == (kind != "pcg")
        iters = []
        while s.step(params): iters.append(len(s.alpha_beta_trace()))
        assert iters == ([0, 0] if dense else [10, 10])
        assert (s.schur_dense_nonpositive() == 0) if dense else (s.schur_dense_nonpositive() == -1)
        costs.append(s.current_cost())
    s.close()
    assert costs[0] == costs[2] and abs(costs[1] - costs[0]) <= 1e-2 * costs[0]


def test_refusals_name_the_energy(torch, monkeypatch, tmp_path):
    """kind 3 is refused exactly where kind 2 is, each by its message; an unknown kind; the covariance on a plan that ran neither kind names both"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energies")
    for dims, f, dbl, word in (((48, 32), thallo_amd.energy_file("image_warping"), False, "dense Cholesky"),
                               ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), False, "dense Cholesky"),
                               ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), True, "doublePrecision"),
                               ((5, 72, 330), thallo_amd.energy_file("bundle_adjustment"), True, "doublePrecision")):
        s = api.ThalloSolver(dims, f, double_precision=dbl)
        assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 3) != 0
        msg = api.last_error()
        assert s.energy_name and s.energy_name in msg and word in msg and ("dense Cholesky" in msg), msg
        with pytest.raises(RuntimeError): s.set_linear_solver("schur_dense")
        assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 0) == 0 and s.schur_dense_nonpositive() == -1
        s.close()
    s = api.ThalloSolver((5, 72, 330), thallo_amd.energy_file("bundle_adjustment"))
    assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 4) != 0 and "unknown linear solver kind 4" in api.last_error()
    with pytest.raises(ValueError): s.set_linear_solver("schur_dense_pcg")
    s.set_linear_solver("schur_dense")
    assert "dense Cholesky of S" in s.schedule_name
    with pytest.raises(RuntimeError, match="bundle_adjustment.*dense Cholesky"):      # a distributed plan: the linear solver first ...
        s.set_distributed(0, 1, 0, 0, device_exchange=False)
    s.close()
    s = api.ThalloSolver((8, 72, 330), thallo_amd.energy_file("bundle_adjustment"))      # ... and the distribution first
    s.set_distributed(0, 1, 0, 0, device_exchange=False)
    with pytest.raises(RuntimeError, match="bundle_adjustment.*dense Cholesky"):
        s.set_linear_solver("schur_dense")
    s.close()
    lines = "".join(f"r.{n}.J:set_materialize(true)\nr.{n}.JtJ:set_materialize(true)\n" for n in ("fit", "reg")) + "r:set_direct_solve(true)\n"
    f = tmp_path / "laplacian_direct.t"
    f.write_text(open(thallo_amd.energy_file("laplacian_graph")).read() + "\n" + lines)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("THALLO_FRONTEND", "generate"); mp.setenv("THALLO_ENABLE_DIRECT_SOLVE", "1")
        s = api.ThalloSolver((256, 255), str(f))
        assert s.schedule_name == "dense direct solve"
        assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 3) != 0
        assert s.energy_name in api.last_error() and "direct-solve" in api.last_error(), api.last_error()
        s.close()
    dims, band, _ = SHAPES[0]
    p, d3 = problem(dims, band, False)
    ids = np.array([0, 1], np.int32); out = np.zeros((2, 9, 9), np.float32)
    for solver in (None, "schur_pcg"):
        s, params, d = plan(d3, p, False, None, None, solver=solver, **GN)
        rc = s._L.ThalloX_PlanCovariance(s.plan, params, 0, ids.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p), None, None)
        msg = api.last_error()
        assert rc < 0 and "THALLOX_SOLVER_SCHUR_EXPLICIT_PCG" in msg and "THALLOX_SOLVER_SCHUR_DENSE" in msg and "ThalloX_PlanSetLinearSolver" in msg
        s.close()
    # the covariance of a kind-3 plan whose factor fails (GN, no gauge): negative, the step's message
    s, params, d = plan(d3, p, False, None, None, solver="schur_dense", **GN)
    rc = s._L.ThalloX_PlanCovariance(s.plan, params, 0, ids.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p), None, None)
    msg = api.last_error()
    assert rc < 0 and "covariance" in msg and re.search(r"camera \d+, scalar \d+", msg) and "hold" in msg, (rc, msg)
    s.close()


def test_a_dense_matrix_over_the_budget_fails_init_and_names_the_bytes(torch, monkeypatch):
    """THALLO_AB=schur_dense_max_mb=0: Init fails and names the bytes wanted (4 ld n + 4 n + 128) and allowed; with 1 MiB the small instance fits.  schur_s_max_mb = 0
    -- kind 2's key, whose count the dense bytes are added to -- refuses it as well"""
    dims, band, _ = SHAPES[0]
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    n = 9 * dims[0]; ld = (n + 31) // 32 * 32
    want = 4 * ld * n + 4 * n + 128
    for key, mb, ok in (("schur_dense_max_mb", "0", False), ("schur_dense_max_mb", "1", True)):
        set_ab(monkeypatch, **{key: mb})
        d = to_device(copy_params(p))
        s = api.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"))
        s.set_linear_solver("schur_dense")
        s.hold(0, cm.gauge_mask(dims[0], dims[1])[:n])
        s.set_solver_parameters(nIterations=1, lIterations=5)
        params = s.make_params(d)
        s.init(params)
        if ok:
            assert s.ready() and s.step(params) and s.schur_dense_nonpositive() == 0
        else:
            msg = api.last_error()
            print(msg)
            assert "wants %d bytes" % want in msg and "budget allows 0" in msg and "schur_dense_max_mb" in msg and "bundle_adjustment" in msg
            assert not s.ready() and not s.step(params) and s.schur_blocks() == -1
        s.close()
    set_ab(monkeypatch, schur_s_max_mb="0")
    d = to_device(copy_params(p))
    s = api.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"))
    s.set_linear_solver("schur_dense")
    s.init(s.make_params(d))
    msg = api.last_error()
    assert not s.ready() and "bytes" in msg and ("dense" in msg) and "budget allows 0" in msg, msg
    s.close()
