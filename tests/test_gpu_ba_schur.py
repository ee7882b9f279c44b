"""The opt-in Schur-complement solve of bundle adjustment (csrc/ba_schur.hip, ThalloX_PlanSetLinearSolver): its kernels against float64, then Levenberg-Marquardt and
Gauss-Newton through the C ABI against the CPU restatement (tests/ba_schur_mirror.py), the default path's bits, the renumbered plan and the refusals.

Kernel instances: (5, 72, 330, band 5) -- cameras with 61 - 70 observations, on both sides of a wave's 64 lanes, points with 4 or 5, on both sides of the point kernel's
four-per-trip loop -- and (3, 160, 480, band 3): three lane rounds per camera, three observations per point.  Each gets one camera and one point that nothing observes and one
point observed exactly once (ba_schur_mirror.with_extras), in the caller's point order and in the plan's renumbered order, with and without the LM shift.

The float64 side is dense S, g and the back-substitution from the device's own Jb (ba_schur_mirror.Schur64); the bar of each operation is 4 e32, e32 the distance from
float64 of the float32 restatement in the kernels' summation order (SchurKernels32), recomputed on every run; the measure is max |err| / max |value|.

Measured on an MI355X (multiples of e32; the tests print them before they assert; also in profiles/ba_schur/README.md): MEASURED below, part of this docstring."""
import ctypes as C
import os

import numpy as np
import pytest

import shim_kernels as sk
import thallo_amd
from shim_kernels import F32
from thallo_amd import api, synthetic as syn

from ba_schur_mirror import BaSchurMirror, Schur64, SchurKernels32, SchurLists, dense_j, rel_max, with_extras
from helpers import copy_params, set_ab, to_device, to_host

pytestmark = pytest.mark.gpu

MEASURED = """device error in multiples of e32 (reduce g / apply S x / back-substitute / consistency on the camera rows / on the point rows; the bar is 4):
  (5, 72, 330)   caller's order  no shift 0.81 / 1.05 / 1.00 / 0.79 / 0.90   LM shift 1.00 / 1.10 / 2.42 / 1.02 / 1.00
  (5, 72, 330)   renumbered      no shift 0.65 / 1.00 / 1.00 / 0.58 / 1.00   LM shift 1.00 / 1.10 / 2.42 / 1.06 / 1.00
  (3, 160, 480)  caller's order  no shift 0.84 / 1.94 / 1.89 / 0.90 / 1.00   LM shift 1.32 / 1.00 / 1.86 / 1.09 / 0.83
  (3, 160, 480)  renumbered      no shift 0.94 / 0.96 / 2.04 / 0.88 / 1.00   LM shift 1.00 / 0.59 / 1.86 / 0.65 / 0.80
e32: 6e-8 ... 2.8e-7 (g), 4e-8 ... 8e-8 (S x), 2e-7 ... 2.9e-7 (back, no shift), 3e-4 ... 3.8e-4 (back, LM shift: the point observed once, third scaled pivot ~1e-4).
Through the C ABI the device's iterations per step are the mirror's exactly: LM 5 x 150 3, 6, 7, 6, 8 and 2, 9, 9, 15, 17; block plan 52 and 69 in total."""

__doc__ += "\n\n" + MEASURED

KERNEL = [((5, 72, 330), 5), ((3, 160, 480), 3)]
TABLE = [((24, 300, 1200), 12), ((48, 1200, 5000), 16)]
LM = dict(nIterations=5, lIterations=150, q_tolerance=0.1, function_tolerance=0.0)
TAIL = 64                                   # canary words behind every device buffer of these tests


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    """the library through a handle of this module's own, with the argtypes of the entry points these tests call"""
    lib = C.CDLL(thallo_amd.lib()._name)
    S, vp, it, lg, fl = api.SumT, C.c_void_p, C.c_int, C.c_long, C.c_float
    sig = {
        "vector_elems": [lg],
        "ba_compute_j": [it] + [vp] * 9, "ba_point_order": [it, vp, vp, vp], "ba_pack_point_blocks": [it, vp, vp, vp, vp],
        "ba_pcg_init": [it, it] + [vp] * 15,
        "lm_finalize_diagonal": [vp] * 7 + [lg, fl, fl, fl, it, it, vp, vp],
        "ba_block_diag": [it, it] + [vp] * 6,
        "ba_schur_factor": [it, vp, vp, vp, vp, vp],
        "ba_schur_rhs": [it, it] + [vp] * 12,
        "ba_schur_apply": [it, it] + [vp] * 13,
        "ba_schur_back": [it, it] + [vp] * 9 + [S, S, vp, vp],
    }
    for name, args in sig.items():
        f = getattr(lib, "thallo_hip_" + name)
        f.argtypes = args
        f.restype = lg if name == "vector_elems" else it
    return lib


def dev(torch, a, dtype=F32):
    """the array, then TAIL canary words"""
    a = np.ascontiguousarray(a, dtype)
    h = np.concatenate([a.view(np.uint32).ravel(), np.full(TAIL, sk.CANARY, np.uint32)])
    return torch.from_numpy(h.view(np.int32)).cuda()


def host(t, n, dtype=F32):
    h = t.cpu().numpy().view(np.uint32)
    assert (h[-TAIL:] == sk.CANARY).all(), "the canary behind a buffer changed"
    return h[:n].view(dtype).copy()


class SchurDevice:
    """One instance (with its extras) on the device as BundleAdjustmentPlugin::prepare + pcg_init (+ PCGFinalizeDiagonal) + thallo_hip_ba_block_diag leave it, then the
    elimination factor with and without the LM shift; the float64 and float32 sides of both from the device's own Jb and b"""

    def __init__(self, torch, L, dims, band, renumber):
        p, d3 = with_extras(syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band))
        self.C, self.P, self.O = C_, P_, O_ = d3
        self.nc, self.n = 9 * C_, 9 * C_ + 3 * P_
        self.lists = ls = SchurLists(p[3], p[4], C_, P_, renumber)
        pts = p[1][ls.new2old]
        i32 = lambda a: dev(torch, a, np.int32)
        self.d = d = dict(cam_ptr=i32(ls.cam_ptr), cam_obs=i32(ls.cam_obs), q_cam=i32(ls.q_cam), q_pt=i32(ls.q_pt), pt_ptr=i32(ls.pt_ptr), pt_pos=i32(ls.pt_pos), q_ptk=i32(np.zeros(O_)),
                          cams=dev(torch, p[0]), pts=dev(torch, pts), obs=dev(torch, p[2]), Jb=dev(torch, np.zeros(24 * O_)), F=dev(torch, np.zeros(2 * O_)),
                          JP=dev(torch, np.zeros(6 * O_)))
        self.na = int(L.thallo_hip_vector_elems(self.n))
        for k in ("r", "pre", "z", "p", "delta", "diag", "SSq", "CtC", "pre_lm", "b", "z_lm"): d[k] = dev(torch, np.zeros(self.na))
        d["H"] = dev(torch, np.zeros(45 * C_ + 6 * P_)); d["part"] = sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
        P = self.ptr
        assert L.thallo_hip_ba_point_order(O_, P("pt_pos"), P("q_ptk"), None) == 0
        assert L.thallo_hip_ba_compute_j(O_, P("cams"), P("pts"), P("obs"), P("cam_obs"), P("q_cam"), P("q_pt"), P("Jb"), P("F"), None) == 0
        assert L.thallo_hip_ba_pack_point_blocks(O_, P("Jb"), P("q_ptk"), P("JP"), None) == 0
        assert L.thallo_hip_ba_pcg_init(C_, P_, P("cam_ptr"), P("q_pt"), P("pt_ptr"), P("pt_pos"), P("q_cam"), P("Jb"), P("F"), P("r"), P("pre"), P("z"), P("p"), P("delta"),
                                        P("diag"), P("part"), None) > 0
        assert L.thallo_hip_lm_finalize_diagonal(P("diag"), P("SSq"), P("CtC"), P("pre_lm"), P("r"), P("b"), P("z_lm"), self.n, 1e4, 1e-6, 1e32, 1, 1, P("part"), None) > 0
        assert L.thallo_hip_ba_block_diag(C_, P_, P("cam_ptr"), P("pt_ptr"), P("Jb"), P("JP"), P("H"), None) == 0
        torch.cuda.synchronize()
        self.Jb = host(d["Jb"], 24 * O_).reshape(O_, 24)
        self.b = self.vec("b")
        self.CtC = self.vec("CtC")
        self.J = dense_j(self.Jb.astype(np.float64), ls)
        self.sides = {}
        for shifted in (False, True):
            G, held = dev(torch, np.full(6 * P_, np.nan)), dev(torch, np.array([77], np.uint32), np.uint32)
            assert L.thallo_hip_ba_schur_factor(P_, P("H") + 4 * 45 * C_, P("CtC") + 4 * self.nc if shifted else None, G.data_ptr(), held.data_ptr(), None) == 0
            torch.cuda.synchronize()
            K = SchurKernels32(self.Jb, ls, self.CtC if shifted else None, self.b)
            Gh = host(G, 6 * P_).reshape(6, P_)
            held_dev = ~Gh.any(0)
            assert np.isfinite(Gh).all()
            assert int(host(held, 1, np.uint32)[0]) == int(K.held.sum()) == int(held_dev.sum()) and (held_dev == K.held).all()
            self.sides[shifted] = (G, K, Schur64(self.J, self.CtC if shifted else None, self.b, K.held, C_))

    def ptr(self, k):
        return self.d[k].data_ptr()

    def vec(self, k):
        return host(self.d[k], self.na)[:self.n]

    def lists_args(self):
        P = self.ptr
        return (self.C, self.P, P("cam_ptr"), P("pt_ptr"), P("pt_pos"), P("Jb"), P("JP"))


@pytest.fixture(scope="module")
def instances(torch, L):
    cache = {}

    def get(dims, band, renumber):
        key = (dims, band, renumber)
        if key not in cache: cache[key] = SchurDevice(torch, L, dims, band, renumber)
        return cache[key]
    return get


CASES = [(d, b, r, s) for d, b in KERNEL for r in (False, True) for s in (False, True)]


def _bar(name, what, got, e32):
    print("schur", name, what, "e32", e32, "device", got, "= %.2f e32" % (got / e32))
    assert e32 > 0 and got <= 4 * e32, (name, what, got, e32)


def _run_ops(torch, L, B, shifted, x):
    """the three operations on the device -> (y, g, r_out, S x, x . S x partials, their number, delta_p)"""
    G, K, R = B.sides[shifted]
    U = dev(torch, np.full(2 * B.O, np.nan)); y = dev(torch, np.full(3 * B.P, np.nan)); g = dev(torch, np.full(B.nc, np.nan)); r_out = dev(torch, np.full(B.nc, np.nan))
    assert L.thallo_hip_ba_schur_rhs(*B.lists_args(), G.data_ptr(), B.ptr("b"), y.data_ptr(), U.data_ptr(), g.data_ptr(), r_out.data_ptr(), None) == 0
    xd = dev(torch, x); Sx = dev(torch, np.full(B.nc, np.nan)); part = sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
    nb = L.thallo_hip_ba_schur_apply(*B.lists_args(), G.data_ptr(), xd.data_ptr(), B.ptr("CtC") if shifted else None, U.data_ptr(), Sx.data_ptr(), part.data_ptr(), None, None)
    delta = dev(torch, np.concatenate([x, np.full(3 * B.P, np.nan)]))
    none = api.SumT(None, 0)
    assert L.thallo_hip_ba_schur_back(*B.lists_args(), G.data_ptr(), B.ptr("b"), delta.data_ptr(), None, none, none, U.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert sk.same_bytes(host(xd, B.nc), x) and sk.same_bytes(host(delta, B.n)[:B.nc], x)
    host(U, 2 * B.O)
    return host(y, 3 * B.P), host(g, B.nc), host(r_out, B.nc), host(Sx, B.nc), part.cpu().numpy(), nb, host(delta, B.n)[B.nc:]


@pytest.mark.parametrize("dims,band,renumber,shifted", CASES)
def test_reduce_apply_and_back_substitute_against_float64(torch, L, instances, dims, band, renumber, shifted):
    """g, S x for a random camera vector x and delta_p = back(x) against the dense float64 forms from the device's own Jb and b, each within 4 e32.  Without the shift the point
    nothing observes and the point observed once are held (the restatement's count and places, checked where the factor is made): their delta_p is exactly 0.  The x . S x
    partials: one per camera workgroup, adding up to the float64 dot of the device's x and S x within the dot bar of tests/test_gpu_block_precond.py.  A second run: the same bits."""
    B = instances(dims, band, renumber)
    if not renumber and dims == KERNEL[0][0]:
        assert sorted(set(np.diff(B.lists.cam_ptr)[:-1])) [0] <= 64 < max(np.diff(B.lists.cam_ptr)) and {4, 5} <= set(np.diff(B.lists.pt_ptr))
    if dims == KERNEL[1][0]: assert list(np.diff(B.lists.cam_ptr)) == [161, 160, 160, 0]
    assert {0, 1} <= set(np.diff(B.lists.pt_ptr)) and np.diff(B.lists.cam_ptr)[-1] == 0
    G, K, R = B.sides[shifted]
    x = (np.random.default_rng([7, int(shifted)]).standard_normal(B.nc) * 1e-3).astype(F32)
    y, g, r_out, Sx, part, nb, dp = _run_ops(torch, L, B, shifted, x)
    name = (dims, "renumbered" if renumber else "caller's order", "shift" if shifted else "no shift")
    assert sk.same_bytes(g, r_out)
    _bar(name, "reduce", rel_max(g, R.g), rel_max(K.reduce(), R.g))
    _bar(name, "apply", rel_max(Sx, R.apply(x)), rel_max(K.apply(x), R.apply(x)))
    _bar(name, "back", rel_max(dp, R.back(x)), rel_max(K.back(x), R.back(x)))
    if not shifted:
        assert int(K.held.sum()) == 2 and K.held[np.diff(B.lists.pt_ptr) <= 1].all()
    assert not dp.reshape(-1, 3)[K.held].any() and not y.reshape(-1, 3)[K.held].any()
    grid = (B.C + 3) // 4
    assert nb == grid and sk.written_slots(part) == grid
    t = x.astype(np.float64) * Sx
    assert abs(part[:grid].astype(np.float64).sum() - t.sum()) <= 13 * sk.EPS * np.abs(t).sum()      # c + 1, c = 12: the product, one term per lane, six butterfly levels, four waves
    again = _run_ops(torch, L, B, shifted, x)
    for a, b in zip((y, g, r_out, Sx, part, dp), (again[0], again[1], again[2], again[3], again[4], again[6])): assert sk.same_bytes(a, b)


@pytest.mark.parametrize("dims,band,renumber,shifted", CASES)
def test_the_three_operations_are_consistent_on_the_oracles_matrix(torch, L, orc, instances, dims, band, renumber, shifted):
    """For a random delta_c the device's g, s = S delta_c and delta_p = back(delta_c) satisfy, in float64 on the oracle's A = J^T J (+ diag(CtC)) and the device's b:
    (A [delta_c; delta_p] - b)_p = 0 on the points that are not held, and (A [delta_c; delta_p] - b)_c = s - g.  Measure: max |err| / max |A delta| over the rows; bar: 4 times
    the same measure of the float32 restatement's g, s and delta_p.  Ties the three operations together: a sign, an ordering or a stale u that they could share with their
    references shows here."""
    B = instances(dims, band, renumber)
    G, K, R = B.sides[shifted]
    p, d3 = with_extras(syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band))
    rp, col, val, _ = orc.Problem(orc.BUNDLE_ADJUST, d3, p).csr()
    import scipy.sparse as sp
    Jo = sp.csr_matrix((val.astype(np.float64), col, rp), shape=(2 * B.O, B.n)).toarray()
    perm = np.concatenate([np.arange(B.nc), B.nc + (3 * B.lists.new2old[:, None] + np.arange(3)).ravel()])      # the plan's unknown order
    Jo = Jo[:, perm]
    A = Jo.T @ Jo + (np.diag(B.CtC.astype(np.float64)) if shifted else 0.0)
    x = (np.random.default_rng([9, int(shifted)]).standard_normal(B.nc) * 1e-3).astype(F32)
    y, g, r_out, Sx, part, nb, dp = _run_ops(torch, L, B, shifted, x)
    free = np.repeat(~K.held, 3)

    def residuals(g_, s_, dp_):
        full = np.concatenate([x.astype(np.float64), np.asarray(dp_, np.float64)])
        Ad = A @ full
        res = Ad - B.b.astype(np.float64)
        rc = res[:B.nc] - (np.asarray(s_, np.float64) - np.asarray(g_, np.float64))
        rp_ = res[B.nc:][free]
        return np.abs(rc).max() / np.abs(Ad[:B.nc]).max(), np.abs(rp_).max() / np.abs(Ad[B.nc:][free]).max()
    dev_c, dev_p = residuals(g, Sx, dp)
    e_c, e_p = residuals(K.reduce(), K.apply(x), K.back(x))
    name = (dims, "renumbered" if renumber else "caller's order", "shift" if shifted else "no shift")
    _bar(name, "consistency, camera rows", dev_c, e_c)
    _bar(name, "consistency, point rows", dev_p, e_p)


def test_a_set_gate_word_leaves_every_output_as_it_was(torch, L, instances):
    dims, band = KERNEL[0]
    B = instances(dims, band, False)
    G, K, R = B.sides[True]
    rng = np.random.default_rng(13)
    x = rng.standard_normal(B.nc).astype(F32)
    u0, s0 = rng.standard_normal(2 * B.O).astype(F32), rng.standard_normal(B.nc).astype(F32)
    for gated in (True, False):
        U, Sx, xd, part = dev(torch, u0), dev(torch, s0), dev(torch, x), sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
        gate = sk.dbuf(torch, np.array([1 if gated else 0, 0], np.uint32))
        nb = L.thallo_hip_ba_schur_apply(*B.lists_args(), G.data_ptr(), xd.data_ptr(), B.ptr("CtC"), U.data_ptr(), Sx.data_ptr(), part.data_ptr(), gate.data_ptr(), None)
        torch.cuda.synchronize()
        assert nb == (B.C + 3) // 4
        same = sk.same_bytes(host(U, 2 * B.O), u0) and sk.same_bytes(host(Sx, B.nc), s0) and sk.written_slots(part.cpu().numpy()) == 0
        assert same == gated and sk.same_bytes(host(xd, B.nc), x)


def test_back_substitution_folds_the_loops_last_delta_term(torch, L, instances):
    """p given: delta_c += alpha p with alpha = alphaN / alphaD from the partials (sk.sum_partials, sk.div32, one fma), bit for bit, and delta_p is back() of that delta_c"""
    dims, band = KERNEL[0]
    B = instances(dims, band, False)
    G, K, R = B.sides[False]
    rng = np.random.default_rng(17)
    dc, p = (rng.standard_normal(B.nc) * 1e-3).astype(F32), (rng.standard_normal(B.nc) * 1e-3).astype(F32)
    parts = [sk.rounded_sum(rng, 65, positive=True), sk.rounded_sum(rng, 5, positive=True)]
    aN, aD = (sk.dbuf(torch, np.asarray(v, F32)) for v in parts)
    alpha = np.float64(sk.div32(sk.sum_partials(parts[0]), sk.sum_partials(parts[1]), guard=True))
    want = (alpha * p.astype(np.float64) + dc.astype(np.float64)).astype(F32)          # one rounding: the fma
    delta, pd, U = dev(torch, np.concatenate([dc, np.full(3 * B.P, np.nan)])), dev(torch, p), dev(torch, np.zeros(2 * B.O))
    assert L.thallo_hip_ba_schur_back(*B.lists_args(), G.data_ptr(), B.ptr("b"), delta.data_ptr(), pd.data_ptr(), sk.sumt(aN), sk.sumt(aD), U.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = host(delta, B.n)
    assert sk.same_bytes(got[:B.nc], want)
    ref = R.back(want)
    _bar((dims, "last term"), "back", rel_max(got[B.nc:], ref), rel_max(K.back(want), ref))


# ------------------------------------------------------------------ through the C ABI
def run(dims, p, lm, solver=None, precond=None, back=False, **sp):
    """-> (costs, PCG iterations per step, held points after every step, fallbacks after every step, cameras, points, schedule name)"""
    d = to_device(copy_params(p))
    s = api.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), solverkind="levenberg_marquardt" if lm else "gauss_newton")
    if lm: s.enable_lm()
    if precond: s.set_preconditioner(precond)
    if solver: s.set_linear_solver(solver)
    if back: s.set_linear_solver("pcg")
    s.set_solver_parameters(**sp)
    params = s.make_params(d)
    s.init(params)
    costs, iters, held, fb = [s.current_cost()], [], [], []
    while s.step(params):
        costs.append(s.current_cost()); iters.append(len(s.alpha_beta_trace())); held.append(s.schur_held_points()); fb.append(s.preconditioner_fallbacks())
    name = s.schedule_name
    s.close()
    return np.array(costs), iters, held, fb, to_host(d[0]).copy(), to_host(d[1]).copy(), name


def rel(a, b):
    m = min(len(a), len(b))
    return np.abs(np.asarray(a[:m], np.float64) - np.asarray(b[:m], np.float64)) / np.abs(np.asarray(b[:m], np.float64))


@pytest.mark.parametrize("dims,band", TABLE)
def test_lm_schur_through_the_c_abi(torch, orc, dims, band):
    """LM 5 x 150 (q_tolerance 0.1, function_tolerance 0): costs per step the mirror's within max(1e-5, 3 err_jacobi), err_jacobi the default path's distance from the oracle's LM
    on the same instance; iterations per step the mirror's up to a summed difference of 2; fewer iterations in total than the block-Jacobi plan; a final cost <= the block
    plan's (1 + 1e-4); no held point and no fallback at any step."""
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    cm, im = BaSchurMirror(dims, p).lm_solve(5, 150, q_tolerance=0.1, function_tolerance=0.0)
    co, _ = orc.Problem(orc.BUNDLE_ADJUST, dims, copy_params(p)).solve(use_lm=1, **LM)
    cj, ij, hj, *_ = run(dims, p, True, **LM)
    cb, ib, *_ = run(dims, p, True, precond="block_jacobi", **LM)
    cs, is_, hs, fs, _, _, name = run(dims, p, True, solver="schur_pcg", **LM)
    err_j, err = rel(cj, co), rel(cs, cm)
    print("LM", dims, "schur", is_, list(cs), "mirror", im, cm, "block", ib, list(cb), "jacobi", ij, "err_jacobi", err_j.max(), "err", err.max())
    assert "Schur complement on the cameras; block-Jacobi on S" in name and hj == [-1] * len(hj)
    assert len(is_) == 5 and len(cs) == len(cm)
    assert err.max() <= max(1e-5, 3 * err_j.max())
    assert sum(abs(a - b) for a, b in zip(is_, im)) <= 2, (is_, im)
    assert sum(is_) < sum(ib), (is_, ib)
    assert cs[-1] <= cb[-1] * (1 + 1e-4)
    assert hs == [0] * 5 and fs == [0] * 5


@pytest.mark.parametrize("dims,band", TABLE)
def test_gn_schur_through_the_c_abi(torch, orc, dims, band):
    """GN 4 x 10: costs per step the mirror's within the LM test's self-calibrated bar, exactly 10 iterations per step; the cost after step 1 below the block plan's after its
    step 1; the final cost <= the block plan's (1 + 1e-5)."""
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    cm = BaSchurMirror(dims, p).gn_solve(4, 10)
    co, _ = orc.Problem(orc.BUNDLE_ADJUST, dims, copy_params(p)).solve(nIterations=4, lIterations=10)
    cj, *_ = run(dims, p, False, nIterations=4, lIterations=10)
    cb, *_ = run(dims, p, False, precond="block_jacobi", nIterations=4, lIterations=10)
    cs, is_, hs, fs, *_ = run(dims, p, False, solver="schur_pcg", nIterations=4, lIterations=10)
    err_j, err = rel(cj, co), rel(cs, cm)
    print("GN", dims, "schur 4x10", list(cs), "mirror", cm, "block 4x10", list(cb), "err_jacobi", err_j.max(), "err", err.max())
    assert len(cs) == 5 and is_ == [10] * 4 and hs == [0] * 4 and fs == [0] * 4
    assert err.max() <= max(1e-5, 3 * err_j.max())
    assert cs[1] < cb[1]
    assert cs[-1] <= cb[-1] * (1 + 1e-5)


@pytest.mark.parametrize("dims,band", KERNEL)
def test_held_points_keep_their_bits_through_a_gn_step(torch, dims, band):
    """the instance with its extras, one GN step of 10 iterations: the point nothing observes and the point observed once are held (the mirror's count), their rows of `points`
    are bit-unchanged, the other points move and the cost falls; the camera nothing observes has a zero block: one fallback"""
    p, d3 = with_extras(syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band))
    m = BaSchurMirror(d3, p); m.gn_step(10)
    for ren in ("0", "1"):
        with pytest.MonkeyPatch.context() as mp:
            set_ab(mp, ba_renumber=ren)
            cs, is_, hs, fs, cams, pts, name = run(d3, p, False, solver="schur_pcg", nIterations=1, lIterations=10)
        assert hs == m.held == [2] and fs == [1] and is_ == [10]
        assert pts[-2:].tobytes() == p[1][-2:].tobytes() and cams[-1].tobytes() == p[0][-1].tobytes()
        assert (pts[:-2] != p[1][:-2]).any() and cs[1] < cs[0]
        assert abs(cs[1] - float(m.cost())) <= 1e-4 * cs[1]


@pytest.mark.parametrize("lm", [False, True])
def test_schur_then_pcg_before_init_is_the_default_plan_bit_for_bit(torch, lm):
    dims, band = TABLE[0]
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    sp = dict(nIterations=3, lIterations=25, q_tolerance=0.02) if lm else dict(nIterations=3, lIterations=10)
    a = run(dims, p, lm, **sp)
    b = run(dims, p, lm, solver="schur_pcg", back=True, **sp)
    assert list(a[0]) == list(b[0]) and a[1] == b[1] and a[6] == b[6] and b[2] == [-1] * len(b[2])
    assert sk.same_bytes(a[4], b[4]) and sk.same_bytes(a[5], b[5])


def test_renumbered_plan_runs_the_same_schur_solve(torch, monkeypatch):
    """the plan-side point order (THALLO_AB=ba_renumber=1): everything works in the plan's internal ids -- the same iterations (summed difference <= 2), costs to 1e-5"""
    dims, band = TABLE[0]
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    set_ab(monkeypatch, ba_renumber="0")
    c0, i0, h0, f0, _, _, n0 = run(dims, p, True, solver="schur_pcg", **LM)
    set_ab(monkeypatch, ba_renumber="1")
    c1, i1, h1, f1, _, _, n1 = run(dims, p, True, solver="schur_pcg", **LM)
    assert "renumbered" in n1 and "renumbered" not in n0
    assert len(i0) == len(i1) and sum(abs(a - b) for a, b in zip(i0, i1)) <= 2 and h1 == [0] * len(h1) and f1 == [0] * len(f1)
    assert rel(c1, c0).max() <= 1e-5


def test_refusals_name_the_energy(torch, monkeypatch, tmp_path):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energies")
    cases = [((48, 32), thallo_amd.energy_file("image_warping"), False),              # another hand-written energy
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), False),          # a generated one
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), True)]           # doublePrecision = 1
    for dims, f, dbl in cases:
        s = api.ThalloSolver(dims, f, double_precision=dbl)
        assert s.schur_held_points() == -1
        assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 1) != 0
        assert s.energy_name and s.energy_name in api.last_error(), api.last_error()
        with pytest.raises(RuntimeError): s.set_linear_solver("schur_pcg")
        assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 0) == 0 and s.schur_held_points() == -1
        s.close()
    s = api.ThalloSolver((5, 72, 330), thallo_amd.energy_file("bundle_adjustment"), double_precision=True)
    assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 1) != 0 and "bundle_adjustment" in api.last_error() and "doublePrecision" in api.last_error()
    s.close()
    s = api.ThalloSolver((5, 72, 330), thallo_amd.energy_file("bundle_adjustment"))
    assert s.schur_held_points() == -1
    assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 7) != 0 and "bundle_adjustment" in api.last_error()
    with pytest.raises(ValueError): s.set_linear_solver("cholesky")
    s.set_linear_solver("schur_pcg")
    with pytest.raises(RuntimeError, match="bundle_adjustment"):          # a distributed plan: the linear solver first ...
        s.set_distributed(0, 1, 0, 0, device_exchange=False)
    s.close()
    s = api.ThalloSolver((8, 72, 330), thallo_amd.energy_file("bundle_adjustment"))      # ... and the distribution first (one rank's camera shard)
    s.set_distributed(0, 1, 0, 0, device_exchange=False)
    with pytest.raises(RuntimeError, match="bundle_adjustment"):
        s.set_linear_solver("schur_pcg")
    s.close()
    # a direct-solve plan (tests/test_gpu_frontend.py::test_direct_solve_is_opt_in_like_the_reference's)
    lines = "".join(f"r.{n}.J:set_materialize(true)\nr.{n}.JtJ:set_materialize(true)\n" for n in ("fit", "reg")) + "r:set_direct_solve(true)\n"
    f = tmp_path / "laplacian_direct.t"
    f.write_text(open(thallo_amd.energy_file("laplacian_graph")).read() + "\n" + lines)
    monkeypatch.setenv("THALLO_FRONTEND", "generate"); monkeypatch.setenv("THALLO_ENABLE_DIRECT_SOLVE", "1")
    s = api.ThalloSolver((256, 255), str(f))
    assert s.schedule_name == "dense direct solve"
    assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 1) != 0
    assert s.energy_name and s.energy_name in api.last_error() and "direct-solve" in api.last_error(), api.last_error()
    s.close()
