"""The opt-in block-Jacobi preconditioner of bundle adjustment (csrc/block_precond.hip, ThalloX_PlanSetPreconditioner): its five kernels against float64, then
Levenberg-Marquardt and Gauss-Newton through the C ABI against the CPU restatement (tests/ba_block_mirror.py), the default path's bits, and the refusals.

Kernel instances: (5, 72, 330, band 5) -- its cameras see 65, 65, 70, 61 and 69 observations, on both sides of a wave's 64 lanes -- and (3, 160, 480, band 3): 160
observations per camera, three lane rounds (three cameras that see every point; 3 cameras cannot give the 4 observations per point that 120 points and 480
observations would need).  Each gets one camera and one point more that nothing observes.

Measured on an MI355X (scaled_error of the device's z against the float64 solve, next to the float32 restatement's e32; the bar is 4 e32; also in
profiles/block_jacobi/README.md; test_factor_and_apply_against_a_float64_solve prints both before it asserts):
  (5, 72, 330)   LM shift: e32 1.02e-5, device 9.60e-6 (0.94 e32)    no shift: e32 1.34e-5, device 1.79e-5 (1.34 e32)
  (3, 160, 480)  LM shift: e32 5.60e-6, device 8.04e-6 (1.43 e32)    no shift: e32 1.27e-5, device 1.15e-5 (0.91 e32)"""
import ctypes as C
import os

import numpy as np
import pytest

import shim_kernels as sk
import thallo_amd
from shim_kernels import EPS, F32
from thallo_amd import api, synthetic as syn

from ba_block_mirror import BaBlockMirror, e32_of, scaled_error
from helpers import copy_params, set_ab, to_device, to_host

pytestmark = pytest.mark.gpu

KERNEL = [((5, 72, 330), 5), ((3, 160, 480), 3)]
TABLE = [((24, 300, 1200), 12), ((48, 1200, 5000), 16)]
LM = dict(nIterations=5, lIterations=150, q_tolerance=0.1, function_tolerance=0.0)
TAIL = 64                                   # canary words behind every device buffer of these tests


class RegionT(C.Structure):                 # thallo_block_region_t
    _fields_ = [("offset", C.c_long), ("size", C.c_int), ("count", C.c_int)]


class RegionsT(C.Structure):                # thallo_block_regions_t
    _fields_ = [("r", RegionT * 4), ("n", C.c_int)]


def regions(C_, P_):
    R = RegionsT()
    R.r[0] = RegionT(0, 9, C_); R.r[1] = RegionT(9 * C_, 3, P_); R.r[2] = RegionT(0, 3, 0); R.r[3] = RegionT(0, 3, 0)
    R.n = 2
    return R


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


def load_shim():
    """the library through a handle of this module's own, with the argtypes of the entry points these tests call"""
    lib = C.CDLL(thallo_amd.lib()._name)
    S, vp, it, lg, fl = api.SumT, C.c_void_p, C.c_int, C.c_long, C.c_float
    sig = {
        "vector_elems": [lg],
        "ba_compute_j": [it] + [vp] * 9, "ba_point_order": [it, vp, vp, vp], "ba_pack_point_blocks": [it, vp, vp, vp, vp],
        "ba_pcg_init": [it, it] + [vp] * 15,
        "lm_finalize_diagonal": [vp] * 7 + [lg, fl, fl, fl, it, it, vp, vp],
        "block_floats": [RegionsT],
        "ba_block_diag": [it, it] + [vp] * 6,
        "block_factor": [RegionsT] + [vp] * 6,
        "block_apply": [RegionsT] + [vp] * 6,
        "block_step2": [RegionsT, vp, vp, vp, vp, S, S, vp, vp],
        "block_step2_lm": [RegionsT] + [vp] * 7 + [S, S, vp, vp, vp, vp],
    }
    for name, args in sig.items():
        f = getattr(lib, "thallo_hip_" + name)
        f.argtypes = args
        f.restype = lg if name in ("vector_elems", "block_floats") else it
    return lib


@pytest.fixture(scope="module")
def L(torch):
    return load_shim()


def dev(torch, a, dtype=F32):
    """the array, then TAIL canary words"""
    a = np.ascontiguousarray(a, dtype)
    h = np.concatenate([a.view(np.uint32).ravel(), np.full(TAIL, sk.CANARY, np.uint32)])
    return torch.from_numpy(h.view(np.int32)).cuda()


def host(t, n, dtype=F32):
    h = t.cpu().numpy().view(np.uint32)
    assert (h[-TAIL:] == sk.CANARY).all(), "the canary behind a buffer changed"
    return h[:n].view(dtype).copy()


def raw(t):
    return t.cpu().numpy().tobytes()


def unpack(Hflat, C_, P_):
    """the packed, block-strided lower triangles -> ([C, 9, 9], [P, 3, 3]) symmetric, float64"""
    out = []
    base = 0
    for n, cnt in ((9, C_), (3, P_)):
        M = np.zeros((cnt, n, n))
        k = 0
        for i in range(n):
            for j in range(i + 1):
                M[:, i, j] = M[:, j, i] = Hflat[base + k * cnt: base + (k + 1) * cnt]; k += 1
        out.append(M); base += n * (n + 1) // 2 * cnt
    return out


class BaDevice:
    """One instance on the device as BundleAdjustmentPlugin::prepare + pcg_init leave it (the index lists restated here, in the caller's point order or -- renumber --
    in the plan's: points by first observing camera, a camera's observations by internal point id), then thallo_hip_ba_block_diag."""

    def __init__(self, torch, L, dims, band, renumber=False):
        p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
        rng = np.random.default_rng(5)
        cams = np.concatenate([p[0], p[0][:1] + 0.01]).astype(F32); pts = np.concatenate([p[1], rng.standard_normal((1, 3))]).astype(F32)      # + one of each that nothing observes
        self.C, self.P, self.O = C_, P_, O_ = dims[0] + 1, dims[1] + 1, dims[2]
        self.n = n = 9 * C_ + 3 * P_
        oc, op = p[3].astype(np.int64), p[4].astype(np.int64)
        if renumber:
            first = np.full(P_, C_); np.minimum.at(first, op, oc)
            new2old = np.argsort(first, kind="stable"); old2new = np.empty(P_, np.int64); old2new[new2old] = np.arange(P_)
            op = old2new[op]; pts = pts[new2old]
        cp = np.concatenate([[0], np.cumsum(np.bincount(oc, minlength=C_))]); pp = np.concatenate([[0], np.cumsum(np.bincount(op, minlength=P_))])
        cobs = np.lexsort((np.arange(O_), op, oc)) if renumber else np.argsort(oc, kind="stable")
        pos = np.empty(O_, np.int64); pos[cobs] = np.arange(O_)
        qc, qp = oc[cobs], op[cobs]
        ppos = np.argsort(qp, kind="stable") if renumber else pos[np.argsort(op, kind="stable")]
        self.cam_ptr, self.pt_ptr, self.q_cam, self.q_pt, self.pt_pos = cp, pp, qc, qp, ppos
        i32 = lambda a: dev(torch, a, np.int32)
        self.d = d = dict(cam_ptr=i32(cp), cam_obs=i32(cobs), q_cam=i32(qc), q_pt=i32(qp), pt_ptr=i32(pp), pt_pos=i32(ppos), q_ptk=i32(np.zeros(O_)),
                          cams=dev(torch, cams), pts=dev(torch, pts), obs=dev(torch, p[2]), Jb=dev(torch, np.zeros(24 * O_)), F=dev(torch, np.zeros(2 * O_)),
                          JP=dev(torch, np.zeros(6 * O_)))
        self.na = int(L.thallo_hip_vector_elems(n))
        for k in ("r", "pre", "z", "p", "delta", "diag", "SSq", "CtC", "pre_lm", "b", "z_lm"): d[k] = dev(torch, np.zeros(self.na))
        self.R = regions(C_, P_)
        self.nf = int(L.thallo_hip_block_floats(self.R))
        assert self.nf == 45 * C_ + 6 * P_
        d["H"] = dev(torch, np.zeros(self.nf)); d["part"] = sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
        P = lambda k: d[k].data_ptr()
        assert L.thallo_hip_ba_point_order(O_, P("pt_pos"), P("q_ptk"), None) == 0
        assert L.thallo_hip_ba_compute_j(O_, P("cams"), P("pts"), P("obs"), P("cam_obs"), P("q_cam"), P("q_pt"), P("Jb"), P("F"), None) == 0
        assert L.thallo_hip_ba_pack_point_blocks(O_, P("Jb"), P("q_ptk"), P("JP"), None) == 0
        assert L.thallo_hip_ba_pcg_init(C_, P_, P("cam_ptr"), P("q_pt"), P("pt_ptr"), P("pt_pos"), P("q_cam"), P("Jb"), P("F"), P("r"), P("pre"), P("z"), P("p"), P("delta"),
                                        P("diag"), P("part"), None) > 0
        # the first LM step's CtC and M^-1 (thallo_hip_lm_finalize_diagonal at the default radius and clamps)
        assert L.thallo_hip_lm_finalize_diagonal(P("diag"), P("SSq"), P("CtC"), P("pre_lm"), P("r"), P("b"), P("z_lm"), n, 1e4, 1e-6, 1e32, 1, 1, P("part"), None) > 0
        assert L.thallo_hip_ba_block_diag(C_, P_, P("cam_ptr"), P("pt_ptr"), P("Jb"), P("JP"), P("H"), None) == 0
        torch.cuda.synchronize()
        self.H = host(d["H"], self.nf)
        self.Hs = unpack(self.H.astype(np.float64), C_, P_)

    def ptr(self, k):
        return self.d[k].data_ptr()

    def vec(self, k):
        return host(self.d[k], self.na)[:self.n]


@pytest.fixture(scope="module")
def instances(torch, L):
    cache = {}

    def get(dims, band, renumber=False):
        key = (dims, band, renumber)
        if key not in cache: cache[key] = BaDevice(torch, L, dims, band, renumber)
        return cache[key]
    return get


# ------------------------------------------------------------------ 1. block_diag
@pytest.mark.parametrize("dims,band,renumber", [(KERNEL[0][0], KERNEL[0][1], False), (KERNEL[1][0], KERNEL[1][1], False), (KERNEL[0][0], KERNEL[0][1], True)])
def test_block_diag_against_float64_of_the_devices_own_jb(torch, L, instances, dims, band, renumber):
    """H against J_c^T J_c formed in float64 from the device's own Jb.  Bar per entry: (2 n_obs + 2) 2^-24 sqrt(H_ii H_jj) -- 2 n_obs products (one rounding each, or none
    where contracted) and 2 n_obs additions in any order including the wave butterfly are bounded by (2 n_obs + 2) 2^-24 sum |a_i a_j|, and sum |a_i a_j| <= sqrt(H_ii H_jj)
    (Cauchy-Schwarz).  The diagonal entries equal thallo_hip_ba_pcg_init's diag_out to the same bar.  renumber: the index lists in the plan's own point order."""
    B = instances(dims, band, renumber)
    if not renumber and dims == KERNEL[0][0]: assert list(np.diff(B.cam_ptr)) == [65, 65, 70, 61, 69, 0]
    if dims == KERNEL[1][0]: assert list(np.diff(B.cam_ptr)) == [160, 160, 160, 0]
    assert B.pt_ptr[-1] - B.pt_ptr[-2] == 0 or renumber          # (renumbered: the unobserved point sorts last too -- its first camera is C)
    Jb = host(B.d["Jb"], 24 * B.O).astype(np.float64).reshape(B.O, 24)
    Jc = np.stack([Jb[:, 0:9], Jb[:, 12:21]], 1); Jp = np.stack([Jb[:, 9:12], Jb[:, 21:24]], 1)
    want_c = np.zeros((B.C, 9, 9)); np.add.at(want_c, B.q_cam, np.einsum("qri,qrj->qij", Jc, Jc))
    want_p = np.zeros((B.P, 3, 3)); np.add.at(want_p, B.q_pt, np.einsum("qri,qrj->qij", Jp, Jp))
    diag = B.vec("diag").astype(np.float64)
    for got, want, nobs, dg in ((B.Hs[0], want_c, np.diff(B.cam_ptr), diag[:9 * B.C].reshape(B.C, 9)), (B.Hs[1], want_p, np.diff(B.pt_ptr), diag[9 * B.C:].reshape(B.P, 3))):
        d = np.einsum("bii->bi", want)
        bar = (2 * nobs + 2)[:, None, None] * EPS * np.sqrt(d[:, :, None] * d[:, None, :])
        err = np.abs(got - want)
        print("block_diag", dims, renumber, got.shape, "largest err / bar", float((err / np.maximum(bar, 1e-300)).max()))
        assert (err <= bar).all()
        assert (np.abs(np.einsum("bii->bi", got) - dg) <= np.einsum("bii->bi", bar)).all()
    assert not B.Hs[0][-1].any() and (nobs[-1] == 0)               # the camera nothing observes: a zero block


# ------------------------------------------------------------------ 2. block_factor + block_apply
def _factor_apply(torch, L, B, shifted, r):
    G, z, st, part = dev(torch, np.zeros(B.nf)), dev(torch, np.full(B.na, np.nan)), dev(torch, np.array([77], np.uint32), np.uint32), sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
    assert L.thallo_hip_block_factor(B.R, B.ptr("H"), B.ptr("CtC") if shifted else None, B.ptr("pre_lm" if shifted else "pre"), G.data_ptr(), st.data_ptr(), None) == 0
    nb = L.thallo_hip_block_apply(B.R, G.data_ptr(), r.data_ptr(), z.data_ptr(), part.data_ptr(), None, None)
    torch.cuda.synchronize()
    return G, z, st, part, nb


@pytest.mark.parametrize("dims,band", KERNEL)
@pytest.mark.parametrize("shifted", [True, False])
def test_factor_and_apply_against_a_float64_solve(torch, L, instances, dims, band, shifted):
    """z = G^T (G r) against the float64 solve of (H + diag(shift)) z = r, H being what the factorisation was handed (the device's float32 blocks).  Measure: scaled_error
    (tests/ba_block_mirror.py); bar: 4 e32, e32 the same measure of the float32 restatement of the algorithm -- the margin covers another operation order and fma
    contraction.  Without the shift the unobserved camera and point have B = 0: two fallbacks, z = pre . r there (to 4 2^-24: sqrt(pre) twice rounded, two products);
    with the LM shift none.  The r . z partials add up to the float64 dot of the device's own r and z within (c + 1) 2^-24 sum |r z|, c = the chain of float additions
    behind a partial: 9 in a block + 1 per block a lane visits, 6 butterfly levels, 4 waves (the bar of tests/test_gpu_pcg_chain.py's dot tests).  A second launch: the same bits."""
    B = instances(dims, band)
    rng = np.random.default_rng(11)
    r = B.vec("r").copy()
    r[9 * (B.C - 1): 9 * B.C] = rng.standard_normal(9); r[-3:] = rng.standard_normal(3)          # something to precondition in the unobserved blocks
    rd = dev(torch, np.concatenate([r, np.zeros(B.na - B.n)]))
    G, z, st, part, nb = _factor_apply(torch, L, B, shifted, rd)
    shift = B.vec("CtC") if shifted else None
    pre = B.vec("pre_lm" if shifted else "pre")
    e32, z64 = e32_of(B.Hs, shift, pre, r, B.C)
    zd = host(z, B.na)[:B.n]
    got = scaled_error(zd, z64, B.Hs, shift, B.C)
    print("factor+apply", dims, "shift" if shifted else "no shift", "e32", e32, "device", got)
    assert np.isfinite(zd).all() and np.isnan(host(z, B.na)[B.n:]).all()
    assert got <= 4 * e32
    fb = int(host(st, 1, np.uint32)[0])
    if shifted: assert fb == 0
    else:
        assert fb == 2
        for sl in (slice(9 * (B.C - 1), 9 * B.C), slice(B.n - 3, B.n)):
            want = pre[sl].astype(np.float64) * r[sl]
            assert (np.abs(zd[sl] - want) <= 4 * EPS * np.abs(want)).all()
    total = B.C + B.P
    grid = (total + 255) // 256
    assert nb == grid and sk.written_slots(part.cpu().numpy()) == grid
    terms = r.astype(np.float64) * zd
    c = 10 * ((total + 256 * grid - 1) // (256 * grid)) + 6 + 4
    assert abs(part.cpu().numpy()[:grid].astype(np.float64).sum() - terms.sum()) <= (c + 1) * EPS * np.abs(terms).sum()
    G2, z2, st2, part2, _ = _factor_apply(torch, L, B, shifted, rd)
    assert raw(G) == raw(G2) and raw(z) == raw(z2) and raw(st) == raw(st2) and raw(part) == raw(part2)


# ------------------------------------------------------------------ 3. block_step2, block_step2_lm
def _apply64(G, x, C_, P_):
    """G^T (G x) and |G|^T (|G| |x|) in float64 from the packed device G"""
    Gs = unpack(G.astype(np.float64), C_, P_)
    out, mag = np.empty(len(x)), np.empty(len(x))
    lo = 0
    for M, n in zip(Gs, (9, 3)):
        Lw = np.tril(M)
        xb = x[lo:lo + n * len(M)].reshape(-1, n)
        out[lo:lo + n * len(M)] = np.einsum("bij,bi->bj", Lw, np.einsum("bij,bj->bi", Lw, xb)).ravel()
        mag[lo:lo + n * len(M)] = np.einsum("bij,bi->bj", np.abs(Lw), np.einsum("bij,bj->bi", np.abs(Lw), np.abs(xb))).ravel()
        lo += n * len(M)
    return out, mag


@pytest.mark.parametrize("lm", [False, True])
def test_block_step2_against_float64(torch, L, instances, lm):
    """One launch on random r, A p (and p, delta, b), as tests/test_gpu_pcg_chain.py checks pcg_step2_full: alpha bit-exactly from sk.sum_partials / sk.div32;
    r -= alpha A p and delta += alpha p within 2 2^-24 (|x| + |alpha y|) (product, sum); z against the float64 G^T (G r) of the device's own G and r within
    2 n 2^-24 |G|^T (|G| |r|), n the block size (y = G r: n products and n - 1 additions per entry; G^T y the same again on top of y's error); the betaN partials against
    the float64 dot of the device's z and r, the q partials against 0.5 delta . (r + b) with one rounding more per term, both within the dot bar (c as in the apply test).
    With the gate word set (LM) nothing is written."""
    dims, band = KERNEL[0]
    B = instances(dims, band)
    rng = np.random.default_rng([3, int(lm)])
    G = dev(torch, np.zeros(B.nf)); st = dev(torch, np.zeros(1, np.uint32), np.uint32)
    assert L.thallo_hip_block_factor(B.R, B.ptr("H"), B.ptr("CtC"), B.ptr("pre_lm"), G.data_ptr(), st.data_ptr(), None) == 0
    torch.cuda.synchronize()
    Gh = host(G, B.nf)
    scale = np.abs(B.vec("r")).max()
    h = {k: (rng.standard_normal(B.n) * scale).astype(F32) for k in ("r", "Ap", "p", "delta", "b")}
    parts = [sk.rounded_sum(rng, 65, positive=True), sk.rounded_sum(rng, 5, positive=True)]
    aN, aD = (sk.dbuf(torch, np.asarray(x, F32)) for x in parts)
    alpha = float(sk.div32(sk.sum_partials(parts[0]), sk.sum_partials(parts[1]), guard=not lm))
    total = B.C + B.P; grid = (total + 255) // 256
    c = 10 * ((total + 256 * grid - 1) // (256 * grid)) + 6 + 4
    for gated in ([False, True] if lm else [False]):
        d = {k: dev(torch, v) for k, v in h.items()}
        z = dev(torch, np.full(B.n, np.nan))
        pb, qb = sk.canary_buf(torch, sk.MAX_PARTIALS + 8), sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
        gate = sk.dbuf(torch, np.array([1 if gated else 0, 0], np.uint32))
        P = lambda k: d[k].data_ptr()
        if lm: ret = L.thallo_hip_block_step2_lm(B.R, G.data_ptr(), P("delta"), P("p"), P("r"), P("Ap"), z.data_ptr(), P("b"), sk.sumt(aN), sk.sumt(aD), pb.data_ptr(), qb.data_ptr(),
                                                 gate.data_ptr(), None)
        else: ret = L.thallo_hip_block_step2(B.R, G.data_ptr(), P("r"), P("Ap"), z.data_ptr(), sk.sumt(aN), sk.sumt(aD), pb.data_ptr(), None)
        torch.cuda.synchronize()
        assert ret == grid
        got = {k: host(d[k], B.n) for k in h}
        zd = host(z, B.n)
        if gated:
            assert all(sk.same_bytes(got[k], h[k]) for k in h) and np.isnan(zd).all()
            assert sk.written_slots(pb.cpu().numpy()) == 0 and sk.written_slots(qb.cpu().numpy()) == 0
            continue
        for k in ("Ap", "p", "b") + (() if lm else ("delta",)): assert sk.same_bytes(got[k], h[k]), k
        f = {k: v.astype(np.float64) for k, v in h.items()}
        assert (np.abs(got["r"] - (f["r"] - alpha * f["Ap"])) <= 2 * EPS * (np.abs(f["r"]) + np.abs(alpha * f["Ap"]))).all()
        if lm: assert (np.abs(got["delta"] - (f["delta"] + alpha * f["p"])) <= 2 * EPS * (np.abs(f["delta"]) + np.abs(alpha * f["p"]))).all()
        rd = got["r"].astype(np.float64)
        z64, mag = _apply64(Gh, rd, B.C, B.P)
        nblk = np.concatenate([np.full(9 * B.C, 9), np.full(3 * B.P, 3)])
        assert (np.abs(zd - z64) <= 2 * nblk * EPS * mag).all()
        t = zd.astype(np.float64) * rd
        assert sk.written_slots(pb.cpu().numpy()) == grid
        assert abs(pb.cpu().numpy()[:grid].astype(np.float64).sum() - t.sum()) <= (c + 1) * EPS * np.abs(t).sum()
        if lm:
            tq = 0.5 * got["delta"].astype(np.float64) * (rd + f["b"])
            assert sk.written_slots(qb.cpu().numpy()) == grid
            assert abs(qb.cpu().numpy()[:grid].astype(np.float64).sum() - tq.sum()) <= (c + 2) * EPS * np.abs(tq).sum()


# ------------------------------------------------------------------ 4 - 7. through the C ABI
def run(dims, p, lm, precond=None, back=False, **sp):
    """-> (costs, PCG iterations per step, fallbacks after every step, cameras, points, schedule name)"""
    d = to_device(copy_params(p))
    s = api.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), solverkind="levenberg_marquardt" if lm else "gauss_newton")
    if lm: s.enable_lm()
    if precond: s.set_preconditioner(precond)
    if back: s.set_preconditioner("jacobi")
    s.set_solver_parameters(**sp)
    params = s.make_params(d)
    s.init(params)
    costs, iters, fb = [s.current_cost()], [], []
    while s.step(params):
        costs.append(s.current_cost()); iters.append(len(s.alpha_beta_trace())); fb.append(s.preconditioner_fallbacks())
    name = s.schedule_name
    s.close()
    return np.array(costs), iters, fb, to_host(d[0]).copy(), to_host(d[1]).copy(), name


def rel(a, b):
    m = min(len(a), len(b))
    return np.abs(np.asarray(a[:m], np.float64) - np.asarray(b[:m], np.float64)) / np.abs(np.asarray(b[:m], np.float64))


@pytest.mark.parametrize("dims,band", TABLE)
def test_lm_block_through_the_c_abi(torch, orc, dims, band):
    """LM 5 x 150 (q_tolerance 0.1, function_tolerance 0): the block form needs at most half the device's own Jacobi iterations, ends at most 1e-4 above its cost, falls back
    nowhere; its iterations per step are the mirror's up to a summed difference of 2 (the existing Jacobi-against-oracle bar is 1 over four steps), its costs per step the
    mirror's within max(1e-5, 3 err_jacobi), err_jacobi being the default path's distance from the oracle's LM on the same instance."""
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    cm, im = BaBlockMirror(dims, p).lm_solve(5, 150, kind="block32", q_tolerance=0.1, function_tolerance=0.0)
    co, _ = orc.Problem(orc.BUNDLE_ADJUST, dims, copy_params(p)).solve(use_lm=1, **LM)
    cj, ij, fj, *_ = run(dims, p, True, **LM)
    cb, ib, fb, _, _, name = run(dims, p, True, "block_jacobi", **LM)
    err_j, err = rel(cj, co), rel(cb, cm)
    print("LM", dims, "jacobi", ij, list(cj), "block", ib, list(cb), "mirror", im, cm, "err_jacobi", err_j.max(), "err", err.max())
    assert "block-Jacobi" in name and fj == [-1] * len(fj)
    assert len(ib) == 5 and len(ij) == 5
    assert sum(ib) <= 0.5 * sum(ij)
    assert cb[-1] <= cj[-1] * (1 + 1e-4)
    assert fb == [0] * 5
    assert sum(abs(a - b) for a, b in zip(ib, im)) <= 2, (ib, im)
    assert err.max() <= max(1e-5, 3 * err_j.max())


def test_gn_block_through_the_c_abi(torch, orc):
    """GN 4 x 10 on the (24, 300, 1200) instance: costs per step the mirror's (the self-calibrated bar of the LM test); four block steps of 10 iterations end below the
    default path's four steps of 25."""
    dims, band = TABLE[0]
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    cm = BaBlockMirror(dims, p).gn_solve(4, 10, "block32")
    co, _ = orc.Problem(orc.BUNDLE_ADJUST, dims, copy_params(p)).solve(nIterations=4, lIterations=10)
    cj10, *_ = run(dims, p, False, nIterations=4, lIterations=10)
    cj25, *_ = run(dims, p, False, nIterations=4, lIterations=25)
    cb, ib, fb, *_ = run(dims, p, False, "block_jacobi", nIterations=4, lIterations=10)
    err_j, err = rel(cj10, co), rel(cb, cm)
    print("GN", "block 4x10", list(cb), "mirror", cm, "jacobi 4x10", list(cj10), "4x25", list(cj25), "err_jacobi", err_j.max(), "err", err.max())
    assert len(cb) == 5 and ib == [10] * 4 and fb == [0] * 4
    assert err.max() <= max(1e-5, 3 * err_j.max())
    assert cb[-1] < cj25[-1]


@pytest.mark.parametrize("lm", [False, True])
def test_block_then_jacobi_before_init_is_the_default_plan_bit_for_bit(torch, lm):
    dims, band = TABLE[0]
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    sp = dict(nIterations=3, lIterations=25, q_tolerance=0.02) if lm else dict(nIterations=3, lIterations=10)
    a = run(dims, p, lm, **sp)
    b = run(dims, p, lm, "block_jacobi", back=True, **sp)
    assert list(a[0]) == list(b[0]) and a[1] == b[1] and a[5] == b[5]
    assert sk.same_bytes(a[3], b[3]) and sk.same_bytes(a[4], b[4])


def test_renumbered_plan_runs_the_same_block_solve(torch, monkeypatch):
    """the plan-side point order (THALLO_AB=ba_renumber=1): the blocks are built in the plan's internal ids -- the same iterations, the same costs to float accuracy"""
    dims, band = TABLE[0]
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    set_ab(monkeypatch, ba_renumber="0")
    c0, i0, f0, _, _, n0 = run(dims, p, True, "block_jacobi", **LM)
    set_ab(monkeypatch, ba_renumber="1")
    c1, i1, f1, _, _, n1 = run(dims, p, True, "block_jacobi", **LM)
    assert "renumbered" in n1 and "renumbered" not in n0
    assert sum(abs(a - b) for a, b in zip(i0, i1)) <= 2 and f1 == [0] * len(f1)
    assert rel(c1, c0).max() <= 1e-5


def test_refusals_name_the_energy(torch):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energies")
    cases = [((48, 32), thallo_amd.energy_file("image_warping"), False),
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), False),
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), True)]
    for dims, f, dbl in cases:
        s = api.ThalloSolver(dims, f, double_precision=dbl)
        assert s._L.ThalloX_PlanSetPreconditioner(s.plan, 1) != 0
        assert s.energy_name and s.energy_name in api.last_error(), api.last_error()
        with pytest.raises(RuntimeError): s.set_preconditioner("block_jacobi")
        assert s._L.ThalloX_PlanSetPreconditioner(s.plan, 0) == 0 and s.preconditioner_fallbacks() == -1
        s.close()
    s = api.ThalloSolver((5, 72, 330), thallo_amd.energy_file("bundle_adjustment"))
    assert s._L.ThalloX_PlanSetPreconditioner(s.plan, 7) != 0 and "bundle_adjustment" in api.last_error()
    s.set_preconditioner("block_jacobi")
    with pytest.raises(RuntimeError, match="bundle_adjustment"):          # a distributed plan: the preconditioner first ...
        s.set_distributed(0, 1, 0, 0, device_exchange=False)
    s.close()
    s = api.ThalloSolver((8, 72, 330), thallo_amd.energy_file("bundle_adjustment"))      # ... and the distribution first (one rank's camera shard)
    s.set_distributed(0, 1, 0, 0, device_exchange=False)
    with pytest.raises(RuntimeError, match="bundle_adjustment"):
        s.set_preconditioner("block_jacobi")
    s.close()
