"""Robust losses in bundle adjustment (ThalloX_PlanSetRobustLoss; the robust instantiations of k_cost, k_compute_j and k_cam2 in csrc/energy_ba.hip): the kernels through
their exported symbols against float64, then Gauss-Newton and Levenberg-Marquardt through the C ABI -- point Jacobi, block Jacobi, the Schur complement and the assembled
reduced camera matrix -- against the CPU restatement (tests/ba_robust_mirror.py), the weights, the launch counts, the plan without a loss bit for bit, and the refusals.

Instances: tests/test_gpu_block_precond.py's KERNEL shapes and device set-up (BaDevice) with the observations of ba_robust_mirror.contaminate -- 5 % displaced by 30 - 150 px;
through the C ABI the contaminated (24, 300, 1200) instance.  Scale 2 px throughout, where about 40 % of the observations are Huber inliers.

The bars.  u = 2^-24.  The device divides and takes square roots correctly rounded (hipcc's default), and energy_ba.hip is compiled with -ffp-contract=on.
  s = r0 r0 + r1 r1      one rounded product, one fused multiply-add: |ds| <= 2 u s
  Huber, s > a^2         w = sqrt(a / sqrt(s)):  sqrt(s) 2 u / 2 + u = 2 u;  a / .  3 u;  sqrt  3 u / 2 + u = 2.5 u
  Cauchy                 t = 1 + s ia2, ia2 = 1 / (a a) on the host (2 u): s ia2 carries 4 u, the fused multiply-add adds u -> at most 5 u on t;  1 / t  6 u;  sqrt  4 u
  => |w - sqrt(rho'(s))| <= W_BAR w with W_BAR = 5 u (4 u to first order, one more for the second-order terms and the float64 reference's own rounding);  the stored block
  and residual are ONE rounded product w x (plain entry): equal to float32(w_device x plain) bit for bit, and within W_BAR + u of sqrt(rho') x plain;  rho' = w w read
  back through ThalloX_PlanRobustWeights: (1 + W_BAR)^2 (1 + u) - 1 <= 2 W_BAR + 2 u.
  rho in float32: Huber beyond a^2, 2 a sqrt(s) - a^2 with 2 a sqrt(s) <= 2 rho: 3 u on the product, u on a^2, u on the difference -> 8 u rho;  Cauchy a^2 log1p(s ia2): 5 u on
  the argument (condition of log1p <= 1), 4 u for log1pf (2 ulp), 2 u for a^2 and the product -> 11 u rho.  RHO_K = 12 roundings per term on top of the summation chain.

Figures measured on an MI355X are printed by every test before it asserts; the largest are quoted in DESIGN.md section 16."""
import ctypes as C
import os

import numpy as np
import pytest

import shim_kernels as sk
import test_gpu_block_precond as bp
import thallo_amd
from shim_kernels import EPS, F32
from thallo_amd import api, synthetic as syn

from ba_block_mirror import BaBlockMirror
from ba_held_mirror import CONFIGS, masks
from ba_robust_mirror import KINDS, contaminate, inlier_rms, rho, robust_mirror
from helpers import copy_params, set_ab, to_device, to_host

pytestmark = pytest.mark.gpu

KERNEL, TABLE = bp.KERNEL, bp.TABLE
SCALE = 2.0
KIND_ID = {"huber": 1, "cauchy": 2}
W_BAR = 5 * EPS
RHO_K = 12
GN = dict(nIterations=3, lIterations=10)
LM_L = 15                                   # (not 50: the reason at the top of tests/test_gpu_ba_held.py)
LM = dict(nIterations=3, lIterations=LM_L, q_tolerance=0.1, function_tolerance=0.0)


class FinT(C.Structure):                    # thallo_fin_t
    _fields_ = [("alphaN", api.SumT), ("tickets", C.c_void_p), ("alphaD_word", C.c_void_p), ("betaN_word", C.c_void_p)]


NO_FIN = FinT(api.SumT(None, 0), None, None, None)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    lib = bp.load_shim()
    vp, it, fl = C.c_void_p, C.c_int, C.c_float
    sig = {
        "ba_cost": [it, it, it] + [vp] * 7,
        "ba_cost_robust": [it, it, it] + [vp] * 5 + [it, fl, vp, vp],
        "ba_compute_j_robust": [it] + [vp] * 6 + [it, fl, vp, vp, vp, vp],
        "ba_apply_jtj2_fin_robust": [it, it] + [vp] * 15 + [FinT, vp, vp],
        "ba_apply_jtj2_lm_robust": [it, it] + [vp] * 15,
        "ba_lm_reset_residual_robust": [it, it] + [vp] * 17,
    }
    for name, args in sig.items():
        f = getattr(lib, "thallo_hip_" + name); f.argtypes = args; f.restype = it
    return lib


class RobustDevice:
    """bp.BaDevice with contaminated observations: the plain kernel's Jb / F (the reference every robust output is compared with), and per loss the robust kernel's"""

    def __init__(self, torch, L, dims, band, renumber, zero_some=False):
        self.B = B = bp.BaDevice(torch, L, dims, band, renumber)
        p, self.outliers = contaminate(syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band))
        self.oc, self.op = p[3], p[4]
        self.torch, self.L = torch, L
        obs = p[2].copy()
        P = B.ptr
        self.cobs = bp.host(B.d["cam_obs"], B.O, np.int32)
        if zero_some:      # the hand-made case: every 7th observation becomes the device's own float32 projection, so its residual is at or next to 0
            F0 = self.plain(obs)[1]
            self.zeroed = np.zeros(B.O, bool); self.zeroed[::7] = True
            pred = np.empty_like(obs); pred[self.cobs] = (obs[self.cobs] - F0.reshape(-1, 2)).astype(F32)
            obs[self.zeroed] = pred[self.zeroed]
        self.obs = obs
        self.Jb0, self.F0 = self.plain(obs)
        self.s64 = (self.F0.astype(np.float64).reshape(-1, 2) ** 2).sum(1)          # camera order q

    def plain(self, obs):
        B, t = self.B, self.torch
        od, Jb, F = bp.dev(t, obs), bp.dev(t, np.full(24 * B.O, np.nan)), bp.dev(t, np.full(2 * B.O, np.nan))
        assert self.L.thallo_hip_ba_compute_j(B.O, B.ptr("cams"), B.ptr("pts"), od.data_ptr(), B.ptr("cam_obs"), B.ptr("q_cam"), B.ptr("q_pt"), Jb.data_ptr(), F.data_ptr(), None) == 0
        t.cuda.synchronize()
        bp.host(od, 1)
        return bp.host(Jb, 24 * B.O), bp.host(F, 2 * B.O)

    def robust(self, kind):
        """-> (Jb, F, w) of the robust kernel on the host, and the device buffers (obs, Jb, F, w) for the launches behind it"""
        B, t = self.B, self.torch
        d = dict(obs=bp.dev(t, self.obs), Jb=bp.dev(t, np.full(24 * B.O, np.nan)), F=bp.dev(t, np.full(2 * B.O, np.nan)), w=bp.dev(t, np.full(B.O, np.nan)))
        assert self.L.thallo_hip_ba_compute_j_robust(B.O, B.ptr("cams"), B.ptr("pts"), d["obs"].data_ptr(), B.ptr("cam_obs"), B.ptr("q_cam"), B.ptr("q_pt"), KIND_ID[kind], SCALE,
                                                     d["Jb"].data_ptr(), d["F"].data_ptr(), d["w"].data_ptr(), None) == 0
        t.cuda.synchronize()
        bp.host(d["obs"], 1)
        return bp.host(d["Jb"], 24 * B.O), bp.host(d["F"], 2 * B.O), bp.host(d["w"], B.O), d


@pytest.fixture(scope="module")
def instances(torch, L):
    cache = {}

    def get(dims, band, renumber=False, zero_some=False):
        key = (dims, band, renumber, zero_some)
        if key not in cache: cache[key] = RobustDevice(torch, L, dims, band, renumber, zero_some)
        return cache[key]
    return get


SHAPES = [(KERNEL[0][0], KERNEL[0][1], False), (KERNEL[1][0], KERNEL[1][1], False), (KERNEL[0][0], KERNEL[0][1], True)]


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims,band,renumber", SHAPES)
def test_weights_and_scaled_blocks_against_float64(torch, L, instances, dims, band, renumber, kind):
    """precomputeJ's robust instantiation: w against sqrt(rho'(s)) in float64, s from the plain kernel's residual (the same expression, so the same bits the robust kernel
    had): within W_BAR; Huber: exactly 1 at the inliers and both branches populated.  Jb and F: float32(w x plain) bit for bit with the device's own w -- one rounded
    product, the same one k_cam2 repeats -- and within W_BAR + u of sqrt(rho') x plain.  Canary words behind every buffer."""
    R = instances(dims, band, renumber)
    if not renumber and dims == KERNEL[0][0]: assert list(np.diff(R.B.cam_ptr)) == [65, 65, 70, 61, 69, 0]      # one trip + an odd tail of 1 .. 6 lanes
    if dims == KERNEL[1][0]: assert list(np.diff(R.B.cam_ptr)) == [160, 160, 160, 0]                            # two trips, the second one half empty
    Jb, F, w, _ = R.robust(kind)
    want = np.sqrt(rho(kind, SCALE, R.s64)[1])
    err = np.abs(w.astype(np.float64) - want) / want
    inl = R.s64 <= SCALE * SCALE
    print("w", dims, renumber, kind, "inliers", float(inl.mean()), "largest |w - sqrt(rho')| / w in u", float(err.max() / EPS))
    assert 0.2 < inl.mean() < 0.8
    assert np.isfinite(w).all() and (w > 0).all() and (w <= 1).all()
    assert (err <= W_BAR).all()
    if kind == "huber":
        clear = np.abs(R.s64 - SCALE ** 2) >= 1e-3 * SCALE ** 2
        assert (w[inl & clear] == 1.0).all() and (w[~inl & clear] < 1.0).all()
    assert sk.same_bytes(Jb.reshape(-1, 24), (R.Jb0.reshape(-1, 24) * w[:, None]).astype(F32))
    assert sk.same_bytes(F.reshape(-1, 2), (R.F0.reshape(-1, 2) * w[:, None]).astype(F32))
    for got, plain, k in ((Jb, R.Jb0, 24), (F, R.F0, 2)):
        ref = plain.astype(np.float64).reshape(-1, k) * want[:, None]
        e = np.abs(got.astype(np.float64).reshape(-1, k) - ref)
        print("   scaled", k, "largest err in u", float((e / np.maximum(np.abs(ref), 1e-300)).max() / EPS))
        assert (e <= (W_BAR + EPS) * np.abs(ref)).all()


@pytest.mark.parametrize("kind", KINDS)
def test_residuals_at_zero_stay_finite_and_carry_weight_one(torch, L, instances, kind):
    """every 7th observation replaced by the device's own float32 projection: s there is 0 or a few ulp of the prediction squared; w = 1 exactly, Jb and F there are the
    plain kernel's bits, everything is finite, and the robust cost is finite and within its bar"""
    dims, band = KERNEL[0]
    R = instances(dims, band, False, True)
    Jb, F, w, _ = R.robust(kind)
    z = R.zeroed[R.cobs]
    print("zeroed", kind, "largest s there", float(R.s64[z].max()), "exact zeros", int((R.s64[z] == 0).sum()), "of", int(z.sum()))
    assert R.s64[z].max() < 1e-4
    assert np.isfinite(Jb).all() and np.isfinite(F).all() and np.isfinite(w).all()
    assert (w[z] == 1.0).all()
    assert sk.same_bytes(Jb.reshape(-1, 24)[z], R.Jb0.reshape(-1, 24)[z]) and sk.same_bytes(F.reshape(-1, 2)[z], R.F0.reshape(-1, 2)[z])
    check_cost(torch, L, R, kind)


def check_cost(torch, L, R, kind):
    """thallo_hip_ba_cost_robust: the partials add up to 1/2 sum rho(s) in float64 (s from the plain kernel's residuals) within (c + 1 + RHO_K) u sum |terms|, c the chain of
    float additions behind a partial: the terms a lane visits, 6 butterfly levels, 4 waves (the bar of the sibling kernel tests' dot products), RHO_K for rho itself"""
    B = R.B
    od, part = bp.dev(torch, R.obs), sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
    oc, op = bp.dev(torch, B.q_cam[np.argsort(R.cobs)], np.int32), bp.dev(torch, B.q_pt[np.argsort(R.cobs)], np.int32)      # observation -> camera / point in the device's ids
    nb = L.thallo_hip_ba_cost_robust(B.C, B.P, B.O, B.ptr("cams"), B.ptr("pts"), od.data_ptr(), oc.data_ptr(), op.data_ptr(), KIND_ID[kind], SCALE, part.data_ptr(), None)
    torch.cuda.synchronize()
    for t in (od, oc, op): bp.host(t, 1, np.uint32)
    grid = (B.O + 255) // 256
    ph = part.cpu().numpy()
    assert nb == grid and sk.written_slots(ph) == grid
    terms = 0.5 * rho(kind, SCALE, R.s64)[0]
    c = (B.O + 256 * grid - 1) // (256 * grid) + 6 + 4
    err = abs(ph[:grid].astype(np.float64).sum() - terms.sum())
    print("cost", kind, "err / bar", err / ((c + 1 + RHO_K) * EPS * terms.sum()))
    assert np.isfinite(ph[:grid]).all()
    assert err <= (c + 1 + RHO_K) * EPS * terms.sum()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims,band,renumber", SHAPES)
def test_robust_cost_against_float64(torch, L, instances, dims, band, renumber, kind):
    check_cost(torch, L, instances(dims, band, renumber), kind)


def dense_js(B, Jb):
    """the stored blocks as a dense float64 matrix [2 O, n]"""
    J = np.zeros((2 * B.O, B.n))
    b = Jb.astype(np.float64).reshape(B.O, 24)
    q = np.arange(B.O)
    for r in range(2):
        for k in range(9): J[2 * q + r, 9 * B.q_cam + k] = b[:, 12 * r + k]
        for k in range(3): J[2 * q + r, 9 * B.C + 3 * B.q_pt + k] = b[:, 12 * r + 9 + k]
    return J


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims,band,renumber", SHAPES)
def test_robust_apply_and_residual_reset_against_float64_of_the_stored_blocks(torch, L, instances, dims, band, renumber, kind):
    """The robust camera launch + the point launch: Ap against J_s^T (J_s p) (GN), + CtC p (LM), and the residual reset r = b - (J_s^T J_s + CtC) delta with the partials
    of r . M^-1 r, in float64 from the device's own stored Jb (J_s as a dense matrix).  Bars of tests/test_gpu_parity.py for the plain apply: |Ap - ref| <= 2e-5 max |ref|,
    p . Ap within 1e-5; the reset likewise (r against max(|b|, |A delta|), the dot against the float64 dot of the device's own r and M^-1)."""
    R = instances(dims, band, renumber)
    B = R.B
    Jb, F, w, d = R.robust(kind)
    J = dense_js(B, Jb)
    rng = np.random.default_rng(17)
    pad = np.zeros(B.na - B.n, F32)
    vec = lambda a: bp.dev(torch, np.concatenate([np.asarray(a, F32), pad]))
    p, delta, b = (rng.standard_normal(B.n).astype(F32) for _ in range(3))
    ctc, pre = rng.uniform(0.5, 2.0, B.n).astype(F32), rng.uniform(0.1, 1.0, B.n).astype(F32)
    pd, dd, bd, cd, md = vec(p), vec(delta), vec(b), vec(ctc), vec(pre)
    JP, JpC = bp.dev(torch, np.full(6 * B.O, np.nan)), bp.dev(torch, np.full(2 * B.O, np.nan))
    assert L.thallo_hip_ba_pack_point_blocks(B.O, d["Jb"].data_ptr(), B.ptr("q_ptk"), JP.data_ptr(), None) == 0
    lists = (B.C, B.P, B.ptr("cam_ptr"), B.ptr("q_pt"), B.ptr("pt_pos"), B.ptr("pt_ptr"), B.ptr("cams"), B.ptr("pts"), JP.data_ptr(), JpC.data_ptr())
    JtJ = J.T @ J
    for lm in (False, True):
        Ap, part = vec(np.full(B.n, np.nan)), sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
        if lm: nb = L.thallo_hip_ba_apply_jtj2_lm_robust(*lists, pd.data_ptr(), cd.data_ptr(), Ap.data_ptr(), part.data_ptr(), None, d["w"].data_ptr(), None)
        else: nb = L.thallo_hip_ba_apply_jtj2_fin_robust(*lists, pd.data_ptr(), Ap.data_ptr(), part.data_ptr(), None, None, None, None, NO_FIN, d["w"].data_ptr(), None)
        torch.cuda.synchronize()
        ph = part.cpu().numpy()
        assert nb > 0 and sk.written_slots(ph) == nb
        got = bp.host(Ap, B.na)[:B.n].astype(np.float64)
        ref = JtJ @ p.astype(np.float64) + (ctc.astype(np.float64) * p if lm else 0.0)
        dot = float(p.astype(np.float64) @ ref)
        e_ap, e_dot = np.abs(got - ref).max() / np.abs(ref).max(), abs(ph[:nb].astype(np.float64).sum() - dot) / abs(dot)
        print("apply", dims, renumber, kind, "LM" if lm else "GN", "Ap err", e_ap, "p.Ap err", e_dot)
        assert e_ap <= 2e-5 and e_dot <= 1e-5
    r, part = vec(np.full(B.n, np.nan)), sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
    nb = L.thallo_hip_ba_lm_reset_residual_robust(*lists, dd.data_ptr(), cd.data_ptr(), bd.data_ptr(), md.data_ptr(), r.data_ptr(), part.data_ptr(), None, d["w"].data_ptr(), None)
    torch.cuda.synchronize()
    ph = part.cpu().numpy()
    assert nb > 0 and sk.written_slots(ph) == nb
    got = bp.host(r, B.na)[:B.n].astype(np.float64)
    Ad = JtJ @ delta.astype(np.float64) + ctc.astype(np.float64) * delta
    ref = b.astype(np.float64) - Ad
    e_r = np.abs(got - ref).max() / max(np.abs(Ad).max(), np.abs(b).max())
    dot = float((pre.astype(np.float64) * got) @ got)
    e_dot = abs(ph[:nb].astype(np.float64).sum() - dot) / abs(dot)
    print("reset", dims, renumber, kind, "r err", e_r, "r.M^-1 r err", e_dot)
    assert e_r <= 2e-5 and e_dot <= 1e-5
    for t in (pd, dd, bd, cd, md, JP, JpC, d["w"], d["Jb"]): bp.host(t, 1, np.uint32)      # (the canaries behind the inputs and the workspace)
    assert sk.same_bytes(bp.host(d["w"], B.O), w)


def test_robust_entry_points_refuse_a_bad_loss_and_a_missing_w(torch, L, instances):
    """an unknown kind, a scale that is not finite and positive, or w == NULL is -hipErrorInvalidValue: these entry points never run the squared loss"""
    R = instances(*KERNEL[0]); B = R.B
    _, _, _, d = R.robust("huber")
    a = (B.O, B.ptr("cams"), B.ptr("pts"), d["obs"].data_ptr(), B.ptr("cam_obs"), B.ptr("q_cam"), B.ptr("q_pt"))
    out = (d["Jb"].data_ptr(), d["F"].data_ptr(), d["w"].data_ptr(), None)
    for kind, scale in ((0, 2.0), (3, 2.0), (1, 0.0), (2, -1.0), (1, float("nan")), (2, float("inf"))):
        assert L.thallo_hip_ba_compute_j_robust(*a, kind, scale, *out) == sk.INVALID
    assert L.thallo_hip_ba_compute_j_robust(*a, 1, 2.0, d["Jb"].data_ptr(), d["F"].data_ptr(), None, None) == sk.INVALID
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. through the C ABI
def run(dims, p, lm, config, loss=None, then_trivial=False, hold=None, **sp):
    """-> dict(costs, iters, cams, pts, name, stats, weights, before_last): loss = (kind, scale) or None (the call is never made)"""
    d = to_device(copy_params(p))
    s = api.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), solverkind="levenberg_marquardt" if lm else "gauss_newton")
    if lm: s.enable_lm()
    if config == "block": s.set_preconditioner("block_jacobi")
    if config == "schur": s.set_linear_solver("schur_pcg")
    if config == "schur_explicit": s.set_linear_solver("schur_explicit_pcg")
    if loss is not None: s.set_robust_loss(*loss)
    if then_trivial: s.set_robust_loss("trivial")
    if hold is not None:
        s.hold(0, hold[:9 * dims[0]]); s.hold(1, hold[9 * dims[0]:])
    s.set_solver_parameters(**sp)
    params = s.make_params(d)
    s.init(params)
    assert s.ready(), api.last_error()
    out = dict(costs=[s.current_cost()], iters=[], before_last=None)
    while True:
        x = (to_host(d[0]).copy(), to_host(d[1]).copy())
        if not s.step(params): break
        out["before_last"] = x
        out["costs"].append(s.current_cost()); out["iters"].append(len(s.alpha_beta_trace()))
    on = loss is not None and loss[0] != "trivial" and not then_trivial
    out.update(name=s.schedule_name, stats={k: v["launches"] for k, v in s.kernel_stats().items() if v["launches"]}, cams=to_host(d[0]).copy(), pts=to_host(d[1]).copy(),
               costs=np.array(out["costs"]), weights=s.robust_weights() if on else None,
               no_weights=s._L.ThalloX_PlanRobustWeights(s.plan, np.empty(dims[2], F32).ctypes.data_as(C.c_void_p), dims[2]))
    s.close()
    return out


def rel(a, b):
    assert len(a) == len(b), (a, b)
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.abs(np.asarray(b, np.float64))


@pytest.fixture(scope="module")
def problem():
    dims, band = TABLE[0]
    p, outliers = contaminate(syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band))
    return dims, p, outliers


@pytest.fixture(scope="module")
def err_j(torch, problem):
    """the PLAIN default plan against the PLAIN mirror on the contaminated instance, GN 3 x 10 and LM 3 x 15: the largest relative cost difference, by branch"""
    dims, p, _ = problem
    out = {}
    for lm in (False, True):
        m = BaBlockMirror(dims, p)
        cm = m.lm_solve(3, LM_L, kind="jacobi", q_tolerance=0.1, function_tolerance=0.0)[0] if lm else m.gn_solve(3, 10, "jacobi")
        out[lm] = float(rel(run(dims, p, lm, "jacobi", **(LM if lm else GN))["costs"], cm).max())
    print("err_jacobi", out)
    return out


_mirrors = {}


def mirror_solve(dims, p, config, lm, kind, which=None):
    """(costs, iterations per step), computed once"""
    key = (config, lm, kind, which)
    if key not in _mirrors:
        m, k = robust_mirror(config, kind, SCALE, dims, p, None if which is None else masks(dims[0], dims[1])[which])
        _mirrors[key] = m.lm_solve(3, LM_L, kind=k, q_tolerance=0.1, function_tolerance=0.0) if lm else (m.gn_solve(3, 10, k), None)
    return _mirrors[key]


def device_s(torch, L, dims, p, x):
    """s per observation (the caller's ids) at the unknowns x = (cameras, points), from the plain precomputeJ kernel's residuals: the bits the robust instantiation forms
    its weights from (the same expression under -ffp-contract=on)"""
    O = dims[2]
    ids = bp.dev(torch, np.arange(O), np.int32)
    t = [bp.dev(torch, a) for a in (x[0], x[1], p[2])] + [ids, bp.dev(torch, p[3], np.int32), bp.dev(torch, p[4], np.int32)]
    Jb, F = bp.dev(torch, np.zeros(24 * O)), bp.dev(torch, np.zeros(2 * O))
    assert L.thallo_hip_ba_compute_j(O, *[a.data_ptr() for a in t], Jb.data_ptr(), F.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return (bp.host(F, 2 * O).astype(np.float64).reshape(-1, 2) ** 2).sum(1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("config", CONFIGS)
def test_robust_solve_through_the_c_abi(torch, L, problem, err_j, config, lm, kind):
    """GN 3 x 10 / LM 3 x 15 (q_tolerance 0.1, function_tolerance 0) on the contaminated (24, 300, 1200) instance, scale 2, in the caller's point order and in the plan's own
    (THALLO_AB=ba_renumber=1).  Costs per step: the robust mirror's within max(1e-5, 3 err_jacobi), err_jacobi the PLAIN default plan against the PLAIN mirror on the same
    instance (existing code against the existing mirror); LM iteration counts within 2 in sum.  robust_weights(), in the caller's observation ids under both orders:
    against the mirror's rho' (ba_robust_mirror.rho, float64) at the last linearisation -- at s of the unknowns as they were before the last step, formed from the plain
    precomputeJ kernel's residuals at those unknowns (device_s: the oracle's float32 residuals differ from the device's by a few ulp of the PREDICTION, some 1e-4 px, which
    on a 2 px residual is 1e-4 of s and would say nothing about w) -- within the w bar squared, 2 W_BAR + 2 u; exactly 1.0 where that s is an inlier's, away from
    |s - a^2| < 1e-3 a^2.  The difference from the mirror's own weights (oracle residuals, the mirror's trajectory) is printed next to it."""
    dims, p, outliers = problem
    cm, im = mirror_solve(dims, p, config, lm, kind)
    m_last = robust_mirror(config, kind, SCALE, dims, p)[0]
    for ren in ("0", "1"):
        with pytest.MonkeyPatch.context() as mp:
            set_ab(mp, ba_renumber=ren)
            o = run(dims, p, lm, config, loss=(kind, SCALE), **(LM if lm else GN))
        err = rel(o["costs"], cm).max()
        print("robust", config, "LM" if lm else "GN", kind, "renumber", ren, list(o["costs"]), o["iters"], "mirror", cm, im, "err", err, "err_jacobi", err_j[lm])
        assert ("renumbered" in o["name"]) == (ren == "1")
        assert "; %s loss, scale 2" % kind in o["name"]
        assert len(o["costs"]) == 4
        assert err <= max(1e-5, 3 * err_j[lm])
        if lm: assert sum(abs(a - b) for a, b in zip(o["iters"], im)) <= 2, (o["iters"], im)
        else: assert o["iters"] == [10] * 3
        s = device_s(torch, L, dims, p, o["before_last"])
        want = rho(kind, SCALE, s)[1]
        got = o["weights"].astype(np.float64)
        e = np.abs(got - want) / want
        m_last.params = [o["before_last"][0].copy(), o["before_last"][1].copy()] + [a.copy() for a in p[2:]]
        m_last.linearise()
        print("   weights: largest |rho' - mirror's rho'(device s)| / rho' in u", float(e.max() / EPS), "; against the mirror's own s", float((np.abs(got - m_last.weights) / m_last.weights).max()),
              "; mean weight of the displaced observations", float(got[outliers].mean()), "of the others", float(got[~outliers].mean()))
        assert (got > 0).all() and (got <= 1).all()
        assert (e <= 2 * W_BAR + 2 * EPS).all()
        if kind == "huber":
            clear = np.abs(s - SCALE ** 2) >= 1e-3 * SCALE ** 2
            assert (got[(s <= SCALE ** 2) & clear] == 1.0).all()
        assert got[outliers].mean() < 0.5 * got[~outliers].mean()


@pytest.mark.parametrize("kind", KINDS)
def test_a_robust_loss_keeps_the_outliers_from_steering_the_device_solve(torch, problem, kind):
    """LM 8 x 50, q_tolerance 0.001, point Jacobi, on the device: the inliers' RMS reprojection error ends below where it started and below half of the squared loss's"""
    dims, p, outliers = problem
    sp = dict(nIterations=8, lIterations=50, q_tolerance=0.001)
    rms = lambda cams, pts: inlier_rms(BaBlockMirror(dims, [cams, pts] + list(p[2:])), outliers)
    start = rms(p[0], p[1])
    a = run(dims, p, True, "jacobi", **sp)
    b = run(dims, p, True, "jacobi", loss=(kind, SCALE), **sp)
    plain, robust = rms(a["cams"], a["pts"]), rms(b["cams"], b["pts"])
    print("inlier RMS on the device", kind, "start", start, "squared loss", plain, "robust", robust, "robust costs", list(b["costs"]))
    assert robust < start and robust < 0.5 * plain


@pytest.mark.parametrize("config", CONFIGS)
def test_huber_with_a_huge_scale_is_the_plan_without_a_loss(torch, problem, config):
    """scale 1e18: every w is exactly 1.0f, so the unknowns after GN 3 x 10 are byte-equal to the never-called plan's; the costs (another instantiation of k_cost, the same
    sums) agree to 1e-6; every weight reads 1.0"""
    dims, p, _ = problem
    a = run(dims, p, False, config, **GN)
    b = run(dims, p, False, config, loss=("huber", 1e18), **GN)
    print("huber 1e18", config, list(a["costs"]), list(b["costs"]))
    assert sk.same_bytes(a["cams"], b["cams"]) and sk.same_bytes(a["pts"], b["pts"])
    assert rel(b["costs"], a["costs"]).max() <= 1e-6
    assert (b["weights"] == 1.0).all() and a["no_weights"] == -1
    assert b["name"] == a["name"] + "; huber loss, scale 1e+18"


@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("config", CONFIGS)
def test_trivial_and_set_then_trivial_are_the_never_called_plan_bit_for_bit(torch, problem, config, lm):
    dims, p, _ = problem
    sp = dict(nIterations=3, lIterations=25, q_tolerance=0.02) if lm else dict(nIterations=3, lIterations=10)
    a = run(dims, p, lm, config, **sp)
    b = run(dims, p, lm, config, loss=("trivial", 0.0), **sp)
    c = run(dims, p, lm, config, loss=("cauchy", SCALE), then_trivial=True, **sp)
    for o in (b, c):
        assert list(a["costs"]) == list(o["costs"]) and a["iters"] == o["iters"] and a["name"] == o["name"] and a["stats"] == o["stats"]
        assert sk.same_bytes(a["cams"], o["cams"]) and sk.same_bytes(a["pts"], o["pts"])
        assert o["no_weights"] == -1 and "loss" not in o["name"]


@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("config", CONFIGS)
def test_no_launch_is_added_by_a_loss(torch, problem, config, lm):
    """ThalloX_GetKernelStat after 2 steps of 12 iterations (past a residual reset in LM): a robust plan's launch counts equal the plain plan's, name by name"""
    dims, p, _ = problem
    sp = dict(nIterations=2, lIterations=12, q_tolerance=-1e30, function_tolerance=0.0) if lm else dict(nIterations=2, lIterations=12)
    a = run(dims, p, lm, config, **sp)["stats"]
    for kind in KINDS:
        b = run(dims, p, lm, config, loss=(kind, SCALE), **sp)["stats"]
        print("launches", config, "LM" if lm else "GN", kind, b)
        assert a == b


@pytest.mark.parametrize("which", ["two_cameras", "intrinsics"])
@pytest.mark.parametrize("config", CONFIGS)
def test_a_loss_and_a_mask_compose(torch, problem, err_j, config, which):
    """Huber 2 and held unknowns, GN 3 x 10: the held scalars keep their bits, the costs are the composed mirror's within the bar, the name carries the loss in front of the
    held count"""
    dims, p, _ = problem
    mask = masks(dims[0], dims[1])[which]
    cm, _ = mirror_solve(dims, p, config, False, "huber", which)
    o = run(dims, p, False, config, loss=("huber", SCALE), hold=mask, **GN)
    before, after = np.concatenate([p[0].ravel(), p[1].ravel()]), np.concatenate([o["cams"].ravel(), o["pts"].ravel()])
    err = rel(o["costs"], cm).max()
    print("robust + held", config, which, list(o["costs"]), "mirror", cm, "err", err)
    assert after[mask].tobytes() == before[mask].tobytes() and (after[~mask] != before[~mask]).any()
    assert err <= max(1e-5, 3 * err_j[False])
    assert o["name"].endswith("; huber loss, scale 2; %d unknowns held" % int(mask.sum()))


# ------------------------------------------------------------------ 3. the interface and its refusals
def test_refusals_name_the_energy_and_the_reason(torch, monkeypatch, tmp_path):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energies")
    cases = [((48, 32), thallo_amd.energy_file("image_warping"), False, False, "no robust loss"),            # another hand-written energy
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), False, False, "no robust loss"),        # a generated one
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), False, True, "no robust loss"),         # ... with THALLO_FRONTEND=generate
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), True, False, "doublePrecision")]        # doublePrecision = 1
    for dims, f, dbl, gen, why in cases:
        with pytest.MonkeyPatch.context() as mp:
            if gen: mp.setenv("THALLO_FRONTEND", "generate")
            s = api.ThalloSolver(dims, f, double_precision=dbl)
            assert s._L.ThalloX_PlanSetRobustLoss(s.plan, 1, 2.0) != 0
            assert s.energy_name and s.energy_name in api.last_error() and why in api.last_error(), api.last_error()
            with pytest.raises(RuntimeError): s.set_robust_loss("cauchy", 2.0)
            s.set_robust_loss("trivial")                                 # (the default is no refusal anywhere)
            with pytest.raises(RuntimeError): s.robust_weights()
            s.close()
    ba = thallo_amd.energy_file("bundle_adjustment")
    s = api.ThalloSolver((5, 72, 330), ba, double_precision=True)
    assert s._L.ThalloX_PlanSetRobustLoss(s.plan, 2, 2.0) != 0 and "bundle_adjustment" in api.last_error() and "doublePrecision" in api.last_error()
    s.close()
    s = api.ThalloSolver((5, 72, 330), ba)
    for kind in (3, -1, 17):
        with pytest.raises(RuntimeError, match="bundle_adjustment.*unknown robust loss kind"): s.set_robust_loss(kind, 2.0)
    with pytest.raises(ValueError): s.set_robust_loss("tukey", 2.0)
    for kind in KINDS:
        for scale in (0.0, -2.0, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(RuntimeError, match="bundle_adjustment.*finite and positive"): s.set_robust_loss(kind, scale)
    assert "loss" not in s.schedule_name
    out = np.empty(330, F32)
    assert s._L.ThalloX_PlanRobustWeights(s.plan, out.ctypes.data_as(C.c_void_p), 330) == -1      # nothing set, nothing initialised
    s.set_robust_loss("huber", 2.0)
    with pytest.raises(RuntimeError, match="bundle_adjustment.*robust losses run on one GPU"):      # a distributed plan: the loss first ...
        s.set_distributed(0, 1, 0, 0, device_exchange=False)
    p = syn.bundle_adjustment(C=5, P=72, O=330, band=5)
    d = to_device(copy_params(p)); params = s.make_params(d)
    assert s._L.ThalloX_PlanRobustWeights(s.plan, out.ctypes.data_as(C.c_void_p), 330) == -1      # ... set, but not in force before Init
    s.init(params)
    assert s.ready() and s.schedule_name.endswith("; huber loss, scale 2")
    assert s._L.ThalloX_PlanRobustWeights(s.plan, out.ctypes.data_as(C.c_void_p), 329) == -1      # a wrong n
    assert s._L.ThalloX_PlanRobustWeights(s.plan, out.ctypes.data_as(C.c_void_p), 330) == 330 and (out == 1.0).all()      # before the first linearisation
    s.set_robust_loss("cauchy", 0.5); s.init(params)                                                # a re-Init takes the new loss
    assert s.ready() and s.schedule_name.endswith("; cauchy loss, scale 0.5")
    s.set_robust_loss("trivial"); s.init(params)
    assert s.ready() and "loss" not in s.schedule_name
    assert s._L.ThalloX_PlanRobustWeights(s.plan, out.ctypes.data_as(C.c_void_p), 330) == -1
    s.close()
    s = api.ThalloSolver((8, 72, 330), ba)                                                          # ... and the distribution first (one rank's camera shard)
    s.set_distributed(0, 1, 0, 0, device_exchange=False)
    with pytest.raises(RuntimeError, match="bundle_adjustment.*distributed"): s.set_robust_loss("huber", 2.0)
    s.close()
    # a direct-solve plan (tests/test_gpu_ba_schur.py::test_refusals_name_the_energy)
    lines = "".join(f"r.{n}.J:set_materialize(true)\nr.{n}.JtJ:set_materialize(true)\n" for n in ("fit", "reg")) + "r:set_direct_solve(true)\n"
    f = tmp_path / "laplacian_direct.t"
    f.write_text(open(thallo_amd.energy_file("laplacian_graph")).read() + "\n" + lines)
    monkeypatch.setenv("THALLO_FRONTEND", "generate"); monkeypatch.setenv("THALLO_ENABLE_DIRECT_SOLVE", "1")
    s = api.ThalloSolver((256, 255), str(f))
    assert s.schedule_name == "dense direct solve"
    assert s._L.ThalloX_PlanSetRobustLoss(s.plan, 1, 2.0) != 0
    assert s.energy_name and s.energy_name in api.last_error() and "direct-solve" in api.last_error(), api.last_error()
    s.close()
