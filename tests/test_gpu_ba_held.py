"""Unknowns held fixed in bundle adjustment (csrc/held.hip, ThalloX_PlanSetHeldUnknowns): the three kernels through their exported symbols against float64, then
Gauss-Newton and Levenberg-Marquardt through the C ABI -- point Jacobi, block Jacobi, the Schur complement and the assembled reduced camera matrix -- against the CPU
restatement (tests/ba_held_mirror.py), the launch counts of the loops, the never-called plan's bits, and the refusals.

Kernel instances and the device set-up are tests/test_gpu_block_precond.py's (BaDevice: the KERNEL shapes plus one camera and one point that nothing observes).  Masks
through the C ABI (ba_held_mirror.masks): cameras {0, 1}; components 6-8 of every camera; three points and one coordinate of a fourth; all points; all cameras.

Measured on an MI355X (the tests print every figure before they assert):
  held factor + apply, scaled_error of the device against the float32 restatement's e32 (bar 4 e32):
    (5, 72, 330)   LM shift: e32 1.02e-5, device 8.25e-6 (0.81 e32)    no shift: e32 1.04e-5, device 1.64e-5 (1.58 e32)
    (3, 160, 480)  LM shift: e32 9.46e-7, device 1.68e-6 (1.78 e32)    no shift: e32 1.09e-6, device 8.19e-7 (0.75 e32)
  hold_pcg's partials: 0.032 and 0.007 of the dot bar
  through the C ABI, 80 solves: the largest relative cost difference from the held mirror 1.1e-6 (bar 1e-5; err_jacobi 8.0e-7 GN, 5.4e-7 LM); LM iterations equal the
  mirror's in every case"""
import ctypes as C
import os

import numpy as np
import pytest

import shim_kernels as sk
import test_gpu_block_precond as bp
import thallo_amd
from shim_kernels import EPS, F32
from thallo_amd import api, synthetic as syn

from ba_block_mirror import BaBlockMirror, scaled_error
from ba_held_mirror import CONFIGS, held_mirror, held_precond, hold_blocks, masks, split
from ba_schur_mirror import with_extras
from helpers import copy_params, set_ab, to_device, to_host

pytestmark = pytest.mark.gpu

KERNEL, TABLE, TAIL = bp.KERNEL, bp.TABLE, bp.TAIL
MASKS = ("two_cameras", "intrinsics", "control_points", "all_points", "all_cameras")
GN = dict(nIterations=3, lIterations=10)
# 15 PCG iterations per LM step: past residual_reset_period = 10, so the residual-reset launches and the iterations behind a reset run under a mask.  Not the CPU tests' 50:
# a point-Jacobi loop that is cut off unconverged after 37 - 50 iterations cannot be pinned to 1e-5 by any float32 implementation -- on the MI355X the plan's own two LM
# loops (the default one and THALLO_AB=lm_fold_p=0, the same arithmetic in another launch order) then differ from EACH OTHER by 4.2e-4 in the cost after a step with control
# points held and by 4.6e-5 with nothing held (q_tolerance 0.001), and from the mirror by 1.2e-4 / 6.9e-5 (cameras {0, 1} / control points held), while at 15 iterations all three agree to
# 6e-7 (profiles/ba_held/README.md).  The block and Schur plans converge in fewer iterations and meet the bar at 50 as well.
LM_L = 15
LM = dict(nIterations=3, lIterations=LM_L, q_tolerance=0.1, function_tolerance=0.0)
HOLD_LAUNCHES = ("HoldPCG", "BlockHold", "BlockHoldFactor")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    lib = bp.load_shim()
    vp, it, lg = C.c_void_p, C.c_int, C.c_long
    for name, args in {"hold_pcg": [vp, vp, vp, vp, lg, vp, vp], "block_hold": [bp.RegionsT, vp, vp, vp], "block_hold_factor": [bp.RegionsT, vp, vp, vp]}.items():
        f = getattr(lib, "thallo_hip_" + name); f.argtypes = args; f.restype = it
    return lib


@pytest.fixture(scope="module")
def instances(torch, L):
    cache = {}

    def get(dims, band):
        if dims not in cache: cache[dims] = bp.BaDevice(torch, L, dims, band)
        return cache[dims]
    return get


def dev_mask(torch, mask):
    """one byte per scalar, padded to whole words, then the canary words"""
    m = np.zeros((len(mask) + 3) // 4 * 4, np.uint8); m[:len(mask)] = mask
    return bp.dev(torch, m.view(np.uint32), np.uint32)


def kernel_mask(B):
    """camera 0 fully held, components 6-8 of camera 1, component 0 of camera 2, components 0-2 of the camera nothing observes; points 1 and P / 2 fully held, one
    coordinate of point 4 and of the point nothing observes"""
    m = np.zeros(B.n, bool)
    mc, mp = split(m, B.C)
    mc[0] = True; mc[1, 6:9] = True; mc[2, 0] = True; mc[-1, 0:3] = True
    mp[1] = True; mp[B.P // 2] = True; mp[4, 1] = True; mp[-1, 0] = True
    return m


# ------------------------------------------------------------------ 1. the three kernels
@pytest.mark.parametrize("dims,band", KERNEL)
def test_hold_pcg_zeroes_the_held_words_and_sums_the_free_ones(torch, L, instances, dims, band):
    """pre and z become 0.0f at exactly the held scalars and keep their bits elsewhere (the padding behind n and the canaries included), r is not written; the partials add
    up to the float64 dot of the device's own r and z within (c + 1) 2^-24 sum |r z|, c = the chain of float additions behind a partial: 1 per scalar a lane visits, 6
    butterfly levels, 4 waves (the bar of tests/test_gpu_block_precond.py's apply test).  A second launch on the same input: the same bits."""
    B = instances(dims, band)
    mask = kernel_mask(B)
    h = {k: bp.host(B.d[k], B.na) for k in ("r", "pre", "z")}
    outs = []
    for _ in range(2):
        d = {k: bp.dev(torch, v) for k, v in h.items()}
        md, part = dev_mask(torch, mask), sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
        nb = L.thallo_hip_hold_pcg(md.data_ptr(), d["r"].data_ptr(), d["pre"].data_ptr(), d["z"].data_ptr(), B.n, part.data_ptr(), None)
        torch.cuda.synchronize()
        bp.host(md, 1, np.uint32)                                   # (the canary behind the mask)
        outs.append((bp.raw(d["pre"]), bp.raw(d["z"]), bp.raw(part)))
    got = {k: bp.host(d[k], B.na) for k in h}
    grid = (B.n + 255) // 256
    assert nb == grid and sk.written_slots(part.cpu().numpy()) == grid
    full = np.concatenate([mask, np.zeros(B.na - B.n, bool)])
    assert sk.same_bytes(got["r"], h["r"])
    for k in ("pre", "z"):
        assert got[k][full].tobytes() == np.zeros(int(full.sum()), F32).tobytes()
        assert sk.same_bytes(got[k][~full], h[k][~full])
    assert h["z"][:B.n][mask].any()                                 # (there was something to zero)
    terms = got["r"][:B.n].astype(np.float64) * got["z"][:B.n]
    c = (B.n + 256 * grid - 1) // (256 * grid) + 6 + 4
    err = abs(part.cpu().numpy()[:grid].astype(np.float64).sum() - terms.sum())
    print("hold_pcg", dims, "held", int(mask.sum()), "sum err / bar", err / ((c + 1) * EPS * np.abs(terms).sum()))
    assert err <= (c + 1) * EPS * np.abs(terms).sum()
    assert outs[0] == outs[1]


@pytest.mark.parametrize("dims,band", KERNEL)
@pytest.mark.parametrize("shifted", [True, False])
def test_held_blocks_factor_to_the_inverse_of_their_free_sub_block(torch, L, instances, dims, band, shifted):
    """block_hold on H, block_factor, block_hold_factor on G, block_apply: z = G^T (G r) against the float64 inverse of every block's free principal sub-block (of
    H + diag(shift), H the device's own float32 blocks) bordered by zeros -- 9 x 9 and 3 x 3 blocks in one launch, with the LM shift and without.  Measure and bar as
    tests/test_gpu_block_precond.py: scaled_error <= 4 e32, e32 the float32 restatement's.  Rows and columns of G at held scalars are zero exactly, so z is 0.0f there; the
    fully held camera has G = 0; H is touched in held rows and columns only.  Without the shift the camera and the point that nothing observes fall back to
    diag(sqrt(pre)) of the masked pre."""
    B = instances(dims, band)
    mask = kernel_mask(B)
    mc, mp = split(mask, B.C)
    rng = np.random.default_rng(13)
    r = B.vec("r").copy()
    r[9 * (B.C - 1): 9 * B.C] = rng.standard_normal(9); r[-3:] = rng.standard_normal(3)
    pre = np.where(mask, F32(0), B.vec("pre_lm" if shifted else "pre")).astype(F32)
    pad = np.zeros(B.na - B.n, F32)
    md, Hd, G = dev_mask(torch, mask), bp.dev(torch, B.H), bp.dev(torch, np.full(B.nf, np.nan))
    rd, pd, z = bp.dev(torch, np.concatenate([r, pad])), bp.dev(torch, np.concatenate([pre, pad])), bp.dev(torch, np.full(B.na, np.nan))
    st, part = bp.dev(torch, np.array([77], np.uint32), np.uint32), sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
    assert L.thallo_hip_block_hold(B.R, md.data_ptr(), Hd.data_ptr(), None) == 0
    assert L.thallo_hip_block_factor(B.R, Hd.data_ptr(), B.ptr("CtC") if shifted else None, pd.data_ptr(), G.data_ptr(), st.data_ptr(), None) == 0
    assert L.thallo_hip_block_hold_factor(B.R, md.data_ptr(), G.data_ptr(), None) == 0
    assert L.thallo_hip_block_apply(B.R, G.data_ptr(), rd.data_ptr(), z.data_ptr(), part.data_ptr(), None, None) > 0
    torch.cuda.synchronize()
    bp.host(md, 1, np.uint32)
    Hh = bp.unpack(bp.host(Hd, B.nf).astype(np.float64), B.C, B.P)
    want = (hold_blocks(B.Hs[0], mc), hold_blocks(B.Hs[1], mp))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(Hh, want))
    Gs = bp.unpack(bp.host(G, B.nf).astype(np.float64), B.C, B.P)
    for Gb, m in zip(Gs, (mc, mp)):
        assert np.isfinite(Gb).all() and not Gb[m[:, :, None] | m[:, None, :]].any()
    assert not Gs[0][0].any() and not Gs[1][1].any()
    shift = B.vec("CtC") if shifted else None
    z64 = held_precond("block64", B.Hs, shift, pre, B.C, mask)[0](r, exact=True)
    M32, fb32 = held_precond("block32", B.Hs, shift, pre, B.C, mask)
    e32 = scaled_error(M32(r), z64, want, shift, B.C)
    zd = bp.host(z, B.na)[:B.n]
    got = scaled_error(zd, z64, want, shift, B.C)
    fb = int(bp.host(st, 1, np.uint32)[0])
    print("held factor+apply", dims, "shift" if shifted else "no shift", "e32", e32, "device", got, "fallbacks", fb)
    assert zd[mask].tobytes() == np.zeros(int(mask.sum()), F32).tobytes() and not z64[mask].any()
    assert fb == fb32 == (0 if shifted else 2)
    assert got <= 4 * e32


# ------------------------------------------------------------------ 2. through the C ABI
def run(dims, p, lm, config, hold=None, clear=False, **sp):
    """-> dict(costs, iters, cams, pts, name, held, stats)"""
    d = to_device(copy_params(p))
    s = api.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), solverkind="levenberg_marquardt" if lm else "gauss_newton")
    if lm: s.enable_lm()
    if config == "block": s.set_preconditioner("block_jacobi")
    if config == "schur": s.set_linear_solver("schur_pcg")
    if config == "schur_explicit": s.set_linear_solver("schur_explicit_pcg")
    if hold is not None:
        s.hold(0, hold[:9 * dims[0]]); s.hold(1, hold[9 * dims[0]:])
    if clear:
        s.hold(0, None); s.hold(1, None)
    s.set_solver_parameters(**sp)
    params = s.make_params(d)
    s.init(params)
    assert s.ready(), api.last_error()
    out = dict(costs=[s.current_cost()], iters=[], held=s.held_unknowns())
    while s.step(params):
        out["costs"].append(s.current_cost()); out["iters"].append(len(s.alpha_beta_trace()))
    out.update(name=s.schedule_name, stats={k: v["launches"] for k, v in s.kernel_stats().items() if v["launches"]}, cams=to_host(d[0]).copy(), pts=to_host(d[1]).copy(),
               costs=np.array(out["costs"]))
    s.close()
    return out


def rel(a, b):
    assert len(a) == len(b), (a, b)
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.abs(np.asarray(b, np.float64))


@pytest.fixture(scope="module")
def problem():
    dims, band = TABLE[0]
    return dims, syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)


@pytest.fixture(scope="module")
def err_j(torch, problem):
    """the unheld default plan against its own mirror, GN 3 x 10 and LM 3 x 15: the largest relative cost difference, by branch"""
    dims, p = problem
    out = {}
    for lm in (False, True):
        sp = LM if lm else GN
        m = BaBlockMirror(dims, p)
        cm = m.lm_solve(3, LM_L, kind="jacobi", q_tolerance=0.1, function_tolerance=0.0)[0] if lm else m.gn_solve(3, 10, "jacobi")
        out[lm] = float(rel(run(dims, p, lm, "jacobi", **sp)["costs"], cm).max())
    print("err_jacobi", out)
    return out


_mirrors = {}


def mirror_solve(dims, p, config, lm, which):
    """(costs, iterations per step, unknowns after the solve), computed once"""
    key = (config, lm, which)
    if key not in _mirrors:
        m, kind = held_mirror(config, dims, p, masks(dims[0], dims[1])[which])
        if lm: costs, iters = m.lm_solve(3, LM_L, kind=kind, q_tolerance=0.1, function_tolerance=0.0)
        else: costs, iters = m.gn_solve(3, 10, kind), None
        _mirrors[key] = (costs, iters, np.concatenate([m.params[0].ravel(), m.params[1].ravel()]))
    return _mirrors[key]


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("config", CONFIGS)
def test_held_solve_through_the_c_abi(torch, problem, err_j, config, lm, which):
    """GN 3 x 10 / LM 3 x 15 (q_tolerance 0.1, function_tolerance 0) on the (24, 300, 1200) instance, in the caller's point order and in the plan's own
    (THALLO_AB=ba_renumber=1; the mask arrives in the caller's ids either way): the held scalars keep their bits after 3 steps and free ones move; the costs per step are the
    held mirror's within max(1e-5, 3 err_jacobi), err_jacobi the unheld default plan against its own mirror (the bar of tests/test_gpu_ba_schur.py: the held solve runs the
    same kernels); LM iteration counts differ from the mirror's by at most 2 in sum; held_unknowns() and the schedule name carry the count."""
    dims, p = problem
    mask = masks(dims[0], dims[1])[which]
    cm, im, _ = mirror_solve(dims, p, config, lm, which)
    before = np.concatenate([p[0].ravel(), p[1].ravel()])
    for ren in ("0", "1"):
        with pytest.MonkeyPatch.context() as mp:
            set_ab(mp, ba_renumber=ren)
            o = run(dims, p, lm, config, hold=mask, **(LM if lm else GN))
        after = np.concatenate([o["cams"].ravel(), o["pts"].ravel()])
        err = rel(o["costs"], cm).max()
        print("held", config, "LM" if lm else "GN", which, "renumber", ren, list(o["costs"]), o["iters"], "mirror", cm, im, "err", err, "err_jacobi", err_j[lm])
        assert ("renumbered" in o["name"]) == (ren == "1")
        assert o["held"] == int(mask.sum()) and o["name"].endswith("; %d unknowns held" % int(mask.sum()))
        assert after[mask].tobytes() == before[mask].tobytes()
        assert (after[~mask] != before[~mask]).any()
        assert err <= max(1e-5, 3 * err_j[lm])
        if lm: assert sum(abs(a - b) for a, b in zip(o["iters"], im)) <= 2, (o["iters"], im)
        else: assert o["iters"] == [0 if config.startswith("schur") and which == "all_cameras" else 10] * 3


@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("config", CONFIGS)
def test_extras_and_a_mask_through_the_c_abi(torch, config, lm):
    """the KERNEL shape with its extras (a camera and a point that nothing observes, a point observed once), one camera and the once-observed point held, one step: the held
    rows keep their bits, the cost falls, and what nothing observes stays where it is as it does without a mask"""
    dims, band = KERNEL[0]
    p, d3 = with_extras(syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band))
    mask = np.zeros(9 * d3[0] + 3 * d3[1], bool); mask[9:18] = True; mask[-3:] = True
    o = run(d3, p, lm, config, hold=mask, **(dict(nIterations=1, lIterations=20, q_tolerance=0.1) if lm else dict(nIterations=1, lIterations=10)))
    assert o["held"] == 12 and o["cams"][1].tobytes() == p[0][1].tobytes() and o["pts"][-1].tobytes() == p[1][-1].tobytes()
    assert o["cams"][-1].tobytes() == p[0][-1].tobytes() and o["pts"][-2].tobytes() == p[1][-2].tobytes()
    assert (o["cams"][0] != p[0][0]).any() and o["costs"][-1] < o["costs"][0]


# ------------------------------------------------------------------ 3. launches
@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("config", CONFIGS)
def test_no_launch_is_added_to_a_pcg_iteration(torch, problem, config, lm):
    """ThalloX_GetKernelStat after 2 steps of 6 iterations: every launch name of the unheld plan has the same count on the held plan (cameras {0, 1} held), and the held
    plan's additional launches are per step only -- HoldPCG once; with blocks BlockHold once and BlockHoldFactor once (block Jacobi) or twice (Schur: the camera blocks and
    the elimination factor)."""
    dims, p = problem
    sp = dict(nIterations=2, lIterations=6, q_tolerance=-1e30, function_tolerance=0.0) if lm else dict(nIterations=2, lIterations=6)
    a = run(dims, p, lm, config, **sp)["stats"]
    b = run(dims, p, lm, config, hold=masks(dims[0], dims[1])["two_cameras"], **sp)["stats"]
    extra = {k: b.pop(k) for k in HOLD_LAUNCHES if k in b}
    print("launches", config, "LM" if lm else "GN", a, extra)
    assert a == b
    assert extra == ({"HoldPCG": 2} if config == "jacobi" else {"HoldPCG": 2, "BlockHold": 2, "BlockHoldFactor": 2 if config == "block" else 4})


# ------------------------------------------------------------------ 4. the never-called plan's bits
@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("config", CONFIGS)
def test_cleared_and_all_zero_masks_are_the_never_called_plan_bit_for_bit(torch, problem, config, lm):
    dims, p = problem
    sp = dict(nIterations=3, lIterations=25, q_tolerance=0.02) if lm else dict(nIterations=3, lIterations=10)
    a = run(dims, p, lm, config, **sp)
    b = run(dims, p, lm, config, hold=masks(dims[0], dims[1])["two_cameras"], clear=True, **sp)
    c = run(dims, p, lm, config, hold=np.zeros(9 * dims[0] + 3 * dims[1], bool), **sp)
    assert a["held"] == -1 and b["held"] == -1 and c["held"] == 0
    for o in (b, c):
        assert list(a["costs"]) == list(o["costs"]) and a["iters"] == o["iters"] and a["name"] == o["name"] and a["stats"] == o["stats"]
        assert sk.same_bytes(a["cams"], o["cams"]) and sk.same_bytes(a["pts"], o["pts"])


# ------------------------------------------------------------------ 5. the interface and its refusals
def test_refusals_name_the_energy_and_the_reason(torch, monkeypatch, tmp_path):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energies")
    one = (C.c_ubyte * 4)(1, 0, 0, 0)
    cases = [((48, 32), thallo_amd.energy_file("image_warping"), False, "no held unknowns"),          # another hand-written energy
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), False, "no held unknowns"),      # a generated one
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), True, "doublePrecision")]        # doublePrecision = 1
    for dims, f, dbl, why in cases:
        s = api.ThalloSolver(dims, f, double_precision=dbl)
        assert s.held_unknowns() == -1
        assert s._L.ThalloX_PlanSetHeldUnknowns(s.plan, 0, one, 4) != 0
        assert s.energy_name and s.energy_name in api.last_error() and why in api.last_error(), api.last_error()
        with pytest.raises(RuntimeError): s.hold(0, np.ones(4))
        assert s._L.ThalloX_PlanSetHeldUnknowns(s.plan, 0, None, 0) == 0 and s.held_unknowns() == -1
        s.close()
    ba = thallo_amd.energy_file("bundle_adjustment")
    s = api.ThalloSolver((5, 72, 330), ba, double_precision=True)
    assert s._L.ThalloX_PlanSetHeldUnknowns(s.plan, 0, one, 4) != 0 and "bundle_adjustment" in api.last_error() and "doublePrecision" in api.last_error()
    s.close()
    s = api.ThalloSolver((5, 72, 330), ba)
    for inp in (2, 3, 4, -1, 7):                                   # observations and the two index lists are no Unknowns; neither is what does not exist
        with pytest.raises(RuntimeError, match="bundle_adjustment.*input %d is not an Unknown" % inp): s.hold(inp, np.ones(45))
    with pytest.raises(RuntimeError, match="bundle_adjustment.*44 bytes.*45 scalars"): s.hold(0, np.ones(44))
    with pytest.raises(RuntimeError, match="bundle_adjustment.*elements x components"): s.hold(1, np.ones(72))
    s.hold(0, np.ones(45))
    with pytest.raises(RuntimeError, match="bundle_adjustment.*held unknowns"):      # a distributed plan: the mask first ...
        s.set_distributed(0, 1, 0, 0, device_exchange=False)
    # ... a mask that holds every unknown: Init fails and says so; with one coordinate free it succeeds
    p = syn.bundle_adjustment(C=5, P=72, O=330, band=5)
    d = to_device(copy_params(p)); params = s.make_params(d)
    s.hold(1, np.ones(216))
    s.init(params)
    assert not s.ready() and "bundle_adjustment" in api.last_error() and "holds every unknown" in api.last_error() and s.held_unknowns() == -1
    pts = np.ones((72, 3)); pts[7, 2] = 0
    s.hold(1, pts); s.init(params)
    assert s.ready() and s.held_unknowns() == 45 + 215 and s.schedule_name.endswith("; 260 unknowns held")
    s.hold(0, None); s.hold(1, None); s.init(params)
    assert s.ready() and s.held_unknowns() == -1 and "held" not in s.schedule_name
    s.close()
    s = api.ThalloSolver((8, 72, 330), ba)                                           # ... and the distribution first (one rank's camera shard)
    s.set_distributed(0, 1, 0, 0, device_exchange=False)
    with pytest.raises(RuntimeError, match="bundle_adjustment.*distributed"): s.hold(0, np.ones(72))
    s.close()
    # a direct-solve plan (tests/test_gpu_ba_schur.py::test_refusals_name_the_energy)
    lines = "".join(f"r.{n}.J:set_materialize(true)\nr.{n}.JtJ:set_materialize(true)\n" for n in ("fit", "reg")) + "r:set_direct_solve(true)\n"
    f = tmp_path / "laplacian_direct.t"
    f.write_text(open(thallo_amd.energy_file("laplacian_graph")).read() + "\n" + lines)
    monkeypatch.setenv("THALLO_FRONTEND", "generate"); monkeypatch.setenv("THALLO_ENABLE_DIRECT_SOLVE", "1")
    s = api.ThalloSolver((256, 255), str(f))
    assert s.schedule_name == "dense direct solve"
    assert s._L.ThalloX_PlanSetHeldUnknowns(s.plan, 0, one, 4) != 0
    assert s.energy_name and s.energy_name in api.last_error() and "direct-solve" in api.last_error(), api.last_error()
    s.close()
