"""The assembled reduced camera matrix of bundle adjustment's Schur-complement solve (csrc/ba_schur_explicit.hip, ThalloX_PlanSetLinearSolver kind 2): W, the assembled S and
S x against float64, the stored S's symmetry and reproducibility, the gate, held points, kind 1's matrix-free apply, then Levenberg-Marquardt and Gauss-Newton through the
C ABI against the CPU restatement (tests/ba_schur_explicit_mirror.py), the default path's bits, the renumbered plan, the block count, the refusals and the budget.

Kernel instances: tests/test_gpu_ba_schur.py's two with their extras -- (5, 72, 330, band 5): cameras on both sides of 64 observations, blocks of 61 - 70 terms;
(3, 160, 480, band 3): 160 terms per block, more than a wave has lanes; both with a camera and a point nothing observes and a point observed once -- and
(72, 500, 2500, band 72), whose rows hold 49 - 69 blocks, on both sides of a wave's 64 lanes.  Each in the caller's point order and in the plan's renumbered order, with and
without the LM shift.  The device state is tests/test_gpu_ba_schur.py's SchurDevice.

The float64 side is block-wise from the device's own Jb (ba_schur_explicit_mirror.blocks64); the bar of each operation is 4 e32, e32 the distance from float64 of the
float32 restatement in the kernels' summation order (w32, cam_blocks32, assemble32, apply32), recomputed on every run; the measure is max |err| / max |value|.

MEASURED below is part of this docstring."""
import ctypes as C
import os

import numpy as np
import pytest

import shim_kernels as sk
import thallo_amd
from shim_kernels import F32
from thallo_amd import api, synthetic as syn

import test_gpu_ba_schur as base
from test_gpu_ba_schur import SchurDevice, dev, host, rel, torch      # noqa: F401  (torch: the module fixture)
from ba_schur_mirror import rel_max, with_extras
from ba_schur_explicit_mirror import BaSchurExplicitMirror, SchurStructure, apply32, assemble32, blocks64, brute_force_counts, cam_blocks32, w32
from ba_schur_mirror import SchurLists
from helpers import copy_params, set_ab, to_device, to_host

pytestmark = pytest.mark.gpu

MEASURED = """Measured on an MI355X (multiples of e32 over the twelve cases; the tests print them before they assert; also in profiles/ba_schur_explicit/README.md; the bar is 4):
  W 0.61 - 1.67, assembled S 1.00 - 2.03, S x 0.74 - 2.23; assembled against matrix-free S x: 0.13 - 0.38 of the sum of the two bars.
e32: W 1.1e-7 ... 2.9e-7 (no shift) and up to 4.1e-6 (LM shift: the point observed once, third scaled pivot ~1e-4), S 1.0e-7 ... 2.4e-7, S x 1.0e-7 ... 4.3e-7.
Through the C ABI the device's iterations per step are the mirror's exactly: LM 5 x 150 3, 6, 7, 6, 8 and 2, 9, 9, 15, 17 (kind 1's too); costs within 7.3e-7 and 2.4e-7."""

__doc__ += "\n\n" + MEASURED

KERNEL = base.KERNEL + [((72, 500, 2500), 72)]
TABLE = base.TABLE
LM = base.LM
WS = 32                                     # THALLO_HIP_SCHUR_W_STRIDE


@pytest.fixture(scope="module")
def L(torch):
    """the library through a handle of this module's own: the entry points SchurDevice calls and the assembled form's three"""
    lib = C.CDLL(thallo_amd.lib()._name)
    S, vp, it, lg, fl = api.SumT, C.c_void_p, C.c_int, C.c_long, C.c_float
    sig = {
        "vector_elems": [lg],
        "ba_compute_j": [it] + [vp] * 9, "ba_point_order": [it, vp, vp, vp], "ba_pack_point_blocks": [it, vp, vp, vp, vp],
        "ba_pcg_init": [it, it] + [vp] * 15,
        "lm_finalize_diagonal": [vp] * 7 + [lg, fl, fl, fl, it, it, vp, vp],
        "ba_block_diag": [it, it] + [vp] * 6,
        "ba_schur_factor": [it, vp, vp, vp, vp, vp],
        "ba_schur_apply": [it, it] + [vp] * 13,
        "ba_schur_w": [it, it] + [vp] * 5,
        "ba_schur_assemble": [it, it, lg] + [vp] * 8,
        "ba_schur_apply_s": [it, lg] + [vp] * 8,
    }
    for name, args in sig.items():
        f = getattr(lib, "thallo_hip_" + name)
        f.argtypes = args
        f.restype = lg if name == "vector_elems" else it
    return lib


class Assembled:
    """One kernel instance: SchurDevice (Jb, H, CtC and both elimination factors on the device, their float32 and float64 sides), the structure of S on the device, and for
    the shifted and the unshifted system the float64 blocks and the float32 restatement -- computed once, shared by the tests, never changed"""

    def __init__(self, torch, L, dims, band, renumber):
        self.B = B = SchurDevice(torch, L, dims, band, renumber)
        self.st = st = SchurStructure(B.lists)
        i32 = lambda a: dev(torch, a, np.int32)
        self.d = dict(row_ptr=i32(st.row_ptr), col=i32(st.col), lower=i32(st.lower), term_ptr=i32(st.term_ptr), terms=i32(st.terms))
        self.B32 = cam_blocks32(B.Jb, B.lists)
        self.x = (np.random.default_rng([23, B.C]).standard_normal(B.nc) * 1e-3).astype(F32)
        self.sides = {}
        for shifted in (False, True):
            G, K, R = B.sides[shifted]
            shift = B.CtC if shifted else None
            W64, S64 = blocks64(B.Jb, B.lists, st, shift, K.held)
            W32 = w32(B.Jb, B.lists.q_pt, K.G)
            S32 = assemble32(st, W32, self.B32, shift)
            self.sides[shifted] = dict(W64=W64, S64=S64, Sx64=st.bsr(S64) @ self.x.astype(np.float64), W32=W32, S32=S32, Sx32=apply32(st, S32, self.x))

    def run(self, torch, L, shifted, gate=None, x=None):
        """W, the assembly and the apply on the device -> (W [O, 9, 3], S [nblk, 9, 9], S x, partials, their number)"""
        B, st, P = self.B, self.st, lambda k: self.d[k].data_ptr()
        G = B.sides[shifted][0]
        W = dev(torch, np.full(WS * B.O, np.nan)); S = dev(torch, np.full(81 * st.nblk, np.nan)); Sx = dev(torch, np.full(B.nc, np.nan))
        xd = dev(torch, self.x if x is None else x); part = sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
        assert L.thallo_hip_ba_schur_w(B.O, B.P, B.ptr("q_pt"), B.ptr("Jb"), G.data_ptr(), W.data_ptr(), None) == 0
        assert L.thallo_hip_ba_schur_assemble(B.C, st.nlower, st.nblk, P("lower"), P("term_ptr"), P("terms"), W.data_ptr(), B.ptr("H"), B.ptr("CtC") if shifted else None,
                                              S.data_ptr(), None) == 0
        nb = L.thallo_hip_ba_schur_apply_s(B.C, st.nblk, P("row_ptr"), P("col"), S.data_ptr(), xd.data_ptr(), Sx.data_ptr(), part.data_ptr(), gate, None)
        torch.cuda.synchronize()
        for k in self.d: host(self.d[k], 1, np.int32)                              # (the canaries behind the structure)
        assert sk.same_bytes(host(xd, B.nc), self.x if x is None else x)
        Wh = host(W, WS * B.O).reshape(B.O, WS)
        assert not Wh[:, 27].any() and np.isnan(Wh[:, 28:]).all()                  # 28 floats written per observation, the rest of the line untouched
        Sh = np.ascontiguousarray(host(S, 81 * st.nblk).reshape(9, 9, st.nblk).transpose(2, 0, 1))
        return Wh[:, :27].reshape(B.O, 9, 3).copy(), Sh, host(Sx, B.nc), part.cpu().numpy(), nb


@pytest.fixture(scope="module")
def instances(torch, L):
    cache = {}

    def get(dims, band, renumber):
        key = (dims, band, renumber)
        if key not in cache: cache[key] = Assembled(torch, L, dims, band, renumber)
        return cache[key]
    return get


CASES = [(d, b, r, s) for d, b in KERNEL for r in (False, True) for s in (False, True)]


def _bar(name, what, got, e32):
    print("schur explicit", name, what, "e32", e32, "device", got, "= %.2f e32" % (got / e32))
    assert e32 > 0 and got <= 4 * e32, (name, what, got, e32)


def _name(dims, renumber, shifted):
    return (dims, "renumbered" if renumber else "caller's order", "shift" if shifted else "no shift")


@pytest.mark.parametrize("dims,band,renumber,shifted", CASES)
def test_w_assembled_s_and_apply_against_float64(torch, L, instances, dims, band, renumber, shifted):
    """W, the stored blocks of S and S x for a random camera vector against float64 from the device's own Jb, each within 4 e32.  The x . S x partials: one per camera
    workgroup, adding up to the float64 dot of the device's x and S x within the dot bar of tests/test_gpu_ba_schur.py.  The stored S is symmetric bit for bit -- block
    (i, j) is the transpose of (j, i), a diagonal block its own -- and a second run of the three launches gives the same bits."""
    A = instances(dims, band, renumber)
    B, st, ref = A.B, A.st, A.sides[shifted]
    if dims == (72, 500, 2500): assert np.diff(st.row_ptr)[:-1].min() <= 64 < np.diff(st.row_ptr).max() and np.diff(st.row_ptr)[-1] == 1
    if dims == (3, 160, 480): assert np.diff(st.term_ptr).max() > 64
    W, S, Sx, part, nb = A.run(torch, L, shifted)
    name = _name(dims, renumber, shifted)
    _bar(name, "W", rel_max(W, ref["W64"]), rel_max(ref["W32"], ref["W64"]))
    _bar(name, "S", rel_max(S, ref["S64"]), rel_max(ref["S32"], ref["S64"]))
    _bar(name, "apply", rel_max(Sx, ref["Sx64"]), rel_max(ref["Sx32"], ref["Sx64"]))
    assert sk.same_bytes(S[st.lower[:, 1]], np.transpose(S[st.lower[:, 0]], (0, 2, 1)))
    grid = (B.C + 3) // 4
    assert nb == grid and sk.written_slots(part) == grid
    t = A.x.astype(np.float64) * Sx
    assert abs(part[:grid].astype(np.float64).sum() - t.sum()) <= 13 * sk.EPS * np.abs(t).sum()
    again = A.run(torch, L, shifted)
    for a, b in zip((W, S, Sx, part), again[:4]): assert sk.same_bytes(a, b)


def test_a_set_gate_word_leaves_every_output_as_it_was(torch, L, instances):
    dims, band = KERNEL[0]
    A = instances(dims, band, False)
    B, st, P = A.B, A.st, lambda k: A.d[k].data_ptr()
    rng = np.random.default_rng(13)
    s0 = rng.standard_normal(B.nc).astype(F32)
    S = dev(torch, A.sides[True]["S32"].transpose(1, 2, 0).ravel())
    for gated in (True, False):
        Sx, xd, part = dev(torch, s0), dev(torch, A.x), sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
        gate = sk.dbuf(torch, np.array([1 if gated else 0, 0], np.uint32))
        nb = L.thallo_hip_ba_schur_apply_s(B.C, st.nblk, P("row_ptr"), P("col"), S.data_ptr(), xd.data_ptr(), Sx.data_ptr(), part.data_ptr(), gate.data_ptr(), None)
        torch.cuda.synchronize()
        assert nb == (B.C + 3) // 4
        same = sk.same_bytes(host(Sx, B.nc), s0) and sk.written_slots(part.cpu().numpy()) == 0
        assert same == gated and sk.same_bytes(host(xd, B.nc), A.x)
        host(S, 81 * st.nblk)
        if not gated: assert rel_max(host(Sx, B.nc), A.sides[True]["Sx64"]) < 1e-5


@pytest.mark.parametrize("dims,band", KERNEL[:2])
@pytest.mark.parametrize("renumber", [False, True])
def test_held_points_contribute_nothing(torch, L, instances, dims, band, renumber):
    """GN (no shift): the point observed once is held (the restatement's count and places equal the device's: checked where SchurDevice makes the factor), so its
    observation's W is exactly zero and its one term adds nothing to S -- the float64 S of the first test drops the held points' rows and columns; the camera nothing
    observes has a zero row, so its S x is 0"""
    A = instances(dims, band, renumber)
    B, st = A.B, A.st
    K = B.sides[False][1]
    W, S, Sx, _, _ = A.run(torch, L, False)
    once = np.nonzero(np.diff(B.lists.pt_ptr) == 1)[0]
    assert len(once) == 1 and K.held[once[0]] and int(K.held.sum()) == 2
    q = B.lists.pt_pos[B.lists.pt_ptr[once[0]]]
    assert not W[q].any() and W[B.lists.q_pt != once[0]].any()
    assert ((st.terms[:, 0] == q) | (st.terms[:, 1] == q)).sum() == 1                 # its one term, (q, q), adds W_q W_q^T = 0 to camera 0's diagonal block
    assert not S[st.row_ptr[-2]:].any() and not Sx[-9:].any()


@pytest.mark.parametrize("dims,band,renumber,shifted", CASES)
def test_assembled_apply_against_the_matrix_free_apply(torch, L, instances, dims, band, renumber, shifted):
    """the assembled S x and thallo_hip_ba_schur_apply's on the same x: apart by no more than the sum of their two bars, 4 e32 each (of max |S x|)"""
    A = instances(dims, band, renumber)
    B = A.B
    G, K, R = B.sides[shifted]
    _, _, Sx, _, _ = A.run(torch, L, shifted)
    U, xd, Sx1, part = dev(torch, np.full(2 * B.O, np.nan)), dev(torch, A.x), dev(torch, np.full(B.nc, np.nan)), sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
    assert L.thallo_hip_ba_schur_apply(*B.lists_args(), G.data_ptr(), xd.data_ptr(), B.ptr("CtC") if shifted else None, U.data_ptr(), Sx1.data_ptr(), part.data_ptr(), None, None) > 0
    torch.cuda.synchronize()
    Sx1 = host(Sx1, B.nc)
    ref = A.sides[shifted]["Sx64"]
    e_free, e_asm = rel_max(K.apply(A.x), R.apply(A.x)), rel_max(A.sides[shifted]["Sx32"], ref)
    got = rel_max(Sx, Sx1.astype(np.float64)) * np.abs(Sx1).max() / np.abs(ref).max()
    print("schur explicit", _name(dims, renumber, shifted), "assembled vs matrix-free", got, "e32 matrix-free", e_free, "assembled", e_asm, "= %.2f of the bar" % (got / (4 * (e_free + e_asm))))
    assert rel_max(R.apply(A.x), ref) <= 1e-9                                # the two float64 sides are one matrix
    assert got <= 4 * e_free + 4 * e_asm


# ------------------------------------------------------------------ through the C ABI
def run(dims, p, lm, solver=None, back=False, **sp):
    """-> (costs, PCG iterations per step, held points after every step, fallbacks after every step, cameras, points, schedule name, schur_blocks() after Init)"""
    d = to_device(copy_params(p))
    s = api.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), solverkind="levenberg_marquardt" if lm else "gauss_newton")
    if lm: s.enable_lm()
    if solver: s.set_linear_solver(solver)
    if back: s.set_linear_solver("pcg")
    s.set_solver_parameters(**sp)
    params = s.make_params(d)
    assert s.schur_blocks() == -1
    s.init(params)
    blocks = s.schur_blocks()
    costs, iters, held, fb = [s.current_cost()], [], [], []
    while s.step(params):
        costs.append(s.current_cost()); iters.append(len(s.alpha_beta_trace())); held.append(s.schur_held_points()); fb.append(s.preconditioner_fallbacks())
    name = s.schedule_name
    s.close()
    return np.array(costs), iters, held, fb, to_host(d[0]).copy(), to_host(d[1]).copy(), name, blocks


@pytest.mark.parametrize("dims,band", TABLE)
def test_lm_assembled_through_the_c_abi(torch, orc, dims, band):
    """LM 5 x 150 (q_tolerance 0.1, function_tolerance 0): costs per step the assembled mirror's within max(1e-5, 3 err_jacobi), err_jacobi the default path's distance from
    the oracle's LM on the same instance; iterations per step the mirror's up to a summed difference of 2 (tests/test_gpu_ba_schur.py's bars); no more iterations in total
    than kind 1; no held point and no fallback; schur_blocks() is the brute-force count and the schedule name carries it."""
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    cm, im = BaSchurExplicitMirror(dims, p).lm_solve(5, 150, q_tolerance=0.1, function_tolerance=0.0)
    co, _ = orc.Problem(orc.BUNDLE_ADJUST, dims, copy_params(p)).solve(use_lm=1, **LM)
    cj, ij, hj, _, _, _, _, bj = run(dims, p, True, **LM)
    c1, i1, _, _, _, _, n1, b1 = run(dims, p, True, solver="schur_pcg", **LM)
    cs, is_, hs, fs, _, _, name, blocks = run(dims, p, True, solver="schur_explicit_pcg", **LM)
    err_j, err = rel(cj, co), rel(cs, cm)
    print("LM", dims, "assembled", is_, list(cs), "mirror", im, cm, "kind 1", i1, list(c1), "jacobi", ij, "err_jacobi", err_j.max(), "err", err.max(), name)
    want = brute_force_counts(p[3], p[4], dims[0])[2]
    assert blocks == want and bj == -1 and b1 == -1 and "assembled" not in n1
    assert "Schur complement on the cameras, assembled (%d blocks); block-Jacobi on S" % want in name and hj == [-1] * len(hj)
    assert len(is_) == 5 and len(cs) == len(cm)
    assert err.max() <= max(1e-5, 3 * err_j.max())
    assert sum(abs(a - b) for a, b in zip(is_, im)) <= 2, (is_, im)
    assert sum(is_) <= sum(i1) + 2, (is_, i1)
    assert hs == [0] * 5 and fs == [0] * 5


@pytest.mark.parametrize("dims,band", TABLE)
def test_gn_assembled_through_the_c_abi(torch, orc, dims, band):
    """GN 4 x 10: costs per step the assembled mirror's within the LM test's self-calibrated bar, exactly 10 iterations per step"""
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    cm = BaSchurExplicitMirror(dims, p).gn_solve(4, 10)
    co, _ = orc.Problem(orc.BUNDLE_ADJUST, dims, copy_params(p)).solve(nIterations=4, lIterations=10)
    cj, *_ = run(dims, p, False, nIterations=4, lIterations=10)
    cs, is_, hs, fs, *_ = run(dims, p, False, solver="schur_explicit_pcg", nIterations=4, lIterations=10)
    err_j, err = rel(cj, co), rel(cs, cm)
    print("GN", dims, "assembled 4x10", list(cs), "mirror", cm, "err_jacobi", err_j.max(), "err", err.max())
    assert len(cs) == 5 and is_ == [10] * 4 and hs == [0] * 4 and fs == [0] * 4
    assert err.max() <= max(1e-5, 3 * err_j.max())


@pytest.mark.parametrize("dims,band", KERNEL[:2])
def test_held_points_keep_their_bits_through_a_gn_step(torch, dims, band):
    """the instance with its extras, one GN step of 10 iterations: the held count is the mirror's (the point nothing observes and the point observed once), their rows of
    `points` are bit-unchanged, the camera nothing observes stays where it was (one fallback); in both point orders"""
    p, d3 = with_extras(syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band))
    m = BaSchurExplicitMirror(d3, p); m.gn_step(10)
    want = brute_force_counts(p[3], p[4], d3[0])[2]
    for ren in ("0", "1"):
        with pytest.MonkeyPatch.context() as mp:
            set_ab(mp, ba_renumber=ren)
            cs, is_, hs, fs, cams, pts, name, blocks = run(d3, p, False, solver="schur_explicit_pcg", nIterations=1, lIterations=10)
        assert hs == m.held == [2] and fs == [1] and is_ == [10] and blocks == want
        assert pts[-2:].tobytes() == p[1][-2:].tobytes() and cams[-1].tobytes() == p[0][-1].tobytes()
        assert (pts[:-2] != p[1][:-2]).any() and cs[1] < cs[0]
        assert abs(cs[1] - float(m.cost())) <= 1e-4 * cs[1]


@pytest.mark.parametrize("lm", [False, True])
def test_assembled_then_pcg_before_init_is_the_default_plan_bit_for_bit(torch, lm):
    dims, band = TABLE[0]
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    sp = dict(nIterations=3, lIterations=25, q_tolerance=0.02) if lm else dict(nIterations=3, lIterations=10)
    a = run(dims, p, lm, **sp)
    b = run(dims, p, lm, solver="schur_explicit_pcg", back=True, **sp)
    assert list(a[0]) == list(b[0]) and a[1] == b[1] and a[6] == b[6] and b[2] == [-1] * len(b[2]) and b[7] == -1
    assert sk.same_bytes(a[4], b[4]) and sk.same_bytes(a[5], b[5])


def test_renumbered_plan_runs_the_same_assembled_solve(torch, monkeypatch):
    """the plan-side point order (THALLO_AB=ba_renumber=1): the structure is built in the plan's internal ids -- the same blocks, the same iterations (summed difference
    <= 2), costs to 1e-5"""
    dims, band = TABLE[0]
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    set_ab(monkeypatch, ba_renumber="0")
    c0, i0, h0, f0, _, _, n0, b0 = run(dims, p, True, solver="schur_explicit_pcg", **LM)
    set_ab(monkeypatch, ba_renumber="1")
    c1, i1, h1, f1, _, _, n1, b1 = run(dims, p, True, solver="schur_explicit_pcg", **LM)
    assert "renumbered" in n1 and "renumbered" not in n0 and b0 == b1 == brute_force_counts(p[3], p[4], dims[0])[2]
    assert len(i0) == len(i1) and sum(abs(a - b) for a, b in zip(i0, i1)) <= 2 and h1 == [0] * len(h1) and f1 == [0] * len(f1)
    assert rel(c1, c0).max() <= 1e-5


def test_a_reinit_with_another_kind_switches_the_apply(torch):
    """kind 2, Init, a step; kind 1, re-Init: the matrix-free apply runs again (schur_blocks() -1) and the step's cost is kind 2's to 1e-5"""
    dims, band = TABLE[0]
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    costs = []
    d = to_device(copy_params(p))
    s = api.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"))
    s.set_solver_parameters(nIterations=1, lIterations=10)
    params = s.make_params(d)
    for kind, blocks in (("schur_explicit_pcg", True), ("schur_pcg", False), ("schur_explicit_pcg", True)):
        for t, a in zip(d[:2], p[:2]): t.copy_(torch.from_numpy(a.copy()))
        s.set_linear_solver(kind)
        s.init(params)
        assert (s.schur_blocks() > 0) == blocks and ("assembled" in s.schedule_name) == blocks
        while s.step(params): pass
        costs.append(s.current_cost())
    s.close()
    assert costs[0] == costs[2] and abs(costs[1] - costs[0]) <= 1e-5 * costs[0]


def test_refusals_name_the_energy(torch, monkeypatch, tmp_path):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energies")
    cases = [((48, 32), thallo_amd.energy_file("image_warping"), False),              # another hand-written energy
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), False),          # a generated one
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), True)]           # doublePrecision = 1
    for dims, f, dbl in cases:
        s = api.ThalloSolver(dims, f, double_precision=dbl)
        assert s.schur_blocks() == -1
        assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 2) != 0
        assert s.energy_name and s.energy_name in api.last_error() and "assembled" in api.last_error(), api.last_error()
        with pytest.raises(RuntimeError): s.set_linear_solver("schur_explicit_pcg")
        assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 0) == 0 and s.schur_blocks() == -1
        s.close()
    s = api.ThalloSolver((5, 72, 330), thallo_amd.energy_file("bundle_adjustment"), double_precision=True)
    assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 2) != 0 and "bundle_adjustment" in api.last_error() and "doublePrecision" in api.last_error() and "assembled" in api.last_error()
    s.close()
    s = api.ThalloSolver((5, 72, 330), thallo_amd.energy_file("bundle_adjustment"))
    s.set_linear_solver("schur_explicit_pcg")
    with pytest.raises(RuntimeError, match="bundle_adjustment.*assembled"):          # a distributed plan: the linear solver first ...
        s.set_distributed(0, 1, 0, 0, device_exchange=False)
    s.close()
    s = api.ThalloSolver((8, 72, 330), thallo_amd.energy_file("bundle_adjustment"))      # ... and the distribution first (one rank's camera shard)
    s.set_distributed(0, 1, 0, 0, device_exchange=False)
    with pytest.raises(RuntimeError, match="bundle_adjustment.*assembled"):
        s.set_linear_solver("schur_explicit_pcg")
    s.close()
    # a direct-solve plan (tests/test_gpu_frontend.py::test_direct_solve_is_opt_in_like_the_reference's)
    lines = "".join(f"r.{n}.J:set_materialize(true)\nr.{n}.JtJ:set_materialize(true)\n" for n in ("fit", "reg")) + "r:set_direct_solve(true)\n"
    f = tmp_path / "laplacian_direct.t"
    f.write_text(open(thallo_amd.energy_file("laplacian_graph")).read() + "\n" + lines)
    monkeypatch.setenv("THALLO_FRONTEND", "generate"); monkeypatch.setenv("THALLO_ENABLE_DIRECT_SOLVE", "1")
    s = api.ThalloSolver((256, 255), str(f))
    assert s.schedule_name == "dense direct solve"
    assert s._L.ThalloX_PlanSetLinearSolver(s.plan, 2) != 0
    assert s.energy_name and s.energy_name in api.last_error() and "direct-solve" in api.last_error() and "assembled" in api.last_error(), api.last_error()
    s.close()


def test_a_structure_over_the_budget_fails_init_and_names_the_bytes(torch, monkeypatch):
    """THALLO_AB=schur_s_max_mb=0: Init fails (no silent fall-back to kind 1), the message names the bytes wanted and the bytes allowed; with 1 MiB the small instance fits,
    and the bytes it names one byte short of are the builder's count"""
    dims, band = KERNEL[0]
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    st = SchurStructure(SchurLists(p[3], p[4], dims[0], dims[1]))
    for mb, ok in (("0", False), ("1", True)):
        set_ab(monkeypatch, schur_s_max_mb=mb)
        d = to_device(copy_params(p))
        s = api.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"))
        s.set_linear_solver("schur_explicit_pcg")
        s.set_solver_parameters(nIterations=1, lIterations=5)
        params = s.make_params(d)
        if ok:
            s.init(params)
            assert s.schur_blocks() == st.nblk and st.bytes(dims[2]) <= 1 << 20
            assert s.ready()
            s.step(params)
            assert s.schur_held_points() == 0
        else:
            s.init(params)
            msg = api.last_error()
            print(msg)
            assert "budget allows 0" in msg and "schur_s_max_mb" in msg and "bytes" in msg and "bundle_adjustment" in msg
            assert s.schur_blocks() == -1 and not s.ready() and not s.step(params)
        s.close()
