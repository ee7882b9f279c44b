"""Marginal covariances of bundle adjustment's cameras and points (csrc/ba_covariance.hip, ThalloX_PlanCovariance): the kernels through their exported symbols against
float64 from the device's own S, W and G, the batch driver against float64 inv(S_FF) of the device's own S, then the C call on Gauss-Newton and Levenberg-Marquardt
plans against the float64 (A_FF)^-1 of the oracle's J at the device's unknowns (tests/ba_covariance_mirror.py), the hold rule, the NaN blocks, the untouched solve, the
refusals.

Kernel instances: tests/test_gpu_ba_schur.py's SchurDevice -- (5, 72, 330) band 5 and (3, 160, 480) band 3 -- and (24, 300, 1200) band 12, each with its extras (a camera
and a point nothing observes, a point observed once), in the caller's point order and in the plan's renumbered order, no LM shift.  The gauge is held as camera 0 entirely
plus scalar 3 of camera 1: thallo_hip_block_hold on H, the two factors, thallo_hip_block_hold_factor, W and the assembly as Plan::forms_setup launches them.

Bars.  A single operation: 4 e32, e32 the distance from float64 of the float32 restatement in the kernels' order (ColumnPCG32) on the same device data, recomputed in
the run; measure max |err| / max |value|.  A covariance: 4 x the restatement's own error against the same float64 reference on the same instance, in the measure
max |Sigma - Sigma_ref|_ab / sqrt(Sigma_ref,aa Sigma_ref,bb) over the free scalars of the requested blocks, held rows and columns compared exactly.  The margin is for
two correct float32 evaluations in different association orders (the device fuses its multiply-adds).  No absolute number is fixed.

MEASURED below is part of this docstring."""
import ctypes as C
import os

import numpy as np
import pytest

import shim_kernels as sk
import test_gpu_block_precond as bp
import thallo_amd
from shim_kernels import EPS, F32
from thallo_amd import api, synthetic as syn

import ba_covariance_mirror as cm
import test_gpu_ba_schur as base
from test_gpu_ba_schur import SchurDevice, dev, host, torch      # noqa: F401  (torch: the module fixture)
from ba_block_mirror import BaBlockMirror
from ba_robust_mirror import robust
from ba_schur_explicit_mirror import SchurStructure, apply32
from ba_schur_mirror import rel_max, with_extras
from helpers import copy_params, set_ab, to_device, to_host

pytestmark = pytest.mark.gpu

MEASURED = """Measured on an MI355X (the tests print every figure before they assert; also in profiles/ba_covariance/README.md):
  single operations, multiples of e32 (bar 4): right-hand sides 0.21 - 1.00, S X on a panel 1.00 - 1.08, G^T G R 0.91 - 1.00, output contraction 0.61 - 1.07;
  e32: 3.7e-8 ... 1.0e-7 (rhs), 1.5e-7 ... 4.9e-7 (S X), 7e-8 ... 1.6e-7 (G^T G R), 8.9e-8 ... 1.7e-7 (output).
  x . S x partials 0.08 - 0.32 of their bar; a panel's column against the one-column apply 0.10 - 0.33 of the summed bars.
  driver against float64 inv(S_FF) of the device's own S, multiples of the restatement's error (bar 4): cameras 0.64 - 1.56 (restatement 5.4e-6 ... 1.2e-5), points
  0.45 - 1.34 (2.3e-6 ... 3.4e-6); 24 - 72 iterations where the restatement freezes its last column after 18 - 65 (chunks of 8); the 1030-camera chain 1.00.
  through the C ABI against the float64 (A_FF)^-1 of the oracle's J, 24 cases each: cameras 0.39 - 3.19 (restatement 3.4e-5 ... 2.2e-4), points 0.22 - 3.32
  (9.0e-6 ... 6.1e-5) -- THE LARGEST MULTIPLE IS 3.32 ((5, 72, 330) with its extras, GN, caller's order, squared loss, points); here the device linearises by itself, so
  the difference of its float32 J from the oracle's is in the multiple as well."""

__doc__ += "\n\n" + MEASURED

K = cm.K
KERNEL = base.KERNEL + [((24, 300, 1200), 12)]
CASES = [(d, b, r) for d, b in KERNEL for r in (False, True)]


class SysT(C.Structure):                    # thallo_cov_sys_t
    _fields_ = [("C", C.c_int), ("P", C.c_int), ("nblk", C.c_long), ("row_ptr", C.c_void_p), ("col", C.c_void_p), ("S", C.c_void_p), ("Gc", C.c_void_p), ("Ge", C.c_void_p),
                ("W", C.c_void_p), ("pt_ptr", C.c_void_p), ("pt_pos", C.c_void_p), ("q_cam", C.c_void_p), ("hold", C.c_void_p)]


class InfoT(C.Structure):                   # thallo_cov_info_t
    _fields_ = [("iterations", C.c_int), ("columns", C.c_int), ("not_converged", C.c_int), ("nan_blocks", C.c_int), ("worst", C.c_float)]


@pytest.fixture(scope="module")
def L(torch):
    lib = C.CDLL(thallo_amd.lib()._name)
    vp, it, lg, fl = C.c_void_p, C.c_int, C.c_long, C.c_float
    R, sp = bp.RegionsT, C.POINTER(SysT)
    sig = {
        "vector_elems": [lg],
        "ba_compute_j": [it] + [vp] * 9, "ba_point_order": [it, vp, vp, vp], "ba_pack_point_blocks": [it, vp, vp, vp, vp],
        "ba_pcg_init": [it, it] + [vp] * 15,
        "lm_finalize_diagonal": [vp] * 7 + [lg, fl, fl, fl, it, it, vp, vp],
        "ba_block_diag": [it, it] + [vp] * 6,
        "ba_schur_factor": [it, vp, vp, vp, vp, vp],
        "block_factor": [R] + [vp] * 6, "block_hold": [R, vp, vp, vp], "block_hold_factor": [R, vp, vp, vp],
        "ba_schur_w": [it, it] + [vp] * 5,
        "ba_schur_assemble": [it, it, lg] + [vp] * 8,
        "ba_schur_apply_s": [it, lg] + [vp] * 8,
        "ba_cov_work_bytes": [it],
        "ba_cov_rhs": [sp, it, vp, it, vp, vp],
        "ba_schur_apply_s_cols": [it, lg] + [vp] * 7,
        "ba_cov_precond_cols": [it] + [vp] * 5,
        "ba_cov_out": [sp, it, vp, it, vp, vp, vp, vp],
        "ba_cov_solve": [sp, it, vp, it, fl, it, vp, vp, vp, C.POINTER(InfoT), vp],
    }
    for name, args in sig.items():
        f = getattr(lib, "thallo_hip_" + name)
        f.argtypes = args
        f.restype = lg if name in ("vector_elems", "ba_cov_work_bytes") else it
    return lib


def tri_unpack(flat, n, cnt):
    """the packed planes of a lower-triangular factor -> [cnt, n, n] (zeros above the diagonal)"""
    G = np.zeros((cnt, n, n), flat.dtype)
    k = 0
    for i in range(n):
        for j in range(i + 1):
            G[:, i, j] = flat[k * cnt:(k + 1) * cnt]; k += 1
    return G


class CovDevice:
    """SchurDevice + the gauge: the held H, both factors, W and the assembled S on the device as a GN step's set-up leaves them; their host copies; the float32
    restatement on exactly those numbers and the float64 sides.  Computed once, shared by the tests, never changed"""

    def __init__(self, torch, L, dims, band, renumber):
        self.B = B = SchurDevice(torch, L, dims, band, renumber)
        self.C, self.P, self.O = C_, P_, O_ = B.C, B.P, B.O
        self.st = st = SchurStructure(B.lists)
        self.mask = cm.gauge_mask(C_, P_)
        i32 = lambda a: dev(torch, a, np.int32)
        m8 = np.zeros((B.n + 3) // 4 * 4, np.uint8); m8[:B.n] = self.mask
        self.d = d = dict(row_ptr=i32(st.row_ptr), col=i32(st.col), lower=i32(st.lower), term_ptr=i32(st.term_ptr), terms=i32(st.terms), mask=dev(torch, m8.view(np.uint32), np.uint32),
                          H=dev(torch, host(B.d["H"], 45 * C_ + 6 * P_)), Gc=dev(torch, np.full(45 * C_, np.nan)), Ge=dev(torch, np.full(6 * P_, np.nan)),
                          W=dev(torch, np.full(32 * O_, np.nan)), S=dev(torch, np.full(81 * st.nblk, np.nan)), status=dev(torch, np.zeros(2, np.uint32), np.uint32))
        P = lambda k: d[k].data_ptr()
        both, cams, pts = bp.regions(C_, P_), bp.regions(C_, P_), bp.regions(C_, P_)
        cams.n = 1; pts.r[0] = pts.r[1]; pts.n = 1
        assert L.thallo_hip_block_hold(both, P("mask"), P("H"), None) == 0
        assert L.thallo_hip_block_factor(cams, P("H"), None, B.ptr("pre"), P("Gc"), P("status"), None) == 0
        assert L.thallo_hip_block_hold_factor(cams, P("mask"), P("Gc"), None) == 0
        assert L.thallo_hip_ba_schur_factor(P_, P("H") + 4 * 45 * C_, None, P("Ge"), P("status") + 4, None) == 0
        assert L.thallo_hip_block_hold_factor(pts, P("mask"), P("Ge"), None) == 0
        assert L.thallo_hip_ba_schur_w(O_, P_, B.ptr("q_pt"), B.ptr("Jb"), P("Ge"), P("W"), None) == 0
        assert L.thallo_hip_ba_schur_assemble(C_, st.nlower, st.nblk, P("lower"), P("term_ptr"), P("terms"), P("W"), P("H"), None, P("S"), None) == 0
        torch.cuda.synchronize()
        self.S = np.ascontiguousarray(host(d["S"], 81 * st.nblk).reshape(9, 9, st.nblk).transpose(2, 0, 1))
        self.Gc = tri_unpack(host(d["Gc"], 45 * C_), 9, C_); self.Ge = tri_unpack(host(d["Ge"], 6 * P_), 3, P_)
        self.W = host(d["W"], 32 * O_).reshape(O_, 32)[:, :27].reshape(O_, 9, 3).copy()
        assert int(host(d["status"], 2, np.uint32)[1]) == 2 and int((~self.Ge.any((1, 2))).sum()) == 2      # the point nothing observes and the point observed once
        self.pcg = cm.ColumnPCG32(st, self.S, self.Gc, self.Ge, self.W, B.lists, self.mask)
        self.sys = SysT(C_, P_, st.nblk, P("row_ptr"), P("col"), P("S"), P("Gc"), P("Ge"), P("W"), B.ptr("pt_ptr"), B.ptr("pt_pos"), B.ptr("q_cam"), P("mask"))
        self.S64 = st.bsr(self.S).toarray()
        self.free_c = ~self.mask[:9 * C_]
        self.free_c[9 * (C_ - 1):] = False                                       # the camera nothing observes: S has a zero row there
        self.Sig_cc = cm.inv_s_ff64(self.S64, self.free_c)
        self.cams = list(range(min(C_ - 1, 7)))
        old = np.argsort(B.lists.new2old)                                        # the caller's point -> the plan's
        self.pts = [int(old[p]) for p in list(range(0, P_ - 2, max(1, P_ // 21)))[:19] + [P_ - 2, P_ - 1]]
        self.work = torch.zeros(int(L.thallo_hip_ba_cov_work_bytes(C_)) // 4 + 64, dtype=torch.float32, device="cuda")

    def ids(self, torch, mode):
        return dev(torch, self.cams if mode == 0 else self.pts, np.int32)

    def panel(self, a):
        """[C, 9, K] <-> the device's [9 C][K]"""
        return np.ascontiguousarray(a, F32).reshape(9 * self.C * K)

    def solve(self, torch, L, mode, ids, rel_tol=1e-6, max_it=500):
        idd, out, info = dev(torch, ids, np.int32), dev(torch, np.full(len(ids) * (81 if mode == 0 else 9), np.nan)), InfoT()
        rc = L.thallo_hip_ba_cov_solve(C.byref(self.sys), mode, idd.data_ptr(), len(ids), rel_tol, max_it, self.work.data_ptr(), None, out.data_ptr(), C.byref(info), None)
        assert rc == 0, rc
        d = 9 if mode == 0 else 3
        return host(out, len(ids) * d * d).reshape(len(ids), d, d), info


@pytest.fixture(scope="module")
def instances(torch, L):
    cache = {}

    def get(dims, band, renumber):
        key = (dims, renumber)
        if key not in cache: cache[key] = CovDevice(torch, L, dims, band, renumber)
        return cache[key]
    return get


def _bar(name, what, got, e32):
    print("covariance", name, what, "e32", e32, "device", got, "= %.2f e32" % (got / e32 if e32 > 0 else np.inf))
    assert e32 > 0 and got <= 4 * e32, (name, what, got, e32)


def _name(dims, renumber):
    return (dims, "renumbered" if renumber else "caller's order")


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("dims,band,renumber", CASES)
def test_right_hand_sides(torch, L, instances, dims, band, renumber):
    """a camera batch: the unit columns exactly, every other word of the panel zero; a point batch: W_q G_p in the rows of c(q) against float64 from the device's own W and
    G within 4 e32, the columns of the two held points exactly zero"""
    A = instances(dims, band, renumber)
    R = dev(torch, np.full(9 * A.C * K, np.nan))
    idd = A.ids(torch, 0)
    assert L.thallo_hip_ba_cov_rhs(C.byref(A.sys), 0, idd.data_ptr(), len(A.cams), R.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert sk.same_bytes(host(R, 9 * A.C * K), A.panel(A.pcg.rhs(0, A.cams)))
    idd = A.ids(torch, 1)
    assert L.thallo_hip_ba_cov_rhs(C.byref(A.sys), 1, idd.data_ptr(), len(A.pts), R.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = host(R, 9 * A.C * K).reshape(A.C, 9, K)
    ref = np.zeros((A.C, 9, K))
    for j, p in enumerate(A.pts):
        for q, c in A.pcg._list(p): ref[c, :, 3 * j:3 * j + 3] += A.W[q].astype(np.float64) @ A.Ge[p].astype(np.float64)
    _bar(_name(dims, renumber), "rhs", rel_max(got, ref), rel_max(A.pcg.rhs(1, A.pts), ref))
    assert not got[:, :, 3 * 19:].any() and not got[:, :, :3 * 19][ref[:, :, :3 * 19] == 0].any()


@pytest.mark.parametrize("dims,band,renumber", CASES)
def test_apply_s_on_a_panel_and_its_partials(torch, L, instances, dims, band, renumber):
    """Y = S X for a random panel against float64 from the device's own S within 4 e32; the partials: one per camera row and column, adding up per column to the float64
    dot of the device's x and S x within 10 u sum |terms| (nine fused additions behind a partial); column k of Y against thallo_hip_ba_schur_apply_s on column k alone
    within the sum of the two bars; the canaries behind every buffer intact; a second launch gives the same bits"""
    A = instances(dims, band, renumber)
    X = (np.random.default_rng([31, A.C]).standard_normal((A.C, 9, K)) * 1e-3).astype(F32)
    P = lambda k: A.d[k].data_ptr()
    runs = []
    for _ in range(2):
        Xd, Y, part = dev(torch, A.panel(X)), dev(torch, np.full(9 * A.C * K, np.nan)), sk.canary_buf(torch, (A.C + 2) * K)
        nb = L.thallo_hip_ba_schur_apply_s_cols(A.C, A.st.nblk, P("row_ptr"), P("col"), P("S"), Xd.data_ptr(), Y.data_ptr(), part.data_ptr(), None)
        torch.cuda.synchronize()
        assert nb == A.C and sk.same_bytes(host(Xd, 9 * A.C * K), A.panel(X))
        ph = part.cpu().numpy().reshape(-1, K)
        assert sk.written_slots(ph) == A.C
        runs.append((host(Y, 9 * A.C * K).reshape(A.C, 9, K), ph[:A.C].copy()))
    for k in A.d: host(A.d[k], 1, np.uint32)
    (Y, part), again = runs
    assert sk.same_bytes(Y, again[0]) and sk.same_bytes(part, again[1])
    ref = (A.S64 @ X.reshape(9 * A.C, K).astype(np.float64)).reshape(A.C, 9, K)
    Y32, _ = A.pcg.apply(X)
    e_cols = rel_max(Y32, ref)
    _bar(_name(dims, renumber), "S X", rel_max(Y, ref), e_cols)
    t = X.astype(np.float64) * Y
    err = np.abs(part.astype(np.float64).sum(0) - t.sum((0, 1)))
    print("covariance", _name(dims, renumber), "x . S x partials: worst error / bar", (err / (10 * EPS * np.abs(t).sum((0, 1)))).max())
    assert (err <= 10 * EPS * np.abs(t).sum((0, 1))).all()
    for k in (0, 17, K - 1):
        xk = np.ascontiguousarray(X[:, :, k]).ravel()
        xd, Sx, p1 = dev(torch, xk), dev(torch, np.full(9 * A.C, np.nan)), sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
        assert L.thallo_hip_ba_schur_apply_s(A.C, A.st.nblk, P("row_ptr"), P("col"), P("S"), xd.data_ptr(), Sx.data_ptr(), p1.data_ptr(), None, None) > 0
        torch.cuda.synchronize()
        one = host(Sx, 9 * A.C); rk = ref[:, :, k].ravel()
        e_one = rel_max(apply32(A.st, A.S, xk), rk)
        ek_cols = rel_max(Y32[:, :, k].ravel(), rk)
        got = float(np.abs(Y[:, :, k].ravel().astype(np.float64) - one).max() / np.abs(rk).max())
        print("covariance", _name(dims, renumber), "column", k, "panel vs one-column apply", got, "= %.2f of the summed bars" % (got / (4 * (e_one + ek_cols))))
        assert got <= 4 * e_one + 4 * ek_cols


@pytest.mark.parametrize("dims,band,renumber", CASES)
def test_block_preconditioner_on_a_panel(torch, L, instances, dims, band, renumber):
    """Z = G^T G R per camera and column against float64 from the device's own G within 4 e32; rows of held scalars exactly zero; the partials of r . z within the dot bar"""
    A = instances(dims, band, renumber)
    R = np.random.default_rng([37, A.C]).standard_normal((A.C, 9, K)).astype(F32)
    Rd, Z, part = dev(torch, A.panel(R)), dev(torch, np.full(9 * A.C * K, np.nan)), sk.canary_buf(torch, (A.C + 2) * K)
    nb = L.thallo_hip_ba_cov_precond_cols(A.C, A.d["Gc"].data_ptr(), Rd.data_ptr(), Z.data_ptr(), part.data_ptr(), None)
    torch.cuda.synchronize()
    ph = part.cpu().numpy().reshape(-1, K)
    assert nb == A.C and sk.written_slots(ph) == A.C and sk.same_bytes(host(Rd, 9 * A.C * K), A.panel(R))
    Zh = host(Z, 9 * A.C * K).reshape(A.C, 9, K)
    G = A.Gc.astype(np.float64)
    ref = np.einsum("cki,ckj,cjn->cin", G, G, R.astype(np.float64))
    _bar(_name(dims, renumber), "G^T G R", rel_max(Zh, ref), rel_max(A.pcg.precond(R)[0], ref))
    assert not Zh.reshape(9 * A.C, K)[A.mask[:9 * A.C]].any()
    t = R.astype(np.float64) * Zh
    assert (np.abs(ph[:A.C].astype(np.float64).sum(0) - t.sum((0, 1))) <= 10 * EPS * np.abs(t).sum((0, 1))).all()


@pytest.mark.parametrize("dims,band,renumber", CASES)
def test_output_contraction(torch, L, instances, dims, band, renumber):
    """from a random panel: a camera's 0.5 (X_ii + X_ii^T) and a point's G^T G + sum_q (W_q G)^T X_c(q), symmetrised, against float64 from the device's own W and G within
    4 e32; bitwise symmetric; the two points the factor rule holds are NaN and counted, once each"""
    A = instances(dims, band, renumber)
    X = np.random.default_rng([41, A.C]).standard_normal((A.C, 9, K)).astype(F32)
    Xd = dev(torch, A.panel(X))
    for mode, ids, d in ((0, A.cams, 9), (1, A.pts, 3)):
        idd, out, cnt = A.ids(torch, mode), dev(torch, np.full(len(ids) * d * d, np.nan)), dev(torch, np.array([5, 0], np.uint32), np.uint32)
        assert L.thallo_hip_ba_cov_out(C.byref(A.sys), mode, idd.data_ptr(), len(ids), Xd.data_ptr(), out.data_ptr(), cnt.data_ptr(), None) == 0
        torch.cuda.synchronize()
        got = host(out, len(ids) * d * d).reshape(len(ids), d, d)
        m32, nans = A.pcg.out(mode, ids, X)
        ok = ~np.isnan(m32[:, 0, 0])
        assert int(host(cnt, 2, np.uint32)[0]) == 5 + nans and nans == (2 if mode else 0) and (np.isnan(got[:, 0, 0]) == ~ok).all() and np.isnan(got[~ok]).all()
        assert sk.same_bytes(got[ok], np.transpose(got[ok], (0, 2, 1)))
        X64 = X.astype(np.float64)
        if mode == 0: ref = np.stack([0.5 * (X64[c, :, 9 * j:9 * j + 9] + X64[c, :, 9 * j:9 * j + 9].T) for j, c in enumerate(ids)])
        else:
            ref = np.zeros((len(ids), 3, 3))
            for j, p in enumerate(ids):
                g = A.Ge[p].astype(np.float64)
                M = g.T @ g
                for q, c in A.pcg._list(p): M = M + (A.W[q].astype(np.float64) @ g).T @ X64[c, :, 3 * j:3 * j + 3]
                ref[j] = 0.5 * (M + M.T)
        _bar(_name(dims, renumber), "out cameras" if mode == 0 else "out points", rel_max(got[ok], ref[ok]), rel_max(m32[ok], ref[ok]))


# ------------------------------------------------------------------ 2. the batch driver
@pytest.mark.parametrize("dims,band,renumber", CASES)
def test_driver_against_float64_and_its_bits(torch, L, instances, dims, band, renumber):
    """thallo_hip_ba_cov_solve under the defaults: the camera blocks against float64 inv(S_FF) of the device's own S within 4 x the restatement's error on the same S;
    every solved column converged; held rows and columns exactly zero (cov_error asserts it); bitwise symmetric; a second run the same bits; one camera alone in a batch is
    the same camera among seven, one point alone the same point among 21, bit for bit"""
    A = instances(dims, band, renumber)
    name = _name(dims, renumber)
    free = A.free_c.reshape(-1, 9)[A.cams]
    ref = cm.blocks_of(A.Sig_cc, A.cams, 9)
    Bd, info = A.solve(torch, L, 0, A.cams)
    Bm, im = A.pcg.solve(0, A.cams)
    e_dev, e_mir = cm.cov_error(Bd, ref, free), cm.cov_error(Bm, ref, free)
    print("covariance", name, "driver, cameras: mirror error", e_mir, "device", e_dev, "= %.2f x" % (e_dev / e_mir), "iterations", info.iterations, "mirror", im["iterations"],
          "worst", info.worst)
    assert info.not_converged == 0 and info.columns == int(free.sum()) == im["columns"] and info.nan_blocks == 0 and 0 < info.worst <= 1e-6
    assert im["iterations"] - 3 <= info.iterations <= im["iterations"] + 2 * 8 + 3      # the batch ends at most two chunks of 8 behind the iteration that froze its last column
    assert e_mir > 0 and e_dev <= 4 * e_mir
    assert sk.same_bytes(Bd, np.transpose(Bd, (0, 2, 1)))
    again, _ = A.solve(torch, L, 0, A.cams)
    assert sk.same_bytes(Bd, again)
    k = len(A.cams) // 2
    alone, _ = A.solve(torch, L, 0, [A.cams[k]])
    assert sk.same_bytes(alone[0], Bd[k])
    Pd, pinfo = A.solve(torch, L, 1, A.pts)
    Pm, pm = A.pcg.solve(1, A.pts)
    ok = ~np.isnan(Pm[:, 0, 0])
    assert pinfo.nan_blocks == 2 == pm["nan_blocks"] and pinfo.not_converged == 0 and (np.isnan(Pd[:, 0, 0]) == ~ok).all() and sk.same_bytes(Pd[ok], np.transpose(Pd[ok], (0, 2, 1)))
    alone, _ = A.solve(torch, L, 1, [A.pts[7]])
    assert sk.same_bytes(alone[0], Pd[7])
    # the points: against the point formula in float64 on the device's own S, W and G
    refp = np.zeros((len(A.pts), 3, 3))
    for j, p in enumerate(A.pts):
        g = A.Ge[p].astype(np.float64)
        V = np.zeros((9 * A.C, 3))
        for q, c in A.pcg._list(p): V[9 * c:9 * c + 9] += A.W[q].astype(np.float64) @ g
        refp[j] = g.T @ g + V.T @ A.Sig_cc @ V
    fp = np.ones((len(A.pts), 3), bool)
    e_dev, e_mir = cm.cov_error(Pd[ok], refp[ok], fp[ok]), cm.cov_error(Pm[ok], refp[ok], fp[ok])
    print("covariance", name, "driver, points: mirror error", e_mir, "device", e_dev, "= %.2f x" % (e_dev / e_mir))
    assert e_mir > 0 and e_dev <= 4 * e_mir


def test_driver_with_one_iteration_reports_the_unconverged_columns(torch, L, instances):
    A = instances(KERNEL[2][0], KERNEL[2][1], False)
    Bd, info = A.solve(torch, L, 0, A.cams, max_it=1)
    free = A.free_c.reshape(-1, 9)[A.cams]
    assert info.iterations == 1 and info.columns == int(free.sum()) and info.not_converged == info.columns and info.worst > 1e-6 and np.isfinite(Bd).all()


class Chain:
    """a block-tridiagonal symmetric positive definite S over C cameras, in the assembled form's layout, with the factors of its diagonal blocks -- for camera counts the
    instances do not reach"""

    def __init__(self, C_, seed=3):
        rng = np.random.default_rng(seed)
        self.C = C_
        n = np.full(C_, 3); n[0] = n[-1] = 2
        self.row_ptr = np.concatenate([[0], np.cumsum(n)]); self.nblk = int(self.row_ptr[-1])
        self.col = np.concatenate([[c + o for o in (-1, 0, 1) if 0 <= c + o < C_] for c in range(C_)])
        off = (0.1 * rng.standard_normal((C_ - 1, 9, 9))).astype(F32)                 # block (c + 1, c)
        D = rng.standard_normal((C_, 9, 9)); D = (4 * np.eye(9) + 0.1 * (D + np.transpose(D, (0, 2, 1)))).astype(F32)
        self.S = np.zeros((self.nblk, 9, 9), F32)
        for c in range(C_):
            for t in range(self.row_ptr[c], self.row_ptr[c + 1]):
                j = self.col[t]
                self.S[t] = D[c] if j == c else off[j].T if j < c else off[c]
        self.Gc = np.tril(np.linalg.inv(np.linalg.cholesky(D.astype(np.float64)))).astype(F32)

    def bsr(self, S):
        import scipy.sparse as sp
        return sp.bsr_matrix((np.asarray(S, np.float64), self.col, self.row_ptr), shape=(9 * self.C, 9 * self.C))


def test_more_cameras_than_partial_slots(torch, L):
    """C = 1030 > 1024: a workgroup of the panel launches then takes more than one camera row and the slots hold 1024 partials per column.  S X, G^T G R and their
    partials within 4 e32, the driver's blocks for cameras on both sides of the wrap (0, 5, 6, 1023, 1024, 1029) against float64 inv(S) within 4 x the restatement's
    error, one camera alone the same bits"""
    T = Chain(1030)
    C_ = T.C
    pcg = cm.ColumnPCG32(T, T.S, T.Gc, np.zeros((0, 3, 3), F32), np.zeros((0, 9, 3), F32), None)
    assert pcg.grid == 1024
    packed = np.concatenate([T.Gc[:, i, j] for i in range(9) for j in range(i + 1)])
    d = dict(row_ptr=dev(torch, T.row_ptr, np.int32), col=dev(torch, T.col, np.int32), S=dev(torch, T.S.transpose(1, 2, 0).ravel()), Gc=dev(torch, packed))
    P = lambda k: d[k].data_ptr()
    X = np.random.default_rng(43).standard_normal((C_, 9, K)).astype(F32)
    Xd, Y, Z = dev(torch, X.ravel()), dev(torch, np.full(9 * C_ * K, np.nan)), dev(torch, np.full(9 * C_ * K, np.nan))
    pa, pb = sk.canary_buf(torch, 1026 * K), sk.canary_buf(torch, 1026 * K)
    assert L.thallo_hip_ba_schur_apply_s_cols(C_, T.nblk, P("row_ptr"), P("col"), P("S"), Xd.data_ptr(), Y.data_ptr(), pa.data_ptr(), None) == 1024
    assert L.thallo_hip_ba_cov_precond_cols(C_, P("Gc"), Xd.data_ptr(), Z.data_ptr(), pb.data_ptr(), None) == 1024
    torch.cuda.synchronize()
    for k in d: host(d[k], 1, np.uint32)
    S64 = T.bsr(T.S).toarray()
    G = T.Gc.astype(np.float64)
    for what, out, part, ref, m32 in (("S X", Y, pa, (S64 @ X.reshape(9 * C_, K).astype(np.float64)).reshape(C_, 9, K), pcg.apply(X)),
                                      ("G^T G R", Z, pb, np.einsum("cki,ckj,cjn->cin", G, G, X.astype(np.float64)), pcg.precond(X))):
        got = host(out, 9 * C_ * K).reshape(C_, 9, K)
        ph = part.cpu().numpy().reshape(-1, K)
        assert sk.written_slots(ph) == 1024
        _bar((C_, "chain"), what, rel_max(got, ref), rel_max(m32[0], ref))
        t = X.astype(np.float64) * got
        assert (np.abs(ph[:1024].astype(np.float64).sum(0) - t.sum((0, 1))) <= 19 * EPS * np.abs(t).sum((0, 1))).all()      # (two rows of nine behind a partial)
    sys = SysT(C_, 0, T.nblk, P("row_ptr"), P("col"), P("S"), P("Gc"), None, None, None, None, None, None)
    work = torch.zeros(int(L.thallo_hip_ba_cov_work_bytes(C_)) // 4 + 64, dtype=torch.float32, device="cuda")
    cams = [0, 5, 6, 1023, 1024, 1029]

    def solve(ids):
        idd, out, info = dev(torch, ids, np.int32), dev(torch, np.full(len(ids) * 81, np.nan)), InfoT()
        assert L.thallo_hip_ba_cov_solve(C.byref(sys), 0, idd.data_ptr(), len(ids), 1e-6, 500, work.data_ptr(), None, out.data_ptr(), C.byref(info), None) == 0
        return host(out, len(ids) * 81).reshape(-1, 9, 9), info
    Bd, info = solve(cams)
    Bm, im = pcg.solve(0, cams)
    ref = cm.blocks_of(np.linalg.inv(S64), cams, 9)
    free = np.ones((len(cams), 9), bool)
    e_dev, e_mir = cm.cov_error(Bd, ref, free), cm.cov_error(Bm, ref, free)
    print("covariance", (C_, "chain"), "driver: mirror error", e_mir, "device", e_dev, "= %.2f x" % (e_dev / e_mir), "iterations", info.iterations, "mirror", im["iterations"])
    assert info.not_converged == 0 and info.columns == 54 and e_mir > 0 and e_dev <= 4 * e_mir
    assert sk.same_bytes(solve([1024])[0][0], Bd[4]) and sk.same_bytes(Bd, np.transpose(Bd, (0, 2, 1)))


# ------------------------------------------------------------------ 3. through the C ABI
SHAPES = [((5, 72, 330), 5, True), ((3, 160, 480), 3, True), ((24, 300, 1200), 12, False)]
GN = dict(nIterations=3, lIterations=10)
LM = dict(nIterations=3, lIterations=50, q_tolerance=0.1, function_tolerance=0.0)


def problem(dims, band, extras):
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    return with_extras(p) if extras else (p, dims)


def plan(dims, p, lm, loss=None, hold=None, solver="schur_explicit_pcg", **sp):
    d = to_device(copy_params(p))
    s = api.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), solverkind="levenberg_marquardt" if lm else "gauss_newton")
    if lm: s.enable_lm()
    if solver: s.set_linear_solver(solver)
    if loss: s.set_robust_loss(loss, 2.0)
    if hold is not None:
        s.hold(0, hold[:9 * dims[0]])
        if hold[9 * dims[0]:].any(): s.hold(1, hold[9 * dims[0]:])
    s.set_solver_parameters(**sp)
    params = s.make_params(d)
    s.init(params)
    assert s.ready(), api.last_error()
    return s, params, d


def requests(dims, extras):
    C_, P_, _ = dims
    cams = list(range(C_ - 1 if extras else 9))                                   # (24 cameras: 9, two batches; the camera nothing observes is not asked for here)
    pts = list(range(0, P_ - 2, max(1, P_ // 25)))[:23] + ([P_ - 2, P_ - 1] if extras else [3, 4])      # 25 points: two batches
    return cams, pts


@pytest.mark.parametrize("loss", [None, "huber"])
@pytest.mark.parametrize("renumber", ["0", "1"])
@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("dims,band,extras", SHAPES)
def test_blocks_through_the_c_abi_against_float64(torch, monkeypatch, dims, band, extras, lm, renumber, loss):
    """after 3 steps (GN 3 x 10, LM 3 x 50): camera and point blocks against the float64 (A_FF)^-1 of the oracle's J at the device's unknowns -- with the robust weights under
    Huber(2) --, within 4 x the float32 restatement's error against the same reference; held scalars' rows and columns exactly zero, the fully held camera a zero block;
    the point nothing observes and the point observed once are NaN blocks and counted; every block symmetric bit for bit; info adds up"""
    p, d3 = problem(dims, band, extras)
    C_, P_, _ = d3
    mask = cm.gauge_mask(C_, P_)
    set_ab(monkeypatch, ba_renumber=renumber)
    s, params, d = plan(d3, p, lm, loss, mask, **(LM if lm else GN))
    while s.step(params): pass
    cams, pts = requests(d3, extras)
    out = s.covariance(params, cameras=cams, points=pts)
    here = [to_host(d[0]).copy(), to_host(d[1]).copy()] + [a.copy() for a in p[2:]]
    s.close()
    m = (robust(BaBlockMirror)(loss, 2.0, d3, here) if loss else BaBlockMirror(d3, here))
    J, sys = cm.system_of(m, mask)
    A = (J.T @ J).toarray()
    free = ~mask & ~cm.undetermined(A, C_)
    Sig = cm.dense_cov64(A, free)
    pcg = cm.ColumnPCG32.of(sys, mask)
    name = (d3, "LM" if lm else "GN", "renumbered" if renumber == "1" else "caller's order", loss or "squared")
    info, columns = out["info"], 0
    for mode, ids, key, dd, off in ((0, cams, "cameras", 9, 0), (1, pts, "points", 3, 9 * C_)):
        got = out[key]
        Bm, im = pcg.solve(mode, ids)
        ok = ~np.isnan(Bm[:, 0, 0]); columns += im["columns"]
        ref = cm.blocks_of(Sig, ids, dd, off)
        fr = free[off:off + dd * (C_ if mode == 0 else P_)].reshape(-1, dd)[ids]
        assert (np.isnan(got[:, 0, 0]) == ~ok).all() and np.isnan(got[~ok]).all() and int((~ok).sum()) == (2 if extras and mode else 0)
        e_dev, e_mir = cm.cov_error(got[ok], ref[ok], fr[ok]), cm.cov_error(Bm[ok], ref[ok], fr[ok])
        print("covariance", name, key, "mirror error", e_mir, "device", e_dev, "= %.2f x" % (e_dev / e_mir), "mirror iterations", im["batch_iterations"])
        assert sk.same_bytes(got[ok], np.transpose(got[ok], (0, 2, 1)))
        assert e_mir > 0 and e_dev <= 4 * e_mir, (name, key, e_dev, e_mir)
    assert not out["cameras"][0].any() and not out["cameras"][1][3].any() and out["cameras"][1][0, 0] > 0
    print("covariance", name, "info", info)
    assert info["not_converged"] == 0 and info["nan_blocks"] == (2 if extras else 0) and 0 < info["worst_residual"] <= 1e-6
    assert info["columns"] == columns >= int(free[:9 * C_].reshape(-1, 9)[cams].sum())


@pytest.mark.parametrize("lm", [False, True])
def test_a_point_the_caller_holds_is_zeros_not_nan(torch, lm):
    dims, band, _ = SHAPES[2]
    p, d3 = problem(dims, band, False)
    mask = cm.gauge_mask(d3[0], d3[1])
    mask[9 * d3[0] + 3 * 5:9 * d3[0] + 3 * 5 + 3] = True; mask[9 * d3[0] + 3 * 6 + 1] = True
    s, params, d = plan(d3, p, lm, None, mask, **(LM if lm else GN))
    s.step(params)
    out = s.covariance(params, points=[5, 6, 7])
    s.close()
    B = out["points"]
    assert not B[0].any() and out["info"]["nan_blocks"] == 0 and not B[1][1].any() and not B[1][:, 1].any() and B[1][0, 0] > 0 and B[2].all() and np.isfinite(B).all()


@pytest.mark.parametrize("lm", [False, True])
def test_the_call_leaves_the_solve_as_it_was(torch, lm):
    """step, covariance, step against step, step: the same unknown bytes, the same costs, the same PCG iterations and alpha / beta traces, the same launch counts by name --
    the call's own launches are kept out of the kernel statistics --, in GN and in LM (radius, SSq, previous cost and prevX are the LM step's)"""
    dims, band, _ = SHAPES[2]
    p, d3 = problem(dims, band, False)
    mask = cm.gauge_mask(d3[0], d3[1])
    sp = dict(LM, nIterations=4) if lm else dict(GN, nIterations=4)
    runs = []
    for call in (False, True):
        s, params, d = plan(d3, p, lm, None, mask, **sp)
        costs, traces = [s.current_cost()], []
        for k in range(4):
            assert s.step(params)
            costs.append(s.current_cost()); traces.append(s.alpha_beta_trace())
            if call and k in (0, 2):
                out = s.covariance(params, cameras=[1, 2], points=[0, 1, 2])
                assert np.isfinite(out["cameras"]).all() and out["info"]["not_converged"] == 0
        stats = {k: v["launches"] for k, v in s.kernel_stats().items() if v["launches"]}
        runs.append((costs, traces, stats, to_host(d[0]).copy(), to_host(d[1]).copy()))
        s.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and not any(k.startswith("Cov") for k in b[2])
    assert sk.same_bytes(a[3], b[3]) and sk.same_bytes(a[4], b[4])
    assert (a[3] != p[0]).any()


def test_one_iteration_returns_the_unconverged_columns(torch):
    dims, band, _ = SHAPES[2]
    p, d3 = problem(dims, band, False)
    s, params, d = plan(d3, p, False, None, cm.gauge_mask(d3[0], d3[1]), **GN)
    s.step(params)
    ids = np.array([1, 2, 3], np.int32); blocks = np.full((3, 9, 9), np.nan, np.float32)
    opt, info = api.CovarianceOptions(1e-6, 1), api.CovarianceInfo()
    rc = s._L.ThalloX_PlanCovariance(s.plan, params, 0, ids.ctypes.data_as(C.c_void_p), 3, blocks.ctypes.data_as(C.c_void_p), C.byref(opt), C.byref(info))
    assert rc == info.not_converged == info.columns == 26 and info.iterations == 1 and info.worst_residual > 1e-6 and np.isfinite(blocks).all()
    rc = s._L.ThalloX_PlanCovariance(s.plan, params, 0, ids.ctypes.data_as(C.c_void_p), 3, blocks.ctypes.data_as(C.c_void_p), None, None)      # the defaults, no info
    assert rc == 0 and blocks[0][0, 0] > 0
    s.close()


def test_refusals_by_their_messages(torch, monkeypatch, tmp_path):
    """wherever the assembled form is refused, and: another linear solver at the last Init (the message says which to set), before Init, an input that is not an Unknown,
    n <= 0, an id out of range or repeated, a rel_tol that is not finite and positive, max_iterations < 1"""
    ids = np.array([0, 1], np.int32); out = np.zeros((2, 9, 9), np.float32)
    ip, op = ids.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def refused(s, params, *words, input=0, idp=ip, n=2, opt=None):
        rc = s._L.ThalloX_PlanCovariance(s.plan, params, input, idp, n, op, None if opt is None else C.byref(opt), None)
        msg = api.last_error()
        assert rc < 0 and s.energy_name in msg and all(w in msg for w in words), (rc, msg, words)

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energies")
    for dims, f, dbl, word in (((48, 32), thallo_amd.energy_file("image_warping"), False, "no covariance for this energy"),
                               ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), False, "no covariance for this energy"),
                               ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), True, "doublePrecision"),
                               ((5, 72, 330), thallo_amd.energy_file("bundle_adjustment"), True, "doublePrecision")):
        s = api.ThalloSolver(dims, f, double_precision=dbl)
        refused(s, None, word)
        with pytest.raises(RuntimeError, match="ThalloX_PlanCovariance failed"): s.covariance(None, cameras=[0])
        s.close()
    s = api.ThalloSolver((8, 72, 330), thallo_amd.energy_file("bundle_adjustment"))      # a distributed plan (one rank's camera shard)
    s.set_distributed(0, 1, 0, 0, device_exchange=False)
    refused(s, None, "distributed")
    s.close()
    lines = "".join(f"r.{n}.J:set_materialize(true)\nr.{n}.JtJ:set_materialize(true)\n" for n in ("fit", "reg")) + "r:set_direct_solve(true)\n"
    f = tmp_path / "laplacian_direct.t"
    f.write_text(open(thallo_amd.energy_file("laplacian_graph")).read() + "\n" + lines)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("THALLO_FRONTEND", "generate"); mp.setenv("THALLO_ENABLE_DIRECT_SOLVE", "1")
        s = api.ThalloSolver((256, 255), str(f))
        assert s.schedule_name == "dense direct solve"
        refused(s, None, "direct-solve")
        s.close()
    dims, band, _ = SHAPES[0]
    p, d3 = problem(dims, band, False)
    s = api.ThalloSolver(d3, thallo_amd.energy_file("bundle_adjustment"))
    s.set_linear_solver("schur_explicit_pcg")
    s.hold(0, cm.gauge_mask(d3[0], d3[1])[:9 * d3[0]])
    s.set_solver_parameters(**GN)
    d = to_device(copy_params(p))
    params = s.make_params(d)
    refused(s, params, "before Thallo_ProblemInit")
    s.init(params)
    refused(s, params, "not an Unknown", input=2)
    refused(s, params, "n > 0", n=0)
    refused(s, params, "n > 0", n=-3)
    bad = np.array([0, d3[0]], np.int32); refused(s, params, "out of range", idp=bad.ctypes.data_as(C.c_void_p))
    bad2 = np.array([-1, 0], np.int32); refused(s, params, "out of range", idp=bad2.ctypes.data_as(C.c_void_p))
    rep = np.array([1, 1], np.int32); refused(s, params, "repeated", idp=rep.ctypes.data_as(C.c_void_p))
    for tol in (0.0, -1e-6, float("nan"), float("inf")): refused(s, params, "rel_tol", opt=api.CovarianceOptions(tol, 500))
    for it in (0, -5): refused(s, params, "max_iterations", opt=api.CovarianceOptions(1e-6, it))
    assert s._L.ThalloX_PlanCovariance(s.plan, params, 0, ip, 2, op, None, None) == 0      # and the plan still answers
    s.close()
    for solver in (None, "schur_pcg"):
        s, params, d = plan(d3, p, False, None, None, solver=solver, **GN)
        refused(s, params, "THALLOX_SOLVER_SCHUR_EXPLICIT_PCG", "ThalloX_PlanSetLinearSolver")
        s.close()


@pytest.mark.parametrize("lm", [False, True])
def test_a_plan_that_never_calls_it_is_the_plan_it_was(torch, lm):
    """a kind-2 plan that never makes the call against one that made it BEFORE its first step and after its last: the same costs, iterations, schedule name, launch
    counts by name (none of them the call's) and unknown bytes -- the call added nothing to Init or to a step, and no existing launch changed
    (tests/test_gpu_ba_schur_explicit.py pins those steps against the CPU restatement and the default plan's bits)"""
    dims, band, _ = SHAPES[2]
    p, d3 = problem(dims, band, False)
    mask = cm.gauge_mask(d3[0], d3[1])
    runs = []
    for call in (False, True):
        s, params, d = plan(d3, p, lm, None, mask, **(LM if lm else GN))
        if call: s.covariance(params, cameras=[1])
        costs, iters = [s.current_cost()], []
        while s.step(params):
            costs.append(s.current_cost()); iters.append(len(s.alpha_beta_trace()))
        if call: s.covariance(params, points=[1])
        runs.append((costs, iters, s.schedule_name, {k: v["launches"] for k, v in s.kernel_stats().items() if v["launches"]}, to_host(d[0]).copy(), to_host(d[1]).copy()))
        s.close()
    a, b = runs
    assert a[:4] == b[:4] and sk.same_bytes(a[4], b[4]) and sk.same_bytes(a[5], b[5])
