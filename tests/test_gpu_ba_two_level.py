"""The two-level preconditioner on bundle adjustment's assembled reduced camera matrix (csrc/ba_coarse.hip, ThalloX_PlanSetPreconditioner kind 2): every kernel through its
exported symbol against float64 from the device's own operands, the covariance's column solve with the coarse operands, then the C call -- trajectories, held bits, the
covariance, unchanged plans, refusals.

Bars.  A single operation is held to 4 e32, e32 the distance of its float32 restatement in the kernel's summation order (tests/ba_two_level_mirror.py: every product and
addition rounded on its own; the device differs by its fused multiply-adds) from the same float64 reference, recomputed in the run.  The scaling is bit for bit.  The factor
and the inverse are held to Higham's componentwise bounds (Accuracy and Stability, theorems 10.3 and 8.5), u = 2^-24, gamma_k = k u / (1 - k u), as
tests/test_gpu_ba_schur_dense.py holds its factor and sweeps: |T - L L^T| <= 2 gamma_{n+1} |L||L|^T and |D - L Z| <= 2 gamma_n |L||Z| (plus 4 n 2^-126 (1 + max |L|): the
entries of Z far from the diagonal of a banded factor lie below the normal range, where an operation has an absolute error); and Z S_c Z^T against the identity
on the live scalars to the first-order bound that follows from the two and the scaling's two roundings,
  |L^-1| (2 gamma_{n+1} |L||L|^T + 2.01 u |T| + 2 gamma_n (|L||Z| D^-1 |T| + its transpose)) |L^-T|,
with 1 % for the second-order terms.  Partial sums: a partial adds t terms one after the other, the reader adds the partials in float64 here: (t + 6) u sum |terms|.
Through the C ABI: costs per step the mirror's within tests/test_gpu_ba_schur_explicit.py's max(1e-5, 3 err_jacobi); covariances within 4 x the column mirror's error.
Every figure is printed before it is asserted.

Instances: (5, 72, 330) and (24, 300, 1200) with their extras (a camera and a point nothing observes, a point observed once) as tests/test_gpu_ba_covariance.py sets them
up, S assembled on the device under the gauge (camera 0 held entirely, scalar 3 of camera 1); a block-tridiagonal chain of 64 cameras.  Aggregates: greedy pairs on the six
cameras; on the 25: one aggregate holding everything (K = 1, n_c = 9), singletons (K = 25, n_c = 225: no multiple of 32, more rows than one workgroup's four), K = 8
(n_c = 72) with scalar 6 held on every member of aggregate 3 (the identity's row, d = 0), the default greedy aggregates; K = 29 (n_c = 261) on the chain.

Measured on an MI355X (the tests print every figure before they assert; also in DESIGN.md section 19): the assembly gives the restatement's bits in all six cases; d within
2 u; largest multiples of the bounds 0.10 (factor), 0.037 (forward sweep) and 0.033 (Z S_c Z^T - I); vector and panel applies 1.00 - 1.55 e32; the partials of y . y
0.02 / 0.012 of their bars; a panel's column against the vector form 0.12 - 0.17 of the summed bars; the column solve 0.34 - 0.61 x the mirror's error in 24 / 56 / 8 iterations
against block Jacobi's 32 / 72 / 72; trajectories: largest cost difference from the mirror 9.3e-7 (err_jacobi 4.6e-7 ... 8.0e-7); the covariance through the C ABI
0.90 - 1.81 x the mirror's error; (200, 6000, 26000): 144 iterations against block Jacobi's 344, every column converged."""
import ctypes as C

import numpy as np
import pytest

import shim_kernels as sk
import test_gpu_block_precond as bp
import thallo_amd
from shim_kernels import EPS, F32
from thallo_amd import api, synthetic as syn

import ba_covariance_mirror as cm
import ba_two_level_mirror as tl
from ba_robust_mirror import robust
from ba_block_mirror import BaBlockMirror
from ba_schur_mirror import rel_max
from helpers import copy_params, set_ab, to_device, to_host
from test_gpu_ba_covariance import Chain, CovDevice, InfoT, SysT, problem
from test_gpu_ba_schur import dev, host, rel, run, torch      # noqa: F401  (torch: the module fixture)

pytestmark = pytest.mark.gpu

K = cm.K
GN = dict(nIterations=3, lIterations=10)
LM = dict(nIterations=3, lIterations=7, q_tolerance=0.1, function_tolerance=0.0)
SHAPES = [((5, 72, 330), 5, True), ((24, 300, 1200), 12, False)]


def gamma(k): return k * EPS / (1 - k * EPS)


class CoarseT(C.Structure):                 # thallo_coarse_t
    _fields_ = [("C", C.c_int), ("K", C.c_int), ("n", C.c_long), ("ld", C.c_long), ("agg", C.c_void_p), ("mem_ptr", C.c_void_p), ("mem", C.c_void_p), ("hold", C.c_void_p),
                ("T", C.c_void_p), ("d", C.c_void_p), ("Z", C.c_void_p), ("Zt", C.c_void_p), ("y", C.c_void_p), ("words", C.c_void_p)]


@pytest.fixture(scope="module")
def L(torch):
    lib = C.CDLL(thallo_amd.lib()._name)
    vp, it, lg, fl = C.c_void_p, C.c_int, C.c_long, C.c_float
    R, spt, cpt = bp.RegionsT, C.POINTER(SysT), C.POINTER(CoarseT)
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
        "ba_cov_work_bytes": [it],
        "ba_cov_solve": [spt, it, vp, it, fl, it, vp, vp, vp, C.POINTER(InfoT), vp],
        "dense_ld": [lg],
        "dense_potrf": [lg, lg, vp, vp, vp],
        "ba_coarse_assemble": [cpt, lg, vp, vp, vp, vp],
        "ba_coarse_scale": [cpt, vp],
        "ba_coarse_panel_floats": [lg],
        "ba_coarse_inverse": [cpt, vp, vp],
        "ba_coarse_apply": [cpt, vp, vp, vp, vp, vp],
        "ba_coarse_cols_work_floats": [lg],
        "ba_coarse_apply_cols": [cpt, vp, vp, vp, vp, vp, vp],
        "ba_cov_coarse_work_bytes": [it, lg],
        "ba_cov_solve_coarse": [spt, cpt, it, vp, it, fl, it, vp, vp, vp, C.POINTER(InfoT), vp],
    }
    for name, args in sig.items():
        f = getattr(lib, "thallo_hip_" + name)
        f.argtypes = args
        f.restype = lg if name in ("vector_elems", "ba_cov_work_bytes", "dense_ld", "ba_coarse_panel_floats", "ba_coarse_cols_work_floats", "ba_cov_coarse_work_bytes") else it
    return lib


# ------------------------------------------------------------------ the cases: an assembled S on the device, aggregates, a mask -- and every stage of the set-up, run once
class Sys:
    """what the coarse kernels read of an assembled S: the structure (C, nblk, row_ptr, col, bsr), the stored blocks on the host, their device copies"""

    def __init__(self, st, S, row_ptr, col, Sd, cov=None):
        self.st, self.S, self.row_ptr, self.col, self.Sd, self.cov = st, S, row_ptr, col, Sd, cov
        self.C = st.C
        self.S64 = st.bsr(S).toarray()


class Case:
    def __init__(self, torch, L, name, sys, agg, mem_ptr, mem, hold_c):
        self.name, self.sys = name, sys
        self.C = C_ = sys.C
        self.agg, self.mem_ptr, self.mem = np.asarray(agg, np.int64), np.asarray(mem_ptr, np.int64), np.asarray(mem, np.int64)
        self.Kc = Kc = len(mem_ptr) - 1
        self.n = n = 9 * Kc
        self.ld = ld = int(L.thallo_hip_dense_ld(n))
        self.hold_c = None if hold_c is None else np.asarray(hold_c, bool).reshape(C_, 9)
        assert tl.validate_aggregates(self.agg, C_) is None and ld % 32 == 0 and n <= ld < n + 32
        i32 = lambda a: dev(torch, a, np.int32)
        m8 = np.zeros((9 * C_ + 3) // 4 * 4, np.uint8)
        if hold_c is not None: m8[:9 * C_] = self.hold_c.ravel()
        self.d = d = dict(agg=i32(self.agg), mem_ptr=i32(self.mem_ptr), mem=i32(self.mem), hold=dev(torch, m8.view(np.uint32), np.uint32),
                          T=dev(torch, np.full(n * ld, sk.CANARY, np.uint32), np.uint32), dd=dev(torch, np.full(n, np.nan)), Z=dev(torch, np.full(n * ld, np.nan)),
                          Zt=dev(torch, np.zeros(n * ld)), y=dev(torch, np.full(n, np.nan)), words=dev(torch, np.array([77, 78, 5, 0], np.uint32), np.uint32),
                          panels=dev(torch, np.full(int(L.thallo_hip_ba_coarse_panel_floats(n)), np.nan)))
        P = lambda k: d[k].data_ptr()
        self.ct = CoarseT(C_, Kc, n, ld, P("agg"), P("mem_ptr"), P("mem"), P("hold") if hold_c is not None else None, P("T"), P("dd"), P("Z"), P("Zt"), P("y"), P("words"))
        self.P64 = tl.prolongation(self.agg, self.hold_c).toarray()
        # stage by stage, the buffers read back behind each
        run = lambda rc: (rc == 0 or pytest.fail("%s: launch code %d" % (name, rc)), torch.cuda.synchronize())
        run(L.thallo_hip_ba_coarse_assemble(C.byref(self.ct), sys.st.nblk, sys.row_ptr.data_ptr(), sys.col.data_ptr(), sys.Sd.data_ptr(), None))
        self.Sc_raw = host(d["T"], n * ld, np.uint32).reshape(n, ld)
        run(L.thallo_hip_ba_coarse_assemble(C.byref(self.ct), sys.st.nblk, sys.row_ptr.data_ptr(), sys.col.data_ptr(), sys.Sd.data_ptr(), None))
        self.Sc_again = host(d["T"], n * ld, np.uint32).reshape(n, ld)
        run(L.thallo_hip_ba_coarse_scale(C.byref(self.ct), None))
        self.T_raw = host(d["T"], n * ld, np.uint32).reshape(n, ld)
        self.dh = host(d["dd"], n)
        self.words_scaled = host(d["words"], 4, np.uint32)
        run(L.thallo_hip_dense_potrf(n, ld, P("T"), P("words"), None))
        self.L_raw = host(d["T"], n * ld, np.uint32).reshape(n, ld)
        run(L.thallo_hip_ba_coarse_inverse(C.byref(self.ct), P("panels"), None))
        self.Z = host(d["Z"], n * ld).reshape(n, ld)
        self.Zt = host(d["Zt"], n * ld).reshape(n, ld)
        self.words = host(d["words"], 4, np.uint32)

    def lower(self, raw):
        """the lower triangle of a stored [n, ld] buffer as float32 [n, n]; the canaries above it and in the padding must be where they were"""
        n = self.n
        up = np.triu_indices(n, 1)
        assert (raw[:, :n][up] == sk.CANARY).all() and (raw[:, n:] == sk.CANARY).all(), "the upper triangle or the padding changed"
        return np.tril(raw[:, :n].view(F32))


def chain_sys(torch, C_):
    T = Chain(C_)
    T.row = np.repeat(np.arange(C_), np.diff(T.row_ptr))
    return Sys(T, T.S, dev(torch, T.row_ptr, np.int32), dev(torch, T.col, np.int32), dev(torch, T.S.transpose(1, 2, 0).ravel()))


CASES = ["six_pairs", "one_aggregate", "singletons", "eight_identity_row", "default_greedy", "chain_29"]


@pytest.fixture(scope="module")
def cases(torch, L):
    cache, systems = {}, {}

    def system(dims, band):
        if dims not in systems:
            A = CovDevice(torch, L, dims, band, False)
            systems[dims] = Sys(A.st, A.S, A.d["row_ptr"], A.d["col"], A.d["S"], A)
        return systems[dims]

    def get(name):
        if name in cache: return cache[name]
        if name == "chain_29":
            s = chain_sys(torch, 64)
            agg = np.arange(64) * 29 // 64
            mem_ptr, mem = tl.member_lists(agg)
            hold = None
        else:
            s = system(*((5, 72, 330), 5) if name == "six_pairs" else ((24, 300, 1200), 12))
            C_ = s.C
            hold = s.cov.mask[:9 * C_].reshape(C_, 9).copy()
            if name == "six_pairs": agg, mem_ptr, mem = tl.greedy_aggregates(s.st, 2)
            elif name == "default_greedy": agg, mem_ptr, mem = tl.greedy_aggregates(s.st, tl.default_k(C_))
            else:
                agg = {"one_aggregate": np.zeros(C_, np.int64), "singletons": np.arange(C_), "eight_identity_row": np.arange(C_) * 8 // C_}[name]
                mem_ptr, mem = tl.member_lists(agg)
            if name == "eight_identity_row": hold[agg == 3, 6] = True
        cache[name] = Case(torch, L, name, s, agg, mem_ptr, mem, hold)
        return cache[name]
    return get


def _bar(name, what, got, e32):
    print("two-level", name, what, "e32", e32, "device", got, "= %.2f e32" % (got / e32 if e32 > 0 else np.inf))
    assert e32 > 0 and got <= 4 * e32, (name, what, got, e32)


# ------------------------------------------------------------------ 1. the set-up
@pytest.mark.parametrize("name", CASES)
def test_assembly_against_the_float64_block_sums(cases, name):
    """the lower triangle of P^T S P from the device's own S within 4 e32, and the restatement's bits (the sums are additions alone); the upper triangle and the padding keep their canaries; two runs the same bits"""
    c = cases(name)
    assert c.Kc == {"six_pairs": c.Kc, "one_aggregate": 1, "singletons": 25, "eight_identity_row": 8, "default_greedy": c.Kc, "chain_29": 29}[name]
    got = c.lower(c.Sc_raw)
    ref = np.tril(c.P64.T @ c.sys.S64 @ c.P64)
    m32 = tl.assemble32(c.sys.st, c.sys.S, c.agg, c.mem_ptr, c.mem, c.hold_c)
    e32, e = rel_max(m32, ref), rel_max(got, ref)
    print("two-level", name, "S_c (K = %d, n_c = %d)" % (c.Kc, c.n), "e32", e32, "device", e)
    assert e <= 4 * e32      # (singletons copy their blocks: both sides are exact)
    assert sk.same_bytes(got, m32)      # additions alone, in the restatement's order: nothing to contract
    assert sk.same_bytes(c.Sc_raw, c.Sc_again)


@pytest.mark.parametrize("name", CASES)
def test_scaling_is_the_two_rounded_products_bit_for_bit(cases, name):
    """d = S_c,ii^-1/2 within 2 u, 0 where the diagonal is not positive (counted: every member held there, or nothing observed); every stored entry
    float32(float32(d_i s_ij) d_j) bit for bit with the identity's rows and columns at d = 0; canaries intact"""
    c = cases(name)
    Sc = c.lower(c.Sc_raw)
    diag = np.diag(Sc)
    dead = ~(diag > 0)
    assert int(c.words_scaled[1]) == int(dead.sum()) and int(c.words_scaled[2]) == 5 and not c.dh[dead].any()
    ref = 1.0 / np.sqrt(diag[~dead].astype(np.float64))
    e = np.abs(c.dh[~dead] - ref) / ref
    print("two-level", name, "d: largest relative error", float(e.max() / EPS), "u; identity rows", int(dead.sum()))
    assert e.max() <= 2 * EPS
    want = np.tril(tl.scale(Sc, c.dh))
    assert sk.same_bytes(c.lower(c.T_raw), want)
    if name == "eight_identity_row":
        i = 9 * 3 + 6
        assert dead[i] and c.lower(c.T_raw)[i, i] == 1 and not np.delete(c.lower(c.T_raw)[i], i).any()
    if name in ("singletons", "one_aggregate"):
        # camera 0 is held entirely, camera 1 holds its scalar 3 and the last camera sees nothing: as singletons 9 + 1 + 9 coarse scalars are dead; in one aggregate none shows
        assert int(dead.sum()) == (19 if name == "singletons" else 0)


@pytest.mark.parametrize("name", CASES)
def test_factor_and_inverse_within_highams_bounds(cases, name):
    """T = L L^T and L Z = D componentwise; Z S_c Z^T = I on the live scalars to the first-order bound of the module's docstring; Z lower triangular with zero padding,
    Zt its transpose bit for bit; zero rows and columns at the identity's scalars; info 0 and no failed factor counted"""
    c = cases(name)
    n = c.n
    assert int(c.words[0]) == 0 and int(c.words[2]) == 5
    T, Lf = c.lower(c.T_raw).astype(np.float64), c.lower(c.L_raw).astype(np.float64)
    Z = c.Z[:, :n].astype(np.float64)
    assert not np.triu(c.Z[:, :n], 1).any() and not c.Z[:, n:].any() and sk.same_bytes(c.Zt[:, :n], c.Z[:, :n].T)
    aL = np.abs(Lf)
    f = np.abs(np.tril(T - Lf @ Lf.T)) / (2 * gamma(n + 1) * (aL @ aL.T) + 1e-300)
    D = np.diag(c.dh.astype(np.float64))
    floor = 4 * n * 2.0 ** -126 * (1 + aL.max())      # (entries of Z far from the diagonal of a banded L fall below the normal range: an absolute error per operation there)
    s = np.abs(D - Lf @ Z) / (2 * gamma(n) * (aL @ np.abs(Z)) + floor)
    print("two-level", name, "n_c", n, "largest multiples: factor", float(f[np.tril_indices(n)].max()), "forward sweep", float(s.max()))
    assert f[np.tril_indices(n)].max() <= 1.0 and s.max() <= 1.0
    live = c.dh > 0
    assert not c.Z[~live].any() and not c.Z[:, :n][:, ~live].any()
    li = np.nonzero(live)[0]
    Sc = c.lower(c.Sc_raw).astype(np.float64); Sc = Sc + np.tril(Sc, -1).T
    Ll, Zl, Tl, dl = Lf[np.ix_(li, li)], Z[np.ix_(li, li)], (T + np.tril(T, -1).T)[np.ix_(li, li)], c.dh[li].astype(np.float64)
    Li = np.abs(np.linalg.inv(Ll))
    cross = (2 * gamma(n) * (np.abs(Ll) @ np.abs(Zl)) + floor) @ (np.abs(Tl) / dl[:, None])
    mid = 2 * gamma(n + 1) * (np.abs(Ll) @ np.abs(Ll).T) + 2.01 * EPS * np.abs(Tl) + cross + cross.T
    bound = 1.01 * (Li @ mid @ Li.T)
    E = np.abs(Zl @ Sc[np.ix_(li, li)] @ Zl.T - np.eye(len(li)))
    print("two-level", name, "Z S_c Z^T - I: largest entry", float(E.max()), "largest multiple of the bound", float((E / bound).max()))
    assert (E <= bound + 1e-300).all()


def test_a_factor_that_failed_gives_a_zero_z_and_counts(torch, L, cases):
    """the packing launch reads the info word on the device: non-zero -> Z and Zt all zero, the counter goes up by one; the apply then leaves z's bits and partials of
    exactly 0; the next good factor gives Z again"""
    c = cases("eight_identity_row")
    P = lambda k: c.d[k].data_ptr()
    n, ld = c.n, c.ld
    w = host(c.d["words"], 4, np.uint32); w[0] = 7
    c.d["words"].copy_(dev(torch, w, np.uint32))
    assert L.thallo_hip_ba_coarse_inverse(C.byref(c.ct), P("panels"), None) == 0
    torch.cuda.synchronize()
    assert not host(c.d["Z"], n * ld).any() and not host(c.d["Zt"], n * ld).any()
    assert host(c.d["words"], 4, np.uint32).tolist() == [7, int(c.words[1]), 6, 0]
    rng = np.random.default_rng(5)
    r, z0 = rng.standard_normal(9 * c.C).astype(F32), rng.standard_normal(9 * c.C).astype(F32)
    rd, zd, part = dev(torch, r), dev(torch, z0), sk.canary_buf(torch, 80)
    nb = L.thallo_hip_ba_coarse_apply(C.byref(c.ct), rd.data_ptr(), zd.data_ptr(), part.data_ptr(), None, None)
    torch.cuda.synchronize()
    ph = part.cpu().numpy()
    assert nb == min((n + 3) // 4, 64) and sk.written_slots(ph.reshape(-1, 1)) == nb and not ph[:nb].any() and sk.same_bytes(host(zd, 9 * c.C), z0)
    w[0] = 0; w[2] = 5
    c.d["words"].copy_(dev(torch, w, np.uint32))
    assert L.thallo_hip_ba_coarse_inverse(C.byref(c.ct), P("panels"), None) == 0
    torch.cuda.synchronize()
    assert sk.same_bytes(host(c.d["Z"], n * ld).reshape(n, ld), c.Z) and sk.same_bytes(host(c.d["Zt"], n * ld).reshape(n, ld), c.Zt)
    assert host(c.d["words"], 4, np.uint32).tolist() == c.words.tolist()


# ------------------------------------------------------------------ 2. the applies
def vector_apply(torch, L, c, r, z0):
    rd, zd, part = dev(torch, r), dev(torch, z0), sk.canary_buf(torch, 80)
    nb = L.thallo_hip_ba_coarse_apply(C.byref(c.ct), rd.data_ptr(), zd.data_ptr(), part.data_ptr(), None, None)
    torch.cuda.synchronize()
    ph = part.cpu().numpy()
    assert nb == min((c.n + 3) // 4, 64) and sk.written_slots(ph.reshape(-1, 1)) == nb and sk.same_bytes(host(rd, 9 * c.C), r)
    return host(zd, 9 * c.C), ph[:nb].copy(), host(c.d["y"], c.n)


@pytest.mark.parametrize("name", CASES)
def test_vector_apply_and_its_partials(torch, L, cases, name):
    """z += P Z^T Z P^T r against float64 from the device's own Z within 4 e32; rows of held scalars exactly zero (and z's own bits where it held something); the partials
    add up to y . y of the device's own y; z + t is one rounded addition; two runs the same bits; a gate word that is set: nothing is written"""
    c = cases(name)
    n, nC = c.n, 9 * c.C
    r = np.random.default_rng([3, c.n]).standard_normal(nC).astype(F32)
    zero = np.zeros(nC, F32)
    t, part, y = vector_apply(torch, L, c, r, zero)
    Z64 = c.Z[:, :n].astype(np.float64)
    y64 = Z64 @ (c.P64.T @ r.astype(np.float64))
    ref = c.P64 @ (Z64.T @ y64)
    m32, y32, p32 = tl.apply32(c.Z[:, :n], c.Zt[:, :n], c.mem_ptr, c.mem, r, c.hold_c)
    _bar(name, "P Z^T Z P^T r", rel_max(t, ref), rel_max(m32, ref))
    _bar(name, "y = Z P^T r", rel_max(y, y64), rel_max(y32, y64))
    held = np.zeros(nC, bool) if c.hold_c is None else c.hold_c.ravel()
    assert not t[held].any()
    trips = -(-n // (4 * len(part)))
    terms = float((y.astype(np.float64) ** 2).sum())
    err = abs(float(part.astype(np.float64).sum()) - terms)
    print("two-level", name, "y . y partials:", len(part), "error / bar", err / ((trips + 6) * EPS * terms))
    assert len(p32) == len(part) and err <= (trips + 6) * EPS * terms
    z0 = np.random.default_rng([4, c.n]).standard_normal(nC).astype(F32)
    z, part2, _ = vector_apply(torch, L, c, r, z0)
    assert sk.same_bytes(z, (z0 + t).astype(F32)) and sk.same_bytes(z[held], z0[held]) and sk.same_bytes(part, part2)
    again, part3, _ = vector_apply(torch, L, c, r, zero)
    assert sk.same_bytes(again, t) and sk.same_bytes(part3, part)
    gate = dev(torch, np.array([1, 0], np.uint32), np.uint32)
    rd, zd, pg = dev(torch, r), dev(torch, z0), sk.canary_buf(torch, 80)
    assert L.thallo_hip_ba_coarse_apply(C.byref(c.ct), rd.data_ptr(), zd.data_ptr(), pg.data_ptr(), gate.data_ptr(), None) == len(part)
    torch.cuda.synchronize()
    assert sk.same_bytes(host(zd, nC), z0) and sk.written_slots(pg.cpu().numpy().reshape(-1, 1)) == 0


def panel_apply(torch, L, c, R, Z0, frozen=None):
    n, pn = c.n, 9 * c.C * K
    g = min(n, 256)
    Rd, Zd, part = dev(torch, R.reshape(pn)), dev(torch, Z0.reshape(pn)), sk.canary_buf(torch, (g + 2) * K)
    work = dev(torch, np.full(int(L.thallo_hip_ba_coarse_cols_work_floats(n)), np.nan))
    fz = None if frozen is None else dev(torch, np.asarray(frozen, np.uint32), np.uint32)
    nb = L.thallo_hip_ba_coarse_apply_cols(C.byref(c.ct), work.data_ptr(), Rd.data_ptr(), Zd.data_ptr(), None if fz is None else fz.data_ptr(), part.data_ptr(), None)
    torch.cuda.synchronize()
    ph = part.cpu().numpy().reshape(-1, K)
    assert nb == g and sk.written_slots(ph) == g and sk.same_bytes(host(Rd, pn), R.reshape(pn))
    return host(Zd, pn).reshape(c.C, 9, K), ph[:g].copy(), host(work, 2 * n * K)[n * K:].reshape(n, K)


@pytest.mark.parametrize("name", CASES)
def test_panel_apply(torch, L, cases, name):
    """the covariance's panel form, a lane per column: against float64 within 4 e32; a column alone (its companions zero) is the column of the full batch bit for bit; a
    zero column stays zero; it equals the vector form within the two bars; the partials per column add up to the device's own y . y; a frozen column is not touched and
    leaves zero partials; two runs the same bits"""
    c = cases(name)
    n, C_ = c.n, c.C
    R = np.random.default_rng([7, n]).standard_normal((C_, 9, K)).astype(F32)
    R[:, :, 5] = 0
    zero = np.zeros_like(R)
    T, part, Y = panel_apply(torch, L, c, R, zero)
    Z64 = c.Z[:, :n].astype(np.float64)
    Y64 = Z64 @ (c.P64.T @ R.reshape(9 * C_, K).astype(np.float64))
    ref = (c.P64 @ (Z64.T @ Y64)).reshape(C_, 9, K)
    m32, Y32 = tl.apply_cols32(c.Z[:, :n], c.Zt[:, :n], c.mem_ptr, c.mem, R, c.hold_c)
    e_cols = rel_max(m32, ref)
    _bar(name, "panel P Z^T Z P^T R", rel_max(T, ref), e_cols)
    assert not T[:, :, 5].any() and not part[:, 5].any()
    if c.hold_c is not None: assert not T[c.hold_c].any()
    rows = -(-n // len(part))
    terms = (Y.astype(np.float64) ** 2).sum(0)
    err = np.abs(part.astype(np.float64).sum(0) - terms)
    live = terms > 0
    print("two-level", name, "panel y . y partials: worst error / bar", float((err[live] / ((rows + 6) * EPS * terms[live])).max()))
    assert (err <= (rows + 6) * EPS * terms).all()
    for k in (0, 41):
        R1 = np.zeros_like(R); R1[:, :, k] = R[:, :, k]
        T1, p1, _ = panel_apply(torch, L, c, R1, zero)
        assert sk.same_bytes(T1[:, :, k], T[:, :, k]) and not np.delete(T1, k, 2).any() and sk.same_bytes(p1[:, k], part[:, k]) and not np.delete(p1, k, 1).any()
        rk = np.ascontiguousarray(R[:, :, k]).ravel()
        one, _, _ = vector_apply(torch, L, c, rk, np.zeros(9 * C_, F32))
        refk = ref[:, :, k].ravel()
        e_one = rel_max(tl.apply32(c.Z[:, :n], c.Zt[:, :n], c.mem_ptr, c.mem, rk, c.hold_c)[0], refk)
        ek = rel_max(m32[:, :, k].ravel(), refk)
        got = float(np.abs(T[:, :, k].ravel().astype(np.float64) - one).max() / np.abs(refk).max())
        print("two-level", name, "column", k, "panel vs vector apply", got, "= %.2f of the summed bars" % (got / (4 * (e_one + ek))))
        assert got <= 4 * e_one + 4 * ek
    Z0 = np.random.default_rng([8, n]).standard_normal((C_, 9, K)).astype(F32)
    frozen = np.zeros(K, np.uint32); frozen[[3, 10]] = 1
    Zf, pf, _ = panel_apply(torch, L, c, R, Z0, frozen)
    fz = frozen != 0
    assert sk.same_bytes(Zf[:, :, fz], Z0[:, :, fz]) and not pf[:, fz].any() and sk.same_bytes(pf[:, ~fz], part[:, ~fz])
    assert sk.same_bytes(Zf[:, :, ~fz], (Z0 + T).astype(F32)[:, :, ~fz])
    again, pa, _ = panel_apply(torch, L, c, R, zero)
    assert sk.same_bytes(again, T) and sk.same_bytes(pa, part)


# ------------------------------------------------------------------ 3. the covariance's column solve
@pytest.mark.parametrize("name", ["six_pairs", "default_greedy", "singletons"])
def test_column_solve_with_the_coarse_operands(torch, L, cases, name):
    """thallo_hip_ba_cov_solve_coarse under the defaults: camera blocks against float64 inv(S_FF) of the device's own S within 4 x the column mirror's error; every column
    converged; never more iterations than the block-Jacobi driver on the same instance; held rows exactly zero, bitwise symmetric, a second run the same bits, one camera
    alone the same camera among seven; with NULL operands it is thallo_hip_ba_cov_solve bit for bit"""
    c = cases(name)
    A = c.sys.cov
    work = torch.zeros(int(L.thallo_hip_ba_cov_coarse_work_bytes(A.C, c.n)) // 4 + 64, dtype=torch.float32, device="cuda")

    def solve(ids, coarse=True, max_it=500):
        idd, out, info = dev(torch, ids, np.int32), dev(torch, np.full(len(ids) * 81, np.nan)), InfoT()
        rc = L.thallo_hip_ba_cov_solve_coarse(C.byref(A.sys), C.byref(c.ct) if coarse else None, 0, idd.data_ptr(), len(ids), 1e-6, max_it, work.data_ptr(), None, out.data_ptr(),
                                              C.byref(info), None)
        assert rc == 0, rc
        return host(out, len(ids) * 81).reshape(len(ids), 9, 9), info
    free = A.free_c.reshape(-1, 9)[A.cams]
    ref = cm.blocks_of(A.Sig_cc, A.cams, 9)
    Bd, info = solve(A.cams)
    Bb, ib = solve(A.cams, coarse=False)
    old, io = A.solve(torch, L, 0, A.cams)
    assert sk.same_bytes(Bb, old) and ib.iterations == io.iterations
    co = tl.Coarse(c.sys.st, c.sys.S, c.agg, c.hold_c, F32)
    Bm, im = tl.two_level_column_pcg(A.pcg, co).solve(0, A.cams)
    e_dev, e_mir, e_blk = cm.cov_error(Bd, ref, free), cm.cov_error(Bm, ref, free), cm.cov_error(Bb, ref, free)
    print("two-level", name, "column solve: mirror error", e_mir, "device", e_dev, "= %.2f x" % (e_dev / e_mir), "(block Jacobi", e_blk, ") iterations", info.iterations, "block Jacobi",
          ib.iterations, "mirror", im["iterations"], "worst", info.worst)
    assert info.not_converged == 0 and info.columns == int(free.sum()) and info.nan_blocks == 0 and 0 < info.worst <= 1e-6
    assert info.iterations <= ib.iterations
    assert e_mir > 0 and e_dev <= 4 * e_mir
    assert sk.same_bytes(Bd, np.transpose(Bd, (0, 2, 1)))
    again, _ = solve(A.cams)
    assert sk.same_bytes(again, Bd)
    k = len(A.cams) // 2
    alone, _ = solve([A.cams[k]])
    assert sk.same_bytes(alone[0], Bd[k])


# ------------------------------------------------------------------ 4. through the C ABI
def tl_plan(d3, p, lm, mask, loss=None, precond="two_level", solver="schur_explicit_pcg", k=None, agg=None, solver_first=True, **sp):
    d = to_device(copy_params(p))
    s = api.ThalloSolver(d3, thallo_amd.energy_file("bundle_adjustment"), solverkind="levenberg_marquardt" if lm else "gauss_newton")
    if lm: s.enable_lm()
    if solver and solver_first: s.set_linear_solver(solver)
    for pc in ([precond] if isinstance(precond, str) else precond or []): s.set_preconditioner(pc)
    if solver and not solver_first: s.set_linear_solver(solver)
    if k is not None or agg is not None: s.set_coarse_aggregates(k, agg)
    if loss: s.set_robust_loss(loss, 2.0)
    if mask is not None:
        s.hold(0, mask[:9 * d3[0]])
        if mask[9 * d3[0]:].any(): s.hold(1, mask[9 * d3[0]:])
    s.set_solver_parameters(**sp)
    params = s.make_params(d)
    s.init(params)
    return s, params, d


def tl_run(d3, p, lm, mask, **kw):
    """-> (costs, PCG iterations per step, cameras, points, schedule name, coarse_space() after the last step, launches by name)"""
    s, params, d = tl_plan(d3, p, lm, mask, **kw)
    assert s.ready(), api.last_error()
    costs, iters = [s.current_cost()], []
    while s.step(params):
        costs.append(s.current_cost()); iters.append(len(s.alpha_beta_trace()))
    out = (np.array(costs), iters, to_host(d[0]).copy(), to_host(d[1]).copy(), s.schedule_name, s.coarse_space(), {k: v["launches"] for k, v in s.kernel_stats().items() if v["launches"]})
    s.close()
    return out


def err_jacobi(orc, d3, p, lm, sp):
    co, _ = orc.Problem(orc.BUNDLE_ADJUST, d3, copy_params(p)).solve(use_lm=1 if lm else 0, **sp)
    cj, *_ = run(d3, p, lm, **sp)
    return float(rel(cj, co).max())


@pytest.mark.parametrize("renumber", ["0", "1"])
@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("dims,band,extras", SHAPES)
def test_trajectories_through_the_c_abi(torch, orc, monkeypatch, dims, band, extras, lm, renumber):
    """GN 3 x 10 and LM 3 x 7 with the gauge held, both point orders: costs per step the two-level mirror's within max(1e-5, 3 err_jacobi); the held scalars keep their
    bits; the schedule name carries the aggregates; no coarse factor failed"""
    p, d3 = problem(dims, band, extras)
    mask = cm.gauge_mask(d3[0], d3[1])
    sp_ = LM if lm else GN
    m = tl.BaTwoLevelMirror(d3, copy_params(p), mask)
    cmir = m.lm_solve(3, 7, q_tolerance=0.1, function_tolerance=0.0)[0] if lm else m.gn_solve(3, 10)
    ej = err_jacobi(orc, d3, p, lm, sp_)
    set_ab(monkeypatch, ba_renumber=renumber)
    cs, its, cams, pts, name, space, stats = tl_run(d3, p, lm, mask, **sp_)
    err = float(rel(cs, cmir).max())
    print("two-level", "LM" if lm else "GN", d3, "renumbered" if renumber == "1" else "caller's order", list(cs), "mirror", cmir, "err_jacobi", ej, "err", err, name, space, its)
    assert len(cs) == len(cmir) == 4 and err <= max(1e-5, 3 * ej)
    Kc = -(-d3[0] // tl.default_k(d3[0])) if d3[0] > 8 else 1
    assert space["aggregates"] >= Kc and space["coarse_scalars"] == 9 * space["aggregates"] and space["failed_factors"] == 0
    assert "assembled (" in name and "two-level on S (%d aggregates, n_c = %d)" % (space["aggregates"], space["coarse_scalars"]) in name and "block-Jacobi on S" not in name
    assert all(stats.get(k, 0) > 0 for k in ("CoarseAssemble", "CoarseScale", "CoarseFactor", "CoarseInverse", "CoarseApply"))
    hold_c = mask[:9 * d3[0]]
    assert sk.same_bytes(cams.reshape(-1)[hold_c], p[0].reshape(-1)[hold_c]) and (cams.reshape(-1)[~hold_c][:9] != p[0].reshape(-1)[~hold_c][:9]).any()
    if extras: assert sk.same_bytes(cams[-1], p[0][-1]) and sk.same_bytes(pts[-2], p[1][-2])      # the camera and the point nothing observes


@pytest.mark.parametrize("lm", [False, True])
def test_it_composes_with_huber_and_a_callers_aggregates(torch, orc, lm):
    """(24, 300, 1200), Huber(2), the gauge held, the caller's aggregates of three consecutive cameras: costs per step the mirror's under the same loss, mask and aggregates"""
    dims, band, _ = SHAPES[1]
    p, d3 = problem(dims, band, False)
    mask = cm.gauge_mask(d3[0], d3[1])
    agg = np.arange(d3[0]) // 3
    sp_ = LM if lm else GN
    m = robust(tl.BaTwoLevelMirror)("huber", 2.0, d3, copy_params(p), mask, agg=agg)
    cmir = m.lm_solve(3, 7, q_tolerance=0.1, function_tolerance=0.0)[0] if lm else m.gn_solve(3, 10)
    ej = err_jacobi(orc, d3, p, lm, sp_)
    cs, its, cams, pts, name, space, _ = tl_run(d3, p, lm, mask, loss="huber", agg=agg, **sp_)
    err = float(rel(cs, cmir).max())
    print("two-level huber", "LM" if lm else "GN", list(cs), "mirror", cmir, "err_jacobi", ej, "err", err, name, space)
    assert len(cs) == len(cmir) == 4 and cs[-1] < cs[0] and err <= max(1e-5, 3 * ej)
    assert space["aggregates"] == 8 and "huber loss, scale 2" in name and "two-level on S (8 aggregates, n_c = 72)" in name
    hold_c = mask[:9 * d3[0]]
    assert sk.same_bytes(cams.reshape(-1)[hold_c], p[0].reshape(-1)[hold_c])


@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("dims,band,extras", SHAPES)
def test_covariance_through_the_c_abi(torch, dims, band, extras, lm):
    """after 3 steps: the blocks of 7 cameras and 21 points against the float64 (A_FF)^-1 of the oracle's J at the device's unknowns within 4 x the two-level column mirror's
    error against the same reference; every column converged; step, covariance, step leaves the bytes of step, step"""
    p, d3 = problem(dims, band, extras)
    C_, P_, _ = d3
    mask = cm.gauge_mask(C_, P_)
    sp_ = dict(LM if lm else GN, nIterations=4)
    runs = []
    for call in (False, True):
        s, params, d = tl_plan(d3, p, lm, mask, **sp_)
        assert s.ready(), api.last_error()
        out = here = None
        for k in range(4):
            assert s.step(params)
            if call and k == 2:
                cams = list(range(min(C_ - 1, 7)))
                pts = list(range(0, P_ - 2, max(1, P_ // 21)))[:21]
                out = s.covariance(params, cameras=cams, points=pts)
                here = [to_host(d[0]).copy(), to_host(d[1]).copy()] + [a.copy() for a in p[2:]]
        runs.append((to_host(d[0]).copy(), to_host(d[1]).copy(), s.current_cost()))
        s.close()
    assert sk.same_bytes(runs[0][0], runs[1][0]) and sk.same_bytes(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    m = BaBlockMirror(d3, here)
    J, sys = cm.system_of(m, mask)
    A = (J.T @ J).toarray()
    free = ~mask & ~cm.undetermined(A, C_)
    Sig = cm.dense_cov64(A, free)
    agg = tl.greedy_aggregates(sys.st, tl.default_k(C_))[0]
    pcg = tl.two_level_column_pcg(cm.ColumnPCG32.of(sys, mask), tl.Coarse(sys.st, sys.S, agg, mask[:9 * C_].reshape(-1, 9), F32))
    info = out["info"]
    for mode, ids, key, dd, off in ((0, cams, "cameras", 9, 0), (1, pts, "points", 3, 9 * C_)):
        got = out[key]
        Bm, im = pcg.solve(mode, ids)
        ok = ~np.isnan(Bm[:, 0, 0])
        refb = cm.blocks_of(Sig, ids, dd, off)
        fr = free[off:off + dd * (C_ if mode == 0 else P_)].reshape(-1, dd)[ids]
        assert (np.isnan(got[:, 0, 0]) == ~ok).all()
        e_dev, e_mir = cm.cov_error(got[ok], refb[ok], fr[ok]), cm.cov_error(Bm[ok], refb[ok], fr[ok])
        print("two-level covariance", d3, "LM" if lm else "GN", key, "mirror error", e_mir, "device", e_dev, "= %.2f x" % (e_dev / e_mir), "mirror iterations", im["batch_iterations"])
        assert sk.same_bytes(got[ok], np.transpose(got[ok], (0, 2, 1)))
        assert e_mir > 0 and e_dev <= 4 * e_mir
    print("two-level covariance", d3, "info", info)
    assert info["not_converged"] == 0 and 0 < info["worst_residual"] <= 1e-6


def test_covariance_at_200_cameras_converges_under_the_defaults(torch):
    """(200, 6000, 26000), band 32, cameras {0, 1} held: the covariance of 7 cameras converges under the default 500 iterations, in no more iterations per batch than the
    CPU study's bound for one unit column allows with its margin (0.75 x block Jacobi's count on the device), and in fewer than block Jacobi takes"""
    d3 = (200, 6000, 26000)
    p = syn.bundle_adjustment(C=d3[0], P=d3[1], O=d3[2], band=32)
    mask = np.zeros(9 * d3[0] + 3 * d3[1], bool); mask[:18] = True
    cams = [2, 50, 100, 101, 150, 198, 199]
    got = {}
    for pc in ("two_level", None):
        s, params, d = tl_plan(d3, p, False, mask, precond=pc, **GN)
        assert s.ready(), api.last_error()
        out = s.covariance(params, cameras=cams)
        got[pc] = out["info"]
        if pc: space = s.coarse_space(); assert space["aggregates"] >= 25 and space["failed_factors"] == 0 and space["identity_rows"] == 0
        else: assert s.coarse_space() is None
        s.close()
    print("two-level covariance at 200 cameras:", got["two_level"], "block Jacobi:", got[None])
    assert got["two_level"]["not_converged"] == 0 and got["two_level"]["worst_residual"] <= 1e-6 and got["two_level"]["iterations"] <= 500
    assert got["two_level"]["iterations"] <= 0.75 * got[None]["iterations"] + 8      # (a batch ends at most a chunk of 8 behind the iteration that froze its last column)


def test_refusals_by_their_messages(torch):
    """Init with linear solver kinds 0 and 1 names both settings, in either order of the setters; a bad aggregate array; a distributed plan; kind 3 ignores the preconditioner"""
    dims, band, _ = SHAPES[0]
    p, d3 = problem(dims, band, False)
    mask = cm.gauge_mask(d3[0], d3[1])
    for solver, word in ((None, "THALLOX_SOLVER_PCG"), ("schur_pcg", "THALLOX_SOLVER_SCHUR_PCG")):
        for first in (True, False):
            s, params, d = tl_plan(d3, p, False, mask, solver=solver, solver_first=first, **GN)
            msg = api.last_error()
            assert not s.ready() and "THALLOX_PRECOND_TWO_LEVEL" in msg and "THALLOX_SOLVER_SCHUR_EXPLICIT_PCG" in msg and word in msg and s.energy_name in msg, msg
            assert s.coarse_space() is None
            s.close()
    s = api.ThalloSolver(d3, thallo_amd.energy_file("bundle_adjustment"))
    for bad, word in ((np.zeros(d3[0] - 1, np.int32), "cameras"), (np.array([0, 0, 1, 1, 3], np.int32), "dense"), (np.array([0, 0, 1, 1, -1], np.int32), "out of range"),
                      (np.array([0, 0, 1, 1, 5], np.int32), "out of range")):
        with pytest.raises(RuntimeError, match="ThalloX_PlanSetCoarseAggregates failed") as e: s.set_coarse_aggregates(aggregates=bad)
        assert word in str(e.value) and s.energy_name in str(e.value), str(e.value)
    with pytest.raises(RuntimeError, match="cameras_per_aggregate"): s.set_coarse_aggregates(-2)
    assert s._L.ThalloX_PlanSetPreconditioner(s.plan, 3) != 0 and "unknown preconditioner kind" in api.last_error()
    s.close()
    s = api.ThalloSolver((48, 32), thallo_amd.energy_file("image_warping"))
    with pytest.raises(RuntimeError, match="no block-Jacobi preconditioner for this energy"): s.set_preconditioner("two_level")
    with pytest.raises(RuntimeError, match="no two-level preconditioner for this energy"): s.set_coarse_aggregates(4)
    s.close()
    s = api.ThalloSolver((8, 72, 330), thallo_amd.energy_file("bundle_adjustment"))      # a distributed plan (one rank's camera shard)
    s.set_distributed(0, 1, 0, 0, device_exchange=False)
    with pytest.raises(RuntimeError, match="distributed"): s.set_preconditioner("two_level")
    s.close()
    s, params, d = tl_plan(d3, p, False, mask, solver="schur_dense", **GN)
    assert s.ready() and "dense Cholesky of S" in s.schedule_name and "two-level" not in s.schedule_name and s.coarse_space() is None
    s.close()


@pytest.mark.parametrize("lm", [False, True])
def test_unchanged_plans_and_a_re_init(torch, lm):
    """a plan that sets two_level and then block_jacobi before Init is the plan that never made the call: costs, iterations, schedule name, launches by name, bytes; a
    two-level plan re-initialised with block_jacobi runs as that plan and reports no coarse space"""
    dims, band, _ = SHAPES[1]
    p, d3 = problem(dims, band, False)
    mask = cm.gauge_mask(d3[0], d3[1])
    sp_ = LM if lm else GN
    never = tl_run(d3, p, lm, mask, precond=None, **sp_)
    back = tl_run(d3, p, lm, mask, precond=["two_level", "block_jacobi"], **sp_)
    assert list(never[0]) == list(back[0]) and never[1] == back[1] and never[4] == back[4] and never[5] is None and back[5] is None and never[6] == back[6]
    assert sk.same_bytes(never[2], back[2]) and sk.same_bytes(never[3], back[3]) and not any(k.startswith("Coarse") for k in back[6])
    assert "block-Jacobi on S" in back[4]
    s, params, d = tl_plan(d3, p, lm, mask, **sp_)
    assert s.ready() and s.coarse_space() is not None and s.step(params)
    s.set_preconditioner("block_jacobi")
    s.set_solver_parameters(trust_region_radius=1e4)      # (an LM step leaves its radius in the solver parameters, as the reference does: a new solve starts from the default again)
    for k, a in enumerate(copy_params(p)[:2]): d[k].copy_(to_device([a])[0])
    s.init(params)
    assert s.ready() and s.coarse_space() is None and "block-Jacobi on S" in s.schedule_name
    costs = [s.current_cost()]
    while s.step(params): costs.append(s.current_cost())
    cams = to_host(d[0]).copy()
    s.close()
    assert costs == list(never[0]) and sk.same_bytes(cams, never[2])
