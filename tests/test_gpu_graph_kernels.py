"""The graph-edge kernels of csrc/energy_graph.hip, entry point by entry point against the float64 references of tests/graph_reference.py.

Every vertex and every edge of every case is compared.  Outputs go into canary-filled buffers (sk.CANARY, a NaN pattern) and everything a launch does not own must
keep it: the entries of vertices outside [n0, n1) on both planes, the ELL padding positions of F and G, the tail behind every buffer, the partial slots behind the
returned count.  The returned count is gr.vgrid(n1 - n0).  Every index handed to a kernel is in range, ELL padding included (gr.build_lists).

Bounds are sk.tol(k, S): S the reference's float64 sum of the absolute values of the terms of that output, k the number of float32 roundings on the longest chain of
operations that leads to it, counted below from the kernel's code as if nothing were contracted into an fma (contraction only removes roundings):

  T       relative error of one device sine / cosine in units of 2^-24: TRIG = 2 x the worst value measured on the MI355X over this file's own angle set
          (profiles/graph_kernels/README.md; the factor 2 because that set is finite)
  K_ROT   = 3 T + 3     an entry of R or of dR/d(angle): at most two products of three trigonometric factors (3 T + 2 each) and their sum
  K_G     = K_ROT + 4   a component of G_e = dR dv: dv = O_a - O_b (1), the product (1), the sum of three (2)
  K_F     = K_G + 2     a component of F_e = w ((P_a - P_b) - R dv): R dv as K_G, P_a - P_b (1, smaller), the subtraction (1), the weight (1)
  K_COST  = 2 K_F + 1 + 3 (maxdeg + 1)    a vertex's cost share: f^2 doubles f's error and rounds once; 3 (deg + 1) squares are added up
  K_R     = 6 + maxdeg + maxin            PCGInit1's r from the stored F, G: a Position entry adds deg + ideg products (1) and the fit term (3) -- 4 + deg + ideg; an
                                          Angle entry adds deg terms w (g.f) (3 products, 2 sums, the weight) -- 6 + deg
  K_D     = 7 + maxdeg + maxin            diag: w^2 (1) added deg + ideg times, + w_fit^2 (2); Angle: w^2 (g.g) (1 + 5 + 1) added deg times
  K_PRE   = K_D + 4                       1 / (1 + sqrt d)^2: d's error passes with a factor sqrt d / (1 + sqrt d) < 1; sqrt, sum, square, quotient (correctly rounded)
  K_Z     = K_PRE + K_R + 1               z = M^-1 r
  K_AP    = 13 + maxdeg + maxin           J^T J p from the stored G: J p per edge = (p_n - p_m) - G p_A is 7 operations; an Angle entry adds deg terms g.(J p) (7 + 1 + 2)
                                          and takes w^2 (2): 12 + deg; a Position entry adds deg + ideg terms (7) and takes w^2 (2) and the fit term (3): 12 + deg + ideg;
                                          one more for the sum with the running value
  K_RC    = K_AP + 2 K_G                  ... with G recomputed: G enters J^T J p twice (J and J^T), each time with K_G on the magnitude G_abs
A partial (one per workgroup) is compared with the float64 sum of the DEVICE's own per-vertex outputs (which the same test has just checked): the terms' products
and sums (stated per test) + one addition per vertex a lane visits + 6 butterfly levels + 4 waves.

The worst observed error / bound ratio per kernel goes to the file THALLO_GRAPH_RATIOS names, when set (that is how profiles/graph_kernels/README.md was filled)."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import graph_reference as gr
import shim_kernels as sk
from shim_kernels import F32

pytestmark = pytest.mark.gpu

TRIG_MEASURED = 2.0346       # worst |sincosf - sin/cos| / (2^-24 |sin/cos|) on the MI355X over all_angles(): 2.03453 (profiles/graph_kernels/README.md)
TRIG = 2.0 * TRIG_MEASURED
K_ROT = 3 * TRIG + 3
K_G = K_ROT + 4
K_F = K_G + 2
PSLOTS = sk.MAX_PARTIALS + 8
TAIL = 64                    # canary words behind every output
EPS64 = 2.0 ** -53

RATIOS = {}


def _note(kernel, err, bound):
    """asserts err <= bound everywhere and keeps the worst ratio"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    bad = ~(err <= bound)                                                   # (NaN counts as bad)
    with np.errstate(all="ignore"):
        ratio = float(np.nanmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))) if err.size else 0.0
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    assert not bad.any(), (kernel, np.flatnonzero(bad.ravel())[:8], ratio)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    return sk.shim()


@pytest.fixture(scope="module", autouse=True)
def _ratios():
    yield
    path = os.environ.get("THALLO_GRAPH_RATIOS")
    if path:
        json.dump(RATIOS, open(path, "w"), indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _stop_at_a_device_fault(torch):
    """a launch that faulted poisons every later one of the process: end the run there instead of reporting its echoes"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error: {e}", returncode=3)


# ------------------------------------------------------------------ cases
SMALL = ["mesh", "deg8", "deg10", "hub", "sparse", "one"]
LAYOUTS = ["csr", "ell"]


def ranges(N):
    """(0, N), (1, N), (100, 257), (N - 1, N): what the multi-GPU partition passes is no multiple of 256"""
    return [r for r in dict.fromkeys([(0, N), (1, N), (100, 257), (N - 1, N)]) if 0 <= r[0] < r[1] <= N]


@functools.lru_cache(maxsize=None)
def problem(name):
    g = gr.GRAPHS[name]()
    inp = gr.arap_inputs(g[0])
    return SimpleNamespace(g=g, N=g[0], inp=inp, ref=gr.ArapRef(g, inp))


def all_angles():
    """every angle this file hands a kernel"""
    return np.concatenate([problem(n).inp.A.ravel() for n in gr.GRAPHS])


def lists(name, layout):
    N, v0, v1 = problem(name).g
    if layout == "csr" or len(v0) == 0:
        return gr.build_lists(N, v0, v1)
    return gr.build_lists(N, v0, v1, *gr.ell_slots(N, v0, v1))


class Dev:
    """one problem in one layout on the device: index lists (4 spare ints behind each, as plugins.cpp uploads them), inputs, and F / G / SC from precompute2"""

    def __init__(self, torch, L, name, layout):
        self.torch, self.L, self.name, self.layout = torch, L, name, layout
        self.pr = problem(name); self.N = self.pr.N; self.inp = self.pr.inp; self.ref = self.pr.ref
        self.ls = ls = lists(name, layout)
        ints = lambda a: sk.dbuf(torch, np.concatenate([a, np.zeros(4, np.int32)]))
        self.out_ptr, self.out_v1, self.in_ptr, self.in_edge, self.in_src = (ints(a) for a in (ls.out_ptr, ls.out_v1, ls.in_ptr, ls.in_edge, ls.in_src))
        self.P, self.A, self.O, self.C = (sk.dbuf(torch, a) for a in (self.inp.P, self.inp.A, self.inp.O, self.inp.C))
        self.wf, self.wr = self.inp.w_fit, self.inp.w_reg
        self.maxdeg, self.maxin = int(ls.odeg.max()), int(ls.ideg.max())
        self.consts = [(t, t.cpu().numpy().copy()) for t in (self.out_ptr, self.out_v1, self.in_ptr, self.in_edge, self.in_src, self.P, self.A, self.O, self.C)]
        self.F = self.G = self.SC = None

    def precompute(self, entry=2):
        """F, G (and SC) into fresh canary buffers; returns the device tensors"""
        ls, t = self.ls, self.torch
        F, G, SC = sk.canary_buf(t, 3 * ls.edges + TAIL), sk.canary_buf(t, 9 * ls.edges + TAIL), sk.canary_buf(t, 6 * self.N + TAIL)
        a = (self.N, self.out_ptr.data_ptr(), self.out_v1.data_ptr(), self.P.data_ptr(), self.A.data_ptr(), self.O.data_ptr(), self.wr, F.data_ptr(), G.data_ptr())
        rc = self.L.thallo_hip_arap_precompute2(*a, SC.data_ptr(), ls.ell_stride, None) if entry == 2 else self.L.thallo_hip_arap_precompute(*a, ls.ell_stride, None)
        t.cuda.synchronize()
        assert rc == 0
        return F, G, SC

    def ready(self):
        if self.F is None:
            self.F, self.G, self.SC = self.precompute()
            self.consts += [(x, x.cpu().numpy().copy()) for x in (self.F, self.G, self.SC)]
            self.Fh = gr.edge_plane(self.ls, self.F.cpu().numpy(), 3).astype(np.float64)                                       # [e, c]
            self.Gh = gr.edge_plane(self.ls, self.G.cpu().numpy(), 9).astype(np.float64).reshape(-1, 3, 3).transpose(0, 2, 1)  # [e, row, col]
        return self

    def inputs_unchanged(self):
        self.torch.cuda.synchronize()
        for t, h in self.consts:
            assert sk.same_bytes(t.cpu().numpy(), h), "a const input changed"


@functools.lru_cache(maxsize=None)
def _dev(torch, L, name, layout):
    return Dev(torch, L, name, layout)


def flat_out(torch, N):
    return sk.canary_buf(torch, 6 * N + TAIL)


def owned(t, N, n0, n1):
    """the entries of a flat output [Position | Angle | tail] that [n0, n1) owns -- and nothing else may have lost the canary"""
    h = t.cpu().numpy()
    m = np.zeros(h.size, bool); m[:6 * N] = gr.planes(h[:6 * N], N, n0, n1)
    assert (h.view(np.uint32)[~m] == sk.CANARY).all(), "written outside the launch's vertex range"
    return h, m


def partial_slots(buf, ret, n0, n1, width=1):
    """the returned count is vgrid(n1 - n0) and exactly that many slots were written; returns them"""
    grid = gr.vgrid(n1 - n0)
    assert ret == grid, (ret, grid)
    h = buf.cpu().numpy().reshape(-1, width) if width > 1 else buf.cpu().numpy()
    assert sk.written_slots(h) == grid
    return h[:grid]


def block_sums(terms, n0, n1):
    return np.bincount(gr.block_of_vertex(n0, n1), weights=np.asarray(terms, np.float64), minlength=gr.vgrid(n1 - n0))


def check_partials(kernel, got, terms, k_terms, N, n0, n1, eps=sk.EPS):
    """one partial per workgroup against the float64 sum of its vertices' terms (`terms`: a flat vector [Position | Angle] or one value per vertex; the magnitude is the
    sum of the absolute values): k_terms roundings inside a vertex's share + one addition per visit + 6 butterfly levels + 4 waves"""
    terms = np.asarray(terms, np.float64)
    tv, ta = (gr.per_vertex(terms, N), gr.per_vertex(np.abs(terms), N)) if terms.size == 6 * N else (terms, np.abs(terms))
    k = k_terms + gr.visits(n0, n1) + 6 + 4
    _note(kernel, np.abs(np.asarray(got, np.float64) - block_sums(tv[n0:n1], n0, n1)), k * eps * block_sums(ta[n0:n1], n0, n1))


def rand_p(N, seed=7):
    return np.random.default_rng([seed, N]).standard_normal(6 * N).astype(F32)


# ------------------------------------------------------------------ sincosf: the one figure the code cannot give
def test_sincos_plane_and_the_measured_trig_error(torch, L):
    """SC = sines | cosines of every vertex's angles against float64 sin / cos of the same float32 angles, in units of 2^-24 of the value.  Prints the worst figure (what
    TRIG_MEASURED records) and holds the device to twice the recorded one."""
    worst, checks = 0.0, []
    for name in gr.GRAPHS:
        d = _dev(torch, L, name, "csr").ready()
        sc = d.SC.cpu().numpy()
        assert (sc[6 * d.N:].view(np.uint32) == sk.CANARY).all()
        want = np.concatenate([d.ref.sin.ravel(), d.ref.cos.ravel()])
        err = np.abs(sc[:6 * d.N].astype(np.float64) - want)
        worst = max(worst, float((err / (sk.EPS * np.abs(want))).max()))
        checks.append((err, sk.tol(TRIG, np.abs(want))))
    RATIOS["sincosf worst relative error in units of 2^-24"] = worst
    print(f"sincosf: worst relative error {worst:.5f} x 2^-24 over {all_angles().size} angles")
    for err, bound in checks:
        _note("sincosf (SC plane)", err, bound)


# ------------------------------------------------------------------ precompute
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SMALL)
def test_arap_precompute(torch, L, name, layout):
    """F_e (K_F on F_abs) and G_e (K_G on G_abs) at the position of every edge; ELL padding and the tails untouched; precompute and precompute2 agree byte for byte."""
    d = _dev(torch, L, name, layout).ready()
    ls, ref = d.ls, d.ref
    Fh, Gh = d.F.cpu().numpy(), d.G.cpu().numpy()
    for arr, w in ((Fh, 3), (Gh, 9)):
        assert (arr[w * ls.edges:].view(np.uint32) == sk.CANARY).all() and (gr.padding_words(ls, arr, w).view(np.uint32) == sk.CANARY).all()
    _note("arap_precompute F", np.abs(d.Fh - ref.F), sk.tol(K_F, ref.F_abs))
    _note("arap_precompute G", np.abs(d.Gh - ref.G), sk.tol(K_G, ref.G_abs))
    F1, G1, SC1 = d.precompute(entry=1)
    assert sk.same_bytes(F1.cpu().numpy(), Fh) and sk.same_bytes(G1.cpu().numpy(), Gh)
    assert (SC1.cpu().numpy().view(np.uint32) == sk.CANARY).all()                           # the entry without SC leaves it alone
    d.inputs_unchanged()


# ------------------------------------------------------------------ cost
def _cost(d, n0, n1):
    out = sk.canary_buf(d.torch, PSLOTS)
    ret = d.L.thallo_hip_arap_cost(d.N, n0, n1, d.out_ptr.data_ptr(), d.out_v1.data_ptr(), d.P.data_ptr(), d.A.data_ptr(), d.O.data_ptr(), d.C.data_ptr(), d.wf, d.wr,
                                   out.data_ptr(), d.ls.ell_stride, None)
    d.torch.cuda.synchronize()
    return partial_slots(out, ret, n0, n1)


@pytest.mark.parametrize("name", SMALL)
def test_arap_cost(torch, L, name):
    """The partials against the float64 cost shares of their vertices (K_COST on the shares' magnitudes), their sum against the float64 cost; ELL and CSR give the same bits."""
    dc, de = _dev(torch, L, name, "csr"), _dev(torch, L, name, "ell")
    t, m = dc.ref.cost_terms()
    for n0, n1 in ranges(dc.N):
        got = _cost(dc, n0, n1)
        k = 2 * K_F + 1 + 3 * (dc.maxdeg + 1) + gr.visits(n0, n1) + 6 + 4
        _note("arap_cost partials", np.abs(got.astype(np.float64) - block_sums(t[n0:n1], n0, n1)), sk.tol(k, block_sums(m[n0:n1], n0, n1)))
        _note("arap_cost sum", abs(float(sk.sum_partials(got)) - t[n0:n1].sum()), sk.tol(k + 16 + 6, m[n0:n1].sum()))      # + the documented sum: 16 per lane, 6 levels
        assert sk.same_bytes(_cost(de, n0, n1), got)
    dc.inputs_unchanged(); de.inputs_unchanged()


# ------------------------------------------------------------------ PCGInit1
def _init(d, n0, n1, with_diag):
    t, N = d.torch, d.N
    o = SimpleNamespace(**{k: flat_out(t, N) for k in ("r", "pre", "z", "p_prev", "delta", "diag")}, aN=sk.canary_buf(t, PSLOTS))
    ret = d.L.thallo_hip_arap_pcg_init(N, n0, n1, d.out_ptr.data_ptr(), d.in_ptr.data_ptr(), d.in_edge.data_ptr(), d.P.data_ptr(), d.C.data_ptr(), d.F.data_ptr(), d.G.data_ptr(),
                                       d.wf, d.wr, o.r.data_ptr(), o.pre.data_ptr(), o.z.data_ptr(), o.p_prev.data_ptr(), o.delta.data_ptr(),
                                       o.diag.data_ptr() if with_diag else None, o.aN.data_ptr(), d.ls.ell_stride, None)
    t.cuda.synchronize()
    o.ret = ret
    return o


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SMALL)
def test_arap_pcg_init(torch, L, name, layout):
    """r, M^-1, z, diag and the alphaN partials against float64 built from the device's own F and G (so only this kernel's roundings count); zeros in p_prev and delta on
    the range only; diag_out NULL changes nothing else; ELL and CSR give the same bits."""
    d = _dev(torch, L, name, layout).ready()
    N = d.N
    s = d.ref.system(F=d.Fh, G=d.Gh)
    k_r, k_d = 6 + d.maxdeg + d.maxin, 7 + d.maxdeg + d.maxin
    other = _dev(torch, L, name, "csr").ready() if layout == "ell" else None
    for n0, n1 in ranges(N):
        o = _init(d, n0, n1, True)
        h = {}
        for key in ("r", "pre", "z", "p_prev", "delta", "diag"):
            arr, m = owned(getattr(o, key), N, n0, n1)
            h[key] = arr[:6 * N]; own = m[:6 * N]
        f = lambda key: h[key][own].astype(np.float64)
        _note("arap_pcg_init r", np.abs(f("r") - s.r[own]), sk.tol(k_r, s.r_abs[own]))
        _note("arap_pcg_init diag", np.abs(f("diag") - s.diag[own]), sk.tol(k_d, s.diag[own]))
        _note("arap_pcg_init pre", np.abs(f("pre") - s.pre[own]), sk.tol(k_d + 4, s.pre[own]))
        _note("arap_pcg_init z", np.abs(f("z") - s.z[own]), sk.tol(k_d + 4 + k_r + 1, s.pre[own] * s.r_abs[own]))
        assert not h["p_prev"][own].view(np.uint32).any() and not h["delta"][own].view(np.uint32).any()
        rz = np.zeros(6 * N); rz[own] = f("r") * f("z")
        got = partial_slots(o.aN, o.ret, n0, n1)
        check_partials("arap_pcg_init alphaN partials", got, rz, 1 + 5, N, n0, n1)     # six products (1) and their sum (5)
        o2 = _init(d, n0, n1, False)
        for key in ("r", "pre", "z", "p_prev", "delta", "aN"):
            assert sk.same_bytes(getattr(o2, key).cpu().numpy(), getattr(o, key).cpu().numpy()), key
        assert (o2.diag.cpu().numpy().view(np.uint32) == sk.CANARY).all() and o2.ret == o.ret
        if other is not None:
            oc = _init(other, n0, n1, True)
            for key in ("r", "pre", "z", "diag", "aN"):
                assert sk.same_bytes(getattr(oc, key).cpu().numpy(), getattr(o, key).cpu().numpy()), key
    d.inputs_unchanged()


# ------------------------------------------------------------------ applyJTJ
def _apply(d, form, n0, n1, p, r=None, pre=None, fin_aN=None):
    """form: "plain" (apply_jtj), "sums", "fin" (sums_fin with tickets), "rc", "rc_fin"; returns Ap, aD, s3 (device tensors), the two words and the return code"""
    t, N, ls = d.torch, d.N, d.ls
    o = SimpleNamespace(Ap=flat_out(t, N), aD=sk.canary_buf(t, PSLOTS), s3=sk.canary_buf(t, 3 * PSLOTS, np.float64), words=sk.canary_buf(t, 2 + TAIL),
                        tickets=sk.dbuf(t, np.zeros(sk.FIN_TICKET_WORDS, np.uint32)))
    head = (N, n0, n1, d.out_ptr.data_ptr(), d.out_v1.data_ptr(), d.in_ptr.data_ptr())
    fin = sk.NO_FIN
    if form in ("fin", "rc_fin"):
        o.aNt = sk.dbuf(t, np.array([fin_aN], F32))
        fin = sk.FinT(sk.sumt(o.aNt), o.tickets.data_ptr(), o.words.data_ptr(), o.words.data_ptr() + 4)
    sums = (r.data_ptr(), pre.data_ptr(), o.s3.data_ptr()) if r is not None else (None, None, None)
    if form in ("rc", "rc_fin"):
        o.ret = d.L.thallo_hip_arap_apply_jtj_rc(*head, d.in_src.data_ptr(), d.C.data_ptr(), d.O.data_ptr(), d.SC.data_ptr(), d.wf, d.wr, p.data_ptr(), o.Ap.data_ptr(),
                                                 o.aD.data_ptr(), ls.ell_stride, *sums, fin, None)
    else:
        mid = (d.in_edge.data_ptr(), d.in_src.data_ptr(), d.C.data_ptr(), d.G.data_ptr(), d.wf, d.wr, p.data_ptr(), o.Ap.data_ptr(), o.aD.data_ptr(), ls.ell_stride)
        if form == "plain": o.ret = d.L.thallo_hip_arap_apply_jtj(*head, *mid, None)
        elif form == "sums": o.ret = d.L.thallo_hip_arap_apply_jtj_sums(*head, *mid, *sums, None)
        else: o.ret = d.L.thallo_hip_arap_apply_jtj_sums_fin(*head, *mid, *sums, fin, None)
    t.cuda.synchronize()
    return o


def _check_apply(kernel, d, o, n0, n1, ph, want, want_abs, k, rh=None, preh=None, fin_aN=None):
    """Ap on the range (k on want_abs), the alphaD partials, and with rh / preh the double sums {N, S1, S2} and (fin_aN) the two scalar words"""
    N = d.N
    arr, m = owned(o.Ap, N, n0, n1)
    own = m[:6 * N]
    Ap = arr[:6 * N].astype(np.float64)
    _note(kernel + " Ap", np.abs(Ap[own] - want[own]), sk.tol(k, want_abs[own]))
    Apz = np.where(own, Ap, 0.0)
    aD = partial_slots(o.aD, o.ret, n0, n1)
    check_partials(kernel + " alphaD partials", aD, ph.astype(np.float64) * Apz, 1 + 5, N, n0, n1)
    if rh is None:
        assert (o.s3.cpu().numpy().view(np.uint32) == sk.CANARY).all()
        return arr, aD, None
    s3 = partial_slots(o.s3, o.ret, n0, n1, 3)
    r64, m64 = rh.astype(np.float64), preh.astype(np.float64)
    for j, terms in enumerate((m64 * r64 * r64, m64 * r64 * Apz, m64 * Apz * Apz)):       # exact products of float data in double: 2 roundings of 2^-53, then the sums
        check_partials(kernel + " {N, S1, S2}", s3[:, j], np.where(own, terms, 0.0), 2 + 5, N, n0, n1, eps=EPS64)
    if fin_aN is not None:
        w = o.words.cpu().numpy()
        assert (w[2:].view(np.uint32) == sk.CANARY).all() and not o.tickets.cpu().numpy().any()
        adw, alpha, bnw, mag = sk.ref_scalars_finish(aD, s3.ravel(), F32(fin_aN))
        assert sk.same_bytes(w[0:1], adw)
        if float(bnw) > 0: assert mag / float(bnw) < 2.0 ** 20
        assert sk.ulp_apart(w[1], bnw) <= 1, (w[1], bnw)
    else:
        assert (o.words.cpu().numpy().view(np.uint32) == sk.CANARY).all()
    return arr, aD, s3


def _vectors(d):
    rng = np.random.default_rng([11, d.N])
    ph, rh, preh = rand_p(d.N), rng.standard_normal(6 * d.N).astype(F32), rng.uniform(0.25, 2.0, 6 * d.N).astype(F32)
    return ph, rh, preh, sk.dbuf(d.torch, ph), sk.dbuf(d.torch, rh), sk.dbuf(d.torch, preh)


FIN_AN = 0.01      # alphaN handed to the in-kernel finish: alpha small, so betaN = N - 2 alpha S1 + alpha^2 S2 stays near N > 0 (no cancellation; asserted)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SMALL)
def test_arap_apply_jtj_stored_g(torch, L, name, layout):
    """thallo_hip_arap_apply_jtj, _sums and _sums_fin against float64 J^T J p built from the device's G (K_AP): the three agree on Ap and the alphaD partials byte for
    byte, _sums and _sums_fin on {N, S1, S2}; the unrolled ELL form (out-slots <= 8; on `hub` the in-lists have 10) equals the loop form bit for bit, and ELL equals CSR."""
    d = _dev(torch, L, name, layout).ready()
    N = d.N
    ph, rh, preh, p, r, pre = _vectors(d)
    want, want_abs = d.ref.apply(ph, G=d.Gh)
    k = 13 + d.maxdeg + d.maxin
    other = _dev(torch, L, name, "csr").ready() if layout == "ell" else None
    for n0, n1 in ranges(N):
        o1 = _apply(d, "plain", n0, n1, p)
        A1, aD1, _ = _check_apply("arap_apply_jtj", d, o1, n0, n1, ph, want, want_abs, k)
        o2 = _apply(d, "sums", n0, n1, p, r, pre)
        A2, aD2, s2 = _check_apply("arap_apply_jtj_sums", d, o2, n0, n1, ph, want, want_abs, k, rh, preh)
        o3 = _apply(d, "fin", n0, n1, p, r, pre, FIN_AN)
        A3, aD3, s3 = _check_apply("arap_apply_jtj_sums_fin", d, o3, n0, n1, ph, want, want_abs, k, rh, preh, FIN_AN)
        assert sk.same_bytes(A1, A2) and sk.same_bytes(A1, A3) and sk.same_bytes(aD1, aD2) and sk.same_bytes(aD1, aD3) and sk.same_bytes(s2, s3)
        if layout == "ell":
            L.thallo_hip_arap_debug_set(0, 0)
            try:
                ol = _apply(d, "sums", n0, n1, p, r, pre)
            finally:
                L.thallo_hip_arap_debug_set(0, 1)
            Al, aDl, sl = _check_apply("arap_apply_jtj (loop form on ELL)", d, ol, n0, n1, ph, want, want_abs, k, rh, preh)
            assert sk.same_bytes(Al, A2) and sk.same_bytes(aDl, aD2) and sk.same_bytes(sl, s2), "the unrolled ELL form differs from the loop form"
            oc = _apply(other, "sums", n0, n1, p, r, pre)
            assert sk.same_bytes(oc.Ap.cpu().numpy(), A2) and sk.same_bytes(oc.aD.cpu().numpy(), o2.aD.cpu().numpy()) and sk.same_bytes(oc.s3.cpu().numpy(), o2.s3.cpu().numpy())
    d.inputs_unchanged()
    for t, h in ((p, ph), (r, rh), (pre, preh)): assert sk.same_bytes(t.cpu().numpy(), h)


@pytest.mark.parametrize("name", ["mesh", "deg8", "hub", "sparse"])
def test_arap_apply_jtj_recomputed_g(torch, L, name):
    """thallo_hip_arap_apply_jtj_rc (ELL, at most 8 out-slots; `deg8` takes <8>, `hub` has 10 in-slots) against float64 J^T J p built from the ANGLES: K_RC on the magnitudes
    with G_abs.  Against the stored-G form the code claims agreement to rounding only: no bit claim is made here."""
    d = _dev(torch, L, name, "ell").ready()
    N = d.N
    assert L.thallo_hip_arap_recompute_supported(N, d.ls.ell_stride) == 1
    ph, rh, preh, p, r, pre = _vectors(d)
    want, want_abs = d.ref.apply(ph, G_abs=d.ref.G_abs)
    k = 13 + d.maxdeg + d.maxin + 2 * K_G
    for n0, n1 in ranges(N):
        o1 = _apply(d, "rc", n0, n1, p)
        A1, aD1, _ = _check_apply("arap_apply_jtj_rc", d, o1, n0, n1, ph, want, want_abs, k)
        o2 = _apply(d, "rc", n0, n1, p, r, pre)
        A2, aD2, s2 = _check_apply("arap_apply_jtj_rc", d, o2, n0, n1, ph, want, want_abs, k, rh, preh)
        o3 = _apply(d, "rc_fin", n0, n1, p, r, pre, FIN_AN)
        A3, aD3, s3 = _check_apply("arap_apply_jtj_rc", d, o3, n0, n1, ph, want, want_abs, k, rh, preh, FIN_AN)
        assert sk.same_bytes(A1, A2) and sk.same_bytes(A1, A3) and sk.same_bytes(aD1, aD2) and sk.same_bytes(aD1, aD3) and sk.same_bytes(s2, s3)
    d.inputs_unchanged()


def test_arap_refusals(torch, L):
    d = _dev(torch, L, "mesh", "ell").ready()
    N, S = d.N, d.ls.ell_stride
    ph, rh, preh, p, r, pre = _vectors(d)
    buf = flat_out(torch, N); part = sk.canary_buf(torch, PSLOTS); s3 = sk.canary_buf(torch, 3 * PSLOTS, np.float64)
    for n0, n1, ell in ((5, 5, S), (7, 3, S), (0, N + 1, S), (0, N, -1)):
        assert L.thallo_hip_arap_cost(N, n0, n1, d.out_ptr.data_ptr(), d.out_v1.data_ptr(), d.P.data_ptr(), d.A.data_ptr(), d.O.data_ptr(), d.C.data_ptr(), d.wf, d.wr,
                                      part.data_ptr(), ell, None) == sk.INVALID
        assert L.thallo_hip_arap_pcg_init(N, n0, n1, d.out_ptr.data_ptr(), d.in_ptr.data_ptr(), d.in_edge.data_ptr(), d.P.data_ptr(), d.C.data_ptr(), d.F.data_ptr(),
                                          d.G.data_ptr(), d.wf, d.wr, *[buf.data_ptr()] * 6, part.data_ptr(), ell, None) == sk.INVALID
        head = (N, n0, n1, d.out_ptr.data_ptr(), d.out_v1.data_ptr(), d.in_ptr.data_ptr(), d.in_edge.data_ptr(), d.in_src.data_ptr(), d.C.data_ptr(), d.G.data_ptr(), d.wf, d.wr,
                p.data_ptr(), buf.data_ptr(), part.data_ptr(), ell)
        assert L.thallo_hip_arap_apply_jtj(*head, None) == sk.INVALID
        assert L.thallo_hip_arap_apply_jtj_sums(*head, r.data_ptr(), pre.data_ptr(), s3.data_ptr(), None) == sk.INVALID
    assert L.thallo_hip_arap_precompute2(N, d.out_ptr.data_ptr(), d.out_v1.data_ptr(), d.P.data_ptr(), d.A.data_ptr(), d.O.data_ptr(), d.wr, d.F.data_ptr(), d.G.data_ptr(),
                                         None, -1, None) == sk.INVALID
    head = (N, 0, N, d.out_ptr.data_ptr(), d.out_v1.data_ptr(), d.in_ptr.data_ptr(), d.in_edge.data_ptr(), d.in_src.data_ptr(), d.C.data_ptr(), d.G.data_ptr(), d.wf, d.wr,
            p.data_ptr(), buf.data_ptr(), part.data_ptr(), S)
    for args in ((None, pre.data_ptr(), s3.data_ptr()), (r.data_ptr(), None, s3.data_ptr()), (r.data_ptr(), pre.data_ptr(), None)):
        assert L.thallo_hip_arap_apply_jtj_sums_fin(*head, *args, sk.NO_FIN, None) == sk.INVALID
    rc_head = (N, 0, N, d.out_ptr.data_ptr(), d.out_v1.data_ptr(), d.in_ptr.data_ptr(), d.in_src.data_ptr(), d.C.data_ptr(), d.O.data_ptr(), d.SC.data_ptr(), d.wf, d.wr,
               p.data_ptr(), buf.data_ptr(), part.data_ptr())
    for ell in (0, S + 1, 9 * N):                                      # CSR, no multiple of N, more than 8 slots
        assert L.thallo_hip_arap_apply_jtj_rc(*rc_head, ell, None, None, None, sk.NO_FIN, None) == sk.NOT_SUPPORTED
        assert L.thallo_hip_arap_recompute_supported(N, ell) == 0
    d10 = _dev(torch, L, "deg10", "ell")
    assert d10.ls.out_slots > 8 and L.thallo_hip_arap_recompute_supported(d10.N, d10.ls.ell_stride) == 0
    torch.cuda.synchronize()
    for t in (buf, part, s3): assert (t.cpu().numpy().view(np.uint32) == sk.CANARY).all()      # a refused call launches nothing
    d.inputs_unchanged()


# ------------------------------------------------------------------ the grid-stride visit
def test_arap_second_visit_of_a_lane(torch, L):
    """N = 1024 * 256 + 300 (a directed ring, one out-slot): the grid is capped at 1024 workgroups, 300 lanes visit a second vertex.  cost, PCGInit1 and one applyJTJ."""
    d = _dev(torch, L, "stride", "ell").ready()
    N = d.N
    assert gr.vgrid(N) == sk.MAX_PARTIALS and gr.visits(0, N) == 2
    _note("arap_precompute F", np.abs(d.Fh - d.ref.F), sk.tol(K_F, d.ref.F_abs)); _note("arap_precompute G", np.abs(d.Gh - d.ref.G), sk.tol(K_G, d.ref.G_abs))
    t, m = d.ref.cost_terms()
    got = _cost(d, 0, N)
    _note("arap_cost partials", np.abs(got.astype(np.float64) - block_sums(t, 0, N)), sk.tol(2 * K_F + 1 + 3 * 2 + 2 + 6 + 4, block_sums(m, 0, N)))
    s = d.ref.system(F=d.Fh, G=d.Gh)
    o = _init(d, 0, N, True)
    k_r, k_d = 6 + 2, 7 + 2
    rr, _ = owned(o.r, N, 0, N); zz, _ = owned(o.z, N, 0, N); dd, _ = owned(o.diag, N, 0, N)
    _note("arap_pcg_init r", np.abs(rr[:6 * N] - s.r), sk.tol(k_r, s.r_abs)); _note("arap_pcg_init diag", np.abs(dd[:6 * N] - s.diag), sk.tol(k_d, s.diag))
    _note("arap_pcg_init z", np.abs(zz[:6 * N] - s.z), sk.tol(k_d + 4 + k_r + 1, s.pre * s.r_abs))
    check_partials("arap_pcg_init alphaN partials", partial_slots(o.aN, o.ret, 0, N), rr[:6 * N].astype(np.float64) * zz[:6 * N], 6, N, 0, N)
    ph, rh, preh, p, r, pre = _vectors(d)
    want, want_abs = d.ref.apply(ph, G=d.Gh)
    _check_apply("arap_apply_jtj_sums", d, _apply(d, "sums", 0, N, p, r, pre), 0, N, ph, want, want_abs, 13 + 2, rh, preh)
    d.inputs_unchanged()


# ------------------------------------------------------------------ graph Laplacian
def _lap_case(name):
    g = gr.graph_chain() if name == "chain" else gr.GRAPHS[name]()
    rng = np.random.default_rng([21, g[0]])
    X, A = rng.standard_normal(g[0]).astype(F32), rng.standard_normal(g[0]).astype(F32)
    return g, X, A, gr.LapRef(g, X, A), gr.build_lists(*g)


@pytest.mark.parametrize("name", ["chain", "sparse", "one", "hub"])
def test_lapgraph_kernels(torch, L, name):
    """cost: a share is 0.5 (f^2 + sum d^2), f = w (x - a) (2), d = x - x_m (1): squares 5 and 3, deg + 1 additions.  init: r = -(w (w (x - a)) + sum (x - x_m) - sum
    (x_m - x)): 3 + 1 per edge term + deg + ideg additions + the last sum; z = r bitwise; diag = w^2 + deg + ideg exactly (small integers and 1/4); zeros in p_prev and
    delta.  apply: the same sums on p."""
    g, X, A, ref, ls = _lap_case(name)
    N = g[0]
    ints = lambda a: sk.dbuf(torch, np.concatenate([a, np.zeros(4, np.int32)]))
    op, ov, ip, isrc = (ints(a) for a in (ls.out_ptr, ls.out_v1, ls.in_ptr, ls.in_src))
    Xd, Ad = sk.dbuf(torch, X), sk.dbuf(torch, A)
    md, mi = int(ls.odeg.max()), int(ls.ideg.max())
    out = sk.canary_buf(torch, PSLOTS)
    ret = L.thallo_hip_lapgraph_cost(N, op.data_ptr(), ov.data_ptr(), Xd.data_ptr(), Ad.data_ptr(), gr.LAP_W_FIT, out.data_ptr(), None)
    torch.cuda.synchronize()
    t, m = ref.cost_terms()
    got = partial_slots(out, ret, 0, N)
    _note("lapgraph_cost partials", np.abs(got.astype(np.float64) - block_sums(t, 0, N)), sk.tol(5 + md + 1 + gr.visits(0, N) + 10, block_sums(m, 0, N)))
    o = SimpleNamespace(**{k: sk.canary_buf(torch, N + TAIL) for k in ("r", "z", "p_prev", "delta", "diag")}, aN=sk.canary_buf(torch, PSLOTS))
    ret = L.thallo_hip_lapgraph_pcg_init(N, op.data_ptr(), ov.data_ptr(), ip.data_ptr(), isrc.data_ptr(), Xd.data_ptr(), Ad.data_ptr(), gr.LAP_W_FIT, o.r.data_ptr(), o.z.data_ptr(),
                                         o.p_prev.data_ptr(), o.delta.data_ptr(), o.diag.data_ptr(), o.aN.data_ptr(), None)
    torch.cuda.synchronize()
    h = {k: getattr(o, k).cpu().numpy() for k in ("r", "z", "p_prev", "delta", "diag")}
    for v in h.values(): assert (v[N:].view(np.uint32) == sk.CANARY).all()
    s = ref.system()
    _note("lapgraph_pcg_init r", np.abs(h["r"][:N] - s.r), sk.tol(5 + md + mi, s.r_abs))
    assert sk.same_bytes(h["z"][:N], h["r"][:N]) and np.array_equal(h["diag"][:N].astype(np.float64), s.diag)
    assert not h["p_prev"][:N].view(np.uint32).any() and not h["delta"][:N].view(np.uint32).any()
    check_partials("lapgraph_pcg_init alphaN partials", partial_slots(o.aN, ret, 0, N), h["r"][:N].astype(np.float64) ** 2, 1, N, 0, N)
    ph = np.random.default_rng([22, N]).standard_normal(N).astype(F32); p = sk.dbuf(torch, ph)
    Ap, aD = sk.canary_buf(torch, N + TAIL), sk.canary_buf(torch, PSLOTS)
    ret = L.thallo_hip_lapgraph_apply_jtj(N, op.data_ptr(), ov.data_ptr(), ip.data_ptr(), isrc.data_ptr(), gr.LAP_W_FIT, p.data_ptr(), Ap.data_ptr(), aD.data_ptr(), None)
    torch.cuda.synchronize()
    Ah = Ap.cpu().numpy()
    assert (Ah[N:].view(np.uint32) == sk.CANARY).all()
    want, want_abs = ref.apply(ph)
    _note("lapgraph_apply_jtj Ap", np.abs(Ah[:N] - want), sk.tol(4 + md + mi, want_abs))
    check_partials("lapgraph_apply_jtj alphaD partials", partial_slots(aD, ret, 0, N), ph.astype(np.float64) * Ah[:N], 1, N, 0, N)
    for tns, hst in ((Xd, X), (Ad, A), (p, ph)): assert sk.same_bytes(tns.cpu().numpy(), hst)


# ------------------------------------------------------------------ permute3, checksum
@pytest.mark.parametrize("N", [1, 257, 300])
def test_permute3(torch, L, N):
    rng = np.random.default_rng([31, N])
    idx = rng.permutation(N).astype(np.int32)
    src = rng.standard_normal((N, 3)).astype(F32)
    di, ds = sk.dbuf(torch, idx), sk.dbuf(torch, src)
    gat, sca, back = (sk.canary_buf(torch, 3 * N + TAIL) for _ in range(3))
    assert L.thallo_hip_permute3(N, di.data_ptr(), ds.data_ptr(), gat.data_ptr(), 0, None) == 0
    assert L.thallo_hip_permute3(N, di.data_ptr(), ds.data_ptr(), sca.data_ptr(), 1, None) == 0
    assert L.thallo_hip_permute3(N, di.data_ptr(), sca.data_ptr(), back.data_ptr(), 0, None) == 0
    assert L.thallo_hip_permute3(N, di.data_ptr(), ds.data_ptr(), ds.data_ptr(), 0, None) == sk.INVALID
    torch.cuda.synchronize()
    g, s, b = (t.cpu().numpy() for t in (gat, sca, back))
    for a in (g, s, b): assert (a[3 * N:].view(np.uint32) == sk.CANARY).all()
    want_s = np.empty_like(src); want_s[idx] = src
    assert sk.same_bytes(g[:3 * N], src[idx]) and sk.same_bytes(s[:3 * N], want_s) and sk.same_bytes(b[:3 * N], src)
    assert sk.same_bytes(ds.cpu().numpy(), src) and sk.same_bytes(di.cpu().numpy(), idx)


@pytest.mark.parametrize("n", [1, 300, 512 * 256 + 5])
def test_checksum_i32(torch, L, n):
    """the formula in Python integers mod 2^64; the kernel ADDS into the word it finds; swapping two unequal entries changes it; 512 * 256 + 5: the grid-stride visit"""
    rng = np.random.default_rng([41, n])
    v = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    start = 0x0123456789ABCDEF
    word = sk.dbuf(torch, np.array([start, sk.CANARY], np.uint64).view(np.int64))
    dv = sk.dbuf(torch, v)
    assert L.thallo_hip_checksum_i32(n, dv.data_ptr(), word.data_ptr(), None) == 0
    torch.cuda.synchronize()
    w = word.cpu().numpy().view(np.uint64)
    assert int(w[0]) == gr.checksum_i32(v, start) and int(w[1]) == sk.CANARY
    if n > 1:
        i, j = 0, int(np.flatnonzero(v != v[0])[-1])
        v2 = v.copy(); v2[[i, j]] = v2[[j, i]]
        word2 = sk.dbuf(torch, np.zeros(1, np.int64))
        assert L.thallo_hip_checksum_i32(n, sk.dbuf(torch, v2).data_ptr(), word2.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert int(word2.cpu().numpy().view(np.uint64)[0]) == gr.checksum_i32(v2) != gr.checksum_i32(v)
    assert L.thallo_hip_checksum_i32(0, dv.data_ptr(), word.data_ptr(), None) == sk.INVALID


# ------------------------------------------------------------------ through the C ABI
def test_hub_solve_with_and_without_the_resident_loop(torch, orc, monkeypatch):
    """The directed `hub` problem (3 out-slots, 10 in-slots: the plugin keeps the ELL layout and the recomputing applyJTJ) through Thallo_* with one launch per PCG
    iteration and with the resident loop: both follow the oracle's trajectory (COST_RTOL / VEC_RTOL of test_gpu_parity.py) and, out-degree <= 8, each other bit for bit."""
    import thallo_amd
    from thallo_amd import api
    from helpers import to_device, to_host, rel_err, copy_params
    COST_RTOL, VEC_RTOL = 1e-5, 2e-4
    g = gr.graph_hub()
    N, E = g[0], len(g[1])
    params = gr.arap_params(g, gr.arap_inputs(N, sentinels=False))
    runs = []
    for resident in ("0", "1"):
        monkeypatch.setenv("THALLO_RESIDENT", resident)
        dev = to_device(copy_params(params))
        s = api.ThalloSolver((N, E), thallo_amd.energy_file("arap_mesh_deformation"), timing_level=2)
        s.set_solver_parameters(nIterations=3, lIterations=10)
        pp = s.make_params(dev); s.init(pp)
        costs, traces = [s.current_cost()], []
        while s.step(pp):
            costs.append(s.current_cost()); traces.append(s.alpha_beta_trace())
        names = s.kernel_stats(); s.close()
        runs.append((costs, traces, to_host(dev[2]).copy(), to_host(dev[3]).copy(), names))
    (c0, t0, P0, A0, k0), (c1, t1, P1, A1, k1) = runs
    assert "PCGLoopResident" not in k0 and k1.get("PCGLoopResident", {}).get("launches") == 3, (k0, k1)
    po = copy_params(params)
    co, _ = orc.Problem(orc.ARAP_MESH, (N, E), po).solve(nIterations=3, lIterations=10)
    for c, P, A in ((c0, P0, A0), (c1, P1, A1)):
        print("hub solve: cost", rel_err(np.array(c), co), "Position", rel_err(P, po[2]), "Angle", np.abs(A - po[3]).max() / max(1.0, np.abs(po[3]).max()))
    for c, P, A in ((c0, P0, A0), (c1, P1, A1)):
        assert rel_err(np.array(c), co) < COST_RTOL, (c, co)
        assert rel_err(P, po[2]) < VEC_RTOL
        assert np.abs(A - po[3]).max() < VEC_RTOL * max(1.0, np.abs(po[3]).max())
    assert t0 == t1 and c0 == c1 and sk.same_bytes(P0, P1) and sk.same_bytes(A0, A1)
