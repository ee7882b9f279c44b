"""The shape_from_shading kernels (csrc/energy_sfs.hip, energy_sfs_pair.hip), entry point by entry point and form by form, against the float64 reference of
tests/sfs_reference.py -- every pixel of every case, per pixel.

Forms: "tile" (thallo_hip_sfs_march_debug_set(2, 0): k_precompute, k_cost, k_fused, k_diag on the float4 / float2 / byte planes), "march" ((2, 1), (6, 0): the one-pixel
marching kernels on the same planes), "pair" ((2, 1), (6, 1), even W: the pixel-pair kernels on the packed planes).  The two-pass form k_rows + k_gather is read from the
environment once per process: the fixture two_pass runs it in ONE fresh child.  Every debug setting is restored behind every test.

Outputs go into canary-filled buffers (sk.CANARY): rows outside [row0, row1), the tail behind every buffer and the partial slots behind the returned count keep it.

Bounds are k 2^-24 S, S from the reference (sfs_reference.py, "Bounds"), k counted from the operation chain as if nothing were contracted into an fma:
  G, BI     the count the reference's tracked tree carries (forward mode for the float4 planes: 97 / 51; closed form for the packed planes: 96 / 51), with the device's
            1 / sqrtf taken as RSQ roundings, + 2 for the second-order terms
  RSQ       = 2 x RSQ_MEASURED: the worst error of the device's inv * n_z (1 / sqrtf and the product behind it) against float64, in units of 2^-24 of the value, on
            inputs where everything before the root is exact (test_device_rsqrt_figure; the factor 2 because that set is finite)
  The linear chains below are built from the DEVICE's own planes (which test_precompute and test_slabs hold to the reference per pixel), so only the roundings of the kernel
  under test count: there both the value and S = |J|^T |J| |p| come from those planes.  test_init_and_apply_against_the_all_reference_system holds r, diag and Ap to the
  system built from the reference alone, with k enlarged by G's count.
  K_W   = 2      a row weight: sqrtf of the parameter, times the mask byte
  K_U   = 10     U = w (w (dB(q) - dB(q+ex))): dB three products and two sums (3), the difference (4), twice the weight (+ 2 + 1 each)
  K_R   = 9      R_c = w_s (4 (coef v) - four coef v): coef a difference and a quotient (2), the product (3), four subtractions (7), w_s (sqrtf, product)
  K_AP  = 25     out = fit + three G T + three w_s (coef lap): T = four U (13), G T (14); lap = 4 R - four R (13), coef lap (16), w_s (18); seven terms added (25)
  K_LM  = 27     ... + CtC v: a product and a sum
  K_INIT = 25    the same chain with dB := BI (shorter) and the fit term w_p (w_p (X - D)) (5); the sign is exact
  K_DIAG = 25    seven shading rows: (g - g) w (4), squared (9), fourteen squares and w_p^2 added (24); the reg rows 16 or 1 times sum (w_s coef)^2 (12); their sum
  K_COST = 25    a pixel's share 0.5 sum f^2: the reg row w_s (4 coef X - ...) (9) squared (19), six squares added
  a sum over pixels (partials added up in float64 by the test): the terms' k + one addition per row a lane visits + 16 (butterfly, waves, the pair of a lane)
The worst error / bound ratio per output and form goes to the file THALLO_SFS_RATIOS names, when set (that is how profiles/sfs_kernels/ratios.json was filled)."""
import functools
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest

import sfs_reference as sr
import shim_kernels as sk
from shim_kernels import F32

pytestmark = pytest.mark.gpu

RSQ_MEASURED = 1.3060          # worst |inv * n_z - float64| / (2^-24 |value|) on the MI355X over test_device_rsqrt_figure's inputs: 1.30592 (profiles/sfs_kernels/README.md)
RSQ = 2.0 * RSQ_MEASURED
K_AP, K_LM, K_INIT, K_DIAG, K_COST = 25, 27, 25, 25, 25
TAIL = 64
PSLOTS = sk.MAX_PARTIALS + 8
EPS64 = 2.0 ** -53
FORMS = ("tile", "march", "pair")
SHAPES = sr.SHAPES
FIN_AN = 0.01

RATIOS = {}


def _note(kernel, err, bound, where=""):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    bad = ~(err <= bound)
    with np.errstate(all="ignore"):
        ratio = float(np.nanmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))) if err.size else 0.0
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    assert not bad.any(), (kernel, where, np.argwhere(bad)[:8].tolist(), ratio, "errors", np.atleast_1d(err)[np.atleast_1d(bad)][:4].tolist(), "bounds", np.atleast_1d(bound)[np.atleast_1d(bad)][:4].tolist())


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
    t0 = time.time()
    yield
    path = os.environ.get("THALLO_SFS_RATIOS")
    if path:
        RATIOS["module run time in seconds"] = round(time.time() - t0, 1)
        json.dump(RATIOS, open(path, "w"), indent=1, sort_keys=True)


def restore(L):
    for what, v in ((0, 0), (1, 0), (2, -1), (3, 1), (4, 1), (5, 0), (6, -1), (7, 0)):
        L.thallo_hip_sfs_march_debug_set(what, v)


@pytest.fixture(autouse=True)
def _restore_and_stop_at_a_device_fault(torch, L):
    """every debug setting back to its default behind every test; a launch that faulted poisons every later one of the process: end the run there"""
    try:
        yield
    finally:
        restore(L)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error: {e}", returncode=3)


def set_form(L, form):
    L.thallo_hip_sfs_march_debug_set(2, 0 if form == "tile" else 1)
    L.thallo_hip_sfs_march_debug_set(6, 1 if form == "pair" else 0)


def forms_for(W):
    return FORMS if W % 2 == 0 else FORMS[:2]


# ------------------------------------------------------------------ one problem on the device
def whole(cs):
    return SimpleNamespace(params=cs.params, W=cs.W, H=cs.H, row0=0, row1=cs.H, yoff=0, Hg=cs.H, rows=slice(0, cs.H), lo=0, hi=cs.H, planes=slice(0, cs.H))


class Dev:
    """the inputs of a case (or of a slab cut of it) on the device, and the planes of one form"""

    def __init__(self, torch, L, cs, geo=None):
        self.torch, self.L, self.cs = torch, L, cs
        self.g = g = geo or whole(cs)
        self.W, self.H, self.N = g.W, g.H, g.W * g.H
        self.hp = np.array([F32(v) for v in g.params[:16]], F32)
        self.X, self.D, self.Im, self.mR, self.mC = (sk.dbuf(torch, a) for a in g.params[16:21])
        self.inputs = [(t, t.cpu().numpy().copy()) for t in (self.X, self.D, self.Im, self.mR, self.mC)]
        self.U, self.R = sk.canary_buf(torch, 2 * self.N + TAIL), sk.canary_buf(torch, 3 * self.N + TAIL)       # scratch of the two-pass form
        self._planes = {}

    def geo(self, row0=None, row1=None):
        g = self.g
        return (g.W, g.H, g.row0 if row0 is None else row0, g.row1 if row1 is None else row1, g.yoff, g.Hg, self.hp.ctypes.data)

    def precompute(self, form, ra=0, rb=None, plain=False, cost_rows=None):
        """fresh canary planes filled by thallo_hip_sfs_precompute (cost_rows: by thallo_hip_sfs_precompute_cost); returns the planes, the cost partials and the return value"""
        t, L, N = self.torch, self.L, self.N
        set_form(L, form)
        L.thallo_hip_sfs_march_debug_set(4, 0 if plain else 1)
        G, Wt, fl = sk.canary_buf(t, 4 * N + TAIL), sk.canary_buf(t, 2 * N + TAIL), sk.canary_buf(t, (N + 3) // 4 + TAIL)
        a = self.geo(ra, self.H if rb is None else rb) + tuple(x.data_ptr() for x in (self.X, self.D, self.Im, self.mR, self.mC, G, Wt, fl))
        cost = None
        if cost_rows is None:
            rc = L.thallo_hip_sfs_precompute(*a, None)
        else:
            cost = sk.canary_buf(t, PSLOTS)
            rc = L.thallo_hip_sfs_precompute_cost(*a, cost_rows[0], cost_rows[1], cost.data_ptr(), None)
        t.cuda.synchronize()
        return SimpleNamespace(G=G, Wt=Wt, fl=fl, cost=cost, rc=rc, packed=form == "pair", kernel=self.pre_kernel(form, plain))

    def pre_kernel(self, form, plain=False):
        """the kernel that fills the planes (energy_sfs.hip sfs_precompute): the pair kernel on packed planes; k_precompute in the tile form, when asked for (what = 4)
        and below four pixels; the one-pixel marching kernel otherwise"""
        return "pair" if form == "pair" else "k_precompute" if form == "tile" or plain or self.N < 4 else "marching"

    def planes(self, form):
        """the planes of the whole local image as the precompute kernel of `form` leaves them, once per KERNEL; host copies: G4 [H, W, 4], and Wt / fl or the packed dword"""
        key = self.pre_kernel(form)
        if key not in self._planes:
            p = self.precompute(form)
            assert p.rc == 0, p.rc
            self._planes[key] = self.host(p)
        return self._planes[key]

    def host(self, p):
        N, H, W = self.N, self.H, self.W
        G, Wt, fl = p.G.cpu().numpy(), p.Wt.cpu().numpy(), p.fl.cpu().numpy()
        p.tails_ok = bool((G[4 * N:].view(np.uint32) == sk.CANARY).all() and (Wt[2 * N:].view(np.uint32) == sk.CANARY).all())
        if p.packed:
            p.G4 = np.ascontiguousarray(G[:4 * N].reshape(4, H, W).transpose(1, 2, 0))
            p.dword = Wt[:N].view(np.uint32).reshape(H, W)
            p.tails_ok = p.tails_ok and bool((Wt[N:2 * N].view(np.uint32) == sk.CANARY).all() and (fl.view(np.uint32) == sk.CANARY).all())      # second half of Wt and fl: not used
        else:
            p.G4 = G[:4 * N].reshape(H, W, 4)
            p.Wt2 = Wt[:2 * N].reshape(H, W, 2)
            p.flb = fl.view(np.uint8)[:N].reshape(H, W)
            flat = fl.view(np.uint8)
            pat = np.frombuffer(np.uint32(sk.CANARY).tobytes(), np.uint8)
            p.tails_ok = p.tails_ok and bool((flat[N:] == pat[np.arange(N, flat.size) % 4]).all())
        return p

    def system(self, form):
        """the float64 system of the LOCAL image built from the device's planes (global coordinates: the case's own decisions and coefficients, cut)"""
        key = ("sys", self.pre_kernel(form))
        if key not in self._planes:
            g, cs = self.g, self.cs
            G4 = np.zeros((cs.H, cs.W, 4))
            G4[g.lo:g.hi] = self.planes(form).G4
            self._planes[key] = cs.system(G=G4)
        return self._planes[key]

    def inputs_unchanged(self):
        self.torch.cuda.synchronize()
        for t, h in self.inputs:
            assert sk.same_bytes(t.cpu().numpy(), h), "a const input changed"


@functools.lru_cache(maxsize=64)
def _dev(torch, L, family, W, H, only=None, cut=None):
    cs = sr.case(family, W, H, 0, only)
    return Dev(torch, L, cs, sr.slab(cs, *cut) if cut else None)


def rows_of(host, d, row0=None, row1=None):
    """a flat per-pixel output [N + TAIL]: the owned rows as [rows, W]; everything else must still hold the canary"""
    g = d.g
    r0, r1 = (g.row0 if row0 is None else row0), (g.row1 if row1 is None else row1)
    body = host[:d.N].reshape(d.H, d.W)
    out = np.ones(host.size, bool); out[r0 * d.W:r1 * d.W] = False
    assert (host.view(np.uint32)[out] == sk.CANARY).all(), "written outside the rows [row0, row1)"
    return body[r0:r1]


def glob(d, flat, row0=None, row1=None):
    """the rows of a GLOBAL per-pixel reference vector that the local rows [row0, row1) are"""
    g = d.g
    r0, r1 = (g.row0 if row0 is None else row0), (g.row1 if row1 is None else row1)
    return np.asarray(flat).reshape(d.cs.H, d.cs.W)[g.lo + r0:g.lo + r1]


def partials(buf, ret, width=1):
    h = buf.cpu().numpy()
    h = h.reshape(-1, width) if width > 1 else h
    assert ret > 0 and sk.written_slots(h) == ret, (ret, sk.written_slots(h))
    return h[:ret]


def check_sum(kernel, parts, terms, k_terms, rows, eps=sk.EPS, where=""):
    """the partials added up in float64 against the float64 sum of the terms"""
    terms = np.asarray(terms, np.float64)
    _note(kernel, abs(float(np.asarray(parts, np.float64).sum()) - float(terms.sum())), (k_terms + rows + 16) * eps * float(np.abs(terms).sum()), where)


def vectors(d, seed=11):
    rng = np.random.default_rng([seed, d.N])
    h = SimpleNamespace(p=rng.standard_normal(d.N).astype(F32), r=rng.standard_normal(d.N).astype(F32), ctc=rng.uniform(0.0, 50.0, d.N).astype(F32))
    return h, SimpleNamespace(**{k: sk.dbuf(d.torch, np.concatenate([v, np.zeros(TAIL, F32)])) for k, v in vars(h).items()})


def local_of(d, flat_local):
    """a LOCAL per-pixel vector placed into a global one (zeros elsewhere): the reference works on the global image"""
    out = np.zeros((d.cs.H, d.cs.W)); out[d.g.lo:d.g.hi] = np.asarray(flat_local, np.float64).reshape(d.H, d.W)
    return out.ravel()


# ------------------------------------------------------------------ the one figure the code cannot give
def test_device_rsqrt_figure(torch, L):
    """constant X = c with 11 fraction bits, f_x = 64, f_y = 128, lighting e_3, Im = 0: n_x = n_y = 0 and n_z = -c^2 / 8192 exactly, |n|^2 = fl(n_z^2) (one known rounding),
    BI = fl(inv * n_z) with inv the device's 1 / sqrtf(|n|^2) and every other term an exact zero.  Against float64 n_z / sqrt(fl(n_z^2)), in units of 2^-24 of the value;
    prints the worst figure (what RSQ_MEASURED records) and holds the device to twice the recorded one -- k_precompute (3 x 3) and the pair kernel (4 x 4)."""
    worst = 0.0
    rng = np.random.default_rng(77)
    for W, H, form in ((3, 3, "tile"), (4, 4, "pair")):
        for j in rng.integers(0, 2048, 24):
            c = F32((2048 + int(j)) / 2048.0)
            X = np.full((H, W), c, F32)
            params = [1.0, 1.0, 1.0, 64.0, 128.0, 1.3, 1.7] + [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0] + [X, np.ones((H, W), F32), np.zeros((H, W), F32),
                                                                                                              np.ones((H, W), np.uint8), np.ones((H, W), np.uint8)]
            d = Dev(torch, L, sr.Case(params))
            p = d.host(d.precompute(form, plain=True))
            assert p.rc == 0
            nz = F32(-(c * c) / F32(8192.0))
            assert float(nz) == -(float(c) ** 2) / 8192.0                      # exact
            sq32 = F32(nz * nz)
            want = float(nz) / np.sqrt(float(sq32))
            got = p.G4[1:, 1:, 3].astype(np.float64)
            worst = max(worst, float((np.abs(got - want) / (sk.EPS * abs(want))).max()))
    RATIOS["device 1 / sqrtf and the product behind it: worst relative error in units of 2^-24"] = worst
    print(f"1 / sqrtf x n_z: worst relative error {worst:.5f} x 2^-24")
    assert worst <= RSQ, worst


# ------------------------------------------------------------------ precompute
def check_planes(d, p, rows=None, tag=""):
    """the planes p of Dev d on the local rows `rows` (default: where they equal the global planes) against the reference; recorded under the kernel that wrote them"""
    cs, g = d.cs, d.g
    kernel = f"precompute [{p.kernel}]{tag}"
    rows = g.planes if rows is None else rows
    G, _ = (cs.bi_closed(RSQ) if p.packed else cs.bi_forward(RSQ))
    cut = lambda a: a[g.lo:g.hi][rows]
    assert p.tails_ok, kernel
    for j, name in enumerate(("dBI/dX(c)", "dBI/dX(c-ex)", "dBI/dX(c-ey)", "BI")):
        _note(f"{kernel} {name}", np.abs(p.G4[rows][..., j].astype(np.float64) - cut(G[j].v)), sk.tol(G[j].k + 2, cut(G[j].m)), cs.name)
    if p.packed:
        assert np.array_equal(p.dword[rows], cut(cs.dword)), (kernel, cs.name, np.argwhere(p.dword[rows] != cut(cs.dword))[:8].tolist())
    else:
        assert np.array_equal(p.flb[rows], cut(cs.fl)), (kernel, cs.name)
        assert sk.same_bytes(p.Wt2[rows], cut(cs.Wt)), (kernel, cs.name)


@pytest.mark.parametrize("family", sr.FAMILIES)
def test_precompute(torch, L, family):
    """thallo_hip_sfs_precompute on every shape: G and BI per pixel (forward-mode bound on the float4 planes by k_precompute and by the marching kernel, closed-form bound
    on the packed planes), fl, Wt and the packed dword exactly; k_precompute and the marching kernel agree on fl and Wt bit for bit; nothing behind the planes is written"""
    for W, H in SHAPES:
        d = _dev(torch, L, family, W, H)
        got = {}
        for form, plain in (("tile", True), ("march", False), ("march", True)) + ((("pair", False),) if W % 2 == 0 else ()):
            set_form(L, form)
            assert L.thallo_hip_sfs_planes_layout(W, H) == (1 if form == "pair" else 0)
            p = d.host(d.precompute(form, plain=plain))
            assert p.rc == 0, (form, W, H, p.rc)
            check_planes(d, p)
            got[(form, plain)] = p
        a, b = got[("tile", True)], got[("march", False)]
        assert a.kernel == "k_precompute" and b.kernel == ("marching" if W * H >= 4 else "k_precompute")
        assert sk.same_bytes(a.flb, b.flb) and sk.same_bytes(a.Wt2, b.Wt2)
        assert sk.same_bytes(got[("march", True)].G4, a.G4)                                  # the same kernel under either setting of what = 2
        d.inputs_unchanged()


@pytest.mark.parametrize("only", ["p", "s", "g"])
def test_precompute_one_weight_at_a_time(torch, L, only):
    for family in sr.FAMILIES:
        for W, H in ((3, 3), (61, 5), (130, 17)):
            d = _dev(torch, L, family, W, H, only)
            for form in forms_for(W):
                check_planes(d, d.host(d.precompute(form)))


def test_precompute_row_range_and_refusals(torch, L):
    """rows [ra, rb) only: the other rows of every plane keep the canary; ra >= rb, rb > H: -hipErrorInvalidValue and nothing written"""
    d = _dev(torch, L, "holes", 130, 17)
    N, W = d.N, d.W
    for form in FORMS:
        for plain in (True, False):
            p = d.host(d.precompute(form, ra=3, rb=9, plain=plain))
            assert p.rc == 0
            check_planes(d, p, rows=slice(3, 9))                   # (rows 3 and 8 read the INPUT rows 2 and 9, which are there: right too)
            G = p.G.cpu().numpy().view(np.uint32)
            if p.packed:
                for k in range(4):
                    pl = G[k * N:(k + 1) * N].reshape(d.H, W)
                    assert (pl[:3] == sk.CANARY).all() and (pl[9:] == sk.CANARY).all()
                dw = p.Wt.cpu().numpy().view(np.uint32)[:N].reshape(d.H, W)
                assert (dw[:3] == sk.CANARY).all() and (dw[9:] == sk.CANARY).all()
            else:
                pl = G[:4 * N].reshape(d.H, W * 4)
                assert (pl[:3] == sk.CANARY).all() and (pl[9:] == sk.CANARY).all()
        for ra, rb in ((5, 5), (9, 3), (0, d.H + 1), (-1, 4)):
            p = d.precompute(form, ra=ra, rb=rb)
            assert p.rc == sk.INVALID
            for t in (p.G, p.Wt, p.fl):
                assert (t.cpu().numpy().view(np.uint32) == sk.CANARY).all()
    d.inputs_unchanged()


# ------------------------------------------------------------------ cost
def cost_reference(d, form, row0=None, row1=None):
    s = d.system(form)
    t = glob(d, s.cost_terms, row0, row1)
    m = glob(d, 0.5 * (s.Fabs.reshape(-1, 6) ** 2).sum(-1), row0, row1)
    return t, m


@pytest.mark.parametrize("family", sr.FAMILIES)
def test_cost_and_precompute_cost(torch, L, family):
    """thallo_hip_sfs_cost (k_cost, float4 planes) and thallo_hip_sfs_precompute_cost (marching and pair kernels): the partials' sum against the float64 cost of the rows, the
    number of partials written is the return value, the planes of precompute_cost are those of precompute bit for bit; on packed planes thallo_hip_sfs_cost refuses"""
    for W, H in SHAPES:
        d = _dev(torch, L, family, W, H)
        for form in forms_for(W):
            planes = d.planes(form)
            t, m = cost_reference(d, form)
            set_form(L, form)
            out = sk.canary_buf(torch, PSLOTS)
            ret = L.thallo_hip_sfs_cost(*d.geo(), d.X.data_ptr(), d.D.data_ptr(), planes.G.data_ptr(), planes.Wt.data_ptr(), planes.fl.data_ptr(), out.data_ptr(), None)
            torch.cuda.synchronize()
            if form == "pair":
                assert ret == sk.NOT_SUPPORTED and (out.cpu().numpy().view(np.uint32) == sk.CANARY).all()
            else:
                got = partials(out, ret)
                _note(f"cost [{form}]", abs(got.astype(np.float64).sum() - t.sum()), sk.tol(K_COST + H + 16, m.sum()), d.cs.name)
            if form == "tile":
                continue
            p = d.precompute(form, cost_rows=(0, H))
            if W * H < 4 and form == "march":
                assert p.rc == sk.NOT_SUPPORTED                                           # the marching precompute does not take fewer than four pixels: the caller launches the two
                continue
            got = partials(p.cost, p.rc)
            _note(f"precompute_cost [{form}]", abs(got.astype(np.float64).sum() - t.sum()), sk.tol(K_COST + H + 16, m.sum()), d.cs.name)
            p, q = d.host(p), planes
            assert sk.same_bytes(p.G4, q.G4) and p.tails_ok, "the planes of precompute_cost differ from those of precompute"
            assert sk.same_bytes(p.dword, q.dword) if p.packed else (sk.same_bytes(p.flb, q.flb) and sk.same_bytes(p.Wt2, q.Wt2))
        d.inputs_unchanged()


# ------------------------------------------------------------------ PCGInit1
def run_init(d, form, with_diag=True, diag_by_march=True, row0=None, row1=None):
    t, L, N = d.torch, d.L, d.N
    set_form(L, form)
    L.thallo_hip_sfs_march_debug_set(3, 1 if diag_by_march else 0)
    pl = d.planes(form)
    set_form(L, form)
    o = SimpleNamespace(**{k: sk.canary_buf(t, N + TAIL) for k in ("r", "z", "p_prev", "delta", "diag")}, aN=sk.canary_buf(t, PSLOTS))
    o.ret = L.thallo_hip_sfs_pcg_init(*d.geo(row0, row1), d.X.data_ptr(), d.D.data_ptr(), pl.G.data_ptr(), pl.Wt.data_ptr(), pl.fl.data_ptr(), d.U.data_ptr(), d.R.data_ptr(),
                                      o.r.data_ptr(), o.z.data_ptr(), o.p_prev.data_ptr(), o.delta.data_ptr(), o.diag.data_ptr() if with_diag else None, o.aN.data_ptr(), None)
    t.cuda.synchronize()
    return o


def check_init(d, form, o, with_diag=True, tag="", row0=None, row1=None):
    s = d.system(form)
    name = f"pcg_init [{form}]"
    r = rows_of(o.r.cpu().numpy(), d, row0, row1)
    _note(name + " r", np.abs(r.astype(np.float64) - glob(d, s.r, row0, row1)), sk.tol(K_INIT, glob(d, s.r_abs, row0, row1)), d.cs.name + tag)
    assert sk.same_bytes(rows_of(o.z.cpu().numpy(), d, row0, row1), r), "z != r"
    assert not rows_of(o.p_prev.cpu().numpy(), d, row0, row1).view(np.uint32).any() and not rows_of(o.delta.cpu().numpy(), d, row0, row1).view(np.uint32).any()
    if with_diag:
        dg = rows_of(o.diag.cpu().numpy(), d, row0, row1)
        _note(name + " diag" + tag, np.abs(dg.astype(np.float64) - glob(d, s.diag, row0, row1)), sk.tol(K_DIAG, glob(d, s.diag_abs, row0, row1)), d.cs.name)
    else:
        assert (o.diag.cpu().numpy().view(np.uint32) == sk.CANARY).all()
    got = partials(o.aN, o.ret)
    check_sum(name + " alphaN", got, r.astype(np.float64) ** 2, 1, r.shape[0], where=d.cs.name)
    return r


@pytest.mark.parametrize("family", sr.FAMILIES)
def test_pcg_init(torch, L, family):
    """thallo_hip_sfs_pcg_init in every form: r = -J^T F and diag(J^T J) per pixel (the diagonal by k_diag and by the marching kernel), z == r, zeros in p_prev and delta,
    the alphaN partials; diag_out NULL changes nothing else"""
    for W, H in SHAPES:
        d = _dev(torch, L, family, W, H)
        for form in forms_for(W):
            o = run_init(d, form)
            check_init(d, form, o)
            if form != "tile":
                o0 = run_init(d, form, diag_by_march=False)
                check_init(d, form, o0, tag=" (k_diag)" if form == "march" else "")
                assert sk.same_bytes(o0.r.cpu().numpy(), o.r.cpu().numpy())
            o2 = run_init(d, form, with_diag=False)
            check_init(d, form, o2, with_diag=False)
            for key in ("r", "z", "p_prev", "delta"):
                assert sk.same_bytes(getattr(o2, key).cpu().numpy(), getattr(o, key).cpu().numpy()), key
        d.inputs_unchanged()


# ------------------------------------------------------------------ applyJTJ
def run_apply(d, form, variant, v, gate=None, fin_aN=None, row0=None, row1=None):
    """variant: plain, gated, lm, sums, fin"""
    t, L, N = d.torch, d.L, d.N
    pl = d.planes(form)
    set_form(L, form)
    o = SimpleNamespace(Ap=sk.canary_buf(t, N + TAIL), aD=sk.canary_buf(t, PSLOTS), s3=sk.canary_buf(t, 3 * PSLOTS, np.float64), words=sk.canary_buf(t, 2 + TAIL),
                        tickets=sk.dbuf(t, np.zeros(sk.FIN_TICKET_WORDS, np.uint32)))
    head = d.geo(row0, row1) + (pl.G.data_ptr(), pl.Wt.data_ptr(), pl.fl.data_ptr(), d.U.data_ptr(), d.R.data_ptr(), v.p.data_ptr())
    g = None if gate is None else sk.dbuf(t, np.array([gate, 0], np.uint32))
    gp = None if g is None else g.data_ptr()
    if variant == "plain": o.ret = L.thallo_hip_sfs_apply_jtj(*head, o.Ap.data_ptr(), o.aD.data_ptr(), None)
    elif variant == "gated": o.ret = L.thallo_hip_sfs_apply_jtj_gated(*head, o.Ap.data_ptr(), o.aD.data_ptr(), gp, None)
    elif variant == "lm": o.ret = L.thallo_hip_sfs_apply_jtj_lm(*head, v.ctc.data_ptr(), o.Ap.data_ptr(), o.aD.data_ptr(), gp, None)
    elif variant == "sums": o.ret = L.thallo_hip_sfs_apply_jtj_sums(*head, o.Ap.data_ptr(), o.aD.data_ptr(), v.r.data_ptr(), o.s3.data_ptr(), None)
    else:
        fin = sk.NO_FIN
        if fin_aN is not None:
            o.aNt = sk.dbuf(t, np.array([fin_aN], F32))
            fin = sk.FinT(sk.sumt(o.aNt), o.tickets.data_ptr(), o.words.data_ptr(), o.words.data_ptr() + 4)
        o.ret = L.thallo_hip_sfs_apply_jtj_sums_fin(*head, o.Ap.data_ptr(), o.aD.data_ptr(), v.r.data_ptr(), o.s3.data_ptr(), fin, None)
    t.cuda.synchronize()
    return o


def check_apply(name, d, form, o, h, lm=False, sums=False, fin_aN=None, row0=None, row1=None):
    s = d.system(form)
    want, mag = s.apply(local_of(d, h.p), local_of(d, h.ctc) if lm else None)
    Ap = rows_of(o.Ap.cpu().numpy(), d, row0, row1)
    _note(name + " Ap", np.abs(Ap.astype(np.float64) - glob(d, want, row0, row1)), sk.tol(K_LM if lm else K_AP, glob(d, mag, row0, row1)), d.cs.name)
    g = d.g
    r0, r1 = (g.row0 if row0 is None else row0), (g.row1 if row1 is None else row1)
    own = lambda a: np.asarray(a, np.float64).reshape(d.H, d.W)[r0:r1]
    aD = partials(o.aD, o.ret)
    check_sum(name + " alphaD", aD, own(h.p) * Ap, 1, r1 - r0, where=d.cs.name)
    if not sums:
        assert (o.s3.cpu().numpy().view(np.uint32) == sk.CANARY).all()
        return Ap, aD, None
    s3 = partials(o.s3, o.ret, 3)
    for j, terms in enumerate(sr.terms_NS1S2(own(h.r), Ap)):
        check_sum(name + " {N, S1, S2}", s3[:, j], terms, 2, r1 - r0, eps=EPS64, where=d.cs.name)
    w = o.words.cpu().numpy()
    if fin_aN is not None:
        assert (w[2:].view(np.uint32) == sk.CANARY).all() and not o.tickets.cpu().numpy().any()
        adw, alpha, bnw, magb = sk.ref_scalars_finish(aD, s3.ravel(), F32(fin_aN))
        assert sk.same_bytes(w[0:1], adw), (name, w[0], adw)
        if float(bnw) > 0: assert magb / float(bnw) < 2.0 ** 20
        assert sk.ulp_apart(w[1], bnw) <= 1, (w[1], bnw)
    else:
        assert (w.view(np.uint32) == sk.CANARY).all()
    return Ap, aD, s3


def all_apply_variants(d, form, h, v, row0=None, row1=None):
    tag = f"apply_jtj [{form}]"
    kw = dict(row0=row0, row1=row1)
    A1, aD1, _ = check_apply(tag, d, form, run_apply(d, form, "plain", v, **kw), h, **kw)
    o0 = run_apply(d, form, "gated", v, gate=0, **kw)
    assert sk.same_bytes(o0.Ap.cpu().numpy()[:d.N], run_apply(d, form, "plain", v, **kw).Ap.cpu().numpy()[:d.N])
    check_apply(tag + " gated", d, form, o0, h, **kw)
    og = run_apply(d, form, "gated", v, gate=1, **kw)
    assert (og.Ap.cpu().numpy().view(np.uint32) == sk.CANARY).all() and (og.aD.cpu().numpy().view(np.uint32) == sk.CANARY).all(), "a gated launch wrote"
    check_apply(tag + " lm", d, form, run_apply(d, form, "lm", v, **kw), h, lm=True, **kw)
    og = run_apply(d, form, "lm", v, gate=1, **kw)
    assert (og.Ap.cpu().numpy().view(np.uint32) == sk.CANARY).all() and (og.aD.cpu().numpy().view(np.uint32) == sk.CANARY).all(), "a gated launch wrote"
    A2, aD2, s2 = check_apply(tag + " sums", d, form, run_apply(d, form, "sums", v, **kw), h, sums=True, **kw)
    A3, aD3, s3 = check_apply(tag + " sums_fin", d, form, run_apply(d, form, "fin", v, **kw), h, sums=True, **kw)
    A4, aD4, s4 = check_apply(tag + " sums_fin", d, form, run_apply(d, form, "fin", v, fin_aN=FIN_AN, **kw), h, sums=True, fin_aN=FIN_AN, **kw)
    assert sk.same_bytes(A1, A2) and sk.same_bytes(A1, A3) and sk.same_bytes(A1, A4), "the variants differ on Ap"
    assert sk.same_bytes(aD1, aD2) and sk.same_bytes(aD1, aD3) and sk.same_bytes(aD1, aD4)
    assert sk.same_bytes(s2, s3) and sk.same_bytes(s2, s4), "_sums and _sums_fin differ on {N, S1, S2}"
    return A1


@pytest.mark.parametrize("family", sr.FAMILIES)
def test_apply_jtj(torch, L, family):
    """thallo_hip_sfs_apply_jtj, _gated (gate 0: the plain launch's bytes; gate 1: nothing written), _lm, _sums, _sums_fin without and with tickets, in every form: Ap per
    pixel against (J^T J + CtC) p, the alphaD partials, the double sums, the two scalar words (alphaD bit-exact, betaN to 1 ulp); the variants agree byte for byte"""
    for W, H in SHAPES:
        d = _dev(torch, L, family, W, H)
        h, v = vectors(d)
        for form in forms_for(W):
            all_apply_variants(d, form, h, v)
        d.inputs_unchanged()
        for key in ("p", "r", "ctc"):
            assert sk.same_bytes(getattr(v, key).cpu().numpy()[:d.N], getattr(h, key))


@pytest.mark.parametrize("only", ["p", "s", "g"])
def test_init_and_apply_one_weight_at_a_time(torch, L, only):
    for family in sr.FAMILIES:
        for W, H in ((3, 3), (61, 5), (130, 17)):
            d = _dev(torch, L, family, W, H, only)
            h, v = vectors(d)
            for form in forms_for(W):
                check_init(d, form, run_init(d, form))
                check_apply(f"apply_jtj [{form}]", d, form, run_apply(d, form, "sums", v), h, sums=True)
                if form != "pair":
                    set_form(L, form)
                    pl = d.planes(form)
                    out = sk.canary_buf(torch, PSLOTS)
                    ret = L.thallo_hip_sfs_cost(*d.geo(), d.X.data_ptr(), d.D.data_ptr(), pl.G.data_ptr(), pl.Wt.data_ptr(), pl.fl.data_ptr(), out.data_ptr(), None)
                    torch.cuda.synchronize()
                    t, m = cost_reference(d, form)
                    _note(f"cost [{form}]", abs(partials(out, ret).astype(np.float64).sum() - t.sum()), sk.tol(K_COST + H + 16, m.sum()), d.cs.name)


def test_init_and_apply_against_the_all_reference_system(torch, L):
    """the tests above build J from the DEVICE's planes, so that only the kernel under test is charged.  Here value AND scale come from the reference alone (its own G,
    the magnitudes of its tree): r, diag and Ap of every form on `holes` 130 x 17 and `masks` 62 x 3, with k enlarged by G's count for each of the two times G enters
    (J and J^T; for r: G and BI): + 2 (k_G + 2)"""
    for family, (W, H) in (("holes", (130, 17)), ("masks", (62, 3))):
        d = _dev(torch, L, family, W, H)
        cs = d.cs
        h, v = vectors(d)
        for form in forms_for(W):
            G, _ = cs.bi_closed(RSQ) if form == "pair" else cs.bi_forward(RSQ)
            kG = 2 * (max(t.k for t in G) + 2)
            s = cs.system(G=np.stack([t.v for t in G], -1), Gmag=np.stack([t.m for t in G], -1))
            o = run_init(d, form)
            r, dg = rows_of(o.r.cpu().numpy(), d).ravel(), rows_of(o.diag.cpu().numpy(), d).ravel()
            _note(f"all-reference pcg_init [{form}] r", np.abs(r - s.r), sk.tol(K_INIT + kG, s.r_abs), cs.name)
            _note(f"all-reference pcg_init [{form}] diag", np.abs(dg - s.diag), sk.tol(K_DIAG + kG, s.diag_abs), cs.name)
            want, mag = s.apply(h.p)
            Ap = rows_of(run_apply(d, form, "plain", v).Ap.cpu().numpy(), d).ravel()
            _note(f"all-reference apply_jtj [{form}] Ap", np.abs(Ap - want), sk.tol(K_AP + kG, mag), cs.name)


# ------------------------------------------------------------------ rows per segment, prefetch depth
@pytest.mark.parametrize("rows", [4, 8, 16])
def test_rows_per_wave_segment(torch, L, rows):
    """thallo_hip_sfs_march_debug_set(0, rows) with H = 15, 16, 17 (and 33): below, equal to and one above a multiple of every value; pair prefetch depth 3 and 6"""
    for family, (W, H) in (("holes", (64, 15)), ("steps", (60, 16)), ("masks", (130, 17)), ("holes", (250, 33))):
        d = _dev(torch, L, family, W, H)
        h, v = vectors(d)
        for form in forms_for(W)[1:]:
            for depth in ((0,) if form == "march" else (3, 6)):
                d.planes(form)
                L.thallo_hip_sfs_march_debug_set(0, rows); L.thallo_hip_sfs_march_debug_set(7, depth)
                check_init(d, form, run_init(d, form))
                L.thallo_hip_sfs_march_debug_set(0, rows); L.thallo_hip_sfs_march_debug_set(7, depth)
                check_apply(f"apply_jtj [{form}]", d, form, run_apply(d, form, "fin", v, fin_aN=FIN_AN), h, sums=True, fin_aN=FIN_AN)
                check_apply(f"apply_jtj [{form}] lm", d, form, run_apply(d, form, "lm", v), h, lm=True)
                p = d.host(d.precompute(form, cost_rows=(0, H)))
                check_planes(d, p)
                restore(L)


# ------------------------------------------------------------------ slabs
SLABS = [(130, 33, (0, 11)), (130, 33, (11, 18)), (130, 33, (13, 14)), (130, 33, (19, 33)), (250, 33, (0, 2)), (250, 33, (7, 20)), (250, 33, (31, 33))]


@pytest.mark.parametrize("family", ["holes", "steps", "masks"])
def test_slabs(torch, L, family):
    """a rank's cut of the 130 x 33 and 250 x 33 images (top, middle, bottom; owned ranges of 1, 2, 7, 11, 13 and 14 rows; yoff 0, 5, 9, 11, 17, 29; Hg = 33 > H): the
    planes where they equal the global ones, the cost of the owned rows, PCGInit1 and every applyJTJ variant on the owned rows against the GLOBAL reference -- pixel
    coordinates and the border guard are global, the bounds of the loads local"""
    for W, H, cut in SLABS:
        d = _dev(torch, L, family, W, H, None, cut)
        g = d.g
        assert g.Hg == H > 0 and g.H < H and g.yoff == max(0, cut[0] - 2)
        h, v = vectors(d)
        for form in FORMS:
            p = d.planes(form)                                  # (tile: k_precompute, march: the one-pixel marching kernel, pair: the pair kernel -- each its own planes)
            assert p.kernel == {"tile": "k_precompute", "march": "marching", "pair": "pair"}[form]
            check_planes(d, p, tag=" slab")
            t, m = cost_reference(d, form)
            if form != "tile":
                pc = d.precompute(form, cost_rows=(g.row0, g.row1))
                _note(f"precompute_cost [{form}]", abs(partials(pc.cost, pc.rc).astype(np.float64).sum() - t.sum()), sk.tol(K_COST + g.H + 16, m.sum()), d.cs.name)
                pc = d.host(pc)
                check_planes(d, pc, tag=" slab")                # the planes precompute_cost leaves on the slab: against the global reference, and the plain launch's bytes
                assert sk.same_bytes(pc.G4, p.G4) and (sk.same_bytes(pc.dword, p.dword) if pc.packed else (sk.same_bytes(pc.flb, p.flb) and sk.same_bytes(pc.Wt2, p.Wt2)))
            if form != "pair":
                set_form(L, form)
                out = sk.canary_buf(torch, PSLOTS)
                ret = L.thallo_hip_sfs_cost(*d.geo(), d.X.data_ptr(), d.D.data_ptr(), p.G.data_ptr(), p.Wt.data_ptr(), p.fl.data_ptr(), out.data_ptr(), None)
                torch.cuda.synchronize()
                _note(f"cost [{form}]", abs(partials(out, ret).astype(np.float64).sum() - t.sum()), sk.tol(K_COST + g.H + 16, m.sum()), d.cs.name)
            check_init(d, form, run_init(d, form))
            if form == "march":
                check_init(d, form, run_init(d, form, diag_by_march=False), tag=" (k_diag)")
            all_apply_variants(d, form, h, v)
        d.inputs_unchanged()


# ------------------------------------------------------------------ the one-launch iterations against the launches they replace
def _dvecs(d, h):
    t, N = d.torch, d.N
    rng = np.random.default_rng([13, N])
    mk = lambda a=None: sk.DVec(t, N, a)
    return SimpleNamespace(r=mk(h.r), Ap_prev=mk(rng.standard_normal(N).astype(F32)), p_prev=mk(h.p), delta=mk(rng.standard_normal(N).astype(F32) * F32(0.1)))


@pytest.mark.parametrize("first", [1, 0])
def test_pcg_iter_equals_update_plus_apply(torch, L, first):
    """thallo_hip_sfs_pcg_iter (marching and pair forms; delta given and NULL) against float64 and, as the header states it, against thallo_hip_pcg_update +
    thallo_hip_sfs_apply_jtj_sums_fin bit for bit: r_out, p_out, delta, Ap_out, the partials, the two words"""
    for family, (W, H) in (("holes", (130, 17)), ("masks", (62, 3)), ("steps", (61, 5)), ("smooth", (250, 33))):
        d = _dev(torch, L, family, W, H)
        N = d.N
        h, _ = vectors(d)
        rng = np.random.default_rng([17, N])
        aN_p, aD_p, bN_p = (rng.uniform(0.5, 2.0, 5).astype(F32) for _ in range(3))
        alpha = sk.div32(sk.sum_partials(aN_p), sk.sum_partials(aD_p), True); beta = sk.div32(sk.sum_partials(bN_p), sk.sum_partials(aN_p), True)
        for form in forms_for(W)[1:]:
            pl = d.planes(form)
            s = d.system(form)
            for with_delta in (True, False):
                set_form(L, form)
                x = _dvecs(d, h)
                sums = [sk.dbuf(torch, a) for a in (aN_p, aD_p, bN_p)]
                S = [sk.sumt(a) for a in sums]
                o = SimpleNamespace(r=sk.DVec(torch, N), Ap=sk.DVec(torch, N), p=sk.DVec(torch, N), aD=sk.canary_buf(torch, PSLOTS), s3=sk.canary_buf(torch, 3 * PSLOTS, np.float64),
                                    words=sk.canary_buf(torch, 2 + TAIL), tickets=sk.dbuf(torch, np.zeros(sk.FIN_TICKET_WORDS, np.uint32)), aNt=sk.dbuf(torch, np.array([FIN_AN], F32)))
                fin = sk.FinT(sk.sumt(o.aNt), o.tickets.data_ptr(), o.words.data_ptr(), o.words.data_ptr() + 4)
                ret = L.thallo_hip_sfs_pcg_iter(*d.geo(), pl.G.data_ptr(), pl.Wt.data_ptr(), pl.fl.data_ptr(), x.r.ptr, o.r.ptr, x.Ap_prev.ptr, o.Ap.ptr, x.p_prev.ptr, o.p.ptr,
                                                x.delta.ptr if with_delta else None, first, *S, o.aD.data_ptr(), o.s3.data_ptr(), fin, None)
                torch.cuda.synchronize()
                assert ret > 0, ret
                # float64
                r1, p1, d1 = sk.ref_pcg_update(h.r, x.Ap_prev.h0[:N], None, h.p, x.delta.h0[:N], alpha, beta, first)
                rr, pp = o.r.get()[:N], o.p.get()[:N]
                mag_r = np.abs(h.r.astype(np.float64)) + abs(float(alpha)) * np.abs(x.Ap_prev.h0[:N].astype(np.float64))
                _note(f"pcg_iter [{form}] r", np.abs(rr - r1), sk.tol(2, mag_r))
                _note(f"pcg_iter [{form}] p", np.abs(pp - p1), sk.tol(4, mag_r + abs(float(beta)) * np.abs(h.p.astype(np.float64))))
                if with_delta and not first:
                    _note(f"pcg_iter [{form}] delta", np.abs(x.delta.get()[:N] - d1), sk.tol(2, np.abs(x.delta.h0[:N].astype(np.float64)) + abs(float(alpha)) * np.abs(h.p.astype(np.float64))))
                else:
                    assert x.delta.unchanged()
                want, mag = s.apply(pp)
                Ap = o.Ap.get()[:N]
                _note(f"pcg_iter [{form}] Ap", np.abs(Ap - want), sk.tol(K_AP, mag))
                aD, s3 = partials(o.aD, ret), partials(o.s3, ret, 3)
                check_sum(f"pcg_iter [{form}] alphaD", aD, pp.astype(np.float64) * Ap, 1, H)
                for j, terms in enumerate(sr.terms_NS1S2(rr, Ap)):
                    check_sum(f"pcg_iter [{form}] {{N, S1, S2}}", s3[:, j], terms, 2, H, eps=EPS64)
                w = o.words.cpu().numpy()
                adw, _, bnw, _ = sk.ref_scalars_finish(aD, s3.ravel(), F32(FIN_AN))
                assert sk.same_bytes(w[0:1], adw) and sk.ulp_apart(w[1], bnw) <= 1 and (w[2:].view(np.uint32) == sk.CANARY).all()
                for vec in (o.r, o.Ap, o.p, x.r, x.Ap_prev, x.p_prev): assert vec.canary_ok()
                assert x.r.unchanged() and x.Ap_prev.unchanged() and x.p_prev.unchanged()
                if not with_delta:              # (thallo_hip_pcg_update has no form without delta: the launch must leave what the one with delta left)
                    assert all(sk.same_bytes(a, b) for a, b in zip(kept, (rr, pp, Ap, aD, s3, w)))
                    continue
                kept = (rr, pp, Ap, aD, s3, w)
                # the two launches it replaces
                y = _dvecs(d, h)
                q = SimpleNamespace(p=sk.DVec(torch, N), Ap=sk.canary_buf(torch, N + TAIL), aD=sk.canary_buf(torch, PSLOTS), s3=sk.canary_buf(torch, 3 * PSLOTS, np.float64),
                                    words=sk.canary_buf(torch, 2 + TAIL), tickets=sk.dbuf(torch, np.zeros(sk.FIN_TICKET_WORDS, np.uint32)))
                assert L.thallo_hip_pcg_update(y.r.ptr, y.Ap_prev.ptr, None, y.p_prev.ptr, q.p.ptr, y.delta.ptr, N, first, *S, None) >= 0
                fin2 = sk.FinT(sk.sumt(o.aNt), q.tickets.data_ptr(), q.words.data_ptr(), q.words.data_ptr() + 4)
                ret2 = L.thallo_hip_sfs_apply_jtj_sums_fin(*d.geo(), pl.G.data_ptr(), pl.Wt.data_ptr(), pl.fl.data_ptr(), d.U.data_ptr(), d.R.data_ptr(), q.p.ptr, q.Ap.data_ptr(),
                                                           q.aD.data_ptr(), y.r.ptr, q.s3.data_ptr(), fin2, None)
                torch.cuda.synchronize()
                assert ret2 == ret
                assert sk.same_bytes(y.r.get()[:N], rr) and sk.same_bytes(q.p.get()[:N], pp) and sk.same_bytes(q.Ap.cpu().numpy()[:N], Ap), (form, first, with_delta)
                assert sk.same_bytes(y.delta.get()[:N], x.delta.get()[:N])
                assert sk.same_bytes(q.aD.cpu().numpy(), o.aD.cpu().numpy()) and sk.same_bytes(q.s3.cpu().numpy(), o.s3.cpu().numpy()) and sk.same_bytes(q.words.cpu().numpy(), w)
        d.inputs_unchanged()


def test_apply_jtj_lm_pupdate(torch, L):
    """thallo_hip_sfs_apply_jtj_lm_pupdate (first 0 and 1, a gate that is set): p_out = z + beta p_in on the rows, Ap = (J^T J + CtC) p_out, the alphaD partials"""
    assert L.thallo_hip_sfs_lm_pupdate_supported() == 1
    for family, (W, H) in (("holes", (130, 17)), ("masks", (62, 3)), ("degenerate", (61, 5))):
        d = _dev(torch, L, family, W, H)
        N = d.N
        h, v = vectors(d)
        rng = np.random.default_rng([19, N])
        zh = rng.standard_normal(N).astype(F32)
        aN_p, bN_p = rng.uniform(0.5, 2.0, 5).astype(F32), rng.uniform(0.5, 2.0, 3).astype(F32)
        beta = sk.div32(sk.sum_partials(bN_p), sk.sum_partials(aN_p), False)
        for form in forms_for(W)[1:]:
            pl = d.planes(form); s = d.system(form)
            for first, gate in ((1, None), (0, None), (0, 0), (0, 1)):
                set_form(L, form)
                z = sk.dbuf(torch, np.concatenate([zh, np.zeros(TAIL, F32)]))
                sums = [sk.dbuf(torch, a) for a in (aN_p, bN_p)]
                o = SimpleNamespace(p=sk.canary_buf(torch, N + TAIL), Ap=sk.canary_buf(torch, N + TAIL), aD=sk.canary_buf(torch, PSLOTS))
                g = None if gate is None else sk.dbuf(torch, np.array([gate, 0], np.uint32))
                ret = L.thallo_hip_sfs_apply_jtj_lm_pupdate(*d.geo(), pl.G.data_ptr(), pl.Wt.data_ptr(), pl.fl.data_ptr(), z.data_ptr(), v.p.data_ptr(), o.p.data_ptr(), v.ctc.data_ptr(),
                                                            o.Ap.data_ptr(), o.aD.data_ptr(), first, sk.sumt(sums[0]), sk.sumt(sums[1]), None if g is None else g.data_ptr(), None)
                torch.cuda.synchronize()
                assert ret > 0
                if gate == 1:
                    for t in (o.p, o.Ap, o.aD): assert (t.cpu().numpy().view(np.uint32) == sk.CANARY).all(), "a gated launch wrote"
                    continue
                pp = rows_of(o.p.cpu().numpy(), d).ravel()
                want_p = sk.ref_step3(h.p, zh, 0.0 if first else beta)
                _note(f"apply_jtj_lm_pupdate [{form}] p", np.abs(pp - want_p), sk.tol(2, np.abs(zh.astype(np.float64)) + abs(float(beta)) * np.abs(h.p.astype(np.float64))))
                want, mag = s.apply(pp, h.ctc)
                Ap = rows_of(o.Ap.cpu().numpy(), d).ravel()
                _note(f"apply_jtj_lm_pupdate [{form}] Ap", np.abs(Ap - want), sk.tol(K_LM, mag))
                check_sum(f"apply_jtj_lm_pupdate [{form}] alphaD", partials(o.aD, ret), pp.astype(np.float64) * Ap, 1, H)
        d.inputs_unchanged()


def test_pcg_init_lm(torch, L):
    """thallo_hip_sfs_pcg_init_lm (packed planes; save_ssq 1 and 0): r and the raw diagonal as thallo_hip_sfs_pcg_init leaves them (r, p_prev, delta bit for bit), and from
    the diagonal SSq = 1 (save_ssq; otherwise the plane -- filled with other values here -- is neither read nor written and the launch computes with 1), CtC, M^-1, b = r, z = M^-1 r against sk.ref_lm_finalize in float64; on the float4 planes the entry point refuses and writes nothing"""
    radius, lo, hi = 1e4, 1e-6, 1e32
    for family, (W, H) in (("holes", (130, 17)), ("masks", (62, 3)), ("degenerate", (126, 9))):
        d = _dev(torch, L, family, W, H)
        N = d.N
        pl = d.planes("pair")
        base = run_init(d, "pair")
        dg = base.diag.cpu().numpy()[:N].astype(np.float64)
        rh = base.r.cpu().numpy()[:N]
        ssq_in = np.random.default_rng([23, N]).uniform(0.01, 1.0, N).astype(F32)      # NOT ones: without save_ssq the launch neither reads nor writes the plane and computes with 1 (thallo_hip.h)
        for save in (1, 0):
            set_form(L, "pair")
            o = SimpleNamespace(**{k: sk.canary_buf(torch, N + TAIL) for k in ("r", "z", "p_prev", "delta", "CtC", "pre", "b")}, aN=sk.canary_buf(torch, PSLOTS))
            o.SSq = sk.canary_buf(torch, N + TAIL) if save else sk.dbuf(torch, np.concatenate([ssq_in, np.full(TAIL, sk.CANARY, np.uint32).view(F32)]))
            ret = L.thallo_hip_sfs_pcg_init_lm(*d.geo(), d.X.data_ptr(), d.D.data_ptr(), pl.G.data_ptr(), pl.Wt.data_ptr(), pl.fl.data_ptr(), o.r.data_ptr(), o.z.data_ptr(),
                                               o.p_prev.data_ptr(), o.delta.data_ptr(), o.SSq.data_ptr(), o.CtC.data_ptr(), o.pre.data_ptr(), o.b.data_ptr(), radius, lo, hi, save,
                                               o.aN.data_ptr(), None)
            torch.cuda.synchronize()
            assert ret > 0, ret
            get = lambda k: rows_of(getattr(o, k).cpu().numpy(), d).ravel()
            assert sk.same_bytes(get("r"), rh) and sk.same_bytes(get("b"), rh) and not get("p_prev").view(np.uint32).any() and not get("delta").view(np.uint32).any()
            SSq, CtC, pre, b, z, _ = sk.ref_lm_finalize(dg, np.ones(N), rh, radius, lo, hi, save, False)      # (this energy has no preconditioner: SSq = 1 when saved)
            # the device forms them from ITS diagonal (K_DIAG on the reference's magnitude, held above); from there: the clamps' quotients 3, M^-1 4 more
            if save:
                assert np.array_equal(get("SSq").astype(np.float64), SSq)
            else:
                assert sk.same_bytes(o.SSq.cpu().numpy()[:N], ssq_in)
            _note("pcg_init_lm CtC", np.abs(get("CtC") - CtC), sk.tol(10, CtC))
            _note("pcg_init_lm pre", np.abs(get("pre") - pre), sk.tol(16, pre))
            _note("pcg_init_lm z", np.abs(get("z") - z), sk.tol(17, np.abs(z)))
            check_sum("pcg_init_lm alphaN", partials(o.aN, ret), rh.astype(np.float64) * get("z"), 1, H)
        for form in ("tile", "march"):
            set_form(L, form)
            lp = d.planes(form)
            set_form(L, form)
            bufs = [sk.canary_buf(torch, N + TAIL) for _ in range(9)]
            assert L.thallo_hip_sfs_pcg_init_lm(*d.geo(), d.X.data_ptr(), d.D.data_ptr(), lp.G.data_ptr(), lp.Wt.data_ptr(), lp.fl.data_ptr(), *[b_.data_ptr() for b_ in bufs[:8]],
                                               radius, lo, hi, 1, bufs[8].data_ptr(), None) == sk.NOT_SUPPORTED
            torch.cuda.synchronize()
            for b_ in bufs: assert (b_.cpu().numpy().view(np.uint32) == sk.CANARY).all()
        d.inputs_unchanged()


# ------------------------------------------------------------------ refusals
def test_refusals(torch, L):
    """each -hipErrorInvalidValue / -hipErrorNotSupported the header promises for the launches above, with nothing written"""
    d = _dev(torch, L, "smooth", 62, 3)
    N = d.N
    h, v = vectors(d)
    out = [sk.canary_buf(torch, N + TAIL) for _ in range(6)]
    part, s3 = sk.canary_buf(torch, PSLOTS), sk.canary_buf(torch, 3 * PSLOTS, np.float64)
    for form in FORMS:
        pl = d.planes(form)
        set_form(L, form)
        P = (pl.G.data_ptr(), pl.Wt.data_ptr(), pl.fl.data_ptr())
        for r0, r1 in ((2, 2), (3, 1), (0, d.H + 1), (-1, 2)):
            geo = d.geo(r0, r1)
            if form != "pair":
                assert L.thallo_hip_sfs_cost(*geo, d.X.data_ptr(), d.D.data_ptr(), *P, part.data_ptr(), None) == sk.INVALID
            assert L.thallo_hip_sfs_pcg_init(*geo, d.X.data_ptr(), d.D.data_ptr(), *P, d.U.data_ptr(), d.R.data_ptr(), *[o.data_ptr() for o in out[:5]], part.data_ptr(), None) == sk.INVALID
            head = geo + P + (d.U.data_ptr(), d.R.data_ptr(), v.p.data_ptr(), out[0].data_ptr(), part.data_ptr())
            assert L.thallo_hip_sfs_apply_jtj(*head, None) == sk.INVALID
            assert L.thallo_hip_sfs_apply_jtj_sums(*head, v.r.data_ptr(), s3.data_ptr(), None) == sk.INVALID
        head = d.geo() + P + (d.U.data_ptr(), d.R.data_ptr(), v.p.data_ptr(), out[0].data_ptr(), part.data_ptr())
        assert L.thallo_hip_sfs_apply_jtj_sums(*head, None, s3.data_ptr(), None) == sk.INVALID
        assert L.thallo_hip_sfs_apply_jtj_sums(*head, v.r.data_ptr(), None, None) == sk.INVALID
        assert L.thallo_hip_sfs_apply_jtj_sums_fin(*head, None, s3.data_ptr(), sk.NO_FIN, None) == sk.INVALID
        tick = sk.dbuf(torch, np.zeros(sk.FIN_TICKET_WORDS, np.uint32))
        assert L.thallo_hip_sfs_apply_jtj_sums_fin(*head, v.r.data_ptr(), s3.data_ptr(), sk.FinT(sk.sumt(part, 1), tick.data_ptr(), None, None), None) == sk.INVALID
        assert L.thallo_hip_sfs_precompute_cost(*d.geo(0, d.H), d.X.data_ptr(), d.D.data_ptr(), d.Im.data_ptr(), d.mR.data_ptr(), d.mC.data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                out[3].data_ptr(), 0, d.H, None, None) == sk.INVALID
        S1 = sk.sumt(part, 1)
        it = d.geo() + P
        if form == "tile":      # the one-launch iterations are marching kernels
            assert L.thallo_hip_sfs_pcg_iter(*it, v.r.data_ptr(), out[0].data_ptr(), v.p.data_ptr(), out[1].data_ptr(), v.ctc.data_ptr(), out[2].data_ptr(), None, 1, S1, S1, S1,
                                             part.data_ptr(), s3.data_ptr(), sk.NO_FIN, None) == sk.NOT_SUPPORTED
            assert L.thallo_hip_sfs_apply_jtj_lm_pupdate(*it, v.r.data_ptr(), v.p.data_ptr(), out[0].data_ptr(), v.ctc.data_ptr(), out[1].data_ptr(), part.data_ptr(), 1, S1, S1, None,
                                                         None) == sk.NOT_SUPPORTED
            assert L.thallo_hip_sfs_march_fits(d.W) == 0 and L.thallo_hip_sfs_lm_pupdate_supported() == 0
        else:
            # r_in == r_out, p_in == p_out, no s3
            assert L.thallo_hip_sfs_pcg_iter(*it, v.r.data_ptr(), v.r.data_ptr(), v.p.data_ptr(), out[1].data_ptr(), v.ctc.data_ptr(), out[2].data_ptr(), None, 1, S1, S1, S1,
                                             part.data_ptr(), s3.data_ptr(), sk.NO_FIN, None) == sk.INVALID
            assert L.thallo_hip_sfs_pcg_iter(*it, v.r.data_ptr(), out[0].data_ptr(), v.p.data_ptr(), out[1].data_ptr(), v.ctc.data_ptr(), v.ctc.data_ptr(), None, 1, S1, S1, S1,
                                             part.data_ptr(), s3.data_ptr(), sk.NO_FIN, None) == sk.INVALID
            assert L.thallo_hip_sfs_pcg_iter(*it, v.r.data_ptr(), out[0].data_ptr(), v.p.data_ptr(), out[1].data_ptr(), v.ctc.data_ptr(), out[2].data_ptr(), None, 1, S1, S1, S1,
                                             part.data_ptr(), None, sk.NO_FIN, None) == sk.INVALID
            assert L.thallo_hip_sfs_apply_jtj_lm_pupdate(*it, v.r.data_ptr(), v.p.data_ptr(), v.p.data_ptr(), v.ctc.data_ptr(), out[1].data_ptr(), part.data_ptr(), 1, S1, S1, None,
                                                         None) == sk.INVALID
        torch.cuda.synchronize()
        for t in out + [part, s3]:
            assert (t.cpu().numpy().view(np.uint32) == sk.CANARY).all(), "a refused call wrote"
    d.inputs_unchanged()


# ------------------------------------------------------------------ the two-pass form, in one fresh child
def two_pass_child(path):
    """runs in the child (THALLO_AB=sfs_fused=0: k_rows + k_gather): the same comparison for pcg_init and apply_jtj on one shape, and the bytes for the parent"""
    import torch as t
    L = sk.shim()
    try:
        d = Dev(t, L, sr.case("holes", 130, 17))
        h, v = vectors(d)
        assert L.thallo_hip_sfs_march_fits(d.W) == 0 and L.thallo_hip_sfs_planes_layout(d.W, d.H) == 0, "the child does not run the two-pass form"
        o = run_init(d, "tile")
        r = check_init(d, "tile", o)
        oa = run_apply(d, "tile", "sums", v)
        Ap, aD, s3 = check_apply("apply_jtj [two-pass]", d, "tile", oa, h, sums=True)
        assert not (d.U.cpu().numpy()[:2 * d.N].view(np.uint32) == sk.CANARY).all(), "the scratch planes were not used: not the two-pass form"
        np.savez(path, r=r, diag=o.diag.cpu().numpy(), aN=o.aN.cpu().numpy(), Ap=Ap, aD=aD, s3=s3)
    finally:
        restore(L)


@pytest.fixture(scope="module")
def two_pass(torch, tmp_path_factory):
    """ONE fresh child process with THALLO_AB=sfs_fused=0 (read once per process); returns its exit status, its output and what it saved"""
    path = str(tmp_path_factory.mktemp("sfs") / "two_pass.npz")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, THALLO_AB="sfs_fused=0", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    env.pop("THALLO_SFS_RATIOS", None)
    try:
        res = subprocess.run([sys.executable, "-c", f"import test_gpu_sfs_kernels as m; m.two_pass_child({path!r})"], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"the two-pass child hung: nothing more is started on the device ({e})", returncode=3)
    if res.returncode not in (0, 1):          # (1: a Python exception, such as a failed comparison; anything else -- a signal, an abort -- is a fault: the run ends here)
        pytest.exit(f"the two-pass child ended with status {res.returncode}: nothing more is started on the device\n" + res.stderr[-2000:], returncode=3)
    return SimpleNamespace(rc=res.returncode, out=res.stdout[-2000:] + res.stderr[-4000:], data=np.load(path) if res.returncode == 0 else None)


def test_two_pass_form_in_a_child_process(two_pass):
    """k_rows + k_gather (THALLO_AB=sfs_fused=0) against the reference: PCGInit1 (r, diag, z == r, zeros, alphaN) and applyJTJ with the sums, with this module's bounds"""
    assert two_pass.rc == 0, two_pass.out


def test_k_fused_equals_the_two_pass_form_bit_for_bit(torch, L, two_pass):
    """energy_sfs.hip states of k_fused: "Same expressions in the same order as k_rows / k_gather: bit-identical outputs".  On the `holes` 130 x 17 image, from the same
    planes (k_precompute's): r and the diagonal of PCGInit1 (k_fused<0>) and Ap of applyJTJ (k_fused<1>) byte for byte.  (Before k_rows pinned its contraction per source
    expression, Ap differed at 205 of the 2210 pixels by up to 432 units of the last place, both forms inside K_AP 2^-24 |J|^T |J| |p|: profiles/sfs_kernels/README.md.)"""
    assert two_pass.rc == 0, two_pass.out
    c = two_pass.data
    d = Dev(torch, L, sr.case("holes", 130, 17))                 # (a Dev of its own: the planes by k_precompute, as in the child)
    h, v = vectors(d)
    o = run_init(d, "tile")
    assert sk.same_bytes(rows_of(o.r.cpu().numpy(), d), c["r"]) and sk.same_bytes(o.diag.cpu().numpy(), c["diag"]), "k_fused<0> differs from k_rows + k_gather"
    Ap = rows_of(run_apply(d, "tile", "sums", v).Ap.cpu().numpy(), d)
    ne = Ap.view(np.uint32) != c["Ap"].view(np.uint32)
    worst = max([sk.ulp_apart(a, b) for a, b in zip(Ap[ne], c["Ap"][ne])], default=0)
    print(f"k_fused<1> against k_rows + k_gather: {int(ne.sum())} of {Ap.size} pixels differ, by up to {worst} ulp")
    RATIOS["k_fused<1> against k_rows + k_gather: pixels that differ"] = int(ne.sum())
    assert not ne.any(), f"k_fused<1> differs from k_rows + k_gather at {int(ne.sum())} of {Ap.size} pixels, by up to {worst} ulp"


# ------------------------------------------------------------------ through the C ABI
@pytest.mark.parametrize("lm", [False, True])
def test_holes_solve_with_and_without_the_resident_loop(torch, orc, monkeypatch, lm):
    """the `holes` family, 64 x 48, through ThalloSolver with one launch per PCG iteration and with the resident loop (which the existing tests hold bit for bit to the
    marching launches this module pins down): GN and LM follow the oracle's trajectory (COST_RTOL / VEC_RTOL of test_gpu_parity.py's shape_from_shading tests)"""
    import thallo_amd
    from thallo_amd import api
    from helpers import to_device, to_host, rel_err, copy_params
    COST_RTOL, VEC_RTOL, LM_RTOL = 1e-5, 2e-4, 2e-4
    W, H = 64, 48
    params = sr.make("holes", W, H)
    po = copy_params(params)
    kw = dict(nIterations=3, lIterations=8)
    co, _ = orc.Problem(orc.SFS, (W, H), po).solve(**(dict(use_lm=1, trust_region_radius=100.0, q_tolerance=0.01) if lm else {}), **kw)
    runs = []
    for resident in ("0", "1"):
        monkeypatch.setenv("THALLO_RESIDENT", resident)
        dev = to_device(copy_params(params))
        s = api.ThalloSolver((W, H), thallo_amd.energy_file("shape_from_shading"), timing_level=2, **(dict(solverkind="levenberg_marquardt") if lm else {}))
        if lm:
            s.enable_lm(); s.set_solver_parameters(trust_region_radius=100.0, q_tolerance=0.01, **kw)
        else:
            s.set_solver_parameters(**kw)
        pp = s.make_params(dev); s.init(pp)
        costs = [s.current_cost()]
        while s.step(pp):
            costs.append(s.current_cost())
        names = {k for k, v in s.kernel_stats().items() if v["launches"]}; s.close()
        runs.append((np.array(costs), to_host(dev[16]).copy(), names))
    assert "PCGLoopResident" in runs[1][2] and "PCGLoopResident" not in runs[0][2], (runs[0][2], runs[1][2])
    for c, X, _ in runs:
        m = min(len(c), len(co))
        print("holes solve", "LM" if lm else "GN", "costs", c, co, "X", rel_err(X, po[16]))
        assert m >= 3
        if lm:
            assert (np.abs(c[:m] - co[:m]) <= LM_RTOL * np.abs(co[:m]) + 1e-9).all(), (c, co)
        else:
            assert len(c) == len(co) and rel_err(c, co) < COST_RTOL, (c, co)
            assert rel_err(X, po[16]) < VEC_RTOL


# ------------------------------------------------------------------ the deferred finish, the one-launch LM iteration, the LM model cost
def _iter_call(L, d, pl, x, o, delta, first, S=None, prev=None, fin=sk.NO_FIN):
    head = d.geo() + (pl.G.data_ptr(), pl.Wt.data_ptr(), pl.fl.data_ptr(), x.r.ptr, o.r.ptr, x.Ap_prev.ptr, o.Ap.ptr, x.p_prev.ptr, o.p.ptr, delta, first)
    if prev is None:
        return L.thallo_hip_sfs_pcg_iter(*head, *S, o.aD.data_ptr(), o.s3.data_ptr(), fin, None)
    return L.thallo_hip_sfs_pcg_iter_deferred(*head, S[0], prev, o.aD.data_ptr(), o.s3.data_ptr(), None)


def _iter_out(torch, N):
    return SimpleNamespace(r=sk.DVec(torch, N), Ap=sk.DVec(torch, N), p=sk.DVec(torch, N), aD=sk.canary_buf(torch, PSLOTS), s3=sk.canary_buf(torch, 3 * PSLOTS, np.float64))


@pytest.mark.parametrize("first", [0, 1])
def test_pcg_iter_deferred(torch, L, first):
    """thallo_hip_sfs_pcg_iter_deferred: the two words of iteration k-1 from its partials (alphaD bit-exact in the documented order, betaN to 1 ulp), and everything else
    the bytes of thallo_hip_sfs_pcg_iter (held to float64 above) called with those words as its scalars -- "the same order, the same bits"; first: the partials are not read"""
    for family, (W, H) in (("holes", (130, 17)), ("masks", (62, 3)), ("steps", (61, 5))):
        d = _dev(torch, L, family, W, H)
        N = d.N
        h, _ = vectors(d)
        rng = np.random.default_rng([29, N])
        count = 7
        aD_prev = rng.uniform(0.5, 2.0, count).astype(F32)
        s3_prev = np.stack([rng.uniform(0.5, 2.0, count), rng.uniform(-0.1, 0.1, count), rng.uniform(0.0, 0.1, count)], 1)
        aN = np.array([0.01], F32)
        for form in forms_for(W)[1:]:
            pl = d.planes(form)
            set_form(L, form)
            x, o = _dvecs(d, h), _iter_out(torch, N)
            aNt, aDt, s3t, words = sk.dbuf(torch, aN), sk.dbuf(torch, aD_prev), sk.dbuf(torch, s3_prev), sk.canary_buf(torch, 2 + TAIL)
            prev = sk.PrevT(aDt.data_ptr(), s3t.data_ptr(), count, words.data_ptr(), words.data_ptr() + 4)
            ret = _iter_call(L, d, pl, x, o, x.delta.ptr, first, S=[sk.sumt(aNt)], prev=prev)
            torch.cuda.synchronize()
            assert ret > 0, ret
            w = words.cpu().numpy()
            if first:
                assert (w.view(np.uint32) == sk.CANARY).all()
                S = [sk.sumt(aNt)] * 3
            else:
                adw, alpha, bnw, mag = sk.ref_scalars_finish(aD_prev, s3_prev.ravel(), aN[0])
                assert sk.same_bytes(w[0:1], adw) and sk.ulp_apart(w[1], bnw) <= 1 and (w[2:].view(np.uint32) == sk.CANARY).all(), (w[:2], adw, bnw)
                wt = sk.dbuf(torch, w[:2].copy())
                S = [sk.sumt(aNt), api_sum(wt, 0), api_sum(wt, 1)]
            y, q = _dvecs(d, h), _iter_out(torch, N)
            assert _iter_call(L, d, pl, y, q, y.delta.ptr, first, S=S) == ret
            torch.cuda.synchronize()
            for a, b in ((o.r, q.r), (o.Ap, q.Ap), (o.p, q.p), (x.delta, y.delta)):
                assert sk.same_bytes(a.get(), b.get()), (form, first)
            assert sk.same_bytes(o.aD.cpu().numpy(), q.aD.cpu().numpy()) and sk.same_bytes(o.s3.cpu().numpy(), q.s3.cpu().numpy())
            partials(o.aD, ret); partials(o.s3, ret, 3)
        d.inputs_unchanged()


def api_sum(t, word):
    """thallo_sum_t over one word of a device tensor"""
    from thallo_amd import api
    return api.SumT(t.data_ptr() + 4 * word, 1)


@pytest.mark.parametrize("first", [0, 1])
def test_pcg_iter_lm(torch, L, first):
    """thallo_hip_sfs_pcg_iter_lm: r_k, delta_k, p_k = M^-1 r_k + beta p_{k-1}, (J^T J + CtC) p_k per pixel; the alphaD, {N, S1, S2} (with M^-1) and {U, T1, T2} partials; the
    last workgroup's words from those partials by the formulas of the header (alphaD bit-exact, betaN and Q1 to 1 ulp; unguarded quotients); the zeta test with a
    tolerance that never / always stops; a gate that is already set: nothing is written"""
    for family, (W, H) in (("holes", (130, 17)), ("masks", (62, 3)), ("degenerate", (61, 5))):
        d = _dev(torch, L, family, W, H)
        N = d.N
        h, _ = vectors(d)
        rng = np.random.default_rng([31, N])
        bh, preh = rng.standard_normal(N).astype(F32), rng.uniform(0.25, 2.0, N).astype(F32)
        aN_p, aD_p, bN_p = (rng.uniform(0.5, 2.0, 5).astype(F32) for _ in range(3))
        alpha = sk.div32(sk.sum_partials(aN_p), sk.sum_partials(aD_p), False); beta = sk.div32(sk.sum_partials(bN_p), sk.sum_partials(aN_p), False)
        kk = 3
        for form in forms_for(W)[1:]:
            pl = d.planes(form); s = d.system(form)
            for q_tol, gate in ((1e-30, 0), (1e30, 0), (1e-30, 1)):
                set_form(L, form)
                x, o = _dvecs(d, h), _iter_out(torch, N)
                ctc, b, pre = sk.DVec(torch, N, h.ctc), sk.DVec(torch, N, bh), sk.DVec(torch, N, preh)
                sums = [sk.dbuf(torch, a) for a in (aN_p, aD_p, bN_p)]
                q3, words, tick, aNt = sk.canary_buf(torch, 3 * PSLOTS, np.float64), sk.canary_buf(torch, 2 + TAIL), sk.dbuf(torch, np.zeros(sk.FIN_TICKET_WORDS, np.uint32)), sk.dbuf(torch, np.array([FIN_AN], F32))
                st0 = np.zeros(8, F32); st0[0] = F32(-1.5); st0.view(np.uint32)[1] = gate; st0.view(np.int32)[2] = 2 if gate else 0
                state = sk.dbuf(torch, st0)
                fin = sk.FinT(sk.sumt(aNt), tick.data_ptr(), words.data_ptr(), words.data_ptr() + 4)
                ret = L.thallo_hip_sfs_pcg_iter_lm(*d.geo(), pl.G.data_ptr(), pl.Wt.data_ptr(), pl.fl.data_ptr(), x.r.ptr, o.r.ptr, x.Ap_prev.ptr, o.Ap.ptr, x.p_prev.ptr, o.p.ptr, x.delta.ptr,
                                                   ctc.ptr, b.ptr, pre.ptr, first, *[sk.sumt(a) for a in sums], o.aD.data_ptr(), o.s3.data_ptr(), q3.data_ptr(), fin, state.data_ptr(), kk,
                                                   q_tol, None)
                torch.cuda.synchronize()
                assert ret > 0, ret
                if gate:
                    for vec in (o.r, o.Ap, o.p): assert vec.unchanged()
                    assert x.delta.unchanged() and sk.same_bytes(state.cpu().numpy(), st0) and (words.cpu().numpy().view(np.uint32) == sk.CANARY).all()
                    assert (o.aD.cpu().numpy().view(np.uint32) == sk.CANARY).all() and (q3.cpu().numpy().view(np.uint32) == sk.CANARY).all()
                    continue
                r1, p1, d1 = sk.ref_pcg_update(h.r, x.Ap_prev.h0[:N], preh, h.p, x.delta.h0[:N], alpha, beta, first)
                rr, pp, dd = o.r.get()[:N], o.p.get()[:N], x.delta.get()[:N]
                a64 = lambda v: np.abs(np.asarray(v, np.float64))
                mag_r = a64(h.r) + abs(float(alpha)) * a64(x.Ap_prev.h0[:N])
                _note(f"pcg_iter_lm [{form}] r", np.abs(rr - r1), sk.tol(2, mag_r))
                _note(f"pcg_iter_lm [{form}] p", np.abs(pp - p1), sk.tol(5, a64(preh) * mag_r + abs(float(beta)) * a64(h.p)))
                if first:
                    assert x.delta.unchanged()
                else:
                    _note(f"pcg_iter_lm [{form}] delta", np.abs(dd - d1), sk.tol(2, a64(x.delta.h0[:N]) + abs(float(alpha)) * a64(h.p)))
                want, mag = s.apply(pp, h.ctc)
                Ap = o.Ap.get()[:N]
                _note(f"pcg_iter_lm [{form}] Ap", np.abs(Ap - want), sk.tol(K_LM, mag))
                aD, s3, q3h = partials(o.aD, ret), partials(o.s3, ret, 3), partials(q3, ret, 3)
                check_sum(f"pcg_iter_lm [{form}] alphaD", aD, pp.astype(np.float64) * Ap, 1, H)
                for j, terms in enumerate(sr.terms_NS1S2(rr, Ap, preh)):
                    check_sum(f"pcg_iter_lm [{form}] {{N, S1, S2}}", s3[:, j], terms, 3, H, eps=EPS64)
                for j, terms in enumerate(sr.terms_UT1T2(dd, rr, bh, pp, Ap)):
                    check_sum(f"pcg_iter_lm [{form}] {{U, T1, T2}}", q3h[:, j], terms, 3, H, eps=EPS64)
                w = words.cpu().numpy()
                adw, al, bnw, _ = sk.ref_scalars_finish(aD, s3.ravel(), F32(FIN_AN), guard=False)
                assert sk.same_bytes(w[0:1], adw) and sk.ulp_apart(w[1], bnw) <= 1 and (w[2:].view(np.uint32) == sk.CANARY).all()
                U, T1, T2 = (sk.sum_partials_f64(q3h[:, j]) for j in range(3))
                Q1 = F32(0.5 * (U + float(al) * (T1 - T2) - float(al) * float(al) * float(adw)))
                st = state.cpu().numpy()
                if q_tol < 1:
                    assert sk.ulp_apart(st[0], Q1) <= 1 and sk.same_bytes(st[1:], st0[1:]), (st, Q1)
                else:
                    want_st = st0.copy(); want_st.view(np.uint32)[1] = 1; want_st.view(np.int32)[2] = kk + 1
                    assert sk.same_bytes(st, want_st), (st, want_st)
                assert not tick.cpu().numpy().any()
                for vec in (x.r, x.Ap_prev, x.p_prev, ctc, b, pre): assert vec.unchanged()
        d.inputs_unchanged()


def test_lm_model_cost(torch, L):
    """thallo_hip_sfs_lm_model_cost, the three (gate, done, L) cases of tools/sfs_probe.py check_pair_lm, with and without X / prevX: delta_out = delta + alpha_kl p_kl
    (kl = -1: delta itself, bit for bit), the partials of delta_out . J^T J delta_out and delta_out . b against float64, prevX = X and X + delta_out in float32 exactly;
    on the float4 planes the entry point refuses"""
    for family, (W, H) in (("holes", (130, 17)), ("masks", (62, 3))):
        d = _dev(torch, L, family, W, H)
        N = d.N
        pl = d.planes("pair"); s = d.system("pair")
        rng = np.random.default_rng([37, N])
        dh, pe, po, bh = (rng.standard_normal(N).astype(F32) * F32(sc) for sc in (1e-3, 1e-3, 1e-3, 1.0))
        wordsh = np.array([2.0, 3.0, 5.0, 7.0, 0.75, 1.5, 9.0, 9.0], F32)           # alphaN_k at [2 k], alphaD_k at [2 k + 1]
        Xh = d.g.params[16].ravel()
        for gate, done, Lm in ((0, 0, 3), (1, 2, 3), (0, 0, 0)):
            kl = (done if gate else Lm) - 1
            for with_x in (True, False):
                set_form(L, "pair")
                st = np.zeros(8, F32); st.view(np.uint32)[1] = gate; st.view(np.int32)[2] = done
                delta, dout, pev, pod, b = sk.DVec(torch, N, dh), sk.DVec(torch, N), sk.DVec(torch, N, pe), sk.DVec(torch, N, po), sk.DVec(torch, N, bh)
                words, state = sk.dbuf(torch, wordsh), sk.dbuf(torch, st)
                qa, qb = sk.canary_buf(torch, PSLOTS), sk.canary_buf(torch, PSLOTS)
                X, pX = sk.DVec(torch, N, Xh), sk.DVec(torch, N)
                ret = L.thallo_hip_sfs_lm_model_cost(*d.geo(), pl.G.data_ptr(), pl.Wt.data_ptr(), pl.fl.data_ptr(), delta.ptr, dout.ptr, pev.ptr, pod.ptr, b.ptr, words.data_ptr(),
                                                     words.data_ptr() + 4, 2, state.data_ptr(), Lm, qa.data_ptr(), qb.data_ptr(), X.ptr if with_x else None, pX.ptr if with_x else None, None)
                torch.cuda.synchronize()
                assert ret > 0, ret
                do = dout.get()[:N]
                if kl < 0:
                    assert sk.same_bytes(do, dh)
                else:
                    alpha = sk.div32(wordsh[2 * kl], wordsh[2 * kl + 1], False)
                    pk = pe if kl % 2 == 0 else po
                    _note("lm_model_cost delta_out", np.abs(do - (dh.astype(np.float64) + float(alpha) * pk)), sk.tol(2, np.abs(dh.astype(np.float64)) + abs(float(alpha)) * np.abs(pk.astype(np.float64))))
                want, mag = s.apply(do)
                t1, t2 = sr.terms_model(do, want, bh)
                _note("lm_model_cost delta . J^T J delta", abs(partials(qa, ret).astype(np.float64).sum() - t1.sum()), sk.tol(K_AP + 1 + H + 16, (np.abs(do.astype(np.float64)) * mag).sum()))
                check_sum("lm_model_cost delta . b", partials(qb, ret), t2, 1, H)
                if with_x:
                    assert sk.same_bytes(pX.get()[:N], Xh) and sk.same_bytes(X.get()[:N], (Xh + do).astype(F32)) and pX.canary_ok() and X.canary_ok()
                else:
                    assert X.unchanged() and pX.unchanged()
                assert delta.unchanged() and dout.canary_ok() and sk.same_bytes(state.cpu().numpy(), st)
        lp = d.planes("march")
        set_form(L, "march")
        bufs = [sk.DVec(torch, N, dh) for _ in range(5)]
        qa = sk.canary_buf(torch, PSLOTS)
        assert L.thallo_hip_sfs_lm_model_cost(*d.geo(), lp.G.data_ptr(), lp.Wt.data_ptr(), lp.fl.data_ptr(), *[v.ptr for v in bufs], qa.data_ptr(), qa.data_ptr() + 4, 2, qa.data_ptr(), 3,
                                              qa.data_ptr(), qa.data_ptr(), None, None, None) == sk.NOT_SUPPORTED
        torch.cuda.synchronize()
        assert (qa.cpu().numpy().view(np.uint32) == sk.CANARY).all() and all(v.unchanged() for v in bufs)
        d.inputs_unchanged()
