"""The image-stencil kernels -- image_warping (csrc/energy_image_warping.hip, _march.hip, _march_rc.hip, _resident.hip) and laplacian_image
(energy_laplacian_image.hip) -- entry point by entry point and form by form against the float64 references of tests/iw_reference.py.

Every pixel of every case (iw.CASES: tile and strip geometry, row ranges with ghost rows, hand-written masks, constraints, four UrShapes, angles in +-3 rad, three
exact cases) is compared; no owned entry is left out.  Outputs go into canary-filled buffers (sk.CANARY, a NaN pattern) and everything a launch does not own must keep
it: the rows outside what include/thallo_hip.h says the launch writes, the tail behind every buffer, the partial slots behind the returned count.  The ghost-row
writes the header promises (pcg_init: cs, bit 0 of flags, p_prev = 0; pcg_step1 and the one-kernel iteration: p, r kept current) are compared with the reference
like owned rows.  Inputs are compared byte for byte after every launch.

The planes fed to the iteration kernels are random float32 vectors, zero at excluded unknowns -- not solver state -- and (cos, sin), the flags byte and M^-1 are
inputs made on the host, so a bound covers the roundings of the one launch under test.  Bounds are absolute error arrays built from sk.tol(k, S): S the reference's
float64 sum of the absolute values of the terms, k the number of float32 roundings on the longest chain of operations, counted from the operations of the formula
as if nothing were contracted into an fma (contraction only removes roundings), and propagated through J^T J with its absolute operator (iw.Stencil.apply's S):

  T          relative error of one device sine / cosine in units of 2^-24: TRIG = 2 x the worst value measured on the MI355X over this file's own angles
             (profiles/iw_kernels/README.md; the factor 2 because that set is finite).  Only pcg_init and the cost kernel call sincosf.
  K_E        = T + 4   a component of e = (o_i - o_j) - R(a_i)(u_i - u_j): u_i - u_j (1), its product with cos / sin (T + 1), the sum of two (1), the difference (1)
  K_G        = T + 3   a component of g = R'(a_i)(u_i - u_j): the same without the last difference
  K_COST     = 2 K_E + 9   a pixel's cost share: the weight (1), the square doubles the error and rounds (1), the sum of two squares (1), five running additions
  K_R        = K_G + K_E + 7   r: an Angle entry adds four terms g . e: product (K_G + K_E + 1), sum of two (1), four running additions... (3 more), w_reg^2 (2);
                               an Offset entry (K_E + 8: e_i - e_j, four additions, w_reg^2, the fit term) is shorter
  K_D        = 2 K_G + 8   raw diagonal: g . g per direction (2 K_G + 2), four additions, w_reg^2 (2); the Offset entries (2 cnt w_reg^2 + w_fit^2: 4) are shorter
  K_PRE      = K_D + 4     1 / (1 + sqrt d)^2: d's error passes with a factor sqrt d / (1 + sqrt d) < 1; sqrt, sum, square, quotient (correctly rounded)
  K_Z        = K_PRE + K_R + 1
  K_M = 8    M^-1 from the flags byte: w_reg^2 (1), its product with 2 cnt (1), w_fit^2 (1), the sum (1), then as K_PRE (4).  0 where M^-1 is the input plane `pre`.
  K_AP = 16  J^T J p with (cos, sin) given: u_i - u_j (1), g (2 more), g pa_i (1), e = dp - g pa_i (1): 5; g . e: 5 + 3 + 1, the sum of two (1), four running
             additions (4), w_reg^2 (2): 16 for an Angle entry; an Offset entry (14) is shorter.  On the unit grid g is exact and the chain is 11.
  delta      2 per `delta += alpha p` (an fma on the device: 1)
  r_out      2 (r - alpha Ap; an fma on the device)
  p_out      K_M + 1 on M^-1 r, r's own error times M^-1, 2 for beta p and the sum
An error of p costs A p |J^T J| times that error, an error of A p costs r alpha times it: added as arrays.  A partial (one per workgroup) is compared with the
float64 sum of the DEVICE's own per-pixel outputs, which the same test has just checked: 3 roundings per pixel (a product, two additions) + one addition per pixel a
thread visits + 6 butterfly levels + 8 waves; the double sums N, S1, S2 the same in units of 2^-53, plus K_M 2^-24 where M^-1 is recomputed on the device.  Which
workgroup owns which pixel: iw.tile_blocks for the tile kernels, thallo_hip_iw_march_place for the marching kernels.

alpha and beta are reproduced bit for bit with sk.div32 from the words or partials a launch is handed.  In the exact cases every float32 operation is exact (M^-1
from the flags byte aside, whose bits iw.pre_from_flags_f32 has): planes must equal the reference bit for bit and sums exactly (sk.assert_exact_sums), so a pixel
counted twice or not at all at a seam fails with zero tolerance.

thallo_hip_iw_pcg_step2's partials are held to their float64 total, not per workgroup: its generic branch is thallo_hip_pcg_step2 / _ranges, whose partials
test_gpu_pcg_chain.py pins per workgroup.

Out of scope here: every `dist` / peer-to-peer form (test_gpu_distributed.py and test_gpu_transport_kernels.py own those), the research and persist kernels, and
thallo_hip_resident_debug_set(2, ...), the fault injection.

With THALLO_IW_RATIOS=<file> the worst error / bound ratio per output and form, and the module's run time, go to that file (profiles/iw_kernels/ratios.json)."""
import ctypes as C
import functools
import json
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest

import iw_reference as iw
import shim_kernels as sk
from shim_kernels import F32

pytestmark = pytest.mark.gpu

TRIG_MEASURED = 1.9085       # worst |sincosf - sin / cos| / (2^-24 |sin / cos|) on the MI355X over all_angles() (profiles/iw_kernels/README.md)
TRIG = 2.0 * TRIG_MEASURED
K_E, K_G = TRIG + 4, TRIG + 3
K_COST = 2 * K_E + 9
K_R = K_G + K_E + 7
K_D = 2 * K_G + 8
K_PRE = K_D + 4
K_Z = K_PRE + K_R + 1
K_M, K_AP = 8, 16
K_LAP = 12                   # laplacian_image: w (w v) (2), four differences (1 each) and their running additions (4), the sum of both parts (1), the sign: 12 with p = z + beta p's 2 in front
PSLOTS = sk.MAX_PARTIALS + 8
TAIL = 64                    # canary words behind every output
EPS64 = 2.0 ** -53
WAVES = 8                    # the widest workgroup (512 threads)

RATIOS = {}
ALL = list(iw.CASES)
GRID = [n for n in ALL if iw.CASES[n][2] in ("unit", "shift")]
MARCHABLE = [n for n in GRID if iw.CASES[n][0] % 2 == 0]
MODES = (1, 0, 2, 4)         # THALLO_IW_STEP1_MODE's values: first, every iteration, deferred, two updates


def _note(kernel, err, bound):
    """asserts err <= bound everywhere and keeps the worst ratio"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64) + np.zeros_like(np.asarray(err, np.float64))
    bad = ~(err <= bound)                                                   # (NaN counts as bad)
    with np.errstate(all="ignore"):
        ratio = float(np.nanmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))) if err.size else 0.0
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    assert not bad.any(), (kernel, np.argwhere(bad)[:8].tolist(), ratio, "errors", np.atleast_1d(err)[np.atleast_1d(bad)][:4].tolist(), "bounds", np.atleast_1d(bound)[np.atleast_1d(bad)][:4].tolist())


DELTA_K = {0: 2, 1: 0, 2: 4}      # roundings of the delta update by its mode: one `delta += alpha p` (2), none, two


def _bits_either(kernel, got, w1, w2):
    """bit for bit one of two values: p = M^-1 r + beta p with an inexact M^-1 may round M^-1 r first or fuse it into the sum"""
    got = np.asarray(got)
    RATIOS.setdefault(kernel + " (bitwise)", 0.0)
    bad = ~((got == np.asarray(w1).astype(got.dtype)) | (got == np.asarray(w2).astype(got.dtype)))
    assert not bad.any(), (kernel, np.argwhere(bad)[:8].tolist(), got[bad][:4].tolist(), np.asarray(w1)[bad][:4].tolist())


def block3(blk, own):
    """the workgroup of every owned entry of a flat vector"""
    return iw.pack(np.repeat(blk[..., None], 2, -1), blk)[own]


def _bits(kernel, got, want):
    """bit-for-bit (the sign of zero aside: x - x and 0 * -1 are written either way)"""
    got, want = np.asarray(got), np.asarray(want)
    RATIOS.setdefault(kernel + " (bitwise)", 0.0)
    bad = ~((got == want.astype(got.dtype)) & (want.astype(got.dtype) == want))
    assert not bad.any(), (kernel, np.argwhere(bad)[:8].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


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
    path = os.environ.get("THALLO_IW_RATIOS")
    if path:
        RATIOS["module run time in seconds"] = round(time.time() - t0, 1)
        json.dump(RATIOS, open(path, "w"), indent=1, sort_keys=True)


def restore(L):
    L.thallo_hip_march_debug_set(0, 0); L.thallo_hip_march_debug_set(6, 0)
    L.thallo_hip_resident_debug_set(0, 0); L.thallo_hip_resident_debug_set(1, 0); L.thallo_hip_resident_debug_set(3, -1)


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


# ------------------------------------------------------------------ buffers
def out3(torch, N):
    return sk.canary_buf(torch, 3 * N + TAIL)


def in3(torch, v, N):
    """an input plane as the solver pads its vectors: the payload, zeros up to a multiple of 4 floats, the canary behind"""
    h = np.full(3 * N + TAIL, sk.CANARY, np.uint32).view(F32)
    h[:3 * N] = v; h[3 * N:sk.ceil4(3 * N)] = 0
    return sk.dbuf(torch, h)


def byte_buf(torch, N, payload=None):
    """the flags plane: N bytes (+ up to 3 of padding the dword reads may touch) and 64 canary bytes (0xA5) behind"""
    n4 = (N + 3) // 4 * 4
    h = np.full(n4 + 64, 0xA5, np.uint8)
    if payload is not None:
        h[:N] = np.asarray(payload, np.uint8).reshape(-1); h[N:n4] = 0
    return sk.dbuf(torch, h)


def word(torch, v, dtype=np.int32):
    return sk.dbuf(torch, np.array([v] + [0] * 15, dtype))


def host(t):
    return t.cpu().numpy()


def canary_elsewhere(h, written, what):
    """every 32-bit word of the buffer outside `written` (a bool array over its first words) still holds the canary"""
    w = np.ascontiguousarray(h).view(np.uint32)
    m = np.zeros(w.size, bool); m[:written.size] = written
    assert (w[~m] == sk.CANARY).all(), f"{what}: written outside what the launch owns at words {np.flatnonzero((w != sk.CANARY) & ~m)[:8].tolist()}"


def slots(buf, count, width=1):
    """exactly `count` leading slots were written; returns them"""
    h = host(buf)
    h = h.reshape(-1, width) if width > 1 else h
    assert sk.written_slots(h) == count, (sk.written_slots(h), count)
    return h[:count]


def pix_mask(W, H, row0, row1, per):
    m = np.zeros((H, W), bool); m[row0:row1] = True
    return np.repeat(m.reshape(-1), per)


class Dev:
    """a case on the device: its inputs, the per-step planes made on the host ((cos, sin) rounded to float32, the flags byte, M^-1), and what keeps inputs honest"""

    def __init__(self, torch, L, name):
        self.torch, self.L, self.name = torch, L, name
        self.c, self.R = c, R = iw.case(name), iw.ref(name)
        self.W, self.H, self.N = c.W, c.H, c.W * c.H
        self.wf, self.wr = F32(c.w_fit), F32(c.w_reg)
        tail = lambda a: np.concatenate([np.ascontiguousarray(a, F32).reshape(-1), np.full(TAIL, sk.CANARY, np.uint32).view(F32)])
        self.off, self.ang, self.ur, self.cons, self.mask = (sk.dbuf(torch, tail(a)) for a in (c.offset, c.angle, c.urshape, c.cons, c.mask))
        self.cs32 = R.cs.astype(F32)                                         # the host's (cos, sin), rounded: an INPUT of the step kernels
        self.cs = sk.dbuf(torch, tail(self.cs32))
        self.flags_h = R.flags()
        self.flags = byte_buf(torch, self.N, self.flags_h)
        s = R.system()
        rng = np.random.default_rng(77)
        self.pre32 = (np.where(R.excluded(), 0, sk.exact_pre(rng, 3 * self.N)) if c.exact else s.pre).astype(F32)
        self.pre = in3(torch, self.pre32, self.N)
        self.irr0, self.irrn = word(torch, 0), word(torch, max(R.irregular(), 1))
        self.consts = [(t, host(t).copy()) for t in (self.off, self.ang, self.ur, self.cons, self.mask, self.cs, self.flags, self.pre, self.irr0, self.irrn)]
        self.st_general = R.stencil(cs=self.cs32)
        self.st_grid = R.stencil(cs=self.cs32, grid=True) if c.grid else None
        mo, ma = iw.pre_from_flags(self.flags_h, c.w_fit, c.w_reg)
        self.M_flags = iw.flat_pre(mo, ma)
        mo, ma = iw.pre_from_flags_f32(self.flags_h, c.w_fit, c.w_reg)
        self.M_flags32 = iw.flat_pre(mo, ma).astype(np.float64)

    def geo(self, row0, row1):
        return (self.W, self.H, row0, row1)

    def keep(self, *ts):
        """further inputs of one launch: returns a check that they, and the case's own, are unchanged"""
        extra = [(t, host(t).copy()) for t in ts]

        def check():
            self.torch.cuda.synchronize()
            for t, h in self.consts + extra:
                assert sk.same_bytes(host(t), h), "an input changed"
        return check

    def path(self, grid):
        """(irregular word, stencil, M^-1 in float64, K_M, M^-1 for the exact regime) of the unit-grid path (M^-1 from the flags byte) or the general one (UrShape and pre read)"""
        if grid:
            return self.irr0, self.st_grid, self.M_flags, K_M, self.M_flags32
        return (None if self.c.grid else self.irrn), self.st_general, self.pre32.astype(np.float64), 0, self.pre32.astype(np.float64)


@functools.lru_cache(maxsize=None)
def dev(torch, L, name):
    return Dev(torch, L, name)


def all_angles():
    """every angle this file hands a kernel"""
    return np.concatenate([iw.case(n).angle.ravel() for n in ALL])


def cases_rows(names):
    return [pytest.param(n, r, id=f"{n}-{r[0]}-{r[1]}") for n in names for r in iw.row_ranges(n)]


def ptr(t):
    return None if t is None else t.data_ptr()


def check_partials(key, got, terms_px, blk, per_visit, exact, eps=sk.EPS, extra=0.0):
    """one partial per workgroup against the float64 sum of its pixels' terms (terms_px: [H, W] per-pixel sums; the magnitude is the sum of their absolute values
    passed as terms_px[1]); per_visit: pixels a thread adds up.  exact: the sums must be equal."""
    val, mag = terms_px
    own = blk >= 0
    grid = len(got)
    want = np.bincount(blk[own], weights=val[own], minlength=grid)
    scale = np.bincount(blk[own], weights=mag[own], minlength=grid)
    if exact:
        assert np.array_equal(np.asarray(got, np.float64), want), (key, np.flatnonzero(np.asarray(got, np.float64) != want)[:8])
        RATIOS.setdefault(key + " (exact sums)", 0.0)
    else:
        _note(key, np.abs(np.asarray(got, np.float64) - want), (3 + per_visit + 6 + WAVES) * eps * scale + extra)


# ------------------------------------------------------------------ the block mirror, UrShape
def test_the_iter_block_mirror_has_the_library_s_size(L):
    assert L.thallo_hip_iw_iter_size() == C.sizeof(sk.IwIterT)


@pytest.mark.parametrize("name", ALL)
def test_urshape_irregular_counts_pixels(torch, L, name):
    """*count_out = the NUMBER of pixels off the unit grid, as the header says (the kernel used to add one per wave with such a pixel)"""
    d = dev(torch, L, name)
    out = sk.dbuf(torch, np.full(16, 0x5A5A5A5A, np.int32))
    check = d.keep()
    assert L.thallo_hip_iw_urshape_irregular(d.W, d.H, d.ur.data_ptr(), out.data_ptr(), None) == 0
    check()
    h = host(out)
    assert h[0] == d.R.irregular() and (h[1:] == 0x5A5A5A5A).all()
    assert (h[0] == 0) == d.c.grid
    RATIOS.setdefault("urshape_irregular count (exact)", 0.0)


# ------------------------------------------------------------------ cost
@pytest.mark.parametrize("name,rows", cases_rows(ALL))
def test_cost(torch, L, name, rows):
    d = dev(torch, L, name)
    row0, row1 = rows
    out = sk.canary_buf(torch, PSLOTS)
    check = d.keep()
    rc = L.thallo_hip_iw_cost(*d.geo(row0, row1), d.off.data_ptr(), d.ang.data_ptr(), d.ur.data_ptr(), d.cons.data_ptr(), d.mask.data_ptr(), d.wf, d.wr, out.data_ptr(), None)
    check()
    ntiles = ((d.W + 63) // 64) * ((row1 - row0 + 3) // 4)
    assert rc == min(ntiles, rc) and rc > 0
    got = slots(out, rc)
    blk, per = iw.tile_blocks(d.W, d.H, row0, row1, rc, 64, 4)
    cost, mag = d.R.cost_pixels()
    if d.c.exact:
        sk.assert_exact_sums(cost[row0:row1].ravel(), rc, 2.0 ** -3, blk[row0:row1].ravel())
        check_partials("cost partials", got, (cost, mag), blk, per, True)
    else:
        own = blk >= 0
        scale = np.bincount(blk[own], weights=mag[own], minlength=rc)
        _note("cost partials", np.abs(got.astype(np.float64) - np.bincount(blk[own], weights=cost[own], minlength=rc)), sk.tol(K_COST + per + 6 + 4, scale))
    _note("cost total", abs(got.astype(np.float64).sum() - cost[row0:row1].sum()), sk.tol(K_COST + per + 10, mag[row0:row1].sum()))


# ------------------------------------------------------------------ PCGInit1
def launch_init(d, row0, row1, with_delta, with_diag, irregular=True):
    t, N = d.torch, d.N
    o = SimpleNamespace(**{k: out3(t, N) for k in ("r", "pre", "z", "p_prev", "delta", "diag")})
    o.cs, o.flags, o.irr, o.aN = sk.canary_buf(t, 2 * N + TAIL), byte_buf(t, N), sk.dbuf(t, np.full(16, 0x5A5A5A5A, np.int32)), sk.canary_buf(t, PSLOTS)
    o.rc = d.L.thallo_hip_iw_pcg_init(*d.geo(row0, row1), d.off.data_ptr(), d.ang.data_ptr(), d.ur.data_ptr(), d.cons.data_ptr(), d.mask.data_ptr(), d.wf, d.wr,
                                      o.r.data_ptr(), o.pre.data_ptr(), o.z.data_ptr(), o.p_prev.data_ptr(), o.delta.data_ptr() if with_delta else None,
                                      o.cs.data_ptr(), o.flags.data_ptr(), o.diag.data_ptr() if with_diag else None, o.irr.data_ptr() if irregular else None, o.aN.data_ptr(), None)
    t.cuda.synchronize()
    return o


@pytest.mark.parametrize("name,rows", cases_rows(ALL))
def test_pcg_init(torch, L, name, rows):
    d = dev(torch, L, name)
    R, W, H, N = d.R, d.W, d.H, d.N
    row0, row1 = rows
    check = d.keep()
    a = launch_init(d, row0, row1, True, True)
    b = launch_init(d, row0, row1, False, False, irregular=False)
    check()
    ntiles = ((W + 63) // 64) * ((row1 - row0 + 15) // 16)
    assert a.rc == b.rc == ntiles
    own = iw.rows_mask(W, H, row0, row1)
    everywhere = np.ones(3 * N, bool)
    s = R.system()
    h = {k: host(getattr(a, k)) for k in ("r", "pre", "z", "p_prev", "delta", "diag")}
    for k in ("r", "pre", "z", "delta", "diag"):
        canary_elsewhere(h[k], own, k)
    canary_elsewhere(h["p_prev"], everywhere, "p_prev")            # owned rows and ghost rows: p_prev = 0
    canary_elsewhere(host(b.delta), np.zeros(0, bool), "delta (NULL)"); canary_elsewhere(host(b.diag), np.zeros(0, bool), "diag_out (NULL)")
    for k in ("r", "pre", "z", "p_prev"):                            # the same bits with and without delta / diag_out / irregular_out
        assert sk.same_bytes(h[k], host(getattr(b, k))), k
    assert sk.same_bytes(host(a.cs), host(b.cs)) and sk.same_bytes(host(a.flags), host(b.flags)) and sk.same_bytes(host(a.aN), host(b.aN))
    assert (h["p_prev"][:3 * N] == 0).all() and (h["delta"][:3 * N][own] == 0).all()
    # cs on every row of the local image, held to the measured sincosf figure; flags: the exact bytes (a ghost row: bit 0 only)
    csh = host(a.cs)
    canary_elsewhere(csh, np.ones(2 * N, bool), "cs")
    got_cs = csh[:2 * N].reshape(H, W, 2).astype(np.float64)
    with np.errstate(all="ignore"):
        rel = np.abs(got_cs - R.cs) / (sk.EPS * np.abs(R.cs))
    RATIOS["sincosf: worst relative error in units of 2^-24"] = max(RATIOS.get("sincosf: worst relative error in units of 2^-24", 0.0), float(np.nanmax(rel)))
    _note("pcg_init cs", np.abs(got_cs - R.cs), sk.tol(TRIG, np.abs(R.cs)))
    fh = host(a.flags)
    assert (fh[(N + 3) // 4 * 4:] == 0xA5).all(), "flags: the tail"
    assert np.array_equal(fh[:N].reshape(H, W), R.flags(row0, row1)), np.argwhere(fh[:N].reshape(H, W) != R.flags(row0, row1))[:8]
    # the irregular word: the number of owned pixels off the grid
    ih = host(a.irr)
    assert ih[0] == R.irregular(row0, row1) and (ih[1:] == 0x5A5A5A5A).all(), (ih[0], R.irregular(row0, row1))
    RATIOS.setdefault("pcg_init irregular_out count (exact)", 0.0)
    # r, diag, pre, z
    g = {k: h[k][:3 * N].astype(np.float64) for k in h}
    if d.c.exact:
        _bits("pcg_init r", h["r"][:3 * N][own], s.r[own])
        _bits("pcg_init diag_out", h["diag"][:3 * N][own], s.diag[own])
    _note("pcg_init r", np.abs(g["r"] - s.r)[own], sk.tol(K_R, s.r_abs)[own])
    _note("pcg_init diag_out", np.abs(g["diag"] - s.diag)[own], sk.tol(K_D, s.diag)[own])
    _note("pcg_init pre", np.abs(g["pre"] - s.pre)[own], sk.tol(K_PRE, s.pre)[own])
    _note("pcg_init z", np.abs(g["z"] - s.z)[own], sk.tol(K_Z, s.z_abs)[own])
    assert np.array_equal(h["z"][:3 * N][own], (h["pre"][:3 * N] * h["r"][:3 * N])[own]), "z == pre * r in float32"
    assert (g["pre"][own & R.excluded()] == 0).all()
    if d.c.grid:                                                     # the flags byte reproduces pre (pre_from_flags): what the z-free schedule relies on
        _note("pcg_init pre against the flags byte", np.abs(g["pre"] - d.M_flags)[own], sk.tol(K_M, d.M_flags)[own])
    # alphaN partials against the device's own r, z
    got = slots(a.aN, a.rc)
    blk, per = iw.tile_blocks(W, H, row0, row1, a.rc)
    terms = g["r"] * g["z"]
    check_partials("pcg_init alphaN partials", got, (iw.per_pixel(terms, W, H), iw.per_pixel(np.abs(terms), W, H)), blk, 4 * per, False)


# ------------------------------------------------------------------ applyJTJ, fused PCGStep1
def bounds_step(o, st, k_z, E_z=0.0, E_pin=0.0, beta=0.0):
    """absolute error arrays of p and A p: p = z + beta p_in with k_z roundings into z (on z's share of S_p) + 2; A p: K_AP + |J^T J| E_p"""
    E_p = sk.tol(k_z + 2, o.p_abs) + E_z + abs(float(beta)) * E_pin
    return E_p, sk.tol(K_AP, o.Ap_abs) + st.apply(E_p)[1]


@pytest.mark.parametrize("name,rows", cases_rows(ALL))
def test_apply_jtj(torch, L, name, rows):
    d = dev(torch, L, name)
    W, H, N = d.W, d.H, d.N
    row0, row1 = rows
    own = iw.rows_mask(W, H, row0, row1)
    P = iw.planes(name, 21)
    p = in3(torch, P.p, N)
    for grid in ([False, True] if d.c.grid else [False]):
        irr, st, _, _, _ = d.path(grid)
        key = "apply_jtj " + ("unit grid" if grid else "general")
        Ap, aD = out3(torch, N), sk.canary_buf(torch, PSLOTS)
        check = d.keep(p)
        rc = L.thallo_hip_iw_apply_jtj(*d.geo(row0, row1), d.cs.data_ptr(), d.ur.data_ptr(), d.flags.data_ptr(), d.wf, d.wr, p.data_ptr(), Ap.data_ptr(), ptr(irr), aD.data_ptr(), None)
        check()
        assert rc == ((W + 63) // 64) * ((row1 - row0 + 15) // 16)
        h = host(Ap)
        canary_elsewhere(h, own, key)
        want, S = st.apply(P.p)
        g = h[:3 * N].astype(np.float64)
        if d.c.exact:
            _bits(key + " Ap", h[:3 * N][own], want[own])
        _note(key + " Ap", np.abs(g - want)[own], sk.tol(K_AP, S)[own])
        blk, per = iw.tile_blocks(W, H, row0, row1, rc)
        terms = P.p.astype(np.float64) * g
        if d.c.exact:
            sk.assert_exact_sums(terms[own], rc, 2.0 ** -6, block3(blk, own))
        check_partials(key + " alphaD partials", slots(aD, rc), (iw.per_pixel(terms, W, H), iw.per_pixel(np.abs(terms), W, H)), blk, 4 * per, d.c.exact)


def scalars(torch, exact):
    """the five words a fused launch is handed and alpha, beta, alpha2 as it forms them"""
    aN, aD, bN, aN2, aD2 = iw.exact_scalars() if exact else iw.rounded_scalars()
    w = sk.dbuf(torch, np.array([aN, aD, bN, aN2, aD2] + [0] * 11, F32))
    S = lambda k: sk.api.SumT(w.data_ptr() + 4 * k, 1)
    return SimpleNamespace(buf=w, aN=S(0), aD=S(1), bN=S(2), aN2=S(3), aD2=S(4), aN_v=aN,
                           alpha=sk.div32(aN, aD, True), beta=sk.div32(bN, aN, True), alpha2=sk.div32(aN2, aD2, True))


@pytest.mark.parametrize("name,rows", cases_rows(ALL))
def test_pcg_step1(torch, L, name, rows):
    """modes 1, 0, 2, 4; the z-free path (r given, *irregular == 0: p = M^-1 r + beta p with M^-1 from the flags byte) and the general one (z read).  Where 2 W H is no
    multiple of 4 the launcher drops to the general path although r and a zero word are given: z and r are different planes here, so the test sees which was read."""
    d = dev(torch, L, name)
    W, H, N = d.W, d.H, d.N
    row0, row1 = rows
    own = iw.rows_mask(W, H, row0, row1)
    P = iw.planes(name, 22)
    sc = scalars(torch, d.c.exact)
    z, r, p_in = in3(torch, P.z, N), in3(torch, P.r, N), in3(torch, P.p, N)
    for zfree in ([False, True] if d.c.grid else [False]):
        irr, st, M, k_m, M32 = d.path(zfree)
        really_zfree = zfree and (2 * W * H) % 4 == 0
        if zfree and not really_zfree:
            st = d.st_general                                          # the launcher's drop: UrShape and z are read
        for mode in MODES:
            key = f"pcg_step1 {'z-free' if really_zfree else 'dropped to general' if zfree else 'general'} mode {mode}"
            p_out, delta, Ap, aD = in3(torch, P.p_old, N), in3(torch, P.delta, N), out3(torch, N), sk.canary_buf(torch, PSLOTS)
            check = d.keep(z, r, p_in, sc.buf)
            rc = L.thallo_hip_iw_pcg_step1(*d.geo(row0, row1), d.cs.data_ptr(), d.ur.data_ptr(), d.flags.data_ptr(), d.wf, d.wr, z.data_ptr(), p_in.data_ptr(), p_out.data_ptr(),
                                           delta.data_ptr(), Ap.data_ptr(), mode, sc.aN, sc.aD, sc.bN, sc.aN2, sc.aD2, ptr(irr), r.data_ptr() if zfree else None, aD.data_ptr(), None)
            check()
            assert rc == ((W + 63) // 64) * ((row1 - row0 + 15) // 16)
            if really_zfree:
                zz, za, k_z, zz32 = M * P.r, M * np.abs(P.r), k_m + 1, M32 * P.r
            else:
                zz, za, k_z, zz32 = P.z.astype(np.float64), np.abs(P.z), 0, P.z.astype(np.float64)
            o = iw.step1(st, zz, za, P.p, P.delta, P.p_old, mode, sc.alpha, sc.beta, sc.alpha2)
            E_p, E_Ap = bounds_step(o, st, k_z)
            hp, hd, hA = host(p_out), host(delta), host(Ap)
            canary_elsewhere(hA, own, key + " Ap")
            assert sk.same_bytes(hp[3 * N:], host(p_in)[3 * N:]) and sk.same_bytes(hd[3 * N:], host(p_in)[3 * N:]), "the tails of p_out / delta"
            gp, gd, gA = (x[:3 * N].astype(np.float64) for x in (hp, hd, hA))
            _note(key + " p_out (ghost rows too)", np.abs(gp - o.p), E_p)                    # every row of the local image: p is kept current on ghost rows
            dm = iw.dmode_of(mode)
            _note(key + " delta", np.abs(gd - o.delta)[own], sk.tol(DELTA_K[dm], o.delta_abs)[own])
            assert sk.same_bytes(hd[:3 * N][~own], P.delta[~own]), "delta outside the owned rows"
            if dm == 1:
                assert sk.same_bytes(hd[:3 * N], P.delta), "delta is not this launch's"
            _note(key + " Ap", np.abs(gA - o.Ap)[own], E_Ap[own])
            if d.c.exact:
                e = iw.step1(st, zz32, za, P.p, P.delta, P.p_old, mode, sc.alpha, sc.beta, sc.alpha2)
                b = 0.0 if mode & 1 else float(sc.beta)
                _bits_either(key + " p_out", hp[:3 * N], e.p.astype(F32), (zz32.astype(F32).astype(np.float64) + b * P.p).astype(F32))
                _bits(key + " delta", hd[:3 * N][own], e.delta[own])
                if not really_zfree:
                    _bits(key + " Ap", hA[:3 * N][own], e.Ap[own])
            blk, per = iw.tile_blocks(W, H, row0, row1, rc)
            terms = gp * gA
            exact = d.c.exact and not really_zfree
            if exact:
                sk.assert_exact_sums(terms[own], rc, 2.0 ** -8, block3(blk, own))
            check_partials(key + " alphaD partials", slots(aD, rc), (iw.per_pixel(np.where(own, terms, 0), W, H), iw.per_pixel(np.where(own, np.abs(terms), 0), W, H)), blk, 4 * per, exact)


# ------------------------------------------------------------------ PCGStep2
@pytest.mark.parametrize("name,rows", cases_rows(ALL))
def test_pcg_step2(torch, L, name, rows):
    """r -= alpha A p on the owned rows; the k_step2_iw branch with a zero word: M^-1 from the flags byte, z untouched; with no word or a nonzero one: pre read, z
    written; the generic kernels where a range is not 16-byte granular: pre read, z written, whatever the word says."""
    d = dev(torch, L, name)
    W, H, N = d.W, d.H, d.N
    row0, row1 = rows
    own = iw.rows_mask(W, H, row0, row1)
    P = iw.planes(name, 23)
    sc = scalars(torch, d.c.exact)
    Ap = in3(torch, P.Ap, N)
    granular = not ((2 * W * row0) | (2 * W * (row1 - row0)) | (2 * N + W * row0) | (W * (row1 - row0)) | (2 * N)) & 3
    for zero_word in ([False, True] if d.c.grid else [False]):
        irr, _, M, k_m, M32 = d.path(zero_word)
        zfree = zero_word and granular
        if zero_word and not zfree:
            M, k_m, M32 = d.pre32.astype(np.float64), 0, d.pre32.astype(np.float64)
        whole = rows == (0, H)
        key = f"pcg_step2 {'k_step2_iw' if granular else 'generic, whole image' if whole else 'element by element'} {'z-free' if zfree else 'pre read'}"
        r, z, bN = in3(torch, P.r, N), out3(torch, N), sk.canary_buf(torch, PSLOTS)
        check = d.keep(Ap, sc.buf)
        rc = L.thallo_hip_iw_pcg_step2(*d.geo(row0, row1), d.flags.data_ptr(), d.wf, d.wr, r.data_ptr(), Ap.data_ptr(), d.pre.data_ptr(), z.data_ptr(), sc.aN, sc.aD, ptr(irr), bN.data_ptr(), None)
        check()
        assert rc > 0
        r1, zz, terms = sk.ref_step2(P.r, P.Ap, M, sc.alpha)
        S_r = np.abs(P.r) + np.abs(float(sc.alpha) * P.Ap)
        hr, hz = host(r), host(z)
        assert sk.same_bytes(hr[:3 * N][~own], P.r[~own]) and sk.same_bytes(hr[3 * N:], host(Ap)[3 * N:]), "r outside the owned rows"
        gr = hr[:3 * N].astype(np.float64)
        _note(key + " r", np.abs(gr - r1)[own], sk.tol(2, S_r)[own])
        if d.c.exact:
            _bits(key + " r", hr[:3 * N][own], r1[own])
        if zfree:
            canary_elsewhere(hz, np.zeros(0, bool), key + " z")
        else:
            zmask = np.zeros(sk.ceil4(3 * N), bool); zmask[:3 * N] = own; zmask[3 * N:] = whole and not granular        # (the padded whole vector: its zeros too)
            canary_elsewhere(hz, zmask, key + " z")
            _note(key + " z", np.abs(hz[:3 * N] - zz)[own], sk.tol(3, M * S_r)[own])
            if d.c.exact:
                _bits(key + " z", hz[:3 * N][own], (M32 * r1)[own])
        got = slots(bN, rc).astype(np.float64)
        dev_terms = M * gr * gr
        _note(key + " betaN total", abs(got.sum() - dev_terms[own].sum()), sk.tol(k_m + 3 + 4 * (3 * N // (256 * rc * 4) + 1) + 6 + 4 + 1, np.abs(dev_terms[own]).sum()))


# ------------------------------------------------------------------ the one-kernel iteration
def march_owner(L, W, H, row0, row1, grid):
    R = L.thallo_hip_iw_march_rows(W, row1 - row0)
    place = np.zeros(12 * grid, np.int32)
    assert L.thallo_hip_iw_march_place(W, row0, row1, R, grid, place.ctypes.data) == 0
    blk = iw.march_blocks(W, H, place, grid)
    assert (blk[row0:row1] >= 0).all() and (blk[:row0] < 0).all() and (blk[row1:] < 0).all()
    return blk, 2 * R


def prev_partials(torch, exact, count=70):
    """iteration k-1's raw partials for the deferred finish: `count` workgroups' alphaD (float) and {N, S1, S2} (double); exact: alphaD = 4, N = 1, S1 = 1, S2 = 2,
    so that alpha = 1/2 and betaN = 1 - 1 + 1/2 = 1/2, beta = 1/4 with alphaN = 2"""
    rng = np.random.default_rng(9)
    if exact:
        aD = sk.exact_sum(rng, count, 4.0)
        s12 = np.stack([sk.exact_sum(rng, count, v).astype(np.float64) for v in (1.0, 1.0, 2.0)], 1)
    else:
        aD = np.abs(sk.rounded_vec(rng, count)) + F32(0.01)
        s12 = np.abs(rng.standard_normal((count, 3)))
        s12[:, 1] *= 0.3
    return aD.astype(F32), np.ascontiguousarray(s12)


def finish_words(aD_part, s12_part, alphaN):
    """what a finish leaves: alphaD (bit-exact) and betaN with its float64 value and magnitude"""
    s12 = np.asarray(s12_part, np.float64).reshape(-1, 3)
    ad = sk.sum_partials(aD_part)
    alpha = sk.div32(alphaN, ad, True)
    bn, mag = sk.beta_n_f64(sk.sum_partials_f64(s12[:, 0]), sk.sum_partials_f64(s12[:, 1]), sk.sum_partials_f64(s12[:, 2]), alpha)
    return ad, alpha, bn, mag


def check_words(key, aD_word, bN_word, aD_part, s12_part, alphaN):
    ad, alpha, bn, mag = finish_words(aD_part, s12_part, alphaN)
    assert np.array(aD_word, F32).view(np.uint32) == np.array(ad, F32).view(np.uint32), (key, aD_word, ad)
    _note(key + " betaN word", abs(float(bN_word) - bn), sk.EPS * abs(bn) + 8 * EPS64 * mag)
    return alpha, F32(bN_word)


def run_iter(d, kernel, row0, row1, mode, finish, grid, P, sc, with_Ap=True):
    """one launch of thallo_hip_iw_pcg_iter and its reference; returns nothing, asserts everything"""
    torch, L, W, H, N = d.torch, d.L, d.W, d.H, d.N
    own = iw.rows_mask(W, H, row0, row1)
    irr, st, M, k_m, M32 = d.path(grid)
    kname = ("tile", "march", "march_rc")[kernel]
    key = f"pcg_iter {kname} {'unit grid' if grid else 'general'} mode {mode}"
    r_in, Ap_in, p_in = in3(torch, P.r, N), in3(torch, P.Ap, N), in3(torch, P.p, N)
    r_out, Ap_out, p_out, delta = out3(torch, N), out3(torch, N), in3(torch, P.p_old, N), in3(torch, P.delta, N)
    aD, s12 = sk.canary_buf(torch, PSLOTS), sk.canary_buf(torch, 3 * PSLOTS, np.float64)
    words = sk.canary_buf(torch, 16)
    tickets = sk.dbuf(torch, np.zeros(sk.FIN_TICKET_WORDS + 16, np.uint32))
    a = sk.IwIterT()
    a.W, a.H, a.row0, a.row1 = W, H, row0, row1
    a.cs, a.urshape, a.flags, a.pre, a.irregular = d.cs.data_ptr(), d.ur.data_ptr(), d.flags.data_ptr(), d.pre.data_ptr(), ptr(irr)
    a.w_fit, a.w_reg = d.wf, d.wr
    a.r_in, a.r_out, a.p_in, a.p_out, a.delta, a.mode = r_in.data_ptr(), r_out.data_ptr(), p_in.data_ptr(), p_out.data_ptr(), delta.data_ptr(), mode
    if with_Ap:
        a.Ap_in, a.Ap_out = Ap_in.data_ptr(), Ap_out.data_ptr()
    a.alphaN_prev, a.alphaD_prev, a.betaN_prev, a.alphaN_prev2, a.alphaD_prev2 = sc.aN, sc.aD, sc.bN, sc.aN2, sc.aD2
    a.alphaD_out, a.s12_out = aD.data_ptr(), s12.data_ptr()
    alpha, beta = sc.alpha, sc.beta
    extra = [sc.buf]
    prev = None
    if finish == "tickets":
        a.fin_tickets, a.alphaD_word, a.betaN_word = tickets.data_ptr(), words.data_ptr(), words.data_ptr() + 4
    if finish == "prev" and not mode & 1:
        pa, ps = prev_partials(torch, d.c.exact)
        pad, ps12, pw = sk.dbuf(torch, pa), sk.dbuf(torch, ps), sk.canary_buf(torch, 16)
        prev = sk.api.PrevT(pad.data_ptr(), ps12.data_ptr(), len(pa), pw.data_ptr() + 8, pw.data_ptr() + 12)
        a.prev = C.pointer(prev)
        extra += [pad, ps12]
        ad, alpha, bn, mag = finish_words(pa, ps, sc.aN_v)
        beta = sk.div32(F32(bn), sc.aN_v, True)
    check = d.keep(r_in, Ap_in, p_in, *extra)
    rc = L.thallo_hip_iw_pcg_iter(kernel, C.byref(a), None)
    check()
    assert rc > 0, rc
    if prev is not None:                                  # the words of iteration k-1 the launch leaves behind, and nothing beside them
        pwh = host(pw)
        _, bword = check_words(key + " deferred", pwh[2], pwh[3], pa, ps, sc.aN_v)
        assert (pwh.view(np.uint32)[[0, 1] + list(range(4, 16))] == sk.CANARY).all()
        beta = sk.div32(bword, sc.aN_v, True)             # (beta from the word the device itself rounded: the reference's betaN may differ in the last place)
    rc_form, whole = kernel == sk.IW_ITER_MARCH_RC, (row0, row1) == (0, H)
    Ap_eff, E_Apin = P.Ap, 0.0
    if rc_form:                                           # A p_{k-1} recomputed from p_in on the owned rows, read from Ap_in on a slab's ghost rows
        Ar, Sa = st.apply(P.p)
        Ap_eff, E_Apin = np.where(own, Ar, P.Ap), np.where(own, sk.tol(K_AP, Sa), 0.0)
    o = iw.iteration(st, M, P.r, Ap_eff, P.p, P.delta, P.p_old, mode, alpha, beta, sc.alpha2)
    E_r = (0.0 if mode & 1 else sk.tol(2, o.r_abs)) + abs(float(alpha)) * E_Apin
    E_p, E_Ap = bounds_step(o, st, k_m + 1, E_z=M * E_r)
    hr, hA, hp, hd = host(r_out), host(Ap_out), host(p_out), host(delta)
    gr, gp, gd = (x[:3 * N].astype(np.float64) for x in (hr, hp, hd))
    canary_elsewhere(hr, np.ones(3 * N, bool), key + " r_out")
    assert sk.same_bytes(hp[3 * N:], host(p_in)[3 * N:]) and sk.same_bytes(hd[3 * N:], host(p_in)[3 * N:]), "the tails of p_out / delta"
    _note(key + " r_out (ghost rows too)", np.abs(gr - o.r), E_r)
    _note(key + " p_out (ghost rows too)", np.abs(gp - o.p), E_p)
    dm = iw.dmode_of(mode)
    _note(key + " delta", np.abs(gd - o.delta)[own], sk.tol(DELTA_K[dm], o.delta_abs)[own])
    assert sk.same_bytes(hd[:3 * N][~own], P.delta[~own]), "delta outside the owned rows"
    if not rc_form:
        canary_elsewhere(hA, own, key + " Ap_out")
        gA = hA[:3 * N].astype(np.float64)
        _note(key + " Ap_out", np.abs(gA - o.Ap)[own], E_Ap[own])
        E_dev = 0.0
    else:                                                 # a whole image: A p is not stored; a slab: its first and last owned row only (what the exchange carries)
        edge = np.zeros(3 * N, bool) if whole else iw.rows_mask(W, H, row0, row0 + 1) | iw.rows_mask(W, H, row1 - 1, row1)
        canary_elsewhere(hA, edge, key + " Ap_out")
        _note(key + " Ap_out (a slab's edge rows)", np.abs(hA[:3 * N].astype(np.float64) - o.Ap)[edge], E_Ap[edge])
        gA, S_dev = st.apply(gp)                          # J^T J of the DEVICE's p_out, which the kernel adds up without storing it
        E_dev = sk.tol(K_AP, S_dev)
    exact_planes = d.c.exact
    if exact_planes:
        e = iw.iteration(st, M32, P.r, Ap_eff, P.p, P.delta, P.p_old, mode, alpha, beta, sc.alpha2)
        b = 0.0 if mode & 1 else float(beta)
        _bits(key + " r_out", hr[:3 * N], e.r); _bits(key + " delta", hd[:3 * N][own], e.delta[own])
        _bits_either(key + " p_out", hp[:3 * N], e.p.astype(F32), ((M32 * e.r).astype(F32).astype(np.float64) + b * P.p).astype(F32))
        if not grid and not rc_form:
            _bits(key + " Ap_out", hA[:3 * N][own], e.Ap[own])
    # the partials: alphaD (float) and {N, S1, S2} (double) per workgroup against the device's own planes
    if kernel == sk.IW_ITER_TILE:
        assert rc == ((W + 63) // 64) * ((row1 - row0 + 15) // 16)
        blk, per = iw.tile_blocks(W, H, row0, row1, rc)
        per *= 4
    else:
        blk, per = march_owner(L, W, H, row0, row1, rc)
    fkey = f"{key} finish {finish}"
    gaD, gs = slots(aD, rc), slots(s12, rc, 3)
    tA, tN, t1, t2 = (np.where(own, t, 0) for t in iw.sums_terms(M, gr, gA, gp))
    px = lambda t: (iw.per_pixel(t, W, H), iw.per_pixel(np.abs(t), W, H))
    exact_sums = exact_planes and not grid and not rc_form
    ownpx = blk >= 0
    e_px = lambda w: np.bincount(blk[ownpx], weights=iw.per_pixel(np.where(own, w, 0), W, H)[ownpx], minlength=rc) if np.ndim(w) else 0.0
    if exact_sums:
        sk.assert_exact_sums(tA[own], rc, 2.0 ** -8, block3(blk, own))
    check_partials(key + " alphaD partials", gaD, px(tA), blk, per, exact_sums, extra=e_px(np.abs(gp) * E_dev))
    for j, (t, nm, ex) in enumerate(((tN, "N", 0.0), (t1, "S1", M * np.abs(gr) * E_dev), (t2, "S2", M * (2 * np.abs(gA) + E_dev) * E_dev))):
        val, mag = px(t)
        want = np.bincount(blk[ownpx], weights=val[ownpx], minlength=rc); scale = np.bincount(blk[ownpx], weights=mag[ownpx], minlength=rc)
        _note(f"{key} {nm} partials", np.abs(gs[:, j] - want), (5 + per + 6 + WAVES) * EPS64 * scale + sk.tol(k_m, scale) + e_px(ex))
    # the finish
    th = host(tickets)
    assert (th == 0).all(), "the tickets are zero again"
    wh = host(words)
    if finish == "tickets":
        check_words(fkey, wh[0], wh[1], gaD, gs, sc.bN.partials and host(sc.buf)[2])
        assert (wh.view(np.uint32)[2:] == sk.CANARY).all()
    else:
        assert (wh.view(np.uint32) == sk.CANARY).all(), "no word without tickets"
        assert L.thallo_hip_iw_pcg_iter_finish(aD.data_ptr(), s12.data_ptr(), rc, sc.bN, words.data_ptr() + 8, words.data_ptr() + 12, None) == 0
        torch.cuda.synchronize()
        wh = host(words)
        check_words(fkey + " (pcg_iter_finish)", wh[2], wh[3], gaD, gs, host(sc.buf)[2])
        assert (wh.view(np.uint32)[[0, 1] + list(range(4, 16))] == sk.CANARY).all()


FINISHES = ("partials", "tickets", "prev")


def forms(rows_index, whole):
    """(mode, finish): on a whole image every mode with every finish; on a row range every mode with one finish, taking turns"""
    if whole:
        return [(m, f) for m in MODES for f in FINISHES]
    return [(m, FINISHES[(i + rows_index) % 3]) for i, m in enumerate(MODES)]


@pytest.mark.parametrize("name,rows", cases_rows(ALL))
def test_pcg_iter_tile(torch, L, name, rows):
    d = dev(torch, L, name)
    P, sc = iw.planes(name, 31), scalars(torch, d.c.exact)
    for grid in ([False, True] if d.c.grid else [False]):
        for mode, finish in forms(iw.row_ranges(name).index(rows), rows == (0, d.H)):
            run_iter(d, sk.IW_ITER_TILE, rows[0], rows[1], mode, finish, grid, P, sc)


@pytest.mark.parametrize("forced", [0, 1, 2, 5])
@pytest.mark.parametrize("name,rows", cases_rows(MARCHABLE))
def test_pcg_iter_march(torch, L, name, rows, forced):
    """the stored-plane marching kernel at the automatic rows per segment and at forced ones (1: every segment a single row; 2, 5: full and short segments)"""
    d = dev(torch, L, name)
    P, sc = iw.planes(name, 32), scalars(torch, d.c.exact)
    L.thallo_hip_march_debug_set(0, forced)
    todo = forms(iw.row_ranges(name).index(rows), rows == (0, d.H)) if forced == 0 else [(1, "partials"), (0, "tickets"), (4, "prev")]
    for mode, finish in todo:
        run_iter(d, sk.IW_ITER_MARCH, rows[0], rows[1], mode, finish, True, P, sc)


@pytest.mark.parametrize("forced", [0, 1, 2, 5])
@pytest.mark.parametrize("name,rows", cases_rows(MARCHABLE))
def test_pcg_iter_march_rc(torch, L, name, rows, forced):
    """the recomputing marching kernel (never a GN step's first iteration); on whole images also without the A p planes"""
    d = dev(torch, L, name)
    P, sc = iw.planes(name, 33), scalars(torch, d.c.exact)
    L.thallo_hip_march_debug_set(0, forced)
    whole = rows == (0, d.H)
    todo = [mf for mf in forms(iw.row_ranges(name).index(rows), whole) if not mf[0] & 1] if forced == 0 else [(0, "tickets"), (2, "partials"), (4, "prev")]
    for mode, finish in todo:
        run_iter(d, sk.IW_ITER_MARCH_RC, rows[0], rows[1], mode, finish, True, P, sc, with_Ap=not whole)
    if whole and forced == 0:                             # ... and with the planes given: Ap_out is not touched either
        run_iter(d, sk.IW_ITER_MARCH_RC, rows[0], rows[1], todo[0][0], todo[0][1], True, P, sc, with_Ap=True)


def test_pcg_iter_refusals(torch, L):
    """every refusal the header states, as that return code, before anything is launched"""
    d = dev(torch, L, "m126x9")
    P, sc, N = iw.planes("m126x9", 5), scalars(torch, False), d.N
    bufs = [in3(torch, P.r, N) for _ in range(7)]
    aD, s12 = sk.canary_buf(torch, PSLOTS), sk.canary_buf(torch, 3 * PSLOTS, np.float64)

    def block(**kw):
        a = sk.IwIterT()
        a.W, a.H, a.row0, a.row1 = d.W, d.H, 0, d.H
        a.cs, a.urshape, a.flags, a.pre, a.irregular, a.w_fit, a.w_reg = d.cs.data_ptr(), d.ur.data_ptr(), d.flags.data_ptr(), d.pre.data_ptr(), d.irr0.data_ptr(), d.wf, d.wr
        a.r_in, a.r_out, a.Ap_in, a.Ap_out, a.p_in, a.p_out, a.delta = (b.data_ptr() for b in bufs)
        a.alphaN_prev, a.alphaD_prev, a.betaN_prev, a.alphaN_prev2, a.alphaD_prev2 = sc.aN, sc.aD, sc.bN, sc.aN2, sc.aD2
        a.alphaD_out, a.s12_out = aD.data_ptr(), s12.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    none = sk.api.SumT(None, 0)
    bad_prev = sk.api.PrevT(aD.data_ptr(), s12.data_ptr(), 0, aD.data_ptr(), aD.data_ptr())                   # count 0
    same_s12 = sk.api.PrevT(aD.data_ptr(), s12.data_ptr(), 8, aD.data_ptr(), aD.data_ptr())                    # reads the buffer it writes
    for kernel in (sk.IW_ITER_TILE, sk.IW_ITER_MARCH, sk.IW_ITER_MARCH_RC):
        for a in (block(row0=3, row1=3), block(row1=d.H + 1), block(row0=-1), block(cs=None), block(flags=None), block(r_out=None), block(p_in=None), block(alphaD_out=None),
                  block(s12_out=None), block(delta=None, mode=0), block(prev=C.pointer(bad_prev)), block(prev=C.pointer(same_s12))):
            assert L.thallo_hip_iw_pcg_iter(kernel, C.byref(a), None) == sk.INVALID
        assert L.thallo_hip_iw_pcg_iter(kernel, None, None) == sk.INVALID
    assert L.thallo_hip_iw_pcg_iter(3, C.byref(block()), None) == sk.INVALID                                # no such kernel
    for kernel in (sk.IW_ITER_TILE, sk.IW_ITER_MARCH):                                                     # the stored-plane kernels need the A p planes
        assert L.thallo_hip_iw_pcg_iter(kernel, C.byref(block(Ap_out=None)), None) == sk.INVALID
        assert L.thallo_hip_iw_pcg_iter(kernel, C.byref(block(Ap_in=None, mode=0)), None) == sk.INVALID
    odd = dev(torch, L, "t65x17")                                                                           # an odd width is a malformed block for the marching kernels
    for kernel in (sk.IW_ITER_MARCH, sk.IW_ITER_MARCH_RC):
        assert L.thallo_hip_iw_pcg_iter(kernel, C.byref(block(W=odd.W, H=odd.H, row1=odd.H, mode=1 if kernel == sk.IW_ITER_MARCH else 0)), None) == sk.INVALID
    assert L.thallo_hip_iw_pcg_iter(sk.IW_ITER_MARCH_RC, C.byref(block(mode=1)), None) == sk.INVALID        # never a GN step's first iteration
    assert L.thallo_hip_iw_pcg_iter(sk.IW_ITER_MARCH_RC, C.byref(block(alphaD_prev=none)), None) == sk.INVALID
    assert L.thallo_hip_iw_pcg_iter(sk.IW_ITER_MARCH_RC, C.byref(block(mode=4, alphaD_prev2=none)), None) == sk.INVALID
    assert L.thallo_hip_iw_pcg_iter(sk.IW_ITER_MARCH_RC, C.byref(block(row0=1, row1=d.H, Ap_in=None)), None) == sk.INVALID      # a slab exchanges rows of A p
    # a shape a kernel does not take: a vector beyond one buffer descriptor (the recomputing kernel), more strips than workgroup slots (both marching kernels)
    assert L.thallo_hip_iw_pcg_iter(sk.IW_ITER_MARCH_RC, C.byref(block(W=32768, H=16384, row1=16384)), None) == sk.NOT_SUPPORTED
    wide = 2 * 124 * 1100
    assert L.thallo_hip_iw_march_rows(wide, 1) == 0
    for kernel in (sk.IW_ITER_MARCH, sk.IW_ITER_MARCH_RC):
        assert L.thallo_hip_iw_pcg_iter(kernel, C.byref(block(W=wide, H=1, row1=1, mode=1 if kernel == sk.IW_ITER_MARCH else 0)), None) == sk.NOT_SUPPORTED
    torch.cuda.synchronize()
    assert (host(aD).view(np.uint32) == sk.CANARY).all() and all(sk.same_bytes(host(b)[:3 * N], P.r) for b in bufs), "a refused block launched something"
    RATIOS.setdefault("pcg_iter refusals (return codes, exact)", 0.0)


@pytest.mark.parametrize("kernel", [sk.IW_ITER_MARCH, sk.IW_ITER_MARCH_RC])
def test_marching_kernels_refuse_an_irregular_urshape_with_nan_scalars(torch, L, kernel):
    """handed a nonzero `irregular` word a marching kernel computes nothing: NaN in its alphaD partials and in the words of its finish, no plane written"""
    d = dev(torch, L, "m126x9")
    P, sc, N = iw.planes("m126x9", 6), scalars(torch, False), d.N
    r_in, Ap_in, p_in = in3(torch, P.r, N), in3(torch, P.Ap, N), in3(torch, P.p, N)
    r_out, Ap_out, p_out, delta = out3(torch, N), out3(torch, N), out3(torch, N), in3(torch, P.delta, N)
    aD, s12, words = sk.canary_buf(torch, PSLOTS), sk.canary_buf(torch, 3 * PSLOTS, np.float64), sk.canary_buf(torch, 16)
    tickets = sk.dbuf(torch, np.zeros(sk.FIN_TICKET_WORDS, np.uint32))
    a = sk.IwIterT()
    a.W, a.H, a.row0, a.row1 = d.W, d.H, 0, d.H
    a.cs, a.flags, a.irregular, a.w_fit, a.w_reg = d.cs.data_ptr(), d.flags.data_ptr(), d.irrn.data_ptr(), d.wf, d.wr
    a.r_in, a.r_out, a.Ap_in, a.Ap_out, a.p_in, a.p_out, a.delta, a.mode = r_in.data_ptr(), r_out.data_ptr(), Ap_in.data_ptr(), Ap_out.data_ptr(), p_in.data_ptr(), p_out.data_ptr(), delta.data_ptr(), 0
    a.alphaN_prev, a.alphaD_prev, a.betaN_prev, a.alphaN_prev2, a.alphaD_prev2 = sc.aN, sc.aD, sc.bN, sc.aN2, sc.aD2
    a.alphaD_out, a.s12_out = aD.data_ptr(), s12.data_ptr()
    a.fin_tickets, a.alphaD_word, a.betaN_word = tickets.data_ptr(), words.data_ptr(), words.data_ptr() + 4
    rc = L.thallo_hip_iw_pcg_iter(kernel, C.byref(a), None)
    torch.cuda.synchronize()
    assert rc > 0
    wh = host(words)
    assert np.isnan(wh[0]) and np.isnan(wh[1]) and wh.view(np.uint32)[0] != sk.CANARY and wh.view(np.uint32)[1] != sk.CANARY
    assert np.isnan(slots(aD, rc)).all()
    for t in (r_out, Ap_out, p_out):
        canary_elsewhere(host(t), np.zeros(0, bool), "a plane of a refused launch")
    assert sk.same_bytes(host(delta)[:3 * N], P.delta)
    RATIOS.setdefault("pcg_iter %s nonzero irregular word: NaN scalars (exact)" % ("march", "march_rc")[kernel - 1], 0.0)


# ------------------------------------------------------------------ the resident loop
@pytest.mark.parametrize("name", MARCHABLE)
def test_pcg_resident(torch, L, name):
    """L = 1 and L = 2 iterations in one launch on whole images that fit, from what pcg_init leaves (r_0, zeros in p and delta).  The reference takes the device's
    own words[] as its scalars; default bounded waits, no fault injected; the status must be clean."""
    d = dev(torch, L, name)
    W, H, N = d.W, d.H, d.N
    assert L.thallo_hip_iw_resident_rows(W, H) > 0, "every case is small enough for the chip's registers"
    P = iw.planes(name, 41)
    st, M = d.st_grid, d.M_flags
    aN0 = F32(1.7)
    aNw = word(torch, aN0, F32)
    zeros = np.zeros(3 * N, F32)
    xbuf = sk.dbuf(torch, np.zeros(L.thallo_hip_iw_resident_bytes(W, H) // 4 + 64, np.uint32))
    o0 = iw.iteration(st, M, P.r, None, zeros, zeros, zeros, 1, 0.0, 0.0)
    E_p0, E_Ap0 = bounds_step(o0, st, K_M + 1)
    first_words = None
    for Lit in (1, 2):
        r_in, p_in = in3(torch, P.r, N), in3(torch, zeros, N)
        r_out, Ap_out, p_out, delta, words = out3(torch, N), out3(torch, N), out3(torch, N), in3(torch, zeros, N), sk.canary_buf(torch, 16)
        check = d.keep(r_in, p_in, aNw)
        rc = L.thallo_hip_iw_pcg_resident(W, H, 0, H, d.cs.data_ptr(), d.flags.data_ptr(), d.wf, d.wr, r_in.data_ptr(), p_in.data_ptr(), r_out.data_ptr(), Ap_out.data_ptr(),
                                          p_out.data_ptr(), delta.data_ptr(), sk.api.SumT(aNw.data_ptr(), 1), words.data_ptr(), d.irr0.data_ptr(), None, None, xbuf.data_ptr(), Lit, None)
        assert rc > 0, rc
        assert L.thallo_hip_iw_resident_status(xbuf.data_ptr(), 0, -1, None, None) == 0, "a bounded wait ran out"
        check()
        wh = host(words)
        assert (wh.view(np.uint32)[2 * Lit:] == sk.CANARY).all()
        hr, hA, hp, hd = (host(t) for t in (r_out, Ap_out, p_out, delta))
        for h, nm in ((hr, "r_out"), (hA, "Ap_out"), (hp, "p_out")):
            canary_elsewhere(h, np.ones(3 * N, bool), nm)
        gr, gA, gp, gd = (h[:3 * N].astype(np.float64) for h in (hr, hA, hp, hd))
        key = f"pcg_resident L = {Lit}"
        if Lit == 1:
            first_words = wh[:2].copy()
            o, E_r, E_p, E_Ap = o0, 0.0, E_p0, E_Ap0
            assert (hd[:3 * N] == 0).all(), "delta without its last term"
        else:
            assert sk.same_bytes(wh[:2], first_words), "iteration 0's words do not depend on L"
            alpha, beta = sk.div32(aN0, wh[0], True), sk.div32(wh[1], aN0, True)
            o = iw.iteration(st, M, P.r, o0.Ap, o0.p, zeros, zeros, 0, alpha, beta)
            E_r = sk.tol(2, o.r_abs) + abs(float(alpha)) * E_Ap0
            E_p, E_Ap = bounds_step(o, st, K_M + 1, E_z=M * E_r, E_pin=E_p0, beta=beta)
            _note(key + " delta", np.abs(gd - o.delta), sk.tol(2, o.delta_abs) + abs(float(alpha)) * E_p0)
        _note(key + " r_out", np.abs(gr - o.r), E_r); _note(key + " p_out", np.abs(gp - o.p), E_p); _note(key + " Ap_out", np.abs(gA - o.Ap), E_Ap)
        tA, tN, t1, t2 = iw.sums_terms(M, gr, gA, gp)
        chain = 3 + 2 * H + 6 + 4 + (rc // 64 + 1) + 6
        _note(key + " alphaD word", abs(float(wh[2 * Lit - 2]) - tA.sum()), sk.tol(chain, np.abs(tA).sum()))
        alpha_k = sk.div32(F32(wh[1]) if Lit == 2 else aN0, wh[2 * Lit - 2], True)
        bn, mag = sk.beta_n_f64(tN.sum(), t1.sum(), t2.sum(), alpha_k)
        _note(key + " betaN word", abs(float(wh[2 * Lit - 1]) - bn), sk.tol(K_M + 1, mag) + 64 * EPS64 * mag)


# ------------------------------------------------------------------ laplacian_image
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("xguard", [0, 1])
@pytest.mark.parametrize("W,H", iw.LAP_CASES)
def test_lapimg(torch, L, W, H, xguard, exact):
    """the four entry points of the other image-stencil plugin: cost, pcg_init (identity preconditioner: z = r), apply_jtj, pcg_step1 (first and later)"""
    X, A, w = iw.lap_inputs(W, H, exact)
    R = iw.LapRef(W, H, X, A, w, xguard)
    N = W * H
    tail = lambda a: np.concatenate([np.ascontiguousarray(a, F32).reshape(-1), np.full(TAIL, sk.CANARY, np.uint32).view(F32)])
    dX, dA = sk.dbuf(torch, tail(X)), sk.dbuf(torch, tail(A))
    keep = [(t, host(t).copy()) for t in (dX, dA)]
    out = lambda: sk.canary_buf(torch, N + TAIL)
    ntiles = ((W + 63) // 64) * ((H + 7) // 8)
    blk, per = iw.tile_blocks(W, H, 0, H, ntiles, 64, 8)
    all_px = np.ones(N, bool)
    form = f"lapimg xguard {xguard}"

    def partials(key, buf, rc, val, mag, k):
        assert rc == ntiles
        got = slots(buf, rc).astype(np.float64)
        want, scale = np.bincount(blk.ravel(), weights=val.ravel(), minlength=rc), np.bincount(blk.ravel(), weights=mag.ravel(), minlength=rc)
        if exact:
            assert np.array_equal(got, want), key
        _note(key, np.abs(got - want), sk.tol(k + 2 * per + 6 + 4, scale))
    # cost: per pixel w (x - a) (2), squared (2 x + 1), two squared differences (3 each), two additions, the half: 8
    cost = out()
    rc = L.thallo_hip_lapimg_cost(W, H, dX.data_ptr(), dA.data_ptr(), F32(w), xguard, cost.data_ptr(), None)
    torch.cuda.synchronize()
    partials(form + " cost partials", cost, rc, *R.cost_pixels(), 8)
    # pcg_init
    r, z, pp, dl, dg, aN = out(), out(), out(), out(), out(), sk.canary_buf(torch, PSLOTS)
    rc = L.thallo_hip_lapimg_pcg_init(W, H, dX.data_ptr(), dA.data_ptr(), F32(w), xguard, r.data_ptr(), z.data_ptr(), pp.data_ptr(), dl.data_ptr(), dg.data_ptr(), aN.data_ptr(), None)
    torch.cuda.synchronize()
    want, S, diag = R.system()
    hr = host(r)
    for t, nm in ((r, "r"), (z, "z"), (pp, "p_prev"), (dl, "delta"), (dg, "diag_out")):
        canary_elsewhere(host(t), all_px, nm)
    assert sk.same_bytes(hr, host(z)) and (host(pp)[:N] == 0).all() and (host(dl)[:N] == 0).all()
    _note(form + " pcg_init r", np.abs(hr[:N] - want.ravel()), sk.tol(K_LAP, S.ravel()))
    _note(form + " pcg_init diag_out", np.abs(host(dg)[:N] - diag.ravel()), sk.tol(5, diag.ravel()))
    g = hr[:N].astype(np.float64).reshape(H, W)
    partials(form + " pcg_init alphaN partials", aN, rc, g * g, g * g, 1)
    if exact:
        _bits(form + " pcg_init r", hr[:N], want.ravel())
    # apply_jtj and pcg_step1 on random planes
    rng = np.random.default_rng(W * 7 + H)
    mk = (lambda: rng.integers(-4, 5, N).astype(F32)) if exact else (lambda: rng.standard_normal(N).astype(F32))
    zv, pv, dv = mk(), mk(), mk()
    dz, dp = sk.dbuf(torch, tail(zv)), sk.dbuf(torch, tail(pv))
    keep += [(t, host(t).copy()) for t in (dz, dp)]
    Ap, aD = out(), sk.canary_buf(torch, PSLOTS)
    rc = L.thallo_hip_lapimg_apply_jtj(W, H, F32(w), xguard, dp.data_ptr(), Ap.data_ptr(), aD.data_ptr(), None)
    torch.cuda.synchronize()
    want, S = R.apply(pv)
    hA = host(Ap); canary_elsewhere(hA, all_px, "Ap")
    _note(form + " apply_jtj Ap", np.abs(hA[:N] - want.ravel()), sk.tol(K_LAP, S.ravel()))
    if exact:
        _bits(form + " apply_jtj Ap", hA[:N], want.ravel())
    t = pv.astype(np.float64) * hA[:N]
    partials(form + " apply_jtj alphaD partials", aD, rc, t.reshape(H, W), np.abs(t).reshape(H, W), 1)
    sc = scalars(torch, exact)
    for first in (1, 0):
        key = f"{form} pcg_step1 first = {first}"
        p_out, delta, Ap, aD = out(), sk.dbuf(torch, tail(dv)), out(), sk.canary_buf(torch, PSLOTS)
        rc = L.thallo_hip_lapimg_pcg_step1(W, H, F32(w), xguard, dz.data_ptr(), dp.data_ptr(), p_out.data_ptr(), delta.data_ptr(), Ap.data_ptr(), first, sc.aN, sc.aD, sc.bN, aD.data_ptr(), None)
        torch.cuda.synchronize()
        b = 0.0 if first else float(sc.beta)
        p1, p1a = zv + b * pv.astype(np.float64), np.abs(zv) + np.abs(b * pv)
        d1, d1a = (dv.astype(np.float64), np.abs(dv)) if first else (dv + float(sc.alpha) * pv.astype(np.float64), np.abs(dv) + np.abs(float(sc.alpha) * pv))
        want, S = R.apply(p1)
        hp, hd, hA = host(p_out), host(delta), host(Ap)
        canary_elsewhere(hp, all_px, "p_out"); canary_elsewhere(hA, all_px, "Ap"); canary_elsewhere(hd, all_px, "delta")
        _note(key + " p_out", np.abs(hp[:N] - p1), sk.tol(2, p1a))
        _note(key + " delta", np.abs(hd[:N] - d1), sk.tol(0 if first else 2, d1a))
        _note(key + " Ap", np.abs(hA[:N] - want.ravel()), sk.tol(K_LAP, S.ravel()) + R.apply(sk.tol(2, p1a))[1].ravel())
        if exact:
            _bits(key + " p_out", hp[:N], p1); _bits(key + " delta", hd[:N], d1); _bits(key + " Ap", hA[:N], want.ravel())
        t = hp[:N].astype(np.float64) * hA[:N]
        partials(key + " alphaD partials", aD, rc, t.reshape(H, W), np.abs(t).reshape(H, W), 1)
    torch.cuda.synchronize()
    for t, h in keep:
        assert sk.same_bytes(host(t), h), "an input changed"
