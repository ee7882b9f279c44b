"""The cross-rank pack / unpack kernels of csrc/pcg_kernels.hip in ONE process: the "gathered" buffer of `world` ranks (up to THALLO_DIST_MAX_WORLD = 8) is put
together in numpy, so the code for 4-8 ranks, 0-8 segments, empty pieces, a NULL neighbour at the image border and the (hi, lo) word encoding of the double sums runs
without a second GPU.  Copies are exact and everything outside the named pieces must keep its bytes (vectors carry sk.DVec's canary); the rank-ordered float sum is a
sequential float32 loop, bitwise; betaN = N - 2 alpha S1 + alpha^2 S2 is held to 1 float ulp of its float64 value (sk.beta_n; the test reads the expression's condition
number off its inputs), and is exact in the exact regime (alpha = 3/4, N, S1, S2 = 12, 8, 16: betaN = 9)."""
import math

import numpy as np
import pytest

import shim_kernels as sk
from shim_kernels import F32

pytestmark = pytest.mark.gpu

WORLDS = [1, 2, 3, 8]
# The pack / unpack launchers return 0, not their grid, so the grid cannot be read; the slab forms launch 8 workgroups of 256, the units / range forms at most 64.  The
# long piece is longer than one pass of ANY grid up to 64 workgroups (eight passes and a ragged one of the slab forms' 8), so it stays "longer than a whole grid pass" if
# those launch shapes change within that range.
LONG = 64 * 256 + 300
SLOT, NSLOT = LONG + 8, 16
PIECES = [0, 1, 255, 257, LONG]
COUNTS = [1, 5, 64, 65, 1024]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    return sk.shim()


def _pieces(rng, nseg, shift, total):
    """nseg pieces with lengths cycling through PIECES from `shift`, at shuffled non-overlapping offsets inside [0, total)"""
    lens = [PIECES[(shift + k) % len(PIECES)] for k in range(nseg)]
    slots = rng.permutation(total // SLOT)[:nseg]
    return [(int(s) * SLOT + int(rng.integers(0, 4)), l) for s, l in zip(slots, lens)]


def _split(total, world):
    """`world` multiples of 1/2 that add up to total"""
    each = np.floor(2.0 * total / world) / 2.0
    return [each] * (world - 1) + [total - each * (world - 1)]


def _apply(vec, pieces, src):
    base = 0
    for off, ln in pieces:
        vec[off:off + ln] = src[base:base + ln]; base += ln


def _check_bn(got, want, mag):
    if float(want) > 0 and np.isfinite(float(want)): assert mag / float(want) < 2.0 ** 20
    assert sk.ulp_apart(got, want) <= 1, (got, want)


NVEC = NSLOT * SLOT


# ------------------------------------------------------------------ row slabs
@pytest.mark.parametrize("count", [0, 1, 5, 1024])
@pytest.mark.parametrize("nseg", [0, 1, 2, 8])
def test_slab_pack(torch, L, nseg, count):
    """out = [sum of the partials in the documented order (count 0: word 0 is not written) | the pieces, concatenated]; nothing behind them."""
    rng = np.random.default_rng([nseg, count])
    vec = sk.DVec(torch, NVEC, sk.rounded_vec(rng, NVEC))
    pieces = _pieces(rng, nseg, count, NVEC)
    total = sum(l for _, l in pieces)
    part = sk.rounded_vec(rng, max(count, 1)); pt = sk.dbuf(torch, part)
    out = sk.canary_buf(torch, 1 + total + 64)
    assert L.thallo_hip_slab_pack(vec.ptr, sk.segs(pieces), sk.sumt(pt, count), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    want = np.full(1 + total + 64, sk.CANARY, np.uint32).view(F32).copy()
    if count: want[0] = sk.sum_partials(part[:count])
    want[1:1 + total] = np.concatenate([vec.h0[o:o + l] for o, l in pieces] + [np.zeros(0, F32)])
    assert sk.same_bytes(out.cpu().numpy(), want) and vec.unchanged()
    assert L.thallo_hip_slab_pack(vec.ptr, _bad_segs(), sk.sumt(pt, count), out.data_ptr(), None) == sk.INVALID


def _bad_segs():
    g = sk.segs([(0, 4)]); g.n = 9
    return g


@pytest.mark.parametrize("null", ["none", "top", "bot", "both"])
@pytest.mark.parametrize("nseg", [0, 1, 2, 8])
@pytest.mark.parametrize("world", WORLDS)
def test_slab_unpack(torch, L, world, nseg, null):
    """sum_out[0] = the ranks' word 0 added in rank order (a sequential float32 loop, bitwise); the ghost pieces <- the neighbours' rows; a NULL source leaves its ghost
    bit-untouched, and so is everything outside the ghost pieces."""
    rng = np.random.default_rng([world, nseg, len(null)])
    vec = sk.DVec(torch, NVEC, sk.rounded_vec(rng, NVEC))
    both = _pieces(rng, 2 * nseg, world, NVEC)
    top, bot = both[:nseg], both[nseg:]
    tt, tb = sum(l for _, l in top), sum(l for _, l in bot)
    stride = 1 + tt + tb + 3
    g = sk.rounded_vec(rng, world * stride); gt = sk.dbuf(torch, g)
    rank = world // 2
    o_top, o_bot = ((rank - 1) % world) * stride + 1, ((rank + 1) % world) * stride + 1 + tt
    p_top = None if null in ("top", "both") else gt.data_ptr() + 4 * o_top
    p_bot = None if null in ("bot", "both") else gt.data_ptr() + 4 * o_bot
    w = sk.canary_buf(torch, 2)
    assert L.thallo_hip_slab_unpack(vec.ptr, sk.segs(top), p_top, sk.segs(bot), p_bot, gt.data_ptr(), stride, world, w.data_ptr(), None) == 0
    torch.cuda.synchronize()
    want = vec.h0.copy()
    if p_top: _apply(want, top, g[o_top:])
    if p_bot: _apply(want, bot, g[o_bot:])
    assert sk.same_bytes(vec.get(), want) and sk.same_bytes(gt.cpu().numpy(), g)
    s = F32(0.0)
    for r in range(world): s = F32(s + g[r * stride])
    wh = w.cpu().numpy()
    assert sk.same_bytes(wh[:1], s) and sk.written_slots(wh) == 1
    vec2 = sk.DVec(torch, NVEC, vec.h0[:NVEC])
    assert L.thallo_hip_slab_unpack(vec2.ptr, sk.segs(top), p_top, sk.segs(bot), p_bot, gt.data_ptr(), stride, world, None, None) == 0       # (sum_out == NULL: rows only)
    torch.cuda.synchronize()
    assert sk.same_bytes(vec2.get(), want)


def _rank_sums(rng, regime, world, counts):
    """per rank: alphaD partials (float) and {N, S1, S2} partials (double).  Exact: they add up to alphaD = 16 and N, S1, S2 = 12, 8, 16 over the ranks."""
    out = []
    for r in range(world):
        c = counts[r % len(counts)]
        if regime == "exact":
            ad = sk.exact_sum(rng, c, _split(16.0, world)[r])
            s3 = np.stack([sk.exact_sum(rng, c, _split(t, world)[r]).astype(np.float64) for t in (12.0, 8.0, 16.0)], axis=1)
        else:
            ad = sk.rounded_sum(rng, c, positive=True)
            s3 = np.abs(rng.standard_normal((c, 3)) * 10.0 ** rng.integers(-3, 4, (c, 3)))
        out.append((ad, np.ascontiguousarray(s3)))
    return out


def _header(ad, s3):
    """the 7 scalar words of a rank's message: [alphaD | N, S1, S2 as (hi, lo)]"""
    return np.concatenate([[sk.sum_partials(ad)]] + [sk.hi_lo_words(sk.sum_partials_f64(s3[:, j])) for j in range(3)]).astype(F32)


@pytest.mark.parametrize("null", ["none", "top", "bot", "both"])
@pytest.mark.parametrize("regime", ["exact", "rounded"])
@pytest.mark.parametrize("nseg", [0, 1, 2, 8])
@pytest.mark.parametrize("world", WORLDS)
def test_slab_pack_iter_then_unpack_iter(torch, L, world, nseg, regime, null):
    """Every rank's message is packed on the device from its partials (counts 1, 5, 64, 65, 1024 in turn): word 0 = alphaD in the documented order, words 1-6 = the double
    sums (lane-strided, then the butterfly) as (hi, lo), bitwise; then the pieces.  The messages, gathered in numpy, are unpacked: alphaD_word = the sequential float32 sum
    over the ranks, bitwise; betaN_word to 1 ulp (exact regime: 9, bitwise).  The unpacking rank sits in the middle: its top ghost pieces take the upper neighbour's rows
    and its bottom ghost pieces -- other offsets, the lengths in reverse order -- the lower neighbour's; a NULL source (none / top / bot / both) leaves that ghost
    bit-untouched, and so is everything outside the ghost pieces."""
    rng = np.random.default_rng([world, nseg, regime == "exact", len(null)])
    gen = sk.exact_vec if regime == "exact" else sk.rounded_vec
    pieces = _pieces(rng, nseg, world, NVEC)
    total = sum(l for _, l in pieces)
    stride = 7 + total + 5
    sums = _rank_sums(rng, regime, world, COUNTS)
    msgs = np.full(world * stride, sk.CANARY, np.uint32).view(F32).copy()
    vecs = []
    for r, (ad, s3) in enumerate(sums):
        v = sk.DVec(torch, NVEC, gen(rng, NVEC)); vecs.append(v)
        adt, s3t, out = sk.dbuf(torch, ad), sk.dbuf(torch, s3), sk.canary_buf(torch, stride)
        assert L.thallo_hip_slab_pack_iter(v.ptr, sk.segs(pieces), adt.data_ptr(), s3t.data_ptr(), len(ad), out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        m = out.cpu().numpy()
        want = np.full(stride, sk.CANARY, np.uint32).view(F32).copy()
        want[:7] = _header(ad, s3)
        want[7:7 + total] = np.concatenate([v.h0[o:o + l] for o, l in pieces] + [np.zeros(0, F32)])
        assert sk.same_bytes(m, want), (r, m[:7], want[:7])
        assert v.unchanged() and sk.same_bytes(adt.cpu().numpy(), ad) and sk.same_bytes(s3t.cpu().numpy(), s3)
        msgs[r * stride:(r + 1) * stride] = m
    gt = sk.dbuf(torch, msgs)
    rank = world // 2
    vec = vecs[rank]
    an = F32(12.0) if regime == "exact" else F32(abs(rng.standard_normal()) + 0.5)
    ant, w = sk.dbuf(torch, np.array([an], F32)), sk.canary_buf(torch, 2)
    where = _pieces(rng, 2 * nseg, 0, NVEC)                          # 2 nseg distinct landing places; the lengths are the packed ones (top) and their reverse (bottom)
    top = [(o, l) for (o, _), (_, l) in zip(where[:nseg], pieces)]
    bot = [(o, l) for (o, _), (_, l) in zip(where[nseg:], pieces[::-1])]
    o_top, o_bot = ((rank - 1) % world) * stride + 7, ((rank + 1) % world) * stride + 7
    p_top = None if null in ("top", "both") else gt.data_ptr() + 4 * o_top
    p_bot = None if null in ("bot", "both") else gt.data_ptr() + 4 * o_bot
    assert L.thallo_hip_slab_unpack_iter(vec.ptr, sk.segs(top), p_top, sk.segs(bot), p_bot, gt.data_ptr(), stride, world, sk.sumt(ant), w.data_ptr(), w.data_ptr() + 4, None) == 0
    torch.cuda.synchronize()
    want = vec.h0.copy()
    if p_top: _apply(want, top, msgs[o_top:])
    if p_bot: _apply(want, bot, msgs[o_bot:])
    assert sk.same_bytes(vec.get(), want) and sk.same_bytes(gt.cpu().numpy(), msgs)
    adw, bnw, mag = sk.ref_rank_scalars(msgs, stride, world, an)
    wh = w.cpu().numpy()
    assert sk.same_bytes(wh[:1], adw)
    if regime == "exact": assert float(adw) == 16.0 and sk.same_bytes(wh[1:], F32(9.0))
    else: _check_bn(wh[1], bnw, mag)


@pytest.mark.parametrize("count", COUNTS)
def test_hi_lo_words_carry_every_double(torch, L, count):
    """Negative, subnormal and huge sums travel exactly: packed on the device and decoded in numpy they are the documented double sums, bit for bit; encoded in numpy and
    unpacked on the device they give betaN to 1 ulp (1e300 -> inf).  A cancelling case proves that the lo words arrive: alpha = 1, N = 3 + 2^-30, S1 = 3/2, S2 = 0 leaves
    betaN = 2^-30 exactly.  The expression is clamped to 0 when it is <= 0 or NaN."""
    rng = np.random.default_rng(count)
    special = np.array([-2.5, 5e-324, 1e300, -1e-310, 3.0 + 2.0 ** -30, -1e300, 2.0 ** -1040, 1.0 / 3.0])
    s3 = np.zeros((count, 3)); s3.reshape(-1)[:min(3 * count, 24)] = np.resize(special, min(3 * count, 24))
    s3[:, 2] = np.abs(s3[:, 2])
    ad = sk.rounded_sum(rng, count, True)
    adt, s3t, out = sk.dbuf(torch, ad), sk.dbuf(torch, s3), sk.canary_buf(torch, 7 + 8)
    vec = sk.DVec(torch, 8, np.arange(8))
    assert L.thallo_hip_slab_pack_iter(vec.ptr, sk.segs([]), adt.data_ptr(), s3t.data_ptr(), count, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    m = out.cpu().numpy()
    assert sk.written_slots(m) == 7
    for j in range(3):
        assert sk.same_bytes(sk.from_hi_lo(m[1 + 2 * j], m[2 + 2 * j]), sk.sum_partials_f64(s3[:, j]))
    cases = [   # (per-rank (alphaD, N, S1, S2), alphaN)
        ([(1.0, -2.5, 5e-324, 1e300), (0.5, 5e-324, -1e-310, 2.0 ** -1040), (0.25, 1e300, 0.0, 1.0)], 0.0),
        ([(2.0, 3.0 + 2.0 ** -30, 1.0, 0.0), (1.0, 0.0, 0.5, 0.0)], 3.0),
        ([(16.0, 1.0, 8.0, 4.0)], 12.0),                                       # 1 - 12 + 2.25 < 0
        ([(16.0, float("nan"), 8.0, 4.0)], 12.0),
        ([(16.0, 4.0, 8.0, 1e300), (0.0, 4.0, 1.0, -1e300)], 12.0),
    ]
    wants = [None, 2.0 ** -30, 0.0, 0.0, None]
    for (ranks, an), exact in zip(cases, wants):
        world, stride = len(ranks), 9
        g = np.zeros(world * stride, F32)
        for r, (a, n_, s1, s2) in enumerate(ranks):
            g[r * stride] = a
            for j, x in enumerate((n_, s1, s2)): g[r * stride + 1 + 2 * j:r * stride + 3 + 2 * j] = sk.hi_lo_words(x)
        gt, ant, w = sk.dbuf(torch, g), sk.dbuf(torch, np.array([an], F32)), sk.canary_buf(torch, 2)
        assert L.thallo_hip_slab_unpack_iter(vec.ptr, sk.segs([]), None, sk.segs([]), None, gt.data_ptr(), stride, world, sk.sumt(ant), w.data_ptr(), w.data_ptr() + 4, None) == 0
        torch.cuda.synchronize()
        adw, bnw, mag = sk.ref_rank_scalars(g, stride, world, F32(an))
        wh = w.cpu().numpy()
        assert sk.same_bytes(wh[:1], adw), (wh, adw)
        if exact is not None: assert sk.same_bytes(wh[1:], F32(exact)) and float(bnw) == exact, (wh, bnw)
        else: assert sk.ulp_apart(wh[1], bnw) <= 1 if np.isfinite(float(bnw)) else sk.same_bytes(wh[1:], bnw), (wh, bnw)
    assert vec.unchanged()


# ------------------------------------------------------------------ ghost units of a partitioned graph
PLANES = {1: [3], 3: [2, 1, 4], 8: [1, 2, 3, 1, 2, 1, 4, 2]}
NUNITS = 400


def _units(torch, rng, nplanes, n, with_src=None):
    lens = PLANES[nplanes]
    u = sk.UnitsT(); u.n = n; u.nplanes = nplanes
    base = 0
    for k, l in enumerate(lens): u.base[k] = base; u.len[k] = l; base += NUNITS * l
    ids = rng.permutation(NUNITS)[:n].astype(np.int32)                 # unsorted, distinct
    keep = [sk.dbuf(torch, ids if n else np.zeros(1, np.int32))]
    u.units = keep[0].data_ptr()
    if with_src is not None:
        keep.append(sk.dbuf(torch, with_src if n else np.zeros(1, np.int64)))
        u.src = keep[1].data_ptr()
    return u, ids, lens, base, keep


def _unit_floats(vec, ids, lens):
    """unit-major: for each listed unit its floats of plane 0, plane 1, ..."""
    out, base = [], 0
    bases = np.concatenate([[0], np.cumsum([NUNITS * l for l in lens])])
    for uid in ids:
        for k, l in enumerate(lens): out.append(vec[bases[k] + uid * l: bases[k] + uid * l + l])
    return np.concatenate(out + [np.zeros(0, F32)])


@pytest.mark.parametrize("n", [0, 1, 300])
@pytest.mark.parametrize("nplanes", [1, 3, 8])
@pytest.mark.parametrize("world", WORLDS)
def test_units_pack_and_unpack(torch, L, world, nplanes, n):
    """thallo_hip_units_pack(_iter): message = [1 (or 7) scalar words as the slab forms write them | unit 0's floats of every plane | unit 1's | ...] for an UNSORTED unit
    list over planes of unequal width; thallo_hip_units_unpack(_iter): vec[plane k of ghost g] <- gathered[src[g] ...], the rank-ordered scalars exactly as the slab forms;
    exact copies, the rest of vec untouched."""
    rng = np.random.default_rng([world, nplanes, n])
    per = sum(PLANES[nplanes]); nvec = NUNITS * per
    vec = sk.DVec(torch, nvec, sk.rounded_vec(rng, nvec))
    u, ids, lens, _, keep = _units(torch, rng, nplanes, n)
    count = COUNTS[(world + nplanes) % 5]
    (ad, s3), = _rank_sums(rng, "rounded", 1, [count])
    adt, s3t = sk.dbuf(torch, ad), sk.dbuf(torch, s3)
    body = _unit_floats(vec.h0, ids, lens)
    for hdr in (1, 7):
        out = sk.canary_buf(torch, hdr + n * per + 16)
        if hdr == 1: assert L.thallo_hip_units_pack(vec.ptr, u, sk.sumt(adt), out.data_ptr(), None) == 0
        else: assert L.thallo_hip_units_pack_iter(vec.ptr, u, adt.data_ptr(), s3t.data_ptr(), count, out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        want = np.full(hdr + n * per + 16, sk.CANARY, np.uint32).view(F32).copy()
        want[:hdr] = _header(ad, s3)[:hdr]; want[hdr:hdr + n * per] = body
        assert sk.same_bytes(out.cpu().numpy(), want)
    assert vec.unchanged()
    for hdr in (1, 7):
        stride = hdr + 40 * per + 3
        g = sk.rounded_vec(rng, world * stride)
        if hdr == 7:
            for r, (a, s) in enumerate(_rank_sums(rng, "rounded", world, COUNTS)): g[r * stride:r * stride + 7] = _header(a, s)
        src = (rng.integers(0, world, n) * stride + hdr + rng.integers(0, 40, n) * per).astype(np.int64)
        u2, ids2, lens, _, keep2 = _units(torch, rng, nplanes, n, with_src=src)
        v = sk.DVec(torch, nvec, vec.h0[:nvec])
        gt, w = sk.dbuf(torch, g), sk.canary_buf(torch, 2)
        an = F32(abs(rng.standard_normal()) + 0.5); ant = sk.dbuf(torch, np.array([an], F32))
        if hdr == 1: assert L.thallo_hip_units_unpack(v.ptr, u2, gt.data_ptr(), stride, world, w.data_ptr(), None) == 0
        else: assert L.thallo_hip_units_unpack_iter(v.ptr, u2, gt.data_ptr(), stride, world, sk.sumt(ant), w.data_ptr(), w.data_ptr() + 4, None) == 0
        torch.cuda.synchronize()
        want = v.h0.copy()
        bases = np.concatenate([[0], np.cumsum([NUNITS * l for l in lens])])
        for gi, uid in enumerate(ids2):
            within = 0
            for k, l in enumerate(lens):
                want[bases[k] + uid * l: bases[k] + uid * l + l] = g[src[gi] + within: src[gi] + within + l]; within += l
        assert sk.same_bytes(v.get(), want) and sk.same_bytes(gt.cpu().numpy(), g)
        wh = w.cpu().numpy()
        if hdr == 1:
            s = F32(0.0)
            for r in range(world): s = F32(s + g[r * stride])
            assert sk.same_bytes(wh[:1], s) and sk.written_slots(wh) == 1
        else:
            adw, bnw, mag = sk.ref_rank_scalars(g, stride, world, an)
            assert sk.same_bytes(wh[:1], adw)
            _check_bn(wh[1], bnw, mag)


# ------------------------------------------------------------------ vertex ranges
@pytest.mark.parametrize("skip", [0, 7])
@pytest.mark.parametrize("lens", [[300], [5, 257, 2100]])
@pytest.mark.parametrize("world", WORLDS)
def test_range_unpack(torch, L, world, lens, skip):
    """vec[first.off[j] + r len[j] + i] = gathered[r stride + skip + (pieces before j) + i] for every rank r and piece j; stride larger than the payload; the rest of vec
    keeps its bytes."""
    rng = np.random.default_rng([world, len(lens), skip])
    offs, at = [], 3
    for l in lens: offs.append(at); at += world * l + 11
    vec = sk.DVec(torch, at, sk.rounded_vec(rng, at))
    stride = skip + sum(lens) + 13
    g = sk.rounded_vec(rng, world * stride); gt = sk.dbuf(torch, g)
    assert L.thallo_hip_range_unpack(vec.ptr, sk.segs(list(zip(offs, lens))), gt.data_ptr(), stride, skip, world, None) == 0
    torch.cuda.synchronize()
    want = vec.h0.copy()
    for r in range(world):
        base = r * stride + skip
        for o, l in zip(offs, lens):
            want[o + r * l:o + (r + 1) * l] = g[base:base + l]; base += l
    assert sk.same_bytes(vec.get(), want) and sk.same_bytes(gt.cpu().numpy(), g)
    assert L.thallo_hip_range_unpack(vec.ptr, sk.segs([]), gt.data_ptr(), stride, skip, world, None) == sk.INVALID


# ------------------------------------------------------------------ shards (bundle adjustment across ranks)
@pytest.mark.parametrize("regime", ["exact", "rounded"])
@pytest.mark.parametrize("has_pre", [True, False])
@pytest.mark.parametrize("n", [4, 1020, 4 * 256 * 33, "ragged"])
def test_block_sums(torch, L, n, has_pre, regime):
    """Per workgroup: the float partial of p.Ap -- within (c + 1) 2^-24 sum|terms| (c = sk.chain_length) -- and the doubles N = sum m r r, S1 = sum m r Ap, S2 = sum m Ap Ap
    from exact products of the float data: the inner product of two floats is exact in double, m (...) rounds once, then c additions: (c + 1) 2^-53 sum|terms|, and one more
    2^-53 for the same rounding in the reference's own terms (its sums are exact: math.fsum).  Equal in
    the exact regime.  pre == NULL: m = 1."""
    cus = L.thallo_hip_device_cu_count()
    if n == "ragged": n = 4 * 256 * sk.flat_grid(10 ** 9, cus) + 4 * 300
    rng = np.random.default_rng([n, has_pre, regime == "exact"])
    gen, genp = (sk.exact_vec, sk.exact_pre) if regime == "exact" else (sk.rounded_vec, sk.rounded_pre)
    p, Ap, r = (sk.DVec(torch, n, gen(rng, n)) for _ in range(3))
    pre = sk.DVec(torch, n, genp(rng, n)) if has_pre else None
    ab, sb = sk.canary_buf(torch, sk.MAX_PARTIALS + 8), sk.canary_buf(torch, 3 * (sk.MAX_PARTIALS + 8), np.float64).reshape(-1, 3)
    ret = L.thallo_hip_block_sums(p.ptr, Ap.ptr, r.ptr, pre.ptr if pre else None, n, ab.data_ptr(), sb.data_ptr(), None)
    torch.cuda.synchronize()
    grid = sk.flat_grid(n // 4, cus)
    assert ret == grid
    for v in (p, Ap, r) + ((pre,) if pre else ()): assert v.unchanged()
    ah, sh = ab.cpu().numpy(), sb.cpu().numpy()
    assert sk.written_slots(ah) == grid and sk.written_slots(sh) == grid
    f = lambda v: v.h0[:n].astype(np.float64)
    terms = sk.ref_block_sums(f(p), f(Ap), f(r), f(pre) if pre else None)
    c = sk.chain_length(n, grid)
    for j, t in enumerate(terms):
        got = ah[:grid].astype(np.float64) if j == 0 else sh[:grid, j - 1]
        if regime == "exact":
            sk.assert_exact_sums(t, grid, 2.0 ** -2)
            assert np.array_equal(got, sk.block_sums(t, grid))
        elif j == 0:
            assert (np.abs(got - sk.block_sums(t, grid)) <= sk.tol(c + 1, sk.block_sums(np.abs(t), grid))).all()
        else:
            # the reference must not spend the budget itself: its terms m (r r) carry one double rounding each (r r is exact), its sums are math.fsum's (exact)
            blk = sk.block_of(n, grid)
            order = np.argsort(blk, kind="stable"); cuts = np.searchsorted(blk[order], np.arange(grid + 1))
            want = np.array([math.fsum(t[order[cuts[b]:cuts[b + 1]]]) for b in range(grid)])
            bound = (c + 2) * 2.0 ** -53 * sk.block_sums(np.abs(t), grid)
            assert (np.abs(got - want) <= bound).all()
    assert L.thallo_hip_block_sums(p.ptr, Ap.ptr, r.ptr, None, 6, ab.data_ptr(), sb.data_ptr(), None) == sk.INVALID


@pytest.mark.parametrize("regime", ["exact", "rounded"])
@pytest.mark.parametrize("count", [1, 65, 1024])
@pytest.mark.parametrize("world", WORLDS)
def test_shard_scalars(torch, L, world, count, regime):
    """alphaD = the ranks' word 0 in rank order (sequential float32) + the shared block's float partials in the documented order, bitwise; betaN from the ranks' (hi, lo)
    doubles + the shared block's double partials, 1 ulp (exact regime: alphaD = 16 + 16, alphaN = 24: alpha = 3/4, N, S1, S2 = 24, 16, 32: betaN = 18, bitwise).
    betaN_word == NULL: only word 0 of every message and the float partials are added."""
    rng = np.random.default_rng([world, count, regime == "exact"])
    stride = 11
    ranks = _rank_sums(rng, regime, world, COUNTS)
    g = sk.rounded_vec(rng, world * stride)
    for r, (a, s) in enumerate(ranks): g[r * stride:r * stride + 7] = _header(a, s)
    (ad, s3), = _rank_sums(rng, regime, 1, [count])
    an = F32(24.0) if regime == "exact" else F32(abs(rng.standard_normal()) + 0.5)
    gt, adt, s3t, ant, w = sk.dbuf(torch, g), sk.dbuf(torch, ad), sk.dbuf(torch, s3), sk.dbuf(torch, np.array([an], F32)), sk.canary_buf(torch, 4)
    assert L.thallo_hip_shard_scalars(gt.data_ptr(), stride, world, adt.data_ptr(), s3t.data_ptr(), count, sk.sumt(ant), w.data_ptr(), w.data_ptr() + 4, None) == 0
    assert L.thallo_hip_shard_scalars(gt.data_ptr(), stride, world, adt.data_ptr(), None, count, sk.sumt(ant), w.data_ptr() + 8, None, None) == 0
    torch.cuda.synchronize()
    for t, h in ((gt, g), (adt, ad), (s3t, s3)): assert sk.same_bytes(t.cpu().numpy(), h)
    adw, bnw, mag = sk.ref_rank_scalars(g, stride, world, an, extra_ad=ad, extra_s3=s3)
    wh = w.cpu().numpy()
    assert sk.same_bytes(wh[0:1], adw) and sk.same_bytes(wh[2:3], adw) and sk.written_slots(wh) == 3
    if regime == "exact": assert float(adw) == 32.0 and sk.same_bytes(wh[1:2], F32(18.0))
    else: _check_bn(wh[1], bnw, mag)
