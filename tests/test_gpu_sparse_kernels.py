"""The materialized-schedule and index kernels of csrc/spmv_kernels.hip against numpy: csr_spmv, ell_apply (three modes), dense_gemv, jtj_scatter and the per-owner
instance lists (incidence_count + incidence_fill: a multi-pass scan with its carry, a heap sort above 32 entries per owner).  Row lengths are mixed and include empty
rows, columns repeat, and the scatter kernels are given many products per slot.

Exact regime: small integers, every sum below 2^24 (asserted on the CPU): the device must equal numpy whatever order its atomics take.  Rounded regime:
standard_normal * 10^U{-3..3}; a sum of m products in float32 lies within (m + 1) 2^-24 sum|terms| of float64 in any order (m - 1 additions, one rounding per product,
one to spare for the `+1`s of the lane-strided forms); each test states its m."""
import ctypes as C

import numpy as np
import pytest

import shim_kernels as sk
from shim_kernels import F32

pytestmark = pytest.mark.gpu
REGIMES = ["exact", "rounded"]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    return sk.shim()


def _vals(rng, regime, shape, amp=8):
    if regime == "exact": return rng.integers(-amp, amp + 1, shape).astype(F32)
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(F32)


def _guarded(torch, a, front=8, back=8):
    """the array `a` on the device with canary words in front of and behind it: returns (tensor, byte offset of a[0], checker)"""
    a = np.ascontiguousarray(a)
    per = a.dtype.itemsize // 4
    h = np.full((front + back) * per + a.size * per, sk.CANARY, np.uint32)
    h[front * per:front * per + a.size * per] = a.view(np.uint32).reshape(-1)
    t = torch.from_numpy(h.copy()).cuda()

    def read():
        g = t.cpu().numpy()
        assert (g[:front * per] == sk.CANARY).all() and (g[front * per + a.size * per:] == sk.CANARY).all(), "wrote outside the buffer"
        return g[front * per:front * per + a.size * per].view(a.dtype).reshape(a.shape)
    return t, t.data_ptr() + 4 * front * per, read


# ------------------------------------------------------------------ CSR
def _csr_grid(rows, cus):
    """thallo_hip_csr_spmv's launch: one workgroup per 256 rows, at most min(4 CUs, 1024)"""
    return max(1, min((rows + 255) // 256, min(4 * cus, sk.MAX_PARTIALS)))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("rows", [1, 255, 256, 257, "ragged"])
def test_csr_spmv(torch, L, rows, regime):
    """y = A x, one thread per row, the row's entries added in their order: |y_i - float64| <= (len_i + 1) 2^-24 sum_k |v_k x_k| (len_i products, len_i - 1 additions and the
    first addition to 0).  Row lengths from {0, 1, 5, 300} (few of the long ones in the largest case, 256 grid + 300 rows: the stride loop's ragged second pass), columns drawn
    with repetition.  With dot_with: the partials of w.y per workgroup (row i -> workgroup (i / 256) % grid), within (c + 1) 2^-24 sum|w y| of the float64 dot of the
    device's y, c = rows per lane + 6 + 4.  Without: dot_out is not touched.  rows == 0 returns 0."""
    cus = L.thallo_hip_device_cu_count()
    big = rows == "ragged"
    if big: rows = 256 * _csr_grid(10 ** 9, cus) + 300
    rng = np.random.default_rng([rows, regime == "exact"])
    lens = rng.choice([0, 1, 5, 300], rows, p=[0.3, 0.4, 0.29, 0.01] if big else [0.25, 0.25, 0.25, 0.25])
    if rows >= 255: lens[:4] = [300, 0, 5, 1]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz, ncols = int(rowptr[-1]), 97
    col = rng.integers(0, ncols, max(nnz, 1)).astype(np.int32)
    if nnz > 8: col[1] = col[0]; col[2] = col[0]                       # (a repeated column inside one row)
    val, x, w = _vals(rng, regime, max(nnz, 1)), _vals(rng, regime, ncols), _vals(rng, regime, rows)
    dev = [sk.dbuf(torch, a) for a in (rowptr, col, val, x, w)]
    grid = _csr_grid(rows, cus)
    prod = val[:nnz].astype(np.float64) * x[col[:nnz]].astype(np.float64)
    row_of = np.repeat(np.arange(rows), lens)
    want = np.bincount(row_of, weights=prod, minlength=rows)
    mag = np.bincount(row_of, weights=np.abs(prod), minlength=rows)
    for with_dot in (True, False):
        yt, yptr, yread = _guarded(torch, np.full(rows, sk.CANARY, np.uint32).view(F32))
        pb = sk.canary_buf(torch, sk.MAX_PARTIALS + 8)
        ret = L.thallo_hip_csr_spmv(rows, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), yptr, dev[4].data_ptr() if with_dot else None,
                                    pb.data_ptr() if with_dot else None, None)
        torch.cuda.synchronize()
        assert ret == grid
        y = yread()
        if regime == "exact":
            assert mag.max() < 2 ** 24 and np.array_equal(y, want.astype(F32))
        else:
            assert (np.abs(y - want) <= sk.tol(1, (lens + 1) * mag)).all()
        ph = pb.cpu().numpy()
        if not with_dot:
            assert sk.written_slots(ph) == 0
            continue
        assert sk.written_slots(ph) == grid
        blk = (np.arange(rows) // 256) % grid
        terms = w.astype(np.float64) * y.astype(np.float64)
        sums, mags = np.bincount(blk, weights=terms, minlength=grid), np.bincount(blk, weights=np.abs(terms), minlength=grid)
        if regime == "exact": assert mags.max() < 2 ** 24 and np.array_equal(ph[:grid], sums.astype(F32))
        else:
            c = (rows + 256 * grid - 1) // (256 * grid) + 6 + 4
            assert (np.abs(ph[:grid] - sums) <= sk.tol(c + 1, mags)).all()
    for t, a in zip(dev, (rowptr, col, val, x, w)): assert sk.same_bytes(t.cpu().numpy(), a)
    assert L.thallo_hip_csr_spmv(0, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), yptr, None, None, None) == 0
    assert L.thallo_hip_csr_spmv(4, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), yptr, dev[4].data_ptr(), None, None) == sk.INVALID


# ------------------------------------------------------------------ ELL
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("rows,K", [(1, 1), (257, 2), (600, 5), (600, 9), (70001, 2), (256 * 4096 + 257, 1)])
def test_ell_apply(torch, L, rows, K, regime):
    """mode 1: Jp_i = sum_k v_ik p[c_ik] over the entries with c >= 0 (K products, K additions from 0: (K + 1) 2^-24 S_i, S_i = sum_k |v p|); mode 2: Ap[c_ik] += Jp_i v_ik
    over the entries with c >= 0 and v != 0; mode 0: both in one pass.  Ap starts non-zero and every row names column 0: a slot that receives m products carries at most
    (m + K + 2) 2^-24 (|Ap_0| + sum_i |v_ic| S_i) of error in any order of the atomics (the K + 1 of Jp_i, the product, m additions) -- loose for the million-row case, where
    the exact regime is the sharp check: there the device equals numpy, and mode 0 equals mode 1 then mode 2.  col = -1 entries are skipped: p[-1] is never needed and the
    word in front of Ap stays a canary.  The last case (K = 1) is past one pass of the 4096-workgroup grid."""
    rng = np.random.default_rng([rows, K, regime == "exact"])
    ncols = 61
    amp = 8 if rows <= 600 else 2 if rows < 10 ** 5 else 1
    val = _vals(rng, regime, (rows, K), amp)
    col = rng.integers(0, ncols, (rows, K)).astype(np.int32)
    col[:, 0] = 0                                                          # contention: every row hits column 0
    if K > 1 or rows > 1: col[rng.uniform(size=(rows, K)) < 0.15] = -1
    val[rng.uniform(size=(rows, K)) < 0.1] = 0.0
    p = _vals(rng, regime, ncols, amp); Ap0 = _vals(rng, regime, ncols, amp)
    on = col >= 0
    cc = np.where(on, col, 0)
    vp = np.where(on, val.astype(np.float64) * p[cc].astype(np.float64), 0.0)
    Jp, S = vp.sum(axis=1), np.abs(vp).sum(axis=1)
    live = on & (val != 0)

    def scatter(jp):
        contrib = np.where(live, jp[:, None] * val.astype(np.float64), 0.0)
        return Ap0.astype(np.float64) + np.bincount(cc.reshape(-1), weights=contrib.reshape(-1), minlength=ncols)
    Ap_mag = np.abs(Ap0.astype(np.float64)) + np.bincount(cc.reshape(-1), weights=np.where(live, np.abs(val.astype(np.float64)) * S[:, None], 0.0).reshape(-1), minlength=ncols)
    m = np.bincount(cc.reshape(-1), weights=live.reshape(-1).astype(np.float64), minlength=ncols)
    vt, ct, pt = sk.dbuf(torch, val), sk.dbuf(torch, col), _guarded(torch, p)
    jt, jptr, jread = _guarded(torch, np.full(rows, sk.CANARY, np.uint32).view(F32))
    outs = {}
    for mode in (1, 2, 0):
        at, aptr, aread = _guarded(torch, Ap0)
        assert L.thallo_hip_ell_apply(mode, rows, K, vt.data_ptr(), ct.data_ptr(), pt[1] if mode != 2 else None, jptr if mode != 0 else None, aptr if mode != 1 else None, None) == 0
        torch.cuda.synchronize()
        outs[mode] = jread().copy() if mode == 1 else aread().copy()
    jp_dev = outs[1]
    if regime == "exact":
        assert S.max() < 2 ** 24 and Ap_mag.max() < 2 ** 24
        assert np.array_equal(jp_dev, Jp.astype(F32))
        assert np.array_equal(outs[2], scatter(Jp).astype(F32)) and np.array_equal(outs[0], outs[2])
    else:
        assert (np.abs(jp_dev - Jp) <= sk.tol(K + 1, S)).all()
        want = scatter(Jp)
        for mode in (0, 2):
            assert (np.abs(outs[mode] - want) <= sk.tol(m + K + 2, Ap_mag)).all(), mode
    assert sk.same_bytes(vt.cpu().numpy(), val) and sk.same_bytes(ct.cpu().numpy(), col) and sk.same_bytes(pt[2](), p)
    assert L.thallo_hip_ell_apply(3, rows, K, vt.data_ptr(), ct.data_ptr(), pt[1], jptr, aptr, None) == sk.INVALID
    assert L.thallo_hip_ell_apply(0, 0, K, vt.data_ptr(), ct.data_ptr(), pt[1], None, aptr, None) == 0


# ------------------------------------------------------------------ dense gemv
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 600])
def test_dense_gemv(torch, L, n, regime):
    """y = M x, one wave per row: lane l adds its ceil(n / 64) products, then 6 butterfly levels: (ceil(n / 64) + 6 + 1) 2^-24 sum_k |M_rk x_k|."""
    rng = np.random.default_rng([n, regime == "exact"])
    M, x = _vals(rng, regime, (n, n)), _vals(rng, regime, n)
    Mt, xt = sk.dbuf(torch, M), sk.dbuf(torch, x)
    yt, yptr, yread = _guarded(torch, np.full(n, sk.CANARY, np.uint32).view(F32))
    assert L.thallo_hip_dense_gemv(n, Mt.data_ptr(), xt.data_ptr(), yptr, None) == 0
    torch.cuda.synchronize()
    y = yread()
    want = M.astype(np.float64) @ x.astype(np.float64)
    mag = np.abs(M.astype(np.float64)) @ np.abs(x.astype(np.float64))
    if regime == "exact": assert mag.max() < 2 ** 24 and np.array_equal(y, want.astype(F32))
    else: assert (np.abs(y - want) <= sk.tol((n + 63) // 64 + 6 + 1, mag)).all()
    assert sk.same_bytes(Mt.cpu().numpy(), M) and sk.same_bytes(xt.cpu().numpy(), x)
    assert L.thallo_hip_dense_gemv(0, Mt.data_ptr(), xt.data_ptr(), yptr, None) == sk.INVALID


# ------------------------------------------------------------------ sparse J^T J, numeric phase
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("rows,K", [(1, 1), (257, 3), (5000, 5), (256 * 4096 + 300, 1)])
def test_jtj_scatter(torch, L, rows, K, regime):
    """out[dest[(i K + a) K + b]] += v_ia v_ib for dest >= 0 (zero products are skipped): 7 slots, so many products land in one; a slot with m products carries at most
    (m + 1) 2^-24 (|out_0| + sum |v v|) in any order.  dest = -1 entries are skipped: the word in front of `out` stays a canary."""
    rng = np.random.default_rng([rows, K, regime == "exact"])
    nslots = 7
    val = _vals(rng, regime, (rows, K), 8 if rows <= 5000 else 2)
    val[rng.uniform(size=(rows, K)) < 0.1] = 0.0
    dest = rng.integers(-1, nslots, (rows, K, K)).astype(np.int32)
    out0 = _vals(rng, regime, nslots)
    prod = val.astype(np.float64)[:, :, None] * val.astype(np.float64)[:, None, :]
    live = (dest >= 0) & (prod != 0)
    dd = np.where(live, dest, 0).reshape(-1)
    want = out0.astype(np.float64) + np.bincount(dd, weights=np.where(live, prod, 0.0).reshape(-1), minlength=nslots)
    mag = np.abs(out0.astype(np.float64)) + np.bincount(dd, weights=np.where(live, np.abs(prod), 0.0).reshape(-1), minlength=nslots)
    m = np.bincount(dd, weights=live.reshape(-1).astype(np.float64), minlength=nslots)
    vt, dt = sk.dbuf(torch, val), sk.dbuf(torch, dest)
    ot, optr, oread = _guarded(torch, out0)
    assert L.thallo_hip_jtj_scatter(rows, K, vt.data_ptr(), dt.data_ptr(), optr, None) == 0
    torch.cuda.synchronize()
    got = oread()
    if regime == "exact": assert mag.max() < 2 ** 24 and np.array_equal(got, want.astype(F32))
    else: assert (np.abs(got - want) <= sk.tol(m + 1, mag)).all()
    assert sk.same_bytes(vt.cpu().numpy(), val) and sk.same_bytes(dt.cpu().numpy(), dest)
    assert L.thallo_hip_jtj_scatter(0, K, vt.data_ptr(), dt.data_ptr(), optr, None) == 0


# ------------------------------------------------------------------ per-owner instance lists
LIST_LENGTHS = [0, 1, 32, 33, 5000]


def _incidence_problem(rng, npix, K, ch):
    """col[n][K], slot bases / channels and the expected owner matrix.  Owners 0..4 (as far as npix has them, spread over the index range) receive lists of exactly
    0, 1, 32, 33 and 5000 instances through slot 0; further slots repeat the instance's owner (counted once), name a random other owner, are -1, point outside
    [0, npix) on either side -- base - 1 and base - 2 included, which a division that rounds towards zero would hand to owner 0 when ch = 3 --, or belong to a slot whose
    base is < 0 (not of the owner group).  The instances arrive shuffled."""
    bases = np.array([1000 + 7 * q for q in range(K)], np.int64)           # every slot its own image offset
    chs = np.full(K, ch, np.int32)
    if K >= 3: bases[K - 1] = -1                                           # this slot's image is not of the owner group
    special = [int(x) for x in np.unique(np.linspace(0, max(npix - 1, 0), 5).astype(int))] if npix else []
    prim = np.concatenate([np.full(l, px) for px, l in zip(special[::-1], LIST_LENGTHS[::-1][:len(special)])] + [np.zeros(0, int)]).astype(np.int64)
    extra = rng.integers(0, max(npix, 1), 200 if K < 48 else 40)
    extra = extra[~np.isin(extra, special)] if npix else np.zeros(7, np.int64)
    prim = rng.permutation(np.concatenate([prim, extra]))
    n = prim.size
    col = np.full((n, K), -1, np.int64)
    hi = lambda q: bases[q] + npix * ch                                       # first index past slot q's image
    col[:, 0] = bases[0] + prim * ch + rng.integers(0, ch, n) if npix else hi(0) + rng.integers(0, 5, n)
    for q in range(1, K):
        kind = rng.integers(0, 5, n)
        if bases[q] < 0:
            col[:, q] = rng.integers(0, 50, n)
            continue
        other = rng.integers(0, max(npix, 1), n)
        other = np.where(np.isin(other, special), prim, other)            # (the five measured lists get nothing but their slot-0 instances)
        col[:, q] = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [bases[q] + prim * ch + rng.integers(0, ch, n), bases[q] + other * ch,
                                                                             -1, hi(q) + rng.integers(0, 9, n)], bases[q] - 1 - rng.integers(0, 9, n))
        if not npix: col[:, q] = np.where(kind < 2, hi(q) + 3, col[:, q])
    return col.astype(np.int32), bases, chs, n


def _incidence_reference(col, bases, chs, npix):
    """(ptr, els): an instance counts once per distinct owner; every owner's list ascending"""
    n, K = col.shape
    c = col.astype(np.int64)
    px = (c - bases[None, :]) // chs[None, :]
    ok = (bases[None, :] >= 0) & (c >= 0) & (c - bases[None, :] >= 0) & (px < npix)
    el = np.repeat(np.arange(n), K).reshape(n, K)
    pairs = np.unique(np.stack([px[ok], el[ok]], axis=1), axis=0) if ok.any() else np.zeros((0, 2), np.int64)      # sorted by owner, then instance; distinct
    ptr = np.concatenate([[0], np.cumsum(np.bincount(pairs[:, 0], minlength=npix))]).astype(np.int32) if npix else np.zeros(1, np.int32)
    return ptr, pairs[:, 1].astype(np.int32)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("K", [1, 3, 48])
@pytest.mark.parametrize("npix", [0, 1, 4095, 4096, 4097, 8193, 3 * 4096 + 5])
def test_incidence_lists(torch, L, npix, K, ch):
    """incidence_count: ptr[0 .. npix] = the CSR row pointer of the lists -- counts, then an in-place scan of 4096 entries per pass with a carried sum: one pass, exactly
    one, two and four passes --, *total = ptr[npix].  incidence_fill: els = every owner's instances ascending (insertion sort up to 32, heap sort above: lists of 33 and
    5000).  Against a numpy construction, exactly; the inputs are not modified and nothing is written behind ptr / els."""
    rng = np.random.default_rng([npix, K, ch])
    col, bases, chs, n = _incidence_problem(rng, npix, K, ch)
    ptr_w, els_w = _incidence_reference(col, bases, chs, npix)
    if npix > 4:
        lens = np.diff(ptr_w)
        assert sorted(set(LIST_LENGTHS) - set(lens.tolist())) == [], "the problem lost one of its list lengths"
    ct = sk.dbuf(torch, col)
    sb, sc = (C.c_long * K)(*[int(b) for b in bases]), (C.c_int * K)(*[int(c) for c in chs])
    pt, pptr, pread = _guarded(torch, np.full(npix + 1, sk.CANARY, np.uint32).view(np.int32))
    tt, tptr, tread = _guarded(torch, np.full(1, -1, np.int64))
    assert L.thallo_hip_incidence_count(ct.data_ptr(), n, K, sb, sc, npix, pptr, tptr, None) == 0
    torch.cuda.synchronize()
    ptr = pread().copy()
    assert np.array_equal(ptr, ptr_w), np.flatnonzero(ptr != ptr_w)[:8]
    total = int(tread()[0])
    assert total == int(ptr[npix]) == els_w.size
    cur = sk.dbuf(torch, np.full(max(npix, 1), 77, np.int32))
    et, eptr, eread = _guarded(torch, np.full(max(total, 1), sk.CANARY, np.uint32).view(np.int32))
    assert L.thallo_hip_incidence_fill(ct.data_ptr(), n, K, sb, sc, npix, pptr, cur.data_ptr(), eptr, None) == 0
    torch.cuda.synchronize()
    els = eread()[:total]
    assert np.array_equal(els, els_w), np.flatnonzero(els != els_w)[:8]
    for a, b in zip(ptr[:-1], ptr[1:]): assert (np.diff(els[a:b]) > 0).all()
    assert np.array_equal(pread(), ptr_w) and sk.same_bytes(ct.cpu().numpy(), col)
    # no instances at all: empty lists
    assert L.thallo_hip_incidence_count(ct.data_ptr(), 0, K, sb, sc, npix, pptr, tptr, None) == 0
    assert L.thallo_hip_incidence_fill(ct.data_ptr(), 0, K, sb, sc, npix, pptr, cur.data_ptr(), eptr, None) == 0
    torch.cuda.synchronize()
    assert not pread().any() and int(tread()[0]) == 0
    assert L.thallo_hip_incidence_count(ct.data_ptr(), n, 49, sb, sc, npix, pptr, tptr, None) == sk.INVALID
