"""The energy-independent PCG / LM chain of csrc/pcg_kernels.hip, kernel by kernel against the float64 references of tests/shim_kernels.py.

Every kernel runs in two input regimes.  EXACT: integers in [-8, 8], preconditioner entries from {1/4, 1/2, 1, 2}, scalar sums that make alpha = 3/4 and beta = -5/8:
every product and sum is exact in float32 whatever the order or fma contraction (asserted on the CPU first), so the device must EQUAL the reference -- this regime carries
the indexing, tail, range, grid-stride, gate and guard checks.  ROUNDED: standard_normal * 10^U{-3..3}; outputs within k 2^-24 sum|terms| of float64 (k = the number of
roundings, stated per test), per-workgroup partials within (c + 1) 2^-24 sum|terms| of the float64 dot of the device's own outputs (c = sk.chain_length: 4 adds per
float4 a lane visits + 6 butterfly levels + 4 waves; + 1 for the product).  alpha and beta come bit-exactly from sk.sum_partials / sk.div32 in both regimes.

Vectors are padded (sk.DVec): payload, zeros up to the next multiple of 4, then a NaN canary that is compared as bytes after every call; `const` inputs must come back
bit-unchanged; a launcher that returns its grid is held to sk.flat_grid and its partials buffer to exactly that many written slots."""
import numpy as np
import pytest

import shim_kernels as sk
from shim_kernels import F32

pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4 * 256 * 31, 4 * 256 * 32 + 4, 4 * 256 * 33, "ragged"]
COUNTS = [1, 5, 64, 65, 1024]
REGIMES = ["exact", "rounded"]
PSLOTS = sk.MAX_PARTIALS + 8


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    return sk.shim()


@pytest.fixture(scope="module")
def cus(L):
    return L.thallo_hip_device_cu_count()


def _n(n, cus):
    """'ragged': the first length at which the grid-stride loop takes a ragged second pass -- every workgroup one full pass, then 300 float4 and one float more"""
    return 4 * 256 * sk.flat_grid(10 ** 9, cus) + 4 * 300 + 1 if n == "ragged" else n


class Env:
    """one test case's inputs: vectors by regime, scalar sums, the bookkeeping of what must stay unchanged"""

    def __init__(self, torch, L, cus, n, regime, seed):
        self.torch, self.L, self.cus, self.n, self.regime = torch, L, cus, n, regime
        self.rng = np.random.default_rng([seed, n, regime == "exact"])
        self.c4 = sk.ceil4(n)
        self.grid = sk.flat_grid(self.c4 // 4, cus)
        self.const, self.all = [], []
        assert L.thallo_hip_vector_elems(n) == (n + 255) // 256 * 256

    def vec(self, const=False, kind="vec", payload=None):
        if payload is None:
            ex = self.regime == "exact"
            payload = {"vec": sk.exact_vec if ex else sk.rounded_vec, "pre": sk.exact_pre if ex else sk.rounded_pre}[kind](self.rng, self.n)
        v = sk.DVec(self.torch, self.n, payload)
        v.f = v.h0[:v.c4].astype(np.float64)
        self.all.append(v)
        if const: self.const.append(v)
        return v

    def out(self):
        v = sk.DVec(self.torch, self.n)
        self.all.append(v)
        return v

    def sums(self, idx, lm=False, targets=(12.0, 16.0, -7.5)):
        """alphaN, alphaD, betaN as thallo_sum_t of rotating counts; exact: alpha = 3/4, beta = -5/8.  Sets .alpha / .beta as the kernels form them."""
        cnt = [COUNTS[(idx + j) % len(COUNTS)] for j in range(3)]
        if self.regime == "exact": parts = [sk.exact_sum(self.rng, cnt[j], targets[j]) for j in range(3)]
        else: parts = [sk.rounded_sum(self.rng, cnt[j], positive=True) for j in range(3)]
        return self.sums_from(parts, lm)

    def sums_from(self, parts, lm=False):
        self.parts = [np.asarray(p, F32) for p in parts]
        self.sum_t = [sk.dbuf(self.torch, p) for p in self.parts]
        self.aN, self.aD, self.bN = (sk.sum_partials(p) for p in self.parts)
        self.alpha = sk.div32(self.aN, self.aD, guard=not lm)
        self.beta = sk.div32(self.bN, self.aN, guard=not lm)
        return [sk.sumt(t) for t in self.sum_t]

    def pbuf(self):
        return sk.canary_buf(self.torch, PSLOTS)

    def finish(self):
        self.torch.cuda.synchronize()
        for v in self.const: assert v.unchanged(), "a const input changed"
        for v in self.all: assert v.canary_ok(), "the canary behind a vector changed"
        for t, p in zip(self.sum_t, self.parts): assert sk.same_bytes(t.cpu().numpy(), p)

    def check(self, v, want, k, scale):
        """a vector output over [0, ceil4(n)): equal in the exact regime, within k 2^-24 scale of float64 in the rounded one"""
        got = v.body()
        want = np.asarray(want, np.float64)
        if self.regime == "exact":
            assert (want == want.astype(F32)).all(), "the reference is not exact in float32"
            assert np.array_equal(got, want.astype(F32)), np.flatnonzero(got != want.astype(F32))[:8]
        else:
            err = np.abs(got.astype(np.float64) - want)
            bound = sk.tol(k, scale)
            assert (err <= bound).all(), (np.flatnonzero(err > bound)[:8], (err / np.maximum(bound, 1e-300)).max())

    def check_partials(self, buf, ret, ref_terms, dev_terms, lsb, extra=0, blk=None, grid=None):
        """the returned grid, exactly that many written slots, and every partial: equal (exact) or within (c + 1 + extra) 2^-24 sum|terms| of the float64 dot"""
        grid = self.grid if grid is None else grid
        assert ret == grid, (ret, grid)
        host = buf.cpu().numpy()
        assert sk.written_slots(host) == grid
        if self.regime == "exact":
            sk.assert_exact_sums(ref_terms, grid, lsb, blk)
            assert np.array_equal(host[:grid], sk.block_sums(ref_terms, grid, blk).astype(F32))
        else:
            c = sk.chain_length(len(dev_terms), grid)
            want = sk.block_sums(dev_terms, grid, blk)
            bound = sk.tol(c + 1 + extra, sk.block_sums(np.abs(dev_terms), grid, blk))
            assert (np.abs(host[:grid].astype(np.float64) - want) <= bound).all()
        return host[:grid]


def f64(v):
    return v.body().astype(np.float64)


def absd(*xs):
    return [np.abs(np.asarray(x, np.float64)) for x in xs]


# ------------------------------------------------------------------ PCGStep2, fused and reference-shaped
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("idx,n", list(enumerate(LENGTHS)))
def test_pcg_step2(torch, L, cus, idx, n, regime):
    """r -= alpha Ap (k = 2: product, subtraction; terms |r|, |alpha Ap|); z = pre r (k = 3: r's two and the product; scale |pre| (|r| + |alpha Ap|));
    betaN partials = sum z.r."""
    for has_pre in (True, False):
        e = Env(torch, L, cus, _n(n, cus), regime, 1)
        r, Ap, z = e.vec(), e.vec(const=True), e.out()
        pre = e.vec(const=True, kind="pre") if has_pre else None
        aN, aD, _ = e.sums(idx + has_pre)
        pb = e.pbuf()
        ret = L.thallo_hip_pcg_step2(r.ptr, Ap.ptr, pre.ptr if pre else None, z.ptr, e.n, aN, aD, pb.data_ptr(), None)
        e.finish()
        r1, z1, bn = sk.ref_step2(r.f, Ap.f, pre.f if pre else None, e.alpha)
        s = np.abs(r.f) + np.abs(float(e.alpha) * Ap.f)
        e.check(r, r1, 2, s); e.check(z, z1, 3, (np.abs(pre.f) if pre else 1.0) * s)
        e.check_partials(pb, ret, bn, f64(z) * f64(r), 2.0 ** -6)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("idx,n", list(enumerate(LENGTHS)))
def test_pcg_step2_full(torch, L, cus, idx, n, regime):
    """As pcg_step2 plus delta += alpha p (k = 2; |delta|, |alpha p|) and, with b, the q partials of 0.5 delta.(r + b): one more rounding per term for (r + b)
    (extra = 1; the factor 0.5 is exact).  Every pre / lm / b instantiation; the LM ones divide unguarded, which changes nothing while alphaD != 0."""
    big = n == "ragged"
    for has_pre, lm, has_b in [(p, l, b) for p in (True, False) for l in (0, 1) for b in (True, False)]:
        if big and (has_pre, lm, has_b) not in ((True, 1, True), (False, 0, False)): continue       # (the ragged second pass once per kernel shape: with and without q)
        e = Env(torch, L, cus, _n(n, cus), regime, 2)
        delta, p, r, Ap, z = e.vec(), e.vec(const=True), e.vec(), e.vec(const=True), e.out()
        pre = e.vec(const=True, kind="pre") if has_pre else None
        b = e.vec(const=True) if has_b else None
        aN, aD, _ = e.sums(idx + has_pre + 2 * lm, lm=bool(lm))
        pb, qb = e.pbuf(), e.pbuf()
        ret = L.thallo_hip_pcg_step2_full(delta.ptr, p.ptr, r.ptr, Ap.ptr, pre.ptr if pre else None, z.ptr, b.ptr if b else None, e.n, aN, aD,
                                          pb.data_ptr(), qb.data_ptr() if b else None, lm, None)
        e.finish()
        d1, r1, z1, bn, q = sk.ref_step2_full(delta.f, p.f, r.f, Ap.f, pre.f if pre else None, b.f if b else None, e.alpha)
        s = np.abs(r.f) + np.abs(float(e.alpha) * Ap.f)
        e.check(delta, d1, 2, np.abs(delta.f) + np.abs(float(e.alpha) * p.f))
        e.check(r, r1, 2, s); e.check(z, z1, 3, (np.abs(pre.f) if pre else 1.0) * s)
        e.check_partials(pb, ret, bn, f64(z) * f64(r), 2.0 ** -6)
        if b:
            e.check_partials(qb, ret, q, 0.5 * f64(delta) * (f64(r) + b.f), 2.0 ** -5, extra=1)
        else:
            assert sk.written_slots(qb.cpu().numpy()) == 0


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("idx,n", list(enumerate(LENGTHS)))
def test_pcg_step3_and_pupdate(torch, L, cus, idx, n, regime):
    """p = z + beta p (k = 2: product, addition; |z|, |beta p|); pupdate: the same into p_out and delta += alpha p_in (k = 2), first: p_out = z and delta untouched,
    delta == NULL: the LM p update (unguarded divide)."""
    for lm in (0, 1):
        e = Env(torch, L, cus, _n(n, cus), regime, 3)
        p, z = e.vec(), e.vec(const=True)
        aN, _, bN = e.sums(idx + lm, lm=bool(lm))
        ret = L.thallo_hip_pcg_step3(p.ptr, z.ptr, e.n, bN, aN, lm, None)
        e.finish()
        assert ret == e.grid
        e.check(p, sk.ref_step3(p.f, z.f, e.beta), 2, np.abs(z.f) + np.abs(float(e.beta) * p.f))
    for first, with_delta in ((0, True), (1, True), (0, False), (1, False)):
        e = Env(torch, L, cus, _n(n, cus), regime, 4)
        z, p_in, p_out = e.vec(const=True), e.vec(const=True), e.out()
        delta = e.vec(const=bool(first)) if with_delta else None
        aN, aD, bN = e.sums(idx + first, lm=not with_delta)
        ret = L.thallo_hip_pcg_pupdate(z.ptr, p_in.ptr, p_out.ptr, delta.ptr if delta else None, e.n, first, aN, aD, bN, None)
        e.finish()
        assert ret == e.grid
        po, d1 = sk.ref_pupdate(z.f, p_in.f, delta.f if delta else None, e.alpha, e.beta, first)
        e.check(p_out, po, 2, np.abs(z.f) + np.abs(float(e.beta) * p_in.f))
        if delta and not first: e.check(delta, d1, 2, np.abs(delta.f) + np.abs(float(e.alpha) * p_in.f))


# ------------------------------------------------------------------ the single-reduction form
def _s3(e, nb):
    """alphaD partials (float) and {N, S1, S2} partials (double) of `nb` workgroups.  Exact: alphaD = 16; N, S1, S2 = 12, 8, 16 -> betaN = 12 - 12 + 9 = 9 with
    alpha = 3/4, and beta = 9 / 12 = 3/4.  Rounded: positive sums with N dominating (2 alpha S1 <= N / 2 cannot be arranged for a random alpha, so the test reads the condition number)."""
    if e.regime == "exact":
        ad = sk.exact_sum(e.rng, nb, 16.0)
        s3 = np.stack([sk.exact_sum(e.rng, nb, t).astype(np.float64) for t in (12.0, 8.0, 16.0)], axis=1)
    else:
        ad = sk.rounded_sum(e.rng, nb, positive=True)
        s3 = np.abs(e.rng.standard_normal((nb, 3)) * 10.0 ** e.rng.integers(-3, 4, (nb, 3)))
    return ad, np.ascontiguousarray(s3)


def _check_bn_word(got, want, mag):
    """betaN = N - 2 alpha S1 + alpha^2 S2: 1 float ulp.  The double expression may be contracted (each of its <= 5 roundings <= 2^-53 sum|terms|), which stays far below
    half a float ulp of the result as long as sum|terms| / |result| < 2^20 -- read off the inputs here, not assumed."""
    if float(want) > 0: assert mag / float(want) < 2.0 ** 20
    assert sk.ulp_apart(got, want) <= 1, (got, want)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("idx,n", list(enumerate(LENGTHS)))
def test_pcg_update_and_its_fused_finish(torch, L, cus, idx, n, regime):
    """thallo_hip_pcg_update: r = fma(-alpha, Ap, r) and delta = fma(alpha, p_in, delta) (k = 1 each); p_out = pre r + beta p_in (k = 4: r's one, pre r, beta p_in, the sum;
    scale |pre| (|r| + |alpha Ap|) + |beta p_in|); first = 1: p_out = pre r, r and delta untouched.  thallo_hip_pcg_update_lm: the same with unguarded divides, first = 2:
    p_out only, betaN left in betaN_word.  thallo_hip_pcg_update_fin with the partials of `nb` workgroups: its two words bitwise those of thallo_hip_pcg_scalars_finish,
    alphaD bit-exact and betaN to 1 ulp against the helper; its vectors as pcg_update with alpha = alphaN / alphaD, beta = betaN / alphaN."""
    nn = _n(n, cus)

    def run(kind, has_pre, first, nb=None):
        e = Env(torch, L, cus, nn, regime, 5)
        r, Ap, p_in, p_out, delta = e.vec(const=first != 0), e.vec(const=True), e.vec(const=True), e.out(), e.vec(const=first != 0)
        pre = e.vec(const=True, kind="pre") if has_pre else None
        aN, aD, bN = e.sums(idx + first, lm=kind == "lm")
        alpha, beta = e.alpha, e.beta
        if kind == "plain":
            ret = L.thallo_hip_pcg_update(r.ptr, Ap.ptr, pre.ptr if pre else None, p_in.ptr, p_out.ptr, delta.ptr, nn, first, aN, aD, bN, None)
        elif kind == "lm":
            state = sk.dbuf(torch, np.zeros(8, F32)); word = sk.canary_buf(torch, 2)
            ret = L.thallo_hip_pcg_update_lm(r.ptr, Ap.ptr, pre.ptr, p_in.ptr, p_out.ptr, delta.ptr, nn, first, aN, aD, bN, word.data_ptr(), state.data_ptr(), None)
        else:
            ad, s3 = _s3(e, nb)
            adt, s3t = sk.dbuf(torch, ad), sk.dbuf(torch, s3)
            w = sk.canary_buf(torch, 4)
            ret = L.thallo_hip_pcg_update_fin(r.ptr, Ap.ptr, pre.ptr if pre else None, p_in.ptr, p_out.ptr, delta.ptr, nn, aN, adt.data_ptr(), s3t.data_ptr(), nb,
                                              w.data_ptr(), w.data_ptr() + 4, None)
            assert L.thallo_hip_pcg_scalars_finish(adt.data_ptr(), s3t.data_ptr(), nb, aN, w.data_ptr() + 8, w.data_ptr() + 12, None) == 0
        e.finish()
        assert ret == 0
        if kind == "lm":
            wh = word.cpu().numpy()
            if first != 1: assert sk.same_bytes(wh[:1], e.bN)
            else: assert sk.written_slots(wh) == 0
            assert sk.same_bytes(state.cpu().numpy(), np.zeros(8, F32))
        if kind == "fin":
            wh = w.cpu().numpy()
            assert sk.same_bytes(wh[0:2], wh[2:4]), wh                          # "same order, same bits"
            adw, alpha, bnw, mag = sk.ref_scalars_finish(ad, s3, e.aN)
            assert sk.same_bytes(wh[0:1], adw)
            _check_bn_word(wh[1], bnw, mag)
            beta = sk.div32(wh[1], e.aN, True)                                  # (the vectors follow the word the device formed)
            assert sk.same_bytes(adt.cpu().numpy(), ad) and sk.same_bytes(s3t.cpu().numpy(), s3)
        r1, po, d1 = sk.ref_pcg_update(r.f, Ap.f, pre.f if pre else None, p_in.f, delta.f, alpha, beta, first)
        m = np.abs(pre.f) if pre else 1.0
        if first == 0:
            e.check(r, r1, 1, np.abs(r.f) + np.abs(float(alpha) * Ap.f)); e.check(delta, d1, 1, np.abs(delta.f) + np.abs(float(alpha) * p_in.f))
            e.check(p_out, po, 4, m * (np.abs(r.f) + np.abs(float(alpha) * Ap.f)) + np.abs(float(beta) * p_in.f))
        else:
            e.check(p_out, po, 3, m * np.abs(r.f) + (np.abs(float(beta) * p_in.f) if first == 2 else 0.0))

    for has_pre in (True, False):
        for first in (0, 1): run("plain", has_pre, first)
    for first in (0, 1, 2): run("lm", True, first)
    for has_pre in (True, False): run("fin", has_pre, 0, nb=COUNTS[(idx + has_pre) % 5])


@pytest.mark.parametrize("nb", COUNTS)
def test_pcg_scalars_finish_clamps_and_guards(torch, L, nb):
    """betaN is clamped to 0 when the expression is <= 0; alphaD = 0: alpha = 0 and betaN = N; alphaN = 0: alpha = 0."""
    rng = np.random.default_rng(nb)
    for ad_t, s3_t, an in ((16.0, (1.0, 8.0, 4.0), 12.0), (0.0, (40.0, 8.0, 4.0), 12.0), (16.0, (40.0, 8.0, 4.0), 0.0)):
        ad = sk.exact_sum(rng, nb, ad_t)
        s3 = np.ascontiguousarray(np.stack([sk.exact_sum(rng, nb, t).astype(np.float64) for t in s3_t], axis=1))
        adt, s3t, ant, w = sk.dbuf(torch, ad), sk.dbuf(torch, s3), sk.dbuf(torch, np.array([an], F32)), sk.canary_buf(torch, 2)
        assert L.thallo_hip_pcg_scalars_finish(adt.data_ptr(), s3t.data_ptr(), nb, sk.sumt(ant), w.data_ptr(), w.data_ptr() + 4, None) == 0
        torch.cuda.synchronize()
        adw, alpha, bnw, _ = sk.ref_scalars_finish(ad, s3, F32(an))
        assert sk.same_bytes(w.cpu().numpy(), np.array([adw, bnw], F32)), (w.cpu().numpy(), adw, bnw)
    assert float(bnw) == 40.0


# ------------------------------------------------------------------ the LM set and PCGInit1_Finish
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("idx,n", list(enumerate(LENGTHS)))
def test_lm_vector_kernels(torch, L, cus, idx, n, regime):
    """lm_step1_finish: Ap += CtC p (k = 2; |Ap|, |CtC p|), alphaD partials p.Ap.  lm_step2_first_half: delta += alpha p (k = 2), unguarded divide.
    lm_step2_second_half: r = b - Adelta (k = 1), z = pre r (k = 2; |pre| (|b| + |Adelta|)), betaN partials z.r, q partials 0.5 delta.(r + b) (extra = 1)."""
    nn = _n(n, cus)
    e = Env(torch, L, cus, nn, regime, 6)
    Ap, CtC, p = e.vec(), e.vec(const=True, kind="pre"), e.vec(const=True)
    e.sums(idx); pb = e.pbuf()
    ret = L.thallo_hip_lm_step1_finish(Ap.ptr, CtC.ptr, p.ptr, nn, pb.data_ptr(), None)
    e.finish()
    a1, t = sk.ref_lm_step1_finish(Ap.f, CtC.f, p.f)
    e.check(Ap, a1, 2, np.abs(Ap.f) + np.abs(CtC.f * p.f))
    e.check_partials(pb, ret, t, p.f * f64(Ap), 2.0 ** -2)

    e = Env(torch, L, cus, nn, regime, 7)
    delta, p = e.vec(), e.vec(const=True)
    aN, aD, _ = e.sums(idx, lm=True)
    ret = L.thallo_hip_lm_step2_first_half(delta.ptr, p.ptr, nn, aN, aD, None)
    e.finish()
    assert ret == e.grid
    e.check(delta, sk.ref_lm_step2_first(delta.f, p.f, e.alpha), 2, np.abs(delta.f) + np.abs(float(e.alpha) * p.f))

    e = Env(torch, L, cus, nn, regime, 8)
    r, z = e.out(), e.out()
    b, Ad, pre, delta = e.vec(const=True), e.vec(const=True), e.vec(const=True, kind="pre"), e.vec(const=True)
    e.sums(idx); pb, qb = e.pbuf(), e.pbuf()
    ret = L.thallo_hip_lm_step2_second_half(r.ptr, b.ptr, Ad.ptr, pre.ptr, z.ptr, delta.ptr, nn, pb.data_ptr(), qb.data_ptr(), None)
    e.finish()
    r1, z1, bn, q = sk.ref_lm_step2_second(b.f, Ad.f, pre.f, delta.f)
    s = np.abs(b.f) + np.abs(Ad.f)
    e.check(r, r1, 1, s); e.check(z, z1, 2, np.abs(pre.f) * s)
    e.check_partials(pb, ret, bn, f64(z) * f64(r), 2.0 ** -2)
    e.check_partials(qb, ret, q, 0.5 * delta.f * (f64(r) + b.f), 2.0 ** -1, extra=1)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("idx,n", list(enumerate(LENGTHS)))
def test_init_finish_and_lm_finalize_diagonal(torch, L, cus, idx, n, regime):
    """pcg_init_finish: pre = 1 / (1 + sqrt(d))^2 -- sqrt, the sum, the square, the division and their propagation: k = 6 relative to pre; z = pre r (k = 7); alphaN
    partials r.z.  Exact regime: d from {0, 1, 9, 49}, so that pre is 1, 1/4, 1/16, 1/64.
    lm_finalize_diagonal: SSq as pre above (k = 6); CtC = clamp(d / radius, min / (SSq radius), max / (SSq radius)): 1 / radius and the product (2), or 1 / SSq (SSq's 6 + 1),
    / radius, * min: k = 9; pre = 1 / (CtC + radius (d / radius)): the larger of the two (9) + the sum + the division: k = 11; z = pre r: k = 12.  All relative to the
    reference value (every quantity is a product / quotient of positives or a sum of positives: no cancellation).  Exact regime: radius = 1 and d from {0, 1} with the
    preconditioner, {0, 1, 2, 4} without (min, max = 1/4, 4), so that every quotient is a power of two."""
    nn = _n(n, cus)
    ex = regime == "exact"
    for usep in (1, 0):
        e = Env(torch, L, cus, nn, regime, 9)
        d = e.rng.choice(np.array([0.0, 1.0, 9.0, 49.0], F32), nn) if ex else np.abs(sk.rounded_vec(e.rng, nn))
        r, diag, pre, z = e.vec(const=True), e.vec(const=True, payload=d), e.out(), e.out()
        e.sums(idx); pb = e.pbuf()
        ret = L.thallo_hip_pcg_init_finish(r.ptr, diag.ptr if usep or idx % 2 else None, pre.ptr, z.ptr, nn, usep, pb.data_ptr(), None)
        e.finish()
        m, z1, t = sk.ref_init_finish(r.f, diag.f, usep)
        e.check(pre, m, 6, m); e.check(z, z1, 7, np.abs(z1))
        e.check_partials(pb, ret, t, r.f * f64(z), 2.0 ** -6)
    for usep, save in ((1, 1), (0, 1), (1, 0)):
        e = Env(torch, L, cus, nn, regime, 10)
        if ex:
            d = e.rng.choice(np.array([0.0, 1.0], F32) if usep else np.array([0.0, 1.0, 2.0, 4.0], F32), nn)
            ssq_in = sk.guarded_invert(d).astype(F32)
            radius, mn, mx = 1.0, 0.25, 4.0
        else:
            d = np.abs(sk.rounded_vec(e.rng, nn))
            ssq_in = e.rng.uniform(0.01, 1.0, nn).astype(F32)
            radius, mn, mx = 30.0, 1e-6, 1e32
        diag, r = e.vec(const=True, payload=d), e.vec(const=True)
        SSq = e.out() if save else e.vec(const=True, payload=ssq_in)
        CtC, pre, b, z = e.out(), e.out(), e.out(), e.out()
        e.sums(idx); pb = e.pbuf()
        ret = L.thallo_hip_lm_finalize_diagonal(diag.ptr, SSq.ptr, CtC.ptr, pre.ptr, r.ptr, b.ptr, z.ptr, nn, radius, mn, mx, save, usep, pb.data_ptr(), None)
        e.finish()
        if not save and ex:
            pad = SSq.f.copy(); pad[nn:] = 1.0      # (the zero padding of an SSq that is an input would divide by zero in the reference only)
        s1, c1, m1, b1, z1, t = sk.ref_lm_finalize(diag.f, None if save else (pad if ex else np.where(SSq.f == 0, 1.0, SSq.f)), r.f, radius, mn, mx, save, usep)
        body = slice(0, nn)
        if save: e.check(SSq, s1, 6, s1)
        for v, want, k in ((CtC, c1, 9), (pre, m1, 11), (z, z1, 12)):
            got = v.body()[body]
            if ex: assert np.array_equal(got, want[body].astype(F32)) and (want[body] == want[body].astype(F32)).all()
            else: assert (np.abs(got - want[body]) <= sk.tol(k, np.abs(want[body]))).all()
        assert np.array_equal(b.body(), r.body())
        zz = np.zeros(e.c4); zz[body] = f64(z)[body]
        tt = np.zeros(e.c4); tt[body] = t[body]
        e.check_partials(pb, ret, tt, r.f * zz, 2.0 ** -3)


# ------------------------------------------------------------------ two ranges of a flat vector
RANGES = [(8, 40, 0, 0), (0, 0, 16, 24), (4, 4, 12, 4), (8, 512, 520, 1028), (0, 300, 1200, 1100)]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("idx,rg", list(enumerate(RANGES)))
def test_two_range_forms(torch, L, cus, idx, rg, regime):
    """pcg_step2_ranges / pcg_pupdate_ranges over [off0, off0 + len0) U [off1, off1 + len1): len1 = 0, len0 = 0, both 4, adjacent, a gap.  Inside: the one-range kernels'
    results (same k); outside: bit-untouched; the partials follow the concatenated index j (float4 j -> workgroup (j / 256) % grid)."""
    off0, len0, off1, len1 = rg
    n = 2400
    idxs = np.concatenate([np.arange(off0, off0 + len0), np.arange(off1, off1 + len1)])
    grid = sk.flat_grid((len0 + len1) // 4, cus)
    blk = sk.block_of(len0 + len1, grid)
    e = Env(torch, L, cus, n, regime, 11)
    r, Ap, pre = e.vec(), e.vec(const=True), e.vec(const=True, kind="pre")
    z = e.vec()                                         # (an in/out buffer here: what lies outside the ranges must survive)
    aN, aD, bN = e.sums(idx)
    pb = e.pbuf()
    ret = L.thallo_hip_pcg_step2_ranges(r.ptr, Ap.ptr, pre.ptr, z.ptr, off0, len0, off1, len1, aN, aD, pb.data_ptr(), None)
    e.finish()
    r1, z1, bn = sk.ref_step2(r.f, Ap.f, pre.f, e.alpha)
    inside = np.zeros(e.c4, bool); inside[idxs] = True
    rw = np.where(inside, r1, r.f); zw = np.where(inside, z1, z.f)
    s = np.abs(r.f) + np.abs(float(e.alpha) * Ap.f)
    e.check(r, rw, 2, s); e.check(z, zw, 3, np.abs(pre.f) * s)
    assert sk.same_bytes(r.body()[~inside], r.h0[:e.c4][~inside]) and sk.same_bytes(z.body()[~inside], z.h0[:e.c4][~inside])
    e.check_partials(pb, ret, bn[idxs], (f64(z) * f64(r))[idxs], 2.0 ** -6, blk=blk, grid=grid)

    e = Env(torch, L, cus, n, regime, 12)
    zz, p_in, p_out, delta = e.vec(const=True), e.vec(const=True), e.vec(), e.vec()
    aN, aD, bN = e.sums(idx + 1)
    ret = L.thallo_hip_pcg_pupdate_ranges(zz.ptr, p_in.ptr, p_out.ptr, delta.ptr, off0, len0, off1, len1, 0, aN, aD, bN, None)
    e.finish()
    assert ret == grid
    po, d1 = sk.ref_pupdate(zz.f, p_in.f, delta.f, e.alpha, e.beta, 0)
    e.check(p_out, np.where(inside, po, p_out.f), 2, np.abs(zz.f) + np.abs(float(e.beta) * p_in.f))
    e.check(delta, np.where(inside, d1, delta.f), 2, np.abs(delta.f) + np.abs(float(e.alpha) * p_in.f))
    assert sk.same_bytes(p_out.body()[~inside], p_out.h0[:e.c4][~inside]) and sk.same_bytes(delta.body()[~inside], delta.h0[:e.c4][~inside])


@pytest.mark.parametrize("bad", [(2, 8, 16, 8), (0, 6, 16, 8), (0, 8, 17, 8), (0, 8, 16, 3)])
def test_two_range_forms_refuse_misaligned_ranges(torch, L, cus, bad):
    """offsets / lengths that are no multiples of 4: -hipErrorInvalidValue and nothing is launched (every buffer keeps its bytes)"""
    e = Env(torch, L, cus, 64, "exact", 13)
    r, Ap, pre, z, delta = e.vec(const=True), e.vec(const=True), e.vec(const=True, kind="pre"), e.vec(const=True), e.vec(const=True)
    aN, aD, bN = e.sums(0)
    pb = e.pbuf()
    assert L.thallo_hip_pcg_step2_ranges(r.ptr, Ap.ptr, pre.ptr, z.ptr, *bad, aN, aD, pb.data_ptr(), None) == sk.INVALID
    assert L.thallo_hip_pcg_pupdate_ranges(z.ptr, Ap.ptr, r.ptr, delta.ptr, *bad, 0, aN, aD, bN, None) == sk.INVALID
    e.finish()
    assert sk.written_slots(pb.cpu().numpy()) == 0


# ------------------------------------------------------------------ the guards
@pytest.mark.parametrize("count", COUNTS)
def test_zero_denominators(torch, L, cus, count):
    """alphaD = 0 in the non-LM kernels: alpha = 0 -- r and delta bitwise unchanged; alphaN = 0: beta = 0 -- p = z.  thallo_hip_alpha_beta reports both.  The LM
    instantiations divide blindly (thallo_hip.h: `lm selects the unguarded divide`): alpha = +-inf, and the outputs are non-finite exactly where the reference's are."""
    n = 1025
    rng = np.random.default_rng(count)
    zero, some = sk.exact_sum(rng, count, 0.0), sk.exact_sum(rng, count, 12.0)

    def env(parts, lm=False):
        e = Env(torch, L, cus, n, "exact", 14 + count)
        return e, e.sums_from(parts, lm)
    # alphaD == 0
    e, (aN, aD, bN) = env([some, zero, some])
    assert e.alpha == 0 and e.beta == 1
    r, Ap, pre, z, delta, p = e.vec(const=True), e.vec(const=True), e.vec(const=True, kind="pre"), e.out(), e.vec(const=True), e.vec(const=True)
    pb = e.pbuf()
    assert L.thallo_hip_pcg_step2(r.ptr, Ap.ptr, pre.ptr, z.ptr, n, aN, aD, pb.data_ptr(), None) == e.grid
    assert L.thallo_hip_pcg_step2_full(delta.ptr, p.ptr, r.ptr, Ap.ptr, pre.ptr, z.ptr, None, n, aN, aD, pb.data_ptr(), None, 0, None) == e.grid
    X = e.vec();
    assert L.thallo_hip_linear_update(X.ptr, delta.ptr, p.ptr, n, aN, aD, None) == sk.flat_grid(n, cus)
    w = sk.canary_buf(torch, 2)
    assert L.thallo_hip_alpha_beta(aN, aD, bN, w.data_ptr(), None) == 0
    e.finish()
    assert np.array_equal(z.body(), (pre.f * r.f).astype(F32)) and np.array_equal(X.body()[:n], (X.f + delta.f)[:n].astype(F32))
    assert sk.same_bytes(w.cpu().numpy(), np.array([0.0, 1.0], F32))
    e, (aN, aD, bN) = env([some, zero, some])
    r, Ap, pre, p_in, p_out, delta = e.vec(const=True), e.vec(const=True), e.vec(const=True, kind="pre"), e.vec(const=True), e.out(), e.vec(const=True)
    assert L.thallo_hip_pcg_update(r.ptr, Ap.ptr, pre.ptr, p_in.ptr, p_out.ptr, delta.ptr, n, 0, aN, aD, bN, None) == 0
    zz = e.vec(const=True); po2 = e.out()
    assert L.thallo_hip_pcg_pupdate(zz.ptr, p_in.ptr, po2.ptr, delta.ptr, n, 0, aN, aD, bN, None) == e.grid
    e.finish()
    assert np.array_equal(p_out.body(), (pre.f * r.f + p_in.f).astype(F32)) and np.array_equal(po2.body(), (zz.f + p_in.f).astype(F32))
    # alphaN == 0
    e, (aN, aD, bN) = env([zero, some, some])
    assert e.alpha == 0 and e.beta == 0
    p, z = e.vec(), e.vec(const=True)
    assert L.thallo_hip_pcg_step3(p.ptr, z.ptr, n, bN, aN, 0, None) == e.grid
    w = sk.canary_buf(torch, 2)
    assert L.thallo_hip_alpha_beta(aN, aD, bN, w.data_ptr(), None) == 0
    e.finish()
    assert np.array_equal(p.body(), z.body()) and sk.same_bytes(w.cpu().numpy(), np.zeros(2, F32))
    # LM: blind division
    e, (aN, aD, bN) = env([some, zero, some], lm=True)
    assert np.isinf(e.alpha)
    delta, p, r, Ap, pre, z, b = e.vec(), e.vec(const=True), e.vec(), e.vec(const=True), e.vec(const=True, kind="pre"), e.out(), e.vec(const=True)
    pb, qb = e.pbuf(), e.pbuf()
    assert L.thallo_hip_pcg_step2_full(delta.ptr, p.ptr, r.ptr, Ap.ptr, pre.ptr, z.ptr, b.ptr, n, aN, aD, pb.data_ptr(), qb.data_ptr(), 1, None) == e.grid
    e.finish()
    d1, r1, z1, _, _ = sk.ref_step2_full(delta.f, p.f, r.f, Ap.f, pre.f, b.f, e.alpha)
    for v, want in ((delta, d1), (r, r1), (z, z1)):
        assert np.array_equal(np.isfinite(v.body()[:n]), np.isfinite(want[:n])) and not np.isfinite(want[:n]).all()
        fin = np.isfinite(want[:n])
        assert np.array_equal(v.body()[:n][fin], want[:n][fin].astype(F32))
    e, (aN, aD, bN) = env([zero, some, some], lm=True)
    p, z = e.vec(), e.vec(const=True)
    assert L.thallo_hip_pcg_step3(p.ptr, z.ptr, n, bN, aN, 1, None) == e.grid
    e.finish()
    want = sk.ref_step3(p.f, z.f, e.beta)
    assert np.array_equal(np.isfinite(p.body()[:n]), np.isfinite(want[:n])) and not np.isfinite(want[:n]).any()


# ------------------------------------------------------------------ the zeta test on the device
ZETA_CASES = {   # name: (Q0, q target (exact sum), k, tolerance)
    "continues": (-1.0, -3.0, 2, 0.5), "tolerance": (-2.0, -2.5, 1, 0.5), "zero": (0.0, 0.0, 4, 0.0), "frozen": (1.0, 5.0, 7, 0.0),
}


def _state(Q0, frozen=0, its=0):
    s = np.zeros(8, F32); s[0] = Q0
    s.view(np.uint32)[1] = frozen; s.view(np.int32)[2] = its
    s[3:] = [3.5, 4.5, 5.5, 6.5, 7.5]
    return s


def _state_want(state0, new):
    s = state0.copy(); s[0] = new[0]; s.view(np.uint32)[1] = new[1]; s.view(np.int32)[2] = new[2]
    return s


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("case", list(ZETA_CASES) + ["inf"])
def test_lm_zeta(torch, L, case, count):
    """The loop continues (state[0] becomes Q1); stops by tolerance, on Q1 = 0 (0 / 0) and on Q1 = inf with state[1] = 1 and state[2] = k + 1; an already frozen state
    does not change.  Words 3..7 are the driver's and stay."""
    rng = np.random.default_rng(count)
    if case == "inf":
        Q0, k, tolr = 1.0, 0, 0.0
        q = sk.exact_sum(rng, count, 2.0); q[0] = np.inf
    else:
        Q0, tq, k, tolr = ZETA_CASES[case]
        q = sk.exact_sum(rng, count, tq)
    s0 = _state(Q0, *((1, 3) if case == "frozen" else (0, 0)))
    st, qt = sk.dbuf(torch, s0), sk.dbuf(torch, q)
    assert L.thallo_hip_lm_zeta(sk.sumt(qt), k, tolr, st.data_ptr(), None) == 0
    torch.cuda.synchronize()
    new = sk.ref_lm_zeta((Q0, int(s0.view(np.uint32)[1]), int(s0.view(np.int32)[2])), sk.sum_partials(q), k, tolr)
    assert new[1] == (case != "continues")
    assert sk.same_bytes(st.cpu().numpy(), _state_want(s0, new)), (st.cpu().numpy(), new)
    z8 = sk.dbuf(torch, _state(9.0, 1, 4))
    assert L.thallo_hip_lm_state_reset(z8.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert sk.same_bytes(z8.cpu().numpy(), np.zeros(8, F32))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", ["continues", "tolerance", "zero", "inf", "frozen_go", "frozen_stop"])
@pytest.mark.parametrize("n", [5, 1025, 4 * 256 * 31, 4 * 256 * 32 + 4, 4 * 256 * 33, "ragged"])
def test_pcg_step2_full_zeta_is_step2_full_then_lm_zeta(torch, L, cus, n, case, regime):
    """One launch against two: every vector, both partial buffers and the 8 state words bitwise equal; the ticket words are all zero again.  31 / 32 / 33 workgroups
    straddle the two-level ticket.  The cases steer Q0 / the tolerance around the q the inputs produce; `zero`: delta = p = 0 so that q = 0; `inf`: one b entry is inf;
    `frozen_go` / `frozen_stop`: the state is frozen already (no gate installed, so the vector update runs in both forms) and its 8 words must stay as they are, whether
    the test on this launch's q would have let the loop go on or stopped it."""
    nn = _n(n, cus)
    outs = []
    for fused in (False, True):
        e = Env(torch, L, cus, nn, regime, 15)
        dl = np.zeros(nn, F32) if case == "zero" else None
        delta, p, r, Ap = e.vec(payload=dl), e.vec(const=True, payload=dl), e.vec(), e.vec(const=True)
        pre, z = e.vec(const=True, kind="pre"), e.out()
        bp = (sk.exact_vec if regime == "exact" else sk.rounded_vec)(e.rng, nn)
        if case == "inf": bp[nn // 2] = np.inf
        b = e.vec(const=True, payload=bp)
        aN, aD, _ = e.sums(2, lm=True)
        d1, r1, z1, bn, q = sk.ref_step2_full(delta.f, p.f, r.f, Ap.f, pre.f, b.f, e.alpha)
        Q1 = q.sum()
        k = 3
        was_frozen = case.startswith("frozen")
        Q0, tolr = {"continues": lambda: (Q1 - abs(Q1) - 1.0, -1e30), "tolerance": lambda: (Q1, 0.5), "zero": lambda: (0.0, 0.0), "inf": lambda: (1.0, 0.0)}[
            {"frozen_go": "continues", "frozen_stop": "tolerance"}.get(case, case)]()
        s0 = _state(Q0, 1, 2) if was_frozen else _state(Q0)
        st, pb, qb = sk.dbuf(torch, s0), e.pbuf(), e.pbuf()
        tickets = sk.dbuf(torch, np.zeros(528, np.uint32))
        if fused:
            ret = L.thallo_hip_pcg_step2_full_zeta(delta.ptr, p.ptr, r.ptr, Ap.ptr, pre.ptr, z.ptr, b.ptr, nn, aN, aD, pb.data_ptr(), qb.data_ptr(), tickets.data_ptr(), k, tolr,
                                                   st.data_ptr(), None)
        else:
            ret = L.thallo_hip_pcg_step2_full(delta.ptr, p.ptr, r.ptr, Ap.ptr, pre.ptr, z.ptr, b.ptr, nn, aN, aD, pb.data_ptr(), qb.data_ptr(), 1, None)
            assert L.thallo_hip_lm_zeta(sk.sumt(qb, ret), k, tolr, st.data_ptr(), None) == 0
        e.finish()
        assert ret == e.grid
        assert not tickets.cpu().numpy().any()
        sh = st.cpu().numpy()
        frozen = int(sh.view(np.uint32)[1])
        assert frozen == (case != "continues"), (case, sh, Q1)
        if was_frozen: assert sk.same_bytes(sh, s0), (sh, s0)
        elif frozen: assert int(sh.view(np.int32)[2]) == k + 1 and sh[0] == F32(Q0)
        else: assert sk.same_bytes(sh[:1], sk.sum_partials(qb.cpu().numpy()[:ret]))
        outs.append([v.get() for v in (delta, r, z)] + [pb.cpu().numpy(), qb.cpu().numpy(), sh])
    for a, bb in zip(*outs):
        assert sk.same_bytes(a, bb)


@pytest.mark.parametrize("n", [5, 4 * 256 * 33])
def test_pcg_step2_full_zeta_behind_the_gate(torch, L, cus, n):
    """The LM drivers install the state's word 1 as the gate (thallo_hip_lm_set_gate(state + 1)): once it is set the fused launch does nothing -- every vector, both
    partial buffers and the 8 state words keep their bytes, and the ticket words are still all zero."""
    e = Env(torch, L, cus, n, "exact", 22)
    delta, p, r, Ap, pre, z, b = e.vec(const=True), e.vec(const=True), e.vec(const=True), e.vec(const=True), e.vec(const=True, kind="pre"), e.out(), e.vec(const=True)
    aN, aD, _ = e.sums(1, lm=True)
    s0 = _state(-3.0, 1, 2)
    st, pb, qb, tickets = sk.dbuf(torch, s0), e.pbuf(), e.pbuf(), sk.dbuf(torch, np.zeros(528, np.uint32))
    try:
        L.thallo_hip_lm_set_gate(st.data_ptr() + 4)
        ret = L.thallo_hip_pcg_step2_full_zeta(delta.ptr, p.ptr, r.ptr, Ap.ptr, pre.ptr, z.ptr, b.ptr, n, aN, aD, pb.data_ptr(), qb.data_ptr(), tickets.data_ptr(), 3, 0.5,
                                               st.data_ptr(), None)
    finally:
        L.thallo_hip_lm_set_gate(None)
    e.finish()
    assert ret == e.grid and z.unchanged()
    assert sk.written_slots(pb.cpu().numpy()) == 0 and sk.written_slots(qb.cpu().numpy()) == 0
    assert sk.same_bytes(st.cpu().numpy(), s0) and not tickets.cpu().numpy().any()


# ------------------------------------------------------------------ the gate word
@pytest.mark.parametrize("word", [0, 1, 0x80000000])
def test_gate_word(torch, L, cus, word):
    """thallo_hip_lm_set_gate: with a non-zero word pcg_pupdate, lm_step1_finish, pcg_step2_full, both lm_step2 halves, pcg_update_lm (its state's word 1) and
    finish_sum_gated leave every buffer bit-untouched (outputs are canary-filled, partial buffers too); with a zero word they run.  The gate is ambient per thread:
    reset in a finally."""
    n = 1025
    e = Env(torch, L, cus, n, "exact", 16)
    gate = sk.dbuf(torch, np.array([word, 0], np.uint32))
    state = _state(2.0, word, 0); st = sk.dbuf(torch, state)
    ins = [e.vec(const=True) for _ in range(5)]; pre = e.vec(const=True, kind="pre")
    v = [e.vec(const=bool(word)) for _ in range(7)]          # in/out vectors: const exactly when gated
    free = e.vec()
    outs = [e.out() for _ in range(5)]
    pbs = [e.pbuf() for _ in range(7)]
    w = sk.canary_buf(torch, 4)
    aN, aD, bN = e.sums(1, lm=True)
    try:
        L.thallo_hip_lm_set_gate(gate.data_ptr())
        rets = [
            L.thallo_hip_pcg_pupdate(ins[0].ptr, ins[1].ptr, outs[0].ptr, v[0].ptr, n, 0, aN, aD, bN, None),
            L.thallo_hip_lm_step1_finish(v[1].ptr, pre.ptr, ins[0].ptr, n, pbs[0].data_ptr(), None),
            L.thallo_hip_pcg_step2_full(v[2].ptr, ins[0].ptr, v[3].ptr, ins[1].ptr, pre.ptr, outs[1].ptr, ins[2].ptr, n, aN, aD, pbs[1].data_ptr(), pbs[2].data_ptr(), 1, None),
            L.thallo_hip_lm_step2_first_half(v[4].ptr, ins[0].ptr, n, aN, aD, None),
            L.thallo_hip_lm_step2_second_half(outs[2].ptr, ins[0].ptr, ins[1].ptr, pre.ptr, outs[3].ptr, ins[2].ptr, n, pbs[3].data_ptr(), pbs[4].data_ptr(), None),
        ]
    finally:
        L.thallo_hip_lm_set_gate(None)
    assert L.thallo_hip_pcg_update_lm(v[5].ptr, ins[0].ptr, pre.ptr, ins[1].ptr, outs[4].ptr, v[6].ptr, n, 0, aN, aD, bN, w.data_ptr(), st.data_ptr(), None) == 0
    assert L.thallo_hip_finish_sum_gated(aN, w.data_ptr() + 4, gate.data_ptr(), None) == 0
    # without the ambient gate the same launch runs whatever the word says
    assert L.thallo_hip_lm_step2_first_half(free.ptr, ins[0].ptr, n, aN, aD, None) == e.grid
    e.finish()
    assert rets == [e.grid] * 5
    assert sk.same_bytes(st.cpu().numpy(), state) and sk.same_bytes(gate.cpu().numpy(), np.array([word, 0], np.uint32))
    wh = w.cpu().numpy()
    assert np.array_equal(free.body(), sk.ref_lm_step2_first(free.f, ins[0].f, e.alpha).astype(F32))            # (no gate installed: it ran)
    if word:
        for o in outs[:5]: assert o.unchanged()
        for pb in pbs: assert sk.written_slots(pb.cpu().numpy()) == 0
        assert sk.written_slots(wh) == 0
    else:
        for o in outs[:5]: assert not np.isnan(o.body()).any()
        for pb in pbs[:5]: assert sk.written_slots(pb.cpu().numpy()) == e.grid
        assert sk.same_bytes(wh[:2], np.array([e.bN, e.aN], F32))
        assert np.array_equal(outs[0].body(), sk.ref_pupdate(ins[0].f, ins[1].f, None, 0, e.beta, 0)[0].astype(F32))
        assert np.array_equal(v[4].body(), sk.ref_lm_step2_first(v[4].f, ins[0].f, e.alpha).astype(F32))


# ------------------------------------------------------------------ LM: the finish deferred into the flat update
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("stop", [False, True, "frozen"])
@pytest.mark.parametrize("words", [(6, 0), (0, 6)])
@pytest.mark.parametrize("nb", COUNTS)
def test_pcg_update_lm_fin(torch, L, cus, nb, words, stop, regime):
    """From the partials of `nb` workgroups: alphaD (bit-exact), betaN (1 ulp), Q1 = 0.5 [U + alpha (T1 - T2) - alpha^2 alphaD] (float64 value to 1 ulp, as betaN: a
    double expression the compiler may contract; its condition number is read off) -- Q0 read from state[q_in], Q1 written to state[q_out] when the loop goes on, in which
    case r, delta (k = 1) and p_out (k = 4) are pcg_update's.  On a stop (tolerance) state[1] = 1, state[2] = k_prev + 1 and r, delta, p_out are bit-untouched; so they are
    when the state was frozen before, and then no word changes either.  Which word Q0 comes from decides the verdict: zeta = 5 (Q1 - Q0) / Q1 against a tolerance of 1
    is 2.5 for Q0 = Q1 / 2 and 0 for Q0 = Q1; state[q_in] holds the one, every other free word (q_out included) the other, so reading the wrong word flips stop / go.
    Both (q_in, q_out) pairs of the loop's parity, (6, 0) and (0, 6)."""
    n = 4 * 256 * 33 + 5
    e = Env(torch, L, cus, n, regime, 17 + nb)
    ex = regime == "exact"
    r, Ap, pre, p_in, p_out, delta = e.vec(const=bool(stop)), e.vec(const=True), e.vec(const=True, kind="pre"), e.vec(const=True), e.out(), e.vec(const=bool(stop))
    aN, _, _ = e.sums(COUNTS.index(nb), lm=True)
    ad, s3 = _s3(e, nb)
    if ex: q3 = np.ascontiguousarray(np.stack([sk.exact_sum(e.rng, nb, t).astype(np.float64) for t in (10.0, 6.0, 2.0)], axis=1))
    else: q3 = np.ascontiguousarray(np.abs(e.rng.standard_normal((nb, 3))) * np.array([100.0, 1.0, 0.5]))
    adw = sk.sum_partials(ad); alpha = sk.div32(e.aN, adw, False)
    U, T1, T2 = (sk.sum_partials_f64(q3[:, j]) for j in range(3))
    a = float(alpha)
    Q1 = 0.5 * (U + a * (T1 - T2) - a * a * float(adw)); qmag = 0.5 * (abs(U) + abs(a * T1) + abs(a * T2) + a * a * abs(float(adw)))
    assert np.isfinite(Q1) and Q1 != 0 and qmag / abs(Q1) < 2.0 ** 20
    kprev, (q_in, q_out), tolr = 4, words, 1.0
    Q0, decoy = (0.5 * Q1, Q1) if stop is False else (Q1, 0.5 * Q1)
    s0 = _state(0.0, 1 if stop == "frozen" else 0, 2 if stop == "frozen" else 0)
    s0[[0, 3, 4, 5, 6, 7]] = decoy; s0[q_in] = Q0
    st, adt, s3t, q3t, w = sk.dbuf(torch, s0), sk.dbuf(torch, ad), sk.dbuf(torch, s3), sk.dbuf(torch, q3), sk.canary_buf(torch, 2)
    assert L.thallo_hip_pcg_update_lm_fin(r.ptr, Ap.ptr, pre.ptr, p_in.ptr, p_out.ptr, delta.ptr, n, aN, adt.data_ptr(), s3t.data_ptr(), q3t.data_ptr(), nb,
                                          w.data_ptr(), w.data_ptr() + 4, st.data_ptr(), kprev, tolr, q_in, q_out, None) == 0
    e.finish()
    sh, wh = st.cpu().numpy(), w.cpu().numpy()
    for t, h in ((adt, ad), (s3t, s3), (q3t, q3)): assert sk.same_bytes(t.cpu().numpy(), h)
    if stop == "frozen":
        assert sk.same_bytes(sh, s0) and sk.written_slots(wh) == 0 and p_out.unchanged()
        return
    _, _, bnw, mag = sk.ref_scalars_finish(ad, s3, e.aN, guard=False)
    assert sk.same_bytes(wh[:1], adw)
    _check_bn_word(wh[1], bnw, mag)
    if stop:
        want = s0.copy(); want.view(np.uint32)[1] = 1; want.view(np.int32)[2] = kprev + 1
        assert sk.same_bytes(sh, want), (sh, want)
        assert p_out.unchanged()
        return
    want = s0.copy(); want[q_out] = sh[q_out]
    assert sk.same_bytes(sh, want) and sk.ulp_apart(sh[q_out], F32(Q1)) <= 1, (sh, Q1)
    beta = sk.div32(wh[1], e.aN, False)
    r1, po, d1 = sk.ref_pcg_update(r.f, Ap.f, pre.f, p_in.f, delta.f, alpha, beta, 0)
    if ex: assert float(wh[1]) == 9.0 and float(beta) == 0.75 and float(sh[q_out]) == 2.0      # 0.5 (10 + 0.75 (6 - 2) - 0.5625 * 16)
    e.check(r, r1, 1, np.abs(r.f) + np.abs(a * Ap.f)); e.check(delta, d1, 1, np.abs(delta.f) + np.abs(a * p_in.f))
    e.check(p_out, po, 4, np.abs(pre.f) * (np.abs(r.f) + np.abs(a * Ap.f)) + np.abs(float(beta) * p_in.f))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", ["frozen_at_3", "frozen_at_4", "not_frozen", "done_0"])
def test_lm_owed_delta(torch, L, cus, case, regime):
    """delta += alpha_kl p_kl with kl = (frozen ? state[2] : L) - 1, one fma (k = 1), the unguarded divide of words `stride` apart; the parity of kl picks p_even / p_odd;
    kl < 0 (frozen before the first iteration): nothing happens."""
    n = 1027
    Lit, stride = 6, 3
    frozen, its = {"frozen_at_3": (1, 3), "frozen_at_4": (1, 4), "not_frozen": (0, 0), "done_0": (1, 0)}[case]
    kl = (its if frozen else Lit) - 1
    e = Env(torch, L, cus, n, regime, 18)
    delta, pe, po = e.vec(const=kl < 0), e.vec(const=True), e.vec(const=True)
    e.sums(0)
    if regime == "exact":
        aNw = np.arange(1, 1 + Lit * stride, dtype=F32); aDw = np.full(Lit * stride, 7.0, F32); aDw[::stride] = 2.0 ** (np.arange(Lit) % 3 + 1)
    else:
        aNw, aDw = sk.rounded_sum(e.rng, Lit * stride, True), sk.rounded_sum(e.rng, Lit * stride, True)
    at, dt, st = sk.dbuf(torch, aNw), sk.dbuf(torch, aDw), sk.dbuf(torch, _state(1.0, frozen, its))
    assert L.thallo_hip_lm_owed_delta(delta.ptr, pe.ptr, po.ptr, n, at.data_ptr(), dt.data_ptr(), stride, st.data_ptr(), Lit, None) == 0
    e.finish()
    if kl < 0: return
    alpha = sk.div32(aNw[kl * stride], aDw[kl * stride], False)
    p = po if kl & 1 else pe
    e.check(delta, sk.ref_lm_step2_first(delta.f, p.f, alpha), 1, np.abs(delta.f) + np.abs(float(alpha) * p.f))


# ------------------------------------------------------------------ PCGLinearUpdate
def _terms(e, L, count):
    """`count` pending terms: planes p_j and their (alphaN, alphaD) sums of rotating counts; exact regime: alpha_j from {1/2, 3/4, -1/4, 3/2}"""
    T = sk.UpdateTermsT(); T.count = count
    ps, alphas, keep = [], [], []
    for j in range(count):
        p = e.vec(const=True)
        if e.regime == "exact": a_n, a_d = [(1.0, 2.0), (3.0, 4.0), (-2.0, 8.0), (6.0, 4.0)][j % 4]; parts = [sk.exact_sum(e.rng, COUNTS[j % 5], a_n), sk.exact_sum(e.rng, COUNTS[(j + 2) % 5], a_d)]
        else: parts = [sk.rounded_sum(e.rng, COUNTS[j % 5], True), sk.rounded_sum(e.rng, COUNTS[(j + 2) % 5], True) * 16]
        ts = [sk.dbuf(e.torch, q) for q in parts]; keep += ts
        T.p[j] = p.ptr; T.alphaN[j] = sk.sumt(ts[0]); T.alphaD[j] = sk.sumt(ts[1])
        ps.append(p); alphas.append(sk.div32(sk.sum_partials(parts[0]), sk.sum_partials(parts[1]), True))
    return T, ps, alphas, keep


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("path,n", [("vector", 4 * 256 * 70 + 4), ("scalar_len", 4 * 256 * 70 + 3), ("scalar_offset", 4 * 256 * 70 + 4)])
@pytest.mark.parametrize("count", [1, 3, 4, 5, 8, 9, 12, 13, 32])
def test_linear_update_n(torch, L, cus, count, path, n, regime):
    """delta += alpha_0 p_0, += alpha_1 p_1, ...: one fma per term on the running value (k = count; scale |delta| + sum |alpha_j p_j|); X given: X += that (k + 1) and
    delta is not written.  The float4 path (aligned pointers, len % 4 == 0: blocks of 8, of 4, singles); the scalar path by an odd length, or by a target (X, or delta
    without X) that starts one float into its buffer.  max_workgroups 0, 1, 256 -- the returned grid is flat_grid with twice the CUs, capped (the scalar path's 281
    workgroups meet the cap of 256).  N terms at once = N single-term calls, bitwise."""
    toff = 1 if path == "scalar_offset" else 0
    ln = n - 4 if path == "scalar_offset" else n
    ts, ss = slice(toff, toff + ln), slice(0, ln)
    g = sk.flat_grid(ln // 4 if path == "vector" else ln, 2 * cus)
    for mw, with_X in ((0, False), (1, True), (256, False), (0, True)):
        e = Env(torch, L, cus, n, regime, 19)
        e.sums(0)
        delta = e.vec(const=with_X)
        T, ps, alphas, keep = _terms(e, L, count)
        X = e.vec() if with_X else None
        dslice = ss if with_X else ts
        dptr = delta.ptr + 4 * dslice.start
        ret = L.thallo_hip_linear_update_n(X.ptr + 4 * toff if with_X else None, dptr, T, ln, mw, None)
        single = sk.DVec(torch, n, delta.h0[:n])
        for j in range(count):
            T1 = sk.UpdateTermsT(); T1.count = 1; T1.p[0] = T.p[j]; T1.alphaN[0] = T.alphaN[j]; T1.alphaD[0] = T.alphaD[j]
            assert L.thallo_hip_linear_update_n(None, single.ptr + 4 * dslice.start, T1, ln, mw, None) > 0
        e.finish()
        assert single.canary_ok()
        assert ret == (min(g, mw) if mw else g), (ret, g, mw)
        pf = [p.f[ss] for p in ps]
        d0 = delta.f[dslice]
        scale = np.abs(d0) + sum(np.abs(float(a) * p) for a, p in zip(alphas, pf))
        Xw, dw = sk.ref_linear_update_n(X.f[ts] if with_X else None, d0, pf, alphas)
        tgt = X if with_X else delta
        want, k, sc = (Xw, count + 1, np.abs(X.f[ts]) + scale) if with_X else (dw, count, scale)
        got = tgt.body()[ts]
        if regime == "exact": assert (want == want.astype(F32)).all() and np.array_equal(got, want.astype(F32))
        else: assert (np.abs(got - want) <= sk.tol(k, sc)).all()
        outside = np.ones(e.c4, bool); outside[ts] = False
        assert sk.same_bytes(tgt.body()[outside], tgt.h0[:e.c4][outside])
        if with_X: assert sk.same_bytes(got, (X.h0[:e.c4][ts] + single.body()[ss]).astype(F32)), "N terms at once differ from N single-term calls"
        else: assert sk.same_bytes(delta.get(), single.get()), "N terms at once differ from N single-term calls"


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("ln", [1, 3, 257])
def test_linear_update_on_an_unpadded_buffer(torch, L, cus, ln, regime):
    """thallo_hip_linear_update / _update2 on a caller buffer of exactly `len` floats with the canary right behind it: X += delta (k = 1), X += fma(alpha, p, delta)
    (k = 2), X += fma(a1, p1, fma(a0, p0, delta)) (k = 3; scale |X| + |delta| + sum |alpha p|)."""
    e = Env(torch, L, cus, ln, regime, 20)
    aN, aD, bN = e.sums(3)
    a0 = e.alpha
    a1 = sk.div32(e.bN, e.aD, True)
    gen = sk.exact_vec if regime == "exact" else sk.rounded_vec
    delta, p0, p1 = e.vec(const=True), e.vec(const=True), e.vec(const=True)
    for which in (0, 1, 2):
        x0 = gen(e.rng, ln)
        h = np.full(ln + 64, sk.CANARY, np.uint32).view(F32).copy(); h[:ln] = x0
        X = sk.dbuf(torch, h)
        if which == 0: ret = L.thallo_hip_linear_update(X.data_ptr(), delta.ptr, None, ln, aN, aD, None); ps, al = [], []
        elif which == 1: ret = L.thallo_hip_linear_update(X.data_ptr(), delta.ptr, p0.ptr, ln, aN, aD, None); ps, al = [p0], [a0]
        else: ret = L.thallo_hip_linear_update2(X.data_ptr(), delta.ptr, p0.ptr, aN, aD, p1.ptr, bN, aD, ln, None); ps, al = [p0, p1], [a0, a1]
        e.finish()
        assert ret == sk.flat_grid(ln, cus)
        got = X.cpu().numpy()
        assert sk.same_bytes(got[ln:], h[ln:])
        pf = [p.f[:ln] for p in ps]
        Xw, _ = sk.ref_linear_update_n(x0, delta.f[:ln], pf, al)
        if regime == "exact": assert np.array_equal(got[:ln], Xw.astype(F32)) and (Xw == Xw.astype(F32)).all()
        else: assert (np.abs(got[:ln] - Xw) <= sk.tol(which + 1, np.abs(x0) + np.abs(delta.f[:ln]) + sum(np.abs(float(a) * p) for a, p in zip(al, pf)))).all()


# ------------------------------------------------------------------ dot, finish_sum_gated, alpha_beta
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("idx,n", list(enumerate(LENGTHS)))
def test_dot_and_scalar_words(torch, L, cus, idx, n, regime):
    """thallo_hip_dot's partials (terms a.b); thallo_hip_finish_sum_gated with a zero gate = the documented sum, bitwise; thallo_hip_alpha_beta = the helper's alpha, beta."""
    nn = _n(n, cus)
    e = Env(torch, L, cus, nn, regime, 21)
    a, b = e.vec(const=True), e.vec(const=True)
    aN, aD, bN = e.sums(idx)
    pb, w, gate = e.pbuf(), sk.canary_buf(torch, 4), sk.dbuf(torch, np.zeros(1, np.uint32))
    ret = L.thallo_hip_dot(a.ptr, b.ptr, nn, pb.data_ptr(), None)
    assert L.thallo_hip_alpha_beta(aN, aD, bN, w.data_ptr(), None) == 0
    assert L.thallo_hip_finish_sum_gated(bN, w.data_ptr() + 8, gate.data_ptr(), None) == 0
    e.finish()
    part = e.check_partials(pb, ret, a.f * b.f, a.f * b.f, 1.0)
    assert sk.same_bytes(w.cpu().numpy()[:3], np.array([e.alpha, e.beta, e.bN], F32))
    pt = sk.dbuf(torch, part)
    assert L.thallo_hip_finish_sum_gated(sk.sumt(pt), w.data_ptr() + 12, gate.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert sk.same_bytes(w.cpu().numpy()[3:], sk.sum_partials(part))
