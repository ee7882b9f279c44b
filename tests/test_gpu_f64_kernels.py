"""The twelve double-precision PCG / LM kernels of csrc/pcg_kernels_f64.hip (thallo_hip_f64_*), one test each, against exact arithmetic.

What an output is held to follows from how many roundings the kernel's text allows it (u = 2^-53, the unit roundoff of a double):

  * ONE operation (z = pre r, r = b - Adelta, X += delta, b = r, p = z): the device must EQUAL numpy's float64 result of the device's own inputs -- IEEE leaves no choice;
  * a + s b (delta += alpha p, r -= alpha Ap, p = z + beta p, Ap += CtC p): the device must equal ONE OF the two results the language allows, fl(a + fl(s b)) or the
    contracted fma(s, b, a).  The fma is computed exactly: s b = hi + lo by Dekker's error-free product, then math.fsum([a, hi, lo]), which rounds the exact sum once;
  * chains with division and square root (guardedInvert, the LM diagonal): k u RELATIVE to the exact value -- every quantity in them is positive, so there is no
    cancellation -- k counted per output in its test.  The exact value is a fractions.Fraction (square roots from integer isqrt to 2^-200) at every element for
    n <= 257 and, at the grid-stride length, on the first and last 300 elements, the elements around every 2^16 and 500 random ones; all 262145 elements are also held
    to the same k u + 2^-58 against an x87 long double evaluation (64-bit significand: 2^-64 per operation), skipped where numpy's longdouble is no wider than a double;
  * sums: every per-workgroup partial within gamma_c of sum |terms| of the exact sum (math.fsum over the error-free products) of the DEVICE's own outputs, c = the
    longest chain of additions behind the partial (visits of one thread, 6 butterfly levels, 4 waves) + the roundings inside one term; gamma_c = c u / (1 - c u).

alpha = alphaN / alphaD and beta = betaN / alphaN are one IEEE division of two device words: Python forms them bit-exactly.  The GN kernels give 0 when the denominator
is 0; the LM kernels divide blindly (gauss_newton.t:226-234), so there a zero denominator must give exactly the infinities and NaNs IEEE arithmetic gives.

Every buffer carries a quiet-NaN canary behind its payload, compared as bytes after every call; `const` inputs must come back bit-unchanged; a launcher that returns
its grid is held to min(ceil(n / 256), 1024) and its partials buffer to exactly that many written slots."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import shim_kernels as sk

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CANARY64 = 0x7FF8BEEF7FF8BEEF            # a quiet NaN as a double, and 0x7FF8BEEF in either 32-bit half
B64 = 256
LENGTHS = [1, 255, 256, 257, 1024 * 256 + 1]       # the last one grid-strides: workgroup 0 comes round a second time for one element
PSLOTS = sk.MAX_PARTIALS + 8
WIDE = np.finfo(np.longdouble).nmant >= 63


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    return sk.shim()


# ------------------------------------------------------------------ buffers
class D64:
    """n doubles of payload (None: canary everywhere) and 256 canary doubles behind them"""

    def __init__(self, torch, n, payload=None):
        h = np.full(n + 256, CANARY64, np.uint64).view(np.float64)
        if payload is not None:
            h[:n] = np.asarray(payload, np.float64)
        self.n, self.h0 = n, h.copy()
        self.t = torch.from_numpy(h).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def body(self):
        return self.t.cpu().numpy()[:self.n]

    def canary_ok(self):
        return self.t.cpu().numpy()[self.n:].tobytes() == self.h0[self.n:].tobytes()

    def unchanged(self):
        return self.t.cpu().numpy().tobytes() == self.h0.tobytes()


def grid_for(n):
    return max(1, min((n + B64 - 1) // B64, sk.MAX_PARTIALS))


def visits(n):
    """most elements one thread of the grid-stride loop adds up"""
    return (n + B64 * grid_for(n) - 1) // (B64 * grid_for(n))


def gamma(c):
    return c * U / (1.0 - c * U)


class Env:
    def __init__(self, torch, L, n, *seed):
        self.torch, self.L, self.n = torch, L, n
        self.rng = np.random.default_rng([n] + [int(s) if not isinstance(s, str) else int.from_bytes(s.encode(), "little") % 2 ** 32 for s in seed])
        self.const, self.all = [], []

    def vec(self, payload=None, const=False, positive=False, n=None):
        n = self.n if n is None else n
        if payload is None:
            payload = self.rng.standard_normal(n) * 10.0 ** self.rng.integers(-3, 4, n)
            payload[payload == 0] = 1.0
            if positive: payload = np.abs(payload)
        v = D64(self.torch, n, np.broadcast_to(np.asarray(payload, np.float64), (n,)))
        v.f = v.h0[:n].copy()
        self.all.append(v)
        if const: self.const.append(v)
        return v

    def word(self, x):
        return self.vec(payload=[x], const=True, n=1)

    def out(self, n=None):
        v = D64(self.torch, self.n if n is None else n)
        self.all.append(v)
        return v

    def pbuf(self):
        return self.out(PSLOTS)

    def finish(self):
        self.torch.cuda.synchronize()
        for v in self.const: assert v.unchanged(), "a const input changed"
        for v in self.all: assert v.canary_ok(), "the canary behind a buffer changed"

    def partials(self, buf, ret, exact_terms, c):
        """`ret` = the grid, exactly that many slots written, each within gamma_c sum|terms| of the exact sum of its workgroup's terms.
        exact_terms: arrays whose elementwise sum is the exact term (error-free pieces)."""
        g = grid_for(self.n)
        assert ret == g, (ret, g)
        host = buf.t.cpu().numpy()[:PSLOTS]
        dirty = host.view(np.uint64) != CANARY64
        assert dirty[:g].all() and not dirty[g:].any(), "written slots are not exactly the grid"
        blk = (np.arange(self.n) // B64) % g
        order = np.argsort(blk, kind="stable")
        cuts = np.cumsum(np.bincount(blk, minlength=g))[:-1]
        pieces = [np.split(np.asarray(t, np.float64)[order], cuts) for t in exact_terms]
        term = np.abs(np.sum(exact_terms, axis=0))
        mags = np.split(term[order], cuts)
        for b in range(g):
            want = math.fsum(x for p in pieces for x in p[b].tolist())
            bound = gamma(c) * math.fsum(mags[b].tolist())
            assert abs(host[b] - want) <= bound, (b, host[b], want, bound)
        return host[:g]


# ------------------------------------------------------------------ exact arithmetic
def _split(a):
    c = 134217729.0 * a                  # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def two_prod(a, b):
    """a b = p + e exactly (Dekker), elementwise; the operands here stay far from overflow and underflow"""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    p = a * b
    ah, al = _split(a); bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma_exact(s, b, a):
    """fma(s, b, a) elementwise: the exact a + s b rounded once"""
    p, e = two_prod(s, b)
    a = np.broadcast_to(np.asarray(a, np.float64), p.shape)
    return np.array([math.fsum(t) for t in zip(a.tolist(), p.tolist(), e.tolist())], np.float64)


def assert_axpy(got, a, s, b, what):
    """got = a + s b with one rounding per operation, contracted or not"""
    with np.errstate(all="ignore"):
        plain = np.asarray(a, np.float64) + np.asarray(s, np.float64) * np.asarray(b, np.float64)
    fused = fma_exact(s, b, a)
    ok = (got == plain) | (got == fused)
    assert ok.all(), (what, np.flatnonzero(~ok)[:8])


def assert_same(got, want, what):
    assert got.tobytes() == np.ascontiguousarray(want, np.float64).tobytes(), (what, np.flatnonzero(got != want)[:8])


def frac_sqrt(x):
    """sqrt of a non-negative Fraction to a relative 2^-200"""
    k = 220
    return Fraction(math.isqrt((x.numerator * x.denominator) << (2 * k)), x.denominator << k)


SLACK = 1 + Fraction(1, 2 ** 20)      # (1 + u)^k - 1 = k u (1 + O(k u)): the second-order terms


def exact_indices(n):
    if n <= 257:
        return np.arange(n)
    rng = np.random.default_rng(n)
    marks = np.concatenate([np.arange(300), np.arange(n - 300, n), rng.integers(0, n, 500)] + [np.arange(m - 2, m + 3) for m in range(65536, n, 65536)])
    return np.unique(marks[(marks >= 0) & (marks < n)])


def assert_relative(got, fn, inputs, k, what):
    """got within k u (relative) of fn(*inputs) in exact arithmetic; fn(sqrt, *scalars-or-arrays) uses + - * / and the sqrt it is given"""
    n = got.size
    idx = exact_indices(n)
    for i in idx.tolist():
        want = fn(frac_sqrt, *[Fraction(float(a[i])) for a in inputs])
        assert abs(Fraction(float(got[i])) - want) <= Fraction(k) * Fraction(U) * SLACK * abs(want), (what, i, float(got[i]), float(want))
    if idx.size < n and WIDE:
        want = fn(np.sqrt, *[np.asarray(a, np.longdouble) for a in inputs])
        err = np.abs(got.astype(np.longdouble) - want)
        bad = err > (k * U + 2.0 ** -58) * np.abs(want)
        assert not bad.any(), (what, np.flatnonzero(bad)[:8])


def ginv(sqrt, d):
    s = 1 + sqrt(d)
    return 1 / (s * s)


K_GINV = 6      # sqrt: 1; 1 + .: 2; squared: 2 * 2 + 1 = 5; reciprocal: 6


def div64(num, den, guard):
    if guard and den == 0.0:
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.float64(num) / np.float64(den))


# ------------------------------------------------------------------ the Gauss-Newton set
@pytest.mark.parametrize("use_pre", [0, 1])
@pytest.mark.parametrize("n", LENGTHS)
def test_f64_init_finish(torch, L, n, use_pre):
    """pre = guardedInvert(pre) (K_GINV u relative to exact) or 1; z = pre r (one product: equal); p = z; partials of r . z (one product per term)"""
    e = Env(torch, L, n, 1, use_pre)
    r, pre = e.vec(const=True), e.vec(positive=True)
    z, p, part = e.out(), e.out(), e.pbuf()
    ret = L.thallo_hip_f64_init_finish(r.ptr, pre.ptr, z.ptr, p.ptr, n, use_pre, part.ptr, None)
    e.finish()
    m = pre.body()
    if use_pre: assert_relative(m, ginv, [pre.f], K_GINV, "pre")
    else: assert_same(m, np.ones(n), "pre")
    assert_same(z.body(), m * r.f, "z")
    assert_same(p.body(), z.body(), "p")
    e.partials(part, ret, two_prod(r.f, z.body()), visits(n) + 10 + 1)


@pytest.mark.parametrize("n", LENGTHS)
def test_f64_dot(torch, L, n):
    e = Env(torch, L, n, 2)
    a, b, part = e.vec(const=True), e.vec(const=True), e.pbuf()
    ret = L.thallo_hip_f64_dot(a.ptr, b.ptr, n, part.ptr, None)
    e.finish()
    first = e.partials(part, ret, two_prod(a.f, b.f), visits(n) + 10 + 1)
    part2 = e.pbuf()
    L.thallo_hip_f64_dot(a.ptr, b.ptr, n, part2.ptr, None)
    e.finish()
    assert_same(part2.t.cpu().numpy()[:first.size], first, "a second run's partials")


@pytest.mark.parametrize("zero_den", [False, True])
@pytest.mark.parametrize("n", LENGTHS)
def test_f64_step2(torch, L, n, zero_den):
    """alpha = alphaN / alphaD, 0 when alphaD = 0; delta += alpha p and r -= alpha Ap (a + s b); z = pre r (equal); partials of z . r"""
    e = Env(torch, L, n, 3, zero_den)
    delta, r, z = e.vec(), e.vec(), e.out()
    p, Ap, pre = e.vec(const=True), e.vec(const=True), e.vec(const=True, positive=True)
    aN, aD = e.word(1.7320508075688772), e.word(0.0 if zero_den else 2.23606797749979)
    part = e.pbuf()
    ret = L.thallo_hip_f64_step2(delta.ptr, r.ptr, z.ptr, p.ptr, Ap.ptr, pre.ptr, n, aN.ptr, aD.ptr, part.ptr, None)
    e.finish()
    alpha = div64(aN.f[0], aD.f[0], True)
    if zero_den:
        assert alpha == 0.0
        assert_same(delta.body(), delta.f, "delta under alpha = 0"); assert_same(r.body(), r.f, "r under alpha = 0")
    else:
        assert_axpy(delta.body(), delta.f, alpha, p.f, "delta")
        assert_axpy(r.body(), r.f, -alpha, Ap.f, "r")
    assert_same(z.body(), pre.f * r.body(), "z")
    e.partials(part, ret, two_prod(z.body(), r.body()), visits(n) + 10 + 1)


@pytest.mark.parametrize("zero_den", [False, True])
@pytest.mark.parametrize("n", LENGTHS)
def test_f64_step3(torch, L, n, zero_den):
    """beta = betaN / alphaN, 0 when alphaN = 0; p = z + beta p"""
    e = Env(torch, L, n, 4, zero_den)
    p, z = e.vec(), e.vec(const=True)
    bN, aN = e.word(0.5772156649015329), e.word(0.0 if zero_den else 1.4142135623730951)
    assert L.thallo_hip_f64_step3(p.ptr, z.ptr, n, bN.ptr, aN.ptr, None) == 0
    e.finish()
    beta = div64(bN.f[0], aN.f[0], True)
    if zero_den: assert_same(p.body(), z.f, "p under beta = 0")
    else: assert_axpy(p.body(), z.f, beta, p.f, "p")


@pytest.mark.parametrize("n", LENGTHS)
def test_f64_linear_update(torch, L, n):
    e = Env(torch, L, n, 5)
    X, delta = e.vec(), e.vec(const=True)
    assert L.thallo_hip_f64_linear_update(X.ptr, delta.ptr, n, None) == 0
    e.finish()
    assert_same(X.body(), X.f + delta.f, "X")


@pytest.mark.parametrize("count", [1, 255, 256, 257, 1024])
def test_f64_finish(torch, L, count):
    """one word = the partials' sum: a thread adds ceil(count / 256) of them, then 6 butterfly levels and 4 waves; the same word in every run"""
    e = Env(torch, L, count, 6)
    part = e.vec(const=True)
    w1, w2 = e.out(1), e.out(1)
    assert L.thallo_hip_f64_finish(part.ptr, count, w1.ptr, None) == 0
    assert L.thallo_hip_f64_finish(part.ptr, count, w2.ptr, None) == 0
    e.finish()
    c = (count + B64 - 1) // B64 + 10
    assert abs(w1.body()[0] - math.fsum(part.f.tolist())) <= gamma(c) * math.fsum(np.abs(part.f).tolist())
    assert_same(w2.body(), w1.body(), "a second run's word")


@pytest.mark.parametrize("count", [0, -1, 1025])
def test_f64_finish_refuses_counts(torch, L, count):
    e = Env(torch, L, 1025, 7)
    part, w = e.vec(const=True), e.out(1)
    assert L.thallo_hip_f64_finish(part.ptr, count, w.ptr, None) == sk.INVALID
    e.finish()
    assert w.unchanged()


def test_f64_finish_refuses_null(torch, L):
    e = Env(torch, L, 257, 7)
    part, w = e.vec(const=True), e.out(1)
    assert L.thallo_hip_f64_finish(None, 257, w.ptr, None) == sk.INVALID
    assert L.thallo_hip_f64_finish(part.ptr, 257, None, None) == sk.INVALID
    e.finish()
    assert w.unchanged()


# ------------------------------------------------------------------ the Levenberg-Marquardt set
def _lm_c(sqrt, d, ss, radius, lo, hi):
    unclamped, cm = d / radius, (1 / ss) / radius
    return min(max(unclamped, lo * cm), hi * cm) if isinstance(d, Fraction) else np.minimum(np.maximum(unclamped, lo * cm), hi * cm)


def _lm_m(sqrt, d, c):
    return 1 / (c + d)


@pytest.mark.parametrize("save_ssq,use_pre", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("n", LENGTHS)
def test_f64_lm_finalize_diagonal(torch, L, n, save_ssq, use_pre):
    """SSq (saved: guardedInvert(d), K_GINV u, or 1; not saved: read, unchanged); CtC = clamp(d / radius, min cm, max cm), cm = (1 / SSq) / radius, from the device's
    own SSq: d / radius 1 rounding, min cm and max cm 3, and a clamp of positive numbers keeps the largest relative error: 3 u; pre = 1 / (CtC + radius (d / radius))
    from the device's own CtC: quotient, product, sum, reciprocal: 4 u of the exact 1 / (CtC + d); b = r and z = pre r equal; partials of r . z.
    min = 0.1 and max = 0.5 put elements on both clamp ends and between them (asserted)."""
    e = Env(torch, L, n, 8, save_ssq, use_pre)
    radius, lo, hi = 3.0e3 / 7.0, 0.1, 0.5
    d = np.abs(e.rng.standard_normal(n)) * 10.0 ** (e.rng.integers(-4, 5, n) if n > 1 else np.array([0]))
    diag, r = e.vec(payload=d, const=True), e.vec(const=True)
    SSq = e.out() if save_ssq else e.vec(payload=e.rng.uniform(0.01, 4.0, n), const=True)
    CtC, pre, b, z, part = e.out(), e.out(), e.out(), e.out(), e.pbuf()
    ret = L.thallo_hip_f64_lm_finalize_diagonal(diag.ptr, SSq.ptr, CtC.ptr, pre.ptr, r.ptr, b.ptr, z.ptr, n, radius, lo, hi, save_ssq, use_pre, part.ptr, None)
    e.finish()
    ss = SSq.body()
    if save_ssq:
        if use_pre: assert_relative(ss, ginv, [diag.f], K_GINV, "SSq")
        else: assert_same(ss, np.ones(n), "SSq")
    cw = np.full(n, radius), np.full(n, lo), np.full(n, hi)
    assert_relative(CtC.body(), _lm_c, [diag.f, ss, *cw], 3, "CtC")
    if n >= 255:
        x, cm = diag.f / radius, 1.0 / ss / radius
        assert (x < 0.99 * lo * cm).any() and (x > 1.01 * hi * cm).any() and ((x > 1.01 * lo * cm) & (x < 0.99 * hi * cm)).any(), "a clamp end is idle"
    assert_relative(pre.body(), _lm_m, [diag.f, CtC.body()], 4, "pre")
    assert_same(b.body(), r.f, "b")
    assert_same(z.body(), pre.body() * r.f, "z")
    e.partials(part, ret, two_prod(r.f, z.body()), visits(n) + 10 + 1)


@pytest.mark.parametrize("n", LENGTHS)
def test_f64_lm_step1_finish(torch, L, n):
    """Ap += CtC p (a + s b); partials of p . Ap"""
    e = Env(torch, L, n, 9)
    Ap, CtC, p, part = e.vec(), e.vec(const=True, positive=True), e.vec(const=True), e.pbuf()
    ret = L.thallo_hip_f64_lm_step1_finish(Ap.ptr, CtC.ptr, p.ptr, n, part.ptr, None)
    e.finish()
    assert_axpy(Ap.body(), Ap.f, CtC.f, p.f, "Ap")
    e.partials(part, ret, two_prod(p.f, Ap.body()), visits(n) + 10 + 1)


def q_terms(delta, r, b):
    """0.5 delta (r + b) in error-free pieces"""
    s, t = two_sum(r, b)
    p1, e1 = two_prod(delta, s)
    p2, e2 = two_prod(delta, t)
    return [0.5 * p1, 0.5 * e1, 0.5 * p2, 0.5 * e2]


def blind(aN, aD, a, sign, b):
    """a + sign (aN / aD) b as IEEE arithmetic gives it, infinities and NaNs included"""
    with np.errstate(all="ignore"):
        return a + (sign * np.float64(aN) / np.float64(aD)) * b


@pytest.mark.parametrize("den", ["regular", "zero", "zero_over_zero"])
@pytest.mark.parametrize("n", LENGTHS)
def test_f64_lm_step2(torch, L, n, den):
    """delta += alpha p, r -= alpha Ap (a + s b), z = pre r (equal), partials of z . r and of q = 0.5 delta . (r + b) (sum, product: 2 roundings per term).
    The division is blind: alphaD = 0 leaves the infinities (NaN for 0 / 0) IEEE gives, in delta, r and z."""
    e = Env(torch, L, n, 10, den)
    delta, r, z = e.vec(), e.vec(), e.out()
    p, Ap, pre, b = e.vec(const=True), e.vec(const=True), e.vec(const=True, positive=True), e.vec(const=True)
    aN = e.word(0.0 if den == "zero_over_zero" else 1.7320508075688772)
    aD = e.word(2.23606797749979 if den == "regular" else 0.0)
    pb, pq = e.pbuf(), e.pbuf()
    ret = L.thallo_hip_f64_lm_step2(delta.ptr, r.ptr, z.ptr, p.ptr, Ap.ptr, pre.ptr, b.ptr, n, aN.ptr, aD.ptr, pb.ptr, pq.ptr, None)
    e.finish()
    assert ret == grid_for(n)
    if den != "regular":
        want_d, want_r = blind(aN.f[0], aD.f[0], delta.f, 1.0, p.f), blind(aN.f[0], aD.f[0], r.f, -1.0, Ap.f)
        assert not np.isfinite(want_d).any() and not np.isfinite(want_r).any()
        assert np.array_equal(delta.body(), want_d, equal_nan=True) and np.array_equal(r.body(), want_r, equal_nan=True)
        with np.errstate(all="ignore"):
            assert np.array_equal(z.body(), pre.f * want_r, equal_nan=True)
        return
    alpha = div64(aN.f[0], aD.f[0], False)
    assert_axpy(delta.body(), delta.f, alpha, p.f, "delta")
    assert_axpy(r.body(), r.f, -alpha, Ap.f, "r")
    assert_same(z.body(), pre.f * r.body(), "z")
    e.partials(pb, ret, two_prod(z.body(), r.body()), visits(n) + 10 + 1)
    e.partials(pq, ret, q_terms(delta.body(), r.body(), b.f), visits(n) + 10 + 2)


@pytest.mark.parametrize("den", ["regular", "zero"])
@pytest.mark.parametrize("n", LENGTHS)
def test_f64_lm_step2_first_half(torch, L, n, den):
    e = Env(torch, L, n, 11, den)
    delta, p = e.vec(), e.vec(const=True)
    aN, aD = e.word(1.7320508075688772), e.word(2.23606797749979 if den == "regular" else 0.0)
    assert L.thallo_hip_f64_lm_step2_first_half(delta.ptr, p.ptr, n, aN.ptr, aD.ptr, None) == 0
    e.finish()
    if den == "regular": assert_axpy(delta.body(), delta.f, div64(aN.f[0], aD.f[0], False), p.f, "delta")
    else: assert np.array_equal(delta.body(), blind(aN.f[0], aD.f[0], delta.f, 1.0, p.f)) and np.isinf(delta.body()).all()


@pytest.mark.parametrize("n", LENGTHS)
def test_f64_lm_step2_second_half(torch, L, n):
    """r = b - Adelta and z = pre r (one operation each: equal); partials of z . r and of q = 0.5 delta . (r + b)"""
    e = Env(torch, L, n, 12)
    r, z = e.out(), e.out()
    b, Ad, pre, delta = e.vec(const=True), e.vec(const=True), e.vec(const=True, positive=True), e.vec(const=True)
    pb, pq = e.pbuf(), e.pbuf()
    ret = L.thallo_hip_f64_lm_step2_second_half(r.ptr, b.ptr, Ad.ptr, pre.ptr, z.ptr, delta.ptr, n, pb.ptr, pq.ptr, None)
    e.finish()
    assert_same(r.body(), b.f - Ad.f, "r")
    assert_same(z.body(), pre.f * r.body(), "z")
    e.partials(pb, ret, two_prod(z.body(), r.body()), visits(n) + 10 + 1)
    e.partials(pq, ret, q_terms(delta.f, r.body(), b.f), visits(n) + 10 + 2)


@pytest.mark.parametrize("den", ["regular", "zero"])
@pytest.mark.parametrize("n", LENGTHS)
def test_f64_lm_step3(torch, L, n, den):
    """p = z + (betaN / alphaN) p, the division blind"""
    e = Env(torch, L, n, 13, den)
    p, z = e.vec(), e.vec(const=True)
    bN, aN = e.word(0.5772156649015329), e.word(1.4142135623730951 if den == "regular" else 0.0)
    assert L.thallo_hip_f64_lm_step3(p.ptr, z.ptr, n, bN.ptr, aN.ptr, None) == 0
    e.finish()
    if den == "regular": assert_axpy(p.body(), z.f, div64(bN.f[0], aN.f[0], False), p.f, "p")
    else: assert np.array_equal(p.body(), blind(bN.f[0], aN.f[0], z.f, 1.0, p.f)) and np.isinf(p.body()).all()


# ------------------------------------------------------------------ refusals
# entry point -> (number of pointer arguments in front of n, what follows n: "p" a pointer, anything else a value passed as it is)
ENTRIES = {
    "init_finish": (4, [1, "p"]), "dot": (2, ["p"]), "step2": (6, ["p", "p", "p"]), "step3": (2, ["p", "p"]), "linear_update": (2, []),
    "lm_finalize_diagonal": (7, [2.0, 0.1, 0.5, 1, 1, "p"]), "lm_step1_finish": (3, ["p"]), "lm_step2": (7, ["p", "p", "p", "p"]),
    "lm_step2_first_half": (2, ["p", "p"]), "lm_step2_second_half": (6, ["p", "p"]), "lm_step3": (2, ["p", "p"]),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_f64_refuses_null_and_empty(torch, L, name):
    """every pointer NULL in turn, n = 0 and n = -1: -hipErrorInvalidValue, and nothing is written"""
    lead, tail = ENTRIES[name]
    n = 257
    e = Env(torch, L, n, 14)
    bufs = [e.vec(const=True, positive=True) for _ in range(lead)] + [e.vec(const=True, n=PSLOTS) for t in tail if t == "p"]
    f = getattr(L, "thallo_hip_f64_" + name)

    def args(null=None, length=n):
        k, out = lead, [b.ptr for b in bufs[:lead]] + [length]
        for t in tail:
            if t == "p": out.append(bufs[k].ptr); k += 1
            else: out.append(t)
        ptrs = [i for i, a in enumerate(out) if i < lead or (i > lead and tail[i - lead - 1] == "p")]
        if null is not None: out[ptrs[null]] = None
        return out + [None], len(ptrs)

    _, nptr = args()
    for k in range(nptr):
        assert f(*args(null=k)[0]) == sk.INVALID, (name, "pointer", k)
    for length in (0, -1):
        assert f(*args(length=length)[0]) == sk.INVALID, (name, "n", length)
    e.finish()
