"""A numpy float64 reference of the shape_from_shading energy, with no device code: what every thallo_hip_sfs_* entry point (include/thallo_hip.h, section E3)
must leave, per pixel, on the GLOBAL image.  tests/test_sfs_reference.py holds it to central differences and to the float32 oracle (oracle/thallo_oracle.c:280-374);
tests/test_gpu_sfs_kernels.py holds the kernels to it.

Written from the comment block at the head of thallo_amd/csrc/energy_sfs.hip (lines 1-24) and from examples/shape_from_shading/shape_from_shading.t:
  :27      w_p, w_s, w_g are the square roots of the caller's parameters
  :40-80   B_I(c) = [D(c-ex) > 0, D(c) > 0, D(c-ey) > 0] (B(n^(c)) - I(c));  n = (u (c - l) / f_y,  l (c - u) / f_x,  n_x (u_x - x) / f_x + n_y (u_y - y) / f_y - l u / (f_x f_y))
           with c, l, u = X(c), X(c-ex), X(c-ey) (:47-49);  n^ = n / |n| (|n|^2 == 0: the factor is 1 and constant, oracle/thallo_oracle.c:314);
           B = L1 + L2 n^y + L3 n^z + L4 n^x + L5 n^x n^y + L6 n^y n^z + L7 (-n^x^2 - n^y^2 + 2 n^z^2) + L8 n^z n^x + L9 (n^x^2 - n^y^2);
           I(c) = 0.5 Im(c) + 0.25 (Im(c-ex) + Im(c-ey)) (:69);  loads outside the image return 0 (thallo.t:876-883)
  :86-87   fit(q)  = [D(q) > 0] w_p (X(q) - D(q))
  :90-93   sh_h(q) = [1 <= x <= W-2, 1 <= y <= H-2] w_g edgeMaskR(q) (BI(q) - BI(q+ex)),  sh_v(q) likewise with edgeMaskC and q+ey
  :96-104  reg_c(q) = [valid(q)] w_s (4 P_c(q) - sum over the four neighbours P_c(nbr)),  P(c) = X(c) ((x - u_x) / f_x, (y - u_y) / f_y, 1);
           valid(q) = D > 0 at q and its four neighbours and |X(q) - X(nbr)| < 0.01
Decisions (D > 0, the 0.01 gate, the inner-pixel guard, |n|^2 > 0) are taken on the float32 inputs as the spec states them and then frozen: zero derivative
(ad.t:824-829).  margins() tells how far every decision is from its threshold, so that a test can require that float32 and float64 decide alike.

Bounds.  Beside each value stands the scale S of its bound k 2^-24 S:
  * G = (dBI/dX(c), dBI/dX(c-ex), dBI/dX(c-ey), BI): the expression tree is evaluated on `Tr` objects, which carry the float64 value, the magnitude (the same tree with every
    + and - replaced by the sum of the magnitudes and every product by the product of the magnitudes) and the number k of float32 roundings on the longest chain
    (a sum: max(k_a, k_b) + 1; a product or quotient: k_a + k_b + 1; first order in 2^-24).  The one exception to "sum of magnitudes" is the difference of two INPUTS,
    c - l and c - u: one operation on exact operands, so its error is one rounding of the difference itself (k = 1, magnitude |c - l|).  Two trees: bi_forward() is the
    3-wide forward-mode evaluation of eval_BI_vals (energy_sfs.hip:69-90), bi_closed() the closed-form partials of eval_BI_pair (energy_sfs_pair.hip:346-387).
  * linear chains: the same chain with absolute values, |J|^T |F|, |J|^T |J| |p|, where |J| is the sum of the magnitudes of the terms of an entry BEFORE they are merged
    (sh_h(q) holds dBI(q)/dX(q) - dBI(q+ex)/dX(q) in column q: its magnitude is the sum of the two).
"""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

F32 = np.float32
EPS = 2.0 ** -24
GATE = F32(0.01)
RSQ = 2                       # roundings of 1 / sqrtf(x) in IEEE arithmetic (a correctly rounded root and a correctly rounded quotient); tests that measure the device pass their own
# the smallest sizes at which the kernels can go wrong (tests/test_gpu_sfs_kernels.py): every width around the strip seams of the one-pixel (60) and the pair (124) kernels and
# the tile width (64), odd and even, one to three strips; heights below, at and above the tile height (16) and the default rows per wave segment
SHAPES = [(1, 1), (2, 2), (3, 3), (4, 5), (59, 2), (60, 16), (61, 5), (62, 3), (64, 15), (65, 17), (124, 16), (125, 1), (126, 9), (130, 17), (250, 33)]
SEAMS_ONE = (59, 60, 61)      # columns around the first strip seam of the one-pixel marching kernel (60 output columns per wave)
SEAMS_PAIR = (123, 124, 125)  # ... and of the pair kernel (124)


# ------------------------------------------------------------------ tracked arithmetic
class Tr:
    """value v, magnitude m >= |v| (arrays), k roundings: a float32 evaluation of the same tree is within k 2^-24 m of v (first order)"""
    __slots__ = ("v", "m", "k")

    def __init__(self, v, m=None, k=0):
        self.v = np.asarray(v, np.float64)
        self.m = np.abs(self.v) if m is None else np.asarray(m, np.float64)
        self.k = k

    @staticmethod
    def of(x):
        return x if isinstance(x, Tr) else Tr(np.float64(x))

    def __add__(self, o):
        o = Tr.of(o)
        return Tr(self.v + o.v, self.m + o.m, max(self.k, o.k) + 1)

    def __sub__(self, o):
        o = Tr.of(o)
        return Tr(self.v - o.v, self.m + o.m, max(self.k, o.k) + 1)

    def __mul__(self, o):
        o = Tr.of(o)
        return Tr(self.v * o.v, self.m * o.m, self.k + o.k + 1)

    __radd__ = __add__
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Tr.of(o)
        with np.errstate(all="ignore"):
            return Tr(self.v / o.v, self.m * o.m / (o.v * o.v), self.k + o.k + 1)

    def exact(self, c):
        """times a power of two or -1: no rounding"""
        return Tr(self.v * c, self.m * abs(c), self.k)

    def rsqrt(self, pos, rsq=RSQ):
        """1 / sqrt where pos, 1 elsewhere: the relative error of the argument halves"""
        with np.errstate(all="ignore"):
            v = np.where(pos, 1.0 / np.sqrt(np.where(pos, self.v, 1.0)), 1.0)
            m = np.where(pos, v * self.m / np.where(pos, self.v, 1.0), 1.0)
        return Tr(v, m, (self.k + 1) // 2 + rsq)

    def where(self, mask, other):
        other = Tr.of(other)
        return Tr(np.where(mask, self.v, other.v), np.where(mask, self.m, other.m), max(self.k, other.k))


def diff_inputs(a, b):
    """a - b of two float32 INPUTS: one rounding of the difference itself"""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return Tr(d, np.abs(d), 1)


class Dual:
    """3-wide forward mode on Tr: value and the partials by X(c), X(c-ex), X(c-ey); the operators of energy_sfs.hip:61-66"""
    __slots__ = ("v", "d")

    def __init__(self, v, d=None):
        self.v = Tr.of(v)
        self.d = d if d is not None else [Tr(0.0), Tr(0.0), Tr(0.0)]

    def __add__(self, o):
        return Dual(self.v + o.v, [a + b for a, b in zip(self.d, o.d)])

    def __sub__(self, o):
        return Dual(self.v - o.v, [a - b for a, b in zip(self.d, o.d)])

    def __mul__(self, o):
        if isinstance(o, Dual):
            return Dual(self.v * o.v, [a * o.v + self.v * b for a, b in zip(self.d, o.d)])
        return Dual(self.v * o, [a * o for a in self.d])

    def exact(self, c):
        return Dual(self.v.exact(c), [a.exact(c) for a in self.d])


# ------------------------------------------------------------------ a problem
def shift(a, dx, dy):
    """a(x + dx, y + dy), 0 outside the image (the guarded load)"""
    H, W = a.shape
    out = np.zeros_like(a)
    ys, yd = (slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0)))
    xs, xd = (slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0)))
    out[yd, xd] = a[ys, xs]
    return out


NBRS = ((-1, 0), (0, -1), (1, 0), (0, 1))


class Case:
    """params: the list of the .t's Inputs{} (0-15 host scalars with SQUARED weights, 16 X, 17 D, 18 Im, 19 / 20 the edge masks), on the global W x H image"""

    def __init__(self, params, name=""):
        self.params, self.name = params, name
        self.hp = np.array([F32(v) for v in params[:16]], F32)
        self.X, self.D, self.Im, self.mR, self.mC = params[16:21]
        self.H, self.W = self.X.shape
        assert self.X.dtype == F32 and self.D.dtype == F32 and self.Im.dtype == F32 and self.mR.dtype == np.uint8 and self.mC.dtype == np.uint8
        h = self.hp.astype(np.float64)
        self.wp, self.ws, self.wg = np.sqrt(h[0]), np.sqrt(h[1]), np.sqrt(h[2])
        self.fx, self.fy, self.ux, self.uy = h[3], h[4], h[5], h[6]
        self.L = h[7:16]
        self.N = self.W * self.H
        ys, xs = np.mgrid[0:self.H, 0:self.W]
        self.xs, self.ys = xs, ys
        # ---- decisions, on the float32 inputs
        X, D = self.X, self.D
        self.pos = D > 0
        self.on = self.pos & (shift(D, -1, 0) > 0) & (shift(D, 0, -1) > 0)                 # BI is evaluated
        valid = self.pos.copy()
        for dx, dy in NBRS:
            valid &= (shift(D, dx, dy) > 0) & (np.abs(X - shift(X, dx, dy)) < GATE)         # (float32 subtraction, float32 comparison)
        self.valid = valid
        self.inner = (xs >= 1) & (xs <= self.W - 2) & (ys >= 1) & (ys <= self.H - 2)
        self.fl = (self.pos.astype(np.uint8) | (valid.astype(np.uint8) << 1))
        # the float32 row weights as every form leaves or rebuilds them: w_g = sqrtf(param) in float32, times the mask byte (one rounding each)
        wg32 = np.sqrt(self.hp[2])
        self.Wt = np.stack([np.where(self.inner, wg32 * self.mR.astype(F32), F32(0)), np.where(self.inner, wg32 * self.mC.astype(F32), F32(0))], -1).astype(F32)
        mr, mc = np.where(self.inner, self.mR, 0).astype(np.uint32), np.where(self.inner, self.mC, 0).astype(np.uint32)
        self.dword = self.fl.astype(np.uint32) | (mr << 8) | (mc << 16)
        self.h = np.where(self.inner, self.wg * self.mR, 0.0)                              # float64 row weights
        self.k = np.where(self.inner, self.wg * self.mC, 0.0)
        self.coef = np.stack([(xs - self.ux) / self.fx, (ys - self.uy) / self.fy, np.ones((self.H, self.W))])      # P's three factors

    # ---- B_I
    def _leaves(self):
        X = self.X.astype(np.float64)
        c, l, u = X, shift(X, -1, 0), shift(X, 0, -1)
        Im = self.Im.astype(np.float64)
        I = Tr(0.5 * Im) + (Tr(shift(Im, -1, 0)) + Tr(shift(Im, 0, -1))).exact(0.25)
        ax = Tr((self.ux - self.xs) / self.fx, k=2)            # a subtraction of exact operands, a quotient
        ay = Tr((self.uy - self.ys) / self.fy, k=2)
        ify, ifx, kxy = Tr(1.0 / self.fy, k=1), Tr(1.0 / self.fx, k=1), Tr(1.0 / (self.fx * self.fy), k=2)
        return c, l, u, I, ax, ay, ify, ifx, kxy

    @functools.lru_cache(maxsize=None)
    def bi_forward(self, rsq=RSQ):
        """G = [d0, d1, d2, BI] as Tr, by the forward-mode tree of eval_BI_vals; also sq (float64) for margins()"""
        c, l, u, I, ax, ay, ify, ifx, kxy = self._leaves()
        one, zero = Tr(1.0), Tr(0.0)
        dc, dl, du = Dual(Tr(c), [one, zero, zero]), Dual(Tr(l), [zero, one, zero]), Dual(Tr(u), [zero, zero, one])
        cl = Dual(diff_inputs(c, l), [one, Tr(-1.0), zero])
        cu = Dual(diff_inputs(c, u), [one, zero, Tr(-1.0)])
        nx = (du * cl) * ify
        ny = (dl * cu) * ifx
        nz = (nx * ax + ny * ay) - (dl * du) * kxy
        sq = nx * nx + ny * ny + nz * nz
        pos = sq.v.v > 0
        inv_v = sq.v.rsqrt(pos, rsq)
        kk = (inv_v.exact(-0.5) / sq.v.where(pos, 1.0)).where(pos, 0.0)
        inv = Dual(inv_v, [(kk * d).where(pos, 0.0) for d in sq.d])
        n0, n1, n2 = inv * nx, inv * ny, inv * nz
        Lc = [Tr(v) for v in self.L]
        B = Dual(Lc[0])
        B = B + n1 * Lc[1]; B = B + n2 * Lc[2]; B = B + n0 * Lc[3]
        B = B + (n0 * n1) * Lc[4]; B = B + (n1 * n2) * Lc[5]
        B = B + (((n0 * n0).exact(-1.0) - n1 * n1) + (n2 * n2).exact(2.0)) * Lc[6]
        B = B + (n2 * n0) * Lc[7]; B = B + (n0 * n0 - n1 * n1) * Lc[8]
        b = B - Dual(I)
        G = [t.where(self.on, 0.0) for t in (b.d[0], b.d[1], b.d[2], b.v)]
        return G, np.where(self.on, sq.v.v, np.nan)

    @functools.lru_cache(maxsize=None)
    def bi_closed(self, rsq=RSQ):
        """the same four numbers by the closed form of eval_BI_pair: dB/dq = h . dn/dq, h = |n|^-1 (g - n^ (g . n^)), g = grad_n^ B"""
        c, l, u, I, ax, ay, ify, ifx, kxy = self._leaves()
        c, l, u = Tr(c), Tr(l), Tr(u)
        cl, cu = diff_inputs(c.v, l.v), diff_inputs(c.v, u.v)
        nx = (u * cl) * ify
        ny = (l * cu) * ifx
        nz = (nx * ax + ny * ay) - (l * u) * kxy
        sq = nx * nx + ny * ny + nz * nz
        pos = sq.v > 0
        inv = sq.rsqrt(pos, rsq)
        n0, n1, n2 = inv * nx, inv * ny, inv * nz
        L = [Tr(v) for v in self.L]
        B = n1 * L[1] + L[0]
        B = B + n2 * L[2]; B = B + n0 * L[3]
        B = B + (n0 * n1) * L[4]; B = B + (n1 * n2) * L[5]
        B = B + (((n0 * n0).exact(-1.0) - n1 * n1) + (n2 * n2).exact(2.0)) * L[6]
        B = B + (n2 * n0) * L[7]; B = B + (n0 * n0 - n1 * n1) * L[8]
        two = lambda t: t.exact(2.0)
        g0 = L[3] + n1 * L[4] - two(L[6]) * n0 + n2 * L[7] + two(L[8]) * n0
        g1 = L[1] + n0 * L[4] + n2 * L[5] - two(L[6]) * n1 - two(L[8]) * n1
        g2 = L[2] + n1 * L[5] + L[6].exact(4.0) * n2 + n0 * L[7]
        gn = g0 * n0 + g1 * n1 + g2 * n2
        h0, h1, h2 = ((inv * (g - n * gn)).where(pos, g) for g, n in ((g0, n0), (g1, n1), (g2, n2)))
        A, Bq, Cq = h0 + h2 * ax, h1 + h2 * ay, h2 * kxy
        uf, lf = u * ify, l * ifx
        G = [A * uf + Bq * lf, Bq * (cu * ifx) - A * uf - Cq * u, A * (cl * ify) - Bq * lf - Cq * l, B - I]
        return [t.where(self.on, 0.0) for t in G], np.where(self.on, sq.v, np.nan)

    def G64(self):
        """[H, W, 4] float64: (dBI/dX(c), dBI/dX(c-ex), dBI/dX(c-ey), BI)"""
        return np.stack([t.v for t in self.bi_forward()[0]], -1)

    # ---- J and what follows from it
    def Gmag(self):
        """the magnitudes of G64()'s entries (the forward-mode tree)"""
        return np.stack([t.m for t in self.bi_forward()[0]], -1)

    def system(self, G=None, Gmag=None):
        """J (6 rows per pixel: fit, sh_h, sh_v, reg_0..2; scipy CSR, float64), |J| and F, from the planes G ([H, W, 4]; default: this reference's own; a test passes the
        DEVICE's planes when only the roundings of the kernel behind them are to count).  Gmag: magnitudes to use for G's entries in |J| and |F| instead of their absolute
        values (Gmag(): when the planes behind a float32 result carry the rounding of the whole BI tree, as the oracle's do)"""
        return System(self, self.G64() if G is None else np.asarray(G, np.float64).reshape(self.H, self.W, 4), Gmag)


class System:
    def __init__(self, cs, G, Gmag=None):
        self.cs, self.G = cs, G
        Gm = np.abs(G) if Gmag is None else np.asarray(Gmag, np.float64)
        H, W, N = cs.H, cs.W, cs.N
        idx = np.arange(N).reshape(H, W)
        rows, cols, vals, mags = [], [], [], []

        def put(row_k, mask, dx, dy, val, mag=None):
            """entries of row kind row_k at the pixels of mask, column = the pixel at (+dx, +dy)"""
            q = idx[mask]
            rows.append(6 * q + row_k); cols.append(q + dy * W + dx); vals.append(np.broadcast_to(val, (H, W))[mask])
            mags.append(np.abs(vals[-1]) if mag is None else np.broadcast_to(mag, (H, W))[mask])

        X, D = cs.X.astype(np.float64), cs.D.astype(np.float64)
        F = np.zeros((H, W, 6))
        put(0, cs.pos, 0, 0, cs.wp)
        F[..., 0] = np.where(cs.pos, cs.wp * (X - D), 0.0)
        Fabs = np.zeros((H, W, 6)); Fabs[..., 0] = np.where(cs.pos, cs.wp * np.abs(X - D), 0.0)      # (one operation on inputs)
        inn = cs.inner
        g = lambda k, dx, dy: shift(G[..., k], dx, dy)
        gm = lambda k, dx, dy: shift(Gm[..., k], dx, dy)
        for rk, w, (ex, ey) in ((1, cs.h, (1, 0)), (2, cs.k, (0, 1))):
            for dx, dy, k, sx, sy, sgn in ((0, 0, 0, 0, 0, 1.0), (-1, 0, 1, 0, 0, 1.0), (0, -1, 2, 0, 0, 1.0), (ex, ey, 0, ex, ey, -1.0), (ex - 1, ey, 1, ex, ey, -1.0), (ex, ey - 1, 2, ex, ey, -1.0)):
                put(rk, inn, dx, dy, sgn * w * g(k, sx, sy), w * gm(k, sx, sy))                   # column (+dx, +dy): partial k of BI at (+sx, +sy)
            F[..., rk] = np.where(inn, w * (g(3, 0, 0) - g(3, ex, ey)), 0.0)
            Fabs[..., rk] = np.where(inn, w * (gm(3, 0, 0) + gm(3, ex, ey)), 0.0)
        for c in range(3):
            co = cs.coef[c]
            put(3 + c, cs.valid, 0, 0, 4.0 * cs.ws * co)
            acc, mag = 4.0 * co * X, 4.0 * np.abs(co * X)
            for dx, dy in NBRS:
                put(3 + c, cs.valid, dx, dy, -cs.ws * shift(co, dx, dy) if c < 2 else -cs.ws)
                con = ((cs.xs + dx - cs.ux) / cs.fx, (cs.ys + dy - cs.uy) / cs.fy, 1.0)[c]       # the neighbour's factor from ITS coordinates (valid: it lies inside)
                acc = acc - con * shift(X, dx, dy); mag = mag + np.abs(con * shift(X, dx, dy))
            F[..., 3 + c] = np.where(cs.valid, cs.ws * acc, 0.0); Fabs[..., 3 + c] = np.where(cs.valid, cs.ws * mag, 0.0)
        rows, cols, vals, mags = (np.concatenate(a) for a in (rows, cols, vals, mags))
        self.J = sp.coo_matrix((vals, (rows, cols)), shape=(6 * N, N)).tocsr()
        self.Jabs = sp.coo_matrix((mags, (rows, cols)), shape=(6 * N, N)).tocsr()
        self.F, self.Fabs = F.reshape(-1), Fabs.reshape(-1)
        self.cost_terms = 0.5 * (F ** 2).sum(-1)                     # [H, W]: a pixel's share of the cost
        self.cost = float(self.cost_terms.sum())
        self.r = -(self.J.T @ self.F)
        self.r_abs = self.Jabs.T @ self.Fabs
        self.diag = np.asarray(self.J.multiply(self.J).sum(0)).ravel()
        self.diag_abs = np.asarray(self.Jabs.multiply(self.Jabs).sum(0)).ravel()

    def jtj(self):
        return (self.J.T @ self.J).tocsr()

    def apply(self, p, ctc=None):
        """(J^T J + CtC) p and its magnitude |J|^T |J| |p| + |CtC p|"""
        p = np.asarray(p, np.float64).ravel()
        out, mag = self.J.T @ (self.J @ p), self.Jabs.T @ (self.Jabs @ np.abs(p))
        if ctc is not None:
            c = np.asarray(ctc, np.float64).ravel()
            out, mag = out + c * p, mag + np.abs(c * p)
        return out, mag


# the terms of the scalars the launches reduce (each a flat vector over the pixels; the scalar is their sum)
def terms_alphaN(r, z=None): r = np.asarray(r, np.float64); return r * (r if z is None else np.asarray(z, np.float64))
def terms_alphaD(p, Ap): return np.asarray(p, np.float64) * np.asarray(Ap, np.float64)
def terms_NS1S2(r, Ap, pre=1.0):
    r, Ap = np.asarray(r, np.float64), np.asarray(Ap, np.float64); m = np.asarray(pre, np.float64)
    return m * r * r, m * r * Ap, m * Ap * Ap
def terms_UT1T2(delta, r, b, p, Ap):
    delta, r, b, p, Ap = (np.asarray(a, np.float64) for a in (delta, r, b, p, Ap))
    return delta * (r + b), p * (r + b), delta * Ap
def terms_model(delta, JtJdelta, b):
    delta = np.asarray(delta, np.float64)
    return delta * np.asarray(JtJdelta, np.float64), delta * np.asarray(b, np.float64)


# ------------------------------------------------------------------ margins
def margins(cs):
    """distance of every decision from its threshold: the smallest | |dX| - 0.01 | over the pairs whose depths are both positive, the smallest positive D, the smallest
    non-zero |n|^2 among the pixels where BI is evaluated (inf where there is none)"""
    X, D = cs.X.astype(np.float64), cs.D.astype(np.float64)
    gate = np.inf
    for dx, dy in ((1, 0), (0, 1)):
        both = cs.pos & (shift(D, dx, dy) > 0)
        if both.any():
            gate = min(gate, float(np.abs(np.abs(X - shift(X, dx, dy))[both] - 0.01).min()))
    sq = cs.bi_forward()[1]
    sq = sq[np.isfinite(sq)]
    return SimpleNamespace(gate=gate, d_pos=float(D[D > 0].min()) if (D > 0).any() else np.inf, sq_zero=int((sq == 0).sum()),
                           sq_pos=float(sq[sq > 0].min()) if (sq > 0).any() else np.inf)


def margins_ok(cs):
    m = margins(cs)
    return m.gate > 1e-5 and not (0 < m.d_pos < 1e-6) and m.sq_pos > 1e-12


# ------------------------------------------------------------------ input families
FAMILIES = ("smooth", "holes", "steps", "masks", "degenerate")
WEIGHTS = {None: (90.7, 37.3, 2.9), "p": (90.7, 0.0, 0.0), "s": (0.0, 37.3, 0.0), "g": (0.0, 0.0, 2.9)}      # w_p, w_s, w_g as the caller passes them (squares of the weights)


def _base(W, H, rng, slope, noise, bumps):
    """a surface whose difference between neighbours is at most slope + 2 noise (the noise is uniform, so the bound is hard)"""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    Wp, Hp = max(W, 8), max(H, 8)
    X = 1.0 + slope * min(Wp, Hp) / (2 * np.pi) * np.sin(2 * np.pi * xs / Wp + 0.3) * np.cos(2 * np.pi * ys / Hp)
    X = X + rng.uniform(-noise, noise, (H, W))
    if bumps:
        X = X + 0.05 * (rng.random((H, W)) < bumps)       # single pixels 5 cm off: they and their four neighbours fail the 0.01 gate by far
    return X


def make(family, W, H, seed=0, only=None):
    """params of one input of `family`: f_x != f_y, a non-integer u_x, u_y off centre, nine random lighting coefficients, three distinct non-square weights
    (`only` in "p", "s", "g": the other two are zero)"""
    rng = np.random.default_rng([seed, W, H, FAMILIES.index(family)])
    fx = 40.0 + 0.85 * W; fy = 1.17 * fx
    ux, uy = 0.47 * W + 0.3, 0.61 * H + 0.2
    L = rng.uniform(-1.0, 1.0, 9)
    wp, ws, wg = WEIGHTS[only]
    steps = family == "steps"
    X = _base(W, H, rng, 5e-4 if steps else 1.5e-3, 2e-4 if steps else 5e-4, 0.05)    # |dX| <= 0.0009 (steps) / 0.0025: with the steps of 0.008 / 0.012 no pair is near the gate
    D = X + 2e-3 * rng.standard_normal((H, W))
    Im = rng.uniform(0.0, 1.0, (H, W))
    mR = (rng.random((H, W)) < 0.9).astype(np.uint8); mC = (rng.random((H, W)) < 0.9).astype(np.uint8)
    seams = [s for s in SEAMS_ONE + SEAMS_PAIR if s < W]
    if family == "smooth":
        if min(W, H) >= 12:
            ys, xs = np.mgrid[0:H, 0:W]
            D[(xs - 0.7 * W) ** 2 + (ys - 0.3 * H) ** 2 < (0.06 * min(W, H)) ** 2] = 0.0
    elif family == "holes":
        if min(W, H) >= 6:
            D[:2, :2] = 0.0; D[:2, -2:] = -1.0; D[-2:, :2] = -0.5; D[-2:, -2:] = 0.0                       # the corners
            D[0, W // 2 - 1:W // 2 + 1] = 0.0; D[-1, W // 3:W // 3 + 2] = -2.0                             # the four borders
            D[H // 2 - 1:H // 2 + 1, 0] = 0.0; D[H // 3:H // 3 + 2, -1] = 0.0
        if W >= 9 and H >= 3:
            D[H - 2, 7:9] = 0.0                                                                            # across an even|odd pair boundary (columns 7|8)
        if min(W, H) >= 9:
            cy, cx = H // 2, W // 2 + 2
            D[cy - 1:cy + 2, cx - 1:cx + 2] = 0.0; D[cy, cx] = X[cy, cx]                                   # one valid pixel alone in a hole
        for s0 in (59, 123):
            if W > s0 + 2:
                D[H // 3:H // 3 + 2, s0:s0 + 3] = 0.0                                                      # across the strip seams
        D[0, 0] = 0.0; D[-1, -1] = -1.0
    elif family == "steps":
        off = np.zeros((H, W))
        cuts = {}                                               # boundary (between column x - 1 and x) -> step
        for x, s in ((W // 3, 0.012), (2 * W // 3, 0.008), (60, 0.012), (61, 0.008), (124, 0.012), (125, 0.008)):
            if 1 <= x < W:
                cuts[x] = cuts.get(x, 0.0) + s
        for x, s in cuts.items():
            off[:, x:] += s
        for y, s in ((H // 2, 0.012), (H // 4, 0.008)):
            if 1 <= y < H:
                off[y:, :] += s
        X = X + off; D = D + off
    elif family == "masks":
        vals = np.array([0, 1, 2, 255], np.uint8)
        mR = rng.choice(vals, (H, W), p=[0.15, 0.55, 0.15, 0.15]); mC = rng.choice(vals, (H, W), p=[0.15, 0.55, 0.15, 0.15])
        both0 = rng.random((H, W)) < 0.1
        mR[both0] = 0; mC[both0] = 0
        mR[H // 3, :] = 0; mC[H // 3, :] = 0; mR[:, W // 3] = 0; mC[:, W // 3] = 0
        for m, v in ((mR, 255), (mC, 2)):
            m[0, :] = v; m[-1, :] = v; m[:, 0] = 1; m[:, -1] = v                                           # non-zero on the border: the guard must ignore them
        if min(W, H) >= 3:
            mR[H // 2, W // 2] = 255; mC[H // 2, W // 2] = 2
    elif family == "degenerate":
        D = np.abs(D)
        X[: max(2, H // 3), : max(2, W // 2)] = 0.0                                                        # X == 0 with D > 0: |n|^2 == 0
        X[H - max(1, H // 3):, W // 3:] = 1.25                                                             # constant X: n_x = n_y = 0
    f32 = lambda a: np.ascontiguousarray(a, F32)
    return [float(wp), float(ws), float(wg), float(fx), float(fy), float(ux), float(uy)] + [float(v) for v in L] + \
           [f32(X), f32(D), f32(Im), np.ascontiguousarray(mR, np.uint8), np.ascontiguousarray(mC, np.uint8)]


@functools.lru_cache(maxsize=None)
def case(family, W, H, seed=0, only=None):
    return Case(make(family, W, H, seed, only), f"{family} {W}x{H} seed {seed}" + (f" only w_{only}" if only else ""))


def branch_hits(cs, family):
    """does the input take the branch its family is named for (None: the size cannot hold it)"""
    X, D = cs.X.astype(np.float64), cs.D
    if family == "smooth":
        return bool(cs.valid.any()) if min(cs.W, cs.H) >= 3 else None
    if family == "holes":
        return bool((D == 0).any() and (D < 0).any()) if cs.N >= 2 else bool((D <= 0).any())
    if family == "steps":
        if cs.W < 3 and cs.H < 4:
            return None
        d = np.concatenate([np.abs(X[:, 1:] - X[:, :-1]).ravel(), np.abs(X[1:] - X[:-1]).ravel()])
        below, above = ((d > 0.006) & (d < 0.01)).any(), ((d > 0.01) & (d < 0.014)).any()
        return bool(below and above) if cs.W >= 3 and cs.H >= 4 else bool(below or above)
    if family == "masks":
        if min(cs.W, cs.H) < 3:
            return None
        big = ((cs.mR >= 2) | (cs.mC >= 2)) & cs.inner
        border = ((cs.mR > 0) | (cs.mC > 0)) & ~cs.inner
        return bool(big.any() and border.any())
    if family == "degenerate":
        if min(cs.W, cs.H) < 3:
            return None
        return margins(cs).sq_zero > 0
    raise KeyError(family)


# ------------------------------------------------------------------ the slab cut
def slab(cs, g0, g1, ghost=2):
    """what a rank that owns the global rows [g0, g1) holds: the local inputs (`ghost` rows of its neighbours on each interior side), the geometry the entry points
    take (H = local rows, row0 / row1 = the owned rows in local numbering, yoff = global row of local row 0, Hg = global height) and `rows`, the slice of a global
    per-row result that the owned rows must equal; `planes` = the local rows on which G / Wt / fl equal the global planes (BI looks one row up, the gate one row up and
    down: the outermost ghost row of an interior side does not)"""
    top, bot = (ghost if g0 > 0 else 0), (ghost if g1 < cs.H else 0)
    lo, hi = g0 - top, g1 + bot
    local = list(cs.params[:16]) + [np.ascontiguousarray(a[lo:hi]) for a in cs.params[16:21]]
    return SimpleNamespace(params=local, W=cs.W, H=hi - lo, row0=top, row1=top + (g1 - g0), yoff=lo, Hg=cs.H, rows=slice(g0, g1), lo=lo, hi=hi,
                           planes=slice(1 if top else 0, (hi - lo) - (1 if bot else 0)))
