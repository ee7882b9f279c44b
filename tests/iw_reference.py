"""Float64 references of the image-stencil plugins (csrc/energy_image_warping*.hip, energy_laplacian_image.hip) for tests/test_gpu_iw_kernels.py, written from
thallo_amd/energies/image_warping.t, laplacian_image.t and the E1 / E5 comments of include/thallo_hip.h -- not from the kernels.  No device is needed here;
tests/test_iw_reference.py checks this module on the CPU (two derivations against each other, the Jacobian against central differences, everything against the
oracle) before any kernel is compared with it.

Everything is numpy float64 computed from the float32 inputs.  Beside every output stands S, the float64 sum of the absolute values of that output's terms at the
granularity of the inputs' products (the scale of sk.tol(k, S)).

The energy (image_warping.t), i a pixel, j = i + d for d in DIRS, R(a) = [[cos a, -sin a], [sin a, cos a]]:
    reg_d(i) = [InBounds(j), Mask_i == 0, Mask_j == 0]  w_reg ((o_i - o_j) - R(a_i)(u_i - u_j))       in R^2
    fit(i)   = [c_i >= 0 (both), Mask_i == 0]           w_fit (o_i - c_i)                              in R^2
J^T J p and J^T F are derived TWICE: residual by residual with array shifts (Stencil / IwRef: every residual's J p, then its three scatters), and as J^T (J p) with J a
scipy.sparse matrix assembled from the residual function itself by complex-step differentiation (IwRef.jacobian) -- a sign error would have to be made in both.

Flat vectors: [Offset 2 pix + c | Angle 2 N + pix] (thallo_hip.h E1), pix = y W + x of the LOCAL image (ghost rows included)."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import shim_kernels as sk
from shim_kernels import F32

TW, TH = 64, 16                     # tiles of the LDS kernels; 64 x 4 for the cost kernel, 64 x 8 for laplacian_image
MARCH_USE = 124                     # output pixels per wave row of the marching kernels
DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1))      # (dx, dy) of reg_px, reg_nx, reg_py, reg_ny


def shift(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx] where that pixel exists, `fill` elsewhere"""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    b[yd, xd] = a[ys, xs]
    return b


def pack(o, a):
    return np.concatenate([np.asarray(o).reshape(-1), np.asarray(a).reshape(-1)])


def unpack(v, W, H):
    N = W * H
    v = np.asarray(v)
    return v[:2 * N].reshape(H, W, 2), v[2 * N:3 * N].reshape(H, W)


def rows_mask(W, H, row0, row1):
    """the entries of a flat vector that the rows [row0, row1) own"""
    m = np.zeros((H, W), bool); m[row0:row1] = True
    return pack(np.repeat(m[..., None], 2, -1), m)


# ------------------------------------------------------------------ M^-1 from the flags byte (thallo_hip.h E1; UrShape on the unit grid)
def diag_from_flags(flags, w_fit, w_reg):
    """raw diag(J^T J) of the two Offset channels and of the Angle channel from the flags byte: 2 cnt w_reg^2 + [fit] w_fit^2 and cnt w_reg^2; 0 where inactive"""
    f = np.asarray(flags).astype(np.int64)
    act, fit, cnt = (f & 1) != 0, (f & 2) != 0, ((f >> 2) & 7).astype(np.float64)
    wf2, wr2 = float(F32(w_fit)) ** 2, float(F32(w_reg)) ** 2
    return np.where(act, 2.0 * cnt * wr2 + fit * wf2, 0.0), np.where(act, cnt * wr2, 0.0), act


def pre_from_flags(flags, w_fit, w_reg):
    """(M^-1 of an Offset channel, of the Angle channel) = guardedInvert of the above; 0 where inactive"""
    do, da, act = diag_from_flags(flags, w_fit, w_reg)
    return np.where(act, sk.guarded_invert(do), 0.0), np.where(act, sk.guarded_invert(da), 0.0)


def pre_from_flags_f32(flags, w_fit, w_reg):
    """the same in float32, operation by operation (IEEE: sqrt and the quotient are correctly rounded): the bits of M^-1 for the exact regime, where M^-1 itself
    is the only inexact factor"""
    f = np.asarray(flags).astype(np.int64)
    act, fit, cnt = (f & 1) != 0, (f & 2) != 0, ((f >> 2) & 7).astype(F32)
    wf2, wr2 = F32(F32(w_fit) * F32(w_fit)), F32(F32(w_reg) * F32(w_reg))
    do = (F32(2.0) * cnt) * wr2
    do = np.where(fit, do + wf2, do).astype(F32)
    da = (cnt * wr2).astype(F32)

    def gi(d):
        s = (F32(1.0) + np.sqrt(d.astype(F32))).astype(F32)
        return (F32(1.0) / (s * s).astype(F32)).astype(F32)
    return np.where(act, gi(do), F32(0.0)).astype(F32), np.where(act, gi(da), F32(0.0)).astype(F32)


def flat_pre(mo, ma):
    """a flat M^-1 vector from the two planes"""
    return pack(np.repeat(np.asarray(mo)[..., None], 2, -1), ma)


# ------------------------------------------------------------------ J^T J of the energy from the planes a kernel is handed
class Stencil:
    """J^T J on a local image from what the PCG kernels are handed: the (cos, sin) plane, the flags byte (bit 0: active, bit 1: fit valid), UrShape (None: the
    unit pixel grid, u_i - u_j = -d exactly) and the two weights.  apply(p) works residual by residual: J p of every residual, then its scatters."""

    def __init__(self, W, H, cs, flags, urshape, w_fit, w_reg):
        self.W, self.H, self.N = W, H, W * H
        cs = np.asarray(cs, np.float64).reshape(H, W, 2)
        self.c, self.s = cs[..., 0], cs[..., 1]
        f = np.asarray(flags).reshape(H, W).astype(np.int64)
        self.act, self.fit = (f & 1) != 0, ((f & 2) != 0) & ((f & 1) != 0)
        self.wf2, self.wr2 = float(F32(w_fit)) ** 2, float(F32(w_reg)) ** 2
        u = None if urshape is None else np.asarray(urshape, np.float64).reshape(H, W, 2)
        self.valid, self.g, self.g_abs = [], [], []
        for dx, dy in DIRS:
            self.valid.append(self.act & shift(self.act, dx, dy, False))
            if u is None:
                dux, duy = np.full((H, W), -float(dx)), np.full((H, W), -float(dy))
            else:
                du = u - shift(u, dx, dy); dux, duy = du[..., 0], du[..., 1]
            # g = R'(a_i)(u_i - u_j), R'(a) = [[-sin, -cos], [cos, -sin]]: d reg_d(i) / d a_i = -w_reg g
            self.g.append(np.stack([-self.s * dux - self.c * duy, self.c * dux - self.s * duy], -1))
            self.g_abs.append(np.stack([np.abs(self.s * dux) + np.abs(self.c * duy), np.abs(self.c * dux) + np.abs(self.s * duy)], -1))
        self.cnt = sum(v.astype(np.int64) for v in self.valid)

    def apply(self, p):
        """(J^T J p, S) as flat vectors"""
        po, pa = unpack(np.asarray(p, np.float64), self.W, self.H)
        oo, oa = np.zeros_like(po), np.zeros_like(pa)
        so, sa = np.zeros_like(po), np.zeros_like(pa)
        for (dx, dy), v, g, ga in zip(DIRS, self.valid, self.g, self.g_abs):
            pj = shift(po, dx, dy)
            E = np.where(v[..., None], (po - pj) - g * pa[..., None], 0.0)                         # J p of reg_d(i) / w_reg
            Ea = np.where(v[..., None], np.abs(po) + np.abs(pj) + ga * np.abs(pa)[..., None], 0.0)
            oo += E - shift(E, -dx, -dy)              # d / d o_i = +1 on reg_d(i), -1 on reg_d(i - d)
            so += Ea + shift(Ea, -dx, -dy)
            oa -= (g * E).sum(-1)                     # d / d a_i = -g
            sa += (ga * Ea).sum(-1)
        oo *= self.wr2; oa *= self.wr2; so *= self.wr2; sa *= self.wr2
        oo += self.wf2 * self.fit[..., None] * po; so += self.wf2 * self.fit[..., None] * np.abs(po)
        return pack(oo, oa), pack(so, sa)

    def diag(self):
        """raw diag(J^T J) as a flat vector"""
        do, da = np.zeros((self.H, self.W)), np.zeros((self.H, self.W))
        for (dx, dy), v, g in zip(DIRS, self.valid, self.g):
            do += v.astype(np.float64) + shift(v, -dx, -dy, False)
            da += np.where(v, (g * g).sum(-1), 0.0)
        do = self.wr2 * do + self.wf2 * self.fit; da = self.wr2 * da
        return pack(np.repeat(do[..., None], 2, -1), da)


# ------------------------------------------------------------------ the problem: residuals, cost, J^T F, flags
class IwRef:
    """one local image of image_warping.t from its float32 inputs (inp: W, H, offset [H, W, 2], angle [H, W], urshape, cons, mask, w_fit, w_reg)"""

    def __init__(self, inp):
        self.inp = inp
        self.W, self.H = W, H = inp.W, inp.H
        self.N = W * H
        self.o, self.a, self.u, self.cn = (np.asarray(x, np.float64) for x in (inp.offset, inp.angle, inp.urshape, inp.cons))
        self.act = np.asarray(inp.mask) == 0                                         # (-0.0 == 0: active)
        self.fit = self.act & (np.asarray(inp.cons)[..., 0] >= 0) & (np.asarray(inp.cons)[..., 1] >= 0)
        self.wf, self.wr = float(F32(inp.w_fit)), float(F32(inp.w_reg))
        self.valid = [self.act & shift(self.act, dx, dy, False) for dx, dy in DIRS]
        self.cnt = sum(v.astype(np.int64) for v in self.valid)
        self.cs = np.stack([np.cos(self.a), np.sin(self.a)], -1)

    # -- the per-step planes
    def flags(self, row0=0, row1=None):
        """the flags byte pcg_init leaves: bit 0 active, bit 1 fit valid, bits 2-4 the count -- on the owned rows; a ghost row carries bit 0 only (the other bits
        depend on rows the local image does not hold: the caller takes them from the neighbour)"""
        row1 = self.H if row1 is None else row1
        f = np.where(self.act, 1 | (self.fit.astype(np.int64) << 1) | (self.cnt << 2), 0)
        g = self.act.astype(np.int64)
        own = np.zeros((self.H, self.W), bool); own[row0:row1] = True
        return np.where(own, f, g).astype(np.uint8)

    def irregular(self, row0=0, row1=None):
        """pixels of rows [row0, row1) whose right / down UrShape neighbour (inside the local image) is not at the exact unit offset"""
        row1 = self.H if row1 is None else row1
        u = np.asarray(self.inp.urshape, F32)
        bad = np.zeros((self.H, self.W), bool)
        dx = (u[:, 1:] - u[:, :-1]).astype(F32); dy = (u[1:] - u[:-1]).astype(F32)
        bad[:, :-1] |= (dx[..., 0] != 1) | (dx[..., 1] != 0)
        bad[:-1] |= (dy[..., 0] != 0) | (dy[..., 1] != 1)
        return int(bad[row0:row1].sum())

    def stencil(self, cs=None, flags=None, grid=False):
        return Stencil(self.W, self.H, self.cs if cs is None else cs, self.flags() if flags is None else flags, None if grid else self.inp.urshape, self.wf, self.wr)

    # -- the residual function (complex arguments allowed: complex-step differentiation)
    def x0(self):
        return pack(self.o, self.a)

    def residuals(self, x, parts=False):
        """F(x): rows ((d N + pix) 2 + c) for the four reg_d, ((4 N + pix) 2 + c) for fit.  parts: (F, sum of the absolute values of each residual's terms)"""
        o, a = unpack(x, self.W, self.H)
        c, s = np.cos(a), np.sin(a)
        out, mag = [], []
        for (dx, dy), v in zip(DIRS, self.valid):
            du = self.u - shift(self.u, dx, dy)
            rot = np.stack([c * du[..., 0] - s * du[..., 1], s * du[..., 0] + c * du[..., 1]], -1)
            out.append(np.where(v[..., None], self.wr * ((o - shift(o, dx, dy)) - rot), 0.0))
            if parts:
                ra = np.stack([np.abs(c * du[..., 0]) + np.abs(s * du[..., 1]), np.abs(s * du[..., 0]) + np.abs(c * du[..., 1])], -1)
                mag.append(np.where(v[..., None], self.wr * (np.abs(o) + np.abs(shift(o, dx, dy)) + ra), 0.0))
        out.append(np.where(self.fit[..., None], self.wf * (o - self.cn), 0.0))
        if parts:
            mag.append(np.where(self.fit[..., None], self.wf * (np.abs(o) + np.abs(self.cn)), 0.0))
            return np.concatenate([f.reshape(-1) for f in out]), np.concatenate([f.reshape(-1) for f in mag])
        return np.concatenate([f.reshape(-1) for f in out])

    def cost_pixels(self):
        """(cost share of every pixel: half the squares of ITS five residuals, S) as [H, W]"""
        F, Fa = self.residuals(self.x0(), parts=True)
        sq = lambda f: 0.5 * (f.reshape(5, self.H, self.W, 2) ** 2).sum((0, 3))
        return sq(F), sq(Fa)

    @functools.lru_cache(maxsize=None)
    def jacobian(self):
        """J = dF/dx at x0 as a sparse matrix, from residuals() alone: Im F(x + i h e) / h is the derivative to rounding (no subtraction), and pixels of one colour
        (x + 2 y) mod 5 share no residual, so 2 x 5 + 1 evaluations give every column"""
        W, H, N, h = self.W, self.H, self.N, 1e-30
        ys, xs = np.mgrid[0:H, 0:W]
        colour = ((xs + 2 * ys) % 5).reshape(-1)
        pix = np.arange(N)
        nbr = [np.where((xs + dx >= 0) & (xs + dx < W) & (ys + dy >= 0) & (ys + dy < H), (ys + dy) * W + xs + dx, -1).reshape(-1) for dx, dy in DIRS]
        rows, cols, vals = [], [], []
        x0 = self.x0().astype(np.complex128)
        for comp in range(2):
            for k in range(5):
                x = x0.copy(); x[2 * pix[colour == k] + comp] += 1j * h
                D = (self.residuals(x).imag / h).reshape(5, N, 2)
                for d in range(5):
                    for owner in ([pix] if d == 4 else [pix, nbr[d]]):          # the residual's own pixel, or its neighbour, has colour k -- never both
                        sel = (owner >= 0) & (colour[np.maximum(owner, 0)] == k)
                        for cc in range(2):
                            rows.append(((d * N + pix[sel]) * 2 + cc)); cols.append(2 * owner[sel] + comp); vals.append(D[d, sel, cc])
        x = x0.copy(); x[2 * N:] += 1j * h                                    # the angles: a residual sees its own pixel's only
        D = (self.residuals(x).imag / h).reshape(5, N, 2)
        for d in range(4):
            for cc in range(2):
                rows.append((d * N + pix) * 2 + cc); cols.append(2 * N + pix); vals.append(D[d, :, cc])
        J = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(10 * N, 3 * N)).tocsr()
        J.eliminate_zeros()
        return J

    # -- J^T F, residual by residual
    def jtf(self):
        """r = -J^T F, S, raw diag(J^T J) as flat vectors (excluded unknowns: 0)"""
        st = self.stencil()
        ro, ra = np.zeros((self.H, self.W, 2)), np.zeros((self.H, self.W))
        so, sa = np.zeros_like(ro), np.zeros_like(ra)
        F, Fa = self.residuals(self.x0(), parts=True)
        F, Fa = F.reshape(5, self.H, self.W, 2), Fa.reshape(5, self.H, self.W, 2)
        for d, (dx, dy) in enumerate(DIRS):
            ro += self.wr * (F[d] - shift(F[d], -dx, -dy)); so += self.wr * (Fa[d] + shift(Fa[d], -dx, -dy))
            ra -= self.wr * (st.g[d] * F[d]).sum(-1); sa += self.wr * (st.g_abs[d] * Fa[d]).sum(-1)
        ro += self.wf * F[4]; so += self.wf * Fa[4]
        return -pack(ro, ra), pack(so, sa), st.diag()

    def excluded(self):
        return ~pack(np.repeat(self.act[..., None], 2, -1), self.act)

    def system(self):
        """everything pcg_init produces on a whole image: r, S_r, diag, pre, z, S_z = pre S_r, the alphaN terms"""
        r, S, diag = self.jtf()
        pre = np.where(self.excluded(), 0.0, sk.guarded_invert(diag))
        return SimpleNamespace(r=r, r_abs=S, diag=diag, pre=pre, z=pre * r, z_abs=pre * S, aN=r * pre * r)


# ------------------------------------------------------------------ one PCG iteration, in every form the kernels have
def delta_update(delta, p_in, p_old, dmode, alpha, alpha2):
    """the delta update a launch carries (thallo_hip.h, pcg_step1's mode): 0: += alpha p_in; 2: += alpha2 p_old, then += alpha p_in; 1: none.  (value, S)"""
    d = np.asarray(delta, np.float64)
    if dmode == 1:
        return d.copy(), np.abs(d)
    t = float(alpha) * np.asarray(p_in, np.float64)
    if dmode == 2:
        t2 = float(alpha2) * np.asarray(p_old, np.float64)
        return d + t2 + t, np.abs(d) + np.abs(t2) + np.abs(t)
    return d + t, np.abs(d) + np.abs(t)


def dmode_of(mode):
    return 1 if mode & 1 else (mode >> 1) & 3


def step1(st, z, z_abs, p_in, delta, p_old, mode, alpha, beta, alpha2=0.0):
    """fused PCGStep3(k-1) + delta update + PCGStep1(k): p = z + beta p_in (first: p = z) on EVERY row of the local image, delta on all rows (the caller looks at
    the owned ones), A p = J^T J p.  z_abs: S of the z handed in (|z|, or M^-1 |r| on the z-free path).  Returns p, S_p, delta, S_d, Ap, S_Ap, and Ap_in = |J^T J| S_p:
    what an error of p costs A p."""
    z, p_in = np.asarray(z, np.float64), np.asarray(p_in, np.float64)
    b = 0.0 if mode & 1 else float(beta)
    p, p_abs = z + b * p_in, np.asarray(z_abs, np.float64) + np.abs(b * p_in)
    d, d_abs = delta_update(delta, p_in, p_old, dmode_of(mode), alpha, alpha2) if delta is not None else (None, None)
    Ap, Ap_abs = st.apply(p)
    return SimpleNamespace(p=p, p_abs=p_abs, delta=d, delta_abs=d_abs, Ap=Ap, Ap_abs=Ap_abs, Ap_in=st.apply(p_abs)[1], alphaD=p * Ap)


def iteration(st, M, r_in, Ap_in, p_in, delta, p_old, mode, alpha, beta, alpha2=0.0):
    """the one-kernel PCG iteration: r = r_in - alpha Ap_in (first: r_in), z = M r, then step1, and the terms of N = r.M r, S1 = r.M Ap, S2 = Ap.M Ap.
    Ap_in None: the recomputing form, Ap_in = J^T J p_in (its S comes back as rc_abs)."""
    r_in, M = np.asarray(r_in, np.float64), np.asarray(M, np.float64)
    rc_abs = None
    if Ap_in is None:
        Ap_in, rc_abs = st.apply(np.asarray(p_in, np.float64))
    if mode & 1:
        r, r_abs = r_in.copy(), np.abs(r_in)
    else:
        t = float(alpha) * np.asarray(Ap_in, np.float64)
        r, r_abs = r_in - t, np.abs(r_in) + np.abs(t)
    o = step1(st, M * r, M * r_abs, p_in, delta, p_old, mode, alpha, beta, alpha2)
    o.r, o.r_abs, o.M, o.rc_abs = r, r_abs, M, rc_abs
    o.N, o.S1, o.S2 = M * r * r, M * r * o.Ap, M * o.Ap * o.Ap
    return o


def sums_terms(M, r, Ap, p):
    """the terms of alphaD, N, S1, S2 from given planes (the device's own, in the tests)"""
    M, r, Ap, p = (np.asarray(x, np.float64) for x in (M, r, Ap, p))
    return p * Ap, M * r * r, M * r * Ap, M * Ap * Ap


def per_pixel(v, W, H):
    """a flat vector's three entries per pixel added up: [H, W]"""
    o, a = unpack(v, W, H)
    return o.sum(-1) + a


# ------------------------------------------------------------------ who adds what up
def tile_blocks(W, H, row0, row1, grid, tw=TW, th=TH):
    """[H, W]: the workgroup of a persistent tile kernel that owns each pixel of rows [row0, row1) (-1 elsewhere).  Tiles tw x th over the owned rows, numbered row by
    row; `grid` workgroups in 8 groups (when grid is a multiple of 8) of contiguous tile ranges, a group's workgroups striding through its range."""
    tx, ty = (W + tw - 1) // tw, (row1 - row0 + th - 1) // th
    nt = tx * ty
    owner = np.full(nt, -1)
    G = 8 if grid >= 8 and grid % 8 == 0 else 1
    per = grid // G
    for b in range(grid):
        g, l = b % G, b // G
        owner[nt * g // G + l:nt * (g + 1) // G:per] = b
    assert (owner >= 0).all()
    out = np.full((H, W), -1)
    ys, xs = np.mgrid[row0:row1, 0:W]
    out[row0:row1] = owner[((ys - row0) // th) * tx + xs // tw]
    return out, int(np.bincount(owner, minlength=grid).max())


def march_blocks(W, H, place, grid):
    """[H, W] workgroup per pixel from thallo_hip_iw_march_place's table (strip, first row, end row per wave; a strip's outputs are 124 columns)"""
    out = np.full((H, W), -1)
    pl = np.asarray(place).reshape(grid, 4, 3)
    for b in range(grid):
        for s, ya, yb in pl[b]:
            if ya < yb:
                assert (out[ya:yb, s * MARCH_USE:(s + 1) * MARCH_USE] == -1).all(), "two waves own one pixel"
                out[ya:yb, s * MARCH_USE:(s + 1) * MARCH_USE] = b
    return out


# ------------------------------------------------------------------ laplacian_image.t (thallo_hip.h E5)
class LapRef:
    """fit = w (X - A); regx = Gx ? X(x, y) - X(x + 1, y) : 0 with Gx = InBounds(x + 1, y + 1) (xguard 0, as shipped) or InBounds(x + 1, y) (xguard 1);
    regy = InBounds(x, y + 1) ? X(x, y) - X(x, y + 1) : 0.  Identity preconditioner."""

    def __init__(self, W, H, X, A, w_fit, xguard):
        self.W, self.H = W, H
        self.X, self.A = np.asarray(X, np.float64).reshape(H, W), np.asarray(A, np.float64).reshape(H, W)
        self.w = float(F32(w_fit))
        ys, xs = np.mgrid[0:H, 0:W]
        self.gx = (xs + 1 < W) if xguard else (xs + 1 < W) & (ys + 1 < H)
        self.gy = ys + 1 < H

    def apply(self, v):
        """(J^T J v, S) as [H, W]"""
        v = np.asarray(v, np.float64).reshape(self.H, self.W)
        out, mag = self.w * (self.w * v), self.w * self.w * np.abs(v)
        for (dx, dy), g in (((1, 0), self.gx), ((0, 1), self.gy)):
            D = np.where(g, v - shift(v, dx, dy), 0.0); Da = np.where(g, np.abs(v) + np.abs(shift(v, dx, dy)), 0.0)
            out = out + D - shift(D, -dx, -dy); mag = mag + Da + shift(Da, -dx, -dy)
        return out, mag

    def jacobian(self):
        N = self.W * self.H
        I = sp.identity(N, format="csr")
        blocks = [self.w * I]
        for (dx, dy), g in (((1, 0), self.gx), ((0, 1), self.gy)):
            pix = np.flatnonzero(g.reshape(-1))
            S = sp.coo_matrix((np.ones(pix.size), (pix, pix + dx + dy * self.W)), shape=(N, N)).tocsr()
            blocks.append(sp.diags(g.reshape(-1).astype(np.float64)) @ I - S)
        return sp.vstack(blocks).tocsr()

    def system(self):
        """r = -J^T F, S, raw diag"""
        fit, fa = self.w * (self.w * (self.X - self.A)), self.w * self.w * (np.abs(self.X) + np.abs(self.A))
        lap, la = self.apply(self.X)
        lap, la = lap - self.w * self.w * self.X, la - self.w * self.w * np.abs(self.X)
        diag = self.w ** 2 + self.gx + shift(self.gx, -1, 0, False) + self.gy + shift(self.gy, 0, -1, False)
        return -(fit + lap), fa + la, diag.astype(np.float64)

    def cost_pixels(self):
        f = self.w * (self.X - self.A); fa = self.w * (np.abs(self.X) + np.abs(self.A))
        out, mag = f * f, fa * fa
        for (dx, dy), g in (((1, 0), self.gx), ((0, 1), self.gy)):
            D = np.where(g, self.X - shift(self.X, dx, dy), 0.0); Da = np.where(g, np.abs(self.X) + np.abs(shift(self.X, dx, dy)), 0.0)
            out = out + D * D; mag = mag + Da * Da
        return 0.5 * out, 0.5 * mag


LAP_CASES = [(1, 1), (2, 1), (1, 9), (63, 7), (64, 8), (65, 9), (130, 17)]


def lap_inputs(W, H, exact=False):
    rng = np.random.default_rng(1000 * W + H)
    if exact:
        return rng.integers(-8, 9, (H, W)).astype(F32), rng.integers(-8, 9, (H, W)).astype(F32), 0.5
    return rng.standard_normal((H, W)).astype(F32), rng.uniform(0, 1, (H, W)).astype(F32), 0.2


# ------------------------------------------------------------------ cases and input makers
STAMP = np.array([[0, 0, 0, 0, 0, 0, 0],          # 1 = masked.  (2, 1) and (2, 4): isolated active pixels (count 0); (1, 2): count 1; (5, 3): count 2; the rim: 3 and 4
                  [0, 1, 0, 1, 1, 1, 0],
                  [1, 0, 1, 1, 0, 1, 0],
                  [0, 1, 0, 1, 1, 1, 0],
                  [0, 0, 0, 0, 0, 0, 0],
                  [0, 1, 1, 0, 1, 0, 0],
                  [0, 0, 0, 0, 0, 0, 0]], bool)

# name: W, H, UrShape ("unit", "shift", "moved", "shear"), angle amplitude, exact regime, owned row ranges beside the whole image, what the mask carries
CASES = {
    "t1x1":    (1, 1, "unit", 3.0, False, [], ()),
    "t2x2":    (2, 2, "unit", 0.1, False, [(0, 1), (1, 2)], ()),
    "t63x15":  (63, 15, "unit", 3.0, False, [(1, 15)], ("stamps",)),
    "t64x16":  (64, 16, "unit", 0.1, False, [(1, 15), (0, 15), (1, 16)], ("stamps", "row")),
    "t65x17":  (65, 17, "shift", 3.0, False, [(1, 16), (1, 17)], ("stamps", "column")),
    "t65x3":   (65, 3, "unit", 3.0, False, [(1, 2)], ()),
    "t130x33": (130, 33, "unit", 3.0, False, [(1, 32)], ("stamps", "row", "column")),
    "m2x7":    (2, 7, "unit", 3.0, False, [(1, 7)], ()),
    "m122x5":  (122, 5, "unit", 0.1, False, [(0, 4)], ("stamps",)),
    "m124x4":  (124, 4, "unit", 3.0, False, [(1, 4), (1, 3)], ("stamps", "row")),
    "m126x9":  (126, 9, "unit", 3.0, False, [(1, 8)], ("stamps", "column")),
    "m126x3":  (126, 3, "unit", 3.0, False, [(1, 2)], ()),
    "m248x3":  (248, 3, "unit", 0.1, False, [], ("strip",)),
    "m250x13": (250, 13, "shift", 3.0, False, [(1, 12)], ("stamps", "row", "column")),
    "moved":   (66, 18, "moved", 3.0, False, [(1, 17)], ("stamps",)),
    "shear":   (34, 9, "shear", 3.0, False, [(1, 9)], ("stamps",)),
    "x130x20": (130, 20, "unit", 0.0, True, [(1, 19)], ("stamps", "row")),
    "x250x7":  (250, 7, "unit", 0.0, True, [(1, 6)], ("stamps", "column")),
    "x65x17":  (65, 17, "unit", 0.0, True, [(1, 17)], ("stamps",)),
}


def stamp_sites(W, H):
    """where the 7 x 7 stamp goes: the image corner, every tile seam and strip seam the image has (clipped to the image)"""
    sites = [(0, 0)]
    if W > TW + 3: sites.append((TW - 3, 0))
    if H > TH + 3: sites.append((8, TH - 3))
    if W > TW + 3 and H > TH + 3: sites.append((TW - 4, TH - 4))
    if W > MARCH_USE + 3: sites.append((MARCH_USE - 3, max(0, H - 7)))
    if W > 2 * TW + 1: sites.append((2 * TW - 5, min(3, H - 1)))
    return sites


@functools.lru_cache(maxsize=None)
def case(name):
    W, H, ur, amp, exact, rows, what = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + W * 131 + H)
    ys, xs = np.mgrid[0:H, 0:W]
    grid = np.stack([xs, ys], -1).astype(F32)
    u = grid.copy()
    if ur == "shift": u += F32(4096.0)                                    # the unit grid, a large integer away
    if ur == "moved": u[H // 2, W // 2] += F32(0.25)                      # one pixel off the grid
    if ur == "shear": u[..., 0] += F32(0.25) * grid[..., 1]
    mask = np.zeros((H, W), F32)
    if "stamps" in what:
        for x0, y0 in stamp_sites(W, H):
            hh, ww = min(7, H - y0), min(7, W - x0)
            mask[y0:y0 + hh, x0:x0 + ww][STAMP[:hh, :ww]] = F32(255.0)
    if "row" in what: mask[H // 2 + 1, :] = F32(1e-30)                    # a fully masked row (any nonzero value masks)
    if "column" in what: mask[:, min(W - 1, MARCH_USE + 1) if W > MARCH_USE else W // 3] = F32(255.0)
    if "strip" in what: mask[:, MARCH_USE:2 * MARCH_USE] = F32(255.0)     # a fully masked strip
    free = np.argwhere(mask == 0)
    for y, x in free[rng.choice(len(free), max(1, len(free) // 16), replace=False)]:
        mask[y, x] = F32(-0.0)                                            # -0.0 == 0: active
    if exact:
        off = (grid + rng.integers(-3, 4, (H, W, 2))).astype(F32)
        ang = np.zeros((H, W), F32)
        w_fit, w_reg = 2.0, 0.5
    else:
        off = (grid + rng.uniform(-0.5, 0.5, (H, W, 2))).astype(F32)
        ang = rng.uniform(-amp, amp, (H, W)).astype(F32)
        w_fit, w_reg = 10.0, 0.1
    cons = np.full((H, W, 2), -1.0, F32)
    pick = rng.random((H, W)) < 0.15                                      # constrained pixels, under the mask too
    cons[pick] = (grid[pick] + rng.integers(0, 3, (int(pick.sum()), 2))).astype(F32)
    flat = cons.reshape(-1, 2)
    order = rng.permutation(W * H)
    specials = [(0.0, 0.0), (-0.0, 5.0), (3.0, -1e-3), (-1.0, 2.0)]        # exactly 0; -0.0 is >= 0; one component negative (twice)
    for k, v in zip(order, specials):
        flat[k] = np.array(v, F32)
    if "stamps" in what and W >= 7 and H >= 7:
        cons[2, 1] = (1.0, 2.0)                                           # one isolated pixel constrained, the other (2, 4) not
        cons[2, 4] = (-1.0, -1.0)
        cons[1, 1] = (1.0, 1.0)                                           # a constrained pixel under the mask
    return SimpleNamespace(name=name, W=W, H=H, offset=off, angle=ang, urshape=u, cons=cons, mask=mask, w_fit=w_fit, w_reg=w_reg, exact=exact, rows=list(rows), grid=ur in ("unit", "shift"))


@functools.lru_cache(maxsize=None)
def ref(name):
    return IwRef(case(name))


def row_ranges(name):
    c = case(name)
    return [(0, c.H)] + c.rows


def params(c):
    """the oracle's parameter list"""
    return [c.offset.copy(), c.angle.copy(), c.urshape.copy(), c.cons.copy(), c.mask.copy(), float(c.w_fit), float(c.w_reg)]


def planes(name, seed, exact=None):
    """random float32 planes for the iteration kernels of a case, zero at excluded unknowns: r, Ap, p, p_old, delta (rounded regime: standard normal; exact regime:
    small integers) -- not solver state, so that a bound covers the roundings of the one launch under test"""
    R = ref(name)
    exact = case(name).exact if exact is None else exact
    rng = np.random.default_rng(seed)
    keep = ~R.excluded()
    mk = (lambda: rng.integers(-2, 3, 3 * R.N).astype(F32)) if exact else (lambda: rng.standard_normal(3 * R.N).astype(F32))
    return SimpleNamespace(**{k: np.where(keep, mk(), F32(0)).astype(F32) for k in ("r", "Ap", "p", "p_old", "delta", "z")})


def exact_scalars():
    """(alphaN, alphaD, betaN) words whose quotients are exact: alpha = 1/2, beta = 1/4; and the pair of iteration k - 2: alpha2 = 2"""
    return F32(2.0), F32(4.0), F32(0.5), F32(4.0), F32(2.0)


def rounded_scalars():
    return F32(1.7), F32(2.9), F32(0.6), F32(1.3), F32(3.1)
