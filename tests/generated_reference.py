"""One plain float64 reference for the generated front-end's kernels (csrc/dsl_codegen.cpp), used by tests/test_generated_reference.py on the CPU and by
tests/test_gpu_generated_kernels.py against the device.  Nothing here needs a device, the library or the front-end.

An Energy is a .t file of tests/energies/ with its inputs and a residual function F(x) in numpy -- x = every unknown image, flattened and concatenated in declaration
order; F is complex-capable.  A Reference is what the three operations of a generated plugin must leave for it:

    F(x), J = dF/dx by complex-step differentiation (exact to rounding: no subtraction), excluded unknowns as constants (zero columns, no row in r or Ap);
    cost = 0.5 |F|^2,  r = -J^T F,  diag = sum J^2,  pre = 1 / (1 + sqrt(diag))^2 (1 without the preconditioner),  Ap = J^T (J p);
    the magnitude companions |J|^T |F| and |J|^T (|J| |p|) against which errors are scaled, and the number of terms behind every element.

The float build receives the float32-rounded inputs, so the reference is evaluated ON those (Energy(..., dbl=False) rounds once, here); the double build gets them as
they are.  The F functions of tests/test_gpu_example_energies.py live here; that file imports them back."""
import functools
import os

import numpy as np
import scipy.sparse as sps

ENERGIES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energies")
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


# worst error / (eps x companion) an MI355X run of tests/test_gpu_generated_kernels.py recorded for the NONLINEAR energies (its RATIOS table; the run, its date and
# commit: profiles/generated_kernels/README.md).  The GPU test allows twice the figure; the CPU mutation check holds every mutant to ten times that bound.
K_EVAL_MEASURED = {
    ("embedded_nodes", "f32"): {"r": 364.44, "diag": 2.16, "Ap": 2.92, "cost": 1.42}, ("embedded_nodes", "f64"): {"r": 1129.58, "diag": 3.98, "Ap": 4.21, "cost": 3.10},
    ("flow_sample", "f32"): {"r": 5.18, "diag": 1.55, "Ap": 14.55, "cost": 0.95}, ("flow_sample", "f64"): {"r": 2.96, "diag": 2.00, "Ap": 3.24, "cost": 1.24},
    ("robust_plane", "f32"): {"r": 9.62, "diag": 2.87, "Ap": 4.13, "cost": 1.37}, ("robust_plane", "f64"): {"r": 7.41, "diag": 3.92, "Ap": 6.09, "cost": 2.19},
    ("volume_arap", "f32"): {"r": 11.06, "diag": 4.31, "Ap": 3.20, "cost": 2.01}, ("volume_arap", "f64"): {"r": 3.73, "diag": 6.58, "Ap": 4.04, "cost": 3.82},
    ("image_warping", "f32"): {"r": 4.11, "diag": 3.96, "Ap": 3.76, "cost": 0.77}, ("image_warping", "f64"): {"r": 3.30, "diag": 5.10, "Ap": 4.02, "cost": 0.00},
    ("shape_from_shading", "f32"): {"r": 2073.68, "diag": 29.51, "Ap": 517.78, "cost": 3.15}, ("shape_from_shading", "f64"): {"r": 905.65, "diag": 44.54, "Ap": 440.94, "cost": 2.65},
    ("arap_mesh_deformation", "f32"): {"r": 5.28, "diag": 5.68, "Ap": 4.37, "cost": 0.70}, ("arap_mesh_deformation", "f64"): {"r": 3.60, "diag": 4.67, "Ap": 3.63, "cost": 0.00},
    ("bundle_adjustment", "f32"): {"r": 829.78, "diag": 464.06, "Ap": 1724.93, "cost": 3.08}, ("bundle_adjustment", "f64"): {"r": 399.09, "diag": 17.00, "Ap": 6.22, "cost": 2.62},
    ("lp_smooth", "f32"): {"r": 2.62, "diag": 2.23, "Ap": 3.30, "cost": 1.32},
    ("layer_sample", "f32"): {"r": 298.72, "diag": 0.0, "Ap": 0.0, "cost": 0.46},
    ("cotan_smooth", "f32"): {"r": 7.11, "diag": 4.19, "Ap": 9.38, "cost": 0.14}, ("cotan_smooth", "f64"): {"r": 8.35, "diag": 5.84, "Ap": 10.50, "cost": 2.09},
}


def k_eval(e):
    """k_eval per quantity ("r", "diag", "Ap") for an Energy: the stated operation count for a linear energy, twice the recorded figure for a nonlinear one, None where
    nothing is recorded yet"""
    if e.k_eval is not None: return {"r": float(e.k_eval), "diag": float(e.k_eval), "Ap": float(e.k_eval), "cost": None}      # (cost: derived from k_eval by the test)
    m = K_EVAL_MEASURED.get((e.name, "f64" if e.dbl else "f32"))
    return None if m is None else {q: 2.0 * v for q, v in m.items()}


def rnd32(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ------------------------------------------------------------------ residual functions (complex-capable; all arguments float64 / int arrays)
def gradient_paste_F(W, H, T):
    """tests/energies/gradient_paste.t: e_right, e_left, e_down, e_up = (X - X_nb) - (T - T_nb) where the neighbour is inside the image, else 0"""
    def F(x):
        X = x.reshape(H, W, 4); out = []
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            r = np.zeros_like(X)
            ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
            yn, xn = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
            r[ys, xs] = (X[ys, xs] - X[yn, xn]) - (T[ys, xs] - T[yn, xn])
            out.append(r.reshape(-1))
        return np.concatenate(out)
    return F


def weighted_laplacian_F(W, H, A, Wt, w_fit):
    """tests/energies/weighted_laplacian.t: fit = w_fit (X - A); regx, regy = Wt (X - X_nb) towards +x / +y where that neighbour exists"""
    def F(x):
        X = x.reshape(H, W, 2); out = [(w_fit * (X - A)).reshape(-1)]
        for dx, dy in ((1, 0), (0, 1)):
            r = np.zeros_like(X)
            r[:H - dy, :W - dx] = Wt[:H - dy, :W - dx, None] * (X[:H - dy, :W - dx] - X[dy:, dx:])
            out.append(r.reshape(-1))
        return np.concatenate(out)
    return F


def cotan_smooth_F(N, v, A, w_fit, w_reg):
    def F(x):
        X = x.reshape(N, 3)
        def cot(p, q, apex):
            a, b = p - apex, q - apex
            c = np.cross(a, b)
            return (a * b).sum(-1) / np.sqrt((c * c).sum(-1))
        p0, p1, p2, p3 = X[v[0]], X[v[1]], X[v[2]], X[v[3]]
        wgt = 0.5 * (cot(p0, p1, p2) + cot(p0, p1, p3))
        return np.concatenate([(w_fit * (X - A)).reshape(-1), (w_reg * wgt[:, None] * (p1 - p0)).reshape(-1)])
    return F


def robust_plane_F(N, T, Nrm, nb, w_rob):
    def F(x):
        X = x[:3 * N].reshape(N, 3); R = x[3 * N:]
        d = (Nrm * (X - T)).sum(-1)
        return np.concatenate([R * R * d, w_rob * (1.0 - R * R), (0.3 * (X - X[nb])).reshape(-1)])
    return F


def rotate3d(a, v):
    """lib.t:123-137 (Euler angles alpha, beta, gamma -> R v), on (..., 3) arrays; complex-capable"""
    ca, cb, cg, sa, sb, sg = np.cos(a[..., 0]), np.cos(a[..., 1]), np.cos(a[..., 2]), np.sin(a[..., 0]), np.sin(a[..., 1]), np.sin(a[..., 2])
    m = [cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca, sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca, -sb, cb * sa, cb * ca]
    return np.stack([m[0] * v[..., 0] + m[1] * v[..., 1] + m[2] * v[..., 2], m[3] * v[..., 0] + m[4] * v[..., 1] + m[5] * v[..., 2],
                     m[6] * v[..., 0] + m[7] * v[..., 1] + m[8] * v[..., 2]], -1)


def volume_arap_F(W, H, D, Rest, Tgt, w_fit, w_reg):
    n = W * H * D * 3
    def F(x):
        P = x[:n].reshape(D, H, W, 3); A = x[n:].reshape(D, H, W, 3)
        held = Tgt[..., 0] >= -999999.9
        out = [np.where(held[..., None], w_fit * (P - Tgt), 0.0).reshape(-1)]
        for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            r = np.zeros_like(P)
            s = (slice(max(0, -dz), D - max(0, dz)), slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))
            t = (slice(max(0, dz), D - max(0, -dz)), slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx)))
            r[s] = w_reg * ((P[s] - P[t]) - rotate3d(A[s], Rest[s] - Rest[t]))
            out.append(r.reshape(-1))
        return np.concatenate(out)
    return F


def two_domains_F(N, U, T):
    def F(x):
        S, P = x[:U], x[U:]
        fit = (S[None, :] + P[:, None] - T[:, None])          # element (n, u); the order of the residuals does not matter to J^T J
        return np.concatenate([fit.reshape(-1), 0.5 * P])
    return F


def conv2d_blur(W, H, KS, Ker, X):
    c = KS // 2
    out = np.zeros((H, W), dtype=X.dtype)
    for ky in range(KS):
        for kx in range(KS):
            out[c:H - c, c:W - c] += Ker[ky, kx] * X[ky:H - 2 * c + ky, kx:W - 2 * c + kx]
    return out


def conv2d_wide_F(W, H, KS, Ker, B, leak_at=None):
    """tests/energies/conv2d_wide.t: data = blur(X) - B where the whole window is inside the image, else 0; reg = 0.05 X.
    leak_at = (x, y), a pixel of the border band (the reference's guarded-load mutant): the window is evaluated there on clamped pixel positions instead of giving 0."""
    c = KS // 2
    def F(x):
        X = x.reshape(H, W)
        data = np.zeros((H, W), dtype=X.dtype)
        data[c:H - c, c:W - c] = (conv2d_blur(W, H, KS, Ker, X) - B)[c:H - c, c:W - c]
        if leak_at is not None:
            lx, ly = leak_at
            ys, xs = np.clip(np.arange(ly - c, ly + c + 1), 0, H - 1), np.clip(np.arange(lx - c, lx + c + 1), 0, W - 1)
            data[ly, lx] = (Ker * X[np.ix_(ys, xs)]).sum() - B[ly, lx]
        return np.concatenate([data.reshape(-1), 0.05 * x])
    return F


def rigid_fit_F(N, Rest, Goal):
    def F(x):
        Shift, Euler = x[:3], x[3:]
        r = rotate3d(np.broadcast_to(Euler, (N, 3)).astype(x.dtype), Rest.astype(x.dtype)) + Shift - Goal
        return np.where((Goal[:, :1] >= -999999.9), r, 0.0).reshape(-1)
    return F


def embedded_nodes_F(N, a, b, Rest, Goal, w_fit, w_reg, w_rot):
    def F(x):
        Off = x[:3 * N].reshape(N, 3); M = x[3 * N:].reshape(N, 3, 3)
        fit = np.where(Goal[:, :1] >= -999999.9, w_fit * (Off - Goal), 0.0)
        d = Rest[b] - Rest[a]
        edge = (Off[b] - Off[a]) - np.einsum("eij,ej->ei", M[a], d.astype(x.dtype))
        c0, c1, c2 = M[:, :, 0], M[:, :, 1], M[:, :, 2]
        dot = lambda u, v: (u * v).sum(-1)
        rot = w_rot * np.stack([dot(c0, c1), dot(c0, c2), dot(c1, c2), dot(c0, c0) - 1, dot(c1, c1) - 1, dot(c2, c2) - 1], -1)
        return np.concatenate([fit.reshape(-1), (w_reg * edge).reshape(-1), rot.reshape(-1)])
    return F


def graph2d_F(W, H, data, mask, right, down, w_fit):
    """tests/energies/graph2d.t, the rows test_gpu_frontend.py states for scipy: w_fit mask (X - data); 0.5 (X - X(right(x, y), y)); X - X(x, down(x, y))"""
    yy, xx = np.mgrid[0:H, 0:W]
    def F(x):
        X = x.reshape(H, W)
        return np.concatenate([(w_fit * mask * (X - data)).reshape(-1), (0.5 * (X - X[yy, right])).reshape(-1), (X - X[down, xx]).reshape(-1)])
    return F


def bilinear(im, x, y, clamp=False):
    """Image:sample (thallo.t:899-907) in float64: corners floor / ceil, 0 outside the image (clamp: the clamped neighbour instead -- the guarded-load mutant)"""
    H, W = im.shape
    x0, x1, y0, y1 = np.floor(x).astype(int), np.ceil(x).astype(int), np.floor(y).astype(int), np.ceil(y).astype(int)
    def get(xx, yy):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(ok | clamp, im[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0.0)
    xn, yn = x - x0, y - y0
    u = (1 - xn) * get(x0, y0) + xn * get(x1, y0)
    b = (1 - xn) * get(x0, y1) + xn * get(x1, y1)
    return (1 - yn) * u + yn * b


def flow_sample_F(W, H, src, dst, ddx, ddy, w_fit, w_reg, leak_at=None):
    """tests/energies/flow_sample.t: w_fit (src_c - dst_c:sample(x + u, y + v)) for the two channels (src_1 = 0.5 src), w_reg (flow - flow_nb) towards +x / +y.
    The partials of a SampledImage are the samples of its two derivative IMAGES (thallo.t:5812-5816), not the slope of the bilinear patch: a complex perturbation
    of the position is carried through them."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    def sample(c, px, py):
        rx, ry = np.real(px), np.real(py)
        v = bilinear(dst[..., c], rx, ry)
        if leak_at is not None:          # (x, y): the samples of that pixel read clamped neighbours where they leave the image
            v = v.copy(); v[leak_at[1], leak_at[0]] = bilinear(dst[..., c], rx, ry, clamp=True)[leak_at[1], leak_at[0]]
        if np.iscomplexobj(px) or np.iscomplexobj(py):
            v = v + bilinear(ddx[..., c], rx, ry) * (px - rx) + bilinear(ddy[..., c], rx, ry) * (py - ry)
        return v
    def F(x):
        f = x.reshape(H, W, 2); px, py = xx + f[..., 0], yy + f[..., 1]
        r = [w_fit * (src - sample(0, px, py)), w_fit * (0.5 * src - sample(1, px, py))]
        sx = np.zeros_like(f); sx[:, :-1] = w_reg * (f[:, :-1] - f[:, 1:])
        sy = np.zeros_like(f); sy[:-1] = w_reg * (f[:-1] - f[1:])
        return np.concatenate([r[0].ravel(), r[1].ravel(), sx.ravel(), sy.ravel()])
    return F


# ------------------------------------------------------------------ energies
class Energy:
    """file, dims, params (slot order: float64 arrays for thallo_float / float arrays -- already rounded for the float build --, int32 arrays, Python floats for Params),
    the unknowns' slots, F, free (bool per unknown: False = excluded), precond (the file's UsePreconditioner), and k_eval (linear energies: stated next to the case; None: nonlinear, measured)."""

    def __init__(self, name, file, dims, params, unknown_slots, F, free=None, precond=True, k_eval=None, dbl=False, guards=False, f32_slots=()):
        self.name, self.file, self.dims, self.params, self.unknown_slots, self.F, self.precond, self.k_eval, self.dbl = name, file, tuple(dims), params, unknown_slots, F, precond, k_eval, dbl
        self.x0 = np.concatenate([np.asarray(params[k], np.float64).reshape(-1) for k in unknown_slots])
        self.n = self.x0.size
        self.free = np.ones(self.n, bool) if free is None else np.asarray(free, bool)
        self.eps = EPS64 if dbl else EPS32
        self.index_slots = [k for k, p in enumerate(params) if isinstance(p, np.ndarray) and p.dtype == np.int32]
        self.guards = guards
        self.f32_slots = tuple(f32_slots)          # arrays declared with the fixed type `float`: floats in the double build too
        self.path = os.path.join(ENERGIES, file)


def _q(dbl):
    return (lambda a: np.asarray(a, np.float64)) if dbl else rnd32


def gradient_paste(W, H, dbl=False):
    """k_eval = 4: (X - Xn), (T - Tn), their difference, the product with the partial (+-1: exact)"""
    rng = np.random.default_rng([5, W, H]); q = _q(dbl)
    T, X0 = q(rng.uniform(0, 1, (H, W, 4))), q(rng.uniform(0, 1, (H, W, 4)))
    M = np.ones((H, W)); M[2:9, 3:12] = 0.0
    if H > 5 and W > 6: M[5, 6] = 1.0          # a region with a pinned pixel inside
    if M.all(): M[H // 2:, W // 2:] = 0.0       # (images smaller than the region's corner: the far quadrant is free)
    return Energy("gradient_paste", "gradient_paste.t", (W, H), [X0, T, M], [0], gradient_paste_F(W, H, T), free=np.repeat(M.reshape(-1) == 0, 4), precond=False, k_eval=4, dbl=dbl,
                  guards=True, f32_slots=(2,))


def weighted_laplacian(W, H, dbl=False):
    """k_eval = 4: X - Xn, the product with Wt, the partial Wt (exact), the product with the partial; the fit term: X - A, times w_fit, times the partial"""
    rng = np.random.default_rng([3, W, H]); q = _q(dbl)
    A = q(rng.uniform(0, 1, (H, W, 2))); Wt = rnd32(rng.uniform(0.5, 1.5, (H, W)))
    Mask = (rng.uniform(0, 1, (H, W)) < 0.1).astype(np.float64)
    X0 = q(A + 0.3 * rng.standard_normal(A.shape)); w_fit = float(np.float32(0.7))
    return Energy("weighted_laplacian", "weighted_laplacian.t", (W, H), [X0, A, Wt, Mask, w_fit], [0], weighted_laplacian_F(W, H, A, Wt, w_fit),
                  free=np.repeat(Mask.reshape(-1) == 0, 2), k_eval=4, dbl=dbl, guards=True, f32_slots=(2, 3))


def weighted_laplacian_rows(W, H, dbl=False):
    """the same energy with J written out as scipy rows (no complex step): for images too large to differentiate column by column"""
    e = weighted_laplacian(W, H, dbl)
    X0, A, Wt, Mask, w_fit = e.params
    n = 2 * W * H; pix = np.arange(W * H).reshape(H, W)
    blocks = [sps.identity(n, format="csr") * w_fit]
    for dx, dy in ((1, 0), (0, 1)):
        ok = np.zeros((H, W), bool); ok[:H - dy, :W - dx] = True
        src, dst, w = pix[ok], pix[ok] + dy * W + dx, Wt[ok]
        rr = np.concatenate([2 * src + c for c in (0, 1)])
        blocks.append(sps.csr_matrix((np.concatenate([w, w, -w, -w]), (np.concatenate([rr, rr]), np.concatenate([rr, np.concatenate([2 * dst + c for c in (0, 1)])]))), shape=(n, n)))
    e.J_rows = (sps.vstack(blocks) @ sps.diags(e.free.astype(np.float64))).tocsc()
    e.J_rows.eliminate_zeros()
    return e


def cotan_smooth(nx=9, ny=7, dbl=False, redirect=None):
    rng = np.random.default_rng(8); q = _q(dbl)
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    A = np.stack([gx, gy, 0.3 * np.sin(0.7 * gx) * np.cos(0.5 * gy)], -1).reshape(-1, 3)
    X0 = q(A + 0.05 * rng.standard_normal(A.shape)); A = q(A)
    vid = lambda i, j: j * nx + i
    e = [(vid(i, j), vid(i + 1, j), vid(i, j + 1), vid(i + 1, j - 1)) for j in range(1, ny - 1) for i in range(nx - 1)]
    v = [np.array([t[k] for t in e], np.int32) for k in range(4)]
    if redirect is not None: v[redirect[0]][redirect[1]] += 1
    N, E = A.shape[0], len(e)
    w_fit, w_reg = float(np.float32(0.8)), float(np.float32(0.6))
    return Energy("cotan_smooth", "cotan_smooth.t", (N, E), [w_fit, w_reg, X0, A, v[0], v[1], v[2], v[3]], [2], cotan_smooth_F(N, v, A, w_fit, w_reg), dbl=dbl)


def robust_plane(N=60, dbl=False, redirect=None):
    rng = np.random.default_rng(12); q = _q(dbl)
    T = q(rng.uniform(-1, 1, (N, 3)))
    Nrm = rng.standard_normal((N, 3)); Nrm = q(Nrm / np.linalg.norm(Nrm, axis=1, keepdims=True))
    X0 = q(T + 0.2 * rng.standard_normal((N, 3))); R0 = q(rng.uniform(0.6, 1.0, N))
    nb = rng.permutation(N).astype(np.int32)
    if redirect is not None: nb[redirect[1]] = (nb[redirect[1]] + 1) % N
    w_rob = float(np.float32(0.35))
    return Energy("robust_plane", "robust_plane.t", (N,), [X0, R0, T, Nrm, w_rob, nb], [0, 1], robust_plane_F(N, T, Nrm, nb, w_rob), dbl=dbl)


def volume_arap(W=5, H=4, D=3, dbl=False):
    rng = np.random.default_rng(21); q = _q(dbl)
    gz, gy, gx = np.meshgrid(np.arange(D, dtype=np.float64), np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    Rest = np.stack([gx, gy, gz], -1)
    Tgt = np.full_like(Rest, -1e6)
    Tgt[0, :, 0] = Rest[0, :, 0]; Tgt[D - 1, :, W - 1] = Rest[D - 1, :, W - 1] + np.array([0.6, 0.2, -0.3])
    Tgt = q(Tgt)
    Pos0, Ang0 = q(Rest + 0.05 * rng.standard_normal(Rest.shape)), q(0.05 * rng.standard_normal(Rest.shape))
    w_fit, w_reg = float(np.float32(2.0)), float(np.float32(0.9))
    return Energy("volume_arap", "volume_arap.t", (W, H, D), [w_fit, w_reg, Pos0, Ang0, Rest, Tgt], [2, 3], volume_arap_F(W, H, D, Rest, Tgt, w_fit, w_reg), dbl=dbl, guards=True)


def two_domains(N, U, dbl=False):
    """k_eval = 3: S + P, minus T, the product with the partial (1: exact)"""
    rng = np.random.default_rng([4, N, U]); q = _q(dbl)
    T, S0, P0 = q(rng.uniform(-1, 1, N)), q(rng.uniform(-0.5, 0.5, U)), q(rng.uniform(-1, 1, N))
    return Energy("two_domains", "two_domains.t", (N, U), [S0, P0, T], [0, 1], two_domains_F(N, U, T), k_eval=3, dbl=dbl)


def conv2d_wide(W=40, H=30, KS=11, dbl=False, leak_at=None):
    """k_eval = 4: the window's products and sums are counted with the accumulation (the row length); blur - B, the product with the partial Ker (exact), 0.05 X and its partial"""
    rng = np.random.default_rng(31); q = _q(dbl)
    Ker = rng.uniform(0.0, 1.0, (KS, KS)); Ker = q(Ker / Ker.sum())
    truth = rng.uniform(0.0, 1.0, (H, W))
    B = q(conv2d_blur(W, H, KS, Ker, truth) + 1e-3 * rng.standard_normal((H, W)))
    X0 = q(B + 0.2 * rng.standard_normal((H, W)))
    return Energy("conv2d_wide", "conv2d_wide.t", (W, H, KS, KS), [X0, B, Ker], [0], conv2d_wide_F(W, H, KS, Ker, B, leak_at), k_eval=4, dbl=dbl, guards=True)


def embedded_nodes(nx=6, ny=5, dbl=False, redirect=None):
    N = nx * ny
    rng = np.random.default_rng(23); q = _q(dbl)
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    Rest = q(np.stack([gx, gy, 0.2 * np.sin(gx + 0.5 * gy)], -1).reshape(N, 3))
    Goal = np.full((N, 3), -1e6); Goal[:nx] = Rest[:nx]; Goal[-nx:] = Rest[-nx:] + np.array([0.3, 0.1, 0.5]); Goal = q(Goal)
    vid = lambda i, j: j * nx + i
    pairs = [(vid(i, j), vid(i + 1, j)) for j in range(ny) for i in range(nx - 1)] + [(vid(i, j), vid(i, j + 1)) for j in range(ny - 1) for i in range(nx)]
    pairs = pairs + [(t, s) for s, t in pairs]
    a = np.array([s for s, _ in pairs], np.int32); b = np.array([t for _, t in pairs], np.int32)
    if redirect is not None: (a, b)[redirect[0]][redirect[1]] += 1
    E = len(pairs)
    Off0 = q(Rest + 0.02 * rng.standard_normal((N, 3)))
    M0 = q(np.tile(np.eye(3).reshape(1, 9), (N, 1)) + 0.02 * rng.standard_normal((N, 9)))
    w_fit, w_reg, w_rot = float(np.float32(3.0)), float(np.float32(1.0)), float(np.float32(2.0))
    return Energy("embedded_nodes", "embedded_nodes.t", (N, E), [w_fit, w_reg, w_rot, Off0, M0, Rest, Goal, a, b], [3, 4],
                  embedded_nodes_F(N, a, b, Rest, Goal, w_fit, w_reg, w_rot), dbl=dbl)


def graph2d(W=23, H=17, dbl=False, redirect=None):
    """(float only: the unknown is declared `float`.)  No entry maps a pixel to itself: there the two accesses of a tie residual are the same unknown, and the
    generated kernels -- like the reference's evalJTF (thallo.t:3688-3697), which squares the partial of every ACCESS -- leave 0.25 + 0.25 in diag where the diagonal
    of J^T J is (0.5 - 0.5)^2 = 0; r and Ap agree either way (seen on the MI355X with such entries: diag off by the whole term at exactly those pixels).  k_eval = 4: X - data, times mask, times w_fit (the partial w_fit mask: one more rounding), the product with the partial"""
    rng = np.random.default_rng(9); q = _q(dbl)
    data = q(rng.normal(0, 1, (H, W))); mask = (rng.random((H, W)) < 0.6).astype(np.float64)
    right = rng.integers(0, W, (H, W)).astype(np.int32); down = rng.integers(0, H, (H, W)).astype(np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    right = np.where(right == xx, (right + 1) % W, right).astype(np.int32); down = np.where(down == yy, (down + 1) % H, down).astype(np.int32)
    if redirect is not None: (right, down)[redirect[0]].reshape(-1)[redirect[1]] = ((right, down)[redirect[0]].reshape(-1)[redirect[1]] + 1) % ((W, H)[redirect[0]])
    x0 = q(rng.normal(0, 1, (H, W))); wf = float(np.float32(1.5))
    return Energy("graph2d", "graph2d.t", (W, H), [wf, x0, data, mask, right, down], [1], graph2d_F(W, H, data, mask, right, down, wf), precond=False, k_eval=4, dbl=dbl)


def flow_sample(W=28, H=20, dbl=False, leak_at=None):
    rng = np.random.default_rng(5); q = _q(dbl)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = lambda X, Y, ph: np.sin(0.31 * X + ph) * np.cos(0.23 * Y - ph) + 0.02 * X
    dimg_x = lambda X, Y, ph: 0.31 * np.cos(0.31 * X + ph) * np.cos(0.23 * Y - ph) + 0.02
    dimg_y = lambda X, Y, ph: -0.23 * np.sin(0.31 * X + ph) * np.sin(0.23 * Y - ph)
    dst = q(np.stack([img(xx, yy, 0.3), 0.5 * img(xx, yy, 0.3) + 0.1 * img(xx, yy, 1.1)], -1))
    ddx = q(np.stack([dimg_x(xx, yy, 0.3), 0.5 * dimg_x(xx, yy, 0.3) + 0.1 * dimg_x(xx, yy, 1.1)], -1))
    ddy = q(np.stack([dimg_y(xx, yy, 0.3), 0.5 * dimg_y(xx, yy, 0.3) + 0.1 * dimg_y(xx, yy, 1.1)], -1))
    src = q(img(xx + 0.6, yy - 0.4, 0.3))
    flow0 = rng.uniform(-1.5, 1.5, (H, W, 2))                                    # some samples leave the image: zeros outside
    if H > 3 and W > 4: flow0[3, 4] = [1.0, -2.0]                                # an integral position (floor == ceil)
    flow0[0, 0] = [-0.25, 0.0]                                                   # a sample off the left edge
    flow0[H - 1, W - 2] = [1.0, 0.0]; flow0[0, W - 1] = [0.5, 0.25]              # a sample at W - 1 exactly, one past the right edge
    flow0 = q(flow0)
    wf, wr = float(np.float32(1.0)), float(np.float32(0.7))
    return Energy("flow_sample", "flow_sample.t", (W, H), [wf, wr, flow0, src, dst, ddx, ddy], [2], flow_sample_F(W, H, src, dst, ddx, ddy, wf, wr, leak_at), precond=False, dbl=dbl, guards=True)


def row_gain(W, H, dbl=False):
    """tests/energies/row_gain.t (float only): fit = I(x, y) G(y) - T(x, y) over (x, y), reg = 0.1 (G(y) - 1) over y: the unknown does not vary with the inner dimension.
    k_eval = 3: the product, the difference, the product with the partial I (exact)"""
    rng = np.random.default_rng([5, W, H])
    I = rnd32(rng.uniform(0.5, 1.5, (H, W))); gain = rng.uniform(0.6, 1.4, (H, 1))
    T = rnd32(I * gain + rng.normal(0, 0.01, (H, W))); G0 = rnd32(rng.uniform(0.5, 1.5, H))
    w = float(np.float32(0.1))
    F = lambda x: np.concatenate([(I * x[:, None] - T).reshape(-1), w * (x - 1.0)])
    return Energy("row_gain", "row_gain.t", (W, H), [I, T, G0], [2], F, k_eval=3, dbl=dbl)


def conv1d(N=64, K=5, dbl=False):
    """tests/energies/conv1d.t (float only; the file materializes Jp): Target(n) - Sum_k Signal(n - k + 2) Kernel(k) inside the border of 2, else 0 -- the expanded Sum,
    every instance scatters to the same K unknowns.  k_eval = 11: five products, four sums, the difference, the product with the partial (a Signal value: exact)"""
    rng = np.random.default_rng([5, N])
    sig = rnd32(rng.uniform(-5, 5, N)); ker = np.array([-1.0, -0.5, 1.0, -0.5, 2.0])
    tgt = sig.copy()
    for i in range(2, N - 2): tgt[i] = sum(sig[i - c + 2] * ker[c] for c in range(K))
    tgt = rnd32(tgt + rng.normal(0, 0.5, N)); k0 = rnd32(rng.uniform(-1, 1, K))
    idx = np.arange(2, N - 2)
    def F(x):
        out = np.zeros(N, dtype=x.dtype)
        out[idx] = tgt[idx] - sum(sig[idx - c + 2] * x[c] for c in range(K))
        return out
    return Energy("conv1d", "conv1d.t", (N, K), [k0, sig, tgt], [0], F, precond=False, k_eval=11, dbl=dbl, guards=True)


def layer_sample(W=28, H=20, T=3, layer=2, sx=-1.75, sy=0.5, dbl=False):
    """tests/energies/layer_sample.t (float only): U(x, y) - (S_0 + 2 S_1) with S = Image:sample of layer `layer` of the stack at (x + sx, y + sy): samples off two
    edges.  Linear in U with partial 1; the samples cancel (values of both signs), so k_eval is measured like a nonlinear energy's"""
    rng = np.random.default_rng([11, W, H])
    stack = rnd32(rng.uniform(-1, 1, (T, H, W, 2))); U0 = rnd32(rng.uniform(-1, 1, (H, W)))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    sx, sy = float(np.float32(sx)), float(np.float32(sy))
    smp = bilinear(stack[layer, ..., 0], xx + sx, yy + sy) + 2.0 * bilinear(stack[layer, ..., 1], xx + sx, yy + sy)
    F = lambda x: x - smp.reshape(-1)
    return Energy("layer_sample", "layer_sample.t", (W, H, T), [U0, stack, float(layer), sx, sy], [0], F, precond=False, dbl=dbl, guards=True)


def image_warping(W, H, dbl=False):
    """the bundled image_warping.t (thallo_amd/energies): two unknown images, Exclude on both, Rotate2D (sin and cos of one angle), five residuals on one domain.
    F is tests/iw_reference.py's restatement of the file.  The inputs are float32 values in both builds.  Nonlinear: k_eval measured"""
    import types
    import iw_reference as iw
    import thallo_amd
    rng = np.random.default_rng([19, W, H]); f32 = np.float32
    ys, xs = np.mgrid[0:H, 0:W]
    grid = np.stack([xs, ys], -1).astype(f32)
    u = grid.copy(); u[H // 2, W // 2] += f32(0.25)
    mask = np.zeros((H, W), f32); mask[1:min(4, H), 2:min(6, W)] = 255.0; mask[H - 1, W // 3] = 1e-30
    off = (grid + rng.uniform(-0.5, 0.5, (H, W, 2))).astype(f32); ang = rng.uniform(-0.4, 0.4, (H, W)).astype(f32)
    cons = np.full((H, W, 2), -1.0, f32); pick = rng.random((H, W)) < 0.15
    cons[pick] = (grid[pick] + rng.integers(0, 3, (int(pick.sum()), 2))).astype(f32)
    inp = types.SimpleNamespace(W=W, H=H, offset=off, angle=ang, urshape=u, cons=cons, mask=mask, w_fit=3.0, w_reg=0.7)
    ref = iw.IwRef(inp)
    q = lambda a: np.asarray(a, np.float64)
    e = Energy("image_warping", "image_warping.t", (W, H), [q(off), q(ang), q(u), q(cons), q(mask), float(f32(3.0)), float(f32(0.7))], [0, 1], ref.residuals,
               free=~np.asarray(ref.excluded(), bool), dbl=dbl, guards=True)
    e.path = thallo_amd.energy_file("image_warping")
    return e


def sparse_exclude(N=150, dbl=False, redirect=None):
    """tests/energies/sparse_exclude.t: an index map and Exclude on one unknown (index evaluation gives -1 at excluded entries).  No entry maps to itself.
    k_eval = 3: the difference, the product with 0.5 (exact), the product with the partial (+-0.5 or 1: exact) -- and one to spare"""
    rng = np.random.default_rng([17, N]); q = _q(dbl)
    A, X0 = q(rng.uniform(-1, 1, N)), q(rng.uniform(-1, 1, N))
    Mask = (rng.random(N) < 0.2).astype(np.float64)
    nb = rng.integers(0, N, N).astype(np.int32); nb = np.where(nb == np.arange(N), (nb + 1) % N, nb).astype(np.int32)
    if redirect is not None: nb[redirect[1]] = (nb[redirect[1]] + 2) % N if (nb[redirect[1]] + 1) % N == redirect[1] else (nb[redirect[1]] + 1) % N
    F = lambda x: np.concatenate([x - A, 0.5 * (x - x[nb])])
    return Energy("sparse_exclude", "sparse_exclude.t", (N,), [X0, A, Mask, nb], [0], F, free=Mask == 0, k_eval=3, dbl=dbl, f32_slots=(2,))


def lp_smooth(N=33, dbl=False):
    """tests/energies/lp_smooth.t (float only): fit = S - A, reg = 1.5 L_p(S(x) - S(x + 1), pNorm) inside the image.  L_p (lib.t:157-169) multiplies the difference by
    sqrt((|v| + 1e-7)^(p - 2)) HELD CONSTANT: the factor is formed from the real part, so the complex step differentiates what the front-end differentiates.
    Nonlinear: k_eval measured"""
    rng = np.random.default_rng([29, N])
    A = rnd32(rng.uniform(-1, 1, (N, 2))); S0 = rnd32(A + 0.3 * rng.standard_normal((N, 2))); pn = float(np.float32(1.2))
    def F(x):
        S = x.reshape(N, 2); reg = np.zeros_like(S)
        v = S[:-1] - S[1:]
        cw = np.sqrt((np.sqrt((np.real(v) ** 2).sum(-1)) + 1e-7) ** (pn - 2.0))
        reg[:-1] = 1.5 * cw[:, None] * v
        return np.concatenate([(S - A).reshape(-1), reg.reshape(-1)])
    e = Energy("lp_smooth", "lp_smooth.t", (N,), [S0, A, pn], [0], F, precond=False, dbl=dbl, guards=True)
    e.detached = True          # (central differences of F see the factor move: not comparable)
    return e


def arap_mesh(dbl=False, redirect=None):
    """the bundled arap_mesh_deformation.t on the 12 x 8 torus (96 vertices, 576 directed edges): two unknown images reached through Sparse maps, Rotate3D.
    J and F are tests/graph_reference.py's ArapRef (caller numbering, one entry per access; the mesh has no self loop).  Nonlinear: k_eval measured"""
    import graph_reference as gref
    import thallo_amd
    g = gref.graph_mesh(); inp = gref.arap_inputs(g[0], sentinels=False)
    if redirect is not None:          # V1 of one edge moves on by one vertex (two, if that would make a self loop)
        v1 = g[2].copy(); k = redirect[1]; v1[k] = (v1[k] + 1) % g[0]
        if v1[k] == g[1][k]: v1[k] = (v1[k] + 1) % g[0]
        g = (g[0], g[1], v1)
    ref = gref.ArapRef(g, inp)
    params = [np.asarray(p, np.float64) if isinstance(p, np.ndarray) and p.dtype == np.float32 else p for p in gref.arap_params(g, inp)]
    e = Energy("arap_mesh_deformation", "arap_mesh_deformation.t", (g[0], len(g[1])), params, [2, 3], ref.residuals, dbl=dbl)
    e.path, e.J_rows, e.F_rows = thallo_amd.energy_file("arap_mesh_deformation"), ref.jacobian()[0].tocsc(), np.asarray(ref.residuals(ref.x0()), np.float64)
    e.detached = True          # (ArapRef.residuals takes real arguments only; test_graph_reference.py holds its J to differences)
    return e


def bundle_adjustment(dbl=False, redirect=None):
    """the bundled bundle_adjustment.t: 20 cameras with 10 observations each, 60 points seen 3 or 4 times -- two unknown spaces through Sparse maps, short lists.
    F and the 2 x 12 blocks of J are tests/ba_reference.py's, in the caller's numbering (a generated plan does not renumber).  Nonlinear: k_eval measured"""
    import ba_reference as br
    import thallo_amd
    inc = br.incidence(np.full(20, 10), np.array([3] * 40 + [4] * 20))
    cams, pts, obs = br.scene(inc)
    oc, op = np.asarray(inc.oToC, np.int32), np.asarray(inc.oToP, np.int32)
    cams, pts, obs = rnd32(cams), rnd32(pts), rnd32(obs)
    if redirect is not None: op[redirect[1]] = (op[redirect[1]] + 1) % inc.P          # one observation looks at the next point
    Fb, Jb = br.residual_and_jacobian(cams, pts, obs, oc, op)
    O = len(oc); C = inc.C
    cols = np.concatenate([9 * oc[:, None] + np.arange(9), 9 * C + 3 * op[:, None] + np.arange(3)], axis=1)
    rows = (2 * np.arange(O)[:, None, None] + np.arange(2)[None, :, None]) + 0 * cols[:, None, :]
    J = sps.csr_matrix((Jb.reshape(-1), (rows.reshape(-1), np.broadcast_to(cols[:, None, :], (O, 2, 12)).reshape(-1))), shape=(2 * O, 9 * C + 3 * inc.P))
    e = Energy("bundle_adjustment", "bundle_adjustment.t", (C, inc.P, O), [cams, pts, obs, oc, op], [0, 1], None, dbl=dbl, f32_slots=(2,))
    e.path, e.J_rows, e.F_rows = thallo_amd.energy_file("bundle_adjustment"), J.tocsc(), np.asarray(Fb, np.float64).reshape(-1)
    e.detached = True
    return e


def shape_from_shading(W, H, dbl=False):
    """the bundled shape_from_shading.t (both builds: the inputs are float32 values either way): computed arrays (B_I and its partials), uint8 edge masks, sixteen Params.  J and F are those of
    tests/sfs_reference.py (its `holes` family: depth holes on every border), which test_sfs_reference.py holds to central differences.  Nonlinear: k_eval measured"""
    import sfs_reference as sr
    import thallo_amd
    cs = sr.case("holes", W, H)
    system = cs.system()
    params = [np.asarray(p, np.float64) if isinstance(p, np.ndarray) and p.dtype == np.float32 else p for p in cs.params]
    path = thallo_amd.energy_file("shape_from_shading")
    e = Energy("shape_from_shading", "shape_from_shading.t", (W, H), params, [16], None, precond="UsePreconditioner(true)" in open(path).read(), dbl=dbl, guards=True)
    e.path, e.J_rows, e.F_rows = path, system.J.tocsc(), np.asarray(system.F, np.float64)
    return e


# ------------------------------------------------------------------ the reference
def jacobian(F, x, free):
    """dF/dx by the complex step (h = 1e-30: no subtraction, exact to rounding), one column per free unknown, as a sparse matrix with zero columns for the others"""
    cols = np.flatnonzero(free)
    ii, jj, vv = [], [], []
    xc = x.astype(np.complex128)
    for j in cols:
        xc[j] += 1e-30j
        d = F(xc).imag / 1e-30
        xc[j] = x[j]
        nz = np.flatnonzero(d)
        ii.append(nz); jj.append(np.full(nz.size, j)); vv.append(d[nz])
    rows = F(x).size
    return sps.csc_matrix((np.concatenate(vv), (np.concatenate(ii), np.concatenate(jj))), shape=(rows, x.size)) if cols.size else sps.csc_matrix((rows, x.size))


class Reference:
    def __init__(self, energy, J=None, Fx=None, diag_extra=None):
        e = self.energy = energy
        if Fx is None: Fx = getattr(e, "F_rows", None)
        self.Fx = np.real(e.F(e.x0)).astype(np.float64) if Fx is None else Fx
        self.J = (getattr(e, "J_rows", None) if J is None else J)
        if self.J is None: self.J = jacobian(e.F, e.x0, e.free)
        J = self.J; self.absJ = abs(J).tocsc()
        self.cost = 0.5 * float(self.Fx @ self.Fx)
        self.r = -(J.T @ self.Fx)
        self.diag = np.asarray(J.multiply(J).sum(axis=0)).ravel()
        if diag_extra is not None: self.diag = self.diag + diag_extra
        self.pre = 1.0 / (1.0 + np.sqrt(self.diag)) ** 2 if e.precond else np.ones(e.n)
        self.z = self.pre * self.r
        self.comp_r = self.absJ.T @ np.abs(self.Fx)                    # |J|^T |F|
        self.m_col = np.diff(self.absJ.indptr)                        # terms accumulated into every unknown
        self.row_len = int(np.diff(self.absJ.tocsr().indptr).max()) if self.absJ.nnz else 0

    def Ap(self, p):
        return self.J.T @ (self.J @ p)

    def comp_Ap(self, p):
        return self.absJ.T @ (self.absJ @ np.abs(p))                   # |J|^T |J| |p|

    # ---- the bound of the GPU test: (gamma_m + k eps) x companion
    def gamma(self, m):
        m = np.asarray(m, np.float64) * self.energy.eps
        return m / (1.0 - m)

    def bound_r(self, k):
        return (self.gamma(self.m_col + 1) + k * self.energy.eps) * self.comp_r

    def bound_diag(self, k):
        return (self.gamma(self.m_col + 1) + k * self.energy.eps) * self.diag

    def bound_Ap(self, k, p, assembled=False):
        """assembled: J^T J formed once (the dense and sparse [JtJ]p schedules) -- an entry of it accumulates at most m_col products, a row of it has m_jtj entries"""
        if assembled:
            if not hasattr(self, "m_jtj"): self.m_jtj = np.diff((self.absJ.T @ self.absJ).tocsr().indptr)
            return (self.gamma(self.m_col + self.m_jtj + 2) + k * self.energy.eps) * self.comp_Ap(p)
        return (self.gamma(self.m_col + self.row_len + 2) + k * self.energy.eps) * self.comp_Ap(p)


@functools.lru_cache(maxsize=None)
def reference(factory, *args, **kw):
    return Reference(factory(*args, **kw))


def probe_vectors(n, seed):
    """the two regimes of p: `random` dense, `decades` spanning six decades; no entry is zero"""
    rng = np.random.default_rng([77, seed, n])
    rnd = rng.standard_normal(n); rnd[np.abs(rnd) < 1e-3] = 0.5
    dec = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 10.0 ** rng.integers(-3, 4, n)
    return {"random": rnd32(rnd), "decades": rnd32(dec)}
