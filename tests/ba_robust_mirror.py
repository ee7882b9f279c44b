"""CPU restatement of bundle adjustment with a robust loss (ThalloX_PlanSetRobustLoss; thallo_amd/csrc/energy_ba.hip) -- TEST INFRASTRUCTURE, not a test.

One loss over the 2-vector residual of an observation: cost = sum_o 1/2 rho(s_o), s = r0^2 + r1^2, scale a > 0 in pixels.

  "huber"   rho = s for s <= a^2, 2 a sqrt(s) - a^2 beyond;   rho' = 1, a / sqrt(s)
  "cauchy"  rho = a^2 log(1 + s / a^2);                        rho' = 1 / (1 + s / a^2)

First order (IRLS; Triggs' correction without the rho'' term): with w = sqrt(rho'(s)), rounded to float32 as the device stores it, a step is the GN / LM step of
J_s = w J, F_s = w F.  robust(cls) wraps the mirrors of tests/ba_block_mirror.py, tests/ba_schur_mirror.py, tests/ba_schur_explicit_mirror.py and tests/ba_held_mirror.py
by overriding their two hooks only -- cost() and linearise(); the loops, the preconditioners, the Schur systems and the masks inherit the rest."""
import numpy as np
import scipy.sparse as sp

from ba_block_mirror import F, stacked_blocks

KINDS = ("huber", "cauchy")


def rho(kind, a, s):
    """-> (rho(s), rho'(s)) in float64, elementwise"""
    s = np.asarray(s, np.float64); a = float(a)
    if kind == "trivial": return s.copy(), np.ones_like(s)
    if kind == "huber":
        out = s > a * a
        rs = np.sqrt(np.where(out, s, 1.0))
        return np.where(out, 2.0 * a * rs - a * a, s), np.where(out, a / rs, 1.0)
    if kind == "cauchy":
        return a * a * np.log1p(s / (a * a)), 1.0 / (1.0 + s / (a * a))
    raise ValueError(kind)


def contaminate(p, seed=5):
    """O // 20 observations displaced by 30 - 150 px (uniform) at a uniform angle -> (params, outlier mask [O]); everything from the one default_rng(seed)"""
    rng = np.random.default_rng(seed)
    q = [a.copy() for a in p]
    O = len(q[2])
    idx = rng.choice(O, O // 20, replace=False)
    mag = rng.uniform(30.0, 150.0, len(idx)); ang = rng.uniform(0.0, 2.0 * np.pi, len(idx))
    q[2][idx] = (q[2][idx].astype(np.float64) + np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)).astype(F)
    mask = np.zeros(O, bool); mask[idx] = True
    return q, mask


def residuals64(cams, pts, obs, oc, op):
    """the reprojection residuals in float64 numpy (the expression of oracle/thallo_oracle.c's bundle adjustment: angle-axis rotation with its small-angle branch,
    translation, -P.xy / P.z, f (1 + r2 (l1 + l2 r2))) -> [O, 2]"""
    c = np.asarray(cams, np.float64)[oc]; X = np.asarray(pts, np.float64)[op]
    w = c[:, 0:3]
    th2 = (w * w).sum(1)
    big = th2 > 1e-8
    th = np.sqrt(np.where(big, th2, 1.0))
    u = w / th[:, None]
    ct, st = np.cos(th)[:, None], np.sin(th)[:, None]
    Pb = X * ct + np.cross(u, X) * st + u * ((u * X).sum(1)[:, None] * (1.0 - ct))
    Ps = X + np.cross(w, X)
    Pc = np.where(big[:, None], Pb, Ps) + c[:, 3:6]
    cx, cy = -Pc[:, 0] / Pc[:, 2], -Pc[:, 1] / Pc[:, 2]
    r2 = cx * cx + cy * cy
    fd = c[:, 6] * (1.0 + r2 * (c[:, 7] + c[:, 8] * r2))
    o = np.asarray(obs, np.float64)
    return np.stack([o[:, 0] - cx * fd, o[:, 1] - cy * fd], 1)


def cost64(kind, a, params, x=None):
    """the robust cost in float64 at the flat unknowns x (default: the params' own)"""
    cams, pts, obs, oc, op = params
    if x is not None: cams, pts = x[:cams.size].reshape(cams.shape), x[cams.size:].reshape(pts.shape)
    r = residuals64(cams, pts, obs, oc, op)
    return 0.5 * rho(kind, a, (r * r).sum(1))[0].sum()


def residuals(m):
    """the oracle's residuals of a mirror's current unknowns: float32 [O, 2]"""
    return m._problem().csr()[3].reshape(-1, 2)


def inlier_rms(m, outliers):
    """RMS reprojection error (pixels, per observation) over the observations that were not displaced"""
    r = residuals(m).astype(np.float64)[~outliers]
    return float(np.sqrt((r * r).sum(1).mean()))


def robust(cls):
    """cls(dims, params, ...) -> a class whose constructor takes (kind, scale) in front: the same mirror under the loss"""

    class Robust(cls):
        def __init__(self, kind, scale, *a, **kw):
            super().__init__(*a, **kw)
            self.kind, self.scale = kind, float(scale)
            self.weights = None                 # rho'(s) per observation (float64 of the float32 w, squared) at the last linearisation

        def cost(self):
            r = residuals(self).astype(np.float64)
            return F(0.5 * rho(self.kind, self.scale, (r * r).sum(1))[0].sum())

        def linearise(self):
            rp, col, val, res = self._problem().csr()
            r2 = res.astype(np.float64).reshape(-1, 2)
            w = np.sqrt(rho(self.kind, self.scale, (r2 * r2).sum(1))[1]).astype(F).astype(np.float64)
            self.weights = w * w
            w = np.repeat(w, 2)                                         # rows 2 o, 2 o + 1 are observation o's
            J = sp.diags(w) @ sp.csr_matrix((val.astype(np.float64), col, rp), shape=(len(res), self.n))
            J = sp.csr_matrix(J)
            Fs = w * res.astype(np.float64)
            r = (-(J.T @ Fs)).astype(F)
            JtJ = (J.T @ J)
            return J, r, JtJ.diagonal().astype(F), stacked_blocks(JtJ, self.C, self.P)

    Robust.__name__ = "Robust" + cls.__name__
    return Robust


def robust_mirror(config, kind, scale, dims, params, mask=None):
    """-> (mirror, the `kind` its gn_solve / lm_solve take): the four configurations of tests/ba_held_mirror.py::CONFIGS, with a mask of held unknowns or without"""
    import ba_held_mirror as bh
    from ba_block_mirror import BaBlockMirror
    from ba_schur_explicit_mirror import BaSchurExplicitMirror
    from ba_schur_mirror import BaSchurMirror
    if mask is not None:
        cls = {"jacobi": bh.HeldBlockMirror, "block": bh.HeldBlockMirror, "schur": bh.HeldSchurMirror, "schur_explicit": bh.HeldSchurExplicitMirror}[config]
        m = robust(cls)(kind, scale, dims, params, mask)
    else:
        cls = {"jacobi": BaBlockMirror, "block": BaBlockMirror, "schur": BaSchurMirror, "schur_explicit": BaSchurExplicitMirror}[config]
        m = robust(cls)(kind, scale, dims, params)
    return m, {"jacobi": "jacobi", "block": "block32"}.get(config, "schur")
