"""CPU restatement of bundle adjustment with Gaussian priors on single unknowns (thallo_amd/csrc/prior.hip, ThalloX_PlanSetPrior) -- TEST INFRASTRUCTURE, not a test.

The energy gains one residual sqrt(w_i) (x_i - mu_i) per scalar with w_i > 0, over [cameras 9 c + k | points 9 C + 3 p + k]:

  cost  += 1/2 sum w (x - mu)^2                  (prior_cost32: thallo_hip_prior_cost's partials in their order)
  b      = -J^T F - W (x - mu),  diag += w       (prior_init32: thallo_hip_prior_init)
  A      = J^T J + W

prior(cls) wraps the mirrors of tests/ba_block_mirror.py (point Jacobi, block), ba_schur_mirror.py, ba_schur_explicit_mirror.py, ba_schur_dense_mirror.py,
ba_two_level_mirror.py, ba_held_mirror.py (a mask, through held_system) and ba_robust_mirror.py (a loss: prior(robust(cls)), so that no loss touches a prior) by overriding
their two hooks, cost() and linearise(); the loops, the preconditioners, the Schur systems, the masks and the losses inherit the rest.

How W reaches the mirrors' matrices.  The device keeps H (the blocks of J^T J) without W and hands W to every factor, apply and assembly as their flat diagonal argument:
GN w itself, LM float32(CtC + w).  The mirrors' loops build their applies from J (J^T (J p), the Schur systems' J_c and J_p) and their factors from the stacked float64
blocks Hs, with the LM CtC as the only diagonal argument.  So linearise() returns
  J    with the rows sqrt(w_i) e_i^T behind the observations' (every J^T J p, the model cost's delta . J^T J delta and the matrix-free Schur apply then carry W; the
       assembled forms read the observations' rows alone -- `observation_rows`),
  r, d in float32 as prior_init32 leaves them,
  Hs   with the diagonal entries float64(float32(float32(H_ii) + w_i)): the factors' `H.astype(float32)` is then bit for bit the device's GN diagonal H_ii + w_i.
In LM the mirrors add CtC to that sum where the device adds float32(CtC + w) to H_ii: the same three numbers in another association, one rounding (2^-24 relative) of a
diagonal entry apart."""
import contextlib

import numpy as np
import scipy.sparse as sp

import ba_schur_explicit_mirror as bse
from ba_block_mirror import F

BLOCK, WAVE, COST_PARTIALS, MAX_PARTIALS = 256, 64, 64, 1024
CONFIGS = ("jacobi", "block", "schur", "schur_explicit", "schur_dense", "two_level")


def grid_for(n, cap):
    return max(1, min((n + BLOCK - 1) // BLOCK, cap))


def workgroup_partials(terms, grid):
    """the partials of a grid-stride launch of `grid` workgroups of 256 lanes: per lane acc += term in the order it visits its scalars, then the wave butterfly
    (lane ^ 32, 16, 8, 4, 2, 1), then the workgroup's waves added in order from 0.0f -- device_common.hpp block_store_partial, every addition rounded to float32"""
    n = len(terms)
    stride = grid * BLOCK
    trips = (n + stride - 1) // stride
    t = np.zeros(trips * stride, F); t[:n] = terms
    acc = np.zeros(stride, F)
    for k in range(trips): acc = (acc + t[k * stride:(k + 1) * stride]).astype(F)
    lanes = acc.reshape(grid, BLOCK // WAVE, WAVE)
    m = WAVE // 2
    while m >= 1:
        idx = np.arange(WAVE) ^ m
        lanes = (lanes + lanes[:, :, idx]).astype(F); m //= 2
    waves = lanes[:, :, 0]
    out = np.zeros(grid, F)
    for w in range(BLOCK // WAVE): out = (out + waves[:, w]).astype(F)
    return out


def prior_cost32(w, mu, x):
    """thallo_hip_prior_cost: the partials of 1/2 sum w (x - mu)^2, float32, one rounding per operation (the device may fuse the last product into the addition)"""
    w, mu, x = np.asarray(w, F), np.asarray(mu, F), np.asarray(x, F)
    d = np.where(w > 0, (x - mu).astype(F), F(0)).astype(F)
    terms = np.where(w > 0, ((F(0.5) * w).astype(F) * (d * d).astype(F)).astype(F), F(0)).astype(F)
    return workgroup_partials(terms, grid_for(len(w), COST_PARTIALS))


def prior_init32(w, mu, x, r, diag, pre, z, use_precond=True):
    """thallo_hip_prior_init -> (r, diag, pre, z, the partials of r . z): only the scalars with w > 0 change"""
    w, mu, x = np.asarray(w, F), np.asarray(mu, F), np.asarray(x, F)
    on = w > 0
    d = np.where(on, (x - mu).astype(F), F(0)).astype(F)
    r2 = np.where(on, (np.asarray(r, F) - (w * d).astype(F)).astype(F), np.asarray(r, F)).astype(F)
    d2 = np.where(on, (np.asarray(diag, F) + w).astype(F), np.asarray(diag, F)).astype(F)
    with np.errstate(all="ignore"):
        m = (F(1) / ((F(1) + np.sqrt(d2)).astype(F) ** 2).astype(F)).astype(F) if use_precond else np.ones_like(d2)
    p2 = np.where(on, m, np.asarray(pre, F)).astype(F)
    z2 = np.where(on, (p2 * r2).astype(F), np.asarray(z, F)).astype(F)
    return r2, d2, p2, z2, workgroup_partials((r2 * z2).astype(F), grid_for(len(w), MAX_PARTIALS))


def prior_lm_shift32(w, ctc):
    """thallo_hip_prior_lm_shift: float32(CtC + w)"""
    return (np.asarray(ctc, F) + np.asarray(w, F)).astype(F)


def prior_cost64(w, mu, x):
    w, mu, x = (np.asarray(a, np.float64) for a in (w, mu, x))
    return 0.5 * float((np.where(w > 0, w * (x - mu) ** 2, 0.0)).sum())


@contextlib.contextmanager
def observation_rows(O):
    """the assembled Schur systems rebuild the observations' 2 x 12 blocks from J's rows (ba_schur_explicit_mirror.jb_of): for the length of a solve they are handed the
    observations' rows alone, without the priors' behind them -- W is in the blocks Hs they assemble B_ii from (the module's name is swapped, as the mirrors swap
    SchurSystem)"""
    saved = bse.jb_of
    bse.jb_of = lambda J, C: saved(sp.csr_matrix(J)[:2 * O], C)
    try: yield
    finally: bse.jb_of = saved


def prior(cls):
    """cls(dims, params, ...) -> a class whose constructor takes (mean, weight) in front, flat float32 over [cameras | points] in the caller's ids: the same mirror with the priors"""

    class Prior(cls):
        def __init__(self, mean, weight, *a, **kw):
            super().__init__(*a, **kw)
            self.w = np.asarray(weight, F).reshape(-1).copy()
            self.mu = np.where(self.w > 0, np.asarray(mean, F).reshape(-1), F(0)).astype(F)
            assert self.w.shape == (self.n,) and (self.w >= 0).all() and np.isfinite(self.w).all() and np.isfinite(self.mu).all()

        def x(self):
            return np.concatenate([self.params[0].ravel(), self.params[1].ravel()]).astype(F)

        def prior_cost(self):
            """the prior's share: the device's partials added in float64 (ThalloX_PlanPriorCost)"""
            return float(prior_cost32(self.w, self.mu, self.x()).astype(np.float64).sum())

        def cost(self):
            return F(float(super().cost()) + float(prior_cost32(self.w, self.mu, self.x()).astype(np.float64).sum()))

        def linearise(self):
            J, r, d, Hs = super().linearise()
            w = self.w
            r, d = prior_init32(w, self.mu, self.x(), r, d, np.zeros(self.n, F), np.zeros(self.n, F))[:2]
            on = np.nonzero(w > 0)[0]
            rows = sp.csr_matrix((np.sqrt(w[on].astype(np.float64)), (np.arange(len(on)), on)), shape=(len(on), self.n))
            J = sp.csr_matrix(sp.vstack([sp.csr_matrix(J), rows]))
            Hc, Hp = Hs[0].copy(), Hs[1].copy()
            i9, i3, nc = np.arange(9), np.arange(3), self.nc
            Hc[:, i9, i9] = (Hc[:, i9, i9].astype(F) + w[:nc].reshape(-1, 9)).astype(F)
            Hp[:, i3, i3] = (Hp[:, i3, i3].astype(F) + w[nc:].reshape(-1, 3)).astype(F)
            return J, r, d, (Hc, Hp)

        def gn_step(self, *a, **kw):
            with observation_rows(self.O): return super().gn_step(*a, **kw)

        def lm_solve(self, *a, **kw):
            with observation_rows(self.O): return super().lm_solve(*a, **kw)

    Prior.__name__ = "Prior" + cls.__name__
    return Prior


def prior_mirror(config, mean, weight, dims, params, mask=None, loss=None):
    """-> (mirror, the `kind` its gn_solve / lm_solve take): the six configurations, with a mask of held unknowns or without, under a loss (kind, scale) or the squared one"""
    import ba_held_mirror as bh
    from ba_block_mirror import BaBlockMirror
    from ba_robust_mirror import robust
    from ba_schur_dense_mirror import BaSchurDenseMirror
    from ba_schur_explicit_mirror import BaSchurExplicitMirror
    from ba_schur_mirror import BaSchurMirror
    from ba_two_level_mirror import BaTwoLevelMirror
    tail = ()
    if config in ("schur_dense", "two_level"):
        cls = BaSchurDenseMirror if config == "schur_dense" else BaTwoLevelMirror
        tail = (mask,)
    elif mask is not None:
        cls = {"jacobi": bh.HeldBlockMirror, "block": bh.HeldBlockMirror, "schur": bh.HeldSchurMirror, "schur_explicit": bh.HeldSchurExplicitMirror}[config]
        tail = (mask,)
    else:
        cls = {"jacobi": BaBlockMirror, "block": BaBlockMirror, "schur": BaSchurMirror, "schur_explicit": BaSchurExplicitMirror}[config]
    if loss is not None: m = prior(robust(cls))(mean, weight, loss[0], loss[1], dims, params, *tail)
    else: m = prior(cls)(mean, weight, dims, params, *tail)
    return m, {"jacobi": "jacobi", "block": "block32"}.get(config, "schur")


# ------------------------------------------------------------------ float64: the semantics alone
def prior_system64(J, res, w, mu, x):
    """(A, b) in float64 from J (sparse or dense), the residuals F and the priors: A = J^T J + W, b = -J^T F - W (x - mu)"""
    J = sp.csr_matrix(J).astype(np.float64)
    w, mu, x = (np.asarray(a, np.float64) for a in (w, mu, x))
    A = np.asarray((J.T @ J).todense()) + np.diag(w)
    return A, -(J.T @ np.asarray(res, np.float64)) - w * np.where(w > 0, x - mu, 0.0)


def soft_gauge(C, P, S_diag, rel=1e-3):
    """the soft gauge of the dense tests: camera 0's six pose scalars and scalar 3 (a translation) of camera 1, each with weight rel x the largest diagonal entry of the
    reduced camera matrix S among the seven (S_diag: its diagonal, 9 C) -> flat weights [9 C + 3 P]"""
    idx = np.array([0, 1, 2, 3, 4, 5, 9 + 3])
    w = np.zeros(9 * C + 3 * P, F)
    w[idx] = F(rel * float(np.asarray(S_diag, np.float64)[idx].max()))
    return w
