"""CPU restatement of bundle adjustment with unknowns held fixed (thallo_amd/csrc/held.hip, ThalloX_PlanSetHeldUnknowns) -- TEST INFRASTRUCTURE, not a test.

The mirrors of tests/ba_block_mirror.py, tests/ba_schur_mirror.py and tests/ba_schur_explicit_mirror.py with a mask (one flag per scalar of [cameras 9 c + k | points
9 C + 3 p + k], True = held) and the device's one rule: every product with M^-1 or Cp^-1 has a zero row and column at a held scalar.  Restated as the device does it:

  point Jacobi   pre = 0 at the held scalars;
  blocks         a held scalar's row and column of its block of H become those of the identity in front of the factorisation, and zero in G (or in the float64 inverse)
                 behind it -- G^T G is then the inverse of the block's free principal sub-block bordered by zeros; the fallback diag(sqrt(pre)) is masked through pre;
  Schur          the same on the camera blocks (the preconditioner of S) and on the elimination factor; g, the apply, the assembly and the back-substitution inherit it.

Nothing else of the loops changes: z, p and delta stay zero at the held scalars by themselves, and the loop's scalars only see the free set."""
import numpy as np
import scipy.sparse as sp

import ba_schur_mirror as bsm
from ba_block_mirror import BaBlockMirror, BlockPrecond, F
from ba_schur_explicit_mirror import ExplicitSchurSystem
from ba_schur_mirror import BaSchurMirror, SchurSystem, block_diag3

CONFIGS = ("jacobi", "block", "schur", "schur_explicit")


def masks(C, P):
    """the masks of the held-unknowns tests, by name -> flat bool [9 C + 3 P]"""
    n, nc = 9 * C + 3 * P, 9 * C
    out = {}
    m = np.zeros(n, bool); m[:18] = True; out["two_cameras"] = m
    m = np.zeros(n, bool); m[:nc].reshape(C, 9)[:, 6:9] = True; out["intrinsics"] = m
    m = np.zeros(n, bool); pm = m[nc:].reshape(P, 3); pm[[1, P // 2, P - 2]] = True; pm[4, 1] = True; out["control_points"] = m
    m = np.zeros(n, bool); m[nc:] = True; out["all_points"] = m
    m = np.zeros(n, bool); m[:nc] = True; out["all_cameras"] = m
    return out


def split(mask, C):
    """flat mask -> ([C, 9], [P, 3])"""
    return mask[:9 * C].reshape(-1, 9), mask[9 * C:].reshape(-1, 3)


def hold_blocks(H, m):
    """[nb, n, n] blocks, [nb, n] flags -> the blocks with the identity's rows and columns at the held scalars (thallo_hip_block_hold)"""
    H = H.copy()
    either = m[:, :, None] | m[:, None, :]
    H[either] = 0
    idx = np.arange(H.shape[1])
    H[:, idx, idx] = np.where(m, 1.0, H[:, idx, idx])
    return H


def hold_factor(G, m):
    """zero rows and columns at the held scalars, in place (thallo_hip_block_hold_factor)"""
    G[m[:, :, None] | m[:, None, :]] = 0
    return G


def held_precond(kind, Hs, shift, pre, C, mask):
    """BaBlockMirror._precond under the mask"""
    pre = np.where(mask, F(0), np.asarray(pre, F)).astype(F)
    if kind == "jacobi":
        return (lambda r: (pre * r).astype(F)), 0
    mc, mp = split(mask, C)
    M = BlockPrecond(kind, (hold_blocks(Hs[0], mc), hold_blocks(Hs[1], mp)), shift, pre, C)
    for (Minv, G, lo, n, nb), m in zip(M.parts, (mc, mp)):
        hold_factor(Minv if G is None else G, m)
    return M, M.fallbacks


class HeldBlockMirror(BaBlockMirror):
    """BaBlockMirror (kinds "jacobi", "block32", "block64") with a mask"""

    def __init__(self, dims, params, mask):
        super().__init__(dims, params)
        self.mask = np.asarray(mask, bool)
        assert self.mask.shape == (self.n,)

    def _precond(self, kind, Hs, shift, pre):
        M, fb = held_precond(kind, Hs, shift, pre, self.C, self.mask)
        self.fallbacks += fb
        return M


def held_system(base, mask):
    """SchurSystem (or ExplicitSchurSystem) under the mask: a class the loops of BaSchurMirror can build by the module's name"""
    core = type("HeldCore", (SchurSystem,), {})

    def init(self, J, Hs, shift, pre, b, C):
        mc, mp = split(mask, C)
        pre = np.where(mask, F(0), np.asarray(pre, F)).astype(F)
        SchurSystem.__init__(self, J, (hold_blocks(Hs[0], mc), hold_blocks(Hs[1], mp)), shift, pre, b, C)
        hold_factor(self.G, mp)
        hold_factor(self.M.parts[0][1], mc)
        G64 = self.G.astype(np.float64)
        self.Cinv = block_diag3(np.einsum("bki,bkj->bij", G64, G64))
        self.y = (self.Cinv @ self.b[self.nc:].astype(np.float64)).astype(F)
        self.g = (self.b[:self.nc].astype(np.float64) - self.Jc.T @ (self.Jp @ self.y.astype(np.float64))).astype(F)
    core.__init__ = init
    return core if base is SchurSystem else type("HeldExplicit", (base, core), {})


class HeldSchurMirror(BaSchurMirror):
    """BaSchurMirror with a mask: the loops build their system by the module's name SchurSystem, which is swapped for the length of a solve (as BaSchurExplicitMirror does)"""
    system = SchurSystem

    def __init__(self, dims, params, mask):
        super().__init__(dims, params)
        self.mask = np.asarray(mask, bool)
        assert self.mask.shape == (self.n,)

    def _held(self, f, *a, **kw):
        saved = bsm.SchurSystem
        bsm.SchurSystem = held_system(self.system, self.mask)
        try: return f(*a, **kw)
        finally: bsm.SchurSystem = saved

    # every camera held: the reduced system is empty and its loop takes no iteration (p_0 = 0 would make LM's unguarded alpha_0 = 0 / 0); the back-substitution from
    # delta_c = 0 is the whole solve -- Plan::schur_empty
    def gn_step(self, L, kind="schur"):
        return self._held(super().gn_step, 0 if self.mask[:self.nc].all() else L, kind)

    def lm_solve(self, nit, lit, kind="schur", **kw):
        return self._held(super().lm_solve, nit, 0 if self.mask[:self.nc].all() else lit, kind, **kw)


class HeldSchurExplicitMirror(HeldSchurMirror):
    system = ExplicitSchurSystem


def held_mirror(config, dims, params, mask):
    """-> (mirror, the `kind` its gn_solve / lm_solve take)"""
    if config == "jacobi": return HeldBlockMirror(dims, params, mask), "jacobi"
    if config == "block": return HeldBlockMirror(dims, params, mask), "block32"
    if config == "schur": return HeldSchurMirror(dims, params, mask), "schur"
    if config == "schur_explicit": return HeldSchurExplicitMirror(dims, params, mask), "schur"
    raise ValueError(config)


# ------------------------------------------------------------------ float64: the rule alone solves A_FF delta_F = b_F
def masked_inverse64(H, m):
    """[nb, n, n] symmetric positive definite blocks (a fully held one may be anything) -> the inverse of every block's free principal sub-block bordered by zeros"""
    return hold_factor(np.linalg.inv(hold_blocks(H, m)), m)


def pcg64(apply, b, Minv, iters, tol=1e-15):
    """float64 PCG on complete vectors; nothing in here knows the mask"""
    x = np.zeros_like(b); r = b.copy(); z = Minv(r); p = z.copy(); rz = r @ z
    for k in range(iters):
        if rz <= 0: break
        Ap = apply(p)
        alpha = rz / (p @ Ap)
        x += alpha * p; r -= alpha * Ap
        z = Minv(r); rz_new = r @ z
        if np.sqrt(abs(rz_new)) <= tol * np.sqrt(abs(b @ Minv(b))): break
        p = z + (rz_new / rz) * p; rz = rz_new
    return x


def block_apply64(Mc, Mp, C):
    nc = 9 * C
    def f(r):
        return np.concatenate([np.einsum("bij,bj->bi", Mc, r[:nc].reshape(-1, 9)).ravel(), np.einsum("bij,bj->bi", Mp, r[nc:].reshape(-1, 3)).ravel()])
    return f


def held_solve64(A, b, mask, C, config, iters=20000):
    """float64, the first LM system A delta = b (A sparse, symmetric positive definite) under the mask, by the device's mechanism: PCG on the COMPLETE vectors with a masked
    M^-1 ("jacobi", "block"), or the points eliminated through the masked Cp^-1 and PCG on the cameras with the masked camera blocks ("schur", "schur_explicit": S formed
    densely)."""
    A = np.asarray(A.todense()) if sp.issparse(A) else np.asarray(A, np.float64)
    nc = 9 * C; P = (len(b) - nc) // 3
    mc, mp = split(mask, C)
    if config == "jacobi":
        pre = np.where(mask, 0.0, 1.0 / np.diag(A))
        return pcg64(lambda x: A @ x, b, lambda r: pre * r, iters)
    Hc = np.stack([A[9 * c:9 * c + 9, 9 * c:9 * c + 9] for c in range(C)]); Hp = np.stack([A[nc + 3 * j:nc + 3 * j + 3, nc + 3 * j:nc + 3 * j + 3] for j in range(P)])
    Mc, Mp = masked_inverse64(Hc, mc), masked_inverse64(Hp, mp)
    if config == "block":
        return pcg64(lambda x: A @ x, b, block_apply64(Mc, Mp, C), iters)
    Ci = np.asarray(block_diag3(Mp).todense())
    B, E = A[:nc, :nc], A[:nc, nc:]
    S = B - E @ Ci @ E.T; g = b[:nc] - E @ (Ci @ b[nc:])
    dc = pcg64(lambda x: S @ x, g, lambda r: np.einsum("bij,bj->bi", Mc, r.reshape(-1, 9)).ravel(), iters)
    return np.concatenate([dc, Ci @ (b[nc:] - E.T @ dc)])
