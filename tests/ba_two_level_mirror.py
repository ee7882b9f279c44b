"""CPU restatement of the two-level preconditioner on bundle adjustment's assembled reduced camera matrix (thallo_amd/csrc/ba_coarse.hip, ThalloX_PlanSetPreconditioner
kind 2) -- TEST INFRASTRUCTURE, not a test.  Everything but the coarse correction is tests/ba_schur_explicit_mirror.py's and tests/ba_held_mirror.py's, imported and left as
they are.

  M^-1 = G^T G + P S_c^-1 P^T,   S_c = P^T S P,   P[9 c + j, 9 a(c) + j] = 1 at a free scalar,   S_c^-1 = Z^T Z,  Z = L^-1 D,  D S_c D = L L^T

  default_k / greedy_aggregates / member_lists / validate_aggregates     the aggregates as csrc/ba_structure.cpp builds them (greedy_aggregates, member_lists:
                          compared entry by entry in tests/test_ba_structure_host.py) and Plan::set_coarse_aggregates checks them
  Coarse                  S_c, its scaling, Z and the apply from the stored blocks of an ExplicitSchurSystem: float64, or float32 (a LAPACK spotrf / strtrs on the rounded S_c)
  two_level_system        an ExplicitSchurSystem (under a mask: held_system) whose M adds the coarse term; BaTwoLevelMirror runs BaSchurMirror's GN and LM loops on it
  pcg32                   a plain float32 PCG on dense matrices for ITERATION COUNTS (not bits): the stop is sqrt(r . z / r0 . z0) <= tol
  assemble32 / scale32 / apply32     float32 in the kernels' summation order, every product and every addition rounded on its own, elementwise numpy: the e32 side"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import ba_schur_mirror as bsm
from ba_held_mirror import HeldSchurMirror, held_system, split
from ba_schur_explicit_mirror import ExplicitSchurSystem

F = np.float32
MAX_N = 8192              # THALLO_HIP_COARSE_MAX_N
PARTIALS = 64             # THALLO_HIP_COARSE_PARTIALS


def default_k(C):
    return max(8, -(-C // 128))


def greedy_aggregates(st, k):
    """cameras in ascending id; an unassigned camera seeds an aggregate, which repeatedly takes the unassigned camera with the largest summed weight (the co-visible points =
    the block's term count) to its members, ties to the lower id, until it has k members or no connected camera is left -> (agg [C], mem_ptr [K + 1], mem [C] in joining order)"""
    C = st.C
    w = np.diff(st.term_ptr)
    adj = [[] for _ in range(C)]
    for i, j, ww in zip(st.row, st.colj, w):
        if i != j: adj[i].append((int(j), max(int(ww), 1))); adj[j].append((int(i), max(int(ww), 1)))
    agg = -np.ones(C, np.int64); mem = []; mem_ptr = []
    K = 0
    for seed in range(C):
        if agg[seed] >= 0: continue
        a = K; K += 1
        mem_ptr.append(len(mem))
        score = {}
        nxt, size = seed, 0
        while nxt >= 0:
            agg[nxt] = a; mem.append(nxt); size += 1
            for u, ww in adj[nxt]:
                if agg[u] < 0: score[u] = score.get(u, 0) + ww
            nxt = -1
            if size >= k: break
            for u, s in score.items():
                if agg[u] < 0 and (nxt < 0 or s > score[nxt] or (s == score[nxt] and u < nxt)): nxt = u
    mem_ptr.append(len(mem))
    return agg, np.asarray(mem_ptr, np.int64), np.asarray(mem, np.int64)


def member_lists(agg):
    """a caller's array -> (mem_ptr, mem), the members in ascending id"""
    agg = np.asarray(agg, np.int64)
    K = int(agg.max()) + 1
    mem = np.argsort(agg, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=K))]), mem


def validate_aggregates(agg, C):
    """what Plan::set_coarse_aggregates refuses -> None, or the reason"""
    agg = np.asarray(agg)
    if agg.shape != (C,): return "the array has %d ids, the plan has %d cameras" % (agg.size, C)
    if (agg < 0).any() or (agg >= C).any(): return "an id is out of range"
    K = int(agg.max()) + 1
    if len(np.unique(agg)) != K: return "the ids must be dense"
    if 9 * K > MAX_N: return "more coarse scalars than the kernels take"
    return None


def prolongation(agg, hold_c):
    """P [9 C, 9 K] (float64 CSR): one 1 per free scalar"""
    agg = np.asarray(agg, np.int64)
    C = len(agg); K = int(agg.max()) + 1
    free = np.ones((C, 9), bool) if hold_c is None else ~np.asarray(hold_c, bool)
    rows = 9 * np.arange(C)[:, None] + np.arange(9)[None, :]; cols = 9 * agg[:, None] + np.arange(9)[None, :]
    return sp.csr_matrix((free.ravel().astype(np.float64), (rows.ravel(), cols.ravel())), shape=(9 * C, 9 * K))


class Coarse:
    """S_c = P^T S P from the stored blocks S [nblk, 9, 9] of the structure st, T = D S_c D with the identity's row where the diagonal is not positive, T = L L^T, Z = L^-1 D.
    dtype float64: everything exact to float64; float32: S_c rounded once, the scaling as two rounded products, a float32 LAPACK factor and triangular solve.  A factor
    that fails leaves Z = 0 (failed = 1): block Jacobi alone."""

    def __init__(self, st, S, agg, hold_c=None, dtype=F):
        self.dtype = dtype
        self.P = prolongation(agg, hold_c)
        self.K = self.P.shape[1] // 9; self.n = n = 9 * self.K
        self.Sc = np.asarray((self.P.T @ st.bsr(S) @ self.P).todense())
        Sc = self.Sc.astype(dtype)
        diag = np.diag(Sc)
        with np.errstate(all="ignore"):
            self.d = d = np.where(diag > 0, dtype(1) / np.sqrt(np.where(diag > 0, diag, 1)).astype(dtype), dtype(0)).astype(dtype)
        self.identity_rows = int((d == 0).sum())
        self.T = scale(Sc, d)
        self.failed = 0
        try:
            self.L = np.linalg.cholesky(self.T).astype(dtype)
            self.Z = sla.solve_triangular(self.L, np.diag(d), lower=True, check_finite=False).astype(dtype)
            if not np.isfinite(self.Z).all(): raise np.linalg.LinAlgError
        except np.linalg.LinAlgError:
            self.failed = 1; self.L = None; self.Z = np.zeros((n, n), dtype)

    def y(self, r):
        return (self.Z @ (self.P.T @ np.asarray(r, np.float64)).astype(self.dtype)).astype(self.dtype)

    def apply(self, r):
        """P Z^T Z P^T r"""
        y = self.y(r)
        return (self.P @ (self.Z.T @ y).astype(np.float64)).astype(self.dtype)

    def dense(self):
        """P Z^T Z P^T as a matrix, float64 products of the stored Z"""
        ZP = self.Z.astype(np.float64) @ self.P.T.toarray()
        return ZP.T @ ZP


def scale(Sc, d):
    """T_ij = (d_i s_ij) d_j, two rounded products; the identity's row and column where d = 0"""
    dt = Sc.dtype.type
    T = ((d[:, None] * Sc).astype(dt) * d[None, :]).astype(dt)
    zero = d == 0
    T[zero, :] = 0; T[:, zero] = 0; T[zero, zero] = 1
    return T


class TwoLevelM:
    """the camera blocks' G^T G plus the coarse term"""

    def __init__(self, M, coarse):
        self.M, self.coarse, self.fallbacks, self.parts = M, coarse, M.fallbacks, M.parts

    def __call__(self, r):
        return (self.M(r) + self.coarse.apply(r)).astype(F)


def two_level_system(base=ExplicitSchurSystem, mask=None, k=None, agg=None, dtype=F):
    """base (under the mask: held_system) with M^-1 = G^T G + P Z^T Z P^T; the aggregates: agg, or greedy with at most k (None: the default) cameras"""
    cls = base if mask is None or not np.asarray(mask).any() else held_system(base, np.asarray(mask, bool))

    def init(self, J, Hs, shift, pre, b, C):
        cls.__init__(self, J, Hs, shift, pre, b, C)
        self.agg = np.asarray(agg, np.int64) if agg is not None else greedy_aggregates(self.st, k or default_k(C))[0]
        hold_c = None if mask is None else split(np.asarray(mask, bool), C)[0]
        self.block_M = self.M
        if hold_c is not None and hold_c.all(): return      # (every camera held: the reduced system is empty, Plan::schur_empty)
        self.coarse = Coarse(self.st, self.S, self.agg, hold_c, dtype)
        self.M = TwoLevelM(self.M, self.coarse)
    return type("TwoLevel", (cls,), {"__init__": init})


class BaTwoLevelMirror(HeldSchurMirror):
    """BaSchurMirror's loops on the assembled S with the two-level preconditioner, with or without a mask"""

    def __init__(self, dims, params, mask=None, k=None, agg=None):
        C, P = dims[0], dims[1]
        super().__init__(dims, params, np.zeros(9 * C + 3 * P, bool) if mask is None else mask)
        self.k, self.agg = k, agg
        self.failed = 0

    def _held(self, f, *a, **kw):
        saved = bsm.SchurSystem
        bsm.SchurSystem = two_level_system(ExplicitSchurSystem, self.mask if self.mask.any() else None, self.k, self.agg)
        try: return f(*a, **kw)
        finally: bsm.SchurSystem = saved


# ------------------------------------------------------------------ iteration counts
def dense_precond32(sys):
    """the camera blocks' G^T G of a system as a dense float32 matrix [9 C, 9 C]"""
    G = np.asarray(sys.block_M.parts[0][1] if hasattr(sys, "block_M") else sys.M.parts[0][1], np.float64)
    C = len(G)
    M = np.zeros((9 * C, 9 * C))
    for c in range(C): M[9 * c:9 * c + 9, 9 * c:9 * c + 9] = G[c].T @ G[c]
    return M.astype(F)


def pcg32(S, Minv, b, tol=1e-6, max_it=5000):
    """float32 PCG with plain mat-vecs; Minv: a matrix or a callable -> (x, iterations, sqrt(r . z / r0 . z0) at the end)"""
    M = (lambda r: (Minv @ r).astype(F)) if not callable(Minv) else Minv
    b = np.asarray(b, F)
    x = np.zeros_like(b); r = b.copy(); z = M(r); p = z.copy()
    rz = F(r @ z); r0 = rz
    rel = 1.0
    for it in range(1, max_it + 1):
        Ap = (S @ p).astype(F)
        pAp = F(p @ Ap)
        if not pAp > 0: return x, it, rel
        alpha = F(rz / pAp)
        x = (x + alpha * p).astype(F); r = (r - alpha * Ap).astype(F)
        z = M(r); rz_new = F(r @ z)
        rel = float(np.sqrt(abs(float(rz_new)) / float(r0)))
        if rel <= tol: return x, it, rel
        p = (z + F(rz_new / rz) * p).astype(F); rz = rz_new
    return x, max_it, rel


def shuffled_cameras(params, seed=3):
    """the instance with its camera ids permuted (new id perm[c] for camera c): the same problem, the chain no longer in id order"""
    cams, pts, obs, oc, op = params
    perm = np.random.default_rng(seed).permutation(len(cams))
    new = np.empty_like(cams); new[perm] = cams
    return [np.ascontiguousarray(new), pts, obs, np.ascontiguousarray(perm[oc].astype(oc.dtype)), op]


# ------------------------------------------------------------------ float32 in the kernels' order
def _mul(a, b): return (np.asarray(a, F) * np.asarray(b, F)).astype(F)
def _add(a, b): return (np.asarray(a, F) + np.asarray(b, F)).astype(F)


def assemble32(st, S, agg, mem_ptr, mem, hold_c=None):
    """k_coarse_assemble: accumulator (a, b, entry), b <= a, takes the members of a in list order and a row's blocks in ascending column; a held row or column adds nothing
    -> the dense lower triangle [9 K, 9 K] float32 (zeros above the diagonal)"""
    S = np.asarray(S, F)
    K = len(mem_ptr) - 1
    acc = np.zeros((K, K, 9, 9), F)
    hold = np.zeros((st.C, 9), bool) if hold_c is None else np.asarray(hold_c, bool)
    for a in range(K):
        for c in mem[mem_ptr[a]:mem_ptr[a + 1]]:
            for t in range(st.row_ptr[c], st.row_ptr[c + 1]):
                cj = st.col[t]; b = agg[cj]
                if b > a: continue
                keep = ~(hold[c][:, None] | hold[cj][None, :])
                acc[a, b] = _add(acc[a, b], np.where(keep, S[t], F(0)))
    return np.tril(acc.transpose(0, 2, 1, 3).reshape(9 * K, 9 * K))


def scale32(Sc):
    """k_coarse_d / k_coarse_scale on the lower triangle -> (T, d, identity rows)"""
    Sc = np.asarray(Sc, F)
    diag = np.diag(Sc)
    with np.errstate(all="ignore"):
        d = np.where(diag > 0, (F(1) / np.sqrt(np.where(diag > 0, diag, F(1)), dtype=F)).astype(F), F(0)).astype(F)
    return np.tril(scale(Sc, d)), d, int((d == 0).sum())


def _wave_rows(M, x, lower):
    """per row i the dot product of M[i] and x over j <= i (lower) or j >= i: lane l adds its j = l, l + 64, ... in ascending order, then the wave butterfly -> [n] float32"""
    n = len(x)
    out = np.zeros(n, F)
    pad = -(-n // 64) * 64
    for i in range(n):
        prod = np.zeros(pad, F)
        j = np.arange(0, i + 1) if lower else np.arange(i, n)
        prod[j] = _mul(M[i, j], x[j])
        lanes = np.zeros(64, F)
        for k in range(pad // 64): lanes = _add(lanes, prod[64 * k:64 * k + 64])      # (a lane's missing terms add +0.0f)
        m = 32
        while m >= 1:
            lanes = _add(lanes[:m], lanes[m:2 * m]); m //= 2
        out[i] = lanes[0]
    return out


def apply32(Z, Zt, mem_ptr, mem, r, hold_c=None):
    """k_coarse_apply_a / _b: r_c over the member lists in list order, y = Z r_c and t = Z^T y by rows, the partials of y . y per workgroup (four waves, a row each per
    trip), then the scatter -> (the coarse term [9 C] float32, y, partials)"""
    r = np.asarray(r, F).reshape(-1, 9)
    C = len(r); K = len(mem_ptr) - 1; n = 9 * K
    hold = np.zeros((C, 9), bool) if hold_c is None else np.asarray(hold_c, bool)
    rc = np.zeros((K, 9), F)
    for a in range(K):
        for c in mem[mem_ptr[a]:mem_ptr[a + 1]]: rc[a] = _add(rc[a], np.where(hold[c], F(0), r[c]))
    y = _wave_rows(np.asarray(Z, F), rc.ravel(), True)
    grid = min(-(-n // 4), PARTIALS)
    part = np.zeros(grid, F)
    for w in range(grid):
        red = np.zeros(4, F)
        for wave in range(4):
            for i in range(4 * w + wave, n, 4 * grid): red[wave] = _add(red[wave], _mul(y[i], y[i]))
        part[w] = _add(_add(_add(red[0], red[1]), red[2]), red[3])
    t = _wave_rows(np.asarray(Zt, F), y, False).reshape(K, 9)
    out = np.zeros((C, 9), F)
    for a in range(K):
        for c in mem[mem_ptr[a]:mem_ptr[a + 1]]: out[c] = np.where(hold[c], F(0), t[a])
    return out.ravel(), y, part


def apply_cols32(Z, Zt, mem_ptr, mem, R, hold_c=None):
    """k_coarse_rc_cols / _y_cols / _t_cols on a panel R [C, 9, K]: one lane per column, every sum sequential in ascending j -> (the coarse term [C, 9, K], Y [n, K])"""
    R = np.asarray(R, F)
    C, _, Kc = R.shape; K = len(mem_ptr) - 1; n = 9 * K
    Z, Zt = np.asarray(Z, F), np.asarray(Zt, F)
    hold = np.zeros((C, 9), bool) if hold_c is None else np.asarray(hold_c, bool)
    rc = np.zeros((K, 9, Kc), F)
    for a in range(K):
        for c in mem[mem_ptr[a]:mem_ptr[a + 1]]: rc[a] = _add(rc[a], np.where(hold[c][:, None], F(0), R[c]))
    rc = rc.reshape(n, Kc)
    Y = np.zeros((n, Kc), F); T = np.zeros((n, Kc), F)
    for i in range(n):
        for j in range(i + 1): Y[i] = _add(Y[i], _mul(Z[i, j], rc[j]))
    for i in range(n):
        for j in range(i, n): T[i] = _add(T[i], _mul(Zt[i, j], Y[j]))
    T = T.reshape(K, 9, Kc)
    out = np.zeros_like(R)
    for a in range(K):
        for c in mem[mem_ptr[a]:mem_ptr[a + 1]]: out[c] = np.where(hold[c][:, None], F(0), T[a])
    return out, Y


def two_level_column_pcg(pcg, coarse):
    """a ColumnPCG32 (tests/ba_covariance_mirror.py) whose Z = M^-1 R adds the coarse term of `coarse` (a float32 Coarse on the same S and mask); r . z is the dot of the
    complete z -- iteration counts and the converged columns, not the device's bits"""
    import copy
    import ba_covariance_mirror as cm
    base = type(pcg)

    class TwoLevelColumnPCG32(base):
        def precond(self, R, live=None):
            Zb, _ = base.precond(self, R, None)
            n = 9 * self.C
            Z = _add(Zb, coarse.apply(R.reshape(n, -1)).reshape(Zb.shape))
            part = self._partials(R, Z)
            if live is not None: Z[:, :, ~live] = 0; part[:, ~live] = 0
            return Z, part
    out = copy.copy(pcg)
    out.__class__ = TwoLevelColumnPCG32
    return out
