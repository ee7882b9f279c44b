"""CPU restatement of bundle adjustment's marginal covariances (thallo_amd/csrc/ba_covariance.hip, ThalloX_PlanCovariance) -- TEST INFRASTRUCTURE, not a test.

With A = J^T J at the current unknowns (J carries the robust weights where a loss is in force; no LM diagonal), F the scalars the caller does not hold and
Sigma = (A_FF)^-1 bordered by zeros, through the Schur complement on the cameras

  Sigma_cc = S^-1 on the free cameras,      Sigma_pp = Cp^-1 + V^T S^-1 V,   V = E_p Cp^-1 (W_q G_p at the rows of camera c(q)),   Cp^-1 = G^T G

  float64   dense_cov64 (the dense inverse of A_FF from the oracle's J), inv_s_ff64 (inv(S_FF) from a given S), point_formula64 and schur_cov64 (the Schur route)
  float32   ColumnPCG32: the column PCG in the kernels' order on an ExplicitSchurSystem (tests/ba_schur_explicit_mirror.py; with a mask: tests/ba_held_mirror.py's
            held_system) -- panels [C, 9, K], one column per lane, every product and every addition rounded on its own, elementwise numpy: the same numbers on every
            machine.  The device differs by its fused multiply-adds.
  cov_error the measure of a covariance: max |Sigma - Sigma_ref|_ab / sqrt(Sigma_ref,aa Sigma_ref,bb) over the free scalars of the blocks; held rows are compared exactly"""
import numpy as np

from ba_block_mirror import guarded_invert
from ba_held_mirror import held_system
from ba_schur_explicit_mirror import ExplicitSchurSystem

F = np.float32
K = 64                    # THALLO_HIP_COV_K
MAX_PARTIALS = 1024


def gauge_mask(C, P):
    """the tests' gauge: camera 0 entirely and scalar 3 of camera 1 -> flat bool [9 C + 3 P]"""
    m = np.zeros(9 * C + 3 * P, bool)
    m[:9] = True; m[9 + 3] = True
    return m


def system_of(m, mask=None):
    """a mirror's (anything with linearise() and C) assembled GN system at its current unknowns -> (J float64 CSR, ExplicitSchurSystem), under the mask where one is given"""
    J, r, d, Hs = m.linearise()
    cls = ExplicitSchurSystem if mask is None else held_system(ExplicitSchurSystem, np.asarray(mask, bool))
    return J, cls(J, Hs, None, guarded_invert(d), r, m.C)


# ------------------------------------------------------------------ float64
def undetermined(A, C):
    """scalars of elements that A does not determine by themselves: cameras nothing observes and points observed once or never (their block of A is singular) -> bool [n]"""
    A = np.asarray(A)
    n = len(A); nc = 9 * C
    out = np.zeros(n, bool)
    for lo, hi, d in ((0, nc, 9), (nc, n, 3)):
        for s in range(lo, hi, d):
            blk = A[s:s + d, s:s + d]
            if not np.diag(blk).all() or np.linalg.matrix_rank(blk) < d: out[s:s + d] = True
    return out


def dense_cov64(A, free):
    """(A_FF)^-1 bordered by zeros -> [n, n]"""
    A = np.asarray(A, np.float64)
    f = np.nonzero(free)[0]
    Sig = np.zeros_like(A)
    Sig[np.ix_(f, f)] = np.linalg.inv(A[np.ix_(f, f)])
    return Sig


def blocks_of(Sig, ids, d, offset=0):
    return np.stack([Sig[offset + d * i:offset + d * i + d, offset + d * i:offset + d * i + d] for i in ids])


def inv_s_ff64(S, free_c):
    """inv(S_FF) of a dense S (9 C x 9 C) on the free camera scalars, bordered by zeros"""
    return dense_cov64(S, free_c)


def point_formula64(A, free, Sig_cc, p, C):
    """Sigma_pp = Cp^-1 + V^T Sigma_cc V, V = E_p Cp^-1 (both on the free scalars, bordered by zeros) -> [3, 3]"""
    A = np.asarray(A, np.float64); nc = 9 * C
    s = nc + 3 * p
    Ci = dense_cov64(A[s:s + 3, s:s + 3], free[s:s + 3])
    V = (A[:nc, s:s + 3] * free[:nc, None]) @ Ci
    return Ci + V.T @ Sig_cc @ V


def schur_cov64(A, free, C):
    """the Schur route in float64: S = B - E Cp^-1 E^T over the free scalars, Sigma_cc = inv(S_FF) -> (Sigma_cc [9 C, 9 C], f(p) -> Sigma_pp)"""
    A = np.asarray(A, np.float64); nc = 9 * C; P = (len(A) - nc) // 3
    Ci = np.zeros((len(A) - nc, len(A) - nc))
    for p in range(P):
        s = 3 * p
        Ci[s:s + 3, s:s + 3] = dense_cov64(A[nc + s:nc + s + 3, nc + s:nc + s + 3], free[nc + s:nc + s + 3])
    E = A[:nc, nc:]
    S = A[:nc, :nc] - E @ Ci @ E.T
    Sig_cc = inv_s_ff64(S, free[:nc])
    return Sig_cc, lambda p: point_formula64(A, free, Sig_cc, p, C)


def cov_error(got, ref, free):
    """got, ref [n, d, d]; free [n, d] bool -> max |got - ref|_ab / sqrt(ref_aa ref_bb) over the free scalars; rows and columns of the others must be exactly zero"""
    worst = 0.0
    for g, r, f in zip(np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(free, bool)):
        assert not g[~f].any() and not g[:, ~f].any(), "a held scalar's row or column is not exactly zero"
        if not f.any(): continue
        s = np.sqrt(np.diag(r)[f])
        worst = max(worst, float((np.abs(g - r)[np.ix_(f, f)] / np.outer(s, s)).max()))
    return worst


# ------------------------------------------------------------------ float32 in the kernels' order
def _mul(a, b): return (np.asarray(a, F) * np.asarray(b, F)).astype(F)
def _add(a, b): return (np.asarray(a, F) + np.asarray(b, F)).astype(F)


def scal_sum(part):
    """k_cov_scal: four waves, each its quarter of the partials in ascending order, then ((s0 + s1) + s2) + s3; part [nparts, K] -> [K]"""
    n = len(part); per = (n + 3) // 4
    s = []
    for v in range(4):
        acc = np.zeros(part.shape[1], F)
        for w in range(v * per, min(n, (v + 1) * per)): acc = _add(acc, part[w])
        s.append(acc)
    return _add(_add(_add(s[0], s[1]), s[2]), s[3])


class ColumnPCG32:
    """the kernels of ba_covariance.hip on the parts of an ExplicitSchurSystem: S [nblk, 9, 9] and its structure, the camera blocks' factor Gc [C, 9, 9], the elimination
    factor Ge [P, 3, 3], W [O, 9, 3] (camera order) and the point lists; hold: the flat mask or None"""

    def __init__(self, st, S, Gc, Ge, W, lists, hold=None):
        self.st, self.S, self.Gc, self.Ge, self.W, self.L = st, np.asarray(S, F), np.asarray(Gc, F), np.asarray(Ge, F), np.asarray(W, F), lists
        self.C, self.P = st.C, len(Ge)
        self.hold = None if hold is None else np.asarray(hold, bool)
        self.grid = min(self.C, MAX_PARTIALS)
        self.cnt = np.diff(st.row_ptr)

    @classmethod
    def of(cls, sys, hold=None):
        return cls(sys.st, sys.S, sys.M.parts[0][1], sys.G, sys.W, sys.lists, hold)

    def _partials(self, a, b):
        """per workgroup w the cameras w, w + grid, ... in order, acc += a b over the nine scalars; a, b [C, 9, K] -> [grid, K]"""
        part = np.zeros((self.grid, a.shape[2]), F)
        for c0 in range(0, self.C, self.grid):
            n = min(self.grid, self.C - c0)
            for i in range(9): part[:n] = _add(part[:n], _mul(a[c0:c0 + n, i], b[c0:c0 + n, i]))
        return part

    def apply(self, X):
        """k_apply_s_cols: per row the blocks in ascending order, y[a] += S[a, b] x[b] with b ascending -> (Y, partials of x . S x)"""
        st = self.st
        Y = np.zeros_like(X)
        for t in range(int(self.cnt.max())):
            m = np.nonzero(self.cnt > t)[0]
            blk = st.row_ptr[m] + t
            Sb, xv = self.S[blk], X[st.col[blk]]
            for b in range(9): Y[m] = _add(Y[m], _mul(Sb[:, :, b, None], xv[:, None, b, :]))
        return Y, self._partials(X, Y)

    def precond(self, R, live=None):
        """k_cov_step: z = G^T (G r) per camera (block_chol.hpp apply_g) -> (Z, partials of r . z); live: the columns that are computed (the others: z = 0 here, a zero partial)"""
        G = self.Gc
        y = np.zeros_like(R); Z = np.zeros_like(R)
        for i in range(9):
            for j in range(i + 1): y[:, i] = _add(y[:, i], _mul(G[:, i, j, None], R[:, j]))
        for j in range(9):
            for i in range(j, 9): Z[:, j] = _add(Z[:, j], _mul(G[:, i, j, None], y[:, i]))
        part = self._partials(R, Z)
        if live is not None: Z[:, :, ~live] = 0; part[:, ~live] = 0
        return Z, part

    def _v(self, q, p):
        """V_q = W_q G_p, [9, 3]: (w0 g00 + w1 g10) + w2 g20, w1 g11 + w2 g21, w2 g22"""
        w, g = self.W[q], self.Ge[p]
        v0 = _add(_add(_mul(w[:, 0], g[0, 0]), _mul(w[:, 1], g[1, 0])), _mul(w[:, 2], g[2, 0]))
        v1 = _add(_mul(w[:, 1], g[1, 1]), _mul(w[:, 2], g[2, 1]))
        return np.stack([v0, v1, _mul(w[:, 2], g[2, 2])], 1)

    def _list(self, p):
        for t in range(self.L.pt_ptr[p], self.L.pt_ptr[p + 1]):
            q = int(self.L.pt_pos[t])
            yield q, int(self.L.q_cam[q])

    def rhs(self, mode, ids):
        """k_cov_rhs -> R [C, 9, K]"""
        R = np.zeros((self.C, 9, K), F)
        assert 1 <= len(ids) <= (K // 9 if mode == 0 else K // 3)
        for j, i in enumerate(ids):
            if mode == 0:
                for a in range(9): R[i, a, 9 * j + a] = 1
            else:
                for q, c in self._list(i): R[c, :, 3 * j:3 * j + 3] = _add(R[c, :, 3 * j:3 * j + 3], self._v(q, i))
        return R

    def solve_panel(self, R, rel_tol=1e-6, max_iterations=500):
        """the PCG of thallo_hip_ba_cov_solve on a panel of right-hand sides -> (X, info): iterations (until every column is frozen), frozen, aN, r0 per column"""
        R = np.array(R, F)
        tol2 = F(F(rel_tol) * F(rel_tol))
        X = np.zeros_like(R)
        Z, pb = self.precond(R)
        aN = scal_sum(pb); r0 = aN.copy()
        with np.errstate(all="ignore"):
            frozen = aN <= _mul(tol2, aN)
            P = None; beta = np.zeros(R.shape[2], F); it = 0
            while it < max_iterations and not frozen.all():
                P = Z.copy() if it == 0 else _add(Z, _mul(beta, P))
                Y, pa = self.apply(P)
                s = scal_sum(pa)
                live = ~frozen
                alpha = np.where(live & (s > 0), (aN / np.where(s > 0, s, F(1))).astype(F), F(0)).astype(F)
                X[:, :, live] = _add(X, _mul(alpha, P))[:, :, live]
                R[:, :, live] = (R - _mul(alpha, Y)).astype(F)[:, :, live]
                Zn, pb = self.precond(R, live)
                Z[:, :, live] = Zn[:, :, live]
                s = scal_sum(pb)
                beta = np.where(live & (aN > 0), (s / np.where(aN > 0, aN, F(1))).astype(F), F(0)).astype(F)
                aN = np.where(live, s, aN).astype(F)
                frozen = frozen | (live & (s <= _mul(tol2, r0)))
                it += 1
        return X, dict(iterations=it, frozen=frozen, aN=aN, r0=r0)

    def out(self, mode, ids, X):
        """k_cov_out -> (blocks, blocks filled with NaN)"""
        if mode == 0:
            B = np.stack([X[c, :, 9 * j:9 * j + 9] for j, c in enumerate(ids)])
            return _mul(F(0.5), _add(B, np.transpose(B, (0, 2, 1)))), 0
        out = np.zeros((len(ids), 3, 3), F); nans = 0
        for j, p in enumerate(ids):
            g = self.Ge[p]
            if not g.any():
                callers = self.hold is not None and self.hold[9 * self.C + 3 * p:9 * self.C + 3 * p + 3].all()
                if not callers: out[j] = np.nan; nans += 1
                continue
            acc = np.zeros((3, 3), F)                       # acc[m, n] = sum over the list and a of V[a, m] x[a, n]
            for q, c in self._list(p):
                V, x = self._v(q, p), X[c, :, 3 * j:3 * j + 3]
                for a in range(9): acc = _add(acc, _mul(V[a][:, None], x[a][None, :]))
            gtg = np.zeros((3, 3), F)
            for l in range(3): gtg = _add(gtg, _mul(g[l][:, None], g[l][None, :]))
            t = _add(gtg, acc)
            out[j] = _mul(F(0.5), _add(t, t.T))
        return out, nans

    def solve(self, mode, ids, rel_tol=1e-6, max_iterations=500):
        """all requests, in batches of 7 cameras or 21 points -> (blocks, info as ThalloX_CovarianceInfo adds it up; iterations: until the batch's columns are frozen)"""
        per = K // 9 if mode == 0 else K // 3
        blocks = []; info = dict(iterations=0, columns=0, not_converged=0, nan_blocks=0, worst_residual=0.0, batch_iterations=[])
        for b0 in range(0, len(ids), per):
            batch = list(ids[b0:b0 + per])
            X, i = self.solve_panel(self.rhs(mode, batch), rel_tol, max_iterations)
            B, nans = self.out(mode, batch, X)
            blocks.append(B)
            cols = np.arange(len(batch) * (9 if mode == 0 else 3))
            solved = cols[i["r0"][cols] > 0]
            info["iterations"] += i["iterations"]; info["batch_iterations"].append(i["iterations"]); info["columns"] += len(solved)
            info["not_converged"] += int((~i["frozen"][solved]).sum()); info["nan_blocks"] += nans
            if len(solved): info["worst_residual"] = max(info["worst_residual"], float(np.sqrt(i["aN"][solved].astype(np.float64) / i["r0"][solved]).max()))
        return np.concatenate(blocks), info
