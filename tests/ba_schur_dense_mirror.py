"""CPU restatement of bundle adjustment's dense Cholesky Schur solve (thallo_amd/csrc/ba_schur_dense.hip, ThalloX_PlanSetLinearSolver kind 3) -- TEST INFRASTRUCTURE, not a
test.  Everything up to and including the assembly of S is tests/ba_schur_explicit_mirror.py's (with a mask: tests/ba_held_mirror.py's), which this file imports and
leaves as it is; only the reduced loop is replaced:

  expand   T = D S D of the float32 assembled S, D = diag(S_ii)^-1/2 in float32, entry (i, j) = float32(float32(d_i S_ij) d_j); a scalar the mask holds, and one whose S_ii
           is not positive (a camera nothing observes), gets d = 0 and the identity's row and column; the latter are counted
  factor   float32 LAPACK Cholesky (spotrf: what scipy.linalg.cholesky calls, asked directly for its info word).  A pivot that is not positive is a DensePivot: the step
           is not taken, the unknowns keep their bits
  solve    delta_c = D L^-T L^-1 D g by two float32 triangular solves (strtrs); exactly 0.0f at the identity rows
  the rest back-substitution, model cost, accept / revert and the trust region as BaSchurMirror runs them behind a loop that took no iteration

The covariance through the factor: X = D L^-T L^-1 D R on ColumnPCG32's right-hand sides, ColumnPCG32's output contraction."""
import numpy as np
import scipy.linalg as sla

from oracle import oracle as orc

import ba_covariance_mirror as cm
from ba_block_mirror import guarded_invert
from ba_held_mirror import held_system
from ba_schur_explicit_mirror import BaSchurExplicitMirror, ExplicitSchurSystem

F = np.float32


class DensePivot(Exception):
    """the factor met a pivot that is not positive at this index of the 9 C camera scalars"""

    def __init__(self, index):
        super().__init__("pivot %d (camera %d, scalar %d) is not positive" % (index, index // 9, index % 9))
        self.index, self.camera, self.scalar = int(index), int(index) // 9, int(index) % 9


def expand32(S, hold_c):
    """dense float32 S [n, n], hold_c bool [n] -> (T float32 [n, n] symmetric with a unit diagonal and identity rows, d float32 [n], non-positive diagonals)"""
    S = np.asarray(S, F); hold_c = np.asarray(hold_c, bool)
    diag = S.diagonal()
    nonpos = ~hold_c & ~(diag > 0)
    live = ~hold_c & ~nonpos
    d = np.zeros(len(S), F)
    d[live] = (F(1) / np.sqrt(diag[live])).astype(F)
    T = ((d[:, None] * S).astype(F) * d[None, :]).astype(F)
    dead = ~live
    T[dead, :] = 0; T[:, dead] = 0
    T[dead, dead] = 1
    return T, d, int(nonpos.sum())


def factor32(T):
    """float32 lower Cholesky factor, or DensePivot"""
    L, info = sla.lapack.spotrf(np.asarray(T, F), lower=1, clean=1)
    if info > 0: raise DensePivot(info - 1)
    assert info == 0 and L.dtype == F
    return L


def sweeps32(L, d, B):
    """D L^-T L^-1 D B for a float32 factor; B [n] or [n, k]"""
    Y = (d.reshape(-1, *([1] * (np.ndim(B) - 1))) * np.asarray(B, F)).astype(F)
    Y = sla.solve_triangular(L, Y, lower=True, check_finite=False)
    Y = sla.solve_triangular(L, Y, lower=True, trans="T", check_finite=False)
    assert Y.dtype == F
    return (d.reshape(-1, *([1] * (np.ndim(B) - 1))) * Y).astype(F)


def dense_system(mask=None):
    """ExplicitSchurSystem (under the mask where one is given) with the dense solve of its reduced system"""
    base = ExplicitSchurSystem if mask is None else held_system(ExplicitSchurSystem, np.asarray(mask, bool))
    hold = None if mask is None else np.asarray(mask, bool)

    class DenseSchurSystem(base):
        def dense(self):
            """-> (S dense float32, hold over the camera scalars)"""
            h = np.zeros(self.nc, bool) if hold is None else hold[:self.nc]
            return self.st.bsr(self.S).toarray().astype(F), h

        def factor(self):
            Sd, h = self.dense()
            T, self.d, self.nonpos = expand32(Sd, h)
            self.L = factor32(T)
            return self.L

        def solve(self):
            """delta_c; DensePivot where the factor fails"""
            self.factor()
            return sweeps32(self.L, self.d, self.g)

    return DenseSchurSystem


class BaSchurDenseMirror(BaSchurExplicitMirror):
    """BaSchurExplicitMirror with the reduced loop replaced by the dense solve; mask: flat bool [9 C + 3 P] or None.  A failed factor ends the solve: `pivot` holds the
    DensePivot, the unknowns are those before the step"""

    def __init__(self, dims, params, mask=None):
        super().__init__(dims, params)
        self.mask = None if mask is None else np.asarray(mask, bool)
        self.pivot = None
        self.nonpos = []

    def _system(self, J, Hs, shift, pre, b):
        S = dense_system(self.mask)(J, Hs, shift, pre, b, self.C)
        self.held.append(int(S.held.sum())); self.fallbacks += S.M.fallbacks
        return S

    def gn_step(self, L=0, kind="schur"):
        """-> True, or False with self.pivot set and the unknowns unchanged"""
        J, r, d, Hs = self.linearise()
        S = self._system(J, Hs, None, guarded_invert(d), r)
        try: dc = S.solve()
        except DensePivot as e:
            self.pivot = e
            return False
        self.nonpos.append(S.nonpos)
        self.last_system, self.last_delta_c = S, dc
        self._update(np.concatenate([dc, S.back(dc)]))
        return True

    def gn_solve(self, nit, lit=0, kind="schur"):
        costs = [float(self.cost())]
        for _ in range(nit):
            if not self.gn_step(): break
            costs.append(float(self.cost()))
        return costs

    def lm_solve(self, nit, lit=0, kind="schur", **kw):
        """-> (costs, linear iterations per step: zeros) -- BaSchurMirror.lm_solve with delta_c from the factor of S + CtC_c"""
        spm = orc.default_params(**kw)
        radius, dec = F(spm.trust_region_radius), F(spm.radius_decrease_factor)
        prev = self.cost(); costs = [float(prev)]; iters = []
        SSq = None
        for it in range(nit):
            J, r, d, Hs = self.linearise()
            if it == 0: SSq = guarded_invert(d)
            unclamped = (d * (F(1) / radius)).astype(F)
            cmx = ((F(1) / SSq) / radius).astype(F)
            CtC = np.minimum(np.maximum(unclamped, F(spm.min_lm_diagonal) * cmx), F(spm.max_lm_diagonal) * cmx).astype(F)
            pre = (F(1) / (CtC + radius * unclamped)).astype(F)
            b = r.copy()
            S = self._system(J, Hs, CtC, pre, b)
            try: dc = S.solve()
            except DensePivot as e:
                self.pivot = e
                break
            self.nonpos.append(S.nonpos)
            iters.append(0)
            delta = np.concatenate([dc, S.back(dc)])
            Ad = (J.T @ (J @ delta.astype(np.float64)))
            dJJd, db = F(float(delta.astype(np.float64) @ Ad)), self._dot(delta, b)
            prevX = [self.params[0].copy(), self.params[1].copy()]
            self._update(delta)
            new = self.cost()
            model = F(db - F(0.5) * dJJd)
            change = F(prev - new); rel = F(change / model)
            if change >= 0 and rel > F(spm.min_relative_decrease):
                if change <= prev * F(spm.function_tolerance):
                    costs.append(float(new)); break
                tmp = 1.0 - (2.0 * float(rel) - 1.0) ** 3
                radius = F(min(float(F(float(radius) / max(1.0 / 3.0, tmp))), spm.max_trust_region_radius)); dec = F(2); prev = new
            else:
                self.params[0][:] = prevX[0]; self.params[1][:] = prevX[1]
                radius = F(radius / dec); dec = F(2 * dec)
                if radius < F(spm.min_trust_region_radius):
                    costs.append(float(prev)); break
            costs.append(float(self.cost()))
        return costs, iters


def gn_system(m, mask=None):
    """a mirror's assembled GN system at its current unknowns with the dense solve -> (J float64 CSR, DenseSchurSystem)"""
    J, r, d, Hs = m.linearise()
    return J, dense_system(mask)(J, Hs, None, guarded_invert(d), r, m.C)


class DenseCovariance:
    """ThalloX_PlanCovariance on a plan of kind 3: ColumnPCG32's right-hand sides and output contraction around two triangular sweeps per batch; one factor per object"""

    def __init__(self, sys, mask):
        self.sys = sys
        self.pcg = cm.ColumnPCG32.of(sys, mask)
        self.hold_c = np.zeros(sys.nc, bool) if mask is None else np.asarray(mask, bool)[:sys.nc]
        sys.factor()                                  # DensePivot where it fails

    def solve(self, mode, ids):
        """-> (blocks, info as ThalloX_CovarianceInfo reports it)"""
        sys, pcg = self.sys, self.pcg
        per = cm.K // 9 if mode == 0 else cm.K // 3
        blocks = []; info = dict(iterations=0, columns=0, not_converged=0, nan_blocks=0, worst_residual=0.0)
        for b0 in range(0, len(ids), per):
            batch = list(ids[b0:b0 + per])
            R = pcg.rhs(mode, batch).reshape(sys.nc, cm.K)
            X = sweeps32(sys.L, sys.d, R).reshape(sys.nc // 9, 9, cm.K)
            B, nans = pcg.out(mode, batch, X)
            blocks.append(B); info["nan_blocks"] += nans
        if mode == 0:
            for c in ids:
                for a in range(9):
                    u = 9 * c + a
                    if self.hold_c[u]: continue
                    if sys.d[u] > 0: info["columns"] += 1
                    else: info["not_converged"] += 1
        else: info["columns"] = 3 * len(ids) - 3 * info["nan_blocks"]
        return np.concatenate(blocks), info
