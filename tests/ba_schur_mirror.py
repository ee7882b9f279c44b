"""CPU restatement of bundle adjustment's opt-in Schur-complement solve (thallo_amd/csrc/ba_schur.hip, ThalloX_PlanSetLinearSolver) -- TEST INFRASTRUCTURE, not a test.
On tests/ba_block_mirror.py's conventions: the oracle's CSR for J, float32 state, float64 sums for the scalars, one float32 rounding per vector operation.

With A = J^T J (+ diag(CtC) in LM) = [[B, E], [E^T, Cp]] over [cameras | points] and b = -J^T F = [b_c; b_p]:

  1. factor   the camera blocks as the block preconditioner does (BlockPrecond "block32" on the camera region: they precondition the reduced system); the point blocks for
              ELIMINATION: the same scaled Cholesky in the device's order (elim_factor32, elementwise numpy), G = L^-1 S, Cp^-1 = G^T G, and a point whose block has a B_ii
              that is not a positive finite number, a squared pivot of the unit-diagonal scaled block below 2^-16 or a non-finite G is HELD: G = 0
  2. reduce   y = Cp^-1 b_p;  g = b_c - E y
  3. apply    S x = J_c^T (I - J_p Cp^-1 J_p^T) J_c x (+ CtC_c x_c in LM), in residual space
  4. PCG on (S, g) with M^-1 = the camera blocks' G^T G: BaBlockMirror's GN loop, and the reference-shaped LM loop with b := g and Q_k = 0.5 delta_c . (r_c + g)
  5. back     delta_p = Cp^-1 (b_p - E^T delta_c); everything behind the loop (model cost on the full J^T J, accept / revert, trust region) on the complete delta."""
import numpy as np
import scipy.sparse as sp

from oracle import oracle as orc

from ba_block_mirror import BaBlockMirror, BlockPrecond, guarded_invert

F = np.float32
PIVOT_FLOOR = F(2.0 ** -16)


def elim_factor32(H, sh):
    """[P, 3, 3] float64 blocks, [P, 3] shift -> (G [P, 3, 3] float32 lower triangular, held [P] bool): ba_schur.hip factor3 step by step, every operation rounded to float32 on
    its own, vectorised over the points (BlockPrecond._factor's float32 branch with the elimination rule instead of the diagonal fallback)"""
    n = 3; idx = np.arange(n); nb = H.shape[0]
    a = H.astype(F); a[:, idx, idx] = (a[:, idx, idx] + sh.astype(F)).astype(F)
    d = a[:, idx, idx]
    ok = ((d > 0) & np.isfinite(d)).all(1)
    inv = np.zeros((nb, n), F)
    with np.errstate(all="ignore"):
        s = (F(1) / np.sqrt(d)).astype(F)
        a = ((a * s[:, :, None]).astype(F) * s[:, None, :]).astype(F)
        for j in range(n):
            dd = a[:, j, j].copy()
            for k in range(j): dd = (dd - (a[:, j, k] * a[:, j, k]).astype(F)).astype(F)
            ok &= (dd >= PIVOT_FLOOR) & np.isfinite(dd)
            inv[:, j] = (F(1) / np.sqrt(dd)).astype(F)
            for i in range(j + 1, n):
                v = a[:, i, j].copy()
                for k in range(j): v = (v - (a[:, i, k] * a[:, j, k]).astype(F)).astype(F)
                a[:, i, j] = (v * inv[:, j]).astype(F)
        for i in range(n):
            li = a[:, i, :].copy()
            for j in range(i):
                v = (li[:, j] * inv[:, j]).astype(F)
                for k in range(j + 1, i): v = (v + (li[:, k] * a[:, k, j]).astype(F)).astype(F)
                a[:, i, j] = (-inv[:, i] * v).astype(F)
            a[:, i, i] = inv[:, i]
        G = (np.tril(a) * s[:, None, :]).astype(F)
    ok &= np.isfinite(G).all((1, 2))
    G[~ok] = 0
    return G, ~ok


def block_diag3(M):
    """[P, 3, 3] -> sparse block-diagonal [3 P, 3 P]"""
    nb = M.shape[0]
    r = (3 * np.arange(nb)[:, None, None] + np.arange(3)[None, :, None] + np.zeros((1, 1, 3), np.int64)).ravel()
    c = (3 * np.arange(nb)[:, None, None] + np.zeros((1, 3, 1), np.int64) + np.arange(3)[None, None, :]).ravel()
    return sp.csr_matrix((M.ravel(), (r, c)), shape=(3 * nb, 3 * nb))


def dense_reduced_solve(A, b, nc):
    """float64: delta from the dense Schur complement of A (sparse or dense, symmetric positive definite) on its first nc unknowns, the rest by back-substitution
    -> (delta, S, g)"""
    A = np.asarray(A.todense()) if sp.issparse(A) else np.asarray(A, np.float64)
    B, E, Cp = A[:nc, :nc], A[:nc, nc:], A[nc:, nc:]
    CiEt = np.linalg.solve(Cp, E.T); Cib = np.linalg.solve(Cp, b[nc:])
    S = B - E @ CiEt; g = b[:nc] - E @ Cib
    dc = np.linalg.solve(S, g)
    dp = Cib - CiEt @ dc
    return np.concatenate([dc, dp]), S, g


def with_extras(p):
    """the instance + one camera and one point that nothing observes + one point observed exactly once (by camera 0, next to the point of camera 0's first observation)
    -> (params, dims); the unobserved point is P, the once-observed one P + 1 (P: the instance's own point count)"""
    cams, pts, obs, oc, op = p
    rng = np.random.default_rng(5)
    P = len(pts)
    o0 = int(np.nonzero(oc == 0)[0][0])
    once = pts[op[o0]] + F(0.01) * rng.standard_normal(3).astype(F)
    q = [np.concatenate([cams, cams[:1] + F(0.01)]).astype(F), np.concatenate([pts, rng.standard_normal((1, 3)).astype(F), once[None]]).astype(F),
         np.concatenate([obs, obs[o0:o0 + 1]]).astype(F), np.concatenate([oc, [0]]).astype(np.int32), np.concatenate([op, [P + 1]]).astype(np.int32)]
    return [np.ascontiguousarray(a) for a in q], (len(q[0]), len(q[1]), len(q[2]))


class SchurSystem:
    """Steps 1 - 3 and 5 of one GN / LM step: J float64 CSR, Hs the stacked blocks of J^T J, shift the LM CtC (flat, float32) or None, pre the point-Jacobi M^-1 (flat)"""

    def __init__(self, J, Hs, shift, pre, b, C):
        self.nc = nc = 9 * C
        J = sp.csc_matrix(J)
        self.Jc, self.Jp = sp.csr_matrix(J[:, :nc]), sp.csr_matrix(J[:, nc:])
        P = Hs[1].shape[0]
        sh = np.zeros((P, 3)) if shift is None else np.asarray(shift[nc:], np.float64).reshape(P, 3)
        self.G, self.held = elim_factor32(Hs[1], sh)
        G64 = self.G.astype(np.float64)
        self.Cinv = block_diag3(np.einsum("bki,bkj->bij", G64, G64))          # G^T G per point, the float32 G's exact product
        self.ctc_c = None if shift is None else np.asarray(shift[:nc], F)
        self.M = BlockPrecond("block32", (Hs[0], np.zeros((0, 3, 3))), None if shift is None else np.asarray(shift[:nc], F), np.asarray(pre[:nc], F), C)
        self.b = np.asarray(b, F)
        bp = self.b[nc:].astype(np.float64)
        self.y = (self.Cinv @ bp).astype(F)
        self.g = (self.b[:nc].astype(np.float64) - self.Jc.T @ (self.Jp @ self.y.astype(np.float64))).astype(F)

    def apply(self, x):
        u = self.Jc @ x.astype(np.float64)
        v = u - self.Jp @ (self.Cinv @ (self.Jp.T @ u))
        s = (self.Jc.T @ v).astype(F)
        return s if self.ctc_c is None else (s + self.ctc_c * x).astype(F)

    def back(self, dc):
        w = self.Jp.T @ (self.Jc @ dc.astype(np.float64))
        return (self.Cinv @ (self.b[self.nc:].astype(np.float64) - w)).astype(F)


class BaSchurMirror(BaBlockMirror):
    def __init__(self, dims, params):
        super().__init__(dims, params)
        self.held = []                          # held points of every step

    def gn_step(self, L, kind="schur"):
        J, r, d, Hs = self.linearise()
        S = SchurSystem(J, Hs, None, guarded_invert(d), r, self.C)
        self.held.append(int(S.held.sum())); self.fallbacks += S.M.fallbacks
        nc = self.nc
        r = S.g.copy(); z = S.M(r)
        aN = self._dot(r, z)
        p = np.zeros(nc, F); delta = np.zeros(nc, F)
        alpha = beta = F(0)
        for k in range(L):
            if k: delta = (delta + alpha * p).astype(F)
            p = (z + beta * p).astype(F) if k else z.copy()
            Ap = S.apply(p)
            aD = self._dot(p, Ap)
            alpha = F(aN / aD) if aD != 0 else F(0)
            r = (r - alpha * Ap).astype(F)
            z = S.M(r)
            bN = self._dot(z, r)
            beta = F(bN / aN) if aN != 0 else F(0)
            aN = bN
        if L: delta = (delta + alpha * p).astype(F)
        self._update(np.concatenate([delta, S.back(delta)]))

    def gn_solve(self, nit, lit, kind="schur"):
        return super().gn_solve(nit, lit, kind)

    def lm_solve(self, nit, lit, kind="schur", **kw):
        """-> (costs, PCG iterations per LM step): BaBlockMirror.lm_solve with the loop on the reduced system"""
        spm = orc.default_params(**kw)
        radius, dec = F(spm.trust_region_radius), F(spm.radius_decrease_factor)
        prev = self.cost(); costs = [float(prev)]; iters = []
        SSq = None; nc = self.nc
        for it in range(nit):
            J, r, d, Hs = self.linearise()
            if it == 0: SSq = guarded_invert(d)                                     # PCGSaveSSq
            unclamped = (d * (F(1) / radius)).astype(F)
            cm = ((F(1) / SSq) / radius).astype(F)
            CtC = np.minimum(np.maximum(unclamped, F(spm.min_lm_diagonal) * cm), F(spm.max_lm_diagonal) * cm).astype(F)
            pre = (F(1) / (CtC + radius * unclamped)).astype(F)
            b = r.copy()
            S = SchurSystem(J, Hs, CtC, pre, b, self.C)
            self.held.append(int(S.held.sum())); self.fallbacks += S.M.fallbacks
            g = S.g
            r = g.copy(); z = S.M(r)
            aN = self._dot(r, z)
            p = np.zeros(nc, F); delta = np.zeros(nc, F)
            Q0 = F(0); beta = F(0); done = 0
            for k in range(lit):
                p = (z + beta * p).astype(F) if k else z.copy()
                Ap = S.apply(p)
                aD = self._dot(p, Ap)
                with np.errstate(all="ignore"):
                    alpha = F(aN / aD)
                delta = (delta + alpha * p).astype(F)
                if (k + 1) % spm.residual_reset_period == 0:                        # :1653-1657 on the reduced system
                    r = (g - S.apply(delta)).astype(F)
                else:
                    r = (r - alpha * Ap).astype(F)
                z = S.M(r)
                bN = self._dot(z, r)
                Q1 = F(0.5 * float(delta.astype(np.float64) @ (r + g).astype(F).astype(np.float64)))
                with np.errstate(all="ignore"):
                    beta = F(bN / aN)
                aN = bN
                done = k + 1
                if not np.isfinite(Q1): break
                with np.errstate(all="ignore"):
                    zeta = F(k + 1) * (Q1 - Q0) / Q1
                if not np.isfinite(zeta) or zeta < F(spm.q_tolerance): break
                Q0 = Q1
            iters.append(done)
            delta = np.concatenate([delta, S.back(delta)])
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

    def first_lm_system(self, **kw):
        """float64: (A, b) of the first LM step -- A = J^T J + diag(CtC), b = -J^T F"""
        Hs, CtC, pre_lm, SSq, r = self.first_step(**kw)
        J = self.linearise()[0]
        A = (J.T @ J) + sp.diags(CtC.astype(np.float64))
        return A, r.astype(np.float64)


# ------------------------------------------------------------------ the kernel tests' two sides: float64 (dense) and float32 in the kernels' order, both from one Jb
class SchurLists:
    """The index lists of BundleAdjustmentPlugin::prepare (csrc/ba_structure.cpp incidence_lists; compared entry by entry in tests/test_ba_structure_host.py) in the caller's point order or -- renumber -- in the plan's (points by first observing camera, a camera's
    observations by internal point id); new2old: the plan's point j is the caller's new2old[j] (identity without renumbering)"""

    def __init__(self, oc, op, C, P, renumber=False):
        oc, op = np.asarray(oc, np.int64), np.asarray(op, np.int64)
        O = len(oc)
        self.C, self.P, self.O = C, P, O
        self.new2old = np.arange(P)
        if renumber:
            first = np.full(P, C); np.minimum.at(first, op, oc)
            self.new2old = np.argsort(first, kind="stable"); old2new = np.empty(P, np.int64); old2new[self.new2old] = np.arange(P)
            op = old2new[op]
        self.cam_ptr = np.concatenate([[0], np.cumsum(np.bincount(oc, minlength=C))]); self.pt_ptr = np.concatenate([[0], np.cumsum(np.bincount(op, minlength=P))])
        self.cam_obs = np.lexsort((np.arange(O), op, oc)) if renumber else np.argsort(oc, kind="stable")
        pos = np.empty(O, np.int64); pos[self.cam_obs] = np.arange(O)
        self.q_cam, self.q_pt = oc[self.cam_obs], op[self.cam_obs]
        self.pt_pos = np.argsort(self.q_pt, kind="stable") if renumber else pos[np.argsort(op, kind="stable")]


def dense_j(Jb, L):
    """[O, 24] blocks in camera order -> dense float64 J [2 O, 9 C + 3 P] over [cameras | points]"""
    J = np.zeros((2 * L.O, 9 * L.C + 3 * L.P))
    q = np.arange(L.O)
    for k in range(9):
        J[2 * q, 9 * L.q_cam + k] = Jb[:, k]; J[2 * q + 1, 9 * L.q_cam + k] = Jb[:, 12 + k]
    for k in range(3):
        J[2 * q, 9 * L.C + 3 * L.q_pt + k] = Jb[:, 9 + k]; J[2 * q + 1, 9 * L.C + 3 * L.q_pt + k] = Jb[:, 21 + k]
    return J


class Schur64:
    """float64, dense: S, g and the back-substitution of A = J^T J + diag(shift) with the held points' rows and columns dropped (a principal submatrix of A)"""

    def __init__(self, J, shift, b, held, C):
        self.nc = nc = 9 * C
        A = J.T @ J
        if shift is not None: A = A + np.diag(np.asarray(shift, np.float64))
        self.A, self.b = A, np.asarray(b, np.float64)
        self.free = np.repeat(~np.asarray(held, bool), 3)                       # point unknowns that are solved for
        ip = nc + np.nonzero(self.free)[0]
        self.B, self.E, Cp = A[:nc, :nc], A[:nc][:, ip], A[ip][:, ip]
        self.CiEt = np.linalg.solve(Cp, self.E.T); self.Cib = np.linalg.solve(Cp, self.b[ip])
        self.S = self.B - self.E @ self.CiEt
        self.g = self.b[:nc] - self.E @ self.Cib

    def apply(self, x):
        return self.S @ np.asarray(x, np.float64)

    def back(self, dc):
        dp = np.zeros(len(self.free))
        dp[self.free] = self.Cib - self.CiEt @ np.asarray(dc, np.float64)
        return dp


class SchurKernels32:
    """float32 in the kernels' order (ba_schur.hip, thallo_hip_ba_block_diag's point half), every product and every addition rounded on its own -- the device differs by its
    fused multiply-adds.  Elementwise numpy only: the same numbers on every machine."""

    def __init__(self, Jb, L, shift, b):
        self.L, self.nc = L, 9 * L.C
        Jb = np.asarray(Jb, F)
        self.a0, self.a1 = Jb[:, 0:9], Jb[:, 12:21]                               # camera rows, camera order
        k2q = L.pt_pos
        self.p0, self.p1 = Jb[k2q, 9:12], Jb[k2q, 21:24]                         # point rows, point order (JP)
        self.cnt = np.diff(L.pt_ptr)
        H = np.zeros((L.P, 3, 3), F)
        for t, m, k in self._trips():
            for i in range(3):
                for j in range(i + 1):
                    H[m, i, j] = (H[m, i, j] + ((self.p0[k, i] * self.p0[k, j]).astype(F) + (self.p1[k, i] * self.p1[k, j]).astype(F)).astype(F)).astype(F)
        H = np.tril(H) + np.transpose(np.tril(H, -1), (0, 2, 1))
        self.shift = None if shift is None else np.asarray(shift, F)
        sh = np.zeros((L.P, 3)) if shift is None else self.shift[self.nc:].reshape(L.P, 3)
        self.G, self.held = elim_factor32(H, sh)
        self.b = np.asarray(b, F)

    def _trips(self):
        for t in range(int(self.cnt.max()) if len(self.cnt) else 0):
            m = np.nonzero(self.cnt > t)[0]
            yield t, m, self.L.pt_ptr[m] + t

    def _apply_g(self, w):
        G = self.G; y = np.zeros_like(w); z = np.zeros_like(w)
        for i in range(3):
            for j in range(i + 1): y[:, i] = (y[:, i] + (G[:, i, j] * w[:, j]).astype(F)).astype(F)
        for j in range(3):
            for i in range(j, 3): z[:, j] = (z[:, j] + (G[:, i, j] * y[:, i]).astype(F)).astype(F)
        return z

    def cam_u(self, x):
        xc = np.asarray(x, F)[:self.nc].reshape(-1, 9)[self.L.q_cam]
        u = np.zeros((self.L.O, 2), F)
        for k in range(9):
            u[:, 0] = (u[:, 0] + (self.a0[:, k] * xc[:, k]).astype(F)).astype(F); u[:, 1] = (u[:, 1] + (self.a1[:, k] * xc[:, k]).astype(F)).astype(F)
        return u

    def pt_w(self, u):
        w = np.zeros((self.L.P, 3), F)
        for t, m, k in self._trips():
            uq = u[self.L.pt_pos[k]]
            for i in range(3):
                w[m, i] = (w[m, i] + ((self.p0[k, i] * uq[:, 0]).astype(F) + (self.p1[k, i] * uq[:, 1]).astype(F)).astype(F)).astype(F)
        return w

    def pt_t(self, y):
        """t_k = J_p,k y per observation in point order -> in camera order"""
        yk = y[np.repeat(np.arange(self.L.P), self.cnt)]
        t = np.zeros((self.L.O, 2), F)
        for row, p in ((0, self.p0), (1, self.p1)):
            t[:, row] = (((p[:, 0] * yk[:, 0]).astype(F) + (p[:, 1] * yk[:, 1]).astype(F)).astype(F) + (p[:, 2] * yk[:, 2]).astype(F)).astype(F)
        out = np.zeros_like(t); out[self.L.pt_pos] = t
        return out

    def cam_gather(self, t):
        """sum_q J_c,q^T t_q: lane l of the camera's wave adds its observations q0 + l, q0 + l + 64, ... in order, then the wave butterfly"""
        C = self.L.C
        out = np.zeros((C, 9), F)
        for c in range(C):
            q0, q1 = self.L.cam_ptr[c], self.L.cam_ptr[c + 1]
            lanes = np.zeros((64, 9), F)
            for r0 in range(q0, q1, 64):
                q = np.arange(r0, min(r0 + 64, q1)); l = q - r0
                lanes[l] = (lanes[l] + ((self.a0[q] * t[q, 0:1]).astype(F) + (self.a1[q] * t[q, 1:2]).astype(F)).astype(F)).astype(F)
            m = 32
            while m >= 1:
                lanes = (lanes[:m] + lanes[m:2 * m]).astype(F); m //= 2
            out[c] = lanes[0]
        return out.ravel()

    def reduce(self):
        self.y = self._apply_g(self.b[self.nc:].reshape(-1, 3))
        return (self.b[:self.nc] - self.cam_gather(self.pt_t(self.y))).astype(F)

    def apply(self, x):
        x = np.asarray(x, F)
        u = self.cam_u(x)
        v = (u - self.pt_t(self._apply_g(self.pt_w(u)))).astype(F)
        s = self.cam_gather(v)
        return s if self.shift is None else (s + (self.shift[:self.nc] * x[:self.nc]).astype(F)).astype(F)

    def back(self, dc):
        w = self.pt_w(self.cam_u(dc))
        return self._apply_g((self.b[self.nc:].reshape(-1, 3) - w).astype(F)).ravel()


def rel_max(a, ref):
    """max |a - ref| / max |ref|"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())
