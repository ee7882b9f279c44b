"""CPU restatement of the Gauss-Newton and Levenberg-Marquardt loops of bundle adjustment with BOTH preconditioners -- TEST INFRASTRUCTURE, not a test
(oracle CSR for J + scipy, float32 state, float64 sums: the shape of tests/ba_scipy_backend.py::BaShardMirror on one rank).

  "jacobi"   the reference's point Jacobi: guardedInvert(diag J^T J) in GN, 1 / (CtC + diag) in LM;
  "block64"  block Jacobi with the blocks inverted in float64: z = (H + diag(shift))^-1 r per 9 x 9 camera / 3 x 3 point block;
  "block32"  the device algorithm (thallo_amd/csrc/block_precond.hip) restated in float32: s = 1 / sqrt(diag B), Cholesky of S B S, G = L^-1 S, z = G^T (G r).

Everything per block is stacked over [blocks, n, n] (np.linalg.inv / eigvalsh / einsum for float64; the float32 restatement spells the kernel's own loops over the <= 9
rows and columns of a block, each step on all blocks at once): no Python loop over points.  The loops are the plan's block schedule: GN =
PCGInit1, blocks, then per iteration PCGStep3 (+ delta) / PCGStep1 / PCGStep2; LM = the reference-shaped loop of gauss_newton.t:1545-1785 with every UsesLambda()
branch taken, SSq and CtC exactly the reference's, the factorisation redone every step with shift = CtC."""
import numpy as np
import scipy.sparse as sp

from oracle import oracle as orc

F = np.float32


def guarded_invert(d):
    return (F(1) / (F(1) + np.sqrt(d.astype(F))) ** 2).astype(F)


def stacked_blocks(JtJ, C, P):
    """The diagonal blocks of a sparse symmetric matrix over [cameras 9 c + k | points 9 C + 3 p + k]: ([C, 9, 9], [P, 3, 3]) float64."""
    M = sp.coo_matrix(JtJ); M.sum_duplicates()
    nc = 9 * C
    Hc, Hp = np.zeros((C, 9, 9)), np.zeros((P, 3, 3))
    r, c, v = M.row, M.col, M.data
    cam = (r < nc) & (c < nc) & (r // 9 == c // 9)
    Hc[r[cam] // 9, r[cam] % 9, c[cam] % 9] = v[cam]
    pt = (r >= nc) & (c >= nc) & ((r - nc) // 3 == (c - nc) // 3)
    Hp[(r[pt] - nc) // 3, (r[pt] - nc) % 3, (c[pt] - nc) % 3] = v[pt]
    return Hc, Hp


def scaled_error(z, z64, Hs, shift, C):
    """Largest deviation of z from z64, per block, in the coordinates the factorisation works in: u = z / s, s = 1 / sqrt(diag B) (the solution of the
    well-conditioned system S B S u = S r): max over blocks of max_i |u_i - u64_i| / max_i |u64_i|.  Blocks whose float64 solution is zero are skipped."""
    nc = 9 * C
    d = np.concatenate([np.einsum("bii->bi", Hs[0]).ravel(), np.einsum("bii->bi", Hs[1]).ravel()]) + (0.0 if shift is None else np.asarray(shift, np.float64))
    ok = d > 0
    s = np.where(ok, 1.0 / np.sqrt(np.where(ok, d, 1.0)), 1.0)
    e = np.abs(np.asarray(z, np.float64) - z64) / s; u = np.abs(z64) / s
    worst = 0.0
    for lo, hi, n in ((0, nc, 9), (nc, len(z64), 3)):
        eb, ub = e[lo:hi].reshape(-1, n).max(1), u[lo:hi].reshape(-1, n).max(1)
        m = ub > 0
        if m.any(): worst = max(worst, float((eb[m] / ub[m]).max()))
    return worst


class BlockPrecond:
    """M^-1 of one GN / LM step.  Hs = (Hc, Hp) float64 blocks; shift: the LM CtC (flat, float32) or None; pre: the point-Jacobi M^-1 (flat): the fallback."""

    def __init__(self, kind, Hs, shift, pre, C):
        assert kind in ("block64", "block32")
        self.kind, self.C, self.pre, self.fallbacks = kind, C, np.asarray(pre, F), 0
        nc = 9 * C
        self.parts = []
        for H, lo, n in ((Hs[0], 0, 9), (Hs[1], nc, 3)):
            nb = H.shape[0]
            sh = np.zeros((nb, n)) if shift is None else np.asarray(shift[lo:lo + n * nb], np.float64).reshape(nb, n)
            pr = self.pre[lo:lo + n * nb].reshape(nb, n)
            self.parts.append(self._factor(H, sh, pr, n) + (lo, n, nb))

    def _factor(self, H, sh, pr, n):
        idx = np.arange(n)
        if self.kind == "block64":
            B = H.copy(); B[:, idx, idx] += sh
            d = B[:, idx, idx]
            bad = ~((d > 0) & np.isfinite(d)).all(1)
            B[bad] = np.eye(n)
            with np.errstate(all="ignore"):
                ev = np.linalg.eigvalsh(B)
            bad |= ~(ev[:, 0] > 0)
            B[bad] = np.eye(n)
            Minv = np.linalg.inv(B)
            for b in np.nonzero(bad)[0]: Minv[b] = np.diag(pr[b].astype(np.float64))
            self.fallbacks += int(bad.sum())
            return (Minv, None)
        # float32, the device's steps in the device's order (block_precond.hip factor<N>), every operation rounded to float32 on its own, vectorised over the blocks:
        # elementwise numpy only, so e32 is the same number on every machine (no LAPACK kernel choice in it); the device differs by its fused multiply-adds
        nb = H.shape[0]
        a = H.astype(F); a[:, idx, idx] = (a[:, idx, idx] + sh.astype(F)).astype(F)
        d = a[:, idx, idx]
        ok = ((d > 0) & np.isfinite(d)).all(1)
        inv = np.zeros((nb, n), F)
        with np.errstate(all="ignore"):
            s = (F(1) / np.sqrt(d)).astype(F)
            a = ((a * s[:, :, None]).astype(F) * s[:, None, :]).astype(F)
            for j in range(n):                                      # Cholesky of S B S, column by column
                dd = a[:, j, j].copy()
                for k in range(j): dd = (dd - (a[:, j, k] * a[:, j, k]).astype(F)).astype(F)
                ok &= (dd > 0) & np.isfinite(dd)
                inv[:, j] = (F(1) / np.sqrt(dd)).astype(F)
                for i in range(j + 1, n):
                    v = a[:, i, j].copy()
                    for k in range(j): v = (v - (a[:, i, k] * a[:, j, k]).astype(F)).astype(F)
                    a[:, i, j] = (v * inv[:, j]).astype(F)
            for i in range(n):                                      # L^-1, row by row
                li = a[:, i, :].copy()
                for j in range(i):
                    v = (li[:, j] * inv[:, j]).astype(F)
                    for k in range(j + 1, i): v = (v + (li[:, k] * a[:, k, j]).astype(F)).astype(F)
                    a[:, i, j] = (-inv[:, i] * v).astype(F)
                a[:, i, i] = inv[:, i]
            G = (np.tril(a) * s[:, None, :]).astype(F)
        ok &= np.isfinite(G).all((1, 2))
        for b in np.nonzero(~ok)[0]: G[b] = np.diag(np.sqrt(pr[b]).astype(F))
        self.fallbacks += int((~ok).sum())
        return (None, G)

    def __call__(self, r, exact=False):
        """z = M^-1 r in float32; exact (block64 only): the float64 solve itself, not its float32 rounding"""
        z = np.empty(len(r), np.float64 if exact else F)
        for Minv, G, lo, n, nb in self.parts:
            rb = r[lo:lo + n * nb].reshape(nb, n)
            if G is None: zb = np.einsum("bij,bj->bi", Minv, rb.astype(np.float64))
            else:                                                   # y = G r, z = G^T y: one rounded product and one rounded addition per term, in index order
                rb = rb.astype(F); y = np.zeros((nb, n), F); zb = np.zeros((nb, n), F)
                for i in range(n):
                    for j in range(i + 1): y[:, i] = (y[:, i] + (G[:, i, j] * rb[:, j]).astype(F)).astype(F)
                for j in range(n):
                    for i in range(j, n): zb[:, j] = (zb[:, j] + (G[:, i, j] * y[:, i]).astype(F)).astype(F)
            z[lo:lo + n * nb] = zb.ravel()
        return z


class BaBlockMirror:
    def __init__(self, dims, params):
        self.dims = tuple(int(x) for x in dims)
        self.params = [a.copy() for a in params]
        self.C, self.P, self.O = self.dims
        self.nc, self.n = 9 * self.C, 9 * self.C + 3 * self.P
        self.fallbacks = 0

    def _problem(self):
        return orc.Problem(orc.BUNDLE_ADJUST, self.dims, self.params)

    def cost(self):
        return F(self._problem().cost())

    def linearise(self):
        """J (float64 CSR), r = -J^T F and the raw diagonal of J^T J (float32), the blocks of J^T J (float64, stacked)"""
        rp, col, val, res = self._problem().csr()
        J = sp.csr_matrix((val.astype(np.float64), col, rp), shape=(len(res), self.n))
        r = (-(J.T @ res.astype(np.float64))).astype(F)
        JtJ = (J.T @ J)
        d = JtJ.diagonal().astype(F)
        return J, r, d, stacked_blocks(JtJ, self.C, self.P)

    def _precond(self, kind, Hs, shift, pre):
        if kind == "jacobi":
            return lambda r: (pre * r).astype(F)
        M = BlockPrecond(kind, Hs, shift, pre, self.C)
        self.fallbacks += M.fallbacks
        return M

    @staticmethod
    def _dot(a, b):
        return F(float(a.astype(np.float64) @ b.astype(np.float64)))

    def _update(self, delta):
        self.params[0].reshape(-1)[:] += delta[:self.nc]
        self.params[1].reshape(-1)[:] += delta[self.nc:]

    # ---- Gauss-Newton: PCGInit1; per iteration PCGStep3 (+ the delta update of the iteration before), PCGStep1, PCGStep2; PCGLinearUpdate
    def gn_step(self, L, kind):
        J, r, d, Hs = self.linearise()
        pre = guarded_invert(d)
        M = self._precond(kind, Hs, None, pre)
        z = M(r)
        aN = self._dot(r, z)
        p = np.zeros(self.n, F); delta = np.zeros(self.n, F)
        alpha = beta = F(0)
        for k in range(L):
            if k: delta = (delta + alpha * p).astype(F)
            p = (z + beta * p).astype(F) if k else z.copy()
            Ap = (J.T @ (J @ p.astype(np.float64))).astype(F)
            aD = self._dot(p, Ap)
            alpha = F(aN / aD) if aD != 0 else F(0)
            r = (r - alpha * Ap).astype(F)
            z = M(r)
            bN = self._dot(z, r)
            beta = F(bN / aN) if aN != 0 else F(0)
            aN = bN
        if L: delta = (delta + alpha * p).astype(F)
        self._update(delta)

    def gn_solve(self, nit, lit, kind="jacobi"):
        costs = [float(self.cost())]
        for _ in range(nit):
            self.gn_step(lit, kind)
            costs.append(float(self.cost()))
        return costs

    # ---- Levenberg-Marquardt (tests/ba_scipy_backend.py::BaShardMirror.lm_solve on one rank, with the preconditioner a parameter)
    def lm_solve(self, nit, lit, kind="jacobi", **kw):
        """-> (costs, PCG iterations per LM step)"""
        spm = orc.default_params(**kw)
        radius, dec = F(spm.trust_region_radius), F(spm.radius_decrease_factor)
        prev = self.cost(); costs = [float(prev)]; iters = []
        SSq = None
        for it in range(nit):
            J, r, d, Hs = self.linearise()
            if it == 0: SSq = guarded_invert(d)                                     # PCGSaveSSq
            unclamped = (d * (F(1) / radius)).astype(F)
            cm = ((F(1) / SSq) / radius).astype(F)
            CtC = np.minimum(np.maximum(unclamped, F(spm.min_lm_diagonal) * cm), F(spm.max_lm_diagonal) * cm).astype(F)
            pre = (F(1) / (CtC + radius * unclamped)).astype(F)
            M = self._precond(kind, Hs, CtC, pre)
            b = r.copy(); z = M(r)
            aN = self._dot(r, z)
            p = np.zeros(self.n, F); delta = np.zeros(self.n, F)
            Q0 = F(0); beta = F(0); done = 0
            for k in range(lit):
                p = (z + beta * p).astype(F) if k else z.copy()
                Ap = ((J.T @ (J @ p.astype(np.float64))).astype(F) + CtC * p).astype(F)
                aD = self._dot(p, Ap)
                with np.errstate(all="ignore"):
                    alpha = F(aN / aD)
                delta = (delta + alpha * p).astype(F)
                if (k + 1) % spm.residual_reset_period == 0:                        # :1653-1657
                    Ad = ((J.T @ (J @ delta.astype(np.float64))).astype(F) + delta * CtC).astype(F)
                    r = (b - Ad).astype(F)
                else:
                    r = (r - alpha * Ap).astype(F)
                z = M(r)
                bN = self._dot(z, r)
                Q1 = F(0.5 * float(delta.astype(np.float64) @ (r + b).astype(F).astype(np.float64)))
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

    # ---- the first LM step's set-up, for the kernel tests: (Hs, CtC, pre_lm, pre_gn, r)
    def first_step(self, **kw):
        spm = orc.default_params(**kw)
        J, r, d, Hs = self.linearise()
        radius = F(spm.trust_region_radius)
        SSq = guarded_invert(d)
        unclamped = (d * (F(1) / radius)).astype(F)
        cm = ((F(1) / SSq) / radius).astype(F)
        CtC = np.minimum(np.maximum(unclamped, F(spm.min_lm_diagonal) * cm), F(spm.max_lm_diagonal) * cm).astype(F)
        return Hs, CtC, (F(1) / (CtC + radius * unclamped)).astype(F), SSq, r


def e32_of(Hs, shift, pre, r, C):
    """(e32, z64): the float32 restatement's deviation from the float64 solve (scaled_error), and that solve"""
    z64 = BlockPrecond("block64", Hs, shift, pre, C)(r, exact=True)
    z32 = BlockPrecond("block32", Hs, shift, pre, C)(r)
    return scaled_error(z32, z64, Hs, shift, C), z64
