"""CPU restatement of the ASSEMBLED reduced camera matrix of bundle adjustment's Schur-complement solve (thallo_amd/csrc/ba_schur_explicit.hip, ThalloX_PlanSetLinearSolver
kind 2) -- TEST INFRASTRUCTURE, not a test.  Everything but the application of S is tests/ba_schur_mirror.py's, which this file imports and leaves as it is.

  S_ij = [i = j] (B_ii + diag CtC_c,i) - sum over the terms (q, q') of block (i, j) of W_q W_q'^T,      W_q = (J_c,q^T J_p,q) G_p^T  (9 x 3),  Cp^-1 = G^T G

  SchurStructure          the symbolic structure as ReducedCameraSystem::configure builds it from csrc/ba_structure.cpp's count_terms / list_terms / place_blocks (vectorised;
                          tests/test_ba_structure_host.py compares the two entry by entry), brute_force_counts the same numbers the slow way
  ExplicitSchurSystem     a SchurSystem whose apply multiplies by an S assembled block-wise from float32 W's with float32 accumulation (BaSchurExplicitMirror runs
                          BaSchurMirror's GN and LM loops on it)
  blocks64                float64 block-wise W and S from one Jb (no dense J)
  w32 / cam_blocks32 / assemble32 / apply32     float32 in the kernels' summation order, every product and every addition rounded on its own, elementwise numpy: the e32 side"""
import numpy as np
import scipy.sparse as sp

import ba_schur_mirror as bsm
from ba_schur_mirror import BaSchurMirror, SchurLists, SchurSystem

F = np.float32


class SchurStructure:
    """From the point incidence lists (pt_ptr / pt_pos over observations in camera order, q_cam their cameras): the stored blocks -- both triangles, a row's blocks
    consecutive with ascending columns (row_ptr, col), every diagonal block present -- and for every lower-triangle block l, in the order (row, column): lower[l] = (place
    of the block, place of its transpose, camera of a diagonal block or -1) and its terms (q, q') at terms[term_ptr[l] : term_ptr[l + 1]], ascending in (q, q').  A (camera,
    point) pair observed twice gives its diagonal block both orders of the pair."""

    def __init__(self, L):
        C, P = L.C, L.P
        pt_ptr, pt_pos, q_cam = np.asarray(L.pt_ptr, np.int64), np.asarray(L.pt_pos, np.int64), np.asarray(L.q_cam, np.int64)
        cnt = np.diff(pt_ptr)
        qs, q2s = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
        for n in np.unique(cnt):
            if n == 0: continue
            q = pt_pos[pt_ptr[:-1][cnt == n][:, None] + np.arange(n)[None, :]]                    # [points with n observations, n]
            a, b = np.broadcast_to(q[:, :, None], (len(q), n, n)).ravel(), np.broadcast_to(q[:, None, :], (len(q), n, n)).ravel()
            keep = q_cam[a] >= q_cam[b]
            qs.append(a[keep]); q2s.append(b[keep])
        q, q2 = np.concatenate(qs), np.concatenate(q2s)
        key = q_cam[q] * C + q_cam[q2]
        order = np.lexsort((q2, q, key))
        q, q2, key = q[order], q2[order], key[order]
        keys = np.union1d(key, np.arange(C) * (C + 1))                                               # every diagonal block is present
        self.C, self.nlower, self.nterms = C, len(keys), len(q)
        self.terms = np.stack([q, q2], 1)
        self.term_ptr = np.searchsorted(key, np.concatenate([keys, [C * C]]))
        self.row, self.colj = keys // C, keys % C                                                   # the lower blocks' cameras (i, j), j <= i
        diag = self.row == self.colj
        per_row = np.bincount(self.row, minlength=C) + np.bincount(self.colj[~diag], minlength=C)
        self.row_ptr = np.concatenate([[0], np.cumsum(per_row)])
        self.nblk = int(self.row_ptr[-1])
        fill = self.row_ptr[:-1].copy()
        self.col = np.zeros(self.nblk, np.int64); self.lower = np.zeros((self.nlower, 3), np.int64)
        for l, (i, j) in enumerate(zip(self.row, self.colj)):      # the keys ascend by (row, column): a row's lower part and diagonal are placed before its first (k, row), k > row
            bij = fill[i]; fill[i] += 1; self.col[bij] = j
            bji = bij
            if i != j: bji = fill[j]; fill[j] += 1; self.col[bji] = i
            self.lower[l] = (bij, bji, i if i == j else -1)
        self.block_row = np.repeat(np.arange(C), per_row)

    def bytes(self, O):
        """what the plugin asks the budget for"""
        return 81 * 4 * self.nblk + 64 + (128 * O + 64) + 8 * self.nterms + 16 + 4 * (self.C + 5) + 4 * (self.nblk + 4) + 4 * (3 * self.nlower + 4) + 4 * (self.nlower + 5)

    def scatter(self, low):
        """[nlower, 9, 9] lower blocks -> [nblk, 9, 9] stored blocks, the transposes filled in"""
        S = np.zeros((self.nblk, 9, 9), low.dtype)
        S[self.lower[:, 1]] = np.transpose(low, (0, 2, 1))
        S[self.lower[:, 0]] = low
        return S

    def bsr(self, S):
        return sp.bsr_matrix((np.asarray(S, np.float64), self.col, self.row_ptr), shape=(9 * self.C, 9 * self.C))


def brute_force_counts(oc, op, C):
    """-> (lower blocks, lower terms, stored blocks, blocks per row) from the observations themselves: every ordered pair of observations of one point whose first camera is
    not below the second is a term of block (first camera, second camera); every diagonal block exists"""
    oc, op = np.asarray(oc), np.asarray(op)
    blocks = {(c, c) for c in range(C)}
    terms = 0
    for o in range(len(oc)):
        for o2 in np.nonzero(op == op[o])[0]:
            if oc[o] >= oc[o2]:
                terms += 1; blocks.add((int(oc[o]), int(oc[o2])))
    per_row = np.zeros(C, np.int64)
    for i, j in blocks:
        per_row[i] += 1
        if i != j: per_row[j] += 1
    return len(blocks), terms, int(per_row.sum()), per_row


def hand_made():
    """4 cameras, 5 points, 12 observations: (camera 1, point 2) is observed twice, (camera 3, point 0) three times; camera 2 sees one point only; point 4 is seen once"""
    oc = np.array([0, 1, 1, 3, 3, 3, 0, 2, 1, 0, 3, 1], np.int32)
    op = np.array([0, 2, 2, 0, 0, 0, 1, 1, 1, 3, 3, 4], np.int32)
    return oc, op, 4, 5


def jb_of(J, C):
    """the oracle's J (CSR, rows 2 o and 2 o + 1 of observation o, nine camera columns then three point columns) -> (Jb [O, 24] float64 in the caller's observation order,
    cameras, points of the observations)"""
    J = sp.csr_matrix(J); J.sort_indices()
    assert (np.diff(J.indptr) == 12).all()
    rows, cols = J.data.reshape(-1, 12), J.indices.reshape(-1, 12)
    assert (cols[0::2] == cols[1::2]).all()
    return np.concatenate([rows[0::2], rows[1::2]], 1), cols[0::2, 0] // 9, (cols[0::2, 9] - 9 * C) // 3


# ------------------------------------------------------------------ float32 in the kernels' order
def w32(Jb, q_pt, G):
    """k_schur_w: E = a0 p0^T + a1 p1^T, W[a, m] = sum over n <= m of E[a, n] G[m, n] from 0 upwards; Jb [O, 24] in camera order, G [P, 3, 3] float32 -> [O, 9, 3]"""
    Jb = np.asarray(Jb, F); g = np.asarray(G, F)[q_pt]
    a0, a1, p0, p1 = Jb[:, 0:9], Jb[:, 12:21], Jb[:, 9:12], Jb[:, 21:24]
    E = ((a0[:, :, None] * p0[:, None, :]).astype(F) + (a1[:, :, None] * p1[:, None, :]).astype(F)).astype(F)
    W = np.zeros((len(Jb), 9, 3), F)
    for m in range(3):
        for n in range(m + 1): W[:, :, m] = (W[:, :, m] + (E[:, :, n] * g[:, m, n][:, None]).astype(F)).astype(F)
    return W


def cam_blocks32(Jb, L):
    """thallo_hip_ba_block_diag's camera half: lane l of a camera's wave adds the observations q0 + l, q0 + l + 64, ..., then the wave butterfly -> [C, 9, 9] float32, symmetric"""
    Jb = np.asarray(Jb, F)
    a0, a1 = Jb[:, 0:9], Jb[:, 12:21]
    H = np.zeros((L.C, 9, 9), F)
    for c in range(L.C):
        q0, q1 = L.cam_ptr[c], L.cam_ptr[c + 1]
        lanes = np.zeros((64, 9, 9), F)
        for r0 in range(q0, q1, 64):
            q = np.arange(r0, min(r0 + 64, q1)); l = q - r0
            lanes[l] = (lanes[l] + ((a0[q][:, :, None] * a0[q][:, None, :]).astype(F) + (a1[q][:, :, None] * a1[q][:, None, :]).astype(F)).astype(F)).astype(F)
        m = 32
        while m >= 1:
            lanes = (lanes[:m] + lanes[m:2 * m]).astype(F); m //= 2
        H[c] = lanes[0]
    return H


def assemble32(st, W, B, ctc):
    """k_schur_assemble: per lower block the terms in the list's order, acc += (x0 y0 + x1 y1) + x2 y2; a diagonal block's entry (a, b) is the sum of (max, min); then
    (B_ii + CtC) - acc.  W [O, 9, 3], B [C, 9, 9] float32, ctc flat (9 C) or None -> the stored blocks [nblk, 9, 9] float32"""
    W = np.asarray(W, F)
    acc = np.zeros((st.nlower, 9, 9), F)
    cnt = np.diff(st.term_ptr)
    for t in range(int(cnt.max()) if len(cnt) else 0):
        m = np.nonzero(cnt > t)[0]
        x, y = W[st.terms[st.term_ptr[m] + t, 0]], W[st.terms[st.term_ptr[m] + t, 1]]
        s = ((x[:, :, None, 0] * y[:, None, :, 0]).astype(F) + (x[:, :, None, 1] * y[:, None, :, 1]).astype(F)).astype(F)
        s = (s + (x[:, :, None, 2] * y[:, None, :, 2]).astype(F)).astype(F)
        acc[m] = (acc[m] + s).astype(F)
    d = st.lower[:, 2] >= 0
    acc[d] = np.tril(acc[d]) + np.transpose(np.tril(acc[d], -1), (0, 2, 1))
    base = np.zeros_like(acc)
    Bd = np.asarray(B, F)[st.lower[d, 2]].copy()
    if ctc is not None:
        i9 = np.arange(9)
        Bd[:, i9, i9] = (Bd[:, i9, i9] + np.asarray(ctc, F)[:9 * st.C].reshape(-1, 9)[st.lower[d, 2]]).astype(F)
    base[d] = Bd
    return st.scatter((base - acc).astype(F))


def apply32(st, S, x):
    """k_schur_apply_s: lane l of a row's wave takes the blocks l, l + 64, ... of the row, y[a] += S[a, b] x[b] with b ascending, then the wave butterfly"""
    x = np.asarray(x, F)[:9 * st.C].reshape(-1, 9)
    out = np.zeros((st.C, 9), F)
    for c in range(st.C):
        t0, t1 = st.row_ptr[c], st.row_ptr[c + 1]
        lanes = np.zeros((64, 9), F)
        for r0 in range(t0, t1, 64):
            t = np.arange(r0, min(r0 + 64, t1)); l = t - r0
            xv = x[st.col[t]]
            for b in range(9): lanes[l] = (lanes[l] + (S[t, :, b] * xv[:, b:b + 1]).astype(F)).astype(F)
        m = 32
        while m >= 1:
            lanes = (lanes[:m] + lanes[m:2 * m]).astype(F); m //= 2
        out[c] = lanes[0]
    return out.ravel()


# ------------------------------------------------------------------ float64, block-wise
def blocks64(Jb, L, st, shift, held, chunk=1 << 18):
    """float64 from one Jb ([O, 24] in camera order): W_q = (J_c^T J_p) G^T with G = chol(Cp)^-1 of the point's exact block (+ shift; a held point: G = 0, its rows and
    columns dropped) and the stored blocks of S = B (+ diag shift_c) - sum of W_q W_q'^T -> (W [O, 9, 3], S [nblk, 9, 9])"""
    Jb = np.asarray(Jb, np.float64)
    a0, a1, p0, p1 = Jb[:, 0:9], Jb[:, 12:21], Jb[:, 9:12], Jb[:, 21:24]
    Cp = np.zeros((L.P, 3, 3))
    np.add.at(Cp, L.q_pt, p0[:, :, None] * p0[:, None, :] + p1[:, :, None] * p1[:, None, :])
    if shift is not None: Cp[:, np.arange(3), np.arange(3)] += np.asarray(shift, np.float64)[9 * L.C:].reshape(-1, 3)
    free = ~np.asarray(held, bool)
    G = np.zeros((L.P, 3, 3))
    G[free] = np.linalg.inv(np.linalg.cholesky(Cp[free]))
    E = a0[:, :, None] * p0[:, None, :] + a1[:, :, None] * p1[:, None, :]
    W = np.einsum("qan,qmn->qam", E, G[L.q_pt])
    B = np.zeros((L.C, 9, 9))
    np.add.at(B, L.q_cam, a0[:, :, None] * a0[:, None, :] + a1[:, :, None] * a1[:, None, :])
    if shift is not None: B[:, np.arange(9), np.arange(9)] += np.asarray(shift, np.float64)[:9 * L.C].reshape(-1, 9)
    low = np.zeros((st.nlower, 9, 9))
    blk = np.repeat(np.arange(st.nlower), np.diff(st.term_ptr))
    for s in range(0, st.nterms, chunk):
        e = slice(s, s + chunk)
        np.add.at(low, blk[e], np.einsum("tam,tbm->tab", W[st.terms[e, 0]], W[st.terms[e, 1]]))
    low = -low
    d = st.lower[:, 2] >= 0
    low[d] += B[st.lower[d, 2]]
    return W, st.scatter(low)


# ------------------------------------------------------------------ the solve
class ExplicitSchurSystem(SchurSystem):
    """SchurSystem with S assembled: float32 W's from the float32 Jb and the mirror's own float32 elimination factor, float32 accumulation in the kernels' order, B_ii the
    float32 rounding of the exact block; apply = the stored float32 S times x in float64, rounded once (SchurSystem's convention for a vector operation).  CtC is in S."""

    def __init__(self, J, Hs, shift, pre, b, C):
        super().__init__(J, Hs, shift, pre, b, C)
        Jb, oc, op = jb_of(J, C)
        self.lists = L = SchurLists(oc, op, C, Hs[1].shape[0])
        self.st = st = SchurStructure(L)
        self.W = w32(Jb[L.cam_obs], L.q_pt, self.G)
        self.S = assemble32(st, self.W, Hs[0].astype(F), self.ctc_c)
        self.Sm = st.bsr(self.S)

    def apply(self, x):
        return (self.Sm @ x.astype(np.float64)).astype(F)


class BaSchurExplicitMirror(BaSchurMirror):
    """BaSchurMirror's GN and LM loops with every S x through the assembled S: the loops build their system by the module's name SchurSystem, which is swapped for the
    length of a solve"""

    def _assembled(self, f, *a, **kw):
        saved = bsm.SchurSystem
        bsm.SchurSystem = ExplicitSchurSystem
        try: return f(*a, **kw)
        finally: bsm.SchurSystem = saved

    def gn_step(self, L, kind="schur"):
        return self._assembled(super().gn_step, L, kind)

    def lm_solve(self, nit, lit, kind="schur", **kw):
        return self._assembled(super().lm_solve, nit, lit, kind, **kw)
