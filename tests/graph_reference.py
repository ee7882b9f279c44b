"""Float64 references, incidence lists, graphs and inputs for the per-kernel tests of csrc/energy_graph.hip (test_graph_reference.py on the CPU,
test_gpu_graph_kernels.py on the device).

Written from thallo_amd/energies/arap_mesh_deformation.t, laplacian_graph.t and the "graph-edge domains" comment of include/thallo_hip.h:
  * ARAP: fit_n = [C_n.x >= -999999.9] w_fit (P_n - C_n); reg_e = w_reg ((P_a - P_b) - R(A_a) (O_a - O_b)), a = V0[e], b = V1[e], R = Rz(gamma) Ry(beta) Rx(alpha);
    unknowns in the flat layout [Position 3n+c | Angle 3N+3n+c]; rows [fit 3n+c | reg 3N+3e+c];
  * graph Laplacian: fit_n = w_fit (X_n - A_n), reg_e = X_a - X_b, w_fit = 0.5, identity preconditioner.
Everything is numpy float64 computed FROM the float32 inputs.  The rotation and its three angle derivatives are products of the three axis matrices (and of the
derivative of one of them), not the expanded entries the kernels spell out, so a wrong sign in one expanded entry cannot be shared.
Beside every output stands the float64 sum of the absolute values of the terms it is made of -- the scale `S` of its error bound sk.tol(k, S).

No function here needs a device."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import shim_kernels as sk
from shim_kernels import F32

BLOCK = 256
MAX_PARTIALS = 1024
UNCONSTRAINED_BELOW = F32(-999999.9)      # arap_mesh_deformation.t: Constraints.x < -999999.9 marks an unconstrained vertex (compared in float32)
LAP_W_FIT = 0.5                           # laplacian_graph.t


def vgrid(n):
    """workgroups of a one-thread-per-vertex launch over n vertices (energy_graph.hip): one per 256, at most 1024, at least 1"""
    return int(max(1, min((n + BLOCK - 1) // BLOCK, MAX_PARTIALS)))


def block_of_vertex(n0, n1):
    """workgroup of every vertex of [n0, n1): vertex n0 + i belongs to workgroup (i // 256) % grid of the grid-stride loop"""
    return (np.arange(n1 - n0) // BLOCK) % vgrid(n1 - n0)


def visits(n0, n1):
    """vertices one lane visits at most"""
    return -(-(n1 - n0) // (BLOCK * vgrid(n1 - n0)))


# ------------------------------------------------------------------ incidence lists
def build_lists(N, v0, v1, out_slots=0, in_slots=0):
    """The incidence lists of thallo_hip.h from (N, v0, v1).  out_slots == 0: CSR (ell_stride 0; in_slots ignored).  out_slots > 0: ELL with that many out-slots and
    in_slots in-slots per vertex -- the j-th out-edge of vertex n at position j*N + n of out_v1, its j-th incoming edge at j*N + n of in_edge / in_src.
    The order within a vertex is the input order (stable).  in_edge holds the edge's position in out_v1 of the same layout.
    ELL padding slots hold an in-range index no list has in that place: a kernel that reads one computes a visibly wrong value and cannot fault.
    Returns a namespace: out_ptr, out_v1, in_ptr, in_edge, in_src (int32), ell_stride, out_slots, in_slots, pos[e] (position of input edge e in the out layout),
    ipos[e] (its position in the in layout), edges (positions the per-edge arrays F / G have: E or ell_stride), pad (bool over `edges`: a padding position)."""
    v0 = np.asarray(v0, np.int64); v1 = np.asarray(v1, np.int64)
    E = len(v0)
    assert ((v0 >= 0) & (v0 < N) & (v1 >= 0) & (v1 < N)).all()
    odeg = np.bincount(v0, minlength=N); ideg = np.bincount(v1, minlength=N)
    out_ptr = np.concatenate([[0], np.cumsum(odeg)]); in_ptr = np.concatenate([[0], np.cumsum(ideg)])
    oorder = np.argsort(v0, kind="stable"); iorder = np.argsort(v1, kind="stable")
    oj = np.empty(E, np.int64); oj[oorder] = np.arange(E) - out_ptr[v0[oorder]]          # edge e is the oj[e]-th out-edge of v0[e]
    ij = np.empty(E, np.int64); ij[iorder] = np.arange(E) - in_ptr[v1[iorder]]
    if out_slots == 0:
        pos = out_ptr[v0] + oj; ipos = in_ptr[v1] + ij
        out_v1 = np.zeros(E, np.int64); in_edge = np.zeros(E, np.int64); in_src = np.zeros(E, np.int64)
        stride, edges = 0, E
        pad = np.zeros(E, bool)
    else:
        assert E > 0 and odeg.max() <= out_slots and ideg.max() <= in_slots
        pos = oj * N + v0; ipos = ij * N + v1
        stride = edges = out_slots * N
        n_of = np.arange(N)
        out_v1 = np.tile((7 * n_of + 3) % N, out_slots)                                    # padding: some vertex, in range
        in_src = np.tile((5 * n_of + 2) % N, in_slots)
        in_edge = pos[(11 * np.arange(in_slots * N) + 1) % E]                              # padding: the position of some real edge, in range
        pad = np.ones(edges, bool); pad[pos] = False
    out_v1[pos] = v1
    in_edge[ipos] = pos; in_src[ipos] = v0
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    return SimpleNamespace(N=N, E=E, out_ptr=i32(out_ptr), out_v1=i32(out_v1), in_ptr=i32(in_ptr), in_edge=i32(in_edge), in_src=i32(in_src), ell_stride=int(stride),
                           out_slots=int(out_slots), in_slots=int(in_slots), pos=pos, ipos=ipos, edges=int(edges), pad=pad, odeg=odeg, ideg=ideg)


def ell_slots(N, v0, v1):
    """(max out-degree, max in-degree), at least 1 each: the slot counts plugins.cpp gives the ELL layout"""
    return max(1, int(np.bincount(v0, minlength=N).max())), max(1, int(np.bincount(v1, minlength=N).max()))


def edge_plane(L, arr, w):
    """a device per-edge array of w floats per position (F: 3, G: 9) as [input edge, component] -- F[e, c]; G[e, 3 * col + row] -- from either layout"""
    arr = np.asarray(arr)[:w * L.edges]
    return arr.reshape(w, L.edges)[:, L.pos].T if L.ell_stride else arr.reshape(L.edges, w)[L.pos]


def padding_words(L, arr, w):
    """the words of a per-edge array (w floats per position) that belong to ELL padding positions"""
    arr = np.asarray(arr)[:w * L.edges]
    return arr.reshape(w, L.edges)[:, L.pad] if L.ell_stride else arr[:0]


# ------------------------------------------------------------------ graphs: (N, v0, v1)
def _i32(*xs):
    return [np.ascontiguousarray(x, np.int32) for x in xs]


def graph_mesh():
    """the torus 12 x 8: 96 vertices, both half-edges, degree 6"""
    from thallo_amd import synthetic as syn
    p = syn.arap_mesh(12, 8)
    N = p[2].shape[0]
    assert N == 96 and (np.bincount(p[6], minlength=N) == 6).all()
    return (N, *_i32(p[6], p[7]))


def _chord_mesh(nu, nv, chords, seed=9):
    """the torus nu x nv with `chords` rounds of extra undirected edges (v, v + 2 along u / along v, alternating) from random vertices"""
    from thallo_amd import synthetic as syn
    p = syn.arap_mesh(nu, nv, n_handles=8)
    N = p[2].shape[0]
    rng = np.random.default_rng(seed)
    v0, v1 = [p[6]], [p[7]]
    idx = np.arange(N); iu, iv = idx % nu, idx // nu
    for c in range(chords):
        pick = rng.random(N) < 0.3
        tgt = (iv * nu + (iu + 2) % nu) if c % 2 == 0 else (((iv + 2) % nv) * nu + iu)
        v0 += [idx[pick], tgt[pick]]; v1 += [tgt[pick], idx[pick]]
    return (N, *_i32(np.concatenate(v0), np.concatenate(v1)))


def graph_deg8():
    """16 x 12 with one round of chords: out-degree 6 .. 8, the <8> instantiations"""
    N, v0, v1 = _chord_mesh(16, 12, 1)
    d = np.bincount(v0, minlength=N)
    assert N == 192 and 6 < d.max() <= 8
    return N, v0, v1


def graph_deg10():
    """... two rounds: out-degree up to 10, the loop form; the recomputing form must refuse it"""
    N, v0, v1 = _chord_mesh(16, 12, 2)
    d = np.bincount(v0, minlength=N)
    assert 8 < d.max() <= 10
    return N, v0, v1


def graph_hub():
    """N = 300, directed: n -> n+1, n+7, n+13 (mod N), except that the third edge of vertices 1 .. 7 goes to vertex 0.  Out-degree 3 everywhere, E = 900, in-degree 10 at
    vertex 0 (its own three sources 299, 293, 287 and the seven redirected ones), and maxin N <= 3 E + N: plugins.cpp keeps the ELL layout, 3 out-slots, 10 in-slots."""
    N = 300
    n = np.arange(N)
    third = (n + 13) % N
    third[1:8] = 0
    v0 = np.stack([n, n, n], 1).ravel(); v1 = np.stack([(n + 1) % N, (n + 7) % N, third], 1).ravel()
    odeg, ideg = np.bincount(v0, minlength=N), np.bincount(v1, minlength=N)
    assert len(v0) == 900 and (odeg == 3).all() and ideg[0] == 10 and ideg.max() == 10 and ideg.argmax() == 0
    assert ideg.max() * N <= 3 * len(v0) + N and odeg.max() * N <= 3 * len(v0) + N
    return (N, *_i32(v0, v1))


def graph_sparse():
    """N = 257: a self loop at vertex 5, the single edge 200 -> 256 (the last vertex, alone in the second workgroup), every other vertex isolated"""
    return (257, *_i32([5, 200], [5, 256]))


def graph_one():
    return (1, *_i32([], []))


def graph_chain(N=300):
    return (N, *_i32(np.arange(N - 1), np.arange(1, N)))


STRIDE_N = MAX_PARTIALS * BLOCK + 300


def graph_stride():
    """a directed ring over 1024 * 256 + 300 vertices, out-degree 1: the smallest shape at which a lane of the capped grid visits a second vertex"""
    n = np.arange(STRIDE_N)
    return (STRIDE_N, *_i32(n, (n + 1) % STRIDE_N))


GRAPHS = {"mesh": graph_mesh, "deg8": graph_deg8, "deg10": graph_deg10, "hub": graph_hub, "sparse": graph_sparse, "one": graph_one, "stride": graph_stride}


# ------------------------------------------------------------------ inputs
def arap_inputs(N, seed=3, sentinels=True, w_fit=2.0, w_reg=1.5):
    """Position, Angle, Original, Constraints (float32 [N,3]) and the two weights.  Original: a unit-scale point cloud; Position: Original + 0.2 noise; angles uniform in
    +-3 rad (every entry of the rotation and of its derivatives carries weight); handles on about 10 % of the vertices, the others at -1e30.
    sentinels: vertex 0 is a handle whose Constraints.x is EXACTLY float32(-999999.9) (the threshold counts as constrained) and vertex 1 (N > 1) holds the next float32
    below it (unconstrained).  The huge fit term this gives sits at vertex 0 only, so every vertex range that starts at 1 or later has unit-scale sums."""
    rng = np.random.default_rng([seed, N])
    O = rng.standard_normal((N, 3)).astype(F32)
    P = (O + 0.2 * rng.standard_normal((N, 3))).astype(F32)
    A = rng.uniform(-3.0, 3.0, (N, 3)).astype(F32)
    C = np.full((N, 3), -1.0e30, F32)
    h = rng.random(N) < 0.1
    C[h] = (O[h] + 0.3 * rng.standard_normal((int(h.sum()), 3))).astype(F32)
    if sentinels:
        C[0] = O[0]; C[0, 0] = UNCONSTRAINED_BELOW
        if N > 1:
            C[1] = O[1]; C[1, 0] = np.nextafter(UNCONSTRAINED_BELOW, F32(-np.inf))
            assert C[1, 0] < UNCONSTRAINED_BELOW
    return SimpleNamespace(P=P, A=A, O=O, C=np.ascontiguousarray(C), w_fit=float(F32(w_fit)), w_reg=float(F32(w_reg)))


def arap_params(g, inp):
    """the params list of arap_mesh_deformation.t Inputs{} (0..7), fresh copies"""
    N, v0, v1 = g
    return [inp.w_fit, inp.w_reg, inp.P.copy(), inp.A.copy(), inp.O.copy(), inp.C.copy(), v0.copy(), v1.copy()]


# ------------------------------------------------------------------ ARAP in float64
def _axis_matrices(ang):
    """Rx(alpha), Ry(beta), Rz(gamma) and their derivatives, [n, 3, 3] each, from float64 angles [n, 3]"""
    s, c = np.sin(ang), np.cos(ang)
    z, o = np.zeros(len(ang)), np.ones(len(ang))
    m = lambda rows: np.stack([np.stack(r, -1) for r in rows], -2)
    sa, sb, sg = s.T; ca, cb, cg = c.T
    Rx = m([[o, z, z], [z, ca, -sa], [z, sa, ca]]);   dRx = m([[z, z, z], [z, -sa, -ca], [z, ca, -sa]])
    Ry = m([[cb, z, sb], [z, o, z], [-sb, z, cb]]);   dRy = m([[-sb, z, cb], [z, z, z], [-cb, z, -sb]])
    Rz = m([[cg, -sg, z], [sg, cg, z], [z, z, o]]);   dRz = m([[-sg, -cg, z], [cg, -sg, z], [z, z, z]])
    return Rx, Ry, Rz, dRx, dRy, dRz


def rotations(ang):
    """R = Rz Ry Rx and dR/dalpha, dR/dbeta, dR/dgamma ([n, 3, 3] each), and the same four with every factor replaced by its absolute value: entry by entry the sum of
    the absolute values of the trigonometric products the entry is made of"""
    Rx, Ry, Rz, dRx, dRy, dRz = _axis_matrices(np.asarray(ang, np.float64))
    mm = lambda a, b, c: a @ b @ c
    val = [mm(Rz, Ry, Rx), mm(Rz, Ry, dRx), mm(Rz, dRy, Rx), mm(dRz, Ry, Rx)]
    mag = [mm(np.abs(Rz), np.abs(Ry), np.abs(Rx)), mm(np.abs(Rz), np.abs(Ry), np.abs(dRx)), mm(np.abs(Rz), np.abs(dRy), np.abs(Rx)), mm(np.abs(dRz), np.abs(Ry), np.abs(Rx))]
    return val, mag


class ArapRef:
    """ARAP terms of one problem in float64.  Per-edge arrays are in INPUT edge order: F[e, c]; G[e, row, col], col = alpha, beta, gamma."""

    def __init__(self, g, inp):
        self.N, v0, v1 = g
        self.v0, self.v1 = np.asarray(v0, np.int64), np.asarray(v1, np.int64)
        self.E = len(self.v0)
        self.inp = inp
        self.wf, self.wr = float(F32(inp.w_fit)), float(F32(inp.w_reg))
        self.handle = inp.C[:, 0] >= UNCONSTRAINED_BELOW                                        # float32 comparison, as the kernel's
        self.P, self.O, self.C = (np.asarray(x, np.float64) for x in (inp.P, inp.O, inp.C))
        self.sin, self.cos = np.sin(inp.A.astype(np.float64)), np.cos(inp.A.astype(np.float64))
        self.F, self.F_abs, self.G, self.G_abs = self._edge_terms(self.P, inp.A.astype(np.float64))
        self.fit, self.fit_abs = self._fit(self.P)

    def _fit(self, P):
        h = self.handle[:, None]
        Cz = np.where(h, self.C, 0.0)
        return np.where(h, self.wf * (P - Cz), 0.0), np.where(h, self.wf * (np.abs(P) + np.abs(Cz)), 0.0)

    def _edge_terms(self, P, A):
        a, b = self.v0, self.v1
        (R, dA, dB, dG), (Rm, dAm, dBm, dGm) = rotations(A[a])
        dv = (self.O[a] - self.O[b])[:, :, None]; dvm = (np.abs(self.O[a]) + np.abs(self.O[b]))[:, :, None]
        F = self.wr * ((P[a] - P[b]) - (R @ dv)[:, :, 0])
        F_abs = self.wr * (np.abs(P[a]) + np.abs(P[b]) + (Rm @ dvm)[:, :, 0])
        G = np.concatenate([dA @ dv, dB @ dv, dG @ dv], 2)
        G_abs = np.concatenate([dAm @ dvm, dBm @ dvm, dGm @ dvm], 2)
        return F, F_abs, G, G_abs

    def residuals(self, x):
        """[fit 3N | reg 3E] at the flat unknown vector x = [Position | Angle]"""
        x = np.asarray(x, np.float64)
        P, A = x[:3 * self.N].reshape(-1, 3), x[3 * self.N:].reshape(-1, 3)
        return np.concatenate([self._fit(P)[0].ravel(), self._edge_terms(P, A)[0].ravel()])

    def x0(self):
        return np.concatenate([self.inp.P.astype(np.float64).ravel(), self.inp.A.astype(np.float64).ravel()])

    def triplets(self, G=None):
        """J as (row, col, value) with one entry per unknown ACCESS of a residual (a self loop's two Position accesses stay two entries)"""
        G = self.G if G is None else np.asarray(G, np.float64)
        N, E, a, b = self.N, self.E, self.v0, self.v1
        c = np.arange(3)
        hn = np.flatnonzero(self.handle)
        rows = [(3 * hn[:, None] + c).ravel()]; cols = [(3 * hn[:, None] + c).ravel()]; vals = [np.full(3 * len(hn), self.wf)]
        er = 3 * N + 3 * np.arange(E)[:, None] + c                                              # [E, 3] rows of edge e
        rows += [er.ravel(), er.ravel()]; cols += [(3 * a[:, None] + c).ravel(), (3 * b[:, None] + c).ravel()]
        vals += [np.full(3 * E, self.wr), np.full(3 * E, -self.wr)]
        for k in range(3):                                                                      # d reg_e[c] / d Angle_a[k] = -w_reg G_e[c, k]
            rows.append(er.ravel()); cols.append(np.repeat(3 * N + 3 * a + k, 3)); vals.append((-self.wr * G[:, :, k]).ravel())
        return np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64), np.concatenate(vals)

    def jacobian(self, G=None, G_abs=None):
        """J and |J| (absolute values taken per access, then added; G_abs: the magnitudes to take for the angle block instead of |G|) as scipy.sparse CSR matrices, and
        diag(J^T J) as the solver defines it: the sum of the squared partials per access (thallo.t: Pre[u] += partial * partial), which differs from the merged
        matrix's diagonal at a self loop only"""
        r, c, v = self.triplets(G)
        va = np.abs(v) if G_abs is None else np.abs(self.triplets(G_abs)[2])
        shape = (3 * self.N + 3 * self.E, 6 * self.N)
        return sp.csr_matrix((v, (r, c)), shape=shape), sp.csr_matrix((va, (r, c)), shape=shape), np.bincount(c, weights=v * v, minlength=6 * self.N)

    def system(self, F=None, G=None):
        """r = -J^T F, diag, M^-1 = guardedInvert(diag), z = M^-1 r and the alphaN terms r.z; F / G: per-edge terms to use instead of the reference's own (the device's,
        promoted: they then count as exact inputs and r_abs takes |F| for them; the fit residual is always formed here, so its magnitude is w_fit (|P| + |C|))"""
        J, Ja, diag = self.jacobian(G)
        res = np.concatenate([self.fit.ravel(), (self.F if F is None else np.asarray(F, np.float64)).ravel()])
        res_abs = np.concatenate([self.fit_abs.ravel(), (self.F_abs if F is None else np.abs(np.asarray(F, np.float64))).ravel()])
        r = -(J.T @ res)
        pre = sk.guarded_invert(diag)
        return SimpleNamespace(r=r, r_abs=Ja.T @ res_abs, diag=diag, pre=pre, z=pre * r, aN_terms=r * (pre * r), J=J, Ja=Ja)

    def apply(self, p, G=None, G_abs=None):
        """J^T J p and the sum of the absolute values of its terms |J|^T |J| |p|"""
        J, Ja, _ = self.jacobian(G, G_abs)
        p = np.asarray(p, np.float64)
        return J.T @ (J @ p), Ja.T @ (Ja @ np.abs(p))

    def cost_terms(self):
        """per vertex: its share of the cost as the kernel splits it, 0.5 (|fit_n|^2 + the |reg_e|^2 of the edges LEAVING n), and the same with every residual replaced by
        the sum of the absolute values of its terms (the scale of the share's error)"""
        t = 0.5 * ((self.fit ** 2).sum(1) + np.bincount(self.v0, weights=(self.F ** 2).sum(1), minlength=self.N))
        m = 0.5 * ((self.fit_abs ** 2).sum(1) + np.bincount(self.v0, weights=(self.F_abs ** 2).sum(1), minlength=self.N))
        return t, m

    def cost(self):
        return float(self.cost_terms()[0].sum())


def planes(v, N, n0, n1):
    """the entries of a flat vector [Position | Angle] that the vertex range [n0, n1) owns, as a mask"""
    m = np.zeros(len(v), bool)
    m[3 * n0:3 * n1] = True; m[3 * N + 3 * n0:3 * N + 3 * n1] = True
    return m


def per_vertex(v, N):
    """a flat vector's six entries per vertex added up: [N]"""
    v = np.asarray(v, np.float64)
    return v[:3 * N].reshape(N, 3).sum(1) + v[3 * N:6 * N].reshape(N, 3).sum(1)


# ------------------------------------------------------------------ graph Laplacian in float64
class LapRef:
    def __init__(self, g, X, A, w=LAP_W_FIT):
        self.N, v0, v1 = g
        self.v0, self.v1 = np.asarray(v0, np.int64), np.asarray(v1, np.int64)
        self.E = len(self.v0)
        self.w = float(F32(w))
        self.X, self.A = np.asarray(X, np.float64), np.asarray(A, np.float64)
        N, E = self.N, self.E
        r = np.concatenate([np.arange(N), N + np.arange(E), N + np.arange(E)])
        c = np.concatenate([np.arange(N), self.v0, self.v1])
        v = np.concatenate([np.full(N, self.w), np.ones(E), -np.ones(E)])
        self.J = sp.csr_matrix((v, (r, c)), shape=(N + E, N)); self.Ja = sp.csr_matrix((np.abs(v), (r, c)), shape=(N + E, N))
        self.diag = np.bincount(c, weights=v * v, minlength=N)                                  # per access, as above
        self.res = np.concatenate([self.w * (self.X - self.A), self.X[self.v0] - self.X[self.v1]])
        self.res_abs = np.concatenate([self.w * (np.abs(self.X) + np.abs(self.A)), np.abs(self.X[self.v0]) + np.abs(self.X[self.v1])])

    def cost_terms(self):
        t = 0.5 * (self.res[:self.N] ** 2 + np.bincount(self.v0, weights=self.res[self.N:] ** 2, minlength=self.N))
        m = 0.5 * (self.res_abs[:self.N] ** 2 + np.bincount(self.v0, weights=self.res_abs[self.N:] ** 2, minlength=self.N))
        return t, m

    def system(self):
        r = -(self.J.T @ self.res)
        return SimpleNamespace(r=r, r_abs=self.Ja.T @ self.res_abs, diag=self.diag, z=r.copy(), aN_terms=r * r)

    def apply(self, p):
        p = np.asarray(p, np.float64)
        return self.J.T @ (self.J @ p), self.Ja.T @ (self.Ja @ np.abs(p))


def checksum_i32(v, start=0):
    """thallo_hip_checksum_i32 in Python integers: start + sum (uint32(v[i]) + 0x9e3779b97f4a7c15) (2 i + 1) mod 2^64"""
    h = int(start)
    for i, x in enumerate(np.asarray(v, np.int32).view(np.uint32).tolist()):
        h += (x + 0x9E3779B97F4A7C15) * (2 * i + 1)
    return h % (1 << 64)
