"""tests/graph_reference.py checked on the CPU before any kernel is compared with it: its Jacobian against central differences of its own residuals, its r / diag /
J^T J p against the oracle (directed graphs included: the reference project's meshes always store both half-edges), and the incidence-list builder's invariants."""
import numpy as np
import pytest

import graph_reference as gr
from shim_kernels import F32

ORACLE_RTOL = 2e-5        # the bar of the oracle-against-CSR checks (test_oracle_golden.py)


def _problem(name, sentinels=False):
    g = gr.GRAPHS[name]()
    return g, gr.arap_inputs(g[0], sentinels=sentinels)


@pytest.mark.parametrize("name", ["mesh", "hub", "sparse", "one"])
def test_arap_jacobian_is_the_derivative_of_the_residuals(name):
    """central differences with step 1e-5 in float64: truncation ~ h^2 |d3 F| / 6 ~ 1e-10, rounding ~ 1e-16 / h ~ 1e-11; asserted to 1e-6 of the largest entry.
    (Without the sentinel constraint: a 1e6 residual would carry 1e-10 of absolute rounding into the quotient.)"""
    g, inp = _problem(name)
    ref = gr.ArapRef(g, inp)
    J = ref.jacobian()[0].toarray()
    x, h = ref.x0(), 1e-5
    fd = np.empty_like(J)
    for k in range(len(x)):
        d = np.zeros_like(x); d[k] = h
        fd[:, k] = (ref.residuals(x + d) - ref.residuals(x - d)) / (2 * h)
    assert J.shape == (3 * ref.N + 3 * ref.E, 6 * ref.N)
    assert np.abs(J - fd).max() <= 1e-6 * max(np.abs(J).max(), 1.0)
    if ref.E:
        assert np.abs(J[:, 3 * ref.N:]).max() > 0.1           # the angle block is there


@pytest.mark.parametrize("sentinels", [False, True])
@pytest.mark.parametrize("name", ["mesh", "hub", "sparse"])
def test_arap_reference_against_the_oracle(orc, name, sentinels):
    """r = -J^T F, diag(J^T J) and J^T J p against the oracle's float32 eval_jtf / apply_jtj.  `hub` and `sparse` are directed (in-degree != out-degree, a self loop,
    isolated vertices): this is also the check that the oracle handles such graphs."""
    g, inp = _problem(name, sentinels)
    ref = gr.ArapRef(g, inp)
    prob = orc.Problem(orc.ARAP_MESH, (ref.N, ref.E), gr.arap_params(g, inp))
    s = ref.system()
    r, diag = prob.eval_jtf()
    assert np.abs(r - s.r).max() <= ORACLE_RTOL * np.abs(s.r).max()
    assert np.abs(diag - s.diag).max() <= ORACLE_RTOL * np.abs(s.diag).max()
    p = np.random.default_rng(5).standard_normal(6 * ref.N).astype(F32)
    Ap, _ = prob.apply_jtj(p)
    want, _ = ref.apply(p)
    assert np.abs(Ap - want).max() <= ORACLE_RTOL * np.abs(want).max()
    assert abs(prob.cost() - ref.cost()) <= ORACLE_RTOL * ref.cost()
    if sentinels:                                                                          # the threshold itself is a handle, the float below it is not
        assert ref.handle[0] and not ref.handle[1] and abs(r[0]) > 1e6


@pytest.mark.parametrize("name", ["sparse", "one", "hub"])
def test_laplacian_reference_against_the_oracle(orc, name):
    g = gr.GRAPHS[name]()
    N = g[0]
    rng = np.random.default_rng(8)
    X, A = rng.standard_normal(N).astype(F32), rng.standard_normal(N).astype(F32)
    ref = gr.LapRef(g, X, A)
    prob = orc.Problem(orc.LAPLACIAN_GRAPH, (N, ref.E), [X.copy(), A.copy(), g[1].copy(), g[2].copy()], fconst=[gr.LAP_W_FIT])
    s = ref.system()
    r, diag = prob.eval_jtf()
    assert np.abs(r - s.r).max() <= ORACLE_RTOL * np.abs(s.r).max()
    assert np.abs(diag - s.diag).max() <= ORACLE_RTOL * s.diag.max()
    p = rng.standard_normal(N).astype(F32)
    assert np.abs(prob.apply_jtj(p)[0] - ref.apply(p)[0]).max() <= ORACLE_RTOL * np.abs(ref.apply(p)[0]).max()
    assert abs(prob.cost() - ref.cost_terms()[0].sum()) <= ORACLE_RTOL * ref.cost_terms()[0].sum()


def test_magnitudes_bound_the_values():
    g, inp = _problem("hub", True)
    ref = gr.ArapRef(g, inp)
    s = ref.system()
    p = np.random.default_rng(5).standard_normal(6 * ref.N)
    Ap, Ap_abs = ref.apply(p)
    assert (np.abs(ref.F) <= ref.F_abs).all() and (np.abs(ref.G) <= ref.G_abs).all() and (np.abs(s.r) <= s.r_abs).all() and (np.abs(Ap) <= Ap_abs).all()
    assert (ref.cost_terms()[0] <= ref.cost_terms()[1]).all()


def _layouts(g):
    N, v0, v1 = g
    out = [gr.build_lists(N, v0, v1)]
    if len(v0):
        mo, mi = gr.ell_slots(N, v0, v1)
        out += [gr.build_lists(N, v0, v1, mo, mi), gr.build_lists(N, v0, v1, mo + 2, mi + 1)]
    return out


@pytest.mark.parametrize("name", ["mesh", "deg8", "deg10", "hub", "sparse", "one"])
def test_incidence_lists(name):
    """Every edge once in each list; in_edge points at the edge's out-position in the same layout; the order within a vertex is the input order; every index, padding
    included, is in range; padding never aliases a real slot."""
    g = gr.GRAPHS[name]()
    N, v0, v1 = g
    E = len(v0)
    for L in _layouts(g):
        assert L.out_ptr[0] == 0 and L.out_ptr[-1] == E and L.in_ptr[-1] == E
        assert np.array_equal(np.diff(L.out_ptr), np.bincount(v0, minlength=N)) and np.array_equal(np.diff(L.in_ptr), np.bincount(v1, minlength=N))
        assert len(np.unique(L.pos)) == E and len(np.unique(L.ipos)) == E                    # once in each list
        assert np.array_equal(L.out_v1[L.pos], v1) and np.array_equal(L.in_src[L.ipos], v0) and np.array_equal(L.in_edge[L.ipos], L.pos)
        for arr, hi in ((L.out_v1, N), (L.in_src, N), (L.in_edge, max(L.edges, 1))):
            assert arr.size == 0 or (arr.min() >= 0 and arr.max() < hi)
        for n in range(N):                                                                  # slot j of vertex n, in input order
            eo, ei = np.flatnonzero(v0 == n), np.flatnonzero(v1 == n)
            if L.ell_stride:
                assert np.array_equal(L.pos[eo], np.arange(len(eo)) * N + n) and np.array_equal(L.ipos[ei], np.arange(len(ei)) * N + n)
            else:
                assert np.array_equal(L.pos[eo], L.out_ptr[n] + np.arange(len(eo))) and np.array_equal(L.ipos[ei], L.in_ptr[n] + np.arange(len(ei)))
        if L.ell_stride:
            assert L.ell_stride == L.out_slots * N and L.out_v1.size == L.ell_stride and L.in_edge.size == L.in_src.size == L.in_slots * N
            assert L.pad.sum() == L.ell_stride - E and not L.pad[L.pos].any()
        else:
            assert L.out_v1.size == E and not L.pad.any()
        F = np.arange(3 * L.edges, dtype=np.float64)                                         # edge_plane reads each layout back into input edge order
        want = (np.arange(3)[None, :] * L.edges + L.pos[:, None]) if L.ell_stride else (3 * L.pos[:, None] + np.arange(3)[None, :])
        assert np.array_equal(gr.edge_plane(L, F, 3), want)


def test_graph_generators_state_their_shapes():
    N, v0, v1 = gr.graph_hub()
    assert gr.ell_slots(N, v0, v1) == (3, 10)
    assert np.bincount(gr.graph_deg8()[1]).min() >= 6
    N, v0, v1 = gr.graph_stride()
    assert N == 1024 * 256 + 300 and gr.vgrid(N) == 1024 and gr.visits(0, N) == 2
    assert gr.vgrid(1) == 1 and gr.vgrid(257) == 2 and gr.visits(100, 257) == 1


def test_checksum_formula():
    v = np.array([3, -1, 7], np.int32)
    want = sum((int(np.uint32(x)) + 0x9E3779B97F4A7C15) * (2 * i + 1) for i, x in enumerate(v)) % 2 ** 64
    assert gr.checksum_i32(v) == want and gr.checksum_i32(v, 5) == (want + 5) % 2 ** 64
    assert gr.checksum_i32(v[[1, 0, 2]]) != want
