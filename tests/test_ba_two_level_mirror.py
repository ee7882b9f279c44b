"""CPU: the restatement of the two-level preconditioner on the assembled reduced camera matrix (tests/ba_two_level_mirror.py; thallo_amd/csrc/ba_coarse.hip,
ThalloX_PlanSetPreconditioner THALLOX_PRECOND_TWO_LEVEL).

The aggregates (a partition, at most k members, deterministic, a caller's array validated); in float64 M^-1 = G^T G + P Z^T Z P^T symmetric, positive definite on the free
scalars, exactly zero at held rows and columns, the identity's row where every member of an aggregate holds a scalar; PCG ITERATION COUNTS in float32 numpy on one unit
column with cameras {0, 1} held and the default aggregates, against block Jacobi on the same S (printed; measured here: (200, 6000, 26000) band 32 in id order 228 -> 96,
ids shuffled 177 -> 68; (600, 40000, 170000) shuffled 701 -> 136); GN 3 x 50 and LM 3 x 50 trajectories against the block-Jacobi mirror; the library's declarations and exports."""
import os
import re

import numpy as np
import pytest

import thallo_amd
from thallo_amd import api, synthetic as syn

import ba_covariance_mirror as cm
import ba_two_level_mirror as tl
from ba_held_mirror import HeldSchurExplicitMirror
from ba_schur_explicit_mirror import BaSchurExplicitMirror, SchurLists, SchurStructure

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = [((24, 300, 1200), 12), ((48, 1200, 5000), 16)]


def two_cameras(C, P):
    m = np.zeros(9 * C + 3 * P, bool); m[:18] = True
    return m


def structure(dims, band, shuffle=False):
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    if shuffle: p = tl.shuffled_cameras(p)
    return SchurStructure(SchurLists(p[3], p[4], dims[0], dims[1]))


@pytest.mark.parametrize("dims,band,shuffle,k", [((24, 300, 1200), 12, False, 8), ((48, 1200, 5000), 16, True, 5), ((200, 6000, 26000), 32, True, 8), ((24, 300, 1200), 12, False, 1),
                                               ((24, 300, 1200), 12, False, 100)])
def test_greedy_aggregates_are_a_deterministic_partition_of_at_most_k(dims, band, shuffle, k):
    st = structure(dims, band, shuffle)
    agg, mem_ptr, mem = tl.greedy_aggregates(st, k)
    C = dims[0]; K = len(mem_ptr) - 1
    assert sorted(mem.tolist()) == list(range(C)) and (agg >= 0).all() and agg.max() == K - 1
    assert np.diff(mem_ptr).max() <= k and np.diff(mem_ptr).min() >= 1
    for a in range(K): assert (agg[mem[mem_ptr[a]:mem_ptr[a + 1]]] == a).all()
    assert [int(mem[mem_ptr[a]]) for a in range(K)] == sorted(int(mem[mem_ptr[a]]) for a in range(K))      # the seeds ascend
    again = tl.greedy_aggregates(structure(dims, band, shuffle), k)
    assert (again[0] == agg).all() and (again[1] == mem_ptr).all() and (again[2] == mem).all()
    assert tl.validate_aggregates(agg, C) is None
    if k == 1: assert K == C
    if k >= C: assert K == 1      # (the ring is connected)


def test_greedy_aggregates_follow_co_visibility_not_ids():
    """with shuffled ids the members of an aggregate are still neighbours on the ring: every member shares points with another member"""
    st = structure((48, 1200, 5000), 16, True)
    agg, mem_ptr, mem = tl.greedy_aggregates(st, 8)
    pairs = {(int(i), int(j)) for i, j in zip(st.row, st.colj)} | {(int(j), int(i)) for i, j in zip(st.row, st.colj)}
    for a in range(len(mem_ptr) - 1):
        ms = mem[mem_ptr[a]:mem_ptr[a + 1]]
        for c in ms[1:]: assert any((int(c), int(o)) in pairs for o in ms if o != c)


def test_a_callers_array_is_validated():
    C = 6
    assert tl.validate_aggregates(np.array([0, 0, 1, 1, 2, 2]), C) is None
    assert "cameras" in tl.validate_aggregates(np.array([0, 0, 1]), C)
    assert "range" in tl.validate_aggregates(np.array([0, 0, 1, 1, 2, -1]), C)
    assert "range" in tl.validate_aggregates(np.array([0, 0, 1, 1, 2, 6]), C)
    assert "dense" in tl.validate_aggregates(np.array([0, 0, 1, 1, 3, 3]), C)
    mem_ptr, mem = tl.member_lists(np.array([1, 0, 1, 0, 2, 2]))
    assert mem_ptr.tolist() == [0, 2, 4, 6] and mem.tolist() == [1, 3, 0, 2, 4, 5]


@pytest.fixture(scope="module")
def small():
    """(24, 300, 1200) after LM 3 x 50 of the assembled mirror; the masks: camera 0 and 1 held; camera 0 held and scalar 6 held on every member of camera 5's aggregate"""
    dims = (24, 300, 1200)
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=12)
    m = BaSchurExplicitMirror(dims, p)
    m.lm_solve(3, 50, q_tolerance=0.1, function_tolerance=0.0)
    return dims, m


@pytest.mark.parametrize("which", ["two_cameras", "scalar_6_of_an_aggregate"])
def test_float64_the_preconditioner_is_symmetric_positive_definite_on_the_free_set_and_zero_at_held_scalars(small, which):
    dims, m = small
    C, P = dims[0], dims[1]
    mask = two_cameras(C, P)
    J, sys = cm.system_of(m, mask)
    agg, mem_ptr, mem = tl.greedy_aggregates(sys.st, 4)
    if which != "two_cameras":
        a = agg[5]
        mask = np.zeros(9 * C + 3 * P, bool); mask[:9] = True
        for c in mem[mem_ptr[a]:mem_ptr[a + 1]]: mask[9 * c + 6] = True
        J, sys = cm.system_of(m, mask)
    hold_c = mask[:9 * C].reshape(-1, 9)
    co = tl.Coarse(sys.st, sys.S, agg, hold_c, np.float64)
    assert co.failed == 0
    G = np.asarray(sys.M.parts[0][1], np.float64)
    MB = np.zeros((9 * C, 9 * C))
    for c in range(C): MB[9 * c:9 * c + 9, 9 * c:9 * c + 9] = G[c].T @ G[c]
    M = MB + co.dense()
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    held = hold_c.ravel()
    assert not M[held].any() and not M[:, held].any()
    f = np.nonzero(~held)[0]
    assert np.linalg.eigvalsh(M[np.ix_(f, f)]).min() > 0
    # the coarse term is the inverse of P^T S P on the coarse scalars that exist: Z^T Z S_c = I there
    live = co.d > 0
    ZtZ = co.Z.T @ co.Z
    assert np.abs((ZtZ @ co.Sc)[np.ix_(live, live)] - np.eye(int(live.sum()))).max() < 1e-8
    if which == "two_cameras":
        assert co.identity_rows == (9 if len(set(agg[:2])) == 1 and np.diff(mem_ptr)[agg[0]] == 2 else 0)
    else:
        i = 9 * agg[5] + 6
        assert co.d[i] == 0 and co.identity_rows >= 1
        assert co.T[i, i] == 1 and not np.delete(co.T[i], i).any() and not np.delete(co.T[:, i], i).any()
        assert not co.Z[i].any() and not co.Z[:, i].any()


def iteration_counts(dims, shuffle):
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=32)
    if shuffle: p = tl.shuffled_cameras(p)
    C, P = dims[0], dims[1]
    mask = two_cameras(C, P)
    J, sys = cm.system_of(BaSchurExplicitMirror(dims, p), mask)
    S = sys.Sm.toarray().astype(F)
    MB = tl.dense_precond32(sys)
    b = np.zeros(9 * C, F); b[9 * (C // 2)] = 1
    _, it_block, rel_block = tl.pcg32(S, MB, b)
    agg = tl.greedy_aggregates(sys.st, tl.default_k(C))[0]
    co = tl.Coarse(sys.st, sys.S, agg, mask[:9 * C].reshape(-1, 9), F)
    assert co.failed == 0
    _, it_two, rel_two = tl.pcg32(S, (MB.astype(np.float64) + co.dense()).astype(F), b)
    print("%s %s: block Jacobi %d iterations (%.2e), two-level %d (%.2e), K = %d, ratio %.3f" % (dims, "shuffled" if shuffle else "in id order", it_block, rel_block, it_two, rel_two, co.K,
                                                                                                it_two / it_block))
    assert rel_block <= 1e-6 and rel_two <= 1e-6
    return it_block, it_two


@pytest.mark.parametrize("shuffle", [False, True])
def test_iterations_at_200_cameras_are_at_most_three_quarters_of_block_jacobis(shuffle):
    it_block, it_two = iteration_counts((200, 6000, 26000), shuffle)
    assert it_two <= 0.75 * it_block


def test_iterations_at_600_shuffled_cameras_are_at_most_two_fifths_of_block_jacobis():
    it_block, it_two = iteration_counts((600, 40000, 170000), True)
    assert it_two <= 0.4 * it_block


@pytest.mark.parametrize("dims,band", TABLE)
def test_trajectories_end_where_block_jacobis_do_with_no_more_iterations(dims, band):
    """GN 3 x 50 and LM 3 x 50 with cameras {0, 1} held: the final cost within the block-Jacobi mirror's own last-step change of cost, no more linear iterations in total.
    (GN runs a fixed number of linear iterations: the two preconditioners take the same step only where both inner solves have converged, so GN gets LM's budget of 50.
    At 10 the two-level form simply ends LOWER: (48, 1200, 5000) 3020.73 against 3021.09, the last change 0.23.)"""
    C, P = dims[0], dims[1]
    mask = two_cameras(C, P)
    def fresh(cls, **kw):
        return cls(dims, syn.bundle_adjustment(C=C, P=P, O=dims[2], band=band), mask, **kw)
    ref = fresh(HeldSchurExplicitMirror).gn_solve(3, 50)
    got = fresh(tl.BaTwoLevelMirror).gn_solve(3, 50)
    print(dims, "GN 3 x 50: block", ref[-1], "two-level", got[-1], "last change", abs(ref[-1] - ref[-2]))
    assert abs(got[-1] - ref[-1]) <= abs(ref[-1] - ref[-2])
    ref, it_ref = fresh(HeldSchurExplicitMirror).lm_solve(3, 50, q_tolerance=0.1, function_tolerance=0.0)
    got, it_got = fresh(tl.BaTwoLevelMirror).lm_solve(3, 50, q_tolerance=0.1, function_tolerance=0.0)
    print(dims, "LM 3 x 50: block", ref[-1], it_ref, "two-level", got[-1], it_got, "last change", abs(ref[-1] - ref[-2]))
    assert abs(got[-1] - ref[-1]) <= abs(ref[-1] - ref[-2])
    assert sum(it_got) <= sum(it_ref)


def test_the_float32_restatements_agree_with_the_float64_coarse_matrix(small):
    """assemble32 / scale32 / apply32 (the kernels' order) against Coarse in float64 on the same S"""
    dims, m = small
    C, P = dims[0], dims[1]
    mask = two_cameras(C, P)
    J, sys = cm.system_of(m, mask)
    hold_c = mask[:9 * C].reshape(-1, 9)
    agg, mem_ptr, mem = tl.greedy_aggregates(sys.st, 4)
    co = tl.Coarse(sys.st, sys.S, agg, hold_c, np.float64)
    Sc = tl.assemble32(sys.st, sys.S, agg, mem_ptr, mem, hold_c)
    assert np.abs(Sc - np.tril(co.Sc)).max() <= 1e-5 * np.abs(co.Sc).max()
    T, d, ident = tl.scale32(Sc)
    assert ident == co.identity_rows and np.abs(T - np.tril(co.T)).max() <= 1e-5
    r = np.random.default_rng(0).standard_normal(9 * C).astype(F)
    out, y, part = tl.apply32(co.Z.astype(F), co.Z.T.astype(F).copy(), mem_ptr, mem, r, hold_c)
    ref = co.apply(r)
    assert np.abs(out - ref).max() <= 1e-4 * np.abs(ref).max()
    assert abs(float(part.astype(np.float64).sum()) - float(co.y(r) @ co.y(r))) <= 1e-4 * float(co.y(r) @ co.y(r))
    assert not out.reshape(-1, 9)[hold_c].any()


def test_the_library_declares_and_exports_the_calls():
    """without the library change this fails: the constant, the setters, the getter and the kernels' entry points are declared in the headers and exported by libThallo.so,
    ThalloSolver knows the kind, the setter and the getter"""
    from thallo_amd.build import build_library
    build_library()
    L = thallo_amd.lib()
    names = {"Thallo.h": ["ThalloX_PlanSetCoarseAggregates", "ThalloX_PlanCoarseSpace"],
             "thallo_hip.h": ["thallo_hip_ba_coarse_assemble", "thallo_hip_ba_coarse_scale", "thallo_hip_ba_coarse_inverse", "thallo_hip_ba_coarse_panel_floats", "thallo_hip_ba_coarse_apply",
                              "thallo_hip_ba_coarse_apply_cols", "thallo_hip_ba_coarse_cols_work_floats", "thallo_hip_ba_cov_solve_coarse", "thallo_hip_ba_cov_coarse_work_bytes"]}
    for header, want in names.items():
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        declared = set(re.findall(r"\b((?:Thallo_|ThalloX_|thallo_hip_)\w+)\s*\(", txt))
        for n in want: assert n in declared and hasattr(L, n), n
    assert re.search(r"#define\s+THALLOX_PRECOND_TWO_LEVEL\s+2\b", open(os.path.join(ROOT, "include", "Thallo.h")).read())
    assert api.ThalloSolver.PRECONDITIONERS["two_level"] == 2
    assert callable(getattr(api.ThalloSolver, "set_coarse_aggregates", None)) and callable(getattr(api.ThalloSolver, "coarse_space", None))
