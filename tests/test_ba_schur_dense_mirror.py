"""CPU: the restatement of bundle adjustment's dense Cholesky Schur solve (tests/ba_schur_dense_mirror.py; thallo_amd/csrc/ba_schur_dense.hip, ThalloX_PlanSetLinearSolver
kind 3).

Instances: the covariance tests' (5, 72, 330) band 5 and (3, 160, 480) band 3 with their extras (a camera and a point nothing observes, a point observed once),
(24, 300, 1200) band 12 and (48, 1200, 5000) band 16.  The gauge, where one is held, is tests/ba_covariance_mirror.py's: camera 0 entirely plus scalar 3 of camera 1.

Bars.  delta_c against float64: with T = D S D the scaled system the factor works on, the float32 Cholesky solve satisfies (T + dT) y = D g with |dT| <= gamma_{3n+1} |L||L^T|
(Higham, Accuracy and Stability, theorem 10.4), hence |y - y_ref| / |y_ref| <= cond_2(T_FF) gamma_{3n+1} in the 2-norm to first order, taking || |L||L^T| ||_2 <= ||T||_2 as the
rule of thumb does (the rigorous factor n is never attained); u = 2^-24.  The covariance: the study's figures behind the issue (7.3e-5 and 2.4e-4 over all cameras), as an upper
bound with a factor 2 for another LAPACK build; the GPU tests take 4 x the mirror's own error, recomputed there.  Every figure is printed before it is asserted."""
import os
import re

import numpy as np
import pytest

import thallo_amd
from thallo_amd import api, synthetic as syn

import ba_covariance_mirror as cm
import ba_schur_dense_mirror as dm
from ba_schur_dense_mirror import BaSchurDenseMirror, DensePivot
from ba_schur_explicit_mirror import BaSchurExplicitMirror
from ba_schur_mirror import with_extras
from test_ba_covariance_mirror import Instance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SHAPES = [((5, 72, 330), 5, True), ((3, 160, 480), 3, True), ((24, 300, 1200), 12, False)]
TABLE = [((24, 300, 1200), 12, 7.3e-5), ((48, 1200, 5000), 16, 2.4e-4)]      # ..., the study's covariance error over all cameras


def gamma(k): return k * U / (1 - k * U)


def instance(dims, band, extras=False):
    p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
    if extras: p, dims = with_extras(p)
    return p, dims


@pytest.fixture(scope="module")
def instances():
    cache = {}

    def get(dims, band, extras):
        if dims not in cache: cache[dims] = Instance(dims, band, extras)
        return cache[dims]
    return get


@pytest.mark.parametrize("dims,band,extras", SHAPES)
def test_delta_c_is_the_float64_solve_on_the_free_cameras(dims, band, extras):
    """one GN step with the gauge held: delta_c against np.linalg.solve in float64 on S_FF of the mirror's own float32 S, in the scaled coordinates; exactly 0.0f at the held
    scalars and at the scalars of the camera nothing observes, which are counted"""
    p, dims = instance(dims, band, extras)
    mask = cm.gauge_mask(dims[0], dims[1])
    m = BaSchurDenseMirror(dims, p, mask)
    before = [a.copy() for a in m.params]
    assert m.gn_step() and m.pivot is None
    S, dc = m.last_system, m.last_delta_c
    Sd, hold = S.dense()
    free = ~hold & (S.d > 0)
    assert S.nonpos == (9 if extras else 0) == int((~hold & ~free).sum())
    assert dc.dtype == np.float32 and not dc[~free].any() and dc[free].all()
    S64 = Sd.astype(np.float64)[np.ix_(free, free)]
    ref = np.linalg.solve(S64, S.g.astype(np.float64)[free])
    d = S.d.astype(np.float64)[free]
    T64 = d[:, None] * S64 * d[None, :]
    n = int(free.sum())
    cond = np.linalg.cond(T64)
    err = np.linalg.norm((dc[free] - ref) / d) / np.linalg.norm(ref / d)
    bar = cond * gamma(3 * n + 1)
    print("dense mirror", dims, "n free", n, "cond(T_FF)", cond, "delta_c error (scaled, 2-norm)", err, "bar", bar, "= %.3f of it" % (err / bar))
    assert err <= bar
    # the held cameras' bits are those before the step
    assert m.params[0].reshape(-1)[hold].tobytes() == before[0].reshape(-1)[hold].tobytes()


def test_the_expansion_is_two_rounded_products_with_identity_rows():
    rng = np.random.default_rng(3)
    M = rng.standard_normal((40, 27)); S = (M @ M.T / 27 + np.eye(40)).astype(np.float32) * np.float32(50)
    S[11, 11] = 0; S[30, 30] = -1
    hold = np.zeros(40, bool); hold[[2, 3]] = True
    T, d, nonpos = dm.expand32(S, hold)
    dead = [2, 3, 11, 30]
    assert nonpos == 2 and not d[dead].any() and (d[np.setdiff1d(np.arange(40), dead)] > 0).all()
    E = np.eye(40, dtype=np.float32)
    assert (T[dead] == E[dead]).all() and (T[:, dead] == E[:, dead]).all()
    i, j = 17, 5
    assert T[i, j] == np.float32(np.float32(d[i] * S[i, j]) * d[j])


@pytest.mark.parametrize("dims,band", [(d, b) for d, b, _ in TABLE])
def test_lm_costs_are_monotone_and_end_at_the_pcg_mirrors_cost(dims, band):
    """LM with the exact solve: over 6 steps the cost never rises; and after STEPS steps it is within the assembled PCG mirror's own last-step change of that mirror's cost
    after as many steps (x 150 iterations, q_tolerance 0.1) -- the exact solve is at the minimum at least as early.  STEPS = 4: the last step at which the PCG mirror still
    moves.  (After 6 steps its last change is exactly 0 in the float32 cost on (24, 300, 1200) while the two minima, 665.04626 and 665.04620, differ by two units in the
    last place of that cost: a comparison below the cost's own resolution.)"""
    STEPS = 4
    p, dims = instance(dims, band)
    kw = dict(q_tolerance=0.1, function_tolerance=0.0)
    dense = BaSchurDenseMirror(dims, p)
    cd, it = dense.lm_solve(6, **kw)
    pcg = BaSchurExplicitMirror(dims, p)
    cp, itp = pcg.lm_solve(STEPS, 150, **kw)
    print("dense mirror LM", dims, "dense", cd, "pcg", cp, itp)
    assert dense.pivot is None and it == [0] * 6 and len(cd) == 7 and len(cp) == STEPS + 1
    assert all(b <= a for a, b in zip(cd, cd[1:]))
    assert cp[-1] != cp[-2]
    assert abs(cd[STEPS] - cp[-1]) <= abs(cp[-1] - cp[-2])
    assert all(a <= b * (1 + 1e-6) for a, b in zip(cd[1:], cp[1:]))      # never behind the PCG mirror, step for step


@pytest.mark.parametrize("dims,band,table", TABLE)
def test_the_covariance_through_the_factor_is_the_studys(instances, dims, band, table):
    """all cameras (and 21 points) through the float32 factor against the float64 dense inverse of A_FF: the error is printed -- it sets the GPU bar -- and is within twice
    the study's figure; the float32 column PCG on the same instance is printed next to it.  Held rows and columns are exactly zero (cov_error asserts it), the blocks
    symmetric bit for bit, nothing iterates"""
    I = instances(dims, band, False)
    _, sys = dm.gn_system(I.m, I.mask)
    cov = dm.DenseCovariance(sys, I.mask)
    cams = [c for c in range(I.C) if not I.und[9 * c]]
    B, info = cov.solve(0, cams)
    err = cm.cov_error(B, I.ref(0, cams), I.free_of(0, cams))
    Bp, ip = I.pcg.solve(0, cams[:7])
    print("dense covariance mirror", I.dims, "cameras: error", err, "study", table, info, "| column PCG on 7 cameras:", cm.cov_error(Bp, I.ref(0, cams[:7]), I.free_of(0, cams[:7])), ip["iterations"])
    assert err <= 2 * table
    assert info == dict(iterations=0, columns=int(I.free_of(0, cams).sum()), not_converged=0, nan_blocks=0, worst_residual=0.0)
    assert B.tobytes() == np.transpose(B, (0, 2, 1)).tobytes()
    Bq, iq = cov.solve(1, I.pts)
    errp = cm.cov_error(Bq, I.ref(1, I.pts), I.free_of(1, I.pts))
    print("dense covariance mirror", I.dims, "points: error", errp, iq)
    assert errp <= 2 * table and iq["nan_blocks"] == 0 and iq["columns"] == 3 * len(I.pts)


def test_the_covariance_with_extras_counts_the_unobserved_camera_and_the_nan_points(instances):
    """(5, 72, 330) with its extras: the camera nothing observes has non-positive diagonals -- its nine columns are reported as not converged and its block stays zero; the
    point nothing observes and the point observed once are NaN blocks"""
    I = instances(*SHAPES[0])
    _, sys = dm.gn_system(I.m, I.mask)
    cov = dm.DenseCovariance(sys, I.mask)
    assert sys.nonpos == 9
    B, info = cov.solve(0, [1, I.C - 1])
    assert info["not_converged"] == 9 and info["columns"] == 8 and not B[1].any() and B[0][0, 0] > 0 and not B[0][3].any()
    Bq, iq = cov.solve(1, I.pts)
    ok = ~np.isnan(Bq[:, 0, 0])
    assert iq["nan_blocks"] == 2 == int((~ok).sum())
    err = cm.cov_error(Bq[ok], I.ref(1, I.pts)[ok], I.free_of(1, I.pts)[ok])
    print("dense covariance mirror", I.dims, "points with extras: error", err)
    assert err < 1e-2


@pytest.mark.parametrize("dims,band,extras", SHAPES)
def test_gn_without_a_gauge_reports_a_pivot_and_with_one_does_not(dims, band, extras):
    """the float32 factor of the singular (but consistent) GN system meets a non-positive pivot at one of its last scalars: the step is not taken, the unknowns keep their
    bits; with the gauge held three GN steps run and lower the cost"""
    p, dims = instance(dims, band, extras)
    m = BaSchurDenseMirror(dims, p)
    before = [a.copy() for a in m.params]
    costs = m.gn_solve(3)
    print("dense mirror GN without a gauge", dims, "pivot", m.pivot)
    assert isinstance(m.pivot, DensePivot) and len(costs) == 1
    assert 0 <= m.pivot.index < 9 * dims[0] and m.pivot.index == 9 * m.pivot.camera + m.pivot.scalar
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.params, before))
    g = BaSchurDenseMirror(dims, p, cm.gauge_mask(dims[0], dims[1]))
    costs = g.gn_solve(3)
    print("dense mirror GN with the gauge held", dims, costs)
    assert g.pivot is None and len(costs) == 4 and costs[-1] < costs[0]
    assert g.params[0].reshape(-1)[:9].tobytes() == np.asarray(p[0]).reshape(-1)[:9].tobytes()


def test_the_library_declares_and_exports_the_calls():
    """without the library change this fails: the constant, the getter and the kernels' entry points are declared in the headers and exported by libThallo.so (as
    tests/test_cabi.py checks every symbol), ThalloSolver knows the kind and the getter, and the THALLO_AB key is in the library's table"""
    from thallo_amd.build import build_library
    build_library()
    L = thallo_amd.lib()
    names = {"Thallo.h": ["ThalloX_PlanSchurDenseNonPositive"],
             "thallo_hip.h": ["thallo_hip_dense_ld", "thallo_hip_ba_schur_dense_expand", "thallo_hip_dense_potrf", "thallo_hip_dense_potrs_cols", "thallo_hip_dense_potrs_vec"]}
    for header, want in names.items():
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        declared = set(re.findall(r"\b((?:Thallo_|ThalloX_|thallo_hip_)\w+)\s*\(", txt))
        for n in want: assert n in declared and hasattr(L, n), n
    assert re.search(r"#define\s+THALLOX_SOLVER_SCHUR_DENSE\s+3\b", open(os.path.join(ROOT, "include", "Thallo.h")).read())
    assert api.ThalloSolver.LINEAR_SOLVERS["schur_dense"] == 3
    assert callable(getattr(api.ThalloSolver, "schur_dense_nonpositive", None))
    assert "schur_dense_max_mb" in open(os.path.join(ROOT, "thallo_amd", "csrc", "solver.cpp")).read()
