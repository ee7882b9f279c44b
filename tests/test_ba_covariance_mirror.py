"""CPU: the restatement of bundle adjustment's marginal covariances (tests/ba_covariance_mirror.py; thallo_amd/csrc/ba_covariance.hip, ThalloX_PlanCovariance).

Instances: the Schur tests' (5, 72, 330) band 5 and (3, 160, 480) band 3 with their extras (a camera and a point nothing observes, a point observed once) and
(24, 300, 1200) band 12, each after LM 3 x 50 of the assembled mirror, the gauge held as camera 0 entirely plus scalar 3 of camera 1.  The reference is the dense float64
inverse of A_FF from the oracle's J, F the scalars that are neither held nor undetermined (the extras).

The float32 column mirror's error and iterations under the defaults (rel_tol 1e-6, 500 iterations) are printed: they are what the GPU tests' bars are taken from
(4 x the mirror's own error on the same instance, recomputed there)."""
import os
import re

import numpy as np
import pytest

import thallo_amd
from thallo_amd import api, synthetic as syn

import ba_covariance_mirror as cm
from ba_schur_explicit_mirror import BaSchurExplicitMirror
from ba_schur_mirror import with_extras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((5, 72, 330), 5, True), ((3, 160, 480), 3, True), ((24, 300, 1200), 12, False)]


class Instance:
    """one shape: the mirror after LM 3 x 50, its masked assembled system, A, the free set, the float64 covariance and the float32 column PCG -- computed once, never changed"""

    def __init__(self, dims, band, extras):
        p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
        if extras: p, dims = with_extras(p)
        self.dims = dims
        self.C, self.P, _ = dims
        self.m = BaSchurExplicitMirror(dims, p)
        self.m.lm_solve(3, 50, q_tolerance=0.1, function_tolerance=0.0)
        self.mask = cm.gauge_mask(self.C, self.P)
        J, self.sys = cm.system_of(self.m, self.mask)
        self.A = (J.T @ J).toarray()
        self.und = cm.undetermined(self.A, self.C)
        self.free = ~self.mask & ~self.und
        self.Sig = cm.dense_cov64(self.A, self.free)
        self.pcg = cm.ColumnPCG32.of(self.sys, self.mask)
        self.cams = [c for c in range(self.C) if not self.und[9 * c]][:7]
        self.pts = list(range(0, self.P - 2, max(1, self.P // 21)))[:19] + ([self.P - 2, self.P - 1] if extras else [])      # (the extras: the point nothing observes, the point observed once)

    def free_of(self, mode, ids):
        nc = 9 * self.C
        return (self.free[:nc].reshape(-1, 9) if mode == 0 else self.free[nc:].reshape(-1, 3))[ids]

    def ref(self, mode, ids):
        return cm.blocks_of(self.Sig, ids, 9) if mode == 0 else cm.blocks_of(self.Sig, ids, 3, 9 * self.C)


@pytest.fixture(scope="module")
def instances():
    cache = {}

    def get(dims, band, extras):
        if dims not in cache: cache[dims] = Instance(dims, band, extras)
        return cache[dims]
    return get


@pytest.mark.parametrize("dims,band,extras", SHAPES)
def test_the_schur_route_in_float64_is_the_dense_inverse(instances, dims, band, extras):
    """Sigma_cc = inv(S_FF) and Sigma_pp = Cp^-1 + V^T Sigma_cc V against the blocks of the dense inverse of A_FF, within 1e-9 of max |Sigma| (measured <= 3e-13)"""
    I = instances(dims, band, extras)
    nc = 9 * I.C
    Scc, point = cm.schur_cov64(I.A, I.free, I.C)
    top = np.abs(I.Sig).max()
    e_c = np.abs(Scc - I.Sig[:nc, :nc]).max() / top
    e_p = max(np.abs(point(p) - I.Sig[nc + 3 * p:nc + 3 * p + 3, nc + 3 * p:nc + 3 * p + 3]).max() for p in range(I.P)) / top
    print("covariance float64", I.dims, "Schur route vs dense inverse: cameras", e_c, "points", e_p)
    assert e_c <= 1e-9 and e_p <= 1e-9
    assert not I.Sig[I.mask].any() and not I.Sig[:, I.mask].any()


@pytest.mark.parametrize("dims,band,extras", SHAPES)
def test_the_float32_column_mirror_converges_under_the_defaults(instances, dims, band, extras):
    """seven cameras and 21 points: every solved column converges within the default 500 iterations to rel_tol 1e-6; the error against float64 and the iterations are
    printed (the GPU bars are 4 x these, recomputed there).  Held scalars' rows and columns are exactly zero (cov_error asserts it), the blocks are symmetric bit for bit,
    the points the factor rule holds come back as NaN and are counted"""
    I = instances(dims, band, extras)
    for mode, ids in ((0, I.cams), (1, I.pts)):
        B, info = I.pcg.solve(mode, ids)
        ok = ~np.isnan(B[:, 0, 0])
        err = cm.cov_error(B[ok], I.ref(mode, ids)[ok], I.free_of(mode, ids)[ok])
        print("covariance float32 mirror", I.dims, "cameras" if mode == 0 else "points", "error", err, info)
        assert info["not_converged"] == 0 and info["iterations"] < 500 and info["worst_residual"] <= 1e-6
        assert B[ok].tobytes() == np.transpose(B[ok], (0, 2, 1)).tobytes()
        assert err < 1e-2                                  # (a sanity bound on the restatement itself, not a bar for the device)
        if mode == 1 and extras:
            und = np.array([I.und[9 * I.C + 3 * p] for p in ids])
            assert (und == ~ok).all() and info["nan_blocks"] == int(und.sum()) == 2 and np.isnan(B[~ok]).all()
        else: assert ok.all() and info["nan_blocks"] == 0
        if mode == 0: assert info["columns"] == int(I.free_of(0, ids).sum())


def test_a_camera_nothing_observes_does_not_converge_and_stays_zero(instances):
    I = instances(*SHAPES[0])
    B, info = I.pcg.solve(0, [I.C - 1], max_iterations=20)
    assert info["not_converged"] == 9 and info["columns"] == 9 and not B.any()


def test_a_column_alone_is_the_column_in_a_full_batch_bit_for_bit(instances):
    """a column's sums, freeze and updates are its own: one column of a full panel solved with the other 63 right-hand sides zero, and one camera alone against the same
    camera among seven at another place of the batch"""
    I = instances(*SHAPES[2])
    R = I.pcg.rhs(0, I.cams)
    X, info = I.pcg.solve_panel(R)
    for k in (10, 37):
        R1 = np.zeros_like(R); R1[:, :, k] = R[:, :, k]
        X1, i1 = I.pcg.solve_panel(R1)
        assert X1[:, :, k].tobytes() == X[:, :, k].tobytes() and not np.delete(X1, k, 2).any()
        assert i1["iterations"] <= info["iterations"]
    alone, _ = I.pcg.solve(0, [I.cams[3]])
    full, _ = I.pcg.solve(0, I.cams)
    assert alone[0].tobytes() == full[3].tobytes()


def test_held_scalars_and_caller_held_points(instances):
    """camera 0 (held entirely) is a zero block; camera 1 has a zero row and column 3; a point the caller holds entirely is zeros, not NaN"""
    I = instances(*SHAPES[2])
    B, _ = I.pcg.solve(0, [0, 1])
    assert not B[0].any() and not B[1][3].any() and not B[1][:, 3].any() and B[1][0, 0] > 0
    mask = I.mask.copy(); mask[9 * I.C + 3 * 5:9 * I.C + 3 * 5 + 3] = True; mask[9 * I.C + 3 * 6 + 1] = True
    _, sys = cm.system_of(I.m, mask)
    B, info = cm.ColumnPCG32.of(sys, mask).solve(1, [5, 6, 7])
    assert not B[0].any() and info["nan_blocks"] == 0
    assert not B[1][1].any() and not B[1][:, 1].any() and B[1][0, 0] > 0 and B[2].all()
    free = ~mask
    ref = cm.blocks_of(cm.dense_cov64(I.A, free), [5, 6, 7], 3, 9 * I.C)
    assert cm.cov_error(B, ref, free[9 * I.C:].reshape(-1, 3)[[5, 6, 7]]) < 1e-2


def test_the_library_declares_and_exports_the_call():
    """without the library change this fails: ThalloX_PlanCovariance is declared in include/Thallo.h and exported by libThallo.so (as tests/test_cabi.py checks every
    symbol), the kernels' entry points likewise, and ThalloSolver.covariance exists"""
    from thallo_amd.build import build_library
    build_library()
    L = thallo_amd.lib()
    names = {"Thallo.h": ["ThalloX_PlanCovariance"],
             "thallo_hip.h": ["thallo_hip_ba_cov_rhs", "thallo_hip_ba_schur_apply_s_cols", "thallo_hip_ba_cov_precond_cols", "thallo_hip_ba_cov_out", "thallo_hip_ba_cov_solve",
                              "thallo_hip_ba_cov_work_bytes"]}
    for header, want in names.items():
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        declared = set(re.findall(r"\b((?:Thallo_|ThalloX_|thallo_hip_)\w+)\s*\(", txt))
        for n in want: assert n in declared and hasattr(L, n), n
    assert callable(getattr(api.ThalloSolver, "covariance", None))
    assert {f[0] for f in api.CovarianceInfo._fields_} == {"iterations", "columns", "not_converged", "nan_blocks", "worst_residual"}
