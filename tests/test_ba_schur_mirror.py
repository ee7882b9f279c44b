"""CPU: the restatement of the Schur-complement solve (tests/ba_schur_mirror.py) is the full system's solve, and satisfies on its own the comparative conditions that
tests/test_gpu_ba_schur.py places on the device -- so a failure there is the device's, not the algorithm's.

Measured here (float64 sums, float32 state; LM 5 x 150, q_tolerance 0.1, function_tolerance 0; iterations per step, total, final cost):
  see the table printed by test_lm_schur_needs_fewer_iterations_than_block_jacobi (recorded in profiles/ba_schur/README.md)."""
import numpy as np
import pytest

from thallo_amd import synthetic as syn

from ba_block_mirror import BaBlockMirror
from ba_schur_mirror import BaSchurMirror, Schur64, SchurKernels32, SchurLists, dense_j, dense_reduced_solve, rel_max, with_extras

LM = dict(q_tolerance=0.1, function_tolerance=0.0)
TABLE = [((24, 300, 1200), 12), ((48, 1200, 5000), 16)]
KERNEL = [((5, 72, 330), 5), ((3, 160, 480), 3)]


def instance(dims, band):
    return syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)


@pytest.mark.parametrize("dims,band", KERNEL + TABLE)
def test_float64_reduced_solve_is_the_full_solve(dims, band):
    """dense S, g and the back-substitution in float64 against the float64 solve of A delta = b of the first LM step (A = J^T J + diag(CtC)): <= 1e-9 of max |delta|"""
    A, b = BaSchurMirror(dims, instance(dims, band)).first_lm_system()
    full = np.linalg.solve(np.asarray(A.todense()), b)
    red, S, g = dense_reduced_solve(A, b, 9 * dims[0])
    err = np.abs(red - full).max() / np.abs(full).max()
    print("reduced vs full", dims, err)
    assert np.linalg.eigvalsh(S).min() > 0
    assert err <= 1e-9


@pytest.mark.parametrize("dims,band", TABLE)
def test_lm_schur_needs_fewer_iterations_than_block_jacobi(dims, band):
    p = instance(dims, band)
    m = BaSchurMirror(dims, p)
    cs, is_ = m.lm_solve(5, 150, **LM)
    cb, ib = BaBlockMirror(dims, p).lm_solve(5, 150, kind="block32", **LM)
    print("LM", dims, "schur", is_, sum(is_), cs, "block32", ib, sum(ib), cb)
    assert len(is_) == 5 and m.held == [0] * 5 and m.fallbacks == 0
    assert sum(is_) < sum(ib), (is_, ib)
    assert abs(cs[-1] - cb[-1]) <= 1e-4 * cb[-1], (cs, cb)


def test_gn_schur_is_below_block_jacobi_after_every_step():
    dims, band = TABLE[0]
    p = instance(dims, band)
    cs = BaSchurMirror(dims, p).gn_solve(4, 10)
    cb = BaBlockMirror(dims, p).gn_solve(4, 10, "block32")
    print("GN 4x10", "schur", cs, "block32", cb)
    assert all(a < b for a, b in zip(cs[1:], cb[1:])), (cs, cb)


@pytest.mark.parametrize("dims,band", KERNEL)
def test_a_point_observed_once_is_held_in_gn_and_left_bit_unchanged(dims, band):
    """its 3 x 3 block J_p^T J_p has rank 2: the third squared pivot of the scaled block is rounding noise, far below 2^-16.  The point nothing observes has B_ii = 0.  Both are
    held: delta_p = 0 exactly.  With the LM shift every block is positive definite and nothing is held."""
    q, d = with_extras(instance(dims, band))
    m = BaSchurMirror(d, q)
    before = m.params[1].copy()
    c0 = float(m.cost())
    m.gn_step(10)
    assert m.held == [2]
    assert m.params[1][-2:].tobytes() == before[-2:].tobytes()
    assert (m.params[1][:-2] != before[:-2]).any() and float(m.cost()) < c0
    m2 = BaSchurMirror(d, q)
    m2.lm_solve(1, 10, **LM)
    assert m2.held == [0]


@pytest.mark.parametrize("dims,band", KERNEL)
@pytest.mark.parametrize("renumber", [False, True])
@pytest.mark.parametrize("shifted", [False, True])
def test_e32_of_the_kernel_tests_operations(orc, dims, band, renumber, shifted):
    """the two sides of tests/test_gpu_ba_schur.py's kernel tests on the oracle's J in place of the device's Jb: the float32 restatement in the kernels' order against the dense
    float64 forms.  e32 of g and S x is a float32 rounding error (the issue: 4e-8 ... 1.1e-7 of max |S x|); the back-substitution's is larger with the LM shift, where the point
    observed once is solved for through a block whose third scaled pivot is ~1e-4."""
    p, d = with_extras(instance(dims, band))
    rp, col, val, res = orc.Problem(orc.BUNDLE_ADJUST, d, p).csr()
    L = SchurLists(p[3], p[4], d[0], d[1], renumber)
    rows = val.reshape(-1, 12)
    Jb = np.concatenate([rows[0::2], rows[1::2]], 1)[L.cam_obs]
    J = dense_j(Jb.astype(np.float64), L)
    b = (-(J.T @ np.stack([res[0::2], res[1::2]], 1)[L.cam_obs].ravel().astype(np.float64))).astype(np.float32)
    CtC = BaSchurMirror(d, p).first_step()[1]
    CtC = np.concatenate([CtC[:9 * d[0]], CtC[9 * d[0]:].reshape(-1, 3)[L.new2old].ravel()])
    shift = CtC if shifted else None
    K = SchurKernels32(Jb, L, shift, b)
    R = Schur64(J, shift, b, K.held, d[0])
    x = np.random.default_rng(3).standard_normal(9 * d[0]).astype(np.float32)
    e = (rel_max(K.reduce(), R.g), rel_max(K.apply(x), R.apply(x)), rel_max(K.back(x), R.back(x)))
    print("e32", dims, renumber, shifted, "held", int(K.held.sum()), e)
    assert int(K.held.sum()) == (0 if shifted else 2)
    assert 2.0 ** -26 < e[0] < 1e-5 and 2.0 ** -26 < e[1] < 1e-5 and 2.0 ** -26 < e[2] < 1e-2
