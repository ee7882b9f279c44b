"""CPU: the float64 / float32-state restatement of the block-Jacobi loops (tests/ba_block_mirror.py) satisfies, on its own, every condition that
tests/test_gpu_block_precond.py places on the device -- so a failure there is the device's, not the algorithm's -- and records e32, the distance of the
float32 restatement of the factorisation from the float64 solve, for the kernel test's instances.

Measured here (float64 sums, float32 state; LM 5 x 150, q_tolerance 0.1, function_tolerance 0):
  (24, 300, 1200, band 12)   jacobi 4, 39, 53, 72, 62 (230)   block 3, 10, 13, 14, 12 (52)   final cost 665.047 / 665.046
  (48, 1200, 5000, band 16)  jacobi 4, 32, 50, 60, 78 (224)   block 3, 10, 14, 16, 26 (69)   final cost 3011.717 / 3011.717
  GN 4 steps on the first instance: block at 10 iterations 665.046, jacobi 679.938 at 10 and 666.917 at 25
  e32 (scaled_error of block32 against the float64 solve, blocks from the oracle's J): (5, 72, 330) 1.35e-5 with the LM shift, 1.63e-5 without;
  (3, 160, 480) 5.9e-6 / 9.5e-6.  On the device's own float32 blocks (what tests/test_gpu_block_precond.py hands the same functions): 1.02e-5 / 1.34e-5 and
  5.6e-6 / 1.27e-5, against which the device measured 9.6e-6 / 1.79e-5 and 8.0e-6 / 1.15e-5 (0.91 - 1.43 e32; the bar is 4 e32).
"""
import numpy as np
import pytest

from thallo_amd import synthetic as syn

from ba_block_mirror import BaBlockMirror, e32_of

LM = dict(q_tolerance=0.1, function_tolerance=0.0)
TABLE = [((24, 300, 1200), 12), ((48, 1200, 5000), 16)]
# The kernel test's instances.  The second is (3, 160, 480): three cameras that each see all 160 points -- 160 observations per camera, three rounds of a wave's 64
# lanes.  (3 cameras cannot give the 4 observations per point that 120 points and 480 observations would need.)
KERNEL = [((5, 72, 330), 5), ((3, 160, 480), 3)]


def instance(dims, band):
    return syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)


@pytest.fixture(scope="module")
def lm_runs():
    out = {}
    for dims, band in TABLE:
        p = instance(dims, band)
        for kind in ("jacobi", "block64", "block32"):
            m = BaBlockMirror(dims, p)
            costs, iters = m.lm_solve(5, 150, kind=kind, **LM)
            out[dims, kind] = (costs, iters, m.fallbacks)
    return out


@pytest.mark.parametrize("dims", [d for d, _ in TABLE])
@pytest.mark.parametrize("kind", ["block64", "block32"])
def test_lm_block_halves_the_iterations_and_reaches_the_same_cost(lm_runs, dims, kind):
    cj, ij, _ = lm_runs[dims, "jacobi"]
    cb, ib, fb = lm_runs[dims, kind]
    print(dims, kind, "jacobi", ij, cj, "block", ib, cb)
    assert len(ib) == 5 and len(ij) == 5
    assert sum(ib) <= 0.5 * sum(ij), (ib, ij)
    assert cb[-1] <= cj[-1] * (1 + 1e-4), (cb, cj)
    assert fb == 0


@pytest.mark.parametrize("dims", [d for d, _ in TABLE])
def test_lm_float32_factorisation_runs_the_float64_trajectory(lm_runs, dims):
    """the float32 Cholesky of the scaled blocks: the same iteration counts, the same costs to float32 accuracy"""
    c64, i64, _ = lm_runs[dims, "block64"]
    c32, i32, _ = lm_runs[dims, "block32"]
    assert sum(abs(a - b) for a, b in zip(i64, i32)) <= 1, (i64, i32)
    assert np.allclose(c64, c32, rtol=1e-5), (c64, c32)


def test_gn_block_at_10_beats_jacobi_at_25():
    dims, band = TABLE[0]
    p = instance(dims, band)
    blk = BaBlockMirror(dims, p).gn_solve(4, 10, "block32")
    j10 = BaBlockMirror(dims, p).gn_solve(4, 10, "jacobi")
    j25 = BaBlockMirror(dims, p).gn_solve(4, 25, "jacobi")
    print("block32 4x10", blk, "jacobi 4x10", j10, "jacobi 4x25", j25)
    assert blk[-1] < j25[-1] < j10[-1]


@pytest.mark.parametrize("dims,band", KERNEL)
@pytest.mark.parametrize("shifted", [True, False])
def test_e32_of_the_kernel_tests_instances(dims, band, shifted):
    """e32 is a float32 rounding error of a system whose condition number the scaling keeps <= ~1e3: far below 1e-3, well above 2^-24"""
    m = BaBlockMirror(dims, instance(dims, band))
    Hs, CtC, pre_lm, pre_gn, r = m.first_step()
    e32, z64 = e32_of(Hs, CtC if shifted else None, pre_lm if shifted else pre_gn, r, dims[0])
    print("e32", dims, "shift" if shifted else "no shift", e32)
    assert np.isfinite(z64).all()
    assert 2.0 ** -24 < e32 < 1e-3
