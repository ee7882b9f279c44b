"""CPU: bundle adjustment with unknowns held fixed (tests/ba_held_mirror.py) -- the one rule "every product with M^-1 or Cp^-1 has a zero row and column at a held scalar"
solves the problem in the free unknowns, in float64 exactly and in the float32 mirrors that tests/test_gpu_ba_held.py compares the device with.

Masks throughout (ba_held_mirror.masks): cameras {0, 1} fully held; components 6-8 of every camera; three points fully held and one point with one coordinate held; all
points (motion-only); all cameras (structure-only)."""
import numpy as np
import pytest

from thallo_amd import synthetic as syn

from ba_block_mirror import BaBlockMirror, BlockPrecond, e32_of, guarded_invert
from ba_held_mirror import CONFIGS, HeldBlockMirror, held_mirror, held_solve64, hold_blocks, masks, split
from ba_schur_mirror import BaSchurMirror

LM = dict(q_tolerance=0.1, function_tolerance=0.0)
TABLE = [((24, 300, 1200), 12), ((48, 1200, 5000), 16)]
KERNEL = [((5, 72, 330), 5), ((3, 160, 480), 3)]
MASKS = ("two_cameras", "intrinsics", "control_points", "all_points", "all_cameras")


def instance(dims, band):
    return syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)


_systems = {}


def first_lm_system(dims, band):
    """(A dense float64, b, the direct solves by mask) of the first LM step, computed once per shape"""
    if dims not in _systems:
        A, b = BaSchurMirror(dims, instance(dims, band)).first_lm_system()
        _systems[dims] = (np.asarray(A.todense()), b, {})
    return _systems[dims]


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("dims,band", KERNEL + [TABLE[0]])
def test_float64_masked_solve_is_the_solve_on_the_free_set(dims, band, config, which):
    """float64 PCG on complete vectors with the masked M^-1 (or the masked elimination and PCG on the cameras), converged, against np.linalg.solve(A_FF, b_F) of the first
    LM system: delta_F within 1e-9 of max |delta|, delta_H = 0 exactly."""
    A, b, direct = first_lm_system(dims, band)
    mask = masks(dims[0], dims[1])[which]
    if which not in direct: direct[which] = np.linalg.solve(A[~mask][:, ~mask], b[~mask])
    want = direct[which]
    got = held_solve64(A, b, mask, dims[0], config)
    err = np.abs(got[~mask] - want).max() / np.abs(want).max()
    print("held float64", dims, config, which, "held", int(mask.sum()), "err", err)
    assert not got[mask].any()
    assert err <= 1e-9


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("lm", [False, True])
def test_float32_mirrors_hold_the_bits_and_lower_the_cost(which, lm):
    """GN 3 x 10 and LM 3 x 50 on the (24, 300, 1200) instance, the four configurations: the held parameters keep their bits, the free ones move, the cost falls, and the
    two Schur mirrors (matrix-free and assembled) take equal iteration counts."""
    dims, band = TABLE[0]
    p = instance(dims, band)
    mask = masks(dims[0], dims[1])[which]
    before = np.concatenate([p[0].ravel(), p[1].ravel()])
    iters = {}
    for config in CONFIGS:
        m, kind = held_mirror(config, dims, p, mask)
        if lm: costs, iters[config] = m.lm_solve(3, 50, kind=kind, **LM)
        else: costs = m.gn_solve(3, 10, kind)
        after = np.concatenate([m.params[0].ravel(), m.params[1].ravel()])
        print("held mirror", "LM" if lm else "GN", which, config, costs, iters.get(config))
        assert after[mask].tobytes() == before[mask].tobytes()
        assert (after[~mask] != before[~mask]).any()
        assert costs[-1] < costs[0]
    if lm: assert iters["schur"] == iters["schur_explicit"]


class _KeepsDelta(HeldBlockMirror):
    """... and keeps the step's delta itself (the unknowns after the step hold it rounded to their own magnitude)"""

    def _update(self, delta):
        self.delta = delta.astype(np.float64)
        super()._update(delta)


def _first_gn_delta(dims, p, mask, L):
    m = _KeepsDelta(dims, p, mask)
    m.gn_step(L, "block32")
    return m.delta


@pytest.mark.parametrize("which", ["all_points", "all_cameras"])
def test_motion_only_and_structure_only_converge_in_one_block_iteration(which):
    """With all points (all cameras) held A_FF is block diagonal and the block preconditioner is its inverse: delta after lIterations = 1 is delta after 5.  Bar: the block
    apply's own float32 error -- e32 of tests/test_gpu_block_precond.py's rule (the float32 restatement against the float64 solve, in the factorisation's coordinates), four
    of them, per block in the same coordinates u = delta / s; one iteration differs from five only by what that apply leaves in the residual."""
    dims, band = KERNEL[0]
    p = instance(dims, band)
    mask = masks(dims[0], dims[1])[which]
    d1, d5 = _first_gn_delta(dims, p, mask, 1), _first_gn_delta(dims, p, mask, 5)
    J, r, d, Hs = BaBlockMirror(dims, p).linearise()
    mc, mp = split(mask, dims[0])
    Hh = (hold_blocks(Hs[0], mc), hold_blocks(Hs[1], mp))
    pre = np.where(mask, np.float32(0), guarded_invert(d))
    e32, _ = e32_of(Hh, None, pre, np.where(mask, np.float32(0), r), dims[0])
    dd = np.concatenate([np.einsum("bii->bi", Hh[0]).ravel(), np.einsum("bii->bi", Hh[1]).ravel()])
    s = 1.0 / np.sqrt(dd)
    worst = 0.0
    for lo, hi, n in ((0, 9 * dims[0], 9), (9 * dims[0], len(d1), 3)):
        e = (np.abs(d1 - d5) / s)[lo:hi].reshape(-1, n).max(1); u = (np.abs(d5) / s)[lo:hi].reshape(-1, n).max(1)
        if (u > 0).any(): worst = max(worst, float((e[u > 0] / u[u > 0]).max()))
    print("one iteration against five", which, "e32", e32, "worst", worst)
    assert not d1[mask].any() and not d5[mask].any() and d5[~mask].any()
    assert worst <= 4 * e32
