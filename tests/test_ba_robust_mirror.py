"""CPU: bundle adjustment with a robust loss (tests/ba_robust_mirror.py) -- the losses' derivatives, the gradient of the reweighted system, the squared loss as the
limit of Huber, what the losses do to a contaminated instance, and that every configuration (with a mask and without) lowers the robust cost.  These are the mirrors that
tests/test_gpu_ba_robust.py compares the device with.

The contaminated instances: ba_robust_mirror.contaminate -- 5 % of the observations displaced by 30 - 150 px."""
import numpy as np
import pytest

from thallo_amd import synthetic as syn

from ba_block_mirror import BaBlockMirror
from ba_held_mirror import CONFIGS, masks
from ba_robust_mirror import KINDS, contaminate, cost64, inlier_rms, rho, robust, robust_mirror

LM = dict(q_tolerance=0.1, function_tolerance=0.0)
TABLE = [((24, 300, 1200), 12)]
KERNEL = [((5, 72, 330), 5), ((3, 160, 480), 3)]
SCALE = 2.0

_instances = {}


def instance(dims, band):
    """(contaminated params, outlier mask), computed once per shape and never written"""
    if dims not in _instances:
        _instances[dims] = contaminate(syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band))
    return _instances[dims]


@pytest.mark.parametrize("kind", KINDS)
def test_rho_prime_is_the_derivative_of_rho(kind):
    """rho' against central differences of rho, 1e-6 relative: at s = 0 (one-sided there is nothing to the left: the difference is taken over [0, 2 h] around h, and rho' at
    0 is compared with it to the same bar, both losses being C^1 with rho'' bounded by 1 / a^2), on both sides of Huber's s = a^2, and far out"""
    a = SCALE
    for s in (0.0, 1e-3, 0.5 * a * a, a * a * (1 - 1e-3), a * a * (1 + 1e-3), 3.0 * a * a, 40.0, 2500.0, 1e5):
        h = 1e-6 * max(s, 1.0) if s > 0 else 1e-7
        c = s if s > 0 else h
        fd = (rho(kind, a, c + h)[0] - rho(kind, a, c - h)[0]) / (2 * h)
        got = float(rho(kind, a, s)[1])
        print("rho'", kind, s, got, fd, abs(got - fd) / abs(fd))
        assert abs(got - fd) <= 1e-6 * abs(fd)
    v, d = rho(kind, a, np.array([0.0, a * a, 1e30]))
    assert v[0] == 0.0 and d[0] == 1.0 and np.isfinite(v).all() and (d > 0).all() and (d <= 1).all()


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_of_the_reweighted_system_is_the_gradient_of_the_robust_cost(kind):
    """-J_s^T F_s (the mirror's r: the oracle's float32 J and residuals, w in float32) against central differences of the float64 robust cost over every unknown of the
    contaminated (5, 72, 330) instance: max |r - (-grad)| <= 1e-3 max |grad| (what is left is the oracle's float32 J; no rho'' term enters a gradient)"""
    dims, band = KERNEL[0]
    p, _ = instance(dims, band)
    m = robust(BaBlockMirror)(kind, SCALE, dims, p)
    r = m.linearise()[1].astype(np.float64)
    x0 = np.concatenate([p[0].ravel(), p[1].ravel()]).astype(np.float64)
    g = np.empty(len(x0))
    for i in range(len(x0)):
        h = 1e-6 * max(abs(x0[i]), 1.0)
        xp, xm = x0.copy(), x0.copy(); xp[i] += h; xm[i] -= h
        g[i] = (cost64(kind, SCALE, p, xp) - cost64(kind, SCALE, p, xm)) / (2 * h)
    err = np.abs(r + g).max() / np.abs(g).max()
    print("gradient", kind, "err", err)
    assert err <= 1e-3


def test_huber_with_a_huge_scale_is_the_plain_mirror():
    """scale 1e18: every w is exactly 1 and rho = s -- costs and iteration counts of LM 3 x 15 equal the plain mirror's exactly"""
    dims, band = TABLE[0]
    p, _ = instance(dims, band)
    plain = BaBlockMirror(dims, p).lm_solve(3, 15, kind="jacobi", **LM)
    hub = robust(BaBlockMirror)("huber", 1e18, dims, p).lm_solve(3, 15, kind="jacobi", **LM)
    print("huber 1e18", hub, "plain", plain)
    assert hub[0] == plain[0] and hub[1] == plain[1]


_long = {}


def long_solve(kind):
    """LM 8 x 50, q_tolerance 0.001, point Jacobi on the contaminated (24, 300, 1200) instance -> (costs, inlier RMS at the start, at the end); once per loss"""
    if kind not in _long:
        dims, band = TABLE[0]
        p, out = instance(dims, band)
        m = BaBlockMirror(dims, p) if kind == "trivial" else robust(BaBlockMirror)(kind, SCALE, dims, p)
        start = inlier_rms(m, out)
        costs, _ = m.lm_solve(8, 50, kind="jacobi", q_tolerance=0.001)
        _long[kind] = (costs, start, inlier_rms(m, out))
    return _long[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_a_robust_loss_keeps_the_outliers_from_steering_the_solve(kind):
    """5 % outliers, LM 8 x 50: the squared loss drags the inliers' RMS reprojection error from 2.5 px to above 10; under Huber(2) and Cauchy(2) it ends below where it
    started and below half of the squared loss's, and the robust cost never rises"""
    costs, start, end = long_solve(kind)
    _, _, plain_end = long_solve("trivial")
    print("inlier RMS", kind, "start", start, "end", end, "squared loss", plain_end, "costs", costs)
    assert end < start
    assert end < 0.5 * plain_end
    assert all(b <= a for a, b in zip(costs, costs[1:]))


@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("dims,band", KERNEL + TABLE)
def test_every_configuration_lowers_the_robust_cost_at_every_step(dims, band, config, kind, lm):
    """GN 3 x 10 and LM 3 x 15 (q_tolerance 0.1, function_tolerance 0) on the contaminated instances"""
    p, _ = instance(dims, band)
    m, k = robust_mirror(config, kind, SCALE, dims, p)
    costs = m.lm_solve(3, 15, kind=k, **LM)[0] if lm else m.gn_solve(3, 10, k)
    print("robust mirror", dims, config, kind, "LM" if lm else "GN", costs)
    assert len(costs) == 4 and all(b < a for a, b in zip(costs, costs[1:]))


@pytest.mark.parametrize("which", ["two_cameras", "intrinsics"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("config", CONFIGS)
def test_the_robust_mirrors_compose_with_masks(config, kind, which):
    """a loss and held unknowns together (GN 3 x 10, the (24, 300, 1200) instance): the held scalars keep their bits, the free ones move, the robust cost goes down"""
    dims, band = TABLE[0]
    p, _ = instance(dims, band)
    mask = masks(dims[0], dims[1])[which]
    before = np.concatenate([p[0].ravel(), p[1].ravel()])
    m, k = robust_mirror(config, kind, SCALE, dims, p, mask)
    costs = m.gn_solve(3, 10, k)
    after = np.concatenate([m.params[0].ravel(), m.params[1].ravel()])
    print("robust + held mirror", config, kind, which, costs)
    assert after[mask].tobytes() == before[mask].tobytes() and (after[~mask] != before[~mask]).any()
    assert all(b < a for a, b in zip(costs, costs[1:]))
