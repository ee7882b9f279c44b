"""CPU: bundle adjustment with Gaussian priors on single unknowns (tests/ba_prior_mirror.py; thallo_amd/csrc/prior.hip, ThalloX_PlanSetPrior) -- the semantics in float64,
the gradient, what a prior at the current unknowns changes, LM's monotone costs, the soft gauge of the dense factor, and the interface.  These are the mirrors that
tests/test_gpu_ba_prior.py compares the device with.

The priors (priors_of): components 6-8 of every camera at sigma = 10 % of |value| + 1e-3 with the mean 2 % off the value; three control points at sigma = 0.01 with the
mean 0.05 away; and the soft gauge -- camera 0's six pose scalars and scalar 3 of camera 1 at their values.  The gauge's weight is SOFT_GAUGE_REL = 1e-3 of the largest of
the seven diagonal entries of the reduced camera matrix S: small against the data's own curvature (it moves no well-determined direction by more than 1e-3 of a sigma),
large against float32's resolution of S (2^-24 ~ 6e-8 of a diagonal entry), which is what a factor needs to see the gauge directions as definite.  The values it gives
are written next to test_the_soft_gauge_makes_the_dense_mirror_factor."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import thallo_amd
from thallo_amd import api, synthetic as syn

import ba_reference as br
from ba_block_mirror import BaBlockMirror, guarded_invert
from ba_held_mirror import held_solve64, masked_inverse64, masks, pcg64, split
from ba_prior_mirror import (CONFIGS, prior, prior_cost32, prior_cost64, prior_init32, prior_lm_shift32, prior_mirror, prior_system64, soft_gauge, workgroup_partials)
from ba_robust_mirror import cost64
from ba_schur_dense_mirror import BaSchurDenseMirror, gn_system
from ba_schur_mirror import block_diag3, dense_reduced_solve
from ba_two_level_mirror import default_k, prolongation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24
SHAPES = [((5, 72, 330), 5), ((24, 300, 1200), 12)]
LM = dict(q_tolerance=0.1, function_tolerance=0.0)
SOFT_GAUGE_REL = 1e-3


def gamma(k): return k * U / (1 - k * U)


def instance(dims, band):
    return syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)


def flat(p):
    return np.concatenate([p[0].ravel(), p[1].ravel()]).astype(F)


def s_diag(dims, p):
    """the diagonal of the reduced camera matrix of the instance's GN system, float64 from the mirror's own float32 S"""
    J, sys = gn_system(BaSchurDenseMirror(dims, p))
    return np.asarray(sys.st.bsr(sys.S).diagonal(), np.float64)


def priors_of(dims, p, gauge=True):
    """-> (mean, weight) flat float32 over [cameras | points], the caller's ids"""
    C, P = dims[0], dims[1]
    x = flat(p)
    w = soft_gauge(C, P, s_diag(dims, p), SOFT_GAUGE_REL) if gauge else np.zeros(len(x), F)
    mu = x.copy()
    cam_w, cam_mu = w[:9 * C].reshape(C, 9), mu[:9 * C].reshape(C, 9)
    v = x[:9 * C].reshape(C, 9)[:, 6:9]
    cam_w[:, 6:9] = (1.0 / (0.1 * np.abs(v.astype(np.float64)) + 1e-3) ** 2).astype(F)
    cam_mu[:, 6:9] = (1.02 * v).astype(F)
    pt_w, pt_mu = w[9 * C:].reshape(P, 3), mu[9 * C:].reshape(P, 3)
    for j in (1, P // 2, P - 2):
        pt_w[j] = F(1e4); pt_mu[j] = (x[9 * C:].reshape(P, 3)[j] + F(0.05)).astype(F)
    return mu, w


_cache = {}


def reference_system(dims, band):
    """(A0 = J^T J dense float64, J, F, x) from tests/ba_reference.py's float64 residual and Jacobian, once per shape"""
    if dims not in _cache:
        p = instance(dims, band)
        C, P, O = dims
        Fr, Jr = br.residual_and_jacobian(p[0], p[1], p[2], p[3], p[4])
        cols = np.concatenate([9 * p[3][:, None] + np.arange(9), 9 * C + 3 * p[4][:, None] + np.arange(3)], 1)
        rows = np.repeat(np.arange(2 * O), 12)
        J = sp.csr_matrix((Jr.reshape(-1), (rows, np.repeat(cols, 2, axis=0).reshape(-1))), shape=(2 * O, 9 * C + 3 * P))
        _cache[dims] = (p, J, Fr.reshape(-1), flat(p).astype(np.float64), priors_of(dims, p))
    return _cache[dims]


def two_level_solve64(A, b, mask, C, iters=20000):
    """float64: the points eliminated through the masked Cp^-1, PCG on the cameras with M^-1 = the masked camera blocks' inverses + P (P^T S P)^-1 P^T"""
    nc = 9 * C; P = (len(b) - nc) // 3
    mc, mp = split(mask, C)
    Hc = np.stack([A[9 * c:9 * c + 9, 9 * c:9 * c + 9] for c in range(C)]); Hp = np.stack([A[nc + 3 * j:nc + 3 * j + 3, nc + 3 * j:nc + 3 * j + 3] for j in range(P)])
    Mc, Mp = masked_inverse64(Hc, mc), masked_inverse64(Hp, mp)
    Ci = np.asarray(block_diag3(Mp).todense())
    B, E = A[:nc, :nc], A[:nc, nc:]
    S = B - E @ Ci @ E.T; g = b[:nc] - E @ (Ci @ b[nc:])
    Pm = np.asarray(prolongation(np.arange(C) // default_k(C), mc).todense())
    Sc = Pm.T @ S @ Pm
    dead = np.diag(Sc) == 0
    Sc[dead, dead] = 1.0
    Zc = np.linalg.inv(Sc); Zc[dead] = 0; Zc[:, dead] = 0
    Minv = lambda r: np.einsum("bij,bj->bi", Mc, r.reshape(-1, 9)).ravel() + Pm @ (Zc @ (Pm.T @ r))
    dc = pcg64(lambda x: S @ x, g, Minv, iters)
    return np.concatenate([dc, Ci @ (b[nc:] - E.T @ dc)])


def dense_solve64(A, b, mask, C):
    """float64: the dense form -- the reduced system of the free set solved directly, zeros at the held scalars"""
    free = ~mask
    nfc = int(free[:9 * C].sum())
    out = np.zeros(len(b))
    out[free] = dense_reduced_solve(A[free][:, free], b[free], nfc)[0] if nfc else np.linalg.solve(A[free][:, free], b[free])
    return out


@pytest.mark.parametrize("which", [None, "two_cameras", "intrinsics"])
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("dims,band", SHAPES)
def test_float64_solve_is_the_solve_of_the_energy_with_the_prior_rows(dims, band, config, which):
    """A = J^T J + W, b = -J^T F - W (x - mu) (ba_prior_mirror.prior_system64; J and F from tests/ba_reference.py) solved in float64 by each configuration's mechanism on
    complete vectors -- PCG with the point-Jacobi or block M^-1, the points eliminated and PCG on the cameras (matrix-free and assembled are one matrix in float64), the
    dense reduced solve, the two-level M^-1 -- against np.linalg.solve(A_FF, b_F) of the normal equations of the stacked residuals [F; sqrt(w) (x - mu)] built
    independently: within 1e-9 of max |delta|, delta_H = 0 exactly.  Without a mask the priors' soft gauge alone makes A definite."""
    p, J, Fr, x, (mu, w) = reference_system(dims, band)
    C = dims[0]
    A, b = prior_system64(J, Fr, w, mu, x)
    on = np.nonzero(w > 0)[0]
    Js = sp.vstack([J, sp.csr_matrix((np.sqrt(w[on].astype(np.float64)), (np.arange(len(on)), on)), shape=(len(on), len(x)))]).toarray()
    Fs = np.concatenate([Fr, np.sqrt(w[on].astype(np.float64)) * (x[on] - mu[on].astype(np.float64))])
    mask = np.zeros(len(x), bool) if which is None else masks(dims[0], dims[1])[which]
    want = np.linalg.solve((Js.T @ Js)[~mask][:, ~mask], -(Js.T @ Fs)[~mask])
    if config in ("jacobi", "block", "schur", "schur_explicit"): got = held_solve64(A, b, mask, C, config)
    elif config == "schur_dense": got = dense_solve64(A, b, mask, C)
    else: got = two_level_solve64(A, b, mask, C)
    err = np.abs(got[~mask] - want).max() / np.abs(want).max()
    print("prior float64", dims, config, which, "priors", int((w > 0).sum()), "err", err)
    assert not got[mask].any()
    assert err <= 1e-9


def test_gradient_of_the_full_cost_is_minus_b():
    """b of the mirror (the oracle's float32 J and residuals, the prior's term in float32) against central differences of the float64 full cost -- reprojection + prior --
    over every unknown of the (5, 72, 330) instance at a random x near the instance's: max |b + grad| <= 1e-3 max |grad| (tests/test_ba_robust_mirror.py's bar: what is
    left is the oracle's float32 J)"""
    dims, band = SHAPES[0]
    p = instance(dims, band)
    mu, w = priors_of(dims, p)
    rng = np.random.default_rng(3)
    q = [a.copy() for a in p]
    q[0] = (q[0] * (1 + 1e-3 * rng.standard_normal(q[0].shape))).astype(F); q[1] = (q[1] + 1e-3 * rng.standard_normal(q[1].shape)).astype(F)
    m = prior(BaBlockMirror)(mu, w, dims, q)
    b = m.linearise()[1].astype(np.float64)
    x0 = flat(q).astype(np.float64)
    full = lambda x: cost64("trivial", 1.0, q, x) + prior_cost64(w, mu, x)
    g = np.empty(len(x0))
    for i in range(len(x0)):
        h = 1e-6 * max(abs(x0[i]), 1.0)
        xp, xm = x0.copy(), x0.copy(); xp[i] += h; xm[i] -= h
        g[i] = (full(xp) - full(xm)) / (2 * h)
    err = np.abs(b + g).max() / np.abs(g).max()
    plain = BaBlockMirror(dims, q).linearise()[1].astype(np.float64)
    print("gradient with priors", "err", err, "the prior's share of |b|", np.abs(b - plain).max() / np.abs(b).max())
    assert np.abs(b - plain).max() > 1e-3 * np.abs(b).max()      # (the priors are felt)
    assert err <= 1e-3


def test_a_prior_at_the_current_unknowns_changes_no_b_and_shifts_the_diagonal():
    """weight w on every scalar with mu = x: b keeps its bits, the diagonal is float32(d + w), every block's diagonal too, the cost gains nothing"""
    dims, band = SHAPES[0]
    p = instance(dims, band)
    x = flat(p)
    wv = F(3.5)
    a = BaBlockMirror(dims, p); m = prior(BaBlockMirror)(x, np.full(len(x), wv, F), dims, p)
    Ja, ra, da, Ha = a.linearise(); Jm, rm, dm, Hm = m.linearise()
    assert rm.tobytes() == ra.tobytes()
    assert dm.tobytes() == (da + wv).astype(F).tobytes()
    for X, Y in zip(Ha, Hm):
        i = np.arange(X.shape[1])
        assert np.array_equal(Y[:, i, i], (X[:, i, i].astype(F) + wv).astype(F).astype(np.float64))
        off = ~np.eye(X.shape[1], dtype=bool)
        assert np.array_equal(X[:, off], Y[:, off])
    v = np.random.default_rng(0).standard_normal(len(x))
    assert np.allclose(Jm.T @ (Jm @ v), Ja.T @ (Ja @ v) + float(wv) * v, rtol=1e-12, atol=0)
    assert float(m.cost()) == float(a.cost()) and m.prior_cost() == 0.0


def test_the_float32_restatements_of_the_three_kernels_against_float64():
    """prior_cost32, prior_init32 and prior_lm_shift32 (what tests/test_gpu_ba_prior.py holds the device's launches against bit-adjacent) on random data, n = 261 and
    70000 (more than one grid stride of the cost launch): the cost within gamma_{m+2} sum |terms| per partial's m terms (summed: of the whole), r and diag within 2 u and
    1 u of their float64 values, the shift plane bit for bit"""
    rng = np.random.default_rng(11)
    for n in (261, 70000):
        w = np.where(rng.random(n) < 0.6, rng.uniform(0.1, 50.0, n), 0.0).astype(F); mu = rng.standard_normal(n).astype(F); x = (mu + 10 * rng.standard_normal(n)).astype(F)
        r, d = rng.standard_normal(n).astype(F), rng.uniform(0.0, 100.0, n).astype(F)
        part = prior_cost32(w, mu, x)
        terms = 0.5 * w.astype(np.float64) * (x.astype(np.float64) - mu) ** 2
        m = -(-n // (256 * len(part))) + 6 + 4
        err = abs(part.astype(np.float64).sum() - terms.sum())
        print("prior_cost32", n, "partials", len(part), "err / bar", err / ((gamma(m + 2) + 3 * U) * terms.sum()))
        assert err <= (gamma(m + 2) + 3 * U) * terms.sum()
        r2, d2, pre, z, rz = prior_init32(w, mu, x, r, d, guarded_invert(d), (guarded_invert(d) * r).astype(F))
        on = w > 0
        r64 = r.astype(np.float64) - w.astype(np.float64) * (x.astype(np.float64) - mu)
        mag = np.abs(r) + np.abs(w.astype(np.float64) * (x.astype(np.float64) - mu))
        assert (np.abs(r2 - r64)[on] <= 3 * U * mag[on]).all() and r2[~on].tobytes() == r[~on].tobytes()
        assert (np.abs(d2 - (d.astype(np.float64) + w))[on] <= U * (d + w)[on]).all() and d2[~on].tobytes() == d[~on].tobytes()
        assert pre.tobytes() == guarded_invert(d2).tobytes() and z.tobytes() == (pre * r2).astype(F).tobytes()
        assert prior_lm_shift32(w, d).tobytes() == (d + w).astype(F).tobytes()
    assert workgroup_partials(np.ones(1, F), 1).tolist() == [1.0]


@pytest.mark.parametrize("config", CONFIGS)
def test_lm_costs_are_monotone_with_priors_on_the_intrinsics(config):
    """LM 6 x 50 on the (24, 300, 1200) instance with priors on components 6-8 of every camera (no other prior, no mask): the full cost never rises, and ends below its start"""
    dims, band = SHAPES[1]
    p = instance(dims, band)
    mu, w = priors_of(dims, p, gauge=False)
    w[9 * dims[0]:] = 0
    m, kind = prior_mirror(config, mu, w, dims, p)
    costs, iters = m.lm_solve(6, 50, kind=kind, **LM)
    print("LM with priors on the intrinsics", config, costs, iters, "prior's share at the end", m.prior_cost())
    assert all(b <= a for a, b in zip(costs, costs[1:])) and costs[-1] < costs[0]


@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("config", CONFIGS)
def test_the_prior_mirrors_compose_with_a_mask_and_a_loss(config, lm):
    """Huber(2) and cameras {0, 1} held together with the priors, GN 3 x 10 and LM 3 x 15: the held bits stay, the cost falls at every step"""
    dims, band = SHAPES[1]
    p = instance(dims, band)
    mu, w = priors_of(dims, p)
    mask = masks(dims[0], dims[1])["two_cameras"]
    m, kind = prior_mirror(config, mu, w, dims, p, mask=mask, loss=("huber", 2.0))
    costs = m.lm_solve(3, 15, kind=kind, **LM)[0] if lm else m.gn_solve(3, 10, kind)
    after = flat(m.params)
    print("prior + mask + loss", config, "LM" if lm else "GN", costs)
    assert after[mask].tobytes() == flat(p)[mask].tobytes()
    assert len(costs) == 4 and all(b < a for a, b in zip(costs, costs[1:]))


def test_the_soft_gauge_makes_the_dense_mirror_factor():
    """GN without a held scalar on the 6-camera instance (the covariance tests' (5, 72, 330) with its extras): the dense mirror's float32 factor fails at a pivot; with
    the soft gauge -- camera 0's six pose scalars and scalar 3 of camera 1 at weight SOFT_GAUGE_REL x the largest of their seven diagonal entries of S -- it factors (the camera nothing observes keeps the identity's
    rows, as with a held gauge) and the steps lower the cost.  The chosen values (printed): weight 1e-3 max_i S_ii over the seven scalars."""
    inst = cm_instance()
    dims, p = inst
    C, P = dims[0], dims[1]
    free = BaSchurDenseMirror(dims, p)
    assert not free.gn_step() and free.pivot is not None
    mu, w = gauge_priors(dims, p)
    m = prior(BaSchurDenseMirror)(mu, w, dims, p)
    costs = m.gn_solve(2)
    print("soft gauge", dims, "weight", float(w[0]), "of max S_ii", float(w[0]) / SOFT_GAUGE_REL, "costs", costs, "pivot", m.pivot)
    assert m.pivot is None and len(costs) == 3 and costs[1] < costs[0]


def cm_instance():
    from ba_schur_mirror import with_extras
    dims, band = SHAPES[0]
    p, d3 = with_extras(instance(dims, band))
    return d3, p


def gauge_priors(dims, p):
    """the soft gauge alone, at the current unknowns"""
    C, P = dims[0], dims[1]
    d = s_diag(dims, p)
    return flat(p), soft_gauge(C, P, d, SOFT_GAUGE_REL)


def test_the_library_declares_and_exports_the_calls():
    """without the library change this fails: the three calls are declared in Thallo.h, the three launches in thallo_hip.h, libThallo.so exports all six, ThalloSolver has
    the three methods, and the refusals' messages are the library's"""
    from thallo_amd.build import build_library
    build_library()
    L = thallo_amd.lib()
    names = {"Thallo.h": ["ThalloX_PlanSetPrior", "ThalloX_PlanPriorTerms", "ThalloX_PlanPriorCost"],
             "thallo_hip.h": ["thallo_hip_prior_cost", "thallo_hip_prior_init", "thallo_hip_prior_lm_shift"]}
    for header, want in names.items():
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        declared = set(re.findall(r"\b((?:Thallo_|ThalloX_|thallo_hip_)\w+)\s*\(", txt))
        for n in want: assert n in declared and hasattr(L, n), n
    for n in ("set_prior", "prior_terms", "prior_cost"): assert callable(getattr(api.ThalloSolver, n, None)), n
    # the refusals at the call: without a device no plan exists to refuse anything, so here the messages are matched against the library's text; tests/test_gpu_ba_prior.py
    # provokes each of them on a plan
    src = "".join(open(os.path.join(ROOT, "thallo_amd", "csrc", f)).read() for f in ("solver_forms.cpp", "solver_dist.cpp", "api.cpp"))
    for msg in ("no priors for this energy", "priors run on one GPU (this plan is distributed)", "priors run on one GPU (ThalloX_PlanSetPrior came first)",
                "a direct-solve plan has no PCG loop to carry a prior through", "doublePrecision=1 solves without priors", "is not an Unknown of this energy",
                "the unknown has %ld (elements x components)", "must be finite and not negative", "must be finite where its weight is positive", "priors need"):
        assert msg in src, msg
