"""Gaussian priors on single unknowns in bundle adjustment (csrc/prior.hip, ThalloX_PlanSetPrior): the three kernels through their exported symbols against float64, then
Gauss-Newton and Levenberg-Marquardt through the C ABI -- point Jacobi, block Jacobi, the Schur complement, the assembled reduced camera matrix, its dense Cholesky factor
and the two-level preconditioner -- against the CPU restatement (tests/ba_prior_mirror.py), one GN step and the covariance under a soft gauge against float64, the launch
counts, the never-called plan's bits, and the refusals.

Bars of the kernel tests, in units of u = 2^-24 (float32 roundoff), derived from each output's operation count as tests/shim_kernels.py does; every reference is the float64
value of the device's own float32 inputs:
  r' = r - w (x - mu)        d = x - mu, w d, the subtraction: three roundings (two where the compiler fuses the last two) on quantities bounded by |r| + |w d|:
                             |r' - ref| <= 3 u (|r| + |w (x - mu)|), first order (3.01 u asserted)
  diag' = diag + w           one rounding: <= u |ref|
  pre = 1 / (1 + sqrt d')^2  of the device's own diag': sqrt, 1 +, the square, the reciprocal, each correctly rounded; the first two are squared: (2 * 2 + 1 + 1) u = 6 u (6.1 asserted)
  z = pre r'                 of the device's own pre and r': one rounding, u
  a partial of m terms       the terms' own roundings (cost: d, d^2, the product with w / 2 -- three; r . z of the device's own r and z: one) and m - 1 additions in any
                             order: gamma_{m + 2} sum |terms|, gamma_k = k u / (1 - k u); m = the scalars the partial's workgroup visits
  shift = CtC + w            bit for bit float32(CtC + w)
Scalars with w = 0 keep every bit of r, diag, pre and z; mu is not read there (the tests put NaN).

Through the C ABI the bar is tests/test_gpu_ba_held.py's: costs per step within max(1e-5, 3 err_jacobi) of the mirror's, err_jacobi the plain default plan against its own
mirror on the same instance."""
import ctypes as C
import os

import numpy as np
import pytest

import shim_kernels as sk
import test_gpu_block_precond as bp
import thallo_amd
from shim_kernels import EPS, F32
from thallo_amd import api, synthetic as syn

import ba_covariance_mirror as cm
import ba_schur_dense_mirror as dm
from ba_block_mirror import BaBlockMirror
from ba_held_mirror import masks
from ba_prior_mirror import CONFIGS, observation_rows, prior, prior_cost64, prior_mirror
from ba_schur_dense_mirror import BaSchurDenseMirror
from ba_schur_mirror import with_extras
from helpers import copy_params, set_ab, to_device, to_host
from test_ba_prior_mirror import SHAPES, flat, gauge_priors, priors_of

pytestmark = pytest.mark.gpu

GN = dict(nIterations=3, lIterations=10)
LM = dict(nIterations=3, lIterations=7, q_tolerance=0.1, function_tolerance=0.0)
PRIOR_LAUNCHES = ("PriorCost", "PriorInit", "PriorShift")
GUARD = 64                       # canary words in front of and behind every output of the kernel tests
COST_PARTIALS = 64               # THALLO_HIP_PRIOR_COST_PARTIALS


def gamma(k): return k * EPS / (1 - k * EPS)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    lib = bp.load_shim()
    vp, it, lg = C.c_void_p, C.c_int, C.c_long
    for name, args in {"prior_cost": [vp] * 4 + [lg, lg, vp, it, vp], "prior_init": [vp] * 4 + [lg, lg] + [vp] * 4 + [it, vp, vp], "prior_lm_shift": [vp, vp, lg, vp, vp],
                       "hold_pcg": [vp, vp, vp, vp, lg, vp, vp]}.items():
        f = getattr(lib, "thallo_hip_" + name); f.argtypes = args; f.restype = it
    return lib


class Guarded:
    """a device buffer with GUARD canary words in front of and behind its payload (payload None: the canary everywhere)"""

    def __init__(self, torch, n, payload=None):
        h = np.full(n + 2 * GUARD, sk.CANARY, np.uint32)
        if payload is not None: h[GUARD:GUARD + n] = np.ascontiguousarray(payload, F32).view(np.uint32)
        self.n, self.t = n, torch.from_numpy(h.view(np.int32)).cuda()
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def words(self):
        h = self.t.cpu().numpy().view(np.uint32)
        assert (h[:GUARD] == sk.CANARY).all() and (h[-GUARD:] == sk.CANARY).all(), "a canary around a buffer changed"
        return h[GUARD:GUARD + self.n].copy()

    def get(self):
        return self.words().view(F32)


def kernel_case(n, pattern, seed):
    """-> dict(w, mu, x, n0, r, diag, pre, z): means far from x (|x - mu| ~ 10), mu = NaN where w = 0"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.1, 50.0, n).astype(F32)
    if pattern == "zero": w[:] = 0
    if pattern == "sparse": w[rng.random(n) < 0.8] = 0; w[n // 2] = F32(7.5)
    mu = rng.standard_normal(n).astype(F32)
    x = (mu + 10 * rng.standard_normal(n)).astype(F32)
    mu[w == 0] = np.nan
    d = rng.uniform(0.0, 100.0, n).astype(F32)
    r = (30 * rng.standard_normal(n)).astype(F32)
    pre = sk.guarded_invert(d).astype(F32)
    return dict(w=w, mu=mu, x=x, n0=45 if n == 261 else (n if n < 64 else n // 3), r=r, diag=d, pre=pre, z=(pre * r).astype(F32))


def visits(n, grid):
    """scalars each workgroup of a grid-stride launch visits -> [grid]"""
    blk = (np.arange(n) // 256) % grid
    return np.bincount(blk, minlength=grid), blk


NS = [1, 63, 64, 65, 257, 261]
PATTERNS = ["zero", "positive", "sparse"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", NS)
def test_prior_cost_partials_against_float64(torch, L, n, pattern):
    """thallo_hip_prior_cost over the two regions of the unknowns: one partial per workgroup, each within gamma_{m + 2} sum |terms| of the float64 sum of its own terms;
    nothing else is written; a second launch gives the same bits; all-zero weights give 0.0f exactly; and the form that adds its partials onto a cost kernel's"""
    k = kernel_case(n, pattern, 100 + n)
    n0 = k["n0"]
    grid = min((n + 255) // 256, COST_PARTIALS)
    outs = []
    for _ in range(2):
        w, mu = Guarded(torch, n, k["w"]), Guarded(torch, n, k["mu"])
        x0, x1 = Guarded(torch, max(n0, 1), k["x"][:n0] if n0 else None), Guarded(torch, max(n - n0, 1), k["x"][n0:] if n0 < n else None)
        part = Guarded(torch, sk.MAX_PARTIALS)
        nb = L.thallo_hip_prior_cost(w.ptr, mu.ptr, x0.ptr, x1.ptr if n0 < n else None, n0, n, part.ptr, 0, None)
        torch.cuda.synchronize()
        assert nb == grid
        outs.append(part.words().tobytes())
        for b, src in ((w, k["w"]), (mu, k["mu"])): assert sk.same_bytes(b.get(), src)
    got = part.get()
    assert sk.written_slots(got) == grid
    on = k["w"] > 0
    terms = np.where(on, 0.5 * k["w"].astype(np.float64) * (k["x"].astype(np.float64) - np.where(on, k["mu"], 0).astype(np.float64)) ** 2, 0.0)
    m, blk = visits(n, grid)
    ref, mag = np.bincount(blk, weights=terms, minlength=grid), np.bincount(blk, weights=np.abs(terms), minlength=grid)
    err = np.abs(got[:grid].astype(np.float64) - ref)
    bar = np.array([gamma(int(mm) + 2) for mm in m]) * mag
    print("prior_cost", n, pattern, "n0", n0, "worst err / bar", float((err / np.where(bar > 0, bar, 1)).max()))
    assert (err <= bar).all()
    if pattern == "zero": assert got[:grid].tobytes() == np.zeros(grid, F32).tobytes()
    assert outs[0] == outs[1]
    # onto = K > 0: the same partials added onto the first of K that another launch left there -- float32(before + partial) bit for bit, the other K - grid words and
    # everything behind them untouched, K returned
    K = grid + 2
    before = (1000 * np.random.default_rng(n).standard_normal(K)).astype(F32)
    slot = Guarded(torch, K, before)
    assert L.thallo_hip_prior_cost(w.ptr, mu.ptr, x0.ptr, x1.ptr if n0 < n else None, n0, n, slot.ptr, K, None) == K
    torch.cuda.synchronize()
    after = slot.get()
    assert sk.same_bytes(after[:grid], (before[:grid] + got[:grid]).astype(F32)) and sk.same_bytes(after[grid:], before[grid:])
    # onto = 1: one workgroup visits every scalar; within gamma_{n + 2} sum |terms| and the one rounding of the addition
    one = Guarded(torch, 1, before[:1])
    assert L.thallo_hip_prior_cost(w.ptr, mu.ptr, x0.ptr, x1.ptr if n0 < n else None, n0, n, one.ptr, 1, None) == 1
    torch.cuda.synchronize()
    want = float(before[0]) + terms.sum()
    assert abs(float(one.get()[0]) - want) <= gamma(n + 2) * np.abs(terms).sum() + EPS * abs(want)


@pytest.mark.parametrize("held", [False, True])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", NS)
def test_prior_init_against_float64(torch, L, n, pattern, held):
    """thallo_hip_prior_init behind a PCGInit1's r, diag, pre, z: the four vectors within the bars at the top of the file where w > 0 and bit for bit unchanged where
    w = 0, the partials of r . z within gamma_{m + 2} sum |r z| of the device's own r and z, canaries around every output intact, two launches the same bits.  held: the
    priors sit on held scalars -- thallo_hip_hold_pcg behind the launch zeroes pre and z at every scalar with a prior, leaves r and diag with the prior's terms, and its
    partials are those of the free scalars alone"""
    k = kernel_case(n, pattern, 200 + n)
    n0 = k["n0"]
    grid = min((n + 255) // 256, sk.MAX_PARTIALS)
    outs = []
    for _ in range(2):
        w, mu = Guarded(torch, n, k["w"]), Guarded(torch, n, k["mu"])
        x0, x1 = Guarded(torch, max(n0, 1), k["x"][:n0] if n0 else None), Guarded(torch, max(n - n0, 1), k["x"][n0:] if n0 < n else None)
        v = {q: Guarded(torch, n, k[q]) for q in ("r", "diag", "pre", "z")}
        part = Guarded(torch, sk.MAX_PARTIALS)
        nb = L.thallo_hip_prior_init(w.ptr, mu.ptr, x0.ptr, x1.ptr if n0 < n else None, n0, n, v["r"].ptr, v["diag"].ptr, v["pre"].ptr, v["z"].ptr, 1, part.ptr, None)
        torch.cuda.synchronize()
        assert nb == grid
        outs.append(b"".join(v[q].words().tobytes() for q in v) + part.words().tobytes())
    g = {q: v[q].get() for q in v}
    gp = part.get()
    assert sk.written_slots(gp) == grid and outs[0] == outs[1]
    on = k["w"] > 0
    for q in g: assert sk.same_bytes(g[q][~on], k[q][~on]), q
    w64, x64, mu64 = k["w"].astype(np.float64), k["x"].astype(np.float64), np.where(on, k["mu"], 0).astype(np.float64)
    wd = w64 * (x64 - mu64)
    e_r = np.abs(g["r"] - (k["r"] - wd))[on] / (np.abs(k["r"]) + np.abs(wd))[on]
    e_d = np.abs(g["diag"] - (k["diag"].astype(np.float64) + w64))[on] / (k["diag"] + w64)[on]
    pre64 = 1.0 / (1.0 + np.sqrt(g["diag"].astype(np.float64))) ** 2
    e_p = (np.abs(g["pre"] - pre64) / pre64)[on]
    z64 = g["pre"].astype(np.float64) * g["r"]
    e_z = (np.abs(g["z"] - z64) / np.where(z64 != 0, np.abs(z64), 1))[on]
    worst = [float(e.max()) / EPS if e.size else 0.0 for e in (e_r, e_d, e_p, e_z)]
    print("prior_init", n, pattern, "errors in u: r %.2f diag %.2f pre %.2f z %.2f" % tuple(worst))
    assert worst[0] <= 3.01 and worst[1] <= 1.0 and worst[2] <= 6.1 and worst[3] <= 1.0
    terms = g["r"].astype(np.float64) * g["z"]
    m, blk = visits(n, grid)
    err = np.abs(gp[:grid].astype(np.float64) - np.bincount(blk, weights=terms, minlength=grid))
    bar = np.array([gamma(int(mm) + 2) for mm in m]) * np.bincount(blk, weights=np.abs(terms), minlength=grid)
    print("prior_init", n, pattern, "partials: worst err / bar", float((err / np.where(bar > 0, bar, 1)).max()))
    assert (err <= bar).all()
    if not held: return
    mask = np.zeros((n + 3) // 4 * 4, np.uint8); mask[:n] = on
    md, part2 = Guarded(torch, len(mask) // 4, mask.view(np.uint32).view(F32)), Guarded(torch, sk.MAX_PARTIALS)
    assert L.thallo_hip_hold_pcg(md.ptr, v["r"].ptr, v["pre"].ptr, v["z"].ptr, n, part2.ptr, None) == grid
    torch.cuda.synchronize()
    h = {q: v[q].get() for q in v}
    assert sk.same_bytes(h["r"], g["r"]) and sk.same_bytes(h["diag"], g["diag"])
    for q in ("pre", "z"):
        assert h[q][on].tobytes() == np.zeros(int(on.sum()), F32).tobytes() and sk.same_bytes(h[q][~on], k[q][~on])
    free_terms = np.where(on, 0.0, k["r"].astype(np.float64) * k["z"])
    err2 = np.abs(part2.get()[:grid].astype(np.float64) - np.bincount(blk, weights=free_terms, minlength=grid))
    assert (err2 <= np.array([gamma(int(mm) + 2) for mm in m]) * np.bincount(blk, weights=np.abs(free_terms), minlength=grid)).all()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", NS)
def test_the_lm_shift_plane_is_float32_of_ctc_plus_w_bit_for_bit(torch, L, n, pattern):
    k = kernel_case(n, pattern, 300 + n)
    ctc = (k["diag"] * F32(1e-4)).astype(F32)
    w, c, out = Guarded(torch, n, k["w"]), Guarded(torch, n, ctc), Guarded(torch, n)
    assert L.thallo_hip_prior_lm_shift(w.ptr, c.ptr, n, out.ptr, None) == 0
    torch.cuda.synchronize()
    assert sk.same_bytes(out.get(), (ctc + k["w"]).astype(F32)) and sk.same_bytes(w.get(), k["w"]) and sk.same_bytes(c.get(), ctc)


def test_the_entry_points_refuse_bad_arguments(torch, L):
    b = Guarded(torch, 64, np.zeros(64, F32))
    p = b.ptr
    assert L.thallo_hip_prior_cost(None, p, p, p, 1, 2, p, 0, None) == sk.INVALID and L.thallo_hip_prior_cost(p, p, p, None, 1, 2, p, 0, None) == sk.INVALID
    assert L.thallo_hip_prior_cost(p, p, p, p, 3, 2, p, 0, None) == sk.INVALID and L.thallo_hip_prior_cost(p, p, p, p, 0, 0, p, 0, None) == sk.INVALID
    assert L.thallo_hip_prior_cost(p, p, p, p, 1, 2, p, -1, None) == sk.INVALID and L.thallo_hip_prior_cost(p, p, p, p, 1, 2, p, sk.MAX_PARTIALS + 1, None) == sk.INVALID
    assert L.thallo_hip_prior_init(p, p, p, p, 1, 2, p, None, p, p, 1, p, None) == sk.INVALID
    assert L.thallo_hip_prior_lm_shift(p, None, 2, p, None) == sk.INVALID
    torch.cuda.synchronize()
    assert not b.get().any()


# ------------------------------------------------------------------ 2. through the C ABI
def plan(dims, p, lm, config, priors=None, hold=None, loss=None, clear=False, **sp):
    """-> (solver, params, device arrays), initialised; priors = (mean, weight) flat over [cameras | points] in the caller's ids"""
    d = to_device(copy_params(p))
    s = api.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), solverkind="levenberg_marquardt" if lm else "gauss_newton")
    if lm: s.enable_lm()
    if config == "block": s.set_preconditioner("block_jacobi")
    if config == "schur": s.set_linear_solver("schur_pcg")
    if config in ("schur_explicit", "two_level"): s.set_linear_solver("schur_explicit_pcg")
    if config == "two_level": s.set_preconditioner("two_level")
    if config == "schur_dense": s.set_linear_solver("schur_dense")
    if loss: s.set_robust_loss(*loss)
    nc = 9 * dims[0]
    if hold is not None:
        s.hold(0, hold[:nc]); s.hold(1, hold[nc:])
    if priors is not None:
        s.set_prior(0, priors[0][:nc], priors[1][:nc]); s.set_prior(1, priors[0][nc:], priors[1][nc:])
    if clear:
        s.set_prior(0, None, None); s.set_prior(1, None, None)
    s.set_solver_parameters(**sp)
    params = s.make_params(d)
    s.init(params)
    assert s.ready(), api.last_error()
    return s, params, d


def run(dims, p, lm, config, **kw):
    """-> dict(costs, iters, cams, pts, name, terms, prior_cost at Init and at the end, stats)"""
    s, params, d = plan(dims, p, lm, config, **kw)
    out = dict(costs=[s.current_cost()], iters=[], terms=s.prior_terms(), prior0=s.prior_cost())
    while s.step(params):
        out["costs"].append(s.current_cost()); out["iters"].append(len(s.alpha_beta_trace()))
    out.update(name=s.schedule_name, stats={k: v["launches"] for k, v in s.kernel_stats().items() if v["launches"]}, cams=to_host(d[0]).copy(), pts=to_host(d[1]).copy(),
               costs=np.array(out["costs"]), prior1=s.prior_cost())
    s.close()
    return out


def rel(a, b):
    assert len(a) == len(b), (a, b)
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.abs(np.asarray(b, np.float64))


_problems = {}


def problem(dims, band):
    """(params, (mean, weight)) once per shape, never written"""
    if dims not in _problems:
        p = syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band)
        _problems[dims] = (p, priors_of(dims, p))
    return _problems[dims]


_err_j = {}


def err_jacobi(dims, band, lm):
    """the plain default plan against its own mirror, GN 3 x 10 / LM 3 x 7 on the instance: the largest relative cost difference"""
    if (dims, lm) not in _err_j:
        p, _ = problem(dims, band)
        m = BaBlockMirror(dims, p)
        c = m.lm_solve(3, LM["lIterations"], kind="jacobi", q_tolerance=0.1, function_tolerance=0.0)[0] if lm else m.gn_solve(3, 10, "jacobi")
        _err_j[(dims, lm)] = float(rel(run(dims, p, lm, "jacobi", **(LM if lm else GN))["costs"], c).max())
        print("err_jacobi", dims, "LM" if lm else "GN", _err_j[(dims, lm)])
    return _err_j[(dims, lm)]


_mirrors = {}


def mirror_solve(dims, band, config, lm, mask=None, loss=None):
    """(costs, iterations per step, the prior's share at the end), once"""
    key = (dims, config, lm, None if mask is None else mask.tobytes(), loss)
    if key not in _mirrors:
        p, (mu, w) = problem(dims, band)
        m, kind = prior_mirror(config, mu, w, dims, p, mask=mask, loss=loss)
        if lm: costs, iters = m.lm_solve(3, LM["lIterations"], kind=kind, q_tolerance=0.1, function_tolerance=0.0)
        else: costs, iters = m.gn_solve(3, 10, kind), None
        _mirrors[key] = (costs, iters, m.prior_cost())
    return _mirrors[key]


@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("dims,band", SHAPES)
def test_solve_with_priors_through_the_c_abi(torch, dims, band, config, lm):
    """GN 3 x 10 / LM 3 x 7 (q_tolerance 0.1, function_tolerance 0) with the priors of tests/test_ba_prior_mirror.py (intrinsics, control points, the soft gauge; no mask:
    the gauge is the priors') in the caller's point order and in the plan's own (THALLO_AB=ba_renumber=1; the priors arrive in the caller's ids either way): costs per step
    the prior mirror's within max(1e-5, 3 err_jacobi); LM iteration counts the mirror's on the block and Schur plans; prior_cost() at Init within the partials' bar of the
    float64 share and at the end within the cost's own bar of the mirror's share; prior_terms() and the schedule name carry the count"""
    p, (mu, w) = problem(dims, band)
    cm_, im, share = mirror_solve(dims, band, config, lm)
    ej = err_jacobi(dims, band, lm)
    bar = max(1e-5, 3 * ej)
    count = int((w > 0).sum())
    share0 = prior_cost64(w, mu, flat(p))
    for ren in ("0", "1"):
        with pytest.MonkeyPatch.context() as mp:
            set_ab(mp, ba_renumber=ren)
            o = run(dims, p, lm, config, priors=(mu, w), **(LM if lm else GN))
        err = rel(o["costs"], cm_).max()
        print("prior", dims, config, "LM" if lm else "GN", "renumber", ren, list(o["costs"]), o["iters"], "mirror", cm_, im, "err", err, "err_jacobi", ej,
              "prior share", o["prior0"], share0, "->", o["prior1"], share)
        assert ("renumbered" in o["name"]) == (ren == "1")
        assert o["terms"] == count and o["name"].endswith("; %d priors" % count)
        assert err <= bar
        assert abs(o["prior0"] - share0) <= gamma(len(w) + 2) * share0
        assert abs(o["prior1"] - share) <= bar * o["costs"][-1]
        assert o["costs"][-1] < o["costs"][0]
        if lm and config in ("block", "schur", "schur_explicit"): assert o["iters"] == im, (o["iters"], im)
        if not lm: assert o["iters"] == [0 if config == "schur_dense" else 10] * 3


@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("config", ["block", "schur_explicit"])
def test_priors_under_huber_and_a_mask_through_the_c_abi(torch, config, lm):
    """Huber(2), cameras {0, 1} held and the priors together on (24, 300, 1200): costs per step the mirror's (the loss is not applied to the priors: prior(robust(...))),
    the held scalars keep their bits although camera 0 carries priors, the prior's share counts the held scalars' constant terms"""
    dims, band = SHAPES[1]
    p, (mu, w) = problem(dims, band)
    mu = mu.copy(); mu[:6] += F32(0.01)                  # (a held scalar whose prior is not at its value: a constant of the cost)
    mask = masks(dims[0], dims[1])["two_cameras"]
    m, kind = prior_mirror(config, mu, w, dims, p, mask=mask, loss=("huber", 2.0))
    cmir = m.lm_solve(3, LM["lIterations"], kind=kind, q_tolerance=0.1, function_tolerance=0.0)[0] if lm else m.gn_solve(3, 10, kind)
    ej = err_jacobi(dims, band, lm)
    o = run(dims, p, lm, config, priors=(mu, w), hold=mask, loss=("huber", 2.0), **(LM if lm else GN))
    err = rel(o["costs"], cmir).max()
    after = np.concatenate([o["cams"].ravel(), o["pts"].ravel()])
    print("prior + huber + mask", config, "LM" if lm else "GN", list(o["costs"]), "mirror", cmir, "err", err, "err_jacobi", ej, o["name"])
    assert err <= max(1e-5, 3 * ej)
    assert after[mask].tobytes() == flat(p)[mask].tobytes()
    held_share = prior_cost64(np.where(mask, w, 0), mu, flat(p))
    assert held_share > 0 and o["prior1"] >= held_share * (1 - 1e-5)
    assert "huber loss, scale 2" in o["name"] and "18 unknowns held" in o["name"] and o["name"].endswith("; %d priors" % int((w > 0).sum()))


@pytest.mark.parametrize("dims,band", SHAPES)
def test_one_gn_step_against_float64(torch, dims, band):
    """one GN step of the dense plan with the priors (no mask): the step x_after - x_before over all unknowns against np.linalg.solve(J^T J + W, b) in float64 from the
    oracle's J, within 4 x the dense prior mirror's own error against the same solve (the bar of the dense form's own step test), each in max |err| / max |delta|"""
    p, (mu, w) = problem(dims, band)
    m = prior(BaSchurDenseMirror)(mu, w, dims, p)
    J, r, d, Hs = m.linearise()
    Jd = np.asarray(J.todense())
    on = np.nonzero(w > 0)[0]
    rows = np.concatenate([m._problem().csr()[3].astype(np.float64), np.sqrt(w[on].astype(np.float64)) * (flat(p)[on].astype(np.float64) - mu[on])])
    ref = np.linalg.solve(Jd.T @ Jd, -(Jd.T @ rows))
    x0 = flat(p).astype(np.float64)
    assert m.gn_step() and m.pivot is None
    step_m = flat(m.params).astype(np.float64) - x0
    s, params, dv = plan(dims, p, False, "schur_dense", priors=(mu, w), nIterations=1, lIterations=10)
    assert s.step(params), api.last_error()
    step_d = np.concatenate([to_host(dv[0]).ravel(), to_host(dv[1]).ravel()]).astype(np.float64) - x0
    s.close()
    top = np.abs(ref).max()
    e_m, e_d = np.abs(step_m - ref).max() / top, np.abs(step_d - ref).max() / top
    print("GN step with priors against float64", dims, "mirror error", e_m, "device", e_d, "= %.2f x" % (e_d / e_m))
    assert e_m > 0 and e_d <= 4 * e_m


def test_the_soft_gauge_gives_every_camera_a_finite_covariance(torch):
    """the 6-camera instance ((5, 72, 330) with a camera and a point nothing observes and a point observed once), no held scalar: the dense GN step fails without priors
    (tests/test_gpu_ba_schur_dense.py) and succeeds with the soft gauge of tests/test_ba_prior_mirror.py; with the same weight on the nine scalars of the camera nothing
    observes, covariance over ALL cameras returns finite blocks without an exact-zero row, within 4 x the dense mirror's error of inv(A + W) in float64"""
    dims, band = SHAPES[0]
    p, d3 = with_extras(syn.bundle_adjustment(C=dims[0], P=dims[1], O=dims[2], band=band))
    C_, P_, O_ = d3
    mu, w = gauge_priors(d3, p)
    s, params, dv = plan(d3, p, False, "schur_dense", priors=(mu, w), nIterations=2, lIterations=10)
    c0 = s.current_cost()
    assert s.step(params), api.last_error()
    assert s.current_cost() < c0 and s.held_unknowns() == -1
    s.close()
    w = w.copy(); w[9 * (C_ - 1):9 * C_] = w[0]
    s, params, dv = plan(d3, p, False, "schur_dense", priors=(mu, w), nIterations=2, lIterations=10)
    assert s.step(params), api.last_error()
    out = s.covariance(params, cameras=list(range(C_)))
    here = [to_host(dv[0]).copy(), to_host(dv[1]).copy()] + [a.copy() for a in p[2:]]
    s.close()
    got = out["cameras"]
    assert np.isfinite(got).all() and (np.abs(got).max(axis=2) > 0).all() and (np.einsum("bii->bi", got) > 0).all()
    m = prior(BaBlockMirror)(mu, w, d3, here)
    mask = np.zeros(9 * C_ + 3 * P_, bool)
    with observation_rows(O_):
        J, sys = dm.gn_system(m, mask)
        A = (J.T @ J).toarray()
        free = ~cm.undetermined(A, C_)
        Sig = cm.dense_cov64(A, free)
        Bm, _ = dm.DenseCovariance(sys, mask).solve(0, list(range(C_)))
    assert free[:9 * C_].all()
    ref = cm.blocks_of(Sig, list(range(C_)), 9, 0)
    fr = free[:9 * C_].reshape(-1, 9)
    e_dev, e_mir = cm.cov_error(got, ref, fr), cm.cov_error(Bm, ref, fr)
    print("soft-gauge covariance", d3, "weight", float(w[0]), "mirror error", e_mir, "device", e_dev, "= %.2f x" % (e_dev / e_mir), out["info"])
    assert out["info"]["not_converged"] == 0 and out["info"]["nan_blocks"] == 0
    assert e_mir > 0 and e_dev <= 4 * e_mir


# ------------------------------------------------------------------ 3. launches
@pytest.mark.parametrize("config,lm", [("jacobi", True), ("schur_explicit", False)])
def test_no_launch_is_added_to_a_pcg_iteration(torch, config, lm):
    """kernel stats after 2 steps of 6 iterations, a point-Jacobi LM plan and an assembled-Schur GN plan: every launch name of the plan without priors has the same count on
    the plan with them, and the additional launches are per step or per cost evaluation only -- PriorInit once per step, PriorShift once per LM step, PriorCost once per
    computeCost"""
    dims, band = SHAPES[1]
    p, pri = problem(dims, band)
    sp = dict(nIterations=2, lIterations=6, q_tolerance=-1e30, function_tolerance=0.0) if lm else dict(nIterations=2, lIterations=6)
    a = run(dims, p, lm, config, **sp)["stats"]
    b = run(dims, p, lm, config, priors=pri, **sp)["stats"]
    extra = {k: b.pop(k) for k in PRIOR_LAUNCHES if k in b}
    print("launches", config, "LM" if lm else "GN", a, extra)
    assert a == b
    want = {"PriorInit": 2, "PriorCost": a["computeCost"] + 1}      # (+ 1: run()'s own prior_cost() call behind Init)
    if lm: want["PriorShift"] = 2
    assert extra == want


# ------------------------------------------------------------------ 4. the never-called plan's bits
@pytest.mark.parametrize("lm", [False, True])
@pytest.mark.parametrize("config", CONFIGS)
def test_cleared_and_all_zero_priors_are_the_never_called_plan_bit_for_bit(torch, config, lm):
    """never called / set then cleared / all-zero weights (with NaN means: a mean is not looked at where its weight is 0) / a plan that ran with priors, cleared them and
    was initialised again: the same costs, iterations, schedule name, launch counts and unknown bytes (cameras {0, 1} held throughout: GN needs a gauge on every plan)"""
    dims, band = SHAPES[1]
    p, pri = problem(dims, band)
    hold = masks(dims[0], dims[1])["two_cameras"]
    sp = LM if lm else GN
    a = run(dims, p, lm, config, hold=hold, **sp)
    b = run(dims, p, lm, config, hold=hold, priors=pri, clear=True, **sp)
    c = run(dims, p, lm, config, hold=hold, priors=(np.full(len(pri[0]), np.nan, F32), np.zeros(len(pri[0]), F32)), **sp)
    assert a["terms"] == b["terms"] == c["terms"] == 0 and "priors" not in a["name"] and a["prior0"] == c["prior1"] == 0.0
    for o in (b, c):
        assert list(a["costs"]) == list(o["costs"]) and a["iters"] == o["iters"] and a["name"] == o["name"] and a["stats"] == o["stats"]
        assert sk.same_bytes(a["cams"], o["cams"]) and sk.same_bytes(a["pts"], o["pts"])
    # a re-Init after clearing: the plan that ran a step with priors runs the never-called plan's solve from the same start
    s, params, d = plan(dims, p, lm, config, hold=hold, priors=pri, **sp)
    assert s.prior_terms() == int((pri[1] > 0).sum()) and s.step(params)
    s.set_prior(0, None, None); s.set_prior(1, None, None)
    for k, a0 in zip((0, 1), p[:2]): d[k].copy_(to_device([a0.copy()])[0])
    s.set_solver_parameters(trust_region_radius=1e4, radius_decrease_factor=2.0, **sp)      # (an LM step leaves its radius in the parameters: a new solve starts from the default)
    s.init(params)
    assert s.ready() and s.prior_terms() == 0 and "priors" not in s.schedule_name
    costs = [s.current_cost()]
    while s.step(params): costs.append(s.current_cost())
    assert costs == list(a["costs"]) and sk.same_bytes(to_host(d[0]), a["cams"]) and sk.same_bytes(to_host(d[1]), a["pts"])
    s.close()


# ------------------------------------------------------------------ 5. the interface and its refusals
def test_refusals_name_the_energy_and_the_reason(torch, monkeypatch, tmp_path):
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energies")
    one = (C.c_float * 4)(1, 0, 0, 0)
    cases = [((48, 32), thallo_amd.energy_file("image_warping"), False, "no priors for this energy"),          # another hand-written energy
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), False, "no priors for this energy"),      # a generated one
             ((512, 1, 512), os.path.join(here, "curve_fit_graph.t"), True, "doublePrecision")]                 # doublePrecision = 1
    for dims, f, dbl, why in cases:
        s = api.ThalloSolver(dims, f, double_precision=dbl)
        assert s.prior_terms() == -1
        assert s._L.ThalloX_PlanSetPrior(s.plan, 0, one, one, 4) != 0
        assert s.energy_name and s.energy_name in api.last_error() and why in api.last_error(), api.last_error()
        with pytest.raises(RuntimeError): s.set_prior(0, np.zeros(4), np.ones(4))
        assert s._L.ThalloX_PlanSetPrior(s.plan, 0, None, None, 0) == 0
        s.close()
    ba = thallo_amd.energy_file("bundle_adjustment")
    s = api.ThalloSolver((5, 72, 330), ba, double_precision=True)
    assert s._L.ThalloX_PlanSetPrior(s.plan, 0, one, one, 4) != 0 and "bundle_adjustment" in api.last_error() and "doublePrecision" in api.last_error()
    s.close()
    s = api.ThalloSolver((5, 72, 330), ba)
    z45, o45 = np.zeros(45), np.ones(45)
    for inp in (2, 3, 4, -1, 7):                                   # observations and the two index lists are no Unknowns; neither is what does not exist
        with pytest.raises(RuntimeError, match="bundle_adjustment.*input %d is not an Unknown" % inp): s.set_prior(inp, z45, o45)
    with pytest.raises(RuntimeError, match="bundle_adjustment.*44 scalars.*45 .elements x components"): s.set_prior(0, np.zeros(44), np.ones(44))
    with pytest.raises(RuntimeError, match="bundle_adjustment.*elements x components"): s.set_prior(1, np.zeros(72), np.ones(72))
    for bad in (-1.0, np.nan, np.inf):
        wv = o45.copy(); wv[7] = bad
        with pytest.raises(RuntimeError, match="bundle_adjustment.*weight of scalar 7 of input 0 must be finite and not negative"): s.set_prior(0, z45, wv)
    mv = z45.copy(); mv[3] = np.nan
    with pytest.raises(RuntimeError, match="bundle_adjustment.*mean of scalar 3 of input 0 must be finite where its weight is positive"): s.set_prior(0, mv, o45)
    wv = o45.copy(); wv[3] = 0
    s.set_prior(0, mv, wv)                                          # (... and is not looked at where the weight is 0)
    with pytest.raises(RuntimeError, match="bundle_adjustment.*priors run on one GPU"):      # a distributed plan: the prior first ...
        s.set_distributed(0, 1, 0, 0, device_exchange=False)
    p = syn.bundle_adjustment(C=5, P=72, O=330, band=5)
    d = to_device(copy_params(p)); params = s.make_params(d)
    s.init(params)
    assert s.ready() and s.prior_terms() == 44 and s.schedule_name.endswith("; 44 priors")
    s.set_prior(0, None, None); s.init(params)
    assert s.ready() and s.prior_terms() == 0 and "priors" not in s.schedule_name and s.prior_cost() == 0.0
    s.close()
    s = api.ThalloSolver((8, 72, 330), ba)                                           # ... and the distribution first (one rank's camera shard)
    s.set_distributed(0, 1, 0, 0, device_exchange=False)
    with pytest.raises(RuntimeError, match="bundle_adjustment.*distributed"): s.set_prior(0, np.zeros(72), np.ones(72))
    s.close()
    # a direct-solve plan (tests/test_gpu_ba_held.py)
    lines = "".join(f"r.{n}.J:set_materialize(true)\nr.{n}.JtJ:set_materialize(true)\n" for n in ("fit", "reg")) + "r:set_direct_solve(true)\n"
    f = tmp_path / "laplacian_direct.t"
    f.write_text(open(thallo_amd.energy_file("laplacian_graph")).read() + "\n" + lines)
    monkeypatch.setenv("THALLO_FRONTEND", "generate"); monkeypatch.setenv("THALLO_ENABLE_DIRECT_SOLVE", "1")
    s = api.ThalloSolver((256, 255), str(f))
    assert s.schedule_name == "dense direct solve"
    assert s._L.ThalloX_PlanSetPrior(s.plan, 0, one, one, 4) != 0
    assert s.energy_name and s.energy_name in api.last_error() and "direct-solve" in api.last_error(), api.last_error()
    s.close()
