"""thallo_hip_linear_update_all (csrc/pcg_kernels.hip k_linear_update_all: up to 128 terms of a GN step applied in one launch to a running value that starts at
0.0f) and the GN step that ends with it (csrc/solver.cpp ring_takes_one_pass / ring_step_update: a loop of 65 .. 128 iterations runs on a ring as long as itself,
no launch touches delta, the step's end is one "PCGDeltaUpdate" launch per unknown image).

Kernel level.  The reference is the parent's function, not the code under test: thallo_hip_linear_update_n_from_zero on the first <= 32 terms and
thallo_hip_linear_update_n on every further batch of <= 32 (delta carried through memory in between, the last batch with X where X is asked for).  The new entry
must leave the SAME BITS -- one fma per term on the running value, oldest first.  The first 32 terms mix words and lists of partials (alphaN_0 of a GN step is a
list); behind them every alpha is a pair of words, which is all the entry accepts there.  Next to the bitwise comparison, a float64 accumulation of the same chain
as a sanity bound: in the exact regime (integers times multiples of 1/4: every fma exact) rtol 1e-6 on the value itself.  The rounded regime is an ADDITION with
a weaker norm: 1e-6 of the sum of the magnitudes that went into the value, not of the value (random signs cancel: no bound relative to the value holds for
float32); a rounding is at most 2^-24 = 6e-8 of the running value, which that sum bounds, and the roundings of the <= 129 operations add up like a random walk,
not to their worst case 129 x 6e-8 (measured: 8.3e-7 at 128 terms).

Solver level.  image_warping 132 x 40 and 250 x 70, two GN steps, lIterations 2, 3, 33, 34, 65, 100: the default, THALLO_DELTA_PLANES=33 (the schedule before
this entry existed) and THALLO_DELTA_PLANES=0 (delta inside every launch) agree bit for bit on unknowns, costs and the alpha / beta trace."""
import ctypes as C

import numpy as np
import pytest

import shim_kernels as sk
from shim_kernels import F32
import thallo_amd
from thallo_amd import api, synthetic as syn
from helpers import to_device, copy_params

pytestmark = pytest.mark.gpu

N_ALIGNED = 4 * 1031
MAX_STEP_TERMS = 128
ALPHAS_EXACT = [(1.0, 2.0), (3.0, 4.0), (-2.0, 8.0), (6.0, 4.0)]      # alpha_j from {1/2, 3/4, -1/4, 3/2}
LIST_LENGTHS = [2, 63, 64, 65, 251, sk.MAX_PARTIALS]


class UpdateTermT(C.Structure):      # thallo_update_term_t
    _fields_ = [("p", C.c_void_p), ("alphaN", api.SumT), ("alphaD", api.SumT)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    lib = sk.shim()
    for f, args in ((lib.thallo_hip_linear_update_n_from_zero, [C.c_void_p, C.c_void_p, sk.UpdateTermsT, C.c_long, C.c_int, C.c_void_p]),
                    (lib.thallo_hip_linear_update_all, [C.c_void_p, C.c_void_p, C.POINTER(UpdateTermT), C.c_int, C.c_long, C.c_int, C.c_void_p])):
        f.argtypes = args; f.restype = C.c_int
    return lib


def _make_terms(torch, rng, regime, n, count, list_at=()):
    """count terms: planes, (alphaN, alphaD) partials on the device, the float32 alphas.  Terms 0, 5, 10, ... below 32 carry lists (term 0 both sums, like
    alphaN_0 / alphaD_0 when nothing has been finished), every other term two words; `list_at`: further terms forced to carry a list."""
    terms = (UpdateTermT * max(count, 1))()
    planes, alphas, keep = [], [], []
    for j in range(count):
        lists = (j < sk.MAX_UPDATE_TERMS and j % 5 == 0) or j in list_at
        cn = LIST_LENGTHS[j % 6] if lists else 1
        cd = LIST_LENGTHS[(j + 3) % 6] if lists and j % 10 == 0 else 1
        if regime == "exact":
            p = sk.exact_vec(rng, n)
            parts = [sk.exact_sum(rng, cn, ALPHAS_EXACT[j % 4][0]), sk.exact_sum(rng, cd, ALPHAS_EXACT[j % 4][1])]
        else:
            p = rng.standard_normal(n).astype(F32)
            parts = [sk.rounded_sum(rng, cn), sk.rounded_sum(rng, cd, True) * 16]
        pv, ts = sk.DVec(torch, n, p), [sk.dbuf(torch, q) for q in parts]
        keep.append((ts, parts))
        terms[j].p = pv.ptr; terms[j].alphaN = sk.sumt(ts[0]); terms[j].alphaD = sk.sumt(ts[1])
        planes.append(pv); alphas.append(sk.div32(sk.sum_partials(parts[0]), sk.sum_partials(parts[1]), True))
    return terms, planes, alphas, keep


def _batch(terms, lo, hi):
    T = sk.UpdateTermsT(); T.count = hi - lo
    for j in range(lo, hi):
        T.p[j - lo] = terms[j].p; T.alphaN[j - lo] = terms[j].alphaN; T.alphaD[j - lo] = terms[j].alphaD
    return T


def _chained_reference(L, terms, count, X, delta, n):
    """the parent's entries, <= 32 terms per launch: delta from zero, then delta += per batch; the last batch adds into X when X is given"""
    cuts = list(range(0, count, sk.MAX_UPDATE_TERMS)) + [count]
    for b, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        last = hi == count
        f = L.thallo_hip_linear_update_n_from_zero if b == 0 else L.thallo_hip_linear_update_n
        assert f(X.ptr if (X is not None and last) else None, delta.ptr, _batch(terms, lo, hi), n, 0, None) > 0


@pytest.mark.parametrize("regime", ["exact", "rounded"])
@pytest.mark.parametrize("form", ["delta", "X"])
@pytest.mark.parametrize("n", [N_ALIGNED, N_ALIGNED + 3], ids=["aligned", "scalar"])
@pytest.mark.parametrize("count", [1, 7, 8, 9, 32, 33, 63, 64, 65, 100, 128])
def test_one_pass_is_bitwise_the_chained_updates(torch, L, count, n, form, regime):
    rng = np.random.default_rng([77, count, n, form == "X", regime == "exact"])
    terms, planes, alphas, keep = _make_terms(torch, rng, regime, n, count)
    x_host = (sk.exact_vec if regime == "exact" else sk.rounded_vec)(rng, n)
    with_X = form == "X"
    cus = L.thallo_hip_device_cu_count()
    g = sk.flat_grid(n // 4 if n % 4 == 0 else n, 2 * cus)
    assert g > 1                                             # (more than one workgroup; the last one partly idle)
    # ---- the reference: delta through memory between batches of <= 32
    d_ref, X_ref = sk.DVec(torch, n), sk.DVec(torch, n, x_host)
    _chained_reference(L, terms, count, X_ref if with_X else None, d_ref, n)
    # ---- the entry under test: delta is an output (X == NULL) or must not be touched at all (X given)
    d_new, X_new = sk.DVec(torch, n), sk.DVec(torch, n, x_host)
    ret = L.thallo_hip_linear_update_all(X_new.ptr if with_X else None, d_new.ptr, terms, count, n, 0, None)
    torch.cuda.synchronize()
    assert ret == g, (ret, g)
    for p in planes: assert p.unchanged(), "a plane changed"
    for ts, parts in keep:
        for t, q in zip(ts, parts): assert sk.same_bytes(t.cpu().numpy(), q)
    pf = [p.h0[:n].astype(np.float64) for p in planes]
    want = np.zeros(n)
    for a, q in zip(alphas, pf): want = want + float(a) * q
    scale = sum(np.abs(float(a) * q) for a, q in zip(alphas, pf))
    if with_X:
        want, scale = want + x_host.astype(np.float64), scale + np.abs(x_host.astype(np.float64))
        got = X_new.get()
        assert sk.same_bytes(got[:n], X_ref.get()[:n]), np.flatnonzero(got[:n] != X_ref.get()[:n])[:8]
        assert sk.same_bytes(got[n:], X_new.h0[n:]), "written behind len"
        assert d_new.unchanged(), "delta was touched although X was given"
        # ... and with no delta at all
        X_nod = sk.DVec(torch, n, x_host)
        assert L.thallo_hip_linear_update_all(X_nod.ptr, None, terms, count, n, 0, None) == g
        assert sk.same_bytes(X_nod.get(), got)
    else:
        got = d_new.get()
        assert sk.same_bytes(got[:n], d_ref.get()[:n]), np.flatnonzero(got[:n] != d_ref.get()[:n])[:8]
        assert sk.same_bytes(got[n:], d_new.h0[n:]), "written behind len"
        assert X_new.unchanged()
    err = np.abs(got[:n].astype(np.float64) - want)
    print(f"count {count} n {n} {form} {regime}: max |err| / scale = {(err / np.maximum(scale, 1e-300)).max():.3e}")
    if regime == "exact": assert np.allclose(got[:n].astype(np.float64), want, rtol=1e-6, atol=0.0)
    else: assert (err <= 1e-6 * scale).all(), (err / np.maximum(scale, 1e-300)).max()


@pytest.mark.parametrize("n", [N_ALIGNED, N_ALIGNED + 3], ids=["aligned", "scalar"])
def test_one_pass_on_one_workgroup(torch, L, n):
    """max_workgroups = 1: every float4 (float) behind the first trip takes the grid-stride loop's path"""
    rng = np.random.default_rng([78, n])
    count = 41
    terms, planes, alphas, keep = _make_terms(torch, rng, "rounded", n, count)
    d_ref, d_new = sk.DVec(torch, n), sk.DVec(torch, n)
    _chained_reference(L, terms, count, None, d_ref, n)
    assert L.thallo_hip_linear_update_all(None, d_new.ptr, terms, count, n, 1, None) == 1
    torch.cuda.synchronize()
    assert sk.same_bytes(d_new.get(), d_ref.get())


def test_one_pass_refuses_what_it_cannot_take(torch, L):
    """more than 128 terms, a list of partials behind term 32 (either sum), no output at all: an error code, and nothing is launched -- the outputs keep their
    sentinels.  A list AT term 31 is taken (the bitwise test above has lists at 0, 5, .. 30; here the last slot that may hold one)."""
    n = N_ALIGNED
    rng = np.random.default_rng(79)
    terms, planes, alphas, keep = _make_terms(torch, rng, "rounded", n, MAX_STEP_TERMS)
    out, X = sk.DVec(torch, n), sk.DVec(torch, n, sk.rounded_vec(rng, n))
    big = (UpdateTermT * (MAX_STEP_TERMS + 1))()
    for j in range(MAX_STEP_TERMS + 1): big[j] = terms[j % MAX_STEP_TERMS]
    assert L.thallo_hip_linear_update_all(None, out.ptr, big, MAX_STEP_TERMS + 1, n, 0, None) == sk.INVALID
    assert L.thallo_hip_linear_update_all(X.ptr, out.ptr, big, MAX_STEP_TERMS + 1, n, 0, None) == sk.INVALID
    assert L.thallo_hip_linear_update_all(None, None, terms, 8, n, 0, None) == sk.INVALID
    assert L.thallo_hip_linear_update_all(None, out.ptr, terms, -1, n, 0, None) == sk.INVALID
    for at in (32, 33, 99):
        for which in ("alphaN", "alphaD"):
            t2, _, _, keep2 = _make_terms(torch, np.random.default_rng([80, at]), "rounded", n, 100)
            lst = sk.dbuf(torch, sk.rounded_sum(rng, 7, True))
            setattr(t2[at], which, sk.sumt(lst))
            assert L.thallo_hip_linear_update_all(None, out.ptr, t2, 100, n, 0, None) == sk.INVALID, (at, which)
            assert L.thallo_hip_linear_update_all(X.ptr, None, t2, 100, n, 0, None) == sk.INVALID, (at, which)
    torch.cuda.synchronize()
    assert out.unchanged() and X.unchanged(), "a refused call launched something"
    # a list at term 31: accepted, and the bits of the chain
    t3, _, _, keep3 = _make_terms(torch, np.random.default_rng(81), "rounded", n, 40, list_at=(31,))
    d_ref, d_new = sk.DVec(torch, n), sk.DVec(torch, n)
    _chained_reference(L, t3, 40, None, d_ref, n)
    assert L.thallo_hip_linear_update_all(None, d_new.ptr, t3, 40, n, 0, None) > 0
    torch.cuda.synchronize()
    assert sk.same_bytes(d_new.get(), d_ref.get())


# ------------------------------------------------------------------ the GN step
def _solve(torch, monkeypatch, p, W, H, lit, planes):
    if planes is None: monkeypatch.delenv("THALLO_DELTA_PLANES", raising=False)
    else: monkeypatch.setenv("THALLO_DELTA_PLANES", planes)
    dev = to_device(copy_params(p))
    s = api.ThalloSolver((W, H), thallo_amd.energy_file("image_warping"), timing_level=2)
    s.set_solver_parameters(nIterations=2, lIterations=lit)
    params = s.make_params(dev)
    s.init(params)
    costs, traces = [s.current_cost()], []
    while s.step(params):
        costs.append(s.current_cost()); traces.append(s.alpha_beta_trace())
    stats = {k: v["launches"] for k, v in s.kernel_stats().items()}
    s.close()
    return costs, traces, dev[0].clone(), dev[1].clone(), stats


def _delta_updates(lit, n):
    """"PCGDeltaUpdate" launches of one step of the schedule before this entry on a ring of n planes: before launch k, when plane k mod n still holds a term that
    is not in delta, everything that has its scalars goes (batches of <= 32); at the end, whatever the tail's 32 terms do not cover"""
    if lit < 3: return 0
    launches = flushed = 0
    for k in range(lit):
        if k >= n and flushed < k - n + 1:
            launches += -(-(k - 1 - flushed) // 32); flushed = k - 1
    if lit - 32 > flushed: launches += -(-(lit - 32 - flushed) // 32)
    return launches


@pytest.mark.parametrize("lit", [2, 3, 33, 34, 65, 100])
@pytest.mark.parametrize("W,H", [(132, 40), (250, 70)])
def test_step_on_a_ring_as_long_as_the_loop_is_bitwise_the_step_before(torch, monkeypatch, W, H, lit):
    p = syn.image_warping(W, H, n_markers=8, mask_disc=0.1)
    monkeypatch.setenv("THALLO_RESIDENT", "0")          # one launch per PCG iteration
    monkeypatch.setenv("THALLO_MARCH", "2")             # the marching kernels (which take any p plane) at these sizes too
    runs = {dp: _solve(torch, monkeypatch, p, W, H, lit, dp) for dp in (None, "33", "0", "17")}
    c, t, o, a, n = runs[None]
    assert all(np.isfinite(c)) and len(c) == 3 and len(t) == 2 and len(t[0]) == lit
    for dp in ("33", "0", "17"):
        c1, t1, o1, a1, n1 = runs[dp]
        assert t == t1, (dp, [(i, k) for i, (x, y) in enumerate(zip(t, t1)) for k, (u, v) in enumerate(zip(x, y)) if u != v][:3])
        assert c == c1, (dp, c, c1)
        assert torch.equal(o, o1) and torch.equal(a, a1), dp
        assert n1["PCGIteration"] == 2 * lit == n["PCGIteration"]
    print(f"{W}x{H} L {lit}: default {n}")
    # the default: at most two launches per step stand for delta; beyond 64 iterations they are the whole end of the step, up to 64 the end is the one before
    assert n.get("PCGDeltaUpdate", 0) <= 2 * 2, n
    if lit > 64: assert n.get("PCGDeltaUpdate", 0) == 2 * 2 and "PCGLinearUpdate" not in n, n
    else: assert n.get("PCGDeltaUpdate", 0) == 2 * _delta_updates(lit, lit) and n["PCGLinearUpdate"] == 2 * 2, n
    # ... the schedule before (a ring of at most 33 planes, flushed inside the loop), and in-loop flushes again on 17 planes
    n33, n17 = runs["33"][4], runs["17"][4]
    assert n33.get("PCGDeltaUpdate", 0) == 2 * _delta_updates(lit, min(lit, 33)) and n33["PCGLinearUpdate"] == 2 * 2, n33
    assert n17.get("PCGDeltaUpdate", 0) == 2 * _delta_updates(lit, min(lit, 17)) and n17["PCGLinearUpdate"] == 2 * 2, n17
    if lit > 17: assert n17["PCGDeltaUpdate"] >= 2, n17
    assert "PCGDeltaUpdate" not in runs["0"][4], runs["0"][4]
