"""The head of thallo_hip_linear_update_n (csrc/pcg_kernels.hip update_alphas: every alpha_j of a launch behind one round trip -- single words by lane j of wave 0,
lists of partials by wave j mod 4), its "delta is zero" entry thallo_hip_linear_update_n_from_zero, the GN step that uses it (PCGInit1 stores no zeros into delta, the
ring schedule's first update of delta starts from 0.0f: THALLO_AB=delta_first_touch=0 restores the zero fill), and the coarse timers' shared event records.

Kernel level, through tests/shim_kernels.py: both entries at 1, 2, 5, 31 and 32 terms whose sums are all words, all lists, or mixed, at list lengths 2, 63, 64, 65, 251
and THALLO_MAX_PARTIALS; n = 4 * 256 * 3 + 4 (float4 path: four workgroups, the last one with a single busy lane) and n - 1 (scalar path); with and without X;
max_workgroups 0 and 1 (one workgroup: four grid-stride trips).  EXACT regime: equality with sk.ref_linear_update_n; ROUNDED: within sk.tol (k = terms, + 1 with X).
alpha_j comes bit-exactly from sk.sum_partials / sk.div32, so N terms at once must equal N single-term calls bitwise in both regimes."""
import ctypes as C

import numpy as np
import pytest

import shim_kernels as sk
from shim_kernels import F32

pytestmark = pytest.mark.gpu

N_VEC = 4 * 256 * 3 + 4
LIST_LENGTHS = [2, 63, 64, 65, 251, sk.MAX_PARTIALS]
ALPHAS_EXACT = [(1.0, 2.0), (3.0, 4.0), (-2.0, 8.0), (6.0, 4.0)]      # alpha_j from {1/2, 3/4, -1/4, 3/2}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    lib = sk.shim()
    f = lib.thallo_hip_linear_update_n_from_zero
    f.argtypes = [C.c_void_p, C.c_void_p, sk.UpdateTermsT, C.c_long, C.c_int, C.c_void_p]
    f.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def cus(L):
    return L.thallo_hip_device_cu_count()


def _sum_lengths(kind, j, count):
    """(partials of alphaN_j, of alphaD_j): 1 = a plain word"""
    ln = LIST_LENGTHS[(j + count) % 6], LIST_LENGTHS[(j + count + 3) % 6]
    if kind == "words": return 1, 1
    if kind == "lists": return ln
    return [(1, 1), (ln[0], 1), (1, ln[1]), ln][j % 4]


def _terms(torch, rng, regime, n, count, kind):
    T = sk.UpdateTermsT(); T.count = count
    planes, alphas, keep = [], [], []
    for j in range(count):
        cn, cd = _sum_lengths(kind, j, count)
        p = sk.DVec(torch, n, (sk.exact_vec if regime == "exact" else sk.rounded_vec)(rng, n))
        if regime == "exact": parts = [sk.exact_sum(rng, cn, ALPHAS_EXACT[j % 4][0]), sk.exact_sum(rng, cd, ALPHAS_EXACT[j % 4][1])]
        else: parts = [sk.rounded_sum(rng, cn, True), sk.rounded_sum(rng, cd, True) * 16]
        ts = [sk.dbuf(torch, q) for q in parts]
        keep.append((ts, parts))
        T.p[j] = p.ptr; T.alphaN[j] = sk.sumt(ts[0]); T.alphaD[j] = sk.sumt(ts[1])
        planes.append(p); alphas.append(sk.div32(sk.sum_partials(parts[0]), sk.sum_partials(parts[1]), True))
    return T, planes, alphas, keep


def _check(regime, got, want, k, scale):
    if regime == "exact": assert (want == want.astype(F32)).all() and np.array_equal(got, want.astype(F32)), np.flatnonzero(got != want.astype(F32))[:8]
    else: assert (np.abs(got.astype(np.float64) - want) <= sk.tol(k, scale)).all()


@pytest.mark.parametrize("regime", ["exact", "rounded"])
@pytest.mark.parametrize("path", ["vector", "scalar"])
@pytest.mark.parametrize("kind", ["words", "lists", "mixed"])
@pytest.mark.parametrize("count", [1, 2, 5, 31, 32])
def test_all_alphas_behind_one_round_trip(torch, L, cus, count, kind, path, regime):
    n = N_VEC if path == "vector" else N_VEC - 1
    c4 = sk.ceil4(n)
    rng = np.random.default_rng([41, count, len(kind), n, regime == "exact"])
    gen = sk.exact_vec if regime == "exact" else sk.rounded_vec
    T, planes, alphas, keep = _terms(torch, rng, regime, n, count, kind)
    pf = [p.h0[:n].astype(np.float64) for p in planes]
    terms_scale = sum(np.abs(float(a) * q) for a, q in zip(alphas, pf))
    g = sk.flat_grid(n // 4 if path == "vector" else n, 2 * cus)
    assert g > 1
    d_host, x_host = gen(rng, n), gen(rng, n)
    for mw in (0, 1):
        for with_X in (False, True):
            # ---- the plain entry against the float64 reference and against the same terms one call at a time
            delta, X, single = sk.DVec(torch, n, d_host), sk.DVec(torch, n, x_host), sk.DVec(torch, n, d_host)
            ret = L.thallo_hip_linear_update_n(X.ptr if with_X else None, delta.ptr, T, n, mw, None)
            for j in range(count):
                T1 = sk.UpdateTermsT(); T1.count = 1; T1.p[0] = T.p[j]; T1.alphaN[0] = T.alphaN[j]; T1.alphaD[0] = T.alphaD[j]
                assert L.thallo_hip_linear_update_n(None, single.ptr, T1, n, mw, None) > 0
            # ---- "delta is zero": a delta full of NaN through the new entry against stored zeros through the plain one
            dnan, Xz = sk.DVec(torch, n), sk.DVec(torch, n, x_host)
            dzero, X0 = sk.DVec(torch, n, np.zeros(n, F32)), sk.DVec(torch, n, x_host)
            retz = L.thallo_hip_linear_update_n_from_zero(Xz.ptr if with_X else None, dnan.ptr, T, n, mw, None)
            assert L.thallo_hip_linear_update_n(X0.ptr if with_X else None, dzero.ptr, T, n, mw, None) == retz
            torch.cuda.synchronize()
            assert ret == retz == (min(g, mw) if mw else g), (ret, retz, g, mw)
            for v in planes + [delta, X, single, dnan, Xz, dzero, X0]: assert v.canary_ok(), "the canary behind a vector changed"
            for p in planes: assert p.unchanged(), "a plane changed"
            for ts, parts in keep:
                for t, q in zip(ts, parts): assert sk.same_bytes(t.cpu().numpy(), q)
            d0, x0 = d_host.astype(np.float64), x_host.astype(np.float64)
            Xw, dw = sk.ref_linear_update_n(x0 if with_X else None, d0, pf, alphas)
            Xwz, dwz = sk.ref_linear_update_n(x0 if with_X else None, np.zeros(n), pf, alphas)
            if with_X:
                _check(regime, X.get()[:n], Xw, count + 1, np.abs(x0) + np.abs(d0) + terms_scale)
                _check(regime, Xz.get()[:n], Xwz, count + 1, np.abs(x0) + terms_scale)
                assert delta.unchanged() and dzero.unchanged(), "delta was written although X was given"
                assert dnan.unchanged(), "the zero-flag entry touched delta although X was given"
                assert sk.same_bytes(X.get()[:n], (x_host + single.get()[:n]).astype(F32)), "N terms at once differ from N single-term calls"
                assert sk.same_bytes(Xz.get(), X0.get()), "starting from 0.0f differs from reading stored zeros"
            else:
                _check(regime, delta.get()[:n], dw, count, np.abs(d0) + terms_scale)
                _check(regime, dnan.get()[:n], dwz, count, terms_scale)
                assert X.unchanged()
                assert sk.same_bytes(delta.get(), single.get()), "N terms at once differ from N single-term calls"
                assert sk.same_bytes(dnan.get()[:n], dzero.get()[:n]), "starting from 0.0f differs from reading stored zeros"
                assert sk.same_bytes(dnan.get()[n:], dnan.h0[n:]), "the zero-flag entry wrote behind len"
                assert sk.same_bytes(delta.get()[n:c4], delta.h0[n:c4])
