"""The number functions of the generated kernels' prelude (csrc/dsl_codegen.cpp) one by one, through tests/energies/ops_probe.t: one unknown image per function and a
single-access residual f(X(i)) + B(i) per image, so that PCGInit1 (thallo_hip_genprobe_pcg_init) leaves r_i = -f'(x_i) (f(x_i) + b_i) and diag_i = f'(x_i)^2 -- two
elementwise observables of f and f', one product away from them.  The reference is numpy float64 on the float32-rounded inputs.

What f and f' are allowed (u = ulp of the float32 nearest the exact value; eps = 2^-24 = half an ulp relative):
  + - *         one rounding each: 0.5 u per operation (and fma contraction only removes one);
  / and sqrt    correctly rounded in HIP's default mode: 0.5 u per operation;
  abs, Select   exact (abs' = sign: 0 at +-0, +-1 at a denormal);
  sin, cos      thallo_sincosf: 1.6 u for |x| <= 1e5 -- what the comment above it claims; beyond 1e5 (the double-precision reduction) the error is RECORDED in RATIOS
                and written to profiles/generated_kernels/README.md, and held only to "finite and within [-1, 1]";
  pow           the device library's powf: 16 u, the bound OpenCL sets for pow (recorded as well).
Propagated through the two products (each rounded once, or to the smallest denormal where it underflows): |r - r_ref| <= |f'| E_F + |F| E_f' + E_f' E_F + eps |r|, with E_F = E_f + eps |f + b| (b = 0 for sin, cos, abs: the sum is exact);
|diag - diag_ref| <= 2 |f'| E_f' + E_f'^2 + eps diag.
The double build (sin, cos, pow from the device library at 2^-53 scale): 4 u for sin and cos, 16 u for pow, u the spacing of doubles.

Angles: every decade from 1e-6 to 1e5, the floats nearest k pi/2 and their neighbours on both sides (k up to 63661: 1e5), +-0 and denormals, 1e5 itself with its
neighbours, where the branch changes, and 1e6 .. 1e9 on the double branch."""
import ctypes as C
import os

import numpy as np
import pytest

import shim_kernels as sk
from generated_probe import CANARY, Handle, Switches, Vec

pytestmark = pytest.mark.gpu
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energies", "ops_probe.t")
NAMES = ["add", "sub", "mul", "div", "rcp", "sqrt", "sin", "cos", "abs", "pow", "sel"]
PW = float(np.float32(2.7))
WORST = {}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    return sk.shim()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nRATIOS  worst error of r and diag over its bound, per function; sincos beyond 1e5 in ulps of the products")
    for k, v in sorted(WORST.items()): print(f"  {k:28s} {v:10.3f}")


def angles():
    rng = np.random.default_rng(41)
    out = [np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1e-38, 1e5, -1e5], np.float32)]
    out.append(np.nextafter(np.float32(1e5), np.float32([0, np.inf, 0, np.inf])) * np.float32([1, 1, -1, -1]))
    for d in range(-6, 5):
        out.append((rng.choice([-1.0, 1.0], 192) * rng.uniform(1.0, 10.0, 192) * 10.0 ** d).astype(np.float32))
    ks = np.unique(np.concatenate([np.arange(1, 129), (2 ** np.arange(7, 16)), rng.integers(129, 63661, 160), [63660, 63661]]))
    near = (ks * (np.pi / 2)).astype(np.float32)
    near = near[near <= 1e5]
    out += [near, np.nextafter(near, np.float32(0)), np.nextafter(near, np.float32(np.inf)), -near]
    small = np.concatenate(out).astype(np.float32)
    small = small[np.abs(small) <= 1e5]
    big = np.concatenate([rng.choice([-1.0, 1.0], 48) * rng.uniform(1.0, 10.0, 48) * 10.0 ** d for d in range(5, 9)]).astype(np.float32)
    big = big[np.abs(big) > 1e5]
    return small, big


def inputs(dbl):
    small, big = angles()
    ang = np.concatenate([small, big]).astype(np.float64)
    N = ang.size
    rng = np.random.default_rng(43)
    q = (lambda a: np.asarray(a, np.float64)) if dbl else (lambda a: np.asarray(a, np.float32).astype(np.float64))
    gen = lambda: q(rng.choice([-1.0, 1.0], N) * rng.uniform(1.0, 10.0, N) * 10.0 ** rng.integers(-3, 4, N))
    X = {n: gen() for n in NAMES}
    X["sqrt"] = np.abs(X["sqrt"]); X["pow"] = q(rng.uniform(0.05, 20.0, N))
    X["sin"] = ang.copy(); X["cos"] = ang.copy()
    X["abs"][:8] = q(np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1e-38, -1e-38]))
    B, Cc = gen(), gen()
    X["sel"][::3] = Cc[::3]                                # ties: greater() is false there
    return N, small.size, X, B, np.zeros(N), Cc


def reference(X, B, Cc):
    """name -> (f, f', b, E_f in u of f, E_f' in u of f')"""
    x = X
    sel = x["sel"] > Cc
    return {
        "add": (x["add"] + Cc, np.ones_like(B), B, 0.5, 0.0),
        "sub": (Cc - x["sub"], -np.ones_like(B), B, 0.5, 0.0),
        "mul": (x["mul"] * Cc, Cc, B, 0.5, 0.0),
        "div": (x["div"] / Cc, 1 / Cc, B, 0.5, 1.5),                      # d/dx (x / c): (1 - (x / c) 0) / c as the dual division forms it: a quotient (+ the exact 0 terms)
        "rcp": (Cc / x["rcp"], -Cc / x["rcp"] ** 2, B, 0.5, 2.0),            # (0 - (c / x) 1) / x: two quotients
        "sqrt": (np.sqrt(x["sqrt"]), 1 / (2 * np.sqrt(x["sqrt"])), B, 0.5, 1.5),  # 0.5 / sqrt: the rounded root, a quotient
        "sin": (np.sin(x["sin"]), np.cos(x["sin"]), 0 * B, 1.6, 1.6),
        "cos": (np.cos(x["cos"]), -np.sin(x["cos"]), 0 * B, 1.6, 1.6),
        "abs": (np.abs(x["abs"]), np.sign(x["abs"]), 0 * B, 0.0, 0.0),
        "pow": (x["pow"] ** PW, PW * x["pow"] ** (PW - 1), B, 16.0, 17.5),    # y powf(x, y - 1): y - 1 rounded (its effect on the power: |y - 1| log(x) eps, below 1 u here), powf, a product
        "sel": (np.where(sel, x["sel"] ** 2, 2 * x["sel"]), np.where(sel, 2 * x["sel"], 2.0), B, 0.5, 0.5),
    }


@pytest.mark.parametrize("auto", [0, 1])
@pytest.mark.parametrize("dbl", [False, True])
def test_prelude_functions(torch, L, dbl, auto):
    N, n_small, X, B, Bz, Cc = inputs(dbl)
    size, eps = (8, 2.0 ** -53) if dbl else (4, 2.0 ** -24)
    ft = np.float64 if dbl else np.float32
    tiny = float(np.finfo(ft).smallest_subnormal)          # a product that underflows is rounded to a multiple of the smallest denormal (sin(1e-38)^2 is 0 in float)
    ulp = lambda v: np.spacing(np.abs(np.asarray(v, np.float64)).astype(ft)).astype(np.float64)
    with Switches():
        H = Handle(L, PATH, (N,), auto, dbl)
        try:
            keep = [torch.from_numpy(X[n].astype(ft)).cuda() for n in NAMES] + [torch.from_numpy(a.astype(ft)).cuda() for a in (B, Bz, Cc)]
            pw = C.c_float(PW)
            ptrs = (C.c_void_p * 15)(*[t.data_ptr() for t in keep], C.addressof(pw))
            assert L.thallo_hip_genprobe_n_unknowns(H.h) == 11 * N
            assert L.thallo_hip_genprobe_bind(H.h, ptrs) == 0 and L.thallo_hip_genprobe_prepare(H.h) == 0
            v = {q: Vec(torch, L, 11 * N, size) for q in ("r", "diag", "pre", "z", "p", "delta")}
            pa = torch.from_numpy(np.full(sk.MAX_PARTIALS + 8, CANARY[size], np.uint32 if size == 4 else np.uint64).view(ft).copy()).cuda()
            # the eleven residuals share one domain and every unknown image has one channel: ONE merged group writes every unknown -- the float build's store form
            assert L.thallo_hip_genprobe_whole_store(H.h) == int(auto == 1 and not dbl)
            cnt = L.thallo_hip_genprobe_pcg_init(H.h, v["r"].ptr, v["diag"].ptr, v["pre"].ptr, v["z"].ptr, v["p"].ptr, v["delta"].ptr, pa.data_ptr()); torch.cuda.synchronize()
            import thallo_amd
            assert cnt >= 1, thallo_amd.last_error()
            assert 1 <= cnt <= sk.MAX_PARTIALS and (pa.cpu().numpy().view(np.uint32 if size == 4 else np.uint64)[cnt:] == CANARY[size]).all(), "partials were written behind the count"
            for q in ("r", "diag", "delta"): v[q].check()
            v["pre"].check(ones_to_ceil4=True); v["p"].check(padding_zero=not dbl); v["z"].check(padding_zero=False)
            pre, z, p = v["pre"].body(), v["z"].body(), v["p"].body()
            assert (pre == 1.0).all() and (z == v["r"].body()).all() and (p == (z if dbl else 0.0)).all()      # UsePreconditioner(false): z = r; p: zeros in float, z in double
            r, diag = v["r"].body().reshape(11, N), v["diag"].body().reshape(11, N)
        finally:
            H.close()
    # the double build is compared with an extended-precision evaluation (x87 long double: 2^-64 per operation); where numpy has none, the float64 reference's own
    # roundings -- at most four on any path here -- are added to the bounds
    wide = dbl and np.finfo(np.longdouble).nmant >= 63
    own = 4 * eps if dbl and not wide else 0.0
    if wide: X, B, Cc = {n: a.astype(np.longdouble) for n, a in X.items()}, B.astype(np.longdouble), Cc.astype(np.longdouble)
    ref = reference(X, B, Cc)
    prec = "f64" if dbl else "f32"
    failures = []
    for k, name in enumerate(NAMES):
        f, fp, b, uf, ufp = ref[name]
        if dbl and name in ("sin", "cos"): uf = ufp = 4.0
        with np.errstate(all="ignore"):
            F = f + b
            EF = uf * ulp(f) + (eps * np.abs(F) if np.any(b) else 0.0)
            Efp = ufp * ulp(fp)
            want_r, want_d = -fp * F, fp * fp
            bound_r = np.abs(fp) * EF + np.abs(F) * Efp + EF * Efp + (eps + own) * np.abs(want_r) + tiny
            bound_d = 2 * np.abs(fp) * Efp + Efp ** 2 + (eps + own) * want_d + tiny
        er, ed = np.abs(r[k] - want_r).astype(np.float64), np.abs(diag[k] - want_d).astype(np.float64)
        bound_r, bound_d, want_r, want_d = (np.asarray(a, np.float64) for a in (bound_r, bound_d, want_r, want_d))
        held = np.ones(N, bool)
        if name in ("sin", "cos") and not dbl:
            held[n_small:] = False                         # beyond 1e5: recorded
            big = ~held
            assert np.isfinite(r[k][big]).all() and (np.abs(r[k][big]) <= 1.0).all() and (diag[k][big] <= 1.0).all()
            WORST[f"{name} {prec} auto{auto} |x|>1e5 r/u"] = float((er[big] / ulp(np.maximum(np.abs(want_r[big]), 1e-30))).max())
            WORST[f"{name} {prec} auto{auto} |x|>1e5 diag/u"] = float((ed[big] / ulp(np.maximum(want_d[big], 1e-30))).max())
        wr, wd = float((er[held] / bound_r[held]).max()), float((ed[held] / bound_d[held]).max())
        WORST[f"{name} {prec} auto{auto} r"] = wr; WORST[f"{name} {prec} auto{auto} diag"] = wd
        print(f"{name:5s} {prec} auto{auto}: worst r error / bound {wr:.3f}, diag {wd:.3f}")
        if name in ("sin", "cos") and not dbl:           # per decade of |x|, for profiles/generated_kernels/README.md
            ax = np.abs(np.asarray(X[name], np.float64)); dec = np.floor(np.log10(np.maximum(ax, 1e-7))).astype(int)
            print("   per decade of |x| (r, diag):", "  ".join(f"1e{d}: {(er / bound_r)[held & (dec == d)].max():.2f} {(ed / bound_d)[held & (dec == d)].max():.2f}" for d in sorted(set(dec[held]))))
        if wr > 1.0 or wd > 1.0:
            i = int(np.argmax(np.where(held, er / bound_r, 0))); failures.append((name, wr, wd, float(X[name][i]), float(r[k][i]), float(want_r[i])))
    assert not failures, failures
