"""The kernels csrc/dsl_codegen.cpp generates, one operation at a time (thallo_hip_genprobe_*: cost, PCGInit1, applyJTJ of the plugin a plan would get) against the
float64 reference of tests/generated_reference.py -- F in numpy on the float32-rounded inputs, J by complex-step differentiation.

Per (energy, lowering): cost (the ordered sum of the partials), r, the raw diagonal, pre, z, p, delta == 0, alphaN, Ap for a dense random p and for a p spanning six
decades, alphaD; excluded unknowns and the padding behind the last unknown exactly 0; lowerings without atomics bit-identical from call to call; every lowering of
one energy within twice the bound of every other.  Every vector has a NaN canary behind it that is compared as bytes after every call.

Bounds.  Elementwise (gamma_m + k_eval eps) x companion: m = the terms accumulated into the unknown, counted from the reference's J (+ 1 for the product; for Ap + the
longest row and one more product), companions |J|^T |F|, sum J^2 and |J|^T |J| |p|, eps = 2^-24 (float build) or 2^-53 (double build).  k_eval covers the float
evaluation of the residual and its partials: for the linear energies the operation count of the longest chain in the .t file (stated next to the factory in
generated_reference.py); for the nonlinear ones twice the worst error / (eps x companion) an MI355X run recorded (generated_reference.K_EVAL_MEASURED;
profiles/generated_kernels/README.md has the table, printed again at the end of this module as RATIOS).  An energy without a recorded figure is measured and
reported, not held: nobody has measured it yet.
pre: (bound_diag / diag + 4 eps) pre (sqrt, sum, square, reciprocal); z: pre bound_r + |r| bound_pre + eps |z|.
cost (linear energies; a nonlinear one: 1 eps for the final rounding + twice its own recorded cost figure): (gamma_64 + 2 k_eval eps) cost -- one partial adds at most 16 squares per thread (the merged cost kernel of four four-channel residuals) + 6 butterfly levels
+ 4 waves at these sizes (asserted: one visit per thread), the ordered sum at most 16 + 6 more; F^2 carries F's relative error twice.
alphaN / alphaD: the sum of the partials in the documented order against the float64 dot product of the DEVICE's own vectors, gamma_c of sum |terms|, c from
shim_kernels.chain_length + the ordered sum.

Lowerings: residual-wise with THALLO_AB=frontend_aggregate=0 and =1; the stencil gather / merged group kernels with frontend_preload=1 and =0; the index-map gather
at inc_lanes = 1, 2, 4, 16, 64; appended schedule lines J / JtJ (dense, and sparse under THALLO_DENSE_JTJ_MAX=0) / Jp:set_materialize; the row-slab unit (first,
middle, last slab, one row, `ghost` rows; owned rows compared); doublePrecision = 1 for every file that allows it.  schedule_name() and the launched kernels' names
say which lowering ran.

Which form ran is asserted per case from the names of the kernels the case launched (the probe reports them), from schedule_name() and, for the `whole_` store form
of the merged kernels, from thallo_hip_genprobe_whole_store and the number of partials applyJTJ returns.  Every kind of kernel these plugins hold is launched by
some case (test_every_kind_of_generated_kernel_was_launched), except jtfg_ / jtjg_ (NEVER_LAUNCHED below says why).  The one-wave-per-owner form and the lane
count are launch arguments, not names: they follow from the documented thresholds, stated at the cases.  The bundled arap_mesh_deformation, bundle_adjustment and shape_from_shading take J and F from the float64 restatements the hand-written kernels' tests use
(graph_reference.py, ba_reference.py, sfs_reference.py).  shape_from_shading, the radius-two stencil, also runs on 2 x 5, 5 x 2 and 33 x 7: images smaller than it."""
import ctypes as C
import os

import numpy as np
import pytest

import generated_reference as gr
import shim_kernels as sk
import collections

from generated_probe import CANARY, Handle, Switches, Vec

pytestmark = pytest.mark.gpu

RATIOS = {}          # (energy, precision) -> {quantity: worst error / (eps x companion)}
SEEN = {}            # (energy, shape, precision) -> {lowering: {quantity: array}}: the cross-lowering comparison
M_COST = 64


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "these tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def L(torch):
    return sk.shim()


@pytest.fixture(scope="module", autouse=True)
def ratios_report():
    yield
    print("\nRATIOS  worst error / (eps x companion), eps = 2^-24 (f32) or 2^-53 (f64)")
    for (name, prec), q in sorted(RATIOS.items()):
        print(f"  {name:20s} {prec}  " + "  ".join(f"{k} {v:8.2f}" for k, v in sorted(q.items())))


@pytest.fixture(scope="module")
def handles(L):
    cache = {}
    yield cache
    for h in cache.values(): h.close()


def upload(torch, e):
    """the parameters as Thallo_ProblemInit takes them: device arrays (floats, or doubles in the double build; fixed-float arrays floats in both), host scalars"""
    keep, ptrs = [], (C.c_void_p * len(e.params))()
    for k, p in enumerate(e.params):
        if isinstance(p, np.ndarray):
            a = p if p.dtype.kind in "iu" else p.astype(np.float64 if e.dbl and k not in e.f32_slots else np.float32)          # (Sparse maps and uint8 masks as they are)
            t = torch.from_numpy(np.ascontiguousarray(a)).cuda(); keep.append(t); ptrs[k] = t.data_ptr()
        else:
            c = C.c_float(p); keep.append(c); ptrs[k] = C.addressof(c)
    return keep, ptrs


def record(e, what, err, comp):
    ok = comp > 0
    if ok.any():
        q = RATIOS.setdefault((e.name, "f64" if e.dbl else "f32"), {})
        q[what] = max(q.get(what, 0.0), float((err[ok] / (e.eps * comp[ok])).max()))


def held(e, k, what, got, want, bound, comp):
    """record the ratio; hold the quantity to its bound when k_eval is known (linear, or measured), exactly 0 where the companion is 0"""
    err = np.abs(got - want)
    record(e, what, err, comp)
    assert (got[comp == 0] == 0).all(), (what, "not 0 where nothing contributes")
    if k is not None:
        bad = err > bound
        assert not bad.any(), (e.name, what, np.flatnonzero(bad)[:8], float((err[bad] / np.maximum(bound[bad], 1e-300)).max()))


Ran = collections.namedtuple("Ran", "name launched handle apply_count")      # what run_case returns: schedule name, kinds of kernel launched by the case, its handle
kind = lambda n: n.split("_")[0]


def k_of(e):
    return gr.k_eval(e)


def run_case(torch, L, handles, factory, args, lowering, auto, ab="", dense_max=None, dbl=False, extra=None, tmp_path=None, expect=None, slab=None, unit=None, whole=None):
    R = gr.reference(factory, *args, dbl=dbl)
    e = R.energy
    size = 8 if dbl else 4
    path = e.path
    if extra:
        path = str(tmp_path / e.file); open(path, "w").write(open(e.path).read() + "\n" + extra)
    with Switches(ab, dense_max):
        key = (e.name, args, dbl, unit or lowering)          # (unit: lowerings that differ only in what the library reads after the plugin is made share its handle)
        if key not in handles: handles[key] = Handle(L, path, e.dims, auto, dbl)
        h = handles[key].h
        handles[key].kernels(2)                                                # (this case's launches start here)
        name = L.thallo_hip_genprobe_schedule_name(h).decode()
        assert L.thallo_hip_genprobe_n_unknowns(h) == e.n and L.thallo_hip_genprobe_use_preconditioner(h) == int(e.precond), (e.n, e.precond)
        keep, ptrs = upload(torch, e)
        assert L.thallo_hip_genprobe_bind(h, ptrs) == 0 and L.thallo_hip_genprobe_prepare(h) == 0
        rows = None
        if slab is not None:
            W, H = e.dims[0], e.dims[1]
            g = L.thallo_hip_genprobe_slab_ghost_rows(h); assert g >= 1
            row0, row1 = {"first": (0, min(H, max(1, H // 3))), "middle": (H // 3, max(H // 3 + 1, 2 * H // 3)), "last": (2 * H // 3, H), "one_row": (H // 2, H // 2 + 1),
                          "ghost_rows": (min(g, H - 1), min(2 * g, H))}[slab]
            assert L.thallo_hip_genprobe_set_slab_global(h, 0, H) == 0 and L.thallo_hip_genprobe_set_row_slab(h, row0, row1) == 0
            per_row = e.n // H
            rows = np.zeros(e.n, bool); rows[row0 * per_row:row1 * per_row] = True
        k = k_of(e)
        own = np.ones(e.n, bool) if rows is None else rows
        out = {}
        vec = lambda payload=None: Vec(torch, L, e.n, size, payload)
        part = lambda: torch.from_numpy(np.full(sk.MAX_PARTIALS + 8, CANARY[size], np.uint32 if size == 4 else np.uint64).view(np.float32 if size == 4 else np.float64).copy()).cuda()
        fsum = (lambda a: float(sk.sum_partials_f64(a))) if dbl else (lambda a: float(sk.sum_partials(a)))

        def partials(buf, cnt):
            hst = buf.cpu().numpy()
            assert 1 <= cnt <= sk.MAX_PARTIALS
            w = hst.view(np.uint32 if size == 4 else np.uint64)
            assert (w[cnt:] == CANARY[size]).all(), "partials were written behind the count"
            return hst[:cnt]

        # ---- cost
        if rows is None and R.Fx.size <= 30000:
            pc = part(); cnt = L.thallo_hip_genprobe_cost(h, pc.data_ptr()); torch.cuda.synchronize()
            cost = fsum(partials(pc, cnt))
            # (at most 30000 instances: one visit per thread of every cost launch, M_COST holds; the grid-striding cost launch has its own case)
            record(e, "cost", np.array([abs(cost - R.cost)]), np.array([R.cost]))
            # linear: derived (above).  Nonlinear: the final rounding of the ordered sum (derived: 1 eps) + twice the energy's own recorded cost figure
            if k is not None and k.get("cost", 0) is None: assert abs(cost - R.cost) <= (R.gamma(M_COST) + 2 * k["r"] * e.eps) * R.cost, (cost, R.cost)
            elif k is not None and "cost" in k: assert abs(cost - R.cost) <= (1 + k["cost"]) * e.eps * R.cost, (cost, R.cost)
        # ---- PCGInit1
        def init():
            v = {q: vec() for q in ("r", "diag", "pre", "z", "p", "delta")}; pa = part()
            cnt = L.thallo_hip_genprobe_pcg_init(h, v["r"].ptr, v["diag"].ptr, v["pre"].ptr, v["z"].ptr, v["p"].ptr, v["delta"].ptr, pa.data_ptr()); torch.cuda.synchronize()
            import thallo_amd
            assert cnt >= 1, thallo_amd.last_error()
            for q in ("r", "diag", "delta"): v[q].check()
            v["pre"].check(ones_to_ceil4=True)
            v["p"].check(padding_zero=not dbl); v["z"].check(padding_zero=False)          # (z is written up to the last unknown; the double build's p = z likewise)
            return v, partials(pa, cnt)
        v, aN = init()
        name = L.thallo_hip_genprobe_schedule_name(h).decode()              # (the instance lists are built by the first PCGInit1: a few_owners fall-back shows now)
        r, diag, pre, z = (v[q].body() for q in ("r", "diag", "pre", "z"))
        bd_r, bd_d = (R.bound_r(k["r"]), R.bound_diag(k["diag"])) if k is not None else (None, None)
        zero = lambda a: np.where(own, a, 0.0)
        held(e, k, "r", r[own], R.r[own], None if k is None else bd_r[own], R.comp_r[own])
        held(e, k, "diag", diag[own], R.diag[own], None if k is None else bd_d[own], R.diag[own])
        assert (r[~e.free] == 0).all() and (diag[~e.free] == 0).all(), "an excluded unknown received a scatter"
        with np.errstate(divide="ignore", invalid="ignore"):
            rel_d = np.where(R.diag > 0, (bd_d if k is not None else 0.0) / np.where(R.diag > 0, R.diag, 1.0), 0.0)
        bd_pre = (rel_d + 4 * e.eps) * R.pre
        if e.precond:
            if k is not None: assert (np.abs(pre - R.pre)[own] <= bd_pre[own]).all(), "pre"
        else: assert (pre[own] == 1.0).all()
        assert (pre[own & (R.diag == 0)] == 1.0).all()
        if k is not None:
            bd_z = R.pre * bd_r + np.abs(R.r) * bd_pre + e.eps * np.abs(R.z)
            assert (np.abs(z - R.z)[own] <= bd_z[own]).all(), "z"
        assert (v["delta"].host()[:e.n] == 0).all()
        p_left = v["p"].host()[:e.n]
        if dbl: assert p_left.tobytes() == v["z"].host()[:e.n].tobytes()
        else: assert (p_left == 0).all()
        c = sk.chain_length(sk.ceil4(e.n), 1) + len(aN) // 64 + 7
        terms = (r * z)[own]
        assert abs(fsum(aN) - terms.sum()) <= R.gamma(c) * np.abs(terms).sum(), ("alphaN", fsum(aN), terms.sum())
        out.update(r=zero(r), diag=zero(diag))
        # ---- applyJTJ
        def apply(p):
            pv, Ap, pa = vec(p), vec(), part()
            cnt = L.thallo_hip_genprobe_apply_jtj(h, pv.ptr, Ap.ptr, pa.data_ptr()); torch.cuda.synchronize()
            import thallo_amd
            assert cnt >= 1, thallo_amd.last_error()
            Ap.check(padding_zero=False); assert pv.host().tobytes() == pv.h0.tobytes(), "p changed"
            return Ap, partials(pa, cnt)
        P = gr.probe_vectors(e.n, 1)
        for regime, p in P.items():
            Ap, aD = apply(p)
            a = Ap.body()
            asm = name in ("dense [JtJ]p", "sparse [[Jt][J]]p")
            held(e, k, "Ap_" + regime, a[own], R.Ap(p)[own], None if k is None else R.bound_Ap(k["Ap"], p, asm)[own], R.comp_Ap(p)[own])
            assert (a[~e.free] == 0).all(), "an excluded unknown received a scatter"
            if rows is not None: assert (a[~own] == 0).all(), "Ap outside the owned rows"
            terms = (p * a)[own]
            assert abs(fsum(aD) - terms.sum()) <= R.gamma(sk.chain_length(sk.ceil4(e.n), 1) + len(aD) // 64 + 7) * np.abs(terms).sum(), ("alphaD", regime)
            out["Ap_" + regime] = zero(a)
        # ---- no atomics: the same bits again
        if name == GATHER or slab is not None and "wide" not in e.name:
            v2, aN2 = init()
            for q in ("r", "diag", "pre", "z"): assert v2[q].host()[:e.n][own].tobytes() == v[q].host()[:e.n][own].tobytes(), (q, "differs between two calls")
            assert aN2.tobytes() == aN.tobytes()
            Ap2, aD2 = apply(P["decades"])
            assert Ap2.host()[:e.n].tobytes() == Ap.host()[:e.n].tobytes() and aD2.tobytes() == aD.tobytes()
        # ---- every lowering of one energy within twice the bound of every other
        if rows is None and k is not None:
            seen = SEEN.setdefault((e.name, args, dbl), {})
            bounds = {"r": bd_r, "diag": bd_d, "Ap_random": R.bound_Ap(k["Ap"], P["random"], True), "Ap_decades": R.bound_Ap(k["Ap"], P["decades"], True)} if seen else {}
            for other, o in seen.items():
                for q in bounds: assert (np.abs(o[q] - out[q]) <= 2 * bounds[q]).all(), (q, lowering, other)
            seen[lowering] = out
        if expect is not None: assert name.split(";")[0] == expect, (name, expect)          # ("; N computed array(s) materialized ..." may follow)
        launched = {kind(n) for n in handles[key].kernels(2)}
        is_whole = L.thallo_hip_genprobe_whole_store(h)
        print(f"{e.name}{args} {lowering}: {name}; whole {is_whole}; launched {sorted(launched)}")
        if whole is not None:
            # the `whole_` store form: the plugin says so, and its applyJTJ returns one partial per workgroup of the group kernel (alphaD rides along: no dot launch)
            assert is_whole == whole, (is_whole, whole)
            if whole: assert len(aD) == min((group_elems(e) + 255) // 256, sk.MAX_PARTIALS), len(aD)
        return Ran(name, launched, handles[key], len(aD))


def group_elems(e):
    """elements of the image domain the merged group kernel of a stencil energy runs over"""
    return e.dims[0] * e.dims[1]


STENCIL = [(gr.gradient_paste, (14, 11)), (gr.gradient_paste, (1, 9)), (gr.gradient_paste, (9, 1)), (gr.gradient_paste, (67, 3)),
           (gr.weighted_laplacian, (40, 28)), (gr.weighted_laplacian, (2, 2)), (gr.volume_arap, ()), (gr.flow_sample, (28, 20)), (gr.flow_sample, (3, 2)),
           (gr.image_warping, (19, 13)), (gr.image_warping, (65, 6)),
           (gr.shape_from_shading, (19, 13)), (gr.shape_from_shading, (65, 6)), (gr.shape_from_shading, (2, 5)), (gr.shape_from_shading, (5, 2)), (gr.shape_from_shading, (33, 7))]
ident = lambda c: c[0].__name__ + "".join(f"-{a}" for a in c[1])
GATHER = "per residual, unknown-wise (gather)"


INDEXED = [(gr.cotan_smooth, ()), (gr.robust_plane, ()), (gr.embedded_nodes, ()), (gr.graph2d, ()), (gr.sparse_exclude, ()), (gr.arap_mesh, ()), (gr.bundle_adjustment, ())]
FEW_OWNERS = [(gr.two_domains, (100, 37)), (gr.two_domains, (64, 5)), (gr.two_domains, (7, 30))]
ONE_WAVE = (gr.two_domains, (300, 260))
FLOAT_ONLY = [(gr.row_gain, (100, 37)), (gr.row_gain, (64, 5)), (gr.row_gain, (7, 30)), (gr.conv1d, ()), (gr.layer_sample, (28, 20)), (gr.layer_sample, (3, 2)),
              (gr.lp_smooth, (33,)), (gr.lp_smooth, (2,))]
WHOLE = (gr.gradient_paste, gr.weighted_laplacian)          # one group, every residual, every channel of the one unknown image: the store form


@pytest.mark.parametrize("agg", [0, 1])
@pytest.mark.parametrize("case", STENCIL + INDEXED + FEW_OWNERS + FLOAT_ONLY + [(gr.conv2d_wide, ())], ids=ident)
def test_residual_wise(torch, L, handles, case, agg):
    ran = run_case(torch, L, handles, case[0], case[1], f"rw_agg{agg}", 0, ab=f"frontend_aggregate={agg}", whole=0)
    assert ran.name.split(";")[0] == "per residual", ran.name          # (shape_from_shading: "; 2 computed array(s) materialized ..." follows)
    assert {"cost", "jtf"} <= ran.launched and not ran.launched & {"jtfgrp", "jtjgrp", "jtfn", "jtjn"}, ran.launched


@pytest.mark.parametrize("preload", [1, 0])
@pytest.mark.parametrize("case", STENCIL, ids=ident)
def test_stencil_gather(torch, L, handles, case, preload):
    ran = run_case(torch, L, handles, case[0], case[1], f"gather_preload{preload}", 1, ab=f"frontend_preload={preload}", expect=GATHER, whole=1 if case[0] in WHOLE else None)
    assert {"jtfgrp", "jtjgrp"} <= ran.launched and not ran.launched & {"jtf", "jtj"}, ran.launched


@pytest.mark.parametrize("case", FLOAT_ONLY, ids=ident)
def test_autoscheduled_float_only_files(torch, L, handles, case):
    """row_gain.t (the unknown invariant in the inner dimension), conv1d.t (expanded Sum, Jp materialized by the file), layer_sample.t (SampledImageArray)"""
    ran = run_case(torch, L, handles, case[0], case[1], "auto", 1)
    assert ran.name.startswith("per residual")


@pytest.mark.parametrize("computed", [1, 0])
@pytest.mark.parametrize("shape", [(19, 13), (65, 6)])
def test_computed_arrays(torch, L, handles, shape, computed):
    """shape_from_shading.t: B_I and its partials materialized by precompute_ kernels (frontend_computed=1, the default) or inlined at every access (=0)"""
    ran = run_case(torch, L, handles, gr.shape_from_shading, shape, f"computed{computed}", 1, ab=f"frontend_computed={computed}")
    assert ("precompute" in ran.launched) == bool(computed) and ("computed array" in ran.name) == bool(computed), (ran.name, ran.launched)


def test_wide_chunked_lowering(torch, L, handles):
    """conv2d_wide.t under the autoscheduler: 121 unknown accesses per instance -- the wide lowering scatters, the regulariser gathers"""
    run_case(torch, L, handles, gr.conv2d_wide, (), "auto", 1, expect="per residual, some unknown-wise (gather)")


@pytest.mark.parametrize("lanes", [1, 2, 4, 16, 64])
@pytest.mark.parametrize("case", INDEXED, ids=ident)
def test_index_map_gather(torch, L, handles, case, lanes):
    """short instance lists (fewer than 16 per owner on average): a group of `lanes` lanes per owner.  cotan_smooth's vertex (0, 0) is in no edge: an empty list."""
    ran = run_case(torch, L, handles, case[0], case[1], f"lanes{lanes}", 1, ab=f"inc_lanes={lanes}", unit="index_map", expect=GATHER)
    assert {"jtfn", "jtjn"} <= ran.launched and not ran.launched & {"jtf", "jtj"}, ran.launched


@pytest.mark.parametrize("case", FEW_OWNERS, ids=ident)
def test_few_owners_fall_back(torch, L, handles, case):
    """two_domains.t at sizes where one owner group has fewer than 256 owners with at least 16 instances each: build_incidence takes the product-domain residual back,
    its residual-wise kernels run (no jtfn_ / jtjn_ launch), the regulariser still gathers"""
    ran = run_case(torch, L, handles, case[0], case[1], "auto", 1, expect="per residual, some unknown-wise (gather)")
    assert {"uidx", "jtf", "jtj"} <= ran.launched and not ran.launched & {"jtfn", "jtjn"}, ran.launched


def test_one_wave_per_owner(torch, L, handles):
    """two_domains.t on 300 x 260: S has 260 owners with 300 instances each, P 300 owners with 261 -- both groups have at least 256 owners and at least 16 instances
    per owner, so every owner gets a wave (inc_lanes does not apply)"""
    ran = run_case(torch, L, handles, ONE_WAVE[0], ONE_WAVE[1], "auto", 1, expect=GATHER)
    assert {"jtfn", "jtjn"} <= ran.launched and not ran.launched & {"jtf", "jtj"}, ran.launched


@pytest.mark.parametrize("auto", [0, 1])
@pytest.mark.parametrize("case", [c for c in STENCIL + INDEXED + FEW_OWNERS + [(gr.conv2d_wide, ())] if c[0] is not gr.graph2d], ids=ident)      # (graph2d.t declares `float`)
def test_double_build(torch, L, handles, case, auto):
    run_case(torch, L, handles, case[0], case[1], f"f64_auto{auto}", auto, dbl=True, whole=0)


LINES = {"J": ("r.fit.J:set_materialize(true)\nr.regx.J:set_materialize(true)\nr.regy.J:set_materialize(true)\n", None, "per residual"),
         "Jp": ("r.regx.Jp:set_materialize(true)\nr.regy.Jp:set_materialize(true)\n", None, "per residual"),
         "J_and_Jp": ("r.fit.J:set_materialize(true)\nr.regx.J:set_materialize(true)\nr.regx.Jp:set_materialize(true)\nr.regy.J:set_materialize(true)\n", None, "per residual"),
         "JtJ_dense": ("".join(f"r.{n}.J:set_materialize(true)\nr.{n}.JtJ:set_materialize(true)\n" for n in ("fit", "regx", "regy")), 4096, "dense [JtJ]p"),
         "JtJ_sparse": ("".join(f"r.{n}.J:set_materialize(true)\nr.{n}.JtJ:set_materialize(true)\n" for n in ("fit", "regx", "regy")), 0, "sparse [[Jt][J]]p")}


@pytest.mark.parametrize("shape", [(14, 9), (2, 2)])
@pytest.mark.parametrize("lines", sorted(LINES))
def test_schedule_lines(torch, L, handles, tmp_path, lines, shape):
    """weighted_laplacian.t with schedule lines appended: materialized J (ELL rows), J^T J dense and sparse, Jp"""
    extra, dense_max, expect = LINES[lines]
    run_case(torch, L, handles, gr.weighted_laplacian, shape, lines, 0, dense_max=dense_max, extra=extra, tmp_path=tmp_path, expect=expect)


@pytest.mark.parametrize("slab", ["first", "middle", "last", "one_row", "ghost_rows"])
@pytest.mark.parametrize("case", [(gr.gradient_paste, (14, 11)), (gr.weighted_laplacian, (40, 28)), (gr.conv2d_wide, ()), (gr.shape_from_shading, (19, 13))], ids=ident)
def test_row_slab_unit(torch, L, handles, case, slab):
    """the slab unit on one device: the whole image local (global row 0, H global rows), owned rows [row0, row1); owned rows compared"""
    run_case(torch, L, handles, case[0], case[1], "slab", 1, slab=slab)


def test_cost_launch_grid_strides(torch, L, handles):
    """two_domains.t on 2100 x 64: 134400 instances of the product-domain residual, more than the (THALLO_HIP_MAX_PARTIALS / 2 residuals) x 256 = 131072 its cost launch
    covers in one pass.  The reference is vectorised (no J).  One partial: two visits of three operations, 6 + 4 levels; the ordered sum 16 + 6: M_COST holds."""
    e = gr.two_domains(2100, 64)
    want = 0.5 * float((e.F(e.x0) ** 2).sum())
    assert e.dims[0] * e.dims[1] > (sk.MAX_PARTIALS // 2) * 256
    with Switches():
        H = Handle(L, e.path, e.dims, 0, False)
        try:
            keep, ptrs = upload(torch, e)
            assert L.thallo_hip_genprobe_bind(H.h, ptrs) == 0 and L.thallo_hip_genprobe_prepare(H.h) == 0
            pc = torch.from_numpy(np.full(sk.MAX_PARTIALS + 8, CANARY[4], np.uint32).view(np.float32).copy()).cuda()
            cnt = L.thallo_hip_genprobe_cost(H.h, pc.data_ptr()); torch.cuda.synchronize()
            hst = pc.cpu().numpy()
        finally:
            H.close()
    assert 1 <= cnt <= sk.MAX_PARTIALS and (hst.view(np.uint32)[cnt:] == CANARY[4]).all()
    got = float(sk.sum_partials(hst[:cnt]))
    print("grid-striding cost:", cnt, "partials,", got, want)
    assert abs(got - want) <= (M_COST * gr.EPS32 / (1 - M_COST * gr.EPS32) + 2 * e.k_eval * gr.EPS32) * want, (got, want)


def test_gather_launch_grid_strides(torch, L, handles):
    """weighted_laplacian.t on 1100 x 960 = 1,056,000 pixels, more than the 4096 x 256 instances a PCGInit1 / applyJTJ launch covers in one pass; J from scipy rows"""
    run_case(torch, L, handles, gr.weighted_laplacian_rows, (1100, 960), "gather_large", 1, expect=GATHER)


# jtfg_ / jtjg_: the gather form of ONE residual, emitted for every residual that has one and launched only for a gathered residual outside every merged group -- the
# plugin puts every gathered residual into a group (groups of one included), so no plan launches them
NEVER_LAUNCHED = {"jtfg", "jtjg"}


def test_every_kind_of_generated_kernel_was_launched(torch, L, handles, tmp_path):
    """by kind (the name up to its first '_'): what the plugins of five cases hold against what those cases launch.  Self-contained: the cases run here (on the
    module's handles where another test has opened them already)."""
    rans = [run_case(torch, L, handles, gr.gradient_paste, (14, 11), "rw_agg1", 0, ab="frontend_aggregate=1"),
            run_case(torch, L, handles, gr.gradient_paste, (14, 11), "gather_preload1", 1, ab="frontend_preload=1"),
            run_case(torch, L, handles, gr.cotan_smooth, (), "lanes1", 1, ab="inc_lanes=1", unit="index_map"),
            run_case(torch, L, handles, gr.weighted_laplacian, (14, 9), "J_and_Jp", 0, extra=LINES["J_and_Jp"][0], tmp_path=tmp_path),
            run_case(torch, L, handles, gr.weighted_laplacian, (14, 9), "Jp", 0, extra=LINES["Jp"][0], tmp_path=tmp_path)]
    held_kinds = {kind(n) for r in rans for n in r.handle.kernels(1)}
    launched_kinds = set().union(*[r.launched for r in rans])
    print("held:", sorted(held_kinds), "launched:", sorted(launched_kinds))
    assert {"cost", "costgrp", "jtf", "jtj", "jtfgrp", "jtjgrp", "uidx", "jtfn", "jtjn", "dumpj", "applyj", "applyjt"} <= launched_kinds
    assert held_kinds - launched_kinds <= NEVER_LAUNCHED, sorted(held_kinds - launched_kinds)
