"""Secondary configs of BASELINE.json (not the headline bench): ms per GN iteration / PCG it/s on one MI355X for
image_warping 512^2, ARAP 102,400 vertices, shape_from_shading 2048^2, bundle adjustment ladybug-1723 shape.
Prints one JSON object; kernel means from the library's sampled HIP events."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import thallo_amd
from thallo_amd import synthetic as syn


def run(name, fname, dims, params, nit, lit, warm=1, lm=False):
    dev = [torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else float(x) for x in params]
    # BC_TIMING (default 0 = Thallo.h's "No timing recorded"): at level 1 every step records eight coarse events, each a barrier packet between two launches -- ~30 us per GN
    # step, which only the small configurations notice
    s = thallo_amd.ThalloSolver(dims, thallo_amd.energy_file(fname), timing_level=int(os.environ.get("BC_TIMING", "0")), **({"solverkind": "levenberg_marquardt"} if lm else {}))
    if lm:
        s.enable_lm()
    s.set_solver_parameters(nIterations=2 * nit + warm, lIterations=lit, **({"q_tolerance": 0.0} if lm else {}))
    prm = s.make_params(dev)
    s.init(prm)
    c0 = s.current_cost()
    for _ in range(warm):
        s.step(prm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()            # the timed pass: no events of any kind in the stream
    for _ in range(nit):
        s.step(prm)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    s.reset_kernel_stats(); s.set_kernel_sampling(4)
    for _ in range(nit):                # a second pass for the per-kernel means (HIP events around every fourth launch of a name)
        s.step(prm)
    torch.cuda.synchronize()
    s.set_kernel_sampling(0)
    ks = {k: round(v["mean_ms"] * 1e3, 2) for k, v in s.kernel_stats().items() if v["mean_ms"]}
    return {"config": name, "ms_per_gn_iter": dt / nit * 1e3, "pcg_iters_per_sec": nit * lit / dt, "us_per_pcg_iter": dt / (nit * lit) * 1e6,
            "cost0": c0, "cost": s.current_cost(), "kernel_mean_us": ks}


def cat512():
    """BASELINE.json configs[1] on the reference's own data: cat512 mask + markers + pinned border (tests/golden fixtures),
    first step of the harness' continuation (targets at 1/19 of the way)."""
    from thallo_amd import formats as F
    g = os.path.join(ROOT, "tests", "golden")
    mask = F.read_png(os.path.join(g, "cat512_mask.png"))[:, :, 0].astype(np.float32)
    H, W = mask.shape
    cons = F.add_border_constraints(F.read_constraints(os.path.join(g, "cat512.constraints")), W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    ur = np.stack([xx, yy], axis=2).astype(np.float32)
    return [ur.copy(), np.zeros((H, W), np.float32), ur.copy(), F.constraint_image(cons, mask, np.float32(1.0 / 19.0)), mask,
            float(np.sqrt(np.float32(100.0))), float(np.sqrt(np.float32(0.01)))]


SCHUR_FORMS = ("schur_pcg", "schur_explicit_pcg")      # linear solvers (set_linear_solver); the other forms are preconditioners of the full system


def solve_ab(name, dims, params, nit, lit, lm, precond, reps=3, **sp):
    """One whole solve (Init + while Step) per pass, from the same start, in one of four forms: "jacobi" (the default plan), "block_jacobi" (the opt-in block
    preconditioner), "schur_pcg" (the opt-in Schur-complement solve; its preconditioner is the camera blocks) or "schur_explicit_pcg" (that solve with the reduced camera
    matrix assembled once per step).  Pass 1 (also the warm-up)
    reads the PCG iterations and the cost after every step; then `reps` timed passes at timingLevel 0 with nothing else in the stream (wall clock, Init to the last Step;
    Init, which ends with a cost read back and in the assembled form builds the structure of S on the host, also on its own);
    then one pass at timingLevel 1 for the coarse "Linear Solve" events and one with every launch sampled for the kernel means."""
    def plan(timing):
        dev = [torch.from_numpy(x.copy()).cuda() for x in params]
        s = thallo_amd.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), timing_level=timing, **({"solverkind": "levenberg_marquardt"} if lm else {}))
        if lm: s.enable_lm()
        if precond in SCHUR_FORMS: s.set_linear_solver(precond)
        else: s.set_preconditioner(precond)
        s.set_solver_parameters(nIterations=nit, lIterations=lit, **sp)
        return s, s.make_params(dev), dev
    s, prm, dev = plan(0)
    s.init(prm)
    costs, iters, fallbacks, held = [s.current_cost()], [], 0, 0
    while s.step(prm):
        costs.append(s.current_cost()); iters.append(len(s.alpha_beta_trace())); fallbacks += max(0, s.preconditioner_fallbacks()); held += max(0, s.schur_held_points())
    sched, blocks = s.schedule_name, s.schur_blocks()
    s.close()
    whole, inits = [], []
    for _ in range(reps):
        s, prm, dev = plan(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.init(prm)
        t1 = time.perf_counter()
        while s.step(prm): pass
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3); inits.append((t1 - t0) * 1e3)
        s.close()
    s, prm, dev = plan(1)
    s.init(prm)
    while s.step(prm): pass
    s.current_cost()
    ps = s.performance_summary()
    s.close()
    s, prm, dev = plan(0)
    s.set_kernel_sampling(1)
    s.init(prm)
    while s.step(prm): pass
    torch.cuda.synchronize()
    ks = {k: round((v["own_mean_ms"] or v["mean_ms"]) * 1e3, 2) for k, v in s.kernel_stats().items() if v["mean_ms"]}
    s.close()
    lin = ps["linearSolve"]
    return {"config": name, "preconditioner": precond, "schedule": sched, "pcg_iters_per_step": iters, "pcg_iters": sum(iters), "cost_after_each_step": costs,
            "whole_solve_ms": [round(x, 3) for x in whole], "whole_solve_ms_min": round(min(whole), 3),
            "init_ms": [round(x, 3) for x in inits], "steps_ms": [round(w - i, 3) for w, i in zip(whole, inits)], "schur_blocks": blocks,
            "linear_solve_ms_per_step": round(lin["meanMS"], 4), "linear_solve_steps": lin["count"],
            "us_per_pcg_iter": round(lin["meanMS"] * lin["count"] / max(1, sum(iters)) * 1e3, 2), "fallbacks": fallbacks, "held_points": held, "kernel_mean_us": ks}


def gn_budget(dims, params, form, target, nit=7, budgets=(5, 10, 15, 20, 25, 35, 50, 75, 100, 150)):
    """The smallest lIterations of `budgets` at which nit GN steps of the form end at or below `target` (the default plan's cost after nit x 150) -> (lIterations, final cost);
    lIterations None: not within the largest budget"""
    last = None
    for lit in budgets:
        dev = [torch.from_numpy(x.copy()).cuda() for x in params]
        s = thallo_amd.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), timing_level=0)
        if form in SCHUR_FORMS: s.set_linear_solver(form)
        else: s.set_preconditioner(form)
        s.set_solver_parameters(nIterations=nit, lIterations=lit)
        prm = s.make_params(dev)
        s.init(prm)
        while s.step(prm): pass
        last = s.current_cost()
        s.close()
        if last <= target: return lit, last
    return None, last


only = sys.argv[1] if len(sys.argv) > 1 else ""      # e.g. "sfs", "ba", "image_warping", "arap": the configurations whose name contains it
want = lambda name: only in name
out = []
if want("image_warping cat512"): out.append(run("image_warping cat512 (reference data) GN 8x100", "image_warping", (512, 512), cat512(), 8, 100))
if want("image_warping 512"): out.append(run("image_warping 512x512 synthetic GN 8x100", "image_warping", (512, 512), syn.image_warping(512, 512), 8, 100))
if want("arap"):
    p = syn.arap_mesh(320, 320)
    out.append(run("arap_mesh 102400 v / 614400 e GN 20x100", "arap_mesh_deformation", (p[2].shape[0], p[6].shape[0]), p, 5, 100))
if want("shape_from_shading") or only == "sfs":
    out.append(run("shape_from_shading 2048x2048 GN x10", "shape_from_shading", (2048, 2048), syn.shape_from_shading(2048, 2048), 6, 10))
    out.append(run("shape_from_shading 2048x2048 LM x10 (BASELINE config 4's solver)", "shape_from_shading", (2048, 2048), syn.shape_from_shading(2048, 2048), 5, 10, lm=True))
if only == "sfs640":      # (not in the default set: tools/profile_configs.sh averages per kernel NAME, so every profiled configuration of an energy has one size)
    out.append(run("shape_from_shading 640x480 GN x10 (the size of the reference's data set)", "shape_from_shading", (640, 480), syn.shape_from_shading(640, 480), 12, 10))
    out.append(run("shape_from_shading 640x480 LM x10", "shape_from_shading", (640, 480), syn.shape_from_shading(640, 480), 10, 10, lm=True))
if want("bundle_adjustment") or only == "ba":
    p = syn.bundle_adjustment()
    out.append(run("bundle_adjustment C=1723 P=156502 O=678718 LM x150 (BASELINE config 5's solver)", "bundle_adjustment", (p[0].shape[0], p[1].shape[0], p[2].shape[0]), p, 3, 150, lm=True))
    out.append(run("bundle_adjustment C=1723 P=156502 O=678718 GN x150", "bundle_adjustment", (p[0].shape[0], p[1].shape[0], p[2].shape[0]), p, 3, 150))
if only == "ba":      # (on request only: the default set is what tools/profile_configs.sh profiles)
    # the opt-in block-Jacobi preconditioner and the opt-in Schur-complement solve against the default Jacobi path of the same build, whole solves from the same start, all in
    # this one process (profiles/block_jacobi/, profiles/ba_schur/, profiles/ba_schur_explicit/)
    d = (p[0].shape[0], p[1].shape[0], p[2].shape[0])
    rows = [("bundle_adjustment ladybug shape LM 5x150 q_tolerance 0.1", 5, 150, True, 3, dict(q_tolerance=0.1, function_tolerance=0.0)),
            ("bundle_adjustment ladybug shape GN 5x10", 5, 10, False, 3, {}),
            ("bundle_adjustment ladybug shape GN 5x25", 5, 25, False, 3, {}),
            ("bundle_adjustment ladybug shape GN 5x150", 5, 150, False, 3, {}),
            ("bundle_adjustment ladybug shape LM 2x150 q_tolerance 0 (every iteration runs: the loop's cost per iteration)", 2, 150, True, 1, dict(q_tolerance=0.0, function_tolerance=0.0))]
    forms = ("jacobi", "block_jacobi", "schur_pcg", "schur_explicit_pcg")
    for name, nit, lit, lm, reps, sp in rows:      # the four forms of a row one after the other
        for pc in forms:
            out.append(solve_ab(name, d, p, nit, lit, lm, pc, reps=reps, **sp))
    # the GN iteration budget at which each form reaches the default plan's 7 x 150 cost
    _, target = gn_budget(d, p, "jacobi", float("-inf"), budgets=(150,))
    out.append({"config": "bundle_adjustment ladybug shape: lIterations at which 7 GN steps reach the default plan's 7x150 cost", "target_cost": target,
                "budget": {pc: dict(zip(("lIterations", "cost"), gn_budget(d, p, pc, target))) for pc in forms}})
print(json.dumps(out, indent=1))
