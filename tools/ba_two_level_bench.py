"""The two-level preconditioner on the assembled Schur PCG of bundle adjustment against block Jacobi (profiles/ba_two_level/): one process, timingLevel 0, cameras
{0, 1} held, both forms on every shape -- (48, 1200, 5000), (200, 6000, 26000), (600, 40000, 170000) and ladybug-1723:

  - the set-up per step: the launch groups CoarseAssemble, CoarseScale, CoarseFactor, CoarseInverse next to SchurW / SchurAssemble (every launch sampled, a pass of its own);
  - a PCG iteration: the launches of the reduced loop (PCGStep3, SchurApplyS, BlockStep2LM, CoarseApply, PCGZeta), and a covariance batch iteration as the call's wall
    time over its iterations;
  - LM 5 x 150 at q_tolerance 0.1 and at 1e-4 (function_tolerance 0): wall time of the steps (host clock, a stream synchronise at the end; the second of two solves),
    linear iterations per step, the final cost;
  - ThalloX_PlanCovariance of 7 cameras after GN 2 x 10 (best of three behind a first call that allocates): iterations, ms, open columns; at the ladybug shape also with
    max_iterations 1000.

    python tools/ba_two_level_bench.py [out.json] [--no-ladybug]
    python tools/ba_two_level_bench.py --default         one JSON line: the default plan's (point Jacobi, full system) step times on the ladybug shape (the child of --ab)
    python tools/ba_two_level_bench.py --ab OTHER_LIB [out.json]     that child in fresh processes, this build and THALLO_LIB=OTHER_LIB interleaved, four rounds"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if len(sys.argv) > 2 and sys.argv[1] == "--ab":
    rounds = []
    for i in range(4):
        for which, lib in (("this build", None), ("other", sys.argv[2])):
            env = dict(os.environ)
            env.pop("THALLO_LIB", None)
            if lib: env["THALLO_LIB"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--default"], env=env, check=True, capture_output=True, text=True).stdout
            r = json.loads([l for l in out.splitlines() if l.startswith("{")][-1]); r.update(build=which, round=i)
            print(json.dumps(r), flush=True)
            rounds.append(r)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f: json.dump(rounds, f, indent=1)
    sys.exit(0)

import numpy as np
import torch

import thallo_amd
from thallo_amd import synthetic as syn

FORMS = (("block Jacobi", None), ("two-level", "two_level"))
SETUP = ("SchurW", "SchurAssemble", "CoarseAssemble", "CoarseScale", "CoarseFactor", "CoarseInverse")
LOOP = ("PCGStep3", "SchurApplyS", "BlockStep2LM", "CoarseApply", "PCGZeta")


def plan(p, dims, precond, lm, sampling=0, solver="schur_explicit_pcg", hold=True, **sp):
    dev = [torch.from_numpy(x.copy()).cuda() for x in p]
    s = thallo_amd.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), timing_level=0, solverkind="levenberg_marquardt" if lm else "gauss_newton")
    if lm: s.enable_lm()
    if solver: s.set_linear_solver(solver)
    if precond: s.set_preconditioner(precond)
    if hold:
        mask = np.zeros(9 * dims[0], np.uint8); mask[:18] = 1
        s.hold(0, mask)
    s.set_solver_parameters(**sp)
    if sampling: s.set_kernel_sampling(sampling)
    prm = s.make_params(dev)
    return s, prm, dev


def lm_solve(p, dims, precond, q_tolerance, sampling=0):
    s, prm, dev = plan(p, dims, precond, True, sampling, nIterations=5, lIterations=150, q_tolerance=q_tolerance, function_tolerance=0.0)
    s.init(prm)
    assert s.ready(), thallo_amd.api.last_error()
    iters = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while s.step(prm): iters.append(len(s.alpha_beta_trace()))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    out = {"ms_5_steps": round(ms, 3), "linear_iterations": iters, "final_cost": s.current_cost(), "schedule": s.schedule_name, "coarse_space": s.coarse_space()}
    ks = s.kernel_stats()
    s.close()
    return out, ks


def covariance(p, dims, precond, max_iterations=500):
    s, prm, dev = plan(p, dims, precond, False, nIterations=2, lIterations=10)
    s.init(prm)
    assert s.ready(), thallo_amd.api.last_error()
    while s.step(prm): pass
    torch.cuda.synchronize()
    ids = list(range(2, 9))
    info = s.covariance(prm, cameras=ids, max_iterations=max_iterations)["info"]
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = s.covariance(prm, cameras=ids, max_iterations=max_iterations)["info"]
        ts.append((time.perf_counter() - t0) * 1e3)
    s.close()
    return {"ms": round(min(ts), 3), "ms_all": [round(t, 3) for t in ts], "iterations": info["iterations"], "open_columns": info["not_converged"], "columns": info["columns"],
            "worst_residual": info["worst_residual"], "us_per_batch_iteration": round(min(ts) * 1e3 / max(1, info["iterations"]), 2), "max_iterations": max_iterations}


if len(sys.argv) > 1 and sys.argv[1] == "--default":
    p = syn.bundle_adjustment()
    dims = (p[0].shape[0], p[1].shape[0], p[2].shape[0])
    r = {}
    for row, lm, sp in (("GN 5x10", False, dict(nIterations=5, lIterations=10)), ("LM 5x150 q_tolerance 0.1", True, dict(nIterations=5, lIterations=150, q_tolerance=0.1, function_tolerance=0.0))):
        steps = []
        for _ in range(5):
            s, prm, dev = plan(p, dims, None, lm, solver=None, hold=False, **sp)
            s.init(prm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            while s.step(prm): n += 1
            torch.cuda.synchronize()
            steps.append((time.perf_counter() - t0) * 1e3 / max(1, n))
            s.close()
        r[row] = round(min(steps), 4)
    print(json.dumps({"ms_per_step_min": r, "lib": os.environ.get("THALLO_LIB", "")}))
    sys.exit(0)

shapes = [dict(C=48, P=1200, O=5000, band=16), dict(C=200, P=6000, O=26000), dict(C=600, P=40000, O=170000)]
if "--no-ladybug" not in sys.argv: shapes.append(dict())
res = {"config": "bundle_adjustment, THALLOX_SOLVER_SCHUR_EXPLICIT_PCG, cameras {0, 1} held, timingLevel 0, one process"}
for kw in shapes:
    p = syn.bundle_adjustment(**kw)
    dims = (p[0].shape[0], p[1].shape[0], p[2].shape[0])
    row = {}
    for label, precond in FORMS:
        r = {}
        for q in (0.1, 1e-4):
            lm_solve(p, dims, precond, q)                               # (warms the shapes)
            r["LM 5x150 q_tolerance %g" % q], _ = lm_solve(p, dims, precond, q)
        _, ks = lm_solve(p, dims, precond, 1e-4, sampling=1)
        us = lambda names: {k: round(ks[k]["mean_ms"] * 1e3, 2) for k in names if k in ks and ks[k]["mean_ms"]}
        r["setup_us"], r["loop_us"] = us(SETUP), us(LOOP)
        r["covariance 7 cameras"] = covariance(p, dims, precond)
        if not kw: r["covariance 7 cameras, max_iterations 1000"] = covariance(p, dims, precond, 1000)
        row[label] = r
        print(dims, label, json.dumps(r), flush=True)
    res["instance %s" % (dims,)] = row
out = [a for a in sys.argv[1:] if not a.startswith("--")]
if out:
    with open(out[0], "w") as f: json.dump(res, f, indent=1)
