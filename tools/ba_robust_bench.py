"""Robust losses on the ladybug-1723 shape (profiles/ba_robust/): the synthetic instance with 5 % of its observations displaced by 30 - 150 px (tests/ba_robust_mirror.py
contaminate), and for each of the four bundle-adjustment plans -- point Jacobi, block Jacobi, Schur, assembled Schur -- whole solves with the squared loss, Huber 2 and
Cauchy 2, GN 5 x 10 and LM 5 x 150, all in one process at timingLevel 0: the cost after every step, the PCG iterations, the time of the steps (wall clock behind Init, best
of three passes), the own times of precomputeJ, computeCost and the applyJTJ launches (PCGStep1: the camera launch, the only one with a robust instantiation, and the point
launch behind it; every launch sampled, a pass of its own) and the inliers' RMS reprojection error at the end.

    python tools/ba_robust_bench.py [out.json [README.md]]
    python tools/ba_robust_bench.py --trivial           one JSON line: the squared-loss point-Jacobi plan's step times only (the child of --ab)
    python tools/ba_robust_bench.py --ab OTHER_LIB [out.json]     that child in fresh processes, this build and THALLO_LIB=OTHER_LIB interleaved, four rounds"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if len(sys.argv) > 2 and sys.argv[1] == "--ab":
    rounds = []
    for i in range(4):
        for which, lib in (("this build", None), ("other", sys.argv[2])):
            env = dict(os.environ)
            env.pop("THALLO_LIB", None)
            if lib: env["THALLO_LIB"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--trivial"], env=env, check=True, capture_output=True, text=True).stdout
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

from ba_robust_mirror import contaminate, residuals64

OWN = ("precomputeJ", "computeCost", "PCGStep1")
FORMS = ("jacobi", "block_jacobi", "schur_pcg", "schur_explicit_pcg")
LOSSES = (("trivial", 0.0), ("huber", 2.0), ("cauchy", 2.0))
ROWS = [("GN 5x10", 5, 10, False, {}), ("LM 5x150 q_tolerance 0.1", 5, 150, True, dict(q_tolerance=0.1, function_tolerance=0.0))]


def plan(dims, params, form, lm, loss, nit, lit, sp):
    dev = [torch.from_numpy(x.copy()).cuda() for x in params]
    s = thallo_amd.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), timing_level=0, **({"solverkind": "levenberg_marquardt"} if lm else {}))
    if lm: s.enable_lm()
    if form.startswith("schur"): s.set_linear_solver(form)
    else: s.set_preconditioner(form)
    if loss[0] != "trivial": s.set_robust_loss(*loss)          # (the squared-loss rows never make the call: they also run on a build that has no such call)
    s.set_solver_parameters(nIterations=nit, lIterations=lit, **sp)
    return s, s.make_params(dev), dev


def timed(dims, params, form, lm, loss, nit, lit, sp, reps=3):
    steps = []
    for _ in range(reps):
        s, prm, dev = plan(dims, params, form, lm, loss, nit, lit, sp)
        s.init(prm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        while s.step(prm): n += 1
        torch.cuda.synchronize()
        steps.append((time.perf_counter() - t0) * 1e3 / max(1, n))
        s.close()
    return steps


def solve(dims, params, outliers, form, lm, loss, nit, lit, sp):
    s, prm, dev = plan(dims, params, form, lm, loss, nit, lit, sp)
    s.init(prm)
    costs, iters = [s.current_cost()], []
    while s.step(prm):
        costs.append(s.current_cost()); iters.append(len(s.alpha_beta_trace()))
    name = s.schedule_name
    r = residuals64(dev[0].cpu().numpy(), dev[1].cpu().numpy(), params[2], params[3], params[4])[~outliers]
    rms = float(np.sqrt((r * r).sum(1).mean()))
    wts = s.robust_weights() if loss[0] != "trivial" else None
    s.close()
    steps = timed(dims, params, form, lm, loss, nit, lit, sp)
    s, prm, dev = plan(dims, params, form, lm, loss, nit, lit, sp)
    s.set_kernel_sampling(1)
    s.init(prm)
    while s.step(prm): pass
    torch.cuda.synchronize()
    ks = {k: round((v["own_mean_ms"] or v["mean_ms"]) * 1e3, 2) for k, v in s.kernel_stats().items() if k in OWN and v["mean_ms"]}
    s.close()
    out = {"schedule": name, "cost_after_each_step": costs, "pcg_iters_per_step": iters, "ms_per_step": [round(x, 4) for x in steps], "ms_per_step_min": round(min(steps), 4),
           "own_mean_us": ks, "inlier_rms_px": round(rms, 4)}
    if wts is not None: out.update(mean_weight_displaced=round(float(wts[outliers].mean()), 5), mean_weight_others=round(float(wts[~outliers].mean()), 5))
    return out


base = syn.bundle_adjustment()
p, outliers = contaminate(base)
dims = (p[0].shape[0], p[1].shape[0], p[2].shape[0])

if len(sys.argv) > 1 and sys.argv[1] == "--trivial":
    r = {row: round(min(timed(dims, p, "jacobi", lm, ("trivial", 0.0), nit, lit, sp, reps=5)), 4) for row, nit, lit, lm, sp in ROWS}
    print(json.dumps({"ms_per_step_min": r, "lib": os.environ.get("THALLO_LIB", "")}))
    sys.exit(0)

r0 = residuals64(p[0], p[1], p[2], p[3], p[4])[~outliers]
start = float(np.sqrt((r0 * r0).sum(1).mean()))
out = []
for row, nit, lit, lm, sp in ROWS:
    for form in FORMS:
        for loss in LOSSES:
            r = solve(dims, p, outliers, form, lm, loss, nit, lit, sp)
            r.update(config="bundle_adjustment ladybug shape, 5 % displaced, " + row, row=row, form=form, loss="%s %g" % loss if loss[1] else loss[0], inlier_rms_start_px=round(start, 4))
            print(json.dumps(r), flush=True)
            out.append(r)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f: json.dump(out, f, indent=1)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        f.write("## Tables (written by tools/ba_robust_bench.py; inlier RMS at the start %.3f px)\n" % start)
        for row, *_ in ROWS:
            f.write("\n### %s\n\n| plan | loss | ms per step (best of 3) | against the squared loss | precomputeJ / computeCost / PCGStep1 own µs | PCG iterations per step | inlier RMS at the end, px | cost after each step |\n|---|---|---|---|---|---|---|---|\n" % row)
            for r in (x for x in out if x["row"] == row):
                t0 = next(x for x in out if x["row"] == row and x["form"] == r["form"] and x["loss"] == "trivial")["ms_per_step_min"]
                f.write("| %s | %s | %.3f | %+.1f %% | %s | %s (%d) | %.3f | %s |\n" % (
                    r["form"], r["loss"], r["ms_per_step_min"], 100.0 * (r["ms_per_step_min"] / t0 - 1.0), " / ".join(str(r["own_mean_us"].get(k, "–")) for k in OWN),
                    ", ".join(map(str, r["pcg_iters_per_step"])), sum(r["pcg_iters_per_step"]), r["inlier_rms_px"], ", ".join("%.1f" % c for c in r["cost_after_each_step"])))
