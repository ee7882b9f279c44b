"""Held unknowns on the ladybug-1723 shape (profiles/ba_held/): for each of the four bundle-adjustment plans -- point Jacobi, block Jacobi, Schur, assembled Schur -- whole solves
with nothing held, with cameras {0, 1} held and with the intrinsics (components 6-8 of every camera) held, all in one process at timingLevel 0: the cost after every step,
the PCG iterations, the time of the steps (wall clock behind Init, best of three) and the mean time of every hold launch (all launches sampled, a pass of its own).

    python tools/ba_held_bench.py [out.json]"""
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

HOLD = ("HoldPCG", "BlockHold", "BlockHoldFactor")
FORMS = ("jacobi", "block_jacobi", "schur_pcg", "schur_explicit_pcg")
ROWS = [("LM 5x150 q_tolerance 0.1", 5, 150, True, dict(q_tolerance=0.1, function_tolerance=0.0)), ("GN 5x10", 5, 10, False, {}),
        ("GN 4x150 (the undamped step solved almost exactly: DESIGN.md 13)", 4, 150, False, {})]


def masks(C, P):
    none = None
    two = np.zeros(9 * C + 3 * P, np.uint8); two[:18] = 1
    intr = np.zeros(9 * C + 3 * P, np.uint8); intr[:9 * C].reshape(C, 9)[:, 6:9] = 1
    return {"nothing held": none, "cameras {0, 1} held": two, "intrinsics held": intr}


def plan(dims, params, form, lm, mask, nit, lit, sp):
    dev = [torch.from_numpy(x.copy()).cuda() for x in params]
    s = thallo_amd.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), timing_level=0, **({"solverkind": "levenberg_marquardt"} if lm else {}))
    if lm: s.enable_lm()
    if form.startswith("schur"): s.set_linear_solver(form)
    else: s.set_preconditioner(form)
    if mask is not None:
        s.hold(0, mask[:9 * dims[0]]); s.hold(1, mask[9 * dims[0]:])
    s.set_solver_parameters(nIterations=nit, lIterations=lit, **sp)
    return s, s.make_params(dev), dev


def solve(dims, params, form, lm, mask, nit, lit, sp, reps=3):
    s, prm, dev = plan(dims, params, form, lm, mask, nit, lit, sp)
    s.init(prm)
    costs, iters = [s.current_cost()], []
    while s.step(prm):
        costs.append(s.current_cost()); iters.append(len(s.alpha_beta_trace()))
    name, held = s.schedule_name, s.held_unknowns()
    s.close()
    steps = []
    for _ in range(reps):
        s, prm, dev = plan(dims, params, form, lm, mask, nit, lit, sp)
        s.init(prm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        while s.step(prm): n += 1
        torch.cuda.synchronize()
        steps.append((time.perf_counter() - t0) * 1e3 / max(1, n))
        s.close()
    s, prm, dev = plan(dims, params, form, lm, mask, nit, lit, sp)
    s.set_kernel_sampling(1)
    s.init(prm)
    while s.step(prm): pass
    torch.cuda.synchronize()
    ks = {k: round((v["own_mean_ms"] or v["mean_ms"]) * 1e3, 2) for k, v in s.kernel_stats().items() if k in HOLD and v["mean_ms"]}
    launches = {k: v["launches"] for k, v in s.kernel_stats().items() if k in HOLD}
    s.close()
    return {"schedule": name, "held_unknowns": held, "cost_after_each_step": costs, "pcg_iters_per_step": iters, "ms_per_step": [round(x, 4) for x in steps],
            "ms_per_step_min": round(min(steps), 4), "hold_launch_mean_us": ks, "hold_launches": launches,
            "hold_us_per_step": round(sum(ks.get(k, 0.0) * launches.get(k, 0) for k in HOLD) / max(1, len(iters)), 2)}


p = syn.bundle_adjustment()
dims = (p[0].shape[0], p[1].shape[0], p[2].shape[0])
out = []
for row, nit, lit, lm, sp in ROWS:
    for form in FORMS:
        for what, mask in masks(dims[0], dims[1]).items():
            r = solve(dims, p, form, lm, mask, nit, lit, sp)
            r.update(config="bundle_adjustment ladybug shape " + row, form=form, mask=what)
            print(json.dumps(r), flush=True)
            out.append(r)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f: json.dump(out, f, indent=1)
