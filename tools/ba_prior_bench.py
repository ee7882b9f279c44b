"""Gaussian priors on the ladybug-1723 shape (profiles/ba_prior/), all in one process at timingLevel 0.

  overhead    for each of the six bundle-adjustment plans -- point Jacobi, block Jacobi, Schur, assembled Schur, its dense Cholesky factor, the two-level preconditioner --
              GN 5 x 10 and LM 5 x 150 without priors and with a prior on components 6-8 of every camera (sigma = 10 % of the initial value): the cost after every step, the
              PCG iterations, the time of the steps (wall clock behind Init, best of three) and the mean time and count of every prior launch (all launches sampled, a pass
              of its own).  Cameras {0, 1} are held in every row, so that the dense factor has a gauge in GN.
  divergence  DESIGN.md 15's GN 4 x 150 on the Schur plan with cameras {0, 1} held: the intrinsics free, held, and under a prior at their initial values with sigma = 1 %,
              10 % and 100 % of each value -- the cost after every step.

    python tools/ba_prior_bench.py [out.json]
    python tools/ba_prior_bench.py --ab OTHER_LIB [out.json]     tools/ba_robust_bench.py --ab: the squared-loss point-Jacobi plan without a prior, this build and OTHER_LIB"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if len(sys.argv) > 2 and sys.argv[1] == "--ab":
    sys.exit(subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ba_robust_bench.py")] + sys.argv[1:]).returncode)

import numpy as np
import torch

import thallo_amd
from thallo_amd import synthetic as syn

PRIOR = ("PriorCost", "PriorInit", "PriorShift")
FORMS = ("jacobi", "block_jacobi", "schur_pcg", "schur_explicit_pcg", "schur_dense", "two_level")
ROWS = [("GN 5x10", 5, 10, False, {}), ("LM 5x150 q_tolerance 0.1", 5, 150, True, dict(q_tolerance=0.1, function_tolerance=0.0))]


def intrinsics_prior(cams, sigma_rel):
    """-> (mean, weight) [C, 9]: components 6-8 at their values, sigma = sigma_rel |value| (a value of exactly 0 gets no prior)"""
    w = np.zeros_like(cams); v = np.abs(cams[:, 6:9].astype(np.float64))
    w[:, 6:9] = np.where(v > 0, 1.0 / np.maximum(sigma_rel * v, 1e-30) ** 2, 0.0).astype(np.float32)
    return cams.copy(), w


def plan(dims, params, form, lm, hold, prior, nit, lit, sp):
    dev = [torch.from_numpy(x.copy()).cuda() for x in params]
    s = thallo_amd.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), timing_level=0, **({"solverkind": "levenberg_marquardt"} if lm else {}))
    if lm: s.enable_lm()
    if form == "two_level": s.set_linear_solver("schur_explicit_pcg"); s.set_preconditioner("two_level")
    elif form.startswith("schur"): s.set_linear_solver(form)
    else: s.set_preconditioner(form)
    if hold is not None: s.hold(0, hold)
    if prior is not None: s.set_prior(0, prior[0], prior[1])
    s.set_solver_parameters(nIterations=nit, lIterations=lit, **sp)
    return s, s.make_params(dev), dev


def solve(dims, params, form, lm, hold, prior, nit, lit, sp, reps=3, timed=True):
    s, prm, dev = plan(dims, params, form, lm, hold, prior, nit, lit, sp)
    s.init(prm)
    costs, iters = [s.current_cost()], []
    while s.step(prm):
        costs.append(s.current_cost()); iters.append(len(s.alpha_beta_trace()))
    out = {"schedule": s.schedule_name, "prior_terms": s.prior_terms(), "prior_cost_at_end": s.prior_cost(), "cost_after_each_step": costs, "pcg_iters_per_step": iters}
    s.close()
    if not timed: return out
    steps = []
    for _ in range(reps):
        s, prm, dev = plan(dims, params, form, lm, hold, prior, nit, lit, sp)
        s.init(prm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        while s.step(prm): n += 1
        torch.cuda.synchronize()
        steps.append((time.perf_counter() - t0) * 1e3 / max(1, n))
        s.close()
    s, prm, dev = plan(dims, params, form, lm, hold, prior, nit, lit, sp)
    s.set_kernel_sampling(1)
    s.init(prm)
    while s.step(prm): pass
    torch.cuda.synchronize()
    ks = {k: round((v["own_mean_ms"] or v["mean_ms"]) * 1e3, 2) for k, v in s.kernel_stats().items() if k in PRIOR and v["mean_ms"]}
    launches = {k: v["launches"] for k, v in s.kernel_stats().items() if k in PRIOR}
    s.close()
    out.update(ms_per_step=[round(x, 4) for x in steps], ms_per_step_min=round(min(steps), 4), prior_launch_mean_us=ks, prior_launches=launches,
               prior_us_per_step=round(sum(ks.get(k, 0.0) * launches.get(k, 0) for k in PRIOR) / max(1, len(iters)), 2))
    return out


p = syn.bundle_adjustment()
dims = (p[0].shape[0], p[1].shape[0], p[2].shape[0])
C_ = dims[0]
two = np.zeros((C_, 9), np.uint8); two[:2] = 1
intr = two.copy(); intr[:, 6:9] = 1
out = []
for row, nit, lit, lm, sp in ROWS:
    for form in FORMS:
        for what, prior in (("no prior", None), ("intrinsics, sigma 10 %", intrinsics_prior(p[0], 0.1))):
            r = solve(dims, p, form, lm, two, prior, nit, lit, sp)
            r.update(part="overhead", config="bundle_adjustment ladybug shape, cameras {0, 1} held, " + row, row=row, form=form, prior=what)
            print(json.dumps(r), flush=True)
            out.append(r)
cases = [("intrinsics free", two, None), ("intrinsics held", intr, None)] + [("prior on the intrinsics, sigma %g %%" % (100 * s_), two, intrinsics_prior(p[0], s_)) for s_ in (0.01, 0.1, 1.0)]
for what, hold, prior in cases:
    r = solve(dims, p, "schur_pcg", False, hold, prior, 4, 150, {}, timed=False)
    r.update(part="divergence", config="bundle_adjustment ladybug shape, GN 4x150, Schur plan, cameras {0, 1} held", prior=what)
    print(json.dumps(r), flush=True)
    out.append(r)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f: json.dump(out, f, indent=1)
