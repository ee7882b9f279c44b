"""Marginal covariances on the ladybug-1723 shape (profiles/ba_covariance/): one Gauss-Newton plan with the assembled reduced camera matrix, cameras {0, 1} held, all in
one process at timingLevel 0.  After two GN steps of 10 iterations:

  - wall time (host clock around the call, which ends in a stream synchronise; best of three behind a first call that allocates) of ThalloX_PlanCovariance for 7 cameras,
    for all cameras and for 21 points, with the iterations each took and the info the call returns;
  - the set-up's share: the same call with max_iterations = 1 (re-linearisation, both factors, W, the assembly, one iteration, the output);
  - the time of one batch iteration: 7 cameras with a rel_tol no column reaches, max_iterations 40 against 200, the difference over 160;
  - the one-column loop of the same plan, for 64 x: the own times of SchurApplyS, BlockStep2 and PCGStep3 (every launch sampled, a pass of its own).

Per-kernel times of the batch iteration come from a kernel trace of this script (rocprofv3 --kernel-trace --stats, a run of its own), not from here.

    python tools/ba_covariance_bench.py [out.json]
    python tools/ba_covariance_bench.py --short          without the all-cameras row (what a kernel trace is taken of)"""
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

p = syn.bundle_adjustment()
C_, P_, O_ = dims = (p[0].shape[0], p[1].shape[0], p[2].shape[0])
mask = np.zeros(9 * C_, np.uint8); mask[:18] = 1


def plan(sampling=0, p=p, dims=dims, mask=mask):
    dev = [torch.from_numpy(x.copy()).cuda() for x in p]
    s = thallo_amd.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), timing_level=0)
    s.set_linear_solver("schur_explicit_pcg")
    s.hold(0, mask)
    s.set_solver_parameters(nIterations=2, lIterations=10)
    if sampling: s.set_kernel_sampling(sampling)
    prm = s.make_params(dev)
    s.init(prm)
    while s.step(prm): pass
    torch.cuda.synchronize()
    return s, prm, dev


def timed(s, prm, reps=3, **kw):
    out = s.covariance(prm, **kw)                       # (the first call of a plan allocates the work vectors; every call warms its shapes)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = s.covariance(prm, **kw)
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(min(ts), 3), [round(t, 3) for t in ts], out["info"]


s, prm, dev = plan()
res = {"config": "bundle_adjustment ladybug shape, GN 2 x 10, cameras {0, 1} held, assembled S", "dims": dims, "schur_blocks": s.schur_blocks(), "schedule": s.schedule_name}
nblk = s.schur_blocks()
cams7, pts21 = list(range(2, 9)), list(range(0, P_, P_ // 21))[:21]
short = "--short" in sys.argv
for name, kw in (("7 cameras", dict(cameras=cams7)), ("all cameras", dict(cameras=list(range(C_)))), ("21 points", dict(points=pts21))):
    if short and name == "all cameras": continue
    best, ts, info = timed(s, prm, **kw)
    one, _, _ = timed(s, prm, max_iterations=1, **kw)
    res[name] = {"ms": best, "ms_all": ts, "info": info, "ms_with_max_iterations_1": one, "setup_share": round(one / best, 3)}
    print(name, res[name], flush=True)
t40, _, i40 = timed(s, prm, cameras=cams7, rel_tol=1e-30, max_iterations=40)
t200, _, i200 = timed(s, prm, cameras=cams7, rel_tol=1e-30, max_iterations=200)
assert i40["iterations"] == 40 and i200["iterations"] == 200
us = (t200 - t40) * 1e3 / 160
res["batch_iteration"] = {"ms_40": t40, "ms_200": t200, "us_per_iteration_of_64_columns": round(us, 2), "launches_per_iteration": 5,
                          "S_bytes": 324 * nblk, "S_bytes_per_s_over_the_whole_iteration": round(324 * nblk / (us * 1e-6), 0)}
print("batch iteration", res["batch_iteration"], flush=True)
if not short:      # where the defaults' 500 iterations do not do: how many do (one call each, not timed)
    res["7 cameras, max_iterations 20000"] = s.covariance(prm, cameras=cams7, max_iterations=20000)["info"]
    print("7 cameras, max_iterations 20000", res["7 cameras, max_iterations 20000"], flush=True)
s.close()
if not short:      # iterations to convergence against the length of the camera chain: smaller instances of the same generator, the same gauge, 7 cameras and 21 points
    for kw in (dict(C=48, P=1200, O=5000, band=16), dict(C=200, P=6000, O=26000), dict(C=600, P=40000, O=170000)):
        q = syn.bundle_adjustment(**kw)
        m = np.zeros(9 * kw["C"], np.uint8); m[:18] = 1
        s, prm, dev = plan(p=q, dims=(kw["C"], kw["P"], kw["O"]), mask=m)
        row = {"blocks": s.schur_blocks()}
        for name, a in (("7 cameras", dict(cameras=list(range(2, 9)))), ("21 points", dict(points=list(range(0, kw["P"], kw["P"] // 21))[:21]))):
            best, _, info = timed(s, prm, max_iterations=5000, **a)
            row[name] = {"ms": best, "info": info}
        s.close()
        res["instance %s" % (tuple(kw.values()),)] = row
        print(kw, row, flush=True)
s, prm, dev = plan(sampling=1)
ks = {k: round((v["own_mean_ms"] or v["mean_ms"]) * 1e3, 2) for k, v in s.kernel_stats().items() if k in ("SchurApplyS", "BlockStep2", "PCGStep3") and v["mean_ms"]}
s.close()
one = sum(ks.values())
res["one_column_loop"] = {"own_mean_us": ks, "us_per_iteration": round(one, 2), "x64": round(64 * one, 1), "batch_over_64_one_column_iterations": round(us / (64 * one), 4)}
print("one-column loop", res["one_column_loop"], flush=True)
if len(sys.argv) > 1 and not short:
    with open(sys.argv[1], "w") as f: json.dump(res, f, indent=1)
