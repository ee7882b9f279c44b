"""The dense Cholesky Schur solve of bundle adjustment against the PCG solvers (profiles/ba_schur_dense/): one process, timingLevel 0, cameras {0, 1} held, per shape

  - the own times of the step's three dense stages (expand, factor, one-column solve; every launch sampled, a pass of its own) and the factor's achieved FLOP/s (n^3 / 3);
  - LM 5 x 150 (q_tolerance 0.1, function_tolerance 0): wall time of the five steps (host clock, a stream synchronise at the end; the second of two solves, the first
    warms the shapes) and the costs per step, for the default plan (kind 0), the assembled PCG (kind 2) and the dense solve (kind 3);
  - ThalloX_PlanCovariance for 7 cameras and for all cameras on a kind-2 and on a kind-3 plan after GN 2 x 10 (wall time, best of three behind a first call that
    allocates), with the info each call returns.

    python tools/ba_schur_dense_bench.py [out.json] [--ladybug]      (--ladybug: the 1723-camera shape too; its kind-2 all-cameras covariance is left out)"""
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

LM = dict(nIterations=5, lIterations=150, q_tolerance=0.1, function_tolerance=0.0)
KINDS = (("kind 0", "pcg"), ("kind 2", "schur_explicit_pcg"), ("kind 3", "schur_dense"))


def plan(p, dims, solver, lm, sampling=0, **sp):
    dev = [torch.from_numpy(x.copy()).cuda() for x in p]
    s = thallo_amd.ThalloSolver(dims, thallo_amd.energy_file("bundle_adjustment"), timing_level=0, solverkind="levenberg_marquardt" if lm else "gauss_newton")
    if lm: s.enable_lm()
    s.set_linear_solver(solver)
    mask = np.zeros(9 * dims[0], np.uint8); mask[:18] = 1
    s.hold(0, mask)
    s.set_solver_parameters(**sp)
    if sampling: s.set_kernel_sampling(sampling)
    prm = s.make_params(dev)
    return s, prm, dev


def lm_solve(p, dims, solver, sampling=0):
    """-> (ms of the five steps, costs, linear iterations per step, the plan's kernel statistics)"""
    s, prm, dev = plan(p, dims, solver, True, sampling, **LM)
    s.init(prm)
    assert s.ready(), thallo_amd.api.last_error()
    costs, iters = [s.current_cost()], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while s.step(prm):
        iters.append(len(s.alpha_beta_trace()))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    costs.append(s.current_cost())
    ks = s.kernel_stats()
    name = s.schedule_name
    s.close()
    return ms, costs, iters, ks, name


def covariance(p, dims, solver, all_cameras):
    s, prm, dev = plan(p, dims, solver, False, nIterations=2, lIterations=10)
    s.init(prm)
    while s.step(prm): pass
    torch.cuda.synchronize()
    out = {}
    for name, ids in (("7 cameras", list(range(2, 9))), ("all cameras", list(range(dims[0])))):
        if name == "all cameras" and not all_cameras: continue
        try: info = s.covariance(prm, cameras=ids)["info"]
        except RuntimeError as e:                       # (kind 3: a factor that met a pivot that is not positive -- the float32 S is not positive definite there)
            out[name] = {"refused": str(e)}
            continue
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = s.covariance(prm, cameras=ids)["info"]
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"ms": round(min(ts), 3), "ms_all": [round(t, 3) for t in ts], "info": info}
    s.close()
    return out


shapes = [dict(C=48, P=1200, O=5000, band=16), dict(C=200, P=6000, O=26000), dict(C=600, P=40000, O=170000)]
if "--ladybug" in sys.argv: shapes.append(dict())
res = {"config": "bundle_adjustment, cameras {0, 1} held, timingLevel 0, one process", "LM": LM}
for kw in shapes:
    p = syn.bundle_adjustment(**kw)
    dims = (p[0].shape[0], p[1].shape[0], p[2].shape[0])
    n = 9 * dims[0]
    row = {"n": n, "dense_bytes": 4 * ((n + 31) // 32 * 32) * n}
    for label, solver in KINDS:
        lm_solve(p, dims, solver)                                       # (warms the shapes)
        ms, costs, iters, _, name = lm_solve(p, dims, solver)
        row[label] = {"ms_5_steps": round(ms, 3), "final_cost": costs[-1], "linear_iterations": iters, "schedule": name}
        print(dims, label, row[label], flush=True)
    _, _, _, ks, _ = lm_solve(p, dims, "schur_dense", sampling=1)
    # (the events around each stage: a stage is several launches -- a clear and two kernels, three per panel of 32 columns, one)
    st = {k: round(ks[k]["mean_ms"] * 1e3, 2) for k in ("SchurDenseExpand", "SchurDenseFactor", "SchurDenseSolve", "SchurW", "SchurAssemble") if k in ks and ks[k]["mean_ms"]}
    row["stages_us"] = st
    if "SchurDenseFactor" in st: row["factor_gflops"] = round(n ** 3 / 3 / (st["SchurDenseFactor"] * 1e-6) / 1e9, 1)
    print(dims, "stages", st, row.get("factor_gflops"), flush=True)
    ladybug = not kw
    row["covariance kind 2"] = covariance(p, dims, "schur_explicit_pcg", not ladybug)
    row["covariance kind 3"] = covariance(p, dims, "schur_dense", True)
    print(dims, "covariance", row["covariance kind 2"], row["covariance kind 3"], flush=True)
    res["instance %s" % (dims,)] = row
out = [a for a in sys.argv[1:] if not a.startswith("--")]
if out:
    with open(out[0], "w") as f: json.dump(res, f, indent=1)
