"""Microseconds per PCG iteration of a GENERATED energy on one GPU: a world-1 row slab (thallo_amd/distributed_generated.py: the front-end's row-slab unit in
solver_dist.cpp's flat form) against the plain generated plan of the same problem.  Per configuration: Gauss-Newton steps at two lIterations values, timed
on the host around synchronised steps; the difference over the extra iterations is the per-iteration cost (set-up, cost evaluation and the linear
update drop out).  One GPU, one rank: this is the slab form's overhead, not a scaling figure.
    python tools/generated_slab_times.py [laplacian_image|shape_from_shading|conv2d_wide ...]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
os.environ["THALLO_FRONTEND"] = "generate"          # (bundled files: the generated kernels, not the hand-written plugins)
import numpy as np
import torch

from thallo_amd import api
from thallo_amd import synthetic as syn
from thallo_amd.distributed_generated import PlanGeneratedSlabSolver

CONFIGS = {"laplacian_image": (2048, 2048), "shape_from_shading": (2048, 2048), "conv2d_wide": (1024, 1024)}


def problem(name, W, H):
    if name == "conv2d_wide":
        rng = np.random.default_rng(7)
        K = rng.uniform(0, 1, (11, 11)).astype(np.float32); K /= K.sum()
        return ([rng.uniform(0, 1, (H, W)).astype(np.float32), rng.uniform(0, 1, (H, W)).astype(np.float32), K], [W, H, 11, 11],
                os.path.join(ROOT, "tests", "energies", "conv2d_wide.t"))
    return getattr(syn, name)(W, H), [W, H], api.energy_file(name)


def per_iteration_us(solver, params, steps=3, l_lo=4, l_hi=24):
    t = {}
    for L in (l_lo, l_hi):
        solver.set_solver_parameters(nIterations=1 << 30, lIterations=L)
        solver.init(params)
        solver.step(params)                          # (warm-up: first launches, the slab unit's first use)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            solver.step(params)
        torch.cuda.synchronize()
        t[L] = time.perf_counter() - t0
    return 1e6 * (t[l_hi] - t[l_lo]) / (steps * (l_hi - l_lo))


def main():
    torch.cuda.set_device(0)
    names = sys.argv[1:] or list(CONFIGS)
    print(f"device: {torch.cuda.get_device_name(0)}")
    for name in names:
        W, H = CONFIGS[name]
        p, dims, path = problem(name, W, H)
        dev = [torch.from_numpy(x.copy()).cuda() if isinstance(x, np.ndarray) else x for x in p]
        plain = api.ThalloSolver(tuple(dims), path, timing_level=0)
        us_plain = per_iteration_us(plain, plain.make_params(dev))
        plain.close()
        slab = PlanGeneratedSlabSolver(path, dims, p, 0, 1, 10)
        us_slab = per_iteration_us(slab.solver, slab.params)
        slab.solver.close()
        print(f"{name} {W}x{H}: plain generated plan {us_plain:.1f} us / PCG iteration, world-1 slab {us_slab:.1f} us / PCG iteration (g = {slab.g})")


if __name__ == "__main__":
    main()
