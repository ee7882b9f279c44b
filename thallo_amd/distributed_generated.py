"""Row slabs of a GENERATED image-stencil energy across GPUs, one process per GPU: any `.t` file with one Unknown over {W, H} whose residuals have the
front-end's unknown-wise form (include/Thallo.h ThalloX_FrontendSlabGhostRows says which, and how many ghost rows g the file's stencil needs).  The
plan runs the front-end's row-slab unit (csrc/dsl_codegen.cpp, Generated::slab_rowdim) in solver_dist.cpp's flat form -- the driver that carries
shape_from_shading's hand-written slabs: g ghost rows per interior side, global pixel coordinates (global_row0 / global_rows), Gauss-Newton in the
single-reduction form or, with lm=True, the Levenberg-Marquardt branch; either transport.
Bundled `.t` files have hand-written plugins; they take this path only under THALLO_FRONTEND=generate, which must be set before the library loads.
This module is set-up only: the row split, the local buffers (the {W, H} inputs sliced, everything else passed whole), the all-gather callback.
"""
import numpy as np
import torch

from . import api
from .distributed import SlabLayout, library_rccl, torch_allgather


def declarations(energy_file, global_dims):
    """The file's inputs as the front-end reads them (ThalloX_FrontendTextDims, what = 0): {slot: (kind, dims)}, kind in unknown / array / sparse / param,
    dims = dimension names (arrays and unknowns)."""
    import ctypes as C
    L = api.lib()
    L.ThalloX_FrontendTextDims.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    L.ThalloX_FrontendTextDims.restype = C.c_int
    d = (C.c_uint * len(global_dims))(*global_dims)
    buf = C.create_string_buffer(1 << 16)
    if L.ThalloX_FrontendTextDims(str(energy_file).encode(), 0, d, buf, len(buf)) < 0:
        raise RuntimeError(api.last_error())
    out, dim_names = {}, []
    for line in buf.value.decode().splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "dims:":
            dim_names = w[1:]
        elif w[0] in ("unknown", "array", "sparse", "param"):
            slot = int(w[w.index("slot") + 1])
            dims = w[w.index("over") + 1:] if "over" in w else []
            dims = [x for x in dims if x in dim_names]
            out[slot] = (w[0], dims)
    return out, dim_names


class PlanGeneratedSlabSolver:
    """One rank's slab of a generated energy.  problem_params: the GLOBAL problem, indexed like the file's Inputs{} slots (arrays over {W, H} as [H, W] or
    [H, W, channels], other arrays and scalars as the whole-image plan takes them).  global_dims: the problem's dimensions (W, H first, then any others)."""

    def __init__(self, energy_file, global_dims, problem_params, rank, world, l_iters, lm=False, group=None, device_exchange=True):
        self.g = api.slab_ghost_rows(energy_file, global_dims)
        decl, dim_names = declarations(energy_file, global_dims)
        W, H = int(global_dims[0]), int(global_dims[1])
        unknowns = [s for s, (k, _) in decl.items() if k == "unknown"]
        wh = unknowns and decl[unknowns[0]][1]           # the unknown's {W, H} names
        self.lay = lay = SlabLayout(H, rank, world, ghost=self.g)
        self.W, self.H, self.rank, self.world = W, H, rank, world
        self.unknown_slot = unknowns[0]
        dev = torch.device("cuda", torch.cuda.current_device())
        self.params_dev = []
        for slot, p in enumerate(problem_params):
            kind, dims = decl.get(slot, ("param", []))
            if isinstance(p, np.ndarray):
                a = lay.local(p) if (kind in ("unknown", "array") and dims == wh) else p
                self.params_dev.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
            else:
                self.params_dev.append(p)
        local_dims = list(global_dims)
        local_dims[1] = lay.Hl
        self.solver = api.ThalloSolver(tuple(local_dims), energy_file, timing_level=0)
        if lm:
            self.solver.enable_lm()
        self.l_iters = l_iters
        self.solver.set_solver_parameters(nIterations=1 << 30, lIterations=l_iters)
        self.library_rccl = library_rccl(self.solver, rank, world, group)
        ag = torch_allgather(group, dev) if world > 1 and not self.library_rccl else None
        self.solver.set_distributed(rank, world, lay.row0, lay.row1, allgather=ag, device_exchange=device_exchange,
                                    global_row0=lay.g0 - lay.top, global_rows=H)
        self.params = self.solver.make_params(self.params_dev)

    def solve(self, n_iters, **solver_params):
        """Init + up to n_iters Steps (LM may stop earlier, on every rank alike); returns the cost trajectory"""
        self.solver.set_solver_parameters(nIterations=n_iters, **solver_params)
        self.solver.init(self.params)
        if not self.solver.ready():
            raise RuntimeError("Thallo_ProblemInit failed: " + api.last_error())
        costs = [self.solver.current_cost()]
        while self.solver.step(self.params):
            costs.append(self.solver.current_cost())
        final = self.solver.current_cost()
        if len(costs) == 1 or final != costs[-1]:
            costs.append(final)
        return costs

    def owned(self):
        """This rank's owned rows of the unknown, [rows, W] or [rows, W, channels]"""
        lay = self.lay
        return self.params_dev[self.unknown_slot][lay.row0:lay.row1].cpu().numpy()
