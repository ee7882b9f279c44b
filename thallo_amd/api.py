"""ctypes mirror of include/Thallo.h (the drop-in C API) and a ThalloSolver harness class.

The class mirrors the reference's application harness, examples/shared/ThalloSolver.h:40-112
(ctor = NewState -> ProblemDefine -> ProblemPlan; solve = SetSolverParameter* -> Solve, or
Init + while(Step) with a cost read after every step like launchProfiledSolve,
examples/shared/ThalloUtils.h:75-92), so parity tests read like the reference's own programs.

There is no CPU fallback: a missing libThallo.so or a missing GPU raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libThallo.so")
ENERGY_DIR = os.path.join(_HERE, "energies")


class InitializationParameters(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("doublePrecision", "verbosityLevel", "timingLevel",
                                       "threadsPerBlock", "useAutoscheduler", "cpuOnly")]


class PerformanceEntry(C.Structure):
    _fields_ = [("count", C.c_uint), ("minMS", C.c_double), ("maxMS", C.c_double),
                ("meanMS", C.c_double), ("stddevMS", C.c_double)]


class PerformanceSummary(C.Structure):
    _fields_ = [(n, PerformanceEntry) for n in ("total", "nonlinearIteration", "nonlinearSetup",
                                                "linearSolve", "nonlinearResolve")]


class SumT(C.Structure):      # thallo_sum_t of include/thallo_hip.h
    _fields_ = [("partials", C.c_void_p), ("count", C.c_int)]


class DistT(C.Structure):
    """thallo_dist_t (include/thallo_hip.h): mailboxes + neighbour r vectors of the device-side multi-GPU exchange"""
    _fields_ = [("mail", C.c_void_p), ("peer_mail", C.c_void_p * 8), ("peer_r", C.c_void_p * 2), ("peer_off_o", C.c_long * 2),
                ("peer_off_a", C.c_long * 2), ("ctl", C.c_void_p), ("world", C.c_int), ("rank", C.c_int)]


class PrevT(C.Structure):     # thallo_prev_t of include/thallo_hip.h
    _fields_ = [("alphaD_partials", C.c_void_p), ("s12_partials", C.c_void_p), ("count", C.c_int), ("alphaD_word", C.c_void_p), ("betaN_word", C.c_void_p)]


class IwIterT(C.Structure):
    """thallo_iw_iter_t (include/thallo_hip.h): everything a launch of the one-kernel PCG iteration carries.  tests/test_march_classes.py pins
    its size against thallo_hip_iw_iter_size()."""
    _fields_ = ([(n, C.c_int) for n in ("W", "H", "row0", "row1")]
                + [(n, C.c_void_p) for n in ("cs", "urshape", "flags", "pre", "irregular")]
                + [("w_fit", C.c_float), ("w_reg", C.c_float)]
                + [(n, C.c_void_p) for n in ("r_in", "r_out", "Ap_in", "Ap_out", "p_in", "p_out", "delta")] + [("mode", C.c_int)]
                + [(n, SumT) for n in ("alphaN_prev", "alphaD_prev", "betaN_prev", "alphaN_prev2", "alphaD_prev2")]
                + [(n, C.c_void_p) for n in ("alphaD_out", "s12_out", "fin_tickets", "alphaD_word", "betaN_word")] + [("slot0", C.c_int)]
                + [("dist", C.POINTER(DistT)), ("prev", C.POINTER(PrevT)), ("prev_slot0", C.c_int), ("gs", C.c_void_p)])


IW_ITER_TILE, IW_ITER_MARCH, IW_ITER_MARCH_RC = 0, 1, 2      # THALLO_IW_ITER_* of include/thallo_hip.h


class SegsT(C.Structure):     # thallo_segs_t of include/thallo_hip.h
    _fields_ = [("off", C.c_long * 8), ("len", C.c_long * 8), ("n", C.c_int)]


INT_PARAMS = ("nIterations", "lIterations", "residual_reset_period", "nIter")

_lib = None


# include/Thallo.h: ThalloX_AllGatherFn / ThalloX_Distributed
AllGatherFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p)
AllReduceFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p)


class DistributedT(C.Structure):
    _fields_ = [("rank", C.c_int), ("world", C.c_int), ("row0", C.c_uint), ("row1", C.c_uint),
                ("allgather", AllGatherFn), ("user", C.c_void_p), ("device_exchange", C.c_int),
                ("global_row0", C.c_uint), ("global_rows", C.c_uint), ("allreduce", AllReduceFn)]


class CovarianceOptions(C.Structure):      # ThalloX_CovarianceOptions of include/Thallo.h
    _fields_ = [("rel_tol", C.c_float), ("max_iterations", C.c_int)]


class CovarianceInfo(C.Structure):         # ThalloX_CovarianceInfo
    _fields_ = [("iterations", C.c_long), ("columns", C.c_long), ("not_converged", C.c_long), ("nan_blocks", C.c_long), ("worst_residual", C.c_float)]


def lib():
    """Load libThallo.so; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("THALLO_LIB") or LIB_PATH          # THALLO_LIB: tools only (an A/B build from `make VARIANT=...`, tools/ab/)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(make -C thallo_amd/csrc). There is no CPU fallback.")
    L = C.CDLL(path)
    vp, vpp = C.c_void_p, C.POINTER(C.c_void_p)
    L.Thallo_NewState.argtypes = [InitializationParameters]; L.Thallo_NewState.restype = vp
    L.Thallo_ProblemDefine.argtypes = [vp, C.c_char_p, C.c_char_p]; L.Thallo_ProblemDefine.restype = vp
    L.Thallo_ProblemDelete.argtypes = [vp, vp]
    L.Thallo_ProblemPlan.argtypes = [vp, vp, C.POINTER(C.c_uint)]; L.Thallo_ProblemPlan.restype = vp
    L.Thallo_PlanFree.argtypes = [vp, vp]
    L.Thallo_SetSolverParameter.argtypes = [vp, vp, C.c_char_p, vp]
    L.Thallo_GetSolverParameter.argtypes = [vp, vp, C.c_char_p, vp]
    L.Thallo_ProblemSolve.argtypes = [vp, vp, vpp]
    L.Thallo_ProblemInit.argtypes = [vp, vp, vpp]
    L.Thallo_ProblemStep.argtypes = [vp, vp, vpp]; L.Thallo_ProblemStep.restype = C.c_int
    L.Thallo_ProblemCurrentCost.argtypes = [vp, vp]; L.Thallo_ProblemCurrentCost.restype = C.c_double
    L.Thallo_GetPerformanceSummary.argtypes = [vp, vp, C.POINTER(PerformanceSummary)]
    L.ThalloX_SetStream.argtypes = [vp, vp]
    L.ThalloX_SetKernelSampling.argtypes = [vp, C.c_int]
    L.ThalloX_GetKernelStat.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_double)]
    L.ThalloX_GetKernelStat.restype = C.c_int
    L.ThalloX_GetKernelStatOwn.argtypes = [vp, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_double)]
    L.ThalloX_GetKernelStatOwn.restype = C.c_int
    L.ThalloX_ResetKernelStats.argtypes = [vp]
    L.ThalloX_GetAlphaBetaTrace.argtypes = [vp, vp, C.c_int]; L.ThalloX_GetAlphaBetaTrace.restype = C.c_int
    L.ThalloX_EnableLM.argtypes = [vp, C.c_int]
    L.ThalloX_PlanEnergyName.argtypes = [vp]; L.ThalloX_PlanEnergyName.restype = C.c_char_p
    L.ThalloX_LastError.restype = C.c_char_p
    L.ThalloX_PlanReady.argtypes = [vp]; L.ThalloX_PlanReady.restype = C.c_int
    L.ThalloX_PlanScheduleName.argtypes = [vp]; L.ThalloX_PlanScheduleName.restype = C.c_char_p
    L.ThalloX_PlanSetPreconditioner.argtypes = [vp, C.c_int]; L.ThalloX_PlanSetPreconditioner.restype = C.c_int
    L.ThalloX_PlanPreconditionerFallbacks.argtypes = [vp]; L.ThalloX_PlanPreconditionerFallbacks.restype = C.c_int
    L.ThalloX_PlanSetLinearSolver.argtypes = [vp, C.c_int]; L.ThalloX_PlanSetLinearSolver.restype = C.c_int
    L.ThalloX_PlanSchurHeldPoints.argtypes = [vp]; L.ThalloX_PlanSchurHeldPoints.restype = C.c_int
    L.ThalloX_PlanSchurBlocks.argtypes = [vp]; L.ThalloX_PlanSchurBlocks.restype = C.c_int
    if hasattr(L, "ThalloX_PlanSchurDenseNonPositive"):      # (THALLO_LIB may name an A/B build from before the call existed)
        L.ThalloX_PlanSchurDenseNonPositive.argtypes = [vp]; L.ThalloX_PlanSchurDenseNonPositive.restype = C.c_int
    if hasattr(L, "ThalloX_PlanSetCoarseAggregates"):      # (likewise)
        L.ThalloX_PlanSetCoarseAggregates.argtypes = [vp, C.c_int, vp, C.c_long]; L.ThalloX_PlanSetCoarseAggregates.restype = C.c_int
        L.ThalloX_PlanCoarseSpace.argtypes = [vp, vp]; L.ThalloX_PlanCoarseSpace.restype = C.c_int
    L.ThalloX_PlanSetHeldUnknowns.argtypes = [vp, C.c_int, vp, C.c_long]; L.ThalloX_PlanSetHeldUnknowns.restype = C.c_int
    L.ThalloX_PlanHeldUnknowns.argtypes = [vp]; L.ThalloX_PlanHeldUnknowns.restype = C.c_long
    if hasattr(L, "ThalloX_PlanSetPrior"):           # (THALLO_LIB may name an A/B build from before the call existed: tools/ba_prior_bench.py --ab)
        L.ThalloX_PlanSetPrior.argtypes = [vp, C.c_int, vp, vp, C.c_long]; L.ThalloX_PlanSetPrior.restype = C.c_int
        L.ThalloX_PlanPriorTerms.argtypes = [vp]; L.ThalloX_PlanPriorTerms.restype = C.c_long
        L.ThalloX_PlanPriorCost.argtypes = [vp, C.POINTER(C.c_double)]; L.ThalloX_PlanPriorCost.restype = C.c_int
    if hasattr(L, "ThalloX_PlanSetRobustLoss"):      # (THALLO_LIB may name an A/B build from before the call existed: tools/ba_robust_bench.py --ab)
        L.ThalloX_PlanSetRobustLoss.argtypes = [vp, C.c_int, C.c_float]; L.ThalloX_PlanSetRobustLoss.restype = C.c_int
        L.ThalloX_PlanRobustWeights.argtypes = [vp, vp, C.c_long]; L.ThalloX_PlanRobustWeights.restype = C.c_long
    if hasattr(L, "ThalloX_PlanCovariance"):         # (likewise: an A/B build from before the call existed)
        L.ThalloX_PlanCovariance.argtypes = [vp, vpp, C.c_int, vp, C.c_long, vp, C.POINTER(CovarianceOptions), C.POINTER(CovarianceInfo)]
        L.ThalloX_PlanCovariance.restype = C.c_long
    L.ThalloX_PlanSetDistributed.argtypes = [vp, C.POINTER(DistributedT)]; L.ThalloX_PlanSetDistributed.restype = C.c_int
    L.ThalloX_PlanDistributedInfo.argtypes = [vp]; L.ThalloX_PlanDistributedInfo.restype = C.c_char_p
    L.ThalloX_DistributedControl.argtypes = [vp, C.c_int, C.c_int]; L.ThalloX_DistributedControl.restype = C.c_int
    L.ThalloX_UnknownsChanged.argtypes = [vp, vp]
    L.ThalloX_RcclUniqueId.argtypes = [vp]; L.ThalloX_RcclUniqueId.restype = C.c_int
    L.ThalloX_PlanUseRccl.argtypes = [vp, vp, C.c_int, C.c_int]; L.ThalloX_PlanUseRccl.restype = C.c_int
    L.ThalloX_RcclSelfTest.argtypes = []; L.ThalloX_RcclSelfTest.restype = C.c_int
    L.ThalloX_RcclAvailable.argtypes = []; L.ThalloX_RcclAvailable.restype = C.c_int
    L.ThalloX_DistributedKernelOnly.argtypes = [vp, C.c_int]; L.ThalloX_DistributedKernelOnly.restype = C.c_int
    L.ThalloX_ProblemFileHash.argtypes = [C.c_char_p, C.c_char_p, C.c_int]; L.ThalloX_ProblemFileHash.restype = C.c_ulonglong
    L.ThalloX_ProblemFileSchedule.argtypes = [C.c_char_p]; L.ThalloX_ProblemFileSchedule.restype = C.c_int
    # --- kernel shim entry points that python drives directly (distributed driver, bench, tests): typed, so a
    #     signature drift raises an ArgumentError instead of corrupting the call
    fl, ci, cl = C.c_float, C.c_int, C.c_long
    L.thallo_hip_vector_elems.argtypes = [cl]; L.thallo_hip_vector_elems.restype = cl
    L.thallo_hip_finish_sum.argtypes = [SumT, vp, vp]
    L.thallo_hip_iw_cost.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp, fl, fl, vp, vp]
    L.thallo_hip_iw_pcg_init.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp, fl, fl, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.thallo_hip_iw_pcg_step1.argtypes = [ci, ci, ci, ci, vp, vp, vp, fl, fl, vp, vp, vp, vp, vp, ci, SumT, SumT, SumT, SumT, SumT, vp, vp, vp, vp]
    L.thallo_hip_linear_update2.argtypes = [vp, vp, vp, SumT, SumT, vp, SumT, SumT, cl, vp]
    L.thallo_hip_ipc_alloc.argtypes = [C.c_long, C.POINTER(vp), vp]
    L.thallo_hip_ipc_alloc2.argtypes = [C.c_long, C.POINTER(vp), vp, C.POINTER(ci)]
    L.thallo_hip_ipc_open.argtypes = [vp, C.POINTER(vp)]
    L.thallo_hip_ipc_close.argtypes = [vp]; L.thallo_hip_ipc_free.argtypes = [vp]
    L.thallo_hip_dist_begin_step.argtypes = [DistT, vp]
    L.thallo_hip_dist_collect.argtypes = [DistT, ci, ci, vp, vp]
    L.thallo_hip_dist_error.argtypes = [DistT, ci, vp]
    L.thallo_hip_slab_pack_iter.argtypes = [vp, SegsT, vp, vp, ci, vp, vp]
    L.thallo_hip_slab_unpack_iter.argtypes = [vp, SegsT, vp, SegsT, vp, vp, cl, ci, SumT, vp, vp, vp]
    L.thallo_hip_dist_exchange.argtypes = [DistT, ci, SumT, vp, vp]
    L.thallo_hip_dist_exchange_iter.argtypes = [DistT, ci, vp, vp, ci, SumT, vp, vp, vp]
    L.thallo_hip_iw_pcg_iter.argtypes = [ci, C.POINTER(IwIterT), vp]
    if hasattr(L, "thallo_hip_iw_iter_size"):      # (THALLO_LIB may name an A/B build from before the block existed)
        L.thallo_hip_iw_iter_size.argtypes = []; L.thallo_hip_iw_iter_size.restype = C.c_uint
    L.thallo_hip_iw_urshape_irregular.argtypes = [ci, ci, vp, vp, vp]
    L.thallo_hip_march_debug_set.argtypes = [ci, ci]
    L.thallo_hip_iw_pcg_iter_finish.argtypes = [vp, vp, ci, SumT, vp, vp, vp]
    L.thallo_hip_iw_pcg_step2_dist.argtypes = [ci, ci, ci, ci, vp, fl, fl, vp, vp, SumT, SumT, DistT, vp, vp]
    L.thallo_hip_iw_pcg_step2.argtypes = [ci, ci, ci, ci, vp, fl, fl, vp, vp, vp, vp, SumT, SumT, vp, vp, vp]
    L.thallo_hip_iw_apply_jtj.argtypes = [ci, ci, ci, ci, vp, vp, vp, fl, fl, vp, vp, vp, vp, vp]
    L.thallo_hip_pcg_step2.argtypes = [vp, vp, vp, vp, cl, SumT, SumT, vp, vp]
    L.thallo_hip_pcg_step2_ranges.argtypes = [vp, vp, vp, vp, cl, cl, cl, cl, SumT, SumT, vp, vp]
    L.thallo_hip_linear_update.argtypes = [vp, vp, vp, cl, SumT, SumT, vp]
    L.thallo_hip_slab_pack.argtypes = [vp, SegsT, SumT, vp, vp]
    L.thallo_hip_slab_unpack.argtypes = [vp, SegsT, vp, SegsT, vp, vp, cl, ci, vp, vp]
    _lib = L
    return L


def energy_file(name):
    """Path of a bundled problem specification (thallo_amd/energies/<name>.t)."""
    p = os.path.join(ENERGY_DIR, name if name.endswith(".t") else name + ".t")
    if not os.path.exists(p):
        raise FileNotFoundError(p)
    return p


def last_error():
    return lib().ThalloX_LastError().decode()


def slab_ghost_rows(path, dims):
    """Ghost rows a row slab of the generated energy in `path` needs towards each neighbour (include/Thallo.h ThalloX_FrontendSlabGhostRows; host only).
    dims: the problem's dimensions.  Raises ValueError, naming the construct, when the file has no row-slab form."""
    L = lib()
    L.ThalloX_FrontendSlabGhostRows.argtypes = [C.c_char_p, C.c_void_p]
    L.ThalloX_FrontendSlabGhostRows.restype = C.c_int
    d = (C.c_uint * len(dims))(*[int(x) for x in dims])
    g = L.ThalloX_FrontendSlabGhostRows(os.fsencode(path), d)
    if g < 0:
        raise ValueError(last_error())
    return g


def rccl_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0); raises when the library cannot bind RCCL"""
    buf = (C.c_ubyte * 128)()
    if lib().ThalloX_RcclUniqueId(C.addressof(buf)) != 0:
        raise RuntimeError("ThalloX_RcclUniqueId failed: " + last_error())
    return bytes(buf)


def _ptr_of(x):
    """Device pointer of a torch tensor, host pointer of a ctypes scalar, or a raw int."""
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, (C.c_float, C.c_int, C.c_double, C.c_uint)):
        return C.addressof(x)
    if isinstance(x, int):
        return x
    raise TypeError(f"cannot turn {type(x)} into a problem parameter")


class ThalloSolver:
    """NewState -> ProblemDefine -> ProblemPlan, like examples/shared/ThalloSolver.h:43-74."""

    def __init__(self, dims, thallofile, solverkind="gauss_newton", verbosity=0, timing_level=1,
                 autoschedule=1, double_precision=False, cpu_only=False):
        L = lib()
        ip = InitializationParameters(int(double_precision), verbosity, timing_level, 0, autoschedule, int(cpu_only))
        self._L = L
        self.state = L.Thallo_NewState(ip)
        if not self.state:
            raise RuntimeError("Thallo_NewState failed: " + last_error())
        self.problem = L.Thallo_ProblemDefine(self.state, os.fsencode(thallofile), solverkind.encode())
        if not self.problem:
            raise RuntimeError("Thallo_ProblemDefine failed: " + last_error())
        self._dims = (C.c_uint * 10)(*dims)          # retained by the plan (thallo.t:1419)
        self.plan = L.Thallo_ProblemPlan(self.state, self.problem, self._dims)
        if not self.plan:
            raise RuntimeError("Thallo_ProblemPlan failed: " + last_error())
        self._keep = None

    def close(self):
        if getattr(self, "plan", None):
            self._L.Thallo_PlanFree(self.state, self.plan); self.plan = None
        if getattr(self, "problem", None):
            self._L.Thallo_ProblemDelete(self.state, self.problem); self.problem = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def energy_name(self):
        return self._L.ThalloX_PlanEnergyName(self.plan).decode()

    @property
    def schedule_name(self):
        return self._L.ThalloX_PlanScheduleName(self.plan).decode()

    def set_solver_parameters(self, **kw):
        for k, v in kw.items():
            val = C.c_int(int(v)) if k in INT_PARAMS else C.c_float(float(v))
            self._L.Thallo_SetSolverParameter(self.state, self.plan, k.encode(), C.addressof(val))

    def get_solver_parameter(self, name):
        val = C.c_int() if name in INT_PARAMS else C.c_float()
        self._L.Thallo_GetSolverParameter(self.state, self.plan, name.encode(), C.addressof(val))
        return val.value

    def make_params(self, problem_params):
        """void** indexed like the .t Inputs{}: tensors -> device pointers, python floats -> host float*."""
        keep = []
        ptrs = []
        for p in problem_params:
            if isinstance(p, np.float64):       # Param(thallo_float, ...) under double_precision=True: a host double
                p = C.c_double(float(p))
            elif isinstance(p, (float, np.float32)):
                p = C.c_float(float(p))
            keep.append(p)
            ptrs.append(_ptr_of(p))
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        self._keep = (keep, arr)
        return arr

    def init(self, params):
        self._L.Thallo_ProblemInit(self.state, self.plan, params)

    def ready(self):
        return self._L.ThalloX_PlanReady(self.plan) == 1

    def step(self, params):
        return self._L.Thallo_ProblemStep(self.state, self.plan, params)

    def current_cost(self):
        return self._L.Thallo_ProblemCurrentCost(self.state, self.plan)

    def solve(self, problem_params, profiled=False, **solver_params):
        """Returns (final_cost, costs): costs[0] is the initial cost, costs[k] the cost after GN step k
        when profiled (Init + while(Step) + CurrentCost, ThalloUtils.h:75-92), else just [final]."""
        self.set_solver_parameters(**solver_params)
        params = problem_params if isinstance(problem_params, C.Array) else self.make_params(problem_params)
        costs = []
        if profiled:
            self.init(params)
            costs.append(self.current_cost())
            while self.step(params):
                costs.append(self.current_cost())
        else:
            self._L.Thallo_ProblemSolve(self.state, self.plan, params)
        final = self.current_cost()
        if not profiled:
            costs.append(final)
        return final, costs

    def performance_summary(self):
        s = PerformanceSummary()
        self._L.Thallo_GetPerformanceSummary(self.state, self.plan, C.byref(s))
        return {n: {"count": getattr(s, n).count, "minMS": getattr(s, n).minMS, "maxMS": getattr(s, n).maxMS,
                    "meanMS": getattr(s, n).meanMS, "stddevMS": getattr(s, n).stddevMS} for n, _ in s._fields_}

    # ---- extensions
    def set_stream(self, stream_ptr):
        self._L.ThalloX_SetStream(self.plan, C.c_void_p(stream_ptr))

    def set_distributed(self, rank, world, row0, row1, allgather=None, device_exchange=True, global_row0=0, global_rows=0, allreduce=None):
        """Collective (include/Thallo.h ThalloX_PlanSetDistributed): this plan is rank `rank`'s row slab; `allgather(send_ptr, recv_ptr,
        bytes_per_rank, stream_ptr) -> None` moves DEVICE bytes (thallo_amd.distributed.torch_allgather builds one over torch.distributed)."""
        def _cb(_user, send, recv, nbytes, stream):
            try:
                allgather(send, recv, nbytes, stream or 0)
                return 0
            except Exception:      # noqa: BLE001 - an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return -1
        def _ar(_user, buf, count, stream):
            try:
                allreduce(buf, count, stream or 0)
                return 0
            except Exception:      # noqa: BLE001
                import traceback
                traceback.print_exc()
                return -1
        self._dist_cb = AllGatherFn(_cb) if allgather is not None else C.cast(None, AllGatherFn)      # kept alive with the plan
        self._dist_ar = AllReduceFn(_ar) if allreduce is not None else C.cast(None, AllReduceFn)
        cfg = DistributedT(rank, world, row0, row1, self._dist_cb, None, 1 if device_exchange else 0, global_row0, global_rows, self._dist_ar)
        if self._L.ThalloX_PlanSetDistributed(self.plan, C.byref(cfg)) != 0:
            raise RuntimeError("ThalloX_PlanSetDistributed failed: " + last_error())

    def set_ghost_exchange(self, boundary_units, ghost_units, ghost_src_rank, ghost_src_pos):
        """Before set_distributed (include/Thallo.h ThalloX_PlanSetGhostExchange): this plan is a rank's LOCAL sub-problem of a partitioned graph energy -- owned units
        first, then ghosts; the lists say which owned units travel and where each ghost's values come from (thallo_amd.distributed_graph.GhostPartition builds them)."""
        import numpy as np
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (boundary_units, ghost_units, ghost_src_rank, ghost_src_pos)]
        self._L.ThalloX_PlanSetGhostExchange.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._L.ThalloX_PlanSetGhostExchange.restype = C.c_int
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        if self._L.ThalloX_PlanSetGhostExchange(self.plan, int(arrs[0].size), ptr(arrs[0]), int(arrs[1].size), ptr(arrs[1]), ptr(arrs[2]), ptr(arrs[3])) != 0:
            raise RuntimeError("ThalloX_PlanSetGhostExchange failed: " + last_error())

    def use_rccl(self, unique_id, rank, world):
        """Collective, before set_distributed: the plan makes its own RCCL communicator from the 128-byte id (rccl_unique_id() on rank 0, handed to every
        rank by the application); set_distributed without callbacks then means ncclAllGather / ncclAllReduce inside the library."""
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
        if self._L.ThalloX_PlanUseRccl(self.plan, C.addressof(buf), rank, world) != 0:
            raise RuntimeError("ThalloX_PlanUseRccl failed: " + last_error())

    def rccl_info(self):
        """{world, device, rank} as the plan's own RCCL communicator reports them (ncclCommCount / CuDevice / UserRank); -1 = no communicator."""
        out = (C.c_int * 3)(-1, -1, -1)
        self._L.ThalloX_PlanRcclInfo.argtypes = [C.c_void_p, C.c_void_p]; self._L.ThalloX_PlanRcclInfo.restype = None
        self._L.ThalloX_PlanRcclInfo(self.plan, C.addressof(out))
        return {"world": out[0], "device": out[1], "rank": out[2]}

    def distributed_info(self):
        import json
        t = self._L.ThalloX_PlanDistributedInfo(self.plan).decode()
        return json.loads(t) if t else {}

    def distributed_error(self, clear=True):
        return self._L.ThalloX_DistributedControl(self.plan, 0, 1 if clear else 0)

    def distributed_use_allgather(self):
        return self._L.ThalloX_DistributedControl(self.plan, 1, 0)

    def distributed_kernel_only(self, reps):
        return self._L.ThalloX_DistributedKernelOnly(self.plan, reps)

    def unknowns_changed(self):
        """The caller rewrote unknowns / inputs in place between two LM steps (include/Thallo.h ThalloX_UnknownsChanged)."""
        self._L.ThalloX_UnknownsChanged(self.state, self.plan)

    def enable_lm(self, on=True):
        """Run the LM branch of gauss_newton.t (dead as shipped in the reference, see include/Thallo.h)."""
        self._L.ThalloX_EnableLM(self.plan, 1 if on else 0)

    PRECONDITIONERS = {"jacobi": 0, "block_jacobi": 1, "two_level": 2}      # THALLOX_PRECOND_* of include/Thallo.h

    def set_preconditioner(self, kind):
        """"jacobi" (the reference's, default), "block_jacobi" (bundle_adjustment: 9 x 9 camera and 3 x 3 point blocks) or "two_level" (on the "schur_explicit_pcg" linear
        solver alone -- init() fails otherwise: the camera blocks plus a dense coarse correction over aggregates of co-visible cameras, for covariances and tight reduced
        solves); before init().  Raises, with the library's reason, where the plan has no block form (include/Thallo.h ThalloX_PlanSetPreconditioner)."""
        if kind not in self.PRECONDITIONERS:
            raise ValueError(f"preconditioner {kind!r}: expected one of {sorted(self.PRECONDITIONERS)}")
        if self._L.ThalloX_PlanSetPreconditioner(self.plan, self.PRECONDITIONERS[kind]) != 0:
            raise RuntimeError("ThalloX_PlanSetPreconditioner failed: " + last_error())

    def set_coarse_aggregates(self, cameras_per_aggregate=None, aggregates=None):
        """The aggregates of the "two_level" preconditioner (include/Thallo.h ThalloX_PlanSetCoarseAggregates): nothing given = the default size, `cameras_per_aggregate`
        = greedy aggregates of at most that many co-visible cameras, or `aggregates` = one dense aggregate id per camera (the caller's camera ids); before init()."""
        if aggregates is not None:
            import numpy as np
            a = np.ascontiguousarray(np.asarray(aggregates), dtype=np.int32).reshape(-1)
            rc = self._L.ThalloX_PlanSetCoarseAggregates(self.plan, 0, a.ctypes.data_as(C.c_void_p), int(a.size))
        else:
            rc = self._L.ThalloX_PlanSetCoarseAggregates(self.plan, int(cameras_per_aggregate or 0), None, 0)
        if rc != 0:
            raise RuntimeError("ThalloX_PlanSetCoarseAggregates failed: " + last_error())

    def coarse_space(self):
        """{"aggregates", "coarse_scalars", "identity_rows", "failed_factors"} of the "two_level" preconditioner since init(), or None when it does not run."""
        out = (C.c_long * 4)()
        if self._L.ThalloX_PlanCoarseSpace(self.plan, out) != 0:
            return None
        return {"aggregates": out[0], "coarse_scalars": out[1], "identity_rows": out[2], "failed_factors": out[3]}

    def preconditioner_fallbacks(self):
        """Blocks of the last step that fell back to their diagonal (-1: the block form does not run)."""
        return self._L.ThalloX_PlanPreconditionerFallbacks(self.plan)

    LINEAR_SOLVERS = {"pcg": 0, "schur_pcg": 1, "schur_explicit_pcg": 2, "schur_dense": 3}      # THALLOX_SOLVER_* of include/Thallo.h

    def set_linear_solver(self, kind):
        """"pcg" (the full system, default), "schur_pcg" (bundle_adjustment: the points eliminated through their 3 x 3 blocks, PCG on the cameras, preconditioned by the
        camera blocks whatever set_preconditioner was given; S x applied matrix-free) or "schur_explicit_pcg" (the same solve with the reduced camera matrix S assembled
        once per step as a block-sparse matrix: one mat-vec per iteration; init() fails, naming the bytes, where its structure does not fit a quarter of the free device
        memory) or "schur_dense" (that assembly, then a dense float32 Cholesky factor of S on the device instead of a PCG loop: the exact solve for up to a few hundred
        cameras; lIterations, q_tolerance and the preconditioner are ignored; a step whose factor meets a pivot that is not positive returns 0 with the unknowns unchanged
        and last_error() naming the camera and scalar -- fix the gauge with hold() or use LM); before init().  Raises, with the library's reason, where the plan has no
        Schur form (include/Thallo.h ThalloX_PlanSetLinearSolver)."""
        if kind not in self.LINEAR_SOLVERS:
            raise ValueError(f"linear solver {kind!r}: expected one of {sorted(self.LINEAR_SOLVERS)}")
        if self._L.ThalloX_PlanSetLinearSolver(self.plan, self.LINEAR_SOLVERS[kind]) != 0:
            raise RuntimeError("ThalloX_PlanSetLinearSolver failed: " + last_error())

    def schur_held_points(self):
        """Points the last step's elimination held fixed (-1: the Schur form does not run)."""
        return self._L.ThalloX_PlanSchurHeldPoints(self.plan)

    def schur_blocks(self):
        """Stored 9 x 9 blocks of the assembled reduced camera matrix after init() (-1: the assembled form does not run)."""
        return self._L.ThalloX_PlanSchurBlocks(self.plan)

    def schur_dense_nonpositive(self):
        """Scalars of the last dense factor whose diagonal of S was not positive and that got the identity's row and column (-1: "schur_dense" does not run)."""
        return self._L.ThalloX_PlanSchurDenseNonPositive(self.plan)

    def hold(self, input, mask):
        """Unknowns that are not to move (include/Thallo.h ThalloX_PlanSetHeldUnknowns): `input` is the Inputs{} index of an Unknown (bundle_adjustment: 0 cameras,
        1 points), `mask` an array of elements x components flags in the caller's ids (nonzero = held), or None to clear that input's mask; before init().  Raises, with
        the library's reason, where the plan cannot hold unknowns."""
        if mask is None:
            rc = self._L.ThalloX_PlanSetHeldUnknowns(self.plan, int(input), None, 0)
        else:
            import numpy as np
            m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).reshape(-1)
            rc = self._L.ThalloX_PlanSetHeldUnknowns(self.plan, int(input), m.ctypes.data_as(C.c_void_p), int(m.size))
        if rc != 0:
            raise RuntimeError("ThalloX_PlanSetHeldUnknowns failed: " + last_error())

    def held_unknowns(self):
        """Scalars held since the last init() (-1: no mask in force)."""
        return self._L.ThalloX_PlanHeldUnknowns(self.plan)

    def set_prior(self, input, mean, weight):
        """Gaussian priors 1/2 w (x - mean)^2 on single scalars (include/Thallo.h ThalloX_PlanSetPrior): `input` is the Inputs{} index of an Unknown (bundle_adjustment:
        0 cameras, 1 points), `mean` and `weight` arrays of elements x components floats in the caller's ids (weight = 1 / sigma^2, 0 = no prior on that scalar), or
        weight None to clear that input's prior; before init().  Raises, with the library's reason, where the plan cannot take priors."""
        if weight is None:
            rc = self._L.ThalloX_PlanSetPrior(self.plan, int(input), None, None, 0)
        else:
            import numpy as np
            w = np.ascontiguousarray(weight, dtype=np.float32).reshape(-1)
            m = np.ascontiguousarray(mean, dtype=np.float32).reshape(-1)
            if m.size != w.size:
                raise ValueError("set_prior: mean has %d scalars, weight %d" % (m.size, w.size))
            rc = self._L.ThalloX_PlanSetPrior(self.plan, int(input), m.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), int(w.size))
        if rc != 0:
            raise RuntimeError("ThalloX_PlanSetPrior failed: " + last_error())

    def prior_terms(self):
        """Scalars with a positive prior weight since the last init() (-1: there was none)."""
        return self._L.ThalloX_PlanPriorTerms(self.plan)

    def prior_cost(self):
        """The prior's share of the current cost, sum 1/2 w (x - mean)^2 (0.0 where no prior is in force)."""
        out = C.c_double(0.0)
        if self._L.ThalloX_PlanPriorCost(self.plan, C.byref(out)) != 0:
            raise RuntimeError("ThalloX_PlanPriorCost failed: " + last_error())
        return out.value

    ROBUST_LOSSES = {"trivial": 0, "huber": 1, "cauchy": 2}

    def set_robust_loss(self, kind, scale=1.0):
        """A robust loss over each observation's residual (include/Thallo.h ThalloX_PlanSetRobustLoss): kind "trivial" (the squared loss, the default), "huber" or
        "cauchy", scale in residual units (pixels); before init().  Raises, with the library's reason, where the plan cannot run one."""
        k = self.ROBUST_LOSSES.get(kind, kind)
        if not isinstance(k, int):
            raise ValueError("robust loss %r: one of %s" % (kind, sorted(self.ROBUST_LOSSES)))
        if self._L.ThalloX_PlanSetRobustLoss(self.plan, k, float(scale)) != 0:
            raise RuntimeError("ThalloX_PlanSetRobustLoss failed: " + last_error())

    def robust_weights(self):
        """rho'(s) per observation at the last linearisation, numpy float32 [O] in the caller's observation ids, values in (0, 1] (1 = the loss treats the observation as
        the squared loss does); raises when no loss is in force since the last init()."""
        import numpy as np
        out = np.empty(int(self._dims[2]), np.float32)      # (bundle_adjustment: dims = (cameras, points, observations); any other plan answers -1 below)
        if self._L.ThalloX_PlanRobustWeights(self.plan, out.ctypes.data_as(C.c_void_p), int(out.size)) != out.size:
            raise RuntimeError("ThalloX_PlanRobustWeights: no robust loss in force on this plan (or it has another number of observations)")
        return out

    def covariance(self, params, cameras=None, points=None, rel_tol=1e-6, max_iterations=500):
        """Marginal covariance blocks at the plan's current unknowns (include/Thallo.h ThalloX_PlanCovariance): `cameras` and `points` are sequences of the caller's ids
        (None: that kind is not asked for).  Returns {"cameras": float32 [n, 9, 9], "points": float32 [m, 3, 3], "info": {...}}: the blocks of (A_FF)^-1, A = J^T J without
        the LM diagonal, unscaled, zero rows and columns at held scalars, NaN blocks for points the elimination holds; info adds up iterations, columns, not_converged and
        nan_blocks over both kinds and keeps the largest worst_residual.  The gauge is the caller's to fix, with hold().  The plan's last init() must have run
        set_linear_solver("schur_explicit_pcg") (columns by PCG) or "schur_dense" (columns through the dense Cholesky factor: rel_tol and max_iterations are ignored,
        iterations and worst_residual are 0, not_converged counts the requested columns at scalars whose diagonal of S is not positive); raises, with the library's
        reason, where the call is refused."""
        import numpy as np
        out = {"cameras": np.zeros((0, 9, 9), np.float32), "points": np.zeros((0, 3, 3), np.float32),
               "info": {"iterations": 0, "columns": 0, "not_converged": 0, "nan_blocks": 0, "worst_residual": 0.0}}
        opt = CovarianceOptions(float(rel_tol), int(max_iterations))
        for key, input, ids, d in (("cameras", 0, cameras, 9), ("points", 1, points, 3)):
            if ids is None:
                continue
            ids = np.ascontiguousarray(np.asarray(ids).reshape(-1), np.int32)
            blocks = np.zeros((len(ids), d, d), np.float32)
            info = CovarianceInfo()
            rc = self._L.ThalloX_PlanCovariance(self.plan, params, input, ids.ctypes.data_as(C.c_void_p), len(ids), blocks.ctypes.data_as(C.c_void_p), C.byref(opt), C.byref(info))
            if rc < 0:
                raise RuntimeError("ThalloX_PlanCovariance failed: " + last_error())
            out[key] = blocks
            for k in ("iterations", "columns", "not_converged", "nan_blocks"):
                out["info"][k] += int(getattr(info, k))
            out["info"]["worst_residual"] = max(out["info"]["worst_residual"], float(info.worst_residual))
        return out

    def set_kernel_sampling(self, period):
        self._L.ThalloX_SetKernelSampling(self.plan, period)

    def reset_kernel_stats(self):
        self._L.ThalloX_ResetKernelStats(self.plan)

    def kernel_stats(self):
        out = {}
        i = 0
        while True:
            name = C.c_char_p(); launches = C.c_long(); samples = C.c_long(); total = C.c_double()
            if self._L.ThalloX_GetKernelStat(self.plan, i, C.byref(name), C.byref(launches), C.byref(samples), C.byref(total)):
                break
            ks = C.c_long(); kt = C.c_double()
            self._L.ThalloX_GetKernelStatOwn(self.plan, i, C.byref(ks), C.byref(kt))
            out[name.value.decode()] = {"launches": launches.value, "samples": samples.value, "total_ms": total.value,
                                        "mean_ms": total.value / samples.value if samples.value else None,
                                        "own_samples": ks.value, "own_mean_ms": kt.value / ks.value if ks.value else None}
            i += 1
        return out

    def alpha_beta_trace(self, cap=4096):
        buf = (C.c_float * (2 * cap))()
        n = self._L.ThalloX_GetAlphaBetaTrace(self.plan, C.addressof(buf), cap)
        n = min(n, cap)
        return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


def iw_fused_bytes_per_iter(L, every_iteration_delta=False, ring=False):
    """Bytes per pixel and PCG iteration the image_warping one-kernel schedule has to move, each array once, averaged over the L iterations of
    a GN step.  Round 4 (energy_image_warping_march_rc.hip, no A p plane): read r 12, p 12, cs 8, flags 1; write r 12, p 12 = 57, + the delta update the launch carries:
    none on odd iterations and two (read delta 12 + p_{k-2} 12, write delta 12 = 36) on even ones -- or, on the multi-GPU device-side transport, one (24) every
    iteration -- or (round 5, ring=True: one GPU, the default) none at all, the update being a launch of its own per ring of p planes; the FIRST iteration of a GN
    step runs the stored-plane kernel without its A p read: 69.  THALLO_MARCH=0 / 3 / 4 (tile kernel / stored-plane marching
    kernel, the A/B forms): 99."""
    if os.environ.get("THALLO_MARCH", "1")[:1] in ("0", "3", "4"):
        return 99.0
    if L < 1:
        return 0.0
    if ring:        # round 5: p_k goes into a ring of planes, no launch touches delta (thallo_hip_linear_update_n does, once per ring: not this kernel's bytes)
        return (69.0 + 57.0 * (L - 1)) / L
    if every_iteration_delta:
        return (69.0 + 81.0 * (L - 1)) / L
    odd, even = L // 2, (L - 1) // 2          # k = 1, 3, ...: no delta update; k = 2, 4, ...: two
    return (69.0 + 57.0 * odd + 93.0 * even) / L

