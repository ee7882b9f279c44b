"""Shared helper of the per-kernel tests (test_gpu_pcg_chain.py, test_gpu_transport_kernels.py, test_gpu_sparse_kernels.py, test_gpu_graph_kernels.py,
test_gpu_sfs_kernels.py, test_gpu_ba_kernels.py, test_gpu_iw_kernels.py, test_ba_reference.py, test_shim_references.py).

Four things live here:
  * shim(): the library with argtypes / restype declared once for every thallo_hip.h entry point those files call;
  * the documented summation order and the PCG scalars in numpy float32 (sum_partials, div32): alpha and beta are known BIT-EXACTLY in every test;
  * flat_grid() restated from csrc/pcg_kernels.hip, padded device vectors with a NaN canary behind them (DVec), the two input regimes;
  * one plain float64 numpy reference per kernel (ref_*), each written from the comment of its entry point in include/thallo_hip.h and the
    gauss_newton.t lines that comment cites.  tests/test_shim_references.py chains them into whole PCG / LM loops on the CPU before any kernel is
    compared with them.

No function here needs a device except shim() and DVec / dbuf (which take the torch module as an argument)."""
import ctypes as C

import numpy as np

F32 = np.float32
EPS = 2.0 ** -24                 # unit roundoff of float32 (round to nearest)
CANARY = 0x7FC0BEEF              # a quiet-NaN bit pattern: whoever reads it poisons its result, whoever overwrites it is caught bytewise
MAX_PARTIALS = 1024
MAX_UPDATE_TERMS = 32
BLOCK = 256


# ------------------------------------------------------------------ ctypes mirrors
from thallo_amd import api          # (structures only: the library itself is loaded by shim())


def _api():
    return api


class UnitsT(C.Structure):       # thallo_units_t
    _fields_ = [("units", C.c_void_p), ("src", C.c_void_p), ("n", C.c_int), ("nplanes", C.c_int), ("base", C.c_long * 8), ("len", C.c_int * 8)]


class UpdateTermsT(C.Structure):     # thallo_update_terms_t
    _fields_ = [("p", C.c_void_p * MAX_UPDATE_TERMS), ("alphaN", api.SumT * MAX_UPDATE_TERMS), ("alphaD", api.SumT * MAX_UPDATE_TERMS), ("count", C.c_int)]


class PrevT(C.Structure):            # thallo_prev_t
    _fields_ = [("alphaD_partials", C.c_void_p), ("s12_partials", C.c_void_p), ("count", C.c_int), ("alphaD_word", C.c_void_p), ("betaN_word", C.c_void_p)]


class FinT(C.Structure):             # thallo_fin_t
    _fields_ = [("alphaN", api.SumT), ("tickets", C.c_void_p), ("alphaD_word", C.c_void_p), ("betaN_word", C.c_void_p)]


IwIterT = api.IwIterT                # thallo_iw_iter_t: the one mirror of the block (thallo_amd/api.py); shim() checks it against thallo_hip_iw_iter_size()
IW_ITER_TILE, IW_ITER_MARCH, IW_ITER_MARCH_RC = api.IW_ITER_TILE, api.IW_ITER_MARCH, api.IW_ITER_MARCH_RC

NO_FIN = FinT(api.SumT(None, 0), None, None, None)
FIN_TICKET_WORDS = 528           # THALLO_HIP_FIN_TICKET_WORDS

_SHIM = None


def shim():
    """The library thallo_amd.lib() loaded, through a handle of this module's own: ctypes keeps argtypes per handle, so declaring them here cannot change how the
    older tests (which call some of the same entry points with hand-wrapped arguments) pass theirs.  Same shared object, same thread-local gate, same device."""
    global _SHIM
    if _SHIM is not None:
        return _SHIM
    import thallo_amd
    L = C.CDLL(thallo_amd.lib()._name)
    S, G = api.SumT, api.SegsT
    vp, lg, it, fl, db = C.c_void_p, C.c_long, C.c_int, C.c_float, C.c_double
    sig = {
        "vector_elems": [lg], "device_cu_count": [],
        "pcg_step2": [vp] * 4 + [lg, S, S, vp, vp],
        "pcg_step2_ranges": [vp] * 4 + [lg] * 4 + [S, S, vp, vp],
        "pcg_step2_full": [vp] * 7 + [lg, S, S, vp, vp, it, vp],
        "pcg_step2_full_zeta": [vp] * 7 + [lg, S, S, vp, vp, vp, it, fl, vp, vp],
        "pcg_step3": [vp, vp, lg, S, S, it, vp],
        "pcg_pupdate": [vp] * 4 + [lg, it, S, S, S, vp],
        "pcg_pupdate_ranges": [vp] * 4 + [lg] * 4 + [it, S, S, S, vp],
        "lm_finalize_diagonal": [vp] * 7 + [lg, fl, fl, fl, it, it, vp, vp],
        "lm_step1_finish": [vp, vp, vp, lg, vp, vp],
        "lm_step2_first_half": [vp, vp, lg, S, S, vp],
        "lm_step2_second_half": [vp] * 6 + [lg, vp, vp, vp],
        "pcg_init_finish": [vp] * 4 + [lg, it, vp, vp],
        "lm_set_gate": [vp], "lm_state_reset": [vp, vp], "lm_zeta": [S, it, fl, vp, vp],
        "dot": [vp, vp, lg, vp, vp],
        "linear_update": [vp, vp, vp, lg, S, S, vp],
        "linear_update2": [vp, vp, vp, S, S, vp, S, S, lg, vp],
        "linear_update_n": [vp, vp, UpdateTermsT, lg, it, vp],
        "finish_sum": [S, vp, vp], "finish_sum_gated": [S, vp, vp, vp], "alpha_beta": [S, S, S, vp, vp],
        "pcg_update": [vp] * 6 + [lg, it, S, S, S, vp],
        "pcg_scalars_finish": [vp, vp, it, S, vp, vp, vp],
        "pcg_update_fin": [vp] * 6 + [lg, S, vp, vp, it, vp, vp, vp],
        "pcg_update_lm": [vp] * 6 + [lg, it, S, S, S, vp, vp, vp],
        "pcg_update_lm_fin": [vp] * 6 + [lg, S, vp, vp, vp, it, vp, vp, vp, it, fl, it, it, vp],
        "lm_owed_delta": [vp, vp, vp, lg, vp, vp, it, vp, it, vp],
        "slab_pack": [vp, G, S, vp, vp],
        "slab_unpack": [vp, G, vp, G, vp, vp, lg, it, vp, vp],
        "slab_pack_iter": [vp, G, vp, vp, it, vp, vp],
        "slab_unpack_iter": [vp, G, vp, G, vp, vp, lg, it, S, vp, vp, vp],
        "block_sums": [vp] * 4 + [lg, vp, vp, vp],
        "shard_scalars": [vp, lg, it, vp, vp, it, S, vp, vp, vp],
        "range_unpack": [vp, G, vp, lg, lg, it, vp],
        "units_pack": [vp, UnitsT, S, vp, vp], "units_unpack": [vp, UnitsT, vp, lg, it, vp, vp],
        "units_pack_iter": [vp, UnitsT, vp, vp, it, vp, vp], "units_unpack_iter": [vp, UnitsT, vp, lg, it, S, vp, vp, vp],
        "csr_spmv": [it] + [vp] * 8,
        "ell_apply": [it, lg, it] + [vp] * 6,
        "dense_gemv": [lg, vp, vp, vp, vp],
        "jtj_scatter": [lg, it, vp, vp, vp, vp],
        "incidence_count": [vp, lg, it, C.POINTER(C.c_long), C.POINTER(C.c_int), lg, vp, vp, vp],      # slot_base / slot_ch: HOST arrays
        "incidence_fill": [vp, lg, it, C.POINTER(C.c_long), C.POINTER(C.c_int), lg, vp, vp, vp, vp],
        # the graph-edge domains (csrc/energy_graph.hip; test_gpu_graph_kernels.py)
        "lapgraph_cost": [it] + [vp] * 4 + [fl, vp, vp],
        "lapgraph_pcg_init": [it] + [vp] * 6 + [fl] + [vp] * 7,
        "lapgraph_apply_jtj": [it] + [vp] * 4 + [fl] + [vp] * 4,
        "arap_cost": [it] * 3 + [vp] * 6 + [fl, fl, vp, lg, vp],
        "arap_precompute": [it] + [vp] * 5 + [fl, vp, vp, lg, vp],
        "arap_precompute2": [it] + [vp] * 5 + [fl, vp, vp, vp, lg, vp],
        "arap_recompute_supported": [it, lg],
        "arap_pcg_init": [it] * 3 + [vp] * 7 + [fl, fl] + [vp] * 7 + [lg, vp],
        "arap_apply_jtj": [it] * 3 + [vp] * 7 + [fl, fl] + [vp] * 3 + [lg, vp],
        "arap_apply_jtj_sums": [it] * 3 + [vp] * 7 + [fl, fl] + [vp] * 3 + [lg] + [vp] * 4,
        "arap_apply_jtj_sums_fin": [it] * 3 + [vp] * 7 + [fl, fl] + [vp] * 3 + [lg] + [vp] * 3 + [FinT, vp],
        "arap_apply_jtj_rc": [it] * 3 + [vp] * 7 + [fl, fl] + [vp] * 3 + [lg] + [vp] * 3 + [FinT, vp],
        "arap_debug_set": [it, it],
        "permute3": [it, vp, vp, vp, it, vp],
        # shape_from_shading (csrc/energy_sfs.hip, energy_sfs_pair.hip; test_gpu_sfs_kernels.py): W, H, row0 / ra, row1 / rb, yoff, Hg, host_params first
        "sfs_precompute": [it] * 6 + [vp] * 10,
        "sfs_precompute_cost": [it] * 6 + [vp] * 9 + [it, it, vp, vp],
        "sfs_cost": [it] * 6 + [vp] * 8,
        "sfs_pcg_init": [it] * 6 + [vp] * 15,
        "sfs_pcg_init_lm": [it] * 6 + [vp] * 14 + [fl, fl, fl, it, vp, vp],
        "sfs_apply_jtj": [it] * 6 + [vp] * 10,
        "sfs_apply_jtj_gated": [it] * 6 + [vp] * 11,
        "sfs_apply_jtj_lm": [it] * 6 + [vp] * 12,
        "sfs_apply_jtj_sums": [it] * 6 + [vp] * 12,
        "sfs_apply_jtj_sums_fin": [it] * 6 + [vp] * 11 + [FinT, vp],
        "sfs_apply_jtj_lm_pupdate": [it] * 6 + [vp] * 10 + [it, S, S, vp, vp],
        "sfs_pcg_iter": [it] * 6 + [vp] * 11 + [it, S, S, S, vp, vp, FinT, vp],
        "sfs_pcg_iter_deferred": [it] * 6 + [vp] * 11 + [it, S, PrevT, vp, vp, vp],
        "sfs_pcg_iter_lm": [it] * 6 + [vp] * 14 + [it, S, S, S, vp, vp, vp, FinT, vp, it, fl, vp],
        "sfs_lm_model_cost": [it] * 6 + [vp] * 11 + [it, vp, it, vp, vp, vp, vp, vp],
        "sfs_march_debug_set": [it, it], "sfs_planes_layout": [it, it], "sfs_march_fits": [it], "sfs_lm_pupdate_supported": [],
        "checksum_i32": [lg, vp, vp, vp],
        # bundle adjustment (csrc/energy_ba.hip; test_gpu_ba_kernels.py): C, P first; the lists, cameras, points, JP, JpC = 8 pointers
        "ba_cost": [it] * 3 + [vp] * 7,
        "ba_compute_j": [it] + [vp] * 9, "ba_compute_j_ad": [it] + [vp] * 9, "ba_compute_j_robust": [it] + [vp] * 6 + [it, fl] + [vp] * 4,
        "ba_pcg_init": [it, it] + [vp] * 15,
        "ba_point_order": [it, vp, vp, vp], "ba_pack_point_blocks": [it, vp, vp, vp, vp],
        "ba_apply2_camera_slots": [it, it],
        "ba_apply_jtj2": [it, it] + [vp] * 8 + [vp] * 7 + [vp],
        "ba_apply_jtj2_fin": [it, it] + [vp] * 8 + [vp] * 7 + [FinT, vp],
        "ba_apply_jtj2_fin_robust": [it, it] + [vp] * 8 + [vp] * 7 + [FinT, vp, vp],
        "ba_apply_jtj2_lm": [it, it] + [vp] * 8 + [vp] * 5 + [vp],
        "ba_lm_reset_residual": [it, it] + [vp] * 8 + [vp] * 7 + [vp],
        "ba_pcg_apply_lm": [it, it] + [vp] * 8 + [vp] * 10 + [FinT, vp, it, fl, it, it, vp],
        # the image-stencil plugins (csrc/energy_image_warping*.hip, energy_laplacian_image.hip; test_gpu_iw_kernels.py): W, H (, row0, row1) first
        "iw_cost": [it] * 4 + [vp] * 5 + [fl, fl, vp, vp],
        "iw_pcg_init": [it] * 4 + [vp] * 5 + [fl, fl] + [vp] * 11,
        "iw_pcg_step1": [it] * 4 + [vp] * 3 + [fl, fl] + [vp] * 5 + [it] + [S] * 5 + [vp] * 4,
        "iw_pcg_step2": [it] * 4 + [vp, fl, fl] + [vp] * 4 + [S, S] + [vp] * 3,
        "iw_apply_jtj": [it] * 4 + [vp] * 3 + [fl, fl] + [vp] * 5,
        "iw_pcg_iter": [it, C.POINTER(api.IwIterT), vp], "iw_iter_size": [],
        "iw_pcg_iter_finish": [vp, vp, it, S, vp, vp, vp],
        "iw_urshape_irregular": [it, it, vp, vp, vp],
        "iw_march_rows": [it, it], "iw_march_place": [it] * 5 + [vp], "march_debug_set": [it, it],
        "iw_resident_rows": [it, it], "iw_resident_bytes": [it, it], "resident_debug_set": [it, it],
        "iw_pcg_resident": [it] * 4 + [vp, vp, fl, fl] + [vp] * 6 + [S] + [vp] * 5 + [it, vp],
        "iw_resident_status": [vp, it, it, vp, vp],
        "lapimg_cost": [it, it, vp, vp, fl, it, vp, vp],
        "lapimg_pcg_init": [it, it, vp, vp, fl, it] + [vp] * 7,
        "lapimg_apply_jtj": [it, it, fl, it] + [vp] * 4,
        "lapimg_pcg_step1": [it, it, fl, it] + [vp] * 5 + [it] + [S] * 3 + [vp, vp],
        # the double-precision PCG / LM kernels (csrc/pcg_kernels_f64.hip; test_gpu_f64_kernels.py): the vectors, n, the device words, the partials, the stream
        "f64_init_finish": [vp] * 4 + [lg, it, vp, vp], "f64_dot": [vp, vp, lg, vp, vp], "f64_step2": [vp] * 6 + [lg] + [vp] * 4,
        "f64_step3": [vp, vp, lg, vp, vp, vp], "f64_linear_update": [vp, vp, lg, vp], "f64_finish": [vp, it, vp, vp],
        "f64_lm_finalize_diagonal": [vp] * 7 + [lg, db, db, db, it, it, vp, vp], "f64_lm_step1_finish": [vp, vp, vp, lg, vp, vp],
        "f64_lm_step2": [vp] * 7 + [lg] + [vp] * 5, "f64_lm_step2_first_half": [vp, vp, lg, vp, vp, vp],
        "f64_lm_step2_second_half": [vp] * 6 + [lg, vp, vp, vp], "f64_lm_step3": [vp, vp, lg, vp, vp, vp],
    }
    for name, args in sig.items():
        f = getattr(L, "thallo_hip_" + name)
        f.argtypes = args
        f.restype = (None if name in ("lm_set_gate", "arap_debug_set", "sfs_march_debug_set", "march_debug_set", "resident_debug_set")
                     else lg if name in ("vector_elems", "iw_resident_bytes") else C.c_uint if name == "iw_iter_size" else it)
    assert L.thallo_hip_iw_iter_size() == C.sizeof(api.IwIterT), "thallo_iw_iter_t and its ctypes mirror differ"
    # the probe of a generated plugin (csrc/dsl_plugin.cpp; test_gpu_generated_kernels.py): name -> (argtypes, restype)
    cs = C.c_char_p
    for name, (args, res) in {"open": ([cs, C.POINTER(C.c_uint), it, it], vp), "close": ([vp], None), "n_unknowns": ([vp], lg), "schedule_name": ([vp], cs),
                              "use_preconditioner": ([vp], it), "whole_store": ([vp], it), "bind": ([vp, C.POINTER(vp)], it), "prepare": ([vp], it), "cost": ([vp, vp], it), "pcg_init": ([vp] * 8, it),
                              "apply_jtj": ([vp] * 4, it), "set_row_slab": ([vp, it, it], it), "set_slab_global": ([vp, it, it], it), "slab_ghost_rows": ([vp], it),
                              "kernels": ([vp, it], cs)}.items():
        f = getattr(L, "thallo_hip_genprobe_" + name)
        f.argtypes, f.restype = args, res
    _SHIM = L
    return L


INVALID = -1          # -hipErrorInvalidValue
NOT_SUPPORTED = -801  # -hipErrorNotSupported


def sumt(t, count=None):
    """thallo_sum_t over a device tensor (all of it, or its first `count` words)"""
    return _api().SumT(t.data_ptr(), int(t.numel() if count is None else count))


def segs(pieces):
    """thallo_segs_t from [(off, len), ...]"""
    g = _api().SegsT()
    for k, (o, l) in enumerate(pieces):
        g.off[k] = int(o); g.len[k] = int(l)
    g.n = len(pieces)
    return g


# ------------------------------------------------------------------ the documented summation order, in numpy float32
def _sum_partials_reference(part):
    """sum_partials() of csrc/device_common.hpp in numpy float32: lane l adds part[l], part[l+64], ... in index order, then the wave64
    butterfly v += shfl_xor(v, m) for m = 32, 16, ..., 1."""
    lanes = np.zeros(64, np.float32)
    for l in range(64):
        acc = np.float32(0.0)
        for x in part[l::64]:
            acc = np.float32(acc + x)
        lanes[l] = acc
    m = 32
    while m >= 1:
        lanes = (lanes + lanes[np.arange(64) ^ m]).astype(np.float32)
        m //= 2
    return lanes[0]


def sum_partials(part):
    """a thallo_sum_t as every consumer reads it (thallo_hip.h: count == 1 is a plain scalar word, taken as it is)"""
    part = np.asarray(part, F32)
    return F32(part[0]) if part.size == 1 else F32(_sum_partials_reference(part))


def sum_partials_f64(part):
    """the double sums N, S1, S2 (U, T1, T2) in the same order: lane-strided, then the butterfly"""
    part = np.asarray(part, np.float64)
    lanes = np.zeros(64, np.float64)
    for l in range(64):
        acc = np.float64(0.0)
        for x in part[l::64]:
            acc = acc + x
        lanes[l] = acc
    m = 32
    while m >= 1:
        lanes = lanes + lanes[np.arange(64) ^ m]
        m //= 2
    return lanes[0]


def div32(num, den, guard):
    """float32 num / den; guard: safeDivideIfNotLM (gauss_newton.t:226-234) -- 0 when den == 0; unguarded (LM): IEEE division, inf / nan included"""
    num, den = F32(num), F32(den)
    if guard and den == 0:
        return F32(0.0)
    with np.errstate(all="ignore"):
        return F32(num / den)


def beta_n_f64(N, S1, S2, alpha):
    """betaN_k = N - 2 alpha S1 + alpha^2 S2 in float64, clamped to 0 when <= 0 or NaN; returns (value, sum |terms|)"""
    a = float(alpha)
    with np.errstate(all="ignore"):
        bn = N - 2.0 * a * S1 + a * a * S2
        mag = abs(N) + abs(2.0 * a * S1) + abs(a * a * S2)
    if not bn > 0.0:
        bn = 0.0
    return bn, mag


def beta_n(N, S1, S2, alpha):
    """... from the double sums and the float32 alpha, as the float32 word the kernels leave; returns (word, sum |terms|)"""
    bn, mag = beta_n_f64(N, S1, S2, alpha)
    with np.errstate(over="ignore"):          # (1e300 -> inf is the conversion's answer)
        return F32(bn), mag


def ulp_apart(a, b):
    """distance of two finite float32 in units of the last place (0 = the same bits up to the sign of zero)"""
    def key(x):
        i = int(np.array(x, F32).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))


def tol(k, scale):
    """k roundings of relative size 2^-24 on quantities bounded by `scale`: k 2^-24 scale"""
    return k * EPS * np.asarray(scale, np.float64)


# ------------------------------------------------------------------ launch shapes
def flat_grid(n4, cus):
    """workgroups of a flat kernel over n4 float4 (csrc/pcg_kernels.hip): one per 256 float4, at most min(4 CUs, 1024) rounded down to a multiple of 8, at least 1"""
    want = (n4 + BLOCK - 1) // BLOCK
    cap = min(4 * cus, MAX_PARTIALS)
    if cap >= 8:
        cap -= cap % 8
    return int(max(1, min(want, cap)))


def ceil4(n):
    return (n + 3) // 4 * 4


def block_of(c4, grid):
    """workgroup that owns each float of a flat vector of c4 floats (float4 j belongs to workgroup (j // 256) % grid of the grid-stride loop)"""
    j = np.arange(c4 // 4)
    return np.repeat((j // BLOCK) % grid, 4)


def block_sums(terms, grid, blk=None):
    """float64 sum of `terms` per workgroup"""
    terms = np.asarray(terms, np.float64)
    blk = block_of(terms.size, grid) if blk is None else blk
    return np.bincount(blk, weights=terms, minlength=grid)


def chain_length(c4, grid):
    """longest chain of float additions behind one partial: the 4 elements of every float4 a lane visits (ceil(n4 / (256 grid)) visits), 6 butterfly levels, 4 waves"""
    n4 = c4 // 4
    return 4 * ((n4 + BLOCK * grid - 1) // (BLOCK * grid)) + 6 + 4


def assert_exact_sums(terms, grid, lsb, blk=None):
    """the exact regime's licence: every term is a multiple of lsb and every workgroup's sum of |terms| stays below 2^24 lsb -- float32 adds them exactly in any order"""
    terms = np.asarray(terms, np.float64)
    assert (terms / lsb == np.rint(terms / lsb)).all()
    assert block_sums(np.abs(terms), grid, blk).max() < 2 ** 24 * lsb


# ------------------------------------------------------------------ device buffers
class DVec:
    """A padded solver vector on the device: thallo_hip_vector_elems(n) + 256 floats; payload in [0, n), zeros in [n, ceil4(n)), the canary from ceil4(n) on.
    payload None: the canary everywhere (an output the kernel must fill -- or must not touch)."""

    def __init__(self, torch, n, payload=None, elems=None):
        self.n, self.c4 = n, ceil4(n)
        total = (elems if elems is not None else (n + 255) // 256 * 256) + 256
        h = np.full(total, CANARY, np.uint32).view(F32)
        if payload is not None:
            h[:n] = np.asarray(payload, F32); h[n:self.c4] = 0
        self.h0 = h.copy()
        self.t = torch.from_numpy(h).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        return self.t.cpu().numpy()

    def body(self):
        return self.get()[:self.c4]

    def canary_ok(self):
        return self.get()[self.c4:].tobytes() == self.h0[self.c4:].tobytes()

    def unchanged(self):
        return self.get().tobytes() == self.h0.tobytes()


def dbuf(torch, a):
    """a plain device buffer with the bytes of the numpy array `a`"""
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def canary_buf(torch, words, dtype=F32):
    """an output buffer of `words` elements of dtype, every 32-bit word the canary"""
    per = np.dtype(dtype).itemsize // 4
    return torch.from_numpy(np.full(words * per, CANARY, np.uint32).view(dtype).copy()).cuda()


def written_slots(buf_host):
    """number of leading elements that no longer hold the canary, asserting that nothing behind them was written (the partials buffer holds exactly `grid` slots)"""
    w = np.ascontiguousarray(buf_host).view(np.uint32).reshape(buf_host.shape[0], -1)
    dirty = (w != CANARY).any(axis=1)
    k = int(dirty.sum())
    assert dirty[:k].all() and not dirty[k:].any(), "written slots are not a prefix"
    return k


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ------------------------------------------------------------------ the two input regimes
def exact_vec(rng, n, amp=8):
    """exact regime: integers in [-amp, amp] (amp <= 8)"""
    return rng.integers(-amp, amp + 1, n).astype(F32)


def exact_pre(rng, n):
    return rng.choice(np.array([0.25, 0.5, 1.0, 2.0], F32), n)


def rounded_vec(rng, n):
    """rounded regime: standard_normal * 10^U{-3..3}"""
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)


def rounded_pre(rng, n):
    return rng.uniform(0.25, 2.0, n).astype(F32)


def exact_sum(rng, count, target):
    """`count` partials, multiples of 1/2 of small magnitude, that add up to `target` (a multiple of 1/2) exactly in any order"""
    p = rng.integers(-4, 5, count).astype(np.float64) * 0.5
    p[-1] += target - p.sum()
    p = p.astype(F32)
    assert float(sum_partials(p)) == target == float(p.astype(np.float64).sum())
    return p


def rounded_sum(rng, count, positive=False):
    p = rounded_vec(rng, count)
    return np.abs(p) if positive else p


# ------------------------------------------------------------------ float64 references, one per kernel
# Arguments are numpy arrays (any float type; promoted to float64) and the scalars alpha / beta as the kernel forms them (float32, from div32).
def _d(*xs):
    return [np.asarray(x, np.float64) for x in xs]


def ref_step2(r, Ap, pre, alpha):
    """thallo_hip_pcg_step2 (gauss_newton.t:801-843 without the delta update): r -= alpha Ap; z = pre r; betaN = sum z.r.  Returns r, z, the betaN terms."""
    r, Ap = _d(r, Ap); pre = 1.0 if pre is None else np.asarray(pre, np.float64)
    with np.errstate(all="ignore"):
        r1 = r - float(alpha) * Ap
        z = pre * r1
        return r1, z, z * r1


def ref_step2_full(delta, p, r, Ap, pre, b, alpha):
    """thallo_hip_pcg_step2_full (gauss_newton.t:801-843): delta += alpha p, then ref_step2, and with b the LM q terms 0.5 delta.(r + b) (:832-837).
    Returns delta, r, z, betaN terms, q terms (None without b)."""
    delta, p = _d(delta, p)
    with np.errstate(all="ignore"):
        d1 = delta + float(alpha) * p
        r1, z, bn = ref_step2(r, Ap, pre, alpha)
        q = None if b is None else 0.5 * d1 * (r1 + np.asarray(b, np.float64))
    return d1, r1, z, bn, q


def ref_step3(p, z, beta):
    """thallo_hip_pcg_step3 (gauss_newton.t:889-899): p = z + beta p"""
    p, z = _d(p, z)
    with np.errstate(all="ignore"):
        return z + float(beta) * p


def ref_pupdate(z, p_in, delta, alpha, beta, first):
    """thallo_hip_pcg_pupdate: delta += alpha p_in (not on the first iteration, not when delta is None); p_out = z + beta p_in (first: p_out = z).  Returns p_out, delta."""
    z, p_in = _d(z, p_in)
    if first:
        return z.copy(), None if delta is None else np.asarray(delta, np.float64).copy()
    with np.errstate(all="ignore"):
        d1 = None if delta is None else np.asarray(delta, np.float64) + float(alpha) * p_in
        return z + float(beta) * p_in, d1


def ref_pcg_update(r, Ap, pre, p_in, delta, alpha, beta, first):
    """thallo_hip_pcg_update(_lm): first == 0: r -= alpha Ap, delta += alpha p_in; always p_out = pre r + beta p_in (first == 1: beta = 0; first == 2, LM behind
    a residual reset: r and delta are already current).  Returns r, p_out, delta."""
    r, p_in = _d(r, p_in); pre = 1.0 if pre is None else np.asarray(pre, np.float64)
    d1 = None if delta is None else np.asarray(delta, np.float64).copy()
    with np.errstate(all="ignore"):
        if first == 0:
            r = r - float(alpha) * np.asarray(Ap, np.float64)
            d1 = d1 + float(alpha) * p_in
        b = 0.0 if first == 1 else float(beta)
        return r, pre * r + (b * p_in if first != 1 else 0.0), d1


def ref_scalars_finish(aD_partials, s3_partials, alphaN, guard=True):
    """thallo_hip_pcg_scalars_finish: alphaD = sum of the float partials (the documented order), N, S1, S2 = the double partials' sums (same order), alpha = alphaN / alphaD,
    betaN = N - 2 alpha S1 + alpha^2 S2 clamped at 0.  Returns alphaD (float32, bit-exact), alpha (float32, bit-exact), betaN (float32, to 1 ulp), sum |terms| of betaN."""
    s3 = np.asarray(s3_partials, np.float64).reshape(-1, 3)
    ad = sum_partials(aD_partials)
    alpha = div32(alphaN, ad, guard)
    bn, mag = beta_n(sum_partials_f64(s3[:, 0]), sum_partials_f64(s3[:, 1]), sum_partials_f64(s3[:, 2]), alpha)
    return ad, alpha, bn, mag


def guarded_invert(d):
    """guardedInvert, CERES flavour (gauss_newton.t:638-648): 1 / (1 + sqrt(d))^2"""
    d = np.asarray(d, np.float64)
    return 1.0 / (1.0 + np.sqrt(d)) ** 2


def ref_init_finish(r, diag, use_preconditioner):
    """thallo_hip_pcg_init_finish (gauss_newton.t:712-731): pre = guardedInvert(diag) or 1; z = pre r; alphaN terms r.z"""
    r, = _d(r)
    pre = guarded_invert(diag) if use_preconditioner else np.ones_like(r)
    z = pre * r
    return pre, z, r * z


def ref_lm_finalize(diag, SSq, r, radius, min_lm, max_lm, save_ssq, use_preconditioner):
    """thallo_hip_lm_finalize_diagonal (gauss_newton.t:929-969, thallo.t:3911-3937).  Returns SSq, CtC, pre, b, z, alphaN terms."""
    diag, r = _d(diag, r)
    radius = float(F32(radius)); min_lm = float(F32(min_lm)); max_lm = float(F32(max_lm))
    if save_ssq:
        SSq = guarded_invert(diag) if use_preconditioner else np.ones_like(diag)
    else:
        SSq = np.asarray(SSq, np.float64)
    unclamped = diag / radius
    cm = (1.0 / SSq) / radius
    CtC = np.minimum(np.maximum(unclamped, min_lm * cm), max_lm * cm)
    pre = 1.0 / (CtC + radius * unclamped)
    z = pre * r
    return SSq, CtC, pre, r.copy(), z, r * z


def ref_lm_step1_finish(Ap, CtC, p):
    """thallo_hip_lm_step1_finish (gauss_newton.t:777-787): Ap += CtC p; alphaD terms p.Ap"""
    Ap, CtC, p = _d(Ap, CtC, p)
    a = Ap + CtC * p
    return a, p * a


def ref_lm_step2_first(delta, p, alpha):
    """thallo_hip_lm_step2_first_half (gauss_newton.t:845-856): delta += alpha p"""
    delta, p = _d(delta, p)
    with np.errstate(all="ignore"):
        return delta + float(alpha) * p


def ref_lm_step2_second(b, Adelta, pre, delta):
    """thallo_hip_lm_step2_second_half (gauss_newton.t:858-886): r = b - A delta; z = pre r; betaN terms z.r; q terms 0.5 delta.(r + b)"""
    b, Adelta, pre, delta = _d(b, Adelta, pre, delta)
    r = b - Adelta
    z = pre * r
    return r, z, z * r, 0.5 * delta * (r + b)


def ref_lm_zeta(state, Q1, k, q_tolerance):
    """thallo_hip_lm_zeta (gauss_newton.t:1666-1686) on the state words [Q0, frozen, iterations]: returns the new (Q0, frozen, iterations).  Frozen already: unchanged.
    Stop when Q1 or zeta = (k + 1)(Q1 - Q0) / Q1 is not finite (0 / 0 included) or zeta < q_tolerance."""
    Q0, frozen, its = state
    if frozen:
        return state
    Q1 = float(Q1)
    with np.errstate(all="ignore"):
        zeta = np.float64(k + 1) * (np.float64(Q1) - np.float64(Q0)) / np.float64(Q1)
    if not np.isfinite(Q1) or not np.isfinite(zeta) or zeta < float(F32(q_tolerance)):
        return (Q0, 1, k + 1)
    return (Q1, 0, its)


def ref_linear_update_n(X, delta, ps, alphas):
    """thallo_hip_linear_update / update2 / update_n (gauss_newton.t:901-906): delta += alpha_0 p_0, += alpha_1 p_1, ...; X given: X += that, delta itself stays.
    Returns (X or None, delta)."""
    d, = _d(delta)
    d = d.copy()
    for p, a in zip(ps, alphas):
        d = d + float(a) * np.asarray(p, np.float64)
    if X is None:
        return None, d
    return np.asarray(X, np.float64) + d, np.asarray(delta, np.float64)


def ref_block_sums(p, Ap, r, pre):
    """thallo_hip_block_sums: terms of alphaD = p.Ap and of N = r.M^-1.r, S1 = r.M^-1.Ap, S2 = Ap.M^-1.Ap"""
    p, Ap, r = _d(p, Ap, r); m = 1.0 if pre is None else np.asarray(pre, np.float64)
    return p * Ap, m * r * r, m * r * Ap, m * Ap * Ap


def hi_lo_words(x):
    """a double as the two float words (hi, lo) that carry its bits through a float message"""
    b = np.array([x], np.float64).view(np.uint64)[0]
    return np.array([b >> np.uint64(32), b & np.uint64(0xFFFFFFFF)], np.uint64).astype(np.uint32).view(F32)


def from_hi_lo(hi, lo):
    b = (np.uint64(np.array(hi, F32).view(np.uint32)) << np.uint64(32)) | np.uint64(np.array(lo, F32).view(np.uint32))
    return np.array([b], np.uint64).view(np.float64)[0]


def ref_rank_scalars(gathered, stride, world, alphaN, extra_ad=None, extra_s3=None):
    """thallo_hip_slab_unpack_iter / units_unpack_iter / shard_scalars: alphaD = the ranks' word 0 added in rank order by a sequential float32 loop (+ the shared block's
    float partials in the documented order), N, S1, S2 = the ranks' (hi, lo) doubles added in rank order (+ the shared block's double sums), alpha = alphaN / alphaD guarded,
    betaN as ref_scalars_finish.  Returns alphaD (bit-exact), betaN (1 ulp), sum |terms|."""
    g = np.asarray(gathered, F32)
    ad = F32(0.0); q = [0.0, 0.0, 0.0]
    with np.errstate(all="ignore"):
        for r in range(world):
            m = g[r * stride:]
            ad = F32(ad + m[0])
            for j in range(3):
                q[j] = q[j] + from_hi_lo(m[1 + 2 * j], m[2 + 2 * j])
        if extra_ad is not None:
            ad = F32(ad + sum_partials(extra_ad))
        if extra_s3 is not None:
            s3 = np.asarray(extra_s3, np.float64).reshape(-1, 3)
            q = [q[j] + sum_partials_f64(s3[:, j]) for j in range(3)]
    alpha = div32(alphaN, ad, True)
    bn, mag = beta_n(q[0], q[1], q[2], alpha)
    return ad, bn, mag
