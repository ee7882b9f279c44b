// prior.hip -- Gaussian priors on single unknowns (ThalloX_PlanSetPrior; DESIGN.md "Gaussian priors").  The solve is that of the energy with one more residual,
// sqrt(w_i) (x_i - mu_i), per scalar with w_i > 0: cost += 1/2 w (x - mu)^2, b = -J^T F - W (x - mu), A = J^T J + W.  W reaches every product with A as the flat
// diagonal the applies, the factors and the assembly already take (the LM CtC's argument); what is not a matrix is formed here.  Nothing here runs inside a PCG
// iteration: two or three launches per step, one per cost evaluation.
//
//   prior_cost      the partials of 1/2 sum w (x - mu)^2, stored or added onto the cost kernel's partials in their slot (the slot keeps its count and its one reader)
//   prior_init      behind PCGInit1: r -= w (x - mu), diag += w, pre = the guarded inverse of diag, z = pre r, the partials of r . z formed anew over the flat vector
//   prior_lm_shift  behind PCGFinalizeDiagonal: shift = float32(CtC + w), the plane LM hands to every ctc / shift argument
//
// w, mu: one float per scalar of the flat vector in the plan's internal ids, w = 0: no prior there.  The unknowns live in two arrays (x0: the first n0 scalars, x1: the
// rest).  One lane per scalar, consecutive lanes on consecutive words; one partial per workgroup in a fixed order, no float atomics.
#include "device_common.hpp"
#include "../../include/thallo_hip.h"

using namespace thallo;
using thallo::launch::check_launch;

namespace {

constexpr int BLOCK = 256;
inline int grid_for(long items, long cap)
{
    long g = (items + BLOCK - 1) / BLOCK;
    if (g > cap) g = cap;
    return g < 1 ? 1 : (int)g;
}

__device__ __forceinline__ float unknown_at(const float* __restrict__ x0, const float* __restrict__ x1, long n0, long i) { return i < n0 ? x0[i] : x1[i - n0]; }

template <bool ONTO>
__global__ __launch_bounds__(BLOCK) void k_prior_cost(const float* __restrict__ w, const float* __restrict__ mu, const float* __restrict__ x0, const float* __restrict__ x1, long n0,
                                                      long n, float* __restrict__ out)
{
    __shared__ float red[16];
    float acc = 0.0f;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
        const float wi = w[i];
        if (wi > 0.0f) { const float d = unknown_at(x0, x1, n0, i) - mu[i]; acc += 0.5f * wi * (d * d); }      // (mu is not read where w = 0: it may hold anything there)
    }
    // block_store_partial's sum; ONTO: added onto the partial an earlier launch of the stream left in this workgroup's place (one writer per word: no atomics)
    const int lane = threadIdx.x & (THALLO_WAVE - 1), wave = threadIdx.x / THALLO_WAVE;
    const float s = wave_sum_all(acc);
    if (lane == 0) red[wave] = s;
    lds_barrier();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int k = 0; k < BLOCK / THALLO_WAVE; ++k) t += red[k];
        out[blockIdx.x] = ONTO ? out[blockIdx.x] + t : t;
    }
}

__global__ __launch_bounds__(BLOCK) void k_prior_init(const float* __restrict__ w, const float* __restrict__ mu, const float* __restrict__ x0, const float* __restrict__ x1, long n0,
                                                      long n, float* __restrict__ r, float* __restrict__ diag, float* __restrict__ pre, float* __restrict__ z, int use_precond,
                                                      float* __restrict__ rz_out)
{
    __shared__ float red[16];
    float acc = 0.0f;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
        const float wi = w[i];
        float rv = r[i], zv;
        if (wi > 0.0f) {
            const float d = unknown_at(x0, x1, n0, i) - mu[i];
            rv -= wi * d;
            const float dv = diag[i] + wi;
            const float m = use_precond ? guarded_invert(dv) : 1.0f;
            zv = m * rv;
            r[i] = rv; diag[i] = dv; pre[i] = m; z[i] = zv;
        } else zv = z[i];      // (PCGInit1's own pre r: nothing of this scalar changes)
        acc += rv * zv;
    }
    block_store_partial(acc, rz_out, red);
}

__global__ __launch_bounds__(BLOCK) void k_prior_lm_shift(const float* __restrict__ w, const float* __restrict__ ctc, long n, float* __restrict__ shift)
{
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) shift[i] = ctc[i] + w[i];
}

}  // namespace

extern "C" {

int thallo_hip_prior_cost(const float* w, const float* mu, const float* x0, const float* x1, long n0, long n, float* out, int onto, thallo_stream_t stream)
{
    if (!w || !mu || !x0 || !out || n < 1 || n0 < 0 || n0 > n || (n0 < n && !x1) || onto < 0 || onto > THALLO_MAX_PARTIALS) return -(int)hipErrorInvalidValue;
    const int grid = grid_for(n, onto > 0 && onto < THALLO_HIP_PRIOR_COST_PARTIALS ? onto : THALLO_HIP_PRIOR_COST_PARTIALS);
    if (onto > 0) hipLaunchKernelGGL(k_prior_cost<true>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, w, mu, x0, x1, n0, n, out);
    else hipLaunchKernelGGL(k_prior_cost<false>, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, w, mu, x0, x1, n0, n, out);
    int e = check_launch(); return e ? e : onto > 0 ? onto : grid;
}

int thallo_hip_prior_init(const float* w, const float* mu, const float* x0, const float* x1, long n0, long n, float* r, float* diag, float* pre, float* z, int use_preconditioner,
                          float* rz_out, thallo_stream_t stream)
{
    if (!w || !mu || !x0 || !r || !diag || !pre || !z || !rz_out || n < 1 || n0 < 0 || n0 > n || (n0 < n && !x1)) return -(int)hipErrorInvalidValue;
    const int grid = grid_for(n, THALLO_MAX_PARTIALS);
    hipLaunchKernelGGL(k_prior_init, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, w, mu, x0, x1, n0, n, r, diag, pre, z, use_preconditioner, rz_out);
    int e = check_launch(); return e ? e : grid;
}

int thallo_hip_prior_lm_shift(const float* w, const float* ctc, long n, float* shift, thallo_stream_t stream)
{
    if (!w || !ctc || !shift || n < 1) return -(int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_prior_lm_shift, dim3(grid_for(n, THALLO_MAX_PARTIALS)), dim3(BLOCK), 0, (hipStream_t)stream, w, ctc, n, shift);
    return check_launch();
}

}  // extern "C"
