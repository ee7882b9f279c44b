// held.hip -- unknowns the caller holds fixed (ThalloX_PlanSetHeldUnknowns; DESIGN.md "Held unknowns").  The solve is that of the problem in which the held scalars
// are constants, A_FF delta_F = b_F on the free set F.  One rule carries it through every PCG loop: every product with M^-1 or Cp^-1 has a zero row and column at a held
// scalar.  Then z, p and delta stay zero there, the loop's scalars see F only, and PCG runs on A_FF.  Nothing here runs inside a PCG iteration: a few launches per step.
//
//   hold_pcg           point Jacobi: pre = z = 0 at held scalars, the partials of r . z formed anew over the flat vector (behind PCGInit1 / PCGFinalizeDiagonal)
//   block_hold         H: a held scalar's row and column of its block become those of the identity (in front of the factor launches)
//   block_hold_factor  G: that row and column become zero (behind them): G^T G is the inverse of the block's free principal sub-block, bordered by zeros
//
// mask: one byte per scalar of the flat vector in the plan's internal ids, nonzero = held.  One lane per scalar (hold_pcg) or per block, consecutive lanes on consecutive
// words; every loop over a block is unrolled (no scratch); one partial per workgroup in a fixed order, no float atomics.
#include "device_common.hpp"
#include "block_regions.hpp"
#include "../../include/thallo_hip.h"

using namespace thallo;
using thallo::launch::check_launch;

namespace {

constexpr int BLOCK = 256;
inline int grid_for(long items)
{
    long g = (items + BLOCK - 1) / BLOCK;
    if (g > THALLO_MAX_PARTIALS) g = THALLO_MAX_PARTIALS;
    return g < 1 ? 1 : (int)g;
}

__global__ __launch_bounds__(BLOCK) void k_hold_pcg(const unsigned char* __restrict__ mask, const float* __restrict__ r, float* __restrict__ pre, float* __restrict__ z, long n,
                                                    float* __restrict__ rz_out)
{
    __shared__ float red[16];
    float acc = 0.0f;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * BLOCK) {
        float zv = z[i];
        if (mask[i]) { zv = 0.0f; pre[i] = 0.0f; z[i] = 0.0f; }
        acc += r[i] * zv;
    }
    block_store_partial(acc, rz_out, red);
}

template <int N> __device__ __forceinline__ void load_mask(const unsigned char* __restrict__ mask, const Where& w, bool (&m)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) m[i] = mask[w.first + (long)N * w.b + i] != 0;
}
// the entries of a held scalar's row and column of the packed lower triangle become `diag` on the diagonal and zero elsewhere; the others are not touched
template <int N> __device__ __forceinline__ void hold_one(const Where& w, const unsigned char* __restrict__ mask, float* __restrict__ T, float diag)
{
    bool m[N];
    load_mask<N>(mask, w, m);
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j)
            if (m[i] || m[j]) T[w.base + (long)tri(i, j) * w.count + w.b] = i == j ? diag : 0.0f;
}
__global__ __launch_bounds__(BLOCK) void k_block_hold(thallo_block_regions_t R, long total, const unsigned char* __restrict__ mask, float* __restrict__ T, float diag)
{
    for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (long)gridDim.x * BLOCK) {
        const Where w = locate(R, t);
        if (w.size == 9) hold_one<9>(w, mask, T, diag); else hold_one<3>(w, mask, T, diag);
    }
}

int block_hold(thallo_block_regions_t regions, const unsigned char* mask, float* T, float diag, thallo_stream_t stream)
{
    if (!regions_ok(regions) || !mask || !T) return -(int)hipErrorInvalidValue;
    const long total = regions_blocks(regions);
    if (total < 1) return 0;
    hipLaunchKernelGGL(k_block_hold, dim3(grid_for(total)), dim3(BLOCK), 0, (hipStream_t)stream, regions, total, mask, T, diag);
    return check_launch();
}

}  // namespace

extern "C" {

int thallo_hip_hold_pcg(const unsigned char* mask, const float* r, float* pre, float* z, long n, float* rz_out, thallo_stream_t stream)
{
    if (!mask || !r || !pre || !z || !rz_out || n < 1) return -(int)hipErrorInvalidValue;
    const int grid = grid_for(n);
    hipLaunchKernelGGL(k_hold_pcg, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, mask, r, pre, z, n, rz_out);
    int e = check_launch(); return e ? e : grid;
}

int thallo_hip_block_hold(thallo_block_regions_t regions, const unsigned char* mask, float* H, thallo_stream_t stream) { return block_hold(regions, mask, H, 1.0f, stream); }

int thallo_hip_block_hold_factor(thallo_block_regions_t regions, const unsigned char* mask, float* G, thallo_stream_t stream) { return block_hold(regions, mask, G, 0.0f, stream); }

}  // extern "C"
