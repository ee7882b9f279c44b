// block_precond.hip -- the opt-in block-Jacobi preconditioner (DESIGN.md "Block-Jacobi preconditioner"): one dense block of J^T J per group of unknowns
// that belongs together -- bundle adjustment: 9 x 9 per camera, 3 x 3 per point -- instead of the reference's point Jacobi (guardedInvert(diag J^T J) in GN,
// 1 / (CtC + diag) in LM; gauss_newton.t:638-648, 929-969).
//
//   block_diag    H  = the lower triangles of the blocks of J^T J, once per GN / LM step, from what precomputeJ wrote          (bundle adjustment's: k_ba_block_diag)
//   block_factor  B  = H + diag(shift);  s_i = 1 / sqrt(B_ii);  L L^T = S B S (Cholesky);  G = L^-1 S, lower triangular, packed          (the factor and its apply: block_chol.hpp)
//   block_apply   z  = G^T (G r)  (= B^-1 r), partials of r . z
//   block_step2   the GN PCGStep2 with that z;  block_step2_lm  the LM PCGStep2 (delta, r, z, betaN, q)
//
// Why G^T G and not a stored inverse: M^-1 = G^T G is symmetric positive definite however G is rounded, which PCG needs; an explicitly rounded B^-1 is
// symmetric at best.  Why the scaling: the camera blocks mix rotation, translation, focal length and distortion columns (condition number up to 8e7, marginal
// in float32); S B S has a unit diagonal and a condition number <= 1.3e3 on the same blocks.
//
// Storage: a REGION is {offset of its first unknown in the flat vector, block size n (3 or 9), block count}.  H and G hold the regions one after the other, each
// as n (n + 1) / 2 planes of `count` floats: entry (i, j), j <= i, of block b at  region_base + (i (i + 1) / 2 + j) * count + b  -- one lane handles one block,
// so consecutive lanes read consecutive words.  Nothing is indexed dynamically: every loop over a block is unrolled, a block lives in registers.
//
// Reductions as everywhere (device_common.hpp): one partial per workgroup, fixed order, no float atomics; bitwise reproducible for a launch shape.
#include "device_common.hpp"
#include "block_regions.hpp"      // tri, regions_ok, locate: shared with held.hip
#include "block_chol.hpp"         // factor, apply_g: shared with ba_schur.hip
#include "ba_blocks.hpp"          // bundle adjustment's blocks and launch shapes (k_ba_block_diag)
#include "../../include/thallo_hip.h"

using namespace thallo;
using thallo::launch::check_launch;

namespace {

constexpr int BLOCK = 256;

inline int block_grid(long blocks)
{
    long g = (blocks + BLOCK - 1) / BLOCK;
    if (g > THALLO_MAX_PARTIALS) g = THALLO_MAX_PARTIALS;
    return g < 1 ? 1 : (int)g;
}

template <int N> __device__ __forceinline__ void load_tri(const float* __restrict__ src, const Where& w, float (&a)[tri_n(N)])
{
#pragma unroll
    for (int k = 0; k < tri_n(N); ++k) a[k] = src[w.base + (long)k * w.count + w.b];
}
template <int N> __device__ __forceinline__ void load_vec(const float* __restrict__ v, const Where& w, float (&x)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = v[w.first + (long)N * w.b + i];
}
template <int N> __device__ __forceinline__ void store_vec(float* __restrict__ v, const Where& w, const float (&x)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) v[w.first + (long)N * w.b + i] = x[i];
}

template <int N> __device__ __forceinline__ bool factor_one(const Where& w, const float* __restrict__ H, const float* __restrict__ shift, const float* __restrict__ pre,
                                                            float* __restrict__ G)
{
    float a[tri_n(N)], sh[N];
    load_tri<N>(H, w, a);
#pragma unroll
    for (int i = 0; i < N; ++i) sh[i] = shift ? shift[w.first + (long)N * w.b + i] : 0.0f;
    const bool ok = factor<N>(a, sh);
    if (!ok) {      // the preconditioner's failure rule: G = diag(sqrt(pre)): G^T G r = pre . r, the point-Jacobi preconditioner the plan already holds
#pragma unroll
        for (int k = 0; k < tri_n(N); ++k) a[k] = 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) a[tri(i, i)] = sqrtf(pre[w.first + (long)N * w.b + i]);
    }
#pragma unroll
    for (int k = 0; k < tri_n(N); ++k) G[w.base + (long)k * w.count + w.b] = a[k];
    return ok;
}

__global__ __launch_bounds__(BLOCK) void k_block_factor(thallo_block_regions_t R, long total, const float* __restrict__ H, const float* __restrict__ shift,
                                                        const float* __restrict__ pre, float* __restrict__ G, unsigned* __restrict__ status)
{
    __shared__ unsigned cnt[BLOCK / THALLO_WAVE];
    unsigned bad = 0;
    for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (long)gridDim.x * BLOCK) {
        const Where w = locate(R, t);
        const bool ok = w.size == 9 ? factor_one<9>(w, H, shift, pre, G) : factor_one<3>(w, H, shift, pre, G);
        bad += ok ? 0u : 1u;
    }
    // an integer count: the order of the additions does not show in the result
    const int lane = threadIdx.x & (THALLO_WAVE - 1), wave = threadIdx.x / THALLO_WAVE;
    unsigned wsum = bad;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) wsum += (unsigned)__shfl_xor((int)wsum, m, THALLO_WAVE);
    if (lane == 0) cnt[wave] = wsum;
    lds_barrier();
    if (threadIdx.x == 0) {
        unsigned s = 0;
        for (int k = 0; k < BLOCK / THALLO_WAVE; ++k) s += cnt[k];
        if (s) atomicAdd(status, s);
    }
}

template <int N> __device__ __forceinline__ float apply_one(const Where& w, const float* __restrict__ G, const float* __restrict__ r, float* __restrict__ z)
{
    float g[tri_n(N)], rv[N], zv[N];
    load_tri<N>(G, w, g); load_vec<N>(r, w, rv);
    apply_g<N>(g, rv, zv);
    store_vec<N>(z, w, zv);
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) acc += rv[i] * zv[i];
    return acc;
}
__global__ __launch_bounds__(BLOCK) void k_block_apply(thallo_block_regions_t R, long total, const float* __restrict__ G, const float* __restrict__ r, float* __restrict__ z,
                                                       float* __restrict__ rz_out, const unsigned* __restrict__ gate)
{
    __shared__ float red[16];
    if (gate != nullptr && __builtin_amdgcn_readfirstlane((int)gate[0]) != 0) return;      // LM: the PCG loop already ended on the device
    float acc = 0.0f;
    for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (long)gridDim.x * BLOCK) {
        const Where w = locate(R, t);
        acc += w.size == 9 ? apply_one<9>(w, G, r, z) : apply_one<3>(w, G, r, z);
    }
    block_store_partial(acc, rz_out, red);
}

// GN PCGStep2 (gauss_newton.t:801-843 minus the delta update, as thallo_hip_pcg_step2): r -= alpha A p; z = G^T (G r); betaN partials
template <int N> __device__ __forceinline__ float step2_one(const Where& w, const float* __restrict__ G, float* __restrict__ r, const float* __restrict__ Ap, float* __restrict__ z,
                                                            float alpha)
{
    float g[tri_n(N)], rv[N], av[N], zv[N];
    load_tri<N>(G, w, g); load_vec<N>(r, w, rv); load_vec<N>(Ap, w, av);
#pragma unroll
    for (int i = 0; i < N; ++i) rv[i] -= alpha * av[i];
    apply_g<N>(g, rv, zv);
    store_vec<N>(r, w, rv); store_vec<N>(z, w, zv);
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) acc += zv[i] * rv[i];
    return acc;
}
__global__ __launch_bounds__(BLOCK) void k_block_step2(thallo_block_regions_t R, long total, const float* __restrict__ G, float* __restrict__ r, const float* __restrict__ Ap,
                                                       float* __restrict__ z, thallo_sum_t aN, thallo_sum_t aD, float* __restrict__ bN_out)
{
    __shared__ float red[16];
    const float alpha = safe_div<false>(sum_partials(aN.partials, aN.count), sum_partials(aD.partials, aD.count));
    float acc = 0.0f;
    for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (long)gridDim.x * BLOCK) {
        const Where w = locate(R, t);
        acc += w.size == 9 ? step2_one<9>(w, G, r, Ap, z, alpha) : step2_one<3>(w, G, r, Ap, z, alpha);
    }
    block_store_partial(acc, bN_out, red);
}

// LM PCGStep2 (gauss_newton.t:801-843 with the UsesLambda() lines, as thallo_hip_pcg_step2_full with lm = 1): delta += alpha p; r -= alpha A p; z; betaN; q = 0.5 delta . (r + b)
template <int N> __device__ __forceinline__ void step2_lm_one(const Where& w, const float* __restrict__ G, float* __restrict__ delta, const float* __restrict__ p, float* __restrict__ r,
                                                              const float* __restrict__ Ap, float* __restrict__ z, const float* __restrict__ b, float alpha, float (&acc)[2])
{
    float g[tri_n(N)], dv[N], pv[N], rv[N], av[N], bv[N], zv[N];
    load_tri<N>(G, w, g); load_vec<N>(delta, w, dv); load_vec<N>(p, w, pv); load_vec<N>(r, w, rv); load_vec<N>(Ap, w, av); load_vec<N>(b, w, bv);
#pragma unroll
    for (int i = 0; i < N; ++i) { dv[i] += alpha * pv[i]; rv[i] -= alpha * av[i]; }
    apply_g<N>(g, rv, zv);
    store_vec<N>(delta, w, dv); store_vec<N>(r, w, rv); store_vec<N>(z, w, zv);
#pragma unroll
    for (int i = 0; i < N; ++i) { acc[0] += zv[i] * rv[i]; acc[1] += 0.5f * (dv[i] * (rv[i] + bv[i])); }
}
__global__ __launch_bounds__(BLOCK) void k_block_step2_lm(thallo_block_regions_t R, long total, const float* __restrict__ G, float* __restrict__ delta, const float* __restrict__ p,
                                                          float* __restrict__ r, const float* __restrict__ Ap, float* __restrict__ z, const float* __restrict__ b,
                                                          thallo_sum_t aN, thallo_sum_t aD, float* __restrict__ bN_out, float* __restrict__ q_out, const unsigned* __restrict__ gate)
{
    __shared__ float red[32];
    if (gate != nullptr && __builtin_amdgcn_readfirstlane((int)gate[0]) != 0) return;      // LM: the PCG loop already ended on the device
    const float alpha = safe_div<true>(sum_partials(aN.partials, aN.count), sum_partials(aD.partials, aD.count));
    float acc[2] = { 0.0f, 0.0f };
    for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (long)gridDim.x * BLOCK) {
        const Where w = locate(R, t);
        if (w.size == 9) step2_lm_one<9>(w, G, delta, p, r, Ap, z, b, alpha, acc); else step2_lm_one<3>(w, G, delta, p, r, Ap, z, b, alpha, acc);
    }
    float* __restrict__ const outs[2] = { bN_out, q_out };
    block_store_partials<2>(acc, outs, red);
}

// ------------------------------------------------------------------------------------------ bundle adjustment's blocks
// Workgroups [0, cam_blocks): one wave per camera, lanes striding its observations (as energy_ba.hip k_gather<0> does for the nine diagonal sums: the diagonal entries
// here are the same sums in the same order), 45 sums of J_c^T J_c over both residual rows from the 96-byte blocks Jb; the rest: one thread per point over its packed
// point blocks JP (contiguous per point), 6 sums.  The two layouts and the launch shape: ba_blocks.hpp.
__global__ __launch_bounds__(BLOCK) void k_ba_block_diag(int C_, int P_, int cam_blocks, const int* __restrict__ cam_ptr, const int* __restrict__ pt_ptr,
                                                         const float4* __restrict__ Jb, const float2* __restrict__ JP, float* __restrict__ H)
{
    if ((int)blockIdx.x < cam_blocks) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int c = blockIdx.x * 4 + wave; c < C_; c += cam_blocks * 4) {
            float s[45];
#pragma unroll
            for (int k = 0; k < 45; ++k) s[k] = 0.0f;
            for (int q = cam_ptr[c] + lane; q < cam_ptr[c + 1]; q += 64) {
                float r0[9], r1[9];
                rows_of(ld_cam_rows(Jb, q), r0, r1);
#pragma unroll
                for (int i = 0; i < 9; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j) s[tri(i, j)] += r0[i] * r0[j] + r1[i] * r1[j];
            }
#pragma unroll
            for (int k = 0; k < 45; ++k) s[k] = wave_sum_all(s[k]);
            if (lane < 45) {
                float v = 0.0f;      // element `lane` without dynamic register indexing
#pragma unroll
                for (int k = 0; k < 45; ++k) if (lane == k) v = s[k];
                H[(long)lane * C_ + c] = v;
            }
        }
    } else {
        const int nb = gridDim.x - cam_blocks;
        float* Hp = H + 45L * C_;
        for (int j = (blockIdx.x - cam_blocks) * BLOCK + threadIdx.x; j < P_; j += nb * BLOCK) {
            float s[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
            for (int k = pt_ptr[j]; k < pt_ptr[j + 1]; ++k) {
                float r0[3], r1[3];
                rows_of(ld_pt_rows(JP, k), r0, r1);
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int jj = 0; jj <= i; ++jj) s[tri(i, jj)] += r0[i] * r0[jj] + r1[i] * r1[jj];
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) Hp[(long)k * P_ + j] = s[k];
        }
    }
}

}  // namespace

extern "C" {

long thallo_hip_block_floats(thallo_block_regions_t regions)
{
    if (!regions_ok(regions)) return -1;
    long t = 0;
    for (int i = 0; i < regions.n; ++i) t += (long)tri_n(regions.r[i].size) * regions.r[i].count;
    return t;
}

int thallo_hip_ba_block_diag(int C_, int P_, const int* cam_ptr, const int* pt_ptr, const float* Jb, const float* JP, float* H, thallo_stream_t stream)
{
    if (C_ < 0 || P_ < 0 || C_ + P_ < 1 || !cam_ptr || !pt_ptr || !Jb || !JP || !H) return -(int)hipErrorInvalidValue;
    int cb, grid; gather_shape(C_, P_, cb, grid);
    hipLaunchKernelGGL(k_ba_block_diag, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, C_, P_, cb, cam_ptr, pt_ptr, (const float4*)Jb, (const float2*)JP, H);
    return check_launch();
}

int thallo_hip_block_factor(thallo_block_regions_t regions, const float* H, const float* shift, const float* pre, float* G, unsigned* status, thallo_stream_t stream)
{
    if (!regions_ok(regions) || !H || !pre || !G || !status) return -(int)hipErrorInvalidValue;
    const long total = regions_blocks(regions);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t me = hipMemsetAsync(status, 0, sizeof(unsigned), s);
    if (me != hipSuccess) return -(int)me;
    if (total < 1) return 0;
    hipLaunchKernelGGL(k_block_factor, dim3(block_grid(total)), dim3(BLOCK), 0, s, regions, total, H, shift, pre, G, status);
    return check_launch();
}

int thallo_hip_block_apply(thallo_block_regions_t regions, const float* G, const float* r, float* z, float* rz_out, const unsigned* gate, thallo_stream_t stream)
{
    if (!regions_ok(regions) || !G || !r || !z || !rz_out) return -(int)hipErrorInvalidValue;
    const long total = regions_blocks(regions);
    const int grid = block_grid(total);
    hipLaunchKernelGGL(k_block_apply, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, regions, total, G, r, z, rz_out, gate);
    int e = check_launch(); return e ? e : grid;
}

int thallo_hip_block_step2(thallo_block_regions_t regions, const float* G, float* r, const float* Ap, float* z, thallo_sum_t aN, thallo_sum_t aD, float* betaN_out,
                           thallo_stream_t stream)
{
    if (!regions_ok(regions) || !G || !r || !Ap || !z || !betaN_out || !aN.partials || !aD.partials || aN.count < 1 || aD.count < 1) return -(int)hipErrorInvalidValue;
    const long total = regions_blocks(regions);
    const int grid = block_grid(total);
    hipLaunchKernelGGL(k_block_step2, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, regions, total, G, r, Ap, z, aN, aD, betaN_out);
    int e = check_launch(); return e ? e : grid;
}

int thallo_hip_block_step2_lm(thallo_block_regions_t regions, const float* G, float* delta, const float* p, float* r, const float* Ap, float* z, const float* b,
                              thallo_sum_t aN, thallo_sum_t aD, float* betaN_out, float* q_out, const unsigned* gate, thallo_stream_t stream)
{
    if (!regions_ok(regions) || !G || !delta || !p || !r || !Ap || !z || !b || !betaN_out || !q_out || !aN.partials || !aD.partials || aN.count < 1 || aD.count < 1)
        return -(int)hipErrorInvalidValue;
    const long total = regions_blocks(regions);
    const int grid = block_grid(total);
    hipLaunchKernelGGL(k_block_step2_lm, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, regions, total, G, delta, p, r, Ap, z, b, aN, aD, betaN_out, q_out, gate);
    int e = check_launch(); return e ? e : grid;
}

}  // extern "C"
