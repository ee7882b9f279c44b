// ba_schur_dense.hip -- a DENSE Cholesky solve of bundle adjustment's reduced camera system (DESIGN.md "Dense Cholesky Schur solve"; ThalloX_PlanSetLinearSolver
// THALLOX_SOLVER_SCHUR_DENSE).  Everything up to and including the assembly of S is ba_schur_explicit.hip's.  Once per step (and once per covariance call)
//
//   expand   the block-sparse, entry-major S becomes the dense lower triangle T = D S D, D = diag(S_ii)^-1/2 (block_chol.hpp's Jacobi scaling, here on the whole matrix),
//            row-major with a leading dimension that is a multiple of the panel width.  A scalar the caller holds, and one whose S_ii is not positive (a camera nothing
//            observes), gets d = 0 and the identity's row and column; the latter are counted in a device word.  Entry (i, j) is float(float(d_i S_ij) d_j): two rounded
//            products, nothing to contract.
//   potrf    T = L L^T in place, blocked right-looking, panels of 32 columns, three launches per panel:
//              diag   one wave factors the 32 x 32 diagonal block in registers, a row per lane, the pivot row's entries passed by v_readlane
//              trsm   the rows below: one row per thread, x L11^T = a by forward substitution in registers, spread over workgroups; L11 is wave-uniform (scalar loads)
//              syrk   A22 -= L21 L21^T on the lower triangle, 128 x 128 per workgroup, 64 x 64 per wave as 2 x 2 accumulators of v_mfma_f32_32x32x2_f32 (f32 in, f32
//                     accumulate: an fmaf chain over the panel's 32 columns in natural order), the two panels staged through LDS once
//            A pivot that is not positive stops nothing: the first such index + 1 goes to the info word and the factor goes on with 1.0 there (k_potrf_panel's convention).
//   potrs    x = D L^-T L^-1 D b.  _cols: panels of THALLO_HIP_COV_K right-hand sides in the covariance's layout [n][K], ONE LANE PER COLUMN, one workgroup per panel and
//            both sweeps in ONE launch: per block of 32 rows every wave solves the diagonal block for its lane's column in registers (the same numbers in every wave, so
//            nothing is broadcast), then the waves share the rows that are left, 32 at a time; L is wave-uniform and streamed once per workgroup.  _vec: one right-hand
//            side, one workgroup of sixteen waves, a row per lane in the diagonal block and a row per thread in the update.
// No float atomics; every element has one fixed summation order per n: two runs give equal bits, and a column's result does not depend on its companions in the panel.
// Nothing is indexed dynamically, every loop over a tile is unrolled.
#include "device_common.hpp"
#include "../../include/thallo_hip.h"

using namespace thallo;
using thallo::launch::check_launch;

namespace {

constexpr int NB = THALLO_HIP_DENSE_NB;
constexpr int K = THALLO_HIP_COV_K;
constexpr int TS = 128;           // the trailing update's tile per workgroup
constexpr int CW = 8;             // waves of a column panel's workgroup
constexpr int VT = 1024;          // threads of the one-column solve
constexpr int TRSM_MAX_WG = 32;   // workgroups of the panel solve (64 rows each); longer panels are strided
static_assert(NB == 32, "one 32x32x2 MFMA tile per panel step, a row per half wave");
typedef float f32x16 __attribute__((ext_vector_type(16)));

// lane `src` 's value (src: a compile-time constant after unrolling)
__device__ __forceinline__ float lane_get(float v, int src) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src)); }

// ------------------------------------------------------------------ expand
__global__ __launch_bounds__(256) void k_dense_scale(int C_, long nblk, const int* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ S,
                                                     const unsigned char* __restrict__ hold, float* __restrict__ d, unsigned* __restrict__ nonpos)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 9 * C_; i += gridDim.x * 256) {
        const int c = i / 9, a = i - 9 * c;
        int t = row_ptr[c];
        const int t1 = row_ptr[c + 1];
        while (t < t1 && col[t] != c) ++t;      // (every diagonal block is present)
        const float s = t < t1 ? S[(long)(10 * a) * nblk + t] : 0.0f;
        float di = 0.0f;
        if (hold != nullptr && hold[i]) di = 0.0f;
        else if (!(s > 0.0f)) atomicAdd(nonpos, 1u);
        else di = 1.0f / sqrtf(s);
        d[i] = di;
    }
}

__global__ __launch_bounds__(256) void k_dense_expand(int C_, long nblk, const int* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ S,
                                                      const float* __restrict__ d, long ld, float* __restrict__ T)
{
    for (int c = blockIdx.x; c < C_; c += gridDim.x) {
        float di[9];
#pragma unroll
        for (int a = 0; a < 9; ++a) di[a] = d[9L * c + a];
        const int t1 = row_ptr[c + 1];
        for (int t = row_ptr[c] + threadIdx.x; t < t1; t += 256) {
            const int cj = col[t];
            if (cj > c) continue;
            float dj[9];
#pragma unroll
            for (int b = 0; b < 9; ++b) dj[b] = d[9L * cj + b];
#pragma unroll
            for (int a = 0; a < 9; ++a)
#pragma unroll
                for (int b = 0; b < 9; ++b) {
                    const long i = 9L * c + a, j = 9L * cj + b;
                    if (j > i) continue;
                    const float s = S[(long)(9 * a + b) * nblk + t];
                    const float v = (di[a] > 0.0f && dj[b] > 0.0f) ? __fmul_rn(__fmul_rn(di[a], s), dj[b]) : (i == j ? 1.0f : 0.0f);
                    T[i * ld + j] = v;
                }
        }
    }
}

// ------------------------------------------------------------------ potrf
// One wave: lane r (and its mirror r + 32, which stores nothing) holds row r of the diagonal block.  Rows past n are the identity's.
__global__ __launch_bounds__(64) void k_dense_potrf_diag(long n, long ld, long k, float* __restrict__ T, int* __restrict__ info)
{
    const int r = threadIdx.x & 31;
    const bool in = k + r < n;
    float* row = T + (k + (in ? r : 0)) * ld + k;
    float a[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) a[c] = (in && c <= r) ? row[c] : (c == r ? 1.0f : 0.0f);
    int bad = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const float djj = lane_get(a[j], j);
        const bool ok = djj > 0.0f;
        if (!ok && bad == 0) bad = j + 1;
        const float l = ok ? sqrtf(djj) : 1.0f;
        if (r == j) a[j] = l; else if (r > j) a[j] = a[j] / l;
#pragma unroll
        for (int c = j + 1; c < NB; ++c) {
            const float lc = lane_get(a[j], c);
            if (r >= c) a[c] -= a[j] * lc;
        }
    }
    if (threadIdx.x == 0 && bad != 0 && info[0] == 0) info[0] = (int)k + bad;
    if (in && threadIdx.x < 32) {
#pragma unroll
        for (int c = 0; c < NB; ++c) if (c <= r) row[c] = a[c];
    }
}

// The rows below a full diagonal block D = L11 (wave-uniform): x L11^T = a, one row per thread
__global__ __launch_bounds__(64) void k_dense_trsm(long n, long ld, long k, const float* __restrict__ D, float* __restrict__ A)
{
    for (long r = k + NB + (long)blockIdx.x * 64 + threadIdx.x; r < n; r += (long)gridDim.x * 64) {
        float4* row = reinterpret_cast<float4*>(A + r * ld + k);
        float x[NB];
#pragma unroll
        for (int c = 0; c < NB / 4; ++c) { const float4 v = row[c]; x[4 * c] = v.x; x[4 * c + 1] = v.y; x[4 * c + 2] = v.z; x[4 * c + 3] = v.w; }
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            float v = x[c];
#pragma unroll
            for (int q = 0; q < c; ++q) v -= x[q] * D[c * ld + q];
            x[c] = v / D[c * ld + c];
        }
#pragma unroll
        for (int c = 0; c < NB / 4; ++c) row[c] = make_float4(x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]);
    }
}

// A22 -= L21 L21^T, lower triangle, TS x TS per workgroup.  Operands of v_mfma_f32_32x32x2_f32: lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31];
// result register v of lane l is element (row (v & 3) + 8 (v >> 2) + 4 (l >> 5), column l & 31)
__global__ __launch_bounds__(256) void k_dense_syrk(long n, long ld, long k, float* __restrict__ T)
{
    __shared__ float P[TS][NB + 1], Q[TS][NB + 1];
    const int tr = blockIdx.y, tc = blockIdx.x;
    if (tc > tr) return;
    const long r0 = k + NB + (long)tr * TS, c0 = k + NB + (long)tc * TS;
    const int t = threadIdx.x;
#pragma unroll
    for (int p = 0; p < TS / 32; ++p) {
        const int i = (t >> 3) + 32 * p, j4 = (t & 7) * 4;
        float4 u = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v = u;
        if (r0 + i < n) u = *reinterpret_cast<const float4*>(T + (r0 + i) * ld + k + j4);
        if (c0 + i < n) v = *reinterpret_cast<const float4*>(T + (c0 + i) * ld + k + j4);
        P[i][j4] = u.x; P[i][j4 + 1] = u.y; P[i][j4 + 2] = u.z; P[i][j4 + 3] = u.w;
        Q[i][j4] = v.x; Q[i][j4 + 1] = v.y; Q[i][j4 + 2] = v.z; Q[i][j4 + 3] = v.w;
    }
    __syncthreads();
    const int w = t >> 6, l = t & 63, m = l & 31, h = l >> 5;
    const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
    if (tr == tc && wc > wr) return;          // (wholly above the diagonal)
    f32x16 acc00, acc01, acc10, acc11;
#pragma unroll
    for (int v = 0; v < 16; ++v) { acc00[v] = 0.0f; acc01[v] = 0.0f; acc10[v] = 0.0f; acc11[v] = 0.0f; }
#pragma unroll
    for (int q = 0; q < NB; q += 2) {
        const float a0 = P[wr + m][q + h], a1 = P[wr + 32 + m][q + h], b0 = Q[wc + m][q + h], b1 = Q[wc + 32 + m][q + h];
        acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
    }
    auto store = [&](const f32x16& acc, int ti, int tj) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const long i = r0 + wr + 32 * ti + (v & 3) + 8 * (v >> 2) + 4 * h, j = c0 + wc + 32 * tj + m;
            if (i < n && j <= i) T[i * ld + j] -= acc[v];
        }
    };
    store(acc00, 0, 0); store(acc01, 0, 1); store(acc10, 1, 0); store(acc11, 1, 1);
}

// ------------------------------------------------------------------ potrs, a panel of K columns per workgroup, a lane per column
// FWD: y = L^-1 D b; BWD: x = D L^-T y (both: one launch; one of them: the sweep alone, for the tests of each sweep's bound)
template <bool FWD, bool BWD>
__global__ __launch_bounds__(64 * CW) void k_dense_potrs_cols(long n, long ld, const float* __restrict__ L, const float* __restrict__ d, float* __restrict__ B)
{
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* X = B + (long)blockIdx.x * n * K + lane;
    if (FWD && d != nullptr) for (long i = w; i < n; i += CW) X[i * K] *= d[i];
    for (long k = 0; FWD && k < n; k += NB) {             // L y = D b
        __syncthreads();
        float xs[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) xs[c] = k + c < n ? X[(k + c) * K] : 0.0f;
        __syncthreads();                                  // (every wave has read the block before wave 0 overwrites it)
#pragma unroll
        for (int c = 0; c < NB; ++c)
            if (k + c < n) {
                const float* lr = L + (k + c) * ld + k;
                float v = xs[c];
#pragma unroll
                for (int q = 0; q < c; ++q) v -= lr[q] * xs[q];
                xs[c] = v / lr[c];
                __builtin_amdgcn_sched_barrier(0);
            }
        if (w == 0) {
#pragma unroll
            for (int c = 0; c < NB; ++c) if (k + c < n) X[(k + c) * K] = xs[c];
        }
        for (long r0 = k + NB + (long)NB * w; r0 < n; r0 += (long)NB * CW) {
#pragma unroll
            for (int i = 0; i < NB; ++i)
                if (r0 + i < n) {
                    const float* lr = L + (r0 + i) * ld + k;
                    float s = 0.0f;
#pragma unroll
                    for (int q = 0; q < NB; ++q) s += lr[q] * xs[q];
                    X[(r0 + i) * K] -= s;
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
    }
    for (long k = (n - 1) / NB * NB; BWD && k >= 0; k -= NB) {   // L^T x = y, then D x
        __syncthreads();
        float xs[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) xs[c] = k + c < n ? X[(k + c) * K] : 0.0f;
        __syncthreads();
#pragma unroll
        for (int c = NB - 1; c >= 0; --c)
            if (k + c < n) {
                float v = xs[c];
#pragma unroll
                for (int q = c + 1; q < NB; ++q) { const long rq = k + q < n ? k + q : n - 1; v -= L[rq * ld + k + c] * xs[q]; }      // (a row past n: the last row's finite entry times 0)
                xs[c] = v / L[(k + c) * ld + k + c];
                __builtin_amdgcn_sched_barrier(0);
            }
        if (w == 0) {
#pragma unroll
            for (int c = 0; c < NB; ++c) if (k + c < n) X[(k + c) * K] = d != nullptr ? xs[c] * d[k + c] : xs[c];
        }
        for (long r0 = (long)NB * w; r0 < k; r0 += (long)NB * CW) {
            float s[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) s[i] = 0.0f;
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const long rq = k + q < n ? k + q : n - 1;
                const float* lr = L + rq * ld + r0;
#pragma unroll
                for (int i = 0; i < NB; ++i) s[i] += lr[i] * xs[q];
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) X[(r0 + i) * K] -= s[i];
        }
    }
}

// ------------------------------------------------------------------ potrs, one right-hand side, one workgroup
template <bool FWD, bool BWD>
__global__ __launch_bounds__(VT) void k_dense_potrs_vec(long n, long ld, const float* __restrict__ L, const float* __restrict__ d, const float* __restrict__ b, float* __restrict__ x)
{
    const int t = threadIdx.x, r = t & 31;
    for (long i = t; i < n; i += VT) x[i] = FWD && d != nullptr ? b[i] * d[i] : b[i];
    for (long k = 0; FWD && k < n; k += NB) {             // L y = D b
        __syncthreads();
        const bool in = k + r < n;
        const float* lrow = L + (k + (in ? r : 0)) * ld + k;
        float a[NB], xs[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) a[c] = (in && c < r) ? lrow[c] : 0.0f;
        const float dg = in ? L[(k + r) * ld + k + r] : 1.0f;
        float xr = in ? x[k + r] : 0.0f;
        __syncthreads();                                  // (every wave has read the block before wave 0 overwrites it)
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            if (r == c) xr = xr / dg;
            xs[c] = lane_get(xr, c);
            if (r > c) xr -= a[c] * xs[c];
        }
        if (t < 32 && in) x[k + r] = xr;
        for (long row = k + NB + t; row < n; row += VT) {
            const float4* lp = reinterpret_cast<const float4*>(L + row * ld + k);
            float s = 0.0f;
#pragma unroll
            for (int q = 0; q < NB / 4; ++q) {
                const float4 v = lp[q];
                s += v.x * xs[4 * q]; s += v.y * xs[4 * q + 1]; s += v.z * xs[4 * q + 2]; s += v.w * xs[4 * q + 3];
            }
            x[row] -= s;
        }
    }
    for (long k = (n - 1) / NB * NB; BWD && k >= 0; k -= NB) {   // L^T x = y, then D x
        __syncthreads();
        const bool in = k + r < n;
        float a[NB], xs[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) a[c] = (c > r && k + c < n) ? L[(k + c) * ld + k + r] : 0.0f;
        const float dg = in ? L[(k + r) * ld + k + r] : 1.0f;
        float xr = in ? x[k + r] : 0.0f;
        __syncthreads();
#pragma unroll
        for (int c = NB - 1; c >= 0; --c) {
            if (r == c) xr = xr / dg;
            xs[c] = lane_get(xr, c);
            if (r < c) xr -= a[c] * xs[c];
        }
        if (t < 32 && in) x[k + r] = d != nullptr ? xr * d[k + r] : xr;
        for (long row = t; row < k; row += VT) {
            float s = 0.0f;
#pragma unroll
            for (int q = 0; q < NB; ++q) { const long rq = k + q < n ? k + q : n - 1; s += L[rq * ld + row] * xs[q]; }      // (a row past n: the last row's finite entry times 0)
            x[row] -= s;
        }
    }
}

inline bool dims_ok(long n, long ld) { return n >= 1 && n <= THALLO_HIP_DENSE_MAX_N && ld >= n && ld % NB == 0; }
inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

long thallo_hip_dense_ld(long n) { return n < 1 ? -1 : (n + NB - 1) / NB * NB; }

int thallo_hip_ba_schur_dense_expand(int C_, long nblk, const int* row_ptr, const int* col, const float* S, const unsigned char* hold, long ld, float* T, float* d, unsigned* nonpos,
                                     thallo_stream_t stream)
{
    if (C_ < 1 || nblk < C_ || !row_ptr || !col || !S || !T || !d || !nonpos || !dims_ok(9L * C_, ld)) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if ((e = hipMemsetAsync(nonpos, 0, sizeof(unsigned), s)) != hipSuccess) return -(int)e;
    if ((e = hipMemsetAsync(T, 0, sizeof(float) * (size_t)ld * 9 * (size_t)C_, s)) != hipSuccess) return -(int)e;      // (the pairs that are not co-visible)
    int g = (9 * C_ + 255) / 256; if (g > 256) g = 256;
    hipLaunchKernelGGL(k_dense_scale, dim3(g), dim3(256), 0, s, C_, nblk, row_ptr, col, S, hold, d, nonpos);
    hipLaunchKernelGGL(k_dense_expand, dim3(C_ > 1024 ? 1024 : C_), dim3(256), 0, s, C_, nblk, row_ptr, col, S, (const float*)d, ld, T);
    return check_launch();
}

int thallo_hip_dense_potrf(long n, long ld, float* T, int* info, thallo_stream_t stream)
{
    if (!dims_ok(n, ld) || !T || !info || !aligned16(T)) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(info, 0, sizeof(int), s);
    if (e != hipSuccess) return -(int)e;
    for (long k = 0; k < n; k += NB) {
        hipLaunchKernelGGL(k_dense_potrf_diag, dim3(1), dim3(64), 0, s, n, ld, k, T, info);
        const long rest = n - k - NB;
        if (rest <= 0) break;
        long g = (rest + 63) / 64; if (g > TRSM_MAX_WG) g = TRSM_MAX_WG;
        hipLaunchKernelGGL(k_dense_trsm, dim3((unsigned)g), dim3(64), 0, s, n, ld, k, (const float*)(T + k * ld + k), T);
        const unsigned tiles = (unsigned)((rest + TS - 1) / TS);
        hipLaunchKernelGGL(k_dense_syrk, dim3(tiles, tiles), dim3(256), 0, s, n, ld, k, T);
    }
    return check_launch();
}

int thallo_hip_dense_potrs_cols(long n, long ld, const float* L, const float* d, float* B, int ngroups, int sweeps, thallo_stream_t stream)
{
    if (!dims_ok(n, ld) || !L || !B || ngroups < 1 || ngroups > 65535 || sweeps < THALLO_HIP_DENSE_BOTH || sweeps > THALLO_HIP_DENSE_BACKWARD) return -(int)hipErrorInvalidValue;
    const dim3 g((unsigned)ngroups), b(64 * CW);
    hipStream_t s = (hipStream_t)stream;
    if (sweeps == THALLO_HIP_DENSE_BOTH) hipLaunchKernelGGL((k_dense_potrs_cols<true, true>), g, b, 0, s, n, ld, L, d, B);
    else if (sweeps == THALLO_HIP_DENSE_FORWARD) hipLaunchKernelGGL((k_dense_potrs_cols<true, false>), g, b, 0, s, n, ld, L, d, B);
    else hipLaunchKernelGGL((k_dense_potrs_cols<false, true>), g, b, 0, s, n, ld, L, d, B);
    return check_launch();
}

int thallo_hip_dense_potrs_vec(long n, long ld, const float* L, const float* d, const float* b, float* x, int sweeps, thallo_stream_t stream)
{
    if (!dims_ok(n, ld) || !L || !b || !x || b == x || !aligned16(L) || sweeps < THALLO_HIP_DENSE_BOTH || sweeps > THALLO_HIP_DENSE_BACKWARD) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    if (sweeps == THALLO_HIP_DENSE_BOTH) hipLaunchKernelGGL((k_dense_potrs_vec<true, true>), dim3(1), dim3(VT), 0, s, n, ld, L, d, b, x);
    else if (sweeps == THALLO_HIP_DENSE_FORWARD) hipLaunchKernelGGL((k_dense_potrs_vec<true, false>), dim3(1), dim3(VT), 0, s, n, ld, L, d, b, x);
    else hipLaunchKernelGGL((k_dense_potrs_vec<false, true>), dim3(1), dim3(VT), 0, s, n, ld, L, d, b, x);
    return check_launch();
}

}  // extern "C"
