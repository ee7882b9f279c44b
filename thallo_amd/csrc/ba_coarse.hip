// ba_coarse.hip -- the COARSE CORRECTION of the two-level preconditioner on bundle adjustment's assembled reduced camera matrix (DESIGN.md "Two-level preconditioner";
// ThalloX_PlanSetPreconditioner THALLOX_PRECOND_TWO_LEVEL).  The cameras are partitioned into K aggregates (built on the host at Init); the coarse space is piecewise
// constant per camera parameter: P[9 c + j, 9 a(c) + j] = 1 at a free scalar, n_c = 9 K.  Once per step, behind ba_schur_explicit.hip's assembly
//
//   assemble   S_c = P^T S P: block (a, b), b <= a, is the sum of S_cc' over c in a, c' in b with the rows and columns of held scalars left out.  One workgroup per
//              coarse block row; every accumulator (b, entry) is owned by ONE thread (wave (b - b0) mod 8 of the workgroup, lane = entry, lanes 0 .. 16 entries 64 .. 80 as
//              well), which walks the members' rows in list order and a row's blocks in ascending column: one fixed order, no atomics.  The accumulators sit in LDS, 128
//              aggregates (41472 bytes) at a time: more aggregates than that are walked in column chunks.  Only the dense lower triangle is written, row-major with
//              thallo_hip_dense_ld's leading dimension.
//   scale      T = D S_c D, D = diag(S_c,ii)^-1/2, float(float(d_i s) d_j): two rounded products, nothing to contract (ba_schur_dense.hip's k_dense_expand).  A coarse
//              scalar whose diagonal is not positive (every member held there, or nothing observed) gets d = 0 and the identity's row and column, and is counted.
//   (factor)   thallo_hip_dense_potrf, unchanged.
//   inverse    Z = L^-1 D: identity panels through thallo_hip_dense_potrs_cols' forward sweep (a lane per column), then a packing launch that stores Z and Z^T row-major so
//              that both products of the apply stream rows.  The packing launch reads the factor's info word ON THE DEVICE: a factor that met a pivot that is not positive
//              leaves Z = 0 for the step (the preconditioner is then block Jacobi alone) and raises a device counter -- no read-back, no failed step.
//   apply      z += P Z^T Z P^T r and the partials of |Z P^T r|^2, two launches.  (a): every workgroup rebuilds the prefix of r_c = P^T r it needs in LDS (a segmented sum over
//              each aggregate's member list in list order; r is 9 C floats, L2-resident), then y = Z r_c, one wave per row (Z is lower triangular: row i reads i + 1
//              words), lanes strided, the wave butterfly; one partial of y . y per workgroup.  (b): one workgroup per aggregate: t = Z^T y for its nine rows, then
//              z[9 c + j] += t[j] at the free scalars of its members -- every camera is in one aggregate, so no two workgroups write one word.
//   apply_cols the covariance's panel form on [9 C][THALLO_HIP_COV_K], ONE LANE PER COLUMN, Z wave-uniform (k_apply_s_cols' pattern), three launches: the panel r_c (a wave
//              per coarse scalar, the member list in list order), Y = Z r_c with one partial of y . y per workgroup and column, and per aggregate T = Z^T Y for its nine
//              rows (a wave each) and the scatter into the panel Z.  Every sum of a column is its lane's alone: a column's result does not depend on its companions, a zero
//              column stays zero; a frozen column is not touched and leaves a zero partial.
// M^-1 = G^T G + (Z P^T)^T (Z P^T) is symmetric positive semi-definite plus the block term whatever the rounding of Z, and has zero rows and columns at held scalars.
// Sums: one fixed order per shape, no float atomics: two runs give equal bits.  All kernels are wave64.
#include "device_common.hpp"
#include "../../include/thallo_hip.h"

using namespace thallo;
using thallo::launch::check_launch;

namespace {

constexpr int K = THALLO_HIP_COV_K;
constexpr int AW = 8;             // waves of the assembly's workgroup
constexpr int ACH = 128;          // aggregates (block columns) whose accumulators sit in LDS at a time
constexpr int NMAX = THALLO_HIP_COARSE_MAX_N;
constexpr int APPLY_WG = THALLO_HIP_COARSE_PARTIALS;

__global__ __launch_bounds__(64 * AW) void k_coarse_assemble(int K_, long nblk, const int* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ S,
                                                             const int* __restrict__ agg, const int* __restrict__ mem_ptr, const int* __restrict__ mem,
                                                             const unsigned char* __restrict__ hold, long ld, float* __restrict__ T)
{
    __shared__ float acc[ACH * 81];
    const int a = blockIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int e1 = lane < 17 ? lane + 64 : lane;          // lanes 0 .. 16 own entries 64 .. 80 as well
    const int i0 = lane / 9, j0 = lane - 9 * i0, i1 = e1 / 9, j1 = e1 - 9 * i1;
    const int m0 = mem_ptr[a], m1 = mem_ptr[a + 1];
    for (int b0 = 0; b0 <= a; b0 += ACH) {
        const int nb = min(ACH, a + 1 - b0);
        for (int i = threadIdx.x; i < nb * 81; i += 64 * AW) acc[i] = 0.0f;
        __syncthreads();
        for (int m = m0; m < m1; ++m) {
            const int c = mem[m];
            const bool hr0 = hold != nullptr && hold[9L * c + i0] != 0, hr1 = hold != nullptr && hold[9L * c + i1] != 0;
            const int t1 = row_ptr[c + 1];
            for (int t = row_ptr[c]; t < t1; ++t) {
                const int cj = col[t], b = agg[cj] - b0;
                if (b < 0 || b >= nb || (b & (AW - 1)) != wave) continue;      // (wave-uniform)
                const bool h0 = hr0 || (hold != nullptr && hold[9L * cj + j0] != 0), h1 = hr1 || (hold != nullptr && hold[9L * cj + j1] != 0);
                const float s0 = S[(long)lane * nblk + t], s1 = S[(long)e1 * nblk + t];
                if (!h0) acc[b * 81 + lane] += s0;
                if (lane < 17 && !h1) acc[b * 81 + e1] += s1;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < nb * 81; i += 64 * AW) {
            const int b = i / 81, e = i - 81 * b, ei = e / 9, ej = e - 9 * ei;
            const long row = 9L * a + ei, cl = 9L * (b0 + b) + ej;
            if (cl <= row) T[row * ld + cl] = acc[i];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_coarse_d(long n, long ld, const float* __restrict__ T, float* __restrict__ d, unsigned* __restrict__ identity)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float s = T[i * ld + i];
        float di = 0.0f;
        if (!(s > 0.0f)) atomicAdd(identity, 1u);
        else di = 1.0f / sqrtf(s);
        d[i] = di;
    }
}

__global__ __launch_bounds__(256) void k_coarse_scale(long n, long ld, const float* __restrict__ d, float* __restrict__ T)
{
    for (long i = blockIdx.x; i < n; i += gridDim.x) {
        const float di = d[i];
        for (long j = threadIdx.x; j <= i; j += 256) {
            const float dj = d[j], s = T[i * ld + j];
            T[i * ld + j] = (di > 0.0f && dj > 0.0f) ? __fmul_rn(__fmul_rn(di, s), dj) : (i == j ? 1.0f : 0.0f);
        }
    }
}

// The identity as ceil(n / K) panels [n][K] of right-hand sides: panel g holds the unit columns K g .. K g + K - 1
__global__ __launch_bounds__(256) void k_coarse_eye(long n, long total, float* __restrict__ B)
{
    for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < total; x += (long)gridDim.x * 256) {
        const long g = x / (n * K), rest = x - g * n * K, i = rest / K, k = rest - i * K;
        B[x] = i == g * K + k ? 1.0f : 0.0f;
    }
}

// Z[i][j] = panel j / K, row i, column j mod K for j <= i, 0 above the diagonal and in the padding columns; Zt its transpose.  A factor whose info word is not zero: zeros
__global__ __launch_bounds__(256) void k_coarse_pack(long n, long ld, const float* __restrict__ B, const int* __restrict__ info, float* __restrict__ Z, float* __restrict__ Zt,
                                                     unsigned* __restrict__ failed)
{
    const bool bad = info[0] != 0;
    if (bad && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(failed, 1u);
    for (long i = blockIdx.x; i < n; i += gridDim.x)
        for (long j = threadIdx.x; j < ld; j += 256) {
            float v = 0.0f;
            if (!bad && j <= i) v = B[((j / K) * n + i) * K + (j % K)];
            Z[i * ld + j] = v;
            if (j < n) Zt[j * ld + i] = v;
        }
}

__global__ __launch_bounds__(256) void k_coarse_apply_a(long n, long ld, const float* __restrict__ Z, const int* __restrict__ mem_ptr, const int* __restrict__ mem,
                                                        const unsigned char* __restrict__ hold, const float* __restrict__ r, float* __restrict__ y, float* __restrict__ part_out,
                                                        const unsigned* __restrict__ gate)
{
    __shared__ float rc[NMAX];
    __shared__ float red[4];
    if (gate != nullptr && __builtin_amdgcn_readfirstlane((int)gate[0]) != 0) return;      // LM: the PCG loop already ended on the device
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // the rows of this workgroup: 4 (blockIdx + trip gridDim) + wave; with one trip the prefix up to its last row is all it reads
    const long need = 4L * gridDim.x >= n ? min(n, 4L * blockIdx.x + 4) : n;
    for (long i = threadIdx.x; i < need; i += 256) {
        const long a = i / 9; const int j = (int)(i - 9 * a);
        float s = 0.0f;
        for (int m = mem_ptr[a]; m < mem_ptr[a + 1]; ++m) {
            const long u = 9L * mem[m] + j;
            if (hold == nullptr || hold[u] == 0) s += r[u];
        }
        rc[i] = s;
    }
    __syncthreads();
    float acc = 0.0f;
    for (long i = 4L * blockIdx.x + wave; i < n; i += 4L * gridDim.x) {
        const float* zr = Z + i * ld;
        float s = 0.0f;
        for (long j = lane; j <= i; j += 64) s += zr[j] * rc[j];
        s = wave_sum_all(s);
        if (lane == 0) y[i] = s;
        acc += s * s;
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part_out[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_coarse_apply_b(long n, long ld, const float* __restrict__ Zt, const int* __restrict__ mem_ptr, const int* __restrict__ mem,
                                                        const unsigned char* __restrict__ hold, const float* __restrict__ y, float* __restrict__ z, const unsigned* __restrict__ gate)
{
    __shared__ float ts[12];
    if (gate != nullptr && __builtin_amdgcn_readfirstlane((int)gate[0]) != 0) return;
    const int a = blockIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int q = wave; q < 9; q += 4) {
        const long i = 9L * a + q;
        const float* zr = Zt + i * ld;
        float s = 0.0f;
        for (long j = (i & ~63L) + lane; j < n; j += 64) if (j >= i) s += zr[j] * y[j];
        s = wave_sum_all(s);
        if (lane == 0) ts[q] = s;
    }
    __syncthreads();
    const int m0 = mem_ptr[a], cnt = (mem_ptr[a + 1] - m0) * 9;
    for (int x = threadIdx.x; x < cnt; x += 256) {
        const int m = x / 9, j = x - 9 * m;
        const long u = 9L * mem[m0 + m] + j;
        if (hold == nullptr || hold[u] == 0) z[u] += ts[j];
    }
}

__global__ __launch_bounds__(K) void k_coarse_rc_cols(long n, const int* __restrict__ mem_ptr, const int* __restrict__ mem, const unsigned char* __restrict__ hold,
                                                      const float* __restrict__ R, float* __restrict__ RC)
{
    const int lane = threadIdx.x;
    for (long i = blockIdx.x; i < n; i += gridDim.x) {
        const long a = i / 9; const int j = (int)(i - 9 * a);
        float s = 0.0f;
        for (int m = mem_ptr[a]; m < mem_ptr[a + 1]; ++m) {
            const long u = 9L * mem[m] + j;
            if (hold == nullptr || hold[u] == 0) s += R[u * K + lane];
        }
        RC[i * K + lane] = s;
    }
}

__global__ __launch_bounds__(K) void k_coarse_y_cols(long n, long ld, const float* __restrict__ Z, const float* __restrict__ RC, float* __restrict__ Y,
                                                     const unsigned* __restrict__ frozen, float* __restrict__ part)
{
    const int lane = threadIdx.x;
    const bool live = frozen == nullptr || frozen[lane] == 0u;
    float acc = 0.0f;
    for (long i = blockIdx.x; i < n; i += gridDim.x) {
        const float* zr = Z + i * ld;
        const float* x = RC + lane;
        float s = 0.0f;
#pragma unroll 8
        for (long j = 0; j <= i; ++j) s += zr[j] * x[j * K];
        Y[i * K + lane] = s;
        acc += s * s;
    }
    part[(long)blockIdx.x * K + lane] = live ? acc : 0.0f;
}

__global__ __launch_bounds__(9 * K) void k_coarse_t_cols(long n, long ld, const float* __restrict__ Zt, const float* __restrict__ Y, const int* __restrict__ mem_ptr,
                                                         const int* __restrict__ mem, const unsigned char* __restrict__ hold, const unsigned* __restrict__ frozen,
                                                         float* __restrict__ Zp)
{
    __shared__ float ts[9 * K];
    const int a = blockIdx.x, lane = threadIdx.x & (K - 1), q = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / K));
    {
        const long i = 9L * a + q;
        const float* zr = Zt + i * ld;
        const float* y = Y + lane;
        float s = 0.0f;
#pragma unroll 8
        for (long j = i; j < n; ++j) s += zr[j] * y[j * K];
        ts[q * K + lane] = s;
    }
    __syncthreads();
    if (frozen != nullptr && frozen[lane] != 0u) return;
    const int m0 = mem_ptr[a], m1 = mem_ptr[a + 1];
    for (int m = m0; m < m1; ++m) {
        const long u = 9L * mem[m] + q;
        if (hold == nullptr || hold[u] == 0) Zp[u * K + lane] += ts[q * K + lane];
    }
}

inline bool coarse_ok(const thallo_coarse_t* c)
{
    return c && c->C >= 1 && c->K >= 1 && c->K <= c->C && c->n == 9L * c->K && c->n <= NMAX && c->ld == thallo_hip_dense_ld(c->n) && c->agg && c->mem_ptr && c->mem && c->T && c->d &&
           c->Z && c->Zt && c->y && c->words;
}

}  // namespace

extern "C" {

long thallo_hip_ba_coarse_panel_floats(long n) { return n < 1 || n > NMAX ? -1 : (n + K - 1) / K * n * K; }

int thallo_hip_ba_coarse_assemble(const thallo_coarse_t* c, long nblk, const int* row_ptr, const int* col, const float* S, thallo_stream_t stream)
{
    if (!coarse_ok(c) || nblk < c->C || !row_ptr || !col || !S) return -(int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_coarse_assemble, dim3((unsigned)c->K), dim3(64 * AW), 0, (hipStream_t)stream, c->K, nblk, row_ptr, col, S, c->agg, c->mem_ptr, c->mem, c->hold, c->ld, c->T);
    return check_launch();
}

int thallo_hip_ba_coarse_scale(const thallo_coarse_t* c, thallo_stream_t stream)
{
    if (!coarse_ok(c)) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(c->words + 1, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(k_coarse_d, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, s, c->n, c->ld, (const float*)c->T, c->d, c->words + 1);
    hipLaunchKernelGGL(k_coarse_scale, dim3((unsigned)(c->n > 1024 ? 1024 : c->n)), dim3(256), 0, s, c->n, c->ld, (const float*)c->d, c->T);
    return check_launch();
}

int thallo_hip_ba_coarse_inverse(const thallo_coarse_t* c, float* panels, thallo_stream_t stream)
{
    if (!coarse_ok(c) || !panels) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const long total = thallo_hip_ba_coarse_panel_floats(c->n);
    const int groups = (int)((c->n + K - 1) / K);
    hipLaunchKernelGGL(k_coarse_eye, dim3((unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256)), dim3(256), 0, s, c->n, total, panels);
    int rc = check_launch();
    if (rc < 0) return rc;
    if ((rc = thallo_hip_dense_potrs_cols(c->n, c->ld, c->T, c->d, panels, groups, THALLO_HIP_DENSE_FORWARD, stream)) < 0) return rc;
    hipLaunchKernelGGL(k_coarse_pack, dim3((unsigned)(c->n > 1024 ? 1024 : c->n)), dim3(256), 0, s, c->n, c->ld, (const float*)panels, (const int*)c->words, c->Z, c->Zt, c->words + 2);
    return check_launch();
}

int thallo_hip_ba_coarse_apply(const thallo_coarse_t* c, const float* r, float* z, float* yy_out, const unsigned* gate, thallo_stream_t stream)
{
    if (!coarse_ok(c) || !r || !z || !yy_out) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    long g = (c->n + 3) / 4; if (g > APPLY_WG) g = APPLY_WG;
    hipLaunchKernelGGL(k_coarse_apply_a, dim3((unsigned)g), dim3(256), 0, s, c->n, c->ld, (const float*)c->Z, c->mem_ptr, c->mem, c->hold, r, c->y, yy_out, gate);
    hipLaunchKernelGGL(k_coarse_apply_b, dim3((unsigned)c->K), dim3(256), 0, s, c->n, c->ld, (const float*)c->Zt, c->mem_ptr, c->mem, c->hold, (const float*)c->y, z, gate);
    const int e = check_launch(); return e ? e : (int)g;
}

long thallo_hip_ba_coarse_cols_work_floats(long n) { return n < 1 || n > NMAX ? -1 : 2 * n * K; }

int thallo_hip_ba_coarse_apply_cols(const thallo_coarse_t* c, float* work, const float* R, float* Zp, const unsigned* frozen, float* yy_out, thallo_stream_t stream)
{
    if (!coarse_ok(c) || !work || !R || !Zp || !yy_out) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    float *RC = work, *Y = work + c->n * K;
    const long g = c->n > THALLO_HIP_COARSE_COLS_PARTIALS ? THALLO_HIP_COARSE_COLS_PARTIALS : c->n;
    hipLaunchKernelGGL(k_coarse_rc_cols, dim3((unsigned)(c->n > 1024 ? 1024 : c->n)), dim3(K), 0, s, c->n, c->mem_ptr, c->mem, c->hold, R, RC);
    hipLaunchKernelGGL(k_coarse_y_cols, dim3((unsigned)g), dim3(K), 0, s, c->n, c->ld, (const float*)c->Z, (const float*)RC, Y, frozen, yy_out);
    hipLaunchKernelGGL(k_coarse_t_cols, dim3((unsigned)c->K), dim3(9 * K), 0, s, c->n, c->ld, (const float*)c->Zt, (const float*)Y, c->mem_ptr, c->mem, c->hold, frozen, Zp);
    const int e = check_launch(); return e ? e : (int)g;
}

}  // extern "C"
