// ba_covariance.hip -- marginal covariances of bundle adjustment's cameras and points (DESIGN.md "Marginal covariances"; ThalloX_PlanCovariance).  With A = J^T J at the
// current unknowns, F the scalars the caller does not hold and Sigma = (A_FF)^-1 bordered by zeros, through the Schur complement on the cameras
//
//   Sigma_cc = S^-1 on the free cameras,          Sigma_pp = Cp^-1 + V^T S^-1 V,   V = E_p Cp^-1 (9 C x 3; W_q G_p at the rows of camera c(q)),  Cp^-1 = G^T G
//
// so a camera's block needs nine columns of S^-1 and a point's three columns of S^-1 V.  The columns are solved in batches of K = 64 by PCG on the ASSEMBLED S
// (ba_schur_explicit.hip) with the camera blocks' G^T G as preconditioner (block_precond.hip), ONE LANE PER COLUMN: a panel is [9 C][K] floats, a scalar's K columns
// consecutive, and every sum, scalar, freeze decision and update of a column is made by that column's lane alone -- a column's result does not depend on its companions.
//
//   cov_rhs            the right-hand sides: a camera's nine unit columns, or a point's W_q G_p over its list in list order (one thread per column)
//   apply_s_cols       Y = S X for a panel and per column the partials of x . S x: one wave per camera row; the row's blocks are read coalesced from the entry-major planes
//                      S[e * nblk + blk] (32 blocks per chunk: lanes 0 .. 31 entries 0 .. 40, lanes 32 .. 63 entries 41 .. 80), staged in LDS (a block's 81 entries would
//                      otherwise be 81 separate lines for a wave that needs them uniform), then every lane runs its column over the chunk's blocks in ascending order,
//                      81 FMAs per block, the rows of X of camera col[t] read coalesced.  No wave reduction.
//   cov_step           Z = G^T G R per camera (block_chol.hpp apply_g, the block's 45 floats wave-uniform) and the partials of r . z; as the PCG update, first
//                      X += alpha P, R -= alpha Y with the column's alpha.  A frozen column is skipped: its X never changes again.
//   cov_scal           one workgroup adds a slot's partials per column in a fixed order and forms the column's scalars, which stay on the device:
//                      alpha = alphaN / alphaD (0 where alphaD <= 0), beta = betaN / alphaN (0 where alphaN <= 0), and the freeze: r . z <= rel_tol^2 r0 . z0
//   cov_pupdate        P = Z + beta P
//   cov_out            a camera's block 0.5 (X_ii + X_ii^T); a point's G^T G + sum_q (W_q G)^T X_c(q) over its list, symmetrised the same way: bitwise symmetric
// Partials: one per workgroup and column, in a fixed order, min(C, 1024) of them whatever the batch holds; no float atomics.  Every loop over a block is unrolled.
#include "device_common.hpp"
#include "block_regions.hpp"      // tri
#include "block_chol.hpp"         // apply_g
#include "../../include/thallo_hip.h"
#include <cmath>

using namespace thallo;
using thallo::launch::check_launch;

namespace {

constexpr int K = THALLO_HIP_COV_K;
constexpr int WS = THALLO_HIP_SCHUR_W_STRIDE;
constexpr int CH = 32;            // blocks of a row staged per chunk
constexpr int LS = 81;            // floats from one staged block to the next: odd, so the 32 lanes of a store hit 32 banks
constexpr int HALF = 41;          // entries 0 .. 40 by lanes 0 .. 31, 41 .. 80 by lanes 32 .. 63
enum { SC_AN = 0, SC_R0, SC_ALPHA, SC_BETA, SC_FROZEN, SC_ROWS };      // the per-column scalars: SC_ROWS rows of K words
enum { SCAL_INIT = 0, SCAL_ALPHA, SCAL_BETA };

inline int cov_grid(int C_) { return C_ > THALLO_MAX_PARTIALS ? THALLO_MAX_PARTIALS : C_; }

// V[a][m] = sum over l >= m of W[a][l] G[l][m] for one row a of W (w: its three floats) -- no dynamic index
__device__ __forceinline__ float v_of(const float (&w)[3], const float (&g)[6], int m)
{
    const float v0 = w[0] * g[tri(0, 0)] + w[1] * g[tri(1, 0)] + w[2] * g[tri(2, 0)];
    const float v1 = w[1] * g[tri(1, 1)] + w[2] * g[tri(2, 1)];
    const float v2 = w[2] * g[tri(2, 2)];
    return m == 0 ? v0 : m == 1 ? v1 : v2;
}
// G[l][m] of the packed lower triangle, 0 above the diagonal
__device__ __forceinline__ float g_at(const float (&g)[6], int l, int m)
{
    float v = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) if (l == i && m == j) v = g[tri(i, j)];
    return v;
}

__global__ __launch_bounds__(K) void k_cov_rhs(int C_, int P_, int mode, int nreq, const int* __restrict__ ids, const int* __restrict__ pt_ptr, const int* __restrict__ pt_pos,
                                               const int* __restrict__ q_cam, const float* __restrict__ W, const float* __restrict__ Ge, float* __restrict__ R)
{
    const int k = threadIdx.x;
    if (mode == 0) {
        const int j = k / 9, a = k - 9 * j;
        if (j < nreq) R[(9L * ids[j] + a) * K + k] = 1.0f;
        return;
    }
    const int j = k / 3, m = k - 3 * j;
    if (j >= nreq) return;
    const int p = ids[j];
    float g[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) g[i] = Ge[(long)i * P_ + p];
    for (int t = pt_ptr[p]; t < pt_ptr[p + 1]; ++t) {
        const int q = pt_pos[t], c = q_cam[q];
        const float* w = W + (long)WS * q;
#pragma unroll
        for (int a = 0; a < 9; ++a) {
            const float wa[3] = { w[3 * a], w[3 * a + 1], w[3 * a + 2] };
            R[(9L * c + a) * K + k] += v_of(wa, g, m);      // (a camera that sees the point twice: both, in list order)
        }
    }
}

__global__ __launch_bounds__(K) void k_apply_s_cols(int C_, long nblk, const int* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ S,
                                                    const float* __restrict__ X, float* __restrict__ Y, float* __restrict__ part)
{
    __shared__ float sm[CH * LS];
    __shared__ int cs[CH];
    const int lane = threadIdx.x, blk = lane & (CH - 1), e0 = (lane >> 5) * HALF;
    float acc = 0.0f;
    for (int c = blockIdx.x; c < C_; c += gridDim.x) {
        float y[9];
#pragma unroll
        for (int a = 0; a < 9; ++a) y[a] = 0.0f;
        const int t1 = row_ptr[c + 1];
        for (int t0 = row_ptr[c]; t0 < t1; t0 += CH) {
            const int n = min(CH, t1 - t0);
            __syncthreads();                                  // the chunk before has been read
            if (blk < n) {
                const float* s = S + t0 + blk;
                float m[HALF];
#pragma unroll
                for (int i = 0; i < HALF; ++i) m[i] = e0 + i < 81 ? s[(long)(e0 + i) * nblk] : 0.0f;
#pragma unroll
                for (int i = 0; i < HALF; ++i) if (e0 + i < 81) sm[blk * LS + e0 + i] = m[i];
                if (lane < CH) cs[blk] = col[t0 + blk];
            }
            __syncthreads();
            for (int j = 0; j < n; ++j) {
                const float* xj = X + 9L * cs[j] * K + lane;
                const float* mj = sm + j * LS;
                float xv[9];
#pragma unroll
                for (int b = 0; b < 9; ++b) xv[b] = xj[(long)b * K];
#pragma unroll
                for (int a = 0; a < 9; ++a)
#pragma unroll
                    for (int b = 0; b < 9; ++b) y[a] += mj[9 * a + b] * xv[b];
            }
        }
        const long base = 9L * c * K + lane;
#pragma unroll
        for (int a = 0; a < 9; ++a) { Y[base + (long)a * K] = y[a]; acc += X[base + (long)a * K] * y[a]; }
    }
    part[(long)blockIdx.x * K + lane] = acc;
}

// UPDATE: X += alpha P, R -= alpha Y first (the column's alpha; a frozen column is left alone and leaves a zero partial).  Then Z = G^T G R and the partials of r . z
template <bool UPDATE>
__global__ __launch_bounds__(K) void k_cov_step(int C_, const float* __restrict__ Gc, float* __restrict__ X, const float* __restrict__ P, float* __restrict__ R,
                                                const float* __restrict__ Y, float* __restrict__ Z, const float* __restrict__ sc, float* __restrict__ part)
{
    const int lane = threadIdx.x;
    const float alpha = UPDATE ? sc[SC_ALPHA * K + lane] : 0.0f;
    const bool live = UPDATE ? reinterpret_cast<const unsigned*>(sc)[SC_FROZEN * K + lane] == 0u : true;
    float acc = 0.0f;
    for (int c = blockIdx.x; c < C_; c += gridDim.x) {
        float g[tri_n(9)];
#pragma unroll
        for (int k = 0; k < tri_n(9); ++k) g[k] = Gc[(long)k * C_ + c];
        if (!live) continue;
        const long base = 9L * c * K + lane;
        float r[9], z[9];
#pragma unroll
        for (int a = 0; a < 9; ++a) {
            const long i = base + (long)a * K;
            r[a] = R[i];
            if (UPDATE) { X[i] += alpha * P[i]; r[a] -= alpha * Y[i]; R[i] = r[a]; }
        }
        apply_g<9>(g, r, z);
#pragma unroll
        for (int a = 0; a < 9; ++a) { Z[base + (long)a * K] = z[a]; acc += r[a] * z[a]; }
    }
    part[(long)blockIdx.x * K + lane] = acc;
}

// One workgroup of four waves: wave v adds its quarter of the slot's partials per column in ascending order, then ((s0 + s1) + s2) + s3
template <int MODE>
__global__ __launch_bounds__(4 * K) void k_cov_scal(int nparts, const float* __restrict__ part, float* __restrict__ sc, float tol2, unsigned* __restrict__ count)
{
    __shared__ float red[4 * K];
    const int lane = threadIdx.x & (K - 1), wave = threadIdx.x / K;
    const int per = (nparts + 3) / 4, w0 = wave * per, w1 = min(nparts, w0 + per);
    float s = 0.0f;
#pragma unroll 8
    for (int w = w0; w < w1; ++w) s += part[(long)w * K + lane];
    red[wave * K + lane] = s;
    __syncthreads();
    if (wave != 0) return;
    s = ((red[lane] + red[K + lane]) + red[2 * K + lane]) + red[3 * K + lane];
    unsigned* fz = reinterpret_cast<unsigned*>(sc) + SC_FROZEN * K + lane;
    if (MODE == SCAL_INIT) {
        sc[SC_AN * K + lane] = s; sc[SC_R0 * K + lane] = s; sc[SC_ALPHA * K + lane] = 0.0f; sc[SC_BETA * K + lane] = 0.0f;
        *fz = s <= tol2 * s ? 1u : 0u;                        // (a zero right-hand side -- an unused column, a held scalar's -- is frozen at once and stays zero)
    } else if (MODE == SCAL_ALPHA) {
        float a = 0.0f;
        if (*fz == 0u && s > 0.0f) a = sc[SC_AN * K + lane] / s;
        sc[SC_ALPHA * K + lane] = a;
    } else {
        float b = 0.0f;
        if (*fz == 0u) {
            const float aN = sc[SC_AN * K + lane];
            if (aN > 0.0f) b = s / aN;
            sc[SC_AN * K + lane] = s;
            if (s <= tol2 * sc[SC_R0 * K + lane]) *fz = 1u;
        }
        sc[SC_BETA * K + lane] = b;
    }
    if (MODE != SCAL_ALPHA) {
        const unsigned long long m = __ballot(*fz != 0u);
        if (lane == 0) count[0] = (unsigned)__popcll(m);
    }
}

__global__ __launch_bounds__(256) void k_cov_pupdate(long n, const float* __restrict__ Z, float* __restrict__ P, const float* __restrict__ sc, int first)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        P[i] = first ? Z[i] : Z[i] + sc[SC_BETA * K + (int)(i & (K - 1))] * P[i];
}

__global__ __launch_bounds__(256) void k_cov_out(int C_, int P_, int mode, int nreq, const int* __restrict__ ids, const int* __restrict__ pt_ptr, const int* __restrict__ pt_pos,
                                                 const int* __restrict__ q_cam, const float* __restrict__ W, const float* __restrict__ Ge, const unsigned char* __restrict__ hold,
                                                 const float* __restrict__ X, float* __restrict__ out, unsigned* __restrict__ nan_count)
{
    const int per = mode == 0 ? 81 : 9;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < nreq * per; t += gridDim.x * 256) {
        const int j = t / per, e = t - per * j;
        if (mode == 0) {
            const int a = e / 9, b = e - 9 * a;
            const long c = ids[j];
            out[t] = 0.5f * (X[(9 * c + a) * K + 9 * j + b] + X[(9 * c + b) * K + 9 * j + a]);
            continue;
        }
        const int m = e / 3, n = e - 3 * m, p = ids[j];
        float g[6];
        bool zero = true;
#pragma unroll
        for (int i = 0; i < 6; ++i) { g[i] = Ge[(long)i * P_ + p]; zero = zero && g[i] == 0.0f; }
        if (zero) {      // G = 0: the caller holds the whole point (zeros), or the factor rule held it (no finite covariance)
            const unsigned char* h = hold ? hold + 9L * C_ + 3L * p : nullptr;
            const bool callers = h && h[0] && h[1] && h[2];
            out[t] = callers ? 0.0f : __builtin_nanf("");
            if (!callers && e == 0) atomicAdd(nan_count, 1u);
            continue;
        }
        float amn = 0.0f, anm = 0.0f;
        for (int u = pt_ptr[p]; u < pt_ptr[p + 1]; ++u) {
            const int q = pt_pos[u];
            const long c = q_cam[q];
            const float* w = W + (long)WS * q;
#pragma unroll
            for (int a = 0; a < 9; ++a) {
                const float wa[3] = { w[3 * a], w[3 * a + 1], w[3 * a + 2] };
                const float* x = X + (9 * c + a) * K + 3 * j;
                amn += v_of(wa, g, m) * x[n];
                anm += v_of(wa, g, n) * x[m];
            }
        }
        float gtg = 0.0f;
#pragma unroll
        for (int l = 0; l < 3; ++l) gtg += g_at(g, l, m) * g_at(g, l, n);
        out[t] = 0.5f * ((gtg + amn) + (gtg + anm));
    }
}

struct Work { float *X, *R, *P, *Z, *Y, *pa, *pb, *sc; unsigned* words; };
inline long panel_floats(int C_) { return 9L * C_ * K; }
inline Work carve(void* work, int C_)
{
    Work w; float* f = (float*)work; const long pn = panel_floats(C_), gn = (long)cov_grid(C_) * K;
    w.X = f; w.R = f + pn; w.P = f + 2 * pn; w.Z = f + 3 * pn; w.Y = f + 4 * pn; w.pa = f + 5 * pn; w.pb = w.pa + gn; w.sc = w.pb + gn;
    w.words = reinterpret_cast<unsigned*>(w.sc + (long)SC_ROWS * K);
    return w;
}
inline bool sys_ok(const thallo_cov_sys_t* s)
{
    return s && s->C >= 1 && s->P >= 0 && s->nblk >= s->C && s->row_ptr && s->col && s->S && s->Gc;
}
inline bool points_ok(const thallo_cov_sys_t* s) { return s->Ge && s->W && s->pt_ptr && s->pt_pos && s->q_cam; }
inline int max_requests(int mode) { return mode == 0 ? K / 9 : K / 3; }

}  // namespace

extern "C" {

long thallo_hip_ba_cov_work_bytes(int C_)
{
    if (C_ < 1) return -1;
    return (5 * panel_floats(C_) + 2L * cov_grid(C_) * K + (long)SC_ROWS * K + 64) * (long)sizeof(float);
}

int thallo_hip_ba_cov_rhs(const thallo_cov_sys_t* sys, int mode, const int* ids, int nreq, float* R, thallo_stream_t stream)
{
    if (!sys_ok(sys) || (mode != 0 && mode != 1) || !ids || nreq < 1 || nreq > max_requests(mode) || !R || (mode == 1 && !points_ok(sys))) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t me = hipMemsetAsync(R, 0, sizeof(float) * (size_t)panel_floats(sys->C), s);
    if (me != hipSuccess) return -(int)me;
    hipLaunchKernelGGL(k_cov_rhs, dim3(1), dim3(K), 0, s, sys->C, sys->P, mode, nreq, ids, sys->pt_ptr, sys->pt_pos, sys->q_cam, sys->W, sys->Ge, R);
    return check_launch();
}

int thallo_hip_ba_schur_apply_s_cols(int C_, long nblk, const int* row_ptr, const int* col, const float* S, const float* X, float* Y, float* xSx_out, thallo_stream_t stream)
{
    if (C_ < 1 || nblk < C_ || !row_ptr || !col || !S || !X || !Y || !xSx_out) return -(int)hipErrorInvalidValue;
    const int g = cov_grid(C_);
    hipLaunchKernelGGL(k_apply_s_cols, dim3(g), dim3(K), 0, (hipStream_t)stream, C_, nblk, row_ptr, col, S, X, Y, xSx_out);
    const int e = check_launch(); return e ? e : g;
}

int thallo_hip_ba_cov_precond_cols(int C_, const float* Gc, const float* R, float* Z, float* rz_out, thallo_stream_t stream)
{
    if (C_ < 1 || !Gc || !R || !Z || !rz_out) return -(int)hipErrorInvalidValue;
    const int g = cov_grid(C_);
    hipLaunchKernelGGL(k_cov_step<false>, dim3(g), dim3(K), 0, (hipStream_t)stream, C_, Gc, (float*)nullptr, (const float*)nullptr, const_cast<float*>(R), (const float*)nullptr, Z,
                       (const float*)nullptr, rz_out);
    const int e = check_launch(); return e ? e : g;
}

int thallo_hip_ba_cov_out(const thallo_cov_sys_t* sys, int mode, const int* ids, int nreq, const float* X, float* out, unsigned* nan_count, thallo_stream_t stream)
{
    if (!sys_ok(sys) || (mode != 0 && mode != 1) || !ids || nreq < 1 || nreq > max_requests(mode) || !X || !out || !nan_count || (mode == 1 && !points_ok(sys)))
        return -(int)hipErrorInvalidValue;
    const int n = nreq * (mode == 0 ? 81 : 9);
    hipLaunchKernelGGL(k_cov_out, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, sys->C, sys->P, mode, nreq, ids, sys->pt_ptr, sys->pt_pos, sys->q_cam, sys->W, sys->Ge,
                       sys->hold, X, out, nan_count);
    return check_launch();
}

int thallo_hip_ba_cov_solve(const thallo_cov_sys_t* sys, int mode, const int* ids, int nreq, float rel_tol, int max_iterations, void* work, unsigned* pinned, float* out,
                            thallo_cov_info_t* info, thallo_stream_t stream)
{
    if (!sys_ok(sys) || (mode != 0 && mode != 1) || !ids || nreq < 1 || nreq > max_requests(mode) || !work || !out || !info || max_iterations < 1 || !(rel_tol > 0.0f) ||
        !std::isfinite(rel_tol) || (mode == 1 && !points_ok(sys))) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const int C_ = sys->C, g = cov_grid(C_);
    const long pn = panel_floats(C_);
    const Work w = carve(work, C_);
    const float tol2 = rel_tol * rel_tol;
    hipError_t he;
    auto bad = [&](hipError_t e) { return -(int)e; };
    if ((he = hipMemsetAsync(w.X, 0, sizeof(float) * (size_t)pn, s)) != hipSuccess) return bad(he);
    if ((he = hipMemsetAsync(w.words, 0, 4 * sizeof(unsigned), s)) != hipSuccess) return bad(he);      // word 0: the frozen columns; word 1: blocks filled with NaN
    int rc;
    if ((rc = thallo_hip_ba_cov_rhs(sys, mode, ids, nreq, w.R, stream)) < 0) return rc;
    if ((rc = thallo_hip_ba_cov_precond_cols(C_, sys->Gc, w.R, w.Z, w.pb, stream)) < 0) return rc;
    hipLaunchKernelGGL(k_cov_scal<SCAL_INIT>, dim3(1), dim3(4 * K), 0, s, g, w.pb, w.sc, tol2, w.words);
    if ((rc = check_launch()) < 0) return rc;
    // the iterations, THALLO_HIP_COV_CHUNK at a time; behind every chunk the frozen count goes to the host, which reads the chunk before it while this one runs
    hipEvent_t ev[2] = { nullptr, nullptr };
    if (pinned) for (int i = 0; i < 2; ++i) if ((he = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming)) != hipSuccess) { if (ev[0]) (void)hipEventDestroy(ev[0]); return bad(he); }
    auto done = [&](int code) { for (int i = 0; i < 2; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]); return code; };
    const int pgrid = (int)((pn + 255) / 256 > 2048 ? 2048 : (pn + 255) / 256);
    int it = 0, chunk = 0;
    unsigned frozen_host = 0;
    bool all_frozen = false;
    while (it < max_iterations && !all_frozen) {
        const int n = max_iterations - it < THALLO_HIP_COV_CHUNK ? max_iterations - it : THALLO_HIP_COV_CHUNK;
        for (int i = 0; i < n; ++i, ++it) {
            hipLaunchKernelGGL(k_cov_pupdate, dim3(pgrid), dim3(256), 0, s, pn, w.Z, w.P, w.sc, it == 0 ? 1 : 0);
            hipLaunchKernelGGL(k_apply_s_cols, dim3(g), dim3(K), 0, s, C_, sys->nblk, sys->row_ptr, sys->col, sys->S, w.P, w.Y, w.pa);
            hipLaunchKernelGGL(k_cov_scal<SCAL_ALPHA>, dim3(1), dim3(4 * K), 0, s, g, w.pa, w.sc, tol2, w.words);
            hipLaunchKernelGGL(k_cov_step<true>, dim3(g), dim3(K), 0, s, C_, sys->Gc, w.X, w.P, w.R, w.Y, w.Z, w.sc, w.pb);
            hipLaunchKernelGGL(k_cov_scal<SCAL_BETA>, dim3(1), dim3(4 * K), 0, s, g, w.pb, w.sc, tol2, w.words);
        }
        if ((rc = check_launch()) < 0) return done(rc);
        if (!pinned) {      // no pinned words: a blocking read per chunk
            if ((he = hipMemcpyAsync(&frozen_host, w.words, sizeof(unsigned), hipMemcpyDeviceToHost, s)) != hipSuccess || (he = hipStreamSynchronize(s)) != hipSuccess) return done(bad(he));
            all_frozen = frozen_host == (unsigned)K;
        } else {
            const int slot = chunk & 1;
            if ((he = hipMemcpyAsync(pinned + slot, w.words, sizeof(unsigned), hipMemcpyDeviceToHost, s)) != hipSuccess || (he = hipEventRecord(ev[slot], s)) != hipSuccess) return done(bad(he));
            if (chunk > 0) {
                if ((he = hipEventSynchronize(ev[slot ^ 1])) != hipSuccess) return done(bad(he));
                all_frozen = pinned[slot ^ 1] == (unsigned)K;
            }
        }
        ++chunk;
    }
    if ((rc = thallo_hip_ba_cov_out(sys, mode, ids, nreq, w.X, out, w.words + 1, stream)) < 0) return done(rc);
    float sc[SC_ROWS * K]; unsigned words[2] = { 0, 0 };
    if ((he = hipMemcpyAsync(sc, w.sc, sizeof(sc), hipMemcpyDeviceToHost, s)) != hipSuccess || (he = hipMemcpyAsync(words, w.words, sizeof(words), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (he = hipStreamSynchronize(s)) != hipSuccess) return done(bad(he));
    info->iterations = it; info->columns = 0; info->not_converged = 0; info->nan_blocks = (int)words[1]; info->worst = 0.0f;
    const unsigned* fz = reinterpret_cast<const unsigned*>(sc) + SC_FROZEN * K;
    for (int k = 0; k < nreq * (mode == 0 ? 9 : 3); ++k) {
        const float r0 = sc[SC_R0 * K + k], rz = sc[SC_AN * K + k];
        if (!(r0 > 0.0f) && !std::isnan(r0)) continue;      // a zero right-hand side: nothing to solve
        info->columns++;
        if (!fz[k]) info->not_converged++;
        const float rel = std::sqrt(rz / r0);
        if (!(rel <= info->worst)) info->worst = rel;        // (a NaN shows)
    }
    return done(0);
}

// ------------------------------------------------------------------ the same batch under the two-level preconditioner (ba_coarse.hip)
// The work buffer: thallo_hip_ba_cov_solve's, then the slot of r . z with room for the coarse partials behind the block term's, then the coarse panels r_c and Y
long thallo_hip_ba_cov_coarse_work_bytes(int C_, long n)
{
    const long base = thallo_hip_ba_cov_work_bytes(C_);
    if (base < 0 || n < 0) return -1;
    if (n == 0) return base;
    const long cw = thallo_hip_ba_coarse_cols_work_floats(n);
    return cw < 0 ? -1 : base + (((long)cov_grid(C_) + THALLO_HIP_COARSE_COLS_PARTIALS) * K + cw + 64) * (long)sizeof(float);
}

int thallo_hip_ba_cov_solve_coarse(const thallo_cov_sys_t* sys, const thallo_coarse_t* coarse, int mode, const int* ids, int nreq, float rel_tol, int max_iterations, void* work,
                                   unsigned* pinned, float* out, thallo_cov_info_t* info, thallo_stream_t stream)
{
    if (!coarse) return thallo_hip_ba_cov_solve(sys, mode, ids, nreq, rel_tol, max_iterations, work, pinned, out, info, stream);
    if (!sys_ok(sys) || (mode != 0 && mode != 1) || !ids || nreq < 1 || nreq > max_requests(mode) || !work || !out || !info || max_iterations < 1 || !(rel_tol > 0.0f) ||
        !std::isfinite(rel_tol) || (mode == 1 && !points_ok(sys)) || coarse->C != sys->C) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const int C_ = sys->C, g = cov_grid(C_);
    const long pn = panel_floats(C_);
    const Work w = carve(work, C_);
    float* pb2 = reinterpret_cast<float*>(static_cast<char*>(work) + thallo_hip_ba_cov_work_bytes(C_));      // the slot of r . z: g partials of the block term, then the coarse term's
    float* cwork = pb2 + ((long)g + THALLO_HIP_COARSE_COLS_PARTIALS) * K;
    const unsigned* frozen = reinterpret_cast<const unsigned*>(w.sc) + SC_FROZEN * K;
    const float tol2 = rel_tol * rel_tol;
    hipError_t he;
    auto bad = [&](hipError_t e) { return -(int)e; };
    if ((he = hipMemsetAsync(w.X, 0, sizeof(float) * (size_t)pn, s)) != hipSuccess) return bad(he);
    if ((he = hipMemsetAsync(w.words, 0, 4 * sizeof(unsigned), s)) != hipSuccess) return bad(he);
    int rc, gc;
    if ((rc = thallo_hip_ba_cov_rhs(sys, mode, ids, nreq, w.R, stream)) < 0) return rc;
    if ((rc = thallo_hip_ba_cov_precond_cols(C_, sys->Gc, w.R, w.Z, pb2, stream)) < 0) return rc;
    if ((gc = thallo_hip_ba_coarse_apply_cols(coarse, cwork, w.R, w.Z, nullptr, pb2 + (long)g * K, stream)) < 0) return gc;
    hipLaunchKernelGGL(k_cov_scal<SCAL_INIT>, dim3(1), dim3(4 * K), 0, s, g + gc, pb2, w.sc, tol2, w.words);
    if ((rc = check_launch()) < 0) return rc;
    hipEvent_t ev[2] = { nullptr, nullptr };
    if (pinned) for (int i = 0; i < 2; ++i) if ((he = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming)) != hipSuccess) { if (ev[0]) (void)hipEventDestroy(ev[0]); return bad(he); }
    auto done = [&](int code) { for (int i = 0; i < 2; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]); return code; };
    const int pgrid = (int)((pn + 255) / 256 > 2048 ? 2048 : (pn + 255) / 256);
    int it = 0, chunk = 0;
    unsigned frozen_host = 0;
    bool all_frozen = false;
    while (it < max_iterations && !all_frozen) {
        const int n = max_iterations - it < THALLO_HIP_COV_CHUNK ? max_iterations - it : THALLO_HIP_COV_CHUNK;
        for (int i = 0; i < n; ++i, ++it) {
            hipLaunchKernelGGL(k_cov_pupdate, dim3(pgrid), dim3(256), 0, s, pn, w.Z, w.P, w.sc, it == 0 ? 1 : 0);
            hipLaunchKernelGGL(k_apply_s_cols, dim3(g), dim3(K), 0, s, C_, sys->nblk, sys->row_ptr, sys->col, sys->S, w.P, w.Y, w.pa);
            hipLaunchKernelGGL(k_cov_scal<SCAL_ALPHA>, dim3(1), dim3(4 * K), 0, s, g, w.pa, w.sc, tol2, w.words);
            hipLaunchKernelGGL(k_cov_step<true>, dim3(g), dim3(K), 0, s, C_, sys->Gc, w.X, w.P, w.R, w.Y, w.Z, w.sc, pb2);
            if ((rc = thallo_hip_ba_coarse_apply_cols(coarse, cwork, w.R, w.Z, frozen, pb2 + (long)g * K, stream)) < 0) return done(rc);
            hipLaunchKernelGGL(k_cov_scal<SCAL_BETA>, dim3(1), dim3(4 * K), 0, s, g + gc, pb2, w.sc, tol2, w.words);
        }
        if ((rc = check_launch()) < 0) return done(rc);
        if (!pinned) {
            if ((he = hipMemcpyAsync(&frozen_host, w.words, sizeof(unsigned), hipMemcpyDeviceToHost, s)) != hipSuccess || (he = hipStreamSynchronize(s)) != hipSuccess) return done(bad(he));
            all_frozen = frozen_host == (unsigned)K;
        } else {
            const int slot = chunk & 1;
            if ((he = hipMemcpyAsync(pinned + slot, w.words, sizeof(unsigned), hipMemcpyDeviceToHost, s)) != hipSuccess || (he = hipEventRecord(ev[slot], s)) != hipSuccess) return done(bad(he));
            if (chunk > 0) {
                if ((he = hipEventSynchronize(ev[slot ^ 1])) != hipSuccess) return done(bad(he));
                all_frozen = pinned[slot ^ 1] == (unsigned)K;
            }
        }
        ++chunk;
    }
    if ((rc = thallo_hip_ba_cov_out(sys, mode, ids, nreq, w.X, out, w.words + 1, stream)) < 0) return done(rc);
    float sc[SC_ROWS * K]; unsigned words[2] = { 0, 0 };
    if ((he = hipMemcpyAsync(sc, w.sc, sizeof(sc), hipMemcpyDeviceToHost, s)) != hipSuccess || (he = hipMemcpyAsync(words, w.words, sizeof(words), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (he = hipStreamSynchronize(s)) != hipSuccess) return done(bad(he));
    info->iterations = it; info->columns = 0; info->not_converged = 0; info->nan_blocks = (int)words[1]; info->worst = 0.0f;
    const unsigned* fz = reinterpret_cast<const unsigned*>(sc) + SC_FROZEN * K;
    for (int k = 0; k < nreq * (mode == 0 ? 9 : 3); ++k) {
        const float r0 = sc[SC_R0 * K + k], rz = sc[SC_AN * K + k];
        if (!(r0 > 0.0f) && !std::isnan(r0)) continue;
        info->columns++;
        if (!fz[k]) info->not_converged++;
        const float rel = std::sqrt(rz / r0);
        if (!(rel <= info->worst)) info->worst = rel;
    }
    return done(0);
}

}  // extern "C"
