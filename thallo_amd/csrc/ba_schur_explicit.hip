// ba_schur_explicit.hip -- the ASSEMBLED reduced camera matrix of bundle adjustment's Schur-complement solve (DESIGN.md "Assembled reduced camera matrix";
// ThalloX_PlanSetLinearSolver THALLOX_SOLVER_SCHUR_EXPLICIT_PCG).  Everything but the application of S is ba_schur.hip's.  Once per step
//
//   S_ij = [i = j] (B_ii + diag CtC_c,i) - sum over the terms (q, q') of block (i, j) of W_q W_q'^T,      W_q = (J_c,q^T J_p,q) G_p^T  (9 x 3)
//
// is formed as a block-sparse matrix over the co-visible camera pairs (E Cp^-1 E^T = sum over the points of (E_q G^T) (E_q' G^T)^T with Cp^-1 = G^T G; a held point has
// G = 0, so W = 0 and it contributes no coupling), and every S x of the PCG loop is one block-sparse mat-vec on 9 C floats.
//
//   schur_w         one thread per observation (camera order): E = J_c^T J_p summed over the two residual rows from the 24 floats of Jb (ba_blocks.hpp), W = E G^T.  W is stored
//                   observation-major, 27 floats at a stride of 32 (one 128-byte line per observation, seven 16-byte stores): the assembly's wave reads the W of ONE
//                   observation pair per term, every lane a few words of the same two lines, so a term costs two lines whatever the lane's entry is.  (Entry-major planes
//                   would make this launch's stores coalesced and every load of the assembly a line of its own.)
//   schur_assemble  one wave per lower-triangle block, lanes as the 81 entries (lanes 0 .. 16 carry entries 64 .. 80 as well), walking the block's terms in the list's
//                   order, four terms per trip with every load of the trip in flight before the first use and the additions one term after the other: one fixed order per
//                   block, no atomics.  The term list and the block's places are wave-uniform (scalar loads).  A diagonal block's lanes compute
//                   entry (max(a, b), min(a, b)), so the stored block is symmetric bit for bit; an off-diagonal block's lane writes its entry and the transpose's.
//                   B_ii: the 45 floats thallo_hip_ba_block_diag left in H; CtC is added here (the apply adds nothing).
//   schur_apply_s   one wave per camera row, one lane per stored block of the row (rows longer than 64 blocks: a second trip), 81 loads per lane from the entry-major
//                   planes S[e * nblk + blk] -- consecutive lanes read consecutive words --, nine sums per lane, the wave butterfly, lanes 0 .. 8 store.  Gated.
// Nothing is indexed dynamically, every loop over a block is unrolled.  Sums: one partial per workgroup, fixed order, no float atomics.
#include "device_common.hpp"
#include "block_regions.hpp"      // tri
#include "ba_blocks.hpp"
#include "../../include/thallo_hip.h"

using namespace thallo;
using thallo::launch::check_launch;

namespace {

constexpr int BLOCK = BA_WG;
constexpr int WSTRIDE = THALLO_HIP_SCHUR_W_STRIDE;
inline int wave_grid(long n) { long g = (n + 3) / 4; if (g > 65536) g = 65536; return g < 1 ? 1 : (int)g; }

__global__ __launch_bounds__(BLOCK) void k_schur_w(int O_, int P_, const int* __restrict__ q_pt, const float4* __restrict__ Jb, const float* __restrict__ G, float4* __restrict__ W)
{
    for (int q = blockIdx.x * BLOCK + threadIdx.x; q < O_; q += gridDim.x * BLOCK) {
        const Blk b = ld_blk(Jb, q);
        const int j = q_pt[q];
        float g[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = G[(long)k * P_ + j];
        float w[28];
#pragma unroll
        for (int a = 0; a < 9; ++a) {
            float e[3];
#pragma unroll
            for (int n = 0; n < 3; ++n) e[n] = b.a[a] * b.a[BA_NC + n] + b.a[BA_ROW + a] * b.a[BA_ROW + BA_NC + n];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                float s = 0.0f;
#pragma unroll
                for (int n = 0; n <= m; ++n) s += e[n] * g[tri(m, n)];
                w[3 * a + m] = s;
            }
        }
        w[27] = 0.0f;
        float4* dst = W + (long)(WSTRIDE / 4) * q;
#pragma unroll
        for (int k = 0; k < 7; ++k) dst[k] = make_float4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    }
}

// One trip of the term walk: the words of four terms (the last trip's spare places repeat the block's last term and are not added) for the lane's two entries, all loads
// in flight before the first use; added one term after the other, so the order of the additions is the list's whatever the trip length
constexpr int TRIP = 4;

__global__ __launch_bounds__(BLOCK) void k_schur_assemble(int C_, int nlower, long nblk, const int* __restrict__ lower, const int* __restrict__ term_ptr, const int2* __restrict__ terms,
                                                          const float* __restrict__ W, const float* __restrict__ H, const float* __restrict__ ctc, float* __restrict__ S)
{
    const int lane = threadIdx.x & 63;
    const int e2 = lane < 17 ? lane + 64 : lane;      // lanes 0 .. 16 carry entries 64 .. 80 as well (the others repeat their own and do not store it twice)
    for (int l0 = blockIdx.x * 4 + (threadIdx.x >> 6); l0 < nlower; l0 += gridDim.x * 4) {
        const int l = __builtin_amdgcn_readfirstlane(l0);
        const int bij = lower[3 * l], bji = lower[3 * l + 1], dc = lower[3 * l + 2];      // the places of (i, j) and (j, i) among the stored blocks; the camera of a diagonal block, else -1
        const int t0 = term_ptr[l], t1 = term_ptr[l + 1];
        const bool diag = dc >= 0;
        int a[2] = { lane / 9, e2 / 9 }, b[2] = { lane - 9 * (lane / 9), e2 - 9 * (e2 / 9) };
        const int ea[2] = { a[0], a[1] }, eb[2] = { b[0], b[1] };
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (diag && a[h] < b[h]) { const int t = a[h]; a[h] = b[h]; b[h] = t; }      // the lower triangle's sum for both entries of a diagonal block
        float acc[2] = { 0.0f, 0.0f };
        for (int t = t0; t < t1; t += TRIP) {
            float x[TRIP][2][3], y[TRIP][2][3];
#pragma unroll
            for (int u = 0; u < TRIP; ++u) {
                const int2 qq = terms[min(t + u, t1 - 1)];      // (wave-uniform)
                const float* wa = W + (long)WSTRIDE * qq.x;
                const float* wb = W + (long)WSTRIDE * qq.y;
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int m = 0; m < 3; ++m) { x[u][h][m] = wa[3 * a[h] + m]; y[u][h][m] = wb[3 * b[h] + m]; }
            }
#pragma unroll
            for (int u = 0; u < TRIP; ++u)
                if (t + u < t1) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) acc[h] += x[u][h][0] * y[u][h][0] + x[u][h][1] * y[u][h][1] + x[u][h][2] * y[u][h][2];
                }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && lane >= 17) continue;
            const int e = h ? e2 : lane;
            float base = 0.0f;
            if (diag) {
                base = H[(long)tri(a[h], b[h]) * C_ + dc];
                if (a[h] == b[h] && ctc != nullptr) base += ctc[9L * dc + a[h]];
            }
            const float v = base - acc[h];
            S[(long)e * nblk + bij] = v;
            if (!diag) S[(long)(9 * eb[h] + ea[h]) * nblk + bji] = v;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_schur_apply_s(int C_, long nblk, const int* __restrict__ row_ptr, const int* __restrict__ col, const float* __restrict__ S,
                                                         const float* __restrict__ x, float* __restrict__ Sx, float* __restrict__ part_out, const unsigned* __restrict__ gate)
{
    __shared__ float red[16];
    if (gate != nullptr && __builtin_amdgcn_readfirstlane((int)gate[0]) != 0) return;      // LM: the PCG loop already ended on the device
    float acc = 0.0f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = blockIdx.x * 4 + wave; c < C_; c += gridDim.x * 4) {
        float y[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) y[k] = 0.0f;
        const float e_x = x[9L * c + (lane < 9 ? lane : 8)];      // the epilogue's word, asked for before the blocks
        const int t1 = row_ptr[c + 1];
        for (int t = row_ptr[c] + lane; t < t1; t += 64) {
            const float* xj = x + 9L * col[t];
            const float* s = S + t;
            float m[81], xv[9];
#pragma unroll
            for (int e = 0; e < 81; ++e) m[e] = s[(long)e * nblk];
#pragma unroll
            for (int k = 0; k < 9; ++k) xv[k] = xj[k];
#pragma unroll
            for (int a = 0; a < 9; ++a)
#pragma unroll
                for (int b = 0; b < 9; ++b) y[a] += m[9 * a + b] * xv[b];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) y[k] = wave_sum_all(y[k]);
        if (lane < 9) {
            float sv = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) if (lane == k) sv = y[k];
            Sx[9L * c + lane] = sv;
            acc += e_x * sv;
        }
    }
    block_store_partial(acc, part_out, red);
}

}  // namespace

extern "C" {

int thallo_hip_ba_schur_w(int O_, int P_, const int* q_pt, const float* Jb, const float* G, float* W, thallo_stream_t stream)
{
    if (O_ < 0 || P_ < 0 || !q_pt || !Jb || !G || !W) return -(int)hipErrorInvalidValue;
    if (O_ < 1) return 0;
    int g = (O_ + BLOCK - 1) / BLOCK; if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_schur_w, dim3(g), dim3(BLOCK), 0, (hipStream_t)stream, O_, P_, q_pt, (const float4*)Jb, G, (float4*)W);
    return check_launch();
}

int thallo_hip_ba_schur_assemble(int C_, int nlower, long nblk, const int* lower, const int* term_ptr, const int* terms, const float* W, const float* H, const float* ctc, float* S,
                                 thallo_stream_t stream)
{
    if (C_ < 1 || nlower < C_ || nblk < nlower || nblk > 2L * nlower || !lower || !term_ptr || !terms || !W || !H || !S) return -(int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_schur_assemble, dim3(wave_grid(nlower)), dim3(BLOCK), 0, (hipStream_t)stream, C_, nlower, nblk, lower, term_ptr, (const int2*)terms, W, H, ctc, S);
    return check_launch();
}

int thallo_hip_ba_schur_apply_s(int C_, long nblk, const int* row_ptr, const int* col, const float* S, const float* x, float* Sx, float* xSx_out, const unsigned* gate,
                                thallo_stream_t stream)
{
    if (C_ < 1 || nblk < C_ || !row_ptr || !col || !S || !x || !Sx || !xSx_out) return -(int)hipErrorInvalidValue;
    const int cb = ba_cam_grid(C_);
    hipLaunchKernelGGL(k_schur_apply_s, dim3(cb), dim3(BLOCK), 0, (hipStream_t)stream, C_, nblk, row_ptr, col, S, x, Sx, xSx_out, gate);
    const int e = check_launch(); return e ? e : cb;
}

}  // extern "C"
