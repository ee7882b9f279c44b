// ba_schur.hip -- the opt-in Schur-complement solve of bundle adjustment (DESIGN.md "Schur complement on the cameras"; ThalloX_PlanSetLinearSolver).
// With A = J^T J (+ diag(CtC) in LM) = [[B, E], [E^T, Cp]] over [cameras | points] and b = -J^T F = [b_c; b_p], the points are eliminated exactly through their 3 x 3
// blocks Cp and PCG runs on the cameras only:  S = B - E Cp^-1 E^T,  g = b_c - E Cp^-1 b_p,  S delta_c = g,  delta_p = Cp^-1 (b_p - E^T delta_c).
//
//   schur_factor  Cp^-1 = G^T G per point: block_chol.hpp's scaled Cholesky (s_i = 1 / sqrt(B_ii), L L^T = S B S, G = L^-1 S) with the ELIMINATION failure rule: a point
//                 whose block has a B_ii that is not a positive finite number, a squared pivot of the unit-diagonal scaled block below 2^-16, or a G that is not finite is
//                 HELD FIXED for the step: G = 0, so delta_p = 0 and the point contributes no coupling term.  (Dropping a point's rows and columns leaves a principal
//                 submatrix of A, whose Schur complement stays positive semidefinite; a diagonal fallback in place of Cp^-1 would not.)  Held points are counted.
//   schur_rhs     point launch: y = Cp^-1 b_p, t_q = J_p,q y into T (camera order);  camera launch: g_c = b_c - sum_q J_c,q^T t_q
//   schur_apply   S x in residual space, J_c^T (I - J_p Cp^-1 J_p^T) J_c x -- no near-equal pair of camera-sized sums is subtracted:
//                 camera launch u_q = J_c,q x_cam(q);  point launch w = sum J_p,q^T u_q, y = G^T (G w), v_q = u_q - J_p,q y over u_q;  camera launch sum_q J_c,q^T v_q
//                 (+ CtC_c x_c in LM) and the partials of x . S x
//   schur_back    camera launch u_q = J_c,q delta_c (GN: the loop's last delta_c += alpha p rides in it);  point launch delta_p = G^T (G (b_p - sum J_p,q^T u_q))
//
// Camera launches: one wave per camera, lanes striding its observations, two observations per trip with every load of the trip in flight before the first use (k_cam2's
// shape).  They LOAD the camera half of an observation's block from Jb (ba_blocks.hpp: 72 of its 96 bytes) rather than rebuild it in closed form as k_cam2 does: the blocks are what
// thallo_hip_ba_block_diag and the point blocks JP were formed from, so B, E and Cp of one step come from one set of numbers and S is the Schur complement of exactly
// the matrix whose blocks were factored.  Point launches: one thread per point over its list, four observations per trip (k_pt2's shape); a point's G (6 words) lives in
// registers.  Every observation belongs to exactly one point, so the in-place v_q over u_q races with nobody; a thread has read all of its u_q before it writes any.
// Nothing is indexed dynamically, every loop over a block is unrolled.  Sums: one partial per workgroup, fixed order, no float atomics; the held count is an integer.
#include "device_common.hpp"
#include "block_chol.hpp"
#include "ba_blocks.hpp"
#include "../../include/thallo_hip.h"

using namespace thallo;
using thallo::launch::check_launch;

namespace {

constexpr int BLOCK = BA_WG;

__global__ __launch_bounds__(BLOCK) void k_schur_factor(int P_, const float* __restrict__ Hp, const float* __restrict__ shift, float* __restrict__ G, unsigned* __restrict__ held)
{
    __shared__ unsigned cnt[BLOCK / THALLO_WAVE];
    unsigned bad = 0;
    for (int j = blockIdx.x * BLOCK + threadIdx.x; j < P_; j += gridDim.x * BLOCK) {
        float a[6], sh[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] = Hp[(long)k * P_ + j];
#pragma unroll
        for (int i = 0; i < 3; ++i) sh[i] = shift ? shift[3L * j + i] : 0.0f;
        const bool ok = factor<3, true>(a, sh);      // false: the point is held, G = 0
#pragma unroll
        for (int k = 0; k < 6; ++k) G[(long)k * P_ + j] = ok ? a[k] : 0.0f;
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
        if (s) atomicAdd(held, s);
    }
}

// u_q = J_c,q x_cam(q), two floats per observation in camera order.  p != NULL (the GN loop's last term): x = delta_c + alpha p, alpha = alphaN / alphaD (0 if alphaD == 0),
// written back over delta_c by lanes 0 .. 8
__global__ __launch_bounds__(BLOCK) void k_schur_cam_u(int C_, const int* __restrict__ cam_ptr, const float4* __restrict__ Jb, float* x, const float* __restrict__ p,
                                                       thallo_sum_t aN, thallo_sum_t aD, float2* __restrict__ U, const unsigned* __restrict__ gate)
{
    if (gate != nullptr && __builtin_amdgcn_readfirstlane((int)gate[0]) != 0) return;      // LM: the PCG loop already ended on the device
    float alpha = 0.0f;
    if (p != nullptr) alpha = safe_div<false>(sum_partials(aN.partials, aN.count), sum_partials(aD.partials, aD.count));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = blockIdx.x * 4 + wave; c < C_; c += gridDim.x * 4) {
        float xc[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) xc[k] = x[9L * c + k];
        if (p != nullptr) {
#pragma unroll
            for (int k = 0; k < 9; ++k) xc[k] = __builtin_fmaf(alpha, p[9L * c + k], xc[k]);      // explicit fma: the same rounding wherever a delta update is applied
        }
        const int q1e = cam_ptr[c + 1];
        for (int q = cam_ptr[c] + lane; q < q1e; q += 128) {
            const bool h1 = q + 64 < q1e;
            const CamLd A = ld_cam_rows(Jb, q), Bq = ld_cam_rows(Jb, h1 ? q + 64 : q);
            float a0[9], a1[9], b0[9], b1[9];
            rows_of(A, a0, a1); rows_of(Bq, b0, b1);
            float ja0 = 0.0f, ja1 = 0.0f, jb0 = 0.0f, jb1 = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) { ja0 += a0[k] * xc[k]; ja1 += a1[k] * xc[k]; jb0 += b0[k] * xc[k]; jb1 += b1[k] * xc[k]; }
            U[q] = make_float2(ja0, ja1);
            if (h1) U[q + 64] = make_float2(jb0, jb1);
        }
        if (p != nullptr && lane < 9) {      // (behind the loop: every lane of the wave has read x by now -- one wave per camera, in program order)
            float v = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) if (lane == k) v = xc[k];
            x[9L * c + lane] = v;
        }
    }
}

// s_c = sum_q J_c,q^T t_q over a camera's observations.  RHS: g_c = b_c - s_c into g and r.  Else: out = s_c (+ CtC_c x_c) and the partials of x . out
template <bool RHS>
__global__ __launch_bounds__(BLOCK) void k_schur_cam_gather(int C_, const int* __restrict__ cam_ptr, const float4* __restrict__ Jb, const float2* __restrict__ T,
                                                            const float* x, const float* __restrict__ ctc, float* __restrict__ out, float* out2, float* __restrict__ part_out,
                                                            const unsigned* __restrict__ gate)
{   // RHS: x = b (flat), out = g, out2 = r (may be b itself: a lane reads its word of b before it writes it)
    __shared__ float red[16];
    if (gate != nullptr && __builtin_amdgcn_readfirstlane((int)gate[0]) != 0) return;
    float acc = 0.0f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = blockIdx.x * 4 + wave; c < C_; c += gridDim.x * 4) {
        float s[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] = 0.0f;
        // the words of the epilogue (lanes 0 .. 8: one camera unknown each), asked for before the observation loop
        const long ie = 9L * c + (lane < 9 ? lane : 8);
        const float e_x = x[ie], e_c = (!RHS && ctc) ? ctc[ie] : 0.0f;
        const int q1e = cam_ptr[c + 1];
        for (int q = cam_ptr[c] + lane; q < q1e; q += 128) {
            const bool h1 = q + 64 < q1e;
            const int qb = h1 ? q + 64 : q;
            const CamLd A = ld_cam_rows(Jb, q), Bq = ld_cam_rows(Jb, qb);
            const float2 ta = T[q], tb = T[qb];
            float a0[9], a1[9], b0[9], b1[9];
            rows_of(A, a0, a1); rows_of(Bq, b0, b1);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                s[k] += a0[k] * ta.x + a1[k] * ta.y;
                if (h1) s[k] += b0[k] * tb.x + b1[k] * tb.y;
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] = wave_sum_all(s[k]);
        if (lane < 9) {
            float sv = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) if (lane == k) sv = s[k];
            const long i = 9L * c + lane;
            if (RHS) { const float gv = e_x - sv; out[i] = gv; if (out2) out2[i] = gv; }
            else {
                if (ctc) sv += e_c * e_x;
                out[i] = sv;
                acc += e_x * sv;
            }
        }
    }
    if (!RHS) block_store_partial(acc, part_out, red);
}

// One thread per point over its observations (JP: the packed point blocks, contiguous per point; pt_pos: an observation's place in camera order).
//   MODE 0 (right-hand side): y = G^T (G b_p) -> yout;  T[q] = J_p,q y
//   MODE 1 (apply):           w = sum_q J_p,q^T U[q];  y = G^T (G w);  U[q] = U[q] - J_p,q y
//   MODE 2 (back-substitute): w as MODE 1;  delta_p = G^T (G (b_p - w)) -> yout
template <int MODE>
__global__ __launch_bounds__(BLOCK) void k_schur_pt(int P_, const int* __restrict__ pt_ptr, const int* __restrict__ pt_pos, const float2* __restrict__ JP, const float* __restrict__ G,
                                                    const float* __restrict__ bp, float2* U, float* __restrict__ yout, const unsigned* __restrict__ gate)
{
    if (gate != nullptr && __builtin_amdgcn_readfirstlane((int)gate[0]) != 0) return;
    for (int j = blockIdx.x * BLOCK + threadIdx.x; j < P_; j += gridDim.x * BLOCK) {
        float g[6], w[3] = { 0.0f, 0.0f, 0.0f }, y[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = G[(long)k * P_ + j];
        float bv[3] = { 0.0f, 0.0f, 0.0f };
        if (MODE != 1) {
#pragma unroll
            for (int u = 0; u < 3; ++u) bv[u] = bp[3L * j + u];
        }
        const int k0b = pt_ptr[j], k1 = pt_ptr[j + 1];
        if (MODE != 0) {
            // four observations per trip, all their loads in flight together; added up in the list's order
            for (int k0 = k0b; k0 < k1; k0 += 4) {
                PtLd jq[4]; float2 jp[4]; int q[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int k = min(k0 + u, k1 - 1); q[u] = pt_pos[k]; jq[u] = ld_pt_rows(JP, k); }
#pragma unroll
                for (int u = 0; u < 4; ++u) jp[u] = U[q[u]];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k0 + u < k1) { w[0] += jq[u].a.x * jp[u].x + jq[u].b.y * jp[u].y; w[1] += jq[u].a.y * jp[u].x + jq[u].c.x * jp[u].y; w[2] += jq[u].b.x * jp[u].x + jq[u].c.y * jp[u].y; }
            }
        }
        if (MODE == 0) { apply_g<3>(g, bv, y); }
        else if (MODE == 1) { apply_g<3>(g, w, y); }
        else { const float d[3] = { bv[0] - w[0], bv[1] - w[1], bv[2] - w[2] }; apply_g<3>(g, d, y); }
        if (MODE != 1) { yout[3L * j] = y[0]; yout[3L * j + 1] = y[1]; yout[3L * j + 2] = y[2]; }
        if (MODE == 2) continue;
        for (int k0 = k0b; k0 < k1; k0 += 4) {
            PtLd jq[4]; float2 jp[4]; int q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const int k = min(k0 + u, k1 - 1); q[u] = pt_pos[k]; jq[u] = ld_pt_rows(JP, k); }
#pragma unroll
            for (int u = 0; u < 4; ++u) jp[u] = MODE == 1 ? U[q[u]] : make_float2(0.0f, 0.0f);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float t0, t1; pt_j_mul(jq[u], y, t0, t1);
                if (k0 + u < k1) U[q[u]] = MODE == 1 ? make_float2(jp[u].x - t0, jp[u].y - t1) : make_float2(t0, t1);
            }
        }
    }
}

inline bool lists_ok(int C_, int P_, const int* cam_ptr, const int* pt_ptr, const int* pt_pos, const float* Jb, const float* JP, const float* G, const float* U)
{ return C_ >= 0 && P_ >= 0 && C_ + P_ >= 1 && cam_ptr && pt_ptr && pt_pos && Jb && JP && G && U; }

}  // namespace

extern "C" {

int thallo_hip_ba_schur_factor(int P_, const float* Hp, const float* shift_p, float* G, unsigned* held, thallo_stream_t stream)
{
    if (P_ < 0 || !Hp || !G || !held) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t me = hipMemsetAsync(held, 0, sizeof(unsigned), s);
    if (me != hipSuccess) return -(int)me;
    if (P_ < 1) return 0;
    hipLaunchKernelGGL(k_schur_factor, dim3(ba_pt_grid(P_)), dim3(BLOCK), 0, s, P_, Hp, shift_p, G, held);
    return check_launch();
}

int thallo_hip_ba_schur_rhs(int C_, int P_, const int* cam_ptr, const int* pt_ptr, const int* pt_pos, const float* Jb, const float* JP, const float* G, const float* b,
                            float* y, float* U, float* g, float* r_out, thallo_stream_t stream)
{
    if (!lists_ok(C_, P_, cam_ptr, pt_ptr, pt_pos, Jb, JP, G, U) || !b || !y || !g) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    if (P_ > 0) hipLaunchKernelGGL(k_schur_pt<0>, dim3(ba_pt_grid(P_)), dim3(BLOCK), 0, s, P_, pt_ptr, pt_pos, (const float2*)JP, G, b + 9L * C_, (float2*)U, y, (const unsigned*)nullptr);
    if (C_ > 0) hipLaunchKernelGGL(k_schur_cam_gather<true>, dim3(ba_cam_grid(C_)), dim3(BLOCK), 0, s, C_, cam_ptr, (const float4*)Jb, (const float2*)U, b, (const float*)nullptr, g, r_out,
                                   (float*)nullptr, (const unsigned*)nullptr);
    return check_launch();
}

int thallo_hip_ba_schur_apply(int C_, int P_, const int* cam_ptr, const int* pt_ptr, const int* pt_pos, const float* Jb, const float* JP, const float* G, const float* x,
                              const float* ctc, float* U, float* Sx, float* xSx_out, const unsigned* gate, thallo_stream_t stream)
{
    if (!lists_ok(C_, P_, cam_ptr, pt_ptr, pt_pos, Jb, JP, G, U) || C_ < 1 || !x || !Sx || !xSx_out) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const int cb = ba_cam_grid(C_);
    const thallo_sum_t none = { nullptr, 0 };
    hipLaunchKernelGGL(k_schur_cam_u, dim3(cb), dim3(BLOCK), 0, s, C_, cam_ptr, (const float4*)Jb, const_cast<float*>(x), (const float*)nullptr, none, none, (float2*)U, gate);
    if (P_ > 0) hipLaunchKernelGGL(k_schur_pt<1>, dim3(ba_pt_grid(P_)), dim3(BLOCK), 0, s, P_, pt_ptr, pt_pos, (const float2*)JP, G, (const float*)nullptr, (float2*)U, (float*)nullptr, gate);
    hipLaunchKernelGGL(k_schur_cam_gather<false>, dim3(cb), dim3(BLOCK), 0, s, C_, cam_ptr, (const float4*)Jb, (const float2*)U, x, ctc, Sx, (float*)nullptr, xSx_out, gate);
    int e = check_launch(); return e ? e : cb;
}

int thallo_hip_ba_schur_back(int C_, int P_, const int* cam_ptr, const int* pt_ptr, const int* pt_pos, const float* Jb, const float* JP, const float* G, const float* b,
                             float* delta, const float* p, thallo_sum_t alphaN, thallo_sum_t alphaD, float* U, thallo_stream_t stream)
{
    if (!lists_ok(C_, P_, cam_ptr, pt_ptr, pt_pos, Jb, JP, G, U) || !b || !delta) return -(int)hipErrorInvalidValue;
    if (p && (!alphaN.partials || !alphaD.partials || alphaN.count < 1 || alphaD.count < 1)) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    if (C_ > 0) hipLaunchKernelGGL(k_schur_cam_u, dim3(ba_cam_grid(C_)), dim3(BLOCK), 0, s, C_, cam_ptr, (const float4*)Jb, delta, p, alphaN, alphaD, (float2*)U, (const unsigned*)nullptr);
    if (P_ > 0) hipLaunchKernelGGL(k_schur_pt<2>, dim3(ba_pt_grid(P_)), dim3(BLOCK), 0, s, P_, pt_ptr, pt_pos, (const float2*)JP, G, b + 9L * C_, (float2*)U, delta + 9L * C_, (const unsigned*)nullptr);
    return check_launch();
}

}  // extern "C"
