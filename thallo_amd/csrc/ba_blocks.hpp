// ba_blocks.hpp -- what bundle adjustment's kernels share (energy_ba.hip, block_precond.hip k_ba_block_diag, ba_schur.hip, ba_schur_explicit.hip): the block of one
// observation, its packed point half, and the launch shapes.
//
// Jb[q], the block of observation q (camera-sorted order): 24 floats = six float4, what precomputeJ wrote (energy_ba.hip k_compute_j)
//
//   float  |  0 ............. 8 |  9  10  11 | 12 ............ 20 | 21  22  23 |
//          |  d r0 / d camera   | d r0 / d X |  d r1 / d camera   | d r1 / d X |
//   float4 |  [0]    [1]    [2].x  [2].yzw   |  [3]    [4]    [5].x  [5].yzw   |
//
// JP[k], its point half, packed once per step in POINT order (k: the observation's place in its point's list): three float2
//   a = (r0.d9, r0.d10), b = (r0.d11, r1.d9), c = (r1.d10, r1.d11)
//
// Everything here is inlined and takes and returns registers; the loads are issued in the order they are written.
#pragma once
#include "device_common.hpp"

namespace thallo {

constexpr int BA_ROW = 12;       // floats per residual row of a block: row 1 starts here
constexpr int BA_NC = 9;         // a row's camera entries come first ...
constexpr int BA_NP = 3;         // ... the point's after them

// the whole block, in the layout's order: entry k of row r for the camera is a[BA_ROW * r + k], for the point a[BA_ROW * r + BA_NC + k]
struct Blk { float a[2 * BA_ROW]; };
__device__ __forceinline__ Blk ld_blk(const float4* __restrict__ Jb, long q)
{
    Blk b; const float4* s = Jb + 6 * q;
#pragma unroll
    for (int k = 0; k < 6; ++k) { const float4 v = s[k]; b.a[4 * k] = v.x; b.a[4 * k + 1] = v.y; b.a[4 * k + 2] = v.z; b.a[4 * k + 3] = v.w; }
    return b;
}

// the camera rows alone, 72 of the block's 96 bytes: as loaded, and as rows
struct CamLd { float4 a0, a1, b0, b1; float a8, b8; };
__device__ __forceinline__ CamLd ld_cam_rows(const float4* __restrict__ Jb, long q)
{
    const float4* s = Jb + 6 * q;
    CamLd r;
    r.a0 = s[0]; r.a1 = s[1]; r.a8 = reinterpret_cast<const float*>(s + 2)[0];
    r.b0 = s[3]; r.b1 = s[4]; r.b8 = reinterpret_cast<const float*>(s + 5)[0];
    return r;
}
__device__ __forceinline__ void rows_of(const CamLd& r, float (&r0)[BA_NC], float (&r1)[BA_NC])
{
    r0[0] = r.a0.x; r0[1] = r.a0.y; r0[2] = r.a0.z; r0[3] = r.a0.w; r0[4] = r.a1.x; r0[5] = r.a1.y; r0[6] = r.a1.z; r0[7] = r.a1.w; r0[8] = r.a8;
    r1[0] = r.b0.x; r1[1] = r.b0.y; r1[2] = r.b0.z; r1[3] = r.b0.w; r1[4] = r.b1.x; r1[5] = r.b1.y; r1[6] = r.b1.z; r1[7] = r.b1.w; r1[8] = r.b8;
}

// JP[k] from Jb[q]: the two float4 that end the rows; .yzw are the point's
__device__ __forceinline__ void pack_pt_rows(const float4* Jb, long q, float2* JP, long k)
{
    const float4 a = Jb[6 * q + 2], b = Jb[6 * q + 5];
    float2* d = JP + 3 * k;
    d[0] = make_float2(a.y, a.z); d[1] = make_float2(a.w, b.y); d[2] = make_float2(b.z, b.w);
}
// JP[k] as loaded, and as rows
struct PtLd { float2 a, b, c; };
__device__ __forceinline__ PtLd ld_pt_rows(const float2* __restrict__ JP, long k)
{
    PtLd r;
    r.a = JP[3 * k]; r.b = JP[3 * k + 1]; r.c = JP[3 * k + 2];
    return r;
}
__device__ __forceinline__ void rows_of(const PtLd& r, float (&r0)[BA_NP], float (&r1)[BA_NP])
{
    r0[0] = r.a.x; r0[1] = r.a.y; r0[2] = r.b.x;
    r1[0] = r.b.y; r1[1] = r.c.x; r1[2] = r.c.y;
}
// (t0, t1) = J_p y.  Its transpose, w += J_p^T u = (a.x u.x + b.y u.y, a.y u.x + c.x u.y, b.x u.x + c.y u.y), stays written out in k_pt2 and k_schur_pt: every
// helper form of it tried (accumulators by reference, a returned float3, rows_of) moved their accumulators' promotion to registers behind the inlining and
// changed those kernels' instruction order.
__device__ __forceinline__ void pt_j_mul(const PtLd& j, const float (&y)[BA_NP], float& t0, float& t1)
{
    t0 = j.a.x * y[0] + j.a.y * y[1] + j.b.x * y[2]; t1 = j.b.y * y[0] + j.c.x * y[1] + j.c.y * y[2];
}

// ------------------------------------------------------------------------------------------ host: the launch shapes
// Every launch here has BA_WG threads per workgroup.  A camera launch gives one wave to a camera, four cameras to a workgroup; a point launch one thread to a point.
// Both are capped and stride over what is left.  The camera launches of one plan must agree on ba_cam_grid: it is the number of partials they leave
// (thallo_hip_ba_apply2_camera_slots, thallo_hip_ba_schur_apply and thallo_hip_ba_schur_apply_s return it, and the solver sizes and sums the slots by it).
constexpr int BA_WG = 256;
inline int ba_cam_grid(int C_) { const int g = (C_ + 3) / 4; return g > 448 ? 448 : g; }      // (0 without cameras: such a launch is skipped or has no camera workgroups)
inline int ba_pt_grid(int P_) { const int g = (P_ + BA_WG - 1) / BA_WG; return g > 512 ? 512 : g < 1 ? 1 : g; }
// the launches that do cameras and points in one grid: workgroups [0, cam_blocks) the cameras, the rest the points; <= 960 partials
inline void gather_shape(int C_, int P_, int& cam_blocks, int& grid) { cam_blocks = ba_cam_grid(C_); grid = cam_blocks + ba_pt_grid(P_); }

}  // namespace thallo
