// iw_device.hpp -- device pieces shared by the image_warping kernels (energy_image_warping.hip: LDS-tiled kernels;
// energy_image_warping_march.hip: the wave-marching one-kernel PCG iteration).
#pragma once
#include "device_common.hpp"
#include "dist_device.hpp"
#include "../../include/thallo_hip.h"

namespace thallo {

// W x H = local image (rows include ghost rows); tiles cover the owned rows [row0,row1) only.
struct Geo { int W, H, row0, row1, tx, ty, ntiles; };

// flags byte: bit0 pixel active (Mask==0), bit1 fit residual valid, bits2-4 = number of valid neighbour pairs (0..4).
// With UrShape on the unit pixel grid (GRID path) diag(J^T J) is a function of this byte alone:
//   offset channels: w_reg^2 * 2*cnt + w_fit^2 [fit]      angle channel: w_reg^2 * cnt   (|R'(a) du|^2 = |du|^2 = 1)
// so the GRID path never reads `pre` and never materialises z = M^-1 r: both are recomputed from r and the flags byte.
__device__ __forceinline__ void pre_from_flags(unsigned char f, float wf2, float wr2, float& mo, float& ma)
{
    if (!(f & 1)) { mo = 0.0f; ma = 0.0f; return; }
    const float cnt = (float)((f >> 2) & 7);
    float dgo = (2.0f * cnt) * wr2;
    if (f & 2) dgo += wf2;
    mo = guarded_invert(dgo); ma = guarded_invert(cnt * wr2);
}

__device__ __forceinline__ double wave_sum_all_d(double v) { return wave_sum_all_f64(v); }

// The scalars a one-kernel PCG iteration starts from: alpha_{k-1} = alphaN_{k-1} / alphaD_{k-1}, beta_{k-1} = betaN_{k-1} / alphaN_{k-1}.
// Either from the finished words of iteration k-1 (aDp, bNp), or -- prev.count > 0, the DEFERRED finish -- from its raw per-workgroup
// partials: every wave adds them itself in k_iter_finish's order (same bits in every wave of every workgroup; the slots are L2-resident,
// the additions overlap the first row loads), and one designated thread leaves alphaD_{k-1}, betaN_{k-1} behind as words for later consumers.
// That takes the last-workgroup read-back (three dependent L2 round trips at the END of a launch, nothing to overlap them with) off the
// critical path between two dependent launches.
// U = slots per lane whose loads are in flight together (the marching kernel adds up with U = 1: it does so behind its first row loads, which
// hide the round trips, and has no registers to spare there).
struct PrevSums { const float* aD_part; const double* s12_part; int count; float* aD_word; float* bN_word;
                  unsigned long long* gs; int xslot; };     // gs != NULL (row slabs, device-side exchange): iteration k-1's sums are THIS rank's; the launch's designated wave trades them
                                                            // with the other ranks through mailbox slots xslot .. xslot + 6 and publishes the two global words as tagged granules gs[0], gs[1]
template <int U = 4>
__device__ __forceinline__ void iteration_scalars(thallo_sum_t aNp, thallo_sum_t aDp, thallo_sum_t bNp, const PrevSums& prev, float& alpha, float& beta, bool writer)
{
    const float an = sum_partials(aNp.partials, aNp.count);
    float ad, bn;
    if (prev.count > 0) {
        const int lane = threadIdx.x & (THALLO_WAVE - 1), nb = prev.count;
        if (U == 1) {           // lean form: same additions in the same order as sum_partials, one load in flight, no staging registers
            float t = 0.0f;
            for (int i = lane; i < nb; i += THALLO_WAVE) t += prev.aD_part[i];
            ad = nb == 1 ? prev.aD_part[0] : wave_sum_all(t);
        } else ad = sum_partials(prev.aD_part, nb);
        double n = 0.0, a1 = 0.0, b1 = 0.0;
        for (int i0 = lane; i0 < nb; i0 += U * THALLO_WAVE) {             // U slots per lane and round in flight; additions in index order
            double v[U][3];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * THALLO_WAVE;
#pragma unroll
                for (int q = 0; q < 3; ++q) v[u][q] = i < nb ? prev.s12_part[3 * i + q] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) { n += v[u][0]; a1 += v[u][1]; b1 += v[u][2]; }
        }
        n = wave_sum_all_d(n); a1 = wave_sum_all_d(a1); b1 = wave_sum_all_d(b1);
        alpha = safe_div<false>(an, ad);
        double bd = n - 2.0 * (double)alpha * a1 + (double)alpha * (double)alpha * b1;
        if (!(bd > 0.0)) bd = 0.0;
        bn = (float)bd;
        if (writer) { prev.aD_word[0] = ad; prev.bN_word[0] = bn; }      // writer: exactly ONE thread of the launch, one that certainly gets here
    } else {
        ad = sum_partials(aDp.partials, aDp.count);
        bn = sum_partials(bNp.partials, bNp.count);
        alpha = safe_div<false>(an, ad);
    }
    beta = safe_div<false>(bn, an);
}

// End of a one-kernel PCG iteration, called by every thread of the workgroup with its private sums: float alphaD partial + the three
// double sums, one set per workgroup; with fin_tickets the launch's last workgroup also finishes alphaD_k / betaN_k (single GPU) or
// IS the cross-rank exchange (DIST).  red >= 16 floats, redd >= 48 doubles of LDS.
template <int NT, bool DIST>
#ifdef THALLO_AD_DOUBLE
__device__ __forceinline__ void iter_tail(double acc_d, double s0, double s1, double s2, float* red, double* redd,
#else
__device__ __forceinline__ void iter_tail(float acc, double s0, double s1, double s2, float* red, double* redd,
#endif
                                          float* __restrict__ aD_out, double* __restrict__ s12_out, thallo_sum_t bNp, const thallo_dist_t* dd,
                                          unsigned* __restrict__ fin_tickets, float* __restrict__ aD_word, float* __restrict__ bN_word, int xslot)
{
    // multi-GPU: EVERY wave of a boundary workgroup has issued peer-to-peer Ap stores; each drains its own before the workgroup
    // barrier below, so that the arrival ticket behind that barrier (and the granules the last arrival sends) cannot overtake them
    if (DIST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // float alphaD partial + the two double sums, one set per workgroup
    const int lane = threadIdx.x & (THALLO_WAVE - 1), wave = threadIdx.x / THALLO_WAVE;
#ifdef THALLO_AD_DOUBLE
    // (experiment, VERDICT r2 "what's weak" 3: alphaD accumulated in double per workgroup like N, S1, S2; the workgroup's total is rounded to float once)
    const double wad = wave_sum_all_d(acc_d);
    if (lane == 0) redd[32 + wave] = wad;
    lds_barrier();
    double tot = 0.0; for (int w = 0; w < NT / THALLO_WAVE; ++w) tot += redd[32 + w];
    const float acc = wave == 0 ? (float)tot : 0.0f;             // the workgroup's alphaD, carried by wave 0 only (all its lanes: wave_sum_all below divides by 64 -> use lane 0)
    const float wa = wave == 0 ? (float)tot : 0.0f; (void)acc;
    const double w0 = wave_sum_all_d(s0), w1 = wave_sum_all_d(s1), w2 = wave_sum_all_d(s2);
#else
    const float wa = wave_sum_all(acc); const double w0 = wave_sum_all_d(s0), w1 = wave_sum_all_d(s1), w2 = wave_sum_all_d(s2);
#endif
    if (lane == 0) { red[wave] = wa; redd[3 * wave] = w0; redd[3 * wave + 1] = w1; redd[3 * wave + 2] = w2; }
    lds_barrier();
    if (threadIdx.x == 0) {
        float a = 0.0f; double b0 = 0.0, b1 = 0.0, b2 = 0.0;
        for (int w = 0; w < NT / THALLO_WAVE; ++w) { a += red[w]; b0 += redd[3 * w]; b1 += redd[3 * w + 1]; b2 += redd[3 * w + 2]; }
        if (!fin_tickets) { aD_out[blockIdx.x] = a; s12_out[3 * blockIdx.x] = b0; s12_out[3 * blockIdx.x + 1] = b1; s12_out[3 * blockIdx.x + 2] = b2; }
        else {
            // in-kernel finish (saves the one-wave k_iter_finish launch: worth 4-5 us per iteration on small images): write-through
            // partials, two-level arrival tickets (workgroup b -> group b % 32, each group word on its own 64-byte line; same-address
            // atomics serialise at ~12 ns each), the last arrival adds everything up in k_iter_finish's order
            typedef unsigned long long u64_t;
            __hip_atomic_store(aD_out + blockIdx.x, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            u64_t* sp = reinterpret_cast<u64_t*>(s12_out) + 3 * blockIdx.x;
            __hip_atomic_store(sp, (u64_t)__double_as_longlong(b0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(sp + 1, (u64_t)__double_as_longlong(b1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(sp + 2, (u64_t)__double_as_longlong(b2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned grp = blockIdx.x % 32, members = (gridDim.x - grp + 31) / 32, groups = gridDim.x < 32 ? gridDim.x : 32;
            unsigned* sub = fin_tickets + 16 + 16 * grp;
            bool last = false;
            if (__hip_atomic_fetch_add(sub, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1) {
                __hip_atomic_store(sub, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = __hip_atomic_fetch_add(fin_tickets, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1;
            }
            red[15] = last ? 1.0f : 0.0f;
        }
    }
    if (fin_tickets) {
        lds_barrier();
        if (red[15] != 0.0f && wave == 0) {
            const IterationSums S = load_iteration_sums(aD_out, s12_out, gridDim.x, bNp);          // bNp = alphaN_k (= betaN_{k-1}; alphaN_0 for the first iteration)
            const float ad = S.ad, an = S.an; const double n = S.n, a1 = S.s1, b1 = S.s2;
            if (lane == 0) __hip_atomic_store(fin_tickets, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (DIST) {     // multi-GPU: the same wave is the exchange (every wave drained its remote Ap rows -- s_waitcnt vmcnt(0) -- before the barrier in front of its workgroup's ticket)
                dist_exchange_iter_wave(*dd, xslot, ad, n, a1, b1, an, aD_word, bN_word);
            } else {
                const float al = safe_div<false>(an, ad);
                double bn = n - 2.0 * (double)al * a1 + (double)al * (double)al * b1;
                if (!(bn > 0.0)) bn = 0.0;
                if (lane == 0) { aD_word[0] = ad; bN_word[0] = (float)bn; }
            }
        }
    }
}

// ---- host side of the one-kernel PCG iteration: thallo_hip_iw_pcg_iter (energy_image_warping.hip) checks the block once and hands it to the kernel's launch

// What every kernel and form asks of a block: owned rows inside the image, the planes every kernel touches, delta unless the launch is a GN step's first, a
// well-formed `prev`, a world within bounds and -- where a wave of the launch exchanges scalars -- its mailbox, even peer offsets, and a form that exists.
// Tickets: all three or none (IterForm below).  Each launch function adds its kernel's own conditions.
inline int iw_iter_check(const thallo_iw_iter_t& a)
{
    const int bad = -(int)hipErrorInvalidValue;
    if (a.row0 < 0 || a.row1 > a.H || a.row0 >= a.row1) return bad;
    if (!a.cs || !a.flags || !a.r_in || !a.r_out || !a.p_in || !a.p_out || !a.alphaD_out || !a.s12_out) return bad;
    if (!(a.mode & 1) && !a.delta) return bad;
    if (a.prev && !(a.mode & 1)) {
        const thallo_prev_t& p = *a.prev;
        if (p.count < 1 || p.count > THALLO_MAX_PARTIALS || !p.alphaD_partials || !p.s12_partials || !p.alphaD_word || !p.betaN_word || p.s12_partials == a.s12_out) return bad;
    }
    if (a.dist) {
        const thallo_dist_t& d = *a.dist;
        const bool fin = !a.prev && a.fin_tickets && a.alphaD_word && a.betaN_word;
        if (d.world < 1 || d.world > THALLO_DIST_MAX_WORLD) return bad;
        if ((fin || a.gs) && (!d.mail || !d.ctl || 7 * d.world > 64)) return bad;
        if (fin && (a.slot0 < 0 || a.betaN_prev.count != 1)) return bad;
        if (a.gs && (!a.prev || a.prev_slot0 < 0 || a.alphaN_prev.count != 1)) return bad;
        for (int k = 0; k < 2; ++k) if (d.peer_r[k] && ((d.peer_off_o[k] | d.peer_off_a[k]) & 1)) return bad;
        if (a.prev && !a.gs) return -(int)hipErrorNotSupported;      // (no kernel finishes a rank's own sums ahead of a launch-end exchange)
    }
    return 0;
}

// What a k_iter* launch hands its kernel behind the planes, derived from the block's form in one place: the deferred forms start from `prev` instead of the
// two finished words and carry no tickets; only a slab launch has a peer block and mailbox slots.
struct IterForm {
    thallo_sum_t aDp, bNp; thallo_dist_t d; unsigned* tickets; float *aD_word, *bN_word; int xslot; PrevSums prev;
    explicit IterForm(const thallo_iw_iter_t& a)
    {
        const thallo_sum_t none = { nullptr, 0 };
        const bool fin = !a.prev && a.fin_tickets && a.alphaD_word && a.betaN_word;
        aDp = a.prev ? none : a.alphaD_prev; bNp = a.prev ? none : a.betaN_prev;
        d = a.dist ? *a.dist : thallo_dist_t{};
        tickets = fin ? a.fin_tickets : nullptr; aD_word = fin ? a.alphaD_word : nullptr; bN_word = fin ? a.betaN_word : nullptr;
        xslot = a.dist && !a.prev ? a.slot0 : 0;
        prev = PrevSums{ nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0 };
        if (a.prev && !(a.mode & 1)) prev = PrevSums{ a.prev->alphaD_partials, a.prev->s12_partials, a.prev->count, a.prev->alphaD_word, a.prev->betaN_word,
                                                      a.dist ? a.gs : nullptr, a.dist ? a.prev_slot0 : 0 };
    }
};

// one per kernel file (the sweep build's probe/march_probe_kernels.hip defines launch_march in the product file's place); the block has passed iw_iter_check
int launch_iter(const thallo_iw_iter_t& a, hipStream_t stream);
int launch_march(const thallo_iw_iter_t& a, hipStream_t stream);
int launch_march_rc(const thallo_iw_iter_t& a, hipStream_t stream);

}  // namespace thallo
