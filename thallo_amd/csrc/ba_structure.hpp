// ba_structure.hpp -- what bundle adjustment's plans rest on, on the host: the incidence lists of the observations, the symbolic structure of the reduced camera matrix S,
// the two-level preconditioner's aggregates and the bytes all of that asks the budget for.  Pure functions over std::vector<int>: no device, no HIP header, so the file
// compiles with a plain C++17 compiler and tools/ba_structure_check.cpp runs it under the sanitizers against the Python restatements (tests/test_ba_structure_host.py).
// BundleAdjustmentPlugin::prepare (plugins.cpp) and ReducedCameraSystem::configure (ba_reduced.cpp) are the callers.
#pragma once
#include <cstddef>
#include <vector>

namespace thallo {
namespace ba {

// ---- incidence lists.  The plan's point order: the caller's, or the points sorted by the first camera that observes them (stable) -- Never, Always, or Auto: when the
// caller's order is far from that (mean jump of the first observing camera between consecutive points > 64).  One point has no order to choose.
enum class Renumber { Never, Always, Auto };
struct Incidence {
    bool perm = false;                          // renumbered: every list below is in the plan's internal point ids
    std::vector<int> cam_ptr, cam_obs;          // C + 1 places; the observations in camera order q (a renumbered plan: each camera's by internal point id, then observation)
    std::vector<int> q_cam, q_pt;               // camera and point of q
    std::vector<int> pt_ptr, pt_pos;            // P + 1 places; each point's q's (a renumbered plan: ascending, i.e. in camera order)
    std::vector<int> new2old;                   // perm: the plan's point j is the caller's new2old[j]; else empty
};
// oToC / oToP: O entries each, already checked to lie in [0, C) and [0, P)
Incidence incidence_lists(int C, int P, int O, const std::vector<int>& oToC, const std::vector<int>& oToP, Renumber renumber);

// ---- the terms of S: (q, q'), two observations of one point with camera(q') <= camera(q).  count_terms sorts each point's list in pt_pos ascending (ascending cameras
// too, so the partners of q are a prefix of the list: what list_terms walks) and counts the terms before anything is built
unsigned long long count_terms(const std::vector<int>& pt_ptr, std::vector<int>& pt_pos, const std::vector<int>& q_cam);

// ---- the structure: the co-visible camera pairs (every diagonal block present, with or without terms), stored in both triangles, a row's blocks consecutive with
// ascending columns.  Per lower-triangle block l, in the order (row, column): keys[l] = row * C + column, its terms (q, q') at terms[2 t], terms[2 t + 1] for t in
// [term_ptr[l], term_ptr[l + 1]), ascending in (q, q'), and lower[3 l ..] = { place of the block, place of its transpose, camera of a diagonal block or -1 }.  A
// (camera, point) pair observed more than once simply yields more terms (both orders of the pair in the diagonal block).
struct Structure {
    std::vector<long> keys;
    std::vector<int> term_ptr, terms;           // list_terms
    unsigned long long nlower = 0, nblk = 0;    // lower-triangle blocks, stored blocks = 2 nlower - C
    std::vector<int> row_ptr, col, lower;       // place_blocks
};
// keys, term_ptr, terms, nlower, nblk from the lists (pt_pos as count_terms left it) -> the terms listed: nterms, or the count was wrong
size_t list_terms(int C, const std::vector<int>& cam_ptr, const std::vector<int>& pt_ptr, const std::vector<int>& pt_pos, const std::vector<int>& q_cam, const std::vector<int>& q_pt,
                  unsigned long long nterms, Structure& st);
// row_ptr, col, lower from the keys (nblk fits an int: the caller has checked)
void place_blocks(int C, Structure& st);

// ---- aggregates of cameras.  greedy_aggregates: at most k cameras each from the lower blocks (the weight of a pair = its block's term count = its co-visible points):
// cameras in ascending id, an unassigned one seeds an aggregate, which repeatedly takes the unassigned camera with the largest summed weight to its members (ties: the
// lower id) until it has k members or no connected camera is left.  Deterministic; the member lists in the order of joining.  member_lists: the lists of a caller's
// array (dense ids, checked by the caller), the members in ascending id
struct Aggregates {
    std::vector<int> agg, mem_ptr, mem;         // aggregate of camera c; members of aggregate a at mem[mem_ptr[a] .. mem_ptr[a + 1])
    int count() const { return (int)mem_ptr.size() - 1; }
};
int default_cameras_per_aggregate(int C);
Aggregates greedy_aggregates(int C, int k, const std::vector<long>& keys, const std::vector<int>& term_ptr);
Aggregates member_lists(const std::vector<int>& agg);

// ---- device bytes, as the budget counts them.  w_stride: floats from one observation's W to the next; ld: the dense layout's leading dimension of n; panel_floats: the
// coarse inverse's work panels (all three are the kernels' numbers, handed in by the caller)
unsigned long long w_bytes(int O, int w_stride);
// known once the terms are counted, before the blocks are: W and the term list -- what the first refusal compares; with the C diagonal blocks every structure has: what it reports
unsigned long long terms_bytes(int O, unsigned long long nterms, int w_stride);
unsigned long long structure_bytes_at_least(int C, int O, unsigned long long nterms, int w_stride);
// S, W, the terms and the four index lists
unsigned long long structure_bytes(int C, int O, unsigned long long nterms, unsigned long long nlower, unsigned long long nblk, int w_stride);
// the dense lower triangle (ld x n), d and the words
unsigned long long dense_bytes(long n, long ld);
// T, Z, Z^T (ld x n each), the panels, d, y, the three lists and the words
unsigned long long coarse_bytes(int C, int K, long n, long ld, long panel_floats);

}  // namespace ba
}  // namespace thallo
