// block_regions.hpp -- what the launches over block regions share (block_precond.hip, held.hip; tri also block_chol.hpp, ba_schur_explicit.hip): the packed lower triangle
// and which region a block belongs to.
// Storage as in block_precond.hip: H and G hold the regions one after the other, each as n (n + 1) / 2 planes of `count` floats; one lane handles one block.
#pragma once
#include "../../include/thallo_hip.h"

namespace thallo {

__host__ __device__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }      // packed index of (i, j), j <= i
__host__ __device__ constexpr int tri_n(int n) { return n * (n + 1) / 2; }

inline bool regions_ok(const thallo_block_regions_t& R)
{
    if (R.n < 1 || R.n > THALLO_HIP_MAX_BLOCK_REGIONS) return false;
    for (int i = 0; i < R.n; ++i) if ((R.r[i].size != 3 && R.r[i].size != 9) || R.r[i].count < 0 || R.r[i].offset < 0) return false;
    return true;
}
inline long regions_blocks(const thallo_block_regions_t& R) { long t = 0; for (int i = 0; i < R.n; ++i) t += R.r[i].count; return t; }

// which region block t (counted over all regions) belongs to: its size, its index inside the region, the region's first unknown and its base in H / G
struct Where { int size; long b, count, first, base; };
__device__ __forceinline__ Where locate(const thallo_block_regions_t& R, long t)
{
    Where w{ 0, 0, 0, 0, 0 };
    long base = 0;
#pragma unroll
    for (int i = 0; i < THALLO_HIP_MAX_BLOCK_REGIONS; ++i) {
        if (i < R.n && w.size == 0) {
            const long c = R.r[i].count;
            if (t < c) { w.size = R.r[i].size; w.b = t; w.count = c; w.first = R.r[i].offset; w.base = base; }
            else { t -= c; base += (long)tri_n(R.r[i].size) * c; }
        }
    }
    return w;
}

}  // namespace thallo
