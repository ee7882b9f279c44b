// block_chol.hpp -- the scaled Cholesky factor of one small dense block and its apply, for every launch that factors a block of J^T J: the block-Jacobi preconditioner
// (block_precond.hip, N = 3 or 9) and the point elimination of the Schur solve (ba_schur.hip, N = 3).
//
//   B = H + diag(shift);  s_i = 1 / sqrt(B_ii);  L L^T = S B S (Cholesky);  G = L^-1 S, lower triangular, packed (block_regions.hpp tri);  B^-1 r = G^T (G r)
//
// A block lives in registers, every loop is unrolled, nothing is indexed dynamically.  factor() returns false for a block that has a diagonal entry that is not a
// positive finite number, a pivot of the unit-diagonal scaled block that fails the pivot test, or a G that came out non-finite.  The two callers differ in the pivot
// test and in what they do with a failed block:
//   preconditioner (ELIM = false): pivot d > 0.  The caller falls back to the DIAGONAL, G = diag(sqrt(pre)): any symmetric positive definite M^-1 serves PCG.
//   elimination    (ELIM = true):  pivot d >= PIVOT_FLOOR.  The caller HOLDS the point for the step, G = 0: Cp^-1 has to be the inverse of the block that is eliminated,
//                                  and dropping a point's rows and columns leaves a principal submatrix, whose Schur complement stays positive semidefinite.
#pragma once
#include "block_regions.hpp"

namespace thallo {

constexpr float PIVOT_FLOOR = 1.0f / 65536.0f;      // 2^-16: the pivots of a unit-diagonal block lie in (0, 1] and carry a few ulps (2^-24) of error; below this fewer than two digits survive

// z = G^T (G r)
template <int N> __device__ __forceinline__ void apply_g(const float (&g)[tri_n(N)], const float (&r)[N], float (&z)[N])
{
    float y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j <= i; ++j) s += g[tri(i, j)] * r[j];
        y[i] = s;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        float s = 0.0f;
#pragma unroll
        for (int i = j; i < N; ++i) s += g[tri(i, j)] * y[i];
        z[j] = s;
    }
}

// a: in, the lower triangle of H; out, G = L^-1 S with L L^T = S (H + diag(sh)) S
template <int N, bool ELIM = false> __device__ __forceinline__ bool factor(float (&a)[tri_n(N)], const float (&sh)[N])
{
    float s[N], inv[N];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float d = a[tri(i, i)] + sh[i];
        ok = ok && d > 0.0f && d < INFINITY;
        s[i] = 1.0f / sqrtf(d);
        a[tri(i, i)] = d;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) a[tri(i, j)] = (a[tri(i, j)] * s[i]) * s[j];
    // Cholesky, column by column, in place
#pragma unroll
    for (int j = 0; j < N; ++j) {
        float d = a[tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= a[tri(j, k)] * a[tri(j, k)];
        ok = ok && (ELIM ? d >= PIVOT_FLOOR : d > 0.0f) && d < INFINITY;
        inv[j] = 1.0f / sqrtf(d);
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            float v = a[tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= a[tri(i, k)] * a[tri(j, k)];
            a[tri(i, j)] = v * inv[j];
        }
    }
    // L^-1, row by row, in place: row i of L is needed for every entry of row i of the inverse, the rows above are the inverse's already
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float li[N];
#pragma unroll
        for (int k = 0; k < i; ++k) li[k] = a[tri(i, k)];
#pragma unroll
        for (int j = 0; j < i; ++j) {
            float v = li[j] * inv[j];
#pragma unroll
            for (int k = j + 1; k < i; ++k) v += li[k] * a[tri(k, j)];
            a[tri(i, j)] = -inv[i] * v;
        }
        a[tri(i, i)] = inv[i];
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) { a[tri(i, j)] *= s[j]; ok = ok && fabsf(a[tri(i, j)]) < INFINITY; }
    return ok;
}

}  // namespace thallo
