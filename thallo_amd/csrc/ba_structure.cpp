// ba_structure.cpp -- see ba_structure.hpp.  Host only.
#include "ba_structure.hpp"
#include <algorithm>
#include <cstdlib>

namespace thallo {
namespace ba {

// (the reference sorts / transposes the CSR with cuSPARSE every GN iteration: gauss_newton.t:1349-1378)
Incidence incidence_lists(int C, int P, int O, const std::vector<int>& oc, const std::vector<int>& oToP, Renumber renumber)
{
    Incidence L;
    std::vector<int> op(oToP);
    {   // the point order
        std::vector<int> first(P, C);
        for (int o = 0; o < O; ++o) if (oc[o] < first[op[o]]) first[op[o]] = oc[o];
        double tv = 0.0; for (int j = 0; j + 1 < P; ++j) tv += std::abs(first[j + 1] - first[j]);
        L.perm = renumber != Renumber::Never && P > 1 && (renumber == Renumber::Always || tv > 64.0 * (double)P);
        if (L.perm) {
            std::vector<int> new2old(P), old2new(P);
            for (int j = 0; j < P; ++j) new2old[j] = j;
            std::stable_sort(new2old.begin(), new2old.end(), [&](int x, int y) { return first[x] < first[y]; });
            for (int j = 0; j < P; ++j) old2new[new2old[j]] = j;
            for (int o = 0; o < O; ++o) op[o] = old2new[op[o]];
            L.new2old = new2old;
        }
    }
    std::vector<int> cp(C + 1, 0), pp(P + 1, 0), cobs(O), qc(O), qp(O), pos(O), ppos(O);
    for (int o = 0; o < O; ++o) { cp[oc[o] + 1]++; pp[op[o] + 1]++; }
    for (int c = 0; c < C; ++c) cp[c + 1] += cp[c];
    for (int j = 0; j < P; ++j) pp[j + 1] += pp[j];
    std::vector<int> cc(cp.begin(), cp.end() - 1), pc(pp.begin(), pp.end() - 1);
    for (int o = 0; o < O; ++o) cobs[cc[oc[o]]++] = o;
    if (L.perm)         // a renumbered plan also walks each camera's observations in the order of the (internal) point ids: its gathers then run through the points front to back
        for (int c = 0; c < C; ++c) std::sort(cobs.begin() + cp[c], cobs.begin() + cp[c + 1], [&](int a, int b) { return op[a] != op[b] ? op[a] < op[b] : a < b; });
    for (int q = 0; q < O; ++q) { const int o = cobs[q]; pos[o] = q; qc[q] = oc[o]; qp[q] = op[o]; }
    if (L.perm) { for (int q = 0; q < O; ++q) ppos[pc[qp[q]]++] = q; }          // ... and each point's observations in camera order
    else for (int o = 0; o < O; ++o) ppos[pc[op[o]]++] = pos[o];
    L.cam_ptr.swap(cp); L.cam_obs.swap(cobs); L.q_cam.swap(qc); L.q_pt.swap(qp); L.pt_ptr.swap(pp); L.pt_pos.swap(ppos);
    return L;
}

unsigned long long count_terms(const std::vector<int>& pp, std::vector<int>& ppos, const std::vector<int>& qc)
{
    const int P = (int)pp.size() - 1;
    // a point's observations ascending in camera order: ascending cameras too, so the partners q' of q with camera(q') <= camera(q) are a prefix of the list
    for (int j = 0; j < P; ++j) std::sort(ppos.begin() + pp[j], ppos.begin() + pp[j + 1]);
    // an observation pairs with every observation of its point whose camera is not above its own
    unsigned long long nterms = 0;
    for (int j = 0; j < P; ++j)
        for (int k = pp[j], e = pp[j]; k < pp[j + 1]; ++k) {
            while (e < pp[j + 1] && qc[ppos[e]] <= qc[ppos[k]]) ++e;
            nterms += (unsigned long long)(e - pp[j]);
        }
    return nterms;
}

// row by row, without a comparison sort of the terms: a row's observations ascend, a counting pass sizes its blocks, a second pass places the terms -- (q, q')
// ascending within every block.  Every diagonal block is present, with or without terms
size_t list_terms(int C, const std::vector<int>& cp, const std::vector<int>& pp, const std::vector<int>& ppos, const std::vector<int>& qc, const std::vector<int>& qp,
                  unsigned long long nterms, Structure& st)
{
    std::vector<int>& term_ptr = st.term_ptr; std::vector<int>& tq = st.terms; std::vector<long>& keys = st.keys;
    keys.clear(); term_ptr.clear(); tq.assign(2 * (size_t)nterms + 2, 0);
    std::vector<int> cnt((size_t)C, 0), touched;
    size_t at = 0;
    for (int i = 0; i < C; ++i) {
        touched.assign(1, i);
        for (int q = cp[i]; q < cp[i + 1]; ++q)
            for (int k = pp[qp[q]]; k < pp[qp[q] + 1] && qc[ppos[k]] <= i; ++k) { const int c2 = qc[ppos[k]]; if (cnt[c2]++ == 0 && c2 != i) touched.push_back(c2); }
        std::sort(touched.begin(), touched.end());
        for (int c2 : touched) { keys.push_back((long)i * C + c2); term_ptr.push_back((int)at); const int n = cnt[c2]; cnt[c2] = (int)at; at += (size_t)n; }      // (cnt: now the block's next free place)
        for (int q = cp[i]; q < cp[i + 1]; ++q)
            for (int k = pp[qp[q]]; k < pp[qp[q] + 1] && qc[ppos[k]] <= i; ++k) { const size_t t = (size_t)cnt[qc[ppos[k]]]++; tq[2 * t] = q; tq[2 * t + 1] = ppos[k]; }
        for (int c2 : touched) cnt[c2] = 0;
    }
    term_ptr.push_back((int)at);
    tq.resize(2 * (size_t)nterms);
    st.nlower = keys.size(); st.nblk = 2 * st.nlower - (unsigned long long)C;
    return at;
}

void place_blocks(int C, Structure& st)
{
    const std::vector<long>& keys = st.keys;
    std::vector<int> row_ptr((size_t)C + 1, 0);
    for (long key : keys) { const int i = (int)(key / C), j = (int)(key % C); row_ptr[i + 1]++; if (i != j) row_ptr[j + 1]++; }
    for (int c = 0; c < C; ++c) row_ptr[c + 1] += row_ptr[c];
    // places: the keys ascend by (row, column), so a row's lower part and diagonal are placed before the first (k, row), k > row, and those arrive with ascending k
    std::vector<int> fill(row_ptr.begin(), row_ptr.end() - 1), col((size_t)st.nblk), lower(3 * (size_t)st.nlower);
    for (size_t l = 0; l < keys.size(); ++l) {
        const int i = (int)(keys[l] / C), j = (int)(keys[l] % C);
        const int bij = fill[i]++; col[bij] = j;
        int bji = bij;
        if (i != j) { bji = fill[j]++; col[bji] = i; }
        lower[3 * l] = bij; lower[3 * l + 1] = bji; lower[3 * l + 2] = i == j ? i : -1;
    }
    st.row_ptr.swap(row_ptr); st.col.swap(col); st.lower.swap(lower);
}

int default_cameras_per_aggregate(int C) { return std::max(8, (C + 127) / 128); }

Aggregates greedy_aggregates(int C_, int k, const std::vector<long>& keys, const std::vector<int>& term_ptr)
{
    Aggregates A;
    std::vector<int>& agg = A.agg; std::vector<int>& mem_ptr = A.mem_ptr; std::vector<int>& mem = A.mem;
    std::vector<size_t> at((size_t)C_ + 1, 0);
    for (long key : keys) { const int i = (int)(key / C_), j = (int)(key % C_); if (i != j) { at[(size_t)i + 1]++; at[(size_t)j + 1]++; } }
    for (int c = 0; c < C_; ++c) at[(size_t)c + 1] += at[(size_t)c];
    std::vector<int> nbr(at[(size_t)C_]), wgt(at[(size_t)C_]);
    std::vector<size_t> fill(at.begin(), at.end() - 1);
    for (size_t l = 0; l < keys.size(); ++l) {
        const int i = (int)(keys[l] / C_), j = (int)(keys[l] % C_), w = term_ptr[l + 1] - term_ptr[l];
        if (i == j) continue;
        nbr[fill[(size_t)i]] = j; wgt[fill[(size_t)i]++] = w; nbr[fill[(size_t)j]] = i; wgt[fill[(size_t)j]++] = w;
    }
    agg.assign((size_t)C_, -1);
    std::vector<long> score((size_t)C_, 0);
    std::vector<int> cand;
    int K_ = 0;
    for (int seed = 0; seed < C_; ++seed) {
        if (agg[(size_t)seed] >= 0) continue;
        const int a = K_++;
        mem_ptr.push_back((int)mem.size());
        cand.clear();
        int next = seed, size = 0;
        while (next >= 0) {
            agg[(size_t)next] = a; mem.push_back(next); ++size;
            for (size_t t = at[(size_t)next]; t < at[(size_t)next + 1]; ++t) {
                const int u = nbr[t];
                if (agg[(size_t)u] >= 0) continue;
                if (score[(size_t)u] == 0) cand.push_back(u);
                score[(size_t)u] += wgt[t] > 0 ? wgt[t] : 1;
            }
            next = -1;
            if (size >= k) break;
            for (int u : cand) if (agg[(size_t)u] < 0 && (next < 0 || score[(size_t)u] > score[(size_t)next] || (score[(size_t)u] == score[(size_t)next] && u < next))) next = u;
        }
        for (int u : cand) score[(size_t)u] = 0;
    }
    mem_ptr.push_back((int)mem.size());
    return A;
}

Aggregates member_lists(const std::vector<int>& given)
{
    Aggregates A;
    A.agg = given;
    int K_ = 0;
    for (int a : A.agg) if (a + 1 > K_) K_ = a + 1;
    A.mem_ptr.assign((size_t)K_ + 1, 0);
    for (int a : A.agg) A.mem_ptr[(size_t)a + 1]++;
    for (int a = 0; a < K_; ++a) A.mem_ptr[(size_t)a + 1] += A.mem_ptr[(size_t)a];
    A.mem.resize(A.agg.size());
    std::vector<int> fillm(A.mem_ptr.begin(), A.mem_ptr.end() - 1);
    for (size_t c = 0; c < A.agg.size(); ++c) A.mem[(size_t)fillm[(size_t)A.agg[c]]++] = (int)c;      // (members in ascending id)
    return A;
}

unsigned long long w_bytes(int O, int w_stride) { return sizeof(float) * (unsigned long long)w_stride * (unsigned long long)O + 64; }

unsigned long long terms_bytes(int O, unsigned long long nterms, int w_stride) { return w_bytes(O, w_stride) + 8ULL * nterms; }

unsigned long long structure_bytes_at_least(int C, int O, unsigned long long nterms, int w_stride) { return terms_bytes(O, nterms, w_stride) + 81ULL * 4 * (unsigned long long)C; }

unsigned long long structure_bytes(int C, int O, unsigned long long nterms, unsigned long long nlower, unsigned long long nblk, int w_stride)
{
    return 81ULL * 4 * nblk + 64 + w_bytes(O, w_stride) + 8ULL * nterms + 16 + 4ULL * ((unsigned long long)C + 5) + 4ULL * (nblk + 4) + 4ULL * (3 * nlower + 4) + 4ULL * (nlower + 5);
}

unsigned long long dense_bytes(long n, long ld) { return 4ULL * (unsigned long long)ld * (unsigned long long)n + 4ULL * (unsigned long long)n + 128; }

unsigned long long coarse_bytes(int C, int K, long n, long ld, long panel_floats)
{
    return 3ULL * 4 * (unsigned long long)ld * (unsigned long long)n + 4ULL * (unsigned long long)panel_floats + 2ULL * 4 * (unsigned long long)n +
           4ULL * (2ULL * (unsigned long long)C + (unsigned long long)K + 1) + 6 * 64;
}

}  // namespace ba
}  // namespace thallo
