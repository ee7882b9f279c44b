// ba_structure_check.cpp -- bundle adjustment's host-side structure builders (thallo_amd/csrc/ba_structure.cpp, nothing else of the library) on one instance from stdin,
// every array printed by name: what tests/test_ba_structure_host.py compares, entry by entry, with the Python restatements (tests/ba_schur_mirror.py SchurLists,
// tests/ba_schur_explicit_mirror.py SchurStructure, tests/ba_two_level_mirror.py greedy_aggregates / member_lists) while the sanitizers watch.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ba_structure_check.cpp thallo_amd/csrc/ba_structure.cpp -o ba_structure_check
//
// stdin, as text: C P O renumber k, then oToC (O ints), then oToP (O ints); renumber: 0 never, 1 always, 2 by the rule; k: cameras per greedy aggregate (0: the default
// size).  C more ints, where they follow: a caller's aggregate array (dense ids) -- without them the greedy aggregates stand in for it.
// stdout: one line per array, "<name> <count> <entries ...>"; scalars as "<name> = <value>".
#include "../thallo_amd/csrc/ba_structure.hpp"
#include <cstdio>
#include <vector>

using namespace thallo::ba;

static const int W_STRIDE = 32;      // THALLO_HIP_SCHUR_W_STRIDE (include/thallo_hip.h)

template <class T> static void print(const char* name, const std::vector<T>& v)
{
    printf("%s %zu", name, v.size());
    for (const T& x : v) printf(" %lld", (long long)x);
    printf("\n");
}

static bool read_ints(std::vector<int>& v) { for (int& x : v) if (scanf("%d", &x) != 1) return false; return true; }

int main()
{
    int C, P, O, renumber, k;
    if (scanf("%d %d %d %d %d", &C, &P, &O, &renumber, &k) != 5 || C < 1 || P < 1 || O < 0 || renumber < 0 || renumber > 2 || k < 0) { fprintf(stderr, "usage: C P O renumber k, oToC, oToP on stdin\n"); return 2; }
    std::vector<int> oc((size_t)O), op((size_t)O);
    if (!read_ints(oc) || !read_ints(op)) { fprintf(stderr, "short input\n"); return 2; }
    for (int o = 0; o < O; ++o) if (oc[o] < 0 || oc[o] >= C || op[o] < 0 || op[o] >= P) { fprintf(stderr, "observation %d out of range\n", o); return 2; }
    std::vector<int> given((size_t)C);
    const bool have_given = read_ints(given);
    if (have_given) for (int a : given) if (a < 0 || a >= C) { fprintf(stderr, "aggregate id %d out of range\n", a); return 2; }

    Incidence L = incidence_lists(C, P, O, oc, op, renumber == 0 ? Renumber::Never : renumber == 1 ? Renumber::Always : Renumber::Auto);
    printf("perm = %d\n", L.perm ? 1 : 0);
    print("cam_ptr", L.cam_ptr); print("cam_obs", L.cam_obs); print("q_cam", L.q_cam); print("q_pt", L.q_pt); print("pt_ptr", L.pt_ptr); print("pt_pos", L.pt_pos);
    print("new2old", L.new2old);

    const unsigned long long nterms = count_terms(L.pt_ptr, L.pt_pos, L.q_cam);
    Structure st;
    const size_t listed = list_terms(C, L.cam_ptr, L.pt_ptr, L.pt_pos, L.q_cam, L.q_pt, nterms, st);
    if (listed != nterms) { fprintf(stderr, "%zu terms listed, %llu counted\n", listed, nterms); return 1; }
    place_blocks(C, st);
    printf("nterms = %llu\nnlower = %llu\nnblk = %llu\n", nterms, st.nlower, st.nblk);
    print("pt_pos_sorted", L.pt_pos); print("keys", st.keys);
    print("row_ptr", st.row_ptr); print("col", st.col); print("lower", st.lower); print("term_ptr", st.term_ptr); print("terms", st.terms);
    printf("w_bytes = %llu\nterms_bytes = %llu\nstructure_bytes_at_least = %llu\nstructure_bytes = %llu\n", w_bytes(O, W_STRIDE), terms_bytes(O, nterms, W_STRIDE),
           structure_bytes_at_least(C, O, nterms, W_STRIDE), structure_bytes(C, O, nterms, st.nlower, st.nblk, W_STRIDE));

    printf("default_cameras_per_aggregate = %d\n", default_cameras_per_aggregate(C));
    const Aggregates A = greedy_aggregates(C, k > 0 ? k : default_cameras_per_aggregate(C), st.keys, st.term_ptr);
    print("agg", A.agg); print("mem_ptr", A.mem_ptr); print("mem", A.mem);
    const Aggregates G = member_lists(have_given ? given : A.agg);
    print("given_agg", G.agg); print("given_mem_ptr", G.mem_ptr); print("given_mem", G.mem);
    // (the dense and coarse counts take the kernels' leading dimension and panel size: here a leading dimension of n and no panels, the formulas' own terms)
    const long n = 9L * C, nc = 9L * A.count();
    printf("dense_bytes = %llu\ncoarse_bytes = %llu\n", dense_bytes(n, n), coarse_bytes(C, A.count(), nc, nc, 0));
    return 0;
}
