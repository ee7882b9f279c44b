// ba_reduced.hpp -- bundle adjustment's reduced camera system: the host side of the Schur complement on the cameras (ba_schur.hip), its assembled form
// (ba_schur_explicit.hip), the dense Cholesky solve (ba_schur_dense.hip), the two-level preconditioner's coarse correction (ba_coarse.hip) and the marginal
// covariances (ba_covariance.hip).  ONE concrete class: bundle adjustment is the one energy with an eliminable region; a second one can extract an interface when it
// exists.  A plugin that has one returns it from EnergyPlugin::reduced_system(); the driver (solver_forms.cpp) calls it directly.
//
// It owns every buffer of the reduced system -- the elimination factor Ge, y and the held-point word; the structure of S, W and S; the dense triangle; the coarse
// matrices; the covariances' work buffers -- and reads the plugin through ReducedSystemView alone.  The host-side structure is ba_structure.hpp's.
#pragma once
#include "plugin.hpp"

namespace thallo {

// What the reduced system reads of its plugin, filled by the plugin's prepare(): the sizes, the incidence lists and the step's blocks, all on the device and in the plan's
// internal point ids (ba_structure.hpp), and the host's copy of the point order
struct ReducedSystemView {
    int C = 0, P = 0, O = 0;
    const int *cam_ptr = nullptr, *cam_obs = nullptr, *q_cam = nullptr, *q_pt = nullptr, *pt_ptr = nullptr, *pt_pos = nullptr;
    const float *Jb = nullptr, *JP = nullptr;      // the observations' Jacobian blocks in camera order; the point halves packed in point order
    float* JpP = nullptr;                          // the launches' u / v / t scratch
    const std::vector<int>* new2old = nullptr;     // the plan's point j is the caller's (*new2old)[j]; NULL: the caller's order
};

class ReducedCameraSystem {
public:
    explicit ReducedCameraSystem(const ReducedSystemView& view) : v_(view) {}
    ~ReducedCameraSystem();
    ReducedCameraSystem(const ReducedCameraSystem&) = delete;
    ReducedCameraSystem& operator=(const ReducedCameraSystem&) = delete;

    // What an Init asks for.  assembled: S built once per step, the applies multiply by it (kind 2).  dense: that, and a dense Cholesky factor of S in place of the
    // reduced PCG loop (kind 3).  two_level: that, and the coarse correction on S -- aggregates: the caller's (C dense ids, checked) or NULL: greedy aggregates of at most
    // cameras_per_aggregate cameras (0: the default size) built from the structure
    struct Want {
        bool assembled = false, dense = false, two_level = false;
        int cameras_per_aggregate = 0;
        const int* aggregates = nullptr;
    };
    // At Init, behind the plugin's prepare().  The dense triangle and the coarse matrices are part of the structure: counted in its budget (a quarter of the free device
    // memory, read before anything of this call is allocated) before anything is allocated, allocated behind it, freed with it or by the next configure that does not want
    // them; the structure is rebuilt by every configure that wants it and freed by one that does not.  Ge, y and the held word are allocated once, last.  -> 0, or -1 with
    // the reason set (budget, int32 indices, memory): then no form runs
    int configure(const Want& want);
    void retire();      // an Init that runs no Schur form: a running structure goes, the dense and coarse matrices with it

    // ---- every step.  reduce: the elimination factor Ge of the point blocks Hp (+ shift_p; hold: the plan's mask over the flat vector or NULL -- Ge then gets zero rows
    // and columns there) with the held count, y and g = b_c - E y (also into r_out).  assemble, behind reduce on the assembled form: W and S from the step's blocks H and
    // the LM CtC of the cameras (or NULL).  apply: Sx = S x (+ ctc x; the assembled S carries ctc already) and the partials of x . S x -> their number.  back: the points
    // of delta from its cameras (p non-NULL: delta_c += (aN / aD) p first)
    int reduce(LaunchCtx&, const float* Hp, const float* shift_p, const float* b, float* g, float* r_out, const unsigned char* hold);
    int assemble(LaunchCtx&, const float* H, const float* ctc);
    int apply(LaunchCtx&, const float* x, const float* ctc, float* Sx, float* xSx_out, const unsigned* gate);
    int back(LaunchCtx&, const float* b, float* delta, const float* p, thallo_sum_t aN, thallo_sum_t aD);
    // dense form, behind assemble: T = D S D with the identity at the scalars `hold` holds and at non-positive diagonals, T = L L^T, delta_c = D L^-T L^-1 D g -> 0 or a
    // negative launch code
    int dense_solve(LaunchCtx&, const unsigned char* hold, const float* g, float* delta_c);
    // two-level form.  coarse_setup, behind assemble: S_c, its scaling, the factor, Z.  coarse_apply: z += P Z^T Z P^T r, the partials of |Z P^T r|^2 into yy_out -> their number
    int coarse_setup(LaunchCtx&, const unsigned char* hold);
    int coarse_apply(LaunchCtx&, const unsigned char* hold, const float* r, float* z, float* yy_out, const unsigned* gate);

    // ---- marginal covariances, behind the GN set-up of the assembled form at the current unknowns (Plan::covariance): the blocks of the n elements ids (the caller's
    // ids, checked) of Unknown `input` into host_out; Gc: the cameras' block factor.  covariance: batches of 7 cameras or 21 points through the column PCG on S (with the
    // coarse correction where the two-level form runs), whose infos are added up -> 0, or -1 with the reason set.  covariance_dense, on the dense form: S expanded and
    // factored once per call, the columns through the factor -> 0, -1 with the reason set, or -2 with *pivot = the index of the pivot that was not positive.  The work
    // buffers are allocated at the first call and kept
    int covariance(LaunchCtx&, int input, const int* ids, long n, const float* Gc, const unsigned char* hold, float rel_tol, int max_iterations, float* host_out, thallo_cov_info_t* info);
    int covariance_dense(LaunchCtx&, int input, const int* ids, long n, const float* Gc, const unsigned char* hold, float* host_out, thallo_cov_info_t* info, int* pivot);

    // ---- what runs since the last configure
    bool assembled() const { return sx_on_; }
    long blocks() const { return sx_on_ ? sx_nblk_ : -1; }                      // stored blocks of S
    long dense_n() const { return sd_on_ ? 9L * v_.C : -1; }                    // order of the dense matrix (-1: the dense form does not run)
    long coarse_n() const { return cz_on_ ? 9L * cz_K_ : -1; }                  // coarse scalars (-1: the two-level form does not run)
    int  coarse_aggregates() const { return cz_on_ ? cz_K_ : -1; }
    long elements(int input) const { return input == 0 ? v_.C : input == 1 ? v_.P : -1; }      // of Unknown `input` (-1: not one of this energy's)
    const unsigned* held_word() const { return (const unsigned*)held_.ptr; }   // points the last reduce held fixed
    // [0] 1 + the index of the last dense factor's first pivot that was not positive (0: none), [1] the non-positive diagonals, [2] the dense covariance's NaN blocks
    const unsigned* dense_words() const { return sd_on_ ? (const unsigned*)sd_words_.ptr : nullptr; }
    // the last coarse factor's info, the coarse scalars with the identity's row, the factors since Init that met a non-positive pivot
    const unsigned* coarse_words() const { return cz_on_ ? (const unsigned*)cz_words_.ptr : nullptr; }

private:
    const ReducedSystemView& v_;
    DeviceBuffer Ge_, y_, held_;
    // the assembled S: its structure (ba_structure.hpp), W and S
    bool sx_on_ = false;
    long sx_nblk_ = 0; int sx_nlower_ = 0;
    DeviceBuffer sx_row_ptr_, sx_col_, sx_lower_, sx_term_ptr_, sx_terms_, sx_W_, sx_S_;
    // the dense form: the lower triangle T of D S D (ld x 9 C floats, factored in place every step), d and the words
    bool sd_on_ = false;
    long sd_ld_ = 0;
    DeviceBuffer sd_T_, sd_d_, sd_words_;
    // the coarse correction: the aggregates, the dense coarse matrix T (S_c, its scaling, its factor in place), d, Z, Z^T, y, the identity panels of the inverse and the words
    bool cz_on_ = false;
    int cz_K_ = 0;
    DeviceBuffer cz_agg_, cz_mem_ptr_, cz_mem_, cz_T_, cz_d_, cz_Z_, cz_Zt_, cz_y_, cz_panels_, cz_words_;
    // the covariances' work buffers; two pinned host words: the frozen counts of the two chunks in flight
    DeviceBuffer cov_work_, cov_ids_, cov_out_;
    unsigned* cov_pinned_ = nullptr;
    static constexpr int SD_GROUPS = 8;
    DeviceBuffer sdc_panels_, sdc_ids_, sdc_out_;

    int configure_assembled(const Want& want);      // configure's steps 2 - 7: the lists, the count, the budgets, the structure, the aggregates, the device
    void release_dense();
    void release_coarse();
    void release_structure();
    thallo_coarse_t coarse_operands(const unsigned char* hold) const;
    int dense_factor(LaunchCtx&, const unsigned char* hold);      // expand + factor of the step's (or the covariance call's) assembled S
    thallo_cov_sys_t cov_system(const float* Gc, const unsigned char* hold) const;
    std::vector<int> internal_ids(int input, const int* ids, long n) const;      // the caller's ids of Unknown `input` -> the plan's
};

}  // namespace thallo
