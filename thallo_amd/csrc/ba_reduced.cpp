// ba_reduced.cpp -- see ba_reduced.hpp.  DESIGN.md "Schur complement on the cameras", "Assembled reduced camera matrix", "Dense Cholesky Schur solve", "Two-level
// preconditioner", "Marginal covariances".
#include "ba_reduced.hpp"
#include "ba_structure.hpp"
#include <cstdlib>

namespace thallo {

namespace {

// the allowance of a structure and the words that name it in a refusal
struct Budget { unsigned long long allowed; const char* why; };
// ... cut down to an A/B switch's MiB count (THALLO_AB=<label's name>=N) where that is less
Budget capped(Budget b, const char* env_name, const char* label)
{
    if (const char* e = env_switch(env_name)) {
        const unsigned long long cap = strtoull(e, nullptr, 10) << 20;
        if (cap < b.allowed) { b.allowed = cap; b.why = label; }
    }
    return b;
}

bool download(std::vector<int>& h, const int* dev) { return h.empty() || hipMemcpy(h.data(), dev, sizeof(int) * h.size(), hipMemcpyDeviceToHost) == hipSuccess; }

}  // namespace

ReducedCameraSystem::~ReducedCameraSystem() { if (cov_pinned_) (void)hipHostFree(cov_pinned_); }

void ReducedCameraSystem::release_dense() { for (DeviceBuffer* b : { &sd_T_, &sd_d_, &sd_words_ }) b->release(); }
void ReducedCameraSystem::release_coarse() { for (DeviceBuffer* b : { &cz_agg_, &cz_mem_ptr_, &cz_mem_, &cz_T_, &cz_d_, &cz_Z_, &cz_Zt_, &cz_y_, &cz_panels_, &cz_words_ }) b->release(); }
void ReducedCameraSystem::release_structure() { for (DeviceBuffer* b : { &sx_row_ptr_, &sx_col_, &sx_lower_, &sx_term_ptr_, &sx_terms_, &sx_W_, &sx_S_ }) b->release(); }

void ReducedCameraSystem::retire()
{
    if (!sx_on_) return;
    sx_on_ = false; sd_on_ = false; cz_on_ = false;
    release_dense(); release_coarse(); release_structure();
}

int ReducedCameraSystem::configure(const Want& want)
{
    // 1. what is no longer wanted goes; what is wanted again stays allocated until the new one replaces it buffer by buffer
    sx_on_ = false; sd_on_ = false; cz_on_ = false;
    if (!want.assembled || !want.dense) release_dense();
    if (!want.assembled || !want.two_level) release_coarse();
    if (!want.assembled) release_structure();
    else if (configure_assembled(want)) return -1;
    // the elimination factor (the lower triangles of P blocks of 3 x 3), y and the held word: once, behind the structure -- its budget is read without them
    if (Ge_.ptr) return 0;
    const size_t np = (size_t)v_.P, ns = 3;
    if (Ge_.alloc((ns * (ns + 1) / 2 * np + 64) * sizeof(float)) || y_.alloc((ns * np + 64) * sizeof(float)) || held_.alloc(64)) {
        for (DeviceBuffer* b : { &Ge_, &y_, &held_ }) b->release();
        set_error("bundle_adjustment: out of device memory for the Schur-complement solve"); return -1;
    }
    return 0;
}

// The symbolic structure is built on the host from the incidence lists as the device holds them (the plan's internal ids, a renumbered plan included)
int ReducedCameraSystem::configure_assembled(const Want& want)
{
    const int C = v_.C, P = v_.P, O = v_.O;
    if (C < 1) { set_error("bundle_adjustment: the assembled Schur-complement solve needs at least one camera"); return -1; }
    // 2. the lists
    std::vector<int> pp((size_t)P + 1), ppos((size_t)O), qc((size_t)O), qp((size_t)O), cp((size_t)C + 1);
    if (!download(pp, v_.pt_ptr) || !download(ppos, v_.pt_pos) || !download(qc, v_.q_cam) || !download(qp, v_.q_pt) || !download(cp, v_.cam_ptr)) { set_error("bundle_adjustment: cannot read the incidence lists"); return -1; }
    // 3. the terms, counted before anything is built
    const unsigned long long nterms = ba::count_terms(pp, ppos, qc);
    // 4. the budgets.  The allowance: a quarter of the free device memory (the rule of the ring of p planes), or less (THALLO_AB=schur_s_max_mb=N)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { set_error("bundle_adjustment: cannot read the free device memory"); return -1; }
    const Budget budget = capped({ free_b / 4, "a quarter of the free device memory" }, "THALLO_SCHUR_S_MAX_MB", "THALLO_AB schur_s_max_mb");
    const unsigned long long allowed = budget.allowed; const char* why = budget.why;
    // the dense form's bytes: known from C alone, refused first
    const long sd_n = 9L * C, sd_ld = thallo_hip_dense_ld(sd_n);
    const unsigned long long dense_bytes = want.dense ? ba::dense_bytes(sd_n, sd_ld) : 0;
    if (want.dense) {
        if (sd_n > THALLO_HIP_DENSE_MAX_N) { set_error("bundle_adjustment: the dense reduced camera matrix has n = %ld, more than the dense kernels take (%ld)", sd_n, (long)THALLO_HIP_DENSE_MAX_N); return -1; }
        const Budget dense = capped(budget, "THALLO_SCHUR_DENSE_MAX_MB", "THALLO_AB schur_dense_max_mb");
        if (dense_bytes > dense.allowed) {
            set_error("bundle_adjustment: the dense reduced camera matrix wants %llu bytes of device memory (n = %ld scalars, leading dimension %ld), the budget allows %llu (%s): "
                      "THALLOX_SOLVER_SCHUR_EXPLICIT_PCG solves on the block-sparse S without it", dense_bytes, sd_n, sd_ld, dense.allowed, dense.why);
            return -1;
        }
    }
    auto over = [&](unsigned long long bytes, unsigned long long blocks, const char* least) {
        if (want.dense)
            set_error("bundle_adjustment: the assembled reduced camera matrix and its dense lower triangle want %s%llu bytes of device memory (%s%llu blocks of 9 x 9, %llu terms, %d observations; "
                      "%llu bytes dense, n = %ld), the budget allows %llu (%s): THALLOX_SOLVER_SCHUR_PCG applies S without assembling it", least, bytes, least, blocks, nterms, O, dense_bytes, sd_n, allowed, why);
        else
            set_error("bundle_adjustment: the assembled reduced camera matrix wants %s%llu bytes of device memory (%s%llu blocks of 9 x 9, %llu terms, %d observations), the budget allows %llu (%s): "
                      "points seen by many cameras make the term count grow with the square of the track length; THALLOX_SOLVER_SCHUR_PCG applies S without assembling it",
                      least, bytes, least, blocks, nterms, O, allowed, why);
        return -1;
    };
    const int ws = THALLO_HIP_SCHUR_W_STRIDE;
    if (nterms > 0x7fffffffULL) { set_error("bundle_adjustment: the assembled reduced camera matrix has %llu terms, more than its int32 indices hold", nterms); return -1; }
    if (ba::terms_bytes(O, nterms, ws) + dense_bytes > allowed) return over(ba::structure_bytes_at_least(C, O, nterms, ws) + dense_bytes, (unsigned long long)C, "at least ");      // (the blocks are not counted yet)
    // 5. the blocks and their terms
    ba::Structure st;
    const size_t listed = ba::list_terms(C, cp, pp, ppos, qc, qp, nterms, st);
    if (listed != nterms) { set_error("bundle_adjustment: internal: %zu terms listed, %llu counted", listed, nterms); return -1; }
    const unsigned long long nlower = st.nlower, nblk = st.nblk;
    if (nblk > 0x7fffffffULL / 3) { set_error("bundle_adjustment: the assembled reduced camera matrix has %llu blocks, more than its int32 indices hold", nblk); return -1; }
    // 6. the coarse correction: its aggregates come from the blocks just listed; its bytes -- T, Z, Z^T, the identity panels, d, y, the lists, the words -- join the count
    ba::Aggregates cz;
    unsigned long long coarse_bytes = 0;
    long cz_n = 0, cz_ld = 0;
    if (want.two_level) {
        cz = want.aggregates ? ba::member_lists(std::vector<int>(want.aggregates, want.aggregates + C))
                             : ba::greedy_aggregates(C, want.cameras_per_aggregate > 0 ? want.cameras_per_aggregate : ba::default_cameras_per_aggregate(C), st.keys, st.term_ptr);
        cz_K_ = cz.count();
        cz_n = 9L * cz_K_; cz_ld = thallo_hip_dense_ld(cz_n);
        if (cz_n > THALLO_HIP_COARSE_MAX_N) {
            set_error("bundle_adjustment: the two-level preconditioner's coarse space has n_c = %ld scalars (%d aggregates), more than its kernels take (%d): use larger aggregates "
                      "(ThalloX_PlanSetCoarseAggregates)", cz_n, cz_K_, THALLO_HIP_COARSE_MAX_N);
            return -1;
        }
        coarse_bytes = ba::coarse_bytes(C, cz_K_, cz_n, cz_ld, thallo_hip_ba_coarse_panel_floats(cz_n));
    }
    const unsigned long long bytes = ba::structure_bytes(C, O, nterms, nlower, nblk, ws) + dense_bytes + coarse_bytes;
    if (bytes > allowed && want.two_level) {
        set_error("bundle_adjustment: the assembled reduced camera matrix and the two-level preconditioner's coarse matrices want %llu bytes of device memory (%llu blocks of 9 x 9, %llu terms, "
                  "%d observations; %llu bytes coarse, %d aggregates, n_c = %ld), the budget allows %llu (%s)", bytes, nblk, nterms, O, coarse_bytes, cz_K_, cz_n, allowed, why);
        return -1;
    }
    if (bytes > allowed) return over(bytes, nblk, "");
    ba::place_blocks(C, st);
    // 7. on the device: the structure, then the dense triangle, then the coarse matrices
    if (sx_row_ptr_.upload(st.row_ptr) || sx_col_.upload(st.col) || sx_lower_.upload(st.lower) || sx_term_ptr_.upload(st.term_ptr) || sx_terms_.upload(st.terms) ||
        sx_W_.alloc((size_t)ba::w_bytes(O, ws)) || sx_S_.alloc(sizeof(float) * 81 * (size_t)nblk + 64)) {
        const std::string whyn = last_error();
        set_error("bundle_adjustment: out of device memory for the assembled reduced camera matrix (%llu bytes): %s", bytes, whyn.c_str());
        return -1;
    }
    if (want.dense && (sd_T_.alloc(4 * (size_t)sd_ld * (size_t)sd_n + 64) || sd_d_.alloc(4 * (size_t)sd_n + 64) || sd_words_.alloc(64))) {
        const std::string whyn = last_error();
        release_dense();
        set_error("bundle_adjustment: out of device memory for the dense reduced camera matrix (%llu bytes): %s", dense_bytes, whyn.c_str());
        return -1;
    }
    if (want.two_level) {
        const size_t tz = 4 * (size_t)cz_ld * (size_t)cz_n + 64;
        if (cz_agg_.upload(cz.agg) || cz_mem_ptr_.upload(cz.mem_ptr) || cz_mem_.upload(cz.mem) || cz_T_.alloc(tz) || cz_Z_.alloc(tz) || cz_Zt_.alloc(tz) || cz_d_.alloc(4 * (size_t)cz_n + 64) ||
            cz_y_.alloc(4 * (size_t)cz_n + 64) || cz_panels_.alloc(4 * (size_t)thallo_hip_ba_coarse_panel_floats(cz_n) + 64) || cz_words_.alloc(64) ||
            hipMemset(cz_words_.ptr, 0, 64) != hipSuccess) {
            const std::string whyn = last_error();
            release_coarse();
            set_error("bundle_adjustment: out of device memory for the two-level preconditioner's coarse matrices (%llu bytes): %s", coarse_bytes, whyn.c_str());
            return -1;
        }
    }
    sx_nblk_ = (long)nblk; sx_nlower_ = (int)nlower; sx_on_ = true; sd_on_ = want.dense; sd_ld_ = sd_ld; cz_on_ = want.two_level;
    return 0;
}

// ------------------------------------------------------------------ every step
// the launches load the camera half of Jb (what block_diag summed), the packed point blocks JP, and use JpP as their u / v / t scratch
int ReducedCameraSystem::reduce(LaunchCtx& c, const float* Hp, const float* shift_p, const float* b, float* g, float* r_out, const unsigned char* hold)
{
    float* Ge = (float*)Ge_.ptr;
    { TimedLaunch t(c, "SchurFactor"); const int rc = thallo_hip_ba_schur_factor(v_.P, Hp, shift_p, Ge, (unsigned*)held_.ptr, c.stream); if (rc < 0) return rc; }
    if (hold) {
        TimedLaunch t(c, "BlockHoldFactor");
        thallo_block_regions_t pts; pts.n = 1;      // (the points' blocks: 3 x 3 each, behind the cameras' scalars in the flat vector)
        pts.r[0] = { 9L * v_.C, 3, v_.P }; pts.r[1] = pts.r[0];
        for (int i = 2; i < THALLO_HIP_MAX_BLOCK_REGIONS; ++i) pts.r[i] = { 0L, 3, 0 };
        const int rc = thallo_hip_block_hold_factor(pts, hold, Ge, c.stream); if (rc < 0) return rc;
    }
    TimedLaunch t(c, "SchurReduce");
    return thallo_hip_ba_schur_rhs(v_.C, v_.P, v_.cam_ptr, v_.pt_ptr, v_.pt_pos, v_.Jb, v_.JP, Ge, b, (float*)y_.ptr, v_.JpP, g, r_out, c.stream);
}

int ReducedCameraSystem::assemble(LaunchCtx& c, const float* H, const float* ctc)
{
    if (!sx_on_) return -1;
    { TimedLaunch t(c, "SchurW"); const int rc = thallo_hip_ba_schur_w(v_.O, v_.P, v_.q_pt, v_.Jb, (const float*)Ge_.ptr, (float*)sx_W_.ptr, c.stream); if (rc < 0) return rc; }
    TimedLaunch t(c, "SchurAssemble");
    return thallo_hip_ba_schur_assemble(v_.C, sx_nlower_, sx_nblk_, (const int*)sx_lower_.ptr, (const int*)sx_term_ptr_.ptr, (const int*)sx_terms_.ptr, (const float*)sx_W_.ptr, H, ctc,
                                        (float*)sx_S_.ptr, c.stream);
}

int ReducedCameraSystem::apply(LaunchCtx& c, const float* x, const float* ctc, float* Sx, float* out, const unsigned* gate)
{
    if (sx_on_) {      // (ctc is in the assembled diagonal blocks already)
        TimedLaunch t(c, "SchurApplyS");
        return thallo_hip_ba_schur_apply_s(v_.C, sx_nblk_, (const int*)sx_row_ptr_.ptr, (const int*)sx_col_.ptr, (const float*)sx_S_.ptr, x, Sx, out, gate, c.stream);
    }
    TimedLaunch t(c, "SchurApply");
    return thallo_hip_ba_schur_apply(v_.C, v_.P, v_.cam_ptr, v_.pt_ptr, v_.pt_pos, v_.Jb, v_.JP, (const float*)Ge_.ptr, x, ctc, v_.JpP, Sx, out, gate, c.stream);
}

int ReducedCameraSystem::back(LaunchCtx& c, const float* b, float* delta, const float* p, thallo_sum_t aN, thallo_sum_t aD)
{
    TimedLaunch t(c, "SchurBack");
    return thallo_hip_ba_schur_back(v_.C, v_.P, v_.cam_ptr, v_.pt_ptr, v_.pt_pos, v_.Jb, v_.JP, (const float*)Ge_.ptr, b, delta, p, aN, aD, v_.JpP, c.stream);
}

// hold: the plan's mask over the flat vector (its first 9 C bytes are the cameras') or NULL
int ReducedCameraSystem::dense_factor(LaunchCtx& c, const unsigned char* hold)
{
    if (!sd_on_) return -1;
    unsigned* words = (unsigned*)sd_words_.ptr;
    {   TimedLaunch t(c, "SchurDenseExpand");
        const int rc = thallo_hip_ba_schur_dense_expand(v_.C, sx_nblk_, (const int*)sx_row_ptr_.ptr, (const int*)sx_col_.ptr, (const float*)sx_S_.ptr, hold, sd_ld_, (float*)sd_T_.ptr, (float*)sd_d_.ptr,
                                                        words + 1, c.stream);
        if (rc < 0) return rc; }
    TimedLaunch t(c, "SchurDenseFactor");
    return thallo_hip_dense_potrf(9L * v_.C, sd_ld_, (float*)sd_T_.ptr, (int*)words, c.stream);
}

int ReducedCameraSystem::dense_solve(LaunchCtx& c, const unsigned char* hold, const float* g, float* delta_c)
{
    const int rc = dense_factor(c, hold);
    if (rc < 0) return rc;
    TimedLaunch t(c, "SchurDenseSolve");
    return thallo_hip_dense_potrs_vec(9L * v_.C, sd_ld_, (const float*)sd_T_.ptr, (const float*)sd_d_.ptr, g, delta_c, THALLO_HIP_DENSE_BOTH, c.stream);
}

thallo_coarse_t ReducedCameraSystem::coarse_operands(const unsigned char* hold) const
{
    thallo_coarse_t c;
    c.C = v_.C; c.K = cz_K_; c.n = 9L * cz_K_; c.ld = thallo_hip_dense_ld(c.n); c.agg = (const int*)cz_agg_.ptr; c.mem_ptr = (const int*)cz_mem_ptr_.ptr; c.mem = (const int*)cz_mem_.ptr;
    c.hold = hold; c.T = (float*)cz_T_.ptr; c.d = (float*)cz_d_.ptr; c.Z = (float*)cz_Z_.ptr; c.Zt = (float*)cz_Zt_.ptr; c.y = (float*)cz_y_.ptr; c.words = (unsigned*)cz_words_.ptr;
    return c;
}

int ReducedCameraSystem::coarse_setup(LaunchCtx& c, const unsigned char* hold)
{
    if (!cz_on_) return -1;
    const thallo_coarse_t cz = coarse_operands(hold);
    int rc;
    {   TimedLaunch t(c, "CoarseAssemble");
        if ((rc = thallo_hip_ba_coarse_assemble(&cz, sx_nblk_, (const int*)sx_row_ptr_.ptr, (const int*)sx_col_.ptr, (const float*)sx_S_.ptr, c.stream)) < 0) return rc; }
    { TimedLaunch t(c, "CoarseScale"); if ((rc = thallo_hip_ba_coarse_scale(&cz, c.stream)) < 0) return rc; }
    { TimedLaunch t(c, "CoarseFactor"); if ((rc = thallo_hip_dense_potrf(cz.n, cz.ld, cz.T, (int*)cz.words, c.stream)) < 0) return rc; }
    TimedLaunch t(c, "CoarseInverse");
    return thallo_hip_ba_coarse_inverse(&cz, (float*)cz_panels_.ptr, c.stream);
}

int ReducedCameraSystem::coarse_apply(LaunchCtx& c, const unsigned char* hold, const float* r, float* z, float* yy_out, const unsigned* gate)
{
    if (!cz_on_) return -1;
    const thallo_coarse_t cz = coarse_operands(hold);
    TimedLaunch t(c, "CoarseApply");
    return thallo_hip_ba_coarse_apply(&cz, r, z, yy_out, gate, c.stream);
}

// ------------------------------------------------------------------ marginal covariances
// S, W and the lists of this step's set-up, both factors and the mask
thallo_cov_sys_t ReducedCameraSystem::cov_system(const float* Gc, const unsigned char* hold) const
{
    thallo_cov_sys_t sys;
    sys.C = v_.C; sys.P = v_.P; sys.nblk = sx_nblk_; sys.row_ptr = (const int*)sx_row_ptr_.ptr; sys.col = (const int*)sx_col_.ptr; sys.S = (const float*)sx_S_.ptr;
    sys.Gc = Gc; sys.Ge = (const float*)Ge_.ptr; sys.W = (const float*)sx_W_.ptr; sys.pt_ptr = v_.pt_ptr; sys.pt_pos = v_.pt_pos; sys.q_cam = v_.q_cam; sys.hold = hold;
    return sys;
}

// the caller's point ids become the plan's as a mask of held points is mapped
std::vector<int> ReducedCameraSystem::internal_ids(int input, const int* ids, long n) const
{
    std::vector<int> in(ids, ids + n);
    if (input == 1 && v_.new2old) {
        const std::vector<int>& new2old = *v_.new2old;
        std::vector<int> old2new((size_t)v_.P);
        for (int j = 0; j < v_.P; ++j) old2new[(size_t)new2old[(size_t)j]] = j;
        for (long i = 0; i < n; ++i) in[(size_t)i] = old2new[(size_t)ids[i]];
    }
    return in;
}

int ReducedCameraSystem::covariance(LaunchCtx& c, int input, const int* ids, long n, const float* Gc, const unsigned char* hold, float rel_tol, int max_iterations, float* host_out,
                                    thallo_cov_info_t* info)
{
    if (!sx_on_) { set_error("bundle_adjustment: a covariance needs the assembled reduced camera matrix"); return -1; }
    const int per = input == 0 ? THALLO_HIP_COV_K / 9 : THALLO_HIP_COV_K / 3, fl = input == 0 ? 81 : 9;
    const long cov_bytes = thallo_hip_ba_cov_coarse_work_bytes(v_.C, cz_on_ ? 9L * cz_K_ : 0);
    if (cov_work_.ptr && cov_work_.bytes < (size_t)cov_bytes) cov_work_.release();      // (a re-Init switched the two-level form on, or to more aggregates)
    if (!cov_work_.ptr && (cov_work_.alloc((size_t)cov_bytes) || cov_ids_.alloc(sizeof(int) * THALLO_HIP_COV_K) ||
                           cov_out_.alloc(sizeof(float) * 81 * (THALLO_HIP_COV_K / 9) + 64))) {
        for (DeviceBuffer* b : { &cov_work_, &cov_ids_, &cov_out_ }) b->release();
        set_error("bundle_adjustment: out of device memory for the covariance's work vectors (%ld bytes)", cov_bytes); return -1;
    }
    if (!cov_pinned_ && hipHostMalloc((void**)&cov_pinned_, 4 * sizeof(unsigned), hipHostMallocDefault) != hipSuccess) { cov_pinned_ = nullptr; (void)hipGetLastError(); }      // (without them: a blocking read per chunk)
    const std::vector<int> in = internal_ids(input, ids, n);
    const thallo_cov_sys_t sys = cov_system(Gc, hold);
    *info = thallo_cov_info_t{ 0, 0, 0, 0, 0.0f };
    thallo_coarse_t cz{};
    if (cz_on_) cz = coarse_operands(hold);      // (the two-level preconditioner of the plan's last Init: its Z is this call's set-up's)
    for (long b0 = 0; b0 < n; b0 += per) {
        const int nreq = (int)(n - b0 < per ? n - b0 : per);
        thallo_cov_info_t bi;
        if (hipMemcpyAsync(cov_ids_.ptr, in.data() + b0, sizeof(int) * (size_t)nreq, hipMemcpyHostToDevice, c.stream) != hipSuccess) { set_error("bundle_adjustment: cannot upload the covariance's ids"); return -1; }
        const int rc = thallo_hip_ba_cov_solve_coarse(&sys, cz_on_ ? &cz : nullptr, input, (const int*)cov_ids_.ptr, nreq, rel_tol, max_iterations, cov_work_.ptr, cov_pinned_,
                                                      (float*)cov_out_.ptr, &bi, c.stream);
        if (rc < 0) { set_error("bundle_adjustment: the covariance's column solve failed (%d)", rc); return -1; }
        if (hipMemcpyAsync(host_out + (size_t)fl * (size_t)b0, cov_out_.ptr, sizeof(float) * (size_t)fl * (size_t)nreq, hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
            hipStreamSynchronize(c.stream) != hipSuccess) { set_error("bundle_adjustment: cannot read the covariance blocks"); return -1; }
        info->iterations += bi.iterations; info->columns += bi.columns; info->not_converged += bi.not_converged; info->nan_blocks += bi.nan_blocks;
        if (!(bi.worst <= info->worst)) info->worst = bi.worst;
    }
    return 0;
}

// Per group of up to SD_GROUPS batches thallo_hip_ba_cov_rhs per batch, ONE thallo_hip_dense_potrs_cols launch (a workgroup per batch) and thallo_hip_ba_cov_out per
// batch.  info->not_converged: the requested camera columns at scalars whose diagonal is not positive
int ReducedCameraSystem::covariance_dense(LaunchCtx& c, int input, const int* ids, long n, const float* Gc, const unsigned char* hold, float* host_out, thallo_cov_info_t* info, int* pivot)
{
    if (!sd_on_) { set_error("bundle_adjustment: the dense covariance needs the dense reduced camera matrix"); return -1; }
    const int K = THALLO_HIP_COV_K, per = input == 0 ? K / 9 : K / 3, fl = input == 0 ? 81 : 9;
    const long sd_n = 9L * v_.C, pn = sd_n * K;
    const long nbatch = (n + per - 1) / per;
    const int groups = (int)(nbatch < SD_GROUPS ? nbatch : SD_GROUPS);
    if (sdc_panels_.bytes < sizeof(float) * (size_t)pn * (size_t)groups + 64 &&
        (sdc_panels_.alloc(sizeof(float) * (size_t)pn * (size_t)groups + 64) || sdc_ids_.alloc(sizeof(int) * K * SD_GROUPS) || sdc_out_.alloc(sizeof(float) * 81 * (K / 9) * SD_GROUPS + 64))) {
        for (DeviceBuffer* b : { &sdc_panels_, &sdc_ids_, &sdc_out_ }) b->release();
        set_error("bundle_adjustment: out of device memory for the dense covariance's panels (%zu bytes)", sizeof(float) * (size_t)pn * (size_t)groups); return -1;
    }
    int rc = dense_factor(c, hold);
    if (rc < 0) { set_error("bundle_adjustment: the dense covariance's expansion or factor failed to launch (%d)", rc); return -1; }
    unsigned words[2] = { 0, 0 };
    std::vector<float> dh((size_t)sd_n);
    std::vector<unsigned char> hh(hold ? (size_t)sd_n : 0);
    if (hipMemcpyAsync(words, sd_words_.ptr, sizeof(words), hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
        hipMemcpyAsync(dh.data(), sd_d_.ptr, sizeof(float) * (size_t)sd_n, hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
        (hold && hipMemcpyAsync(hh.data(), hold, (size_t)sd_n, hipMemcpyDeviceToHost, c.stream) != hipSuccess) ||
        hipStreamSynchronize(c.stream) != hipSuccess) { set_error("bundle_adjustment: cannot read the dense factor's status"); return -1; }
    if (words[0]) { *pivot = (int)words[0] - 1; return -2; }
    const std::vector<int> in = internal_ids(input, ids, n);
    const thallo_cov_sys_t sys = cov_system(Gc, hold);
    *info = thallo_cov_info_t{ 0, 0, 0, 0, 0.0f };
    unsigned* nan_word = (unsigned*)sd_words_.ptr + 2;
    if (hipMemsetAsync(nan_word, 0, sizeof(unsigned), c.stream) != hipSuccess) { set_error("bundle_adjustment: cannot clear the dense covariance's NaN count"); return -1; }
    for (long g0 = 0; g0 < nbatch; g0 += groups) {
        const int ng = (int)(nbatch - g0 < groups ? nbatch - g0 : groups);
        const long first = g0 * per, last = first + (long)ng * per < n ? first + (long)ng * per : n;
        auto nreq_of = [&](int g) { const long b0 = first + (long)g * per; return (int)(last - b0 < per ? last - b0 : per); };
        std::vector<int> padded((size_t)ng * (size_t)K, 0);      // (a batch's ids at a stride of K)
        for (int g = 0; g < ng; ++g) for (int j = 0; j < nreq_of(g); ++j) padded[(size_t)g * K + (size_t)j] = in[(size_t)(first + (long)g * per + j)];
        if (hipMemcpy(sdc_ids_.ptr, padded.data(), sizeof(int) * padded.size(), hipMemcpyHostToDevice) != hipSuccess) { set_error("bundle_adjustment: cannot upload the covariance's ids"); return -1; }
        for (int g = 0; g < ng; ++g)
            if ((rc = thallo_hip_ba_cov_rhs(&sys, input, (const int*)sdc_ids_.ptr + (size_t)g * K, nreq_of(g), (float*)sdc_panels_.ptr + (size_t)g * (size_t)pn, c.stream)) < 0) break;
        if (rc >= 0) rc = thallo_hip_dense_potrs_cols(sd_n, sd_ld_, (const float*)sd_T_.ptr, (const float*)sd_d_.ptr, (float*)sdc_panels_.ptr, ng, THALLO_HIP_DENSE_BOTH, c.stream);
        for (int g = 0; g < ng && rc >= 0; ++g)
            rc = thallo_hip_ba_cov_out(&sys, input, (const int*)sdc_ids_.ptr + (size_t)g * K, nreq_of(g), (const float*)sdc_panels_.ptr + (size_t)g * (size_t)pn,
                                       (float*)sdc_out_.ptr + (size_t)g * (size_t)fl * (size_t)per, nan_word, c.stream);
        if (rc < 0) { set_error("bundle_adjustment: the dense covariance's column solve failed (%d)", rc); return -1; }
        if (hipMemcpyAsync(host_out + (size_t)fl * (size_t)first, sdc_out_.ptr, sizeof(float) * (size_t)fl * (size_t)(last - first), hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
            hipStreamSynchronize(c.stream) != hipSuccess) { set_error("bundle_adjustment: cannot read the covariance blocks"); return -1; }
    }
    unsigned nans = 0;
    if (hipMemcpy(&nans, nan_word, sizeof(nans), hipMemcpyDeviceToHost) != hipSuccess) { set_error("bundle_adjustment: cannot read the covariance's NaN count"); return -1; }
    info->nan_blocks = (int)nans;
    if (input == 0) {
        for (long i = 0; i < n; ++i)
            for (int a = 0; a < 9; ++a) {
                const size_t u = 9 * (size_t)ids[i] + (size_t)a;
                if (hold && hh[u]) continue;                                  // (a held scalar's unit column is zero and needs no solve)
                if (dh[u] > 0.0f) info->columns++; else info->not_converged++;
            }
    } else info->columns = (int)(3 * n) - 3 * (int)nans;
    return 0;
}

}  // namespace thallo
