// solver.hpp -- Gauss-Newton / Levenberg-Marquardt outer step + PCG inner loop (host driver).
// Restates API/src/gauss_newton.t:1166-1198 (init), :1545-1785 (step), :1200-1212 (finalize),
// :1787-1799 (cost / summary), :1806-1862 (solver parameters), :1963-2071 (makePlan) for the
// fused MI355X schedule documented in DESIGN.md.
#pragma once
#include "plugin.hpp"
#include "ba_reduced.hpp"
#include "rccl_transport.hpp"
#include "../../include/Thallo.h"

namespace thallo {

#define HIP_OK(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) set_error("%s failed: %s", #call, hipGetErrorString(e__)); } while (0)

struct SolverParameters {   // gauss_newton.t:200-216, defaults :41-55
    float min_relative_decrease = 1e-3f;
    float min_trust_region_radius = 1e-32f;
    float max_trust_region_radius = 1e16f;
    float q_tolerance = 0.0001f;
    float function_tolerance = 0.000001f;
    float trust_region_radius = 1e4f;
    float radius_decrease_factor = 2.0f;
    float min_lm_diagonal = 1e-6f;
    float max_lm_diagonal = 1e32f;
    float max_solver_time_in_seconds = 0.0f;
    int residual_reset_period = 10;
    int nIter = 0;
    int nIterations = 10;
    int lIterations = 10;
};

// util.Timer (util.t:446-541) with hipEvents; names as in gauss_newton.t:1173,1563-1564,1611,1690
class CoarseTimer {
public:
    struct Info { std::string name; hipEvent_t start, end; bool owns_start = true, owns_end = true; };
    std::vector<Info> events;
    bool enabled = true;      // Thallo_InitializationParameters.timingLevel 0 = "No timing recorded" (Thallo.h): no events at all -- an event record is a barrier packet between two launches
    int  start(const char* name, hipStream_t s);
    void stop(int idx, hipStream_t s);
    // One record per distinct stream position (an event record is a barrier packet between two launches):
    int  start_with(int outer, const char* name, hipStream_t s);    // start(name) right behind start(outer), nothing enqueued between them: the new interval starts at outer's start event
    int  stop_start(int idx, const char* name, hipStream_t s);      // stop(idx) and start(name) with nothing enqueued between them: the new interval starts at idx's end event
    void stop_both(int idx, int outer, hipStream_t s);              // stop(idx) and stop(outer) at one position: outer ends at idx's end event
    void evaluate(Thallo_PerformanceSummary* out, bool print_table, KernelTimer* kt);
    void cleanup();
    ~CoarseTimer() { cleanup(); }
};

// Multi-GPU state of a Plan (one process per GPU; SURVEY.md 8e -- the reference is single-device, util.t:769-772, so this is new design).  solver_dist.cpp.
// The form a plan runs in across ranks: chosen once, by Plan::dist_pick_form, from what the plugin can do.
enum class DistForm {
    Slab,       // image_warping's row slabs: the Plan was made for the LOCAL image {W, owned rows + ghost rows}; rows [row0,row1) are owned.  Per PCG iteration ONE kernel +
                // ONE exchange: either the caller's all-gather (RCCL) of [alphaD, N, S1, S2 | boundary rows of Ap], or -- after a self-check on this very topology -- device
                // mailboxes + peer-to-peer ghost-row stores done by the kernel itself (dist_device.hpp)
    Flat,       // row slabs of single-image energies with apply_jtj_sums (shape_from_shading, generated stencils): vectors stay where the Plan allocated them
    Range,      // graph domains (ARAP): every rank holds the whole problem and FULL-length vectors and owns the contiguous unit range [row0, row1) (units = vertices), equal on all ranks
    Partition,  // ... or (ThalloX_PlanSetGhostExchange) the rank holds its owned units [0, row1) + ghost units; only the boundary units' values travel
    Shard       // bundle adjustment's camera shards: the unknowns [sh_off, sh_off + sh_len) (the points) are replicated; their J^T F / diag / A p are partial sums over the
                // rank's residuals and are all-reduced; sums over them are taken after that, by every rank for itself
};
struct DistState {
    ThalloX_Distributed cfg;
    DistForm form = DistForm::Slab;
    // What the call sites ask of the form (the four booleans these replace: flat = Flat; range = Range, Partition, Shard; part = Partition; shard = Shard):
    //                      Slab  Flat  Range  Partition  Shard
    //   full_vectors()      -     -     x       x         x     was `range`: linear updates and the like cover the whole local vector, not the owned rows
    //   flat_exchange()     -     x     -       x         x     was `flat || shard || part`: the device-side exchange is a launch of its own (xrows / xunits / allreduce)
    //   runs_lm()           -     x     -       -         x     was `shard || (flat && !range)`: Levenberg-Marquardt runs across ranks
    // `form == DistForm::Slab` was `!flat && !range` (with or without `&& !shard`, `&& !part`: both imply range)
    bool full_vectors() const { return form == DistForm::Range || form == DistForm::Partition || form == DistForm::Shard; }
    bool flat_exchange() const { return form == DistForm::Flat || form == DistForm::Partition || form == DistForm::Shard; }
    bool runs_lm() const { return form == DistForm::Flat || form == DistForm::Shard; }
    // ---- every form
    DeviceBuffer send, gath;                             // message buffers (floats), sized for the larger of the two message kinds
    long msg = 0, msg_iter = 0, msg_x = 0;
    int Hl = 0, row0 = 0, row1 = 0;                      // row forms: the local image's rows, [row0,row1) owned; unit forms: units, [row0,row1) owned
    // ---- Slab and Flat: the rows
    int W = 0, top = 0, bot = 0, ghost = 1;
    long N = 0, na = 0;
    // ---- Slab
    void* block = nullptr; bool block_ipc = false;      // [r | z | r' | Ap | Ap'] (one allocation peers can map)
    unsigned char handle_block[64];
    thallo_segs_t seg_first_last, seg_top, seg_bot, seg_iter_fl, seg_iter_top, seg_iter_bot;
    bool resident_all = false;                           // EVERY rank's slab fits the resident PCG kernel (agreed once per Init: a rank whose last segment cannot be a full one says no)
    int mail_L = 0;
    long ghost_off = 0;                                  // byte offset of the resident kernel's ghost area inside every rank's mailbox block (0: none)
    int defer_state = -1;                                // the deferred cross-rank finish: -1 not agreed on yet, 0 no, 1 every rank runs it
    DeviceBuffer gs;                                     // two tagged granules: the global words a launch's designated wave publishes for its other waves (deferred cross-rank finish)
    thallo_dist_t d_iter[2];
    // ---- Flat
    long rowlen = 0;                                     // floats per image row
    thallo_segs_t seg_rows_fl, seg_rows_top, seg_rows_bot;   // first / last `ghost` owned rows; the ghost rows above / below
    thallo_segs_t seg_rows_first, seg_rows_last;             // ... the first and the last owned rows separately (device-side exchange: one goes up, one goes down)
    // ---- Range and Partition.  pieces = rank 0's owned slice of every plane of the flat vector (rank r's: + r * len)
    thallo_segs_t pieces_first, pieces_mine;
    long piece_floats = 0;                               // floats a rank owns in a flat vector
    // ---- Partition
    DeviceBuffer g_boundary, g_ghost, g_src1, g_src7, g_srcx;   // device copies of the index lists; element offsets of the ghosts' sources for the two message kinds
                                                                // (g_srcx: the ghosts' sources inside this rank's device-side inbox)
    thallo_units_t u_send, u_recv1, u_recv7;
    thallo_units_t u_recvx; long unit_slot = 0;          // device-side exchange of the partition form (thallo_hip_dist_xunits)
    // ---- Shard
    long sh_off = 0, sh_len = 0;
    DeviceBuffer sh_aD, sh_s3;                           // the shared block's partials of an iteration
    DeviceBuffer sh_lm;                                  // ... of the second sum of an LM exchange (q next to betaN, delta.b next to delta.J^T J delta)
    thallo_xreduce_t xa;                                 // device-side all-reduce of the shared block (thallo_hip_dist_allreduce): inbox geometry
    // ---- device-side exchange, every form that has one
    bool want_p2p = false, mapped = false, p2p_on = false, checked = false;
    thallo_xrows_t xr;                                   // Flat, Partition, Shard: inbox geometry, neighbours (thallo_hip_dist_xrows / xunits / xscalars_shard)
    bool xrows_now = false;                              // Flat, Partition: the transport dist_sum_slot / dist_sum_and_rows / dist_gn_flat / dist_ghosts use right now (= p2p_on outside the self-check)
    void* mail = nullptr;
    unsigned char handle_mail[64];
    int mem_kind[2] = { -1, -1 };                        // of the block, of the mailbox: 1 fine-grained
    DeviceBuffer ctl;
    thallo_dist_t d;
    std::vector<void*> opened;
    // ---- what distributed_info() says: facts here, the JSON rendered from them (Plan::dist_render_info) after set-up, after the self-check and after a switch-off
    std::string form_text;                               // "form" (the Slab form has none)
    struct SelfCheck {                                   // the outcome of dist_self_check, if it ran
        bool ran = false, pass = false, all = false, resident_loop = false;
        int count = 0, timeout = 0;                      // exchanges (Slab: PCG iterations) run; 0, or which bounded wait ran out
        double rel = 0.0;                                // Slab: largest relative difference of the alpha / beta scalars between the two transports
        unsigned pm[5] = { 0, 0, 0, 0, 0 };
    } check;
    bool switched_off = false;                           // dist_control(1, 0) took a passing device-side exchange out of use
    std::string info;
    // A rank-local failure (a launch, a copy, an allocation at Step time) must not end this rank's part of the collective sequence -- the other
    // ranks would wait in the matching all-gather forever.  From the first failure on the rank skips its own launches, keeps issuing every
    // collective of the sequence with a poisoned payload (NaN header: every rank's alpha / beta / cost turn NaN), and the error becomes
    // everybody's at the next cost evaluation (dist_cost carries the flag; Init, Finalize and Thallo_ProblemCurrentCost all end there).
    bool failed = false;
    bool stopped = false;                                // the failure was agreed on: every rank's plan refuses further steps, its cost reads NaN
    int inject = 0;                                      // tests (ThalloX_DistributedControl what = 2): the n-th rank-local launch / copy from now on reports a failure
};
struct DistPeerInfo;        // what a rank publishes about itself when the device-side exchange is set up (solver_dist.cpp)

class Plan {
public:
    Plan(EnergyPlugin* plugin, const Thallo_InitializationParameters& ip, bool lm, unsigned* dims);
    ~Plan();
    bool ok() const { return ok_; }
    bool ready() const { return ok_ && ready_; }

    void init(void** params);
    int  step(void** params);
    double cost();
    void set_param(const char* name, const void* value);
    void get_param(const char* name, void* value);
    int  alpha_beta_trace(float* out_pairs, int cap);
    void unknowns_changed();       // the caller rewrote unknowns / inputs in place between two LM steps (ThalloX_UnknownsChanged)
    void enable_lm(bool on);       // extension: run the LM branch the reference text describes (dead as shipped, thallo.t:463)
    bool lm() const { return lm_; }
    // ThalloX_PlanSetPreconditioner: THALLOX_PRECOND_JACOBI (the reference's, default) or THALLOX_PRECOND_BLOCK_JACOBI; takes effect at the next Init.  0 = ok
    int  set_preconditioner(int kind);
    // ThalloX_PlanSetCoarseAggregates: the two-level preconditioner's aggregates -- (0, NULL, 0) the default size, (k, NULL, 0) greedy aggregates of at most k cameras, or
    // the caller's array of n = C dense ids; takes effect at the next Init.  0 = ok
    int  set_coarse_aggregates(int cameras_per_aggregate, const int* aggregate_of_camera, long n);
    // ThalloX_PlanCoarseSpace: { aggregates, coarse scalars, coarse scalars of the last set-up with the identity's row, coarse factors since Init that met a non-positive pivot } -> 0, or -1 (the form does not run)
    int  coarse_space(long out[4]);
    int  preconditioner_fallbacks();      // blocks of the last step's factorisation that fell back to the diagonal (-1: the block form does not run)
    const char* schedule_name();          // the plugin's, and the opt-in forms that run (before the first Init: that were asked for)
    // ThalloX_PlanSetLinearSolver: THALLOX_SOLVER_PCG (default), THALLOX_SOLVER_SCHUR_PCG, THALLOX_SOLVER_SCHUR_EXPLICIT_PCG or THALLOX_SOLVER_SCHUR_DENSE; takes effect at the next Init.  0 = ok
    int  set_linear_solver(int kind);
    int  schur_blocks() const { return schur_assembled() ? (int)reduced()->blocks() : -1; }      // stored blocks of the assembled S (-1: the assembled form does not run)
    int  schur_held_points();             // points the last step's elimination held fixed (-1: the Schur form does not run)
    int  schur_dense_nonpositive();       // scalars of the last dense factor whose diagonal of S was not positive (identity rows; -1: the dense form does not run)
    // ThalloX_PlanSetHeldUnknowns: the mask of one Unknown (host bytes in the caller's ids, nonzero = that scalar is a constant of the solve; NULL clears it); takes effect
    // at the next Init.  0 = ok
    int  set_held_unknowns(int input, const unsigned char* held, long n);
    long held_unknowns() const { return ready_ ? held_count_ : -1; }      // held scalars since the last Init (-1: no mask in force)
    // ThalloX_PlanSetPrior: a Gaussian prior 1/2 w (x - mean)^2 per scalar of one Unknown (host floats in the caller's ids; weight 0: none there; weight NULL clears the
    // input's prior); takes effect at the next Init.  0 = ok
    int  set_prior(int input, const float* mean, const float* weight, long n);
    long prior_terms() const { return ready_ ? prior_count_ : -1; }      // scalars with a positive weight since the last Init (-1: there was none)
    int  prior_cost(double* out);                       // the prior's share of the cost at the current unknowns (0 where no prior is in force); nonzero: failed
    // ThalloX_PlanSetRobustLoss: kind THALLOX_LOSS_*, scale in residual units; takes effect at the next Init.  0 = ok
    int  set_robust_loss(int kind, float scale);
    long robust_weights(float* host_out, long n);      // rho'(s) per observation of the last linearisation, the caller's ids -> O, or -1 (no loss in force, n != O)
    // ThalloX_PlanCovariance (solver_forms.cpp): marginal covariance blocks at the current unknowns -> 0, the columns that did not converge, or < 0 (refused)
    long covariance(void** params, int input, const int* ids, long n, float* host_out, const ThalloX_CovarianceOptions* opt, ThalloX_CovarianceInfo* info);
    // collective over the ranks; before Thallo_ProblemInit.  0 on success (every rank returns the same value)
    int  set_distributed(const ThalloX_Distributed& cfg);
    int  set_ghost_exchange(int n_boundary, const int* boundary_units, int n_ghost, const int* ghost_units, const int* ghost_src_rank, const int* ghost_src_pos);
    // collective; before set_distributed: the plan's own RCCL communicator -- then a NULL all-gather / all-reduce callback means "ncclAllGather / ncclAllReduce on the plan's stream"
    int  use_rccl(const unsigned char* id128, int rank, int world);
    const char* distributed_info() const { return dist_ ? dist_->info.c_str() : ""; }
    void rccl_info(int out[3]);     // what the plan's RCCL communicator says about itself: world, device, rank (-1: no communicator / no answer)
    int  dist_control(int what, int value);
    int  dist_kernel_only(int reps);      // bench: `reps` back-to-back one-kernel iterations on this rank's slab, no exchange

    EnergyPlugin* plugin;
    SolverParameters sp;
    Thallo_InitializationParameters ip;
    Thallo_PerformanceSummary summary;
    LaunchCtx ctx;
    KernelTimer ktimer;
    std::vector<float> ab_trace;   // alpha,beta per PCG iteration of the last step
    int last_l_iters = 0;
    unsigned* dims;

private:
    bool ok_ = false;
    bool ready_ = false;           // Init succeeded (parameters bound, plugin prepared)
    bool lm_ = false;
    bool finalized_ = true;
    float prev_cost_ = 0.0f;
    SolverVectors v_;
    std::vector<DeviceBuffer*> bufs_;
    DeviceBuffer* register_buffer();     // a new, empty entry of bufs_ (released with the plan)
    void* device_alloc(size_t bytes);    // ... allocated and zero-filled -> its pointer, or nullptr
    DeviceBuffer parts_;            // reduction partial slots: (2*L+4) x THALLO_HIP_MAX_PARTIALS floats
    int parts_slots_ = 0;
    DeviceBuffer scratch_;          // a few scalar words (cost, trace)
    DeviceBuffer trace_;
    std::vector<int> nb_;           // partial count per slot
    CoarseTimer timer_;
    float* host_words_ = nullptr;      // 16 pinned host words: the step's read-backs (a cost, the LM report) land here -- a copy into pageable memory is staged and synchronous
    int ev_total_ = -1;
    size_t bufs_at_step_ = 0;       // bufs_.size() when the step's "Nonlinear Iteration" started: unchanged = no allocation (and no clear behind one) has been enqueued since
    int cur_ = 0;

    float* slot(int j) { return (float*)parts_.ptr + (size_t)j * THALLO_HIP_MAX_PARTIALS; }
    std::vector<char> fin_;         // slot already reduced to one word (scal(j)) by a 1-wave finish_sum launch
    bool fin_in_kernel_ = true, one_kernel_ = true, batch_delta_ = true, lm_fold_p_ = true, lm_fold_step_ = true, delta_first_touch_ = true, lean_head_ = true;   // A/B switches: read_ab_switches()
    int delta_planes_ = -1;         // THALLO_DELTA_PLANES (-1: unset)
    std::vector<float*> ring_;      // the ring of p planes of the one-kernel GN loop (ring_planes)
    bool ring_possible() const;     // the plugin's iteration takes any p plane, on one GPU or on a row slab of the one-kernel schedule
    int  ring_wanted(int L) const;  // planes a loop of L iterations would like (0: no ring), from THALLO_DELTA_PLANES and L alone
    int  ring_planes(int L);        // how many planes the loop of L iterations runs on (allocates nothing unless lIterations changed since Init)
    void ring_prepare(int L);       // allocates the ring's planes: at Init, and once per change of lIterations; a memory-limited attempt is cached (ring_tried_)
    int  ring_tried_ = 0, ring_L_ = -1;
    // One step's view of the ring: launch k writes p_k into plane k mod n and leaves delta alone; delta takes the pending alpha_j p_j in batches.  Bookkeeping only:
    // the ring says when a flush is due and hands back the batches, its caller launches them and reports a failure its own way (one GPU: set_error, the step ends;
    // a row slab: DLOCAL, the rank stays in step).  `async` (one GPU, THALLO_DELTA_PLANES=N:W): the batches go out on the plan's second stream.
    struct PRing {
        Plan& P;
        const int n;                                    // planes (< 2: no ring)
        const bool async;
        bool delta_zero = false;                        // delta has not been touched since the step began and PCGInit1 left it unset: its first update starts from 0.0f (one GPU, updates on the loop's stream)
        int flushed = 0;                                // p_0 .. p_{flushed-1} are in delta, or on their way there (async)
        int synced = 0;                                 // ... and the loop's stream has waited for the updates of p_0 .. p_{synced-1}
        struct Sent { int upto; hipEvent_t done; };
        std::vector<Sent> sent;                         // async: the updates that went out, in order
        size_t n_ev = 0;
        SolverVectors v;                                // what the plugin is handed: plane k-1 as p[cur], plane k as p[cur ^ 1]
        PRing(Plan& plan, int planes, bool on_second_stream) : P(plan), n(planes), async(on_second_stream), v(plan.v_) {}
        PRing(const PRing&) = delete;
        // whichever way the step is left, the loop's stream ends up behind every update that went out on the second stream: the next step's PCGInit1 zeroes delta
        // (on a failed launch too -- the caller may call Step again)
        ~PRing() { if (!sent.empty()) (void)hipStreamWaitEvent(P.ctx.stream, sent.back().done, 0); }
        bool on() const { return n >= 2; }
        SolverVectors& vectors() { return on() ? v : P.v_; }
        float* plane(int k) const { return k < 0 ? P.v_.p[0] : P.ring_[(size_t)(k % n)]; }
        int  launch(int k, int cur) { v.p[cur] = plane(k - 1); v.p[cur ^ 1] = plane(k); return k == 0 ? 1 : 2; }      // the planes of launch k; its delta mode (none)
        // Before launch k: the last term that has to go into delta now, or -1.  Terms up to k - 2 can go (launch k - 1 leaves their scalars).  Default: plane k mod n
        // still holds p_{k-n}, which has to be in delta before launch k overwrites it -- then everything goes; async: half a ring at a time, as soon as it is there
        int  flush_due(int k) const { const int chunk = (n - 1) / 2 > 0 ? (n - 1) / 2 : 1; return (async ? k - 1 - flushed >= chunk : (k >= n && flushed < k - n + 1)) ? k - 2 : -1; }
        bool next_batch(int upto, thallo_update_terms_t& T);      // the next <= THALLO_HIP_MAX_UPDATE_TERMS terms of p_flushed .. p_upto, oldest first (their scalars are words once what is enqueued has run)
        bool events(hipEvent_t& words, hipEvent_t& done);         // async: the two events of the next update (the plan's list grows on demand)
        int  wait_for(int term);                                  // the loop's stream goes on only when the update that took p_term has run
        int  wait_to_overwrite(int k) { return k >= n && synced < k - n + 1 ? wait_for(k - n) : 0; }      // ... before launch k writes plane k mod n
    };
    int  ring_flush(PRing& R, int upto);                // one GPU: delta += alpha_j p_j for every j <= upto not flushed yet ("PCGDeltaUpdate", on the loop's or the second stream)
    bool ring_takes_one_pass(const PRing& R, int L);    // the step's end is ONE pass over all L terms (nothing flushed, 64 < L <= 128, words behind term 32, loop's own stream)
    bool ring_step_update(PRing& R, int L);             // ... that pass: X += sum_j alpha_j p_j per unknown image, delta neither read nor written ("PCGDeltaUpdate")
    struct Owned { long lo, len; };
    Owned owned_range(size_t u) const;                  // the part of unknown image u this plan updates: its owned rows on a row slab, else all of it
    // PCGLinearUpdate with the ring's pending terms p_flushed .. p_{L-1} riding in it, over the owned range of every unknown image; `launched(rc)` says whether to go on
    template <class Launched> bool ring_linear_update(PRing& R, int L, Launched launched);
    hipStream_t aux_ = nullptr; bool aux_failed_ = false;      // the plan's second stream (background delta updates)
    std::vector<hipEvent_t> aux_events_;
    bool aux_async_ = false;        // THALLO_DELTA_PLANES=N:W: the delta updates of the ring on the second stream, next to the loop
    int aux_workgroups_ = 0;        // share of the chip a background update takes (0: one workgroup per CU -- measured: 64 / 128 too slow, the loop ends up waiting; 320+ put two
                                    // on some CUs, whose marching workgroups then hold everybody's iteration up: 6.4 against 6.0-6.1 ms per GN step)
    bool aux_stream();
    bool fin_deferred_ = true;      // THALLO_FIN_IN_KERNEL unset: the single-reduction GN loop finishes iteration k-1 inside the flat update of iteration k (=1: by the applyJTJ launch's last workgroup; =0: a one-wave launch)
    void read_ab_switches();
    float* scal(int j) { return (float*)parts_.ptr + (size_t)parts_slots_ * THALLO_HIP_MAX_PARTIALS + j; }
    thallo_sum_t partial_sum(int j) { thallo_sum_t s; s.partials = slot(j); s.count = nb_[j]; return s; }
    thallo_sum_t sum(int j) { if (fin_[j]) { thallo_sum_t s; s.partials = scal(j); s.count = 1; return s; } return partial_sum(j); }
    void set_nb(int j, int nb) { nb_[j] = nb; fin_[j] = 0; }
    // Adds the slot's partials once, in the order every consumer would use, so the next kernels read ONE word instead of each of
    // their waves re-adding up to 1024 partials in the prologue (measured: -10 us per PCG iteration at 2048^2)
    // (small launches -- <= 4 partials per lane -- are cheaper to re-add in place than to pay one more launch for)
    void finish(int j) { if (nb_[j] <= 256) return; thallo_hip_finish_sum(partial_sum(j), scal(j), ctx.stream); fin_[j] = 1; }
    void words_done(int k) { const int jD = 2 + 2 * k + 1, jB = jD + 1; fin_[jD] = 1; set_nb(jB, 1); fin_[jB] = 1; }      // iteration k's two words exist: alphaD_k, betaN_k = alphaN_{k+1}
    // alpha_{k-1} and alpha_{k-2} as their numerator / denominator sums, as launch k takes them (k = 0, and k = 1 for the second pair: iteration k's own slots stand in, unread)
    struct PrevAlpha { thallo_sum_t aN, aD, aN2, aD2; };
    PrevAlpha prev_alpha(int k) { const int jN = 2 + 2 * k, jD = jN + 1; return { sum(k ? jN - 2 : jN), sum(k ? jD - 2 : jD), sum(k > 1 ? jN - 4 : jN), sum(k > 1 ? jD - 4 : jD) }; }
    int  ensure_slots(int L);
    int  ensure_iter_buffers();
    int  ensure_sums_buffer();
    int  step_gn_expanded(int ev_iter);
    // ---- the one-kernel GN step: step_gn_one_kernel = set-up, one of three PCG loops (gn_schedule), the shared finish
    enum class GnSchedule { Persist, Deferred, FinishInLaunch };
    struct GnStep {                                     // what the loops of one step share
        const int L;
        const bool batched;                             // no ring: every other delta update is deferred (THALLO_IW_STEP1_MODE(k, 1))
        PRing ring;
        int nb_prev = 0;                                // deferred finish: the partial count of the launch before
        bool lean = false;                              // PCGInit1 left pre, z and p_{-1} out; launch 0 keeps no A p_0 (step_gn_one_kernel)
    };
    SolverVectors& first_launch_vectors(GnStep& st, int k, SolverVectors& v0);
    int  step_gn_one_kernel(int ev_iter);
    GnSchedule gn_schedule(int L, int n_ring);
    int  gn_launch_mode(GnStep& st, int k);             // the ring made ready for launch k; the launch's delta mode (< 0: failed)
    bool gn_finish_last(GnStep& st, int k, int nb);     // deferred finish: the one-wave launch behind the step's last iteration
    bool gn_loop_persist(GnStep& st);
    bool gn_loop_deferred(GnStep& st, int k_end);       // iterations [0, k_end)
    bool gn_loop_finish_in_launch(GnStep& st);
    int  step_gn_resident(int ev_iter);
    bool gn_begin(int ev_iter, int& ev_lin, bool delta_unset = false, bool lean = false);      // the head of every PCG-loop GN step: "Nonlinear Setup", PCGInit1 into slot 2 (delta_unset: it stores no zeros into delta), forms_setup, "Linear Solve" started
    int  gn_finish(int L, int ev_lin);                  // ... its tail: "Nonlinear Finish" started (the caller's update of the unknowns follows) ...
    int  gn_end(int ev_fin, int ev_iter);               // ... and the step counted, its events ended
    bool resident_used_ = false;    // a resident launch ran since the last cost evaluation (its error word is read there)
    bool resident_wait_ran_out(const char* void_what);      // ... read: true = a bounded wait of the resident kernel ran out, the error says that `void_what`
    float compute_cost();
    float* host_words();
    int   step_gn(int ev_iter);
    // solver_forms.cpp: the opt-in forms of a one-GPU PCG plan.  Each is asked for by its setter, decided at Init (forms_prepare, where everything it needs is allocated --
    // never inside a step) and runs until the next Init: want = what was asked for, on = what this solve runs
    int   forms_prepare();                              // Init, behind prepare(): held_prepare, the robust loss, schur_prepare or block_prepare, precond_regions_; nonzero: not ready
    bool  refuse_unless_one_gpu_pcg(bool ok, const char* what_needs);      // "<what_needs> a one-GPU PCG plan" unless ok (the plugin's *_ok()) on a one-GPU PCG plan
    bool  forms_behind_init() const { return held_on() || schur_on_ || block_on_; }
    // behind PCGInit1 (GN: gn_begin; LM: lm_setup), if forms_behind_init(): the mask, the blocks, both factors, the Schur reduction, z = M^-1 r -> the partial count of
    // r . z in rz_out (nb: PCGInit1's, where nothing replaces them) or a negative code, `what` failed.  shift: the LM CtC or NULL; b: the right-hand side
    int   forms_setup(const float* shift, const float* b, float* rz_out, int nb, const char*& what);
    int   step_gn_blocks(int ev_iter);                  // the GN step of the block-Jacobi and the Schur form: the generic loop with thallo_hip_block_step2 as PCGStep2; Schur: on (S, g), then the back-substitution
    int   read_word(const unsigned* dev);               // a status word of the last step, read back (-1: the copy failed)
    std::string schedule_text_;                         // schedule_name()'s text
    // ---- held unknowns (held.hip): the caller's masks by unknown image; since the last Init their count and the mask over the flat vector in the plan's internal ids on
    // the device.  The launches run only when something is held
    std::map<int, std::vector<unsigned char>> held_masks_;
    long held_count_ = -1;
    unsigned char* held_mask_ = nullptr;
    long held_first_ = 0;                               // ... of them in the first unknown image (the Schur form's kept region)
    bool  held_on() const { return held_count_ > 0; }
    // every unknown of the reduced system is held (structure-only bundle adjustment on a Schur plan): the reduced system is empty, its PCG loop takes no iteration (p_0 = 0
    // would make LM's unguarded alpha_0 = 0 / 0) and the back-substitution from delta_c = 0 is the whole solve
    bool  schur_empty() const { return schur_on_ && held_on() && held_first_ == schur_n_; }
    int   held_prepare();
    int   hold_pcg(float* rz_out);                      // pre = z = 0 at the held scalars, the partials of r . z anew -> their number
    // ---- Gaussian priors (prior.hip): the caller's (mean, weight) by unknown image; since the last Init the count of positive weights and the planes w, mu over the flat
    // vector in the plan's internal ids on the device.  The launches run only when a weight is positive.  W reaches A through the shift: GN hands w itself to every
    // ctc / shift argument, LM float32(CtC + w) in a plane of its own (prior_shift_, formed behind PCGFinalizeDiagonal); H stays without W
    struct PriorInput { std::vector<float> mean, weight; };
    std::map<int, PriorInput> prior_inputs_;
    long prior_count_ = -1;
    float *prior_w_ = nullptr, *prior_mu_ = nullptr, *prior_shift_ = nullptr;
    bool  prior_on() const { return prior_count_ > 0; }
    int   prior_prepare();
    const float* gn_shift() const { return prior_on() ? prior_w_ : nullptr; }      // what a GN step (and the covariance) hands to a ctc / shift argument
    const float* lm_shift() const { return prior_on() ? prior_shift_ : v_.CtC; }   // ... and an LM step
    int   prior_cost_partials(float* out, int onto);    // the partials of the prior's cost at the current unknowns: stored (onto = 0 -> their number) or added onto the `onto` partials in out (-> onto)
    int   prior_init(float* rz_out);                    // behind PCGInit1: r, diag, pre, z at the scalars with a prior, the partials of r . z anew -> their number
    int   cost_partials(float* out);                    // the plugin's cost partials with the prior's added onto them -> the slot's count, the plugin's
    int   gn_step1(int k, const PrevAlpha& a, thallo_sum_t bN, float* out);      // PCGStep3 + the apply of a GN iteration: the plugin's pcg_step1, with priors (J^T J + W) p
    // ---- robust loss (energy_ba.hip): handed to the plugin at Init
    int   robust_want_ = 0, robust_on_ = 0;
    float robust_want_scale_ = 0.0f, robust_on_scale_ = 0.0f;
    bool  robust_on() const { return ready_ && robust_on_ != 0; }
    // ---- block-Jacobi preconditioner (block_precond.hip): H, G (the blocks and their factors) and the status word
    bool block_want_ = false, block_on_ = false;
    thallo_block_regions_t block_regions_;              // the plugin's regions
    thallo_block_regions_t precond_regions_;            // ... those the preconditioner runs on (set once per Init): all of them; on a Schur plan the first, the cameras
    float *block_H_ = nullptr, *block_G_ = nullptr;
    unsigned* block_status_ = nullptr;
    int   block_prepare();                              // Init: the regions and the buffers
    // ---- the two-level preconditioner on the assembled S (ba_coarse.hip): M^-1 = G^T G + P Z^T Z P^T.  Asked for by kind 2 of set_preconditioner (block_want_ goes with
    // it), runs on kind 2 of the linear solver alone; the aggregates and every coarse buffer are the reduced system's, built and allocated with the structure of S
    bool coarse_want_ = false;
    int  coarse_k_ = 0;                                 // cameras per aggregate asked for (0: the default)
    std::vector<int> coarse_agg_;                       // ... or the caller's aggregates (empty: greedy)
    // z += the coarse term of M^-1 r behind the launch that left z = G^T G r and nb partials of r . z in `part`: the partials of |Z P^T r|^2 go behind them, so every reader
    // of the slot adds r . z_B + |y|^2 in one fixed order -> the slot's partial count (nb itself where the form does not run), or a negative code
    int   coarse_apply(float* part, int nb, const unsigned* gate);
    // ---- Schur complement on the cameras (ba_schur.hip): PCG on the 9 C camera unknowns, the points eliminated through their blocks.  H, G (the camera blocks: the
    // preconditioner of S) and the status word are the block preconditioner's; the elimination factor, y, the held count and every buffer of the assembled, dense and
    // two-level forms are the plugin's reduced system's (ba_reduced.hpp), which also answers what runs since the last Init; g is the plan's, a solver vector
    bool schur_want_ = false, schur_on_ = false;
    bool schur_explicit_want_ = false;                  // kind 2 asked for: S assembled once per step (ba_schur_explicit.hip), the loop's applies multiply by it
    bool schur_dense_want_ = false;                     // kind 3 asked for: kind 2's structure and assembly, and a dense Cholesky factor of S in place of the reduced PCG loop (ba_schur_dense.hip)
    ReducedCameraSystem* reduced() const { return plugin->reduced_system(); }      // non-NULL wherever schur_on_
    bool  schur_assembled() const { return schur_on_ && reduced()->assembled(); }
    bool  schur_dense() const { return schur_on_ && reduced()->dense_n() >= 0; }
    bool  coarse_on() const { return schur_on_ && reduced()->coarse_n() >= 0; }
    bool  schur_dense_step(const float* g);             // expand, factor, delta_c = S^-1 g, the read-back of the factor's info word; false: the error is set, nothing was applied
    void  schur_dense_pivot_error(int index, const char* where);
    long schur_n_ = 0, schur_hp_off_ = 0, schur_pt_off_ = 0;      // camera unknowns; the point blocks' place in H; the points' place in the flat vector
    float* schur_g_ = nullptr;
    int   schur_prepare();                              // Init: the offsets, the reduced system's configure, g
    // ---- Levenberg-Marquardt: step_lm = lm_setup, one of five PCG loops (lm_schedule), lm_finish
    enum class LmSchedule { Reference, OneKernel, OneKernelSlab, Resident, Blocks };
    // Between the LM state reset and the end of the PCG loop the plugin's launches are gated on the state's gate word (the zeta test on the device); whichever way
    // the loop is left, the gate is off again before the next launch that has to run
    struct GateOff {
        LaunchCtx& c;
        GateOff(LaunchCtx& ctx, const unsigned* gate) : c(ctx) { thallo_hip_lm_set_gate(gate); c.gate = gate; }
        void off() { thallo_hip_lm_set_gate(nullptr); c.gate = nullptr; }
        ~GateOff() { off(); }
    };
    // What every part of one LM step needs, computed once (lm_setup), and what the loop hands to lm_finish.
    // Slots: 0 cost, QS q, B.. as in GN (alphaN_k = B+2k, alphaD_k = B+2k+1, betaN_k = B+2k+2); T0, T1: scratch dots (the model cost's two sums).
    struct LmStep {
        Plan& P;
        hipStream_t s;
        int L, T0, T1, period;
        static constexpr int B = 2, QS = 1;
        bool slab;                                      // one row slab of a multi-GPU run (flat form)
        long o, n, oe, ne;                              // the owned rows' sub-vector [o, o + n); with the ghost rows [oe, oe + ne)
        bool pc, fold_ctc, fold_init;
        float* lmst;                                    // 8 words: Q0, gate, iterations done, | dJJd, db, new cost
        const unsigned* gate;
        int ev_iter, ev_lin = -1;
        int k_done = 0;
        bool model_cost_done = false;                   // the two sums of the model cost are already in slots T0 / T1, the unknowns saved and updated
        bool failed = false;                            // one GPU: a launch failed, the step ends
        bool coll_failed = false;                       // a collective itself failed: nothing left to stay in step with
        LmStep(Plan& plan, int ev_iter);
        bool skip() const { return failed || (slab && P.dist_->failed); }
        void check(int rc, const char* what);
        int  global(int j) { return slab ? P.dist_sum_slot(j) : 0; }                              // nonzero: the collective itself failed
        int  global_rows(int j, float* vec) { return slab ? P.dist_sum_and_rows(j, vec) : 0; }
    };
    int   step_lm(int ev_iter);
    bool  lm_setup(LmStep& st);
    LmSchedule lm_schedule(const LmStep& st);
    void  lm_loop_reference(LmStep& st);
    void  lm_loop_blocks(LmStep& st);                   // solver_forms.cpp: the reference-shaped loop of the block-Jacobi and the Schur form; Schur: on (S + CtC_c, g), then the back-substitution
    void  lm_loop_one_kernel(LmStep& st);
    void  lm_loop_one_kernel_slab(LmStep& st);
    void  lm_loop_resident(LmStep& st);
    int   lm_finish(LmStep& st);
    bool  lm_agree_all();
    int   lm_accept_or_revert(float dJJd, float db, float newCost, int k_done, int ev_fin, int ev_iter);      // the end of an LM step: accept / revert, trust region (shared by step_lm and the shard form)
    int   step_lm_shard(int ev_iter);                   // solver_dist.cpp: LM on residual shards (bundle adjustment's camera shards)
    // ... and what the two drivers share
    void  lm_trust_region_at_start() { if (sp.nIter == 0) { radius_ = sp.trust_region_radius; decrease_factor_ = sp.radius_decrease_factor; } }   // gauss_newton.t:1185-1186 (copied at init)
    hipError_t copy_unknowns(bool restore);             // savePreviousUnknowns (unknowns -> prevX) / revertUpdate (prevX -> unknowns)
    static int lm_iterations_done(const float* rep, int enqueued);      // the step's report: the iteration the zeta test froze the loop at, if it did
    int   ensure_lm_vectors();
    float read_sum(int j);
    float radius_ = 1e4f, decrease_factor_ = 2.0f;
    void finalize();
    void linear_update_tail(int L, bool batched);
    // solver_dist.cpp
    DistState* dist_ = nullptr;
    RcclComm* rccl_ = nullptr;
    struct GhostSpec { bool given = false; std::vector<int> boundary, ghost, src_rank, src_pos; } ghost_spec_;
    // set-up: set_distributed_impl = dist_pick_form, dist_world_ok, one dist_setup_* (the shared steps below, each in the form's own place), dist_render_info
    int  set_distributed_impl(const ThalloX_Distributed& cfg);
    int  dist_pick_form(DistForm& form);
    int  dist_world_ok(const ThalloX_Distributed& cfg, bool needs_allreduce);
    int  dist_setup_shard(const ThalloX_Distributed& cfg), dist_setup_range(const ThalloX_Distributed& cfg, bool part), dist_setup_flat(const ThalloX_Distributed& cfg), dist_setup_slab(const ThalloX_Distributed& cfg);
    DistState* dist_new_state(const ThalloX_Distributed& cfg, DistForm form);
    DistState* dist_new_row_state(const ThalloX_Distributed& cfg, DistForm form);      // Slab and Flat: the rows checked and handed to the plugin first
    int  dist_alloc_messages(size_t words);             // rank-local: there is nothing to agree through without them
    int  dist_agree_or_fail(bool mine, const char* mine_no, const char* others_no);     // ONE collective: 0, or every rank returns -1 (the rank that said no with mine_no)
    bool dist_p2p_requested() const;                    // cfg.device_exchange, unless THALLO_DIST_P2P=0
    bool dist_alloc_ctl();
    int  dist_agree_p2p(bool mine);                     // ONE collective: want_p2p = every rank wants (and can have) the device-side exchange
    bool dist_partition_lists_ok(const ThalloX_Distributed& cfg, long U);
    void dist_partition_upload(const int* counts, const thallo_units_t& planes, long per_unit, bool& lists_ok, bool& mem_ok);
    void dist_render_info();
    // device-side exchange: the mailboxes (ONE all-gather of one DistPeerInfo, then ONE agreement); the Slab form adds its neighbours' blocks in between
    int  dist_exchange_mail(long bytes, bool same_bytes, DistPeerInfo& mine, DistPeerInfo* infos, bool& ok);
    int  dist_agree_mapped(bool ok);
    int  dist_map_peers();                              // Slab: mailbox + the resident kernel's ghost area; the neighbours' blocks
    int  dist_map_mail(long bytes);                     // Flat, Partition, Shard: only the mailbox is shared between ranks
    // its self-check at the first Init: dist_self_check = one of four checks, each inside the frame dist_check_begin / _read_error / _finish
    int  dist_self_check(), dist_check_units(), dist_check_allreduce(), dist_check_rows(), dist_check_slab();
    void dist_check_begin(), dist_check_read_error();
    int  dist_check_finish(bool pass, float* scratch, size_t scratch_floats, bool xrows);
    template <class Fill, class Exchange, class Verify> int dist_check_pattern(float* vec, size_t n, bool with_sum, bool xrows, Fill fill, Exchange exchange, Verify verify);
    // the exchanges
    int  dist_allgather(const void* send, void* recv, long bytes);
    int  dist_agree(bool flag, bool& all);
    void dist_fail(const char* fmt, ...);               // first rank-local failure: report it, switch this rank to "collectives only" (DistState::failed)
    bool dist_skip() const { return dist_ && dist_->failed; }
    void dist_exchange_rc(int rc, const char* what);    // the result of a device-side exchange's launch: an injection point; "<what> failed (rc)" on a healthy rank
    // what a rank hands an iteration's device-side exchange: its own sums and slots or, once it has failed, dummies that only have to be launchable (it sends NaN)
    struct DistPayload { thallo_sum_t sum; const float* slot; int nb, poison; };
    DistPayload dist_payload(thallo_sum_t sum, const float* slot, int nb) { const float* dummy = (const float*)dist_->send.ptr; return dist_->failed ? DistPayload{ { dummy, 1 }, dummy, 1, 1 } : DistPayload{ sum, slot, nb, 0 }; }
    int  dist_xrows_lm(float* vec, int jN, int jD, int jB, int nb, float* lm_state, int k);      // the ONE exchange of a slab's one-launch LM iteration
    int  dist_two_sums_and_rows(int j1, int j2, float* vec, float* zeta_state = nullptr, int zeta_k = 0, bool* zeta_done = nullptr);
    int  dist_xrows(float* vec, bool rows, int mode, thallo_sum_t s, const float* aD_part, const double* s3, int nb, float* out0, float* out1, float* zeta_state = nullptr, int zeta_k = 0);
    int  dist_sum_slot(int j);                          // slot j (local partials) -> scal(j) = rank-ordered global sum
    int  dist_sum_and_rows(int j, float* vec);          // ... and the ghost rows of a flat vector from the neighbours' boundary rows (j < 0: rows only)
    int  dist_exchange_unknown_rows();
    int  dist_replicate(float* vec, int sum_slot);      // Range: every rank's owned pieces of `vec` to every rank (and, sum_slot >= 0, that slot's global sum)
    int  dist_ghosts(float* vec, int sum_slot);         // Partition: `vec` at my boundary units to the ranks that hold them as ghosts (and the sum)
    int  dist_allreduce(float* buf, long count);        // Shard: the shared block's partial sums added over the ranks, in place
    // the Gauss-Newton step, per form
    int  step_gn_slab(int ev_iter);
    int  dist_pcg_init();                               // every form's head: cur_ = 0, PCGInit1 into slot 2 -> its partial count (the caller decides whether it is the slot's)
    int  dist_three_launch_iter(int k, long o, long n); // Flat, Range, Partition, Shard: PCGUpdate over [o, o + n), applyJTJ with its sums into alphaD_k's slot -> its partial count
    // Slab: dist_gn = dist_gn_begin, ONE of the four PCG loops, the shared finish (linear update over the owned rows, ghost refresh); no bookkeeping
    int  dist_gn(int L, bool p2p);
    int  dist_gn_begin(bool p2p);
    int  dist_agree_defer();                            // ONE collective: D.defer_state = every rank can run the marching kernel's deferred cross-rank finish
    void dist_ring_flush(PRing& R, int upto);
    int  dist_launch_mode(PRing& R, int k, bool batch);
    void dist_gn_loop_resident(int L);
    void dist_gn_loop_deferred(int L, PRing& R, bool batch);
    void dist_gn_loop_p2p(int L, PRing& R, bool batch);
    int  dist_gn_loop_allgather(int L, PRing& R, bool batch);
    int  dist_allgather_iter(float* Ap, int k, int nb);      // Slab, Flat: the all-gather exchange of iteration k: [alphaD | N, S1, S2 | boundary rows of the new A p]
    // Flat: PCGInit + ONE exchange per PCG iteration behind pcg_iter (one launch) or pcg_update + apply_jtj_sums (three launches) + linear update + ghost refresh
    int  dist_gn_flat(int L);
    int  dist_gn_flat_loop_one_launch(int L), dist_gn_flat_loop_three_launch(int L);
    int  dist_flat_exchange_iter(float* Ap, int k, int nb);
    // Range, Partition: dist_gn_range = its begin (clears, PCGInit1, alphaN_0 and r everywhere), L x (dist_three_launch_iter on the full vector, ONE exchange), linear update of all unknowns
    int  dist_gn_range(int L), dist_gn_range_begin(), dist_range_exchange_iter(int k, int nb);
    // Shard: dist_gn_shard = its begin (through alphaN_0), L x (dist_three_launch_iter, all-reduce of the point block of A p + block sums + the camera sums), linear update
    int  dist_gn_shard(int L), dist_gn_shard_begin(), dist_shard_exchange_iter(int k, int cam_slots);
    struct TwoBlocks { int cam = 0, pt = 0; };          // partial counts of one element-wise launch on the camera block and on the point block
    template <class Launch> TwoBlocks dist_on_blocks(float* cam_partials, float* pt_partials, const char* what, Launch launch);      // launch(offset, n, partials); "<what> launch failed (cam, pt)"
    struct ShardSum { int j; float* pts; int nbp; float* out; };      // camera partials in slot j (rank-ordered over the ranks) + the point block's -> out (nullptr: scal(j), the slot's final word)
    int  dist_shard_sums(std::initializer_list<ShardSum> sums, const char* what_cam, const char* what_sum);      // ONE all-gather of one float per sum
    // Shard, LM: step_lm_shard = lm_shard_setup, lm_shard_loop (its residual-reset branch: lm_shard_residual_reset), lm_shard_finish
    struct ShardLm;
    bool lm_shard_setup(ShardLm& st), lm_shard_loop(ShardLm& st), lm_shard_residual_reset(ShardLm& st, int k, TwoBlocks& nb);
    int  lm_shard_apply(float* x, float* Ax, int T0, const char* what), lm_shard_finish(ShardLm& st);
    float dist_cost();
    void dist_release();
};

template <class Launched> bool Plan::ring_linear_update(PRing& R, int L, Launched launched)
{
    thallo_update_terms_t T; T.count = 0;
    for (int j = R.flushed; j < L; ++j) { T.p[T.count] = R.plane(j); T.alphaN[T.count] = sum(2 + 2 * j); T.alphaD[T.count] = sum(2 + 2 * j + 1); ++T.count; }
    long off = 0;
    for (size_t u = 0; u < plugin->unknown_images().size(); ++u) {
        TimedLaunch t(ctx, "PCGLinearUpdate");
        const Owned o = owned_range(u);
        thallo_update_terms_t Tu = T;
        for (int j = 0; j < Tu.count; ++j) Tu.p[j] += off + o.lo;
        // (R.delta_zero: no update has run in this step -- every image's part of delta is read for the first time here, as zeros; X is given, so delta stays unwritten)
        if (!launched((R.delta_zero ? thallo_hip_linear_update_n_from_zero : thallo_hip_linear_update_n)(plugin->unknown_ptr((int)u) + o.lo, v_.delta + off + o.lo, Tu, o.len, 0, ctx.stream))) return false;
        off += plugin->unknown_images()[u].n_floats;
    }
    return true;
}

}  // namespace thallo
