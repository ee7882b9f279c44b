/*
 * Thallo.h -- public C API of the MI355X-native Thallo solver backend (libThallo.so).
 *
 * ABI-compatible with the reference's API/release/include/Thallo.h:1-105: same 3 opaque
 * handle types, same 6-int initialization struct passed BY VALUE, same 13 entry points and
 * the same performance-summary structs, so an application written against the reference
 * (examples/shared/ThalloSolver.h:43-106, every tests/<x>/main.cpp) relinks unchanged.
 * Callers in C++ wrap the include in extern "C" exactly as they do for the reference; this
 * header also does it itself.
 *
 * Behavioural notes (where this backend differs from the reference are marked DIFF):
 *  - problem specifications: the bundled energies are recognised from the .t file and run on
 *    precompiled gfx950 plugins; an unrecognised .t makes Thallo_ProblemPlan print a
 *    diagnostic and return NULL (the reference prints a Lua traceback and returns NULL,
 *    API/src/thallo.t:1431-1432).
 *  - DIFF: cpuOnly=1 is rejected (NULL state); this build has no CPU fallback on purpose.
 *  - doublePrecision=1 (API/src/precision.t:3-6: thallo_float = double): every problem file goes through the
 *    front-end, whose kernels are generated with thallo_float = double, and the reference-shaped double loop drives
 *    them (Gauss-Newton, and with ThalloX_EnableLM the LM branch; one GPU).  Unknowns / thallo_float arrays are
 *    doubles, arrays and Params declared `float` stay floats, solver parameters stay floats (gauss_newton.t:200-216).
 *    DIFF: the ThalloX_ multi-GPU extensions are not available in this mode.
 *  - DIFF: GPU errors are reported on stderr and surface as NULL / 0 returns; the process is
 *    never exit()ed (reference: API/src/cuda_util.t:103-118).
 */
#ifndef THALLO_H
#define THALLO_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct Thallo_State   Thallo_State;
typedef struct Thallo_Plan    Thallo_Plan;
typedef struct Thallo_Problem Thallo_Problem;

/* Set once per Thallo_NewState; an all-zero struct is the fast default. */
struct Thallo_InitializationParameters {
    int doublePrecision;   /* 1: thallo_float = double (generated kernels, see above) */
    int verbosityLevel;    /* 0 quiet, >=1 prints solver log + timing table at the end of a solve */
    int timingLevel;       /* 0 no timing recorded (no events in the stream: Thallo_GetPerformanceSummary reports zeros), 1 coarse events (eight per solver step -- each one
                              a barrier packet between two launches: ~30 us per step, which small problems notice), 2 per-kernel hipEvents, 3 additionally device-syncs around them */
    int threadsPerBlock;   /* accepted for compatibility; kernels carry their own tuned shapes */
    int useAutoscheduler;  /* bundled energies: their hand-written plugin (a fixed schedule) either way.  Generated plugins (a .t file no plugin recognises, or
                              THALLO_FRONTEND=generate): 1 = the autoscheduler's lowering where it applies -- residuals that live on their unknowns' grid become
                              unknown-wise gather kernels, one merged kernel per (domain, schedule) group, no atomics (API/src/thallo.t:5173-5190,5273-5306);
                              0 = the reference's default residual-wise scatter (thallo.t:4096-4098).  Every example passes 1 (examples/.../main.cpp:37). */
    int cpuOnly;           /* must be 0: Thallo_NewState returns NULL for 1.  The product has no CPU path by design (the reference's needs Terra, API/src/cpu_cuda.t);
                              the CPU restatement under oracle/ is test infrastructure and is never linked or loaded by this library. */
};
typedef struct Thallo_InitializationParameters Thallo_InitializationParameters;

Thallo_State* Thallo_NewState(Thallo_InitializationParameters params);

/* solverkind: "gauss_newton" or "levenberg_marquardt" (anything else: NULL). */
Thallo_Problem* Thallo_ProblemDefine(Thallo_State* state, const char* filename, const char* solverkind);
void            Thallo_ProblemDelete(Thallo_State* state, Thallo_Problem* problem);

/* dimensions[i] is the extent of the i-th Dims() name of the .t; the pointer is retained. */
Thallo_Plan* Thallo_ProblemPlan(Thallo_State* state, Thallo_Problem* problem, unsigned int* dimensions);
void         Thallo_PlanFree(Thallo_State* state, Thallo_Plan* plan);

/* Solver parameters by name; *value has the parameter's own type: int for nIterations,
 * lIterations, residual_reset_period; float for the rest (API/src/gauss_newton.t:200-216). */
void Thallo_SetSolverParameter(Thallo_State* state, Thallo_Plan* plan, const char* name, void* value);
void Thallo_GetSolverParameter(Thallo_State* state, Thallo_Plan* plan, const char* name, void* value);

/* problemparams[i] belongs to input index i of the .t: device pointers for Unknown/Array/Sparse,
 * host pointers to the scalar for Param.  Unknown buffers are updated in place. */
void   Thallo_ProblemSolve(Thallo_State* state, Thallo_Plan* plan, void** problemparams);
void   Thallo_ProblemInit(Thallo_State* state, Thallo_Plan* plan, void** problemparams);
int    Thallo_ProblemStep(Thallo_State* state, Thallo_Plan* plan, void** problemparams);   /* 0 = finished */
double Thallo_ProblemCurrentCost(Thallo_State* state, Thallo_Plan* plan);

struct Thallo_PerformanceEntry {
    unsigned int count;
    double minMS;
    double maxMS;
    double meanMS;
    double stddevMS;
};
typedef struct Thallo_PerformanceEntry Thallo_PerformanceEntry;

struct Thallo_PerformanceSummary {
    Thallo_PerformanceEntry total;
    Thallo_PerformanceEntry nonlinearIteration;
    Thallo_PerformanceEntry nonlinearSetup;
    Thallo_PerformanceEntry linearSolve;
    Thallo_PerformanceEntry nonlinearResolve;
};
typedef struct Thallo_PerformanceSummary Thallo_PerformanceSummary;

void Thallo_GetPerformanceSummary(Thallo_State* state, Thallo_Plan* plan, Thallo_PerformanceSummary* summary);

/* ------------------------------------------------------------------------------------------
 * Extensions (not in the reference; prefixed ThalloX_).  Used by bench.py and the tests.
 * ------------------------------------------------------------------------------------------ */

/* Launch on `stream` (a hipStream_t) instead of the legacy default stream. */
void ThalloX_SetStream(Thallo_Plan* plan, void* stream);

/* Bracket every `period`-th launch of each kernel with hipEvents (0 = off).  Cheap enough to
 * leave on inside a timed region; results via ThalloX_GetKernelStat. */
void ThalloX_SetKernelSampling(Thallo_Plan* plan, int period);
/* Enumerate sampled kernels: returns 0 while index is valid. launches = all launches,
 * samples = timed launches, total_ms = sum over timed launches.  Synchronises the device. */
int  ThalloX_GetKernelStat(Thallo_Plan* plan, int index, const char** name, long* launches, long* samples, double* total_ms);
void ThalloX_ResetKernelStats(Thallo_Plan* plan);
/* ... of the same entry: how many of the sampled launches carried their own start / stop events (the kernel's begin-to-end time, without the dispatch gap that
   events recorded around a launch include) and their total; 0 samples where the kernel's shim does not offer it */
int ThalloX_GetKernelStatOwn(Thallo_Plan* plan, int index, long* samples, double* total_ms);

/* alpha/beta of every PCG iteration of the most recent Step (tests): writes up to cap pairs,
 * returns the number of PCG iterations run. */
int  ThalloX_GetAlphaBetaTrace(Thallo_Plan* plan, float* out_pairs, int cap);

/* Run the Levenberg-Marquardt branch as the reference's text describes it (gauss_newton.t, every UsesLambda()
 * branch).  Off by default even for "levenberg_marquardt": the reference as shipped executes plain GN for that
 * kind (thallo.t:463 matches "LM", which no accepted kind string contains).  Call before Thallo_ProblemInit. */
void ThalloX_EnableLM(Thallo_Plan* plan, int enable);
/* Between two LM steps the branch lives on state of the previous step's end, like the reference (pd.hd.prevCost, gauss_newton.t:1710,1732) -- here also what a
 * plugin derived from the unknowns at that point (shape_from_shading's precomputed planes).  A caller that rewrites the unknowns or the input images IN PLACE
 * between two LM steps (same pointers: parameter binding cannot see it) says so with this call: derived state is dropped and the carried cost re-evaluated.
 * Gauss-Newton steps derive everything from the unknowns as they are at the call and never need it. */
void ThalloX_UnknownsChanged(Thallo_State* state, Thallo_Plan* plan);

/* Name of the plugin a plan runs ("image_warping", "laplacian_image", ...). */
const char* ThalloX_PlanEnergyName(Thallo_Plan* plan);

/* The J^T J p schedule the plan's plugin runs: "matrix-free" (hand-written plugins), or for generated plugins "per residual" (each residual's own
 * schedule lines), "dense [JtJ]p", "sparse [[Jt][J]]p", "dense direct solve". */
const char* ThalloX_PlanScheduleName(Thallo_Plan* plan);

/* The PCG preconditioner.  THALLOX_PRECOND_JACOBI: the reference's point Jacobi (guardedInvert(diag J^T J); in the LM branch 1 / (CtC + diag)) -- the default, and what a
 * plan that never makes this call runs, launch for launch.  THALLOX_PRECOND_BLOCK_JACOBI: one dense block of J^T J (+ the LM diagonal) per group of unknowns that belongs
 * together, factored once per step -- bundle_adjustment: 9 x 9 per camera, 3 x 3 per point; Gauss-Newton and ThalloX_EnableLM; one GPU; the plan then runs its unfused PCG
 * loop (ThalloX_PlanScheduleName says so).  Between Thallo_ProblemPlan and Thallo_ProblemInit, or before a re-Init: it takes effect at the next Init.  Returns 0, or nonzero
 * with ThalloX_LastError naming the energy and the reason: an energy without blocks (every other energy, generated ones included), a doublePrecision = 1 state, a distributed
 * plan (ThalloX_PlanSetDistributed after this call is refused likewise), a direct-solve plan. */
#define THALLOX_PRECOND_JACOBI       0   /* the reference's; default */
#define THALLOX_PRECOND_BLOCK_JACOBI 1
/* THALLOX_PRECOND_TWO_LEVEL: on the ASSEMBLED reduced camera matrix (THALLOX_SOLVER_SCHUR_EXPLICIT_PCG below), the camera blocks plus a coarse correction that couples
 * neighbouring cameras, M^-1 = G^T G + P S_c^-1 P^T: the cameras are aggregated by co-visibility, the coarse space is piecewise constant per camera parameter (9 K scalars
 * for K aggregates, empty at held scalars), S_c = P^T S P is assembled, Jacobi-scaled and factored densely in float32 every step (in LM with the step's diagonal), and
 * every M^-1 r of the reduced PCG loop -- ThalloX_PlanCovariance's column PCG too -- adds P Z^T Z P^T r, Z = L^-1 D.  It removes most of the growth of the iteration count
 * with the length of the camera chain, which the camera blocks cannot bridge: it is for covariances and for tight reduced solves (a small q_tolerance, GN with many
 * lIterations); at q_tolerance = 0.1 an LM step's reduced solve takes 2 - 3 iterations either way and the set-up is pure cost.  What it does not fix: the converged float32
 * column still differs from a float64 solve by the float32 S's own error.  Accepted and refused exactly where THALLOX_PRECOND_BLOCK_JACOBI is; takes effect at the next
 * Init, WHICH FAILS (ThalloX_PlanReady 0, ThalloX_LastError naming both settings) unless the plan's linear solver is THALLOX_SOLVER_SCHUR_EXPLICIT_PCG -- in whichever
 * order the two setters were called; THALLOX_SOLVER_SCHUR_DENSE ignores the preconditioner as before.  ThalloX_PlanScheduleName then ends "...; two-level on S (K
 * aggregates, n_c = N)".  A coarse factor that meets a pivot that is not positive fails nothing: Z = 0 for that step (block Jacobi alone) and ThalloX_PlanCoarseSpace
 * counts it.  The coarse matrices' bytes are added to the structure's count before anything is allocated.  A plan that never asks for it launches what it launched before. */
#define THALLOX_PRECOND_TWO_LEVEL    2
int ThalloX_PlanSetPreconditioner(Thallo_Plan* plan, int kind);
/* The aggregates of THALLOX_PRECOND_TWO_LEVEL, between Thallo_ProblemPlan and Thallo_ProblemInit (or before a re-Init).  (0, NULL, 0): the default, greedy aggregates of at
 * most k = max(8, ceil(C / 128)) cameras; (k >= 1, NULL, 0): greedy aggregates of at most k cameras -- built on the host at Init from the structure of S: cameras in
 * ascending id, an unassigned camera seeds an aggregate, which repeatedly takes the unassigned camera with the largest summed number of co-visible points to its members
 * (ties: the lower id) until it has k members or no connected camera is left; deterministic; held cameras are assigned like any other (their rows of P are zero).  Or
 * aggregate_of_camera: n = C ids in the caller's camera ids, dense 0 .. K - 1 with every id used.  Returns 0, or nonzero with ThalloX_LastError naming the reason. */
int ThalloX_PlanSetCoarseAggregates(Thallo_Plan* plan, int cameras_per_aggregate, const int* aggregate_of_camera, long n);
/* out = { the aggregates K, the coarse scalars n_c = 9 K, the coarse scalars of the last set-up that were given the identity's row (every member held there, or nothing
 * observed), the coarse factors since Thallo_ProblemInit that met a pivot that is not positive }; returns 0, or -1 when the two-level form does not run.  Synchronises the
 * plan's stream. */
int ThalloX_PlanCoarseSpace(Thallo_Plan* plan, long out[4]);
/* Blocks of the last step's factorisation that were not positive definite in float32 and fell back to their point-Jacobi diagonal (they behave as under
 * THALLOX_PRECOND_JACOBI); -1 when the block form does not run.  Synchronises the plan's stream. */
int ThalloX_PlanPreconditionerFallbacks(Thallo_Plan* plan);

/* The linear solver of a step.  THALLOX_SOLVER_PCG: PCG on the full system J^T J delta = -J^T F (+ the LM diagonal) -- the default, and what a plan that never makes this call
 * runs, launch for launch.  THALLOX_SOLVER_SCHUR_PCG: bundle_adjustment's points are eliminated exactly through their 3 x 3 blocks and PCG runs on the Schur complement over
 * the 9 C camera unknowns, preconditioned by the 9 x 9 camera blocks -- whatever ThalloX_PlanSetPreconditioner was given; the points follow by back-substitution
 * (Gauss-Newton and ThalloX_EnableLM; one GPU; ThalloX_PlanScheduleName says "Schur complement on the cameras; block-Jacobi on S").  Between Thallo_ProblemPlan and
 * Thallo_ProblemInit, or before a re-Init: it takes effect at the next Init.  Returns 0, or nonzero with ThalloX_LastError naming the energy and the reason: every energy but
 * bundle_adjustment (generated ones included), a doublePrecision = 1 state, a distributed plan (ThalloX_PlanSetDistributed after this call is refused likewise), a
 * direct-solve plan.  THALLOX_SOLVER_SCHUR_EXPLICIT_PCG: the same solve -- elimination, right-hand side, preconditioner, PCG chain, back-substitution -- with the reduced
 * camera matrix S ASSEMBLED once per step as a block-sparse matrix over the co-visible camera pairs (9 x 9 blocks, both triangles), so that every S x of the loop is one
 * block-sparse mat-vec instead of three passes over the observations (ThalloX_PlanScheduleName: "Schur complement on the cameras, assembled (N blocks); block-Jacobi on
 * S").  Its structure (blocks, term lists, one 9 x 3 block per observation) is built at Init and must fit a quarter of the free device memory and int32 indices: otherwise Init
 * fails with ThalloX_LastError naming the bytes wanted and allowed -- the term count grows with the square of a point's track length; there is no silent fall-back to
 * THALLOX_SOLVER_SCHUR_PCG.  Refused where THALLOX_SOLVER_SCHUR_PCG is.
 * THALLOX_SOLVER_SCHUR_DENSE: the exact solve for small and medium problems (up to a few hundred cameras).  Elimination, right-hand side and assembly are
 * THALLOX_SOLVER_SCHUR_EXPLICIT_PCG's (its structure and budget are implied); then S is expanded to a dense lower triangle, Jacobi-scaled to a unit diagonal, factored by a
 * float32 Cholesky on the device and delta_c = S^-1 g follows by two triangular sweeps -- no PCG loop on S: lIterations, q_tolerance and ThalloX_PlanSetPreconditioner are
 * ignored, the step reports 0 linear iterations.  In LM every step factors anew (S carries the step's diagonal).  ThalloX_PlanScheduleName: "... assembled (N blocks);
 * dense Cholesky of S (n = 9 C)".  A scalar the caller holds, and a scalar whose diagonal of S is not positive (a camera nothing observes; counted by
 * ThalloX_PlanSchurDenseNonPositive), gets the identity's row and column: delta is exactly 0 there.  A FACTOR THAT MEETS A PIVOT THAT IS NOT POSITIVE FAILS THE STEP:
 * Thallo_ProblemStep returns 0, the unknowns are unchanged, and ThalloX_LastError names the camera and scalar of the pivot.  Gauss-Newton without a fixed gauge is such a
 * system (singular but consistent: PCG tolerates it, a factorisation does not): hold a camera and one more scalar (ThalloX_PlanSetHeldUnknowns) or use ThalloX_EnableLM.
 * One blocking 4-byte read-back per step reports it.  The dense matrix takes 4 ld n bytes (n = 9 C, ld = n rounded up to 32), added to the structure's bytes before
 * anything is allocated: Init fails, naming the bytes wanted and allowed, above a quarter of the free device memory.  Refused where THALLOX_SOLVER_SCHUR_PCG is. */
#define THALLOX_SOLVER_PCG                0   /* default */
#define THALLOX_SOLVER_SCHUR_PCG          1
#define THALLOX_SOLVER_SCHUR_EXPLICIT_PCG 2
#define THALLOX_SOLVER_SCHUR_DENSE        3
int ThalloX_PlanSetLinearSolver(Thallo_Plan* plan, int kind);
/* The stored 9 x 9 blocks of the assembled S (both triangles) after Thallo_ProblemInit; -1 when the assembled form does not run. */
int ThalloX_PlanSchurBlocks(Thallo_Plan* plan);
/* Points that the last step's elimination held fixed (delta = 0 for the step: their 3 x 3 block did not factor, or has a squared pivot of the Jacobi-scaled block below 2^-16);
 * -1 when the Schur form does not run.  ThalloX_PlanPreconditionerFallbacks then reports the camera blocks' fallbacks.  Synchronises the plan's stream. */
int ThalloX_PlanSchurHeldPoints(Thallo_Plan* plan);
/* Scalars of the last dense factor (a step's, or a ThalloX_PlanCovariance call's) whose diagonal of S was not positive and that were given the identity's row and column;
 * -1 when THALLOX_SOLVER_SCHUR_DENSE does not run.  Synchronises the plan's stream. */
int ThalloX_PlanSchurDenseNonPositive(Thallo_Plan* plan);

/* Unknowns that are not to move: gauge fixing (one or two cameras), fixed intrinsics (components 6..8 of every camera), motion-only or structure-only bundle adjustment,
 * known control points.  `input` is the Inputs{} index of an Unknown (bundle_adjustment: 0 cameras, 1 points); held is a HOST array of n = elements x components bytes in
 * the caller's ids, held[element * components + k] != 0 meaning that this scalar is a constant of the solve; held == NULL clears that input's mask.  Every step is then the
 * GN / LM step of the problem in the free unknowns, delta at a held scalar is exactly 0.0f and the unknown keeps its bits through Thallo_ProblemStep / Solve (an LM revert
 * included); cost, model cost, the zeta test, accept / revert and the trust region run unchanged.  Works with every preconditioner and linear solver above; no launch is
 * added to a PCG iteration.  A plan that never makes the call, clears its masks or holds nothing launches what it launches otherwise, bit for bit.  Between
 * Thallo_ProblemPlan and Thallo_ProblemInit, or before a re-Init: it takes effect at the next Init, which fails (ThalloX_PlanReady 0) when the masks hold every unknown.
 * Returns 0, or nonzero with ThalloX_LastError naming the energy and the reason: every energy but bundle_adjustment (generated ones included), a doublePrecision = 1 state,
 * a distributed plan (ThalloX_PlanSetDistributed after this call is refused likewise), a direct-solve plan, an input that is not an Unknown, an n that is not
 * elements x components. */
int ThalloX_PlanSetHeldUnknowns(Thallo_Plan* plan, int input, const unsigned char* held, long n);
/* Scalars held since the last Thallo_ProblemInit (ThalloX_PlanScheduleName then ends in "; N unknowns held"); -1 when no mask is in force.  ThalloX_PlanSchurHeldPoints keeps
 * its meaning: the points the elimination's factor rule held. */
long ThalloX_PlanHeldUnknowns(Thallo_Plan* plan);

/* Gaussian priors on single unknowns, the soft form of ThalloX_PlanSetHeldUnknowns: calibrated intrinsics with a tolerance, GPS / IMU pose priors, surveyed control
 * points, a soft gauge.  `input` is the Inputs{} index of an Unknown (bundle_adjustment: 0 cameras, 1 points); mean and weight are HOST arrays of n = elements x components
 * floats in the caller's ids; weight is the precision 1 / sigma^2 in residual^2 per unknown^2, 0 = no prior on that scalar; weight == NULL clears that input's prior.
 * The solve is that of the energy with one more residual sqrt(w) (x - mean) per scalar with w > 0: the cost gains 1/2 w (x - mean)^2 (Thallo_ProblemCurrentCost, accept /
 * revert and the trust region see the full cost; ThalloX_PlanPriorCost returns the prior's share), the right-hand side -W (x - mean), the system matrix W -- in PCG's
 * preconditioner, the block and elimination factors, the assembled S, LM's diagonal and model cost, and ThalloX_PlanCovariance, whose Sigma becomes (A_FF)^-1 with W
 * inside A: a prior on one camera's pose and one more scalar is a gauge under which every camera has a finite block.  A robust loss is never applied to a prior; a held
 * scalar with a prior keeps delta = 0 and its constant term still counts in the cost.  Works with every preconditioner, linear solver, loss and mask above; no launch is
 * added to a PCG iteration.  A plan that never makes the call, clears its priors or sets no positive weight launches what it launches otherwise, bit for bit.  Between
 * Thallo_ProblemPlan and Thallo_ProblemInit, or before a re-Init: it takes effect at the next Init.
 * Returns 0, or nonzero with ThalloX_LastError naming the energy and the reason: every energy but bundle_adjustment (generated ones included), a doublePrecision = 1 state,
 * a distributed plan (ThalloX_PlanSetDistributed after this call is refused likewise), a direct-solve plan, an input that is not an Unknown, an n that is not
 * elements x components, a weight that is negative or not finite, a mean that is not finite where its weight is positive. */
int ThalloX_PlanSetPrior(Thallo_Plan* plan, int input, const float* mean, const float* weight, long n);
/* Scalars with a positive weight since the last Thallo_ProblemInit (ThalloX_PlanScheduleName then ends in "; N priors"); -1 when there was no Init. */
long ThalloX_PlanPriorTerms(Thallo_Plan* plan);
/* The prior's share of the cost at the current unknowns, sum 1/2 w (x - mean)^2, into *out (0 where no prior is in force): Thallo_ProblemCurrentCost minus it is the
 * reprojection cost.  Synchronises the plan's stream.  Returns 0, or nonzero on failure. */
int ThalloX_PlanPriorCost(Thallo_Plan* plan, double* out);

/* A robust loss for observations that are mismatches: one loss over the whole residual vector of an observation (bundle_adjustment: its 2 reprojection components).  With
 * s = |r|^2 of an observation and scale a > 0 in residual units (pixels) the cost becomes sum_o 1/2 rho(s_o):
 *   THALLOX_LOSS_TRIVIAL  rho = s                                        (the default: the squared loss)
 *   THALLOX_LOSS_HUBER    rho = s for s <= a^2, 2 a sqrt(s) - a^2 beyond;   rho' = 1, a / sqrt(s)
 *   THALLOX_LOSS_CAUCHY   rho = a^2 log(1 + s / a^2);                       rho' = 1 / (1 + s / a^2)
 * Linearisation is first order (iteratively reweighted least squares; Triggs' correction without the rho'' term): with w = sqrt(rho'(s)) in float32 every step is the GN / LM
 * step of J_s = w J, F_s = w F, so -J_s^T F_s is the exact gradient of the robust cost; Thallo_ProblemCurrentCost, the accept / revert test and function_tolerance see the
 * robust cost.  Works with every preconditioner, linear solver and mask above; no launch is added to a step.  A plan that never makes the call, or sets
 * THALLOX_LOSS_TRIVIAL, launches what it launches otherwise, bit for bit.  Between Thallo_ProblemPlan and Thallo_ProblemInit, or before a re-Init: it takes effect at the
 * next Init; ThalloX_PlanScheduleName then carries "; huber loss, scale 2" / "; cauchy loss, scale 2" (in front of the held count).  Returns 0, or nonzero with
 * ThalloX_LastError naming the energy and the reason: every energy but bundle_adjustment (generated ones included), a doublePrecision = 1 state, a distributed plan
 * (ThalloX_PlanSetDistributed after this call is refused likewise), a direct-solve plan, an unknown kind, a scale that is not finite and positive (Huber, Cauchy). */
#define THALLOX_LOSS_TRIVIAL 0
#define THALLOX_LOSS_HUBER   1
#define THALLOX_LOSS_CAUCHY  2
int ThalloX_PlanSetRobustLoss(Thallo_Plan* plan, int kind, float scale);
/* rho'(s) of every observation at the last linearisation (1 before the first), in (0, 1], into the HOST array host_out[n], the caller's observation ids: what a caller reads
 * the inliers off.  Returns the number of observations, or -1 when no loss is in force since the last Init or n is not that number.  Synchronises the plan's stream. */
long ThalloX_PlanRobustWeights(Thallo_Plan* plan, float* host_out, long n);

/* How well the cameras and points are determined: marginal blocks of the covariance at the plan's current unknowns.  With A = J_s^T J_s there (J_s carries the robust
 * weights when a loss is in force; NO LM diagonal is added, on a ThalloX_EnableLM plan too) and F the scalars the caller does not hold (ThalloX_PlanSetHeldUnknowns),
 * Sigma = (A_FF)^-1 bordered by exact zero rows and columns at the held scalars.  input 0: the 9 x 9 block of every camera ids[i] into host_out[81 i ..]; input 1: the
 * 3 x 3 block of every point ids[i] into host_out[9 i ..]; row-major, symmetric bit for bit, the caller's ids.  The blocks are UNSCALED, as the common packages return them:
 * multiply by your sigma^2.  FIXING THE GAUGE IS THE CALLER'S JOB, through ThalloX_PlanSetHeldUnknowns (a camera and one more scalar, or two cameras): without it A is
 * singular and the columns do not converge.  A point that the elimination's factor rule holds (observed once or never, or a squared pivot below 2^-16; see
 * ThalloX_PlanSchurHeldPoints) has no finite covariance: its block is filled with quiet NaNs and counted; a point the caller holds entirely returns zeros; the columns
 * of a camera nothing observes do not converge and its block stays zero.
 * Computed through the Schur complement on the cameras, S^-1 and Cp^-1 + V^T S^-1 V, by a float32 PCG on the assembled S, 64 columns at a time: the plan's last
 * Thallo_ProblemInit must have run THALLOX_SOLVER_SCHUR_EXPLICIT_PCG.  A column ends when sqrt(r . z / r0 . z0) <= rel_tol or after max_iterations; opt == NULL: 1e-6 and
 * 500 (from a CPU study in float32: the error against float64 levels off at 3e-6 ... 2e-5 of sqrt(Sigma_aa Sigma_bb) from there on).  The call re-linearises at the
 * current unknowns and leaves the solve as it was: unknowns, the LM radius, costs and the kernel statistics of the steps are untouched, and a plan that never makes
 * the call launches what it launched before.  Its work vectors are allocated at the first call and freed with the plan.  Synchronises the plan's stream.
 * Returns 0; or the number of columns that did not converge (> 0; host_out is written all the same); or a negative number with ThalloX_LastError naming the energy
 * and the reason: wherever THALLOX_SOLVER_SCHUR_EXPLICIT_PCG is refused, a plan whose last Init ran another linear solver, a call before Thallo_ProblemInit, an input
 * that is not an Unknown, n <= 0, an id out of range or repeated, a rel_tol that is not finite and positive, max_iterations < 1.
 * On a plan whose last Thallo_ProblemInit ran THALLOX_SOLVER_SCHUR_DENSE the columns come from a dense Cholesky factor of S instead (expanded and factored once per call,
 * two triangular sweeps per batch, whatever the length of the camera chain): rel_tol and max_iterations are accepted and ignored; info reports 0 iterations and a worst
 * residual of 0; not_converged -- and the return value -- count the requested camera columns at scalars whose diagonal of S is not positive (their blocks stay zero); a
 * factor that meets a pivot that is not positive returns a negative number, ThalloX_LastError naming the camera and scalar. */
typedef struct ThalloX_CovarianceOptions {
    float rel_tol;               /* default 1e-6 */
    int   max_iterations;        /* default 500 */
} ThalloX_CovarianceOptions;
typedef struct ThalloX_CovarianceInfo {
    long  iterations;            /* PCG iterations run, added over the batches of 64 columns */
    long  columns;               /* columns solved (a held scalar's unit column and a held point's columns are zero and need no solve) */
    long  not_converged;         /* ... of them not converged */
    long  nan_blocks;            /* blocks filled with NaN */
    float worst_residual;        /* the largest sqrt(r . z / r0 . z0) a column ended with */
} ThalloX_CovarianceInfo;
long ThalloX_PlanCovariance(Thallo_Plan* plan, void** problem_params, int input, const int* ids, long n, float* host_out, const ThalloX_CovarianceOptions* opt,
                            ThalloX_CovarianceInfo* info);

/* 1 if the most recent Thallo_ProblemInit on this plan succeeded (parameters bound, plugin prepared), else 0: Init itself returns void. */
int ThalloX_PlanReady(Thallo_Plan* plan);

/* Last error message of this thread ("" if none). */
const char* ThalloX_LastError(void);

/* What a problem file asks for with its `r.<residual>.J:set_materialize(true)` / `.JtJ:set_materialize(true)` lines
 * (API/src/thallo.t:5661-5690): 0 = matrix-free, 1 = `[Jt][[J]p]` (J and J^T as CSR, two SpMVs per PCG iteration), 2 = `[[Jt][J]]p`
 * (J^T J formed once, one SpMV); -1 = no plugin for the file.  Honoured by the two Laplacian energies (constant J). */
int ThalloX_ProblemFileSchedule(const char* filename);
unsigned long long ThalloX_ProblemFileHash(const char* filename, char* energy_out, int cap);
/* FNV-1a-64 of the translation unit the front-end generates from the file, residual names aside (0: outside the supported subset, ThalloX_LastError).
 * Two files with the same value state the same energy.  A file with a bundled energy's declarations runs on that energy's hand-written plugin only if
 * its text is a known one or this value is the bundled file's; otherwise on generated kernels. */
unsigned long long ThalloX_ProblemFileUnitHash(const char* filename);

/* The mini front-end (thallo_amd/csrc/dsl.hpp) run on a .t file without a device: what = 0 its declarations as text, 1 the HIP translation unit it
 * generates (residual-wise cost / evalJTF / applyJTJ / applyJ / applyJt kernels per named residual).  Returns the text's length (the copy is truncated
 * to cap - 1) or -1 (ThalloX_LastError).  A Plan on a file no hand-written plugin recognises -- or on any file under THALLO_FRONTEND=generate -- compiles
 * that unit with hipRTC and runs it. */
int ThalloX_FrontendText(const char* filename, int what, char* out, int cap);
/* ... given the problem's dimensions (the array Thallo_ProblemPlan takes): needed by files that use Sum, which is expanded for those sizes.
 * what = 2: the ROW-SLAB unit a distributed plan of the file compiles (owned-row kernels, global pixel coordinates; -1 if the file has no row-slab form) */
int ThalloX_FrontendTextDims(const char* filename, int what, const unsigned* dims, char* out, int cap);
/* Row slabs of a generated energy, host only (no device): the ghost rows g >= 1 a slab needs towards each neighbour -- the largest row span of one residual's
 * data accesses, computed arrays composed with their own footprint -- or -1 with ThalloX_LastError naming the construct that has no row-slab form
 * (SampledImage, Sparse maps, graph or 3-D domains, more than one Unknown, materialize lines, direct solve).  global_dims: the problem's dimensions. */
int ThalloX_FrontendSlabGhostRows(const char* filename, const unsigned* global_dims);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU, one process per GPU (the reference is single-device, API/src/util.t:769-772).
 *
 * Image-stencil problems are split into contiguous ROW SLABS.  Each process makes its Plan for its LOCAL image -- the rows it owns plus one
 * ghost row towards each neighbour -- passes the local buffers to Init / Step as usual, and declares the split once, before
 * Thallo_ProblemInit, with ThalloX_PlanSetDistributed.  From then on Thallo_ProblemInit / Step / CurrentCost are COLLECTIVE: every rank calls
 * them in the same order; costs, alpha and beta are rank-ordered sums, bit-identical on every rank.  Per PCG iteration each rank runs ONE
 * kernel and ONE exchange:
 *   - the caller's all-gather (RCCL: ncclAllGather on `stream`) of [alphaD, N, S1, S2 | first and last owned row of Ap], or
 *   - when device_exchange != 0 and the self-check at the first Init passes on this topology: no host-visible collective at all -- the
 *     kernel stores its scalars into every rank's mailbox and its boundary rows into the neighbours' ghost rows over xGMI
 *     (hipIpc-mapped fine-grained memory) and its last workgroup waits for the peers' granules.
 * Supported: image_warping (one ghost row per neighbour; UrShape on the unit pixel grid, W % 4 == 0; Gauss-Newton; both transports) and
 * shape_from_shading (TWO ghost rows per neighbour; Gauss-Newton and ThalloX_EnableLM; BOTH transports: per PCG iteration one exchange -- the
 * all-gather carries the GN form's sums and rows, and the LM form's alphaD, then betaN + q + the ghost rows of z, in two; on the device-side
 * transport the LM iteration is one launch + ONE mailbox / peer-to-peer exchange that also finishes alphaD, betaN, q and the zeta test,
 * thallo_hip_dist_xrows_lm); and GENERATED image energies (files run through the front-end, dsl.hpp) with one Unknown over {W, H}, every input that has
 * the H dimension over exactly {W, H}, fixed-offset accesses and residuals with the unknown-wise form: g ghost rows per neighbour as
 * ThalloX_FrontendSlabGhostRows says (the stencil's row span, >= 1), global_row0 / global_rows required when world > 1, Gauss-Newton and ThalloX_EnableLM,
 * both transports; the plan compiles the front-end's row-slab unit (ThalloX_FrontendTextDims what = 2) at this call.
 * Graph energies (arap_mesh_deformation) are split into contiguous VERTEX RANGES instead: every rank makes its Plan for the WHOLE problem, passes the
 * whole (replicated) buffers, and sets row0 / row1 to the vertex range it owns (equal ranges: N % world == 0); per PCG iteration one all-gather
 * of [alphaD, N, S1, S2 | the owned slice of A p]; the unknowns stay replicated bit for bit.  Gauss-Newton, all-gather transport.
 * bundle_adjustment is split into CAMERA SHARDS: every rank makes its Plan for its SUB-INSTANCE -- its cameras (count padded to a multiple of 4 with
 * unobserved cameras), ALL points, the observations of its cameras with camera indices renumbered locally; row0 / row1 are not used.  The camera block
 * of J^T J p is complete on the rank; the point block is a partial sum and is all-reduced (`allreduce`, 3P floats per PCG iteration), after which
 * every rank updates the (replicated) points identically; the scalars: one all-gather of the ranks' camera sums + the point sums every rank
 * computes for itself.  Gauss-Newton and, after ThalloX_EnableLM, Levenberg-Marquardt (round 6: the element-wise LM kernels run on the camera block and
 * the point block separately; accept / revert and the trust region are decided by every rank on identical scalars).
 * Everything else returns an error.
 * ------------------------------------------------------------------------------------------ */
/* Every rank contributes `bytes_per_rank` bytes at `send` and receives world * bytes_per_rank at `recv`, rank order; DEVICE pointers;
 * enqueued on `stream` (a hipStream_t).  Return 0 on success.  world == 1: may be NULL. */
typedef int (*ThalloX_AllGatherFn)(void* user, const void* send, void* recv, long bytes_per_rank, void* stream);
/* In-place sum over all ranks of `count` floats at `buf` (DEVICE pointer), on `stream` (ncclAllReduce, ncclSum).  Only the shard form needs it. */
typedef int (*ThalloX_AllReduceFn)(void* user, void* buf, long count, void* stream);
typedef struct ThalloX_Distributed {
    int rank, world;                 /* world <= 8 (THALLO_DIST_MAX_WORLD) */
    unsigned int row0, row1;         /* owned rows [row0, row1) of the local image; g ghost rows above iff row0 == g, below iff row1 == H_local - g (g >= 1: the energy's, see below) */
    ThalloX_AllGatherFn allgather;
    void* user;
    int device_exchange;             /* 1: try the mailbox / peer-to-peer exchange (falls back to the all-gather if its self-check fails) */
    unsigned int global_row0;        /* global index of the local image's row 0 (ghost rows included) and the global image height: energies */
    unsigned int global_rows;        /* whose expressions use pixel coordinates (shape_from_shading) need them; 0 0 = not given */
    ThalloX_AllReduceFn allreduce;   /* bundle adjustment (camera shards) only; NULL otherwise */
} ThalloX_Distributed;
/* Graph energies (arap_mesh_deformation) as a REAL vertex partition (round 3; the replicated "vertex range" form stays): the Plan is made for the rank's LOCAL
 * sub-problem -- its owned vertices first (local ids [0, n_own)), then the GHOSTS: vertices owned elsewhere that an owned vertex shares an edge with; the edges are all
 * directed edges with an owned end.  Call this before ThalloX_PlanSetDistributed (whose row0 / row1 are then 0 / n_own).  boundary_units: local ids of this rank's owned
 * vertices that some other rank holds as ghosts, in an order every rank agrees on (ascending global id); ghost_units[g] (local id, >= n_own), filled from position
 * ghost_src_pos[g] of rank ghost_src_rank[g]'s boundary list.  Host arrays, copied.  Per PCG iteration the ranks exchange [alphaD | N, S1, S2 | A p at the boundary
 * vertices] in one all-gather; vectors, memory and the vector updates are local-sized (thallo_amd/distributed_graph.py builds the lists from the global edge list). */
int ThalloX_PlanSetGhostExchange(Thallo_Plan* plan, int n_boundary, const int* boundary_units, int n_ghost, const int* ghost_units, const int* ghost_src_rank,
                                 const int* ghost_src_pos);
/* Collective.  0 on success, -1 on error (ThalloX_LastError); every rank gets the same answer. */
int ThalloX_PlanSetDistributed(Thallo_Plan* plan, const ThalloX_Distributed* cfg);
/* The collectives INSIDE the library (round 3; no callback, no host-language hop in the PCG loop): rank 0 makes a 128-byte RCCL unique id, the application
 * hands it to every rank by whatever channel it has (MPI, a file, torch.distributed), and each rank gives it to its plan BEFORE ThalloX_PlanSetDistributed
 * (collective: ncclCommInitRank, the rank's GPU current).  A NULL allgather / allreduce in ThalloX_Distributed then means ncclAllGather / ncclAllReduce on the
 * plan's stream.  RCCL is bound at run time (dlopen: the copy already in the process if there is one); -1 + ThalloX_LastError when it is not there.
 * ThalloX_RcclSelfTest: a one-rank communicator moves a small buffer through both collectives (0 = fine). */
int ThalloX_RcclAvailable(void);      /* 1: librccl can be bound in this process (rank-local; all-reduce it before the collective ThalloX_PlanUseRccl) */
int ThalloX_RcclUniqueId(unsigned char* id_out128);
int ThalloX_PlanUseRccl(Thallo_Plan* plan, const unsigned char* id128, int rank, int world);
int ThalloX_RcclSelfTest(void);
/* what the plan's communicator says about itself: out3 = { ncclCommCount, ncclCommCuDevice, ncclCommUserRank }, -1 where there is no communicator or no answer.
 * Diagnostics for the first run on a real node: a count of 1 next to a torch.distributed world of N means the ranks never met. */
void ThalloX_PlanRcclInfo(Thallo_Plan* plan, int out3[3]);
/* JSON text: transport in use ("exchange": "p2p-mailbox" | "allgather"), memory kind of the mapped blocks, self-check outcome. */
const char* ThalloX_PlanDistributedInfo(Thallo_Plan* plan);
/* what = 0: read (and with value != 0 clear) the device-side exchange's error word -- 1 if a bounded mailbox wait timed out since the last clear
 *           (synchronises the stream); what = 1: value 0 switches this plan to the all-gather transport for good (every rank must do the same);
 *           what = 2 (tests): the value-th rank-local launch from now on reports a failure.
 * Returns the word / 0, or -1.
 *
 * Failures across ranks.  Decisions that change the sequence of collectives are unanimous (set-up, Init, the device-side exchange's self-check: a
 * rank that cannot allocate, bind or prepare says so in an agreement, and then EVERY rank returns the error).  A launch or copy that fails on ONE
 * rank in the middle of a step does not end that rank's part of the sequence: it skips its own launches, keeps issuing every collective with a
 * poisoned payload (NaN scalars on every rank) and goes on returning 1 from Thallo_ProblemStep like the others; at the next cost evaluation --
 * the end of Thallo_ProblemSolve, every Thallo_ProblemCurrentCost, every LM step -- all ranks learn of it together, report it, and their plans
 * stop (Step returns 0, the cost is NaN).  What stays rank-local: a failing collective callback itself, and running out of memory for the two
 * message buffers inside ThalloX_PlanSetDistributed before the first collective. */
int ThalloX_DistributedControl(Thallo_Plan* plan, int what, int value);
/* bench: `reps` back-to-back launches of the one-kernel PCG iteration on this rank's slab, without the exchange (kernel time per rank) */
int ThalloX_DistributedKernelOnly(Thallo_Plan* plan, int reps);

#ifdef __cplusplus
}
#endif
#endif
