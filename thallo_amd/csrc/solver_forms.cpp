// solver_forms.cpp -- the opt-in forms of a one-GPU PCG plan (solver.hpp "solver_forms.cpp"): robust losses, held unknowns, the block-Jacobi preconditioner and the
// Schur complement on the cameras.  What they ask for is set between Plan and Init (the setters), decided and allocated at Init (forms_prepare: never inside a step) and
// run by ONE set-up behind PCGInit1 (forms_setup), ONE GN step (step_gn_blocks) and ONE LM loop (lm_loop_blocks) for the block-Jacobi and the Schur form alike.
#include "solver.hpp"
#include <cmath>
#include <cstdio>

namespace thallo {

// Init: every opt-in form needs a one-GPU PCG plan (`ok`: the plugin's *_ok() answer; `what_needs`: "a robust loss needs").  true: refused, the error is set
bool Plan::refuse_unless_one_gpu_pcg(bool ok, const char* what_needs)
{
    if (!dist_ && !plugin->direct_solve() && ok) return false;
    set_error("%s: %s a one-GPU PCG plan", plugin->name(), what_needs);
    return true;
}

// The blocking read-back of one status word of the last step (-1: the copy failed)
int Plan::read_word(const unsigned* dev)
{
    unsigned n = 0;
    if (hipMemcpyAsync(&n, dev, sizeof(n), hipMemcpyDeviceToHost, ctx.stream) != hipSuccess || hipStreamSynchronize(ctx.stream) != hipSuccess) return -1;
    return (int)n;
}

// Init, behind prepare() (the plugin's numbering is decided): what this solve runs, in this order; every buffer of a form is allocated here.  Nonzero: the plan is not ready
int Plan::forms_prepare()
{
    if (held_prepare()) return -1;
    if (prior_prepare()) return -1;
    robust_on_ = 0;
    if (robust_want_ && refuse_unless_one_gpu_pcg(plugin->robust_ok(), "a robust loss needs")) return -1;
    if (plugin->robust_prepare(robust_want_, robust_want_scale_)) return -1;      // (kind 0: the plugin's routes launch what they launch without the call)
    robust_on_ = robust_want_; robust_on_scale_ = robust_want_scale_;
    block_on_ = false;
    schur_on_ = false;
    if (coarse_want_ && !(schur_want_ && schur_explicit_want_)) {
        set_error("%s: the two-level preconditioner (ThalloX_PlanSetPreconditioner THALLOX_PRECOND_TWO_LEVEL) needs the assembled reduced camera matrix: set "
                  "ThalloX_PlanSetLinearSolver(plan, THALLOX_SOLVER_SCHUR_EXPLICIT_PCG); this plan's linear solver is %s", plugin->name(),
                  schur_want_ ? "THALLOX_SOLVER_SCHUR_PCG" : "THALLOX_SOLVER_PCG");
        return -1;
    }
    if (schur_want_) { if (schur_prepare()) return -1; schur_on_ = true; }      // (its preconditioner is the camera blocks whatever block_want_ says)
    else if (ReducedCameraSystem* rs = reduced()) rs->retire();      // (a plan that ran the assembled form and was switched back: its structure goes, the dense matrix with it)
    if (!schur_want_ && block_want_) { if (block_prepare()) return -1; block_on_ = true; }
    if (schur_on_ || block_on_) { precond_regions_ = block_regions_; if (schur_on_) precond_regions_.n = 1; }      // (Schur: the camera region alone)
    return 0;
}

// Behind PCGInit1 (+ PCGFinalizeDiagonal in LM; r = b = -J^T F over all unknowns, pre = the point-Jacobi M^-1, the blocks' fallback), what the forms put in front of the
// loop.  shift: the LM CtC or NULL; b: the right-hand side (GN: r); rz_out: the slot of alphaN_0; nb: PCGInit1's partial count.  -> the slot's partial count (nb where no form
// writes it anew), or a negative code with `what` naming what failed.
//   held unknowns: pre = z = 0 at the held scalars, alphaN_0 over the free ones; behind it every launch forms M^-1 r from pre or from the blocks
//   block forms:   H of both regions (held: its rows and columns in one launch -- the camera blocks and the point blocks lie one behind the other), G of the preconditioner's
//                  regions, z = G^T G r and alphaN_0 anew.  Schur: in between the elimination factor, y and g (r_c becomes g; the point part of r stays b_p) and, assembled,
//                  W and S -- every step: B, the factor and in LM CtC are the step's.  g, W, the assembly, both applies and the back-substitution inherit the held rule
//                  through the two factors
int Plan::forms_setup(const float* shift, const float* b, float* rz_out, int nb, const char*& what)
{
    hipStream_t s = ctx.stream;
    what = "held unknowns: the mask launch";
    if (held_on() && (nb = hold_pcg(rz_out)) < 0) return nb;
    if (!schur_on_ && !block_on_) return nb;
    what = schur_on_ ? "Schur-complement set-up" : "block preconditioner set-up";
    int rc = plugin->block_diag(ctx, block_H_);
    if (rc < 0) return rc;
    if (held_on()) { TimedLaunch t(ctx, "BlockHold"); if ((rc = thallo_hip_block_hold(block_regions_, held_mask_, block_H_, s)) < 0) return rc; }
    { TimedLaunch t(ctx, "BlockFactor"); if ((rc = thallo_hip_block_factor(precond_regions_, block_H_, shift, v_.pre, block_G_, block_status_, s)) < 0) return rc; }
    if (held_on()) { TimedLaunch t(ctx, "BlockHoldFactor"); if ((rc = thallo_hip_block_hold_factor(precond_regions_, held_mask_, block_G_, s)) < 0) return rc; }
    if (schur_on_) {
        ReducedCameraSystem& rs = *reduced();
        if ((rc = rs.reduce(ctx, block_H_ + schur_hp_off_, shift ? shift + schur_pt_off_ : nullptr, b, schur_g_, v_.r, held_on() ? held_mask_ : nullptr)) < 0) return rc;
        if (rs.assembled() && (rc = rs.assemble(ctx, block_H_, shift)) < 0) return rc;
        if (coarse_on() && !schur_empty() && (rc = rs.coarse_setup(ctx, held_on() ? held_mask_ : nullptr)) < 0) { what = "two-level preconditioner set-up"; return rc; }
    }
    { TimedLaunch t(ctx, "BlockApply"); rc = thallo_hip_block_apply(precond_regions_, block_G_, v_.r, v_.z, rz_out, nullptr, s); }
    return coarse_apply(rz_out, rc, nullptr);
}

int Plan::coarse_apply(float* part, int nb, const unsigned* gate)
{
    if (!coarse_on() || schur_empty() || nb < 0) return nb;
    if (nb + THALLO_HIP_COARSE_PARTIALS > THALLO_HIP_MAX_PARTIALS) return -(int)hipErrorInvalidValue;
    const int nc = reduced()->coarse_apply(ctx, held_on() ? held_mask_ : nullptr, v_.r, v_.z, part + nb, gate);
    return nc < 0 ? nc : nb + nc;
}

// One GN step of the block-Jacobi and of the Schur form: the generic GN loop (step_gn's last branch) with M^-1 = G^T G -- forms_setup behind PCGInit1 replaces its
// point-Jacobi z and sum, PCGStep2 is thallo_hip_block_step2; PCGInit1 leaves p_prev = 0 and the first iteration forms p = z, as in every schedule.
// Schur: the loop runs on the reduced system (S, g) -- PCGStep3 and the plugin's apply instead of its PCGStep1 --, every vector of it is its camera part ([0, 9 C) of the
// plan's vectors), the point part of r stays b_p, which the back-substitution reads.  The loop's last delta_c += alpha p rides in the back-substitution's camera launch;
// PCGLinearUpdate then adds the complete delta.
int Plan::step_gn_blocks(int ev_iter)
{
    const int L = schur_empty() || schur_dense() ? 0 : sp.lIterations, B = 2;   // slot layout: alphaN_k = B+2k, alphaD_k = B+2k+1, betaN_k = B+2k+2
    hipStream_t s = ctx.stream;
    int ev_lin, nb;
    if (!gn_begin(ev_iter, ev_lin)) return 0;
    if (schur_dense() && !schur_dense_step(schur_g_)) return 0;      // (delta_c is in place, or the factor failed: nothing has been applied)
    for (int k = 0; k < L; ++k) {
        const int jN = B + 2 * k, jD = jN + 1, jB = jN + 2;
        const PrevAlpha a = prev_alpha(k);
        if (schur_on_) {
            {   TimedLaunch t(ctx, "PCGStep3");
                nb = thallo_hip_pcg_pupdate(v_.z, v_.p[cur_], v_.p[cur_ ^ 1], v_.delta, schur_n_, k == 0 ? 1 : 0, a.aN, a.aD, sum(jN), s); }
            if (nb < 0) { set_error("PCGStep3 launch failed (%d)", nb); return 0; }
            nb = reduced()->apply(ctx, v_.p[cur_ ^ 1], gn_shift(), v_.Ap, slot(jD), nullptr);
            if (nb < 0) { set_error("Schur apply launch failed (%d)", nb); return 0; }
        } else {
            nb = gn_step1(k, a, sum(jN), slot(jD));
            if (nb < 0) { set_error("PCGStep1 launch failed (%d)", nb); return 0; }
        }
        set_nb(jD, nb); finish(jD); cur_ ^= 1;
        {   TimedLaunch t(ctx, "BlockStep2");
            nb = thallo_hip_block_step2(precond_regions_, block_G_, v_.r, v_.Ap, v_.z, sum(jN), sum(jD), slot(jB), s); }
        if (nb < 0) { set_error("PCGStep2 (block) launch failed (%d)", nb); return 0; }
        if ((nb = coarse_apply(slot(jB), nb, nullptr)) < 0) { set_error("PCGStep2 (coarse apply) launch failed (%d)", nb); return 0; }
        set_nb(jB, nb); finish(jB);
    }
    if (schur_on_) {
        const int jL = B + 2 * (L - 1);
        nb = reduced()->back(ctx, v_.r, v_.delta, L > 0 ? v_.p[cur_] : nullptr, sum(L > 0 ? jL : B), sum(L > 0 ? jL + 1 : B));
        if (nb < 0) { set_error("Schur back-substitution launch failed (%d)", nb); return 0; }
    }
    const int ev_fin = gn_finish(L, ev_lin);
    linear_update_tail(schur_on_ ? 0 : L, false);
    return gn_end(ev_fin, ev_iter);
}

// The LM loop of the block-Jacobi and of the Schur form, on one GPU: the reference-shaped loop (PCGStep3 / the apply with CtC folded in / PCGStep2 / zeta, the residual
// reset every residual_reset_period iterations) with thallo_hip_block_step2_lm as PCGStep2; every launch takes the gate word.  Block-Jacobi: on the full system, through
// the plugin's applyJTJ (EnergyPlugin::block_precond_ok: it adds CtC p).  Schur: on the reduced system (S + CtC_c, g): b := g, Q_k = 0.5 delta_c . (r_c + g) -- the full
// model's value minus the constant 0.5 b_p . Cp^-1 b_p, which the zeta test (Ceres' criterion on the reduced model) does not use --, then the back-substitution, which
// does not take the gate word.
void Plan::lm_loop_blocks(LmStep& st)
{
    hipStream_t s = st.s;
    const bool schur = schur_on_;
    const int L = schur_empty() || schur_dense() ? 0 : st.L, B = st.B, QS = st.QS, T0 = st.T0, T1 = st.T1;
    const long n = schur ? schur_n_ : v_.n;
    const float* b = schur ? schur_g_ : v_.b;
    float* p = v_.p[0];
    auto apply = [&](const float* x, float* Ax, float* xAx_out) {      // (S + CtC_c) x or (J^T J + CtC) x ; the partials of x . that
        if (schur) return reduced()->apply(ctx, x, lm_shift(), Ax, xAx_out, ctx.gate);
        ctx.lm_ctc = lm_shift();
        const int rc = plugin->apply_jtj(ctx, x, Ax, xAx_out);
        ctx.lm_ctc = nullptr;
        return rc;
    };
    int nb = 0;
    if (schur_dense() && !schur_dense_step(schur_g_)) { st.failed = true; return; }      // (S carries the step's CtC: each step factors anew)
    for (int k = 0; k < L; ++k) {
        const int jN = B + 2 * k, jD = jN + 1, jB = jN + 2;
        {   TimedLaunch t(ctx, "PCGStep3");                   // p = z + beta p  (k = 0: p = z)
            st.check(thallo_hip_pcg_pupdate(v_.z, p, p, nullptr, n, k == 0, sum(k ? jN - 2 : jN), sum(k ? jD - 2 : jD), sum(jN), s), "PCGStep3 launch"); }
        if (st.failed) return;
        nb = apply(p, v_.Ap, slot(jD));                       // alphaD
        st.check(nb, schur ? "Schur apply launch" : "PCGStep1 launch");
        if (st.failed) return;
        set_nb(jD, nb);
        int nbq = 0;
        if (((k + 1) % sp.residual_reset_period) == 0) {      // :1653-1657: r = b - A delta, one more apply
            { TimedLaunch t(ctx, "PCGStep2"); st.check(thallo_hip_lm_step2_first_half(v_.delta, p, n, sum(jN), sum(jD), s), "PCGStep2 (first half) launch"); }
            if (st.failed) return;
            nb = apply(v_.delta, v_.Adelta, slot(T0));
            st.check(nb, schur ? "Schur apply (reset) launch" : "computeAdelta launch");
            if (st.failed) return;
            // (the second half's point-Jacobi z and betaN partials go to waste -- the partials into the scratch slot T1 --, the block apply behind it forms both anew: two
            //  launches on every residual_reset_period-th iteration rather than one more fused kernel)
            { TimedLaunch t(ctx, "PCGStep2"); nb = thallo_hip_lm_step2_second_half(v_.r, b, v_.Adelta, v_.pre, v_.z, v_.delta, n, slot(T1), slot(QS), s); st.check(nb, "PCGStep2 (second half) launch"); }
            if (st.failed) return;
            nbq = nb;
            { TimedLaunch t(ctx, "BlockApply"); nb = thallo_hip_block_apply(precond_regions_, block_G_, v_.r, v_.z, slot(jB), ctx.gate, s); st.check(nb, "PCGStep2 (block apply) launch"); }
            if (st.failed) return;
            nb = coarse_apply(slot(jB), nb, ctx.gate); st.check(nb, "PCGStep2 (coarse apply) launch");
        } else {
            {   TimedLaunch t(ctx, "BlockStep2LM");
                nb = thallo_hip_block_step2_lm(precond_regions_, block_G_, v_.delta, p, v_.r, v_.Ap, v_.z, b, sum(jN), sum(jD), slot(jB), slot(QS), ctx.gate, s); }
            st.check(nb, "PCGStep2 launch");
            nbq = nb;
            if (st.failed) return;
            nb = coarse_apply(slot(jB), nb, ctx.gate); st.check(nb, "PCGStep2 (coarse apply) launch");
        }
        if (st.failed) return;
        set_nb(jB, nb); set_nb(QS, nbq);
        st.k_done = k + 1;
        {   TimedLaunch t(ctx, "PCGZeta");
            st.check(thallo_hip_lm_zeta(sum(QS), k, sp.q_tolerance, st.lmst, s), "PCGZeta launch"); }
        if (st.failed) return;
    }
    if (!schur) return;
    const thallo_sum_t none = { nullptr, 0 };
    st.check(reduced()->back(ctx, v_.b, v_.delta, nullptr, none, none), "Schur back-substitution launch");
}

const char* Plan::schedule_name()
{
    std::string& t = schedule_text_;
    t = plugin->schedule_name();
    if (schur_on_ || schur_want_) {
        if (schur_on_ ? schur_assembled() : schur_explicit_want_) {
            t += "; Schur complement on the cameras, assembled";
            if (schur_on_) t += " (" + std::to_string(reduced()->blocks()) + " blocks)";
        } else t += "; Schur complement on the cameras";
        if (schur_on_ ? schur_dense() : schur_dense_want_) {
            t += "; dense Cholesky of S";
            if (schur_on_) t += " (n = " + std::to_string(reduced()->dense_n()) + ")";
        } else if (schur_on_ ? coarse_on() : coarse_want_ && schur_explicit_want_) {
            t += "; two-level on S";
            if (schur_on_) t += " (" + std::to_string(reduced()->coarse_aggregates()) + " aggregates, n_c = " + std::to_string(reduced()->coarse_n()) + ")";
        } else t += "; block-Jacobi on S";
    } else if (block_on_ || block_want_) t += "; block-Jacobi preconditioner (unfused PCG loop)";
    const int kind = ready_ ? robust_on_ : robust_want_;      // (since the last Init: what runs; before it: what was asked for)
    if (kind) {
        char sc[32]; snprintf(sc, sizeof sc, "%g", (double)(ready_ ? robust_on_scale_ : robust_want_scale_));
        t += kind == THALLOX_LOSS_HUBER ? "; huber loss, scale " : "; cauchy loss, scale ";
        t += sc;
    }
    if (held_on()) t += "; " + std::to_string(held_count_) + " unknowns held";
    if (prior_on()) t += "; " + std::to_string(prior_count_) + " priors";
    return t.c_str();
}

// ------------------------------------------------------------------ robust losses (energy_ba.hip, DESIGN.md "Robust losses")
int Plan::set_robust_loss(int kind, float scale)
{
    if (kind != THALLOX_LOSS_TRIVIAL && kind != THALLOX_LOSS_HUBER && kind != THALLOX_LOSS_CAUCHY) { set_error("%s: unknown robust loss kind %d", plugin->name(), kind); return -1; }
    if (kind == THALLOX_LOSS_TRIVIAL) { robust_want_ = 0; robust_want_scale_ = 0.0f; return 0; }
    if (!ok_) return -1;
    if (plugin->direct_solve()) { set_error("%s: a direct-solve plan has no linearisation to reweight (no robust loss)", plugin->name()); return -1; }
    if (!plugin->robust_ok()) { set_error("%s: no robust loss for this energy (its cost, precomputeJ and apply routes have no robust instantiation; bundle_adjustment's do)", plugin->name()); return -1; }
    if (dist_) { set_error("%s: robust losses run on one GPU (this plan is distributed)", plugin->name()); return -1; }
    if (!(scale > 0.0f) || !std::isfinite(scale)) { set_error("%s: the scale of a robust loss must be finite and positive (got %g)", plugin->name(), (double)scale); return -1; }
    robust_want_ = kind; robust_want_scale_ = scale;
    return 0;
}

long Plan::robust_weights(float* host_out, long n)
{
    if (!ok_ || !robust_on()) return -1;
    return plugin->robust_weights(ctx, host_out, n);
}

// ------------------------------------------------------------------ held unknowns (held.hip, DESIGN.md "Held unknowns")
int Plan::set_held_unknowns(int input, const unsigned char* held, long n)
{
    if (!ok_) return -1;
    const auto& imgs = plugin->unknown_images();
    int k = -1;
    for (size_t i = 0; i < imgs.size(); ++i) if (imgs[i].param_index == input) k = (int)i;
    if (!held) { if (k >= 0) held_masks_.erase(k); return 0; }
    if (plugin->direct_solve()) { set_error("%s: a direct-solve plan has no PCG loop to hold unknowns in", plugin->name()); return -1; }
    if (!plugin->hold_ok()) { set_error("%s: no held unknowns for this energy (not every PCG route of its plugin takes M^-1 from the stored vector; bundle_adjustment's do)", plugin->name()); return -1; }
    if (dist_) { set_error("%s: held unknowns run on one GPU (this plan is distributed)", plugin->name()); return -1; }
    if (k < 0) { set_error("%s: input %d is not an Unknown of this energy", plugin->name(), input); return -1; }
    if (n != imgs[(size_t)k].n_floats) { set_error("%s: the mask of input %d has %ld bytes, the unknown has %ld scalars (elements x components)", plugin->name(), input, n, imgs[(size_t)k].n_floats); return -1; }
    held_masks_[k].assign(held, held + n);
    return 0;
}

int Plan::held_prepare()
{   // the masks in the plan's internal ids, counted, uploaded
    held_count_ = -1; held_first_ = 0;
    if (held_masks_.empty()) return 0;
    if (refuse_unless_one_gpu_pcg(plugin->hold_ok(), "held unknowns need")) return -1;
    std::vector<unsigned char> flat((size_t)v_.n, 0);
    for (const auto& m : held_masks_) plugin->hold_to_internal(m.first, m.second.data(), flat.data());
    long count = 0;
    for (unsigned char f : flat) count += f != 0;
    if (count == v_.n) { set_error("%s: the mask holds every unknown (%ld scalars): nothing is left to solve for", plugin->name(), count); return -1; }
    { const long n0 = plugin->unknown_images()[0].n_floats; for (long i = 0; i < n0; ++i) held_first_ += flat[(size_t)i] != 0; }
    held_count_ = count;
    if (count == 0) return 0;      // (nothing held: the plan launches what it launches without a mask)
    if (!held_mask_ && !(held_mask_ = (unsigned char*)device_alloc((size_t)v_.n_alloc + 64))) { held_count_ = -1; set_error("%s: out of device memory for the mask of held unknowns", plugin->name()); return -1; }
    if (hipMemcpy(held_mask_, flat.data(), flat.size(), hipMemcpyHostToDevice) != hipSuccess) { held_count_ = -1; set_error("%s: cannot upload the mask of held unknowns", plugin->name()); return -1; }
    return 0;
}

int Plan::hold_pcg(float* rz_out)
{
    TimedLaunch t(ctx, "HoldPCG");
    return thallo_hip_hold_pcg(held_mask_, v_.r, v_.pre, v_.z, v_.n, rz_out, ctx.stream);
}

// ------------------------------------------------------------------ Gaussian priors (prior.hip, DESIGN.md "Gaussian priors")
int Plan::set_prior(int input, const float* mean, const float* weight, long n)
{
    if (!ok_) return -1;
    const auto& imgs = plugin->unknown_images();
    int k = -1;
    for (size_t i = 0; i < imgs.size(); ++i) if (imgs[i].param_index == input) k = (int)i;
    if (!weight) { if (k >= 0) prior_inputs_.erase(k); return 0; }
    if (plugin->direct_solve()) { set_error("%s: a direct-solve plan has no PCG loop to carry a prior through", plugin->name()); return -1; }
    if (!plugin->hold_ok() || !plugin->apply_adds_ctc()) { set_error("%s: no priors for this energy (not every route of its plugin takes a flat diagonal next to J^T J; bundle_adjustment's do)", plugin->name()); return -1; }
    if (dist_) { set_error("%s: priors run on one GPU (this plan is distributed)", plugin->name()); return -1; }
    if (k < 0) { set_error("%s: input %d is not an Unknown of this energy", plugin->name(), input); return -1; }
    if (n != imgs[(size_t)k].n_floats) { set_error("%s: the prior of input %d has %ld scalars, the unknown has %ld (elements x components)", plugin->name(), input, n, imgs[(size_t)k].n_floats); return -1; }
    if (!mean) { set_error("%s: the prior of input %d has weights but no means", plugin->name(), input); return -1; }
    for (long i = 0; i < n; ++i) {
        if (!(weight[i] >= 0.0f) || !std::isfinite(weight[i])) { set_error("%s: the prior's weight of scalar %ld of input %d must be finite and not negative (got %g)", plugin->name(), i, input, (double)weight[i]); return -1; }
        if (weight[i] > 0.0f && !std::isfinite(mean[i])) { set_error("%s: the prior's mean of scalar %ld of input %d must be finite where its weight is positive (got %g)", plugin->name(), i, input, (double)mean[i]); return -1; }
    }
    PriorInput& in = prior_inputs_[k];
    in.mean.assign(mean, mean + n); in.weight.assign(weight, weight + n);
    return 0;
}

int Plan::prior_prepare()
{   // the planes in the plan's internal ids, counted, uploaded
    prior_count_ = 0;
    if (prior_inputs_.empty()) return 0;
    if (refuse_unless_one_gpu_pcg(plugin->hold_ok() && plugin->apply_adds_ctc(), "priors need")) { prior_count_ = -1; return -1; }
    std::vector<float> w((size_t)v_.n, 0.0f), mu((size_t)v_.n, 0.0f);
    for (const auto& in : prior_inputs_) { plugin->prior_to_internal(in.first, in.second.weight.data(), w.data()); plugin->prior_to_internal(in.first, in.second.mean.data(), mu.data()); }
    long count = 0;
    for (size_t i = 0; i < w.size(); ++i) { if (w[i] > 0.0f) ++count; else mu[i] = 0.0f; }
    if (count == 0) return 0;      // (no positive weight: the plan launches what it launches without a prior)
    const size_t bytes = ((size_t)v_.n_alloc + 64) * sizeof(float);
    if (!prior_w_) { prior_w_ = (float*)device_alloc(bytes); prior_mu_ = (float*)device_alloc(bytes); prior_shift_ = (float*)device_alloc(bytes); }
    if (!v_.diag) v_.diag = (float*)device_alloc((size_t)v_.n_alloc * sizeof(float));      // (GN keeps no raw diagonal otherwise; the LM vectors take it over)
    if (!prior_w_ || !prior_mu_ || !prior_shift_ || !v_.diag) { prior_w_ = prior_mu_ = prior_shift_ = nullptr; set_error("%s: out of device memory for the priors' planes", plugin->name()); return -1; }
    if (hipMemcpy(prior_w_, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(prior_mu_, mu.data(), mu.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { set_error("%s: cannot upload the priors' planes", plugin->name()); return -1; }
    prior_count_ = count;
    return 0;
}

int Plan::prior_cost_partials(float* out, int onto)
{
    TimedLaunch t(ctx, "PriorCost");
    const long n0 = plugin->unknown_images()[0].n_floats;
    return thallo_hip_prior_cost(prior_w_, prior_mu_, plugin->unknown_ptr(0), n0 < v_.n ? plugin->unknown_ptr(1) : nullptr, n0, v_.n, out, onto, ctx.stream);
}

int Plan::prior_init(float* rz_out)
{
    TimedLaunch t(ctx, "PriorInit");
    const long n0 = plugin->unknown_images()[0].n_floats;
    return thallo_hip_prior_init(prior_w_, prior_mu_, plugin->unknown_ptr(0), n0 < v_.n ? plugin->unknown_ptr(1) : nullptr, n0, v_.n, v_.r, v_.diag, v_.pre, v_.z,
                                 plugin->use_preconditioner() ? 1 : 0, rz_out, ctx.stream);
}

// The cost kernel's partials with the prior's added onto the first of them, in the same slot: the slot's one reader adds everything in a fixed order and the slot keeps its
// count, with priors and without (bundle adjustment's cost kernel fills all THALLO_HIP_MAX_PARTIALS from 262144 observations on: there is no room behind them)
int Plan::cost_partials(float* out)
{
    const int nb = plugin->cost(ctx, out);      // (it also brings the plan's copy of the unknowns up to date: the prior's launch reads that copy)
    if (nb < 1 || !prior_on()) return nb;
    return prior_cost_partials(out, nb);
}

int Plan::prior_cost(double* out)
{
    if (!ok_ || !out) return -1;
    *out = 0.0;
    if (!ready_ || !prior_on()) return 0;
    float* part = slot(1);      // (LM's q slot: written anew by every step before it is read)
    const int nb = prior_cost_partials(part, 0);
    if (nb < 0) { set_error("%s: the prior's cost launch failed (%d)", plugin->name(), nb); return -1; }
    float h[THALLO_HIP_PRIOR_COST_PARTIALS];
    if (hipMemcpyAsync(h, part, sizeof(float) * (size_t)nb, hipMemcpyDeviceToHost, ctx.stream) != hipSuccess || hipStreamSynchronize(ctx.stream) != hipSuccess) {
        set_error("%s: cannot read the prior's cost", plugin->name()); return -1;
    }
    for (int i = 0; i < nb; ++i) *out += (double)h[i];
    return 0;
}

// PCGStep3 + the apply of one iteration of the generic GN loop.  Without priors the plugin's pcg_step1; with them the same two launches, the apply through the plugin's
// CtC-carrying entry point with w as the diagonal (ungated: GN has no gate word)
int Plan::gn_step1(int k, const PrevAlpha& a, thallo_sum_t bN, float* out)
{
    if (!prior_on()) return plugin->pcg_step1(ctx, v_, cur_, k == 0, a.aN, a.aD, bN, out);
    { TimedLaunch t(ctx, "PCGStep3"); const int rc = thallo_hip_pcg_pupdate(v_.z, v_.p[cur_], v_.p[cur_ ^ 1], v_.delta, v_.n, k == 0 ? 1 : 0, a.aN, a.aD, bN, ctx.stream); if (rc < 0) return rc; }
    ctx.lm_ctc = prior_w_;
    const int nb = plugin->apply_jtj(ctx, v_.p[cur_ ^ 1], v_.Ap, out);
    ctx.lm_ctc = nullptr;
    return nb;
}

// ------------------------------------------------------------------ block-Jacobi preconditioner (block_precond.hip, DESIGN.md "Block-Jacobi preconditioner")
int Plan::set_preconditioner(int kind)
{
    if (kind != THALLOX_PRECOND_JACOBI && kind != THALLOX_PRECOND_BLOCK_JACOBI && kind != THALLOX_PRECOND_TWO_LEVEL) { set_error("%s: unknown preconditioner kind %d", plugin->name(), kind); return -1; }
    if (kind == THALLOX_PRECOND_JACOBI) { block_want_ = false; coarse_want_ = false; return 0; }
    if (!ok_) return -1;
    if (!plugin->block_precond_ok()) { set_error("%s: no block-Jacobi preconditioner for this energy (its plugin states no blocks; bundle_adjustment does)", plugin->name()); return -1; }
    if (dist_) { set_error("%s: the block-Jacobi preconditioner runs on one GPU (this plan is distributed)", plugin->name()); return -1; }
    if (plugin->direct_solve()) { set_error("%s: a direct-solve plan has no PCG loop to precondition", plugin->name()); return -1; }
    block_want_ = true;
    coarse_want_ = kind == THALLOX_PRECOND_TWO_LEVEL;
    return 0;
}

// ------------------------------------------------------------------ two-level preconditioner on the assembled S (ba_coarse.hip, DESIGN.md "Two-level preconditioner")
int Plan::set_coarse_aggregates(int k, const int* agg, long n)
{
    if (!ok_) return -1;
    const ReducedCameraSystem* rs = reduced();
    const long C_ = rs ? rs->elements(0) : -1;
    if (!rs) { set_error("%s: no two-level preconditioner for this energy (its plugin assembles no reduced matrix; bundle_adjustment does)", plugin->name()); return -1; }
    if (!agg) {
        if (k < 0 || n != 0) { set_error("%s: coarse aggregates: cameras_per_aggregate must be >= 0 (0: the default) and n = 0 without an array (got %d, n = %ld)", plugin->name(), k, n); return -1; }
        coarse_k_ = k; coarse_agg_.clear();
        return 0;
    }
    if (n != C_) { set_error("%s: coarse aggregates: the array has %ld ids, the plan has %ld cameras", plugin->name(), n, C_); return -1; }
    int K_ = 0;
    for (long c = 0; c < n; ++c) {
        if (agg[c] < 0 || agg[c] >= n) { set_error("%s: coarse aggregates: id %d of camera %ld is out of range [0, %ld)", plugin->name(), agg[c], c, n); return -1; }
        if (agg[c] + 1 > K_) K_ = agg[c] + 1;
    }
    std::vector<char> used((size_t)K_, 0);
    for (long c = 0; c < n; ++c) used[(size_t)agg[c]] = 1;
    for (int a = 0; a < K_; ++a) if (!used[(size_t)a]) { set_error("%s: coarse aggregates: the ids must be dense: aggregate %d of 0 .. %d has no camera", plugin->name(), a, K_ - 1); return -1; }
    if (9L * K_ > THALLO_HIP_COARSE_MAX_N) { set_error("%s: coarse aggregates: %d aggregates give n_c = %ld coarse scalars, more than the kernels take (%d)", plugin->name(), K_, 9L * K_, THALLO_HIP_COARSE_MAX_N); return -1; }
    coarse_k_ = 0; coarse_agg_.assign(agg, agg + n);
    return 0;
}

int Plan::coarse_space(long out[4])
{
    if (!ok_ || !ready_ || !coarse_on() || !out) return -1;
    unsigned w[3] = { 0, 0, 0 };
    if (hipMemcpyAsync(w, reduced()->coarse_words(), sizeof(w), hipMemcpyDeviceToHost, ctx.stream) != hipSuccess || hipStreamSynchronize(ctx.stream) != hipSuccess) return -1;
    out[0] = reduced()->coarse_aggregates(); out[1] = reduced()->coarse_n(); out[2] = (long)w[1]; out[3] = (long)w[2];
    return 0;
}

int Plan::block_prepare()
{   // the regions; H, G and the status word
    if (refuse_unless_one_gpu_pcg(plugin->block_precond_ok(), "the block-Jacobi preconditioner needs")) return -1;
    if (!plugin->apply_adds_ctc()) { set_error("%s: the block-Jacobi preconditioner needs a plugin whose applyJTJ adds the LM diagonal (apply_adds_ctc)", plugin->name()); return -1; }
    block_regions_ = plugin->block_regions();
    const long nf = thallo_hip_block_floats(block_regions_);
    if (nf < 0) { set_error("%s: invalid block regions", plugin->name()); return -1; }
    if (block_H_) return 0;
    block_H_ = (float*)device_alloc(((size_t)nf + 64) * sizeof(float)); block_G_ = (float*)device_alloc(((size_t)nf + 64) * sizeof(float)); block_status_ = (unsigned*)device_alloc(64);
    if (!block_H_ || !block_G_ || !block_status_) { block_H_ = block_G_ = nullptr; block_status_ = nullptr; set_error("%s: out of device memory for the block preconditioner", plugin->name()); return -1; }
    return 0;
}

int Plan::preconditioner_fallbacks() { return (block_on_ || schur_on_) && block_status_ ? read_word(block_status_) : -1; }

// ------------------------------------------------------------------ Schur complement on the cameras (ba_schur.hip, DESIGN.md "Schur complement on the cameras")
int Plan::set_linear_solver(int kind)
{
    if (kind != THALLOX_SOLVER_PCG && kind != THALLOX_SOLVER_SCHUR_PCG && kind != THALLOX_SOLVER_SCHUR_EXPLICIT_PCG && kind != THALLOX_SOLVER_SCHUR_DENSE) {
        set_error("%s: unknown linear solver kind %d", plugin->name(), kind); return -1;
    }
    if (kind == THALLOX_SOLVER_PCG) { schur_want_ = false; schur_explicit_want_ = false; schur_dense_want_ = false; return 0; }
    if (!ok_) return -1;
    const bool dense = kind == THALLOX_SOLVER_SCHUR_DENSE, ex = dense || kind == THALLOX_SOLVER_SCHUR_EXPLICIT_PCG;      // (kind 3 implies the structure of kind 2)
    const char* what = dense ? "dense Cholesky Schur-complement solve" : ex ? "assembled Schur-complement solve" : "Schur-complement solve";
    if (plugin->direct_solve()) {
        if (dense) set_error("%s: a direct-solve plan has no Schur complement to factor (it solves the full normal equations directly)", plugin->name());
        else set_error("%s: a direct-solve plan has no PCG loop to run on %s Schur complement", plugin->name(), ex ? "an assembled" : "a");
        return -1;
    }
    if (!reduced() || !plugin->block_precond_ok()) { set_error("%s: no %s for this energy (its plugin eliminates nothing; bundle_adjustment does)", plugin->name(), what); return -1; }
    if (dist_) { set_error("%s: the %s runs on one GPU (this plan is distributed)", plugin->name(), what); return -1; }
    schur_want_ = true; schur_explicit_want_ = ex; schur_dense_want_ = dense;
    return 0;
}

int Plan::schur_prepare()
{
    if (refuse_unless_one_gpu_pcg(reduced() != nullptr, "the Schur-complement solve needs")) return -1;
    if (block_prepare()) return -1;                      // H, G, the status word (G's camera region: the preconditioner of S)
    if (block_regions_.n != 2 || block_regions_.r[0].offset != 0) { set_error("%s: the Schur-complement solve needs two block regions, the kept one first", plugin->name()); return -1; }
    thallo_block_regions_t cameras = block_regions_; cameras.n = 1;
    schur_n_ = (long)block_regions_.r[0].size * block_regions_.r[0].count;
    schur_hp_off_ = thallo_hip_block_floats(cameras);
    schur_pt_off_ = block_regions_.r[1].offset;
    // the reduced system's forms: the structure of S with the dense triangle or the coarse matrices, sized and checked against its budget before it is allocated; behind
    // it the elimination factor and y, then g
    ReducedCameraSystem::Want want;
    want.assembled = schur_explicit_want_; want.dense = schur_dense_want_;
    want.two_level = coarse_want_ && schur_explicit_want_ && !schur_dense_want_;      // (the dense form ignores the preconditioner)
    want.cameras_per_aggregate = coarse_k_;
    want.aggregates = want.two_level && !coarse_agg_.empty() ? coarse_agg_.data() : nullptr;
    if (reduced()->configure(want)) return -1;
    if (schur_g_) return 0;
    if (!(schur_g_ = (float*)device_alloc(((size_t)v_.n_alloc + 64) * sizeof(float)))) { set_error("%s: out of device memory for the Schur-complement solve", plugin->name()); return -1; }
    return 0;
}

int Plan::schur_held_points() { return schur_on_ ? read_word(reduced()->held_word()) : -1; }

// ------------------------------------------------------------------ dense Cholesky of S (ba_schur_dense.hip, DESIGN.md "Dense Cholesky Schur solve")
int Plan::schur_dense_nonpositive() { return schur_dense() ? read_word(reduced()->dense_words() + 1) : -1; }

void Plan::schur_dense_pivot_error(int index, const char* where)
{
    set_error("%s: %sthe dense Cholesky factor of the reduced camera matrix met a pivot that is not positive at camera %d, scalar %d (index %d of %ld): the system is singular or "
              "indefinite in float32 -- fix the gauge with ThalloX_PlanSetHeldUnknowns (hold) or use Levenberg-Marquardt (ThalloX_EnableLM)", plugin->name(), where, index / 9, index % 9, index,
              reduced()->dense_n());
}

// One step's dense solve behind forms_setup: expand, factor, delta_c = D L^-T L^-1 D g into the camera part of delta.  The step's ONE extra read-back sits here, behind
// the solve's launch and in front of the back-substitution: a failed factor ends the step before anything is applied to the unknowns.  false: the error is set
bool Plan::schur_dense_step(const float* g)
{
    const int rc = reduced()->dense_solve(ctx, held_on() ? held_mask_ : nullptr, g, v_.delta);
    if (rc < 0) { set_error("%s: the dense Cholesky Schur-complement solve failed to launch (%d)", plugin->name(), rc); return false; }
    const int info = read_word(reduced()->dense_words());
    if (info < 0) { set_error("%s: cannot read the dense Cholesky factor's status word", plugin->name()); return false; }
    if (info > 0) { schur_dense_pivot_error(info - 1, ""); return false; }
    return true;
}

// ------------------------------------------------------------------ marginal covariances (ba_covariance.hip, DESIGN.md "Marginal covariances")
// Sigma = (A_FF)^-1 with A = J_s^T J_s (+ W where priors are in force) at the current unknowns, no CtC, on an LM plan too: the call re-linearises with the launches of a GN step's head -- PCGInit1
// (precomputeJ, `pre`) and forms_setup with shift = NULL: the mask, the block diagonal, both factors, W and the assembly -- and hands the step's S, both factors and the
// mask to the plugin's column solve.  Everything those launches write, every step rewrites before use (r, pre, z, p, delta, diag; H, G, the status words, y, g, W, S;
// slot 2); the LM state -- the radius and its decrease factor, SSq, CtC, b, the previous cost, prevX -- and the unknowns are not touched, no partial count is recorded, and
// the launches are kept out of the kernel statistics, which stay the steps'.
long Plan::covariance(void** params, int input, const int* ids, long n, float* host_out, const ThalloX_CovarianceOptions* opt, ThalloX_CovarianceInfo* info)
{
    if (!ok_) return -1;
    const char* e = plugin->name();
    if (plugin->direct_solve()) { set_error("%s: a direct-solve plan has no assembled Schur complement to take a covariance from", e); return -1; }
    if (!reduced()) { set_error("%s: no covariance for this energy (its plugin eliminates nothing and assembles no reduced matrix; bundle_adjustment does)", e); return -1; }
    if (dist_) { set_error("%s: the covariance runs on one GPU (this plan is distributed)", e); return -1; }
    if (!ready_) { set_error("%s: ThalloX_PlanCovariance before Thallo_ProblemInit: the covariance is taken at the unknowns of an initialised plan", e); return -1; }
    if (!schur_assembled()) {
        set_error("%s: the plan's last Init did not run the assembled Schur-complement solve: set ThalloX_PlanSetLinearSolver(plan, THALLOX_SOLVER_SCHUR_EXPLICIT_PCG) before Thallo_ProblemInit "
                  "(columns by PCG), or THALLOX_SOLVER_SCHUR_DENSE (columns through a dense Cholesky factor)", e);
        return -1;
    }
    const long elems = reduced()->elements(input);
    if (elems < 0) { set_error("%s: input %d is not an Unknown of this energy", e, input); return -1; }
    if (n <= 0 || !ids || !host_out) { set_error("%s: a covariance needs n > 0 ids and an output array (n = %ld)", e, n); return -1; }
    const float rel_tol = opt ? opt->rel_tol : 1e-6f;
    const int max_it = opt ? opt->max_iterations : 500;
    if (schur_dense()) {}      // (the dense form accepts and ignores both)
    else if (!(rel_tol > 0.0f) || !std::isfinite(rel_tol)) { set_error("%s: the covariance's rel_tol must be finite and positive (got %g)", e, (double)rel_tol); return -1; }
    if (!schur_dense() && max_it < 1) { set_error("%s: the covariance's max_iterations must be at least 1 (got %d)", e, max_it); return -1; }
    {   std::vector<char> seen((size_t)elems, 0);
        for (long i = 0; i < n; ++i) {
            if (ids[i] < 0 || ids[i] >= elems) { set_error("%s: covariance id %d (at %ld) is out of range: input %d has %ld elements", e, ids[i], i, input, elems); return -1; }
            if (seen[(size_t)ids[i]]++) { set_error("%s: covariance id %d is repeated (at %ld)", e, ids[i], i); return -1; }
        }
    }
    if (params && plugin->bind(params)) { set_error("%s: parameter binding failed", e); return -1; }
    if (!lm_) plugin->unknowns_changed();      // (as a GN step: everything is derived from the unknowns as they are now)
    struct NoStats { LaunchCtx& c; KernelTimer* t; NoStats(LaunchCtx& ctx) : c(ctx), t(ctx.timer) { c.timer = nullptr; } ~NoStats() { c.timer = t; } } no_stats(ctx);
    int nb = plugin->pcg_init(ctx, v_, 0, slot(2));
    if (nb < 0) { set_error("%s: covariance: PCGInit1 launch failed (%d)", e, nb); return -1; }
    if (prior_on() && (nb = prior_init(slot(2))) < 0) { set_error("%s: covariance: the prior's launch failed (%d)", e, nb); return -1; }      // (W is part of A: the shift is w, on an LM plan too)
    const char* what = nullptr;
    if ((nb = forms_setup(gn_shift(), v_.r, slot(2), nb, what)) < 0) { set_error("%s: covariance: %s failed (%d)", e, what, nb); return -1; }
    thallo_cov_info_t ci;
    if (schur_dense()) {      // expand and factor once per call, then every batch through two triangular sweeps: iterations 0, worst residual 0
        int pivot = -1;
        const int rc = reduced()->covariance_dense(ctx, input, ids, n, block_G_, held_on() ? held_mask_ : nullptr, host_out, &ci, &pivot);
        if (rc == -2) { schur_dense_pivot_error(pivot, "covariance: "); return -2; }
        if (rc) return -1;
    } else
    if (reduced()->covariance(ctx, input, ids, n, block_G_, held_on() ? held_mask_ : nullptr, rel_tol, max_it, host_out, &ci)) return -1;
    if (info) { info->iterations = ci.iterations; info->columns = ci.columns; info->not_converged = ci.not_converged; info->nan_blocks = ci.nan_blocks; info->worst_residual = ci.worst; }
    return ci.not_converged;
}

}  // namespace thallo
