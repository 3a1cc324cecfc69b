// pvae_lookahead.hip -- the training step at lookahead > 1: the multi-step unroll of tpv:367-428, forward and backward plan.
#include "pvae_internal.h"

// s1 of step t+1 = world-model prediction of step t (tpv:421): copy the first Db columns of the
// valid rows of `src` into the current-state columns of up to four input panels.
__global__ void __launch_bounds__(256)
scatter_state_kernel(const float* __restrict__ src, int lds_, int rows, int Db, float* __restrict__ d0, int ld0,
                     float* __restrict__ d1, int ld1, float* __restrict__ d2, int ld2, float* __restrict__ d3,
                     int ld3) {
    const int total = rows * Db;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / Db, c = idx - r * Db;
        const float v = src[(size_t)r * lds_ + c];
        if (d0) d0[(size_t)r * ld0 + c] = v;
        if (d1) d1[(size_t)r * ld1 + c] = v;
        if (d2) d2[(size_t)r * ld2 + c] = v;
        if (d3) d3[(size_t)r * ld3 + c] = v;
    }
}

// ---------------------------------------------------------------------------------------
// lookahead > 1: the multi-step unroll of tpv:367-428
// ---------------------------------------------------------------------------------------
// Per step t: x_t = [s1_t | s2gt_t] -> encoder -> sampler -> decoder -> world model with the
// decoder's action (its output is both the cycle-loss prediction and s1_{t+1}, tpv:417-421) and,
// when world_model_s_rec_coeff > 0, the world model with the demonstrated action (tpv:411-414).
// All of it runs in BOTH phases (the world phase needs the chain because s1_{t+1} is a
// prediction), in row block t of every panel; the world model uses block t for the
// demonstrated-action invocation and block L+t for the predicted-action one.
struct Unroll {
    int T, rows, rows_pad;
    bool use_g;                        // demonstrated-action world-model invocations exist
    int64_t blk(int slot) const { return (int64_t)slot * rows_pad; }
};

static Unroll make_unroll(const pvae_ctx* c, int phase, int rows, const pvae_step_params* sp) {
    Unroll u;
    u.T = c->W.L; u.rows = rows; u.rows_pad = pad32(rows);
    u.use_g = sp->s_rec_coeff > 0.0f;      // (both phases: tpv:411-414 does not ask which one)
    return u;
}

int run_forward_unrolled(pvae_ctx* c, int phase, int rows, const pvae_step_params* sp, const float* eps,
                                bool backward, const StepShape& S, hipStream_t st) {
    int rc;
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action, Z = c->L.cfg.latent;
    const Unroll u = make_unroll(c, phase, rows, sp);
    float* w = c->ws;
    float* part = w + c->W.loss_part;
    const NetLayout& TE = c->L.net[PVAE_NET_TE];
    const NetLayout& MD = c->L.net[PVAE_NET_MD];
    const NetLayout& WM = c->L.net[PVAE_NET_WM];
    const NetWork& wte = c->W.net[PVAE_NET_TE];
    const NetWork& wmd = c->W.net[PVAE_NET_MD];
    const NetWork& wwm = c->W.net[PVAE_NET_WM];
    const int ld_te = TE.layers[0].ld, ld_md = MD.layers[0].ld, ld_wm = WM.layers[0].ld;
    const int ldo_te = TE.layers.back().n_out_pad, ldo_wm = WM.layers.back().n_out_pad;
    const bool joint = phase == PVAE_PHASE_JOINT;
    for (int t = 0; t < u.T; ++t) {
        const int64_t bt = u.blk(t), bp = u.blk(u.T + t);
        if ((rc = forward_net(c, PVAE_NET_TE, u.rows_pad, st, FwdTail(), bt))) return rc;
        if ((rc = launch_sampler(c, w + wte.act.back() + bt * ldo_te, ldo_te, eps ? eps + (size_t)t * rows * Z : (const float*)nullptr,
                                 w + c->W.eps + bt * Z, w + wmd.in + bt * ld_md, ld_md, rows, u.rows_pad, 1,
                                 (unsigned long long)sp->rng_seed, (unsigned long long)(sp->rng_offset + t),
                                 part + 2 * kLossParts + t * S.gridz, (float*)nullptr, (const float*)nullptr, 0, st)))
            return rc;
        FwdTail md_tail;                       // a_hat -> action columns of the predicted-action WM input
        md_tail.out2 = w + wwm.in + bp * ld_wm; md_tail.ld2 = ld_wm; md_tail.off2 = Db; md_tail.n2 = Da;
        if ((rc = forward_net(c, PVAE_NET_MD, u.rows_pad, st, md_tail, bt))) return rc;
        if (!c->L.net[PVAE_NET_MH].layers.empty()) {        // rmt:833-835 in every unrolled step: a_hat_t += range * helper(x_t)
            if ((rc = forward_net(c, PVAE_NET_MH, u.rows_pad, st, FwdTail(), bt))) return rc;
            if ((rc = helper_add_launch(c, rows, bt, bp, st))) return rc;
        }
        EpiMse mse;
        memset(&mse, 0, sizeof(mse));
        mse.target = w + c->W.s2 + bt * pad64(Db); mse.ldt = pad64(Db);
        mse.ldz = ldo_wm; mse.rows = rows; mse.D = Db; mse.l1 = S.l1;
        FwdTail wm_tail;
        wm_tail.mse = &mse;
        // predicted action: cycle loss (tpv:417-419) + the state of the next step
        mse.dz = backward ? w + wwm.dz.back() + bp * ldo_wm : nullptr;
        mse.grad_scale = joint ? sp->cycle_coeff * S.gs / (S.Bg * Db) : 0.0f;
        mse.partial = part + 4 * kLossParts + t * S.wm_tiles;
        if ((rc = forward_net(c, PVAE_NET_WM, u.rows_pad, st, wm_tail, bp))) return rc;
        if (u.use_g) {                         // demonstrated action: state reconstruction (tpv:411-414)
            // (joint phase, step 0: s1 and a_gt are data and the world model is frozen -- a loss term, no gradient)
            mse.dz = backward && (!joint || t > 0) ? w + wwm.dz.back() + bt * ldo_wm : nullptr;
            mse.grad_scale = sp->s_rec_coeff * S.gs / (S.Bg * Db);
            mse.partial = part + 3 * kLossParts + t * S.wm_tiles;
            if ((rc = forward_net(c, PVAE_NET_WM, u.rows_pad, st, wm_tail, bt))) return rc;
        }
        if (t + 1 < u.T) {                     // s1 of the next step (tpv:421)
            const int64_t nt = u.blk(t + 1), np = u.blk(u.T + t + 1);
            hipLaunchKernelGGL(scatter_state_kernel, dim3(grid1d(rows * Db, 256)), dim3(256), 0, st,
                               w + wwm.act.back() + bp * ldo_wm, ldo_wm, rows, Db,
                               // (input subsets: a stack that does not read s_t keeps zeros there)
                               c->L.cfg.te_inputs == PVAE_INPUT_TASK ? (float*)nullptr : w + wte.in + nt * ld_te, ld_te,
                               c->L.cfg.md_inputs == PVAE_INPUT_TASK ? (float*)nullptr : w + wmd.in + nt * ld_md, ld_md,
                               w + wwm.in + np * ld_wm, ld_wm,
                               u.use_g ? w + wwm.in + nt * ld_wm : (float*)nullptr, ld_wm);
            HIP_TRY(hipGetLastError());
        }
    }
    return 0;
}

// Backward through the unroll, last step first.  Input gradients are needed in full here (the
// current-state columns of every consumer feed the previous step), weight gradients contract over
// ALL steps at once: the time-step blocks are stacked along the row axis, so one launch per layer
// with K = blocks * rows_pad yields sum_t X_t^T dZ_t (and Adam runs once, in its epilogue).
void plan_backward_unrolled(pvae_ctx* c, int phase, int rows, const pvae_step_params* sp, bool backward,
                                   bool fused, const StepShape& S, hipStream_t st, Plan& plan) {
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action, Z = c->L.cfg.latent;
    const Unroll u = make_unroll(c, phase, rows, sp);
    const int T = u.T;
    float* w = c->ws;
    const bool joint = phase == PVAE_PHASE_JOINT;
    const NetLayout* NL = c->L.net;
    const NetWork* NW = c->W.net;
    std::vector<BwdNet> nets;                  // every stack's backward view; a launch names its row block (u.blk(slot))
    for (int n = 0; n < PVAE_NUM_NETS; ++n) nets.emplace_back(c, n, sp, st);
    // which invocations carry gradient (evaluated last step first)
    const bool a_grad = joint && sp->a_rec_coeff > 0.0f;
    std::vector<char> p_act(T, 0), md_act(T, 0), any(T + 1, 0);
    for (int t = T - 1; t >= 0; --t) {
        p_act[t] = S.cyc_grad || (t + 1 < T && any[t + 1]);
        md_act[t] = a_grad || p_act[t];
        any[t] = md_act[t] || p_act[t] || u.use_g;
    }
    // full dgrad chain of net n over row block `slot`; layer 0 only when its input gradient is consumed
    auto dgrad_chain = [&](int n, int slot, bool layer0) {
        const BwdNet bn = nets[n];
        const int64_t b = u.blk(slot);
        const int rows_pad = u.rows_pad;
        for (int i = bn.last(); i >= (layer0 ? 0 : 1); --i) push(plan, [=] { return bn.dgrad(i, b, rows_pad); });
    };
    const int ld_te = NL[PVAE_NET_TE].layers[0].ld, ld_md = NL[PVAE_NET_MD].layers[0].ld;
    const int ld_wm = NL[PVAE_NET_WM].layers[0].ld;
    const int ldo_wm = NL[PVAE_NET_WM].layers.back().n_out_pad;
    const NetWork* wte = &NW[PVAE_NET_TE];
    const NetWork* wmd = &NW[PVAE_NET_MD];
    const NetWork* wwm = &NW[PVAE_NET_WM];

    // Weight gradients contract over ALL steps at once (row blocks stacked): rows [0, krows) of a trainable stack.
    // Row blocks that receive no gradient are cut off the end or zero-filled; the fills go first (nothing writes
    // those blocks afterwards).
    // The motor decoder's helper (rmt:670-680, 833-835) sits in every step's a_hat_t.  Nothing in the trainer freezes it
    // (tpv:326-329, 347-350), and with lookahead > 1 the WORLD phase reaches it as well: the state the world model continues
    // from is its own prediction under the helped action (tpv:417-421).  So it is a trainable stack of both phases here
    // (adam_t[PVAE_NET_MH] == 0: frozen for this step), and the world phase's step 0 -- whose frozen decoder and encoder
    // lead nowhere -- still has to bring the action's gradient to it.
    const bool helper = !NL[PVAE_NET_MH].layers.empty();
    const bool mh_train = helper && sp->adam_t[PVAE_NET_MH] > 0;
    const NetWork* wmh = &NW[PVAE_NET_MH];
    std::vector<int> train_nets;
    if (mh_train) train_nets.push_back(PVAE_NET_MH);
    if (joint) { train_nets.push_back(PVAE_NET_MD); train_nets.push_back(PVAE_NET_TE); }
    else train_nets.push_back(PVAE_NET_WM);
    int krows_of[PVAE_NUM_NETS] = {};
    if (backward) {
        for (int n : train_nets) {
            const NetLayout* N = &NL[n];
            const NetWork* nw = &NW[n];
            std::vector<char> act;
            if (n == PVAE_NET_WM) {
                for (int t = 0; t < T; ++t) act.push_back(u.use_g);
                for (int t = 0; t < T; ++t) act.push_back(p_act[t]);
            } else {                               // (decoder, encoder, helper: one block per step that the action's gradient reaches)
                for (int t = 0; t < T; ++t) act.push_back(md_act[t]);
            }
            int blocks = (int)act.size();
            while (blocks > 0 && !act[blocks - 1]) --blocks;
            for (int b = 0; b < blocks; ++b) {
                if (act[b]) continue;
                const int64_t r0 = u.blk(b);
                const size_t nrows = (size_t)u.rows_pad;
                push(plan, [=]() -> int {
                    for (const Layer& l : N->layers)
                        HIP_TRY(hipMemsetAsync(w + nw->dz[l.index] + r0 * l.n_out_pad, 0, nrows * l.n_out_pad * sizeof(float), st));
                    return 0;
                });
            }
            krows_of[n] = blocks * u.rows_pad;
        }
    }
    const LossFinal* fold = S.lf.out ? &S.lf : nullptr;
    // Step 0's input-gradient launches of a trainable stack run LAST in the backward pass, so by the time layer i's
    // input gradient of step 0 is launched, dz[i] is final for every step: its weight gradient (over all steps) can
    // share that launch -- the same-layer pairing of the lookahead-1 schedule (gradient stored, Adam deferred to
    // workgroups of the next launch), instead of 3 weight-gradient launches per stack at the end (PVAE_LOOK_PAIR=0).
    const bool look_pair = backward && g_look_pair && c->pair_launch && c->same_layer_pairs && (!fused || can_defer_adam(c, fused));
    bool paired_done[PVAE_NUM_NETS] = {};
    // layers last .. lo of stack n: dgrad_i over row block `slot` || wgrad_i over rows [0, krows); then, when lo == 1,
    // layer 0's weight gradient on its own.  `with_fold`: the stack's last launch also finalises the losses.
    auto paired_chain = [&](int n, int slot, int lo, bool with_fold) {
        const BwdNet bn = nets[n];
        const int64_t b = u.blk(slot);
        const int rows_pad = u.rows_pad, krows = krows_of[n];
        LossFinal foldv;
        memset(&foldv, 0, sizeof(foldv));
        if (with_fold && fold) foldv = *fold;
        for (int i = bn.last(); i >= 0; --i) {
            const bool has_d = i >= lo;
            const bool f = with_fold && fold && i == 0;
            bn.ready(push(plan, [=]() -> int {
                const Layer& l = bn.layer(i);
                const double fl = 2.0 * bn.rowsf * l.n_in * l.n_out;
                const AdamPair ad = take_pending(c);               // (every launch takes all that is pending: no narrow rule here)
                hipError_t he;
                if (has_d) {
                    EpiGradStore es = bn.store_epi(i);
                    if (f) es.loss = foldv;
                    const int pp = g_prof.begin(3, fl * (1.0 + (double)krows / rows_pad), st);
                    he = bn.wgrad_with_dgrad(i, krows, bn.dgrad_args(i, b, rows_pad), es, ad);
                    g_prof.end(pp, st);
                    // (this launch read W_i: its update waits for the next one)
                    if (he == hipSuccess && fused) c->pending_adam = bn.adam_seg(i);
                } else {
                    const int pw = g_prof.begin(2, fl * ((double)krows / rows_pad), st);
                    he = bn.with_grad_epi<false>(i, fused, [&](auto e) -> hipError_t {
                        if (f) e.loss = foldv;
                        return bn.wgrad(i, krows, e, &ad);
                    });
                    g_prof.end(pw, st);
                }
                if (he != hipSuccess) return fail(-10, "paired backward launch: %s", hipGetErrorString(he));
                return 0;
            }), i, i);
        }
        paired_done[n] = true;
    };
    for (int t = T - 1; t >= 0; --t) {
        const int64_t bt = u.blk(t), bp = u.blk(T + t);
        // step 0 in the WORLD phase: what flows back through the (frozen) decoder and encoder of step 0 reaches no
        // trainable parameter -- only the world model's own layers above layer 0 need their input gradients
        const bool upstream = joint || t > 0;
        const bool up_a = upstream || mh_train;   // the action's gradient of this step is wanted (by the helper, if by nobody else)
        const bool pair_wm = look_pair && t == 0 && !joint && krows_of[PVAE_NET_WM] > 0;
        // joint phase: the world model is frozen (tpv:347-350), so its demonstrated-action invocation is a dgrad-only chain
        // whose one product is the state columns of d(wm_in) -- the gradient wrt s1_t, a prediction for t >= 1; step 0 has
        // none to give (pair_wm is false there: no weight gradient, no Adam for the world model)
        if (backward && u.use_g && (!joint || t > 0)) {
            if (pair_wm && !p_act[t]) paired_chain(PVAE_NET_WM, t, 1, true);    // (no predicted-action chain follows)
            else dgrad_chain(PVAE_NET_WM, t, t > 0);
        }
        if (backward && p_act[t]) {
            if (t + 1 < T && any[t + 1]) {        // + gradient wrt s1_{t+1}, from every consumer of it
                const int64_t nt = u.blk(t + 1), np = u.blk(T + t + 1);
                const float* s_te = md_act[t + 1] ? w + wte->d_in + nt * ld_te : nullptr;
                const float* s_md = md_act[t + 1] ? w + wmd->d_in + nt * ld_md : nullptr;
                const float* s_p = p_act[t + 1] ? w + wwm->d_in + np * ld_wm : nullptr;
                const float* s_g = u.use_g ? w + wwm->d_in + nt * ld_wm : nullptr;
                push(plan, [=] {
                    return add_cols_launch(w + wwm->dz.back() + bp * ldo_wm, ldo_wm, rows, Db, s_te, ld_te, s_md, ld_md, s_p, ld_wm,
                                           s_g, ld_wm, st);
                });
            }
            if (pair_wm) paired_chain(PVAE_NET_WM, T + t, up_a ? 0 : 1, true);
            else dgrad_chain(PVAE_NET_WM, T + t, up_a);
        }
        if (!up_a) continue;
        // action reconstruction (tpv:381-382) + gradient arriving through the world model
        if (md_act[t] || (joint && sp->a_rec_coeff > 0.0f)) {
            const float ga = joint ? sp->a_rec_coeff * S.gs / (S.Bg * Da) : 0.0f;
            const int nparts = S.nparts_a, l1 = S.l1;
            const bool extra = p_act[t] && backward;
            push(plan, [=] { return action_loss_launch(c, rows, t, bt, bp, nparts, ga, l1, backward, extra, st); });
        }
        if (!backward || !md_act[t]) continue;
        if (helper) {
            // d a_hat_t (just formed) -> the helper's output layer through range * tanh', then its own layers; its input
            // gradient matters where the decoder's does (z -> encoder, s1_t -> the previous step)
            push(plan, [=] { return helper_seed_launch(c, rows, bt, st); });
            dgrad_chain(PVAE_NET_MH, t, upstream);
        }
        if (!upstream) continue;
        const bool pair_here = look_pair && t == 0 && joint;
        if (pair_here && krows_of[PVAE_NET_MD] > 0) paired_chain(PVAE_NET_MD, t, 0, false);
        else dgrad_chain(PVAE_NET_MD, t, true);
        if (helper) {                              // x_t = [s1_t | z_t] feeds the helper too: its input gradient joins the decoder's
            const int ld_mh = NL[PVAE_NET_MH].layers[0].ld;
            push(plan, [=] {
                return add_cols_launch(w + wmd->d_in + bt * ld_md, ld_md, rows, Db + Z, w + wmh->d_in + bt * ld_mh, ld_mh, nullptr, 0,
                                       nullptr, 0, nullptr, 0, st);
            });
        }
        const float kls = S.kl_active ? sp->kl_coeff / S.Bg : 0.0f;
        push(plan, [=] { return reparam_bwd_launch(c, rows, bt, kls, st); });
        if (pair_here && krows_of[PVAE_NET_TE] > 0) paired_chain(PVAE_NET_TE, t, 1, true);
        else dgrad_chain(PVAE_NET_TE, t, t > 0);
    }
    if (!backward) return;

    // weight gradients of the stacks whose launches were not paired above: one contraction per layer over the
    // stacked blocks
    for (size_t k = 0; k < train_nets.size(); ++k) {
        const int n = train_nets[k];
        if (paired_done[n]) continue;
        const BwdNet bn = nets[n];
        const int blocks = krows_of[n] / u.rows_pad;
        const int krows = krows_of[n];
        const bool last_net = k + 1 == train_nets.size();
        // two layers per launch (wgrad_pair_kernel), last layer first; an odd layer count leaves layer 0
        // on its own.  The launch that contains layer 0 of the last net also finalises the losses.
        const bool pairs = c->pair_launch && krows > 0;
        for (int i = bn.last(); i >= 0;) {
            const int j = (pairs && i >= 1) ? i - 1 : -1;             // second layer of this launch
            const int lo = j >= 0 ? j : i;
            const bool with_fold = fold && last_net && lo == 0;
            LossFinal foldv;
            memset(&foldv, 0, sizeof(foldv));
            if (with_fold) foldv = *fold;
            bn.ready(push(plan, [=]() -> int {
                const Layer& l = bn.layer(i);
                double fl = 2.0 * bn.rowsf * blocks * l.n_in * l.n_out;
                if (j >= 0) fl += 2.0 * bn.rowsf * blocks * bn.layer(j).n_in * bn.layer(j).n_out;
                const int pw = g_prof.begin(2, fl, st);
                int rc2 = 0;
                if (krows > 0) {                   // (0: nothing reached this net, its gradient stays as it is)
                    // (Adam in the epilogues: these launches take no pending segment)
                    const hipError_t he = bn.with_grad_epi<false>(i, fused, [&](auto e1) -> hipError_t {
                        if (with_fold) e1.loss = foldv;                   // block 0 of the launch runs e1's problem
                        if (j < 0) return bn.wgrad(i, krows, e1, nullptr);
                        const Layer& l2 = bn.layer(j);
                        return gemm_wgrad_pair(bn.dz(i), l.n_out_pad, bn.x(i), l.ld, l.n_out_pad, l.ld, e1, bn.dz(j), l2.n_out_pad,
                                               bn.x(j), l2.ld, l2.n_out_pad, l2.ld, bn.like(e1, j), krows, st);
                    });
                    if (he != hipSuccess) rc2 = fail(-10, "weight-gradient launch: %s", hipGetErrorString(he));
                }
                g_prof.end(pw, st);
                return rc2;
            }), lo, i);
            i = lo - 1;
        }
    }
}
