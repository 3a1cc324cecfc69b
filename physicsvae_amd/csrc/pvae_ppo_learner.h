// pvae_ppo_learner.h -- the PPO learner's host driver, written once for the stack set (pvae_fc.hip) and PhysicsVAE
// (pvae_ppo.hip): what every pvae_fc_ppo_* / pvae_ppo_* entry point does between its model's checks and the launches of
// pvae_ppo_core.hip.  Function templates over a MODEL ADAPTER, a small struct each unit builds over its handle per call
// (on the stack; nothing here allocates), which answers only what differs between the two:
//   learner()                       the PpoLearner (pvae_internal.h); null: a null handle, which every check_* refuses
//                                   before anything here dereferences it
//   k(), n_in(), max_minibatch()    action and observation width, the largest minibatch and evaluate chunk
//   check_step(..), check_apply(..), check_eval(..)
//                                   the model's argument checks of a step, of its second half (the step's parts that do
//                                   not concern the batch) and of an evaluate pass: in its order, with its texts
//   grad_half(.., step, minibatch, dpart, st, &launches)
//                                   forward, loss head, backward into the bound gradient arena(s); `step`, `minibatch`:
//                                   where the step's own latent draws lie (PhysicsVAE)
//   segments(p, sg)                 what the Adam launch runs over
//   eval_rows(.., epi), eval_boot(..)   the rows through the model in chunks, epi(panels, first row, chunk index) launching
//                                   a chunk's epilogue; the value stack's bootstrap pass
//   peer_arenas(arg, arenas, floats), peer_timeout()
//                                   the gradient arena(s) the exchange maps (their number, or < 0: refused; `arg`: the
//                                   caller's blob pointer), and its timeout ticks
//   params_written(st), eps_out()   after a call that wrote parameters; where the epilogues copy the latent draws
// What needs no adapter is not here: *_ppo_diag, *_ppo_grad_clip, *_ppo_peer_close and *_ppo_peer_status call
// ppo_diag_bind, ppo_clip_bind and ppo_peer_* on the handle's PpoLearner directly.
#pragma once
#include "pvae_internal.h"

// one minibatch (arguments checked by the caller): the first half, then the Adam launch -- its exchanged form while a
// gradient exchange between workers is open (*_ppo_peer_open); `step`: the minibatch's number within the call, which
// is also its row of a bound diagnostics buffer
template <class M>
int learner_minibatch(M& m, const pvae_fc_ppo_batch* b, const int32_t* index, long long first, int rows,
                      const pvae_fc_ppo_params* p, int step, int minibatch, float* stats_out, hipStream_t st) {
    PpoLearner& q = *m.learner();
    int launches = 0;
    const PpoDiagRow dg = diag_row(q.diag, step);
    int rc = m.grad_half(b, index, first, rows, p, step, minibatch, dg.dpart, st, &launches);
    if (rc) return rc;
    PpoAdamSegs sg;
    if ((rc = m.segments(p, sg))) return rc;
    const int colsum = p->log_std_kind == 1;
    // a clip bound (*_ppo_grad_clip): this worker's sum of squares first, ONE launch more; the Adam launch forms coef from it
    if (q.clip.slot && (rc = ppo_clip_sumsq_launch(sg, p, rows, b->k, q.scratch, colsum, q.log_std, q.clip, st, &launches))) return rc;
    rc = q.peers.open ? ppo_adam_exchange_launch(q.peers, m.peer_timeout(), sg, p, p->adam_t + step, rows, b->k, q.scratch, colsum,
                                                 q.log_std, q.log_std_m, q.log_std_v, stats_out, dg, q.clip, st, &launches)
                      : ppo_adam_launch(sg, p, p->adam_t + step, rows, b->k, q.scratch, colsum, q.log_std, q.log_std_m,
                                        q.log_std_v, stats_out, dg, q.clip, st, &launches);
    if (rc) return rc;
    q.launches = launches;
    return 0;
}

template <class M>
int learner_step(M m, const pvae_fc_ppo_batch* b, const int32_t* index, long long first, int rows,
                 const pvae_fc_ppo_params* p, float* stats_out, hipStream_t st) {
    int rc = m.check_step(b, p, first, rows, stats_out);
    if (rc) return rc;
    if ((rc = learner_minibatch(m, b, index, first, rows, p, 0, rows, stats_out, st))) return rc;
    m.params_written(st);
    return 0;
}

// num_sgd_iter passes over the batch in minibatches: pass i takes its rows through perm[i] (null: in order), step j
// counts Adam's t on from p->adam_t and leaves its stats in stats_out[5 j ..]
template <class M>
int learner_sgd(M m, const pvae_fc_ppo_batch* b, const int32_t* perm, int minibatch, int num_sgd_iter,
                const pvae_fc_ppo_params* p, float* stats_out, hipStream_t st) {
    if (minibatch < 1 || num_sgd_iter < 1) return fail(-1, "minibatch and num_sgd_iter must be positive");
    int rc = m.check_step(b, p, 0, 1, stats_out);
    if (rc) return rc;
    if (minibatch > m.max_minibatch()) return fail(-1, "minibatch %d > max_batch %d", minibatch, m.max_minibatch());
    const PpoLearner& q = *m.learner();
    const long long steps = num_sgd_iter * ((b->n_rows + minibatch - 1) / minibatch);
    if (q.diag.out && steps > q.diag.capacity)
        return fail(-1, "%lld steps, the bound diagnostics buffer holds %d rows", steps, q.diag.capacity);
    int step = 0;
    for (int pass = 0; pass < num_sgd_iter; ++pass)
        for (long long first = 0; first < b->n_rows; first += minibatch, ++step) {
            const int rows = (int)(b->n_rows - first < minibatch ? b->n_rows - first : minibatch);
            rc = learner_minibatch(m, b, perm ? perm + (size_t)pass * b->n_rows : nullptr, first, rows, p, step, minibatch,
                                   stats_out + 5 * (size_t)step, st);
            if (rc) return rc;
        }
    m.params_written(st);
    return 0;
}

// The step in two halves (include/pvae.h "Gradient exchange between workers"): the first half with the finish launch in
// place of the Adam launch, and Adam alone on grad_scale * what the caller left in the gradient arena(s)
template <class M>
int learner_grad(M m, const pvae_fc_ppo_batch* b, const int32_t* index, long long first, int rows,
                 const pvae_fc_ppo_params* p, float* stats_out, float* ls_grad, hipStream_t st) {
    int rc = m.check_step(b, p, first, rows, stats_out);
    if (rc) return rc;
    const int colsum = p->log_std_kind == 1;
    if (colsum && !ls_grad) return fail(-1, "ls_grad is null (log_std_kind 1)");
    PpoLearner& q = *m.learner();
    int launches = 0;
    const PpoDiagRow dg = diag_row(q.diag, 0);
    if ((rc = m.grad_half(b, index, first, rows, p, 0, rows, dg.dpart, st, &launches))) return rc;
    PpoAdamSegs sg;
    if (q.clip.slot) {
        if ((rc = m.segments(p, sg))) return rc;
        if ((rc = ppo_clip_sumsq_launch(sg, p, rows, b->k, q.scratch, colsum, q.log_std, q.clip, st, &launches))) return rc;
    }
    if ((rc = ppo_grad_finish_launch(rows, b->k, q.scratch, colsum, ls_grad, stats_out, dg, st, &launches))) return rc;
    // a clip bound: the gradient left behind is the clipped one (and *_ppo_apply does not clip again)
    if (q.clip.slot && (rc = ppo_clip_scale_launch(sg, p, b->k, ls_grad, colsum, q.clip, dg, st, &launches))) return rc;
    q.launches = launches;
    return 0;
}

template <class M>
int learner_apply(M m, const pvae_fc_ppo_params* p, float grad_scale, const float* ls_grad, hipStream_t st) {
    int rc = m.check_apply(p, ls_grad);
    if (rc) return rc;
    PpoLearner& q = *m.learner();
    PpoAdamSegs sg;
    if ((rc = m.segments(p, sg))) return rc;
    int launches = 0;
    if ((rc = ppo_apply_launch(sg, p, p->adam_t, m.k(), grad_scale, ls_grad, p->log_std_kind == 1, q.log_std, q.log_std_m,
                               q.log_std_v, diag_row(q.diag, 0), st, &launches)))
        return rc;
    q.launches = launches;
    m.params_written(st);
    return 0;
}

// ---- gradient exchange between workers ----
template <class M>
int learner_peer_export(M m, void* blob) {
    float* arenas[kPpoPeerArenas];
    long long floats[kPpoPeerArenas];
    const int n = m.peer_arenas(blob, arenas, floats);
    return n < 0 ? n : ppo_peer_export(m.learner()->peers, arenas, floats, n, m.k(), blob);
}

template <class M>
int learner_peer_open(M m, int rank, int world, const void* blobs) {
    float* arenas[kPpoPeerArenas];
    long long floats[kPpoPeerArenas];
    const int n = m.peer_arenas(blobs, arenas, floats);
    return n < 0 ? n : ppo_peer_open(m.learner()->peers, arenas, rank, world, blobs, m.peer_timeout());
}

// ---- launch counters (`q` null: a null handle) ----
inline int learner_launches(const PpoLearner* q, int32_t* per_step) {
    if (!q || !per_step) return fail(-1, "null argument");
    *per_step = q->launches;
    return 0;
}
inline int learner_gae_launches(const PpoLearner& q, int32_t* evaluate, int32_t* rest) {
    if (evaluate) *evaluate = q.eval_launches;
    if (rest) *rest = q.gae_launches;
    return 0;
}

// ---- train-batch preparation and action sampling: evaluate, prepare and act zero both counters on entry (a refused call
// reports that it launched nothing) ----
// the rows pass with the evaluate epilogue: vf_preds, old_dist and old_logp of the rollout's own actions
template <class M>
int learner_eval_rows(M& m, const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out, hipStream_t st,
                      int& launches) {
    const int k = ro->k;
    return m.eval_rows(ro->obs, ro->n_rows, k, p, st, launches, [&](const PpoPanels& pan, long long first, uint64_t) {
        PpoEval e;
        memset(&e, 0, sizeof(e));
        static_cast<PpoPanels&>(e) = pan;
        e.actions = ro->actions + (size_t)first * k;
        e.vf = out->vf_preds + first; e.dist = out->old_dist + (size_t)first * 2 * k; e.logp = out->old_logp + first;
        if (float* eps_out = m.eps_out()) e.eps_dst = eps_out + (size_t)first * pan.Z;
        return ppo_eval_launch(e, st);
    });
}

template <class M>
int learner_evaluate(M m, const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out, hipStream_t st) {
    const bool rows_pass = out && out->vf_preds, boot = out && out->last_value;
    if (PpoLearner* q = m.learner()) q->eval_launches = q->gae_launches = 0;
    int rc = m.check_eval(ro, p, out, rows_pass);
    if (rc) return rc;
    if (!rows_pass && !boot) return fail(-1, "neither vf_preds nor last_value: nothing to compute");
    if (boot && (rc = check_boot(ro, out))) return rc;
    int ev = 0, rest = 0;
    if (rows_pass && (rc = learner_eval_rows(m, ro, p, out, st, ev))) return rc;
    if (boot && (rc = m.eval_boot(ro, out, st, rest))) return rc;
    m.learner()->eval_launches = ev; m.learner()->gae_launches = rest;
    return 0;
}

template <class M>
int learner_prepare(M m, const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out, void* scratch,
                    size_t scratch_bytes, hipStream_t st) {
    if (PpoLearner* q = m.learner()) q->eval_launches = q->gae_launches = 0;
    int given = 0;
    int rc = check_prepare(ro, p, out, scratch, scratch_bytes, &given,
                           [&](bool rows_pass) { return m.check_eval(ro, p, out, rows_pass); });
    if (rc) return rc;
    int ev = 0, rest = 0;
    if (given == 0 && (rc = learner_eval_rows(m, ro, p, out, st, ev))) return rc;
    if ((rc = m.eval_boot(ro, out, st, rest))) return rc;
    // (last_value already holds the zeros of the done segments)
    if ((rc = run_gae(ro->rewards, given ? ro->vf_preds : out->vf_preds, out->last_value, nullptr, ro->seg_start, ro->n_rows,
                      ro->n_segs, p, out->advantages, out->value_targets, scratch, st, rest)))
        return rc;
    m.learner()->eval_launches = ev; m.learner()->gae_launches = rest;
    return 0;
}

template <class M>
int learner_act(M m, const pvae_ppo_act_in* in, const pvae_gae_params* p, const pvae_ppo_act_out* out, hipStream_t st) {
    if (PpoLearner* q = m.learner()) q->eval_launches = q->gae_launches = 0;
    if (!in || !p || !out) return fail(-1, "null in, params or out");
    // the model's side of the checks is evaluate's: the same rows, the action column the one written here
    pvae_fc_rollout ro;
    pvae_fc_prepared ev;
    act_as_evaluate(in, out, ro, ev);
    int rc = m.check_eval(&ro, p, &ev, true);
    if (rc) return rc;
    if ((rc = check_act(in, out))) return rc;
    int launches = 0;
    rc = m.eval_rows(in->obs, in->n_rows, in->k, p, st, launches, [&](const PpoPanels& pan, long long first, uint64_t i) {
        PpoAct a;
        fill_act(a, pan, in, out, first, i, m.n_in());
        a.eps_dst = m.eps_out();
        return ppo_act_launch(a, st);
    });
    if (rc) return rc;
    m.learner()->eval_launches = launches;
    return 0;
}
