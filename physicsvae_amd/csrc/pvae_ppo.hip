// pvae_ppo.hip -- the PPO learner step of PhysicsVAE (include/pvae.h pvae_ppo_*; `run: DDPPO`, `custom_model: physics_vae`):
// one minibatch update -- rmt:742-771 without the world model, the clipped-surrogate loss, backward, Adam -- as ONE
// library call with no host synchronisation.  It joins launches that exist: the stacks' forward and backward plans of
// pvae_net.hip (through pvae_infer.hip's hooks), the stack set's grouped launches (the value branch, pvae_fc.hip) and the learner's model-independent launches
// (loss head, Adam + stats, evaluate epilogue, GAE: pvae_ppo_core.hip).  What is PhysicsVAE's own stays here: the copy-in
// into three input panels, the sampler's backward, and the order of the launches.  No forward is
// recomputed: the encoder's, the decoder's and the value stack's panels stay live from the forward to their backward
// (the three stacks share no panel).  Launch order of a step:
//   copy-in | [rows <= 4: zero pad rows] | TE layers | sampler | MD layers | value layers | loss head |
//   MD backward (input gradient when the encoder is trained) | sampler backward | TE backward | value backward | Adam + stats
// and its first half, train-batch preparation (pvae_ppo_evaluate / pvae_ppo_prepare): the step's forward launches in chunks of
// max_batch rows with the evaluate epilogue in place of the loss head, then the value stack's bootstrap pass and the GAE and
// standardise launches.  Launch order of a chunk:
//   copy-in | TE layers | sampler | MD layers | value layers | epilogue
// The sequence of a call -- sgd loop, Adam launch, evaluate / prepare / act -- is the host driver's (pvae_ppo_learner.h);
// this unit gives it VaeLearner, the model adapter: PhysicsVAE's checks, first half, Adam segments and chunked rows pass.
#include "pvae_internal.h"
#include "pvae_ppo_learner.h"

namespace {

// obs[index[r]] = [s_body (Db) | s_task (Db)] into the three input panels, each written over its WHOLE [rows_pad][ld]
// block: zeros in pad rows, in pad columns and in the blocks an input subset leaves out (StageArgs::in_off).  The decoder's
// z columns are written by the sampler.  blockIdx.y = panel: 0 encoder, 1 decoder, 2 value stack.
struct PpoCopyIn {
    const float* obs; const int32_t* index; long long row0, n_rows;
    int rows, rows_pad, Db, in_off;
    float* dst[3]; int ld[3];
};
__global__ void __launch_bounds__(256)
ppo_copy_in_kernel(PpoCopyIn a) {
    const int k = blockIdx.y;
    float* __restrict__ dst = a.dst[k];
    const int ld = a.ld[k], Db = a.Db;
    const int total = a.rows_pad * ld;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / ld, c = idx - r * ld;
        bool on = r < a.rows;
        if (k == 0) on = on && c < 2 * Db && !(a.in_off & (c < Db ? 1 : 2));
        else if (k == 1) on = on && c < Db && !(a.in_off & 4);
        else on = on && c < 2 * Db;
        dst[idx] = on ? a.obs[(size_t)batch_row(a.index, a.row0, a.n_rows, r) * (2 * Db) + c] : 0.f;
    }
}

// Backward of the sampler on the panels (sampler_bwd_kernel's arithmetic, pvae_infer.hip; autograd of rmt:734-740, no KL term:
// the PPO loss has none): dz = the z columns of the decoder's input gradient, mu_logvar = the encoder's output panel,
// d_mu_logvar -> the encoder's output gradient panel, written over its whole [rows_pad][ld] block (zeros in pad rows / columns).
//   N(mu, s^2):  dmu = dz, dlv = dz eps exp(lv / 2) / 2 (noise = 0: z = mu, dlv = 0);   no prior (False): de = dz
__global__ void __launch_bounds__(256)
ppo_sampler_bwd_kernel(const float* __restrict__ te_out, const float* __restrict__ eps_used, const float* __restrict__ d_md_in,
                       int ld_md, int Db, int Z, int rows, int rows_pad, int with_logvar, int noise, float* __restrict__ dz_te, int ld) {
    const int total = rows_pad * ld;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / ld, c = idx - r * ld;
        float d = 0.f;
        if (r < rows) {
            if (c < Z) d = d_md_in[(size_t)r * ld_md + Db + c];
            else if (with_logvar && noise && c < 2 * Z) {
                const int j = c - Z;
                d = d_md_in[(size_t)r * ld_md + Db + j] * eps_used[(size_t)r * Z + j] * 0.5f * expf(0.5f * te_out[idx]);
            }
        }
        dz_te[idx] = d;
    }
}

// The same under the sphere prior (PVAE_PRIOR_HYPERSPHERE; forward: sphere_kernel, z = e / max(|e|, 1e-12)), which needs a
// reduction over the row: one wavefront per row, four rows per workgroup, grid rows_pad / 4, the row's arithmetic that of
// the autograd path (sphere_bwd_row, pvae_internal.h).  e = the encoder's output panel, g = the z columns of the decoder's
// input gradient; de -> the encoder's output gradient panel, again over its WHOLE [rows_pad][ld] block: zeros in the pad
// columns [Z, ld) and in the pad rows.  No atomics, one summation order: the same bits every run.
__global__ void __launch_bounds__(256)
ppo_sphere_bwd_kernel(const float* __restrict__ te_out, const float* __restrict__ d_md_in, int ld_md, int Db, int Z, int rows,
                      int rows_pad, float* __restrict__ dz_te, int ld) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows_pad) return;
    float* d = dz_te + (size_t)r * ld;
    if (r >= rows) {
        for (int c = lane; c < ld; c += 64) d[c] = 0.f;
        return;
    }
    sphere_bwd_row(te_out + (size_t)r * ld, d_md_in + (size_t)r * ld_md + Db, Z, lane, d);
    for (int c = Z + lane; c < ld; c += 64) d[c] = 0.f;
}

enum { kTrainTE = 1, kTrainMD = 2, kTrainValue = 4 };

// the copy-in launch: rows `index[r]` (index NULL: row0 + r) of obs [n_rows][2 Db] into the three input panels
int ppo_copy_in(pvae_ctx* c, const FcValueStack& vs, const float* obs, const int32_t* index, long long row0, long long n_rows,
                int rows, hipStream_t st) {
    const pvae_config& cfg = c->L.cfg;
    const NetLayout& TE = c->L.net[PVAE_NET_TE];
    const NetLayout& MD = c->L.net[PVAE_NET_MD];
    const int rows_pad = pad32(rows);
    float* w = c->ws;
    PpoCopyIn a;
    memset(&a, 0, sizeof(a));
    a.obs = obs; a.index = index; a.row0 = row0; a.n_rows = n_rows;
    a.rows = rows; a.rows_pad = rows_pad; a.Db = cfg.dim_body;
    const int te = cfg.te_inputs, md = cfg.md_inputs;
    a.in_off = (te == PVAE_INPUT_TASK ? 1 : 0) | (te == PVAE_INPUT_BODY ? 2 : 0) | (md == PVAE_INPUT_TASK ? 4 : 0);
    a.dst[0] = w + c->W.net[PVAE_NET_TE].in; a.ld[0] = TE.layers[0].ld;
    a.dst[1] = w + c->W.net[PVAE_NET_MD].in; a.ld[1] = MD.layers[0].ld;
    a.dst[2] = vs.in; a.ld[2] = vs.ld_in;
    const int ldmax = std::max(a.ld[0], std::max(a.ld[1], a.ld[2]));
    int gx = (rows_pad * ldmax + 255) / 256;
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(ppo_copy_in_kernel, dim3(gx, 3), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t scratch_bytes(const pvae_config& cfg) { return ppo_scratch_bytes(cfg.max_batch, cfg.dim_action); }

// what neither the step nor the evaluate pass runs: lookahead > 1, the helper, and -- in a context that was not told
// otherwise (option "ppo_priors") -- the learned and the sphere prior
int check_ppo_config(const pvae_ctx* c) {
    const pvae_config& cfg = c->L.cfg;
    if (cfg.lookahead != 1) return fail(-1, "the PPO step needs a lookahead 1 context, got %d", cfg.lookahead);
    if (!c->ppo_priors && cfg.prior_kind != PVAE_PRIOR_ZERO_MEAN && cfg.prior_kind != PVAE_PRIOR_NONE)
        return fail(-1, "the PPO step supports the priors normal_zero_mean_one_std and False, got prior_kind %d", cfg.prior_kind);
    if (cfg.mh_depth > 0) return fail(-1, "the PPO step does not run the motor decoder's helper");
    return 0;
}

// ---- the PPO learner and its train-batch preparation: PhysicsVAE as the driver (pvae_ppo_learner.h) sees it ----
// The context, the value stack set as the checks resolved it, and the latent draws of the call: a step's (`eps`, `noise`,
// `seed`, `offset`), or an evaluate pass's (`draws`).
struct VaeLearner {
    pvae_ctx* c;
    const pvae_ppo_draws* draws = nullptr;
    const float* eps = nullptr; int noise = 0; uint64_t seed = 0, offset = 0;
    FcValueStack vs{};
    PpoLearner* learner() const { return c ? &c->ppo : nullptr; }
    int k() const { return c->L.cfg.dim_action; }
    int n_in() const { return vs.n_in; }
    int max_minibatch() const { return std::min(c->L.cfg.max_batch, vs.max_batch); }
    long long peer_timeout() const { return c->p2p.timeout_ticks; }
    void params_written(hipStream_t st) const { params_touched(c, st); }
    float* eps_out() const { return draws ? draws->eps_out : nullptr; }

    // the checks of a step in their order; check_bound, check_kind and check_update are the parts the second half shares
    int check_bound() const {
        const int rc = check_ready(c, true);
        if (rc) return rc;
        const pvae_ctx::Ppo& q = c->ppo;
        if (!q.grad || !q.m || !q.v || !q.scratch || !q.value) return fail(-2, "pvae_ppo_bind has not been called");
        return 0;
    }
    int check_kind(int log_std_kind) const {
        if (log_std_kind != 0 && log_std_kind != 1)
            return fail(-1, "log_std_kind %d: PhysicsVAE has a constant (0) or state_independent (1) log-std", log_std_kind);
        return 0;
    }
    int check_update(const pvae_fc_ppo_params* p) const {
        if (p->adam_t < 1) return fail(-1, "adam_t must be >= 1");
        if (p->train_mask < 0 || p->train_mask > 7) return fail(-1, "train_mask names a net that does not exist (bits: 1 TE, 2 MD, 4 value)");
        return 0;
    }
    int check_value_stack(pvae_fc* value) {
        const int rc = fc_value_stack(value, &vs);
        if (rc) return rc;
        const int n_obs = 2 * c->L.cfg.dim_body;
        if (vs.n_in != n_obs) return fail(-1, "the value stack reads %d inputs, the observation has %d", vs.n_in, n_obs);
        return 0;
    }
    int check_step(const pvae_fc_ppo_batch* b, const pvae_fc_ppo_params* p, long long first, int rows, const float* stats) {
        int rc = check_bound();
        if (rc) return rc;
        const pvae_ctx::Ppo& q = c->ppo;
        if ((rc = check_loss_args(b, p, rows))) return rc;
        if (!b->obs) return fail(-1, "batch obs is null");
        if (!stats) return fail(-1, "stats_out is null");
        const pvae_config& cfg = c->L.cfg;
        if ((rc = check_ppo_config(c)) || (rc = check_kind(p->log_std_kind))) return rc;
        if (!q.log_std) return fail(-2, "log_std vector not bound (pvae_ppo_bind)");
        if (p->log_std_kind == 1 && (!q.log_std_m || !q.log_std_v)) return fail(-2, "log_std moments not bound (pvae_ppo_bind)");
        if (b->k != cfg.dim_action) return fail(-1, "batch k %d != dim_action %d", b->k, cfg.dim_action);
        if (rows > cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, cfg.max_batch);
        if (first < 0 || first + rows > b->n_rows) return fail(-1, "rows [%lld, +%d) outside the batch of %lld", first, rows, (long long)b->n_rows);
        if ((rc = check_update(p)) || (rc = check_value_stack(q.value))) return rc;
        if (rows > vs.max_batch) return fail(-1, "rows %d > max_batch %d of the value stack set", rows, vs.max_batch);
        return 0;
    }
    int check_apply(const pvae_fc_ppo_params* p, const float* ls_grad) {
        int rc = check_ready(c, true);
        if (rc) return rc;
        if (!p) return fail(-1, "null params");
        if ((rc = check_bound()) || (rc = check_kind(p->log_std_kind)) || (rc = check_update(p))) return rc;
        const pvae_ctx::Ppo& q = c->ppo;
        if (p->log_std_kind == 1 && (!q.log_std || !q.log_std_m || !q.log_std_v)) return fail(-2, "log_std vector or its moments not bound (pvae_ppo_bind)");
        if (p->log_std_kind == 1 && !ls_grad) return fail(-1, "ls_grad is null (log_std_kind 1)");
        return fc_value_stack(q.value, &vs);
    }
    int check_eval(const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out, bool rows_pass);

    int grad_half(const pvae_fc_ppo_batch* b, const int32_t* index, long long first, int rows, const pvae_fc_ppo_params* p,
                  int step, int minibatch, float* dpart, hipStream_t st, int* launches_out) const;
    int segments(const pvae_fc_ppo_params* p, PpoAdamSegs& sg) const;
    template <class Epi>
    int eval_rows(const float* obs, long long n_rows, int k, const pvae_gae_params*, hipStream_t st, int& launches, Epi&& epi) const;
    int eval_boot(const pvae_fc_rollout* ro, const pvae_fc_prepared* out, hipStream_t st, int& launches) const {
        return fc_eval_boot(c->ppo.value, 0, max_minibatch(), ro, out, st, launches);
    }
    // the learner's two gradient arenas as the exchange maps them: the one of pvae_ppo_bind, and the value stack set's
    int peer_arenas(const void*, float** arenas, long long* floats) {
        if (!c) return fail(-1, "null ctx");
        const pvae_ctx::Ppo& q = c->ppo;
        if (!q.grad || !q.value) return fail(-2, "pvae_ppo_bind has not been called");
        const int rc = fc_value_stack(q.value, &vs);
        if (rc) return rc;
        arenas[0] = q.grad; floats[0] = c->L.arena_floats;
        arenas[1] = vs.grad; floats[1] = vs.arena_floats;
        return 2;
    }
};

// The first half of a minibatch's step, everything before the Adam launch: forward, loss head, backward into the bound
// gradient arenas (arguments checked by the caller); `launches_out` counts what went out.  Step `step` of a call draws
// from eps + step * minibatch * Z, or from Philox at offset + step.
int VaeLearner::grad_half(const pvae_fc_ppo_batch* b, const int32_t* index, long long first, int rows, const pvae_fc_ppo_params* p,
                          int step, int minibatch, float* dpart, hipStream_t st, int* launches_out) const {
    const pvae_ctx::Ppo& q = c->ppo;
    const pvae_config& cfg = c->L.cfg;
    const int Db = cfg.dim_body, Z = cfg.latent;
    const int mask = p->train_mask ? p->train_mask : 7;
    const bool train_te = mask & kTrainTE, train_md = mask & kTrainMD, train_v = mask & kTrainValue;
    const int rows_pad = pad32(rows);
    const NetLayout& TE = c->L.net[PVAE_NET_TE];
    const NetLayout& MD = c->L.net[PVAE_NET_MD];
    const NetWork& wte = c->W.net[PVAE_NET_TE];
    const NetWork& wmd = c->W.net[PVAE_NET_MD];
    float* w = c->ws;
    int launches = 0, rc;
    ppo_enter(c, rows);
    if ((rc = ppo_copy_in(c, vs, b->obs, index ? index + first : nullptr, first, b->n_rows, rows, st))) return rc;
    ++launches;
    if (rows <= 4 && rows < rows_pad) {
        ZeroRows z;
        memset(&z, 0, sizeof(z));
        for (const Layer& l : TE.layers) z.add(w + wte.act[l.index], l.n_out_pad, l.n_out_pad);
        for (const Layer& l : MD.layers) z.add(w + wmd.act[l.index], l.n_out_pad, l.n_out_pad);
        for (int i = 0; i < vs.n_panels; ++i) z.add(vs.panel[i], vs.panel_ld[i], vs.panel_ld[i]);
        z.r0 = rows; z.r1 = rows_pad;
        if ((rc = zero_rows_launch(z, st))) return rc;
        ++launches;
    }
    if ((rc = ppo_forward_net(c, PVAE_NET_TE, rows, st, &launches))) return rc;
    if ((rc = ppo_sampler(c, eps ? eps + (size_t)minibatch * Z * step : nullptr, rows, noise, seed, offset + (uint64_t)step, st, &launches)))
        return rc;
    if ((rc = ppo_forward_net(c, PVAE_NET_MD, rows, st, &launches))) return rc;
    if ((rc = fc_value_forward(q.value, 0, rows, st, &launches))) return rc;
    const Layer& md_last = MD.layers.back();
    const Layer& te_last = TE.layers.back();
    const int colsum = p->log_std_kind == 1;
    const bool md_back = train_md || train_te;           // the decoder's backward runs: for its own gradient, or to pass one on
    {
        PpoHead h;
        fill_head(h, b, p, index ? index + first : nullptr, first, rows, rows_pad);
        h.mean = w + wmd.act.back(); h.ld_mean = md_last.n_out_pad;
        h.ls = q.log_std;
        h.value = vs.value; h.ld_value = vs.ld_value;
        if (md_back) { h.d_mean = w + wmd.dz.back(); h.ld_dm = md_last.n_out_pad; h.width_dm = md_last.n_out_pad; }
        if (train_v) { h.d_value = vs.d_value; h.ld_dv = vs.ld_dv; h.width_dv = vs.width_dv; }
        h.part = q.scratch; h.part_stride = part_stride(b->k, colsum != 0); h.colsum = colsum;
        h.dpart = dpart;                                     // (the head's diagnostics partial rows, or null)
        if ((rc = ppo_head_launch(h, st))) return rc;
        ++launches;
    }
    if (md_back && (rc = ppo_backward_net(c, PVAE_NET_MD, rows, train_md, train_te, q.grad, st, &launches))) return rc;
    if (train_te) {
        if (cfg.prior_kind == PVAE_PRIOR_HYPERSPHERE) {
            hipLaunchKernelGGL(ppo_sphere_bwd_kernel, dim3(rows_pad / 4), dim3(256), 0, st, w + wte.act.back(), w + wmd.d_in,
                               MD.layers[0].ld, Db, Z, rows, rows_pad, w + wte.dz.back(), te_last.n_out_pad);
        } else {
            // the learned prior mean (PVAE_PRIOR_STATE_MEAN) is recorded only (rmt:801-809): the sampler is the zero-mean one
            const int with_logvar = cfg.prior_kind == PVAE_PRIOR_ZERO_MEAN || cfg.prior_kind == PVAE_PRIOR_STATE_MEAN;
            int gx = (rows_pad * te_last.n_out_pad + 255) / 256;
            if (gx > 256) gx = 256;
            hipLaunchKernelGGL(ppo_sampler_bwd_kernel, dim3(gx), dim3(256), 0, st, w + wte.act.back(), w + c->W.eps, w + wmd.d_in,
                               MD.layers[0].ld, Db, Z, rows, rows_pad, with_logvar ? 1 : 0, noise ? 1 : 0, w + wte.dz.back(),
                               te_last.n_out_pad);
        }
        HIP_TRY(hipGetLastError());
        ++launches;
        if ((rc = ppo_backward_net(c, PVAE_NET_TE, rows, true, false, q.grad, st, &launches))) return rc;
    }
    if (train_v && (rc = fc_value_backward(q.value, 0, rows, st, &launches))) return rc;
    *launches_out = launches;
    return 0;
}

// the trained nets' segments: what the Adam launch runs over (TE, MD: their parts of the arena; value: its own arena)
int VaeLearner::segments(const pvae_fc_ppo_params* p, PpoAdamSegs& sg) const {
    const pvae_ctx::Ppo& q = c->ppo;
    const int mask = p->train_mask ? p->train_mask : 7;
    const NetLayout& TE = c->L.net[PVAE_NET_TE];
    const NetLayout& MD = c->L.net[PVAE_NET_MD];
    memset((void*)&sg, 0, sizeof(sg));
    auto add = [&](float* pp, const float* gg, float* mm, float* vv, long long n) {
        sg.p[sg.n] = pp; sg.g[sg.n] = gg; sg.m[sg.n] = mm; sg.v[sg.n] = vv; sg.n4[sg.n] = n / 4; ++sg.n;
    };
    if (mask & kTrainTE) add(c->params + TE.off, q.grad + TE.off, q.m + TE.off, q.v + TE.off, TE.count);
    if (mask & kTrainMD) add(c->params + MD.off, q.grad + MD.off, q.m + MD.off, q.v + MD.off, MD.count);
    if (mask & kTrainValue) add(vs.params, vs.grad, vs.m, vs.v, vs.arena_floats);
    return 0;
}

// ---- train-batch preparation (include/pvae.h "Train-batch preparation for PhysicsVAE") ----
// what evaluate and prepare ask of the context; `rows_pass`: the policy's distribution is evaluated over the rows
int VaeLearner::check_eval(const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out, bool rows_pass) {
    const pvae_ppo_draws* d = draws;
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!ro || !p || !out) return fail(-1, "null rollout, params or outputs");
    const pvae_ctx::Ppo& q = c->ppo;
    if (!q.value) return fail(-2, "pvae_ppo_bind has not been called");
    const pvae_config& cfg = c->L.cfg;
    if ((rc = check_ppo_config(c))) return rc;
    if (ro->n_rows < 1 || ro->n_rows > 0x7fffffffll) return fail(-1, "n_rows %lld out of range", (long long)ro->n_rows);
    if (rows_pass) {
        if ((rc = check_kind(p->log_std_kind))) return rc;
        if (!q.log_std) return fail(-2, "log_std vector not bound (pvae_ppo_bind)");
        if (ro->k != cfg.dim_action) return fail(-1, "rollout k %d != dim_action %d", ro->k, cfg.dim_action);
        if (!ro->obs || !ro->actions) return fail(-1, "rollout obs or actions is null");
        if (!out->vf_preds || !out->old_dist || !out->old_logp) return fail(-1, "an evaluate output (vf_preds, old_dist, old_logp) is null");
        if (!d) return fail(-1, "draws is null");
        if (d->noise != 0 && d->noise != 1) return fail(-1, "draws noise must be 0 or 1, got %d", d->noise);
    }
    return check_value_stack(q.value);
}

// rows [n_rows][2 Db] of `obs` through encoder, sampler, decoder and value stack in chunks of max_batch:
// copy-in | TE layers | sampler | MD layers | value layers | the chunk's epilogue -- epi(panels, first row, chunk index)
// launches it (the evaluate one, or the sampling one of pvae_ppo_act)
template <class Epi>
int VaeLearner::eval_rows(const float* obs, long long n_rows, int k, const pvae_gae_params*, hipStream_t st, int& launches,
                          Epi&& epi) const {
    const pvae_config& cfg = c->L.cfg;
    const pvae_ppo_draws* d = draws;
    const int Z = cfg.latent, chunk = max_minibatch();
    const Layer& md_last = c->L.net[PVAE_NET_MD].layers.back();
    uint64_t i = 0;
    for (long long first = 0; first < n_rows; first += chunk, ++i) {
        const int rows = (int)(n_rows - first < chunk ? n_rows - first : chunk);
        int rc;
        ppo_enter(c, rows);
        if ((rc = ppo_copy_in(c, vs, obs, nullptr, first, n_rows, rows, st))) return rc;
        ++launches;
        if ((rc = ppo_forward_net(c, PVAE_NET_TE, rows, st, &launches))) return rc;
        if ((rc = ppo_sampler(c, d->eps ? d->eps + (size_t)first * Z : nullptr, rows, d->noise, d->rng_seed, d->rng_offset + i, st,
                              &launches)))
            return rc;
        if ((rc = ppo_forward_net(c, PVAE_NET_MD, rows, st, &launches))) return rc;
        if ((rc = fc_value_forward(c->ppo.value, 0, rows, st, &launches))) return rc;
        PpoPanels e;
        memset(&e, 0, sizeof(e));
        e.mean = c->ws + c->W.net[PVAE_NET_MD].act.back(); e.ld_mean = md_last.n_out_pad;
        e.ls = c->ppo.log_std;
        e.value = vs.value; e.ld_value = vs.ld_value;
        e.rows = rows; e.k = k;
        e.eps_src = c->ws + c->W.eps; e.Z = Z;
        if ((rc = epi(e, first, i))) return rc;
        ++launches;
    }
    return 0;
}
}  // namespace

extern "C" {

size_t pvae_ppo_workspace_bytes(const pvae_config* cfg) {
    if (!cfg) return 0;
    const Layout L = make_layout(*cfg);
    if (!L.ok) { fail(-1, "bad config: %s", L.why); return 0; }
    return scratch_bytes(*cfg);
}

int pvae_ppo_sizeof(int which) {
    return which == 0 ? (int)sizeof(pvae_fc_ppo_params) : which == 1 ? (int)sizeof(pvae_fc_ppo_batch)
         : which == 2 ? (int)sizeof(pvae_config) : fail(-1, "which must be 0, 1 or 2");
}

int pvae_ppo_bind(pvae_ctx* c, float* grad, float* m, float* v, void* scratch, size_t bytes, float* log_std,
                  float* log_std_m, float* log_std_v, pvae_fc* value) {
    if (!c || !grad || !m || !v || !scratch || !value) return fail(-1, "null argument");
    if (!c->params) return fail(-2, "parameter arena not bound");
    const size_t need = scratch_bytes(c->L.cfg);
    if (bytes < need) return fail(-1, "scratch too small: %zu < %zu bytes", bytes, need);
    int rc = check_ppo_buffers(grad, m, v, scratch, log_std, log_std_m, log_std_v);
    if (rc) return rc;
    if ((rc = VaeLearner{c}.check_value_stack(value))) return rc;
    pvae_ctx::Ppo& q = c->ppo;
    q.grad = grad; q.m = m; q.v = v; q.scratch = (float*)scratch;
    q.log_std = log_std; q.log_std_m = log_std_m; q.log_std_v = log_std_v;
    q.value = value;
    return 0;
}

int pvae_ppo_step(pvae_ctx* c, const pvae_fc_ppo_batch* b, const int32_t* index, int64_t first, int32_t rows,
                  const pvae_fc_ppo_params* p, const float* eps, int noise, uint64_t rng_seed, uint64_t rng_offset,
                  float* stats_out, void* stream) {
    return learner_step(VaeLearner{c, nullptr, eps, noise, rng_seed, rng_offset}, b, index, first, rows, p, stats_out,
                        (hipStream_t)stream);
}

int pvae_ppo_sgd(pvae_ctx* c, const pvae_fc_ppo_batch* b, const int32_t* perm, int32_t minibatch, int32_t num_sgd_iter,
                 const pvae_fc_ppo_params* p, const float* eps, int noise, uint64_t rng_seed, uint64_t rng_offset,
                 float* stats_out, void* stream) {
    return learner_sgd(VaeLearner{c, nullptr, eps, noise, rng_seed, rng_offset}, b, perm, minibatch, num_sgd_iter, p, stats_out,
                       (hipStream_t)stream);
}

size_t pvae_ppo_diag_bytes(pvae_ctx* c, int32_t steps) {
    if (!c) { fail(-1, "null ctx"); return 0; }
    if (steps < 1) { fail(-1, "steps must be >= 1, got %d", steps); return 0; }
    return ppo_diag_bytes(c->L.cfg.max_batch);           // (the norm is finished per step: no per-step slot rows)
}

int pvae_ppo_diag(pvae_ctx* c, float* diag, int32_t capacity_steps, void* scratch, size_t scratch_bytes) {
    if (!c) return fail(-1, "null ctx");
    return ppo_diag_bind(c->ppo.diag, diag, capacity_steps, scratch, scratch_bytes, c->L.cfg.max_batch);
}

size_t pvae_ppo_grad_clip_bytes(pvae_ctx* c) {
    if (!c) { fail(-1, "null ctx"); return 0; }
    return ppo_clip_bytes();                             // (one slot per workgroup of a bounded grid: no size enters)
}

int pvae_ppo_grad_clip(pvae_ctx* c, float max_norm, void* scratch, size_t scratch_bytes) {
    if (!c) return fail(-1, "null ctx");
    return ppo_clip_bind(c->ppo.clip, max_norm, scratch, scratch_bytes);
}

int pvae_ppo_grad(pvae_ctx* c, const pvae_fc_ppo_batch* b, const int32_t* index, int64_t first, int32_t rows,
                  const pvae_fc_ppo_params* p, const float* eps, int noise, uint64_t rng_seed, uint64_t rng_offset,
                  float* stats_out, float* ls_grad, void* stream) {
    return learner_grad(VaeLearner{c, nullptr, eps, noise, rng_seed, rng_offset}, b, index, first, rows, p, stats_out, ls_grad,
                        (hipStream_t)stream);
}

int pvae_ppo_apply(pvae_ctx* c, const pvae_fc_ppo_params* p, float grad_scale, const float* ls_grad, void* stream) {
    return learner_apply(VaeLearner{c}, p, grad_scale, ls_grad, (hipStream_t)stream);
}

int pvae_ppo_peer_export(pvae_ctx* c, void* blob) {
    return learner_peer_export(VaeLearner{c}, blob);
}

int pvae_ppo_peer_open(pvae_ctx* c, int rank, int world, const void* blobs) {
    return learner_peer_open(VaeLearner{c}, rank, world, blobs);
}

int pvae_ppo_peer_close(pvae_ctx* c) {
    if (!c) return fail(-1, "null ctx");
    return ppo_peer_close(c->ppo.peers);
}

int pvae_ppo_peer_status(pvae_ctx* c, int* rank, int* world, uint32_t* timeouts, void* stream) {
    if (!c) return fail(-1, "null ctx");
    return ppo_peer_status(c->ppo.peers, rank, world, timeouts, (hipStream_t)stream);
}

int pvae_ppo_launches(pvae_ctx* c, int32_t* per_step) {
    return learner_launches(c ? &c->ppo : nullptr, per_step);
}

int pvae_ppo_evaluate(pvae_ctx* c, const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_ppo_draws* d,
                      const pvae_fc_prepared* out, void* stream) {
    return learner_evaluate(VaeLearner{c, d}, ro, p, out, (hipStream_t)stream);
}

int pvae_ppo_prepare(pvae_ctx* c, const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_ppo_draws* d,
                     const pvae_fc_prepared* out, void* scratch, size_t scratch_bytes, void* stream) {
    return learner_prepare(VaeLearner{c, d}, ro, p, out, scratch, scratch_bytes, (hipStream_t)stream);
}

int pvae_ppo_act(pvae_ctx* c, const pvae_ppo_act_in* in, const pvae_gae_params* p, const pvae_ppo_draws* d,
                 const pvae_ppo_act_out* out, void* stream) {
    return learner_act(VaeLearner{c, d}, in, p, out, (hipStream_t)stream);
}

int pvae_ppo_gae_launches(pvae_ctx* c, int32_t* evaluate, int32_t* rest) {
    if (!c) return fail(-1, "null ctx");
    return learner_gae_launches(c->ppo, evaluate, rest);
}

}  // extern "C"
