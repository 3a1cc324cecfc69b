// pvae_step.hip -- the training step at lookahead 1 (forward launches, loss terms, the backward plan across the stacks) and
// the step's C ABI: pvae_forward_backward and its pieces, the Adam calls, the direct, prefetch and data-parallel steps.
#include "pvae_internal.h"

// dst[r][c] += s0[r][c] (+ s1 + s2 + s3), c < n, r < rows: the gradient wrt the state handed from
// step t to step t+1 is the sum of what came back through every consumer of that state (encoder,
// decoder and the world-model invocations of step t+1).  Fixed summation order.
__global__ void __launch_bounds__(256)
add_cols_kernel(float* __restrict__ dst, int ldd, int rows, int n, const float* __restrict__ s0, int l0,
                const float* __restrict__ s1, int l1, const float* __restrict__ s2, int l2,
                const float* __restrict__ s3, int l3) {
    const int total = rows * n;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / n, c = idx - r * n;
        float v = dst[(size_t)r * ldd + c];
        if (s0) v += s0[(size_t)r * l0 + c];
        if (s1) v += s1[(size_t)r * l1 + c];
        if (s2) v += s2[(size_t)r * l2 + c];
        if (s3) v += s3[(size_t)r * l3 + c];
        dst[(size_t)r * ldd + c] = v;
    }
}

int add_cols_launch(float* dst, int ldd, int rows, int n, const float* s0, int l0, const float* s1, int l1, const float* s2,
                    int l2, const float* s3, int l3, hipStream_t st) {
    hipLaunchKernelGGL(add_cols_kernel, dim3(grid1d(rows * n, 256)), dim3(256), 0, st, dst, ldd, rows, n, s0, l0, s1, l1, s2, l2,
                       s3, l3);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Backward of the motor decoder's helper term (helper_add_kernel, pvae_net.hip): the gradient wrt the action reaches the helper's pre-activation through range * tanh'
// (dz_h = range * (1 - h^2) * d a_hat); pad rows / columns of the panel are written as zeros.
__global__ void __launch_bounds__(256)
helper_seed_kernel(const float* __restrict__ dz_a, int lda, const float* __restrict__ h, float* __restrict__ dz_h, int ldh,
                   int rows, int rows_pad, int Da, float range) {
    const int total = rows_pad * ldh;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / ldh, c = idx - r * ldh;
        float g = 0.f;
        if (r < rows && c < Da) {
            const float t = h[idx];
            g = range * (1.0f - t * t) * dz_a[(size_t)r * lda + c];
        }
        dz_h[idx] = g;
    }
}

int helper_seed_launch(pvae_ctx* c, int rows, int64_t row0, hipStream_t st) {
    const int ld_md = c->L.net[PVAE_NET_MD].layers.back().n_out_pad, ldh = c->L.net[PVAE_NET_MH].layers.back().n_out_pad;
    const NetWork& wmh = c->W.net[PVAE_NET_MH];
    hipLaunchKernelGGL(helper_seed_kernel, dim3(grid1d(pad32(rows) * ldh, 256)), dim3(256), 0, st,
                       c->ws + c->W.net[PVAE_NET_MD].dz.back() + row0 * ld_md, ld_md, c->ws + wmh.act.back() + row0 * ldh,
                       c->ws + wmh.dz.back() + row0 * ldh, ldh, rows, pad32(rows), c->L.cfg.dim_action, c->L.cfg.mh_range);
    HIP_TRY(hipGetLastError());
    return 0;
}

// nn.MSELoss (tm:99; or nn.L1Loss, tm:100-101, when l1) of pred vs target over rows x D, plus its
// gradient:
//   partial[b] = sum (pred - target)^2 over this block's rows      (finalize scales by 1/(B*D))
//   dz = grad_scale * (pred - target) [+ extra]                    grad_scale = coeff*2/(B*D)
//   L1: partial = sum |pred - target|, dz = grad_scale * sign(pred - target), grad_scale = coeff/(B*D)
// Used for the world-model MSE (tpv:411-414), the cycle loss (tpv:417-419) and the action
// reconstruction loss (tpv:381-382; `extra` = gradient arriving through the frozen world
// model, columns [Db, Db+Da) of d(wm_in)).
__global__ void __launch_bounds__(256)
mse_grad_kernel(const float* __restrict__ pred, int ldp, const float* __restrict__ target, int ldt,
                float* __restrict__ dz, int ldz, int rows, int rows_pad, int D, float grad_scale,
                const float* __restrict__ extra, int lde, int extra_col0, float* __restrict__ partial, int l1) {
    float acc = 0.f;
    for (int r = blockIdx.x; r < rows_pad; r += gridDim.x) {
        const bool valid = r < rows;
        for (int c = threadIdx.x; c < ldz; c += 256) {
            float g = 0.f;
            if (valid && c < D) {
                const float d = pred[(size_t)r * ldp + c] - target[(size_t)r * ldt + c];
                acc += l1 ? fabsf(d) : d * d;
                g = grad_scale * (l1 ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : d);
                if (extra) g += extra[(size_t)r * lde + extra_col0 + c];
            }
            if (dz) dz[(size_t)r * ldz + c] = g;
        }
    }
    const float s = block_sum_256(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the action-reconstruction term of time step t: the decoder's row block `row0` against a_t, `extra` from the input
// gradient of the world model's row block `wm_row0`
int action_loss_launch(pvae_ctx* c, int rows, int t, int64_t row0, int64_t wm_row0, int nparts, float grad_scale, int l1,
                       bool backward, bool extra, hipStream_t st) {
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action;
    const int ld_md = c->L.net[PVAE_NET_MD].layers.back().n_out_pad, ld_wm = c->L.net[PVAE_NET_WM].layers[0].ld;
    const NetWork& wmd = c->W.net[PVAE_NET_MD];
    hipLaunchKernelGGL(mse_grad_kernel, dim3(nparts), dim3(256), 0, st, c->ws + wmd.act.back() + row0 * ld_md, ld_md,
                       c->ws + c->W.act_t + row0 * pad64(Da), pad64(Da),
                       backward ? c->ws + wmd.dz.back() + row0 * ld_md : (float*)nullptr, ld_md, rows, pad32(rows), Da, grad_scale,
                       extra ? c->ws + c->W.net[PVAE_NET_WM].d_in + wm_row0 * ld_wm : (const float*)nullptr, ld_wm, Db,
                       c->ws + c->W.loss_part + 1 * kLossParts + t * nparts, l1);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Backward of the sampler + KL (autograd of rmt:734-740 and tpv:388):
//   dmu = dz + (beta/B) mu ;  dlogvar = dz * eps * 0.5 exp(0.5 lv) + (beta/B) 0.5 (exp(lv) - 1)
__global__ void __launch_bounds__(256)
reparam_bwd_kernel(const float* __restrict__ d_md_in, int ld_md, int Db, const float* __restrict__ te_out,
                   int ldte, const float* __restrict__ eps_used, float* __restrict__ dz_te, int ld_dz,
                   int rows, int rows_pad, int Z, float kl_scale, const float* __restrict__ mu_p = nullptr,
                   int ldmp = 0, float* __restrict__ dz_p = nullptr, int ldzp = 0) {
    const int total = rows_pad * ld_dz;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / ld_dz, c = idx - r * ld_dz;
        float g = 0.f;
        if (r < rows && c < 2 * Z) {
            const int cz = c < Z ? c : c - Z;
            const float dzv = d_md_in[(size_t)r * ld_md + Db + cz];
            const float mu = te_out[(size_t)r * ldte + cz];
            const float lv = te_out[(size_t)r * ldte + Z + cz];
            if (c < Z) {
                if (mu_p) {
                    const float gp = kl_scale * (mu - mu_p[(size_t)r * ldmp + cz]);
                    g = dzv + gp;
                    if (dz_p) dz_p[(size_t)r * ldzp + cz] = -gp;
                } else {
                    g = dzv + kl_scale * mu;
                }
            } else {
                const float e = eps_used[(size_t)r * Z + cz];
                g = dzv * e * 0.5f * expf(0.5f * lv) + kl_scale * 0.5f * (expf(lv) - 1.0f);
            }
        }
        dz_te[idx] = g;
        if (dz_p && c < Z && r >= rows) dz_p[(size_t)r * ldzp + c] = 0.f;
    }
}

// on row block `row0`: the decoder's input gradient -> the encoder's (and the learned prior's) output gradient
int reparam_bwd_launch(pvae_ctx* c, int rows, int64_t row0, float kl_scale, hipStream_t st) {
    const int Db = c->L.cfg.dim_body, Z = c->L.cfg.latent, rows_pad = pad32(rows);
    const int ld_md = c->L.net[PVAE_NET_MD].layers[0].ld, ld_te = c->L.net[PVAE_NET_TE].layers.back().n_out_pad;
    const NetWork& wte = c->W.net[PVAE_NET_TE];
    const NetLayout& PR = c->L.net[PVAE_NET_PR];
    const NetWork& wpr = c->W.net[PVAE_NET_PR];
    const bool learned_prior = !PR.layers.empty();             // (lookahead 1 only: row0 == 0)
    const int ld_pr = learned_prior ? PR.layers.back().n_out_pad : 0;
    hipLaunchKernelGGL(reparam_bwd_kernel, dim3(grid1d(rows_pad * ld_te, 256)), dim3(256), 0, st,
                       c->ws + c->W.net[PVAE_NET_MD].d_in + row0 * ld_md, ld_md, Db, c->ws + wte.act.back() + row0 * ld_te, ld_te,
                       c->ws + c->W.eps + row0 * Z, c->ws + wte.dz.back() + row0 * ld_te, ld_te, rows, rows_pad, Z, kl_scale,
                       learned_prior ? c->ws + wpr.act.back() : (const float*)nullptr, ld_pr,
                       learned_prior ? c->ws + wpr.dz.back() : (float*)nullptr, ld_pr);
    HIP_TRY(hipGetLastError());
    return 0;
}

// its backward: g = dL/dz = (what came back through the decoder) + (beta/B) u;  dL/de = (g - z <z, g>) / |e|
__global__ void __launch_bounds__(256)
sphere_bwd_kernel(const float* __restrict__ d_md_in, int ld_md, int Db, const float* __restrict__ te_out, int ldte,
                  const float* __restrict__ u_used, float* __restrict__ dz_te, int ld_dz, int rows, int rows_pad,
                  int Z, float kl_scale, int normalize) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;
    if (r >= rows_pad) return;
    float e2 = 0.f, zg = 0.f;
    if (r < rows)
        for (int c = lane; c < Z; c += 64) {
            const float e = te_out[(size_t)r * ldte + c];
            e2 += e * e;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e2 += __shfl_xor(e2, o, 64);
    const float ie = 1.0f / fmaxf(sqrtf(e2), 1e-12f);
    if (!normalize) {                          // z = e: the decoder's input gradient is the encoder's output gradient
        for (int c = lane; c < ld_dz; c += 64)
            dz_te[(size_t)r * ld_dz + c] = (r < rows && c < Z) ? d_md_in[(size_t)r * ld_md + Db + c] : 0.f;
        return;
    }
    if (r < rows)
        for (int c = lane; c < Z; c += 64) {
            const float g = d_md_in[(size_t)r * ld_md + Db + c] + kl_scale * u_used[(size_t)r * Z + c];
            zg += te_out[(size_t)r * ldte + c] * ie * g;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) zg += __shfl_xor(zg, o, 64);
    for (int c = lane; c < ld_dz; c += 64) {
        float d = 0.f;
        if (r < rows && c < Z) {
            const float g = d_md_in[(size_t)r * ld_md + Db + c] + kl_scale * u_used[(size_t)r * Z + c];
            d = (g - te_out[(size_t)r * ldte + c] * ie * zg) * ie;
        }
        dz_te[(size_t)r * ld_dz + c] = d;
    }
}

// Evaluation-only finalisation (training folds it into the last weight-gradient launch).
__global__ void finalize_loss_kernel(LossFinal f) { finalize_loss_wave(f, threadIdx.x); }

// Can this training step read the demonstration set directly?  (Everything else keeps the staging launch.)
static bool direct_ok(const pvae_ctx* c, int phase, int rows, const pvae_step_params* sp, bool fused) {
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action, Z = c->L.cfg.latent;
    if (!c->direct || !c->data_slack || !c->states || c->next_states || c->W.L != 1 || !c->pair_launch || !c->same_layer_pairs)
        return false;
    if (rows <= 4 || c->L.cfg.prior_kind != PVAE_PRIOR_ZERO_MEAN || !c->L.net[PVAE_NET_PR].layers.empty()) return false;
    // input subsets: the staged panels carry the zeros.  Each field on its own -- BODY (1) on one stack and TASK (2) on
    // the other OR to 3, which is also what "both" is spelt as
    if (c->L.cfg.te_inputs % 3 != 0 || c->L.cfg.md_inputs % 3 != 0) return false;
    if (!c->L.net[PVAE_NET_MH].layers.empty()) return false;                     // the helper reads the staged decoder panel
    if (fused && !can_defer_adam(c, fused)) return false;             // (the same-layer schedule of plan_backward_net)
    if (Da > ProCols::kMaxN || Z > ProCols::kMaxN || Db < 64 || 2 * Db >= 65536) return false;
    const int rp = pad32(rows);
    // a first layer on 64-row tiles has no Pro patch: its second column block is chunk-selected, which needs dim_body % 4 == 0
    auto layer0_ok = [&](int net, bool second_block) {
        const NetLayout& N = c->L.net[net];
        if (N.layers.size() < 2) return false;
        const int n = N.layers[0].n_out_pad;
        if (!forward_gather_ok(rp, n)) return false;
        return !(second_block && uses_64x32(rp, n) && (Db & 3));
    };
    if (phase == PVAE_PHASE_WORLD) return layer0_ok(PVAE_NET_WM, true);
    if (!(sp->cycle_coeff > 0.0f)) return false;                      // (the action loss sits in the world model's seed epilogue)
    if (!layer0_ok(PVAE_NET_TE, false) || !layer0_ok(PVAE_NET_MD, true) || !layer0_ok(PVAE_NET_WM, true)) return false;
    // decoder on 32x32 tiles: z comes from the sampler prologue of that very launch
    if (!uses_64x32(rp, c->L.net[PVAE_NET_MD].layers[0].n_out_pad) && !sampler_folds(c, rows)) return false;
    return true;
}

static int step_shape(pvae_ctx* c, int phase, int rows, const pvae_step_params* sp, float* loss_out, bool backward,
                      StepShape& S) {
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action, Z = c->L.cfg.latent;
    S.rows_pad = pad32(rows);
    S.l1 = sp->loss_kind == PVAE_LOSS_L1 ? 1 : 0;
    S.gs = S.l1 ? 1.0f : 2.0f;
    S.Bg = (float)(sp->global_rows > 0 ? sp->global_rows : rows);
    const int T = c->W.L;
    S.wm_tiles = forward_tiles(S.rows_pad, c->L.net[PVAE_NET_WM].layers.back().n_out_pad);
    if ((int64_t)S.wm_tiles * T > kLossParts)
        return fail(-1, "batch x dim_body x lookahead too large for the loss partial buffer");
    S.Bg *= (float)T;                          // every term is the mean over the L steps (tpv:423-428)
    S.gridz = sampler_grid(c, S.rows_pad);
    S.fold_sampler = phase == PVAE_PHASE_JOINT && sampler_folds(c, rows);
    if (S.fold_sampler) S.gridz = S.rows_pad / 32;          // one KL partial per row block
    (void)Z;
    S.nparts_a = S.rows_pad < 64 ? S.rows_pad : 64;
    S.cyc_grad = backward && phase == PVAE_PHASE_JOINT && sp->cycle_coeff > 0.0f;
    S.kl_active = phase == PVAE_PHASE_JOINT && sp->kl_coeff > 0.0f && sp->a_rec_coeff > 0.0f &&   // tpv:381-384
                  c->L.cfg.prior_kind != PVAE_PRIOR_NONE;                 // (`if self.latent_prior_type and ...`)
    // (the sphere's backward needs a dot product over a whole latent row, which no tile epilogue sees)
    // (a helper stack sits between the two hand-overs -- its seed reads the decoder's, its input gradient joins the
    //  decoder's before the sampler backward -- so a helper model takes the stand-alone glue kernels)
    S.seed_sampler = backward && phase == PVAE_PHASE_JOINT && c->W.L == 1 && c->pair_launch &&
                     c->L.cfg.prior_kind < PVAE_PRIOR_HYPERSPHERE && c->L.net[PVAE_NET_MH].layers.empty();
    S.seed_action = S.seed_sampler && S.cyc_grad;
    float* part = c->ws + c->W.loss_part;
    memset(&S.lf, 0, sizeof(S.lf));
    for (int t = 0; t < 4; ++t) S.lf.part[t] = part + (t + 1) * kLossParts;
    S.lf.out = loss_out;
    S.lf.scale[0] = 1.0f / (S.Bg * Da); S.lf.scale[1] = 1.0f / S.Bg;
    S.lf.scale[2] = 1.0f / (S.Bg * Db); S.lf.scale[3] = 1.0f / (S.Bg * Db);
    S.lf.coeff[0] = sp->a_rec_coeff; S.lf.coeff[1] = sp->kl_coeff;
    S.lf.coeff[2] = sp->s_rec_coeff; S.lf.coeff[3] = sp->cycle_coeff;
    if (phase == PVAE_PHASE_WORLD) {
        S.lf.nparts[2] = S.wm_tiles * T;
    } else {
        if (sp->a_rec_coeff > 0.0f)
            S.lf.nparts[0] = S.seed_action ? dgrad_tiles(S.rows_pad, seed_window(Db, Da).width) : S.nparts_a * T;
        if (S.kl_active) S.lf.nparts[1] = S.gridz * T;
        if (sp->s_rec_coeff > 0.0f) S.lf.nparts[2] = S.wm_tiles * T;       // tpv:411-414 with the world model frozen
        if (sp->cycle_coeff > 0.0f) S.lf.nparts[3] = S.wm_tiles * T;
    }
    return 0;
}

static int check_step(pvae_ctx* c, int phase, int32_t rows, const pvae_step_params* sp, bool backward, bool fused) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!sp) return fail(-1, "null step params");
    if (phase != PVAE_PHASE_WORLD && phase != PVAE_PHASE_JOINT) return fail(-1, "unknown phase %d", phase);
    if (sp->loss_kind != PVAE_LOSS_MSE && sp->loss_kind != PVAE_LOSS_L1) return fail(-1, "unknown loss_kind %d", sp->loss_kind);
    if (rows < 1 || rows > c->L.cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, c->L.cfg.max_batch);
    if (rows != c->staged_rows) return fail(-2, "rows %d != staged rows %d", rows, c->staged_rows);
    if (backward && fused && (!c->m || !c->v)) return fail(-2, "Adam moment arenas not bound");
    if (backward && !fused && !c->grads) return fail(-2, "gradient arena not bound");
    // (the reference's joint default is 0.0, tpv:284: a context runs the term in the joint phase once its owner has said so)
    if (phase == PVAE_PHASE_JOINT && sp->s_rec_coeff != 0.0f && !c->joint_s_rec)
        return fail(-4, "joint phase with world_model_s_rec_coeff != 0 is not supported unless the context opts in "
                        "(pvae_set_option \"joint_s_rec\"; reference default is 0.0, tpv:284)");
    return 0;
}

// Forward launches + loss partials + the gradient seed of the world model's output layer.
static int run_forward(pvae_ctx* c, int phase, int rows, const pvae_step_params* sp, const float* eps, bool backward,
                       const StepShape& S, hipStream_t st) {
    if (c->W.L > 1) return run_forward_unrolled(c, phase, rows, sp, eps, backward, S, st);
    int rc;
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action, Z = c->L.cfg.latent;
    float* w = c->ws;
    float* part = w + c->W.loss_part;
    const NetLayout& TE = c->L.net[PVAE_NET_TE];
    const NetLayout& MD = c->L.net[PVAE_NET_MD];
    const NetLayout& WM = c->L.net[PVAE_NET_WM];
    const NetWork& wte = c->W.net[PVAE_NET_TE];
    const NetWork& wmd = c->W.net[PVAE_NET_MD];
    const NetWork& wwm = c->W.net[PVAE_NET_WM];
    // world-model output layer fused with MSE(s2, .) and its gradient
    EpiMse mse;
    memset(&mse, 0, sizeof(mse));
    mse.target = w + c->W.s2; mse.ldt = pad64(Db);
    mse.dz = backward ? w + wwm.dz.back() : nullptr; mse.ldz = WM.layers.back().n_out_pad;
    mse.rows = rows; mse.D = Db; mse.l1 = S.l1;
    FwdTail wm_tail;
    wm_tail.mse = &mse;
    // direct step: every stack's first layer gathers its rows itself, s_{t+1} is read from `states` by the loss epilogue
    const bool dx = c->dx.on;
    XSrc xs_te, xs_md, xs_wm, xs_wg;
    ProCols wm_cols, wg_cols;
    // the world model's gathered first layer: [s_t | a_t] (`src_phase` WORLD) or [s_t | a_hat] (JOINT)
    auto wm_direct = [&](int src_phase, XSrc& xs, ProCols& cols, FwdTail& tail) {
        memset(&cols, 0, sizeof(cols));
        const bool wm64 = uses_64x32(S.rows_pad, WM.layers[0].n_out_pad);
        xs = xsrc_of(c, PVAE_NET_WM, src_phase, wm64, rows);
        tail.xs0 = &xs;
        if (!wm64) {
            const XSrc full = xsrc_of(c, PVAE_NET_WM, src_phase, true, rows);
            cols.src = full.s1; cols.ind = full.ind1; cols.rm = full.rm; cols.ld = full.ld1; cols.c0 = Db; cols.n = Da;
            cols.rows = rows;
            tail.cols0 = &cols;
        }
    };
    memset(&wm_cols, 0, sizeof(wm_cols));
    if (dx) {
        mse.target = c->states + Db; mse.ldt = Db; mse.tind = 1; mse.trm = c->dx.rm;   // row + 1 of the window's s_t
        wm_direct(phase, xs_wm, wm_cols, wm_tail);
    }
    if (phase == PVAE_PHASE_WORLD) {
        // tpv:411-414: L = s_rec * MSE(s2, WM(s1, a_gt)); only the world model learns (tpv:326-329)
        mse.grad_scale = sp->s_rec_coeff * S.gs / (S.Bg * Db);
        mse.partial = part + 3 * kLossParts;
        return forward_net(c, PVAE_NET_WM, S.rows_pad, st, wm_tail);
    }
    const NetLayout& PR = c->L.net[PVAE_NET_PR];
    const NetWork& wpr = c->W.net[PVAE_NET_PR];
    const bool learned_prior = !PR.layers.empty();
    if (!c->seed_pads_clean) {
        // the seed epilogues (plan_backward) write only the real columns of these gradient
        // panels; their pad columns must be zero and nothing else ever writes them
        HIP_TRY(hipMemsetAsync(w + wmd.dz.back(), 0, (size_t)c->W.Bp * MD.layers.back().n_out_pad * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(w + wte.dz.back(), 0, (size_t)c->W.Bp * TE.layers.back().n_out_pad * sizeof(float), st));
        if (learned_prior)
            HIP_TRY(hipMemsetAsync(w + wpr.dz.back(), 0, (size_t)c->W.Bp * PR.layers.back().n_out_pad * sizeof(float), st));
        c->seed_pads_clean = true;
    }
    if (sp->s_rec_coeff > 0.0f) {
        // tpv:411-414 with the world model frozen (tpv:347-350): s1 and a_gt are data, so MSE(s2, WM(s1, a_gt)) adds
        // s_rec * loss_s to the loss and nothing to any gradient -- forward only, no dz.  It runs FIRST: the input panel
        // holds [s1 | a_gt] until the decoder's tail puts a_hat into the action columns, and the activations it leaves
        // are overwritten by the predicted-action pass below.
        EpiMse mse_g = mse;
        mse_g.dz = nullptr; mse_g.grad_scale = 0.0f;
        mse_g.partial = part + 3 * kLossParts;
        FwdTail wg_tail;
        wg_tail.mse = &mse_g;
        if (dx) wm_direct(PVAE_PHASE_WORLD, xs_wg, wg_cols, wg_tail);
        if ((rc = forward_net(c, PVAE_NET_WM, S.rows_pad, st, wg_tail))) return rc;
    }
    // joint forward: [prior mean ->] TE -> sampler -> MD -> WM (rmt:742-771, 801-809)
    if (learned_prior && (rc = forward_net(c, PVAE_NET_PR, S.rows_pad, st))) return rc;
    FwdTail te_tail;
    if (dx) { xs_te = xsrc_of(c, PVAE_NET_TE, phase, false, rows); te_tail.xs0 = &xs_te; }
    if ((rc = forward_net(c, PVAE_NET_TE, S.rows_pad, st, te_tail))) return rc;
    ProSampler pro;
    memset(&pro, 0, sizeof(pro));
    if (S.fold_sampler) {                      // the sampler rides in the decoder's first-layer launch
        pro.te_out = w + wte.act.back(); pro.ldte = TE.layers.back().n_out_pad;
        pro.eps_in = eps; pro.eps_used = w + c->W.eps;
        pro.md_in = w + wmd.in; pro.ld_md = MD.layers[0].ld;
        pro.c0 = Db; pro.Z = Z; pro.rows = rows; pro.noise = 1;
        pro.seed = (unsigned long long)sp->rng_seed; pro.offset = (unsigned long long)sp->rng_offset;
        pro.partial = part + 2 * kLossParts;
    } else if ((rc = launch_sampler(c, w + wte.act.back(), TE.layers.back().n_out_pad, eps, w + c->W.eps, w + wmd.in,
                                    MD.layers[0].ld, rows, S.rows_pad, 1, (unsigned long long)sp->rng_seed,
                                    (unsigned long long)sp->rng_offset, part + 2 * kLossParts, (float*)nullptr,
                                    learned_prior ? w + wpr.act.back() : (const float*)nullptr,
                                    learned_prior ? PR.layers.back().n_out_pad : 0, st))) {
        return rc;
    }
    FwdTail md_tail;                           // a_hat also lands in the action columns of the WM input
    md_tail.out2 = w + wwm.in; md_tail.ld2 = WM.layers[0].ld; md_tail.off2 = Db; md_tail.n2 = Da;
    if (S.fold_sampler) md_tail.pro0 = &pro;
    if (dx) { xs_md = xsrc_of(c, PVAE_NET_MD, phase, !S.fold_sampler, rows); md_tail.xs0 = &xs_md; }
    if ((rc = forward_net(c, PVAE_NET_MD, S.rows_pad, st, md_tail))) return rc;
    const NetLayout& MH = c->L.net[PVAE_NET_MH];
    if (!MH.layers.empty()) {                  // rmt:833-835: the helper's term joins the action before anything reads it
        if ((rc = forward_net(c, PVAE_NET_MH, S.rows_pad, st))) return rc;
        if ((rc = helper_add_launch(c, rows, 0, 0, st))) return rc;
    }
    // cycle loss (tpv:417-419) fused into the world model's output layer
    mse.grad_scale = sp->cycle_coeff * S.gs / (S.Bg * Db);
    mse.partial = part + 4 * kLossParts;
    return forward_net(c, PVAE_NET_WM, S.rows_pad, st, wm_tail);
}

// Everything after the forward pass, as stages.  (The action-reconstruction loss sits here: its
// gradient needs what came back through the frozen world model.)
static void plan_backward(pvae_ctx* c, int phase, int rows, const pvae_step_params* sp, bool backward, bool fused,
                          const StepShape& S, hipStream_t st, Plan& plan) {
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action, Z = c->L.cfg.latent;
    if (c->W.L > 1) {
        plan_backward_unrolled(c, phase, rows, sp, backward, fused, S, st, plan);
        return;
    }
    float* w = c->ws;
    float* part = w + c->W.loss_part;
    const LossFinal* fold = S.lf.out ? &S.lf : nullptr;
    if (phase == PVAE_PHASE_WORLD) {
        if (backward) plan_backward_net(c, PVAE_NET_WM, S.rows_pad, true, false, sp, fused, st, fold, plan);
        return;
    }
    const NetLayout* TE = &c->L.net[PVAE_NET_TE];
    const NetLayout* MD = &c->L.net[PVAE_NET_MD];
    const NetWork* wte = &c->W.net[PVAE_NET_TE];
    const NetWork* wmd = &c->W.net[PVAE_NET_MD];
    const NetLayout* PR = &c->L.net[PVAE_NET_PR];
    const NetWork* wpr = &c->W.net[PVAE_NET_PR];
    const bool learned_prior = !PR->layers.empty();
    const bool sphere = c->L.cfg.prior_kind >= PVAE_PRIOR_HYPERSPHERE;     // (incl. NONE: the same kernel, not normalising)
    const int sphere_norm = c->L.cfg.prior_kind == PVAE_PRIOR_HYPERSPHERE ? 1 : 0;
    const int ldo_md = MD->layers.back().n_out_pad, ldo_te = TE->layers.back().n_out_pad;
    const float ga = sp->a_rec_coeff * S.gs / (S.Bg * Da);
    // The two gradient hand-overs between stacks live in the epilogue of the consuming stack's
    // first-layer input-gradient launch (InputSeed) whenever that launch exists and runs the paired
    // schedule; otherwise the stand-alone glue kernels do the same arithmetic.
    const bool seed_action = S.seed_action, seed_sampler = S.seed_sampler;
    if (S.cyc_grad) {                          // gradient through the frozen world model (dgrad only)
        InputSeed sd;
        if (seed_action) {
            sd.kind = 1;
            memset(&sd.a, 0, sizeof(sd.a));
            sd.a.pred = w + wmd->act.back(); sd.a.ldp = ldo_md;
            sd.a.target = w + c->W.act_t; sd.a.ldt = pad64(Da);
            if (c->dx.on) { sd.a.target = c->actions; sd.a.ldt = Da; sd.a.tind = 1; sd.a.trm = c->dx.rm; }     // a_t where it lies
            sd.a.dz = w + wmd->dz.back(); sd.a.ldz = ldo_md;
            sd.a.c0 = Db; sd.a.n = Da; sd.a.rows = rows;
            sd.a.grad_scale = ga; sd.a.l1 = S.l1;
            sd.a.partial = part + 1 * kLossParts;
        }
        plan_backward_net(c, PVAE_NET_WM, S.rows_pad, false, true, sp, fused, st, nullptr, plan, &sd);
    }
    // action reconstruction (tpv:381-382) + gradient arriving through the world model
    if (!seed_action) {
        const int nparts = S.nparts_a, l1 = S.l1;
        const bool cyc = S.cyc_grad;
        push(plan, [=] { return action_loss_launch(c, rows, 0, 0, 0, nparts, ga, l1, backward, cyc, st); });
    }
    if (!backward) return;
    const NetLayout* MH = &c->L.net[PVAE_NET_MH];
    const NetWork* wmh = &c->W.net[PVAE_NET_MH];
    const bool helper = !MH->layers.empty();
    if (helper) {
        // d a_hat (just formed above: reconstruction + what came back through the world model) -> the helper's output layer,
        // then the helper's own backward: trained like the decoder (adam_t[PVAE_NET_MH] > 0) or passed through
        push(plan, [=] { return helper_seed_launch(c, rows, 0, st); });
        plan_backward_net(c, PVAE_NET_MH, S.rows_pad, sp->adam_t[PVAE_NET_MH] > 0, true, sp, fused, st, nullptr, plan);
    }
    const float kls = S.kl_active ? sp->kl_coeff / S.Bg : 0.0f;
    InputSeed ss;
    if (seed_sampler) {
        ss.kind = 2;
        memset(&ss.s, 0, sizeof(ss.s));
        ss.s.te_out = w + wte->act.back(); ss.s.ldte = ldo_te;
        ss.s.eps = w + c->W.eps;
        ss.s.dz = w + wte->dz.back(); ss.s.ldz = ldo_te;
        ss.s.c0 = Db; ss.s.Z = Z; ss.s.rows = rows;
        ss.s.kl_scale = kls;
        if (learned_prior) {
            ss.s.mu_p = w + wpr->act.back(); ss.s.ldmp = PR->layers.back().n_out_pad;
            ss.s.dz_p = w + wpr->dz.back(); ss.s.ldzp = PR->layers.back().n_out_pad;
        }
    }
    CarriedWgrad carry;
    plan_backward_net(c, PVAE_NET_MD, S.rows_pad, true, true, sp, fused, st, nullptr, plan, &ss,
                      seed_sampler ? &carry : nullptr, nullptr,
                      /* hidden-layer pairs of the encoder follow the decoder's first-layer pair: */
                      !learned_prior && TE->layers.size() >= 3);
    if (!seed_sampler) {
        const int rows_pad = S.rows_pad;
        push(plan, [=]() -> int {
            int rc = 0;                        // z feeds the helper too: its input gradient joins the decoder's
            if (helper && (rc = add_cols_launch(w + wmd->d_in + Db, MD->layers[0].ld, rows, Z, w + wmh->d_in + Db, MH->layers[0].ld,
                                                nullptr, 0, nullptr, 0, nullptr, 0, st)))
                return rc;
            if (!sphere) return reparam_bwd_launch(c, rows, 0, kls, st);
            hipLaunchKernelGGL(sphere_bwd_kernel, dim3((rows_pad + 3) / 4), dim3(256), 0, st, w + wmd->d_in,
                               MD->layers[0].ld, Db, w + wte->act.back(), TE->layers.back().n_out_pad, w + c->W.eps,
                               w + wte->dz.back(), TE->layers.back().n_out_pad, rows, rows_pad, Z, kls, sphere_norm);
            HIP_TRY(hipGetLastError());
            return 0;
        });
    }
    // the learned prior mean trains through the KL term only (its output gradient was written beside the
    // encoder's by the sampler backward above); no input gradient
    if (learned_prior) plan_backward_net(c, PVAE_NET_PR, S.rows_pad, true, false, sp, fused, st, nullptr, plan);
    plan_backward_net(c, PVAE_NET_TE, S.rows_pad, true, false, sp, fused, st, fold, plan, nullptr, nullptr, &carry);
}

extern "C" {

int pvae_forward_backward(pvae_ctx* c, int phase, int32_t rows, const pvae_step_params* sp, const float* eps,
                          float* loss_out, int flags, void* stream) {
    const bool backward = !(flags & PVAE_FLAG_NO_BACKWARD);
    const bool fused = (flags & PVAE_FLAG_FUSED_ADAM) != 0;
    int rc = check_step(c, phase, rows, sp, backward, fused);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (backward && fused) params_touched(c, st);
    StepShape S;
    if ((rc = step_shape(c, phase, rows, sp, loss_out, backward, S))) return rc;
    if ((rc = run_forward(c, phase, rows, sp, eps, backward, S, st))) return rc;
    Plan plan;
    plan_backward(c, phase, rows, sp, backward, fused, S, st, plan);
    c->pending_adam = c->held_adam = AdamSeg();
    for (Stage& s : plan)
        if ((rc = s.run())) { c->pending_adam = c->held_adam = AdamSeg(); return rc; }
    if ((rc = flush_pending_adam(c, st))) return rc;
    if (loss_out && !backward) {
        hipLaunchKernelGGL(finalize_loss_kernel, dim3(1), dim3(64), 0, st, S.lf);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int pvae_forward_seed(pvae_ctx* c, int phase, int32_t rows, const pvae_step_params* sp, const float* eps,
                      void* stream) {
    int rc = check_step(c, phase, rows, sp, true, false);
    if (rc) return rc;
    StepShape S;
    if ((rc = step_shape(c, phase, rows, sp, nullptr, true, S))) return rc;
    return run_forward(c, phase, rows, sp, eps, true, S, (hipStream_t)stream);
}

int pvae_backward_stage(pvae_ctx* c, int phase, int32_t rows, const pvae_step_params* sp, int stage,
                        float* loss_out, void* stream, int64_t* ready_offset, int64_t* ready_count,
                        int* ready_net, int* num_stages) {
    int rc = check_step(c, phase, rows, sp, true, false);
    if (rc) return rc;
    StepShape S;
    if ((rc = step_shape(c, phase, rows, sp, loss_out, true, S))) return rc;
    Plan plan;
    plan_backward(c, phase, rows, sp, true, false, S, (hipStream_t)stream, plan);
    if (num_stages) *num_stages = (int)plan.size();
    if (stage < 0 || stage >= (int)plan.size()) return fail(-1, "stage %d outside [0, %d)", stage, (int)plan.size());
    if (ready_offset) *ready_offset = plan[stage].ready_off;
    if (ready_count) *ready_count = plan[stage].ready_cnt;
    if (ready_net) *ready_net = plan[stage].net;
    return plan[stage].run();
}

int pvae_backward_plan(pvae_ctx* c, int phase, const pvae_step_params* sp, int64_t* offset, int64_t* count, int* net,
                       int max, int* num_stages) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!sp) return fail(-1, "null step params");
    if (phase != PVAE_PHASE_WORLD && phase != PVAE_PHASE_JOINT) return fail(-1, "unknown phase %d", phase);
    StepShape S;
    if ((rc = step_shape(c, phase, 1, sp, nullptr, true, S))) return rc;
    Plan plan;                                  // (stages are closures: building them launches nothing and changes no state)
    plan_backward(c, phase, 1, sp, true, false, S, (hipStream_t) nullptr, plan);
    if (num_stages) *num_stages = (int)plan.size();
    for (int k = 0; k < (int)plan.size() && k < max; ++k) {
        if (offset) offset[k] = plan[k].ready_off;
        if (count) count[k] = plan[k].ready_cnt;
        if (net) net[k] = plan[k].net;
    }
    return 0;
}

int pvae_adam_segment(pvae_ctx* c, int net, int64_t offset, int64_t count, const pvae_step_params* sp,
                      void* stream) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!sp) return fail(-1, "null step params");
    if (!c->grads || !c->m || !c->v) return fail(-2, "grads / Adam moment arenas not bound");
    if (net < 0 || net >= PVAE_NUM_NETS) return fail(-1, "bad net id %d", net);
    const NetLayout& N = c->L.net[net];
    if (offset < N.off || count < 0 || offset + count > N.off + N.count || (offset & 3) || (count & 3))
        return fail(-1, "segment [%lld, +%lld) not inside net %d or not float4-aligned", (long long)offset,
                    (long long)count, net);
    if (count == 0) return 0;
    params_touched(c, (hipStream_t)stream);
    return adam_flat_launch(c->params + offset, c->grads + offset, c->m + offset, c->v + offset, count / 4, adam_scalars(sp, net),
                            (hipStream_t)stream);
}

int pvae_adam(pvae_ctx* c, int net_mask, const pvae_step_params* sp, void* stream) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!sp) return fail(-1, "null step params");
    if (!c->grads || !c->m || !c->v) return fail(-2, "grads / Adam moment arenas not bound");
    params_touched(c, (hipStream_t)stream);
    for (int n = 0; n < PVAE_NUM_NETS; ++n) {
        if (!(net_mask & (1 << n))) continue;
        const NetLayout& N = c->L.net[n];
        if (N.count == 0) continue;            // (segments are multiples of 64 floats)
        if ((rc = adam_flat_launch(c->params + N.off, c->grads + N.off, c->m + N.off, c->v + N.off, N.count / 4,
                                   adam_scalars(sp, n), (hipStream_t)stream)))
            return rc;
    }
    return 0;
}

// A training step that reads the demonstration set directly: nothing is staged; `dx` tells run_forward /
// plan_backward_net to use the gathered first layers.  on == false: the step takes the staging launch as before.  The scope
// ends the direct step on every return path: the input panels do not hold this minibatch, so a later pvae_forward_backward
// must stage first.
struct DirectStep {
    pvae_ctx* c;
    const bool on;
    DirectStep(pvae_ctx* c_, int phase, int64_t first_window, int rows, const pvae_step_params* sp, bool fused)
        : c(c_), on(check_ready(c_, true) == 0 && enter(c_, phase, first_window, rows, sp, fused)) {}
    DirectStep(const DirectStep&) = delete;
    ~DirectStep() {
        if (on) { c->dx.on = false; c->staged_rows = 0; }
    }
    static bool enter(pvae_ctx* c, int phase, int64_t first_window, int rows, const pvae_step_params* sp, bool fused);
};
bool DirectStep::enter(pvae_ctx* c, int phase, int64_t first_window, int rows, const pvae_step_params* sp, bool fused) {
    c->dx.on = false;
    if (!sp || !c->states || first_window < 0 || rows < 1 || rows > c->L.cfg.max_batch || first_window + rows > c->n_windows) return false;
    if (phase != PVAE_PHASE_WORLD && phase != PVAE_PHASE_JOINT) return false;
    if (!direct_ok(c, phase, rows, sp, fused)) return false;
    const RowMap rm = row_map(c, first_window, rows);
    if (!rm.seg) return false;             // (more than one episode jump inside the minibatch, or no host copy of window_row)
    // The encoder's gathered operand [s_t | s_{t+1}] ends inside a 16-byte chunk when 2 Db is no multiple of 4; the chunk's
    // tail is what follows the row in memory -- the next row, data -- and meets W's zero pad columns (QGather).  Behind the
    // LAST row of `states` lies no data: the bytes are readable (data_slack), but a NaN or Inf pattern there times zero is
    // NaN, and the hidden ReLU then drops that window's whole first layer.  The one minibatch of an epoch that holds this
    // window stages its panels instead (same bits).
    if (phase == PVAE_PHASE_JOINT && ((2 * c->L.cfg.dim_body) & 3)) {
        const int64_t last0 = (int64_t)rm.b0 + (rm.q1 < rows ? rm.q1 : rows) - 1;
        const int64_t last1 = rm.q1 < rows ? (int64_t)rm.b1 + (rows - rm.q1) - 1 : -1;
        if ((last0 > last1 ? last0 : last1) + 2 >= c->n_rows) return false;
    }
    c->dx.on = true;
    c->dx.rm = rm;
    memset(&c->next_touch, 0, sizeof(c->next_touch));
    c->staged_rows = rows;
    c->staged_rows_f = rows;
    c->pf.valid = false;
    c->next_stage.rows_pad = 0;
    c->next_carried = false;
    return true;
}

// Gather prefetch (lookahead 1): this minibatch is already in the alternate panels when the previous step's last launch carried
// its gather -- the panels flip --, else it is gathered now; then the gather of the next one is armed for this step's last
// launch.  `can`: the step has a launch that carries it (the one that folds the loss).
static int prefetch_begin(pvae_ctx* c, bool can, int64_t first_window, int rows, int64_t next_first, int next_rows, void* stream) {
    if (can && c->pf.valid && c->pf.first == first_window && c->pf.rows == rows && c->pf.states == c->states) {
        flip_stage_panels(c);
        c->staged_rows = rows;
        c->staged_rows_f = rows;
    } else if (int rc = pvae_gather(c, first_window, rows, stream)) {
        return rc;
    }
    c->pf.valid = false;
    c->next_stage.rows_pad = 0;
    c->next_carried = false;
    if (can && next_rows > 0 && next_rows <= c->L.cfg.max_batch && next_first >= 0 && next_first + next_rows <= c->n_windows)
        c->next_stage = stage_args(c, next_first, nullptr, nullptr, next_rows, true, 1, true);
    return 0;
}
// ... and after the step: what the alternate panels hold now
static void prefetch_end(pvae_ctx* c, bool ok, int64_t next_first, int next_rows) {
    if (ok && c->next_carried) {
        c->pf.valid = true; c->pf.first = next_first; c->pf.rows = next_rows; c->pf.states = c->states;
    }
    c->next_stage.rows_pad = 0;
    c->next_carried = false;
}
// 1: the next training step on this binding would read the demonstration set directly (same arguments as the step)
int pvae_direct_active(pvae_ctx* c, int phase, int32_t rows, const pvae_step_params* sp, int fused) {
    if (!c || !sp) return fail(-1, "null argument");
    if (check_ready(c, true)) return 0;
    return c->states && direct_ok(c, phase, rows, sp, fused != 0) ? 1 : 0;
}

int pvae_dp_train_step(pvae_ctx* c, int phase, int64_t first_window, int32_t rows, const pvae_step_params* sp,
                       const float* eps, float* loss_out, int64_t next_first, int32_t next_rows, void* stream) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!c->comm && !(c->p2p.open && (c->exchange_mode == PVAE_EXCHANGE_P2P || c->exchange_mode == PVAE_EXCHANGE_P2P_PUSH ||
                                      c->exchange_mode == PVAE_EXCHANGE_LOCAL)))
        return fail(-2, "no communicator (pvae_comm_init) and no peer-mapped exchange (pvae_p2p_open + pvae_comm_mode)");
    if (!sp) return fail(-1, "null step params");
    if (!c->grads || !c->m || !c->v) return fail(-2, "grads / Adam moment arenas not bound");
    if (phase != PVAE_PHASE_WORLD && phase != PVAE_PHASE_JOINT) return fail(-1, "unknown phase %d", phase);
    hipStream_t st = (hipStream_t)stream;
    params_touched(c, st);
    const bool learned_prior = !c->L.net[PVAE_NET_PR].layers.empty();
    const bool helper = !c->L.net[PVAE_NET_MH].layers.empty() && sp->adam_t[PVAE_NET_MH] > 0;
    // (the helper trains with the decoder in the joint phase and, with lookahead > 1, in the world phase too: plan_backward_unrolled)
    const int nets[4] = {(phase == PVAE_PHASE_WORLD && c->W.L == 1) || !helper ? -1 : PVAE_NET_MH,
                         phase == PVAE_PHASE_WORLD ? PVAE_NET_WM : PVAE_NET_MD,
                         phase == PVAE_PHASE_WORLD ? -1 : (learned_prior ? PVAE_NET_PR : PVAE_NET_TE),
                         phase == PVAE_PHASE_WORLD || !learned_prior ? -1 : PVAE_NET_TE};      // backward order
    c->bucket_bytes_now = auto_bucket_bytes(c, phase);
    hipStream_t cs = (c->bucket_bytes_now > 0 && c->comm_stream) ? c->comm_stream : st;
    int n_events = 0;
    auto join = [&]() -> int {                 // later work on the caller's stream sees the updated parameters
        if (cs == st) return 0;
        HIP_TRY(hipEventRecord(c->comm_done, cs));
        HIP_TRY(hipStreamWaitEvent(st, c->comm_done, 0));
        return 0;
    };
    if (rows == 0) {
        // empty shard of a ragged last global batch: contribute zeros, apply the same update
        for (int n : nets) {
            if (n < 0) continue;
            const NetLayout& N = c->L.net[n];
            HIP_TRY(hipMemsetAsync(c->grads + N.off, 0, (size_t)N.count * sizeof(float), st));
            for (const Bucket& b : exchange_buckets(c, n))
                if ((rc = exchange_bucket(c, n, b, sp, st, cs, n_events))) return rc;
        }
        return join();
    }
    // gather prefetch as in pvae_train_step_prefetch: this rank's next shard rides in the last launch
    const DirectStep direct(c, phase, first_window, rows, sp, false);
    const bool can = c->W.L == 1 && c->pair_launch && loss_out != nullptr && c->states != nullptr;
    if (direct.on) {
        // (first layers gather their rows themselves: no staging launch; the last launch pre-touches the next shard's rows)
        if (loss_out) plan_touch(c, next_first, next_rows);
    } else if ((rc = prefetch_begin(c, can, first_window, rows, next_first, next_rows, stream))) {
        return rc;
    }
    if ((rc = check_step(c, phase, rows, sp, true, false))) return rc;
    StepShape S;
    if ((rc = step_shape(c, phase, rows, sp, loss_out, true, S))) return rc;
    if ((rc = run_forward(c, phase, rows, sp, eps, true, S, st))) return rc;
    Plan plan;
    plan_backward(c, phase, rows, sp, true, false, S, st, plan);
    // A stack's slices become final last layer first.  Each time the finished region reaches down
    // to the start of the next exchange bucket, that bucket goes to the exchange stream (reduce over
    // the ranks, then Adam on it) while this stream keeps launching the rest of the backward pass;
    // the parameters a bucket's Adam rewrites are not read again in this step (the fused path
    // rewrites them in the same launches).  The caller's stream rejoins at the end.
    std::vector<Bucket> bk[PVAE_NUM_NETS];
    size_t next_bk[PVAE_NUM_NETS] = {};
    int64_t low[PVAE_NUM_NETS];
    for (int n : nets)
        if (n >= 0) { bk[n] = exchange_buckets(c, n); low[n] = c->L.net[n].off + c->L.net[n].count; }
    for (Stage& s : plan) {
        if ((rc = s.run())) break;
        if (s.ready_cnt <= 0 || s.net < 0) continue;
        const int n = s.net;
        if (s.ready_off + s.ready_cnt != low[n]) {
            rc = fail(-2, "backward plan finished [%lld, +%lld) of stack %d out of order", (long long)s.ready_off,
                      (long long)s.ready_cnt, n);
            break;
        }
        low[n] = s.ready_off;
        while (!rc && next_bk[n] < bk[n].size() && bk[n][next_bk[n]].off >= low[n])
            rc = exchange_bucket(c, n, bk[n][next_bk[n]++], sp, st, cs, n_events);
        if (rc) break;
    }
    if (!rc)
        for (int n : nets)
            if (n >= 0 && next_bk[n] != bk[n].size()) rc = fail(-2, "stack %d left the backward pass unfinished", n);
    const int jrc = join();
    if (!rc) rc = jrc;
    prefetch_end(c, !rc, next_first, next_rows);
    return rc;
}

int pvae_train_step(pvae_ctx* c, int phase, int64_t first_window, int32_t rows, const pvae_step_params* sp,
                    const float* eps, float* loss_out, void* stream) {
    if (!c) return fail(-1, "null ctx");
    if (!c->states) return fail(-2, "dataset not bound");
    const DirectStep direct(c, phase, first_window, rows, sp, true);
    if (!direct.on)
        if (int rc = pvae_gather(c, first_window, rows, stream)) return rc;
    return pvae_forward_backward(c, phase, rows, sp, eps, loss_out, PVAE_FLAG_FUSED_ADAM, stream);
}

int pvae_train_step_prefetch(pvae_ctx* c, int phase, int64_t first_window, int32_t rows, const pvae_step_params* sp,
                             const float* eps, float* loss_out, int64_t next_first, int32_t next_rows, void* stream) {
    if (!c) return fail(-1, "null ctx");
    if (!c->states) return fail(-2, "dataset not bound");
    const DirectStep direct(c, phase, first_window, rows, sp, true);
    if (direct.on) {
        // (first layers gather their rows themselves: no staging launch; the last launch pre-touches the next minibatch's rows)
        if (loss_out) plan_touch(c, next_first, next_rows);
        return pvae_forward_backward(c, phase, rows, sp, eps, loss_out, PVAE_FLAG_FUSED_ADAM, stream);
    }
    const bool can = c->W.L == 1 && c->pair_launch && loss_out != nullptr;   // the carrier is the folding launch
    int rc = prefetch_begin(c, can, first_window, rows, next_first, next_rows, stream);
    if (rc) return rc;
    rc = pvae_forward_backward(c, phase, rows, sp, eps, loss_out, PVAE_FLAG_FUSED_ADAM, stream);
    prefetch_end(c, !rc, next_first, next_rows);
    return rc;
}

}  // extern "C"
