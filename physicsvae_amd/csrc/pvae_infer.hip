// pvae_infer.hip -- rollout and inference (pvae_infer*, pvae_mlp_forward), the autograd entry points on one stack or on the
// sampler (pvae_net_forward / _backward, pvae_reparam / _backward), and what the PPO learner step runs of a stack (ppo_*).
#include "pvae_internal.h"

// dst[rows_pad][ld] = zero-padded copy of dense src[rows][n]; only the columns [c0, c0 + nw) of src are taken (the
// window a first layer with an input subset reads: whatever the caller put in the other columns meets structural-zero
// weights, and the panel keeps exact zeros there like a staged one)
__global__ void __launch_bounds__(256)
pad_copy_kernel(const float* __restrict__ src, int n, int rows, float* __restrict__ dst, int ld, int rows_pad, int c0, int nw) {
    const int total = rows_pad * ld;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / ld, c = idx - r * ld;
        dst[idx] = (r < rows && c < n && c >= c0 && c < c0 + nw) ? src[(size_t)r * n + c] : 0.f;
    }
}

// Output gradient of one stack from a caller's dy (pvae_net_backward; autograd of rmt:773-853): dz[r][c] = dy[r][c] *
// act'(y[r][c]) with y the recomputed output panel (act 0: linear output layer, the derivative is 1; the helper's tanh:
// 1 - y^2).  Written over ALL of [rows_pad][ld]: pad rows and pad columns get zeros, so that nothing an earlier call
// left in them reaches a contraction.
__global__ void __launch_bounds__(256)
net_seed_kernel(const float* __restrict__ dy, int n, int rows, const float* __restrict__ y, int ld, int rows_pad, int act,
                float* __restrict__ dz) {
    const int total = rows_pad * ld;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / ld, c = idx - r * ld;
        float g = 0.f;
        if (r < rows && c < n) {
            g = dy[(size_t)r * n + c];
            if (act) g *= act_grad(y[idx], act);
        }
        dz[idx] = g;
    }
}

// Backward of the sampler on its own (pvae_reparam_backward; autograd of rmt:734-740 and, per prior kind, 795-816), no
// KL term: dense mu_logvar / d_mu_logvar [rows][ldte], dz / eps_used [rows][Z].  One wave per row.
//   N(mu, s^2) kinds:   z = mu + eps exp(lv / 2)      dmu = dz, dlv = dz eps exp(lv / 2) / 2  (noise = 0: z = mu, dlv = 0)
//   hypersphere:        z = e / max(|e|, 1e-12)      de = (dz - z <z, dz>) / max(|e|, 1e-12)
//   none (False):       z = e                        de = dz
__global__ void __launch_bounds__(256)
sampler_bwd_kernel(const float* __restrict__ mu_logvar, int ldte, const float* __restrict__ eps_used,
                   const float* __restrict__ dz, int rows, int Z, int kind, int noise, float* __restrict__ d_ml) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* e = mu_logvar + (size_t)r * ldte;
    const float* g = dz + (size_t)r * Z;
    float* d = d_ml + (size_t)r * ldte;
    if (kind == PVAE_PRIOR_HYPERSPHERE) {
        sphere_bwd_row(e, g, Z, lane, d);                          // (pvae_internal.h: shared with the fused PPO step)
    } else if (kind == PVAE_PRIOR_NONE) {
        for (int c = lane; c < Z; c += 64) d[c] = g[c];
    } else {
        for (int c = lane; c < Z; c += 64) {
            d[c] = g[c];
            d[Z + c] = noise ? g[c] * eps_used[(size_t)r * Z + c] * 0.5f * expf(0.5f * e[Z + c]) : 0.f;
        }
    }
}

// Rollout forward with fewer launches (pvae_infer at <= 4 rows): the layer kernel assembles its R input
// rows in LDS itself, so the staging launch, the sampler launch and the copy-out launches disappear --
// 7 launches for observation -> action (TE 3, MD 4 at the trainer's default sizes) instead of 9, 10 with
// the world model's prediction instead of 14.  The input of a layer is
//   kind 0: rows of a padded activation panel (hidden layers)
//   kind 1: the caller's dense observation rows obs[r][0:Ka]                       (first encoder layer)
//   kind 2: [obs[r][0:Ka] | z_r],  z = mu + eps * exp(logvar / 2) from the encoder's output   (first decoder layer:
//           the sampler of rmt:734-740 runs here; workgroup 0 also records z and the draws)
//   kind 3: [obs[r][0:Ka] | src_b[r][0:Kb]]                                        (first world-model layer: a_hat)
//   kinds 4 / 5: [obs[r][0:Ka] | e_r] resp. [obs | e_r / |e_r|], e = the encoder's Z outputs (latent_prior_type False /
//           hypersphere_uniform: what sphere_kernel computes on the training path)
// One wave per output feature streams its weight row once (as gemv_rows_kernel); rows >= `rows` of the
// R-row template are computed on zeros and never stored.
struct RolloutIn {
    int kind;
    const float* a; int lda, Ka;      // panel (kind 0: Ka = padded width) or dense observation
    const float* b; int ldb, Kb;      // kind 2: encoder output [mu | logvar] (Kb = Z); kind 3: second source
    const float* eps; int noise;      // kind 2: supplied draws [rows][Z] or null (Philox) / noise off
    unsigned long long seed, offset;
    float* z_out; float* eps_used;    // kind 2, written by workgroup 0 (z_out may be null)
    float* keep;                      // kind 1: workgroup 0 copies the observation rows here ([rows][Ka]; may be null)
};
template <int R>
__global__ void __launch_bounds__(256)
gemv_rollout_kernel(RolloutIn in, int rows, const float* __restrict__ W, int ldw, const float* __restrict__ bias,
                    float* __restrict__ out, int ldo, int K, int relu, float* __restrict__ out2, int ld2, int n2,
                    int n_valid, const float* __restrict__ ls) {
    extern __shared__ __attribute__((aligned(16))) float xs[];         // [R][K], K = ld of the layer (multiple of 64)
    const int tid = threadIdx.x;
    // this wave's weight row: the first 1024 columns are requested BEFORE the input rows are assembled,
    // so that the two memory latencies of a layer (inputs, weights) overlap instead of adding up
    const int n = blockIdx.x * 4 + (tid >> 6);
    const int lane = tid & 63;
    const float* wrow = W + (size_t)n * ldw;
    v4f wpre[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = lane * 4 + 256 * j;
        wpre[j] = k < K ? *reinterpret_cast<const v4f*>(wrow + k) : v4f{0.f, 0.f, 0.f, 0.f};
    }
    if (in.kind == 0) {                   // hidden layers: whole padded panel rows, 16 bytes per load
        const int kq = K >> 2;
        for (int i = tid; i < R * kq; i += 256) {
            const int r = i / kq, k = (i - r * kq) * 4;
            *reinterpret_cast<v4f*>(xs + r * K + k) =
                r < rows ? *reinterpret_cast<const v4f*>(in.a + (size_t)r * in.lda + k) : v4f{0.f, 0.f, 0.f, 0.f};
        }
    }
    for (int i = tid; in.kind != 0 && i < R * K; i += 256) {
        const int r = i / K, k = i - r * K;
        float v = 0.f;
        if (r < rows) {
            if (k < in.Ka) {
                v = in.a[(size_t)r * in.lda + k];
                if (in.kind == 1 && in.keep && blockIdx.x == 0) in.keep[(size_t)r * in.Ka + k] = v;
            } else if (k < in.Ka + in.Kb) {
                const int j = k - in.Ka;
                if (in.kind == 2) {
                    const float mu = in.b[(size_t)r * in.ldb + j], lv = in.b[(size_t)r * in.ldb + in.Kb + j];
                    float e = 0.f;
                    if (in.noise) e = in.eps ? in.eps[(size_t)r * in.Kb + j] : philox_normal(in.seed, in.offset, r, j);
                    v = mu + e * expf(0.5f * lv);
                    if (blockIdx.x == 0) {
                        if (in.z_out) in.z_out[(size_t)r * in.Kb + j] = v;
                        in.eps_used[(size_t)r * in.Kb + j] = e;
                    }
                } else if (in.kind == 3) {
                    v = in.b[(size_t)r * in.ldb + j];
                } else if (in.kind == 4) {          // latent_prior_type False: the encoder's outputs are the code
                    v = in.b[(size_t)r * in.ldb + j];
                    if (blockIdx.x == 0) {
                        if (in.z_out) in.z_out[(size_t)r * in.Kb + j] = v;
                        in.eps_used[(size_t)r * in.Kb + j] = 0.f;
                    }
                } else if (in.kind == 5) {          // hypersphere: z = e / max(|e|, 1e-12) (sphere_kernel)
                    float e2 = 0.f;
                    for (int q = 0; q < in.Kb; ++q) { const float e = in.b[(size_t)r * in.ldb + q]; e2 += e * e; }
                    v = in.b[(size_t)r * in.ldb + j] * (1.0f / fmaxf(sqrtf(e2), 1e-12f));
                    if (blockIdx.x == 0) {
                        float u = 0.f;
                        if (in.noise) {             // the prior sample of this forward, recorded only
                            float n2 = 0.f, mine = 0.f;
                            for (int q = 0; q < in.Kb; ++q) {
                                const float nz = in.eps ? in.eps[(size_t)r * in.Kb + q] : philox_normal(in.seed, in.offset, r, q);
                                n2 += nz * nz;
                                if (q == j) mine = nz;
                            }
                            u = mine * (1.0f / fmaxf(sqrtf(n2), 1e-12f));
                        }
                        if (in.z_out) in.z_out[(size_t)r * in.Kb + j] = v;
                        in.eps_used[(size_t)r * in.Kb + j] = u;
                    }
                }
            }
        }
        xs[i] = v;
    }
    __syncthreads();
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = lane * 4 + 256 * j;
        if (k < K) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const v4f xv = *reinterpret_cast<const v4f*>(xs + r * K + k);
                acc[r] = fmaf(wpre[j].x, xv.x, fmaf(wpre[j].y, xv.y, fmaf(wpre[j].z, xv.z, fmaf(wpre[j].w, xv.w, acc[r]))));
            }
        }
    }
    for (int k = lane * 4 + 1024; k < K; k += 256) {
        const v4f wv = *reinterpret_cast<const v4f*>(wrow + k);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const v4f xv = *reinterpret_cast<const v4f*>(xs + r * K + k);
            acc[r] = fmaf(wv.x, xv.x, fmaf(wv.y, xv.y, fmaf(wv.z, xv.z, fmaf(wv.w, xv.w, acc[r]))));
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float v = acc[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0 && r < rows) {
            v += bias[n];
            v = (relu > 1 && n >= n_valid) ? 0.f : act_apply(v, relu);
            out[(size_t)r * ldo + n] = v;
            if (out2 && n < n2) {
                out2[(size_t)r * ld2 + n] = v;
                if (ls) out2[(size_t)r * ld2 + n2 + n] = ls[n];       // AppendLogStd (rmt:160-206): [a_hat | log_std]
            }
        }
    }
}

// logits[r][n .. 2n) = log_std[0 .. n) for the staged inference path (AppendLogStd, rmt:160-206)
__global__ void __launch_bounds__(256)
append_logstd_kernel(float* __restrict__ logits, int ld, int n, int rows, const float* __restrict__ ls) {
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < rows * n; idx += gridDim.x * 256) {
        const int r = idx / n, c = idx - r * n;
        logits[(size_t)r * ld + n + c] = ls[c];
    }
}

// A stack of dense Linear layers on caller-owned row-major weights W_i[n_out][n_in] (any row stride, any
// alignment), hidden activation act_apply(code), linear output: pvae_mlp_forward.  One wave per output feature
// and chunk of R rows; made for the value branch at rollout batch sizes (rmt:846-853: 2*Db -> 256 -> 256 -> 1).
template <int R>
__global__ void __launch_bounds__(256)
gemv_dense_kernel(const float* __restrict__ x, int ldx, int rows, const float* __restrict__ W, int ldw,
                  const float* __restrict__ bias, int K, int N, int act, float* __restrict__ out, int ldo) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, r0 = blockIdx.y * R;
    if (n >= N) return;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float w = W[(size_t)n * ldw + k];
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r0 + r < rows) acc[r] = fmaf(w, x[(size_t)(r0 + r) * ldx + k], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float v = acc[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0 && r0 + r < rows) out[(size_t)(r0 + r) * ldo + n] = act_apply(v + (bias ? bias[n] : 0.f), act);
    }
}

// pvae_infer / pvae_infer_logits: the action lands in a_hat[r * ld_a + 0 .. Da) and, when `log_std` is given, the
// decoder's log-std vector behind it (AppendLogStd rmt:160-206: logits = [a_hat | log_std]).
// option "rollout_fused" = 0: rollout calls of <= 4 rows go through the staged path (A/B)
static int infer_impl(pvae_ctx* c, const float* obs, int32_t rows, const float* eps, int noise, uint64_t rng_seed,
                      uint64_t rng_offset, float* a_hat, int ld_a, const float* log_std, float* s2_hat, float* z_out,
                      void* stream) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!obs || !a_hat) return fail(-1, "obs / a_hat is null");
    if (ld_a < c->L.cfg.dim_action * (log_std ? 2 : 1)) return fail(-1, "row stride %d of the action buffer is too small", ld_a);
    hipStream_t st = (hipStream_t)stream;
    if (rows < 1 || rows > c->L.cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, c->L.cfg.max_batch);
    const bool helper = !c->L.net[PVAE_NET_MH].layers.empty();          // (its term joins between decoder and world model: staged path)
    const bool fused_rollout = g_rollout_fused && !helper;
    if (rows <= 4 && fused_rollout) {
        // latency path of the control loop (rmt:742-771 at B = 1): no staging / sampler / copy launches, the
        // input panels of a staged training minibatch are not touched
        const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action, Z = c->L.cfg.latent;
        float* w = c->ws;
        // (staged_rows / staged_rows_f stay as they are: a staged training minibatch remains valid, and
        //  forward_net picks its kernels by staged_rows_f)
        auto run_net = [&](int n, RolloutIn first, float* out2, int ld2, int n2, const float* ls) -> int {
            const NetLayout& N = c->L.net[n];
            RolloutIn in = first;
            for (const Layer& l : N.layers) {
                float* out = w + c->W.net[n].act[l.index];
                const dim3 grid(l.n_out_pad / 4), block(256);
                const size_t shm = (size_t)(rows <= 1 ? 1 : rows == 2 ? 2 : 4) * l.ld * sizeof(float);
                float* o2 = l.last ? out2 : nullptr;
                const int ps = g_prof.begin(0, 2.0 * rows * l.n_in * l.n_out, st);
#define PVAE_ROLL(R)                                                                                                  \
    hipLaunchKernelGGL((gemv_rollout_kernel<R>), grid, block, shm, st, in, (int)rows, c->params + l.w_off, l.ld,      \
                       c->params + l.b_off, out, l.n_out_pad, l.ld, l.act, o2, ld2, n2, l.n_out, l.last ? ls : nullptr)
                if (rows == 1) PVAE_ROLL(1);
                else if (rows == 2) PVAE_ROLL(2);
                else PVAE_ROLL(4);
#undef PVAE_ROLL
                g_prof.end(ps, st);
                HIP_TRY(hipGetLastError());
                memset(&in, 0, sizeof(in));
                in.kind = 0; in.a = out; in.lda = l.n_out_pad; in.Ka = l.n_out_pad;
            }
            return 0;
        };
        RolloutIn te;
        memset(&te, 0, sizeof(te));
        te.kind = 1; te.a = obs; te.lda = 2 * Db; te.Ka = 2 * Db;
        te.keep = w + c->W.obs_keep;       // what a deferred read of this forward (mu / logvar / prediction / value) re-uses
        if ((rc = run_net(PVAE_NET_TE, te, nullptr, 0, 0, nullptr))) return rc;
        RolloutIn md;
        memset(&md, 0, sizeof(md));
        md.kind = c->L.cfg.prior_kind == PVAE_PRIOR_NONE ? 4 : c->L.cfg.prior_kind == PVAE_PRIOR_HYPERSPHERE ? 5 : 2;
        md.a = obs; md.lda = 2 * Db; md.Ka = Db;
        md.b = w + c->W.net[PVAE_NET_TE].act.back(); md.ldb = c->L.net[PVAE_NET_TE].layers.back().n_out_pad; md.Kb = Z;
        md.eps = eps; md.noise = noise ? 1 : 0; md.seed = rng_seed; md.offset = rng_offset;
        md.z_out = z_out; md.eps_used = w + c->W.eps;
        if ((rc = run_net(PVAE_NET_MD, md, a_hat, ld_a, Da, log_std))) return rc;
        if (s2_hat) {
            RolloutIn wm;
            memset(&wm, 0, sizeof(wm));
            wm.kind = 3; wm.a = obs; wm.lda = 2 * Db; wm.Ka = Db;
            wm.b = w + c->W.net[PVAE_NET_MD].act.back(); wm.ldb = c->L.net[PVAE_NET_MD].layers.back().n_out_pad; wm.Kb = Da;
            if ((rc = run_net(PVAE_NET_WM, wm, s2_hat, Db, Db, nullptr))) return rc;
        }
        return 0;
    }
    if ((rc = stage(c, 0, obs, nullptr, rows, false, st, 1))) return rc;
    c->staged_rows = 0;      // not a training batch
    const int rows_pad = pad32(rows);
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action, Z = c->L.cfg.latent;
    float* w = c->ws;
    const NetLayout& TE = c->L.net[PVAE_NET_TE];
    const NetLayout& MD = c->L.net[PVAE_NET_MD];
    const NetLayout& WM = c->L.net[PVAE_NET_WM];
    if ((rc = forward_net(c, PVAE_NET_TE, rows_pad, st))) return rc;
    // (the learned prior mean plays no part in the action: rmt:801-809 only records it)
    if ((rc = launch_sampler(c, w + c->W.net[PVAE_NET_TE].act.back(), TE.layers.back().n_out_pad, eps, w + c->W.eps,
                             w + c->W.net[PVAE_NET_MD].in, MD.layers[0].ld, rows, rows_pad, noise ? 1 : 0,
                             (unsigned long long)rng_seed, (unsigned long long)rng_offset, (float*)nullptr, z_out,
                             (const float*)nullptr, 0, st)))                 // z also lands in the caller's buffer
        return rc;
    (void)Z;
    // The decoder's output layer can write a second copy of a_hat: into the world model's input
    // panel when the prediction is wanted, else straight into the caller's buffer (row counts the
    // GEMV kernel covers exactly -- the control loop's B = 1 -- so no padded row is written).
    const bool direct = !helper && !s2_hat && (rows == 1 || rows == 2 || rows == 4);
    FwdTail md_tail;
    if (direct) {
        md_tail.out2 = a_hat; md_tail.ld2 = ld_a; md_tail.off2 = 0; md_tail.n2 = Da;
    } else {
        md_tail.out2 = w + c->W.net[PVAE_NET_WM].in; md_tail.ld2 = WM.layers[0].ld; md_tail.off2 = Db; md_tail.n2 = Da;
    }
    if ((rc = forward_net(c, PVAE_NET_MD, rows_pad, st, md_tail))) return rc;
    if (helper) {                              // rmt:833-835
        if ((rc = forward_net(c, PVAE_NET_MH, rows_pad, st))) return rc;
        if ((rc = helper_add_launch(c, rows, 0, 0, st))) return rc;
    }
    if (!direct && (rc = copy_cols_launch(w + c->W.net[PVAE_NET_MD].act.back(), MD.layers.back().n_out_pad, 0, a_hat, ld_a, 0,
                                          rows, Da, st)))
        return rc;
    if (log_std) {
        hipLaunchKernelGGL(append_logstd_kernel, dim3(8), dim3(256), 0, st, a_hat, ld_a, Da, rows, log_std);
        HIP_TRY(hipGetLastError());
    }
    if (s2_hat) {
        if ((rc = forward_net(c, PVAE_NET_WM, rows_pad, st))) return rc;
        return copy_cols_launch(w + c->W.net[PVAE_NET_WM].act.back(), WM.layers.back().n_out_pad, 0, s2_hat, Db, 0, rows, Db, st);
    }
    return 0;
}

// The opening of pvae_net_forward / pvae_net_backward: the stack's input panel = the zero-padded copy of the caller's dense rows
static int net_input(pvae_ctx* c, int net, const float* in, int rows, hipStream_t st) {
    const NetLayout& N = c->L.net[net];
    const int rows_pad = pad32(rows), ld = N.layers[0].ld;
    hipLaunchKernelGGL(pad_copy_kernel, dim3(grid1d(rows_pad * ld, 1024)), dim3(256), 0, st, in, N.n_in, rows,
                       c->ws + c->W.net[net].in, ld, rows_pad, N.layers[0].col0, N.layers[0].n_in);
    HIP_TRY(hipGetLastError());
    c->staged_rows = 0;     // the training panels are no longer a coherent batch
    c->staged_rows_f = rows;
    return 0;
}

// A borrowed context: a stack's backward plan run with another gradient destination.  The trainer's arena, its pending
// updates and its direct step are set aside and put back on every return path; grad_accum is false outside such a scope.
struct BorrowedCtx {
    pvae_ctx* c;
    float* const grads;
    const AdamSeg pending, held;
    const bool dx;
    BorrowedCtx(pvae_ctx* c_, float* grad_arena, bool accumulate)
        : c(c_), grads(c_->grads), pending(c_->pending_adam), held(c_->held_adam), dx(c_->dx.on) {
        c->grads = grad_arena;
        c->grad_accum = accumulate;
        c->pending_adam = c->held_adam = AdamSeg();
        c->dx.on = false;
    }
    BorrowedCtx(const BorrowedCtx&) = delete;
    ~BorrowedCtx() {
        c->grads = grads;
        c->grad_accum = false;
        c->pending_adam = pending;
        c->held_adam = held;
        c->dx.on = dx;
    }
};
// the trainer's per-layer plan of one stack with a gradient store (or accumulate) into `grad_arena` (arena layout) instead of Adam
static int backward_net_into(pvae_ctx* c, int net, int rows_pad, bool train, bool input_grad, float* grad_arena, bool accumulate,
                             hipStream_t st, int* launches) {
    const BorrowedCtx borrowed(c, grad_arena, accumulate);
    pvae_step_params sp;
    memset(&sp, 0, sizeof(sp));
    Plan plan;
    plan_backward_net(c, net, rows_pad, train, input_grad, &sp, false, st, nullptr, plan);
    for (Stage& s : plan) {
        if (int rc = s.run()) return rc;
        ++*launches;
    }
    return 0;
}

extern "C" {
int pvae_rollout_is_fused(void) { return g_rollout_fused ? 1 : 0; }

int pvae_infer(pvae_ctx* c, const float* obs, int32_t rows, const float* eps, int noise, uint64_t rng_seed,
               uint64_t rng_offset, float* a_hat, float* s2_hat, float* z_out, void* stream) {
    return infer_impl(c, obs, rows, eps, noise, rng_seed, rng_offset, a_hat, c ? c->L.cfg.dim_action : 0, nullptr, s2_hat,
                      z_out, stream);
}

int pvae_infer_logits(pvae_ctx* c, const float* obs, int32_t rows, const float* eps, int noise, uint64_t rng_seed,
                      uint64_t rng_offset, float* logits, int32_t ld_logits, const float* log_std, float* s2_hat,
                      float* z_out, void* stream) {
    return infer_impl(c, obs, rows, eps, noise, rng_seed, rng_offset, logits, ld_logits, log_std, s2_hat, z_out, stream);
}

int pvae_mlp_forward(const float* x, int32_t rows, int32_t ldx, int32_t n_layers, const float* const* W,
                     const float* const* bias, const int32_t* n_in, const int32_t* n_out, const int32_t* ldw,
                     int32_t act_kind, const int32_t* layer_acts, float* scratch, float* out, int32_t ld_out,
                     void* stream) {
    if (!x || !W || !n_in || !n_out || !ldw || !out) return fail(-1, "null argument");
    if (rows < 1 || n_layers < 1 || n_layers > 16) return fail(-1, "rows %d / layers %d out of range", rows, n_layers);
    const int out_code = (act_kind >> 8) & 0xff;                 // 1 + PVAE_ACT_* of the OUTPUT layer (0: linear)
    act_kind &= 0xff;
    if (act_kind < 0 || act_kind > PVAE_ACT_ELU) return fail(-1, "unknown act_kind %d", act_kind);
    if (out_code > PVAE_ACT_ELU + 1) return fail(-1, "unknown output activation %d", out_code - 1);
    for (int i = 0; layer_acts && i + 1 < n_layers; ++i)
        if (layer_acts[i] < 0 || layer_acts[i] > PVAE_ACT_LINEAR) return fail(-1, "unknown activation %d of layer %d", layer_acts[i], i);
    int wmax = 0;
    for (int i = 0; i + 1 < n_layers; ++i) wmax = n_out[i] > wmax ? n_out[i] : wmax;
    if (n_layers > 1 && !scratch) return fail(-1, "scratch (2 * rows * widest hidden layer floats) is null");
    hipStream_t st = (hipStream_t)stream;
    const float* in = x;
    int ldi = ldx;
    for (int i = 0; i < n_layers; ++i) {
        if (n_in[i] < 1 || n_out[i] < 1 || ldw[i] < n_in[i] || !W[i]) return fail(-1, "bad layer %d", i);
        if (i > 0 && n_in[i] != n_out[i - 1]) return fail(-1, "layer %d reads %d features, layer %d emits %d", i, n_in[i], i - 1, n_out[i - 1]);
        const bool last = i == n_layers - 1;
        float* o = last ? out : scratch + (size_t)(i & 1) * rows * wmax;
        const int ldo = last ? ld_out : wmax;
        const dim3 grid((n_out[i] + 3) / 4, (rows + 3) / 4);
        hipLaunchKernelGGL((gemv_dense_kernel<4>), grid, dim3(256), 0, st, in, ldi, (int)rows, W[i], (int)ldw[i],
                           bias ? bias[i] : (const float*)nullptr, (int)n_in[i], (int)n_out[i],
                           last ? out_code : (layer_acts ? (layer_acts[i] == PVAE_ACT_LINEAR ? 0 : layer_acts[i] + 1) : act_kind + 1), o, ldo);
        HIP_TRY(hipGetLastError());
        in = o;
        ldi = ldo;
    }
    return 0;
}

int pvae_net_forward(pvae_ctx* c, int net, const float* in, int32_t rows, float* out, void* stream) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (net < 0 || net >= PVAE_NUM_NETS) return fail(-1, "bad net id %d", net);
    if (!in || !out) return fail(-1, "in / out is null");
    if (rows < 1 || rows > c->L.cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, c->L.cfg.max_batch);
    hipStream_t st = (hipStream_t)stream;
    const NetLayout& N = c->L.net[net];
    if ((rc = net_input(c, net, in, rows, st))) return rc;
    if ((rc = forward_net(c, net, pad32(rows), st))) return rc;
    return copy_cols_launch(c->ws + c->W.net[net].act.back(), N.layers.back().n_out_pad, 0, out, N.n_out, 0, rows, N.n_out, st);
}

int pvae_reparam(pvae_ctx* c, const float* mu_logvar, int32_t rows, const float* eps, int noise, uint64_t rng_seed,
                 uint64_t rng_offset, float* z_out, void* stream) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!mu_logvar || !z_out) return fail(-1, "mu_logvar / z_out is null");
    if (rows < 1 || rows > c->L.cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, c->L.cfg.max_batch);
    hipStream_t st = (hipStream_t)stream;
    const int Z = c->L.cfg.latent;
    const int ld_md = c->L.net[PVAE_NET_MD].layers[0].ld;
    c->staged_rows = 0;
    const int ldte = c->L.cfg.prior_kind >= PVAE_PRIOR_HYPERSPHERE ? Z : 2 * Z;       // dense [rows][n_out of the encoder]
    // pad rows are not touched: `rows` doubles as rows_pad (the sphere kernel rounds its grid up itself)
    return launch_sampler(c, mu_logvar, ldte, eps, c->ws + c->W.eps, c->ws + c->W.net[PVAE_NET_MD].in, ld_md, rows, rows,
                          noise ? 1 : 0, (unsigned long long)rng_seed, (unsigned long long)rng_offset, (float*)nullptr,
                          z_out, (const float*)nullptr, 0, st);
}

int pvae_net_backward(pvae_ctx* c, int net, const float* in, int32_t rows, const float* dy, float* dx, float* grad,
                      int32_t accumulate, void* stream) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (net < 0 || net >= PVAE_NUM_NETS || c->L.net[net].layers.empty()) return fail(-1, "bad net id %d (or no such stack)", net);
    if (!in || !dy) return fail(-1, "in / dy is null");
    if (!dx && !grad) return fail(-1, "neither dx nor grad: nothing to compute");
    if (rows < 1 || rows > c->L.cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, c->L.cfg.max_batch);
    hipStream_t st = (hipStream_t)stream;
    const NetLayout& N = c->L.net[net];
    const NetWork& w = c->W.net[net];
    const Layer& last = N.layers.back();
    const int rows_pad = pad32(rows), ld = N.layers[0].ld;
    // recompute: the very launches of pvae_net_forward, so the panels hold what that forward computed
    if ((rc = net_input(c, net, in, rows, st))) return rc;
    if (rows <= 4 && rows < rows_pad) {       // GEMV path: the pad rows of the layer outputs are not written
        ZeroRows z{};
        z.r0 = rows; z.r1 = rows_pad;
        for (const Layer& l : N.layers) z.add(c->ws + w.act[l.index], l.n_out_pad, l.n_out_pad);
        if ((rc = zero_rows_launch(z, st))) return rc;
    }
    if ((rc = forward_net(c, net, rows_pad, st))) return rc;
    hipLaunchKernelGGL(net_seed_kernel, dim3(grid1d(rows_pad * last.n_out_pad, 1024)), dim3(256), 0, st, dy, N.n_out, rows,
                       c->ws + w.act.back(), last.n_out_pad, rows_pad, last.act, c->ws + w.dz.back());
    HIP_TRY(hipGetLastError());
    // the trainer's per-layer plan, gradient store (or accumulate) instead of Adam, into the caller's buffer
    int launches = 0;
    if ((rc = backward_net_into(c, net, rows_pad, grad != nullptr, dx != nullptr, grad ? grad - N.off : c->grads, accumulate != 0,
                                st, &launches)))
        return rc;
    return dx ? copy_cols_launch(c->ws + w.d_in, ld, 0, dx, N.n_in, 0, rows, N.n_in, st) : 0;
}

int pvae_reparam_backward(pvae_ctx* c, const float* mu_logvar, const float* eps_used, const float* dz, int32_t rows,
                          int noise, float* d_mu_logvar, void* stream) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!mu_logvar || !dz || !d_mu_logvar) return fail(-1, "mu_logvar / dz / d_mu_logvar is null");
    const int kind = c->L.cfg.prior_kind;
    if (noise && kind < PVAE_PRIOR_HYPERSPHERE && !eps_used) return fail(-1, "eps_used is null with noise on");
    if (rows < 1 || rows > c->L.cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, c->L.cfg.max_batch);
    const int Z = c->L.cfg.latent;
    const int ldte = kind >= PVAE_PRIOR_HYPERSPHERE ? Z : 2 * Z;
    hipLaunchKernelGGL(sampler_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, mu_logvar, ldte,
                       eps_used, dz, rows, Z, kind, noise ? 1 : 0, d_mu_logvar);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// what the fused PPO learner step (pvae_ppo.hip) runs of this unit: a stack's forward on the panels as they are, the
// sampler into the decoder's input panel, and a stack's backward plan with a gradient store into `grad_arena` -- the
// launches of pvae_infer / pvae_net_backward without their copies, seed launches and recomputed forward
// ---------------------------------------------------------------------------------------
void ppo_enter(pvae_ctx* c, int rows) {
    c->staged_rows = 0;          // the training panels are no longer a coherent batch
    c->staged_rows_f = rows;
    c->pf.valid = false;
    c->dx.on = false;
}

int ppo_forward_net(pvae_ctx* c, int net, int rows, hipStream_t st, int* launches) {
    const int rc = forward_net(c, net, pad32(rows), st);
    if (rc == 0) *launches += (int)c->L.net[net].layers.size();
    return rc;
}

int ppo_sampler(pvae_ctx* c, const float* eps, int rows, int noise, uint64_t seed, uint64_t offset, hipStream_t st,
                int* launches) {
    const NetLayout& TE = c->L.net[PVAE_NET_TE];
    // the sphere prior's sample reaches neither the action nor the PPO loss (rmt:810-814 records it): nothing is drawn,
    // whatever the caller passed, and the draws that come back are zeros -- as under latent_prior_type False
    if (c->L.cfg.prior_kind == PVAE_PRIOR_HYPERSPHERE) noise = 0;
    const int rc = launch_sampler(c, c->ws + c->W.net[PVAE_NET_TE].act.back(), TE.layers.back().n_out_pad, eps,
                                  c->ws + c->W.eps, c->ws + c->W.net[PVAE_NET_MD].in, c->L.net[PVAE_NET_MD].layers[0].ld, rows,
                                  pad32(rows), noise ? 1 : 0, (unsigned long long)seed, (unsigned long long)offset,
                                  (float*)nullptr, (float*)nullptr, (const float*)nullptr, 0, st);
    if (rc == 0) ++*launches;
    return rc;
}

int ppo_backward_net(pvae_ctx* c, int net, int rows, bool train, bool input_grad, float* grad_arena, hipStream_t st,
                     int* launches) {
    return backward_net_into(c, net, pad32(rows), train, input_grad, grad_arena, false, st, launches);
}
