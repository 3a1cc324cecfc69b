// pvae_net.hip -- one stack of PhysicsVAE: its forward launches, the sampler between encoder and decoder, and its backward
// plan with the deferred-Adam hand-over between launches.  The step (pvae_step.hip), the unroll (pvae_lookahead.hip) and
// rollout / autograd / the PPO hooks (pvae_infer.hip) are built from these.
#include "pvae_internal.h"

// The motor decoder's helper (rmt:833-835): a_hat[:, :Da] += range * h, h = the helper stack's tanh output.  The decoder's
// output layer has already left a second copy of its own a_hat in the action columns of the world model's input panel.
__global__ void __launch_bounds__(256)
helper_add_kernel(float* __restrict__ a_hat, int lda, const float* __restrict__ h, int ldh, float* __restrict__ wm_in,
                  int ldw, int col0, int rows, int Da, float range) {
    const int total = rows * Da;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / Da, c = idx - r * Da;
        const float v = __fmaf_rn(range, h[(size_t)r * ldh + c], a_hat[(size_t)r * lda + c]);
        a_hat[(size_t)r * lda + c] = v;
        if (wm_in) wm_in[(size_t)r * ldw + col0 + c] = v;
    }
}
int helper_add_launch(pvae_ctx* c, int rows, int64_t row0, int64_t wm_row0, hipStream_t st) {
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action;
    const int ld_md = c->L.net[PVAE_NET_MD].layers.back().n_out_pad, ld_mh = c->L.net[PVAE_NET_MH].layers.back().n_out_pad;
    const int ld_wm = c->L.net[PVAE_NET_WM].layers[0].ld;
    hipLaunchKernelGGL(helper_add_kernel, dim3(grid1d(rows * Da, 256)), dim3(256), 0, st,
                       c->ws + c->W.net[PVAE_NET_MD].act.back() + row0 * ld_md, ld_md,
                       c->ws + c->W.net[PVAE_NET_MH].act.back() + row0 * ld_mh, ld_mh,
                       c->ws + c->W.net[PVAE_NET_WM].in + wm_row0 * ld_wm, ld_wm, Db, rows, Da, c->L.cfg.mh_range);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Reparameterisation sampler + KL-to-N(0,I) partial sums (rmt:734-740, 795-800; tpv:384-389):
//   z = mu + eps * exp(0.5 logvar)      written into md_in[:, Db:Db+Z]
//   partial[b] = sum -0.5 (1 + logvar - mu^2 - exp(logvar))     (finalize scales by 1/B)
__global__ void __launch_bounds__(256)
reparam_kernel(const float* __restrict__ te_out, int ldte, const float* __restrict__ eps_in,
               float* __restrict__ eps_used, float* __restrict__ md_in, int ld_md, int Db, int Z, int rows,
               int rows_pad, int noise, unsigned long long seed, unsigned long long offset,
               float* __restrict__ partial, float* __restrict__ z_dense,
               const float* __restrict__ mu_p = nullptr, int ldmp = 0) {
    float acc = 0.f;
    const int total = rows_pad * Z;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / Z, c = idx - r * Z;
        float z = 0.f, e = 0.f;
        if (r < rows) {
            const float mu = te_out[(size_t)r * ldte + c];
            const float lv = te_out[(size_t)r * ldte + Z + c];
            if (noise) e = eps_in ? eps_in[(size_t)r * Z + c] : philox_normal(seed, offset, r, c);
            z = __fmaf_rn(e, expf(0.5f * lv), mu);
            if (mu_p) {               // KL(N(mu, s^2) || N(mu_p, 1)), oracle/refpath.py PRIORS
                const float d = mu - mu_p[(size_t)r * ldmp + c];
                acc += 0.5f * (expf(lv) + d * d - 1.0f - lv);
            } else {
                acc += -0.5f * (1.0f + lv - mu * mu - expf(lv));
            }
        }
        md_in[(size_t)r * ld_md + Db + c] = z;
        eps_used[(size_t)r * Z + c] = e;
        if (z_dense && r < rows) z_dense[(size_t)r * Z + c] = z;      // caller's [rows][Z] copy (rollout path)
    }
    const float s = block_sum_256(acc);
    if (threadIdx.x == 0 && partial) partial[blockIdx.x] = s;
}

// PVAE_PRIOR_HYPERSPHERE (oracle/refpath.py PRIORS; rmt:810-814, tpv:404-407): the encoder's Z outputs
// e are projected onto the unit sphere, z = e / max(|e|, 1e-12) (F.normalize), z goes to the decoder;
// the prior sample of this forward is u = n / max(|n|, 1e-12), n ~ N(0, I) (the supplied eps, or Philox),
// and the KL slot of the loss is mean_i <z_i, u_i>.  One wave per row.
//   md_in[:, Db:Db+Z] = z     eps_used = u (zeros without noise)     partial[b] = sum over its rows of <z, u>
__global__ void __launch_bounds__(256)
sphere_kernel(const float* __restrict__ te_out, int ldte, const float* __restrict__ eps_in,
              float* __restrict__ eps_used, float* __restrict__ md_in, int ld_md, int Db, int Z, int rows,
              int rows_pad, int noise, unsigned long long seed, unsigned long long offset,
              float* __restrict__ partial, float* __restrict__ z_dense, int normalize) {
    // normalize == 0: latent_prior_type = False (rmt:815-816) -- z = e, nothing sampled, no loss term
    if (!normalize) noise = 0;
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;
    float dot = 0.f;
    if (r < rows_pad) {
        float e2 = 0.f, n2 = 0.f;
        for (int c = lane; c < Z; c += 64) {
            if (r < rows) {
                const float e = te_out[(size_t)r * ldte + c];
                e2 += e * e;
                if (noise) {
                    const float nz = eps_in ? eps_in[(size_t)r * Z + c] : philox_normal(seed, offset, r, c);
                    n2 += nz * nz;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { e2 += __shfl_xor(e2, o, 64); n2 += __shfl_xor(n2, o, 64); }
        const float ie = normalize ? 1.0f / fmaxf(sqrtf(e2), 1e-12f) : 1.0f, in_ = 1.0f / fmaxf(sqrtf(n2), 1e-12f);
        for (int c = lane; c < Z; c += 64) {
            float z = 0.f, u = 0.f;
            if (r < rows) {
                z = te_out[(size_t)r * ldte + c] * ie;
                if (noise) u = (eps_in ? eps_in[(size_t)r * Z + c] : philox_normal(seed, offset, r, c)) * in_;
                dot += z * u;
                if (z_dense) z_dense[(size_t)r * Z + c] = z;
            }
            md_in[(size_t)r * ld_md + Db + c] = z;
            eps_used[(size_t)r * Z + c] = u;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    }
    if (lane == 0) part[wave] = dot;
    __syncthreads();
    if (threadIdx.x == 0 && partial) partial[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// Multi-tensor Adam over one contiguous arena segment (data-parallel path, after the
// gradient all-reduce).  28 B/param of traffic: read p,g,m,v, write p,m,v.
__global__ void __launch_bounds__(256)
adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                 float* __restrict__ v, long long n4, AdamScalars s) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += gridDim.x * 256ll) {
        v4f pp = reinterpret_cast<v4f*>(p)[i];
        const v4f gg = reinterpret_cast<const v4f*>(g)[i];
        v4f mm = reinterpret_cast<v4f*>(m)[i];
        v4f vv = reinterpret_cast<v4f*>(v)[i];
        adam_update4(gg, pp, mm, vv, s);
        reinterpret_cast<v4f*>(p)[i] = pp;
        reinterpret_cast<v4f*>(m)[i] = mm;
        reinterpret_cast<v4f*>(v)[i] = vv;
    }
}

int adam_flat_launch(float* p, const float* g, float* m, float* v, long long n4, const AdamScalars& s, hipStream_t st) {
    hipLaunchKernelGGL(adam_flat_kernel, dim3(grid1d(n4, 2048)), dim3(256), 0, st, p, g, m, v, n4, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Rollout-batch forward layer (rows <= 4; rmt:742-771 runs at B = 1 inside the 30 Hz control
// loop): out[r][n] = act(sum_k x[r][k] W[n][k] + b[n]).  One wave per output feature streams its
// weight row once with float4 loads (all 256 CUs busy: n_out/4 blocks of 4 waves), the R input
// rows come from L1/L2, lanes split K and combine with a shuffle tree.  HBM/L2-bound: 4 B per
// weight, ~2 flops per byte -- the tile kernels would push the same panel through 32 workgroups.
template <int R>
__global__ void __launch_bounds__(256)
gemv_rows_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ W, int ldw,
                 const float* __restrict__ bias, float* __restrict__ out, int ldo, int K, int relu,
                 float* __restrict__ out2, int ld2, int off2, int n2, int n_valid) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const float* wrow = W + (size_t)n * ldw;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
        const v4f wv = *reinterpret_cast<const v4f*>(wrow + k);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const v4f xv = *reinterpret_cast<const v4f*>(x + (size_t)r * ldx + k);
            acc[r] = fmaf(wv.x, xv.x, fmaf(wv.y, xv.y, fmaf(wv.z, xv.z, fmaf(wv.w, xv.w, acc[r]))));
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float v = acc[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) {
            v += bias[n];
            v = (relu > 1 && n >= n_valid) ? 0.f : act_apply(v, relu);
            out[(size_t)r * ldo + n] = v;
            if (out2 && n < n2) out2[(size_t)r * ld2 + off2 + n] = v;
        }
    }
}

int forward_net(pvae_ctx* c, int n, int rows_pad, hipStream_t st, const FwdTail& tail, int64_t row0) {
    const NetLayout& N = c->L.net[n];
    const float* x = c->ws + c->W.net[n].in + row0 * N.layers[0].ld;
    int ldx = N.layers[0].ld;
    for (const Layer& l : N.layers) {
        float* out = c->ws + c->W.net[n].act[l.index] + row0 * l.n_out_pad;
        const int rows = (int)c->staged_rows_f;
        // (category 5: the narrow layers that run on 16x16 tiles -- another kernel, gemm_splitk_reg16_kernel)
        const int ps = g_prof.begin(forward_uses_16x16(pad32(rows), l.n_out_pad) && rows > 4 ? 5 : 0,
                                    2.0 * c->staged_rows_f * l.n_in * l.n_out, st);
        if (rows <= 4 && !tail.mse) {            // rollout batch: stream W once over all CUs
            float* o2 = (l.last && tail.out2) ? tail.out2 : nullptr;
            const dim3 grid(l.n_out_pad / 4), block(256);
#define PVAE_GEMV(R)                                                                                        \
    PVAE_LAUNCH((gemv_rows_kernel<R>), grid, block, st, x, ldx, c->params + l.w_off, l.ld,           \
                       c->params + l.b_off, out, l.n_out_pad, l.ld, l.act, o2, tail.ld2, tail.off2, tail.n2, l.n_out)
            if (rows == 1) PVAE_GEMV(1);
            else if (rows == 2) PVAE_GEMV(2);
            else PVAE_GEMV(4);
#undef PVAE_GEMV
            HIP_TRY(hipGetLastError());
        } else if (l.last && tail.mse) {
            EpiMse e = *tail.mse;
            e.out = out; e.ldo = l.n_out_pad; e.bias = c->params + l.b_off;
            HIP_TRY(gemm_forward_epi(x, ldx, c->params + l.w_off, l.ld, rows_pad, l.n_out_pad, l.ld, e, st));
        } else {
            EpiBiasAct e{out, l.n_out_pad, c->params + l.b_off, l.act};
            e.n_valid = l.n_out;
            if (l.last && tail.out2) { e.out2 = tail.out2; e.ld2 = tail.ld2; e.off2 = tail.off2; e.n2 = tail.n2; }
            if (l.index == 0 && tail.xs0 && tail.pro0)
                HIP_TRY(gemm_forward_pro_gather(*tail.xs0, c->params + l.w_off, l.ld, rows_pad, l.n_out_pad, l.ld, e, *tail.pro0, st));
            else if (l.index == 0 && tail.xs0 && tail.cols0)
                HIP_TRY(gemm_forward_pro_gather(*tail.xs0, c->params + l.w_off, l.ld, rows_pad, l.n_out_pad, l.ld, e, *tail.cols0, st));
            else if (l.index == 0 && tail.xs0)
                HIP_TRY(gemm_forward_gather(*tail.xs0, c->params + l.w_off, l.ld, rows_pad, l.n_out_pad, l.ld, e, st));
            else if (l.index == 0 && tail.pro0)
                HIP_TRY(gemm_forward_pro(x, ldx, c->params + l.w_off, l.ld, rows_pad, l.n_out_pad, l.ld, e, *tail.pro0, st));
            else
                HIP_TRY(gemm_forward_epi(x, ldx, c->params + l.w_off, l.ld, rows_pad, l.n_out_pad, l.ld, e, st));
        }
        g_prof.end(ps, st);
        x = out;
        ldx = l.n_out_pad;
    }
    return 0;
}

// the pending deferred-Adam segment, handed to the launch that is about to go out
// What the launch that is about to go out carries.  A hidden-layer pair absorbs the 28 B/param of a 1024x1024 update
// at ~1 us; a launch with little work of its own (a stack's first / last layer) is as long as the update it
// carries (the sampler-seed pair: 9.6 us, 40 MB).  So such a NARROW launch passes a big pending segment on (it stays
// `held` for the next WIDE launch) and takes only what is small; wide launches and the step's last launch take all.
constexpr long long kBigAdamSeg = 150000;                       // float4 elements (a 1024x256 layer: 65.8 K, 1024x1024: 262 K)
AdamPair take_pending(pvae_ctx* c, int how) {
    AdamPair p;
    if (how == kTakeSmall && c->pending_adam.n4 >= kBigAdamSeg && c->held_adam.n4 <= 0) {
        c->held_adam = c->pending_adam;                         // pass it on
        c->pending_adam = AdamSeg();
        return p;
    }
    if (how == kTakeSmall && c->held_adam.n4 > 0) {             // still holding one: take the recent one if it is small
        if (c->pending_adam.n4 < kBigAdamSeg) { p.s[0] = c->pending_adam; c->pending_adam = AdamSeg(); }
        else { p.s[0] = c->held_adam; c->held_adam = c->pending_adam; c->pending_adam = AdamSeg(); }   // (two big ones: oldest goes)
        return p;
    }
    p.s[0] = c->held_adam;
    p.s[1] = c->pending_adam;
    if (p.s[0].n4 <= 0) { p.s[0] = p.s[1]; p.s[1] = AdamSeg(); }
    c->held_adam = AdamSeg();
    c->pending_adam = AdamSeg();
    return p;
}
// nothing left to carry them: their own launches
int flush_pending_adam(pvae_ctx* c, hipStream_t st) {
    const AdamPair p = take_pending(c);
    int rc = 0;
    for (const AdamSeg& a : p.s)
        if (a.n4 > 0 && (rc = adam_flat_launch(a.p, a.g, a.m, a.v, a.n4, a.s, st))) break;
    return rc;
}

// ---- the backward plan of one stack at lookahead 1 ---------------------------------------------------------------
// What the schedules below launch: the stack's BwdNet on row block 0, and what this call of plan_backward_net was told.
struct NetPass {
    BwdNet bn;
    int rows_pad;
    bool input_grad, fused;
    bool can_defer;                // a stored gradient's update may ride in a later launch (can_defer_adam)
    bool wide_follows_layer0;
    bool dx0;                      // direct step: the weight gradient of layer 0 contracts over the gathered input (XSrc), not over a staged panel
    XSrc xs0;
    LossFinal fold;                // executed by the blocks of the launch planned `with_fold`
    InputSeed seed;
    bool has_dgrad(int i) const { return i > 0 || input_grad; }
    int dgrad(int i) const;
    int wgrad(int i, int j, bool with_fold) const;
    int wgrad_pair10(bool with_fold) const;
    int wgrad_last0(bool with_fold) const;
};

// The seeded input gradient of layer 0: only the input columns the seed consumes are contracted (a 32-aligned window
// of W_0), and the seed's epilogue counts its columns from the window's first one.
template <class Seed>
struct SeededW0 { const float* W; int width; Seed epi; };
template <class Seed>
static SeededW0<Seed> seeded_w0(const BwdNet& bn, Seed e, int cols) {
    const SeedWindow sw = seed_window(e.c0, cols);
    e.c0 -= sw.lo;
    return SeededW0<Seed>{bn.c->params + bn.layer(0).w_off + sw.lo, sw.width, e};
}

int NetPass::dgrad(int i) const {
    if (i > 0 || seed.kind == 0) return bn.dgrad(i, 0, rows_pad);
    const Layer& l = bn.layer(0);
    const int ps = g_prof.begin(1, 2.0 * bn.rowsf * bn.dgrad_cols(0) * l.n_out, bn.st);
    if (seed.kind == 1) {
        const auto s = seeded_w0(bn, seed.a, seed.a.n);
        HIP_TRY(gemm_dgrad_epi(bn.dz(0), l.n_out_pad, s.W, l.ld, rows_pad, s.width, l.n_out_pad, s.epi, bn.st));
    } else {
        const auto s = seeded_w0(bn, seed.s, seed.s.Z);
        HIP_TRY(gemm_dgrad_epi(bn.dz(0), l.n_out_pad, s.W, l.ld, rows_pad, s.width, l.n_out_pad, s.epi, bn.st));
    }
    g_prof.end(ps, bn.st);
    return 0;
}

// wgrad of layer i, optionally fused with the dgrad of layer j (j < 0: alone).  In a fused pair
// that is not the step's last launch the gradient is stored and Adam deferred to workgroups of
// the next weight-gradient launch (AdamSeg); every launch carries whatever is pending.
int NetPass::wgrad(int i, int j, bool with_fold) const {
    pvae_ctx* c = bn.c;
    const Layer& l = bn.layer(i);
    const int last = bn.last();
    // (j == i: the launch also reads W_i, so the update MUST wait for the next one)
    const bool defer = can_defer && j >= 0 && (!with_fold || j == i);
    // (narrow launches -- a stack's last and first layer -- hand a big pending update on to the next hidden-layer
    //  pair of the step, when there is one: take_pending)
    const bool narrow = j == i && !with_fold && ((i == last && last >= 2) || (i == 0 && wide_follows_layer0));
    auto go = [&](auto e) -> int {
        if (with_fold) e.loss = fold;
        const AdamPair ad = take_pending(c, narrow ? kTakeSmall : kTakeAll);
        if (j >= 0) {
            const Layer& d = bn.layer(j);
            const int pp = g_prof.begin(3, 2.0 * bn.rowsf * ((double)l.n_in * l.n_out + (double)bn.dgrad_cols(j) * d.n_out), bn.st);
            if (j == 0 && seed.kind == 2) {
                const auto s = seeded_w0(bn, seed.s, seed.s.Z);
                if (dx0)                  // (i == 0 too: the decoder's first layer, X = [s_t | z] gathered)
                    HIP_TRY(gemm_bwd_pair_epi_gather(bn.dz(0), d.n_out_pad, s.W, d.ld, rows_pad, s.width, d.n_out_pad, s.epi, bn.dz(i),
                                                     l.n_out_pad, xs0, l.n_out_pad, l.ld, rows_pad, e, bn.st, &ad));
                else
                    HIP_TRY(gemm_bwd_pair_epi(bn.dz(0), d.n_out_pad, s.W, d.ld, rows_pad, s.width, d.n_out_pad, s.epi, bn.dz(i),
                                              l.n_out_pad, bn.x(i), l.ld, l.n_out_pad, l.ld, rows_pad, e, bn.st, &ad));
            } else {
                HIP_TRY(bn.wgrad_with_dgrad(i, rows_pad, bn.dgrad_args(j, 0, rows_pad), e, ad));
            }
            g_prof.end(pp, bn.st);
        } else {
            const int pw = g_prof.begin(2, 2.0 * bn.rowsf * l.n_in * l.n_out, bn.st);
            HIP_TRY(bn.wgrad(i, rows_pad, e, &ad));
            g_prof.end(pw, bn.st);
        }
        return 0;
    };
    // (with_grad_epi plus the deferring arm, spelt out: the code object holds this unit's kernels in the order in which
    //  the unit first names their launchers, and this is the order it has had -- docs/experiments.md, "Device code, byte for byte")
    if (!fused) return c->grad_accum ? go(bn.accum_epi(i)) : go(bn.store_epi(i));
    if (!defer) return go(bn.adam_epi(i));
    const int rc = go(bn.store_epi(i));
    if (rc == 0) c->pending_adam = bn.adam_seg(i);
    return rc;
}

// The step's last launch of a stack without input gradient: the loss finalisation, the pending update and the gather
// of the next minibatch ride in it.  One-behind schedule: layers 1 and 0 in one launch ...
int NetPass::wgrad_pair10(bool with_fold) const {
    pvae_ctx* c = bn.c;
    const Layer& l1 = bn.layer(1);
    const Layer& l0 = bn.layer(0);
    const int pw2 = g_prof.begin(2, 2.0 * bn.rowsf * ((double)l1.n_in * l1.n_out + (double)l0.n_in * l0.n_out), bn.st);
    const int rc = bn.with_grad_epi(1, fused, [&](auto e1) -> int {
        if (with_fold) e1.loss = fold;            // block 0 of the launch belongs to the first problem
        // the step's LAST launch also gathers the next minibatch into the alternate panels
        const bool carry = with_fold && c->next_stage.rows_pad > 0;
        const AdamPair ad = take_pending(c);
        HIP_TRY(gemm_wgrad_pair(bn.dz(1), l1.n_out_pad, bn.x(1), l1.ld, l1.n_out_pad, l1.ld, e1, bn.dz(0), l0.n_out_pad, bn.x(0),
                                l0.ld, l0.n_out_pad, l0.ld, bn.like(e1, 0), rows_pad, bn.st, carry ? &c->next_stage : nullptr, &ad));
        if (carry) c->next_carried = true;
        return 0;
    });
    g_prof.end(pw2, bn.st);
    return rc;
}
// ... same-layer schedule: layer 0 alone
int NetPass::wgrad_last0(bool with_fold) const {
    pvae_ctx* c = bn.c;
    const Layer& l0 = bn.layer(0);
    const int pw = g_prof.begin(2, 2.0 * bn.rowsf * l0.n_in * l0.n_out, bn.st);
    const int rc = bn.with_grad_epi(0, fused, [&](auto e0) -> int {
        if (with_fold) e0.loss = fold;
        const bool carry = with_fold && c->next_stage.rows_pad > 0;
        const AdamPair ad = take_pending(c);
        if (dx0) {                        // X gathered from the demonstration set: nothing was staged, nothing to stage
            HIP_TRY(gemm_wgrad_pair_gather(bn.dz(0), l0.n_out_pad, xs0, l0.n_out_pad, l0.ld, e0, rows_pad, bn.st, &ad,
                                           with_fold && c->next_touch.blocks > 0 ? &c->next_touch : nullptr));
            return 0;
        }
        HIP_TRY(gemm_wgrad_pair(bn.dz(0), l0.n_out_pad, bn.x(0), l0.ld, l0.n_out_pad, l0.ld, e0, (const float*)nullptr, 0,
                                (const float*)nullptr, 0, 0, l0.ld, e0, rows_pad, bn.st, carry ? &c->next_stage : nullptr, &ad));
        if (carry) c->next_carried = true;
        return 0;
    });
    g_prof.end(pw, bn.st);
    return rc;
}

// dz[last] must be filled.  Layer by layer, last to first: the input gradient of layer i reads
// W_i; a weight gradient of layer i with Adam in its epilogue overwrites W_i.  Two schedules:
//  * same layer (the default whenever the update can be deferred, and for the gradient-store path
//    of the data-parallel exchange): wgrad_i only stores its gradient, shares ONE horizontally
//    fused launch with dgrad_i, and Adam_i runs as extra workgroups of the next launch:
//        dgrad_L + wgrad_L | dgrad_{L-1} + wgrad_{L-1} + Adam_L | ... | wgrad_0 + Adam_1
//  * one behind (Adam in the epilogue; no gradient arena, PVAE_SAME_LAYER=0 / PVAE_DEFER_ADAM=0):
//    dgrad_{i-1} (needs dz_{i-1}, W_{i-1}) and wgrad_i (needs dz_i, x_i; writes W_i) are independent:
//        dgrad_L | dgrad_{L-1} + wgrad_L | ... | dgrad_1 + wgrad_2 | [dgrad_0] + wgrad_1 | wgrad_0
//    (without an input gradient the two last weight gradients share a launch).
// `fold`: the blocks of the stack's last launch execute NetPass::fold.
static void plan_dgrad_only(const NetPass& p, Plan& plan) {             // a frozen stack
    for (int i = p.bn.last(); i >= 0; --i)
        if (p.has_dgrad(i)) push(plan, [=] { return p.dgrad(i); });
}
static void plan_unpaired(const NetPass& p, bool fold, Plan& plan) {    // PVAE_PAIR=0: every contraction its own launch
    for (int i = p.bn.last(); i >= 0; --i) {
        if (p.has_dgrad(i)) push(plan, [=] { return p.dgrad(i); });
        const bool f = fold && i == 0;
        p.bn.ready(push(plan, [=] { return p.wgrad(i, -1, f); }), i, i);
    }
}
// Same-layer schedule: with the update deferred (or no update at all: gradient store for the
// data-parallel exchange) wgrad_i no longer writes W_i, so it shares a launch with dgrad_i
// instead of trailing one launch behind it:
//     dgrad_L + wgrad_L | dgrad_{L-1} + wgrad_{L-1} [+ Adam_L] | ... | wgrad_0 [+ Adam_1]
// The short first launch (K = output width) and the short last one (narrow layer 0) each get
// a partner of their own size, instead of a lone short launch at one end and two narrow
// problems in one launch at the other.
static void plan_same_layer(const NetPass& p, bool fold, Plan& plan) {
    for (int i = p.bn.last(); i >= 0; --i) {
        const bool f = fold && i == 0;
        if (p.has_dgrad(i)) p.bn.ready(push(plan, [=] { return p.wgrad(i, i, f); }), i, i);
        else p.bn.ready(push(plan, [=] { return p.wgrad_last0(f); }), 0, 0);
    }
}
// One behind.  A lone trailing weight gradient (`carry_out`, no fold) is handed to the next stack's plan, whose first
// input gradient (`carry_in`) it then shares a launch with.
static void plan_one_behind(const NetPass& p, bool fold, Plan& plan, CarriedWgrad* carry_out, const CarriedWgrad* carry_in) {
    const BwdNet bn = p.bn;
    const int last = bn.last(), rows_pad = p.rows_pad;
    if (p.has_dgrad(last)) {
        if (carry_in && carry_in->valid) {
            // the previous stack's trailing weight gradient rides with this stack's first input gradient
            const CarriedWgrad cw = *carry_in;
            const DgradArgs da = bn.dgrad_args(last, 0, rows_pad);
            Stage& sref = push(plan, [=] { return cw.run_with_dgrad(da); });
            sref.ready_off = cw.ready_off; sref.ready_cnt = cw.ready_cnt; sref.net = cw.net;
        } else {
            push(plan, [=] { return p.dgrad(last); });
        }
    }
    for (int i = last; i >= 0; --i) {
        const int j = i - 1;                       // dgrad_{i-1} rides with wgrad_i
        if (j >= 0 && p.has_dgrad(j)) {
            const bool f = fold && i == 0;
            bn.ready(push(plan, [=] { return p.wgrad(i, j, f); }), i, i);
        } else if (i == 1 && !p.has_dgrad(0)) {
            bn.ready(push(plan, [=] { return p.wgrad_pair10(fold); }), 0, 1);
            return;
        } else if (i == 0 && carry_out && !fold) {
            // hand the lone trailing weight gradient to the next stack's plan
            const bool fused = p.fused;
            carry_out->valid = true;
            bn.ready(*carry_out, 0, 0);
            carry_out->run_with_dgrad = [=](const DgradArgs& d) -> int {
                const Layer& l = bn.layer(0);
                const int pp = g_prof.begin(3, d.flops + 2.0 * bn.rowsf * l.n_in * l.n_out, bn.st);
                const AdamPair ad = take_pending(bn.c);
                // (Adam or store, never the accumulating form; spelt out for the kernel order, as in NetPass::wgrad)
                const hipError_t he = fused ? bn.wgrad_with_dgrad(0, rows_pad, d, bn.adam_epi(0), ad)
                                            : bn.wgrad_with_dgrad(0, rows_pad, d, bn.store_epi(0), ad);
                g_prof.end(pp, bn.st);
                if (he != hipSuccess) return fail(-10, "gemm_bwd_pair: %s", hipGetErrorString(he));
                return 0;
            };
        } else {
            const bool f = fold && i == 0;
            bn.ready(push(plan, [=] { return p.wgrad(i, -1, f); }), i, i);
        }
    }
}

void plan_backward_net(pvae_ctx* c, int n, int rows_pad, bool train, bool input_grad, const pvae_step_params* sp, bool fused,
                       hipStream_t st, const LossFinal* fold, Plan& plan, const InputSeed* seed, CarriedWgrad* carry_out,
                       const CarriedWgrad* carry_in, bool wide_follows_layer0) {
    NetPass p{BwdNet(c, n, sp, st), rows_pad, input_grad, fused, can_defer_adam(c, fused), wide_follows_layer0};
    p.bn.dx0_cols = n == PVAE_NET_WM ? c->L.cfg.dim_action : c->L.cfg.latent;
    p.dx0 = c->dx.on && train && n != PVAE_NET_PR;
    if (p.dx0) p.xs0 = xsrc_of(c, n, n == PVAE_NET_WM ? PVAE_PHASE_WORLD : PVAE_PHASE_JOINT, true, (int)c->staged_rows_f);
    memset(&p.fold, 0, sizeof(p.fold));
    if (fold) p.fold = *fold;
    if (seed) p.seed = *seed;
    if (!train) return plan_dgrad_only(p, plan);
    if (!c->pair_launch) return plan_unpaired(p, fold != nullptr, plan);
    if ((!fused || p.can_defer) && c->same_layer_pairs) return plan_same_layer(p, fold != nullptr, plan);
    plan_one_behind(p, fold != nullptr, plan, carry_out, carry_in);
}

// The sampler of the configured prior kind (rmt:795-819): reparam_kernel (N(mu, s^2); KL to N(0, I) or to
// the learned prior mean mu_p) or sphere_kernel (unit-sphere encoder).  `partial` may be null (rollout).
int sampler_grid(const pvae_ctx* c, int rows_pad) {
    if (c->L.cfg.prior_kind >= PVAE_PRIOR_HYPERSPHERE) return rows_pad / 4;
    const int Z = c->L.cfg.latent;
    return grid1d(rows_pad * Z, 64);
}
// Where the sampler's z goes: columns [Db, Db + Z) of the decoder's input panel -- or, for a decoder that reads s_t only
// (motor_decoder_inputs = ["body"], rmt:822-829), of a side panel of the same shape: the code is still drawn, kept for
// pvae_read_tensor and priced by the KL term, but must not sit in the operand of the decoder's weight gradient (the
// weights of those columns are structural zeros and stay so because the operand is zero there).
int64_t z_panel(const pvae_ctx* c) {
    return c->L.cfg.md_inputs == PVAE_INPUT_BODY ? c->W.z_side : c->W.net[PVAE_NET_MD].in;
}
int launch_sampler(pvae_ctx* c, const float* te_out, int ldte, const float* eps, float* eps_used, float* md_in, int ld_md,
                   int rows, int rows_pad, int noise, unsigned long long seed, unsigned long long offset, float* partial,
                   float* z_dense, const float* mu_p, int ldmp, hipStream_t st) {
    const int Db = c->L.cfg.dim_body, Z = c->L.cfg.latent;
    md_in += z_panel(c) - c->W.net[PVAE_NET_MD].in;
    if (c->L.cfg.prior_kind >= PVAE_PRIOR_HYPERSPHERE) {
        hipLaunchKernelGGL(sphere_kernel, dim3((rows_pad + 3) / 4), dim3(256), 0, st, te_out, ldte, eps, eps_used, md_in,
                           ld_md, Db, Z, rows, rows_pad, noise, seed, offset, partial, z_dense,
                           c->L.cfg.prior_kind == PVAE_PRIOR_HYPERSPHERE ? 1 : 0);
    } else {
        hipLaunchKernelGGL(reparam_kernel, dim3(sampler_grid(c, rows_pad)), dim3(256), 0, st, te_out, ldte, eps, eps_used,
                           md_in, ld_md, Db, Z, rows, rows_pad, noise, seed, offset, partial, z_dense, mu_p, ldmp);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The sampler runs as the prologue of the decoder's first-layer launch (ProSampler) when that launch is the 32x32-tile
// kernel and the prior is the reference's default: joint training steps at lookahead 1, more than 4 rows.
bool sampler_folds(const pvae_ctx* c, int rows) {
    const NetLayout& MD = c->L.net[PVAE_NET_MD];
    return c->fold_sampler && c->pair_launch && c->W.L == 1 && c->L.cfg.prior_kind == PVAE_PRIOR_ZERO_MEAN &&
           c->L.cfg.md_inputs != PVAE_INPUT_BODY &&
           c->L.net[PVAE_NET_PR].layers.empty() && c->L.cfg.latent <= ProSampler::kMaxZ && c->L.cfg.latent % 4 == 0 &&
           rows > 4 &&
           MD.layers.size() > 1 && forward_pro_ok(pad32(rows), MD.layers[0].n_out_pad);
}

// ---- first layers on the demonstration set (XSrc) ------------------------------------------------------------
// The gathered input of stack `net` in the step in flight.  `with_s1`: the second column block is part of the operand
// (weight gradients; forward layers on 64-row tiles) -- false when a Pro patch of the launch supplies those columns.
XSrc xsrc_of(const pvae_ctx* c, int net, int phase, bool with_s1, int rows) {
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action, Z = c->L.cfg.latent;
    XSrc x;
    memset(&x, 0, sizeof(x));
    x.s0 = c->states; x.rm = c->dx.rm; x.ld0 = Db; x.rows = rows;
    x.zero = c->ws + c->W.zero;
    x.s1 = x.zero;
    if (net == PVAE_NET_TE) { x.n0 = 2 * Db; return x; }               // [s_t | s_{t+1}]: one run of 2 Db floats of `states`
    x.n0 = Db;
    if (!with_s1) return x;
    if (net == PVAE_NET_MD) {                                          // [s_t | z]: z where the sampler stored it
        x.s1 = c->ws + c->W.net[PVAE_NET_MD].in + Db; x.ind1 = 0; x.ld1 = c->L.net[PVAE_NET_MD].layers[0].ld; x.n1 = Z;
    } else if (phase == PVAE_PHASE_WORLD) {                            // [s_t | a_t]
        x.s1 = c->actions; x.ind1 = 1; x.ld1 = Da; x.n1 = Da;
    } else {                                                           // [s_t | a_hat]: the decoder's output panel
        x.s1 = c->ws + c->W.net[PVAE_NET_MD].act.back(); x.ind1 = 0; x.ld1 = c->L.net[PVAE_NET_MD].layers.back().n_out_pad; x.n1 = Da;
    }
    return x;
}
