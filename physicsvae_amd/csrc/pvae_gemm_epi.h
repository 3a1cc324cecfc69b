// pvae_gemm_epi.h -- epilogues: what a contraction body does with a finished tile (activation, loss seeds, gradient store, Adam).
#pragma once
#include "pvae_gemm_common.h"
#include "pvae_gemm_src.h"
#include "pvae_adam.h"

namespace pvae {
// ---------------------------------------------------------------------------------------
// epilogues: (q, p, 4 consecutive p values)
// ---------------------------------------------------------------------------------------
// sum over a block of 256 or 512 threads (fixed order: deterministic)
__device__ inline float block_sum_256(float v, float* scratch) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
    if (blockDim.x > 256) s += (scratch[4] + scratch[5]) + (scratch[6] + scratch[7]);
    return s;
}

// Hidden-layer activation (get_activation_fn rmt:30-46 via gen_layers' act_hidden, tpv:180-192):
// internal codes 0 linear, 1 relu (the trainer's "act_fn"), 2 tanh, 3 sigmoid, 4 elu (alpha 1).  The backward
// pass needs only the layer's OUTPUT a: relu' = [a > 0], tanh' = 1 - a^2, sigmoid' = a (1 - a), elu' = a > 0 ? 1 : a + 1.
__device__ inline float act_apply(float x, int act) {
    switch (act) {
        case 1: return fmaxf(x, 0.f);
        case 2: return tanhf(x);
        case 3: return 1.f / (1.f + expf(-x));
        case 4: return x > 0.f ? x : expm1f(x);
        default: return x;
    }
}
__device__ inline float act_grad(float a, int act) {
    switch (act) {
        case 2: return 1.f - a * a;
        case 3: return a * (1.f - a);
        case 4: return a > 0.f ? 1.f : a + 1.f;
        default: return 1.f;
    }
}

struct EpiBiasAct {           // forward layer: out = act(acc + bias)
    float* out;
    int ldo;
    const float* bias;        // may be null
    int act;                  // act_apply code (0: linear output layer)
    float* out2 = nullptr;    // optional second destination for columns [0, n2): out2[q][off2 + p]
    int ld2 = 0, off2 = 0, n2 = 0;   // (motor-decoder output -> action columns of the world-model input)
    int n_valid = 1 << 30;    // real width of the layer: pad columns stay 0 also where act(0) != 0 (sigmoid),
                              // so that padding never reaches a weight gradient
    // operands of the epilogue that do not depend on the contraction are fetched BEFORE the main
    // loop (`preload`) and handed back at the end: their latency hides under the loop instead of
    // sitting between the last MFMA and the stores
    struct Pre { v4f b; };
    __device__ inline Pre preload(int, int p) const {
        Pre r;
        r.b = bias ? *reinterpret_cast<const v4f*>(bias + p) : v4f{0.f, 0.f, 0.f, 0.f};
        return r;
    }
    __device__ inline void operator()(int q, int p, v4f v, const Pre& pre) const {
        v += pre.b;
        if (act == 1) {
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f);
            v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        } else if (act > 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = p + e < n_valid ? act_apply(v[e], act) : 0.f;
        }
        store_stream(out + (size_t)q * ldo + p, v);
        if (out2) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p + e < n2) out2[(size_t)q * ld2 + off2 + p + e] = v[e];
        }
    }
    __device__ inline void finish(float*, int, int) const {}
};

// Output layer fused with nn.MSELoss (tm:99) and its gradient (world-model MSE tpv:411-414,
// cycle loss tpv:417-419): pred = acc + bias is stored, dz = grad_scale * (pred - target) for
// valid rows/columns (zeros elsewhere, so padded tiles stay inert downstream), and the
// workgroup's squared-error sum goes to partial[tile] (summed later in a fixed order).
struct EpiMse {
    float* out;
    int ldo;
    const float* bias;
    const float* target;
    int ldt;
    float* dz;                // may be null (forward only)
    int ldz;
    int rows, D;
    float grad_scale;
    float* partial;
    int l1;                   // 0: nn.MSELoss (sum d^2, grad 2d/n), 1: nn.L1Loss (sum |d|, grad sign(d)/n)
    float sq = 0.f;
    int tind = 0;                    // 1: the target of batch row q is row trm.at(q) of `target` (s_{t+1} read from `states`
    RowMap trm{};                    // where it lies, 4-byte aligned; columns >= D are never used)
    struct Pre { v4f b, t; };
    __device__ inline Pre preload(int q, int p) const {
        Pre r;
        r.b = bias ? *reinterpret_cast<const v4f*>(bias + p) : v4f{0.f, 0.f, 0.f, 0.f};
        const size_t tq = tind ? (size_t)trm.at(q < rows ? q : 0) : (size_t)q;
        r.t = *reinterpret_cast<const v4f*>(target + tq * ldt + (tind && p >= D ? 0 : p));
        return r;
    }
    __device__ inline void operator()(int q, int p, v4f v, const Pre& pre) {
        v += pre.b;
        *reinterpret_cast<v4f*>(out + (size_t)q * ldo + p) = v;
        const v4f t = pre.t;
        v4f g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool valid = q < rows && p + e < D;
            const float d = v[e] - t[e];
            if (valid) sq += l1 ? fabsf(d) : d * d;
            const float gd = l1 ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : d;
            g[e] = valid ? grad_scale * gd : 0.f;
        }
        if (dz) *reinterpret_cast<v4f*>(dz + (size_t)q * ldz + p) = g;
    }
    __device__ inline void finish(float* scratch, int tile, int tid) {
        const float s = block_sum_256(sq, scratch);
        if (tid == 0) partial[tile] = s;
    }
};

struct EpiMask {              // input gradient: out = acc * act'(a)   (relu: acc where a > 0, else 0)
    float* out;
    int ldo;
    const float* mask;        // activation a of the producing layer (its output), or null
    int ldm;
    int act = 1;              // act_grad code of that layer (0: linear, the gradient passes unchanged)
    struct Pre { v4f m; };
    __device__ inline Pre preload(int q, int p) const {
        Pre r;
        r.m = mask ? *reinterpret_cast<const v4f*>(mask + (size_t)q * ldm + p) : v4f{1.f, 1.f, 1.f, 1.f};
        return r;
    }
    __device__ inline void operator()(int q, int p, v4f v, const Pre& pre) const {
        const v4f m = pre.m;
        if (act == 0) {                         // no activation behind that layer (rmt:32-33 "linear"): dz = acc
        } else if (act == 1 || !mask) {
            v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f;
            v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
        } else {
            v.x *= act_grad(m.x, act); v.y *= act_grad(m.y, act);
            v.z *= act_grad(m.z, act); v.w *= act_grad(m.w, act);
        }
        store_stream(out + (size_t)q * ldo + p, v);
    }
    __device__ inline void finish(float*, int, int) const {}
};

// Input gradient of the WORLD MODEL's first layer (joint phase): its columns [c0, c0+n) are
// d(loss)/d(a_hat) arriving through the frozen world model (cycle loss, tpv:417-419).  Instead of
// storing the panel for a separate kernel, this epilogue forms the motor decoder's output gradient
// right here (tpv:381-382 + chain rule):
//     dz[q][c] = grad_scale * f(a_hat[q][c] - a[q][c]) + acc[q][c0+c]        (f: MSE d, L1 sign d)
// and the action-reconstruction loss partial of its workgroup.  The other columns (gradient wrt the
// state) have no consumer at lookahead 1 and are not stored.  Rows >= `rows` get zeros.
struct EpiActionSeed {
    const float* pred;  int ldp;      // a_hat: motor decoder output
    const float* target; int ldt;     // demonstrated action
    float* dz; int ldz;               // -> gradient wrt the decoder's output layer
    int c0, n, rows;
    float grad_scale;
    int l1;
    float* partial;
    float sq = 0.f;
    int tind = 0;                     // 1: the demonstrated action of batch row q is row trm.at(q) of `target` (`actions`)
    RowMap trm{};
    struct Pre {};
    __device__ inline Pre preload(int, int) const { return Pre(); }
    __device__ inline void operator()(int q, int p, v4f v, const Pre&) {
        if (p + 3 < c0 || p >= c0 + n) return;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = p + e - c0;
            if (c < 0 || c >= n) continue;
            float g = 0.f;
            if (q < rows) {
                const float d = pred[(size_t)q * ldp + c] - target[(size_t)(tind ? trm.at(q) : q) * ldt + c];
                sq += l1 ? fabsf(d) : d * d;
                g = grad_scale * (l1 ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : d) + v[e];
            }
            dz[(size_t)q * ldz + c] = g;
        }
    }
    __device__ inline void finish(float* scratch, int tile, int tid) {
        const float s = block_sum_256(sq, scratch);
        if (tid == 0) partial[tile] = s;
    }
};

// Input gradient of the MOTOR DECODER's first layer: its columns [c0, c0+Z) are d(loss)/dz.  This
// epilogue is the backward of the sampler + KL (autograd of rmt:734-740 and tpv:388) and writes the
// task encoder's output gradient directly:
//     dmu = dz + (beta/B) mu ;  dlogvar = dz * eps * 0.5 exp(0.5 lv) + (beta/B) 0.5 (exp(lv) - 1)
// Nothing else of the panel has a consumer at lookahead 1.
struct EpiSamplerSeed {
    const float* te_out; int ldte;    // [mu | logvar]
    const float* eps;                 // [rows_pad][Z] draws actually used
    float* dz; int ldz;               // -> gradient wrt the encoder's output layer [.. | dmu | dlogvar]
    int c0, Z, rows;
    float kl_scale;
    // learned prior mean (PVAE_PRIOR_STATE_MEAN; null otherwise): KL(N(mu,s^2) || N(mu_p,1)) pulls mu and
    // mu_p together -- dmu gets +kl (mu - mu_p), the prior stack's output gradient is the negative of it
    const float* mu_p = nullptr; int ldmp = 0;
    float* dz_p = nullptr; int ldzp = 0;
    struct Pre {};
    __device__ inline Pre preload(int, int) const { return Pre(); }
    __device__ inline void operator()(int q, int p, v4f v, const Pre&) const {
        if (p + 3 < c0 || p >= c0 + Z) return;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = p + e - c0;
            if (j < 0 || j >= Z) continue;
            float gm = 0.f, gl = 0.f, gp = 0.f;
            if (q < rows) {
                const float mu = te_out[(size_t)q * ldte + j];
                const float lv = te_out[(size_t)q * ldte + Z + j];
                const float ep = eps[(size_t)q * Z + j];
                if (mu_p) {
                    gp = kl_scale * (mu - mu_p[(size_t)q * ldmp + j]);
                    gm = v[e] + gp;
                } else {
                    gm = v[e] + kl_scale * mu;
                }
                gl = v[e] * ep * 0.5f * expf(0.5f * lv) + kl_scale * 0.5f * (expf(lv) - 1.0f);
            }
            dz[(size_t)q * ldz + j] = gm;
            dz[(size_t)q * ldz + Z + j] = gl;
            if (dz_p) dz_p[(size_t)q * ldzp + j] = -gp;
        }
    }
    __device__ inline void finish(float*, int, int) const {}
};

// Fixed-order sum of the per-workgroup loss partials -> {total, loss_a, loss_kl, loss_s,
// loss_cyc} (tpv:430-435 weighting).  Runs in one wave: as the tail of the step's last
// weight-gradient launch (training) or as its own tiny kernel (evaluation).
struct LossFinal {
    const float* part[4];     // per-term partial arrays (a, kl, s, cyc)
    float* out;               // null = nothing to do
    float scale[4];           // a, kl, s, cyc: 1/(B*Da), 1/B, 1/(B*Db), 1/(B*Db)
    float coeff[4];
    int nparts[4];            // 0 = term inactive
};
__device__ inline void finalize_loss_wave(const LossFinal& f, int lane) {
    float total = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float s = 0.f;
        for (int i = lane; i < f.nparts[t]; i += 64) s += f.part[t][i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        s *= f.scale[t];
        if (lane == 0) f.out[1 + t] = s;
        total += f.coeff[t] * s;
    }
    if (lane == 0) f.out[0] = total;
}

struct EpiGradStore {         // weight gradient -> gradient arena (data-parallel path)
    float* g;
    int ld;
    float* gb = nullptr;      // bias gradient destination (null = none)
    LossFinal loss{};
    struct Pre {};
    __device__ inline Pre load(int, int) const { return Pre{}; }
    __device__ inline void apply(int q, int p, v4f v, const Pre&) const { (*this)(q, p, v); }
    __device__ inline void operator()(int q, int p, v4f v) const { store_stream(g + (size_t)q * ld + p, v); }
    __device__ inline bool has_bias() const { return gb != nullptr; }
    __device__ inline void bias(int q, float v) const { gb[q] = v; }
};

// Read-add-write form of EpiGradStore (pvae_net_backward with accumulate = 1: one caller buffer summed over chunks of
// a minibatch).  Every output tile -- and every bias column block -- belongs to ONE workgroup whose contraction runs in
// a fixed order, so the same operands give the same bits; the old value is fetched under the loop like Adam's operands.
struct EpiGradAccum {
    float* g;
    int ld;
    float* gb = nullptr;
    LossFinal loss{};
    struct Pre { v4f g; };
    __device__ inline Pre load(int q, int p) const { return Pre{*reinterpret_cast<const v4f*>(g + (size_t)q * ld + p)}; }
    __device__ inline void apply(int q, int p, v4f v, const Pre& pre) const { store_stream(g + (size_t)q * ld + p, pre.g + v); }
    __device__ inline void operator()(int q, int p, v4f v) const { apply(q, p, v, load(q, p)); }
    __device__ inline bool has_bias() const { return gb != nullptr; }
    __device__ inline void bias(int q, float v) const { gb[q] += v; }
};

struct EpiGradAdam {          // weight gradient consumed in registers by Adam (1-GPU path)
    float* w;
    float* m;
    float* v;
    int ld;
    AdamScalars s;
    float* b = nullptr;       // bias / its moments (null = none)
    float* bm = nullptr;
    float* bv = nullptr;
    LossFinal loss{};
    struct Pre { v4f w, m, v; };
    // the Adam operands of a tile are fetched while the contraction runs (load) and consumed
    // in registers afterwards (apply)
    __device__ inline Pre load(int q, int p) const {
        const size_t o = (size_t)q * ld + p;
        return Pre{*reinterpret_cast<const v4f*>(w + o), *reinterpret_cast<const v4f*>(m + o),
                   *reinterpret_cast<const v4f*>(v + o)};
    }
    __device__ inline void apply(int q, int p, v4f g, Pre pre) const {
        const size_t o = (size_t)q * ld + p;
        adam_update4(g, pre.w, pre.m, pre.v, s);
        store_stream(w + o, pre.w);
        store_stream(m + o, pre.m);
        store_stream(v + o, pre.v);
    }
    __device__ inline void operator()(int q, int p, v4f g) const { apply(q, p, g, load(q, p)); }
    __device__ inline bool has_bias() const { return b != nullptr; }
    __device__ inline void bias(int q, float g) const {
        float pb = b[q], pm = bm[q], pv = bv[q];
        adam_update(g, pb, pm, pv, s);
        b[q] = pb; bm[q] = pm; bv[q] = pv;
    }
};
}  // namespace pvae
