// pvae_ppo_core.hip -- what the on-device PPO learner holds that no model owns (include/pvae.h "PPO learner step",
// "Train-batch preparation", "Action sampling", "Learner diagnostics"): the loss head and its finishing reduction (with the
// per-step diagnostics and the gradient norm's partial sums as template instantiations), the Adam + stats launch, the
// evaluate and the sampling epilogue, the pad copy, the zero-rows launch, GAE and standardisation, the minibatch order
// ("Minibatch order of the PPO learner"), their argument checks, and the entry points that need no model at all
// (pvae_ppo_loss, pvae_gae, pvae_ppo_order).  The stack set's learner (pvae_fc.hip) and
// PhysicsVAE's (pvae_ppo.hip) fill the argument structs of pvae_internal.h from their own panels and call the launch
// functions here: one kernel per job.
#include "pvae_internal.h"

#include <mutex>

namespace {

// ---------------------------------------------------------------------------------------
// PPO learner step: the loss head and the Adam + stats launch (include/pvae.h "PPO learner step")
// ---------------------------------------------------------------------------------------
// A wave works on one row at a time, lanes over the k actions, butterfly reductions (every lane ends with the same sum, in
// an order that depends on nothing but k).  The launch has one wave for every two padded rows (head_waves): wave w takes
// rows w, w + waves, ... one after the other: its sums of the five per-row terms and,
// for a state-independent log-std, of the log-std gradient columns go to partial row w of the scratch buffer -- no
// atomics, so the finishing reduction (ppo_finish) adds them in a fixed order.
constexpr int kHeadMaxBlocks = 1024;
constexpr int kPartStats = 8;             // floats reserved for the stats at the head of a partial row
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// DIAG (include/pvae.h "Learner diagnostics"): the wave also leaves, in diagnostics partial row w (kDiagPart floats),
// over its rows: [0] rows with the ratio outside [1 - clip, 1 + clip] (the negation of the comparison below), [1] rows with
// |value - vf_preds| > vf_clip, [2] max |ratio - 1| (this one ratio re-formed in double, see below), and the four sums of the two variances, [3] sum (y - y0), [4] sum
// (y - y0)^2, [5] sum (e - e0), [6] sum (e - e0)^2 with y = value_targets, e = y - value -- taken around the FIRST
// minibatch row's y0 and e0, which every wave reads for itself: raw float32 sums of y and y^2 lose the variance of targets
// far from zero (1000 +- 2: off by up to 5e-2; the pivoted sums are within 1e-7 of float64).  The stats partial row
// keeps its layout and its bits; without DIAG the kernel is the one it was.
template <bool DIAG>
__global__ void __launch_bounds__(256)
ppo_head_kernel(PpoHead h) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
    const int k = h.k;
    float* __restrict__ part = h.part + (size_t)wave * h.part_stride;
    if (h.colsum)
        for (int j = lane; j < k; j += 64) part[kPartStats + j] = 0.f;
    float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float dg[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float y0 = 0.f, e0 = 0.f;
    if constexpr (DIAG) {
        y0 = h.vtarg[batch_row(h.index, h.row0, h.n_rows, 0)];
        e0 = y0 - h.value[0];
    }
    for (int r = wave; r < h.rows_pad; r += waves) {
        const bool live = r < h.rows;
        float dlogp = 0.f, dval = 0.f;
        const float* mu = nullptr; const float* ls = nullptr; const float* act = nullptr; const float* od = nullptr;
        if (live) {
            const long long br = batch_row(h.index, h.row0, h.n_rows, r);
            mu = h.mean + r * h.ld_mean; ls = h.ls + r * h.ld_ls;
            act = h.actions + br * k; od = h.old_dist + br * 2 * k;
            float zz = 0.f, lss = 0.f, kl = 0.f;
            [[maybe_unused]] double zz_d = 0.0, lss_d = 0.0;
            for (int j = lane; j < k; j += 64) {
                const float l = h.ls_base + ls[j], inv_sig = expf(-l);
                const float z = (act[j] - mu[j]) * inv_sig, d = od[j] - mu[j], lo = od[k + j];
                zz = fmaf(z, z, zz);
                lss += l;
                if constexpr (DIAG) {
                    const double zd = ((double)act[j] - (double)mu[j]) * exp(-(double)l);
                    zz_d = fma(zd, zd, zz_d);
                    lss_d += (double)l;
                }
                kl += l - lo + (expf(2.f * lo) + d * d) * (0.5f * inv_sig * inv_sig) - 0.5f;
            }
            zz = wave_sum(zz); lss = wave_sum(lss); kl = wave_sum(kl);
            const float logp = -0.5f * zz - lss - 0.5f * k * 1.8378770664093453f;          // log(2 pi)
            const float adv = h.adv[br], ratio = expf(logp - h.old_logp[br]);
            const float lo_r = 1.f - h.clip, hi_r = 1.f + h.clip;
            const float s1 = adv * ratio, s2 = adv * fminf(fmaxf(ratio, lo_r), hi_r);
            const float surr = fminf(s1, s2);
            if (s1 < s2 || (ratio >= lo_r && ratio <= hi_r)) dlogp = -h.inv_rows * s1;
            const float ent = lss + 0.5f * k * 2.8378770664093453f;                       // log(2 pi e)
            const float val = h.value[r * h.ld_value], vt = h.vtarg[br], vp = h.vpred[br];
            const float dv = val - vp, e1 = val - vt;
            const float e2 = vp + fminf(fmaxf(dv, -h.vf_clip), h.vf_clip) - vt;
            const float vf1 = e1 * e1, vf2 = e2 * e2, vf = fmaxf(vf1, vf2);
            if (vf1 >= vf2 || fabsf(dv) <= h.vf_clip) dval = h.vf_coeff * h.inv_rows * 2.f * e1;
            st[0] += -surr + h.kl_coeff * kl + h.vf_coeff * vf - h.ent_coeff * ent;
            st[1] += -surr; st[2] += vf; st[3] += kl; st[4] += ent;
            if constexpr (DIAG) {
                if (ratio < lo_r || ratio > hi_r) dg[0] += 1.f;
                if (fabsf(dv) > h.vf_clip) dg[1] += 1.f;
                // ratio_max_dev from the log-density summed in double: the loss's own float32 logp is a sum of ~k terms
                // of magnitude ~k, whose ulp at k >= 130 (1.5e-5) would show in exp(logp - old_logp) - 1
                zz_d = wave_sum_d(zz_d); lss_d = wave_sum_d(lss_d);
                const double logp_d = -0.5 * zz_d - lss_d - 0.5 * k * 1.8378770664093453;
                dg[2] = fmaxf(dg[2], (float)fabs(exp(logp_d - (double)h.old_logp[br]) - 1.0));
                const float dy = vt - y0, de = (vt - val) - e0;
                dg[3] += dy; dg[4] = fmaf(dy, dy, dg[4]);
                dg[5] += de; dg[6] = fmaf(de, de, dg[6]);
            }
        }
        // the gradients, over the whole padded width of the row: zeros in pad rows and pad columns
        const int wmax = max(h.d_mean ? h.width_dm : k, h.d_ls ? h.width_dls : k);
        const float klc = h.kl_coeff * h.inv_rows, entc = h.ent_coeff * h.inv_rows;
        for (int j = lane; j < wmax; j += 64) {
            float gm = 0.f, gl = 0.f;
            if (live && j < k) {
                const float l = h.ls_base + ls[j], inv_sig = expf(-l), inv_var = inv_sig * inv_sig;
                const float am = act[j] - mu[j], z = am * inv_sig, d = od[j] - mu[j];
                gm = dlogp * am * inv_var - klc * d * inv_var;
                gl = dlogp * (z * z - 1.f) + klc * (1.f - (expf(2.f * od[k + j]) + d * d) * inv_var) - entc;
                if (h.colsum) part[kPartStats + j] += gl;
            }
            if (h.d_mean && j < h.width_dm) h.d_mean[(size_t)r * h.ld_dm + j] = gm;
            if (h.d_ls && j < h.width_dls) h.d_ls[(size_t)r * h.ld_dls + j] = gl;
        }
        if (h.d_value)
            for (int j = lane; j < h.width_dv; j += 64) h.d_value[(size_t)r * h.ld_dv + j] = j == 0 ? dval : 0.f;
    }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < 5; ++t) part[t] = st[t];
        if constexpr (DIAG) {
            float* __restrict__ dp = h.dpart + (size_t)wave * kDiagPart;
#pragma unroll
            for (int t = 0; t < 7; ++t) dp[t] = dg[t];
            dp[7] = 0.f;
        }
    }
}

// Diagnostics entries 0..3 from the diagnostics partial rows, by ONE wave: lane l adds rows l, l + 64, ... in double,
// then a butterfly -- an order that depends on nothing but nparts.  The variances are finished in double from the pivoted
// sums; vf_explained_var = max(-1, 1 - Var(y - v) / Var(y)), exactly -1 for one row or Var(y) == 0.  The reserved
// entries 5..7 get 0, and `zero4` entry 4 too (the stand-alone head: no gradient norm).
__device__ inline void ppo_diag_finish(const float* __restrict__ dpart, int nparts, int rows, float* __restrict__ out, int zero4,
                                       int lane) {
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < nparts; i += 64) {
        const float* __restrict__ dp = dpart + (size_t)i * kDiagPart;
        s[0] += (double)dp[0]; s[1] += (double)dp[1];
        s[2] = fmax(s[2], (double)dp[2]);
        s[3] += (double)dp[3]; s[4] += (double)dp[4]; s[5] += (double)dp[5]; s[6] += (double)dp[6];
    }
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        if (t == 2) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s[2] = fmax(s[2], __shfl_xor(s[2], o, 64));
        } else {
            s[t] = wave_sum_d(s[t]);
        }
    }
    if (lane != 0) return;
    const double n = (double)rows, my = s[3] / n, me = s[5] / n;
    const double var_y = s[4] / n - my * my, var_e = s[6] / n - me * me;
    double ev = -1.0;
    if (rows > 1 && var_y > 0.0) ev = fmax(-1.0, 1.0 - fmax(var_e, 0.0) / var_y);
    out[0] = (float)ev;
    out[1] = (float)(s[0] / n);
    out[2] = (float)(s[1] / n);
    out[3] = (float)s[2];
    if (zero4) out[4] = 0.f;
    out[5] = 0.f; out[6] = 0.f; out[7] = 0.f;
}

// The gradient norm's two ends.  Every workgroup of an Adam launch ends with block_sum_sq: the squares of the gradient
// values its threads loaded, added in double -- a butterfly per wave, then the four waves through LDS in wave order --
// into the workgroup's OWN slot: no atomics, and the grid-stride map fixes which elements a workgroup holds, so the
// sum depends on (segment sizes, grid) and never on timing.  ppo_gnorm_kernel, one wave of a later launch, adds the slots
// in slot order (lane l: slots l, l + 64, ..., then a butterfly) and writes sqrt as float32 to diagnostics entry 4.
__device__ inline double sq4(const v4f& g) {
    return ((double)g[0] * (double)g[0] + (double)g[1] * (double)g[1]) + ((double)g[2] * (double)g[2] + (double)g[3] * (double)g[3]);
}
__device__ inline void block_sum_sq(double sq, double* __restrict__ slot) {
    __shared__ double red[4];
    sq = wave_sum_d(sq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) *slot = ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ void __launch_bounds__(64)
ppo_gnorm_kernel(const double* __restrict__ gslot, int nslots, float* __restrict__ out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nslots; i += 64) s += gslot[i];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) *out = (float)sqrt(s);
}
// The partial rows summed in a fixed order by ONE wave: stats_out[5] (means over the rows)
__device__ inline void ppo_finish(const float* __restrict__ part, int nparts, int stride, float inv_rows, float* __restrict__ out,
                                  int lane) {
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        float s = 0.f;
        for (int i = lane; i < nparts; i += 64) s += part[(size_t)i * stride + t];
        s = wave_sum(s) * inv_rows;
        if (lane == 0) out[t] = s;
    }
}
__global__ void __launch_bounds__(64)
ppo_finish_kernel(const float* part, int nparts, int stride, float inv_rows, float* out) {
    ppo_finish(part, nparts, stride, inv_rows, out, threadIdx.x);
}
// the finishing launch of the stand-alone head and of the step's first half with diagnostics: wave 0 the stats, wave 1 the
// diagnostics entries
__global__ void __launch_bounds__(128)
ppo_finish_diag_kernel(const float* part, int nparts, int stride, float inv_rows, float* out, const float* dpart, int rows,
                       float* diag, int zero4) {
    if (threadIdx.x < 64) ppo_finish(part, nparts, stride, inv_rows, out, threadIdx.x);
    else ppo_diag_finish(dpart, nparts, rows, diag, zero4, threadIdx.x - 64);
}

// column j of a state-independent log-std's gradient: the partial rows added in partial-row order
__device__ inline float ppo_ls_colsum(const float* __restrict__ part, int nparts, int stride, int j) {
    double gs = 0.0;                           // (a few hundred signed terms per column: in double, so that the order does not show)
    for (int i = 0; i < nparts; ++i) gs += (double)part[(size_t)i * stride + kPartStats + j];
    return (float)gs;
}

// Adam over the trained segments (adam_update4 with the AdamScalars the trainer's adam_flat_kernel gets: the same bits)
// + ONE extra workgroup, the last: the stats and, for a state-independent log-std, that vector's gradient (the column
// sums, added in partial-row order) and its Adam update.  A segment is a run of float4 elements with its own parameter,
// gradient and moment base pointers: the trained stacks' parts of one stack-set arena, or the encoder's and the decoder's
// parts of PhysicsVAE's arena and the value stack set's arena.
struct PpoAdam {
    PpoAdamSegs seg;
    long long end4[kAdamSegs];                      // running float4 count through segment i
    AdamScalars s;
    const float* part; int nparts, part_stride; float inv_rows; float* stats_out;
    int k; float* ls; float* ls_m; float* ls_v;
    // DIAG instantiations only: the head's diagnostics partial rows and the row they finish into (entries 0..3), the
    // minibatch's rows, and the gradient-norm slots, one per workgroup of the launch
    const float* dpart; int rows; float* diag; double* gslot;
    // CLIP instantiations and the clip launches only (include/pvae.h "Gradient clipping inside the PPO learners"): the
    // slots the sum-of-squares launch filled, their number, and the threshold
    double* cslot; int ncslots; float max_norm;
};

// ---------------------------------------------------------------------------------------
// global-norm gradient clipping (include/pvae.h "Gradient clipping inside the PPO learners")
// ---------------------------------------------------------------------------------------
// The sum-of-squares launch, between the backward and the Adam launch: a grid-stride pass over the segments the Adam
// launch runs over, every workgroup's squares (sq4 / block_sum_sq: in double) into ITS slot of the clip scratch; ONE extra
// workgroup, the last, squares the state-independent log-std vector's gradient, the column sums the Adam launch's last
// workgroup forms again (ppo_ls_colsum: the same bits).  Its grid is its own (kClipGrid + 1 workgroups at the most):
// every workgroup of the launch behind it re-adds all slots.
__global__ void __launch_bounds__(256)
ppo_clip_sumsq_kernel(PpoAdam a) {
    double sq = 0.0;
    if (blockIdx.x == gridDim.x - 1) {
        if (a.ls)
            for (int j = threadIdx.x; j < a.k; j += 256) {
                const float g = ppo_ls_colsum(a.part, a.nparts, a.part_stride, j);
                sq += (double)g * (double)g;
            }
    } else {
        const long long n4 = a.seg.n ? a.end4[a.seg.n - 1] : 0;
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (gridDim.x - 1) * 256ll) {
            int k = 0;
            while (i >= a.end4[k]) ++k;
            const long long q = i - (k ? a.end4[k - 1] : 0);
            sq += sq4(reinterpret_cast<const v4f*>(a.seg.g[k])[q]);
        }
    }
    block_sum_sq(sq, a.cslot + blockIdx.x);
}
// norm = float32(sqrt(sum of the slots)), coef = min(1, max_norm / (norm + 1e-6)) in float32 (torch's clip_grad_norm_;
// a NaN quotient stays NaN, as torch.clamp leaves it), by ONE full wave: lane l adds slots l, l + 64, ... then the double
// butterfly, as ppo_gnorm_kernel -- an order that depends on nothing but the slot count, so every workgroup of every launch
// forms the same bits.  Every lane returns the same pair.
__device__ inline float clip_coef_wave(const double* __restrict__ cslot, int ncslots, float max_norm, int lane, float* norm_out) {
    double s = 0.0;
    for (int i = lane; i < ncslots; i += 64) s += cslot[i];
    s = wave_sum_d(s);
    const float norm = (float)sqrt(s);
    const float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
    *norm_out = norm;
    return c > 1.0f ? 1.0f : c;
}
// ... by a workgroup's first wave, handed to the others through LDS (every thread of the workgroup must call)
__device__ inline float block_clip_coef(const PpoAdam& a, float* norm_out) {
    __shared__ float cc[2];
    if (threadIdx.x < 64) {
        float norm;
        const float c = clip_coef_wave(a.cslot, a.ncslots, a.max_norm, threadIdx.x, &norm);
        if (threadIdx.x == 0) { cc[0] = c; cc[1] = norm; }
    }
    __syncthreads();
    *norm_out = cc[1];
    return cc[0];
}
__device__ inline v4f scale4(const v4f& g, float s) {       // (pinned: no contraction with Adam's first operation)
    return v4f{__fmul_rn(g[0], s), __fmul_rn(g[1], s), __fmul_rn(g[2], s), __fmul_rn(g[3], s)};
}
// The clip's product g * coef.  __fmul_rn is a plain `*` to this compiler: what keeps scale4's products whole is that each
// has several uses in Adam.  A product with ONE use -- a term of the exchanged launch's rank-order sum -- would be
// contracted into an fma and round differently from the product *_ppo_grad stores; without the contract flag no later
// addition can absorb it.
__device__ inline float clip_mul(float g, float coef) {
#pragma clang fp contract(off)
    return g * coef;
}
__device__ inline v4f clip4(const v4f& g, float coef) {
    return v4f{clip_mul(g[0], coef), clip_mul(g[1], coef), clip_mul(g[2], coef), clip_mul(g[3], coef)};
}
// *_ppo_grad's last launch while a clip is bound: the gradient in the arena(s) and ls_grad scaled IN PLACE by coef, so
// that a transport outside the library sums clipped gradients.  The extra last workgroup takes ls_grad and, with a
// diagnostics row, writes its entries 5 (the raw norm) and 6 (coef).
__global__ void __launch_bounds__(256)
ppo_clip_scale_kernel(PpoAdam a, float* __restrict__ ls_grad) {
    float norm;
    const float coef = block_clip_coef(a, &norm);
    if (blockIdx.x == gridDim.x - 1) {
        if (a.ls)
            for (int j = threadIdx.x; j < a.k; j += 256) ls_grad[j] = clip_mul(ls_grad[j], coef);
        if (a.diag && threadIdx.x == 0) { a.diag[5] = norm; a.diag[6] = coef; }
        return;
    }
    const long long n4 = a.seg.n ? a.end4[a.seg.n - 1] : 0;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (gridDim.x - 1) * 256ll) {
        int k = 0;
        while (i >= a.end4[k]) ++k;
        const long long q = i - (k ? a.end4[k - 1] : 0);
        v4f* g = reinterpret_cast<v4f*>(const_cast<float*>(a.seg.g[k])) + q;
        *g = clip4(*g, coef);
    }
}
// the diagnostics' finishing launch of a clipped step: wave 0 is ppo_gnorm_kernel (entry 4: what Adam consumed), wave 1
// writes entry 5, this worker's own norm before the clip, and entry 6, coef
__global__ void __launch_bounds__(128)
ppo_gnorm_clip_kernel(const double* __restrict__ gslot, int nslots, const double* __restrict__ cslot, int ncslots, float max_norm,
                      float* __restrict__ row) {
    if (threadIdx.x < 64) {
        double s = 0.0;
        for (int i = threadIdx.x; i < nslots; i += 64) s += gslot[i];
        s = wave_sum_d(s);
        if (threadIdx.x == 0) row[4] = (float)sqrt(s);
    } else {
        float norm;
        const float c = clip_coef_wave(cslot, ncslots, max_norm, threadIdx.x - 64, &norm);
        if (threadIdx.x == 64) { row[5] = norm; row[6] = c; }
    }
}

// DIAG: + the diagnostics entries 0..3 by the extra workgroup's second wave, and every workgroup's sum of squares of the
// gradient values it consumed into its slot (block_sum_sq; the extra workgroup: the log-std vector's gradient)
// CLIP: every workgroup forms coef from the clip slots (block_clip_coef) and multiplies each gradient value it loads by
// it -- one pinned float32 multiply, also when coef == 1, where the product is the value itself
template <bool DIAG, bool CLIP>
__global__ void __launch_bounds__(256)
ppo_adam_kernel(PpoAdam a) {
    [[maybe_unused]] double sq = 0.0;
    [[maybe_unused]] float coef = 1.0f;
    if constexpr (CLIP) {
        float norm;
        coef = block_clip_coef(a, &norm);
    }
    if (blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x < 64) ppo_finish(a.part, a.nparts, a.part_stride, a.inv_rows, a.stats_out, threadIdx.x);
        if constexpr (DIAG)
            if (threadIdx.x >= 64 && threadIdx.x < 128) ppo_diag_finish(a.dpart, a.nparts, a.rows, a.diag, 0, threadIdx.x - 64);
        if (a.ls)
            for (int j = threadIdx.x; j < a.k; j += 256) {
                float g = ppo_ls_colsum(a.part, a.nparts, a.part_stride, j);
                if constexpr (CLIP) g = clip_mul(g, coef);
                if constexpr (DIAG) sq += (double)g * (double)g;
                float p = a.ls[j], m = a.ls_m[j], v = a.ls_v[j];
                adam_update(g, p, m, v, a.s);
                a.ls[j] = p; a.ls_m[j] = m; a.ls_v[j] = v;
            }
        if constexpr (DIAG) block_sum_sq(sq, a.gslot + blockIdx.x);
        return;
    }
    const long long n4 = a.seg.n ? a.end4[a.seg.n - 1] : 0;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (gridDim.x - 1) * 256ll) {
        int k = 0;
        while (i >= a.end4[k]) ++k;
        const long long q = i - (k ? a.end4[k - 1] : 0);
        v4f pp = reinterpret_cast<v4f*>(a.seg.p[k])[q];
        v4f gg = reinterpret_cast<const v4f*>(a.seg.g[k])[q];
        if constexpr (CLIP) gg = clip4(gg, coef);
        if constexpr (DIAG) sq += sq4(gg);
        v4f mm = reinterpret_cast<v4f*>(a.seg.m[k])[q];
        v4f vv = reinterpret_cast<v4f*>(a.seg.v[k])[q];
        adam_update4(gg, pp, mm, vv, a.s);
        reinterpret_cast<v4f*>(a.seg.p[k])[q] = pp;
        reinterpret_cast<v4f*>(a.seg.m[k])[q] = mm;
        reinterpret_cast<v4f*>(a.seg.v[k])[q] = vv;
    }
    if constexpr (DIAG) block_sum_sq(sq, a.gslot + blockIdx.x);
}

// ---------------------------------------------------------------------------------------
// the step in two halves, and the exchanged Adam launch (include/pvae.h "Gradient exchange between workers")
// ---------------------------------------------------------------------------------------
// first half's end: the log-std gradient where the caller can reduce it over the workers (the stats: ppo_finish_kernel)
__global__ void __launch_bounds__(256)
ppo_ls_grad_kernel(const float* part, int nparts, int stride, int k, float* __restrict__ ls_grad) {
    for (int j = blockIdx.x * 256 + threadIdx.x; j < k; j += gridDim.x * 256) ls_grad[j] = ppo_ls_colsum(part, nparts, stride, j);
}

// Adam on float4 element q of segment k with the gradient gg: the local parameters and moments, as ppo_adam_kernel
__device__ inline void ppo_adam_elem(const PpoAdam& a, int k, long long q, const v4f& gg) {
    v4f pp = reinterpret_cast<v4f*>(a.seg.p[k])[q];
    v4f mm = reinterpret_cast<v4f*>(a.seg.m[k])[q];
    v4f vv = reinterpret_cast<v4f*>(a.seg.v[k])[q];
    adam_update4(gg, pp, mm, vv, a.s);
    reinterpret_cast<v4f*>(a.seg.p[k])[q] = pp;
    reinterpret_cast<v4f*>(a.seg.m[k])[q] = mm;
    reinterpret_cast<v4f*>(a.seg.v[k])[q] = vv;
}
// second half: ppo_adam_kernel on scale * gradient, the log-std vector from scale * ls_grad; no stats (the first half wrote them)
// (DIAG: the slots get the squares of scale * gradient, what Adam consumes)
template <bool DIAG>
__global__ void __launch_bounds__(256)
ppo_apply_kernel(PpoAdam a, float scale, const float* __restrict__ ls_grad) {
    [[maybe_unused]] double sq = 0.0;
    if (blockIdx.x == gridDim.x - 1) {
        if (a.ls)
            for (int j = threadIdx.x; j < a.k; j += 256) {
                float p = a.ls[j], m = a.ls_m[j], v = a.ls_v[j];
                const float g = __fmul_rn(ls_grad[j], scale);
                if constexpr (DIAG) sq += (double)g * (double)g;
                adam_update(g, p, m, v, a.s);
                a.ls[j] = p; a.ls_m[j] = m; a.ls_v[j] = v;
            }
        if constexpr (DIAG) block_sum_sq(sq, a.gslot + blockIdx.x);
        return;
    }
    const long long n4 = a.seg.n ? a.end4[a.seg.n - 1] : 0;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (gridDim.x - 1) * 256ll) {
        int k = 0;
        while (i >= a.end4[k]) ++k;
        const long long q = i - (k ? a.end4[k - 1] : 0);
        const v4f gg = scale4(reinterpret_cast<const v4f*>(a.seg.g[k])[q], scale);
        if constexpr (DIAG) sq += sq4(gg);
        ppo_adam_elem(a, k, q, gg);
    }
    if constexpr (DIAG) block_sum_sq(sq, a.gslot + blockIdx.x);
}

// The exchanged form of ppo_adam_kernel: N workers' gradients, each in its own process' buffers and mapped into this one
// (PpoPeers), summed IN RANK ORDER, scaled by float(1 / N), and Adam applied to the LOCAL parameters and moments -- every
// rank updates every element, so the replicas and their moments stay whole and bit-identical.  The hand-off is
// p2p_exchange_kernel's (pvae_exchange.hip): the gradient was written by earlier launches of the stream, so
//   1. workgroup 0 stores this rank's log-std gradient to its slot in the flag block, fences (system-scope release) and
//      tells every peer "ready": epoch -> peer's ready[me];
//   2. every workgroup waits for all peers' "ready" (p2p_wait: bounded), acquires, and reads every handed-off byte with
//      `buffer_load ... sc0 sc1` through descriptors over the segment in each rank's arena;
//   3. the extra last workgroup finishes the stats (this worker's own) and updates the log-std vector from the N slots;
//   4. the last workgroup to finish (ticket) tells every peer "done" and waits for theirs: when the launch ends the next
//      step's backward may overwrite the gradient buffers.
// A wait that gives up aborts this rank's update -- nothing moves, the error word counts it, "done" is still sent.
// Every workgroup of the launch spins until the peers arrive, so the grid stays far below what fills the device
// (kExchangeMaxBlocks): workers that share one GPU must be able to run their launches side by side.
constexpr int kExchangeMaxBlocks = 256;
struct PpoAdamPeers {
    unsigned* f[PVAE_P2P_MAX_RANKS];                         // flag blocks
    const float* arena[kPpoPeerArenas][PVAE_P2P_MAX_RANKS];  // gradient arenas
    int seg_arena[kAdamSegs]; long long seg_off[kAdamSegs];  // where segment i's gradient lies: arena, float offset
    int me; unsigned epoch; long long timeout_ticks;
    float inv_n;
};
// DIAG: as ppo_adam_kernel's -- the slots get the squares of the AVERAGED gradient, so every rank reports the same norm
// CLIP: every worker clips its own gradient first, then the clipped gradients are averaged.  Every workgroup forms this
// rank's coef from its own clip slots; workgroup 0 stores it to word kPpoPeerCoef of the flag block ahead of the "ready"
// release, and a reader loads peer q's coef_q behind the acquire, with the system-scope load it reads the log-std slot
// with -- no new wait.  The sum in rank order is over the products g_q * coef_q, each rounded on its own (clip_mul); the
// log-std slots hold the RAW column sums and are scaled by the reader in the same way.
template <int N, bool DIAG, bool CLIP>
__global__ void __launch_bounds__(256)
ppo_adam_exchange_kernel(PpoAdam a, PpoAdamPeers x) {
    [[maybe_unused]] double sq = 0.0;
    unsigned* mine = x.f[x.me];
    const int tid = threadIdx.x, me = x.me;
    [[maybe_unused]] __shared__ float coefs[N];
    if constexpr (CLIP) {
        float norm;
        const float coef = block_clip_coef(a, &norm);
        if (tid == 0) coefs[me] = coef;                  // (read behind the barriers below)
        if (blockIdx.x == 0 && tid == 0)
            __hip_atomic_store((float*)(mine + kPpoPeerCoef), coef, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (blockIdx.x == 0) {
        if (a.ls)
            for (int j = tid; j < a.k; j += 256)
                __hip_atomic_store((float*)(mine + kPpoPeerLs) + j, ppo_ls_colsum(a.part, a.nparts, a.part_stride, j),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid < N && tid != me) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");             // (system scope; the launches that wrote the gradient ended before this one began)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            p2p_st(x.f[tid] + kPpoPeerReady + me, x.epoch);
        }
    }
    __shared__ int abort_;
    if (tid == 0) abort_ = 0;
    __syncthreads();
    if (tid < N && tid != me) {
        if (!p2p_wait(mine + kPpoPeerReady + tid, x.epoch, x.timeout_ticks, mine + kPpoPeerErr)) abort_ = 1;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        if constexpr (CLIP)
            coefs[tid] = __hip_atomic_load((const float*)(x.f[tid] + kPpoPeerCoef), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads();
    const bool go = !abort_;
    if (blockIdx.x == gridDim.x - 1) {
        if (tid < 64) ppo_finish(a.part, a.nparts, a.part_stride, a.inv_rows, a.stats_out, tid);
        if constexpr (DIAG)
            if (tid >= 64 && tid < 128) ppo_diag_finish(a.dpart, a.nparts, a.rows, a.diag, 0, tid - 64);
        if (a.ls && go)
            for (int j = tid; j < a.k; j += 256) {
                float g = 0.f;                 // (the own column is summed here again: no workgroup waits for another of its launch)
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    float gq = q == me ? ppo_ls_colsum(a.part, a.nparts, a.part_stride, j)
                                       : __hip_atomic_load((const float*)(x.f[q] + kPpoPeerLs) + j, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_SYSTEM);
                    if constexpr (CLIP) gq = clip_mul(gq, coefs[q]);
                    g = q == 0 ? gq : g + gq;                         // rank order
                }
                float p = a.ls[j], m = a.ls_m[j], v = a.ls_v[j];
                const float gs = __fmul_rn(g, x.inv_n);
                if constexpr (DIAG) sq += (double)gs * (double)gs;
                adam_update(gs, p, m, v, a.s);
                a.ls[j] = p; a.ls_m[j] = m; a.ls_v[j] = v;
            }
    } else if (go) {
        for (int k = 0; k < a.seg.n; ++k) {
            const long long n4 = a.seg.n4[k];
            __amdgpu_buffer_rsrc_t rg[N];
#pragma unroll
            for (int q = 0; q < N; ++q)
                rg[q] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x.arena[x.seg_arena[k]][q] + x.seg_off[k]), 0,
                                                          (unsigned)(n4 * 16), 0x00020000);
            for (long long i = blockIdx.x * 256ll + tid; i < n4; i += (gridDim.x - 1) * 256ll) {
                v4f g[N];
#pragma unroll
                for (int q = 0; q < N; ++q)
                    g[q] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rg[q], (unsigned)(i * 16), 0, 17));
                if constexpr (CLIP) {
#pragma unroll
                    for (int q = 0; q < N; ++q) g[q] = clip4(g[q], coefs[q]);
                }
                v4f sum = g[0];
#pragma unroll
                for (int q = 1; q < N; ++q) sum += g[q];              // rank order
                const v4f gs = scale4(sum, x.inv_n);
                if constexpr (DIAG) sq += sq4(gs);
                ppo_adam_elem(a, k, i, gs);
            }
        }
    }
    if constexpr (DIAG) block_sum_sq(sq, a.gslot + blockIdx.x);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ unsigned last;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        last = atomicAdd(mine + kPpoPeerTicket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    if (tid == 0) mine[kPpoPeerTicket] = 0;
    if (tid < N && tid != me) {
        p2p_st(x.f[tid] + kPpoPeerDone + me, x.epoch);
        p2p_wait(mine + kPpoPeerDone + tid, x.epoch, x.timeout_ticks, mine + kPpoPeerErr);
    }
}

// ---------------------------------------------------------------------------------------
// glue: the pad copy and the zero-rows launch (pvae_internal.h)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
ppo_pad_copy_kernel(const float* __restrict__ src, int n, int rows, float* __restrict__ dst, int ld, int rows_pad,
                    const int32_t* __restrict__ index, long long n_rows, const uint8_t* __restrict__ done) {
    const int total = rows_pad * ld;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / ld, c = idx - r * ld;
        dst[idx] = (r < rows && c < n && !(done && done[r])) ? src[(size_t)batch_row(index, 0, n_rows, r) * n + c] : 0.f;
    }
}

// blockIdx.y = panel
__global__ void __launch_bounds__(256)
ppo_zero_rows_kernel(ZeroRows z) {
    const int k = blockIdx.y;
    float* __restrict__ p = z.p[k];
    const int ld = z.ld[k], width = z.width[k];
    const int total = (z.r1 - z.r0) * width;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / width, c = idx - r * width;
        p[(size_t)(z.r0 + r) * ld + c] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------
// train-batch preparation: evaluate epilogue, GAE, standardisation (include/pvae.h "Train-batch preparation")
// ---------------------------------------------------------------------------------------
// The epilogue of one evaluated chunk: a wave per row reads the stacks' outputs in their panels and writes vf[r],
// dist[r] = [mean | log_std] and logp[r] of actions[r] -- the arithmetic of ppo_head_kernel's logp, term for term, so
// that the learner's first step sees a ratio of exactly 1.  mean == NULL: the bootstrap use -- the value stack ran alone;
// vf[r] = done[r] ? 0 : value[r].  The output pointers are those of the chunk's first row.  eps_dst (PhysicsVAE's evaluate
// pass): the latent draws of the chunk, eps_src [rows][Z], copied to the caller's rows.
constexpr int kEvalMaxBlocks = 1024;
// the log-density's arithmetic, shared by the evaluate and the sampling epilogue so that both give the same bits:
// one column's terms into the lane's sums, and lane 0's closing expression over the wave sums
__device__ inline void logp_column(float a, float mu, float l, float& zz, float& lss) {
    const float inv_sig = expf(-l);
    const float z = (a - mu) * inv_sig;
    zz = fmaf(z, z, zz);
    lss += l;
}
__device__ inline float logp_close(float zz, float lss, int k) {
    return -0.5f * zz - lss - 0.5f * k * 1.8378770664093453f;                               // log(2 pi)
}
__global__ void __launch_bounds__(256)
ppo_eval_epilogue_kernel(PpoEval e) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
    const int k = e.k;
    for (int r = wave; r < e.rows; r += waves) {
        if (!e.mean) {
            if (lane == 0) e.vf[r] = e.done[r] ? 0.f : e.value[r * e.ld_value];
            continue;
        }
        const float* mu = e.mean + r * e.ld_mean;
        const float* ls = e.ls + r * e.ld_ls;
        const float* act = e.actions + (size_t)r * k;
        float* dist = e.dist + (size_t)r * 2 * k;
        float zz = 0.f, lss = 0.f;
        for (int j = lane; j < k; j += 64) {
            const float l = e.ls_base + ls[j];
            logp_column(act[j], mu[j], l, zz, lss);
            dist[j] = mu[j];
            dist[k + j] = l;
        }
        zz = wave_sum(zz); lss = wave_sum(lss);
        if (lane == 0) {
            e.logp[r] = logp_close(zz, lss, k);
            e.vf[r] = e.value[r * e.ld_value];
        }
        if (e.eps_dst)
            for (int j = lane; j < e.Z; j += 64) e.eps_dst[(size_t)r * e.Z + j] = e.eps_src[(size_t)r * e.Z + j];
    }
}

// The sampling epilogue of one chunk (include/pvae.h "Action sampling"): a wave per row, lane l holds columns l, l + 64,
// ... as in the evaluate epilogue, so that the log-density's sums run in its order.  Lanes 4q .. 4q + 3 hold the four
// columns of one Philox group: lane 4q makes the call (row = the chunk's row, group = 0x80000000 + column / 4: the high
// bit keeps the action noise apart from the latent draws, whose groups are < Z / 4) and the other three read their
// component from it; a tail group is used in part.  The log-density is that of the STORED float32 action, never formed
// from the noise.  Every destination row is clamped into [0, n_dst_rows); plain stores, no atomics.
__global__ void __launch_bounds__(256)
ppo_act_epilogue_kernel(PpoAct a) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
    const int k = a.k;
    for (int r = wave; r < a.rows; r += waves) {
        const long long dst = batch_row(a.out_row, a.row0, a.n_dst_rows, r);
        const float* mu = a.mean + r * a.ld_mean;
        const float* ls = a.ls + r * a.ld_ls;
        float* act = a.actions + (size_t)dst * k;
        float* dist = a.dist + (size_t)dst * 2 * k;
        float zz = 0.f, lss = 0.f;
        for (int j0 = 0; j0 < k; j0 += 64) {                     // (wave-uniform trip count: the shuffles below need every lane)
            const int j = j0 + lane;
            const bool live = j < k;
            float n = 0.f;
            if (a.explore) {
                if (a.noise) {
                    if (live) n = a.noise[(size_t)r * k + j];
                } else {
                    v4f g = v4f{0.f, 0.f, 0.f, 0.f};
                    if ((lane & 3) == 0 && live) g = philox_normal4(a.seed, a.offset, (uint32_t)r, 0x80000000u + (uint32_t)(j >> 2));
                    const int src = lane & ~3;
                    const float g0 = __shfl(g[0], src, 64), g1 = __shfl(g[1], src, 64);
                    const float g2 = __shfl(g[2], src, 64), g3 = __shfl(g[3], src, 64);
                    const int c = lane & 3;
                    n = c == 0 ? g0 : c == 1 ? g1 : c == 2 ? g2 : g3;
                }
            }
            if (live) {
                const float m = mu[j], l = a.ls_base + ls[j];
                const float x = a.explore ? fmaf(expf(l), n, m) : m;
                logp_column(x, m, l, zz, lss);
                act[j] = x;
                if (a.env_actions) a.env_actions[(size_t)dst * k + j] = fminf(fmaxf(x, a.clip_low), a.clip_high);
                dist[j] = m;
                dist[k + j] = l;
                if (a.explore && a.noise_out) a.noise_out[(size_t)dst * k + j] = n;
            }
        }
        zz = wave_sum(zz); lss = wave_sum(lss);
        if (lane == 0) {
            a.logp[dst] = a.explore ? logp_close(zz, lss, k) : 0.f;
            a.vf[dst] = a.value[r * a.ld_value];
        }
        if (a.eps_dst)
            for (int j = lane; j < a.Z; j += 64) a.eps_dst[(size_t)dst * a.Z + j] = a.eps_src[(size_t)r * a.Z + j];
        if (a.obs_dst)
            for (int j = lane; j < a.n_in; j += 64) a.obs_dst[(size_t)dst * a.n_in + j] = a.obs[(size_t)r * a.n_in + j];
    }
}

// GAE: adv[t] = delta[t] + gamma lambda adv[t + 1] inside a segment, a reverse linear recurrence.  One wavefront per
// segment (wave w takes segments w, w + waves, ...) walks it from its end in 64-row pieces: lane l holds the row l places
// before the piece's last one, the piece is an inclusive wave scan of the pairs (c, delta) under
// (a2, b2) o (a1, b1) = (a1 a2, b2 + a2 b1), and the advantage of the row after the piece is the carry into it.  Segment
// bounds are clamped into [0, n_rows]: a bad table cannot make the kernel touch memory outside the columns.  Every
// workgroup leaves the sums of adv and adv^2 over its waves' rows, in double, in part[block][2]: no atomics, the
// standardisation adds them in block order.
constexpr int kGaeMaxBlocks = 1024;
struct GaeArgs {
    const float* rewards; const float* vpred; const float* last_value;
    const uint8_t* done;                  // null: last_value as given
    const int32_t* seg_start;
    long long n_rows;
    int n_segs;
    float gamma, c;                       // c = gamma lambda
    float* adv; float* vtarg;
    double* part;
};
__global__ void __launch_bounds__(256)
gae_kernel(GaeArgs g) {
    __shared__ double red[4][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wave = blockIdx.x * 4 + wv, waves = gridDim.x * 4;
    double s1 = 0.0, s2 = 0.0;
    for (int s = wave; s < g.n_segs; s += waves) {
        long long a = g.seg_start[s], b = g.seg_start[s + 1];
        a = a < 0 ? 0 : (a > g.n_rows ? g.n_rows : a);
        b = b < a ? a : (b > g.n_rows ? g.n_rows : b);
        if (b <= a) continue;             // (the same for every lane of the wave)
        const float last = (g.done && g.done[s]) ? 0.f : g.last_value[s];
        float carry = 0.f;
        for (long long hi = b; hi > a; hi -= 64) {
            const long long t = hi - 1 - lane;
            const bool live = t >= a;
            float pa = 1.f, pb = 0.f, v = 0.f;
            if (live) {
                v = g.vpred[t];
                const float vn = t + 1 < b ? g.vpred[t + 1] : last;
                pb = g.rewards[t] + g.gamma * vn - v;
                pa = g.c;
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float qa = __shfl_up(pa, o, 64), qb = __shfl_up(pb, o, 64);
                if (lane >= o) { pb = fmaf(pa, qb, pb); pa *= qa; }
            }
            const float x = fmaf(pa, carry, pb);
            carry = __shfl(x, 63, 64);
            if (live) {
                g.adv[t] = x;
                g.vtarg[t] = x + v;
                s1 += (double)x;
                s2 += (double)x * (double)x;
            }
        }
    }
    s1 = wave_sum_d(s1); s2 = wave_sum_d(s2);
    if (lane == 0) { red[wv][0] = s1; red[wv][1] = s2; }
    __syncthreads();
    if (threadIdx.x < 2)
        g.part[(size_t)blockIdx.x * 2 + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// advantages = (adv - mean) / max(1e-4, std), population std: every workgroup adds the GAE launch's partial sums in the
// same order (thread i the partials i, i + 256, ..., then a tree over the threads) and rescales its slice in place
__global__ void __launch_bounds__(256)
gae_standardize_kernel(float* __restrict__ adv, long long n, const double* __restrict__ part, int nparts) {
    __shared__ double sh[2][256];
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int i = tid; i < nparts; i += 256) { a += part[2 * (size_t)i]; b += part[2 * (size_t)i + 1]; }
    sh[0][tid] = a; sh[1][tid] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { sh[0][tid] += sh[0][tid + o]; sh[1][tid] += sh[1][tid + o]; }
        __syncthreads();
    }
    const double mean = sh[0][0] / (double)n;
    double var = sh[1][0] / (double)n - mean * mean;
    if (!(var > 0.0)) var = 0.0;
    const double sd = sqrt(var), inv = 1.0 / (sd > 1e-4 ? sd : 1e-4);
    for (long long i = blockIdx.x * 256ll + tid; i < n; i += gridDim.x * 256ll) adv[i] = (float)(((double)adv[i] - mean) * inv);
}

// ---------------------------------------------------------------------------------------
// minibatch order: every pass's row order from the Philox stream (include/pvae.h "Minibatch order of the PPO learner")
// ---------------------------------------------------------------------------------------
// packed(p, i) = key32(p, i) << 32 | i is unique, so sorting it ascending is the whole job and neither stability nor timing
// can show.  Pass p is its own problem: blockIdx.y, striding by gridDim.y past kOrderMaxY passes.  No atomics, no workgroup
// waits for another: a sort that spans workgroups synchronises at kernel boundaries; every loop's trip count is known at
// launch.  The sizes at which the algorithm changes form:
//   * n <= kOrderTile (8192): ONE launch.  One workgroup per pass forms the keys in LDS (thread q: one Philox call, rows
//     4q .. 4q + 3), sorts them there with a bitonic network and writes the low words to perm.  8192 packed keys are 64 KiB
//     of the CU's 160 KiB (MI355X: LDS per CU), what a workgroup may declare statically.  The network runs over
//     n_pad = max(256, the next power of two >= n) keys, rows >= n holding the all-ones key, which sorts behind every
//     packed one (i < 2^31): the stage count changes at n = 256, 512, 1024, 2048, 4096.
//   * n > kOrderTile: tiles = ceil(n / 8192) workgroups per pass sort one tile each (the last one partial, padded as
//     above) into the scratch's first key buffer, then ceil(log2(tiles)) merge launches double the sorted run, ping-pong
//     between the scratch's two buffers: element i of a run finds its rank in the sibling run by a binary search (<= 31
//     probes) and stores itself at (its place in its own run + that rank) -- a scatter of distinct places, since the keys
//     are unique.  A run without a sibling (an odd run count) is copied.  The LAST merge launch writes the low words to perm.
//     The merge count changes at n = 16384 (2), 32768 (3), 65536 (4), ...; an odd run count first shows at 3 tiles.
constexpr int kOrderTile = 8192;
constexpr int kOrderThreads = 1024;
constexpr int kOrderMinPad = 256;
constexpr int kOrderMaxY = 1024;           // grid rows (passes side by side); more passes: a workgroup strides
constexpr int kOrderMaxX = 4096;           // grid columns of either launch; more tiles / elements: a workgroup strides
struct OrderArgs {
    uint64_t seed, offset;
    long long n, tiles;
    int passes, n_pad;                     // n_pad: the keys a workgroup sorts in LDS, a power of two in [256, 8192]
    const uint64_t* src;                   // merge: the runs
    uint64_t* dst;                         // the packed keys, [passes][n]; null: the low words go to perm
    int32_t* perm;                         // [passes][n]
    int run_shift;                         // merge: sorted runs of 1 << run_shift keys come in
};

// w[0..3](g) of pass p: Philox4x32-10 at counter {offset, g, 0xC0000000 + p}, philox_normal4's key schedule
__device__ inline void order_words(uint32_t (&c)[4], uint64_t seed, uint64_t offset, uint32_t g, uint32_t p) {
    c[0] = (uint32_t)offset; c[1] = (uint32_t)(offset >> 32); c[2] = g; c[3] = 0xC0000000u + p;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

__global__ void __launch_bounds__(kOrderThreads)
ppo_order_tile_kernel(OrderArgs a) {
    __shared__ uint64_t key[kOrderTile];
    const int tid = threadIdx.x, n_pad = a.n_pad;
    for (int p = blockIdx.y; p < a.passes; p += gridDim.y) {
        for (long long t = blockIdx.x; t < a.tiles; t += gridDim.x) {       // (both trip counts: the same for the whole workgroup)
            const long long row0 = t * kOrderTile;
            for (int q = tid; q < n_pad / 4; q += kOrderThreads) {
                const long long i0 = row0 + 4ll * q;
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                if (i0 < a.n) order_words(w, a.seed, a.offset, (uint32_t)(i0 >> 2), (uint32_t)p);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    key[4 * q + c] = i0 + c < a.n ? ((uint64_t)w[c] << 32) | (uint64_t)(i0 + c) : ~0ull;
            }
            __syncthreads();
            for (int k = 2; k <= n_pad; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int u = tid; u < n_pad / 2; u += kOrderThreads) {
                        const int lo = ((u & ~(j - 1)) << 1) | (u & (j - 1)), hi = lo + j;
                        const uint64_t x = key[lo], y = key[hi];
                        if ((x > y) == ((lo & k) == 0)) { key[lo] = y; key[hi] = x; }
                    }
                    __syncthreads();
                }
            const long long live = a.n - row0 < n_pad ? a.n - row0 : n_pad;      // the all-ones keys lie behind them
            const size_t out0 = (size_t)p * (size_t)a.n + (size_t)row0;
            for (int j = tid; j < live; j += kOrderThreads) {
                if (a.dst) a.dst[out0 + j] = key[j];
                else a.perm[out0 + j] = (int32_t)(uint32_t)key[j];
            }
            __syncthreads();                                                   // (the next tile overwrites the keys)
        }
    }
}

__global__ void __launch_bounds__(256)
ppo_order_merge_kernel(OrderArgs a) {
    const long long n = a.n, run = 1ll << a.run_shift;
    for (int p = blockIdx.y; p < a.passes; p += gridDim.y) {
        const uint64_t* __restrict__ src = a.src + (size_t)p * (size_t)n;
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) {
            const uint64_t x = src[i];
            const long long r = i >> a.run_shift, a0 = (r & ~1ll) << a.run_shift;
            const long long mid = a0 + run < n ? a0 + run : n, end = a0 + 2 * run < n ? a0 + 2 * run : n;
            const bool first = i < mid;                                        // i lies in the pair's first run
            const long long s0 = first ? mid : a0;                             // the sibling run: [s0, s1), empty for a lone run
            long long lo = s0, hi = first ? end : mid;
            for (int it = 0; it < 32 && lo < hi; ++it) {                       // (a run has < 2^31 keys)
                const long long m = lo + ((hi - lo) >> 1);
                if (src[m] < x) lo = m + 1; else hi = m;
            }
            const size_t pos = (size_t)p * (size_t)n + (size_t)(a0 + (i - (first ? a0 : mid)) + (lo - s0));
            if (a.dst) a.dst[pos] = x;
            else a.perm[pos] = (int32_t)(uint32_t)x;
        }
    }
}

long long order_tiles(long long n) { return (n + kOrderTile - 1) / kOrderTile; }
int order_merges(long long tiles) {
    int m = 0;
    while ((1ll << m) < tiles) ++m;
    return m;
}
int check_order_sizes(long long n_rows, int passes) {
    if (n_rows < 1 || n_rows > 0x7fffffffll) return fail(-1, "n_rows %lld out of range [1, 2^31)", n_rows);
    if (passes < 1 || passes >= (1 << 30)) return fail(-1, "num_sgd_iter %d out of range [1, 2^30)", passes);
    return 0;
}
// the scratch: nothing but 16 bytes up to one tile; past it two buffers of [passes][n] packed keys, one behind the other
size_t order_scratch_bytes(long long n_rows, int passes) {
    if (n_rows <= kOrderTile) return 16;
    return ((size_t)2 * (size_t)passes * (size_t)n_rows * sizeof(uint64_t) + 15) / 16 * 16;
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
AdamScalars ppo_adam_scalars(const pvae_fc_ppo_params* p, int t) {
    pvae_step_params sp;
    memset(&sp, 0, sizeof(sp));
    sp.lr = p->lr; sp.beta1 = p->beta1; sp.beta2 = p->beta2; sp.adam_eps = p->adam_eps; sp.weight_decay = p->weight_decay;
    sp.adam_t[0] = t;
    return adam_scalars(&sp, 0);
}

// scratch of pvae_ppo_loss (no context to hold one): one small buffer per (device, stream), made at the first call on that
// stream and kept -- calls on one stream are ordered, so they can share it
struct LossScratch { int dev; hipStream_t st; float* p; };
std::vector<LossScratch> g_loss_scratch;
std::mutex g_loss_scratch_mu;
int loss_scratch(hipStream_t st, float** out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_loss_scratch_mu);
    for (const LossScratch& e : g_loss_scratch)
        if (e.dev == dev && e.st == st) { *out = e.p; return 0; }
    float* p = nullptr;
    // (the stats partial rows, then the diagnostics partial rows of pvae_ppo_loss_diag)
    HIP_TRY(hipMalloc((void**)&p, (size_t)4 * kHeadMaxBlocks * (kPartStats + kDiagPart) * sizeof(float)));
    g_loss_scratch.push_back(LossScratch{dev, st, p});
    *out = p;
    return 0;
}

int gae_blocks(int n_segs) {
    const int b = (n_segs + 3) / 4;
    return b > kGaeMaxBlocks ? kGaeMaxBlocks : (b < 1 ? 1 : b);
}
size_t gae_scratch_bytes(int n_segs) { return (size_t)gae_blocks(n_segs) * 2 * sizeof(double); }

}  // namespace

// ---- PPO learner step ----
int head_waves(int rows_pad) {
    int w = (rows_pad + 1) / 2;                       // two rows per wave
    w = (w + 3) / 4 * 4;
    return w > 4 * kHeadMaxBlocks ? 4 * kHeadMaxBlocks : w;
}
int part_stride(int k, bool colsum) { return kPartStats + (colsum ? (k + 3) / 4 * 4 : 0); }
size_t ppo_scratch_bytes(int max_batch, int k) {
    return ((size_t)head_waves(pad32(max_batch)) * part_stride(k, true) * sizeof(float) + 15) / 16 * 16;
}

int check_loss_args(const pvae_fc_ppo_batch* b, const pvae_fc_ppo_params* p, int rows) {
    if (!b || !p) return fail(-1, "null batch or params");
    if (!b->actions || !b->old_dist || !b->old_logp || !b->advantages || !b->value_targets || !b->vf_preds)
        return fail(-1, "a batch column is null");
    if (b->n_rows < 1 || b->n_rows > 0x7fffffffll) return fail(-1, "n_rows %lld out of range", (long long)b->n_rows);
    if (b->k < 1) return fail(-1, "k must be positive");
    if (rows < 1) return fail(-1, "rows must be positive");
    if (p->log_std_kind < 0 || p->log_std_kind > 2) return fail(-1, "log_std_kind %d outside [0, 2]", p->log_std_kind);
    if (!(p->clip_param >= 0.f) || !(p->vf_clip_param >= 0.f)) return fail(-1, "clip_param and vf_clip_param must be >= 0");
    return 0;
}

void fill_head(PpoHead& h, const pvae_fc_ppo_batch* b, const pvae_fc_ppo_params* p, const int32_t* index, long long row0,
               int rows, int rows_pad) {
    memset(&h, 0, sizeof(h));
    h.actions = b->actions; h.old_dist = b->old_dist; h.old_logp = b->old_logp;
    h.adv = b->advantages; h.vtarg = b->value_targets; h.vpred = b->vf_preds;
    h.index = index; h.row0 = row0; h.n_rows = b->n_rows;
    h.rows = rows; h.rows_pad = rows_pad; h.k = b->k;
    h.clip = p->clip_param; h.vf_clip = p->vf_clip_param; h.vf_coeff = p->vf_loss_coeff;
    h.kl_coeff = p->kl_coeff; h.ent_coeff = p->entropy_coeff;
    h.inv_rows = (float)(1.0 / rows);
}

int ppo_head_launch(const PpoHead& h, hipStream_t st) {
    const dim3 grid(head_waves(pad32(h.rows)) / 4);
    if (h.dpart) hipLaunchKernelGGL(ppo_head_kernel<true>, grid, dim3(256), 0, st, h);
    else hipLaunchKernelGGL(ppo_head_kernel<false>, grid, dim3(256), 0, st, h);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- learner diagnostics: the bound buffers ----
size_t ppo_diag_bytes(int max_batch) {
    return (size_t)kDiagSlots * sizeof(double) + (size_t)head_waves(pad32(max_batch)) * kDiagPart * sizeof(float);
}
int ppo_diag_bind(PpoDiag& d, float* diag, int capacity, void* scratch, size_t bytes, int max_batch) {
    if (!diag) { d = PpoDiag(); return 0; }
    if (capacity < 1) return fail(-1, "capacity_steps must be >= 1, got %d", capacity);
    if (!scratch) return fail(-1, "diagnostics scratch is null");
    if ((uintptr_t)scratch & 15) return fail(-1, "diagnostics scratch must be 16-byte aligned");
    if (bytes < ppo_diag_bytes(max_batch)) return fail(-1, "diagnostics scratch too small: %zu < %zu bytes", bytes, ppo_diag_bytes(max_batch));
    d.out = diag; d.capacity = capacity;
    d.gslot = (double*)scratch; d.dpart = (float*)((double*)scratch + kDiagSlots);
    return 0;
}
// ---- gradient clipping: the bound scratch ----
size_t ppo_clip_bytes() { return (size_t)kClipSlots * sizeof(double); }
int ppo_clip_bind(PpoClip& c, float max_norm, void* scratch, size_t bytes) {
    if (!(max_norm >= 0.f) || !std::isfinite(max_norm)) return fail(-1, "max_norm must be finite and >= 0, got %g", (double)max_norm);
    if (max_norm == 0.f && !scratch) { c = PpoClip(); return 0; }
    if (max_norm == 0.f) return fail(-1, "max_norm 0 unbinds: its scratch must be NULL");
    if (!scratch) return fail(-1, "clip scratch is null");
    if ((uintptr_t)scratch & 15) return fail(-1, "clip scratch must be 16-byte aligned");
    if (bytes < ppo_clip_bytes()) return fail(-1, "clip scratch too small: %zu < %zu bytes", bytes, ppo_clip_bytes());
    c.max_norm = max_norm; c.slot = (double*)scratch;
    return 0;
}
static int clip_slots(long long total4) {                 // workgroups of the sum-of-squares launch = slots it fills
    long long grid = (total4 + 255) / 256;
    if (grid > kClipGrid) grid = kClipGrid;
    return (int)grid + 1;
}

// the slots of an Adam launch of `nslots` workgroups added into entry 4 of the row; `a`: that launch's arguments -- with a
// clip, entries 5 and 6 from the clip slots in the same launch
static int ppo_gnorm_launch(const PpoDiagRow& dg, int nslots, const PpoAdam& a, hipStream_t st, int* launches) {
    if (a.cslot)
        hipLaunchKernelGGL(ppo_gnorm_clip_kernel, dim3(1), dim3(128), 0, st, (const double*)dg.gslot, nslots, (const double*)a.cslot,
                           a.ncslots, a.max_norm, dg.row);
    else
        hipLaunchKernelGGL(ppo_gnorm_kernel, dim3(1), dim3(64), 0, st, (const double*)dg.gslot, nslots, dg.row + 4);
    HIP_TRY(hipGetLastError());
    if (launches) ++*launches;
    return 0;
}

// the arguments of the Adam launch in its three forms; returns the float4 elements of all segments
static long long fill_adam(PpoAdam& a, const PpoAdamSegs& segs, const pvae_fc_ppo_params* p, int adam_t, int rows, int k,
                           const float* part, int colsum, float* ls, float* ls_m, float* ls_v, float* stats_out,
                           const PpoDiagRow& dg, const PpoClip& clip = PpoClip()) {
    memset((void*)&a, 0, sizeof(a));
    a.seg = segs;
    long long total4 = 0;
    for (int i = 0; i < segs.n; ++i) { total4 += segs.n4[i]; a.end4[i] = total4; }
    a.s = ppo_adam_scalars(p, adam_t);
    a.part = part; a.nparts = head_waves(pad32(rows)); a.part_stride = part_stride(k, colsum != 0);
    a.inv_rows = (float)(1.0 / rows); a.stats_out = stats_out;
    a.k = k;
    if (colsum) { a.ls = ls; a.ls_m = ls_m; a.ls_v = ls_v; }
    a.dpart = dg.dpart; a.rows = rows; a.diag = dg.row; a.gslot = dg.gslot;
    if (clip.slot) { a.cslot = clip.slot; a.ncslots = clip_slots(total4); a.max_norm = clip.max_norm; }
    return total4;
}

// the sum-of-squares launch of a clipped step: between the backward and the Adam launch (or *_ppo_grad's finish)
int ppo_clip_sumsq_launch(const PpoAdamSegs& segs, const pvae_fc_ppo_params* p, int rows, int k, const float* part, int colsum,
                          float* ls, const PpoClip& clip, hipStream_t st, int* launches) {
    PpoAdam a;
    fill_adam(a, segs, p, 1, rows, k, part, colsum, ls, nullptr, nullptr, nullptr, PpoDiagRow{nullptr, nullptr, nullptr}, clip);
    static_assert(kClipGrid + 1 <= kClipSlots, "one clip slot per workgroup");
    hipLaunchKernelGGL(ppo_clip_sumsq_kernel, dim3(a.ncslots), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    ++*launches;
    return 0;
}

// *_ppo_grad's last launch of a clipped first half: the arena(s) and ls_grad scaled in place (+ diagnostics entries 5, 6)
int ppo_clip_scale_launch(const PpoAdamSegs& segs, const pvae_fc_ppo_params* p, int k, float* ls_grad, int colsum,
                          const PpoClip& clip, const PpoDiagRow& dg, hipStream_t st, int* launches) {
    PpoAdam a;
    const long long total4 = fill_adam(a, segs, p, 1, 1, k, nullptr, colsum, ls_grad, nullptr, nullptr, nullptr, dg, clip);
    long long grid = (total4 + 255) / 256;
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(ppo_clip_scale_kernel, dim3((int)grid + 1), dim3(256), 0, st, a, ls_grad);
    HIP_TRY(hipGetLastError());
    ++*launches;
    return 0;
}

int ppo_adam_launch(const PpoAdamSegs& segs, const pvae_fc_ppo_params* p, int adam_t, int rows, int k, const float* part,
                    int colsum, float* ls, float* ls_m, float* ls_v, float* stats_out, const PpoDiagRow& dg, const PpoClip& clip,
                    hipStream_t st, int* launches) {
    PpoAdam a;
    const long long total4 = fill_adam(a, segs, p, adam_t, rows, k, part, colsum, ls, ls_m, ls_v, stats_out, dg, clip);
    long long grid = (total4 + 255) / 256;
    if (grid > 2048) grid = 2048;
    static_assert(2048 + 1 <= kDiagSlots, "one gradient-norm slot per workgroup");
    const dim3 g((int)grid + 1);
    if (clip.slot) {
        if (dg.row) hipLaunchKernelGGL((ppo_adam_kernel<true, true>), g, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((ppo_adam_kernel<false, true>), g, dim3(256), 0, st, a);
    } else {
        if (dg.row) hipLaunchKernelGGL((ppo_adam_kernel<true, false>), g, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((ppo_adam_kernel<false, false>), g, dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    ++*launches;
    return dg.row ? ppo_gnorm_launch(dg, (int)grid + 1, a, st, launches) : 0;
}

int ppo_grad_finish_launch(int rows, int k, const float* part, int colsum, float* ls_grad, float* stats_out,
                           const PpoDiagRow& dg, hipStream_t st, int* launches) {
    const int nparts = head_waves(pad32(rows)), stride = part_stride(k, colsum != 0);
    if (dg.row)
        hipLaunchKernelGGL(ppo_finish_diag_kernel, dim3(1), dim3(128), 0, st, part, nparts, stride, (float)(1.0 / rows), stats_out,
                           (const float*)dg.dpart, rows, dg.row, 0);
    else
        hipLaunchKernelGGL(ppo_finish_kernel, dim3(1), dim3(64), 0, st, part, nparts, stride, (float)(1.0 / rows), stats_out);
    HIP_TRY(hipGetLastError());
    ++*launches;
    if (colsum) {
        hipLaunchKernelGGL(ppo_ls_grad_kernel, dim3((k + 255) / 256), dim3(256), 0, st, part, nparts, stride, k, ls_grad);
        HIP_TRY(hipGetLastError());
        ++*launches;
    }
    return 0;
}

int ppo_apply_launch(const PpoAdamSegs& segs, const pvae_fc_ppo_params* p, int adam_t, int k, float grad_scale,
                     const float* ls_grad, int colsum, float* ls, float* ls_m, float* ls_v, const PpoDiagRow& dg, hipStream_t st,
                     int* launches) {
    PpoAdam a;
    const long long total4 = fill_adam(a, segs, p, adam_t, 1, k, nullptr, colsum, ls, ls_m, ls_v, nullptr, dg);
    long long grid = (total4 + 255) / 256;
    if (grid > 2048) grid = 2048;
    if (dg.row) hipLaunchKernelGGL(ppo_apply_kernel<true>, dim3((int)grid + 1), dim3(256), 0, st, a, grad_scale, ls_grad);
    else hipLaunchKernelGGL(ppo_apply_kernel<false>, dim3((int)grid + 1), dim3(256), 0, st, a, grad_scale, ls_grad);
    HIP_TRY(hipGetLastError());
    ++*launches;
    return dg.row ? ppo_gnorm_launch(dg, (int)grid + 1, a, st, launches) : 0;
}

int ppo_adam_exchange_launch(PpoPeers& P, long long timeout_ticks, const PpoAdamSegs& segs, const pvae_fc_ppo_params* p,
                             int adam_t, int rows, int k, const float* part, int colsum, float* ls, float* ls_m, float* ls_v,
                             float* stats_out, const PpoDiagRow& dg, const PpoClip& clip, hipStream_t st, int* launches) {
    if (!P.open) return fail(-2, "the PPO gradient exchange is not open");
    if (colsum && k != P.k) return fail(-2, "log-std vector of %d values, the exchange was exported for %d", k, P.k);
    PpoAdam a;
    const long long total4 = fill_adam(a, segs, p, adam_t, rows, k, part, colsum, ls, ls_m, ls_v, stats_out, dg, clip);
    PpoAdamPeers x;
    memset((void*)&x, 0, sizeof(x));
    for (int q = 0; q < P.world; ++q) {
        x.f[q] = P.peer_flags[q];
        for (int r = 0; r < P.n_arenas; ++r) x.arena[r][q] = P.arena[r][q];
    }
    for (int i = 0; i < segs.n; ++i) {
        int r = 0;
        for (; r < P.n_arenas; ++r) {
            const float* base = P.arena[r][P.rank];
            if (segs.g[i] >= base && segs.g[i] + 4 * segs.n4[i] <= base + P.floats[r]) break;
        }
        if (r == P.n_arenas) return fail(-2, "the gradient buffers were re-bound after the exchange was exported");
        // (the kernel addresses a segment through a 32-bit buffer descriptor)
        if (segs.n4[i] >= ((long long)1 << 28)) return fail(-1, "segment of %lld floats: the exchanged launch takes < 2^30", 4 * segs.n4[i]);
        x.seg_arena[i] = r; x.seg_off[i] = segs.g[i] - P.arena[r][P.rank];
    }
    x.me = P.rank; x.epoch = ++P.epoch; x.timeout_ticks = timeout_ticks;
    x.inv_n = (float)(1.0 / P.world);
    long long grid = (total4 + 255) / 256;
    if (grid > kExchangeMaxBlocks) grid = kExchangeMaxBlocks;
    if (grid < 1) grid = 1;
    const dim3 g((int)grid + 1);
    switch (P.world) {
#define PVAE_PPO_PEER_CASE(N)                                                                                              \
    case N:                                                                                                                \
        if (clip.slot) {                                                                                                   \
            if (dg.row) hipLaunchKernelGGL((ppo_adam_exchange_kernel<N, true, true>), g, dim3(256), 0, st, a, x);          \
            else hipLaunchKernelGGL((ppo_adam_exchange_kernel<N, false, true>), g, dim3(256), 0, st, a, x);                \
        } else {                                                                                                           \
            if (dg.row) hipLaunchKernelGGL((ppo_adam_exchange_kernel<N, true, false>), g, dim3(256), 0, st, a, x);         \
            else hipLaunchKernelGGL((ppo_adam_exchange_kernel<N, false, false>), g, dim3(256), 0, st, a, x);               \
        }                                                                                                                  \
        break;
        PVAE_PPO_PEER_CASE(1) PVAE_PPO_PEER_CASE(2) PVAE_PPO_PEER_CASE(3) PVAE_PPO_PEER_CASE(4)
        PVAE_PPO_PEER_CASE(5) PVAE_PPO_PEER_CASE(6) PVAE_PPO_PEER_CASE(7) PVAE_PPO_PEER_CASE(8)
#undef PVAE_PPO_PEER_CASE
        default: return fail(-1, "world %d", P.world);
    }
    HIP_TRY(hipGetLastError());
    ++*launches;
    return dg.row ? ppo_gnorm_launch(dg, (int)grid + 1, a, st, launches) : 0;
}

int check_ppo_buffers(const float* grad, const float* m, const float* v, const void* scratch, const float* log_std,
                      const float* log_std_m, const float* log_std_v) {
    if (((uintptr_t)grad | (uintptr_t)m | (uintptr_t)v | (uintptr_t)scratch) & 15)
        return fail(-1, "grad, m, v and scratch must be 16-byte aligned");
    if ((log_std_m != nullptr) != (log_std_v != nullptr) || (log_std_m && !log_std))
        return fail(-1, "log_std_m and log_std_v go together, with log_std");
    return 0;
}

int zero_rows_launch(const ZeroRows& z, hipStream_t st) {
    int wmax = 0;
    for (int i = 0; i < z.n; ++i) wmax = std::max(wmax, z.width[i]);
    int gx = ((z.r1 - z.r0) * wmax + 255) / 256;
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(ppo_zero_rows_kernel, dim3(gx, z.n), dim3(256), 0, st, z);
    HIP_TRY(hipGetLastError());
    return 0;
}

int pad_copy_launch(const float* src, int n, int rows, float* dst, int ld, int rows_pad, const int32_t* index, long long n_rows,
                    const uint8_t* done, hipStream_t st) {
    int grid = (rows_pad * ld + 255) / 256;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(ppo_pad_copy_kernel, dim3(grid), dim3(256), 0, st, src, n, rows, dst, ld, rows_pad, index, n_rows, done);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- train-batch preparation ----
int ppo_eval_launch(const PpoEval& e, hipStream_t st) {
    int blocks = (e.rows + 3) / 4;
    if (blocks > kEvalMaxBlocks) blocks = kEvalMaxBlocks;
    hipLaunchKernelGGL(ppo_eval_epilogue_kernel, dim3(blocks), dim3(256), 0, st, e);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ppo_act_launch(const PpoAct& a, hipStream_t st) {
    int blocks = (a.rows + 3) / 4;
    if (blocks > kEvalMaxBlocks) blocks = kEvalMaxBlocks;
    hipLaunchKernelGGL(ppo_act_epilogue_kernel, dim3(blocks), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int check_act(const pvae_ppo_act_in* in, const pvae_ppo_act_out* out) {
    if (in->explore != 0 && in->explore != 1) return fail(-1, "explore must be 0 or 1, got %d", in->explore);
    if (in->n_dst_rows < 1 || in->n_dst_rows > 0x7fffffffll) return fail(-1, "n_dst_rows %lld out of range", (long long)in->n_dst_rows);
    if (!in->out_row && in->n_dst_rows < in->n_rows)
        return fail(-1, "n_dst_rows %lld < n_rows %lld without out_row", (long long)in->n_dst_rows, (long long)in->n_rows);
    if (in->clip != 0 && in->clip != 1) return fail(-1, "clip must be 0 or 1, got %d", in->clip);
    if ((in->clip != 0) != (out->env_actions != nullptr)) return fail(-1, "clip and env_actions go together: both or neither");
    if (in->clip && !(in->clip_low <= in->clip_high)) return fail(-1, "clip_low %g > clip_high %g", in->clip_low, in->clip_high);
    return 0;
}

void act_as_evaluate(const pvae_ppo_act_in* in, const pvae_ppo_act_out* out, pvae_fc_rollout& ro, pvae_fc_prepared& ev) {
    memset(&ro, 0, sizeof(ro));
    ro.obs = in->obs; ro.actions = out->actions; ro.n_rows = in->n_rows; ro.k = in->k;
    memset(&ev, 0, sizeof(ev));
    ev.vf_preds = out->vf_preds; ev.old_dist = out->old_dist; ev.old_logp = out->old_logp;
}

void fill_act(PpoAct& a, const PpoPanels& pan, const pvae_ppo_act_in* in, const pvae_ppo_act_out* out, long long first,
              uint64_t chunk, int n_in) {
    memset((void*)&a, 0, sizeof(a));
    static_cast<PpoPanels&>(a) = pan;
    a.noise = in->explore && in->noise ? in->noise + (size_t)first * in->k : nullptr;
    a.out_row = in->out_row ? in->out_row + first : nullptr;
    a.row0 = first; a.n_dst_rows = in->n_dst_rows;
    a.explore = in->explore; a.clip = in->clip; a.clip_low = in->clip_low; a.clip_high = in->clip_high;
    a.seed = in->rng_seed; a.offset = in->rng_offset + chunk;
    a.actions = out->actions; a.env_actions = in->clip ? out->env_actions : nullptr;
    a.dist = out->old_dist; a.logp = out->old_logp; a.vf = out->vf_preds; a.noise_out = out->noise_out;
    a.obs = in->obs + (size_t)first * n_in; a.obs_dst = out->obs_dst; a.n_in = n_in;
}

int check_gae_params(const pvae_gae_params* p) {
    if (!p) return fail(-1, "null params");
    if (!(p->gamma >= 0.f && p->gamma <= 1.f) || !(p->lambda >= 0.f && p->lambda <= 1.f))
        return fail(-1, "gamma and lambda must lie in [0, 1]");
    return 0;
}

int check_segments(long long n_rows, int n_segs, long long seg_first, long long seg_last) {
    if (n_rows < 1 || n_rows > 0x7fffffffll) return fail(-1, "n_rows %lld out of range", n_rows);
    if (n_segs < 1) return fail(-1, "n_segs must be >= 1, got %d", n_segs);
    if (n_segs > n_rows) return fail(-1, "n_segs %d > n_rows %lld: a segment has at least one row", n_segs, n_rows);
    if (seg_first != 0 || seg_last != n_rows)
        return fail(-1, "seg_start must run from 0 to n_rows %lld, got %lld .. %lld", n_rows, seg_first, seg_last);
    return 0;
}

int check_gae_scratch(const void* scratch, size_t bytes, int n_segs) {
    if (!scratch) return fail(-1, "scratch is null");
    if ((uintptr_t)scratch & 15) return fail(-1, "scratch must be 16-byte aligned");
    if (bytes < gae_scratch_bytes(n_segs)) return fail(-1, "scratch too small: %zu < %zu bytes", bytes, gae_scratch_bytes(n_segs));
    return 0;
}

// the GAE launch and, with `standardize`, the rescale launch (arguments checked by the caller); `launches` counts them
int run_gae(const float* rewards, const float* vpred, const float* last_value, const uint8_t* done, const int32_t* seg_start,
            long long n_rows, int n_segs, const pvae_gae_params* p, float* adv, float* vtarg, void* scratch, hipStream_t st,
            int& launches) {
    GaeArgs g;
    memset(&g, 0, sizeof(g));
    g.rewards = rewards; g.vpred = vpred; g.last_value = last_value; g.done = done; g.seg_start = seg_start;
    g.n_rows = n_rows; g.n_segs = n_segs; g.gamma = p->gamma; g.c = p->gamma * p->lambda;
    g.adv = adv; g.vtarg = vtarg; g.part = (double*)scratch;
    const int blocks = gae_blocks(n_segs);
    hipLaunchKernelGGL(gae_kernel, dim3(blocks), dim3(256), 0, st, g);
    HIP_TRY(hipGetLastError());
    ++launches;
    if (p->standardize) {
        long long grid = (n_rows + 255) / 256;
        if (grid > 1024) grid = 1024;
        hipLaunchKernelGGL(gae_standardize_kernel, dim3((int)grid), dim3(256), 0, st, adv, n_rows, (const double*)scratch, blocks);
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    return 0;
}

int check_boot(const pvae_fc_rollout* ro, const pvae_fc_prepared* out) {
    if (ro->n_segs < 1) return fail(-1, "n_segs must be >= 1, got %d", ro->n_segs);
    if (!ro->boot_obs || !ro->seg_done) return fail(-1, "rollout boot_obs or seg_done is null");
    if (!out->last_value) return fail(-1, "last_value is null");
    return 0;
}


// pvae_ppo_loss and pvae_ppo_loss_diag (diag_out != NULL: the head's DIAG instantiation and the two-wave finish)
static int ppo_loss_run(const float* mean, const float* log_std, int64_t log_std_row_stride, const float* value,
                        const pvae_fc_ppo_batch* b, const int32_t* index, int32_t rows, const pvae_fc_ppo_params* p,
                        float* d_mean, float* d_log_std, float* d_value, float* stats_out, float* diag_out, void* stream) {
    int rc = check_loss_args(b, p, rows);
    if (rc) return rc;
    if (!mean || !log_std || !value) return fail(-1, "mean, log_std or value is null");
    if (!d_mean || !d_log_std || !d_value || !stats_out) return fail(-1, "an output is null");
    if (log_std_row_stride < 0) return fail(-1, "log_std_row_stride must be >= 0");
    if (!index && rows > b->n_rows) return fail(-1, "rows %d > n_rows %lld without an index", rows, (long long)b->n_rows);
    hipStream_t st = (hipStream_t)stream;
    float* part = nullptr;
    if ((rc = loss_scratch(st, &part))) return rc;
    const int k = b->k, waves = head_waves(pad32(rows));      // (the fused step's row -> wave map: the same stats bits)
    PpoHead h;
    fill_head(h, b, p, index, 0, rows, rows);
    h.mean = mean; h.ld_mean = k; h.ls = log_std; h.ld_ls = log_std_row_stride; h.value = value; h.ld_value = 1;
    h.d_mean = d_mean; h.ld_dm = k; h.width_dm = k;
    h.d_ls = d_log_std; h.ld_dls = k; h.width_dls = k;
    h.d_value = d_value; h.ld_dv = 1; h.width_dv = 1;
    h.part = part; h.part_stride = kPartStats; h.colsum = 0;
    if (diag_out) h.dpart = part + (size_t)4 * kHeadMaxBlocks * kPartStats;
    if ((rc = ppo_head_launch(h, st))) return rc;
    if (diag_out)
        hipLaunchKernelGGL(ppo_finish_diag_kernel, dim3(1), dim3(128), 0, st, (const float*)part, waves, (int)kPartStats, h.inv_rows,
                           stats_out, (const float*)h.dpart, (int)rows, diag_out, 1);
    else
        hipLaunchKernelGGL(ppo_finish_kernel, dim3(1), dim3(64), 0, st, part, waves, kPartStats, h.inv_rows, stats_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

int pvae_ppo_loss(const float* mean, const float* log_std, int64_t log_std_row_stride, const float* value,
                  const pvae_fc_ppo_batch* b, const int32_t* index, int32_t rows, const pvae_fc_ppo_params* p,
                  float* d_mean, float* d_log_std, float* d_value, float* stats_out, void* stream) {
    return ppo_loss_run(mean, log_std, log_std_row_stride, value, b, index, rows, p, d_mean, d_log_std, d_value, stats_out, nullptr,
                        stream);
}

int pvae_ppo_loss_diag(const float* mean, const float* log_std, int64_t log_std_row_stride, const float* value,
                       const pvae_fc_ppo_batch* b, const int32_t* index, int32_t rows, const pvae_fc_ppo_params* p,
                       float* d_mean, float* d_log_std, float* d_value, float* stats_out, float* diag_out, void* stream) {
    if (!diag_out) return fail(-1, "diag_out is null");
    return ppo_loss_run(mean, log_std, log_std_row_stride, value, b, index, rows, p, d_mean, d_log_std, d_value, stats_out, diag_out,
                        stream);
}

size_t pvae_fc_gae_workspace_bytes(int32_t n_segs) {
    if (n_segs < 1) { fail(-1, "n_segs must be >= 1, got %d", n_segs); return 0; }
    return (gae_scratch_bytes(n_segs) + 15) / 16 * 16;
}

int pvae_gae_sizeof(int which) {
    return which == 0 ? (int)sizeof(pvae_gae_params) : which == 1 ? (int)sizeof(pvae_fc_rollout)
         : which == 2 ? (int)sizeof(pvae_fc_prepared) : fail(-1, "which must be 0, 1 or 2");
}

int pvae_gae(const float* rewards, const float* vf_preds, const float* last_values, const int32_t* seg_start,
             const uint8_t* seg_done, int64_t n_rows, int32_t n_segs, int64_t seg_first, int64_t seg_last,
             const pvae_gae_params* p, float* advantages, float* value_targets, void* scratch, size_t scratch_bytes,
             void* stream) {
    int rc = check_gae_params(p);
    if (rc) return rc;
    if (!rewards || !vf_preds || !last_values || !seg_start) return fail(-1, "rewards, vf_preds, last_values or seg_start is null");
    if (!advantages || !value_targets) return fail(-1, "an output is null");
    if ((rc = check_segments(n_rows, n_segs, seg_first, seg_last))) return rc;
    if ((rc = check_gae_scratch(scratch, scratch_bytes, n_segs))) return rc;
    int launches = 0;
    if ((rc = run_gae(rewards, vf_preds, last_values, seg_done, seg_start, n_rows, n_segs, p, advantages, value_targets, scratch,
                      (hipStream_t)stream, launches)))
        return rc;
    return launches;
}

size_t pvae_ppo_order_workspace_bytes(int64_t n_rows, int32_t num_sgd_iter) {
    if (check_order_sizes(n_rows, num_sgd_iter)) return 0;
    if (n_rows > kOrderTile && (uint64_t)num_sgd_iter > (UINT64_MAX / 32) / (uint64_t)n_rows) {
        fail(-1, "%d passes over %lld rows: the packed keys do not fit a size_t", num_sgd_iter, (long long)n_rows);
        return 0;
    }
    return order_scratch_bytes(n_rows, num_sgd_iter);
}

int pvae_ppo_order(int64_t n_rows, int32_t num_sgd_iter, uint64_t seed, uint64_t offset, int32_t* perm, void* scratch,
                   size_t scratch_bytes, void* stream) {
    const size_t need = pvae_ppo_order_workspace_bytes(n_rows, num_sgd_iter);
    if (!need) return -1;
    if (!perm) return fail(-1, "perm is null");
    if ((uintptr_t)perm & 3) return fail(-1, "perm must be 4-byte aligned");
    if (!scratch) return fail(-1, "scratch is null");
    if ((uintptr_t)scratch & 15) return fail(-1, "scratch must be 16-byte aligned");
    if (scratch_bytes < need) return fail(-1, "scratch too small: %zu < %zu bytes", scratch_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    OrderArgs a;
    memset((void*)&a, 0, sizeof(a));
    a.seed = seed; a.offset = offset; a.n = n_rows; a.passes = num_sgd_iter; a.perm = perm;
    a.tiles = order_tiles(n_rows);
    a.n_pad = kOrderMinPad;
    while (a.n_pad < kOrderTile && a.n_pad < n_rows) a.n_pad <<= 1;
    const int merges = order_merges(a.tiles);
    uint64_t* buf[2] = {(uint64_t*)scratch, (uint64_t*)scratch + (size_t)num_sgd_iter * (size_t)n_rows};
    const int gy = num_sgd_iter < kOrderMaxY ? num_sgd_iter : kOrderMaxY;
    a.dst = merges ? buf[0] : nullptr;
    hipLaunchKernelGGL(ppo_order_tile_kernel, dim3((int)std::min<long long>(a.tiles, kOrderMaxX), gy), dim3(kOrderThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    const int gx = (int)std::min<long long>((n_rows + 255) / 256, kOrderMaxX);
    for (int m = 0; m < merges; ++m) {
        a.src = buf[m & 1];
        a.dst = m == merges - 1 ? nullptr : buf[(m + 1) & 1];
        a.run_shift = 13 + m;
        hipLaunchKernelGGL(ppo_order_merge_kernel, dim3(gx, gy), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    static_assert(kOrderTile == 1 << 13, "run_shift of the first merge");
    return 1 + merges;
}

}  // extern "C"
