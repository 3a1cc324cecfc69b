// pvae_fc.hip -- the stack set (include/pvae.h pvae_fc_*): S fully connected stacks on one shared input, run TOGETHER.
// FullyConnectedPolicy (rmt:323-457) is two or three small stacks (256x2 / 64x2) on the same observation; at those sizes a
// launch boundary (~2.85 us) outweighs a layer's arithmetic, so every layer depth is one launch for all stacks:
//   forward    copy-in | layer 0 of all stacks as ONE GEMM over the concatenated output features | per deeper depth one
//              grouped launch, workgroup index -> (stack, tile)
//   backward   copy-in | the forward again | one seed launch | per depth, last to first, one grouped launch holding the
//              input-gradient tiles, the weight-gradient tiles and the bias sums of every participating stack | the first-
//              layer launch: ONE input-gradient GEMM (its contraction over the concatenated features is the sum over the
//              stacks) + the stacks' weight gradients | copy-out of dx
// The tile bodies are those of pvae_gemm.h (register-staged 32x32 / 16x16 forward and input-gradient bodies, the weight-
// gradient bodies, the bias sums), on (pointer, ld) operands into the arena of pvae_fc_layout.h; a group launch only
// decides which body a workgroup runs and on which operands.  A problem's tile geometry depends on the problem alone,
// never on what shares its launch, so the per-stack schedule (option "fc_per_stack") gives the same bits.
#include "pvae_internal.h"
#include "pvae_fc_layout.h"

#include <mutex>

struct pvae_fc {
    FcLayout L;
    FcWork W;
    float* params = nullptr;
    float* ws = nullptr;
    int fwd_launches = 0, bwd_launches = 0;
    // PPO learner step (pvae_fc_ppo_bind)
    float* grad = nullptr;
    float* m = nullptr;
    float* v = nullptr;
    float* scratch = nullptr;
    float* log_std = nullptr;
    float* log_std_m = nullptr;
    float* log_std_v = nullptr;
    int ppo_launches = 0;
    int eval_launches = 0, gae_launches = 0;      // pvae_fc_ppo_prepare / pvae_fc_ppo_evaluate (pvae_fc_gae_launches)
};

namespace {

constexpr int kS = PVAE_FC_MAX_STACKS;

// ---------------------------------------------------------------------------------------
// glue kernels
// ---------------------------------------------------------------------------------------
// batch row of minibatch row r: index[r] clamped into [0, n_rows) (a bad entry must not read out of bounds), or row0 + r
__device__ inline long long batch_row(const int32_t* __restrict__ index, long long row0, long long n_rows, int r) {
    if (!index) return row0 + r;
    const long long i = index[r];
    return i < 0 ? 0 : (i >= n_rows ? n_rows - 1 : i);
}

// dst[rows_pad][ld] = zero-padded copy of dense src[rows][n]; with `index` (the PPO step) of the rows src[index[r]]
__global__ void __launch_bounds__(256)
fc_pad_copy_kernel(const float* __restrict__ src, int n, int rows, float* __restrict__ dst, int ld, int rows_pad,
                   const int32_t* __restrict__ index, long long n_rows) {
    const int total = rows_pad * ld;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / ld, c = idx - r * ld;
        dst[idx] = (r < rows && c < n) ? src[(size_t)batch_row(index, 0, n_rows, r) * n + c] : 0.f;
    }
}

// dst[rows][n] (dense) = src[rows][0:n] of a panel with row stride ld
__global__ void __launch_bounds__(256)
fc_copy_out_kernel(const float* __restrict__ src, int ld, float* __restrict__ dst, int n, int rows) {
    const int total = rows * n;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / n, c = idx - r * n;
        dst[idx] = src[(size_t)r * ld + c];
    }
}

// Output gradients of all stacks in one launch (autograd of rmt:434-438): dz[r][c] = dy[r][c] (linear output layers), written
// over the WHOLE [rows_pad][width] block of each stack's last gradient panel -- pad rows and pad columns get zeros, so
// nothing an earlier call left there reaches a contraction.  dy == NULL: zeros everywhere (the first-layer columns of a stack
// without a gradient that lie inside the one input-gradient GEMM).  blockIdx.y = entry.
struct FcSeed {
    const float* dy[kS];
    float* dz[kS];
    int n[kS], width[kS], ld[kS];
    int rows, rows_pad;
};
__global__ void __launch_bounds__(256)
fc_seed_kernel(FcSeed a) {
    const int s = blockIdx.y;
    const float* __restrict__ dy = a.dy[s];
    float* __restrict__ dz = a.dz[s];
    const int n = a.n[s], width = a.width[s], ld = a.ld[s];
    const int total = a.rows_pad * width;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / width, c = idx - r * width;
        dz[(size_t)r * ld + c] = (dy && r < a.rows && c < n) ? dy[(size_t)r * n + c] : 0.f;
    }
}

// Rows [r0, r1) of the layer-output panels set to zero: a <= 4-row forward runs on the GEMV kernels, which write the live
// rows only, while the backward contractions read whole 32-row tiles (a stale NaN in a pad row would meet a zero gradient
// row and the product is NaN).  blockIdx.y = panel.
constexpr int kZeroPanels = 1 + kS * PVAE_MAX_HIDDEN;
struct FcZeroRows {
    float* p[kZeroPanels];
    int ld[kZeroPanels], width[kZeroPanels];
    int r0, r1;
};
__global__ void __launch_bounds__(256)
fc_zero_rows_kernel(FcZeroRows z) {
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
// forward epilogue: out = act(acc + bias) per COLUMN SEGMENT (the concatenated first layers: every stack's block has its
// own activation and its own real width), pad columns forced to 0 (so padding never reaches a weight gradient, also where
// act(0) != 0), and -- an output layer -- the live rows and real columns stored to the caller's dense result as well
// ---------------------------------------------------------------------------------------
struct EpiFc {
    float* out;
    int ldo;
    const float* bias;
    int nseg, rows;
    int end[kS];              // segment s = columns [end[s-1], end[s])
    int act[kS];              // act_apply code of the segment
    int valid[kS];            // first pad column of the segment
    float* dense[kS];         // dense[rows][ldd] destination of the segment's real columns (null: none)
    int ldd[kS];
    struct Pre { v4f b; };
    __device__ inline Pre preload(int, int p) const { return Pre{*reinterpret_cast<const v4f*>(bias + p)}; }
    __device__ inline void operator()(int q, int p, v4f v, const Pre& pre) const {
        int a = act[0], nv = valid[0], c0 = 0, ld_d = ldd[0];
        float* d = dense[0];
#pragma unroll
        for (int s = 1; s < kS; ++s)
            if (s < nseg && p >= end[s - 1]) { a = act[s]; nv = valid[s]; c0 = end[s - 1]; d = dense[s]; ld_d = ldd[s]; }
        v += pre.b;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = p + e < nv ? act_apply(v[e], a) : 0.f;
        store_stream(out + (size_t)q * ldo + p, v);
        if (d && q < rows) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p + e < nv) d[(size_t)q * ld_d + (p - c0) + e] = v[e];
        }
    }
    __device__ inline void finish(float*, int, int) const {}
};

// ---------------------------------------------------------------------------------------
// grouped launches
// ---------------------------------------------------------------------------------------
// forward, tile path: workgroups [end[k-1], end[k]) run problem k on the register-staged 32x32 body or, for narrow
// problems (GemmArgs::tile16), the 16x16 body -- both 256 threads, 32 KB of LDS
struct FcFwdGroup {
    int n;
    int end[kS];
    GemmArgs ga[kS];
    EpiFc e[kS];
};
__global__ void __launch_bounds__(256)
fc_forward_group_kernel(FcFwdGroup g) {
    __shared__ __attribute__((aligned(16))) float lds[kRegRingFloats];
    const int b = blockIdx.x;
    int k = 0;
    while (k + 1 < g.n && b >= g.end[k]) ++k;
    const int lo = k ? g.end[k - 1] : 0;
    const GemmArgs ga = g.ga[k];
    EpiFc e = g.e[k];
    if (ga.tile16) splitk_reg16_body<true, EpiFc>(lds, b - lo, ga, e);
    else splitk_reg_body<true, EpiFc, 0>(lds, b - lo, ga, e);
}

// forward, rows <= 4: the arithmetic of gemv_rows_kernel (pvae.hip) -- one wave per output feature streams its weight row
// once with float4 loads, lanes split K and combine with a shuffle tree -- over the layers of one depth of all stacks
struct FcGemvProb {
    const float* x; const float* W; const float* bias;
    float* out; float* dense;
    int ldx, ldw, ldo, ldd, K, act, n_valid;
};
struct FcGemvGroup {
    int n, rows;              // rows: live rows (R may exceed them: the surplus rows stay inside the panels)
    int end[kS];
    FcGemvProb p[kS];
};
template <int R>
__global__ void __launch_bounds__(256)
fc_gemv_group_kernel(FcGemvGroup g) {
    const int b = blockIdx.x;
    int k = 0;
    while (k + 1 < g.n && b >= g.end[k]) ++k;
    const FcGemvProb pr = g.p[k];
    const int n = (b - (k ? g.end[k - 1] : 0)) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const float* __restrict__ wrow = pr.W + (size_t)n * pr.ldw;
    const float* __restrict__ x = pr.x;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    for (int kk = lane * 4; kk < pr.K; kk += 256) {
        const v4f wv = *reinterpret_cast<const v4f*>(wrow + kk);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const v4f xv = *reinterpret_cast<const v4f*>(x + (size_t)r * pr.ldx + kk);
            acc[r] = fmaf(wv.x, xv.x, fmaf(wv.y, xv.y, fmaf(wv.z, xv.z, fmaf(wv.w, xv.w, acc[r]))));
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float v = acc[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) {
            v = n < pr.n_valid ? act_apply(v + pr.bias[n], pr.act) : 0.f;
            pr.out[(size_t)r * pr.ldo + n] = v;
            if (pr.dense && r < g.rows && n < pr.n_valid) pr.dense[(size_t)r * pr.ldd + n] = v;
        }
    }
}

// backward: input-gradient problems first (their workgroups are dispatched first, as in bwd_pair_kernel: it is the input
// gradient whose reduction + store epilogue hides under the partner's MFMAs), then the weight-gradient problems, then the
// bias sums of the weight-gradient problems.  end[] holds the running workgroup count over those nd + 2 nw segments.
template <class EpiW>
struct FcBwdGroup {
    int nd, nw;
    int end[3 * kS];
    GemmArgs gd[kS];
    EpiMask ed[kS];
    GemmArgs gw[kS];
    EpiW ew[kS];
};
template <class EpiW>
__global__ void __launch_bounds__(256)
fc_backward_group_kernel(FcBwdGroup<EpiW> g) {
    __shared__ __attribute__((aligned(16))) float lds[kPairLdsFloats];
    const int b = blockIdx.x, nseg = g.nd + 2 * g.nw;
    int k = 0;
    while (k + 1 < nseg && b >= g.end[k]) ++k;
    const int lb = b - (k ? g.end[k - 1] : 0);
    if (k < g.nd) {
        const GemmArgs gd = g.gd[k];
        EpiMask ed = g.ed[k];
        if (gd.tile16) splitk_reg16_body<false, EpiMask>(lds, lb, gd, ed);
        else splitk_reg_body<false, EpiMask, 0>(lds, lb, gd, ed);
    } else if (k < g.nd + g.nw) {
        const GemmArgs gw = g.gw[k - g.nd];
        EpiW ew = g.ew[k - g.nd];
        wgrad_body<EpiW>(lds, lb, gw, ew);
    } else {
        const GemmArgs gw = g.gw[k - g.nd - g.nw];
        EpiW ew = g.ew[k - g.nd - g.nw];
        bias_grad_body(lds, lb, gw, ew);
    }
}

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
struct PpoHead {
    const float* mean; const float* ls; const float* value;       // row r at r * ld_*: panels or dense tensors
    long long ld_mean, ld_ls, ld_value;
    float ls_base;
    const float* actions; const float* old_dist; const float* old_logp;
    const float* adv; const float* vtarg; const float* vpred;
    const int32_t* index; long long row0, n_rows;
    int rows, rows_pad, k;
    float clip, vf_clip, vf_coeff, kl_coeff, ent_coeff, inv_rows;
    float* d_mean; float* d_ls; float* d_value;                  // [rows_pad][width_*] blocks, row stride ld_d* (null: none)
    int ld_dm, ld_dls, ld_dv, width_dm, width_dls, width_dv;
    float* part; int part_stride; int colsum;                    // partial rows [waves][part_stride]; colsum: + the log-std columns
};
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__global__ void __launch_bounds__(256)
fc_ppo_head_kernel(PpoHead h) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), waves = gridDim.x * 4;
    const int k = h.k;
    float* __restrict__ part = h.part + (size_t)wave * h.part_stride;
    if (h.colsum)
        for (int j = lane; j < k; j += 64) part[kPartStats + j] = 0.f;
    float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r = wave; r < h.rows_pad; r += waves) {
        const bool live = r < h.rows;
        float dlogp = 0.f, dval = 0.f;
        const float* mu = nullptr; const float* ls = nullptr; const float* act = nullptr; const float* od = nullptr;
        if (live) {
            const long long br = batch_row(h.index, h.row0, h.n_rows, r);
            mu = h.mean + r * h.ld_mean; ls = h.ls + r * h.ld_ls;
            act = h.actions + br * k; od = h.old_dist + br * 2 * k;
            float zz = 0.f, lss = 0.f, kl = 0.f;
            for (int j = lane; j < k; j += 64) {
                const float l = h.ls_base + ls[j], inv_sig = expf(-l);
                const float z = (act[j] - mu[j]) * inv_sig, d = od[j] - mu[j], lo = od[k + j];
                zz = fmaf(z, z, zz);
                lss += l;
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
    }
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

// Adam over the trained segments of the arena (adam_update4 with the AdamScalars the trainer's adam_flat_kernel gets:
// the same bits) + ONE extra workgroup, the last: the stats and, for a state-independent log-std, that vector's gradient
// (the column sums, added in partial-row order) and its Adam update.
constexpr int kAdamSegs = 3 * kS;
struct FcAdam {
    float* p; const float* g; float* m; float* v;
    int nseg;
    long long off4[kAdamSegs], end4[kAdamSegs];     // float4 offset of segment i; running float4 count through segment i
    AdamScalars s;
    const float* part; int nparts, part_stride; float inv_rows; float* stats_out;
    int k; float* ls; float* ls_m; float* ls_v;     // ls null: no trained log-std vector
};
__global__ void __launch_bounds__(256)
fc_adam_kernel(FcAdam a) {
    if (blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x < 64) ppo_finish(a.part, a.nparts, a.part_stride, a.inv_rows, a.stats_out, threadIdx.x);
        if (a.ls)
            for (int j = threadIdx.x; j < a.k; j += 256) {
                double gs = 0.0;               // (a few hundred signed terms per column: in double, so that the order does not show)
                for (int i = 0; i < a.nparts; ++i) gs += (double)a.part[(size_t)i * a.part_stride + kPartStats + j];
                const float g = (float)gs;
                float p = a.ls[j], m = a.ls_m[j], v = a.ls_v[j];
                adam_update(g, p, m, v, a.s);
                a.ls[j] = p; a.ls_m[j] = m; a.ls_v[j] = v;
            }
        return;
    }
    const long long n4 = a.nseg ? a.end4[a.nseg - 1] : 0;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (gridDim.x - 1) * 256ll) {
        int k = 0;
        while (i >= a.end4[k]) ++k;
        const long long q = a.off4[k] + (i - (k ? a.end4[k - 1] : 0));
        v4f pp = reinterpret_cast<v4f*>(a.p)[q];
        const v4f gg = reinterpret_cast<const v4f*>(a.g)[q];
        v4f mm = reinterpret_cast<v4f*>(a.m)[q];
        v4f vv = reinterpret_cast<v4f*>(a.v)[q];
        adam_update4(gg, pp, mm, vv, a.s);
        reinterpret_cast<v4f*>(a.p)[q] = pp;
        reinterpret_cast<v4f*>(a.m)[q] = mm;
        reinterpret_cast<v4f*>(a.v)[q] = vv;
    }
}

// fc_adam_kernel over segments of up to three DIFFERENT arenas (the PhysicsVAE step: the encoder's and the decoder's
// segments of the five-net arena and the value stack set's arena, each with its own gradient and moment buffers): the
// same adam_update4 per element, the same last workgroup for the stats and the log-std vector.
struct PpoAdam {
    PpoAdamSegs seg;
    long long end4[3];                              // running float4 count through segment i
    AdamScalars s;
    const float* part; int nparts, part_stride; float inv_rows; float* stats_out;
    int k; float* ls; float* ls_m; float* ls_v;
};
__global__ void __launch_bounds__(256)
ppo_adam_kernel(PpoAdam a) {
    if (blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x < 64) ppo_finish(a.part, a.nparts, a.part_stride, a.inv_rows, a.stats_out, threadIdx.x);
        if (a.ls)
            for (int j = threadIdx.x; j < a.k; j += 256) {
                double gs = 0.0;
                for (int i = 0; i < a.nparts; ++i) gs += (double)a.part[(size_t)i * a.part_stride + kPartStats + j];
                const float g = (float)gs;
                float p = a.ls[j], m = a.ls_m[j], v = a.ls_v[j];
                adam_update(g, p, m, v, a.s);
                a.ls[j] = p; a.ls_m[j] = m; a.ls_v[j] = v;
            }
        return;
    }
    const long long n4 = a.seg.n ? a.end4[a.seg.n - 1] : 0;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (gridDim.x - 1) * 256ll) {
        int k = 0;
        while (i >= a.end4[k]) ++k;
        const long long q = i - (k ? a.end4[k - 1] : 0);
        v4f pp = reinterpret_cast<v4f*>(a.seg.p[k])[q];
        const v4f gg = reinterpret_cast<const v4f*>(a.seg.g[k])[q];
        v4f mm = reinterpret_cast<v4f*>(a.seg.m[k])[q];
        v4f vv = reinterpret_cast<v4f*>(a.seg.v[k])[q];
        adam_update4(gg, pp, mm, vv, a.s);
        reinterpret_cast<v4f*>(a.seg.p[k])[q] = pp;
        reinterpret_cast<v4f*>(a.seg.m[k])[q] = mm;
        reinterpret_cast<v4f*>(a.seg.v[k])[q] = vv;
    }
}

// ---------------------------------------------------------------------------------------
// train-batch preparation: evaluate epilogue, GAE, standardisation (include/pvae.h "Train-batch preparation")
// ---------------------------------------------------------------------------------------
// input panel of the bootstrap pass: fc_pad_copy_kernel, except that row r of a segment that ended its episode (done[r])
// is zeros and its source row is never read
__global__ void __launch_bounds__(256)
fc_boot_copy_kernel(const float* __restrict__ src, int n, int rows, float* __restrict__ dst, int ld, int rows_pad,
                    const uint8_t* __restrict__ done) {
    const int total = rows_pad * ld;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / ld, c = idx - r * ld;
        dst[idx] = (r < rows && c < n && !done[r]) ? src[(size_t)r * n + c] : 0.f;
    }
}

// The epilogue of one evaluated chunk: a wave per row reads the stacks' outputs in their panels and writes vf[r],
// dist[r] = [mean | log_std] and logp[r] of actions[r] -- the arithmetic of fc_ppo_head_kernel's logp, term for term, so
// that the learner's first step sees a ratio of exactly 1.  mean == NULL: the bootstrap use -- the value stack ran alone;
// vf[r] = done[r] ? 0 : value[r].  The output pointers are those of the chunk's first row.  eps_dst (PhysicsVAE's evaluate
// pass): the latent draws of the chunk, eps_src [rows][Z], copied to the caller's rows.
constexpr int kEvalMaxBlocks = 1024;
struct FcEval {
    const float* mean; const float* ls; const float* value;
    long long ld_mean, ld_ls, ld_value;
    float ls_base;
    const float* actions;
    const uint8_t* done;
    int rows, k;
    float* vf; float* dist; float* logp;
    const float* eps_src; float* eps_dst; int Z;
};
__global__ void __launch_bounds__(256)
fc_eval_epilogue_kernel(FcEval e) {
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
            const float l = e.ls_base + ls[j], inv_sig = expf(-l);
            const float z = (act[j] - mu[j]) * inv_sig;
            zz = fmaf(z, z, zz);
            lss += l;
            dist[j] = mu[j];
            dist[k + j] = l;
        }
        zz = wave_sum(zz); lss = wave_sum(lss);
        if (lane == 0) {
            e.logp[r] = -0.5f * zz - lss - 0.5f * k * 1.8378770664093453f;                  // log(2 pi)
            e.vf[r] = e.value[r * e.ld_value];
        }
        if (e.eps_dst)
            for (int j = lane; j < e.Z; j += 64) e.eps_dst[(size_t)r * e.Z + j] = e.eps_src[(size_t)r * e.Z + j];
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
__device__ inline double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__global__ void __launch_bounds__(256)
fc_gae_kernel(GaeArgs g) {
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
fc_standardize_kernel(float* __restrict__ adv, long long n, const double* __restrict__ part, int nparts) {
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
// host side
// ---------------------------------------------------------------------------------------
struct Run {
    pvae_fc* c;
    hipStream_t st;
    int rows, rows_pad;
    int launches = 0;
    bool want[kS] = {};       // the stack runs
    int s_lo = 0, s_hi = 0;   // first-layer range: first and last stack that runs
};

float* act_ptr(const pvae_fc* c, int s, int i) {
    return i == 0 ? c->ws + c->W.act0 + c->L.stack[s][0].col0 : c->ws + c->W.act[s][i];
}
float* dz_ptr(const pvae_fc* c, int s, int i) {
    return i == 0 ? c->ws + c->W.dz0 + c->L.stack[s][0].col0 : c->ws + c->W.dz[s][i];
}
int panel_ld(const pvae_fc* c, int s, int i) { return i == 0 ? c->L.n0 : c->L.stack[s][i].n_out_pad; }

struct FwdProb { GemmArgs ga; EpiFc e; int grid; };

// forward problem out[M][N] = act(X W^T + b); `t16`: 16x16 tiles
FwdProb fwd_prob(const float* X, int ldx, const float* W, int ldw, int M, int N, int K, bool t16, const EpiFc& e) {
    const GemmGrid g = t16 ? make_grid(M, N, 16, 16) : make_grid(M, N, 32, 32);
    FwdProb p{GemmArgs{X, ldx, W, ldw, K, g.tiles_q, g.tiles_p, g.p_per_xcd}, e, g.grid};
    p.ga.krot = 0; p.ga.rowxcd = 0;
    p.ga.tile16 = t16 ? 1 : 0;
    return p;
}

int launch_fwd(Run& r, const std::vector<FwdProb>& probs) {
    const size_t per = g_fc_per_stack ? 1 : probs.size();
    for (size_t i0 = 0; i0 < probs.size(); i0 += per) {
        FcFwdGroup g;
        memset(&g, 0, sizeof(g));
        int total = 0;
        for (size_t i = i0; i < i0 + per && i < probs.size(); ++i) {
            g.ga[g.n] = probs[i].ga;
            g.e[g.n] = probs[i].e;
            total += probs[i].grid;
            g.end[g.n++] = total;
        }
        hipLaunchKernelGGL(fc_forward_group_kernel, dim3(total), dim3(256), 0, r.st, g);
        HIP_TRY(hipGetLastError());
        ++r.launches;
    }
    return 0;
}

int launch_gemv(Run& r, const std::vector<FcGemvProb>& probs, const std::vector<int>& blocks) {
    const size_t per = g_fc_per_stack ? 1 : probs.size();
    for (size_t i0 = 0; i0 < probs.size(); i0 += per) {
        FcGemvGroup g;
        memset(&g, 0, sizeof(g));
        g.rows = r.rows;
        int total = 0;
        for (size_t i = i0; i < i0 + per && i < probs.size(); ++i) {
            g.p[g.n] = probs[i];
            total += blocks[i];
            g.end[g.n++] = total;
        }
        if (r.rows == 1) hipLaunchKernelGGL((fc_gemv_group_kernel<1>), dim3(total), dim3(256), 0, r.st, g);
        else if (r.rows == 2) hipLaunchKernelGGL((fc_gemv_group_kernel<2>), dim3(total), dim3(256), 0, r.st, g);
        else hipLaunchKernelGGL((fc_gemv_group_kernel<4>), dim3(total), dim3(256), 0, r.st, g);
        HIP_TRY(hipGetLastError());
        ++r.launches;
    }
    return 0;
}

int copy_in(Run& r, const float* x, const int32_t* index = nullptr, long long n_rows = 0) {
    const pvae_fc* c = r.c;
    int grid = (r.rows_pad * c->L.ld0 + 255) / 256;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(fc_pad_copy_kernel, dim3(grid), dim3(256), 0, r.st, x, c->L.cfg.n_in, r.rows, c->ws + c->W.in,
                       c->L.ld0, r.rows_pad, index, n_rows);
    HIP_TRY(hipGetLastError());
    ++r.launches;
    return 0;
}

// the layers of the stacks that run, depth by depth; `dense` (may be null, as may its entries): the callers' results
int run_forward(Run& r, float* const* dense) {
    pvae_fc* c = r.c;
    const FcLayout& L = c->L;
    const float* in = c->ws + c->W.in;
    const bool gemv = r.rows <= 4;
    // (the first layers' tile geometry is decided on the WHOLE shared block, whichever stacks run and however they are
    //  launched: a stack's first layer gives the same bits alone, in a range, or in the full block)
    const bool t16_0 = forward_uses_16x16(r.rows_pad, L.n0);
    for (int i = 0; i < L.max_layers; ++i) {
        std::vector<FwdProb> tp;
        std::vector<FcGemvProb> gp;
        std::vector<int> gb;
        if (i == 0 && !gemv && !g_fc_per_stack) {
            // ONE GEMM over the concatenated output features of the stacks s_lo .. s_hi
            const FcLayer& a = L.stack[r.s_lo][0];
            EpiFc e;
            memset(&e, 0, sizeof(e));
            e.out = c->ws + c->W.act0 + a.col0; e.ldo = L.n0; e.bias = c->params + a.b_off; e.rows = r.rows;
            int N = 0;
            for (int s = r.s_lo; s <= r.s_hi; ++s) {
                const FcLayer& l = L.stack[s][0];
                const int k = e.nseg++;
                e.act[k] = l.act; e.valid[k] = N + l.n_out; e.end[k] = N + l.n_out_pad;
                if (l.last && dense && dense[s] && r.want[s]) { e.dense[k] = dense[s]; e.ldd[k] = l.n_out; }
                N += l.n_out_pad;
            }
            tp.push_back(fwd_prob(in, L.ld0, c->params + a.w_off, L.ld0, r.rows_pad, N, L.ld0, t16_0, e));
        } else {
            for (int s = 0; s < L.S; ++s) {
                if (!r.want[s] || i >= (int)L.stack[s].size()) continue;
                const FcLayer& l = L.stack[s][i];
                const float* x = i == 0 ? in : act_ptr(c, s, i - 1);
                const int ldx = i == 0 ? L.ld0 : panel_ld(c, s, i - 1);
                float* d = (l.last && dense) ? dense[s] : nullptr;
                if (gemv) {
                    gp.push_back(FcGemvProb{x, c->params + l.w_off, c->params + l.b_off, act_ptr(c, s, i), d, ldx, l.ld,
                                            panel_ld(c, s, i), l.n_out, l.ld, l.act, l.n_out});
                    gb.push_back(l.n_out_pad / 4);
                } else {
                    EpiFc e;
                    memset(&e, 0, sizeof(e));
                    e.out = act_ptr(c, s, i); e.ldo = panel_ld(c, s, i); e.bias = c->params + l.b_off; e.rows = r.rows;
                    e.nseg = 1; e.act[0] = l.act; e.valid[0] = l.n_out; e.end[0] = l.n_out_pad;
                    e.dense[0] = d; e.ldd[0] = l.n_out;
                    const bool t16 = i == 0 ? t16_0 : forward_uses_16x16(r.rows_pad, l.n_out_pad);
                    tp.push_back(fwd_prob(x, ldx, c->params + l.w_off, l.ld, r.rows_pad, l.n_out_pad, l.ld, t16, e));
                }
            }
        }
        int rc = 0;
        if (!tp.empty() && (rc = launch_fwd(r, tp))) return rc;
        if (!gp.empty() && (rc = launch_gemv(r, gp, gb))) return rc;
    }
    return 0;
}

struct DProb { GemmArgs ga; EpiMask e; int grid; };
template <class EpiW> struct WProb { GemmArgs ga; EpiW e; int grid, nbias; };

DProb d_prob(const float* dZ, int ldz, const float* W, int ldw, int M, int Kin, int N, const EpiMask& e) {
    DgradPlan d = plan_dgrad(dZ, ldz, W, ldw, M, Kin, N);
    d.ga.krot = 0; d.ga.rowxcd = 0;
    return DProb{d.ga, e, d.grid};
}
template <class EpiW>
WProb<EpiW> w_prob(const float* dZ, int ldz, const float* X, int ldx, int N, int Kin, int M, float* g, float* gb) {
    WgradPlan w = plan_wgrad(dZ, ldz, X, ldx, N, Kin, M);
    w.ga.krot = 0; w.ga.rowxcd = 0;
    EpiW e{g, Kin};
    e.gb = gb;
    return WProb<EpiW>{w.ga, e, w.grid, w.nbias};
}

template <class EpiW>
int launch_bwd_one(Run& r, const DProb* d, int nd, const WProb<EpiW>* w, int nw) {
    if (nd + nw == 0) return 0;
    FcBwdGroup<EpiW> g;
    memset((void*)&g, 0, sizeof(g));
    int total = 0, k = 0;
    g.nd = nd; g.nw = nw;
    for (int i = 0; i < nd; ++i) { g.gd[i] = d[i].ga; g.ed[i] = d[i].e; total += d[i].grid; g.end[k++] = total; }
    for (int i = 0; i < nw; ++i) { g.gw[i] = w[i].ga; g.ew[i] = w[i].e; total += w[i].grid; g.end[k++] = total; }
    for (int i = 0; i < nw; ++i) { total += w[i].nbias; g.end[k++] = total; }
    hipLaunchKernelGGL((fc_backward_group_kernel<EpiW>), dim3(total), dim3(256), 0, r.st, g);
    HIP_TRY(hipGetLastError());
    ++r.launches;
    return 0;
}

// One layer depth of the backward pass.  `stack_of_*`: which stack a problem belongs to (the per-stack schedule launches a
// stack's input gradient and weight gradient together, as the trainer's same-layer pairs do; -1: the shared first-layer
// input gradient, a launch of its own there).
template <class EpiW>
int launch_bwd(Run& r, const std::vector<DProb>& d, const std::vector<int>& stack_of_d, const std::vector<WProb<EpiW>>& w,
               const std::vector<int>& stack_of_w) {
    if (!g_fc_per_stack) return launch_bwd_one<EpiW>(r, d.data(), (int)d.size(), w.data(), (int)w.size());
    int rc = 0;
    for (size_t i = 0; i < d.size(); ++i)
        if (stack_of_d[i] < 0 && (rc = launch_bwd_one<EpiW>(r, &d[i], 1, nullptr, 0))) return rc;
    for (int s = 0; s < kS; ++s) {
        const DProb* dp = nullptr;
        const WProb<EpiW>* wp = nullptr;
        for (size_t i = 0; i < d.size(); ++i) if (stack_of_d[i] == s) dp = &d[i];
        for (size_t i = 0; i < w.size(); ++i) if (stack_of_w[i] == s) wp = &w[i];
        if ((rc = launch_bwd_one<EpiW>(r, dp, dp ? 1 : 0, wp, wp ? 1 : 0))) return rc;
    }
    return 0;
}

template <class EpiW>
int run_backward_layers(Run& r, bool want_dx, float* grad, int grad_mask) {
    pvae_fc* c = r.c;
    const FcLayout& L = c->L;
    const int M = r.rows_pad;
    for (int i = L.max_layers - 1; i >= 1; --i) {
        std::vector<DProb> d;
        std::vector<WProb<EpiW>> w;
        std::vector<int> sd, sw;
        for (int s = 0; s < L.S; ++s) {
            if (!r.want[s] || i >= (int)L.stack[s].size()) continue;
            const FcLayer& l = L.stack[s][i];
            const bool train = grad && ((grad_mask >> s) & 1);
            if (train || want_dx) {          // (a stack that runs has one of the two: dz of the layer below feeds them)
                const EpiMask e{dz_ptr(c, s, i - 1), panel_ld(c, s, i - 1), act_ptr(c, s, i - 1), panel_ld(c, s, i - 1),
                                L.stack[s][i - 1].act};
                d.push_back(d_prob(dz_ptr(c, s, i), panel_ld(c, s, i), c->params + l.w_off, l.ld, M, l.ld, l.n_out_pad, e));
                sd.push_back(s);
            }
            if (train) {
                w.push_back(w_prob<EpiW>(dz_ptr(c, s, i), panel_ld(c, s, i), act_ptr(c, s, i - 1), panel_ld(c, s, i - 1),
                                         l.n_out_pad, l.ld, M, grad + l.w_off, grad + l.b_off));
                sw.push_back(s);
            }
        }
        int rc = launch_bwd<EpiW>(r, d, sd, w, sw);
        if (rc) return rc;
    }
    // first layers: ONE input-gradient GEMM over the concatenated features of s_lo .. s_hi + the stacks' weight gradients
    std::vector<DProb> d;
    std::vector<WProb<EpiW>> w;
    std::vector<int> sd, sw;
    if (want_dx) {
        const FcLayer& a = L.stack[r.s_lo][0];
        int N = 0;
        for (int s = r.s_lo; s <= r.s_hi; ++s) N += L.stack[s][0].n_out_pad;
        const EpiMask e{c->ws + c->W.d_in, L.ld0, nullptr, 0, 0};
        d.push_back(d_prob(c->ws + c->W.dz0 + a.col0, L.n0, c->params + a.w_off, L.ld0, M, L.ld0, N, e));
        sd.push_back(-1);
    }
    for (int s = 0; s < L.S; ++s) {
        if (!r.want[s] || !(grad && ((grad_mask >> s) & 1))) continue;
        const FcLayer& l = L.stack[s][0];
        w.push_back(w_prob<EpiW>(dz_ptr(c, s, 0), L.n0, c->ws + c->W.in, L.ld0, l.n_out_pad, L.ld0, M, grad + l.w_off,
                                 grad + l.b_off));
        sw.push_back(s);
    }
    return launch_bwd<EpiW>(r, d, sd, w, sw);
}

// GEMV path (rows <= 4): the pad rows of the layer outputs are not written by the forward; zero them for the contractions
int zero_pad_rows(Run& r) {
    pvae_fc* c = r.c;
    const FcLayout& L = c->L;
    const int rows = r.rows;
    if (!(rows <= 4 && rows < r.rows_pad)) return 0;
    {
        FcZeroRows z;
        memset(&z, 0, sizeof(z));
        int n = 0, wmax = L.n0;
        z.p[n] = c->ws + c->W.act0; z.ld[n] = L.n0; z.width[n] = L.n0; ++n;
        for (int s = 0; s < L.S; ++s)
            for (int i = 1; r.want[s] && i < (int)L.stack[s].size(); ++i) {
                z.p[n] = act_ptr(c, s, i); z.ld[n] = z.width[n] = L.stack[s][i].n_out_pad;
                if (z.width[n] > wmax) wmax = z.width[n];
                ++n;
            }
        z.r0 = rows; z.r1 = r.rows_pad;
        int gx = ((z.r1 - z.r0) * wmax + 255) / 256;
        if (gx > 64) gx = 64;
        hipLaunchKernelGGL(fc_zero_rows_kernel, dim3(gx, n), dim3(256), 0, r.st, z);
        HIP_TRY(hipGetLastError());
        ++r.launches;
    }
    return 0;
}

int check_call(pvae_fc* c, const float* x, int rows) {
    if (!c) return fail(-1, "null stack set");
    if (!c->params || !c->ws) return fail(-2, "pvae_fc_bind has not been called");
    if (!x) return fail(-1, "x is null");
    if (rows < 1 || rows > c->L.cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, c->L.cfg.max_batch);
    return 0;
}

void set_range(Run& r, int S) {
    r.s_lo = -1;
    for (int s = 0; s < S; ++s)
        if (r.want[s]) { if (r.s_lo < 0) r.s_lo = s; r.s_hi = s; }
}


// ---- PPO learner step, host side ----
int head_waves(int rows_pad) {
    int w = (rows_pad + 1) / 2;                       // two rows per wave
    w = (w + 3) / 4 * 4;
    return w > 4 * kHeadMaxBlocks ? 4 * kHeadMaxBlocks : w;
}
int part_stride(int k, bool colsum) { return kPartStats + (colsum ? (k + 3) / 4 * 4 : 0); }
size_t ppo_scratch_floats(const FcLayout& L) {
    return (size_t)head_waves(pad32(L.cfg.max_batch)) * part_stride(L.cfg.n_out[0], true);
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
    HIP_TRY(hipMalloc((void**)&p, (size_t)4 * kHeadMaxBlocks * kPartStats * sizeof(float)));
    g_loss_scratch.push_back(LossScratch{dev, st, p});
    *out = p;
    return 0;
}

int check_ppo(pvae_fc* c, const pvae_fc_ppo_batch* b, const pvae_fc_ppo_params* p, long long first, int rows, const float* stats) {
    if (!c) return fail(-1, "null stack set");
    if (!c->params || !c->ws) return fail(-2, "pvae_fc_bind has not been called");
    if (!c->grad || !c->m || !c->v || !c->scratch) return fail(-2, "pvae_fc_ppo_bind has not been called");
    int rc = check_loss_args(b, p, rows);
    if (rc) return rc;
    if (!b->obs) return fail(-1, "batch obs is null");
    if (!stats) return fail(-1, "stats_out is null");
    const FcLayout& L = c->L;
    if (L.S < 2 || L.S > 3) return fail(-1, "a PPO step needs [policy, value] or [policy, value, log-std] stacks, got %d", L.S);
    if (L.cfg.n_out[1] != 1) return fail(-1, "stacks in the wrong order: stack 1 must be the value function (n_out 1, got %d)", L.cfg.n_out[1]);
    if (L.S == 3 && L.cfg.n_out[2] != L.cfg.n_out[0])
        return fail(-1, "stacks in the wrong order: the log-std stack (2) must be as wide as the policy stack (0)");
    if ((p->log_std_kind == 2) != (L.S == 3)) return fail(-1, "log_std_kind %d does not fit %d stacks", p->log_std_kind, L.S);
    if (b->k != L.cfg.n_out[0]) return fail(-1, "batch k %d != policy outputs %d", b->k, L.cfg.n_out[0]);
    if (p->log_std_kind != 2 && !c->log_std) return fail(-2, "log_std vector not bound (pvae_fc_ppo_bind)");
    if (p->log_std_kind == 1 && (!c->log_std_m || !c->log_std_v)) return fail(-2, "log_std moments not bound (pvae_fc_ppo_bind)");
    if (rows > L.cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, L.cfg.max_batch);
    if (first < 0 || first + rows > b->n_rows) return fail(-1, "rows [%lld, +%d) outside the batch of %lld", first, rows, (long long)b->n_rows);
    if (p->adam_t < 1) return fail(-1, "adam_t must be >= 1");
    if (p->train_mask < 0 || p->train_mask >= (1 << L.S)) return fail(-1, "train_mask names a stack that does not exist");
    return 0;
}

// one minibatch (arguments checked by the caller)
int ppo_step(pvae_fc* c, const pvae_fc_ppo_batch* b, const int32_t* index, long long first, int rows,
             const pvae_fc_ppo_params* p, int adam_t, float* stats_out, hipStream_t st) {
    const FcLayout& L = c->L;
    const int mask = p->train_mask ? p->train_mask : (1 << L.S) - 1;
    Run r{c, st, rows, pad32(rows)};
    for (int s = 0; s < L.S; ++s) r.want[s] = true;
    set_range(r, L.S);
    int rc;
    if (index) rc = copy_in(r, b->obs, index + first, b->n_rows);
    else rc = copy_in(r, b->obs + (size_t)first * L.cfg.n_in);
    if (rc) return rc;
    if ((rc = zero_pad_rows(r))) return rc;
    if ((rc = run_forward(r, nullptr))) return rc;
    const bool colsum = p->log_std_kind == 1;
    const int waves = head_waves(r.rows_pad), stride = part_stride(b->k, colsum);
    {
        PpoHead h;
        fill_head(h, b, p, index ? index + first : nullptr, first, rows, r.rows_pad);
        const int lp = (int)L.stack[0].size() - 1, lv = (int)L.stack[1].size() - 1;
        h.mean = act_ptr(c, 0, lp); h.ld_mean = panel_ld(c, 0, lp);
        h.value = act_ptr(c, 1, lv); h.ld_value = panel_ld(c, 1, lv);
        if (p->log_std_kind == 2) {
            const int ll = (int)L.stack[2].size() - 1;
            h.ls = act_ptr(c, 2, ll); h.ld_ls = panel_ld(c, 2, ll); h.ls_base = p->log_std_base;
            if ((mask >> 2) & 1) { h.d_ls = dz_ptr(c, 2, ll); h.ld_dls = panel_ld(c, 2, ll); h.width_dls = L.stack[2][ll].n_out_pad; }
        } else {
            h.ls = c->log_std; h.ld_ls = 0;
        }
        if (mask & 1) { h.d_mean = dz_ptr(c, 0, lp); h.ld_dm = panel_ld(c, 0, lp); h.width_dm = L.stack[0][lp].n_out_pad; }
        if (mask & 2) { h.d_value = dz_ptr(c, 1, lv); h.ld_dv = panel_ld(c, 1, lv); h.width_dv = L.stack[1][lv].n_out_pad; }
        h.part = c->scratch; h.part_stride = stride; h.colsum = colsum;
        hipLaunchKernelGGL(fc_ppo_head_kernel, dim3(waves / 4), dim3(256), 0, st, h);
        HIP_TRY(hipGetLastError());
        ++r.launches;
    }
    for (int s = 0; s < L.S; ++s) r.want[s] = (mask >> s) & 1;
    if ((rc = run_backward_layers<EpiGradStore>(r, false, c->grad, mask))) return rc;
    {
        FcAdam a;
        memset((void*)&a, 0, sizeof(a));
        a.p = c->params; a.g = c->grad; a.m = c->m; a.v = c->v;
        // the trained stacks' parts of the arena, in arena order, adjacent ones merged
        std::vector<std::pair<long long, long long>> seg;
        auto add = [&](long long off, long long n) {
            if (!seg.empty() && seg.back().first + seg.back().second == off) seg.back().second += n;
            else seg.push_back({off, n});
        };
        for (int s = 0; s < L.S; ++s)
            if ((mask >> s) & 1) add(L.stack[s][0].w_off, (long long)L.stack[s][0].n_out_pad * L.stack[s][0].ld);
        for (int s = 0; s < L.S; ++s)
            if ((mask >> s) & 1) add(L.stack[s][0].b_off, L.stack[s][0].n_out_pad);
        for (int s = 0; s < L.S; ++s)
            for (size_t i = 1; ((mask >> s) & 1) && i < L.stack[s].size(); ++i) {
                add(L.stack[s][i].w_off, (long long)L.stack[s][i].n_out_pad * L.stack[s][i].ld);
                add(L.stack[s][i].b_off, L.stack[s][i].n_out_pad);
            }
        long long total4 = 0;
        for (const auto& sg : seg) {
            if (a.nseg == kAdamSegs) return fail(-3, "the trained parts of the arena form more than %d segments", kAdamSegs);
            a.off4[a.nseg] = sg.first / 4;
            total4 += sg.second / 4;
            a.end4[a.nseg++] = total4;
        }
        a.s = ppo_adam_scalars(p, adam_t);
        a.part = c->scratch; a.nparts = waves; a.part_stride = stride; a.inv_rows = (float)(1.0 / rows); a.stats_out = stats_out;
        a.k = b->k;
        if (colsum) { a.ls = c->log_std; a.ls_m = c->log_std_m; a.ls_v = c->log_std_v; }
        long long grid = (total4 + 255) / 256;
        if (grid > 2048) grid = 2048;
        hipLaunchKernelGGL(fc_adam_kernel, dim3((int)grid + 1), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
        ++r.launches;
    }
    c->ppo_launches = r.launches;
    return 0;
}

// ---- train-batch preparation, host side ----
int gae_blocks(int n_segs) {
    const int b = (n_segs + 3) / 4;
    return b > kGaeMaxBlocks ? kGaeMaxBlocks : (b < 1 ? 1 : b);
}
size_t gae_scratch_bytes(int n_segs) { return (size_t)gae_blocks(n_segs) * 2 * sizeof(double); }

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
    hipLaunchKernelGGL(fc_gae_kernel, dim3(blocks), dim3(256), 0, st, g);
    HIP_TRY(hipGetLastError());
    ++launches;
    if (p->standardize) {
        long long grid = (n_rows + 255) / 256;
        if (grid > 1024) grid = 1024;
        hipLaunchKernelGGL(fc_standardize_kernel, dim3((int)grid), dim3(256), 0, st, adv, n_rows, (const double*)scratch, blocks);
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    return 0;
}

// what evaluate and prepare ask of the stack set; `rows_pass`: the policy's distribution is evaluated (its log-std is needed)
int check_eval(pvae_fc* c, const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out, bool rows_pass) {
    if (!c) return fail(-1, "null stack set");
    if (!ro || !p || !out) return fail(-1, "null rollout, params or outputs");
    if (!c->params || !c->ws) return fail(-2, "pvae_fc_bind has not been called");
    const FcLayout& L = c->L;
    if (L.S < 2 || L.S > 3) return fail(-1, "a PPO learner needs [policy, value] or [policy, value, log-std] stacks, got %d", L.S);
    if (L.cfg.n_out[1] != 1) return fail(-1, "stacks in the wrong order: stack 1 must be the value function (n_out 1, got %d)", L.cfg.n_out[1]);
    if (L.S == 3 && L.cfg.n_out[2] != L.cfg.n_out[0])
        return fail(-1, "stacks in the wrong order: the log-std stack (2) must be as wide as the policy stack (0)");
    if (ro->n_rows < 1 || ro->n_rows > 0x7fffffffll) return fail(-1, "n_rows %lld out of range", (long long)ro->n_rows);
    if (rows_pass) {
        if (p->log_std_kind < 0 || p->log_std_kind > 2) return fail(-1, "log_std_kind %d outside [0, 2]", p->log_std_kind);
        if ((p->log_std_kind == 2) != (L.S == 3)) return fail(-1, "log_std_kind %d does not fit %d stacks", p->log_std_kind, L.S);
        if (ro->k != L.cfg.n_out[0]) return fail(-1, "rollout k %d != policy outputs %d", ro->k, L.cfg.n_out[0]);
        if (p->log_std_kind != 2 && !c->log_std) return fail(-2, "log_std vector not bound (pvae_fc_ppo_bind)");
        if (!ro->obs || !ro->actions) return fail(-1, "rollout obs or actions is null");
        if (!out->vf_preds || !out->old_dist || !out->old_logp) return fail(-1, "an evaluate output (vf_preds, old_dist, old_logp) is null");
    }
    return 0;
}

int check_boot(const pvae_fc_rollout* ro, const pvae_fc_prepared* out) {
    if (ro->n_segs < 1) return fail(-1, "n_segs must be >= 1, got %d", ro->n_segs);
    if (!ro->boot_obs || !ro->seg_done) return fail(-1, "rollout boot_obs or seg_done is null");
    if (!out->last_value) return fail(-1, "last_value is null");
    return 0;
}

void fill_eval_value(FcEval& e, const pvae_fc* c) {
    const int lv = (int)c->L.stack[1].size() - 1;
    e.value = act_ptr(c, 1, lv); e.ld_value = panel_ld(c, 1, lv);
}

int launch_eval_epilogue(Run& r, const FcEval& e) {
    int blocks = (e.rows + 3) / 4;
    if (blocks > kEvalMaxBlocks) blocks = kEvalMaxBlocks;
    hipLaunchKernelGGL(fc_eval_epilogue_kernel, dim3(blocks), dim3(256), 0, r.st, e);
    HIP_TRY(hipGetLastError());
    ++r.launches;
    return 0;
}

// rows of the rollout through all stacks in chunks of max_batch: copy-in, one launch per depth, the epilogue
int eval_rows(pvae_fc* c, const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out, hipStream_t st,
              int& launches) {
    const FcLayout& L = c->L;
    const int k = ro->k;
    for (long long first = 0; first < ro->n_rows; first += L.cfg.max_batch) {
        const int rows = (int)(ro->n_rows - first < L.cfg.max_batch ? ro->n_rows - first : L.cfg.max_batch);
        Run r{c, st, rows, pad32(rows)};
        for (int s = 0; s < L.S; ++s) r.want[s] = true;
        set_range(r, L.S);
        int rc;
        if ((rc = copy_in(r, ro->obs + (size_t)first * L.cfg.n_in))) return rc;
        if ((rc = run_forward(r, nullptr))) return rc;
        FcEval e;
        memset(&e, 0, sizeof(e));
        const int lp = (int)L.stack[0].size() - 1;
        e.mean = act_ptr(c, 0, lp); e.ld_mean = panel_ld(c, 0, lp);
        fill_eval_value(e, c);
        if (p->log_std_kind == 2) {
            const int ll = (int)L.stack[2].size() - 1;
            e.ls = act_ptr(c, 2, ll); e.ld_ls = panel_ld(c, 2, ll); e.ls_base = p->log_std_base;
        } else {
            e.ls = c->log_std; e.ld_ls = 0;
        }
        e.actions = ro->actions + (size_t)first * k;
        e.rows = rows; e.k = k;
        e.vf = out->vf_preds + first; e.dist = out->old_dist + (size_t)first * 2 * k; e.logp = out->old_logp + first;
        if ((rc = launch_eval_epilogue(r, e))) return rc;
        launches += r.launches;
    }
    return 0;
}

// last_value[s] = seg_done[s] ? 0 : value(boot_obs[s]): the value stack alone, in chunks of max_batch
int eval_boot(pvae_fc* c, const pvae_fc_rollout* ro, const pvae_fc_prepared* out, hipStream_t st, int& launches) {
    const FcLayout& L = c->L;
    for (int first = 0; first < ro->n_segs; first += L.cfg.max_batch) {
        const int rows = ro->n_segs - first < L.cfg.max_batch ? ro->n_segs - first : L.cfg.max_batch;
        Run r{c, st, rows, pad32(rows)};
        r.want[1] = true;
        set_range(r, L.S);
        int rc;
        if ((rc = ppo_boot_copy_launch(ro->boot_obs + (size_t)first * L.cfg.n_in, L.cfg.n_in, rows, c->ws + c->W.in, L.ld0,
                                       r.rows_pad, ro->seg_done + first, st)))
            return rc;
        ++r.launches;
        if ((rc = run_forward(r, nullptr))) return rc;
        FcEval e;
        memset(&e, 0, sizeof(e));
        fill_eval_value(e, c);
        e.done = ro->seg_done + first;
        e.rows = rows; e.k = ro->k;
        e.vf = out->last_value + first;
        if ((rc = launch_eval_epilogue(r, e))) return rc;
        launches += r.launches;
    }
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// what the PPO learner step of PhysicsVAE (pvae_ppo.hip) runs of this unit (pvae_internal.h)
// ---------------------------------------------------------------------------------------
int fc_value_stack(pvae_fc* c, FcValueStack* out) {
    if (!c) return fail(-1, "null value stack set");
    if (!c->params || !c->ws) return fail(-2, "value stack set: pvae_fc_bind has not been called");
    if (!c->grad || !c->m || !c->v) return fail(-2, "value stack set: pvae_fc_ppo_bind has not been called");
    const FcLayout& L = c->L;
    if (L.S != 1 || L.cfg.n_out[0] != 1) return fail(-1, "the value stack set must be one stack with one output, got %d stacks", L.S);
    const int lv = (int)L.stack[0].size() - 1;
    memset(out, 0, sizeof(*out));
    out->in = c->ws + c->W.in; out->ld_in = L.ld0; out->n_in = L.cfg.n_in;
    out->value = act_ptr(c, 0, lv); out->ld_value = panel_ld(c, 0, lv);
    out->d_value = dz_ptr(c, 0, lv); out->ld_dv = panel_ld(c, 0, lv); out->width_dv = L.stack[0][lv].n_out_pad;
    out->params = c->params; out->grad = c->grad; out->m = c->m; out->v = c->v;
    out->arena_floats = L.arena_floats;
    out->max_batch = L.cfg.max_batch;
    for (int i = 0; i <= lv; ++i) {
        out->panel[i] = act_ptr(c, 0, i);
        out->panel_ld[i] = panel_ld(c, 0, i);
    }
    out->n_panels = lv + 1;
    return 0;
}

int fc_value_forward(pvae_fc* c, int rows, hipStream_t st, int* launches) {
    Run r{c, st, rows, pad32(rows)};
    r.want[0] = true;
    set_range(r, 1);
    const int rc = run_forward(r, nullptr);
    *launches += r.launches;
    return rc;
}

int fc_value_backward(pvae_fc* c, int rows, hipStream_t st, int* launches) {
    Run r{c, st, rows, pad32(rows)};
    r.want[0] = true;
    set_range(r, 1);
    const int rc = run_backward_layers<EpiGradStore>(r, false, c->grad, 1);
    *launches += r.launches;
    return rc;
}

int ppo_eval_launch(const PpoEvalIo& io, hipStream_t st) {
    FcEval e;
    memset(&e, 0, sizeof(e));
    e.mean = io.mean; e.ld_mean = io.ld_mean; e.ls = io.ls; e.ld_ls = 0; e.value = io.value; e.ld_value = io.ld_value;
    e.actions = io.actions; e.done = io.done; e.rows = io.rows; e.k = io.k;
    e.vf = io.vf; e.dist = io.dist; e.logp = io.logp;
    e.eps_src = io.eps_src; e.eps_dst = io.eps_dst; e.Z = io.Z;
    Run r{nullptr, st, io.rows, pad32(io.rows)};
    return launch_eval_epilogue(r, e);
}

int ppo_boot_copy_launch(const float* src, int n, int rows, float* dst, int ld, int rows_pad, const uint8_t* done, hipStream_t st) {
    int grid = (rows_pad * ld + 255) / 256;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(fc_boot_copy_kernel, dim3(grid), dim3(256), 0, st, src, n, rows, dst, ld, rows_pad, done);
    HIP_TRY(hipGetLastError());
    return 0;
}

int gae_check_params(const pvae_gae_params* p) { return check_gae_params(p); }
int gae_check_boot(const pvae_fc_rollout* ro, const pvae_fc_prepared* out) { return check_boot(ro, out); }
int gae_check_segments(long long n_rows, int n_segs, long long seg_first, long long seg_last) {
    return check_segments(n_rows, n_segs, seg_first, seg_last);
}
int gae_check_scratch(const void* scratch, size_t bytes, int n_segs) { return check_gae_scratch(scratch, bytes, n_segs); }

int gae_launch(const float* rewards, const float* vpred, const float* last_value, const int32_t* seg_start, long long n_rows,
               int n_segs, const pvae_gae_params* p, float* adv, float* vtarg, void* scratch, hipStream_t st, int* launches) {
    return run_gae(rewards, vpred, last_value, nullptr, seg_start, n_rows, n_segs, p, adv, vtarg, scratch, st, *launches);
}

size_t ppo_head_scratch_floats(int max_batch, int k) { return (size_t)head_waves(pad32(max_batch)) * part_stride(k, true); }

int ppo_head_check(const pvae_fc_ppo_batch* b, const pvae_fc_ppo_params* p, int rows) { return check_loss_args(b, p, rows); }

int ppo_head_launch(const pvae_fc_ppo_batch* b, const pvae_fc_ppo_params* p, const int32_t* index, long long row0, int rows,
                    const PpoHeadIo& io, hipStream_t st) {
    const int rows_pad = pad32(rows);
    PpoHead h;
    fill_head(h, b, p, index, row0, rows, rows_pad);
    h.mean = io.mean; h.ld_mean = io.ld_mean; h.ls = io.ls; h.ld_ls = 0; h.value = io.value; h.ld_value = io.ld_value;
    h.d_mean = io.d_mean; h.ld_dm = io.ld_dm; h.width_dm = io.width_dm;
    h.d_value = io.d_value; h.ld_dv = io.ld_dv; h.width_dv = io.width_dv;
    h.part = io.part; h.part_stride = part_stride(b->k, io.colsum != 0); h.colsum = io.colsum;
    hipLaunchKernelGGL(fc_ppo_head_kernel, dim3(head_waves(rows_pad) / 4), dim3(256), 0, st, h);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ppo_adam_launch(const PpoAdamSegs& segs, const pvae_fc_ppo_params* p, int adam_t, int rows, int k, const float* part,
                    int colsum, float* ls, float* ls_m, float* ls_v, float* stats_out, hipStream_t st) {
    PpoAdam a;
    memset((void*)&a, 0, sizeof(a));
    a.seg = segs;
    long long total4 = 0;
    for (int i = 0; i < segs.n; ++i) { total4 += segs.n4[i]; a.end4[i] = total4; }
    a.s = ppo_adam_scalars(p, adam_t);
    a.part = part; a.nparts = head_waves(pad32(rows)); a.part_stride = part_stride(k, colsum != 0);
    a.inv_rows = (float)(1.0 / rows); a.stats_out = stats_out;
    a.k = k;
    if (colsum) { a.ls = ls; a.ls_m = ls_m; a.ls_v = ls_v; }
    long long grid = (total4 + 255) / 256;
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(ppo_adam_kernel, dim3((int)grid + 1), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" {

int pvae_fc_num_layers(const pvae_fc_config* cfg) {
    if (!cfg) return fail(-1, "null config");
    const FcLayout L = make_fc_layout(*cfg);
    if (!L.ok) return fail(-1, "bad stack-set config: %s", L.why);
    int n = 0;
    for (int s = 0; s < L.S; ++s) n += (int)L.stack[s].size();
    return n;
}

int pvae_fc_layer(const pvae_fc_config* cfg, int i, pvae_layer_info* out) {
    if (!cfg || !out) return fail(-1, "null argument");
    const FcLayout L = make_fc_layout(*cfg);
    if (!L.ok) return fail(-1, "bad stack-set config: %s", L.why);
    for (int s = 0; s < L.S; ++s) {
        if (i >= 0 && i < (int)L.stack[s].size()) {
            const FcLayer& l = L.stack[s][i];
            out->net = s; out->index = l.index; out->n_in = l.n_in; out->n_out = l.n_out; out->ld = l.ld;
            out->n_out_pad = l.n_out_pad; out->w_offset = l.w_off; out->b_offset = l.b_off;
            out->act = l.act == 0 ? PVAE_ACT_LINEAR : l.act - 1;
            out->col0 = 0;
            return 0;
        }
        i -= (int)L.stack[s].size();
    }
    return fail(-1, "layer index out of range");
}

int64_t pvae_fc_arena_floats(const pvae_fc_config* cfg) {
    if (!cfg) return fail(-1, "null config");
    const FcLayout L = make_fc_layout(*cfg);
    if (!L.ok) return fail(-1, "bad stack-set config: %s", L.why);
    return L.arena_floats;
}

size_t pvae_fc_workspace_bytes(const pvae_fc_config* cfg) {
    if (!cfg) return 0;
    const FcLayout L = make_fc_layout(*cfg);
    if (!L.ok) { fail(-1, "bad stack-set config: %s", L.why); return 0; }
    return (size_t)make_fc_work(L).total_floats * sizeof(float);
}

int pvae_fc_create(const pvae_fc_config* cfg, pvae_fc** out) {
    if (!cfg || !out) return fail(-1, "null argument");
    FcLayout L = make_fc_layout(*cfg);
    if (!L.ok) return fail(-1, "bad stack-set config: %s", L.why);
    pvae_fc* c = new (std::nothrow) pvae_fc();
    if (!c) return fail(-3, "out of host memory");
    c->W = make_fc_work(L);
    c->L = std::move(L);
    *out = c;
    return 0;
}

void pvae_fc_destroy(pvae_fc* fc) { delete fc; }

int pvae_fc_bind(pvae_fc* c, float* params, void* workspace, size_t workspace_bytes) {
    if (!c || !params || !workspace) return fail(-1, "null argument");
    if (workspace_bytes < (size_t)c->W.total_floats * sizeof(float))
        return fail(-1, "workspace too small: %zu < %zu bytes", workspace_bytes, (size_t)c->W.total_floats * sizeof(float));
    if (((uintptr_t)params | (uintptr_t)workspace) & 15) return fail(-1, "arena and workspace must be 16-byte aligned");
    c->params = params;
    c->ws = (float*)workspace;
    return 0;
}

int pvae_fc_forward(pvae_fc* c, const float* x, int32_t rows, float* const* out, void* stream) {
    int rc = check_call(c, x, rows);
    if (rc) return rc;
    if (!out) return fail(-1, "out is null");
    Run r{c, (hipStream_t)stream, rows, pad32(rows)};
    for (int s = 0; s < c->L.S; ++s) r.want[s] = out[s] != nullptr;
    set_range(r, c->L.S);
    if (r.s_lo < 0) return fail(-1, "no output wanted: nothing to compute");
    if ((rc = copy_in(r, x))) return rc;
    if ((rc = run_forward(r, out))) return rc;
    c->fwd_launches = r.launches;
    return 0;
}

int pvae_fc_backward(pvae_fc* c, const float* x, int32_t rows, const float* const* dy, float* dx, float* grad,
                     int32_t grad_mask, int32_t accumulate, void* stream) {
    int rc = check_call(c, x, rows);
    if (rc) return rc;
    if (!dy) return fail(-1, "dy is null");
    if (!dx && !grad) return fail(-1, "neither dx nor grad: nothing to compute");
    if (grad && ((uintptr_t)grad & 15)) return fail(-1, "grad must be 16-byte aligned");
    const FcLayout& L = c->L;
    Run r{c, (hipStream_t)stream, rows, pad32(rows)};
    // a stack runs when it has an output gradient and somebody consumes what it yields: dx, or its own parameter gradient
    for (int s = 0; s < L.S; ++s) r.want[s] = dy[s] != nullptr && (dx != nullptr || (grad && ((grad_mask >> s) & 1)));
    set_range(r, L.S);
    if (r.s_lo < 0) return fail(-1, "no stack with an output gradient and a consumer: nothing to compute");
    if ((rc = copy_in(r, x))) return rc;
    if ((rc = zero_pad_rows(r))) return rc;
    if ((rc = run_forward(r, nullptr))) return rc;
    {
        FcSeed a;
        memset(&a, 0, sizeof(a));
        int n = 0, wmax = 0;
        for (int s = r.s_lo; s <= r.s_hi; ++s) {
            // (a stack without a gradient inside the first-layer range: zeros in its columns of the shared gradient panel)
            if (!r.want[s] && !dx) continue;
            const int i = r.want[s] ? (int)L.stack[s].size() - 1 : 0;
            const FcLayer& l = L.stack[s][i];
            a.dy[n] = r.want[s] ? dy[s] : nullptr;
            a.dz[n] = dz_ptr(c, s, i); a.n[n] = l.n_out; a.width[n] = l.n_out_pad; a.ld[n] = panel_ld(c, s, i);
            if (l.n_out_pad > wmax) wmax = l.n_out_pad;
            ++n;
        }
        a.rows = rows; a.rows_pad = r.rows_pad;
        int gx = (r.rows_pad * wmax + 255) / 256;
        if (gx > 256) gx = 256;
        hipLaunchKernelGGL(fc_seed_kernel, dim3(gx, n), dim3(256), 0, r.st, a);
        HIP_TRY(hipGetLastError());
        ++r.launches;
    }
    rc = accumulate ? run_backward_layers<EpiGradAccum>(r, dx != nullptr, grad, grad_mask)
                    : run_backward_layers<EpiGradStore>(r, dx != nullptr, grad, grad_mask);
    if (rc) return rc;
    if (dx) {
        int grid = (rows * L.cfg.n_in + 255) / 256;
        if (grid > 1024) grid = 1024;
        hipLaunchKernelGGL(fc_copy_out_kernel, dim3(grid), dim3(256), 0, r.st, c->ws + c->W.d_in, L.ld0, dx, L.cfg.n_in, rows);
        HIP_TRY(hipGetLastError());
        ++r.launches;
    }
    c->bwd_launches = r.launches;
    return 0;
}

int pvae_fc_launches(pvae_fc* c, int32_t* forward, int32_t* backward) {
    if (!c) return fail(-1, "null stack set");
    if (forward) *forward = c->fwd_launches;
    if (backward) *backward = c->bwd_launches;
    return 0;
}

size_t pvae_fc_ppo_workspace_bytes(const pvae_fc_config* cfg) {
    if (!cfg) return 0;
    const FcLayout L = make_fc_layout(*cfg);
    if (!L.ok) { fail(-1, "bad stack-set config: %s", L.why); return 0; }
    return (ppo_scratch_floats(L) * sizeof(float) + 15) / 16 * 16;
}

int pvae_fc_ppo_sizeof(int which) {
    return which == 0 ? (int)sizeof(pvae_fc_ppo_params) : which == 1 ? (int)sizeof(pvae_fc_ppo_batch) : fail(-1, "which must be 0 or 1");
}

int pvae_fc_ppo_bind(pvae_fc* c, float* grad, float* m, float* v, void* scratch, size_t scratch_bytes, float* log_std,
                     float* log_std_m, float* log_std_v) {
    if (!c || !grad || !m || !v || !scratch) return fail(-1, "null argument");
    if (!c->params || !c->ws) return fail(-2, "pvae_fc_bind has not been called");
    const size_t need = (ppo_scratch_floats(c->L) * sizeof(float) + 15) / 16 * 16;
    if (scratch_bytes < need) return fail(-1, "scratch too small: %zu < %zu bytes", scratch_bytes, need);
    if (((uintptr_t)grad | (uintptr_t)m | (uintptr_t)v | (uintptr_t)scratch) & 15)
        return fail(-1, "grad, m, v and scratch must be 16-byte aligned");
    if ((log_std_m != nullptr) != (log_std_v != nullptr) || (log_std_m && !log_std))
        return fail(-1, "log_std_m and log_std_v go together, with log_std");
    c->grad = grad; c->m = m; c->v = v; c->scratch = (float*)scratch;
    c->log_std = log_std; c->log_std_m = log_std_m; c->log_std_v = log_std_v;
    return 0;
}

int pvae_ppo_loss(const float* mean, const float* log_std, int64_t log_std_row_stride, const float* value,
                  const pvae_fc_ppo_batch* b, const int32_t* index, int32_t rows, const pvae_fc_ppo_params* p,
                  float* d_mean, float* d_log_std, float* d_value, float* stats_out, void* stream) {
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
    hipLaunchKernelGGL(fc_ppo_head_kernel, dim3(waves / 4), dim3(256), 0, st, h);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ppo_finish_kernel, dim3(1), dim3(64), 0, st, part, waves, kPartStats, h.inv_rows, stats_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int pvae_fc_ppo_step(pvae_fc* c, const pvae_fc_ppo_batch* b, const int32_t* index, int64_t first, int32_t rows,
                     const pvae_fc_ppo_params* p, float* stats_out, void* stream) {
    int rc = check_ppo(c, b, p, first, rows, stats_out);
    if (rc) return rc;
    return ppo_step(c, b, index, first, rows, p, p->adam_t, stats_out, (hipStream_t)stream);
}

int pvae_fc_ppo_sgd(pvae_fc* c, const pvae_fc_ppo_batch* b, const int32_t* perm, int32_t minibatch, int32_t num_sgd_iter,
                    const pvae_fc_ppo_params* p, float* stats_out, void* stream) {
    if (minibatch < 1 || num_sgd_iter < 1) return fail(-1, "minibatch and num_sgd_iter must be positive");
    int rc = check_ppo(c, b, p, 0, 1, stats_out);
    if (rc) return rc;
    if (minibatch > c->L.cfg.max_batch) return fail(-1, "minibatch %d > max_batch %d", minibatch, c->L.cfg.max_batch);
    int step = 0;
    for (int pass = 0; pass < num_sgd_iter; ++pass)
        for (long long first = 0; first < b->n_rows; first += minibatch, ++step) {
            const int rows = (int)(b->n_rows - first < minibatch ? b->n_rows - first : minibatch);
            rc = ppo_step(c, b, perm ? perm + (size_t)pass * b->n_rows : nullptr, first, rows, p, p->adam_t + step,
                          stats_out + 5 * (size_t)step, (hipStream_t)stream);
            if (rc) return rc;
        }
    return 0;
}

int pvae_fc_ppo_launches(pvae_fc* c, int32_t* per_step) {
    if (!c || !per_step) return fail(-1, "null argument");
    *per_step = c->ppo_launches;
    return 0;
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

int pvae_fc_ppo_evaluate(pvae_fc* c, const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out,
                         void* stream) {
    const bool rows_pass = out && out->vf_preds, boot = out && out->last_value;
    int rc = check_eval(c, ro, p, out, rows_pass);
    if (rc) return rc;
    if (!rows_pass && !boot) return fail(-1, "neither vf_preds nor last_value: nothing to compute");
    if (boot && (rc = check_boot(ro, out))) return rc;
    int ev = 0, rest = 0;
    if (rows_pass && (rc = eval_rows(c, ro, p, out, (hipStream_t)stream, ev))) return rc;
    if (boot && (rc = eval_boot(c, ro, out, (hipStream_t)stream, rest))) return rc;
    c->eval_launches = ev; c->gae_launches = rest;
    return 0;
}

int pvae_fc_ppo_prepare(pvae_fc* c, const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out,
                        void* scratch, size_t scratch_bytes, void* stream) {
    int rc = check_gae_params(p);
    if (rc) return rc;
    if (!ro || !out) return fail(-1, "null rollout or outputs");
    const int given = (ro->vf_preds != nullptr) + (ro->old_dist != nullptr) + (ro->old_logp != nullptr);
    if (given != 0 && given != 3) return fail(-1, "the sampler's vf_preds, old_dist and old_logp go together: all three or none");
    if ((rc = check_eval(c, ro, p, out, given == 0))) return rc;
    if ((rc = check_boot(ro, out))) return rc;
    if (!ro->rewards || !ro->seg_start) return fail(-1, "rollout rewards or seg_start is null");
    if (!out->advantages || !out->value_targets) return fail(-1, "advantages or value_targets is null");
    if ((rc = check_segments(ro->n_rows, ro->n_segs, ro->seg_first, ro->seg_last))) return rc;
    if ((rc = check_gae_scratch(scratch, scratch_bytes, ro->n_segs))) return rc;
    hipStream_t st = (hipStream_t)stream;
    int ev = 0, rest = 0;
    if (given == 0 && (rc = eval_rows(c, ro, p, out, st, ev))) return rc;
    if ((rc = eval_boot(c, ro, out, st, rest))) return rc;
    // (last_value already holds the zeros of the done segments)
    if ((rc = run_gae(ro->rewards, given ? ro->vf_preds : out->vf_preds, out->last_value, nullptr, ro->seg_start, ro->n_rows,
                      ro->n_segs, p, out->advantages, out->value_targets, scratch, st, rest)))
        return rc;
    c->eval_launches = ev; c->gae_launches = rest;
    return 0;
}

int pvae_fc_gae_launches(pvae_fc* c, int32_t* evaluate, int32_t* rest) {
    if (!c) return fail(-1, "null stack set");
    if (evaluate) *evaluate = c->eval_launches;
    if (rest) *rest = c->gae_launches;
    return 0;
}

}  // extern "C"
