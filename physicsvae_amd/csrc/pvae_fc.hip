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
// Below the stack set itself: its PPO learner (pvae_fc_ppo_*) -- FcLearner, the model adapter the host driver of
// pvae_ppo_learner.h runs: the set's checks, and the forward and backward launches above around the loss head of
// pvae_ppo_core.hip -- and the value stack alone as PhysicsVAE's learner (pvae_ppo.hip) runs it.
#include "pvae_internal.h"
#include "pvae_fc_layout.h"
#include "pvae_ppo_learner.h"

struct pvae_fc {
    FcLayout L;
    FcWork W;
    float* params = nullptr;
    float* ws = nullptr;
    int fwd_launches = 0, bwd_launches = 0;
    PpoLearner ppo;                               // PPO learner (pvae_fc_ppo_bind)
};

namespace {

constexpr int kS = PVAE_FC_MAX_STACKS;

// ---------------------------------------------------------------------------------------
// glue kernels (the padded copy-in is pad_copy_launch, pvae_ppo_core.hip)
// ---------------------------------------------------------------------------------------
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

// forward, rows <= 4: the arithmetic of gemv_rows_kernel (pvae_net.hip) -- one wave per output feature streams its weight row
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

// forward problem out[M][N] = act(X W^T + b) on 16x16 or 32x32 tiles (tile16: the group kernel's switch between them)
constexpr TileRule kFwdRule{false, false, TileRule::kForward, true};
FwdProb fwd_prob(const float* X, int ldx, const float* W, int ldw, int M, int N, int K, TileGeom geom, const EpiFc& e) {
    const TilePlan t = plan_tiles(geom, kFwdRule, X, ldx, W, ldw, M, N, K);
    FwdProb p{t.ga, e, t.grid};
    p.ga.tile16 = geom == kTile16;
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

int copy_in(Run& r, const float* x, const int32_t* index = nullptr, long long n_rows = 0, const uint8_t* done = nullptr) {
    const pvae_fc* c = r.c;
    const int rc = pad_copy_launch(x, c->L.cfg.n_in, r.rows, c->ws + c->W.in, c->L.ld0, r.rows_pad, index, n_rows, done, r.st);
    if (rc) return rc;
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
    const TileGeom geom0 = tile_geometry(kFwdRule, r.rows_pad, L.n0);
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
            tp.push_back(fwd_prob(in, L.ld0, c->params + a.w_off, L.ld0, r.rows_pad, N, L.ld0, geom0, e));
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
                    const TileGeom geom = i == 0 ? geom0 : tile_geometry(kFwdRule, r.rows_pad, l.n_out_pad);
                    tp.push_back(fwd_prob(x, ldx, c->params + l.w_off, l.ld, r.rows_pad, l.n_out_pad, l.ld, geom, e));
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
    const TilePlan d = plan_dgrad(dZ, ldz, W, ldw, M, Kin, N, true);
    return DProb{d.ga, e, d.grid};
}
template <class EpiW>
WProb<EpiW> w_prob(const float* dZ, int ldz, const float* X, int ldx, int N, int Kin, int M, float* g, float* gb) {
    const WgradPlan w = plan_wgrad(dZ, ldz, X, ldx, N, Kin, M, true);
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
    if (!(r.rows <= 4 && r.rows < r.rows_pad)) return 0;
    ZeroRows z;
    memset(&z, 0, sizeof(z));
    z.add(c->ws + c->W.act0, L.n0, L.n0);
    for (int s = 0; s < L.S; ++s)
        for (int i = 1; r.want[s] && i < (int)L.stack[s].size(); ++i)
            z.add(act_ptr(c, s, i), L.stack[s][i].n_out_pad, L.stack[s][i].n_out_pad);
    z.r0 = r.rows; z.r1 = r.rows_pad;
    const int rc = zero_rows_launch(z, r.st);
    if (rc) return rc;
    ++r.launches;
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

// ---- the PPO learner and its train-batch preparation: the stack set as the driver (pvae_ppo_learner.h) sees it ----
struct FcLearner {
    pvae_fc* c;
    PpoLearner* learner() const { return c ? &c->ppo : nullptr; }
    int k() const { return c->L.cfg.n_out[0]; }
    int n_in() const { return c->L.cfg.n_in; }
    int max_minibatch() const { return c->L.cfg.max_batch; }
    long long peer_timeout() const { return g_ppo_peer_timeout_ticks; }
    void params_written(hipStream_t) const {}
    float* eps_out() const { return nullptr; }

    // the checks of a step in their order; check_bound and check_update are the parts the second half shares
    int check_bound() const {
        if (!c) return fail(-1, "null stack set");
        if (!c->params || !c->ws) return fail(-2, "pvae_fc_bind has not been called");
        const PpoLearner& q = c->ppo;
        if (!q.grad || !q.m || !q.v || !q.scratch) return fail(-2, "pvae_fc_ppo_bind has not been called");
        return 0;
    }
    int check_update(const pvae_fc_ppo_params* p) const {
        if (p->adam_t < 1) return fail(-1, "adam_t must be >= 1");
        if (p->train_mask < 0 || p->train_mask >= (1 << c->L.S)) return fail(-1, "train_mask names a stack that does not exist");
        return 0;
    }
    int check_step(const pvae_fc_ppo_batch* b, const pvae_fc_ppo_params* p, long long first, int rows, const float* stats) const {
        int rc = check_bound();
        if (rc) return rc;
        if ((rc = check_loss_args(b, p, rows))) return rc;
        if (!b->obs) return fail(-1, "batch obs is null");
        if (!stats) return fail(-1, "stats_out is null");
        const FcLayout& L = c->L;
        const PpoLearner& q = c->ppo;
        if (L.S < 2 || L.S > 3) return fail(-1, "a PPO step needs [policy, value] or [policy, value, log-std] stacks, got %d", L.S);
        if (L.cfg.n_out[1] != 1) return fail(-1, "stacks in the wrong order: stack 1 must be the value function (n_out 1, got %d)", L.cfg.n_out[1]);
        if (L.S == 3 && L.cfg.n_out[2] != L.cfg.n_out[0])
            return fail(-1, "stacks in the wrong order: the log-std stack (2) must be as wide as the policy stack (0)");
        if ((p->log_std_kind == 2) != (L.S == 3)) return fail(-1, "log_std_kind %d does not fit %d stacks", p->log_std_kind, L.S);
        if (b->k != L.cfg.n_out[0]) return fail(-1, "batch k %d != policy outputs %d", b->k, L.cfg.n_out[0]);
        if (p->log_std_kind != 2 && !q.log_std) return fail(-2, "log_std vector not bound (pvae_fc_ppo_bind)");
        if (p->log_std_kind == 1 && (!q.log_std_m || !q.log_std_v)) return fail(-2, "log_std moments not bound (pvae_fc_ppo_bind)");
        if (rows > L.cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, L.cfg.max_batch);
        if (first < 0 || first + rows > b->n_rows) return fail(-1, "rows [%lld, +%d) outside the batch of %lld", first, rows, (long long)b->n_rows);
        return check_update(p);
    }
    int check_apply(const pvae_fc_ppo_params* p, const float* ls_grad) const {
        if (!c) return fail(-1, "null stack set");
        if (!p) return fail(-1, "null params");
        int rc = check_bound();
        if (rc) return rc;
        if (p->log_std_kind < 0 || p->log_std_kind > 2) return fail(-1, "log_std_kind %d outside [0, 2]", p->log_std_kind);
        if ((p->log_std_kind == 2) != (c->L.S == 3)) return fail(-1, "log_std_kind %d does not fit %d stacks", p->log_std_kind, c->L.S);
        if ((rc = check_update(p))) return rc;
        const PpoLearner& q = c->ppo;
        if (p->log_std_kind == 1 && (!q.log_std || !q.log_std_m || !q.log_std_v)) return fail(-2, "log_std vector or its moments not bound (pvae_fc_ppo_bind)");
        if (p->log_std_kind == 1 && !ls_grad) return fail(-1, "ls_grad is null (log_std_kind 1)");
        return 0;
    }

    int check_eval(const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out, bool rows_pass) const;

    int grad_half(const pvae_fc_ppo_batch* b, const int32_t* index, long long first, int rows, const pvae_fc_ppo_params* p,
                  int step, int minibatch, float* dpart, hipStream_t st, int* launches) const;
    int segments(const pvae_fc_ppo_params* p, PpoAdamSegs& sg) const;
    template <class Epi>
    int eval_rows(const float* obs, long long n_rows, int k, const pvae_gae_params* p, hipStream_t st, int& launches, Epi&& epi) const;
    int eval_boot(const pvae_fc_rollout* ro, const pvae_fc_prepared* out, hipStream_t st, int& launches) const {
        return fc_eval_boot(c, 1, c->L.cfg.max_batch, ro, out, st, launches);
    }
    int peer_arenas(const void* arg, float** arenas, long long* floats) const {
        if (!c || !arg) return fail(-1, "null argument");
        if (!c->ppo.grad) return fail(-2, "pvae_fc_ppo_bind has not been called");
        arenas[0] = c->ppo.grad; floats[0] = c->L.arena_floats;
        return 1;
    }
};

// The first half of a minibatch's step, everything before the Adam launch: forward, loss head, backward into the bound
// gradient arena (arguments checked by the caller); `launches` counts what went out; `dpart`: the head's diagnostics partial rows
int FcLearner::grad_half(const pvae_fc_ppo_batch* b, const int32_t* index, long long first, int rows, const pvae_fc_ppo_params* p,
                         int, int, float* dpart, hipStream_t st, int* launches) const {
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
            h.ls = c->ppo.log_std; h.ld_ls = 0;
        }
        if (mask & 1) { h.d_mean = dz_ptr(c, 0, lp); h.ld_dm = panel_ld(c, 0, lp); h.width_dm = L.stack[0][lp].n_out_pad; }
        if (mask & 2) { h.d_value = dz_ptr(c, 1, lv); h.ld_dv = panel_ld(c, 1, lv); h.width_dv = L.stack[1][lv].n_out_pad; }
        h.part = c->ppo.scratch; h.part_stride = part_stride(b->k, colsum); h.colsum = colsum;
        h.dpart = dpart;
        if ((rc = ppo_head_launch(h, st))) return rc;
        ++r.launches;
    }
    for (int s = 0; s < L.S; ++s) r.want[s] = (mask >> s) & 1;
    if ((rc = run_backward_layers<EpiGradStore>(r, false, c->ppo.grad, mask))) return rc;
    *launches = r.launches;
    return 0;
}

// the trained stacks' parts of the arena, in arena order, adjacent ones merged: what the Adam launch runs over
int FcLearner::segments(const pvae_fc_ppo_params* p, PpoAdamSegs& sg) const {
    const FcLayout& L = c->L;
    const PpoLearner& q = c->ppo;
    const int mask = p->train_mask ? p->train_mask : (1 << L.S) - 1;
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
    memset((void*)&sg, 0, sizeof(sg));
    for (const auto& e : seg) {
        if (sg.n == kAdamSegs) return fail(-3, "the trained parts of the arena form more than %d segments", kAdamSegs);
        sg.p[sg.n] = c->params + e.first; sg.g[sg.n] = q.grad + e.first; sg.m[sg.n] = q.m + e.first; sg.v[sg.n] = q.v + e.first;
        sg.n4[sg.n++] = e.second / 4;
    }
    return 0;
}

// what evaluate and prepare ask of the stack set; `rows_pass`: the policy's distribution is evaluated (its log-std is needed)
int FcLearner::check_eval(const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out, bool rows_pass) const {
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
        if (p->log_std_kind != 2 && !c->ppo.log_std) return fail(-2, "log_std vector not bound (pvae_fc_ppo_bind)");
        if (!ro->obs || !ro->actions) return fail(-1, "rollout obs or actions is null");
        if (!out->vf_preds || !out->old_dist || !out->old_logp) return fail(-1, "an evaluate output (vf_preds, old_dist, old_logp) is null");
    }
    return 0;
}

// rows [n_rows][n_in] of `obs` through all stacks in chunks of max_batch: copy-in, one launch per depth, then the chunk's
// epilogue -- epi(panels, first row, chunk index) launches it (the evaluate one, or the sampling one of pvae_fc_ppo_act)
template <class Epi>
int FcLearner::eval_rows(const float* obs, long long n_rows, int k, const pvae_gae_params* p, hipStream_t st, int& launches,
                         Epi&& epi) const {
    const FcLayout& L = c->L;
    uint64_t i = 0;
    for (long long first = 0; first < n_rows; first += L.cfg.max_batch, ++i) {
        const int rows = (int)(n_rows - first < L.cfg.max_batch ? n_rows - first : L.cfg.max_batch);
        Run r{c, st, rows, pad32(rows)};
        for (int s = 0; s < L.S; ++s) r.want[s] = true;
        set_range(r, L.S);
        int rc;
        if ((rc = copy_in(r, obs + (size_t)first * L.cfg.n_in))) return rc;
        if ((rc = run_forward(r, nullptr))) return rc;
        PpoPanels e;
        memset(&e, 0, sizeof(e));
        const int lp = (int)L.stack[0].size() - 1, lv = (int)L.stack[1].size() - 1;
        e.mean = act_ptr(c, 0, lp); e.ld_mean = panel_ld(c, 0, lp);
        e.value = act_ptr(c, 1, lv); e.ld_value = panel_ld(c, 1, lv);
        if (p->log_std_kind == 2) {
            const int ll = (int)L.stack[2].size() - 1;
            e.ls = act_ptr(c, 2, ll); e.ld_ls = panel_ld(c, 2, ll); e.ls_base = p->log_std_base;
        } else {
            e.ls = c->ppo.log_std; e.ld_ls = 0;
        }
        e.rows = rows; e.k = k;
        if ((rc = epi(e, first, i))) return rc;
        launches += r.launches + 1;
    }
    return 0;
}
// one stack alone, as PhysicsVAE's learner and the bootstrap pass run the value function
Run value_run(pvae_fc* c, int s, int rows, hipStream_t st) {
    Run r{c, st, rows, pad32(rows)};
    r.want[s] = true;
    set_range(r, c->L.S);
    return r;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// the value stack alone: what PhysicsVAE's learner (pvae_ppo.hip) and the bootstrap pass run of this unit (pvae_internal.h)
// ---------------------------------------------------------------------------------------
int fc_value_stack(pvae_fc* c, FcValueStack* out) {
    if (!c) return fail(-1, "null value stack set");
    if (!c->params || !c->ws) return fail(-2, "value stack set: pvae_fc_bind has not been called");
    if (!c->ppo.grad || !c->ppo.m || !c->ppo.v) return fail(-2, "value stack set: pvae_fc_ppo_bind has not been called");
    const FcLayout& L = c->L;
    if (L.S != 1 || L.cfg.n_out[0] != 1) return fail(-1, "the value stack set must be one stack with one output, got %d stacks", L.S);
    const int lv = (int)L.stack[0].size() - 1;
    memset(out, 0, sizeof(*out));
    out->in = c->ws + c->W.in; out->ld_in = L.ld0; out->n_in = L.cfg.n_in;
    out->value = act_ptr(c, 0, lv); out->ld_value = panel_ld(c, 0, lv);
    out->d_value = dz_ptr(c, 0, lv); out->ld_dv = panel_ld(c, 0, lv); out->width_dv = L.stack[0][lv].n_out_pad;
    out->params = c->params; out->grad = c->ppo.grad; out->m = c->ppo.m; out->v = c->ppo.v;
    out->arena_floats = L.arena_floats;
    out->max_batch = L.cfg.max_batch;
    for (int i = 0; i <= lv; ++i) {
        out->panel[i] = act_ptr(c, 0, i);
        out->panel_ld[i] = panel_ld(c, 0, i);
    }
    out->n_panels = lv + 1;
    return 0;
}

int fc_value_forward(pvae_fc* c, int s, int rows, hipStream_t st, int* launches) {
    Run r = value_run(c, s, rows, st);
    const int rc = run_forward(r, nullptr);
    *launches += r.launches;
    return rc;
}

int fc_value_backward(pvae_fc* c, int s, int rows, hipStream_t st, int* launches) {
    Run r = value_run(c, s, rows, st);
    const int rc = run_backward_layers<EpiGradStore>(r, false, c->ppo.grad, 1 << s);
    *launches += r.launches;
    return rc;
}

int fc_eval_boot(pvae_fc* c, int s, int chunk, const pvae_fc_rollout* ro, const pvae_fc_prepared* out, hipStream_t st,
                 int& launches) {
    const int n_in = c->L.cfg.n_in, lv = (int)c->L.stack[s].size() - 1;
    for (int first = 0; first < ro->n_segs; first += chunk) {
        const int rows = ro->n_segs - first < chunk ? ro->n_segs - first : chunk;
        Run r = value_run(c, s, rows, st);
        int rc;
        if ((rc = copy_in(r, ro->boot_obs + (size_t)first * n_in, nullptr, 0, ro->seg_done + first))) return rc;
        if ((rc = run_forward(r, nullptr))) return rc;
        PpoEval e;
        memset(&e, 0, sizeof(e));
        e.value = act_ptr(c, s, lv); e.ld_value = panel_ld(c, s, lv);
        e.done = ro->seg_done + first;
        e.rows = rows; e.k = ro->k;
        e.vf = out->last_value + first;
        if ((rc = ppo_eval_launch(e, st))) return rc;
        launches += r.launches + 1;
    }
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

void pvae_fc_destroy(pvae_fc* fc) {
    if (fc) ppo_peer_free(fc->ppo.peers);
    delete fc;
}

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
    return ppo_scratch_bytes(L.cfg.max_batch, L.cfg.n_out[0]);
}

int pvae_fc_ppo_sizeof(int which) {
    return which == 0 ? (int)sizeof(pvae_fc_ppo_params) : which == 1 ? (int)sizeof(pvae_fc_ppo_batch) : fail(-1, "which must be 0 or 1");
}

int pvae_fc_ppo_bind(pvae_fc* c, float* grad, float* m, float* v, void* scratch, size_t scratch_bytes, float* log_std,
                     float* log_std_m, float* log_std_v) {
    if (!c || !grad || !m || !v || !scratch) return fail(-1, "null argument");
    if (!c->params || !c->ws) return fail(-2, "pvae_fc_bind has not been called");
    const size_t need = ppo_scratch_bytes(c->L.cfg.max_batch, c->L.cfg.n_out[0]);
    if (scratch_bytes < need) return fail(-1, "scratch too small: %zu < %zu bytes", scratch_bytes, need);
    const int rc = check_ppo_buffers(grad, m, v, scratch, log_std, log_std_m, log_std_v);
    if (rc) return rc;
    PpoLearner& q = c->ppo;
    q.grad = grad; q.m = m; q.v = v; q.scratch = (float*)scratch;
    q.log_std = log_std; q.log_std_m = log_std_m; q.log_std_v = log_std_v;
    return 0;
}


int pvae_fc_ppo_step(pvae_fc* c, const pvae_fc_ppo_batch* b, const int32_t* index, int64_t first, int32_t rows,
                     const pvae_fc_ppo_params* p, float* stats_out, void* stream) {
    return learner_step(FcLearner{c}, b, index, first, rows, p, stats_out, (hipStream_t)stream);
}

int pvae_fc_ppo_sgd(pvae_fc* c, const pvae_fc_ppo_batch* b, const int32_t* perm, int32_t minibatch, int32_t num_sgd_iter,
                    const pvae_fc_ppo_params* p, float* stats_out, void* stream) {
    return learner_sgd(FcLearner{c}, b, perm, minibatch, num_sgd_iter, p, stats_out, (hipStream_t)stream);
}

size_t pvae_fc_ppo_diag_bytes(const pvae_fc_config* cfg, int32_t steps) {
    if (!cfg) return 0;
    if (steps < 1) { fail(-1, "steps must be >= 1, got %d", steps); return 0; }
    const FcLayout L = make_fc_layout(*cfg);
    if (!L.ok) { fail(-1, "bad stack-set config: %s", L.why); return 0; }
    return ppo_diag_bytes(L.cfg.max_batch);              // (the norm is finished per step: no per-step slot rows)
}

int pvae_fc_ppo_diag(pvae_fc* c, float* diag, int32_t capacity_steps, void* scratch, size_t scratch_bytes) {
    if (!c) return fail(-1, "null stack set");
    return ppo_diag_bind(c->ppo.diag, diag, capacity_steps, scratch, scratch_bytes, c->L.cfg.max_batch);
}

size_t pvae_fc_ppo_grad_clip_bytes(const pvae_fc_config* cfg) {
    if (!cfg) return 0;
    const FcLayout L = make_fc_layout(*cfg);
    if (!L.ok) { fail(-1, "bad stack-set config: %s", L.why); return 0; }
    return ppo_clip_bytes();                             // (one slot per workgroup of a bounded grid: no size enters)
}

int pvae_fc_ppo_grad_clip(pvae_fc* c, float max_norm, void* scratch, size_t scratch_bytes) {
    if (!c) return fail(-1, "null stack set");
    return ppo_clip_bind(c->ppo.clip, max_norm, scratch, scratch_bytes);
}

int pvae_fc_ppo_grad(pvae_fc* c, const pvae_fc_ppo_batch* b, const int32_t* index, int64_t first, int32_t rows,
                     const pvae_fc_ppo_params* p, float* stats_out, float* ls_grad, void* stream) {
    return learner_grad(FcLearner{c}, b, index, first, rows, p, stats_out, ls_grad, (hipStream_t)stream);
}

int pvae_fc_ppo_apply(pvae_fc* c, const pvae_fc_ppo_params* p, float grad_scale, const float* ls_grad, void* stream) {
    return learner_apply(FcLearner{c}, p, grad_scale, ls_grad, (hipStream_t)stream);
}

int pvae_fc_ppo_peer_export(pvae_fc* c, void* blob) {
    return learner_peer_export(FcLearner{c}, blob);
}

int pvae_fc_ppo_peer_open(pvae_fc* c, int rank, int world, const void* blobs) {
    return learner_peer_open(FcLearner{c}, rank, world, blobs);
}

int pvae_fc_ppo_peer_close(pvae_fc* c) {
    if (!c) return fail(-1, "null stack set");
    return ppo_peer_close(c->ppo.peers);
}

int pvae_fc_ppo_peer_status(pvae_fc* c, int* rank, int* world, uint32_t* timeouts, void* stream) {
    if (!c) return fail(-1, "null stack set");
    return ppo_peer_status(c->ppo.peers, rank, world, timeouts, (hipStream_t)stream);
}

int pvae_fc_ppo_launches(pvae_fc* c, int32_t* per_step) {
    return learner_launches(c ? &c->ppo : nullptr, per_step);
}

int pvae_fc_ppo_evaluate(pvae_fc* c, const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out,
                         void* stream) {
    return learner_evaluate(FcLearner{c}, ro, p, out, (hipStream_t)stream);
}

int pvae_fc_ppo_prepare(pvae_fc* c, const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out,
                        void* scratch, size_t scratch_bytes, void* stream) {
    return learner_prepare(FcLearner{c}, ro, p, out, scratch, scratch_bytes, (hipStream_t)stream);
}

int pvae_fc_ppo_act(pvae_fc* c, const pvae_ppo_act_in* in, const pvae_gae_params* p, const pvae_ppo_act_out* out, void* stream) {
    if (!c) return fail(-1, "null stack set");
    return learner_act(FcLearner{c}, in, p, out, (hipStream_t)stream);
}

int pvae_ppo_act_sizeof(int which) {
    return which == 0 ? (int)sizeof(pvae_ppo_act_in) : which == 1 ? (int)sizeof(pvae_ppo_act_out)
                                                                  : fail(-1, "which must be 0 or 1");
}

int pvae_fc_gae_launches(pvae_fc* c, int32_t* evaluate, int32_t* rest) {
    if (!c) return fail(-1, "null stack set");
    return learner_gae_launches(c->ppo, evaluate, rest);
}

}  // extern "C"
