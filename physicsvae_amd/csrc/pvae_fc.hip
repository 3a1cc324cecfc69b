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

struct pvae_fc {
    FcLayout L;
    FcWork W;
    float* params = nullptr;
    float* ws = nullptr;
    int fwd_launches = 0, bwd_launches = 0;
};

namespace {

constexpr int kS = PVAE_FC_MAX_STACKS;

// ---------------------------------------------------------------------------------------
// glue kernels
// ---------------------------------------------------------------------------------------
// dst[rows_pad][ld] = zero-padded copy of dense src[rows][n]
__global__ void __launch_bounds__(256)
fc_pad_copy_kernel(const float* __restrict__ src, int n, int rows, float* __restrict__ dst, int ld, int rows_pad) {
    const int total = rows_pad * ld;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / ld, c = idx - r * ld;
        dst[idx] = (r < rows && c < n) ? src[(size_t)r * n + c] : 0.f;
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

int copy_in(Run& r, const float* x) {
    const pvae_fc* c = r.c;
    int grid = (r.rows_pad * c->L.ld0 + 255) / 256;
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(fc_pad_copy_kernel, dim3(grid), dim3(256), 0, r.st, x, c->L.cfg.n_in, r.rows, c->ws + c->W.in,
                       c->L.ld0, r.rows_pad);
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

}  // namespace

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
    if (rows <= 4 && rows < r.rows_pad) {       // GEMV path: the pad rows of the layer outputs are not written
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

}  // extern "C"
