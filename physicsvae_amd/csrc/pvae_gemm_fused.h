// pvae_gemm_fused.h -- kernels that hold several jobs: weight gradient + bias gradient + deferred Adam, two weight gradients,
// input gradient || weight gradient, with staging or cache-warming workgroups behind.
#pragma once
#include "pvae_gemm_common.h"
#include "pvae_stage.h"
#include "pvae_gemm_src.h"
#include "pvae_gemm_reg.h"
#include "pvae_gemm_wgrad.h"
#include "pvae_adam.h"

namespace pvae {
template <class Epi, int ABL = 0>
__global__ void __launch_bounds__(256)
gemm_wgrad_reg_kernel(PVAE_GA_PARAMS(a_), int nw, Epi epi, AdamPair ad) {
    const GemmArgs ga = PVAE_GA_OF(a_);
    __shared__ __attribute__((aligned(16))) float lds[kPairLdsFloats];
    const int b = blockIdx.x, nb = bias_tiles(ga);
    if (b < nw) wgrad_body<Epi, ABL>(lds, b, ga, epi);
    else if (b < nw + nb) bias_grad_body(lds, b - nw, ga, epi);
    else adam_pair_body(ad, b - nw - nb);
}

// Horizontal fusion of two independent backward contractions in ONE launch: blocks [0, nd) run
// the input-gradient tiles of layer l-1, blocks [nd, nd + nw) the weight-gradient(+Adam) tiles of
// layer l.  The dgrad blocks are dispatched first (one per CU), the wgrad blocks land beside
// them (2 waves per SIMD), so one workgroup's load / Adam-traffic phases hide under the other's
// MFMA phases, and a launch boundary disappears.
// The next tiles_q blocks of each problem sum its bias gradient (bias_grad_body); the blocks past
// those (sa.rows_pad of them) stage the NEXT minibatch into the
// alternate input panels (StageArgs / stage_row below): the gather rides in the last launch of the
// step that precedes it instead of being a launch of its own.
// What the step's LAST launch does for the NEXT minibatch of a direct run: nothing is staged, but the rows the next
// step's first layers will gather are cold in HBM (an epoch walks the whole set once), and their first touch would sit on
// the critical path of those launches (+2 us each, measured).  A few workgroups of this launch read one dword per
// 128-byte line of those rows -- up to four contiguous runs: the state rows and the action rows of the (at most two)
// episode segments of the minibatch -- so that the Infinity Cache holds them when the next step starts.
struct TouchRuns {
    const float* p[4];
    int lines[4];                 // 128-byte lines per run (0: none)
    int blocks;                   // workgroups that do the touching
};
__device__ inline void touch_body(const TouchRuns& t, int blk) {
    float sink = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        for (int i = blk * 256 + (int)threadIdx.x; i < t.lines[r]; i += t.blocks * 256)
            asm volatile("global_load_dword %0, %1, off" : "+v"(sink) : "v"(t.p[r] + (size_t)i * 32) : "memory");
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(sink)::"memory");
}
// The step's trailing weight gradient on the gathered first-layer input (no second problem, no staging workgroups).  The
// whole operand descriptor travels in the 14 preloadable leading dwords -- the s0 and s1 runs, their strides and widths,
// the batch's rows as two (base, start) runs -- so that the first tile fetch waits for no s_load (`rest` is only read for
// the index array of a minibatch with more than one episode jump).
template <class EpiW>
__global__ void __launch_bounds__(256, 3)       // (three waves per SIMD, as the staged kernel gets on its own: <= 168 VGPRs)
wgrad_pair_gather_kernel(const float* aQ, const float* g_s0, const float* g_s1, unsigned a_ld, unsigned a_t, unsigned a_k,
                         unsigned g_ld0n0, unsigned g_ld1n1, unsigned g_rq1, int g_b0, int g_b1, int na, EpiW e1, AdamPair ad,
                         TouchRuns touch, XSrc rest) {
    __shared__ __attribute__((aligned(16))) float lds[kPairLdsFloats];
    GemmArgs g1 = ga_unpack(aQ, nullptr, a_ld, a_t, a_k);
    const int gfl = g1.krot;                     // (the rotation bits carry: bit 0 = two-run row map, bit 1 = s1 row-indirect)
    g1.krot = 0;
    PGather ps;
    ps.x = rest;
    ps.x.s0 = g_s0; ps.x.ld0 = (int)(g_ld0n0 & 0xffffu); ps.x.n0 = (int)(g_ld0n0 >> 16);
    ps.x.s1 = g_s1; ps.x.ld1 = (int)(g_ld1n1 & 0xffffu); ps.x.n1 = (int)(g_ld1n1 >> 16);
    ps.x.ind1 = (gfl >> 1) & 1;
    ps.x.rows = (int)(g_rq1 & 0xffffu) + 1;
    ps.x.rm.seg = gfl & 1; ps.x.rm.q1 = (int)(g_rq1 >> 16) + 1; ps.x.rm.b0 = g_b0; ps.x.rm.b1 = g_b1;
    const int n1 = ga_grid(g1), nb1 = bias_tiles(g1);
    const int b = blockIdx.x;
    if (b < n1) wgrad_body<EpiW, 0, PGather>(lds, b, g1, e1, ps);
    else if (b < n1 + nb1) bias_grad_body(lds, b - n1, g1, e1);
    else if (b < n1 + nb1 + na) adam_pair_body(ad, b - n1 - nb1);
    else touch_body(touch, b - n1 - nb1 - na);
}
template <class EpiD, class EpiW, class PS>
__global__ void __launch_bounds__(256, 3)
bwd_pair_gather_kernel(PVAE_GA2_PARAMS, EpiD ed, EpiW ew, AdamPair ad, PS ps) {
    __shared__ __attribute__((aligned(16))) float lds[kPairLdsFloats];
    const GemmArgs gd = PVAE_GA2_A, gw = PVAE_GA2_B;
    const int nd = ga_grid(gd), nw = ga_grid(gw);
    const int b = blockIdx.x;
    if (b < nd) {
        if (gd.tile16) splitk_reg16_body<false, EpiD>(lds, b, gd, ed);
        else splitk_reg_body<false, EpiD, 0>(lds, b, gd, ed);
    } else if (b < nd + nw) wgrad_body<EpiW, 0, PS>(lds, b - nd, gw, ew, ps);
    else if (b < nd + nw + bias_tiles(gw)) bias_grad_body(lds, b - nd - nw, gw, ew);
    else adam_pair_body(ad, b - nd - nw - bias_tiles(gw));
}

template <class EpiW>
__global__ void __launch_bounds__(256)
wgrad_pair_kernel(PVAE_GA2_PARAMS, int na, EpiW e1, EpiW e2, StageArgs sa, AdamPair ad) {
    __shared__ __attribute__((aligned(16))) float lds[kPairLdsFloats];
    const GemmArgs g1 = PVAE_GA2_A, g2 = PVAE_GA2_B;
    const int n1 = ga_grid(g1), n12 = n1 + ga_grid(g2);
    const int b = blockIdx.x;
    const int nb1 = bias_tiles(g1), nb2 = bias_tiles(g2);
    if (b < n1) wgrad_body<EpiW>(lds, b, g1, e1);
    else if (b < n12) wgrad_body<EpiW>(lds, b - n1, g2, e2);
    else if (b < n12 + nb1) bias_grad_body(lds, b - n12, g1, e1);
    else if (b < n12 + nb1 + nb2) bias_grad_body(lds, b - n12 - nb1, g2, e2);
    else if (b < n12 + nb1 + nb2 + na) adam_pair_body(ad, b - n12 - nb1 - nb2);
    else stage_row(sa, b - n12 - nb1 - nb2 - na, 0, sa.rows_pad);
}

// (The dgrad half stays on the register-staged body here: with the wave-specialised body the
// pair needs 512-thread blocks and 64 KB of LDS per workgroup and measured 15 % slower.)
template <class EpiD, class EpiW, int ABL = 0>          // ABL: ablation bits of the two bodies (probes only)
__global__ void __launch_bounds__(256)
bwd_pair_kernel(PVAE_GA2_PARAMS, EpiD ed, EpiW ew, AdamPair ad) {
    __shared__ __attribute__((aligned(16))) float lds[kPairLdsFloats];
    const GemmArgs gd = PVAE_GA2_A, gw = PVAE_GA2_B;
    const int nd = ga_grid(gd), nw = ga_grid(gw);          // (a body with tiles_q = 0 is absent: ablation probes)
    PVAE_MARK(0, 0);
    PVAE_MARK_HW();
    // (dispatch order matters: input-gradient workgroups first.  Weight-gradient workgroups first: world step
    //  90.0 -> 93.5 us; the two kinds interleaved: 91.8 us -- the older waves of a SIMD win issue arbitration,
    //  and it is the input gradient whose reduction + store epilogue can hide under the partner's MFMAs)
    const int b = blockIdx.x;
    if (b < nd) {
        if (gd.tile16) splitk_reg16_body<false, EpiD>(lds, b, gd, ed);
        else splitk_reg_body<false, EpiD, ABL>(lds, b, gd, ed);
    } else if (b < nd + nw) wgrad_body<EpiW, (ABL & 32) ? 0 : ABL>(lds, b - nd, gw, ew);   // (bit 32: the input-gradient body alone)
    else if (b < nd + nw + bias_tiles(gw)) bias_grad_body(lds, b - nd - nw, gw, ew);
    else adam_pair_body(ad, b - nd - nw - bias_tiles(gw));
    PVAE_MARK(0, 3);
}

// The same fused launch with the input gradient on 64x32 tiles (splitk_reg64_body; 48 KB of LDS per workgroup): 512 rows
// and more.
template <class EpiD, class EpiW>
__global__ void __launch_bounds__(256)
bwd_pair64_kernel(PVAE_GA2_PARAMS, EpiD ed, EpiW ew, AdamPair ad) {
    __shared__ __attribute__((aligned(16))) float lds[kReg64RingFloats];
    const GemmArgs gd = PVAE_GA2_A, gw = PVAE_GA2_B;
    const int nd = ga_grid(gd), nw = ga_grid(gw);
    const int b = blockIdx.x;
    if (b < nd) splitk_reg64_body<EpiD>(lds, b, gd, ed);
    else if (b < nd + nw) wgrad_body<EpiW>(lds, b - nd, gw, ew);
    else if (b < nd + nw + bias_tiles(gw)) bias_grad_body(lds, b - nd - nw, gw, ew);
    else adam_pair_body(ad, b - nd - nw - bias_tiles(gw));
}
}  // namespace pvae
