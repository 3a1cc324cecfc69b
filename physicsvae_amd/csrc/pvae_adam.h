// pvae_adam.h -- the Adam update on the device: per element, per float4, and as the deferred-update workgroups of a later launch.
#pragma once
#include "pvae_gemm_common.h"

namespace pvae {
struct AdamScalars {
    float step_size;          // lr / (1 - beta1^t)
    float inv_bc2_sqrt;       // 1 / sqrt(1 - beta2^t)
    float beta1, beta2, eps;
    float one_minus_beta1, one_minus_beta2;   // computed in double on the host, as torch does
    float weight_decay = 0.f;                 // L2 term folded into the gradient (0: the trainer's setting)
};

// torch.optim.Adam single-tensor update (amsgrad False), tm:119-122,143:
//   g <- g + weight_decay p (when set) ; m <- m + (g - m)(1 - b1) ; v <- v b2 + (1 - b2) g g ; p <- p - step_size * m / (sqrt(v)/bc2_sqrt + eps)
__device__ inline void adam_update(float g, float& p, float& m, float& v, const AdamScalars& s) {
    // Moments: every operation pinned (no context-dependent fma contraction), so the fused
    // epilogue and the flat multi-tensor kernel stay bit-identical.  Step: v_sqrt_f32 / v_rcp_f32
    // (1 ulp) instead of the correctly rounded sequences (~10x the instructions); the term they
    // feed is scaled by lr/(1-b1^t) ~ 5e-4 before it meets p, so p moves by < 0.1 ulp of itself.
    if (s.weight_decay != 0.f) g = __fmaf_rn(s.weight_decay, p, g);
    m = __fmaf_rn(__fsub_rn(g, m), s.one_minus_beta1, m);
    v = __fmaf_rn(v, s.beta2, __fmul_rn(__fmul_rn(s.one_minus_beta2, g), g));
    const float denom = __fmaf_rn(__builtin_amdgcn_sqrtf(v), s.inv_bc2_sqrt, s.eps);
    p = __fmaf_rn(-s.step_size, __fmul_rn(m, __builtin_amdgcn_rcpf(denom)), p);
}

__device__ inline void adam_update4(const v4f& g, v4f& p, v4f& m, v4f& v, const AdamScalars& s) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_update(g[e], pe, me, ve, s);
        p[e] = pe; m[e] = me; v[e] = ve;
    }
}

// Deferred Adam: a layer whose weight gradient went to the gradient arena in the PREVIOUS launch is
// updated by `kAdamBlocks` extra workgroups of the current one (p, g, m, v streamed while the other
// workgroups contract).  With Adam in the weight-gradient epilogue every workgroup of the launch does
// its update at the same moment, after the matrix pipe has gone idle: 15.7 us for the fused pair
// against 12.7 with a plain gradient store; store + 256 co-resident update workgroups: 14.2
// (tools/pair_probe.hip).  Same arithmetic as the epilogue and as adam_flat_kernel: bit-identical.
struct AdamSeg {
    float* p = nullptr;
    const float* g = nullptr;
    float* m = nullptr;
    float* v = nullptr;
    long long n4 = 0;          // float4 count (0: nothing pending)
    AdamScalars s{};
};
constexpr int kAdamBlocks = 256;    // workgroups per deferred-Adam segment (128 / 512 measured slower: profiles/r03_ab_adam_blocks.txt)
__device__ inline void adam_seg_body(const AdamSeg& a, int blk) {
    // (one float4 per thread in flight: two or four, and a delayed start, measured no better -- docs/experiments.md round 2)
    constexpr long long kStride = kAdamBlocks * 256ll;
    for (long long i = blk * 256ll + threadIdx.x; i < a.n4; i += kStride) {
        v4f pp = reinterpret_cast<v4f*>(a.p)[i];
        const v4f gg = reinterpret_cast<const v4f*>(a.g)[i];
        v4f mm = reinterpret_cast<v4f*>(a.m)[i];
        v4f vv = reinterpret_cast<v4f*>(a.v)[i];
        adam_update4(gg, pp, mm, vv, a.s);
        store_stream(a.p + 4 * i, pp);
        store_stream(a.m + 4 * i, mm);
        store_stream(a.v + 4 * i, vv);
    }
}
inline int adam_blocks(const AdamSeg* a) { return a && a->n4 > 0 ? kAdamBlocks : 0; }
// What one launch carries: up to two pending updates (a launch with little work of its own passes a big segment on to
// the next wide one and takes a small one instead: see take_pending in pvae.hip), kAdamBlocks workgroups each.
struct AdamPair {
    AdamSeg s[2];
    AdamPair() {}
    AdamPair(const AdamSeg& a) { s[0] = a; }                  // (probes under tools/ pass a single segment)
};
inline int adam_blocks(const AdamPair* p) { return p ? adam_blocks(&p->s[0]) + adam_blocks(&p->s[1]) : 0; }
__device__ inline void adam_pair_body(const AdamPair& p, int blk) {
    if (p.s[0].n4 > 0) {
        if (blk < kAdamBlocks) { adam_seg_body(p.s[0], blk); return; }
        blk -= kAdamBlocks;
    }
    adam_seg_body(p.s[1], blk);
}
}  // namespace pvae
