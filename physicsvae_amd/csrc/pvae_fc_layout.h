// pvae_fc_layout.h -- host-side layout arithmetic of a STACK SET (include/pvae.h pvae_fc_*): S independent fully
// connected stacks on one shared input (rmt:323-457: the policy, the value function and the optional log-std function of
// FullyConnectedPolicy all read the same observation).  Pure C++ (no HIP), so the layout queries work without a GPU.
//
// Arena: the padding rules of pvae_layout.h (W[n_out_pad][ld] row-major, ld = n_in rounded up to 64, n_out_pad = n_out
// rounded up to 64, bias[n_out_pad], pads zero), in this order:
//   [ W_0 of stack 0 | W_0 of stack 1 | ... | b_0 of stack 0 | b_0 of stack 1 | ... |  then per stack: W_1 b_1 W_2 b_2 ... ]
// The first layers share their input, hence their ld: stored back to back they are ONE weight block
// W_0[n0][ld0] (n0 = sum of the stacks' padded first-layer widths) with ONE bias vector -- the operands of one GEMM over
// the concatenated output features, and of one input-gradient GEMM whose contraction over n0 IS the sum over the stacks.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pvae_layout.h"

namespace pvae {

inline int g_fc_per_stack = 0;        // pvae_set_option(NULL, "fc_per_stack", 1): one launch per stack instead of one per depth

struct FcLayer {
    int stack, index, n_in, n_out, ld, n_out_pad;
    int64_t w_off, b_off;
    bool last;
    int act;                      // act_apply / act_grad code of the layer's output: 0 linear, 1 + PVAE_ACT_* otherwise
    int col0;                     // layer 0: first column of this stack's block in the shared first-layer panels
};

struct FcLayout {
    pvae_fc_config cfg{};
    int S = 0;
    std::vector<FcLayer> stack[PVAE_FC_MAX_STACKS];
    int ld0 = 0, n0 = 0;          // row stride of the input panel; width of the shared first-layer panels
    int max_layers = 0;           // layers of the deepest stack
    int64_t b0_off = 0;           // the concatenated first-layer bias
    int64_t arena_floats = 0;
    bool ok = false;
    const char* why = "";
};

inline FcLayout make_fc_layout(const pvae_fc_config& c) {
    FcLayout L;
    L.cfg = c;
    if (c.n_stacks < 1 || c.n_stacks > PVAE_FC_MAX_STACKS) { L.why = "n_stacks must be in [1, 4]"; return L; }
    if (c.n_in < 1 || c.n_in > 65472) { L.why = "n_in out of range"; return L; }
    if (c.max_batch <= 0 || c.max_batch > 65536) { L.why = "max_batch out of range"; return L; }
    L.S = c.n_stacks;
    L.ld0 = pad64(c.n_in);
    for (int s = 0; s < L.S; ++s) {
        if (c.depth[s] < 0 || c.depth[s] > PVAE_MAX_HIDDEN) { L.why = "depth must be in [0, 15]"; return L; }
        if (c.n_out[s] < 1) { L.why = "n_out must be positive"; return L; }
        int prev = c.n_in;
        for (int i = 0; i <= c.depth[s]; ++i) {
            FcLayer l{};
            l.stack = s; l.index = i; l.n_in = prev;
            l.last = i == c.depth[s];
            l.n_out = l.last ? c.n_out[s] : c.width[s][i];
            if (l.n_out < 1) { L.why = "hidden width must be positive"; return L; }
            const int a = l.last ? PVAE_ACT_LINEAR : c.act[s][i];
            if (a < 0 || a > PVAE_ACT_LINEAR) { L.why = "unknown activation"; return L; }
            l.act = a == PVAE_ACT_LINEAR ? 0 : a + 1;
            l.ld = pad64(prev);
            l.n_out_pad = pad64(l.n_out);
            if (l.ld >= 65536 || l.n_out_pad >= 65536) { L.why = "layer wider than 65535 (padded) unsupported"; return L; }
            L.stack[s].push_back(l);
            prev = l.n_out;
        }
        if ((int)L.stack[s].size() > L.max_layers) L.max_layers = (int)L.stack[s].size();
    }
    int64_t off = 0;
    for (int s = 0; s < L.S; ++s) {                       // the shared first-layer weight block
        FcLayer& l = L.stack[s][0];
        l.col0 = L.n0;
        l.w_off = off; off += (int64_t)l.n_out_pad * l.ld;
        L.n0 += l.n_out_pad;
    }
    if (L.n0 >= 65536) { L.why = "first layers wider than 65535 (padded, summed) unsupported"; return L; }
    L.b0_off = off;
    for (int s = 0; s < L.S; ++s) { L.stack[s][0].b_off = off; off += L.stack[s][0].n_out_pad; }
    for (int s = 0; s < L.S; ++s)
        for (size_t i = 1; i < L.stack[s].size(); ++i) {
            FcLayer& l = L.stack[s][i];
            l.w_off = off; off += (int64_t)l.n_out_pad * l.ld;
            l.b_off = off; off += l.n_out_pad;
        }
    L.arena_floats = off;
    L.ok = true;
    return L;
}

// Workspace (offsets in floats, every buffer 64-float aligned): the input panel and its gradient [Bp][ld0], the shared
// first-layer output panel and its gradient [Bp][n0], and per stack and deeper layer an output panel and a gradient panel
// [Bp][n_out_pad].  Bp = max_batch rounded up to 32.
struct FcWork {
    int Bp = 0;
    int64_t in = 0, d_in = 0, act0 = 0, dz0 = 0;
    std::vector<int64_t> act[PVAE_FC_MAX_STACKS], dz[PVAE_FC_MAX_STACKS];     // index 0 unused (the shared panels)
    int64_t total_floats = 0;
};

inline FcWork make_fc_work(const FcLayout& L) {
    FcWork W;
    W.Bp = pad32(L.cfg.max_batch);
    int64_t off = 0;
    auto take = [&](int64_t n) { int64_t o = off; off += (n + 63) / 64 * 64; return o; };
    W.in = take((int64_t)W.Bp * L.ld0);
    W.d_in = take((int64_t)W.Bp * L.ld0);
    W.act0 = take((int64_t)W.Bp * L.n0);
    W.dz0 = take((int64_t)W.Bp * L.n0);
    for (int s = 0; s < L.S; ++s)
        for (size_t i = 0; i < L.stack[s].size(); ++i) {
            W.act[s].push_back(i ? take((int64_t)W.Bp * L.stack[s][i].n_out_pad) : 0);
            W.dz[s].push_back(i ? take((int64_t)W.Bp * L.stack[s][i].n_out_pad) : 0);
        }
    W.total_floats = off;
    return W;
}

}  // namespace pvae
