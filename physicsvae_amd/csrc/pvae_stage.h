// pvae_stage.h -- minibatch staging (no contraction): one batch row of one time step into the input and target panels.
#pragma once
#include "pvae_gemm_common.h"

namespace pvae {
// ---------------------------------------------------------------------------------------
// minibatch staging (device side; launched as stage_batch_kernel or as tail blocks of the step's
// last weight-gradient launch)
// ---------------------------------------------------------------------------------------
// One call = one (padded) batch row r of time step t.  Builds the network input panels and the two
// target panels from either the HBM-resident demonstration set (window_row != null: step t of
// window i reads rows s+t and s+t+1 of `states`, row s+t of `actions`; tpv:133-156 windows,
// tm:52-56 float64->float32, tm:166-175 collate) or explicit x[rows][L][2Db] / y[rows][L][Da]
// (tpv:365-376).  Pad rows and pad columns are written as zeros so that every GEMM can run on
// whole tiles without bounds checks.  Time step t lives in row block t of every panel
// (pvae_layout.h).  For t > 0 the current-state columns are left zero here: they are the world
// model's own prediction of step t-1 (tpv:421), copied in by scatter_state_kernel during the
// forward pass.  `wm_pred` (L > 1 only) is the input panel of the world-model invocations that
// take the decoder's action.
struct StageArgs {
    const float* states;
    const float* next_states;     // null: the second half of x / the target s2 is the NEXT row of `states`;
                                  // else row-aligned with `states` (cond "rel": s_{t+1} - s_t, tpv:149-150)
    const float* actions;
    const int32_t* window_row;
    long long first_window;
    const float* x;
    const float* y;
    int rows, rows_pad, Db, Da, L;
    float* te_in; int ld_te;
    float* md_in; int ld_md;
    float* wm_in; int ld_wm;
    float* s2; int ld_s2;
    float* act_t; int ld_a;
    float* wm_pred;
    float* pr_in; int ld_pr;      // input panel of the learned prior stack [s1 | 0] (null: no such stack)
    int in_off = 0;               // input subsets (pvae_config.te_inputs / md_inputs): blocks written as ZEROS -- 1: the encoder's
                                  // s_t, 2: the encoder's s_{t+1}, 4: the decoder's s_t (the weights there are structural zeros;
                                  // a zero operand keeps their gradient exactly zero)
};

__device__ inline void stage_row(const StageArgs& a, int r, int t, int rows_pad) {
    const int Db = a.Db, Da = a.Da;
    const size_t prow = (size_t)t * rows_pad + r;          // row inside the stacked panels
    const bool valid = r < a.rows;
    const bool first = t == 0;
    const float* p1 = nullptr;
    const float* p2 = nullptr;
    const float* pa = nullptr;
    if (valid) {
        if (a.window_row) {
            const long long s = (long long)a.window_row[a.first_window + r] + t;
            p1 = a.states + s * Db;
            p2 = a.next_states ? a.next_states + s * Db : p1 + Db;
            pa = a.actions + s * Da;
        } else {
            p1 = a.x + ((size_t)r * a.L + t) * 2 * Db;
            p2 = p1 + Db;
            pa = a.y ? a.y + ((size_t)r * a.L + t) * Da : nullptr;
        }
    }
    int ld_max = a.ld_te;
    if (a.ld_md > ld_max) ld_max = a.ld_md;
    if (a.ld_wm > ld_max) ld_max = a.ld_wm;
    for (int c = threadIdx.x; c < ld_max; c += 256) {
        if (a.pr_in && c < a.ld_pr) a.pr_in[prow * a.ld_pr + c] = (valid && first && c < Db) ? p1[c] : 0.f;
        const float v1 = (valid && first && c < Db) ? p1[c] : 0.f;
        const float v2 = (valid && c < Db) ? p2[c] : 0.f;
        const float va = (valid && pa && c < Da) ? pa[c] : 0.f;
        if (c < a.ld_te) {
            float u = v1;
            if (c >= Db) u = (valid && c < 2 * Db) ? p2[c - Db] : 0.f;
            if (a.in_off & (c < Db ? 1 : 2)) u = 0.f;
            a.te_in[prow * a.ld_te + c] = u;
        }
        if (c < a.ld_md) a.md_in[prow * a.ld_md + c] = (a.in_off & 4) ? 0.f : v1;      // z columns filled by reparam
        if (c < a.ld_wm) {
            float u = v1;
            if (c >= Db) u = (valid && pa && c < Db + Da) ? pa[c - Db] : 0.f;
            a.wm_in[prow * a.ld_wm + c] = u;
            if (a.wm_pred) a.wm_pred[prow * a.ld_wm + c] = c < Db ? v1 : 0.f;   // a_hat columns filled by the decoder
        }
        if (c < a.ld_s2) a.s2[prow * a.ld_s2 + c] = v2;
        if (c < a.ld_a) a.act_t[prow * a.ld_a + c] = va;
    }
}

// The same row by ONE wave with every source load in flight before the first store (the stand-alone gather launch:
// stage_batch_kernel, four rows per workgroup).  Lane l owns columns l + 64 k of every panel, so each load and each
// store instruction of the wave covers 256 contiguous bytes -- whole 128-byte lines on the panel side (rows are
// 64-float aligned), and on the source side as well as rows of dim_body / dim_action floats allow (they are 4-byte
// aligned only, which is why the copy is dword-granular: 16-byte accesses would straddle).  Every access is a BUFFER
// access through a descriptor that spans exactly one source row / one panel row: a load past the row's end returns 0
// and a store past it is dropped by the address unit, which is precisely "pad columns are zero" / "this panel is
// narrower" -- so the body has no branch at all and hipcc's wait counts stay exact: per chunk of 512 columns up to
// 5 x 8 independent loads ([s_t | s_{t+1}] is ONE contiguous run of 2 Db floats of `states`; the target panel and the
// action columns of the world-model panel re-read it at their own lane mapping: L1 hits) and only then the stores,
// which retire in the background while the wave's next chunk / the SIMD's other seven waves load.  The dataset rows
// are read once per epoch: nontemporal loads.  Same values as stage_row / stage_row_vec, bit for bit (a copy).
// `w` = the wave's index inside the workgroup, wave-uniform by construction (readfirstlane'd by the caller).
__device__ inline void stage_row_wave(const StageArgs& a, int r, int t, int rows_pad, int lane) {
    const int Db = a.Db, Da = a.Da;
    const size_t prow = (size_t)t * rows_pad + r;
    const bool valid = r < a.rows;
    const bool first = t == 0;
    const float* p1 = a.te_in;                          // (any mapped address: descriptors of absent rows have length 0)
    const float* p2 = a.te_in;
    const float* pa = a.te_in;
    bool have_a = false;
    if (valid) {
        if (a.window_row) {
            const long long s = (long long)__builtin_amdgcn_readfirstlane(a.window_row[a.first_window + r]) + t;
            p1 = a.states + s * Db;
            p2 = a.next_states ? a.next_states + s * Db : p1 + Db;
            pa = a.actions + s * Da;
            have_a = true;
        } else {
            p1 = a.x + ((size_t)r * a.L + t) * 2 * Db;
            p2 = p1 + Db;
            if (a.y) { pa = a.y + ((size_t)r * a.L + t) * Da; have_a = true; }
        }
    }
    int ld_max = a.ld_te;
    if (a.ld_md > ld_max) ld_max = a.ld_md;
    if (a.ld_wm > ld_max) ld_max = a.ld_wm;
    if (a.ld_s2 > ld_max) ld_max = a.ld_s2;
    if (a.ld_a > ld_max) ld_max = a.ld_a;
    if (a.pr_in && a.ld_pr > ld_max) ld_max = a.ld_pr;
    constexpr int kFlags = 0x00020000, kNt = 2;         // raw buffer, 32-bit data; aux bit 1 = nontemporal
    const auto src = [](const float* p, int n) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, n * 4, kFlags); };
    const auto dst = [&](float* p, int ld) { return __builtin_amdgcn_make_buffer_rsrc(p ? p + prow * ld : a.te_in, 0, p ? ld * 4 : 0, kFlags); };
    const __amdgpu_buffer_rsrc_t rs1 = src(p1, valid && first ? Db : 0), rs2 = src(p2, valid ? Db : 0), ra = src(pa, have_a ? Da : 0);
    const __amdgpu_buffer_rsrc_t dte = dst(a.te_in, a.ld_te), dmd = dst(a.md_in, a.ld_md), dwm = dst(a.wm_in, a.ld_wm),
                                 dwp = dst(a.wm_pred, a.ld_wm), dpr = dst(a.pr_in, a.ld_pr), ds2 = dst(a.s2, a.ld_s2),
                                 dac = dst(a.act_t, a.ld_a);
    constexpr int KC = 8;                               // columns per lane and chunk
    for (int c0 = 0; c0 < ld_max; c0 += 64 * KC) {
        float v1[KC], v2[KC], vt[KC], vw[KC], va[KC];   // s1, s2 at the encoder's mapping; s2 at the target's; action at the world model's; action
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const int c = c0 + 64 * k + lane;           // (offsets below zero wrap to far beyond any row: read as 0)
            v1[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs1, (unsigned)c * 4u, 0, kNt));
            v2[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs2, (unsigned)(c - Db) * 4u, 0, kNt));
            vt[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs2, (unsigned)c * 4u, 0, kNt));
            vw[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, (unsigned)(c - Db) * 4u, 0, kNt));
            va[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, (unsigned)c * 4u, 0, kNt));
        }
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const int c = c0 + 64 * k + lane;
            const unsigned off = (unsigned)c * 4u;
            const unsigned u1 = __builtin_bit_cast(unsigned, v1[k]);
            __builtin_amdgcn_raw_buffer_store_b32(u1, dpr, off, 0, 0);
            const float ute = (a.in_off & (c < Db ? 1 : 2)) ? 0.f : (c < Db ? v1[k] : v2[k]);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, ute), dte, off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32((a.in_off & 4) ? 0u : u1, dmd, off, 0, 0);   // z columns filled by the sampler
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, c < Db ? v1[k] : vw[k]), dwm, off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(u1, dwp, off, 0, 0);            // a_hat columns filled by the decoder
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vt[k]), ds2, off, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, va[k]), dac, off, 0, 0);
        }
    }
}

// The same row by one wave THROUGH LDS (what the stand-alone gather launch runs when a row's sources fit the wave's
// 8 KB of LDS): the sources -- [s_t | s_{t+1}] and a_t, 4-byte aligned runs of dim_body / dim_action floats -- land in
// LDS by LDS-DMA (global_load_lds_dword: 256 contiguous bytes per instruction, no register, nothing waited for until
// all of the row is in flight: ceil((2 Db + Da) / 64) instructions), and every panel row is then written with whole
// 16-byte stores assembled from LDS (the misalignment between a source run and the 64-float-aligned panel is absorbed
// by the LDS reads, which cost nothing next to the memory system).  Per window at the configs[2] dims: 8 loads + 6
// stores instead of stage_row_wave's 40 + 56 dword-granular buffer instructions (most of them out of range), which
// made that form instruction-bound (16.2 us per 8192 windows against 13.3 for stage_row_vec).  Bit-identical (a copy).
constexpr int kStageLdsFloats = 2048;                   // per wave, at most (the launch sizes it to the row: stage_lds_floats)
__device__ inline void stage_row_lds(const StageArgs& a, int r, int t, int rows_pad, int lane, float* sl, int mask) {
    const int Db = a.Db, Da = a.Da;
    const size_t prow = (size_t)t * rows_pad + r;
    const bool valid = r < a.rows;
    const bool first = t == 0;
    bool have_a = false;
    if (valid) {
        const float* p1; const float* p2; const float* pa = nullptr;
        if (a.window_row) {
            const long long s = (long long)__builtin_amdgcn_readfirstlane(a.window_row[a.first_window + r]) + t;
            p1 = a.states + s * Db;
            p2 = a.next_states ? a.next_states + s * Db : p1 + Db;
            pa = a.actions + s * Da;
        } else {
            p1 = a.x + ((size_t)r * a.L + t) * 2 * Db;
            p2 = p1 + Db;
            if (a.y) pa = a.y + ((size_t)r * a.L + t) * Da;
        }
        have_a = pa != nullptr;
        // LDS image: [0, Db) s1, [Db, 2 Db) s2, [2 Db, 2 Db + Da) action; the tail of each 64-float DMA group that
        // reaches past a run lands in the next run's space (overwritten by that run's own DMA, issued later) or past
        // the end (never read).  Order: s1, s2, action.
        auto dma = [&](const float* src, int n, int dst0) {
            for (int c = 0; c < n; c += 64) {
                const int cc = c + lane < n ? c + lane : n - 1;          // (clamped: no read past the run)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + cc),
                                                 (__attribute__((address_space(3))) void*)(sl + dst0 + c), 4, 0, 2);
            }
        };
        if (p2 == p1 + Db) dma(p1, 2 * Db, 0);
        else { dma(p1, Db, 0); dma(p2, Db, Db); }
        if (have_a) dma(pa, Da, 2 * Db);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // value(c) = (LDS index, condition): the read is unconditional (any index inside the wave's region is safe), the
    // zero-fill a select -- no divergent branch per element
    auto put = [&](float* panel, int ld, auto&& where) {                 // 16 bytes per lane and trip
        if (!panel) return;
        float* row = panel + prow * ld;
        // (read j of lane l takes element (j + l / 8) & 3 of the lane's four: lanes l, l + 8, l + 16, l + 24 -- whose
        //  elements would share a bank, 4 l + e mod 32 -- hit four different banks; PMC: 70 % conflict cycles without)
        const int rot = (lane >> 3) & 3;
        for (int c = lane * 4; c < ld; c += 256) {
            v4f v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = (j + rot) & 3;
                int idx; bool on;
                where(c + e, idx, on);
                const float raw = sl[idx & mask];                 // (unconditional: any masked index is inside the wave's image)
                const float x = on ? raw : 0.f;
                v[0] = e == 0 ? x : v[0];
                v[1] = e == 1 ? x : v[1];
                v[2] = e == 2 ? x : v[2];
                v[3] = e == 3 ? x : v[3];
            }
            *reinterpret_cast<v4f*>(row + c) = v;
        }
    };
    const bool s1_on = valid && first;
    const bool te_b = s1_on && !(a.in_off & 1), te_t = valid && !(a.in_off & 2), md_b = s1_on && !(a.in_off & 4);
    put(a.te_in, a.ld_te, [&](int c, int& i, bool& on) { i = c; on = c < Db ? te_b : (te_t && c < 2 * Db); });
    put(a.md_in, a.ld_md, [&](int c, int& i, bool& on) { i = c; on = md_b && c < Db; });           // z columns filled by the sampler
    put(a.wm_in, a.ld_wm, [&](int c, int& i, bool& on) { i = c < Db ? c : c + Db; on = c < Db ? s1_on : (have_a && c < Db + Da); });
    put(a.wm_pred, a.ld_wm, [&](int c, int& i, bool& on) { i = c; on = s1_on && c < Db; });        // a_hat columns filled by the decoder
    put(a.pr_in, a.ld_pr, [&](int c, int& i, bool& on) { i = c; on = s1_on && c < Db; });
    put(a.s2, a.ld_s2, [&](int c, int& i, bool& on) { i = Db + c; on = valid && c < Db; });
    put(a.act_t, a.ld_a, [&](int c, int& i, bool& on) { i = 2 * Db + c; on = have_a && c < Da; });
}
}  // namespace pvae
