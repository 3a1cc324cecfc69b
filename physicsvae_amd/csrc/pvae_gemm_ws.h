// pvae_gemm_ws.h -- wave-specialised LDS-DMA forward / input-gradient bodies (32x32, 64x32, 64x64 tiles) and their six kernels.
#pragma once
#include "pvae_gemm_common.h"
#include "pvae_gemm_src.h"
#include "pvae_gemm_reg.h"

namespace pvae {
// ---- forward / dgrad, wave-specialised LDS-DMA ring (512 threads) ----------------------------
// 8 waves = 4 compute + 4 loaders.  The loaders only issue global_load_lds_dwordx4 (tiles land in
// LDS without touching a VGPR) into a ring of kWsStages slots and certify "tile t+1 has landed"
// at barrier t; the compute waves do nothing but ds_read_b128/b64 + MFMA, with the fragments of
// tile t+1 read while the MFMAs of tile t run.  An LDS-DMA instruction costs ~150 issue cycles,
// which is why it must not sit in the instruction stream that feeds the matrix pipe (a 4-wave
// DMA ring measured 9.5 us for 256x1024x1024; this one 7.7 us; the register-staged loop 8.45).
// Ring depth: 4 is the optimum on MI355X -- 3 starves, 5..8 get progressively slower (8: 8.5 us);
// more requests in flight per CU do not help the L2 -> CU path, they hurt it.
// Same LDS image / swizzles / split-K layout as splitk_reg_body, results are bit-identical.
// Ring of the plain 32x32 kernel: SIX slots, super-steps of TWO k-tiles per workgroup barrier -- at the barrier in front of
// tiles (t0, t0+1) the tiles t0+1, t0+2 have landed, t0+3, t0+4 are in flight and t0+5, t0+6 are requested: half the
// barriers, a continuous load stream (joint step 243.7 -> 241.5 us).  The same on a 4-slot ring leaves nothing in flight
// across a barrier and loses 9 % (profiles/r03_ab_ws_superstep.txt).  The Pro variant (a patch needs its own barrier per
// patched tile) keeps one barrier per tile on four slots.
constexpr int kWsLoaders = 4, kWsThreads = 256 + 64 * kWsLoaders, kWsPer = 8 / kWsLoaders;   // DMA pairs per loader wave and tile
constexpr int kWsStages = 4;
constexpr int kWsFloats = kWsStages * 2 * 32 * 64;       // 64 KB

template <int N>
__device__ inline void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ inline void lds_dma16(const float* src, float* dst_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst_wave_base, 16, 0, 0);
}
// The same DMA with a wave-uniform 64-bit base in SGPRs and a per-lane 32-bit byte offset (scalar-base form).  A loader
// wave shares its SIMD with a compute wave whose back-to-back fp32 MFMAs hold the vector issue (tools/dual_pipe.hip:
// other waves' vector-ALU instructions drop to a fifth of their rate), so the loaders' steady state must issue NO
// vector-ALU instruction: the lane offsets are computed once in front of the loop, one VGPR per DMA piece of a tile (no
// piece waits for another's address register), and the k-tile advance is scalar arithmetic on the base.  hipcc turns
// `base + offset` handed to the builtin back into a 64-bit vector add per DMA (v_lshl_add_u64, all pieces through one
// register pair), hence inline assembly; M0 (the LDS destination) is compiler-reserved, so it is saved, written and
// restored inside the statement that reads it, with the wait state the DMA needs after a scalar write of M0.  hipcc does
// not count the instruction: every wait for it is one of the explicit wait_vmcnt<> here, as it already was.
__device__ inline void lds_dma16_sbase(const char* base_uniform, unsigned lane_byte_off, float* dst_wave_base) {
    const unsigned m0v = (unsigned)(size_t)(__attribute__((address_space(3))) void*)dst_wave_base;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(lane_byte_off), "s"(base_uniform), "s"(m0v)
                 : "memory");
}
// A/B switches of the diagnostic builds (build.py defines=["PVAE_LOADER_VADDR"] into ab_libs/).  PVAE_LOADER_VADDR: the
// dense loaders as they were, one 64-bit vector add in front of every DMA.  PVAE_WS_READS_AHEAD: the plain 32x32 body's
// compute waves as they were, the next tile's fragment reads in front of a half-step's MFMAs instead of between them.
#ifdef PVAE_LOADER_VADDR
constexpr bool kLoaderScalarBase = false;
#else
constexpr bool kLoaderScalarBase = true;
#endif
#ifdef PVAE_WS_READS_AHEAD
constexpr bool kReadsUnderMfma = false;
#else
constexpr bool kReadsUnderMfma = true;
#endif
// PVAE_WS_PROLOGUE_SERIAL: the plain dense 32x32 body's prologue as it was -- only k-tile 0 fetched by all eight waves, tile 1
// by the loaders in front of barrier #0 and tiles 2-4 behind it.  PVAE_WS_PROLOGUE_AHEAD=0 / 1 / 2: how many of the loaders'
// tiles 3 and 4 the new prologue requests in front of barrier #0 (1: tile 3 in front, tile 4 behind -- with both in front
// barrier #0 moves 0.2 us later and the step gains nothing; profiles/r09_ab_prologue.txt).
#ifdef PVAE_WS_PROLOGUE_SERIAL
constexpr bool kWidePrologue = false;
#else
constexpr bool kWidePrologue = true;
#endif
#ifndef PVAE_WS_PROLOGUE_AHEAD
#define PVAE_WS_PROLOGUE_AHEAD 1
#endif
constexpr int kPrologueAhead = PVAE_WS_PROLOGUE_AHEAD;     // of the loaders' tiles 3 and 4, how many go in front of barrier #0
static_assert(kPrologueAhead >= 0 && kPrologueAhead <= 2, "tiles 3 and 4");
// Lane offsets are 32-bit: a tile spans at most 64 rows x ld floats (checked where the launches are planned).
inline bool ws_offsets_fit(int ldq, int ldp) { return ldq >= 0 && ldq < (1 << 24) && ldp >= 0 && ldp < (1 << 24); }
// The dense loaders' walk over the k-tiles: tile bases (bytes) and ring slot advance by wrap-around increments, all of it
// wave-uniform (SGPRs; no division per issue).  Tiles are issued strictly in order, starting at step `t`.
struct DenseWalk {
    const char *q0, *p0, *q, *p;      // bases of k-tile 0 and of the next tile to issue
    unsigned long long kq, kp;        // bytes per k-tile
    int kt, nk, slot;
    __device__ inline DenseWalk(const char* qb, const char* pb, unsigned long long kq_, unsigned long long kp_, int nk_)
        : q0(qb), p0(pb), q(qb), p(pb), kq(kq_), kp(kp_), kt(0), nk(nk_), slot(0) {}
    __device__ inline void seek(int kt_, int slot_) { kt = kt_; slot = slot_; q = q0 + kt_ * kq; p = p0 + kt_ * kp; }
    template <int S>
    __device__ inline void next() {
        q += kq; p += kp;
        if (++kt == nk) { kt = 0; q = q0; p = p0; }           // (k_rotation's wrap)
        if (++slot == S) slot = 0;
    }
};
// this wave's DMAs of a tile have landed once at most `younger` tiles (4 instructions each)
// issued after it are still in flight
__device__ inline void wait_dma_tile(int younger) {
    switch (younger) {
        case 0: wait_vmcnt<0>(); break;
        case 1: wait_vmcnt<2 * kWsPer>(); break;
        default: wait_vmcnt<4 * kWsPer>(); break;          // kWsStages - 2 = 2 is the most that can be younger
    }
}

template <bool P_ROW, class Epi, class Pro = NoPro, class QS = QDense>
__device__ inline void splitk_ws_body(float* lds, int bid, const GemmArgs& ga, Epi& epi, const Pro& pro = Pro(),
                                      float* scratch = nullptr, const QS& qs = QS()) {
    // (plain kernel: six slots, two k-tiles per barrier; with a Pro patch: four slots, one barrier per tile)
    constexpr int BK = 64, kTile = 32 * 64, kStage = 2 * kTile, S = Pro::kActive ? kWsStages : 6;
    const float* __restrict__ Q = ga.Q;
    const float* __restrict__ P = ga.P;
    const int ldq = ga.ldq, ldp = ga.ldp, K = ga.K, tiles_q = ga.tiles_q, tiles_p = ga.tiles_p;
    const int xcd = bid & 7, loc = bid >> 3;
    int tile_p = xcd * ga.p_per_xcd + loc / tiles_q;
    int tile_q = loc % tiles_q;
    if (ga.rowxcd && tiles_q == 8 && tiles_p == 8 * ga.p_per_xcd) { tile_q = xcd; tile_p = loc; }
    if (tile_p >= tiles_p) return;
    const int q0 = tile_q * 32, p0 = tile_p * 32;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lh = lane >> 4;
    const int nk = K / BK;
    PVAE_MARK(0, 0);                                             // workgroup entered
    typename Epi::Pre epre{};
    v4f acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = v4f{0.f, 0.f, 0.f, 0.f};

    const size_t kstep_p = P_ROW ? (size_t)BK : (size_t)BK * ldp;
    const int rot = k_rotation(ga, loc, tile_q, nk);
    // Dense operands: wave-uniform byte bases of k-tile 0's two panels + each lane's 32-bit byte offset of 16-byte slot j
    // (the XOR swizzle stays on the source offset) -- see lds_dma16_sbase.  Gathered operands keep per-lane pointers.
    constexpr bool kSB = QS::kAlwaysFast && kLoaderScalarBase;
    const char* const qb0 = reinterpret_cast<const char*>(Q + (size_t)q0 * ldq);
    const char* const pb0 = reinterpret_cast<const char*>(P_ROW ? P + (size_t)p0 * ldp : P + p0);
    auto off_rows = [](int j, int ld) {
        const int row = j >> 4, c = (j & 15) ^ (row & 15);
        return ((unsigned)row * (unsigned)ld + c * 4) * 4u;
    };
    auto off_q = [&](int j) { return off_rows(j, ldq); };
    auto off_p = [&](int j) {
        if (P_ROW) return off_rows(j, ldp);
        const int r = j >> 3, k = r ^ ((r >> 2) & 1);
        return ((unsigned)k * (unsigned)ldp + (j & 7) * 4) * 4u;
    };
    // k-tile 0 is fetched by ALL eight waves (one eighth of each operand image per wave, two DMA
    // instructions each): it is in flight ~0.1 us after the workgroup starts instead of queueing
    // behind the loaders' three-tile prologue (each global_load_lds holds its wave ~150 cycles, so
    // the prologue alone took 0.67 us -- tools/timeline_probe.hip).
    // Plain dense body: so are k-tiles 1 and 2 -- six DMAs per wave through the two lane offsets of tile 0, ring slot and
    // k-tile advanced by the loaders' walk (SGPRs).  All three are requested before anything is waited for: the first
    // super-step's barrier certifies tiles 1 and 2, and behind a loaders-only prologue tile 2 was requested only after tile 0
    // had landed (two memory round trips in a row in front of the first MFMA).  Slots 1-4 have never been read at this point,
    // so the restaging rule of the super-step barrier (see the compute waves) is not involved.
    constexpr bool kWide = kSB && !Pro::kActive && kWidePrologue;
    DenseWalk walk(qb0, pb0, BK * 4, kstep_p * 4, nk);
    unsigned vq[kWsPer], vp[kWsPer];                      // dense loaders: lane offsets of this wave's pieces of a tile
    if constexpr (kWide) {
        const int j = wave * 64 + lane;                   // 16-byte slot inside the 8 KB tile image
        const unsigned vq0 = off_q(j), vp0 = off_p(j);
        // A loader wave's second piece of a tile is its eighth of it; the offsets of its first piece are computed HERE, in
        // front of the DMAs: behind them hipcc puts an s_waitcnt vmcnt(0) in front of the loader path's first vector-ALU
        // instruction (it merges the compute path's pending epilogue preload into that block), and the loaders then request
        // nothing more until everything above has landed.
        static_assert(kWsLoaders == 4 && kWsPer == 2, "loader wave w takes pieces w - 4 and w");
        if (wave >= 4) {
            vq[0] = off_q(j - 256), vp[0] = off_p(j - 256);
            vq[1] = vq0, vp[1] = vp0;
        }
        if (!PVAE_PROBE(6)) {
            walk.seek(rot, 0);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (i < nk) {
                    float* slot = lds + walk.slot * kStage;
                    lds_dma16_sbase(i && PVAE_PROBE(2) ? qb0 : walk.q, vq0, slot + wave * 256);
                    lds_dma16_sbase(i && PVAE_PROBE(2) ? pb0 : walk.p, vp0, slot + kTile + wave * 256);
                    walk.template next<S>();              // (ends on tile 3 / slot 3, where the loaders go on)
                }
        }
    } else if constexpr (kSB) {
        if (!PVAE_PROBE(6) && wave < 8) {
            const int j = wave * 64 + lane;               // 16-byte slot inside the 8 KB tile image
            lds_dma16_sbase(qb0 + (size_t)rot * (BK * 4), off_q(j), lds + wave * 256);
            lds_dma16_sbase(pb0 + (size_t)rot * kstep_p * 4, off_p(j), lds + kTile + wave * 256);
        }
    } else if (!PVAE_PROBE(6) && wave < 8) {
        const int j = wave * 64 + lane;                   // 16-byte slot inside the 8 KB tile image
        typename QS::Base s0q;
        const float* s0p;
        {
            const int row = j >> 4, c = (j & 15) ^ (row & 15);
            s0q = qs.base(Q, ldq, q0 + row, c * 4);
        }
        if (P_ROW) {
            const int row = j >> 4, c = (j & 15) ^ (row & 15);
            s0p = P + (size_t)(p0 + row) * ldp + c * 4;
        } else {
            const int r = j >> 3, k = r ^ ((r >> 2) & 1);
            s0p = P + (size_t)k * ldp + p0 + (j & 7) * 4;
        }
        if (QS::kAlwaysFast || qs.fast(rot)) lds_dma16(qs.tile_fast(s0q, rot), lds + wave * 256);
        else lds_dma16(qs.tile(s0q, rot), lds + wave * 256);
        lds_dma16(s0p + (size_t)rot * kstep_p, lds + kTile + wave * 256);
    }
    if (wave >= 4) {
        // ---------------- loader waves ----------------  (s_setprio 1 here, or on the compute waves: +-0)
        const int u0 = wave - 4;
        typename QS::Base sq[kWsPer];
        const float* sp[kWsPer];
#pragma unroll
        for (int u = 0; u < kWsPer; ++u) {
            const int j = (u0 + kWsLoaders * u) * 64 + lane;       // 16-byte slot inside the 8 KB tile image
            {
                const int row = j >> 4, c = (j & 15) ^ (row & 15);
                sq[u] = qs.base(Q, ldq, q0 + row, c * 4);
            }
            if (P_ROW) {
                const int row = j >> 4, c = (j & 15) ^ (row & 15);
                sp[u] = P + (size_t)(p0 + row) * ldp + c * 4;
            } else {
                const int r = j >> 3, k = r ^ ((r >> 2) & 1);
                sp[u] = P + (size_t)k * ldp + p0 + (j & 7) * 4;
            }
        }
        // dense operands: lane offsets of this wave's pieces (distinct VGPRs), tile walk in SGPRs; issue() is called
        // for t = 1, 2, 3, ... in order, so the walk only ever steps to the next tile
        if constexpr (!kWide) {
#pragma unroll
            for (int u = 0; u < kWsPer; ++u) {
                vq[u] = off_q((u0 + kWsLoaders * u) * 64 + lane);
                vp[u] = off_p((u0 + kWsLoaders * u) * 64 + lane);
            }
            walk.seek(rot + 1 < nk ? rot + 1 : 0, 1);
        }                                                 // (wide prologue: offsets and walk stand as it left them)
        auto issue = [&](int t) {
            if (PVAE_PROBE(6)) return;                    // probe: loaders only keep the barriers
            if constexpr (kSB) {
                float* slot = lds + walk.slot * kStage;
                const char* const qb = PVAE_PROBE(2) ? qb0 : walk.q;   // probe: every step re-reads tile 0 (cache-resident)
                const char* const pb = PVAE_PROBE(2) ? pb0 : walk.p;
#pragma unroll
                for (int u = 0; u < kWsPer; ++u) {
                    lds_dma16_sbase(qb, vq[u], slot + (u0 + kWsLoaders * u) * 256);
                    lds_dma16_sbase(pb, vp[u], slot + kTile + (u0 + kWsLoaders * u) * 256);
                }
                walk.template next<S>();
                return;
            }
            float* slot = lds + (t % S) * kStage;
            int kt = t + rot;                             // k-tile this workgroup reads at step t
            if (kt >= nk) kt -= nk;
            if (PVAE_PROBE(2)) kt = 0;                    // probe: every step re-reads tile 0 (cache-resident)
            if (QS::kAlwaysFast || qs.fast(kt)) {
#pragma unroll
                for (int u = 0; u < kWsPer; ++u) {
                    lds_dma16(qs.tile_fast(sq[u], kt), slot + (u0 + kWsLoaders * u) * 256);
                    lds_dma16(sp[u] + (size_t)kt * kstep_p, slot + kTile + (u0 + kWsLoaders * u) * 256);
                }
            } else {                              // (a gathered first layer's last tiles: the second block, the zero line)
#pragma unroll
                for (int u = 0; u < kWsPer; ++u) {
                    lds_dma16(qs.tile(sq[u], kt), slot + (u0 + kWsLoaders * u) * 256);
                    lds_dma16(sp[u] + (size_t)kt * kstep_p, slot + kTile + (u0 + kWsLoaders * u) * 256);
                }
            }
        };
        if constexpr (kWide) {
            // tile 3 rides on tile 0's flight time, tile 4 follows behind barrier #0 (kPrologueAhead).  This wave's share of
            // tile 0 (its oldest two DMAs) has landed once only its shares of tiles 1, 2 (two each) and its pieces of the
            // tiles requested here (2 * kWsPer each) are in flight.
            static_assert(kWsPer == 2, "the counted waits of the prologue");
            if (3 < nk && kPrologueAhead >= 1) issue(3);
            if (4 < nk && kPrologueAhead >= 2) issue(4);
            PVAE_MARK(256, 4);
            if (4 < nk && kPrologueAhead >= 2) wait_vmcnt<12>();
            else if (3 < nk && kPrologueAhead >= 1) wait_vmcnt<8>();
            else if (2 < nk) wait_vmcnt<4>();
            else if (nk == 2) wait_vmcnt<2>();
            else wait_vmcnt<0>();
        } else {
        if (1 < nk) issue(1);                                    // rides on tile 0's flight time
        PVAE_MARK(256, 4);
        if (1 < nk) wait_vmcnt<2 * kWsPer>(); else wait_vmcnt<0>();   // this wave's share of tile 0 landed
        }
        PVAE_MARK(256, 5);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if constexpr (Pro::kActive) {
            if (pro.needs(0)) __builtin_amdgcn_s_barrier();        // (the compute waves patch tile 0 in between)
        }
        if constexpr (!Pro::kActive) {
            // super-steps of TWO k-tiles per workgroup barrier.  At the barrier in front of tiles (t0, t0+1): t0+1 and t0+2
            // have landed, t0+3 and t0+4 are in flight; the slots of t0-1 and t0 (whose fragment reads the compute waves
            // have retired, see there) take t0+5 and t0+6.
            // (Wide prologue: tiles 1 and 2 came from all eight waves -- this wave's shares are older than its tiles 3 and
            // 4, so the same ladder certifies them at t0 = 0, and the compute waves wait for theirs in front of their loop.)
            if constexpr (kWide) {
                if (3 < nk && kPrologueAhead < 1) issue(3);
                if (4 < nk && kPrologueAhead < 2) issue(4);
            } else {
                if (2 < nk) issue(2);
                if (3 < nk) issue(3);
                if (4 < nk) issue(4);
            }
            for (int t0 = 0; t0 < nk; t0 += 2) {
                const int younger = nk - 3 - t0;                   // tiles t0+3, t0+4 that exist
                if (younger >= 2) wait_vmcnt<4 * kWsPer>();
                else if (younger == 1) wait_vmcnt<2 * kWsPer>();
                else wait_vmcnt<0>();
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if (t0 + 5 < nk) issue(t0 + 5);
                if (t0 + 6 < nk) issue(t0 + 6);
            }
        } else {
#pragma unroll
        for (int t = 2; t < S - 1; ++t)
            if (t < nk) issue(t);
        for (int t = 0; t < nk; ++t) {
            // tile t+1 landed: younger tiles in flight = t+2 .. min(t+S-2, nk-1)
            int y = nk - 2 - t;
            if (y > S - 3) y = S - 3;
            if (y < 0) y = 0;
            wait_dma_tile(y);
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if constexpr (Pro::kActive) {
                if (t + 1 < nk && pro.needs(t + 1)) __builtin_amdgcn_s_barrier();
            }
            if (t + S - 1 < nk) issue(t + S - 1);                  // refill the slot tile t-1 vacated
        }
        }
    } else {
        // ---------------- compute waves ----------------
        int oq[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int row = 16 * a + li;
            oq[a] = row * 64 + (((4 * wave + lh) ^ (row & 15)) << 2);
        }
        const int kq = 16 * wave + 4 * lh;
        // this wave's share of tile 0 landed (wide prologue: its shares of tiles 1 and 2, two DMAs each, may still be in
        // flight -- one wave's DMAs retire in order, tools/lds_dma_order_probe.hip)
        // Wide prologue: the epilogue operands are requested in front of that wait -- the vmcnt(0) in front of the loop waits for
        // them as well, and requested behind the wait they were ~80 ns late for it (timeline probe).  Being younger than the
        // DMAs they only make the counted wait stricter.
        if constexpr (kWide) epre = epi.preload(q0 + (tid >> 3), p0 + ((tid & 7) << 2));
        if (kWide && 2 < nk) wait_vmcnt<4>();
        else if (kWide && 1 < nk) wait_vmcnt<2>();
        else wait_vmcnt<0>();
        if constexpr (!kWide) epre = epi.preload(q0 + (tid >> 3), p0 + ((tid & 7) << 2));   // epilogue operands: arrive under the loop
        typename Pro::State pst = pro.prepare(q0, tid);
        struct Frag { v4f q[2], p[2]; v2f c[4]; };
        auto fread = [&](const float* st, Frag& f) {
#pragma unroll
            for (int a = 0; a < 2; ++a) f.q[a] = *reinterpret_cast<const v4f*>(st + oq[a]);
            if (P_ROW) {
#pragma unroll
                for (int b = 0; b < 2; ++b) f.p[b] = *reinterpret_cast<const v4f*>(st + kTile + oq[b]);
            } else {
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2)
                    f.c[s2] = *reinterpret_cast<const v2f*>(st + kTile + (((kq + s2) ^ (lh & 1)) * 32) + 2 * li);
            }
        };
        auto mfmas = [&](const Frag& f) {
            if (PVAE_PROBE(4)) {                          // probe: no MFMAs (fragments stay live)
                asm volatile("" ::"v"(f.q[0]), "v"(f.q[1]), "v"(f.p[0]), "v"(f.p[1]));
                return;
            }
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const float pv = P_ROW ? f.p[b][s2] : f.c[s2][b];
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv, f.q[a][s2], acc[a][b], 0, 0, 0);
                    }
        };
        // The plain kernel's half-step: the 16 MFMAs of the tile in registers with the NEXT tile's fragment reads between
        // them, one read behind every second MFMA.  All four compute waves leave a barrier together; with the reads in
        // front, their 16 KB queue on the one LDS port while the in-order wave cannot issue an MFMA until its last read
        // has issued, and the matrix pipe drains twice per super-step.  Opened with MFMAs, the pipe is busy from the
        // barrier on and the reads return under it.  (MFMA i of a tile: s2 = i / 4, a = (i / 2) & 1, b = i & 1 -- the
        // order of mfmas(), so every accumulator sees the same sequence.)
        constexpr int kReads = P_ROW ? 4 : 6;                      // ds_read instructions per fragment set
        constexpr int kGap = 2;                                    // MFMAs per read (1 and 3 measured the same)
        auto fread_one = [&](const float* st, Frag& f, int r) {
            if (r < 2) f.q[r] = *reinterpret_cast<const v4f*>(st + oq[r]);
            else if (P_ROW) f.p[r - 2] = *reinterpret_cast<const v4f*>(st + kTile + oq[r - 2]);
            else f.c[r - 2] = *reinterpret_cast<const v2f*>(st + kTile + (((kq + r - 2) ^ (lh & 1)) * 32) + 2 * li);
        };
        auto mfma_range = [&](const Frag& f, int lo, int hi) {
#pragma unroll
            for (int i = lo; i < hi; ++i) {
                const int s2 = i >> 2, a = (i >> 1) & 1, b = i & 1;
                const float pv = P_ROW ? f.p[b][s2] : f.c[s2][b];
                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv, f.q[a][s2], acc[a][b], 0, 0, 0);
            }
        };
        auto half_step = [&](const Frag& cur, Frag& nxt, const float* st) {
            if (PVAE_PROBE(4)) {                          // probe: no MFMAs (one branch per half-step, as mfmas() has)
                fread(st, nxt);
                mfmas(cur);
                return;
            }
#pragma unroll
            for (int r = 0; r < kReads; ++r) {
                mfma_range(cur, kGap * r, kGap * r + kGap);
                __builtin_amdgcn_sched_barrier(0);
                fread_one(st, nxt, r);
                __builtin_amdgcn_sched_barrier(0);
            }
            mfma_range(cur, kGap * kReads, 16);
        };
        __builtin_amdgcn_s_barrier();                              // tile 0 landed
        asm volatile("" ::: "memory");
#ifdef PVAE_TIMELINE
        // (where mark 6 exists, mark 1 is taken here and stored with it: a store counts on vmcnt, and the wide prologue's
        // vmcnt(0) in front of the loop would wait ~80 ns for it)
        constexpr bool kSeenLater = !Pro::kActive && kReadsUnderMfma && QS::kAlwaysFast;
        const unsigned long long t_seen = wall_clock64();
        if (!kSeenLater && tid == 0) g_timeline[(size_t)blockIdx.x * 8 + 1] = t_seen;
#endif
        if constexpr (Pro::kActive) {
            if (pro.needs(0)) {
                pro.patch(lds, scratch, pst, 0, q0, tile_p, tile_q, tid);
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                pro.publish(scratch, 0, tile_p, tile_q, tid);
            }
        }
        Frag F0, F1;
        fread(lds, F0);
        if constexpr (!Pro::kActive) {
            // The fragments of tile t0 (read in the second half of the previous super-step) must have LEFT the LDS before
            // the barrier of a super-step: behind it the loaders restage that slot (tile t0+6) and the slot of t0-1 (tile
            // t0+5), ONE phase after their last reads -- and nothing orders an LDS-DMA write behind a ds_read that is still
            // queued (cdna_hip_programming.md: restage >= 2 phases after the last read, or 1 phase when an lgkmcnt retired
            // the reads first).  Alone on the chip the reads return in ~100 cycles and the DMA data arrives >= 1000 cycles
            // later; with other processes' workgroups on the same CU saturating its LDS port the window opens: round 5
            // saw ~1 wrong 16- or 32-row tile per 100 hidden-layer launches with 4-8 processes on one GPU
            // (tools/p2p_race_hunt.py; the one-barrier-per-tile ring restages two phases later and never showed it).
            // The wait is free: the reads were issued among or before the 16 MFMAs of the previous half-step.
            auto superstep_barrier = [&]() {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                      // tiles t0+1 and t0+2 landed; slots of t0-1, t0 are free
                asm volatile("" ::: "memory");
            };
            // wide prologue: this wave's shares of tiles 1 and 2 landed -- certified by the first super-step's barrier, which
            // waits for the loaders' shares of the same tiles anyway; nothing is added inside the loop
            if constexpr (kWide) wait_vmcnt<0>();
            if constexpr (kReadsUnderMfma && QS::kAlwaysFast) {    // (dense operands; the gathered first layers keep their loop)
                // Whole super-steps without a branch inside (behind a branch hipcc sinks the first half's reads into the
                // second half, in front of its MFMAs), then the odd tile: one barrier per super-step, as the loaders count
                // them.  A read is still never issued ahead of the barrier that certifies its tile: the reads of t0+1 and
                // t0+2 both follow the barrier of their super-step (the last super-step reads a stale slot, never used).
                int t0 = 0, s1 = 1, s2 = 2;                        // ring slots of tiles t0+1, t0+2
#ifdef PVAE_TIMELINE
                // (timeline builds: the first super-step stands in front of the loop, for the mark at its barrier's exit)
                if (1 < nk) {
                    superstep_barrier();
                    PVAE_MARK(0, 6);                               // first super-step open
                    if (tid == 0) g_timeline[(size_t)blockIdx.x * 8 + 1] = t_seen;
                    __builtin_amdgcn_sched_barrier(0);
                    half_step(F0, F1, lds + s1 * kStage);
                    half_step(F1, F0, lds + s2 * kStage);
                    t0 = 2, s1 = 3, s2 = 4;
                }
#endif
                for (; t0 + 1 < nk; t0 += 2) {
                    superstep_barrier();
                    __builtin_amdgcn_sched_barrier(0);             // (and no MFMA of this super-step ahead of the barrier)
                    half_step(F0, F1, lds + s1 * kStage);
                    half_step(F1, F0, lds + s2 * kStage);
                    s1 = s1 + 2 >= S ? s1 + 2 - S : s1 + 2;
                    s2 = s2 + 2 >= S ? s2 + 2 - S : s2 + 2;
                }
                if (t0 < nk) {
                    superstep_barrier();
#ifdef PVAE_TIMELINE
                    if (t0 == 0) {                                 // (a single k-tile: its only barrier)
                        PVAE_MARK(0, 6);
                        if (tid == 0) g_timeline[(size_t)blockIdx.x * 8 + 1] = t_seen;
                    }
#endif
                    __builtin_amdgcn_sched_barrier(0);
                    mfmas(F0);
                }
            } else {
            for (int t0 = 0; t0 < nk; t0 += 2) {
                superstep_barrier();
                fread(lds + ((t0 + 1) % S) * kStage, F1);          // (past the end: stale slot, never used)
                __builtin_amdgcn_sched_barrier(0);
                mfmas(F0);
                if (t0 + 1 < nk) {
                    fread(lds + ((t0 + 2) % S) * kStage, F0);
                    __builtin_amdgcn_sched_barrier(0);
                    mfmas(F1);
                }
            }
            }
        } else
        for (int t0 = 0; t0 < nk; t0 += 2) {
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const int t = t0 + d;
                if (t < nk) {
                    Frag& F = d ? F1 : F0;
                    Frag& Gf = d ? F0 : F1;
                    __builtin_amdgcn_s_barrier();                  // tile t+1 landed; tile t-1's slot is free
                    asm volatile("" ::: "memory");
                    if constexpr (Pro::kActive) {
                        if (t + 1 < nk && pro.needs(t + 1)) {
                            pro.patch(lds + ((t + 1) % S) * kStage, scratch, pst, t + 1, q0, tile_p, tile_q, tid);
                            __builtin_amdgcn_s_barrier();
                            asm volatile("" ::: "memory");
                            pro.publish(scratch, t + 1, tile_p, tile_q, tid);
                        }
                    }
                    fread(lds + ((t + 1) % S) * kStage, Gf);       // (past the end: stale slot, never used)
                    __builtin_amdgcn_sched_barrier(0);
                    mfmas(F);
                }
            }
        }
    }
    // split-K reduction through LDS (fixed order: compute wave 0..3), epilogue on float4s by the
    // 256 compute threads; every wave takes part in the barriers
    PVAE_MARK(0, 2);                                             // main loop done (compute wave 0)
    __syncthreads();
    constexpr int RS = 36;
    if (wave < 4) store_partial_32x32<P_ROW>(lds + wave * (32 * RS), acc, li, lh);
    __syncthreads();
    if (wave < 4) {
        const int ql = tid >> 3, pl = (tid & 7) << 2;
        v4f v = *reinterpret_cast<const v4f*>(lds + ql * RS + pl);
#pragma unroll
        for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const v4f*>(lds + w * (32 * RS) + ql * RS + pl);
        epi(q0 + ql, p0 + pl, v, epre);
    }
    epi.finish(lds, tile_q * tiles_p + tile_p, tid);
    PVAE_MARK(0, 3);                                             // epilogue stores issued
}

// The same kernel on 64 x 32 output tiles (Q tile 64 rows, P tile 32 rows), for 512 rows and more: with 32x32 tiles a
// 512-row layer is 512 workgroups, two per CU, each landing its own 16 KB per k-tile through an LDS-DMA path that
// saturates at ~27 B/clk per CU -- the loop there IS loader-bound (not fetching X at all buys 1 us
// of 13).  One 64x32 workgroup per CU lands 24 KB per k-tile for the MFMA work of two 32x32 tiles (32 KB): a quarter
// less DMA traffic per flop.  Every output element is still the sum of the same four k-quarters in the same order, so
// results equal the 32x32 kernel's bit for bit.  Ring: 4 slots x 24 KB = 96 KB.
constexpr int kWs64Stages = 4;      // ring slots of the 64x32 kernel (24 KB each; 5 and 6 slots measured 2-4 % slower)
// PT = 32: the 64x32 tile above.  PT = 64 (round 4, 1024 rows and more): 64x64 outputs per workgroup, 32 KB per k-tile for
// twice the MFMA work of the 24 KB of 64x32 -- 16 flop per DMA byte instead of 10.7; the k-loop is as long as its DMA stream
// (docs/experiments.md), so that is what pays.  Ring 4 x 32 KB.  Same k-quarters per wave, same order: bit-identical again.
template <int PT> constexpr int ws64_floats() { return (PT == 64 ? 4 : kWs64Stages) * (64 + PT) * 64; }
template <bool P_ROW, class Epi, int PT = 32, class QS = QDense>
__device__ inline void splitk_ws64_body(float* lds, int bid, const GemmArgs& ga, Epi& epi, const QS& qs = QS()) {
    static_assert(PT == 32 || PT == 64, "P tile of 32 or 64 rows");
    constexpr int BK = 64, kTileQ = 64 * 64, kTileP = PT * 64, kStage = kTileQ + kTileP, S = PT == 64 ? 4 : kWs64Stages;
    constexpr int NB = PT / 16;                                  // 16-wide p blocks of the tile = P DMA instructions per loader wave
    constexpr int PER = 4 + NB;                                  // DMA instructions per loader wave and tile
    static_assert(kWsLoaders == 4, "written for four loader waves");
    static_assert(S >= 4 && S <= 6, "the loaders' wait ladder covers up to four tiles in flight");
    const float* __restrict__ Q = ga.Q;
    const float* __restrict__ P = ga.P;
    const int ldq = ga.ldq, ldp = ga.ldp, K = ga.K, tiles_q = ga.tiles_q, tiles_p = ga.tiles_p;
    const int xcd = bid & 7, loc = bid >> 3;
    int tile_p = xcd * ga.p_per_xcd + loc / tiles_q;
    int tile_q = loc % tiles_q;
    if (PT == 64 && ga.rowxcd) {
        // Many row blocks (1024 rows and more): every XCD takes a RANGE OF ROW BLOCKS and walks all column blocks with it,
        // row blocks fastest -- its share of X (rq x 256 KB) stays in its L2 while the W tiles stream through once per
        // XCD.  The column-range mapping above re-reads all of X for every column block an XCD owns: at 4096 rows 256 MB
        // of fabric traffic per layer against 48 MB here.
        const int rq = (tiles_q + 7) >> 3;
        tile_q = xcd * rq + loc % rq;
        tile_p = loc / rq;
        if (tile_q >= tiles_q) return;
    }
    if (tile_p >= tiles_p) return;
    const int q0 = tile_q * 64, p0 = tile_p * PT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lh = lane >> 4;
    const int nk = K / BK;
    typename Epi::Pre epre[NB] = {};
    v4f acc[4][NB];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = v4f{0.f, 0.f, 0.f, 0.f};
    const size_t kstep_p = P_ROW ? (size_t)BK : (size_t)BK * ldp;
    // 16-byte slot j of an operand image -> its global source (same swizzles as splitk_ws_body)
    auto src_q = [&](int j) {
        const int row = j >> 4, c = (j & 15) ^ (row & 15);
        return qs.base(Q, ldq, q0 + row, c * 4);
    };
    auto src_p = [&](int j) {
        if (P_ROW) {
            const int row = j >> 4, c = (j & 15) ^ (row & 15);
            return P + (size_t)(p0 + row) * ldp + c * 4;
        }
        if (PT == 64) return P + (size_t)(j >> 4) * ldp + p0 + (j & 15) * 4;   // [64 k][64 p]: a k-row is all 64 banks, no swizzle
        const int r = j >> 3, k = r ^ ((r >> 2) & 1);
        return P + (size_t)k * ldp + p0 + (j & 7) * 4;
    };
    // dense operands: wave-uniform panel bases + 32-bit lane offsets of the same slots (lds_dma16_sbase)
    constexpr bool kSB = QS::kAlwaysFast && kLoaderScalarBase;
    const char* const qb0 = reinterpret_cast<const char*>(Q + (size_t)q0 * ldq);
    const char* const pb0 = reinterpret_cast<const char*>(P_ROW ? P + (size_t)p0 * ldp : P + p0);
    auto off_rows = [](int j, int ld) {
        const int row = j >> 4, c = (j & 15) ^ (row & 15);
        return ((unsigned)row * (unsigned)ld + c * 4) * 4u;
    };
    auto off_q = [&](int j) { return off_rows(j, ldq); };
    auto off_p = [&](int j) {
        if (P_ROW) return off_rows(j, ldp);
        if (PT == 64) return ((unsigned)(j >> 4) * (unsigned)ldp + (j & 15) * 4) * 4u;
        const int r = j >> 3, k = r ^ ((r >> 2) & 1);
        return ((unsigned)k * (unsigned)ldp + (j & 7) * 4) * 4u;
    };
    // k-tile 0 by all eight waves: Q image = 1024 slots (two per lane and wave), P image = 512 / 1024 (one / two)
    if constexpr (kSB) {
        lds_dma16_sbase(qb0, off_q(wave * 64 + lane), lds + wave * 256);
        lds_dma16_sbase(qb0, off_q((wave + 8) * 64 + lane), lds + (wave + 8) * 256);
        lds_dma16_sbase(pb0, off_p(wave * 64 + lane), lds + kTileQ + wave * 256);
        if (PT == 64) lds_dma16_sbase(pb0, off_p((wave + 8) * 64 + lane), lds + kTileQ + (wave + 8) * 256);
    } else {
    if (QS::kAlwaysFast || qs.fast(0)) {
        lds_dma16(qs.tile_fast(src_q(wave * 64 + lane), 0), lds + wave * 256);
        lds_dma16(qs.tile_fast(src_q((wave + 8) * 64 + lane), 0), lds + (wave + 8) * 256);
    } else {
        lds_dma16(qs.tile(src_q(wave * 64 + lane), 0), lds + wave * 256);
        lds_dma16(qs.tile(src_q((wave + 8) * 64 + lane), 0), lds + (wave + 8) * 256);
    }
    lds_dma16(src_p(wave * 64 + lane), lds + kTileQ + wave * 256);
    if (PT == 64) lds_dma16(src_p((wave + 8) * 64 + lane), lds + kTileQ + (wave + 8) * 256);
    }
    if (wave >= 4) {
        // ---------------- loader waves: 4 Q + NB P instructions per tile ----------------
        const int u0 = wave - 4;
        typename QS::Base sq[4];
        const float* sp[NB];
#pragma unroll
        for (int u = 0; u < 4; ++u) sq[u] = src_q((u0 + 4 * u) * 64 + lane);
#pragma unroll
        for (int u = 0; u < NB; ++u) sp[u] = src_p((u0 + 4 * u) * 64 + lane);
        unsigned vq[4], vp[NB];                                  // (dense: see splitk_ws_body)
#pragma unroll
        for (int u = 0; u < 4; ++u) vq[u] = off_q((u0 + 4 * u) * 64 + lane);
#pragma unroll
        for (int u = 0; u < NB; ++u) vp[u] = off_p((u0 + 4 * u) * 64 + lane);
        DenseWalk walk(qb0, pb0, BK * 4, kstep_p * 4, nk);
        walk.seek(1 < nk ? 1 : 0, 1);
        auto issue = [&](int t) {                                // called for t = 1, 2, 3, ... in order
            if constexpr (kSB) {
                float* slot = lds + walk.slot * kStage;
#pragma unroll
                for (int u = 0; u < 4; ++u) lds_dma16_sbase(walk.q, vq[u], slot + (u0 + 4 * u) * 256);
#pragma unroll
                for (int u = 0; u < NB; ++u) lds_dma16_sbase(walk.p, vp[u], slot + kTileQ + (u0 + 4 * u) * 256);
                walk.template next<S>();
                return;
            }
            float* slot = lds + (t % S) * kStage;
            if (QS::kAlwaysFast || qs.fast(t)) {
#pragma unroll
                for (int u = 0; u < 4; ++u) lds_dma16(qs.tile_fast(sq[u], t), slot + (u0 + 4 * u) * 256);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) lds_dma16(qs.tile(sq[u], t), slot + (u0 + 4 * u) * 256);
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) lds_dma16(sp[u] + (size_t)t * kstep_p, slot + kTileQ + (u0 + 4 * u) * 256);
        };
        if (1 < nk) issue(1);
        if (1 < nk) wait_vmcnt<PER>(); else wait_vmcnt<0>();     // this wave's share of tile 0 landed
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int t = 2; t < S - 1; ++t)
            if (t < nk) issue(t);
        for (int t = 0; t < nk; ++t) {
            int y = nk - 2 - t;                                  // tiles younger than t+1 still in flight
            if (y > S - 3) y = S - 3;
            if (y <= 0) wait_vmcnt<0>();
            else if (y == 1) wait_vmcnt<PER>();
            else if (y == 2) wait_vmcnt<2 * PER>();
            else wait_vmcnt<3 * PER>();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (t + S - 1 < nk) issue(t + S - 1);
        }
    } else {
        // ---------------- compute waves: 64 x PT over this wave's k-quarter ----------------
        int oq[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int row = 16 * a + li;
            oq[a] = row * 64 + (((4 * wave + lh) ^ (row & 15)) << 2);
        }
        const int kq = 16 * wave + 4 * lh;
        wait_vmcnt<0>();                                         // this wave's share of tile 0 landed
#pragma unroll
        for (int h = 0; h < NB; ++h)
            epre[h] = PT == 64 ? epi.preload(q0 + 16 * h + (tid >> 4), p0 + ((tid & 15) << 2))
                               : epi.preload(q0 + 32 * h + (tid >> 3), p0 + ((tid & 7) << 2));
        struct Frag { v4f q[4], p[NB]; v2f c[4]; v4f c4[4]; };   // (P_ROW: p; P_COL: c at PT = 32, c4 at PT = 64)
        auto fread = [&](const float* st, Frag& f) {
#pragma unroll
            for (int a = 0; a < 4; ++a) f.q[a] = *reinterpret_cast<const v4f*>(st + oq[a]);
            if (P_ROW) {
#pragma unroll
                for (int b = 0; b < NB; ++b) f.p[b] = *reinterpret_cast<const v4f*>(st + kTileQ + oq[b]);
            } else if (PT == 64) {
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2) f.c4[s2] = *reinterpret_cast<const v4f*>(st + kTileQ + (kq + s2) * 64 + 4 * li);
            } else {
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2)
                    f.c[s2] = *reinterpret_cast<const v2f*>(st + kTileQ + (((kq + s2) ^ (lh & 1)) * 32) + 2 * li);
            }
        };
        auto mfmas = [&](const Frag& f) {
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const float pv = P_ROW ? f.p[b][s2] : (PT == 64 ? f.c4[s2][b] : f.c[s2][b]);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv, f.q[a][s2], acc[a][b], 0, 0, 0);
                    }
        };
        __builtin_amdgcn_s_barrier();                            // tile 0 landed
        asm volatile("" ::: "memory");
        Frag F0, F1;
        fread(lds, F0);
        for (int t0 = 0; t0 < nk; t0 += 2) {
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const int t = t0 + d;
                if (t < nk) {
                    Frag& F = d ? F1 : F0;
                    Frag& Gf = d ? F0 : F1;
                    __builtin_amdgcn_s_barrier();                // tile t+1 landed; tile t-1's slot is free
                    asm volatile("" ::: "memory");
                    fread(lds + ((t + 1) % S) * kStage, Gf);
                    __builtin_amdgcn_sched_barrier(0);
                    mfmas(F);
                }
            }
        }
    }
    // split-K reduction through LDS (fixed order: compute wave 0..3), epilogue on float4s by the 256 compute threads
    __syncthreads();
    constexpr int RS = PT + 4;
    if (wave < 4) {
        float* red = lds + wave * (64 * RS);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            float* row = red + (16 * a + li) * RS;           // (16-byte writes: see store_partial_32x32)
            if (P_ROW) {
#pragma unroll
                for (int b = 0; b < NB; ++b) *reinterpret_cast<v4f*>(row + 16 * b + 4 * lh) = acc[a][b];
            } else if constexpr (PT == 64) {                 // lane holds p = 16 lh + 4 j + b of row 16 a + li
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    *reinterpret_cast<v4f*>(row + 16 * lh + 4 * j) = v4f{acc[a][0][j], acc[a][1][j], acc[a][2][j], acc[a][3][j]};
            } else {
                *reinterpret_cast<v4f*>(row + 8 * lh) = v4f{acc[a][0][0], acc[a][1][0], acc[a][0][1], acc[a][1][1]};
                *reinterpret_cast<v4f*>(row + 8 * lh + 4) = v4f{acc[a][0][2], acc[a][1][2], acc[a][0][3], acc[a][1][3]};
            }
        }
    }
    __syncthreads();
    if (wave < 4) {
#pragma unroll
        for (int h = 0; h < NB; ++h) {
            const int ql = PT == 64 ? 16 * h + (tid >> 4) : 32 * h + (tid >> 3);
            const int pl = PT == 64 ? (tid & 15) << 2 : (tid & 7) << 2;
            v4f v = *reinterpret_cast<const v4f*>(lds + ql * RS + pl);
#pragma unroll
            for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const v4f*>(lds + w * (64 * RS) + ql * RS + pl);
            epi(q0 + ql, p0 + pl, v, epre[h]);
        }
    }
    epi.finish(lds, tile_q * tiles_p + tile_p, tid);
}

template <bool P_ROW, class Epi, int PT = 32>
__global__ void __launch_bounds__(512)
gemm_splitk_ws64_kernel(PVAE_GA_PARAMS(a_), Epi epi) {
    const GemmArgs ga = PVAE_GA_OF(a_);
    __shared__ __attribute__((aligned(16))) float lds[ws64_floats<PT>()];
    splitk_ws64_body<P_ROW, Epi, PT>(lds, blockIdx.x, ga, epi);
}

template <bool P_ROW, class Epi>
__global__ void __launch_bounds__(kWsThreads)
gemm_splitk_ws_kernel(PVAE_GA_PARAMS(a_), Epi epi) {
    const GemmArgs ga = PVAE_GA_OF(a_);
    __shared__ __attribute__((aligned(16))) float lds[6 * 2 * 32 * 64];
    splitk_ws_body<P_ROW, Epi>(lds, blockIdx.x, ga, epi);
}
template <class Epi, class Pro>
__global__ void __launch_bounds__(kWsThreads)
gemm_splitk_ws_pro_kernel(PVAE_GA_PARAMS(a_), Epi epi, Pro pro) {
    const GemmArgs ga = PVAE_GA_OF(a_);
    __shared__ __attribute__((aligned(16))) float lds[kWsFloats];
    __shared__ __attribute__((aligned(16))) float scratch[Pro::kScratchFloats];
    splitk_ws_body<true, Epi, Pro>(lds, blockIdx.x, ga, epi, pro, scratch);
}
// the first layer of a stack on the gathered operand (XSrc): 32x32 tiles, plain or with a Pro patch; 64 x PT tiles
template <class Epi>
__global__ void __launch_bounds__(kWsThreads)
gemm_splitk_ws_gather_kernel(PVAE_GG_PARAMS, Epi epi, XSrc xs) {
    const GemmArgs ga = PVAE_GG_GA;
    __shared__ __attribute__((aligned(16))) float lds[6 * 2 * 32 * 64];
    splitk_ws_body<true, Epi, NoPro, QGather>(lds, blockIdx.x, ga, epi, NoPro(), nullptr, PVAE_GG_QS(xs));
}
template <class Epi, class Pro>
__global__ void __launch_bounds__(kWsThreads)
gemm_splitk_ws_pro_gather_kernel(PVAE_GG_PARAMS, Epi epi, Pro pro, XSrc xs) {
    const GemmArgs ga = PVAE_GG_GA;
    __shared__ __attribute__((aligned(16))) float lds[kWsFloats];
    __shared__ __attribute__((aligned(16))) float scratch[Pro::kScratchFloats];
    splitk_ws_body<true, Epi, Pro, QGather>(lds, blockIdx.x, ga, epi, pro, scratch, PVAE_GG_QS(xs));
}
template <class Epi, int PT>
__global__ void __launch_bounds__(512)
gemm_splitk_ws64_gather_kernel(PVAE_GG_PARAMS, Epi epi, XSrc xs) {
    const GemmArgs ga = PVAE_GG_GA;
    __shared__ __attribute__((aligned(16))) float lds[ws64_floats<PT>()];
    splitk_ws64_body<true, Epi, PT, QGather>(lds, blockIdx.x, ga, epi, PVAE_GG_QS(xs));
}
}  // namespace pvae
