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
// patched tile) keeps one barrier per tile on four slots.  One body per schedule: splitk_ws_superstep_body (the plain kernels,
// dense or gathered) and splitk_ws_pertile_body (the Pro kernels); splitk_ws64_body is the per-tile schedule on 64-row tiles.
// The bodies keep statement order and some shapes (a tail written out twice, a `return` in front of dead code) because hipcc's
// schedule follows them: tools/isa_diff.py against the parent commit is the check for any edit that means to change nothing.
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

// ---- pieces the bodies below share ---------------------------------------------------------------------------------
constexpr int kWsTile = 32 * 64;                         // floats of one operand image of a 32x32 stage (32 rows x BK)
// Workgroup -> output tile: XCD x (bid & 7) owns a range of p_per_xcd column blocks and walks the row blocks fastest.
struct WsTileMap {
    int xcd, loc, tile_q, tile_p;
    __device__ inline WsTileMap(int bid, const GemmArgs& ga) : xcd(bid & 7), loc(bid >> 3) {
        tile_p = xcd * ga.p_per_xcd + loc / ga.tiles_q;
        tile_q = loc % ga.tiles_q;
    }
};
// 16-byte slot j of an operand's tile image in LDS -> where it comes from: the lane's 32-bit byte offset from the tile's
// base (dense operands, lds_dma16_sbase) or its pointer (gathered operands, lds_dma16).  The XOR swizzle of the image stays
// on the source side.  Q and a P_ROW P are [row][64 k] images; a P_COL P is [64 k][PT p] -- at PT = 32 two k-rows share a
// bank line and the k-swizzle separates them, at PT = 64 a k-row is all 64 banks and needs none.
template <bool P_ROW, int PT = 32>
struct WsSlot {
    __device__ static inline unsigned off_rows(int j, int ld) {
        const int row = j >> 4, c = (j & 15) ^ (row & 15);
        return ((unsigned)row * (unsigned)ld + c * 4) * 4u;
    }
    __device__ static inline unsigned off_q(int j, int ldq) { return off_rows(j, ldq); }
    __device__ static inline unsigned off_p(int j, int ldp) {
        if (P_ROW) return off_rows(j, ldp);
        if (PT == 64) return ((unsigned)(j >> 4) * (unsigned)ldp + (j & 15) * 4) * 4u;
        const int r = j >> 3, k = r ^ ((r >> 2) & 1);
        return ((unsigned)k * (unsigned)ldp + (j & 7) * 4) * 4u;
    }
    template <class QS>
    __device__ static inline typename QS::Base src_q(const QS& qs, const float* Q, int ldq, int q0, int j) {
        const int row = j >> 4, c = (j & 15) ^ (row & 15);
        return qs.base(Q, ldq, q0 + row, c * 4);
    }
    __device__ static inline const float* src_p(const float* P, int ldp, int p0, int j) {
        if (P_ROW) {
            const int row = j >> 4, c = (j & 15) ^ (row & 15);
            return P + (size_t)(p0 + row) * ldp + c * 4;
        }
        if (PT == 64) return P + (size_t)(j >> 4) * ldp + p0 + (j & 15) * 4;
        const int r = j >> 3, k = r ^ ((r >> 2) & 1);
        return P + (size_t)k * ldp + p0 + (j & 7) * 4;
    }
};
// k-tile 0 is fetched by ALL eight waves, a wave's eighth of it (one 16-byte slot per lane of each operand image) each: it
// is in flight ~0.1 us after the workgroup starts instead of queueing behind the loaders' prologue (each global_load_lds
// holds its wave ~150 cycles, so a three-tile prologue alone took 0.67 us -- tools/timeline_probe.hip).  Dense operands:
// two lds_dma16_sbase where the bodies stand (a helper's argument evaluation moved the probe build's selects); gathered
// operands: this, k-tile kt by the lane's pointers.
template <bool P_ROW, class QS>
__device__ inline void ws_fetch_eighth_gather(float* stage, int wave, int lane, const QS& qs, const float* Q, int ldq, int q0,
                                              const float* P, int ldp, int p0, int kt, size_t kstep_p) {
    const int j = wave * 64 + lane;                       // 16-byte slot inside the 8 KB tile image
    const typename QS::Base s0q = WsSlot<P_ROW>::src_q(qs, Q, ldq, q0, j);
    const float* const s0p = WsSlot<P_ROW>::src_p(P, ldp, p0, j);
    if (qs.fast(kt)) lds_dma16(qs.tile_fast(s0q, kt), stage + wave * 256);
    else lds_dma16(qs.tile(s0q, kt), stage + wave * 256);
    lds_dma16(s0p + (size_t)kt * kstep_p, stage + kWsTile + wave * 256);
}
// A compute wave's fragments of one k-tile of a 32x32 stage (its k-quarter: 16 k of 64), their kReads ds_reads and the 16
// MFMAs on them.  MFMA i of a tile: s2 = i / 4, a = (i / 2) & 1, b = i & 1 -- every accumulator sees the same sequence
// however a body cuts the range.  (The lane's offsets travel by reference, as the lambdas these helpers were captured them:
// by value hipcc schedules the P_COL instances differently.)
template <bool P_ROW>
struct WsFrag {
    static constexpr int kReads = P_ROW ? 4 : 6;          // ds_read instructions per fragment set
    v4f q[2], p[2];
    v2f c[4];                                             // (P_ROW: p; P_COL: c)
    __device__ inline void read_one(const float* st, const int (&oq)[2], const int& kq, const int& li, const int& lh, int r) {
        if (r < 2) q[r] = *reinterpret_cast<const v4f*>(st + oq[r]);
        else if (P_ROW) p[r - 2] = *reinterpret_cast<const v4f*>(st + kWsTile + oq[r - 2]);
        else c[r - 2] = *reinterpret_cast<const v2f*>(st + kWsTile + (((kq + r - 2) ^ (lh & 1)) * 32) + 2 * li);
    }
    __device__ inline void read(const float* st, const int (&oq)[2], const int& kq, const int& li, const int& lh) {
#pragma unroll
        for (int r = 0; r < kReads; ++r) read_one(st, oq, kq, li, lh, r);
    }
    __device__ inline void mfma_range(v4f (&acc)[2][2], int lo, int hi) const {
#pragma unroll
        for (int i = lo; i < hi; ++i) {
            const int s2 = i >> 2, a = (i >> 1) & 1, b = i & 1;
            const float pv = P_ROW ? p[b][s2] : c[s2][b];
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv, q[a][s2], acc[a][b], 0, 0, 0);
        }
    }
};

// ---- 32x32, super-steps: SIX slots, two k-tiles per workgroup barrier (the plain kernels, dense or gathered) ---------
template <bool P_ROW, class Epi, class QS = QDense>
__device__ inline void splitk_ws_superstep_body(float* lds, int bid, const GemmArgs& ga, Epi& epi, const QS& qs = QS()) {
    constexpr int BK = 64, kTile = kWsTile, kStage = 2 * kTile, S = 6;
    constexpr bool kDense = QS::kAlwaysFast;              // (the gathered first layers: per-lane pointers, their own loop)
    using Slot = WsSlot<P_ROW>;
    using Frag = WsFrag<P_ROW>;
    const float* __restrict__ Q = ga.Q;
    const float* __restrict__ P = ga.P;
    const int ldq = ga.ldq, ldp = ga.ldp, K = ga.K, tiles_q = ga.tiles_q, tiles_p = ga.tiles_p;
    const WsTileMap tm(bid, ga);
    const int xcd = tm.xcd, loc = tm.loc;
    int tile_p = tm.tile_p, tile_q = tm.tile_q;
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
    // -- see lds_dma16_sbase.  (Unused by the gathered instances, which keep per-lane pointers.)
    const char* const qb0 = reinterpret_cast<const char*>(Q + (size_t)q0 * ldq);
    const char* const pb0 = reinterpret_cast<const char*>(P_ROW ? P + (size_t)p0 * ldp : P + p0);
    DenseWalk walk(qb0, pb0, BK * 4, kstep_p * 4, nk);
    unsigned vq[kWsPer], vp[kWsPer];                      // dense loaders: lane offsets of this wave's pieces of a tile
    if constexpr (kDense) {
        // The wide prologue.  k-tile 0 is fetched by all eight waves (see ws_fetch_eighth_gather), and so are k-tiles 1 and 2 -- six DMAs
        // per wave through the two lane offsets of tile 0, ring slot and k-tile advanced by the loaders' walk (SGPRs).  All
        // three are requested before anything is waited for: the first super-step's barrier certifies tiles 1 and 2, and behind
        // a loaders-only prologue tile 2 was requested only after tile 0 had landed (two memory round trips in a row in front of
        // the first MFMA).  Slots 1-4 have never been read at this point, so the restaging rule of the super-step barrier (see
        // the compute waves) is not involved.
        const int j = wave * 64 + lane;                   // 16-byte slot inside the 8 KB tile image
        const unsigned vq0 = Slot::off_q(j, ldq), vp0 = Slot::off_p(j, ldp);
        // A loader wave's second piece of a tile is its eighth of it; the offsets of its first piece are computed HERE, in
        // front of the DMAs: behind them hipcc puts an s_waitcnt vmcnt(0) in front of the loader path's first vector-ALU
        // instruction (it merges the compute path's pending epilogue preload into that block), and the loaders then request
        // nothing more until everything above has landed.
        static_assert(kWsLoaders == 4 && kWsPer == 2, "loader wave w takes pieces w - 4 and w");
        if (wave >= 4) {
            vq[0] = Slot::off_q(j - 256, ldq), vp[0] = Slot::off_p(j - 256, ldp);
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
    } else if (wave < 8) {                                // (always true; see splitk_ws_pertile_body)
        ws_fetch_eighth_gather<P_ROW>(lds, wave, lane, qs, Q, ldq, q0, P, ldp, p0, rot, kstep_p);
    }
    if (wave >= 4) {
        // ---------------- loader waves ----------------  (s_setprio 1 here, or on the compute waves: +-0)
        const int u0 = wave - 4;
        typename QS::Base sq[kWsPer];                     // gathered operands: the lane's pointers of this wave's pieces
        const float* sp[kWsPer];
        if constexpr (!kDense) {
#pragma unroll
            for (int u = 0; u < kWsPer; ++u) {
                sq[u] = Slot::src_q(qs, Q, ldq, q0, (u0 + kWsLoaders * u) * 64 + lane);
                sp[u] = Slot::src_p(P, ldp, p0, (u0 + kWsLoaders * u) * 64 + lane);
            }
        }
        // dense operands: lane offsets (distinct VGPRs) and tile walk (SGPRs) stand as the wide prologue left them; issue() is
        // called for t = 3, 4, 5, ... in order, so the walk only ever steps to the next tile
        auto issue = [&](int t) {
            if constexpr (kDense) {
                if (PVAE_PROBE(6)) return;                // probe: loaders only keep the barriers
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
            }   // (no `else`: see splitk_ws64_body)
            float* slot = lds + (t % S) * kStage;
            int kt = t + rot;                             // k-tile this workgroup reads at step t
            if (kt >= nk) kt -= nk;
            if (qs.fast(kt)) {
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
        if constexpr (kDense) {
            // tile 3 rides on tile 0's flight time, tile 4 follows behind barrier #0 (with both in front barrier #0 moves
            // 0.2 us later and the step gains nothing; profiles/r09_ab_prologue.txt).  This wave's share of tile 0 (its oldest
            // two DMAs) has landed once only its shares of tiles 1, 2 (two each) and its pieces of tile 3 (2 * kWsPer) are in
            // flight.
            static_assert(kWsPer == 2, "the counted waits of the prologue");
            if (3 < nk) issue(3);
            PVAE_MARK(256, 4);
            if (3 < nk) wait_vmcnt<8>();
            else if (2 < nk) wait_vmcnt<4>();
            else if (nk == 2) wait_vmcnt<2>();
            else wait_vmcnt<0>();
        } else {
            if (1 < nk) issue(1);                                    // rides on tile 0's flight time
            if (1 < nk) wait_vmcnt<2 * kWsPer>(); else wait_vmcnt<0>();   // this wave's share of tile 0 landed
        }
        PVAE_MARK(256, 5);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // super-steps of TWO k-tiles per workgroup barrier.  At the barrier in front of tiles (t0, t0+1): t0+1 and t0+2
        // have landed, t0+3 and t0+4 are in flight; the slots of t0-1 and t0 (whose fragment reads the compute waves
        // have retired, see there) take t0+5 and t0+6.
        // (Wide prologue: tiles 1 and 2 came from all eight waves -- this wave's shares are older than its tiles 3 and
        // 4, so the same ladder certifies them at t0 = 0, and the compute waves wait for theirs in front of their loop.)
        if constexpr (!kDense) {
            if (2 < nk) issue(2);
            if (3 < nk) issue(3);
        }
        if (4 < nk) issue(4);
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
        // ---------------- compute waves ----------------
        int oq[2];                                                 // where this lane's fragments lie inside a stage
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
        if constexpr (kDense) epre = epi.preload(q0 + (tid >> 3), p0 + ((tid & 7) << 2));
        if (kDense && 2 < nk) wait_vmcnt<4>();
        else if (kDense && 1 < nk) wait_vmcnt<2>();
        else wait_vmcnt<0>();
        if constexpr (!kDense) epre = epi.preload(q0 + (tid >> 3), p0 + ((tid & 7) << 2));   // epilogue operands: arrive under the loop
        // (the body's handles on the fragment helpers; mfmas() carries the probe's switch)
        auto fread = [&](const float* st, Frag& f) { f.read(st, oq, kq, li, lh); };
        auto fread_one = [&](const float* st, Frag& f, int r) { f.read_one(st, oq, kq, li, lh, r); };
        auto mfma_range = [&](const Frag& f, int lo, int hi) { f.mfma_range(acc, lo, hi); };
        auto mfmas = [&](const Frag& f) {
            if (PVAE_PROBE(4)) {                          // probe: no MFMAs (fragments stay live)
                asm volatile("" ::"v"(f.q[0]), "v"(f.q[1]), "v"(f.p[0]), "v"(f.p[1]));
                return;
            }
            // (Frag::mfmas written out: only so does the timeline build keep its branch on the switch as it was emitted)
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
        // The half-step of the dense loop: the 16 MFMAs of the tile in registers with the NEXT tile's fragment reads between
        // them, one read behind every second MFMA.  All four compute waves leave a barrier together; with the reads in
        // front, their 16 KB queue on the one LDS port while the in-order wave cannot issue an MFMA until its last read
        // has issued, and the matrix pipe drains twice per super-step.  Opened with MFMAs, the pipe is busy from the
        // barrier on and the reads return under it.
        constexpr int kGap = 2;                                    // MFMAs per read (1 and 3 measured the same)
        auto half_step = [&](const Frag& cur, Frag& nxt, const float* st) {
            if (PVAE_PROBE(4)) {                          // probe: no MFMAs (one branch per half-step, as mfmas() has)
                fread(st, nxt);
                mfmas(cur);
                return;
            }
#pragma unroll
            for (int r = 0; r < Frag::kReads; ++r) {
                mfma_range(cur, kGap * r, kGap * r + kGap);
                __builtin_amdgcn_sched_barrier(0);
                fread_one(st, nxt, r);
                __builtin_amdgcn_sched_barrier(0);
            }
            mfma_range(cur, kGap * Frag::kReads, 16);
        };
        __builtin_amdgcn_s_barrier();                              // tile 0 landed
        asm volatile("" ::: "memory");
#ifdef PVAE_TIMELINE
        // (dense: mark 1 is taken here and stored with mark 6 -- a store counts on vmcnt, and the wide prologue's vmcnt(0) in
        // front of the loop would wait ~80 ns for it)
        const unsigned long long t_seen = wall_clock64();
        if (!kDense && tid == 0) g_timeline[(size_t)blockIdx.x * 8 + 1] = t_seen;
#endif
        Frag F0, F1;
        fread(lds, F0);
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
        if constexpr (kDense) {
            // wide prologue: this wave's shares of tiles 1 and 2 landed -- certified by the first super-step's barrier, which
            // waits for the loaders' shares of the same tiles anyway; nothing is added inside the loop
            wait_vmcnt<0>();
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
            // (gathered first layers: each tile's fragment reads in front of the previous tile's MFMAs)
            for (int t0 = 0; t0 < nk; t0 += 2) {
                superstep_barrier();
                fread(lds + ((t0 + 1) % S) * kStage, F1);        // (past the end: stale slot, never used)
                __builtin_amdgcn_sched_barrier(0);
                mfmas(F0);
                if (t0 + 1 < nk) {
                    fread(lds + ((t0 + 2) % S) * kStage, F0);
                    __builtin_amdgcn_sched_barrier(0);
                    mfmas(F1);
                }
            }
        }
    }
    PVAE_MARK(0, 2);                                             // main loop done (compute wave 0)
    // split-K reduction through LDS (fixed order: compute wave 0..3), epilogue on float4s by the
    // 256 compute threads; every wave takes part in the barriers
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

// ---- 32x32, one barrier per tile: FOUR slots, with a Pro patch (a patch needs its own barrier per patched tile) ------
// P is always ROW here (forward layers).  No probe hooks: no tool launches these kernels.
template <class Epi, class Pro, class QS = QDense>
__device__ inline void splitk_ws_pertile_body(float* lds, float* scratch, int bid, const GemmArgs& ga, Epi& epi, const Pro& pro,
                                              const QS& qs = QS()) {
    constexpr int BK = 64, kTile = kWsTile, kStage = 2 * kTile, S = kWsStages;
    constexpr bool kDense = QS::kAlwaysFast;
    using Slot = WsSlot<true>;
    using Frag = WsFrag<true>;
    const float* __restrict__ Q = ga.Q;
    const float* __restrict__ P = ga.P;
    const int ldq = ga.ldq, ldp = ga.ldp, K = ga.K, tiles_q = ga.tiles_q, tiles_p = ga.tiles_p;
    const WsTileMap tm(bid, ga);
    const int xcd = tm.xcd, loc = tm.loc;
    int tile_p = tm.tile_p, tile_q = tm.tile_q;
    if (ga.rowxcd && tiles_q == 8 && tiles_p == 8 * ga.p_per_xcd) { tile_q = xcd; tile_p = loc; }
    if (tile_p >= tiles_p) return;
    const int q0 = tile_q * 32, p0 = tile_p * 32;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lh = lane >> 4;
    const int nk = K / BK;
    typename Epi::Pre epre{};
    v4f acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = v4f{0.f, 0.f, 0.f, 0.f};

    const size_t kstep_p = BK;
    const int rot = k_rotation(ga, loc, tile_q, nk);
    const char* const qb0 = reinterpret_cast<const char*>(Q + (size_t)q0 * ldq);      // (dense: see lds_dma16_sbase)
    const char* const pb0 = reinterpret_cast<const char*>(P + (size_t)p0 * ldp);
    // k-tile 0 by all eight waves.  (`wave < 8` is always true in a 512-thread launch, but hipcc does not know it and
    // branches on it; the test stays so that these kernels' code stays what it was.)
    if constexpr (kDense) {
        if (wave < 8) {
            const int j = wave * 64 + lane;               // 16-byte slot inside the 8 KB tile image
            lds_dma16_sbase(qb0 + (size_t)rot * (BK * 4), Slot::off_q(j, ldq), lds + wave * 256);
            lds_dma16_sbase(pb0 + (size_t)rot * kstep_p * 4, Slot::off_p(j, ldp), lds + kTile + wave * 256);
        }
    } else if (wave < 8) {
        ws_fetch_eighth_gather<true>(lds, wave, lane, qs, Q, ldq, q0, P, ldp, p0, rot, kstep_p);
    }
    if (wave >= 4) {
        // ---------------- loader waves ----------------
        const int u0 = wave - 4;
        // the lane's sources of this wave's pieces: 32-bit offsets and the tile walk in SGPRs (dense) or pointers (gathered)
        unsigned vq[kWsPer], vp[kWsPer];
        typename QS::Base sq[kWsPer];
        const float* sp[kWsPer];
        DenseWalk walk(qb0, pb0, BK * 4, kstep_p * 4, nk);
#pragma unroll
        for (int u = 0; u < kWsPer; ++u) {
            const int j = (u0 + kWsLoaders * u) * 64 + lane;       // 16-byte slot inside the 8 KB tile image
            if constexpr (kDense) {
                vq[u] = Slot::off_q(j, ldq);
                vp[u] = Slot::off_p(j, ldp);
            } else {
                sq[u] = Slot::src_q(qs, Q, ldq, q0, j);
                sp[u] = Slot::src_p(P, ldp, p0, j);
            }
        }
        if constexpr (kDense) walk.seek(rot + 1 < nk ? rot + 1 : 0, 1);
        auto issue = [&](int t) {                         // called for t = 1, 2, 3, ... in order: the walk only steps to the next tile
            if constexpr (kDense) {
                float* slot = lds + walk.slot * kStage;
#pragma unroll
                for (int u = 0; u < kWsPer; ++u) {
                    lds_dma16_sbase(walk.q, vq[u], slot + (u0 + kWsLoaders * u) * 256);
                    lds_dma16_sbase(walk.p, vp[u], slot + kTile + (u0 + kWsLoaders * u) * 256);
                }
                walk.template next<S>();
                return;
            }   // (no `else`: see splitk_ws64_body)
            float* slot = lds + (t % S) * kStage;
            int kt = t + rot;                             // k-tile this workgroup reads at step t
            if (kt >= nk) kt -= nk;
            if (qs.fast(kt)) {
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
        if (1 < nk) issue(1);                                    // rides on tile 0's flight time
        if (1 < nk) wait_vmcnt<2 * kWsPer>(); else wait_vmcnt<0>();   // this wave's share of tile 0 landed
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (pro.needs(0)) __builtin_amdgcn_s_barrier();        // (the compute waves patch tile 0 in between)
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
            if (t + 1 < nk && pro.needs(t + 1)) __builtin_amdgcn_s_barrier();
            if (t + S - 1 < nk) issue(t + S - 1);                  // refill the slot tile t-1 vacated
        }
    } else {
        // ---------------- compute waves ----------------
        int oq[2];                                                 // where this lane's fragments lie inside a stage
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int row = 16 * a + li;
            oq[a] = row * 64 + (((4 * wave + lh) ^ (row & 15)) << 2);
        }
        const int kq = 16 * wave + 4 * lh;
        wait_vmcnt<0>();                                           // this wave's share of tile 0 landed
        epre = epi.preload(q0 + (tid >> 3), p0 + ((tid & 7) << 2));   // epilogue operands: arrive under the loop
        typename Pro::State pst = pro.prepare(q0, tid);
        __builtin_amdgcn_s_barrier();                              // tile 0 landed
        asm volatile("" ::: "memory");
        if (pro.needs(0)) {
            pro.patch(lds, scratch, pst, 0, q0, tile_p, tile_q, tid);
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            pro.publish(scratch, 0, tile_p, tile_q, tid);
        }
        Frag F0, F1;
        F0.read(lds, oq, kq, li, lh);
        for (int t0 = 0; t0 < nk; t0 += 2) {
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const int t = t0 + d;
                if (t < nk) {
                    Frag& F = d ? F1 : F0;
                    Frag& Gf = d ? F0 : F1;
                    __builtin_amdgcn_s_barrier();                  // tile t+1 landed; tile t-1's slot is free
                    asm volatile("" ::: "memory");
                    if (t + 1 < nk && pro.needs(t + 1)) {
                        pro.patch(lds + ((t + 1) % S) * kStage, scratch, pst, t + 1, q0, tile_p, tile_q, tid);
                        __builtin_amdgcn_s_barrier();
                        asm volatile("" ::: "memory");
                        pro.publish(scratch, t + 1, tile_p, tile_q, tid);
                    }
                    Gf.read(lds + ((t + 1) % S) * kStage, oq, kq, li, lh);     // (past the end: stale slot, never used)
                    __builtin_amdgcn_sched_barrier(0);
                    F.mfma_range(acc, 0, 16);
                }
            }
        }
    }
    // split-K reduction through LDS (fixed order: compute wave 0..3), epilogue on float4s by the
    // 256 compute threads; every wave takes part in the barriers
    __syncthreads();
    constexpr int RS = 36;
    if (wave < 4) store_partial_32x32<true>(lds + wave * (32 * RS), acc, li, lh);
    __syncthreads();
    if (wave < 4) {
        const int ql = tid >> 3, pl = (tid & 7) << 2;
        v4f v = *reinterpret_cast<const v4f*>(lds + ql * RS + pl);
#pragma unroll
        for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const v4f*>(lds + w * (32 * RS) + ql * RS + pl);
        epi(q0 + ql, p0 + pl, v, epre);
    }
    epi.finish(lds, tile_q * tiles_p + tile_p, tid);
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
    const WsTileMap tm(bid, ga);
    const int xcd = tm.xcd, loc = tm.loc;
    int tile_p = tm.tile_p, tile_q = tm.tile_q;
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
    constexpr bool kDense = QS::kAlwaysFast;
    using Slot = WsSlot<P_ROW, PT>;
    // dense operands: wave-uniform panel bases + 32-bit lane offsets (lds_dma16_sbase); gathered: per-lane pointers
    const char* const qb0 = reinterpret_cast<const char*>(Q + (size_t)q0 * ldq);
    const char* const pb0 = reinterpret_cast<const char*>(P_ROW ? P + (size_t)p0 * ldp : P + p0);
    // k-tile 0 by all eight waves: Q image = 1024 slots (two per lane and wave), P image = 512 / 1024 (one / two)
    if constexpr (kDense) {
        lds_dma16_sbase(qb0, Slot::off_q(wave * 64 + lane, ldq), lds + wave * 256);
        lds_dma16_sbase(qb0, Slot::off_q((wave + 8) * 64 + lane, ldq), lds + (wave + 8) * 256);
        lds_dma16_sbase(pb0, Slot::off_p(wave * 64 + lane, ldp), lds + kTileQ + wave * 256);
        if (PT == 64) lds_dma16_sbase(pb0, Slot::off_p((wave + 8) * 64 + lane, ldp), lds + kTileQ + (wave + 8) * 256);
    } else {
        if (qs.fast(0)) {
            lds_dma16(qs.tile_fast(Slot::src_q(qs, Q, ldq, q0, wave * 64 + lane), 0), lds + wave * 256);
            lds_dma16(qs.tile_fast(Slot::src_q(qs, Q, ldq, q0, (wave + 8) * 64 + lane), 0), lds + (wave + 8) * 256);
        } else {
            lds_dma16(qs.tile(Slot::src_q(qs, Q, ldq, q0, wave * 64 + lane), 0), lds + wave * 256);
            lds_dma16(qs.tile(Slot::src_q(qs, Q, ldq, q0, (wave + 8) * 64 + lane), 0), lds + (wave + 8) * 256);
        }
        lds_dma16(Slot::src_p(P, ldp, p0, wave * 64 + lane), lds + kTileQ + wave * 256);
        if (PT == 64) lds_dma16(Slot::src_p(P, ldp, p0, (wave + 8) * 64 + lane), lds + kTileQ + (wave + 8) * 256);
    }
    if (wave >= 4) {
        // ---------------- loader waves: 4 Q + NB P instructions per tile ----------------
        const int u0 = wave - 4;
        // the lane's sources of this wave's pieces: 32-bit offsets (dense) or pointers (gathered) -- only one set is formed
        unsigned vq[4], vp[NB];
        typename QS::Base sq[4];
        const float* sp[NB];
        if constexpr (kDense) {
#pragma unroll
            for (int u = 0; u < 4; ++u) vq[u] = Slot::off_q((u0 + 4 * u) * 64 + lane, ldq);
#pragma unroll
            for (int u = 0; u < NB; ++u) vp[u] = Slot::off_p((u0 + 4 * u) * 64 + lane, ldp);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) sq[u] = Slot::src_q(qs, Q, ldq, q0, (u0 + 4 * u) * 64 + lane);
#pragma unroll
            for (int u = 0; u < NB; ++u) sp[u] = Slot::src_p(P, ldp, p0, (u0 + 4 * u) * 64 + lane);
        }
        DenseWalk walk(qb0, pb0, BK * 4, kstep_p * 4, nk);       // (dense: the k-tile walk in SGPRs, see DenseWalk)
        walk.seek(1 < nk ? 1 : 0, 1);
        auto issue = [&](int t) {                                // called for t = 1, 2, 3, ... in order
            if constexpr (kDense) {
                float* slot = lds + walk.slot * kStage;
#pragma unroll
                for (int u = 0; u < 4; ++u) lds_dma16_sbase(walk.q, vq[u], slot + (u0 + 4 * u) * 256);
#pragma unroll
                for (int u = 0; u < NB; ++u) lds_dma16_sbase(walk.p, vp[u], slot + kTileQ + (u0 + 4 * u) * 256);
                walk.template next<S>();
                return;
            }   // (no `else`: with the gathered form discarded from the dense instances hipcc schedules the P_COL ones differently)
            float* slot = lds + (t % S) * kStage;
            if (qs.fast(t)) {
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
    splitk_ws_superstep_body<P_ROW, Epi>(lds, blockIdx.x, ga, epi);
}
template <class Epi, class Pro>
__global__ void __launch_bounds__(kWsThreads)
gemm_splitk_ws_pro_kernel(PVAE_GA_PARAMS(a_), Epi epi, Pro pro) {
    const GemmArgs ga = PVAE_GA_OF(a_);
    __shared__ __attribute__((aligned(16))) float lds[kWsFloats];
    __shared__ __attribute__((aligned(16))) float scratch[Pro::kScratchFloats];
    splitk_ws_pertile_body(lds, scratch, blockIdx.x, ga, epi, pro);
}
// the first layer of a stack on the gathered operand (XSrc): 32x32 tiles, plain or with a Pro patch; 64 x PT tiles
template <class Epi>
__global__ void __launch_bounds__(kWsThreads)
gemm_splitk_ws_gather_kernel(PVAE_GG_PARAMS, Epi epi, XSrc xs) {
    const GemmArgs ga = PVAE_GG_GA;
    __shared__ __attribute__((aligned(16))) float lds[6 * 2 * 32 * 64];
    splitk_ws_superstep_body<true, Epi, QGather>(lds, blockIdx.x, ga, epi, PVAE_GG_QS(xs));
}
template <class Epi, class Pro>
__global__ void __launch_bounds__(kWsThreads)
gemm_splitk_ws_pro_gather_kernel(PVAE_GG_PARAMS, Epi epi, Pro pro, XSrc xs) {
    const GemmArgs ga = PVAE_GG_GA;
    __shared__ __attribute__((aligned(16))) float lds[kWsFloats];
    __shared__ __attribute__((aligned(16))) float scratch[Pro::kScratchFloats];
    splitk_ws_pertile_body(lds, scratch, blockIdx.x, ga, epi, pro, PVAE_GG_QS(xs));
}
template <class Epi, int PT>
__global__ void __launch_bounds__(512)
gemm_splitk_ws64_gather_kernel(PVAE_GG_PARAMS, Epi epi, XSrc xs) {
    const GemmArgs ga = PVAE_GG_GA;
    __shared__ __attribute__((aligned(16))) float lds[ws64_floats<PT>()];
    splitk_ws64_body<true, Epi, PT, QGather>(lds, blockIdx.x, ga, epi, PVAE_GG_QS(xs));
}
}  // namespace pvae
