// pvae_gemm_common.h -- shared by every contraction header: vector types, the streamed store, the timeline-probe macros,
// GemmArgs and its kernel-argument packing, the k-rotation experiment.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdlib>
#include <cstring>
#include <type_traits>

// Timeline probe (tools/timeline_probe.hip defines PVAE_TIMELINE): thread `tid_` of each workgroup
// stores the 100 MHz wall clock at numbered points of the wave-specialised kernel, and GemmArgs::krot
// values >= 2 switch parts of it off (ablation).  Compiled out of the library.
#ifdef PVAE_TIMELINE
extern __device__ unsigned long long* g_timeline;
#define PVAE_MARK(tid_, id_)                                                                   \
    do {                                                                                       \
        if ((int)threadIdx.x == (tid_)) g_timeline[(size_t)blockIdx.x * 8 + (id_)] = wall_clock64(); \
    } while (0)
#define PVAE_PROBE(mode_) (ga.krot == (mode_))
// slot 6: HW_ID (bits 8..11 CU, 12..13 SH, 13..15 SE on gfx9), slot 7: XCC_ID
#define PVAE_MARK_HW()                                                                         \
    do {                                                                                       \
        if (threadIdx.x == 0) {                                                                \
            g_timeline[(size_t)blockIdx.x * 8 + 6] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)); \
            g_timeline[(size_t)blockIdx.x * 8 + 7] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)); \
        }                                                                                      \
    } while (0)
#else
#define PVAE_MARK_HW() do { } while (0)
#define PVAE_MARK(tid_, id_) do { } while (0)
#define PVAE_PROBE(mode_) false
#endif

namespace pvae {
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

// Streamed 16-byte store.  Everything these kernels write (activations, input gradients, weight
// gradients, Adam's p / m / v) is consumed by a LATER launch, on other CUs and mostly other XCDs, so
// keeping the lines dirty in the writer's L2 buys nothing: they are written back when the kernel ends,
// and the next launch waits for that (MI355X_MICROARCH.md, `boundary` row: + dirty bytes / 6 TB/s, i.e.
// ~2.8 us behind the 17 MB a fused backward launch leaves behind).  `sc1` stores are written through
// while the kernel is still computing.  (Measured alternatives, docs/experiments.md round 3: `sc0 sc1` the same,
// `nt` / `sc1 nt` 13 % slower -- the consumer launch then finds nothing in the Infinity Cache; plain stores +1 %.)
__device__ inline void store_stream(float* p, const v4f& v) {
    // (s_nop 1: the store reads its four data registers over the following states and hipcc pads nothing
    //  inside an asm statement -- cdna_hip_programming.md 5.7)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

// register sets in flight per lane in the register-staged kernels (A/B on the whole step: 2 / 2 /
// 4 beats 4 / 4 / 4 by 1.8 %, 3 and 8 lose; compile-time switches for re-measuring.  Re-measured every round: 2 / 2 / 4 at
// 256 rows, 1 for the 64x32 input-gradient body of the >= 512-row pairs; profiles/r03_ab_regdepth_final.txt,
// r03_ab_regdepth_c5.txt)
constexpr int kRegDepthD = 2, kRegDepthD64 = 1, kRegDepth16 = 4, kRegDepthW = 2;
// host-side default for GemmArgs::krot: off (measured: no gain); PVAE_KROT=1 enables
inline int g_krot = 0;                       // pvae_set_option(NULL, "krot", 1)
// Experiment (off by default): XCD x takes q-tile (row block) x of a 256-row layer and ALL its p-tiles, instead of
// all q-tiles of an eighth of the p-tiles -- the operand traffic a row-block-stationary multi-layer kernel would
// have (every XCD streams the whole weight matrix through its L2).  Same tiles, same results.
inline int g_rowxcd = 0;                     // pvae_set_option(NULL, "rowxcd", 1)
struct GemmArgs {
    const float* Q;
    int ldq;
    const float* P;
    int ldp;
    int K, tiles_q, tiles_p, p_per_xcd;
    int krot = g_krot;        // rotate each workgroup's K order (see k_rotation)
    int tile32 = 0;           // weight gradient on 32x32 output tiles (wgrad32_body) instead of 64x64
    int tile16 = 0;           // input gradient on 16x16 output tiles (splitk_reg16_body<false>) instead of 32x32
    int rowxcd = g_rowxcd;    // see g_rowxcd
};
// Kernel-argument preload (gfx950: the first user SGPRs are filled by the hardware at wave launch; hipcc -mllvm
// -amdgpu-kernarg-preload-count=16 in physicsvae_amd/build.py, at most 14 dwords, scalars and pointers only -- a
// struct passed by value is fetched by s_load inside the kernel, ~0.26 us on the critical path of every dependent
// launch: tools/kernarg_preload_probe.hip).  The contraction kernels therefore take the operands every workgroup
// needs before it can issue its first load as LEADING scalar parameters (11 dwords) and rebuild the GemmArgs from
// them; epilogue structs follow and arrive by s_load while the first tiles are in flight.
#define PVAE_GA_PARAMS(n) const float* n##Q, const float* n##P, int n##ldq, int n##ldp, int n##K, int n##tq, int n##tp, \
                          int n##ppx, int n##fl
#define PVAE_GA_PASS(g) (g).Q, (g).P, (g).ldq, (g).ldp, (g).K, (g).tiles_q, (g).tiles_p, (g).p_per_xcd, ga_flags(g)
#define PVAE_GA_OF(n) GemmArgs{n##Q, n##ldq, n##P, n##ldp, n##K, n##tq, n##tp, n##ppx, n##fl & 7, (n##fl >> 3) & 1, (n##fl >> 4) & 1, (n##fl >> 5) & 1}
// Launches that hold TWO contractions (input gradient || weight gradient, or the two trailing weight gradients) carry
// both sets of operands in the 14 preloadable dwords: four pointers, and per contraction the two row strides, the two
// tile counts (16 bits each) and the contraction length with the six switch bits (26 + 6 bits).  The workgroup
// counts of the two bodies follow from the tile counts (make_grid).  A/B of what is preloaded, joint step / config-5
// sizes: nothing 248.2 / 391.1 us, weight-gradient operands 246.4 / 388.7, input-gradient operands 244.4 / 385.5,
// both (this) -- profiles/r03_ab_kernarg_preload.txt.
#define PVAE_GA2_PARAMS const float* aQ, const float* aP, const float* bQ, const float* bP, unsigned a_ld, unsigned b_ld, \
                        unsigned a_t, unsigned b_t, unsigned a_k, unsigned b_k
#define PVAE_GA2_PASS(ga, gb) (ga).Q, (ga).P, (gb).Q, (gb).P, ga_pack_ld(ga), ga_pack_ld(gb), ga_pack_t(ga), ga_pack_t(gb), \
                              ga_pack_k(ga), ga_pack_k(gb)
#define PVAE_GA2_A ga_unpack(aQ, aP, a_ld, a_t, a_k)
#define PVAE_GA2_B ga_unpack(bQ, bP, b_ld, b_t, b_k)
// (krot: three bits -- the probes under tools/ use it as their ablation mode)
inline int ga_flags(const GemmArgs& g) { return (g.krot & 7) | ((g.tile32 & 1) << 3) | ((g.tile16 & 1) << 4) | ((g.rowxcd & 1) << 5); }
inline unsigned ga_pack_ld(const GemmArgs& g) { return (unsigned)g.ldq | ((unsigned)g.ldp << 16); }
inline unsigned ga_pack_t(const GemmArgs& g) { return (unsigned)g.tiles_q | ((unsigned)g.tiles_p << 16); }
inline unsigned ga_pack_k(const GemmArgs& g) { return (unsigned)g.K | ((unsigned)ga_flags(g) << 26); }
// what the packed form can carry (checked by the launchers; pvae_layout.h refuses stacks beyond it)
inline bool ga_packable(const GemmArgs& g) {
    return g.ldq >= 0 && g.ldq < 65536 && g.ldp >= 0 && g.ldp < 65536 && g.tiles_q >= 0 && g.tiles_q < 65536 &&
           g.tiles_p >= 0 && g.tiles_p < 65536 && g.K >= 0 && g.K < (1 << 26) && g.p_per_xcd == (g.tiles_p + 7) / 8;
}
__host__ __device__ inline int ga_grid(const GemmArgs& g) { return 8 * g.p_per_xcd * g.tiles_q; }
__device__ inline GemmArgs ga_unpack(const float* Q, const float* P, unsigned ld, unsigned t, unsigned k) {
    const int tp = (int)(t >> 16), fl = (int)(k >> 26);
    return GemmArgs{Q, (int)(ld & 0xffffu), P, (int)(ld >> 16), (int)(k & 0x3ffffffu), (int)(t & 0xffffu), tp, (tp + 7) / 8,
                    fl & 7, (fl >> 3) & 1, (fl >> 4) & 1, (fl >> 5) & 1};
}

// Experiment (off by default): start each workgroup at a different k-tile and wrap around, so that
// the workgroups of an XCD that share operand rows (same q-tile: X rows, same p-tile: W rows) do
// not walk K in lockstep -- a k-slab would be pulled into L2 by one workgroup and found there by the
// others a few tiles later.  Hypothesis: lockstep first-touch misses bound the tile rate.
// Measured: no change to slightly worse (hidden layer 8.44 -> 8.47 us, step 114 -> 117 us), i.e.
// the per-iteration rate is not miss-latency bound.  The summation order over K would differ per
// workgroup but stay a fixed function of the block index (deterministic).
__device__ inline int k_rotation(const GemmArgs& ga, int loc, int tile_q, int nk) {
    if (!ga.krot || nk < 2) return 0;
    const int pi = loc / ga.tiles_q;                       // position among this XCD's p-tiles
    int sq = nk / ga.p_per_xcd, sp = nk / ga.tiles_q;
    if (sq < 1) sq = 1;
    if (sp < 1) sp = 1;
    return (pi * sq + tile_q * sp) % nk;
}
constexpr int kRegRingFloats = 2 * 2 * 32 * 64;      // 2 LDS slots x (Q tile + P tile) = 32 KB
}  // namespace pvae
