// pvae_gemm_reg.h -- register-staged split-K forward / input-gradient bodies (32x32, 64x32, 16x16 tiles) and their kernels.
#pragma once
#include "pvae_gemm_common.h"

namespace pvae {
// ---------------------------------------------------------------------------------------
// The contraction kernels.
//
// Fragments are fetched with as few, as wide DS reads as the MFMA layout allows, because with
// one wave per SIMD ds_read_b32/b64 issue at ~1/5 of the LDS rate (MI355X_MICROARCH.md LDS
// table) while ds_read_b128 runs at full rate:
//   * k-contiguous ("ROW") operands: ONE ds_read_b128 = 4 k-values of one row per lane; lane
//     (i, h) holds k = 16c + 4h + s, MFMA step s takes element s (the k order inside a 16-chunk
//     is a permutation, shared by both operands);
//   * output-contiguous ("COL") operands: ds_read_b64 = 2 consecutive outputs of one k per
//     lane, feeding TWO interleaved MFMA tiles (tile u owns outputs 2i + u);
//   * the 4 waves of a workgroup split K instead of the tile (forward / dgrad): every wave owns
//     the whole 32x32 output as 2x2 MFMA tiles, so each fragment feeds two MFMAs; partial tiles
//     are summed through LDS in a fixed order at the end.
// Tiles travel global -> VGPR (plain global_load_dwordx4, D register sets per lane, see kRegDepth*) ->
// ds_write_b128 into a 2-slot LDS image.  The image is lane-linear (slot j = 16-byte chunk j of
// the tile) with the chunk order XOR-permuted on the way in and, identically, on the fragment
// read (involutions), which removes bank conflicts without padding:
//   ROW tile [32][64]   b128 reads : chunk ^= row & 15
//   COL tile [64 k][32] b64 reads  : LDS row = k ^ ((k >> 2) & 1)   (rows k, k+4 of one 32-lane
//                                    group land in different bank halves)
//   COL tile [32 k][64] b64 reads  : chunk ^= (row & 1) << 3        (rows k, k+1 likewise)
// (An LDS-DMA ring variant of the same kernels -- global_load_lds, 8 stages, counted vmcnt --
// measured ~12 % slower because a DMA instruction costs ~150 issue cycles on the wave that also
// feeds the matrix pipe; it was dropped after round 1, the measurement is in DESIGN.md section 4.)
// ---------------------------------------------------------------------------------------
// ---- forward / dgrad: C[32 q][32 p] per workgroup, BK = 64, the 4 waves split K -------------
//   Q is always ROW (X or dZ, k-contiguous).  P_ROW: W[p][k] (forward);  !P_ROW: W[k][p] (dgrad).
// ABL (tools/pair_lab.hip, tools/pair_probe.hip only; 0 in production): 1 = no tile staging in the loop, 2 = no LDS
// fragment reads, 4 = no MFMA, 8 = no barrier (here: no ordering point in the k-loop), 16 = no gradient store
// (wgrad_reg_body only: epi.apply skipped), 32 = the bits apply to the input-gradient body of a pair alone.
// ---------------------------------------------------------------------------------------
// Wave-private staging.  Wave w reads only its own k-quarter of a staged tile -- chunks 4w .. 4w+3 of every row of a ROW
// operand, k-rows 16w .. 16w+15 of a COL operand -- so no byte of the image is read by a wave that did not write it if
// every wave stages exactly the chunks it reads: LDS transposes lanes, it shares nothing.  One wave's LDS instructions
// execute in order, so the k-loops of splitk_reg_body and splitk_reg16_body hold no workgroup barrier (splitk_reg64_body
// keeps the thread-linear map and its barriers: see there); the first barrier of a body stands between the loop
// and the split-K reduction buffer, which overlays the staging ring (a fast wave's partial tile would otherwise land on
// chunks a slower wave has yet to read).  The 2-slot ring holds as before: a wave's write of slot (t+1)&1 follows its
// own reads of that slot in its own LDS queue.
//   ROW tile: lanes 4m .. 4m+3 stage chunks 4w .. 4w+3 (64 contiguous bytes) of row 16u + stage_row16(lane).  The eight
//   lanes of a ds_write_b128 group hold two rows; a row's four chunks fill one 64-byte half of the 128-byte bank line,
//   which half is bit 2 of (chunk ^ row), so the two rows of a group differ in bit 2 (rows r and r + 4): conflict-free
//   (row = lane >> 2 would pair rows r and r + 1 on the same half: 2-way).
//   COL tile: eight (PT = 32) or four (PT = 16) lanes stage one whole k-row; a write group covers 128 contiguous bytes.
__device__ inline int stage_row16(int lane) {
    const int m = lane >> 2;
    return (m & 8) | ((m & 1) << 2) | ((m >> 1) & 3);
}
// What stands where the k-loop barrier stood: nothing for the hardware, an ordering point for the compiler -- a lane reads
// what other lanes of its wave wrote, and hipcc may otherwise prove that a thread's own store and load do not alias and
// hoist the read over the write.
__device__ inline void wave_order_point() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// ---------------------------------------------------------------------------------------
// Split-K partial tile of a wave -> its LDS reduction buffer red[32][RS], with 16-byte writes: the MFMA layout gives
// each lane runs of consecutive p (P_ROW: acc[a][b] = 4 consecutive p of row 16a + li; output-contiguous operands:
// for one a the eight values acc[a][0..1][0..3] are columns 8 lh .. 8 lh + 7).  RS = 36: the eight lanes of a
// ds_write_b128 group (li = 0..7) land on rows 36 dwords apart = all 32 banks once; the scalar writes this replaces
// hit 4-8 lanes per bank (PMC: 12-15 % of LDS cycles in the narrow launches of round 2).
template <bool P_ROW>
__device__ inline void store_partial_32x32(float* red, const v4f (&acc)[2][2], int li, int lh) {
    constexpr int RS = 36;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        float* row = red + (16 * a + li) * RS;
        if (P_ROW) {
#pragma unroll
            for (int b = 0; b < 2; ++b) *reinterpret_cast<v4f*>(row + 16 * b + 4 * lh) = acc[a][b];
        } else {
            *reinterpret_cast<v4f*>(row + 8 * lh) = v4f{acc[a][0][0], acc[a][1][0], acc[a][0][1], acc[a][1][1]};
            *reinterpret_cast<v4f*>(row + 8 * lh + 4) = v4f{acc[a][0][2], acc[a][1][2], acc[a][0][3], acc[a][1][3]};
        }
    }
}

template <bool P_ROW, class Epi, int ABL = 0>
__device__ inline void splitk_reg_body(float* lds, int bid, const GemmArgs& ga, Epi& epi) {
    constexpr int BK = 64, kTile = 32 * 64, kStage = 2 * kTile, D = kRegDepthD, S = 2;
    static_assert(S * kStage >= 4 * 32 * 36, "ring must hold the split-K reduction buffer");
    const float* __restrict__ Q = ga.Q;
    const float* __restrict__ P = ga.P;
    const int ldq = ga.ldq, ldp = ga.ldp, K = ga.K, tiles_q = ga.tiles_q, tiles_p = ga.tiles_p;

    const int xcd = bid & 7, loc = bid >> 3;
    const int tile_p = xcd * ga.p_per_xcd + loc / tiles_q;
    const int tile_q = loc % tiles_q;
    if (tile_p >= tiles_p) return;
    const int q0 = tile_q * 32, p0 = tile_p * 32;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int li = lane & 15, lh = lane >> 4;

    // wave-private staging (see above): two chunks of each operand tile per thread
    const float* sq[2];
    const float* sp[2];
    int slot_off[2], slot_off_p[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int row = 16 * u + stage_row16(lane), c = 4 * wave + (lane & 3);
        slot_off[u] = (row * 16 + (c ^ (row & 15))) * 4;
        sq[u] = Q + (size_t)(q0 + row) * ldq + c * 4;
        if (P_ROW) {
            slot_off_p[u] = slot_off[u];
            sp[u] = P + (size_t)(p0 + row) * ldp + c * 4;
        } else {
            const int k = 16 * wave + 8 * u + (lane >> 3);
            slot_off_p[u] = (k ^ ((k >> 2) & 1)) * 32 + (lane & 7) * 4;
            sp[u] = P + (size_t)k * ldp + p0 + (lane & 7) * 4;
        }
    }
    const size_t kstep_p = P_ROW ? (size_t)BK : (size_t)BK * ldp;

    v4f rg[D][4];
    auto gload = [&](int t, v4f(&r)[4]) {
        r[0] = *reinterpret_cast<const v4f*>(sq[0] + (size_t)t * BK);
        r[1] = *reinterpret_cast<const v4f*>(sp[0] + (size_t)t * kstep_p);
        r[2] = *reinterpret_cast<const v4f*>(sq[1] + (size_t)t * BK);
        r[3] = *reinterpret_cast<const v4f*>(sp[1] + (size_t)t * kstep_p);
    };
    auto lwrite = [&](float* slot, const v4f(&r)[4]) {
        *reinterpret_cast<v4f*>(slot + slot_off[0]) = r[0];
        *reinterpret_cast<v4f*>(slot + kTile + slot_off_p[0]) = r[1];
        *reinterpret_cast<v4f*>(slot + slot_off[1]) = r[2];
        *reinterpret_cast<v4f*>(slot + kTile + slot_off_p[1]) = r[3];
    };

    v4f acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = v4f{0.f, 0.f, 0.f, 0.f};

    int oq[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int row = 16 * a + li;
        oq[a] = row * 64 + (((4 * wave + lh) ^ (row & 15)) << 2);
    }
    const int kq = 16 * wave + 4 * lh;

    const int nk = K / BK;
#pragma unroll
    for (int d = 0; d < D; ++d) gload(d < nk ? d : nk - 1, rg[d]);     // (clamped, not guarded: exact vmcnt)
    lwrite(lds, rg[0]);
    gload(D < nk ? D : nk - 1, rg[0]);
    const typename Epi::Pre epre = epi.preload(q0 + (tid >> 3), p0 + ((tid & 7) << 2));   // arrives under the loop
    wave_order_point();

    v4f abl_q = v4f{1.f, 2.f, 3.f, 4.f} * (float)(lane + 1);
    asm volatile("" : "+v"(abl_q));
    // one k-tile; see wgrad_reg_body for why the full groups are branch-free (exact vmcnt: the
    // three younger register sets stay in flight across the LDS write of the oldest)
    auto tile_step = [&](int t, int d, bool guarded) {
        const float* st = lds + (t & 1) * kStage;
        v4f fq[2], fp[2];
        v2f fc[4];
        if (ABL & 2) {            // (probes) loop-invariant fragments the compiler cannot see through
#pragma unroll
            for (int a = 0; a < 2; ++a) { fq[a] = abl_q; fp[a] = abl_q; }
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) fc[s2] = v2f{abl_q[0], abl_q[1]};
            asm volatile("" : "+v"(fq[0]), "+v"(fq[1]), "+v"(fp[0]), "+v"(fp[1]));
        } else {
#pragma unroll
            for (int a = 0; a < 2; ++a) fq[a] = *reinterpret_cast<const v4f*>(st + oq[a]);
            if (P_ROW) {
#pragma unroll
                for (int b = 0; b < 2; ++b) fp[b] = *reinterpret_cast<const v4f*>(st + kTile + oq[b]);
            } else {
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2)
                    fc[s2] = *reinterpret_cast<const v2f*>(st + kTile + (((kq + s2) ^ (lh & 1)) * 32) + 2 * li);
            }
        }
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const float pv = P_ROW ? fp[b][s2] : fc[s2][b];
                    if (ABL & 4) acc[a][b][0] += pv * fq[a][s2];
                    else acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv, fq[a][s2], acc[a][b], 0, 0, 0);
                }
            if (s2 == 1 && !(ABL & 1)) {
                // tile t+1 sits in register set (d+1)%D: park it in the other LDS slot and
                // refill the registers with tile t+1+D
                if (!guarded) {
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    const int tn = t + 1 + D < nk ? t + 1 + D : nk - 1;
                    gload(tn, rg[(d + 1) % D]);
                } else if (t + 1 < nk) {
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    if (t + 1 + D < nk) gload(t + 1 + D, rg[(d + 1) % D]);
                }
            }
        }
        if (!(ABL & 8)) wave_order_point();
    };
    int t0 = 0;
    for (; t0 + D <= nk; t0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) tile_step(t0 + d, d, false);
    }
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (t0 + d < nk) tile_step(t0 + d, d, true);

    __syncthreads();                       // the reduction buffer overlays the ring: every wave has read its last tile
    constexpr int RS = 36;
    store_partial_32x32<P_ROW>(lds + wave * (32 * RS), acc, li, lh);
    __syncthreads();
    {
        const int ql = tid >> 3, pl = (tid & 7) << 2;
        v4f v = *reinterpret_cast<const v4f*>(lds + ql * RS + pl);
#pragma unroll
        for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const v4f*>(lds + w * (32 * RS) + ql * RS + pl);
        epi(q0 + ql, p0 + pl, v, epre);
    }
    epi.finish(lds, tile_q * tiles_p + tile_p, tid);
}


// ---- input gradient on 64 x 32 output tiles, register-staged (the dgrad half of the fused pairs at >= 512 rows) ----
// Same contraction and the same LDS images / swizzles as splitk_reg_body<false>, but the workgroup owns 64 batch rows:
// per k-tile it stages a [64][64] dZ tile + a [64 k][32] W tile (24 KB) for the MFMA work of two 32x32 tiles (which
// stage 2 x 16 KB), and every P fragment read feeds four MFMA tiles instead of two -- at 512 rows the 32x32 form put
// 512 input-gradient workgroups beside the weight-gradient ones and the launch was bound by what they stage
// (config-5 sizes).  Each wave still owns one k-quarter of every k-tile and walks it in the same order, and
// the four partial tiles are summed in the same order, so results equal the 32x32 body's bit for bit.
constexpr int kReg64RingFloats = 2 * (64 * 64 + 64 * 32);          // 2 slots x 24 KB = 48 KB
template <class Epi>
__device__ inline void splitk_reg64_body(float* lds, int bid, const GemmArgs& ga, Epi& epi) {
    constexpr int BK = 64, kTileQ = 64 * 64, kTileP = 64 * 32, kStage = kTileQ + kTileP, D = kRegDepthD64;
    constexpr int RS = 36;
    static_assert(2 * kStage >= 4 * 64 * RS, "ring must hold the split-K reduction buffer");
    const float* __restrict__ Q = ga.Q;
    const float* __restrict__ P = ga.P;
    const int ldq = ga.ldq, ldp = ga.ldp, K = ga.K, tiles_q = ga.tiles_q, tiles_p = ga.tiles_p;
    const int xcd = bid & 7, loc = bid >> 3;
    const int tile_p = xcd * ga.p_per_xcd + loc / tiles_q;
    const int tile_q = loc % tiles_q;
    if (tile_p >= tiles_p) return;
    const int q0 = tile_q * 64, p0 = tile_p * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lh = lane >> 4;

    // (slot j = 16-byte chunk j of the tile, staged by thread j & 255: whole 256-byte rows per 16 lanes, and a barrier behind
    //  every k-tile.  The wave-private map of splitk_reg_body measured SLOWER here -- 1024 rows 585.9 -> 599.8 us, 512 rows
    //  unchanged, profiles/r12_ab_reg_private.txt -- and was taken out again.)
    const float* sq[4];
    const float* sp[2];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j = tid + 256 * u, row = j >> 4, c = (j & 15) ^ (row & 15);
        sq[u] = Q + (size_t)(q0 + row) * ldq + c * 4;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int j = tid + 256 * u, r = j >> 3, k = r ^ ((r >> 2) & 1);
        sp[u] = P + (size_t)k * ldp + p0 + (j & 7) * 4;
    }
    const size_t kstep_p = (size_t)BK * ldp;
    v4f rg[D][6];
    auto gload = [&](int t, v4f(&r)[6]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = *reinterpret_cast<const v4f*>(sq[u] + (size_t)t * BK);
#pragma unroll
        for (int u = 0; u < 2; ++u) r[4 + u] = *reinterpret_cast<const v4f*>(sp[u] + (size_t)t * kstep_p);
    };
    auto lwrite = [&](float* slot, const v4f(&r)[6]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) *reinterpret_cast<v4f*>(slot + (tid + 256 * u) * 4) = r[u];
#pragma unroll
        for (int u = 0; u < 2; ++u) *reinterpret_cast<v4f*>(slot + kTileQ + (tid + 256 * u) * 4) = r[4 + u];
    };
    v4f acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = v4f{0.f, 0.f, 0.f, 0.f};
    int oq[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int row = 16 * a + li;
        oq[a] = row * 64 + (((4 * wave + lh) ^ (row & 15)) << 2);
    }
    const int kq = 16 * wave + 4 * lh;
    const int nk = K / BK;
#pragma unroll
    for (int d = 0; d < D; ++d) gload(d < nk ? d : nk - 1, rg[d]);     // (clamped, not guarded: exact vmcnt)
    lwrite(lds, rg[0]);
    gload(D < nk ? D : nk - 1, rg[0]);
    typename Epi::Pre epre[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) epre[h] = epi.preload(q0 + 32 * h + (tid >> 3), p0 + ((tid & 7) << 2));
    __syncthreads();
    auto tile_step = [&](int t, int d, bool guarded) {
        const float* st = lds + (t & 1) * kStage;
        v4f fq[4];
        v2f fc[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) fq[a] = *reinterpret_cast<const v4f*>(st + oq[a]);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
            fc[s2] = *reinterpret_cast<const v2f*>(st + kTileQ + (((kq + s2) ^ (lh & 1)) * 32) + 2 * li);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fc[s2][b], fq[a][s2], acc[a][b], 0, 0, 0);
            if (s2 == 1) {
                if (!guarded) {
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    const int tn = t + 1 + D < nk ? t + 1 + D : nk - 1;
                    gload(tn, rg[(d + 1) % D]);
                } else if (t + 1 < nk) {
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    if (t + 1 + D < nk) gload(t + 1 + D, rg[(d + 1) % D]);
                }
            }
        }
        __syncthreads();
    };
    int t0 = 0;
    for (; t0 + D <= nk; t0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) tile_step(t0 + d, d, false);
    }
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (t0 + d < nk) tile_step(t0 + d, d, true);

    float* red = lds + wave * (64 * RS);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        float* row = red + (16 * a + li) * RS;                       // (16-byte writes: see store_partial_32x32)
        *reinterpret_cast<v4f*>(row + 8 * lh) = v4f{acc[a][0][0], acc[a][1][0], acc[a][0][1], acc[a][1][1]};
        *reinterpret_cast<v4f*>(row + 8 * lh + 4) = v4f{acc[a][0][2], acc[a][1][2], acc[a][0][3], acc[a][1][3]};
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ql = 32 * h + (tid >> 3), pl = (tid & 7) << 2;
        v4f v = *reinterpret_cast<const v4f*>(lds + ql * RS + pl);
#pragma unroll
        for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const v4f*>(lds + w * (64 * RS) + ql * RS + pl);
        epi(q0 + ql, p0 + pl, v, epre[h]);
    }
    epi.finish(lds, tile_q * tiles_p + tile_p, tid);
}

template <bool P_ROW, class Epi, int ABL = 0>
__global__ void __launch_bounds__(256)
gemm_splitk_reg_kernel(PVAE_GA_PARAMS(a_), Epi epi) {
    const GemmArgs ga = PVAE_GA_OF(a_);
    __shared__ __attribute__((aligned(16))) float lds[kRegRingFloats];
    splitk_reg_body<P_ROW, Epi, ABL>(lds, blockIdx.x, ga, epi);
}

// ---- forward, 16x16 tile per workgroup (narrow output layers) ----------------------------------
// An output layer with few features (197 / 64 / 45 -> 8 or fewer 32-wide p-tiles) gives the 32x32
// kernel under 128 workgroups: most CUs idle for a full K = 1024 pass.  Same algorithm on a
// 16x16 tile (one MFMA tile per wave, two accumulators alternating over the k-steps so the
// dependent-issue latency is covered; the 4 waves still split K): 4x the workgroups, each
// streaming (16 + 16) rows.  4 flop/B, so it only pays when the grid would otherwise be small.
// P_ROW = false is the input-gradient form (P = W[k][p], p contiguous) for first-layer gradients:
// 256 x 256 outputs are 64 tiles of 32x32 that run a full K = 1024 pass on a quarter of the CUs
// (9.5 us), 256 of these.  Its P image is [64 k][16 p] row-major, read one dword per k-step.
template <bool P_ROW, class Epi>
__device__ inline void splitk_reg16_body(float* lds, int bid, const GemmArgs& ga, Epi& epi) {
    constexpr int BK = 64, kTile = 16 * 64, kStage = 2 * kTile, D = kRegDepth16;
    const float* __restrict__ Q = ga.Q;
    const float* __restrict__ P = ga.P;
    const int ldq = ga.ldq, ldp = ga.ldp, K = ga.K, tiles_q = ga.tiles_q, tiles_p = ga.tiles_p;

    const int xcd = bid & 7, loc = bid >> 3;
    const int tile_p = xcd * ga.p_per_xcd + loc / tiles_q;
    const int tile_q = loc % tiles_q;
    if (tile_p >= tiles_p) return;
    const int q0 = tile_q * 16, p0 = tile_p * 16;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int li = lane & 15, lh = lane >> 4;

    // one 16-byte chunk of each operand tile per thread, wave-private (see splitk_reg_body): chunk 4 wave + (lane & 3) of
    // row stage_row16(lane), kept at slot row * 16 + (chunk ^ row)
    const int srow = stage_row16(lane), schunk = 4 * wave + (lane & 3);
    const float* sq = Q + (size_t)(q0 + srow) * ldq + schunk * 4;
    const float* sp = P_ROW ? P + (size_t)(p0 + srow) * ldp + schunk * 4
                            : P + (size_t)(tid >> 2) * ldp + p0 + (tid & 3) * 4;      // k = tid/4 = 16 wave + lane/4, 4 chunks per row
    const size_t kstep_p = P_ROW ? (size_t)BK : (size_t)BK * ldp;
    const int slot_off = (srow * 16 + (schunk ^ srow)) * 4;
    // input-gradient form: P image rows k are kept at row k ^ ((k >> 2) & 1).  A fragment read touches rows
    // 4 lh + s2 (16 dwords each): rows 4 apart would otherwise fall on the same 16 banks for both halves of a
    // 32-lane read group (2-way conflict on every k-step: 15 % of the LDS cycles of the sampler-seed launch)
    const int pk = tid >> 2;
    const int slot_off_p = P_ROW ? slot_off : ((pk ^ ((pk >> 2) & 1)) * 16 + (tid & 3) * 4);

    v4f rg[D][2];
    auto gload = [&](int t, v4f(&r)[2]) {
        r[0] = *reinterpret_cast<const v4f*>(sq + (size_t)t * BK);
        r[1] = *reinterpret_cast<const v4f*>(sp + (size_t)t * kstep_p);
    };
    auto lwrite = [&](float* slot, const v4f(&r)[2]) {
        *reinterpret_cast<v4f*>(slot + slot_off) = r[0];
        *reinterpret_cast<v4f*>(slot + kTile + slot_off_p) = r[1];
    };
    v4f acc[2] = {v4f{0.f, 0.f, 0.f, 0.f}, v4f{0.f, 0.f, 0.f, 0.f}};
    const int of = li * 64 + (((4 * wave + lh) ^ li) << 2);

    const int nk = K / BK;
#pragma unroll
    for (int d = 0; d < D; ++d) gload(d < nk ? d : nk - 1, rg[d]);     // (clamped, not guarded: exact vmcnt)
    lwrite(lds, rg[0]);
    gload(D < nk ? D : nk - 1, rg[0]);
    wave_order_point();

    // (full groups of D tiles are branch-free so that the compiler counts the outstanding loads
    // exactly -- see wgrad_reg_body)
    auto frag_read = [&](const float* st, v4f& fq, v4f& fp) {
        fq = *reinterpret_cast<const v4f*>(st + of);
        if (P_ROW) {
            fp = *reinterpret_cast<const v4f*>(st + kTile + of);
        } else {
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) fp[s2] = st[kTile + ((16 * wave + 4 * lh + s2) ^ (lh & 1)) * 16 + li];
        }
    };
    auto tile_step = [&](int t, int d, bool guarded) {
        v4f fq, fp;
        frag_read(lds + (t & 1) * kStage, fq, fp);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
            acc[s2 & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(fp[s2], fq[s2], acc[s2 & 1], 0, 0, 0);
            if (s2 == 1) {
                if (!guarded) {
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    const int tn = t + 1 + D < nk ? t + 1 + D : nk - 1;
                    gload(tn, rg[(d + 1) % D]);
                } else if (t + 1 < nk) {
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    if (t + 1 + D < nk) gload(t + 1 + D, rg[(d + 1) % D]);
                }
            }
        }
        wave_order_point();
    };
    int t0 = 0;
    for (; t0 + D <= nk; t0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) tile_step(t0 + d, d, false);
    }
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (t0 + d < nk) tile_step(t0 + d, d, true);

    // split-K reduction (fixed order) + epilogue: 64 threads x float4 cover the 16x16 tile
    __syncthreads();                       // the reduction buffer overlays the ring: every wave has read its last tile
    constexpr int RS = 20;
    float* red = lds + wave * (16 * RS);
    const v4f mine = acc[0] + acc[1];
    *reinterpret_cast<v4f*>(red + li * RS + 4 * lh) = mine;
    __syncthreads();
    if (tid < 64) {
        const int ql = tid >> 2, pl = (tid & 3) << 2;
        v4f v = *reinterpret_cast<const v4f*>(lds + ql * RS + pl);
#pragma unroll
        for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const v4f*>(lds + w * (16 * RS) + ql * RS + pl);
        epi(q0 + ql, p0 + pl, v, epi.preload(q0 + ql, p0 + pl));
    }
    epi.finish(lds, tile_q * tiles_p + tile_p, tid);
}

template <bool P_ROW, class Epi>
__global__ void __launch_bounds__(256)
gemm_splitk_reg16_kernel(PVAE_GA_PARAMS(a_), Epi epi) {
    const GemmArgs ga = PVAE_GA_OF(a_);
    __shared__ __attribute__((aligned(16))) float lds[2 * 2 * 16 * 64];
    splitk_reg16_body<P_ROW, Epi>(lds, blockIdx.x, ga, epi);
}
}  // namespace pvae
