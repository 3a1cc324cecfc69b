// pvae_gemm_wgrad.h -- weight-gradient bodies (64x64 and 32x32 tiles) and the bias-gradient body of the same launches.
#pragma once
#include "pvae_gemm_common.h"
#include "pvae_gemm_src.h"

namespace pvae {
// ---- wgrad: G[64 q][64 p] per workgroup, reduction over batch rows (BK = 32), both operands COL,
// waves 2x2 with 32x32 each; the epilogue operands (Adam's p, m, v) are fetched under the loop --
template <class Epi, int ABL = 0, class PS = PDense>
__device__ inline void wgrad_reg_body(float* lds, int bid, const GemmArgs& ga, Epi& epi, const PS& ps = PS()) {
    constexpr int BK = 32, kTile = 32 * 64, kStage = 2 * kTile, D = kRegDepthW, S = 2;
    static_assert(S * kStage == kRegRingFloats, "LDS budget");
    const float* __restrict__ Q = ga.Q;
    const float* __restrict__ P = ga.P;
    const int ldq = ga.ldq, ldp = ga.ldp, K = ga.K, tiles_q = ga.tiles_q, tiles_p = ga.tiles_p;

    const int xcd = bid & 7, loc = bid >> 3;
    const int tile_p = xcd * ga.p_per_xcd + loc / tiles_q;
    const int tile_q = loc % tiles_q;
    if (tile_p >= tiles_p) return;
    const int q0 = tile_q * 64, p0 = tile_p * 64;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int li = lane & 15, lh = lane >> 4;
    const int wq = (wave >> 1) * 32, wp = (wave & 1) * 32;

    const float* sq[2];
    const float* sp[2];
    int slot_off[2];
    XLanes<2, BK, D> xl;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int j = (wave + 4 * u) * 64 + lane;
        slot_off[u] = j * 4;
        const int row = j >> 4, c = (j & 15) ^ ((row & 1) << 3);
        sq[u] = Q + (size_t)row * ldq + q0 + c * 4;
        sp[u] = P + (size_t)row * ldp + p0 + c * 4;
        if constexpr (PS::kGather) xl.set(ps.x, u, row, p0 + c * 4);
    }
    const int nk_ = K / BK;
    if constexpr (PS::kGather) {
#pragma unroll
        for (int d = 0; d < D; ++d) xl.fetch(ps.x, d < nk_ ? d : nk_ - 1, d);
    }
    v4f rg[D][4];
    auto gload = [&](int t, v4f(&r)[4], int s_ = 0) {
        if constexpr (PS::kGather) {
            v4f o[2];
            r[0] = *reinterpret_cast<const v4f*>(sq[0] + (size_t)t * BK * ldq);
            r[2] = *reinterpret_cast<const v4f*>(sq[1] + (size_t)t * BK * ldq);
            xl.load(ps.x, t, t + D < nk_ ? t + D : nk_ - 1, s_, o);
            r[1] = o[0]; r[3] = o[1];
        } else {
            r[0] = *reinterpret_cast<const v4f*>(sq[0] + (size_t)t * BK * ldq);
            r[1] = *reinterpret_cast<const v4f*>(sp[0] + (size_t)t * BK * ldp);
            r[2] = *reinterpret_cast<const v4f*>(sq[1] + (size_t)t * BK * ldq);
            r[3] = *reinterpret_cast<const v4f*>(sp[1] + (size_t)t * BK * ldp);
        }
    };
    auto lwrite = [&](float* slot, const v4f(&r)[4]) {
        *reinterpret_cast<v4f*>(slot + slot_off[0]) = r[0];
        *reinterpret_cast<v4f*>(slot + kTile + slot_off[0]) = r[1];
        *reinterpret_cast<v4f*>(slot + slot_off[1]) = r[2];
        *reinterpret_cast<v4f*>(slot + kTile + slot_off[1]) = r[3];
    };

    v4f acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = v4f{0.f, 0.f, 0.f, 0.f};

    const int sw = (lh & 1) << 3;
    const int cq = wq + 2 * li, cp = wp + 2 * li;
    const int oq = lh * 64 + ((((cq >> 2) ^ sw)) << 2) + (cq & 3);
    const int op = kTile + lh * 64 + ((((cp >> 2) ^ sw)) << 2) + (cp & 3);

    const int nk = K / BK;
#pragma unroll
    for (int d = 0; d < D; ++d) gload(d < nk ? d : nk - 1, rg[d], d);     // (clamped, not guarded: exact vmcnt)
    lwrite(lds, rg[0]);
    gload(D < nk ? D : nk - 1, rg[0], 0);
    // epilogue operands: queued behind the first D tiles, they arrive while the loop runs
#ifdef PVAE_WGRAD_EPI_DIRECT
    typename Epi::Pre pre[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        pre[a][0] = epi.load(q0 + wq + 2 * li + a, p0 + wp + 8 * lh);
        pre[a][1] = epi.load(q0 + wq + 2 * li + a, p0 + wp + 8 * lh + 4);
    }
#else
    // (the epilogue's mapping: thread t owns columns 4 (t & 15) .. + 3 of rows (t >> 4) + 16 i -- whole 256-byte rows)
    const int eq = tid >> 4, ep = (tid & 15) << 2;
    typename Epi::Pre pre[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pre[i] = epi.load(q0 + eq + 16 * i, p0 + ep);
#endif
    __syncthreads();

    // one k-tile: 8 steps of (2 fragment reads, 4 MFMAs); after step 3 the next tile moves from its
    // register set into the other LDS slot and that set is refilled D tiles ahead
    // fragments of k-step kk+4 are requested before the MFMAs of k-step kk are issued: inside a tile
    // only the first read's latency is exposed (left to itself hipcc reads two k-steps with one
    // ds_read2st64_b64, waits for them, issues 8 MFMAs, and repeats: 4 exposed waits per tile;
    // fused backward launch 15.1 -> 14.8 us)
    auto tile_step_piped = [&](int t, int d, bool guarded) {
        const float* st = lds + (t & 1) * kStage;
        v2f fq[2], fp[2];
        fq[0] = *reinterpret_cast<const v2f*>(st + oq);
        fp[0] = *reinterpret_cast<const v2f*>(st + op);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            const int c = (kk >> 2) & 1, n = c ^ 1;
            if (kk + 4 < BK) {
                fq[n] = *reinterpret_cast<const v2f*>(st + oq + (kk + 4) * 64);
                fp[n] = *reinterpret_cast<const v2f*>(st + op + (kk + 4) * 64);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fp[c][b], fq[c][a], acc[a][b], 0, 0, 0);
            if (kk == 12) {
                if (!guarded) {
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    const int tn = t + 1 + D < nk ? t + 1 + D : nk - 1;
                    gload(tn, rg[(d + 1) % D], (d + 1) % D);
                } else if (t + 1 < nk) {
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    if (t + 1 + D < nk) gload(t + 1 + D, rg[(d + 1) % D], (d + 1) % D);
                }
            }
        }
        __syncthreads();
    };
    v2f abl_f = v2f{1.f, 2.f} * (float)(lane + 1);
    asm volatile("" : "+v"(abl_f));
    auto tile_step_plain = [&](int t, int d, bool guarded) {
        const float* st = lds + (t & 1) * kStage;
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            v2f fq, fp;
            if (ABL & 2) {        // (probes) loop-invariant fragments the compiler cannot see through
                fq = abl_f;
                fp = abl_f;
                asm volatile("" : "+v"(fq), "+v"(fp));
            } else {
                fq = *reinterpret_cast<const v2f*>(st + oq + kk * 64);
                fp = *reinterpret_cast<const v2f*>(st + op + kk * 64);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    if (ABL & 4) acc[a][b][0] += fp[b] * fq[a];
                    else acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fp[b], fq[a], acc[a][b], 0, 0, 0);
                }
            if (kk == 12 && !(ABL & 1)) {
                if (!guarded) {
                    // branch-free: past the end this stores a stale register set into the idle slot
                    // and re-reads the last tile -- both unused.  Without branches the compiler counts
                    // the outstanding loads exactly (vmcnt(12): three younger sets stay in flight);
                    // with the guards it drained the whole prefetch queue before every LDS write.
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    const int tn = t + 1 + D < nk ? t + 1 + D : nk - 1;
                    gload(tn, rg[(d + 1) % D], (d + 1) % D);
                } else if (t + 1 < nk) {
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    if (t + 1 + D < nk) gload(t + 1 + D, rg[(d + 1) % D], (d + 1) % D);
                }
            }
        }
        if (!(ABL & 8)) __syncthreads();
    };
    auto tile_step = [&](int t, int d, bool guarded) {
        if constexpr ((ABL & 15) == 0) tile_step_piped(t, d, guarded);
        else tile_step_plain(t, d, guarded);
    };
    int t0 = 0;
    for (; t0 + D <= nk; t0 += D) {            // full groups of D tiles: no branch inside
#pragma unroll
        for (int d = 0; d < D; ++d) tile_step(t0 + d, d, false);
    }
#pragma unroll
    for (int d = 0; d < D; ++d)                // remaining nk % D tiles
        if (t0 + d < nk) tile_step(t0 + d, d, true);

    PVAE_MARK(0, 2);                                             // contraction done, epilogue (Adam) starts
    auto emit = [&](int q, int p, v4f v, const typename Epi::Pre& pr) {
        if (ABL & 16) asm volatile("" ::"v"(v));       // (probes) the finished values stay live, nothing is stored
        else epi.apply(q, p, v, pr);
    };
#ifdef PVAE_WGRAD_EPI_DIRECT
    // straight out of the MFMA layout: a wave-instruction writes 16 rows x four 16-byte pieces 32 bytes apart, and a
    // second one fills the holes (kept for the A/B)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int q = q0 + wq + 2 * li + a, p = p0 + wp + 8 * lh;
        emit(q, p, v4f{acc[a][0][0], acc[a][1][0], acc[a][0][1], acc[a][1][1]}, pre[a][0]);
        emit(q, p + 4, v4f{acc[a][0][2], acc[a][1][2], acc[a][0][3], acc[a][1][3]}, pre[a][1]);
    }
#else
    // Through LDS into whole rows.  Lane (li, lh) holds, for a = 0, 1, columns 8 lh .. 8 lh + 7 of row 2 li + a of its
    // wave's 32x32 sub-tile; stored as it stands, each line of G is written by two instructions with a checkerboard
    // byte mask.  The ring is free (every thread has passed the last tile's barrier), so the tile goes to LDS and comes
    // back as 4 rows x 256 contiguous bytes per wave-instruction.  Row 2 li + a of a sub-tile is kept at LDS row
    // 16 a + li of its 32-row half, rows RS = 68 dwords apart: the eight lanes of a ds_write_b128 group (li = 0..7) are
    // 68 = 4 (mod 32) dwords apart, every bank once; a ds_read_b128 group is 8 + 8 lanes of two LDS rows 16 apart
    // (16 x 68 = 0 mod 64) covering dwords 0-15, 48-63 of one and 16-47 of the other, every bank once.
    constexpr int RS = 68;
    static_assert(64 * RS <= kRegRingFloats, "ring must hold the output tile");
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        float* row = lds + (wq + 16 * a + li) * RS + wp + 8 * lh;
        *reinterpret_cast<v4f*>(row) = v4f{acc[a][0][0], acc[a][1][0], acc[a][0][1], acc[a][1][1]};
        *reinterpret_cast<v4f*>(row + 4) = v4f{acc[a][0][2], acc[a][1][2], acc[a][0][3], acc[a][1][3]};
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = eq + 16 * i;                                      // output row of the tile
        const int lr = (r & 32) + 16 * (r & 1) + ((r & 31) >> 1);       // where it is kept
        emit(q0 + r, p0 + ep, *reinterpret_cast<const v4f*>(lds + lr * RS + ep), pre[i]);
    }
#endif
    if (epi.loss.out && bid == 0 && wave == 3) finalize_loss_wave(epi.loss, lane);
}

// ---- weight gradient, 32x32 output tile per workgroup ------------------------------------------
// A weight matrix with few 64x64 tiles (first / last layers: 1024x256 -> 64 tiles) occupies a
// quarter of the CUs with workgroups that run as long as those of a full 1024x1024 layer; in a fused
// launch they decide its length (layer-1 + layer-0 gradients: 16.7 us, layer 1 alone 11.2).  On 32x32
// tiles the same matrix gives four times the workgroups, each a quarter as long: the four waves
// split every 64-row k-tile (16 rows = 4 MFMA k-steps each) over the whole tile and reduce through
// LDS at the end, like the input-gradient body.  Needs K % 64 == 0 (wgrad_uses_32x32).
template <class Epi, class PS = PDense>
__device__ inline void wgrad32_body(float* lds, int bid, const GemmArgs& ga, Epi& epi, const PS& ps = PS()) {
    constexpr int BK = 64, kTile = 64 * 32, kStage = 2 * kTile, D = kRegDepthW, S = 2;
    static_assert(S * kStage == kRegRingFloats, "LDS budget");
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

    // operand images in LDS: [64 k-rows][32 columns], row-major (fragment reads and 16-byte writes
    // are conflict-free as they are); 512 16-byte chunks per operand, two per thread
    const float* sq[2];
    const float* sp[2];
    int slot_off[2];
    XLanes<2, BK, D> xl;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int j = tid + 256 * u;
        const int row = j >> 3, c = j & 7;
        slot_off[u] = j * 4;
        sq[u] = Q + (size_t)row * ldq + q0 + c * 4;
        sp[u] = P + (size_t)row * ldp + p0 + c * 4;
        if constexpr (PS::kGather) xl.set(ps.x, u, row, p0 + c * 4);
    }
    const int nk_ = K / BK;
    if constexpr (PS::kGather) {
#pragma unroll
        for (int d = 0; d < D; ++d) xl.fetch(ps.x, d < nk_ ? d : nk_ - 1, d);
    }
    v4f rg[D][4];
    auto gload = [&](int t, v4f(&r)[4], int s_ = 0) {
        if constexpr (PS::kGather) {
            v4f o[2];
            r[0] = *reinterpret_cast<const v4f*>(sq[0] + (size_t)t * BK * ldq);
            r[2] = *reinterpret_cast<const v4f*>(sq[1] + (size_t)t * BK * ldq);
            xl.load(ps.x, t, t + D < nk_ ? t + D : nk_ - 1, s_, o);
            r[1] = o[0]; r[3] = o[1];
        } else {
            r[0] = *reinterpret_cast<const v4f*>(sq[0] + (size_t)t * BK * ldq);
            r[1] = *reinterpret_cast<const v4f*>(sp[0] + (size_t)t * BK * ldp);
            r[2] = *reinterpret_cast<const v4f*>(sq[1] + (size_t)t * BK * ldq);
            r[3] = *reinterpret_cast<const v4f*>(sp[1] + (size_t)t * BK * ldp);
        }
    };
    auto lwrite = [&](float* slot, const v4f(&r)[4]) {
        *reinterpret_cast<v4f*>(slot + slot_off[0]) = r[0];
        *reinterpret_cast<v4f*>(slot + kTile + slot_off[0]) = r[1];
        *reinterpret_cast<v4f*>(slot + slot_off[1]) = r[2];
        *reinterpret_cast<v4f*>(slot + kTile + slot_off[1]) = r[3];
    };

    v4f acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = v4f{0.f, 0.f, 0.f, 0.f};

    const int of = (16 * wave + lh) * 32 + 2 * li;       // this lane's fragment pair at k-step 0 of its slice

    const int nk = K / BK;
#pragma unroll
    for (int d = 0; d < D; ++d) gload(d < nk ? d : nk - 1, rg[d], d);     // (clamped, not guarded: exact vmcnt)
    lwrite(lds, rg[0]);
    gload(D < nk ? D : nk - 1, rg[0], 0);
    const typename Epi::Pre pre = epi.load(q0 + (tid >> 3), p0 + ((tid & 7) << 2));   // arrives under the loop
    __syncthreads();

    auto tile_step = [&](int t, int d, bool guarded) {
        const float* st = lds + (t & 1) * kStage;
        v2f fq[2], fp[2];
        fq[0] = *reinterpret_cast<const v2f*>(st + of);
        fp[0] = *reinterpret_cast<const v2f*>(st + kTile + of);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
            const int c = s2 & 1, n = c ^ 1;
            if (s2 + 1 < 4) {
                fq[n] = *reinterpret_cast<const v2f*>(st + of + (s2 + 1) * 128);
                fp[n] = *reinterpret_cast<const v2f*>(st + kTile + of + (s2 + 1) * 128);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fp[c][b], fq[c][a], acc[a][b], 0, 0, 0);
            if (s2 == 1) {
                if (!guarded) {
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    const int tn = t + 1 + D < nk ? t + 1 + D : nk - 1;
                    gload(tn, rg[(d + 1) % D], (d + 1) % D);
                } else if (t + 1 < nk) {
                    lwrite(lds + ((t + 1) & 1) * kStage, rg[(d + 1) % D]);
                    if (t + 1 + D < nk) gload(t + 1 + D, rg[(d + 1) % D], (d + 1) % D);
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

    // split-K reduction over the four waves (fixed order), epilogue on float4s by all 256 threads
    // (lane (li, lh) holds, for a = 0, 1, the eight columns 8 lh .. 8 lh + 7 of output row 2 li + a.  Row 2 li + a is
    //  kept at LDS row 16 a + li, so that the eight lanes of a 16-byte write group are 36 dwords apart: every bank once)
    constexpr int RS = 36;
    float* red = lds + wave * (32 * RS);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        float* row = red + (16 * a + li) * RS;
        *reinterpret_cast<v4f*>(row + 8 * lh) = v4f{acc[a][0][0], acc[a][1][0], acc[a][0][1], acc[a][1][1]};
        *reinterpret_cast<v4f*>(row + 8 * lh + 4) = v4f{acc[a][0][2], acc[a][1][2], acc[a][0][3], acc[a][1][3]};
    }
    __syncthreads();
    {
        const int ql = tid >> 3, pl = (tid & 7) << 2;
        const int qr = 16 * (ql & 1) + (ql >> 1);                   // LDS row of output row ql
        v4f v = *reinterpret_cast<const v4f*>(lds + qr * RS + pl);
#pragma unroll
        for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const v4f*>(lds + w * (32 * RS) + qr * RS + pl);
        epi.apply(q0 + ql, p0 + pl, v, pre);
    }
    if (epi.loss.out && bid == 0 && wave == 3) finalize_loss_wave(epi.loss, lane);
}

// either geometry, chosen per problem on the host
constexpr int kPairLdsFloats = kRegRingFloats;
template <class Epi, int ABL = 0, class PS = PDense>
__device__ inline void wgrad_body(float* lds, int bid, const GemmArgs& ga, Epi& epi, const PS& ps = PS()) {
    if (ga.tile32) wgrad32_body<Epi, PS>(lds, bid, ga, epi, ps);
    else wgrad_reg_body<Epi, ABL, PS>(lds, bid, ga, epi, ps);
}

// Bias gradient of a weight-gradient problem, db[q] = sum over the K rows of Q[k][q], for 32
// columns per workgroup (fixed summation order), handed to the epilogue's bias() (store, or Adam on
// the bias).  These few light workgroups are appended to every weight-gradient launch: summing the
// fragments inside the contraction loop instead put two VALU adds beside every four MFMAs of EVERY
// wave (only 1 tile column in 16 needs them) and cost 2 % of the step.
// Shape: a launch ends with its last workgroup, and these are latency chains sharing their CU with two
// contraction workgroups -- 16 workgroups of 64 columns x 16 row groups walked K = 256 rows in 8
// dependent round trips and kept the fused backward launch open 0.8 us longer (tools/pair_lab.hip:
// 14.28 vs 13.47 us).  32 columns x 32 row groups with all K / 32 loads of a thread in flight at once
// (full 128-byte lines per row) is ONE round trip for batches up to 256 rows.
__host__ __device__ inline int bias_tiles(const GemmArgs& ga) { return ga.tile32 ? ga.tiles_q : 2 * ga.tiles_q; }
template <class Epi>
__device__ inline void bias_grad_body(float* lds, int tile, const GemmArgs& ga, Epi& epi) {
    if (!epi.has_bias() || tile >= bias_tiles(ga)) return;
    const int tid = threadIdx.x, c4 = (tid & 7) * 4, r0 = tid >> 3;       // 32 rows x 32 columns per pass
    const float* __restrict__ src = ga.Q + (size_t)r0 * ga.ldq + tile * 32 + c4;
    const size_t step = (size_t)32 * ga.ldq;
    v4f s = v4f{0.f, 0.f, 0.f, 0.f};
    int k = r0;
    for (; k + 7 * 32 < ga.K; k += 8 * 32) {      // 8 rows per thread in flight (256 batch rows per trip)
        v4f t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = *reinterpret_cast<const v4f*>(src + i * step);
        s += ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
        src += 8 * step;
    }
    for (; k < ga.K; k += 32) {
        s += *reinterpret_cast<const v4f*>(src);
        src += step;
    }
    *reinterpret_cast<v4f*>(lds + r0 * 32 + c4) = s;
    __syncthreads();
    if (tid < 32) {
        float v = 0.f;
#pragma unroll
        for (int r = 0; r < 32; ++r) v += lds[r * 32 + tid];
        epi.bias(tile * 32 + tid, v);
    }
}
}  // namespace pvae
