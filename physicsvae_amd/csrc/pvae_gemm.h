// pvae_gemm.h -- fp32 MFMA kernels for the three contractions of an MLP layer at minibatch
// scale (M = 32 rows and up, measured to 4096; tiles of 16x16 to 64x64 by problem size).  gfx950 only.
//
//   C[q][p] = sum_k Q(q,k) * P(p,k)            C row-major, p contiguous
//
//   forward  : q = batch row, p = out feature, k = in feature   Q = X  (k-contig)  P = W  (k-contig)
//   dgrad    : q = batch row, p = in feature,  k = out feature  Q = dZ (k-contig)  P = W  (p-contig)
//   wgrad    : q = out feat,  p = in feature,  k = batch row    Q = dZ (q-contig)  P = X  (p-contig)
//
// An operand is "ROW" when its reduction index is the contiguous one in memory and "COL" when
// its output index is.  Tiles are fetched with full-line 16-byte accesses along the contiguous
// index and kept in that orientation in LDS (no transposes); the MFMA is
// v_mfma_f32_16x16x4_f32 (exact fp32 fma chain, 157 TFLOP/s peak).  The MFMA "A" slot takes the P
// fragment and the "B" slot the Q fragment, so D = C^T-tile: each lane ends up with consecutive
// p of one q -> float4 epilogue loads/stores.
//
// Block -> tile mapping is XCD-aware: block b runs on XCD b%8 (observed dispatch order, used for
// L2 locality only); each XCD is given a contiguous range of p-tiles and all q-tiles of it, so
// the P panel it streams is fetched once per XCD and the (small) Q operand stays in that L2.
//
// What bounds these kernels (tools/timeline_probe.hip, pair_probe.hip, wgrad_probe.hip, mfma_rate.hip
// on MI355X): v_mfma_f32_16x16x4_f32 issues every 32 cycles at 2.35-2.39 GHz,
// i.e. 218 ns for the 16 MFMAs a compute wave spends on a 32x32x64 k-tile.  A forward / dgrad
// launch is ~1.7 us of launch + drain, ~1 us until the first k-tile is in LDS, 272 ns per k-tile
// (the per-CU load path delivers a 16 KB tile in 170-240 ns when nothing else runs) and ~0.5 us of
// split-K reduction + epilogue; the weight-gradient body runs at ~63 % of the matrix pipe's issue
// rate (one LDS round trip in front of every 8 MFMAs) and its Adam epilogue moves 24 B per
// parameter.  hipcc's wait-count pass only stays exact in branch-free loop bodies, which is why the
// register-staged loops are written as full groups plus a guarded tail.
#pragma once
#include "pvae_gemm_common.h"
#include "pvae_stage.h"
#include "pvae_gemm_src.h"
#include "pvae_gemm_reg.h"
#include "pvae_gemm_ws.h"
#include "pvae_gemm_wgrad.h"
#include "pvae_adam.h"
#include "pvae_gemm_fused.h"
#include "pvae_gemm_epi.h"
#include "pvae_gemm_launch.h"
