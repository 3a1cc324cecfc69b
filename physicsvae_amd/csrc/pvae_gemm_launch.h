// pvae_gemm_launch.h -- host side: which tile geometry a problem gets, its GemmArgs and grid, and the launchers.
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

namespace pvae {
// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------
// When the profiler arms a pair of events, the next launch goes through hipExtLaunchKernelGGL, which
// stamps them with the kernel's own start and end on the device (what rocprofv3 reports as the kernel
// duration); events recorded around a plain launch would include the launch seam.
inline hipEvent_t g_kernel_ev[2] = {nullptr, nullptr};
#define PVAE_LAUNCH(kernel, grid, block, st, ...)                                                          \
    do {                                                                                                   \
        if (g_kernel_ev[0]) {                                                                              \
            hipExtLaunchKernelGGL(kernel, grid, block, 0, st, g_kernel_ev[0], g_kernel_ev[1], 0, __VA_ARGS__); \
            g_kernel_ev[0] = g_kernel_ev[1] = nullptr;                                                     \
        } else                                                                                               \
            hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);                                   \
    } while (0)
struct GemmGrid {
    int tiles_q, tiles_p, p_per_xcd, grid;
};
inline GemmGrid make_grid(int rows_q, int cols_p, int bq, int bp) {
    GemmGrid g;
    g.tiles_q = rows_q / bq;
    g.tiles_p = cols_p / bp;
    g.p_per_xcd = (g.tiles_p + 7) / 8;
    g.grid = 8 * g.p_per_xcd * g.tiles_q;
    return g;
}

// 512 rows and more: 64x32 tiles (splitk_ws64_body) whenever they still give every CU a workgroup; PVAE_WS64=0: off (A/B)
inline int g_ws64 = 1;                       // pvae_set_option(NULL, "ws64", 0): off (tests compare the tilings bit for bit)
inline bool uses_64x32(int M, int N) { return g_ws64 && M >= 512 && M % 64 == 0 && (M / 64) * (N / 32) >= 256; }
// 1024 rows and more: 64x64 tiles whenever THEY still give every CU a workgroup; PVAE_WS6464=0: off (A/B)
inline int g_ws6464 = 1;                     // option "ws6464"
inline bool uses_64x64(int M, int N) { return g_ws6464 && uses_64x32(M, N) && N % 64 == 0 && (M / 64) * (N / 64) >= 256; }
// ... with the XCDs partitioning the ROW blocks (see splitk_ws64_body); PVAE_WS6464_ROWS=0: column ranges as elsewhere (A/B)
inline int g_ws6464_rows = 1;                // option "ws6464_rows"
// ... and the input-gradient half of the fused backward pairs (PVAE_PAIR64=0: off, A/B)
inline int g_pair64 = 1;                     // option "pair64"
inline bool pair_uses_64x32(int M, int N) { return g_pair64 && uses_64x32(M, N); }
// narrow outputs: under 128 workgroups of 32x32 -> use 16x16 tiles (4x the workgroups)
inline bool forward_uses_16x16(int M, int N) { return (M / 32) * (N / 32) < 128; }
// ... the input gradient likewise (narrow first layers; PVAE_DGRAD16=0 switches it off: A/B)
inline int g_dgrad16 = 1;                    // option "dgrad16"
inline bool dgrad_uses_16x16(int M, int Kin) { return g_dgrad16 && (M / 32) * (Kin / 32) < 128; }

// The tile geometry of a row-major [M x N] output of the forward / input-gradient family, decided in ONE place.  A call
// site says which geometries it has kernels for (TileRule); the selectors above say which of those the sizes ask for.
// The order of the checks is immaterial, because the classes are disjoint: uses_64x32 (hence uses_64x64 and
// pair_uses_64x32) needs M % 64 == 0 and (M / 64) (N / 32) >= 256, i.e. (M / 32) (N / 32) >= 512, while both 16x16
// rules need (M / 32) (N / 32) < 128.
enum TileGeom { kTile16, kTile32, kTile64x32, kTile64x64 };
struct TileRule {
    enum Narrow { kNever, kForward, kDgrad };
    bool wide = false;         // 64x64 and 64x32 (wave-specialised kernels of EpiBiasAct forward / EpiMask input gradient)
    bool pair = false;         // 64x32 alone, under `pair64`: the EpiMask input-gradient half of a fused pair
    Narrow narrow = kNever;    // 16x16 by forward_uses_16x16, or by dgrad_uses_16x16 -- which also sets GemmArgs::tile16, the
                               // switch inside the pair kernels; never for the gathered operand
    bool plain = false;        // krot / rowxcd stay 0 whatever the options say (the grouped launches of pvae_fc.hip)
};
inline TileGeom tile_geometry(const TileRule& r, int M, int N) {
    if (r.wide && uses_64x64(M, N)) return kTile64x64;
    if ((r.wide && uses_64x32(M, N)) || (r.pair && pair_uses_64x32(M, N))) return kTile64x32;
    if (r.narrow == TileRule::kForward ? forward_uses_16x16(M, N) : r.narrow == TileRule::kDgrad && dgrad_uses_16x16(M, N)) return kTile16;
    return kTile32;
}
struct TilePlan {
    TileGeom geom;
    GemmArgs ga;
    int grid;
    int tiles() const { return ga.tiles_q * ga.tiles_p; }     // workgroups whose epilogue sees a tile
};
// C[M][N] = Q[M][K] x P on tiles of `geom`: every field of the GemmArgs, and the grid (64x64 under `ws6464_rows`: the
// XCDs partition the row blocks)
inline TilePlan plan_tiles(TileGeom geom, const TileRule& r, const float* Q, int ldq, const float* P, int ldp, int M, int N, int K) {
    const int bq = geom == kTile16 ? 16 : geom == kTile32 ? 32 : 64, bp = geom == kTile16 ? 16 : geom == kTile64x64 ? 64 : 32;
    const GemmGrid g = make_grid(M, N, bq, bp);
    TilePlan t{geom, GemmArgs{Q, ldq, P, ldp, K, g.tiles_q, g.tiles_p, g.p_per_xcd, r.plain ? 0 : g_krot, 0,
                              geom == kTile16 && r.narrow == TileRule::kDgrad, r.plain ? 0 : g_rowxcd}, g.grid};
    if (geom == kTile64x64 && g_ws6464_rows) {
        t.ga.rowxcd = 1;
        t.grid = 8 * ((g.tiles_q + 7) / 8) * g.tiles_p;
    }
    return t;
}
inline TilePlan plan_tiles(const TileRule& r, const float* Q, int ldq, const float* P, int ldp, int M, int N, int K) {
    return plan_tiles(tile_geometry(r, M, N), r, Q, ldq, P, ldp, M, N, K);
}
// the input gradient wherever it shares its launch (pairs, groups): 16x16 or 32x32
inline TilePlan plan_dgrad(const float* dZ, int ldz, const float* W, int ldw, int M, int Kin, int N, bool plain = false) {
    return plan_tiles(TileRule{false, false, TileRule::kDgrad, plain}, dZ, ldz, W, ldw, M, Kin, N);
}
inline int forward_tiles(int M, int N) {
    return plan_tiles(TileRule{false, false, TileRule::kForward}, nullptr, 0, nullptr, 0, M, N, 0).tiles();
}
// (= loss partials a seed epilogue writes)
inline int dgrad_tiles(int M, int Kin) { return plan_dgrad(nullptr, 0, nullptr, 0, M, Kin, 0).tiles(); }

// the wide geometries have kernels of one epilogue per family: EpiBiasAct forward (P_ROW), EpiMask input gradient
template <bool P_ROW, class Epi>
inline constexpr bool kHasWide = std::is_same<Epi, typename std::conditional<P_ROW, EpiBiasAct, EpiMask>::type>::value;
template <bool P_ROW, class Epi>
inline void launch_wide(const TilePlan& t, const Epi& e, hipStream_t st) {
    if (t.geom == kTile64x64) PVAE_LAUNCH((gemm_splitk_ws64_kernel<P_ROW, Epi, 64>), dim3(t.grid), dim3(512), st, PVAE_GA_PASS(t.ga), e);
    else PVAE_LAUNCH((gemm_splitk_ws64_kernel<P_ROW, Epi>), dim3(t.grid), dim3(512), st, PVAE_GA_PASS(t.ga), e);
}

// forward: out[M][N] = act(X[M][K] W[N][K]^T + b)
template <class Epi>
inline hipError_t gemm_forward_epi(const float* X, int ldx, const float* W, int ldw, int M, int N, int K,
                                   const Epi& e, hipStream_t st) {
    if (!ws_offsets_fit(ldx, ldw)) return hipErrorInvalidValue;
    const TilePlan t = plan_tiles(TileRule{kHasWide<true, Epi>, false, TileRule::kForward}, X, ldx, W, ldw, M, N, K);
    // (the order in which the kernels are named here is the order in which their code is emitted)
    if (t.geom == kTile16) PVAE_LAUNCH((gemm_splitk_reg16_kernel<true, Epi>), dim3(t.grid), dim3(256), st, PVAE_GA_PASS(t.ga), e);
    else if (t.geom != kTile32) { if constexpr (kHasWide<true, Epi>) launch_wide<true>(t, e, st); }
    else PVAE_LAUNCH((gemm_splitk_ws_kernel<true, Epi>), dim3(t.grid), dim3(kWsThreads), st, PVAE_GA_PASS(t.ga), e);
    return hipGetLastError();
}
// forward layer on 32x32 tiles whose launch forms some of its own input columns (Pro, see splitk_ws_pertile_body)
inline bool forward_pro_ok(int M, int N) { return !forward_uses_16x16(M, N) && !uses_64x32(M, N) && !g_krot && !g_rowxcd; }
template <class Epi, class Pro>
inline hipError_t gemm_forward_pro(const float* X, int ldx, const float* W, int ldw, int M, int N, int K, const Epi& e,
                                   const Pro& pro, hipStream_t st) {
    if (!ws_offsets_fit(ldx, ldw)) return hipErrorInvalidValue;
    const TilePlan t = plan_tiles(kTile32, TileRule{}, X, ldx, W, ldw, M, N, K);
    PVAE_LAUNCH((gemm_splitk_ws_pro_kernel<Epi, Pro>), dim3(t.grid), dim3(kWsThreads), st, PVAE_GA_PASS(t.ga), e, pro);
    return hipGetLastError();
}
// a stack's FIRST layer on the gathered operand (XSrc): same tile geometries as gemm_forward_epi, never the 16x16 kernel
inline bool forward_gather_ok(int M, int N) { return !forward_uses_16x16(M, N) && !g_krot && !g_rowxcd; }
#define PVAE_GG_PASS(xs, ga) (xs).s0, (ga).P, (int)((unsigned)(xs).ld0 | ((unsigned)(xs).n0 << 16)), (ga).ldp, (ga).K, (ga).tiles_q, (ga).tiles_p, \
                             (ga).p_per_xcd, ga_flags(ga) | ((xs).rm.seg ? 64 : 0), (int)((unsigned)((xs).rows - 1) | ((unsigned)((xs).rm.q1 - 1) << 16)), \
                             (xs).rm.b0, (xs).rm.b1
inline bool gather_packable(const XSrc& xs) {
    return xs.ld0 > 0 && xs.ld0 < 65536 && xs.n0 >= 64 && xs.n0 < 65536 && xs.rows >= 1 && xs.rows <= 65536 && xs.rm.q1 >= 1 && xs.rm.q1 <= 65536;
}
template <class Epi>
inline hipError_t gemm_forward_gather(const XSrc& xs, const float* W, int ldw, int M, int N, int K, const Epi& e, hipStream_t st) {
    if (!gather_packable(xs)) return hipErrorInvalidValue;
    const TilePlan t = plan_tiles(TileRule{kHasWide<true, Epi>}, nullptr, 0, W, ldw, M, N, K);
    if constexpr (kHasWide<true, Epi>) {
        if (t.geom == kTile64x64) {
            PVAE_LAUNCH((gemm_splitk_ws64_gather_kernel<Epi, 64>), dim3(t.grid), dim3(512), st, PVAE_GG_PASS(xs, t.ga), e, xs);
            return hipGetLastError();
        }
        if (t.geom == kTile64x32) {
            PVAE_LAUNCH((gemm_splitk_ws64_gather_kernel<Epi, 32>), dim3(t.grid), dim3(512), st, PVAE_GG_PASS(xs, t.ga), e, xs);
            return hipGetLastError();
        }
    }
    PVAE_LAUNCH((gemm_splitk_ws_gather_kernel<Epi>), dim3(t.grid), dim3(kWsThreads), st, PVAE_GG_PASS(xs, t.ga), e, xs);
    return hipGetLastError();
}
template <class Epi, class Pro>
inline hipError_t gemm_forward_pro_gather(const XSrc& xs, const float* W, int ldw, int M, int N, int K, const Epi& e,
                                          const Pro& pro, hipStream_t st) {
    if (!gather_packable(xs)) return hipErrorInvalidValue;
    const TilePlan t = plan_tiles(kTile32, TileRule{}, nullptr, 0, W, ldw, M, N, K);
    PVAE_LAUNCH((gemm_splitk_ws_pro_gather_kernel<Epi, Pro>), dim3(t.grid), dim3(kWsThreads), st, PVAE_GG_PASS(xs, t.ga), e, pro, xs);
    return hipGetLastError();
}
inline hipError_t gemm_forward(const float* X, int ldx, const float* W, int ldw, const float* bias,
                               float* out, int ldo, int M, int N, int K, int act, hipStream_t st) {
    EpiBiasAct e{out, ldo, bias, act};
    return gemm_forward_epi(X, ldx, W, ldw, M, N, K, e, st);
}
// dgrad: dX[M][Kin] = (dZ[M][N] W[N][Kin]) .* (mask > 0), or with a caller-supplied epilogue (gradient seeds of the
// producing stack)
template <class EpiD>
inline hipError_t gemm_dgrad_epi(const float* dZ, int ldz, const float* W, int ldw, int M, int Kin, int N,
                                 const EpiD& e, hipStream_t st) {
    if (!ws_offsets_fit(ldz, ldw)) return hipErrorInvalidValue;
    const TilePlan t = plan_tiles(TileRule{kHasWide<false, EpiD>, false, TileRule::kDgrad}, dZ, ldz, W, ldw, M, Kin, N);
    if (t.geom == kTile64x64 || t.geom == kTile64x32) { if constexpr (kHasWide<false, EpiD>) launch_wide<false>(t, e, st); }
    else if (t.geom == kTile16) PVAE_LAUNCH((gemm_splitk_reg16_kernel<false, EpiD>), dim3(t.grid), dim3(256), st, PVAE_GA_PASS(t.ga), e);
    else PVAE_LAUNCH((gemm_splitk_ws_kernel<false, EpiD>), dim3(t.grid), dim3(kWsThreads), st, PVAE_GA_PASS(t.ga), e);
    return hipGetLastError();
}
inline hipError_t gemm_dgrad(const float* dZ, int ldz, const float* W, int ldw, const float* mask,
                             int ldm, float* dX, int ldo, int M, int Kin, int N, hipStream_t st, int act = 1) {
    const EpiMask e{dX, ldo, mask, ldm, act};
    return gemm_dgrad_epi(dZ, ldz, W, ldw, M, Kin, N, e, st);
}
// wgrad: G[N][Kin] = dZ[M][N]^T X[M][Kin]  (+ bias gradient, + optional loss finalisation)
// Tile geometry per problem: 64x64, or 32x32 when that leaves at most half the CUs with a tile
// (PVAE_WGRAD32=0 switches the small geometry off: A/B).
inline int g_wgrad32 = 1;                    // option "wgrad32": 0 never, 1 where it pays, 2 always
inline bool wgrad_uses_32x32(int N, int Kin, int M) {
    return g_wgrad32 && ((N / 64) * (Kin / 64) <= 128 || g_wgrad32 == 2) && M % 64 == 0;
}
struct WgradPlan {
    GemmArgs ga;
    int grid, nbias;          // contraction workgroups, bias-gradient workgroups (32 columns each)
};
// (`plain`: as TileRule::plain)
inline WgradPlan plan_wgrad(const float* dZ, int ldz, const float* X, int ldx, int N, int Kin, int M, bool plain = false) {
    const bool t32 = wgrad_uses_32x32(N, Kin, M);
    const GemmGrid g = t32 ? make_grid(N, Kin, 32, 32) : make_grid(N, Kin, 64, 64);
    return WgradPlan{GemmArgs{dZ, ldz, X, ldx, M, g.tiles_q, g.tiles_p, g.p_per_xcd, plain ? 0 : g_krot, t32, 0, plain ? 0 : g_rowxcd},
                     g.grid, N / 32};
}
template <class Epi>
inline hipError_t gemm_wgrad(const float* dZ, int ldz, const float* X, int ldx, int N, int Kin, int M,
                             const Epi& e, hipStream_t st, const AdamPair* ad = nullptr) {
    const WgradPlan w = plan_wgrad(dZ, ldz, X, ldx, N, Kin, M);
    PVAE_LAUNCH((gemm_wgrad_reg_kernel<Epi>), dim3(w.grid + w.nbias + adam_blocks(ad)), dim3(256), st, PVAE_GA_PASS(w.ga),
                w.grid, e, ad ? *ad : AdamPair());
    return hipGetLastError();
}
// one launch, two independent weight gradients (the two last layers of a backward pass)
template <class EpiW>
inline hipError_t gemm_wgrad_pair(const float* dZ1, int ldz1, const float* X1, int ldx1, int N1, int Kin1,
                                  const EpiW& e1, const float* dZ2, int ldz2, const float* X2, int ldx2, int N2,
                                  int Kin2, const EpiW& e2, int M, hipStream_t st, const StageArgs* next = nullptr,
                                  const AdamPair* ad = nullptr) {
    const WgradPlan w1 = plan_wgrad(dZ1, ldz1, X1, ldx1, N1, Kin1, M);
    const WgradPlan w2 = plan_wgrad(dZ2, ldz2, X2, ldx2, N2, Kin2, M);
    StageArgs sa;
    memset(&sa, 0, sizeof(sa));
    if (next) sa = *next;                     // rows_pad extra blocks gather the next minibatch
    if (!ga_packable(w1.ga) || !ga_packable(w2.ga) || ga_grid(w1.ga) != w1.grid || ga_grid(w2.ga) != w2.grid) return hipErrorInvalidValue;
    PVAE_LAUNCH((wgrad_pair_kernel<EpiW>), dim3(w1.grid + w2.grid + w1.nbias + w2.nbias + adam_blocks(ad) + sa.rows_pad),
                dim3(256), st, PVAE_GA2_PASS(w1.ga, w2.ga), adam_blocks(ad), e1, e2, sa, ad ? *ad : AdamPair());
    return hipGetLastError();
}
// the same with problem 1's X gathered (XSrc) -- a stack's first layer; nothing to stage then
template <class EpiW>
inline hipError_t gemm_wgrad_pair_gather(const float* dZ1, int ldz1, const XSrc& xs, int N1, int Kin1, const EpiW& e1, int M,
                                         hipStream_t st, const AdamPair* ad = nullptr, const TouchRuns* touch = nullptr) {
    WgradPlan w1 = plan_wgrad(dZ1, ldz1, nullptr, 0, N1, Kin1, M);
    if (!ga_packable(w1.ga) || ga_grid(w1.ga) != w1.grid || !gather_packable(xs) || xs.ld1 < 0 || xs.ld1 >= 65536 || xs.n1 < 0 ||
        xs.n1 >= 65536)
        return hipErrorInvalidValue;
    w1.ga.krot = (xs.rm.seg ? 1 : 0) | (xs.ind1 ? 2 : 0);
    TouchRuns tr;
    memset(&tr, 0, sizeof(tr));
    if (touch) tr = *touch;
    const float* s1 = xs.n1 > 0 ? xs.s1 : xs.s0;                 // (never dereferenced for a value when n1 == 0, but always an address)
    PVAE_LAUNCH((wgrad_pair_gather_kernel<EpiW>), dim3(w1.grid + w1.nbias + adam_blocks(ad) + tr.blocks), dim3(256), st,
                w1.ga.Q, xs.s0, s1, ga_pack_ld(w1.ga), ga_pack_t(w1.ga), ga_pack_k(w1.ga), (unsigned)xs.ld0 | ((unsigned)xs.n0 << 16),
                (unsigned)xs.ld1 | ((unsigned)xs.n1 << 16), (unsigned)(xs.rows - 1) | ((unsigned)(xs.rm.q1 - 1) << 16), xs.rm.b0, xs.rm.b1,
                adam_blocks(ad), e1, ad ? *ad : AdamPair(), tr, xs);
    return hipGetLastError();
}
// input gradient (16x16 / 32x32 tiles, caller's epilogue) || weight gradient on the gathered X
template <class EpiD, class EpiW>
inline hipError_t gemm_bwd_pair_epi_gather(const float* dZd, int ldzd, const float* Wd, int ldwd, int Md, int Kind, int Nd,
                                           const EpiD& ed, const float* dZw, int ldzw, const XSrc& xs, int Nw, int Kinw,
                                           int Mw, const EpiW& ew, hipStream_t st, const AdamPair* ad = nullptr) {
    const TilePlan d = plan_dgrad(dZd, ldzd, Wd, ldwd, Md, Kind, Nd);
    const WgradPlan w = plan_wgrad(dZw, ldzw, nullptr, 0, Nw, Kinw, Mw);
    if (!ga_packable(d.ga) || !ga_packable(w.ga) || ga_grid(d.ga) != d.grid || ga_grid(w.ga) != w.grid) return hipErrorInvalidValue;
    const PGather ps{xs};
    PVAE_LAUNCH((bwd_pair_gather_kernel<EpiD, EpiW, PGather>), dim3(d.grid + w.grid + w.nbias + adam_blocks(ad)), dim3(256), st,
                PVAE_GA2_PASS(d.ga, w.ga), ed, ew, ad ? *ad : AdamPair(), ps);
    return hipGetLastError();
}
// one launch: dX'[M][Kin'] = (dZ'[M][N'] W'[N'][Kin']) .* mask   ||   G[N][Kin] = dZ[M][N]^T X[M][Kin]
template <class EpiD, class EpiW>
inline hipError_t gemm_bwd_pair_epi(const float* dZd, int ldzd, const float* Wd, int ldwd, int Md, int Kind, int Nd,
                                    const EpiD& ed, const float* dZw, int ldzw, const float* Xw, int ldxw, int Nw,
                                    int Kinw, int Mw, const EpiW& ew, hipStream_t st, const AdamPair* ad = nullptr) {
    constexpr bool kPair64 = std::is_same<EpiD, EpiMask>::value;      // hidden-layer input gradient at >= 512 rows
    const TilePlan d = plan_tiles(TileRule{false, kPair64, TileRule::kDgrad}, dZd, ldzd, Wd, ldwd, Md, Kind, Nd);
    const WgradPlan w = plan_wgrad(dZw, ldzw, Xw, ldxw, Nw, Kinw, Mw);
    if (!ga_packable(d.ga) || !ga_packable(w.ga) || ga_grid(d.ga) != d.grid || ga_grid(w.ga) != w.grid) return hipErrorInvalidValue;
    const dim3 grid(d.grid + w.grid + w.nbias + adam_blocks(ad));
    if constexpr (kPair64) {
        if (d.geom == kTile64x32) {
            PVAE_LAUNCH((bwd_pair64_kernel<EpiD, EpiW>), grid, dim3(256), st, PVAE_GA2_PASS(d.ga, w.ga), ed, ew, ad ? *ad : AdamPair());
            return hipGetLastError();
        }
    }
    PVAE_LAUNCH((bwd_pair_kernel<EpiD, EpiW>), grid, dim3(256), st, PVAE_GA2_PASS(d.ga, w.ga), ed, ew, ad ? *ad : AdamPair());
    return hipGetLastError();
}
template <class EpiW>
inline hipError_t gemm_bwd_pair(const float* dZd, int ldzd, const float* Wd, int ldwd, const float* mask, int ldm,
                                float* dXd, int ldod, int Md, int Kind, int Nd,
                                const float* dZw, int ldzw, const float* Xw, int ldxw, int Nw, int Kinw, int Mw,
                                const EpiW& ew, hipStream_t st, const AdamPair* ad = nullptr, int act = 1) {
    const EpiMask ed{dXd, ldod, mask, ldm, act};
    return gemm_bwd_pair_epi(dZd, ldzd, Wd, ldwd, Md, Kind, Nd, ed, dZw, ldzw, Xw, ldxw, Nw, Kinw, Mw, ew, st, ad);
}
}  // namespace pvae
