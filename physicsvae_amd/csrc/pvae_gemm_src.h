// pvae_gemm_src.h -- operand sources: the gathered first-layer input as the Q operand of the wave-specialised forward
// bodies (with the Pro patches) and as the P operand of the weight-gradient bodies.
#pragma once
#include "pvae_gemm_common.h"

namespace pvae {
// ---------------------------------------------------------------------------------------
// First layers that read the demonstration set where it lies (the torch.cat sites tpv:377, rmt:829, 842
// as address arithmetic inside the loaders).  The input of a stack's first layer is a VIRTUAL matrix
//     X[q][k] = s0[row(q) * ld0 + k]                               k <  n0        (rows of `states`: s_t, or [s_t | s_{t+1}])
//             = s1[(ind1 ? row(q) : q) * ld1 + (k - n0)]      n0 <= k <  n0 + n1   (a_t rows of `actions`, or a z / a_hat panel)
//             = 0                                              elsewhere, and for q >= rows
// never materialised: the forward kernels' loaders fetch every 16-byte chunk of a Q tile from the source that holds it
// (LDS-DMA from 4-byte-aligned addresses lands at the aligned rate: tools/unaligned_probe.hip) and the weight-gradient
// bodies do the same through registers, zeroing what lies beyond the valid columns exactly.  The sources must be
// readable 16 bytes past their last element (pvae_bind_dataset checks the allocations).
// ---------------------------------------------------------------------------------------
// Which row of the demonstration set batch row q reads.  A minibatch is a run of consecutive windows, and window -> row is
// the identity plus a jump at every episode end: with at most one jump inside the minibatch the map is two (base, start)
// pairs that travel as kernel arguments (the host keeps a copy of `window_row` from bind time) -- no index load in front of
// the first tile fetch of the launch.  Otherwise: the index array itself.
struct RowMap {
    const int32_t* row;           // window_row + first_window (host side only: not read by the kernels)
    int seg, q1, b0, b1;          // rows q < q1 read row b0 + q, the others b1 + (q - q1); seg = 0: more than one jump --
                                  // such a minibatch (episodes shorter than the batch) takes the staging launch instead
    __device__ inline int at(int q) const { return q < q1 ? b0 + q : b1 + (q - q1); }   // (pure arithmetic: no load, no branch)
};
struct XSrc {
    const float* s0; int ld0, n0;
    const float* s1; int ld1, n1;
    int ind1;                     // 1: s1 is row-indirect like s0 (a_t rows of `actions`); 0: s1 row = batch row (a panel)
    RowMap rm;
    int rows;
    const float* zero;            // >= 256 zero bytes
};
// Q-operand policies of the wave-specialised forward kernels: where lane-slot (row q, 16-byte chunk at column c4) of
// k-tile kt comes from.  QDense: the panel Q[q][ldq] (every launch but a gathered first layer).
struct QDense {
    static constexpr bool kAlwaysFast = true;
    struct Base { const float* p; };
    __device__ inline Base base(const float* Q, int ldq, int q, int c4) const { return Base{Q + (size_t)q * ldq + c4}; }
    __device__ inline bool fast(int) const { return true; }
    __device__ inline const float* tile_fast(const Base& b, int kt) const { return b.p + (size_t)kt * 64; }
    __device__ inline const float* tile(const Base& b, int kt) const { return b.p + (size_t)kt * 64; }
};
// QGather: the virtual matrix above.  Its s0 run -- base pointer, row stride, width, the batch's rows as two (base, start)
// runs -- travels in the kernel's leading scalar arguments, which gfx950 preloads into SGPRs: the k-tiles that lie wholly
// inside [0, n0) (`fast`) are fetched without waiting for anything else.  The rest (`x`: the s1 block, the zero line, the
// index array for a minibatch with more than one episode jump) arrives by s_load while those tiles are in flight and is
// first touched by a tile that needs it.  A chunk that straddles n0 (n0 % 4 != 0) comes from s0 with the first floats of
// what follows the row in memory behind it: the launch's Pro patch overwrites those columns (n1 > 0 stacks), or they meet
// W's zero pad columns (n1 == 0); likewise the floats past n0 + n1.  Rows past the batch re-read the batch's last row
// (their outputs are never used and their gradient rows are zero).  Forward only: garbage x 0 = 0, a gradient would not.
struct QGather {
    static constexpr bool kAlwaysFast = false;
    const float* s0; int ld0, n0, rows, q1, b0, b1, seg;
    XSrc x;
    struct Base { const float* p0; int c4, q, r; };
    __device__ inline Base base(const float*, int, int q, int c4) const {
        Base b;
        b.q = q < rows ? q : rows - 1;
        b.r = b.q < q1 ? b0 + b.q : b1 + (b.q - q1);
        b.c4 = c4;
        b.p0 = s0 + (size_t)b.r * ld0 + c4;
        return b;
    }
    __device__ inline bool fast(int kt) const { return (kt + 1) * 64 <= n0; }              // (uniform: a scalar branch)
    __device__ inline const float* tile_fast(const Base& b, int kt) const { return b.p0 + kt * 64; }
    __device__ inline const float* tile(const Base& b, int kt) const {
        const int k0 = b.c4 + kt * 64, j = k0 - n0;
        if (k0 < n0) return b.p0 + kt * 64;
        return j < x.n1 ? x.s1 + (size_t)(x.ind1 ? b.r : b.q) * x.ld1 + j : x.zero + (b.c4 & 60);
    }
};
// the leading (preloadable) arguments of the gathered forward kernels: 14 dwords
#define PVAE_GG_PARAMS const float* g_s0, const float* g_P, int g_ld0n0, int g_ldp, int g_K, int g_tq, int g_tp, int g_ppx, int g_fl, \
                       int g_rq1, int g_b0, int g_b1
#define PVAE_GG_GA GemmArgs{nullptr, 0, g_P, g_ldp, g_K, g_tq, g_tp, g_ppx, g_fl & 7, (g_fl >> 3) & 1, (g_fl >> 4) & 1, (g_fl >> 5) & 1}
#define PVAE_GG_QS(xs) QGather{g_s0, g_ld0n0 & 0xffff, (int)((unsigned)g_ld0n0 >> 16), (g_rq1 & 0xffff) + 1, (int)((unsigned)g_rq1 >> 16) + 1, \
                               g_b0, g_b1, (g_fl >> 6) & 1, xs}

// Prologue hook of the wave-specialised kernel: a launch can OWN some columns of its Q operand -- form them itself
// instead of reading what a separate launch stored.  The compute waves `prepare` (request the inputs of those
// values for the workgroup's 32 rows: the loads travel while the first k-tiles are contracted) and `patch` the
// values over the tile image of every k-tile that holds such columns, right after that tile has landed and before
// its fragments are read (one extra workgroup barrier per patched tile; whatever the DMA brought for those columns
// is overwritten); `publish` runs behind that barrier.  NoPro: nothing of this exists in the instantiation.  The one user is the decoder's first layer, whose input [s1 | z] carries the
// sampler's z = mu + eps exp(logvar / 2) (ProSampler in pvae.hip: the sampler launch disappears).
struct NoPro {
    static constexpr bool kActive = false;
    static constexpr int kScratchFloats = 4;
    struct State {};
    __device__ inline bool needs(int) const { return false; }
    __device__ inline State prepare(int, int) const { return State(); }
    __device__ inline void patch(float*, float*, State&, int, int, int, int, int) const {}
    __device__ inline void publish(const float*, int, int, int, int) const {}
};

// Pro patch that COPIES columns [c0, c0 + n) of the Q tile from a second source (the world model's first layer on the
// gathered operand: [s_t | a_t] with a_t a row of `actions`, or [s_t | a_hat] with a_hat the decoder's output panel).
// The loaders bring the s_t columns straight from `states`; the chunk that straddles c0 (dim_body % 4 != 0) arrives with
// foreign floats behind s_t's last one, and this patch overwrites all n columns after the tile has landed.
struct ProCols {
    static constexpr bool kActive = true;
    static constexpr int kMaxN = 96, kScratchFloats = 4;
    static constexpr int kPer = 32 * kMaxN / 256;          // elements per thread at n = kMaxN
    const float* src; int ld, ind;                         // value (q, j) = src[(ind ? rm.at(q) : q) * ld + j]
    RowMap rm;
    int c0, n, rows;
    struct State { float v[kPer]; };
    __device__ inline bool needs(int t) const { return t >= (c0 >> 6) && t <= ((c0 + n - 1) >> 6); }
    __device__ inline State prepare(int q0, int tid) const {
        State st;
        const float* __restrict__ s_ = src;
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int e = tid + 256 * u, r = e / n, j = e - r * n, q = q0 + r;
            const bool live = e < 32 * n && q < rows;
            st.v[u] = live ? s_[(size_t)(ind ? rm.at(q) : q) * ld + j] : 0.f;
        }
        return st;
    }
    __device__ inline void patch(float* tile, float*, State& st, int t, int, int, int, int tid) const {
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int e = tid + 256 * u;
            if (e >= 32 * n) break;
            const int r = e / n, c = c0 + (e - r * n);
            if ((c >> 6) != t) continue;
            const int kc = c & 63;
            tile[r * 64 + (((kc >> 2) ^ (r & 15)) << 2) + (kc & 3)] = st.v[u];
        }
    }
    __device__ inline void publish(const float*, int, int, int, int) const {}
};

// ---- the gathered operand (XSrc) as the P = X operand of a weight-gradient body --------------------------------
// A lane owns U 16-byte chunks per k-tile: columns k0 .. k0 + 3 of batch row t * BKR + row.  Every chunk is fetched with
// TWO loads -- from the s0 row and from the s1 row (a zero line where the chunk has nothing from that source) -- and the
// elements are selected by masks that do not depend on the tile: branch-free, so hipcc's wait counts stay exact, and
// what lies beyond the valid columns is exactly zero (a gradient, unlike a forward product, must not see garbage there:
// it would move W's pad columns off zero).  The chunk that straddles n0 takes its tail from the START of the s1 row,
// shifted by n0 - k0 elements.  Row indices for the load D calls ahead are fetched BEFORE this call's data, so waiting
// for them never waits for younger data (loads retire in order).
struct PDense { static constexpr bool kGather = false; };
struct PGather { static constexpr bool kGather = true; XSrc x; };
template <int U, int BKR, int D>
struct XLanes {
    int k0[U], row[U];            // (everything else is recomputed per load from these and the wave-uniform descriptor:
                                  //  the weight-gradient bodies sit at the edge of three waves per SIMD)
    __device__ inline void set(const XSrc&, int u, int row_, int k0_) { k0[u] = k0_; row[u] = row_; }
    __device__ inline void fetch(const XSrc&, int, int) {}
    // the chunks of tile t (t_next, s: unused -- the row map is arithmetic for a minibatch with at most one episode jump;
    // otherwise an index load precedes the data, which only the rare minibatch with several jumps pays)
    __device__ inline void load(const XSrc& x, int t, int, int, v4f (&out)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int rr = t * BKR + row[u], k = k0[u];
            const bool valid = rr < x.rows;
            const int rc = valid ? rr : x.rows - 1;
            const int i0 = x.rm.at(rc), i1 = x.ind1 ? i0 : rc;
            const bool has0 = k < x.n0, has1 = k + 3 >= x.n0 && k < x.n0 + x.n1;
            const int d = has0 ? x.n0 - k : 0;                             // 1 .. 3 in the chunk that straddles n0, else 0 or >= 4
            // (always an address inside the row: what a source does not contribute, and every row past the batch, is masked below)
            const float* pa = x.s0 + (size_t)i0 * x.ld0 + (has0 ? k : 0);
            const float* pb = x.s1 + (size_t)i1 * x.ld1 + (has1 && k > x.n0 ? k - x.n0 : 0);
            const v4f a = *reinterpret_cast<const v4f*>(pa);
            const v4f w = *reinterpret_cast<const v4f*>(pb);
            v4f ws;                                                        // w shifted right by d elements (d < 4)
            ws[0] = d == 0 ? w[0] : 0.f;
            ws[1] = d == 0 ? w[1] : (d == 1 ? w[0] : 0.f);
            ws[2] = d == 0 ? w[2] : (d == 1 ? w[1] : (d == 2 ? w[0] : 0.f));
            ws[3] = d == 0 ? w[3] : (d == 1 ? w[2] : (d == 2 ? w[1] : w[0]));
#pragma unroll
            for (int e = 0; e < 4; ++e)
                out[u][e] = !valid ? 0.f : (k + e < x.n0 ? a[e] : (k + e < x.n0 + x.n1 ? ws[e] : 0.f));
        }
    }
};
}  // namespace pvae
