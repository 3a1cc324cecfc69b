// pvae_internal.h -- what the translation units of libpvae_gfx950.so share: error handling, the optional per-launch
// profiler, the run-time RCCL binding, the context, Philox, and the few functions one unit calls in another.
//   pvae.hip                 the context: layout queries, lifecycle, options, bindings, minibatch staging, pvae_read_tensor
//   pvae_net.hip             one stack: forward launches, the sampler, the backward plan (one function per schedule, on BwdNet
//                            below) and its deferred-Adam hand-over
//   pvae_step.hip            the training step at lookahead 1 and the step's C ABI (direct, prefetch and data-parallel steps)
//   pvae_lookahead.hip       the training step at lookahead > 1 (the multi-step unroll)
//   pvae_infer.hip           rollout and inference, the autograd entry points, the PPO learner's hooks into a stack
//   pvae_imagine.hip         imagined rollouts: the H-step closed-loop unroll of policy and world model, its hand-over launch
//   pvae_plan.hip            planning over imagined rollouts: sampled candidate codes, per-row cost in the hand-over, selection
//   pvae_refine.hip          backpropagation through the unroll (state tape, per-step recompute, the backward hand-over) and
//                            gradient refinement of a plan: Adam on the codes, keeping the best iterate
//   pvae_exchange.hip        data-parallel exchange: RCCL calls, the peer-mapped exchange kernels, their set-up and self-test;
//                            the set-up of the PPO learners' gradient exchange between workers
//   pvae_rollout_server.hip  the call-persistent rollout server
//   pvae_probe.hip           measurement entry points (clock probe, profiler read-out, contraction probe)
//   pvae_fc.hip              the stack set, and what its PPO learner runs of it: the model adapter of pvae_ppo_learner.h
//   pvae_ppo_core.hip        the PPO learner's model-independent kernels, launches and checks (loss head, Adam + stats and its
//                            two-halves and exchanged forms, evaluate epilogue, pad copy, zero rows, GAE, minibatch order),
//                            pvae_ppo_loss, pvae_gae and pvae_ppo_order
//   pvae_ppo.hip             what PhysicsVAE's PPO learner runs of pvae_infer.hip and pvae_fc.hip: its model adapter
//   pvae_ppo_learner.h       the PPO learner's host driver, once for both models: step, sgd loop, the two halves, exchange set-up,
//                            evaluate, prepare and act, as function templates over a unit's model adapter
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "pvae_gemm.h"
#include "pvae_layout.h"

using namespace pvae;

// ---------------------------------------------------------------------------------------
// error handling
// ---------------------------------------------------------------------------------------
inline thread_local char g_err[512] = "";

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) return fail(-10, "%s: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

// ---------------------------------------------------------------------------------------
// optional per-launch timing (HIP events on the launch stream)
// ---------------------------------------------------------------------------------------
struct Profiler {
    bool on = false;
    static constexpr int kMax = 8192;
    hipEvent_t ev[kMax][2];
    int cat[kMax];
    double flops[kMax];
    int n = 0, created = 0;
    // begin() arms the slot's event pair; the launch wrapper (PVAE_LAUNCH, pvae_gemm.h) hands it to
    // hipExtLaunchKernelGGL, so the pair brackets the kernel itself and not the launch seam.  Every
    // profiled range holds exactly one launch; a range that launched nothing is dropped.
    int begin(int category, double fl, hipStream_t) {
        if (!on || n >= kMax) return -1;
        if (n >= created) {
            if (hipEventCreate(&ev[n][0]) != hipSuccess || hipEventCreate(&ev[n][1]) != hipSuccess) return -1;
            created = n + 1;
        }
        cat[n] = category;
        flops[n] = fl;
        g_kernel_ev[0] = ev[n][0];
        g_kernel_ev[1] = ev[n][1];
        return n;
    }
    void end(int slot, hipStream_t) {
        if (slot < 0) return;
        if (!g_kernel_ev[0]) n = slot + 1;          // consumed by a launch
        g_kernel_ev[0] = g_kernel_ev[1] = nullptr;
    }
    // a range that is not one of our launches (the RCCL collective): events recorded on the stream
    // around the call; `fl` carries the payload bytes instead of flops
    int begin_range(int category, double fl, hipStream_t st) {
        if (!on || n >= kMax) return -1;
        if (n >= created) {
            if (hipEventCreate(&ev[n][0]) != hipSuccess || hipEventCreate(&ev[n][1]) != hipSuccess) return -1;
            created = n + 1;
        }
        cat[n] = category;
        flops[n] = fl;
        if (hipEventRecord(ev[n][0], st) != hipSuccess) return -1;
        return n;
    }
    void end_range(int slot, hipStream_t st) {
        if (slot < 0) return;
        if (hipEventRecord(ev[slot][1], st) == hipSuccess) n = slot + 1;
    }
};
inline Profiler g_prof;

// ---------------------------------------------------------------------------------------
// RCCL, resolved at run time.  PyTorch-ROCm ships its own librccl.so.1 and has it loaded; the
// library binds to THAT instance (RTLD_NOLOAD first) instead of linking a second copy, and
// falls back to the system one (/opt/rocm/lib) when used without torch.  Only the five entry
// points of the data-parallel exchange are needed; prototypes as in rccl/rccl.h (2.2x).
// ---------------------------------------------------------------------------------------
struct RcclId { char internal[128]; };                 // ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128)
struct Rccl {
    void* h = nullptr;
    int (*GetUniqueId)(RcclId*) = nullptr;
    int (*CommInitRank)(void**, int, RcclId, int) = nullptr;          // id is passed BY VALUE
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*ReduceScatter)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;   // optional
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;            // optional
    int (*CommDestroy)(void*) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    int (*CommUserRank)(void*, int*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok() const { return h && GetUniqueId && CommInitRank && AllReduce && CommDestroy && GetErrorString; }
};
inline Rccl g_rccl;
enum { kNcclSum = 0, kNcclFloat32 = 7 };

inline int rccl_load() {
    if (g_rccl.ok()) return 0;
    const char* names[] = {"librccl.so.1", "librccl.so"};
    void* h = nullptr;
    for (const char* n : names)
        if ((h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;            // the instance torch already mapped
    if (!h)
        for (const char* n : names)
            if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return fail(-20, "RCCL not found (librccl.so.1): %s", dlerror());
    g_rccl.h = h;
    g_rccl.GetUniqueId = (int (*)(RcclId*))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(void**, int, RcclId, int))dlsym(h, "ncclCommInitRank");
    g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclAllReduce");
    g_rccl.ReduceScatter = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclReduceScatter");
    g_rccl.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
    g_rccl.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    g_rccl.CommCount = (int (*)(void*, int*))dlsym(h, "ncclCommCount");           // optional (pvae_comm_info)
    g_rccl.CommUserRank = (int (*)(void*, int*))dlsym(h, "ncclCommUserRank");
    g_rccl.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.ok()) {
        g_rccl = Rccl();
        return fail(-20, "RCCL library lacks an expected symbol");
    }
    return 0;
}
#define RCCL_TRY(expr)                                                                        \
    do {                                                                                      \
        int r_ = (expr);                                                                      \
        if (r_ != 0) return fail(-21, "%s: %s", #expr, g_rccl.GetErrorString(r_));            \
    } while (0)

// ---- the PPO learners' peer-mapped gradient exchange: its state (functions: below, "the PPO learner") ----
// A learner's exchange state: every rank's gradient arena(s) and flag block mapped into this process (index = rank;
// [rank] = the local pointers).  Parameters and moments are NOT mapped: every rank reads all gradients and updates its own
// replica whole.  Flag block: [0, 8) ready[src], [8, 16) done[src], 16 ticket, 17 waits that gave up, [32, 64) the attach-time
// check's tokens, then from word kPpoPeerLs the k floats of this rank's log-std gradient, where the peers read them.
// Word 18: this rank's clip coefficient of the step in flight, a float (a clip bound: PpoClip).
constexpr int kPpoPeerReady = 0, kPpoPeerDone = 8, kPpoPeerTicket = 16, kPpoPeerErr = 17, kPpoPeerCoef = 18, kPpoPeerSelf = 32, kPpoPeerGradA = 40,
              kPpoPeerGradB = 48, kPpoPeerFin = 56, kPpoPeerPayload = 64, kPpoPeerLs = 256;
constexpr int kPpoPeerArenas = 2;                // a stack set has one gradient arena, PhysicsVAE two (its own + the value stack set's)
struct PpoPeers {
    bool open = false;
    int rank = 0, world = 0, n_arenas = 0, k = 0;
    unsigned* flags = nullptr;                               // own flag block (hipExtMallocWithFlags, uncached)
    size_t flag_bytes = 0;
    unsigned* peer_flags[PVAE_P2P_MAX_RANKS] = {};
    float* arena[kPpoPeerArenas][PVAE_P2P_MAX_RANKS] = {};   // gradient arenas
    long long floats[kPpoPeerArenas] = {};
    void* mapped[PVAE_P2P_MAX_RANKS][kPpoPeerArenas + 1] = {};   // what hipIpcOpenMemHandle returned (to close)
    unsigned epoch = 0;                                      // exchanged launches issued so far (identical on every rank)
    unsigned selftests = 0;
    float* self_buf = nullptr;                               // the attach-time check's saved gradient line
};

// Learner diagnostics (include/pvae.h "Learner diagnostics"): what *_ppo_diag bound -- `out` [capacity][PVAE_PPO_DIAG] rows
// of the caller's, and the scratch cut in two: `gslot`, one double per workgroup of an Adam launch (the sum of squares
// of the gradient values it loaded; the launch's extra workgroup: the log-std vector's), and `dpart`, the loss head's
// diagnostics partial rows.  `out` null: nothing bound, every launch below runs its instantiation without diagnostics.
// A PpoDiagRow names the row one step writes.  The norm is finished by ONE SMALL LAUNCH PER STEP (ppo_gnorm_launch): the
// Adam launch's extra workgroup runs beside the others and cannot wait for their slots.
constexpr int kDiagPart = 8;                    // floats of a diagnostics partial row: 2 counts, 1 max, 4 pivoted sums, 1 spare
constexpr int kDiagSlots = 2056;                // >= the largest Adam grid (2048 + 1), a multiple of 8
struct PpoDiag {
    float* out = nullptr; int capacity = 0;
    double* gslot = nullptr; float* dpart = nullptr;
};
struct PpoDiagRow { float* row; double* gslot; float* dpart; };
inline PpoDiagRow diag_row(const PpoDiag& d, long long step) {
    return d.out ? PpoDiagRow{d.out + step * PVAE_PPO_DIAG, d.gslot, d.dpart} : PpoDiagRow{nullptr, nullptr, nullptr};
}

// Gradient clipping (include/pvae.h "Gradient clipping inside the PPO learners"): what *_ppo_grad_clip bound -- the
// threshold and the scratch, one double per workgroup of the sum-of-squares launch that goes between the backward and the
// Adam launch.  `slot` null: nothing bound, every launch runs its instantiation without a clip.  Not the diagnostics'
// gslot: the Adam launch writes that one later.  The launch's grid is at most kClipGrid workgroups over the segments + the
// log-std vector's: every workgroup of the Adam launch behind it (up to 2049) adds ALL slots again, one wave, four loads
// per lane at 256 slots, while 255 workgroups of 256 threads already put a wave on every SIMD of the device for the read.
constexpr int kClipGrid = 255;
constexpr int kClipSlots = 256;
struct PpoClip {
    float max_norm = 0.f;
    double* slot = nullptr;
};

// What a PPO learner keeps, whichever model it trains (the stack set: in pvae_fc; PhysicsVAE: pvae_ctx::ppo): what *_ppo_bind
// bound, the launch counts of the last calls, the exchange and the diagnostics binding.  Its host driver: pvae_ppo_learner.h.
struct PpoLearner {
    float* grad = nullptr; float* m = nullptr; float* v = nullptr;
    float* scratch = nullptr;
    float* log_std = nullptr; float* log_std_m = nullptr; float* log_std_v = nullptr;
    int launches = 0;                                    // *_ppo_launches
    int eval_launches = 0, gae_launches = 0;             // *_gae_launches
    PpoPeers peers;                                      // gradient exchange between workers (*_ppo_peer_*)
    PpoDiag diag;                                        // learner diagnostics (*_ppo_diag)
    PpoClip clip;                                        // gradient clipping (*_ppo_grad_clip)
};

struct pvae_ctx {
    void* comm = nullptr;        // ncclComm_t of the data-parallel group (pvae_comm_init)
    int comm_rank = 0, comm_world = 1;
    // overlapped gradient exchange (pvae_dp_train_step): the buckets of a stack are reduced and
    // applied on comm_stream while the compute stream keeps producing the next ones
    hipStream_t comm_stream = nullptr;
    static constexpr int kMaxBuckets = 64;
    hipEvent_t bucket_ready[kMaxBuckets] = {};
    hipEvent_t comm_done = nullptr;
    int exchange_mode = 0;             // PVAE_EXCHANGE_*: all-reduce + replicated Adam, or sharded (ZeRO-1 shaped)
    int64_t bucket_bytes = -1;         // > 0: bucketed + overlapped; 0: one bucket per stack, in line on the compute
                                       // stream; -1 (default): chosen per step by auto_bucket_bytes()
    int64_t bucket_bytes_now = 0;      // what the step in flight uses (exchange_buckets / dp_train_step)
    int comm_test_delay_us = 0;        // tests: a spin kernel in front of every reduction
    Layout L;
    Workspace W;
    float* params = nullptr;
    float* grads = nullptr;
    float* m = nullptr;
    float* v = nullptr;
    float* ws = nullptr;
    const float* states = nullptr;
    const float* next_states = nullptr;      // pvae_bind_dataset_next (null: next row of `states`)
    const float* actions = nullptr;
    const int32_t* window_row = nullptr;
    int64_t n_rows = 0, n_windows = 0;
    int staged_rows = 0;
    double staged_rows_f = 0;    // rows of the batch being processed (for the profiler's flop count)
    // First layers on the demonstration set where it lies (XSrc in pvae_gemm.h): the training-step entry
    // points (pvae_train_step, _prefetch, pvae_dp_train_step) stage nothing when `direct_ok` holds -- the first layer of
    // every stack gathers its rows of `states` / `actions` itself, the two targets are read from there by the loss
    // epilogues.  pvae_gather / pvae_set_batch + pvae_forward_backward keep the panel path (inspection, explicit batches,
    // lookahead > 1, evaluation, the other priors).  OPT-IN (pvae_set_direct(ctx, 1)): bit-identical to the staged step,
    // but at 256 rows the staged step is the faster one -- its gather rides in the previous step's last launch for free,
    // while the gathered layer-0 weight gradients assemble every chunk of X from two unaligned loads and a select in the
    // launch that also carries the Adam epilogue: joint 250.0 vs 240.3 us, world 92.2 vs 86.6 (docs/experiments.md, round 5).
    bool direct = false;
    bool data_slack = false;     // both dataset arrays are readable 16 bytes past their last row (checked at bind time)
    struct { bool on = false; RowMap rm{}; } dx;                     // the step in flight: batch row -> row of the set
    TouchRuns next_touch{};                                          // rows of the NEXT minibatch for the last launch to pre-touch
    std::vector<int32_t> window_row_host;                            // copied at bind time: the host finds the episode jumps
    bool pair_launch = true;     // PVAE_PAIR=0 launches every contraction on its own (A/B)
    // gather prefetch (pvae_train_step_prefetch): what the alternate staging panels hold, and the
    // staging job the current step's last launch should carry
    struct { bool valid = false; int64_t first = 0; int rows = 0; const float* states = nullptr; } pf;
    StageArgs next_stage;        // rows_pad > 0: pending for the last launch of this step
    bool next_carried = false;   // set by the launch that took it
    bool seed_pads_clean = false;  // pad columns of the seed panels zeroed (see plan_backward)
    bool grad_accum = false;       // pvae_net_backward(accumulate = 1): the plan's gradient stores add into the arena
    // deferred Adam (AdamSeg, pvae_gemm.h): the layer whose gradient the last launch stored; the next
    // weight-gradient launch of the step updates it with extra workgroups (PVAE_DEFER_ADAM=0: off)
    AdamSeg pending_adam;          // the most recent one
    AdamSeg held_adam;             // a big one that a narrow launch passed on to the next wide launch (take_pending)
    bool defer_adam = true;
    bool same_layer_pairs = true;  // PVAE_SAME_LAYER=0: wgrad_i rides with dgrad_{i-1} as before (A/B)
    bool p2p_selftest_flags_only = false;   // option: the attach-time self-test skips the cached-arena part
    int server_mailbox = 0;                 // option: where the rollout server's request block lives (0 auto, 1 host, 2 device)
    bool joint_s_rec = false;      // option "joint_s_rec": the joint phase runs with world_model_s_rec_coeff != 0 (default: refused, -4)
    bool ppo_priors = false;       // option "ppo_priors": the PPO passes run under the learned and the sphere prior (default: refused, -1)
    bool fold_sampler = true;      // the sampler runs as the prologue of the decoder's first-layer launch (PVAE_FOLD_SAMPLER=0: its own launch)
                                   // (ProSampler).  Off by default: one launch less, but the step is not shorter -- the kernel
                                   // trace shows 6.4-7.0 us for the merged launch against 4.4 + 4.6, and the un-profiled
                                   // step 254.8 vs 254.5 us (profiles/r03_ab_fold_sampler.txt, docs/experiments.md)
    // peer-mapped exchange (PVAE_EXCHANGE_P2P): every rank's gradient arena, parameter arena and flag block,
    // mapped into this process with hipIpcOpenMemHandle (index = rank; [rank] = the local pointers)
    struct P2p {
        bool open = false;
        int rank = 0, world = 0;
        unsigned* flags = nullptr;                       // own flag block (uncached device memory)
        float* grads[PVAE_P2P_MAX_RANKS] = {};
        float* params[PVAE_P2P_MAX_RANKS] = {};
        unsigned* peer_flags[PVAE_P2P_MAX_RANKS] = {};
        float* staging = nullptr;                        // own staging buffer of the push form (hipMalloc, arena-sized)
        float* peer_staging[PVAE_P2P_MAX_RANKS] = {};
        void* mapped[PVAE_P2P_MAX_RANKS][4] = {};        // what hipIpcOpenMemHandle returned (to close)
        unsigned epoch = 0;                              // exchanges issued so far (identical on every rank)
        float* self_buf = nullptr;                       // self-test scratch: saved regions + checksums (hipMalloc)
        unsigned selftests = 0;                          // self-tests run since the flags were zeroed (identical on every rank)
        long long timeout_ticks = 20ll * 100000000ll;    // 100 MHz wall clock
    } p2p;
    struct RolloutServer* server = nullptr;              // call-persistent rollout kernel (pvae_rollout_server_*)
    // every call that changes parameters through this library counts here and leaves its stream: the rollout server re-reads
    // its resident copy when the count moved (after that stream has drained)
    unsigned long long param_version = 0;
    hipStream_t param_stream = nullptr;                  // (NULL is a stream too: the default one.  The caller's stream must
                                                         //  outlive the writes it queued, as for any other call here.)
    bool param_pending = false;                          // work that writes the parameters may still be queued on it
    // PPO learner (pvae_ppo_bind): its gradient and moment arenas have the parameter arena's layout -- they are not the
    // supervised trainer's grads / m / v above --, and the value branch is a stack set of its own
    struct Ppo : PpoLearner { pvae_fc* value = nullptr; } ppo;
};
static inline void params_touched(pvae_ctx* c, hipStream_t st, bool queued = true) {
    // one stream is remembered: writes still queued on ANOTHER one are drained here (a caller that switches streams with
    // parameter writes in flight -- rare, and it costs that caller one wait -- instead of a server that reloads too early)
    if (c->param_pending && c->param_stream != st) (void)hipStreamSynchronize(c->param_stream);
    ++c->param_version; c->param_stream = st; c->param_pending = queued;
}
static inline hipError_t params_settle(pvae_ctx* c) {
    if (!c->param_pending) return hipSuccess;
    c->param_pending = false;
    return hipStreamSynchronize(c->param_stream);
}
void server_free(pvae_ctx* c);                 // pvae_rollout_server.hip


// ---------------------------------------------------------------------------------------
// Philox (the sampler of the training step, the rollout launches and the rollout server draw the same stream)
// ---------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11) -> one standard normal via Box-Muller.
__device__ inline void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
// One Philox call = four standard normals: the draws of columns 4g .. 4g + 3 of row `row` (counter = {offset, row,
// g}; two Box-Muller pairs from the four 32-bit outputs).  Hardware transcendentals (v_log_f32, v_sqrt_f32,
// v_sin_f32 / v_cos_f32, which take their argument in revolutions: cos(2 pi u) is ONE instruction): ~1 ulp, which a
// random draw does not notice, at a tenth of the instructions of logf / cosf -- the draws are formed inside a
// contraction launch by every workgroup that needs them (ProSampler below), so their cost is multiplied.
__device__ inline v4f philox_normal4(uint64_t seed, uint64_t offset, uint32_t row, uint32_t group) {
    uint32_t c[4] = {(uint32_t)offset, (uint32_t)(offset >> 32), row, group};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    v4f n;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = ((float)c[2 * h] + 0.5f) * 2.3283064365386963e-10f;       // (0, 1)
        const float u2 = ((float)c[2 * h + 1] + 0.5f) * 2.3283064365386963e-10f;
        const float r = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));   // sqrt(-2 ln u1), log2 form
        n[2 * h] = r * __builtin_amdgcn_cosf(u2);
        n[2 * h + 1] = r * __builtin_amdgcn_sinf(u2);
    }
    return n;
}
__device__ inline float philox_normal(uint64_t seed, uint64_t offset, uint32_t row, uint32_t col) {
    return philox_normal4(seed, offset, row, col >> 2)[col & 3];
}

__device__ inline float block_sum_256(float v) {
    __shared__ float red[4];
    return block_sum_256(v, red);
}

// Backward of the unit-sphere projection z = e / max(|e|, 1e-12) (sphere_kernel, pvae_net.hip) on ONE row by ONE wavefront
// (all 64 lanes call it): e, g = dz, d = de each Z floats.  Lanes stride the columns by 64, then the xor-shuffle tree from 32
// down -- the one summation order of the autograd path (sampler_bwd_kernel, pvae_infer.hip) and of the fused PPO step
// (ppo_sphere_bwd_kernel, pvae_ppo.hip), which both call this.
//   ie = 1 / max(sqrt(sum e^2), 1e-12);   zg = (sum e g) ie = <z, dz>;   de = (g - e ie zg) ie
__device__ inline void sphere_bwd_row(const float* __restrict__ e, const float* __restrict__ g, int Z, int lane,
                                      float* __restrict__ d) {
    float e2 = 0.f, eg = 0.f;
    for (int c = lane; c < Z; c += 64) { e2 += e[c] * e[c]; eg += e[c] * g[c]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { e2 += __shfl_xor(e2, o, 64); eg += __shfl_xor(eg, o, 64); }
    const float ie = 1.0f / fmaxf(sqrtf(e2), 1e-12f);
    const float zg = eg * ie;                                  // <z, dz>
    for (int c = lane; c < Z; c += 64) d[c] = (g[c] - e[c] * ie * zg) * ie;
}

// The same sampler as the PROLOGUE of the decoder's first-layer launch (pvae_gemm_ws.h, splitk_ws_pertile_body): every
// workgroup of that launch forms z for its own 32 batch rows while its first k-tile is in flight and patches it over
// the z columns of its input tile in LDS; the workgroups of column tile 0 also store z (the decoder's first-layer
// weight gradient reads it from the input panel), the draws actually used, and the KL partial of their row block.
// One launch less per joint step (the sampler launch was ~4.5 us of fixed cost for 8 K elements).
struct ProSampler {
    static constexpr bool kActive = true;
    static constexpr int kMaxZ = 64, kScratchFloats = 8;
    static constexpr int kPer = 32 * kMaxZ / 4 / 256;     // work items per thread at Z = kMaxZ
    const float* te_out; int ldte;       // encoder output [mu | logvar]
    const float* eps_in;                 // supplied draws [rows][Z], or null: Philox
    float* eps_used;                     // [rows_pad][Z]
    float* md_in; int ld_md;             // the decoder's input panel: z columns written by column tile 0
    int c0, Z, rows, noise;              // z columns = [c0, c0 + Z), Z % 4 == 0
    unsigned long long seed, offset;
    float* partial;                      // KL partial per row block (tiles_q of them), or null
    // work item = 4 consecutive z columns of one row (one Philox call, 16-byte accesses): item e of the workgroup is
    // row e / (Z/4), columns 4 (e % (Z/4)) ..; thread tid owns items tid, tid + 256, ...
    struct State { v4f mu[kPer], lv[kPer], ep[kPer], z[kPer]; bool formed; };
    __device__ inline bool needs(int t) const { return t == (c0 >> 6) || t == ((c0 + Z - 1) >> 6); }
    // request the inputs (the encoder's output was written through by the previous launch: cold fetches, which now
    // travel while the k-tiles in front of the z columns are contracted)
    __device__ inline State prepare(int q0, int tid) const {
        State st;
        const int G = Z >> 2;
        const float* __restrict__ te = te_out;
        const float* __restrict__ ei = eps_in;
        const v4f zero = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int e = tid + 256 * u;
            const int r = e / G, j = (e - r * G) * 4, q = q0 + r;
            const bool live = e < 32 * G && q < rows;
            st.mu[u] = live ? *reinterpret_cast<const v4f*>(te + (size_t)q * ldte + j) : zero;
            st.lv[u] = live ? *reinterpret_cast<const v4f*>(te + (size_t)q * ldte + Z + j) : zero;
            st.ep[u] = (live && noise && ei) ? *reinterpret_cast<const v4f*>(ei + (size_t)q * Z + j) : zero;
            st.z[u] = zero;
        }
        st.formed = false;
        return st;
    }
    // tile = the swizzled [32][64] image of k-tile t (chunk ^= row & 15, as the loaders write it)
    __device__ inline void patch(float* tile, float* scratch, State& st, int t, int q0, int tile_p, int, int tid) const {
        const int G = Z >> 2;
        if (!st.formed) {                 // first patched tile: form z, KL partial, and (column tile 0) store z and the draws
            float acc = 0.f;
#pragma unroll
            for (int u = 0; u < kPer; ++u) {
                const int e = tid + 256 * u;
                if (e >= 32 * G) break;
                const int r = e / G, j = (e - r * G) * 4, q = q0 + r;
                v4f ee = v4f{0.f, 0.f, 0.f, 0.f};
                if (q < rows) {
                    if (noise) ee = eps_in ? st.ep[u] : philox_normal4(seed, offset, q, j >> 2);
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        st.z[u][x] = __fmaf_rn(ee[x], expf(0.5f * st.lv[u][x]), st.mu[u][x]);
                        acc += -0.5f * (1.0f + st.lv[u][x] - st.mu[u][x] * st.mu[u][x] - expf(st.lv[u][x]));
                    }
                }
                if (tile_p == 0) {
#pragma unroll
                    for (int x = 0; x < 4; ++x) md_in[(size_t)q * ld_md + c0 + j + x] = st.z[u][x];      // (c0 = dim_body: unaligned)
                    *reinterpret_cast<v4f*>(eps_used + (size_t)q * Z + j) = ee;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
            if ((tid & 63) == 0) scratch[tid >> 6] = acc;
            st.formed = true;
        }
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int e = tid + 256 * u;
            if (e >= 32 * G) break;
            const int r = e / G, j = (e - r * G) * 4;
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int c = c0 + j + x;
                if ((c >> 6) != t) continue;
                const int kc = c & 63;
                tile[r * 64 + ((((kc >> 2) ^ (r & 15))) << 2) + (kc & 3)] = st.z[u][x];
            }
        }
    }
    // behind the barrier that follows the first patch: the four compute waves' KL sums are in the scratch
    __device__ inline void publish(const float* scratch, int t, int tile_p, int tile_q, int tid) const {
        if (t == (c0 >> 6) && tile_p == 0 && tid == 0 && partial)
            partial[tile_q] = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
    }
};

// ---------------------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------------------
inline AdamScalars adam_scalars(const pvae_step_params* sp, int net) {
    // torch computes the bias corrections in Python floats (double): tm:119-122 -> torch/optim/adam.py
    const int t = sp->adam_t[net] > 0 ? sp->adam_t[net] : 1;
    const double bc1 = 1.0 - std::pow(sp->beta1, t);
    const double bc2 = 1.0 - std::pow(sp->beta2, t);
    AdamScalars s;
    s.step_size = (float)(sp->lr / bc1);
    s.inv_bc2_sqrt = (float)(1.0 / std::sqrt(bc2));
    s.beta1 = (float)sp->beta1;
    s.beta2 = (float)sp->beta2;
    s.eps = (float)sp->adam_eps;
    s.one_minus_beta1 = (float)(1.0 - sp->beta1);
    s.one_minus_beta2 = (float)(1.0 - sp->beta2);
    s.weight_decay = sp->weight_decay;
    return s;
}

inline int check_ready(const pvae_ctx* c, bool need_arenas) {
    if (!c) return fail(-1, "null ctx");
    if (!c->ws) return fail(-2, "workspace not bound");
    if (need_arenas && !c->params) return fail(-2, "parameter arena not bound");
    return 0;
}


// grid of a 1-D glue launch: one thread per element in blocks of 256, at most `cap` blocks (the kernels stride)
inline int grid1d(long long n, int cap) {
    const long long g = (n + 255) / 256;
    return (int)(g < cap ? g : cap);
}

// ---------------------------------------------------------------------------------------
// the training step of PhysicsVAE: what pvae.hip, pvae_net.hip, pvae_step.hip, pvae_lookahead.hip and pvae_infer.hip
// call in one another
// ---------------------------------------------------------------------------------------
inline bool g_look_pair = true, g_rollout_fused = true;          // process-wide options "look_pair", "rollout_fused"

// ---- pvae.hip: staging ----
// Arguments of a staging job into the CURRENT (alt == false) or the alternate set of input panels; `steps`: time steps to
// stage (the ctx's lookahead for training batches, 1 for rollout inference)
StageArgs stage_args(const pvae_ctx* c, long long first_window, const float* x, const float* y, int rows, bool from_set,
                     int steps, bool alt);
int stage(pvae_ctx* c, long long first_window, const float* x, const float* y, int rows, bool from_set, hipStream_t st, int steps);
void flip_stage_panels(pvae_ctx* c);
RowMap row_map(const pvae_ctx* c, int64_t first_window, int rows);
void plan_touch(pvae_ctx* c, int64_t next_first, int next_rows);
int copy_cols_launch(const float* src, int lds_, int src_col0, float* dst, int ldd, int dst_col0, int rows, int ncols,
                     hipStream_t st);                           // dst[r][dst_col0 + c] = src[r][src_col0 + c]

// ---- pvae_net.hip: one stack ----
struct FwdTail {              // what the output layer's epilogue does besides bias
    const EpiMse* mse = nullptr;      // fused MSE loss + gradient
    float* out2 = nullptr;            // or: copy the first n2 output columns to out2[:, off2:]
    int ld2 = 0, off2 = 0, n2 = 0;
    const ProSampler* pro0 = nullptr; // layer 0 forms the sampler's z columns of its input itself (decoder, joint step)
    const XSrc* xs0 = nullptr;        // layer 0 gathers its input rows from the demonstration set (direct steps)
    const ProCols* cols0 = nullptr;   // ... and copies these columns over its input tile (world model: a_t / a_hat)
};
// `row0`: first row of the time-step block to run on (0 unless lookahead > 1)
int forward_net(pvae_ctx* c, int n, int rows_pad, hipStream_t st, const FwdTail& tail = FwdTail(), int64_t row0 = 0);
// a_hat += range * (the helper's output), also into the world model's action columns; row blocks `row0` / `wm_row0`
int helper_add_launch(pvae_ctx* c, int rows, int64_t row0, int64_t wm_row0, hipStream_t st);
int sampler_grid(const pvae_ctx* c, int rows_pad);
int64_t z_panel(const pvae_ctx* c);
int launch_sampler(pvae_ctx* c, const float* te_out, int ldte, const float* eps, float* eps_used, float* md_in, int ld_md,
                   int rows, int rows_pad, int noise, unsigned long long seed, unsigned long long offset, float* partial,
                   float* z_dense, const float* mu_p, int ldmp, hipStream_t st);
bool sampler_folds(const pvae_ctx* c, int rows);
XSrc xsrc_of(const pvae_ctx* c, int net, int phase, bool with_s1, int rows);
// ---- pvae_imagine.hip: the closed-loop unroll, shared with pvae_plan.hip ----
// What the kernels of an unroll know of the call: the input panels of row block 0 (null: the mode does not run that stack),
// the sources, and how the next step's z columns come about.
enum { kZNone = 0, kZSupplied = 1, kZDrawn = 2, kZLater = 3 };   // kZLater: prior(s_t) + n_t, formed by prior_z_kernel
struct ImagineIo {
    float* te_in; int ld_te;
    float* md_in; int ld_md;
    float* md_z;                        // the panel whose columns [Db, Db + Z) take z (z_panel(): md_in, or the side panel)
    float* wm_in; int ld_wm;
    float* pr_in; int ld_pr;
    int te_body, te_task, md_body;      // input subsets: 0 = the stack does not read that block, which stays zero
    int Db, Da, Z, rows, rows_pad, mode, zkind;
    pvae_imagine_src s0, goals, actions, z, targets;
    unsigned long long seed, offset;
};

__device__ inline const float* src_row(const pvae_imagine_src& s, int r, long long t) {
    const long long i = s.row_index ? (long long)s.row_index[r] : (long long)r;
    return s.base + i * s.ld + t * s.step;
}
// One row's cost term of step t (plan.py step 3; the hand-overs of pvae_plan.hip and pvae_refine.hip), by ONE wavefront:
//   sw_t * (sum_c cw[c] * double(d) * double(d)) / Db,   d = s[c] - tg[c] in float,
// lanes striding the columns, then the xor tree from 32 down: every lane returns the same double.
__device__ inline double rollout_cost_row(const float* __restrict__ s, const float* __restrict__ tg, const float* __restrict__ cw,
                                          const float* __restrict__ sw, int t, int Db, int lane) {
    double acc = 0.0;
    for (int c = lane; c < Db; c += 64) {
        const float d = s[c] - tg[c];
        const double q = (double)d * (double)d;
        acc += cw ? (double)cw[c] * q : q;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    return (sw ? (double)sw[t] : 1.0) * acc / (double)Db;
}
// The panels and sizes of a call on `rows` rows (sources, seed and offset are the caller's to fill in); marks the staging
// panels as overwritten, as pvae_net_forward does.
ImagineIo imagine_io(pvae_ctx* c, int mode, int zkind, int rows);
int imagine_per_step(const pvae_ctx* c, int mode, bool z_supplied);      // launches of one step, the hand-over included
// Steps t = 0 .. H - 1 on panels that hold step 0 already: per step the stacks' own launches, then `handover(t, more)`, ONE
// launch that feeds s_{t+1} and the next drive into the panels.  `eps`, `noise`, `z_out`: track mode's draws and the dense
// z result of track mode and of prior mode under the learned prior.  Adds what it enqueued to *launches.
int imagine_unroll(pvae_ctx* c, const ImagineIo& io, int H, const float* eps, int noise, float* z_out,
                   const std::function<int(int t, bool more)>& handover, hipStream_t st, int* launches);

// A backward pass is a list of stages = launches in stream order.  `ready_*` names the slice of
// the gradient arena that is final once the stage has run (data-parallel callers start that
// slice's all-reduce right away, while later stages execute).
struct Stage {
    std::function<int()> run;
    int64_t ready_off = 0, ready_cnt = 0;
    int net = -1;
};
typedef std::vector<Stage> Plan;
enum { kTakeAll = 0, kTakeSmall = 1 };
AdamPair take_pending(pvae_ctx* c, int how = kTakeAll);
int flush_pending_adam(pvae_ctx* c, hipStream_t st);
int adam_flat_launch(float* p, const float* g, float* m, float* v, long long n4, const AdamScalars& s, hipStream_t st);
// What the input-gradient launch of a stack's FIRST layer does with its result (lookahead 1):
// nothing special (store the panel), or form the gradient seed of the stack that produced those
// input columns in its epilogue (pvae_gemm.h: EpiActionSeed / EpiSamplerSeed).
// Columns [c0, c0 + n) of a first-layer input gradient, widened to whole 32-column tiles: the only
// part of that panel a gradient seed reads, so the only part its launch contracts.
struct SeedWindow { int lo, width; };
static inline SeedWindow seed_window(int c0, int n) {
    const int lo = c0 & ~31;
    return SeedWindow{lo, pad32(c0 + n) - lo};
}
struct InputSeed {
    int kind = 0;                      // 0 none, 1 action seed (world model -> decoder), 2 sampler seed (decoder -> encoder)
    EpiActionSeed a;
    EpiSamplerSeed s;
};
// A weight-gradient launch handed from one stack's plan to the next one's first input-gradient
// launch, so the two go out as ONE horizontally fused launch across the stack boundary.
struct DgradArgs {
    const float* dZ; int ldz; const float* W; int ldw; const float* mask; int ldm; float* dX; int ldo;
    int M, Kin, Nd;
    double flops;
    int act = 1;          // act_grad code of the layer behind `mask`
};
struct CarriedWgrad {
    bool valid = false;
    std::function<int(const DgradArgs&)> run_with_dgrad;
    int64_t ready_off = 0, ready_cnt = 0;
    int net = -1;
};
inline Stage& push(Plan& plan, std::function<int()> fn) {
    plan.emplace_back();
    plan.back().run = std::move(fn);
    return plan.back();
}
// a fused step may store a layer's gradient and leave its update to workgroups of a later launch (AdamSeg)
inline bool can_defer_adam(const pvae_ctx* c, bool fused) { return fused && c->defer_adam && c->grads != nullptr; }

// One stack's backward pass as both planners see it (plan_backward_net: lookahead 1; plan_backward_unrolled): the operands of
// layer i on the row block that starts at row `blk` (lookahead 1: 0; the unroll: Unroll::blk(slot)), its input-gradient
// launch, its three gradient epilogues and the choice between them, its deferred-Adam segment and its slice of the arena.
// A plain value: the stages of a plan keep a copy.
struct BwdNet {
    pvae_ctx* c;
    int n;
    const NetLayout* N;
    const NetWork* w;
    AdamScalars as;
    hipStream_t st;
    double rowsf;                  // rows of the batch (the profiler's flop counts)
    int dx0_cols = 0;              // > 0: the columns of layer 0's input gradient that anything reads (flop counts only)
    BwdNet(pvae_ctx* c_, int n_, const pvae_step_params* sp, hipStream_t st_)
        : c(c_), n(n_), N(&c_->L.net[n_]), w(&c_->W.net[n_]), as(adam_scalars(sp, n_)), st(st_), rowsf(c_->staged_rows_f) {}
    int last() const { return (int)N->layers.size() - 1; }
    const Layer& layer(int i) const { return N->layers[i]; }

    // x: the input panel or act[i-1];  dz: the output gradient;  dx_out: where the input gradient goes, dz[i-1] or d_in
    const float* x(int i, int64_t blk = 0) const { return c->ws + (i == 0 ? w->in : w->act[i - 1]) + blk * layer(i).ld; }
    const float* dz(int i, int64_t blk = 0) const { return c->ws + w->dz[i] + blk * layer(i).n_out_pad; }
    float* dx_out(int i, int64_t blk = 0) const { return c->ws + (i > 0 ? w->dz[i - 1] : w->d_in) + blk * layer(i).ld; }
    // act_grad code of the layer whose output masks the input gradient of layer i (layer i - 1; none for i == 0)
    int mask_act(int i) const { return i > 0 ? layer(i - 1).act : 1; }
    int dgrad_cols(int i) const { return i > 0 || dx0_cols <= 0 ? layer(i).n_in : dx0_cols; }

    // dgrad of layer i: dz[i] (.) W_i -> dz[i-1] (masked) or d_in (i == 0, unmasked)
    DgradArgs dgrad_args(int i, int64_t blk, int rows_pad) const {
        const Layer& l = layer(i);
        return DgradArgs{dz(i, blk), l.n_out_pad, c->params + l.w_off, l.ld, i > 0 ? x(i, blk) : nullptr, l.ld, dx_out(i, blk), l.ld,
                         rows_pad, l.ld, l.n_out_pad, 2.0 * rowsf * dgrad_cols(i) * l.n_out, mask_act(i)};
    }
    int dgrad(int i, int64_t blk, int rows_pad) const {
        const DgradArgs d = dgrad_args(i, blk, rows_pad);
        const int ps = g_prof.begin(1, d.flops, st);
        HIP_TRY(gemm_dgrad(d.dZ, d.ldz, d.W, d.ldw, d.mask, d.ldm, d.dX, d.ldo, d.M, d.Kin, d.Nd, st, d.act));
        g_prof.end(ps, st);
        return 0;
    }
    // wgrad of layer i over rows [0, krows), alone or sharing its launch with the input gradient `d` (of any stack)
    template <class E>
    hipError_t wgrad(int i, int krows, const E& e, const AdamPair* ad) const {
        const Layer& l = layer(i);
        return gemm_wgrad(dz(i), l.n_out_pad, x(i), l.ld, l.n_out_pad, l.ld, krows, e, st, ad);
    }
    template <class E>
    hipError_t wgrad_with_dgrad(int i, int krows, const DgradArgs& d, const E& e, const AdamPair& ad) const {
        const Layer& l = layer(i);
        return gemm_bwd_pair(d.dZ, d.ldz, d.W, d.ldw, d.mask, d.ldm, d.dX, d.ldo, d.M, d.Kin, d.Nd, dz(i), l.n_out_pad, x(i), l.ld,
                             l.n_out_pad, l.ld, krows, e, st, &ad, d.act);
    }

    // what a weight-gradient launch does with layer i's gradient: Adam in place, store, or add into the arena
    EpiGradAdam adam_epi(int i) const {
        const Layer& l = layer(i);
        EpiGradAdam e{c->params + l.w_off, c->m + l.w_off, c->v + l.w_off, l.ld, as};
        e.b = c->params + l.b_off; e.bm = c->m + l.b_off; e.bv = c->v + l.b_off;
        return e;
    }
    EpiGradStore store_epi(int i) const {
        const Layer& l = layer(i);
        EpiGradStore e{c->grads + l.w_off, l.ld};
        e.gb = c->grads + l.b_off;
        return e;
    }
    EpiGradAccum accum_epi(int i) const {
        const Layer& l = layer(i);
        EpiGradAccum e{c->grads + l.w_off, l.ld};
        e.gb = c->grads + l.b_off;
        return e;
    }
    // the epilogue of e's kind for layer i (the second problem of a two-layer launch)
    EpiGradAdam like(const EpiGradAdam&, int i) const { return adam_epi(i); }
    EpiGradStore like(const EpiGradStore&, int i) const { return store_epi(i); }
    EpiGradAccum like(const EpiGradAccum&, int i) const { return accum_epi(i); }
    // f(epilogue of layer i): Adam when `fused`, else the store -- or, kAccum, the add that pvae_net_backward(accumulate)
    // asks for.  (kAccum = false: the unroll, which is never run accumulating and whose unit therefore holds no kernel
    // with that epilogue; naming it there would instantiate them.)
    // (the return type is f's declared one -- int or hipError_t --, not deduced from this body: a deduced one would
    //  instantiate f, and with it the kernels it launches, where the call is parsed and not at the unit's end)
    template <bool kAccum = true, class F>
    std::invoke_result_t<F&, EpiGradAdam> with_grad_epi(int i, bool fused, F&& f) const {
        if (fused) return f(adam_epi(i));
        if constexpr (kAccum)
            if (c->grad_accum) return f(accum_epi(i));
        return f(store_epi(i));
    }
    // the update of layer i as a segment for workgroups of a later launch (its gradient stored by this one)
    AdamSeg adam_seg(int i) const {
        const Layer& l = layer(i);
        AdamSeg a;
        a.p = c->params + l.w_off; a.g = c->grads + l.w_off; a.m = c->m + l.w_off; a.v = c->v + l.w_off;
        a.n4 = (l.b_off + l.n_out_pad - l.w_off) / 4;
        a.s = as;
        return a;
    }
    // the stage finishes layers lo..hi (lo <= hi) of this stack's slice of the gradient arena
    template <class S>                         // (a Stage, or the CarriedWgrad that stands in for one)
    void ready(S& s, int lo, int hi) const {
        s.ready_off = layer(lo).w_off;
        s.ready_cnt = layer(hi).b_off + layer(hi).n_out_pad - layer(lo).w_off;
        s.net = n;
    }
};
void plan_backward_net(pvae_ctx* c, int n, int rows_pad, bool train, bool input_grad, const pvae_step_params* sp, bool fused,
                       hipStream_t st, const LossFinal* fold, Plan& plan, const InputSeed* seed = nullptr,
                       CarriedWgrad* carry_out = nullptr, const CarriedWgrad* carry_in = nullptr,
                       bool wide_follows_layer0 = false);

// ---- pvae_step.hip: the step's shape, and the glue launches the unroll shares with the lookahead-1 plan ----
// Everything a step needs that is a pure function of (phase, rows, step params).
struct StepShape {
    bool fold_sampler;
    int rows_pad, wm_tiles, gridz, nparts_a;
    bool seed_action, seed_sampler;   // stack hand-overs fused into input-gradient epilogues (plan_backward)
    int l1;                    // loss_kind of the three reconstruction terms
    float gs;                  // d(mean loss)/d(residual) factor: 2 for MSE, 1 for L1
    float Bg;
    bool cyc_grad, kl_active;
    LossFinal lf;
};
int add_cols_launch(float* dst, int ldd, int rows, int n, const float* s0, int l0, const float* s1, int l1, const float* s2,
                    int l2, const float* s3, int l3, hipStream_t st);                 // dst[r][c] += s0[r][c] (+ s1 + s2 + s3)
// on the row block `row0` of time step t (`wm_row0`: the world model's predicted-action block)
int helper_seed_launch(pvae_ctx* c, int rows, int64_t row0, hipStream_t st);
int action_loss_launch(pvae_ctx* c, int rows, int t, int64_t row0, int64_t wm_row0, int nparts, float grad_scale, int l1,
                       bool backward, bool extra, hipStream_t st);
int reparam_bwd_launch(pvae_ctx* c, int rows, int64_t row0, float kl_scale, hipStream_t st);

// ---- pvae_lookahead.hip ----
int run_forward_unrolled(pvae_ctx* c, int phase, int rows, const pvae_step_params* sp, const float* eps, bool backward,
                         const StepShape& S, hipStream_t st);
void plan_backward_unrolled(pvae_ctx* c, int phase, int rows, const pvae_step_params* sp, bool backward, bool fused,
                            const StepShape& S, hipStream_t st, Plan& plan);

// ---- pvae_exchange.hip, called by the data-parallel step in pvae_step.hip ----
struct Bucket { int64_t off, cnt; };
int64_t auto_bucket_bytes(const pvae_ctx* c, int phase);
std::vector<Bucket> exchange_buckets(const pvae_ctx* c, int net);
int exchange_bucket(pvae_ctx* c, int net, const Bucket& b, const pvae_step_params* sp, hipStream_t st, hipStream_t cs, int& n_events);

// ---- the PPO learner: what is model-independent (pvae_ppo_core.hip), one struct and one launch per kernel ----
// batch row of minibatch row r: index[r] clamped into [0, n_rows) (a bad entry must not read out of bounds), or row0 + r
__device__ inline long long batch_row(const int32_t* __restrict__ index, long long row0, long long n_rows, int r) {
    if (!index) return row0 + r;
    const long long i = index[r];
    return i < 0 ? 0 : (i >= n_rows ? n_rows - 1 : i);
}
// The loss head on any panels or dense tensors.  fill_head sets the batch / params part and zeroes the rest; the caller
// sets the panel fields, `part`, `part_stride` (= part_stride(k, colsum)) and `colsum`.
struct PpoHead {
    const float* mean; const float* ls; const float* value;       // row r at r * ld_*: panels or dense tensors
    long long ld_mean, ld_ls, ld_value;
    float ls_base;
    const float* actions; const float* old_dist; const float* old_logp;
    const float* adv; const float* vtarg; const float* vpred;
    const int32_t* index; long long row0, n_rows;
    int rows, rows_pad, k;
    float clip, vf_clip, vf_coeff, kl_coeff, ent_coeff, inv_rows;
    float* d_mean; float* d_ls; float* d_value;                  // [rows_pad][width_*] blocks, row stride ld_d* (null: none)
    int ld_dm, ld_dls, ld_dv, width_dm, width_dls, width_dv;
    float* part; int part_stride; int colsum;                    // partial rows [waves][part_stride]; colsum: + the log-std columns
    float* dpart;                                                // diagnostics partial rows [waves][kDiagPart] (null: none; PpoDiag)
};
int head_waves(int rows_pad);                                    // partial rows a head launch over rows_pad rows leaves
int part_stride(int k, bool colsum);
size_t ppo_scratch_bytes(int max_batch, int k);                  // the partial rows of the largest step, 16-byte rounded
int check_loss_args(const pvae_fc_ppo_batch* b, const pvae_fc_ppo_params* p, int rows);
void fill_head(PpoHead& h, const pvae_fc_ppo_batch* b, const pvae_fc_ppo_params* p, const int32_t* index, long long row0,
               int rows, int rows_pad);
int ppo_head_launch(const PpoHead& h, hipStream_t st);
// Adam over up to kAdamSegs segments, each with its own parameter, gradient and moment base pointers, + the stats and the
// log-std vector's update (colsum) in the launch's last workgroup
constexpr int kAdamSegs = 3 * PVAE_FC_MAX_STACKS;
struct PpoAdamSegs {
    int n;
    float* p[kAdamSegs]; const float* g[kAdamSegs]; float* m[kAdamSegs]; float* v[kAdamSegs];
    long long n4[kAdamSegs];                    // float4 elements of segment i
};
// learner diagnostics (PpoDiag, above pvae_ctx)
size_t ppo_diag_bytes(int max_batch);
int ppo_diag_bind(PpoDiag& d, float* diag, int capacity, void* scratch, size_t bytes, int max_batch);
// gradient clipping (PpoClip, above pvae_ctx): the bind, the sum-of-squares launch ahead of the Adam launch (or of
// *_ppo_grad's finish) and *_ppo_grad's in-place scale; with `clip.slot` the two Adam launches below run their CLIP form
size_t ppo_clip_bytes();
int ppo_clip_bind(PpoClip& c, float max_norm, void* scratch, size_t bytes);
int ppo_clip_sumsq_launch(const PpoAdamSegs& segs, const pvae_fc_ppo_params* p, int rows, int k, const float* part, int colsum,
                          float* ls, const PpoClip& clip, hipStream_t st, int* launches);
int ppo_clip_scale_launch(const PpoAdamSegs& segs, const pvae_fc_ppo_params* p, int k, float* ls_grad, int colsum,
                          const PpoClip& clip, const PpoDiagRow& dg, hipStream_t st, int* launches);
int ppo_adam_launch(const PpoAdamSegs& segs, const pvae_fc_ppo_params* p, int adam_t, int rows, int k, const float* part,
                    int colsum, float* ls, float* ls_m, float* ls_v, float* stats_out, const PpoDiagRow& dg, const PpoClip& clip,
                    hipStream_t st, int* launches);
// The step in two halves (include/pvae.h "Gradient exchange between workers").  The first half ends with
// ppo_grad_finish_launch in place of the Adam launch: stats_out[5] (ppo_finish_kernel) and, colsum, ls_grad[k] = the column
// sums of the partial rows, the value the Adam launch's last workgroup forms; `launches` counts what went out.  The second
// half is ppo_apply_launch: Adam over the segments on grad_scale * gradient, the log-std vector from grad_scale * ls_grad.
// With a diagnostics row: the finish launch also writes its entries 0..3 (and zeros the reserved ones), the apply launch
// leaves the squares of what Adam consumed in the slots and one more launch writes entry 4.
int ppo_grad_finish_launch(int rows, int k, const float* part, int colsum, float* ls_grad, float* stats_out,
                           const PpoDiagRow& dg, hipStream_t st, int* launches);
int ppo_apply_launch(const PpoAdamSegs& segs, const pvae_fc_ppo_params* p, int adam_t, int k, float grad_scale,
                     const float* ls_grad, int colsum, float* ls, float* ls_m, float* ls_v, const PpoDiagRow& dg, hipStream_t st,
                     int* launches);

// ---- the PPO learners' peer-mapped gradient exchange (set-up: pvae_exchange.hip; the launch: pvae_ppo_core.hip) ----
// Flag words of the peer-mapped exchanges (unsigned, one block per rank in uncached device memory): epochs and tokens only
// grow, a wait compares with >=, and every wait is bounded -- a peer that never signals raises the error word.
__device__ inline unsigned p2p_ld(const unsigned* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ inline void p2p_st(unsigned* q, unsigned x) { __hip_atomic_store(q, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ inline bool p2p_wait(const unsigned* flag, unsigned epoch, long long timeout, unsigned* err) {
    const long long t0 = wall_clock64();
    while ((int)(p2p_ld(flag) - epoch) < 0) {
        __builtin_amdgcn_s_sleep(8);
        if (wall_clock64() - t0 > timeout) { atomicAdd(err, 1u); return false; }
    }
    return true;
}
// `arenas` / `floats`: the local gradient arenas as bound; k: the log-std vector's length
int ppo_peer_export(PpoPeers& P, float* const* arenas, const long long* floats, int n_arenas, int k, void* blob);
int ppo_peer_open(PpoPeers& P, float* const* arenas, int rank, int world, const void* blobs, long long timeout_ticks);
int ppo_peer_close(PpoPeers& P);
int ppo_peer_status(const PpoPeers& P, int* rank, int* world, uint32_t* timeouts, hipStream_t st);
void ppo_peer_free(PpoPeers& P);
inline long long g_ppo_peer_timeout_ticks = 20ll * 100000000ll;     // stack sets (pvae_set_option(NULL, "p2p_timeout_ms")); 100 MHz
// The exchanged form of ppo_adam_launch: one launch, the N ranks' gradients summed in rank order and scaled by float(1 / N)
int ppo_adam_exchange_launch(PpoPeers& P, long long timeout_ticks, const PpoAdamSegs& segs, const pvae_fc_ppo_params* p,
                             int adam_t, int rows, int k, const float* part, int colsum, float* ls, float* ls_m, float* ls_v,
                             float* stats_out, const PpoDiagRow& dg, const PpoClip& clip, hipStream_t st, int* launches);
int check_ppo_buffers(const float* grad, const float* m, const float* v, const void* scratch, const float* log_std,
                      const float* log_std_m, const float* log_std_v);      // the alignment and pairing rules of *_ppo_bind
// Rows [r0, r1) of up to kZeroPanels panels (columns [0, width) of row stride ld) set to zero: a <= 4-row forward runs on
// the GEMV kernels, which write the live rows only, while the backward contractions read whole 32-row tiles (a stale NaN
// in a pad row would meet a zero gradient row and the product is NaN).
constexpr int kZeroPanels = 1 + PVAE_FC_MAX_STACKS * PVAE_MAX_HIDDEN;       // a stack set: the shared first panel + the deeper ones
static_assert(kZeroPanels >= 3 * (PVAE_MAX_HIDDEN + 1), "kZeroPanels must also hold PhysicsVAE's encoder, decoder and value panels");
struct ZeroRows {
    int n;
    float* p[kZeroPanels];
    int ld[kZeroPanels], width[kZeroPanels];
    int r0, r1;
    void add(float* ptr, int ld_, int width_) { p[n] = ptr; ld[n] = ld_; width[n] = width_; ++n; }
};
int zero_rows_launch(const ZeroRows& z, hipStream_t st);
// dst[rows_pad][ld] = zero-padded copy of src[rows][n]; `index`: of the rows src[index[r]] (clamped into n_rows);
// `done`: row r with done[r] is zeros and its source row is never read
int pad_copy_launch(const float* src, int n, int rows, float* dst, int ld, int rows_pad, const int32_t* index, long long n_rows,
                    const uint8_t* done, hipStream_t st);
// The outputs of one evaluated chunk where its stacks left them: row r of mean / ls / value at r * ld_* (ls: the bound
// vector with ld_ls 0, or the third stack's panel with ls_base), and PhysicsVAE's latent draws eps_src [rows][Z].
struct PpoPanels {
    const float* mean; const float* ls; const float* value;
    long long ld_mean, ld_ls, ld_value;
    float ls_base;
    int rows, k;
    const float* eps_src; int Z;
};
// The evaluate epilogue of one chunk on any panels: vf[r], dist[r] = [mean | ls] and logp[r] of actions[r] for rows
// r < rows (pointers: the chunk's first row), and, eps_dst given, the chunk's draws eps_src [rows][Z] copied out.
// mean == NULL: the bootstrap use, vf[r] = done[r] ? 0 : value[r].
struct PpoEval : PpoPanels {
    const float* actions;
    const uint8_t* done;
    float* vf; float* dist; float* logp;
    float* eps_dst;
};
int ppo_eval_launch(const PpoEval& e, hipStream_t st);
// The sampling epilogue of one chunk (include/pvae.h "Action sampling"): the evaluate epilogue with the action drawn
// instead of read.  Row r of the chunk goes to row dst = out_row ? clamp(out_row[r], [0, n_dst_rows)) : row0 + r of the
// caller's columns, whose BASE pointers the output fields are; noise / obs / out_row: the chunk's first row.
struct PpoAct : PpoPanels {
    const float* noise;                   // [rows][k] supplied draws, or null: Philox (explore only)
    const int32_t* out_row;               // [rows], or null
    long long row0, n_dst_rows;
    int explore, clip;
    float clip_low, clip_high;
    unsigned long long seed, offset;
    float* actions; float* env_actions; float* dist; float* logp; float* vf; float* noise_out;
    const float* obs; float* obs_dst; int n_in;
    float* eps_dst;
};
int ppo_act_launch(const PpoAct& a, hipStream_t st);
// what both sampling entry points ask of their in / out structs beyond their model's check_eval
int check_act(const pvae_ppo_act_in* in, const pvae_ppo_act_out* out);
// the evaluate call over the same rows whose action column is the one a sampling call writes: what check_eval is given
void act_as_evaluate(const pvae_ppo_act_in* in, const pvae_ppo_act_out* out, pvae_fc_rollout& ro, pvae_fc_prepared& ev);
void fill_act(PpoAct& a, const PpoPanels& pan, const pvae_ppo_act_in* in, const pvae_ppo_act_out* out, long long first,
              uint64_t chunk, int n_in);
// GAE: the argument checks, and the GAE launch + (params->standardize) the rescale launch; `launches` counts them
int check_gae_params(const pvae_gae_params* p);
int check_boot(const pvae_fc_rollout* ro, const pvae_fc_prepared* out);
int check_segments(long long n_rows, int n_segs, long long seg_first, long long seg_last);
int check_gae_scratch(const void* scratch, size_t bytes, int n_segs);
int run_gae(const float* rewards, const float* vpred, const float* last_value, const uint8_t* done, const int32_t* seg_start,
            long long n_rows, int n_segs, const pvae_gae_params* p, float* adv, float* vtarg, void* scratch, hipStream_t st,
            int& launches);
// What *_ppo_prepare checks before it launches, in order; `check_eval(rows_pass)` is the caller's own check of its model.
// *given: 3 when the sampler's columns came with the rollout, 0 when the rows pass computes them.
template <class CheckEval>
int check_prepare(const pvae_fc_rollout* ro, const pvae_gae_params* p, const pvae_fc_prepared* out, const void* scratch,
                  size_t scratch_bytes, int* given, CheckEval&& check_eval) {
    int rc = check_gae_params(p);
    if (rc) return rc;
    if (!ro || !out) return fail(-1, "null rollout or outputs");
    *given = (ro->vf_preds != nullptr) + (ro->old_dist != nullptr) + (ro->old_logp != nullptr);
    if (*given != 0 && *given != 3) return fail(-1, "the sampler's vf_preds, old_dist and old_logp go together: all three or none");
    if ((rc = check_eval(*given == 0))) return rc;
    if ((rc = check_boot(ro, out))) return rc;
    if (!ro->rewards || !ro->seg_start) return fail(-1, "rollout rewards or seg_start is null");
    if (!out->advantages || !out->value_targets) return fail(-1, "advantages or value_targets is null");
    if ((rc = check_segments(ro->n_rows, ro->n_segs, ro->seg_first, ro->seg_last))) return rc;
    return check_gae_scratch(scratch, scratch_bytes, ro->n_segs);
}

// ---- the PPO learner step of PhysicsVAE (pvae_ppo.hip) and what it runs of pvae_infer.hip and pvae_fc.hip ----
// pvae_infer.hip: a stack's forward on the panels as they are, the sampler into the decoder's input panel, a stack's backward plan
// with a gradient store into `grad_arena` (arena layout); `launches` counts what went out
void ppo_enter(pvae_ctx* c, int rows);
int ppo_forward_net(pvae_ctx* c, int net, int rows, hipStream_t st, int* launches);
int ppo_sampler(pvae_ctx* c, const float* eps, int rows, int noise, uint64_t seed, uint64_t offset, hipStream_t st, int* launches);
int ppo_backward_net(pvae_ctx* c, int net, int rows, bool train, bool input_grad, float* grad_arena, hipStream_t st, int* launches);
// pvae_fc.hip: the one-stack set [value] that carries the value branch, as the step sees it
struct FcValueStack {
    float* in; int ld_in, n_in;                 // input panel [rows_pad][ld_in] of n_in live columns
    const float* value; int ld_value;           // column 0 of the output layer's panel
    float* d_value; int ld_dv, width_dv;        // the output gradient block [rows_pad][width_dv]
    float* params; float* grad; float* m; float* v;
    long long arena_floats;
    int max_batch;
    int n_panels;                               // the layer-output panels (what a <= 4-row forward leaves unwritten below its rows)
    float* panel[PVAE_MAX_HIDDEN + 1];
    int panel_ld[PVAE_MAX_HIDDEN + 1];
};
int fc_value_stack(pvae_fc* c, FcValueStack* out);                                   // < 0: not a bound [value] set
// pvae_fc.hip: stack s of a set as the value function (1 of an fcnn set, 0 of PhysicsVAE's one-stack set), alone
int fc_value_forward(pvae_fc* c, int s, int rows, hipStream_t st, int* launches);    // on the input panel as it is
int fc_value_backward(pvae_fc* c, int s, int rows, hipStream_t st, int* launches);   // from its output gradient block, into `grad`
// last_value[i] = seg_done[i] ? 0 : value(boot_obs[i]) in chunks of `chunk` segments: copy | the value layers | epilogue
int fc_eval_boot(pvae_fc* c, int s, int chunk, const pvae_fc_rollout* ro, const pvae_fc_prepared* out, hipStream_t st,
                 int& launches);
