// pvae.hip -- the context of libpvae_gfx950.so (C ABI: include/pvae.h): layout queries, lifecycle, options and bindings,
// minibatch staging, pvae_read_tensor.
//
// Reference lines restated by each kernel are cited at the kernel (tpv / tm / rmt as in
// include/pvae.h).
#include "pvae_internal.h"
#include "pvae_fc_layout.h"

// Minibatch staging as a launch of its own: one block per (padded) batch row and time step
// (blockIdx.y = t < L); the work is stage_row (pvae_gemm.h).
// (four rows per workgroup, one wave each: the row's sources land in LDS by LDS-DMA and the panels are written with whole
//  16-byte stores, stage_row_lds; rows too wide for the wave's LDS: stage_row_wave, branch-free dword-granular buffer
//  accesses.  Round 3's scalar-load form measured 14.2 / 30.3 us per 8192 windows against 14.0 / 20.0: docs/experiments.md)
// per-wave LDS of the gather: the smallest power of two that holds a row's sources + one DMA group of slack (2 KB at the
// configs[2] dims, 4 KB at configs[4]'s: all eight workgroups a CU can hold are resident at once); 0: rows too wide
static inline int stage_lds_floats(int Db, int Da) {
    const int need = 2 * Db + Da + 64;
    if (need > kStageLdsFloats) return 0;
    int n = 256;
    while (n < need) n <<= 1;
    return n;
}
__global__ void __launch_bounds__(256) stage_batch_kernel(StageArgs a, int lds_floats) {
    extern __shared__ float stage_lds[];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                      // (provably wave-uniform: the row's
    const int r = blockIdx.x * 4 + w;                                                    //  descriptors / LDS base live in SGPRs)
    if (r >= a.rows_pad) return;
    if (lds_floats > 0) stage_row_lds(a, r, blockIdx.y, a.rows_pad, threadIdx.x & 63, stage_lds + w * lds_floats, lds_floats - 1);
    else stage_row_wave(a, r, blockIdx.y, a.rows_pad, threadIdx.x & 63);
}

// dst[r][dst_col0 + c] = src[r][src_col0 + c]
__global__ void __launch_bounds__(256)
copy_cols_kernel(const float* __restrict__ src, int lds_, int src_col0, float* __restrict__ dst, int ldd,
                 int dst_col0, int rows, int ncols) {
    const int total = rows * ncols;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / ncols, c = idx - r * ncols;
        dst[(size_t)r * ldd + dst_col0 + c] = src[(size_t)r * lds_ + src_col0 + c];
    }
}
int copy_cols_launch(const float* src, int lds_, int src_col0, float* dst, int ldd, int dst_col0, int rows, int ncols,
                     hipStream_t st) {
    hipLaunchKernelGGL(copy_cols_kernel, dim3(32), dim3(256), 0, st, src, lds_, src_col0, dst, ldd, dst_col0, rows, ncols);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
extern "C" {

int pvae_abi_version(void) { return PVAE_ABI_VERSION; }
const char* pvae_last_error(void) { return g_err; }

int pvae_num_layers(const pvae_config* cfg) {
    if (!cfg) return fail(-1, "null cfg");
    Layout L = make_layout(*cfg);
    if (!L.ok) return fail(-1, "bad config: %s", L.why);
    int n = 0;
    for (auto& N : L.net) n += (int)N.layers.size();
    return n;
}

int pvae_layer(const pvae_config* cfg, int i, pvae_layer_info* out) {
    if (!cfg || !out) return fail(-1, "null argument");
    Layout L = make_layout(*cfg);
    if (!L.ok) return fail(-1, "bad config: %s", L.why);
    for (int n : kArenaOrder) {
        const NetLayout& N = L.net[n];
        if (i < (int)N.layers.size()) {
            const Layer& l = N.layers[i];
            out->net = l.net; out->index = l.index; out->n_in = l.n_in; out->n_out = l.n_out; out->col0 = l.col0;
            out->ld = l.ld; out->n_out_pad = l.n_out_pad; out->w_offset = l.w_off; out->b_offset = l.b_off;
            out->act = l.act == 0 ? PVAE_ACT_LINEAR : l.act - 1;
            return 0;
        }
        i -= (int)N.layers.size();
    }
    return fail(-1, "layer index out of range");
}

int64_t pvae_arena_floats(const pvae_config* cfg) {
    if (!cfg) return fail(-1, "null cfg");
    Layout L = make_layout(*cfg);
    if (!L.ok) return fail(-1, "bad config: %s", L.why);
    return L.arena_floats;
}

int pvae_net_segment(const pvae_config* cfg, int net, int64_t* offset, int64_t* count) {
    if (!cfg || !offset || !count) return fail(-1, "null argument");
    if (net < 0 || net >= PVAE_NUM_NETS) return fail(-1, "bad net id %d", net);
    Layout L = make_layout(*cfg);
    if (!L.ok) return fail(-1, "bad config: %s", L.why);
    *offset = L.net[net].off;
    *count = L.net[net].count;
    return 0;
}

size_t pvae_workspace_bytes(const pvae_config* cfg) {
    if (!cfg) return 0;
    Layout L = make_layout(*cfg);
    if (!L.ok) return 0;
    return (size_t)make_workspace(L).total_floats * sizeof(float);
}

int64_t pvae_workspace_offset(const pvae_config* cfg, int kind, int net, int layer) {
    if (!cfg) return fail(-1, "null cfg");
    Layout L = make_layout(*cfg);
    if (!L.ok) return fail(-1, "bad config: %s", L.why);
    Workspace W = make_workspace(L);
    if (kind >= 0 && kind <= 3) {
        if (net < 0 || net >= PVAE_NUM_NETS || L.net[net].layers.empty()) return fail(-1, "bad net id %d", net);
        if (kind >= 2 && (layer < 0 || layer >= (int)L.net[net].layers.size())) return fail(-1, "bad layer %d", layer);
    }
    switch (kind) {
        case 0: return W.net[net].in;
        case 1: return W.net[net].d_in;
        case 2: return W.net[net].act[layer];
        case 3: return W.net[net].dz[layer];
        case 4: return W.s2;
        case 5: return W.act_t;
        case 6: return W.eps;
        case 7: return W.obs_keep;
        default: return fail(-1, "bad kind %d", kind);
    }
}

int pvae_create(const pvae_config* cfg, pvae_ctx** out) {
    if (!cfg || !out) return fail(-1, "null argument");
    Layout L = make_layout(*cfg);
    if (!L.ok) return fail(-1, "bad config: %s", L.why);
    pvae_ctx* c = new (std::nothrow) pvae_ctx();
    if (!c) return fail(-3, "out of host memory");
    c->L = L;
    c->W = make_workspace(L);
    memset(&c->next_stage, 0, sizeof(c->next_stage));
    *out = c;
    return 0;
}

// Switches of schedule and tile geometry (what used to be PVAE_* environment variables read inside the library): explicit,
// through the ABI.  ctx == NULL: process-wide kernel-geometry switches; else that context's schedule.  The production
// values are the defaults; the parity tests flip them to hold every variant to the same bits.
int pvae_set_option(pvae_ctx* c, const char* name, int64_t value) {
    if (!name) return fail(-1, "null option name");
    const std::string k(name);
    const int v = (int)value;
    if (!c) {
        if (k == "krot") g_krot = v;
        else if (k == "rowxcd") g_rowxcd = v;
        else if (k == "ws64") g_ws64 = v;
        else if (k == "ws6464") g_ws6464 = v;
        else if (k == "ws6464_rows") g_ws6464_rows = v;
        else if (k == "pair64") g_pair64 = v;
        else if (k == "dgrad16") g_dgrad16 = v;
        else if (k == "wgrad32") g_wgrad32 = v;
        else if (k == "look_pair") g_look_pair = v != 0;
        else if (k == "rollout_fused") g_rollout_fused = v != 0;
        else if (k == "fc_per_stack") g_fc_per_stack = v != 0;
        else if (k == "p2p_timeout_ms") { if (value > 0) g_ppo_peer_timeout_ticks = (long long)value * 100000ll; }
        else return fail(-1, "unknown process-wide option '%s'", name);
        return 0;
    }
    if (k == "pair") c->pair_launch = v != 0;
    else if (k == "defer_adam") c->defer_adam = v != 0;
    else if (k == "same_layer") c->same_layer_pairs = v != 0;
    else if (k == "fold_sampler") c->fold_sampler = v != 0;
    else if (k == "joint_s_rec") c->joint_s_rec = v != 0;
    else if (k == "ppo_priors") c->ppo_priors = v != 0;
    else if (k == "direct") return pvae_set_direct(c, v);
    else if (k == "p2p_timeout_ms") { if (value > 0) c->p2p.timeout_ticks = (long long)value * 100000ll; }
    else if (k == "p2p_selftest_flags_only") c->p2p_selftest_flags_only = v != 0;
    else if (k == "server_mailbox") c->server_mailbox = v;             // 0 auto (device memory with a large BAR), 1 host, 2 device
    else return fail(-1, "unknown context option '%s'", name);
    return 0;
}

void pvae_destroy(pvae_ctx* ctx) {
    if (ctx && ctx->comm && g_rccl.ok()) g_rccl.CommDestroy(ctx->comm);
    if (ctx) {
        pvae_p2p_close(ctx);
        if (ctx->p2p.flags) (void)hipFree(ctx->p2p.flags);
        if (ctx->p2p.staging) (void)hipFree(ctx->p2p.staging);
        if (ctx->p2p.self_buf) (void)hipFree(ctx->p2p.self_buf);
        ppo_peer_free(ctx->ppo.peers);
        server_free(ctx);
    }
    delete ctx;
}

int pvae_bind_arenas(pvae_ctx* c, float* params, float* grads, float* exp_avg, float* exp_avg_sq) {
    if (!c) return fail(-1, "null ctx");
    if (!params) return fail(-1, "params arena is null");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15)
        return fail(-1, "arenas must be 16-byte aligned");
    c->params = params; c->grads = grads; c->m = exp_avg; c->v = exp_avg_sq;
    params_touched(c, nullptr, false);
    return 0;
}

int pvae_bind_workspace(pvae_ctx* c, void* workspace, size_t bytes) {
    if (!c) return fail(-1, "null ctx");
    if (!workspace || ((uintptr_t)workspace & 255)) return fail(-1, "workspace must be 256-byte aligned");
    if (bytes < (size_t)c->W.total_floats * sizeof(float))
        return fail(-1, "workspace too small: %zu < %zu", bytes, (size_t)c->W.total_floats * sizeof(float));
    c->ws = (float*)workspace;
    c->seed_pads_clean = false;
    c->pf.valid = false;
    return 0;
}

int pvae_bind_dataset(pvae_ctx* c, const float* states, const float* actions, const int32_t* window_row,
                      int64_t n_rows, int64_t n_windows) {
    if (!c) return fail(-1, "null ctx");
    if (!states || !actions || !window_row) return fail(-1, "null dataset pointer");
    if (n_rows < 2 || n_windows < 1) return fail(-1, "empty dataset");
    if (n_rows > 2147483647ll) return fail(-1, "more than 2^31-1 rows");
    c->states = states; c->actions = actions; c->window_row = window_row;
    c->next_states = nullptr;
    c->n_rows = n_rows; c->n_windows = n_windows;
    c->pf.valid = false;         // a minibatch gathered ahead came from the previous binding
    // the gathered first layers fetch whole 16-byte chunks: the last one of a row may reach 12 bytes past it, i.e. past the
    // array for its very last row.  Only allocations with that much room behind them qualify (else: the panel path).
    auto roomy = [](const float* p, int64_t floats) {
        void* base = nullptr; size_t size = 0;
        if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return false; }
        return (const char*)(p + floats) + 16 <= (const char*)base + size;
    };
    c->data_slack = roomy(states, n_rows * c->L.cfg.dim_body) && roomy(actions, n_rows * c->L.cfg.dim_action);
    // window -> row on the host (RowMap: a minibatch's rows as two runs in kernel arguments instead of an index load in
    // front of every first-layer launch).  The caller's array must be final when it is bound.
    c->window_row_host.clear();
    if (c->data_slack && c->direct) {                   // (pvae_set_direct after the bind: index loads instead -- still correct)
        c->window_row_host.resize((size_t)n_windows);
        if (hipMemcpy(c->window_row_host.data(), window_row, (size_t)n_windows * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            c->window_row_host.clear();
        }
    }
    return 0;
}

int pvae_set_direct(pvae_ctx* c, int on) {
    if (!c) return fail(-1, "null ctx");
    c->direct = on != 0;
    if (c->direct && c->data_slack && c->window_row && (int64_t)c->window_row_host.size() != c->n_windows) {
        c->window_row_host.resize((size_t)c->n_windows);
        if (hipMemcpy(c->window_row_host.data(), c->window_row, (size_t)c->n_windows * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            c->window_row_host.clear();
        }
    }
    return 0;
}

int pvae_bind_dataset_next(pvae_ctx* c, const float* next_states) {
    if (!c) return fail(-1, "null ctx");
    if (!c->states) return fail(-2, "dataset not bound");
    c->next_states = next_states;
    c->pf.valid = false;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// staging
// ---------------------------------------------------------------------------------------
// Arguments of a staging job into the CURRENT (alt == false) or the alternate set of input panels.
StageArgs stage_args(const pvae_ctx* c, long long first_window, const float* x, const float* y, int rows,
                            bool from_set, int steps, bool alt) {
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action;
    float* w = c->ws;
    const int ld_wm = c->L.net[PVAE_NET_WM].layers[0].ld;
    StageArgs a;
    memset(&a, 0, sizeof(a));
    a.states = from_set ? c->states : nullptr;
    a.next_states = from_set ? c->next_states : nullptr;
    a.actions = from_set ? c->actions : nullptr;
    a.window_row = from_set ? c->window_row : nullptr;
    a.first_window = first_window;
    a.x = x; a.y = y;
    a.rows = rows; a.rows_pad = pad32(rows); a.Db = Db; a.Da = Da; a.L = steps;
    a.te_in = w + (alt ? c->W.alt_in[PVAE_NET_TE] : c->W.net[PVAE_NET_TE].in); a.ld_te = c->L.net[PVAE_NET_TE].layers[0].ld;
    a.md_in = w + (alt ? c->W.alt_in[PVAE_NET_MD] : c->W.net[PVAE_NET_MD].in); a.ld_md = c->L.net[PVAE_NET_MD].layers[0].ld;
    a.wm_in = w + (alt ? c->W.alt_in[PVAE_NET_WM] : c->W.net[PVAE_NET_WM].in); a.ld_wm = ld_wm;
    a.s2 = w + (alt ? c->W.alt_s2 : c->W.s2); a.ld_s2 = pad64(Db);
    a.act_t = w + (alt ? c->W.alt_act_t : c->W.act_t); a.ld_a = pad64(Da);
    a.wm_pred = (steps > 1 && !alt) ? a.wm_in + (int64_t)steps * a.rows_pad * ld_wm : nullptr;
    if (!c->L.net[PVAE_NET_PR].layers.empty()) {
        a.pr_in = w + (alt ? c->W.alt_in[PVAE_NET_PR] : c->W.net[PVAE_NET_PR].in);
        a.ld_pr = c->L.net[PVAE_NET_PR].layers[0].ld;
    }
    const int te = c->L.cfg.te_inputs, md = c->L.cfg.md_inputs;          // input subsets: the blocks left out are staged as zeros
    a.in_off = (te == PVAE_INPUT_TASK ? 1 : 0) | (te == PVAE_INPUT_BODY ? 2 : 0) | (md == PVAE_INPUT_TASK ? 4 : 0);
    return a;
}

// `steps`: time steps to stage (the ctx's lookahead for training batches, 1 for rollout inference)
int stage(pvae_ctx* c, long long first_window, const float* x, const float* y, int rows, bool from_set,
                 hipStream_t st, int steps) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (rows < 1 || rows > c->L.cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, c->L.cfg.max_batch);
    c->dx.on = false;
    const StageArgs a = stage_args(c, first_window, x, y, rows, from_set, steps, false);
    const int lf = stage_lds_floats(a.Db, a.Da);
    hipLaunchKernelGGL(stage_batch_kernel, dim3((a.rows_pad + 3) / 4, steps), dim3(256), (size_t)4 * lf * sizeof(float), st, a, lf);
    HIP_TRY(hipGetLastError());
    c->staged_rows = rows;
    c->staged_rows_f = rows;
    return 0;
}

// swap the roles of the two sets of staging panels
void flip_stage_panels(pvae_ctx* c) {
    for (int n = 0; n < PVAE_NUM_NETS; ++n) std::swap(c->W.net[n].in, c->W.alt_in[n]);
    std::swap(c->W.s2, c->W.alt_s2);
    std::swap(c->W.act_t, c->W.alt_act_t);
}

RowMap row_map(const pvae_ctx* c, int64_t first_window, int rows) {
    RowMap rm;
    rm.row = c->window_row + first_window;
    rm.seg = 0; rm.q1 = rows; rm.b0 = rm.b1 = 0;
    if ((int64_t)c->window_row_host.size() == c->n_windows) {          // at most one jump inside the minibatch: two runs
        const int32_t* wr = c->window_row_host.data() + first_window;
        int jumps = 0, at = rows;
        for (int q = 1; q < rows && jumps < 2; ++q)
            if (wr[q] != wr[q - 1] + 1) { ++jumps; at = q; }
        if (jumps < 2) { rm.seg = 1; rm.q1 = at; rm.b0 = wr[0]; rm.b1 = at < rows ? wr[at] : 0; }
    }
    return rm;
}
// the rows the NEXT minibatch's first layers will gather, as runs of 128-byte lines for the last launch of this step to touch
void plan_touch(pvae_ctx* c, int64_t next_first, int next_rows) {
    memset(&c->next_touch, 0, sizeof(c->next_touch));
    if (next_rows <= 0 || next_first < 0 || next_first + next_rows > c->n_windows) return;
    const RowMap rm = row_map(c, next_first, next_rows);
    if (!rm.seg) return;
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action;
    const int n[2] = {rm.q1, next_rows - rm.q1}, b[2] = {rm.b0, rm.b1};
    int total = 0;
    for (int s = 0; s < 2; ++s) {
        if (n[s] <= 0) continue;
        c->next_touch.p[2 * s] = c->states + (size_t)b[s] * Db;
        c->next_touch.lines[2 * s] = (int)(((size_t)(n[s] + 1) * Db * 4 + 127) / 128);     // (+ 1: s_{t+1} of the run's last window)
        c->next_touch.p[2 * s + 1] = c->actions + (size_t)b[s] * Da;
        c->next_touch.lines[2 * s + 1] = (int)(((size_t)n[s] * Da * 4 + 127) / 128);
        total += c->next_touch.lines[2 * s] + c->next_touch.lines[2 * s + 1];
    }
    c->next_touch.blocks = total > 0 ? (total + 255) / 256 : 0;
    if (c->next_touch.blocks > 64) c->next_touch.blocks = 64;
}

extern "C" {

int pvae_invalidate_staging(pvae_ctx* c) {
    if (!c) return fail(-1, "null ctx");
    c->pf.valid = false;
    c->staged_rows = 0;
    return 0;
}

int pvae_gather(pvae_ctx* c, int64_t first_window, int32_t rows, void* stream) {
    if (!c) return fail(-1, "null ctx");
    if (!c->states) return fail(-2, "dataset not bound");
    if (first_window < 0 || first_window + rows > c->n_windows)
        return fail(-1, "windows [%lld, %lld) outside [0, %lld)", (long long)first_window,
                    (long long)(first_window + rows), (long long)c->n_windows);
    return stage(c, first_window, nullptr, nullptr, rows, true, (hipStream_t)stream, c->W.L);
}

int pvae_set_batch(pvae_ctx* c, const float* x, const float* y, int32_t rows, void* stream) {
    if (!c) return fail(-1, "null ctx");
    if (!x) return fail(-1, "x is null");
    return stage(c, 0, x, y, rows, false, (hipStream_t)stream, c->W.L);
}

int pvae_read_tensor(pvae_ctx* c, int what, float* dst, int32_t rows, void* stream) {
    int rc = check_ready(c, false);
    if (rc) return rc;
    if (!dst || rows < 1 || rows > c->W.Bp) return fail(-1, "bad dst/rows");
    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action, Z = c->L.cfg.latent;
    const int t = what >> 3;                   // time step (lookahead > 1), 0 otherwise
    what &= 7;
    if (t < 0 || t >= c->W.L) return fail(-1, "time step %d outside [0, %d)", t, c->W.L);
    const int rows_pad = pad32(c->staged_rows > 0 ? c->staged_rows : rows);
    int64_t blk = (int64_t)t * rows_pad;
    const float* src; int ld, col0, nc;
    const NetWork& wte = c->W.net[PVAE_NET_TE];
    switch (what) {
        case 0: src = c->ws + wte.act.back(); ld = c->L.net[PVAE_NET_TE].layers.back().n_out_pad; col0 = 0; nc = Z; break;
        case 1:
            if (c->L.cfg.prior_kind >= PVAE_PRIOR_HYPERSPHERE) return fail(-1, "this encoder has no logvar");
            src = c->ws + wte.act.back(); ld = c->L.net[PVAE_NET_TE].layers.back().n_out_pad; col0 = Z; nc = Z; break;
        case 2: src = c->ws + z_panel(c); ld = c->L.net[PVAE_NET_MD].layers[0].ld; col0 = Db; nc = Z; break;
        case 3: src = c->ws + c->W.net[PVAE_NET_MD].act.back(); ld = c->L.net[PVAE_NET_MD].layers.back().n_out_pad; col0 = 0; nc = Da; break;
        case 4: src = c->ws + c->W.net[PVAE_NET_WM].act.back(); ld = c->L.net[PVAE_NET_WM].layers.back().n_out_pad; col0 = 0; nc = Db;
                if (c->W.L > 1) blk += (int64_t)c->W.L * rows_pad;      // the predicted-action invocation
                break;
        case 5: src = c->ws + c->W.eps; ld = Z; col0 = 0; nc = Z; break;
        case 6:
            if (c->L.net[PVAE_NET_PR].layers.empty()) return fail(-1, "no learned prior in this configuration");
            src = c->ws + c->W.net[PVAE_NET_PR].act.back(); ld = c->L.net[PVAE_NET_PR].layers.back().n_out_pad; col0 = 0; nc = Z;
            break;
        default: return fail(-1, "unknown tensor id %d", what);
    }
    src += blk * ld;
    return copy_cols_launch(src, ld, col0, dst, nc, 0, rows, nc, (hipStream_t)stream);
}

}  // extern "C"
