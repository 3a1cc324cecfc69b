// pvae_imagine.hip -- imagined rollouts (pvae_imagine*): H closed-loop steps of the policy and the world model in one call.
// Per step the launches are the staged rollout path's own (pvae_infer.hip: forward_net, launch_sampler, the decoder's tail
// into the world model's panel, helper_add_launch); what is new is the HAND-OVER between two steps, one launch that does the
// work of the staged path's stage / copy-out launches and of the unroll's scatter_state_kernel, plus the per-horizon error.
#include "pvae_internal.h"

#include <cstdint>

// z of step t, row r, column j as the hand-over (or the staging launch) puts it into the decoder's input: a supplied code,
// or the sampler's eps draw (latent groups below Z / 4 of Philox row r at offset + t)
__device__ inline float drive_z(const ImagineIo& io, const float* zrow, int r, long long t, int j) {
    return io.zkind == kZSupplied ? zrow[j] : philox_normal(io.seed, io.offset + t, r, j);
}

// Step 0's panels, once per call: one wave per padded row writes EVERY column of every input panel the mode uses -- s_0
// in the body columns (subsets respected), step 0's goal / action / z columns, zeros in pad columns and pad rows, so that
// nothing an earlier call left there reaches a contraction.  The staged path's stage() + sampler-side pad writes, for the
// three modes.
__global__ void __launch_bounds__(256)
imagine_stage_kernel(ImagineIo io, float* __restrict__ z_out) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= io.rows_pad) return;
    const bool valid = r < io.rows;
    const int Db = io.Db, Da = io.Da, Z = io.Z;
    const float* s = valid ? src_row(io.s0, r, 0) : nullptr;
    const float* g = valid && io.mode == PVAE_IMAGINE_TRACK ? src_row(io.goals, r, 0) : nullptr;
    const float* a = valid && io.mode == PVAE_IMAGINE_REPLAY ? src_row(io.actions, r, 0) : nullptr;
    const float* zr = valid && io.zkind == kZSupplied ? src_row(io.z, r, 0) : nullptr;
    const bool have_z = valid && (io.zkind == kZSupplied || io.zkind == kZDrawn);
    int ld_max = io.ld_wm;
    if (io.te_in && io.ld_te > ld_max) ld_max = io.ld_te;
    if (io.md_in && io.ld_md > ld_max) ld_max = io.ld_md;
    if (io.pr_in && io.ld_pr > ld_max) ld_max = io.ld_pr;
    for (int c = lane; c < ld_max; c += 64) {
        const float sv = (valid && c < Db) ? s[c] : 0.f;
        if (io.te_in && c < io.ld_te) {
            float u = 0.f;
            if (c < Db) u = io.te_body ? sv : 0.f;
            else if (g && c < 2 * Db && io.te_task) u = g[c - Db];
            io.te_in[(size_t)r * io.ld_te + c] = u;
        }
        float zv = 0.f;
        if (have_z && c >= Db && c < Db + Z) zv = drive_z(io, zr, r, 0, c - Db);
        if (io.md_in && c < io.ld_md) {
            float u = c < Db ? (io.md_body ? sv : 0.f) : 0.f;
            if (c >= Db && io.md_z == io.md_in) u = zv;
            io.md_in[(size_t)r * io.ld_md + c] = u;
            if (io.md_z != io.md_in && have_z && c >= Db && c < Db + Z) io.md_z[(size_t)r * io.ld_md + c] = zv;
        }
        if (have_z && z_out && c >= Db && c < Db + Z) z_out[(size_t)r * Z + (c - Db)] = zv;
        if (c < io.ld_wm) {
            float u = sv;
            if (c >= Db) u = (a && c < Db + Da) ? a[c - Db] : 0.f;
            io.wm_in[(size_t)r * io.ld_wm + c] = u;
        }
        if (io.pr_in && c < io.ld_pr) io.pr_in[(size_t)r * io.ld_pr + c] = sv;
    }
}

// The hand-over behind step t: one wave per valid row, lanes over the columns (every load and store of the wave covers 256
// contiguous bytes; sources and the body columns of a panel are 4-byte aligned only, hence dword accesses).  The row's
// loads -- the prediction, the target, the action, the next step's drive -- are independent of one another and of every
// store, so they are all in flight together: the launch is a few microseconds of latency on the dependent chain of the
// unroll whatever its arithmetic, and rows / 4 workgroups of four waves put it on as many CUs as there are rows to serve.
//   s_{t+1} = wm_out[r][0:Db]  -> states_out[t], the body columns of the next step's panels (valid rows; subsets respected)
//   a_t                        -> actions_out[t]
//   step t+1's goal / action / z columns from their sources
//   part[blockIdx.x] = sum over the workgroup's rows of (s_{t+1} - target)^2 in double, waves added in a fixed order
__global__ void __launch_bounds__(256)
imagine_handover_kernel(ImagineIo io, const float* __restrict__ wm_out, int ldo_wm, const float* a_src, int lda,
                        long long t, int more, float* __restrict__ states_out, float* __restrict__ actions_out,
                        float* __restrict__ z_out_next, double* __restrict__ part) {
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = blockIdx.x * 4 + wave;
    const int Db = io.Db, Da = io.Da, Z = io.Z;
    double acc = 0.0;
    if (r < io.rows) {
        const float* s = wm_out + (size_t)r * ldo_wm;
        const float* tg = part ? src_row(io.targets, r, t) : nullptr;
        for (int c = lane; c < Db; c += 64) {
            const float v = s[c];
            if (tg) { const float d = v - tg[c]; acc += (double)d * (double)d; }
            if (states_out) states_out[(size_t)r * Db + c] = v;
            if (more) {
                if (io.te_in && io.te_body) io.te_in[(size_t)r * io.ld_te + c] = v;
                if (io.md_in && io.md_body) io.md_in[(size_t)r * io.ld_md + c] = v;
                io.wm_in[(size_t)r * io.ld_wm + c] = v;
                if (io.pr_in) io.pr_in[(size_t)r * io.ld_pr + c] = v;
            }
        }
        if (actions_out)
            for (int c = lane; c < Da; c += 64) actions_out[(size_t)r * Da + c] = a_src[(size_t)r * lda + c];
        if (more) {
            if (io.mode == PVAE_IMAGINE_TRACK) {
                if (io.te_task) {
                    const float* g = src_row(io.goals, r, t + 1);
                    for (int c = lane; c < Db; c += 64) io.te_in[(size_t)r * io.ld_te + Db + c] = g[c];
                }
            } else if (io.mode == PVAE_IMAGINE_REPLAY) {
                const float* a = src_row(io.actions, r, t + 1);
                for (int c = lane; c < Da; c += 64) io.wm_in[(size_t)r * io.ld_wm + Db + c] = a[c];
            } else if (io.zkind == kZSupplied || io.zkind == kZDrawn) {
                const float* zr = io.zkind == kZSupplied ? src_row(io.z, r, t + 1) : nullptr;
                for (int c = lane; c < Z; c += 64) {
                    const float v = drive_z(io, zr, r, t + 1, c);
                    io.md_z[(size_t)r * io.ld_md + Db + c] = v;
                    if (z_out_next) z_out_next[(size_t)r * Z + c] = v;
                }
            }
        }
    }
    if (!part) return;                                     // (uniform over the launch)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// prior mode under the learned prior, z drawn: z_t = prior(s_t) + n_t, one float add (the sampler's place in this mode)
__global__ void __launch_bounds__(256)
imagine_prior_z_kernel(const float* __restrict__ pr_out, int ldp, float* __restrict__ md_z, int ld_md, int Db, int Z, int rows,
                       unsigned long long seed, unsigned long long offset, float* __restrict__ z_out) {
    const int total = rows * Z;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int r = idx / Z, c = idx - r * Z;
        float v;
        {
#pragma clang fp contract(off)                                     // (the draw ends in a product: no fma with the prior's mean)
            v = pr_out[(size_t)r * ldp + c] + philox_normal(seed, offset, r, c);
        }
        md_z[(size_t)r * ld_md + Db + c] = v;
        if (z_out) z_out[idx] = v;
    }
}

// err[t] = float(sum of step t's workgroup partials / (rows * Db)): one wave per step, lanes stride the partials, then the
// xor tree -- a fixed order
__global__ void __launch_bounds__(64)
imagine_fold_kernel(const double* __restrict__ part, int nwg, double inv_n, float* __restrict__ err) {
    const int lane = threadIdx.x, t = blockIdx.x;
    double acc = 0.0;
    for (int i = lane; i < nwg; i += 64) acc += part[(size_t)t * nwg + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) err[t] = (float)(acc * inv_n);
}

static bool imagine_draws_prior(const pvae_ctx* c) { return c->L.cfg.prior_kind == PVAE_PRIOR_STATE_MEAN; }

int imagine_per_step(const pvae_ctx* c, int mode, bool z_supplied) {
    const auto layers = [&](int n) { return (int)c->L.net[n].layers.size(); };
    int n = layers(PVAE_NET_WM) + 1;                                   // the world model + the hand-over
    if (mode != PVAE_IMAGINE_REPLAY) {
        n += layers(PVAE_NET_MD);
        if (layers(PVAE_NET_MH)) n += layers(PVAE_NET_MH) + 1;         // the helper's layers + its add
    }
    if (mode == PVAE_IMAGINE_TRACK) n += layers(PVAE_NET_TE) + 1;      // the encoder + the sampler
    if (mode == PVAE_IMAGINE_PRIOR && !z_supplied && imagine_draws_prior(c)) n += layers(PVAE_NET_PR) + 1;
    return n;
}

ImagineIo imagine_io(pvae_ctx* c, int mode, int zkind, int rows) {
    float* w = c->ws;
    const bool track = mode == PVAE_IMAGINE_TRACK, prior = mode == PVAE_IMAGINE_PRIOR;
    ImagineIo io;
    memset(&io, 0, sizeof(io));
    if (track) { io.te_in = w + c->W.net[PVAE_NET_TE].in; io.ld_te = c->L.net[PVAE_NET_TE].layers[0].ld; }
    if (track || prior) {
        io.md_in = w + c->W.net[PVAE_NET_MD].in; io.ld_md = c->L.net[PVAE_NET_MD].layers[0].ld;
        io.md_z = w + z_panel(c);
    }
    io.wm_in = w + c->W.net[PVAE_NET_WM].in; io.ld_wm = c->L.net[PVAE_NET_WM].layers[0].ld;
    if (zkind == kZLater) { io.pr_in = w + c->W.net[PVAE_NET_PR].in; io.ld_pr = c->L.net[PVAE_NET_PR].layers[0].ld; }
    io.te_body = c->L.cfg.te_inputs != PVAE_INPUT_TASK; io.te_task = c->L.cfg.te_inputs != PVAE_INPUT_BODY;
    io.md_body = c->L.cfg.md_inputs != PVAE_INPUT_TASK;
    io.Db = c->L.cfg.dim_body; io.Da = c->L.cfg.dim_action; io.Z = c->L.cfg.latent;
    io.rows = rows; io.rows_pad = pad32(rows); io.mode = mode; io.zkind = zkind;
    // the training panels are no longer a coherent batch (as pvae_net_forward leaves them); forward_net picks its kernels
    // by staged_rows_f
    c->staged_rows = 0;
    c->staged_rows_f = rows;
    c->dx.on = false;
    return io;
}

int imagine_unroll(pvae_ctx* c, const ImagineIo& io, int H, const float* eps, int noise, float* z_out,
                   const std::function<int(int t, bool more)>& handover, hipStream_t st, int* launches) {
    int rc;
    float* w = c->ws;
    const int Db = io.Db, Da = io.Da, Z = io.Z, rows = io.rows, rows_pad = io.rows_pad;
    const NetLayout& TE = c->L.net[PVAE_NET_TE];
    const NetLayout& MD = c->L.net[PVAE_NET_MD];
    const NetLayout& WM = c->L.net[PVAE_NET_WM];
    const NetLayout& PR = c->L.net[PVAE_NET_PR];
    const bool helper = !c->L.net[PVAE_NET_MH].layers.empty();
    const bool track = io.mode == PVAE_IMAGINE_TRACK, prior = io.mode == PVAE_IMAGINE_PRIOR;
    const bool prior_later = io.zkind == kZLater;
    const int ldo_te = TE.layers.back().n_out_pad;
    for (int t = 0; t < H; ++t) {
        if (track) {
            if ((rc = forward_net(c, PVAE_NET_TE, rows_pad, st))) return rc;
            *launches += (int)TE.layers.size();
            // (the learned prior mean plays no part in the action: rmt:801-809 only records it)
            if ((rc = launch_sampler(c, w + c->W.net[PVAE_NET_TE].act.back(), ldo_te,
                                     eps ? eps + (size_t)t * rows * Z : (const float*)nullptr, w + c->W.eps, io.md_in,
                                     io.ld_md, rows, rows_pad, noise ? 1 : 0, io.seed, io.offset + t, (float*)nullptr,
                                     z_out ? z_out + (size_t)t * rows * Z : (float*)nullptr, (const float*)nullptr, 0, st)))
                return rc;
            ++*launches;
        }
        if (prior_later) {
            if ((rc = forward_net(c, PVAE_NET_PR, rows_pad, st))) return rc;
            *launches += (int)PR.layers.size();
            hipLaunchKernelGGL(imagine_prior_z_kernel, dim3(grid1d((long long)rows * Z, 64)), dim3(256), 0, st,
                               w + c->W.net[PVAE_NET_PR].act.back(), PR.layers.back().n_out_pad, io.md_z, io.ld_md, Db, Z, rows,
                               io.seed, io.offset + t, z_out ? z_out + (size_t)t * rows * Z : (float*)nullptr);
            HIP_TRY(hipGetLastError());
            ++*launches;
        }
        if (track || prior) {
            FwdTail md_tail;                   // a_hat -> the action columns of the world model's input panel
            md_tail.out2 = io.wm_in; md_tail.ld2 = io.ld_wm; md_tail.off2 = Db; md_tail.n2 = Da;
            if ((rc = forward_net(c, PVAE_NET_MD, rows_pad, st, md_tail))) return rc;
            *launches += (int)MD.layers.size();
            if (helper) {                      // rmt:833-835
                if ((rc = forward_net(c, PVAE_NET_MH, rows_pad, st))) return rc;
                if ((rc = helper_add_launch(c, rows, 0, 0, st))) return rc;
                *launches += (int)c->L.net[PVAE_NET_MH].layers.size() + 1;
            }
        }
        if ((rc = forward_net(c, PVAE_NET_WM, rows_pad, st))) return rc;
        *launches += (int)WM.layers.size();
        if ((rc = handover(t, t + 1 < H))) return rc;
        ++*launches;
    }
    return 0;
}

extern "C" {

int pvae_imagine_sizeof(int which) {
    return which == 0 ? (int)sizeof(pvae_imagine_args) : which == 1 ? (int)sizeof(pvae_imagine_src) : fail(-1, "which = 0 / 1");
}

size_t pvae_imagine_scratch_bytes(const pvae_ctx* c, int32_t horizon) {
    if (!c || horizon < 1) { fail(-1, "null ctx or horizon < 1"); return 0; }
    const size_t nwg = (size_t)(c->L.cfg.max_batch + 3) / 4;
    return (nwg * (size_t)horizon * sizeof(double) + 15) / 16 * 16;
}

int pvae_imagine_launches(const pvae_ctx* c, int mode, int32_t* per_step, int32_t* per_call) {
    if (!c) return fail(-1, "null ctx");
    if (mode < PVAE_IMAGINE_REPLAY || mode > PVAE_IMAGINE_PRIOR) return fail(-1, "unknown mode %d", mode);
    if (per_step) *per_step = imagine_per_step(c, mode, false);
    if (per_call) *per_call = 2;
    return 0;
}

int pvae_imagine(pvae_ctx* c, const pvae_imagine_args* a, void* stream) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!a) return fail(-1, "args is null");
    const int mode = a->mode, rows = a->rows, H = a->horizon;
    if (mode < PVAE_IMAGINE_REPLAY || mode > PVAE_IMAGINE_PRIOR) return fail(-1, "unknown mode %d", mode);
    if (!a->s0.base) return fail(-1, "s0 is null");
    if (rows < 1 || rows > c->L.cfg.max_batch) return fail(-1, "rows %d outside [1, %d]", rows, c->L.cfg.max_batch);
    if (H < 1) return fail(-1, "horizon %d < 1", H);
    if (mode == PVAE_IMAGINE_REPLAY && !a->actions.base) return fail(-1, "replay mode needs actions");
    if (mode == PVAE_IMAGINE_TRACK && !a->goals.base) return fail(-1, "track mode needs goals");
    const int kind = c->L.cfg.prior_kind;
    const bool z_supplied = mode == PVAE_IMAGINE_PRIOR && a->z.base;
    if (mode == PVAE_IMAGINE_PRIOR && !z_supplied && kind >= PVAE_PRIOR_HYPERSPHERE)
        return fail(-1, "prior mode needs z under this latent prior (nothing to draw from: rllib_env_imitation.py:246-258 raises)");
    if (a->err && !a->targets.base) return fail(-1, "err without targets");
    const bool with_err = a->err != nullptr;
    if (with_err && (!a->scratch || a->scratch_bytes < pvae_imagine_scratch_bytes(c, H)))
        return fail(-1, "err needs scratch of pvae_imagine_scratch_bytes(ctx, horizon) bytes");
    if (with_err && ((uintptr_t)a->scratch & 7)) return fail(-1, "scratch is not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;

    const int Db = c->L.cfg.dim_body, Da = c->L.cfg.dim_action, Z = c->L.cfg.latent;
    float* w = c->ws;
    const bool prior = mode == PVAE_IMAGINE_PRIOR;
    const bool prior_later = prior && !z_supplied && imagine_draws_prior(c);

    ImagineIo io = imagine_io(c, mode, !prior ? kZNone : z_supplied ? kZSupplied : prior_later ? kZLater : kZDrawn, rows);
    io.s0 = a->s0; io.goals = a->goals; io.actions = a->actions; io.z = a->z; io.targets = a->targets;
    io.seed = a->rng_seed; io.offset = a->rng_offset;

    int launches = 0;
    hipLaunchKernelGGL(imagine_stage_kernel, dim3(io.rows_pad / 4), dim3(256), 0, st, io, prior ? a->z_out : (float*)nullptr);
    HIP_TRY(hipGetLastError());
    ++launches;

    const int nwg = (rows + 3) / 4;
    double* part = with_err ? (double*)a->scratch : nullptr;
    const int ldo_md = c->L.net[PVAE_NET_MD].layers.back().n_out_pad, ldo_wm = c->L.net[PVAE_NET_WM].layers.back().n_out_pad;
    const float* a_src = mode == PVAE_IMAGINE_REPLAY ? io.wm_in + Db : w + c->W.net[PVAE_NET_MD].act.back();
    const int lda = mode == PVAE_IMAGINE_REPLAY ? io.ld_wm : ldo_md;
    const auto handover = [&](int t, bool more) {
        hipLaunchKernelGGL(imagine_handover_kernel, dim3(nwg), dim3(256), 0, st, io, w + c->W.net[PVAE_NET_WM].act.back(), ldo_wm,
                           a_src, lda, (long long)t, more ? 1 : 0,
                           a->states_out ? a->states_out + (size_t)t * rows * Db : (float*)nullptr,
                           a->actions_out ? a->actions_out + (size_t)t * rows * Da : (float*)nullptr,
                           (prior && more && a->z_out) ? a->z_out + (size_t)(t + 1) * rows * Z : (float*)nullptr,
                           part ? part + (size_t)t * nwg : (double*)nullptr);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    if ((rc = imagine_unroll(c, io, H, a->eps, a->noise, a->z_out, handover, st, &launches))) return rc;
    if (with_err) {
        hipLaunchKernelGGL(imagine_fold_kernel, dim3(H), dim3(64), 0, st, part, nwg, 1.0 / ((double)rows * Db), a->err);
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    return launches;
}

}  // extern "C"
