// pvae_refine.hip -- backpropagation through imagined rollouts (pvae_imagine_grad*) and gradient-refined latent plans
// (pvae_plan_refine*).  The rule is stated in torch in physicsvae_amd/refine.py.  Row r = e * G + g; start states and
// targets are per environment e = r / G; the codes z [H][rows][Z] are per row.
//
// Forward: imagine_unroll in prior mode with z supplied (pvae_imagine.hip: the same launches); its hand-over here keeps
// s_{t+1} on a state tape in the caller's scratch and adds the row's cost term (rollout_cost_row, shared with pvae_plan.hip).
// The hand-over behind the LAST step also forms the world model's output seed of step H - 1 (ds_H = 0).
//
// Backward, t = H - 1 .. 0.  The workspace holds ONE step's activations: step H - 1's are still in the panels; for t < H - 1
// the panels were restaged (by the backward hand-over of step t + 1) and the decoder, helper and world-model forward
// launches run again.  Then, per step:
//     the world model's input-gradient plan          layers(WM) launches   (a frozen-stack plan: ppo_backward_net, train = false)
//     the action-seed launch                         1                     d a_t -> the decoder's seed and, range * (1 - tanh^2), the helper's
//     the decoder's plan [+ the helper's]            layers(MD) [+ layers(MH)]
//     the backward hand-over                         1                     ds_t, dz_t, the seed of step t - 1, the panels of step t - 1
// = layers(WM) + layers(MD) [+ layers(MH)] + 2 launches per backward step, + the recomputed forward (the forward step
// without its hand-over) for every step but the last.  The world model's last layer is linear, so the seed of step t - 1 is
// cot = coef * (s_t - target) + ds_t from the tape: the backward hand-over of step t writes it before the recompute runs.
// No atomics: every element has one owner (the wave of row r in every launch), the cost is summed in double in a fixed
// order, and the same bits come back on every call.  Every seed and gradient panel is written whole -- pad rows and pad
// columns zero -- by the call itself; parameters, the gradient arena and the Adam state are not touched.
#include "pvae_internal.h"

#include <cstdint>

struct GradIo {
    int G, H;
    const float* z;                     // [H][rows][Z]
    const float* cw;                    // [Db] or null
    const float* sw;                    // [H] or null
    double* J;                          // scratch: the rows' costs
    float* tape;                        // scratch: s_1 .. s_H [H][rows][Db]
    float* cost;                        // [rows] or null
    float* dz;                          // [H][rows][Z] or null
    float* ds;                          // [H][rows][Db] or null
    float* states_out;                  // [H][rows][Db] or null
};

// coef(t, c) = float(2 * sw[t] * cw[c] / Db), formed in double and rounded once
__device__ inline float cost_coef(const GradIo& g, int t, int c, int Db) {
    return (float)(2.0 * (g.sw ? (double)g.sw[t] : 1.0) * (g.cw ? (double)g.cw[c] : 1.0) / (double)Db);
}

// One padded row of the decoder's and the world model's input panels, every column (plan_stage_kernel's work): the state s
// in the body columns (subsets respected), the code in the z columns, zeros in pad columns and pad rows; the action columns
// are the decoder's tail's to write.
__device__ inline void stage_row(const ImagineIo& io, int r, bool valid, const float* __restrict__ s, const float* __restrict__ zr,
                                 int lane) {
    const int Db = io.Db, Z = io.Z;
    const int ld_max = io.ld_wm > io.ld_md ? io.ld_wm : io.ld_md;
    for (int c = lane; c < ld_max; c += 64) {
        const float sv = (valid && c < Db) ? s[c] : 0.f;
        const float zv = (valid && c >= Db && c < Db + Z) ? zr[c - Db] : 0.f;
        if (c < io.ld_md) {
            float u = c < Db ? (io.md_body ? sv : 0.f) : 0.f;
            if (c >= Db && io.md_z == io.md_in) u = zv;
            io.md_in[(size_t)r * io.ld_md + c] = u;
            if (io.md_z != io.md_in && valid && c >= Db && c < Db + Z) io.md_z[(size_t)r * io.ld_md + c] = zv;
        }
        if (c < io.ld_wm) io.wm_in[(size_t)r * io.ld_wm + c] = sv;
    }
}

// Step 0's panels: one wave per padded row.  `zr` (a call of at most 4 rows, whose forward layers write the live rows
// only): the pad rows of the stacks' output panels are zeroed, so that the masks of the backward launches read nothing an
// earlier call left there.
__global__ void __launch_bounds__(256)
refine_stage_kernel(ImagineIo io, GradIo g, ZeroRows zr) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= io.rows_pad) return;
    const bool valid = r < io.rows;
    stage_row(io, r, valid, valid ? src_row(io.s0, r / g.G, 0) : nullptr, valid ? g.z + (size_t)r * io.Z : nullptr, lane);
    if (r >= zr.r0 && r < zr.r1)
        for (int p = 0; p < zr.n; ++p)
            for (int c = lane; c < zr.width[p]; c += 64) zr.p[p][(size_t)r * zr.ld[p] + c] = 0.f;
}

// The forward hand-over behind step t: s_{t+1} onto the tape (and into `states_out`), the body and z columns of the next
// step's panels, J(r) (+)= the row's cost term; behind the last step (`seed` given, the launch then covers the padded rows)
// the world model's output seed of step H - 1, coef * d, whole panel, and cost[r] = float(J(r)).
__global__ void __launch_bounds__(256)
refine_handover_kernel(ImagineIo io, GradIo g, const float* __restrict__ wm_out, int ldo_wm, int t, int more,
                       float* __restrict__ seed) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= io.rows_pad) return;
    if (r >= io.rows) {
        if (seed)
            for (int c = lane; c < ldo_wm; c += 64) seed[(size_t)r * ldo_wm + c] = 0.f;
        return;
    }
    const int Db = io.Db, Z = io.Z;
    const float* s = wm_out + (size_t)r * ldo_wm;
    const float* tg = src_row(io.targets, r / g.G, t);
    const double j_prev = (lane == 0 && t > 0) ? g.J[r] : 0.0;      // (asked for first: off the reduction's path)
    const double step = rollout_cost_row(s, tg, g.cw, g.sw, t, Db, lane);
    float* tape = g.tape + ((size_t)t * io.rows + r) * Db;
    float* so = g.states_out ? g.states_out + ((size_t)t * io.rows + r) * Db : nullptr;
    for (int c = lane; c < Db; c += 64) {
        const float v = s[c];
        tape[c] = v;
        if (so) so[c] = v;
        if (more) {
            if (io.md_body) io.md_in[(size_t)r * io.ld_md + c] = v;
            io.wm_in[(size_t)r * io.ld_wm + c] = v;
        }
    }
    if (more) {
        const float* zr = g.z + ((size_t)(t + 1) * io.rows + r) * Z;
        for (int c = lane; c < Z; c += 64) io.md_z[(size_t)r * io.ld_md + Db + c] = zr[c];
    }
    if (seed)
        for (int c = lane; c < ldo_wm; c += 64)
            seed[(size_t)r * ldo_wm + c] = c < Db ? cost_coef(g, t, c, Db) * (s[c] - tg[c]) : 0.f;
    if (lane == 0) {
        const double j = j_prev + step;
        g.J[r] = j;
        if (!more && g.cost) g.cost[r] = (float)j;
    }
}

// The action seed of a backward step: one wave per padded row.  The action columns of the world model's input gradient
// become the decoder's output seed (times act'(y) of its output layer: linear, 1) and, times range * (1 - h^2), the
// helper's; both panels whole, pad rows and pad columns zero.
__global__ void __launch_bounds__(256)
refine_action_seed_kernel(const float* __restrict__ wm_din, int ld_wm, int Db, int Da, int rows, int rows_pad,
                          const float* __restrict__ md_y, int md_act, float* __restrict__ md_dz, int ldo_md,
                          const float* __restrict__ mh_h, float* __restrict__ mh_dz, int ldo_mh, float range) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows_pad) return;
    const bool valid = r < rows;
    const int ld_max = (mh_dz && ldo_mh > ldo_md) ? ldo_mh : ldo_md;
    for (int c = lane; c < ld_max; c += 64) {
        const float da = (valid && c < Da) ? wm_din[(size_t)r * ld_wm + Db + c] : 0.f;
        if (c < ldo_md) {
            float v = da;
            if (valid && c < Da && md_act) v *= act_grad(md_y[(size_t)r * ldo_md + c], md_act);
            md_dz[(size_t)r * ldo_md + c] = v;
        }
        if (mh_dz && c < ldo_mh) {
            float v = 0.f;
            if (valid && c < Da) {
                const float h = mh_h[(size_t)r * ldo_mh + c];
                v = range * (1.0f - h * h) * da;
            }
            mh_dz[(size_t)r * ldo_mh + c] = v;
        }
    }
}

// The backward hand-over behind step t: one wave per padded row.
//   ds_t(r, c) = the world model's input gradient + (where the decoder reads the body) the decoder's + the helper's, in this order
//   dz_t(r, j) = the decoder's z columns + the helper's, or +0.0 where the decoder does not read the code
//   t > 0: the world model's output seed of step t - 1, coef * (s_t - target) + ds_t (a product, then a sum), whole panel,
//          and the panels of step t - 1 from the tape (or s0) and z[t - 1]
__global__ void __launch_bounds__(256)
refine_bwd_handover_kernel(ImagineIo io, GradIo g, int t, const float* __restrict__ wm_din, const float* __restrict__ md_din,
                           const float* __restrict__ mh_din, int ld_mh, float* __restrict__ seed, int ldo_wm) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= io.rows_pad) return;
    const bool valid = r < io.rows;
    const int Db = io.Db, Z = io.Z, rows = io.rows;
    const bool reads_z = io.md_z == io.md_in;
    if (valid) {
        const float* s_t = t > 0 ? g.tape + ((size_t)(t - 1) * rows + r) * Db : nullptr;
        const float* tg = t > 0 ? src_row(io.targets, r / g.G, t - 1) : nullptr;
        float* dso = g.ds ? g.ds + ((size_t)t * rows + r) * Db : nullptr;
        for (int c = lane; c < Db; c += 64) {
            float v = wm_din[(size_t)r * io.ld_wm + c];
            if (io.md_body) {
                v += md_din[(size_t)r * io.ld_md + c];
                if (mh_din) v += mh_din[(size_t)r * ld_mh + c];
            }
            if (dso) dso[c] = v;
            if (t > 0) {
#pragma clang fp contract(off)
                const float q = cost_coef(g, t - 1, c, Db) * (s_t[c] - tg[c]);
                seed[(size_t)r * ldo_wm + c] = q + v;
            }
        }
        if (g.dz) {
            float* dzo = g.dz + ((size_t)t * rows + r) * Z;
            for (int j = lane; j < Z; j += 64) {
                float v = 0.f;
                if (reads_z) {
                    v = md_din[(size_t)r * io.ld_md + Db + j];
                    if (mh_din) v += mh_din[(size_t)r * ld_mh + Db + j];
                }
                dzo[j] = v;
            }
        }
    }
    if (t == 0) return;
    for (int c = lane + (valid ? Db : 0); c < ldo_wm; c += 64)
        if (!valid || c >= Db) seed[(size_t)r * ldo_wm + c] = 0.f;
    const float* s_prev = !valid ? nullptr : t > 1 ? g.tape + ((size_t)(t - 2) * rows + r) * Db : src_row(io.s0, r / g.G, 0);
    stage_row(io, r, valid, s_prev, valid ? g.z + ((size_t)(t - 1) * rows + r) * Z : nullptr, lane);
}

// ---- refinement -------------------------------------------------------------------------------------------------------
struct RefineIo {
    int E, H, Z, sphere;
    float* v;                           // the iterate [H][E][Z]
    float* zc;                          // the code fed to the unroll: v, or its projection
    float* m; float* w;                 // Adam moments
    float* dz;                          // dJ/dz of the last backward
    float* gv;                          // dJ/dv (the pull-back's result under the sphere)
    float* best_z;                      // the best iterate's code so far
    float* best_cost; int* best_it;     // [E]
    const double* J;                    // the unroll's costs (E rows)
};
struct RefineAdam { float b1, b2, omb1, omb2, step, ibc2, eps; };

// v_0 = the nominal (or zeros), zero moments, z_0 = v_0 or its projection (plan_candidates_kernel's arithmetic): one wave
// per (t, e)
__global__ void __launch_bounds__(256)
refine_init_kernel(RefineIo p, const float* __restrict__ nominal, float* __restrict__ z_iters0) {
    const int lane = threadIdx.x & 63;
    const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= (long long)p.H * p.E) return;
    const size_t o = (size_t)wv * p.Z;
    float e2 = 0.f;
    for (int j = lane; j < p.Z; j += 64) {
        const float v = nominal ? nominal[o + j] : 0.f;
        p.v[o + j] = v; p.m[o + j] = 0.f; p.w[o + j] = 0.f;
        e2 += v * v;
    }
    float ie = 1.0f;
    if (p.sphere) {
#pragma unroll
        for (int q = 32; q > 0; q >>= 1) e2 += __shfl_xor(e2, q, 64);
        ie = 1.0f / fmaxf(sqrtf(e2), 1e-12f);
    }
    for (int j = lane; j < p.Z; j += 64) {
        const float z = p.sphere ? p.v[o + j] * ie : p.v[o + j];      // (each lane reads back its own stores)
        p.zc[o + j] = z;
        if (z_iters0) z_iters0[o + j] = z;
    }
}

// The update behind iteration i: one workgroup per environment.  Thread 0 stores the float cost and decides, on that stored
// value, whether iterate i is the best so far (strictly smaller: ties stay with the lowest i); the workgroup copies the
// code if so.  Then, one wave per step t: the projection's pull-back under the sphere (sphere_bwd_row), Adam on v, every
// operation rounded on its own, and the new iterate's projection.  `last`: no update; the best code, its cost and its
// iteration go to the caller's buffers.
__global__ void __launch_bounds__(256)
refine_update_kernel(RefineIo p, int i, int last, RefineAdam a, float* __restrict__ iter_cost, float* __restrict__ z_next,
                     float* __restrict__ grad_out, float* __restrict__ plan_z, float* __restrict__ cost, int* __restrict__ best_iter) {
    __shared__ int s_take;
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, Z = p.Z;
    if (tid == 0) {
        const float c = (float)p.J[e];
        if (iter_cost) iter_cost[(size_t)i * p.E + e] = c;
        const bool take = i == 0 || c < p.best_cost[e];
        if (take) { p.best_cost[e] = c; p.best_it[e] = i; }
        s_take = take ? 1 : 0;
        if (last) {
            if (cost) cost[e] = take ? c : p.best_cost[e];
            if (best_iter) best_iter[e] = take ? i : p.best_it[e];
        }
    }
    __syncthreads();
    const int take = s_take, HZ = p.H * Z;
    for (int q = tid; q < HZ; q += 256) {
        const int t = q / Z, j = q - t * Z;
        const size_t o = ((size_t)t * p.E + e) * Z + j;
        const float z = take ? p.zc[o] : p.best_z[o];
        if (take) p.best_z[o] = z;
        if (last && plan_z) plan_z[o] = z;
    }
    if (last) return;
    __syncthreads();                                    // (the copy has read zc before any wave overwrites it)
    for (int t = tid >> 6; t < p.H; t += 4) {
        const size_t o = ((size_t)t * p.E + e) * Z;
        const float* g = p.dz + o;
        if (p.sphere) { sphere_bwd_row(p.v + o, p.dz + o, Z, lane, p.gv + o); g = p.gv + o; }
        float e2 = 0.f;
        for (int j = lane; j < Z; j += 64) {
#pragma clang fp contract(off)
            const float gj = g[j];
            const float m = a.b1 * p.m[o + j] + a.omb1 * gj;
            const float w = a.b2 * p.w[o + j] + a.omb2 * (gj * gj);
            const float den = sqrtf(w) * a.ibc2 + a.eps;
            const float v = p.v[o + j] - a.step * (m / den);
            p.m[o + j] = m; p.w[o + j] = w; p.v[o + j] = v;
            if (grad_out) grad_out[o + j] = gj;
            e2 += v * v;
        }
        float ie = 1.0f;
        if (p.sphere) {
#pragma unroll
            for (int q = 32; q > 0; q >>= 1) e2 += __shfl_xor(e2, q, 64);
            ie = 1.0f / fmaxf(sqrtf(e2), 1e-12f);
        }
        for (int j = lane; j < Z; j += 64) {
            const float z = p.sphere ? p.v[o + j] * ie : p.v[o + j];
            p.zc[o + j] = z;
            if (z_next) z_next[o + j] = z;
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
static size_t round16(size_t n) { return (n + 15) / 16 * 16; }

// scratch of the unroll: [rows] double costs | the state tape [H][rows][Db]
static size_t grad_scratch_layout(int Db, int H, int rows, size_t* tape_off) {
    const size_t j = round16((size_t)rows * sizeof(double));
    if (tape_off) *tape_off = j;
    return j + round16((size_t)H * rows * Db * sizeof(float));
}

static bool has_helper(const pvae_ctx* c) { return !c->L.net[PVAE_NET_MH].layers.empty(); }
static int bwd_per_step(const pvae_ctx* c) {
    const auto layers = [&](int n) { return (int)c->L.net[n].layers.size(); };
    return layers(PVAE_NET_WM) + layers(PVAE_NET_MD) + (has_helper(c) ? layers(PVAE_NET_MH) : 0) + 2;
}
static int grad_launches(const pvae_ctx* c, int H, bool backward) {
    const int f = imagine_per_step(c, PVAE_IMAGINE_PRIOR, true);
    return 1 + H * f + (backward ? H * bwd_per_step(c) + (H - 1) * (f - 1) : 0);
}

// the unroll on panels and scratch that the caller checked: forward, and (backward) t = H - 1 .. 0
static int grad_run(pvae_ctx* c, int E, const pvae_imagine_src& s0, const pvae_imagine_src& targets, const GradIo& g, bool backward,
                    hipStream_t st, int* launches) {
    int rc;
    const int rows = E * g.G, H = g.H;
    ImagineIo io = imagine_io(c, PVAE_IMAGINE_PRIOR, kZSupplied, rows);
    io.s0 = s0; io.targets = targets;
    float* w = c->ws;
    const NetLayout& MD = c->L.net[PVAE_NET_MD];
    const NetLayout& MH = c->L.net[PVAE_NET_MH];
    const NetLayout& WM = c->L.net[PVAE_NET_WM];
    const NetWork& wmd = c->W.net[PVAE_NET_MD];
    const NetWork& wmh = c->W.net[PVAE_NET_MH];
    const NetWork& wwm = c->W.net[PVAE_NET_WM];
    const bool helper = has_helper(c);
    const int ldo_wm = WM.layers.back().n_out_pad, ldo_md = MD.layers.back().n_out_pad;
    const int ldo_mh = helper ? MH.layers.back().n_out_pad : 0;
    const int rows_pad = io.rows_pad;
    float* seed = w + wwm.dz.back();

    ZeroRows zr{};
    if (backward && rows <= 4 && rows < rows_pad) {      // the GEMV forward layers write the live rows only
        zr.r0 = rows; zr.r1 = rows_pad;
        for (const Layer& l : MD.layers) zr.add(w + wmd.act[l.index], l.n_out_pad, l.n_out_pad);
        for (const Layer& l : MH.layers) zr.add(w + wmh.act[l.index], l.n_out_pad, l.n_out_pad);
        for (const Layer& l : WM.layers) zr.add(w + wwm.act[l.index], l.n_out_pad, l.n_out_pad);
    }
    hipLaunchKernelGGL(refine_stage_kernel, dim3(rows_pad / 4), dim3(256), 0, st, io, g, zr);
    HIP_TRY(hipGetLastError());
    ++*launches;
    const auto handover = [&](int t, bool more) {
        const bool seeds = backward && !more;
        hipLaunchKernelGGL(refine_handover_kernel, dim3(seeds ? rows_pad / 4 : (rows + 3) / 4), dim3(256), 0, st, io, g,
                           w + wwm.act.back(), ldo_wm, t, more ? 1 : 0, seeds ? seed : (float*)nullptr);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    if ((rc = imagine_unroll(c, io, H, nullptr, 0, nullptr, handover, st, launches))) return rc;
    if (!backward) return 0;

    for (int t = H - 1; t >= 0; --t) {
        if (t < H - 1) {                               // step t's activations again, on the panels the hand-over of t + 1 staged
            FwdTail md_tail;
            md_tail.out2 = io.wm_in; md_tail.ld2 = io.ld_wm; md_tail.off2 = io.Db; md_tail.n2 = io.Da;
            if ((rc = forward_net(c, PVAE_NET_MD, rows_pad, st, md_tail))) return rc;
            *launches += (int)MD.layers.size();
            if (helper) {
                if ((rc = forward_net(c, PVAE_NET_MH, rows_pad, st))) return rc;
                if ((rc = helper_add_launch(c, rows, 0, 0, st))) return rc;
                *launches += (int)MH.layers.size() + 1;
            }
            if ((rc = forward_net(c, PVAE_NET_WM, rows_pad, st))) return rc;
            *launches += (int)WM.layers.size();
        }
        if ((rc = ppo_backward_net(c, PVAE_NET_WM, rows, false, true, nullptr, st, launches))) return rc;
        hipLaunchKernelGGL(refine_action_seed_kernel, dim3(rows_pad / 4), dim3(256), 0, st, w + wwm.d_in, io.ld_wm, io.Db, io.Da,
                           rows, rows_pad, w + wmd.act.back(), MD.layers.back().act, w + wmd.dz.back(), ldo_md,
                           helper ? w + wmh.act.back() : (const float*)nullptr, helper ? w + wmh.dz.back() : (float*)nullptr,
                           ldo_mh, c->L.cfg.mh_range);
        HIP_TRY(hipGetLastError());
        ++*launches;
        if ((rc = ppo_backward_net(c, PVAE_NET_MD, rows, false, true, nullptr, st, launches))) return rc;
        if (helper && (rc = ppo_backward_net(c, PVAE_NET_MH, rows, false, true, nullptr, st, launches))) return rc;
        hipLaunchKernelGGL(refine_bwd_handover_kernel, dim3(rows_pad / 4), dim3(256), 0, st, io, g, t, w + wwm.d_in, w + wmd.d_in,
                           helper ? w + wmh.d_in : (const float*)nullptr, helper ? MH.layers[0].ld : 0, seed, ldo_wm);
        HIP_TRY(hipGetLastError());
        ++*launches;
    }
    return 0;
}

// scratch of a refinement: the unroll's | v | zc | m | w | dz | gv | best_z (each [H][E][Z]) | best_cost [E] | best_it [E]
static size_t refine_scratch_layout(int Db, int Z, int H, int E, size_t* code_off, size_t* code_bytes, size_t* best_off) {
    const size_t g = grad_scratch_layout(Db, H, E, nullptr);
    const size_t code = round16((size_t)H * E * Z * sizeof(float));
    const size_t be = round16((size_t)E * sizeof(float));
    if (code_off) *code_off = g;
    if (code_bytes) *code_bytes = code;
    if (best_off) *best_off = g + 7 * code;
    return g + 7 * code + 2 * be;
}

extern "C" {

int pvae_imagine_grad_sizeof(int which) {
    return which == 0 ? (int)sizeof(pvae_imagine_grad_args) : fail(-1, "which = 0");
}

size_t pvae_imagine_grad_scratch_bytes(const pvae_ctx* c, int32_t horizon, int32_t rows) {
    if (!c || horizon < 1 || rows < 1) { fail(-1, "null ctx, horizon < 1 or rows < 1"); return 0; }
    return grad_scratch_layout(c->L.cfg.dim_body, horizon, rows, nullptr);
}

int pvae_imagine_grad_launches(const pvae_ctx* c, int32_t* fwd_per_step, int32_t* bwd_per_step_out, int32_t* per_call) {
    if (!c) return fail(-1, "null ctx");
    if (fwd_per_step) *fwd_per_step = imagine_per_step(c, PVAE_IMAGINE_PRIOR, true);
    if (bwd_per_step_out) *bwd_per_step_out = bwd_per_step(c);
    if (per_call) *per_call = 1;                       // the stage launch
    return 0;
}

int pvae_imagine_grad(pvae_ctx* c, const pvae_imagine_grad_args* a, void* stream) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!a) return fail(-1, "args is null");
    if (!a->s0.base) return fail(-1, "s0 is null");
    if (!a->targets.base) return fail(-1, "targets is null");
    if (!a->z) return fail(-1, "z is null");
    const int E = a->envs, G = a->group, H = a->horizon;
    if (E < 1) return fail(-1, "envs %d < 1", E);
    if (G < 1) return fail(-1, "group %d < 1", G);
    const long long rows_ll = (long long)E * G;
    if (rows_ll > c->L.cfg.max_batch) return fail(-1, "rows %lld = envs * group outside [1, %d]", rows_ll, c->L.cfg.max_batch);
    if (H < 1) return fail(-1, "horizon %d < 1", H);
    const int rows = (int)rows_ll, Db = c->L.cfg.dim_body;
    size_t tape_off;
    const size_t need = grad_scratch_layout(Db, H, rows, &tape_off);
    if (!a->scratch || a->scratch_bytes < need) return fail(-1, "scratch is missing or shorter than pvae_imagine_grad_scratch_bytes");
    if ((uintptr_t)a->scratch & 15) return fail(-1, "scratch is not 16-byte aligned");
    GradIo g;
    memset(&g, 0, sizeof(g));
    g.G = G; g.H = H; g.z = a->z; g.cw = a->col_weight; g.sw = a->step_weight;
    g.J = (double*)a->scratch; g.tape = (float*)((char*)a->scratch + tape_off);
    g.cost = a->cost; g.dz = a->dz; g.ds = a->ds; g.states_out = a->states_out;
    int launches = 0;
    if ((rc = grad_run(c, E, a->s0, a->targets, g, a->dz || a->ds, (hipStream_t)stream, &launches))) return rc;
    return launches;
}

int pvae_plan_refine_sizeof(int which) {
    return which == 0 ? (int)sizeof(pvae_plan_refine_args) : fail(-1, "which = 0");
}

size_t pvae_plan_refine_scratch_bytes(const pvae_ctx* c, int32_t horizon, int32_t envs) {
    if (!c || horizon < 1 || envs < 1) { fail(-1, "null ctx, horizon < 1 or envs < 1"); return 0; }
    return refine_scratch_layout(c->L.cfg.dim_body, c->L.cfg.latent, horizon, envs, nullptr, nullptr, nullptr);
}

int pvae_plan_refine_launches(const pvae_ctx* c, int32_t* per_iter, int32_t* per_call) {
    if (!c) return fail(-1, "null ctx");
    if (per_iter) *per_iter = 1;                                                       // the update launch
    if (per_call) *per_call = 2 + imagine_per_step(c, PVAE_IMAGINE_PRIOR, true) + 1;   // init, the last keep, the closing pass
    return 0;
}

int pvae_plan_refine(pvae_ctx* c, const pvae_plan_refine_args* a, void* stream) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!a) return fail(-1, "args is null");
    if (!a->s0.base) return fail(-1, "s0 is null");
    if (!a->targets.base) return fail(-1, "targets is null");
    const int E = a->envs, H = a->horizon, steps = a->steps;
    if (E < 1) return fail(-1, "envs %d < 1", E);
    if (E > c->L.cfg.max_batch) return fail(-1, "rows %d = envs outside [1, %d]", E, c->L.cfg.max_batch);
    if (H < 1) return fail(-1, "horizon %d < 1", H);
    if (steps < 0) return fail(-1, "steps %d < 0", steps);
    if (!(a->lr > 0.f) || !std::isfinite(a->lr)) return fail(-1, "lr is not finite or not positive");
    const int Db = c->L.cfg.dim_body, Z = c->L.cfg.latent;
    size_t code_off, code, best_off;
    const size_t need = refine_scratch_layout(Db, Z, H, E, &code_off, &code, &best_off);
    if (!a->scratch || a->scratch_bytes < need) return fail(-1, "scratch is missing or shorter than pvae_plan_refine_scratch_bytes");
    if ((uintptr_t)a->scratch & 15) return fail(-1, "scratch is not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)a->scratch;
    size_t tape_off;
    grad_scratch_layout(Db, H, E, &tape_off);

    RefineIo p;
    memset(&p, 0, sizeof(p));
    p.E = E; p.H = H; p.Z = Z; p.sphere = c->L.cfg.prior_kind == PVAE_PRIOR_HYPERSPHERE;
    p.v = (float*)(base + code_off); p.zc = (float*)(base + code_off + code);
    p.m = (float*)(base + code_off + 2 * code); p.w = (float*)(base + code_off + 3 * code);
    p.dz = (float*)(base + code_off + 4 * code); p.gv = (float*)(base + code_off + 5 * code);
    p.best_z = (float*)(base + code_off + 6 * code);
    p.best_cost = (float*)(base + best_off);
    p.best_it = (int*)(base + best_off + round16((size_t)E * sizeof(float)));
    p.J = (const double*)base;

    GradIo g;
    memset(&g, 0, sizeof(g));
    g.G = 1; g.H = H; g.z = p.zc; g.cw = a->col_weight; g.sw = a->step_weight;
    g.J = (double*)base; g.tape = (float*)(base + tape_off);
    g.dz = p.dz;

    const size_t HEZ = (size_t)H * E * Z;
    int launches = 0;
    hipLaunchKernelGGL(refine_init_kernel, dim3((int)(((long long)H * E + 3) / 4)), dim3(256), 0, st, p, a->nominal, a->z_iters);
    HIP_TRY(hipGetLastError());
    ++launches;
    RefineAdam ad;
    ad.b1 = 0.9f; ad.b2 = 0.999f; ad.omb1 = (float)(1.0 - 0.9); ad.omb2 = (float)(1.0 - 0.999); ad.eps = 1e-8f;
    ad.step = 0.f; ad.ibc2 = 0.f;
    if (steps == 0 && a->grad) HIP_TRY(hipMemsetAsync(a->grad, 0, HEZ * sizeof(float), st));
    for (int i = 0; i <= steps; ++i) {
        const bool last = i == steps;
        if ((rc = grad_run(c, E, a->s0, a->targets, g, !last, st, &launches))) return rc;
        if (!last) {
            ad.step = (float)((double)a->lr / (1.0 - std::pow(0.9, i + 1)));
            ad.ibc2 = (float)(1.0 / std::sqrt(1.0 - std::pow(0.999, i + 1)));
        }
        hipLaunchKernelGGL(refine_update_kernel, dim3(E), dim3(256), 0, st, p, i, last ? 1 : 0, ad, a->iter_cost,
                           (a->z_iters && !last) ? a->z_iters + (size_t)(i + 1) * HEZ : (float*)nullptr,
                           (i + 1 == steps) ? a->grad : (float*)nullptr, a->plan_z, a->cost, a->best_iter);
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    // the refined plan's first step once more, on E rows with z = plan_z[0]: an imagine prior-mode call of horizon 1
    pvae_imagine_args q;
    memset(&q, 0, sizeof(q));
    q.mode = PVAE_IMAGINE_PRIOR; q.rows = E; q.horizon = 1;
    q.s0 = a->s0;
    q.z.base = p.best_z; q.z.ld = Z; q.z.step = (int64_t)E * Z;
    q.actions_out = a->a0; q.states_out = a->s1;
    if ((rc = pvae_imagine(c, &q, stream)) < 0) return rc;
    return launches + rc;
}

}  // extern "C"
