// pvae_plan.hip -- planning over imagined rollouts (pvae_plan*): K sampled candidate code sequences per environment, the
// H-step unroll of pvae_imagine.hip on E * K rows (imagine_unroll, prior mode with z supplied: the same launches), a
// per-row cost accumulated by the hand-over launch, and a selection launch per iteration.  The rule is stated in torch in
// physicsvae_amd/plan.py.  Row r = e * K + k; targets, start states and the nominal are per environment e = r / K.
// No atomics: every J(r), every candidate and every output element has one owner, and launch order serialises the steps.
#include "pvae_internal.h"

#include <cstdint>

struct PlanIo {
    int E, K, H, sphere;
    float sigma;
    double lam;
    const float* noise;                 // [H][rows][Z] of this iteration, or null: Philox
    const float* cw;                    // [Db] or null
    const float* sw;                    // [H] or null
    unsigned long long seed, offset;    // offset of this iteration's step 0
    long long row0;
    float* zc;                          // scratch: the iteration's candidate codes [H][rows][Z]
    double* J;                          // scratch: the rows' costs
};

// Candidates of one iteration: one wave per (t, row).  v = u(t, e) + sigma * n (mul, then add: two roundings as in torch);
// candidate 0 is the nominal itself, nothing drawn.  Under the sphere the row is projected as sphere_kernel projects the
// encoder's output: lanes stride the columns, the xor tree, z = v * (1 / max(sqrt(sum v^2), 1e-12)).
__global__ void __launch_bounds__(256)
plan_candidates_kernel(PlanIo p, int Z, const float* __restrict__ u, float* __restrict__ z_cand, float* __restrict__ noise_out) {
    const int lane = threadIdx.x & 63;
    const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int rows = p.E * p.K;
    if (wv >= (long long)p.H * rows) return;
    const int t = (int)(wv / rows), r = (int)(wv - (long long)t * rows), e = r / p.K, k = r - e * p.K;
    const float* ur = u ? u + ((size_t)t * p.E + e) * Z : nullptr;
    float* zr = p.zc + (size_t)wv * Z;
    float e2 = 0.f;
    for (int j = lane; j < Z; j += 64) {
        const float base = ur ? ur[j] : 0.f;
        float n = 0.f, v = base;
        if (k > 0) {
            n = p.noise ? p.noise[(size_t)wv * Z + j] : philox_normal(p.seed, p.offset + t, (uint32_t)(p.row0 + r), j);
            {
#pragma clang fp contract(off)
                const float sn = p.sigma * n;
                v = base + sn;
            }
        }
        if (noise_out) noise_out[(size_t)wv * Z + j] = n;
        zr[j] = v;
        e2 += v * v;
    }
    if (p.sphere) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) e2 += __shfl_xor(e2, o, 64);
        const float ie = 1.0f / fmaxf(sqrtf(e2), 1e-12f);
        for (int j = lane; j < Z; j += 64) zr[j] = zr[j] * ie;      // (each lane reads back its own stores)
    }
    if (z_cand)
        for (int j = lane; j < Z; j += 64) z_cand[(size_t)wv * Z + j] = zr[j];
}

// Step 0's panels of an iteration: imagine_stage_kernel for prior mode with z supplied, the start state of row r read from
// environment r / K and its code from the candidates.  One wave per padded row writes every column of the decoder's and the
// world model's input panels (pad rows and columns zero).
__global__ void __launch_bounds__(256)
plan_stage_kernel(ImagineIo io, PlanIo p) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= io.rows_pad) return;
    const bool valid = r < io.rows;
    const int Db = io.Db, Z = io.Z;
    const float* s = valid ? src_row(io.s0, r / p.K, 0) : nullptr;
    const float* zr = valid ? p.zc + (size_t)r * Z : nullptr;
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
        if (c < io.ld_wm) io.wm_in[(size_t)r * io.ld_wm + c] = sv;   // (the action columns: the decoder's tail writes them)
    }
}

// The hand-over behind step t with the row's cost: imagine_handover_kernel's work for prior mode with z supplied (s_{t+1}
// into `states_out` and the body columns of the next step's panels, the next step's code from the candidates), and
//   J(r) (+)= sw[t] * (sum_c cw[c] * double(d) * double(d)) / Db,   d = s_{t+1}(r, c) - targets(t, r / K, c) in float,
// lanes striding the columns, then the xor tree; step 0 stores, later steps add -- the wave that owns row r in every launch.
__global__ void __launch_bounds__(256)
plan_handover_kernel(ImagineIo io, PlanIo p, const float* __restrict__ wm_out, int ldo_wm, int t, int more,
                     float* __restrict__ states_out) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= io.rows) return;
    const int Db = io.Db, Z = io.Z;
    const float* s = wm_out + (size_t)r * ldo_wm;
    const float* tg = src_row(io.targets, r / p.K, t);
    const double j_prev = (lane == 0 && t > 0) ? p.J[r] : 0.0;      // (asked for first: off the reduction's path)
    const double step = rollout_cost_row(s, tg, p.cw, p.sw, t, Db, lane);      // (pvae_internal.h: shared with pvae_refine.hip)
    for (int c = lane; c < Db; c += 64) {
        const float v = s[c];
        if (states_out) states_out[(size_t)r * Db + c] = v;
        if (more) {
            if (io.md_body) io.md_in[(size_t)r * io.ld_md + c] = v;
            io.wm_in[(size_t)r * io.ld_wm + c] = v;
        }
    }
    if (more) {
        const float* zr = p.zc + ((size_t)(t + 1) * io.rows + r) * Z;
        for (int c = lane; c < Z; c += 64) io.md_z[(size_t)r * io.ld_md + Db + c] = zr[c];
    }
    if (lane == 0) p.J[r] = j_prev + step;
}

// Selection: one workgroup per environment.  The K costs, rounded once to float, go through LDS (and to `cost`); wave 0
// finds the smallest, ties to the lowest k; the weights exp(-(cost_k - cost_best) / lam) in
// double through LDS; each thread owns (t, j) outputs and loops k in ascending order.  lam == 0: the best candidate's code,
// copied.  Under the sphere the weighted mean is projected again (one wave per t, after a barrier).
__global__ void __launch_bounds__(256)
plan_select_kernel(PlanIo p, int Z, float* __restrict__ u_next, float* __restrict__ plan_z, int* __restrict__ best,
                   float* __restrict__ cost, float* __restrict__ iter_cost) {
    extern __shared__ double lds_w[];                  // [K] weights, then [K] float costs
    float* lds_c = (float*)(lds_w + p.K);
    __shared__ int s_best;
    const int e = blockIdx.x, K = p.K, tid = threadIdx.x, lane = tid & 63, rows = p.E * K;
    for (int k = tid; k < K; k += 256) {
        const float c = (float)p.J[(size_t)e * K + k];
        lds_c[k] = c;
        if (cost) cost[(size_t)e * K + k] = c;
    }
    __syncthreads();
    if (tid < 64) {
        float bc = lds_c[0];
        int bk = 0;
        for (int k = lane; k < K; k += 64) {           // (ascending per lane: a strict < keeps the lowest k)
            const float c = lds_c[k];
            if (c < bc || (k < bk && c == bc)) { bc = c; bk = k; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float oc = __shfl_xor(bc, o, 64);
            const int ok = __shfl_xor(bk, o, 64);
            if (oc < bc || (oc == bc && ok < bk)) { bc = oc; bk = ok; }
        }
        if (lane == 0) {
            s_best = bk;
            if (best) best[e] = bk;
            if (iter_cost) iter_cost[e] = lds_c[bk];
        }
    }
    __syncthreads();
    const int bk = s_best;
    const int HZ = p.H * Z;
    if (p.lam == 0.0) {
        for (int i = tid; i < HZ; i += 256) {
            const int t = i / Z, j = i - t * Z;
            const float v = p.zc[((size_t)t * rows + (size_t)e * K + bk) * Z + j];
            u_next[((size_t)t * p.E + e) * Z + j] = v;
            if (plan_z) plan_z[((size_t)t * p.E + e) * Z + j] = v;
        }
        return;
    }
    const double cb = (double)lds_c[bk];
    for (int k = tid; k < K; k += 256) lds_w[k] = exp(-((double)lds_c[k] - cb) / p.lam);
    __syncthreads();
    for (int i = tid; i < HZ; i += 256) {
        const int t = i / Z, j = i - t * Z;
        const float* zt = p.zc + ((size_t)t * rows + (size_t)e * K) * Z + j;
        double num = 0.0, den = 0.0;
        for (int k0 = 0; k0 < K; k0 += 8) {             // eight loads in flight, then their sums in ascending k
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = k0 + q < K ? zt[(size_t)(k0 + q) * Z] : 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (k0 + q < K) {
                    const double w = lds_w[k0 + q];
                    num += w * (double)v[q];
                    den += w;
                }
            }
        }
        u_next[((size_t)t * p.E + e) * Z + j] = (float)(num / den);
    }
    __syncthreads();                                    // (the workgroup's stores to u_next are visible to its waves)
    for (int t = tid >> 6; t < p.H; t += 4) {
        float* ur = u_next + ((size_t)t * p.E + e) * Z;
        float ie = 1.0f;
        if (p.sphere) {
            float e2 = 0.f;
            for (int j = lane; j < Z; j += 64) e2 += ur[j] * ur[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) e2 += __shfl_xor(e2, o, 64);
            ie = 1.0f / fmaxf(sqrtf(e2), 1e-12f);
        }
        for (int j = lane; j < Z; j += 64) {
            const float v = p.sphere ? ur[j] * ie : ur[j];
            if (p.sphere) ur[j] = v;
            if (plan_z) plan_z[((size_t)t * p.E + e) * Z + j] = v;
        }
    }
}

// scratch: [rows] double costs | [H][rows][Z] candidate codes | [H][rows][Z] the nominal between iterations (E <= rows)
static size_t plan_scratch_layout(int Z, int H, int rows, size_t* zc_off, size_t* u_off) {
    const size_t j = ((size_t)rows * sizeof(double) + 15) / 16 * 16;
    const size_t zc = ((size_t)H * rows * Z * sizeof(float) + 15) / 16 * 16;
    if (zc_off) *zc_off = j;
    if (u_off) *u_off = j + zc;
    return j + 2 * zc;
}

extern "C" {

int pvae_plan_sizeof(int which) { return which == 0 ? (int)sizeof(pvae_plan_args) : fail(-1, "which = 0"); }

size_t pvae_plan_scratch_bytes(const pvae_ctx* c, int32_t horizon, int32_t rows) {
    if (!c || horizon < 1 || rows < 1) { fail(-1, "null ctx, horizon < 1 or rows < 1"); return 0; }
    return plan_scratch_layout(c->L.cfg.latent, horizon, rows, nullptr, nullptr);
}

int pvae_plan_launches(const pvae_ctx* c, int32_t* per_step, int32_t* per_iter, int32_t* closing) {
    if (!c) return fail(-1, "null ctx");
    const int n = imagine_per_step(c, PVAE_IMAGINE_PRIOR, true);
    if (per_step) *per_step = n;
    if (per_iter) *per_iter = 3;                       // candidates, stage, selection
    if (closing) *closing = n + 1;                     // pvae_imagine at horizon 1 without err: its stage + one step
    return 0;
}

int pvae_plan(pvae_ctx* c, const pvae_plan_args* a, void* stream) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!a) return fail(-1, "args is null");
    if (!a->s0.base) return fail(-1, "s0 is null");
    if (!a->targets.base) return fail(-1, "targets is null");
    const int E = a->envs, K = a->candidates, H = a->horizon, iters = a->iters;
    if (E < 1) return fail(-1, "envs %d < 1", E);
    if (K < 1 || K > PVAE_PLAN_MAX_CANDIDATES) return fail(-1, "candidates %d outside [1, %d]", K, PVAE_PLAN_MAX_CANDIDATES);
    const long long rows_ll = (long long)E * K;
    if (rows_ll < 1 || rows_ll > c->L.cfg.max_batch)
        return fail(-1, "rows %lld = envs * candidates outside [1, %d]", rows_ll, c->L.cfg.max_batch);
    if (H < 1) return fail(-1, "horizon %d < 1", H);
    if (iters < 1) return fail(-1, "iters %d < 1", iters);
    if (!(a->sigma >= 0.f) || !std::isfinite(a->sigma)) return fail(-1, "sigma is negative or not finite");
    if (!(a->lam >= 0.f) || !std::isfinite(a->lam)) return fail(-1, "lam is negative or not finite");
    if (a->row0 < 0 || a->row0 + rows_ll > 0xffffffffLL) return fail(-1, "row0 outside the 32-bit Philox row domain");
    const int rows = (int)rows_ll, Db = c->L.cfg.dim_body, Z = c->L.cfg.latent;
    size_t zc_off, u_off;
    const size_t need = plan_scratch_layout(Z, H, rows, &zc_off, &u_off);
    if (!a->scratch || a->scratch_bytes < need) return fail(-1, "scratch is missing or shorter than pvae_plan_scratch_bytes");
    if ((uintptr_t)a->scratch & 15) return fail(-1, "scratch is not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;

    ImagineIo io = imagine_io(c, PVAE_IMAGINE_PRIOR, kZSupplied, rows);
    io.s0 = a->s0; io.targets = a->targets;
    PlanIo p;
    memset(&p, 0, sizeof(p));
    p.E = E; p.K = K; p.H = H; p.sphere = c->L.cfg.prior_kind == PVAE_PRIOR_HYPERSPHERE;
    p.sigma = a->sigma; p.lam = (double)a->lam;
    p.cw = a->col_weight; p.sw = a->step_weight;
    p.seed = a->rng_seed; p.row0 = a->row0;
    p.J = (double*)a->scratch;
    p.zc = (float*)((char*)a->scratch + zc_off);
    float* u = (float*)((char*)a->scratch + u_off);

    float* w = c->ws;
    const int ldo_wm = c->L.net[PVAE_NET_WM].layers.back().n_out_pad;
    const int cand_grid = (int)(((long long)H * rows + 3) / 4);
    int launches = 0;
    for (int i = 0; i < iters; ++i) {
        const bool last = i + 1 == iters;
        p.noise = a->noise ? a->noise + (size_t)i * H * rows * Z : nullptr;
        p.offset = a->rng_offset + (unsigned long long)i * H;
        hipLaunchKernelGGL(plan_candidates_kernel, dim3(cand_grid), dim3(256), 0, st, p, Z, i == 0 ? a->nominal : (const float*)u,
                           last ? a->z_cand : (float*)nullptr, last ? a->noise_out : (float*)nullptr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(plan_stage_kernel, dim3(io.rows_pad / 4), dim3(256), 0, st, io, p);
        HIP_TRY(hipGetLastError());
        launches += 2;
        const auto handover = [&](int t, bool more) {
            hipLaunchKernelGGL(plan_handover_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, io, p,
                               w + c->W.net[PVAE_NET_WM].act.back(), ldo_wm, t, more ? 1 : 0,
                               (last && a->states) ? a->states + (size_t)t * rows * Db : (float*)nullptr);
            HIP_TRY(hipGetLastError());
            return 0;
        };
        if ((rc = imagine_unroll(c, io, H, nullptr, 0, nullptr, handover, st, &launches))) return rc;
        hipLaunchKernelGGL(plan_select_kernel, dim3(E), dim3(256), (size_t)K * (sizeof(double) + sizeof(float)), st, p, Z, u,
                           last ? a->plan_z : (float*)nullptr, last ? a->best : (int*)nullptr, last ? a->cost : (float*)nullptr,
                           a->iter_cost ? a->iter_cost + (size_t)i * E : (float*)nullptr);
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    // the plan's first step once more, on E rows with z = u(0): an imagine prior-mode call of horizon 1
    pvae_imagine_args g;
    memset(&g, 0, sizeof(g));
    g.mode = PVAE_IMAGINE_PRIOR; g.rows = E; g.horizon = 1;
    g.s0 = a->s0;
    g.z.base = u; g.z.ld = Z; g.z.step = (int64_t)E * Z;
    g.actions_out = a->a0; g.states_out = a->s1;
    if ((rc = pvae_imagine(c, &g, stream)) < 0) return rc;
    return launches + rc;
}

}  // extern "C"
