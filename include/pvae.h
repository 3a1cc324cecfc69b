/* pvae.h -- C ABI of libpvae_gfx950.so: the MI355X-native hot path of the PhysicsVAE
 * supervised training loop (world model + conditional VAE).
 *
 * The reference has no FFI on this path: it is pure Python calling stock PyTorch ops
 * (SURVEY.md 8b).  The entry points below are therefore the boundary a maintainer would
 * bind from the reference's own Python (ctypes stub in INTEGRATION.md); each one names
 * the reference code it replaces.  `tpv` = train_physics_vae.py, `tm` = torch_models.py,
 * `rmt` = rllib_model_torch.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every call returns 0 on success, <0 on error; pvae_last_error() gives the text
 *     (thread-local).  No call synchronises the host with the device.
 *   - the CALLER owns every device buffer (parameters, Adam moments, gradients, dataset,
 *     workspace) and passes the hipStream_t (as void*) to launch on.  The library owns
 *     only the opaque pvae_ctx (layout tables + bound pointers).  One ctx per process per
 *     GPU; a ctx is not thread-safe.
 *   - all arithmetic is fp32 (v_mfma_f32_16x16x4_f32 for the contractions).
 *
 * Parameter arena.  The trainable stacks live in ONE flat fp32 arena
 *   [ task encoder | motor decoder | decoder helper | learned prior | world model ]      (TE | MD | MH | PR | WM;
 *   MH and PR are empty segments unless the configuration has them -- see the PVAE_NET_* enum below)
 * each Linear stored as W[n_out_pad][ld] (row-major, ld = n_in rounded up to 64 floats,
 * n_out_pad = n_out rounded up to 64) followed by bias[n_out_pad]; pad entries are zero
 * and stay zero.  The checkpoint tensor `<net>._model.<i>._model.0.weight` of shape
 * [n_out, n_in] (rmt:234-283) is the strided view W[:n_out, :n_in] of that block, so the
 * reference's state_dict layout is the source of truth and no packing pass exists.
 * Gradients and the two Adam moments use arenas of the same layout.
 */
#ifndef PVAE_H
#define PVAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVAE_ABI_VERSION 12

typedef struct pvae_ctx pvae_ctx;

/* PVAE_NET_PR: the learned prior mean `_latent_prior` (rmt:627-635), present only with
 * PVAE_PRIOR_STATE_MEAN.  PVAE_NET_MH: the motor decoder's helper `_motor_decoder_helper` (rmt:670-680, 833-835),
 * present only with pvae_config.mh_depth > 0: a second stack on the decoder's input whose tanh output, scaled by
 * mh_range, is added to the action; the reference's supervised loss sees that term inside a_hat, so the joint phase
 * trains the helper with the decoder (pvae_step_params.adam_t[PVAE_NET_MH] == 0: frozen for this step).  With
 * lookahead > 1 (tpv:367-428) the helper runs in every unrolled step and the WORLD phase trains it too -- the state the
 * world model continues from is its own prediction under the helped action (tpv:417-421) -- as upstream, whose trainer
 * never freezes it.
 * Arena order is TE | MD | MH | PR | WM, so that the stacks trained together in the joint phase form one
 * contiguous segment. */
enum { PVAE_NET_TE = 0, PVAE_NET_MD = 1, PVAE_NET_WM = 2, PVAE_NET_PR = 3, PVAE_NET_MH = 4, PVAE_NUM_NETS = 5 };
/* latent_prior_type (rmt:614-635, 795-819; tpv:384-409).  Only the first runs upstream; the other two
 * follow the specification in oracle/refpath.py (the reference sketches them and crashes):
 *   ZERO_MEAN   "normal_zero_mean_one_std"  KL(N(mu,s^2) || N(0,1))
 *   STATE_MEAN  "normal_state_mean_one_std" KL(N(mu,s^2) || N(mu_p(s_body),1)), mu_p = PR stack (Db -> Z)
 *   HYPERSPHERE "hypersphere_uniform"       encoder emits Z values, z = e/|e|, loss_kl = mean <z, n/|n|>
 *   NONE        latent_prior_type = False   encoder emits Z values that ARE the code: no sampling, no KL term
 *                                           (rmt:622-623, 815-816; a mode the reference runs: pinned by a capture)
 * The non-default kinds need lookahead == 1. */
enum { PVAE_PRIOR_ZERO_MEAN = 0, PVAE_PRIOR_STATE_MEAN = 1, PVAE_PRIOR_HYPERSPHERE = 2, PVAE_PRIOR_NONE = 3 };
enum { PVAE_PHASE_WORLD = 0, PVAE_PHASE_JOINT = 1 };
/* loss_fn of the three reconstruction terms (get_loss_fn tm:97-107; trainer key "loss", tpv:257) */
enum { PVAE_LOSS_MSE = 0, PVAE_LOSS_L1 = 1 };

/* hidden-layer activations (pvae_config.act_kind / layer_act; get_activation_fn rmt:30-46).  "swish" is not
 * offered: upstream it is ray's Swish module with a learnable beta (a parameter outside the five checkpoint
 * files' Linear tensors), and it needs the pre-activation in the backward pass.  PVAE_ACT_LINEAR: no
 * activation after a hidden layer (rmt:32-33 "linear" / None), per-layer use only. */
enum { PVAE_ACT_RELU = 0, PVAE_ACT_TANH = 1, PVAE_ACT_SIGMOID = 2, PVAE_ACT_ELU = 3, PVAE_ACT_LINEAR = 4 };
#define PVAE_MAX_HIDDEN 15 /* hidden layers per stack */

/* flags for pvae_forward_backward */
enum {
    PVAE_FLAG_FUSED_ADAM = 1, /* apply Adam inside the backward launches (1 GPU): in the weight-
                               * gradient epilogue, or -- when a gradient arena is bound -- deferred by
                               * one launch to extra workgroups, the arena serving as scratch (its
                               * contents are unspecified afterwards); same arithmetic either way  */
    PVAE_FLAG_NO_BACKWARD = 2 /* forward + losses only (tm:147-156 test loop, parity probes) */
};

/* Architecture.  Mirrors the dict keys of tpv:247-286 / gen_layers tpv:180-192:
 * TE: 2*Db -> te_width x te_depth -> 2*Z (Z with PVAE_PRIOR_HYPERSPHERE) ; MD: Db+Z -> ... -> Da ;
 * WM: Db+Da -> ... -> Db ; PR (PVAE_PRIOR_STATE_MEAN): Db -> pr_width x pr_depth -> Z.
 * act_kind after every hidden layer (ReLU unless set), linear output layer. */
typedef struct pvae_config {
    int32_t dim_body;   /* Db */
    int32_t dim_action; /* Da */
    int32_t latent;     /* Z  */
    int32_t te_width, te_depth;
    int32_t md_width, md_depth;
    int32_t wm_width, wm_depth;
    int32_t max_batch;  /* largest minibatch (rows) this ctx will be asked to process */
    int32_t lookahead;  /* L >= 1: steps unrolled through the world model per sample (tpv:277,
                           367-428); sizes the workspace (L blocks per panel) */
    int32_t prior_kind; /* PVAE_PRIOR_* (0 = the reference's working default)                 */
    int32_t pr_width, pr_depth; /* learned prior stack (PVAE_PRIOR_STATE_MEAN only; else ignored) */
    int32_t act_kind;   /* PVAE_ACT_*: hidden activation of every stack = the trainer's "act_fn" (tpv:262;
                           get_activation_fn rmt:30-46).  0 = relu, so a zeroed field keeps the default */
    /* Stacks gen_layers cannot emit but FC accepts (rmt:234-270: any list of fc layers, each with its own
     * hidden_size and activation; reached through custom_model_config's *_layers, rmt:462-510).  Indexed
     * [PVAE_NET_*][hidden layer]; zeroed = the uniform stack described by <net>_width / act_kind. */
    int32_t layer_width[PVAE_NUM_NETS][16]; /* > 0: width of that hidden layer instead of <net>_width    */
    int32_t layer_act[PVAE_NUM_NETS][16];   /* > 0: 1 + PVAE_ACT_* of that hidden layer instead of act_kind */
    /* `task_encoder_inputs` / `motor_decoder_inputs` (rmt:470, 485; 607-613, 646-653, 776-783, 822-829): which of
     * (body, task) the encoder reads -- s_t, s_{t+1} -- and which of (body, task) the decoder reads -- s_t, z.
     * PVAE_INPUT_* bits; 0 = both (a zeroed field keeps the default).  A subset is a COLUMN WINDOW of the same
     * first-layer weight block: the block keeps its full-width layout [body | task], the columns outside the window
     * are structural zeros (never touched by initialisation or checkpoints, and kept exactly zero by training: the
     * staged input panels hold zeros there, so their weight gradient is exactly zero); pvae_layer_info reports the
     * window (n_in, col0), so a checkpoint tensor has the reference's shape. */
    int32_t te_inputs, md_inputs;
    /* motor_decoder_helper_enable / _layers / _range (rmt:490-498): mh_depth hidden layers (0: no helper) of mh_width
     * (layer_width / layer_act[PVAE_NET_MH] per layer), an output layer of dim_action values ending in tanh, input =
     * the decoder's (md_inputs applies); needs mh_range > 0 (asserted upstream, rmt:672-673). */
    int32_t mh_width, mh_depth;
    float mh_range;
} pvae_config;
#define PVAE_INPUT_BODY 1
#define PVAE_INPUT_TASK 2

typedef struct pvae_layer_info {
    int32_t net;       /* PVAE_NET_*                                    */
    int32_t index;     /* position inside the stack (0 = first Linear)  */
    int32_t n_in;      /* checkpoint shape is [n_out, n_in]             */
    int32_t n_out;
    int32_t ld;        /* row stride of W in floats (n_in padded to 64) */
    int32_t n_out_pad; /* rows allocated (n_out padded to 64)           */
    int64_t w_offset;  /* float offset of W[0][0] in the arena          */
    int64_t b_offset;  /* float offset of bias[0] in the arena          */
    int32_t act;       /* PVAE_ACT_* applied to this layer's output (PVAE_ACT_LINEAR for the output layer) */
    int32_t col0;      /* first column of the checkpoint tensor inside the block's rows: W[r][c] of the checkpoint is
                          arena[w_offset + r * ld + col0 + c] (non-zero only for a first layer on an input subset) */
} pvae_layer_info;

/* Loss weights and Adam hyper-parameters of one optimizer step.
 * tpv:331-335 (phase coefficients), tm:119-122 (Adam defaults), tm:158-159 (lr from StepLR). */
typedef struct pvae_step_params {
    float a_rec_coeff;     /* motor_decoder_a_rec_coeff (1.0)  */
    float kl_coeff;        /* vae_kl_coeff (beta)              */
    float s_rec_coeff;     /* world_model_s_rec_coeff: weight of MSE(s2, WM(s1, a_gt)) (tpv:411-414) in BOTH phases
                              (1.0 in the world phase, tpv:331-335; the trainer's joint default is 0.0, tpv:284) */
    float cycle_coeff;     /* vae_cycle_coeff (1e-3)           */
    double lr;             /* learning rate of this epoch (double: torch keeps these as   */
    double beta1, beta2, adam_eps; /* Python floats; 1 - beta and the bias corrections are   */
                           /* formed in double before rounding to fp32)               */
    int32_t adam_t[PVAE_NUM_NETS]; /* 1-based Adam step count per net for THIS update */
    int32_t global_rows;   /* rows of the global minibatch (= rows on 1 GPU); losses and
                              gradients are scaled by 1/global_rows so a sum all-reduce over
                              ranks yields the reference's batch-mean gradient */
    uint64_t rng_seed;     /* Philox key when eps == NULL      */
    uint64_t rng_offset;   /* (global step, first global row) -> counter */
    int32_t loss_kind;     /* PVAE_LOSS_MSE (nn.MSELoss, the trainer's setting) or PVAE_LOSS_L1 */
    float weight_decay;    /* torch.optim.Adam's L2 term: g <- g + weight_decay * p before the moments
                              (tm:119-122; the trainer's config holds 0.0, tpv:253) */
} pvae_step_params;

/* ---- layout queries (pure host arithmetic, no GPU needed) --------------------------- */
int pvae_abi_version(void);
const char* pvae_last_error(void);
int pvae_num_layers(const pvae_config* cfg);
int pvae_layer(const pvae_config* cfg, int i, pvae_layer_info* out);
int64_t pvae_arena_floats(const pvae_config* cfg);
/* contiguous [offset, offset+count) of one net inside the arena */
int pvae_net_segment(const pvae_config* cfg, int net, int64_t* offset, int64_t* count);
size_t pvae_workspace_bytes(const pvae_config* cfg);
/* Float offset of a workspace panel (inspection / tests).  kind: 0 = input panel of `net`
 * [Bp][ld0], 1 = its gradient, 2 = output of layer `layer` [Bp][n_out_pad], 3 = gradient wrt the
 * pre-activation of that layer, 4 = target next-state panel, 5 = target action panel,
 * 6 = eps [Bp][Z], 7 = dense copy [rows][2 Db] of the observation rows of the last pvae_infer /
 * pvae_infer_logits call with <= 4 rows (what a deferred read of that forward -- mu / logvar, the
 * world model's prediction, the value estimate -- re-uses, so the caller may recycle its buffer).
 * Bp = max_batch rounded up to 32.  Returns <0 on bad arguments.
 * (Kinds 0, 4, 5 name the FIRST of the two sets of staging panels; pvae_train_step_prefetch /
 * pvae_dp_train_step alternate between the two, so inspect these panels only around the plain
 * pvae_gather / pvae_set_batch entry points.) */
int64_t pvae_workspace_offset(const pvae_config* cfg, int kind, int net, int layer);

/* ---- context ------------------------------------------------------------------------ */
int pvae_create(const pvae_config* cfg, pvae_ctx** out);
void pvae_destroy(pvae_ctx* ctx);
/* params / grads / exp_avg / exp_avg_sq: device arenas of pvae_arena_floats() floats.
 * Replaces the per-tensor storage of nn.Linear + torch.optim.Adam state (tm:119-122). */
int pvae_bind_arenas(pvae_ctx* ctx, float* params, float* grads, float* exp_avg,
                     float* exp_avg_sq);
/* workspace: device buffer of at least pvae_workspace_bytes() bytes, 256-byte aligned.  It must be ZERO-FILLED when it is
 * bound, and the caller must not write it afterwards (reading panels through pvae_workspace_offset is fine).  Two things
 * rely on that: the 64 floats at its end that no launch ever writes and that a gathered first-layer operand reads as its
 * "no source" columns (pvae_set_direct), and the pad columns of the gradient-seed panels outside the range the library
 * clears itself on the first backward pass after a bind -- the seed epilogues write the real columns only, and whole
 * padded tiles are contracted over both.  Everything else the library keeps out of its sums on its own, whatever earlier
 * calls (of any row count, any phase, pvae_infer included) left behind: held by tests/test_gpu_step_history.py; that no
 * launch reads into a result or writes outside the bytes counted here, by tests/test_gpu_step_guards.py. */
int pvae_bind_workspace(pvae_ctx* ctx, void* workspace, size_t bytes);
/* Demonstration set resident in HBM, de-duplicated: states[n_rows][Db], actions[n_rows][Da]
 * (fp32, dense), window_row[n_windows] = row of s_t (s_{t+1} is row+1, a_t is the same row;
 * with lookahead L the window spans rows row .. row+L, which must stay inside one episode).
 * Replaces the float64 X[N,1,2Db] / Y[N,1,Da] arrays of load_dataset_for_PhysicsVAE
 * (tpv:117-164) and DatasetBase.__getitem__ (tm:52-56). */
int pvae_bind_dataset(pvae_ctx* ctx, const float* states, const float* actions,
                      const int32_t* window_row, int64_t n_rows, int64_t n_windows);
/* Optional, after pvae_bind_dataset: `next_states` [n_rows][Db] fp32, row-aligned with `states`; row r
 * holds what follows state r in a window -- the second half of x and the state-reconstruction target
 * are then read from next_states[row] instead of states[row + 1].  This is how cond = "rel" of
 * load_dataset_for_PhysicsVAE (tpv:149-150: x = [s_t | s_{t+1} - s_t]) reaches the gather kernel: the
 * differences are formed once in float64 on the host, as the reference does.  NULL restores the
 * default; a new pvae_bind_dataset resets it. */
int pvae_bind_dataset_next(pvae_ctx* ctx, const float* next_states);
/* First layers that read the demonstration set where it lies (the torch.cat sites tpv:377, rmt:829, 842
 * as address arithmetic inside the kernels' loaders).  The training-step entry points (pvae_train_step, _prefetch,
 * pvae_dp_train_step) stage NOTHING when the step qualifies: the first layer of every stack fetches its rows of
 * `states` / `actions` itself (16-byte chunks from 4-byte-aligned rows), the z / a_hat column blocks come from where the
 * sampler / the decoder left them, and the two targets s_{t+1}, a_t are read from the set by the loss epilogues.  A step
 * qualifies at lookahead 1 with the default prior, more than 4 rows, first layers wide enough for the 32x32 / 64-row
 * tile kernels, no `next_states` array, and dataset allocations that are readable 16 bytes past their last row (checked
 * at pvae_bind_dataset with hipMemGetAddressRange: a chunk may reach 12 bytes past a row).  What those bytes hold reaches
 * no result: the one joint-phase minibatch whose last window ends on the very last row of `states` stages its panels when
 * 2 * dim_body is no multiple of 4 (the encoder's operand would otherwise end in a chunk whose tail lies behind the array,
 * and a NaN pattern there survives the multiplication by the weight block's zero pad columns).  Everything else -- and
 * pvae_gather / pvae_set_batch + pvae_forward_backward always -- goes through the staging launch as before; both paths
 * give the same bits.  OPT-IN: pvae_set_direct(ctx, 1) (default off -- at BASELINE's 256 rows per GPU the staged step is
 * the faster one: its gather rides in the previous step's last launch); pvae_direct_active tells
 * whether a step with these arguments would take the direct path (1 / 0). */
int pvae_set_direct(pvae_ctx* ctx, int on);
/* Switches of schedule and tile geometry.  The library reads NO environment variable: what rounds 1-4 switched through
 * PVAE_* variables is set here (the Python host, physicsvae_amd/engine.py, still maps those variables onto these calls for
 * the tests and the A/B scripts).  Defaults are the production values.
 *   ctx == NULL, process-wide kernel geometry:  "ws64" "ws6464" "ws6464_rows" "pair64" "dgrad16" (0 / 1), "wgrad32" (0 / 1 / 2),
 *       "krot" "rowxcd" (0 / 1, experiments, default 0), "look_pair" "rollout_fused" (0 / 1),
 *       "fc_per_stack" (0 / 1: the stack set's launches one per stack instead of one per layer depth, see pvae_fc_* below),
 *       "p2p_timeout_ms" (> 0: the bounded waits of the stack sets' PPO gradient exchange, pvae_fc_ppo_peer_*)
 *   ctx, that context's schedule:  "pair" "defer_adam" "same_layer" "fold_sampler" (0 / 1), "direct" (= pvae_set_direct),
 *       "p2p_timeout_ms" (> 0), "p2p_selftest_flags_only" (0 / 1), "server_mailbox" (0 auto, 1 pinned host memory, 2 device)
 * Every variant gives the same bits as the default (held by tests/test_gpu_shapes.py, test_gpu_fuzz.py).  -1: unknown name.
 *   ctx, not a schedule switch:  "joint_s_rec" (0 / 1, default 0): the joint phase accepts pvae_step_params.s_rec_coeff != 0
 *       (see pvae_forward_backward).  A context that has not opted in keeps refusing that combination with -4, as every
 *       context did before the term was built; the supervised trainer opts in when its config holds a non-zero
 *       world_model_s_rec_coeff.
 *   "ppo_priors" (0 / 1, default 0): the PPO passes of PhysicsVAE (pvae_ppo_step / _sgd / _grad / _apply / _evaluate /
 *       _prepare / _act) also run under the priors STATE_MEAN and HYPERSPHERE (see "PPO learner step of PhysicsVAE").  A
 *       context that has not opted in keeps answering -1 with the message every context gave before they were built. */
int pvae_set_option(pvae_ctx* ctx, const char* name, int64_t value);
int pvae_direct_active(pvae_ctx* ctx, int phase, int32_t rows, const pvae_step_params* sp, int fused);

/* ---- hot path ------------------------------------------------------------------------ */
/* Minibatch gather: windows [first_window, first_window+rows) -> network input panels.
 * Replaces DataLoader + default collate over DatasetBase (tm:166-175, 137-139). */
int pvae_gather(pvae_ctx* ctx, int64_t first_window, int32_t rows, void* stream);
/* Declare the staging panels dirty: the staged training minibatch and a minibatch gathered ahead
 * (pvae_train_step_prefetch) are forgotten, so the next training call gathers again and
 * pvae_forward_backward without a new gather fails with "staged rows" instead of running on
 * overwritten panels.  Needed by callers that replay a captured HIP graph of pvae_infer: the graph
 * writes the panels that were current when it was captured, and the host-side bookkeeping of
 * pvae_infer does not run on replay.  Host-side only; launches nothing. */
int pvae_invalidate_staging(pvae_ctx* ctx);
/* Same, from explicit device tensors x[rows][L][2*Db], y[rows][L][Da] (dense fp32, L =
 * lookahead): the compute_loss(y, x) entry of tpv:361 for callers that bring their own batch. */
int pvae_set_batch(pvae_ctx* ctx, const float* x, const float* y, int32_t rows, void* stream);

/* Forward + losses (+ backward, + optional fused Adam) over the batch staged by
 * pvae_gather/pvae_set_batch.  Replaces compute_loss (tpv:361-435), PhysicsVAE.forward
 * (rmt:742-853), loss.backward() (tm:142) and, with PVAE_FLAG_FUSED_ADAM,
 * optimizer.step() (tm:143).
 *   eps      : device [L][rows][Z] standard-normal draws for the reparameterisation
 *              (rmt:734-740; one [rows][Z] slice per unrolled step, in call order), or NULL to
 *              draw them on chip (Philox4x32-10, Box-Muller; step t uses rng_offset + t).
 *   loss_out : device float[5] = {total, loss_a, loss_kl, loss_s, loss_cyc} (this rank's
 *              share: sums over local rows / global_rows).
 * World phase, lookahead 1: only the world model runs (the reference's discarded TE/MD/VB
 * forward, tpv:378, is not algorithmically required and is skipped).
 * lookahead L > 1 (tpv:367-428): step t+1 starts from the world model's own prediction of step
 * t, so encoder, sampler, decoder and world model run for every step in BOTH phases, the
 * backward pass walks the steps last to first through all three stacks, and each layer's weight
 * gradient is one contraction over the L stacked steps.  Terms are means over the L steps.
 * Joint phase with s_rec_coeff > 0 (tpv:411-414 while the world model is frozen, tpv:347-350; the context has opted in
 * with pvae_set_option(ctx, "joint_s_rec", 1), else -4): the world model also runs
 * on the DEMONSTRATED action.  At lookahead 1 its inputs are data: a forward-only pass before the decoder's action
 * overwrites the input panel's action columns, loss_s in loss_out, no gradient -- encoder and decoder gradients are the
 * bits of the same step with s_rec_coeff = 0.  At lookahead > 1 the state of step t >= 1 is a prediction: the pass of
 * step t is followed by an input-gradient-only chain whose state columns join the other consumers of step t-1's
 * prediction.  In neither case is a weight gradient, an Adam update or a gradient-arena write made for the world
 * model, and the stages pvae_backward_plan reports as finishing a slice are those of s_rec_coeff = 0. */
int pvae_forward_backward(pvae_ctx* ctx, int phase, int32_t rows, const pvae_step_params* sp,
                          const float* eps, float* loss_out, int flags, void* stream);
/* Adam over the nets in net_mask (bit n = PVAE_NET_n) using the bound grads arena.
 * Replaces torch.optim.Adam.step (tm:143) for the data-parallel path (after the gradient
 * all-reduce). */
int pvae_adam(pvae_ctx* ctx, int net_mask, const pvae_step_params* sp, void* stream);

/* Staged variant for data-parallel training (overlap of the gradient all-reduce with backward):
 *   pvae_forward_seed          forward + loss partials + gradient seeds (no backward launches)
 *   pvae_backward_stage(k)     launch k of the backward pass, k = 0 .. *num_stages-1 in order;
 *                              [*ready_offset, +*ready_count) is the slice of the GRADIENT arena
 *                              (net *ready_net) that is final after this stage (count 0: none) --
 *                              the caller may start its all-reduce immediately; loss_out (may be
 *                              NULL) is finalised by the last stage
 *   pvae_adam_segment          Adam on one such slice once its reduction has completed
 * Together they replace loss.backward() + optimizer.step() (tm:142-143) on N GPUs. */
int pvae_forward_seed(pvae_ctx* ctx, int phase, int32_t rows, const pvae_step_params* sp, const float* eps,
                      void* stream);
int pvae_backward_stage(pvae_ctx* ctx, int phase, int32_t rows, const pvae_step_params* sp, int stage,
                        float* loss_out, void* stream, int64_t* ready_offset, int64_t* ready_count,
                        int* ready_net, int* num_stages);
int pvae_adam_segment(pvae_ctx* ctx, int net, int64_t offset, int64_t count, const pvae_step_params* sp,
                      void* stream);
/* The backward pass of a (phase, sp) step as pvae_backward_stage would walk it, WITHOUT launching anything: stage k
 * finishes the slice [offset[k], +count[k]) of net[k] (count 0: none).  At most `max` entries are written; *num_stages
 * is the total.  Does not depend on the rows of the minibatch nor on what is staged -- so a rank whose shard of a ragged
 * last global minibatch is EMPTY (no launch at all on it) can issue the very sequence of collectives its peers issue
 * behind their stages (tm:142-143 on N GPUs; physicsvae_amd/torch_models.py dp_step). */
int pvae_backward_plan(pvae_ctx* ctx, int phase, const pvae_step_params* sp, int64_t* offset, int64_t* count, int* net,
                       int max, int* num_stages);

/* Data-parallel exchange issued by the library itself (RCCL over xGMI; one process per GPU).
 * Replaces what DistributedDataParallel would add around tm:142-143; the reference has no
 * multi-GPU path (tm:115-118 moves one model to one device).
 *   pvae_comm_unique_id   rank 0: 128-byte RCCL id, to be handed to every rank by the caller
 *                         (torch.distributed broadcast, a file, MPI ...)
 *   pvae_comm_init        collective: every rank joins the communicator (rank, world, id)
 *   pvae_allreduce_grads  in-place SUM all-reduce of a slice of the gradient arena, stream-ordered
 *                         on `stream` like any other launch of this library (no side stream)
 *   pvae_dp_train_step    one data-parallel optimizer step in ONE call: gather + forward +
 *                         backward (gradients scaled by 1/global_rows) + all-reduce + Adam.
 *                         Default: one reduction per stack, in line on `stream` as soon as the
 *                         stack's gradient is final (no cross-stream hand-off: one costs
 *                         ~18 us of idle GPU each way on this runtime).
 *                         With bucket_bytes > 0 (pvae_comm_config) the exchange is bucketed
 *                         and overlapped instead: a stack's gradient becomes final last layer
 *                         first, and every time whole layers worth bucket_bytes are done
 *                         that bucket is reduced and Adam-applied on the library's own
 *                         high-priority exchange stream while `stream` keeps launching the
 *                         rest of the backward pass; `stream` rejoins (event wait) before the
 *                         call returns.  Bucket boundaries depend on the layout and
 *                         bucket_bytes only -- identical on every rank.  rows may be 0 (empty
 *                         shard of a ragged last global batch);
 *                         [next_first, +next_rows) = this rank's shard of the following step
 *                         (0 rows: unknown), gathered inside this step's last launch as in
 *                         pvae_train_step_prefetch.
 * The RCCL library is resolved at run time (the copy PyTorch already loaded, else the system
 * one); a missing library is an error from these calls only. */
int pvae_comm_unique_id(void* id128);
int pvae_comm_init(pvae_ctx* ctx, int rank, int world, const void* id128);
int pvae_comm_destroy(pvae_ctx* ctx);
/* What the ctx's communicator itself reports (ncclCommUserRank / ncclCommCount): *nranks = 0 when
 * the ctx has no communicator.  bench.py prints this as `rccl_ranks`, so that the number of ranks
 * in the JSON line comes from RCCL and not from a command-line flag. */
int pvae_comm_info(pvae_ctx* ctx, int* rank, int* nranks);
/* Exchange settings of pvae_dp_train_step (same values on every rank): bucket_bytes = 0: one bucket per
 * stack, reduced in line on the caller's stream; > 0: buckets of that size, reduced and applied on the
 * library's exchange stream while the backward pass continues.  Until this is called (or
 * PVAE_DP_BUCKET_MB is set at pvae_comm_init) the library chooses per step: in line with one rank and in
 * the world phase, 6 MiB overlapped buckets in the joint phase with more than one rank (the decoder's
 * reduction then hides behind the encoder's backward pass); test_delay_us > 0 puts a spin kernel of that length in
 * front of every reduction (ordering tests).  Overlap pays when the backward work still to be
 * launched after a bucket closes exceeds the two hand-offs (long stacks, lookahead > 1, slow
 * links); with the caller on the NULL stream also set GPU_MAX_HW_QUEUES=8 before HIP starts --
 * with the default 4 hardware queues the exchange stream can share one with the NULL stream and
 * every hand-off then stalls ~250 us. */
int pvae_comm_config(pvae_ctx* ctx, int64_t bucket_bytes, int32_t test_delay_us);
/* How pvae_dp_train_step exchanges a bucket (same value on every rank, chosen before the first step
 * and not changed afterwards):
 *   PVAE_EXCHANGE_ALLREDUCE (default)  ncclAllReduce of the gradient, then every rank applies the same
 *                                      Adam update to the whole bucket (replicated moments);
 *   PVAE_EXCHANGE_SHARDED              ncclReduceScatter (rank r ends with the summed gradient of ITS
 *                                      1/N slice), Adam on that slice only (1/N of the p, g, m, v
 *                                      traffic per rank), ncclAllGather of the updated parameter
 *                                      slices.  Each rank then holds valid Adam moments for its own
 *                                      slice only (ZeRO-1 shaped).  Buckets whose length is not a
 *                                      multiple of 4*N floats fall back to the all-reduce form.
 *   PVAE_EXCHANGE_P2P                  no RCCL: the direct all-pairs exchange of SURVEY.md section 8e over
 *                                      peer-mapped arenas (pvae_p2p_export / pvae_p2p_open below).  ONE
 *                                      launch per bucket: rank r signals "my gradient is final", waits for
 *                                      every peer's signal, reads slice r of every rank's gradient arena
 *                                      directly (7 links in parallel on an 8-GPU xGMI mesh), sums in RANK
 *                                      ORDER (so every element is reduced once, by its owner, the same way:
 *                                      replicas stay bit-identical by construction), applies Adam to its
 *                                      slice and writes the updated parameters straight into every peer's
 *                                      parameter arena; the last workgroup tells the peers it is done and
 *                                      waits for theirs.  Moments as in the sharded form (ZeRO-1 shaped).
 * PVAE_DP_SHARDED=1 in the environment selects the sharded form at pvae_comm_init. */
enum { PVAE_EXCHANGE_ALLREDUCE = 0, PVAE_EXCHANGE_SHARDED = 1, PVAE_EXCHANGE_P2P = 2,
       PVAE_EXCHANGE_LOCAL = 3 /* MEASUREMENT ONLY: no exchange at all, every rank applies Adam to its own
                                  gradient (replicas diverge) -- the step time without the collective, against
                                  which bench.py reports what an exchange adds */,
       PVAE_EXCHANGE_P2P_PUSH = 4 /* PVAE_EXCHANGE_P2P with remote WRITES only: every rank pushes its contribution to
                                  slice q into owner q's staging buffer, the owner sums its slice from LOCAL memory in
                                  rank order, applies Adam and pushes the parameters (same result bit for bit; links
                                  that favour posted writes over read round trips want this form) */ };
int pvae_comm_mode(pvae_ctx* ctx, int mode);
/* Peer-mapped exchange (PVAE_EXCHANGE_P2P).  The reference has no counterpart (tm:131-161 is one process);
 * this is what `north_star` asks for on top of it.  Set-up, after pvae_bind_arenas:
 *   pvae_p2p_export   writes PVAE_P2P_BLOB_BYTES describing this rank's gradient arena, parameter arena, flag
 *                     block and staging buffer (hipIpcGetMemHandle of the allocations they live in + offsets).  The arenas
 *                     must come from hipMalloc (PyTorch's default allocator does; expandable segments do not).
 *   (caller)          all-gathers the blobs of all ranks, by any transport (torch.distributed, a file, MPI)
 *   pvae_p2p_open     collective in effect: maps every peer's three buffers (hipIpcOpenMemHandle) -- peers may
 *                     be other GPUs of the node (xGMI) or other processes on the SAME device (functional tests
 *                     on a 1-GPU box).  world <= PVAE_P2P_MAX_RANKS.
 *   pvae_p2p_status   *timeouts = waits that gave up (a peer never signalled within the time-out, default 20 s,
 *                     PVAE_P2P_TIMEOUT_MS): results are then garbage and the caller must stop.  Synchronises
 *                     `stream`.  *rank / *world as passed to pvae_p2p_open (0 ranks: not open).
 * pvae_dp_train_step then runs with or without an RCCL communicator. */
#define PVAE_P2P_BLOB_BYTES 512
#define PVAE_P2P_MAX_RANKS 8
int pvae_p2p_export(pvae_ctx* ctx, void* blob);
int pvae_p2p_open(pvae_ctx* ctx, int rank, int world, const void* blobs);
int pvae_p2p_close(pvae_ctx* ctx);
int pvae_p2p_status(pvae_ctx* ctx, int* rank, int* world, uint32_t* timeouts, void* stream);
/* Collective in effect (every rank calls it after pvae_p2p_open): (1) each rank writes a record into every peer's flag
 * block, signals, checks the records that arrived in its own block and reads its records back from the peers' --
 * remote write, remote read and flag delivery are proven (or fail within 1 s) before the first training step;
 * (2) the CACHED arenas, through the exchange's own access paths: a test region of the parameter arena and of the
 * staging buffer is first read into this device's L2s from every XCD (LDS-DMA and plain loads, what the forward
 * kernels use), the peers overwrite it with the exchange's `buffer_store ... sc0 sc1`, and a fresh dependent launch
 * re-reads it from every XCD -- a stale line is an error; a gradient line is read remotely, overwritten by its owner
 * and read again (reader-side staleness).  The regions are restored.  A failure (-22) means this machine must not
 * run the peer-mapped forms: replicas would stay bit-identical while training on stale weights.
 * PVAE_P2P_SELFTEST_FLAGS_ONLY=1 skips (2).  Synchronises `stream`. */
int pvae_p2p_selftest(pvae_ctx* ctx, void* stream);
/* Zero the count pvae_p2p_status reports (after the caller has handled the time-outs, e.g. dropped a calibration
 * candidate and restored its snapshot).  Since ABI 7 a wait that gives up also ABORTS that rank's part of the
 * exchange launch: no gradient is summed, no moment moves, nothing is pushed to the peers.  Synchronises `stream`. */
int pvae_p2p_clear_errors(pvae_ctx* ctx, void* stream);
/* One bucket through the peer-mapped exchange, stream-ordered like any launch of this library: the slice
 * [offset, offset + count) of the gradient arena (inside stack `net`, float4-aligned) is summed over the ranks
 * by its owners, Adam-applied and the updated parameters written to every rank -- what pvae_dp_train_step does
 * per bucket in PVAE_EXCHANGE_P2P mode.  Every rank must issue the same sequence of calls. */
int pvae_p2p_exchange(pvae_ctx* ctx, int net, int64_t offset, int64_t count, const pvae_step_params* sp,
                      void* stream);
/* Which ranges of the arenas THIS rank keeps valid Adam moments for, for stack `net` trained in `phase`, under the
 * current exchange mode and bucket settings: one entry per exchange bucket -- the rank's slice of it (sharded / peer-
 * mapped forms; replicated[i] = 0) or the whole bucket (all-reduce form and buckets that fall back to it;
 * replicated[i] = 1: every rank holds the same values).  What a checkpoint writer needs to assemble full moments
 * (physicsvae_amd TrainModel.gather_moments).  *n entries are written (at most `max`). */
int pvae_owned_slices(pvae_ctx* ctx, int phase, int net, int64_t* offsets, int64_t* counts, int32_t* replicated,
                      int32_t max, int32_t* n);
int pvae_allreduce_grads(pvae_ctx* ctx, int64_t offset, int64_t count, void* stream);
int pvae_dp_train_step(pvae_ctx* ctx, int phase, int64_t first_window, int32_t rows,
                       const pvae_step_params* sp, const float* eps, float* loss_out,
                       int64_t next_first, int32_t next_rows, void* stream);

/* One whole optimizer step on the bound dataset: gather + forward/backward + Adam.
 * This is the body of the `for data in self.train_loader` loop (tm:137-144). */
int pvae_train_step(pvae_ctx* ctx, int phase, int64_t first_window, int32_t rows,
                    const pvae_step_params* sp, const float* eps, float* loss_out, void* stream);

/* pvae_train_step that also gathers the NEXT minibatch (windows [next_first, +next_rows), 0 rows:
 * none): the gather rides as extra workgroups in this step's last launch and lands in a second set
 * of input panels; the following call finds its minibatch already staged and skips the gather
 * launch (falls back to a normal gather whenever what was prefetched is not what is asked for).
 * Same results as pvae_train_step, one launch less per step (lookahead 1). */
int pvae_train_step_prefetch(pvae_ctx* ctx, int phase, int64_t first_window, int32_t rows,
                             const pvae_step_params* sp, const float* eps, float* loss_out,
                             int64_t next_first, int32_t next_rows, void* stream);

/* ---- inspection (parity tests) ------------------------------------------------------- */
/* Copy a forward intermediate of the last pvae_forward_backward into dst (dense
 * [rows][width] fp32, device).  what: 0 = mu, 1 = logvar, 2 = z, 3 = a_hat (MD output),
 * 4 = s2_hat (WM output; with lookahead > 1 the prediction that feeds the next step), 5 = eps
 * actually used (PVAE_PRIOR_HYPERSPHERE: the unit prior sample u), 6 = prior mean mu_p
 * (PVAE_PRIOR_STATE_MEAN).  With PVAE_PRIOR_HYPERSPHERE 0 reads the raw encoder output e, 2 the
 * unit vector z = e/|e|, and 1 is not available.  Add 8*t to read time step t of a
 * lookahead > 1 batch. */
int pvae_read_tensor(pvae_ctx* ctx, int what, float* dst, int32_t rows, void* stream);

/* Rollout inference (rmt:742-771 at small batch): obs[rows][2*Db] -> a_hat[rows][Da]
 * (+ optional s2_hat[rows][Db], mu/logvar/z).  eps NULL + noise=0 -> z = mu
 * (latent_prior_noise False). */
int pvae_infer(pvae_ctx* ctx, const float* obs, int32_t rows, const float* eps, int noise,
               uint64_t rng_seed, uint64_t rng_offset, float* a_hat, float* s2_hat, float* z_out,
               void* stream);
/* 1 when calls of <= 4 rows take the rollout path that keeps the observation rows for deferred reads (rmt:742-771's
 * _cur_* state) and leaves a staged training minibatch alone; 0 under PVAE_ROLLOUT_FUSED=0 (read once per process by
 * the LIBRARY: callers ask here instead of reading the environment themselves). */
int pvae_rollout_is_fused(void);
/* pvae_infer with the module's output layout (rmt:742-771 + AppendLogStd rmt:160-206): the action lands in
 * logits[r * ld_logits + 0 .. Da) and, when log_std (device, [Da]) is given, log_std behind it --
 * logits = [a_hat | log_std], what PhysicsVAE.forward returns to RLlib's action distribution. */
int pvae_infer_logits(pvae_ctx* ctx, const float* obs, int32_t rows, const float* eps, int noise,
                      uint64_t rng_seed, uint64_t rng_offset, float* logits, int32_t ld_logits,
                      const float* log_std, float* s2_hat, float* z_out, void* stream);
/* ---- call-persistent rollout server (the single-launch rollout path) ------------------------
 * Replaces, for the 30 Hz control loop's forward at B = 1, PhysicsVAE.forward (rmt:742-771: task encoder ->
 * sampler rmt:734-740 -> motor decoder; callers envs/rllib_env_imitation.py:215-266) by ZERO launches per call: one
 * kernel stays resident on the 32 CUs of one XCD with the encoder's and the decoder's weights in LDS (1/32 of every
 * layer's output features per workgroup), polls a mailbox in pinned host memory, walks the layers -- every value handed
 * from a layer to the next as one tagged 8-byte word that the consumer polls in that XCD's L2, no barrier -- and writes
 * the action back to the mailbox.  All pointers below are HOST pointers; the
 * calls are plain host functions (no stream, no launch) once the server runs.
 *   pvae_rollout_server_start   plans the LDS layout, allocates the mailbox and launches the kernel on a stream of its own;
 *                               returns once it serves.  scope 0: one XCD (32 workgroups; the other seven XCDs stay free
 *                               for training launches) when 1/32 of every layer fits a CU's LDS, else the whole chip (256
 *                               workgroups, 1/256 of every layer each: 4x1024 stacks take 122 KB per CU -- kernels that
 *                               need more than the remaining LDS then wait for the server to leave); 1 / 2 force either
 *                               (PVAE_SERVER_SCOPE=xcd|chip as well).  A hand-over word costs 0.43-0.53 us inside an XCD,
 *                               0.51-0.64 us across XCDs (tools/xcd_pingpong.hip).  -24 with a message when nothing fits.  The kernel
 *                               leaves by itself after idle_timeout_ms without a request (default 100 ms; the next
 *                               pvae_rollout_server_infer brings it back) and never lives longer than lifetime_s
 *                               (default 600 s).  Arguments <= 0 keep the current / default values.  While it is
 *                               resident a DEVICE-wide synchronisation waits for it (at most the idle time-out).
 *   pvae_rollout_server_infer   obs[2*Db] -> a_hat[Da] (+ mu_logvar[2*Z], z[Z] when not NULL): the same values as
 *                               pvae_infer(rows = 1, eps = NULL, noise, rng_seed, rng_offset), bit for bit.  reload != 0:
 *                               the weights are copied from the parameter arena into LDS again first (after an
 *                               optimizer step or load_weights*, rmt:870-928).  Blocks at most timeout_ms (<= 0: 1 s).
 *                               Optimizer steps issued through THIS library (pvae_train_step*, pvae_dp_train_step,
 *                               pvae_adam*, pvae_p2p_exchange) are noticed: the next request waits for their stream and
 *                               re-reads the weights by itself.  Parameters written behind the library's back (a
 *                               framework's load_state_dict into the arena, rmt:870-928) are announced with
 *                               pvae_params_changed.
 *   pvae_rollout_server_infer_rows  the same for 1-4 observations in one request.  A server starts as the single-row
 *                               instance of the kernel; the first request with more rows swaps in the multi-row instance
 *                               (once, a few hundred microseconds; it needs LDS for four input vectors -- -24 if that no
 *                               longer fits, the single-row instance then stays); it serves until pvae_rollout_server_stop.
 *                               A model with the motor decoder's helper
 *                               (pvae_config.mh_depth > 0) is served with the helper's layers behind the decoder's.
 *   pvae_rollout_server_stop    ends the kernel (also done by pvae_destroy).
 *   pvae_rollout_server_status  *lds_bytes < 0: dealt out over the whole chip (|value| bytes per workgroup).
 *                               *serving != 0 while the kernel is resident and answering: 2 when the request block lives in
 *                               DEVICE memory that the host writes through the BAR (hipDeviceAttributeIsLargeBar; the host
 *                               pushes the observation, the kernel polls local memory), 1 when it lives in pinned host
 *                               memory that the kernel pulls from (PVAE_SERVER_MAILBOX=host forces this form). */
int pvae_rollout_server_start(pvae_ctx* ctx, double idle_timeout_ms, double lifetime_s, int scope);
int pvae_rollout_server_infer(pvae_ctx* ctx, const float* obs, int noise, uint64_t rng_seed, uint64_t rng_offset, int reload,
                              float* a_hat, float* mu_logvar, float* z, double timeout_ms);
/* pvae_rollout_server_infer for 1 <= rows <= 4 observations in ONE request (rmt:742-771 serves any batch):
 * obs[rows][2*Db] -> a_hat[rows][Da] (+ mu_logvar[rows][2*Z], z[rows][Z]); row r draws Philox row r, as pvae_infer does --
 * bit-identical to pvae_infer on the same rows.  Every weight fragment read from LDS feeds all rows. */
int pvae_rollout_server_infer_rows(pvae_ctx* ctx, const float* obs, int32_t rows, int noise, uint64_t rng_seed,
                                   uint64_t rng_offset, int reload, float* a_hat, float* mu_logvar, float* z, double timeout_ms);
/* forward_decoder at B = 1 (rmt:822-837; the "pass_through" rollout of envs/rllib_env_imitation.py:233-258, where the caller draws
 * z itself): s1_z = [s1 (Db) | z (Z)] (host) -> a_hat[Da] (host).  The encoder's layers are skipped.
 * Without a helper: the same bits as pvae_net_forward(PVAE_NET_MD) on that row.  With one (pvae_config.mh_depth > 0) the
 * reply is decoder + mh_range * helper (rmt:833-835), formed by ONE fma in the kernel (as the served full request does):
 * within an ulp of a host that adds mh_range * h to pvae_net_forward's row itself (tests/test_gpu_rollout_server.py). */
int pvae_rollout_server_decode(pvae_ctx* ctx, const float* s1_z, float* a_hat, double timeout_ms);
int pvae_rollout_server_stop(pvae_ctx* ctx);
/* The caller wrote the parameter arena itself (load_state_dict / load_weights*, rmt:870-928; a torch optimizer) with work
 * queued on `stream` (NULL: the default stream): whatever holds a copy of the parameters -- the rollout server's LDS -- refreshes it before its
 * next answer, after that stream has drained. */
int pvae_params_changed(pvae_ctx* ctx, void* stream);
/* Measurement: n requests back to back with one observation, us[i] = host observation -> host action of request i on the
 * host's steady clock, taken inside the call (a compiled host's view; tools/infer_latency.py reports it next to Python's). */
int pvae_rollout_server_selfbench(pvae_ctx* ctx, const float* obs, int noise, int32_t n, double* us);
/* Measurement: where the LAST request's time went on the device (wall-clock stamps of workgroup 0, microseconds after it saw
 * the request): us[1 + 2 l] = layer l's inputs in LDS, us[2 + 2 l] = layer l's outputs published, us[1 + 2 n_layers] =
 * completion word issued, then ONE more entry: the shader clock during the request in MHz (s_memtime ticks per microsecond
 * of the 100 MHz wall clock: a mostly-idle resident kernel lets the part clock down).  *n = entries written (at most max). */
int pvae_rollout_server_timeline(pvae_ctx* ctx, double* us, int32_t max, int32_t* n);
int pvae_rollout_server_status(pvae_ctx* ctx, int32_t* serving, uint32_t* served, int32_t* lds_bytes);

/* A stack of Linear layers on CALLER-owned dense row-major weights (W[i]: [n_out[i]][n_in[i]], row stride
 * ldw[i], no alignment needed; bias may be NULL), hidden activation PVAE_ACT_* (act_kind for every hidden
 * layer, or layer_acts[i] per hidden layer when not NULL), linear output layer -- or, with (1 + PVAE_ACT_*) << 8 added
 * to act_kind, that activation on the output layer (the motor decoder's helper ends in tanh, rmt:491-495, 672).
 * scratch: 2 * rows * (widest hidden layer) floats (device).  No context: this is the value branch of
 * the rollout model (rmt:846-853, value_fn_layers 2*Db -> 256 -> 256 -> 1), whose parameters stay plain
 * torch tensors because the supervised loss never touches them; likewise the motor decoder's helper (rmt:670-680,
 * 833-835), a residual policy for RL fine-tuning that train_physics_vae.py never builds. */
int pvae_mlp_forward(const float* x, int32_t rows, int32_t ldx, int32_t n_layers, const float* const* W,
                     const float* const* bias, const int32_t* n_in, const int32_t* n_out,
                     const int32_t* ldw, int32_t act_kind, const int32_t* layer_acts, float* scratch, float* out,
                     int32_t ld_out, void* stream);

/* One stack on its own: in[rows][n_in] (dense) -> out[rows][n_out] (dense).  The building
 * block behind forward_encoder / forward_decoder / forward_world (rmt:773-844) when a caller
 * drives the stages separately (e.g. EnvRunner pass_through: z ~ N(0,I) straight into the
 * motor decoder, envs/rllib_env_imitation.py:234-266). */
int pvae_net_forward(pvae_ctx* ctx, int net, const float* in, int32_t rows, float* out, void* stream);
/* Sampler on its own (rmt:734-740): mu_logvar[rows][2Z] -> z[rows][Z];
 * eps NULL -> Philox; noise = 0 -> z = mu. */
int pvae_reparam(pvae_ctx* ctx, const float* mu_logvar, int32_t rows, const float* eps, int noise,
                 uint64_t rng_seed, uint64_t rng_offset, float* z_out, void* stream);

/* ---- imagined rollouts: H closed-loop steps of the policy and the world model in ONE call ------------------------------
 * Replaces the Python loop a user of the reference writes to unroll a trained model without the simulator: per step
 * forward_encoder + reparameterize + forward_decoder (+ the helper, rmt:833-835) + forward_world (rmt:773-844, 734-740;
 * the "pass_through" rollout of envs/rllib_env_imitation.py:234-258 when the code comes from the prior), with the world
 * model's prediction fed back as the next body state (what tpv:417-421 does inside the lookahead loss) -- torch.cat,
 * three or four module calls and their pad / copy launches per step.  The rule is stated in torch in
 * physicsvae_amd/imagine.py (imagine_torch), which is the specification.
 *
 * Step t = 0 .. horizon - 1 on `rows` start states s_0:
 *   PVAE_IMAGINE_REPLAY   a_t = actions(t);                                   s_{t+1} = WM([s_t | a_t])
 *   PVAE_IMAGINE_TRACK    h = TE([s_t | goals(t)]); z_t = sampler(h) as pvae_infer forms it (eps(t) supplied, or Philox at
 *                         (rng_seed, rng_offset + t), row r drawing row r; noise 0: z = mu); a_t = MD([s_t | z_t])
 *                         (+ mh_range * helper);                               s_{t+1} = WM([s_t | a_t])
 *   PVAE_IMAGINE_PRIOR    z_t = z(t) when supplied; else PVAE_PRIOR_ZERO_MEAN: z_t = n_t, PVAE_PRIOR_STATE_MEAN: z_t =
 *                         prior(s_t) + n_t (one float add), n_t = the draw the sampler would use as eps at (rng_seed,
 *                         rng_offset + t); the other prior kinds need z.  Then the decoder, the helper and the world model.
 * Input subsets hold (a stack that does not read the body columns never sees s_t); the actions are the decoder's means; the
 * value branch does not run.
 *
 * A source (s0, goals, actions, z, targets) is a descriptor: element (t, r, c) = base[idx(r) * ld + t * step + c], idx(r) =
 * row_index ? row_index[r] : r.  Dense [H][rows][D]: {p, D, rows * D, NULL}.  The demonstration set in place, window starts
 * in a device index array: {states + Db, Db, Db, window_row}.  s0 is read at t = 0.  Rows need 4-byte alignment only; the
 * index array's contents are the caller's contract (as seg_start is).  base NULL: absent.
 * Results (each may be NULL), dense: states_out [H][rows][Db] = s_1 .. s_H, actions_out [H][rows][Da], z_out [H][rows][Z]
 * (not written in replay mode), err [H]: with targets, err[t] = float(sum_{r,c} double(d) * double(d) / (rows * Db)), d =
 * s_{t+1} - targets(t) in float; partial sums in double in `scratch` (pvae_imagine_scratch_bytes), one per workgroup, folded
 * in a fixed order -- no atomics, the same bits on every call.
 *
 * Launches per step: the forward launches of the stacks the mode runs (as pvae_infer's staged path issues them), the
 * sampler, the helper's layers and its add, and ONE hand-over launch, which writes s_{t+1} to states_out and into the body
 * columns of the next step's input panels, copies a_t out, fetches the next step's goal / action / z columns and adds the
 * step's squared-error partials.  Per call: one launch that stages step 0 (pad rows and columns zeroed) and, with err, one
 * that folds the partials.  No per-step stage, pad or copy launch, no host synchronisation, no allocation.
 * pvae_imagine_launches states the counts of a call with err (per_call = 2) and, in prior mode under
 * PVAE_PRIOR_STATE_MEAN, with z drawn (the prior stack's layers + the launch that adds n_t; a call with z supplied issues
 * neither).  pvae_imagine returns the number of launches it enqueued.
 * The workspace is row block 0 of the context's panels: horizon is free of pvae_config.lookahead.  Like pvae_net_forward the
 * call overwrites the staging panels (the trainer gathers again).
 * Refused with -1 and a message, nothing launched: null args / s0, rows outside [1, max_batch], horizon < 1, a mode's drive
 * missing (replay: actions; track: goals; prior without z under PVAE_PRIOR_HYPERSPHERE / PVAE_PRIOR_NONE), err without
 * targets or without scratch of pvae_imagine_scratch_bytes(ctx, horizon) bytes.
 *   pvae_imagine_sizeof          sizeof(pvae_imagine_args) / sizeof(pvae_imagine_src): which = 0 / 1
 *   pvae_imagine_scratch_bytes   a multiple of 16; 0 on error */
#define PVAE_IMAGINE_REPLAY 0
#define PVAE_IMAGINE_TRACK 1
#define PVAE_IMAGINE_PRIOR 2
typedef struct pvae_imagine_src {      /* element (t, r, c) = base[idx(r) * ld + t * step + c] */
    const float* base;                 /* idx(r) = row_index ? row_index[r] : r */
    int64_t ld;
    int64_t step;
    const int32_t* row_index;
} pvae_imagine_src;
typedef struct pvae_imagine_args {
    int32_t mode;                      /* PVAE_IMAGINE_* */
    int32_t rows;                      /* 1 .. max_batch */
    int32_t horizon;                   /* >= 1 */
    int32_t noise;                     /* track: 0 -> z = mu */
    pvae_imagine_src s0;               /* [rows][Db] */
    pvae_imagine_src goals;            /* track: (t, r, 0 .. Db) */
    pvae_imagine_src actions;          /* replay: (t, r, 0 .. Da) */
    pvae_imagine_src z;                /* prior: (t, r, 0 .. Z), or absent: drawn */
    pvae_imagine_src targets;          /* (t, r, 0 .. Db) = what s_{t+1} is compared with, or absent */
    const float* eps;                  /* track: dense [H][rows][Z] draws, or NULL: Philox */
    uint64_t rng_seed, rng_offset;
    float* states_out;
    float* actions_out;
    float* z_out;
    float* err;
    void* scratch;
    size_t scratch_bytes;
} pvae_imagine_args;
int pvae_imagine(pvae_ctx* ctx, const pvae_imagine_args* args, void* stream);
int pvae_imagine_sizeof(int which);
size_t pvae_imagine_scratch_bytes(const pvae_ctx* ctx, int32_t horizon);
int pvae_imagine_launches(const pvae_ctx* ctx, int mode, int32_t* per_step, int32_t* per_call);

/* ---- planning in the latent space: sampled candidates over imagined rollouts ------------------------------------------
 * Random shooting / MPPI over the decoder's codes, in one call: `candidates` (K) code sequences per environment, each
 * unrolled `horizon` steps through the decoder (+ helper) and the world model, scored against a target sequence, and the
 * nominal moved to the best (lam == 0) or to the cost-weighted mean (lam > 0); `iters` times.  The rule is this
 * project's own (the reference has no planner) and is stated in torch in physicsvae_amd/plan.py (plan_torch), which is the
 * specification.
 *
 * rows = envs * candidates, row r = e * K + k.  s0 (e, 0 .. Db) and targets (t, e, 0 .. Db) are pvae_imagine_src
 * descriptors OVER ENVIRONMENTS (row r reads environment r / K), so the demonstration set can be read in place.  Iteration
 * i = 0 .. iters - 1, nominal u [H][E][Z] (NULL: zeros):
 *   candidates  v(t, r) = u(t, e) + sigma * n_i(t, r); candidate k = 0 is the nominal itself (noise 0, not drawn).  n from
 *               `noise` [iters][H][rows][Z], or Philox at (rng_seed, rng_offset + i * H + t), Philox row row0 + r, the
 *               sampler's groups below Z / 4.  z = v; under PVAE_PRIOR_HYPERSPHERE z = v / max(|v|, 1e-12).  The learned
 *               prior's mean does not enter: candidates are centred on the nominal.
 *   unroll      pvae_imagine's prior mode with z supplied on `rows` rows: the same launches.
 *   cost        J(r) = sum_t sw[t] * sum_c cw[c] * double(d)^2 / Db, d = s_{t+1}(r, c) - targets(t, e, c) in float, squares
 *               and sums in double in a fixed order, added by the hand-over launches (no atomics); rounded once to float.
 *   selection   best(e) = argmin_k cost(e, k), ties to the lowest k.  lam == 0: u'(t, e) = z(t, e * K + best).  lam > 0:
 *               w_k = exp(-(cost_k - cost_best) / lam) in double, u' = float(sum_k w_k z_k / sum_k w_k), k ascending, and
 *               projected onto the sphere again under PVAE_PRIOR_HYPERSPHERE.  iter_cost[i][e] = cost(e, best).
 * After the last iteration the plan's first step runs once more on `envs` rows with z = u(0) -- pvae_imagine, prior mode,
 * horizon 1 -- for a0 [E][Da] (the decoder's mean, + the helper) and s1 [E][Db].
 * Results (each may be NULL), dense: plan_z [H][E][Z], best [E], cost [E][K], iter_cost [iters][E], a0, s1 and, of the last
 * iteration, z_cand / noise_out [H][rows][Z] and states [H][rows][Db].
 *
 * Launches: iters * (horizon * per_step + per_iter) + closing, as pvae_plan_launches states them (per_step: the unroll's;
 * per_iter = 3: candidates, stage, selection; closing: the one-step pass).  pvae_plan returns the number it enqueued.  No host
 * synchronisation, no allocation; `scratch` (pvae_plan_scratch_bytes(ctx, horizon, rows), 16-byte aligned) is the
 * caller's: the rows' costs in double, the candidate codes, the nominal between iterations.
 * Selection keeps the K costs and weights of an environment in LDS: candidates above PVAE_PLAN_MAX_CANDIDATES are REFUSED
 * (not tiled).  Refused with -1 and a message, nothing launched: null args / s0 / targets, envs < 1, candidates outside
 * [1, PVAE_PLAN_MAX_CANDIDATES], rows outside [1, max_batch], horizon < 1, iters < 1, sigma or lam negative or not finite,
 * scratch missing, short or misaligned.
 *   pvae_plan_sizeof          sizeof(pvae_plan_args): which = 0
 *   pvae_plan_scratch_bytes   a multiple of 16; 0 on error */
#define PVAE_PLAN_MAX_CANDIDATES 4096
typedef struct pvae_plan_args {
    int32_t envs;                      /* E >= 1 */
    int32_t candidates;                /* K >= 1; envs * candidates <= max_batch */
    int32_t horizon;                   /* >= 1 */
    int32_t iters;                     /* >= 1 */
    float sigma;                       /* >= 0 */
    float lam;                         /* 0: take the best; > 0: MPPI temperature */
    pvae_imagine_src s0;               /* (e, 0 .. Db) */
    pvae_imagine_src targets;          /* (t, e, 0 .. Db) */
    const float* nominal;              /* [H][E][Z], or NULL: zeros */
    const float* noise;                /* [iters][H][rows][Z], or NULL: Philox */
    const float* col_weight;           /* cw [Db] >= 0, or NULL: ones */
    const float* step_weight;          /* sw [H] >= 0, or NULL: ones */
    uint64_t rng_seed, rng_offset;
    int64_t row0;                      /* Philox row of row 0 (chunked callers number their rows globally) */
    float* plan_z;
    int32_t* best;
    float* cost;
    float* iter_cost;
    float* a0;
    float* s1;
    float* z_cand;
    float* noise_out;
    float* states;
    void* scratch;
    size_t scratch_bytes;
} pvae_plan_args;
int pvae_plan(pvae_ctx* ctx, const pvae_plan_args* args, void* stream);
int pvae_plan_sizeof(int which);
size_t pvae_plan_scratch_bytes(const pvae_ctx* ctx, int32_t horizon, int32_t rows);
int pvae_plan_launches(const pvae_ctx* ctx, int32_t* per_step, int32_t* per_iter, int32_t* closing);

/* ---- backpropagation through imagined rollouts; gradient-refined latent plans -----------------------------------------
 * The rule is this project's own and is stated in torch in physicsvae_amd/refine.py (rollout_grad_torch, refine_torch),
 * which is the specification.  Every stack is frozen: parameters, the gradient arena and the Adam state are not touched.
 *
 * pvae_imagine_grad: the planner's unroll (pvae_imagine's prior mode with z supplied: the same launches) on rows = envs *
 * group rows, row r = e * G + g; s0 (e, 0 .. Db) and targets (t, e, 0 .. Db) are descriptors OVER ENVIRONMENTS, z is dense
 * [H][rows][Z], the code as the decoder reads it.  cost [rows] is pvae_plan's J(r), bit for bit (the same per-row
 * arithmetic, by the hand-over launches); dz [H][rows][Z] = dJ(r) / dz_t(r) and ds [H][rows][Db] = dJ(r) / ds_t(r)
 * (ds[0]: at the start state) by backpropagation through time through the decoder, the helper and the world model:
 *   cot_{t+1} = coef(t, c) * d + ds_{t+1},  coef = float(2 * sw[t] * cw[c] / Db) formed in double, d = s_{t+1} - target in
 *   float, a product and then a sum, ds_H = 0; ds_t = the world model's body columns + (where the decoder reads the body)
 *   the decoder's + the helper's, in this order; dz_t = +0.0 where the decoder does not read the code.
 * The workspace holds one step's activations: the states are kept on a tape in `scratch`, and for t < H - 1 the step's
 * forward launches run again before its backward launches.  Launches: per_call + horizon * fwd_per_step and, when dz or ds
 * is asked for, + horizon * bwd_per_step + (horizon - 1) * (fwd_per_step - 1), as pvae_imagine_grad_launches states them
 * (bwd_per_step = the layers of the world model, the decoder and the helper + 2: the action seed and the backward
 * hand-over).  No atomics, a fixed summation order: the same bits on every call.  Results (each may be NULL and is then not
 * written): cost, dz, ds, states_out [H][rows][Db] = s_1 .. s_H.  With neither dz nor ds the call is forward only.
 * Refused with -1 and a message, nothing launched: null args / s0 / targets / z, envs < 1, group < 1, rows above
 * max_batch, horizon < 1, scratch (pvae_imagine_grad_scratch_bytes(ctx, horizon, rows), 16-byte aligned) missing, short or
 * misaligned.
 *
 * pvae_plan_refine: `steps` Adam steps on the codes of `envs` environments (group 1) from `nominal` [H][E][Z] (NULL: zeros),
 * entirely on the stream.  The iterate is v; the code fed to the unroll is z = v, under PVAE_PRIOR_HYPERSPHERE z = v /
 * max(|v|, 1e-12).  Iteration i = 0 .. steps - 1: forward and backward at z_i (iter_cost[i][e] = float(J)), then ONE update
 * launch, a workgroup per environment: keep z_i if its stored float cost is smaller than the best so far (ties: the lowest
 * i), pull dz back through the projection under the sphere, Adam on v (beta 0.9 / 0.999, eps 1e-8, bias-corrected, zero
 * moments at the start of every call, float, every operation rounded on its own, the order of refine.py), project the new
 * iterate.  Then one forward-only unroll for iter_cost[steps], the last keep, and the closing pass: pvae_imagine, prior mode,
 * horizon 1, on z = plan_z[0] for a0 [E][Da] and s1 [E][Db].  Results (each may be NULL and is then not written): plan_z
 * [H][E][Z] = z_{best_iter(e)}, cost [E] = iter_cost[best_iter], best_iter [E], iter_cost [steps + 1][E], a0, s1, z_iters
 * [steps + 1][H][E][Z], grad [H][E][Z] = dJ / dv of the last backward (zeros with steps == 0).
 * Launches: steps * (G(horizon) + per_iter) + F(horizon) + per_call, G / F = pvae_imagine_grad's count with / without the
 * backward, as pvae_plan_refine_launches states per_iter (1) and per_call (init, the last keep, the closing pass).
 * Refused with -1: null args / s0 / targets, envs < 1, rows (= envs) above max_batch, horizon < 1, steps < 0, lr not finite
 * or <= 0, scratch (pvae_plan_refine_scratch_bytes(ctx, horizon, envs), 16-byte aligned) missing, short or misaligned.
 *   pvae_*_sizeof          sizeof the args struct: which = 0
 *   pvae_*_scratch_bytes   a multiple of 16; 0 on error */
typedef struct pvae_imagine_grad_args {
    int32_t envs;                      /* E >= 1 */
    int32_t group;                     /* G >= 1; envs * group <= max_batch */
    int32_t horizon;                   /* >= 1 */
    int32_t reserved;
    pvae_imagine_src s0;               /* (e, 0 .. Db) */
    pvae_imagine_src targets;          /* (t, e, 0 .. Db) */
    const float* z;                    /* [H][rows][Z] */
    const float* col_weight;           /* cw [Db] >= 0, or NULL: ones */
    const float* step_weight;          /* sw [H] >= 0, or NULL: ones */
    float* cost;
    float* dz;
    float* ds;
    float* states_out;
    void* scratch;
    size_t scratch_bytes;
} pvae_imagine_grad_args;
int pvae_imagine_grad(pvae_ctx* ctx, const pvae_imagine_grad_args* args, void* stream);
int pvae_imagine_grad_sizeof(int which);
size_t pvae_imagine_grad_scratch_bytes(const pvae_ctx* ctx, int32_t horizon, int32_t rows);
int pvae_imagine_grad_launches(const pvae_ctx* ctx, int32_t* fwd_per_step, int32_t* bwd_per_step, int32_t* per_call);
typedef struct pvae_plan_refine_args {
    int32_t envs;                      /* E >= 1, <= max_batch */
    int32_t horizon;                   /* >= 1 */
    int32_t steps;                     /* >= 0 */
    float lr;                          /* > 0 */
    pvae_imagine_src s0;               /* (e, 0 .. Db) */
    pvae_imagine_src targets;          /* (t, e, 0 .. Db) */
    const float* nominal;              /* [H][E][Z], or NULL: zeros */
    const float* col_weight;           /* cw [Db] >= 0, or NULL: ones */
    const float* step_weight;          /* sw [H] >= 0, or NULL: ones */
    float* plan_z;
    float* cost;
    int32_t* best_iter;
    float* iter_cost;
    float* a0;
    float* s1;
    float* z_iters;
    float* grad;
    void* scratch;
    size_t scratch_bytes;
} pvae_plan_refine_args;
int pvae_plan_refine(pvae_ctx* ctx, const pvae_plan_refine_args* args, void* stream);
int pvae_plan_refine_sizeof(int which);
size_t pvae_plan_refine_scratch_bytes(const pvae_ctx* ctx, int32_t horizon, int32_t envs);
int pvae_plan_refine_launches(const pvae_ctx* ctx, int32_t* per_iter, int32_t* per_call);

/* ---- backward of the stand-alone stages (torch autograd through the module: physicsvae_amd/autograd.py) ---------
 * What PPO's loss.backward() does to PhysicsVAE.forward / forward_encoder / forward_decoder / forward_world
 * (rmt:743-771 -> rmt:773-853) when the stacks are learnable (rmt:473, 488), on the tile kernels of the trainer.
 *
 * Backward of one arena stack from a caller-supplied output gradient (autograd of rmt:773-853).
 * in[rows][n_in] dense (the same input pvae_net_forward takes), dy[rows][n_out] dense = dL/d(output AFTER the
 * output activation: the helper's tanh).  dx[rows][n_in] (NULL: not wanted).  grad: pvae_net_segment(net)
 * `count` floats, element 0 = arena offset `offset`, same layout as the arena (NULL: no parameter gradient,
 * input-gradient launches only).  accumulate: 0 store, 1 add into grad.  1 <= rows <= max_batch.
 * Recompute, not saved activations: `in` is padded into the stack's panels and the forward runs again (the launches of
 * pvae_net_forward: the same bits), then the trainer's per-layer backward plan runs with a gradient store (or a
 * read-add-write, EpiGradAccum: each output tile summed by one workgroup in a fixed order, so equal operands give equal
 * bits) and no Adam.  The extra forward is about one third of forward + backward: the price of a forward under
 * autograd that costs nothing extra when no backward follows.  The pad rows of the panels are zeroed or kept out of
 * every contraction, so what earlier calls left there never reaches a gradient.  Like pvae_net_forward it overwrites
 * the staging panels (the HIP trainer gathers again).  Weight-gradient launches count in pvae_profile_read
 * categories 1-3. */
int pvae_net_backward(pvae_ctx* ctx, int net, const float* in, int32_t rows, const float* dy, float* dx,
                      float* grad, int32_t accumulate, void* stream);
/* Backward of pvae_reparam (rmt:734-740, 795-816 per prior kind): d_mu_logvar from dz, the draws the forward used
 * (eps_used, as the forward left them) and the forward's mu_logvar; noise = 0: z = mu.  No KL term (the caller's loss
 * owns it).  mu_logvar / d_mu_logvar are [rows][2 Z] ([rows][Z] for PVAE_PRIOR_HYPERSPHERE / PVAE_PRIOR_NONE, where
 * eps_used is not read), eps_used / dz [rows][Z], all dense. */
int pvae_reparam_backward(pvae_ctx* ctx, const float* mu_logvar, const float* eps_used, const float* dz,
                          int32_t rows, int noise, float* d_mu_logvar, void* stream);

/* ---- stack set: S fully connected stacks on ONE shared input (FullyConnectedPolicy "fcnn", rmt:323-457) -------------
 * The reference's other custom model: `_policy_fn`, `_value_fn` and, with log_std_type "state_dependent", `_log_std_fn`
 * (rmt:386-427) are independent FC stacks (rmt:234-283) that all read the same observation (rmt:430-441).  At their sizes
 * (256x2 / 64x2) a step is bound by launch boundaries, so the stacks run TOGETHER: one launch per layer depth for all of
 * them, instead of one per layer per stack.
 *
 * pvae_fc_config: stack s has depth[s] hidden layers of width[s][i] with activation act[s][i] (PVAE_ACT_*), then a linear
 * output layer of n_out[s] values.  1 <= n_stacks <= PVAE_FC_MAX_STACKS, depth in [0, PVAE_MAX_HIDDEN].  depth 0 -- the
 * stack is its linear output layer alone, a column block of the shared first-layer GEMM -- is supported and tested
 * (tests/test_gpu_fc_shapes.py, forward and backward against float64, both schedules), though the Python `Stack` refuses it.
 *
 * Arena (one flat fp32 buffer, the padding rules of the five-net arena: W[n_out_pad][ld] row-major with ld = n_in rounded
 * up to 64 and n_out_pad = n_out rounded up to 64, then bias[n_out_pad]; pads are zero and stay zero):
 *   [ W_0 of stack 0 | W_0 of stack 1 | ... | bias_0 of stack 0 | bias_0 of stack 1 | ... | per stack: W_1 b_1 W_2 b_2 ... ]
 * The first layers share their input and therefore their row stride: back to back they are one weight block, so the
 * first layer of all stacks is ONE GEMM over the concatenated output features, and the gradient with respect to the
 * input is one GEMM whose contraction over those features is the sum over the stacks.  The checkpoint tensor
 * `_policy_fn._model.<i>._model.0.weight` [n_out, n_in] is the strided view W[:n_out, :n_in] of its block; nothing is
 * packed or copied per call.  A gradient arena has the same layout.
 *
 *   pvae_fc_num_layers / pvae_fc_layer   enumerate the Linear layers stack by stack, first layer first (pvae_layer_info:
 *                       net = stack, col0 = 0); offsets follow the arena order above, not the enumeration order
 *   pvae_fc_arena_floats / pvae_fc_workspace_bytes   sizes of the parameter (gradient) arena and of the workspace
 *   pvae_fc_create / pvae_fc_destroy / pvae_fc_bind   the opaque context (layout tables + the two bound device buffers)
 *   pvae_fc_forward     x[rows][n_in] dense -> out[s][rows][n_out[s]] dense per stack (out[s] NULL: not wanted -- the stack
 *                       still runs unless no later stack is wanted either), 1 <= rows <= max_batch.  Replaces
 *                       FullyConnectedPolicy.forward's three FC calls (rmt:434-438).  rows <= 4: the GEMV family (one
 *                       wave per output feature, rollout latency); above: tile kernels.  Launches: one copy of x into the
 *                       padded input panel, ONE for the first layer of all stacks, ONE per deeper layer depth in which
 *                       the workgroup index maps to (stack, tile) -- stacks that are shallower drop out, narrower ones
 *                       contribute fewer tiles.  The output layers write the dense results themselves.
 *   pvae_fc_backward    what loss.backward() does to those calls.  dy[s][rows][n_out[s]] dense per stack, NULL: that stack
 *                       gets no gradient and costs nothing (its layers run neither forward nor backward, except where
 *                       its first layer lies between two wanted ones in the shared block).  dx[rows][n_in] (NULL: not
 *                       wanted) = the input gradient SUMMED over the stacks with a dy.  grad (NULL: none): a gradient
 *                       arena; stack s writes its part only when bit s of grad_mask is set (a frozen stack passes the
 *                       input gradient and leaves its part of `grad` untouched); accumulate: 0 store, 1 read-add-write
 *                       (EpiGradAccum, as pvae_net_backward: every output tile summed by one workgroup in a fixed order).
 *                       Recompute, as pvae_net_backward: the forward launches run again on the panels, a seed launch
 *                       forms every output gradient, then ONE launch per layer depth, last to first, holding the input-
 *                       gradient and the weight-gradient tiles (and bias sums) of every participating stack at that depth
 *                       (the same-layer pairing of the trainer's backward plan, inside the group); the first-layer launch
 *                       holds the one input-gradient GEMM and the stacks' weight gradients.  Pad rows and pad columns of
 *                       every panel a contraction reads are written (zeros, or finite values that meet zeros) by this
 *                       call, so nothing an earlier call left in the workspace reaches a gradient.
 *   pvae_fc_launches    kernel launches of the last pvae_fc_forward / pvae_fc_backward call on this context.
 * pvae_set_option(NULL, "fc_per_stack", 1): the same tiles, one launch per stack where the default issues one per depth
 * (the A/B baseline of the grouping; the input-gradient GEMM of the first layers stays one launch -- split, it would need
 * a sum over the stacks in another order).  Tile geometry is a function of the problem alone, so both schedules give the
 * same bits. */
#define PVAE_FC_MAX_STACKS 4
typedef struct pvae_fc_config {
    int32_t n_in;       /* width of the shared input (the flattened observation, rmt:384) */
    int32_t n_stacks;
    int32_t max_batch;  /* largest number of rows of one call */
    int32_t depth[PVAE_FC_MAX_STACKS];      /* hidden layers per stack */
    int32_t n_out[PVAE_FC_MAX_STACKS];      /* width of the linear output layer */
    int32_t width[PVAE_FC_MAX_STACKS][16];  /* hidden widths */
    int32_t act[PVAE_FC_MAX_STACKS][16];    /* PVAE_ACT_* per hidden layer (0 = relu) */
} pvae_fc_config;
typedef struct pvae_fc pvae_fc;
int pvae_fc_num_layers(const pvae_fc_config* cfg);
int pvae_fc_layer(const pvae_fc_config* cfg, int i, pvae_layer_info* out);
int64_t pvae_fc_arena_floats(const pvae_fc_config* cfg);
size_t pvae_fc_workspace_bytes(const pvae_fc_config* cfg);
int pvae_fc_create(const pvae_fc_config* cfg, pvae_fc** out);
void pvae_fc_destroy(pvae_fc* fc);
int pvae_fc_bind(pvae_fc* fc, float* params, void* workspace, size_t workspace_bytes);
int pvae_fc_forward(pvae_fc* fc, const float* x, int32_t rows, float* const* out, void* stream);
int pvae_fc_backward(pvae_fc* fc, const float* x, int32_t rows, const float* const* dy, float* dx, float* grad,
                     int32_t grad_mask, int32_t accumulate, void* stream);
int pvae_fc_launches(pvae_fc* fc, int32_t* forward, int32_t* backward);

/* ---- PPO learner step on a stack set (the imitation stage: `run: DDPPO`, `custom_model: fcnn`) ----------------------
 * One minibatch update -- forward, clipped-surrogate loss, backward, Adam -- as ONE library call with no host
 * synchronisation: the stack set must be [policy (n_out = k), value (n_out = 1)] or, log_std_kind 2, [policy, value,
 * log-std (n_out = k)].  The loss, for B rows (c = 1 / B), mean / log_std [B][k], value [B] and the batch columns below:
 *   logp    = -0.5 sum_j ((a_j - mean_j) / exp(ls_j))^2 - sum_j ls_j - 0.5 k log(2 pi)
 *   ratio   = exp(logp - old_logp);  surr = min(adv ratio, adv clamp(ratio, 1 - clip_param, 1 + clip_param))
 *   kl      = sum_j [ ls_j - ls_old_j + (exp(2 ls_old_j) + (mean_old_j - mean_j)^2) / (2 exp(2 ls_j)) - 0.5 ]
 *   entropy = sum_j (ls_j + 0.5 log(2 pi e))
 *   vf      = max((value - value_targets)^2, (vf_preds + clamp(value - vf_preds, -vf_clip_param, vf_clip_param) - value_targets)^2)
 *   total   = mean_rows(-surr + kl_coeff kl + vf_loss_coeff vf - entropy_coeff entropy)
 *   stats   = [ total, mean(-surr), mean(vf), mean(kl), mean(entropy) ]
 * log_std by kind: 0 constant (a vector of k values, no gradient), 1 state_independent (a trained vector of k values,
 * gradient = column sum over the rows), 2 state_dependent (log_std_base + the third stack's output).
 *
 * Launches of one step: the stack set's forward (copy-in, which gathers obs[index[r]], + one per layer depth), ONE loss
 * head (reads the stacks' outputs in their panels and the batch columns through `index`; writes every stack's output
 * gradient over its whole padded panel -- zeros in pad rows and pad columns -- and per-wave partial sums of the stats and,
 * kind 1, of the log-std columns), one backward launch per layer depth (no recompute: the forward's panels are live;
 * gradients stored to the bound gradient arena), ONE Adam launch over the arena whose extra workgroup sums the partials in
 * a fixed order, writes stats_out[5] and, kind 1, finishes the log-std gradient and applies Adam to that vector.  At the
 * default sizes: 4 + 1 + 3 + 1 = 9 launches for two or three stacks alike (rows <= 4: one more, zeroing the pad rows the
 * GEMV forward leaves).  Every summation order is fixed: the same inputs give the same bits.
 *
 *   pvae_fc_ppo_workspace_bytes   size of the scratch buffer (partial sums), a multiple of 16
 *   pvae_fc_ppo_bind      grad / m / v: buffers with the arena's layout (m and v zero-initialised by the caller; pads stay
 *                         zero); scratch; log_std: kind 0 the constant vector (log_std_m / log_std_v NULL), kind 1 the trained
 *                         vector and its moments, kind 2 all three NULL.  pvae_fc_bind must have been called.
 *   pvae_ppo_loss         the head alone on dense tensors (no stack set): mean [rows][k], log_std rows log_std_row_stride
 *                         floats apart (0: one vector for all rows), value [rows]; row r reads the batch columns at
 *                         index[r] (index NULL: at r).  Writes d_mean / d_log_std [rows][k], d_value [rows] (the gradients of
 *                         `total`; d_log_std per row for every kind) and stats_out[5].  One launch + the finishing reduction.
 *                         params: the loss coefficients only; k = batch->k.  It has no context to keep its partial
 *                         sums in: the FIRST call on a (device, stream) pair allocates a 128 KB buffer (hipMalloc) that the
 *                         library keeps for the life of the process, so make that first call outside a stream capture,
 *                         and do not call it on an unbounded number of short-lived streams.
 *   pvae_fc_ppo_step      one minibatch: rows r = 0 .. rows-1 are batch rows index[first + r] (index NULL: first + r),
 *                         1 <= rows <= max_batch, first + rows <= n_rows.  adam_t >= 1 is this step's Adam time step.
 *                         train_mask: bit s = stack s is trained (0: all); a stack that is not trained runs forward only, and
 *                         neither its parameters nor its moments are touched.
 *   pvae_fc_ppo_sgd       the SGD loop: per pass p the minibatches [first, first + minibatch) of perm + p n_rows (device
 *                         int32 [num_sgd_iter][n_rows]; NULL: row order), the last one short; adam_t advances by one per step
 *                         from params->adam_t; stats_out[steps][5] with steps = num_sgd_iter * ceil(n_rows / minibatch).
 *                         Every launch is enqueued on `stream`; nothing synchronises.
 *   pvae_fc_ppo_launches  kernel launches of the last pvae_fc_ppo_step (the last step of a pvae_fc_ppo_sgd).
 * Index entries outside [0, n_rows) are clamped into it.  Bad arguments, an unbound buffer, or a stack set that is not
 * [policy, value(, log-std)] return a negative code and launch nothing. */
typedef struct pvae_fc_ppo_params {
    float clip_param, vf_clip_param, vf_loss_coeff, kl_coeff, entropy_coeff;
    float weight_decay;
    double lr, beta1, beta2, adam_eps;
    int32_t adam_t;
    int32_t log_std_kind;   /* 0 constant, 1 state_independent, 2 state_dependent */
    float log_std_base;     /* kind 2: log_std = log_std_base + third stack */
    int32_t train_mask;     /* bit s: stack s is trained; 0 = every stack */
} pvae_fc_ppo_params;
typedef struct pvae_fc_ppo_batch {
    const float* obs;             /* [n_rows][n_in]   (not read by pvae_ppo_loss) */
    const float* actions;         /* [n_rows][k] */
    const float* old_dist;        /* [n_rows][2k]: old [mean | log_std] */
    const float* old_logp;        /* [n_rows] */
    const float* advantages;      /* [n_rows] */
    const float* value_targets;   /* [n_rows] */
    const float* vf_preds;        /* [n_rows] */
    int64_t n_rows;
    int32_t k;                    /* actions per row */
    int32_t reserved;
} pvae_fc_ppo_batch;
size_t pvae_fc_ppo_workspace_bytes(const pvae_fc_config* cfg);
int pvae_fc_ppo_bind(pvae_fc* fc, float* grad, float* m, float* v, void* scratch, size_t scratch_bytes, float* log_std,
                     float* log_std_m, float* log_std_v);
int pvae_ppo_loss(const float* mean, const float* log_std, int64_t log_std_row_stride, const float* value,
                  const pvae_fc_ppo_batch* batch, const int32_t* index, int32_t rows, const pvae_fc_ppo_params* params,
                  float* d_mean, float* d_log_std, float* d_value, float* stats_out, void* stream);
int pvae_fc_ppo_step(pvae_fc* fc, const pvae_fc_ppo_batch* batch, const int32_t* index, int64_t first, int32_t rows,
                     const pvae_fc_ppo_params* params, float* stats_out, void* stream);
int pvae_fc_ppo_sgd(pvae_fc* fc, const pvae_fc_ppo_batch* batch, const int32_t* perm, int32_t minibatch,
                    int32_t num_sgd_iter, const pvae_fc_ppo_params* params, float* stats_out, void* stream);
int pvae_fc_ppo_launches(pvae_fc* fc, int32_t* per_step);
/* sizeof(pvae_fc_ppo_params) / sizeof(pvae_fc_ppo_batch) as the library was compiled (binding self-check): which = 0 / 1 */
int pvae_fc_ppo_sizeof(int which);

/* ---- Train-batch preparation for the PPO learner: evaluate, bootstrap, GAE, standardisation ---------------------------
 * What RLlib 1.11 does on the host between rollout and SGD (postprocessing.compute_advantages + standardized), on the
 * device, so that a learner needs only obs, actions, rewards and the fragment table there and hands the result straight
 * to pvae_fc_ppo_sgd.  A SEGMENT is a run of consecutive rows of one episode in time order (what RLlib postprocesses as one
 * trajectory): segment s = rows seg_start[s] .. seg_start[s + 1] - 1; last_value[s] = 0 if it ended its episode
 * (seg_done[s]), else the value function at the observation after its last row (boot_obs[s]).  Rows t of a segment, last
 * row first (adv past the end = 0, v_next of the last row = last_value[s]):
 *   delta[t] = rewards[t] + gamma v_next[t] - vf_preds[t];  adv[t] = delta[t] + gamma lambda adv[t + 1]
 *   value_targets[t] = adv[t] + vf_preds[t]
 * then, over all n_rows rows and only with `standardize` (population std):
 *   advantages = (adv - mean(adv)) / max(1e-4, std(adv))
 *
 * Launches.  Evaluate: per chunk of max_batch rows the stack set's forward (copy-in + one per layer depth) + ONE epilogue
 * that reads the stacks' outputs in their panels and writes vf_preds[r], old_dist[r] = [mean | log_std] and old_logp[r] of
 * actions[r] (the loss head's logp, term for term; log_std by kind as in the PPO step, the vector taken from
 * pvae_fc_ppo_bind).  Bootstrap: the same path with the value stack alone over boot_obs; the copy-in never reads the row of
 * a done segment and the epilogue writes last_value[s] = 0 for it.  GAE: ONE launch, a wavefront per segment walking it
 * from its end in 64-row pieces (a wave scan per piece, the carry passed on), any segment length >= 1; it leaves per-
 * workgroup sums of adv and adv^2, in double, in the scratch.  Standardise: ONE launch, every workgroup adds those partials
 * in the same order and rescales its slice in place; skipped when standardize == 0.  No atomics, no host synchronisation,
 * no allocation: the same inputs give the same bits.
 *
 * seg_start lives on the device, so the library cannot read it without a synchronisation: the caller passes the two ends
 * it wrote (seg_first = seg_start[0], seg_last = seg_start[n_segs]), which must be 0 and n_rows; that the table increases
 * in between is the caller's contract.  The kernels clamp every bound into [0, n_rows]: a table that breaks the contract
 * gives wrong numbers, never an access outside the columns.
 *
 *   pvae_fc_gae_workspace_bytes   size of the scratch (the partial sums) for n_segs segments, a multiple of 16; 0 on error
 *   pvae_gae               the dense form, no stack set: rewards / vf_preds [n_rows], last_values [n_segs] (read as 0 where
 *                          seg_done[s]; seg_done NULL: as given) -> advantages, value_targets [n_rows].  Returns the
 *                          number of launches it enqueued (2, or 1 without standardize).
 *   pvae_fc_ppo_evaluate   the evaluate pass alone: the rows (when out->vf_preds is given; then old_dist and old_logp too)
 *                          and / or the bootstrap values (when out->last_value is given).
 *   pvae_fc_ppo_prepare    all of it on one stream: evaluate -- or, when the rollout carries the sampler's own vf_preds,
 *                          old_dist and old_logp (all three or none), those as they are and no evaluate launch over the
 *                          rows --, bootstrap, GAE, standardise.
 *   pvae_fc_gae_launches   launches of the last pvae_fc_ppo_prepare / pvae_fc_ppo_evaluate on this context: the evaluate
 *                          pass over the rows, and the rest (bootstrap + GAE + standardise).  Both counters are zeroed on entry of
 *                          either call, so after a refused call they read 0, 0 (after one that a HIP error cut short: 0, 0 too).
 * Bad arguments (ends of seg_start that are not 0 and n_rows, n_segs < 1, a stack set that is not [policy, value(,
 * log-std)], an unbound buffer, a short scratch) return a negative code and launch nothing. */
typedef struct pvae_gae_params {
    float gamma, lambda;
    int32_t standardize;    /* 0: the raw advantages, no rescale launch */
    int32_t log_std_kind;   /* evaluate: 0 constant, 1 state_independent, 2 state_dependent (as pvae_fc_ppo_params) */
    float log_std_base;     /* kind 2: log_std = log_std_base + third stack */
    int32_t reserved;
} pvae_gae_params;
typedef struct pvae_fc_rollout {
    const float* obs;             /* [n_rows][n_in] */
    const float* actions;         /* [n_rows][k] */
    const float* rewards;         /* [n_rows] */
    const int32_t* seg_start;     /* [n_segs + 1], increasing from 0 to n_rows */
    const uint8_t* seg_done;      /* [n_segs]: the segment ended its episode */
    const float* boot_obs;        /* [n_segs][n_in]: the observation after each segment's last row (done: never read) */
    const float* vf_preds;        /* the sampler's own columns, all three or none (NULL): [n_rows] */
    const float* old_dist;        /* [n_rows][2k] */
    const float* old_logp;        /* [n_rows] */
    int64_t n_rows;
    int32_t n_segs;
    int32_t k;                    /* actions per row */
    int64_t seg_first, seg_last;  /* seg_start[0] and seg_start[n_segs] as the caller wrote them */
} pvae_fc_rollout;
typedef struct pvae_fc_prepared {
    float* vf_preds;              /* [n_rows]     written by evaluate (may be NULL when the sampler's are given) */
    float* old_dist;              /* [n_rows][2k] */
    float* old_logp;              /* [n_rows] */
    float* last_value;            /* [n_segs] */
    float* advantages;            /* [n_rows] */
    float* value_targets;         /* [n_rows] */
} pvae_fc_prepared;
size_t pvae_fc_gae_workspace_bytes(int32_t n_segs);
int pvae_gae(const float* rewards, const float* vf_preds, const float* last_values, const int32_t* seg_start,
             const uint8_t* seg_done, int64_t n_rows, int32_t n_segs, int64_t seg_first, int64_t seg_last,
             const pvae_gae_params* params, float* advantages, float* value_targets, void* scratch, size_t scratch_bytes,
             void* stream);
int pvae_fc_ppo_evaluate(pvae_fc* fc, const pvae_fc_rollout* rollout, const pvae_gae_params* params,
                         const pvae_fc_prepared* out, void* stream);
int pvae_fc_ppo_prepare(pvae_fc* fc, const pvae_fc_rollout* rollout, const pvae_gae_params* params,
                        const pvae_fc_prepared* out, void* scratch, size_t scratch_bytes, void* stream);
int pvae_fc_gae_launches(pvae_fc* fc, int32_t* evaluate, int32_t* rest);
/* sizeof(pvae_gae_params) / sizeof(pvae_fc_rollout) / sizeof(pvae_fc_prepared) as the library was compiled: which = 0 / 1 / 2 */
int pvae_gae_sizeof(int which);

/* ---- PPO learner step of PhysicsVAE (the second stage: `run: DDPPO`, `custom_model: physics_vae`) --------------------
 * One minibatch update of PhysicsVAE -- its forward without the world model (rmt:742-771), the loss above, backward, Adam --
 * as ONE library call with no host synchronisation.  The value branch (rmt:846-853) is a ONE-stack stack set [value] with
 * n_in = 2 Db, bound with pvae_fc_bind and pvae_fc_ppo_bind (its gradient arena and moments are the ones bound there).
 *
 * Launches of one step, in order:
 *   copy-in            obs[index[r]] = [s_body | s_task] into the encoder's input panel, the body columns of the decoder's and
 *                      the value stack's input panel (whole padded panels; an input subset's left-out block is zeros)
 *   [rows <= 4]        zero the pad rows of the layer-output panels the GEMV forward leaves unwritten
 *   TE layers          one per layer -> [mu | logvar]
 *   sampler            z = mu + eps exp(logvar / 2) into the decoder's input panel (noise = 0: z = mu; prior False: z = e)
 *   MD layers          one per layer -> a_hat
 *   value layers       the stack set's forward, one per layer
 *   loss head          reads a_hat, the log-std vector and the value in their panels and the batch columns through `index`;
 *                      writes d_mean and d_value over the padded gradient panels and the per-wave partials
 *   MD backward        one per layer, last to first (input gradient + weight gradient of a layer in one launch; weight
 *                      gradients only when MD is trained, the first layer's input gradient only when TE is trained);
 *                      skipped when neither TE nor MD is trained
 *   sampler backward   the z columns of the decoder's input gradient -> the encoder's output gradient (TE trained)
 *   TE backward        one per layer (TE trained)
 *   value backward     one per layer (value trained)
 *   Adam + stats       ONE launch over the trained segments (TE, MD: their segments of the arena; value: its own arena);
 *                      its extra workgroup finishes stats_out[5] and, log_std_kind 1, the log-std gradient and its update
 * No forward is recomputed: the three stacks share no panel, and every panel stays live until its backward has run.
 * Gradients go to `grad`, moments to `m` / `v` of pvae_ppo_bind: buffers of the parameter arena's layout that are NOT the
 * ones of pvae_bind_arenas (the supervised trainer's gradient arena and moments are never touched).
 *
 *   pvae_ppo_workspace_bytes  size of the scratch (the head's partial sums), a multiple of 16; 0 on error
 *   pvae_ppo_bind      grad / m / v (arena layout, m and v zero-initialised by the caller), scratch, log_std: the vector of
 *                      Da values, with its moments when it is trained (log_std_kind 1); value: the bound [value] stack set
 *   pvae_ppo_step      one minibatch, rows and index as pvae_fc_ppo_step.  params: pvae_fc_ppo_params with log_std_kind 0 / 1;
 *                      train_mask bits: 1 TE, 2 MD, 4 value (0: all three) -- a net that is not trained runs forward (and, the
 *                      decoder, passes the gradient on) and neither its parameters nor its moments are touched.
 *                      eps: device [rows][Z] draws, or NULL: Philox (rng_seed, rng_offset) as pvae_infer; noise = 0: z = mu.
 *                      The draws used are left in workspace panel 6.  batch->obs is [n_rows][2 Db], batch->k = Da.
 *   pvae_ppo_sgd       the SGD loop as pvae_fc_ppo_sgd; step i uses eps + i minibatch Z (dense per step: [steps][minibatch][Z],
 *                      not gathered through perm) or Philox offset rng_offset + i, and Adam time step adam_t + i.
 *   pvae_ppo_launches  kernel launches of the last step.
 *   pvae_ppo_sizeof    sizeof(pvae_fc_ppo_params) / sizeof(pvae_fc_ppo_batch) / sizeof(pvae_config): which = 0 / 1 / 2
 * The priors STATE_MEAN and HYPERSPHERE are OPT-IN: pvae_set_option(ctx, "ppo_priors", 1); a context that was not told answers
 * -1 for them ("the PPO step supports the priors normal_zero_mean_one_std and False ...").  With the option set:
 *   STATE_MEAN   the policy's output does not depend on the learned prior mean (rmt:801-809 only records it) and the PPO
 *                loss has no KL-to-prior term: every pass launches exactly what ZERO_MEAN launches, the sampler backward with
 *                its logvar half.  The prior stack (PVAE_NET_PR) is never launched and is in no Adam segment: its bits in the
 *                parameter arena and in grad / m / v are left alone, and it enters neither the clip norm nor grad_gnorm.
 *   HYPERSPHERE  the encoder's output is Z wide; sampler: z = e / max(|e|, 1e-12) (sphere_kernel).  NOTHING is drawn: the prior
 *                sample of rmt:810-814 reaches neither the action nor the loss, so the PPO passes run the sampler with noise
 *                off whatever the caller passed; eps / noise are accepted and not read, and the draws that come back
 *                (the panel of the draws used, pvae_ppo_draws.eps_out) are zeros, as under NONE.  Sampler backward: one wavefront per
 *                row, grid rows_pad / 4, with e the encoder's output row and g the z columns of the decoder's input gradient
 *                    ie = 1 / max(sqrt(sum e^2), 1e-12);   zg = (sum e g) ie;   de = (g - e ie zg) ie
 *                in the summation order of pvae_reparam_backward (one device function serves both), over the whole padded
 *                panel, no atomics, the same bits every run.  It takes the sampler-backward slot: the launch count is the
 *                one above.  Under md_inputs = BODY the encoder's gradient is exactly zero.  (Z = 1: z = sign(e), and the
 *                encoder's gradient is a rounding residue around an exact zero.)
 * The helper stack and lookahead > 1 remain refused with or without the option.
 * Needs lookahead 1, prior ZERO_MEAN or NONE (or the option above), no helper stack.  Bad arguments, an unbound buffer or rows > max_batch return a
 * negative code and launch nothing.  Within that, nothing else about the configuration is refused, and all of it is tested
 * against float64 (tests/test_gpu_ppo_vae_shapes.py, the evaluate pass below included): input subsets on either stack
 * (te_inputs / md_inputs; the columns outside a window stay exactly zero in parameters, gradients and both moments, and
 * under md_inputs = BODY the encoder's whole gradient is exactly zero), stacks given layer by layer (layer_width / layer_act:
 * a width and an activation per layer, depths that differ between encoder, decoder and value branch), both priors (NONE:
 * the encoder's output is Z wide), noise = 0 (the logvar half of the encoder's output layer then has gradient exactly zero),
 * every train_mask, 1 .. 4 rows, Z = 1 and Da = 1. */
size_t pvae_ppo_workspace_bytes(const pvae_config* cfg);
int pvae_ppo_bind(pvae_ctx* ctx, float* grad, float* m, float* v, void* scratch, size_t scratch_bytes, float* log_std,
                  float* log_std_m, float* log_std_v, pvae_fc* value);
int pvae_ppo_step(pvae_ctx* ctx, const pvae_fc_ppo_batch* batch, const int32_t* index, int64_t first, int32_t rows,
                  const pvae_fc_ppo_params* params, const float* eps, int noise, uint64_t rng_seed, uint64_t rng_offset,
                  float* stats_out, void* stream);
int pvae_ppo_sgd(pvae_ctx* ctx, const pvae_fc_ppo_batch* batch, const int32_t* perm, int32_t minibatch, int32_t num_sgd_iter,
                 const pvae_fc_ppo_params* params, const float* eps, int noise, uint64_t rng_seed, uint64_t rng_offset,
                 float* stats_out, void* stream);
int pvae_ppo_launches(pvae_ctx* ctx, int32_t* per_step);
int pvae_ppo_sizeof(int which);

/* ---- Gradient exchange between workers inside the PPO learners (`run: DDPPO`, `num_workers: 8`) ----------------------------
 * Both training specs that use these models are decentralised PPO with eight workers (data/spec/loco/loco_imitation.yaml:1,35;
 * data/spec/loco/loco_runtime_physics_vae.yaml:1,36): every worker runs the learner on its own train batch, and after every
 * minibatch's backward pass the workers average their gradients before each takes the -- then identical -- Adam step.  The
 * reference leaves that to RLlib; there is no reference counterpart of what follows.  The rule, with N workers and g_r the
 * gradient worker r's own minibatch gives (the mean over ITS rows, as the step computes it):
 *     g = (((g_0 + g_1) + g_2) + ... + g_{N-1}) * float32(1 / N)
 * in float32, in rank order, element by element over every trained segment and the state-independent log-std vector; N = 1
 * gives g_0 bit for bit.  Minibatches of different row counts give the mean of the workers' means (as DDP does), not the
 * row-weighted mean.  The stats stay each worker's own.  Every worker must issue the same number of steps.  The rank does
 * not enter the Philox stream: distinct draws per worker come from distinct seeds.
 *
 * The step in two halves, for a transport outside the library (torch.distributed: nccl between GPUs, gloo anywhere):
 *   pvae_fc_ppo_grad / pvae_ppo_grad     everything *_ppo_step does before its Adam launch, with the step's arguments: the
 *                         gradient lies in the bound gradient buffers; then the five stats are finished into stats_out and,
 *                         log_std_kind 1, the log-std vector's gradient is written to ls_grad[k] (device; may be NULL for the
 *                         other kinds) -- the value the Adam launch's last workgroup forms.  No parameter, no moment moves.
 *   pvae_fc_ppo_apply / pvae_ppo_apply   Adam over the trained segments (params->train_mask, adam_t, log_std_kind as the step's)
 *                         on grad_scale * gradient, the product formed in float32 element by element, and on the log-std
 *                         vector from grad_scale * ls_grad.  grad + apply(1.0) is the step, bit for bit.
 * Neither half ever exchanges.
 *
 * The exchange inside the library, peer-mapped (as pvae_p2p_*; no RCCL form): every worker maps its peers' gradient
 * buffers -- a stack set's gradient arena; PhysicsVAE's, the one of pvae_ppo_bind and the value stack set's -- and a flag
 * block whose tail holds the k floats of the log-std gradient.  Parameters and moments are not mapped: every rank reads
 * every rank's gradient ((N - 1) x the gradient bytes come in over the links per step) and updates its own replica whole,
 * so moments stay complete on every rank and nobody writes into a peer's parameters.  While an exchange is open,
 * *_ppo_step and *_ppo_sgd issue the exchanged form of their Adam launch -- ONE launch, the launch count unchanged: ready
 * flags, a bounded wait for the peers', the N gradients read with system-scope loads and summed in rank order, Adam on the
 * local parameters, the log-std vector from the N slots, a "done" hand-shake so that the next step's backward may overwrite
 * the buffers.  A wait that gives up ("p2p_timeout_ms"; for stack sets the process-wide option of that name) aborts this
 * rank's update -- nothing moves -- and is counted.  With world 1 the exchanged launch gives the plain step's bits.
 *   *_peer_export   writes this worker's blob (PVAE_P2P_BLOB_BYTES: IPC handles, offsets, sizes); zeroes the flag block.
 *                   *_ppo_bind must have been called, and the buffers must come from hipMalloc.
 *   *_peer_open     blobs: world x PVAE_P2P_BLOB_BYTES in rank order (an exchange of the blobs between the workers is the
 *                   barrier between export and open); world <= PVAE_P2P_MAX_RANKS, world 1 is legal.  Ends with an attach-time
 *                   check, collective and bounded (< 1 s per wait): flag delivery both ways, and a gradient line read
 *                   remotely, overwritten by its owner and read again must not be stale.  On failure nothing stays open.
 *   *_peer_close    unmaps the peers (after every worker's last step has completed); export + open again starts from clean flags.
 *   *_peer_status   rank and world (0, 0 when not open), and the waits that gave up so far (synchronises `stream`). */
int pvae_fc_ppo_grad(pvae_fc* fc, const pvae_fc_ppo_batch* batch, const int32_t* index, int64_t first, int32_t rows,
                     const pvae_fc_ppo_params* params, float* stats_out, float* ls_grad, void* stream);
int pvae_fc_ppo_apply(pvae_fc* fc, const pvae_fc_ppo_params* params, float grad_scale, const float* ls_grad, void* stream);
int pvae_ppo_grad(pvae_ctx* ctx, const pvae_fc_ppo_batch* batch, const int32_t* index, int64_t first, int32_t rows,
                  const pvae_fc_ppo_params* params, const float* eps, int noise, uint64_t rng_seed, uint64_t rng_offset,
                  float* stats_out, float* ls_grad, void* stream);
int pvae_ppo_apply(pvae_ctx* ctx, const pvae_fc_ppo_params* params, float grad_scale, const float* ls_grad, void* stream);
int pvae_fc_ppo_peer_export(pvae_fc* fc, void* blob);
int pvae_fc_ppo_peer_open(pvae_fc* fc, int rank, int world, const void* blobs);
int pvae_fc_ppo_peer_close(pvae_fc* fc);
int pvae_fc_ppo_peer_status(pvae_fc* fc, int* rank, int* world, uint32_t* timeouts, void* stream);
int pvae_ppo_peer_export(pvae_ctx* ctx, void* blob);
int pvae_ppo_peer_open(pvae_ctx* ctx, int rank, int world, const void* blobs);
int pvae_ppo_peer_close(pvae_ctx* ctx);
int pvae_ppo_peer_status(pvae_ctx* ctx, int* rank, int* world, uint32_t* timeouts, void* stream);

/* ---- Learner diagnostics from inside the fused PPO steps ----------------------------------------------------------------
 * Both specs train with `kl_coeff: 0.0` and `vf_clip_param: 1000` (data/spec/loco/loco_imitation.yaml:15-16;
 * data/spec/loco/loco_runtime_physics_vae.yaml:15-16): the kl stat and half of the vf stat say nothing in those runs, and
 * the value outputs, the ratios and the gradient live only inside the call.  The reference leaves its learner stats to
 * RLlib (vf_explained_var among them); there is no reference counterpart of what follows.  A diagnostics row is
 * PVAE_PPO_DIAG floats per step (the specification: physicsvae_amd/ppo.py `learner_diag_torch`, `grad_gnorm_torch`), with
 * y = value_targets, v = the step's value output and ratio as the loss forms it, over the minibatch's B rows:
 *   [0] vf_explained_var  max(-1, 1 - Var(y - v) / Var(y)); exactly -1 for B == 1 or Var(y) == 0.  The variances come from
 *                         float32 sums taken around the first row's y and y - v and are finished in double.
 *   [1] clip_frac         share of rows with ratio < 1 - clip_param or ratio > 1 + clip_param
 *   [2] vf_clip_frac      share of rows with |v - vf_preds| > vf_clip_param
 *   [3] ratio_max_dev     max over the rows of |ratio - 1|, this ratio re-formed from a log-density summed in double (the
 *                         loss's float32 logp, a sum of ~k terms, would show its ulp here at k >= 130)
 *   [4] grad_gnorm        sqrt(sum g^2) over every element the step's Adam consumes: all trained segments and a trained
 *                         log-std vector, after the workers' exchange and after grad_scale, before weight decay; frozen
 *                         stacks (train_mask) do not enter.  Squares and sums in double; every workgroup of the Adam launch
 *                         leaves ONE partial in a slot of its own (no atomics) and ONE SMALL LAUNCH PER STEP adds the slots in
 *                         slot order -- the same inputs and grid give the same bits.
 *   [5..7]                reserved, written as 0 (5 and 6 get a meaning while a clip is bound: "Gradient clipping inside the
 *                         PPO learners")
 *   *_diag_bytes    the scratch *_ppo_diag wants (gradient-norm slots + the loss head's diagnostics partial rows); `steps`
 *                   >= 1 is accepted for a later per-call finish and does not enter today.
 *   *_ppo_diag      binds `diag` (device, capacity_steps x PVAE_PPO_DIAG floats) and the scratch (device, 16-byte aligned);
 *                   diag == NULL unbinds.  While bound: *_ppo_step writes row 0; *_ppo_grad entries 0..3 (and the reserved
 *                   ones) of row 0; *_ppo_apply entry 4 of row 0; *_ppo_sgd rows 0 .. steps-1, and answers a negative code,
 *                   launching nothing, when steps > capacity_steps.  A step has one launch more (*_ppo_grad: none; *_ppo_apply:
 *                   one); every other output keeps its bits, nothing synchronises.  Not bound: every entry point is what
 *                   it was, bit for bit and launch for launch.
 *   pvae_ppo_loss_diag   pvae_ppo_loss with diag_out[PVAE_PPO_DIAG]: entries 0..3, and 0 in the rest. */
#define PVAE_PPO_DIAG 8
size_t pvae_fc_ppo_diag_bytes(const pvae_fc_config* cfg, int32_t steps);
int pvae_fc_ppo_diag(pvae_fc* fc, float* diag, int32_t capacity_steps, void* scratch, size_t scratch_bytes);
size_t pvae_ppo_diag_bytes(pvae_ctx* ctx, int32_t steps);
int pvae_ppo_diag(pvae_ctx* ctx, float* diag, int32_t capacity_steps, void* scratch, size_t scratch_bytes);
int pvae_ppo_loss_diag(const float* mean, const float* log_std, int64_t log_std_row_stride, const float* value,
                       const pvae_fc_ppo_batch* batch, const int32_t* index, int32_t rows, const pvae_fc_ppo_params* params,
                       float* d_mean, float* d_log_std, float* d_value, float* stats_out, float* diag_out, void* stream);

/* ---- Gradient clipping inside the PPO learners ---------------------------------------------------------------------------
 * RLlib's `grad_clip` (global-norm clipping, torch.nn.utils.clip_grad_norm_; the usual setting for continuous control is
 * 40) inside the fused steps of both learners; there is no reference counterpart.  The rule (the specification:
 * physicsvae_amd/ppo.py `clip_coef_torch`, `dp_clip_mean_torch`), for one minibatch step of one worker with g this worker's
 * own gradient over everything its Adam launch would consume -- every trained segment and a trained state-independent
 * log-std vector; stacks frozen by train_mask do not enter; before weight decay:
 *     s    = sum g_i^2                                    squares and sums in double, fixed order, no atomics
 *     norm = float32(sqrt(s))
 *     coef = min(1.0f, max_norm / (norm + 1e-6f))         float32 throughout; a NaN quotient stays NaN (torch.clamp)
 *     g'_i = g_i * coef                                   one float32 multiply per element, also when coef == 1
 * and Adam consumes g'.  With coef == 1.0f the product is g bit for bit: a threshold that never bites gives the unclipped
 * step's parameters, moments and stats.  More than one worker: EVERY WORKER CLIPS ITS OWN GRADIENT FIRST, then the clipped
 * gradients are averaged by the rule of "Gradient exchange between workers":
 *     g = (((g'_0 + g'_1) + ...) + g'_{N-1}) * float32(1 / N)
 * (RLlib 1.11's order as recalled -- the clip runs after backward() and before the all-reduce --, not checked against a ray
 * installation).  Non-finite norms follow the float32 formula, whatever it gives.
 *   *_grad_clip_bytes   the scratch *_ppo_grad_clip wants (a multiple of 16): one double per workgroup of the sum-of-squares
 *                       launch, whose grid is bounded, so no size of the model enters.
 *   *_ppo_grad_clip     binds the threshold and the scratch (device, 16-byte aligned); max_norm == 0 with a NULL scratch
 *                       unbinds.  max_norm < 0 or non-finite, a null handle, a null or misaligned scratch and too few
 *                       bytes are answered with a negative code; nothing is ever launched.  pvae_fc_ppo_params keeps its
 *                       layout.  While bound:
 *       *_ppo_step, *_ppo_sgd   (plain and with a peer exchange open) clip as above: ONE launch more per step, the sum of
 *                       squares between the backward and the Adam launch; every workgroup of the Adam launch adds its slots in
 *                       slot order and forms coef.  Exchanged: the owner hands coef over in a word of its flag block with
 *                       the "ready" release, the readers scale peer q's gradient and log-std slot by coef_q; no new wait.
 *       *_ppo_grad      the gradient left in the bound buffers and ls_grad are the CLIPPED ones, scaled in place behind the
 *                       norm: the caller's all-reduce sums clipped gradients.  Two launches more.
 *       *_ppo_apply     ignores the binding (it must not clip a second time): grad + all-reduce + apply(1 / N) is the rule
 *                       above, grad + apply(1.0) the clipped step bit for bit; with NO clip bound, grad + apply(coef) is too.
 *       diagnostics     (both bound) entry 4 grad_gnorm keeps its meaning -- what Adam consumes, after clip and average;
 *                       [5] grad_gnorm_raw = this worker's own `norm` before the clip (what RLlib reports as grad_gnorm),
 *                       [6] grad_clip_coef = coef; *_ppo_grad writes 5 and 6, *_ppo_apply leaves them.  Without a clip
 *                       bound, entries 5..7 stay 0.
 *   Not bound: every entry point is what it was, bit for bit and launch for launch. */
size_t pvae_fc_ppo_grad_clip_bytes(const pvae_fc_config* cfg);
int pvae_fc_ppo_grad_clip(pvae_fc* fc, float max_norm, void* scratch, size_t scratch_bytes);
size_t pvae_ppo_grad_clip_bytes(pvae_ctx* ctx);
int pvae_ppo_grad_clip(pvae_ctx* ctx, float max_norm, void* scratch, size_t scratch_bytes);

/* ---- Train-batch preparation for PhysicsVAE: evaluate, bootstrap, GAE, standardisation -------------------------------
 * "Train-batch preparation for the PPO learner" above, with PhysicsVAE as the policy: from a device-resident rollout to the
 * seven columns pvae_ppo_sgd reads, on one stream.  The rollout, the parameters and the outputs are the structs of that
 * section: pvae_fc_rollout with obs [n_rows][2 Db], k = Da and boot_obs [n_segs][2 Db]; pvae_gae_params with log_std_kind
 * 0 or 1; pvae_fc_prepared.  The action distribution of a row depends on a latent draw, which pvae_ppo_draws names:
 *   eps        device [n_rows][Z] draws, row-aligned: the chunk that starts at row f reads eps + f Z, so the result does not
 *              depend on the chunking.  NULL: Philox (rng_seed, rng_offset + i) for chunk i, as step i of pvae_ppo_sgd
 *   eps_out    optional, device [n_rows][Z]: receives the draws actually used (workspace panel 6 of each chunk), so that a
 *              learner or a test can replay them; zeros with noise = 0 and with the prior False
 *   noise      0: z = mu
 *
 * Launches.  Evaluate, per chunk of at most max_batch rows, in order:
 *   copy-in            rows f .. f + rows - 1 of obs into the encoder's, the decoder's and the value stack's input panel
 *                      (whole padded panels; an input subset's left-out block is zeros)
 *   TE layers          one per layer -> [mu | logvar]
 *   sampler            z into the decoder's input panel, the draws used into workspace panel 6
 *   MD layers          one per layer -> a_hat
 *   value layers       the stack set's forward, one per layer
 *   epilogue           ONE launch: reads a_hat, the bound log-std vector and the value where they lie in their panels and
 *                      writes vf_preds[r], old_dist[r] = [a_hat | log_std] and old_logp[r] of actions[r] (the loss head's
 *                      logp, term for term: the learner's first step sees a ratio of exactly 1 under the same draws) and,
 *                      eps_out given, the chunk's draws
 * No backward follows, so a chunk of <= 4 rows (the GEMV forward, which writes the live rows only) needs no launch that
 * zeroes pad rows: nothing reads them.  Bootstrap, per chunk of at most max_batch segments: the boot copy-in (never reads
 * the row of a done segment), the value layers alone, the epilogue in its bootstrap mode (last_value[s] = 0 where
 * seg_done[s]).  GAE: ONE launch; standardise: ONE launch, skipped when standardize == 0 -- the launches of the section
 * above, with pvae_fc_gae_workspace_bytes(n_segs) for the scratch.  With T / M / V layers in the encoder, the decoder
 * and the value stack: evaluate = ceil(n_rows / max_batch) (T + M + V + 3), rest = ceil(n_segs / max_batch) (V + 2) + 1 +
 * standardize.  No atomics, no host synchronisation, no allocation, fixed summation order: the same inputs give the same
 * bits.  The parameters are not written (a running rollout server is not disturbed); the input and output panels of the
 * three stacks and workspace panel 6 are.
 *
 *   pvae_ppo_evaluate      the evaluate pass alone: the rows (when out->vf_preds is given; then old_dist and old_logp too,
 *                          and `draws`) and / or the bootstrap values (when out->last_value is given; `draws` may be NULL
 *                          when only they are asked for).
 *   pvae_ppo_prepare       all of it: evaluate -- or, when the rollout carries the sampler's own vf_preds, old_dist and
 *                          old_logp (all three or none), those as they are, no launch over the rows and `draws` not read
 *                          (may be NULL) --, bootstrap, GAE, standardise.
 *   pvae_ppo_gae_launches  launches of the last pvae_ppo_prepare / pvae_ppo_evaluate on this context: the evaluate pass over
 *                          the rows, and the rest (bootstrap + GAE + standardise).  Both counters are zeroed on entry of
 *                          either call, so after a refused call they read 0, 0 (after one that a HIP error cut short: 0, 0 too).
 * pvae_ppo_sizeof does not cover pvae_ppo_draws (which = 3 stays refused): a binding checks that struct against this header.
 * pvae_ppo_bind must have been called (the log-std vector and the [value] stack set are the ones bound there).  Needs
 * lookahead 1, prior ZERO_MEAN or NONE, no helper stack, log_std_kind 0 or 1.  Every kernel bound is clamped: a seg_start
 * that breaks its contract gives wrong numbers, never an access outside the columns.  Bad arguments, an unbound buffer, a
 * short scratch or ends of seg_start that are not 0 and n_rows return a negative code and launch nothing. */
typedef struct pvae_ppo_draws {
    const float* eps;             /* [n_rows][Z], or NULL: Philox */
    float* eps_out;               /* [n_rows][Z], or NULL: not wanted */
    int32_t noise;                /* 0: z = mu */
    int32_t reserved;
    uint64_t rng_seed, rng_offset;
} pvae_ppo_draws;
int pvae_ppo_evaluate(pvae_ctx* ctx, const pvae_fc_rollout* rollout, const pvae_gae_params* params,
                      const pvae_ppo_draws* draws, const pvae_fc_prepared* out, void* stream);
int pvae_ppo_prepare(pvae_ctx* ctx, const pvae_fc_rollout* rollout, const pvae_gae_params* params,
                     const pvae_ppo_draws* draws, const pvae_fc_prepared* out, void* scratch, size_t scratch_bytes,
                     void* stream);
int pvae_ppo_gae_launches(pvae_ctx* ctx, int32_t* evaluate, int32_t* rest);

/* ---- Action sampling: the rollout worker's policy step (RLlib's compute_actions) for both PPO policies -----------------
 * The producer of the sampler's own columns that both *_ppo_prepare calls take as given: from the observations of the
 * n_rows vectorised environments of one step to the sampled actions, action_dist_inputs = [mean | log_std], action_logp and
 * vf_preds, in ONE library call with no host synchronisation.  Both specs sample a diagonal Gaussian (loco_imitation.yaml:1,35
 * and loco_runtime_physics_vae.yaml:1,36: `run: DDPPO`, `clip_actions: true`); the reference leaves this to RLlib's
 * TorchDiagGaussian + StochasticSampling, so there is no reference line to cite.
 *
 * The rule, for row r with the policy's mean[r], l[r] = log_std (by kind, exactly as the evaluate epilogue forms it, ls_base +
 * included) and standard-normal noise n[r], all [k]:
 *   explore 1:  action[j] = fmaf(expf(l[j]), n[j], mean[j]);  action_logp = the log-density of the STORED float32 action by the
 *               evaluate epilogue's arithmetic, term for term and in its summation order -- never formed from n --, so that
 *               *_ppo_evaluate over the same observation and the returned action gives the same bits and the learner's
 *               first step sees a ratio of 1
 *   explore 0:  action = mean bit for bit, action_logp = 0, no noise drawn, read or written
 *   always:     old_dist = [mean | l] and vf_preds = value: the evaluate epilogue's bits
 * The stored actions are unclipped (what a sample batch holds); with clip = 1 a second output env_actions =
 * min(max(action, clip_low), clip_high) is what the environment takes.
 *
 * Noise: supplied ([n_rows][k]) or Philox4x32-10 at (rng_seed, rng_offset + chunk), counter row = the row within its chunk,
 * group = 0x80000000 + (j >> 2) for columns 4 (j >> 2) .. + 3: the high bit keeps the action noise apart from PhysicsVAE's
 * latent draws (groups < Z / 4) under one (seed, offset).  The noise used is written to noise_out, as the latent draws are:
 * Philox goes through hardware transcendentals and cannot be reproduced on the host.
 *
 * Destination rows.  Row r of the call is written to row dst = out_row ? out_row[r] : r of EVERY output column (out_row
 * clamped into [0, n_dst_rows): a bad table gives wrong numbers, never an access outside the columns); with obs_dst the
 * row's observation is copied to obs_dst[dst] as well, so that after T steps a train batch's columns are complete with no
 * copy.  Inputs (obs, noise, draws->eps) are read at r.
 *
 * Launches: exactly those of the evaluate pass over the same rows (per chunk of max_batch rows: copy-in, one per layer
 * depth -- for PhysicsVAE TE layers, sampler, MD layers, value layers --, ONE epilogue, the sampling one in place of the
 * evaluate one), reported by *_gae_launches under `evaluate` (rest = 0).  Plain stores, no atomics, no allocation: the
 * same inputs give the same bits.  The parameters are not written.
 *
 *   pvae_fc_ppo_act      a stack set [policy, value(, log-std)]; params->log_std_kind / log_std_base as for
 *                        pvae_fc_ppo_evaluate (gamma, lambda, standardize are not read); pvae_fc_ppo_bind must have been
 *                        called for kinds 0 and 1 (the log-std vector is the one bound there)
 *   pvae_ppo_act         PhysicsVAE; `draws`: the latent draws as for pvae_ppo_evaluate (eps read at r, eps_out written at
 *                        dst: [n_dst_rows][Z]); pvae_ppo_bind must have been called; needs what pvae_ppo_evaluate needs
 *   pvae_ppo_act_sizeof  sizeof(pvae_ppo_act_in) / sizeof(pvae_ppo_act_out) as the library was compiled: which = 0 / 1
 * Bad arguments (a null struct, k that is not the policy's width, a log_std_kind that does not fit the stacks, an unbound
 * buffer, explore or clip not 0 or 1, n_rows < 1, n_dst_rows < n_rows without out_row, clip_low > clip_high, clip without
 * env_actions or env_actions without clip, a null obs or a null required output) return a negative code and launch nothing. */
typedef struct pvae_ppo_act_in {
    const float* obs;             /* [n_rows][n_in] (PhysicsVAE: n_in = 2 Db) */
    const float* noise;           /* [n_rows][k] standard-normal draws, or NULL: Philox; never read with explore 0 */
    const int32_t* out_row;       /* [n_rows] destination rows, or NULL: row r goes to row r */
    int64_t n_rows;               /* >= 1; above max_batch the call runs in chunks */
    int64_t n_dst_rows;           /* rows of every output column; without out_row >= n_rows */
    int32_t k;                    /* actions per row */
    int32_t explore;              /* 0 or 1 */
    uint64_t rng_seed, rng_offset; /* Philox: chunk i draws at (rng_seed, rng_offset + i) */
    int32_t clip;                 /* 0 or 1; 1 and out->env_actions go together: both or neither */
    float clip_low, clip_high;    /* clip 1: clip_low <= clip_high */
    int32_t reserved;
} pvae_ppo_act_in;
typedef struct pvae_ppo_act_out { /* every pointer: a column of n_dst_rows rows */
    float* actions;               /* [n_dst_rows][k], unclipped */
    float* env_actions;           /* [n_dst_rows][k], or NULL (clip 0) */
    float* old_dist;              /* [n_dst_rows][2k] = [mean | log_std] */
    float* old_logp;              /* [n_dst_rows] */
    float* vf_preds;              /* [n_dst_rows] */
    float* noise_out;             /* [n_dst_rows][k] the noise used, or NULL: not wanted; not written with explore 0 */
    float* obs_dst;               /* [n_dst_rows][n_in], or NULL: the observations are not copied */
} pvae_ppo_act_out;
int pvae_fc_ppo_act(pvae_fc* fc, const pvae_ppo_act_in* in, const pvae_gae_params* params, const pvae_ppo_act_out* out,
                    void* stream);
int pvae_ppo_act(pvae_ctx* ctx, const pvae_ppo_act_in* in, const pvae_gae_params* params, const pvae_ppo_draws* draws,
                 const pvae_ppo_act_out* out, void* stream);
int pvae_ppo_act_sizeof(int which);

/* ---- Minibatch order of the PPO learner: every pass's row order, drawn on the device from the Philox stream -------------
 * pvae_fc_ppo_sgd / pvae_ppo_sgd take the row order of every pass as `perm` (NULL: row order, no shuffling).  This call
 * makes it from a (seed, offset) of the stream the latent draws and the action noise come from, so that the learner's
 * result is a function of the module's own (seed, call counter).  The rule is the project's own (it is not RLlib's
 * shuffle) and is integer arithmetic only: `ppo.minibatch_order` reproduces it bit for bit in numpy.  For a train batch of
 * n_rows rows and pass p of num_sgd_iter:
 *   w[0..3](g)  = Philox4x32-10(counter = {lo32(offset), hi32(offset), g, 0xC0000000 + p}, key = {lo32(seed), hi32(seed)})
 *   key32(p, i) = w[i & 3](i >> 2)                  one Philox call serves four consecutive rows
 *   packed(p,i) = (uint64(key32(p, i)) << 32) | i   unique: equal 32-bit keys are ordered by row
 *   perm[p]     = the rows i = 0 .. n_rows - 1 sorted by packed(p, i), ascending
 * Minibatch j of pass p takes rows perm[p][j * mb .. (j + 1) * mb - 1].  The counter's fourth word keeps the order apart
 * from the other streams at the same offset: latent draws use groups below Z / 4, action noise groups from 0x80000000,
 * the order groups from 0xC0000000 -- hence num_sgd_iter < 2^30.
 *
 * Launches (all on `stream`; no atomics, no workgroup waits for another, no allocation, no host synchronisation):
 *   n_rows <= 8192   ONE: a workgroup per pass forms the packed keys in LDS (64 KiB), sorts them there (a bitonic network
 *                    over max(256, next power of two >= n_rows) keys, all-ones keys behind the rows) and writes perm.
 *   n_rows >  8192   1 + ceil(log2(tiles)), tiles = ceil(n_rows / 8192): the same kernel sorts every tile of every pass into
 *                    the scratch, then each merge launch doubles the sorted run (every key finds its rank in the sibling
 *                    run by binary search), ping-pong between the scratch's two buffers; the last one writes perm.
 * Scratch: 16 bytes (unused) up to 8192 rows; above, two buffers of uint64 [num_sgd_iter][n_rows], one behind the other.
 *
 *   pvae_ppo_order_workspace_bytes   size of the scratch, a multiple of 16; 0 on error
 *   pvae_ppo_order                   perm: device int32 [num_sgd_iter][n_rows].  Returns the number of launches it
 *                                    enqueued, or a negative code and launches nothing.
 * Refused with a message, before any HIP call: n_rows < 1 or >= 2^31, num_sgd_iter < 1 or >= 2^30, perm NULL or not
 * 4-byte aligned, scratch NULL or not 16-byte aligned, scratch_bytes below the size above. */
size_t pvae_ppo_order_workspace_bytes(int64_t n_rows, int32_t num_sgd_iter);
int pvae_ppo_order(int64_t n_rows, int32_t num_sgd_iter, uint64_t seed, uint64_t offset, int32_t* perm, void* scratch,
                   size_t scratch_bytes, void* stream);

/* Per-kernel timing with HIP events on the launch stream (bench.py's `roofline` object).
 * While enabled every contraction launch carries an event pair stamped by the device at the
 * kernel's own start and end (hipExtLaunchKernelGGL), i.e. the duration rocprofv3 --kernel-trace
 * reports, without the launch seam (this serialises the host a little, so it is used in a
 * separate instrumented pass, never in a timed region).
 * category: 0 = forward kernel (32x32 / 64x32 tiles), 5 = forward kernel of the narrow layers (16x16 tiles: output
 * layers, the fused-loss layer), 1 = input-gradient kernel (alone), 2 = weight-gradient(+Adam)
 * launches (single or the two trailing layers in one launch), 3 = fused input-gradient +
 * weight-gradient(+Adam) launch, 4 = the RCCL all-reduce of pvae_allreduce_grads /
 * pvae_dp_train_step (events recorded on the stream around the collective; total_flops then
 * carries the payload BYTES).
 * pvae_profile_read synchronises on the recorded events and returns the summed duration
 * (ms), launch count and ALGORITHMIC flops (2*rows*n_in*n_out on the unpadded dims). */
int pvae_profile_enable(int on);
/* Shader clock the chip sustains while every SIMD issues fp32 MFMAs back to back on `operands` (>= 8192
 * floats of representative data, e.g. the parameter arena; DVFS makes this depend on the data: zeros run at
 * the 2.4 GHz spec clock, trained weights ~10 % lower) and the fp32-MFMA peak that clock allows
 * (CUs x 256 FLOP/clk x clock).  `scratch` = 512 device floats.  Synchronises `stream` (measurement aid for
 * bench.py: context for `roofline.frac`, which is quoted against the 2.4 GHz spec peak). */
int pvae_mfma_clock_probe(const float* operands, int64_t n_operands, float* scratch, double* ghz,
                          double* tflops_peak, void* stream);
int pvae_profile_read(int category, double* total_ms, int64_t* launches, double* total_flops);

/* GEMM micro-entry for kernel-level parity/roofline probes:
 * kind 0: C[M][N] = relu?(A[M][K] * W[N][K]^T + bias)   (forward layer)
 * kind 1: C[M][K] = (dZ[M][N] * W[N][K]) (.* (mask > 0)) (input gradient)
 * kind 2: C[N][K] = dZ[M][N]^T * X[M][K]                 (weight gradient)
 * All dims multiples of 64 (M of 32), leading dims given in floats. */
int pvae_gemm_probe(int kind, const float* a, int lda, const float* b, int ldb, float* c, int ldc,
                    const float* bias_or_mask, int ld_mask, int m, int n, int k, int relu,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PVAE_H */
