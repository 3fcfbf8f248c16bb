/*
 * crowdmod_hip.h -- C ABI of libcrowdmod_hip.so: the MI355X-native DDPM-UNet
 * denoiser + sampler hot path of marcemq/crowdmod-ddpm-4D.
 *
 * The reference has no FFI of its own: the seam is three Python call
 * signatures plus the checkpoint format.  Each entry
 * point below names the reference interface it replaces.  All tensors that
 * cross this ABI use the REFERENCE layout [B, C, H(rows), W(cols), L(frames)]
 * fp32 contiguous, L innermost (utils/dataset.py:48-51); the library permutes
 * to its internal channels-last layout on the device.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure;
 *     cm_last_error() returns a thread-local description of the last failure;
 *   - no exceptions cross the ABI; no torch / C++ types in signatures;
 *   - handles are opaque, created and destroyed by the caller;
 *   - the caller owns every buffer it passes in;
 *   - "d_" pointers are device pointers on the handle's device, "h_" host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the handle's stream);
 *   - one handle is not thread-safe; distinct handles on distinct devices are.
 */
#ifndef CROWDMOD_HIP_H
#define CROWDMOD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CM_ABI_VERSION 3
#define CM_MAX_LEVELS 8

typedef struct cm_model cm_model;       /* UNet denoiser: weights + workspace   */
typedef struct cm_schedule cm_schedule; /* ForwardSampler / DDPM schedule tables */

/* Hyper-parameters of reference UNet.__init__ (models/backbones/unet.py:11-25)
 * plus the tensor geometry the reference takes from cfg.MACROPROPS / cfg.DATASET
 * (models/diffusion/ddpm.py:211). */
typedef struct cm_unet_config {
  int32_t in_channels;                    /* mprops_count: 3 or 4               */
  int32_t out_channels;
  int32_t num_res_blocks;                 /* NUM_RES_BLOCKS                     */
  int32_t base_channels;                  /* BASE_CH (multiple of 8)            */
  int32_t n_levels;                       /* len(BASE_CH_MULT)                  */
  int32_t channel_mult[CM_MAX_LEVELS];    /* BASE_CH_MULT                       */
  int32_t apply_attention[CM_MAX_LEVELS]; /* APPLY_ATTENTION (first n_levels)   */
  int32_t time_multiple;                  /* TIME_EMB_MULT                      */
  int32_t rows, cols;                     /* MACROPROPS.ROWS / COLS             */
  int32_t past_len, future_len;           /* DATASET.PAST_LEN / FUTURE_LEN      */
  int32_t max_batch;                      /* workspace is sized for this batch  */
  int32_t device;                         /* HIP device ordinal; < 0: host-only handle (state_dict plan:
                                             names, shapes, set / get) that can never be finalized      */
} cm_unet_config;

/* Hyper-parameters of reference DiT4D_V4.__init__ (models/backbones/DiT4D_V4.py:235-254) plus the tensor geometry, as
 * DDPM_model builds it for arch "DDPM-DiT" (models/diffusion/ddpm.py:88-104).  A DiT handle is the same opaque cm_model,
 * tagged with its backbone: cm_model_destroy / num_params / param_info / set_param / get_param / set_precision (F32 or F16;
 * FM-DiT: F32 or F16A, see there) / finalize / cm_unet_forward[_host] (the denoiser forward) / cm_sample_loop[_host] / cm_model_cost work on it, and
 * cm_debug_activation serves "patch_embed" and "blocks.<i>" (see there); every other handle entry point (training,
 * dropout width, the conv and loop debug hooks, profiling, FLOP splits) returns non-zero. */
typedef struct cm_dit_config {
  int32_t in_channels;                    /* mprops_count                                        */
  int32_t out_channels;
  int32_t rows, cols;                     /* MACROPROPS.ROWS / COLS (multiples of patch_size)    */
  int32_t past_len, future_len;           /* DATASET.PAST_LEN / FUTURE_LEN                       */
  int32_t patch_size;                     /* PATCH_SIZE                                          */
  int32_t t_patch_size;                   /* T_PATCH_SIZE (divides past_len + future_len)        */
  int32_t hidden_size;                    /* HIDDEN_SIZE = num_heads * 64                        */
  int32_t depth;                          /* DEPTH                                               */
  int32_t num_heads;                      /* NUM_HEADS                                           */
  int32_t mlp_hidden;                     /* int(HIDDEN_SIZE * MLP_RATIO), a multiple of 64      */
  int32_t time_multiple;                  /* TIME_EMB_MULT                                       */
  int32_t t_max;                          /* T_max (constructor default 32)                      */
  int32_t max_batch;                      /* workspace is sized for this batch                   */
  int32_t device;                         /* HIP device ordinal; < 0: host-only handle            */
} cm_dit_config;

/* Hyper-parameters of reference DiT2D.__init__ (models/backbones/DiT2D.py:152-168) plus the tensor geometry, as FM_model
 * builds it for arch "FM-DiT" (models/flow_matching/flow_matching.py:72-84): one patch embedding per frame, one
 * self-attention over all (past_len + future_len) * (rows / patch_size) * (cols / patch_size) tokens of a sample per
 * block.  The handle is the same opaque cm_model and serves the entry points a cm_dit_config handle serves. */
typedef struct cm_dit2d_config {
  int32_t in_channels;                    /* mprops_count                                        */
  int32_t out_channels;
  int32_t rows, cols;                     /* MACROPROPS.ROWS / COLS (multiples of patch_size)    */
  int32_t past_len, future_len;           /* DATASET.PAST_LEN / FUTURE_LEN                       */
  int32_t patch_size;                     /* PATCH_SIZE                                          */
  int32_t hidden_size;                    /* HIDDEN_SIZE = num_heads * 64                        */
  int32_t depth;                          /* DEPTH                                               */
  int32_t num_heads;                      /* NUM_HEADS                                           */
  int32_t mlp_hidden;                     /* int(HIDDEN_SIZE * MLP_RATIO), a multiple of 64      */
  int32_t time_multiple;                  /* TIME_EMB_MULT                                       */
  int32_t t_max;                          /* rows of temporal_pos_embed (constructor default 8, which FM_model keeps) */
  int32_t max_batch;                      /* workspace is sized for this batch                   */
  int32_t device;                         /* HIP device ordinal; < 0: host-only handle            */
} cm_dit2d_config;

/* ---- errors / info ------------------------------------------------------ */
const char *cm_last_error(void);
int cm_abi_version(void);
int cm_device_count(int *count);

/* ---- raw device memory (for hosts without a tensor library) ------------- */
int cm_malloc(int device, void **d_ptr, size_t bytes);
int cm_free(int device, void *d_ptr);
int cm_memcpy_h2d(int device, void *d_dst, const void *h_src, size_t bytes);
int cm_memcpy_d2h(int device, void *h_dst, const void *d_src, size_t bytes);
int cm_memcpy_d2d(int device, void *d_dst, const void *d_src, size_t bytes);
int cm_device_synchronize(int device);

/* ---- denoiser: replaces UNet(...) / .load_state_dict / .state_dict ------ */
/* unet.py:11-122 (ctor). */
int cm_model_create(const cm_unet_config *cfg, cm_model **out);
/* DiT4D_V4.__init__ (DiT4D_V4.py:235-315): 15 + 14 * depth state_dict tensors in the reference's order.  Refused with a
 * status: a grid not divisible by patch_size, past_len + future_len not divisible by t_patch_size, more temporal slots
 * than temporal_pos_embed has (t_max / t_patch_size), hidden_size not divisible by num_heads, a head dim other than 64,
 * mlp_hidden not a multiple of 64, more than 64 spatial patches or 8 temporal slots. */
int cm_model_create_dit(const cm_dit_config *cfg, cm_model **out);
/* DiT2D.__init__ (DiT2D.py:152-214): 15 + 10 * depth state_dict tensors in the reference's order.  Refused with a status
 * that names the limit: channels outside [1,8], a grid not divisible by patch_size, past_len + future_len above t_max
 * (DiT2D.py:244), hidden_size not divisible by num_heads, a head dim other than 64, mlp_hidden not a positive multiple
 * of 64, more than 1024 tokens per sample.  There is no limit on the patches per frame. */
int cm_model_create_dit2d(const cm_dit2d_config *cfg, cm_model **out);
int cm_model_destroy(cm_model *m);
/* state_dict() enumeration: names and shapes are the reference's (169 tensors
 * for config/ATC.yml; conv weights [Co,Ci,kH,kW,kL]). */
int cm_model_num_params(const cm_model *m, int32_t *count);
int cm_model_param_info(const cm_model *m, int32_t index, const char **name, int64_t shape[5],
                        int32_t *ndim);
/* load_state_dict(): ddpm.py:161,288.  `numel` must match the tensor's size. */
int cm_model_set_param(cm_model *m, const char *name, const float *h_data, int64_t numel);
int cm_model_get_param(const cm_model *m, const char *name, float *h_data, int64_t numel);
/* Matrix-core operand type of the inference plan, chosen before cm_model_finalize.  CM_PRECISION_F32 (default):
 * fp32 arithmetic everywhere -- fp32 tensors and accumulation; products on fp32 matrix instructions or, in the 3x3x3 layers that
 * carry most of the FLOPs, formed from exact-remainder splits of both operands on the 16-bit matrix instructions (f16 two-way
 * splits / three cross terms where the operand range is bounded, bf16 three-way splits / six cross terms otherwise and in the
 * training step): the measured error against the reference is that of an fp32 chain (rms 4e-7).
 * CM_PRECISION_F16: the Winograd 3x3x3 layers (every stride-1 3x3x3 conv with an even
 * in-plane grid: 71-98 % of the FLOPs) contract f16 operands with fp32 accumulation (v_mfma_f32_32x32x16_f16);
 * GroupNorm statistics, SiLU, residuals, attention and the sampler update stay fp32.  The reference's analogue is
 * torch.amp.autocast around the denoiser (models/diffusion/ddpm.py:116-120).  Tolerance: tests/test_gpu_f16.py.
 * CM_PRECISION_F32R ("relaxed fp32"): fp32 tensors and fp32 accumulation as in the default plan, but the layers whose fp32
 * products are formed from bf16 splits keep only the three leading cross terms of the six (hi x hi, hi x mid, mid x hi: two-way
 * splits, ~16 mantissa bits per product instead of 24) -- the analogue of PyTorch's default conv arithmetic on the reference's own
 * GPUs (torch.backends.cudnn.allow_tf32 = True: 10 mantissa bits), six bits finer.  Inference only; the forward stays inside the
 * 1e-4 max-abs bound against the reference (tests/test_gpu_relaxed.py), not inside the default plan's 2e-6.
 * CM_PRECISION_F32X ("strict fp32", round 3's arithmetic): the default plan with the f16 two-way-split form switched off -- every
 * split layer forms its products from exact three-way bf16 splits, six cross terms (all 24 mantissa bits of both operands, dropped
 * terms <= 2^-24 of a product, fp32's whole exponent range).  Same measured error as the default plan, 16 % slower; for callers
 * that want the stronger per-product statement, and the reference point of the A/B in DESIGN.md section 4.
 * DiT handles: a DDPM-DiT handle (cm_model_create_dit) takes CM_PRECISION_F32 (default) or CM_PRECISION_F16 -- the sampling plan
 * whose six token Linears per block (both q|k|v in-projections, both out-projections, fc1, fc2) contract f16 operands with fp32
 * accumulation: each weight rounded once at cm_model_finalize (round-to-nearest-even, no clamp; the fp32 copies stay), the
 * activation operand rounded when staged; patch embedding, final layer, conditioning tables, LayerNorm + modulate, attention,
 * gates, every tensor and the sampler stay fp32.  Inference only: cm_dit4d_train_init refuses such a handle.  Never worse than the
 * reference's own autocast forward against float64 (tests/test_gpu_dit_f16.py; DESIGN.md section 10 "f16 plan").  F32R and F32X
 * are conv split forms and are refused on it.
 * An FM-DiT handle (cm_model_create_dit2d) takes CM_PRECISION_F32 (default) or CM_PRECISION_F16A ("f16 operands, attention
 * included") and refuses the other three; DDPM-DiT and UNet handles refuse CM_PRECISION_F16A.  The f16a plan: the four token
 * Linears of every block (q|k|v, attention out-projection, fc1, fc2) contract f16 operands with fp32 accumulation exactly as above
 * (weights rounded once at cm_model_finalize, fp32 copies kept), and both products of the full self-attention run on
 * v_mfma_f32_32x32x16_f16: q * 0.125 is formed in fp32 and then rounded, k and v are rounded when loaded, p = expf(s - m) is
 * fp32, the softmax denominator accumulates the unrounded p, p is rounded as the operand of p v, and the rescale and o / den are
 * fp32.  All roundings are round-to-nearest-even without clamp: a value past 65504 becomes +-inf and surfaces as a non-finite
 * output.  Patch embedding, final layer, conditioning tables, LayerNorm statistics + modulate, gates, every tensor and the sampler
 * stay fp32.  Inference only: cm_dit_train_init refuses such a handle.  It is a name of its own because the arithmetic differs from
 * the DDPM-DiT "f16" plan, whose attention stays fp32.  Never worse than the reference's own autocast forward against float64
 * (tests/test_gpu_dit2d_f16a.py; DESIGN.md section 11 "f16a plan"). */
enum { CM_PRECISION_F32 = 0, CM_PRECISION_F16 = 1, CM_PRECISION_F32R = 2, CM_PRECISION_F32X = 3, CM_PRECISION_F16A = 4 };
int cm_model_set_precision(cm_model *m, int32_t precision);
/* Packs weights into MFMA fragment order and precomputes the time-embedding
 * tables; must be called after the last cm_model_set_param and before any
 * forward.  Fails if a tensor was never set. */
int cm_model_finalize(cm_model *m);

/* UNet.forward(future, t, past) in eval mode -- unet.py:124-167.
 *   d_future [B,C,H,W,F] f32, d_t [B] i64 in [0,1000), d_past [B,C,H,W,P] f32
 *   d_out    [B,C,H,W,F] f32 (eps_hat).  B <= max_batch. */
int cm_unet_forward(cm_model *m, const float *d_future, const int64_t *d_t, const float *d_past,
                    float *d_out, int32_t B, void *stream);
/* Same with host buffers (staged through the workspace; synchronous). */
int cm_unet_forward_host(cm_model *m, const float *h_future, const int64_t *h_t, const float *h_past,
                         float *h_out, int32_t B);
/* Training-mode forward -- unet.py:124-167 with nn.Dropout3d active (layers.py:42,71): one
 * keep-mask/(1-p) value per (sample, ResnetBlock, channel).  d_dropmask [B][width] injects the
 * masks (width from cm_model_dropout_width: the blocks in state_dict order, Cout entries each);
 * NULL draws them from the device Philox stream (seed, sample_id_base + b).  Used by
 * DDPM_model._train_step (ddpm.py:111-121) when only the prediction is wanted; the full step
 * (loss, backward, Adam) is cm_train_step below. */
int cm_model_dropout_width(const cm_model *m, int32_t *width);
int cm_unet_forward_train(cm_model *m, const float *d_future, const int64_t *d_t, const float *d_past,
                          const float *d_dropmask, float p, uint64_t seed, int64_t sample_id_base,
                          float *d_out, int32_t B, void *stream);
/* F.mse_loss(pred, target) with reduction='mean' (ddpm.py:120); the scalar lands in *h_loss. */
int cm_mse_loss(cm_model *m, const float *d_pred, const float *d_target, int64_t n, float *h_loss,
                void *stream);
/* Test hook: copy an internal activation (by reference module name, e.g.
 * "encoder_blocks.0") of the last forward to the host in reference layout
 * [B,C,H,W,L].  `shape` receives {B,C,H,W,L}.
 * DiT handle: `name` is "patch_embed" or "blocks.<i>"; the tensor is the residual stream [B, T_p*N_s, D] after that
 * stage (blocks.<i>: what a forward hook on the reference module sees; patch_embed: the tokens entering blocks.0,
 * i.e. with both position embeddings added), `shape` receives {B, T_p*N_s, D, 1, 1}.  Read-only: the
 * last forward's inputs are still in the workspace, and the forward is run again from them up to the named stage.  B
 * is the batch of the last forward (samples of an earlier, larger batch follow it); fails before the first forward. */
int cm_debug_activation(cm_model *m, const char *name, float *h_out, int64_t capacity,
                        int64_t shape[5]);
/* Test hook, finalized FM-DiT (DiT2D) handles only (other handles are refused by name): ONE launch of the full-attention kernel of
 * the handle's plan -- dit_attn_full_kernel on the fp32 plan, dit_attn_full_f16_kernel on the f16a plan -- on host q|k|v
 * h_qkv [B][S][3E] (S = (past_len + future_len) * patches, E = hidden_size), result to host h_out [B][S][E].  1 <= B <= max_batch.
 * It goes through the handle's own QKV / AO workspace, which every forward rewrites before reading. */
int cm_debug_dit_attn(cm_model *m, const float *h_qkv, float *h_out, int32_t B);

/* ---- schedule: replaces ForwardSampler.__init__ (forward.py:10-27) ------ */
int cm_schedule_create(int32_t timesteps, float scale, float beta_start, float beta_end,
                       int32_t device, cm_schedule **out);
int cm_schedule_destroy(cm_schedule *s);
enum {
  CM_TAB_BETA = 0,
  CM_TAB_ALPHA = 1,
  CM_TAB_ALPHA_BAR = 2,
  CM_TAB_SQRT_ALPHA_BAR = 3,
  CM_TAB_ONE_BY_SQRT_ALPHA = 4,
  CM_TAB_SQRT_ONE_MINUS_ALPHA_BAR = 5
};
/* The six [T] buffers the reference exposes as attributes (ddpm.py:246-248). */
int cm_schedule_table(const cm_schedule *s, int32_t which, float *h_out, int32_t capacity);

/* ---- sampler steps ------------------------------------------------------- */
/* ForwardSampler.forward (forward.py:29-36) with the noise supplied by the
 * caller: d_xt = sqrt_alpha_bar[t_b] * x0 + sqrt_one_minus_alpha_bar[t_b] * eps.
 * per_sample = C*H*W*F. */
int cm_q_sample(const cm_schedule *s, const float *d_x0, const int64_t *d_t, const float *d_eps,
                float *d_xt, int32_t B, int64_t per_sample, void *stream);
/* DDPM.step (ddpm.py:25-38): d_x is updated in place.  d_noise == NULL draws
 * z from the device Philox stream (seed, sample_id_base + b, step t); it is
 * ignored (z = 0) when t == 0, as in the reference. */
int cm_ddpm_step(const cm_schedule *s, const float *d_eps, float *d_x, int32_t t, const float *d_noise,
                 uint64_t seed, int64_t sample_id_base, int32_t B, int64_t per_sample, void *stream);

/* ---- whole reverse loop --------------------------------------------------- */
enum { CM_SAMPLER_DDPM = 0, CM_SAMPLER_DDIM = 1, CM_SAMPLER_FM_EULER = 2 };
enum { CM_GUIDANCE_NONE = 0, CM_GUIDANCE_SPARSITY = 1, CM_GUIDANCE_MASS_PRESERVATION = 2 };

typedef struct cm_sample_opts {
  int32_t sampler;        /* cfg.MODEL.DDPM.SAMPLER                              */
  int32_t guidance;       /* cfg.MODEL.DDPM.GUIDANCE: "None" | "Sparsity" | "mass_preservation" (CM_GUIDANCE_*).
                             Sparsity (ddpm.py:223-226, 268-271): x[:,0] -= lambda_guidance * sqrt(beta_t) * sign(x[:,0])
                             after every DDPM / DDIM step.  mass_preservation (ddpm.py:227-229): after every DDPM step
                             x -= (1 - alpha_t) * cm_mass_preservation_grad(x, delta_t = 1, delta_l = 1, eps = 0.1), the
                             history row holding the guided x; with CM_SAMPLER_DDIM / CM_SAMPLER_FM_EULER it is ignored,
                             as in the reference.  Needs in_channels >= 3. */
  float lambda_guidance;  /* cfg.MODEL.DDPM.LAMBDA_GUIDANCE                      */
  float ddim_sigma;       /* cfg.MODEL.DDPM.SIGMA                                */
  int32_t ddim_divider;   /* cfg.MODEL.DDPM.DDIM_DIVIDER: taus = arange(0,T-1,d) */
  int32_t first_steps;    /* >0: run only the first n visited steps (benchmarks) */
  uint64_t seed;          /* device RNG seed (used when x_T / noise are NULL)    */
  int64_t sample_id_base; /* global index of sample 0 (batch sharding)           */
  int32_t use_graph;      /* 1: capture one step as a hipGraph (per-step scalars in a device table) and replay
                             it for the remaining steps; the call then returns after the loop has finished   */
  int32_t check_finite;   /* 1: after the last step count the non-finite elements of x_0; the call then returns
                             after the loop has finished, with a non-zero status (and the count in
                             cm_last_error) if any element is NaN / Inf -- the sampler-output health check
                             (the reference's analogue is the NaN stop of its training loop, ddpm.py:183-192) */
  /* CM_SAMPLER_FM_EULER -- FM_model.sampling_with_euler (models/flow_matching/flow_matching.py:203-224), on any
   * denoiser handle (UNet, DiT4D_V4, DiT2D):
   * x <- x + (1/N) u(x, idx_i, past) for t_i = linspace(0,1,N)[i], idx_i = clamp(t_i * TIME_MAX_POS, 0,
   * TIME_MAX_POS-1) truncated; the schedule handle is not consulted. */
  int32_t fm_steps;        /* cfg.MODEL.FM.INTEGRATOR_STEPS.EULER                 */
  int32_t fm_time_max_pos; /* cfg.MODEL.FM.TIME_MAX_POS (<= 1000 table rows)      */
} cm_sample_opts;

/* DDPM_model._generate_ddpm / _generate_ddim (ddpm.py:206-282): all T (or
 * len(taus)) steps run on the device behind this one call.
 *   d_past   [B,C,H,W,P]
 *   d_xT     [B,C,H,W,F] or NULL (draw from the device RNG)
 *   d_noise  [nsteps,B,C,H,W,F] in visiting order, or NULL (device RNG).
 *            DDPM: step k is t = T-1-k, rows for t = 0 are not read
 *            (nsteps = T-1 suffices); DDIM: step k is reversed(taus)[k].
 *   d_out    [B,C,H,W,F] final sample x_0
 *   d_history NULL, or [nsteps+1,B,C,H,W,F]: x_T followed by x after every step
 *            (the `history=True` list of the reference). */
int cm_sample_loop(cm_model *m, const cm_schedule *s, const float *d_past, const float *d_xT,
                   const float *d_noise, const cm_sample_opts *opts, float *d_out, float *d_history,
                   int32_t B, void *stream);
/* Host-buffer variant (synchronous). */
int cm_sample_loop_host(cm_model *m, const cm_schedule *s, const float *h_past, const float *h_xT,
                        const float *h_noise, const cm_sample_opts *opts, float *h_out,
                        float *h_history, int32_t B);
/* Number of UNet evaluations cm_sample_loop performs for these options. */
int cm_sample_num_steps(const cm_schedule *s, const cm_sample_opts *opts, int32_t *nsteps);

/* ---- instrumentation ------------------------------------------------------ */
/* Per-kernel-class device time of the LAST forward/loop, measured with HIP
 * events on the launch stream when enabled (adds synchronisation; off by
 * default).  classes: 0 conv3x3x3, 1 conv1x1x1/GEMM, 2 stats+GN, 3 attention,
 * 4 elementwise (assemble/step).  `ms` and `launches` hold 8 entries. */
int cm_profile_enable(cm_model *m, int32_t on);
int cm_profile_read(cm_model *m, float ms[8], int64_t launches[8]);
/* Per class: length (ms) of the UNION of its launch intervals over all batch lanes of the last profiled call -- with
   two lanes the launches of a class overlap, so the sum of their durations in cm_profile_read exceeds the wall time
   they occupied; with one lane the two agree. */
int cm_profile_read_union(cm_model *m, float ms[8]);
/* Text table of the per-launch averages behind cm_profile_read (one line per op). */
int cm_profile_report(cm_model *m, char *buf, int64_t capacity);
/* Algorithmic FLOPs and bytes of one forward at batch B. */
int cm_model_cost(const cm_model *m, int32_t B, double *flops, double *bytes);
/* Algorithmic FLOPs of one forward per kernel class (same indices as cm_profile_read). */
int cm_model_class_flops(const cm_model *m, int32_t B, double flops[8]);
/* Matrix-core FLOPs the plan EXECUTES per class (parity-form upsample convs: 8 of 27 taps; Winograd F(2x2,3x3)
 * layers: 16 multiplies per 2x2 outputs and z tap instead of 36) -- the hardware-utilisation side of the roofline. */
int cm_model_exec_flops(const cm_model *m, int32_t B, double flops[8]);
/* The same accounting for the TRAINING forward in the handle's current mode (cm_train_set_autocast): flops = all executed
 * matrix-core FLOPs per kernel class, f16 = the part of the convolutions that runs on f16 operands (0 with the mode off). */
int cm_train_exec_flops(const cm_model *m, int32_t B, double flops[8], double f16[8]);
/* The same FLOPs by the matrix instruction that issues them: `f32` = issued as fp32 instructions (v_mfma_f32_32x32x2_f32),
 * `b16` = ISSUED FLOPs of 16-bit-operand instructions (v_mfma_f32_32x32x16_{bf16,f16}): a six-term layer -- fp32 products
 * from exact three-way bf16 splits -- issues six of them per fp32-equivalent product, an f16-plan layer one.  The time the
 * matrix pipe needs at its peaks is f32 / peak_fp32 + b16 / peak_16bit: the numerator of bench.py's roofline fraction. */
int cm_model_issue_flops(const cm_model *m, int32_t B, double f32[8], double b16[8]);

/* ---- sampling metrics: the per-frame reductions of utils/metrics/metricsGenerator.py:70-92,
 * 120-186,293-339 (PSNR, masked PSNR, relative density error, total variation) on the device.
 *   d_pred, d_gt [N,C,H,W,F] f32 (device);  h_out [N][C][F][8] f64: sse, masked sse, masked count
 *   (mask = gt[:,0] > 1e-5), tv_pred, tv_gt, sum_pred, sum_gt, 0;  h_minmax [N][C][F][2] f32: min / max
 *   of the gt plane.  The log10 / max-over-repeats tail on [N,C,F] numbers stays on the host. */
int cm_frame_metrics(int32_t device, const float *d_pred, const float *d_gt, int32_t N, int32_t C, int32_t H,
                     int32_t W, int32_t F, double *h_out, float *h_minmax);

/* ---- sampling metrics: the SSIM, energy and motion-feature tables on the device (cm_metrics.hip) ----
 * The host route (crowdmod-ddpm-4d_amd/metrics.py: _ssim2d, compute_energy, _mf_polar, motion_feature_vectors,
 * bhattacharyya) is the yardstick these restate.  Inputs are float32 device tensors [N,C,H,W,F], F innermost; results are
 * float64 host arrays.  Every argument is checked before the first device call.  Each output element has one writer, every
 * floating-point sum a fixed order, and the only atomics are integer LDS counters: two runs give identical bits.
 *
 * cm_ssim_frames: h_out[n][c][f] = mean SSIM of the (sample, channel, frame) image pair -- 7 x 7 uniform window, only the
 *   (H - 6)(W - 6) windows wholly inside the image, cov_norm = 49 / 48, C1 = (0.01 R)^2, C2 = (0.03 R)^2 with R = h_range[c],
 *   v = cov_norm (mean(x^2) - mean(x)^2) and so on; everything in float64.  min(H, W) < 7 is refused (the host raises
 *   ValueError), and so is W * F > 1024 (a band of rows is staged in LDS; H is not limited).
 *
 * cm_energy: h_out[n] = compute_energy (models/guidance.py:10-42) of x[n]: the residual f = term1 + term2 + term3 + term4
 *   over interior cells in float32, in the host's operation order without fused multiply-add; f f and the sum in float64;
 *   0.5 sum / (H W L).  h_factor [C] (or NULL) multiplies each channel in float32 first.  C < 3 is refused; a grid with no
 *   interior cell (H < 3, W < 3 or L < 2) gives 0.
 *
 * cm_motion_feature_vectors / cm_motion_feature_tables (utils/metrics/motionFeatureExtractor.py:34-59,166-303,
 *   metricsGenerator.py:240-258; 16 x 16 bins, volumes of f frames x k x k cells, ragged at the far edges, in
 *   (frame block, row block, column block) order).  `vectors` returns the two normalised vectors of d_seq (h_mf2
 *   [N][nvol 256], h_mf1 [N][nvol 16]); `tables` returns per sample MSE 2-D, MSE 1-D, Bhattacharyya distance 2-D, 1-D,
 *   coefficient 2-D, 1-D (h_out [N][6]) without materialising the vectors: its device workspace is those six numbers.
 *   C < 3, f < 1, k < 1 are refused.  The arithmetic that decides a bin:
 *     magnitude   sqrt(vx vx + vy vy) in float32 (each product rounded, then the sum, then a correctly rounded root),
 *                 widened; per grid cell lo / hi over its F frames, rng = hi - lo (1 when below 10 DBL_EPSILON),
 *                 scale = 255.0 / rng, y = mag scale + (0.0 - lo scale) + 1.0 in that order in IEEE float64 without
 *                 contraction, lm = log2(y).  A NaN in any frame of a cell makes its lo / hi NaN: all its frames leave
 *                 the 2-D histogram (and carry a NaN weight in the 1-D one, as on the host); no other cell changes.
 *     top edge    decided on y, not on the device's log2: 256 <= y <= 256 + 2 * 2^-44 is the last magnitude bin (a
 *                 correctly rounded log2 gives 8.0 exactly there, which histogram2d keeps), anything above and NaN are
 *                 outside, every y below 256 stays at or below bin 15.  Interior edges i / 2 are decided on lm.
 *     angle       atan2f(vy, vx) in float32, widened; edges -pi + i pi / 8 in float64; the 2-D histogram closes its last
 *                 bin on == pi (float64), the 1-D one does not; float32 +-pi fall outside both.
 *     bins        searchsorted(side = 'right') - 1; the whole first magnitude bin moves to angle bin 8.
 *     1-D weight  lm ** gamma in float64.  Normalisers: sum + 1.
 *     tables      MSE = mean over all nvol 256 (nvol 16) bins of the squared difference of the two normalised values (the
 *                 difference is formed per bin: identical sequences give exactly 0); coefficient = clip(sum sqrt(P Q),
 *                 0.01, 1), distance = -log(coefficient). */
int cm_ssim_frames(int32_t device, const float *d_pred, const float *d_gt, int32_t N, int32_t C, int32_t H, int32_t W,
                   int32_t F, const double *h_range, double *h_out);
int cm_energy(int32_t device, const float *d_x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t L, float delta_t,
              float delta_l, const float *h_factor, double *h_out);
int cm_motion_feature_vectors(int32_t device, const float *d_seq, int32_t N, int32_t C, int32_t H, int32_t W, int32_t F,
                              int32_t f, int32_t k, double gamma, double *h_mf2, double *h_mf1);
int cm_motion_feature_tables(int32_t device, const float *d_pred, const float *d_gt, int32_t N, int32_t C, int32_t H,
                             int32_t W, int32_t F, int32_t f, int32_t k, double gamma, double *h_out);

/* ---- mass_preservation guidance: preservationMassNumericalGradientOptimal (models/guidance.py:44-69) ----
 * d_grad[i] = (E(x + eps e_i) - E(x)) / eps for every element i of d_x [B,C,H,W,L], E = compute_energy(x, delta_t,
 * delta_l) (guidance.py:10-42) -- the reference's forward-difference quotient, evaluated in closed form (f is linear in
 * every single element: at most four residual cells per element).  Channels >= 3 and elements
 * no residual cell touches get exactly 0; H < 3, W < 3 or L < 2 give all zeros.  C < 3 is an error (the energy reads
 * channels 0-2).  d_grad must not alias d_x.  Asynchronous on `stream` (NULL = the device's default stream). */
int cm_mass_preservation_grad(int32_t device, const float *d_x, int32_t B, int32_t C, int32_t H, int32_t W, int32_t L,
                              float delta_t, float delta_l, float eps, float *d_grad, void *stream);

/* ---- tuning hooks (tools/tune_tiles.py): time one convolution of the plan with an explicit tile
 * geometry.  Diagnostics only -- the product path never calls them. */
/* Process-wide diagnostic switches of the conv kernels (the CM_CONV_DBG bit mask of DESIGN.md; 4096 = XCD tile
 * remap off); flags < 0 returns to the environment value.  Results are only defined for 0 / 4096 / 2048 / 512. */
int cm_debug_conv_flags(int32_t flags);
int cm_debug_conv_count(const cm_model *m, int32_t *count);
/* One line of text per op of the plan.  A convolution: "conv <label> ..." (fields: cm_model.cpp).  A fused attention block:
 * "other <label> <kernel>", <kernel> = attn_sample_kernel or attn_head_kernel -- what this handle's inference plan launches for
 * the block at the batch of its last forward (planned again on each call, not a record of a launch).  A GroupNorm finalisation, once a
 * forward has run: "other <label> fin <who> <ns0> <ns1>", <who> = qr | combine | wino | alone -- what merged its slot statistics in the
 * last forward (the whole-sample quarter-resolution conv, the second pass of a K-split conv / attention block, the Winograd
 * consumer's prologue, gn_finalize_kernel) and the slots per sample of its one or two sources.  Anything else: "other <label>". */
int cm_debug_conv_info(const cm_model *m, int32_t index, char *buf, int64_t capacity);
/* The backward plan cm_train_init built (and cm_train_set_autocast re-plans), as text: one line per launching entry in execution
 * (reverse) order.  "conv <label> wgrad <WG_...> <form> dgrad <DG_...> <form>": the kernels of the conv's weight gradient and
 * data gradient (the enumerators of cm_model.cpp) and their operand forms (fp32 | b6 | f16).  "attn <label> S <tokens> D
 * <channels per head> <lds | slab>": an attention core, and whether the S x S matrices of a (sample, head) live in LDS or in the
 * global scratch slab.  Read-only: no device call.  *needed = bytes of the whole text with its terminator; at most `capacity`
 * are written (capacity 0, buf NULL: size query).  An error before cm_train_init. */
int cm_debug_bwd_plan(const cm_model *m, char *buf, int64_t capacity, int64_t *needed);
/* Test hook: conv op `index` alone on caller data (no GroupNorm / SiLU / time row / residual / fused skip; bias stays).
 * h_in0 / h_in1: host channels-last [B][Zs][Ys][Xs][C0 / C1]; h_out: host [B][Zo][Yo][Xo][C of the output tensor -- the last
 * field of cm_debug_conv_info];
 * mode 0 = the six-term bf16 form where the plan has one (raw operands are unbounded: never the h2 form), 1 = the same layer on
 * fp32 matrix instructions (split fragments withheld), 2 = the h2 form (f16 two-way splits) where the plan has one: the caller
 * keeps |x| inside the bound the plan guarantees for that layer (8000; tests/test_gpu_h2.py), 3 = the op exactly as the sampling
 * forward launches it (GroupNorm + SiLU on load, time row, residual, fused skip conv) on the caller's sources; everything else it
 * reads is what the last forward left.  With cm_debug_conv_flags(1 << 20) -- a bit no kernel reads; any non-zero value marks a
 * diagnostic run -- the Winograd launcher takes its generic kernel instead of a specialised launch form: the two must agree
 * bit for bit (tests/test_gpu_wino_forms.py).  A CM_PRECISION_F16 handle: host data is converted to and from the tensors that
 * plan stores as _Float16 (round to nearest even), and modes 1 and 2 equal mode 0 -- that plan has one operand form per conv
 * (tests/test_gpu_f16_layers.py). */
int cm_debug_conv_io(cm_model *m, int32_t index, int32_t mode, const float *h_in0, const float *h_in1, float *h_out, int32_t B);
/* Statistics slots of conv op `index`, in the slot count of the last forward's plan: h_part [B][*nslots][*C][2], h_cnt [B][*nslots]; with null buffers
 * only the two sizes are returned. */
int cm_debug_conv_stats(cm_model *m, int32_t index, int32_t B, float *h_part, float *h_cnt, int32_t *nslots, int32_t *C);
/* Launches of the table-driven Winograd kernel per launch form since the last reset (process-wide): counts[0] = the generic kernel,
 * counts[f] = the instantiation compiled for form f (bits: 1 one sample per workgroup, 2 plain GroupNorm + SiLU load, 4 GroupNorm
 * finalised from slot partials, 8 whole full-resolution tiles). */
int cm_debug_wino_form_counts(int64_t counts[16], int32_t reset);
/* ... and how many of those launches ran the halo-ahead order of the specialised forms (halo loads a chunk period ahead of the
 * weight ring, skip-conv operands double-buffered); the form index above does not carry that bit. */
int cm_debug_wino_ahead_count(int64_t *launches, int32_t reset);
/* ... and how many of the halo-ahead launches also staged the next chunk's activated image under the current chunk's matrix phase. */
int cm_debug_wino_under_count(int64_t *launches, int32_t reset);
int cm_debug_time_conv(cm_model *m, int32_t index, int32_t MB, int32_t bz, int32_t by, int32_t bx,
                       int32_t B, int32_t iters, float *us);

/* ---- training step: replaces DDPM_model._train_step + optimizer.step() -----
 * (models/diffusion/ddpm.py:111-121,142-144; optimizer built at ddpm.py:53-56:
 * torch.optim.Adam(lr, betas, weight_decay) -- L2 coupled into the gradient.)
 * cm_train_init allocates master weights / gradients / Adam moments on the device
 * (state_dict order) and the backward workspace; call once after cm_model_finalize.
 * A shape the forward admits and the backward cannot hold is refused HERE, in words ("training refused: ..."; today: an
 * attention level with more tokens than the backward's LDS tiles hold) -- never inside a step; the handle then keeps no
 * training state and goes on as the inference handle it was.
 * The step runs in fp32 unless cm_train_set_autocast switches its Winograd layers to f16 operands (below). */
int cm_train_init(cm_model *m, float lr, float beta1, float beta2, float eps, float weight_decay,
                  float dropout_rate /* cfg DROPOUT_RATE: nn.Dropout3d(p), layers.py:42 */);
int cm_train_set_lr(cm_model *m, float lr);
/* The reference trains this UNet under torch.amp.autocast("cuda") without a GradScaler (ddpm.py:116-120).
 * 0 = fp32 step (default, today's launches), 1 = autocast: f16 matrix-core operands with fp32 accumulation in the
 * stride-1 3x3x3 layers of the Winograd route -- training forward, data gradient and weight gradient; activations,
 * gradients, GroupNorm, attention and Adam stay fp32.  The loss gradient is multiplied by 2^k and the flat gradient
 * buffer by 2^-k at the end of the backward, so every reader of the gradients sees unscaled numbers.
 * loss_scale_log2 < 0 = automatic: the largest k with 2^k <= B*C*H*W*F of the step (a function of B alone).
 * Call after cm_train_init, between steps.  Governs cm_train_step, cm_train_step_xt and cm_unet_forward_train;
 * cm_unet_forward and cm_sample_loop are untouched. */
int cm_train_set_autocast(cm_model *m, int32_t mode, int32_t loss_scale_log2);
/* *loss_scale_log2: the exponent in force (automatic: for the batch of the last step, max_batch before the first). */
int cm_train_get_autocast(const cm_model *m, int32_t *mode, int32_t *loss_scale_log2);
/* Data-parallel training: global index of this rank's sample 0 (rank * per-rank batch).  The device
 * Philox streams of eps and of the Dropout3d masks are addressed by (seed, step, GLOBAL sample index), so
 * ranks draw different noise and a job's samples draw the same numbers however it is sharded.  Default 0. */
int cm_train_set_sample_base(cm_model *m, int64_t sample_id_base);
/* One step on device buffers:
 *   x_t = q_sample(d_future, d_t, d_eps)          (forward.py:29-35 with the caller's noise)
 *   eps_hat = UNet(x_t, d_t, d_past) in train mode (Dropout3d masks: d_dropmask [B][width] or
 *             NULL -> device Philox stream keyed by (seed, step))
 *   *h_loss = mse(eps_hat, d_eps); backward; if apply_update != 0: Adam step + weight re-pack.
 * Synchronous (returns after the step has finished). */
int cm_train_step(cm_model *m, const cm_schedule *s, const float *d_future, const float *d_past,
                  const int64_t *d_t, const float *d_eps, const float *d_dropmask, uint64_t seed,
                  float *h_loss, int32_t B, int32_t apply_update, void *stream);
/* d_eps may be NULL: eps ~ N(0,1) is then drawn from the device Philox stream (seed, step, sample),
 * the analogue of torch.randn_like in forward.py:33.
 * Data-parallel use: cm_train_step(apply_update=0) on every rank, all-reduce(mean) the flat gradient
 * buffer from cm_train_flat_grads, then cm_train_apply (Adam + re-pack). */
int cm_train_flat_grads(cm_model *m, void **d_grads, int64_t *numel);
int cm_train_apply(cm_model *m, void *stream);
/* Adam state for the "opt" entry of a checkpoint (utils/utils.py:140-147): which = 0 exp_avg, 1 exp_avg_sq; any other
 * value is refused.  The three families' accessors share these rules: a copy-out (gradient, optimizer state) waits for
 * the device first; *_opt_step reads the step counter into *step, after setting it from *step when set != 0; a negative
 * step is refused and changes nothing. */
int cm_train_get_opt_state(cm_model *m, const char *name, int32_t which, float *h_out, int64_t numel);
int cm_train_set_opt_state(cm_model *m, const char *name, int32_t which, const float *h_in, int64_t numel);
int cm_train_opt_step(cm_model *m, int32_t *step, int32_t set);
/* The same step with the caller's noised input and regression target (flow matching,
 * flow_matching.py:128-146: x_t and u_target from w_linear / w_conic, d_t = (t * TIME_MAX_POS).long()):
 * eps_hat = UNet(d_xt, d_t, d_past) in train mode; *h_loss = mse(eps_hat, d_target); backward; update. */
int cm_train_step_xt(cm_model *m, const float *d_xt, const float *d_past, const int64_t *d_t,
                     const float *d_target, const float *d_dropmask, uint64_t seed, float *h_loss,
                     int32_t B, int32_t apply_update, void *stream);
/* Gradient of one state_dict tensor after the last cm_train_step (reference layout). */
int cm_train_get_grad(cm_model *m, const char *name, float *h_out, int64_t numel);
/* Copy the trained master weights back into the handle's state_dict (cm_model_get_param then
 * returns them) and refresh the eval-mode time-embedding table. */
int cm_train_sync(cm_model *m);

/* ---- FM-DiT training: replaces FM_model._train_step + optimizer.step() for arch "FM-DiT" ----
 * (models/flow_matching/flow_matching.py:104-157, models/backbones/DiT2D.py in train mode; torch.optim.Adam with
 * coupled L2.)  A family of its own: cm_train_* keep refusing DiT handles.  Only a finalized DiT2D handle on a device
 * trains; a UNet handle, a DDPM-DiT (DiT4D_V4) handle and a host-only handle are refused by name.  fp32 throughout,
 * head dim 64, at most 1024 tokens per sample, 64 heads; single GPU plus the flat-gradient protocol below.
 * cm_dit_train_init allocates the master weights, gradients and Adam moments (flat, state_dict order) and the tape
 * of the train-mode forward for max_batch samples; dropout_rate is DiT2D's DROPOUT_RATE (attention probabilities,
 * after GELU, after fc2), in [0, 1). */
int cm_dit_train_init(cm_model *m, float lr, float beta1, float beta2, float eps, float weight_decay,
                      float dropout_rate);
int cm_dit_train_set_lr(cm_model *m, float lr);
/* Global index of this rank's sample 0: the dropout masks are a function of (seed, optimizer step, GLOBAL sample
 * index, block, site, head, row, column), so a sample's masks do not depend on its batch.  Indices stay below 2^32. */
int cm_dit_train_set_sample_base(cm_model *m, int64_t sample_id_base);
/* One step on device buffers: u_hat = DiT2D(d_xt, d_t, d_past) in train mode (masks from the device Philox stream
 * keyed by `seed`); *h_loss = mse(u_hat, d_target); backward; if apply_update != 0: Adam.  Synchronous. */
int cm_dit_train_step_xt(cm_model *m, const float *d_xt, const float *d_past, const int64_t *d_t,
                         const float *d_target, uint64_t seed, float *h_loss, int32_t B, int32_t apply_update,
                         void *stream);
/* Data-parallel use: step(apply_update=0) on every rank, all-reduce(mean) the flat buffer, cm_dit_train_apply. */
int cm_dit_train_flat_grads(cm_model *m, void **d_grads, int64_t *numel);
int cm_dit_train_apply(cm_model *m, void *stream);
int cm_dit_train_get_grad(cm_model *m, const char *name, float *h_out, int64_t numel);
/* which = 0 exp_avg, 1 exp_avg_sq, 2 (get only) the master weights, anything else is refused; the step counter as in
 * cm_train_opt_step. */
int cm_dit_train_get_opt_state(cm_model *m, const char *name, int32_t which, float *h_out, int64_t numel);
int cm_dit_train_set_opt_state(cm_model *m, const char *name, int32_t which, const float *h_in, int64_t numel);
int cm_dit_train_opt_step(cm_model *m, int32_t *step, int32_t set);
/* Copy the master weights into the handle's state_dict and the eval path's weights, and rebuild the eval path's
 * 1000-row conditioning table from them.  Until this call the eval forward computes what it did before training. */
int cm_dit_train_sync(cm_model *m);
/* The train-mode prediction [B,C,H,W,F] of the last step (host buffer). */
int cm_dit_train_get_pred(cm_model *m, float *h_out, int64_t numel);

/* ---- DDPM-DiT training: DDPM_model._train_step (models/diffusion/ddpm.py:111-154) on the DiT4D_V4 denoiser --------------
 * (t ~ U{0..T-1}; (x_t, eps) = q_sample(future, t); eps_hat = DiT4D_V4(x_t, t, past) in train mode; loss = mse(eps_hat,
 * eps); backward; torch.optim.Adam with coupled L2.  The reference runs this step under fp16 autocast; the path is
 * fp32 unless cm_dit4d_train_set_autocast switches the blocks' token Linears to f16 operands, below.)
 * The sibling of cm_dit_train_*, entry for entry; only a finalized DiT4D_V4 handle on a device
 * trains: a UNet handle, an FM-DiT (DiT2D) handle and a host-only handle are refused by name.  Head dim 64, at most 64
 * heads.  dropout_rate is DiT4D_V4's DROPOUT_RATE (both attentions' probabilities, after GELU, after fc2), in [0, 1);
 * the masks are a function of (seed, optimizer step, GLOBAL sample index, block, site, head, row, column). */
int cm_dit4d_train_init(cm_model *m, float lr, float beta1, float beta2, float eps, float weight_decay,
                        float dropout_rate);
int cm_dit4d_train_set_lr(cm_model *m, float lr);
int cm_dit4d_train_set_sample_base(cm_model *m, int64_t sample_id_base);
/* The reference trains this denoiser under torch.amp.autocast("cuda") without a GradScaler (ddpm.py:116-120).
 * 0 = fp32 step (default: exactly the launches of a handle that never heard of the mode), 1 = autocast: in every block the
 * spatial and temporal q|k|v in-projections, both out-projections, fc1 and fc2 take f16 operands with fp32 accumulation
 * (v_mfma_f32_32x32x16_f16) in the training forward, the data gradient and the weight gradient.  An operand is rounded
 * once, to nearest even, from its fp32 value when it is staged (the LayerNorm + modulate output, the saved activations, dY and
 * the fp32 master weights: no f16 weight copy exists); a value outside f16's range becomes +-inf and shows as a non-finite
 * loss.  The patch embedding, the final layer, the conditioning chain, both attention cores, LayerNorm, GELU, the gates, the
 * tape, every gradient tensor and Adam stay fp32.  The loss gradient is multiplied by 2^k and the flat gradient buffer by
 * 2^-k at the end of the backward, so every reader of the gradients sees unscaled numbers.
 * loss_scale_log2 < 0 = automatic: the largest k with 2^k <= B*C*H*W*F of the step (a function of B alone); an explicit k
 * in [0, 24] is taken as is.  Call after cm_dit4d_train_init, between steps.  Governs cm_dit4d_train_step and
 * cm_dit4d_train_step_xt; cm_unet_forward and the sampling loops are untouched.  Refused by name: a null, UNet, FM-DiT
 * (DiT2D: the reference trains flow matching in fp32) or untrained handle, and an unknown mode. */
int cm_dit4d_train_set_autocast(cm_model *m, int32_t mode, int32_t loss_scale_log2);
/* *loss_scale_log2: the exponent in force (automatic: for the batch of the last step, max_batch before the first; 0 with the
 * mode off). */
int cm_dit4d_train_get_autocast(const cm_model *m, int32_t *mode, int32_t *loss_scale_log2);
/* One step on device buffers with the caller's noised input and regression target; *h_loss = mse(eps_hat, d_target);
 * backward; if apply_update != 0: Adam.  Synchronous. */
int cm_dit4d_train_step_xt(cm_model *m, const float *d_xt, const float *d_past, const int64_t *d_t,
                           const float *d_target, uint64_t seed, float *h_loss, int32_t B, int32_t apply_update,
                           void *stream);
/* cm_train_step's shape: x_t = sqrt_alpha_bar[t] * d_future + sqrt_one_minus_alpha_bar[t] * eps, target eps.
 * d_eps == NULL draws eps ~ N(0,1) from the device Philox stream (seed, draw, global sample), as cm_train_step does. */
int cm_dit4d_train_step(cm_model *m, const cm_schedule *s, const float *d_future, const float *d_past,
                        const int64_t *d_t, const float *d_eps, uint64_t seed, float *h_loss, int32_t B,
                        int32_t apply_update, void *stream);
int cm_dit4d_train_flat_grads(cm_model *m, void **d_grads, int64_t *numel);
int cm_dit4d_train_apply(cm_model *m, void *stream);
int cm_dit4d_train_get_grad(cm_model *m, const char *name, float *h_out, int64_t numel);
/* which = 0 exp_avg, 1 exp_avg_sq, 2 (get only) the master weights */
int cm_dit4d_train_get_opt_state(cm_model *m, const char *name, int32_t which, float *h_out, int64_t numel);
int cm_dit4d_train_set_opt_state(cm_model *m, const char *name, int32_t which, const float *h_in, int64_t numel);
int cm_dit4d_train_opt_step(cm_model *m, int32_t *step, int32_t set);
/* Until this call the eval forward and the sampling loops compute what they computed before training. */
int cm_dit4d_train_sync(cm_model *m);
int cm_dit4d_train_get_pred(cm_model *m, float *h_out, int64_t numel);

/* ---- ConvRNN forecaster: replaces Forecaster(...) (models/convRNN/forecaster.py) and
 * ConvRNN_model._generate_convRNN (models/convRNN/convRNN.py:223-231) -----------------------------------
 * The deterministic ConvGRU / ConvLSTM encoder-forecaster baseline of arch "ConvRNN".  It has no timestep and no
 * sampler, so it is a handle of its own.  Exact fp32 on v_mfma_f32_32x32x2_f32 throughout by default; an opt-in f16
 * forecast plan (cm_convrnn_set_precision) forms the products of all but the first and the last conv on
 * v_mfma_f32_32x32x16_f16. */
enum { CM_CELL_GRU = 0, CM_CELL_LSTM = 1 };
typedef struct cm_convrnn_config {
  int32_t in_channels;                    /* mprops_count: 4 (channels 0 and 3 are indexed)       */
  int32_t rows, cols;                     /* MACROPROPS.ROWS / COLS: multiples of 4               */
  int32_t past_len, future_len;           /* DATASET.PAST_LEN / FUTURE_LEN, each >= 1             */
  int32_t cell;                           /* MODEL.CONVRNN.CELL_CLASS: CM_CELL_GRU / CM_CELL_LSTM */
  int32_t enc_hidden[6], forc_hidden[7];  /* ENC_HIDDEN_CH, FORC_HIDDEN_CH                        */
  int32_t enc_kernels[6], forc_kernels[7];/* ENC_KERNELS, FORC_KERNELS                            */
  int32_t max_batch;                      /* workspace is sized for this batch                    */
  int32_t device;                         /* HIP device ordinal; < 0: host-only handle (names, shapes, set / get) */
} cm_convrnn_config;
typedef struct cm_convrnn cm_convrnn;
/* Refused with a status that names the violated constraint (the reference would fail in torch.cat or in a conv):
 * in_channels != 4; rows or cols no multiple of 4; enc_kernels other than [3,3,3,3,3,3] or forc_kernels other than
 * [3,4,3,4,3,3,3]; a channel count that is no multiple of 8 in [8, 1024]; feed-through counts enc_hidden[2] ==
 * enc_hidden[1], enc_hidden[4] == enc_hidden[3], forc_hidden[0] == enc_hidden[5]; shared-state counts forc_hidden[1] ==
 * enc_hidden[5], forc_hidden[3] == enc_hidden[3], forc_hidden[5] == enc_hidden[1]; past_len or future_len < 1;
 * max_batch * rows * cols above 2^31 - 64. */
int cm_convrnn_create(const cm_convrnn_config *cfg, cm_convrnn **out);
int cm_convrnn_destroy(cm_convrnn *m);
/* state_dict() enumeration in the reference's order (bias=False: weights only): encoder.encoder_cell_list.0-5, then
 * forecaster_cell_list.0-6; 25 tensors with GRU cells, 13 with LSTM cells. */
int cm_convrnn_num_params(const cm_convrnn *m, int32_t *count);
int cm_convrnn_param_info(const cm_convrnn *m, int32_t index, const char **name, int64_t shape[4], int32_t *ndim);
int cm_convrnn_set_param(cm_convrnn *m, const char *name, const float *h_data, int64_t numel);
int cm_convrnn_get_param(const cm_convrnn *m, const char *name, float *h_data, int64_t numel);
/* The forecast plan, chosen before cm_convrnn_finalize (refused after it: create a new handle).  CM_PRECISION_F32 is the
 * default; a handle that never calls this is unchanged.  CM_PRECISION_F16: every conv launch of a forecast except the first
 * encoder conv (layer 0: it reads the observation window, data in physical units with exp applied) and the forecaster's last
 * conv (layer 12: it writes the forecast) forms its products on v_mfma_f32_32x32x16_f16.  Operands are rounded once,
 * fp32 -> f16, round-to-nearest-even, no clamp: the weights on the host in cm_convrnn_finalize, an activation when a launch
 * stages it (the GRU candidate's r * h_prev is the fp32 product, then rounded).  Products are exact, accumulation is fp32
 * with k ascending in a fixed order (64-product chains, then one add into the running sum), and everything else is fp32 and
 * the default plan's code: the accumulator tile, every epilogue (sigmoid, tanh, LeakyReLU, the GRU / LSTM state updates,
 * exp), the hidden and cell states, the window, the forecast.  One writer per output element, no atomics, and a result
 * that does not depend on the batch it ran in or on max_batch, as on the default plan.  The plan is inference only:
 * cm_convrnn_train_init and the entry points that run the training forward (cm_convrnn_loss, cm_convrnn_loss_sums,
 * cm_convrnn_train_step, cm_convrnn_train_forward) refuse an f16-plan handle and say so.  CM_PRECISION_F32R and
 * CM_PRECISION_F32X are conv split forms of the UNet and are refused. */
int cm_convrnn_set_precision(cm_convrnn *m, int32_t precision);
/* Packs the weights once and allocates the workspace; fails if a tensor was never set or on a host-only handle. */
int cm_convrnn_finalize(cm_convrnn *m);
/* Forecaster.forward(x_obs, target_obs, teacher_forcing) -- forecaster.py:89-176: all future_len steps behind one call,
 * hidden states zero at its start.
 *   d_past [B,4,H,W,P], d_target [B,4,H,W,F] (read only under teacher forcing; may be NULL otherwise),
 *   d_out [B,4,H,W,F]: the raw frames, or with exp_output != 0 with exp on channels 0 and 3 (convRNN.py:228-229). */
int cm_convrnn_forecast(cm_convrnn *m, const float *d_past, const float *d_target, int32_t teacher_forcing,
                        int32_t exp_output, float *d_out, int32_t B, void *stream);
/* Same with host buffers (synchronous). */
int cm_convrnn_forecast_host(cm_convrnn *m, const float *h_past, const float *h_target, int32_t teacher_forcing,
                             int32_t exp_output, float *h_out, int32_t B);
/* Test hook: the hidden state the last call left, as [B,C,h,w]; level 0 quarter, 1 half, 2 full resolution; which 0 = h,
 * 1 = c (LSTM only).  The caller has synchronised the stream of that call. */
int cm_convrnn_debug_state(cm_convrnn *m, int32_t level, int32_t which, float *h_out, int64_t capacity, int64_t shape[4]);
/* Test hook: ONE launch of layer `layer` (0-11 in state_dict order: encoder.encoder_cell_list.0-5, forecaster_cell_list.0-5;
 * the last conv writes the forecast itself and is reached through cm_convrnn_forecast) on host-supplied sources, with the
 * handle's weights under the handle's plan, at batch B in [1, max_batch].  Every array is a host buffer in the reference's
 * layout [B, C, h, w] at the layer's own resolution; sources are independent of each other and of the handle's states,
 * which the call leaves alone.  Synchronous.
 *   a conv layer (0, 2, 4, 7, 9, 11), part 0:  x0 [B, cin, hin, win] -> y0 [B, cout, hout, wout] (LeakyReLU applied)
 *   a GRU cell (1, 3, 5, 6, 8, 10), part 0, the gates: x0 [B, cin, h, w], x1 = h [B, hid, h, w] (the conv's second
 *     source), hprev [B, hid, h, w] (the epilogue's) -> y0 = r * hprev, y1 = u
 *   a GRU cell, part 1, the candidate: x0, x1 = r * h, hprev, u -> y0 = (1 - u) tanh(conv) + u hprev
 *   an LSTM cell, part 0: x0, x1 = h, c -> y0 = h', y1 = c'
 * Pointers a launch does not use may be NULL. */
int cm_convrnn_debug_launch(cm_convrnn *m, int32_t layer, int32_t part, const float *h_x0, const float *h_x1,
                            const float *h_hprev, const float *h_u, const float *h_c, float *h_y0, float *h_y1, int32_t B);
/* Algorithmic FLOPs and bytes of one forecast at batch B: 2 FLOPs per multiply-add of the reference's convolutions on
 * either plan; the bytes of every launch's sources, outputs and weights under the handle's plan (the f16 plan's weights
 * of layers 1-11 are two bytes each, every tensor stays fp32). */
int cm_convrnn_cost(const cm_convrnn *m, int32_t B, double *flops, double *bytes);

/* ---- ConvRNN training (convRNN.py:98-171): evaluate_loss (utils/loss.py:15-52), backpropagation through all future_len
 * steps, torch.optim.Adam(amsgrad=True) with coupled L2.  Exact fp32 products, deterministic (fixed summation order, no
 * atomics; results do not depend on max_batch).  Every entry point below refuses a host-only handle, and the ones that take
 * a batch refuse B outside [1, max_batch]; cm_last_error names the reason. */
/* Master weights, flat gradient, exp_avg, exp_avg_sq, max_exp_avg_sq and the activation tape for max_batch, after
 * cm_convrnn_finalize.  On an allocation failure cm_last_error reports the bytes requested so far. */
int cm_convrnn_train_init(cm_convrnn *m, float lr, float beta1, float beta2, float eps, float weight_decay);
/* Forward and loss only (the validation half): h_terms = rloss, vloss, loss_considering_density,
 * loss_not_considering_density.  d_past [B,4,H,W,P], d_target [B,4,H,W,F] device buffers; loss_eps = MACROPROPS.EPS. */
int cm_convrnn_loss(cm_convrnn *m, const float *d_past, const float *d_target, int32_t teacher_forcing, double loss_eps,
                    double h_terms[4], int32_t B, void *stream);
/* One training step on rloss + alpha * vloss: forward, loss, every gradient and, with apply_update != 0, the AMSGrad
 * update and the re-pack of the weights.  Nothing synchronises or allocates until the read-back of h_terms (may be NULL:
 * then the call only enqueues).  Without teacher forcing the fed-back frames carry gradient, as in the reference. */
int cm_convrnn_train_step(cm_convrnn *m, const float *d_past, const float *d_target, int32_t teacher_forcing, double loss_eps,
                          double alpha, double h_terms[4], int32_t B, int32_t apply_update, void *stream);
/* The AMSGrad update from the gradients the last step left (advances the optimizer step). */
int cm_convrnn_train_apply(cm_convrnn *m, void *stream);
int cm_convrnn_train_set_lr(cm_convrnn *m, float lr);
/* The raw frames [B,4,H,W,F] of the last training or loss forward (host buffer). */
int cm_convrnn_train_get_forecast(cm_convrnn *m, float *h_out, int64_t numel);
/* Gradient of a state_dict tensor, in its reference layout (host buffer). */
int cm_convrnn_train_get_grad(cm_convrnn *m, const char *name, float *h_data, int64_t numel);
/* which: 0 exp_avg, 1 exp_avg_sq, 2 max_exp_avg_sq, anything else is refused. */
int cm_convrnn_train_get_opt_state(cm_convrnn *m, const char *name, int32_t which, float *h_data, int64_t numel);
int cm_convrnn_train_set_opt_state(cm_convrnn *m, const char *name, int32_t which, const float *h_data, int64_t numel);
/* Reads the optimizer's step count into *step, after setting it from *step when set != 0 (a negative step is refused). */
int cm_convrnn_train_opt_step(cm_convrnn *m, int32_t *step, int32_t set);
/* Copies the master weights back to the state_dict (cm_convrnn_get_param) and re-packs every weight layout. */
int cm_convrnn_train_sync(cm_convrnn *m);

/* ---- The training step cut where the loss has its reduction over the whole batch (data-parallel training).  The loss
 * divides by counts over ALL samples of a step, so N ranks cannot each run cm_convrnn_train_step and average: each runs
 * cm_convrnn_train_forward, the six sums are added over the ranks, each runs cm_convrnn_train_backward with the totals, the
 * flat gradients (each rank's share of the global objective's gradient) are added over the ranks, and each runs
 * cm_convrnn_train_apply.  Fed its own sums, the pair equals cm_convrnn_train_step(apply_update = 0) bit for bit.
 * sums[0..4] = Poisson-KL sum, occupied MSE sum, occupied count, empty penalty sum, empty count; sums[5] = B*H*W*F. */
/* The forward with its activations kept, and the six sums of this call's samples after one synchronisation.  The target
 * frames are copied: neither device buffer is read after the call returns. */
int cm_convrnn_train_forward(cm_convrnn *m, const float *d_past, const float *d_target, int32_t teacher_forcing, int32_t B,
                             void *stream, double h_sums[6]);
/* h_terms (may be NULL: then the call only enqueues) = the four loss terms of the global sums; every gradient of
 * rloss + alpha * vloss with the global denominators, over this handle's samples; no update.  Refused unless a
 * cm_convrnn_train_forward on this handle came directly before: any other forward, step, loss or update in between, on
 * the training or the forecasting side, invalidates it.  The three counts must be numbers >= 0, with sums[5] >= this handle's own element count. */
int cm_convrnn_train_backward(cm_convrnn *m, const double h_global_sums[6], double loss_eps, double alpha, double h_terms[4],
                              void *stream);
/* The flat fp32 gradient buffer on the device, in state_dict order (the optimizer store's layout): what a data-parallel
 * run reduces in place before cm_convrnn_train_apply.  The coupled L2 term is not in it: the update adds it. */
int cm_convrnn_train_flat_grads(cm_convrnn *m, float **d_ptr, int64_t *numel);
/* The validation half: forward and the six sums, no tape kept for a backward. */
int cm_convrnn_loss_sums(cm_convrnn *m, const float *d_past, const float *d_target, int32_t teacher_forcing, int32_t B,
                         void *stream, double h_sums[6]);
/* Host only, no handle: the four loss terms of six (global) sums, by the expressions the device evaluates. */
int cm_convrnn_loss_terms_from_sums(const double sums[6], double eps, double terms[4]);

#ifdef __cplusplus
}
#endif
#endif /* CROWDMOD_HIP_H */
