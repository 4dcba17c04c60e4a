/*
 * soccerdiffusion_hip.h — C ABI of the MI355X (gfx950) denoiser hot path.
 *
 * Drop-in boundary for the diffusion-policy denoising path of bit-bots/SoccerDiffusion.
 * The reference is pure Python/PyTorch and has no FFI of its own; each entry point below
 * replaces the ATen work behind one reference method (file:line relative to the
 * reference checkout) and is what a ctypes binding on the reference side would call
 * (INTEGRATION.md shows that binding).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous row-major fp32 unless stated;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); no entry point
 *     allocates, frees or synchronises, so all of them can be captured into a hipGraph;
 *   - scratch memory comes from the caller: ask sd_workspace_floats() and pass a buffer of
 *     at least that many floats;
 *   - return value: 0 = ok, negative = invalid argument (SD_E_*), positive = hipError_t
 *     of the failing launch.  sd_last_error() returns a static description.
 *   - inputs are never modified unless the argument is documented as in/out.
 *
 * Numerics: data, accumulation and every elementwise operation are fp32.  Contractions run either on
 * v_mfma_f32_32x32x2_f32 (exact fp32 fma chain) or - the row GEMMs behind sd_op_linear*, and sd_ddim_sample
 * in mode 2 (sd_sampler_mode) - as three v_mfma_f32_32x32x16_f16 per product on operands split into fp16
 * hi + lo pairs (22 mantissa bits, fp32 accumulate): measured error against fp64 at or below the fp32 fma
 * chain's own.  LayerNorm eps = 1e-5 biased variance, GELU = exact erf form, softmax in
 * fp32.  Parity bar: <= 1e-4 relative L2 vs the fp32 CPU path (BASELINE.json); measured ~4e-7.
 */
#ifndef SOCCERDIFFUSION_HIP_H
#define SOCCERDIFFUSION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_ABI_VERSION 1

#define SD_E_BADARG (-1)   /* null pointer / non-positive size                       */
#define SD_E_BADDIM (-2)   /* hidden_dim not in {64,128,256,512} or not /heads        */
#define SD_E_TOOBIG (-3)   /* sequence longer than the kernels support               */
#define SD_E_UNSUPPORTED (-4) /* sd_sampler_prepare / sd_sampler_eps: this shape does not take the trajectory kernels */

/* One pre-norm transformer layer (torch nn.TransformerDecoderLayer / EncoderLayer with
 * norm_first=True, activation="gelu", dim_feedforward=d — reference
 * soccer_diffusion/ml/model/decoder.py:25-35, encoder/base.py:29-40).  Pointer names are
 * the checkpoint keys.  Encoder layers leave ca_* and n3_* NULL and
 * use n2_* as the FFN norm. */
typedef struct sd_layer_weights {
    const float *sa_in_w;   /* self_attn.in_proj_weight      (3d, d) */
    const float *sa_in_b;   /* self_attn.in_proj_bias        (3d)    */
    const float *sa_out_w;  /* self_attn.out_proj.weight     (d, d)  */
    const float *sa_out_b;  /* self_attn.out_proj.bias       (d)     */
    const float *ca_in_w;   /* multihead_attn.in_proj_weight (3d, d) */
    const float *ca_in_b;   /* multihead_attn.in_proj_bias   (3d)    */
    const float *ca_out_w;  /* multihead_attn.out_proj.weight (d, d) */
    const float *ca_out_b;  /* multihead_attn.out_proj.bias  (d)     */
    const float *lin1_w;    /* linear1.weight (d, d) */
    const float *lin1_b;    /* linear1.bias   (d)    */
    const float *lin2_w;    /* linear2.weight (d, d) */
    const float *lin2_b;    /* linear2.bias   (d)    */
    const float *n1_w, *n1_b;  /* norm1 */
    const float *n2_w, *n2_b;  /* norm2 */
    const float *n3_w, *n3_b;  /* norm3 (decoder only) */
} sd_layer_weights;

/* DiffusionActionGenerator parameters — reference soccer_diffusion/ml/model/decoder.py:23-36. */
typedef struct sd_denoiser_weights {
    int32_t d;       /* hidden_dim                     */
    int32_t J;       /* num_joints                     */
    int32_t L;       /* num_decoder_layers             */
    int32_t heads;   /* 4 (model.py:115)               */
    const float *emb_w;  /* embedding.weight (d, J)    */
    const float *emb_b;  /* embedding.bias   (d)       */
    const float *out_w;  /* fc_out.weight    (J, d)    */
    const float *out_b;  /* fc_out.bias      (J)       */
    const float *pe;     /* positional table (T_max, d): PositionalEncoding.pe, misc.py:43-56 */
    int32_t T_max;       /* rows of pe (= trajectory_prediction_length) */
    int32_t _pad;
    const sd_layer_weights *layers;  /* HOST array of L entries (device pointers inside) */
} sd_denoiser_weights;

/* BaseEncoder parameters — reference soccer_diffusion/ml/model/encoder/base.py:27-40. */
typedef struct sd_encoder_weights {
    int32_t d;       /* hidden_dim                                  */
    int32_t C;       /* input_dim                                   */
    int32_t p;       /* patch_size (Conv1d kernel = stride)         */
    int32_t L;       /* num_layers                                  */
    int32_t heads;   /* 4 (8 for the image sequence encoder)        */
    int32_t S_max;   /* rows of pe                                  */
    const float *emb_w;  /* embedding.weight (d, C, p)  Conv1d      */
    const float *emb_b;  /* embedding.bias   (d)                    */
    const float *pe;     /* positional table (S_max, d)             */
    const sd_layer_weights *layers;  /* HOST array of L entries     */
} sd_encoder_weights;

int sd_abi_version(void);
const char *sd_last_error(void);

/* Floats of caller-provided scratch for the calls below (upper bound over all of them)
 * for batch B, horizon T (decoder tokens or encoder patches), memory tokens M. */
size_t sd_workspace_floats(int B, int T, int M, int d, int L, int n_steps);

/* Which kernels a sampler call (sd_ddim_sample*, sd_sampler_prepare / sd_sampler_eps) runs: one route per call, chosen from the shape, the
 * cap and five A/B switches of the environment (soccerdiffusion_amd/csrc/sd_sampler_plan.h).  Results agree within fp32 rounding.
 *   route              mode  what runs
 *   CHAINS_F32          0    unfused row chains on the fp32 MFMA
 *   CHAINS_F16          0    unfused row chains on split fp16 (chain_f16_kernel)
 *   FUSED               0    fused decoder-layer kernel, the memory's K / V placed per step
 *   FUSED_FOLD          1    the same with the cross-attention's Q / out projections folded into the cached memory
 *   FUSED_FOLD_F16      2    decoder_layer_f16_kernel: mode 1 with every row GEMM and the self-attention as three fp16 MFMAs on hi + lo operands
 *   TRAJ_TUNED          3    traj_step_kernel<.., true>: ONE launch per step, a workgroup owns a trajectory; three fp16 products at every site
 *   TRAJ_TUNED_2P       4    traj_step_kernel<.., false>: two products at the Q | K | V site (~ 1.15 x; opt-in, see SD_STATUS_SHARP_LOGITS)
 *   TRAJ_TUNED_WIDE     3    traj_step_wide_kernel: 2 .. 4 key tiles in the folded cross-attention
 *   TRAJ_GENERIC        3    traj_step_generic_kernel<D, ..>: the memory's projected K / V streamed from HBM
 * When each applies (Mk = Mc + 1 memory rows; the first that holds, from the bottom of the table upwards):
 *   TRAJ_*: cap >= 3, 4 heads, J <= 32, L <= 8; off with SD_SAMPLER_TRAJ=0 or SD_SAMPLER_GEMM=f32.
 *   TRAJ_TUNED / _2P / _WIDE: hidden_dim 256, T <= 100, Mk <= 64 (SD_TRAJ_MAXROWS lowers that), B * Mk * 2 d < 2^30 floats of K / V.
 *     Mk <= 16: TRAJ_TUNED at cap 3, TRAJ_TUNED_2P at cap 4; Mk >= 17: TRAJ_TUNED_WIDE at either cap.
 *   TRAJ_GENERIC: every other hidden_dim 128 / 256 (T <= 100) / 512 (T <= 48: a longer panel does not fit the CU's LDS) shape; off with SD_SAMPLER_TRAJG=0.
 *   FUSED*: 4 heads, hidden_dim >= 128, (ceil(63 / T) + 1) * Mk <= 64 memory keys per 64-row panel, B * Mk * 2 d < 2^30.
 *   FUSED_FOLD: cap >= 1, Mk <= 16, T >= 64.  FUSED_FOLD_F16: cap >= 2, hidden_dim 256, J % 4 == 0; off with SD_SAMPLER_GEMM=f32.
 *   CHAINS_F16: cap >= 2, hidden_dim 128 / 256 / 512, J % 4 == 0, a memory the fused kernel does not take; off with SD_SAMPLER_GEMM=f32.
 *   CHAINS_F32: everything else.
 * sd_sampler_route: reporting only; max_mode as sd_ddim_sample_ex (-1 = 3), SD_E_BADARG outside -1 .. 4.
 * sd_sampler_mode: the mode of sd_sampler_route(d, heads, T, Mc, J, 1, 1, 3) - it sees neither the layer count nor the batch. */
#define SD_ROUTE_CHAINS_F32 0
#define SD_ROUTE_CHAINS_F16 1
#define SD_ROUTE_FUSED 2
#define SD_ROUTE_FUSED_FOLD 3
#define SD_ROUTE_FUSED_FOLD_F16 4
#define SD_ROUTE_TRAJ_TUNED 5
#define SD_ROUTE_TRAJ_TUNED_2P 6
#define SD_ROUTE_TRAJ_TUNED_WIDE 7
#define SD_ROUTE_TRAJ_GENERIC 8
int sd_sampler_route(int d, int heads, int T, int Mc, int J, int L, int B, int max_mode);
/* The rollout form of the TRAJ_TUNED / TRAJ_TUNED_2P routes.  FUSED: every DDIM step of a trajectory in one launch of
 * traj_step_rollout_kernel (a workgroup keeps its CU and its trajectory's folded planes stay in the Infinity Cache; at most 64 steps per
 * launch, longer rollouts in chunks) - sd_ddim_sample / _ex / _eps calls without trace and eps_trace.  PER_STEP: one launch per step - calls
 * that return something per step (trace, eps_trace), pinned calls, the loop form (sd_sampler_eps), every other route, and every call with
 * SD_TRAJ_ROLLOUT=steps in the environment.  Both forms compute the same bits.
 * Asked through sd_sampler_route with max_mode = SD_ASK_ROLLOUT + cap (0 .. 4) [+ SD_ASK_TRACE] [+ SD_ASK_PIN] [+ SD_ASK_LOOP]: the return is
 * SD_ROLLOUT_* of that kind of call instead of the route. */
#define SD_ASK_ROLLOUT 0x100
#define SD_ASK_TRACE 0x10
#define SD_ASK_PIN 0x20
#define SD_ASK_LOOP 0x40
#define SD_ROLLOUT_PER_STEP 0
#define SD_ROLLOUT_FUSED 1
int sd_sampler_mode(int d, int heads, int T, int Mc, int J);

/* StepToken.forward — soccer_diffusion/ml/model/misc.py:25-35.
 * steps: B values, int64 if steps_is_i64 else fp32.  freq: d/4 host-built frequencies
 * (built in fp32 exactly as misc.py:32 does).  token: learned (d/2).  Writes row b of the
 * step token to out + b*out_row_stride (d floats), so the caller can aim it at the last
 * row of each sample's memory block (model.py:176). */
int sd_step_token(const void *steps, int steps_is_i64, const float *freq, const float *token,
                  float *out, long out_row_stride, int B, int d, void *stream);

/* DiffusionActionGenerator.forward — soccer_diffusion/ml/model/decoder.py:38-54.
 * x (B,T,J), memory (B,M,d) [context tokens + step token], eps_out (B,T,J). */
int sd_denoiser_forward(const sd_denoiser_weights *w, const float *x, const float *memory,
                        float *eps_out, float *workspace, int B, int T, int M, void *stream);

/* BaseEncoder.forward — soccer_diffusion/ml/model/encoder/base.py:41-53.
 * x (B,S,C) -> out (B,S/p,d). */
int sd_encoder_forward(const sd_encoder_weights *w, const float *x, float *out,
                       float *workspace, int B, int S, void *stream);

/* GameStateEncoder.forward — soccer_diffusion/ml/model/encoder/game_state.py:19-27.
 * idx: B int64 indices; table (n_states,d); writes row b to out + b*out_row_stride. */
int sd_game_state_embed(const int64_t *idx, const float *table, float *out, long out_row_stride,
                        int B, int d, int n_states, void *stream);

/* DDIMScheduler.add_noise — call site soccer_diffusion/ml/training/train.py:218.
 * t: B int64 timesteps; acp: device table alphas_cumprod (n_train). rows = T*J per sample. */
int sd_ddim_add_noise(const float *x0, const float *noise, const int64_t *t, const float *acp,
                      float *out, int B, int per_sample, void *stream);

/* DDIMScheduler.step(...).prev_sample (eta = 0, epsilon prediction, no clipping) — call
 * site soccer_diffusion/ml/inference/plot.py:131.  In place on x is allowed.
 * sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, sqrt_1m_a_prev are the four fp32 scalars. */
int sd_ddim_step(const float *eps, const float *x, float *x_prev, float sqrt_a_t, float sqrt_1m_a_t,
                 float sqrt_a_prev, float sqrt_1m_a_prev, long n, void *stream);
/* One step of the second-order multistep solver (sd_ddim_sample_multistep) for a caller that evaluates the denoiser itself:
 *   x0 = (x - coef4[1] eps) / coef4[0];  x_prev = coef4[2] x0 + coef4[3] eps + w * (hist - x0);  hist = x0
 * coef4: the step's four fp32 scalars in HOST memory, in sd_ddim_step's order.  w == 0: hist is not read.  In place on x is allowed; hist
 * (n floats, device) must alias none of the others (SD_E_BADARG). */
int sd_multistep_step(const float *eps, const float *x, float *x_prev, float *hist, const float *coef4, float w, long n, void *stream);
/* One step of sd_ddim_sample_limits for a caller that evaluates the denoiser itself (element i belongs to joint i % J):
 *   x0 = (x - coef4[1] eps) / coef4[0];  x0c = x0 < lo[j] ? lo[j] : (x0 > hi[j] ? hi[j] : x0)       (compares: a NaN stays NaN)
 *   e' = reproject && x0c != x0 ? (x - coef4[0] x0c) / coef4[1] : eps;  x_prev = coef4[2] x0c + coef4[3] e' + w * (hist - x0c);  hist = x0c
 * hist NULL: first-order DDIM, nothing written (w must be 0).  lo, hi: 32 floats each in device memory (ops.joint_limits); coef4 in HOST
 * memory.  In place on x is allowed.  SD_E_BADARG (nothing launched): a NULL operand, J outside 1 .. 32, n % J != 0, w != 0 without hist,
 * hist aliasing eps, x or x_prev. */
int sd_ddim_limit_step(const float *eps, const float *x, float *x_prev, float *hist_or_null, const float *coef4, float w, const float *lo,
                       const float *hi, int reproject, long n, int J, void *stream);

/* One step of sd_ddim_sample_slew for a caller that evaluates the denoiser itself: sd_ddim_limit_step with the slew scan of that call over
 * the rows of every trajectory.  eps, x, x_prev, hist: whole (B, T, J) samples - the scan needs a trajectory's rows in order.  v: 32 floats,
 * start: (B, 32) floats or NULL, lo / hi: 32 floats each (all in device memory).  hold_x0 (B, T, J) and hold_mask (B, T): both or neither -
 * a held element enters the scan as hold_x0 and its x_prev is the scan's update of that value (the caller's hold overwrites it).  One
 * thread per (trajectory, joint).  SD_E_BADARG (nothing launched): a NULL operand, J outside 1 .. 32, w != 0 without hist, hist aliasing
 * eps, x or x_prev, one of hold_x0 / hold_mask without the other. */
int sd_ddim_slew_step(const float *eps, const float *x, float *x_prev, float *hist_or_null, const float *coef4, float w, const float *lo,
                      const float *hi, int reproject, const float *v, const float *start_or_null, const float *hold_x0, const int32_t *hold_mask,
                      int B, int T, int J, void *stream);

/* A distilled one-step decoder (one forward at the step token of t = 0, whose output is the clean trajectory: the reference's robot node,
 * soccer_diffusion/ml/inference/ros.py:293-298) under held elements, per-joint limits and slew limits, as sd_ddim_sample_slew defines
 * them for the predicted x0 of a rollout - whose last step "returns the clamped x0 itself"; a one-step model is that last step alone:
 *   raw = denoiser(ctx, step_token, x);  x0[t][j] = held(t, j) ? hold_x0[t][j] : raw[t][j];
 *   y = start[j] (NaN: none);  for t = 0 .. T-1:  z = x0 < fl(y - v[j]) ? fl(y - v[j]) : (x0 > fl(y + v[j]) ? fl(y + v[j]) : x0);
 *   z = z < lo[j] ? lo[j] : (z > hi[j] ? hi[j] : z);  out[t][j] = y = held(t, j) ? hold_x0[t][j] : z
 * (compares and selects: a NaN prediction stays NaN and limits nothing after it; -0 stays -0).  x (B, T, J) is only read; out (B, T, J)
 * receives the projection, raw_or_null (B, T, J) the unprojected prediction.  step_token: ONE row of d floats.  ctx: (B / draws, Mc, d),
 * prepared once per context as sd_ddim_sample_draws does.  lo, hi: 32 floats each (-inf / +inf: none), v_or_null: 32 floats (NULL: no slew
 * limit - no scan at all), start_or_null: (B, 32) floats; hold_x0 (B, T, J) and hold_mask (B, T): both or neither.  All in device memory.
 * The route is the one host-side plan's: on a trajectory route ONE launch of a direct twin of the step kernels, on any other the eps
 * launches and the projection kernel behind them.  max_mode as sd_ddim_sample_ex (4 is read as 3); status as sd_ddim_sample_slew
 * (SD_STATUS_NONFINITE from out).  workspace: sd_workspace_floats(B, T, max(Mc, 1), d, L, 1).  With no mask, infinite limits and no v,
 * out is raw bit for bit.  SD_E_BADARG (nothing launched): a NULL operand, J > 32, draws not dividing B, one of hold_x0 / hold_mask
 * without the other, out or raw aliasing each other, x or hold_x0. */
int sd_direct_sample(const sd_denoiser_weights *w, const float *ctx, const float *step_token, const float *x, float *out,
                     float *raw_or_null, float *workspace, int B, int T, int Mc, int32_t *status, int max_mode,
                     const float *hold_x0, const int32_t *hold_mask, int draws, const float *lo, const float *hi,
                     const float *v_or_null, const float *start_or_null, void *stream);

/* The projection of sd_direct_sample alone: out = project(raw; hold, limits, slew, start), one thread per (trajectory, joint).  raw, out:
 * (B, T, J), not aliased.  An infinite prediction comes out as its limit, -0 as -0.  SD_E_BADARG: a NULL operand, J outside 1 .. 32,
 * one of hold_x0 / hold_mask without the other, out aliasing raw or hold_x0. */
int sd_direct_project(const float *raw, float *out, const float *hold_x0, const int32_t *hold_mask, const float *lo, const float *hi,
                      const float *v_or_null, const float *start_or_null, int B, int T, int J, void *stream);

/* sd_ddim_slew_step with the acceleration scan of sd_ddim_sample_accel: a 32 floats, start2 (B, 32) floats or NULL (device memory); v must
 * be given and may be all +inf.  One thread per (trajectory, joint).  SD_E_BADARG as sd_ddim_slew_step, and for a NULL. */
int sd_ddim_accel_step(const float *eps, const float *x, float *x_prev, float *hist_or_null, const float *coef4, float w, const float *lo,
                       const float *hi, int reproject, const float *v, const float *start_or_null, const float *a, const float *start2_or_null,
                       const float *hold_x0, const int32_t *hold_mask, int B, int T, int J, void *stream);

/* Normalizer.normalize (inverse = 0: (x - mean) / std) and .denormalize (inverse = 1:
 * x * std + mean), per joint — soccer_diffusion/dataset/pytorch.py:410-414.  n = rows * J. */
int sd_normalize(const float *x, const float *mean, const float *stdv, float *out, long n, int J, int inverse,
                 void *stream);

/* The iterated sampler — reference loops soccer_diffusion/ml/inference/plot.py:122-131,
 * ml/training/distill.py:179-189, ml/inference/ros.py:301-310: for every t in timesteps:
 * eps = forward_with_context(ctx, x, t); x = scheduler.step(eps, t, x).prev_sample.
 *   ctx (B,Mc,d) context tokens WITHOUT the step token (may be NULL when Mc = 0);
 *   step_tokens (n_steps,d): row i = StepToken(timesteps[i]) (same for the whole batch);
 *   coef (HOST pointer, n_steps*4 floats): per step sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev);
 *   x (B,T,J) in/out: x_T on entry, the sample on return;
 *   trace (n_steps,B,T,J) or NULL: x after every step (parity tests).
 * Context keys/values are projected once per rollout and the n_steps step-token
 * keys/values once per call (memory is not layer-normed before the K/V projection). */
int sd_ddim_sample(const sd_denoiser_weights *w, const float *ctx, const float *step_tokens,
                   const float *coef, float *x, float *trace, float *workspace,
                   int B, int T, int Mc, int n_steps, void *stream);

/* sd_ddim_sample with a range guard and a kernel-selection cap (same loop, same reference call sites).
 *   status (DEVICE pointer to one int32, or NULL): zeroed at the start of the call; at its end a pass over the sample
 *     ORs SD_STATUS_NONFINITE into it when any value of x is inf / NaN.  The split-fp16 kernels of mode 2 use fixed
 *     power-of-two activation scales (8 for LayerNorm / attention / GELU outputs): a value with |8 v| >= 65520 becomes an
 *     fp16 infinity, its products NaN, and the NaN stays in its trajectory down to x - so a set bit means "operand
 *     range of mode 2 exceeded (e.g. a LayerNorm weight in the thousands) or non-finite input", never silently wrong
 *     finite numbers.  No synchronisation: read the word after the stream has drained.
 *   max_mode: 0 .. 4 = never use a mode above this one; -1 = automatic = sd_sampler_mode (at most 3: valid for any weights).
 *     max_mode = 4 opts in to mode 4 where the shape allows it and REQUIRES `status` (its SD_STATUS_SHARP_LOGITS bit);
 *     max_mode <= 1 also keeps the memory K/V projections on the exact-fp32 MFMA: the rerun path after SD_STATUS_NONFINITE
 *     (soccerdiffusion_amd.ops.ddim_sample_guarded does both reruns). */
#define SD_STATUS_NONFINITE 1
/* Mode 4 only: some self-attention logit q.k / sqrt(hd) exceeded SD_SHARP_LOGIT_LIMIT in magnitude.  The two-product Q | K | V
 * site of mode 4 (see sd_sampler_mode) is validated against the fp64 oracle up to that sharpness (tests/test_gpu_denoiser.py::
 * test_mode3_noise_prediction_*: <= 5e-5, half of north_star's 1e-4); beyond it the caller repeats the rollout with max_mode = 3
 * (three products everywhere), which soccerdiffusion_amd.ops.ddim_sample_guarded does - and remembers for that model.  The
 * result of a flagged call is finite; the bit says "not validated", not "wrong". */
#define SD_STATUS_SHARP_LOGITS 2
#define SD_SHARP_LOGIT_LIMIT 5.0f
int sd_ddim_sample_ex(const sd_denoiser_weights *w, const float *ctx, const float *step_tokens,
                      const float *coef, float *x, float *trace, float *workspace,
                      int B, int T, int Mc, int n_steps, int32_t *status, int max_mode, void *stream);

/* sd_ddim_sample_ex that also hands back the denoiser's noise prediction of every step - the reference's
 * `model.forward_with_context(...)` value inside the loop (soccer_diffusion/ml/inference/plot.py:128, ml/training/distill.py:186),
 * i.e. exactly what the DDIM update of that step consumed, from whichever kernels the call selected.
 *   eps_trace (n_steps,B,T,J) or NULL.  SURVEY 8(d)'s parity gate (i) "single eps-hat" for the sampler kernels: with n_steps = 1
 *   it is one forward of mode 3's trajectory kernel (sd_denoiser_forward runs the row-panel kernels instead). */
int sd_ddim_sample_eps(const sd_denoiser_weights *w, const float *ctx, const float *step_tokens,
                       const float *coef, float *x, float *trace, float *eps_trace, float *workspace,
                       int B, int T, int Mc, int n_steps, int32_t *status, int max_mode, void *stream);

/* sd_ddim_sample_eps with pinned leading rows (conditioning by inpainting: the first rows of the new trajectory are held to the rows of
 * the one the robot is still executing).  Row t of trajectory b is pinned iff t < pin_rows[b].
 *   pin_x0 (B,T,J): the known rows, in normalised space; only the pinned rows are read.  pin_noise (B,T,J): the rollout's start noise
 *   (what x holds on entry); it must not alias x.  pin_rows (B) int32 in device memory, 0 <= pin_rows[b] <= T: a batch may mix pinned
 *   and unpinned trajectories (pin_rows[b] = 0), and a captured graph needs no new arguments when the counts change.
 *   On entry:     pinned elements of x = c0[0] * pin_x0 + c1[0] * pin_noise           (coef[i] = (c0, c1, c2, c3) as for sd_ddim_sample)
 *   after step i: pinned elements of x = c2[i] * pin_x0 + c3[i] * pin_noise in place of the DDIM update; every other element gets the
 *                 update of sd_ddim_sample_eps unchanged.  eps_trace stays the network's prediction for all rows.
 * With the sampler's leading spacing c2[i] == c0[i+1] and c3[i] == c1[i+1]: at the entry of every step the pinned rows are the forward-
 * noised pin_x0 at that step's t - exactly a training-time add_noise sample, which the network reads through self-attention.  The last
 * step has c2 = 1, c3 = 0: the pinned rows of the returned sample equal pin_x0 bit for bit (finite noise).
 * Kernels: on the trajectory routes (SD_ROUTE_TRAJ_*) the lane that stores a step's DDIM update stores the pinned value instead, in the
 * same single launch (pinned instantiations of the step kernels); on the row-panel and chain routes one elementwise launch follows each
 * step's update (on SD_ROUTE_FUSED_FOLD_F16 every step's head is then a launch of its own: the head merged into the previous step's last
 * layer would read x before the pinned rows are rewritten).  The entry overwrite is one elementwise launch per rollout on every
 * route.  Mode 4's two-product kernels have no pinned twin: max_mode = 4 runs the mode-3 kernels (and needs no status word).
 * Everything else as sd_ddim_sample_eps.
 * SD_E_BADARG on a NULL pin pointer or pin_noise == x, before any launch. */
int sd_ddim_sample_pin(const sd_denoiser_weights *w, const float *ctx, const float *step_tokens, const float *coef, float *x, float *trace,
                       float *eps_trace, float *workspace, int B, int T, int Mc, int n_steps, int32_t *status, int max_mode,
                       const float *pin_x0, const float *pin_noise, const int32_t *pin_rows, void *stream);

/* Several draws per observation from one shared context: sd_ddim_sample_pin with `draws` trajectories per context.  ctx (B / draws, Mc, d);
 * trajectory b reads context b / draws (the draws of a context are contiguous); x, trace, eps_trace, the pin arrays and the status word
 * are per trajectory as ever.  pin_x0 = pin_noise = pin_rows = NULL: unpinned.
 *   On the trajectory routes (SD_ROUTE_TRAJ_*) the context is projected, folded and packed once per CONTEXT - the abs-max words and scales
 *   are taken over the B / draws contexts, and a maximum over duplicates is the same maximum, so the planes are bit for bit those of the
 *   call on the repeated context - and shared-context instantiations of the step kernels read them at b / draws (pinned and unpinned calls
 *   run the same kernel: a pinned call stays one launch per step; an unpinned one-key-tile rollout without traces is the fused rollout
 *   form).  The tuned kernels' size limit (sd_sampler_route_draws) counts contexts, not trajectories.  The result equals
 *   sd_ddim_sample_eps / _pin on the repeated context bit for bit.
 *   On the routes without trajectory kernels (modes 0 - 2, the rerun at max_mode 1 after SD_STATUS_NONFINITE included) one gather launch
 *   expands the context rows to B in the workspace and the kernels of old run on the copy: correct, but not shared.
 *   draws == 1 is the existing call, launch for launch; so is any valid draws with Mc = 0 (nothing to share).  workspace:
 *   sd_workspace_floats(B, ...) as for the other calls (the tail of the plane regions stays unused).
 * SD_E_BADARG (nothing launched): draws < 1, B % draws != 0, or only some of the pin pointers NULL. */
int sd_ddim_sample_draws(const sd_denoiser_weights *w, const float *ctx, const float *step_tokens, const float *coef, float *x, float *trace,
                         float *eps_trace, float *workspace, int B, int T, int Mc, int n_steps, int32_t *status, int max_mode,
                         const float *pin_x0, const float *pin_noise, const int32_t *pin_rows, int draws, void *stream);
/* sd_ddim_sample_draws with held ELEMENTS instead of pinned leading rows ("hold" is the element form, "pin" the leading-row form): joints
 * another module owns, keyframes, or both.  Element (b, t, j) is held iff bit j of hold_mask[b][t] is set.
 *   hold_mask (B,T) int32 in device memory: one word per (trajectory, row); J <= 32, bits >= J are never read.  hold_x0, hold_noise
 *   (B,T,J) as pin_x0, pin_noise; only held elements are read; hold_noise must not alias x.  A captured graph needs no new arguments
 *   when the mask changes.
 *   On entry:     held elements of x = c0[0] * hold_x0 + c1[0] * hold_noise
 *   after step i: held elements of x = c2[i] * hold_x0 + c3[i] * hold_noise in place of the DDIM update; every other element gets the
 *                 update unchanged; eps_trace stays the network's prediction for all elements.  The last step (1, 0) returns hold_x0 on
 *                 the held elements bit for bit.  A mask whose set rows are exactly the leading pin_rows[b] full rows is the pinned call.
 * Kernels: on the trajectory routes the hold instantiations of the step kernels (one per family and tile count; `draws` is a runtime
 * argument, so draws == 1 and draws > 1 run the same kernel) - the lane that stores the update of (token, 4 joints) loads the token's mask
 * word once, and reads hold_x0 / hold_noise only where one of its four bits is set; one launch per step (no fused rollout form, no mode-4
 * twin: max_mode = 4 runs the mode-3 kernels).  On the row-panel and chain routes one elementwise launch follows each step's update, as
 * for the pin (SD_ROUTE_FUSED_FOLD_F16: every step's head a launch of its own).  The entry overwrite is one elementwise launch per
 * rollout on every route.  The route is that of the pinned call of the same shape.
 * SD_E_BADARG (nothing launched): a NULL hold pointer, hold_noise == x, draws < 1, B % draws != 0, or J > 32. */
int sd_ddim_sample_hold(const sd_denoiser_weights *w, const float *ctx, const float *step_tokens, const float *coef, float *x, float *trace,
                        float *eps_trace, float *workspace, int B, int T, int Mc, int n_steps, int32_t *status, int max_mode,
                        const float *hold_x0, const float *hold_noise, const int32_t *hold_mask, int draws, void *stream);
/* sd_ddim_sample_hold with the second-order multistep solver (DPM-Solver++ 2M in its x0 form) in place of first-order DDIM: no extra
 * denoiser evaluation, one fused multiply-add per element.
 *   after step i: x0_i = (x - c1[i] eps) / c0[i];  x = c2[i] x0_i + c3[i] eps + msw[i] * (x0_{i-1} - x0_i);  history = x0_i
 *   msw (n_steps floats in HOST memory; ops.multistep_weights): msw[0] must be 0 - there is no history yet - and the step to a_prev = 1
 *   has msw = 0 as well.  All msw == 0 is the DDIM rollout.
 *   history (B,T,J) floats in device memory, the caller's (sd_workspace_floats is unchanged).  It is read only by steps with msw[i] != 0
 *   and written by every step, the last one included, so it needs no clearing: a replayed graph cannot see the rollout before, and a stale
 *   NaN in it is harmless.  On return it holds the x0 of the last step.
 *   hold_x0, hold_noise, hold_mask: all three (sd_ddim_sample_hold's meaning; J <= 32) or all NULL (nothing held, any J).  A held element
 *   gets the hold's value; its history entry is the model's x0 all the same.  Pinned leading rows are a mask.
 * Kernels: on the trajectory routes the multistep instantiations of the step kernels (one per family and tile count, the mask an optional
 * pointer and `draws` a runtime argument): the lane that stores the update of (token, 4 joints) requests its history values where the
 * hold requests its mask word, only when msw[i] != 0.  One launch per step: no fused rollout form and no mode-4 twin (max_mode = 4 runs
 * the mode-3 kernels).  On the row-panel and chain routes each step returns eps and one elementwise launch (sd_multistep_step's kernel)
 * updates x and the history; the hold's launch follows it.  The route is that of the pinned call of the same shape.
 * SD_E_BADARG (nothing launched): msw or history NULL, msw[0] != 0, a partial hold triple, history aliasing x or a hold buffer,
 * hold_noise == x, draws < 1, B % draws != 0, or a mask with J > 32. */
int sd_ddim_sample_multistep(const sd_denoiser_weights *w, const float *ctx, const float *step_tokens, const float *coef, float *x, float *trace,
                             float *eps_trace, float *workspace, int B, int T, int Mc, int n_steps, int32_t *status, int max_mode,
                             const float *hold_x0, const float *hold_noise, const int32_t *hold_mask, int draws, const float *msw,
                             float *history, void *stream);
/* sd_ddim_sample_multistep with per-joint limits on the predicted clean trajectory (diffusers' clip_sample / clip_sample_range, per joint),
 * inside the step launch.  All in normalised space; with (c0, c1, c2, c3) of step i, e the denoiser's prediction and w = msw[i] (0: DDIM):
 *   x0  = (x - c1 e) / c0                        (fma(-c1, e, x) / c0, the multistep form)
 *   x0c = x0 < lo[j] ? lo[j] : (x0 > hi[j] ? hi[j] : x0)
 *   e'  = e                                      reproject == 0 (diffusers' default, use_clipped_model_output=False)
 *       = (x0c == x0) ? e : (x - c0 x0c) / c1    reproject != 0
 *   x   = fma(c2, x0c, c3 e') + w (history - x0c);   history = x0c
 *   lo, hi: 32 floats each in device memory, lo[j] <= hi[j] for j < J, [J, 32) padded with -inf / +inf (ops.joint_limits); -inf / +inf: no
 *   limit on that side.  They are read on the device at every step, so a captured graph follows a rewrite in place.  J <= 32.
 *   The clamp is two compares and selects: a NaN x0 stays NaN (no fmin / fmax / med3, which would publish a limit for a non-finite
 *   prediction).  The last step (c2 = 1, c3 = 0) therefore leaves every free element bitwise inside [lo[j], hi[j]]; with all limits
 *   infinite every step is bitwise sd_ddim_sample_multistep's, with all msw == 0 besides bitwise the DDIM call's; with reproject an element
 *   that is not clamped takes e itself.  There is no count of clamped elements: a clamped element's x0 of the next steps sits within
 *   rounding of its limit, so two correct implementations would disagree on it - after the last step a clamped element equals its limit.
 *   msw, history: both (sd_ddim_sample_multistep's meaning; the history holds the clamped x0), or msw NULL: first-order DDIM, and history
 *   may be NULL too (given, it still receives the clamped x0 of every step).
 *   hold_x0, hold_noise, hold_mask: all three or all NULL.  A held element gets the hold's value whatever the limits say; its history entry
 *   is x0c as everything else's.  eps_trace stays the network's e for every element.
 * Kernels: on the trajectory routes the limits instantiations of the step kernels (sd_traj_lim.hip; traj_step_generic_lim_kernel), the
 * multistep twins plus the clamp in the lane that already holds x0: one launch per step, no fused rollout form, no mode-4 twin (max_mode = 4
 * runs the mode-3 kernels).  On the row-panel and chain routes each step returns eps and ddim_limit_step_kernel updates x (and the history);
 * the hold's launch follows it.  The route is that of the pinned call of the same shape.
 * SD_E_BADARG (nothing launched): lo or hi NULL, a partial hold triple, msw without history, msw[0] != 0, history
 * aliasing x or a hold buffer, hold_noise == x, draws < 1, B % draws != 0, J > 32. */
int sd_ddim_sample_limits(const sd_denoiser_weights *w, const float *ctx, const float *step_tokens, const float *coef, float *x, float *trace,
                          float *eps_trace, float *workspace, int B, int T, int Mc, int n_steps, int32_t *status, int max_mode,
                          const float *hold_x0, const float *hold_noise, const int32_t *hold_mask, int draws, const float *msw, float *history,
                          const float *lo, const float *hi, int reproject, void *stream);
/* sd_ddim_sample_limits with per-joint slew (velocity) limits beside the box: consecutive rows of the predicted clean trajectory differ by
 * at most v[j], at every step, before the update is formed.  With x0 of row t as in sd_ddim_sample_limits, per trajectory b and joint j:
 *   y = start[b][j]                                        (NaN, or start NULL: row 0 is free)
 *   for t = 0 .. T-1:
 *     a = y - v[j];  c = y + v[j]                          (fp32, one rounding each)
 *     z = x0[t] < a ? a : (x0[t] > c ? c : x0[t])          (compares: a NaN x0 stays NaN, a NaN y limits nothing)
 *     z = z < lo[j] ? lo[j] : (z > hi[j] ? hi[j] : z)      (the box last: it always wins)
 *     if bit j of hold_mask[b][t]: z = hold_x0[b][t][j]    (a held element is the scan's state as it stands)
 *     x0c[t] = z;  y = z
 *   e' = reproject && x0c != x0 ? (x - c0 x0c) / c1 : e;   x = fma(c2, x0c, c3 e') + w (history - x0c);   history = x0c
 * The row order is part of the definition.  v: 32 floats in device memory, v[j] >= 0, [J, 32) padded with +inf (ops.joint_slew); +inf: no
 * limit.  start: (B, 32) floats in device memory padded with NaN, one row per TRAJECTORY (a group of draws repeats its row), or NULL.
 * lo / hi must be given and may all be infinite.  Both arrays are read on the device at every step.
 * The last step therefore returns every free element bitwise inside [lo, hi] and, against a predecessor p inside the box that is not NaN,
 * inside [fl(p - v), fl(p + v)]; a jump INTO a held element is not limited.  All v infinite and no start: every step bitwise
 * sd_ddim_sample_limits'.
 * Kernels: on the trajectory routes the slew instantiations of the step kernels (sd_traj_slew.hip; traj_step_generic_slew_kernel), the
 * limits twins around the scan: the storing lanes exchange x0 through an fp32 plane in LDS behind two workgroup barriers and one lane per
 * joint walks the rows; one launch per step, no fused rollout form, no mode-4 twin (max_mode = 4 runs the mode-3 kernels).  On the
 * row-panel and chain routes each step returns eps and ddim_slew_step_kernel - one thread per (trajectory, joint), fetching its rows in
 * blocks ahead of the chain - updates x (and the history); the hold's launch follows it.
 * SD_E_BADARG: as sd_ddim_sample_limits, and for v NULL. */
int sd_ddim_sample_slew(const sd_denoiser_weights *w, const float *ctx, const float *step_tokens, const float *coef, float *x, float *trace,
                        float *eps_trace, float *workspace, int B, int T, int Mc, int n_steps, int32_t *status, int max_mode,
                        const float *hold_x0, const float *hold_noise, const int32_t *hold_mask, int draws, const float *msw, float *history,
                        const float *lo, const float *hi, int reproject, const float *v, const float *start_or_null, void *stream);
/* sd_ddim_sample_slew with per-joint acceleration limits beside the slew limits and the box: the second difference of consecutive rows of
 * the predicted clean trajectory is at most a[j], at every step, before the update is formed.  Per trajectory b and joint j the scan's
 * state is y1 (the row before; row -1: start[b][j]) and y2 (the row before that; row -2: start2[b][j]); NaN: no such row.
 *   for t = 0 .. T-1:
 *     d = y1 - y2;  p = y1 + d                             (fp32, one rounding each: the constant-velocity continuation)
 *     al = p - a[j];  ah = p + a[j]                        (one rounding each)
 *     z = x0[t] < al ? al : (x0[t] > ah ? ah : x0[t])      (compares: a NaN x0 stays NaN, a NaN p limits nothing)
 *     z = the slew interval around y1, then the box, then the hold, as sd_ddim_sample_slew applies them to z
 *     x0c[t] = z;  y2 = y1;  y1 = z
 * and the update is sd_ddim_sample_slew's on x0c.  Priority: box, then slew, then acceleration.  The row order is part of the definition.
 * a: 32 floats in device memory, a[j] >= 0, [J, 32) padded with +inf; +inf: no limit.  start2: (B, 32) floats in device memory padded with
 * NaN, one row per TRAJECTORY, or NULL.  lo / hi and v must be given and may all be infinite.  There is no braking ahead of the box: where
 * the box or the slew interval wins, the second difference at that row can exceed a; without a box or a slew limit the velocity can
 * accumulate and the scan can run away from the prediction.  All a infinite and no start2: every step bitwise sd_ddim_sample_slew's.
 * Kernels: on the trajectory routes the acceleration instantiations of the step kernels (sd_traj_acc.hip; traj_step_generic_accel_kernel),
 * the slew twins with two rows of state in the scan; one launch per step, no fused rollout form, no mode-4 twin (max_mode = 4 runs the
 * mode-3 kernels).  On the row-panel and chain routes each step returns eps and ddim_accel_step_kernel updates x (and the history).
 * SD_E_BADARG: as sd_ddim_sample_slew, and for a NULL. */
int sd_ddim_sample_accel(const sd_denoiser_weights *w, const float *ctx, const float *step_tokens, const float *coef, float *x, float *trace,
                         float *eps_trace, float *workspace, int B, int T, int Mc, int n_steps, int32_t *status, int max_mode,
                         const float *hold_x0, const float *hold_noise, const int32_t *hold_mask, int draws, const float *msw, float *history,
                         const float *lo, const float *hi, int reproject, const float *v, const float *start_or_null, const float *a,
                         const float *start2_or_null, void *stream);
/* The projection of a one-step decoder's output under acceleration limits: sd_direct_project with the scan above (direct_project_accel_kernel).
 * A one-step call under acceleration limits is two launches: sd_direct_sample with nothing set, which returns raw, then this.  v NULL: no
 * slew limit. */
int sd_direct_project_accel(const float *raw, float *out, const float *hold_x0, const int32_t *hold_mask, const float *lo, const float *hi,
                            const float *v_or_null, const float *start_or_null, const float *a, const float *start2_or_null, int B, int T, int J,
                            void *stream);
/* sd_direct_sample under acceleration limits in one call: the plain direct launch (no hold, no scan), which returns the unprojected
 * prediction in raw - it must be given - then sd_direct_project_accel from raw to out.  Arguments as sd_direct_sample's, plus a and
 * start2.  The status word tells of out.  SD_E_BADARG as sd_direct_sample, and for raw or a NULL. */
int sd_direct_sample_accel(const sd_denoiser_weights *w, const float *ctx, const float *step_token, const float *x, float *out, float *raw,
                           float *workspace, int B, int T, int Mc, int32_t *status, int max_mode, const float *hold_x0,
                           const int32_t *hold_mask, int draws, const float *lo, const float *hi, const float *v_or_null,
                           const float *start_or_null, const float *a, const float *start2_or_null, void *stream);
/* sd_sampler_route (plain route numbers only) of a sd_ddim_sample_draws call of B trajectories. */
int sd_sampler_route_draws(int d, int heads, int T, int Mc, int J, int L, int B, int max_mode, int draws);

/* The representative of each context's draws: index[c] = argmin_i sum_k |x[c,i] - x[c,k]|^2 over the G draws of context c (x (C, G, T, J), the
 * space the sampler works in), and, with out (C, T, J) != NULL, out[c] = x[c, index[c]].  One workgroup per context, fp32 in fixed orders
 * (a pair's distance is computed once, so d(i,k) == d(k,i); the score sums k = 0 .. G-1 in that order, the zero self term included; ties go
 * to the lowest index, so bitwise-equal draws tie exactly); no atomics: the result does not depend on scheduling.  1 <= G <= 64. */
int sd_select_medoid(const float *x, int32_t *index, float *out /* or NULL */, int C, int G, int T, int J, void *stream);

/* The draw that continues the previous plan (the backward-coherence criterion of Bidirectional Decoding, Liu et al. 2024): ticks that
 * overlap by R = T - shift rows describe the same instants twice, and among the G draws of context c the one closest to what the last
 * committed plan said about them is chosen.  Per context c, fp32 in fixed orders, the sampler's normalised space:
 *   x (C, G, T, J), a context's draws contiguous;  prev (Cp, T, J): context c reads prev[robots ? robots[c] : c] (robots[c] in [0, Cp) is
 *   the caller's to guarantee: the device checks nothing), a NaN element: no plan there;  w (T) row weights >= 0 in device memory, only
 *   w[0 .. R-1] are read;  0 <= shift < T;  lam >= 0.
 *   d = x[c,g,tau,j] - prev[.,tau+shift,j];  term = w[tau] * (d * d), SELECTED to 0.f (not multiplied by zero) where prev is NaN or
 *   w[tau] == 0;  coh[g] = sum of term over tau < R and j, in sd_select_medoid's order: lane l of a wave adds elements l, l + 64, ... of
 *   the R * J overlap elements in that order, then the xor butterfly 32 .. 1; one wave per draw.
 *   med[g] = sd_select_medoid's score of draw g, same order of operations, computed only where it is needed.
 *   Context c HAS A PLAN iff an overlap element has w[tau] > 0 and a prev that is not NaN.  With a plan cost[g] = coh[g] + lam * med[g]
 *   (the product rounds on its own; coh[g] itself when lam == 0: G distance sums instead of G (G - 1) / 2); without one cost[g] = med[g]
 *   and index[c] is sd_select_medoid's bit for bit.
 *   index[c] = the lowest g among the smallest costs (compare <, from draw 0).  out (C, T, J) != NULL: out[c] = x[c, index[c]];
 *   cost (C, G) != NULL: the costs.
 * One workgroup per context, no atomics: the result does not depend on C, on the grid or on which rows of prev other contexts read.
 * SD_E_BADARG before any launch: x, prev, w or index NULL; C, T, J < 1, G outside [1, 64], shift outside [0, T); lam < 0, NaN or
 * infinite; out or cost overlapping x or prev (prev's extent is taken as C plans, one where robots is given). */
int sd_select_coherent(const float *x, const float *prev, const int32_t *robots /* or NULL */, const float *w, int32_t *index,
                       float *out /* or NULL */, float *cost /* or NULL */, int C, int G, int T, int J, int shift, float lam, void *stream);

/* The denoiser evaluated ONE step at a time on the trajectory kernels of sampler modes 3 / 4 - the reference's own loop form,
 *   for t in scheduler.timesteps: eps = model.forward_with_context(ctx, x, t); x = scheduler.step(eps, t, x).prev_sample
 * (soccer_diffusion/ml/inference/plot.py:122-131, ml/training/distill.py:179-189, ml/inference/ros.py:301-310), whose
 * forward_with_context (ml/model/model.py:159-179) cannot know that it is inside a loop: what does not depend on x or the step is
 * prepared once into the caller's workspace and reused by every evaluation.
 *   sd_sampler_prepare: `what` = SD_PREPARE_WEIGHTS (abs-max + split fp16 planes of every matrix: once per weight update) |
 *     SD_PREPARE_CONTEXT (K / V of the context rows, folded with Wq / Woc as sd_ddim_sample does: once per context).
 *   sd_sampler_eps: eps (B,T,J) = denoiser(x, [ctx rows | step token]); step_tokens (n_tok,d) with n_tok = 1 (one step for the
 *     whole batch) or n_tok = B (row b = sample b's StepToken); x is only read.  status / max_mode as sd_ddim_sample_ex (3 or -1:
 *     three products everywhere, no status needed; 4: the guarded two-product Q | K | V site).
 * Both calls must see the same (w, workspace, B, T, Mc, n_tok, max_mode); workspace = sd_workspace_floats(B, T, max(Mc, 1), d, L,
 * n_tok) floats, owned by the caller and left alone between the calls.  Return SD_E_UNSUPPORTED (nothing launched) where the shape
 * does not take the trajectory kernels (sd_sampler_route names no TRAJ route): the caller then uses sd_denoiser_forward. */
#define SD_PREPARE_WEIGHTS 1
#define SD_PREPARE_CONTEXT 2
int sd_sampler_prepare(const sd_denoiser_weights *w, const float *ctx, float *workspace, int B, int T, int Mc, int n_tok,
                       int what, int max_mode, void *stream);
int sd_sampler_eps(const sd_denoiser_weights *w, const float *step_tokens, const float *x, float *eps, float *workspace,
                   int B, int T, int Mc, int n_tok, int32_t *status, int max_mode, void *stream);
/* The loop form with a group size: the two calls above with ctx (B / draws, Mc, d), trajectory b reads context b / draws (the draws of a
 * context are contiguous).  The context is projected, folded and packed once per CONTEXT, exactly as sd_ddim_sample_draws does it, and the
 * shared-context instantiations of the step kernels read it; the tuned kernels' size limit counts contexts.  n_tok is 1 or B as before; with
 * n_tok = B trajectory b reads its own step token and only the distinct tokens are folded - the denoiser at K timesteps of the same window
 * is B = C K trajectories, draws = K, reading C folded contexts.  eps equals sd_sampler_eps on the repeated context bit for bit.
 * workspace: sd_workspace_floats(B, ...) (the tail of the plane regions stays unused).  draws == 1 or Mc == 0: the calls above, launch for
 * launch (they are the draws = 1 case of these).  SD_E_BADARG (nothing launched): draws < 1 or B % draws != 0.  SD_E_UNSUPPORTED as above:
 * the caller expands the context rows and uses the existing path. */
int sd_sampler_prepare_draws(const sd_denoiser_weights *w, const float *ctx, float *workspace, int B, int T, int Mc, int n_tok,
                             int what, int max_mode, int draws, void *stream);
int sd_sampler_eps_draws(const sd_denoiser_weights *w, const float *step_tokens, const float *x, float *eps, float *workspace,
                         int B, int T, int Mc, int n_tok, int32_t *status, int max_mode, int draws, void *stream);

/* out[n][j] = max over t of |r[t + 1] - r[t]|, r = x std + mean (fp32, two roundings): the largest step between consecutive rows of
 * trajectory n at joint j, in the space of the denormalised trajectories.  x (N, T, J), out (N, J); one thread per (n, j).  T == 1: 0. */
int sd_eval_max_step(const float *x, const float *mean, const float *stdv, float *out, long N, int T, int J, void *stream);
/* out[n][j] = max over t of |(r[t + 1] - r[t]) - (r[t] - r[t - 1])|, r as above (fp32, one rounding per operation, in that order): the largest
 * second difference of trajectory n at joint j - the number an acceleration limit is chosen from.  One thread per (n, j); two runs agree
 * bit for bit.  T <= 2: 0. */
int sd_max_accel(const float *x, const float *mean, const float *stdv, float *out, long N, int T, int J, void *stream);
/* ---- held-out evaluation (csrc/sd_eval.hip; soccerdiffusion_amd/evaluation.py) --------------------------------------------
 * Both kernels: fp32, contraction off, no atomics, every sum in a fixed order that depends on the shape alone (written out at the top of
 * sd_eval.hip), so two runs agree bit for bit.
 *   sd_eval_sqerr_rows: out[r] = (1 / per) sum_i (a[r,i] - b[r,i])^2 for `rows` rows of `per` floats - with per = T J the loss of one
 *     trajectory.  One workgroup per row.
 *   sd_eval_trajectory_errors: x (C, G, T, J) samples in the sampler's normalised space, target (C, T, J) the recorded joint commands as the
 *     data source delivers them (radians in [0, 2 pi)).  Per element y = x std + mean (one rounding per operation, as sd_session_commit),
 *     d = y - target and, with angular != 0, d -= 2 pi rintf(d / (2 pi)): the angles are stored modulo 2 pi, so an error of 2 pi - 0.01 is
 *     an error of 0.01.  err (C, G) = mean of d^2 over T J; row_err (C, G, T) or NULL = mean over J; joint_err (C, G, J) or NULL = mean over
 *     T; best (C) or NULL = argmin over g of err, ties to the lowest index.  One workgroup per context.  1 <= G <= 64, J <= 32, T >= 1.
 * SD_E_BADARG (nothing launched) outside those limits or with a required pointer NULL. */
int sd_eval_sqerr_rows(const float *a, const float *b, float *out, long rows, long per, void *stream);
int sd_eval_trajectory_errors(const float *x, const float *target, const float *mean, const float *stdv, float *err, float *row_err /* or NULL */,
                              float *joint_err /* or NULL */, int32_t *best /* or NULL */, int C, int G, int T, int J, int angular,
                              void *stream);

/* ---- image path: ResNet basic-block convolution -------------------------------------------------------
 * y = act(BatchNorm_eval(conv3x3(x, w; stride 1, padding 1)) [+ res]) - torchvision BasicBlock's conv1/bn1/relu and
 * conv2/bn2 (+ identity) / relu as the reference configures them (soccer_diffusion/ml/model/encoder/image.py:55-83), inference mode.
 * Tensors are NHWC fp32: x (N,H,W,Cin), res / y (N,H,W,Cout); Cin, Cout multiples of 64; x, y, res, bn_scale and bn_shift 16-byte aligned
 * (SD_E_BADARG otherwise: the kernels use 16-byte accesses).  bn_scale = gamma / sqrt(var + eps),
 * bn_shift = beta - mean * bn_scale (per output channel).  Implicit GEMM with three fp16 MFMAs per product on hi + lo operands,
 * fp32 accumulate (fp32-grade results; soccerdiffusion_amd/csrc/sd_conv.hip).
 *   sd_conv3x3_pack: w (Cout,Cin,3,3) fp32 -> sd_conv3x3_packed_halfs(Cout,Cin) fp16 values in fragment order + the power-of-two
 *     scale they carry (device float) - once per weight update; amax_word: one uint32 of device scratch.
 *   x_amax / y_amax: device words holding the bits of max|x| / receiving max|y| (atomic max: zero y_amax before the call; NULL =
 *     not needed).  sd_absmax_word computes such a word for a tensor no convolution produced (x 16-byte aligned). */
size_t sd_conv3x3_packed_halfs(int Cout, int Cin);
int sd_conv3x3_pack(const float *w, int Cout, int Cin, void *planes, float *scale, uint32_t *amax_word, void *stream);
int sd_conv3x3_bn_act(const float *x, const void *w_planes, const float *w_scale, const uint32_t *x_amax, const float *bn_scale,
                      const float *bn_shift, const float *res, float *y, uint32_t *y_amax, int N, int H, int W, int Cin, int Cout,
                      int relu, void *stream);
int sd_absmax_word(const float *x, int64_t n, uint32_t *word, void *stream);
/* The same launch for a 1 x 1 stride-1 convolution (torchvision Bottleneck's conv1 / conv3 and the stride-1 shortcut of ResNet-50's
 * layer 1, reference option image_encoder_type "resnet50": soccer_diffusion/ml/model/encoder/image.py:62-66): weights (Cout,Cin,1,1)
 * packed by sd_conv_pack(ksize = 1); same tensors, epilogue (BatchNorm, residual, ReLU) and conventions as sd_conv3x3_bn_act. */
int sd_conv1x1_bn_act(const float *x, const void *w_planes, const float *w_scale, const uint32_t *x_amax, const float *bn_scale,
                      const float *bn_shift, const float *res, float *y, uint32_t *y_amax, int N, int H, int W, int Cin, int Cout,
                      int relu, void *stream);
/* The striding convolutions of a ResNet stage entry (conv1 of layers 2 - 4 and their 1 x 1 shortcut): y = act(BatchNorm_eval(conv(x, w; kernel
 * ksize = 3 with padding 1, or ksize = 1 with padding 0; stride 2))), NHWC fp32, x (N,H,W,Cin) -> y (N,ceil(H/2),ceil(W/2),Cout); Cin a
 * multiple of 64, Cout of 128; weights (Cout,Cin,ksize,ksize) packed by sd_conv_pack (sd_conv_packed_halfs fp16 values).  Same arithmetic,
 * scale and abs-max conventions as sd_conv3x3_bn_act. */
size_t sd_conv_packed_halfs(int Cout, int Cin, int ksize);
int sd_conv_pack(const float *w, int Cout, int Cin, int ksize, void *planes, float *scale, uint32_t *amax_word, void *stream);
int sd_conv_s2_bn_act(const float *x, const void *w_planes, const float *w_scale, const uint32_t *x_amax, const float *bn_scale,
                      const float *bn_shift, float *y, uint32_t *y_amax, int N, int H, int W, int Cin, int Cout, int ksize, int relu,
                      void *stream);
/* The ResNet stem in one launch: y = maxpool3x3/s2/p1(relu(BatchNorm_eval(conv7x7/s2/p3(x, w)))) - torchvision ResNet.conv1 / bn1 / relu /
 * maxpool as the reference instantiates them (soccer_diffusion/ml/model/encoder/image.py:55-83).  x (N,3,H,W) fp32 NCHW frames (the
 * reference's own layout) -> y (N,Hp,Wp,64) fp32 NHWC with Hc = (H-1)/2+1, Hp = (Hc-1)/2+1 (likewise W); w (64,3,7,7) packed by
 * sd_stem_pack (sd_stem_packed_halfs fp16 values).  Same arithmetic, scale and abs-max conventions as sd_conv3x3_bn_act. */
size_t sd_stem_packed_halfs(void);
int sd_stem_pack(const float *w, void *planes, float *scale, uint32_t *amax_word, void *stream);
int sd_stem_conv_bn_relu_pool(const float *x, const void *w_planes, const float *w_scale, const uint32_t *x_amax, const float *bn_scale,
                              const float *bn_shift, float *y, uint32_t *y_amax, int N, int H, int W, void *stream);

/* ---- single-op entry points (unit parity tests and host-side composition) ---------- */

/* out[R,N] = act(LN?(A)[R,d] @ W[N,d]^T + bias) (+ res).  ln_w/ln_b NULL = no LayerNorm;
 * act: 0 none, 1 gelu(erf); res NULL or [R,N] (may alias out).  N % d == 0. */
int sd_op_linear(const float *A, const float *W, const float *bias, const float *ln_w,
                 const float *ln_b, const float *res, float *out, int R, int N, int d, int act,
                 void *stream);

/* Multi-head attention core, unmasked: out[b,i,h*hd:(h+1)*hd] = softmax(q k^T / sqrt(hd)) v.
 * q rows (B*Tq) with row stride ldq; k, v rows (B*S) with row stride ldkv; optional extra
 * key/value row shared by the whole batch (k_extra/v_extra, d floats each, NULL = none).
 * A packed self-attention buffer (k = q + d, v = q + 2d, ldq = ldkv = 3d, Tq = S <= 128, head dim 64,
 * no extra row) runs on the split-fp16 MFMA kernel of the sampler (22-bit operands, fp32 accumulate). */
int sd_op_attention(const float *q, int ldq, const float *k, const float *v, int ldkv,
                    const float *k_extra, const float *v_extra, float *out, int ldo,
                    int B, int Tq, int S, int d, int heads, void *stream);

/* Host-only, reporting: the kernel the attention core launches for a call that does not take the split-fp16 kernel above -
 * 1 = attention_pipe_kernel (a workgroup per sample walking its heads: Tq <= 128, no extra row, no dropout, B >= 64),
 * 0 = attention_kernel (a workgroup per (sample, head)).  has_extra: an extra key/value row is passed; dropout: p > 0.
 * The function the launch itself asks.  SD_E_BADARG on an empty shape. */
int sd_attention_route(int B, int Tq, int S, int has_extra, int dropout);

/* out (B,S/p,d) = Conv1d(k=s=p)(x (B,S,C)) + bias + pe[:S/p]; p = 1 is nn.Linear + PE.  Any C*p: up to 319 the patches and a column
 * chunk of W^T are staged whole in LDS, beyond that (the image tokens of a hidden_dim-512 model) 128 values of k at a time. */
int sd_op_patch_embed(const float *x, const float *w, const float *b, const float *pe,
                      float *out, int B, int S, int C, int p, int d, void *stream);

/* eps[R,J] = h[R,d] @ W[J,d]^T + b.  If x_io != NULL also applies the DDIM update to it in
 * place using coef[4] (see sd_ddim_step).  eps may be NULL when x_io is given. */
int sd_op_fc_out(const float *h, const float *W, const float *b, float *eps, float *x_io,
                 const float *coef4_host, int R, int d, int J, void *stream);

/* ---- training: backward of the blocks, loss, optimizer -------------------------------
 * One training step of the reference (soccer_diffusion/ml/training/train.py:204-240:
 * add_noise, forward, F.mse_loss, backward, AdamW.step) at dropout p = 0 is composed from
 * these entry points by soccerdiffusion_amd/training.py (autograd nodes per block). */

/* sd_op_linear with a row stride on A (lda >= d, multiple of 4): lets dX = dY[:, slice] W^T-slices
 * accumulate through `res` without copying the slice. */
int sd_op_linear_strided(const float *A, int lda, const float *W, const float *bias, const float *ln_w,
                         const float *ln_b, const float *res, float *out, int R, int N, int d, int act,
                         void *stream);

/* sd_op_attention that also writes lse2[b, head, q] = log2-sum-exp of the scaled scores
 * (log2 domain), which the backward uses to recompute the probabilities. */
int sd_op_attention_lse(const float *q, int ldq, const float *k, const float *v, int ldkv, float *out,
                        int ldo, float *lse2, int B, int Tq, int S, int d, int heads, void *stream);

/* dq, dk, dv of softmax(q k^T / sqrt(hd)) v given dO.  dk/dv rows are fully overwritten. */
int sd_op_attention_bwd(const float *q, int ldq, const float *k, const float *v, int ldkv, const float *o,
                        int ldo, const float *dO, int lddo, const float *lse2, float *dq, int lddq, float *dk,
                        float *dv, int lddkv, int B, int Tq, int S, int d, int heads, void *stream);

/* ---- dropout (training) -----------------------------------------------------------------------------------------
 * The reference trains with torch's default dropout p = 0.1 (soccer_diffusion/ml/model/decoder.py:26-33 and
 * encoder/base.py:29-40 never set it; train.py never calls .eval()): on the attention probabilities
 * (nn.MultiheadAttention), after each attention out-projection (dropout1 / dropout2), after the GELU and after linear2
 * (dropout / dropout3).  ONE counter-based mask for every kernel, nothing stored: element (row, col) of the logical
 * (rows x width) tensor of site `site` is kept iff word (col & 3) of Philox4x32-7(counter = {quad lo, quad hi, site lo,
 * site hi}, key = seed) >= p * 2^32, quad = (row * ceil4(width) + col) >> 2; kept values are scaled by 1 / (1 - p).
 * The backward entry points regenerate the mask from the same (p, seed, site).  p = 0 is the parity path. */

/* out = x o mask (forward of a stand-alone site; backward of a fused one: dy o mask).  out may alias x. */
int sd_op_dropout(const float *x, float *out, long rows, int width, float p, uint64_t seed, uint64_t site, void *stream);
/* mask[rows, width] = 0 or 1 / (1 - p): what the kernels apply (tests hand it to the oracle). */
int sd_op_dropout_mask(float *mask, long rows, int width, float p, uint64_t seed, uint64_t site, void *stream);
/* out = gelu(pre) o mask;  dpre = dy o mask o gelu'(pre)   (FFN: linear2(dropout(gelu(linear1 x)))) */
int sd_op_gelu_dropout_fwd(const float *pre, float *out, long rows, int width, float p, uint64_t seed, uint64_t site, void *stream);
int sd_op_gelu_dropout_bwd(const float *dy, const float *pre, float *dpre, long rows, int width, float p, uint64_t seed,
                           uint64_t site, void *stream);
/* out[R,N] = res + dropout(A[R,d] W[N,d]^T + bias), mask rows = R, width = N (x + dropout1(sa_block(x)) etc.);
 * A may have a row stride lda >= d (0 = d).  res is required and may alias out. */
int sd_op_linear_dropout(const float *A, int lda, const float *W, const float *bias, const float *res, float *out, int R,
                         int N, int d, float p, uint64_t seed, uint64_t site, void *stream);
/* Training GEMMs on pre-split weights.  sd_pack_weight_blocks splits n_blocks d x d fp32 blocks (block b = d rows of d
 * floats at src + src_off_dev[b]; offsets in a DEVICE int64 array) into the fp16 hi | lo fragment planes the kernels read
 * (2 d^2 halfs per block, consecutive in dst; scale 2^8: |w| < 256) in ONE launch - once per optimizer step for every weight
 * and, with transposed != 0 (planes of the block's TRANSPOSE), for the B operands of the dX GEMMs.  sd_op_linear_packed is sd_op_linear_strided / sd_op_linear_dropout with `wpk` =
 * the planes of the N / d consecutive blocks of W instead of W itself (LayerNorm or residual [+ dropout], no activation). */
int sd_pack_weight_blocks(const float *src, const int64_t *src_off_dev, int n_blocks, void *dst, int d, int transposed, void *stream);
int sd_op_linear_packed(const float *A, int lda, const void *wpk, const float *bias, const float *ln_w, const float *ln_b,
                        const float *res, float *out, int R, int N, int d, float p, uint64_t seed, uint64_t site, void *stream);

/* ---- Fused row chains of one transformer layer for TRAINING (reference: the nn.TransformerDecoderLayer / EncoderLayer
 * blocks built by soccer_diffusion/ml/model/decoder.py:26-33 and encoder/base.py:29-40, norm_first = True, as autograd runs
 * them in ml/training/train.py:204-240).  One 64-row panel per workgroup goes through every row-local operation between
 * two attention cores in ONE launch; the forward writes exactly the tensors the backward and the weight-gradient GEMMs read.
 * All weights are split planes (sd_pack_weight_blocks); all row tensors are [R, d] fp32, contiguous, unless noted.
 * d in {64, 128, 256}; p = 0 turns every mask off; mask rows = R, width = d (sites as in sd_op_linear_dropout /
 * sd_op_gelu_dropout_fwd).  Stages with a NULL first pointer are skipped.
 *
 * sd_train_fwd_chain:
 *   [a]    h1 = h_in + dropout_{site_out}(a Wo^T + bo)                 -> h_out            (a == NULL: h1 = h_in)
 *   [w1]   n = LN(h1; ln_w, ln_b) -> n_out;  pre = n W1^T + b1 -> pre;  u = dropout_{site_act}(gelu(pre)) -> u
 *          h2 = h1 + dropout_{site_ffn}(u W2^T + b2)                   -> h2_out           (w1 == NULL: h2 = h1)
 *   [wn]   nn = LN(h2; nln_w, nln_b) -> nn_out;  y = nn Wn^T + bn      -> y_out [R, n_next d]   (n_next = 0: stop)
 * sd_train_bwd_chain (dY [R, passes d] with row stride ldy; wt = planes of the `passes` TRANSPOSED blocks):
 *   g = dropout_{site_in}(dy) -> dym (p > 0, passes == 1, not for the x-without-pre form);   t = g Wt   (dX of a linear layer)
 *   [pre]  t = t o gelu'(pre) o mask_{site_act} -> dpre;  t = t Wt1                    (back through FFN1)
 *   [x]    dx = LayerNorm-backward(t; x, ln_w) + dres -> dx;  dg += sum_rows t o xhat;  db += sum_rows t   (fp32 atomics)
 *          (x == NULL: dx = t) */
#define SD_AMAX_WORDS 64
typedef struct sd_train_fwd_chain_args {
    int64_t R;
    int32_t d, n_next;
    const float *a; const void *wo; const float *bo; const float *h_in; float *h_out;
    const float *ln_w, *ln_b; float *n_out; const void *w1; const float *b1; float *pre; float *u;
    const void *w2; const float *b2; float *h2_out;
    const float *nln_w, *nln_b; float *nn_out; const void *wn; const float *bn; float *y_out;
    float p;
    uint64_t seed, site_out, site_act, site_ffn;
    /* optional: bits of max |x| over a, n_out, u, nn_out are atomically max-ed into these arrays of SD_AMAX_WORDS words
     * (zero them first; a workgroup uses word blockIdx % SD_AMAX_WORDS) - the per-tensor scales of sd_gemm_tn_grouped, a
     * by-product of the row passes */
    uint32_t *amax_a, *amax_n, *amax_u, *amax_nn;
    uint32_t *amax_h2;   /* optional: max |h2_out| (the input of fc_out after the last layer) */
} sd_train_fwd_chain_args;
typedef struct sd_train_bwd_chain_args {
    int64_t R;
    int32_t d, passes, ldy;
    const float *dy; float *dym; const void *wt;
    const float *pre; float *dpre; const void *wt1;
    const float *x; const float *ln_w; const float *dres; float *dg; float *db;
    float *dx;
    float p;
    uint64_t seed, site_in, site_act;
    uint32_t *amax_dy, *amax_dpre;   /* optional, as above: max |.| of the (masked) dy over all passes, and of dpre */
    uint32_t *amax_dx;               /* optional: max |dx| of the LayerNorm-backward form (the embedding's dY under layer 0) */
} sd_train_bwd_chain_args;
int sd_train_fwd_chain(const sd_train_fwd_chain_args *args, void *stream);
int sd_train_bwd_chain(const sd_train_bwd_chain_args *args, void *stream);

/* The forward of ONE decoder layer for training with a workgroup per trajectory (soccerdiffusion_amd/csrc/sd_train_traj.hip): the self-attention
 * core, [h1 = h + drop(a_sa Wo^T + bo); n2 = LN2(h1); q = n2 Wq^T + bq], the cross-attention core over the M projected memory rows,
 * [h2 = h1 + drop(a_ca Woc^T + boc); nf = LN3(h2); pre = nf W1^T + b1; u = drop(gelu(pre)); h3 = h2 + drop(u W2^T + b2)] and - when w_n
 * is given - the next layer's [nn1 = LN1'(h3); qkv2 = nn1 Wn^T + bn] in one launch, i.e. sd_op_attention_lse_dropout x 2 +
 * sd_train_fwd_chain x 2 of the same layer (reference: nn.TransformerDecoderLayer, norm_first, as built by
 * soccer_diffusion/ml/model/decoder.py:26-33; training loop ml/training/train.py:204-240).  It stores the same tensors in the same layouts
 * (rows [B*T, 256]; qkv / qkv2 [B*T, 768]; lse [B, 4, T] as sd_op_attention_lse; kv [B, M, 512] = the memory's K | V projection) and the
 * same abs-max words, with dropout masks at the same (site, row, column) indices, so sd_train_bwd_chain / sd_op_attention_bwd_dropout /
 * sd_gemm_tn_grouped consume them unchanged.  hidden_dim 256, 4 heads, T <= 100, M <= 16 (sd_train_layer_fwd_ok).  Weights: planes from
 * sd_pack_weight_traj (sd_pack_weight_traj_halfs(N, K) fp16 values; K = 256 - or <= 32 for the embedding -, N = 256, or 768 for w_n),
 * repacked after every optimizer step. */
typedef struct sd_train_layer_fwd_args {
    int32_t B, T, M, d, heads;
    const float *h, *qkv;
    float *a_sa, *lse_sa, *h1, *n2, *q;
    const float *kv;
    float *a_ca, *lse_ca, *h2, *nf, *pre, *u, *h3, *nn1, *qkv2;
    const void *w_o, *w_q, *w_oc, *w_1, *w_2, *w_n;
    const float *b_o, *b_q, *b_oc, *b_1, *b_2, *b_n;
    const float *n2_w, *n2_b, *n3_w, *n3_b, *nn_w, *nn_b;
    float p;
    uint64_t seed, site_sa_probs, site_sa_out, site_ca_probs, site_ca_out, site_act, site_ffn;
    uint32_t *amax_a_sa, *amax_n2, *amax_a_ca, *amax_nf, *amax_u, *amax_nn, *amax_out;   /* SD_AMAX_WORDS words each, or NULL */
} sd_train_layer_fwd_args;
int sd_train_layer_fwd_ok(int d, int heads, int T, int M);
int sd_train_layer_fwd(const sd_train_layer_fwd_args *args, void *stream);
/* The entry of the decoder stack in the same geometry: h0 = x Wemb^T + b + pe[:T] (nn.Linear(J -> 256) + PositionalEncoding,
 * soccer_diffusion/ml/model/decoder.py:48-50), n1 = LN1(h0) of layer 0, qkv = n1 Wqkv^T + b: sd_op_patch_embed (p = 1) + the head launch of
 * sd_train_fwd_chain in one.  x (B,T,J), J a multiple of 4 up to 32; w_emb / w_qkv: planes from sd_pack_weight_traj ((256, J) and (768, 256)). */
int sd_train_head_fwd(const float *x, const void *w_emb, const float *b_emb, const float *pe, float *h0, const float *ln_w, const float *ln_b,
                      float *n1, const void *w_qkv, const float *b_qkv, float *qkv, uint32_t *amax_n1, int B, int T, int J, void *stream);
size_t sd_pack_weight_traj_halfs(int N, int K);
int sd_pack_weight_traj(const float *w, int N, int K, void *planes, void *stream);
/* n matrices in one launch: matrix i = rows[i] x 256 floats at base + src_offsets[i] (floats; rows multiples of 16) -> planes +
 * dst_offsets[i] (halfs); the three arrays are DEVICE arrays, max_rows = the largest rows[i]. */
int sd_pack_weight_traj_multi(const float *base, const int64_t *src_offsets, const int32_t *rows, const int64_t *dst_offsets, int n,
                              int max_rows, void *planes, void *stream);

/* Several weight gradients dW += dY^T X (and db += column sums of dY, db may be NULL) in one launch, on the fp16 matrix
 * pipe with ONE power-of-two scale per operand tensor: amax_dy / amax_x point at SD_AMAX_WORDS device words whose maximum is
 * the bits of (an upper bound of) max |dY| / max |X| - what sd_train_*_chain leave behind.  dY [R, N] and X [R, K] with row strides ldy / ldx
 * (multiples of 4, 16-byte aligned), N and K multiples of 4 (tiles of 128 x 128, ragged ones masked); dW [N, K] with row
 * stride ldw.  Accumulates with fp32 atomics.  sd_op_absmax fills the words of an operand no chain produced (zero them first). */
typedef struct sd_gemm_tn_problem {
    const float *dY; const float *X; float *dW; float *db;
    const uint32_t *amax_dy; const uint32_t *amax_x;
    int64_t R;
    int32_t N, K, ldy, ldx, ldw;
} sd_gemm_tn_problem;
int sd_gemm_tn_grouped(const sd_gemm_tn_problem *problems, int n_problems, void *stream);
/* Host-only: the slabs-per-workgroup sd_gemm_tn_grouped would choose for cnt (<= 64) problems of R[i] rows and N[i] x K[i]
 * outputs, and the workgroups that makes (*total_wgs, may exceed one chip-full for very large groups).  No launch; -1 on bad
 * arguments.  (CPU unit test of the partitioning arithmetic.) */
long sd_gemm_tn_grouped_plan(const long *R, const long *N, const long *K, int cnt, long *total_wgs);
int sd_op_absmax(const float *x, int64_t rows, int width, int ld, uint32_t *amax, void *stream);

/* sd_op_attention_lse / sd_op_attention_bwd with dropout on the probabilities: O = (softmax(S) o mask) V, the softmax
 * normaliser and lse2 are those of the un-dropped probabilities; mask rows = (b * heads + h) * Tq + q, width = S. */
int sd_op_attention_lse_dropout(const float *q, int ldq, const float *k, const float *v, int ldkv, float *out,
                                int ldo, float *lse2, int B, int Tq, int S, int d, int heads, float p, uint64_t seed,
                                uint64_t site, void *stream);
int sd_op_attention_bwd_dropout(const float *q, int ldq, const float *k, const float *v, int ldkv, const float *o,
                                int ldo, const float *dO, int lddo, const float *lse2, float *dq, int lddq, float *dk,
                                float *dv, int lddkv, int B, int Tq, int S, int d, int heads, float p, uint64_t seed,
                                uint64_t site, void *stream);

/* Cross-attention of C * K trajectories over C shared contexts (training with several noise draws per window): trajectory b's keys are the
 * Mc rows of context b / K followed by its own token row at key index Mc - the order of cat(context, token).  q, out (C*K, T, d);
 * kv_ctx (C, Mc, 2d) and kv_tok (C*K, 1, 2d): packed K | V rows; lse2 (C*K, heads, T) as sd_op_attention_lse.  Dropout on the
 * probabilities uses sd_op_attention_lse_dropout's mask index for (b, head, t, key) with S = Mc + 1: the call equals that one on the
 * expanded K | V under the same (p, seed, site).  The backward returns dq, dkv_tok and dkv_ctx (C, Mc, 2d), the sum over the K draws of a
 * context and their T rows: one workgroup per (context, head) adds them in draw order without atomics, so two runs give the same bits.
 * Head dims 16, 32, 64; 1 <= T <= 100; Mc >= 1; any K (sd_train_xattn_shared_ok); anything else: SD_E_UNSUPPORTED, nothing launched. */
int sd_train_xattn_shared_ok(int d, int heads, int T, int Mc);
int sd_train_xattn_shared_fwd(const float *q, const float *kv_ctx, const float *kv_tok, float *out, float *lse2, int C, int K,
                              int T, int Mc, int d, int heads, float p, uint64_t seed, uint64_t site, void *stream);
int sd_train_xattn_shared_bwd(const float *q, const float *kv_ctx, const float *kv_tok, const float *o, const float *dO,
                              const float *lse2, float *dq, float *dkv_ctx, float *dkv_tok, int C, int K, int T, int Mc, int d,
                              int heads, float p, uint64_t seed, uint64_t site, void *stream);
/* out[b] = in[b / K] for C * K rows of `row` floats (a multiple of 4, 16-byte aligned), and its backward din[c] = sum over the K rows
 * of a group of dout, added in draw order (deterministic): where the shared kernels do not apply the context is expanded. */
int sd_train_expand_rows(const float *in, float *out, long C, int K, long row, void *stream);
int sd_train_expand_rows_bwd(const float *dout, float *din, long C, int K, long row, void *stream);

/* dW[N,K] += dY[R,N]^T X[R,K];  db[N] += column sums of dY (db may be NULL).  Accumulates
 * with fp32 atomics: zero dW/db first (summation order is not fixed). */
int sd_op_gemm_tn(const float *dY, int ldy, const float *X, int ldx, float *dW, int ldw, float *db, long R,
                  int N, int K, void *stream);

/* y = LayerNorm(x) * g + b (eps 1e-5, biased variance); mean/rstd (R) may be NULL. */
int sd_op_layernorm_fwd(const float *x, const float *g, const float *b, float *y, float *mean, float *rstd,
                        long R, int d, void *stream);
/* dx = LN backward of dy (+ dres if not NULL; dx may alias dres); dg/db accumulate (atomics). */
int sd_op_layernorm_bwd(const float *dy, const float *x, const float *mean, const float *rstd, const float *g,
                        const float *dres, float *dx, float *dg, float *db, long R, int d, void *stream);

int sd_op_gelu_fwd(const float *pre, float *out, long n, void *stream);
int sd_op_gelu_bwd(const float *dy, const float *pre, float *dpre, long n, void *stream);

/* out[c] += sum over rows of src[r*row_stride + c], c < width. */
int sd_op_colsum(const float *src, long row_stride, long rows, int width, float *out, void *stream);
/* out[R,N] = A[R,K] B[K,N] for K <= 64 (input gradient of fc_out). */
int sd_op_small_k_matmul(const float *A, const float *Bm, float *out, long R, int K, int N, void *stream);

/* F.mse_loss(pred, target) -> loss[0]; grad (may be NULL) = 2 (pred - target) / n.
 * scratch256d: 256 doubles of device scratch.  Deterministic. (train.py:229) */
int sd_mse_loss(const float *pred, const float *target, float *loss, float *grad, void *scratch256d, long n,
                void *stream);

/* torch.optim.AdamW update on flat buffers (train.py:162,239), `step` = 1-based step count. */
int sd_adamw_step(float *p, const float *g, float *m, float *v, long n, double lr, double beta1, double beta2,
                  double eps, double weight_decay, long step, void *stream);

/* The same update with its seven scalars in DEVICE memory (hyper7[0..6] = 1 - lr*wd, 1 - beta1, beta2, 1 - beta2,
 * lr / (1 - beta1^step), sqrt(1 - beta2^step), eps; sd_adamw_hyper fills a HOST array with them): kernel arguments are
 * frozen in a captured hipGraph, the learning rate (OneCycleLR), beta1 and the bias corrections change every step. */
int sd_adamw_step_dev(float *p, const float *g, float *m, float *v, long n, const float *hyper7_dev, void *stream);
int sd_adamw_hyper(double lr, double beta1, double beta2, double eps, double weight_decay, long step, float *hyper7_host);

/* sd_adamw_step / sd_adamw_step_dev plus an exponential moving average of the weights in the SAME launch: p, m, v come out bit
 * for bit as from those two, then ema[i] += ema_weight * (p_new[i] - ema[i]) on the value just computed (one more read and one
 * more write per element, no pass of its own).  ema_weight in [0, 1] is the weight of THIS update (1 - decay after warmup; the
 * caller owns the schedule); the _dev form reads it from *ema_weight_dev - a pointer of its own, since the graphed step keeps
 * the dropout epoch in the word behind hyper7.  16-byte loads and stores where all five buffers are 16-byte aligned, element by
 * element otherwise; any n >= 1. */
int sd_adamw_ema_step(float *p, const float *g, float *m, float *v, float *ema, long n, double lr, double beta1, double beta2,
                      double eps, double weight_decay, long step, double ema_weight, void *stream);
int sd_adamw_ema_step_dev(float *p, const float *g, float *m, float *v, float *ema, long n, const float *hyper7_dev,
                          const float *ema_weight_dev, void *stream);

/* Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, norm type 2) and the non-finite guard, on device memory so that a
 * captured hipGraph replays them.  sd_grad_norm, two launches:
 *   s = sum g[i]^2 in fp64 (the product of two fp32 values is exact there), in one fixed order that depends on n alone - not on
 *       the device, the grid or g's alignment: deterministic, and 1e20 or 1e-25 gradients neither overflow nor vanish;
 *   clip2[0] = norm = (float)sqrt(s);  clip2[1] = coef = min(1, max_norm / (norm + 1e-6f)) in fp32, or 0 where norm is not finite -
 *       then the int32 *skipped goes up by one (plain store: the caller zeroes it once).
 * partials_ws: sd_grad_norm_workspace_doubles() doubles of device scratch.  max_norm >= 0; +inf = norm and guard only (coef = 1).
 * sd_adamw_clip_step / _dev: sd_adamw_step / sd_adamw_ema_step (ema != NULL; ema_weight[_dev] is read only then) and their _dev
 * forms on g[i] * coef (one fp32 rounding; g itself is not written), bit for bit what those write for a gradient buffer that holds
 * the products - so coef = 1 is their step exactly.  Where clip2[0] is not finite nothing is read or written: p, m, v, ema keep
 * their bits.  SD_E_BADARG, nothing launched: a NULL operand, n <= 0, max_norm negative or NaN. */
int sd_grad_norm_workspace_doubles(void);
int sd_grad_norm(const float *g, long n, void *partials_ws, float *clip2, int *skipped, float max_norm, void *stream);
int sd_adamw_clip_step(float *p, const float *g, float *m, float *v, float *ema, long n, double lr, double beta1, double beta2,
                       double eps, double weight_decay, long step, double ema_weight, const float *clip2, void *stream);
int sd_adamw_clip_step_dev(float *p, const float *g, float *m, float *v, float *ema, long n, const float *hyper7_dev,
                           const float *ema_weight_dev, const float *clip2, void *stream);

/* Per-step part of the dropout mask key from DEVICE memory: when set (non-NULL), every dropout kernel adds *device_word to
 * the high half of its Philox key at run time, so a hipGraph replay of a training step draws fresh masks once the host has
 * changed the word.  Process-wide; NULL switches it off. */
int sd_set_dropout_epoch(const uint32_t *device_word);

/* ---- image path, TRAINING: torchvision BasicBlock / Bottleneck under autograd with BatchNorm2d in training mode, as the
 * reference trains its backbone with every step (soccer_diffusion/ml/training/train.py:226-240 -> ml/model/encoder/image.py:38-83).  NHWC fp32
 * tensors of npix = N * H * W pixels x C channels (C in {64, 128, 256, 512, 1024, 2048}), 16-byte aligned (soccerdiffusion_amd/csrc/sd_conv_train.hip).
 *   sd_bn_train_fwd: batch statistics of y (the raw convolution output) -> mean, rstd = 1 / sqrt(biased var + eps) (C floats each);
 *     z = relu?((y - mean) rstd gamma + beta (+ res)); running_mean / running_var updated as torch.nn.BatchNorm2d does (momentum, unbiased
 *     variance) unless NULL; z_amax (one uint32, zeroed by the caller) receives the bits of max |z| for the next convolution's fp16 scale.
 *     acc: 2 C doubles (the channel sums, an output); scratch: sd_bn_scratch_floats(npix, C) floats - the workgroups' partial sums (plain
 *     stores, added up in double by a second launch: no atomics, deterministic).
 *   sd_bn_train_bwd: g = dz behind the ReLU mask (z > 0; z NULL with relu = 1 and NO residual operand: the mask is recomputed from y, gamma, beta -
 *     one tensor less to read; beta may be NULL otherwise); dgamma = sum g x_hat, dbeta = sum g,
 *     dy = gamma rstd (g - mean(g) - x_hat mean(g x_hat)); dres (or NULL) receives g, the gradient of the residual operand; dy_amax as above.
 *   sd_conv_wgrad: dw (Cout, Cin, k, k) (torch layout, ZEROED by the caller) += sum over output pixels of dy[pixel][co] x[pixel * stride + tap - k/2][ci]
 *     for the k x k (1 or 3), stride 1 or 2, padding k / 2 convolution of x (N,H,W,Cin) with output dy (N,Ho,Wo,Cout); Cin, Cout multiples
 *     of 64.  Split-fp16 MFMAs, fp32 atomics.  dy_amax / x_amax: the tensors' abs-max words (as sd_bn_train_bwd / sd_bn_train_fwd leave them)
 *     -> one power-of-two scale per operand for the launch; either NULL -> block floating point per 32 pixels (abs-max taken inside).
 * The data gradient is the forward convolution (sd_conv3x3_bn_act / sd_conv1x1_bn_act, identity epilogue) of dy - dilated with zeros for a
 * stride-2 convolution - with the flipped, transposed weights. */
size_t sd_bn_scratch_floats(int64_t npix, int C);
int sd_bn_train_fwd(const float *y, const float *gamma, const float *beta, const float *res, float *z, float *mean, float *rstd,
                    float *running_mean, float *running_var, double *acc, float *scratch, uint32_t *z_amax, int64_t npix, int C, float eps,
                    float momentum, int relu, void *stream);
int sd_bn_train_bwd(const float *dz, const float *z, const float *y, const float *mean, const float *rstd, const float *gamma, const float *beta,
                    float *dy,
                    float *dres, float *dgamma, float *dbeta, double *acc, float *scratch, uint32_t *dy_amax, int64_t npix, int C, int relu,
                    void *stream);
/* Data gradient of a 3 x 3 / stride-2 / padding-1 convolution (conv1 of ResNet layers 2 - 4): dx (N, H, W, Cout) = the transposed convolution of
 * dy (N, (H + 1) / 2, (W + 1) / 2, Cin) with w_planes = sd_conv3x3_pack of the FLIPPED, TRANSPOSED weights (Cout = the forward's input channels) -
 * what sd_conv3x3_bn_act computes on dy dilated with zeros, without the zeros: one launch per parity class of the output pixels, each with
 * its 1 / 2 / 2 / 4 live taps (csrc/sd_conv.hip: convt3x3_s2_kernel).  Epilogue as sd_conv3x3_bn_act without ReLU: dx = acc * bn_scale + bn_shift (+ res). */
int sd_convt3x3_s2(const float *dy, const void *w_planes, const float *w_scale, const uint32_t *dy_amax, const float *bn_scale, const float *bn_shift,
                   const float *res, float *dx, uint32_t *dx_amax, int N, int H, int W, int Cin, int Cout, void *stream);
/* ... and of the 1 x 1 / stride-2 shortcut (w_planes = sd_conv_pack(ksize 1) of the transposed weights): dx[2 i][2 j] = dy[i][j] . w; the other
 * three quarters of dx are NOT written - the caller zeroes dx first. */
int sd_convt1x1_s2(const float *dy, const void *w_planes, const float *w_scale, const uint32_t *dy_amax, const float *bn_scale, const float *bn_shift,
                   float *dx, int N, int H, int W, int Cin, int Cout, void *stream);
/* The stem's BatchNorm (batch statistics) + ReLU + max-pool 3 x 3 / stride 2 / padding 1 (torchvision ResNet.forward: maxpool(relu(bn1(conv1 x)))) fused:
 * y (N, Hc, Wc, C) -> p (N, Hp, Wp, C), Hp = (Hc - 1) / 2 + 1, and idx (N, Hp, Wp, C / 4 words: one byte per element = the winner's position 0 .. 8
 * in its window, first maximum in scan order as ATen's kernel, 9 = no positive value); z = relu(BN(y)) is never materialised.  The backward gathers
 * the pool's gradient from dp and idx (no dz tensor) inside the two BatchNorm-backward launches: dy, dgamma, dbeta as sd_bn_train_bwd.
 * acc / scratch / the abs-max words as sd_bn_train_fwd (scratch: sd_bn_scratch_floats(N * Hc * Wc, C)). */
int sd_bn_relu_pool_fwd(const float *y, const float *gamma, const float *beta, float *p, uint32_t *idx, float *mean, float *rstd, float *running_mean,
                        float *running_var, double *acc, float *scratch, uint32_t *p_amax, int N, int Hc, int Wc, int C, float eps, float momentum,
                        void *stream);
int sd_bn_relu_pool_bwd(const float *dp, const uint32_t *idx, const float *y, const float *mean, const float *rstd, const float *gamma, float *dy,
                        float *dgamma, float *dbeta, double *acc, float *scratch, uint32_t *dy_amax, int N, int Hc, int Wc, int C, void *stream);
/* BatchNorm on FROZEN statistics inside a training backbone (bn.eval(): fine-tuning on the running statistics, which are never written).
 *   sd_bn_frozen_fold: rstd = 1 / sqrt(running_var + eps), s = gamma rstd, t = beta - running_mean s (C floats each, formed in double); runs on
 *     the device with every forward, so a captured training step folds what the optimizer last wrote.
 *   sd_bn_frozen_fwd: z = relu?(y s + t (+ res)) and the abs-max word of z - the forward of a unit whose affine pair is TRAINED (y is kept for
 *     dgamma).  Where the pair needs no gradient the forward is the inference launch (sd_conv3x3_bn_act / sd_conv_s2_bn_act with s, t) and y
 *     is never written.
 *   sd_bn_frozen_bwd: g = dz behind the ReLU mask, dres (or NULL) = g, dy = g s, dy_amax = the bits of max |dy|.  dgamma NULL (with dbeta, y, t,
 *     running_mean, rstd, acc, scratch unused): ONE element-wise launch, the mask is z > 0.  Otherwise dbeta = sum g, dgamma = sum g (y -
 *     running_mean) rstd from the same single pass over the tensors (partial sums in scratch, added up in double in a fixed order into acc: no
 *     atomics, two runs agree bit for bit); z NULL with relu and no residual operand: the mask is recomputed from y, s, t.
 *   sd_bn_frozen_relu_pool_fwd / _bwd: the stem, max_pool(relu(y s + t), 3, 2, 1) with the window scan, tie rule and index bytes of
 *     sd_bn_relu_pool_fwd; the backward in one pass (dy = g s; dgamma / dbeta as above, or both NULL); scratch: sd_bn_scratch_floats(N Hc Wc, C). */
int sd_bn_frozen_fold(const float *gamma, const float *beta, const float *running_mean, const float *running_var, float eps, int C, float *s, float *t,
                      float *rstd, void *stream);
int sd_bn_frozen_fwd(const float *y, const float *s, const float *t, const float *res, float *z, uint32_t *z_amax, int64_t npix, int C, int relu,
                     void *stream);
int sd_bn_frozen_bwd(const float *dz, const float *z, const float *y, const float *s, const float *t, const float *running_mean, const float *rstd,
                     float *dy, float *dres, float *dgamma, float *dbeta, double *acc, float *scratch, uint32_t *dy_amax, int64_t npix, int C, int relu,
                     void *stream);
int sd_bn_frozen_relu_pool_fwd(const float *y, const float *s, const float *t, float *p, uint32_t *idx, uint32_t *p_amax, int N, int Hc, int Wc, int C,
                               void *stream);
int sd_bn_frozen_relu_pool_bwd(const float *dp, const uint32_t *idx, const float *y, const float *s, const float *running_mean, const float *rstd,
                               float *dy, float *dgamma, float *dbeta, double *acc, float *scratch, uint32_t *dy_amax, int N, int Hc, int Wc, int C,
                               void *stream);
/* The stem in training: sd_stem_conv_raw = the bare 7 x 7 / stride-2 / padding-3 convolution of sd_stem_conv_bn_relu_pool (same packed planes,
 * same kernel) -> y_raw (N, Hc, Wc, 64) NHWC, Hc = (H - 1) / 2 + 1; sd_stem_wgrad: its weight gradient dw (64, 3, 7, 7) from dy (N, Hc, Wc, 64)
 * and the frames x (N, 3, H, W), both with their abs-max words; scratch: sd_stem_wgrad_scratch_floats(N, H, W) floats.  (The frames need no gradient.) */
int sd_stem_conv_raw(const float *x, const void *w_planes, const float *w_scale, const uint32_t *x_amax, float *y_raw, int N, int H, int W,
                     void *stream);
size_t sd_stem_wgrad_scratch_floats(int N, int H, int W);
int sd_stem_wgrad(const float *dy, const float *x, const uint32_t *dy_amax, const uint32_t *x_amax, float *dw, float *scratch, int N, int H, int W,
                  void *stream);
/* scratch (sd_conv_wgrad_scratch_floats floats, or NULL): the 3 x 3 kernel (LDS-staged column strips, all taps of a staging; stride 2: one launch
 * per row / column parity class of x) stores one partial tile per workgroup there and a second launch adds them up (no atomics: hundreds of
 * workgroups adding to the same Cout x Cin x 9 floats are bound by the L2's atomic rate; deterministic).  Without scratch (or abs-max words), and for
 * 1 x 1 convolutions, the per-wave kernel with atomics runs. */
size_t sd_conv_wgrad_scratch_floats(int N, int H, int W, int Cin, int Cout, int ksize, int stride);
int sd_conv_wgrad(const float *dy, const float *x, const uint32_t *dy_amax, const uint32_t *x_amax, float *dw, float *scratch, int N, int H, int W,
                  int Cin, int Cout, int ksize, int stride, void *stream);

/* ---- Swin-T / Swin-S image encoder, inference (reference option image_encoder_type "swin_transformer_tiny" / "swin_transformer_small":
 * soccer_diffusion/ml/model/encoder/image.py:11-20, 86-100; torchvision.models.swin_transformer V1 as restated in
 * soccerdiffusion_amd/ml/model/encoder/image.py, _ShiftedWindowAttention / _SwinBlock / _PatchMerging / _SwinTransformer).  Tokens are NHWC fp32
 * rows (N * H * W, C).  Products on split fp16 operands (three v_mfma_f32_16x16x32_f16, fp32 accumulation; csrc/sd_swin.hip), LayerNorm /
 * erf-GELU / softmax in fp32.
 *   sd_token_pack: W (N, K) fp32 (nn.Linear.weight), K a multiple of 32 -> sd_token_packed_halfs(N, K) fp16 values in fragment order and
 *     w_inv (sd_token_pad_cols(N) floats): the inverse power-of-two scale of each weight row.  Once per weight update.
 *   sd_token_linear: out (R, N) = epi(pro(A) W^T + bias); A (R, K) 16-byte aligned, any R.  pro: LayerNorm over K with ln_w / ln_b (both NULL:
 *     none; K <= 1536 with it); epi: erf-GELU if gelu, then + res (R, N) (NULL: none; res may equal out: the residual add in place).
 *   sd_token_merge_linear: the same GEMM (no bias, no epilogue) on torchvision PatchMerging's A operand, gathered in the load: x (Nimg, H, W, C)
 *     -> rows of cat(x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2]) (zero padding for an odd H or W), K = 4 C <= 1536, LayerNorm
 *     over K -> out (Nimg, ceil(H/2), ceil(W/2), N).
 *   sd_swin_window_plan: plan6 = (pH, pW, sh, sw, nWy, nWx) of _ShiftedWindowAttention.forward: the map padded to whole windows, the shift
 *     per dimension (0 where the window covers the padded map), the window counts.
 *   sd_swin_window_attention: qkv (Nimg * H * W, 3 C) = the qkv Linear's output on the un-padded, un-rolled map -> out (Nimg * H * W, C): the
 *     shifted-window attention before proj, heads = C / 32 (head dimension 32), window <= 8.  Window token (i, j) of window (wy, wx) is position
 *     ((wy w + i + sh) mod pH, (wx w + j + sw) mod pW); a position past H / W is padding: its q / k / v are qkv_bias (3 C), it is NOT masked as a
 *     key, its output is dropped.  Adds table[rpi[q w^2 + k]][head] (relative_position_bias_table ((2w-1)^2, heads), relative_position_index
 *     (w^2 * w^2) int64) and, when a shift is nonzero, -100 between tokens of different regions of the rolled map.
 *   sd_swin_patch_embed: x (Nimg, 3, H, W) NCHW frames -> out (Nimg, H/4, W/4, 96): conv 4 x 4 / stride 4 (w (96, 3, 4, 4), bias (96)) and
 *     LayerNorm(96) in one launch (fp32 FMA: K = 48).
 *   sd_swin_head_pool: x (Nimg, T, C) -> pooled (Nimg, C) = mean over the T tokens of LayerNorm(x); C a multiple of 64, <= 1024.  The head
 *     Linear follows as sd_token_linear. */
size_t sd_token_packed_halfs(int N, int K);
int sd_token_pad_cols(int N);
int sd_token_pack(const float *w, int N, int K, void *planes, float *w_inv, void *stream);
int sd_token_linear(const float *A, const void *planes, const float *w_inv, const float *bias, const float *ln_w, const float *ln_b, float ln_eps,
                    const float *res, float *out, int64_t R, int N, int K, int gelu, void *stream);
int sd_token_merge_linear(const float *x, int Nimg, int H, int W, int C, const void *planes, const float *w_inv, const float *ln_w, const float *ln_b,
                          float ln_eps, float *out, int N, void *stream);
int sd_swin_window_plan(int H, int W, int window, int shift, int *plan6);
int sd_swin_window_attention(const float *qkv, const float *qkv_bias, const float *table, const int64_t *rpi, float *out, int Nimg, int H, int W,
                             int C, int heads, int window, int shift, void *stream);
int sd_swin_patch_embed(const float *x, const float *w, const float *bias, const float *ln_w, const float *ln_b, float ln_eps, float *out, int Nimg,
                        int H, int W, void *stream);
int sd_swin_head_pool(const float *x, const float *ln_w, const float *ln_b, float ln_eps, float *pooled, int Nimg, int T, int C, void *stream);

/* ---- image feed: the reference's frame preprocessing (soccer_diffusion/dataset/pytorch.py:209-211: cv2.resize(frame, (R, R),
 * interpolation=cv2.INTER_AREA), then torchvision's ToDtype(float32, scale=True) and Normalize(ImageNet mean, std)), csrc/sd_frames.hip.
 *   sd_frames_area: store (n_frames, 480, 480, 3) uint8 (the recordings' frames), 16-byte aligned; index (n_slots) int64 into it, -1 (any
 *     index outside [0, n_frames)) = a zero frame -> out (n_slots, 3, R, R) fp32, 1 <= R <= 480, one launch.  An integer factor 480 / R
 *     takes OpenCV's resizeAreaFast (taps / weights unused, may be NULL); any other R takes resizeArea with computeResizeAreaTab's table
 *     of one axis (both axes are 480 -> R): taps (3 R) int32 = first source index, tap count, offset into weights per output index;
 *     weights (n_weights <= 1440) fp32.  fp32 without FMA contraction, round half to even.
 *   sd_camera_intake: the robot node's preprocessing (soccer_diffusion/ml/inference/ros.py:186-200: cv2.resize(img, (R, R)) with the default
 *     INTER_LINEAR, then the same ToDtype and Normalize) of raw camera frames: frames (n_frames, H, W, 3) uint8 in device memory at any
 *     address (no alignment is asked for), 1 <= H, W, R <= 4096 -> out (n_frames, 3, R, R) fp32, out[c] from source channel c, or 2 - c
 *     with bgr != 0.  cv::resize's three routes, chosen here: H == R and W == R the source pixel; H == 2 R and W == 2 R INTER_AREA's
 *     (2 x 2 block sum + 2) >> 2; anything else the separable 11-bit fixed-point bilinear pass with the tables of ops.linear_taps
 *     (W -> R: xidx (R) int32 first tap, xcoef (R, 2) int16 summing to 2048; H -> R: yidx, ycoef; unused and may be NULL on the other two
 *     routes): h = S[s] c0 + S[min(s + 1, W - 1)] c1, v = (((b0 (h0 >> 4)) >> 16) + ((b1 (h1 >> 4)) >> 16) + 2) >> 2. */
/* ---- the ResNet encoder heads (soccer_diffusion/ml/model/encoder/image.py:61-83), csrc/sd_head.hip: avgpool -> fc, or the no-avgpool
 * head's Conv2d(C, 32, 1) + bias flattened in NCHW order -> fc, forward and backward, from the last block's NHWC map.
 *   sd_head_gemm: C (M x N) = A (M x K) B (K x N) (+ bias (N)), or C += that with accumulate; fp32 FMA.  Element (i, j) of an operand is
 *     ptr[off(i, row_div, row_s1, row_s0) + off(j, col_div, col_s1, col_s0)], off(i, d, s1, s0) = (i / d) s1 + (i % d) s0, or i s0 for d = 0
 *     (s0 = 0: a broadcast scalar, e.g. a single 1.0f for a column sum).  scratch: sd_head_gemm_scratch_floats(M, N, K) floats (0: none
 *     needed; NULL: one pass) - a long reduction with few output tiles is split over workgroups into it and summed by a second launch in a
 *     fixed order: deterministic, no atomics.
 *   sd_head_pool: pooled (N, C) = mean over the HW pixels of x (N, HW, C);  sd_head_pool_bwd: dx (N, HW, C) = dpooled (N, C) / HW. */
typedef struct sd_strided_operand {
    float *ptr;
    int64_t row_div, row_s1, row_s0;
    int64_t col_div, col_s1, col_s0;
} sd_strided_operand;
typedef struct sd_head_gemm_args {
    int64_t M, N, K;
    sd_strided_operand A, B, C;
    const float *bias;
    float *scratch;
    int32_t accumulate, _pad;
} sd_head_gemm_args;
size_t sd_head_gemm_scratch_floats(int64_t M, int64_t N, int64_t K);
int sd_head_gemm(const sd_head_gemm_args *args, void *stream);
int sd_head_pool(const float *x, float *pooled, int N, int HW, int C, void *stream);
int sd_head_pool_bwd(const float *dpooled, float *dx, int N, int HW, int C, void *stream);

int sd_frames_area(const uint8_t *store, int64_t n_frames, const int64_t *index, int64_t n_slots, int R, const int32_t *taps, const float *weights,
                   int n_weights, float *out, void *stream);
int sd_camera_intake(const uint8_t *frames, int64_t n_frames, int H, int W, int bgr, int R, const int32_t *xidx, const int16_t *xcoef,
                     const int32_t *yidx, const int16_t *ycoef, float *out, void *stream);

/* ---- closed-loop policy session (the receding-horizon tick of soccer_diffusion/ml/inference/ros.py:165-335), csrc/sd_session.hip.
 * A sensor ring is an fp32 device buffer (B, L, C) - one ring of L rows per robot - with one int32 head word per robot's ring in device
 * memory (head (B)): the index of the ring's OLDEST row, which is also where the next row is written.  Chronological row i of robot b is
 * ring[b][(head[b] + i) % L].  The head lives on the device so that a launch's arguments are the same at every tick.  One workgroup owns
 * a robot's ring: it reads the head, writes the rows, and moves the head after a barrier - no atomics.
 *   sd_ring_push: appends n rows per robot, oldest first, from src (B, n, C) (device memory, or pinned host memory the device can read);
 *     ring row = src row - sub (C) where sub is given (NULL: a copy); with n > L only the last L rows are written; head += n (mod L).
 *   sd_ring_window: out (B, L, C) = the chronological window of the ring (a copy).
 *   sd_session_windows: the same for up to SD_SESSION_MAX_RINGS rings in one launch; a view with wrap != 0 writes the reference's
 *     (x + 3 * np.pi) % (2 * np.pi) (ros.py:266-273) as torch evaluates it on an fp32 tensor: a = x + float(3 pi), r = fmodf(a, float(2 pi)),
 *     r += float(2 pi) where r != 0 and r < 0 - every operation exactly rounded.
 *   sd_session_commit: x (B, T, J) the sampled normalised trajectory -> out (B, T, J) = x * std + mean - float(pi) (the published trajectory,
 *     ros.py:313,327; product, sum and difference rounded one by one) and the same T rows pushed into the action-history ring (B, L, J)
 *     (ros.py:316-318).  Every element is read once and stored to both places, so out may be x (in place).
 * A subset of the robots (robots that tick at their own times, episodes that end robot by robot): the *_at forms take robots (S), int32
 * indices in device memory, and launch S workgroups (per ring); workgroup s owns robot robots[s], and the caller's arrays are compact.
 * The indices MUST BE DISTINCT: two workgroups of one launch that own the same ring race on its rows and its head word.  Nothing on the
 * device checks that - it is the host's job, before the indices are uploaded (ops.robot_index).  An index outside [0, B) is tolerated:
 * its workgroup performs no store.  Rings and head words of robots that are not named are neither read nor written.
 *   sd_ring_push_at: src (S, n, C); block s is appended to the ring of robot robots[s], as sd_ring_push appends block b to robot b's.
 *   sd_ring_window_at, sd_session_windows_at: out (S, L, C) per ring; row block s = the chronological window of robot robots[s], with
 *     the same wrap and the same 16-byte path as sd_session_windows.
 *   sd_session_commit_at: x and out (S, T, J); the T rows go into the action ring of robot robots[s] only, rounded as in sd_session_commit.
 *   sd_ring_push_quat: quats (S, n, 4) xyzw orientation samples as the IMU delivers them (ros.py:216-253) into the rotation ring, whose
 *     width says what is stored: C == 4 the rows unchanged, C == 5 dataset.quats_to_5d's row (axis xyz, sin angle, cos angle) -
 *     utils/utils.py:9-24 - computed in fp64 with the same operations in the same order (squared norm, the eps^2 guard, normalise, the
 *     (3 eps)^2 identity test giving axis (1, 0, 0) and angle 0, theta = 2 acos(clamp(w)), axis, sin, cos) and rounded to fp32 once.
 *     robots NULL: S == B and workgroup b owns robot b; otherwise as sd_ring_push_at.  n > L keeps the last L rows.
 *   S == 0 (and n == 0 in a push) returns 0 without a launch.
 *   sd_session_reset: the start state of an episode for the robots with mask[b] != 0 (mask (B) uint8 in device memory - a simulator's
 *     done flags as they are; NULL: every robot), for up to SD_SESSION_MAX_RESET_RINGS rings in ONE launch of (B, n_rings) workgroups:
 *     all L rows of the robot's ring = fill (C floats in device memory; NULL: zeros), its head word = 0 (by one thread, after a barrier),
 *     and, in ring 0's workgroup, game_state[b] = game_state_value (game_state (B) int64; NULL: none).  A workgroup whose robot is not
 *     selected returns at once.  The arguments are the same whichever robots are selected and the host reads nothing back.
 * Overlapping ticks (a session that carries the tail of one tick's trajectory into the next as pinned rows of sd_ddim_sample_pin):
 *   sd_session_commit_carry, sd_session_commit_carry_at: sd_session_commit / sd_session_commit_at that also prepare the next tick, in the
 *     same ONE launch.  All T rows are published, rounded the same way; only the first `advance` of them - the commands executed before
 *     the next tick - go into the action ring (head += advance); rows [advance, advance + carry) of x, as sampled (normalised space),
 *     become rows [0, carry) of pin_x0[robot] (pin_x0 (B, T, J)) and pin_rows[robot] = carry (pin_rows (B) int32).  advance, carry >= 0,
 *     advance + carry <= T.  x and out are indexed by workgroup (compact in the _at form), pin_x0 and pin_rows by robot.
 *   sd_session_reset_carry: sd_session_reset that also sets pin_rows[b] = 0 for the selected robots (ring 0's workgroup): their next tick
 *     is unpinned.  One launch, nothing read back.
 * Held joints (a session that hands sd_ddim_sample_hold a mask: joints another module owns, a motor that is switched off):
 *   sd_session_hold: ONE launch, one workgroup per selected robot (robots as in the _at forms; NULL: S == B).  set != 0: values of the n
 *     joints `joints` (n int32 in HOST memory, read before the launch; 0 <= joint < J <= 32) - radians as published, values[s][t][k] at
 *     s * stride_robot + t * stride_row + k, a stride of 0 broadcasts - are normalised, ((v + pi) - mean[j]) / std[j] with every
 *     operation rounded on its own (the inverse of the commit's expression), and written to pin_x0[b][t][j] for all T rows; the joints'
 *     bits are set in held[b] (held (B) int32).  set == 0: the bits are cleared, pin_x0 stays, values / mean / std may be NULL.  One
 *     thread moves the robot's word after the values are written: no atomics.
 *   sd_session_hold_mask: ONE launch composes a tick's mask, mask[(s * draws + g)][t] = held[b] | (t < pin_rows[b] ? all J bits : 0) for
 *     robot b = robots[s] (NULL: s) and every draw g; mask (S * draws, T) int32; pin_rows NULL: no carried rows.  It reads device buffers
 *     only: inside a captured tick it serves every later hold, release and reset.
 * Joint limits (a session that hands sd_ddim_sample_limits its lo / hi):
 *   sd_session_limits: ONE launch of 64 threads writes the 32-float device arrays lo_n / hi_n from limits in radians AS PUBLISHED (lo_rad,
 *     hi_rad: J floats each in HOST memory, read before the launch and passed by value; -inf / +inf: no limit; real numbers, no modular
 *     arithmetic).  A bound begins as the inverse of the commit's expression, ((v + pi) - mean[j]) / std[j], and moves inward by nextafterf
 *     (or by a quarter ulp of the commit's largest intermediate, in normalised units, where that is more; 64 tries at most) until both roundings of the commit's expression - fma(x, std, mean) - pi and
 *     (x * std + mean) - pi - give a value inside [lo, hi]: the commit is monotonic in x (std > 0), so a trajectory sampled under
 *     lo_n / hi_n is published inside the radians bit for bit with no clamp in the commit.  Slots [J, 32) get -inf / +inf.  A range
 *     narrower than the commit's resolution collapses to its upper bound.  SD_E_BADARG also for lo_rad[j] > hi_rad[j] or a NaN.
 * Slew limits (a session that hands sd_ddim_sample_slew its v and start):
 *   sd_session_slew: ONE launch of 64 threads writes the 32-float device array v_n from v_rad, radians per row AS PUBLISHED (J floats in
 *     HOST memory, passed by value; +inf: no limit), and bound_rad, a finite bound on |published value| per joint (J floats, HOST):
 *     v_n[j] = (v_rad[j] - margin) / std[j] rounded toward zero, margin = std hu(XS / std) + 2 hu(XS) + 2 hu(pi + R) + 2 hu(R) with
 *     R = bound_rad[j], XS = R + |pi - mean[j]| and hu(z) half an fp32 ulp at z, in fp64 - what the rounding of y +- v in the scan and both roundings of the commit's expression can add to a difference of two
 *     published values.  Consecutive published rows of a rollout sampled under v_n then differ by at most v_rad[j],
 *     evaluated exactly, as long as |published| <= bound_rad[j].  Slots [J, 32): +inf.  SD_E_BADARG also for a negative or NaN v_rad[j].
 *   sd_session_anchor: ONE launch copies row `row` of x (S, T, J; normalised space, as sampled) into anchor (B * draws, 32), rows
 *     (b * draws + g) for robot b = robots[s] (NULL: s) and every draw g - the start array of the robot's next tick.
 * Acceleration limits (a session that hands sd_ddim_sample_accel its a, start and start2):
 *   sd_session_accel: sd_session_slew for a_rad, radians per row^2 AS PUBLISHED: a_n[j] = (a_rad[j] - margin) / std[j] rounded toward zero,
 *     margin = 4 std hu(3 XS / std) + 4 hu(XS) + 4 hu(pi + R) + 4 hu(R) - the four roundings of the scan's row function at magnitudes up to
 *     3 XS / std and both roundings of the commit's expression at three published values with weights 1, 2 and 1.
 *   sd_session_anchor2: sd_session_anchor with a second destination, in ONE launch: anchor2 <- row >= 1 ? row (row - 1) of x : the old
 *     anchor, then anchor <- row `row` of x (row = advance - 1).  anchor and anchor2: (B * draws, 32) each, not the same array.
 * SD_E_BADARG on null pointers or non-positive sizes, before any launch. */
#define SD_SESSION_MAX_RINGS 3
#define SD_SESSION_MAX_RESET_RINGS 5
typedef struct sd_ring_view {
    const float *ring;     /* (B, L, C) */
    const int32_t *head;   /* (B) */
    float *out;            /* (B, L, C) */
    int32_t L, C;
    int32_t wrap, _pad;
} sd_ring_view;
typedef struct sd_ring_reset {
    float *ring;         /* (B, L, C) */
    int32_t *head;       /* (B) */
    const float *fill;   /* (C), or NULL for zeros */
    int32_t L, C;
} sd_ring_reset;
int sd_ring_push(float *ring, int32_t *head, const float *src, const float *sub, int B, int L, int C, int n, void *stream);
int sd_ring_window(const float *ring, const int32_t *head, float *out, int B, int L, int C, void *stream);
int sd_session_windows(const sd_ring_view *views, int n_views, int B, void *stream);
int sd_session_commit(const float *x, const float *mean, const float *stdv, float *out, float *ring, int32_t *head, int B, int T, int J, int L,
                      void *stream);
int sd_ring_push_at(float *ring, int32_t *head, const float *src, const float *sub, const int32_t *robots, int S, int B, int L, int C, int n,
                    void *stream);
int sd_ring_push_quat(float *ring, int32_t *head, const float *quats, const int32_t *robots, int S, int B, int L, int C, int n, void *stream);
int sd_ring_window_at(const float *ring, const int32_t *head, float *out, const int32_t *robots, int S, int B, int L, int C, void *stream);
int sd_session_windows_at(const sd_ring_view *views, int n_views, const int32_t *robots, int S, int B, void *stream);
int sd_session_commit_at(const float *x, const float *mean, const float *stdv, float *out, float *ring, int32_t *head, const int32_t *robots,
                         int S, int B, int T, int J, int L, void *stream);
int sd_session_reset(const sd_ring_reset *rings, int n_rings, const uint8_t *mask, int64_t *game_state, int64_t game_state_value, int B,
                     void *stream);
int sd_session_commit_carry(const float *x, const float *mean, const float *stdv, float *out, float *ring, int32_t *head, int B, int T, int J,
                            int L, int advance, int carry, float *pin_x0, int32_t *pin_rows, void *stream);
int sd_session_commit_carry_at(const float *x, const float *mean, const float *stdv, float *out, float *ring, int32_t *head,
                               const int32_t *robots, int S, int B, int T, int J, int L, int advance, int carry, float *pin_x0,
                               int32_t *pin_rows, void *stream);
int sd_session_reset_carry(const sd_ring_reset *rings, int n_rings, const uint8_t *mask, int64_t *game_state, int64_t game_state_value,
                           int32_t *pin_rows, int B, void *stream);
int sd_session_hold(float *pin_x0, int32_t *held, const float *values, int64_t stride_robot, int64_t stride_row, const int32_t *joints, int n,
                    const float *mean, const float *stdv, const int32_t *robots, int S, int B, int T, int J, int set, void *stream);
int sd_session_limits(float *lo_n, float *hi_n, const float *lo_rad, const float *hi_rad, const float *mean, const float *stdv, int J, void *stream);
int sd_session_slew(float *v_n, const float *v_rad, const float *bound_rad, const float *mean, const float *stdv, int J, void *stream);
int sd_session_anchor(float *anchor, const float *x, const int32_t *robots, int S, int B, int T, int J, int row, int draws, void *stream);
int sd_session_accel(float *a_n, const float *a_rad, const float *bound_rad, const float *mean, const float *stdv, int J, void *stream);
int sd_session_anchor2(float *anchor, float *anchor2, const float *x, const int32_t *robots, int S, int B, int T, int J, int row, int draws,
                       void *stream);
int sd_session_hold_mask(int32_t *mask, const int32_t *held, const int32_t *pin_rows, const int32_t *robots, int S, int B, int T, int J,
                         int draws, void *stream);

/* ---- measurement hooks (bench.py roofline leg; not part of the reference's surface) ----
 * While enabled, every kernel launch made by this library is bracketed by a hipEvent pair
 * on the launch stream.  sd_profile_collect waits for them, returns the summed device
 * milliseconds and launch counts per kernel class, and clears the records.  Do not
 * enable during hipGraph capture. */
#define SD_KCLASS_PANEL_GEMM 0   /* panel_gemm_kernel<...>  (all LN/act/res variants)  */
#define SD_KCLASS_ATTENTION 1    /* attention_kernel<HD>                                */
#define SD_KCLASS_PATCH_EMBED 2  /* patch_embed_kernel                                  */
#define SD_KCLASS_FC_OUT 3       /* fc_out_kernel (+ fused DDIM update)                 */
#define SD_KCLASS_LAYER_CHAIN 4  /* decoder_layer_kernel / chain_a_kernel / chain_b_kernel */
#define SD_KCLASS_HEAD 5         /* decoder_head_kernel (embed + LN1 + QKV of layer 0)   */
#define SD_KCLASS_TRAJ_STEP 6    /* traj_step_kernel: one whole denoiser step per launch (sampler mode 3) */
#define SD_KCLASS_COUNT 7
int sd_profile_enable(int on);
int sd_profile_collect(double *ms_by_class, long *launches_by_class, int n_classes);

#ifdef __cplusplus
}
#endif
#endif /* SOCCERDIFFUSION_HIP_H */
