// Host interface of the tuned trajectory step kernels (sd_traj.hip; device code: sd_traj.h) towards the sampler's driver (sd_kernels.hip).
// Not part of the public ABI.
#ifndef SD_TRAJ_HOST_H
#define SD_TRAJ_HOST_H
#include "sd_common.h"
#include "sd_sampler_plan.h"   // traj_ok: the shapes the tuned kernels are instantiated for
struct sd_denoiser_weights;

// The tuned path has no workspace region of its own: it writes its operands into the regions the driver carves for sampler mode 2
// (same folded blocks and abs-max words, the split planes in sd_traj.h's fragment order).  Filled from the driver's carve-up in one place.
struct TrajWs {
    float *kvtmp, *kvstep;              // fp32 scratch for the projected context rows / step tokens
    float *gv, *cb, *gvstep, *cstep;    // folded cross-attention blocks
    f16 *wf, *g16, *v16, *gstep16, *vstep16, *wio;
    float *scales;
    unsigned *maxbits;
    int *stepmap;
};

// the three preparation stages (weights; context rows; n_tok step tokens - per_traj: one per trajectory, the distinct ones only)
int traj_prepare_weights(const sd_denoiser_weights *w, const TrajWs &s, hipStream_t st);
// nkt: the plan's key tiles (SamplerPlan::key_tiles), the same for traj_prepare_ctx and traj_step of one workspace
int traj_prepare_ctx(const sd_denoiser_weights *w, const TrajWs &s, const float *ctx, int B, int Mc, int nkt, hipStream_t st);
int traj_prepare_steps(const sd_denoiser_weights *w, const TrajWs &s, const float *tokens, int n_tok, int Mc, hipStream_t st, bool per_traj = false);
// one denoiser step (+ DDIM update when coef != NULL); step index i of the n_tok prepared step blocks, or block b for trajectory b (per_traj).
// precise: three fp16 products at the Q | K | V site (sampler mode 3), else two (mode 4, which reports sharp logits through status).
// pin (needs coef and precise: mode 4 has no pinned twin): rows below pin->rows[b] become c2 * x0 + c3 * noise in the same launch
int traj_step(const sd_denoiser_weights *w, const TrajWs &s, float *x, float *eps, int B, int T, int Mc, int i, int n_tok, const float *coef,
              bool per_traj, hipStream_t st, int nkt, bool precise, int32_t *status, const PinArgs *pin = nullptr);
// DDIM steps i0 .. i0 + n - 1 of the n_tok prepared ones in ONE launch of the rollout kernel (the plan's rollout_fused: one key tile, nothing
// returned per step, no pin); n <= TRAJ_ROLLOUT_MAX_STEPS - the per-step scalars travel in the kernel argument - so the driver launches a
// longer rollout in chunks.  coef: the rollout's whole table (4 per step).
constexpr int TRAJ_ROLLOUT_MAX_STEPS = 64;
int traj_steps_fused(const sd_denoiser_weights *w, const TrajWs &s, float *x, int B, int T, int Mc, int i0, int n, int n_tok, const float *coef,
                     hipStream_t st, bool precise, int32_t *status);
// Shared-context calls (sd_ddim_sample_draws, draws > 1; sd_traj_draws.hip): the B trajectories read the folded blocks of C = B / draws
// contexts - traj_prepare_ctx ran with C - through the shared instantiations of the step kernels.  pin may be NULL (one kernel serves
// both); the two-product kernels (precise false) take no pin.  Otherwise traj_step / traj_steps_fused argument for argument.
int traj_step_draws(const sd_denoiser_weights *w, const TrajWs &s, float *x, float *eps, int B, int T, int Mc, int i, int n_tok, const float *coef,
                    hipStream_t st, int nkt, bool precise, int32_t *status, const PinArgs *pin, int draws);
int traj_steps_fused_draws(const sd_denoiser_weights *w, const TrajWs &s, float *x, int B, int T, int Mc, int i0, int n, int n_tok, const float *coef,
                           hipStream_t st, bool precise, int32_t *status, int draws);
#endif
