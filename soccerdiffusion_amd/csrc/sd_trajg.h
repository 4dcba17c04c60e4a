// Host interface of the generic trajectory step kernels (sd_trajg.hip) towards the sampler's driver (sd_kernels.hip).  Not part of the
// public ABI.
#ifndef SD_TRAJG_H
#define SD_TRAJG_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "sd_common.h"          // PinArgs
#include "sd_sampler_plan.h"   // trajg_ok: the shapes the generic kernels are instantiated for
struct sd_denoiser_weights;

// floats of workspace behind the driver's own carve-up: split weight planes, the memory's K / V^T planes, step rows, scales
size_t trajg_workspace_floats(int B, int Mc, int d, int L, int n_tok);
// the three preparation stages of the trajectory path (as traj_prepare_* of the tuned family: sd_traj_host.h); kvtmp / kvstep: fp32 scratch of
// L * B * Mc * 2 d and L * n_tok * 2 d floats for the projected rows
int trajg_prepare_weights(const sd_denoiser_weights *w, float *gws, int B, int Mc, int n_tok, hipStream_t st);
// C > 0: ctx holds C contexts shared by B / C consecutive trajectories each (sd_ddim_sample_draws): only they are projected and packed
int trajg_prepare_ctx(const sd_denoiser_weights *w, float *gws, const float *ctx, float *kvtmp, int B, int Mc, int n_tok, hipStream_t st, int C = 0);
// map (or NULL): per-trajectory step tokens, trajectory b uses the rows of token map[b] (step_map_kernel: duplicates of token 0 are prepared once)
int trajg_prepare_steps(const sd_denoiser_weights *w, float *gws, const float *tokens, float *kvstep, int B, int Mc, int n_tok, hipStream_t st,
                        const int *map = nullptr);
// one denoiser step (+ DDIM update when coef != NULL); step index i of the n_tok prepared step rows, or row b for trajectory b (per_traj).
// pin (needs coef): the pinned instantiation - rows below pin->rows[b] become c2 * x0 + c3 * noise in the same launch
int trajg_step(const sd_denoiser_weights *w, float *gws, float *x, float *eps, int B, int T, int Mc, int i, int n_tok, const float *coef,
               bool per_traj, hipStream_t st, const int *map = nullptr, const PinArgs *pin = nullptr, int draws = 1);
// draws > 1 (not per_traj): trajectory b reads the planes of context b / draws - traj_step_generic_draws_kernel, pinned or not
#endif
