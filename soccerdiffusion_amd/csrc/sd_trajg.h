// Host interface of the generic trajectory step kernels (sd_trajg.hip) towards the sampler's driver (sd_kernels.hip).  Not part of the
// public ABI.
#ifndef SD_TRAJG_H
#define SD_TRAJG_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "sd_common.h"          // StepReq
#include "sd_sampler_plan.h"   // trajg_ok: the shapes the generic kernels are instantiated for
struct sd_denoiser_weights;

// floats of workspace behind the driver's own carve-up: split weight planes, the memory's K / V^T planes, step rows, scales
size_t trajg_workspace_floats(int B, int Mc, int d, int L, int n_tok);
// the three preparation stages of the trajectory path (as traj_prepare_* of the tuned family: sd_traj_host.h); kvtmp / kvstep: fp32 scratch of
// L * B * Mc * 2 d and L * n_tok * 2 d floats for the projected rows
int trajg_prepare_weights(const sd_denoiser_weights *w, float *gws, int B, int Mc, int n_tok, hipStream_t st);
// ctx holds C contexts, each shared by B / C consecutive trajectories (C = B, or B / draws of sd_ddim_sample_draws): they are projected and packed
int trajg_prepare_ctx(const sd_denoiser_weights *w, float *gws, const float *ctx, float *kvtmp, int B, int Mc, int n_tok, hipStream_t st, int C);
// map (or NULL): per-trajectory step tokens, trajectory b uses the rows of token map[b] (step_map_kernel: duplicates of token 0 are prepared once)
int trajg_prepare_steps(const sd_denoiser_weights *w, float *gws, const float *tokens, float *kvstep, int B, int Mc, int n_tok, hipStream_t st,
                        const int *map = nullptr);
// One denoiser step (+ DDIM update when r.coef != NULL) in one launch (StepReq: sd_common.h).  map: the step map of a per_traj request.
// r.pin (needs r.coef): the pinned instantiation - rows below pin->rows[b] become c2 * x0 + c3 * noise in the same launch.
// r.draws > 1 (not per_traj): trajectory b reads the planes of context b / draws - traj_step_generic_draws_kernel, pinned or not
// r.hold (needs r.coef, excludes r.pin): held elements (HoldArgs) - traj_step_generic_hold_kernel, whatever r.draws
// r.ms (needs r.coef, excludes r.pin; r.hold optional): the multistep twin (MultistepArgs) - traj_step_generic_ms_kernel, whatever r.draws
// r.lim (needs r.ms, whose hist may then be NULL: DDIM): the limits twin (LimitArgs) - traj_step_generic_lim_kernel, whatever r.draws
// r.slew (needs r.lim, whose bounds may all be infinite): the slew twin (SlewArgs) - traj_step_generic_slew_kernel, whatever r.draws
int trajg_step(const sd_denoiser_weights *w, float *gws, const StepReq &r, hipStream_t st, const int *map = nullptr);
#endif
