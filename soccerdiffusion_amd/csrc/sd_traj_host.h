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
// B: the contexts to fold - the call's trajectories, or B / draws of a shared-context call
int traj_prepare_ctx(const sd_denoiser_weights *w, const TrajWs &s, const float *ctx, int B, int Mc, int nkt, hipStream_t st);
int traj_prepare_steps(const sd_denoiser_weights *w, const TrajWs &s, const float *tokens, int n_tok, int Mc, hipStream_t st, bool per_traj = false);
// One denoiser step (+ DDIM update when r.coef != NULL) in one launch (StepReq: sd_common.h).
// precise: three fp16 products at the Q | K | V site (sampler mode 3), else two (mode 4, which reports sharp logits through r.status).
// r.pin (needs r.coef and precise: mode 4 has no pinned twin): rows below pin->rows[b] become c2 * x0 + c3 * noise in the same launch.
// r.draws > 1 (rollouts only: not per_traj): the B trajectories read the folded blocks of C = B / draws contexts - traj_prepare_ctx ran
// with C - through the shared-context instantiations (sd_traj_draws.hip), pinned or not.
// r.hold (needs r.coef and precise, excludes r.pin): the elements whose bit is set in hold->mask become c2 * x0 + c3 * noise in the
// same launch - the hold instantiations (sd_traj_hold.hip), which take r.draws at run time (1 included).
// r.ms (needs r.coef and precise, excludes r.pin; r.hold optional, its mask too): the multistep instantiations (sd_traj_ms.hip) - the
// hold's epilogue plus ms->w * (ms->hist - x0) on the DDIM update, x0 left in ms->hist; ms->hist is not read when ms->w == 0.
// r.lim (needs r.ms, whose hist may then be NULL: first-order DDIM): the limits instantiations (sd_traj_lim.hip) - the multistep epilogue on
// x0 clamped to [lim->lo[j], lim->hi[j]] (LimitArgs, sd_common.h).
// r.slew (needs r.lim, whose bounds may all be infinite): the slew instantiations (sd_traj_slew.hip) - the limits epilogue on x0 after the
// scan over the rows (SlewArgs, sd_common.h), exchanged through LDS behind two workgroup barriers.
int traj_step(const sd_denoiser_weights *w, const TrajWs &s, const StepReq &r, hipStream_t st, int nkt, bool precise);
// DDIM steps r.i .. r.i + n - 1 of the r.n_tok prepared ones in ONE launch of the rollout kernel (the plan's rollout_fused: one key tile,
// nothing returned per step, no pin: r.eps, r.pin NULL); n <= TRAJ_ROLLOUT_MAX_STEPS - the per-step scalars travel in the kernel
// argument - so the driver launches a longer rollout in chunks.  r.coef: the rollout's whole table (4 per step).  r.draws as traj_step.
constexpr int TRAJ_ROLLOUT_MAX_STEPS = 64;
int traj_steps_fused(const sd_denoiser_weights *w, const TrajWs &s, const StepReq &r, int n, hipStream_t st, bool precise);
#endif
