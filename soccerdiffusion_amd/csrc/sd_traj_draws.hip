// Shared-context instantiations of the tuned trajectory step kernels (sd_traj.h: traj_step_draws_kernel, traj_step_wide_draws_kernel,
// traj_step_rollout_draws_kernel): sd_ddim_sample_draws with draws > 1 - the B trajectories of a call are C = B / draws groups of `draws`
// consecutive ones, and a group reads ONE context's folded cross-attention blocks, prepared once (traj_prepare_ctx over C rows of
// context).  This unit holds the 35 instantiations and nothing else: they compile beside sd_traj.hip's, not behind them.  sd_traj.hip asks
// for the kernel pointers and launches them (traj_step, traj_steps_fused with draws > 1).
//
// Built without packed fp32 vector instructions like sd_traj.hip (soccerdiffusion_amd/build.py, EXTRA_FLAGS); build() checks the object.

#include <hip/hip_runtime.h>
#include <math.h>

#include "sd_common.h"
#include "sd_traj.h"

// ntt = ceil(T / 16) token tiles; variant as in sd_traj.hip: 0 = two products at the Q | K | V site, 1 = three, 2 = the wide kernel
typedef void (*TrajStepDrawsFn)(tj::StepArgs, PinArgs, int);
TrajStepDrawsFn traj_step_draws_fn(int ntt, int variant) {
    return by_ntt<7>(ntt, [variant](auto n) {
        constexpr int N = decltype(n)::value;
        return variant == 2 ? tj::traj_step_wide_draws_kernel<N> : variant == 1 ? tj::traj_step_draws_kernel<N, true> : tj::traj_step_draws_kernel<N, false>;
    });
}
typedef void (*TrajRolloutDrawsFn)(tj::RolloutDrawsArgs);
TrajRolloutDrawsFn traj_rollout_draws_fn(int ntt, bool precise) {
    return by_ntt<7>(ntt, [precise](auto n) {
        constexpr int N = decltype(n)::value;
        return precise ? tj::traj_step_rollout_draws_kernel<N, true> : tj::traj_step_rollout_draws_kernel<N, false>;
    });
}
