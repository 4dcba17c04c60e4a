// Limits instantiations of the tuned trajectory step kernels (sd_traj.h: traj_step_lim_kernel, traj_step_wide_lim_kernel):
// sd_ddim_sample_limits - per-joint limits on the predicted clean trajectory inside the step launch.  The epilogue is the multistep twins'
// (sd_traj_ms.hip) with an optional history (MultistepArgs.hist NULL: first-order DDIM) plus one clamp: the lane that stores the update of
// (token, 4 joints) clamps x0 to [lo[j], hi[j]] with compares and selects - a NaN stays NaN - forms the update from the clamped x0 and
// leaves the clamped x0 in the history array (LimitArgs, limit_update: sd_common.h).  The group size of a shared-context call is a runtime
// argument, so the 7 + 7 instantiations serve DDIM and multistep, plain, pinned (a leading-rows mask), held and shared-context calls alike.
// This unit holds them and nothing else: they compile beside sd_traj.hip's, not behind them.  sd_traj.hip asks for the kernel pointers and
// launches them (traj_step).
//
// Built without packed fp32 vector instructions like sd_traj.hip (soccerdiffusion_amd/build.py, EXTRA_FLAGS); build() checks the object.

#include <hip/hip_runtime.h>
#include <math.h>

#include "sd_common.h"
#include "sd_traj.h"

// ntt = ceil(T / 16) token tiles; wide: more than 16 memory rows.  Three fp16 products everywhere (mode 4 has no limits twin).
typedef void (*TrajStepLimFn)(tj::StepArgs, HoldArgs, MultistepArgs, LimitArgs, int);
TrajStepLimFn traj_step_lim_fn(int ntt, bool wide) {
    return by_ntt<7>(ntt, [wide](auto n) {
        constexpr int N = decltype(n)::value;
        return wide ? tj::traj_step_wide_lim_kernel<N> : tj::traj_step_lim_kernel<N>;
    });
}
