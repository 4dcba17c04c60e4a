// Multistep instantiations of the tuned trajectory step kernels (sd_traj.h: traj_step_ms_kernel, traj_step_wide_ms_kernel):
// sd_ddim_sample_multistep - the second-order multistep solver (DPM-Solver++ 2M in its x0 form) inside the step launch.  The epilogue is the
// hold twins' (sd_traj_hold.hip) with an optional mask (HoldArgs.mask NULL: nothing held) plus one term: the lane that stores the update of
// (token, 4 joints) adds w * (x0 of the previous step - x0 of this one) to the DDIM update and leaves this step's x0 in the history array
// (MultistepArgs, sd_common.h).  w == 0 (the first and the last step): the history is not read.  The group size of a shared-context call is
// a runtime argument, so the 7 + 7 instantiations serve plain, pinned (a leading-rows mask), held and shared-context calls alike.  This
// unit holds them and nothing else: they compile beside sd_traj.hip's, not behind them.  sd_traj.hip asks for the kernel pointers and
// launches them (traj_step).
//
// Built without packed fp32 vector instructions like sd_traj.hip (soccerdiffusion_amd/build.py, EXTRA_FLAGS); build() checks the object.

#include <hip/hip_runtime.h>
#include <math.h>

#include "sd_common.h"
#include "sd_traj.h"

// ntt = ceil(T / 16) token tiles; wide: more than 16 memory rows.  Three fp16 products everywhere (mode 4 has no multistep twin).
typedef void (*TrajStepMsFn)(tj::StepArgs, HoldArgs, MultistepArgs, int);
TrajStepMsFn traj_step_ms_fn(int ntt, bool wide) {
    return by_ntt<7>(ntt, [wide](auto n) {
        constexpr int N = decltype(n)::value;
        return wide ? tj::traj_step_wide_ms_kernel<N> : tj::traj_step_ms_kernel<N>;
    });
}
