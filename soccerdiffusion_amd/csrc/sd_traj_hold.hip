// Hold instantiations of the tuned trajectory step kernels (sd_traj.h: traj_step_hold_kernel, traj_step_wide_hold_kernel):
// sd_ddim_sample_hold - chosen ELEMENTS of a trajectory (one mask word per (trajectory, row): HoldArgs, sd_common.h) are held at
// c2 * known + c3 * noise in the step's own epilogue instead of receiving the DDIM update.  The group size of a shared-context call is a
// runtime argument of these kernels, so the 7 + 7 instantiations serve draws == 1 and draws > 1 alike.  This unit holds them and nothing
// else: they compile beside sd_traj.hip's, not behind them.  sd_traj.hip asks for the kernel pointers and launches them (traj_step).
//
// Built without packed fp32 vector instructions like sd_traj.hip (soccerdiffusion_amd/build.py, EXTRA_FLAGS); build() checks the object.

#include <hip/hip_runtime.h>
#include <math.h>

#include "sd_common.h"
#include "sd_traj.h"

// ntt = ceil(T / 16) token tiles; wide: more than 16 memory rows.  Three fp16 products everywhere (mode 4 has no hold twin).
typedef void (*TrajStepHoldFn)(tj::StepArgs, HoldArgs, int);
TrajStepHoldFn traj_step_hold_fn(int ntt, bool wide) {
    return by_ntt<7>(ntt, [wide](auto n) {
        constexpr int N = decltype(n)::value;
        return wide ? tj::traj_step_wide_hold_kernel<N> : tj::traj_step_hold_kernel<N>;
    });
}
