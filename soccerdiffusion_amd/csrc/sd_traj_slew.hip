// Slew instantiations of the tuned trajectory step kernels (sd_traj.h: traj_step_slew_kernel, traj_step_wide_slew_kernel):
// sd_ddim_sample_slew - per-joint slew (velocity) limits on the predicted clean trajectory inside the step launch.  The epilogue is the
// limits twins' (sd_traj_lim.hip) around the scan over the rows: the storing lanes write x0 of (token, 4 joints) - the hold's value where
// the mask says so - into an fp32 plane in the Q | K region of LDS, a workgroup barrier, lane j of wave 0 runs slew_row (sd_common.h) down
// column j in row order, a second barrier, and the storing lanes form the update from the x0c they read back.  Both barriers stand outside
// the epilogue's `if (c.w < NTT)`: all eight waves reach them.  LDS_BYTES is what it was.  The group size of a shared-context call is a
// runtime argument, so the 7 + 7 instantiations serve DDIM and multistep, plain, pinned (a leading-rows mask), held and shared-context
// calls alike.  This unit holds them and nothing else.  sd_traj.hip asks for the kernel pointers and launches them (traj_step).
//
// Built without packed fp32 vector instructions like sd_traj.hip (soccerdiffusion_amd/build.py, EXTRA_FLAGS); build() checks the object.

#include <hip/hip_runtime.h>
#include <math.h>

#include "sd_common.h"
#include "sd_traj.h"

// ntt = ceil(T / 16) token tiles; wide: more than 16 memory rows.  Three fp16 products everywhere (mode 4 has no slew twin).
typedef void (*TrajStepSlewFn)(tj::StepArgs, HoldArgs, MultistepArgs, LimitArgs, SlewArgs, int);
TrajStepSlewFn traj_step_slew_fn(int ntt, bool wide) {
    return by_ntt<7>(ntt, [wide](auto n) {
        constexpr int N = decltype(n)::value;
        return wide ? tj::traj_step_wide_slew_kernel<N> : tj::traj_step_slew_kernel<N>;
    });
}
