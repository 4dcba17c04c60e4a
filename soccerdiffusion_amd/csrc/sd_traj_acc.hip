// Acceleration instantiations of the tuned trajectory step kernels (sd_traj.h: traj_step_accel_kernel, traj_step_wide_accel_kernel):
// sd_ddim_sample_accel - per-joint acceleration limits on the predicted clean trajectory inside the step launch.  They are the slew twins
// (sd_traj_slew.hip), phase for phase - x0 exchanged through the fp32 plane in the Q | K region of LDS, two workgroup barriers that all
// eight waves reach, lane j of wave 0 walking column j in row order - with accel_row (sd_common.h) in the scan: the lane carries the two
// rows before and limits x0 around their constant-velocity continuation before the slew interval, the box and the hold.  LDS_BYTES is
// what it was.  The group size of a shared-context call is a runtime argument, so the 7 + 7 instantiations serve DDIM and multistep,
// plain, pinned (a leading-rows mask), held and shared-context calls alike.  This unit holds them and nothing else.  sd_traj.hip asks for
// the kernel pointers and launches them (traj_step).
//
// Built without packed fp32 vector instructions like sd_traj.hip (soccerdiffusion_amd/build.py, EXTRA_FLAGS); build() checks the object.

#include <hip/hip_runtime.h>
#include <math.h>

#include "sd_common.h"
#include "sd_traj.h"

// ntt = ceil(T / 16) token tiles; wide: more than 16 memory rows.  Three fp16 products everywhere (mode 4 has no acceleration twin).
typedef void (*TrajStepAccelFn)(tj::StepArgs, HoldArgs, MultistepArgs, LimitArgs, SlewArgs, AccelArgs, int);
TrajStepAccelFn traj_step_accel_fn(int ntt, bool wide) {
    return by_ntt<7>(ntt, [wide](auto n) {
        constexpr int N = decltype(n)::value;
        return wide ? tj::traj_step_wide_accel_kernel<N> : tj::traj_step_accel_kernel<N>;
    });
}
