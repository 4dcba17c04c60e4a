// Direct instantiations of the tuned trajectory step kernels (sd_traj.h: traj_step_direct_kernel, traj_step_wide_direct_kernel):
// sd_direct_sample - a distilled one-step decoder under held elements, per-joint limits and slew limits in ONE launch.  The network's
// output is x0: the epilogue is the slew twins' (sd_traj_slew.hip) without a DDIM coefficient, an update or a history - the storing lanes
// write the prediction of (token, 4 joints) to eps_out and, the hold's value where the mask says so, into the fp32 plane in the Q | K
// region of LDS, a workgroup barrier, lane j of wave 0 runs slew_row (sd_common.h) down column j in row order, a second barrier, and the
// storing lanes store the x0c they read back to `out`.  Both barriers stand outside the epilogue's `if (c.w < NTT)`; without slew limits
// (sl.v NULL: uniform over the workgroup) there is no exchange, no scan and no barrier.  x is only read.  LDS_BYTES is what it was.  The
// group size of a shared-context call is a runtime argument, so the 7 + 7 instantiations serve plain, held, limited, slewed and
// shared-context calls alike.  This unit holds them and nothing else.  sd_traj.hip asks for the kernel pointers and launches them
// (traj_step).
//
// Built without packed fp32 vector instructions like sd_traj.hip (soccerdiffusion_amd/build.py, EXTRA_FLAGS); build() checks the object.

#include <hip/hip_runtime.h>
#include <math.h>

#include "sd_common.h"
#include "sd_traj.h"

// ntt = ceil(T / 16) token tiles; wide: more than 16 memory rows.  Three fp16 products everywhere (mode 4 has no direct twin).
typedef void (*TrajStepDirectFn)(tj::StepArgs, HoldArgs, LimitArgs, SlewArgs, DirectArgs, int);
TrajStepDirectFn traj_step_direct_fn(int ntt, bool wide) {
    return by_ntt<7>(ntt, [wide](auto n) {
        constexpr int N = decltype(n)::value;
        return wide ? tj::traj_step_wide_direct_kernel<N> : tj::traj_step_direct_kernel<N>;
    });
}
