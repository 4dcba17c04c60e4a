// Shared-context instantiations of the tuned trajectory step kernels (sd_traj.h: traj_step_draws_kernel, traj_step_wide_draws_kernel,
// traj_step_rollout_draws_kernel) and their launches: sd_ddim_sample_draws with draws > 1 - the B trajectories of a call are C = B / draws
// groups of `draws` consecutive ones, and a group reads ONE context's folded cross-attention blocks, prepared once (traj_prepare_ctx over C
// rows of context).  A unit of its own: the 35 instantiations compile beside sd_traj.hip's, not behind them, and that unit's object stays
// the parent's.  Interface towards the sampler's driver (sd_kernels.hip): sd_traj_host.h.
//
// Built without packed fp32 vector instructions like sd_traj.hip (soccerdiffusion_amd/build.py, EXTRA_FLAGS); build() checks the object.

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/soccerdiffusion_hip.h"

#include "sd_common.h"
#include "sd_traj.h"
#include "sd_traj_host.h"

// sd_traj.hip: the kernel argument of step i, the layers' plane regions C contexts long
tj::StepArgs traj_step_args(const sd_denoiser_weights *w, const TrajWs &s, float *x, float *eps, int B, int T, int Mc, int i, int n_steps, const float *coef,
                            bool per_traj, int nkt, int32_t *status, int C);

typedef void (*TrajStepDrawsFn)(tj::StepArgs, PinArgs, int);
static TrajStepDrawsFn traj_step_wide_draws_fn(int ntt) {
    switch (ntt) {
        case 1: return tj::traj_step_wide_draws_kernel<1>;
        case 2: return tj::traj_step_wide_draws_kernel<2>;
        case 3: return tj::traj_step_wide_draws_kernel<3>;
        case 4: return tj::traj_step_wide_draws_kernel<4>;
        case 5: return tj::traj_step_wide_draws_kernel<5>;
        case 6: return tj::traj_step_wide_draws_kernel<6>;
        case 7: return tj::traj_step_wide_draws_kernel<7>;
        default: return nullptr;
    }
}
template <bool PRECISE>
static TrajStepDrawsFn traj_step_draws_fn(int ntt) {
    switch (ntt) {
        case 1: return tj::traj_step_draws_kernel<1, PRECISE>;
        case 2: return tj::traj_step_draws_kernel<2, PRECISE>;
        case 3: return tj::traj_step_draws_kernel<3, PRECISE>;
        case 4: return tj::traj_step_draws_kernel<4, PRECISE>;
        case 5: return tj::traj_step_draws_kernel<5, PRECISE>;
        case 6: return tj::traj_step_draws_kernel<6, PRECISE>;
        case 7: return tj::traj_step_draws_kernel<7, PRECISE>;
        default: return nullptr;
    }
}
typedef void (*TrajRolloutDrawsFn)(tj::RolloutDrawsArgs);
template <bool PRECISE>
static TrajRolloutDrawsFn traj_rollout_draws_fn(int ntt) {
    switch (ntt) {
        case 1: return tj::traj_step_rollout_draws_kernel<1, PRECISE>;
        case 2: return tj::traj_step_rollout_draws_kernel<2, PRECISE>;
        case 3: return tj::traj_step_rollout_draws_kernel<3, PRECISE>;
        case 4: return tj::traj_step_rollout_draws_kernel<4, PRECISE>;
        case 5: return tj::traj_step_rollout_draws_kernel<5, PRECISE>;
        case 6: return tj::traj_step_rollout_draws_kernel<6, PRECISE>;
        case 7: return tj::traj_step_rollout_draws_kernel<7, PRECISE>;
        default: return nullptr;
    }
}

// one denoiser step + DDIM update of B = C * draws trajectories in ONE launch (traj_step with the context index b / draws)
int traj_step_draws(const sd_denoiser_weights *w, const TrajWs &s, float *x, float *eps, int B, int T, int Mc, int i, int n_steps, const float *coef,
                    hipStream_t st, int nkt, bool precise, int32_t *status, const PinArgs *pin, int draws) {
    if (draws < 2 || B % draws) return fail(SD_E_BADARG, "traj_step_draws_kernel: B must be a multiple of draws >= 2");
    const tj::StepArgs a = traj_step_args(w, s, x, eps, B, T, Mc, i, n_steps, coef, false, nkt, status, B / draws);
    const int ntt = (T + 15) / 16;
    const int variant = nkt > 1 ? 2 : (precise ? 1 : 0);
    const TrajStepDrawsFn fn = variant == 2 ? traj_step_wide_draws_fn(ntt) : (precise ? traj_step_draws_fn<true>(ntt) : traj_step_draws_fn<false>(ntt));
    if (!fn) return fail(SD_E_BADARG, "traj_step_draws_kernel: horizon out of range");
    if (pin && (!coef || variant == 0)) return fail(SD_E_BADARG, "traj_step_draws_kernel: pinned rows need the DDIM coefficients and the three-product kernels");
    ProfScope prof(SD_KCLASS_TRAJ_STEP, st);
    static DevFlag attr_set[3][8];
    if (!attr_set[variant][ntt]) {
        const hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, tj::LDS_BYTES);
        if (e != hipSuccess) return fail((int)e, "traj_step_draws_kernel: hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
        attr_set[variant][ntt] = true;
    }
    SD_LAUNCH(fn, dim3((unsigned)B), dim3(tj::NTHREADS), (size_t)tj::LDS_BYTES, st, a, pin ? *pin : PinArgs{nullptr, nullptr, nullptr}, draws);
    SD_CHECK_LAUNCH("traj_step_draws_kernel");
    return 0;
}

// DDIM steps i0 .. i0 + n - 1 in ONE launch of the shared rollout kernel (traj_steps_fused with the context index b / draws)
int traj_steps_fused_draws(const sd_denoiser_weights *w, const TrajWs &s, float *x, int B, int T, int Mc, int i0, int n, int n_steps, const float *coef,
                           hipStream_t st, bool precise, int32_t *status, int draws) {
    static_assert(sizeof(tj::RolloutDrawsArgs) <= 4096, "kernel argument");
    if (draws < 2 || B % draws) return fail(SD_E_BADARG, "traj_step_rollout_draws_kernel: B must be a multiple of draws >= 2");
    if (n < 1 || n > tj::ROLL_MAX_STEPS || i0 < 0 || i0 + n > n_steps || !coef) return fail(SD_E_BADARG, "traj_step_rollout_draws_kernel: bad step range");
    tj::RolloutDrawsArgs da{};
    da.draws = draws;
    da.ra.a = traj_step_args(w, s, x, nullptr, B, T, Mc, i0, n_steps, coef + 4 * i0, false, 1, status, B / draws);
    tj::RollArgs &r = da.ra.r;
    r.n_steps = n;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 4; ++k) r.coef[i][k] = coef[4 * (i0 + i) + k];
    const int ntt = (T + 15) / 16;
    const TrajRolloutDrawsFn fn = precise ? traj_rollout_draws_fn<true>(ntt) : traj_rollout_draws_fn<false>(ntt);
    if (!fn) return fail(SD_E_BADARG, "traj_step_rollout_draws_kernel: horizon out of range");
    ProfScope prof(SD_KCLASS_TRAJ_STEP, st);
    static DevFlag attr_set[2][8];
    if (!attr_set[precise ? 1 : 0][ntt]) {
        const hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, tj::LDS_BYTES);
        if (e != hipSuccess) return fail((int)e, "traj_step_rollout_draws_kernel: hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
        attr_set[precise ? 1 : 0][ntt] = true;
    }
    SD_LAUNCH(fn, dim3((unsigned)B), dim3(tj::NTHREADS), (size_t)tj::LDS_BYTES, st, da);
    SD_CHECK_LAUNCH("traj_step_rollout_draws_kernel");
    return 0;
}
