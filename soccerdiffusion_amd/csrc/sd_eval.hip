// Held-out evaluation: the two reductions behind soccerdiffusion_amd/evaluation.py (interface: include/soccerdiffusion_hip.h,
// sd_eval_sqerr_rows and sd_eval_trajectory_errors).  The tensors are kilobytes and the work is launch-bound: one launch and one definition
// of each quantity instead of a dozen framework launches is all these kernels are for.
//
// Arithmetic: fp32, contraction off (every product, sum and difference rounds on its own), no atomics, and every sum in a fixed order that
// depends on the shape alone - two runs agree bit for bit.  The orders:
//
//   sd_eval_sqerr_rows, one workgroup of four waves per row: thread t (0 .. 255) sums (a[i] - b[i])^2 over i = t, t + 256, ... in that order;
//   the 64 lanes of a wave meet in the xor butterfly 32, 16, .. 1 (every lane ends with the same bits); the four wave sums are added
//   ((w0 + w1) + w2) + w3; one division by `per`.
//
//   sd_eval_trajectory_errors, one workgroup of four waves per context, wave w owns draws w, w + 4, ...  A draw is walked two rows at a time:
//   lanes 0 .. 31 hold joints 0 .. 31 of row 2 p, lanes 32 .. 63 those of row 2 p + 1 (d^2, or 0 beyond J and T).
//     row sum   = xor butterfly 16, 8, .. 1 inside each half of the wave;             row_err = row sum / J
//     joint sum = lane j adds its rows 0, 2, 4, ... (lane 32 + j: 1, 3, 5, ...) in that order, then even + odd (xor 32);
//                                                                                     joint_err = joint sum / T
//     draw sum  = each half adds its row sums in row order (0, 2, 4, ... and 1, 3, 5, ...; 0 for a row beyond T), then even + odd (xor 32);
//                                                                                     err = draw sum / (T J)
//     best      = the lowest g among the smallest err[c][g], a scan g = 0 .. G - 1 by one thread.
#include "../../include/soccerdiffusion_hip.h"
#include "sd_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace ev {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_G = 64, MAX_J = 32;

__device__ __forceinline__ float butterfly(float v, int from) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        if (o <= from) v = v + __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(THREADS) void sqerr_rows_kernel(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ out,
                                                               long per) {
    __shared__ float part[WAVES];
    const long r = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float *ar = a + r * per, *br = b + r * per;
    float acc = 0.f;
    for (long i = threadIdx.x; i < per; i += THREADS) {
        const float d = ar[i] - br[i];
        acc = acc + d * d;
    }
    acc = butterfly(acc, 32);
    if (lane == 0) part[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[r] = (((part[0] + part[1]) + part[2]) + part[3]) / (float)per;
}

// the error of one element: denormalise as sd_session.hip's commit does (x std + mean, two roundings), subtract the target, and - angular -
// take the representative of the difference modulo 2 pi that lies in [-pi, pi]
__device__ __forceinline__ float element_error(float x, float sd, float mu, float target, int angular) {
    const float two_pi = (float)(2.0 * M_PI);
    float d = (x * sd + mu) - target;
    if (angular) d = d - two_pi * rintf(d / two_pi);
    return d;
}

__global__ __launch_bounds__(THREADS) void trajectory_errors_kernel(const float *__restrict__ x, const float *__restrict__ target,
                                                                      const float *__restrict__ mean, const float *__restrict__ stdv,
                                                                      float *__restrict__ err, float *__restrict__ row_err,
                                                                      float *__restrict__ joint_err, int32_t *__restrict__ best, int G, int T, int J,
                                                                      int angular) {
    __shared__ float errs[MAX_G];
    const long c = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = lane & 31, half = lane >> 5;
    const float *tc = target + c * (long)T * J;
    const float sd = j < J ? stdv[j] : 0.f, mu = j < J ? mean[j] : 0.f;
    for (int g = wv; g < G; g += WAVES) {   // wave-uniform
        const long cg = c * G + g;
        const float *xg = x + cg * (long)T * J;
        float joint = 0.f, total = 0.f;
        for (int t0 = 0; t0 < T; t0 += 2) {
            const int t = t0 + half;
            float sq = 0.f;
            if (t < T && j < J) {
                const float d = element_error(xg[t * J + j], sd, mu, tc[t * J + j], angular);
                sq = d * d;
            }
            joint = joint + sq;
            const float rs = butterfly(sq, 16);
            total = total + rs;
            if (row_err && j == 0 && t < T) row_err[cg * T + t] = rs / (float)J;
        }
        joint = joint + __shfl_xor(joint, 32, 64);
        if (joint_err && lane < J) joint_err[cg * J + lane] = joint / (float)T;
        total = total + __shfl_xor(total, 32, 64);
        const float e = total / (float)(T * J);
        if (lane == 0) {
            errs[g] = e;
            err[cg] = e;
        }
    }
    __syncthreads();
    if (best && threadIdx.x == 0) {
        int bi = 0;
        float be = errs[0];
        for (int g = 1; g < G; ++g)
            if (errs[g] < be) {
                be = errs[g];
                bi = g;
            }
        best[c] = bi;
    }
}

// The largest step between consecutive rows of every trajectory, per joint: out[n][j] = max_t |r[t + 1] - r[t]| with r = x std + mean (the
// commit's denormalisation, two roundings; a constant shift such as the published - pi changes no difference beyond its rounding).  One
// thread per (trajectory, joint) walks the rows in order; a maximum has no order to fix.  T == 1: 0.  A NaN difference is skipped by fmaxf.
__global__ void max_step_kernel(const float *__restrict__ x, const float *__restrict__ mean, const float *__restrict__ stdv, float *__restrict__ out,
                                long N, int T, int J) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * J) return;
    const long n = i / J;
    const int j = (int)(i - n * J);
    const float sd = stdv[j], mu = mean[j];
    const float *xn = x + n * (long)T * J + j;
    float prev = xn[0] * sd + mu, worst = 0.f;
    for (int t = 1; t < T; ++t) {
        const float cur = xn[(long)t * J] * sd + mu;
        worst = fmaxf(worst, fabsf(cur - prev));
        prev = cur;
    }
    out[i] = worst;
}

// The largest second difference of consecutive rows of every trajectory, per joint: out[n][j] = max_t |(r[t + 1] - r[t]) - (r[t] - r[t - 1])|
// with r = x std + mean as in max_step_kernel - three subtractions in fp32, one rounding each, in that order.  One thread per (trajectory,
// joint) walks the rows in order; a maximum has no order to fix, so two runs agree bit for bit.  T <= 2: 0.  A NaN is skipped by fmaxf.
__global__ void max_accel_kernel(const float *__restrict__ x, const float *__restrict__ mean, const float *__restrict__ stdv, float *__restrict__ out,
                                 long N, int T, int J) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * J) return;
    const long n = i / J;
    const int j = (int)(i - n * J);
    const float sd = stdv[j], mu = mean[j];
    const float *xn = x + n * (long)T * J + j;
    float worst = 0.f;
    if (T >= 3) {
        float p2 = xn[0] * sd + mu, p1 = xn[J] * sd + mu;
        for (int t = 2; t < T; ++t) {
            const float cur = xn[(long)t * J] * sd + mu;
            worst = fmaxf(worst, fabsf((cur - p1) - (p1 - p2)));
            p2 = p1;
            p1 = cur;
        }
    }
    out[i] = worst;
}

}   // namespace ev

extern "C" int sd_max_accel(const float *x, const float *mean, const float *stdv, float *out, long N, int T, int J, void *stream) {
    if (!x || !mean || !stdv || !out || N <= 0 || T < 1 || J < 1 || J > ev::MAX_J || N * J > 0x7fffffffL * 256)
        return fail(SD_E_BADARG, "sd_max_accel: x, mean, std and out must be given; N > 0, T >= 1, 1 <= J <= 32");
    SD_LAUNCH(ev::max_accel_kernel, dim3((unsigned)((N * J + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, mean, stdv, out, N, T, J);
    SD_CHECK_LAUNCH("max_accel_kernel");
    return 0;
}

extern "C" int sd_eval_max_step(const float *x, const float *mean, const float *stdv, float *out, long N, int T, int J, void *stream) {
    if (!x || !mean || !stdv || !out || N <= 0 || T < 1 || J < 1 || J > ev::MAX_J || N * J > 0x7fffffffL * 256)
        return fail(SD_E_BADARG, "sd_eval_max_step: x, mean, std and out must be given; N > 0, T >= 1, 1 <= J <= 32");
    SD_LAUNCH(ev::max_step_kernel, dim3((unsigned)((N * J + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, mean, stdv, out, N, T, J);
    SD_CHECK_LAUNCH("max_step_kernel");
    return 0;
}

extern "C" int sd_eval_sqerr_rows(const float *a, const float *b, float *out, long rows, long per, void *stream) {
    if (!a || !b || !out || rows <= 0 || rows > 0x7fffffffL || per <= 0)
        return fail(SD_E_BADARG, "sd_eval_sqerr_rows: a, b and out must be given; 0 < rows < 2^31, per > 0");
    SD_LAUNCH(ev::sqerr_rows_kernel, dim3((unsigned)rows), dim3(ev::THREADS), 0, (hipStream_t)stream, a, b, out, per);
    SD_CHECK_LAUNCH("sqerr_rows_kernel");
    return 0;
}

extern "C" int sd_eval_trajectory_errors(const float *x, const float *target, const float *mean, const float *stdv, float *err, float *row_err,
                                         float *joint_err, int32_t *best, int C, int G, int T, int J, int angular, void *stream) {
    if (!x || !target || !mean || !stdv || !err || C <= 0 || G < 1 || G > ev::MAX_G || T < 1 || (long)T * J > (1L << 30) || J < 1 || J > ev::MAX_J)
        return fail(SD_E_BADARG, "sd_eval_trajectory_errors: x, target, mean, std and err must be given; C > 0, 1 <= G <= 64, T >= 1, "
                                 "1 <= J <= 32");
    SD_LAUNCH(ev::trajectory_errors_kernel, dim3((unsigned)C), dim3(ev::THREADS), 0, (hipStream_t)stream, x, target, mean, stdv, err, row_err, joint_err,
              best, G, T, J, angular);
    SD_CHECK_LAUNCH("trajectory_errors_kernel");
    return 0;
}
