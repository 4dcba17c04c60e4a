// Closed-loop policy session: the buffer work of the receding-horizon tick (soccer_diffusion/ml/inference/ros.py:165-335) on the device.
// Interface, ring layout and citations: include/soccerdiffusion_hip.h (sd_ring_push, sd_ring_window, sd_session_windows, sd_session_commit,
// their *_at forms for a subset of the robots, sd_ring_push_quat, sd_session_reset, and sd_session_commit_carry(_at) / sd_session_reset_carry for a
// session whose ticks overlap, and sd_session_hold / sd_session_hold_mask for a session that holds chosen joints inside the rollout).
//
// ros.py keeps every sensor stream as a Python list of CPU tensors (append, then trim to the context length: ros.py:203,256-257,316-318)
// and stacks + uploads every list at every tick (ros.py:265-275).  Here a stream is a ring (B, L, C) in device memory with one head word per
// robot's ring: head = index of the oldest row = where the next row goes.  One workgroup owns one robot's ring: every thread reads the head,
// the rows are written, and after a barrier thread 0 moves the head - nothing else in the launch reads it, so no atomics are needed.  Every
// index is reduced mod L before it addresses memory: a head word that was overwritten by something else cannot send a store out of the ring.
//
// Which robot a workgroup owns: robot blockIdx.x, or robots[blockIdx.x] where the launch names a subset (the *_at entry points); the caller's
// arrays (src, x, out) are then compact, one block per named robot.  A name outside [0, B) makes its workgroup return before any store.
//
// Arithmetic: contraction is off in this file.  The wrap and the published trajectory are compared bit for bit with torch's CPU expressions,
// which round every product, sum and difference on its own.
#include "../../include/soccerdiffusion_hip.h"
#include "sd_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace ss {

constexpr int THREADS = 256;

// the robot of workgroup s, or -1 (no store) where the subset names a robot that does not exist; the same in every thread of the workgroup
__device__ __forceinline__ int robot_of(const int32_t *robots, int s, int B) {
    const int b = robots ? robots[s] : s;
    return (unsigned)b < (unsigned)B ? b : -1;
}

__device__ __forceinline__ int head_of(const int32_t *head, int b, int L) {
    const int h = head[b] % L;
    return h < 0 ? h + L : h;
}

// (x + 3 * np.pi) % (2 * np.pi) of ros.py:266-273 on an fp32 tensor: the Python doubles 3 pi and 2 pi become fp32 scalars, the sum is
// one rounded fp32 addition, and torch's remainder is fmod (exact) with the divisor added where the result is non-zero and negative
__device__ __forceinline__ float wrap_angle(float x) {
    const float three_pi = (float)(3.0 * M_PI), two_pi = (float)(2.0 * M_PI);
    const float a = x + three_pi;
    float r = fmodf(a, two_pi);
    if (r != 0.f && r < 0.f) r = r + two_pi;
    return r;
}

// rows [max(0, n - L), n) of a robot's n new rows go to ring rows (h + r) % L: L consecutive r never share a row
template <typename F>
__device__ __forceinline__ void push_rows(float *ring, int h, int L, int C, int n, F value) {
    const int r0 = n > L ? n - L : 0;
    const int count = (n - r0) * C;
    for (int i = threadIdx.x; i < count; i += THREADS) {
        const int r = r0 + i / C, c = i % C;
        ring[(long)((h + r) % L) * C + c] = value(r, c);
    }
}

__global__ __launch_bounds__(THREADS) void ring_push_kernel(float *ring, int32_t *head, const float *__restrict__ src, const float *__restrict__ sub,
                                                            const int32_t *__restrict__ robots, int B, int L, int C, int n) {
    const int b = robot_of(robots, blockIdx.x, B);
    if (b < 0) return;
    const int h = head_of(head, b, L);
    const float *s = src + (long)blockIdx.x * n * C;
    push_rows(ring + (long)b * L * C, h, L, C, n, [&](int r, int c) {
        const float v = s[(long)r * C + c];
        return sub ? v - sub[c] : v;
    });
    __syncthreads();                           // every thread has read the head
    if (threadIdx.x == 0) head[b] = (h + n % L) % L;
}

// dataset.quats_to_5d (soccer_diffusion/utils/utils.py:9-24 with transforms3d's quat2axangle) of one xyzw quaternion: (axis xyz, sin angle,
// cos angle), in fp64 with numpy's operations in numpy's order - contraction is off - and one rounding to fp32 per value
__device__ __forceinline__ void quat_to_5d(const float *q, float *row) {
    double x = q[0], y = q[1], z = q[2], w = q[3];
    const double eps = 2.220446049250313e-16;                  // np.finfo(np.float64).eps
    const double nq = w * w + x * x + y * y + z * z;
    const bool tiny = nq < eps * eps;
    const double s = sqrt(tiny ? 1.0 : nq);
    w = w / s; x = x / s; y = y / s; z = z / s;
    const double len2 = x * x + y * y + z * z;
    const bool ident = tiny || len2 < (3 * eps) * (3 * eps);
    const double theta = ident ? 0.0 : 2 * acos(fmin(fmax(w, -1.0), 1.0));
    const double inv = 1.0 / sqrt(ident ? 1.0 : len2);
    row[0] = ident ? 1.f : (float)(x * inv);
    row[1] = ident ? 0.f : (float)(y * inv);
    row[2] = ident ? 0.f : (float)(z * inv);
    row[3] = (float)sin(theta);
    row[4] = (float)cos(theta);
}

// quats (S, n, 4) xyzw -> the rotation ring (B, L, C): C == 4 the rows as they are, C == 5 quat_to_5d of them; a thread owns whole rows
__global__ __launch_bounds__(THREADS) void ring_push_quat_kernel(float *ring, int32_t *head, const float *__restrict__ quats,
                                                                 const int32_t *__restrict__ robots, int B, int L, int C, int n) {
    const int b = robot_of(robots, blockIdx.x, B);
    if (b < 0) return;
    const int h = head_of(head, b, L);
    const float *q = quats + (long)blockIdx.x * n * 4;
    float *rb = ring + (long)b * L * C;
    for (int r = (n > L ? n - L : 0) + threadIdx.x; r < n; r += THREADS) {   // (as push_rows: with n > L only the last L rows)
        float *row = rb + (long)((h + r) % L) * C;
        if (C == 5) {
            quat_to_5d(q + (long)r * 4, row);
        } else {
            for (int c = 0; c < 4; ++c) row[c] = q[(long)r * 4 + c];
        }
    }
    __syncthreads();                           // every thread has read the head
    if (threadIdx.x == 0) head[b] = (h + n % L) % L;
}

struct Views {
    sd_ring_view v[SD_SESSION_MAX_RINGS];
    const int32_t *robots;
    int B;
};

// grid (S, n_views): chronological row i of robot b = ring row (head + i) % L; 16-byte pieces where the rows allow it
__global__ __launch_bounds__(THREADS) void ring_windows_kernel(Views a) {
    const sd_ring_view v = a.v[blockIdx.y];
    const int b = robot_of(a.robots, blockIdx.x, a.B), L = v.L, C = v.C;
    if (b < 0) return;
    const int h = head_of(v.head, b, L);
    const float *ring = v.ring + (long)b * L * C;
    float *out = v.out + (long)blockIdx.x * L * C;
    const bool vec = (C & 3) == 0 && !v.wrap && ((reinterpret_cast<uintptr_t>(v.ring) | reinterpret_cast<uintptr_t>(v.out)) & 15) == 0;
    if (vec) {
        const int C4 = C >> 2;
        for (int i = threadIdx.x; i < L * C4; i += THREADS) {
            const int r = i / C4, c = i - r * C4;
            reinterpret_cast<f32x4 *>(out)[i] = reinterpret_cast<const f32x4 *>(ring + (long)((h + r) % L) * C)[c];
        }
        return;
    }
    for (int i = threadIdx.x; i < L * C; i += THREADS) {
        const int r = i / C, c = i - r * C;
        const float x = ring[(long)((h + r) % L) * C + c];
        out[i] = v.wrap ? wrap_angle(x) : x;
    }
}

__global__ __launch_bounds__(THREADS) void session_commit_kernel(const float *x, const float *__restrict__ mean,
                                                                 const float *__restrict__ stdv, float *out, float *ring,
                                                                 int32_t *head, const int32_t *__restrict__ robots, int B, int T, int J,
                                                                 int L) {
    const int b = robot_of(robots, blockIdx.x, B);
    if (b < 0) return;
    const int h = head_of(head, b, L);
    const float *xb = x + (long)blockIdx.x * T * J;
    float *ob = out + (long)blockIdx.x * T * J;
    float *rb = ring + (long)b * L * J;
    const float pi = (float)M_PI;
    const int r0 = T > L ? T - L : 0;          // (as push_rows: with T > L only the last L rows reach the ring)
    for (int i = threadIdx.x; i < T * J; i += THREADS) {
        const int r = i / J, c = i - r * J;
        const float v = (xb[i] * stdv[c] + mean[c]) - pi;   // denormalize, then - np.pi (ros.py:313,317,327); read once: out may be x
        ob[i] = v;
        if (r >= r0) rb[(long)((h + r) % L) * J + c] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) head[b] = (h + T % L) % L;
}

// session_commit_kernel that also prepares the next tick: all T rows are published (the same expression), the first `advance` of them - the
// commands executed before the next tick - go to the action ring, rows [advance, advance + carry) of x (normalised space, as sampled) become
// rows [0, carry) of the robot's pin_x0 block and pin_rows[robot] = carry.  x is indexed by workgroup, pin_x0 and pin_rows by robot.
__global__ __launch_bounds__(THREADS) void session_commit_carry_kernel(const float *x, const float *__restrict__ mean,
                                                                       const float *__restrict__ stdv, float *out, float *ring,
                                                                       int32_t *head, const int32_t *__restrict__ robots, int B, int T, int J,
                                                                       int L, int advance, int carry, float *pin_x0, int32_t *pin_rows) {
    const int b = robot_of(robots, blockIdx.x, B);
    if (b < 0) return;
    const int h = head_of(head, b, L);
    const float *xb = x + (long)blockIdx.x * T * J;
    float *ob = out + (long)blockIdx.x * T * J;
    float *rb = ring + (long)b * L * J;
    float *pb = pin_x0 + (long)b * T * J;
    const float pi = (float)M_PI;
    const int r0 = advance > L ? advance - L : 0;   // (as push_rows: with advance > L only the last L rows reach the ring)
    for (int i = threadIdx.x; i < T * J; i += THREADS) {
        const int r = i / J, c = i - r * J;
        const float xv = xb[i];                             // read once: out may be x
        const float v = (xv * stdv[c] + mean[c]) - pi;
        ob[i] = v;
        if (r >= r0 && r < advance) rb[(long)((h + r) % L) * J + c] = v;
        if (r >= advance && r < advance + carry) pb[i - advance * J] = xv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        head[b] = (h + advance % L) % L;
        pin_rows[b] = carry;
    }
}

static int launch_windows(const Views &a, int n_views, int S, hipStream_t st) {
    SD_LAUNCH(ring_windows_kernel, dim3((unsigned)S, (unsigned)n_views), dim3(THREADS), 0, st, a);
    SD_CHECK_LAUNCH("ring_windows_kernel");
    return 0;
}

struct Resets {
    sd_ring_reset r[SD_SESSION_MAX_RESET_RINGS];
};

// grid (B, n_rings): a selected robot's ring back to L rows of fill (zeros without one) and its head to 0; ring 0's workgroup also writes the
// robot's game state.  The mask is read, never the head: a reset does not depend on what the head word holds.
__global__ __launch_bounds__(THREADS) void session_reset_kernel(Resets a, const uint8_t *__restrict__ mask, int64_t *game_state,
                                                                int64_t game_state_value) {
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;
    const sd_ring_reset r = a.r[blockIdx.y];
    const int L = r.L, C = r.C;
    float *ring = r.ring + (long)b * L * C;
    for (int i = threadIdx.x; i < L * C; i += THREADS) ring[i] = r.fill ? r.fill[i % C] : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
        r.head[b] = 0;
        if (blockIdx.y == 0 && game_state) game_state[b] = game_state_value;
    }
}

// session_reset_kernel for a session with carry: ring 0's workgroup also zeroes the robot's pin_rows word - its next tick is unpinned
__global__ __launch_bounds__(THREADS) void session_reset_carry_kernel(Resets a, const uint8_t *__restrict__ mask, int64_t *game_state,
                                                                      int64_t game_state_value, int32_t *pin_rows) {
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;
    const sd_ring_reset r = a.r[blockIdx.y];
    const int L = r.L, C = r.C;
    float *ring = r.ring + (long)b * L * C;
    for (int i = threadIdx.x; i < L * C; i += THREADS) ring[i] = r.fill ? r.fill[i % C] : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
        r.head[b] = 0;
        if (blockIdx.y == 0) {
            pin_rows[b] = 0;
            if (game_state) game_state[b] = game_state_value;
        }
    }
}

// ---- held joints (PolicySession(holds=True): sd_ddim_sample_hold's mask and known values, kept per robot) ------------------------------
struct HoldJoints {   // the joints of one hold / release call, by value in the kernel argument: J <= 32
    int n;
    int j[32];
};

// One workgroup per selected robot.  set: values[s][t][k] (radians as published; robot and row strides, 0 = broadcast) of joint j[k] go,
// normalised - ((v + pi) - mean[j]) / std[j], the inverse of the commit's expression, every operation rounded on its own - to
// pin_x0[b][t][j] for all T rows, and the joints' bits are set in held[b]; else the bits are cleared and pin_x0 stays.  One thread
// moves the robot's word: no atomics.
__global__ __launch_bounds__(THREADS) void session_hold_kernel(float *pin_x0, int32_t *held, const float *__restrict__ values, long stride_robot,
                                                               long stride_row, HoldJoints hj, const float *__restrict__ mean,
                                                               const float *__restrict__ stdv, const int32_t *__restrict__ robots, int B, int T,
                                                               int J, int set) {
    const int b = robot_of(robots, blockIdx.x, B);
    if (b < 0) return;
    const float pi = (float)M_PI;
    unsigned bits = 0;
    for (int k = 0; k < hj.n; ++k)
        if ((unsigned)hj.j[k] < (unsigned)J) bits |= 1u << hj.j[k];
    if (set) {
        const float *vb = values + (long)blockIdx.x * stride_robot;
        float *pb = pin_x0 + (long)b * T * J;
        for (int i = threadIdx.x; i < T * hj.n; i += THREADS) {
            const int t = i / hj.n, k = i - t * hj.n, j = hj.j[k];
            if ((unsigned)j >= (unsigned)J) continue;
            pb[t * J + j] = ((vb[(long)t * stride_row + k] + pi) - mean[j]) / stdv[j];
        }
    }
    if (threadIdx.x == 0) held[b] = (int32_t)(set ? ((unsigned)held[b] | bits) : ((unsigned)held[b] & ~bits));
}

// ---- joint limits (PolicySession(limits=...): sd_ddim_sample_limits' lo / hi, from radians as published) -------------------------------
struct SessionLimits {   // the limits of one set_limits call in radians, by value in the kernel argument: J <= 32
    float lo[32], hi[32];
};
// both roundings of the commit's expression (session_commit_kernel's line, which a compiler is free to contract).  Plain operators: it is
// this file's pragma that keeps them apart - the __fmul_rn / __fadd_rn wrappers are compiled under the header's contraction and fuse.
static __device__ __forceinline__ float commit_fused(float x, float s, float m) { return __builtin_fmaf(x, s, m) - (float)M_PI; }
static __device__ __forceinline__ float commit_plain(float x, float s, float m) { return (x * s + m) - (float)M_PI; }
// One thread per slot of the 32-float arrays.  Joint j < J: the bound in normalised space begins as the inverse of the commit's expression,
// ((v + pi) - mean[j]) / std[j], and moves inward - by nextafterf, or by a quarter ulp of the commit's largest intermediate in normalised
// units where that is more (x near 0 has ulps far below the published value's), 64 tries at most (measured on the host: 5) - until both
// roundings of the commit's expression give a value inside [lo, hi].  The commit is monotonic in x (std > 0), so every x0 clamped to the
// result is published inside the radians bit for bit.  An infinite bound stays infinite.  A range narrower than the commit's resolution
// collapses to its upper bound.  Slots >= J: -inf / +inf.
__global__ void session_limits_kernel(float *lo_n, float *hi_n, SessionLimits rad, const float *__restrict__ mean, const float *__restrict__ stdv,
                                      int J) {
    const int j = threadIdx.x;
    if (j >= 32) return;
    float lo = -INFINITY, hi = INFINITY;
    if (j < J) {
        const float pi = (float)M_PI, m = mean[j], s = stdv[j];
        const float rl = rad.lo[j], rh = rad.hi[j];
        if (rl > -INFINITY) {
            const float big = fmaxf(fmaxf(fabsf(rl + pi), fabsf(m)), fabsf(rl));
            const float q = (nextafterf(big, INFINITY) - big) * 0.25f / s;
            lo = ((rl + pi) - m) / s;
            for (int k = 0; k < 64 && !(commit_fused(lo, s, m) >= rl && commit_plain(lo, s, m) >= rl); ++k)
                lo = fmaxf(nextafterf(lo, INFINITY), lo + q);
        }
        if (rh < INFINITY) {
            const float big = fmaxf(fmaxf(fabsf(rh + pi), fabsf(m)), fabsf(rh));
            const float q = (nextafterf(big, INFINITY) - big) * 0.25f / s;
            hi = ((rh + pi) - m) / s;
            for (int k = 0; k < 64 && !(commit_fused(hi, s, m) <= rh && commit_plain(hi, s, m) <= rh); ++k)
                hi = fminf(nextafterf(hi, -INFINITY), hi - q);
        }
        if (lo > hi) lo = hi;
    }
    lo_n[j] = lo;
    hi_n[j] = hi;
}

// ---- slew limits (PolicySession(slew=...): sd_ddim_sample_slew's v, from radians per row as published) ---------------------------------
struct SessionSlew {   // one set_slew call by value: v in radians per row, and the bound R[j] on |published value| of joint j
    float v[32], r[32];
};
// half an ulp of the fp32 binade of z (1 + 2^-20): the most one rounding to nearest adds to a result of magnitude <= z
__device__ __forceinline__ double half_ulp(double z) { return z > 0.0 ? ldexp(1.0, ilogb(z * (1.0 + 9.5367431640625e-07)) - 24) : 0.0; }
// One thread per slot.  v_n = (v_rad - margin) / std, rounded toward zero, with
//   margin = std hu(XS / std) + 2 hu(XS) + 2 hu(pi + R) + 2 hu(R),   XS = R + |pi - mean|,   hu = half_ulp
// in fp64 (DESIGN.md 5.7.4 derives it): consecutive rows of the rollout differ by at most fl(y + v_n) - y <= v_n + hu(|x|) in normalised
// space, |x| <= XS / std; the commit multiplies that by std and adds up to three roundings per published value in its plain form (x * std,
// + mean, - pi: two in the fused form), each half an ulp of its result: |x std| <= XS, |x std + mean| <= R + pi, |published| <= R.  So the fp32 values the commit
// publishes differ by at most v_rad, evaluated exactly.  A v_rad of +inf stays +inf; one not above its margin gives 0 (the host refuses
// it before the launch).  Slots >= J: +inf.
__global__ void session_slew_kernel(float *v_n, SessionSlew rad, const float *__restrict__ mean, const float *__restrict__ stdv, int J) {
    const int j = threadIdx.x;
    if (j >= 32) return;
    float out = INFINITY;
    if (j < J && rad.v[j] < INFINITY) {
        const double s = (double)stdv[j], R = (double)rad.r[j], XS = R + fabs(M_PI - (double)mean[j]);
        const double margin = s * half_ulp(XS / s) + 2.0 * half_ulp(XS) + 2.0 * half_ulp(M_PI + R) + 2.0 * half_ulp(R);
        const double v = ((double)rad.v[j] - margin) / s;
        out = v > 0.0 ? (float)v : 0.f;
        if ((double)out > v) out = nextafterf(out, 0.f);
    }
    v_n[j] = out;
}
// The anchor of the next tick's scan: anchor[(b * draws + g)][j] = x[s][row][j] for robot b = robots[s] (NULL: s) and every draw g, j < J -
// the last committed row of the robot's trajectory in normalised space, as sampled.  Slots [J, 32) keep their NaN.
__global__ void session_anchor_kernel(float *anchor, const float *__restrict__ x, const int32_t *__restrict__ robots, int S, int B, int T, int J,
                                      int row, int draws) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * draws * J) return;
    const int j = i % J, g = (i / J) % draws, s = i / (J * draws);
    const int b = robot_of(robots, s, B);
    if (b < 0) return;
    anchor[((long)b * draws + g) * 32 + j] = x[((long)s * T + row) * J + j];
}

// ---- acceleration limits (sd_ddim_sample_accel's a, from radians per row^2 as published) ----------------------------------------------
// One thread per slot.  a_n = (a_rad - margin) / std, rounded toward zero, with
//   margin = 4 std hu(3 XS / std) + 4 hu(XS) + 4 hu(pi + R) + 4 hu(R),   XS = R + |pi - mean|,   hu = half_ulp
// in fp64 (DESIGN.md 5.7.6 derives it): a row of the scan lies within a_n of 2 y1 - y2 up to the four roundings of accel_row (d, p,
// p - a, p + a), each half an ulp of a result of magnitude <= 3 XS / std, since |x| <= XS / std inside the box; the commit multiplies by
// std and adds up to three roundings per published value (x * std, + mean, - pi; |x std| <= XS, |x std + mean| <= R + pi,
// |published| <= R), and a second difference takes three published values with weights 1, 2 and 1.  So the second difference of the
// fp32 values the commit publishes is at most a_rad, evaluated exactly.  +inf stays +inf; an a_rad not above its margin gives 0 (the
// host refuses it before the launch).  Slots >= J: +inf.
__global__ void session_accel_kernel(float *a_n, SessionSlew rad, const float *__restrict__ mean, const float *__restrict__ stdv, int J) {
    const int j = threadIdx.x;
    if (j >= 32) return;
    float out = INFINITY;
    if (j < J && rad.v[j] < INFINITY) {
        const double s = (double)stdv[j], R = (double)rad.r[j], XS = R + fabs(M_PI - (double)mean[j]);
        const double margin = 4.0 * s * half_ulp(3.0 * XS / s) + 4.0 * half_ulp(XS) + 4.0 * half_ulp(M_PI + R) + 4.0 * half_ulp(R);
        const double a = ((double)rad.v[j] - margin) / s;
        out = a > 0.0 ? (float)a : 0.f;
        if ((double)out > a) out = nextafterf(out, 0.f);
    }
    a_n[j] = out;
}
// session_anchor_kernel with a second destination, for a scan whose state is two rows: per robot b = robots[s] (NULL: s), draw g and
// joint j < J,  anchor2 <- row >= 1 ? x[s][row - 1][j] : the old anchor;  anchor <- x[s][row][j]  (row = advance - 1).  One thread reads
// the old anchor before it writes either destination, and no other thread touches its two slots.  Slots [J, 32) keep their NaN.
__global__ void session_anchor2_kernel(float *anchor, float *anchor2, const float *__restrict__ x, const int32_t *__restrict__ robots, int S, int B, int T,
                                       int J, int row, int draws) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * draws * J) return;
    const int j = i % J, g = (i / J) % draws, s = i / (J * draws);
    const int b = robot_of(robots, s, B);
    if (b < 0) return;
    const long at = ((long)b * draws + g) * 32 + j;
    const float old = anchor[at];
    anchor2[at] = row >= 1 ? x[((long)s * T + row - 1) * J + j] : old;
    anchor[at] = x[((long)s * T + row) * J + j];
}

// The tick's mask: mask[s * draws + g][t] = held[b] | (t < pin_rows[b] ? all J bits : 0), b = robot s of the launch (robots NULL: s);
// pin_rows NULL: a session without carried rows.  n = S * draws * T words.
__global__ __launch_bounds__(THREADS) void session_hold_mask_kernel(int32_t *__restrict__ mask, const int32_t *__restrict__ held,
                                                                    const int32_t *__restrict__ pin_rows, const int32_t *__restrict__ robots,
                                                                    int n, int B, int T, int J, int draws) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int row = i / T, t = i - row * T;
    const int b = robot_of(robots, row / draws, B);
    if (b < 0) return;
    const unsigned all = J >= 32 ? 0xffffffffu : (1u << J) - 1u;
    mask[i] = (int32_t)(((unsigned)held[b] & all) | ((pin_rows && t < pin_rows[b]) ? all : 0u));
}

}   // namespace ss

static bool dims_ok(int B, int L, int C) { return B > 0 && L > 0 && C > 0 && (long)L * C <= 0x7fffffffL / 2; }   // (row * C + column stays an int)

extern "C" int sd_ring_push(float *ring, int32_t *head, const float *src, const float *sub, int B, int L, int C, int n, void *stream) {
    if (!ring || !head || !dims_ok(B, L, C) || n < 0 || (n > 0 && !src) || (long)n * C > 0x7fffffffL / 2)
        return fail(SD_E_BADARG, "sd_ring_push: ring, head and (for n > 0) src must be given; B, L, C > 0, n >= 0");
    if (n == 0) return 0;
    SD_LAUNCH(ss::ring_push_kernel, dim3((unsigned)B), dim3(ss::THREADS), 0, (hipStream_t)stream, ring, head, src, sub, (const int32_t *)nullptr, B, L, C,
              n);
    SD_CHECK_LAUNCH("ring_push_kernel");
    return 0;
}

extern "C" int sd_ring_push_at(float *ring, int32_t *head, const float *src, const float *sub, const int32_t *robots, int S, int B, int L, int C, int n,
                               void *stream) {
    if (!ring || !head || !dims_ok(B, L, C) || S < 0 || n < 0 || (long)n * C > 0x7fffffffL / 2 || (S > 0 && (!robots || (n > 0 && !src))))
        return fail(SD_E_BADARG, "sd_ring_push_at: ring, head and (for S, n > 0) src and robots must be given; B, L, C > 0, S, n >= 0");
    if (S == 0 || n == 0) return 0;
    SD_LAUNCH(ss::ring_push_kernel, dim3((unsigned)S), dim3(ss::THREADS), 0, (hipStream_t)stream, ring, head, src, sub, robots, B, L, C, n);
    SD_CHECK_LAUNCH("ring_push_kernel");
    return 0;
}

extern "C" int sd_ring_push_quat(float *ring, int32_t *head, const float *quats, const int32_t *robots, int S, int B, int L, int C, int n,
                                 void *stream) {
    if (!ring || !head || !dims_ok(B, L, C) || (C != 4 && C != 5) || S < 0 || n < 0 || (long)n * 5 > 0x7fffffffL / 2 || (!robots && S != B) ||
        (S > 0 && n > 0 && !quats))
        return fail(SD_E_BADARG, "sd_ring_push_quat: ring, head and (for S, n > 0) quats must be given; B, L > 0, C = 4 or 5, S, n >= 0, S = B "
                                 "without robots");
    if (S == 0 || n == 0) return 0;
    SD_LAUNCH(ss::ring_push_quat_kernel, dim3((unsigned)S), dim3(ss::THREADS), 0, (hipStream_t)stream, ring, head, quats, robots, B, L, C, n);
    SD_CHECK_LAUNCH("ring_push_quat_kernel");
    return 0;
}

extern "C" int sd_ring_window(const float *ring, const int32_t *head, float *out, int B, int L, int C, void *stream) {
    if (!ring || !head || !out || !dims_ok(B, L, C)) return fail(SD_E_BADARG, "sd_ring_window: ring, head and out must be given; B, L, C > 0");
    ss::Views a{};
    a.v[0].ring = ring; a.v[0].head = head; a.v[0].out = out; a.v[0].L = L; a.v[0].C = C;
    a.B = B;
    return ss::launch_windows(a, 1, B, (hipStream_t)stream);
}

extern "C" int sd_ring_window_at(const float *ring, const int32_t *head, float *out, const int32_t *robots, int S, int B, int L, int C, void *stream) {
    if (!ring || !head || !dims_ok(B, L, C) || S < 0 || (S > 0 && (!out || !robots)))
        return fail(SD_E_BADARG, "sd_ring_window_at: ring, head and (for S > 0) out and robots must be given; B, L, C > 0, S >= 0");
    if (S == 0) return 0;
    ss::Views a{};
    a.v[0].ring = ring; a.v[0].head = head; a.v[0].out = out; a.v[0].L = L; a.v[0].C = C;
    a.robots = robots; a.B = B;
    return ss::launch_windows(a, 1, S, (hipStream_t)stream);
}

extern "C" int sd_session_windows(const sd_ring_view *views, int n_views, int B, void *stream) {
    if (!views || n_views < 1 || n_views > SD_SESSION_MAX_RINGS || B <= 0)
        return fail(SD_E_BADARG, "sd_session_windows: 1 .. 3 views and B > 0");
    ss::Views a{};
    for (int i = 0; i < n_views; ++i) {
        if (!views[i].ring || !views[i].head || !views[i].out || !dims_ok(B, views[i].L, views[i].C))
            return fail(SD_E_BADARG, "sd_session_windows: every view needs ring, head and out; L, C > 0");
        a.v[i] = views[i];
    }
    a.B = B;
    return ss::launch_windows(a, n_views, B, (hipStream_t)stream);
}

extern "C" int sd_session_windows_at(const sd_ring_view *views, int n_views, const int32_t *robots, int S, int B, void *stream) {
    if (!views || n_views < 1 || n_views > SD_SESSION_MAX_RINGS || B <= 0 || S < 0 || (S > 0 && !robots))
        return fail(SD_E_BADARG, "sd_session_windows_at: 1 .. 3 views, B > 0, S >= 0 and (for S > 0) robots");
    ss::Views a{};
    for (int i = 0; i < n_views; ++i) {
        if (!views[i].ring || !views[i].head || !views[i].out || !dims_ok(B, views[i].L, views[i].C))
            return fail(SD_E_BADARG, "sd_session_windows_at: every view needs ring, head and out; L, C > 0");
        a.v[i] = views[i];
    }
    if (S == 0) return 0;
    a.robots = robots; a.B = B;
    return ss::launch_windows(a, n_views, S, (hipStream_t)stream);
}

extern "C" int sd_session_commit(const float *x, const float *mean, const float *stdv, float *out, float *ring, int32_t *head, int B, int T, int J,
                                 int L, void *stream) {
    if (!x || !mean || !stdv || !out || !ring || !head || !dims_ok(B, L, J) || !dims_ok(B, T, J))
        return fail(SD_E_BADARG, "sd_session_commit: x, mean, std, out, ring and head must be given; B, T, J, L > 0");
    SD_LAUNCH(ss::session_commit_kernel, dim3((unsigned)B), dim3(ss::THREADS), 0, (hipStream_t)stream, x, mean, stdv, out, ring, head,
              (const int32_t *)nullptr, B, T, J, L);
    SD_CHECK_LAUNCH("session_commit_kernel");
    return 0;
}

extern "C" int sd_session_commit_at(const float *x, const float *mean, const float *stdv, float *out, float *ring, int32_t *head, const int32_t *robots,
                                    int S, int B, int T, int J, int L, void *stream) {
    if (!mean || !stdv || !ring || !head || !dims_ok(B, L, J) || !dims_ok(B, T, J) || S < 0 || (S > 0 && (!x || !out || !robots)))
        return fail(SD_E_BADARG, "sd_session_commit_at: mean, std, ring, head and (for S > 0) x, out and robots must be given; B, T, J, L > 0, S >= 0");
    if (S == 0) return 0;
    SD_LAUNCH(ss::session_commit_kernel, dim3((unsigned)S), dim3(ss::THREADS), 0, (hipStream_t)stream, x, mean, stdv, out, ring, head, robots, B, T, J,
              L);
    SD_CHECK_LAUNCH("session_commit_kernel");
    return 0;
}

static bool carry_ok(int T, int advance, int carry) { return advance >= 0 && carry >= 0 && advance + carry <= T; }

extern "C" int sd_session_commit_carry(const float *x, const float *mean, const float *stdv, float *out, float *ring, int32_t *head, int B, int T,
                                       int J, int L, int advance, int carry, float *pin_x0, int32_t *pin_rows, void *stream) {
    if (!x || !mean || !stdv || !out || !ring || !head || !pin_x0 || !pin_rows || !dims_ok(B, L, J) || !dims_ok(B, T, J) || !carry_ok(T, advance, carry))
        return fail(SD_E_BADARG, "sd_session_commit_carry: x, mean, std, out, ring, head, pin_x0 and pin_rows must be given; B, T, J, L > 0, "
                                 "advance, carry >= 0, advance + carry <= T");
    SD_LAUNCH(ss::session_commit_carry_kernel, dim3((unsigned)B), dim3(ss::THREADS), 0, (hipStream_t)stream, x, mean, stdv, out, ring, head,
              (const int32_t *)nullptr, B, T, J, L, advance, carry, pin_x0, pin_rows);
    SD_CHECK_LAUNCH("session_commit_carry_kernel");
    return 0;
}

extern "C" int sd_session_commit_carry_at(const float *x, const float *mean, const float *stdv, float *out, float *ring, int32_t *head,
                                          const int32_t *robots, int S, int B, int T, int J, int L, int advance, int carry, float *pin_x0,
                                          int32_t *pin_rows, void *stream) {
    if (!mean || !stdv || !ring || !head || !pin_x0 || !pin_rows || !dims_ok(B, L, J) || !dims_ok(B, T, J) || !carry_ok(T, advance, carry) || S < 0 ||
        (S > 0 && (!x || !out || !robots)))
        return fail(SD_E_BADARG, "sd_session_commit_carry_at: mean, std, ring, head, pin_x0, pin_rows and (for S > 0) x, out and robots must be given; "
                                 "B, T, J, L > 0, S >= 0, advance, carry >= 0, advance + carry <= T");
    if (S == 0) return 0;
    SD_LAUNCH(ss::session_commit_carry_kernel, dim3((unsigned)S), dim3(ss::THREADS), 0, (hipStream_t)stream, x, mean, stdv, out, ring, head, robots, B,
              T, J, L, advance, carry, pin_x0, pin_rows);
    SD_CHECK_LAUNCH("session_commit_carry_kernel");
    return 0;
}

extern "C" int sd_session_reset_carry(const sd_ring_reset *rings, int n_rings, const uint8_t *mask, int64_t *game_state, int64_t game_state_value,
                                      int32_t *pin_rows, int B, void *stream) {
    if (!rings || n_rings < 1 || n_rings > SD_SESSION_MAX_RESET_RINGS || B <= 0 || !pin_rows)
        return fail(SD_E_BADARG, "sd_session_reset_carry: 1 .. 5 rings, pin_rows and B > 0");
    ss::Resets a{};
    for (int i = 0; i < n_rings; ++i) {
        if (!rings[i].ring || !rings[i].head || !dims_ok(B, rings[i].L, rings[i].C))
            return fail(SD_E_BADARG, "sd_session_reset_carry: every ring needs ring and head; L, C > 0");
        a.r[i] = rings[i];
    }
    SD_LAUNCH(ss::session_reset_carry_kernel, dim3((unsigned)B, (unsigned)n_rings), dim3(ss::THREADS), 0, (hipStream_t)stream, a, mask, game_state,
              game_state_value, pin_rows);
    SD_CHECK_LAUNCH("session_reset_carry_kernel");
    return 0;
}

extern "C" int sd_session_hold(float *pin_x0, int32_t *held, const float *values, int64_t stride_robot, int64_t stride_row, const int32_t *joints, int n,
                               const float *mean, const float *stdv, const int32_t *robots, int S, int B, int T, int J, int set, void *stream) {
    if (!held || !joints || n < 1 || n > 32 || J < 1 || J > 32 || !dims_ok(B, T, J) || S < 0 || (!robots && S != B))
        return fail(SD_E_BADARG, "sd_session_hold: held and joints must be given; 1 <= n <= 32, 1 <= J <= 32, B, T > 0, S >= 0, S = B without robots");
    if (set && (!pin_x0 || !values || !mean || !stdv || stride_robot < 0 || stride_row < 0))
        return fail(SD_E_BADARG, "sd_session_hold: a hold needs pin_x0, values, mean and std; strides >= 0");
    ss::HoldJoints hj{};
    hj.n = n;
    for (int k = 0; k < n; ++k) {
        if (joints[k] < 0 || joints[k] >= J) return fail(SD_E_BADARG, "sd_session_hold: joint index out of range");
        hj.j[k] = joints[k];
    }
    if (S == 0) return 0;
    SD_LAUNCH(ss::session_hold_kernel, dim3((unsigned)S), dim3(ss::THREADS), 0, (hipStream_t)stream, pin_x0, held, values, (long)stride_robot,
              (long)stride_row, hj, mean, stdv, robots, B, T, J, set ? 1 : 0);
    SD_CHECK_LAUNCH("session_hold_kernel");
    return 0;
}

extern "C" int sd_session_hold_mask(int32_t *mask, const int32_t *held, const int32_t *pin_rows, const int32_t *robots, int S, int B, int T, int J,
                                    int draws, void *stream) {
    if (!mask || !held || J < 1 || J > 32 || !dims_ok(B, T, J) || S < 0 || draws < 1 || (!robots && S != B) || (long)S * draws * T > 0x7fffffffL / 2)
        return fail(SD_E_BADARG, "sd_session_hold_mask: mask and held must be given; 1 <= J <= 32, B, T > 0, S >= 0, draws >= 1, S = B without robots");
    if (S == 0) return 0;
    const int n = S * draws * T;
    SD_LAUNCH(ss::session_hold_mask_kernel, dim3((unsigned)((n + ss::THREADS - 1) / ss::THREADS)), dim3(ss::THREADS), 0, (hipStream_t)stream, mask, held,
              pin_rows, robots, n, B, T, J, draws);
    SD_CHECK_LAUNCH("session_hold_mask_kernel");
    return 0;
}

extern "C" int sd_session_limits(float *lo_n, float *hi_n, const float *lo_rad, const float *hi_rad, const float *mean, const float *stdv, int J,
                                 void *stream) {
    if (!lo_n || !hi_n || !lo_rad || !hi_rad || !mean || !stdv || J < 1 || J > 32)
        return fail(SD_E_BADARG, "sd_session_limits: lo_n, hi_n, lo_rad, hi_rad, mean and std must be given; 1 <= J <= 32");
    ss::SessionLimits rad{};
    for (int j = 0; j < J; ++j) {
        if (!(lo_rad[j] <= hi_rad[j])) return fail(SD_E_BADARG, "sd_session_limits: lo[j] <= hi[j], no NaN");
        rad.lo[j] = lo_rad[j];
        rad.hi[j] = hi_rad[j];
    }
    SD_LAUNCH(ss::session_limits_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, lo_n, hi_n, rad, mean, stdv, J);
    SD_CHECK_LAUNCH("session_limits_kernel");
    return 0;
}

extern "C" int sd_session_slew(float *v_n, const float *v_rad, const float *bound_rad, const float *mean, const float *stdv, int J, void *stream) {
    if (!v_n || !v_rad || !bound_rad || !mean || !stdv || J < 1 || J > 32)
        return fail(SD_E_BADARG, "sd_session_slew: v_n, v_rad, bound_rad, mean and std must be given; 1 <= J <= 32");
    ss::SessionSlew rad{};
    for (int j = 0; j < J; ++j) {
        if (!(v_rad[j] >= 0.f) || !(bound_rad[j] >= 0.f) || bound_rad[j] == INFINITY)
            return fail(SD_E_BADARG, "sd_session_slew: v_rad[j] >= 0 and a finite bound_rad[j] >= 0, no NaN");
        rad.v[j] = v_rad[j];
        rad.r[j] = bound_rad[j];
    }
    SD_LAUNCH(ss::session_slew_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, v_n, rad, mean, stdv, J);
    SD_CHECK_LAUNCH("session_slew_kernel");
    return 0;
}

extern "C" int sd_session_anchor(float *anchor, const float *x, const int32_t *robots, int S, int B, int T, int J, int row, int draws, void *stream) {
    if (!anchor || !x || S < 1 || B < 1 || S > B || T < 1 || J < 1 || J > 32 || row < 0 || row >= T || draws < 1)
        return fail(SD_E_BADARG, "sd_session_anchor: bad argument");
    const int n = S * draws * J;
    SD_LAUNCH(ss::session_anchor_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, anchor, x, robots, S, B, T, J, row, draws);
    SD_CHECK_LAUNCH("session_anchor_kernel");
    return 0;
}

extern "C" int sd_session_accel(float *a_n, const float *a_rad, const float *bound_rad, const float *mean, const float *stdv, int J, void *stream) {
    if (!a_n || !a_rad || !bound_rad || !mean || !stdv || J < 1 || J > 32)
        return fail(SD_E_BADARG, "sd_session_accel: a_n, a_rad, bound_rad, mean and std must be given; 1 <= J <= 32");
    ss::SessionSlew rad{};
    for (int j = 0; j < J; ++j) {
        if (!(a_rad[j] >= 0.f) || !(bound_rad[j] >= 0.f) || bound_rad[j] == INFINITY)
            return fail(SD_E_BADARG, "sd_session_accel: a_rad[j] >= 0 and a finite bound_rad[j] >= 0, no NaN");
        rad.v[j] = a_rad[j];
        rad.r[j] = bound_rad[j];
    }
    SD_LAUNCH(ss::session_accel_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a_n, rad, mean, stdv, J);
    SD_CHECK_LAUNCH("session_accel_kernel");
    return 0;
}

extern "C" int sd_session_anchor2(float *anchor, float *anchor2, const float *x, const int32_t *robots, int S, int B, int T, int J, int row, int draws,
                                  void *stream) {
    if (!anchor || !anchor2 || anchor == anchor2 || !x || S < 1 || B < 1 || S > B || T < 1 || J < 1 || J > 32 || row < 0 || row >= T || draws < 1)
        return fail(SD_E_BADARG, "sd_session_anchor2: bad argument");
    const int n = S * draws * J;
    SD_LAUNCH(ss::session_anchor2_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, anchor, anchor2, x, robots, S, B, T, J, row, draws);
    SD_CHECK_LAUNCH("session_anchor2_kernel");
    return 0;
}

// ---- the representative of a context's draws (sd_ddim_sample_draws + select="medoid") ------------------------------------------------
// One workgroup per context: index[c] = argmin_i sum_k |x[c, i] - x[c, k]|^2 over the G draws (T x J each, the sampler's normalised space),
// and optionally out[c] = x[c, index[c]].  fp32 in fixed orders, so the choice does not depend on scheduling and bitwise-equal draws tie
// exactly: the distance of a pair i < k is computed ONCE - lane l of a wave sums elements l, l + 64, ... of (x_i - x_k)^2 in that order, the
// 64 partial sums meet in the xor butterfly 32, 16, .. 1 (every lane ends with the same bits) - and stored as d[i][k] and d[k][i]; the score
// of draw i is d[i][0] + d[i][1] + ... + d[i][G - 1] in that order (d[i][i] = 0 included); the lowest index among the smallest scores wins.
// No atomics; contraction is off in this file, so every product and sum rounds on its own.
namespace ss {
constexpr int MEDOID_MAX_G = 64;
__global__ __launch_bounds__(THREADS) void select_medoid_kernel(const float *__restrict__ x, int32_t *__restrict__ index, float *__restrict__ out,
                                                                  int G, int n) {
    __shared__ float dist[MEDOID_MAX_G][MEDOID_MAX_G + 1];
    __shared__ float score[MEDOID_MAX_G];
    __shared__ int best;
    const int c = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float *xc = x + (long)c * G * n;
    if ((int)threadIdx.x < G) dist[threadIdx.x][threadIdx.x] = 0.f;
    const int pairs = G * (G - 1) / 2;
    for (int p = wv; p < pairs; p += THREADS / 64) {
        // pair p of the row-major list (0,1) (0,2) .. (0,G-1) (1,2) ..: wave-uniform
        int i = 0, left = p;
        while (left >= G - 1 - i) {
            left -= G - 1 - i;
            ++i;
        }
        const int k = i + 1 + left;
        const float *a = xc + (long)i * n, *b = xc + (long)k * n;
        float acc = 0.f;
        for (int e = lane; e < n; e += 64) {
            const float df = a[e] - b[e];
            acc = acc + df * df;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
        if (lane == 0) {
            dist[i][k] = acc;
            dist[k][i] = acc;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < G) {
        float sc = 0.f;
        for (int k = 0; k < G; ++k) sc = sc + dist[threadIdx.x][k];
        score[threadIdx.x] = sc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int bi = 0;
        float bs = score[0];
        for (int i = 1; i < G; ++i)
            if (score[i] < bs) {
                bs = score[i];
                bi = i;
            }
        best = bi;
        index[c] = bi;
    }
    __syncthreads();
    if (out) {
        const float *src = xc + (long)best * n;
        float *dst = out + (long)c * n;
        for (int e = threadIdx.x; e < n; e += THREADS) dst[e] = src[e];
    }
}
}   // namespace ss

extern "C" int sd_select_medoid(const float *x, int32_t *index, float *out, int C, int G, int T, int J, void *stream) {
    if (!x || !index || C <= 0 || G < 1 || G > ss::MEDOID_MAX_G || T <= 0 || J <= 0 || (long)T * J > (1L << 30))
        return fail(SD_E_BADARG, "sd_select_medoid: x and index must be given; C, T, J > 0, 1 <= G <= 64");
    if (out == x) return fail(SD_E_BADARG, "sd_select_medoid: out must not alias x");
    SD_LAUNCH(ss::select_medoid_kernel, dim3((unsigned)C), dim3(ss::THREADS), 0, (hipStream_t)stream, x, index, out, G, T * J);
    SD_CHECK_LAUNCH("select_medoid_kernel");
    return 0;
}

// ---- the draw that continues the previous plan (PolicySession(select="coherent")) -------------------------------------------------------
// One workgroup per context, waves stride over the draws.  The overlap of the new draws with the previous plan is rows [0, R) of a draw
// against rows [S, T) of the plan, R = T - S: both are R * J contiguous floats.  coh[g] = sum of w[tau] * (x - prev)^2 over them, a term
// SELECTED to 0.f where prev is NaN or the row's weight is not above zero; one wave per draw, in select_medoid_kernel's order (lane l adds
// elements l, l + 64, ..., then the xor butterfly 32 .. 1).  Every wave sees the same prev and w, so wave 0 - which always has draw 0 -
// says whether the context has a plan at all (one contributing element).  The medoid scores are computed only where they are needed - no
// plan, or lam != 0 - by select_medoid_kernel's statements in its order, so a context without a plan gets sd_select_medoid's index bit
// for bit.  cost[g] = coh[g] (lam == 0) or coh[g] + lam * med[g] (the product rounds on its own: contraction is off) with a plan, med[g]
// without one; the lowest index among the smallest costs wins.  No atomics.
namespace ss {
__global__ __launch_bounds__(THREADS) void select_coherent_kernel(const float *__restrict__ x, const float *__restrict__ prev,
                                                                    const int32_t *__restrict__ robots, const float *__restrict__ w,
                                                                    int32_t *__restrict__ index, float *__restrict__ out, float *__restrict__ cost,
                                                                    int G, int n, int J, int shift, float lam) {
    __shared__ float dist[MEDOID_MAX_G][MEDOID_MAX_G + 1];
    __shared__ float score[MEDOID_MAX_G];
    __shared__ float coh[MEDOID_MAX_G];
    __shared__ int best, has_plan;
    const int c = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float *xc = x + (long)c * G * n;
    const float *pc = prev + (long)(robots ? robots[c] : c) * n + (long)shift * J;   // row S of the context's plan
    const int m = n - shift * J;                                                       // R * J overlap elements
    for (int g = wv; g < G; g += THREADS / 64) {
        const float *a = xc + (long)g * n;
        float acc = 0.f;
        bool any = false;
        for (int e = lane; e < m; e += 64) {
            const float p = pc[e], wt = w[e / J];
            const float df = a[e] - p;
            const float term = wt * (df * df);
            const bool counts = wt > 0.f && p == p;
            any = any || counts;
            acc = acc + (counts ? term : 0.f);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
        const bool plan = __any(any);
        if (lane == 0) {
            coh[g] = acc;
            if (g == 0) has_plan = plan;
        }
    }
    __syncthreads();
    const bool plan = has_plan != 0;
    const bool medoid = !plan || lam != 0.f;   // the same in every thread of the workgroup
    if (medoid) {
        if ((int)threadIdx.x < G) dist[threadIdx.x][threadIdx.x] = 0.f;
        const int pairs = G * (G - 1) / 2;
        for (int p = wv; p < pairs; p += THREADS / 64) {
            int i = 0, left = p;
            while (left >= G - 1 - i) {
                left -= G - 1 - i;
                ++i;
            }
            const int k = i + 1 + left;
            const float *a = xc + (long)i * n, *b = xc + (long)k * n;
            float acc = 0.f;
            for (int e = lane; e < n; e += 64) {
                const float df = a[e] - b[e];
                acc = acc + df * df;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
            if (lane == 0) {
                dist[i][k] = acc;
                dist[k][i] = acc;
            }
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < G) {
        float sc = coh[threadIdx.x];
        if (medoid) {
            float med = 0.f;
            for (int k = 0; k < G; ++k) med = med + dist[threadIdx.x][k];
            if (plan) {
                const float scaled = lam * med;
                sc = sc + scaled;
            } else {
                sc = med;
            }
        }
        score[threadIdx.x] = sc;
        if (cost) cost[(long)c * G + threadIdx.x] = sc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int bi = 0;
        float bs = score[0];
        for (int i = 1; i < G; ++i)
            if (score[i] < bs) {
                bs = score[i];
                bi = i;
            }
        best = bi;
        index[c] = bi;
    }
    __syncthreads();
    if (out) {
        const float *src = xc + (long)best * n;
        float *dst = out + (long)c * n;
        for (int e = threadIdx.x; e < n; e += THREADS) dst[e] = src[e];
    }
}

// [a, a + na) and [b, b + nb) floats share an address
static bool floats_overlap(const float *a, long na, const float *b, long nb) {
    return a && b && a < b + nb && b < a + na;
}
}   // namespace ss

extern "C" int sd_select_coherent(const float *x, const float *prev, const int32_t *robots, const float *w, int32_t *index, float *out, float *cost,
                                  int C, int G, int T, int J, int shift, float lam, void *stream) {
    if (!x || !prev || !w || !index)
        return fail(SD_E_BADARG, "sd_select_coherent: x, prev, w and index must be given");
    if (C <= 0 || G < 1 || G > ss::MEDOID_MAX_G || T <= 0 || J <= 0 || (long)T * J > (1L << 30) || shift < 0 || shift >= T)
        return fail(SD_E_BADARG, "sd_select_coherent: C, T, J > 0, 1 <= G <= 64, 0 <= shift < T");
    if (!(lam >= 0.f) || lam == INFINITY) return fail(SD_E_BADARG, "sd_select_coherent: lam is a finite number >= 0");
    // the extents the call itself fixes: x holds C * G draws, prev at least C plans (one where robots names the rows), out C, cost C * G
    const long n = (long)T * J, nx = (long)C * G * n, np = (robots ? 1 : (long)C) * n;
    if (ss::floats_overlap(out, (long)C * n, x, nx) || ss::floats_overlap(out, (long)C * n, prev, np) ||
        ss::floats_overlap(cost, (long)C * G, x, nx) || ss::floats_overlap(cost, (long)C * G, prev, np))
        return fail(SD_E_BADARG, "sd_select_coherent: out and cost must not alias x or prev");
    SD_LAUNCH(ss::select_coherent_kernel, dim3((unsigned)C), dim3(ss::THREADS), 0, (hipStream_t)stream, x, prev, robots, w, index, out, cost, G,
              T * J, J, shift, lam);
    SD_CHECK_LAUNCH("select_coherent_kernel");
    return 0;
}

extern "C" int sd_session_reset(const sd_ring_reset *rings, int n_rings, const uint8_t *mask, int64_t *game_state, int64_t game_state_value, int B,
                                void *stream) {
    if (!rings || n_rings < 1 || n_rings > SD_SESSION_MAX_RESET_RINGS || B <= 0)
        return fail(SD_E_BADARG, "sd_session_reset: 1 .. 5 rings and B > 0");
    ss::Resets a{};
    for (int i = 0; i < n_rings; ++i) {
        if (!rings[i].ring || !rings[i].head || !dims_ok(B, rings[i].L, rings[i].C))
            return fail(SD_E_BADARG, "sd_session_reset: every ring needs ring and head; L, C > 0");
        a.r[i] = rings[i];
    }
    SD_LAUNCH(ss::session_reset_kernel, dim3((unsigned)B, (unsigned)n_rings), dim3(ss::THREADS), 0, (hipStream_t)stream, a, mask, game_state,
              game_state_value);
    SD_CHECK_LAUNCH("session_reset_kernel");
    return 0;
}
