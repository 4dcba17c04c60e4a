// Closed-loop policy session: the buffer work of the receding-horizon tick (soccer_diffusion/ml/inference/ros.py:165-335) on the device.
// Interface, ring layout and citations: include/soccerdiffusion_hip.h (sd_ring_push, sd_ring_window, sd_session_windows, sd_session_commit).
//
// ros.py keeps every sensor stream as a Python list of CPU tensors (append, then trim to the context length: ros.py:203,256-257,316-318)
// and stacks + uploads every list at every tick (ros.py:265-275).  Here a stream is a ring (B, L, C) in device memory with one head word per
// robot's ring: head = index of the oldest row = where the next row goes.  One workgroup owns one robot's ring: every thread reads the head,
// the rows are written, and after a barrier thread 0 moves the head - nothing else in the launch reads it, so no atomics are needed.  Every
// index is reduced mod L before it addresses memory: a head word that was overwritten by something else cannot send a store out of the ring.
//
// Arithmetic: contraction is off in this file.  The wrap and the published trajectory are compared bit for bit with torch's CPU expressions,
// which round every product, sum and difference on its own.
#include "../../include/soccerdiffusion_hip.h"
#include "sd_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace ss {

constexpr int THREADS = 256;

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
                                                            int L, int C, int n) {
    const int b = blockIdx.x;
    const int h = head_of(head, b, L);
    const float *s = src + (long)b * n * C;
    push_rows(ring + (long)b * L * C, h, L, C, n, [&](int r, int c) {
        const float v = s[(long)r * C + c];
        return sub ? v - sub[c] : v;
    });
    __syncthreads();                           // every thread has read the head
    if (threadIdx.x == 0) head[b] = (h + n % L) % L;
}

struct Views {
    sd_ring_view v[SD_SESSION_MAX_RINGS];
};

// grid (B, n_views): chronological row i of robot b = ring row (head + i) % L; 16-byte pieces where the rows allow it
__global__ __launch_bounds__(THREADS) void ring_windows_kernel(Views a) {
    const sd_ring_view v = a.v[blockIdx.y];
    const int b = blockIdx.x, L = v.L, C = v.C;
    const int h = head_of(v.head, b, L);
    const float *ring = v.ring + (long)b * L * C;
    float *out = v.out + (long)b * L * C;
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
                                                                 int32_t *head, int T, int J, int L) {
    const int b = blockIdx.x;
    const int h = head_of(head, b, L);
    const float *xb = x + (long)b * T * J;
    float *ob = out + (long)b * T * J;
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

static int launch_windows(const Views &a, int n_views, int B, hipStream_t st) {
    SD_LAUNCH(ring_windows_kernel, dim3((unsigned)B, (unsigned)n_views), dim3(THREADS), 0, st, a);
    SD_CHECK_LAUNCH("ring_windows_kernel");
    return 0;
}

}   // namespace ss

static bool dims_ok(int B, int L, int C) { return B > 0 && L > 0 && C > 0 && (long)L * C <= 0x7fffffffL / 2; }   // (row * C + column stays an int)

extern "C" int sd_ring_push(float *ring, int32_t *head, const float *src, const float *sub, int B, int L, int C, int n, void *stream) {
    if (!ring || !head || !dims_ok(B, L, C) || n < 0 || (n > 0 && !src) || (long)n * C > 0x7fffffffL / 2)
        return fail(SD_E_BADARG, "sd_ring_push: ring, head and (for n > 0) src must be given; B, L, C > 0, n >= 0");
    if (n == 0) return 0;
    SD_LAUNCH(ss::ring_push_kernel, dim3((unsigned)B), dim3(ss::THREADS), 0, (hipStream_t)stream, ring, head, src, sub, L, C, n);
    SD_CHECK_LAUNCH("ring_push_kernel");
    return 0;
}

extern "C" int sd_ring_window(const float *ring, const int32_t *head, float *out, int B, int L, int C, void *stream) {
    if (!ring || !head || !out || !dims_ok(B, L, C)) return fail(SD_E_BADARG, "sd_ring_window: ring, head and out must be given; B, L, C > 0");
    ss::Views a{};
    a.v[0].ring = ring; a.v[0].head = head; a.v[0].out = out; a.v[0].L = L; a.v[0].C = C;
    return ss::launch_windows(a, 1, B, (hipStream_t)stream);
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
    return ss::launch_windows(a, n_views, B, (hipStream_t)stream);
}

extern "C" int sd_session_commit(const float *x, const float *mean, const float *stdv, float *out, float *ring, int32_t *head, int B, int T, int J,
                                 int L, void *stream) {
    if (!x || !mean || !stdv || !out || !ring || !head || !dims_ok(B, L, J) || !dims_ok(B, T, J))
        return fail(SD_E_BADARG, "sd_session_commit: x, mean, std, out, ring and head must be given; B, T, J, L > 0");
    SD_LAUNCH(ss::session_commit_kernel, dim3((unsigned)B), dim3(ss::THREADS), 0, (hipStream_t)stream, x, mean, stdv, out, ring, head, T, J, L);
    SD_CHECK_LAUNCH("session_commit_kernel");
    return 0;
}
