// SoccerDiffusion image feed: the reference's frame preprocessing (soccer_diffusion/dataset/pytorch.py:209-211 - cv2.resize(img, (R, R),
// interpolation=cv2.INTER_AREA), ToDtype(float32, scale=True), Normalize(ImageNet)) on the stored 480 x 480 rgb8 frames, gathered by an
// index table, in one launch.  Interface and citations: include/soccerdiffusion_hip.h (sd_frames_area).
//
// OpenCV's INTER_AREA down-scaling (imgproc/src/resize.cpp), restated in DESIGN.md section 2:
//   - an integer factor k = 480 / R (|scale - round(scale)| < DBL_EPSILON, scale = 1 / (R / 480.0)): resizeAreaFast - the k x k block sum in
//     integers, (sum + 2) >> 2 for k = 2, cvRound(float(sum) * (1.f / (k k))) otherwise;
//   - any other R: resizeArea with computeResizeAreaTab's per-axis taps (built on the host: ops.area_taps): per source row, buf = buf + S alpha
//     over the output column's taps in table order, then per output row sum = sum + beta buf over its row taps in table order; fp32, every
//     product and sum rounded on its own (no FMA: contraction is off in this file), then saturate_cast<uchar> = round half to even, clamp.
//
// A workgroup owns one frame slot and one band of output rows.  It streams the band's source rows through LDS G at a time (contiguous
// 16-byte loads; the next group is loaded into registers while the current one is used) and keeps, per (channel, x) column, the sums of
// the current output row and of the next one: source row sy contributes to at most those two (consecutive outputs share at most their
// boundary row, ops.area_taps checks it).  The output row is finished at its last tap row and stored as fp32 rows of the channel planes.
#include "../../include/soccerdiffusion_hip.h"
#include "sd_common.h"

#include <float.h>
#include <math.h>

#include <algorithm>
#include <type_traits>

#pragma clang fp contract(off)

namespace fr {

constexpr int SRC = 480;                       // the recordings store 480 x 480 rgb8 frames (dataset/models.py:111-113)
constexpr int ROW_BYTES = SRC * 3;             // 1440 = 90 x 16 B
constexpr int ROW_VEC = ROW_BYTES / 16;
constexpr int THREADS = 256;
constexpr int COLS = (3 * SRC + THREADS - 1) / THREADS;    // (channel, x) columns per thread: 3 R <= 1440
constexpr int G = 8;                           // source rows per LDS stage
constexpr int STAGE_VEC = G * ROW_VEC;         // 720 x 16 B
constexpr int VPT = (STAGE_VEC + THREADS - 1) / THREADS;
constexpr int BAND_SRC_ROWS = 32;              // source rows per workgroup (the band's output rows follow from the scale)
constexpr int MAX_W = 3 * SRC;                 // weights of one axis: <= 480 full taps + 2 partial ones per output

struct Args {
    const uint8_t *store;
    long n_frames;
    const int64_t *index;
    int R, k;                                  // k > 0: integer factor (resizeAreaFast); 0: the generic tables
    int bands, rows_per_band;
    const int *tab;                            // first[R], count[R], woff[R]
    const float *w;
    int n_w;
    float *out;
};

__device__ __forceinline__ float normalize(float v, int c) {
    // ToDtype(float32, scale=True) then Normalize(mean, std) of torchvision: IEEE divisions, as the host path (dataset._preprocess)
    const float m = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
    const float s = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
    return (v / 255.0f - m) / s;
}

template <bool FAST>
__global__ __launch_bounds__(THREADS) void frames_area_kernel(Args a) {
    __shared__ uint4 stage[STAGE_VEC];
    __shared__ float wts[FAST ? 1 : MAX_W];
    __shared__ int tab[FAST ? 1 : 3 * SRC];

    const int R = a.R, t = threadIdx.x;
    const long slot = blockIdx.x / a.bands;
    const int band = blockIdx.x % a.bands;
    const int y0 = band * a.rows_per_band, y1 = min(R, y0 + a.rows_per_band);
    const long plane = (long)R * R;
    float *out = a.out + slot * 3 * plane;
    const long f = a.index[slot];
    if (f < 0 || f >= a.n_frames) {            // padding slot (-1) or an index outside the store: a zero frame
        const int n = (y1 - y0) * R;
        for (int c = 0; c < 3; ++c)
            for (int i = t; i < n; i += THREADS) out[c * plane + (long)y0 * R + i] = 0.f;
        return;
    }
    const uint8_t *frame = a.store + f * (long)(SRC * ROW_BYTES);

    if constexpr (!FAST) {
        // the tables, clamped so that no entry can address outside the frame, the stage or the weights
        for (int i = t; i < a.n_w; i += THREADS) wts[i] = a.w[i];
        for (int i = t; i < R; i += THREADS) {
            const int first = min(max(a.tab[i], 0), SRC - 1);
            const int cnt = min(min(max(a.tab[R + i], 1), SRC - first), a.n_w);
            tab[i] = first;
            tab[R + i] = cnt;
            tab[2 * R + i] = min(max(a.tab[2 * R + i], 0), a.n_w - cnt);
        }
        __syncthreads();
    }
    auto first_of = [&](int y) { return FAST ? y * a.k : tab[y]; };
    auto last_of = [&](int y) { return FAST ? y * a.k + a.k - 1 : tab[y] + tab[R + y] - 1; };

    // this thread's columns: col = t + j THREADS = c R + x
    const int ncol = 3 * R;
    int cc[COLS], fx[COLS], cx[COLS], wo[COLS];
#pragma unroll
    for (int j = 0; j < COLS; ++j) {
        const int col = t + j * THREADS;
        const int c = col < ncol ? col / R : 0, x = col < ncol ? col - c * R : 0;
        cc[j] = c;
        fx[j] = FAST ? x * a.k : tab[x];
        cx[j] = FAST ? a.k : tab[R + x];
        wo[j] = FAST ? 0 : tab[2 * R + x];
    }

    typedef typename std::conditional<FAST, int, float>::type acc_t;
    acc_t acc0[COLS], acc1[COLS];
#pragma unroll
    for (int j = 0; j < COLS; ++j) acc0[j] = acc1[j] = 0;

    const int sy_lo = first_of(y0), sy_hi = last_of(y1 - 1);
    // the current output row and the next one (inside the band), with their tap rows
    int ycur = y0;
    int cur_first = first_of(y0), cur_last = last_of(y0);
    int nxt_first = y0 + 1 < y1 ? first_of(y0 + 1) : SRC, nxt_last = y0 + 1 < y1 ? last_of(y0 + 1) : -1;

    static_assert(VPT == 3, "three 16-byte pieces per thread and stage");
    uint4 pre0 = {}, pre1 = {}, pre2 = {};
    auto load = [&](int s0) {
        const int nv = min(G, sy_hi - s0 + 1) * ROW_VEC;
        const uint4 *src = reinterpret_cast<const uint4 *>(frame + (long)s0 * ROW_BYTES);
        if (t < nv) pre0 = src[t];
        if (t + THREADS < nv) pre1 = src[t + THREADS];
        if (t + 2 * THREADS < nv) pre2 = src[t + 2 * THREADS];
    };
    if (sy_lo <= sy_hi) load(sy_lo);
    const uint8_t *S = reinterpret_cast<const uint8_t *>(stage);

    for (int s0 = sy_lo; s0 <= sy_hi; s0 += G) {
        const int nr = min(G, sy_hi - s0 + 1);
        __syncthreads();                       // the previous stage is no longer read
        if (t < nr * ROW_VEC) stage[t] = pre0;
        if (t + THREADS < nr * ROW_VEC) stage[t + THREADS] = pre1;
        if (t + 2 * THREADS < nr * ROW_VEC) stage[t + 2 * THREADS] = pre2;
        __syncthreads();
        if (s0 + G <= sy_hi) load(s0 + G);     // in flight while this stage is used

        for (int r = 0; r < nr && ycur < y1; ++r) {
            const int sy = s0 + r;
            const bool in0 = sy >= cur_first && sy <= cur_last, in1 = sy >= nxt_first && sy <= nxt_last;
            if (in0 || in1) {
                const uint8_t *row = S + r * ROW_BYTES;
                float beta0 = 0.f, beta1 = 0.f;
                if constexpr (!FAST) {
                    if (in0) beta0 = wts[tab[2 * R + ycur] + sy - cur_first];
                    if (in1) beta1 = wts[tab[2 * R + ycur + 1] + sy - nxt_first];
                }
#pragma unroll
                for (int j = 0; j < COLS; ++j) {
                    if (t + j * THREADS >= ncol) continue;
                    const uint8_t *p = row + fx[j] * 3 + cc[j];
                    acc_t h = 0;
                    for (int q = 0; q < cx[j]; ++q) {
                        if constexpr (FAST) h += p[3 * q];
                        else h = h + (float)p[3 * q] * wts[wo[j] + q];
                    }
                    if constexpr (FAST) {
                        if (in0) acc0[j] += h;         // (a source row belongs to one output row: the block sum in integers)
                    } else {
                        if (in0) acc0[j] = acc0[j] + beta0 * h;
                        if (in1) acc1[j] = acc1[j] + beta1 * h;
                    }
                }
            }
            if (sy == cur_last) {              // the current output row is complete
                float *orow = out + (long)ycur * R;
#pragma unroll
                for (int j = 0; j < COLS; ++j) {
                    const int col = t + j * THREADS;
                    if (col >= ncol) continue;
                    float v;
                    if constexpr (FAST) {
                        v = a.k == 2 ? (float)((acc0[j] + 2) >> 2) : rintf((float)acc0[j] * (1.0f / (float)(a.k * a.k)));
                    } else {
                        v = rintf(acc0[j]);
                    }
                    v = fminf(fmaxf(v, 0.f), 255.f);
                    orow[cc[j] * plane + (col - cc[j] * R)] = normalize(v, cc[j]);
                    acc0[j] = acc1[j];
                    acc1[j] = 0;
                }
                ++ycur;
                cur_first = nxt_first;
                cur_last = nxt_last;
                nxt_first = ycur + 1 < y1 ? first_of(ycur + 1) : SRC;
                nxt_last = ycur + 1 < y1 ? last_of(ycur + 1) : -1;
            }
        }
    }
}

}   // namespace fr

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int sd_frames_area(const uint8_t *store, int64_t n_frames, const int64_t *index, int64_t n_slots, int R, const int32_t *taps,
                              const float *weights, int n_weights, float *out, void *stream) {
    if (R < 1 || R > fr::SRC || n_frames < 0 || n_slots < 0 || (n_slots > 0 && (!index || !out)) || (n_frames > 0 && !store))
        return fail(SD_E_BADARG, "sd_frames_area: 1 <= R <= 480, index and out for n_slots > 0, a store for n_frames > 0");
    if (!aligned16(store)) return fail(SD_E_BADARG, "sd_frames_area: the frame store must be 16-byte aligned");
    // OpenCV's choice of resizeAreaFast: an integer scale (cv::resize, imgproc/src/resize.cpp)
    const double scale = 1.0 / ((double)R / (double)fr::SRC);
    const int iscale = (int)lrint(scale);
    const int k = fabs(scale - iscale) < DBL_EPSILON ? iscale : 0;
    if (!k && (!taps || !weights || n_weights < 1 || n_weights > fr::MAX_W))
        return fail(SD_E_BADARG, "sd_frames_area: a non-integer factor needs the tap tables (1 .. 1440 weights)");
    if (n_slots == 0) return 0;
    fr::Args a{};
    a.store = store; a.n_frames = n_frames; a.index = index; a.R = R; a.k = k;
    a.rows_per_band = std::max(1, (fr::BAND_SRC_ROWS * R + fr::SRC - 1) / fr::SRC);
    a.bands = (R + a.rows_per_band - 1) / a.rows_per_band;
    a.tab = taps; a.w = weights; a.n_w = n_weights; a.out = out;
    const long blocks = (long)n_slots * a.bands;
    if (blocks > 0x7fffffffL) return fail(SD_E_BADDIM, "sd_frames_area: grid too large");
    if (k) SD_LAUNCH(fr::frames_area_kernel<true>, dim3((unsigned)blocks), dim3(fr::THREADS), 0, (hipStream_t)stream, a);
    else SD_LAUNCH(fr::frames_area_kernel<false>, dim3((unsigned)blocks), dim3(fr::THREADS), 0, (hipStream_t)stream, a);
    SD_CHECK_LAUNCH("frames_area_kernel");
    return 0;
}
