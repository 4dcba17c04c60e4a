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


// ---- camera intake: the robot node's frame preprocessing (soccer_diffusion/ml/inference/ros.py:186-200 - cv2.resize(img, (R, R)) with the
// default INTER_LINEAR, ToDtype(float32, scale=True), Normalize(ImageNet)) on raw (H, W, 3) uint8 frames.  Interface: sd_camera_intake.
//
// cv::resize for 8-bit INTER_LINEAR (imgproc/src/resize.cpp), restated in DESIGN.md section 2:
//   - H == R and W == R: the source pixel;
//   - H == 2 R and W == 2 R: cv::resize turns INTER_LINEAR into INTER_AREA (resizeAreaFast): (2 x 2 block sum + 2) >> 2;
//   - anything else: resizeGeneric_ with HResizeLinear / VResizeLinear in 11-bit fixed point.  Per axis a first tap index and a pair of
//     int16 coefficients that sum to 2048 (built on the host: ops.linear_taps), the second tap at min(first + 1, size - 1); horizontally
//     h = S[s] c0 + S[s + 1] c1 in int32, vertically (((b0 (h0 >> 4)) >> 16) + ((b1 (h1 >> 4)) >> 16) + 2) >> 2 with arithmetic shifts.
//
// A workgroup owns one frame and one band of output rows.  The (at most two) source rows of an output row are staged in two LDS slots,
// source row s in slot s & 1 - the two rows of an output are neighbours, so they never share a slot - and a slot that already holds the
// row an output needs is not loaded again (up-scaling: consecutive outputs share source rows).  Rows of 3 W bytes start anywhere: a row is
// staged at its global address's offset inside a 16-byte unit, so its 16-byte aligned middle moves with 16-byte loads and LDS stores and only
// the ragged head and tail move byte by byte.  The horizontal taps are read from LDS and combined in registers; the value v is an integer in
// 0 .. 255, so normalize(v, c) comes from a 3 x 256 table the workgroup computes once with normalize itself (the same bits); a thread's
// consecutive columns are consecutive x of a channel plane.
constexpr int CAM_MAX = 4096;                  // H, W, R <= 4096: a staged row is at most 12 KiB
constexpr int CAM_COLS = 3;                    // (channel, x) columns a thread keeps its taps in registers for: 3 R <= 768
constexpr int CAM_ROWS_PER_BAND = 8;
enum { CAM_COPY = 0, CAM_AREA2 = 1, CAM_LINEAR = 2 };

struct CamArgs {
    const uint8_t *frames;
    int H, W, bgr, R;
    int bands, row_stride;                     // row_stride: LDS bytes per staged row, a multiple of 16, >= 3 W + 15
    const int32_t *xidx, *yidx;
    const int16_t *xcoef, *ycoef;
    float *out;
};

struct CamTap {
    int c, x;                                  // the output's channel plane and column
    int p0, p1;                                // byte offsets of the two horizontal taps inside a source row
    int c0, c1;
};

template <int MODE>
__device__ __forceinline__ CamTap cam_tap(const CamArgs &a, int col) {
    CamTap q;
    q.c = col / a.R;
    q.x = col - q.c * a.R;
    const int cs = a.bgr ? 2 - q.c : q.c;
    int s = q.x, s1 = q.x;
    q.c0 = 2048;
    q.c1 = 0;
    if constexpr (MODE == CAM_AREA2) {
        s = 2 * q.x;
        s1 = s + 1;
    }
    if constexpr (MODE == CAM_LINEAR) {        // clamped: no table entry can address outside the staged row
        s = min(max(a.xidx[q.x], 0), a.W - 1);
        s1 = min(s + 1, a.W - 1);
        q.c0 = a.xcoef[2 * q.x];
        q.c1 = a.xcoef[2 * q.x + 1];
    }
    q.p0 = 3 * s + cs;
    q.p1 = 3 * s1 + cs;
    return q;
}

template <int MODE, bool SMALL>
__global__ __launch_bounds__(THREADS) void camera_intake_kernel(CamArgs a) {
    extern __shared__ uint4 cam_lds[];         // two staged rows, then the 3 x 256 normalised values
    uint8_t *rows = reinterpret_cast<uint8_t *>(cam_lds);
    float *lut = reinterpret_cast<float *>(rows + 2 * a.row_stride);

    const int R = a.R, t = threadIdx.x, rb = 3 * a.W;
    const long slot = blockIdx.x / a.bands;
    const int band = blockIdx.x % a.bands;
    const int y0 = band * CAM_ROWS_PER_BAND, y1 = min(R, y0 + CAM_ROWS_PER_BAND);
    const long plane = (long)R * R;
    const uint8_t *frame = a.frames + slot * ((long)a.H * rb);
    float *out = a.out + slot * 3 * plane;

    for (int i = t; i < 3 * 256; i += THREADS) lut[i] = normalize((float)(i & 255), i >> 8);

    const int ncol = 3 * R;
    CamTap taps[SMALL ? CAM_COLS : 1];
    if constexpr (SMALL) {
#pragma unroll
        for (int j = 0; j < CAM_COLS; ++j) taps[j] = cam_tap<MODE>(a, min(t + j * THREADS, ncol - 1));
    }

    int held[2] = {-1, -1}, off[2] = {0, 0};   // the source row a slot holds, and where its byte 0 lies in the slot (0 .. 15)
    // source row s -> slot s & 1; `turn` rotates the threads so that the two rows of one output are fetched by different waves
    auto stage = [&](int s, int turn) {
        const int k = s & 1;
        const uint8_t *g = frame + (long)s * rb;
        const int mis = (int)(reinterpret_cast<uintptr_t>(g) & 15);
        const int head = mis ? min(16 - mis, rb) : 0;
        const int nvec = (rb - head) >> 4, tail = rb - head - (nvec << 4);
        uint8_t *l = rows + k * a.row_stride + mis;          // row byte j at l[j]: l + head is 16-byte aligned, as g + head is
        const uint4 *gv = reinterpret_cast<const uint4 *>(g + head);
        uint4 *lv = reinterpret_cast<uint4 *>(l + head);
        for (int i = (t + turn * (THREADS / 2)) % THREADS; i < nvec + head + tail; i += THREADS) {
            if (i < nvec) {
                lv[i] = gv[i];
            } else {
                const int j = i - nvec < head ? i - nvec : head + (nvec << 4) + (i - nvec - head);
                l[j] = g[j];
            }
        }
        held[k] = s;
        off[k] = mis;
    };

    for (int y = y0; y < y1; ++y) {
        int sa = y, sb = y, b0 = 2048, b1 = 0;
        if constexpr (MODE == CAM_AREA2) {
            sa = 2 * y;
            sb = sa + 1;
        }
        if constexpr (MODE == CAM_LINEAR) {
            sa = min(max(a.yidx[y], 0), a.H - 1);
            sb = min(sa + 1, a.H - 1);
            b0 = a.ycoef[2 * y];
            b1 = a.ycoef[2 * y + 1];
        }
        const bool need_a = held[sa & 1] != sa, need_b = sb != sa && held[sb & 1] != sb;
        if (need_a || need_b) {                // (the same in every thread)
            __syncthreads();                   // the rows of the previous output are no longer read
            if (need_a) stage(sa, 0);
            if (need_b) stage(sb, 1);
            __syncthreads();                   // (the first one also publishes lut)
        }
        const uint8_t *ra = rows + (sa & 1) * a.row_stride + off[sa & 1];
        const uint8_t *rbp = rows + (sb & 1) * a.row_stride + off[sb & 1];
        float *orow = out + (long)y * R;
        auto emit = [&](const CamTap &q) {
            int v;
            if constexpr (MODE == CAM_COPY) {
                v = ra[q.p0];
            } else if constexpr (MODE == CAM_AREA2) {
                v = ((int)ra[q.p0] + (int)ra[q.p1] + (int)rbp[q.p0] + (int)rbp[q.p1] + 2) >> 2;
            } else {
                const int h0 = (int)ra[q.p0] * q.c0 + (int)ra[q.p1] * q.c1;
                const int h1 = (int)rbp[q.p0] * q.c0 + (int)rbp[q.p1] * q.c1;
                v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
            }
            v = min(max(v, 0), 255);           // saturate_cast<uchar>
            orow[q.c * plane + q.x] = lut[q.c * 256 + v];
        };
        if constexpr (SMALL) {
#pragma unroll
            for (int j = 0; j < CAM_COLS; ++j)
                if (t + j * THREADS < ncol) emit(taps[j]);
        } else {
            for (int col = t; col < ncol; col += THREADS) emit(cam_tap<MODE>(a, col));
        }
    }
}

template <int MODE>
static void launch_camera(const CamArgs &a, long blocks, hipStream_t st) {
    const size_t lds = 2 * (size_t)a.row_stride + 3 * 256 * sizeof(float);    // <= 2 * 12320 + 3072 bytes
    if (3 * a.R <= CAM_COLS * THREADS) SD_LAUNCH((camera_intake_kernel<MODE, true>), dim3((unsigned)blocks), dim3(THREADS), lds, st, a);
    else SD_LAUNCH((camera_intake_kernel<MODE, false>), dim3((unsigned)blocks), dim3(THREADS), lds, st, a);
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

extern "C" int sd_camera_intake(const uint8_t *frames, int64_t n_frames, int H, int W, int bgr, int R, const int32_t *xidx, const int16_t *xcoef,
                                const int32_t *yidx, const int16_t *ycoef, float *out, void *stream) {
    if (H < 1 || H > fr::CAM_MAX || W < 1 || W > fr::CAM_MAX || R < 1 || R > fr::CAM_MAX || n_frames < 0 || (n_frames > 0 && (!frames || !out)))
        return fail(SD_E_BADARG, "sd_camera_intake: 1 <= H, W, R <= 4096, frames and out for n_frames > 0");
    // cv::resize's routes for INTER_LINEAR: nothing to do at the same size, INTER_AREA (resizeAreaFast) at an exact factor 2 on both axes
    const int mode = (H == R && W == R) ? fr::CAM_COPY : ((H == 2 * R && W == 2 * R) ? fr::CAM_AREA2 : fr::CAM_LINEAR);
    if (mode == fr::CAM_LINEAR && (!xidx || !xcoef || !yidx || !ycoef))
        return fail(SD_E_BADARG, "sd_camera_intake: the linear route needs the tap tables of both axes");
    if (n_frames == 0) return 0;
    fr::CamArgs a{};
    a.frames = frames; a.H = H; a.W = W; a.bgr = bgr != 0; a.R = R;
    a.bands = (R + fr::CAM_ROWS_PER_BAND - 1) / fr::CAM_ROWS_PER_BAND;
    a.row_stride = (3 * W + 15 + 15) / 16 * 16;
    a.xidx = xidx; a.yidx = yidx; a.xcoef = xcoef; a.ycoef = ycoef; a.out = out;
    const int64_t blocks = n_frames * a.bands;
    if (blocks > 0x7fffffffL) return fail(SD_E_BADDIM, "sd_camera_intake: grid too large");
    if (mode == fr::CAM_COPY) fr::launch_camera<fr::CAM_COPY>(a, blocks, (hipStream_t)stream);
    else if (mode == fr::CAM_AREA2) fr::launch_camera<fr::CAM_AREA2>(a, blocks, (hipStream_t)stream);
    else fr::launch_camera<fr::CAM_LINEAR>(a, blocks, (hipStream_t)stream);
    SD_CHECK_LAUNCH("camera_intake_kernel");
    return 0;
}
