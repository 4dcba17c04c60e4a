// Tuned trajectory step kernels of the sampler (modes 3 / 4: hidden_dim 256, 4 heads, horizon <= 100, <= 64 memory rows): the host side
// of sd_traj.h - shape test, the three preparation stages, the step launch (traj_step) and the rollout launch (traj_steps_fused), each
// for every form of the kernel: plain, pinned, shared context, held elements (the last two's instantiations compile in sd_traj_draws.hip
// and sd_traj_hold.hip) - and the
// step-token kernels that only this path launches.
// Interface towards the sampler's driver (sd_kernels.hip): sd_traj_host.h, function for function what sd_trajg.h is for the generic family.
//
// Built without packed fp32 vector instructions (soccerdiffusion_amd/build.py, EXTRA_FLAGS): the step kernel lives on the overlap of
// plain fp32 instructions with MFMAs.  build() checks the object.

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/soccerdiffusion_hip.h"

#include "sd_common.h"
#include "sd_traj.h"
#include "sd_traj_host.h"

// ---- sampler mode 3: the trajectory-owning step kernel (sd_traj.h) ---------------------------------------
// One launch per DDIM step: embedding, all layers (self-attention inside), fc_out and the DDIM update for one trajectory per
// workgroup.  Same folded cross-attention blocks (gv, cb) and abs-max words as mode 2; the split planes are written in the
// 16x16x32 fragment order of sd_traj.h into the same workspace regions.
// The shapes instantiated below (the environment's switches are the plan's business: sd_sampler_plan.h).  Any joint count up to 32: the
// embedding's K and fc_out's N are zero-padded to 32 in the packed planes; the reference's database has 22 joints
// (soccer_diffusion/dataset/models.py:222-247).  Key tiles of 16 memory slots in the folded blocks: 1 for the trajectory kernels proper,
// 2 .. 4 for traj_step_wide_kernel (17 .. 64 rows).
bool traj_ok(int d, int heads, int T, int Mk, int J, int L) {
    return d == 256 && heads == 4 && T >= 1 && T <= tj::TMAX && Mk >= 1 && Mk <= 64 && J >= 1 && J <= 32 && L >= 1 && L <= tj::MAX_L;
}

// The kernel pointers.  Token tiles: ntt = ceil(T / 16), 1 .. 7 (by_ntt: sd_common.h).  Variant: 0 = two fp16 products at the Q | K | V
// site (sampler mode 4), 1 = three (mode 3), 2 = the wide kernel (more than 16 memory rows: three products everywhere, whatever the mode
// asked for).  The pinned twins (sd_ddim_sample_pin) exist for variants 1 and 2, the rollout kernel (all DDIM steps of a trajectory in one
// launch) for 0 and 1.
typedef void (*TrajStepFn)(tj::StepArgs);
typedef void (*TrajStepPinFn)(tj::StepArgs, PinArgs);
typedef void (*TrajRolloutFn)(tj::RolloutArgs);
static TrajStepFn traj_step_fn(int ntt, int variant) {
    return by_ntt<7>(ntt, [variant](auto n) {
        constexpr int N = decltype(n)::value;
        return variant == 2 ? tj::traj_step_wide_kernel<N> : variant == 1 ? tj::traj_step_kernel<N, true> : tj::traj_step_kernel<N, false>;
    });
}
static TrajStepPinFn traj_step_pin_fn(int ntt, int variant) {
    return by_ntt<7>(ntt, [variant](auto n) {
        constexpr int N = decltype(n)::value;
        return variant == 2 ? tj::traj_step_wide_pin_kernel<N> : tj::traj_step_pin_kernel<N>;
    });
}
static TrajRolloutFn traj_rollout_fn(int ntt, bool precise) {
    return by_ntt<7>(ntt, [precise](auto n) {
        constexpr int N = decltype(n)::value;
        return precise ? tj::traj_step_rollout_kernel<N, true> : tj::traj_step_rollout_kernel<N, false>;
    });
}
// sd_traj_draws.hip: the shared-context instantiations of the same rows (one kernel serves pinned and unpinned calls: pin.rows NULL)
typedef void (*TrajStepDrawsFn)(tj::StepArgs, PinArgs, int);
typedef void (*TrajRolloutDrawsFn)(tj::RolloutDrawsArgs);
TrajStepDrawsFn traj_step_draws_fn(int ntt, int variant);
TrajRolloutDrawsFn traj_rollout_draws_fn(int ntt, bool precise);
// sd_traj_hold.hip: the hold instantiations (held elements: HoldArgs; the group size is a runtime argument, 1 included)
typedef void (*TrajStepHoldFn)(tj::StepArgs, HoldArgs, int);
TrajStepHoldFn traj_step_hold_fn(int ntt, bool wide);
// sd_traj_ms.hip: the multistep instantiations (the hold's, its mask optional, plus the second-order solver's history term: MultistepArgs)
typedef void (*TrajStepMsFn)(tj::StepArgs, HoldArgs, MultistepArgs, int);
TrajStepMsFn traj_step_ms_fn(int ntt, bool wide);
// sd_traj_lim.hip: the limits instantiations (the multistep's, its history optional, plus the per-joint clamp of x0: LimitArgs)
typedef void (*TrajStepLimFn)(tj::StepArgs, HoldArgs, MultistepArgs, LimitArgs, int);
TrajStepLimFn traj_step_lim_fn(int ntt, bool wide);
// sd_traj_slew.hip: the slew instantiations (the limits', plus the scan over the rows behind two workgroup barriers: SlewArgs)
typedef void (*TrajStepSlewFn)(tj::StepArgs, HoldArgs, MultistepArgs, LimitArgs, SlewArgs, int);
TrajStepSlewFn traj_step_slew_fn(int ntt, bool wide);
// sd_traj_acc.hip: the acceleration instantiations (the slew twins with accel_row in the scan: AccelArgs)
typedef void (*TrajStepAccelFn)(tj::StepArgs, HoldArgs, MultistepArgs, LimitArgs, SlewArgs, AccelArgs, int);
TrajStepAccelFn traj_step_accel_fn(int ntt, bool wide);
// sd_traj_direct.hip: the direct instantiations (the network's output is x0: the slew twins' epilogue without coefficients, update or history)
typedef void (*TrajStepDirectFn)(tj::StepArgs, HoldArgs, LimitArgs, SlewArgs, DirectArgs, int);
TrajStepDirectFn traj_step_direct_fn(int ntt, bool wide);

// zeroes words [col0, col0 + ncols) of every 8-word row of the abs-max table
__global__ void zero_word_cols_kernel(unsigned *mb, int rows, int col0, int ncols) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows * ncols) mb[(i / ncols) * 8 + col0 + i % ncols] = 0u;
}
static int zero_word_cols(unsigned *mb, int rows, int col0, int ncols, hipStream_t st) {
    SD_LAUNCH(zero_word_cols_kernel, dim3((unsigned)((rows * ncols + 63) / 64)), dim3(64), 0, st, mb, rows, col0, ncols);
    SD_CHECK_LAUNCH("zero_word_cols_kernel");
    return 0;
}

// The trajectory path prepares its operands in three independent stages (sd_ddim_sample_eps runs all three per call;
// sd_sampler_prepare / sd_sampler_eps let a caller that evaluates the denoiser step by step - the reference's own loop,
// soccer_diffusion/ml/inference/plot.py:122-131 - keep the first two across calls):
//   weights: abs-max + split planes of every matrix (words 0 .. 3 of a layer's row of the abs-max table, 6 / 7 of row L)
//   context: K / V of the context rows, the fold, its split blocks g16 / v16 (words 4 / 5, scales sc[4] / sc[5])
//   steps:   K / V of the n_tok step tokens, their fold, the split step blocks (words 6 / 7, scales sc[6] / sc[7])
int traj_prepare_weights(const sd_denoiser_weights *w, const TrajWs &s, hipStream_t st) {
    const int d = w->d, L = w->L;
    int rc = zero_word_cols(s.maxbits, L, 0, 4, st);
    if (!rc) rc = zero_word_cols(s.maxbits + L * 8, 1, 6, 2, st);
    if (rc) return rc;
    for (int l = 0; l < L; ++l) {
        const sd_layer_weights &lw = w->layers[l];
        const float *mats[4] = {lw.sa_out_w, lw.lin1_w, lw.lin2_w, lw.sa_in_w};
        const int rows[4] = {d, d, d, 3 * d};
        for (int m = 0; m < 4; ++m) {
            if ((rc = f16_absmax(mats[m], (long)rows[m] * d, s.maxbits + l * 8 + m, st))) return rc;
        }
    }
    if ((rc = f16_absmax(w->emb_w, (long)d * w->J, s.maxbits + L * 8 + 6, st))) return rc;
    if ((rc = f16_absmax(w->out_w, (long)d * w->J, s.maxbits + L * 8 + 7, st))) return rc;
    SD_LAUNCH(tj::pack_w16_kernel, dim3(grid_for((long)d * 4)), dim3(256), 0, st, w->emb_w, d, w->J, d, 32, s.maxbits + L * 8 + 6, 0.f, s.wio,
              s.scales + L * 8 + 6);
    SD_CHECK_LAUNCH("pack_w16_kernel");
    SD_LAUNCH(tj::pack_w16_kernel, dim3(grid_for((long)32 * d / 8)), dim3(256), 0, st, w->out_w, w->J, d, 32, d, s.maxbits + L * 8 + 7, 0.f,
              s.wio + (size_t)2 * 32 * d, s.scales + L * 8 + 7);
    SD_CHECK_LAUNCH("pack_w16_kernel");
    for (int l = 0; l < L; ++l) {
        const sd_layer_weights &lw = w->layers[l];
        const float *mats[4] = {lw.sa_out_w, lw.lin1_w, lw.lin2_w, lw.sa_in_w};
        const int rows[4] = {d, d, d, 3 * d};
        for (int m = 0; m < 4; ++m) {
            SD_LAUNCH(tj::pack_w16_kernel, dim3(grid_for((long)rows[m] * d / 8)), dim3(256), 0, st, mats[m], rows[m], d, rows[m], d, s.maxbits + l * 8 + m, 0.f,
                      f16_wf(s.wf, l, d, m), s.scales + l * 8 + m);
            SD_CHECK_LAUNCH("pack_w16_kernel");
        }
    }
    return 0;
}

int traj_prepare_ctx(const sd_denoiser_weights *w, const TrajWs &s, const float *ctx, int B, int Mc, int nkt, hipStream_t st) {
    const int d = w->d, L = w->L;
    const size_t gvstride = (size_t)B * nkt * 64 * 2 * d, cbstride = (size_t)B * nkt * 64;
    int rc = zero_async(s.gv, L * gvstride * sizeof(float), st);   // unused key slots must be finite
    if (!rc) rc = zero_async(s.cb, L * cbstride * sizeof(float), st);
    if (!rc) rc = zero_word_cols(s.maxbits, L, 4, 2, st);
    if (rc) return rc;
    const size_t blk = (size_t)32 * d;   // halfs per (trajectory, head)
    for (int l = 0; l < L; ++l) {
        const sd_layer_weights &lw = w->layers[l];
        unsigned *mb = s.maxbits + l * 8;
        if (Mc > 0) {
            const long rows = (long)B * Mc;
            float *kvl = s.kvtmp + (size_t)l * B * Mc * 2 * d;
            rc = linear(ctx, lw.ca_in_w + (size_t)d * d, lw.ca_in_b + d, nullptr, nullptr, nullptr, kvl, B * Mc, 2 * d, d, 0, st, 0);
            if (rc) return rc;
            rc = xattn_fold(kvl, rows, Mc, lw.ca_in_w, lw.ca_in_b, lw.ca_out_w, s.gv + l * gvstride, s.cb + l * cbstride, 64L * nkt, 16, d, mb + 4, mb + 5, st);
            if (rc) return rc;
        }
        SD_LAUNCH(tj::pack_g16_kernel, dim3(grid_for((long)B * nkt * 4 * 16 * d / 8)), dim3(256), 0, st, s.gv + l * gvstride, (long)B * nkt, Mc, mb + 4,
                  s.g16 + (size_t)l * B * nkt * 4 * blk, s.scales + l * 8 + 4, nkt);
        SD_CHECK_LAUNCH("pack_g16_kernel");
        SD_LAUNCH(tj::pack_v16_kernel, dim3(grid_for((long)B * nkt * 16 * 2 * 64)), dim3(256), 0, st, s.gv + l * gvstride, (long)B * nkt, Mc, mb + 5,
                  s.v16 + (size_t)l * B * nkt * 4 * blk, s.scales + l * 8 + 5, nkt);
        SD_CHECK_LAUNCH("pack_v16_kernel");
    }
    return 0;
}

// ---- the step tokens' part of the preparation, all layers in one launch each (a forward_with_context call of the reference's loop pays
// it once per call: four launches instead of four per layer)
struct StepFoldArgs { const float *wkv[tj::MAX_L], *bkv[tj::MAX_L], *wq[tj::MAX_L], *bq[tj::MAX_L], *woc[tj::MAX_L]; };
// hidden_dim 256.  step_kv_kernel, grid (n_tok, L, 8), 256 threads: rows 64 z .. 64 z + 63 of K | V = Wkv tok + bkv (memory rows are not
// layer-normed) -> kvstep[l][tok][2 D].  step_fold_all_kernel, grid (n_tok, L, 4 heads): the fold of xattn_fold_kernel for this one row and head:
// G_h = Wq_h^T K_h, V'_h = Woc_h V_h, c_h = bq_h . K_h -> gvstep row [tok * 4 + h][2 D], cstep [tok * 4 + h]; abs-max of G / V' -> words 6 / 7 of
// the layer's row.  (One workgroup per (token, layer) did all of it as a chain of dependent weight loads: 130 us for ONE token - what every
// forward_with_context call of the reference's loop pays, 27 % of a B = 256 rollout; 16 rows in flight per wave: 100 us; the work of a token
// and layer spread over 8 + 4 workgroups: see NOTEBOOK round 5.)
__global__ __launch_bounds__(256) void step_kv_kernel(StepFoldArgs a, const float *__restrict__ tokens, float *__restrict__ kvstep, long n_tok,
                                                      const int *__restrict__ map) {
    constexpr int D = tj::D;
    const int l = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long tok = blockIdx.x;
    if (map && map[tok] != (int)tok) return;   // a duplicate of token 0: nobody reads its blocks
    const f32x4 t4 = *reinterpret_cast<const f32x4 *>(tokens + tok * D + 4 * lane);
    const float *wkv = a.wkv[l], *bkv = a.bkv[l];
    const int o0 = blockIdx.z * 64 + wv * 16;
    f32x4 w4[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) w4[u] = *reinterpret_cast<const f32x4 *>(wkv + (long)(o0 + u) * D + 4 * lane);
    float *out = kvstep + ((long)l * n_tok + tok) * 2 * D;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const float s = wave_sum((w4[u][0] * t4[0] + w4[u][1] * t4[1]) + (w4[u][2] * t4[2] + w4[u][3] * t4[3]));
        if (lane == 0) out[o0 + u] = s + bkv[o0 + u];
    }
}
__global__ __launch_bounds__(256) void step_fold_all_kernel(StepFoldArgs a, const float *__restrict__ kvstep, long n_tok, float *__restrict__ gvstep,
                                                            long gv_layer_stride, float *__restrict__ cstep, long c_layer_stride,
                                                            unsigned *maxbits, const int *__restrict__ map) {
    constexpr int D = tj::D, HD = tj::HD;
    __shared__ __attribute__((aligned(16))) float sk[HD], sv[HD];
    const int l = blockIdx.y, h = blockIdx.z, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long tok = blockIdx.x;
    if (map && map[tok] != (int)tok) return;
    const int n = threadIdx.x;
    const float *wq = a.wq[l], *woc = a.woc[l] + (long)n * D;
    // the head's weights first (64 + 16 loads per thread in flight), then its K / V slice
    float wqv[HD];
    f32x4 wov[HD / 4];
#pragma unroll
    for (int j = 0; j < HD; ++j) wqv[j] = wq[(long)(h * HD + j) * D + n];
#pragma unroll
    for (int j = 0; j < HD / 4; ++j) wov[j] = *reinterpret_cast<const f32x4 *>(woc + h * HD + 4 * j);
    const float *kv = kvstep + ((long)l * n_tok + tok) * 2 * D;
    if (threadIdx.x < HD) sk[threadIdx.x] = kv[h * HD + threadIdx.x];
    else if (threadIdx.x < 2 * HD) sv[threadIdx.x - HD] = kv[D + h * HD + threadIdx.x - HD];
    __syncthreads();
    if (wv == 0) {   // the score bias of head h
        const float c = wave_sum(a.bq[l][h * HD + lane] * sk[lane]);
        if (lane == 0) cstep[l * c_layer_stride + tok * 4 + h] = c;
    }
    float g = 0.f, v = 0.f;
#pragma unroll
    for (int j = 0; j < HD; ++j) g += wqv[j] * sk[j];
#pragma unroll
    for (int j = 0; j < HD / 4; ++j) {
        const f32x4 v4 = *reinterpret_cast<const f32x4 *>(sv + 4 * j);
        v += (wov[j][0] * v4[0] + wov[j][1] * v4[1]) + (wov[j][2] * v4[2] + wov[j][3] * v4[3]);
    }
    float *out = gvstep + l * gv_layer_stride + tok * 4 * 2 * D;
    out[(long)h * 2 * D + n] = g;
    out[(long)h * 2 * D + D + n] = v;
    float mg = fabsf(g), mv = fabsf(v);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mg = fmaxf(mg, __shfl_xor(mg, o, 64));
        mv = fmaxf(mv, __shfl_xor(mv, o, 64));
    }
    if (lane == 0) {
        const unsigned bg = __builtin_bit_cast(unsigned, mg), bv = __builtin_bit_cast(unsigned, mv);
        if (bg > __atomic_load_n(maxbits + l * 8 + 6, __ATOMIC_RELAXED)) atomicMax(maxbits + l * 8 + 6, bg);
        if (bv > __atomic_load_n(maxbits + l * 8 + 7, __ATOMIC_RELAXED)) atomicMax(maxbits + l * 8 + 7, bv);
    }
}
// grid (blocks, L): the step tokens' folded keys -> [item][head][ks][plane][g][8] and folded values -> [item][plane][head][n] of every layer
// (scales from words 6 / 7 -> sc[6], sc[7]); with
// no_ctx also sc[4] = sc[6], sc[5] = sc[7] (no context rows: the all-zero context blocks carry no scale of their own - a scale of 1 from an
// abs-max of 0 would drag the common value scale of tj::step_scale down to 1)
__global__ void pack_step16_all_kernel(const float *__restrict__ gvstep, long gv_layer_stride, long n_tok, const unsigned *maxbits,
                                       f16 *__restrict__ gdst, long g_layer_stride, f16 *__restrict__ vdst, long v_layer_stride, float *scales,
                                       int no_ctx, const int *__restrict__ map) {
    constexpr int D = tj::D;
    const int l = blockIdx.y;
    const float sg = f16_scale_from_bits(maxbits[l * 8 + 6]), sv = f16_scale_from_bits(maxbits[l * 8 + 7]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        scales[l * 8 + 6] = sg;
        scales[l * 8 + 7] = sv;
        if (no_ctx) {
            scales[l * 8 + 4] = sg;
            scales[l * 8 + 5] = sv;
        }
    }
    const float *src = gvstep + l * gv_layer_stride;
    f16 *gd = gdst + l * g_layer_stride, *vd = vdst + l * v_layer_stride;
    const long ng = n_tok * 4 * (D / 8), nv = n_tok * 4 * D;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < ng + nv; i += (long)gridDim.x * blockDim.x) {
        if (i < ng) {
            const int k8 = (int)(i % (D / 8));
            const long ih = i / (D / 8);
            if (map && map[ih >> 2] != (int)(ih >> 2)) continue;
            f16x4 h0, l0, h1, l1;
            const float *row = src + ih * 2 * D + tj::kperm(k8, 0);
            f16_split4(*reinterpret_cast<const f32x4 *>(row), sg, h0, l0);
            f16_split4(*reinterpret_cast<const f32x4 *>(row + 16), sg, h1, l1);
            f16 *o = gd + ih * (8 * 2 * 32) + ((k8 >> 2) * 2) * 32 + (k8 & 3) * 8;
            *reinterpret_cast<f16x4 *>(o) = h0;
            *reinterpret_cast<f16x4 *>(o + 4) = h1;
            *reinterpret_cast<f16x4 *>(o + 32) = l0;
            *reinterpret_cast<f16x4 *>(o + 36) = l1;
        } else {
            const long j = i - ng;
            const int n = (int)(j % D), head = (int)((j / D) & 3);
            const long item = j / D / 4;
            if (map && map[item] != (int)item) continue;
            const float v = src[(item * 4 + head) * 2 * D + D + n] * sv;
            const f16 h = (f16)v;
            vd[(item * 2 + 0) * 4 * D + head * D + n] = h;
            vd[(item * 2 + 1) * 4 * D + head * D + n] = (f16)(v - (float)h);
        }
    }
}

// n_tok step tokens (rows of `tokens`): one per DDIM step of a rollout, or one per trajectory of a single evaluation
int traj_prepare_steps(const sd_denoiser_weights *w, const TrajWs &s, const float *tokens, int n_tok, int Mc, hipStream_t st, bool per_traj) {
    const int d = w->d, L = w->L;
    const size_t gvsstride = (size_t)n_tok * 4 * 2 * d, cssstride = (size_t)n_tok * 4;
    const size_t blk = (size_t)32 * d;
    int rc = zero_word_cols(s.maxbits, L, 6, 2, st);
    if (rc) return rc;
    const int *map = nullptr;
    if (per_traj) {   // one token per trajectory: fold the distinct ones only (see step_map_kernel in sd_kernels.hip)
        if ((rc = step_map(tokens, n_tok, d, s.stepmap, st))) return rc;
        map = s.stepmap;
    }
    StepFoldArgs fa{};
    for (int l = 0; l < L; ++l) {
        const sd_layer_weights &lw = w->layers[l];
        fa.wkv[l] = lw.ca_in_w + (size_t)d * d; fa.bkv[l] = lw.ca_in_b + d;
        fa.wq[l] = lw.ca_in_w; fa.bq[l] = lw.ca_in_b; fa.woc[l] = lw.ca_out_w;
    }
    SD_LAUNCH(step_kv_kernel, dim3((unsigned)n_tok, (unsigned)L, 8), dim3(256), 0, st, fa, tokens, s.kvstep, (long)n_tok, map);
    SD_CHECK_LAUNCH("step_kv_kernel");
    SD_LAUNCH(step_fold_all_kernel, dim3((unsigned)n_tok, (unsigned)L, 4), dim3(256), 0, st, fa, s.kvstep, (long)n_tok, s.gvstep, (long)gvsstride, s.cstep,
              (long)cssstride, s.maxbits, map);
    SD_CHECK_LAUNCH("step_fold_all_kernel");
    // per-layer regions as carved for mode 2 (n_tok * 4 * blk / n_tok * blk halfs), the step blocks packed densely inside
    unsigned gx = grid_for((long)n_tok * 4 * (d / 8 + d));
    SD_LAUNCH(pack_step16_all_kernel, dim3(gx, (unsigned)L), dim3(256), 0, st, s.gvstep, (long)gvsstride, (long)n_tok, s.maxbits, s.gstep16,
              (long)((size_t)n_tok * 4 * blk), s.vstep16, (long)((size_t)n_tok * blk), s.scales, Mc == 0 ? 1 : 0, map);
    SD_CHECK_LAUNCH("pack_step16_all_kernel");
    return 0;
}

// the kernel argument of step r.i of the r.n_tok prepared ones (the rollout kernel: of the steps from r.i on); coef: that step's four
// C = B / draws: the contexts traj_prepare_ctx folded (the layers' plane regions are C blocks long)
static tj::StepArgs traj_step_args(const sd_denoiser_weights *w, const TrajWs &s, const StepReq &r, const float *coef, int nkt) {
    const int d = w->d, L = w->L, C = r.B / r.draws, n_steps = r.n_tok, i = r.i;
    const size_t blk = (size_t)32 * d, cbstride = (size_t)C * nkt * 64;
    tj::StepArgs a{};
    a.nkt = nkt;
    a.status = r.status;
    a.x = r.x;
    a.eps_out = r.eps;
    a.w_emb = s.wio;
    a.b_emb = w->emb_b;
    a.pe = w->pe;
    a.n1_w = w->layers[0].n1_w;
    a.n1_b = w->layers[0].n1_b;
    a.w_out = s.wio + (size_t)2 * 32 * d;
    a.b_out = w->out_b;
    a.sc_io = s.scales + L * 8 + 6;
    if (coef) { a.c0 = coef[0]; a.c1 = coef[1]; a.c2 = coef[2]; a.c3 = coef[3]; }
    a.scale_log2e = (1.0f / sqrtf((float)(d / w->heads))) * 1.44269504088896340736f;
    a.T = r.T; a.B = r.B; a.J = w->J; a.L = L; a.Mk = r.Mc + 1; a.update_x = coef ? 1 : 0;
    a.step_per_traj = r.per_traj ? 1 : 0;
    a.step_map = r.per_traj ? s.stepmap : nullptr;
    for (int l = 0; l < L; ++l) {
        const sd_layer_weights &lw = w->layers[l];
        tj::LayerW &q = a.layer[l];
        q.n2_w = lw.n2_w; q.n2_b = lw.n2_b; q.n3_w = lw.n3_w; q.n3_b = lw.n3_b;
        q.w_o = f16_wf(s.wf, l, d, 0); q.w_1 = f16_wf(s.wf, l, d, 1); q.w_2 = f16_wf(s.wf, l, d, 2); q.w_in = f16_wf(s.wf, l, d, 3);
        q.b_in = lw.sa_in_b; q.b_o = lw.sa_out_b; q.b_1 = lw.lin1_b; q.b_2 = lw.lin2_b; q.b_oc = lw.ca_out_b;
        q.sc = s.scales + l * 8;
        q.g16 = s.g16 + (size_t)l * C * nkt * 4 * blk;
        q.v16 = s.v16 + (size_t)l * C * nkt * 4 * blk;
        q.cb = s.cb + l * cbstride;
        // per-layer regions as carved for mode 2 (n_steps * 4 * blk / n_steps * blk halfs), the step blocks packed densely inside
        q.gstep = s.gstep16 + (size_t)l * n_steps * 4 * blk + (size_t)i * (4 * 8 * 2 * 32);
        q.vstep = s.vstep16 + (size_t)l * n_steps * blk + (size_t)i * (2 * 4 * d);
        q.cstep = s.cstep + ((size_t)l * n_steps + i) * 4;
        q.nln_w = l + 1 < L ? w->layers[l + 1].n1_w : nullptr;
        q.nln_b = l + 1 < L ? w->layers[l + 1].n1_b : nullptr;
    }
    return a;
}

// B a multiple of draws.  The step kernels index the context (b / draws) and the step block (per_traj: step_map[b]) separately, so a group
// of draws may carry per-trajectory step tokens (sd_sampler_eps_draws); the rollout kernel has no per-trajectory tokens at all.
static bool traj_groups_ok(const StepReq &r) { return r.draws >= 1 && r.B > 0 && r.B % r.draws == 0; }

// one denoiser step + DDIM update in ONE launch: the plain kernel, its pinned twin, or - draws > 1 - the shared-context one, which takes the pin
// as a runtime option; r.hold: the hold twin (sd_traj_hold.hip), whatever the group size; r.ms: the multistep twin (sd_traj_ms.hip);
// r.lim: the limits twin (sd_traj_lim.hip); r.slew: the slew twin (sd_traj_slew.hip); r.direct: the direct twin (sd_traj_direct.hip);
// r.accel: the acceleration twin (sd_traj_acc.hip)
int traj_step(const sd_denoiser_weights *w, const TrajWs &s, const StepReq &r, hipStream_t st, int nkt, bool precise) {
    const int ntt = (r.T + 15) / 16;
    const int variant = nkt > 1 ? 2 : (precise ? 1 : 0);
    if (ntt < 1 || ntt > 7) return fail(SD_E_BADARG, "traj_step_kernel: horizon out of range");
    if (!traj_groups_ok(r)) return fail(SD_E_BADARG, "traj_step_draws_kernel: B must be a multiple of draws >= 1");
    if (r.direct) {   // x0 = the network's output: hold, scan (slew->v given) and box in the epilogue, x only read
        if (r.coef || r.pin || r.ms || variant == 0 || !r.direct->out || !r.lim || !r.lim->lo || !r.lim->hi || w->J > 32 ||
            (r.hold && r.hold->mask && !r.hold->x0))
            return fail(SD_E_BADARG, "traj_step_direct_kernel: the direct twins take no coefficients, pin or history; they need out, lo and hi, the three-product kernels and J <= 32");
        const tj::StepArgs a = traj_step_args(w, s, r, nullptr, nkt);
        static DevFlag direct_attr_set[2][8];   // [one key tile | wide][ntt]
        return launch_step_kernel(traj_step_direct_fn(ntt, variant == 2), "traj_step_direct_kernel", direct_attr_set[variant == 2][ntt], tj::LDS_BYTES, r.B,
                                  tj::NTHREADS, tj::LDS_BYTES, st, a, r.hold ? *r.hold : HoldArgs{nullptr, nullptr, nullptr}, *r.lim,
                                  r.slew ? *r.slew : SlewArgs{nullptr, nullptr}, *r.direct, r.draws);
    }
    if (r.pin && (!r.coef || variant == 0)) return fail(SD_E_BADARG, "traj_step_pin_kernel: pinned rows need the DDIM coefficients and the three-product kernels");
    if (r.hold && (!r.coef || variant == 0 || r.pin))
        return fail(SD_E_BADARG, "traj_step_hold_kernel: held elements need the DDIM coefficients and the three-product kernels, and exclude a pin");
    if (r.ms && (!r.coef || variant == 0 || r.pin || (!r.ms->hist && !r.lim)))
        return fail(SD_E_BADARG, "traj_step_ms_kernel: the multistep term needs the DDIM coefficients, the three-product kernels and a history buffer, and excludes a pin");
    if (r.lim && (!r.ms || !r.lim->lo || !r.lim->hi || (!r.ms->hist && r.ms->w != 0.f)))
        return fail(SD_E_BADARG, "traj_step_lim_kernel: limits need lo and hi and the multistep arguments (a history buffer wherever w != 0)");
    if (r.slew && (!r.lim || !r.slew->v || w->J > 32))
        return fail(SD_E_BADARG, "traj_step_slew_kernel: slew limits need v, the limits arguments (which may all be infinite) and J <= 32");
    if (r.accel && (!r.slew || !r.accel->a))
        return fail(SD_E_BADARG, "traj_step_accel_kernel: acceleration limits need a and the slew arguments (whose v may all be infinite)");
    const tj::StepArgs a = traj_step_args(w, s, r, r.coef, nkt);
    if (r.accel) {   // the slew call with two rows of state in the scan
        static DevFlag accel_attr_set[2][8];   // [one key tile | wide][ntt]
        return launch_step_kernel(traj_step_accel_fn(ntt, variant == 2), "traj_step_accel_kernel", accel_attr_set[variant == 2][ntt], tj::LDS_BYTES, r.B,
                                  tj::NTHREADS, tj::LDS_BYTES, st, a, r.hold ? *r.hold : HoldArgs{nullptr, nullptr, nullptr}, *r.ms, *r.lim, *r.slew, *r.accel,
                                  r.draws);
    }
    if (r.slew) {   // the limits call plus the scan over the rows
        static DevFlag slew_attr_set[2][8];   // [one key tile | wide][ntt]
        return launch_step_kernel(traj_step_slew_fn(ntt, variant == 2), "traj_step_slew_kernel", slew_attr_set[variant == 2][ntt], tj::LDS_BYTES, r.B, tj::NTHREADS,
                                  tj::LDS_BYTES, st, a, r.hold ? *r.hold : HoldArgs{nullptr, nullptr, nullptr}, *r.ms, *r.lim, *r.slew, r.draws);
    }
    if (r.lim) {   // DDIM (ms->hist NULL) or multistep, held or not, whatever the group size
        static DevFlag lim_attr_set[2][8];   // [one key tile | wide][ntt]
        return launch_step_kernel(traj_step_lim_fn(ntt, variant == 2), "traj_step_lim_kernel", lim_attr_set[variant == 2][ntt], tj::LDS_BYTES, r.B, tj::NTHREADS,
                                  tj::LDS_BYTES, st, a, r.hold ? *r.hold : HoldArgs{nullptr, nullptr, nullptr}, *r.ms, *r.lim, r.draws);
    }
    if (r.ms) {   // held or not (a hold's mask may be NULL), whatever the group size
        static DevFlag ms_attr_set[2][8];   // [one key tile | wide][ntt]
        return launch_step_kernel(traj_step_ms_fn(ntt, variant == 2), "traj_step_ms_kernel", ms_attr_set[variant == 2][ntt], tj::LDS_BYTES, r.B, tj::NTHREADS,
                                  tj::LDS_BYTES, st, a, r.hold ? *r.hold : HoldArgs{nullptr, nullptr, nullptr}, *r.ms, r.draws);
    }
    if (r.hold) {
        static DevFlag hold_attr_set[2][8];   // [one key tile | wide][ntt]
        return launch_step_kernel(traj_step_hold_fn(ntt, variant == 2), "traj_step_hold_kernel", hold_attr_set[variant == 2][ntt], tj::LDS_BYTES, r.B, tj::NTHREADS,
                                  tj::LDS_BYTES, st, a, *r.hold, r.draws);
    }
    static DevFlag attr_set[3][3][8];   // [plain | pinned | shared context][variant][ntt]
    DevFlag &flag = attr_set[r.draws > 1 ? 2 : r.pin ? 1 : 0][variant][ntt];
    if (r.draws > 1)
        return launch_step_kernel(traj_step_draws_fn(ntt, variant), "traj_step_draws_kernel", flag, tj::LDS_BYTES, r.B, tj::NTHREADS, tj::LDS_BYTES, st,
                                  a, r.pin ? *r.pin : PinArgs{nullptr, nullptr, nullptr}, r.draws);
    if (r.pin)
        return launch_step_kernel(traj_step_pin_fn(ntt, variant), "traj_step_pin_kernel", flag, tj::LDS_BYTES, r.B, tj::NTHREADS, tj::LDS_BYTES, st, a, *r.pin);
    return launch_step_kernel(traj_step_fn(ntt, variant), "traj_step_kernel", flag, tj::LDS_BYTES, r.B, tj::NTHREADS, tj::LDS_BYTES, st, a);
}

// DDIM steps r.i .. r.i + n - 1 of the r.n_tok prepared ones in ONE launch, x updated in place (n <= TRAJ_ROLLOUT_MAX_STEPS; one key tile).
// Step for step the arithmetic of traj_step; profiled under the same class.
int traj_steps_fused(const sd_denoiser_weights *w, const TrajWs &s, const StepReq &r, int n, hipStream_t st, bool precise) {
    static_assert(TRAJ_ROLLOUT_MAX_STEPS == tj::ROLL_MAX_STEPS, "one cap on both sides of the interface");
    static_assert(sizeof(tj::RolloutDrawsArgs) <= 4096, "kernel argument (RolloutArgs and the group size)");
    const int ntt = (r.T + 15) / 16;
    if (ntt < 1 || ntt > 7) return fail(SD_E_BADARG, "traj_step_rollout_kernel: horizon out of range");
    if (n < 1 || n > tj::ROLL_MAX_STEPS || r.i < 0 || r.i + n > r.n_tok || !r.coef) return fail(SD_E_BADARG, "traj_step_rollout_kernel: bad step range");
    if (!traj_groups_ok(r) || r.eps || r.per_traj || r.pin || r.hold || r.ms || r.lim || r.slew)
        return fail(SD_E_BADARG, "traj_step_rollout_kernel: B a multiple of draws; nothing returned per step, no per-trajectory tokens, no pin");
    tj::RolloutDrawsArgs da{};
    da.draws = r.draws;
    da.ra.a = traj_step_args(w, s, r, r.coef + 4 * r.i, 1);
    da.ra.r.n_steps = n;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 4; ++k) da.ra.r.coef[i][k] = r.coef[4 * (r.i + i) + k];
    static DevFlag attr_set[2][2][8];   // [own | shared context][precise][ntt]
    if (r.draws > 1)
        return launch_step_kernel(traj_rollout_draws_fn(ntt, precise), "traj_step_rollout_draws_kernel", attr_set[1][precise][ntt], tj::LDS_BYTES, r.B, tj::NTHREADS,
                                  tj::LDS_BYTES, st, da);
    return launch_step_kernel(traj_rollout_fn(ntt, precise), "traj_step_rollout_kernel", attr_set[0][precise][ntt], tj::LDS_BYTES, r.B, tj::NTHREADS, tj::LDS_BYTES, st,
                              da.ra);
}
