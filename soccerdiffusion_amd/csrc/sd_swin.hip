// SoccerDiffusion image path, Swin-T / Swin-S inference (reference option image_encoder_type "swin_transformer_tiny" / "_small":
// soccer_diffusion/ml/model/encoder/image.py:11-20, 86-100; torchvision.models.swin_transformer V1, restated in
// soccerdiffusion_amd/ml/model/encoder/image.py).  Interface and citations: include/soccerdiffusion_hip.h (sd_token_* / sd_swin_*).
//
// Tokens are NHWC fp32 rows end to end.  A Swin block is five launches: qkv (LayerNorm prologue), window attention, proj (+ residual in
// place), fc1 (LayerNorm prologue, erf-GELU epilogue), fc2 (+ residual in place); patch merging is one launch (2 x 2 gather + LayerNorm in
// the A-operand load of its GEMM); the stem (patch embedding + LayerNorm) and the head (LayerNorm + mean over tokens) one launch each.
//
// Precision contract: every product runs on split fp16 operands - x s = hi + lo with hi = fp16(x s), lo = fp16(x s -
// hi), s a power of two - as three v_mfma_f32_16x16x32_f16 (lo.hi, hi.lo, hi.hi) accumulated in fp32 and un-scaled in the epilogue.
// Scales: one per weight row (output column), one per activation row (token GEMM: computed by the kernel's own row pass), one per
// operand tile of a (window, head) in the attention.  LayerNorm, GELU (erff) and softmax are fp32.
#include "../../include/soccerdiffusion_hip.h"
#include "sd_common.h"
#include "sd_mfma16.h"

namespace sw {

// a . b on split operands: lo.hi + hi.lo + hi.hi (lo.lo is below fp32 rounding)
__device__ __forceinline__ f32x4 mfma16x3(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x4 c) {
    c = mfma16(al, bh, c);
    c = mfma16(ah, bl, c);
    return mfma16(ah, bh, c);
}
__device__ __forceinline__ void split8(const float (&v)[8], float s, f16x8 &h, f16x8 &l) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = v[e] * s;
        h[e] = (f16)x;
        l[e] = (f16)(x - (float)h[e]);
    }
}
__device__ __forceinline__ float scale_for(float amax) { return f16_scale_from_bits(__builtin_bit_cast(unsigned, amax)); }

// ---------------------------------------------------------------------------------------------------
// token GEMM: out[R, N] = epi(pro(A)[R, K] . W^T + bias)
// ---------------------------------------------------------------------------------------------------
constexpr int BM = 64, BN = 64, KC = 64;   // rows, columns per workgroup; k per LDS chunk (two 32-wide k-steps)
constexpr int PITCH = KC + 8;              // halfs per LDS row (144 bytes: 16 lanes of a ds_read_b128 hit distinct 16-byte slots)
constexpr int LN_VEC = 6;                  // f32x4 per lane of a row held in registers by the LayerNorm row pass: K <= 64 * 4 * 6 = 1536
constexpr int LN_KMAX = 64 * 4 * LN_VEC;

// W (N, K) fp32 -> planes [Npad / 16 column tiles][K / 32 k-steps][hi | lo][64 lanes][8]: lane l holds W[16 ct + (l & 15)][32 ks + 8 (l >> 4) + e]
// * s_n (the B fragment of v_mfma_f32_16x16x32_f16); w_inv[n] = 1 / s_n, s_n the power of two of row n's abs-max.  Rows n >= N: zeros.
__global__ __launch_bounds__(64) void token_pack_kernel(const float *__restrict__ W, int N, int K, f16 *__restrict__ dst, float *__restrict__ w_inv) {
    const int n = blockIdx.x, lane = threadIdx.x;
    float m = 0.f;
    if (n < N)
        for (int k = lane; k < K; k += 64) m = fmaxf(m, fabsf(W[(long)n * K + k]));
    m = wave_max(m);
    const float s = scale_for(m);
    if (lane == 0) w_inv[n] = n < N ? 1.0f / s : 0.f;
    const int ct = n >> 4, nks = K / 32;
    for (int kg = lane; kg < K / 8; kg += 64) {
        const int ks = kg >> 2, g = kg & 3;
        f16 *o = dst + ((long)(ct * nks + ks) * 2) * 512 + ((n & 15) + 16 * g) * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = n < N ? W[(long)n * K + 8 * kg + e] * s : 0.f;
            const f16 h = (f16)v;
            o[e] = h;
            o[512 + e] = (f16)(v - (float)h);
        }
    }
}

struct TokArgs {
    const float *A;          // [R][lda] rows, or the source map [Nimg][gH][gW][gC] of a patch merging
    long lda;
    int gather, gH, gW, gC;  // gather: A row r = (n, i, j) of the (ceil(gH/2), ceil(gW/2)) map, k = (quadrant q, channel c)
    const f16 *w;            // token_pack_kernel planes
    const float *w_inv;      // [Npad]
    const float *bias;       // [N] or NULL
    const float *ln_w, *ln_b;   // [K] or NULL (no LayerNorm prologue)
    float eps;
    const float *res;        // [R][N] or NULL; may alias out
    float *out;              // [R][N]
    long R;
    int K, N, gelu;
};

// the 4 floats A[row][k .. k + 3] (k % 4 == 0; C % 32 == 0 keeps them inside one quadrant of a merge) or zeros (a padded row / position)
__device__ __forceinline__ f32x4 load_a4(const TokArgs &a, long row, int k) {
    if (row >= a.R) return f32x4{0.f, 0.f, 0.f, 0.f};
    if (!a.gather) return *reinterpret_cast<const f32x4 *>(a.A + row * a.lda + k);
    // torchvision PatchMerging: cat(x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2]) after zero padding to even H, W
    const int Ho = (a.gH + 1) >> 1, Wo = (a.gW + 1) >> 1;
    const long n = row / ((long)Ho * Wo);
    const int rem = (int)(row - n * Ho * Wo), i = rem / Wo, j = rem - (rem / Wo) * Wo;
    const int q = k / a.gC, c = k - q * a.gC;
    const int y = 2 * i + (q & 1), x = 2 * j + (q >> 1);
    if (y >= a.gH || x >= a.gW) return f32x4{0.f, 0.f, 0.f, 0.f};
    return *reinterpret_cast<const f32x4 *>(a.A + ((n * a.gH + y) * a.gW + x) * a.gC + c);
}

// One workgroup (4 waves) owns 64 rows x 64 columns; wave w computes rows 32 (w & 1) .. + 31 x columns 32 (w >> 1) .. + 31 as 2 x 2 tiles
// of 16 x 16.  Before the k loop each wave makes one pass over 16 of the rows: LayerNorm statistics (two-pass, the row in registers) and the
// power of two of the row's (normalised) abs-max.  Per 64-wide k chunk the A panel is normalised, scaled, split and staged once through LDS;
// the weight fragments of the chunk come straight from L2 (fragment-major planes, requested before the staging so that it covers them).
__global__ __launch_bounds__(256, 2) void token_gemm_kernel(TokArgs a) {
    __shared__ __attribute__((aligned(16))) f16 sA[2][BM * PITCH];
    __shared__ float4 stats[BM];   // mean, rstd, s, 1 / s
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ncb = (a.N + BN - 1) / BN;
    const long row0 = (long)(blockIdx.x / ncb) * BM;
    const int col0 = (blockIdx.x % ncb) * BN;
    const bool ln = a.ln_w != nullptr;

    // ---- row pass
    for (int r = 16 * w; r < 16 * w + 16; ++r) {
        const long row = row0 + r;
        float mean = 0.f, rstd = 0.f, amax = 0.f;
        if (row < a.R) {
            if (ln) {
                f32x4 v[LN_VEC];
                float s1 = 0.f;
#pragma unroll
                for (int q = 0; q < LN_VEC; ++q) {
                    const int k = 4 * (lane + 64 * q);
                    v[q] = k < a.K ? load_a4(a, row, k) : f32x4{0.f, 0.f, 0.f, 0.f};
                    s1 += (v[q][0] + v[q][1]) + (v[q][2] + v[q][3]);
                }
                mean = wave_sum(s1) / (float)a.K;
                float s2 = 0.f;
#pragma unroll
                for (int q = 0; q < LN_VEC; ++q) {
                    const int k = 4 * (lane + 64 * q);
                    if (k < a.K)
#pragma unroll
                        for (int e = 0; e < 4; ++e) s2 += (v[q][e] - mean) * (v[q][e] - mean);
                }
                rstd = 1.0f / sqrtf(wave_sum(s2) / (float)a.K + a.eps);
#pragma unroll
                for (int q = 0; q < LN_VEC; ++q) {
                    const int k = 4 * (lane + 64 * q);
                    if (k < a.K)
#pragma unroll
                        for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf((v[q][e] - mean) * rstd * a.ln_w[k + e] + a.ln_b[k + e]));
                }
            } else {
                for (int k = 4 * lane; k < a.K; k += 256) {
                    const f32x4 v = load_a4(a, row, k);
                    amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
                }
            }
            amax = wave_max(amax);
        }
        const float s = scale_for(amax);
        if (lane == 0) stats[r] = make_float4(mean, rstd, s, 1.0f / s);
    }

    const int rw = (w & 1) * 32, cw = (w >> 1) * 32;   // this wave's 32 x 32 sub-tile
    const int nks = a.K / 32;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // B fragments of column tile (col0 + cw) / 16 + ct, k-step ks: planes + ((tile * nks + ks) * 2 + plane) * 512 + lane * 8
    const f16 *wb = a.w + (long)((col0 + cw) >> 4) * nks * 1024 + lane * 8;
    const bool wave_live = col0 + cw < a.N;   // a wave whose 32 columns lie past N (the last block of an N = 32 (mod 64)) skips its MFMAs

    // staged A elements of this thread: 4 x (row i >> 4, 4 columns 4 (i & 15)) of the 64 x 64 chunk, i = tid + 256 q
    f32x4 pre[4];
    auto fetch = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + 256 * q, r = i >> 4, k = kc + 4 * (i & 15);
            pre[q] = k < a.K ? load_a4(a, row0 + r, k) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    __syncthreads();   // stats
    fetch(0);
    for (int kc = 0; kc < a.K; kc += KC) {
        const int steps = min(2, (a.K - kc) / 32);
        f16x8 bw[2][2][2];   // [k-step][column tile][plane]
        if (wave_live) {
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (s < steps)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        const f16 *p = wb + ((long)ct * nks + kc / 32 + s) * 1024;
                        bw[s][ct][0] = *reinterpret_cast<const f16x8 *>(p);
                        bw[s][ct][1] = *reinterpret_cast<const f16x8 *>(p + 512);
                    }
        }
        if (kc > 0) __syncthreads();   // every wave has consumed the previous chunk
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + 256 * q, r = i >> 4, c4 = i & 15, k = kc + 4 * c4;
            if (k >= a.K) continue;
            const float4 st = stats[r];
            f32x4 v = pre[q];
            if (ln) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (v[e] - st.x) * st.y * a.ln_w[k + e] + a.ln_b[k + e];
                if (row0 + r >= a.R) v = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            f16x4 h, l;
            f16_split4(v, st.z, h, l);
            *reinterpret_cast<f16x4 *>(&sA[0][r * PITCH + 4 * c4]) = h;
            *reinterpret_cast<f16x4 *>(&sA[1][r * PITCH + 4 * c4]) = l;
        }
        if (kc + KC < a.K) fetch(kc + KC);   // the next chunk's loads fly over this chunk's MFMAs
        __syncthreads();
        if (wave_live) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (s >= steps) break;
                f16x8 ah[2], al[2];
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    const int off = (rw + 16 * rt + (lane & 15)) * PITCH + 32 * s + 8 * (lane >> 4);
                    ah[rt] = *reinterpret_cast<const f16x8 *>(&sA[0][off]);
                    al[rt] = *reinterpret_cast<const f16x8 *>(&sA[1][off]);
                }
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = mfma16x3(ah[rt], al[rt], bw[s][ct][0], bw[s][ct][1], acc[rt][ct]);
            }
        }
    }
    if (!wave_live) return;
    // ---- epilogue: C/D map col = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int col = col0 + cw + 16 * ct + (lane & 15);
        if (col >= a.N) continue;
        const float winv = a.w_inv[col], bias = a.bias ? a.bias[col] : 0.f;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = rw + 16 * rt + 4 * (lane >> 4) + e;
                const long row = row0 + r;
                if (row >= a.R) continue;
                float v = acc[rt][ct][e] * (stats[r].w * winv) + bias;
                if (a.gelu) v = gelu_erf(v);
                if (a.res) v += a.res[row * a.N + col];
                a.out[row * a.N + col] = v;
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// shifted-window attention: one wave per (image, window, head); head dimension 32, window <= 8 (<= 64 tokens)
// ---------------------------------------------------------------------------------------------------
struct AttnArgs {
    const float *qkv;        // [Nimg * H * W][3 C]: q | k | v, head h at columns 32 h .. 32 h + 31 of each third
    const float *qkv_bias;   // [3 C]: q / k / v of a padding token (padding comes after norm1: qkv(0) = bias)
    const float *table;      // relative_position_bias_table [(2 w - 1)^2][heads]
    const int64_t *rpi;      // relative_position_index [w^2 * w^2]
    float *out;              // [Nimg * H * W][C]
    int H, W, C, heads, win, pH, pW, sh, sw, nWy, nWx;
};
constexpr int PP = 64 + 8;   // halfs per row of the LDS probability planes

// source row of window token t, -1 for a padding position, -2 for a slot past the window's w^2 tokens.  Token (i, j) of window (wy, wx)
// reads position ((wy w + i + sh) mod pH, (wx w + j + sw) mod pW) of the padded map (torch.roll by (-sh, -sw)); the reverse roll of the
// output sends its result back to that same position.
__device__ __forceinline__ long token_src(const AttnArgs &a, long n, int wy, int wx, int t) {
    if (t >= a.win * a.win) return -2;
    const int i = t / a.win, j = t - (t / a.win) * a.win;
    int y = wy * a.win + i + a.sh, x = wx * a.win + j + a.sw;
    if (y >= a.pH) y -= a.pH;
    if (x >= a.pW) x -= a.pW;
    if (y >= a.H || x >= a.W) return -1;
    return (n * a.H + y) * a.W + x;
}
// region id of window token t on the rolled, padded map: the attention mask of a shifted block is -100 between tokens of different regions.
// Rows: slices [0, pH - w), [pH - w, pH - sh), [pH - sh, pH) get 0, 1, 2 - with sh = 0 the last slice [0, pH) overwrites the others: 2.
__device__ __forceinline__ int token_region(const AttnArgs &a, int wy, int wx, int t) {
    const int i = t / a.win, j = t - (t / a.win) * a.win;
    const int y = wy * a.win + i, x = wx * a.win + j;
    const int ry = a.sh == 0 ? 2 : (y < a.pH - a.win ? 0 : (y < a.pH - a.sh ? 1 : 2));
    const int rx = a.sw == 0 ? 2 : (x < a.pW - a.win ? 0 : (x < a.pW - a.sw ? 1 : 2));
    return 3 * ry + rx;
}
// 8 consecutive floats of head h's q / k / v (which = 0 / 1 / 2) of a token, from its qkv row, the bias (padding) or zeros (no token)
__device__ __forceinline__ void load8(const AttnArgs &a, long src, int which, int h, int d0, float (&v)[8]) {
    const int col = which * a.C + 32 * h + d0;
    if (src == -2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
        return;
    }
    if (src == -1) {   // (parameters: no alignment assumed - an optimizer's flat buffer places them anywhere)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = a.qkv_bias[col + e];
        return;
    }
    const float *p = a.qkv + src * 3 * a.C + col;
    const f32x4 x0 = *reinterpret_cast<const f32x4 *>(p), x1 = *reinterpret_cast<const f32x4 *>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = x0[e];
        v[4 + e] = x1[e];
    }
}

// S = (q 32^-0.5) k^T + bias + mask as 4 x 4 tiles of 16 x 16 (queries x keys), softmax per query row in registers (a row's 64 keys are 4
// registers x 16 lanes of one DPP row), P split into LDS, O = P V as 4 x 2 tiles.  q / k fragments are loaded straight into the A / B
// operand lanes; v fragments (B of P V: 8 keys per lane) element-wise.
__global__ __launch_bounds__(64) void swin_attention_kernel(AttnArgs a) {
    __shared__ __attribute__((aligned(16))) f16 sP[2][64 * PP];
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
    long b = blockIdx.x;
    const int h = (int)(b % a.heads);
    b /= a.heads;
    const int wx = (int)(b % a.nWx);
    b /= a.nWx;
    const int wy = (int)(b % a.nWy);
    const long n = b / a.nWy;
    const float qscale = 0.17677669529663688110f;   // 32 ** -0.5

    float qv[4][8], kv[4][8], vv[2][2][8];   // [query tile], [key tile], [k-step][d tile]
    long src_c[4];                            // source of token 16 t + c (query / key rows of this lane)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        src_c[t] = token_src(a, n, wy, wx, 16 * t + c);
        load8(a, src_c[t], 0, h, 8 * g, qv[t]);
        load8(a, src_c[t], 1, h, 8 * g, kv[t]);
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[t][e] *= qscale;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const long src = token_src(a, n, wy, wx, 32 * s + 8 * g + e);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const int col = 2 * a.C + 32 * h + 16 * dt + c;
                vv[s][dt][e] = src == -2 ? 0.f : (src >= 0 ? a.qkv[src * 3 * a.C + col] : a.qkv_bias[col]);
            }
        }
    float mq = 0.f, mk = 0.f, mv = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            mq = fmaxf(mq, fabsf(qv[t][e]));
            mk = fmaxf(mk, fabsf(kv[t][e]));
            mv = fmaxf(mv, fabsf(vv[t >> 1][t & 1][e]));
        }
    const float sq = scale_for(wave_max(mq)), sk = scale_for(wave_max(mk)), sv = scale_for(wave_max(mv));

    // ---- S = q k^T
    f32x4 S[4][4];
    {
        f16x8 kh[4], kl[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) split8(kv[t], sk, kh[t], kl[t]);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            f16x8 qh, ql;
            split8(qv[mt], sq, qh, ql);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) S[mt][nt] = mfma16x3(qh, ql, kh[nt], kl[nt], f32x4{0.f, 0.f, 0.f, 0.f});
        }
    }
    const float inv_qk = 1.0f / (sq * sk);
    const int T = a.win * a.win;
    const bool masked = (a.sh | a.sw) != 0;
    int key_region[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) key_region[nt] = masked && 16 * nt + c < T ? token_region(a, wy, wx, 16 * nt + c) : 0;
    // ---- + relative position bias (+ mask), softmax over the keys, P -> LDS (scale 2^14: p <= 1)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int q = 16 * mt + 4 * g + e;
            const int qr = masked && q < T ? token_region(a, wy, wx, q) : 0;
            float x[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int key = 16 * nt + c;
                float v = S[mt][nt][e] * inv_qk;
                if (key >= T) v = -INFINITY;
                else if (q < T) {
                    v += a.table[a.rpi[q * T + key] * a.heads + h];
                    if (masked && qr != key_region[nt]) v += -100.0f;
                }
                x[nt] = v;
            }
            const float m = row16_max(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
            float sum = 0.f;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                x[nt] = expf(x[nt] - m);
                sum += x[nt];
            }
            const float r = 16384.0f / row16_sum(sum);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const float p = x[nt] * r;
                const f16 ph = (f16)p;
                sP[0][q * PP + 16 * nt + c] = ph;
                sP[1][q * PP + 16 * nt + c] = (f16)(p - (float)ph);
            }
        }
    __syncthreads();
    // ---- O = P V
    f16x8 vh[2][2], vl[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) split8(vv[s][dt], sv, vh[s][dt], vl[s][dt]);
    const float inv_pv = 1.0f / (16384.0f * sv);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        f32x4 O[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int off = (16 * mt + c) * PP + 32 * s + 8 * g;
            const f16x8 ph = *reinterpret_cast<const f16x8 *>(&sP[0][off]), pl = *reinterpret_cast<const f16x8 *>(&sP[1][off]);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) O[dt] = mfma16x3(ph, pl, vh[s][dt], vl[s][dt], O[dt]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int q = 16 * mt + 4 * g + e;
            const long src = token_src(a, n, wy, wx, q);
            if (src < 0) continue;   // a padding position (cropped by the module) or no token
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) a.out[src * a.C + 32 * h + 16 * dt + c] = O[dt][e] * inv_pv;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// patch embedding: conv 4 x 4 / stride 4, 3 -> 96 channels (+ bias), LayerNorm(96); NCHW frames -> NHWC tokens.  K = 48: fp32 FMA.
// One workgroup: 64 tokens; thread (token group tid >> 4: tokens 4 (tid >> 4) .. + 3, channel lane c = tid & 15: channels c + 16 i).
// ---------------------------------------------------------------------------------------------------
constexpr int PE_C = 96, PE_K = 48, PE_TOK = 64;
__global__ __launch_bounds__(256) void swin_patch_embed_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                                               const float *__restrict__ ln_w, const float *__restrict__ ln_b, float eps,
                                                               float *__restrict__ out, long ntok, int H, int W) {
    __shared__ float sw_[PE_K][PE_C];
    __shared__ float sx[PE_TOK][PE_K + 1];
    const int tid = threadIdx.x, Ho = H / 4, Wo = W / 4;
    const long tok0 = (long)blockIdx.x * PE_TOK;
    for (int i = tid; i < PE_K * PE_C; i += 256) sw_[i % PE_K][i / PE_K] = w[i];   // w (96, 3, 4, 4): [c][k], k = (ci, ky, kx)
    for (int i = tid; i < PE_TOK * PE_K; i += 256) {
        const int t = i / PE_K, k = i - (i / PE_K) * PE_K;
        const long tok = tok0 + t;
        float v = 0.f;
        if (tok < ntok) {
            const long n = tok / ((long)Ho * Wo);
            const int rem = (int)(tok - n * Ho * Wo), oy = rem / Wo, ox = rem - (rem / Wo) * Wo;
            const int ci = k >> 4, ky = (k >> 2) & 3, kx = k & 3;
            v = x[((n * 3 + ci) * H + 4 * oy + ky) * (long)W + 4 * ox + kx];
        }
        sx[t][k] = v;
    }
    __syncthreads();
    const int tg = tid >> 4, c = tid & 15;
    float acc[4][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float b = bias[c + 16 * i];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][i] = b;
    }
    for (int k = 0; k < PE_K; ++k) {
        float wk[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) wk[i] = sw_[k][c + 16 * i];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float xv = sx[4 * tg + t][k];
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[t][i] = fmaf(xv, wk[i], acc[t][i]);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 6; ++i) s += acc[t][i];
        const float mean = row16_sum(s) / (float)PE_C;
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 6; ++i) s2 += (acc[t][i] - mean) * (acc[t][i] - mean);
        const float rstd = 1.0f / sqrtf(row16_sum(s2) / (float)PE_C + eps);
        const long tok = tok0 + 4 * tg + t;
        if (tok < ntok)
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int ch = c + 16 * i;
                out[tok * PE_C + ch] = (acc[t][i] - mean) * rstd * ln_w[ch] + ln_b[ch];
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// head pooling: pooled[n][c] = mean over the T tokens of image n of LayerNorm(x)[c]; one workgroup per image, wave w takes tokens w, w + 4, ..
// (the row in registers: C <= 64 * 16, C % 64 == 0)
// ---------------------------------------------------------------------------------------------------
constexpr int HP_MAXV = 16;
__global__ __launch_bounds__(256) void swin_head_pool_kernel(const float *__restrict__ x, const float *__restrict__ ln_w, const float *__restrict__ ln_b,
                                                             float eps, float *__restrict__ pooled, int T, int C) {
    __shared__ float red[4][64 * HP_MAXV];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nv = C / 64;
    const long n = blockIdx.x;
    float acc[HP_MAXV];
#pragma unroll
    for (int i = 0; i < HP_MAXV; ++i) acc[i] = 0.f;
    for (int t = w; t < T; t += 4) {
        const float *row = x + (n * T + t) * (long)C;
        float v[HP_MAXV], s = 0.f;
#pragma unroll
        for (int i = 0; i < HP_MAXV; ++i) {
            v[i] = i < nv ? row[lane + 64 * i] : 0.f;
            s += v[i];
        }
        const float mean = wave_sum(s) / (float)C;
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < HP_MAXV; ++i)
            if (i < nv) s2 += (v[i] - mean) * (v[i] - mean);
        const float rstd = 1.0f / sqrtf(wave_sum(s2) / (float)C + eps);
#pragma unroll
        for (int i = 0; i < HP_MAXV; ++i)
            if (i < nv) acc[i] += (v[i] - mean) * rstd * ln_w[lane + 64 * i] + ln_b[lane + 64 * i];
    }
#pragma unroll
    for (int i = 0; i < HP_MAXV; ++i)
        if (i < nv) red[w][lane + 64 * i] = acc[i];
    __syncthreads();
    for (int ch = threadIdx.x; ch < C; ch += 256)
        pooled[n * C + ch] = ((red[0][ch] + red[1][ch]) + (red[2][ch] + red[3][ch])) / (float)T;
}

}   // namespace sw

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" size_t sd_token_packed_halfs(int N, int K) { return (size_t)((N + 63) / 64 * 64) * (size_t)K * 2; }
extern "C" int sd_token_pad_cols(int N) { return (N + 63) / 64 * 64; }

extern "C" int sd_token_pack(const float *w, int N, int K, void *planes, float *w_inv, void *stream) {
    if (!w || !planes || !w_inv || N <= 0 || K <= 0 || K % 32) return fail(SD_E_BADARG, "sd_token_pack: N > 0, K a positive multiple of 32");
    SD_LAUNCH(sw::token_pack_kernel, dim3((unsigned)sd_token_pad_cols(N)), dim3(64), 0, (hipStream_t)stream, w, N, K, (f16 *)planes, w_inv);
    SD_CHECK_LAUNCH("token_pack_kernel");
    return 0;
}

static int token_gemm_launch(sw::TokArgs &a, void *stream, const char *name) {
    if (!a.A || !a.w || !a.w_inv || !a.out || a.R <= 0 || a.N <= 0 || a.K <= 0 || a.K % 32) return fail(SD_E_BADARG, name);
    if ((a.ln_w == nullptr) != (a.ln_b == nullptr)) return fail(SD_E_BADARG, name);
    if (a.ln_w && a.K > sw::LN_KMAX) return fail(SD_E_BADDIM, name);
    if (!aligned16(a.A) || (!a.gather && a.lda % 4)) return fail(SD_E_BADARG, name);
    const long blocks = (a.R + sw::BM - 1) / sw::BM * ((a.N + sw::BN - 1) / sw::BN);
    if (blocks > 0x7fffffffL) return fail(SD_E_BADDIM, name);
    SD_LAUNCH(sw::token_gemm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    SD_CHECK_LAUNCH("token_gemm_kernel");
    return 0;
}

extern "C" int sd_token_linear(const float *A, const void *planes, const float *w_inv, const float *bias, const float *ln_w, const float *ln_b,
                               float ln_eps, const float *res, float *out, int64_t R, int N, int K, int gelu, void *stream) {
    sw::TokArgs a{};
    a.A = A; a.lda = K; a.gather = 0;
    a.w = (const f16 *)planes; a.w_inv = w_inv; a.bias = bias; a.ln_w = ln_w; a.ln_b = ln_b; a.eps = ln_eps;
    a.res = res; a.out = out; a.R = R; a.K = K; a.N = N; a.gelu = gelu != 0;
    return token_gemm_launch(a, stream, "sd_token_linear: bad arguments (K % 32, K <= 1536 with LayerNorm, 16-byte aligned A)");
}

extern "C" int sd_token_merge_linear(const float *x, int Nimg, int H, int W, int C, const void *planes, const float *w_inv, const float *ln_w,
                                     const float *ln_b, float ln_eps, float *out, int N, void *stream) {
    if (Nimg <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 32) return fail(SD_E_BADDIM, "sd_token_merge_linear: C a positive multiple of 32");
    sw::TokArgs a{};
    a.A = x; a.lda = 0; a.gather = 1; a.gH = H; a.gW = W; a.gC = C;
    a.w = (const f16 *)planes; a.w_inv = w_inv; a.bias = nullptr; a.ln_w = ln_w; a.ln_b = ln_b; a.eps = ln_eps;
    a.res = nullptr; a.out = out; a.R = (long)Nimg * ((H + 1) / 2) * ((W + 1) / 2); a.K = 4 * C; a.N = N; a.gelu = 0;
    return token_gemm_launch(a, stream, "sd_token_merge_linear: bad arguments (4 C <= 1536, 16-byte aligned x)");
}

extern "C" int sd_swin_window_plan(int H, int W, int window, int shift, int *plan6) {
    if (H <= 0 || W <= 0 || window <= 0 || shift < 0 || !plan6) return fail(SD_E_BADARG, "sd_swin_window_plan: bad arguments");
    const int pH = H + (window - H % window) % window, pW = W + (window - W % window) % window;
    plan6[0] = pH;
    plan6[1] = pW;
    plan6[2] = window >= pH ? 0 : shift;
    plan6[3] = window >= pW ? 0 : shift;
    plan6[4] = pH / window;
    plan6[5] = pW / window;
    return 0;
}

extern "C" int sd_swin_window_attention(const float *qkv, const float *qkv_bias, const float *table, const int64_t *rpi, float *out, int Nimg,
                                        int H, int W, int C, int heads, int window, int shift, void *stream) {
    if (!qkv || !qkv_bias || !table || !rpi || !out || Nimg <= 0 || heads <= 0 || C != 32 * heads || window < 1 || window > 8 || shift < 0 ||
        shift >= window)
        return fail(SD_E_BADARG, "sd_swin_window_attention: head dimension 32 (C = 32 heads), window 1 .. 8, 0 <= shift < window");
    if (!aligned16(qkv)) return fail(SD_E_BADARG, "sd_swin_window_attention: qkv must be 16-byte aligned");
    int p[6];
    int rc = sd_swin_window_plan(H, W, window, shift, p);
    if (rc) return rc;
    sw::AttnArgs a{qkv, qkv_bias, table, rpi, out, H, W, C, heads, window, p[0], p[1], p[2], p[3], p[4], p[5]};
    const long blocks = (long)Nimg * p[4] * p[5] * heads;
    if (blocks > 0x7fffffffL) return fail(SD_E_BADDIM, "sd_swin_window_attention: grid too large");
    SD_LAUNCH(sw::swin_attention_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, a);
    SD_CHECK_LAUNCH("swin_attention_kernel");
    return 0;
}

extern "C" int sd_swin_patch_embed(const float *x, const float *w, const float *bias, const float *ln_w, const float *ln_b, float ln_eps, float *out,
                                   int Nimg, int H, int W, void *stream) {
    if (!x || !w || !bias || !ln_w || !ln_b || !out || Nimg <= 0 || H < 4 || W < 4)
        return fail(SD_E_BADARG, "sd_swin_patch_embed: null pointer or frames smaller than one 4 x 4 patch");
    const long ntok = (long)Nimg * (H / 4) * (W / 4);
    const long blocks = (ntok + sw::PE_TOK - 1) / sw::PE_TOK;
    SD_LAUNCH(sw::swin_patch_embed_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, w, bias, ln_w, ln_b, ln_eps, out, ntok, H, W);
    SD_CHECK_LAUNCH("swin_patch_embed_kernel");
    return 0;
}

extern "C" int sd_swin_head_pool(const float *x, const float *ln_w, const float *ln_b, float ln_eps, float *pooled, int Nimg, int T, int C,
                                 void *stream) {
    if (!x || !ln_w || !ln_b || !pooled || Nimg <= 0 || T <= 0 || C <= 0 || C % 64 || C > 64 * sw::HP_MAXV)
        return fail(SD_E_BADARG, "sd_swin_head_pool: C a multiple of 64, at most 1024");
    SD_LAUNCH(sw::swin_head_pool_kernel, dim3((unsigned)Nimg), dim3(256), 0, (hipStream_t)stream, x, ln_w, ln_b, ln_eps, pooled, T, C);
    SD_CHECK_LAUNCH("swin_head_pool_kernel");
    return 0;
}
