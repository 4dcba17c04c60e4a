// SoccerDiffusion image path: the ResNet encoder heads (soccer_diffusion/ml/model/encoder/image.py:61-83), inference and training.
// Interface and citations: include/soccerdiffusion_hip.h (sd_head_*).
//
// Both heads start from the last block's NHWC map x (N, Hf, Wf, C): the avgpool head is fc(mean over Hf Wf), the no-avgpool head is
// fc(flatten_NCHW(conv1x1(x) + bias)) with 32 output channels.  Every product of either head, forward and backward, is one strided fp32
// GEMM (sd_head_gemm): each operand is addressed through a two-level stride per index, so the NCHW flattening of the 1 x 1 convolution's
// output, its transposes in the backward and the (image, pixel) split of the weight gradient's reduction index are read and written in
// place - no layout copies.  Long reductions (weight and bias gradients over N Hf Wf rows) are split over workgroups into a scratch buffer
// and summed by a second launch in a fixed order: deterministic, no atomics.  fp32 FMA throughout.
#include "../../include/soccerdiffusion_hip.h"
#include "sd_common.h"

#include <algorithm>

namespace hd {

constexpr int BM = 64, BN = 64, BK = 16, THREADS = 256;
constexpr long SPLIT_K = 256;     // reduction rows per split when a GEMM has too few output tiles to fill the chip
constexpr int MAX_SPLITS = 64;

__device__ __forceinline__ long off(long i, long d, long s1, long s0) { return d > 0 ? (i / d) * s1 + (i % d) * s0 : i * s0; }

__global__ __launch_bounds__(THREADS) void head_gemm_kernel(sd_head_gemm_args a, long kchunk, int splits) {
    __shared__ float As[BK][BM + 4];
    __shared__ float Bs[BK][BN + 4];
    const int t = threadIdx.x;
    const long m0 = (long)blockIdx.x * BM, n0 = (long)blockIdx.y * BN;
    const int z = blockIdx.z;
    const long kb = z * kchunk, ke = std::min(a.K, kb + kchunk);
    const sd_strided_operand &A = a.A, &B = a.B, &Co = a.C;

    const int am = t >> 2, ak = (t & 3) * 4;           // A tile (BM x BK): one row, four k per thread
    const bool am_ok = m0 + am < a.M;
    const long a_row = am_ok ? off(m0 + am, A.row_div, A.row_s1, A.row_s0) : 0;
    const int bk = t >> 4, bn = (t & 15) * 4;          // B tile (BK x BN): one k, four columns per thread
    long b_col[4];
    bool bn_ok[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        bn_ok[e] = n0 + bn + e < a.N;
        b_col[e] = bn_ok[e] ? off(n0 + bn + e, B.col_div, B.col_s1, B.col_s0) : 0;
    }
    const int tm = (t >> 4) * 4, tn = (t & 15) * 4;
    float acc[4][4] = {};
    for (long k0 = kb; k0 < ke; k0 += BK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long k = k0 + ak + e;
            As[ak + e][am] = (am_ok && k < ke) ? A.ptr[a_row + off(k, A.col_div, A.col_s1, A.col_s0)] : 0.f;
        }
        {
            const long k = k0 + bk;
            const long b_row = k < ke ? off(k, B.row_div, B.row_s1, B.row_s0) : 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) Bs[bk][bn + e] = (k < ke && bn_ok[e]) ? B.ptr[b_row + b_col[e]] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; ++kk) {
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = As[kk][tm + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = Bs[kk][tn + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long gm = m0 + tm + i;
        if (gm >= a.M) continue;
        const long orow = off(gm, Co.row_div, Co.row_s1, Co.row_s0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long gn = n0 + tn + j;
            if (gn >= a.N) continue;
            if (splits > 1) {
                a.scratch[((long)z * a.M + gm) * a.N + gn] = acc[i][j];
            } else {
                float v = acc[i][j];
                if (a.bias) v += a.bias[gn];
                float *o = Co.ptr + orow + off(gn, Co.col_div, Co.col_s1, Co.col_s0);
                *o = a.accumulate ? *o + v : v;
            }
        }
    }
}

// the second level of a split reduction: the partials of every output summed in split order
__global__ __launch_bounds__(THREADS) void head_gemm_reduce_kernel(sd_head_gemm_args a, int splits) {
    const long MN = a.M * a.N;
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < MN; i += (long)gridDim.x * THREADS) {
        float v = 0.f;
        for (int z = 0; z < splits; ++z) v += a.scratch[(long)z * MN + i];
        const long gm = i / a.N, gn = i % a.N;
        if (a.bias) v += a.bias[gn];
        float *o = a.C.ptr + off(gm, a.C.row_div, a.C.row_s1, a.C.row_s0) + off(gn, a.C.col_div, a.C.col_s1, a.C.col_s0);
        *o = a.accumulate ? *o + v : v;
    }
}

__global__ __launch_bounds__(THREADS) void head_pool_kernel(const float *x, float *pooled, int N, int HW, int C) {
    const long NC = (long)N * C;
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < NC; i += (long)gridDim.x * THREADS) {
        const long n = i / C, c = i % C;
        const float *p = x + n * HW * C + c;
        float s = 0.f;
        for (int q = 0; q < HW; ++q) s += p[(long)q * C];
        pooled[i] = s / (float)HW;
    }
}

__global__ __launch_bounds__(THREADS) void head_pool_bwd_kernel(const float *dpooled, float *dx, int N, int HW, int C) {
    const long total = (long)N * HW * C;
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < total; i += (long)gridDim.x * THREADS) {
        const long c = i % C, n = i / ((long)HW * C);
        dx[i] = dpooled[n * C + c] / (float)HW;
    }
}

static int splits_for(long M, long N, long K) {
    const long tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    if (tiles >= 256 || K <= 2 * SPLIT_K) return 1;
    long s = std::min<long>((K + SPLIT_K - 1) / SPLIT_K, (512 + tiles - 1) / tiles);
    return (int)std::max<long>(1, std::min<long>(s, MAX_SPLITS));
}

}   // namespace hd

extern "C" size_t sd_head_gemm_scratch_floats(int64_t M, int64_t N, int64_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int s = hd::splits_for(M, N, K);
    return s > 1 ? (size_t)s * (size_t)M * (size_t)N : 0;
}

extern "C" int sd_head_gemm(const sd_head_gemm_args *args, void *stream) {
    if (!args || args->M <= 0 || args->N <= 0 || args->K <= 0 || !args->A.ptr || !args->B.ptr || !args->C.ptr ||
        args->A.row_div < 0 || args->A.col_div < 0 || args->B.row_div < 0 || args->B.col_div < 0 || args->C.row_div < 0 || args->C.col_div < 0)
        return fail(SD_E_BADARG, "sd_head_gemm: positive M, N, K, operands, non-negative divisors");
    sd_head_gemm_args a = *args;
    int splits = hd::splits_for(a.M, a.N, a.K);
    if (!a.scratch) splits = 1;
    const long kchunk = (a.K + splits - 1) / splits;
    const long gx = (a.M + hd::BM - 1) / hd::BM, gy = (a.N + hd::BN - 1) / hd::BN;
    if (gx > 0x7fffffffL || gy > 65535) return fail(SD_E_BADDIM, "sd_head_gemm: grid too large");
    SD_LAUNCH(hd::head_gemm_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)splits), dim3(hd::THREADS), 0, (hipStream_t)stream, a, kchunk, splits);
    SD_CHECK_LAUNCH("head_gemm_kernel");
    if (splits > 1) {
        SD_LAUNCH(hd::head_gemm_reduce_kernel, dim3(grid_for(a.M * a.N, hd::THREADS)), dim3(hd::THREADS), 0, (hipStream_t)stream, a, splits);
        SD_CHECK_LAUNCH("head_gemm_reduce_kernel");
    }
    return 0;
}

extern "C" int sd_head_pool(const float *x, float *pooled, int N, int HW, int C, void *stream) {
    if (!x || !pooled || N <= 0 || HW <= 0 || C <= 0) return fail(SD_E_BADARG, "sd_head_pool: bad arguments");
    SD_LAUNCH(hd::head_pool_kernel, dim3(grid_for((long)N * C, hd::THREADS)), dim3(hd::THREADS), 0, (hipStream_t)stream, x, pooled, N, HW, C);
    SD_CHECK_LAUNCH("head_pool_kernel");
    return 0;
}

extern "C" int sd_head_pool_bwd(const float *dpooled, float *dx, int N, int HW, int C, void *stream) {
    if (!dpooled || !dx || N <= 0 || HW <= 0 || C <= 0) return fail(SD_E_BADARG, "sd_head_pool_bwd: bad arguments");
    SD_LAUNCH(hd::head_pool_bwd_kernel, dim3(grid_for((long)N * HW * C, hd::THREADS)), dim3(hd::THREADS), 0, (hipStream_t)stream, dpooled, dx, N,
              HW, C);
    SD_CHECK_LAUNCH("head_pool_bwd_kernel");
    return 0;
}
