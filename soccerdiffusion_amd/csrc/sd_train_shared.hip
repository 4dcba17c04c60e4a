// Training with several noise draws per window (train_step(draws=K)): the cross-attention of C K trajectories over the C encoded
// contexts they share.  Trajectory b attends to the Mc projected rows of context b / K followed by its own projected step token at key
// index Mc - the order of cat(context, token) - so K | V of the context rows are projected, stored and read once per context instead of
// once per trajectory, and their gradient is summed over the K draws here, in a fixed order, instead of by K times as many GEMM rows.
//
// Both kernels are the fp32-MFMA attention kernels of sd_kernels.hip / sd_train.hip (attention_kernel, attention_bwd_kernel) in their
// transposed orientation - keys on the accumulator rows, a query per lane column - with the key rows gathered from two segments:
// same products, same softmax, same dropout mask index ((b * heads + h) * T + t, key, width Mc + 1), so a shared call and the existing
// call on expanded K | V drop the same probabilities and agree to fp32 rounding.
//   forward:  one workgroup per (trajectory, head), as attention_kernel.
//   backward: one workgroup per (CONTEXT, head) walks the K draws of its group one after the other.  dK | dV of a context key tile are
//             added draw by draw by the lane that owns the element (plain loads and stores in program order: no atomics, the same bits
//             every run); the token key's row belongs to one draw and is stored once.  Where the whole key set is one LDS chunk
//             (Mc < 64: sim_scratch.yaml's 41 rows) the context rows are staged once per workgroup and only the token row changes
//             between draws; longer memories (default.yaml's 302 rows) restage their 64-key chunks per draw from L2.
//             The draws of a group run one after the other on fp32 MFMAs, in a grid of only C x heads workgroups: measured, the step
//             on these kernels is NOT faster than the step on the expanded context.  Packing the K T query rows of a
//             group into one pass would need the token key - one per draw - outside the shared key tile; not done.
#include "sd_common.h"

namespace {

constexpr int XS_KC = 64;        // keys per LDS chunk (two 32-key tiles)
constexpr int XS_QP = 128;       // query rows of one draw held in LDS (T <= 100: four waves of 32)
constexpr int XS_MAX_T = 100;

template <int HD>
struct XsFwdCfg {
    static constexpr int FT = (HD + 31) / 32;
    static constexpr int LDK = HD + 4;
    static constexpr int LDV = FT * 32;
    static constexpr int KSTEPS = HD / 8;
};

template <int HD>
struct XsBwdCfg {
    static constexpr int FT = (HD + 31) / 32;
    static constexpr int FW = FT * 32;
    static constexpr int LDF = FW + 4;
    static constexpr int LDP = XS_QP + 4;
    static constexpr int KSTEPS = HD / 8;
    static constexpr size_t LDS_BYTES = ((size_t)2 * XS_QP * LDF + 2 * XS_KC * LDF + 2 * 32 * LDP) * sizeof(float);
};

// key row `key` of trajectory b: context rows first, the trajectory's own token row at index Mc, zeros past it
__device__ __forceinline__ void xs_load_kv(const float *kc, const float *kt, int ldkv, int d, int key, int Mc, int col, f32x4 &kf, f32x4 &vf) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    kf = z;
    vf = z;
    if (key <= Mc) {
        const float *row = key < Mc ? kc + (long)key * ldkv : kt;
        kf = *reinterpret_cast<const f32x4 *>(row + col);
        vf = *reinterpret_cast<const f32x4 *>(row + d + col);
    }
}

template <int HD, bool DROP>
__global__ __launch_bounds__(256) void xattn_shared_fwd_kernel(const float *__restrict__ q, const float *__restrict__ kv_ctx,
                                                                const float *__restrict__ kv_tok, float *__restrict__ out,
                                                                float *__restrict__ lse2, int K, int T, int Mc, int heads, float scale_log2e,
                                                                DropoutArgs da) {
    using C = XsFwdCfg<HD>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int S_all = Mc + 1, d = heads * HD, ldkv = 2 * d;
    const int rows_cap = min(XS_KC, ((S_all + 31) / 32) * 32);
    float *sK = smem;
    float *sV = smem + rows_cap * C::LDK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const float *qb = q + (long)b * T * d + h * HD;
    const float *kc = kv_ctx + (long)(b / K) * Mc * ldkv + h * HD;
    const float *kt = kv_tok + (long)b * ldkv + h * HD;

    const int q0 = wave * 32;
    const bool wave_active = q0 < T;   // wave-uniform
    const int qi = q0 + l31;
    f32x4 qf[C::KSTEPS];
#pragma unroll
    for (int st = 0; st < C::KSTEPS; ++st) {
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (qi < T) t = *reinterpret_cast<const f32x4 *>(qb + (long)qi * d + st * 8 + 4 * half);
        qf[st] = t;
    }
    f32x16 o[C::FT];
#pragma unroll
    for (int ft = 0; ft < C::FT; ++ft)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[ft][r] = 0.f;
    float m_run = -INFINITY, l_part = 0.f;

    for (int kc0 = 0; kc0 < S_all; kc0 += XS_KC) {
        __syncthreads();
        constexpr int KV4 = HD / 4;
        const int rows_staged = ((min(S_all - kc0, XS_KC) + 31) / 32) * 32;
        for (int i = tid; i < rows_staged * KV4; i += 256) {
            const int row = i / KV4, c4 = i - row * KV4;
            f32x4 kf, vf;
            xs_load_kv(kc, kt, ldkv, d, kc0 + row, Mc, c4 * 4, kf, vf);
            *reinterpret_cast<f32x4 *>(sK + row * C::LDK + c4 * 4) = kf;
            *reinterpret_cast<f32x4 *>(sV + row * C::LDV + c4 * 4) = vf;
        }
        if constexpr (C::LDV > HD) {
            constexpr int PADW = C::LDV - HD;
            for (int i = tid; i < rows_staged * PADW; i += 256) sV[(i / PADW) * C::LDV + HD + (i % PADW)] = 0.f;
        }
        __syncthreads();
        if (!wave_active) continue;

        constexpr int KT = XS_KC / 32;
        f32x16 sc[KT];
        const int kt_valid = (min(S_all - kc0, XS_KC) + 31) / 32;
#pragma unroll
        for (int kt_ = 0; kt_ < KT; ++kt_) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[kt_][r] = 0.f;
            if (kt_ < kt_valid) {
                const float *kp = sK + (kt_ * 32 + l31) * C::LDK + 4 * half;
#pragma unroll
                for (int st = 0; st < C::KSTEPS; ++st) {
                    const f32x4 kf = *reinterpret_cast<const f32x4 *>(kp + st * 8);
#pragma unroll
                    for (int j = 0; j < 4; ++j) sc[kt_] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j], qf[st][j], sc[kt_], 0, 0, 0);
                }
            }
        }
        float m_c = -INFINITY;
#pragma unroll
        for (int kt_ = 0; kt_ < KT; ++kt_)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kc0 + kt_ * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const float sv = (key < S_all) ? sc[kt_][r] : -INFINITY;
                sc[kt_][r] = sv;
                m_c = fmaxf(m_c, sv);
            }
        m_c = fmaxf(m_c, __shfl_xor(m_c, 32, 64));
        const float m_new = fmaxf(m_run, m_c);   // finite: every chunk holds >= 1 valid key
        const float alpha = exp2f((m_run - m_new) * scale_log2e);
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int kt_ = 0; kt_ < KT; ++kt_)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = exp2f((sc[kt_][r] - m_new) * scale_log2e);
                sc[kt_][r] = p;
                psum += p;
            }
        if constexpr (DROP) {   // the mask index of sd_op_attention_lse_dropout for (b, h, t, key) with S = Mc + 1
            const unsigned long mrow = ((unsigned long)b * heads + h) * T + (qi < T ? qi : 0);
            const unsigned long wq = (unsigned long)((S_all + 3) >> 2);
#pragma unroll
            for (int kt_ = 0; kt_ < KT; ++kt_)
                if (kt_ < kt_valid) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 m4 = dropout_quad(da, mrow * wq + (unsigned long)((kc0 + kt_ * 32 + 8 * g + 4 * half) >> 2));
#pragma unroll
                        for (int e = 0; e < 4; ++e) sc[kt_][4 * g + e] *= m4[e];
                    }
                }
        }
        l_part = l_part * alpha + psum;
#pragma unroll
        for (int ft = 0; ft < C::FT; ++ft)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[ft][r] *= alpha;
#pragma unroll
        for (int kt_ = 0; kt_ < KT; ++kt_) {
            if (kt_ < kt_valid) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (kc0 + kt_ * 32 + 8 * g < S_all) {
#pragma unroll
                        for (int ri = 0; ri < 4; ++ri) {
                            const int r = 4 * g + ri;
                            const int krow = kt_ * 32 + ri + 8 * g + 4 * half;
#pragma unroll
                            for (int ft = 0; ft < C::FT; ++ft) {
                                const float a = sV[krow * C::LDV + ft * 32 + l31];
                                o[ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sc[kt_][r], o[ft], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        }
    }
    if (wave_active) {
        const float l_tot = l_part + __shfl_xor(l_part, 32, 64);
        const float inv = 1.0f / l_tot;
        if (qi < T && half == 0) lse2[((long)b * heads + h) * T + qi] = m_run * scale_log2e + log2f(l_tot);
        if (qi < T) {
            float *op = out + ((long)b * T + qi) * d + h * HD;
#pragma unroll
            for (int ft = 0; ft < C::FT; ++ft)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int f = ft * 32 + 8 * g + 4 * half;
                    if (f < HD) {
                        f32x4 t = {o[ft][4 * g] * inv, o[ft][4 * g + 1] * inv, o[ft][4 * g + 2] * inv, o[ft][4 * g + 3] * inv};
                        *reinterpret_cast<f32x4 *>(op + f) = t;
                    }
                }
        }
    }
}

// (dkv_ctx is read back by the lane that wrote it: no __restrict__ on the outputs)
template <int HD, bool DROP>
__global__ __launch_bounds__(256) void xattn_shared_bwd_kernel(const float *__restrict__ q, const float *__restrict__ kv_ctx,
                                                                const float *__restrict__ kv_tok, const float *__restrict__ o,
                                                                const float *__restrict__ dO, const float *__restrict__ lse2, float *dq,
                                                                float *dkv_ctx, float *dkv_tok, int K, int T, int Mc, int heads, float scale,
                                                                DropoutArgs da) {
    using C = XsBwdCfg<HD>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sQ = smem;
    float *sdO = sQ + XS_QP * C::LDF;
    float *sK = sdO + XS_QP * C::LDF;
    float *sV = sK + XS_KC * C::LDF;
    float *sP = sV + XS_KC * C::LDF;
    float *sdS = sP + 32 * C::LDP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int c = blockIdx.x / heads, h = blockIdx.x % heads;
    const int S_all = Mc + 1, d = heads * HD, ldkv = 2 * d;
    const float sl2e = scale * 1.44269504088896340736f;
    const float *kc = kv_ctx + (long)c * Mc * ldkv + h * HD;
    float *dkc = dkv_ctx + (long)c * Mc * ldkv + h * HD;
    const bool one_chunk = S_all <= XS_KC;   // the context rows stay in LDS over the draws
    constexpr int F4 = C::FW / 4;

    const int q0 = wave * 32;                     // this wave's queries of the draw
    const int qi = q0 + l31;
    const bool wave_active = q0 < T;              // wave-uniform
    const bool q_ok = qi < T;
    const int q_rows = (T + 7) & ~7;              // dV / dK contract over the draw's rows only: the P^T / dS^T columns past T are zero

    for (int g = 0; g < K; ++g) {
        const int b = c * K + g;
        const float *qb = q + (long)b * T * d + h * HD;
        const float *ob = o + (long)b * T * d + h * HD;
        const float *dob = dO + (long)b * T * d + h * HD;
        const float *kt = kv_tok + (long)b * ldkv + h * HD;
        float *dkt = dkv_tok + (long)b * ldkv + h * HD;
        __syncthreads();
        // ---- stage Q and dO of this draw (zero rows past T, zero feature padding) ---
        for (int i = tid; i < XS_QP * F4; i += 256) {
            const int row = i / F4, c4 = i - row * F4;
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, dd = {0.f, 0.f, 0.f, 0.f};
            if (row < T && c4 * 4 < HD) {
                a = *reinterpret_cast<const f32x4 *>(qb + (long)row * d + c4 * 4);
                dd = *reinterpret_cast<const f32x4 *>(dob + (long)row * d + c4 * 4);
            }
            *reinterpret_cast<f32x4 *>(sQ + row * C::LDF + c4 * 4) = a;
            *reinterpret_cast<f32x4 *>(sdO + row * C::LDF + c4 * 4) = dd;
        }
        float delta = 0.f, lse = 0.f;
        if (q_ok) {
            for (int f = half * (HD / 2); f < (half + 1) * (HD / 2); f += 4) {
                const f32x4 ov = *reinterpret_cast<const f32x4 *>(ob + (long)qi * d + f);
                const f32x4 dv4 = *reinterpret_cast<const f32x4 *>(dob + (long)qi * d + f);
                delta += ov[0] * dv4[0] + ov[1] * dv4[1] + ov[2] * dv4[2] + ov[3] * dv4[3];
            }
            lse = lse2[((long)b * heads + h) * T + qi];
        }
        delta += __shfl_xor(delta, 32, 64);
        f32x16 dqT[C::FT];
#pragma unroll
        for (int ft = 0; ft < C::FT; ++ft)
#pragma unroll
            for (int r = 0; r < 16; ++r) dqT[ft][r] = 0.f;
        __syncthreads();
        f32x4 qf[C::KSTEPS], dof[C::KSTEPS];
#pragma unroll
        for (int st = 0; st < C::KSTEPS; ++st) {
            const int row = wave_active ? q0 + l31 : 0;
            qf[st] = *reinterpret_cast<const f32x4 *>(sQ + row * C::LDF + st * 8 + 4 * half);
            dof[st] = *reinterpret_cast<const f32x4 *>(sdO + row * C::LDF + st * 8 + 4 * half);
        }

        for (int kc0 = 0; kc0 < S_all; kc0 += XS_KC) {
            __syncthreads();
            const bool all_rows = !one_chunk || g == 0;   // else only the token row changes
            for (int i = tid; i < XS_KC * F4; i += 256) {
                const int row = i / F4, c4 = i - row * F4;
                const int key = kc0 + row;
                if (!all_rows && key != Mc) continue;
                f32x4 a = {0.f, 0.f, 0.f, 0.f}, dd = {0.f, 0.f, 0.f, 0.f};
                if (c4 * 4 < HD) xs_load_kv(kc, kt, ldkv, d, key, Mc, c4 * 4, a, dd);
                *reinterpret_cast<f32x4 *>(sK + row * C::LDF + c4 * 4) = a;
                *reinterpret_cast<f32x4 *>(sV + row * C::LDF + c4 * 4) = dd;
            }
            __syncthreads();
            const int tiles = (min(S_all - kc0, XS_KC) + 31) / 32;
            for (int kt_ = 0; kt_ < tiles; ++kt_) {
                f32x16 pT, dsT;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    pT[r] = 0.f;
                    dsT[r] = 0.f;
                }
                if (wave_active) {
                    const float *kp = sK + (kt_ * 32 + l31) * C::LDF + 4 * half;
                    const float *vp = sV + (kt_ * 32 + l31) * C::LDF + 4 * half;
#pragma unroll
                    for (int st = 0; st < C::KSTEPS; ++st) {
                        const f32x4 kf = *reinterpret_cast<const f32x4 *>(kp + st * 8);
                        const f32x4 vf = *reinterpret_cast<const f32x4 *>(vp + st * 8);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            pT = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j], qf[st][j], pT, 0, 0, 0);     // S^T
                            dsT = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[j], dof[st][j], dsT, 0, 0, 0);  // dP^T
                        }
                    }
                    f32x4 dm[4];
                    if constexpr (DROP) {
                        const unsigned long mrow = ((unsigned long)b * heads + h) * T + (q_ok ? qi : 0);
                        const unsigned long wq = (unsigned long)((S_all + 3) >> 2);
#pragma unroll
                        for (int gg = 0; gg < 4; ++gg) dm[gg] = dropout_quad(da, mrow * wq + (unsigned long)((kc0 + kt_ * 32 + 8 * gg + 4 * half) >> 2));
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = kc0 + kt_ * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        const float p = (key < S_all && q_ok) ? exp2f(pT[r] * sl2e - lse) : 0.f;
                        if constexpr (DROP) {
                            const float mk = dm[r >> 2][r & 3];
                            pT[r] = p * mk;
                            dsT[r] = p * (dsT[r] * mk - delta) * scale;
                        } else {
                            pT[r] = p;
                            dsT[r] = p * (dsT[r] - delta) * scale;
                        }
                    }
                    // dQ^T += K^T dS^T
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int krow = kt_ * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
#pragma unroll
                        for (int ft = 0; ft < C::FT; ++ft) {
                            const float a = sK[krow * C::LDF + ft * 32 + l31];
                            dqT[ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, dsT[r], dqT[ft], 0, 0, 0);
                        }
                    }
                }
                // P^T / dS^T tiles -> LDS [32 keys][XS_QP queries]
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int krow = (r & 3) + 8 * (r >> 2) + 4 * half;
                    sP[krow * C::LDP + q0 + l31] = pT[r];
                    sdS[krow * C::LDP + q0 + l31] = dsT[r];
                }
                __syncthreads();
                // dV tile (32 keys x 32 features) = P^T dO ; dK tile = dS^T Q ; 2 * FT jobs over 4 waves
                for (int job = wave; job < 2 * C::FT; job += 4) {
                    const bool is_dk = job >= C::FT;
                    const int ft = is_dk ? job - C::FT : job;
                    const float *aT = is_dk ? sdS : sP;
                    const float *bM = is_dk ? sQ : sdO;
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
                    for (int kq = 0; kq < q_rows; kq += 8) {
                        const f32x4 af = *reinterpret_cast<const f32x4 *>(aT + l31 * C::LDP + kq + 4 * half);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float bf = bM[(kq + 4 * half + j) * C::LDF + ft * 32 + l31];
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j], bf, acc, 0, 0, 0);
                        }
                    }
                    const int f = ft * 32 + l31;
                    if (f < HD) {
                        const int col = (is_dk ? 0 : d) + f;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int key = kc0 + kt_ * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                            if (key < Mc) {
                                // this lane owns the element over all K draws: they are added in draw order
                                float *pd = dkc + (long)key * ldkv + col;
                                *pd = (g == 0) ? acc[r] : *pd + acc[r];
                            } else if (key == Mc) {
                                dkt[col] = acc[r];   // the draw's own token row
                            }
                        }
                    }
                }
                __syncthreads();
            }
        }
        if (q_ok) {
            float *op = dq + ((long)b * T + qi) * d + h * HD;
#pragma unroll
            for (int ft = 0; ft < C::FT; ++ft)
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) {
                    const int f = ft * 32 + 8 * gg + 4 * half;
                    if (f < HD) {
                        f32x4 t = {dqT[ft][4 * gg], dqT[ft][4 * gg + 1], dqT[ft][4 * gg + 2], dqT[ft][4 * gg + 3]};
                        *reinterpret_cast<f32x4 *>(op + f) = t;
                    }
                }
        }
    }
}

// out[b] = in[b / K] over rows of `row` floats (a multiple of 4): the context rows of the trajectories of a group
__global__ __launch_bounds__(256) void expand_rows_kernel(const f32x4 *__restrict__ in, f32x4 *__restrict__ out, long n4_out, long row4, int K) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4_out; i += (long)gridDim.x * 256) {
        const long b = i / row4, e = i - b * row4;
        out[i] = in[(b / K) * row4 + e];
    }
}
// out[c] = sum over g < K of in[c * K + g], in draw order
__global__ __launch_bounds__(256) void expand_rows_bwd_kernel(const f32x4 *__restrict__ in, f32x4 *__restrict__ out, long n4_out, long row4, int K) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4_out; i += (long)gridDim.x * 256) {
        const long c = i / row4, e = i - c * row4;
        f32x4 acc = in[(c * K) * row4 + e];
        for (int g = 1; g < K; ++g) acc += in[(c * K + g) * row4 + e];
        out[i] = acc;
    }
}

bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int shape_ok(int d, int heads, int T, int Mc) {
    if (d <= 0 || heads <= 0 || d % heads != 0) return 0;
    const int hd = d / heads;
    return (hd == 16 || hd == 32 || hd == 64) && T >= 1 && T <= XS_MAX_T && Mc >= 1;
}

}   // namespace

extern "C" int sd_train_xattn_shared_ok(int d, int heads, int T, int Mc) { return shape_ok(d, heads, T, Mc); }

extern "C" int sd_train_xattn_shared_fwd(const float *q, const float *kv_ctx, const float *kv_tok, float *out, float *lse2, int C, int K,
                                         int T, int Mc, int d, int heads, float p, uint64_t seed, uint64_t site, void *stream) {
    if (!q || !kv_ctx || !kv_tok || !out || !lse2 || C <= 0 || K <= 0 || !al16(q) || !al16(kv_ctx) || !al16(kv_tok) || !al16(out))
        return fail(SD_E_BADARG, "sd_train_xattn_shared_fwd: null or misaligned pointer, or empty shape");
    if (!(p >= 0.f) || !(p < 1.f)) return fail(SD_E_BADARG, "sd_train_xattn_shared_fwd: p must be in [0, 1)");
    if (!shape_ok(d, heads, T, Mc))
        return fail(SD_E_UNSUPPORTED, "sd_train_xattn_shared_fwd: head dim 16, 32 or 64, 1 <= T <= 100, Mc >= 1");
    const DropoutArgs da = make_dropout(p, seed, site);
    const int hd = d / heads, rows_cap = (Mc + 1) >= XS_KC ? XS_KC : ((Mc + 1 + 31) / 32) * 32;
    const float sl2e = (1.0f / sqrtf((float)hd)) * 1.44269504088896340736f;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(SD_KCLASS_ATTENTION, s);
    dim3 grid((unsigned)((long)C * K * heads)), block(256);
#define SD_XSF(HD_)                                                                                                          \
    do {                                                                                                                     \
        const size_t lds = (size_t)rows_cap * (XsFwdCfg<HD_>::LDK + XsFwdCfg<HD_>::LDV) * sizeof(float);                     \
        if (da.thresh) SD_LAUNCH((xattn_shared_fwd_kernel<HD_, true>), grid, block, lds, s, q, kv_ctx, kv_tok, out, lse2, K, T, Mc, heads, sl2e, da); \
        else SD_LAUNCH((xattn_shared_fwd_kernel<HD_, false>), grid, block, lds, s, q, kv_ctx, kv_tok, out, lse2, K, T, Mc, heads, sl2e, da);          \
    } while (0)
    switch (hd) {
        case 16: SD_XSF(16); break;
        case 32: SD_XSF(32); break;
        default: SD_XSF(64); break;
    }
#undef SD_XSF
    SD_CHECK_LAUNCH("xattn_shared_fwd_kernel");
    return 0;
}

extern "C" int sd_train_xattn_shared_bwd(const float *q, const float *kv_ctx, const float *kv_tok, const float *o, const float *dO,
                                         const float *lse2, float *dq, float *dkv_ctx, float *dkv_tok, int C, int K, int T, int Mc, int d,
                                         int heads, float p, uint64_t seed, uint64_t site, void *stream) {
    if (!q || !kv_ctx || !kv_tok || !o || !dO || !lse2 || !dq || !dkv_ctx || !dkv_tok || C <= 0 || K <= 0 || !al16(q) || !al16(kv_ctx) ||
        !al16(kv_tok) || !al16(o) || !al16(dO) || !al16(dq))
        return fail(SD_E_BADARG, "sd_train_xattn_shared_bwd: null or misaligned pointer, or empty shape");
    if (int rc = (!(p >= 0.f) || !(p < 1.f)) ? fail(SD_E_BADARG, "sd_train_xattn_shared_bwd: p must be in [0, 1)") : 0) return rc;
    if (!shape_ok(d, heads, T, Mc))
        return fail(SD_E_UNSUPPORTED, "sd_train_xattn_shared_bwd: head dim 16, 32 or 64, 1 <= T <= 100, Mc >= 1");
    const DropoutArgs da = make_dropout(p, seed, site);
    const int hd = d / heads;
    const float scale = 1.0f / sqrtf((float)hd);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(SD_KCLASS_ATTENTION, s);
    dim3 grid((unsigned)((long)C * heads)), block(256);
#define SD_XSB(HD_)                                                                                                          \
    do {                                                                                                                     \
        auto kfn = da.thresh ? xattn_shared_bwd_kernel<HD_, true> : xattn_shared_bwd_kernel<HD_, false>;                     \
        const size_t lds = XsBwdCfg<HD_>::LDS_BYTES;                                                                         \
        static DevFlag attr_set[2];                                                                                          \
        if (lds > 64 * 1024 && !attr_set[da.thresh ? 1 : 0]) {                                                               \
            (void)hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);              \
            attr_set[da.thresh ? 1 : 0] = true;                                                                              \
        }                                                                                                                    \
        SD_LAUNCH(kfn, grid, block, lds, s, q, kv_ctx, kv_tok, o, dO, lse2, dq, dkv_ctx, dkv_tok, K, T, Mc, heads, scale, da); \
    } while (0)
    switch (hd) {
        case 16: SD_XSB(16); break;
        case 32: SD_XSB(32); break;
        default: SD_XSB(64); break;
    }
#undef SD_XSB
    SD_CHECK_LAUNCH("xattn_shared_bwd_kernel");
    return 0;
}

extern "C" int sd_train_expand_rows(const float *in, float *out, long C, int K, long row, void *stream) {
    if (!in || !out || C <= 0 || K <= 0 || row <= 0 || row % 4 || !al16(in) || !al16(out))
        return fail(SD_E_BADARG, "sd_train_expand_rows: 16-byte aligned rows of a multiple of 4 floats");
    const long n4 = C * K * (row / 4);
    SD_LAUNCH(expand_rows_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const f32x4 *>(in),
              reinterpret_cast<f32x4 *>(out), n4, row / 4, K);
    SD_CHECK_LAUNCH("expand_rows_kernel");
    return 0;
}

extern "C" int sd_train_expand_rows_bwd(const float *dout, float *din, long C, int K, long row, void *stream) {
    if (!dout || !din || C <= 0 || K <= 0 || row <= 0 || row % 4 || !al16(dout) || !al16(din))
        return fail(SD_E_BADARG, "sd_train_expand_rows_bwd: 16-byte aligned rows of a multiple of 4 floats");
    const long n4 = C * (row / 4);
    SD_LAUNCH(expand_rows_bwd_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const f32x4 *>(dout),
              reinterpret_cast<f32x4 *>(din), n4, row / 4, K);
    SD_CHECK_LAUNCH("expand_rows_bwd_kernel");
    return 0;
}
