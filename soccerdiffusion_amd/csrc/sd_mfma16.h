// Device primitives of the kernels built on v_mfma_f32_16x16x32_f16 with split fp16 operands (sd_traj.h, sd_trajg.hip, sd_swin.hip):
// the MFMA itself, the three-product form, the hi / lo split of an accumulator and the reductions over an accumulator tile's rows.
#pragma once
#include "sd_common.h"

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
// c += (ah + al) (bh + bl) without lo.lo, small terms first
__device__ __forceinline__ void mma3(f32x4 &c, f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl) {
    c = mfma16(al, bh, c);
    c = mfma16(ah, bl, c);
    c = mfma16(ah, bh, c);
}

// all-reduce over the four 16-lane rows of a wave (lanes t, t+16, t+32, t+48): two v_permlane*_swap, no LDS round trip.
// (__builtin_amdgcn_permlane32_swap(v, v) folds its two results into one on ROCm 7.2: inline assembly, checked on gfx950
// by tools/exp/perm_test.hip.)
__device__ __forceinline__ float rows4_sum(float v) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    v = a + b;
    a = v;
    b = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return a + b;
}
__device__ __forceinline__ float rows4_max(float v) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    v = fmaxf(a, b);
    a = v;
    b = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}

// x (already scaled) as hi = fp16(x), lo = fp16(x - hi): v_cvt_pk_f16_f32 both ways, 3 VALU instructions per element
__device__ __forceinline__ void split4(const f32x4 &x, f16x4 &h, f16x4 &l) {
    h = __builtin_convertvector(x, f16x4);
    l = __builtin_convertvector(x - __builtin_convertvector(h, f32x4), f16x4);
}
__device__ __forceinline__ void split_store(char *hi_at, char *lo_at, const f32x4 &v) {
    f16x4 h, l;
    split4(v, h, l);
    *reinterpret_cast<f16x4 *>(hi_at) = h;
    *reinterpret_cast<f16x4 *>(lo_at) = l;
}

__device__ __forceinline__ f16x8 lds16(const char *p) { return *reinterpret_cast<const f16x8 *>(p); }
