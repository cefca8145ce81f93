// nrc_chain8.h — the FP8 (OCP e4m3fn) chain of the width-64 inference kernel (nrc_infer8.hip) for TILES 32-query
// tiles, shared with the kernels built around it outside that unit (nrc_infer_culled.hip): layer 0 on 32x32x16 f16
// MFMAs, the hidden layers and the output layer on v_mfma_scale_f32_32x32x64_f8f6f4, the accumulators packed into the
// next layer's operand in register order, so the radiance is bit-identical to nrc_infer's on an FP8 handle. Weights:
// the LDS image of infer8_kernel (10 layer-0 f16 fragments, then 9 FP8 fragments).
#pragma once

#include "nrc_device.h"

namespace nrc_amd {

typedef __attribute__((address_space(3))) const h8 lds_h8;
// hide the LDS image base from loop-invariant code motion: fragments are re-read per layer, not hoisted into VGPRs
__device__ __forceinline__ lds_h8* launder8(lds_h8* p) {
    asm volatile("" : "+v"(p));
    return p;
}

constexpr int kL0H8 = 10 * 64;               // h8 (16-byte) units of the layer-0 f16 fragments
constexpr int kImg8H8 = kInfer8ImgBytes / 16;  // ... of the FP8 fragments

// FP8 fragment f of the lane: its two planes as one 32-byte operand
__device__ __forceinline__ i8v frag8(lds_h8* wl, int f) {
    typedef int i4v __attribute__((ext_vector_type(4)));
    const h8 lo = wl[kL0H8 + 2 * f * 64], hi = wl[kL0H8 + (2 * f + 1) * 64];
    return (i8v)__builtin_shufflevector(__builtin_bit_cast(i4v, lo), __builtin_bit_cast(i4v, hi), 0, 1, 2, 3, 4, 5, 6, 7);
}

// ReLU + e4m3 of a layer's two accumulators, in register order (byte j = register j & 15 of block j >> 4): the scaled
// convert saturates at 448 under MODE.FP16_OVFL, the ReLU zeroes the bytes whose sign bit is set (-0 included); 3 VALU
// per 4 values. The first convert's "old" operand is the previous group's shifted word, a register that dies there.
__device__ __forceinline__ i8v pack8(const f16v (&c)[2]) {
    i8v y;
    uint32_t spare = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const f16v& cc = c[d >> 2];
        const int q = d & 3;
        const uint32_t lo = cvt_sat_fp8<false>(cc[4 * q + 0], cc[4 * q + 1], spare);
        const uint32_t w = cvt_sat_fp8<true>(cc[4 * q + 2], cc[4 * q + 3], lo);
        const uint32_t sh = w << 8;
        y[d] = (int)relu_e4m3x4(w, sh);
        spare = sh;
    }
    return y;
}

// the whole chain for TILES tiles; every weight fragment read from LDS feeds all of them
template <int TILES>
__device__ __forceinline__ void mlp8(lds_h8* lw_lane, const h8 (&x)[TILES][5], const uint32_t (&sc)[5], f16v (&o)[TILES]) {
    f16v c[TILES][2];
    i8v y[TILES];
    {
        lds_h8* wl = launder8(lw_lane);
#pragma unroll
        for (int t = 0; t < TILES; ++t) c[t][0] = c[t][1] = zero16();
#pragma unroll
        for (int kk = 0; kk < 5; ++kk) {
            const h8 a0 = wl[fwd_frag(0, 0, kk) * 64], a1 = wl[fwd_frag(0, 1, kk) * 64];
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                c[t][0] = mfma(a0, x[t][kk], c[t][0]);
                c[t][1] = mfma(a1, x[t][kk], c[t][1]);
            }
        }
#pragma unroll
        for (int t = 0; t < TILES; ++t) y[t] = pack8(c[t]);
    }
#pragma unroll
    for (int l = 1; l < 5; ++l) {
        lds_h8* wl = launder8(lw_lane);
        const i8v a0 = frag8(wl, infer8_frag(l, 0)), a1 = frag8(wl, infer8_frag(l, 1));
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            c[t][0] = mfma_fp8<0>(a0, y[t], zero16(), sc[l - 1]);
            c[t][1] = mfma_fp8<1>(a1, y[t], zero16(), sc[l - 1]);
        }
#pragma unroll
        for (int t = 0; t < TILES; ++t) y[t] = pack8(c[t]);
    }
    lds_h8* wl = launder8(lw_lane);
    const i8v a5 = frag8(wl, infer8_frag(5, 0));
#pragma unroll
    for (int t = 0; t < TILES; ++t) o[t] = mfma_fp8<0>(a5, y[t], zero16(), sc[4]);
}

}  // namespace nrc_amd
