// nrc_chain47.h — the f16 chain of the product inference kernel (variant 47 of nrc_kernels.hip) for one 32-query tile,
// shared by the kernels built around it outside that unit (nrc_infer_sparse.hip, nrc_infer_factored.hip,
// nrc_infer_culled.hip): the same 32x32x16 f16 MFMAs in the same K order per layer, the 4x4x4 output layer and the
// permlane32 half sums, so the radiance is bit-identical to nrc_infer's. Weights: the handle's f16 inference image,
// resident in LDS.
#pragma once

#include "nrc_device.h"

namespace nrc_amd {

typedef __attribute__((address_space(3))) const h8 lds_h8;
// hide the LDS image base from loop-invariant code motion: fragments are re-read per layer, not hoisted into VGPRs
__device__ __forceinline__ lds_h8* launder_s(lds_h8* p) {
    asm volatile("" : "+v"(p));
    return p;
}

// ReLU of 8 accumulator registers as the next layer's f16 B operand (relu_h8 of nrc_kernels.hip)
__device__ __forceinline__ h8 relu_pack(const f16v& a, int base) {
    h8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)a[base + j];
    const h8 z = {};
    return __builtin_elementwise_max(v, z);
}

// one hidden layer of variant 47: k-steps in ascending order, M-block 0 then 1 inside a step
template <int KK>
__device__ __forceinline__ void hidden_layer(lds_h8* lw_lane, int layer, const h8 (&in)[KK], h8 (&y)[4]) {
    lds_h8* wl = launder_s(lw_lane);
    h8 a[2][KK];
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        a[0][kk] = wl[fwd_frag(layer, 0, kk) * 64];
        a[1][kk] = wl[fwd_frag(layer, 1, kk) * 64];
    }
    f16v c0 = zero16(), c1 = zero16();
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        c0 = mfma(a[0][kk], in[kk], c0);
        c1 = mfma(a[1][kk], in[kk], c1);
    }
    y[0] = relu_pack(c0, 0);
    y[1] = relu_pack(c0, 8);
    y[2] = relu_pack(c1, 0);
    y[3] = relu_pack(c1, 8);
}

// The chain of one tile; L0..L2 = the radiance of query lane % 32 (valid in lane half 0), through f16 as the dense
// kernel's output. Output layer on v_mfma_f32_4x4x4_16b_f16 and the permlane32 half sums: mlp_tiles / the ABL 65536
// epilogue of nrc_kernels.hip, operation for operation.
__device__ __forceinline__ void chain47(lds_h8* lw_lane, const h8 (&x)[5], float& L0, float& L1, float& L2) {
    h8 y[4], z[4];
    hidden_layer<5>(lw_lane, 0, x, y);
#pragma unroll
    for (int l = 1; l < 5; ++l) {
        hidden_layer<4>(lw_lane, l, y, z);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) y[kk] = z[kk];
    }
    const int ln = threadIdx.x & 63;
    lds_h8* w4 = launder_s(lw_lane + (((ln & 3) | (ln & 32)) - ln));
    f4v c4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const h8 a = w4[fwd_frag(5, 0, kk) * 64];
        c4 = __builtin_amdgcn_mfma_f32_4x4x4f16(__builtin_shufflevector(a, a, 0, 1, 2, 3),
                                                __builtin_shufflevector(y[kk], y[kk], 0, 1, 2, 3), c4, 0, 0, 0);
        c4 = __builtin_amdgcn_mfma_f32_4x4x4f16(__builtin_shufflevector(a, a, 4, 5, 6, 7),
                                                __builtin_shufflevector(y[kk], y[kk], 4, 5, 6, 7), c4, 0, 0, 0);
    }
    const u4 ob = __builtin_bit_cast(u4, c4);
    const auto s01 = __builtin_amdgcn_permlane32_swap(ob[0], ob[1], false, false);
    const auto s23 = __builtin_amdgcn_permlane32_swap(ob[2], ob[3], false, false);
    const f2 p01 = __builtin_bit_cast(f2, s01), p23 = __builtin_bit_cast(f2, s23);
    const float A = p01[0] + p01[1];
    const float B = p23[0] + p23[1];
    const h2 zero = {};
    const h2 ab = __builtin_elementwise_max(__builtin_bit_cast(h2, pk2(A, B)), zero);
    const float LA = (float)ab[0], LB = (float)ab[1];
    const uint32_t la = __builtin_bit_cast(uint32_t, LA);
    const auto s11 = __builtin_amdgcn_permlane32_swap(la, la, false, false);
    L0 = LA;
    L1 = __builtin_bit_cast(f2, s11)[1];
    L2 = LB;
}

}  // namespace nrc_amd
