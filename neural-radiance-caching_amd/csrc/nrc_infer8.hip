// nrc_infer8.hip — FP8 (OCP e4m3fn) inference of the reference's 64-wide network (NRCNetworkConfigs.h:26-33) on
// v_mfma_scale_f32_32x32x64_f8f6f4, InputEncoding::Frequency, compact queries (DESIGN.md §12 "width 64").
// Numerics: the width-128 FP8 contract (oracle/nrc_wide_oracle.c:15-22) at width 64 -- layer 0 f16 x f16 with f32
// accumulation; the ReLU outputs of layers 0..4 saturated at 448 and rounded (RNE) onto e4m3; W1..W5 e4m3 with one
// power-of-two scale per output row (the MX scale-A byte); the final ReLU output rounded through f16.
//
// Operand chain. One wave = 32 queries on the MFMA column axis, lane (n, h) = (lane & 31, lane >> 5). A layer's 64
// outputs are two 32x32 f32 accumulators (M-blocks 0, 1); register i of lane (n, h) of block mb is row
// 32 mb + 8 (i >> 2) + 4 h + (i & 3) of query n. Those 2 x 16 values, converted to bytes in register order, ARE the
// 32-byte B operand of the next layer's single K = 64 step for lane (n, h): byte j = row f8_row64(h, j). The MX MFMA
// pairs byte j of A-lane (r, h) with byte j of B-lane (n, h), so the weight image stores W[32 mb + r][f8_row64(h, j)]
// at byte j of lane (r, h) and nothing moves across lanes. A hidden layer is 2 MFMAs (8 of 32x32x16 f16), 8 VGPRs of B.
//
// Output layer: one 32x32x64 MX MFMA whose A rows 16..31 are zero (W5 has 16 padded rows, 3 used). The activations are
// already the B operand; every narrower shape (16x16x128, 4x4x4 f16) wants another lane layout or f16 operands, i.e.
// cross-lane movement or a second conversion per value, for an MFMA that is 2 of the chain's ~28 f16 equivalents.
//
// LDS (28 KiB + 4 B): the 10 layer-0 f16 fragments of the handle's f16 image, then 9 FP8 fragments of 2 KiB (L1..L4
// x 2 M-blocks, L5), each two 1-KiB planes (bytes 0-15 / 16-31 of every lane's operand, lane-linear: one conflict-free
// ds_read_b128 per plane). The per-lane E8M0 scale words (5, byte mb = row 32 mb + r via op_sel) stay in VGPRs.
//
// Work split: persistent blocks, one per CU slot; a block owns a contiguous range of tile groups and its waves draw
// from an LDS counter one group ahead (as variant 47 of the f16 kernel). TILES = tiles per wave iteration: the
// product shape and the A/B loser are named at launch_infer8.
#include "nrc_chain8.h"

namespace nrc_amd {
namespace {

// fused accumulate_render_radiance (nrc_helpers.cu:77-129) for queries [0, n_acc): as InferEpilogue of nrc_kernels.hip
// (factored modes: thr is not read in mode 4 and may be null)
struct Accum8 {
    const float* thr;
    float4* rgba;
    int64_t n_acc;
    float w;
};

// EPI -1 plain, 0 / 2 fused accumulate_render_radiance (RenderMode Full / CacheOnly) for queries [0, n_acc).
// EPI kInfer8Factored + 0 / 2 / 4: the same with USE_REFLECTANCE_FACTORING 1 (accumulate_kernel<MODE, true> of nrc_frame.hip,
// operation for operation; 4 = DebugCacheNoThroughputModulation, the factored copy_radiance_to_output_buffer). The
// reflectance diffuse + specular comes from the tile's QLane registers (reflectance_half0) before the prefetch
// overwrites them: no memory traffic, three registers per tile live across the MLP.
// wf: the handle's f16 inference image (its first 10 fragments are layer 0); img8: FP8 fragments + scale words.
template <int EPI, int TILES, int THREADS>
__global__ __launch_bounds__(THREADS, 1) void infer8_kernel(const float* __restrict__ q, float* __restrict__ out,
                                                             int64_t n, const h8* __restrict__ wf,
                                                             const h8* __restrict__ img8, Accum8 epi) {
    __shared__ __attribute__((aligned(16))) h8 lw[kL0H8 + kImg8H8];
    __shared__ uint32_t wq_next;
    constexpr bool RF = EPI >= kInfer8Factored;
    constexpr int MODE = RF ? EPI - kInfer8Factored : EPI;  // the RenderMode of the epilogue (-1: none)
    fp32_flush_output_denorms();  // as the f16 kernel (same layer-0 / encoder arithmetic)
    fp8_saturating_converts();    // pack8
    for (int i = threadIdx.x; i < kL0H8; i += THREADS) lw[i] = wf[i];
    for (int i = threadIdx.x; i < kImg8H8; i += THREADS) lw[kL0H8 + i] = img8[i];
    if (threadIdx.x == 0) wq_next = 0;
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int h = lane >> 5, r = lane & 31;
    uint32_t sc[5];
    {
        const uint32_t* scales = reinterpret_cast<const uint32_t*>(img8 + kImg8H8);
#pragma unroll
        for (int l = 0; l < 5; ++l) sc[l] = scales[l * 32 + r];
    }
    const int64_t ntiles = (n + 31) >> 5, ngroups_all = (ntiles + TILES - 1) / TILES;
    const int64_t gbase = (int64_t)blockIdx.x * ngroups_all / gridDim.x;
    const int64_t gend = (int64_t)(blockIdx.x + 1) * ngroups_all / gridDim.x;  // end of this block's range
    uint32_t t0 = 0;
    if (lane == 0) t0 = atomicAdd(&wq_next, 1u);
    int64_t g = gbase + (int64_t)__builtin_amdgcn_readfirstlane(t0);
    if (g >= gend) return;
    if (lane == 0) t0 = atomicAdd(&wq_next, 1u);
    int64_t ng = gbase + (int64_t)__builtin_amdgcn_readfirstlane(t0);
    uint32_t nn_raw = 0;
    const int64_t last = n - 1;
    QLane Q[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) Q[t] = load_q(q, min((g * TILES + t) * 32 + r, last), h);
    // stores that the hardware drops (empty descriptors): the loop is entered with the back-edge's vmcnt pattern
    if constexpr (EPI >= 0) __builtin_amdgcn_raw_buffer_store_b128(u4{0u, 0u, 0u, 0u}, buffer_rsrc(out, 0), 0, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b96(u3{0u, 0u, 0u}, buffer_rsrc(out, 0), 0, 0, 0);
    for (bool first = true; g < gend; first = false) {
        if (!first) {
            // the draw issued one iteration ago (an asm readfirstlane stays here; the builtin would be hoisted to the
            // atomic and the wave would wait for it there)
            uint32_t t;
            asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(t) : "v"(nn_raw));
            ng = gbase + (int64_t)t;
        }
        h8 x[TILES][5];
#pragma unroll
        for (int t = 0; t < TILES; ++t) encode_v3(Q[t], h, x[t]);
        [[maybe_unused]] float R[TILES][3];
        if constexpr (RF) {
#pragma unroll
            for (int t = 0; t < TILES; ++t) reflectance_half0(Q[t], R[t]);
        }
        if (lane == 0) nn_raw = atomicAdd(&wq_next, 1u);  // the group after next
#pragma unroll
        for (int t = 0; t < TILES; ++t)
            Q[t] = load_q(q, min((ng * TILES + t) * 32 + r, last), h);  // clamped, branch-free prefetch
        // epilogue operands are fetched before the MLP so their latency hides under the MFMAs
        float tr[TILES][3] = {};
        float4 acc[TILES] = {};
        if constexpr (EPI >= 0) {
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                const int64_t s0 = (g * TILES + t) * 32;
                const int rows = tile_rows(epi.n_acc, s0);
                if constexpr (MODE != 4) {
                    const u3 tv = __builtin_amdgcn_raw_buffer_load_b96(buffer_rsrc(epi.thr + s0 * 3, rows * 12),
                                                                       h ? kBufferOff : r * 12, 0, 0);
                    typedef float f3 __attribute__((ext_vector_type(3)));
                    const f3 tf = __builtin_bit_cast(f3, tv);  // whole-vector bit_cast (clang 22 element bit_cast bug)
                    tr[t][0] = tf.x;
                    tr[t][1] = tf.y;
                    tr[t][2] = tf.z;
                }
                if constexpr (MODE == 0) {
                    const u4 av = __builtin_amdgcn_raw_buffer_load_b128(buffer_rsrc(epi.rgba + s0, rows * 16),
                                                                        h ? kBufferOff : r * 16, 0, 0);
                    acc[t] = __builtin_bit_cast(float4, av);
                }
            }
        }
        f16v o[TILES];
        mlp8<TILES>((lds_h8*)(lw + lane), x, sc, o);
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            // rows 0..2 of query r are registers 0..2 of lane half 0; ReLU, then through f16 as the f16 kernel's output
            const int64_t s0 = (g * TILES + t) * 32, sq = s0 + r;
            const float L0 = (float)(_Float16)fmaxf(o[t][0], 0.0f);
            const float L1 = (float)(_Float16)fmaxf(o[t][1], 0.0f);
            const float L2 = (float)(_Float16)fmaxf(o[t][2], 0.0f);
            bool to_out = h == 0;
            if constexpr (EPI >= 0) {
                float4 v;
                if constexpr (RF && MODE == 0) {  // Full: dst += ((T * L) * R) * w
                    v = acc[t];
                    v.x = __builtin_fmaf((tr[t][0] * L0) * R[t][0], epi.w, v.x);
                    v.y = __builtin_fmaf((tr[t][1] * L1) * R[t][1], epi.w, v.y);
                    v.z = __builtin_fmaf((tr[t][2] * L2) * R[t][2], epi.w, v.z);
                } else if constexpr (RF && MODE == 2) {  // CacheOnly: (L * T) * R
                    v.x = (L0 * tr[t][0]) * R[t][0];
                    v.y = (L1 * tr[t][1]) * R[t][1];
                    v.z = (L2 * tr[t][2]) * R[t][2];
                } else if constexpr (RF) {  // copy_radiance_to_output_buffer: L * R
                    v.x = L0 * R[t][0];
                    v.y = L1 * R[t][1];
                    v.z = L2 * R[t][2];
                } else if constexpr (EPI == 0) {  // Full: dst += (T * L) * w
                    v = acc[t];
                    v.x = __builtin_fmaf(tr[t][0] * L0, epi.w, v.x);
                    v.y = __builtin_fmaf(tr[t][1] * L1, epi.w, v.y);
                    v.z = __builtin_fmaf(tr[t][2] * L2, epi.w, v.z);
                } else {  // CacheOnly
                    v.x = L0 * tr[t][0];
                    v.y = L1 * tr[t][1];
                    v.z = L2 * tr[t][2];
                }
                v.w = 1.0f;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v),
                                                       buffer_rsrc(epi.rgba + s0, tile_rows(epi.n_acc, s0) * 16),
                                                       h ? kBufferOff : r * 16, 0, 0);
                to_out = to_out && sq >= epi.n_acc;
            }
            const u3 ov = {__builtin_bit_cast(uint32_t, L0), __builtin_bit_cast(uint32_t, L1),
                           __builtin_bit_cast(uint32_t, L2)};
            // exact-n: the descriptor ends at the tile's last valid row, rows past n are dropped by the hardware
            __builtin_amdgcn_raw_buffer_store_b96(ov, buffer_rsrc(out + s0 * NRC_OUTPUT_DIMS, tile_rows(n, s0) * 12),
                                                  to_out ? r * 12 : kBufferOff, 0, 0);
        }
        g = ng;
    }
}

// Weight pack: thread = (row unit, 4 columns); 16 threads share a row. Units 0..255 = rows of W1..W4, 256..287 = the
// output fragment's 32 rows (W5's 16 padded rows, then zeros). Row max over the 16 threads, the row exponent
// (orc_fp8_row_exponent: smallest e with max|w| <= 448 * 2^e, 0 for an all-zero row), then the permuted e4m3 bytes and
// the scale byte. No host synchronisation, no atomics: legal inside a captured graph.
constexpr int kPackUnits = 4 * 64 + 32;
__global__ __launch_bounds__(256) void pack8_kernel(const float* __restrict__ w_infer, uint8_t* __restrict__ img8) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int unit = t >> 4, c = (t & 15) * 4;
    if (unit >= kPackUnits) return;  // whole 16-thread groups
    const int layer = unit < 256 ? 1 + (unit >> 6) : 5;
    const int row = unit < 256 ? unit & 63 : unit - 256;
    float4 w = {0.0f, 0.0f, 0.0f, 0.0f};
    if (layer < 5 || row < NRC_OUT_PADDED)
        w = *reinterpret_cast<const float4*>(w_infer + NRC_W1_OFFSET + (layer - 1) * NRC_WIDTH * NRC_WIDTH + row * NRC_WIDTH + c);
    float amax = fmaxf(fmaxf(fabsf(w.x), fabsf(w.y)), fmaxf(fabsf(w.z), fabsf(w.w)));
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
    int e = 0;
    if (amax > 0.0f) {
        int E = 0;
        const float M = frexpf(amax, &E);
        e = M <= 0.875f ? E - 9 : E - 8;
        e = max(-127, min(127, e));
    }
    const float a0 = __builtin_amdgcn_fmed3f(ldexpf(w.x, -e), -448.0f, 448.0f);
    const float a1 = __builtin_amdgcn_fmed3f(ldexpf(w.y, -e), -448.0f, 448.0f);
    const float a2 = __builtin_amdgcn_fmed3f(ldexpf(w.z, -e), -448.0f, 448.0f);
    const float a3 = __builtin_amdgcn_fmed3f(ldexpf(w.w, -e), -448.0f, 448.0f);
    const uint32_t lo = __builtin_amdgcn_cvt_pk_fp8_f32(a0, a1, 0, false);
    const uint32_t wd = __builtin_amdgcn_cvt_pk_fp8_f32(a2, a3, lo, true);
    // columns c .. c + 3 = bytes j .. j + 3 of lane (r, h): the inverse of f8_row64
    const int mb = row >> 5, r = row & 31, h = (c >> 2) & 1, j = 16 * (c >> 5) + 4 * ((c >> 3) & 3);
    static_assert(f8_row64(1, 16 + 4 * 2 + 3) == 32 + 8 * 2 + 4 + 3, "f8_row64");
    const int f = infer8_frag(layer, mb);
    *reinterpret_cast<uint32_t*>(img8 + ((f * 2 + (j >> 4)) * 64 + r + 32 * h) * 16 + (j & 15)) = wd;
    if (c == 0) {  // byte mb of lane r's scale word of the layer (the other bytes stay 127 = 2^0 from allocation)
        const int word = (layer - 1) * 32 + r;
        img8[kInfer8ImgBytes + word * 4 + (layer < 5 ? mb : 0)] = (uint8_t)(e + 127);
    }
}

int num_cus8() {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
        v = 256;
    return v;
}

template <int EPI, int TILES, int THREADS>
hipError_t launch8(const float* queries, float* out, int64_t n, const _Float16* wf, const uint8_t* img8,
                   const Accum8& epi, hipStream_t s) {
    static int bpc = 0;  // resident blocks per CU of this shape
    if (!bpc) {
        int v = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, infer8_kernel<EPI, TILES, THREADS>, THREADS, 0) !=
                hipSuccess || v <= 0)
            v = 1;
        bpc = v;
    }
    const int64_t ngroups = ((n + 31) / 32 + TILES - 1) / TILES;
    const int64_t want = (ngroups + THREADS / 64 - 1) / (THREADS / 64), cap = (int64_t)num_cus8() * bpc;
    hipLaunchKernelGGL((infer8_kernel<EPI, TILES, THREADS>), dim3((unsigned)(want < cap ? want : cap)), dim3(THREADS),
                       0, s, queries, out, n, reinterpret_cast<const h8*>(wf), reinterpret_cast<const h8*>(img8), epi);
    return hipGetLastError();
}

template <int TILES, int THREADS>
hipError_t launch8_modes(const float* queries, float* out, int64_t n, const _Float16* wf, const uint8_t* img8,
                         const Accum8& epi, int mode, hipStream_t s) {
    switch (mode) {
        case -1: return launch8<-1, TILES, THREADS>(queries, out, n, wf, img8, epi, s);
        case 0: return launch8<0, TILES, THREADS>(queries, out, n, wf, img8, epi, s);
        case 2: return launch8<2, TILES, THREADS>(queries, out, n, wf, img8, epi, s);
        case kInfer8Factored + 0: return launch8<kInfer8Factored + 0, TILES, THREADS>(queries, out, n, wf, img8, epi, s);
        case kInfer8Factored + 2: return launch8<kInfer8Factored + 2, TILES, THREADS>(queries, out, n, wf, img8, epi, s);
        case kInfer8Factored + 4: return launch8<kInfer8Factored + 4, TILES, THREADS>(queries, out, n, wf, img8, epi, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_pack8(const float* w_infer, uint8_t* img8, hipStream_t s) {
    hipLaunchKernelGGL(pack8_kernel, dim3(kPackUnits * 16 / 256), dim3(256), 0, s, w_infer, img8);
    return hipGetLastError();
}

hipError_t launch_infer8(int variant, const float* queries, float* out, int64_t n, const _Float16* wf,
                         const uint8_t* img8, const float* thr, float* rgba, int64_t n_acc, int mode, float w,
                         hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const Accum8 epi{thr, reinterpret_cast<float4*>(rgba), n_acc, w};
    // product shape: one tile per wave iteration, 1024-thread blocks (4 waves per SIMD)
    if (variant == 0) return launch8_modes<1, 1024>(queries, out, n, wf, img8, epi, mode, s);
#if NRC_DEBUG_KERNELS  // the A/B loser: two tiles per wave iteration in 512-thread blocks, debug library
    if (variant == 1 && mode == -1) return launch8<-1, 2, 512>(queries, out, n, wf, img8, epi, s);
    return hipErrorInvalidValue;
#else
    return hipErrorNotSupported;
#endif
}

}  // namespace nrc_amd
