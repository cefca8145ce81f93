// nrc_infer_factored.hip — inference with the reflectance-factored accumulate_render_radiance fused into its epilogue
// (nrc_infer_accumulate_factored, DESIGN.md §9 "Fused factored accumulation"): USE_REFLECTANCE_FACTORING 1 of the
// reference (nrc_helpers.cu:66-68, 95-97, 111-113, 118-120). Width 64, InputEncoding::Frequency, NRC_PRECISION_F16,
// compact queries. (FP8 handles: the factored EPI values of infer8_kernel, nrc_infer8.hip.)
//
// For a render query i < n_acc the frame buffer receives what accumulate_kernel<MODE, true> (nrc_frame.hip) computes
// from nrc_infer's radiance L, the throughput T and the query's reflectance R = diffuse + specular:
//   Full (0)       dst.c = fmaf((T.c * L.c) * R.c, w, dst.c)
//   CacheOnly (2)  dst.c = (L.c * T.c) * R.c
//   mode 4         dst.c = L.c * R.c          (the factored copy_radiance_to_output_buffer; T is never read)
// and dst.w = 1, by the same float operations in the same order; its radiance is not written. Queries [n_acc, n) go
// to out as nrc_infer writes them. The chain is variant 47's (nrc_chain47.h), so L is bit-identical to nrc_infer.
//
// Reflectance without memory traffic. The wave that runs a tile already holds both halves of R: QLane::i0..i2 of
// lane (r, 0) = diffuse (floats 9..11) of query r, of lane (r, 1) = specular (12..14). After the encoder has consumed
// the tile's QLane, three v_permlane32_swap bring specular to lane half 0 and three adds make R there; only then is
// the QLane overwritten by the next tile's prefetch. The three R registers are what stays live across the chain (not a
// second QLane), and the swaps and adds issue before the first MFMA.
//
// Work split (as infer8_kernel): persistent 1024-thread blocks, one per CU slot; a block owns the contiguous tile
// range [b nt / G, (b + 1) nt / G) and its waves draw tiles from an LDS counter one tile ahead. The next tile's
// load_q is a clamped, branch-free prefetch; throughput (12 B per row) and, for Full, the pixel (16 B per row) are
// fetched before the chain through descriptors clamped to the tile's rows below n_acc; the stores are exact-n buffer
// stores (rows past n_acc / n are dropped by the hardware). Row indices are 64-bit.
//
// LDS: the 46 KiB f16 weight image + the tile counter. 90 VGPRs (Full; 87 CacheOnly, 83 mode 4), no scratch: the 4
// waves per SIMD of a 1024-thread block fit (<= 128), two blocks per CU.
#include "nrc_chain47.h"

namespace nrc_amd {
namespace {

constexpr int kThreads = 1024;

struct FactoredEpilogue {
    const float* thr;  // [n_acc] float3 lastRenderThroughput (mode 4: not read, may be null)
    float4* rgba;      // [n_acc] frame buffer
    int64_t n_acc;
    float w;  // 1 / (iterationIndex + 1)
};

// MODE 0 / 2 / 4: RenderMode Full / CacheOnly / DebugCacheNoThroughputModulation
template <int MODE>
__global__ __launch_bounds__(kThreads, 1) void infer_factored_kernel(const float* __restrict__ q,
                                                                     float* __restrict__ out, int64_t n,
                                                                     const h8* __restrict__ wf, FactoredEpilogue epi) {
    __shared__ __attribute__((aligned(16))) h8 lw[kFwdFrags * 64];
    __shared__ uint32_t wq_next;
    fp32_flush_output_denorms();  // as the dense kernel (same encoder and epilogue arithmetic)
    for (int i = threadIdx.x; i < kFwdFrags * 64; i += kThreads) lw[i] = wf[i];
    if (threadIdx.x == 0) wq_next = 0;
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int h = lane >> 5, r = lane & 31;
    const int64_t ntiles = (n + 31) >> 5;
    const int64_t gbase = (int64_t)blockIdx.x * ntiles / gridDim.x;
    const int64_t gend = (int64_t)(blockIdx.x + 1) * ntiles / gridDim.x;  // end of this block's range
    uint32_t t0 = 0;
    if (lane == 0) t0 = atomicAdd(&wq_next, 1u);
    int64_t g = gbase + (int64_t)__builtin_amdgcn_readfirstlane(t0);
    if (g >= gend) return;
    if (lane == 0) t0 = atomicAdd(&wq_next, 1u);
    int64_t ng = gbase + (int64_t)__builtin_amdgcn_readfirstlane(t0);
    uint32_t nn_raw = 0;
    const int64_t last = n - 1;
    QLane Q = load_q(q, min(g * 32 + r, last), h);
    // stores that the hardware drops (empty descriptors): the loop is entered with the back-edge's vmcnt pattern, so
    // the wait for the prefetched queries at its head does not also wait for the previous tile's stores
    __builtin_amdgcn_raw_buffer_store_b128(u4{0u, 0u, 0u, 0u}, buffer_rsrc(out, 0), 0, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b96(u3{0u, 0u, 0u}, buffer_rsrc(out, 0), 0, 0, 0);
    for (bool first = true; g < gend; first = false) {
        if (!first) {
            // the draw issued one iteration ago (an asm readfirstlane stays here; the builtin would be hoisted to the
            // atomic and the wave would wait for it there)
            uint32_t t;
            asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(t) : "v"(nn_raw));
            ng = gbase + (int64_t)t;
        }
        h8 x[5];
        encode_v3(Q, h, x);
        float R[3];
        reflectance_half0(Q, R);  // from the finished tile's registers, before the prefetch takes them
        if (lane == 0) nn_raw = atomicAdd(&wq_next, 1u);  // the tile after next
        Q = load_q(q, min(ng * 32 + r, last), h);         // clamped, branch-free prefetch
        // epilogue operands are fetched before the chain so their latency hides under the MFMAs
        const int64_t s0 = g * 32;
        const int rows = tile_rows(epi.n_acc, s0);  // render queries of the tile
        float tr[3] = {};
        float4 acc = {};
        if constexpr (MODE != 4) {
            const u3 tv = __builtin_amdgcn_raw_buffer_load_b96(buffer_rsrc(epi.thr + s0 * 3, rows * 12),
                                                               h ? kBufferOff : r * 12, 0, 0);
            typedef float f3 __attribute__((ext_vector_type(3)));
            const f3 tf = __builtin_bit_cast(f3, tv);  // whole-vector bit_cast (clang 22 element bit_cast bug)
            tr[0] = tf.x;
            tr[1] = tf.y;
            tr[2] = tf.z;
        }
        if constexpr (MODE == 0) {
            const u4 av = __builtin_amdgcn_raw_buffer_load_b128(buffer_rsrc(epi.rgba + s0, rows * 16),
                                                                h ? kBufferOff : r * 16, 0, 0);
            acc = __builtin_bit_cast(float4, av);
        }
        float L0, L1, L2;
        chain47((lds_h8*)(lw + lane), x, L0, L1, L2);
        float4 v;
        if constexpr (MODE == 0) {  // Full: dst += ((T * L) * R) * w
            v = acc;
            v.x = __builtin_fmaf((tr[0] * L0) * R[0], epi.w, v.x);
            v.y = __builtin_fmaf((tr[1] * L1) * R[1], epi.w, v.y);
            v.z = __builtin_fmaf((tr[2] * L2) * R[2], epi.w, v.z);
        } else if constexpr (MODE == 2) {  // CacheOnly: (L * T) * R
            v.x = (L0 * tr[0]) * R[0];
            v.y = (L1 * tr[1]) * R[1];
            v.z = (L2 * tr[2]) * R[2];
        } else {  // copy_radiance_to_output_buffer: L * R
            v.x = L0 * R[0];
            v.y = L1 * R[1];
            v.z = L2 * R[2];
        }
        v.w = 1.0f;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), buffer_rsrc(epi.rgba + s0, rows * 16),
                                               h ? kBufferOff : r * 16, 0, 0);
        const u3 ov = {__builtin_bit_cast(uint32_t, L0), __builtin_bit_cast(uint32_t, L1),
                       __builtin_bit_cast(uint32_t, L2)};
        // exact-n: the descriptor ends at the tile's last valid row, rows past n are dropped by the hardware
        __builtin_amdgcn_raw_buffer_store_b96(ov, buffer_rsrc(out + s0 * NRC_OUTPUT_DIMS, tile_rows(n, s0) * 12),
                                              h == 0 && s0 + r >= epi.n_acc ? r * 12 : kBufferOff, 0, 0);
        g = ng;
    }
}

int num_cus_factored() {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
        v = 256;
    return v;
}

template <int MODE>
hipError_t launch_factored(const float* queries, float* out, int64_t n, const _Float16* wf, const FactoredEpilogue& epi,
                           hipStream_t s) {
    static int bpc = 0;  // resident blocks per CU
    if (!bpc) {
        int v = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, infer_factored_kernel<MODE>, kThreads, 0) != hipSuccess ||
            v <= 0)
            v = 1;
        bpc = v;
    }
    // at least one tile per wave, at most one block per CU slot
    const int64_t ntiles = (n + 31) / 32;
    const int64_t want = (ntiles + kThreads / 64 - 1) / (kThreads / 64), cap = (int64_t)num_cus_factored() * bpc;
    hipLaunchKernelGGL(infer_factored_kernel<MODE>, dim3((unsigned)(want < cap ? want : cap)), dim3(kThreads), 0, s,
                       queries, out, n, reinterpret_cast<const h8*>(wf), epi);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_infer_accumulate_factored(const float* queries, float* out, int64_t n, const _Float16* wf,
                                            const float* thr, float* rgba, int64_t n_acc, int mode, float w,
                                            hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const FactoredEpilogue epi{thr, reinterpret_cast<float4*>(rgba), n_acc, w};
    switch (mode) {
        case 0: return launch_factored<0>(queries, out, n, wf, epi, s);
        case 2: return launch_factored<2>(queries, out, n, wf, epi, s);
        case 4: return launch_factored<4>(queries, out, n, wf, epi, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace nrc_amd
