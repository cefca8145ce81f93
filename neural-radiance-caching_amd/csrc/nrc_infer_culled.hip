// nrc_infer_culled.hip — fused inference + accumulate_render_radiance that culls the render queries whose
// lastRenderThroughput is zero before the MLP runs (nrc_infer_accumulate_culled, DESIGN.md §9 "Culled fused
// accumulation"). Width 64, InputEncoding::Frequency, compact queries; NRC_PRECISION_F16 or NRC_PRECISION_FP8; plain or
// reflectance-factored accumulation. Three launches, ordered by the stream (no cross-block wait anywhere):
//
// 1. cull_classify_kernel<MODE>: one streaming pass over the throughputs. A wave owns the kCullSegment pixels
//    [seg * kCullSegment, ...) and takes 64 of them per step. A pixel is dead iff all three throughput words are +-0
//    ((bits & 0x7fffffff) == 0; NaN and denormals are live). A dead lane finishes its pixel itself with the dense
//    epilogue's operations for radiance +0: Full dst.c = fmaf(T.c * 0, w, dst.c), CacheOnly dst.c = 0 * T.c, dst.w = 1.
//    The live lanes are compacted by ballot + popcount and the wave appends their pixel indices, ascending, at
//    list[seg * kCullSegment + running]: a segment's own index range is its slot space, so waves never coordinate --
//    no LDS, no barrier, no atomics. At the end the wave writes count[seg]. Every access goes through a descriptor of
//    the segment (loads past it return 0, stores past it and those of masked lanes, at kBufferOff, are dropped).
// 2. cull_pack_kernel: block seg sums the counts in front of it (integer sums: the order does not matter), copies its
//    run to dense[prefix ..]; the last block writes total_live. Deterministic.
// 3. culled_tiles_kernel<FP8, MODE, RF>: the dense persistent kernels walking entries instead of rows. The entry space
//    is [0, total_live + (n - num_pixels)): entry e < total_live is row dense[e], any other row num_pixels + (e -
//    total_live). total_live is read at block start; the grid is the dense kernels' grid for n, and a block derives
//    its tile range from the entry count. Only the last tile is partial: its surplus lanes clamp to the last entry and
//    their stores are dropped. Waves draw tiles from an LDS counter two ahead: the entry -> row load of a tile is issued
//    one draw before its query records, so the dependent hop is never waited on at the head of the chain. Lane (r, h)
//    gathers its query with load_q(q, row, h), its throughput and (Full) pixel through descriptors before the MLP, and
//    the epilogue selects per lane between the 16-B rgba store (row < num_pixels) and the 12-B results store.
//    F16: variant 47's chain (nrc_chain47.h); FP8: mlp8 (nrc_chain8.h), the LDS image and scale words of
//    infer8_kernel. The reflectance comes from the tile's QLane (reflectance_half0). A query is one MFMA column, so a
//    live query's result is that of the dense entries bit for bit whatever its tile mates are.
//
// n <= 2^26 keeps every byte offset (60 n, 16 num_pixels) below 2^32 and every descriptor below 2^31 bytes.
// LDS: the f16 weight image (46 KiB) or the FP8 image (28 KiB) + the tile counter. 4 waves per SIMD (<= 128 VGPRs).
#include "nrc_chain47.h"
#include "nrc_chain8.h"

namespace nrc_amd {
namespace {

constexpr int kThreads = 1024;
constexpr int kClassifyThreads = 256, kPackThreads = 256;
constexpr int kSegSteps = kCullSegment / 64;
static_assert(kCullSegment % 64 == 0, "whole wave steps");
typedef float f3 __attribute__((ext_vector_type(3)));

// MODE 0 / 2: RenderMode Full / CacheOnly
template <int MODE>
__global__ __launch_bounds__(kClassifyThreads) void cull_classify_kernel(const float* __restrict__ thr,
                                                                        float4* __restrict__ rgba, uint32_t npix,
                                                                        float w, uint32_t* __restrict__ list,
                                                                        uint32_t* __restrict__ counts) {
    fp32_flush_output_denorms();  // the float mode of the dense epilogue
    const int lane = threadIdx.x & 63;
    const uint32_t seg = __builtin_amdgcn_readfirstlane(blockIdx.x * (kClassifyThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nseg = (npix + kCullSegment - 1) / kCullSegment;
    if (seg >= nseg) return;  // the whole wave
    const uint32_t s0 = seg * kCullSegment;
    const uint32_t rows = npix - s0 < (uint32_t)kCullSegment ? npix - s0 : (uint32_t)kCullSegment;
    const __amdgpu_buffer_rsrc_t rt = buffer_rsrc(thr + (size_t)s0 * 3, (int)rows * 12);
    const __amdgpu_buffer_rsrc_t rp = buffer_rsrc(rgba + s0, (int)rows * 16);
    const __amdgpu_buffer_rsrc_t rl = buffer_rsrc(list + s0, (int)rows * 4);
    uint32_t running = 0;
#pragma unroll 4
    for (int k = 0; k < kSegSteps; ++k) {
        const uint32_t j = (uint32_t)k * 64 + lane;  // pixel s0 + j
        const bool in = j < rows;
        const u3 tv = __builtin_amdgcn_raw_buffer_load_b96(rt, (int)j * 12, 0, 0);  // past the segment: 0
        const bool dead = in && ((tv.x | tv.y | tv.z) & 0x7fffffffu) == 0;
        const bool live = in && !dead;
        const int doff = dead ? (int)j * 16 : kBufferOff;
        const f3 T = __builtin_bit_cast(f3, tv);
        float4 v;
        if constexpr (MODE == 0) {  // Full: dst += (T * 0) * w
            v = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rp, doff, 0, 0));
            v.x = __builtin_fmaf(T.x * 0.0f, w, v.x);
            v.y = __builtin_fmaf(T.y * 0.0f, w, v.y);
            v.z = __builtin_fmaf(T.z * 0.0f, w, v.z);
        } else {  // CacheOnly
            v.x = 0.0f * T.x;
            v.y = 0.0f * T.y;
            v.z = 0.0f * T.z;
        }
        v.w = 1.0f;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), rp, doff, 0, 0);
        const uint64_t bal = __ballot(live);
        const uint32_t pos = running + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
        __builtin_amdgcn_raw_buffer_store_b32(s0 + j, rl, live ? (int)pos * 4 : kBufferOff, 0, 0);
        running += (uint32_t)__builtin_popcountll(bal);
    }
    __builtin_amdgcn_raw_buffer_store_b32(running, buffer_rsrc(counts, (int)nseg * 4), lane == 0 ? (int)seg * 4 : kBufferOff,
                                          0, 0);
}

// grid = max(nseg, 1) blocks
__global__ __launch_bounds__(kPackThreads) void cull_pack_kernel(const uint32_t* __restrict__ list,
                                                                const uint32_t* __restrict__ counts, uint32_t nseg,
                                                                uint32_t npix, uint32_t* __restrict__ dense,
                                                                uint32_t* __restrict__ total) {
    __shared__ uint32_t part[kPackThreads / 64];
    const uint32_t seg = blockIdx.x, tid = threadIdx.x;
    if (seg >= nseg) {  // no pixels at all
        if (tid == 0) *total = 0;
        return;
    }
    uint32_t s = 0;
    for (uint32_t i = tid; i < seg; i += kPackThreads) s += counts[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    uint32_t prefix = 0;
#pragma unroll
    for (int k = 0; k < kPackThreads / 64; ++k) prefix += part[k];
    const uint32_t s0 = seg * kCullSegment;
    const uint32_t cap = npix - s0 < (uint32_t)kCullSegment ? npix - s0 : (uint32_t)kCullSegment;
    const uint32_t cnt = counts[seg] < cap ? counts[seg] : cap;
    for (uint32_t i = tid; i < cnt; i += kPackThreads)
        if (prefix + i < npix) dense[prefix + i] = list[s0 + i];
    if (seg == nseg - 1 && tid == 0) *total = prefix + cnt < npix ? prefix + cnt : npix;
}

struct CullEpilogue {
    const float* thr;       // [npix] float3 lastRenderThroughput
    float4* rgba;           // [npix] frame buffer
    const uint32_t* dense;  // [total_live] live render rows, ascending
    const uint32_t* total;  // total_live
    uint32_t npix;
    float w;  // 1 / (iterationIndex + 1)
};

// FP8: the handle's precision; MODE 0 / 2: RenderMode Full / CacheOnly; RF: USE_REFLECTANCE_FACTORING 1
// wf: the f16 inference image (FP8: its first 10 fragments, layer 0); img8: FP8 fragments + scale words (FP8 only)
template <bool FP8, int MODE, bool RF>
__global__ __launch_bounds__(kThreads, 1) void culled_tiles_kernel(const float* __restrict__ q, float* __restrict__ out,
                                                                   uint32_t n, const h8* __restrict__ wf,
                                                                   const h8* __restrict__ img8, CullEpilogue epi) {
    constexpr int kLw = FP8 ? kL0H8 + kImg8H8 : kFwdFrags * 64;
    __shared__ __attribute__((aligned(16))) h8 lw[kLw];
    __shared__ uint32_t wq_next;
    fp32_flush_output_denorms();  // as the dense kernels (same encoder and epilogue arithmetic)
    if constexpr (FP8) {
        fp8_saturating_converts();  // pack8
        for (int i = threadIdx.x; i < kL0H8; i += kThreads) lw[i] = wf[i];
        for (int i = threadIdx.x; i < kImg8H8; i += kThreads) lw[kL0H8 + i] = img8[i];
    } else {
        for (int i = threadIdx.x; i < kLw; i += kThreads) lw[i] = wf[i];
    }
    if (threadIdx.x == 0) wq_next = 0;
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int h = lane >> 5, r = lane & 31;
    [[maybe_unused]] uint32_t sc[5];
    if constexpr (FP8) {
        const uint32_t* scales = reinterpret_cast<const uint32_t*>(img8 + kImg8H8);
#pragma unroll
        for (int l = 0; l < 5; ++l) sc[l] = scales[l * 32 + r];
    }
    const uint32_t npix = epi.npix;
    const uint32_t total = min(__builtin_amdgcn_readfirstlane(*epi.total), npix);
    const uint32_t entries = total + (n - npix);
    const uint32_t ntiles = (entries + 31) >> 5;
    const uint32_t gbase = (uint32_t)((uint64_t)blockIdx.x * ntiles / gridDim.x);
    const uint32_t gend = (uint32_t)((uint64_t)(blockIdx.x + 1) * ntiles / gridDim.x);  // end of this block's range
    const __amdgpu_buffer_rsrc_t rd = buffer_rsrc(epi.dense, (int)total * 4);
    const __amdgpu_buffer_rsrc_t rt = buffer_rsrc(epi.thr, (int)npix * 12);
    const __amdgpu_buffer_rsrc_t rp = buffer_rsrc(epi.rgba, (int)npix * 16);
    const __amdgpu_buffer_rsrc_t ro = buffer_rsrc(out, (int)n * 12);
    // entry of lane r in tile g, clamped to the last entry, and its list word (0 for an entry past the list)
    auto entry = [&](uint32_t g) { return min(g * 32 + (uint32_t)r, entries - 1); };
    auto list_word = [&](uint32_t g) { return __builtin_amdgcn_raw_buffer_load_b32(rd, (int)entry(g) * 4, 0, 0); };
    auto row_of = [&](uint32_t g, uint32_t word) {
        const uint32_t e = entry(g);
        return min(e < total ? word : npix + (e - total), n - 1);
    };
    auto draw = [&]() {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(&wq_next, 1u);
        return t;
    };
    uint32_t g0 = gbase + __builtin_amdgcn_readfirstlane(draw());
    if (g0 >= gend) return;
    uint32_t g1 = gbase + __builtin_amdgcn_readfirstlane(draw());
    uint32_t nn_raw = draw();  // the tile after next: read at the head of the loop
    uint32_t row0 = row_of(g0, list_word(g0));
    uint32_t word1 = list_word(g1);
    QLane Q = load_q(q, (int64_t)row0, h);
    while (g0 < gend) {
        // the draw issued one iteration ago (an asm readfirstlane stays here; the builtin would be hoisted to the
        // atomic and the wave would wait for it there)
        uint32_t t;
        asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(t) : "v"(nn_raw));
        const uint32_t g2 = gbase + t;
        h8 x[5];
        encode_v3(Q, h, x);
        [[maybe_unused]] float R[3];
        if constexpr (RF) reflectance_half0(Q, R);  // from the finished tile's registers, before the prefetch takes them
        if (lane == 0) nn_raw = atomicAdd(&wq_next, 1u);
        const uint32_t row1 = row_of(g1, word1);  // its list word was loaded one iteration ago
        Q = load_q(q, (int64_t)row1, h);          // gathered prefetch of the next tile
        const uint32_t word2 = list_word(g2);     // consumed one iteration from now
        // epilogue operands are fetched before the chain so their latency hides under the MFMAs
        const bool valid = g0 * 32 + (uint32_t)r < entries;  // surplus lanes of the last tile store nothing
        const bool px = h == 0 && row0 < npix;
        const f3 tr = __builtin_bit_cast(f3, __builtin_amdgcn_raw_buffer_load_b96(rt, px ? (int)row0 * 12 : kBufferOff, 0, 0));
        float4 acc = {};
        if constexpr (MODE == 0)
            acc = __builtin_bit_cast(float4,
                                     __builtin_amdgcn_raw_buffer_load_b128(rp, px ? (int)row0 * 16 : kBufferOff, 0, 0));
        float L0, L1, L2;
        if constexpr (FP8) {
            h8 xt[1][5];
#pragma unroll
            for (int kk = 0; kk < 5; ++kk) xt[0][kk] = x[kk];
            f16v o[1];
            mlp8<1>((lds_h8*)(lw + lane), xt, sc, o);
            // rows 0..2 of query r are registers 0..2 of lane half 0; ReLU, then through f16 as infer8_kernel's output
            L0 = (float)(_Float16)fmaxf(o[0][0], 0.0f);
            L1 = (float)(_Float16)fmaxf(o[0][1], 0.0f);
            L2 = (float)(_Float16)fmaxf(o[0][2], 0.0f);
        } else {
            chain47((lds_h8*)(lw + lane), x, L0, L1, L2);
        }
        float4 v;
        if constexpr (RF && MODE == 0) {  // Full: dst += ((T * L) * R) * w
            v = acc;
            v.x = __builtin_fmaf((tr.x * L0) * R[0], epi.w, v.x);
            v.y = __builtin_fmaf((tr.y * L1) * R[1], epi.w, v.y);
            v.z = __builtin_fmaf((tr.z * L2) * R[2], epi.w, v.z);
        } else if constexpr (RF) {  // CacheOnly: (L * T) * R
            v.x = (L0 * tr.x) * R[0];
            v.y = (L1 * tr.y) * R[1];
            v.z = (L2 * tr.z) * R[2];
        } else if constexpr (MODE == 0) {  // Full: dst += (T * L) * w
            v = acc;
            v.x = __builtin_fmaf(tr.x * L0, epi.w, v.x);
            v.y = __builtin_fmaf(tr.y * L1, epi.w, v.y);
            v.z = __builtin_fmaf(tr.z * L2, epi.w, v.z);
        } else {  // CacheOnly
            v.x = L0 * tr.x;
            v.y = L1 * tr.y;
            v.z = L2 * tr.z;
        }
        v.w = 1.0f;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), rp, valid && px ? (int)row0 * 16 : kBufferOff, 0,
                                               0);
        const u3 ov = {__builtin_bit_cast(uint32_t, L0), __builtin_bit_cast(uint32_t, L1),
                       __builtin_bit_cast(uint32_t, L2)};
        __builtin_amdgcn_raw_buffer_store_b96(ov, ro, valid && h == 0 && row0 >= npix ? (int)row0 * 12 : kBufferOff, 0, 0);
        g0 = g1;
        g1 = g2;
        row0 = row1;
        word1 = word2;
    }
}

int num_cus_culled() {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
        v = 256;
    return v;
}

template <int MODE>
hipError_t launch_classify(const CullEpilogue& epi, uint32_t nseg, uint32_t* list, uint32_t* counts, hipStream_t s) {
    constexpr uint32_t kWaves = kClassifyThreads / 64;
    hipLaunchKernelGGL(cull_classify_kernel<MODE>, dim3((nseg + kWaves - 1) / kWaves), dim3(kClassifyThreads), 0, s,
                       epi.thr, epi.rgba, epi.npix, epi.w, list, counts);
    return hipGetLastError();
}

template <bool FP8, int MODE, bool RF>
hipError_t launch_tiles(const float* queries, float* out, uint32_t n, const _Float16* wf, const uint8_t* img8,
                        const CullEpilogue& epi, hipStream_t s) {
    static int bpc = 0;  // resident blocks per CU
    if (!bpc) {
        int v = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, culled_tiles_kernel<FP8, MODE, RF>, kThreads, 0) !=
                hipSuccess || v <= 0)
            v = 1;
        bpc = v;
    }
    // the dense kernels' grid for n: at least one tile per wave, at most one block per CU slot
    const int64_t ntiles = ((int64_t)n + 31) / 32;
    const int64_t want = (ntiles + kThreads / 64 - 1) / (kThreads / 64), cap = (int64_t)num_cus_culled() * bpc;
    hipLaunchKernelGGL((culled_tiles_kernel<FP8, MODE, RF>), dim3((unsigned)(want < cap ? want : cap)), dim3(kThreads), 0,
                       s, queries, out, n, reinterpret_cast<const h8*>(wf), reinterpret_cast<const h8*>(img8), epi);
    return hipGetLastError();
}

template <bool FP8, int MODE>
hipError_t launch_tiles_rf(bool rf, const float* queries, float* out, uint32_t n, const _Float16* wf,
                           const uint8_t* img8, const CullEpilogue& epi, hipStream_t s) {
    return rf ? launch_tiles<FP8, MODE, true>(queries, out, n, wf, img8, epi, s)
              : launch_tiles<FP8, MODE, false>(queries, out, n, wf, img8, epi, s);
}

}  // namespace

size_t cull_workspace_bytes(uint32_t pixels) {
    return ((size_t)2 * pixels + cull_segments(pixels) + 1) * sizeof(uint32_t);
}

hipError_t launch_infer_accumulate_culled(const float* queries, float* out, uint32_t n, const _Float16* wf,
                                          const uint8_t* img8, const float* thr, float* rgba, uint32_t npix, int mode,
                                          float w, bool factored, uint32_t* ws, uint32_t ws_pixels, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (npix > n || npix > ws_pixels || n > kCullMaxQueries || (mode != 0 && mode != 2)) return hipErrorInvalidValue;
    // workspace: list[ws_pixels] | dense[ws_pixels] | count[segments(ws_pixels)] | total
    uint32_t* const list = ws;
    uint32_t* const dense = ws + ws_pixels;
    uint32_t* const counts = dense + ws_pixels;
    uint32_t* const total = counts + cull_segments(ws_pixels);
    const uint32_t nseg = cull_segments(npix);
    const CullEpilogue epi{thr, reinterpret_cast<float4*>(rgba), dense, total, npix, w};
    hipError_t e = hipSuccess;
    if (nseg) e = mode == 0 ? launch_classify<0>(epi, nseg, list, counts, s) : launch_classify<2>(epi, nseg, list, counts, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cull_pack_kernel, dim3(nseg ? nseg : 1), dim3(kPackThreads), 0, s, list, counts, nseg, npix, dense,
                       total);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (img8)
        return mode == 0 ? launch_tiles_rf<true, 0>(factored, queries, out, n, wf, img8, epi, s)
                         : launch_tiles_rf<true, 2>(factored, queries, out, n, wf, img8, epi, s);
    return mode == 0 ? launch_tiles_rf<false, 0>(factored, queries, out, n, wf, img8, epi, s)
                     : launch_tiles_rf<false, 2>(factored, queries, out, n, wf, img8, epi, s);
}

}  // namespace nrc_amd
