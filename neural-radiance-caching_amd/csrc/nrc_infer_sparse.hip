// nrc_infer_sparse.hip — fused inference + accumulate_render_radiance that skips the MLP for render queries whose
// lastRenderThroughput is exactly zero (nrc_infer_accumulate_sparse, DESIGN.md §9 "Sparse fused accumulation").
// Width 64, InputEncoding::Frequency, NRC_PRECISION_F16, compact queries.
//
// A render query i < n_acc is dead iff T.x == 0 && T.y == 0 && T.z == 0 (IEEE compares: +-0 dead, NaN live). The
// dense epilogue multiplies a dead query's radiance by that zero, so its pixel is finished without the network:
// Full dst.c = fmaf(T.c * 0, w, dst.c), CacheOnly dst.c = 0 * T.c, dst.w = 1 -- the dense float operations with
// radiance +0. Every other query (the live render queries and all of [n_acc, n)) runs the f16 chain of the product
// inference kernel (variant 47 of nrc_kernels.hip): the same MFMA shapes in the same K order per layer, the 4x4x4
// output layer and the same epilogue arithmetic, so its result is bit-identical to nrc_infer_accumulate's.
//
// Work split. Persistent 1024-thread blocks, one per CU slot; a block owns the contiguous index range
// [b n / G, (b + 1) n / G) and walks it in chunks of kSparseChunk indices.
//   classify(c): thread t takes indices chunk + t and chunk + 1024 + t. It loads the throughput (indices >= n_acc are
//     live without a load), finishes a dead pixel on the spot (rgba load, the formula above, 16-B store), and the wave
//     compacts its live indices by ballot + popcount into the chunk's LDS list. A wave reserves its run of list slots
//     with one LDS atomic add on the chunk's live counter (not a 16-entry offset table: the table needs a barrier
//     between the counts and the writes, the atomic keeps one barrier per chunk). Runs land in arrival order; inside a
//     run the indices ascend, so a tile's gathers stay within a few 64-index neighbourhoods.
//   tiles(c): waves draw tiles of 32 list entries from an LDS counter. Lane (r, h) reads its row from the list, gathers
//     the query (load_q with a per-lane row), its throughput and pixel, encodes, runs the chain and scatters the
//     result: a 16-B rgba store for row < n_acc, a 12-B results store otherwise. The next tile's rows and queries
//     are fetched before the chain (draw one ahead), as the dense kernels do.
//   carry: the total % 32 live indices a chunk leaves over move to slots [32 - rem, 32) of the other list, directly in
//     front of the next chunk's entries (which start at slot 32), so every tile is a full 32 live queries except the
//     last tile of the block's range.
//   Two lists ping-pong: between two barriers a wave first classifies chunk c + 1 into list (c + 1) & 1, then draws
//   tiles of chunk c from list c & 1: one barrier per chunk. The live and draw counters rotate over four slots; slot
//   (c + 2) & 3 is cleared in stage c, two barriers from either use. (Issuing the throughput loads before the tiles
//   and consuming them after measured no faster, DESIGN.md §9: a stage's cost is its fill and drain, not the classify.)
//
// LDS: 46 KiB f16 weight image + 2 x 2080 list entries (16.25 KiB) + 8 counters. 4 waves per SIMD (<= 128 VGPRs).
#include "nrc_chain47.h"

namespace nrc_amd {
namespace {

constexpr int kThreads = 1024;
constexpr int kPer = kSparseChunk / kThreads;  // indices a thread classifies per chunk
constexpr int kListCap = 32 + kSparseChunk;    // 32 carry slots in front of a chunk's entries
static_assert(kSparseChunk % kThreads == 0, "whole classify rounds");

struct SparseEpilogue {
    const float* thr;  // [n_acc] float3 lastRenderThroughput
    float4* rgba;      // [n_acc] frame buffer
    int64_t n_acc;
    float w;  // 1 / (iterationIndex + 1)
};

// EPI 0 / 2: RenderMode Full / CacheOnly
template <int EPI>
__global__ __launch_bounds__(kThreads, 1) void infer_sparse_kernel(const float* __restrict__ q, float* __restrict__ out,
                                                                   int64_t n, const h8* __restrict__ wf,
                                                                   SparseEpilogue epi) {
    __shared__ __attribute__((aligned(16))) h8 lw[kFwdFrags * 64];
    __shared__ uint32_t list[2][kListCap];
    __shared__ uint32_t live_cnt[4], tile_cnt[4];
    fp32_flush_output_denorms();  // as the dense kernel (same encoder and epilogue arithmetic)
    for (int i = threadIdx.x; i < kFwdFrags * 64; i += kThreads) lw[i] = wf[i];
    if (threadIdx.x < 4) live_cnt[threadIdx.x] = tile_cnt[threadIdx.x] = 0;
    __syncthreads();

    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r = lane & 31;
    const int64_t b0 = (int64_t)blockIdx.x * n / gridDim.x, b1 = (int64_t)(blockIdx.x + 1) * n / gridDim.x;
    const int nch = (int)((b1 - b0 + kSparseChunk - 1) / kSparseChunk);
    if (nch == 0) return;  // the whole block

    auto classify = [&](int c) {
        const int64_t cb = b0 + (int64_t)c * kSparseChunk;
        const int64_t ce = cb + kSparseChunk < b1 ? cb + kSparseChunk : b1;
        uint32_t* const lst = list[c & 1];
        bool live[kPer];
        uint64_t bal[kPer];
        uint32_t total = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int64_t i = cb + k * kThreads + tid;
            bool lv = i < ce;
            if (lv && i < epi.n_acc) {
                const float* T = epi.thr + i * 3;
                const float tx = T[0], ty = T[1], tz = T[2];
                if (tx == 0.0f && ty == 0.0f && tz == 0.0f) {
                    lv = false;
                    float4 v;
                    if constexpr (EPI == 0) {  // Full: dst += (T * 0) * w
                        v = epi.rgba[i];
                        v.x = __builtin_fmaf(tx * 0.0f, epi.w, v.x);
                        v.y = __builtin_fmaf(ty * 0.0f, epi.w, v.y);
                        v.z = __builtin_fmaf(tz * 0.0f, epi.w, v.z);
                    } else {  // CacheOnly
                        v.x = 0.0f * tx;
                        v.y = 0.0f * ty;
                        v.z = 0.0f * tz;
                    }
                    v.w = 1.0f;
                    epi.rgba[i] = v;
                }
            }
            live[k] = lv;
            bal[k] = __ballot(lv);
            total += (uint32_t)__builtin_popcountll(bal[k]);
        }
        uint32_t base = 0;
        if (lane == 0 && total) base = atomicAdd(&live_cnt[c & 3], total);
        base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (live[k])
                lst[32 + base + (uint32_t)__builtin_popcountll(bal[k] & ((1ull << lane) - 1ull))] =
                    (uint32_t)(cb + k * kThreads + tid);
            base += (uint32_t)__builtin_popcountll(bal[k]);
        }
    };

    classify(0);
    lds_barrier();
    int start = 32;  // first entry of the current list: 32 - carried entries
    for (int c = 0; c < nch; ++c) {
        const uint32_t* const lst = list[c & 1];
        const int end = 32 + (int)live_cnt[c & 3];
        const bool lastc = c + 1 == nch;
        const int total = end - start;
        const int ntile = lastc ? (total + 31) >> 5 : total >> 5;
        const int rem = lastc ? 0 : total & 31;
        if (tid == 0) live_cnt[(c + 2) & 3] = tile_cnt[(c + 2) & 3] = 0;
        if (!lastc) classify(c + 1);
        if (tid < rem) list[(c + 1) & 1][32 - rem + tid] = lst[start + ntile * 32 + tid];

        auto draw = [&]() -> int {
            uint32_t t = 0;
            if (lane == 0) t = atomicAdd(&tile_cnt[c & 3], 1u);
            return (int)__builtin_amdgcn_readfirstlane(t);
        };
        int t = draw();
        if (t < ntile) {
            int e = start + t * 32 + r;
            bool valid = e < end;  // lanes past the list's end gather a clamped valid row and store nothing
            int64_t row = lst[valid ? e : end - 1];
            QLane Q = load_q(q, row, h);
            for (;;) {
                const int nt = draw();
                h8 x[5];
                encode_v3(Q, h, x);
                // epilogue operands are fetched before the chain so their latency hides under the MFMAs
                const bool px = valid && h == 0 && row < epi.n_acc;
                float tr0 = 0.0f, tr1 = 0.0f, tr2 = 0.0f;
                float4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                if (px) {
                    const float* T = epi.thr + row * 3;
                    tr0 = T[0];
                    tr1 = T[1];
                    tr2 = T[2];
                    if constexpr (EPI == 0) acc = epi.rgba[row];
                }
                const bool more = nt < ntile;
                bool nvalid = false;
                int64_t nrow = row;
                if (more) {
                    const int ne = start + nt * 32 + r;
                    nvalid = ne < end;
                    nrow = lst[nvalid ? ne : end - 1];
                    Q = load_q(q, nrow, h);
                }
                float L0, L1, L2;
                chain47((lds_h8*)(lw + lane), x, L0, L1, L2);
                if (px) {
                    float4 v;
                    if constexpr (EPI == 0) {  // Full: dst += (T * L) * w
                        v = acc;
                        v.x = __builtin_fmaf(tr0 * L0, epi.w, v.x);
                        v.y = __builtin_fmaf(tr1 * L1, epi.w, v.y);
                        v.z = __builtin_fmaf(tr2 * L2, epi.w, v.z);
                    } else {  // CacheOnly
                        v.x = L0 * tr0;
                        v.y = L1 * tr1;
                        v.z = L2 * tr2;
                    }
                    v.w = 1.0f;
                    epi.rgba[row] = v;
                } else if (valid && h == 0) {
                    float* dst = out + row * NRC_OUTPUT_DIMS;
                    dst[0] = L0;
                    dst[1] = L1;
                    dst[2] = L2;
                }
                if (!more) break;
                t = nt;
                row = nrow;
                valid = nvalid;
            }
        }
        start = 32 - rem;
        lds_barrier();
    }
}

int num_cus_sparse() {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
        v = 256;
    return v;
}

template <int EPI>
hipError_t launch_sparse(const float* queries, float* out, int64_t n, const _Float16* wf, const SparseEpilogue& epi,
                         hipStream_t s) {
    static int bpc = 0;  // resident blocks per CU
    if (!bpc) {
        int v = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, infer_sparse_kernel<EPI>, kThreads, 0) != hipSuccess || v <= 0)
            v = 1;
        bpc = v;
    }
    // at least 16 tiles' worth of indices per block, at most one block per CU slot
    const int64_t want = (n + 511) / 512, cap = (int64_t)num_cus_sparse() * bpc;
    hipLaunchKernelGGL(infer_sparse_kernel<EPI>, dim3((unsigned)(want < cap ? want : cap)), dim3(kThreads), 0, s, queries,
                       out, n, reinterpret_cast<const h8*>(wf), epi);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_infer_accumulate_sparse(const float* queries, float* out, int64_t n, const _Float16* wf,
                                          const float* thr, float* rgba, int64_t n_acc, int mode, float w,
                                          hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const SparseEpilogue epi{thr, reinterpret_cast<float4*>(rgba), n_acc, w};
    switch (mode) {
        case 0: return launch_sparse<0>(queries, out, n, wf, epi, s);
        case 2: return launch_sparse<2>(queries, out, n, wf, epi, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace nrc_amd
