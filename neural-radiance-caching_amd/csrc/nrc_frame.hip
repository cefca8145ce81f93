// nrc_frame.hip — the per-frame kernels around the network (include/nrc/frame.h).
//
// All four are HBM/latency-bound integer-and-copy work on a few MB: one thread per pixel,
// tile or output dword, coalesced where the layout allows, no LDS, no MFMA. Float arithmetic is written with
// explicit fmaf where the reference's nvcc --use_fast_math build contracts `a += b * c`
// (CMakeLists.txt:256-257), so results are bit-identical to the oracle (oracle/nrc_frame_oracle.c).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "nrc_internal.h"
#include "nrc_shuffle.h"

namespace nrc_amd {

namespace {

struct F3 {
    float x, y, z;
};
struct TrainRecord {  // neural_radiance_caching.h:57-75
    int prop_to;
    F3 lt;
    int pixel, tile, len;
};
struct EndVertex {  // neural_radiance_caching.h:78-94
    int start;
    float mask;
    int pixel, tile;
};
static_assert(sizeof(TrainRecord) == 28 && sizeof(EndVertex) == 16, "reference record sizes");

// RadianceQuery::reflectance() = diffuse + specular (neural_radiance_caching.h:118; compact record: floats 9..11, 12..14;
// X = 1: padded 16-float record, one float further)
template <int X = 0>
__device__ __forceinline__ F3 reflectance(const float* __restrict__ q, uint32_t i) {
    const float* r = q + (size_t)i * (NRC_INPUT_DIMS + X) + X;
    return F3{r[9] + r[12], r[10] + r[13], r[11] + r[14]};
}

// accumulate_render_radiance (nrc_helpers.cu:77-129), one pixel per lane; MODE is the RenderMode.
// w = 1/(iterationIndex+1) comes from the host (correctly rounded).
// RF: USE_REFLECTANCE_FACTORING 1 (nrc_helpers.cu:95-97, 111-113, 118-120; copy_radiance_to_output_buffer :66-68): the
// radiance times the render query's reflectance, after the throughput product
template <int MODE, bool RF = false, int X = 0>  // X = 1: padded RadianceQuery records
__global__ __launch_bounds__(256) void accumulate_kernel(const F3* __restrict__ rad, const F3* __restrict__ thr,
                                                         float4* __restrict__ rgba, uint32_t n, float w,
                                                         const float* __restrict__ queries = nullptr) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4 o;
    F3 R = {1.0f, 1.0f, 1.0f};
    if constexpr (RF && MODE != 5) R = reflectance<X>(queries, i);
    if constexpr (MODE == 0) {  // Full: dst += (T * L) * w   (RF: ((T * L) * R) * w)
        const F3 L = rad[i], T = thr[i];
        o = rgba[i];
        if constexpr (RF) {
            o.x = __builtin_fmaf((T.x * L.x) * R.x, w, o.x);
            o.y = __builtin_fmaf((T.y * L.y) * R.y, w, o.y);
            o.z = __builtin_fmaf((T.z * L.z) * R.z, w, o.z);
        } else {
            o.x = __builtin_fmaf(T.x * L.x, w, o.x);
            o.y = __builtin_fmaf(T.y * L.y, w, o.y);
            o.z = __builtin_fmaf(T.z * L.z, w, o.z);
        }
    } else if constexpr (MODE == 2) {  // CacheOnly   (RF: (L * T) * R)
        const F3 L = rad[i], T = thr[i];
        o.x = L.x * T.x;
        o.y = L.y * T.y;
        o.z = L.z * T.z;
        if constexpr (RF) {
            o.x *= R.x;
            o.y *= R.y;
            o.z *= R.z;
        }
    } else if constexpr (MODE == 4) {  // DebugCacheNoThroughputModulation / copy_radiance_to_output_buffer (RF: L * R)
        const F3 L = rad[i];
        o.x = L.x;
        o.y = L.y;
        o.z = L.z;
        if constexpr (RF) {
            o.x *= R.x;
            o.y *= R.y;
            o.z *= R.z;
        }
    } else {  // 5: DebugThroughputOnly
        const F3 T = thr[i];
        o.x = T.x;
        o.y = T.y;
        o.z = T.z;
    }
    o.w = 1.0f;
    rgba[i] = o;
}

// propagate_train_radiance (nrc_helpers.cu:131-224), one tile per lane walking its own record chain.
// Chains are disjoint (one train path per tile), so the read-modify-write of targets needs no atomics.
// Every lane exits: an index outside [0, nrec) ends the chain, and a chain is cut after nrec steps.
// RF: USE_REFLECTANCE_FACTORING 1 (nrc_helpers.cu:156-160, 191-204): the targets hold radiance / reflectance; the end
// radiance is multiplied by the end query's reflectance, each record's target by its own query's before the update and
// divided by it after (safeDiv: a zero component gives 0, nrc_helpers.cu:28-35); the chain carries the radiance itself.
template <bool RF = false, int X = 0>  // X = 1: padded RadianceQuery records
__global__ __launch_bounds__(256) void propagate_kernel(const EndVertex* __restrict__ ends,
                                                        const F3* __restrict__ end_rad, uint32_t tiles,
                                                        const TrainRecord* __restrict__ rec, F3* targets,
                                                        uint32_t nrec, const float* __restrict__ end_q = nullptr,
                                                        const float* __restrict__ train_q = nullptr) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= tiles) return;
    const EndVertex ev = ends[t];
    const F3 er = end_rad[t];
    F3 last = {er.x * ev.mask, er.y * ev.mask, er.z * ev.mask};  // :154
    if constexpr (RF) {                                            // :159
        const F3 R = reflectance<X>(end_q, t);
        last.x *= R.x;
        last.y *= R.y;
        last.z *= R.z;
    }
    int i = ev.start;
    for (uint32_t steps = 0; i >= 0 && (uint32_t)i < nrec && steps < nrec; ++steps) {
        const int next = rec[i].prop_to;
        const F3 lt = rec[i].lt;
        F3 v = targets[i];
        F3 R = {1.0f, 1.0f, 1.0f};
        if constexpr (RF) {  // :191-193 radianceTo = targetTo * refl
            R = reflectance<X>(train_q, (uint32_t)i);
            v.x *= R.x;
            v.y *= R.y;
            v.z *= R.z;
        }
        v.x = __builtin_fmaf(lt.x, last.x, v.x);  // :199 radianceTo += localThroughput * lastRadiance
        v.y = __builtin_fmaf(lt.y, last.y, v.y);
        v.z = __builtin_fmaf(lt.z, last.z, v.z);
        if constexpr (RF) {  // :203 targetTo = safeDiv(radianceTo, refl)
            targets[i] = F3{R.x != 0.0f ? v.x / R.x : 0.0f, R.y != 0.0f ? v.y / R.y : 0.0f,
                            R.z != 0.0f ? v.z / R.z : 0.0f};
        } else {
            targets[i] = v;  // :205
        }
        last = v;  // :213
        i = next;  // :214
    }
}

// ---- shuffle permutation: the keyed Feistel network of nrc_shuffle.h (mix32, FeistelKey, feistel_perm, make_key)
__global__ __launch_bounds__(256) void permutation_kernel(FeistelKey fk, int* __restrict__ perm) {
    const uint32_t d = blockIdx.x * 256u + threadIdx.x;
    if (d >= fk.n) return;
    perm[d] = (int)feistel_perm(d, fk);
}

// permute_train_data (nrc_helpers.cu:226-249) as a dword copy: threads [0, QW n) write the query array,
// threads [QW n, (QW + 3) n) the target array, so every wave's stores are contiguous; each lane re-derives its
// record's source index (a few dozen integer ops, cheaper than a second pass through HBM). QW: dwords per
// RadianceQuery (15 compact, 16 padded).
template <uint32_t QW = 15u>
__global__ __launch_bounds__(256) void permute_kernel(const uint32_t* __restrict__ qs, const uint32_t* __restrict__ ts,
                                                      const int* __restrict__ perm, FeistelKey fk, uint32_t nrec,
                                                      uint32_t* __restrict__ qd, uint32_t* __restrict__ td) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const uint32_t nq = fk.n * QW;
    if (g >= nq + fk.n * 3u) return;
    const bool is_q = g < nq;
    const uint32_t gg = is_q ? g : g - nq;
    const uint32_t d = is_q ? gg / QW : gg / 3u;  // constant divisors: mul-hi, no integer division
    const uint32_t k = gg - d * (is_q ? QW : 3u);
    const uint32_t p = perm ? (uint32_t)perm[d] : feistel_perm(d, fk);
    const uint32_t s = p % nrec;  // :245 (a negative caller entry reads as unsigned: never out of bounds)
    if (is_q)
        qd[gg] = qs[(size_t)s * QW + k];
    else
        td[gg] = ts[(size_t)s * 3u + k];
}


// ---- the reference's own shuffle contract (NRCUtil.cu:19-35): cub::DeviceRadixSort::SortPairs of caller-supplied u32
// keys with the values [0, n), bits [0, 32) -- an LSD radix sort, so equal keys keep index order. Four passes of 8-bit
// digits over at most kSortBlocks blocks (the reference's 65,536 keys: 64 blocks of 1,024). Round 6 (VERDICT r05 item 6:
// the round-5 form -- a histogram and a scatter launch per pass -- took 54.5 us for 65,536 keys):
//   * sort_hist_kernel runs once, for pass 0 (and zeroes the count tables of passes 1..3);
//   * pass p's scatter also counts pass p + 1's digits per destination block (the block that will own output position
//     pos in the next pass is pos / chunk): one no-return atomic add per key into that table, so the next pass needs no
//     histogram launch -- 5 launches instead of 8;
//   * a scatter wave loads its keys and values once, up front (256 per wave: 4 per lane), counts and ranks them from
//     registers; the round-5 loop re-loaded them and waited one memory round trip per 64 keys;
//   * each block reads its digit's 64 block counts as 16-byte loads (count rows padded to kSortBlocks).
constexpr uint32_t kSortBlocks = 64;
constexpr uint32_t kSortHist = 256 * kSortBlocks;  // one pass's count table: [digit][block], rows of kSortBlocks
constexpr int kSortPerLane = 4;                    // keys per lane and group (256 per wave)

__global__ __launch_bounds__(256) void sort_hist_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t chunk,
                                                        uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    // the tables of passes 1..3 start at zero (their counts arrive by atomics from the previous pass's scatter)
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < 3u * kSortHist; i += gridDim.x * 256u) hist[kSortHist + i] = 0u;
    __syncthreads();
    const uint32_t b0 = blockIdx.x * chunk, b1 = min(n, b0 + chunk);
    for (uint32_t i = b0 + threadIdx.x; i < b1; i += 256u) atomicAdd(&h[keys[i] & 255u], 1u);
    __syncthreads();
    hist[threadIdx.x * kSortBlocks + blockIdx.x] = h[threadIdx.x];
}

// vin == nullptr: the values are the indices (the first pass of SortPairs(keys, iota)). hist_next: the next pass's
// table (counted here), or null for the last pass.
__global__ __launch_bounds__(256) void sort_scatter_kernel(const uint32_t* __restrict__ kin, const int* __restrict__ vin,
                                                           uint32_t* __restrict__ kout, int* __restrict__ vout,
                                                           uint32_t n, uint32_t chunk, int shift,
                                                           const uint32_t* __restrict__ hist,
                                                           uint32_t* __restrict__ hist_next) {
    __shared__ uint32_t tot[256];     // digit totals, then their inclusive scan
    __shared__ uint32_t cnt[4][256];  // per-wave digit counts, then each wave's next output position per digit
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const uint32_t nblk = gridDim.x, b = blockIdx.x;
    const uint32_t per = chunk / 4u, w0 = b * chunk + (uint32_t)w * per, w1 = min(n, w0 + per);
    // this wave's first group of keys and values, in flight with the count-table reads below. Branch-free: every lane
    // loads at a clamped index (< n) and the value array is selected, not branched on -- a load behind a scalar branch
    // and an exec-masked store in one loop is the combination tools/asm_hazard_check.py rule 3 bans
    uint32_t key[kSortPerLane];
    int val[kSortPerLane];
    const int* const vsrc = vin ? vin : reinterpret_cast<const int*>(kin);
    auto load_group = [&](uint32_t g0) {
#pragma unroll
        for (int j = 0; j < kSortPerLane; ++j) {
            const uint32_t i = g0 + 64u * j + lane;
            const uint32_t ic = i < w1 ? i : (w1 > 0 ? w1 - 1 : 0);
            key[j] = kin[ic];
            const int v = vsrc[ic];
            val[j] = vin ? v : (int)i;
        }
    };
    load_group(w0);
    // digit tid: its count over all blocks and over the blocks before this one (16-byte loads of its table row)
    uint32_t total = 0u, before = 0u;
    {
        typedef uint32_t u4v __attribute__((ext_vector_type(4)));
        const u4v* row = reinterpret_cast<const u4v*>(hist + (uint32_t)tid * kSortBlocks);
        u4v c[kSortBlocks / 4];
#pragma unroll
        for (uint32_t q = 0; q < kSortBlocks / 4; ++q) c[q] = row[q];
#pragma unroll
        for (uint32_t q = 0; q < kSortBlocks; ++q) {
            const uint32_t v = q < nblk ? c[q / 4][q % 4] : 0u;
            total += v;
            before += q < b ? v : 0u;
        }
    }
    tot[tid] = total;
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt[j][tid] = 0u;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t v = tid >= off ? tot[tid - off] : 0u;
        __syncthreads();
        tot[tid] += v;
        __syncthreads();
    }
    const uint32_t dbase = tot[tid] - total + before;  // first output slot of digit tid in this block
    // per-wave digit counts (the group in registers; a range past one group re-loads, n > 65,536 keys only)
    for (uint32_t g0 = w0; g0 < w1; g0 += 64u * kSortPerLane) {
        if (g0 != w0) load_group(g0);
#pragma unroll
        for (int j = 0; j < kSortPerLane; ++j)
            if (g0 + 64u * j + lane < w1) atomicAdd(&cnt[w][(key[j] >> shift) & 255u], 1u);
    }
    __syncthreads();
    uint32_t run = dbase;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t c = cnt[j][tid];
        cnt[j][tid] = run;
        run += c;
    }
    __syncthreads();
    // wave w: its range in order, 64 at a time (wave-uniform); lanes holding the same digit are matched by 8 ballots,
    // rank = the matching lanes below this one, the lowest of them advances the digit's position
    auto scatter_group = [&](uint32_t g0) {
#pragma unroll
        for (int j = 0; j < kSortPerLane; ++j) {
            const uint32_t i0 = g0 + 64u * j;
            if (i0 >= w1) continue;  // wave-uniform
            const bool valid = i0 + lane < w1;
            const uint32_t d = (key[j] >> shift) & 255u;
            uint64_t m = __ballot(valid);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool set = (d >> bit) & 1u;
                const uint64_t bb = __ballot(set);
                m &= set ? bb : ~bb;
            }
            const uint32_t rank = (uint32_t)__popcll(m & __lanemask_lt());
            const uint32_t base = cnt[w][d];
            if (valid && rank == 0u) cnt[w][d] = base + (uint32_t)__popcll(m);
            if (valid) {
                const uint32_t pos = base + rank;
                kout[pos] = key[j];
                vout[pos] = val[j];
                if (hist_next)
                    __hip_atomic_fetch_add(hist_next + ((key[j] >> (shift + 8)) & 255u) * kSortBlocks + pos / chunk, 1u,
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    };
    if (w1 <= w0 + 64u * kSortPerLane) {
        scatter_group(w0);  // one group (every wave at n <= 65,536 keys): still in registers, no loop
    } else {
        for (uint32_t g0 = w0; g0 < w1; g0 += 64u * kSortPerLane) {
            load_group(g0);  // the counting loop moved past the first group
            scatter_group(g0);
        }
    }
}

inline dim3 grid_for(uint64_t threads) { return dim3((unsigned)((threads + 255) / 256)); }

}  // namespace

hipError_t launch_accumulate(const float* rad, const float* thr, float* rgba, uint32_t n, int mode, float w,
                             hipStream_t s, const float* queries, bool padq) {
    if (n == 0) return hipSuccess;
    const F3* r = reinterpret_cast<const F3*>(rad);
    const F3* t = reinterpret_cast<const F3*>(thr);
    float4* o = reinterpret_cast<float4*>(rgba);
    const dim3 g = grid_for(n), b(256);
    if (queries && padq) {  // USE_REFLECTANCE_FACTORING 1 over padded RadianceQuery records
        switch (mode) {
        case 0: hipLaunchKernelGGL((accumulate_kernel<0, true, 1>), g, b, 0, s, r, t, o, n, w, queries); break;
        case 2: hipLaunchKernelGGL((accumulate_kernel<2, true, 1>), g, b, 0, s, r, t, o, n, w, queries); break;
        case 4: hipLaunchKernelGGL((accumulate_kernel<4, true, 1>), g, b, 0, s, r, t, o, n, w, queries); break;
        case 5: hipLaunchKernelGGL((accumulate_kernel<5, true, 1>), g, b, 0, s, r, t, o, n, w, queries); break;
        default: return hipSuccess;
        }
        return hipGetLastError();
    }
    if (queries) {  // USE_REFLECTANCE_FACTORING 1
        switch (mode) {
        case 0: hipLaunchKernelGGL((accumulate_kernel<0, true>), g, b, 0, s, r, t, o, n, w, queries); break;
        case 2: hipLaunchKernelGGL((accumulate_kernel<2, true>), g, b, 0, s, r, t, o, n, w, queries); break;
        case 4: hipLaunchKernelGGL((accumulate_kernel<4, true>), g, b, 0, s, r, t, o, n, w, queries); break;
        case 5: hipLaunchKernelGGL((accumulate_kernel<5, true>), g, b, 0, s, r, t, o, n, w, queries); break;
        default: return hipSuccess;
        }
        return hipGetLastError();
    }
    switch (mode) {
    case 0: hipLaunchKernelGGL(accumulate_kernel<0>, g, b, 0, s, r, t, o, n, w, nullptr); break;
    case 2: hipLaunchKernelGGL(accumulate_kernel<2>, g, b, 0, s, r, t, o, n, w, nullptr); break;
    case 4: hipLaunchKernelGGL(accumulate_kernel<4>, g, b, 0, s, r, t, o, n, w, nullptr); break;
    case 5: hipLaunchKernelGGL(accumulate_kernel<5>, g, b, 0, s, r, t, o, n, w, nullptr); break;
    default: return hipSuccess;  // NoCache / CacheFirstVertex: nothing to accumulate (nrc_helpers.cu:104-107)
    }
    return hipGetLastError();
}

hipError_t launch_propagate(const void* ends, const float* end_rad, uint32_t tiles, const void* records,
                            float* targets, uint32_t nrec, hipStream_t s, const float* end_queries,
                            const float* train_queries, bool padq) {
    if (tiles == 0 || nrec == 0) return hipSuccess;
    if ((end_queries == nullptr) != (train_queries == nullptr)) return hipErrorInvalidValue;
    if (end_queries && padq)
        hipLaunchKernelGGL((propagate_kernel<true, 1>), grid_for(tiles), dim3(256), 0, s,
                           reinterpret_cast<const EndVertex*>(ends), reinterpret_cast<const F3*>(end_rad), tiles,
                           reinterpret_cast<const TrainRecord*>(records), reinterpret_cast<F3*>(targets), nrec,
                           end_queries, train_queries);
    else if (end_queries)
        hipLaunchKernelGGL(propagate_kernel<true>, grid_for(tiles), dim3(256), 0, s,
                           reinterpret_cast<const EndVertex*>(ends), reinterpret_cast<const F3*>(end_rad), tiles,
                           reinterpret_cast<const TrainRecord*>(records), reinterpret_cast<F3*>(targets), nrec,
                           end_queries, train_queries);
    else
        hipLaunchKernelGGL(propagate_kernel<false>, grid_for(tiles), dim3(256), 0, s,
                           reinterpret_cast<const EndVertex*>(ends), reinterpret_cast<const F3*>(end_rad), tiles,
                           reinterpret_cast<const TrainRecord*>(records), reinterpret_cast<F3*>(targets), nrec,
                           nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_permutation(uint64_t seed, uint32_t frame, int* perm, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(permutation_kernel, grid_for(n), dim3(256), 0, s, make_key(seed, frame, n), perm);
    return hipGetLastError();
}

hipError_t launch_permute(const float* qs, const float* ts, const int* perm, uint64_t seed, uint32_t frame,
                          uint32_t nrec, float* qd, float* td, uint32_t n_out, hipStream_t s, bool padq) {
    if (n_out == 0 || nrec == 0) return hipSuccess;
    if (padq)
        hipLaunchKernelGGL(permute_kernel<16u>, grid_for((uint64_t)n_out * 19u), dim3(256), 0, s,
                           reinterpret_cast<const uint32_t*>(qs), reinterpret_cast<const uint32_t*>(ts), perm,
                           make_key(seed, frame, n_out), nrec, reinterpret_cast<uint32_t*>(qd),
                           reinterpret_cast<uint32_t*>(td));
    else
        hipLaunchKernelGGL(permute_kernel<15u>, grid_for((uint64_t)n_out * 18u), dim3(256), 0, s,
                           reinterpret_cast<const uint32_t*>(qs), reinterpret_cast<const uint32_t*>(ts), perm,
                           make_key(seed, frame, n_out), nrec, reinterpret_cast<uint32_t*>(qd),
                           reinterpret_cast<uint32_t*>(td));
    return hipGetLastError();
}

// Temporary storage of launch_sort_pairs: ping keys + values, second key buffer, the four passes' digit-count tables.
size_t sort_pairs_temp_bytes(uint32_t n) { return sizeof(uint32_t) * (3 * (size_t)n + 4 * (size_t)kSortHist); }

hipError_t launch_sort_pairs(const uint32_t* keys, uint32_t* keys_out, int* vals_out, uint32_t n, void* temp,
                             hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!keys || !vals_out || !temp) return hipErrorInvalidValue;
    const uint32_t nblk = std::min<uint32_t>(kSortBlocks, (n + 1023u) / 1024u);
    const uint32_t chunk = ((n + nblk - 1u) / nblk + 255u) / 256u * 256u;  // elements per block, 64 per wave-step
    uint32_t* kA = static_cast<uint32_t*>(temp);
    int* vA = reinterpret_cast<int*>(kA + n);
    uint32_t* kB = kA + 2 * (size_t)n;
    uint32_t* hist = kA + 3 * (size_t)n;
    // pass p reads (ki, vi), writes (ko, vo): keys -> A -> B/vals_out -> A -> keys_out/B, vals_out
    const uint32_t* ki[4] = {keys, kA, kB, kA};
    const int* vi[4] = {nullptr, vA, vals_out, vA};
    uint32_t* ko[4] = {kA, kB, kA, keys_out ? keys_out : kB};
    int* vo[4] = {vA, vals_out, vA, vals_out};
    hipLaunchKernelGGL(sort_hist_kernel, dim3(nblk), dim3(256), 0, s, keys, n, chunk, hist);
    for (int p = 0; p < 4; ++p)
        hipLaunchKernelGGL(sort_scatter_kernel, dim3(nblk), dim3(256), 0, s, ki[p], vi[p], ko[p], vo[p], n, chunk, 8 * p,
                           hist + p * kSortHist, p < 3 ? hist + (p + 1) * kSortHist : nullptr);
    return hipGetLastError();
}

}  // namespace nrc_amd
