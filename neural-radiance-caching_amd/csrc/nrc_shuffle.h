// nrc_shuffle.h — the training shuffle's permutation, shared by the frame kernels that materialise it (nrc_frame.hip:
// permutation_kernel, permute_kernel) and the training kernels that gather through it (nrc_train16.hip,
// nrc_train_dc.hip: nrc_train_gather). Keyed 4-round Feistel network on [0, 2^(2h)) with cycle walking into [0, n);
// spec in DESIGN.md §9 (restated independently in oracle/nrc_frame_oracle.c).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nrc_amd {

__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

struct FeistelKey {
    uint32_t k[4];
    uint32_t h, n;
};

__device__ __forceinline__ uint32_t feistel_perm(uint32_t d, const FeistelKey& fk) {
    const uint32_t mask = (1u << fk.h) - 1u;
    uint32_t x = d;
    do {
        uint32_t L = x >> fk.h, R = x & mask;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t nl = R;
            R = L ^ (mix32(R ^ fk.k[r]) & mask);
            L = nl;
        }
        x = (L << fk.h) | R;
    } while (x >= fk.n);  // terminates: the walk stays on d's cycle, which contains d < n
    return x;
}

inline FeistelKey make_key(uint64_t seed, uint32_t frame, uint32_t n) {
    FeistelKey fk{};
    for (uint32_t r = 0; r < 4; ++r)
        fk.k[r] = mix32((uint32_t)seed ^ mix32((uint32_t)(seed >> 32) ^ mix32(frame + 0x9e3779b9u * (r + 1))));
    uint32_t b = 2;
    while (b < 32 && (1ull << b) < (uint64_t)n) ++b;
    if (b & 1) ++b;
    fk.h = b / 2;
    fk.n = n;
    return fk;
}

// Source of a gathered training step (nrc_train_gather): sample d of the step is record
//     perm(first + d) % nrec,  perm(i) = perm[i] if perm != null, else feistel_perm(i, fk)
// of the traced buffers -- permute_kernel's row, computed by the kernel that consumes the record. feistel_perm reads
// no memory, so its cycle walk may diverge freely; at n_out = 2^(2h) (the frame's 65,536) the walk is never taken:
// four rounds, about 40 integer VALU. The modulo (nrc_helpers.cu:245) is a real division, done once per sample.
struct GatherSrc {
    const int* perm;  // the caller's (or the key sort's) permutation of [0, fk.n), or null: Feistel
    FeistelKey fk;    // key of (seed, frame_index) on [0, n_out)
    uint32_t first;   // row of the shuffled order that the step's sample 0 takes
    uint32_t nrec;    // min(num_records, n_out) >= 1
};

}  // namespace nrc_amd
