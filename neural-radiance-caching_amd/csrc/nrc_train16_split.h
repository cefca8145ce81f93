// nrc_train16_split.h -- the role-split t16 training block (train16_split_body) with its LDS carve-up and dW-tile
// helpers, shared by the units that build kernels from it: nrc_train16.hip (train16_split_kernel, the fused step, Hash)
// and nrc_train_gather.hip (the gather form, nrc_train_gather). Device code with internal linkage per unit.
#pragma once

#include "nrc_t16.h"
#include "nrc_hash.h"

#include <type_traits>

namespace nrc_amd {
namespace {

using namespace t16;

// LDS carve-up (bytes). The four [128][64] f16 images (deltas and activations, double-buffered) sit at offset 0, so
// that an image access is one per-lane offset VGPR plus an immediate (the 16-bit DS offset field reaches every image);
// then the [128][32] image of layer-0 K slots 64..95, the loss partials, the backward image (36 KiB) and the forward
// image (46 KiB + 2 KiB that the fixed-count LDS-DMA overruns into).
constexpr int kImg = 128 * 128;
constexpr int kOffImg = 0;
constexpr int kOffX2 = 4 * kImg;                          // 65536
constexpr int kOffRed = kOffX2 + 128 * 64;                // 73728
constexpr int kOffWb = kOffRed + 256;                     // 73984
constexpr int kOffWf = kOffWb + kT16BwdFrags * 1024;      // 110848
constexpr int kLds = kOffWf + 48 * 1024;                  // 160000
static_assert(kLds <= 160 * 1024, "LDS budget");

// Transposed-read operand of one 16-feature tile over the block's 128 samples (4 k-steps of 32): the lane's byte
// offsets of its two reads (samples 8G + q and 8G + 4 + q of each k-step) and the image's bytes per 32 samples.
struct TrTile {
    const char* img;
    int o0, o1, stride;
};
__device__ __forceinline__ h8 tr_op(const TrTile& t, int kk) {
    return tr_pair(t.img + t.o0 + t.stride * kk, t.img + t.o1 + t.stride * kk);
}

// dW tiles A_i x B_j (i < NA, j < NB) over 128 samples: A = delta-image tiles (rows), B = activation-image tiles
// (columns). Every operand read is issued before the first MFMA.
template <int NA, int NB, int KS = 4>  // KS k-steps of 32 samples (the block's samples)
__device__ __forceinline__ void dw_tiles(const TrTile (&ta)[NA], const TrTile (&tb)[NB], f4 (&acc)[NA][NB]) {
    h8 A[NA][KS], B[NB][KS];
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) A[i][kk] = tr_op(ta[i], kk);
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) B[j][kk] = tr_op(tb[j], kk);
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[i][j] = mfma16(A[i][kk], B[j][kk], acc[i][j]);
}

// backward fragments of W_L^T (L = 1..4), 4 M-blocks x 2 k-steps
template <int L>
__device__ __forceinline__ void load_wt(const h8* lwb, int lane, h8 (&W)[4][2]) {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int s = 0; s < 2; ++s) W[mb][s] = lwb[t16_bwd_frag(L, mb, s) * 64 + lane];
}

constexpr int kWaves = 4;  // 4 waves x 2 groups x 16 samples = 128 samples per block

// Role-split variant (NRC_T16_SPLIT, A/B): 8 waves per block, 2 per SIMD. Waves 0..3 ("chain") do what
// train16_kernel's waves do except the weight gradients: encode, forward, loss, then per backward step the delta chain
// (W_L^T delta_L, ReLU gate) and the image writes. Waves 4..7 ("dW") sit through the forward at its barriers and then,
// in each backward step, compute the block's dW_L tiles from the images the chain waves wrote in the step before and
// stream them to the slab. The two halves of a step share the SIMDs' MFMA pipes and hide each other's LDS and
// dependency latency; the step's critical path is the chain alone instead of chain + dW.
// G: 16-sample groups per chain wave (64 G samples per block); PADQ: padded RadianceQuery records (16 floats: the
// position load takes pad_ along, 16 bytes instead of 12, the other loads one float further)
// ENC 3 / 1 (round 5): InputEncoding::Hash -- the encoder reads each lane group's 4 grid levels (t16_hash_slot_feature)
// from the batch's feature pass (3) or gathers them from the table (1, A/B),
// and after the last chain step the chain waves form dL/d(grid features) = W0^T delta_0 (4 MFMAs per group from the
// backward image's fragments 36..39, read from global memory) and write it with the sample positions for
// grid_scatter_kernel (ho). Everything else -- forward, loss, delta chain, dW waves, slab layout -- is the Frequency
// kernel's.
// The body takes the block's LDS and index from its kernel (train16_split_kernel, or the fused step's trainer blocks).
// PRIO (debug library, A/B): 1 = the dW waves at s_setprio 1, 2 = the chain waves at s_setprio 1 (issue arbitration
// is by priority, then age; the chain waves are the older half)
// GATHER 1 / 2 (nrc_train_gather, G = 2, Frequency; 1 a permutation array, 2 Feistel -- two builds, so that no load
// sits behind a branch: tools/asm_hazard_check.py rule 2): q / t are the traced buffers and the step's sample d is their record
// perm(gs.first + d) % gs.nrec (nrc_shuffle.h) -- the shuffle's copy (permute_kernel) never happens. A chain wave's 32
// samples take one source row each: lane l (and l + 32) derives sample l & 31's, the lane group that loads the
// sample fetches it with one ds_bpermute. The index -> row hop hides behind the forward image's DMAs: the
// permutation entry (4 B) is the wave's oldest load, layers 0 and 1 (DMAs 0..4) go out behind it, then the row
// (Feistel: computed here instead, no load), the record loads through per-lane 64-bit rows -- the dense loads, whose
// dwordx3 / dwordx2 split already serves 60-B records at odd rows (4-byte aligned) -- and DMAs 5..11. One wait,
// vmcnt(7), covers the records and layers 0, 1; every later count sees the same younger loads as the dense kernel.
template <int AUX, int G = 2, bool PADQ = false, int ENC = 0, int PRIO = 0, int GATHER = 0>
__device__ __forceinline__ void train16_split_body(char* __restrict__ smem, const int blk,
                                                   const float* __restrict__ q, const float* __restrict__ t, int64_t b,
                                                   float n_total, float loss_scale, const h8* __restrict__ wf,
                                                   const h8* __restrict__ wb, _Float16* __restrict__ slabs,
                                                   float* __restrict__ loss_partials, const HashTrainOut& ho,
                                                   const GatherSrc& gs = GatherSrc{}) {
    static_assert(!GATHER || (G == 2 && ENC == 0), "the gather form is the production Frequency shape");
    const int lane = threadIdx.x & 63;
    h8* lwb = (h8*)(smem + kOffWb);
    h8* lwf = (h8*)(smem + kOffWf);
    char* const img_a0 = smem + kOffImg;
    char* const img_a1 = smem + kOffImg + kImg;
    char* const img_d0 = smem + kOffImg + 2 * kImg;
    char* const img_d1 = smem + kOffImg + 3 * kImg;
    char* const img_x2 = smem + kOffX2;
    float* red = (float*)(smem + kOffRed);
    const int wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool dw_wave = wave_all >= kWaves;
    const int wave = dw_wave ? wave_all - kWaves : wave_all;
    const int g = lane >> 4, c = lane & 15;
    _Float16* slab = slabs + (int64_t)blk * slab_floats(0);

    if (dw_wave) {
        if constexpr (PRIO == 1) __builtin_amdgcn_s_setprio(1);
        // ---- dW waves: the forward's six barriers, then one dW step per backward step
        for (int i = 0; i < 6; ++i) lds_barrier();
        const int lg = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
        const int r0 = 8 * lg + qq, r1 = r0 + 4;
        const int tm0 = 2 * (wave >> 1), tn0 = 2 * (wave & 1);
        int oa[2][2], ob[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            oa[i][0] = off64(r0, 4 * (tm0 + i) + pp);
            oa[i][1] = off64(r1, 4 * (tm0 + i) + pp);
            ob[i][0] = off64(r0, 4 * (tn0 + i) + pp);
            ob[i][1] = off64(r1, 4 * (tn0 + i) + pp);
        }
        // step 5 (buffer 1): dW5 tile (0, wave)
        {
            f4 acc[1][1];
            const TrTile ta[1] = {TrTile{img_d1, off64(r0, pp), off64(r1, pp), 4096}};
            const TrTile tb[1] = {TrTile{img_a1, off64(r0, 4 * wave + pp), off64(r1, 4 * wave + pp), 4096}};
            dw_tiles<1, 1, 2 * G>(ta, tb, acc);
            slab_single_b<AUX>(slab, 5, 0, wave, lane, acc[0][0]);
        }
        lds_barrier();
        // steps 4..1: dW_L tiles (tm0 + i, tn0 + j) from buffer L & 1
#pragma unroll
        for (int L = 4; L >= 1; --L) {
            const char* imgd = (L & 1) ? img_d1 : img_d0;
            const char* imga = (L & 1) ? img_a1 : img_a0;
            TrTile ta[2], tb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ta[i] = TrTile{imgd, oa[i][0], oa[i][1], 4096};
                tb[i] = TrTile{imga, ob[i][0], ob[i][1], 4096};
            }
            f4 acc[2][2];
            dw_tiles<2, 2, 2 * G>(ta, tb, acc);
#pragma unroll
            for (int i = 0; i < 2; ++i) slab_pair_b<AUX>(slab, L, tm0 + i, tn0, lane, pack_pair(acc[i][0], acc[i][1]));
            lds_barrier();
        }
        // step 0 (buffer 0): dW0 tiles (tm0 + i, 3 (wave & 1) + j); columns 4, 5 are K slots 64..95 (img_x2)
        {
            f4 acc[2][3];
            const TrTile ta[2] = {TrTile{img_d0, oa[0][0], oa[0][1], 4096}, TrTile{img_d0, oa[1][0], oa[1][1], 4096}};
            if ((wave & 1) == 0) {
                const TrTile tb[3] = {TrTile{img_a0, off64(r0, pp), off64(r1, pp), 4096},
                                      TrTile{img_a0, off64(r0, 4 + pp), off64(r1, 4 + pp), 4096},
                                      TrTile{img_a0, off64(r0, 8 + pp), off64(r1, 8 + pp), 4096}};
                dw_tiles<2, 3, 2 * G>(ta, tb, acc);
            } else {
                const TrTile tb[3] = {TrTile{img_a0, off64(r0, 12 + pp), off64(r1, 12 + pp), 4096},
                                      TrTile{img_x2, off32(r0, pp), off32(r1, pp), 2048},
                                      TrTile{img_x2, off32(r0, 4 + pp), off32(r1, 4 + pp), 2048}};
                dw_tiles<2, 3, 2 * G>(ta, tb, acc);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if ((wave & 1) == 0) {
                    slab_pair_b<AUX>(slab, 0, tm0 + i, 0, lane, pack_pair(acc[i][0], acc[i][1]));
                    slab_single_b<AUX>(slab, 0, tm0 + i, 2, lane, acc[i][2]);
                } else {
                    slab_single_b<AUX>(slab, 0, tm0 + i, 3, lane, acc[i][0]);
                    slab_pair_b<AUX>(slab, 0, tm0 + i, 4, lane, pack_pair(acc[i][1], acc[i][2]));
                }
            }
        }
        return;
    }

    // ---- chain waves: as train16_kernel
    if constexpr (PRIO == 2) __builtin_amdgcn_s_setprio(1);
    int r[G];
    bool valid[G];
    typedef float f3 __attribute__((ext_vector_type(3)));
    typedef float f4v __attribute__((ext_vector_type(4)));
    typedef std::conditional_t<PADQ, f4v, f3> PQ;
    constexpr int X = PADQ ? 1 : 0;
    PQ pq[G];
    f3 tq[G];
    f2 bl[G], id[G];
    [[maybe_unused]] uint32_t F[G][4];  // ENC 3: the sample's level features 4g .. 4g + 3 (hash_feature_kernel)
    const int gg = g < 3 ? g : 0;
    [[maybe_unused]] uint32_t row = 0;  // GATHER: source record of the wave's sample lane & 31
    if constexpr (GATHER) {
        // padding samples (past b) take the step's last sample, as the dense kernel reads it
        const int64_t sl = (int64_t)blk * (64 * G) + 16 * G * wave + (lane & 31);
        const uint32_t i = gs.first + (uint32_t)(sl < b ? sl : b - 1);
        uint32_t p = 0;
        if constexpr (GATHER == 1) asm volatile("global_load_dword %0, %1, off" : "=v"(p) : "v"(gs.perm + i) : "memory");
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int f = wave + kWaves * k;
            __builtin_amdgcn_global_load_lds((const void*)(wf + f * 64 + lane),
                                             (__attribute__((address_space(3))) void*)(lwf + f * 64), 16, 0, 0);
        }
        if constexpr (GATHER == 1) asm volatile("s_waitcnt vmcnt(5)" : "+v"(p) : : "memory");
        else p = feistel_perm(i, gs.fk);
        row = p % gs.nrec;
        asm volatile("" : "+v"(row));  // one division per sample: not sunk below the two bpermutes
    }
#pragma unroll
    for (int u = 0; u < G; ++u) {
        r[u] = 16 * (G * wave + u) + c;
        const int64_t s = (int64_t)blk * (64 * G) + r[u];
        valid[u] = s < b;
        int64_t sc = valid[u] ? s : b - 1;
        if constexpr (GATHER) sc = (uint32_t)__shfl((int)row, 16 * u + c);
        const float* qr = q + sc * (NRC_INPUT_DIMS + X);
        if constexpr (PADQ) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(pq[u]) : "v"(qr) : "memory");
        else asm volatile("global_load_dwordx3 %0, %1, off" : "=v"(pq[u]) : "v"(qr) : "memory");
        asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(bl[u]) : "v"(qr + 3 + X + 2 * gg) : "memory");
        asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(id[u]) : "v"(qr + 9 + X + 2 * gg) : "memory");
        asm volatile("global_load_dwordx3 %0, %1, off" : "=v"(tq[u]) : "v"(t + sc * 3) : "memory");
        if constexpr (ENC == 3) {
            // padding samples read the last sample's features (finite), as they read its query
            const uint32_t* fr = ho.feat + (int64_t)(4 * g) * kHashFeatStride + sc;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                asm volatile("global_load_dword %0, %1, off" : "=v"(F[u][i]) : "v"(fr + i * kHashFeatStride) : "memory");
        }
    }
#pragma unroll
    for (int k = GATHER ? 5 : 0; k < 12; ++k) {
        const int f = wave + kWaves * k;
        __builtin_amdgcn_global_load_lds((const void*)(wf + (f < kT16FwdFrags ? f : kT16FwdFrags - 1) * 64 + lane),
                                         (__attribute__((address_space(3))) void*)(lwf + f * 64), 16, 0, 0);
    }
    if constexpr (GATHER)  // the records and DMAs 0..4 (issued before them); DMAs 5..11 may be in flight
        asm volatile("s_waitcnt vmcnt(7)"
                     : "+v"(pq[0]), "+v"(pq[1]), "+v"(bl[0]), "+v"(bl[1]), "+v"(id[0]), "+v"(id[1]), "+v"(tq[0]), "+v"(tq[1])
                     :
                     : "memory");
    else if constexpr (G == 2 && ENC == 3)
        asm volatile("s_waitcnt vmcnt(12)"
                     : "+v"(pq[0]), "+v"(pq[1]), "+v"(bl[0]), "+v"(bl[1]), "+v"(id[0]), "+v"(id[1]), "+v"(tq[0]), "+v"(tq[1]),
                       "+v"(F[0][0]), "+v"(F[0][1]), "+v"(F[0][2]), "+v"(F[0][3]), "+v"(F[1][0]), "+v"(F[1][1]),
                       "+v"(F[1][2]), "+v"(F[1][3])
                     :
                     : "memory");
    else if constexpr (G == 2)
        asm volatile("s_waitcnt vmcnt(12)"
                     : "+v"(pq[0]), "+v"(pq[1]), "+v"(bl[0]), "+v"(bl[1]), "+v"(id[0]), "+v"(id[1]), "+v"(tq[0]), "+v"(tq[1])
                     :
                     : "memory");
    else
        asm volatile("s_waitcnt vmcnt(12)" : "+v"(pq[0]), "+v"(bl[0]), "+v"(id[0]), "+v"(tq[0]) : : "memory");
    h8 x[G][3];
    float tg[G][3];
#pragma unroll
    for (int u = 0; u < G; ++u) {
        tg[u][0] = tq[u].x; tg[u][1] = tq[u].y; tg[u][2] = tq[u].z;
        float pad = 1.0f;
        if constexpr (PADQ) pad = pq[u].w;
        if constexpr (ENC == 3) encode16_hashf(F[u], bl[u].x, bl[u].y, id[u].x, id[u].y, g, x[u], pad);
        else if constexpr (ENC == 1) encode16_hash(pq[u].x, pq[u].y, pq[u].z, bl[u].x, bl[u].y, id[u].x, id[u].y, g, ho.table, x[u], pad);
        else encode16(pq[u].x, pq[u].y, pq[u].z, bl[u].x, bl[u].y, id[u].x, id[u].y, g, x[u], pad);
        const u4 w = __builtin_bit_cast(u4, x[u][2]);
        *(u2*)(img_x2 + off32(r[u], 2 * g)) = u2{w.x, w.y};
        *(u2*)(img_x2 + off32(r[u], 2 * g + 1)) = u2{w.z, w.w};
    }
    asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    lds_barrier();  // barrier 1
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int f = wave + kWaves * k;
        __builtin_amdgcn_global_load_lds((const void*)(wb + f * 64 + lane),
                                         (__attribute__((address_space(3))) void*)(lwb + f * 64), 16, 0, 0);
    }
    h8 a[5][G][2];
    f4 o[G];
    {
        h8 w0[12], w1[8];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) w0[mb * 3 + ks] = lwf[t16_fwd_frag(0, mb, ks) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 8; ++i) w1[i] = lwf[t16_fwd_frag(1, i >> 1, i & 1) * 64 + lane];
        __builtin_amdgcn_sched_barrier(0);
        f4 cc[G][4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
            for (int u = 0; u < G; ++u) cc[u][mb] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 3; ++ks)
#pragma unroll
                for (int u = 0; u < G; ++u) cc[u][mb] = mfma16(w0[mb * 3 + ks], x[u][ks], cc[u][mb]);
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
            a[0][u][0] = relu_b(cc[u][0], cc[u][1]);
            a[0][u][1] = relu_b(cc[u][2], cc[u][3]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int l = 1; l < 6; ++l) {
            h8 wn[8];
            if (l < 5) {
                if (l == 1) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
                if (l == 2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
                if (l == 3) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
                if (l == 4) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
                lds_barrier();  // barriers 2..5
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (l + 1 < 5 || i < 2) wn[i] = lwf[t16_fwd_frag(l + 1, l + 1 < 5 ? i >> 1 : 0, i & 1) * 64 + lane];
            }
            __builtin_amdgcn_sched_barrier(0);
            if (l < 5) {
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
                    for (int u = 0; u < G; ++u) cc[u][mb] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                        for (int u = 0; u < G; ++u) cc[u][mb] = mfma16(w1[mb * 2 + ks], a[l - 1][u][ks], cc[u][mb]);
                }
#pragma unroll
                for (int u = 0; u < G; ++u) {
                    a[l][u][0] = relu_b(cc[u][0], cc[u][1]);
                    a[l][u][1] = relu_b(cc[u][2], cc[u][3]);
                }
            } else {
#pragma unroll
                for (int u = 0; u < G; ++u) o[u] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int u = 0; u < G; ++u) o[u] = mfma16(w1[ks], a[4][u][ks], o[u]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 8; ++i) w1[i] = wn[i];
        }
    }
    float lossv = 0.0f;
    h4 d5[G];
#pragma unroll
    for (int u = 0; u < G; ++u) d5[u] = h4{};
    if (g == 0) {
#pragma unroll
        for (int u = 0; u < G; ++u) {
            float y[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) y[k] = (float)(_Float16)fmaxf(o[u][k], 0.0f);
            const float lum = 0.299f * y[0] + 0.587f * y[1] + 0.114f * y[2];
            const float inv = 1.0f / ((lum * lum + NRC_LUM_EPS) * n_total);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float diff = y[k] - tg[u][k];
                lossv += valid[u] ? diff * diff * inv : 0.0f;
                d5[u][k] = (valid[u] && y[k] > 0.0f) ? (_Float16)(loss_scale * 2.0f * diff * inv) : (_Float16)0.0f;
            }
        }
    }
    lossv = row_sum16(lossv);
    if (lane == 0) red[wave] = lossv;
    int wo[G][4];
#pragma unroll
    for (int u = 0; u < G; ++u) {
        row_offsets(r[u], g, wo[u]);
        asm volatile("" : "+v"(wo[u][0]), "+v"(wo[u][1]), "+v"(wo[u][2]), "+v"(wo[u][3]));
    }
#pragma unroll
    for (int u = 0; u < G; ++u) {
        *(h4*)(img_d1 + off64(r[u], g)) = d5[u];
        put_rows64(img_a1, wo[u], a[4][u]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // backward image landed
    lds_barrier();  // barrier 6
    if (threadIdx.x == 0) {
        const float lp = (red[0] + red[1]) + (red[2] + red[3]);
        // an agent-scope store (sc1): the fused step's reducers on other XCDs read it in the same launch
        __hip_atomic_store(loss_partials + blk, lp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    h8 d[G][2], dn[G][2], W[4][2];
    // step 5: delta_4 = W5^T delta_5 * [a_4 > 0] (16x16x16: K = 16 output rows) into buffer 0 with a_3
    {
        const h4* lwb4 = (const h4*)lwb;
        h4 W5[4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) W5[mb] = lwb4[t16_bwd_frag(5, mb, 0) * 128 + lane];
#pragma unroll
        for (int u = 0; u < G; ++u) {
            f4 cc[4];
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) cc[mb] = mfma16k16(W5[mb], d5[u], f4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) d[u][s2] = gate_b(cc[2 * s2], cc[2 * s2 + 1], a[4][u][s2]);
            put_rows64(img_d0, wo[u], d[u]);
            put_rows64(img_a0, wo[u], a[3][u]);
        }
        load_wt<4>(lwb, lane, W);
    }
    lds_barrier();
    // steps 4..1: delta_{L-1} into the other buffer with a_{L-2} (step 1: the input slots 0..63)
#define NRC_T16S_STEP(L, NIMGD, NIMGA)                                                                              \
    {                                                                                                              \
        _Pragma("unroll") for (int u = 0; u < G; ++u) {                                                            \
            if constexpr (L > 1) {                                                                                 \
                put_rows64(NIMGA, wo[u], a[L > 1 ? L - 2 : 0][u]);                                                 \
            } else {                                                                                               \
                _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                 \
                    const u4 w = __builtin_bit_cast(u4, x[u][ks]);                                                 \
                    *(u2*)(NIMGA + off64(r[u], 8 * ks + 2 * g)) = u2{w.x, w.y};                                    \
                    *(u2*)(NIMGA + off64(r[u], 8 * ks + 2 * g + 1)) = u2{w.z, w.w};                                \
                }                                                                                                  \
            }                                                                                                      \
        }                                                                                                          \
        chain_groups<G>(W, d, a[L - 1], dn);                                                                                \
        if constexpr (L > 1) load_wt<(L > 1 ? L - 1 : 1)>(lwb, lane, W);                                           \
        _Pragma("unroll") for (int u = 0; u < G; ++u) {                                                            \
            put_rows64(NIMGD, wo[u], dn[u]);                                                                       \
            _Pragma("unroll") for (int s2 = 0; s2 < 2; ++s2) d[u][s2] = dn[u][s2];                                 \
        }                                                                                                          \
    }                                                                                                              \
    lds_barrier();
    // Hash: W0^T of the grid features (16x16x32 A operands, fragments 36 + 2 mb + s), loaded from global memory during
    // the chain (they are read once, after the last step)
    [[maybe_unused]] h8 W0g[2][2];
    if constexpr (ENC == 1 || ENC == 3) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int s = 0; s < 2; ++s) W0g[mb][s] = wb[(kT16BwdFrags + 2 * mb + s) * 64 + lane];
    }
    NRC_T16S_STEP(4, img_d1, img_a1)
    NRC_T16S_STEP(3, img_d0, img_a0)
    NRC_T16S_STEP(2, img_d1, img_a1)
    NRC_T16S_STEP(1, img_d0, img_a0)
#undef NRC_T16S_STEP
    if constexpr (ENC == 1 || ENC == 3) {
        // dL/d(grid slot 16 mb + 4 g + i) of sample c = (W0^T delta_0): registers (0, 1) / (2, 3) of M-block mb are the
        // two features of levels 8 mb + 2 g and 8 mb + 2 g + 1; f16 pairs [level][sample], zeros for padding samples
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int64_t sg = (int64_t)blk * (64 * G) + r[u];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                f4 c = mfma16(W0g[mb][0], d[u][0], f4{0.f, 0.f, 0.f, 0.f});
                c = mfma16(W0g[mb][1], d[u][1], c);
                const int lv = 8 * mb + 2 * g;
                ho.dy[(int64_t)lv * ho.bcap + sg] = valid[u] ? pk2(c[0], c[1]) : 0u;
                ho.dy[(int64_t)(lv + 1) * ho.bcap + sg] = valid[u] ? pk2(c[2], c[3]) : 0u;
            }
            if (g == 0) ho.pos[sg] = float4{pq[u].x, pq[u].y, pq[u].z, 0.0f};
        }
    }
}

}  // namespace
}  // namespace nrc_amd
