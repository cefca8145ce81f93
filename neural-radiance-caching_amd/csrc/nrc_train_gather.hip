// nrc_train_gather.hip -- the gather form of the role-split Frequency training kernel (nrc_train_gather,
// include/nrc/frame.h; DESIGN.md section 9 "Gathered training step"): train16_split_body with GATHER, in a unit of its
// own. The gather form of the decoupled-chain kernel (small batches) is in nrc_train_dc.hip.
#include "nrc_train16_split.h"

namespace nrc_amd {
namespace {

// The gather form of train16_split_kernel<16, 2, PADQ> (nrc_train_gather): same blocks, slabs and loss partials, the
// samples read from the traced buffers through the shuffle's permutation. SRC: 1 permutation array, 2 Feistel.
template <bool PADQ, int SRC>
__global__ __launch_bounds__(512, 1) void train16_gather_kernel(const float* __restrict__ q, const float* __restrict__ t,
                                                                int64_t b, float n_total, float loss_scale,
                                                                const h8* __restrict__ wf, const h8* __restrict__ wb,
                                                                _Float16* __restrict__ slabs,
                                                                float* __restrict__ loss_partials, GatherSrc gs) {
    __shared__ __attribute__((aligned(16))) char smem[kLds];
    train16_split_body<16, 2, PADQ, 0, 0, SRC>(smem, blockIdx.x, q, t, b, n_total, loss_scale, wf, wb, slabs,
                                               loss_partials, HashTrainOut{}, gs);
}

}  // namespace

hipError_t launch_train16_gather(const float* queries_src, const float* targets_src, const GatherSrc& gs, int64_t b,
                                 float n_total, float loss_scale, const _Float16* wf, const _Float16* wb,
                                 _Float16* slabs, float* loss_partials, hipStream_t s, bool padq) {
    if (b <= 0) return hipSuccess;
    // every row the kernel forms stays below nrec; every permutation index below first + b <= n_out
    if (gs.nrec == 0 || gs.nrec > gs.fk.n || (uint64_t)gs.first + (uint64_t)b > gs.fk.n) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((b + 127) / 128)), block(128 * kWaves);
    const h8 *f = (const h8*)wf, *bw = (const h8*)wb;
#define NRC_T16_GATHER(PADQ, SRC)                                                                                   \
    hipLaunchKernelGGL((train16_gather_kernel<PADQ, SRC>), grid, block, 0, s, queries_src, targets_src, b, n_total, \
                       loss_scale, f, bw, slabs, loss_partials, gs)
    if (padq && gs.perm) NRC_T16_GATHER(true, 1);
    else if (padq) NRC_T16_GATHER(true, 2);
    else if (gs.perm) NRC_T16_GATHER(false, 1);
    else NRC_T16_GATHER(false, 2);
#undef NRC_T16_GATHER
    return hipGetLastError();
}

}  // namespace nrc_amd
