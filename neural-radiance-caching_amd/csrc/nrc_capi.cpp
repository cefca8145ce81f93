// nrc_capi.cpp — C-ABI implementation (include/nrc/nrc_c.h). Owns parameters, optimizer state,
// MFMA weight images and workspaces (the reference's tcnn::TrainableModel, NRCNetwork.cu:15-20).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "nrc/frame.h"
#include "nrc/nrc_c.h"
#include "nrc_guard.h"
#include "nrc_internal.h"

using namespace nrc_amd;

namespace {

// pcg32 (tcnn common/random.h) for xavier-uniform init [M: tcnn's init cannot be reproduced bit for bit].
struct Pcg32 {
    uint64_t state = 0, inc = 1;
    Pcg32(uint64_t initstate, uint64_t initseq) {
        inc = (initseq << 1u) | 1u;
        next();
        state += initstate;
        next();
    }
    uint32_t next() {
        uint64_t old = state;
        state = old * 6364136223846793005ULL + inc;
        uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
        uint32_t rot = (uint32_t)(old >> 59u);
        return (xs >> rot) | (xs << ((~rot + 1u) & 31));
    }
    float next_float() {
        uint32_t u = (next() >> 9) | 0x3f800000u;
        float f;
        std::memcpy(&f, &u, 4);
        return f - 1.0f;
    }
};

constexpr int kLayerIn[NRC_NUM_LAYERS] = {NRC_ENC_WIDTH, 64, 64, 64, 64, 64};
constexpr int kLayerOut[NRC_NUM_LAYERS] = {64, 64, 64, 64, 64, NRC_OUT_PADDED};
constexpr int kLayerOff[NRC_NUM_LAYERS] = {NRC_W0_OFFSET, NRC_W1_OFFSET, NRC_W2_OFFSET,
                                           NRC_W3_OFFSET, NRC_W4_OFFSET, NRC_W5_OFFSET};

void init_params(std::vector<float>& p, uint64_t seed) {
    Pcg32 rng(seed, 0xda3e39cb94b95bdbULL);
    for (int l = 0; l < NRC_NUM_LAYERS; ++l) {
        const float scale = std::sqrt(6.0f / (float)(kLayerIn[l] + kLayerOut[l]));
        const int cnt = kLayerIn[l] * kLayerOut[l];
        for (int i = 0; i < cnt; ++i) p[kLayerOff[l] + i] = (rng.next_float() * 2.0f - 1.0f) * scale;
    }
}

// Hash config (oracle/nrc_hash_oracle.c orc_hash_init_params): the same xavier stream over the 64-wide layer 0,
// grid uniform in [-1e-4, 1e-4] from a second pcg32 stream [M].
void init_params_hash(std::vector<float>& p, uint64_t seed) {
    const int in[NRC_NUM_LAYERS] = {NRC_HASH_ENC_WIDTH, 64, 64, 64, 64, 64};
    const int off[NRC_NUM_LAYERS] = {NRC_HASH_W0_OFFSET, NRC_HASH_W1_OFFSET, NRC_HASH_W1_OFFSET + 4096,
                                     NRC_HASH_W1_OFFSET + 8192, NRC_HASH_W1_OFFSET + 12288, NRC_HASH_W5_OFFSET};
    Pcg32 rng(seed, 0xda3e39cb94b95bdbULL);
    for (int l = 0; l < NRC_NUM_LAYERS; ++l) {
        const float scale = std::sqrt(6.0f / (float)(in[l] + kLayerOut[l]));
        for (int i = 0; i < in[l] * kLayerOut[l]; ++i) p[off[l] + i] = (rng.next_float() * 2.0f - 1.0f) * scale;
    }
    Pcg32 g(seed, 0x9e3779b97f4a7c15ULL);
    for (int i = 0; i < NRC_HASH_GRID_PARAMS; ++i) p[NRC_HASH_GRID_OFFSET + i] = (g.next_float() * 2.0f - 1.0f) * 1e-4f;
}

// Width-128 network (BASELINE configs[4]): the same xavier-uniform stream over the wide shapes.
void init_params_wide(std::vector<float>& p, uint64_t seed) {
    const int in[NRC_NUM_LAYERS] = {NRC_ENC_WIDTH, 128, 128, 128, 128, 128};
    const int out[NRC_NUM_LAYERS] = {128, 128, 128, 128, 128, NRC_OUT_PADDED};
    Pcg32 rng(seed, 0xda3e39cb94b95bdbULL);
    int off = 0;
    for (int l = 0; l < NRC_NUM_LAYERS; ++l) {
        const float scale = std::sqrt(6.0f / (float)(in[l] + out[l]));
        for (int i = 0; i < in[l] * out[l]; ++i) p[off + i] = (rng.next_float() * 2.0f - 1.0f) * scale;
        off += in[l] * out[l];
    }
}

// Parameter of every position of the fragment-major weight-gradient slab (nrc_internal.h slab_block_base):
// position (block, j, lane, e) holds accumulator register 4j + e of that lane, i.e. dW[row][col] with
// row = 32 mb + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), col = 32 nb + (lane & 31) (layer 0: K slot -> feature).
std::vector<int> build_slab_map(int encoding) {
    const bool hash = encoding == NRC_ENCODING_HASH;
    const int enc = hash ? 1 : encoding == NRC_ENCODING_FREQUENCY_SH ? 2 : 0;
    const int in0 = hash ? NRC_HASH_ENC_WIDTH : NRC_ENC_WIDTH;
    int off[NRC_NUM_LAYERS];
    for (int l = 0; l < NRC_NUM_LAYERS; ++l)
        off[l] = hash ? (l == 0 ? NRC_HASH_W0_OFFSET : l <= 4 ? NRC_HASH_W1_OFFSET + (l - 1) * 4096 : NRC_HASH_W5_OFFSET)
                      : kLayerOff[l];
    std::vector<int> m(slab_floats(enc), -1);
    for (int L = 0; L < NRC_NUM_LAYERS; ++L) {
        const int nmb = L == 5 ? 1 : 2, nnb = L == 0 ? slab_l0_nb(enc) : 2, nreg = L == 5 ? 8 : 16;
        const int in_dim = L == 0 ? in0 : 64;
        for (int mb = 0; mb < nmb; ++mb)
            for (int nb = 0; nb < nnb; ++nb)
                for (int lane = 0; lane < 64; ++lane)
                    for (int reg = 0; reg < nreg; ++reg) {
                        const int row = 32 * mb + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                        const int col = 32 * nb + (lane & 31);
                        if (L == 0 && col >= in0) continue;  // x_hi block lanes past the 80 inputs
                        const int fcol = L == 0 ? enc_k0_feature(enc, col) : col;
                        const int pos = slab_block_base(enc, L, mb, nb) + ((reg >> 2) * 64 + lane) * 4 + (reg & 3);
                        m[pos] = off[L] + row * in_dim + fcol;
                    }
    }
    return m;
}

// Position of every canonical parameter inside the forward / backward MFMA fragment images.
void build_scatter_maps(std::vector<int>& fwd, std::vector<int>& bwd, int encoding) {
    const bool hash = encoding == NRC_ENCODING_HASH;
    const int n = hash ? NRC_HASH_MLP_PARAMS : NRC_NUM_PARAMS;
    const int in0 = hash ? NRC_HASH_ENC_WIDTH : NRC_ENC_WIDTH;
    int off[NRC_NUM_LAYERS];
    for (int l = 0; l < NRC_NUM_LAYERS; ++l)
        off[l] = hash ? (l == 0 ? NRC_HASH_W0_OFFSET : l <= 4 ? NRC_HASH_W1_OFFSET + (l - 1) * 4096 : NRC_HASH_W5_OFFSET)
                      : kLayerOff[l];
    fwd.assign(n, -1);
    bwd.assign(n, -1);
    // inverse of acc_row over (kk, h, j) for a 64-feature axis
    int row_kk[64], row_h[64], row_j[64];
    for (int kk = 0; kk < 4; ++kk)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < 8; ++j) {
                const int r = acc_row(kk, h, j);
                row_kk[r] = kk;
                row_h[r] = h;
                row_j[r] = j;
            }
    int f_kk[NRC_ENC_WIDTH], f_h[NRC_ENC_WIDTH], f_j[NRC_ENC_WIDTH];
    for (int h = 0; h < 2; ++h)
        for (int sn = 0; sn < (hash ? 32 : 40); ++sn) {
            const int f = hash                                  ? hash_slot_feature(sn, h)
                          : encoding == NRC_ENCODING_FREQUENCY_SH ? sh_slot_feature(sn, h)
                                                                : slot_feature(sn, h);
            f_kk[f] = sn / 8;
            f_h[f] = h;
            f_j[f] = sn % 8;
        }
    auto pos = [](int frag, int lane, int j) { return frag * kFragHalves + lane * 8 + j; };
    for (int o = 0; o < 64; ++o)
        for (int f = 0; f < in0; ++f) {
            const int p = off[0] + o * in0 + f;
            fwd[p] = pos(fwd_frag(0, o / 32, f_kk[f]), o % 32 + 32 * f_h[f], f_j[f]);
            // Hash: W0^T for the 32 grid features, rows permuted (hash_dx_row), k order = delta_0's acc_row order
            if (hash && f < 2 * NRC_HASH_LEVELS)
                bwd[p] = pos(kBwdFrags + row_kk[o], hash_dx_row(f) + 32 * row_h[o], row_j[o]);
        }
    for (int l = 1; l <= 4; ++l)
        for (int o = 0; o < 64; ++o)
            for (int i = 0; i < 64; ++i) {
                const int p = off[l] + o * 64 + i;
                fwd[p] = pos(fwd_frag(l, o / 32, row_kk[i]), o % 32 + 32 * row_h[i], row_j[i]);
                bwd[p] = pos(bwd_frag(l, i / 32, row_kk[o]), i % 32 + 32 * row_h[o], row_j[o]);
            }
    for (int o = 0; o < NRC_OUT_PADDED; ++o)
        for (int i = 0; i < 64; ++i) {
            const int p = off[5] + o * 64 + i;
            fwd[p] = pos(fwd_frag(5, 0, row_kk[i]), o + 32 * row_h[i], row_j[i]);
            // W5^T: rows acc_row(0, h, j) in [0,16) index the output neuron o
            bwd[p] = pos(bwd_frag(5, i / 32, 0), i % 32 + 32 * row_h[o], row_j[o]);
        }
}

// The same two maps for the t16 training layout (Frequency, nrc_train16.hip): position in the 16x16x32 forward
// training image (fwdt) and in its backward image (bwd). The inference image keeps build_scatter_maps' fwd.
// Hash (round 5): its layer offsets and slot map (t16_hash_slot_feature), and W0^T of the 32 grid features in the
// backward image's fragments 36..39 (kT16BwdFragsHash).
int t16_layer_off(int encoding, int l) {
    if (encoding != NRC_ENCODING_HASH) return kLayerOff[l];
    return l == 0 ? NRC_HASH_W0_OFFSET : l <= 4 ? NRC_HASH_W1_OFFSET + (l - 1) * 4096 : NRC_HASH_W5_OFFSET;
}
int t16_feature(int encoding, int K) {
    return encoding == NRC_ENCODING_HASH ? t16_hash_slot_feature(K) : t16_slot_feature(K);
}

void build_t16_maps(std::vector<int>& fwdt, std::vector<int>& bwd, int encoding) {
    const bool hash = encoding == NRC_ENCODING_HASH;
    const int n = hash ? NRC_HASH_MLP_PARAMS : NRC_NUM_PARAMS, in0 = hash ? NRC_HASH_ENC_WIDTH : NRC_ENC_WIDTH;
    int off[NRC_NUM_LAYERS];
    for (int l = 0; l < NRC_NUM_LAYERS; ++l) off[l] = t16_layer_off(encoding, l);
    fwdt.assign(n, -1);
    bwd.assign(n, -1);
    auto pos = [](int frag, int lane, int j) { return frag * kFragHalves + lane * 8 + j; };
    // row o of a 64-row operand <-> (k-step s, lane group g, element j) of t16_row
    auto sgj = [](int o, int& s, int& g, int& j) {
        s = o >> 5;
        g = (o >> 2) & 3;
        j = 4 * ((o >> 4) & 1) + (o & 3);
    };
    for (int K = 0; K < 96; ++K) {
        const int f = t16_feature(encoding, K);
        if (f < 0) continue;
        for (int o = 0; o < 64; ++o) {
            fwdt[off[0] + o * in0 + f] = pos(t16_fwd_frag(0, o >> 4, K >> 5), 16 * ((K >> 3) & 3) + (o & 15), K & 7);
            if (hash && f < 2 * NRC_HASH_LEVELS) {
                // W0^T: A[grid slot f (M-block f >> 4, row f & 15)][k = row o of delta_0 (k-step s, group g, element j)]
                int s, g, j;
                sgj(o, s, g, j);
                bwd[off[0] + o * in0 + f] = pos(kT16BwdFrags + 2 * (f >> 4) + s, 16 * g + (f & 15), j);
            }
        }
    }
    for (int l = 1; l <= 4; ++l)
        for (int o = 0; o < 64; ++o)
            for (int i = 0; i < 64; ++i) {
                const int p = off[l] + o * 64 + i;
                int s, g, j;
                sgj(i, s, g, j);
                fwdt[p] = pos(t16_fwd_frag(l, o >> 4, s), 16 * g + (o & 15), j);
                sgj(o, s, g, j);
                bwd[p] = pos(t16_bwd_frag(l, i >> 4, s), 16 * g + (i & 15), j);
            }
    for (int o = 0; o < NRC_OUT_PADDED; ++o)
        for (int i = 0; i < 64; ++i) {
            const int p = off[5] + o * 64 + i;
            int s, g, j;
            sgj(i, s, g, j);
            fwdt[p] = pos(t16_fwd_frag(5, 0, s), 16 * g + o, j);
            // W5^T as 16x16x16 A operands: lane (g, m) halves k = 4g + j = output row o, 4 halves per lane
            bwd[p] = t16_bwd_frag(5, i >> 4, 0) * kFragHalves + (16 * (o >> 2) + (i & 15)) * 4 + (o & 3);
        }
}

// Slab map of the t16 layout (t16_slab_pos): register i of lane l of tile (tm, tn) holds dW[16 tm + 4 (l >> 4) + i]
// [16 tn + (l & 15)] (layer 0: column = K slot -> feature, -1 for the dummy slots).
std::vector<int> build_t16_slab_map(int encoding) {
    const bool hash = encoding == NRC_ENCODING_HASH;
    std::vector<int> m(slab_floats(0), -1);
    for (int L = 0; L < NRC_NUM_LAYERS; ++L) {
        const int ntm = L == 5 ? 1 : 4, in_dim = L == 0 ? (hash ? NRC_HASH_ENC_WIDTH : NRC_ENC_WIDTH) : 64;
        for (int tm = 0; tm < ntm; ++tm)
            for (int tn = 0; tn < t16_ntn(L); ++tn)
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < 4; ++i) {
                        const int row = 16 * tm + 4 * (lane >> 4) + i, col = 16 * tn + (lane & 15);
                        const int f = L == 0 ? t16_feature(encoding, col) : col;
                        if (f < 0) continue;
                        m[t16_slab_pos(L, tm, tn, lane, i)] = t16_layer_off(encoding, L) + row * in_dim + f;
                    }
    }
    return m;
}

// Training kernel of a 64-wide Frequency network: the t16-layout kernels (f16 slabs) unless the train_kernel knob
// selects the round-1 32x32x16 train_kernel (in-process A/B; read once per nrc_init).
// Round 5: InputEncoding::Hash too (compact and padded records).
// backward image allocation: the largest layout (32x32 Hash 38 fragments, t16 Frequency 36, t16 Hash 40)
constexpr int kWbHalves = (kBwdFragsHash > kT16BwdFragsHash ? kBwdFragsHash : kT16BwdFragsHash) * kFragHalves;
bool want_t16(int encoding) {
    if (knob(kKnobTrainKernel) == 32) return false;
    return encoding == NRC_ENCODING_FREQUENCY || encoding == NRC_ENCODING_HASH;
}

std::atomic<int> g_knobs[kKnobCount] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
const char* const kKnobNames[kKnobCount] = {"train_kernel", "train_shape", "scatter_min", "scatter_max", "dc_dw0_delay",
                                            "hash_infer", "hash_feat_abl", "t16_groups", "hash_feat_p", "peer_path",
                                            "px_polls", "scatter_part", "scatter_compact", "hash_train_feat",
                                            "hash_adam", "train_fused", "fuse_mode", "tcnn_reentry", "train_prio",
                                            "frame_sparse", "frame_factored_fused", "frame_train_gather",
                                            "frame_culled"};
static_assert(kKnobCount == 23, "one initial value and one name per knob");

std::string config_json(int encoding, const nrc_config& c) {
    char buf[2048];
    if (encoding == NRC_ENCODING_FREQUENCY) {
        std::snprintf(buf, sizeof(buf),
                      "{\"encoding\":{\"nested\":[{\"n_dims_to_encode\":3,\"n_frequencies\":12,\"otype\":"
                      "\"TriangleWave\"},{\"n_bins\":4,\"n_dims_to_encode\":6,\"otype\":\"OneBlob\"},{\"n_dims_to_"
                      "encode\":6,\"otype\":\"Identity\"}],\"otype\":\"Composite\"},\"loss\":{\"otype\":"
                      "\"RelativeL2Luminance\"},\"network\":{\"activation\":\"ReLU\",\"n_hidden_layers\":5,\"n_"
                      "neurons\":64,\"otype\":\"FullyFusedMLP\",\"output_activation\":\"ReLU\"},\"optimizer\":{"
                      "\"decay\":%g,\"nested\":{\"beta1\":%g,\"beta2\":%g,\"epsilon\":%g,\"l2_reg\":%g,\"learning_"
                      "rate\":%g,\"otype\":\"Adam\"},\"otype\":\"EMA\"}}",
                      c.ema_decay, c.beta1, c.beta2, c.epsilon, c.l2_reg, c.learning_rate);
    } else if (encoding == NRC_ENCODING_FREQUENCY_SH) {
        std::snprintf(buf, sizeof(buf),
                      "{\"encoding\":{\"nested\":[{\"n_dims_to_encode\":3,\"n_frequencies\":12,\"otype\":"
                      "\"TriangleWave\"},{\"degree\":4,\"n_dims_to_encode\":2,\"otype\":\"SphericalHarmonics\"},"
                      "{\"n_bins\":4,\"n_dims_to_encode\":4,\"otype\":\"OneBlob\"},{\"n_dims_to_encode\":6,\"otype\":"
                      "\"Identity\"}],\"otype\":\"Composite\"},\"loss\":{\"otype\":\"RelativeL2Luminance\"},"
                      "\"network\":{\"activation\":\"ReLU\",\"n_hidden_layers\":5,\"n_neurons\":64,\"otype\":"
                      "\"FullyFusedMLP\",\"output_activation\":\"ReLU\"},\"optimizer\":{\"decay\":%g,\"nested\":{"
                      "\"beta1\":%g,\"beta2\":%g,\"epsilon\":%g,\"l2_reg\":%g,\"learning_rate\":%g,\"otype\":"
                      "\"Adam\"},\"otype\":\"EMA\"}}",
                      c.ema_decay, c.beta1, c.beta2, c.epsilon, c.l2_reg, c.learning_rate);
    } else {
        std::snprintf(buf, sizeof(buf),
                      "{\"encoding\":{\"nested\":[{\"base_resolution\":16,\"log2_hashmap_size\":15,\"n_dims_to_"
                      "encode\":3,\"n_features_per_level\":2,\"n_levels\":16,\"otype\":\"HashGrid\",\"per_level_"
                      "scale\":2.0},{\"n_bins\":4,\"n_dims_to_encode\":6,\"otype\":\"OneBlob\"},{\"n_dims_to_"
                      "encode\":6,\"otype\":\"Identity\"}],\"otype\":\"Composite\"},\"loss\":{\"otype\":"
                      "\"RelativeL2Luminance\"},\"network\":{\"activation\":\"ReLU\",\"n_hidden_layers\":5,\"n_"
                      "neurons\":64,\"otype\":\"FullyFusedMLP\",\"output_activation\":\"ReLU\"},\"optimizer\":{"
                      "\"decay\":%g,\"nested\":{\"epsilon\":%g,\"l2_reg\":%g,\"learning_rate\":%g,\"otype\":"
                      "\"Adam\"},\"otype\":\"EMA\"}}",
                      c.ema_decay, c.epsilon, c.l2_reg, c.learning_rate);
    }
    std::string r = buf;
    if (c.width != 64) {
        const std::string k = "\"n_neurons\":64";
        const size_t at = r.find(k);
        if (at != std::string::npos) r.replace(at, k.size(), "\"n_neurons\":" + std::to_string(c.width));
    }
    if (c.query_layout == NRC_QUERY_PADDED) {
        // USE_COMPACT_RADIANCE_QUERY 0: Identity(1) of pad_ after the position encoding (NRCNetworkConfigs.h:61-67, :106-111)
        const std::string k = "{\"n_bins\":4";
        const size_t at = r.find(k);
        if (at != std::string::npos) r.insert(at, "{\"n_dims_to_encode\":1,\"otype\":\"Identity\"},");
    }
    return r;
}

}  // namespace

struct nrc_net;
// nrc_peer_exchange_open_local: the handles of one in-process exchange group, each holding raw pointers to the others'
// receive buffers. Every member owns the group; closing any member (nrc_peer_exchange_close, nrc_destroy, a new open on
// a subset) closes all of them after syncing every member's stream, so no handle keeps a pointer to a freed buffer
// (ADVICE r05).
struct LocalPeerGroup {
    std::vector<nrc_net*> members;
};

struct nrc_net {
    hipStream_t stream = nullptr;
    int encoding = NRC_ENCODING_FREQUENCY;
    int config_encoding = NRC_ENCODING_FREQUENCY;  // what nrc_set_config last asked for (JSON only, see there)
    nrc_config cfg{};
    bool initialized = false;
    bool destroyed = false;
    int device = 0;
    uint32_t step = 0;

    float *params = nullptr, *m = nullptr, *v = nullptr, *ema = nullptr, *infer = nullptr;
    _Float16 *wf_train = nullptr, *wb_train = nullptr, *wf_infer = nullptr;
    _Float16* wf_infer16 = nullptr;  // t16 nets: inference image in the t16 layout (nrc_infer16.hip)
    int *fwd_pos = nullptr, *bwd_pos = nullptr;
    int* fwdt_pos = nullptr;  // t16 training layout only (else the training image is laid out as fwd_pos)
    bool t16 = false;         // Frequency training in the t16 layout (f16 slabs)
    // round 6: the role-split step as one launch (launch_train16_fused; knob train_fused, read at nrc_init) and its
    // reducers' counters
    bool fused = false;
    uint32_t* fuse_sync = nullptr;
    uint32_t* fuse_flags = nullptr;  // [kFuseMaxFlags] per trainer block: the generation of its last fused launch
    uint32_t fuse_gen = 0;
    // the next launch's generation: never 0 (the flags' initial value) and never the previous launch's
    uint32_t next_fuse_gen() { return fuse_gen = fuse_gen == 0xFFFFFFFFu ? 1u : fuse_gen + 1u; }
    int t16_kernel = 0;       // 0 decoupled chain (nrc_train_dc.hip, default), 1 / 2 round-2 role split / 4-wave
                              // (nrc_train16.hip); the train_kernel knob at nrc_init
    int* slab_param = nullptr;  // [n_slab] parameter of each weight-gradient slab position
    int n_slab = 0;
    float* slabs = nullptr;
    int slab_blocks = 0;
    float* loss_partials = nullptr;
    // minibatch-loss slots: host-mapped fine-grained (coherent) pinned memory written directly by the reduce/Adam
    // kernels, so reading a loss back costs one stream sync and no D2H copy launch (the copy was ~4.5 us)
    uint32_t* work_queue = nullptr;  // inference work-pool counters (two sets, launch parity pool_parity)
    int pool_parity = 0;
    ncclComm_t comm = nullptr;       // attached RCCL communicator (not owned), nrc_set_comm
    int comm_rank = 0, comm_world = 1;
    float* dp_grad = nullptr;        // [grad_floats] gradient exchange buffer of nrc_train_dp
    void* frame_scratch = nullptr;   // frame driver scratch (net_frame_scratch): the key sort's permutation + temp
    size_t frame_scratch_bytes = 0;
    uint32_t* cull_ws = nullptr;     // nrc_infer_accumulate_culled: row lists, segment counts and the live total of
    uint32_t cull_ws_pixels = 0;     // cull_ws_pixels pixels (cull_workspace_bytes); grown on demand
    float* loss_dev = nullptr;   // device view of loss_host
    float* loss_host = nullptr;
    // training-protocol error word (round 4), in the same mapped allocation as the loss slots (index kProtoErrSlot):
    // the decoupled-chain kernel sets it when a bounded LDS wait runs out (nrc_train_dc.hip lds_wait_ge); sticky until
    // the next nrc_init, checked before every training launch and after every host sync of the training path
    static constexpr int kProtoErrSlot = 4;
    uint32_t* proto_err_dev() const { return reinterpret_cast<uint32_t*>(loss_dev + kProtoErrSlot); }
    void check_protocol() const {
        const uint32_t e = loss_host ? reinterpret_cast<volatile uint32_t*>(loss_host)[kProtoErrSlot] : 0u;
        if (e == 2u)
            throw ApiError(NRC_ERR_INTERNAL,
                           "nrc_train_dp: a peer's gradient did not arrive (peer exchange wait timed out; the step's "
                           "update and every state derived from it are invalid; re-initialise the network)");
        if (e != 0u)
            throw ApiError(NRC_ERR_INTERNAL,
                           "training kernel: an LDS protocol wait timed out (the gradient of that step and every state "
                           "derived from it are invalid; re-initialise the network)");
    }
    // one-shot peer gradient exchange (nrc_peer_exchange_*; round 4): own receive buffer, the IPC-mapped buffers of
    // the peers (px_peers.p[px_rank] = px_buf), the step sequence number (the tag of the last step's words)
    float* px_buf = nullptr;
    PeerPtrs px_peers{};
    int px_world = 0, px_rank = -1;
    uint32_t px_seq = 0;
    bool px_open = false;
    bool px_shared = false;   // a peer's buffer lives on this rank's device (ranks sharing a GPU): split exchange
    bool px_local = false;    // nrc_peer_exchange_open_local: the peers' buffers are other handles' own (no IPC)
    bool px_pending = false;  // knob peer_path 3 pushed a step whose wait + sum + Adam (peer_path 4) is still to run
    std::shared_ptr<LocalPeerGroup> px_group;  // open_local: the group this handle's exchange belongs to
    void peer_close();        // this handle's exchange, and with it its whole local group (defined below)
    void peer_close_own() {
        px_group.reset();
        if (px_open && !px_local)
            for (int r = 0; r < px_world; ++r)
                if (r != px_rank && px_peers.p[r]) (void)hipIpcCloseMemHandle(px_peers.p[r]);
        px_peers = PeerPtrs{};
        if (px_buf) (void)hipFree(px_buf);
        px_buf = nullptr;
        px_world = 0;
        px_rank = -1;
        px_seq = 0;
        px_open = false;
        px_shared = false;
        px_local = false;
        px_pending = false;
    }
    void alloc_loss_slots() {
        HIP_CHECK(hipMalloc(&work_queue, kInferPoolBytes));
        HIP_CHECK(hipMemset(work_queue, 0, kInferPoolBytes));
        HIP_CHECK(hipHostMalloc(&loss_host, sizeof(float) * 8, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_CHECK(hipHostGetDevicePointer((void**)&loss_dev, loss_host, 0));
        for (int i = 0; i < 8; ++i) loss_host[i] = 0.0f;
    }
    // stream-ordered read of loss slot 0 (blocks the host, as the reference's Trainer::loss does)
    float read_loss() {
        HIP_CHECK(hipStreamSynchronize(stream));
        check_protocol();
        return loss_host[0];
    }
    // InputEncoding::Hash: grid part of the model arrays starts at n_mlp
    int n_mlp = NRC_NUM_PARAMS, n_grid = 0;
    int64_t* grid_grad = nullptr;  // [n_grid] exact fixed-point sums (x 2^24) of the f16 grid-gradient contributions
    uint32_t* grid_steps = nullptr;
    float2* grid_bias = nullptr;  // Adam bias-correction table of the grid parameters (GridBuffers::bias)
    _Float16 *table_train = nullptr, *table_infer = nullptr;
    uint32_t* hash_feat = nullptr;  // [NRC_HASH_LEVELS][kHashFeatStride] level features of an inference pass
    uint32_t* hash_feat_arg() const { return knob(kKnobHashInfer) == 1 ? nullptr : hash_feat; }
    // The feature workspace is one per handle, and nrc_infer_stream / the fused accumulation may launch each call on
    // another stream: a Hash inference on stream s first waits for the previous one's MLP pass when that
    // ran on another stream (an event recorded after it), so overlapping calls serialise instead of overwriting each
    // other's level features. Calls on one stream need nothing (stream order).
    hipEvent_t feat_done = nullptr;
    hipStream_t feat_stream = nullptr;
    bool feat_pending = false;
    void hash_feat_acquire(hipStream_t s) {
        if (feat_pending && feat_stream != s) HIP_CHECK(hipStreamWaitEvent(s, feat_done, 0));
    }
    void hash_feat_release(hipStream_t s) {
        if (!feat_done) HIP_CHECK(hipEventCreateWithFlags(&feat_done, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(feat_done, s));
        feat_stream = s;
        feat_pending = true;
    }
    HashScatter scatter{};  // Hash training: per-sample positions and grid-feature gradients (grid_scatter_kernel)
    int scatter_blocks = 0;
    int64_t* scatter_part = nullptr;  // per-slice partial sums of the fused step's fine levels (ScatterPartials)
    size_t scatter_part_bytes = 0;
    // the partial layout of a fused b-sample step (knob scatter_part: first level with partials), buffer grown to fit:
    // the int64 form, the int32 form (same element count) and the per-block form flags, in one allocation
    ScatterPartials step_partials(uint32_t b) {
        const int k = knob(kKnobScatterPart);
        ScatterPartials p = scatter_partials_layout(b, k >= 0 ? k : kScatterPartFirst);
        const size_t bytes = (size_t)p.total * (sizeof(int64_t) + sizeof(int32_t)) + sizeof(uint32_t) * (size_t)p.nflags;
        if (bytes > scatter_part_bytes) {
            if (scatter_part) HIP_CHECK(hipFree(scatter_part));
            scatter_part = nullptr;
            scatter_part_bytes = 0;
            HIP_CHECK(hipMalloc(&scatter_part, bytes));
            scatter_part_bytes = bytes;
        }
        if (p.total) {
            p.base = scatter_part;
            p.base32 = reinterpret_cast<int32_t*>(scatter_part + p.total);
            p.flags = reinterpret_cast<uint32_t*>(p.base32 + p.total);
        }
        return p;
    }
    uint8_t* grid_nf = nullptr;       // [n_grid] non-finite contribution codes (GridNonFinite)
    uint32_t* grid_nf_tag = nullptr;  // tag of the last scatter that recorded one
    uint32_t nf_seq = 0;              // tag of the current step's scatter
    GridNonFinite nonfinite() const { return GridNonFinite{grid_nf, grid_nf_tag, nf_seq}; }
    // the scatter workspace for a new training step (a fresh non-finite tag)
    const HashScatter* step_scatter(int blocks, const ScatterPartials& part) {
        ensure_scatter(blocks);
        nf_seq = nf_seq + 1u ? nf_seq + 1u : 1u;
        scatter.nf = nonfinite();
        scatter.part = part;
        return &scatter;
    }

    // width-128 network (BASELINE configs[4]): inference images (f16, FP8 + row scales), training images (f16
    // forward / backward from the master weights) and the training workspace
    uint8_t *wide_img16 = nullptr, *wide_img8 = nullptr;
    uint32_t* wide_scales = nullptr;
    _Float16 *wide_fwd_train = nullptr, *wide_bwd_train = nullptr;
    _Float16 *wide_ws_in = nullptr, *wide_ws_d = nullptr;
    float *wide_slabs = nullptr, *wide_loss_partials = nullptr;
    int64_t wide_ws_bpad = 0;

    // width-64 FP8 inference (nrc_infer8.hip): FP8 fragments of W1..W5 + row scale words, repacked from the inference
    // weights after every launch that rewrites them; allocated only when the handle is configured with FP8
    uint8_t* img8 = nullptr;
    bool fp8_64() const { return cfg.width == NRC_WIDTH && cfg.infer_precision == NRC_PRECISION_FP8; }

    bool hash() const { return encoding == NRC_ENCODING_HASH; }
    bool wide() const { return cfg.width == NRC_WIDE_WIDTH; }
    bool padq() const { return cfg.query_layout == NRC_QUERY_PADDED; }
    size_t n_total() const { return (size_t)n_mlp + (size_t)n_grid; }
    size_t grad_floats() const { return n_total() + 4; }

    void release() {
        peer_close();
        auto f = [](void* p) {
            if (p) (void)hipFree(p);
        };
        f(params); f(m); f(v); f(ema); f(infer);
        f(wf_train); f(wb_train); f(wf_infer); f(wf_infer16);
        f(fwd_pos); f(bwd_pos); f(fwdt_pos); f(slab_param);
        f(slabs); f(loss_partials);  // loss_dev aliases loss_host (freed below)
        f(work_queue);
        work_queue = nullptr;
        f(dp_grad);
        dp_grad = nullptr;
        f(frame_scratch);
        frame_scratch = nullptr;
        frame_scratch_bytes = 0;
        f(cull_ws);
        cull_ws = nullptr;
        cull_ws_pixels = 0;
        f(grid_grad); f(grid_steps); f(grid_bias); f(table_train); f(table_infer); f(hash_feat);
        hash_feat = nullptr;
        if (feat_done) (void)hipEventDestroy(feat_done);
        feat_done = nullptr;
        feat_stream = nullptr;
        feat_pending = false;
        f(grid_nf); f(grid_nf_tag);
        grid_nf = nullptr;
        grid_nf_tag = nullptr;
        f(scatter.pos); f(scatter.dy); f(scatter_part);
        scatter = HashScatter{};
        scatter_part = nullptr;
        scatter_part_bytes = 0;
        scatter_blocks = 0;
        f(img8);
        img8 = nullptr;
        f(wide_img16); f(wide_img8); f(wide_scales);
        f(wide_fwd_train); f(wide_bwd_train); f(wide_ws_in); f(wide_ws_d); f(wide_slabs); f(wide_loss_partials);
        wide_img16 = wide_img8 = nullptr;
        wide_scales = nullptr;
        wide_fwd_train = wide_bwd_train = wide_ws_in = wide_ws_d = nullptr;
        wide_slabs = wide_loss_partials = nullptr;
        wide_ws_bpad = 0;
        grid_grad = nullptr;
        grid_steps = nullptr;
        grid_bias = nullptr;
        table_train = table_infer = nullptr;
        if (loss_host) (void)hipHostFree(loss_host);
        f(fuse_sync);
        f(fuse_flags);
        fuse_sync = nullptr;
        fuse_flags = nullptr;
        fuse_gen = 0;
        fused = false;
        params = m = v = ema = infer = nullptr;
        wf_train = wb_train = wf_infer = wf_infer16 = nullptr;
        fwd_pos = bwd_pos = fwdt_pos = nullptr;
        t16 = false;
        slab_param = nullptr;
        slabs = loss_partials = loss_dev = loss_host = nullptr;
        slab_blocks = 0;
        initialized = false;
    }

    ModelBuffers buffers() const {
        ModelBuffers b;
        b.params = params; b.m = m; b.v = v; b.ema = ema; b.infer = infer;
        b.wf_train = wf_train; b.wb_train = wb_train; b.wf_infer = wf_infer; b.wf_infer16 = wf_infer16;
        b.fwd_pos = fwd_pos; b.bwd_pos = bwd_pos;
        b.fwdt_pos = fwdt_pos ? fwdt_pos : fwd_pos;
        b.slab_f16 = t16;
        b.n_mlp = n_mlp;
        b.n_total = (int)n_total();
        b.slab_param = slab_param;
        b.n_slab = n_slab;
        b.slab_closed = t16 ? (hash() ? 2 : 1) : 0;
        return b;
    }
    GridBuffers grid_buffers(const ScatterPartials& part = ScatterPartials{}) const {
        GridBuffers g;
        g.part = part;
        g.params = params + n_mlp; g.m = m + n_mlp; g.v = v + n_mlp; g.ema = ema + n_mlp; g.infer = infer + n_mlp;
        g.grad64 = grid_grad; g.grad32 = nullptr; g.fixed = nullptr; g.steps = grid_steps;
        g.nf = nonfinite();
        g.table_train = table_train; g.table_infer = table_infer;
        g.bias = grid_bias; g.bias_len = grid_bias ? kGridBiasLen : 0;
        g.n = n_grid;
        return g;
    }
    OptimArgs optim(uint32_t s) const {
        OptimArgs o;
        o.lr = cfg.learning_rate; o.beta1 = cfg.beta1; o.beta2 = cfg.beta2; o.eps = cfg.epsilon;
        o.l2_reg = cfg.l2_reg; o.ema_decay = cfg.ema_decay; o.loss_scale = cfg.loss_scale; o.step = s;
        return o;
    }
    void ensure_wide_ws(int64_t b) {
        const int64_t bpad = wide_bpad(b);
        if (bpad <= wide_ws_bpad) return;
        auto f = [](void* p) {
            if (p) HIP_CHECK(hipFree(p));
        };
        f(wide_ws_in); f(wide_ws_d); f(wide_slabs); f(wide_loss_partials);
        wide_ws_in = wide_ws_d = nullptr;
        wide_slabs = wide_loss_partials = nullptr;
        wide_ws_bpad = 0;
        // rows of wide_ld(bpad) >= bpad samples (the row stride; see wide_ld)
        HIP_CHECK(hipMalloc(&wide_ws_in, sizeof(_Float16) * kWideInRows * wide_ld(bpad)));
        HIP_CHECK(hipMalloc(&wide_ws_d, sizeof(_Float16) * kWideDRows * wide_ld(bpad)));
        HIP_CHECK(hipMalloc(&wide_slabs, sizeof(float) * NRC_WIDE_NUM_PARAMS * (size_t)wide_chunks(bpad)));
        HIP_CHECK(hipMalloc(&wide_loss_partials, sizeof(float) * (size_t)(bpad / 32)));
        wide_ws_bpad = bpad;
    }
    const HashScatter* ensure_scatter(int blocks) {
        if (blocks > scatter_blocks) {
            if (scatter.pos) HIP_CHECK(hipFree(scatter.pos));
            if (scatter.dy) HIP_CHECK(hipFree(scatter.dy));
            scatter = HashScatter{};
            scatter_blocks = 0;
            const int64_t bcap = (int64_t)blocks * kTrainSamplesPerBlock;
            HIP_CHECK(hipMalloc(&scatter.pos, sizeof(float4) * (size_t)bcap));
            HIP_CHECK(hipMalloc(&scatter.dy, sizeof(uint32_t) * NRC_HASH_LEVELS * (size_t)bcap));
            scatter.bcap = bcap;
            scatter_blocks = blocks;
        }
        return &scatter;
    }
    void ensure_slabs(int blocks) {
        if (blocks <= slab_blocks) return;
        if (slabs) HIP_CHECK(hipFree(slabs));
        if (loss_partials) HIP_CHECK(hipFree(loss_partials));
        slabs = nullptr;
        loss_partials = nullptr;
        slab_blocks = 0;
        HIP_CHECK(hipMalloc(&slabs, sizeof(float) * (size_t)blocks * n_slab));
        HIP_CHECK(hipMalloc(&loss_partials, sizeof(float) * (size_t)blocks));
        slab_blocks = blocks;
    }
};

void nrc_net::peer_close() {
    if (!px_group) {
        peer_close_own();
        return;
    }
    // a local group: no member may still have a step in flight that stores into a buffer about to be freed
    const std::shared_ptr<LocalPeerGroup> g = px_group;
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (nrc_net* n : g->members) {
        (void)hipSetDevice(n->device);
        (void)hipStreamSynchronize(n->stream);
    }
    for (nrc_net* n : g->members) n->peer_close_own();
    if (have_cur) (void)hipSetDevice(cur);
}

namespace {

void check_live(const nrc_net* net) {
    if (!net) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null handle");
    if (net->destroyed) throw ApiError(NRC_ERR_DESTROYED, "network was destroyed");
    if (!net->initialized) throw ApiError(NRC_ERR_NOT_INITIALIZED, "network is not initialised (call nrc_init)");
}

void upload_all(nrc_net* net, const std::vector<float>& params, const std::vector<float>& infer) {
    HIP_CHECK(hipMemcpy(net->params, params.data(), sizeof(float) * net->n_total(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(net->infer, infer.data(), sizeof(float) * net->n_total(), hipMemcpyHostToDevice));
}

WideImages wide_images(const nrc_net* net) {
    return WideImages{reinterpret_cast<_Float16*>(net->wide_img16), net->wide_img8, net->wide_scales, net->wide_fwd_train,
                      net->wide_bwd_train, net->encoding == NRC_ENCODING_FREQUENCY_SH ? 2 : 0};
}

// FP8-configured width-64 handles: the FP8 image follows the inference weights (after every launch on s that rewrote
// them); every other handle launches nothing
void pack_fp8_64(nrc_net* net, hipStream_t s) {
    if (net->fp8_64()) HIP_CHECK(launch_pack8(net->infer, net->img8, s));
}

void repack(nrc_net* net, hipStream_t s) {
    if (net->wide()) {
        HIP_CHECK(launch_wide_pack(net->infer, net->params, wide_images(net), s));
        return;
    }
    HIP_CHECK(launch_reduce_adam(kPackOnly, nullptr, 0, nullptr, nullptr, nullptr, net->buffers(), net->optim(1), s));
    pack_fp8_64(net, s);
    if (net->hash()) HIP_CHECK(launch_grid_adam(kPackOnly, net->grid_buffers(), net->optim(1), s));
}

// width-128 fwd/bwd + dW partials of b samples normalised by n_total (nrc_kernels.hip wide_fwd_bwd_kernel)
void wide_grad_partials(nrc_net* net, const float* in, const float* tgt, uint32_t b, float n_total) {
    net->ensure_wide_ws(b);
    HIP_CHECK(launch_wide_train_fwd_bwd(net->encoding == NRC_ENCODING_FREQUENCY_SH ? 2 : 0, in, tgt, b, n_total,
                                        net->cfg.loss_scale, net->wide_fwd_train, net->wide_bwd_train, net->wide_ws_in,
                                        net->wide_ws_d, net->wide_slabs, net->wide_loss_partials, net->stream));
}

int t16_groups() { return knob(kKnobT16Groups) == 1 ? 1 : 2; }
// Hash: 64-sample blocks by default (every CU at 16,384 samples; the doubled MLP slabs are reduced inside the merged
// optimizer launch, beside the grid Adam): step 48.6 vs 50.0 us (profiles/r05_hash/ab_hash_t16_groups.json); knob
// t16_groups = 2 keeps 128-sample blocks
int hash_t16_groups() { return knob(kKnobT16Groups) == 2 ? 2 : 1; }
// the Hash training kernel's feature source: the handle's feature workspace (batches of any size, in chunks of
// kHashFeatStride samples), or -- knob hash_infer = 1, compact records only -- the gathering encoder, which exists in the
// 128-sample block shape only (that knob used to fail under the 64-sample default)
bool hash_train_gathers(const nrc_net* net) { return knob(kKnobHashInfer) == 1 && !net->padq(); }
int hash_train_groups(const nrc_net* net) { return hash_train_gathers(net) ? 2 : hash_t16_groups(); }

// dc shape of a b-sample step (train_shape knob, else by batch size)
int dc_shape(uint32_t b) {
    const int k = knob(kKnobTrainShape);
    return k >= 0 ? k : dc_auto_shape(b);
}

// training blocks = weight-gradient slabs of a b-sample step of this handle's training kernel
int train_block_count(const nrc_net* net, uint32_t b) {
    if (net->t16 && net->hash()) {  // the role-split kernel, 64 x hash_train_groups() samples per block
        const uint32_t S = 64u * (uint32_t)hash_train_groups(net);
        return (int)((b + S - 1) / S);
    }
    if (net->t16 && net->t16_kernel == 0 && dc_shape(b) >= 0) {
        const int S = dc_samples_per_block(dc_shape(b));
        if (S <= 0) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "train_shape knob names no decoupled-chain shape");
        return (int)((b + (uint32_t)S - 1) / (uint32_t)S);
    }
    if (net->t16 && net->t16_kernel != 2) {
        const uint32_t S = 64u * (uint32_t)t16_groups();
        return (int)((b + S - 1) / S);
    }
    return train_blocks(b);
}

// round 6: a b-sample step of this handle runs as one launch (launch_train16_fused) when it would run on the role-split
// kernel with 128-sample blocks (not the decoupled-chain shapes of small batches, no stamps)
// Not while the stream is being captured into a graph: the launch's generation is a host counter, and a graph would
// replay the same value (a reducer could then take a previous replay's flags for this one's); captured steps take the
// two launches.
bool fused_step(const nrc_net* net, uint32_t b) {
    if (!net->fused || (net->t16_kernel == 0 && dc_shape(b) >= 0) || t16_groups() != 2) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(net->stream, &cs) != hipSuccess) return false;
    return cs == hipStreamCaptureStatusNone;
}
int fuse_mode() { const int k = knob(kKnobFuseMode); return k < 0 ? 0 : k; }
constexpr int kFuseMaxFlags = 1024;  // trainer blocks of one fused launch (CU-bound anyway)
constexpr int kFusePolls = 1 << 21;  // the reducers' bounded wait (~2 s: a trainer step takes ~10 us)
int device_cus(const nrc_net* net) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, net->device) != hipSuccess || v <= 0) v = 256;
    return v;
}

// 64-wide Frequency / FrequencySH fwd + loss + bwd + per-block dW slabs (n_total = 3 x global batch)
void train_partials(nrc_net* net, const float* in, const float* tgt, uint32_t b, float n_total,
                    uint64_t* stamps = nullptr) {
    net->check_protocol();  // an earlier step's kernel (completed by now or not) may have reported a timeout
    if (net->padq() && (!net->t16 || net->t16_kernel == 2 || stamps))
        throw ApiError(NRC_ERR_UNSUPPORTED, "padded queries: the production training kernels only (knobs at default, no stamps)");
    if (net->t16 && net->t16_kernel == 0 && dc_shape(b) >= 0)
        HIP_CHECK(launch_train_dc(dc_shape(b), in, tgt, b, n_total, net->cfg.loss_scale, net->wf_train, net->wb_train,
                                  reinterpret_cast<_Float16*>(net->slabs), net->loss_partials, net->proto_err_dev(),
                                  net->stream, stamps, net->padq()));
    else if (net->t16)
        HIP_CHECK(launch_train16(in, tgt, b, n_total, net->cfg.loss_scale, net->wf_train, net->wb_train,
                                 reinterpret_cast<_Float16*>(net->slabs), net->loss_partials, stamps, net->stream,
                                 net->t16_kernel != 2, t16_groups(), net->padq()));
    else if (stamps)
        HIP_CHECK(launch_train_stamped(in, tgt, b, n_total, net->cfg.loss_scale, net->wf_train, net->wb_train,
                                       net->slabs, net->loss_partials, stamps, net->stream));
    else
        HIP_CHECK(launch_train_fwd_bwd(in, tgt, b, n_total, net->cfg.loss_scale, net->wf_train, net->wb_train,
                                       net->slabs, net->loss_partials, net->stream, net->encoding));
}

// Hash fwd + loss + bwd + dW slabs + grid scatter of b samples (n_total = 3 x global batch). The t16 kernel reads the
// batch's level features from the handle's feature workspace (shared with inference: the event protocol of
// hash_feat_acquire / _release orders them across streams); knob hash_infer = 1 keeps the gathering encoder (A/B).
// part: the fused step's partial sums (do_train; the next grid_adam_kernel consumes them), else none (grad64 only).
void train_hash(nrc_net* net, const float* in, const float* tgt, uint32_t b, float n_total, int blocks,
                const ScatterPartials& part = ScatterPartials{}) {
    uint32_t* const feat = net->t16 && !hash_train_gathers(net) ? net->hash_feat : nullptr;
    if (feat) net->hash_feat_acquire(net->stream);
    HIP_CHECK(launch_train_hash(in, tgt, b, n_total, net->cfg.loss_scale, net->wf_train, net->wb_train, net->table_train,
                                net->grid_grad, net->slabs, net->loss_partials, net->stream,
                                net->step_scatter(blocks, part), net->padq(), net->t16, feat, hash_train_groups(net)));
    if (feat) net->hash_feat_release(net->stream);
}

void do_train(nrc_net* net, const float* in, const float* tgt, uint32_t b, float* loss_h, float* loss_d = nullptr) {
    check_live(net);
    if (b == 0) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "batch size must be >= 1");
    if (!in || !tgt) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null input/target pointer");
    if (net->wide()) {
        wide_grad_partials(net, in, tgt, b, 3.0f * (float)b);
        net->step += 1;
        HIP_CHECK(launch_wide_adam(kReduceFused, net->wide_slabs, wide_chunks(b), net->wide_loss_partials,
                                   (int)(wide_bpad(b) / 32), nullptr, loss_d ? loss_d : net->loss_dev, net->buffers(),
                                   net->optim(net->step), wide_images(net), net->stream));
        if (loss_h) {
            *loss_h = net->read_loss();
        }
        return;
    }
    const int blocks = train_block_count(net, b);
    net->ensure_slabs(blocks);
    if (net->hash()) {
        // training kernel + grid scatter, then the MLP and grid optimizer updates (a second stream for the MLP update, beside
        // the scatter, measured slower: each cross-stream event added ~6 us of idle GPU; one launch holding both updates
        // as noinline halves ran 75 us)
        // the fine levels' scatter stores per-slice partials that the grid update sums (no memory-side atomics)
        // (the grid Adam inside the scatter launch, its group's last block applying it, measured slower: 69.7 vs 56.2 us)
        const ScatterPartials part = net->step_partials(b);
        train_hash(net, in, tgt, b, 3.0f * (float)b, blocks, part);
        net->step += 1;
        if (net->t16 && knob(kKnobHashAdam) != 0) {  // both updates in one launch (hash_adam_kernel)
            HIP_CHECK(launch_hash_adam(net->slabs, blocks, net->loss_partials, loss_d ? loss_d : net->loss_dev,
                                       net->buffers(), net->grid_buffers(part), net->optim(net->step), net->stream));
            if (loss_h) *loss_h = net->read_loss();
            return;
        }
        HIP_CHECK(launch_reduce_adam(kReduceFused, net->slabs, blocks, net->loss_partials, nullptr,
                                     loss_d ? loss_d : net->loss_dev, net->buffers(), net->optim(net->step), net->stream));
        HIP_CHECK(launch_grid_adam(kReduceFused, net->grid_buffers(part), net->optim(net->step), net->stream));
        if (loss_h) *loss_h = net->read_loss();
        return;
    }
    if (fused_step(net, b)) {
        net->check_protocol();
        const hipError_t e = launch_train16_fused(in, tgt, b, 3.0f * (float)b, net->cfg.loss_scale, net->wf_train,
                                                  net->wb_train, reinterpret_cast<_Float16*>(net->slabs),
                                                  net->loss_partials, net->fuse_sync, net->proto_err_dev(), kFusePolls,
                                                  loss_d ? loss_d : net->loss_dev, net->buffers(),
                                                  net->optim(net->step + 1), net->stream, net->padq(), device_cus(net),
                                                  fuse_mode(), net->next_fuse_gen(), net->fuse_flags, kFuseMaxFlags);
        if (e != hipErrorNotSupported) {
            HIP_CHECK(e);
            net->step += 1;
            pack_fp8_64(net, net->stream);
            if (loss_h) *loss_h = net->read_loss();
            return;
        }
    }
    train_partials(net, in, tgt, b, 3.0f * (float)b);
    net->step += 1;
    HIP_CHECK(launch_reduce_adam(kReduceFused, net->slabs, blocks, net->loss_partials, nullptr,
                                 loss_d ? loss_d : net->loss_dev, net->buffers(), net->optim(net->step), net->stream));
    pack_fp8_64(net, net->stream);
    if (loss_h) {
        *loss_h = net->read_loss();
    }
}

// why nrc_train_gather cannot serve a b-sample step of the handle (names the combination), or null. The gather forms
// exist for the two production Frequency kernels; a knob that selects another kernel or block shape is refused too.
const char* train_gather_unsupported(const nrc_net* net, uint32_t b) {
    if (net->wide()) return "gathered training step: width 128 is not supported (width 64 only)";
    if (net->hash()) return "gathered training step: InputEncoding::Hash is not supported (Frequency only)";
    if (net->encoding == NRC_ENCODING_FREQUENCY_SH)
        return "gathered training step: InputEncoding::FrequencySH is not supported (Frequency only)";
    const bool dc = net->t16 && net->t16_kernel == 0 && dc_shape(b) >= 0;
    if (!net->t16 || net->t16_kernel == 2 || (dc ? dc_shape(b) != 7 : t16_groups() != 2))
        return "gathered training step: the production training kernels only (knobs train_kernel, train_shape, "
               "t16_groups at default)";
    return nullptr;
}

// nrc_train_gather: do_train's two-launch Frequency step with the gather form of its training kernel. The reduce /
// Adam launch sees the same per-block slabs and loss partials in the same order, so the step is bitwise do_train's on
// the permuted rows (a handle that fuses the step into one launch, knob train_fused, is bitwise the two launches too).
void do_train_gather(nrc_net* net, const float* qs, const float* ts, const GatherSrc& gs, uint32_t b, float* loss_d) {
    const int blocks = train_block_count(net, b);
    net->ensure_slabs(blocks);
    net->check_protocol();
    const float n_total = 3.0f * (float)b;
    _Float16* const slabs = reinterpret_cast<_Float16*>(net->slabs);
    if (net->t16_kernel == 0 && dc_shape(b) >= 0)
        HIP_CHECK(launch_train_dc_gather(dc_shape(b), qs, ts, gs, b, n_total, net->cfg.loss_scale, net->wf_train,
                                         net->wb_train, slabs, net->loss_partials, net->proto_err_dev(), net->stream,
                                         net->padq()));
    else
        HIP_CHECK(launch_train16_gather(qs, ts, gs, b, n_total, net->cfg.loss_scale, net->wf_train, net->wb_train, slabs,
                                        net->loss_partials, net->stream, net->padq()));
    net->step += 1;
    HIP_CHECK(launch_reduce_adam(kReduceFused, net->slabs, blocks, net->loss_partials, nullptr,
                                 loss_d ? loss_d : net->loss_dev, net->buffers(), net->optim(net->step), net->stream));
    pack_fp8_64(net, net->stream);
}

int wide_enc(const nrc_net* net) { return net->encoding == NRC_ENCODING_FREQUENCY_SH ? 2 : 0; }

hipError_t infer_wide(nrc_net* net, int prec, const float* in, float* out, uint32_t n, const float* thr, float* rgba,
                      uint32_t n_acc, int mode, float w, hipStream_t s) {
    return launch_infer_wide(prec, wide_enc(net), in, out, n, (prec & 15) ? net->wide_img8 : net->wide_img16, net->wide_scales,
                             thr, rgba, n_acc, mode, w, s);
}

hipError_t infer_any(nrc_net* net, const float* in, float* out, uint32_t n) {
    if (net->wide())
        return infer_wide(net, (int)net->cfg.infer_precision, in, out, n, nullptr, nullptr, 0, -1, 1.0f, net->stream);
    if (net->hash()) {
        uint32_t* const feat = net->hash_feat_arg();
        if (feat) net->hash_feat_acquire(net->stream);
        if (net->padq() && !feat) throw ApiError(NRC_ERR_UNSUPPORTED, "padded queries: the feature-pass Hash inference only");
        if (net->cfg.infer_precision == NRC_PRECISION_F16_ACC16) {
            if (!net->hash_feat) throw ApiError(NRC_ERR_INTERNAL, "Hash feature workspace missing");
            net->hash_feat_acquire(net->stream);
            const hipError_t e = launch_infer_hash_tcnn(in, out, n, net->wf_infer, net->infer, net->table_infer,
                                                        net->hash_feat, net->stream);
            if (e == hipSuccess) net->hash_feat_release(net->stream);
            return e;
        }
        const hipError_t e = launch_infer_hash(in, out, n, net->wf_infer, net->table_infer, nullptr, nullptr, 0, -1, 1.0f,
                                               net->stream, feat, net->padq());
        if (e == hipSuccess && feat) net->hash_feat_release(net->stream);
        return e;
    }
    if (net->encoding == NRC_ENCODING_FREQUENCY_SH)
        return launch_infer_sh(in, out, n, net->wf_infer, nullptr, nullptr, 0, -1, 1.0f, net->stream);
    if (net->cfg.infer_precision == NRC_PRECISION_F16_ACC16)
        return launch_infer_tcnn(in, out, n, net->wf_infer, net->infer, net->stream);
    if (net->fp8_64())
        return launch_infer8(0, in, out, n, net->wf_infer, net->img8, nullptr, nullptr, 0, -1, 1.0f, net->stream);
    return launch_infer(in, out, n, net->wf_infer, net->stream, net->work_queue, &net->pool_parity, net->padq());
}

void require_frequency(const nrc_net* net, const char* what) {
    if (net->encoding != NRC_ENCODING_FREQUENCY)
        throw ApiError(NRC_ERR_UNSUPPORTED, std::string(what) + " is implemented for InputEncoding::Frequency only");
}

// Padded RadianceQuery layout (nrc_config.query_layout = NRC_QUERY_PADDED): the handle computes in the compact
// encoding's column order with the first constant-one column (Frequency 66, Hash 62) carrying pad_; the API blob
// follows the reference's padded encoding (layout.h), where pad_'s Identity column sits right after the position
// encoding (Frequency 36, Hash 32) and the columns up to the first one-column shift by one. to_api: internal -> API
// order of W0's columns in place (else API -> internal); the other layers and the grid are the same in both.
int padq_api_column(int encoding, int c) {
    const int R = encoding == NRC_ENCODING_HASH ? 32 : 36;  // real columns before pad_
    const int E = encoding == NRC_ENCODING_HASH ? 62 : 66;  // internal column carrying pad_
    return c < R ? c : c < E ? c + 1 : c == E ? R : c;
}
void padq_w0_columns(int encoding, float* blob, bool to_api) {
    const int in = encoding == NRC_ENCODING_HASH ? NRC_HASH_ENC_WIDTH : NRC_ENC_WIDTH;
    std::vector<float> row(in);
    for (int o = 0; o < NRC_WIDTH; ++o) {
        float* w = blob + (size_t)o * in;
        for (int c = 0; c < in; ++c) {
            const int a = padq_api_column(encoding, c);
            if (to_api) row[a] = w[c];
            else row[c] = w[a];
        }
        std::copy(row.begin(), row.end(), w);
    }
}

float* slot_ptr(nrc_net* net, int slot) {
    switch (slot) {
        case NRC_STATE_PARAMS: return net->params;
        case NRC_STATE_INFER: return net->infer;
        case NRC_STATE_EMA: return net->ema;
        case NRC_STATE_ADAM_M: return net->m;
        case NRC_STATE_ADAM_V: return net->v;
        default: throw ApiError(NRC_ERR_INVALID_ARGUMENT, "unknown state slot " + std::to_string(slot));
    }
}

}  // namespace

namespace {
void do_train_dp(nrc_net* net, const float* in, const float* tgt, uint32_t b_local, uint32_t global_b, float* loss_h,
                 float* loss_d);
}  // namespace

void nrc_amd::net_train_dp_async(nrc_net* net, const float* in, const float* tgt, uint32_t b_local, uint32_t global_b,
                                 float* loss_d) {
    do_train_dp(net, in, tgt, b_local, global_b, nullptr, loss_d);
}

bool nrc_amd::net_comm(nrc_net* net, int* rank, int* world) {
    check_live(net);
    if (net->px_open) {  // the peer exchange takes precedence (nrc_train_dp uses it when open)
        *rank = net->px_rank;
        *world = net->px_world;
        return true;
    }
    *rank = net->comm_rank;
    *world = net->comm_world;
    return net->comm != nullptr;
}

void* nrc_amd::net_frame_scratch(nrc_net* net, size_t bytes) {
    check_live(net);
    if (bytes > net->frame_scratch_bytes) {
        if (net->frame_scratch) {
            HIP_CHECK(hipStreamSynchronize(net->stream));  // a queued kernel may still use the old buffer
            HIP_CHECK(hipFree(net->frame_scratch));
        }
        net->frame_scratch = nullptr;
        net->frame_scratch_bytes = 0;
        HIP_CHECK(hipMalloc(&net->frame_scratch, bytes));
        net->frame_scratch_bytes = bytes;
    }
    return net->frame_scratch;
}

bool nrc_amd::net_infer_fusable(nrc_net* net) {
    check_live(net);
    return net->cfg.infer_precision != NRC_PRECISION_F16_ACC16;
}

// why nrc_infer_accumulate_sparse cannot serve the handle (names the combination), or null
static const char* sparse_unsupported(nrc_net* net) {
    if (net->wide()) return "sparse fused accumulation: width 128 is not supported (width 64 only)";
    if (net->hash()) return "sparse fused accumulation: InputEncoding::Hash is not supported (Frequency only)";
    if (net->encoding == NRC_ENCODING_FREQUENCY_SH)
        return "sparse fused accumulation: InputEncoding::FrequencySH is not supported (Frequency only)";
    if (net->cfg.infer_precision == NRC_PRECISION_F16_ACC16)
        return "sparse fused accumulation: NRC_PRECISION_F16_ACC16 is not supported (F16 only)";
    if (net->fp8_64()) return "sparse fused accumulation: FP8 at width 64 is not supported (F16 only)";
    if (net->padq()) return "sparse fused accumulation: padded queries are not supported (compact only)";
    return nullptr;
}

bool nrc_amd::net_infer_sparse_ok(nrc_net* net) {
    check_live(net);
    return sparse_unsupported(net) == nullptr;
}

// why nrc_infer_accumulate_factored cannot serve the handle (names the combination), or null
static const char* factored_unsupported(nrc_net* net) {
    if (net->wide()) return "fused factored accumulation: width 128 is not supported (width 64 only)";
    if (net->hash()) return "fused factored accumulation: InputEncoding::Hash is not supported (Frequency only)";
    if (net->encoding == NRC_ENCODING_FREQUENCY_SH)
        return "fused factored accumulation: InputEncoding::FrequencySH is not supported (Frequency only)";
    if (net->cfg.infer_precision == NRC_PRECISION_F16_ACC16)
        return "fused factored accumulation: NRC_PRECISION_F16_ACC16 is not supported (F16 and FP8 only)";
    if (net->padq()) return "fused factored accumulation: padded queries are not supported (compact only)";
    return nullptr;
}

bool nrc_amd::net_infer_factored_ok(nrc_net* net) {
    check_live(net);
    return factored_unsupported(net) == nullptr;
}

// why nrc_infer_accumulate_culled cannot serve the handle (names the combination), or null
static const char* culled_unsupported(nrc_net* net) {
    if (net->wide()) return "culled fused accumulation: width 128 is not supported (width 64 only)";
    if (net->hash()) return "culled fused accumulation: InputEncoding::Hash is not supported (Frequency only)";
    if (net->encoding == NRC_ENCODING_FREQUENCY_SH)
        return "culled fused accumulation: InputEncoding::FrequencySH is not supported (Frequency only)";
    if (net->cfg.infer_precision == NRC_PRECISION_F16_ACC16)
        return "culled fused accumulation: NRC_PRECISION_F16_ACC16 is not supported (F16 and FP8 only)";
    if (net->padq()) return "culled fused accumulation: padded queries are not supported (compact only)";
    return nullptr;
}

bool nrc_amd::net_infer_culled_ok(nrc_net* net) {
    check_live(net);
    return culled_unsupported(net) == nullptr;
}

bool nrc_amd::net_train_gather_ok(nrc_net* net, uint32_t b) {
    check_live(net);
    return train_gather_unsupported(net, b) == nullptr;
}

void nrc_amd::net_check_protocol(nrc_net* net) {
    check_live(net);
    net->check_protocol();
}

bool nrc_amd::net_padq(nrc_net* net) {
    check_live(net);
    return net->padq();
}

nrc_loss_slots nrc_amd::net_loss_slots(nrc_net* net) {
    check_live(net);
    return {net->loss_dev, net->loss_host};
}

int nrc_amd::knob(Knob k) { return g_knobs[k].load(std::memory_order_relaxed); }

namespace {
// accepted values per knob (an out-of-range train_shape made train_block_count divide by zero); -1 = default
bool knob_value_ok(Knob k, int v) {
    switch (k) {
        case kKnobTrainKernel: return v == -1 || v == 0 || v == 1 || v == 2 || v == 32;
        case kKnobTrainShape: return v >= -1 && v <= 7;
        case kKnobScatterMin:
        case kKnobScatterMax: return v == -1 || (v >= 16 && v <= (1 << 20));
        case kKnobDcDw0Delay: return v >= -1 && v <= (1 << 20);
        case kKnobHashInfer: return v >= -1 && v <= 1;
        case kKnobHashFeatAbl: return v >= -1 && (v <= 36 || v == 128);
        case kKnobT16Groups: return v == -1 || v == 1 || v == 2;
        case kKnobHashFeatP: return v == -1 || (v >= 8 && v <= 256 && v % 8 == 0);
        case kKnobPeerPath: return v >= -1 && v <= 4;
        case kKnobPxPolls: return v == -1 || (v >= 1 && v <= kPeerPolls);
        case kKnobScatterPart:
        case kKnobScatterCompact: return v >= -1 && v <= NRC_HASH_LEVELS;
        case kKnobHashTrainFeat: return v >= -1 && v <= 1;
        case kKnobHashAdam: return v >= -1 && v <= 0;
        case kKnobTrainFused: return v >= -1 && v <= 1;
        case kKnobFuseMode: return v >= -1 && v <= 4;
        case kKnobTcnnReentry: return v >= -1 && v <= 1;
        case kKnobTrainPrio: return v >= -1 && v <= 2;
        case kKnobFrameSparse: return v >= -1 && v <= 1;
        case kKnobFrameFactoredFused: return v >= -1 && v <= 1;
        case kKnobFrameTrainGather: return v >= -1 && v <= 1;
        case kKnobFrameCulled: return v >= -1 && v <= 1;
        default: return false;
    }
}

const char* const kDebugOnly =
    "diagnostic kernel of the debug library: load libnrc_amd_debug.so (NRC_LIB_PATH) for stamps, clocks and A/B variants";
}

extern "C" {

nrc_status nrc_debug_set_knob(const char* name, int value) {
    return guarded([&] {
        if (!name) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null knob name");
        for (int k = 0; k < kKnobCount; ++k)
            if (std::strcmp(name, kKnobNames[k]) == 0) {
                if (!knob_value_ok(static_cast<Knob>(k), value))
                    throw ApiError(NRC_ERR_INVALID_ARGUMENT,
                                   std::string("knob ") + name + ": value " + std::to_string(value) + " out of range");
                g_knobs[k].store(value, std::memory_order_relaxed);
                return;
            }
        throw ApiError(NRC_ERR_INVALID_ARGUMENT, std::string("unknown knob ") + name);
    });
}

nrc_status nrc_debug_get_knob(const char* name, int* value) {
    return guarded([&] {
        if (!name || !value) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null argument");
        for (int k = 0; k < kKnobCount; ++k)
            if (std::strcmp(name, kKnobNames[k]) == 0) {
                *value = g_knobs[k].load(std::memory_order_relaxed);
                return;
            }
        throw ApiError(NRC_ERR_INVALID_ARGUMENT, std::string("unknown knob ") + name);
    });
}

const char* nrc_version(void) { return "nrc-mi355x 0.1 (gfx950)"; }
const char* nrc_last_error(void) { return g_last_error.c_str(); }

nrc_config nrc_default_config(int encoding) {
    nrc_config c;
    c.learning_rate = encoding == NRC_ENCODING_HASH ? NRC_TRAIN_LR_HASH : NRC_TRAIN_LR_FREQUENCY;
    c.beta1 = NRC_ADAM_BETA1;
    c.beta2 = NRC_ADAM_BETA2;
    c.epsilon = encoding == NRC_ENCODING_HASH ? NRC_ADAM_EPS_HASH : NRC_ADAM_EPS_FREQ;
    c.l2_reg = NRC_ADAM_L2_REG;
    c.ema_decay = NRC_EMA_DECAY;
    c.loss_scale = NRC_LOSS_SCALE;
    c.seed = 1337;
    c.width = NRC_WIDTH;
    c.infer_precision = NRC_PRECISION_F16;
    c.query_layout = NRC_QUERY_COMPACT;
    return c;
}

nrc_status nrc_create(nrc_net** out) {
    return guarded([&] {
        if (!out) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null output pointer");
        *out = new nrc_net();
        (*out)->cfg = nrc_default_config(NRC_ENCODING_FREQUENCY);
    });
}

nrc_status nrc_free(nrc_net* net) {
    return guarded([&] {
        if (!net) return;
        if (!net->destroyed && net->initialized)
            std::fprintf(stderr, "WARNING: NRC Network must be explicitly destroy() in the context it was created in!\n");
        net->release();
        delete net;
    });
}

nrc_status nrc_init(nrc_net* net, hipStream_t stream, int encoding, const nrc_config* cfg, int verbose) {
    return guarded([&] {
        if (!net) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null handle");
        if (encoding != NRC_ENCODING_FREQUENCY && encoding != NRC_ENCODING_HASH && encoding != NRC_ENCODING_FREQUENCY_SH)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "Unsupported input encoding");
        const nrc_config c = cfg ? *cfg : nrc_default_config(encoding);
        if (c.width != NRC_WIDTH && c.width != NRC_WIDE_WIDTH)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "width must be 64 or 128");
        if (c.infer_precision != NRC_PRECISION_F16 && c.infer_precision != NRC_PRECISION_FP8 &&
            c.infer_precision != NRC_PRECISION_F16_ACC16)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "unknown infer_precision");
        if (c.infer_precision == NRC_PRECISION_F16_ACC16 &&
            (c.width != NRC_WIDTH || encoding == NRC_ENCODING_FREQUENCY_SH))
            throw ApiError(NRC_ERR_UNSUPPORTED,
                           "F16_ACC16 (tcnn numerics) is implemented for the width-64 Frequency and Hash networks");
        if (c.infer_precision == NRC_PRECISION_FP8 && c.width == NRC_WIDTH &&
            (encoding != NRC_ENCODING_FREQUENCY || c.query_layout == NRC_QUERY_PADDED))
            throw ApiError(NRC_ERR_UNSUPPORTED,
                           std::string("FP8 inference at width 64 is implemented for InputEncoding::Frequency with compact "
                                       "queries; requested: ") +
                               (encoding == NRC_ENCODING_HASH ? "Hash" : encoding == NRC_ENCODING_FREQUENCY_SH ? "FrequencySH" : "Frequency") +
                               (c.query_layout == NRC_QUERY_PADDED ? " with NRC_QUERY_PADDED" : ""));
        if (c.width == NRC_WIDE_WIDTH && encoding == NRC_ENCODING_HASH)
            throw ApiError(NRC_ERR_UNSUPPORTED, "the width-128 network supports the Frequency / FrequencySH encodings");
        if (c.query_layout != NRC_QUERY_COMPACT && c.query_layout != NRC_QUERY_PADDED)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "unknown query_layout");
        if (c.query_layout == NRC_QUERY_PADDED &&
            (c.width != NRC_WIDTH || encoding == NRC_ENCODING_FREQUENCY_SH || c.infer_precision != NRC_PRECISION_F16))
            throw ApiError(NRC_ERR_UNSUPPORTED, "padded RadianceQuery records (USE_COMPACT_RADIANCE_QUERY 0): the width-64 "
                                                "Frequency / Hash networks with F16 inference");
        net->release();
        net->stream = stream;
        net->encoding = encoding;
        net->config_encoding = encoding;
        net->cfg = c;
        net->destroyed = false;
        net->step = 0;
        HIP_CHECK(hipGetDevice(&net->device));
        if (net->wide()) {
            net->n_mlp = NRC_WIDE_NUM_PARAMS;
            net->n_grid = 0;
            const size_t pb = sizeof(float) * net->n_total();
            HIP_CHECK(hipMalloc(&net->params, pb));
            HIP_CHECK(hipMalloc(&net->m, pb));
            HIP_CHECK(hipMalloc(&net->v, pb));
            HIP_CHECK(hipMalloc(&net->ema, pb));
            HIP_CHECK(hipMalloc(&net->infer, pb));
            HIP_CHECK(hipMemset(net->m, 0, pb));
            HIP_CHECK(hipMemset(net->v, 0, pb));
            HIP_CHECK(hipMemset(net->ema, 0, pb));
            HIP_CHECK(hipMalloc(&net->wide_img16, kWideF16Bytes));
            HIP_CHECK(hipMalloc(&net->wide_img8, kWide8Bytes));
            HIP_CHECK(hipMalloc(&net->wide_scales, sizeof(uint32_t) * 5 * 32));
            HIP_CHECK(hipMalloc(&net->wide_fwd_train, kWideF16Bytes));
            HIP_CHECK(hipMalloc(&net->wide_bwd_train, kWideBwdBytes));
            net->alloc_loss_slots();
            std::vector<float> p(net->n_total());
            init_params_wide(p, net->cfg.seed);
            upload_all(net, p, p);
            net->initialized = true;
            repack(net, nullptr);
            HIP_CHECK(hipDeviceSynchronize());
            net->ensure_wide_ws(NRC_BATCH_SIZE);
            if (verbose)
                std::printf("\n----------------------- NETWORK CONFIG -----------------------\n%s\n"
                            "--------------------------------------------------------------\n\n",
                            config_json(net->encoding, net->cfg).c_str());
            return;
        }
        net->n_mlp = net->hash() ? NRC_HASH_MLP_PARAMS : NRC_NUM_PARAMS;
        net->n_grid = net->hash() ? NRC_HASH_GRID_PARAMS : 0;
        const size_t pb = sizeof(float) * net->n_total();
        HIP_CHECK(hipMalloc(&net->params, pb));
        HIP_CHECK(hipMalloc(&net->m, pb));
        HIP_CHECK(hipMalloc(&net->v, pb));
        HIP_CHECK(hipMalloc(&net->ema, pb));
        HIP_CHECK(hipMalloc(&net->infer, pb));
        HIP_CHECK(hipMalloc(&net->wf_train, sizeof(_Float16) * kFwdHalves));
        HIP_CHECK(hipMalloc(&net->wb_train, sizeof(_Float16) * kWbHalves));
        HIP_CHECK(hipMalloc(&net->wf_infer, sizeof(_Float16) * kFwdHalves));
        HIP_CHECK(hipMalloc(&net->fwd_pos, sizeof(int) * net->n_mlp));
        HIP_CHECK(hipMalloc(&net->bwd_pos, sizeof(int) * net->n_mlp));
        if (net->hash()) {
            const size_t ng = (size_t)net->n_grid;
            HIP_CHECK(hipMalloc(&net->grid_grad, sizeof(int64_t) * ng));
            HIP_CHECK(hipMalloc(&net->grid_steps, sizeof(uint32_t) * ng));
            HIP_CHECK(hipMalloc(&net->table_train, sizeof(_Float16) * ng));
            HIP_CHECK(hipMalloc(&net->table_infer, sizeof(_Float16) * ng));
            HIP_CHECK(hipMalloc(&net->hash_feat, sizeof(uint32_t) * NRC_HASH_LEVELS * (size_t)kHashFeatStride));
            HIP_CHECK(hipMemset(net->grid_grad, 0, sizeof(int64_t) * ng));
            HIP_CHECK(hipMalloc(&net->grid_nf, ng));
            HIP_CHECK(hipMemset(net->grid_nf, 0, ng));
            HIP_CHECK(hipMalloc(&net->grid_nf_tag, sizeof(uint32_t)));
            HIP_CHECK(hipMemset(net->grid_nf_tag, 0, sizeof(uint32_t)));
            HIP_CHECK(hipMemset(net->grid_steps, 0, sizeof(uint32_t) * ng));
            std::vector<float2> bias(kGridBiasLen + 1, float2{0.0f, 0.0f});
            for (uint32_t st = 1; st <= kGridBiasLen; ++st)
                bias[st] = float2{sqrtf(1.0f - powf(net->cfg.beta2, (float)st)), 1.0f - powf(net->cfg.beta1, (float)st)};
            HIP_CHECK(hipMalloc(&net->grid_bias, sizeof(float2) * bias.size()));
            HIP_CHECK(hipMemcpy(net->grid_bias, bias.data(), sizeof(float2) * bias.size(), hipMemcpyHostToDevice));
        }
        net->alloc_loss_slots();
        HIP_CHECK(hipMemset(net->m, 0, pb));
        HIP_CHECK(hipMemset(net->v, 0, pb));
        HIP_CHECK(hipMemset(net->ema, 0, pb));
        HIP_CHECK(hipMemset(net->wf_train, 0, sizeof(_Float16) * kFwdHalves));
        HIP_CHECK(hipMemset(net->wb_train, 0, sizeof(_Float16) * kWbHalves));
        HIP_CHECK(hipMemset(net->wf_infer, 0, sizeof(_Float16) * kFwdHalves));
        if (net->fp8_64()) {
            HIP_CHECK(hipMalloc(&net->img8, kInfer8Bytes));
            HIP_CHECK(hipMemset(net->img8, 127, kInfer8Bytes));  // scale bytes the pack never writes: 2^0
        }
        std::vector<int> fwd, bwd;
        build_scatter_maps(fwd, bwd, net->encoding);
        net->t16 = want_t16(net->encoding);
        {
            // the decoupled-chain kernel is the default; knob train_kernel = 1 / 2 selects round 2's role-split /
            // 4-wave t16 kernels (in-process A/B)
            const int k = knob(kKnobTrainKernel);
            net->t16_kernel = (k == 1 || (k == 2 && NRC_DEBUG_KERNELS)) ? k : 0;
        }
        net->fused = net->t16 && net->encoding == NRC_ENCODING_FREQUENCY && net->t16_kernel != 2 &&
                     knob(kKnobTrainFused) == 1;
        if (net->fused) {
            HIP_CHECK(hipExtMallocWithFlags(reinterpret_cast<void**>(&net->fuse_sync), 512, hipDeviceMallocUncached));
            HIP_CHECK(hipMemset(net->fuse_sync, 0, 512));
            HIP_CHECK(hipMalloc(&net->fuse_flags, sizeof(uint32_t) * kFuseMaxFlags));
            HIP_CHECK(hipMemset(net->fuse_flags, 0, sizeof(uint32_t) * kFuseMaxFlags));
        }
        if (net->t16) {
            std::vector<int> fwdt;
            build_t16_maps(fwdt, bwd, net->encoding);
            HIP_CHECK(hipMalloc(&net->fwdt_pos, sizeof(int) * net->n_mlp));
            HIP_CHECK(hipMemcpy(net->fwdt_pos, fwdt.data(), sizeof(int) * net->n_mlp, hipMemcpyHostToDevice));
#if NRC_DEBUG_KERNELS
            // debug library only (variants 50/51, nrc_infer16.hip, rejected in round 2: DESIGN.md §8): the t16-layout
            // inference image, packed by the optimizer
            static_assert(kT16FwdFrags * kFragHalves == kFwdHalves, "t16 forward image size");
            HIP_CHECK(hipMalloc(&net->wf_infer16, sizeof(_Float16) * kFwdHalves));
            HIP_CHECK(hipMemset(net->wf_infer16, 0, sizeof(_Float16) * kFwdHalves));  // dummy slots stay 0
#endif
        }
        HIP_CHECK(hipMemcpy(net->fwd_pos, fwd.data(), sizeof(int) * net->n_mlp, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(net->bwd_pos, bwd.data(), sizeof(int) * net->n_mlp, hipMemcpyHostToDevice));
        {
            const std::vector<int> sm = net->t16 ? build_t16_slab_map(net->encoding) : build_slab_map(net->encoding);
            if (net->t16)  // the reduction maps t16 slab positions in closed form (t16_slab_param, t16_hash_slab_param)
                for (size_t i = 0; i < sm.size(); ++i)
                    if (sm[i] != (net->hash() ? t16_hash_slab_param((int)i) : t16_slab_param((int)i)))
                        throw ApiError(NRC_ERR_INTERNAL, "t16_slab_param disagrees with the slab map at " + std::to_string(i));
            net->n_slab = (int)sm.size();
            HIP_CHECK(hipMalloc(&net->slab_param, sizeof(int) * sm.size()));
            HIP_CHECK(hipMemcpy(net->slab_param, sm.data(), sizeof(int) * sm.size(), hipMemcpyHostToDevice));
        }
        std::vector<float> p(net->n_total());
        if (net->hash()) init_params_hash(p, net->cfg.seed);
        else init_params(p, net->cfg.seed);
        upload_all(net, p, p);  // before the first step inference uses the initial weights
        net->initialized = true;
        repack(net, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        net->ensure_slabs(train_block_count(net, NRC_BATCH_SIZE));
        if (verbose) {
            std::printf("\n----------------------- NETWORK CONFIG -----------------------\n%s\n"
                        "--------------------------------------------------------------\n\n",
                        config_json(net->encoding, net->cfg).c_str());
        }
    });
}

nrc_status nrc_destroy(nrc_net* net) {
    return guarded([&] {
        if (!net) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null handle");
        if (net->destroyed) return;
        net->release();
        net->destroyed = true;
    });
}

nrc_status nrc_train(nrc_net* net, const float* in, const float* tgt, float* loss_h) {
    return guarded([&] { do_train(net, in, tgt, NRC_BATCH_SIZE, loss_h); });
}

nrc_status nrc_train_stream(nrc_net* net, const float* in, const float* tgt, hipStream_t stream, float* loss_h) {
    return guarded([&] {
        check_live(net);
        net->stream = stream;
        do_train(net, in, tgt, NRC_BATCH_SIZE, loss_h);
    });
}

nrc_status nrc_train_batch(nrc_net* net, const float* in, const float* tgt, uint32_t b, float* loss_h) {
    return guarded([&] { do_train(net, in, tgt, b, loss_h); });
}

nrc_status nrc_train_async(nrc_net* net, const float* in, const float* tgt, uint32_t b, float* loss_d) {
    return guarded([&] {
        check_live(net);
        // loss_d == NULL: the loss still lands in the handle's own slot
        do_train(net, in, tgt, b, nullptr, loss_d);
    });
}

nrc_status nrc_train_gather(nrc_net* net, const float* qs, const nrc_float3* ts, const int32_t* perm, uint64_t seed,
                            uint32_t frame_index, int32_t num_records, uint32_t n_out, uint32_t first, uint32_t b,
                            float* loss_d) {
    return guarded([&] {
        check_live(net);
        if (num_records <= 0) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "num_records must be >= 1");
        if (n_out == 0 || n_out > (1u << 30)) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "n_out must be in 1..2^30");
        if (b == 0) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "batch size must be >= 1");
        if ((uint64_t)first + b > n_out) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "first + b must be <= n_out");
        if (const char* why = train_gather_unsupported(net, b)) throw ApiError(NRC_ERR_UNSUPPORTED, why);
        if (!qs || !ts) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null query/target pointer");
        if ((reinterpret_cast<uintptr_t>(qs) | reinterpret_cast<uintptr_t>(ts) | reinterpret_cast<uintptr_t>(perm)) & 3)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "buffers must be 4-byte aligned");
        const GatherSrc gs{perm, make_key(seed, frame_index, n_out), first,
                           (uint32_t)std::min<int64_t>(num_records, (int64_t)n_out)};  // nrc_helpers.cu:236
        do_train_gather(net, qs, reinterpret_cast<const float*>(ts), gs, b, loss_d);
    });
}

nrc_status nrc_infer_accumulate(nrc_net* net, const float* in, float* out, uint32_t n, const nrc_float3* thr,
                                float* rgba, uint32_t num_pixels, int mode, uint32_t iteration_index) {
    return guarded([&] {
        check_live(net);
        if (mode != NRC_RENDER_FULL && mode != NRC_RENDER_CACHE_ONLY)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "fused accumulation supports RenderMode Full and CacheOnly only");
        if (num_pixels > n) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "num_pixels > n");
        if (n == 0) return;
        if (!in || (num_pixels < n && !out)) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null query/result pointer");
        if (num_pixels > 0 && (!thr || !rgba || (reinterpret_cast<uintptr_t>(rgba) & 15)))
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "throughput / 16-byte aligned float4 frame buffer required");
        const float w = 1.0f / (float)(iteration_index + 1u);  // nrc_helpers.cu:98
        if (!net->wide() && net->cfg.infer_precision == NRC_PRECISION_F16_ACC16)
            throw ApiError(NRC_ERR_UNSUPPORTED, "fused accumulation runs the F16 numerics (use infer + accumulate)");
        if (net->wide())
            HIP_CHECK(infer_wide(net, (int)net->cfg.infer_precision, in, out, n, reinterpret_cast<const float*>(thr),
                                 rgba, num_pixels, mode, w, net->stream));
        else if (net->hash()) {
            uint32_t* const feat = net->hash_feat_arg();
            if (net->padq() && !feat)
                throw ApiError(NRC_ERR_UNSUPPORTED, "padded queries: the feature-pass Hash inference only");
            if (feat) net->hash_feat_acquire(net->stream);
            HIP_CHECK(launch_infer_hash(in, out, n, net->wf_infer, net->table_infer, reinterpret_cast<const float*>(thr),
                                        rgba, num_pixels, mode, w, net->stream, feat, net->padq()));
            if (feat) net->hash_feat_release(net->stream);
        }
        else if (net->encoding == NRC_ENCODING_FREQUENCY_SH)
            HIP_CHECK(launch_infer_sh(in, out, n, net->wf_infer, reinterpret_cast<const float*>(thr), rgba, num_pixels,
                                      mode, w, net->stream));
        else if (net->fp8_64())
            HIP_CHECK(launch_infer8(0, in, out, n, net->wf_infer, net->img8, reinterpret_cast<const float*>(thr), rgba,
                                    num_pixels, mode, w, net->stream));
        else
            HIP_CHECK(launch_infer_accumulate(in, out, n, net->wf_infer, reinterpret_cast<const float*>(thr), rgba,
                                              num_pixels, mode, w, net->stream, net->padq()));
    });
}

nrc_status nrc_infer_accumulate_sparse(nrc_net* net, const float* in, float* out, uint32_t n, const nrc_float3* thr,
                                       float* rgba, uint32_t num_pixels, int mode, uint32_t iteration_index) {
    return guarded([&] {
        check_live(net);
        if (mode != NRC_RENDER_FULL && mode != NRC_RENDER_CACHE_ONLY)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "fused accumulation supports RenderMode Full and CacheOnly only");
        if (num_pixels > n) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "num_pixels > n");
        if (const char* why = sparse_unsupported(net)) throw ApiError(NRC_ERR_UNSUPPORTED, why);
        if (n == 0) return;
        if (!in || (num_pixels < n && !out)) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null query/result pointer");
        if (num_pixels > 0 && (!thr || !rgba || (reinterpret_cast<uintptr_t>(rgba) & 15)))
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "throughput / 16-byte aligned float4 frame buffer required");
        const float w = 1.0f / (float)(iteration_index + 1u);  // nrc_helpers.cu:98
        HIP_CHECK(launch_infer_accumulate_sparse(in, out, n, net->wf_infer, reinterpret_cast<const float*>(thr), rgba,
                                                 num_pixels, mode, w, net->stream));
    });
}

nrc_status nrc_infer_accumulate_factored(nrc_net* net, const float* in, float* out, uint32_t n, const nrc_float3* thr,
                                         float* rgba, uint32_t num_pixels, int mode, uint32_t iteration_index) {
    return guarded([&] {
        check_live(net);
        const bool copy = mode == NRC_RENDER_DEBUG_CACHE_NO_THROUGHPUT_MODULATION;  // reads no throughput
        if (mode != NRC_RENDER_FULL && mode != NRC_RENDER_CACHE_ONLY && !copy)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "fused factored accumulation supports RenderMode Full, CacheOnly and "
                                                     "DebugCacheNoThroughputModulation only");
        if (num_pixels > n) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "num_pixels > n");
        if (const char* why = factored_unsupported(net)) throw ApiError(NRC_ERR_UNSUPPORTED, why);
        if (n == 0) return;
        if (!in || (num_pixels < n && !out)) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null query/result pointer");
        if (num_pixels > 0 && ((!copy && !thr) || !rgba || (reinterpret_cast<uintptr_t>(rgba) & 15)))
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "throughput / 16-byte aligned float4 frame buffer required");
        const float w = 1.0f / (float)(iteration_index + 1u);  // nrc_helpers.cu:98
        if (net->fp8_64())
            HIP_CHECK(launch_infer8(0, in, out, n, net->wf_infer, net->img8, reinterpret_cast<const float*>(thr), rgba,
                                    num_pixels, kInfer8Factored + mode, w, net->stream));
        else
            HIP_CHECK(launch_infer_accumulate_factored(in, out, n, net->wf_infer, reinterpret_cast<const float*>(thr),
                                                       rgba, num_pixels, mode, w, net->stream));
    });
}

nrc_status nrc_infer_accumulate_culled(nrc_net* net, const float* in, float* out, uint32_t n, const nrc_float3* thr,
                                       float* rgba, uint32_t num_pixels, int mode, uint32_t iteration_index,
                                       int reflectance_factoring) {
    return guarded([&] {
        check_live(net);
        if (mode != NRC_RENDER_FULL && mode != NRC_RENDER_CACHE_ONLY)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "culled fused accumulation supports RenderMode Full and CacheOnly only");
        if (num_pixels > n) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "num_pixels > n");
        if (n > kCullMaxQueries) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "culled fused accumulation: n must be <= 2^26");
        if (const char* why = culled_unsupported(net)) throw ApiError(NRC_ERR_UNSUPPORTED, why);
        if (n == 0) return;
        if (!in || (num_pixels < n && !out)) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null query/result pointer");
        if (num_pixels > 0 && (!thr || !rgba || (reinterpret_cast<uintptr_t>(rgba) & 15)))
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "throughput / 16-byte aligned float4 frame buffer required");
        if (!net->cull_ws || num_pixels > net->cull_ws_pixels) {  // grow: allocates (not capturable into a graph)
            if (net->cull_ws) {
                HIP_CHECK(hipStreamSynchronize(net->stream));  // a queued kernel may still use the old workspace
                HIP_CHECK(hipFree(net->cull_ws));
            }
            net->cull_ws = nullptr;
            net->cull_ws_pixels = 0;
            HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&net->cull_ws), cull_workspace_bytes(num_pixels)));
            net->cull_ws_pixels = num_pixels;
        }
        const float w = 1.0f / (float)(iteration_index + 1u);  // nrc_helpers.cu:98
        HIP_CHECK(launch_infer_accumulate_culled(in, out, n, net->wf_infer, net->fp8_64() ? net->img8 : nullptr,
                                                 reinterpret_cast<const float*>(thr), rgba, num_pixels, mode, w,
                                                 reflectance_factoring != 0, net->cull_ws, net->cull_ws_pixels,
                                                 net->stream));
    });
}

nrc_status nrc_infer(nrc_net* net, const float* in, float* out, uint32_t n) {
    return guarded([&] {
        check_live(net);
        if (n == 0) return;
        if (!in || !out) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null input/output pointer");
        HIP_CHECK(infer_any(net, in, out, n));
    });
}

nrc_status nrc_infer_stream(nrc_net* net, const float* in, float* out, uint32_t n, hipStream_t stream) {
    return guarded([&] {
        check_live(net);
        net->stream = stream;
        if (n == 0) return;
        if (!in || !out) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null input/output pointer");
        HIP_CHECK(infer_any(net, in, out, n));
    });
}

nrc_status nrc_set_stream(nrc_net* net, hipStream_t stream) {
    return guarded([&] {
        if (!net) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null handle");
        net->stream = stream;
    });
}

nrc_status nrc_get_stream(const nrc_net* net, hipStream_t* stream) {
    return guarded([&] {
        if (!net || !stream) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null argument");
        *stream = net->stream;
    });
}

nrc_status nrc_set_hyper_params(nrc_net* net, const nrc_hyper_params* hp) {
    return guarded([&] {
        check_live(net);
        if (!hp) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null hyper params");
        if (!(hp->learning_rate >= 0.0f) || !std::isfinite(hp->learning_rate))
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "learning rate must be finite and >= 0");
        net->cfg.learning_rate = hp->learning_rate;
    });
}

nrc_status nrc_set_config(nrc_net* net, int encoding) {
    return guarded([&] {
        if (!net) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null handle");
        if (encoding != NRC_ENCODING_FREQUENCY && encoding != NRC_ENCODING_HASH && encoding != NRC_ENCODING_FREQUENCY_SH)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "Unsupported input encoding");
        // The reference's setConfig only rewrites the config JSON (NRCNetwork.cu:96-99); the live model keeps its
        // encoding, weights and optimizer state until the next init_ (:106-112), which re-derives the config from
        // its own encoding argument. On a live handle this therefore changes only what nrc_get_config_json prints;
        // the encoding, the hyper-parameters and every buffer layout the kernels depend on stay untouched.
        net->config_encoding = encoding;
        if (!net->initialized) {
            net->encoding = encoding;
            net->cfg = nrc_default_config(encoding);
        }
    });
}

nrc_status nrc_get_learning_rate(const nrc_net* net, float* lr) {
    return guarded([&] {
        check_live(net);
        if (!lr) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null output");
        *lr = net->cfg.learning_rate;
    });
}

nrc_status nrc_get_config_json(const nrc_net* net, char* buf, size_t cap, size_t* needed) {
    return guarded([&] {
        if (!net) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null handle");
        // after a setConfig on a live handle: the JSON of that encoding's default config (as the reference's
        // printConfig_ would print it), otherwise the live model's config
        const std::string s = net->config_encoding != net->encoding
                                  ? config_json(net->config_encoding, nrc_default_config(net->config_encoding))
                                  : config_json(net->encoding, net->cfg);
        if (needed) *needed = s.size() + 1;
        if (buf && cap) {
            const size_t k = s.size() < cap - 1 ? s.size() : cap - 1;
            std::memcpy(buf, s.data(), k);
            buf[k] = '\0';
        }
    });
}

namespace {
void do_train_grad(nrc_net* net, const float* in, const float* tgt, uint32_t b, uint32_t global_b, float* grad_d,
                   int64_t* grid_fixed = nullptr);
void do_train_apply(nrc_net* net, const float* grad_d, float* loss_h, float* loss_d,
                    const int64_t* grid_fixed = nullptr);
void require_hash(const nrc_net* net, const char* what) {
    check_live(net);
    if (!net->hash()) throw ApiError(NRC_ERR_UNSUPPORTED, std::string(what) + ": InputEncoding::Hash only");
}
}  // namespace

nrc_status nrc_train_grad(nrc_net* net, const float* in, const float* tgt, uint32_t b, uint32_t global_b,
                          float* grad_d) {
    return guarded([&] { do_train_grad(net, in, tgt, b, global_b, grad_d); });
}

nrc_status nrc_train_apply(nrc_net* net, const float* grad_d, float* loss_h) {
    return guarded([&] { do_train_apply(net, grad_d, loss_h, nullptr); });
}

nrc_status nrc_train_grad_fixed(nrc_net* net, const float* in, const float* tgt, uint32_t b, uint32_t global_b,
                                float* grad_d, int64_t* grid_fixed_d) {
    return guarded([&] {
        require_hash(net, "nrc_train_grad_fixed");
        if (!grid_fixed_d) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null grid_fixed_d");
        do_train_grad(net, in, tgt, b, global_b, grad_d, grid_fixed_d);
    });
}

nrc_status nrc_train_apply_fixed(nrc_net* net, const float* grad_d, const int64_t* grid_fixed_d, float* loss_h) {
    return guarded([&] {
        require_hash(net, "nrc_train_apply_fixed");
        if (!grid_fixed_d) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null grid_fixed_d");
        do_train_apply(net, grad_d, loss_h, nullptr, grid_fixed_d);
    });
}

namespace {
void nccl_check(ncclResult_t r, const char* what) {
    if (r != ncclSuccess)
        throw ApiError(NRC_ERR_HIP, std::string(what) + " failed: " + ncclGetErrorString(r));
}

// Sequence number of the peer exchange's next step: never 0 (the tag of a zeroed receive buffer), and its parity (the
// buffer half a step uses) alternates across the wrap, 0xFFFFFFFF -> 2, as the two-parity protocol requires.
uint32_t px_next(uint32_t seq) { return seq == 0xFFFFFFFFu ? 2u : seq + 1u; }

int px_polls() {
    const int k = knob(kKnobPxPolls);
    return k > 0 ? k : kPeerPolls;
}

// nrc_train_dp over an open peer exchange. Every argument is checked and the protocol state read before anything is
// launched, and the handle's sequence number advances only once the exchange launch has been issued: a call rejected
// on one rank leaves that rank's sequence where its peers expect it, so the next step still pairs up.
void do_peer_step(nrc_net* net, const float* in, const float* tgt, uint32_t b_local, uint32_t global_b, float* loss_h,
                  float* loss_d) {
    const int kp = knob(kKnobPeerPath);
    const int nfl = (int)net->grad_floats();
    const int polls = px_polls();
    if (kp != 4) {
        if (global_b < b_local || global_b == 0)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "global_b must be >= b and >= 1");
        if (b_local > 0 && (!in || !tgt)) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null input/target pointer");
    }
    if ((kp == 4) != net->px_pending)
        throw ApiError(NRC_ERR_INVALID_ARGUMENT, net->px_pending
                                                     ? "peer exchange: a pushed step awaits its apply (knob peer_path 4)"
                                                     : "peer exchange: no pushed step to apply (knob peer_path 3 first)");
    net->check_protocol();
    if (kp == 3 && loss_h) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "peer_path 3 pushes only: no loss to return");
    const int form = kp == -1 ? (net->px_shared ? kPxSplit : kPxFused)
                     : kp == 1 ? kPxFused
                     : kp == 2 ? kPxSplit
                     : kp == 3 ? kPxPushOnly
                     : kp == 4 ? kPxApplyOnly
                               : -1;  // 0: the reduce + push + apply launches
    float* const ld = loss_d ? loss_d : net->loss_dev;
    const uint32_t st = net->step + 1;
    if (form == kPxApplyOnly) {
        // the pushed step's sequence number is already committed; a slab count of 1 is a placeholder (no reduce runs)
        HIP_CHECK(launch_reduce_exchange(net->slabs, 1, net->loss_partials, net->px_peers, net->px_rank, net->px_world,
                                         nfl, net->px_seq, net->proto_err_dev(), ld, net->buffers(), net->optim(st),
                                         net->stream, kPxApplyOnly, polls));
        net->step = st;
        net->px_pending = false;
        pack_fp8_64(net, net->stream);
    } else {
        const uint32_t seq = px_next(net->px_seq);
        if (form >= 0) {
            // the exchange fused into the reduction: gradient pass -> one launch that reduces the slabs, pushes each
            // block's partials to every rank, waits for the same block of every rank, sums in rank order, Adam/EMA
            // (split: the wait + sum + Adam as a second, small launch -- ranks sharing this device)
            int blocks = 1;
            if (b_local > 0) {
                blocks = train_block_count(net, b_local);
                net->ensure_slabs(blocks);
                train_partials(net, in, tgt, b_local, 3.0f * (float)global_b);
            } else {  // no local samples: one zero slab and a zero loss partial (the rank still takes part)
                net->ensure_slabs(1);
                const ModelBuffers mb = net->buffers();
                HIP_CHECK(hipMemsetAsync(net->slabs, 0, (mb.slab_f16 ? 2 : 4) * (size_t)mb.n_slab, net->stream));
                HIP_CHECK(hipMemsetAsync(net->loss_partials, 0, sizeof(float), net->stream));
            }
            HIP_CHECK(launch_reduce_exchange(net->slabs, blocks, net->loss_partials, net->px_peers, net->px_rank,
                                             net->px_world, nfl, seq, net->proto_err_dev(), ld, net->buffers(),
                                             net->optim(st), net->stream, form, polls));
        } else {
            // round 4's first version (knob peer_path = 0; world >= 2): reduce to a gradient -> push the gradient to
            // every peer's receive slot -> wait + rank-order sum + Adam/EMA
            if (!net->dp_grad) HIP_CHECK(hipMalloc(&net->dp_grad, sizeof(float) * net->grad_floats()));
            do_train_grad(net, in, tgt, b_local, global_b, net->dp_grad);
            HIP_CHECK(launch_peer_push(net->dp_grad, nfl, net->px_peers, net->px_rank, net->px_world, seq, net->stream));
            HIP_CHECK(launch_peer_apply(net->px_buf, net->px_world, nfl, seq, net->proto_err_dev(), ld, net->buffers(),
                                        net->optim(st), net->stream, polls));
        }
        net->px_seq = seq;
        if (form == kPxPushOnly) {
            net->px_pending = true;
        } else {
            net->step = st;
            pack_fp8_64(net, net->stream);
        }
    }
    if (loss_h) {
        if (loss_d) {
            HIP_CHECK(hipStreamSynchronize(net->stream));
            net->check_protocol();
            HIP_CHECK(hipMemcpy(loss_h, loss_d, sizeof(float), hipMemcpyDeviceToHost));
        } else {
            *loss_h = net->read_loss();
        }
    }
}

void do_train_dp(nrc_net* net, const float* in, const float* tgt, uint32_t b_local, uint32_t global_b, float* loss_h,
                 float* loss_d) {
    check_live(net);
    if (!net->comm && !net->px_open)
        throw ApiError(NRC_ERR_INVALID_ARGUMENT, "no communicator attached (nrc_set_comm / nrc_peer_exchange_open)");
    if (net->px_open) {
        do_peer_step(net, in, tgt, b_local, global_b, loss_h, loss_d);
        return;
    }
    if (!net->dp_grad) HIP_CHECK(hipMalloc(&net->dp_grad, sizeof(float) * net->grad_floats()));
    if (net->hash()) {
        // exact grid exchange: each rank's fixed-point sums, exchange-encoded in place in the handle's accumulator,
        // summed as int64 beside the f32 MLP gradient and loss (one RCCL group on the handle's stream), then rounded
        // to f16 once by the grid Adam -- every rank applies the sums a single GPU forms over the global minibatch
        if (net->comm_world > kFixedMaxRanks)
            throw ApiError(NRC_ERR_UNSUPPORTED, "Hash data parallelism: at most 63 ranks (exchange encoding)");
        do_train_grad(net, in, tgt, b_local, global_b, net->dp_grad, net->grid_grad);
        nccl_check(ncclGroupStart(), "ncclGroupStart");
        nccl_check(ncclAllReduce(net->dp_grad, net->dp_grad, net->n_mlp, ncclFloat32, ncclSum, net->comm, net->stream),
                   "ncclAllReduce");
        nccl_check(ncclAllReduce(net->dp_grad + net->n_total(), net->dp_grad + net->n_total(), 4, ncclFloat32, ncclSum,
                                 net->comm, net->stream), "ncclAllReduce");
        nccl_check(ncclAllReduce(net->grid_grad, net->grid_grad, net->n_grid, ncclInt64, ncclSum, net->comm,
                                 net->stream), "ncclAllReduce");
        nccl_check(ncclGroupEnd(), "ncclGroupEnd");
        do_train_apply(net, net->dp_grad, loss_h, loss_d, net->grid_grad);
        return;
    }
    do_train_grad(net, in, tgt, b_local, global_b, net->dp_grad);
    // one all-reduce of the gradient and the loss partial, on the handle's stream (stream-ordered with the kernels)
    nccl_check(ncclAllReduce(net->dp_grad, net->dp_grad, net->grad_floats(), ncclFloat32, ncclSum, net->comm,
                             net->stream), "ncclAllReduce");
    do_train_apply(net, net->dp_grad, loss_h, loss_d);
}

void do_train_grad(nrc_net* net, const float* in, const float* tgt, uint32_t b, uint32_t global_b, float* grad_d,
                   int64_t* grid_fixed) {
    {
        check_live(net);
        if (!grad_d) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null gradient buffer");
        if (global_b < b || global_b == 0) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "global_b must be >= b and >= 1");
        if (b == 0) {
            HIP_CHECK(hipMemsetAsync(grad_d, 0, sizeof(float) * net->grad_floats(), net->stream));
            if (grid_fixed) HIP_CHECK(hipMemsetAsync(grid_fixed, 0, sizeof(int64_t) * net->n_grid, net->stream));
            return;
        }
        if (!in || !tgt) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null input/target pointer");
        if (net->wide()) {
            wide_grad_partials(net, in, tgt, b, 3.0f * (float)global_b);
            HIP_CHECK(launch_wide_adam(kReduceOnly, net->wide_slabs, wide_chunks(b), net->wide_loss_partials,
                                       (int)(wide_bpad(b) / 32), grad_d, nullptr, net->buffers(),
                                       net->optim(net->step + 1), wide_images(net), net->stream));
            return;
        }
        const int blocks = train_block_count(net, b);
        net->ensure_slabs(blocks);
        if (net->hash()) {
            // the grid-table gradient accumulates in the handle's exact fixed-point buffer (grid_scatter_kernel) and is
            // exported after the MLP part: rounded to f16, as f32, into the caller's gradient (nrc_train_grad), or
            // exchange-encoded into grid_fixed (nrc_train_grad_fixed, nrc_train_dp); the export zeroes the buffer
            // (unless grid_fixed is the buffer itself)
            train_hash(net, in, tgt, b, 3.0f * (float)global_b, blocks);
            if (grid_fixed)
                HIP_CHECK(launch_grid_grad_export_fixed(net->grid_grad, grid_fixed, net->n_grid, net->nonfinite(),
                                                        net->stream));
            else
                HIP_CHECK(launch_grid_grad_export(net->grid_grad, grad_d + net->n_mlp, net->n_grid, net->nonfinite(),
                                                  net->stream));
        } else {
            train_partials(net, in, tgt, b, 3.0f * (float)global_b);
        }
        HIP_CHECK(launch_reduce_adam(kReduceOnly, net->slabs, blocks, net->loss_partials, grad_d, nullptr,
                                     net->buffers(), net->optim(net->step + 1), net->stream));
    }
}

void do_train_apply(nrc_net* net, const float* grad_d, float* loss_h, float* loss_d, const int64_t* grid_fixed) {
    check_live(net);
    if (!grad_d) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null gradient buffer");
    net->step += 1;
    float* ld = loss_d ? loss_d : net->loss_dev;
    if (net->wide()) {
        HIP_CHECK(launch_wide_adam(kApplyOnly, nullptr, 0, nullptr, 0, const_cast<float*>(grad_d), ld, net->buffers(),
                                   net->optim(net->step), wide_images(net), net->stream));
    } else {
        HIP_CHECK(launch_reduce_adam(kApplyOnly, nullptr, 0, nullptr, const_cast<float*>(grad_d), ld, net->buffers(),
                                     net->optim(net->step), net->stream));
        pack_fp8_64(net, net->stream);
        if (net->hash()) {
            GridBuffers gb = net->grid_buffers();
            gb.grad32 = grad_d + net->n_mlp;  // read-only in kApplyOnly
            gb.fixed = grid_fixed;            // kApplyFixed: read-only unless it is the handle's accumulator
            HIP_CHECK(launch_grid_adam(grid_fixed ? kApplyFixed : kApplyOnly, gb, net->optim(net->step), net->stream));
        }
    }
    if (loss_h) {
        if (loss_d) {
            HIP_CHECK(hipStreamSynchronize(net->stream));
            net->check_protocol();
            HIP_CHECK(hipMemcpy(loss_h, loss_d, sizeof(float), hipMemcpyDeviceToHost));
        } else {
            *loss_h = net->read_loss();
        }
    }
}
}  // namespace

nrc_status nrc_comm_get_unique_id(void* id_out) {
    return guarded([&] {
        if (!id_out) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null output");
        static_assert(sizeof(ncclUniqueId) == NRC_COMM_UNIQUE_ID_BYTES, "unique id size");
        ncclUniqueId id;
        nccl_check(ncclGetUniqueId(&id), "ncclGetUniqueId");
        std::memcpy(id_out, &id, sizeof(id));
    });
}

nrc_status nrc_comm_init_rank(void** comm_out, const void* unique_id, int world, int rank) {
    return guarded([&] {
        if (!comm_out || !unique_id) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null argument");
        if (world < 1 || rank < 0 || rank >= world) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "bad rank / world");
        ncclUniqueId id;
        std::memcpy(&id, unique_id, sizeof(id));
        ncclComm_t c = nullptr;
        nccl_check(ncclCommInitRank(&c, world, id, rank), "ncclCommInitRank");
        *comm_out = c;
    });
}

nrc_status nrc_comm_destroy(void* comm) {
    return guarded([&] {
        if (comm) nccl_check(ncclCommDestroy(static_cast<ncclComm_t>(comm)), "ncclCommDestroy");
    });
}

nrc_status nrc_set_comm(nrc_net* net, void* comm) {
    return guarded([&] {
        check_live(net);
        net->comm = static_cast<ncclComm_t>(comm);
        net->comm_rank = 0;
        net->comm_world = 1;
        if (net->comm) {
            nccl_check(ncclCommUserRank(net->comm, &net->comm_rank), "ncclCommUserRank");
            nccl_check(ncclCommCount(net->comm, &net->comm_world), "ncclCommCount");
        }
    });
}

nrc_status nrc_get_comm_rank(const nrc_net* net, int* rank, int* world) {
    return guarded([&] {
        check_live(net);
        if (!rank || !world) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null output");
        *rank = net->comm_rank;
        *world = net->comm_world;
    });
}

nrc_status nrc_train_dp(nrc_net* net, const float* in, const float* tgt, uint32_t b_local, uint32_t global_b,
                        float* loss_h) {
    return guarded([&] { do_train_dp(net, in, tgt, b_local, global_b, loss_h, nullptr); });
}

nrc_status nrc_train_dp_async(nrc_net* net, const float* in, const float* tgt, uint32_t b_local, uint32_t global_b,
                              float* loss_d) {
    return guarded([&] { do_train_dp(net, in, tgt, b_local, global_b, nullptr, loss_d); });
}

nrc_status nrc_peer_exchange_handle(nrc_net* net, int world, void* handle_out) {
    return guarded([&] {
        check_live(net);
        if (!handle_out) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null handle output");
        if (net->hash() || net->wide())
            throw ApiError(NRC_ERR_UNSUPPORTED, "the peer exchange is implemented for the width-64 Frequency / FrequencySH "
                                                "networks (Hash and width 128 use the RCCL path)");
        if (world < 1 || world > kPeerMaxRanks) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "world must be 1..16");
        static_assert(sizeof(hipIpcMemHandle_t) == NRC_PEER_HANDLE_BYTES, "IPC handle size");
        net->peer_close();
        const size_t bytes = peer_buffer_bytes(world, (int)net->grad_floats(), net->buffers().n_slab);
        // uncached device memory: the peers' xGMI stores and this GPU's loads meet in memory, not in a stale L2 line
        HIP_CHECK(hipExtMallocWithFlags(reinterpret_cast<void**>(&net->px_buf), bytes, hipDeviceMallocUncached));
        HIP_CHECK(hipMemset(net->px_buf, 0, bytes));  // flags 0: before any peer can know the handle
        HIP_CHECK(hipDeviceSynchronize());
        net->px_world = world;
        HIP_CHECK(hipIpcGetMemHandle(static_cast<hipIpcMemHandle_t*>(handle_out), net->px_buf));
    });
}

nrc_status nrc_peer_exchange_open(nrc_net* net, int rank, int world, const void* handles) {
    return guarded([&] {
        check_live(net);
        if (!handles) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null handles");
        if (!net->px_buf || net->px_open || world != net->px_world)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "call nrc_peer_exchange_handle with the same world first (once)");
        if (rank < 0 || rank >= world) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "bad rank");
        PeerPtrs p{};
        const auto* h = static_cast<const hipIpcMemHandle_t*>(handles);
        for (int r = 0; r < world; ++r) {
            if (r == rank) {
                p.p[r] = net->px_buf;
                continue;
            }
            void* ptr = nullptr;
            const hipError_t e = hipIpcOpenMemHandle(&ptr, h[r], hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess) {
                for (int q = 0; q < r; ++q)
                    if (q != rank && p.p[q]) (void)hipIpcCloseMemHandle(p.p[q]);
                throw ApiError(NRC_ERR_HIP, std::string("hipIpcOpenMemHandle(rank ") + std::to_string(r) +
                                                "): " + hipGetErrorString(e));
            }
            p.p[r] = static_cast<float*>(ptr);
        }
        // ranks on one device (tests; oversubscription): the exchange's waits go to the split path's small apply grid
        bool shared = false;
        for (int r = 0; r < world; ++r) {
            if (r == rank) continue;
            hipPointerAttribute_t a{};
            if (hipPointerGetAttributes(&a, p.p[r]) == hipSuccess && a.device == net->device) shared = true;
        }
        net->px_shared = shared;
        net->px_peers = p;
        net->px_rank = rank;
        net->px_seq = 0;
        net->px_open = true;
    });
}

nrc_status nrc_peer_exchange_close(nrc_net* net) {
    return guarded([&] {
        check_live(net);
        HIP_CHECK(hipStreamSynchronize(net->stream));
        net->peer_close();
    });
}

nrc_status nrc_peer_exchange_open_local(nrc_net* const* nets, int world) {
    return guarded([&] {
        if (!nets) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null handle array");
        if (world < 1 || world > kPeerMaxRanks) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "world must be 1..16");
        for (int r = 0; r < world; ++r) {
            check_live(nets[r]);
            if (nets[r]->hash() || nets[r]->wide())
                throw ApiError(NRC_ERR_UNSUPPORTED, "the peer exchange is implemented for the width-64 Frequency / "
                                                    "FrequencySH networks (Hash and width 128 use the RCCL path)");
            if (nets[r]->encoding != nets[0]->encoding)
                throw ApiError(NRC_ERR_INVALID_ARGUMENT, "every handle of one exchange must have the same encoding");
            for (int q = 0; q < r; ++q)
                if (nets[q] == nets[r]) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "a handle appears twice");
        }
        int cur = 0;
        HIP_CHECK(hipGetDevice(&cur));
        struct Restore {
            int dev;
            ~Restore() { (void)hipSetDevice(dev); }
        } restore{cur};
        for (int r = 0; r < world; ++r) {
            HIP_CHECK(hipStreamSynchronize(nets[r]->stream));
            nets[r]->peer_close();
        }
        // each rank's receive buffer on its own device (uncached, as for the IPC form); the peers store into it
        // through plain device pointers, over xGMI when the devices differ (peer access enabled both ways)
        for (int r = 0; r < world; ++r) {
            nrc_net* n = nets[r];
            HIP_CHECK(hipSetDevice(n->device));
            const size_t bytes = peer_buffer_bytes(world, (int)n->grad_floats(), n->buffers().n_slab);
            const hipError_t e = hipExtMallocWithFlags(reinterpret_cast<void**>(&n->px_buf), bytes, hipDeviceMallocUncached);
            if (e != hipSuccess) {
                for (int q = 0; q <= r; ++q) nets[q]->peer_close();
                throw ApiError(e == hipErrorOutOfMemory ? NRC_ERR_OUT_OF_MEMORY : NRC_ERR_HIP,
                               std::string("hipExtMallocWithFlags: ") + hipGetErrorString(e));
            }
            HIP_CHECK(hipMemset(n->px_buf, 0, bytes));
            for (int q = 0; q < world; ++q) {
                if (nets[q]->device == n->device) continue;
                const hipError_t pe = hipDeviceEnablePeerAccess(nets[q]->device, 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled)
                    throw ApiError(NRC_ERR_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(pe));
                (void)hipGetLastError();
            }
            HIP_CHECK(hipDeviceSynchronize());
        }
        PeerPtrs p{};
        for (int r = 0; r < world; ++r) p.p[r] = nets[r]->px_buf;
        auto group = std::make_shared<LocalPeerGroup>();
        group->members.assign(nets, nets + world);
        for (int r = 0; r < world; ++r) {
            nrc_net* n = nets[r];
            n->px_group = group;
            bool shared = false;
            for (int q = 0; q < world; ++q) shared = shared || (q != r && nets[q]->device == n->device);
            n->px_peers = p;
            n->px_world = world;
            n->px_rank = r;
            n->px_seq = 0;
            n->px_shared = shared;
            n->px_local = true;
            n->px_pending = false;
            n->px_open = true;
        }
    });
}

nrc_status nrc_debug_set_peer_seq(nrc_net* net, uint32_t seq) {
    return guarded([&] {
        check_live(net);
        if (!net->px_open || net->px_pending)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "no open peer exchange between steps");
        if (seq == 0) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "sequence number 0 is the tag of an empty buffer");
        net->px_seq = seq;
    });
}

nrc_status nrc_get_state(nrc_net* net, int slot, float* host_dst) {
    return guarded([&] {
        check_live(net);
        if (!host_dst) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null destination");
        float* src = slot_ptr(net, slot);
        HIP_CHECK(hipStreamSynchronize(net->stream));
        net->check_protocol();
        HIP_CHECK(hipMemcpy(host_dst, src, sizeof(float) * net->n_total(), hipMemcpyDeviceToHost));
        if (net->padq()) padq_w0_columns(net->encoding, host_dst, true);
    });
}

nrc_status nrc_set_state(nrc_net* net, int slot, const float* host_src) {
    return guarded([&] {
        check_live(net);
        if (!host_src) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null source");
        float* dst = slot_ptr(net, slot);
        HIP_CHECK(hipStreamSynchronize(net->stream));
        if (net->padq()) {
            std::vector<float> tmp(host_src, host_src + net->n_total());
            padq_w0_columns(net->encoding, tmp.data(), false);
            HIP_CHECK(hipMemcpy(dst, tmp.data(), sizeof(float) * net->n_total(), hipMemcpyHostToDevice));
        } else {
            HIP_CHECK(hipMemcpy(dst, host_src, sizeof(float) * net->n_total(), hipMemcpyHostToDevice));
        }
        if (slot == NRC_STATE_PARAMS || slot == NRC_STATE_INFER) {
            repack(net, net->stream);
            HIP_CHECK(hipStreamSynchronize(net->stream));
        }
    });
}

nrc_status nrc_get_num_params(const nrc_net* net, uint64_t* n) {
    return guarded([&] {
        check_live(net);
        if (!n) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null output pointer");
        *n = net->n_total();
    });
}

nrc_status nrc_get_grad_floats(const nrc_net* net, uint64_t* n) {
    return guarded([&] {
        check_live(net);
        if (!n) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null output");
        *n = net->grad_floats();
    });
}

nrc_status nrc_debug_encode_net(nrc_net* net, const float* in, float* enc, uint32_t n, hipStream_t stream) {
    return guarded([&] {
        check_live(net);
        if (n == 0) return;
        if (!in || !enc) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null pointer");
        if (net->hash()) HIP_CHECK(launch_encode_hash(in, net->table_infer, enc, n, stream));
        else if (net->encoding == NRC_ENCODING_FREQUENCY_SH) HIP_CHECK(launch_encode_sh(in, enc, n, stream));
        else HIP_CHECK(launch_encode_fast(in, enc, n, stream));
    });
}

nrc_status nrc_get_step(const nrc_net* net, uint32_t* step) {
    return guarded([&] {
        check_live(net);
        if (!step) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null output");
        *step = net->step;
    });
}

nrc_status nrc_set_step(nrc_net* net, uint32_t step) {
    return guarded([&] {
        check_live(net);
        net->step = step;
    });
}

nrc_status nrc_debug_infer_variant(nrc_net* net, int variant, const float* in, float* out, uint32_t n,
                                   hipStream_t stream) {
    return guarded([&] {
        check_live(net);
        require_frequency(net, "nrc_debug_infer_variant");
        if (net->wide()) throw ApiError(NRC_ERR_UNSUPPORTED, "inference variants are 64-wide kernels");
        if (variant < 0 || variant >= kNumInferVariants) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "unknown variant");
        if (n == 0) return;
        if (!in || !out) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null input/output pointer");
#if NRC_DEBUG_KERNELS
        if (variant == 50 || variant == 51) {  // 51 (debug): the t16 training image (master weights)
            if (!net->wf_infer16) throw ApiError(NRC_ERR_UNSUPPORTED, "variants 50/51 need a Frequency t16 handle");
            HIP_CHECK(launch_infer16(in, out, n, variant == 50 ? net->wf_infer16 : net->wf_train, stream));
            return;
        }
#endif
        const hipError_t e = launch_infer_variant(variant, in, out, n, net->wf_infer, stream, net->work_queue,
                                                  &net->pool_parity);
        if (e == hipErrorInvalidValue && variant != kProductInferVariant)
            throw ApiError(NRC_ERR_UNSUPPORTED, "inference variant " + std::to_string(variant) +
                                                    " is an A/B kernel of the debug library (libnrc_amd_debug.so via "
                                                    "NRC_LIB_PATH)");
        HIP_CHECK(e);
    });
}

nrc_status nrc_debug_read_infer_clock(uint64_t* host_dst, uint32_t cap_waves, uint32_t* waves) {
    return guarded([&] {
        if (!host_dst || !waves) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null pointer");
        int64_t w = 0;
        HIP_CHECK(hipDeviceSynchronize());
        const hipError_t e = read_infer_clock(host_dst, (int64_t)cap_waves, &w);
        if (e == hipErrorNotSupported) throw ApiError(NRC_ERR_UNSUPPORTED, kDebugOnly);
        HIP_CHECK(e);
        *waves = (uint32_t)w;
    });
}

nrc_status nrc_debug_infer_stamps(nrc_net* net, const float* in, float* out, uint32_t n, uint64_t* stamps_d,
                                  uint64_t* waves_h) {
    return guarded([&] {
        check_live(net);
        require_frequency(net, "nrc_debug_infer_stamps");
        if (net->wide()) throw ApiError(NRC_ERR_UNSUPPORTED, "inference stamps are a 64-wide diagnostic");
        if (!in || !out || !stamps_d || !waves_h || n == 0) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "bad arguments");
        int64_t waves = 0;
        const hipError_t e = launch_infer_stamped(in, out, n, net->wf_infer, stamps_d, &waves, net->stream);
        if (e == hipErrorNotSupported) throw ApiError(NRC_ERR_UNSUPPORTED, kDebugOnly);
        HIP_CHECK(e);
        if (waves > NRC_INFER_STAMP_WAVES_MAX) throw ApiError(NRC_ERR_INTERNAL, "stamp buffer too small");
        *waves_h = (uint64_t)waves;
    });
}

nrc_status nrc_debug_train_stamps(nrc_net* net, const float* in, const float* tgt, uint32_t b, uint64_t* stamps_d) {
    return guarded([&] {
        check_live(net);
        require_frequency(net, "nrc_debug_train_stamps");
        if (net->wide()) throw ApiError(NRC_ERR_UNSUPPORTED, "training stamps are a 64-wide diagnostic");
        if (!in || !tgt || !stamps_d || b == 0) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "bad arguments");
#if !NRC_DEBUG_KERNELS
        throw ApiError(NRC_ERR_UNSUPPORTED, kDebugOnly);
#endif
        const int blocks = train_block_count(net, b);
        net->ensure_slabs(blocks);
        train_partials(net, in, tgt, b, 3.0f * (float)b, stamps_d);
    });
}

nrc_status nrc_debug_hash_scatter_inputs(nrc_net* net, float* pos_d, uint32_t* dy_d, uint32_t b) {
    return guarded([&] {
        check_live(net);
        if (!net->hash()) throw ApiError(NRC_ERR_UNSUPPORTED, "nrc_debug_hash_scatter_inputs: InputEncoding::Hash only");
        if (!pos_d || !dy_d || b == 0) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "bad arguments");
        if (!net->scatter.pos || (int64_t)b > net->scatter.bcap)
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "b exceeds the last training call's scatter buffers");
        HIP_CHECK(hipMemcpyAsync(pos_d, net->scatter.pos, sizeof(float4) * b, hipMemcpyDeviceToDevice, net->stream));
        for (int l = 0; l < NRC_HASH_LEVELS; ++l)
            HIP_CHECK(hipMemcpyAsync(dy_d + (size_t)l * b, net->scatter.dy + (size_t)l * net->scatter.bcap,
                                     sizeof(uint32_t) * b, hipMemcpyDeviceToDevice, net->stream));
    });
}

nrc_status nrc_debug_infer_precision(nrc_net* net, int precision, const float* in, float* out, uint32_t n,
                                     hipStream_t stream) {
    return guarded([&] {
        check_live(net);
        if (!net->wide() && precision == NRC_PRECISION_F16_ACC16) {  // tcnn numerics on a width-64 network
            if (net->encoding == NRC_ENCODING_FREQUENCY_SH || net->padq())
                throw ApiError(NRC_ERR_UNSUPPORTED, "F16_ACC16 is implemented for the compact Frequency / Hash encodings");
            if (n == 0) return;
            if (!in || !out) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null input/output pointer");
            if (net->hash()) {
                net->hash_feat_acquire(stream);
                HIP_CHECK(launch_infer_hash_tcnn(in, out, n, net->wf_infer, net->infer, net->table_infer, net->hash_feat,
                                                 stream));
                net->hash_feat_release(stream);
            } else {
                HIP_CHECK(launch_infer_tcnn(in, out, n, net->wf_infer, net->infer, stream));
            }
            return;
        }
        if (net->fp8_64()) {
            // a width-64 handle configured with FP8 keeps its f16 image: F16 = the production f16 kernel, FP8 = the FP8
            // kernel (bits 4+: 1 = its A/B loser shape, debug library), for the in-process A/B
            const int prec = precision & 15, variant = precision >> 4;
            if ((prec != NRC_PRECISION_F16 && prec != NRC_PRECISION_FP8) || variant < 0 || variant > 1 ||
                (variant && prec != NRC_PRECISION_FP8))
                throw ApiError(NRC_ERR_INVALID_ARGUMENT, "unknown precision");
            if (n == 0) return;
            if (!in || !out) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null input/output pointer");
            const hipError_t e =
                prec == NRC_PRECISION_F16
                    ? launch_infer(in, out, n, net->wf_infer, stream, net->work_queue, &net->pool_parity, false)
                    : launch_infer8(variant, in, out, n, net->wf_infer, net->img8, nullptr, nullptr, 0, -1, 1.0f, stream);
            if (e == hipErrorNotSupported) throw ApiError(NRC_ERR_UNSUPPORTED, kDebugOnly);
            HIP_CHECK(e);
            return;
        }
        if (!net->wide()) throw ApiError(NRC_ERR_UNSUPPORTED, "precision selection is for the width-128 network");
        // bits 4+: kernel variant (0 = production; 1 = 1024-thread blocks, Frequency only; 2 = FP8 with the ReLU on
        // the converted bytes)
        const int prec = precision & 15, variant = precision >> 4;
        if ((prec != NRC_PRECISION_F16 && prec != NRC_PRECISION_FP8) || variant < 0 || variant > 2 ||
            (variant == 2 && prec != NRC_PRECISION_FP8))
            throw ApiError(NRC_ERR_INVALID_ARGUMENT, "unknown precision");
        if (variant && wide_enc(net) != 0) throw ApiError(NRC_ERR_UNSUPPORTED, "kernel variants are Frequency-only");
        if (n == 0) return;
        if (!in || !out) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null input/output pointer");
        const hipError_t e = infer_wide(net, precision, in, out, n, nullptr, nullptr, 0, -1, 1.0f, stream);
        if (e == hipErrorNotSupported) throw ApiError(NRC_ERR_UNSUPPORTED, kDebugOnly);
        HIP_CHECK(e);
    });
}

nrc_status nrc_debug_fp8_convert(const float* x, uint8_t* y, uint32_t n, int relu, hipStream_t stream) {
    return guarded([&] {
        if (n == 0) return;
        if (!x || !y) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null pointer");
        HIP_CHECK(launch_fp8_convert(x, y, n, relu, stream));
    });
}

nrc_status nrc_encode(const float* in, float* enc, uint32_t n, hipStream_t stream) {
    return guarded([&] {
        if (n == 0) return;
        if (!in || !enc) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null pointer");
        HIP_CHECK(launch_encode(in, enc, n, stream));
    });
}

nrc_status nrc_debug_encode_fast(const float* in, float* enc, uint32_t n, hipStream_t stream) {
    return guarded([&] {
        if (n == 0) return;
        if (!in || !enc) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null pointer");
        HIP_CHECK(launch_encode_fast(in, enc, n, stream));
    });
}

nrc_status nrc_debug_encode_fast_variant(int variant, const float* in, float* enc, uint32_t n, hipStream_t stream) {
    return guarded([&] {
        if (variant < 0 || variant > 2) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "encoder variant must be 0, 1 or 2");
        if (n == 0) return;
        if (!in || !enc) throw ApiError(NRC_ERR_INVALID_ARGUMENT, "null pointer");
        HIP_CHECK(launch_encode_fast(in, enc, n, stream, variant));
    });
}

}  // extern "C"
