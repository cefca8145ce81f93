"""FP8 (e4m3 MX MFMA) inference of the 64-wide Frequency network (nrc_infer8.hip, DESIGN.md §12 "Width 64") against a
float64 numpy model of its contract: layer 0 f16 x f16; ReLU outputs of layers 0..4 clamped to [0, 448] and rounded (RNE)
onto e4m3; W1..W5 e4m3 with one power-of-two scale per row; f32 pre-activations; output through f16. Single-term weights:
bitwise. Dense weights: the MX MFMA's block sum is not f32-exact (<= 2.2e-5 sum|a b|), so a pre-activation near an e4m3
boundary can land one step away: rel-L2(GPU, model) <= B = 1.5 x the first GPU measurement (ceiling 6e-2)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(64, 80), (64, 64), (64, 64), (64, 64), (64, 64), (16, 64)]
OFFS = np.cumsum([0] + [o * i for o, i in SHAPES])
# measured on MI355X, dense xavier weights (gain 1.6): rel-L2 1.134e-2 at n = 4097 with 98.57 % of the outputs within
# 2^-10 relative (2.1e-5 and 100 % at n = 33); B = 1.5 x 1.134e-2, below the 6e-2 ceiling
B = 1.7e-2

def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))

def e4m3(x):  # RNE onto OCP e4m3fn of |x| <= 448 (vectorised orc.e4m3)
    a = np.abs(np.asarray(x, np.float64))
    quantum = np.ldexp(1.0, np.maximum(np.frexp(a)[1] - 1, -6) - 3)
    return np.copysign(np.rint(a / quantum) * quantum, x)

def model(orc, p, q):
    p = np.asarray(p, np.float32)
    x = orc.encode(q).astype(np.float16).astype(np.float64)
    w0 = p[:OFFS[1]].reshape(64, 80).astype(np.float16).astype(np.float64)
    a = (x @ w0.T).astype(np.float32)
    for l in range(1, 6):
        w = p[OFFS[l]:OFFS[l + 1]].reshape(SHAPES[l]).astype(np.float64)
        ex = np.array([orc.fp8_row_exponent(float(m)) for m in np.abs(w).max(axis=1)])[:, None]
        wq = np.ldexp(e4m3(np.ldexp(w, -ex)), ex)
        a = (e4m3(np.clip(a, 0.0, 448.0)) @ wq.T).astype(np.float32)
    return np.maximum(a[:, :3], 0.0).astype(np.float16).astype(np.float32)

@pytest.fixture()
def net8(nrc, dev):
    import torch
    enc = nrc.InputEncoding.Frequency
    net = nrc.Network()
    net.init(stream=torch.cuda.current_stream(), encoding=enc,
             config=nrc.default_config(enc, infer_precision=nrc._lib.PRECISION_FP8))
    yield net
    net.destroy()

def run(net, dev, q, precision=None, offset=0):
    import torch  # the records start `offset` floats into their buffer; the rows past n must stay untouched
    n = len(q)
    buf = torch.zeros(n * 15 + offset, device=dev)
    buf[offset:] = _t(q, dev).reshape(-1)
    out = torch.full((n + 8, 3), 777.0, device=dev)
    if precision is None:
        net.infer(buf[offset:], out, n)
    else:
        net.infer_precision(precision, buf[offset:], out, n)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[n:] == 777.0).all(), "infer wrote past n"
    return o[:n]

def exact_queries(n, seed):
    """The encoding is exact in any f32 evaluation: positions on the 2^-12 grid (every triangle-wave octave a multiple of
    2^-11), OneBlob inputs at 2.5 (all mass in the wrap bin 3), Identity inputs on the 2^-6 grid"""
    rng = np.random.default_rng(seed)
    q = np.full((n, 15), 2.5, np.float32)
    q[:, :3] = rng.integers(0, 4096, (n, 3)) / 4096.0
    q[:, 9:] = rng.integers(0, 64, (n, 6)) / 64.0
    return q

def single_path_params():
    """Signed, scaled permutation matrices: one term per dot product"""
    rng = np.random.default_rng(3)
    p = np.zeros(OFFS[-1], np.float32)
    # W0: hidden unit r <- feature f[r], injective: 36 TriangleWave, bin 3 of the 6 OneBlob dims, 2 empty OneBlob bins,
    # 6 Identity, 14 constant ones (row 63: gain 2^9 on a constant one, saturating at 448)
    f = np.concatenate([np.arange(36), 36 + 4 * np.arange(6) + 3, [36, 40], np.arange(60, 80)])
    w0 = np.zeros((64, 80), np.float32)
    w0[np.arange(64), f] = np.exp2(rng.integers(-1, 3, 64))
    w0[63, f[63]] = 512.0
    w0[rng.choice(60, 4, replace=False)] *= -1.0
    p[:OFFS[1]] = w0.ravel()
    sat = 63  # the unit carrying the saturated value: its path keeps weight +1, so the tap reads 448 x W5's weight
    for l in range(1, 5):
        w = np.zeros((64, 64), np.float32)
        perm = rng.permutation(64)
        w[np.arange(64), perm] = np.exp2(rng.integers(-2, 3, 64))  # row scales, op_sel
        rows = rng.choice(64, 6, replace=False)
        w[rows[:4]] *= -1.0  # byte ReLU, -0 included
        w[rows[4:]] = 0.0    # row exponent 0
        w[int(np.flatnonzero(perm == sat)[0]), sat] = 1.0
        sat = int(np.flatnonzero(perm == sat)[0])
        p[OFFS[l]:OFFS[l + 1]] = w.ravel()
    return p

@pytest.mark.parametrize("n,offset", [(1, 0), (33, 1), (257, 0)])
def test_single_path_bitwise(nrc, orc, dev, net8, n, offset):
    q = exact_queries(n, 70 + n)
    p = single_path_params()
    got, want = [], []
    for j in range(22):  # W5's three rows tap hidden units 3j .. 3j + 2: every unit lies on one observed chain
        w5 = np.zeros((16, 64), np.float32)
        w5[np.arange(3), (3 * j + np.arange(3)) % 64] = [1.0, 0.5, 2.0]
        p[OFFS[5]:] = w5.ravel()
        net8.set_state(nrc.StateSlot.INFER, p)
        got.append(run(net8, dev, q, offset=offset))
        want.append(model(orc, p, q))
    want = np.stack(want)
    assert np.mean(want != 0.0) >= 1.0 / 3.0 and np.isin(want, [224.0, 448.0, 896.0]).any(), "vacuous model outputs"
    np.testing.assert_array_equal(np.stack(got), want)

def dense_params(seed, gain=1.6):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1, 1, o * i) * np.sqrt(6.0 / (o + i)) * gain for o, i in SHAPES]).astype(np.float32)

@pytest.mark.parametrize("n", [33, 4097])
def test_dense_weights(nrc, orc, dev, net8, n):
    """Measured: see B; rel-L2(FP8, F16) 0.23 / 0.24. The launcher has one launch shape: no switch to straddle."""
    p = dense_params(12)
    net8.set_state(nrc.StateSlot.INFER, p)
    q = nrc.synthetic.cornell_queries(n, seed=500 + n)
    o8, y8 = run(net8, dev, q), model(orc, p, q)
    close = float(np.mean(np.abs(o8 - y8) <= 2.0 ** -10 * np.abs(y8) + 1e-6))
    o16 = run(net8, dev, q, precision=nrc._lib.PRECISION_F16)
    print(f"n={n}: FP8 vs model rel-L2 {rel(o8, y8):.3e}, {close:.4f} within 2^-10; FP8 vs F16 {rel(o8, o16):.3e}")
    assert rel(o8, y8) <= B
    assert rel(o8, o16) >= 0.1, "the FP8 path did not run"
    np.testing.assert_array_equal(o8, run(net8, dev, q, precision=nrc._lib.PRECISION_FP8))

def test_image_follows_weights(nrc, orc, dev, net8):
    import torch
    q = nrc.synthetic.cornell_queries(4097, seed=31)
    bq, bt = nrc.synthetic.cornell_batch(nrc.BATCH_SIZE, seed=32)
    bq, bt = _t(bq, dev), _t(bt, dev)

    def check(what):
        r = rel(run(net8, dev, q), model(orc, net8.get_state(nrc.StateSlot.INFER), q))
        print(f"{what}: rel-L2 {r:.3e}")
        assert r <= B, what

    net8.set_state(nrc.StateSlot.PARAMS, dense_params(13, 1.2))
    for _ in range(3):
        net8.train(bq, bt)
    check("train")
    grad = torch.zeros(net8.grad_floats, device=dev)
    net8.train_grad(bq, bt, nrc.BATCH_SIZE, nrc.BATCH_SIZE, grad)
    net8.train_apply(grad)
    check("train_grad + train_apply")
    net8.set_state(nrc.StateSlot.INFER, dense_params(14))
    check("set_state")
    cs = torch.cuda.Stream()
    net8.setStream(cs)
    qd, out = _t(q, dev), torch.zeros((len(q), 3), device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        net8.train(bq, bt)
        net8.infer(qd, out, len(q))
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        r = rel(out.cpu().numpy(), model(orc, net8.get_state(nrc.StateSlot.INFER), q))
        print(f"graph replay {i}: rel-L2 {r:.3e}")
        assert r <= B

def test_process_frame_fused_epilogue(nrc, dev, net8):
    import torch
    F = nrc.frame
    net8.set_state(nrc.StateSlot.INFER, dense_params(15))
    f = nrc.synthetic.cornell_frame(160, 96, (8, 8), seed=11)
    S, T = f.screen_size, f.num_tiles
    cap, z = F.NUM_TRAINING_RECORDS_PER_FRAME, lambda *sh: torch.zeros(sh, device=dev)  # noqa: E731
    fb = F.FrameBuffers(_t(f.queries_inference, dev), z(S + T, 3), _t(f.last_render_throughput, dev),
                        torch.full((S, 4), 0.25, device=dev), F.records_to_device(f.end_vertices, dev),
                        F.records_to_device(np.zeros(cap, F.TRAINING_RECORD_DTYPE), dev),
                        [z(cap, 15), z(cap, 15)], [z(cap, 3), z(cap, 3)])
    F.process_frame(net8, fb, F.FrameParams(S, T, 0, F.RenderMode.Full, 3, 3, 1, train=False), loss=False)
    rad = z(S + T, 3)
    net8.infer(_t(f.queries_inference, dev), rad, S + T)
    rgba = torch.full((S, 4), 0.25, device=dev)
    F.accumulate_render_radiance(rad, _t(f.last_render_throughput, dev), rgba, S, F.RenderMode.Full, 3,
                                 stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert float(rad.abs().sum()) > 0.0
    assert torch.equal(fb.output_rgba, rgba)
    assert torch.equal(fb.results_inference[S:], rad[S:])

@pytest.mark.parametrize("encoding,padded", [("Hash", False), ("FrequencySH", False), ("Frequency", True)])
def test_refusals(nrc, dev, encoding, padded):
    import torch
    enc = getattr(nrc.InputEncoding, encoding)
    cfg = nrc.default_config(enc, infer_precision=nrc._lib.PRECISION_FP8)
    cfg.query_layout = nrc.QUERY_PADDED if padded else nrc.QUERY_COMPACT
    net = nrc.Network()
    with pytest.raises(nrc.NrcError, match="FP8 inference at width 64"):
        net.init(stream=torch.cuda.current_stream(), encoding=enc, config=cfg)
    net.destroy()
