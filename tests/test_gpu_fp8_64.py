"""FP8 (e4m3 MX MFMA) inference of the 64-wide Frequency network (nrc_infer8.hip, DESIGN.md §12 "Width 64") against a
float64 numpy model of its contract: layer 0 f16 x f16; ReLU outputs of layers 0..4 clamped to [0, 448] and rounded (RNE)
onto e4m3; W1..W5 e4m3 with one power-of-two scale per row; f32 pre-activations; output through f16. Single-term weights:
bitwise. Dense weights: the MX MFMA's block sum is not f32-exact (<= 2.2e-5 sum|a b|), so a pre-activation near an e4m3
boundary can land one step away: rel-L2(GPU, model) <= B = 1.5 x the first GPU measurement (ceiling 6e-2).

Also pinned, all bitwise:
- the persistent loop's steady state (test_persistent_loop_*): 786,469 queries, at least two tile groups per wave at the
  highest residency a CU allows, as a small base block tiled to that size -- against the model (single-term weights) and
  against the base block's own launch (dense weights);
- the fused accumulate epilogue (test_infer_accumulate_fp8_bitwise): RenderMode Full and CacheOnly, tiles that straddle
  n_acc, n_acc = 0 and n_acc = n, and inside the steady-state loop, against infer + accumulate_render_radiance;
- pack8_kernel's row rules (test_pack_row_rules_bitwise), observed through single-term dot products: the row exponent
  at amax = 448 x 2^k and one float above, RNE ties, e4m3 subnormals and underflow of weights small beside their row's
  maximum, the sign, the clamp of the exponent to the E8M0 range, in W1..W4 and in W5;
- the debug library's two-tiles-per-wave shape against the product shape (test_two_tile_variant_bitwise), an odd tile
  count included; the product library's refusal of it;
- non-finite queries stay in their own columns; the per-call stream of infer()."""
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

# ---- the persistent loop's steady state: a launch larger than every wave's first tile group
N_BIG, N_BASE = 3 * 2 ** 18 + 37, 4099  # the base block is odd: no two tiles of the tiled launch hold the same rows
_SHARED = {}

def big_n(dev):
    """N_BIG, or more where it takes more for two tile groups per wave: a CU holds 2048 threads, i.e. at most two
    1024-thread blocks of 16 waves, and launch8 starts no more than CUs x resident blocks"""
    import torch
    waves = 2 * 16 * torch.cuda.get_device_properties(dev).multi_processor_count
    n = N_BIG
    while -(-n // 32) <= 2 * waves:
        n += 2 ** 18
    assert -(-n // 32) > 2 * waves
    return n

def tiled(a, n):
    return a[np.arange(n) % len(a)]

def rows_vary(y):  # a tile's rows are not its neighbours': a wrong tile index cannot pass
    return np.mean((y[:-32] != y[32:]).any(axis=1)) >= 0.9

def loop_single_path(orc):
    """(base queries, params, model outputs): single_path_params with the W5 tap set whose outputs vary most"""
    if "single" not in _SHARED:
        q, p, best = exact_queries(N_BASE, 91), single_path_params(), None
        for j in range(22):
            w5 = np.zeros((16, 64), np.float32)
            w5[np.arange(3), (3 * j + np.arange(3)) % 64] = [1.0, 0.5, 2.0]
            p[OFFS[5]:] = w5.ravel()
            want = model(orc, p, q)
            distinct = len(np.unique(want, axis=0))
            if np.mean(want != 0.0) >= 1.0 / 3.0 and (best is None or distinct > best[0]):
                best = (distinct, p.copy(), want)
        _SHARED["single"] = (q, best[1], best[2])
    return _SHARED["single"]

@pytest.mark.parametrize("offset", [0, 1])
def test_persistent_loop_single_path_bitwise(nrc, orc, dev, net8, offset):
    n = big_n(dev)
    q, p, want = loop_single_path(orc)
    assert np.mean(want != 0.0) >= 1.0 / 3.0 and rows_vary(want), "vacuous model outputs"
    net8.set_state(nrc.StateSlot.INFER, p)
    np.testing.assert_array_equal(run(net8, dev, tiled(q, n), offset=offset), tiled(want, n))

def test_persistent_loop_dense_chunk_independence(nrc, dev, net8):
    """Each query is its own MFMA column: the large launch is the base block's own launch (bounded by B against the
    model in test_dense_weights), tiled"""
    n = big_n(dev)
    net8.set_state(nrc.StateSlot.INFER, dense_params(12))
    q = nrc.synthetic.cornell_queries(N_BASE, seed=77)
    base = run(net8, dev, q)
    assert rows_vary(base), "vacuous outputs"
    np.testing.assert_array_equal(run(net8, dev, tiled(q, n)), tiled(base, n))

@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("n,n_acc", [(100_003, 90_001), (4096, 4096), (777, 0), (33, 1), (N_BIG, 700_001)])
def test_infer_accumulate_fp8_bitwise(nrc, dev, net8, mode, n, n_acc):
    """Fused epilogue of the FP8 kernel == its infer + nrc_accumulate_render_radiance, bit for bit (w = 1/6); render
    radiance is not written, train-suffix radiance is, the frame buffer past n_acc is left alone. The last case runs
    the epilogue's prefetched operands inside the steady-state loop."""
    import torch
    F = nrc.frame
    net8.set_state(nrc.StateSlot.INFER, dense_params(15))
    if n == N_BIG:
        n = big_n(dev)
        q = tiled(nrc.synthetic.cornell_queries(N_BASE, seed=78), n)
    else:
        q = nrc.synthetic.cornell_queries(n, seed=n)
    q = _t(q, dev)
    rng = np.random.default_rng(n_acc)
    thr = _t(rng.uniform(0, 1, (max(n_acc, 1), 3)).astype(np.float32), dev)
    rgba0 = _t(rng.uniform(0, 1, (n_acc + 8, 4)).astype(np.float32), dev)
    ref_res = torch.empty((n, 3), device=dev)
    net8.infer(q, ref_res, n)
    ref_rgba = rgba0.clone()
    F.accumulate_render_radiance(ref_res, thr, ref_rgba, n_acc, mode, 5)
    res = torch.full((n, 3), -3.0, device=dev)
    rgba = rgba0.clone()
    F.infer_accumulate(net8, q, res, n, thr, rgba, n_acc, mode, 5)
    torch.cuda.synchronize()
    assert float(ref_res.abs().sum()) > 0.0
    assert n_acc == 0 or not torch.equal(ref_rgba[:n_acc, :3], rgba0[:n_acc, :3]), "vacuous accumulation"
    assert torch.equal(rgba, ref_rgba)
    assert torch.equal(rgba[n_acc:], rgba0[n_acc:])
    assert torch.equal(res[n_acc:], ref_res[n_acc:])
    assert torch.all(res[:n_acc] == -3.0)
    with pytest.raises(nrc.NrcError):
        F.infer_accumulate(net8, q, res, n, thr, rgba, n_acc, F.RenderMode.DebugThroughputOnly, 0)

# ---- pack8_kernel's row rules. The pack image cannot be read back: a row under test has weight v on a live unit (a
# constant-one feature times a power of two, act) and weight M on a dead unit (an empty OneBlob bin: exactly +0), so M
# sets the row exponent and the dot product keeps one term; identity weights carry act x quantised(v) to the output.
def probe_params(layer, rows):
    """rows: three (v, M, act), or (v, None, act) for v in every column; chain c lives on unit u[c] of every layer"""
    u, d = (layer, 29 + layer, 58 + layer), 40 + layer
    p = np.zeros(OFFS[-1], np.float32)
    w0 = np.zeros((64, 80), np.float32)
    w0[u, 66 + np.arange(3)] = [act for _, _, act in rows]
    w0[d, 36] = 1.0
    p[:OFFS[1]] = w0.ravel()
    for l in range(1, 6):
        w = np.zeros(SHAPES[l], np.float32)
        for c, (v, M, _) in enumerate(rows):
            r = c if l == 5 else u[c]
            if l != layer:
                w[r, u[c]] = 1.0
            elif M is None:
                w[r] = v
            else:
                w[r, u[c]], w[r, d] = v, M
        p[OFFS[l]:OFFS[l + 1]] = w.ravel()
    return p

def pack_cases():
    """(group, v, M, act, expected output), worked by hand: e = the row exponent of M, the output act x RNE_e4m3(v /
    2^e) x 2^e. act keeps that value a normal e4m3 number, so the later layers and the f16 output pass it on exactly."""
    f32, up = np.float32, lambda x: np.nextafter(np.float32(x), np.float32(np.inf))  # noqa: E731
    cases = []
    for k, act in ((-3, 256.0), (0, 64.0), (2, 64.0)):
        s, m = 2.0 ** k, f32(448.0 * 2.0 ** k)
        # amax = 448 x 2^k: e = k; one float above: e = k + 1. Normal e4m3 numbers scale with e: 17 -> 16, 8.5 -> 8 (ties
        # to even), the same value. The two exponents differ only below 2^-6: 3 x 2^-9 is an exact subnormal under
        # e = k, and the tie 1.5 x 2^-9 -> 2 x 2^-9 under e = k + 1
        cases += [("boundary", 17.0 * s, m, 1.0, 16.0 * s), ("boundary", 17.0 * s, up(m), 1.0, 16.0 * s),
                  ("boundary", 3.0 * s / 512.0, m, act, act * 3.0 * s / 512.0),
                  ("boundary", 3.0 * s / 512.0, up(m), act, act * 4.0 * s / 512.0)]
    cases += [("tie", 17.0, 448.0, 1.0, 16.0), ("tie", 19.0, 448.0, 1.0, 20.0), ("tie", up(17.0), 448.0, 1.0, 18.0)]
    cases += [("subnormal", k / 512.0, 448.0, 64.0, k / 8.0) for k in range(1, 8)]
    cases += [("subnormal", 1.5 / 512.0, 448.0, 64.0, 0.25), ("subnormal", 2.5 / 512.0, 448.0, 64.0, 0.25),
              ("subnormal", 0.5 / 512.0, 448.0, 64.0, 0.0), ("subnormal", 0.75 / 512.0, 448.0, 64.0, 0.125),
              ("subnormal", 2.0 ** -11, 448.0, 64.0, 0.0)]
    cases += [("sign", -v, M, act, 0.0) for g, v, M, act, _ in cases]
    # e clamps to -127 (1e-40 is an f32 denormal: frexp gives e = -141); 3e38 = 0.88 x 2^128: e = 120, under which 1 is
    # flushed and 2^114 = 2^-6 x 2^120 is the smallest normal (the pre-activation 2^114 saturates at 448)
    cases += [("clamp", 1e-40, None, 1.0, 0.0), ("clamp", 1.0, 3e38, 1.0, 0.0), ("clamp", 2.0 ** 114, 3e38, 1.0, 448.0)]
    return cases

@pytest.mark.parametrize("layer", [1, 2, 3, 4, 5])
def test_pack_row_rules_bitwise(nrc, orc, dev, net8, layer):
    """layer 5: W5, whose fragment uses scale byte 0 only; its three rows carry three different exponents at once. W5's
    output is not clamped, so 2^114 (inf in f16) is left to the hidden layers. Rows 3..31 of W5's fragment reach no
    output and cannot be observed."""
    cases = [c for c in pack_cases() if layer < 5 or c[4] <= 448.0 and c[1] < 2.0 ** 100]
    cases += [("fill", 1.0, 448.0, 1.0, 1.0)] * (-len(cases) % 3)
    q = exact_queries(5, 17)
    for i in range(0, len(cases), 3):
        trio = cases[i:i + 3]
        p = probe_params(layer, [(v, M, act) for _, v, M, act, _ in trio])
        net8.set_state(nrc.StateSlot.INFER, p)
        got, want = run(net8, dev, q), model(orc, p, q)
        hand = np.tile(np.float32([c[4] for c in trio]), (len(q), 1))
        np.testing.assert_array_equal(want, hand, err_msg=f"the probe does not carry {trio} to the output")
        assert np.isfinite(got).all(), trio
        np.testing.assert_array_equal(got, want, err_msg=f"layer {layer}: {trio}")
    for group in ("boundary", "tie", "subnormal"):
        assert any(c[0] == group and c[4] != 0.0 for c in cases), group

# ---- the debug library's two-tiles-per-wave shape (launch8<-1, 2, 512>)
def test_two_tile_variant_bitwise(nrc, dev, net8):
    """Two tiles per wave iteration == the product shape, bit for bit; with an odd tile count (n = 1, 33, 65, 4097) the
    second tile of the last group lies wholly past n. Debug library only (tests/test_gpu_debug_lib.py runs it there)."""
    if not nrc._lib.is_debug_library():
        pytest.skip("A/B variant of the debug library (libnrc_amd_debug.so)")
    net8.set_state(nrc.StateSlot.INFER, dense_params(16))
    base = nrc.synthetic.cornell_queries(N_BASE, seed=79)
    for n in (1, 33, 65, 4097, big_n(dev)):
        q = tiled(base, n)
        one = run(net8, dev, q, precision=nrc._lib.PRECISION_FP8)
        assert n < 33 or rows_vary(one), "vacuous outputs"
        np.testing.assert_array_equal(run(net8, dev, q, precision=nrc._lib.PRECISION_FP8 | (1 << 4)), one, err_msg=str(n))

def test_two_tile_variant_refused_by_product_library(nrc, dev, net8):
    if nrc._lib.is_debug_library():
        return
    with pytest.raises(nrc.NrcError, match="debug library"):
        run(net8, dev, nrc.synthetic.cornell_queries(33, seed=80), precision=nrc._lib.PRECISION_FP8 | (1 << 4))

# ---- small things
def test_non_finite_queries_stay_in_their_columns(nrc, dev, net8):
    net8.set_state(nrc.StateSlot.INFER, dense_params(17))
    q = nrc.synthetic.cornell_queries(33, seed=81)
    bad = q.copy()
    bad[5] = np.nan
    bad[20, 1] = np.inf
    import domain_cases as dc  # NaN, +-inf and 1e30 per field class, in the first tile and the ragged last one
    h = dc.hostile_rows()
    rows = np.array([0, 2, 4, 7, 9, 12, 15, 19, 23, 27, 30, 31, 32])
    bad[rows] = h[np.arange(len(rows)) * 2 % len(h)]
    keep = np.setdiff1d(np.arange(33), np.concatenate([rows, [5, 20]]))
    np.testing.assert_array_equal(run(net8, dev, bad)[keep], run(net8, dev, q)[keep])

def test_infer_on_a_side_stream(nrc, dev, net8):
    """infer(stream=) (nrc_infer_stream) after a train on the handle's own stream: the training step's weights and its
    FP8 repack are ordered before the side stream's launch by an event, nothing else"""
    import torch
    net8.set_state(nrc.StateSlot.PARAMS, dense_params(18, 1.2))
    bq, bt = nrc.synthetic.cornell_batch(nrc.BATCH_SIZE, seed=33)
    bq, bt = _t(bq, dev), _t(bt, dev)
    n = 4097
    q = _t(nrc.synthetic.cornell_queries(n, seed=82), dev)
    out, ref = torch.full((n + 8, 3), 777.0, device=dev), torch.empty((n, 3), device=dev)
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    before = net8.get_state(nrc.StateSlot.INFER)
    net8.train(bq, bt)
    done = torch.cuda.Event()
    done.record(main)
    side.wait_event(done)
    net8.infer(q, out, n, stream=side)
    side.synchronize()
    net8.setStream(main)
    net8.infer(q, ref, n)
    torch.cuda.synchronize()
    assert not np.array_equal(before, net8.get_state(nrc.StateSlot.INFER)), "the step changed nothing"
    assert torch.equal(out[:n], ref) and torch.all(out[n:] == 777.0)
    assert float(ref.abs().sum()) > 0.0
