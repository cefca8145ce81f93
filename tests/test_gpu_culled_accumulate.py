"""nrc_infer_accumulate_culled (csrc/nrc_infer_culled.hip, include/nrc/frame.h): fused accumulation that culls the
zero-throughput render queries before the network runs, on F16 and FP8 handles, plain or reflectance-factored. The
reference is the dense entry on the same handle (nrc_infer_accumulate / nrc_infer_accumulate_factored); "equal" is
equality of the bit patterns (int32 views). Queries are the synthetic Cornell stream (reflectance in [0, 1], finite
radiance), so the dead-pixel equality of the contract holds for every row."""
import numpy as np
import pytest

from oracle import oracle_np
from test_gpu_frame import _device_frame, _t
from test_gpu_fp8_64 import B as FP8_BOUND
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

BIG = (20011, 20088)  # 10 classify segments of 2,048 pixels, more tiles than one block's first draw
DEAD = {  # dead mask over p pixels
    "all_live": lambda p: np.zeros(p, bool),
    "all_dead": lambda p: np.ones(p, bool),
    "alternating": lambda p: np.arange(p) % 2 == 1,
    "random_half": lambda p: np.random.default_rng(p).permutation(p) < p // 2,
    "first_9000_dead": lambda p: np.arange(p) < 9000,  # whole empty segments
    "last_live": lambda p: np.arange(p) != p - 1,
}
CASES = [(0, 33, "alternating"), (1, 1, "all_live"), (1, 1, "all_dead"), (31, 31, "alternating"),
         (33, 40, "alternating")] + [BIG + (m,) for m in DEAD]
PRECISIONS = ["PRECISION_F16", "PRECISION_FP8"]


def _make(nrc, precision, **kw):
    import torch
    enc = nrc.InputEncoding.Frequency
    net = nrc.Network()
    net.init(stream=torch.cuda.current_stream(), encoding=enc,
             config=nrc.default_config(enc, infer_precision=getattr(nrc._lib, precision), **kw))
    return net


@pytest.fixture(scope="module")
def nets(nrc, dev):
    made = {p: _make(nrc, p) for p in PRECISIONS}
    yield made
    for n in made.values():
        n.destroy()


def _case(nrc, dev, npix, n, mask):
    """Queries, throughput (zero rows where the mask is dead) and a random frame buffer, each with one guard row."""
    rng = np.random.default_rng(n + npix)
    thr = rng.uniform(0.05, 1, (npix + 1, 3)).astype(np.float32)
    thr[:npix][DEAD[mask](npix)] = 0.0
    rgba0 = rng.uniform(0, 1, (npix + 1, 4)).astype(np.float32)
    return _t(nrc.synthetic.cornell_queries(n, seed=n), dev), _t(thr, dev), _t(rgba0, dev)


def _check_bitwise(nrc, dev, net, q, thr, rgba0, npix, n, mode, rf):
    import torch
    F = nrc.frame
    ref_res, ref_rgba = torch.full((n + 1, 3), -3.0, device=dev), rgba0.clone()
    (F.infer_accumulate_factored if rf else F.infer_accumulate)(net, q, ref_res, n, thr, ref_rgba, npix, mode, 5)
    res, rgba = torch.full((n + 1, 3), -3.0, device=dev), rgba0.clone()
    F.infer_accumulate_culled(net, q, res, n, thr, rgba, npix, mode, 5, rf)
    torch.cuda.synchronize()
    i32 = torch.int32
    assert torch.equal(rgba.view(i32), ref_rgba.view(i32))  # the guard row past num_pixels included
    assert torch.equal(res[npix:n].view(i32), ref_res[npix:n].view(i32))
    assert torch.all(res[:npix] == -3.0) and torch.all(res[n] == -3.0)
    return rgba


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("rf", [0, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("npix,n,mask", CASES)
def test_culled_bitwise_vs_dense(nrc, dev, nets, npix, n, mask, precision, rf, mode):
    _check_bitwise(nrc, dev, nets[precision], *_case(nrc, dev, npix, n, mask), npix, n, mode, rf)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_culled_workspace_growth(nrc, dev, precision):
    """A fresh handle: the first call allocates the workspace, a second call with more pixels grows it."""
    net = _make(nrc, precision)
    for npix, n in [(33, 40), BIG]:
        _check_bitwise(nrc, dev, net, *_case(nrc, dev, npix, n, "random_half"), npix, n, 0, 1)
    net.destroy()


@pytest.mark.parametrize("rf", [0, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_culled_special_throughputs(nrc, dev, nets, precision, rf):
    """(-0, +0, 0) is dead; one NaN component and (0, 0, 2^-149) are live."""
    import torch
    npix, n = 33, 40
    q, thr, rgba0 = _case(nrc, dev, npix, n, "alternating")
    thr[2] = torch.tensor([-0.0, 0.0, 0.0])
    rgba0[2] = torch.tensor([0.0, -0.0, 0.25, 0.5])
    thr[4] = torch.tensor([float("nan"), 0.0, 0.0])
    thr[6] = torch.tensor([0.0, 0.0, 2.0 ** -149])
    rgba = _check_bitwise(nrc, dev, nets[precision], q, thr, rgba0, npix, n, 0, rf)
    assert torch.isnan(rgba[4, 0]) and torch.equal(rgba[2, :3], rgba0[2, :3])


@pytest.mark.parametrize("rf", [0, 1])
@pytest.mark.parametrize("precision,bound", [("PRECISION_F16", 1e-3), ("PRECISION_FP8", FP8_BOUND)])
def test_culled_vs_float64(nrc, dev, nets, precision, bound, rf):
    """Frame buffer (Full, w = 1/6) against oracle_np's float64 radiance and the contract's formulas; bounds: F16 the
    rel-L2 of test_gpu_parity, FP8 the B of test_gpu_fp8_64."""
    import torch
    npix, n, net = 33, 40, nets[precision]
    q, thr, rgba0 = _case(nrc, dev, npix, n, "alternating")
    rgba = rgba0.clone()
    nrc.frame.infer_accumulate_culled(net, q, torch.empty((n, 3), device=dev), n, thr, rgba, npix, 0, 5, rf)
    torch.cuda.synchronize()
    qn = q.cpu().numpy().astype(np.float64)
    L = oracle_np.forward(net.get_state(nrc.StateSlot.INFER), qn)[0][:npix, :3]
    T, want = thr[:npix].cpu().numpy().astype(np.float64), rgba0[:npix].cpu().numpy().astype(np.float64)
    R = qn[:npix, 9:12] + qn[:npix, 12:15] if rf else 1.0
    want[:, :3] += np.where((T == 0).all(axis=1, keepdims=True), T * 0.0, T * L * R) / 6.0
    want[:, 3] = 1.0
    got = rel(rgba[:npix].cpu().numpy(), want)
    print(f"{precision} rf={rf}: rel-L2 {got:.3e} (bound {bound:.1e})")
    assert got <= bound


@pytest.mark.parametrize("rf", [0, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_frame_culled_knob(nrc, dev, precision, rf):
    """process_frame (Full, train = 1) with knob frame_culled = 1 == the knob off, bitwise."""
    import torch
    F = nrc.frame
    f = nrc.synthetic.cornell_frame(160, 96, (8, 8))
    S = f.screen_size
    assert (f.last_render_throughput == 0).all(axis=1).any()
    out = []
    try:
        for knob in (1, -1):
            nrc._lib.set_knob("frame_culled", knob)
            net = _make(nrc, precision)
            fb, *_ = _device_frame(nrc, f, dev)
            fb.output_rgba.uniform_(0, 1, generator=torch.Generator(dev).manual_seed(3))
            fb.results_inference.fill_(-3.0)
            F.process_frame(net, fb, F.FrameParams(S, f.num_tiles, f.num_training_records, 0, iteration_index=2,
                                                   reflectance_factoring=bool(rf)), loss=False)
            torch.cuda.synchronize()
            out.append([t.clone().view(torch.int32) for t in
                        (fb.output_rgba, fb.results_inference[S:], fb.train_targets[0])])
            assert knob != 1 or torch.all(fb.results_inference[:S] == -3.0)
            net.destroy()
    finally:
        nrc._lib.set_knob("frame_culled", -1)
    assert all(torch.equal(a, b) for a, b in zip(*out))


@pytest.mark.parametrize("what,enc,kw,padded,mode,n,status", [
    ("Hash", "Hash", {}, False, 0, 32, 5),
    ("FrequencySH", "FrequencySH", {}, False, 0, 32, 5),
    ("padded", "Frequency", {}, True, 0, 32, 5),
    ("F16_ACC16", "Frequency", {"infer_precision": "PRECISION_F16_ACC16"}, False, 0, 32, 5),
    ("128", "Frequency", {"width": 128}, False, 0, 32, 5),
    ("Full and CacheOnly", "Frequency", {}, False, 4, 32, 1),
    ("Full and CacheOnly", "Frequency", {}, False, 5, 32, 1),
    ("n must be", "Frequency", {}, False, 0, 2 ** 26 + 1, 1)])
def test_culled_refusals(nrc, dev, what, enc, kw, padded, mode, n, status):
    import torch
    enc = getattr(nrc.InputEncoding, enc)
    cfg = nrc.default_config(enc, **{k: getattr(nrc._lib, v) if isinstance(v, str) else v for k, v in kw.items()})
    cfg.query_layout = nrc.QUERY_PADDED if padded else nrc.QUERY_COMPACT
    net = nrc.Network()
    net.init(stream=torch.cuda.current_stream(), encoding=enc, config=cfg)
    buf = torch.zeros((32, 16), device=dev)
    with pytest.raises(nrc.NrcError, match=what) as e:
        nrc.frame.infer_accumulate_culled(net, buf, buf, n, buf, buf, 32, mode, 0)
    assert e.value.status == status
    net.destroy()


def test_frame_culled_knob_range(nrc):
    with pytest.raises(nrc.NrcError) as e:
        nrc._lib.set_knob("frame_culled", 2)
    assert e.value.status == 1 and nrc._lib.get_knob("frame_culled") == -1
