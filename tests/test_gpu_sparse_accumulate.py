"""nrc_infer_accumulate_sparse (csrc/nrc_infer_sparse.hip, include/nrc/frame.h): fused inference + accumulation that
skips the network for render queries whose throughput is exactly zero. The reference is the dense path, code that is
not under test here (net.infer + accumulate_render_radiance, as test_infer_accumulate_fused_bitwise); "equal" is equality
of the bit patterns (int32 views), so -0 / +0 and NaN payloads count."""
import numpy as np
import pytest

from test_gpu_frame import _device_frame, _t
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

BIG = (2_073_600 + 32_400, 2_073_600)  # the 1080p frame: pixels + train tiles
# name -> (dead mask over p pixels, the dead count the name promises)
MASKS = {
    "none": (lambda p: np.zeros(p, bool), lambda p: 0),
    "all": (lambda p: np.ones(p, bool), lambda p: p),
    "alternating": (lambda p: np.arange(p) % 2 == 1, lambda p: p // 2),
    "one_live_in_33": (lambda p: np.arange(p) % 33 != 0, lambda p: p - (p + 32) // 33),
    "random_half": (lambda p: np.random.default_rng(p).permutation(p) < p // 2, lambda p: p // 2),
    "runs_1000": (lambda p: (np.arange(p) // 1000) % 2 == 1, lambda p: p // 2000 * 1000 + max(0, p % 2000 - 1000)),
}
SMALL = [(1, 1), (33, 33), (777, 0), (4096, 4096), (100_003, 90_001)]
CASES = [(n, p, m) for n, p in SMALL for m in MASKS] + [BIG + ("one_live_in_33",), BIG + ("random_half",)]


@pytest.fixture(scope="module")
def net(nrc, dev):
    import torch
    n = nrc.Network()
    n.init(stream=torch.cuda.current_stream())
    yield n
    n.destroy()


def _case(nrc, dev, n, npix, mask):
    """Queries, throughput (zero rows where the mask is dead) and a random frame buffer with one guard row."""
    dead = MASKS[mask][0](npix)
    assert int(dead.sum()) == MASKS[mask][1](npix) and dead.size == npix
    rng = np.random.default_rng(n + npix)
    thr = rng.uniform(0.05, 1, (npix + 1, 3)).astype(np.float32)
    thr[:npix][dead] = 0.0
    rgba0 = rng.uniform(0, 1, (npix + 1, 4)).astype(np.float32)
    return _t(nrc.synthetic.cornell_queries(n, seed=n), dev), _t(thr, dev), _t(rgba0, dev)


def _dense_and_sparse(nrc, dev, net, q, thr, rgba0, n, npix, mode):
    import torch
    F = nrc.frame
    ref_res = torch.empty((n, 3), device=dev)
    net.infer(q, ref_res, n)
    ref_rgba = rgba0.clone()
    F.accumulate_render_radiance(ref_res, thr, ref_rgba, npix, mode, 5)
    res = torch.full((n + 1, 3), -3.0, device=dev)
    rgba = rgba0.clone()
    F.infer_accumulate_sparse(net, q, res, n, thr, rgba, npix, mode, 5)
    torch.cuda.synchronize()
    # a default-initialised network on cornell_queries stays finite: if this trips, the inputs are wrong
    assert torch.isfinite(ref_res[:npix]).all()
    return ref_res, ref_rgba, res, rgba


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("n,npix,mask", CASES)
def test_sparse_bitwise_vs_dense(nrc, dev, net, n, npix, mask, mode):
    import torch
    if (n, npix) == BIG:  # every block walks >= 2 chunks (with carry between them), even at two blocks per CU
        assert n // (2 * torch.cuda.get_device_properties(dev).multi_processor_count) > nrc.frame.SPARSE_CHUNK
    q, thr, rgba0 = _case(nrc, dev, n, npix, mask)
    ref_res, ref_rgba, res, rgba = _dense_and_sparse(nrc, dev, net, q, thr, rgba0, n, npix, mode)
    i32 = torch.int32
    assert torch.equal(rgba[:npix].view(i32), ref_rgba[:npix].view(i32))
    assert torch.equal(res[npix:n].view(i32), ref_res[npix:].view(i32))
    assert torch.all(res[:npix] == -3.0)
    assert torch.all(res[n] == -3.0) and torch.equal(rgba[npix], rgba0[npix])  # guard rows


def test_sparse_special_values(nrc, dev, net):
    """Dead pixels with signed zeros in T and dst; T = (NaN, 0, 0) and T = (0, 0, 1e-38) are live."""
    import torch
    n = 257
    q, thr, rgba0 = _case(nrc, dev, n, n, "alternating")
    thr[3] = torch.tensor([-0.0, 0.0, -0.0])
    rgba0[3] = torch.tensor([0.0, -0.0, 0.0, 0.5])
    thr[5] = torch.tensor([0.0, -0.0, 0.0])
    rgba0[5] = torch.tensor([-0.0, -0.0, -0.0, 0.5])
    thr[101] = torch.tensor([float("nan"), 0.0, 0.0])
    thr[201] = torch.tensor([0.0, 0.0, 1e-38])
    _, ref_rgba, res, rgba = _dense_and_sparse(nrc, dev, net, q, thr, rgba0, n, n, 0)
    assert torch.equal(rgba.view(torch.int32), ref_rgba.view(torch.int32))
    assert torch.isnan(rgba[101, 0]) and torch.all(res == -3.0)


def test_sparse_vs_oracle(nrc, orc, dev, net):
    """Frame buffer against the CPU oracle's inference + accumulate, at test_gpu_parity's f16-vs-ORC_MIXED tolerance."""
    import torch
    n, npix = 4097, 4000
    q, thr, rgba0 = _case(nrc, dev, n, npix, "random_half")
    rgba = rgba0.clone()
    nrc.frame.infer_accumulate_sparse(net, q, torch.empty((n, 3), device=dev), n, thr, rgba, npix, 0, 5)
    torch.cuda.synchronize()
    y = orc.forward(net.get_state(nrc.StateSlot.INFER), q.cpu().numpy(), orc.MIXED)
    want = orc.accumulate(y[:npix], thr[:npix].cpu().numpy(), rgba0[:npix].cpu().numpy(), 0, 5)
    assert rel(rgba[:npix].cpu().numpy(), want) <= 1e-3


@pytest.mark.parametrize("mode", [0, 2])
def test_frame_sparse_knob(nrc, dev, mode):
    """process_frame with knob frame_sparse = 1 == the dense frame, bitwise (frame buffer and train-suffix radiance)."""
    import torch
    F = nrc.frame
    f = nrc.synthetic.cornell_frame(160, 96, (8, 8))
    assert (f.last_render_throughput == 0).all(axis=1).any()
    out = []
    try:
        for knob in (1, -1):
            nrc._lib.set_knob("frame_sparse", knob)
            net = nrc.Network()
            net.init(stream=torch.cuda.current_stream())
            fb, *_ = _device_frame(nrc, f, dev)
            fb.output_rgba.uniform_(0, 1, generator=torch.Generator(dev).manual_seed(3))
            F.process_frame(net, fb, F.FrameParams(f.screen_size, f.num_tiles, 0, mode, iteration_index=2), loss=False)
            torch.cuda.synchronize()
            out.append((fb.output_rgba.view(torch.int32), fb.results_inference[f.screen_size:].view(torch.int32)))
            net.destroy()
    finally:
        nrc._lib.set_knob("frame_sparse", -1)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("what,enc,kw,padded,mode,status", [
    ("FP8", "Frequency", {"infer_precision": "PRECISION_FP8"}, False, 0, 5),
    ("Hash", "Hash", {}, False, 0, 5),
    ("FrequencySH", "FrequencySH", {}, False, 0, 5),
    ("padded", "Frequency", {}, True, 0, 5),
    ("F16_ACC16", "Frequency", {"infer_precision": "PRECISION_F16_ACC16"}, False, 0, 5),
    ("128", "Frequency", {"width": 128}, False, 0, 5),
    ("Full and CacheOnly", "Frequency", {}, False, 5, 1)])
def test_sparse_refusals(nrc, dev, what, enc, kw, padded, mode, status):
    import torch
    enc = getattr(nrc.InputEncoding, enc)
    cfg = nrc.default_config(enc, **{k: getattr(nrc._lib, v) if isinstance(v, str) else v for k, v in kw.items()})
    cfg.query_layout = nrc.QUERY_PADDED if padded else nrc.QUERY_COMPACT
    net = nrc.Network()
    net.init(stream=torch.cuda.current_stream(), encoding=enc, config=cfg)
    buf = torch.zeros((32, 16), device=dev)
    with pytest.raises(nrc.NrcError, match=what) as e:
        nrc.frame.infer_accumulate_sparse(net, buf, buf, 32, buf, buf, 32, mode, 0)
    assert e.value.status == status
    net.destroy()
