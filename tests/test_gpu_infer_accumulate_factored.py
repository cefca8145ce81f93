"""nrc_infer_accumulate_factored (csrc/nrc_infer_factored.hip, the factored EPI values of csrc/nrc_infer8.hip,
include/nrc/frame.h): inference with the reflectance-factored accumulation in its epilogue, and the frame driver's knob
"frame_factored_fused". References: the unfused pair (net.infer + accumulate_render_radiance_factored, kernels not under
test here) and the CPU oracle's factored accumulate; "equal" is equality of bit patterns."""
import numpy as np
import pytest

from test_gpu_frame import _device_frame, _t

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (33, 0), (97, 33), (97, 97), (4099, 4001)]  # one row, no pixels, inside a tile, all pixels, odd tail
IT = 5


@pytest.fixture(scope="module", params=["PRECISION_F16", "PRECISION_FP8"])
def net(request, nrc, orc, dev):
    import torch
    enc = nrc.InputEncoding.Frequency
    n = nrc.Network()
    n.init(stream=torch.cuda.current_stream(), encoding=enc,
           config=nrc.default_config(enc, infer_precision=getattr(nrc._lib, request.param)))
    n.set_state(nrc.StateSlot.INFER, orc.init_params(1337) * np.float32(1.6))  # dense weights: non-trivial radiance
    yield n
    n.destroy()


def _case(nrc, dev, n, npix, base=None, offset=0):
    """Cornell queries whose diffuse / specular (floats 9..11 / 12..14) are independent seeded non-zero draws, the
    throughput and a seeded frame buffer with one guard row; the records start `offset` floats into their buffer."""
    import torch
    rng = np.random.default_rng(n + npix)
    q = nrc.synthetic.cornell_queries(base or n, seed=n)
    q[:, 9:15] = rng.uniform(0.05, 1.0, (len(q), 6))
    q = q[np.arange(n) % len(q)]  # base: an odd-sized block tiled to n
    buf = torch.zeros(n * 15 + offset, device=dev)
    buf[offset:] = _t(q, dev).reshape(-1)
    thr = rng.uniform(0.05, 1, (npix + 1, 3)).astype(np.float32)
    rgba0 = rng.uniform(0, 1, (npix + 1, 4)).astype(np.float32)
    return q, buf[offset:], _t(thr, dev), _t(rgba0, dev)


def _check(nrc, dev, net, qd, thr, rgba0, n, npix, mode):
    """Fused entry against infer + accumulate_render_radiance_factored; returns (unfused radiance, fused rgba)."""
    import torch
    F, i32 = nrc.frame, torch.int32
    T = None if mode == 4 else thr
    ref_res = torch.empty((n, 3), device=dev)
    net.infer(qd, ref_res, n)
    ref_rgba = rgba0.clone()
    F.accumulate_render_radiance_factored(ref_res, qd, T, ref_rgba, npix, mode, IT)
    res = torch.full((n + 1, 3), -3.0, device=dev)
    rgba = rgba0.clone()
    F.infer_accumulate_factored(net, qd, res, n, T, rgba, npix, mode, IT)
    torch.cuda.synchronize()
    if npix:
        assert (ref_res[:npix] != 0).any(dim=1).float().mean() > 0.5, "vacuous radiance"
    assert torch.equal(rgba[:npix].view(i32), ref_rgba[:npix].view(i32))
    assert torch.equal(res[npix:n].view(i32), ref_res[npix:].view(i32))
    assert torch.all(res[:npix] == -3.0)
    assert torch.all(res[n] == -3.0) and torch.equal(rgba[npix], rgba0[npix])  # guard rows
    return ref_res, rgba


@pytest.mark.parametrize("mode", [0, 2, 4])
@pytest.mark.parametrize("n,npix", SHAPES)
def test_factored_bitwise(nrc, orc, dev, net, n, npix, mode):
    q, qd, thr, rgba0 = _case(nrc, dev, n, npix, offset=1 if (n, npix) == (97, 33) else 0)
    ref_res, rgba = _check(nrc, dev, net, qd, thr, rgba0, n, npix, mode)
    want = orc.accumulate(ref_res[:npix].cpu().numpy(), thr[:npix].cpu().numpy(), rgba0[:npix].cpu().numpy(), mode, IT,
                          queries=q[:npix])
    np.testing.assert_array_equal(rgba[:npix].cpu().numpy().view(np.int32), want.view(np.int32))


def test_factored_steady_state_loop(nrc, dev, net):
    """Every wave owns at least two tiles at full residency: a CU holds at most two 1024-thread blocks of 16 waves."""
    import torch
    waves = 2 * 16 * torch.cuda.get_device_properties(dev).multi_processor_count
    n = 32 * 2 * waves + 4099
    assert -(-n // 32) > 2 * waves
    npix = n - 12_345
    _, qd, thr, rgba0 = _case(nrc, dev, n, npix, base=4099)
    _check(nrc, dev, net, qd, thr, rgba0, n, npix, 0)


@pytest.mark.parametrize("kind", ["full_train", "cache_first_vertex", "shard"])
def test_frame_factored_fused_knob(nrc, orc, dev, kind):
    """process_frame with knob frame_factored_fused = 1 == the unfused factored frame, bitwise; the render radiance is
    not written."""
    import torch
    F, i32 = nrc.frame, torch.int32
    f = nrc.synthetic.cornell_frame(160, 96, (8, 8))
    S = f.screen_size
    cfv = kind == "cache_first_vertex"
    fp = F.FrameParams(S, f.num_tiles, 0 if cfv else f.num_training_records,
                       F.RenderMode.CacheFirstVertex if cfv else F.RenderMode.Full, iteration_index=2, frame_index=2,
                       shuffle_seed=7, train=not cfv, reflectance_factoring=True)
    out = []
    try:
        for knob in (1, 0):
            nrc._lib.set_knob("frame_factored_fused", knob)
            net = nrc.Network()
            net.init(stream=torch.cuda.current_stream())
            for slot in (nrc.StateSlot.PARAMS, nrc.StateSlot.INFER):
                net.set_state(slot, orc.init_params(1337) * np.float32(1.6))
            fb, *_ = _device_frame(nrc, f, dev)
            fb.output_rgba.uniform_(0, 1, generator=torch.Generator(dev).manual_seed(3))
            fb.results_inference.fill_(-3.0)
            fb.results_cache_vis.fill_(-3.0)
            if kind == "shard":
                F.process_frame_shard(net, fb, fp, 1001, S - 777, loss=False)
            else:
                F.process_frame(net, fb, fp, loss=False)
            torch.cuda.synchronize()
            out.append(fb)
            net.destroy()
    finally:
        nrc._lib.set_knob("frame_factored_fused", -1)
    fused, ref = out
    rad = ref.results_cache_vis if cfv else ref.results_inference[1001:S - 777]
    assert (rad != 0).any(dim=1).float().mean() > 0.5, "vacuous radiance"
    assert torch.equal(fused.output_rgba.view(i32), ref.output_rgba.view(i32))
    assert torch.equal(fused.results_inference[S:].view(i32), ref.results_inference[S:].view(i32))
    assert torch.equal(fused.train_targets[0].view(i32), ref.train_targets[0].view(i32))
    assert torch.all(fused.results_inference[:S] == -3.0)
    assert torch.all(fused.results_cache_vis == -3.0) and (cfv or torch.all(ref.results_cache_vis == -3.0))
    assert cfv == bool(torch.any(ref.results_cache_vis != -3.0))  # the unfused frame did write what the fused one skips


@pytest.mark.parametrize("what,enc,kw,padded,mode,status", [
    ("Hash", "Hash", {}, False, 0, 5),
    ("FrequencySH", "FrequencySH", {}, False, 0, 5),
    ("padded", "Frequency", {}, True, 0, 5),
    ("F16_ACC16", "Frequency", {"infer_precision": "PRECISION_F16_ACC16"}, False, 0, 5),
    ("128", "Frequency", {"width": 128}, False, 0, 5),
    ("DebugCacheNoThroughputModulation only", "Frequency", {}, False, 5, 1)])
def test_factored_refusals(nrc, dev, what, enc, kw, padded, mode, status):
    import torch
    enc = getattr(nrc.InputEncoding, enc)
    cfg = nrc.default_config(enc, **{k: getattr(nrc._lib, v) if isinstance(v, str) else v for k, v in kw.items()})
    cfg.query_layout = nrc.QUERY_PADDED if padded else nrc.QUERY_COMPACT
    net = nrc.Network()
    net.init(stream=torch.cuda.current_stream(), encoding=enc, config=cfg)
    buf = torch.zeros((32, 16), device=dev)
    with pytest.raises(nrc.NrcError, match=what) as e:
        nrc.frame.infer_accumulate_factored(net, buf, buf, 32, buf, buf, 32, mode, 0)
    assert e.value.status == status
    net.destroy()


def test_factored_knob_range(nrc):
    with pytest.raises(nrc.NrcError) as e:
        nrc._lib.set_knob("frame_factored_fused", 2)
    assert e.value.status == 1 and nrc._lib.get_knob("frame_factored_fused") == -1
