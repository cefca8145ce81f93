"""nrc_train_gather (csrc/nrc_train16.hip train16_gather_kernel, csrc/nrc_train_dc.hip train_dc_gather_kernel,
include/nrc/frame.h) and the frame driver's knob "frame_train_gather": an optimizer step whose samples are read from
the traced buffers through the shuffle's permutation. References: the unfused pair (permute_train_data + train_async,
kernels not under test here) and the CPU oracle's training step; "equal" is numpy array_equal on every state slot."""
import numpy as np
import pytest

from test_gpu_frame import _device_frame, _t

pytestmark = pytest.mark.gpu


def _perm(seed, frame, n):
    """The Feistel permutation of (seed, frame) on [0, n), restated: 4 keyed rounds on 2h bits, walked
    until the value is below n."""
    M = 0xFFFFFFFF

    def mix(x):
        x = (x ^ (x >> 16)) * 0x7FEB352D & M
        x = (x ^ (x >> 15)) * 0x846CA68B & M
        return x ^ (x >> 16)

    keys = [int(mix((seed & M) ^ mix((seed >> 32) ^ mix((frame + 0x9E3779B9 * (r + 1)) & M)))) for r in range(4)]
    bits = max(2, (n - 1).bit_length())
    h = (bits + (bits & 1)) // 2
    x = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, bool)
    while todo.any():
        L, R = x[todo] >> np.uint64(h), x[todo] & np.uint64((1 << h) - 1)
        for k in keys:
            L, R = R, L ^ (mix(R ^ np.uint64(k)) & np.uint64((1 << h) - 1))
        x[todo] = (L << np.uint64(h)) | R
        todo = x >= n
    return x.astype(np.int64)


def _net(nrc, padded=False, **kw):
    import torch
    enc = kw.pop("encoding", nrc.InputEncoding.Frequency)
    cfg = nrc.default_config(enc, **kw)
    cfg.query_layout = nrc.QUERY_PADDED if padded else nrc.QUERY_COMPACT
    net = nrc.Network()
    net.init(stream=torch.cuda.current_stream(), encoding=enc, config=cfg)
    return net


@pytest.fixture(scope="module")
def traced(nrc):
    """65,536 traced records (compact; the padded cases insert pad_) and an explicit random permutation."""
    q, t = nrc.synthetic.cornell_batch(65536, seed=41)
    rng = np.random.default_rng(5)
    return q, t, rng.uniform(0.5, 1.5, 65536).astype(np.float32), rng.permutation(65536).astype(np.int32)


@pytest.mark.parametrize("padded", [False, True], ids=["compact", "padded"])
@pytest.mark.parametrize("first,b", [(0, 16384), (49152, 16384), (4096, 2048), (7, 130)])
@pytest.mark.parametrize("n_out", [65536, 50000])
@pytest.mark.parametrize("num_records", [65536, 40000, 100])
@pytest.mark.parametrize("explicit", [True, False], ids=["perm", "feistel"])
def test_gather_step_bitwise(nrc, dev, traced, explicit, num_records, n_out, first, b, padded):
    """Two steps of train_gather == two steps of permute_train_data + train_async on rows [first, first + b), on every
    state slot and the loss. (first + b must be <= n_out: at n_out = 50,000 the last-slice case starts at n_out - b.)"""
    import torch
    F, L = nrc.frame, nrc._lib
    first = min(first, n_out - b)
    q, t, pad, perm = traced
    qs = _t(np.insert(q, 3, pad, axis=1) if padded else q, dev)
    ts = _t(t, dev)
    pd = _t(perm[perm < n_out], dev) if explicit else None  # a permutation of [0, n_out)
    ref, got = _net(nrc, padded), _net(nrc, padded)
    loss = torch.zeros((2, 2), device=dev)
    for step in range(2):
        qd, td = torch.zeros((n_out, qs.shape[1]), device=dev), torch.zeros((n_out, 3), device=dev)
        F.permute_train_data(qs, ts, pd, 77, 9 + step, num_records, qd, td, n_out, padded=padded)
        L.check(L.lib().nrc_train_async(ref._h, qd[first:].data_ptr(), td[first:].data_ptr(), b, loss[0, step:].data_ptr()))
        F.train_gather(got, qs, ts, pd, 77, 9 + step, num_records, first, b, n_out, loss=loss[1, step:])
    torch.cuda.synchronize()
    assert torch.all(loss[0] > 0) and torch.equal(loss[0], loss[1])
    for slot in nrc.StateSlot:
        np.testing.assert_array_equal(got.get_state(slot), ref.get_state(slot), err_msg=slot.name)
    assert got.step == ref.step == 2
    ref.destroy()
    got.destroy()


def test_gather_step_vs_oracle(nrc, orc, dev, traced, golden):
    """One gathered step of 2,048 samples from the golden weights against the oracle's step on the same samples,
    gathered in numpy; the bounds are those of tests/test_gpu_parity.py for a training step against ORC_MIXED."""
    import torch
    q, t, _, _ = traced
    first, b, nrec = 4096, 2048, 40000
    rows = _perm(0xDEADBEEF12345, 5, 65536)[first:first + b] % nrec
    net = _net(nrc)
    net.set_state(nrc.StateSlot.PARAMS, golden["params_b"])
    loss = torch.zeros(1, device=dev)
    nrc.frame.train_gather(net, _t(q, dev), _t(t, dev), None, 0xDEADBEEF12345, 5, nrec, first, b, loss=loss)
    torch.cuda.synchronize()
    st = orc.AdamEmaState(golden["params_b"])
    g, l_ref = orc.grad(st.params, q[rows], t[rows], mode=orc.MIXED)
    st.apply(g)
    rel = lambda a, w: np.linalg.norm(np.float64(a) - w) / np.linalg.norm(np.float64(w))  # noqa: E731
    np.testing.assert_allclose(loss.item(), l_ref, rtol=2e-2)
    assert rel(net.get_state(nrc.StateSlot.PARAMS), st.params) <= 1e-3
    assert rel(net.get_state(nrc.StateSlot.INFER), st.infer) <= 1e-3
    net.destroy()


@pytest.mark.parametrize("with_keys", [False, True], ids=["feistel", "shuffle_keys"])
def test_frame_train_gather_knob(nrc, dev, with_keys):
    """process_frame with knob frame_train_gather = 1 == the permuting frame on state, loss and frame buffer, bitwise;
    the shuffled [1] buffers are not written."""
    import torch
    F = nrc.frame
    f = nrc.synthetic.cornell_frame(64, 48, (8, 8))
    keys = np.random.default_rng(3).integers(0, 1 << 32, 65536, dtype=np.uint64).astype(np.uint32).view(np.int32)
    out = []
    try:
        for knob in (1, 0):
            nrc._lib.set_knob("frame_train_gather", knob)
            net = _net(nrc)
            fb, *_ = _device_frame(nrc, f, dev)
            fb.shuffle_keys = _t(keys, dev) if with_keys else None
            fb.train_queries[1].fill_(-3.0)
            fb.train_targets[1].fill_(-3.0)
            loss = F.process_frame(net, fb, F.FrameParams(f.screen_size, f.num_tiles, f.num_training_records,
                                                          frame_index=2, shuffle_seed=7))
            torch.cuda.synchronize()
            out.append((loss, fb, [net.get_state(s) for s in nrc.StateSlot]))
            net.destroy()
    finally:
        nrc._lib.set_knob("frame_train_gather", -1)
    (l1, fb1, s1), (l0, fb0, s0) = out
    assert l1 == l0 and l0 > 0
    assert torch.equal(fb1.output_rgba, fb0.output_rgba)
    for a, w in zip(s1, s0):
        np.testing.assert_array_equal(a, w)
    assert torch.all(fb1.train_queries[1] == -3.0) and torch.all(fb1.train_targets[1] == -3.0)
    assert not torch.any(fb0.train_queries[1] == -3.0)  # the permuting frame did write what the gather skips


@pytest.mark.parametrize("what,kw,args,status", [
    ("Hash", {"encoding": "Hash"}, (100, 65536, 0, 128), 5),
    ("FrequencySH", {"encoding": "FrequencySH"}, (100, 65536, 0, 128), 5),
    ("128", {"width": 128}, (100, 65536, 0, 128), 5),
    ("num_records", {}, (0, 65536, 0, 128), 1),
    ("batch size", {}, (100, 65536, 0, 0), 1),
    ("first \\+ b", {}, (100, 65536, 65536 - 127, 128), 1),
    ("n_out", {}, (100, 0, 0, 128), 1)])
def test_gather_refusals(nrc, dev, what, kw, args, status):
    import torch
    kw = {k: getattr(nrc.InputEncoding, v) if k == "encoding" else v for k, v in kw.items()}
    net = _net(nrc, **kw)
    buf = torch.zeros((65536, 16), device=dev)
    num_records, n_out, first, b = args
    with pytest.raises(nrc.NrcError, match=what) as e:
        nrc.frame.train_gather(net, buf, buf, None, 1, 2, num_records, first, b, n_out)
    assert e.value.status == status and net.step == 0
    net.destroy()


def test_gather_knob_range(nrc):
    with pytest.raises(nrc.NrcError) as e:
        nrc._lib.set_knob("frame_train_gather", 2)
    assert e.value.status == 1 and nrc._lib.get_knob("frame_train_gather") == -1
