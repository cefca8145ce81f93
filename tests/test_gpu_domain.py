"""Every kernel path over the whole query domain (tests/domain_cases.py) instead of the 0.1-wide Cornell cube:

* encoders: every feature of every bulk and branch row within one f16 ulp + 2e-6 of the f16-rounded oracle encoding;
* inference against the oracle of the same numerics, at the bounds each path's own parity test states;
* the fused epilogues bitwise against infer + the accumulation kernel, throughputs with exact zeros;
* gradients per parameter block: rel-L2 <= max(2e-3, 2 d_block), d_block the oracle's own MIXED-vs-FP32 distance
  (tests/test_domain_oracle.py); Hash grid levels by touched entries and signs;
* rows that must not matter, bitwise against a clean run: non-finite rows inside a launch, NaN rows past n or b.
"""
import numpy as np
import pytest

import domain_cases as dc
from test_gpu_fp8_64 import dense_params, model as fp8_model
from test_gpu_padded import api_column
from test_gpu_wide import wide_params

pytestmark = pytest.mark.gpu
SENT = 777.0
# the fused entries and the precisions each has a kernel for (no sparse FP8: test_sparse_refusals)
EPILOGUES = [("dense", "PRECISION_F16"), ("dense", "PRECISION_FP8"), ("sparse", "PRECISION_F16"),
             ("factored", "PRECISION_F16"), ("factored", "PRECISION_FP8")]


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# kind -> (encoding, config keywords, padded records, oracle kind, oracle mode name)
PATHS = {
    "f16": ("Frequency", {}, False, "frequency", "MIXED"),
    "acc16": ("Frequency", {"infer_precision": "PRECISION_F16_ACC16"}, False, "frequency", "TCNN"),
    "fp8_64": ("Frequency", {"infer_precision": "PRECISION_FP8"}, False, "frequency", None),
    "wide_f16": ("Frequency", {"width": 128}, False, "wide", "MIXED"),
    "wide_fp8": ("Frequency", {"width": 128, "infer_precision": "PRECISION_FP8"}, False, "wide", "FP8"),
    "sh": ("FrequencySH", {}, False, "sh", "MIXED"),
    "padded": ("Frequency", {}, True, "padded", "MIXED"),
    "hash": ("Hash", {}, False, "hash", "MIXED"),
    "hash_gather": ("Hash", {}, False, "hash", "MIXED"),
    "hash_acc16": ("Hash", {"infer_precision": "PRECISION_F16_ACC16"}, False, "hash", "TCNN"),
    "hash_padded": ("Hash", {}, True, "hash_padded", "MIXED"),
}


def make_net(nrc, kind):
    import torch
    enc, kw, pad, _, _ = PATHS[kind]
    enc = getattr(nrc.InputEncoding, enc)
    cfg = nrc.default_config(enc, **{k: getattr(nrc._lib, v) if isinstance(v, str) else v for k, v in kw.items()})
    cfg.query_layout = nrc.QUERY_PADDED if pad else nrc.QUERY_COMPACT
    net = nrc.Network()
    net.init(stream=torch.cuda.current_stream(), encoding=enc, config=cfg)
    return net


def path_params(kind, orc, golden):
    if kind == "fp8_64":
        return dense_params(12)
    if kind == "wide_fp8":
        return wide_params(12)
    return dc.case_params(PATHS[kind][3], orc, golden)


def infer(nrc, dev, net, kind, q, n=None, offset=0):
    """outputs of the first n rows of q (the buffer holds all of q, `offset` floats in), sentinels past n checked"""
    import torch
    n = len(q) if n is None else n
    buf = torch.zeros(q.size + offset, device=dev)
    buf[offset:] = _t(q, dev).reshape(-1)
    out = torch.full((n + 8, 3), SENT, device=dev)
    try:
        if kind == "hash_gather":
            nrc._lib.set_knob("hash_infer", 1)
        net.infer(buf[offset:], out, n)
    finally:
        if kind == "hash_gather":
            nrc._lib.set_knob("hash_infer", -1)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[n:] == SENT).all(), "infer wrote past n"
    return o[:n]


# ---- encoders ---------------------------------------------------------------------------------------------------------
def _check_features(got, ref32, what):
    with np.errstate(over="ignore"):
        ref = ref32.astype(np.float16).astype(np.float32)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]) or np.array_equal(got[~fin], ref32[~fin]), f"{what}: f16-inf features"
    with np.errstate(invalid="ignore"):
        bad = np.argwhere(fin & ~(np.abs(got - ref) <= np.abs(ref) * 2.0 ** -10 + 2e-6))
    assert bad.size == 0, f"{what}: {len(bad)} features off, first (row, feature, got, want): " \
                          f"{[(int(r), int(f), float(got[r, f]), float(ref[r, f])) for r, f in bad[:5]]}"


@pytest.mark.parametrize("entry", ["encode", "fast0", "fast1", "fast2", "net_frequency", "net_sh", "net_hash"])
def test_encoders_on_the_domain(nrc, orc, golden, dev, entry):
    import torch
    L = nrc._lib.lib()
    q = dc.domain_queries(4097, hash_safe=entry == "net_hash")  # branch rows included, overflow rows too
    n, qd = len(q), _t(q, dev)
    enc = torch.full((n, 64 if entry == "net_hash" else 80), SENT, device=dev)
    if entry == "encode":
        nrc.encode(qd, enc, n)
        ref = orc.encode(q)
    elif entry.startswith("fast"):
        nrc._lib.check(L.nrc_debug_encode_fast_variant(int(entry[4]), qd.data_ptr(), enc.data_ptr(), n, None))
        ref = orc.encode(q)
    else:
        kind = {"net_frequency": "f16", "net_sh": "sh", "net_hash": "hash"}[entry]
        net = make_net(nrc, kind)
        params = path_params(kind, orc, golden)
        net.set_state(nrc.StateSlot.INFER, params)
        net.encode_features(qd, enc, n)
        ref = {"f16": orc.encode, "sh": orc.encode_sh}[kind](q) if kind != "hash" else orc.hash_encode(params, q, orc.MIXED)
    torch.cuda.synchronize()
    _check_features(enc.cpu().numpy(), ref, entry)
    if not entry.startswith(("encode", "fast")):
        net.destroy()


# ---- inference --------------------------------------------------------------------------------------------------------
_REF = {}


def reference(orc, golden, kind, n):
    """oracle outputs of the first n network rows in the path's numerics, computed once per (oracle kind, mode)"""
    _, _, _, okind, mode = PATHS[kind]
    key = (okind, mode, n, kind if mode is None or kind.startswith("wide") else "")
    if key not in _REF:
        q = dc.case_queries(okind, n)
        p = path_params(kind, orc, golden)
        y = fp8_model(orc, p, q) if mode is None else dc.oracle_forward(orc, okind, p, q, getattr(orc, mode))
        assert np.isfinite(y).all()
        _REF[key] = (q, y)
    return _REF[key]


def check_parity(kind, o, y):
    n = len(y)
    r = dc.rel_l2(o, y)
    if kind == "fp8_64":   # tests/test_gpu_fp8_64.py: B
        print(f"{kind}: rel-L2 {r:.3e}")
        assert r <= 1.7e-2
        return
    if kind == "wide_fp8":  # tests/test_gpu_wide.py::test_wide_fp8_infer_parity
        close = float(np.mean(np.abs(o - y) <= 2.0 ** -10 * np.abs(y) + 1e-6))
        print(f"{kind}: rel-L2 {r:.3e}, {close:.4f} within 2^-10")
        assert r <= (2.2e-2 if n > 1000 else 3e-2) and (n <= 1000 or close > 0.98)
        return
    err = np.abs(o - y).max(axis=1)
    tol = 16.0 * 2.0 ** -11 * np.maximum(np.abs(y).max(axis=1), 1e-2)
    far = np.flatnonzero(err > tol)
    print(f"{kind}: rel-L2 {r:.3e}, {far.size} of {n} rows beyond 16 ulps (cap {0.001 * n:.1f})")
    assert far.size <= 0.001 * n, (far[:5], o[far[:2]], y[far[:2]])
    assert r <= 1e-3, r


@pytest.mark.parametrize("kind", list(PATHS))
def test_inference_on_the_domain(nrc, orc, golden, dev, kind):
    net = make_net(nrc, kind)
    try:
        net.set_state(nrc.StateSlot.INFER, path_params(kind, orc, golden))
        q, y = reference(orc, golden, kind, dc.N_INFER)
        o = infer(nrc, dev, net, kind, q)
        check_parity(kind, o, y)
        m = 777  # not a multiple of 32, the records one float into their buffer
        np.testing.assert_array_equal(infer(nrc, dev, net, kind, q[:m], offset=1), o[:m])
        if kind == "hash":
            np.testing.assert_array_equal(infer(nrc, dev, net, "hash_gather", q), o)
    finally:
        net.destroy()


@pytest.mark.parametrize("entry,prec", EPILOGUES)
def test_fused_epilogues_on_the_domain(nrc, orc, golden, dev, entry, prec):
    import torch
    F, i32 = nrc.frame, torch.int32
    net = make_net(nrc, "f16" if prec == "PRECISION_F16" else "fp8_64")
    try:
        net.set_state(nrc.StateSlot.INFER, orc.init_params(1337) * np.float32(1.6))
        n, npix = 4099, 4001
        q = dc.case_queries("frequency", n)
        rng = np.random.default_rng(npix)
        thr = rng.uniform(0.05, 1, (npix + 1, 3)).astype(np.float32)
        thr[:npix][rng.random(npix) < 0.3] = 0.0  # dead and live pixels inside one tile
        qd, thr, rgba0 = _t(q, dev), _t(thr, dev), _t(rng.uniform(0, 1, (npix + 1, 4)).astype(np.float32), dev)
        for mode in (0, 2):
            ref_res = torch.empty((n, 3), device=dev)
            net.infer(qd, ref_res, n)
            ref_rgba, rgba = rgba0.clone(), rgba0.clone()
            res = torch.full((n + 1, 3), -3.0, device=dev)
            if entry == "factored":
                F.accumulate_render_radiance_factored(ref_res, qd, thr, ref_rgba, npix, mode, 5)
                F.infer_accumulate_factored(net, qd, res, n, thr, rgba, npix, mode, 5)
            else:
                F.accumulate_render_radiance(ref_res, thr, ref_rgba, npix, mode, 5)
                (F.infer_accumulate if entry == "dense" else F.infer_accumulate_sparse)(net, qd, res, n, thr, rgba, npix,
                                                                                       mode, 5)
            torch.cuda.synchronize()
            assert torch.isfinite(ref_res).all() and (ref_res[:npix] != 0).any(dim=1).float().mean() > 0.5
            assert torch.equal(rgba.view(i32), ref_rgba.view(i32)), (entry, mode)
            assert torch.equal(res[npix:n].view(i32), ref_res[npix:].view(i32))
            assert torch.all(res[:npix] == -3.0) and torch.all(res[n] == -3.0)
    finally:
        net.destroy()


# ---- gradients per block ----------------------------------------------------------------------------------------------
GRAD_NET = {"frequency": "f16", "padded": "padded", "sh": "sh", "wide": "wide_f16", "hash": "hash"}


@pytest.mark.parametrize("kind,b", dc.GRAD_CASES)
def test_gradient_blocks_on_the_domain(nrc, orc, golden, dev, kind, b):
    import torch
    q = dc.train_queries(kind, b)
    t = dc.train_targets(nrc, b)
    params = dc.case_params(kind, orc, golden)
    g_ref, loss_ref, d = dc.block_distances(orc, kind, params, q, t)
    P = g_ref.size
    net = make_net(nrc, GRAD_NET[kind])

    def gpu_grad(qq, tt):
        grad = torch.full((net.grad_floats,), 7.0, device=dev)
        net.train_grad(_t(qq, dev), _t(tt, dev), len(qq), b, grad)
        torch.cuda.synchronize()
        g = grad.cpu().numpy()
        loss, g = g[P], g[:P].copy()
        if kind == "padded":  # the handle's gradient is in its internal (compact) column order
            w0 = g[:5120].reshape(64, 80).copy()
            g[:5120].reshape(64, 80)[:, [api_column(False, c) for c in range(80)]] = w0
        return g, loss

    mlp = np.concatenate([i for k, i in dc.case_blocks(kind).items() if not k.startswith("grid.")])
    try:
        net.set_state(nrc.StateSlot.PARAMS, params)
        g, loss = gpu_grad(q, t)
        # measured beside the assertions: the same comparison without the rows at the output ReLU's kink, whose whole
        # contribution passes the gate in one numerics and not in another (dc.kink_rows)
        keep = ~dc.kink_rows(orc, kind, params, q)
        gk, _ = gpu_grad(q[keep], t[keep])
        rk, _ = dc.oracle_grad(orc, kind, params, q[keep], t[keep], orc.MIXED, n_total=3.0 * b)
        r32, _ = dc.oracle_grad(orc, kind, params, q[keep], t[keep], orc.FP32, n_total=3.0 * b)
        print(f"{kind} b={b}: MLP gradient GPU vs MIXED {dc.rel_l2(g[mlp], g_ref[mlp]):.2e} (MIXED vs FP32 "
              f"{dc.rel_l2(g_ref[mlp], dc.oracle_grad(orc, kind, params, q, t, orc.FP32)[0][mlp]):.2e}); without the "
              f"{int((~keep).sum())} kink rows {dc.rel_l2(gk[mlp], rk[mlp]):.2e} (MIXED vs FP32 {dc.rel_l2(rk[mlp], r32[mlp]):.2e})")
    finally:
        net.destroy()
    assert abs(loss - loss_ref) <= 1e-3 * abs(loss_ref), (loss, loss_ref)
    fails = []
    for name, idx in dc.case_blocks(kind).items():
        if name.startswith("grid."):
            continue
        if not g_ref[idx].any():
            assert not g[idx].any(), f"{name}: the oracle's gradient is exactly zero"
            continue
        r, bound = dc.rel_l2(g[idx], g_ref[idx]), max(2e-3, 2.0 * d[name])
        print(f"{kind} b={b} {name}: rel-L2 {r:.2e} (bound {bound:.2e}, d_block {d[name]:.2e})")
        if not r <= bound:
            fails.append((name, r, bound))
    assert not fails, fails
    if kind == "hash":  # tests/test_gpu_hash.py::test_hash_train_step_matches_oracle's criterion, per level
        for name, sl in dc.hash_level_blocks().items():
            a, r = g[sl], g_ref[sl]
            ta, tr = a != 0, r != 0
            both = ta & tr
            print(f"{name}: touched {int(ta.sum())} vs {int(tr.sum())}, agree {np.mean(ta == tr):.5f}, "
                  f"signs {np.mean(np.sign(a[both]) == np.sign(r[both])):.4f}")
            if name in ("grid.L0", "grid.L1"):
                assert np.count_nonzero(r.reshape(-1, 2).any(axis=1)) > 1000, f"{name}: vacuous batch"
            assert np.mean(ta == tr) >= 0.995, name
            assert np.mean(np.sign(a[both]) == np.sign(r[both])) >= 0.99, name


# ---- rows that must not matter ----------------------------------------------------------------------------------------
ISOLATED = ["f16", "acc16", "hash", "hash_gather", "sh", "padded", "wide_f16", "wide_fp8"]
BAD_AT = [0, 5, 31, 32, 40, 63, 64, 95, 96]  # first tile, a middle tile, the ragged last tile of n = 97


def _hostile(kind, q):
    """q with the rows BAD_AT replaced by hostile rows, all of them used over the kinds"""
    h = dc.hostile_rows()
    bad = q.copy()
    pick = h[(np.arange(len(BAD_AT)) * 3 + sorted(PATHS).index(kind)) % len(h)]
    bad[BAD_AT] = dc.padded(pick, np.nan) if q.shape[1] == 16 else pick
    return bad


@pytest.mark.parametrize("kind", ISOLATED)
def test_bad_rows_stay_in_their_rows(nrc, orc, golden, dev, kind):
    """n = 97: hostile rows change their own outputs only; NaN rows past n (n = 97 and 1 of 128) change nothing; a clean
    call afterwards is the first clean run"""
    net = make_net(nrc, kind)
    try:
        net.set_state(nrc.StateSlot.INFER, path_params(kind, orc, golden))
        okind = PATHS[kind][3]
        q = dc.case_queries(okind, 128)
        clean = infer(nrc, dev, net, kind, q[:97])
        assert np.isfinite(clean).all() and clean.any()
        keep = np.setdiff1d(np.arange(97), BAD_AT)
        got = infer(nrc, dev, net, kind, _hostile(kind, q[:97]))
        np.testing.assert_array_equal(got[keep].view(np.int32), clean[keep].view(np.int32))
        tail = q.copy()
        for n in (97, 1):
            tail[n:] = np.nan
            np.testing.assert_array_equal(infer(nrc, dev, net, kind, tail, n=n).view(np.int32), clean[:n].view(np.int32))
        np.testing.assert_array_equal(infer(nrc, dev, net, kind, q[:97]).view(np.int32), clean.view(np.int32))
    finally:
        net.destroy()


@pytest.mark.parametrize("entry,prec", EPILOGUES)
def test_bad_rows_stay_in_their_pixels(nrc, orc, golden, dev, entry, prec):
    import torch
    F = nrc.frame
    kind = "f16" if prec == "PRECISION_F16" else "fp8_64"
    net = make_net(nrc, kind)
    try:
        net.set_state(nrc.StateSlot.INFER, orc.init_params(1337) * np.float32(1.6))
        n, npix = 97, 70
        q = dc.case_queries("frequency", 128)
        rng = np.random.default_rng(7)
        thr = rng.uniform(0.05, 1, (npix, 3)).astype(np.float32)
        thr[[3, 33, 66]] = 0.0
        rgba0 = rng.uniform(0, 1, (npix + 1, 4)).astype(np.float32)
        call = {"dense": F.infer_accumulate, "sparse": F.infer_accumulate_sparse, "factored": F.infer_accumulate_factored}[entry]

        def run(rows, n_rows=n):
            res, rgba = torch.full((n + 8, 3), SENT, device=dev), _t(rgba0, dev)
            call(net, _t(rows, dev), res, n_rows, _t(thr, dev), rgba, min(npix, n_rows), 0, 5)
            torch.cuda.synchronize()
            return res.cpu().numpy().view(np.int32), rgba.cpu().numpy().view(np.int32)

        res0, rgba0_out = run(q[:97])
        keep = np.setdiff1d(np.arange(97), BAD_AT)
        res1, rgba1 = run(_hostile(kind, q[:97]))
        np.testing.assert_array_equal(res1[97:], res0[97:])  # sentinels
        np.testing.assert_array_equal(res1[keep], res0[keep])
        kp = np.setdiff1d(np.arange(npix + 1), BAD_AT)
        np.testing.assert_array_equal(rgba1[kp], rgba0_out[kp])
        tail = q.copy()
        tail[97:] = np.nan
        res2, rgba2 = run(tail)
        np.testing.assert_array_equal(res2, res0)
        np.testing.assert_array_equal(rgba2, rgba0_out)
        # n = 1 of 128 rows (one pixel; train-suffix form: npix = 0), rows 1..127 NaN: row / pixel 0 and every sentinel
        for pix in (1, 0):
            def run1(rows):
                res, rgba = torch.full((n + 8, 3), SENT, device=dev), _t(rgba0, dev)
                call(net, _t(rows, dev), res, 1, _t(thr, dev), rgba, pix, 0, 5)
                torch.cuda.synchronize()
                return res.cpu().numpy().view(np.int32), rgba.cpu().numpy().view(np.int32)
            tail1 = q.copy()
            tail1[1:] = np.nan
            res_c, rgba_c = run1(q[:1])
            res_t, rgba_t = run1(tail1)
            np.testing.assert_array_equal(res_t, res_c)
            np.testing.assert_array_equal(rgba_t, rgba_c)
            assert (res_c[1:] == res0[97:][0]).all() and np.array_equal(rgba_c[1:], _t(rgba0, dev).cpu().numpy().view(np.int32)[1:])
            assert (rgba_c[0] != rgba0.view(np.int32)[0]).any() if pix else (res_c[0] != res0[97]).any()
        res3, rgba3 = run(q[:97])
        np.testing.assert_array_equal(res3, res0)
        np.testing.assert_array_equal(rgba3, rgba0_out)
    finally:
        net.destroy()


@pytest.mark.parametrize("kind", ["frequency", "padded", "sh", "wide", "hash"])
def test_training_ignores_rows_past_b(nrc, orc, golden, dev, kind):
    """b = 100 of 128 rows: NaN in the tail of queries and targets == a zero tail, bitwise: gradient buffer and loss of
    nrc_train_grad; loss and all five state slots of nrc_train_batch"""
    import torch
    q = dc.case_queries(kind, 128)
    t = nrc.synthetic.cornell_targets(128, seed=428)
    b = 100
    results = []
    for fill in (0.0, np.nan):
        qq, tt = q.copy(), t.copy()
        qq[b:], tt[b:] = fill, fill
        net = make_net(nrc, GRAD_NET[kind])
        try:
            for slot in (nrc.StateSlot.PARAMS, nrc.StateSlot.INFER):
                net.set_state(slot, dc.case_params(kind, orc, golden))
            qd, td = _t(qq, dev), _t(tt, dev)
            grad = torch.full((net.grad_floats,), 7.0, device=dev)
            net.train_grad(qd, td, b, b, grad)
            loss = net.train_batch(qd, td, b, loss=True)
            torch.cuda.synchronize()
            results.append([grad.cpu().numpy(), np.float32(loss)] + [net.get_state(s) for s in nrc.StateSlot])
        finally:
            net.destroy()
    P = results[0][0].size - 4
    assert np.isfinite(results[0][0][:P + 1]).all() and results[0][0][:P].any() and np.isfinite(results[0][1])
    for what, a, c in zip(["grad", "loss"] + [s.name for s in nrc.StateSlot], results[0], results[1]):
        a, c = np.atleast_1d(a), np.atleast_1d(c)
        if what == "grad":
            a, c = a[:P + 1], c[:P + 1]
        np.testing.assert_array_equal(a.view(np.int32), c.view(np.int32), err_msg=what)
