"""In-process A/B of the culled fused accumulation (nrc_infer_accumulate_culled, nrc_infer_culled.hip) on the 1080p
frame (2,073,600 pixels + 32,400 train tiles) with bench.py's weights and query stream (tools/energy_ab.py
bench_weights). Four forms: F16 / FP8 handles x plain / reflectance-factored accumulation; the baseline is always the
dense entry of the form in the same process (nrc_infer_accumulate / nrc_infer_accumulate_factored); F16 plain also
times the sparse entry. Per live-fraction case the paths are interleaved round by round, the order reversed every other
round: back-to-back launches for --seconds after a --settle of the same launches, event-timed per chunk of launches.
The first launch of every path is compared bit for bit with the dense one. spread = (max - min) / median of a path's
round medians; a difference between the paths counts only beyond it.

    python tools/ab_culled.py > profiles/culled/ab_culled.json
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import nrc_loader  # noqa: E402
from ab_sparse import CASES, TILES, H, W, dead_mask  # noqa: E402
from energy_ab import bench_weights  # noqa: E402

FORMS = [("f16_plain", "PRECISION_F16", 0), ("fp8_plain", "PRECISION_FP8", 0),
         ("f16_factored", "PRECISION_F16", 1), ("fp8_factored", "PRECISION_FP8", 1)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--settle", type=float, default=0.3)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--mode", type=int, default=0, help="RenderMode: 0 Full, 2 CacheOnly")
    ap.add_argument("--forms", default=",".join(f[0] for f in FORMS))
    args = ap.parse_args()
    import torch

    nrc = nrc_loader.load()
    F = nrc.frame
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    npix, n = W * H, W * H + TILES
    enc = nrc.InputEncoding.Frequency
    res = torch.empty((n, 3), device=dev)
    out = {}
    for form, precision, rf in FORMS:
        if form not in args.forms.split(","):
            continue
        net = nrc.Network()
        net.init(stream=stream, encoding=enc, config=nrc.default_config(enc, infer_precision=getattr(nrc._lib, precision)))
        q = torch.from_numpy(bench_weights(nrc, net, torch, dev, n)).to(dev)
        fns = {"dense": F.infer_accumulate_factored if rf else F.infer_accumulate}
        if form == "f16_plain":
            fns["sparse"] = F.infer_accumulate_sparse
        fns["culled"] = lambda *a: F.infer_accumulate_culled(*a, rf)  # noqa: E731
        rng = np.random.default_rng(nrc.synthetic.SEED)
        out[form] = {}
        for case in CASES:
            dead = dead_mask(case, rng)
            thr_np = rng.uniform(0.05, 1, (npix, 3)).astype(np.float32)
            thr_np[dead] = 0.0
            thr = torch.from_numpy(thr_np).to(dev)
            rgba0 = torch.from_numpy(rng.uniform(0, 1, (npix, 4)).astype(np.float32)).to(dev)
            first = {}
            for name, fn in fns.items():
                rgba, r = rgba0.clone(), torch.zeros((n, 3), device=dev)
                fn(net, q, r, n, thr, rgba, npix, args.mode, 0)
                torch.cuda.synchronize()
                first[name] = (rgba.view(torch.int32), r[npix:].view(torch.int32))
            same = {name: bool(torch.equal(first["dense"][0], v[0]) and torch.equal(first["dense"][1], v[1]))
                    for name, v in first.items() if name != "dense"}
            rgba = rgba0.clone()

            def run_for(fn, seconds):
                us, t0 = [], time.perf_counter()
                while time.perf_counter() - t0 < seconds:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(args.chunk):
                        fn(net, q, res, n, thr, rgba, npix, args.mode, 0)
                    e1.record(stream)
                    e1.synchronize()
                    us.append(e0.elapsed_time(e1) / args.chunk * 1e3)
                return float(np.median(us))

            rounds = {name: [] for name in fns}
            for k in range(args.rounds):
                for name in (list(fns) if k % 2 == 0 else list(fns)[::-1]):
                    run_for(fns[name], args.settle)
                    rounds[name].append(run_for(fns[name], args.seconds))
            rec = {"live_fraction": float(1.0 - dead.mean()), "bitwise_equal_first_launch": same}
            for name in fns:
                m = float(np.median(rounds[name]))
                rec[name] = {"us_median": m, "spread": (max(rounds[name]) - min(rounds[name])) / m,
                             "rounds_us": rounds[name]}
            rec["culled_over_dense"] = rec["culled"]["us_median"] / rec["dense"]["us_median"]
            out[form][case] = rec
        net.destroy()
    print(json.dumps({"n": n, "num_pixels": npix, "mode": args.mode, "device": torch.cuda.get_device_properties(0).name,
                      "rounds": args.rounds, "seconds": args.seconds, "forms": out}, indent=1))


if __name__ == "__main__":
    main()
