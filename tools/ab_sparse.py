"""In-process A/B of the fused inference + accumulation on the 1080p frame (2,073,600 pixels + 32,400 train tiles): the
dense kernel (nrc_infer_accumulate) against the sparse one (nrc_infer_accumulate_sparse, nrc_infer_sparse.hip) on ONE
handle with bench.py's weights and query stream (tools/energy_ab.py bench_weights). Per live-fraction case the two paths
are interleaved round by round: back-to-back launches for --seconds after a --settle of the same launches, event-timed
per chunk of launches. The first launch of every case is compared bit for bit. spread = (max - min) / median of a path's
round medians; a difference between the paths counts only beyond it.

    python tools/ab_sparse.py > profiles/sparse/ab_sparse.json
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
from energy_ab import bench_weights  # noqa: E402

W, H, TILES = 1920, 1080, 32_400


def dead_mask(case: str, rng) -> np.ndarray:
    p = W * H
    if case == "live_1.0":
        return np.zeros(p, bool)
    if case == "live_0.95_synthetic":  # synthetic.cornell_frame kills a random 5 % of the pixels
        return rng.random(p) < 0.05
    if case == "live_0.5_random":
        return rng.permutation(p) < p // 2
    if case == "live_0.5_coherent":  # the top half of the image
        return np.arange(p) < p // 2
    if case == "live_0.1_random":
        return rng.permutation(p) < p - p // 10
    raise ValueError(case)


CASES = ["live_1.0", "live_0.95_synthetic", "live_0.5_random", "live_0.5_coherent", "live_0.1_random"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--settle", type=float, default=0.3)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--mode", type=int, default=0, help="RenderMode: 0 Full, 2 CacheOnly")
    args = ap.parse_args()
    import torch

    nrc = nrc_loader.load()
    F = nrc.frame
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    net = nrc.Network()
    net.init(stream=stream)
    npix, n = W * H, W * H + TILES
    q = torch.from_numpy(bench_weights(nrc, net, torch, dev, n)).to(dev)
    res = torch.empty((n, 3), device=dev)
    fns = {"dense": F.infer_accumulate, "sparse": F.infer_accumulate_sparse}
    rng = np.random.default_rng(nrc.synthetic.SEED)
    out = {}
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
        same = bool(torch.equal(first["dense"][0], first["sparse"][0]) and torch.equal(first["dense"][1], first["sparse"][1]))
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
        for _ in range(args.rounds):
            for name, fn in fns.items():
                run_for(fn, args.settle)
                rounds[name].append(run_for(fn, args.seconds))
        rec = {"live_fraction": float(1.0 - dead.mean()), "bitwise_equal_first_launch": same}
        for name in fns:
            m = float(np.median(rounds[name]))
            rec[name] = {"us_median": m, "spread": (max(rounds[name]) - min(rounds[name])) / m, "rounds_us": rounds[name]}
        rec["sparse_over_dense"] = rec["sparse"]["us_median"] / rec["dense"]["us_median"]
        out[case] = rec
    net.destroy()
    print(json.dumps({"n": n, "num_pixels": npix, "mode": args.mode, "device": torch.cuda.get_device_properties(0).name,
                      "rounds": args.rounds, "seconds": args.seconds, "cases": out}, indent=1))


if __name__ == "__main__":
    main()
