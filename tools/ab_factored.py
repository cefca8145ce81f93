"""In-process A/B of the reflectance-factored frame (nrc_frame_params.reflectance_factoring = 1, train = 0) on the
synthetic 1080p Cornell frame (2,073,600 pixels + 32,400 train tiles): the frame driver with knob frame_factored_fused
= 0 (nrc_infer_stream + the factored accumulation kernel) against = 1 (nrc_infer_accumulate_factored: the accumulation
in the inference epilogue, nrc_infer_factored.hip / nrc_infer8.hip). Per handle (F16, FP8; bench.py's weights,
tools/energy_ab.py bench_weights) and frame (Full, CacheFirstVertex) the two knob values are interleaved round by
round, once in the order 0, 1 and once in the order 1, 0: back-to-back process_frame calls for --seconds after a --settle
of the same calls, event-timed per chunk of calls. The first frame of every case is compared bit for bit. spread =
(max - min) / median of a knob value's round medians; a difference between the two counts only beyond it.

    python tools/ab_factored.py > profiles/factored/ab_factored.json
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

W, H, TILE = 1920, 1080, 8
KNOB = "frame_factored_fused"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--settle", type=float, default=0.3)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    args = ap.parse_args()
    import torch

    nrc = nrc_loader.load()
    F = nrc.frame
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    f = nrc.synthetic.cornell_frame(args.width, args.height, (TILE, TILE), seed=1)
    S, T = f.screen_size, f.num_tiles
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cap = F.NUM_TRAINING_RECORDS_PER_FRAME
    rgba0 = torch.rand((S, 4), device=dev, generator=torch.Generator(dev).manual_seed(3))
    fb = F.FrameBuffers(t(f.queries_inference), torch.zeros((S + T, 3), device=dev), t(f.last_render_throughput),
                        rgba0.clone(), F.records_to_device(f.end_vertices, dev),
                        torch.zeros((cap, 7), dtype=torch.int32, device=dev),
                        [torch.zeros((cap, 15), device=dev) for _ in range(2)],
                        [torch.zeros((cap, 3), device=dev) for _ in range(2)],
                        queries_cache_vis=t(f.queries_cache_vis), results_cache_vis=torch.zeros((S, 3), device=dev))
    frames = {"full": F.FrameParams(S, T, 0, F.RenderMode.Full, 3, 0, 1, train=False, reflectance_factoring=True),
              "cache_first_vertex": F.FrameParams(S, T, 0, F.RenderMode.CacheFirstVertex, 0, 0, 1, train=False,
                                                  reflectance_factoring=True)}
    out = {}
    try:
        for prec in ("PRECISION_F16", "PRECISION_FP8"):
            enc = nrc.InputEncoding.Frequency
            net = nrc.Network()
            net.init(stream=stream, encoding=enc, config=nrc.default_config(enc, infer_precision=getattr(nrc._lib, prec)))
            bench_weights(nrc, net, torch, dev, 1)
            for fname, fp in frames.items():
                first = {}
                for knob in (0, 1):
                    nrc._lib.set_knob(KNOB, knob)
                    fb.output_rgba.copy_(rgba0)
                    F.process_frame(net, fb, fp, loss=False)
                    torch.cuda.synchronize()
                    first[knob] = (fb.output_rgba.clone().view(torch.int32), fb.results_inference[S:].clone().view(torch.int32))
                same = bool(torch.equal(first[0][0], first[1][0]) and torch.equal(first[0][1], first[1][1]))

                def run_for(knob, seconds):
                    nrc._lib.set_knob(KNOB, knob)
                    us, t0 = [], time.perf_counter()
                    while time.perf_counter() - t0 < seconds:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        for _ in range(args.chunk):
                            F.process_frame(net, fb, fp, loss=False)
                        e1.record(stream)
                        e1.synchronize()
                        us.append(e0.elapsed_time(e1) / args.chunk * 1e3)
                    return float(np.median(us))

                rec = {"bitwise_equal_first_frame": same}
                for order in ((0, 1), (1, 0)):
                    rounds = {0: [], 1: []}
                    for _ in range(args.rounds):
                        for knob in order:
                            run_for(knob, args.settle)
                            rounds[knob].append(run_for(knob, args.seconds))
                    o = {}
                    for knob, name in ((0, "unfused"), (1, "fused")):
                        m = float(np.median(rounds[knob]))
                        o[name] = {"us_median": m, "spread": (max(rounds[knob]) - min(rounds[knob])) / m,
                                   "rounds_us": rounds[knob]}
                    o["fused_over_unfused"] = o["fused"]["us_median"] / o["unfused"]["us_median"]
                    rec["order_%d_%d" % order] = o
                out[f"{prec[10:]}/{fname}"] = rec
            net.destroy()
    finally:
        nrc._lib.set_knob(KNOB, -1)
    print(json.dumps({"screen": S, "tiles": T, "train": 0, "reflectance_factoring": 1,
                      "device": torch.cuda.get_device_properties(0).name, "rounds": args.rounds,
                      "seconds": args.seconds, "cases": out}, indent=1))


if __name__ == "__main__":
    main()
