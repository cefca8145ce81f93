"""In-process A/B of the training frame (nrc_frame_params.train = 1, RenderMode Full) on the synthetic 1080p Cornell
frame (2,073,600 pixels + 32,400 train tiles, 65,536 training records): the frame driver with knob frame_train_gather
= 0 (propagate -> permute_train_data -> 4 x train on the shuffled buffers) against = 1 (propagate -> 4 x
nrc_train_gather on the traced buffers: no permute launch, csrc/nrc_train_gather.hip). Per permutation source
(Feistel, shuffle keys) the two knob values are interleaved round by round, once in the order 0, 1 and once in the
order 1, 0: back-to-back process_frame calls for --seconds after a --settle of the same calls, event-timed per chunk of
calls. Before timing, two handles with the same state run one frame under each knob value and every state slot and
the loss are compared bit for bit. spread = (max - min) / median of a knob value's round medians; a difference
between the two counts only beyond it.

--tree PATH times another checkout's package and library (e.g. the parent commit, built) on the same frame in the same
run: a tree without the knob gives the "baseline" rows only, so that a regression of the default path would show.

    python tools/ab_train_gather.py [--tree ../parent] > profiles/train_gather/ab_train_gather.json
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
W, H, TILE = 1920, 1080, 8
KNOB = "frame_train_gather"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--settle", type=float, default=0.3)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--tree", type=Path, default=ROOT)
    args = ap.parse_args()
    tree = args.tree.resolve()
    sys.path.insert(0, str(tree))
    sys.path.insert(0, str(tree / "tools"))
    import nrc_loader
    import torch
    from energy_ab import bench_weights

    nrc = nrc_loader.load()
    F = nrc.frame
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    try:
        nrc._lib.get_knob(KNOB)
        knobs = (0, 1)
    except nrc.NrcError:
        knobs = (0,)  # a tree from before the knob: the permuting sequence only
    f = nrc.synthetic.cornell_frame(args.width, args.height, (TILE, TILE), seed=1)
    S, T = f.screen_size, f.num_tiles
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cap = F.NUM_TRAINING_RECORDS_PER_FRAME

    def rows(a, width, dtype=np.float32):
        out = np.zeros((cap, width) if width else cap, dtype)
        out[: len(a)] = a[:cap]
        return out

    targets0 = t(rows(f.train_targets, 3))  # propagation adds into [0]: restored before every compared frame
    keys = np.random.default_rng(3).integers(0, 1 << 32, cap, dtype=np.uint64).astype(np.uint32).view(np.int32)
    fb = F.FrameBuffers(t(f.queries_inference), torch.zeros((S + T, 3), device=dev), t(f.last_render_throughput),
                        torch.zeros((S, 4), device=dev), F.records_to_device(f.end_vertices, dev),
                        F.records_to_device(rows(f.train_records, 0, F.TRAINING_RECORD_DTYPE), dev),
                        [t(rows(f.train_queries, 15)), torch.zeros((cap, 15), device=dev)],
                        [targets0.clone(), torch.zeros((cap, 3), device=dev)])
    fp = F.FrameParams(S, T, f.num_training_records, F.RenderMode.Full, 3, 0, 1)

    def new_net():
        net = nrc.Network()
        net.init(stream=stream)
        bench_weights(nrc, net, torch, dev, 1)
        return net

    out = {}
    try:
        for source in ("feistel", "shuffle_keys"):
            fb.shuffle_keys = t(keys) if source == "shuffle_keys" else None
            rec = {}
            if len(knobs) == 2:
                first = {}
                for knob in knobs:
                    nrc._lib.set_knob(KNOB, knob)
                    net = new_net()
                    fb.train_targets[0].copy_(targets0)
                    loss = F.process_frame(net, fb, fp)
                    first[knob] = [np.float32(loss)] + [net.get_state(s) for s in nrc.StateSlot]
                    net.destroy()
                rec["bitwise_equal_first_frame"] = all(np.array_equal(a, b) for a, b in zip(first[0], first[1]))
            net = new_net()

            def run_for(knob, seconds):
                if len(knobs) == 2:
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

            names = {0: "permute" if len(knobs) == 2 else "baseline", 1: "gather"}
            for order in ((0, 1), (1, 0)) if len(knobs) == 2 else ((0,),):
                rounds = {k: [] for k in order}
                for _ in range(args.rounds):
                    for knob in order:
                        run_for(knob, args.settle)
                        rounds[knob].append(run_for(knob, args.seconds))
                o = {}
                for knob in order:
                    m = float(np.median(rounds[knob]))
                    o[names[knob]] = {"us_median": m, "spread": (max(rounds[knob]) - min(rounds[knob])) / m,
                                      "rounds_us": rounds[knob]}
                if len(order) == 2:
                    o["gather_minus_permute_us"] = o["gather"]["us_median"] - o["permute"]["us_median"]
                rec["order_" + "_".join(map(str, order))] = o
            net.destroy()
            out[source] = rec
    finally:
        if len(knobs) == 2:
            nrc._lib.set_knob(KNOB, -1)
    print(json.dumps({"tree": "this" if tree == ROOT else tree.name, "screen": S, "tiles": T, "train": 1,
                      "records": int(f.num_training_records), "device": torch.cuda.get_device_properties(0).name,
                      "rounds": args.rounds, "seconds": args.seconds, "cases": out}, indent=1))


if __name__ == "__main__":
    main()
