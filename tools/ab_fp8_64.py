"""In-process A/B of width-64 inference: the f16 production kernel against the FP8 kernel (nrc_infer8.hip) on ONE handle
configured with infer_precision FP8 (its f16 image is always there), through nrc_debug_infer_precision. bench.py's
state and query stream (tools/energy_ab.py bench_weights), interleaved rounds: per code, back-to-back launches for
--seconds after a --settle of the same launches, event-timed per chunk, while a sampler thread reads socket power and
the gfx clock (amdsmi, read-only). Codes: 0 = f16, 1 = FP8 (product shape), 17 = FP8 two tiles per wave iteration in
512-thread blocks (debug library only; skipped when the library does not have it).

    NRC_LIB_PATH=neural-radiance-caching_amd/libnrc_amd_debug.so python tools/ab_fp8_64.py > profiles/fp8_64/ab.json
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
from energy_ab import Sampler, bench_weights  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 21)
    ap.add_argument("--codes", default="0,1,17")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--settle", type=float, default=0.4)
    ap.add_argument("--chunk", type=int, default=50)
    args = ap.parse_args()
    import torch

    nrc = nrc_loader.load()
    L = nrc._lib.lib()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sp = int(stream.cuda_stream)
    enc = nrc.InputEncoding.Frequency
    net = nrc.Network()
    net.init(stream=stream, encoding=enc, config=nrc.default_config(enc, infer_precision=nrc._lib.PRECISION_FP8))
    q = torch.from_numpy(bench_weights(nrc, net, torch, dev, args.n)).to(dev)
    outs, codes = {}, []
    for c in (int(c) for c in args.codes.split(",")):
        o = torch.empty((args.n, 3), device=dev)
        if L.nrc_debug_infer_precision(net._h, c, q.data_ptr(), o.data_ptr(), args.n, sp) == 0:
            codes.append(c)
            outs[c] = o
    torch.cuda.synchronize()
    rel = lambda a, b: float(torch.linalg.norm(a - b) / torch.linalg.norm(b))  # noqa: E731
    check = {c: {"rel_l2_vs_f16": rel(outs[c], outs[0]) if 0 in outs else None,
                 "identical_to_fp8_product": bool(torch.equal(outs[c], outs[1])) if c != 1 and (c & 15) == 1 else None}
             for c in codes}
    out = outs[codes[0]]
    props = torch.cuda.get_device_properties(0)
    try:
        smp = Sampler(f"{props.pci_bus_id:02x}:{props.pci_device_id:02x}")
        smp.start()
    except Exception:  # no amdsmi: times only
        smp = None

    def run_for(c, seconds):
        us, launches, t0 = [], 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.chunk):
                L.nrc_debug_infer_precision(net._h, c, q.data_ptr(), out.data_ptr(), args.n, sp)
            e1.record(stream)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) / args.chunk * 1e3)
            launches += args.chunk
        return launches, us, t0, time.perf_counter()

    rounds = {c: [] for c in codes}
    for _ in range(args.rounds):
        for c in codes:
            run_for(c, args.settle)
            launches, us, t0, t1 = run_for(c, args.seconds)
            w = smp.window(t0, t1) if smp else {}
            rec = {"launches": launches, "us_median": float(np.median(us)), **w}
            if "power_w" in w:
                rec["nj_per_query"] = w["power_w"] * float(np.median(us)) * 1e-6 / args.n * 1e9
            rounds[c].append(rec)
    if smp:
        smp.stop()
    med = lambda c, k: float(np.median([x.get(k, np.nan) for x in rounds[c]]))  # noqa: E731
    res = {c: {"us_median": med(c, "us_median"), "gqueries_per_s": args.n / med(c, "us_median") * 1e-3,
               "power_w": med(c, "power_w"), "gfx_mhz": med(c, "gfx_mhz"), "nj_per_query": med(c, "nj_per_query"),
               **check[c], "rounds": rounds[c]} for c in codes}
    net.destroy()
    print(json.dumps({"n": args.n, "device": props.name, "codes": res}, indent=1))


if __name__ == "__main__":
    main()
