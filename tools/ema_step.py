#!/usr/bin/env python3
"""The weight average (optim.WeightEMA, csrc/ema.hip): the update alone, torch's foreach restatement of it, and the update inside the
captured train step.

  (a) rn_ema_update + rn_ema_advance alone on R50-FPN's fp32 master set (4 B read of the master, 4 B read and 4 B written of the
      average: 12 B per element), captured in a graph and replayed: us per call, GB/s and the fraction of the 6.29 TB/s copy ceiling,
      back to back and with the cache evicted by a 1 GiB fill before every replay;
  (b) ``torch._foreach_lerp_(averages, masters, 1 - decay)`` on the same fp32 tensors, captured and replayed the same way, in the
      same run -- what a user would write by hand;
  (c) bench.py's step -- R50-FPN, bf16 autocast, B = 8 at 3 x 800 x 1333, MasterSGD, graph.CapturedTrainStep -- without and with
      ``optimizer.weight_ema``, alternating for ``--rounds`` rounds: mean ms per step, host ms per call, captures.
Claims: (a) <= (b); the step delta of (c) is of the size of (a) and the host time per call does not move.
Prints one JSON line (and writes it to ``--out`` when given).

usage: ema_step.py [--steps 20] [--warmup 6] [--rounds 3] [--iters 200] [--skip-step] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth                                                        # noqa: E402
from pytorch_retinanet_amd import tuning                            # noqa: E402
from pytorch_retinanet_amd.graph import CapturedTrainStep           # noqa: E402
from pytorch_retinanet_amd.optim import MasterSGD, WeightEMA        # noqa: E402
from accum_step import B, CEILING_TBS, H, W, back_to_back, r50, replay_times     # noqa: E402


def timed(graph, iters, nbytes, evict):
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    b2b = back_to_back(graph, iters)
    warm_med, warm_min = replay_times(graph, iters)
    cold_med, cold_min = replay_times(graph, max(iters // 4, 10), evict)
    r = {"bytes": nbytes, "us_back_to_back": round(b2b, 2), "us_warm_median": round(warm_med, 2), "us_warm_min": round(warm_min, 2),
         "us_evicted_median": round(cold_med, 2), "us_evicted_min": round(cold_min, 2)}
    for k in ("us_back_to_back", "us_evicted_median"):
        gbs = nbytes / r[k] / 1e3
        r[k.replace("us_", "gb_per_s_")] = round(gbs, 1)
        r[k.replace("us_", "fraction_of_copy_ceiling_")] = round(gbs / 1e3 / CEILING_TBS, 3)
    return r


def update_alone(net, iters):
    params = list(net.parameters())
    masters = [p.master if hasattr(p, "master") else p.data for p in params]
    elems = sum(w.numel() for w in masters)
    nbytes = 12 * elems
    evict = torch.empty(1 << 28, dtype=torch.float32, device=masters[0].device)      # 1 GiB: four times the Infinity Cache
    ema = WeightEMA(0.9998)
    ema.update(params)                                              # (creates the averages and the block; updates = 1 from here on)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ema.update(params)
    res = {"tensors": len(params), "elements": elems, "rn_ema_update": timed(graph, iters, nbytes, evict)}
    del graph
    avgs = [torch.empty_like(w).copy_(w) for w in masters]
    torch._foreach_lerp_(avgs, masters, 1.0 - 0.9998)               # (warm: nothing is allocated under the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        torch._foreach_lerp_(avgs, masters, 1.0 - 0.9998)
    res["torch_foreach_lerp"] = timed(graph, iters, nbytes, evict)
    del graph, avgs, evict
    a, b = res["rn_ema_update"], res["torch_foreach_lerp"]
    res["not_slower_than_foreach_lerp"] = bool(a["us_back_to_back"] <= b["us_back_to_back"] and a["us_evicted_median"] <= b["us_evicted_median"])
    res["updates_after"] = ema.updates
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--skip-step", action="store_true", help="(a) and (b) only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tuning.use_shipped_miopen_db(0)
    tuning.enable_conv_autotune()
    net = r50(dev)
    line = {"tool": "ema_step", "copy_ceiling_tb_per_s": CEILING_TBS, "iters": args.iters, "update_alone": update_alone(net, args.iters)}

    if not args.skip_step:
        g = torch.Generator().manual_seed(0)
        images = [torch.rand(3, H, W, generator=g).to(dev) for _ in range(B)]
        rng = np.random.default_rng(7)
        tg = []
        for _ in range(B):
            b, l = synth.gt_boxes(rng, 8, H, W)
            tg.append({"boxes": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)})
        opt = MasterSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
        stepper = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2)
        ema = WeightEMA(0.9998)
        per = {"without": [], "with": []}
        host = {"without": [], "with": []}
        for kind in ("without", "with"):                            # (two eager and one capturing call of each key, then replays)
            opt.weight_ema = ema if kind == "with" else None
            for _ in range(args.warmup):
                out = stepper(images, tg)
        for _ in range(args.rounds):
            for kind in ("without", "with"):
                opt.weight_ema = ema if kind == "with" else None
                stepper(images, tg)
                torch.cuda.synchronize()
                h = 0.0
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    h0 = time.perf_counter()
                    out = stepper(images, tg)
                    h += time.perf_counter() - h0
                torch.cuda.synchronize()
                per[kind].append((time.perf_counter() - t0) / args.steps * 1e3)
                host[kind].append(h / args.steps * 1e3)
        assert np.isfinite(float(out["loss"])), "non-finite loss"
        kernel_ms = line["update_alone"]["rn_ema_update"]["us_back_to_back"] / 1e3
        cold_ms = line["update_alone"]["rn_ema_update"]["us_evicted_median"] / 1e3
        m0, m1 = float(np.mean(per["without"])), float(np.mean(per["with"]))
        spread = max(per["without"]) - min(per["without"])
        line.update({
            "workload": f"R50-FPN bf16 train step, B={B} at 3x{H}x{W}, T=8, MasterSGD",
            "steps_per_round": args.steps, "rounds": args.rounds,
            "ms_per_step_without": round(m0, 3), "ms_per_step_with": round(m1, 3), "per_round_ms_without": [round(v, 3) for v in per["without"]],
            "per_round_ms_with": [round(v, 3) for v in per["with"]], "step_delta_ms": round(m1 - m0, 4), "update_ms_back_to_back": round(kernel_ms, 4),
            "update_ms_evicted": round(cold_ms, 4), "spread_without_ms": round(spread, 3),
            "delta_within_update_plus_spread": bool(m1 - m0 <= cold_ms + spread),
            "host_ms_per_call_without": round(float(np.mean(host["without"])), 3), "host_ms_per_call_with": round(float(np.mean(host["with"])), 3),
            "captures": stepper.captures, "replays": stepper.replays, "ema_stats": ema.stats()})
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
