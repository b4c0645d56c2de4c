#!/usr/bin/env python3
"""Gradient accumulation (optim.GradAccumulator, csrc/accum.hip): the accumulate kernel alone and inside the captured train step.

  (a) rn_grad_accumulate alone on R50-FPN's gradient set -- bf16 gradients for the conv weights, fp32 for BN / biases, fp32
      accumulators -- captured in a graph and replayed, at window position 0 (the accumulators are overwritten: 2 B read + 4 B
      written per bf16 element) and at a later position (read-modify-write: 10 B per bf16 element): us per call, GB/s and the
      fraction of the 6.29 TB/s copy ceiling, back to back and with the cache evicted by a 1 GiB fill before every replay;
  (b) bench.py's step -- R50-FPN, bf16 autocast, B = 8 at 3 x 800 x 1333, MasterSGD, graph.CapturedTrainStep -- with
      ``accumulate=GradAccumulator(N)`` over whole windows, for ``--rounds`` rounds: mean ms per micro-batch, host ms per call,
      captures, replays; then ``n`` rewritten between windows (no capture).
The yardstick of (b) is the PARENT commit's replayed step as ``python bench.py`` reports it on the same machine in the same visit:
pass its ms_per_step figures with ``--parent-ms`` (one per run) and its host figure with ``--parent-host-ms``.  Claim: mean ms per
micro-batch <= mean(parent) + (max - min)(parent) + the accumulate kernel's back-to-back time at a later position.
Prints one JSON line (and writes it to ``--out`` when given).

usage: accum_step.py [--n 4] [--windows 5] [--warmup-windows 3] [--rounds 3] [--iters 200] [--parent-ms A,B,C] [--parent-host-ms H]
                     [--skip-step] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth                                                        # noqa: E402
import pytorch_retinanet_amd as P                                   # noqa: E402
from pytorch_retinanet_amd import tuning                            # noqa: E402
from pytorch_retinanet_amd.graph import CapturedTrainStep           # noqa: E402
from pytorch_retinanet_amd.optim import GradAccumulator, MasterSGD, use_16bit_conv_weights   # noqa: E402

B, H, W = 8, 800, 1333
CEILING_TBS = 6.29


def r50(dev):
    torch.manual_seed(0)
    net = P.Retinanet(num_classes=90, backbone_kind="resnet50", pretrained=False, min_size=800, max_size=1333)
    net = net.to(dev).to(memory_format=torch.channels_last).train()
    use_16bit_conv_weights(net, torch.bfloat16)
    return net


def replay_times(graph, iters, evict=None):
    "Median / min us of ``graph.replay()`` over ``iters`` replays, each between its own pair of events (``evict``: filled before each)."
    out = []
    for _ in range(iters):
        if evict is not None:
            evict.fill_(1.0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        graph.replay()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3)
    return float(np.median(out)), float(np.min(out))


def back_to_back(graph, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3


def kernel_alone(net, iters):
    dev = next(net.parameters()).device
    g = torch.Generator(device=dev).manual_seed(1)
    params = list(net.parameters())
    for p in params:
        x = (torch.randn(p.shape, device=dev, generator=g) * 1e-3).to(p.dtype)
        p.grad = x.contiguous(memory_format=torch.channels_last) if p.dim() == 4 else x
    elems16 = sum(p.numel() for p in params if p.dtype != torch.float32)
    elems32 = sum(p.numel() for p in params if p.dtype == torch.float32)
    grad_bytes = 2 * elems16 + 4 * elems32
    acc = GradAccumulator(4)
    acc.accumulate(params)                                          # (creates the accumulators and the block; position stays 0)
    evict = torch.empty(1 << 28, dtype=torch.float32, device=dev)   # 1 GiB: four times the Infinity Cache
    res = {}
    for name, nbytes in (("position_0", grad_bytes + 4 * (elems16 + elems32)), ("position_1", grad_bytes + 8 * (elems16 + elems32))):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            acc.accumulate(params)                                  # (the accumulate launches alone: the position does not move)
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
        res[name] = r
        del graph
        if name == "position_0":
            acc.advance(False)                                      # position 1: the accumulators are read and added to from here on
    assert acc.position == 1 and float(acc.found_inf()) == 0.0
    res.update(gradient_tensors=len(params), gradient_elements=elems16 + elems32, gradient_bytes=grad_bytes)
    for p in params:
        p.grad = None
    del evict, acc
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup-windows", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--parent-ms", default="", help="the parent commit's bench.py ms_per_step figures of this visit, comma-separated")
    ap.add_argument("--parent-host-ms", type=float, default=None, help="the parent's host_enqueue_ms_per_step")
    ap.add_argument("--skip-step", action="store_true", help="(a) only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tuning.use_shipped_miopen_db(0)
    tuning.enable_conv_autotune()
    net = r50(dev)
    line = {"tool": "accum_step", "copy_ceiling_tb_per_s": CEILING_TBS, "iters": args.iters, "kernel_alone": kernel_alone(net, args.iters)}

    if not args.skip_step:
        n = args.n
        g = torch.Generator().manual_seed(0)
        images = [torch.rand(3, H, W, generator=g).to(dev) for _ in range(B)]
        rng = np.random.default_rng(7)
        tg = []
        for _ in range(B):
            b, l = synth.gt_boxes(rng, 8, H, W)
            tg.append({"boxes": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)})
        opt = MasterSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
        acc = GradAccumulator(n)
        stepper = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, eager_steps=2, accumulate=acc)
        for _ in range(args.warmup_windows * n):                    # (two eager and one capturing call of each kind, then replays)
            out = stepper(images, tg)
        per_round, host_round = [], []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            host = 0.0
            t0 = time.perf_counter()
            for _ in range(args.windows * n):
                h0 = time.perf_counter()
                out = stepper(images, tg)
                host += time.perf_counter() - h0
            torch.cuda.synchronize()
            per_round.append((time.perf_counter() - t0) / (args.windows * n) * 1e3)
            host_round.append(host / (args.windows * n) * 1e3)
        assert np.isfinite(float(out["loss"])), "non-finite loss"
        captures, replays = stepper.captures, stepper.replays
        acc.n = 2                                                   # n between windows: the next window is two micro-batches, no capture
        stepper(images, tg)
        stepper(images, tg)
        torch.cuda.synchronize()
        parent = [float(v) for v in args.parent_ms.split(",") if v]
        kernel_ms = line["kernel_alone"]["position_1"]["us_back_to_back"] / 1e3
        mean_ms = float(np.mean(per_round))
        line.update({
            "workload": f"R50-FPN bf16 train step, B={B} at 3x{H}x{W}, T=8, MasterSGD, accumulate_grad_batches={n}",
            "windows_per_round": args.windows, "rounds": args.rounds, "ms_per_micro_batch": round(mean_ms, 3),
            "per_round_ms": [round(v, 3) for v in per_round], "host_ms_per_call": round(float(np.mean(host_round)), 3),
            "captures": captures, "replays": replays, "captures_after_n_rewritten": stepper.captures, "position_after": acc.position,
            "accumulator_stats": acc.stats(), "graph_nodes": dict(P.graph.LAST_CENSUS) if hasattr(P, "graph") else None})
        if parent:
            spread = max(parent) - min(parent)
            bar = float(np.mean(parent)) + spread + kernel_ms
            line.update({"parent_bench_ms_per_step": parent, "parent_mean_ms": round(float(np.mean(parent)), 3),
                         "parent_spread_ms": round(spread, 3), "parent_host_ms_per_step": args.parent_host_ms,
                         "accumulate_kernel_ms": round(kernel_ms, 4), "bar_ms": round(bar, 3),
                         "excess_over_parent_ms": round(mean_ms - float(np.mean(parent)), 3), "within_bar": bool(mean_ms <= bar)})
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
