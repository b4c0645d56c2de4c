#!/usr/bin/env python3
"""Global-norm gradient clipping (optim.GradClip, csrc/clip.hip): the norm alone, against torch's clip, and inside the train step.

  (a) rn_grad_norm_clip (norm + finalize) alone on R50-FPN's gradient set -- bf16 gradients for the conv weights, fp32 for BN /
      biases -- captured in a graph and replayed: us per call, GB/s and the fraction of the 6.29 TB/s copy ceiling, warm (the set
      fits the 256 MB Infinity Cache) and with the cache evicted by a 1 GiB fill before every replay (timed with events around the
      replay alone);
  (b) torch.nn.utils.clip_grad_norm_ (foreach) on the same gradients, timed the same way.  (a) must not be slower than (b);
  (c) bench.py's step -- R50-FPN, bf16 autocast, B = 8 at 3 x 800 x 1333, graph.CapturedTrainStep -- with MasterSGD and with MasterAdamW,
      each with and without a clip, interleaved for ``--rounds`` rounds in one process: ms per step, host ms per step, captures;
      then max_norm rewritten between two replays of the clipped steppers (the coefficient follows, captures stays 1).
      Bar: clipped <= unclipped + (a) + the spread (max - min over the rounds) of the unclipped step.
Prints one JSON line (and writes it to ``--out`` when given).

usage: clip_step.py [--steps 20] [--warmup 4] [--rounds 3] [--iters 200] [--skip-step] [--out FILE]"""
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
from pytorch_retinanet_amd._lib import RN_BF16                      # noqa: E402
from pytorch_retinanet_amd.graph import CapturedTrainStep           # noqa: E402
from pytorch_retinanet_amd.optim import GradClip, MasterAdamW, MasterSGD, use_16bit_conv_weights   # noqa: E402

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


def norm_alone(net, iters):
    dev = next(net.parameters()).device
    g = torch.Generator(device=dev).manual_seed(1)
    grads = []
    for p in net.parameters():
        x = (torch.randn(p.shape, device=dev, generator=g) * 1e-3).to(p.dtype)
        grads.append(x.contiguous(memory_format=torch.channels_last) if p.dim() == 4 else x)
    nbytes = sum(x.numel() * x.element_size() for x in grads)
    clip = GradClip(1.0)
    args = ([x.data_ptr() for x in grads], [x.data_ptr() if x.dtype != torch.float32 else 0 for x in grads], [x.numel() for x in grads],
            RN_BF16, None, dev)
    clip.compute(*args)
    torch.cuda.synchronize()
    ours = torch.cuda.CUDAGraph()
    with torch.cuda.graph(ours):
        clip.compute(*args)
    params = [torch.nn.Parameter(torch.empty_like(x)) for x in grads]
    for q, x in zip(params, grads):
        q.grad = x
    torch.nn.utils.clip_grad_norm_(params, 1e30, foreach=True)      # (max_norm 1e30: the gradients are multiplied by 1.0, unchanged)
    torch.cuda.synchronize()
    theirs = torch.cuda.CUDAGraph()
    with torch.cuda.graph(theirs):
        torch.nn.utils.clip_grad_norm_(params, 1e30, foreach=True)
    evict = torch.empty(1 << 28, dtype=torch.float32, device=dev)   # 1 GiB: four times the Infinity Cache
    res = {}
    for name, graph in (("hip", ours), ("torch_foreach", theirs)):
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        b2b = back_to_back(graph, iters)
        warm_med, warm_min = replay_times(graph, iters)
        cold_med, cold_min = replay_times(graph, max(iters // 4, 10), evict)
        res[name] = {"us_back_to_back": round(b2b, 2), "us_warm_median": round(warm_med, 2), "us_warm_min": round(warm_min, 2),
                     "us_evicted_median": round(cold_med, 2), "us_evicted_min": round(cold_min, 2)}
    for k in ("us_back_to_back", "us_evicted_median"):
        gbs = nbytes / res["hip"][k] / 1e3
        res["hip"][k.replace("us_", "gb_per_s_")] = round(gbs, 1)
        res["hip"][k.replace("us_", "fraction_of_copy_ceiling_")] = round(gbs / 1e3 / CEILING_TBS, 3)
    res["total_norm"] = float(clip.total_norm)
    res["gradient_bytes"] = nbytes
    res["gradient_tensors"] = len(grads)
    res["gradient_elements"] = sum(x.numel() for x in grads)
    res["hip_not_slower_than_torch"] = bool(res["hip"]["us_back_to_back"] <= res["torch_foreach"]["us_back_to_back"]
                                            and res["hip"]["us_evicted_median"] <= res["torch_foreach"]["us_evicted_median"])
    del ours, theirs, evict
    return res


def timed(name, stepper, images, batches):
    torch.cuda.synchronize()
    host = 0.0
    t0 = time.perf_counter()
    for tg in batches:
        h0 = time.perf_counter()
        out = stepper(images, tg)
        host += time.perf_counter() - h0
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert np.isfinite(float(out["loss"])), f"{name}: non-finite loss"
    return wall / len(batches) * 1e3, host / len(batches) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--skip-step", action="store_true", help="(a) and (b) only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tuning.use_shipped_miopen_db(0)
    tuning.enable_conv_autotune()
    net = r50(dev)
    line = {"tool": "clip_step", "copy_ceiling_tb_per_s": CEILING_TBS, "iters": args.iters, "norm_alone": norm_alone(net, args.iters)}

    if not args.skip_step:
        g = torch.Generator().manual_seed(0)
        images = [torch.rand(3, H, W, generator=g).to(dev) for _ in range(B)]
        rng = np.random.default_rng(7)
        tg = []
        for _ in range(B):
            b, l = synth.gt_boxes(rng, 8, H, W)
            tg.append({"boxes": torch.from_numpy(b).to(dev), "labels": torch.from_numpy(l).to(dev)})
        batches = [tg] * (args.warmup + args.steps)
        mk = {"sgd": lambda c: MasterSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4, max_grad_norm=c),
              "adamw": lambda c: MasterAdamW(net.parameters(), lr=1e-5, weight_decay=1e-2, max_grad_norm=c)}
        opts = {f"{k}{'_clip' if c else ''}": mk[k](c) for k in mk for c in (None, 1.0)}
        phases = {k: CapturedTrainStep(net, o, amp_dtype=torch.bfloat16, eager_steps=2) for k, o in opts.items()}
        res = {k: [] for k in phases}
        for _ in range(args.rounds):
            for k, st in phases.items():
                for b in batches[:args.warmup]:
                    st(images, b)
                res[k].append(timed(k, st, images, batches[args.warmup:]))
        ms = {k: float(np.mean([v[0] for v in res[k]])) for k in res}
        host = {k: float(np.mean([v[1] for v in res[k]])) for k in res}
        spread = {k: float(np.max([v[0] for v in res[k]]) - np.min([v[0] for v in res[k]])) for k in res}
        norm_ms = line["norm_alone"]["hip"]["us_back_to_back"] / 1e3
        follows = {}
        for k in ("sgd_clip", "adamw_clip"):                            # max_norm between replays: the next coefficient follows, no capture
            clip, seen = opts[k].grad_clip, []
            for mn in (1e-4, 1e6):
                clip.max_norm = mn
                phases[k](images, tg)
                seen.append(float(clip.clip_coef))
            clip.max_norm = 1.0
            follows[k] = {"coef_at_1e-4": seen[0], "coef_at_1e6": seen[1], "followed": bool(seen[0] < 1.0 and seen[1] == 1.0)}
        line.update({
            "workload": f"R50-FPN bf16 train step, B={B} at 3x{H}x{W}, T=8", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
            "train_ms_per_step": {k: round(v, 3) for k, v in ms.items()}, "host_ms_per_step": {k: round(v, 3) for k, v in host.items()},
            "per_round_ms": {k: [round(v[0], 3) for v in res[k]] for k in res}, "spread_ms": {k: round(v, 3) for k, v in spread.items()},
            "clip_cost_ms": {k: round(ms[k + "_clip"] - ms[k], 3) for k in mk},
            "clip_cost_bar_ms": {k: round(norm_ms + spread[k], 3) for k in mk},
            "clip_cost_within_bar": {k: bool(ms[k + "_clip"] - ms[k] <= norm_ms + spread[k]) for k in mk},
            "captures": {k: phases[k].captures for k in phases}, "replays": {k: phases[k].replays for k in phases},
            "max_norm_between_replays": follows, "clip_stats": {k: opts[k].grad_clip.stats() for k in ("sgd_clip", "adamw_clip")}})
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
