#!/usr/bin/env python3
"""Out-of-bounds probe for the hand-written kernels: every INPUT tensor is placed at the very END of its own device mapping
(no caching allocator: one hipMalloc per tensor, 2 MiB granules), so a kernel that reads or writes past an operand runs off the
mapping and the GPU raises a memory access fault (the process aborts) instead of silently touching a neighbour.  Found this way:
``stem_fwd_kernel`` -- a wave of the last workgroup that owns no tile loaded at a tile index past the last image.

usage: guard_probe.py stem B H W | w3 N H W C | n3 N H W | dense | pw | pool | bottleneck | step KIND MIN MAX | detect DT B H W K [MEAN] |
       loss DT B H W K T | gt | affine | adam [bf16|f16] | clip [bf16|f16] | accum [bf16|f16]        (driven by tests/test_guard_gpu.py;
       gt: by tests/test_gt_capacity_gpu.py; affine: by tests/test_shift_scale_rotate_gpu.py; adam: by tests/test_master_adam_gpu.py; clip: by tests/test_grad_clip_gpu.py;
       accum: by tests/test_grad_accum_gpu.py; sgd_dev [bf16|f16]: by tests/test_master_sgd_capturable_gpu.py;
       softnms: by tests/test_soft_nms_gpu.py)
Prints one "ok ..." line per case; a fault kills the process (non-zero exit status, no "ok" line for the case)."""
import ctypes as C
import os
import sys

os.environ["PYTORCH_NO_CUDA_MEMORY_CACHING"] = "1"
import torch                                                       # noqa: E402
import torch.nn as nn                                              # noqa: E402

from pytorch_retinanet_amd._lib import RN_BF16, check, lib         # noqa: E402

DEV = torch.device("cuda:0")
GRAN = 2 << 20
_KEEP = []


def raw_at_end(nbytes: int, fill=None) -> torch.Tensor:
    tot = (nbytes + GRAN - 1) // GRAN * GRAN
    base = torch.empty((tot,), dtype=torch.uint8, device=DEV)
    base.fill_(0x7f if fill is None else fill)                     # bf16 0x7f7f = 3.4e38: a stray read of the padding shows in the results too
    _KEEP.append(base)
    off = (tot - nbytes) // 16 * 16
    return base[off: off + nbytes]


def cl_at_end(N: int, C: int, H: int, W: int, scale: float = 1.0, seed: int = 0) -> torch.Tensor:
    "bf16 channels-last [N, C, H, W] random tensor whose last byte is the last byte (mod 16) of its mapping"
    g = torch.Generator(device=DEV).manual_seed(seed)
    src = (torch.randn((N, H, W, C), device=DEV, generator=g) * scale).to(torch.bfloat16)
    raw = raw_at_end(src.numel() * 2)
    t = raw.view(torch.bfloat16).view(N, H, W, C)
    t.copy_(src)
    return t.permute(0, 3, 1, 2)


def main() -> None:
    which = sys.argv[1]
    st = torch.cuda.current_stream().cuda_stream
    if which == "stem":
        B, H, W = (int(v) for v in sys.argv[2:5])
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        x, w, g = raw_at_end(B * H * W * 3 * 2, 0x3c), raw_at_end(64 * 147 * 2, 0x3c), raw_at_end(B * Ho * Wo * 64 * 2, 0x3c)
        xp, wk, z = raw_at_end(lib.rn_stem_padded_bytes(B, H, W)), raw_at_end(64 * 7 * 32 * 2), raw_at_end(B * Ho * Wo * 64 * 2)
        part = raw_at_end(lib.rn_stem_partial_rows(B, H, W) * 2 * 64 * 4)
        check(lib.rn_stem_conv_forward(x.data_ptr(), w.data_ptr(), xp.data_ptr(), wk.data_ptr(), z.data_ptr(), part.data_ptr(), RN_BF16, B, H, W,
                                       st), "rn_stem_conv_forward")
        torch.cuda.synchronize()
        need = lib.rn_stem_wgrad_workspace_bytes(B, H, W)
        ws, dw = raw_at_end(need), raw_at_end(64 * 147 * 2)
        check(lib.rn_stem_conv_wgrad(g.data_ptr(), xp.data_ptr(), dw.data_ptr(), RN_BF16, B, H, W, ws.data_ptr(), need, st), "rn_stem_conv_wgrad")
        torch.cuda.synchronize()
        print("ok stem", B, H, W, flush=True)
    elif which == "w3":
        N, H, W, Cc = (int(v) for v in sys.argv[2:6])
        g, x = raw_at_end(N * H * W * Cc * 2, 0x3c), raw_at_end(N * H * W * Cc * 2, 0x3c)
        need = lib.rn_conv3x3_wgrad_narrow_workspace_bytes(Cc, Cc)
        dw, ws, zp = raw_at_end(Cc * Cc * 9 * 2), raw_at_end(need), raw_at_end(256, 0)
        check(lib.rn_conv3x3_wgrad_narrow(g.data_ptr(), x.data_ptr(), dw.data_ptr(), RN_BF16, N, H, W, Cc, Cc, zp.data_ptr(), ws.data_ptr(), need,
                                          st), "rn_conv3x3_wgrad_narrow")
        torch.cuda.synchronize()
        print("ok w3", N, H, W, Cc, flush=True)
    elif which == "n3":
        # forward product of the 64-channel 3x3 convolution (csrc/narrow3x3.hip): LDS-DMA row staging with a zero page for the halo
        N, H, W = (int(v) for v in sys.argv[2:5])
        x, w = raw_at_end(N * H * W * 64 * 2, 0x3c), raw_at_end(64 * 64 * 9 * 2, 0x3c)
        y, zp = raw_at_end(N * H * W * 64 * 2), raw_at_end(256, 0)
        check(lib.rn_conv3x3_narrow_forward(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), RN_BF16, N, H, W, 64, 0, zp.data_ptr(), st), "rn_conv3x3_narrow_forward")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y.view(torch.bfloat16).float()).all()), "a pixel outside the image was read"       # (padding is 3.4e38: 9 * 64 of them overflow)
        print("ok n3", N, H, W, flush=True)
    elif which == "dense":
        from pytorch_retinanet_amd import biasact
        for N, shapes in [(2, [(25, 42), (13, 21), (7, 11)]), (1, [(1, 300), (3, 1), (2, 2)]), (3, [(9, 30)])]:
            convs = [nn.Conv2d(256, 256, 3, 1, 1).to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last) for _ in shapes]
            for c in convs:
                c.bias.data = c.bias.data.float()
            xs = [cl_at_end(N, 256, h, w, seed=i).requires_grad_() for i, (h, w) in enumerate(shapes)]
            ys = biasact.dense_conv_group(xs, convs)
            torch.autograd.backward(ys, [cl_at_end(N, 256, h, w, seed=9 + i) for i, (h, w) in enumerate(shapes)])
            torch.cuda.synchronize()
            # layer3's conv2: forward and both gradients, P = 1
            c2 = nn.Conv2d(256, 256, 3, 1, 1, bias=False).to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last)
            x2 = cl_at_end(N, 256, *shapes[0], seed=5).requires_grad_()
            biasact.conv3x3_mfma_bwd(c2, x2).backward(cl_at_end(N, 256, *shapes[0], seed=6))
            torch.cuda.synchronize()
            print("ok dense", N, shapes, flush=True)
    elif which == "pw":
        from pytorch_retinanet_amd import pwconv
        for (N, cin, cout, H, W, k, s) in [(2, 64, 256, 9, 13, 1, 1), (1, 256, 64, 7, 5, 1, 1), (2, 128, 128, 11, 14, 3, 1), (2, 128, 128, 11, 14, 3, 2),
                                           (1, 512, 1024, 6, 10, 1, 2), (3, 1024, 256, 5, 3, 1, 1)]:
            x = cl_at_end(N, cin, H, W, seed=1)
            w = cl_at_end(cout, cin, k, k, 0.05, seed=2)
            y = pwconv.pw_forward(x, w, stride=s)
            g = cl_at_end(*y.shape, seed=3)
            pwconv.pw_wgrad(g, x, w, stride=s)
            torch.cuda.synchronize()
            print("ok pw", N, cin, cout, H, W, k, s, flush=True)
    elif which == "pool":
        from pytorch_retinanet_amd.pool import FusedMaxPool2d
        for (N, Cc, H, W) in [(2, 64, 37, 53), (1, 64, 1, 1), (1, 8, 5, 2), (2, 64, 30, 301)]:
            x = cl_at_end(N, Cc, H, W, seed=1).requires_grad_()
            y = FusedMaxPool2d(3, 2, 1)(x)
            y.backward(cl_at_end(*y.shape, seed=2))
            torch.cuda.synchronize()
            print("ok pool", N, Cc, H, W, flush=True)
    elif which == "bottleneck":
        from pytorch_retinanet_amd import backbone, optim
        for (inpl, planes, stride, H, W) in [(64, 64, 1, 19, 27), (256, 64, 1, 19, 27), (256, 128, 2, 18, 26), (1024, 512, 2, 7, 9), (2048, 512, 1, 5, 7)]:
            ds = None
            if stride != 1 or inpl != planes * 4:
                ds = nn.Sequential(nn.Conv2d(inpl, planes * 4, 1, stride, bias=False), backbone.FusedBatchNorm2d(planes * 4))
            blk = backbone.Bottleneck(inpl, planes, stride, ds).to(DEV).to(memory_format=torch.channels_last).train()
            for m in blk.modules():
                if isinstance(m, nn.Conv2d):
                    m.weight.data = m.weight.data.to(torch.bfloat16)
            x = cl_at_end(2, inpl, H, W, seed=1).requires_grad_()
            y = blk(x)
            y.backward(cl_at_end(*y.shape, seed=2))
            torch.cuda.synchronize()
            print("ok bottleneck", inpl, planes, stride, H, W, flush=True)
    elif which == "step":
        # whole train steps + one inference pass with one device allocation per tensor (page-granular mappings: an overrun of more
        # than a page past ANY tensor of the step faults), R50 trunk, odd image sizes, eager
        import numpy as np
        import pytorch_retinanet_amd as P
        import synth
        from pytorch_retinanet_amd.graph import CapturedTrainStep
        from pytorch_retinanet_amd.optim import MasterSGD, use_bf16_conv_weights
        torch.manual_seed(3)
        kind, lo, hi = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        net = P.Retinanet(num_classes=7, backbone_kind=kind, pretrained=False, min_size=lo, max_size=hi).to(DEV)
        net = net.to(memory_format=torch.channels_last).train()
        use_bf16_conv_weights(net)
        opt = MasterSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
        step = CapturedTrainStep(net, opt, amp_dtype=torch.bfloat16, enabled=False)
        rng = np.random.default_rng(1)
        for hw in [(lo - 3, hi - 7), (lo + 5, hi - 21)]:
            images = [torch.from_numpy(rng.random((3, *hw), dtype=np.float32)).to(DEV) for _ in range(2)]
            targets = []
            for _ in range(2):
                b, l = synth.gt_boxes(rng, 4, hw[0], hw[1], num_classes=7, wh_lo=20.0, wh_hi=90.0)
                targets.append({"boxes": torch.from_numpy(b).to(DEV), "labels": torch.from_numpy(l).to(DEV)})
            loss = float(step(images, targets)["loss"])
            assert loss == loss, "loss is NaN"
        net.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            net([torch.from_numpy(rng.random((3, lo - 1, hi - 2), dtype=np.float32)).to(DEV)])
        torch.cuda.synchronize()
        print("ok step", kind, lo, hi, flush=True)
    elif which == "detect":
        # K4-K7 (rn_detect_levels): every per-level logit / delta tensor, the anchors and the image sizes at the end of their own mappings
        import numpy as np
        import synth
        from pytorch_retinanet_amd import ops
        from pytorch_retinanet_amd.anchors import AnchorGenerator
        dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[sys.argv[2]]
        B, H, W, K = (int(v) for v in sys.argv[3:7])
        mean = float(sys.argv[7]) if len(sys.argv) > 7 else -4.6
        std, dstd = (float(sys.argv[8]), float(sys.argv[9])) if len(sys.argv) > 9 else (1.2, 0.1)
        levels = synth.levels_for(H, W)
        ag = AnchorGenerator().to(DEV)
        anc_src = ops.anchors_emit(levels, list(ag.cell_anchors), 0.0)
        anc = raw_at_end(anc_src.numel() * 4).view(torch.float32).view(-1, 4)
        anc.copy_(anc_src)
        g = torch.Generator(device=DEV).manual_seed(1)
        cl, bl = [], []
        for (h, w, _) in levels:
            n = h * w * 9
            c = raw_at_end(B * n * K * dt.itemsize).view(dt).view(B, n, K)
            c.copy_((torch.randn((B, n, K), device=DEV, generator=g) * std + mean).to(dt))
            d = raw_at_end(B * n * 4 * dt.itemsize).view(dt).view(B, n, 4)
            d.copy_((torch.randn((B, n, 4), device=DEV, generator=g) * dstd).to(dt))
            cl.append(c); bl.append(d)
        dets = ops.detect_levels(cl, bl, anc, [(H - 5, W - 3)] * B, 0.05, 1e-2, 0.5, 100)
        torch.cuda.synchronize()
        print("ok detect", sys.argv[2], B, H, W, K, mean, [int(d["scores"].numel()) for d in dets], flush=True)
    elif which == "loss":
        # K2 + K3 (rn_iou_match_special + rn_loss_fwd_bwd_levels_ex, and the one-launch form): per-level logits / deltas, anchors, GT
        # boxes / labels / offsets at the end of their own mappings; ragged GT counts incl. an image without GT
        import numpy as np
        import synth
        from pytorch_retinanet_amd import ops
        from pytorch_retinanet_amd.anchors import AnchorGenerator
        dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[sys.argv[2]]
        B, H, W, K, T = (int(v) for v in sys.argv[3:8])
        levels = synth.levels_for(H, W)
        ag = AnchorGenerator().to(DEV)
        anc_src = ops.anchors_emit(levels, list(ag.cell_anchors), 0.0)
        anc = raw_at_end(anc_src.numel() * 4).view(torch.float32).view(-1, 4)
        anc.copy_(anc_src)
        rng = np.random.default_rng(2)
        Ts = [T if i != 1 else 0 for i in range(B)]
        gtb, gtl = zip(*[synth.gt_boxes(rng, t, H, W, num_classes=K, wh_lo=20.0, wh_hi=min(H, W) * 0.6) for t in Ts])
        gb = np.concatenate(gtb).astype(np.float32); gl = np.concatenate(gtl).astype(np.int64)
        gt_t = raw_at_end(max(gb.size, 4) * 4).view(torch.float32)[:gb.size].view(-1, 4); gt_t.copy_(torch.from_numpy(gb))
        gl_t = raw_at_end(max(gl.size, 1) * 8).view(torch.int64)[:gl.size]; gl_t.copy_(torch.from_numpy(gl))
        off_src = ops.gt_offsets(Ts, DEV)
        off = raw_at_end(off_src.numel() * 4).view(torch.int32); off.copy_(off_src)
        g = torch.Generator(device=DEV).manual_seed(1)
        cl, bl = [], []
        for (h, w, _) in levels:
            n = h * w * 9
            c = raw_at_end(B * n * K * dt.itemsize).view(dt).view(B, n, K)
            c.copy_((torch.randn((B, n, K), device=DEV, generator=g) - 4.6).to(dt))
            d = raw_at_end(B * n * 4 * dt.itemsize).view(dt).view(B, n, 4)
            d.copy_((torch.randn((B, n, 4), device=DEV, generator=g) * 0.1).to(dt))
            cl.append(c); bl.append(d)
        p = ops.make_loss_params(0.25, 2.0, 0.1)
        m, nfg, sp = ops.iou_match(anc, gt_t, off, B, 0.5, 0.4, want_special=True)
        loss, gc, gbx = ops.loss_fwd_bwd_levels(cl, bl, anc, gt_t, gl_t, off, m, nfg, p, True, special=sp)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss).all())
        if max(Ts) <= 64:
            out = ops.loss_match_fwd_bwd_levels(cl, bl, anc, gt_t, gl_t, off, max(Ts), 0.5, 0.4, p, True, want_matches=True)
            torch.cuda.synchronize()
            assert out is None or (torch.equal(out[0], loss) and torch.equal(out[4], m))
        print("ok loss", sys.argv[2], B, H, W, K, T, [float(x) for x in loss], flush=True)
    elif which == "gt":
        # rn_gt_stage + rn_gt_scale_packed (csrc/gt.hip): every per-image box / label tensor, the packed outputs and the offsets end
        # EXACTLY at the end of their mappings (a 1-box label tensor is 8 bytes: a 16-byte read of it would fault); B = 70: two launches
        from pytorch_retinanet_amd import ops

        def exact_end(n: int, dtype, fill=0x7f):
            nbytes = max(n, 1) * dtype.itemsize
            tot = (nbytes + GRAN - 1) // GRAN * GRAN
            base = torch.empty((tot,), dtype=torch.uint8, device=DEV)
            base.fill_(fill)
            _KEEP.append(base)
            return base[tot - n * dtype.itemsize:].view(dtype)
        B, cap = 70, 9
        counts = [(i * 7) % (cap + 1) for i in range(B)]
        counts[3], counts[B - 1] = 1, 1
        g = torch.Generator(device=DEV).manual_seed(4)
        boxes, labels = [], []
        for c in counts:
            b = exact_end(4 * c, torch.float32).view(c, 4); b.copy_(torch.rand((c, 4), device=DEV, generator=g) * 500)
            l = exact_end(c, torch.int64); l.copy_(torch.randint(1, 90, (c,), device=DEV, generator=g))
            boxes.append(b); labels.append(l)
        R = B * cap
        out = ops.PackedGT(exact_end(4 * R, torch.float32).view(R, 4), exact_end(R, torch.int64), exact_end(B + 1, torch.int32),
                           exact_end(B, torch.int32), cap)
        ops.gt_stage(boxes, labels, out)
        ratios = [(1.5, 0.75) if i % 2 else (1.0, 2.0) for i in range(B)]
        dst = exact_end(4 * R, torch.float32).view(R, 4)
        check(lib.rn_gt_scale_packed(out.gt_boxes.data_ptr(), dst.data_ptr(), out.gt_off.data_ptr(),
                                     (C.c_float * (2 * B))(*[v for r in ratios for v in r]), B, R, cap, st), "rn_gt_scale_packed")
        torch.cuda.synchronize()
        n = sum(counts)
        assert torch.equal(out.gt_boxes[:n], torch.cat(boxes)) and torch.equal(out.gt_labels[:n], torch.cat(labels))
        assert out.gt_off.tolist() == [sum(counts[:i]) for i in range(B + 1)] and int(out.num_fg.abs().sum()) == 0
        sc = torch.tensor([[rw, rh, rw, rh] for (rh, rw), c in zip(ratios, counts) for _ in range(c)], device=DEV)
        assert torch.equal(dst[:n], out.gt_boxes[:n] * sc)
        print("ok gt", B, cap, n, flush=True)
    elif which == "affine":
        # rn_affine_draw + rn_image_warp_stage (csrc/affine.hip) on hostile device data: the state block, the packed GT, the offsets,
        # the sizes, the coefficients, both arenas and every output end EXACTLY at the end of their mappings.  Image 1 claims h = 0,
        # image 3 a size no slot holds; gt_off starts below 0 and ends past rows.  Everything else must come out as the restatement says.
        from pytorch_retinanet_amd import draw_state, ops
        from pytorch_retinanet_amd.augment import AffineCoefs, ShiftScaleRotate

        def exact_end(n: int, dtype, fill=0x7f):
            nbytes = max(n, 1) * dtype.itemsize
            tot = (nbytes + GRAN - 1) // GRAN * GRAN
            base = torch.empty((tot,), dtype=torch.uint8, device=DEV)
            base.fill_(fill)
            _KEEP.append(base)
            return base[tot - n * dtype.itemsize:].view(dtype)
        sizes = [(37, 53), (20, 24), (64, 40), (9, 11), (1, 9)]
        B, slot, R = len(sizes), 3 * 64 * 40, 12
        g = torch.Generator(device=DEV).manual_seed(8)
        ims = [torch.rand((3, h, w), device=DEV, generator=g) for h, w in sizes]
        arena = exact_end(B * slot, torch.float32).view(B, slot)
        arena.fill_(-7.25)
        for b, im in enumerate(ims):
            arena[b, : im.numel()] = im.reshape(-1)
        hostile = [(37, 53), (0, 24), (64, 40), (30000, 30000), (1, 9)]
        in_hw = exact_end(2 * B, torch.int32).view(B, 2)
        in_hw.copy_(torch.tensor(hostile, dtype=torch.int32))
        boxes = torch.tensor([[3.5, 4.0, 20.0, 30.0], [49.0, 1.0, 52.5, 4.0], [10.0, 2.0, 40.25, 12.0], [2.0, 3.0, 9.0, 12.0],
                              [5.0, 6.0, 20.0, 50.0], [36.0, 0.5, 39.5, 3.0], [22.0, 30.0, 38.5, 61.0], [1.0, 1.0, 5.0, 6.0], [2.0, 0.0, 7.0, 1.0]])
        n = boxes.shape[0]
        gt_boxes = exact_end(4 * R, torch.float32).view(R, 4)
        gt_boxes.fill_(-7.25)
        gt_boxes[:n] = boxes.to(DEV)
        gt_labels = exact_end(R, torch.int64)
        gt_labels.copy_(torch.arange(1, R + 1, device=DEV))
        off = [-5, 3, 4, 7, 8, R + 9]                                  # clamped: 0, 3, 4, 7, 8, R -- image 4 owns rows 8 .. R - 1
        gt_off = exact_end(B + 1, torch.int32)
        gt_off.copy_(torch.tensor(off, dtype=torch.int32))
        clamped = [min(max(v, 0), R) for v in off]
        block = exact_end(ops.AFFINE_STATE_BYTES, torch.uint8)
        draw_state.write(draw_state.AFFINE, block, seed=2, counter=0, p=1.0, min_visibility=0.0, lo=(-45.0, 0.9, -0.0625, -0.0625), hi=(45.0, 1.1, 0.0625, 0.0625))
        coef = exact_end(B * ops.AFFINE_COEF_WORDS, torch.int32).view(B, ops.AFFINE_COEF_WORDS)
        out_boxes, out_labels, out_off = exact_end(4 * R, torch.float32).view(R, 4), exact_end(R, torch.int64), exact_end(B + 1, torch.int32)
        out_boxes.fill_(-7.25)
        check(lib.rn_affine_draw(block.data_ptr(), gt_boxes.data_ptr(), gt_labels.data_ptr(), gt_off.data_ptr(), in_hw.data_ptr(), B,
                                 coef.data_ptr(), out_boxes.data_ptr(), out_labels.data_ptr(), out_off.data_ptr(), R, st), "rn_affine_draw")
        dst = exact_end(B * slot, torch.float32).view(B, slot)
        dst.fill_(-7.25)
        check(lib.rn_image_warp_stage(arena.data_ptr(), slot, in_hw.data_ptr(), coef.data_ptr(), B, dst.data_ptr(), slot, st), "rn_image_warp_stage")
        torch.cuda.synchronize()
        c = AffineCoefs.from_device(coef)
        rows_in = gt_boxes.cpu()
        per = [rows_in[lo:hi] for lo, hi in zip(clamped[:-1], clamped[1:])]
        host = ShiftScaleRotate.draw_coefs(2, 0, hostile, per, 1.0, (-45.0, 0.9, -0.0625, -0.0625), (45.0, 1.1, 0.0625, 0.0625))
        assert c.applied == host.applied and not c.applied[1] and c.applied[0] and c.applied[2], c.applied      # (h < 1: left alone)
        lab = [gt_labels.cpu()[lo:hi] for lo, hi in zip(clamped[:-1], clamped[1:])]
        want = ShiftScaleRotate.warp_boxes(c, hostile, per, lab)
        counts = [int(w[0].shape[0]) for w in want]
        assert out_off.tolist() == [min(sum(counts[:i]), R) for i in range(B + 1)], (out_off.tolist(), counts)
        total = out_off.tolist()[-1]
        assert torch.equal(out_boxes.cpu()[:total].view(torch.int32), torch.cat([w[0] for w in want])[:total].view(torch.int32))
        assert torch.equal(out_labels.cpu()[:total], torch.cat([w[1] for w in want])[:total])
        assert bool((out_boxes[total:] == -7.25).all()) and draw_state.read(draw_state.AFFINE, block)[1] == 1
        for b, im in enumerate(ims):
            if b in (1, 3):                                                        # skipped: the slot is as it was
                assert bool((dst[b] == -7.25).all()), b
                continue
            ref = ShiftScaleRotate.warp_image(im, c.inv[b], c.applied[b]).reshape(-1)
            assert torch.equal(dst[b, : ref.numel()].view(torch.int32), ref.view(torch.int32)), b
            assert bool((dst[b, ref.numel():] == -7.25).all()), b
        print("ok affine", B, counts, total, flush=True)
    elif which == "adam":
        # rn_adam_master_step (csrc/adam.hip): 45 tensors (two launches of 40 + 5), every master / moment / gradient / 16-bit copy,
        # the hparams block and the GradScaler scalars at the end of their own mappings; sizes through the scalar tail path.
        # Three steps against torch.optim.AdamW(foreach=False) on fp32 copies.
        from pytorch_retinanet_amd._lib import RN_F16
        sizes = [1, 3, 4, 5, 1023, 4097, 64 * 3 * 7 * 7 + 2] + [(i * 37) % 301 + 1 for i in range(38)]
        dt = torch.bfloat16 if len(sys.argv) < 3 or sys.argv[2] == "bf16" else torch.float16
        g = torch.Generator(device=DEV).manual_seed(9)

        def at_end(src: torch.Tensor) -> torch.Tensor:
            t = raw_at_end(src.numel() * src.element_size()).view(src.dtype)
            t.copy_(src.reshape(-1))
            return t
        n_t = len(sizes)
        with16 = [i % 3 != 0 for i in range(n_t)]                       # (BN-like plain fp32 tensors between the 16-bit ones)
        w32 = [torch.randn(n, device=DEV, generator=g) for n in sizes]
        masters = [at_end(w) for w in w32]
        p16 = [at_end(w.to(dt)) if h else None for w, h in zip(w32, with16)]
        ms = [at_end(torch.zeros(n, device=DEV)) for n in sizes]
        vs = [at_end(torch.zeros(n, device=DEV)) for n in sizes]
        hp = at_end(torch.zeros(16, dtype=torch.float64, device=DEV))
        scale, found = at_end(torch.full((1,), 8.0, device=DEV)), at_end(torch.zeros(1, device=DEV))
        ref = [w.clone().requires_grad_(False) for w in w32]
        ropt = torch.optim.AdamW([torch.nn.Parameter(r) for r in ref], lr=1e-2, weight_decay=0.1, foreach=False)
        for step in range(3):
            lr = 1e-2 * (1.0 + 0.5 * step)
            gs = [torch.randn(n, device=DEV, generator=g) for n in sizes]
            gs16 = [x.to(dt) if h else x for x, h in zip(gs, with16)]
            gd = [at_end(x * 8.0) for x in gs16]                         # (scaled by the GradScaler's 8: exact)
            check(lib.rn_adam_hparams_set(hp.data_ptr(), lr, 0.9, 0.999, 1e-8, 0.1, -1.0, st), "rn_adam_hparams_set")
            ptrs = lambda ts: (C.c_void_p * n_t)(*[t.data_ptr() if t is not None else 0 for t in ts])
            check(lib.rn_adam_master_step(ptrs(masters), ptrs(ms), ptrs(vs), ptrs(gd), ptrs(p16), (C.c_int64 * n_t)(*sizes), n_t, 1,
                                          RN_F16 if dt == torch.float16 else RN_BF16, 1, hp.data_ptr(), scale.data_ptr(), found.data_ptr(),
                                          None, st), "rn_adam_master_step")
            for prm, x in zip(ropt.param_groups[0]["params"], gs16):
                prm.grad = x.float()
            ropt.param_groups[0]["lr"] = lr
            ropt.step()
        torch.cuda.synchronize()
        worst = 0.0
        for mst, c16, prm in zip(masters, p16, ropt.param_groups[0]["params"]):
            d = float(((mst - prm.detach()).abs() / (prm.detach().abs() + 1e-4)).max())
            worst = max(worst, d)
            if c16 is not None:
                assert torch.equal(c16, mst.to(dt)), "16-bit copy != round(master)"
        assert worst < 1e-4, worst
        assert float(hp[5]) == 3.0, float(hp[5])
        print("ok adam", str(dt), n_t, f"{worst:.2e}", flush=True)
    elif which == "sgd_dev":
        # rn_sgd_master_step_dev (csrc/optim.hip): 52 tensors (two launches of 48 + 4), every master / momentum buffer / gradient /
        # 16-bit copy, the 32-byte hparams block and the GradScaler scalars at the end of their own mappings; sizes through the
        # scalar tail path.  Three steps (the first reads no buffer) against rn_sgd_master_step on ordinary copies, bit for bit.
        from pytorch_retinanet_amd._lib import RN_F16
        sizes = [1, 3, 4, 5, 1023, 4097, 64 * 3 * 7 * 7 + 2] + [(i * 37) % 301 + 1 for i in range(45)]
        dt = torch.bfloat16 if len(sys.argv) < 3 or sys.argv[2] == "bf16" else torch.float16
        dt16 = RN_F16 if dt == torch.float16 else RN_BF16
        g = torch.Generator(device=DEV).manual_seed(15)

        def at_end(src: torch.Tensor) -> torch.Tensor:
            t = raw_at_end(src.numel() * src.element_size()).view(src.dtype)
            t.copy_(src.reshape(-1))
            return t
        n_t = len(sizes)
        with16 = [i % 3 != 0 for i in range(n_t)]
        w32 = [torch.randn(n, device=DEV, generator=g) for n in sizes]
        masters, ref_m = [at_end(w) for w in w32], [w.clone() for w in w32]
        p16 = [at_end(w.to(dt)) if h else None for w, h in zip(w32, with16)]
        ref_p16 = [w.to(dt) if h else None for w, h in zip(w32, with16)]
        moms, ref_moms = [at_end(torch.zeros(n, device=DEV)) for n in sizes], [torch.zeros(n, device=DEV) for n in sizes]
        hp = at_end(torch.zeros(8, dtype=torch.int32, device=DEV))
        scale, found = at_end(torch.full((1,), 8.0, device=DEV)), at_end(torch.zeros(1, device=DEV))
        ptrs = lambda ts: (C.c_void_p * n_t)(*[t.data_ptr() if t is not None else 0 for t in ts])
        for step in range(3):
            lr = 1e-2 * (1.0 + 0.5 * step)
            gs = [torch.randn(n, device=DEV, generator=g) for n in sizes]
            gs = [(x.to(dt) if h else x) * 8.0 for x, h in zip(gs, with16)]       # (scaled by the GradScaler's 8: exact)
            gd = [at_end(x) for x in gs]
            check(lib.rn_sgd_hparams_set(hp.data_ptr(), lr, 0.9, 0.1, 1e-4, 0, -1, st), "rn_sgd_hparams_set")
            check(lib.rn_sgd_master_step_dev(ptrs(masters), ptrs(moms), ptrs(gd), ptrs(p16), (C.c_int64 * n_t)(*sizes), n_t, 1, dt16, 1,
                                             hp.data_ptr(), scale.data_ptr(), found.data_ptr(), None, st), "rn_sgd_master_step_dev")
            check(lib.rn_sgd_master_step(ptrs(ref_m), ptrs(ref_moms), ptrs(gs), ptrs(ref_p16), (C.c_int64 * n_t)(*sizes), n_t, 1, dt16, lr, 0.9,
                                         0.1, 1e-4, 0, int(step == 0), scale.data_ptr(), found.data_ptr(), None, st), "rn_sgd_master_step")
        torch.cuda.synchronize()
        for a, b in zip(masters + moms + [c for c in p16 if c is not None], ref_m + ref_moms + [c for c in ref_p16 if c is not None]):
            assert torch.equal(a, b), "device-block step != by-value step"
        assert hp.tolist()[5:7] == [3, 0], hp.tolist()
        print("ok sgd_dev", str(dt), n_t, flush=True)
    elif which == "clip":
        # rn_grad_norm_clip + rn_sgd_master_step + rn_adam_master_step with a clip_coef (csrc/clip.hip, optim.hip, adam.hip): 230 tensors (two
        # norm launches of 224 + 6), every gradient ENDING at the last byte its alignment contract allows in its own mapping (16-bit
        # gradients 8-byte aligned: the norm kernel's head path; sizes through the tail paths; one tensor of three chunks), the
        # scratch buffer of exactly the required slots and the clip block at the end of theirs.  The norm against float64, the two
        # steps against torch fed g * coef.
        from pytorch_retinanet_amd._lib import RN_F16
        from pytorch_retinanet_amd.optim import GradClip
        sizes = [1, 3, 4, 5, 7, 8, 9, 1023, 4097, 16384, 16385, 2 * 16384 + 11] + [(i * 37) % 301 + 1 for i in range(218)]
        dt = torch.bfloat16 if len(sys.argv) < 3 or sys.argv[2] == "bf16" else torch.float16
        dt16 = RN_F16 if dt == torch.float16 else RN_BF16
        g = torch.Generator(device=DEV).manual_seed(11)

        def at_end(src: torch.Tensor, align: int = 16) -> torch.Tensor:
            nbytes = src.numel() * src.element_size()
            tot = (nbytes + GRAN - 1) // GRAN * GRAN
            base = torch.empty((tot,), dtype=torch.uint8, device=DEV)
            base.fill_(0x7f)
            _KEEP.append(base)
            off = (tot - nbytes) // align * align
            t = base[off: off + nbytes].view(src.dtype)
            t.copy_(src.reshape(-1))
            return t
        n_t = len(sizes)
        with16 = [i % 3 != 0 for i in range(n_t)]
        w32 = [torch.randn(n, device=DEV, generator=g) for n in sizes]
        gs = [(torch.randn(n, device=DEV, generator=g) * 0.1) for n in sizes]
        gs = [x.to(dt) if h else x for x, h in zip(gs, with16)]
        gd = [at_end(x * 8.0, 8 if h else 16) for x, h in zip(gs, with16)]            # (scaled by the GradScaler's 8: exact)
        slots = sum((n + 16383) // 16384 for n in sizes)
        scratch = at_end(torch.zeros(slots, dtype=torch.float64, device=DEV), 8)
        blk = at_end(torch.zeros(8, dtype=torch.float64, device=DEV), 8)
        scale, found = at_end(torch.full((1,), 8.0, device=DEV), 4), at_end(torch.zeros(1, device=DEV), 4)
        ptrs = lambda ts: (C.c_void_p * n_t)(*[t.data_ptr() if t is not None else 0 for t in ts])
        check(lib.rn_grad_clip_set(blk.data_ptr(), 0.5, st), "rn_grad_clip_set")
        p16_flags = [x if h else None for x, h in zip(gd, with16)]
        check(lib.rn_grad_norm_clip(ptrs(gd), ptrs(p16_flags), (C.c_int64 * n_t)(*sizes), n_t, 1, dt16, scale.data_ptr(), scratch.data_ptr(), slots,
                                    blk.data_ptr(), st), "rn_grad_norm_clip")
        torch.cuda.synchronize()
        f32 = blk.view(torch.float32)
        total, coef = float(f32[1]), float(f32[2])
        ref = float(torch.linalg.vector_norm(torch.cat([x.double() for x in gs])))
        assert abs(total - ref) <= 1e-6 * ref, (total, ref)
        assert coef == GradClip.coef(total, 0.5) and coef < 1.0, (coef, total)
        assert blk.view(torch.int64)[2:5].tolist() == [1, 1, 0]
        coef_ptr = blk.data_ptr() + 8
        clipped = [x.float() * f32[2] for x in gs]
        # SGD
        masters = [at_end(w) for w in w32]
        p16 = [at_end(w.to(dt), 8) if h else None for w, h in zip(w32, with16)]
        moms = [at_end(torch.zeros(n, device=DEV)) for n in sizes]
        gd16 = [at_end(x * 8.0) for x in gs]                                           # (the SGD step wants 16-byte aligned gradients)
        check(lib.rn_sgd_master_step(ptrs(masters), ptrs(moms), ptrs(gd16), ptrs(p16), (C.c_int64 * n_t)(*sizes), n_t, 1, dt16, 0.05, 0.9, 0.0,
                                     1e-2, 0, 1, scale.data_ptr(), found.data_ptr(), coef_ptr, st), "rn_sgd_master_step")
        ref_p = [torch.nn.Parameter(w.clone()) for w in w32]
        ropt = torch.optim.SGD(ref_p, lr=0.05, momentum=0.9, weight_decay=1e-2, foreach=False)
        for prm, x in zip(ref_p, clipped):
            prm.grad = x
        ropt.step()
        torch.cuda.synchronize()
        for mst, c16, prm in zip(masters, p16, ref_p):
            torch.testing.assert_close(mst, prm.detach().reshape(-1), rtol=2e-5, atol=1e-6)
            if c16 is not None:
                assert torch.equal(c16, mst.to(dt)), "16-bit copy != round(master)"
        # AdamW
        masters = [at_end(w) for w in w32]
        p16 = [at_end(w.to(dt), 8) if h else None for w, h in zip(w32, with16)]
        ms = [at_end(torch.zeros(n, device=DEV)) for n in sizes]
        vs = [at_end(torch.zeros(n, device=DEV)) for n in sizes]
        hp = at_end(torch.zeros(16, dtype=torch.float64, device=DEV), 8)
        check(lib.rn_adam_hparams_set(hp.data_ptr(), 1e-2, 0.9, 0.999, 1e-8, 0.1, -1.0, st), "rn_adam_hparams_set")
        check(lib.rn_adam_master_step(ptrs(masters), ptrs(ms), ptrs(vs), ptrs(gd), ptrs(p16), (C.c_int64 * n_t)(*sizes), n_t, 1, dt16, 1,
                                      hp.data_ptr(), scale.data_ptr(), found.data_ptr(), coef_ptr, st), "rn_adam_master_step")
        ref_p = [torch.nn.Parameter(w.clone()) for w in w32]
        ropt = torch.optim.AdamW(ref_p, lr=1e-2, weight_decay=0.1, foreach=False)
        for prm, x in zip(ref_p, clipped):
            prm.grad = x
        ropt.step()
        torch.cuda.synchronize()
        worst = 0.0
        for mst, c16, prm in zip(masters, p16, ref_p):
            worst = max(worst, float(((mst - prm.detach()).abs() / (prm.detach().abs() + 1e-4)).max()))
            if c16 is not None:
                assert torch.equal(c16, mst.to(dt)), "16-bit copy != round(master)"
        assert worst < 1e-4, worst
        assert float(hp[5]) == 1.0, float(hp[5])
        print("ok clip", str(dt), n_t, slots, f"norm {total:.6f} coef {coef:.6f} adam {worst:.2e}", flush=True)
    elif which == "accum":
        # rn_grad_accumulate (csrc/accum.hip): 170 tensors (two launches of 160 + 10), every gradient and every accumulator ENDING at
        # the last byte its alignment contract allows in its own mapping (16-bit gradients 8-byte aligned: the head path; sizes
        # through the tail paths; one tensor of three chunks), the block at the end of its own.  A window of three micro-batches
        # (overwrite, then two adds) against the torch restatement, bit for bit.
        from pytorch_retinanet_amd._lib import RN_F16
        sizes = [1, 3, 4, 5, 7, 8, 9, 1023, 4097, 16384, 16385, 2 * 16384 + 11] + [(i * 37) % 301 + 1 for i in range(158)]
        dt = torch.bfloat16 if len(sys.argv) < 3 or sys.argv[2] == "bf16" else torch.float16
        dt16 = RN_F16 if dt == torch.float16 else RN_BF16
        g = torch.Generator(device=DEV).manual_seed(13)

        def at_end(src: torch.Tensor, align: int = 16) -> torch.Tensor:
            nbytes = src.numel() * src.element_size()
            tot = (nbytes + GRAN - 1) // GRAN * GRAN
            base = torch.empty((tot,), dtype=torch.uint8, device=DEV)
            base.fill_(0x7f)
            _KEEP.append(base)
            off = (tot - nbytes) // align * align
            t = base[off: off + nbytes].view(src.dtype)
            t.copy_(src.reshape(-1))
            return t
        n_t = len(sizes)
        with16 = [i % 3 != 0 for i in range(n_t)]
        accs = [at_end(torch.full((n,), float("nan"), device=DEV)) for n in sizes]
        blk = at_end(torch.zeros(8, dtype=torch.float64, device=DEV), 8)
        ptrs = lambda ts: (C.c_void_p * n_t)(*[t.data_ptr() if t is not None else 0 for t in ts])
        N = 3
        check(lib.rn_grad_accum_set(blk.data_ptr(), N, st), "rn_grad_accum_set")
        w = torch.tensor(1.0 / N, dtype=torch.float32, device=DEV)
        want = [torch.zeros(n, device=DEV) for n in sizes]
        for k in range(N):
            gs = [(torch.randn(n, device=DEV, generator=g) * 0.1) for n in sizes]
            gs = [x.to(dt) if h else x for x, h in zip(gs, with16)]
            gd = [at_end(x, 8 if h else 16) for x, h in zip(gs, with16)]
            flags = [x if h else None for x, h in zip(gd, with16)]
            check(lib.rn_grad_accumulate(ptrs(accs), ptrs(gd), ptrs(flags), (C.c_int64 * n_t)(*sizes), n_t, 1, dt16, blk.data_ptr(), st),
                  "rn_grad_accumulate")
            check(lib.rn_grad_accum_advance(blk.data_ptr(), int(k == N - 1), st), "rn_grad_accum_advance")
            want = [a + x.float() * w for a, x in zip(want, gs)]
        torch.cuda.synchronize()
        for a, r in zip(accs, want):
            assert torch.equal(a, r), "accumulator != restatement"
        assert blk.view(torch.int32)[1:3].tolist() == [N, 0] and float(blk.view(torch.float32)[3]) == 0.0
        assert blk.view(torch.int64)[2:5].tolist() == [1, 0, N]
        print("ok accum", str(dt), n_t, sum(sizes), flush=True)
    elif which == "softnms":
        # Soft-NMS at the op boundary (rn_soft_nms_segments, csrc/softnms.hip): boxes, scores, segment offsets, the three outputs and the
        # workspace at the end of their own mappings; a 65-entry segment (the first length of the block kernel's register form) and a
        # 2049-entry one (the first of its HBM form), both methods, against the numpy restatement
        import numpy as np
        import soft_nms_cases as cases
        from pytorch_retinanet_amd._lib import RnNmsParams
        boxes, scores, off = cases.segments(92, (65, 2049))
        N, S = len(scores), len(off) - 1

        def at_end(a):
            src = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
            t = raw_at_end(src.numel() * src.element_size()).view(src.dtype).view(src.shape)
            t.copy_(src)
            return t
        db, ds, do = at_end(boxes), at_end(scores), at_end(off)
        need = lib.rn_nms_workspace_bytes(N, S)
        for code, method in ((1, "soft_linear"), (2, "soft_gaussian")):
            keep, ks, cnt, ws = raw_at_end(N * 8, 0), raw_at_end(N * 4, 0), raw_at_end(S * 4, 0), raw_at_end(need)
            params = RnNmsParams(code, 0.5, 1e-3, cases.CAP)
            check(lib.rn_soft_nms_segments(db.data_ptr(), ds.data_ptr(), do.data_ptr(), S, N, cases.IOU_THR, C.byref(params), keep.data_ptr(),
                                           ks.data_ptr(), cnt.data_ptr(), ws.data_ptr(), need, st), "rn_soft_nms_segments")
            torch.cuda.synchronize()
            wk, wsc, wc, _ = cases.expected(boxes, scores, off, method, cases.CAP)
            got_c = cnt.view(torch.int32).cpu().numpy()
            assert np.array_equal(got_c, wc), (method, got_c, wc)
            got_k, got_s = keep.view(torch.int64).cpu().numpy(), ks.view(torch.float32).cpu().numpy()
            for i in range(S):
                lo, hi = int(off[i]), int(off[i]) + int(wc[i])
                assert np.array_equal(got_k[lo:hi], wk[lo:hi]), (method, i)
                if code == 1:
                    assert np.array_equal(got_s[lo:hi].view(np.uint32), wsc[lo:hi].view(np.uint32)), (method, i)
                else:
                    np.testing.assert_allclose(got_s[lo:hi], wsc[lo:hi], rtol=cases.gaussian_bound(wc[i]), atol=0)
        print("ok softnms", N, S, flush=True)
    else:
        raise SystemExit(f"unknown probe {which!r}")


if __name__ == "__main__":
    main()
