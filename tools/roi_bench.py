"""Forward time of the frozen box branch of StandardROIHeads (afigan_amd/roi_heads.py) at the R50-FPN inference settings: 2 images, 1000
proposals each, C = 256, the pyramid of an 800 x 1344 input (200 x 336 ... 25 x 42), K = 80, S = 7, two FCs of 1024.  ROIAlign, fc1,
fc2 + predictor, the selection stages and forward_padded are timed each alone, next to a torch-eager restatement of the same stage on the same
GPU with the same weights: median (min / max) of CUDA-event-timed calls after warm-up.  Prints one line per part and a JSON summary line.

    python tools/roi_bench.py --rounds 9 [--trace-only]

Baselines (torch alone: there is no torchvision here):
  ROIAlign    per level one gather of the four corners of every sample of every box assigned to it (fixed 2 x 2 grid: the adaptive grid needs
              a ragged loop in eager torch, and 2 x 2 is what these proposals mostly get) and a weighted sum;
  fc1 / fc2 + predictor   F.linear + relu -- hipBLASLt;
  selection   softmax, the decode as elementwise ops, torch.topk over the image's scores, the class-offset batched NMS with the 64-row sweep
              of tools/rpn_bench.py, the first 100.
--trace-only: one warm-up and three timed forward_padded calls, nothing else (for a rocprofv3 kernel trace)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rpn_bench import _time, torch_nms  # noqa: E402

LEVELS = ["p2", "p3", "p4", "p5"]
CLAMP = math.log(1000.0 / 16)


def build(channels=256, K=80):
    import afigan_amd as amd
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": LEVELS, "NUM_CLASSES": K},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "POOLER_RESOLUTION": 7}})
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=4 * 2 ** i) for i, f in enumerate(LEVELS)})
    g = torch.Generator().manual_seed(0)
    for name, p in h.named_parameters():
        if name.endswith("weight"):
            p.copy_(torch.randn(p.shape, generator=g) * (3.0 if "cls_score" in name else 1.0) / math.sqrt(p.shape[1]))
        else:
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return h.cuda().eval()


def make_boxes(N, P, H, W, seed=2):
    g = torch.Generator().manual_seed(seed)
    side = torch.exp(torch.empty((N, P, 2)).uniform_(math.log(16), math.log(600), generator=g))
    ctr = torch.rand((N, P, 2), generator=g) * torch.tensor([W, H], dtype=torch.float32)
    b = torch.cat([ctr - side / 2, ctr + side / 2], -1)
    b[..., 0::2] = b[..., 0::2].clamp(0, W)
    b[..., 1::2] = b[..., 1::2].clamp(0, H)
    return b.cuda()


def torch_roi_align(xs, boxes, S=7, grid=2, min_level=2):
    """[N P, C, S, S] with torch gathers, a fixed grid x grid sampling (NCHW levels)."""
    N, P = boxes.shape[:2]
    C = xs[0].shape[1]
    b = boxes.reshape(-1, 4)
    img = torch.arange(N, device=b.device).repeat_interleave(P)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lvl = torch.floor(4 + torch.log2(torch.sqrt(area.clamp(min=1e-12)) / 224)).clamp(min_level, min_level + len(xs) - 1).long()
    out = torch.zeros((N * P, C, S, S), device=b.device)
    t = (torch.arange(S * grid, device=b.device).float() + 0.5) / grid         # sample positions in bin units
    for l, x in enumerate(xs):
        sel = torch.nonzero(lvl == min_level + l).flatten()
        if not len(sel):
            continue
        Hl, Wl = x.shape[2:]
        sc = 1.0 / 2 ** (min_level + l)
        bb = b[sel] * sc
        ys = bb[:, 1, None] - 0.5 + t[None] * ((bb[:, 3] - bb[:, 1]) / S)[:, None]
        xw = bb[:, 0, None] - 0.5 + t[None] * ((bb[:, 2] - bb[:, 0]) / S)[:, None]

        def axis(v, size):
            ok = (v >= -1) & (v <= size)
            v = v.clamp(min=0)
            lo = v.floor().clamp(max=size - 1)
            hi = (lo + 1).clamp(max=size - 1)
            v = torch.where(lo >= size - 1, lo, v)
            frac = v - lo
            return lo.long(), hi.long(), (1 - frac) * ok, frac * ok
        yl, yh, wyl, wyh = axis(ys, Hl)
        xl, xh, wxl, wxh = axis(xw, Wl)
        f = x[img[sel]]                                                        # [r, C, H, W]
        r = len(sel)
        ar = torch.arange(r, device=b.device)[:, None, None]

        def tap(yi, xi, wy, wx):
            return f[ar, :, yi[:, :, None], xi[:, None, :]] * (wy[:, :, None] * wx[:, None, :])[..., None]
        v = tap(yl, xl, wyl, wxl) + tap(yl, xh, wyl, wxh) + tap(yh, xl, wyh, wxl) + tap(yh, xh, wyh, wxh)       # [r, S g, S g, C]
        out[sel] = v.reshape(r, S, grid, S, grid, C).mean((2, 4)).permute(0, 3, 1, 2)
    return out


def torch_select(h, pred, boxes, counts, hw, M=1024):
    N, P = boxes.shape[:2]
    K = h.num_classes
    res = []
    wx, wy, ww, wh = h.box_weights
    for n in range(N):
        c = int(counts[n])
        q, pb = pred[n * P:n * P + c], boxes[n, :c]
        sc = F.softmax(q[:, :K + 1], 1)[:, :K]
        d = q[:, K + 1:K + 1 + 4 * K].reshape(c, K, 4)
        w, hh = (pb[:, 2] - pb[:, 0])[:, None], (pb[:, 3] - pb[:, 1])[:, None]
        cx, cy = pb[:, 0, None] + 0.5 * w, pb[:, 1, None] + 0.5 * hh
        pcx, pcy = d[..., 0] / wx * w + cx, d[..., 1] / wy * hh + cy
        pw, ph = torch.exp((d[..., 2] / ww).clamp(max=CLAMP)) * w, torch.exp((d[..., 3] / wh).clamp(max=CLAMP)) * hh
        bx = torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], -1)
        bx[..., 0::2] = torch.minimum(bx[..., 0::2].clamp(min=0), hw[n, 1])
        bx[..., 1::2] = torch.minimum(bx[..., 1::2].clamp(min=0), hw[n, 0])
        v, i = torch.topk(sc.reshape(-1), min(M, sc.numel()), sorted=True)
        ok = v > h.test_score_thresh
        v, i = v[ok], i[ok]
        cb, cls = bx.reshape(-1, 4)[i], i % K
        kp = torch_nms(cb + (cls.float() * (cb.max() + 1))[:, None], h.test_nms_thresh)         # torchvision's batched_nms offset
        res.append((cb[kp][:h.test_detections_per_img], v[kp][:h.test_detections_per_img], cls[kp][:h.test_detections_per_img]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    N, P, H, W, C = 2, 1000, 800, 1344, 256
    with torch.no_grad():
        h = build(C)
        g = torch.Generator().manual_seed(1)
        xs = [torch.randn((N, C, -(-H // (4 * 2 ** i)), -(-W // (4 * 2 ** i))), generator=g).cuda() for i in range(4)]
        feats = {f: x.contiguous(memory_format=torch.channels_last) for f, x in zip(LEVELS, xs)}
        boxes = make_boxes(N, P, H, W)
        counts = torch.full((N,), P, dtype=torch.int32, device="cuda")
        hw = torch.tensor([[H, W]] * N, dtype=torch.float32, device="cuda")
        if args.trace_only:
            _time(lambda: h.forward_padded(hw, feats, boxes, counts), 3, warmup=1)
            print("[trace] ROI heads 2x1000: 1 warm-up + 3 forward_padded", flush=True)
            return
        from afigan_amd import ops
        from afigan_amd.roi_heads import _pixels_as_rows, _rows_as_pixels
        pooled = h.box_features(feats, boxes, counts)
        w1, wp, bp = h._prepare()
        fc1, fc2 = h.box_head.fcs
        x0 = _rows_as_pixels(pooled.permute(0, 2, 3, 1).reshape(N * P, -1))
        a1 = ops.conv1x1_fwd(x0, w1, fc1.bias, act=2)
        pred = h.box_head_forward(pooled)
        flat = pooled.flatten(1).contiguous()                  # the torch baseline's own layout ([C][S][S] order)
        t1 = F.relu(F.linear(flat, fc1.weight, fc1.bias))
        pr = h.box_predictor

        def torch_tail():
            t2 = F.relu(F.linear(t1, fc2.weight, fc2.bias))
            return torch.cat([F.linear(t2, pr.cls_score.weight, pr.cls_score.bias), F.linear(t2, pr.bbox_pred.weight, pr.bbox_pred.bias)], 1)
        tpred = torch_tail()
        parts = {"ROIAlign HIP": lambda: h.box_features(feats, boxes, counts), "ROIAlign torch": lambda: torch_roi_align(xs, boxes),
                 "fc1 HIP": lambda: ops.conv1x1_fwd(x0, w1, fc1.bias, act=2), "fc1 torch": lambda: F.relu(F.linear(flat, fc1.weight, fc1.bias)),
                 "fc2+predictor HIP": lambda: ops.conv1x1_fwd(ops.conv1x1_fwd(a1, fc2.weight, fc2.bias, act=2), wp, bp), "fc2+predictor torch": torch_tail,
                 "selection HIP": lambda: h.select(pred, boxes, counts, hw), "selection torch": lambda: torch_select(h, tpred, boxes, counts, hw),
                 "forward_padded HIP": lambda: h.forward_padded(hw, feats, boxes, counts)}
        r = {}
        for name, fn in parts.items():
            ts = _time(fn, args.rounds)
            r[name] = statistics.median(ts)
            print(f"{name:22s}: median {r[name]:8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  ({len(ts)} rounds)", flush=True)
        # ROIAlign's algorithmic traffic: R S^2 grid^2 4 gathers of C floats, plus the output
        from_tests = os.path.join(ROOT, "tests")
        sys.path.insert(0, from_tests)
        import roi_f64 as Q
        b64 = boxes.cpu().double().numpy().reshape(-1, 4)
        lv = Q.level_of(b64, 2, 5)
        samples = sum(gh * gw for gh, gw, _, _ in (Q.grid_of(b, l, 7, 0) for b, l in zip(b64, lv)) if gh > 0 and gw > 0)
        nbytes = (samples * 49 * 4 * C + N * P * 49 * C) * 4
        r["roialign_algorithmic_GB"] = nbytes / 1e9
        r["roialign_GBps"] = nbytes / 1e9 / (r["ROIAlign HIP"] * 1e-3)
        print(f"ROIAlign: {samples} samples per bin set, {nbytes / 1e6:.1f} MB algorithmic traffic, {r['roialign_GBps']:.0f} GB/s", flush=True)
        c = h.select(pred, boxes, counts, hw)["counts"].tolist()
        print(f"detections per image: HIP {c}, torch {[len(v) for _, v, _ in torch_select(h, tpred, boxes, counts, hw)]}", flush=True)
    print(json.dumps({"rounds": args.rounds, "median_ms": r, "baseline": "torch gathers; F.linear; softmax + topk + IoU matrix with 64-row sweep"}))


if __name__ == "__main__":
    main()
