"""Forward time of the frozen CascadeROIHeads (afigan_amd/roi_heads.py) at the Cascade inference configs' settings: 2 images, 1000 proposals
each, C = 256, the pyramid of an 800 x 1344 input (200 x 336 ... 25 x 42), K = 80, S = 7, three stages of four SyncBN 3x3 convs and one FC of
1024 (no mask branch: tools/mask_bench.py times that).  Per stage ROIAlign, the four convs, fc1, the predictor and afi_roi_cascade_stage are
timed each alone on that stage's own inputs, then the selection and forward_padded, each next to a torch-eager restatement of the same part on
the same GPU with the same weights: median (min / max) of CUDA-event-timed calls after warm-up.  Prints one line per part and a JSON summary.

    python tools/cascade_bench.py --rounds 9 [--trace-only]

By count the convs dominate: 98 000 pixels x 256 x 256 x 9 x 2 = 116 GFLOP per conv, 1.39 TFLOP for the twelve, against 3 x 51 GFLOP for fc1.
Baselines (torch alone): tools/roi_bench.py's gather ROIAlign (fixed 2 x 2 grid); F.conv2d + F.batch_norm (eval) + relu on channels-last
tensors -- MIOpen; F.linear -- hipBLASLt; softmax, the decode as elementwise ops, add and scale; topk + class-offset NMS as roi_bench.py.
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

from roi_bench import CLAMP, LEVELS, make_boxes, torch_roi_align  # noqa: E402
from rpn_bench import _time, torch_nms  # noqa: E402


def build(channels=256, K=80, stages=3):
    import afigan_amd as amd
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ROI_HEADS": {"NAME": "CascadeROIHeads", "IN_FEATURES": LEVELS, "NUM_CLASSES": K},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 1, "NUM_CONV": 4, "NORM": "SyncBN", "POOLER_RESOLUTION": 7,
                                                "CLS_AGNOSTIC_BBOX_REG": True}})
    assert len(cfg.MODEL.ROI_BOX_CASCADE_HEAD.IOUS) == stages
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=4 * 2 ** i) for i, f in enumerate(LEVELS)}, cascade=True)
    g = torch.Generator().manual_seed(0)
    for name, p in list(h.named_parameters()) + list(h.named_buffers()):
        leaf = name.split(".")[-1]
        if leaf == "num_batches_tracked":
            continue
        if ".norm." in name:
            p.copy_(0.5 + torch.rand(p.shape, generator=g) if leaf in ("weight", "running_var") else torch.randn(p.shape, generator=g) * 0.1)
        elif leaf == "weight":
            p.copy_(torch.randn(p.shape, generator=g) * (3.0 if "cls_score" in name else 1.4) / math.sqrt(p[0].numel()))
        else:
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return h.cuda().eval()


def torch_convs(head, x):
    for c in head.conv_norm_relus:
        n = c.norm
        x = F.relu(F.batch_norm(F.conv2d(x, c.weight, None, padding=1), n.running_mean, n.running_var, n.weight, n.bias, False, 0.0, n.eps))
    return x


def torch_stage(pred, K, boxes, hw, weights, prev, scale):
    """softmax, the class-agnostic decode and clip, the running score: eager torch on [N, P, .] tensors."""
    N, P = boxes.shape[:2]
    q = pred.view(N, P, -1)
    s = F.softmax(q[..., :K + 1], -1)[..., :K]
    d = q[..., K + 1:K + 5]
    wx, wy, ww, wh = weights
    w, hh = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
    cx, cy = boxes[..., 0] + 0.5 * w, boxes[..., 1] + 0.5 * hh
    pcx, pcy = d[..., 0] / wx * w + cx, d[..., 1] / wy * hh + cy
    pw, ph = torch.exp((d[..., 2] / ww).clamp(max=CLAMP)) * w, torch.exp((d[..., 3] / wh).clamp(max=CLAMP)) * hh
    bx = torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], -1)
    bx[..., 0::2] = torch.minimum(bx[..., 0::2].clamp(min=0), hw[:, None, 1:2])
    bx[..., 1::2] = torch.minimum(bx[..., 1::2].clamp(min=0), hw[:, None, 0:1])
    s = s if prev is None else prev + s
    return (s * scale if scale != 1.0 else s), bx


def torch_pick(h, scores, boxes, M=1024):
    res = []
    K = scores.shape[2]
    for n in range(scores.shape[0]):
        v, i = torch.topk(scores[n].reshape(-1), min(M, scores[n].numel()), sorted=True)
        ok = v > h.test_score_thresh
        v, i = v[ok], i[ok]
        cb, cls = boxes[n][i // K], i % K
        kp = torch_nms(cb + (cls.float() * (cb.max() + 1))[:, None], h.test_nms_thresh)         # torchvision's batched_nms offset
        res.append((cb[kp][:h.test_detections_per_img], v[kp][:h.test_detections_per_img], cls[kp][:h.test_detections_per_img]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    N, P, H, W, C, K = 2, 1000, 800, 1344, 256, 80
    with torch.no_grad():
        h = build(C, K)
        g = torch.Generator().manual_seed(1)
        xs = [torch.randn((N, C, -(-H // (4 * 2 ** i)), -(-W // (4 * 2 ** i))), generator=g).cuda() for i in range(4)]
        feats = {f: x.contiguous(memory_format=torch.channels_last) for f, x in zip(LEVELS, xs)}
        boxes = make_boxes(N, P, H, W)
        counts = torch.full((N,), P, dtype=torch.int32, device="cuda")
        hw = torch.tensor([[H, W]] * N, dtype=torch.float32, device="cuda")
        if args.trace_only:
            _time(lambda: h.forward_padded(hw, feats, boxes, counts), 3, warmup=1)
            print("[trace] Cascade ROI heads 2x1000, 3 stages: 1 warm-up + 3 forward_padded", flush=True)
            return
        from afigan_amd import ops
        from afigan_amd.frozen import conv3x3
        from afigan_amd.roi_heads import _rows_as_pixels
        S = h.num_stages
        inter = h.forward_padded(hw, feats, boxes, counts, intermediates=True)
        r = {}

        def timed(name, fn):
            ts = _time(fn, args.rounds)
            r[name] = statistics.median(ts)
            print(f"{name:30s}: median {r[name]:8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  ({len(ts)} rounds)", flush=True)

        for k, st in enumerate(inter["stages"]):
            head, pr = h.box_head[k], h.box_predictor[k]
            convs, (w1, wp, bp) = h._prepare(k)
            fc1 = head.fcs[0]
            props, pooled, last = st["proposals"], st["pooled"], st["convs"][-1]
            prev = inter["stages"][k - 1]["scores"] if k else None
            scale = 1.0 / S if k == S - 1 else 1.0
            x0 = _rows_as_pixels(last.permute(0, 2, 3, 1).reshape(N * P, -1))
            a1 = _rows_as_pixels(st["fc"][0])
            flat = last.flatten(1).contiguous()                    # the torch baseline's own layout ([C][S][S] order)

            def hip_convs(x=pooled, convs=convs):
                for wb in convs:
                    x = conv3x3(x, wb, relu=True)
                return x
            timed(f"stage {k} ROIAlign HIP", lambda: h.box_pooler(list(feats.values()), props, counts))
            timed(f"stage {k} ROIAlign torch", lambda: torch_roi_align(xs, props))
            timed(f"stage {k} 4 convs HIP", hip_convs)
            timed(f"stage {k} 4 convs torch", lambda: torch_convs(head, pooled))
            timed(f"stage {k} fc1 HIP", lambda: ops.conv1x1_fwd(x0, w1, fc1.bias, act=2))
            timed(f"stage {k} fc1 torch", lambda: F.relu(F.linear(flat, fc1.weight, fc1.bias)))
            timed(f"stage {k} predictor HIP", lambda: ops.conv1x1_fwd(a1, wp, bp))
            timed(f"stage {k} predictor torch", lambda: torch.cat([F.linear(st["fc"][0], pr.cls_score.weight, pr.cls_score.bias),
                                                                    F.linear(st["fc"][0], pr.bbox_pred.weight, pr.bbox_pred.bias)], 1))
            timed(f"stage {k} cascade_stage HIP", lambda: ops.roi_cascade_stage(st["pred"], K, props, counts, hw, h.stage_weights[k], prev_scores=prev,
                                                                                out_scale=scale))
            timed(f"stage {k} cascade_stage torch", lambda: torch_stage(st["pred"], K, props, hw, h.stage_weights[k], prev, scale))
        sc, bx = inter["class_scores"], inter["class_boxes"]
        timed("selection HIP", lambda: h._pick(sc, bx))
        timed("selection torch", lambda: torch_pick(h, sc, bx.view(N, P, 4)))
        timed("forward_padded HIP", lambda: h.forward_padded(hw, feats, boxes, counts))
        flop = 2.0 * N * P * 49 * 9 * C * C
        per_conv = statistics.median([r[f"stage {k} 4 convs HIP"] for k in range(S)]) / 4
        r["conv_GFLOP"] = flop / 1e9
        r["conv_TFLOPs"] = flop / 1e12 / (per_conv * 1e-3)
        print(f"convs: {flop / 1e9:.0f} GFLOP each, {per_conv:.3f} ms each (median stage / 4), {r['conv_TFLOPs']:.1f} TFLOP/s algorithmic", flush=True)
        print(f"detections per image: HIP {inter['counts'].tolist()}, torch {[len(v) for _, v, _ in torch_pick(h, sc, bx.view(N, P, 4))]}", flush=True)
    print(json.dumps({"rounds": args.rounds, "median_ms": r,
                      "baseline": "torch gathers; F.conv2d + F.batch_norm + relu; F.linear; softmax + elementwise decode; topk + IoU matrix with 64-row sweep"}))


if __name__ == "__main__":
    main()
