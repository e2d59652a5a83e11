"""Forward time of the frozen mask branch of StandardROIHeads (afigan_amd/roi_heads.py) at the Mask R-CNN R50-FPN inference settings: 2 images,
100 detections each, C = 256, the pyramid of an 800 x 1344 input, K = 80, S = 14, four 3x3 convs, paste at 800 x 1333.  The mask ROIAlign, the
four convs, the deconv, afi_roi_mask_probs, afi_mask_paste and the whole branch are timed each alone, next to a torch-eager restatement of the
same stage on the same GPU with the same weights: median (min / max) of 9 CUDA-event-timed calls after warm-up.  Prints one line per part, the
achieved bytes/s of the two new kernels against their algorithmic traffic, and a JSON summary line.

    python tools/mask_bench.py --rounds 9

Baselines (torch alone): ROIAlign tools/roi_bench.py's gather form (fixed 2 x 2 grid); the convs F.conv2d + relu (MIOpen); the deconv
F.conv_transpose2d + relu; the predictor F.conv2d to all K channels, a gather of the row's class, sigmoid; the paste F.grid_sample over the
whole image + ``>=``, 25 detections at a time (the full batch's sampling grid alone is 1.7 GB)."""
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

from roi_bench import LEVELS, make_boxes, torch_roi_align  # noqa: E402
from rpn_bench import _time  # noqa: E402


def build(channels=256, K=80, D=100):
    import afigan_amd as amd
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": True, "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": LEVELS, "NUM_CLASSES": K},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "POOLER_RESOLUTION": 7},
                               "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": 4, "POOLER_RESOLUTION": 14}})
    cfg.TEST.DETECTIONS_PER_IMAGE = D
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=4 * 2 ** i) for i, f in enumerate(LEVELS)}, masks=True)
    g = torch.Generator().manual_seed(0)
    for name, p in h.named_parameters():
        if name.endswith("weight"):
            fan_in = p.shape[0] if "deconv" in name else p[0].numel()
            p.copy_(torch.randn(p.shape, generator=g) * 1.4 / math.sqrt(fan_in))
        else:
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return h.cuda().eval()


def torch_paste(probs, boxes, H, W, chunk=25):
    out = []
    ys = torch.arange(H, device=probs.device, dtype=torch.float32) + 0.5
    xs = torch.arange(W, device=probs.device, dtype=torch.float32) + 0.5
    for i in range(0, len(probs), chunk):
        b = boxes[i:i + chunk]
        gy = (ys[None] - b[:, 1:2]) / (b[:, 3:4] - b[:, 1:2]) * 2 - 1
        gx = (xs[None] - b[:, 0:1]) / (b[:, 2:3] - b[:, 0:1]) * 2 - 1
        grid = torch.stack([gx[:, None, :].expand(-1, H, -1), gy[:, :, None].expand(-1, -1, W)], -1)
        out.append(F.grid_sample(probs[i:i + chunk, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0] >= 0.5)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    N, D, H, W, C, K, S, PH, PW = 2, 100, 800, 1344, 256, 80, 14, 800, 1333
    with torch.no_grad():
        h = build(C, K, D)
        g = torch.Generator().manual_seed(1)
        xs = [torch.randn((N, C, -(-H // (4 * 2 ** i)), -(-W // (4 * 2 ** i))), generator=g).cuda() for i in range(4)]
        feats = {f: x.contiguous(memory_format=torch.channels_last) for f, x in zip(LEVELS, xs)}
        boxes = make_boxes(N, D, PH, PW)
        counts = torch.full((N,), D, dtype=torch.int32, device="cuda")
        classes = torch.randint(0, K, (N, D), generator=g).to(torch.int32).cuda()
        from afigan_amd import ops
        from afigan_amd.frozen import conv3x3
        mh = h.mask_head
        convs, (wd, bd), (wp, bp) = h._prepare_mask()
        pooled = h.mask_features(feats, boxes, counts)
        probs, acts, dec = h.mask_head_forward(pooled, classes, counts, intermediates=True)
        flat_boxes, flat_probs = boxes.reshape(-1, 4), probs.reshape(N * D, 2 * S, 2 * S)
        pooled_t = pooled.contiguous()                              # the torch baselines' own layout (NCHW)
        act_t = acts[-1].contiguous()
        idx = classes.reshape(-1).long()

        def hip_convs():
            x = pooled
            for wb in convs:
                x = conv3x3(x, wb, relu=True)
            return x

        def torch_convs():
            x = pooled_t
            for l in mh.conv_norm_relus:
                x = F.relu(F.conv2d(x, l.weight, l.bias, padding=1))
            return x

        def torch_deconv():
            return F.relu(F.conv_transpose2d(act_t, mh.deconv.weight, mh.deconv.bias, stride=2))
        up_t = torch_deconv()

        def torch_probs():
            return torch.sigmoid(F.conv2d(up_t, mh.predictor.weight, mh.predictor.bias)[torch.arange(N * D, device="cuda"), idx])

        def torch_branch():
            p = torch_roi_align(xs, boxes, S=S)
            for l in mh.conv_norm_relus:
                p = F.relu(F.conv2d(p, l.weight, l.bias, padding=1))
            p = F.relu(F.conv_transpose2d(p, mh.deconv.weight, mh.deconv.bias, stride=2))
            p = torch.sigmoid(F.conv2d(p, mh.predictor.weight, mh.predictor.bias)[torch.arange(N * D, device="cuda"), idx])
            return torch_paste(p, flat_boxes, PH, PW)

        def hip_branch():
            p = h._mask_branch(list(feats.values()), boxes, classes, counts)
            return ops.mask_paste(p.reshape(N * D, 2 * S, 2 * S), flat_boxes, (PH, PW))
        parts = {"mask ROIAlign HIP": lambda: h.mask_features(feats, boxes, counts), "mask ROIAlign torch": lambda: torch_roi_align(xs, boxes, S=S),
                 "4 convs HIP": hip_convs, "4 convs torch": torch_convs,
                 "deconv HIP": lambda: ops.conv1x1_fwd(acts[-1], wd, bd, act=2), "deconv torch": torch_deconv,
                 "mask_probs HIP": lambda: ops.roi_mask_probs(dec, wp, bp, classes, counts), "mask_probs torch": torch_probs,
                 "paste HIP": lambda: ops.mask_paste(flat_probs, flat_boxes, (PH, PW)), "paste torch": lambda: torch_paste(flat_probs, flat_boxes, PH, PW),
                 "branch HIP": hip_branch, "branch torch": torch_branch}
        r = {}
        for name, fn in parts.items():
            ts = _time(fn, args.rounds)
            r[name] = statistics.median(ts)
            print(f"{name:22s}: median {r[name]:8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  ({len(ts)} rounds)", flush=True)
        R = N * D
        pb, sb = R * 4 * S * S * C * 4, R * PH * PW
        r["mask_probs_algorithmic_MB"], r["mask_probs_GBps"] = pb / 1e6, pb / 1e9 / (r["mask_probs HIP"] * 1e-3)
        r["paste_algorithmic_MB"], r["paste_GBps"] = sb / 1e6, sb / 1e9 / (r["paste HIP"] * 1e-3)
        print(f"afi_roi_mask_probs: {pb / 1e6:.1f} MB read, {r['mask_probs_GBps']:.0f} GB/s;  afi_mask_paste: {sb / 1e6:.1f} MB written, "
              f"{r['paste_GBps']:.0f} GB/s", flush=True)
        same = (ops.mask_paste(flat_probs, flat_boxes, (PH, PW)) == torch_paste(flat_probs, flat_boxes, PH, PW)).float().mean().item()
        print(f"paste HIP == paste torch (fp32 grid_sample) on {100 * same:.4f} % of the pixels", flush=True)
        r["deconv_plus_probs_share_of_branch"] = (r["deconv HIP"] + r["mask_probs HIP"]) / r["branch HIP"]
    print(json.dumps({"rounds": args.rounds, "median_ms": r, "baseline": "torch gathers; F.conv2d; F.conv_transpose2d; F.grid_sample + >="}))


if __name__ == "__main__":
    main()
