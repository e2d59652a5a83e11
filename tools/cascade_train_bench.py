"""Time of CascadeROIHeads in training (afigan_amd/roi_heads.py: CascadeROIHeads.losses; csrc/cascade_train.hip) at the Cascade configs' size --
N = 2 at 800 x 1344, four levels of 256 channels, 1000 proposals and 20 boxes per image, BATCH_SIZE_PER_IMAGE 512, three stages with four
SyncBN convs and one FC of 1024 each, 80 classes, 7 x 7 bins -- next to a torch-eager restatement on the same GPU with the same weights:
median (min / max) of device-event-timed runs after 3 warm-ups.  The box branch only: the mask head (which trains, normed or not) has no column
here yet -- its torch restatement needs a 14 x 14 pooler and polygon targets this tool does not build.

    python tools/cascade_train_bench.py [--rounds 20] [--ratio 2]

Parts:
  losses fwd+bwd   CascadeROIHeads.losses and .backward() to the four feature maps and every parameter, against: label_and_sample_proposals as a
                   G x R IoU matrix (tools/roi_loss_bench.py), per stage a pure-torch gather ROIAlign, nn.functional conv2d / batch_norm
                   (training) / relu / linear on the compacted rows, apply_deltas + clip + nonempty filter + IoU matrix for the next stage,
                   autograd;
  relabel          afi_roi_cascade_relabel alone on stage 0's output;
  each list-masked BatchNorm pass alone on [2 x 512, 49, 256] with every row valid and with (512, 300) rows valid, as GB/s of the bytes the
  pass has to move (statistics 1, apply 2, backward sums 3, backward apply 4 tensors of the VALID rows) next to the 6.29 TB/s copy rate of
  DESIGN 26.  No figure is a pass criterion."""
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
import roi_loss_bench as RB  # noqa: E402

LEVELS, S = RB.LEVELS, RB.S
IOUS = (0.5, 0.6, 0.7)
WEIGHTS = ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))
COPY_RATE_GBS = 6290.0


def build(ratio, channels=256, batch=512):
    import afigan_amd as amd
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": False, "ROI_HEADS": {"NAME": "CascadeROIHeads", "IN_FEATURES": LEVELS, "BATCH_SIZE_PER_IMAGE": batch},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 1, "NUM_CONV": 4, "CONV_DIM": channels, "NORM": "SyncBN",
                                                "POOLER_RESOLUTION": S, "POOLER_SAMPLING_RATIO": ratio, "CLS_AGNOSTIC_BBOX_REG": True},
                               "ROI_BOX_CASCADE_HEAD": {"IOUS": IOUS, "BBOX_REG_WEIGHTS": WEIGHTS}})
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=4 * 2 ** i) for i, f in enumerate(LEVELS)}, cascade=True)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for k, p in h.named_parameters():
            fan = p[0].numel() if p.dim() > 1 else 1
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if k.endswith("bias") else (0.1 if "bbox_pred" in k else 1.0) / math.sqrt(fan)))
    return h.cuda().trainable_().train()


def torch_stage(h, k, pooled):
    x = pooled
    for conv in h.box_head[k].conv_norm_relus:
        x = F.relu(F.batch_norm(F.conv2d(x, conv.weight, None, padding=1), None, None, conv.norm.weight, conv.norm.bias, training=True, eps=conv.norm.eps))
    x = x.flatten(1)
    for fc in h.box_head[k].fcs:
        x = F.relu(F.linear(x, fc.weight, fc.bias))
    pr = h.box_predictor[k]
    return F.linear(x, pr.cls_score.weight, pr.cls_score.bias), F.linear(x, pr.bbox_pred.weight, pr.bbox_pred.bias)


def torch_stage_losses(h, k, logits, deltas, boxes, cls, gboxes):
    n = cls.numel()
    loss_cls = F.cross_entropy(logits, cls, reduction="sum") / n
    fg = torch.nonzero(cls < h.num_classes).squeeze(1)
    a, b = boxes[fg], gboxes[fg]
    sw, sh, tw, th = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    wx, wy, ww, wh = h.stage_weights[k]
    tgt = torch.stack([wx * (b[:, 0] + 0.5 * tw - a[:, 0] - 0.5 * sw) / sw, wy * (b[:, 1] + 0.5 * th - a[:, 1] - 0.5 * sh) / sh,
                       ww * torch.log(tw / sw), wh * torch.log(th / sh)], 1)
    return loss_cls, (deltas[fg] - tgt).abs().sum() / n


def torch_relabel(h, k, deltas, boxes, img, gts, gcls, hw):
    """_create_proposals_from_boxes + _match_and_label_boxes per image: [(boxes, classes, matched boxes)]"""
    wx, wy, ww, wh = h.stage_weights[k]
    w, hg = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cx, cy = boxes[:, 0] + 0.5 * w, boxes[:, 1] + 0.5 * hg
    d = deltas.detach()
    pcx, pcy = d[:, 0] / wx * w + cx, d[:, 1] / wy * hg + cy
    pw, ph = torch.exp((d[:, 2] / ww).clamp(max=math.log(1000.0 / 16))) * w, torch.exp((d[:, 3] / wh).clamp(max=math.log(1000.0 / 16))) * hg
    nb = torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 1)
    out = []
    for n, (gt, gc) in enumerate(zip(gts, gcls)):
        b = nb[img == n]
        b = torch.stack([b[:, 0].clamp(0, hw[1]), b[:, 1].clamp(0, hw[0]), b[:, 2].clamp(0, hw[1]), b[:, 3].clamp(0, hw[0])], 1)
        b = b[((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)]
        area_g, area_c = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        whi = (torch.min(gt[:, None, 2:], b[:, 2:]) - torch.max(gt[:, None, :2], b[:, :2])).clamp(min=0)
        inter = whi[..., 0] * whi[..., 1]
        iou = torch.where(inter > 0, inter / (area_g[:, None] + area_c - inter), torch.zeros((), device=gt.device))
        vals, midx = iou.max(dim=0)
        cls = torch.where(vals >= IOUS[k + 1], gc[midx].long(), torch.full_like(midx, h.num_classes))
        out.append((b, cls, gt[midx]))
    return out


def torch_losses(h, xs, props, gts, gcls, ratio, hw):
    h.iou_threshold = IOUS[0]
    lists = [RB.torch_assign(h, p, g, c) for p, g, c in zip(props, gts, gcls)]
    total = 0
    for k in range(h.num_stages):
        boxes, cls, gb = (torch.cat([l[i] for l in lists]) for i in range(3))
        img = torch.cat([torch.full((l[0].shape[0],), n, device=boxes.device, dtype=torch.int64) for n, l in enumerate(lists)])
        pooled = RB.torch_roi_align(xs, boxes, img, h.box_pooler.min_level, ratio)
        pooled = pooled * (1.0 / h.num_stages) + (pooled * (1 - 1.0 / h.num_stages)).detach()             # _ScaleGradient
        lg, dl = torch_stage(h, k, pooled)
        lc, lb = torch_stage_losses(h, k, lg, dl, boxes, cls, gb)
        total = total + lc + lb
        if k + 1 < h.num_stages:
            with torch.no_grad():
                lists = torch_relabel(h, k, dl, boxes, img, gts, gcls, hw)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--boxes", type=int, default=20)
    ap.add_argument("--proposals", type=int, default=1000)
    ap.add_argument("--ratio", type=int, default=2)
    ap.add_argument("--shape", default="2x800x1344")
    args = ap.parse_args()
    from afigan_amd import ops
    N, H, W = (int(v) for v in args.shape.split("x"))
    P, G = args.proposals, args.boxes
    h = build(args.ratio)
    K, B = h.num_classes, h.batch_size_per_image
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn((N, 256, -(-H // (4 * 2 ** i)), -(-W // (4 * 2 ** i))), generator=g).cuda() for i in range(4)]
    feats = {f: x.contiguous(memory_format=torch.channels_last).requires_grad_(True) for f, x in zip(LEVELS, xs)}
    xs = [x.requires_grad_(True) for x in xs]

    def rand_boxes(n, lo, hi):
        c = torch.rand((n, 2), generator=g) * torch.tensor([W, H])
        wh = torch.exp(torch.rand((n, 2), generator=g) * math.log(hi / lo)) * lo
        return torch.cat([c - wh / 2, c + wh / 2], 1).clamp(min=0).minimum(torch.tensor([W, H, W, H]).float())
    gts, gcls, props = [], [], []
    for n in range(N):
        gt = rand_boxes(G, 24, 500)
        gt = gt[((gt[:, 2] - gt[:, 0]) > 4) & ((gt[:, 3] - gt[:, 1]) > 4)]
        near = gt[torch.randint(0, gt.shape[0], (P // 4,), generator=g)]
        near = near + (torch.rand(near.shape, generator=g) - 0.5) * 0.2 * (near[:, 2:] - near[:, :2]).repeat(1, 2)
        gts.append(gt.cuda())
        gcls.append(torch.randint(0, K, (gt.shape[0],), generator=g).to(torch.int32).cuda())
        props.append(torch.cat([near, rand_boxes(P - P // 4, 8, 600)]).cuda())
    prop_obj = [RB.Obj(proposal_boxes=p, image_size=(H, W)) for p in props]
    tgt_obj = [RB.Obj(gt_boxes=b, gt_classes=c) for b, c in zip(gts, gcls)]
    gt_pad, gc_pad, gcounts = h._targets(tgt_obj, N, "cuda")
    keys = torch.randint(-2 ** 31, 2 ** 31, (N, P + gt_pad.shape[1]), device="cuda", dtype=torch.int32)
    hw = torch.tensor([[H, W]] * N, dtype=torch.float32, device="cuda")

    out = h.losses(None, feats, prop_obj, tgt_obj, keys)
    st = h.last_assignment["stages"]
    print(f"{P} proposals + {G} boxes per image, B = {B}: rows per stage {[s['counts'].tolist() for s in st]}, foreground "
          f"{[[int((s['gt_classes'][n] >= 0).logical_and(s['gt_classes'][n] < K).sum()) for n in range(N)] for s in st]}")
    print("losses:", {k: round(v.item(), 5) for k, v in out.items()}, flush=True)
    s0 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st[0].items()}

    def hip_full():
        sum(h.losses(None, feats, prop_obj, tgt_obj, keys).values()).backward()

    def torch_full():
        torch_losses(h, xs, props, gts, gcls, args.ratio, (H, W)).backward()

    def hip_relabel():
        return ops.roi_cascade_relabel(s0["pred"], K, s0["boxes"], s0["counts"], hw, WEIGHTS[0], gt_pad, gc_pad, gcounts, IOUS[1])

    results = {}
    for name, fn in (("losses fwd+bwd HIP", hip_full), ("losses fwd+bwd torch", torch_full), ("relabel HIP", hip_relabel)):
        ts = RB._time(fn, args.rounds)
        results[name] = statistics.median(ts)
        print(f"{name:34s} median {results[name]:9.3f} ms  min {min(ts):9.3f}  max {max(ts):9.3f}  ({len(ts)} rounds)", flush=True)

    # the list-masked BatchNorm passes alone
    P1, C_ = S * S, 256
    x = torch.randn((N * B, P1, C_), device="cuda")
    gq = torch.randn_like(x)
    gamma, beta = torch.rand(C_, device="cuda") + 0.5, torch.randn(C_, device="cuda")
    for label, cn in (("all rows", [B] * N), ("(512, 300) rows", [B, 300][:N])):
        counts = torch.tensor(cn, dtype=torch.int32, device="cuda")
        valid_bytes = sum(cn) * P1 * C_ * 4
        mean, invstd = ops.roi_bn_stats(x, counts, 1e-5, 0.1)
        y = ops.roi_bn_relu_fwd(x, counts, mean, invstd, gamma, beta)
        sums = ops.roi_bn_relu_bwd_sums(gq, x, y, counts, mean, invstd)
        for name, tensors, fn in (("roi_bn_stats", 1, lambda: ops.roi_bn_stats(x, counts, 1e-5, 0.1)),
                                  ("roi_bn_relu_fwd", 2, lambda: ops.roi_bn_relu_fwd(x, counts, mean, invstd, gamma, beta)),
                                  ("roi_bn_relu_bwd_sums", 3, lambda: ops.roi_bn_relu_bwd_sums(gq, x, y, counts, mean, invstd)),
                                  ("roi_bn_relu_bwd_apply", 4, lambda: ops.roi_bn_relu_bwd_apply(gq, x, y, counts, mean, invstd, gamma, sums))):
            ts = RB._time(fn, args.rounds)
            med = statistics.median(ts)
            gbs = tensors * valid_bytes / (med * 1e-3) / 1e9
            results[f"{name} {label}"] = med
            print(f"{name:24s} {label:16s} median {med * 1e3:8.1f} us  min {min(ts) * 1e3:8.1f}  max {max(ts) * 1e3:8.1f}   {gbs:7.0f} GB/s "
                  f"({100 * gbs / COPY_RATE_GBS:4.1f} % of the {COPY_RATE_GBS / 1e3:.2f} TB/s copy rate)", flush=True)
    print(json.dumps({"rounds": args.rounds, "shape": args.shape, "proposals": P, "boxes": G, "batch_per_image": B, "sampling_ratio": args.ratio,
                      "median_ms": results}))


if __name__ == "__main__":
    main()
