"""Time of the RPN's training side (afigan_amd/rpn.py: RPN.losses; csrc/rpn_loss.hip) at the training configs' size -- N = 2, 800 x 1333 (padded to
800 x 1344), five levels, A = 3, about 267 000 anchors and 20 boxes per image, BATCH_SIZE_PER_IMAGE 256 -- next to a torch-eager restatement of
the detectron2 formulas on the same GPU with the same weights: median (min / max) of CUDA-event-timed runs after a warm-up.

    python tools/rpn_loss_bench.py [--rounds 20] [--boxes 20]

Parts:
  assign + loss   afi_rpn_match + afi_rpn_sample + afi_rpn_loss on given head outputs, against: the anchors materialised, pairwise_iou as a
                  G x R matrix per image, max along both axes, the == promotion, nonzero + randperm sampling, get_deltas and the two summed
                  losses as elementwise torch ops (what detectron2 v0.1.1 runs);
  losses fwd+bwd  RPN.losses and .backward() to the five feature maps and the six parameters, against F.conv2d (MIOpen) for the head, the
                  restatement above and torch autograd.
Before timing, the two sides are compared on one assignment: the restatement evaluated on the HIP side's own labels and sample must give its
losses (printed).  No speed figure is a pass criterion."""
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

LEVELS = ["p2", "p3", "p4", "p5", "p6"]


def _time(fn, rounds, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def build(channels=256):
    import afigan_amd as amd
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[32], [64], [128], [256], [512]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": LEVELS, "PRE_NMS_TOPK_TEST": 1000, "POST_NMS_TOPK_TEST": 1000}})
    m = amd.RPN(cfg, {f: ShapeSpec(channels=channels, stride=4 * 2 ** i) for i, f in enumerate(LEVELS)})
    g = torch.Generator().manual_seed(0)
    for name, s in (("conv", 1.0 / math.sqrt(9 * channels)), ("objectness_logits", 1.0 / math.sqrt(channels)), ("anchor_deltas", 0.6 / math.sqrt(channels))):
        layer = getattr(m.rpn_head, name)
        layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * s)
        layer.bias.copy_(torch.randn(layer.bias.shape, generator=g) * 0.1)
    return m.cuda().trainable_(True)


class GT:
    def __init__(self, boxes):
        self.gt_boxes = boxes


def torch_anchors(m, shapes):
    out = []
    for l, (H, W) in enumerate(shapes):
        s = m.anchor_generator.strides[l]
        ys, xs = torch.meshgrid(torch.arange(H, device="cuda") * s, torch.arange(W, device="cuda") * s, indexing="ij")
        shift = torch.stack([xs, ys, xs, ys], -1).reshape(-1, 1, 4).float()
        out.append((shift + m.anchor_generator.cell_anchors[l][None]).reshape(-1, 4))
    return torch.cat(out)


def torch_head(m, xs):
    h = m.rpn_head
    out = []
    for x in xs:
        t = F.relu(F.conv2d(x, h.conv.weight, h.conv.bias, padding=1))
        out.append((F.conv2d(t, h.objectness_logits.weight, h.objectness_logits.bias), F.conv2d(t, h.anchor_deltas.weight, h.anchor_deltas.bias)))
    return out


def torch_flat(heads, n):
    """logits [R] and deltas [R, 4] of image n in anchor order"""
    lg = torch.cat([h[0][n].permute(1, 2, 0).reshape(-1) for h in heads])
    dl = torch.cat([h[1][n].permute(1, 2, 0).reshape(-1, 4) for h in heads])
    return lg, dl


def torch_assign(m, anchors, gt):
    """Matcher with low-quality matches and subsample_labels: (positive indices, negative indices, matched box per anchor)"""
    area_g, area_a = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]), (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
    wh = (torch.min(gt[:, None, 2:], anchors[:, 2:]) - torch.max(gt[:, None, :2], anchors[:, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    iou = torch.where(inter > 0, inter / (area_g[:, None] + area_a - inter), torch.zeros((), device=gt.device))
    vals, midx = iou.max(dim=0)
    labels = torch.ones_like(midx, dtype=torch.int8)
    labels[vals < m.iou_thresholds[1]] = -1
    labels[vals < m.iou_thresholds[0]] = 0
    best, _ = iou.max(dim=1)
    labels[torch.nonzero(iou == best[:, None])[:, 1]] = 1
    pos, neg = torch.nonzero(labels == 1).squeeze(1), torch.nonzero(labels == 0).squeeze(1)
    n_pos = min(pos.numel(), int(m.batch_size_per_image * m.positive_fraction))
    n_neg = min(neg.numel(), m.batch_size_per_image - n_pos)
    pos = pos[torch.randperm(pos.numel(), device=pos.device)[:n_pos]]
    neg = neg[torch.randperm(neg.numel(), device=neg.device)[:n_neg]]
    return pos, neg, midx


def torch_loss(m, lg, dl, anchors, gt, pos, neg, midx):
    """rpn_losses of one image's sample, unscaled sums"""
    idx = torch.cat([pos, neg])
    t = torch.cat([torch.ones_like(pos, dtype=torch.float32), torch.zeros_like(neg, dtype=torch.float32)])
    cls = F.binary_cross_entropy_with_logits(lg[idx], t, reduction="sum")
    a, b = anchors[pos], gt[midx[pos].long()]
    sw, sh, tw, th = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    wx, wy, ww, wh = m.box_weights
    tgt = torch.stack([wx * (b[:, 0] + 0.5 * tw - a[:, 0] - 0.5 * sw) / sw, wy * (b[:, 1] + 0.5 * th - a[:, 1] - 0.5 * sh) / sh,
                       ww * torch.log(tw / sw), wh * torch.log(th / sh)], 1)
    d = (dl[pos] - tgt).abs()
    beta = m.smooth_l1_beta
    loc = d.sum() if beta < 1e-5 else torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta).sum()
    return cls, loc


def torch_losses(m, heads, anchors, gts, assignment=None):
    N = len(gts)
    cls = loc = 0.0
    for n in range(N):
        lg, dl = torch_flat(heads, n)
        pos, neg, midx = assignment[n] if assignment is not None else torch_assign(m, anchors, gts[n])
        c, l = torch_loss(m, lg, dl, anchors, gts[n], pos, neg, midx)
        cls, loc = cls + c, loc + l
    s = m.loss_weight / (m.batch_size_per_image * N)
    return cls * s, loc * s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--boxes", type=int, default=20)
    ap.add_argument("--shape", default="2x800x1344")
    args = ap.parse_args()
    from afigan_amd import ops
    N, H, W = (int(v) for v in args.shape.split("x"))
    m = build()
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn((N, 256, -(-H // (4 * 2 ** i)), -(-W // (4 * 2 ** i))), generator=g).cuda() for i in range(5)]
    feats = {f: x.contiguous(memory_format=torch.channels_last).requires_grad_(True) for f, x in zip(LEVELS, xs)}
    xs = [x.requires_grad_(True) for x in xs]
    gts = []
    for n in range(N):
        c = torch.rand((args.boxes, 2), generator=g) * torch.tensor([W, H])
        wh = 16 + torch.rand((args.boxes, 2), generator=g) ** 2 * 400
        gts.append(torch.cat([c - wh / 2, c + wh / 2], 1).clamp(min=0).cuda())
    gt_inst = [GT(b) for b in gts]
    ag, A = m.anchor_generator, m.num_anchors
    cell = torch.stack(list(ag.cell_anchors)).contiguous()
    with torch.no_grad():
        m.eval()
        heads = m.head(feats)
        m.train()
        theads = torch_head(m, xs)
        anchors = torch_anchors(m, [tuple(h.shape[2:]) for h in heads])
    R = anchors.shape[0]
    gt_pad = torch.zeros((N, args.boxes, 4), device="cuda")
    for n in range(N):
        gt_pad[n] = gts[n]
    counts = torch.full((N,), args.boxes, dtype=torch.int32, device="cuda")
    keys = torch.randint(-2 ** 31, 2 ** 31, (N, R), device="cuda", dtype=torch.int32)
    scale = m.loss_weight / (m.batch_size_per_image * N)

    def hip_assign_loss():
        labels, midx = ops.rpn_match([tuple(h.shape[2:]) for h in heads], ag.strides, cell, A, gt_pad, counts, m.iou_thresholds)
        labels, sidx, n_pos, n_neg = ops.rpn_sample(labels, keys, m.batch_size_per_image, m.positive_fraction)
        return ops.rpn_loss(heads, ag.strides, cell, A, gt_pad, counts, midx, sidx, n_pos, n_neg, m.box_weights, m.smooth_l1_beta, scale, scale)[0]

    def torch_assign_loss():
        with torch.no_grad():
            return torch_losses(m, theads, anchors, gts)

    def hip_full():
        out = m.losses(None, feats, gt_inst, keys)
        (out["loss_rpn_cls"] + out["loss_rpn_loc"]).backward()

    def torch_full():
        c, l = torch_losses(m, torch_head(m, xs), anchors, gts)
        (c + l).backward()

    # the two sides on ONE assignment (the HIP side's)
    out = m.losses(None, feats, gt_inst, keys)
    asg = m.last_assignment
    n_pos, n_neg = asg["n_pos"].tolist(), asg["n_neg"].tolist()
    given = [(asg["sampled_idx"][n, :n_pos[n]].long(), asg["sampled_idx"][n, n_pos[n]:n_pos[n] + n_neg[n]].long(), asg["matched_idx"][n]) for n in range(N)]
    with torch.no_grad():
        tc, tl = torch_losses(m, theads, anchors, gts, given)
        pos_t = [torch_assign(m, anchors, gts[n])[0].numel() for n in range(N)]
    print(f"R = {R} anchors, {args.boxes} boxes per image; sampled positives HIP {n_pos} (torch restatement {pos_t}), negatives {n_neg}")
    print(f"losses on the HIP side's assignment: HIP cls {out['loss_rpn_cls'].item():.7g} loc {out['loss_rpn_loc'].item():.7g}; "
          f"torch restatement cls {tc.item():.7g} loc {tl.item():.7g}", flush=True)
    results = {}
    for name, fn in (("assign+loss HIP", hip_assign_loss), ("assign+loss torch", torch_assign_loss), ("losses fwd+bwd HIP", hip_full),
                     ("losses fwd+bwd torch", torch_full)):
        ts = _time(fn, args.rounds)
        results[name] = statistics.median(ts)
        print(f"{name:22s} {args.shape:>12s}: median {results[name]:8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  ({len(ts)} rounds)", flush=True)
    print(json.dumps({"rounds": args.rounds, "shape": args.shape, "anchors": R, "boxes": args.boxes, "median_ms": results,
                      "baseline": "anchors materialised, G x R IoU matrix, max / nonzero / randperm, elementwise losses; F.conv2d head + autograd"}))


if __name__ == "__main__":
    main()
