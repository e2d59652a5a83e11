"""Time of the training side of the box branch of StandardROIHeads (afigan_amd/roi_heads.py: StandardROIHeads.losses; csrc/roi_loss.hip) at the
training configs' size -- N = 2 at 800 x 1344, four levels of 256 channels (strides 4 .. 32), 1000 proposals and 20 boxes per image,
BATCH_SIZE_PER_IMAGE 512, two FCs of 1024, 80 classes, 7 x 7 bins -- next to a torch-ROCm restatement of the detectron2 formulas on the same GPU
with the same weights: median (min / max) of device-event-timed runs after a warm-up.

    python tools/roi_loss_bench.py [--rounds 20] [--boxes 20] [--ratio 2]

Parts:
  label+sample+gather  afi_roi_label + afi_rpn_sample + afi_roi_gather_samples, against: cat([proposals, gt]), pairwise_iou as a G x R matrix per
                       image, max, nonzero + randperm sampling, index selects;
  loss                 afi_roi_box_loss (both losses and d loss / d predictor output), against F.cross_entropy, get_deltas and smooth L1 as
                       elementwise torch ops and autograd back to the predictor output;
  roi_align_bwd        afi_roi_align_bwd alone, against autograd's backward through the restated pooler;
  losses fwd+bwd       StandardROIHeads.losses and .backward() to the four feature maps and the eight parameters, against the restatement above,
                       torch's linear layers and autograd.
torchvision is not installed, so the baseline's pooler is a pure-torch ROIAlign: per level, the four corner values of every sample gathered by
index tensors, weighted and averaged per bin.  It needs one grid for all boxes, so both sides run POOLER_SAMPLING_RATIO = --ratio (2) rather
than the adaptive grid.  Before timing, the two sides are compared on one assignment: the restatement evaluated on the HIP side's own training
list must give its losses (printed).  No speed figure is a pass criterion."""
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

LEVELS = ["p2", "p3", "p4", "p5"]
S = 7


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


def build(ratio, channels=256, batch=512):
    import afigan_amd as amd
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": False, "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": LEVELS, "BATCH_SIZE_PER_IMAGE": batch},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "POOLER_RESOLUTION": S, "POOLER_SAMPLING_RATIO": ratio}})
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=4 * 2 ** i) for i, f in enumerate(LEVELS)})
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for k, p in h.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if k.endswith("bias") else 1.0 / math.sqrt(p.shape[1])))
    return h.cuda().trainable_()


class Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ------------------------------------------------------------------------------------------------ the restatement
def torch_assign(h, props, gt, gcls):
    """label_and_sample_proposals of one image: (boxes [n, 4], classes [n] with K for background, matched boxes [n, 4])"""
    cand = torch.cat([props, gt]) if h.proposal_append_gt else props
    area_g, area_c = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]), (cand[:, 2] - cand[:, 0]) * (cand[:, 3] - cand[:, 1])
    wh = (torch.min(gt[:, None, 2:], cand[:, 2:]) - torch.max(gt[:, None, :2], cand[:, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    iou = torch.where(inter > 0, inter / (area_g[:, None] + area_c - inter), torch.zeros((), device=gt.device))
    vals, midx = iou.max(dim=0)
    fg = vals >= h.iou_threshold
    pos, neg = torch.nonzero(fg).squeeze(1), torch.nonzero(~fg).squeeze(1)
    n_pos = min(pos.numel(), int(h.batch_size_per_image * h.positive_fraction))
    n_neg = min(neg.numel(), h.batch_size_per_image - n_pos)
    pos = pos[torch.randperm(pos.numel(), device=pos.device)[:n_pos]]
    neg = neg[torch.randperm(neg.numel(), device=neg.device)[:n_neg]]
    idx = torch.cat([pos, neg])
    cls = torch.cat([gcls[midx[pos]].long(), torch.full((n_neg,), h.num_classes, device=gt.device, dtype=torch.int64)])
    return cand[idx], cls, gt[midx[idx]]


def torch_roi_align(xs, boxes, img, min_level, ratio):
    """ROIAlignV2 of boxes [R, 4] (image index img [R]) on the levels xs (NCHW): [R, C, S, S]; every sample's four corners by index tensors."""
    R, C = boxes.shape[0], xs[0].shape[1]
    w, hgt = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    lvl = torch.floor(4 + torch.log2(torch.sqrt((w * hgt).clamp(min=1e-12)) / 224)).clamp(min_level, min_level + len(xs) - 1).long()
    out = torch.zeros((R, C, S, S), device=boxes.device, dtype=xs[0].dtype)
    grid = (torch.arange(S, device=boxes.device)[:, None] + (torch.arange(ratio, device=boxes.device)[None, :] + 0.5) / ratio).reshape(-1)
    for l, x in enumerate(xs):
        sel = torch.nonzero((lvl == min_level + l) & (w > 0) & (hgt > 0)).squeeze(1)
        if sel.numel() == 0:
            continue
        H, W = x.shape[2:]
        scale = 1.0 / (1 << (min_level + l))
        b = boxes[sel] * scale

        def axis(start, roi, size):
            v = start[:, None] - 0.5 + grid[None, :] * (roi[:, None] / S)
            ok = ((v >= -1) & (v <= size)).to(x.dtype)
            v = v.clamp(min=0)
            lo = v.floor().long().clamp(max=size - 1)
            last = lo >= size - 1
            v = torch.where(last, lo.to(v.dtype), v)
            hi = torch.where(last, lo, lo + 1)
            frac = v - lo
            return lo, hi, (1 - frac) * ok, frac * ok
        yl, yh, wyl, wyh = axis(b[:, 1], b[:, 3] - b[:, 1], H)
        xl, xh, wxl, wxh = axis(b[:, 0], b[:, 2] - b[:, 0], W)
        f = x.permute(0, 2, 3, 1)
        n = img[sel][:, None, None]
        val = (f[n, yl[:, :, None], xl[:, None, :]] * (wyl[:, :, None] * wxl[:, None, :])[..., None]
               + f[n, yl[:, :, None], xh[:, None, :]] * (wyl[:, :, None] * wxh[:, None, :])[..., None]
               + f[n, yh[:, :, None], xl[:, None, :]] * (wyh[:, :, None] * wxl[:, None, :])[..., None]
               + f[n, yh[:, :, None], xh[:, None, :]] * (wyh[:, :, None] * wxh[:, None, :])[..., None])
        out = out.index_copy(0, sel, val.view(-1, S, ratio, S, ratio, C).mean((2, 4)).permute(0, 3, 1, 2))
    return out


def torch_box_losses(h, pred_cls, pred_box, boxes, cls, gboxes):
    K = h.num_classes
    n = cls.numel()
    loss_cls = F.cross_entropy(pred_cls, cls, reduction="sum") / n
    fg = torch.nonzero(cls < K).squeeze(1)
    a, b = boxes[fg], gboxes[fg]
    sw, sh, tw, th = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    wx, wy, ww, wh = h.box_weights
    tgt = torch.stack([wx * (b[:, 0] + 0.5 * tw - a[:, 0] - 0.5 * sw) / sw, wy * (b[:, 1] + 0.5 * th - a[:, 1] - 0.5 * sh) / sh,
                       ww * torch.log(tw / sw), wh * torch.log(th / sh)], 1)
    cols = 4 * cls[fg][:, None] + torch.arange(4, device=cls.device)
    d = (pred_box[fg[:, None], cols] - tgt).abs()
    beta = h.smooth_l1_beta
    loss_box = (d.sum() if beta < 1e-5 else torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta).sum()) / n
    return loss_cls, loss_box


def torch_head(h, pooled):
    x = pooled.flatten(1)
    for fc in h.box_head.fcs:
        x = F.relu(F.linear(x, fc.weight, fc.bias))
    pr = h.box_predictor
    return F.linear(x, pr.cls_score.weight, pr.cls_score.bias), F.linear(x, pr.bbox_pred.weight, pr.bbox_pred.bias)


def torch_losses(h, xs, props, gts, gcls, ratio, given=None):
    lists = given if given is not None else [torch_assign(h, p, g, c) for p, g, c in zip(props, gts, gcls)]
    boxes, cls, gb = (torch.cat([l[i] for l in lists]) for i in range(3))
    img = torch.cat([torch.full((l[0].shape[0],), n, device=boxes.device, dtype=torch.int64) for n, l in enumerate(lists)])
    pooled = torch_roi_align(xs, boxes, img, h.box_pooler.min_level, ratio)
    pc, pb = torch_head(h, pooled)
    return torch_box_losses(h, pc, pb, boxes, cls, gb)


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
        near = gt[torch.randint(0, gt.shape[0], (P // 4,), generator=g)]           # a quarter of the proposals sit on a box, as an RPN's do
        near = near + (torch.rand(near.shape, generator=g) - 0.5) * 0.2 * (near[:, 2:] - near[:, :2]).repeat(1, 2)
        gts.append(gt.cuda())
        gcls.append(torch.randint(0, K, (gt.shape[0],), generator=g).to(torch.int32).cuda())
        props.append(torch.cat([near, rand_boxes(P - P // 4, 8, 600)]).cuda())
    prop_obj = [Obj(proposal_boxes=p) for p in props]
    tgt_obj = [Obj(gt_boxes=b, gt_classes=c) for b, c in zip(gts, gcls)]
    pboxes, pcounts = h._padded_proposals(prop_obj, N, "cuda")
    gt_pad, gc_pad, gcounts = h._targets(tgt_obj, N, "cuda")
    R = P + gt_pad.shape[1]
    keys = torch.randint(-2 ** 31, 2 ** 31, (N, R), device="cuda", dtype=torch.int32)

    # the two sides on ONE assignment (the HIP side's)
    out = h.losses(None, feats, prop_obj, tgt_obj, keys)
    asg = {k: v.clone() for k, v in h.last_assignment.items()}
    cnt = asg["counts"].tolist()
    given = [(asg["boxes"][n, :cnt[n]], asg["gt_classes"][n, :cnt[n]].long(), asg["gt_boxes"][n, :cnt[n]]) for n in range(N)]
    tc, tb = torch_losses(h, xs, props, gts, gcls, args.ratio, given)
    print(f"{P} proposals + {G} boxes per image, B = {B}: sampled foreground {asg['n_pos'].tolist()}, background {asg['n_neg'].tolist()}")
    print(f"losses on the HIP side's assignment: HIP cls {out['loss_cls'].item():.7g} box {out['loss_box_reg'].item():.7g}; "
          f"torch restatement cls {tc.item():.7g} box {tb.item():.7g}", flush=True)
    pred = asg["pred"]
    pred_t = pred.detach().clone().requires_grad_(True)
    boxes_t, cls_t, gb_t = (torch.cat([l[i] for l in given]) for i in range(3))
    rows_t = torch.cat([torch.arange(cnt[n], device="cuda") + n * B for n in range(N)])
    dpooled = torch.randn((N * B, S, S, 256), device="cuda").permute(0, 3, 1, 2)
    level_shapes = [tuple(x.shape[2:]) for x in xs]
    img_t = torch.cat([torch.full((cnt[n],), n, device="cuda", dtype=torch.int64) for n in range(N)])
    pooled_t = torch_roi_align(xs, boxes_t, img_t, h.box_pooler.min_level, args.ratio)
    dp_t = dpooled[rows_t].contiguous()

    def hip_assign():
        labels, midx = ops.roi_label(pboxes, pcounts, gt_pad, gcounts, h.iou_threshold, h.proposal_append_gt)
        labels, sidx, n_pos, n_neg = ops.rpn_sample(labels, keys, B, h.positive_fraction)
        return ops.roi_gather_samples(pboxes, pcounts, gt_pad, gc_pad, gcounts, midx, sidx, n_pos, n_neg, K, h.proposal_append_gt)

    def torch_assign_all():
        with torch.no_grad():
            return [torch_assign(h, p, b, c) for p, b, c in zip(props, gts, gcls)]

    def hip_loss():
        return ops.roi_box_loss(pred, K, False, asg["boxes"], asg["counts"], asg["gt_classes"], asg["gt_boxes"], h.box_weights, h.smooth_l1_beta)

    def torch_loss():
        pred_t.grad = None
        p = pred_t[rows_t]
        lc, lb = torch_box_losses(h, p[:, :K + 1], p[:, K + 1:K + 1 + 4 * K], boxes_t, cls_t, gb_t)
        (lc + lb).backward()

    def hip_align_bwd():
        return ops.roi_align_bwd(dpooled, level_shapes, h.box_pooler.min_level, asg["boxes"], asg["counts"], args.ratio)

    def torch_align_bwd():
        return torch.autograd.grad(pooled_t, xs, dp_t, retain_graph=True, allow_unused=True)

    def hip_full():
        o = h.losses(None, feats, prop_obj, tgt_obj, keys)
        (o["loss_cls"] + o["loss_box_reg"]).backward()

    def torch_full():
        c, b = torch_losses(h, xs, props, gts, gcls, args.ratio)
        (c + b).backward()

    results = {}
    for name, fn in (("label+sample+gather HIP", hip_assign), ("label+sample+gather torch", torch_assign_all), ("loss HIP", hip_loss),
                     ("loss torch", torch_loss), ("roi_align_bwd HIP", hip_align_bwd), ("roi_align_bwd torch", torch_align_bwd),
                     ("losses fwd+bwd HIP", hip_full), ("losses fwd+bwd torch", torch_full)):
        ts = _time(fn, args.rounds)
        results[name] = statistics.median(ts)
        print(f"{name:26s} {args.shape:>12s}: median {results[name]:8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  ({len(ts)} rounds)", flush=True)
    print(json.dumps({"rounds": args.rounds, "shape": args.shape, "proposals": P, "boxes": G, "batch_per_image": B, "sampling_ratio": args.ratio,
                      "median_ms": results,
                      "baseline": "G x R IoU matrix, max / nonzero / randperm, F.cross_entropy + elementwise smooth L1, F.linear FCs, "
                                  "pure-torch gather ROIAlign, autograd"}))


if __name__ == "__main__":
    main()
