"""Time of the training side of the mask branch of StandardROIHeads (afigan_amd/roi_heads.py: _ROIMaskLossFn; csrc/mask_loss.hip) at the
training configs' size -- N = 2 at 800 x 1344, four levels of 256 channels, BATCH_SIZE_PER_IMAGE 512 with POSITIVE_FRACTION 0.25 (Bf = 128
rows per image), 80 classes, NUM_CONV 4, 14 x 14 bins, COCO-like polygons of 20 .. 200 vertices -- next to a torch-ROCm restatement on the same
GPU with the same weights: median (min / max) of device-event-timed runs after a warm-up.

    python tools/mask_loss_bench.py [--rounds 20] [--boxes 20] [--ratio 2]

Parts:
  targets             afi_mask_targets on the call's uploaded polygons.  There is no torch rasteriser: the baseline is the HOST rasterisation of
                      the same rows by the plain-loop checker (tests/mask_loss_f64.py, Python), timed once by the wall clock -- a statement of
                      what the kernel replaces, not a competitor;
  loss + dz           afi_mask_loss, against the selected logits as one einsum, F.binary_cross_entropy_with_logits and autograd back to them;
  mask_pred_bwd       afi_mask_pred_bwd, against dh, dW (index_add_ by class) and db as torch ops;
  loss_mask fwd+bwd   _ROIMaskLossFn forward and backward to the four feature maps and the twelve parameters on a given training list, against
                      tools/roi_loss_bench.py's pure-torch ROIAlign, F.conv2d / F.conv_transpose2d and autograd.
Both sides run POOLER_SAMPLING_RATIO = --ratio (the torch pooler needs one grid for all boxes).  Before timing, the restatement evaluated on
the HIP side's own list and targets must give its loss (printed).  Also printed: the share of the Bf rows that are padding (Bf - n_pos: the head
runs on them, pooled as zeros) and the size of dh.  No speed figure is a pass criterion."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import roi_loss_bench as RB  # noqa: E402

LEVELS = RB.LEVELS
S = 14
RB.S = S                     # its pure-torch ROIAlign reads the pooled size from its module


def build(ratio, channels=256, batch=512, num_conv=4):
    import afigan_amd as amd
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": True, "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": LEVELS, "BATCH_SIZE_PER_IMAGE": batch},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "POOLER_RESOLUTION": 7, "POOLER_SAMPLING_RATIO": ratio},
                               "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": num_conv, "CONV_DIM": channels,
                                                 "POOLER_RESOLUTION": S, "POOLER_SAMPLING_RATIO": ratio}})
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=4 * 2 ** i) for i, f in enumerate(LEVELS)}, masks=True)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for k, p in h.named_parameters():
            fan = p[0].numel() if "deconv" not in k else p.shape[0]
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if k.endswith("bias") else math.sqrt(2.0 / fan)))
    return h.cuda().trainable_(mask_head=True)


def polygon(box, rng):
    """A closed curve of 20 .. 200 vertices inside the box: an ellipse whose radius wobbles."""
    k = int(rng.integers(20, 201))
    a = np.sort(rng.uniform(0, 2 * math.pi, k))
    r = 0.35 + 0.12 * np.sin(3 * a + rng.uniform(0, 6)) + rng.uniform(-0.02, 0.02, k)
    cx, cy, w, hgt = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2, box[2] - box[0], box[3] - box[1]
    return np.stack([cx + r * w * np.cos(a), cy + r * hgt * np.sin(a)], 1).reshape(-1)


def torch_selected(hv, w, b, cls):
    """hv [R, 4, C, S, S] -> the rows' own-class logits [R, 4, S, S]"""
    return torch.einsum("rpcyx,rc->rpyx", hv, w[cls]) + b[cls][:, None, None, None]


def torch_mask_head(h, pooled):
    mh = h.mask_head
    x = pooled
    for conv in mh.conv_norm_relus:
        x = F.relu(F.conv2d(x, conv.weight, conv.bias, padding=1))
    x = F.relu(F.conv_transpose2d(x, mh.deconv.weight, mh.deconv.bias, stride=2))
    return F.conv2d(x, mh.predictor.weight, mh.predictor.bias)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--boxes", type=int, default=20)
    ap.add_argument("--proposals", type=int, default=1000)
    ap.add_argument("--ratio", type=int, default=2)
    ap.add_argument("--shape", default="2x800x1344")
    args = ap.parse_args()
    from afigan_amd import ops
    from afigan_amd.roi_heads import _ROIMaskLossFn
    import mask_loss_f64 as Q
    N, H, W = (int(v) for v in args.shape.split("x"))
    P, G = args.proposals, args.boxes
    h = build(args.ratio)
    K, B, Bf = h.num_classes, h.batch_size_per_image, h.mask_batch_per_image
    g = torch.Generator().manual_seed(1)
    rng = np.random.default_rng(1)
    xs = [torch.randn((N, 256, -(-H // (4 * 2 ** i)), -(-W // (4 * 2 ** i))), generator=g).cuda() for i in range(4)]
    feats = {f: x.contiguous(memory_format=torch.channels_last).requires_grad_(True) for f, x in zip(LEVELS, xs)}
    xs = [x.requires_grad_(True) for x in xs]

    def rand_boxes(n, lo, hi):
        c = torch.rand((n, 2), generator=g) * torch.tensor([W, H])
        wh = torch.exp(torch.rand((n, 2), generator=g) * math.log(hi / lo)) * lo
        return torch.cat([c - wh / 2, c + wh / 2], 1).clamp(min=0).minimum(torch.tensor([W, H, W, H]).float())
    gts, gcls, props, inst = [], [], [], []
    for n in range(N):
        gt = rand_boxes(G, 24, 500)
        gt = gt[((gt[:, 2] - gt[:, 0]) > 4) & ((gt[:, 3] - gt[:, 1]) > 4)]
        near = gt[torch.randint(0, gt.shape[0], (P // 4,), generator=g)]           # a quarter of the proposals sit on a box, as an RPN's do
        near = near + (torch.rand(near.shape, generator=g) - 0.5) * 0.2 * (near[:, 2:] - near[:, :2]).repeat(1, 2)
        inst.append([[polygon(b, rng)] for b in gt.double().numpy()])
        gts.append(gt.cuda())
        gcls.append(torch.randint(0, K, (gt.shape[0],), generator=g).to(torch.int32).cuda())
        props.append(torch.cat([near, rand_boxes(P - P // 4, 8, 600)]).cuda())
    prop_obj = [RB.Obj(proposal_boxes=p) for p in props]
    tgt_obj = [RB.Obj(gt_boxes=b, gt_classes=c, gt_masks=m) for b, c, m in zip(gts, gcls, inst)]
    gt_pad, gc_pad, gcounts = h._targets(tgt_obj, N, "cuda")
    gmax = gt_pad.shape[1]
    keys = torch.randint(-2 ** 31, 2 ** 31, (N, P + gmax), device="cuda", dtype=torch.int32)
    polys = ops.mask_polygons(inst, N, gmax, "cuda")

    out = h.losses(None, feats, prop_obj, tgt_obj, keys)
    a = dict(h.last_assignment)
    n_pos = a["n_pos"].tolist()
    cfg, tg, hh, dz = a["counts_fg"], a["mask_targets"], a["mask_deconv"], a["mask_dz"]
    cls = a["gt_classes"][:, :Bf]
    wp, bp = h._prepare_mask()[2]
    nv = [len(p[0]) // 2 for im in inst for p in im]
    print(f"{P} proposals + {G} boxes per image, B = {B}, Bf = {Bf}: foreground rows {n_pos}; padding rows {[Bf - p for p in n_pos]} = "
          f"{100.0 * sum(Bf - p for p in n_pos) / (N * Bf):.1f} % of the mask head's rows; polygons of {min(nv)} .. {max(nv)} vertices")
    print(f"dh [{N * Bf}][{S}][{S}][4][256] fp32 = {N * Bf * S * S * 4 * 256 * 4 / 2 ** 20:.1f} MiB written by afi_mask_pred_bwd and read twice by "
          "the deconv's backward")
    # the restatement on the HIP side's own list and targets
    live = torch.cat([torch.arange(n_pos[n], device="cuda") + n * Bf for n in range(N)])
    boxes_t = torch.cat([a["boxes"][n, :n_pos[n]] for n in range(N)])
    img_t = torch.cat([torch.full((n_pos[n],), n, device="cuda", dtype=torch.int64) for n in range(N)])
    cls_t = cls.reshape(-1)[live].long()
    t_img = tg.view(N * Bf, 2 * S, 2 * S)[live].float()

    def torch_full():
        pooled = RB.torch_roi_align(xs, boxes_t, img_t, h.mask_pooler.min_level, args.ratio)
        logits = torch_mask_head(h, pooled)
        loss = F.binary_cross_entropy_with_logits(logits[torch.arange(cls_t.numel(), device="cuda"), cls_t], t_img, reduction="mean")
        loss.backward()
        return loss
    print(f"loss_mask on the HIP side's list and targets: HIP {out['loss_mask'].item():.7g}; torch restatement {torch_full().item():.7g}", flush=True)

    t0 = time.perf_counter()
    an = {k: v.cpu().numpy() for k, v in a.items() if k in ("boxes", "sampled_idx", "matched_idx", "n_pos")}
    want, _ = Q.targets(inst, an["boxes"], an["sampled_idx"], an["matched_idx"], an["n_pos"], gcounts.cpu().numpy(), Bf, 2 * S)
    host_ms = (time.perf_counter() - t0) * 1e3
    print(f"targets: the host checker's masks equal the kernel's: {bool(np.array_equal(want, tg.cpu().numpy()))}")

    hv = hh.permute(0, 2, 3, 1).reshape(N * Bf, S, S, 4, 256).permute(0, 3, 4, 1, 2)[live]          # [R', 4, C, S, S] (a view)
    t_ph = tg.view(N * Bf, S, 2, S, 2).permute(0, 2, 4, 1, 3).reshape(N * Bf, 4, S, S)[live].float()
    dz_t = dz.permute(0, 3, 1, 2)[live]

    def hip_targets():
        return ops.mask_targets(*polys, a["boxes"], a["sampled_idx"], a["matched_idx"], gcounts, gmax, a["n_pos"], Bf, 2 * S)

    def hip_loss():
        return ops.mask_loss(hh, wp, bp, cls, cfg, tg)

    def torch_loss():
        z = torch_selected(hv, wp, bp, cls_t).requires_grad_(True)
        return torch.autograd.grad(F.binary_cross_entropy_with_logits(z, t_ph, reduction="mean"), z)

    def hip_pred_bwd():
        return ops.mask_pred_bwd(hh, dz, wp, cls, cfg)

    def torch_pred_bwd():
        dh = dz_t[:, :, None] * wp[cls_t][:, None, :, None, None] * (hv > 0)
        dW = torch.zeros_like(wp).index_add_(0, cls_t, torch.einsum("rpyx,rpcyx->rc", dz_t, hv))
        db = torch.zeros_like(bp).index_add_(0, cls_t, dz_t.sum((1, 2, 3)))
        return dh, dW, db
    mh = h.mask_head
    mparams = [t for l in mh.conv_norm_relus + [mh.deconv, mh.predictor] for t in (l.weight, l.bias)]
    fx = [feats[f] for f in LEVELS]

    def hip_full():
        _ROIMaskLossFn.apply(h, polys, gcounts, gmax, 4, *fx, *mparams).backward()

    results = {"targets host checker (wall clock, once)": host_ms}
    print(f"{'targets host checker':26s} {args.shape:>12s}: {host_ms:8.1f} ms  (Python on the CPU, wall clock, one run)")
    for name, fn in (("targets HIP", hip_targets), ("loss+dz HIP", hip_loss), ("loss+dz torch", torch_loss), ("mask_pred_bwd HIP", hip_pred_bwd),
                     ("mask_pred_bwd torch", torch_pred_bwd), ("loss_mask fwd+bwd HIP", hip_full), ("loss_mask fwd+bwd torch", torch_full)):
        ts = RB._time(fn, args.rounds)
        results[name] = statistics.median(ts)
        print(f"{name:26s} {args.shape:>12s}: median {results[name]:8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  ({len(ts)} rounds)", flush=True)
    print(json.dumps({"rounds": args.rounds, "shape": args.shape, "proposals": P, "boxes": G, "batch_per_image": B, "mask_rows_per_image": Bf,
                      "n_pos": n_pos, "sampling_ratio": args.ratio, "median_ms": results,
                      "baseline": "pure-torch gather ROIAlign, F.conv2d / F.conv_transpose2d, einsum-selected logits, "
                                  "F.binary_cross_entropy_with_logits, autograd; targets: the host checker"}))


if __name__ == "__main__":
    main()
