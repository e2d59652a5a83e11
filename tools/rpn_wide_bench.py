"""Time of the RPN's selection at the reference's TRAINING settings (A = 3, PRE_NMS_TOPK_TRAIN 2000, POST_NMS_TOPK_TRAIN 1000, NMS_THRESH 0.7, five
levels at 2 x 800 x 1344: four lists of 2000 on the wide kernels of csrc/rpn.hip, p6's 819 on the narrow ones), whole and stage by stage, next
to a torch-eager restatement on the same head outputs, and afi_rpn_nms_wide against afi_rpn_nms on the same lists of 1000 boxes: median
(min / max) of 20 device-event-timed runs after 3 warm-ups.  Prints one line per part and a JSON summary line.  No figure is a pass criterion.

    python tools/rpn_wide_bench.py [--shape 2x800x1344] [--rounds 20] [--no-torch]

The torch restatement (torch alone: there is no torchvision here): per level torch.topk(sorted=True) + gather + the decode as elementwise ops,
the IoU matrix of each (image, level) list on the device and the greedy sweep over it 64 rows at a time -- the 64 x 64 diagonal block resolved
on the host, the kept rows' suppression OR-ed on the device -- then cat + sort: tools/rpn_bench.py's baseline at the training values."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = ["p2", "p3", "p4", "p5", "p6"]
CLAMP = math.log(1000.0 / 16)
PRE_K, POST_K = 2000, 1000


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
                               "RPN": {"IN_FEATURES": LEVELS, "PRE_NMS_TOPK_TEST": 1000, "POST_NMS_TOPK_TEST": 1000, "PRE_NMS_TOPK_TRAIN": PRE_K,
                                       "POST_NMS_TOPK_TRAIN": POST_K, "NMS_THRESH": 0.7}})
    m = amd.RPN(cfg, {f: ShapeSpec(channels=channels, stride=4 * 2 ** i) for i, f in enumerate(LEVELS)})
    g = torch.Generator().manual_seed(0)
    for name, s in (("conv", 1.0 / math.sqrt(9 * channels)), ("objectness_logits", 1.0 / math.sqrt(channels)), ("anchor_deltas", 0.6 / math.sqrt(channels))):
        layer = getattr(m.rpn_head, name)
        layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * s)
        layer.bias.copy_(torch.randn(layer.bias.shape, generator=g) * 0.1)
    return m.cuda().eval()


def torch_nms(boxes, thresh):
    """Greedy NMS of boxes [k, 4] in list order with torch alone: keep mask [k]."""
    k = boxes.shape[0]
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    wh = (torch.min(boxes[:, None, 2:], boxes[None, :, 2:]) - torch.max(boxes[:, None, :2], boxes[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    over = (inter / (area[:, None] + area[None, :] - inter) > thresh).triu(1)
    sup = torch.zeros(k, dtype=torch.bool, device=boxes.device)
    keep = torch.zeros(k, dtype=torch.bool, device=boxes.device)
    for c in range(0, k, 64):
        e = min(c + 64, k)
        blk = over[c:e, c:e].cpu()
        s = sup[c:e].cpu()
        kp = torch.zeros(e - c, dtype=torch.bool)
        for i in range(e - c):
            if not s[i]:
                kp[i] = True
                s |= blk[i]
        kd = kp.to(boxes.device)
        keep[c:e] = kd
        sup |= over[c:e][kd].any(0)
    return keep


def torch_select(m, heads, image_hw, pre_k, post_k):
    """heads: the pixel-major head outputs [N, Cpad, H, W] (channels 0..A-1 the logits, A..5A-1 the deltas)."""
    A, res = m.num_anchors, []
    wx, wy, ww, wh = m.box_weights
    for n in range(heads[0].shape[0]):
        bs, ls = [], []
        for l, hd in enumerate(heads):
            H, W = hd.shape[2:]
            flat = hd[n, :A].permute(1, 2, 0).reshape(-1)
            v, i = torch.topk(flat, min(pre_k, flat.numel()), sorted=True)
            d = hd[n, A:5 * A].reshape(A, 4, H, W).permute(2, 3, 0, 1).reshape(-1, 4)[i]
            a, pix = i % A, i // A
            s = m.anchor_generator.strides[l]
            shift = torch.stack([(pix % W) * s, (pix // W) * s, (pix % W) * s, (pix // W) * s], 1).float()
            an = m.anchor_generator.cell_anchors[l][a] + shift
            w, h = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
            cx, cy = an[:, 0] + 0.5 * w, an[:, 1] + 0.5 * h
            pcx, pcy = d[:, 0] / wx * w + cx, d[:, 1] / wy * h + cy
            pw, ph = torch.exp((d[:, 2] / ww).clamp(max=CLAMP)) * w, torch.exp((d[:, 3] / wh).clamp(max=CLAMP)) * h
            b = torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 1)
            b[:, 0::2] = torch.minimum(b[:, 0::2].clamp(min=0), image_hw[n, 1])
            b[:, 1::2] = torch.minimum(b[:, 1::2].clamp(min=0), image_hw[n, 0])
            ok = ((b[:, 2] - b[:, 0]) > m.min_box_side_len) & ((b[:, 3] - b[:, 1]) > m.min_box_side_len)
            b, v = b[ok], v[ok]
            kp = torch_nms(b, m.nms_thresh)
            bs.append(b[kp])
            ls.append(v[kp])
        b, v = torch.cat(bs), torch.cat(ls)
        o = torch.sort(v, descending=True, stable=True).indices[:post_k]
        res.append((b[o], v[o]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="2x800x1344")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from afigan_amd import ops
    from afigan_amd.rpn import SCALE_CLAMP
    out = {}

    def row(name, fn):
        ts = _time(fn, args.rounds)
        out[name] = [statistics.median(ts), min(ts), max(ts)]
        print(f"{name:44s} median {out[name][0]:8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  ({len(ts)} runs)", flush=True)

    with torch.no_grad():
        m = build()
        N, H, W = (int(v) for v in args.shape.split("x"))
        g = torch.Generator().manual_seed(1)
        feats = {f: torch.randn((N, 256, -(-H // (4 * 2 ** i)), -(-W // (4 * 2 ** i))), generator=g).cuda().contiguous(memory_format=torch.channels_last)
                 for i, f in enumerate(LEVELS)}
        hw = torch.tensor([[H, W]] * N, dtype=torch.float32, device="cuda")
        heads = m.head(feats)
        A, ag = m.num_anchors, m.anchor_generator
        r = m.select(heads, hw, PRE_K, POST_K)
        off = r["level_off"]
        ks = [off[l + 1] - off[l] for l in range(len(heads))]
        wide = [l for l, k in enumerate(ks) if k > ops.RPN_MAX_TOPK]
        narrow = [l for l, k in enumerate(ks) if k <= ops.RPN_MAX_TOPK]
        print(f"lists per level {ks}: wide levels {wide}, narrow {narrow}; proposals {r['counts'].tolist()}", flush=True)
        sl = [slice(off[l], off[l + 1]) for l in range(len(heads))]
        vals, idx, boxes, valid, keep = (r[k] for k in ("vals", "idx", "level_boxes", "valid", "keep"))

        def stage(fn, levels):
            def run():
                for l in levels:
                    fn(l)
            return run
        row(f"selection {PRE_K} / {POST_K} HIP", lambda: m.select(heads, hw, PRE_K, POST_K))
        row(f"  afi_rpn_topk_wide, {len(wide)} levels", stage(lambda l: ops.rpn_topk_wide(heads[l], A, ks[l], vals[:, sl[l]], idx[:, sl[l]]), wide))
        row(f"  afi_rpn_decode, {len(ks)} levels", stage(lambda l: ops.rpn_decode(heads[l], A, A, ag.cell_anchors[l], ag.strides[l], idx[:, sl[l]], ks[l], hw,
                                                                                  m.box_weights, SCALE_CLAMP, m.min_box_side_len, boxes[:, sl[l]], valid[:, sl[l]]),
                                                         range(len(ks))))
        row(f"  afi_rpn_nms_wide, {len(wide)} levels", stage(lambda l: ops.rpn_nms_wide(boxes[:, sl[l]], valid[:, sl[l]], m.nms_thresh, keep[:, sl[l]]), wide))
        row(f"  afi_rpn_topk + afi_rpn_nms, {len(narrow)} narrow", stage(lambda l: (ops.rpn_topk(heads[l], A, ks[l], vals[:, sl[l]], idx[:, sl[l]]),
                                                                                     ops.rpn_nms(boxes[:, sl[l]], valid[:, sl[l]], m.nms_thresh, keep[:, sl[l]])),
                                                                        narrow))
        row("  afi_rpn_merge_wide", lambda: ops.rpn_merge_wide(boxes, vals, keep, off, POST_K))
        row("selection 1000 / 1000 HIP (narrow kernels)", lambda: m.select(heads, hw, 1000, 1000))
        if not args.no_torch:
            row(f"selection {PRE_K} / {POST_K} torch eager", lambda: torch_select(m, heads, hw, PRE_K, POST_K))
            print(f"proposals per image: HIP {r['counts'].tolist()}, torch {[len(v) for _, v in torch_select(m, heads, hw, PRE_K, POST_K)]}", flush=True)
        # the two NMS forms on the same lists: the first 1000 boxes of each level's list (a prefix of a sorted list is a sorted list)
        for l in wide:
            b, v = boxes[:, sl[l]][:, :1000].contiguous(), valid[:, sl[l]][:, :1000].contiguous()
            same = torch.equal(ops.rpn_nms_wide(b, v, m.nms_thresh), ops.rpn_nms(b, v, m.nms_thresh))
            row(f"k = 1000, {LEVELS[l]}: afi_rpn_nms (LDS)", lambda: ops.rpn_nms(b, v, m.nms_thresh))
            row(f"k = 1000, {LEVELS[l]}: afi_rpn_nms_wide (same keep: {same})", lambda: ops.rpn_nms_wide(b, v, m.nms_thresh))
    print(json.dumps({"shape": args.shape, "rounds": args.rounds, "pre_k": PRE_K, "post_k": POST_K, "median_min_max_ms": out}))


if __name__ == "__main__":
    main()
