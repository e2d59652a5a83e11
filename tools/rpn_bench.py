"""Forward time of the frozen RPN proposal generator (afigan_amd/rpn.py) at the inference configs' settings (A = 3, PRE / POST_NMS_TOPK_TEST 1000,
NMS_THRESH 0.7, five levels), head and selection separately, each next to a torch-eager baseline on the same GPU with the same weights:
median (min / max) of CUDA-event-timed forwards after warm-up.  Prints one line per part and shape, and a JSON summary line.

    python tools/rpn_bench.py --shapes 2x800x1344 2x400x672 --rounds 9 [--trace-only]

Baselines (torch alone: there is no torchvision here):
  head       F.conv2d (3x3 + ReLU, then the two 1x1 convs) on NCHW tensors -- MIOpen;
  selection  per level torch.topk(sorted=True) + gather + the decode as elementwise torch ops, then the best NMS torch alone offers: the IoU
             matrix of each (image, level) list on the device and the greedy sweep over it 64 rows at a time -- the 64 x 64 diagonal block
             is resolved on the host (one device-to-host copy per chunk), the kept rows' suppression OR-ed on the device; then cat + sort.
             (A sweep of one device op per row takes ~1000 dependent launches per list and is slower still.)
--trace-only: one warm-up and three timed forward_padded calls at the first shape, nothing else (for a rocprofv3 kernel trace)."""
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
CLAMP = math.log(1000.0 / 16)


def _time(fn, rounds, warmup=2):
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
                               "RPN": {"IN_FEATURES": LEVELS, "PRE_NMS_TOPK_TEST": 1000, "POST_NMS_TOPK_TEST": 1000, "NMS_THRESH": 0.7}})
    m = amd.RPN(cfg, {f: ShapeSpec(channels=channels, stride=4 * 2 ** i) for i, f in enumerate(LEVELS)})
    g = torch.Generator().manual_seed(0)
    for name, s in (("conv", 1.0 / math.sqrt(9 * channels)), ("objectness_logits", 1.0 / math.sqrt(channels)), ("anchor_deltas", 0.6 / math.sqrt(channels))):
        layer = getattr(m.rpn_head, name)
        layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * s)
        layer.bias.copy_(torch.randn(layer.bias.shape, generator=g) * 0.1)
    return m.cuda().eval()


def torch_head(m, xs):
    h = m.rpn_head
    out = []
    for x in xs:
        t = F.relu(F.conv2d(x, h.conv.weight, h.conv.bias, padding=1))
        out.append((F.conv2d(t, h.objectness_logits.weight, h.objectness_logits.bias), F.conv2d(t, h.anchor_deltas.weight, h.anchor_deltas.bias)))
    return out


def torch_nms(boxes, thresh):
    """Greedy NMS of boxes [k, 4] in list order with torch alone: keep mask [k] (see the module docstring for the form)."""
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


def torch_select(m, heads, image_hw):
    A, res = m.num_anchors, []
    N = heads[0][0].shape[0]
    wx, wy, ww, wh = m.box_weights
    for n in range(N):
        bs, ls = [], []
        for l, (lg, dl) in enumerate(heads):
            H, W = lg.shape[2:]
            flat = lg[n].permute(1, 2, 0).reshape(-1)
            k = min(m.pre_nms_topk, flat.numel())
            v, i = torch.topk(flat, k, sorted=True)
            d = dl[n].reshape(A, 4, H, W).permute(2, 3, 0, 1).reshape(-1, 4)[i]
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
        o = torch.sort(v, descending=True, stable=True).indices[:m.post_nms_topk]
        res.append((b[o], v[o]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["2x800x1344", "2x400x672"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    results = {}
    with torch.no_grad():
        m = build()
        for s in args.shapes:
            N, H, W = (int(v) for v in s.split("x"))
            g = torch.Generator().manual_seed(1)
            xs = [torch.randn((N, 256, -(-H // (4 * 2 ** i)), -(-W // (4 * 2 ** i))), generator=g).cuda() for i in range(5)]
            feats = {f: x.contiguous(memory_format=torch.channels_last) for f, x in zip(LEVELS, xs)}
            hw = torch.tensor([[H, W]] * N, dtype=torch.float32, device="cuda")
            if args.trace_only:
                _time(lambda: m.forward_padded(hw, feats), 3, warmup=1)
                print(f"[trace] RPN {s}: 1 warm-up + 3 forward_padded", flush=True)
                return
            heads = m.head(feats)
            theads = torch_head(m, xs)
            parts = {"head HIP": lambda: m.head(feats), "head torch": lambda: torch_head(m, xs),
                     "selection HIP": lambda: m.select(heads, hw), "selection torch": lambda: torch_select(m, theads, hw),
                     "forward_padded HIP": lambda: m.forward_padded(hw, feats)}
            r = {}
            for name, fn in parts.items():
                ts = _time(fn, args.rounds)
                r[name] = statistics.median(ts)
                print(f"{name:20s} {s:>12s}: median {r[name]:8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  ({len(ts)} rounds)", flush=True)
            # the two selections agree on how many proposals there are (boxes may differ where rounding moves one across a cut)
            c = m.select(heads, hw)["counts"].tolist()
            ct = [len(v) for _, v in torch_select(m, theads, hw)]
            print(f"proposals per image: HIP {c}, torch {ct}", flush=True)
            r["selection_share_of_forward"] = r["selection HIP"] / r["forward_padded HIP"]
            results[s] = r
    print(json.dumps({"rounds": args.rounds, "median_ms": results, "baseline": "F.conv2d head; torch.topk + IoU matrix on the device + 64-row sweep"}))


if __name__ == "__main__":
    main()
