"""fp64 restatement of the RPN proposal generator's inference path (detectron2 v0.1.1 semantics, afigan_amd/rpn.py's docstring), the checker of
tests/test_gpu_rpn.py and tests/test_rpn_host.py: plain numpy / torch on the CPU, written from the semantics, stage by stage so that a
test can feed each stage the KERNEL's previous output (no rounding difference then leaks into a discrete decision).

Also the generator of the NMS tests' inputs (``nms_case``) with the two conditions the tests assert on them (``nms_case_facts``)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

SCALE_CLAMP = math.log(1000.0 / 16)


def cell_anchors(sizes, ratios):
    """[len(sizes) len(ratios), 4] fp64: (-w/2, -h/2, w/2, h/2), w = sqrt(size^2 / ratio), h = ratio w; sizes, then ratios."""
    out = []
    for s in sizes:
        for r in ratios:
            w = math.sqrt(s * s / r)
            out.append((-w / 2, -r * w / 2, w / 2, r * w / 2))
    return np.array(out, dtype=np.float64)


def topk(logits, k):
    """Indices of the k highest of a 1-D fp32 array: descending, equal values (-0 = +0) in ascending index, NaN below every number."""
    x = np.asarray(logits, dtype=np.float32)
    return np.argsort(-x, kind="stable")[:k].astype(np.int32)          # numpy sorts NaN last; stable keeps index order among equals


def decode(deltas, idx, cell, stride, W, A, weights, image_hw, min_size, clamp=SCALE_CLAMP):
    """deltas [k, 4] (the fp32 deltas of the selected anchors), idx [k]: boxes [k, 4] fp64 clipped to image_hw = (h, w), valid [k],
    and the un-clipped centres / sizes (pcx, pcy, pw, ph) the error bound is stated in."""
    d = np.asarray(deltas, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    cell = np.asarray(cell, dtype=np.float64)
    a, pix = idx % A, idx // A
    x, y = pix % W, pix // W
    shift = np.stack([x * stride, y * stride, x * stride, y * stride], 1).astype(np.float64)
    an = cell[a] + shift
    w, h = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
    cx, cy = an[:, 0] + w / 2, an[:, 1] + h / 2
    wx, wy, ww, wh = weights
    dx, dy = d[:, 0] / wx, d[:, 1] / wy
    dw, dh = np.minimum(d[:, 2] / ww, clamp), np.minimum(d[:, 3] / wh, clamp)
    pcx, pcy, pw, ph = dx * w + cx, dy * h + cy, np.exp(dw) * w, np.exp(dh) * h
    b = np.stack([pcx - pw / 2, pcy - ph / 2, pcx + pw / 2, pcy + ph / 2], 1)
    ih, iw = image_hw
    b[:, 0::2] = b[:, 0::2].clip(0, iw)
    b[:, 1::2] = b[:, 1::2].clip(0, ih)
    valid = ((b[:, 2] - b[:, 0]) > min_size) & ((b[:, 3] - b[:, 1]) > min_size)
    return b, valid, (pcx, pcy, pw, ph)


def iou_matrix(b):
    b = np.asarray(b, dtype=np.float64)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = np.maximum(b[:, None, :2], b[None, :, :2])
    rb = np.minimum(b[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clip(0)
    inter = wh[..., 0] * wh[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area[:, None] + area[None] - inter)


def overlaps32(b, thresh):
    """inter / (area_a + area_b - inter) > thresh evaluated in fp32, operation by operation in that form (no fused multiply-add): the
    statement the NMS kernel is compiled to."""
    b = np.asarray(b, dtype=np.float32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), np.float32(0))
    ih = np.maximum(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), np.float32(0))
    inter = iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / ((area[:, None] + area[None, :]) - inter) > np.float32(thresh)


def nms(boxes, valid, thresh, rounding_pairs_in_fp32=False):
    """Greedy NMS in list order: keep [k] bool.  A box that is not valid is neither kept nor suppresses.  rounding_pairs_in_fp32: a pair
    whose fp64 IoU lies within 1e-5 of thresh -- which the fp32 evaluation decides by rounding -- is decided as overlaps32 decides it (for
    boxes that a kernel produced, where no seed can be chosen to avoid such pairs); every other pair by the fp64 value."""
    n = len(boxes)
    keep = np.zeros(n, dtype=bool)
    if n == 0:
        return keep
    I = iou_matrix(boxes)
    over = I > thresh
    if rounding_pairs_in_fp32:
        near = np.abs(I - thresh) < 1e-5
        if near.any():
            over = np.where(near, overlaps32(boxes, thresh), over)
    sup = ~np.asarray(valid, dtype=bool)
    later = np.arange(n)
    for i in range(n):
        if sup[i]:
            continue
        keep[i] = True
        sup |= over[i] & (later > i)
    return keep


def merge(vals, keep, level_off, post_k):
    """Concatenated positions of the kept entries by (logit descending, level, rank) -- a stable sort over the levels side by side -- cut to post_k."""
    pos = np.nonzero(np.asarray(keep, dtype=bool))[0]
    order = np.argsort(-np.asarray(vals, dtype=np.float32)[pos], kind="stable")
    return pos[order][:post_k]


def head(x, params, dtype=torch.float64):
    """StandardRPNHead on one level: (logits [N, A, H, W], deltas [N, 4A, H, W]) in `dtype` on the CPU."""
    p = {k: v.detach().cpu().to(dtype) for k, v in params.items()}
    t = F.relu(F.conv2d(x.detach().cpu().to(dtype), p["conv.weight"], p["conv.bias"], padding=1))
    return (F.conv2d(t, p["objectness_logits.weight"], p["objectness_logits.bias"]),
            F.conv2d(t, p["anchor_deltas.weight"], p["anchor_deltas.bias"]))


# ------------------------------------------------------------------------------------------------ NMS test inputs
NMS_SIZES = (1000, 333, 64, 1, 0)
NMS_SEEDS = (3, 6)                    # one per image of the batch; both meet the conditions below at every size and threshold
NMS_THRESHOLDS = (0.7, 0.5)
NMS_IMAGE = (800, 1344)


def nms_case(seed, n, img=NMS_IMAGE):
    """n clustered boxes (fp32, inside an img[0] x img[1] image, non-empty), in the order of a random score, descending."""
    r = np.random.RandomState(seed)
    if n == 0:
        return np.zeros((0, 4), np.float32), np.zeros((0,), np.float32)
    nc = max(4, n // 12)
    c = r.rand(nc, 2) * [img[1], img[0]]
    s = np.exp(r.uniform(np.log(16), np.log(400), nc))
    k = r.randint(0, nc, n)
    ctr = c[k] + r.randn(n, 2) * s[k, None] * 0.15
    wh = s[k, None] * np.exp(r.randn(n, 2) * 0.25)
    b = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)
    b[:, 0::2] = b[:, 0::2].clip(0, img[1])
    b[:, 1::2] = b[:, 1::2].clip(0, img[0])
    b = b.astype(np.float32)
    sc = r.randn(n).astype(np.float32)
    o = np.argsort(-sc, kind="stable")
    return b[o], sc[o]


def nms_case_facts(boxes, thresh):
    """(all boxes non-empty, pairs whose fp64 IoU lies within 1e-5 of thresh, fraction kept by the fp64 greedy NMS)."""
    n = len(boxes)
    b = boxes.astype(np.float64)
    nonempty = bool((((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)).all())
    I = iou_matrix(b)
    iu = np.triu_indices(n, 1)
    ambiguous = int((np.abs(I[iu] - thresh) < 1e-5).sum())
    kept = int(nms(b, np.ones(n, bool), thresh).sum())
    return nonempty, ambiguous, kept / max(n, 1)
