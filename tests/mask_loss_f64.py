"""The plain-loop checker of the training side of the mask branch of StandardROIHeads (afigan_amd/roi_heads.py: _ROIMaskLossFn;
csrc/mask_loss.hip): detectron2 v0.1.1's mask_rcnn_loss restated -- the targets of PolygonMasks.crop_and_resize /
rasterize_polygons_within_box on poly_f64.ann_mask with the transformed vertices formed in numpy by the restated steps, the binary
cross-entropy with logits and its gradient in float64, the backward of the class-selected predictor, and a torch restatement of the mask
pooler, the head and the loss for autograd in any dtype.

Also here, because the host test and the GPU test share them: the target, loss and end-to-end cases."""
import math

import numpy as np

import mask_f64
import poly_f64
import roi_loss_f64 as T

F = np.float32
EPS = 2.0 ** -24
N, P, B, BF = T.N, T.P, T.B, 8                           # Bf = int(32 * 0.25)


# ------------------------------------------------------------------------------------------------ targets
def ratio(side, M, variant="numpy"):
    """M / max(side, 0.1) for a numpy.float32 side.  "numpy": as detectron2 evaluates it -- Python's max returns the float32 side unless
    0.1 > side (a NaN side stays), and an int divided by a float32 is the float32 quotient; the float64 quotient otherwise.  "fp64": the
    quotient in float64 always (what the kernel must NOT compute)."""
    side = F(side)
    with np.errstate(all="ignore"):
        if variant == "fp64":
            return float(M) / (float(side) if not float(side) < 0.1 else 0.1)
        if not float(side) < 0.1:
            return float(F(M) / side)
        return float(M) / 0.1


def transformed(polys, box, M, variant="numpy"):
    """The polygons of one instance in the M x M frame of the fp32 box: X = (x - x0) rw, Y = (y - y0) rh, one float64 subtraction and one
    float64 product each."""
    b = np.asarray(box, F)
    with np.errstate(all="ignore"):
        w, h = F(b[2] - b[0]), F(b[3] - b[1])
    rw, rh, x0, y0 = ratio(w, M, variant), ratio(h, M, variant), float(b[0]), float(b[1])
    out = []
    for p in polys:
        c = np.asarray(p, np.float64).reshape(-1)
        t = np.empty_like(c)
        with np.errstate(all="ignore"):
            t[0::2] = (c[0::2] - x0) * rw
            t[1::2] = (c[1::2] - y0) * rh
        out.append(t)
    return out


def row_target(polys, box, M, variant="numpy"):
    """The bool [M, M] target of one row: the union of the instance's transformed polygons (poly_f64.ann_mask: section 20's steps 1-5); all
    zero when a transformed coordinate is not finite or has |5 c + .5| >= 2^30; empty for an instance without polygons."""
    tp = transformed(polys, box, M, variant)
    for t in tp:
        with np.errstate(all="ignore"):
            if not (np.abs(5.0 * t + 0.5) < float(1 << 30)).all():
                return np.zeros((M, M), bool)
    return poly_f64.ann_mask([t.tolist() for t in tp if t.size], M, M)


def targets(instances, boxes, sidx, midx, n_pos, counts_g, Bf, M, variant="numpy"):
    """(targets uint8 [N, Bf, M, M], counts_fg [N]) of a training list: row j of image n is live when j < clamp(n_pos[n], 0, Bf), its
    sampled index lies inside matched_idx's row and the image has instances; its instance is matched_idx[n][sampled_idx[n][j]] clamped."""
    n_img, R = len(instances), midx.shape[1]
    out, cfg = np.zeros((n_img, Bf, M, M), np.uint8), np.zeros(n_img, np.int32)
    for n in range(n_img):
        cfg[n] = min(max(int(n_pos[n]), 0), Bf)
        G = int(counts_g[n])
        for j in range(cfg[n]):
            i = int(sidx[n, j])
            if G <= 0 or not 0 <= i < R:
                continue
            g = min(max(int(midx[n, i]), 0), G - 1)
            out[n, j] = row_target(instances[n][g], boxes[n, j], M, variant)
    return out, cfg


def _ngon(cx, cy, rx, ry, k, phase=0.1):
    a = phase + 2 * math.pi * np.arange(k) / k
    return np.stack([cx + rx * np.cos(a), cy + ry * np.sin(a)], 1).reshape(-1).tolist()


def bbox_of(polys):
    c = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in polys])
    return np.array([c[:, 0].min(), c[:, 1].min(), c[:, 0].max(), c[:, 1].max()], F)


def split_polygon(M, w, x0=10.0, y0=20.0, h=9.0):
    """A rectangle and an fp32 box of width w (M / w differs between float32 and float64 rounding) whose left edge sits where the two
    quotients upsample it to different columns: (polys, box); the caller proves that the two variants rasterise it differently."""
    r32, r64 = ratio(F(w), M), ratio(F(w), M, "fp64")
    assert r32 != r64, (M, w)
    lo, hi = min(r32, r64), max(r32, r64)
    for k in range(3, 5 * M - 5, 5):                    # the left edge's column moves between k - 1 = 5 q + 2 and k
        thr = (k - 0.5) / 5.0
        x = x0 + thr * 2.0 / (lo + hi)
        d = x - x0
        if d * hi >= thr > d * lo and 0.3 * w < d < 0.7 * w:
            return [[x, y0 + 1.0, x0 + w, y0 + 1.0, x0 + w, y0 + h - 1.0, x, y0 + h - 1.0]], np.array([x0, y0, x0 + w, y0 + h], F)
    raise AssertionError("no splitting column found")


SPLIT_W = {28: 3.0, 6: 7.0}                             # 28 / 3 and 6 / 7 round differently in float32 and float64 (6 / 3 does not)


def target_case(M):
    """A training list built by hand (afi_mask_targets reads the list, not the sampler): image 0 has five instances and one row of every
    kind, image 1 two instances.  Returns dict(instances, boxes [N, B, 4], sidx [N, B], midx [N, R], counts_g, kinds = image 0's row names)."""
    inst0 = [
        [_ngon(50.0, 60.0, 30.0, 22.0, 8)],                                                                    # 0: one octagon, wider than high
        [_ngon(110.0, 40.0, 20.0, 20.0, 12), _ngon(112.0, 42.0, 8.0, 7.0, 6), _ngon(128.0, 52.0, 9.0, 12.0, 5)],   # 1: three polygons, one inside another
        [_ngon(20.0, 110.0, 6.0, 5.0, 7)],                                                                     # 2: far from its row's box
        [_ngon(90.0, 100.0, 14.0, 14.0, 3, 0.7)],                                                              # 3: a triangle
        [],                                                                                                    # 4: no polygon
    ]
    sp, spbox = split_polygon(M, SPLIT_W[M])
    inst0.append(sp)                                                                                           # 5: the float32 / float64 splitter
    inst1 = [[_ngon(40.0, 40.0, 25.0, 18.0, 20, 0.3)], [_ngon(100.0, 80.0, 12.0, 30.0, 9), _ngon(100.0, 80.0, 30.0, 6.0, 4, 0.0)]]
    b0, b1 = bbox_of(inst0[0]), bbox_of(inst0[1])
    half = b0.copy()
    half[[0, 2]] += F(0.5) * (b0[2] - b0[0])
    rows0 = [("own_box", b0, 0), ("half_outside", half, 0), ("three_polygons", b1, 1), ("polygon_outside_box", np.array([100, 10, 140, 50], F), 2),
             ("side_below_0.1", np.array([40.0, 30.0, 40.05, 75.0], F), 0), ("zero_area", np.array([50, 60, 50, 60], F), 0),
             ("square_box", np.array([76, 86, 104, 114], F), 3), ("split_quotient", spbox, 5)]
    rows1 = [("own_box", bbox_of(inst1[0]), 0), ("cross", bbox_of(inst1[1]), 1), ("cross_shifted", bbox_of(inst1[1]) + F(7.25), 1),
             ("no_polygon_of_other_image", b0, 0)] + [("again%d" % k, bbox_of(inst1[k % 2]) + F(k), k % 2) for k in range(4)]
    G = len(inst0)
    R = P + G
    boxes = np.zeros((N, B, 4), F)
    sidx, midx = np.full((N, B), -1, np.int32), np.full((N, R), 10 ** 6, np.int32)       # unsampled entries must never be looked at
    rng = np.random.default_rng(5)
    for n, rows in enumerate((rows0, rows1)):
        slots = rng.permutation(R)[:B]
        for j, (_, bx, g) in enumerate(rows):
            boxes[n, j], sidx[n, j], midx[n, slots[j]] = bx, slots[j], g
        for j in range(len(rows), B):                                                    # background rows behind them: boxes, matched to slot 0
            boxes[n, j], sidx[n, j], midx[n, slots[j]] = np.array([5, 5, 60, 70], F) + F(j), slots[j], 0
    return dict(instances=[inst0, inst1], boxes=boxes, sidx=sidx, midx=midx, counts_g=np.array([G, len(inst1)], np.int32), Gmax=G,
                kinds=[k for k, _, _ in rows0])


N_POS_CASES = {"all": (BF, BF), "none": (0, 0), "between": (5, 3), "above_and_below": (BF + 4, -2)}


# ------------------------------------------------------------------------------------------------ loss, dz, the predictor's backward
def image_order(dz):
    """[R, S, S, 4] in h's pixel order (y, x, phase 2a + b) -> [R, 2S, 2S]: output pixel (2y + a, 2x + b)."""
    R, S = dz.shape[:2]
    return dz.reshape(R, S, S, 2, 2).transpose(0, 1, 3, 2, 4).reshape(R, 2 * S, 2 * S)


def mask_loss(h, w, b, classes, counts, tg):
    """h [N D, 4 C, S, S] fp32, w [Km, C], b [Km], classes [N, D], counts [N], tg [N, D, 2S, 2S] 0 / 1.  Returns dict(loss, dz [N D, 2S, 2S]
    in image order, ez = section 16's logit bar (C + 6) 2^-24 (sum |w h| + |b|) per pixel (zero on rows that are not live), absterm, mtot)."""
    z, mag, live = mask_f64.selected_logits(h, w, b, classes, counts)
    C = np.asarray(w).reshape(len(b), -1).shape[1]
    t = np.asarray(tg, np.float64).reshape(z.shape)
    M2 = z.shape[1] * z.shape[2]
    mtot = M2 * int(sum(min(max(int(c), 0), np.asarray(classes).shape[1]) for c in counts))
    lv = live[:, None, None]
    term = np.where(lv, np.maximum(z, 0.0) - z * t + np.log1p(np.exp(-np.abs(z))), 0.0)
    ez = np.where(lv, (C + 6) * EPS * mag, 0.0)
    if mtot == 0:
        return dict(loss=0.0, dz=np.zeros_like(z), ez=ez, absterm=0.0, mtot=0, z=z, live=live)
    return dict(loss=term.sum() / mtot, dz=np.where(lv, (mask_f64.sigmoid(z) - t) / mtot, 0.0), ez=ez, absterm=np.abs(term).sum(), mtot=mtot,
                z=z, live=live)


def pred_bwd(h, dz, w, classes, counts):
    """h [R, 4 C, S, S], dz [R, S, S, 4] (the kernel's order), w [Km, C].  Returns dict(dh [R, 4 C, S, S], dh_mag = |dz w|, dW [Km, C], dW_abs
    = sum |dz h|, db [Km], db_abs = sum |dz|, terms [Km] = the number of added terms of a class: its live rows times 4 S S), float64."""
    h = np.asarray(h, np.float64)
    dz = np.asarray(dz, np.float64)
    w = np.asarray(w, np.float64)
    Km, C = w.shape
    R, _, S, _ = h.shape
    D = np.asarray(classes).shape[1]
    dh, mag = np.zeros(h.shape), np.zeros(h.shape)
    dW, aW, db, ab, terms = np.zeros((Km, C)), np.zeros((Km, C)), np.zeros(Km), np.zeros(Km), np.zeros(Km, np.int64)
    for r in range(R):
        n, d = divmod(r, D)
        c = 0 if Km == 1 else int(classes[n][d])
        if d >= min(max(int(counts[n]), 0), D) or not 0 <= c < Km:
            continue
        terms[c] += 4 * S * S
        for ph in range(4):
            g = dz[r, :, :, ph]                                                 # [S, S]
            hp = h[r, ph * C:(ph + 1) * C]                                      # [C, S, S]
            dh[r, ph * C:(ph + 1) * C] = g[None] * w[c][:, None, None] * (hp > 0)
            mag[r, ph * C:(ph + 1) * C] = np.abs(g[None] * w[c][:, None, None])
            dW[c] += (g[None] * hp).sum((1, 2))
            aW[c] += np.abs(g[None] * hp).sum((1, 2))
            db[c] += g.sum()
            ab[c] += np.abs(g).sum()
    return dict(dh=dh, dh_mag=mag, dW=dW, dW_abs=aW, db=db, db_abs=ab, terms=terms)


LOSS_CASES = {"C8_S14_K80": (8, 14, 80, {}), "C256_S14_K3": (256, 14, 3, {}), "C8_S3_K1": (8, 3, 1, {}), "C256_S3_K80": (256, 3, 80, {}),
              "C12_S5_K3": (12, 5, 3, {}), "mtot_zero": (8, 14, 3, {"empty": True}), "logits_of_40": (8, 3, 3, {"big": True})}


def loss_case(C, S, Km, empty=False, big=False, seed=11):
    """(h [N Bf, 4 C, S, S] fp32 >= 0, w [Km, C], b [Km], classes [N, B] int32 -- the training list's classes, read with their row stride;
    background K and padding -1 behind the foreground rows --, counts_fg [N], targets uint8 [N, Bf, 2S, 2S])."""
    rng = np.random.default_rng(seed + C + 31 * S + 977 * Km)
    h = np.maximum(rng.standard_normal((N * BF, 4 * C, S, S)), 0).astype(F)
    w = (rng.standard_normal((Km, C)) * (3.0 / np.sqrt(C))).astype(F)
    b = (rng.standard_normal(Km) * 0.5).astype(F)
    if big:                                              # |z| around 40: exp(z) overflows nothing in the stable form, 1 - sigmoid underflows to 0 in fp32
        w *= F(25.0)
        b[:] = [40.0, -40.0, 3.0][:Km]
    cls = np.full((N, B), -1, np.int32)
    counts = np.array([0, 0] if empty else [5, BF], np.int32)
    for n in range(N):
        cls[n, :BF + 6] = Km if Km > 1 else 1            # what the list holds behind the positives: the background class
        cls[n, :BF] = rng.integers(0, Km, BF)
        cls[n, 0], cls[n, 1] = 0, Km - 1
    tg = (rng.random((N, BF, 2 * S, 2 * S)) < 0.45).astype(np.uint8)
    return h, w, b, cls, counts, tg


# ------------------------------------------------------------------------------------------------ the end-to-end case and its restatement
def e2e_polygons(case):
    """One ten-gon per ground-truth box of roi_loss_f64.e2e_case, inscribed in 90 % of the box: the instances of every image."""
    out = []
    for g in case["gts"]:
        g = np.asarray(g, np.float64)
        out.append([[_ngon((b[0] + b[2]) / 2, (b[1] + b[3]) / 2, 0.45 * (b[2] - b[0]), 0.45 * (b[3] - b[1]), 10, 0.2)] for b in g])
    return out


FEATURES = ["p2", "p3", "p4", "p5"]
# The feature seed of each end-to-end fixture.  The gradient comparison is only meaningful where every ReLU unit's sign is decided at fp32
# resolution (torch_mask_loss' margins > 1: tests/test_mask_loss_host.py proves it on the CPU); of the 2.4 M units of the 128-channel chain
# one in about three seeds holds a unit closer to zero than that -- at 128 channels seed 2 holds a deconv pre-activation of 7e-8 among summands of order 1 --
# so the seed is chosen by that CPU condition alone.
E2E_SEEDS = {8: 2, 128: 7}


def e2e_heads(amd, channels, fc_dim=32, K=5, num_conv=2, agnostic=False):
    """StandardROIHeads with the mask branch (on the CPU: the caller moves them): NUM_CONV convs of `channels` channels, mask pooler 14,
    sampling ratio 2; parameters drawn large enough that logits and deltas are not all near zero."""
    import torch
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": True, "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": FEATURES, "NUM_CLASSES": K,
                                                              "BATCH_SIZE_PER_IMAGE": B},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "FC_DIM": fc_dim, "POOLER_RESOLUTION": 7,
                                                "POOLER_SAMPLING_RATIO": 2},
                               "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": num_conv, "CONV_DIM": channels, "POOLER_RESOLUTION": 14,
                                                 "POOLER_SAMPLING_RATIO": 2, "CLS_AGNOSTIC_MASK": agnostic}})
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=2 ** int(f[1:])) for f in FEATURES}, masks=True)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                                    # detectron2's std 0.001 for the predictor would leave every logit near 0
        for k, p in h.named_parameters():
            fan = p[0].numel() if "deconv" not in k else p.shape[0]
            std = 0.2 if k.endswith("bias") else (2.0 / fan) ** 0.5 * (3.0 if "predictor" in k else 1.0)
            p.copy_(torch.randn(p.shape, generator=g) * std)
    return h


def e2e_features(channels, seed=None):
    import torch
    g = torch.Generator().manual_seed(E2E_SEEDS.get(channels, 2) if seed is None else seed)
    return {f: torch.randn((N, channels, H, W), generator=g) for f, (H, W) in zip(FEATURES, T.LEVELS)}


def torch_mask_loss(xs, params, min_level, S, sampling_ratio, boxes, counts, cls, tg, Km, margins=None):
    """The mask pooler (ROIAlign as the two axis-weight matrices of every box), ``mask_fcn`` convs with ReLU, the deconv with ReLU, the
    predictor and F.binary_cross_entropy_with_logits(reduction="mean") on the rows' own classes, in torch, in the dtype of `xs`;
    differentiable in xs [N, C, H_l, W_l] and params = [mask_fcn1.weight, .bias, ..., deconv.weight, .bias, predictor.weight, .bias].  boxes
    [N, Bf, 4], counts [N], cls [N, >= Bf], tg [N, Bf, 2S, 2S]: the foreground list and its targets are given.  margins: a list that receives,
    per ReLU layer, the smallest |pre-activation| / (2^-24 (sum |w x| + |b|)) of its units: below 1 a unit's sign is not decided at fp32
    resolution -- one rounding of its largest partial sum can flip it -- and a gradient comparison would measure that flip."""
    import torch
    import torch.nn.functional as Fn
    dt = xs[0].dtype
    live = {(n, j): (bx, level) for n, j, bx, level in T._live_boxes(boxes, counts, min_level, len(xs))}
    C = xs[0].shape[1]
    rows, meta = [], []
    for n in range(boxes.shape[0]):
        for j in range(int(counts[n])):
            if (n, j) in live:
                bx, level = live[(n, j)]
                f = xs[level - min_level][n]
                Wy, Wx, gh, gw = T._box_tables(bx, level, S, sampling_ratio, f.shape[1], f.shape[2])
                rows.append(torch.einsum("ph,chw,qw->cpq", torch.tensor(Wy, dtype=dt), f, torch.tensor(Wx, dtype=dt)) / max(gh * gw, 1))
            else:
                rows.append(torch.zeros((C, S, S), dtype=dt))
            meta.append((n, j))
    if not rows:
        return sum(x.sum() for x in xs) * 0
    x = torch.stack(rows)
    nconv = (len(params) - 4) // 2

    def relu(v, mag):
        if margins is not None:
            with torch.no_grad():
                margins.append((v.abs() / (EPS * mag())).min().item())
        return torch.relu(v)
    for k in range(nconv):
        w, b = params[2 * k], params[2 * k + 1]
        x = relu(Fn.conv2d(x, w, b, padding=1), lambda: Fn.conv2d(x.abs(), w.abs(), b.abs(), padding=1))
    w, b = params[-4], params[-3]
    x = relu(Fn.conv_transpose2d(x, w, b, stride=2), lambda: Fn.conv_transpose2d(x.abs(), w.abs(), b.abs(), stride=2))
    logits = Fn.conv2d(x, params[-2], params[-1])
    sel = torch.stack([logits[i, 0 if Km == 1 else int(cls[n, j])] for i, (n, j) in enumerate(meta)])
    t = torch.tensor(np.stack([tg[n, j] for n, j in meta]).astype(np.float64), dtype=dt)
    return Fn.binary_cross_entropy_with_logits(sel, t, reduction="mean")
