"""The plain checker of CascadeROIHeads' training passes (csrc/cascade_train.hip), shared by tests/test_cascade_train_host.py and
tests/test_gpu_cascade_train.py.  Restated from detectron2 v0.1.1's rules (cascade_rcnn.py: _create_proposals_from_boxes,
_match_and_label_boxes) and torch.nn.BatchNorm2d's; NOT run against detectron2, which is not a dependency.

  relabel        the keep rule Boxes.nonempty() in numpy.float32 and the matching roi_loss_f64.label (rpn_loss_f64.iou32, numpy.float32 in
                 the stated order) on decoded fp32 boxes: given the boxes, everything compares for EQUALITY.  The decode itself is
                 roi_f64.scores_boxes (fp64, rounded once), which the kernels meet to a few ulp: the GPU test takes afi_roi_cascade_stage's
                 boxes, which the relabel kernel must reproduce bit for bit.
  masked BN      the valid rows (j < counts[n]) of x [N B, P1, C] are taken out by index selection and handed to elementwise_f64's float64
                 references (bn_stats, bn_apply, bn_bwd_sums, bn_bwd_dx) as one dense [Pn, C] matrix; results are scattered back, padding
                 rows zero.  The ReLU mask of the backward is the STORED y's, as the kernels take it.
Also the seeded inputs of both test files."""
import math

import numpy as np
import torch

import cascade_f64 as QC
import elementwise_f64 as E
import roi_f64 as QB
import roi_loss_f64 as RL

F = np.float32


# ------------------------------------------------------------------------------------------------ relabel
def decode(pred, K, proposals, counts, image_hw, weights):
    """afi_roi_cascade_stage's boxes [N, B, 4] from the float64 restatement (roi_f64.scores_boxes), rounded once to fp32.  The kernel's own
    boxes agree with these to a few ulp (tests/test_gpu_cascade.py's bar), not bit for bit: a GPU test hands ``relabel_boxes`` the KERNEL's."""
    pr = np.asarray(proposals, F)
    B = pr.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        _, bx, _ = QB.scores_boxes(pred, K, True, pr, [min(max(int(c), 0), B) for c in counts], image_hw, weights)
        return bx[:, :, 0].astype(F)


def relabel_boxes(b32, K, counts, gt, gt_classes, counts_g, thresh):
    """The relabel rule on decoded and clipped fp32 boxes b32 [N, B, 4] (rows below counts): dict of boxes [N, B, 4] fp32, counts [N],
    gt_classes [N, B] int32, gt_boxes [N, B, 4] fp32, src [N, B] int32, matched_idx [N, B] int32: afi_roi_cascade_relabel's outputs."""
    b32 = np.asarray(b32, F)
    N, B = b32.shape[:2]
    out = {"boxes": np.zeros((N, B, 4), F), "counts": np.zeros(N, np.int32), "gt_classes": np.full((N, B), -1, np.int32),
           "gt_boxes": np.zeros((N, B, 4), F), "src": np.full((N, B), -1, np.int32), "matched_idx": np.zeros((N, B), np.int32)}
    for n in range(N):
        G = min(max(int(counts_g[n]), 0), gt.shape[1])
        g = np.asarray(gt[n, :G], F)
        with np.errstate(invalid="ignore"):
            kept = [j for j in range(min(max(int(counts[n]), 0), B))
                    if (b32[n, j, 2] - b32[n, j, 0] > F(0)) and (b32[n, j, 3] - b32[n, j, 1] > F(0))]
        kb = b32[n, kept].reshape(-1, 4)
        labels, midx = RL.label(kb, len(kept), g, len(kept), thresh, append_gt=False)
        out["counts"][n] = len(kept)
        for i, j in enumerate(kept):
            out["boxes"][n, i], out["src"][n, i], out["matched_idx"][n, i] = kb[i], j, midx[i]
            out["gt_classes"][n, i] = gt_classes[n, midx[i]] if labels[i] == 1 else K
            if G:
                out["gt_boxes"][n, i] = g[midx[i]]
    return out


def relabel(pred, K, proposals, counts, image_hw, weights, gt, gt_classes, counts_g, thresh):
    """``relabel_boxes`` on the float64 decode of pred [N B, >= K + 5] fp32 and proposals [N, B, 4]."""
    return relabel_boxes(decode(pred, K, proposals, counts, image_hw, weights), K, counts, gt, gt_classes, counts_g, thresh)


RELABEL_N, RELABEL_B, RELABEL_GMAX = 2, 50, 6
RELABEL_KS = (3, 80)
RELABEL_CASES = (((50, 17), (6, 0)), ((0, 50), (0, 3)))          # (counts, counts_g)
RELABEL_HW = QC.STAGE_HW
RELABEL_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
RELABEL_THRESH = 0.5
PUSHED_OUT = (5, 6, 7, 8) + tuple(range(30, 40))                # rows of the main image whose deltas push them out of the image
NAN_ROW, TIE_ROW, EXACT_ROW, BELOW_ROW = 9, 12, 13, 14


def relabel_case(case, K, seed=31):
    """The inputs of one relabel case as numpy arrays: pred [100, Cpad], proposals [2, 50, 4], counts, image_hw, gt [2, 6, 4], gt_classes,
    counts_g.  The `main` image (the one with 50 rows and ground truth) holds: rows 5 / 6 / 7 / 8 pushed out to the left / top / right / bottom
    and rows 30..39 to the left (all clip to empty), row 9 with a NaN dx, row 12 whose decoded box IS ground-truth boxes 1 and 2 (equal
    IoU: the lower index wins), row 13 with IoU exactly 0.5 to box 0 (label 1 at the threshold) and, with six boxes, row 14 one ulp below 0.5
    to box 5.  The other image has no ground truth; its 17 rows (case 0) are all pushed out.  Everything past a count is poison."""
    counts, counts_g = RELABEL_CASES[case]
    main = int(np.argmax(counts))
    r = np.random.RandomState(seed + 7 * case + K)
    N, B, Gmax = RELABEL_N, RELABEL_B, RELABEL_GMAX
    cpad = (K + 1 + 4 + 3) // 4 * 4
    pred = np.full((N * B, cpad), np.nan, F)
    props = np.tile(np.array([0, 0, 1000, 1000], F), (N, B, 1))
    for n in range(N):
        c = counts[n]
        ih, iw = RELABEL_HW[n]
        ctr = r.rand(c, 2) * [0.6 * iw, 0.6 * ih] + [0.2 * iw, 0.2 * ih]
        wh = np.exp(r.uniform(np.log(6), np.log(30), (c, 2)))
        props[n, :c] = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)
        rows = slice(n * B, n * B + c)
        pred[rows] = 0
        pred[rows, :K + 1] = r.uniform(-5, 5, (c, K + 1))
        pred[rows, K + 1:K + 5] = r.randn(c, 4) * [1.0, 1.0, 0.5, 0.5]
        if n != main:
            pred[rows, K + 1] = -2400.0                          # every box of the other image leaves on the left
    o = main * B
    for j in PUSHED_OUT:
        pred[o + j, K + 1:K + 5] = {5: (-2400, 0, 0, 0), 6: (0, -2400, 0, 0), 7: (2400, 0, 0, 0), 8: (0, 2400, 0, 0)}.get(j, (-2400, 0, 0, 0))
    pred[o + NAN_ROW, K + 1] = np.nan                           # dx: the centre is NaN (a NaN dw / dh is clamped away by fmin)
    for j, p in ((EXACT_ROW, (0, 0, 10, 10)), (BELOW_ROW, (20, 0, 28, 30))):
        props[main, j] = p
        pred[o + j, K + 1:K + 5] = 0                             # zero deltas on small integers: the decoded box is the proposal, exactly
    hw = np.array(RELABEL_HW, F)
    _, bx, _ = QB.scores_boxes(np.nan_to_num(pred), K, True, props, counts, hw, RELABEL_WEIGHTS)
    dec = bx[main, :, 0].astype(F)
    below = np.array([20, 0, 28, np.nextafter(F(15), F(0))], F)
    gts = {6: [(0, 0, 10, 5), dec[TIE_ROW], dec[TIE_ROW], dec[10], dec[11] + F(0.25), below], 3: [(0, 0, 10, 5), dec[TIE_ROW], dec[TIE_ROW]]}
    gt = np.full((N, Gmax, 4), 1e6, F)
    gc = np.full((N, Gmax), 10 ** 6, np.int32)
    G = counts_g[main]
    gt[main, :G] = np.array(gts[G], F)
    gc[main, :G] = (np.arange(G) + 1) % K
    return {"pred": pred, "proposals": props, "counts": np.array(counts, np.int32), "image_hw": hw, "gt": gt, "gt_classes": gc,
            "counts_g": np.array(counts_g, np.int32), "main": main}


# ------------------------------------------------------------------------------------------------ list-masked BatchNorm + ReLU
BN_SHAPES = ((2, 5, 49, 12), (3, 40, 49, 96), (2, 24, 196, 256))             # (N, B, P1, C)
BN_FAMILIES = ("unit", "offset_1e4", "const_channel")
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def bn_counts(N, B):
    """name -> counts of a masked-BN case: a full image beside an empty one (and a partial one when N = 3), all full, all zero; one entry above
    B and one below 0, which the kernels clamp."""
    mixed = [B, 0, max(1, B // 3)][:N]
    return {"mixed": mixed, "full": [B] * N, "zero": [0] * N, "clamped": ([B + 3, -2, 1])[:N]}


def valid_rows(counts, B):
    """bool [N B]: row n B + j is valid iff j < min(max(counts[n], 0), B)"""
    return torch.cat([torch.arange(B) < min(max(int(c), 0), B) for c in counts])


def bn_input(family, N, B, P1, C, counts, seed=0):
    """x [N B, P1, C] fp32 of a family of elementwise_f64.stats_input over the whole list, NaN on the padding rows."""
    x = E.stats_input(family, N * B * P1, C, seed).view(N * B, P1, C).clone()
    x[~valid_rows(counts, B)] = float("nan")
    return x


def masked_stats(x, counts, B, eps, momentum=None, running_mean=None, running_var=None):
    """elementwise_f64.bn_stats over the valid pixels; no valid row: mean 0, var 0, invstd 1 / sqrt(eps), the running buffers unchanged."""
    v = valid_rows(counts, B)
    C = x.shape[-1]
    if not bool(v.any()):
        out = {"mean": torch.zeros(C, dtype=torch.float64), "var": torch.zeros(C, dtype=torch.float64),
               "invstd": torch.full((C,), 1.0 / math.sqrt(E.f32(eps)), dtype=torch.float64)}
        if running_mean is not None:
            out["running_mean"], out["running_var"] = E.d(running_mean), E.d(running_var)
        return out
    return E.bn_stats(x[v].reshape(-1, C), eps, momentum, running_mean, running_var)


def _scatter(v, compact, shape):
    out = torch.zeros(shape, dtype=torch.float64)
    out[v] = compact.view(-1, *shape[1:])
    return out


def masked_relu_fwd(x, counts, B, mean, invstd, gamma, beta, relu=True):
    """(y, terms) [N B, P1, C] float64: relu (or not) of elementwise_f64.bn_apply on the valid rows, zero on the padding rows."""
    v = valid_rows(counts, B)
    C = x.shape[-1]
    y, terms = E.bn_apply(x[v].reshape(-1, C), mean, invstd, gamma, beta, 0.0 if relu else 1.0)
    return _scatter(v, y, x.shape), _scatter(v, terms, x.shape)


def masked_gprime(g, y, counts, B, relu=True):
    """g' on the valid rows as a dense [Pn, C] fp32 matrix: g [y > 0] with the given (stored) y"""
    v = valid_rows(counts, B)
    gv = g[v].reshape(-1, g.shape[-1])
    return gv * (y[v].reshape(-1, g.shape[-1]) > 0) if relu else gv


def masked_bwd_sums(g, x, y, counts, B, mean, invstd, relu=True):
    """(sum g', sum g' xhat) float64 over the valid rows; zeros when there is none"""
    v = valid_rows(counts, B)
    C = x.shape[-1]
    if not bool(v.any()):
        return torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    return E.bn_bwd_sums(masked_gprime(g, y, counts, B, relu), x[v].reshape(-1, C), mean, invstd)


def masked_bwd_dx(g, x, y, counts, B, mean, invstd, gamma, s0, s1, relu=True):
    """(dx, terms) [N B, P1, C] float64 from the given sums: elementwise_f64.bn_bwd_dx with Pn = the valid pixels, zero on the padding rows"""
    v = valid_rows(counts, B)
    C = x.shape[-1]
    if not bool(v.any()):
        return torch.zeros(x.shape, dtype=torch.float64), torch.zeros(x.shape, dtype=torch.float64)
    Pn = int(v.sum()) * x.shape[1]
    dx, terms = E.bn_bwd_dx(masked_gprime(g, y, counts, B, relu), x[v].reshape(-1, C), mean, invstd, gamma, s0, s1, Pn)
    return _scatter(v, dx, x.shape), _scatter(v, terms, x.shape)


# ------------------------------------------------------------------------------------------------ the whole heads in torch autograd
class _ScaleGradient(torch.autograd.Function):
    """detectron2's _ScaleGradient: identity forward, the gradient times `scale`"""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.scale, None


def pooled_rows(xs, min_level, S, sampling_ratio, boxes, counts):
    """(the ROIAlign features of the VALID rows [Rv, C, S, S] in the dtype of xs, differentiable in xs; [(n, j)] of those rows): the two
    axis-weight matrices of every box, as roi_loss_f64.torch_losses builds them; a box with a non-positive side pools to zeros."""
    dt, C = xs[0].dtype, xs[0].shape[1]
    live = {(n, j): (bx, level) for n, j, bx, level in RL._live_boxes(boxes, counts, min_level, len(xs))}
    rows, meta = [], []
    for n in range(boxes.shape[0]):
        for j in range(int(counts[n])):
            if (n, j) in live:
                bx, level = live[(n, j)]
                f = xs[level - min_level][n]
                Wy, Wx, gh, gw = RL._box_tables(bx, level, S, sampling_ratio, f.shape[1], f.shape[2])
                rows.append(torch.einsum("ph,chw,qw->cpq", torch.tensor(Wy, dtype=dt), f, torch.tensor(Wx, dtype=dt)) / max(gh * gw, 1))
            else:
                rows.append(torch.zeros((C, S, S), dtype=dt))
            meta.append((n, j))
    return torch.stack(rows), meta


def conv_norm_relu_train(x, sd, q, norm, eps=1e-5, momentum=0.1, buffers=None):
    """relu(norm(conv2d(x, sd[q.weight], sd[q.bias] or None, padding 1))) with the norm in training: F.batch_norm(training=True) over the rows
    of x for "BN" / "SyncBN" (buffers: {key: running statistic} updated in place, or None), the frozen formula for "FrozenBN"."""
    Fn = torch.nn.functional
    x = Fn.conv2d(x, sd[q + ".weight"], sd.get(q + ".bias"), padding=1)
    if norm in ("BN", "SyncBN"):
        rm, rv = (buffers[q + ".norm.running_mean"], buffers[q + ".norm.running_var"]) if buffers is not None else (None, None)
        x = Fn.batch_norm(x, rm, rv, sd[q + ".norm.weight"], sd[q + ".norm.bias"], training=True, momentum=momentum, eps=eps)
    elif norm == "FrozenBN":
        g, b, m, v = (sd[f"{q}.norm.{k}"].view(1, -1, 1, 1) for k in QC.NORM_KEYS)
        x = (x - m) / torch.sqrt(v + eps) * g + b
    return torch.relu(x)


def torch_normed_mask_loss(xs, sd, norm, min_level, S, sampling_ratio, boxes, counts, cls, tg, Km, buffers=None, prefix="mask_head."):
    """mask_loss_f64.torch_mask_loss for a mask head with normed convs: the mask pooler on the valid foreground rows, ``conv_norm_relu_train``
    per ``mask_fcn``, the deconv with ReLU, the predictor and the mean binary cross-entropy with logits of the rows' own classes."""
    Fn = torch.nn.functional
    x, meta = pooled_rows(xs, min_level, S, sampling_ratio, boxes, counts)
    i = 1
    while f"{prefix}mask_fcn{i}.weight" in sd:
        x = conv_norm_relu_train(x, sd, f"{prefix}mask_fcn{i}", norm, buffers=buffers)
        i += 1
    x = torch.relu(Fn.conv_transpose2d(x, sd[prefix + "deconv.weight"], sd[prefix + "deconv.bias"], stride=2))
    logits = Fn.conv2d(x, sd[prefix + "predictor.weight"], sd[prefix + "predictor.bias"])
    sel = torch.stack([logits[i, 0 if Km == 1 else int(cls[n, j])] for i, (n, j) in enumerate(meta)])
    t = torch.tensor(np.stack([tg[n, j] for n, j in meta]).astype(np.float64), dtype=x.dtype)
    return Fn.binary_cross_entropy_with_logits(sel, t, reduction="mean")


def head_forward(x, sd, stage, norm, eps=1e-5, momentum=0.1, buffers=None):
    """Stage `stage`'s (logits [Rv, K + 1], deltas [Rv, 4]) on the valid rows x [Rv, C, S, S]: F.conv2d, the norm -- F.batch_norm(training=True)
    over exactly these rows for "BN" / "SyncBN" (`buffers`: {key: tensor} running statistics updated in place, or None), the frozen formula
    for "FrozenBN" --, relu, the flatten in [C][S][S] order, F.linear + relu, the predictor.  sd: the heads' state dict in x's dtype."""
    Fn = torch.nn.functional
    hd, pr, i = f"box_head.{stage}.", f"box_predictor.{stage}.", 1
    while f"{hd}conv{i}.weight" in sd:
        x = conv_norm_relu_train(x, sd, f"{hd}conv{i}", norm, eps, momentum, buffers)
        i += 1
    x, i = x.flatten(1), 1
    while f"{hd}fc{i}.weight" in sd:
        x = torch.relu(Fn.linear(x, sd[f"{hd}fc{i}.weight"], sd[f"{hd}fc{i}.bias"]))
        i += 1
    return Fn.linear(x, sd[pr + "cls_score.weight"], sd[pr + "cls_score.bias"]), Fn.linear(x, sd[pr + "bbox_pred.weight"], sd[pr + "bbox_pred.bias"])


def stage_losses(logits, deltas, meta, boxes, cls, gboxes, K, weights, beta):
    """FastRCNNOutputs' two losses (class-agnostic regression) over the valid rows `meta`, as roi_loss_f64.torch_losses states them"""
    Fn = torch.nn.functional
    dt = logits.dtype
    tc = torch.tensor([int(cls[n, j]) for n, j in meta], dtype=torch.int64)
    rtot = len(meta)
    loss_cls = Fn.cross_entropy(logits, tc, reduction="sum") / rtot
    fg = [i for i, (n, j) in enumerate(meta) if cls[n, j] < K]
    if not fg:
        return loss_cls, deltas.sum() * 0
    tgt = torch.tensor([[float(F(v)) for v in RL.rl.get_deltas(boxes[meta[i]], gboxes[meta[i]], weights)] for i in fg], dtype=dt)
    d = deltas[torch.tensor(fg)] - tgt
    ad = d.abs()
    return loss_cls, (ad.sum() if beta < 1e-5 else torch.where(ad < beta, 0.5 * d * d / beta, ad - 0.5 * beta).sum()) / rtot


def torch_cascade_losses(xs, sd, stages, min_level, S, sampling_ratio, K, stage_weights, beta, norm, buffers=None):
    """[(loss_cls_k, loss_box_reg_k)] of the whole box cascade in the dtype of xs on a GIVEN per-stage assignment (stages[k]: boxes, counts,
    gt_classes, gt_boxes as numpy arrays): per stage the valid rows by index selection, the pooled features through _ScaleGradient(1 / S),
    ``head_forward``, ``stage_losses``.  Differentiable in xs and in the tensors of sd."""
    out = []
    for k, st in enumerate(stages):
        x, meta = pooled_rows(xs, min_level, S, sampling_ratio, st["boxes"], st["counts"])
        x = _ScaleGradient.apply(x, 1.0 / len(stages))
        lg, dl = head_forward(x, sd, k, norm, buffers=buffers)
        out.append(stage_losses(lg, dl, meta, st["boxes"], st["gt_classes"], st["gt_boxes"], K, stage_weights[k], beta))
    return out


# ------------------------------------------------------------------------------------------------ whole-heads test inputs
HEAD_FEATURES = ("p2", "p3", "p4", "p5")
HEAD_IMAGE, HEAD_LEVELS, HEAD_MIN_LEVEL = QB.ALIGN_IMAGE, QB.ALIGN_LEVELS, QB.ALIGN_MIN_LEVEL
HEAD_N, HEAD_K, HEAD_BATCH, HEAD_FRACTION, HEAD_S, HEAD_FC = 2, 5, 24, 0.5, 7, 32
HEAD_IOUS = (0.5, 0.6, 0.7)
HEAD_WEIGHTS = ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))
HEAD_VARIANTS = {"c8": (8, "", 3), "c8_syncbn": (8, "SyncBN", 3), "c8_frozenbn": (8, "FrozenBN", 3), "c128_syncbn": (128, "SyncBN", 3),
                 "c8_syncbn_one_stage": (8, "SyncBN", 1)}                           # channels, NORM, stages


def head_case(seed=11):
    """roi_loss_f64.e2e_case's layout for the cascade: per image 4 ground-truth boxes, 14 proposals that are jittered copies of them (IoU well
    above 0.7) and 12 background proposals far from every box, two of them of zero width -- they are sampled (the background quota takes all
    twelve), pool to zeros and are dropped by the first relabel."""
    rng = np.random.default_rng(seed)
    ih, iw = HEAD_IMAGE
    gts, gcs, props = [], [], []
    for n in range(HEAD_N):
        side = np.array([[14, 18], [22, 16], [30, 34], [18, 26]], np.float64)
        ctr = np.array([[14, 14], [60, 16], [38, 42], [64, 48]], np.float64) + rng.uniform(-2, 2, (4, 2))
        g = np.concatenate([ctr - side / 2, ctr + side / 2], 1)
        g[:, 0::2], g[:, 1::2] = g[:, 0::2].clip(0, iw), g[:, 1::2].clip(0, ih)
        j = np.arange(14) % 4
        fg = g[j] + rng.uniform(-1, 1, (14, 4)) * 0.03 * np.minimum(side[j, :1], side[j, 1:])
        c = np.array([[3, 40], [12, 58], [30, 8], [40, 6], [76, 4], [4, 60], [50, 60], [22, 30], [74, 30], [46, 20], [33, 62], [8, 32]], np.float64)
        bg = np.concatenate([c - 2.5, c + 2.5], 1)
        bg[3, 2], bg[9, 2] = bg[3, 0], bg[9, 0]                     # zero width
        p = np.concatenate([fg, bg], 0)
        p[:, 0::2], p[:, 1::2] = p[:, 0::2].clip(0, iw), p[:, 1::2].clip(0, ih)
        gts.append(g.astype(F))
        gcs.append(rng.integers(0, HEAD_K, 4).astype(np.int32))
        props.append(p.astype(F))
    keys = rng.integers(0, 2 ** 32, size=(HEAD_N, 26 + 4), dtype=np.uint64).astype(np.uint32)
    return dict(proposals=np.stack(props), counts_p=np.array([26, 26], np.int32), gts=gts, gt_classes=gcs, keys=keys)


def head_features(channels, seed=12):
    g = torch.Generator().manual_seed(seed)
    return {f: torch.randn((HEAD_N, channels, h, w), generator=g) for f, (h, w) in zip(HEAD_FEATURES, HEAD_LEVELS)}


def build_train_heads(amd, channels, norm, stages, masks=False, mask_norm="", seed=13, box_scale=0.3):
    """CascadeROIHeads on the CPU for the training tests: NUM_CONV 2, NUM_FC 1, BATCH_SIZE_PER_IMAGE 24 with half of it foreground, seeded
    weights (cascade_f64.build_heads' scales; small box deltas, so that a stage's boxes stay near the ground truth they were matched to)."""
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": bool(masks),
                               "ROI_HEADS": {"NAME": "CascadeROIHeads", "IN_FEATURES": list(HEAD_FEATURES), "NUM_CLASSES": HEAD_K,
                                             "BATCH_SIZE_PER_IMAGE": HEAD_BATCH, "POSITIVE_FRACTION": HEAD_FRACTION},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 1, "FC_DIM": HEAD_FC, "NUM_CONV": 2, "CONV_DIM": channels,
                                                "NORM": norm, "POOLER_RESOLUTION": HEAD_S, "POOLER_SAMPLING_RATIO": 2, "CLS_AGNOSTIC_BBOX_REG": True},
                               "ROI_BOX_CASCADE_HEAD": {"IOUS": HEAD_IOUS[:stages], "BBOX_REG_WEIGHTS": HEAD_WEIGHTS[:stages]},
                               "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": 2, "CONV_DIM": 16, "NORM": mask_norm,
                                                 "POOLER_RESOLUTION": 14, "POOLER_SAMPLING_RATIO": 2}})
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=2 ** int(f[1:])) for f in HEAD_FEATURES}, masks=bool(masks), cascade=True)
    g = torch.Generator().manual_seed(seed)
    for name, p in list(h.named_parameters()) + list(h.named_buffers()):
        leaf, owner = name.split(".")[-1], name.split(".")[-2]
        if leaf == "num_batches_tracked":
            continue
        if owner == "norm":
            v = {"weight": 0.5 + torch.rand(p.shape, generator=g), "bias": torch.randn(p.shape, generator=g) * 0.1,
                 "running_mean": torch.randn(p.shape, generator=g) * 0.1, "running_var": 0.5 + 1.5 * torch.rand(p.shape, generator=g)}[leaf]
        elif leaf == "weight":
            fan_in = p[0].numel() if "deconv" not in name else p.shape[0]
            v = torch.randn(p.shape, generator=g) * {"cls_score": 2.0, "bbox_pred": box_scale, "predictor": 3.0}.get(owner, 1.4) / math.sqrt(fan_in)
        else:
            v = torch.randn(p.shape, generator=g) * 0.1
        with torch.no_grad():
            p.copy_(v)
    return h


def chain_train(sd, feats, case, norm, stages):
    """The per-stage assignment of the whole cascade on the CPU in float64: stage 0 by roi_loss_f64.assign, stage k > 0 by ``relabel`` on the
    float64 head's predictor output rounded to fp32.  [dict(boxes, counts, gt_classes, gt_boxes)] -- what the host test proves the
    conditions of the GPU test's inputs on."""
    a = RL.assign(case, HEAD_K, HEAD_BATCH, HEAD_FRACTION, HEAD_IOUS[0])
    st = dict(boxes=a["boxes"], counts=a["counts"], gt_classes=a["cls"], gt_boxes=a["gboxes"])
    gt, gc, cg = RL.pad_lists([np.zeros((0, 4), F)] * HEAD_N, case["gts"], case["gt_classes"])[2:]
    sd64 = {k: v.detach().double() for k, v in sd.items() if v.is_floating_point()}
    xs = [feats[f].double() for f in HEAD_FEATURES]
    hw = np.array([HEAD_IMAGE] * HEAD_N, F)
    out = [st]
    for k in range(stages - 1):
        with torch.no_grad():
            x, meta = pooled_rows(xs, HEAD_MIN_LEVEL, HEAD_S, 2, st["boxes"], st["counts"])
            lg, dl = head_forward(x, sd64, k, norm)
        pred = np.zeros((HEAD_N * HEAD_BATCH, HEAD_K + 5), F)
        for i, (n, j) in enumerate(meta):
            pred[n * HEAD_BATCH + j] = torch.cat([lg[i], dl[i]]).numpy()
        r = relabel(pred, HEAD_K, st["boxes"], st["counts"], hw, HEAD_WEIGHTS[k], gt, gc, cg, HEAD_IOUS[k + 1])
        st = dict(boxes=r["boxes"], counts=r["counts"], gt_classes=r["gt_classes"], gt_boxes=r["gt_boxes"], src=r["src"])
        out.append(st)
    return out
