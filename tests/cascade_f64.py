"""fp64 restatement of CascadeROIHeads at inference (detectron2 v0.1.1 semantics, afigan_amd/roi_heads.py's docstring), the checker of
tests/test_gpu_cascade.py and tests/test_cascade_host.py.  ROIAlign, scores / boxes, candidates, NMS, pick and the mask stages are roi_f64's and
mask_f64's; new here: conv + norm + ReLU (un-folded: the conv, then the norm's formula), the conv-FC head chain, the normed mask head chain and
the mean of the stages' scores in numpy fp32.  Staged as those checkers are: a test feeds each stage the KERNEL's previous output; ``chain``
runs the whole cascade on the CPU (what the host test proves the seeded inputs' conditions on).  Also the seeded inputs of both test files."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import mask_f64 as QM
import roi_f64 as QB

NORM_EPS = 1e-5
NORM_KEYS = ("weight", "bias", "running_mean", "running_var")


# ------------------------------------------------------------------------------------------------ the head
def norm_of(params, prefix):
    """The four tensors of the norm child of the conv `prefix` (None when the conv has a bias instead)."""
    return {k: params[f"{prefix}.norm.{k}"] for k in NORM_KEYS} if f"{prefix}.norm.weight" in params else None


def conv_norm_relu(x, weight, bias=None, norm=None, dtype=torch.float64):
    """relu(norm(conv2d(x, weight [O, I, 3, 3], bias, padding 1))) in `dtype` on the CPU; norm: y = (x - running_mean) / sqrt(running_var + eps)
    weight + bias, applied to the conv's output (not folded)."""
    y = F.conv2d(x.detach().cpu().to(dtype), weight.detach().cpu().to(dtype), None if bias is None else bias.detach().cpu().to(dtype), padding=1)
    if norm is not None:
        g, b, m, v = (norm[k].detach().cpu().to(dtype).view(1, -1, 1, 1) for k in NORM_KEYS)
        y = (y - m) / torch.sqrt(v + NORM_EPS) * g + b
    return torch.relu(y)


def conv_fc_head(pooled, params, stage=0, dtype=torch.float64):
    """pooled [R, C, S, S]; params: the heads' state dict.  Stage `stage`'s ([conv outputs [R, CONV_DIM, S, S]], [fc outputs [R, FC]], cls logits
    [R, K + 1], deltas [R, 4]) in `dtype`, the flatten in detectron2's [C][S][S] order."""
    p = {k: v.detach().cpu() for k, v in params.items()}
    hd, pr = f"box_head.{stage}.", f"box_predictor.{stage}."
    x, convs, fcs, i = pooled.detach().cpu().to(dtype), [], [], 1
    while f"{hd}conv{i}.weight" in p:
        x = conv_norm_relu(x, p[f"{hd}conv{i}.weight"], p.get(f"{hd}conv{i}.bias"), norm_of(p, f"{hd}conv{i}"), dtype)
        convs.append(x)
        i += 1
    x, i = x.flatten(1), 1
    while f"{hd}fc{i}.weight" in p:
        x = torch.relu(x @ p[f"{hd}fc{i}.weight"].to(dtype).t() + p[f"{hd}fc{i}.bias"].to(dtype))
        fcs.append(x)
        i += 1
    return (convs, fcs, x @ p[pr + "cls_score.weight"].to(dtype).t() + p[pr + "cls_score.bias"].to(dtype),
            x @ p[pr + "bbox_pred.weight"].to(dtype).t() + p[pr + "bbox_pred.bias"].to(dtype))


def mask_head_chain(pooled, params, dtype=torch.float64, prefix="mask_head."):
    """([every mask_fcn's output], the deconv's 4-phase output) of the mask head with or without norm, in `dtype`."""
    x, acts, i = pooled, [], 1
    while f"{prefix}mask_fcn{i}.weight" in params:
        q = f"{prefix}mask_fcn{i}"
        x = conv_norm_relu(x, params[q + ".weight"], params.get(q + ".bias"), norm_of(params, q), dtype)
        acts.append(x)
        i += 1
    return acts, QM.deconv_phases(x, params[f"{prefix}deconv.weight"], params[f"{prefix}deconv.bias"], dtype)


def mean_scores(per_stage):
    """detectron2's ``sum(scores_per_stage) * (1.0 / S)`` on fp32 tensors: ((s0 + s1) + ...) * float32(1 / S), every operation in fp32."""
    acc = np.asarray(per_stage[0], np.float32)
    with np.errstate(invalid="ignore"):
        for s in per_stage[1:]:
            acc = acc + np.asarray(s, np.float32)
        return acc * np.float32(1.0 / len(per_stage))


def chain(params, levels, min_level, boxes, counts, image_hw, S, sampling_ratio, K, weights):
    """The whole box cascade on the CPU: per stage fp64 ROIAlign, head and decode from that stage's fp32 box list, the predictor's output and
    the stage's scores and boxes rounded to fp32 (what the kernels store).  Returns (mean scores [N, P, K] fp32, last boxes [N, P, 4] fp32,
    [per-stage fp32 scores])."""
    cur, per = np.asarray(boxes, np.float32), []
    for k, w in enumerate(weights):
        pooled, _, _ = QB.roi_align(levels, min_level, cur, counts, S, sampling_ratio)
        _, _, lg, dl = conv_fc_head(torch.from_numpy(pooled), params, k)
        pred = torch.cat([lg, dl], 1).float().numpy()
        s, b, _ = QB.scores_boxes(pred, K, True, cur, counts, image_hw, w)
        per.append(s.astype(np.float32))
        cur = b[:, :, 0].astype(np.float32)
    return mean_scores(per), cur, per


def selection_facts(scores, boxes, thresh, nms_thresh, M=1024):
    """Per image of scores [N, P, K] / boxes [N, P, 4]: (valid candidates, kept by the class-aware greedy NMS)."""
    out = []
    for n in range(scores.shape[0]):
        idx, valid, _ = QB.candidates(scores[n], thresh, M)
        r, c = idx // scores.shape[2], idx % scores.shape[2]
        keep = QB.nms_classes(boxes[n][r], c, valid, nms_thresh, rounding_pairs_in_fp32=True)
        out.append((int(valid.sum()), int(keep.sum())))
    return out


# ------------------------------------------------------------------------------------------------ afi_roi_cascade_stage test inputs
STAGE_N, STAGE_P = 2, 50
STAGE_COUNTS = ((50, 17), (0, 50))
STAGE_KS = (80, 3, 1)
STAGE_WEIGHTS = ((10.0, 10.0, 5.0, 5.0), (30.0, 30.0, 15.0, 15.0))
STAGE_HW = ((60.0, 90.0), (75.0, 50.0))


def stage_case(K, seed=21):
    """(pred [100, Cpad] fp32: logits in +-30, 4 deltas; proposals [2, 50, 4]).  Rows 3 / 4 (and 53 / 54): dw / dh above the clamp under both
    weight sets; 5 / 55: clipped at 0; 6 / 56: clipped at the image size; 7 / 57: a NaN logit."""
    r = np.random.RandomState(seed + K)
    N, P = STAGE_N, STAGE_P
    cpad = (K + 1 + 4 + 3) // 4 * 4
    pred = np.zeros((N * P, cpad), np.float32)
    pred[:, :K + 1] = r.uniform(-30, 30, (N * P, K + 1))
    pred[:, K + 1:K + 5] = r.randn(N * P, 4) * 4
    for o in (0, P):
        pred[o + 3, K + 3] = 90.0                             # dw above the clamp: 90 / 15 = 6 > log(1000 / 16)
        pred[o + 4, K + 4] = 75.0
        pred[o + 5, K + 1:K + 5] = (-2400, -2400, 0, 0)
        pred[o + 6, K + 1:K + 5] = (2400, 2400, 0, 0)
        pred[o + 7, 0] = np.nan
    props = np.zeros((N, P, 4), np.float32)
    for n in range(N):
        ctr = r.rand(P, 2) * [STAGE_HW[n][1], STAGE_HW[n][0]]
        wh = np.exp(r.uniform(np.log(2), np.log(40), (P, 2)))
        props[n] = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)
    return pred, props


def stage_prev(K, counts, seed=23):
    """An arbitrary running score [2, 50, K] fp32 (sums of up to three probabilities), -inf in the rows past counts."""
    r = np.random.RandomState(seed + K)
    prev = (r.rand(STAGE_N, STAGE_P, K) * 3).astype(np.float32)
    for n, c in enumerate(counts):
        prev[n, c:] = -np.inf
    return prev


# ------------------------------------------------------------------------------------------------ head test inputs
HEAD_CASES = {"a": (256, 7, 4, 256, 1024, 24), "b": (256, 7, 4, 256, 1024, 5), "c": (16, 7, 4, 16, 64, 24)}    # C, S, NUM_CONV, CONV_DIM, FC, R / 2
HEAD_NORMS = ("SyncBN", "")


def build_heads(amd, features, channels, K=80, S=7, fc=64, num_conv=4, conv_dim=None, norm="SyncBN", stages=3, masks=False, Sm=14, mask_conv=2,
                thresh=0.05, D=20, seed=0, cls_scale=3.0, box_scale=2.0, cls_bias=None):
    """CascadeROIHeads on the CPU with seeded weights, non-trivial norm statistics (running_var in [0.5, 2]) and every parameter set; the
    caller moves it to the GPU."""
    from afigan_amd.fpn_sr import ShapeSpec
    weights = ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))[:stages]
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": bool(masks),
                               "ROI_HEADS": {"NAME": "CascadeROIHeads", "IN_FEATURES": list(features), "NUM_CLASSES": K, "SCORE_THRESH_TEST": thresh},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 1, "FC_DIM": fc, "NUM_CONV": num_conv, "CONV_DIM": conv_dim or channels,
                                                "NORM": norm, "POOLER_RESOLUTION": S, "CLS_AGNOSTIC_BBOX_REG": True},
                               "ROI_BOX_CASCADE_HEAD": {"IOUS": (0.5, 0.6, 0.7)[:stages], "BBOX_REG_WEIGHTS": weights},
                               "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": mask_conv, "CONV_DIM": conv_dim or channels, "NORM": norm,
                                                 "POOLER_RESOLUTION": Sm}})
    cfg.TEST.DETECTIONS_PER_IMAGE = D
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=2 ** int(f[1:])) for f in features}, masks=bool(masks), cascade=True)
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
            scale = {"cls_score": cls_scale, "bbox_pred": box_scale, "predictor": 3.0}.get(owner, 1.4)
            v = torch.randn(p.shape, generator=g) * scale / math.sqrt(fan_in)
        else:
            v = torch.randn(p.shape, generator=g) * 0.1
            if owner == "cls_score" and cls_bias is not None:
                v[:len(cls_bias)] += torch.tensor(cls_bias)
        with torch.no_grad():
            p.copy_(v)
    return h.eval()


# ------------------------------------------------------------------------------------------------ whole-heads test inputs
WHOLE_P, WHOLE_COUNTS = 24, (24, 9)
WHOLE_LAYOUTS = {"fpn": (("p2", "p3", "p4", "p5"), (64, 80), QB.ALIGN_LEVELS, ((64.0, 80.0), (60.0, 77.0))),
                 "swin": (("p3", "p4", "p5", "p6"), (128, 160), ((16, 20), (8, 10), (4, 5), (2, 3)), ((128.0, 160.0), (120.0, 153.0)))}
WHOLE_CASES = (("fpn", 3, 80, True), ("fpn", 1, 3, False), ("swin", 3, 3, False))          # layout, stages, K, masks
WHOLE_C, WHOLE_FC = 16, 64
WHOLE_CLS_BIAS = (3.0, 2.5, 2.0)                              # three favoured classes, so that boxes of one class overlap and NMS has work


def whole_boxes(layout, seed=7):
    """[2, 24, 4] fp32 inside the image: jittered copies of five base boxes per image (so that NMS both keeps and suppresses), all random: no
    box is built on a level or grid boundary."""
    _, (ih, iw), _, _ = WHOLE_LAYOUTS[layout]
    r = np.random.RandomState(seed + len(layout))
    out = np.zeros((2, WHOLE_P, 4), np.float32)
    for n in range(2):
        side = np.exp(r.uniform(np.log(0.2 * ih), np.log(0.8 * ih), (5, 2)))
        ctr = r.rand(5, 2) * [0.6 * iw, 0.6 * ih] + [0.2 * iw, 0.2 * ih]
        j = np.arange(WHOLE_P) % 5
        s = side[j] * np.exp(r.randn(WHOLE_P, 2) * 0.08)
        c = ctr[j] + r.randn(WHOLE_P, 2) * 0.05 * side[j]
        b = np.concatenate([c - s / 2, c + s / 2], 1)
        b[:, 0::2] = b[:, 0::2].clip(0, iw)
        b[:, 1::2] = b[:, 1::2].clip(0, ih)
        out[n] = b.astype(np.float32)
    return out


def whole_features(layout, seed=52):
    g = torch.Generator().manual_seed(seed)
    feats, _, levels, _ = WHOLE_LAYOUTS[layout]
    return {f: torch.randn((2, WHOLE_C, hh, ww), generator=g) for f, (hh, ww) in zip(feats, levels)}


def whole_heads(amd, layout, stages, K, masks):
    feats = WHOLE_LAYOUTS[layout][0]
    return build_heads(amd, feats, WHOLE_C, K=K, S=7, fc=WHOLE_FC, num_conv=2, norm="SyncBN", stages=stages, masks=masks, mask_conv=2, D=20, seed=51,
                       cls_scale=2.0, box_scale=1.0, cls_bias=WHOLE_CLS_BIAS[:min(K, 3)])
