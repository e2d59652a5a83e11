"""The frozen box branch of the inference configs' ROI heads: detectron2 v0.1.1's ``StandardROIHeads`` (``ROIPooler`` with ROIAlignV2,
``FastRCNNConvFCHead`` with FCs only, ``FastRCNNOutputLayers``, ``fast_rcnn_inference``) at inference, forward only, fp32, on this package's
HIP kernels; with ``masks=True`` the mask branch as well (``MaskRCNNConvUpsampleHead``, ``mask_rcnn_inference``; below).  ``CascadeROIHeads``
(``build_roi_heads(cfg, input_shape, cascade=True)``; at the end) shares all of it.  The keypoint branch is out of scope.

Per image, on the padded proposal list boxes [N, P, 4] with counts [N] (``RPN.forward_padded``'s layout):
  - ROIPooler: box -> level clamp(floor(4 + log2(sqrt(area) / 224)), min, max) of ``MODEL.ROI_HEADS.IN_FEATURES`` (zero / negative area: min),
    ROIAlignV2 (aligned: start = x1 / stride - 0.5) to POOLER_RESOLUTION^2 bins, POOLER_SAMPLING_RATIO samples per bin and axis or
    ceil(roi / S) when it is 0; a box with a non-positive side pools to zeros.  Rows past counts are zero.
  - box head: x = relu(fc_i(x)), fc1 on the flattened [C, S, S] features; predictor: K + 1 class logits (background last) and 4 K (or 4,
    CLS_AGNOSTIC_BBOX_REG) deltas.
  - scores = softmax without the background column; boxes = Box2BoxTransform(BBOX_REG_WEIGHTS).apply_deltas with dw / dh clamped at
    log(1000 / 16), clipped to the image; both in fp64 from the fp32 values, rounded once.
  - the M = 1024 highest scores of the image (score descending, index r K + c ascending -- detectron2 leaves ties open; this is the rule
    here; NaN below every number), valid = score > SCORE_THRESH_TEST; class-aware greedy NMS at NMS_THRESH_TEST on the boxes as they are
    (torchvision's batched_nms adds a per-class coordinate offset first, which rounds the boxes: not done); the first
    TEST.DETECTIONS_PER_IMAGE kept candidates.
  - ``truncated`` = more than M scores above the threshold AND fewer than DETECTIONS_PER_IMAGE kept: the one case in which the cut at M can
    change the result (greedy NMS in score order is decided by the list's prefix up to the last kept box).  ``forward`` raises then.

Keys: ``box_head.fc{i}.{weight, bias}``, ``box_predictor.{cls_score, bbox_pred}.{weight, bias}`` -- detectron2's, so a detector checkpoint's
``roi_heads.box_*`` keys load with strict=True.  Every parameter has requires_grad False until ``trainable_()``.

Training, box branch (``StandardROIHeads.losses``, and ``forward`` in training mode with ``targets``): ROIHeads.label_and_sample_proposals,
get_deltas, softmax_cross_entropy_loss and smooth_l1_loss on afi_roi_label / afi_rpn_sample / afi_roi_gather_samples / afi_roi_box_loss
(csrc/roi_loss.hip), the pooler and head forward on the kernels above, their backward on afi_conv1x1_dgrad / afi_conv1x1_wgrad / afi_relu_bwd
and afi_roi_align_bwd (``_ROIBoxLossFn``).  The sample is decided by 32-bit keys, as in ``RPN.losses``.  One IOU_THRESHOLDS entry with
IOU_LABELS [0, 1]; crowd handling and TRAIN_ON_PRED_BOXES are out of scope (AfiError).  CascadeROIHeads trains after its ``trainable_()`` (at the end).

Training, mask branch (heads built with ``masks=True``: ``losses`` returns ``loss_mask`` as well): detectron2's mask_rcnn_loss on the first
Bf = int(BATCH_SIZE_PER_IMAGE POSITIVE_FRACTION) rows of the box branch's training list, whose n_pos positives come first -- one label /
sample / gather for both branches.  The targets are the matched instance's polygons (``gt_masks``) rasterised inside the row's box on the
2S x 2S canvas (afi_mask_targets: PolygonMasks.crop_and_resize restated), the loss is the mean binary cross-entropy with logits of the row's
own class (afi_mask_loss), the predictor's backward is afi_mask_pred_bwd, and the rest of the chain runs on the conv entry points and
afi_roi_align_bwd (``_ROIMaskLossFn``; csrc/mask_loss.hip).  ``trainable_(mask_head=True)`` makes the mask head's parameters trainable.  Bitmask targets and a mask loss weight (v0.1.1 has none) are out of scope.

Kernels: afi_roi_align; the FCs and the predictor are afi_conv1x1_fwd over the R = N P rows as pixels (fc1 reads the pooled [R][S][S][C]
memory in place, its weight permuted once from [out][C][S][S] to [out][S][S][C]; cls_score and bbox_pred are ONE weight, zero-padded to a
multiple of 4; both rebuilt when a parameter changes: frozen.prepared); afi_roi_scores_boxes, afi_roi_candidates, afi_roi_nms,
afi_roi_pick (csrc/roi.hip).  No torch mm / addmm / softmax / sort / topk, MIOpen or hipBLASLt kernel runs.  ``forward_padded`` has no host
read and can be captured in a hipGraph; ``forward`` reads ``counts`` and ``truncated`` once.

The mask branch (``build_roi_heads(cfg, input_shape, masks=True)`` with MODEL.MASK_ON True; without the keyword a MASK_ON config is refused
as before), on the box branch's padded detections boxes [N, D, 4], classes [N, D], counts [N]:
  - mask pooler: a second ROIPooler (ROI_MASK_HEAD.POOLER_RESOLUTION / POOLER_SAMPLING_RATIO / POOLER_TYPE) on the PREDICTED boxes;
  - ``mask_fcn1`` .. ``mask_fcn{NUM_CONV}``: Conv2d 3x3, pad 1, bias, ReLU (frozen.conv3x3: Winograd from R S^2 >= 1024 pixels, direct below);
  - ``deconv``: ConvTranspose2d(kernel 2, stride 2) + ReLU as ONE afi_conv1x1_fwd over the prepared weight [4 Cout][Cin] (row (2a + b) Cout + co
    = deconv.weight[ci, co, a, b], the bias four times): its dense output [R][S][S][4][Cout] is the four phases of every input pixel side by
    side, and no pixel shuffle is materialised;
  - ``predictor`` (1x1 to Km = NUM_CLASSES, or 1 under CLS_AGNOSTIC_MASK) for the row's own class only, sigmoid in fp64 rounded once:
    afi_roi_mask_probs -> masks [N, D, 2S, 2S], rows past counts zero.  ``forward`` stores them as ``pred_masks`` [n, 1, 2S, 2S];
  - ``paste_masks_in_image`` (afi_mask_paste) pastes them into image-size bool masks; the extractor's postprocess calls it.
  - ``paste_masks_rle`` (afi_mask_rle_count / afi_mask_rle_emit) gives the same masks as COCO RLEs without ever forming them: the postprocess
    under ``inference(..., mask_format="rle")``; ``instances_to_coco_json`` is the evaluator's step on either form.
Keys: ``mask_head.{mask_fcn{i}, deconv, predictor}.{weight, bias}`` -- detectron2's.

``CascadeROIHeads`` (detectron2 v0.1.1's cascade_rcnn.py at inference): S = len(MODEL.ROI_BOX_CASCADE_HEAD.IOUS) stages on ONE box pooler, every
stage with its own ``box_head.{k}`` (``conv1`` .. ``conv{NUM_CONV}``: 3x3, pad 1, norm, ReLU; flatten in [C][S][S] order; ``fc1`` ..) and
``box_predictor.{k}`` (K + 1 logits, 4 class-agnostic deltas) and its own BBOX_REG_WEIGHTS[k]:
  - stage k pools its box list, runs head and predictor, and afi_roi_cascade_stage gives boxes_k = clip(apply_deltas(weights_k)) -- the next
    stage's list, no box dropped -- and the running score (s_0 + s_1 + ...) in fp32, left to right, times float32(1 / S) at the last stage:
    detectron2's ``sum(scores_per_stage) * (1.0 / S)``.  The S score tensors are never stored;
  - then fast_rcnn_inference on the mean scores and the last stage's boxes (class-agnostic), and StandardROIHeads' mask branch.
The norm of a conv (ROI_BOX_HEAD.NORM / ROI_MASK_HEAD.NORM: "", "BN", "SyncBN", "FrozenBN") is its child ``norm`` (buffers weight, bias,
running_mean, running_var; BN / SyncBN also num_batches_tracked, so an nn.SyncBatchNorm checkpoint loads with strict=True), at inference always on its running
statistics, eps 1e-5, folded into the conv in fp64 (frozen.fold_conv) and cached (frozen.prepared).  The conv head and the normed mask head are
the Cascade class's only.

``CascadeROIHeads`` in training (detectron2 v0.1.1's ``_forward_box`` with targets; opt-in: ``trainable_()`` enables it, heads on which it was
never called refuse as before): ``losses`` / ``losses_padded`` / ``forward`` in training mode with targets return ``loss_cls_stage{k}`` and
``loss_box_reg_stage{k}`` (``_CascadeBoxLossFn``).  Stage 0's training list is the parent's label / sample / gather at IOUS[0]; stage k's is
afi_roi_cascade_relabel on stage k - 1's predictor output and boxes at IOUS[k] (decode and clip as afi_roi_cascade_stage does, boxes that
clipped to empty dropped in order, the rest matched; csrc/cascade_train.hip), which is why these calls need the image sizes.  Every stage: the
box pooler, its convs as ``_train_conv`` blocks -- no norm: biased conv + ReLU; FrozenBN: the folded conv + ReLU, the weight gradient through
afi_frozen_wgrad_unfold; BN / SyncBN in training mode: the conv without bias, then afi_roi_bn_stats and afi_roi_bn_relu_fwd over the rows below
counts (the running buffers advance; the affine is a pair of parameters under ``norm.weight`` / ``norm.bias``), backward on
afi_roi_bn_relu_bwd_sums / _apply --, the FCs, the predictor and afi_roi_box_loss (class-agnostic, BBOX_REG_WEIGHTS[k]).  The features get
(1 / S) of every stage's ROIAlign backward (_ScaleGradient).  With masks=True ``loss_mask`` is computed on the foreground prefix of stage 0's
list; a normed ``mask_fcn`` chain trains through the same blocks (``_CascadeMaskLossFn``).  Refused: BN / SyncBN heads in eval mode with
targets, SyncBN under a process group of more than one rank.  ``last_assignment["stages"]`` holds every stage's list."""
import math

import torch
import torch.nn as nn

from . import _lib, ops, rle
from ._lib import AfiError
from .frozen import FROZEN_BN_EPS, FrozenBatchNorm2d, cfg_get, check_feature, conv3x3, fold_conv, prepared
from .registry import detectron2_or_local
from .rpn import SCALE_CLAMP, Boxes, Proposals, _wino

ROI_MAX_CANDIDATES = ops.ROI_MAX_CANDIDATES


ROI_HEADS_REGISTRY = detectron2_or_local("detectron2.modeling.roi_heads", "ROI_HEADS_REGISTRY", "StandardROIHeads", "ROI_HEADS")


def _check_feature(where, name, x):
    check_feature(where, name, x, "the ROI heads run")


class ROIPooler(nn.Module):
    """detectron2's ROIPooler for ``pooler_type`` ROIAlignV2 on a padded box list: one afi_roi_align over all levels."""

    def __init__(self, output_size, scales, sampling_ratio, pooler_type="ROIAlignV2", canonical_box_size=224, canonical_level=4,
                 section="ROI_BOX_HEAD"):
        super().__init__()
        if pooler_type != "ROIAlignV2":
            raise AfiError(f"roi_heads: MODEL.{section}.POOLER_TYPE {pooler_type!r} is not supported (ROIAlignV2 only)")
        if isinstance(output_size, (tuple, list)):
            if len(output_size) != 2 or output_size[0] != output_size[1]:
                raise AfiError(f"roi_heads: MODEL.{section}.POOLER_RESOLUTION {output_size} must be square")
            output_size = output_size[0]
        self.output_size, self.sampling_ratio = int(output_size), int(sampling_ratio)
        if not 0 < self.output_size <= ops.ROI_MAX_POOLED:
            raise AfiError(f"roi_heads: MODEL.{section}.POOLER_RESOLUTION {output_size} is outside 1..{ops.ROI_MAX_POOLED}")
        if self.sampling_ratio < 0:
            raise AfiError(f"roi_heads: MODEL.{section}.POOLER_SAMPLING_RATIO {sampling_ratio} must be >= 0")
        if canonical_box_size != 224 or canonical_level != 4:
            raise AfiError("roi_heads: the canonical box size / level are fixed at 224 / 4 (detectron2's defaults)")
        levels = [-math.log2(s) for s in scales]
        if not levels or len(levels) > ops.RPN_MAX_LEVELS or any(abs(l - round(l)) > 1e-9 for l in levels) \
                or any(round(b) - round(a) != 1 for a, b in zip(levels, levels[1:])) or round(levels[0]) < 0:
            raise AfiError(f"roi_heads: the strides of MODEL.ROI_HEADS.IN_FEATURES must be 1..{ops.RPN_MAX_LEVELS} consecutive powers of two, "
                           f"got scales {list(scales)}")
        self.min_level, self.max_level = int(round(levels[0])), int(round(levels[-1]))

    def forward(self, x, boxes, counts):
        """x: the levels [N, C, H_l, W_l]; boxes [N, P, 4], counts [N] int32 -> pixel-major [N P, C, S, S]."""
        if len(x) != self.max_level - self.min_level + 1:
            raise AfiError(f"roi_heads: {len(x)} feature levels for a pooler of {self.max_level - self.min_level + 1}")
        return ops.roi_align([ops.pixel_major(t) for t in x], self.min_level, boxes, counts, self.output_size, self.sampling_ratio)


HEAD_NORMS = ("", "BN", "SyncBN", "FrozenBN")


class TrackedFrozenBatchNorm2d(FrozenBatchNorm2d):
    """The frozen norm under nn.BatchNorm2d's / nn.SyncBatchNorm's keys: the four buffers and ``num_batches_tracked`` (never read)."""

    def __init__(self, num_features, eps=FROZEN_BN_EPS):
        super().__init__(num_features, eps)
        self.running_var.fill_(1.0)
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


def _check_norm(section, norm):
    if norm not in HEAD_NORMS:
        raise AfiError(f"roi_heads: MODEL.{section}.NORM {norm!r} is not supported ('', 'BN', 'SyncBN' or 'FrozenBN': a norm on its running "
                       "statistics, folded into its conv)")


def _head_norm(section, norm, channels):
    _check_norm(section, norm)
    return None if not norm else FrozenBatchNorm2d(channels) if norm == "FrozenBN" else TrackedFrozenBatchNorm2d(channels)


def _head_conv(section, cin, cout, norm):
    """detectron2's Conv2d(3x3, pad 1, bias = not norm) of a head, its norm the child ``norm``."""
    conv = nn.Conv2d(cin, cout, 3, padding=1, bias=not norm)
    if norm:
        conv.norm = _head_norm(section, norm, cout)
    return conv


def _conv_tensors(conv):
    """What a head conv's folded weight depends on: weight, bias and the norm's four tensors."""
    n = getattr(conv, "norm", None)
    return [t for t in (conv.weight, conv.bias) + ((n.weight, n.bias, n.running_mean, n.running_var) if n is not None else ()) if t is not None]


class FastRCNNConvFCHead(nn.Module):
    """detectron2's FastRCNNConvFCHead: ``fc1`` .. ``fc{NUM_FC}`` with ReLU; with convs=True (CascadeROIHeads) ``conv1`` .. ``conv{NUM_CONV}``
    (3x3, norm, ReLU) in front of them."""

    def __init__(self, input_shape, num_fc, fc_dim, num_conv=0, norm="", conv_dim=256, convs=False):
        super().__init__()
        if num_conv != 0 and not convs:
            raise AfiError(f"roi_heads: MODEL.ROI_BOX_HEAD.NUM_CONV {num_conv} is not supported (FC-only box head; the conv head is CascadeROIHeads' "
                           "and out of scope)")
        if norm and not convs:
            raise AfiError(f"roi_heads: MODEL.ROI_BOX_HEAD.NORM {norm!r} is not supported (the FC-only box head has no norm)")
        _check_norm("ROI_BOX_HEAD", norm)
        if num_conv < 0:
            raise AfiError(f"roi_heads: MODEL.ROI_BOX_HEAD.NUM_CONV {num_conv} must be >= 0")
        if num_fc < 1:
            raise AfiError(f"roi_heads: MODEL.ROI_BOX_HEAD.NUM_FC {num_fc} must be >= 1")
        if fc_dim <= 0 or fc_dim % 4:
            raise AfiError(f"roi_heads: MODEL.ROI_BOX_HEAD.FC_DIM {fc_dim} must be a positive multiple of 4")
        if convs and (conv_dim <= 0 or conv_dim % 4):
            raise AfiError(f"roi_heads: MODEL.ROI_BOX_HEAD.CONV_DIM {conv_dim} must be a positive multiple of 4")
        self.input_shape = tuple(int(s) for s in input_shape)          # (C, S, S)
        self.conv_norm_relus, self.fcs = [], []
        dim = self.input_shape[0]
        for k in range(num_conv):
            conv = _head_conv("ROI_BOX_HEAD", dim, conv_dim, norm)
            nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")          # detectron2's c2_msra_fill
            if conv.bias is not None:
                nn.init.constant_(conv.bias, 0)
            self.add_module(f"conv{k + 1}", conv)
            self.conv_norm_relus.append(conv)
            dim = conv_dim
        self.conv_output_shape = (dim, self.input_shape[1], self.input_shape[2])
        dim = dim * self.input_shape[1] * self.input_shape[2]
        for k in range(num_fc):
            fc = nn.Linear(dim, fc_dim)
            nn.init.kaiming_uniform_(fc.weight, a=1)                   # detectron2's c2_xavier_fill
            nn.init.constant_(fc.bias, 0)
            self.add_module(f"fc{k + 1}", fc)
            self.fcs.append(fc)
            dim = fc_dim
        self.output_size = dim


class FastRCNNOutputLayers(nn.Module):
    def __init__(self, input_size, num_classes, cls_agnostic_bbox_reg, box_dim=4):
        super().__init__()
        self.num_classes, self.cls_agnostic_bbox_reg = int(num_classes), bool(cls_agnostic_bbox_reg)
        self.cls_score = nn.Linear(input_size, num_classes + 1)
        self.bbox_pred = nn.Linear(input_size, (1 if cls_agnostic_bbox_reg else num_classes) * box_dim)
        nn.init.normal_(self.cls_score.weight, std=0.01)               # detectron2's initialisation
        nn.init.normal_(self.bbox_pred.weight, std=0.001)
        for l in (self.cls_score, self.bbox_pred):
            nn.init.constant_(l.bias, 0)


class MaskRCNNConvUpsampleHead(nn.Module):
    """detectron2's MaskRCNNConvUpsampleHead: ``mask_fcn1`` .. ``mask_fcn{NUM_CONV}`` (3x3, ReLU), ``deconv`` (ConvTranspose2d kernel 2,
    stride 2, ReLU), ``predictor`` (1x1 to Km classes); without norm, or with norms=True (CascadeROIHeads) a norm in every ``mask_fcn``."""

    def __init__(self, input_shape, num_classes, num_conv, conv_dim, norm="", cls_agnostic_mask=False, norms=False):
        super().__init__()
        if norm and not norms:
            raise AfiError(f"roi_heads: MODEL.ROI_MASK_HEAD.NORM {norm!r} is not supported (the mask head without norm only; the SyncBN head is "
                           "the Cascade configs' and out of scope)")
        _check_norm("ROI_MASK_HEAD", norm)
        if num_conv < 0:
            raise AfiError(f"roi_heads: MODEL.ROI_MASK_HEAD.NUM_CONV {num_conv} must be >= 0")
        if conv_dim <= 0 or conv_dim % 4:
            raise AfiError(f"roi_heads: MODEL.ROI_MASK_HEAD.CONV_DIM {conv_dim} must be a positive multiple of 4")
        self.input_shape = tuple(int(s) for s in input_shape)          # (C, S, S)
        self.num_mask_classes = 1 if cls_agnostic_mask else int(num_classes)
        self.conv_norm_relus = []
        dim = self.input_shape[0]
        for k in range(num_conv):
            conv = _head_conv("ROI_MASK_HEAD", dim, conv_dim, norm)
            self.add_module(f"mask_fcn{k + 1}", conv)
            self.conv_norm_relus.append(conv)
            dim = conv_dim
        self.deconv = nn.ConvTranspose2d(dim, conv_dim, 2, stride=2, padding=0)
        self.predictor = nn.Conv2d(conv_dim, self.num_mask_classes, 1)
        for l in self.conv_norm_relus + [self.deconv]:                 # detectron2's c2_msra_fill
            nn.init.kaiming_normal_(l.weight, mode="fan_out", nonlinearity="relu")
            if l.bias is not None:
                nn.init.constant_(l.bias, 0)
        nn.init.normal_(self.predictor.weight, std=0.001)
        nn.init.constant_(self.predictor.bias, 0)


def deconv_as_conv1x1(weight, bias):
    """ConvTranspose2d(kernel 2, stride 2) parameters (weight [Cin, Cout, 2, 2]) as the 1x1 conv that writes the four output phases of an
    input pixel side by side: ([4 Cout, Cin] with row (2a + b) Cout + co = weight[ci, co, a, b], the bias four times)."""
    cin, cout = weight.shape[:2]
    return weight.detach().float().permute(2, 3, 1, 0).reshape(4 * cout, cin).contiguous(), bias.detach().float().repeat(4).contiguous()


class Detections:
    """One image's detections when detectron2's Instances is not importable: ``image_size``, ``pred_boxes``, ``scores``, ``pred_classes`` and,
    from the mask branch, ``pred_masks`` (else None) or, at the extractor's ``mask_format="rle"``, ``pred_masks_rle``."""

    def __init__(self, image_size, pred_boxes, scores, pred_classes, pred_masks=None, pred_masks_rle=None):
        self.image_size, self.pred_boxes, self.scores, self.pred_classes = image_size, pred_boxes, scores, pred_classes
        self.pred_masks = pred_masks
        self.pred_masks_rle = pred_masks_rle             # a list of COCO RLE dicts (host data) from inference(..., mask_format="rle")

    def __len__(self):
        return len(self.pred_boxes)

    def to(self, device):
        return Detections(self.image_size, self.pred_boxes.to(device), self.scores.to(device), self.pred_classes.to(device),
                          self.pred_masks.to(device) if self.pred_masks is not None else None, self.pred_masks_rle)


def _make_detections(image_size, boxes, scores, classes, masks=None):
    try:
        from detectron2.structures import Boxes as D2Boxes, Instances
    except Exception:
        return Detections(tuple(image_size), Boxes(boxes), scores, classes, masks)
    r = Instances(tuple(image_size))
    r.pred_boxes = D2Boxes(boxes)
    r.scores = scores
    r.pred_classes = classes
    if masks is not None:
        r.pred_masks = masks
    return r


def paste_masks_in_image(masks, boxes, image_shape, threshold=0.5):
    """detectron2's paste_masks_in_image on the GPU: masks [R, M, M] (or [R, 1, M, M]) fp32 probabilities, boxes [R, 4] or Boxes, image_shape
    (H, W) -> bool [R, H, W] (afi_mask_paste; pixels whose centre is outside their box are False)."""
    boxes = boxes.tensor if hasattr(boxes, "tensor") else boxes
    if not torch.is_tensor(masks) or not torch.is_tensor(boxes) or not masks.is_cuda or not boxes.is_cuda:
        raise AfiError("paste_masks_in_image: masks and boxes must be GPU tensors; the paste runs on the GPU only, there is no CPU fallback")
    if masks.dim() == 4 and masks.shape[1] == 1:
        masks = masks[:, 0]
    return ops.mask_paste(masks, boxes.reshape(-1, 4), image_shape, threshold)


def paste_masks_rle(masks, boxes, image_shape, threshold=0.5):
    """paste_masks_in_image's masks as COCO RLEs, without the image-size masks: a list of R ``{"size": [H, W], "counts": str}``, what
    pycocotools' ``encode`` gives for each pasted mask (afi_mask_rle_count / afi_mask_rle_emit find the runs on the GPU from the pixels inside
    each box; the host only turns the run starts into strings: rle.py).  Same inputs as paste_masks_in_image, same refusals."""
    boxes = boxes.tensor if hasattr(boxes, "tensor") else boxes
    if not torch.is_tensor(masks) or not torch.is_tensor(boxes) or not masks.is_cuda or not boxes.is_cuda:
        raise AfiError("paste_masks_rle: masks and boxes must be GPU tensors; the paste runs on the GPU only, there is no CPU fallback")
    if masks.dim() == 4 and masks.shape[1] == 1:
        masks = masks[:, 0]
    hw = (int(image_shape[0]), int(image_shape[1]))
    starts, nstarts = ops.mask_paste_rle(masks, boxes.reshape(-1, 4), hw, threshold)
    strings = rle.to_strings(rle.counts_from_starts(starts.cpu().numpy(), nstarts.numpy(), hw))
    return [{"size": [hw[0], hw[1]], "counts": s} for s in strings]


def instances_to_coco_json(instances, img_id):
    """One image's detections (``Detections`` or detectron2 ``Instances``, postprocessed) as COCO result dicts, the reference evaluator's
    function: ``image_id``, ``category_id``, ``bbox`` (XYWH), ``score`` and, with masks, ``segmentation`` = an RLE with a str ``counts`` --
    ``pred_masks_rle`` as it is when present (inference(..., mask_format="rle")), else bool ``pred_masks`` copied to the host and encoded there
    one mask at a time (rle.encode: the slow path, kept for parity).  Keypoints are refused."""
    def field(name):
        if hasattr(instances, "has") and hasattr(instances, "get"):       # detectron2's Instances
            return instances.get(name) if instances.has(name) else None
        return getattr(instances, name, None)
    n = len(instances)
    if n == 0:
        return []
    if field("pred_keypoints") is not None:
        raise AfiError("instances_to_coco_json: `pred_keypoints` are not supported (the keypoint branch is out of scope)")
    boxes = field("pred_boxes")
    b = (boxes.tensor if hasattr(boxes, "tensor") else boxes).detach().cpu().double()
    xywh = torch.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).tolist()
    scores, classes = field("scores").tolist(), field("pred_classes").tolist()
    segs = field("pred_masks_rle")
    if segs is None and field("pred_masks") is not None:
        m = field("pred_masks")
        if m.dim() != 3 or m.dtype != torch.bool:
            raise AfiError(f"instances_to_coco_json: bool `pred_masks` [n, H, W] expected (postprocessed instances), got {m.dtype} "
                           f"{tuple(m.shape)}")
        m = m.cpu().numpy()
        segs = [rle.to_rle(rle.encode(x), x.shape) for x in m]
    if segs is not None and len(segs) != n:
        raise AfiError(f"instances_to_coco_json: {len(segs)} masks for {n} instances")
    out = []
    for k in range(n):
        d = {"image_id": img_id, "category_id": classes[k], "bbox": xywh[k], "score": scores[k]}
        if segs is not None:
            d["segmentation"] = segs[k]
        out.append(d)
    return out


def _rows_as_pixels(t2d):
    """A dense [R, C] matrix as the pixel-major [1, C, 1, R] tensor afi_conv1x1_fwd reads: one row per pixel, no copy."""
    R, C_ = t2d.shape
    return t2d.view(1, 1, R, C_).permute(0, 3, 1, 2)


def _pixels_as_rows(t):
    """The dense pixel-major [1, C, 1, R] output of afi_conv1x1_fwd as its [R, C] matrix, no copy."""
    return t.permute(0, 2, 3, 1).reshape(t.shape[3], t.shape[1])


def _reg_weights(key, w):
    try:
        out = tuple(float(v) for v in w)
    except TypeError:
        out = (w,)
    if len(out) != 4 or not min(out) > 0:
        raise AfiError(f"roi_heads: {key} {out} must be four positive numbers")
    return out


class _ROIBoxLossFn(torch.autograd.Function):
    """(loss_cls, loss_box_reg) of the features and the parameters of the FCs and the predictor.  Forward: afi_roi_label, afi_rpn_sample,
    afi_roi_gather_samples, then the pooler and ``_run_head`` -- the very kernels inference runs -- on the sampled boxes, then afi_roi_box_loss,
    which also leaves d loss / d predictor output.  Backward: the two upstream scalars as one per-column multiply of that gradient;
    afi_conv1x1_dgrad / afi_conv1x1_wgrad and the bias column sums for the predictor and every FC, afi_relu_bwd between them (cls_score /
    bbox_pred split back out of the concatenated weight, fc1's weight gradient permuted from [out][S][S][C] back to [out][C S S]); then
    afi_roi_align_bwd.  Proposals, labels and regression targets are not differentiable."""
    NARGS = 8                              # the non-differentiable leading arguments of forward

    @staticmethod
    @_lib.ctx_forward
    def forward(ctx, heads, pboxes, pcounts, gt, gcls, gcounts, keys, nlev, *ts):
        xs = [ops.pixel_major(x.detach()) for x in ts[:nlev]]
        head, pr, pool = heads.box_head, heads.box_predictor, heads.box_pooler
        K, B = heads.num_classes, heads.batch_size_per_image
        labels, midx = ops.roi_label(pboxes, pcounts, gt, gcounts, heads.iou_threshold, heads.proposal_append_gt)
        if keys is None:                                     # every 32-bit pattern equally likely, from torch's generator for this device
            keys = torch.randint(-2 ** 31, 2 ** 31, labels.shape, device=labels.device, dtype=torch.int32)
        labels, sidx, n_pos, n_neg = ops.rpn_sample(labels, keys, B, heads.positive_fraction)
        boxes, counts, cls, gboxes = ops.roi_gather_samples(pboxes, pcounts, gt, gcls, gcounts, midx, sidx, n_pos, n_neg, K,
                                                            heads.proposal_append_gt)
        pooled = pool(xs, boxes, counts)
        w1, wp, bp = heads._prepare()
        pred, _, acts = heads._run_head(head, [], (w1, wp, bp), pooled)
        loss, dpred = ops.roi_box_loss(pred, K, pr.cls_agnostic_bbox_reg, boxes, counts, cls, gboxes, heads.box_weights, heads.smooth_l1_beta)
        ctx.save_for_backward(w1, wp, *[fc.weight.detach() for fc in head.fcs[1:]], pooled, *acts, dpred, boxes, counts)
        ctx.nlev, ctx.nfc, ctx.nc, ctx.nb = nlev, len(head.fcs), pr.cls_score.weight.shape[0], pr.bbox_pred.weight.shape[0]
        ctx.level_shapes, ctx.min_level, ctx.sampling_ratio = [tuple(x.shape[2:]) for x in xs], pool.min_level, pool.sampling_ratio
        heads.last_assignment = {"labels": labels, "matched_idx": midx, "sampled_idx": sidx, "n_pos": n_pos, "n_neg": n_neg, "boxes": boxes,
                                 "counts": counts, "gt_classes": cls, "gt_boxes": gboxes, "pred": pred}
        return loss[0], loss[1]

    @staticmethod
    @_lib.ctx_backward
    def backward(ctx, dcls, dbox):
        sv, L, F, nc, nb = ctx.saved_tensors, ctx.nlev, ctx.nfc, ctx.nc, ctx.nb
        w1, wp, fcw = sv[0], sv[1], sv[2:1 + F]
        pooled, acts = sv[1 + F], sv[2 + F:2 + 2 * F]
        dpred, boxes, counts = sv[2 + 2 * F:]
        na = _ROIBoxLossFn.NARGS
        need = ctx.needs_input_grad
        need_x, need_w = any(need[na:na + L]), any(need[na + L:])
        R, Cp = dpred.shape
        dev = dpred.device
        # the kernel left d loss_cls / d logit in columns 0..K and d loss_box_reg / d delta behind them: the two upstream scalars, per column
        s = torch.zeros(Cp, device=dev, dtype=torch.float32)
        s[:nc], s[nc:nc + nb] = dcls.float(), dbox.float()
        g = _rows_as_pixels(dpred * s)
        x0 = pooled.permute(0, 2, 3, 1).reshape(R, -1)                      # fc1's input rows, in the pooled memory's [S][S][C] order
        ins = [_rows_as_pixels(x0)] + [_rows_as_pixels(a) for a in acts]    # ins[k]: the input of FC k; ins[F]: the predictor's
        dx, fgrads, pgrads = _fc_chain_backward(g, ins, w1, wp, fcw, (pooled.shape[1], pooled.shape[2]), nc, nb, need_w, need_x)
        dxs = [None] * L
        if need_x:
            C_, S = pooled.shape[1], pooled.shape[2]
            dpooled = _pixels_as_rows(dx).view(R, S, S, C_).permute(0, 3, 1, 2)
            dxs = ops.roi_align_bwd(dpooled, ctx.level_shapes, ctx.min_level, boxes, counts, ctx.sampling_ratio)
            dxs = [d if n else None for d, n in zip(dxs, need[na:na + L])]
        h = fgrads + pgrads if need_w else [None] * (2 * F + 4)
        return (*[None] * na, *dxs, *[v if n else None for v, n in zip(h, need[na + L:])])


class _ROIMaskLossFn(torch.autograd.Function):
    """loss_mask of the features and the mask head's parameters, on the foreground prefix of the training list ``_ROIBoxLossFn`` left in
    ``heads.last_assignment`` (one label / sample / gather for both branches).  Forward: afi_mask_targets, then the mask pooler, the 3x3 convs
    and the deconv as one 1x1 conv -- the very chain inference runs --, then afi_mask_loss, which also leaves d loss / d logit.  Backward: the
    upstream scalar as one multiply of that gradient; afi_mask_pred_bwd (dh already carries the deconv's ReLU mask); the deconv on
    afi_conv1x1_wgrad / afi_conv1x1_dgrad over the prepared [4 Cout][Cin] weight (its gradient permuted back to [Cin][Cout][2][2], its bias
    gradient summed over the four phases); afi_relu_bwd and the 3x3 wgrad / dgrad of every ``mask_fcn`` in the regime its forward ran in;
    then afi_roi_align_bwd at the mask pooler's resolution.  Targets and boxes are not differentiable."""
    NARGS = 5                              # the non-differentiable leading arguments of forward

    @staticmethod
    @_lib.ctx_forward
    def forward(ctx, heads, polys, gcounts, gmax, nlev, *ts):
        xs = [ops.pixel_major(x.detach()) for x in ts[:nlev]]
        a, pool, Bf = heads.last_assignment, heads.mask_pooler, heads.mask_batch_per_image
        tg, cfg_ = ops.mask_targets(*polys, a["boxes"], a["sampled_idx"], a["matched_idx"], gcounts, gmax, a["n_pos"], Bf, 2 * pool.output_size)
        boxes = a["boxes"][:, :Bf].contiguous()         # the pooler reads a dense list: N Bf 16 bytes, on the device
        cls = a["gt_classes"][:, :Bf]                   # read in place, with the list's row stride
        pooled = pool(xs, boxes, cfg_)
        convs, (wd, bd), (wp, bp) = heads._prepare_mask()
        x, acts = pooled, []
        for wb in convs:
            x = conv3x3(x, wb, relu=True)
            acts.append(x)
        h = ops.conv1x1_fwd(x, wd, bd, act=2)
        loss, dz = ops.mask_loss(h, wp, bp, cls, cfg_, tg)
        ctx.save_for_backward(wd, wp, *[wb[0] for wb in convs], pooled, *acts, h, dz, boxes, cfg_, cls)
        ctx.nlev, ctx.nconv = nlev, len(convs)
        ctx.level_shapes, ctx.min_level, ctx.sampling_ratio = [tuple(x.shape[2:]) for x in xs], pool.min_level, pool.sampling_ratio
        a.update(mask_targets=tg, counts_fg=cfg_, mask_boxes=boxes, mask_deconv=h, mask_dz=dz)
        return loss[0]

    @staticmethod
    @_lib.ctx_backward
    def backward(ctx, dloss):
        sv, L, F = ctx.saved_tensors, ctx.nlev, ctx.nconv
        wd, wp, cw = sv[0], sv[1], sv[2:2 + F]
        pooled, acts = sv[2 + F], sv[3 + F:3 + 2 * F]
        h, dz, boxes, cfg_, cls = sv[3 + 2 * F:]
        na = _ROIMaskLossFn.NARGS
        need = ctx.needs_input_grad
        need_x, need_w = any(need[na:na + L]), any(need[na + L:])
        ins = [pooled] + list(acts)                                          # ins[k]: the input of mask_fcn k + 1; ins[F]: the deconv's
        dh, dwp, dbp = ops.mask_pred_bwd(h, dz * dloss.float(), wp, cls, cfg_)
        cgrads, dgrads = [], []
        if need_w:
            cout, cin = wd.shape[0] // 4, wd.shape[1]
            dwd = ops.conv1x1_wgrad(dh, ins[F]).view(2, 2, cout, cin).permute(3, 2, 0, 1)       # row (2a + b) Cout + co, column ci
            dgrads = [dwd, ops.bias_grad(dh).view(4, cout).sum(0)]
        dx = ops.conv1x1_dgrad(dh, wd) if F > 0 or need_x else None
        for k in reversed(range(F)):
            du = ops.relu_bwd(dx, ins[k + 1])
            wino = _wino(ins[k], du.shape[1])
            if need_w:
                cgrads = [(ops.conv3x3_wino_wgrad if wino else ops.conv3x3_wgrad)(du, ins[k]), ops.bias_grad(du)] + cgrads
            if k > 0 or need_x:
                dx = (ops.conv3x3_wino_dgrad if wino else ops.conv3x3_dgrad)(du, cw[k])
        dxs = [None] * L
        if need_x:
            dxs = ops.roi_align_bwd(dx, ctx.level_shapes, ctx.min_level, boxes, cfg_, ctx.sampling_ratio)
            dxs = [d if n else None for d, n in zip(dxs, need[na:na + L])]
        g = cgrads + dgrads + [dwp.view(dwp.shape[0], -1, 1, 1), dbp] if need_w else [None] * (2 * F + 4)
        return (*[None] * na, *dxs, *[v if n else None for v, n in zip(g, need[na + L:])])


def _fc_chain_backward(g, ins, w1, wp, fcw, pooled_shape, nc, nb, need_w, need_x):
    """The backward of ``_run_head``'s FCs and predictor, shared by ``_ROIBoxLossFn`` and ``_CascadeBoxLossFn``: g = d loss / d predictor output as pixels, ins[k] the
    input rows of FC k (ins[F]: the predictor's) as pixels.  Returns (d loss / d the rows fc1 read, as pixels, or None; the FCs' [weight, bias]
    gradients, fc1's back in [out][C][S][S] order; the predictor's four)."""
    F, R, dev = len(ins) - 1, g.shape[3], g.device

    def layer_grads(dy, x):
        cout, cin = dy.shape[1], x.shape[1]
        dw = torch.zeros((cout, cin), device=dev, dtype=torch.float32)
        _lib.call("afi_conv1x1_wgrad", ops.view_of(dy), ops.view_of(x), 1, 1, R, cout, cin, ops._p(dw), 1.0, ops.stream_ptr())
        db = torch.zeros((cout,), device=dev, dtype=torch.float32)
        ops.colsum_accum(_pixels_as_rows(dy), db)
        return dw, db
    pgrads, fgrads = [], []
    if need_w:
        dwp, dbp = layer_grads(g, ins[F])
        pgrads = [dwp[:nc], dbp[:nc], dwp[nc:nc + nb], dbp[nc:nc + nb]]
    dx = ops.conv1x1_dgrad(g, wp)
    for k in reversed(range(F)):
        du = ops.relu_bwd(dx, ins[k + 1])
        if need_w:
            dw, db = layer_grads(du, ins[k])
            if k == 0:
                C_, S = pooled_shape
                dw = dw.view(-1, S, S, C_).permute(0, 3, 1, 2).reshape(dw.shape[0], -1)
            fgrads = [dw, db] + fgrads
        dx = ops.conv1x1_dgrad(du, fcw[k - 1] if k > 0 else w1) if k > 0 or need_x else None
    return dx, fgrads, pgrads


def _train_convs_backward(dx, kinds, ct, x0, counts, slots, pgrads, need_w, need_x):
    """The backward of a chain of ``CascadeROIHeads._train_conv`` blocks on the padded rows: dx = d loss / d the last block's output, kinds[i] /
    ct[i] what block i's forward kept, x0 the chain's input, slots[i] where block i's parameter gradients go in `pgrads`.  Per block: the
    ReLU mask (no norm, FrozenBN) or the two list-masked BatchNorm halves over the rows below counts, then the 3x3 weight and data gradients
    in the forward's regime; the FrozenBN weight gradient goes through afi_frozen_wgrad_unfold.  Returns d loss / d x0 (None unless need_x)."""
    for i in reversed(range(len(ct))):
        kind, tt, slot = kinds[i], ct[i], slots[i]
        xin = ct[i - 1][0] if i > 0 else x0
        if kind == "bn":
            y, u, mean, invstd, gamma, w = tt
            dgamma, dbeta = torch.zeros_like(mean), torch.zeros_like(mean)
            sums = ops.roi_bn_relu_bwd_sums(dx, u, y, counts, mean, invstd, dgamma, dbeta)
            du = ops.roi_bn_relu_bwd_apply(dx, u, y, counts, mean, invstd, gamma, sums)
            if need_w:
                pgrads[slot["gamma"]], pgrads[slot["beta"]] = dgamma, dbeta
        else:
            y, w = tt[0], tt[1]
            du = ops.relu_bwd(dx, y)
        wino = _wino(xin, du.shape[1])
        if need_w:
            dw = (ops.conv3x3_wino_wgrad if wino else ops.conv3x3_wgrad)(du, xin)
            if kind == "frozen":                                        # the gradient of the FOLDED weight: back to the parameter's
                gw = torch.zeros(dw.shape, device=dw.device, dtype=torch.float32)
                ops.frozen_wgrad_unfold([(dw, gw, tt[2])])
                dw = gw
            pgrads[slot["weight"]] = dw
            if slot["bias"] is not None:
                pgrads[slot["bias"]] = ops.bias_grad(du)
        dx = (ops.conv3x3_wino_dgrad if wino else ops.conv3x3_dgrad)(du, w) if i > 0 or need_x else None
    return dx


class _CascadeMaskLossFn(torch.autograd.Function):
    """``_ROIMaskLossFn`` for a mask head whose ``mask_fcn`` convs carry a norm (CascadeROIHeads: ROI_MASK_HEAD.NORM "BN" / "SyncBN" /
    "FrozenBN"): the same targets, pooler, deconv, loss and predictor backward on the foreground prefix of stage 0's training list; the convs
    run as ``CascadeROIHeads._train_conv`` blocks, the list-masked BatchNorm passes over the rows below counts_fg at 14 x 14 pixels a row."""
    NARGS = 5

    @staticmethod
    @_lib.ctx_forward
    def forward(ctx, heads, polys, gcounts, gmax, nlev, *ts):
        xs = [ops.pixel_major(x.detach()) for x in ts[:nlev]]
        a, pool, Bf, mh = heads.last_assignment, heads.mask_pooler, heads.mask_batch_per_image, heads.mask_head
        tg, cfg_ = ops.mask_targets(*polys, a["boxes"], a["sampled_idx"], a["matched_idx"], gcounts, gmax, a["n_pos"], Bf, 2 * pool.output_size)
        boxes = a["boxes"][:, :Bf].contiguous()
        cls = a["gt_classes"][:, :Bf]
        pooled = pool(xs, boxes, cfg_)
        _, (wd, bd), (wp, bp) = heads._prepare_mask()
        x, recs = pooled, []
        for i, conv in enumerate(mh.conv_norm_relus):
            x, rec = heads._train_conv(f"m{i}", conv, x, cfg_, lambda i=i: heads._prepare_mask()[0][i])
            recs.append(rec)
        h = ops.conv1x1_fwd(x, wd, bd, act=2)
        loss, dz = ops.mask_loss(h, wp, bp, cls, cfg_, tg)
        ctx.save_for_backward(wd, wp, pooled, h, dz, boxes, cfg_, cls, *[t for r in recs for t in r["tensors"]])
        ctx.kinds, ctx.nts, ctx.nlev, ctx.layout = [r["kind"] for r in recs], [len(r["tensors"]) for r in recs], nlev, heads._mask_layout
        ctx.level_shapes, ctx.min_level, ctx.sampling_ratio = [tuple(x.shape[2:]) for x in xs], pool.min_level, pool.sampling_ratio
        a.update(mask_targets=tg, counts_fg=cfg_, mask_boxes=boxes, mask_deconv=h, mask_dz=dz)
        return loss[0]

    @staticmethod
    @_lib.ctx_backward
    def backward(ctx, dloss):
        sv, L, na = ctx.saved_tensors, ctx.nlev, _CascadeMaskLossFn.NARGS
        wd, wp, pooled, h, dz, boxes, cfg_, cls = sv[:8]
        ct, pos = [], 8
        for n in ctx.nts:
            ct.append(sv[pos:pos + n])
            pos += n
        need = ctx.needs_input_grad
        need_x, need_w = any(need[na:na + L]), any(need[na + L:])
        lay = ctx.layout
        pgrads = [None] * (len(need) - na - L)
        x_last = ct[-1][0] if ct else pooled
        dh, dwp, dbp = ops.mask_pred_bwd(h, dz * dloss.float(), wp, cls, cfg_)
        if need_w:
            cout, cin = wd.shape[0] // 4, wd.shape[1]
            pgrads[lay["deconv"][0]] = ops.conv1x1_wgrad(dh, x_last).view(2, 2, cout, cin).permute(3, 2, 0, 1)
            pgrads[lay["deconv"][1]] = ops.bias_grad(dh).view(4, cout).sum(0)
            pgrads[lay["pred"][0]], pgrads[lay["pred"][1]] = dwp.view(dwp.shape[0], -1, 1, 1), dbp
        dx = ops.conv1x1_dgrad(dh, wd) if ct or need_x else None
        dx = _train_convs_backward(dx, ctx.kinds, ct, pooled, cfg_, lay["conv"], pgrads, need_w, need_x)
        dxs = [None] * L
        if need_x:
            dxs = ops.roi_align_bwd(dx, ctx.level_shapes, ctx.min_level, boxes, cfg_, ctx.sampling_ratio)
            dxs = [d if n else None for d, n in zip(dxs, need[na:na + L])]
        return (*[None] * na, *dxs, *[v if n else None for v, n in zip(pgrads, need[na + L:])])


class _CascadeBoxLossFn(torch.autograd.Function):
    """(loss_cls_stage0, loss_box_reg_stage0, ...) of the features and every stage's parameters: detectron2 v0.1.1's
    CascadeROIHeads._forward_box in training.  Forward, per stage: stage 0's training list is the parent's label / sample / gather at IOUS[0],
    stage k > 0's is afi_roi_cascade_relabel on stage k - 1's predictor output and boxes at IOUS[k]; then the box pooler, the conv-norm-ReLU
    chain (``heads._train_conv``), the FCs and the predictor, and afi_roi_box_loss (class-agnostic, BBOX_REG_WEIGHTS[k]) over the stage's own
    rows.  Backward, per stage: ``_fc_chain_backward``, the convs' backward in the forward's regime (ReLU mask or the list-masked BatchNorm
    halves; the FrozenBN weight gradient through afi_frozen_wgrad_unfold), afi_roi_align_bwd of (1 / S) d pooled (detectron2's _ScaleGradient),
    summed over the stages.  Boxes, labels and targets are not differentiable."""
    NARGS = 9

    @staticmethod
    @_lib.ctx_forward
    def forward(ctx, heads, pboxes, pcounts, gt, gcls, gcounts, keys, image_hw, nlev, *ts):
        xs = [ops.pixel_major(x.detach()) for x in ts[:nlev]]
        pool, K, B, S_ = heads.box_pooler, heads.num_classes, heads.batch_size_per_image, heads.num_stages
        saved, meta, losses, stages = [], [], [], []
        boxes = counts = pred = None
        for k in range(S_):
            head, pr = heads.box_head[k], heads.box_predictor[k]
            if k == 0:
                labels, midx = ops.roi_label(pboxes, pcounts, gt, gcounts, heads.stage_ious[0], heads.proposal_append_gt)
                if keys is None:
                    keys = torch.randint(-2 ** 31, 2 ** 31, labels.shape, device=labels.device, dtype=torch.int32)
                labels, sidx, n_pos, n_neg = ops.rpn_sample(labels, keys, B, heads.positive_fraction)
                boxes, counts, cls, gboxes = ops.roi_gather_samples(pboxes, pcounts, gt, gcls, gcounts, midx, sidx, n_pos, n_neg, K,
                                                                    heads.proposal_append_gt)
                first = {"labels": labels, "matched_idx": midx, "sampled_idx": sidx, "n_pos": n_pos, "n_neg": n_neg}
                st = {"src": None, "matched_idx": None}
            else:
                r = ops.roi_cascade_relabel(pred, K, boxes, counts, image_hw, heads.stage_weights[k - 1], gt, gcls, gcounts, heads.stage_ious[k],
                                            SCALE_CLAMP)
                boxes, counts, cls, gboxes = r["boxes"], r["counts"], r["gt_classes"], r["gt_boxes"]
                st = {"src": r["src"], "matched_idx": r["matched_idx"]}
            pooled = pool(xs, boxes, counts)
            x, convs = pooled, []
            for i, conv in enumerate(head.conv_norm_relus):
                x, rec = heads._train_conv(f"{k}_{i}", conv, x, counts, lambda k=k, i=i, head=head: heads._prepare_convs(head, f"prep_convs{k}")[i])
                convs.append(rec)
            w1, wp, bp = heads._prepare_head(head, pr, f"prep{k}")
            pred, _, acts = heads._run_head(head, [], (w1, wp, bp), x)
            loss, dpred = ops.roi_box_loss(pred, K, True, boxes, counts, cls, gboxes, heads.stage_weights[k], heads.smooth_l1_beta)
            losses += [loss[0], loss[1]]
            t = [w1, wp, *[fc.weight.detach() for fc in head.fcs[1:]], pooled, *acts, dpred, boxes, counts]
            for rec in convs:
                t += rec["tensors"]
            meta.append({"at": len(saved), "n": len(t), "nfc": len(head.fcs), "nc": pr.cls_score.weight.shape[0], "nb": pr.bbox_pred.weight.shape[0],
                         "convs": [{"kind": rec["kind"], "nt": len(rec["tensors"])} for rec in convs]})
            saved += t
            st.update(boxes=boxes, counts=counts, gt_classes=cls, gt_boxes=gboxes, pred=pred)
            stages.append(st)
        ctx.save_for_backward(*saved)
        ctx.meta, ctx.nlev, ctx.layout = meta, nlev, heads._train_layout
        ctx.level_shapes, ctx.min_level, ctx.sampling_ratio = [tuple(x.shape[2:]) for x in xs], pool.min_level, pool.sampling_ratio
        s0 = stages[0]
        heads.last_assignment = dict(first, boxes=s0["boxes"], counts=s0["counts"], gt_classes=s0["gt_classes"], gt_boxes=s0["gt_boxes"], pred=s0["pred"],
                                     stages=stages)
        return tuple(losses)

    @staticmethod
    @_lib.ctx_backward
    def backward(ctx, *dlosses):
        sv, L, na = ctx.saved_tensors, ctx.nlev, _CascadeBoxLossFn.NARGS
        need = ctx.needs_input_grad
        need_x = any(need[na:na + L])
        S_ = len(ctx.meta)
        pgrads = [None] * (len(need) - na - L)
        dxs = None
        for k, m in enumerate(ctx.meta):
            t = sv[m["at"]:m["at"] + m["n"]]
            F = m["nfc"]
            w1, wp, fcw, pooled, acts = t[0], t[1], t[2:1 + F], t[1 + F], t[2 + F:2 + 2 * F]
            dpred, boxes, counts = t[2 + 2 * F:5 + 2 * F]
            ct, pos = [], 5 + 2 * F
            for c in m["convs"]:
                ct.append(t[pos:pos + c["nt"]])
                pos += c["nt"]
            lay = ctx.layout[k]
            need_w = any(need[na + L + i] for i in lay["all"])
            nc, nb = m["nc"], m["nb"]
            s = torch.zeros(dpred.shape[1], device=dpred.device, dtype=torch.float32)
            s[:nc], s[nc:nc + nb] = dlosses[2 * k].float(), dlosses[2 * k + 1].float()
            g = _rows_as_pixels(dpred * s)
            R = dpred.shape[0]
            x_last = ct[-1][0] if ct else pooled                               # what fc1 read: the last conv's output, or the pooled features
            C_, S = x_last.shape[1], x_last.shape[2]
            ins = [_rows_as_pixels(x_last.permute(0, 2, 3, 1).reshape(R, -1))] + [_rows_as_pixels(a) for a in acts]
            dx, fgrads, prg = _fc_chain_backward(g, ins, w1, wp, fcw, (C_, S), nc, nb, need_w, need_x or bool(ct))
            if need_w:
                for i, v in zip(lay["fc"] + lay["pred"], fgrads + prg):
                    pgrads[i] = v
            if dx is not None:
                dx = _pixels_as_rows(dx).view(R, S, S, C_).permute(0, 3, 1, 2)
            dx = _train_convs_backward(dx, [c["kind"] for c in m["convs"]], ct, pooled, counts, lay["conv"], pgrads, need_w, need_x)
            if need_x:
                d = ops.roi_align_bwd(dx * (1.0 / S_), ctx.level_shapes, ctx.min_level, boxes, counts, ctx.sampling_ratio)
                dxs = d if dxs is None else [a + b for a, b in zip(dxs, d)]
        dxs = [d if n else None for d, n in zip(dxs, need[na:na + L])] if need_x else [None] * L
        return (*[None] * na, *dxs, *[v if n else None for v, n in zip(pgrads, need[na + L:])])


def _make_sampled(image_size, boxes, gt_classes, gt_boxes):
    """One image's sampled proposals in training: ``proposal_boxes``, ``gt_classes`` (int64, NUM_CLASSES = background) and ``gt_boxes``."""
    try:
        from detectron2.structures import Boxes as D2Boxes, Instances
    except Exception:
        r = Proposals(tuple(image_size), Boxes(boxes), None)
        r.gt_classes, r.gt_boxes = gt_classes, Boxes(gt_boxes)
        return r
    r = Instances(tuple(image_size))
    r.proposal_boxes = D2Boxes(boxes)
    r.gt_classes = gt_classes
    r.gt_boxes = D2Boxes(gt_boxes)
    return r


def _target_field(t, name):
    v = t.get(name) if isinstance(t, dict) else getattr(t, name, None)
    return getattr(v, "tensor", v)


@ROI_HEADS_REGISTRY.register()
class StandardROIHeads(nn.Module):
    conv_norm_heads = False           # the conv box head and the normed mask head: CascadeROIHeads only

    def _refuse_name(self, name):
        return AfiError(f"roi_heads: MODEL.ROI_HEADS.NAME {name!r} is not supported (StandardROIHeads only; CascadeROIHeads is out of scope)")

    def __init__(self, cfg, input_shape, masks=False):
        super().__init__()
        m = cfg.MODEL
        rh, bh = cfg_get(m, "ROI_HEADS", None), cfg_get(m, "ROI_BOX_HEAD", None)
        if rh is None or bh is None:
            raise AfiError("roi_heads: the config has no MODEL.ROI_HEADS / MODEL.ROI_BOX_HEAD section (afigan_amd.config.get_cfg declares them)")
        if cfg_get(rh, "NAME", "StandardROIHeads") != type(self).__name__:
            raise self._refuse_name(rh.NAME)
        if masks and not cfg_get(m, "MASK_ON", False):
            raise AfiError("roi_heads: masks=True builds the mask branch and needs MODEL.MASK_ON True")
        if cfg_get(m, "MASK_ON", False) and not masks:
            raise AfiError("roi_heads: MODEL.MASK_ON is set -- box branch only; set MODEL.MASK_ON False, or build the mask branch as well with "
                           "build_roi_heads(cfg, input_shape, masks=True)")
        if cfg_get(m, "KEYPOINT_ON", False):
            raise AfiError("roi_heads: MODEL.KEYPOINT_ON is set -- box branch only; set MODEL.KEYPOINT_ON False")
        if cfg_get(bh, "NAME", "FastRCNNConvFCHead") != "FastRCNNConvFCHead":
            raise AfiError(f"roi_heads: MODEL.ROI_BOX_HEAD.NAME {bh.NAME!r} is not supported (FastRCNNConvFCHead only)")
        self.in_features = list(rh.IN_FEATURES)
        missing = [f for f in self.in_features if f not in input_shape]
        if missing or not self.in_features:
            raise AfiError(f"roi_heads: MODEL.ROI_HEADS.IN_FEATURES {self.in_features} are not all outputs of the backbone ({sorted(input_shape)})")
        shapes = [input_shape[f] for f in self.in_features]
        channels = {s.channels for s in shapes}
        if len(channels) != 1:
            raise AfiError(f"roi_heads: every feature of MODEL.ROI_HEADS.IN_FEATURES must have one channel count, got {sorted(channels)}")
        C_ = self.channels = channels.pop()
        if C_ % 4:
            raise AfiError(f"roi_heads: {C_} feature channels; a multiple of 4 is needed")
        self.num_classes = int(cfg_get(rh, "NUM_CLASSES", 80))
        if not 0 < self.num_classes <= ops.ROI_MAX_CLASSES:
            raise AfiError(f"roi_heads: MODEL.ROI_HEADS.NUM_CLASSES {self.num_classes} is outside 1..{ops.ROI_MAX_CLASSES}")
        self.test_score_thresh = float(cfg_get(rh, "SCORE_THRESH_TEST", 0.05))
        self.test_nms_thresh = float(cfg_get(rh, "NMS_THRESH_TEST", 0.5))
        self.test_detections_per_img = int(cfg_get(cfg_get(cfg, "TEST", None), "DETECTIONS_PER_IMAGE", 100))
        if not 0 < self.test_detections_per_img <= ROI_MAX_CANDIDATES:
            raise AfiError(f"roi_heads: TEST.DETECTIONS_PER_IMAGE {self.test_detections_per_img} is outside 1..{ROI_MAX_CANDIDATES}, the candidate "
                           "list the selection kernels hold")
        res = cfg_get(bh, "POOLER_RESOLUTION", 14)
        self.box_pooler = ROIPooler(res, [1.0 / s.stride for s in shapes], cfg_get(bh, "POOLER_SAMPLING_RATIO", 0), cfg_get(bh, "POOLER_TYPE", "ROIAlignV2"))
        self._build_box_branch(cfg, bh)
        self.mask_on, self.keypoint_on = bool(masks), False
        if self.mask_on:
            mh = cfg_get(m, "ROI_MASK_HEAD", None)
            if mh is None:
                raise AfiError("roi_heads: the config has no MODEL.ROI_MASK_HEAD section (afigan_amd.config.get_cfg declares it)")
            if cfg_get(mh, "NAME", "MaskRCNNConvUpsampleHead") != "MaskRCNNConvUpsampleHead":
                raise AfiError(f"roi_heads: MODEL.ROI_MASK_HEAD.NAME {mh.NAME!r} is not supported (MaskRCNNConvUpsampleHead only)")
            self.mask_pooler = ROIPooler(cfg_get(mh, "POOLER_RESOLUTION", 14), [1.0 / s.stride for s in shapes], cfg_get(mh, "POOLER_SAMPLING_RATIO", 0),
                                         cfg_get(mh, "POOLER_TYPE", "ROIAlignV2"), section="ROI_MASK_HEAD")
            Sm = self.mask_pooler.output_size
            self.mask_head = MaskRCNNConvUpsampleHead((C_, Sm, Sm), self.num_classes, int(cfg_get(mh, "NUM_CONV", 0)), int(cfg_get(mh, "CONV_DIM", 256)),
                                                      cfg_get(mh, "NORM", ""), bool(cfg_get(mh, "CLS_AGNOSTIC_MASK", False)), norms=self.conv_norm_heads)
            self.mask_norm = cfg_get(mh, "NORM", "")
        for p in self.parameters():
            p.requires_grad_(False)
        # ---- the training side (losses): read here, so that a config it cannot honour fails at construction
        thr = [float(t) for t in cfg_get(rh, "IOU_THRESHOLDS", [0.5])]
        if len(thr) != 1:
            raise AfiError(f"roi_heads: MODEL.ROI_HEADS.IOU_THRESHOLDS {thr} is not supported (one threshold only)")
        if [int(v) for v in cfg_get(rh, "IOU_LABELS", [0, 1])] != [0, 1]:
            raise AfiError(f"roi_heads: MODEL.ROI_HEADS.IOU_LABELS {list(rh.IOU_LABELS)} is not supported ([0, 1] only)")
        self.iou_threshold = thr[0]
        self.batch_size_per_image = int(cfg_get(rh, "BATCH_SIZE_PER_IMAGE", 512))
        self.positive_fraction = float(cfg_get(rh, "POSITIVE_FRACTION", 0.25))
        if not 0 < self.batch_size_per_image <= ops.RPN_MAX_BATCH:
            raise AfiError(f"roi_heads: MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE {self.batch_size_per_image} is outside 1..{ops.RPN_MAX_BATCH}")
        if not 0.0 <= self.positive_fraction <= 1.0:
            raise AfiError(f"roi_heads: MODEL.ROI_HEADS.POSITIVE_FRACTION {self.positive_fraction} is outside 0..1")
        self.proposal_append_gt = bool(cfg_get(rh, "PROPOSAL_APPEND_GT", True))
        self.smooth_l1_beta = float(cfg_get(bh, "SMOOTH_L1_BETA", 0.0))
        if not self.smooth_l1_beta >= 0:
            raise AfiError(f"roi_heads: MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA {self.smooth_l1_beta} must not be negative")
        self.last_assignment = None

    def trainable_(self, flag=True, mask_head=False):
        """Turn the parameters of the box head and the box predictor into trainable ones (or back); with mask_head=True those of the mask
        head as well (heads built with masks=True; without the keyword the mask head is left as it is, frozen at construction, as before
        the mask loss existed).  The prepared weights follow the parameters' versions (frozen.prepared), so an optimizer step is seen by
        the next call."""
        if mask_head and not self.mask_on:
            raise AfiError("roi_heads: trainable_(mask_head=True) on heads built without the mask branch (build_roi_heads(cfg, input_shape, masks=True))")
        for mod in (self.box_head, self.box_predictor) + ((self.mask_head,) if mask_head else ()):
            for p in mod.parameters():
                p.requires_grad_(bool(flag))
        return self

    def _make_box_head(self, bh):
        """One FastRCNNConvFCHead and its FastRCNNOutputLayers from MODEL.ROI_BOX_HEAD."""
        S = self.box_pooler.output_size
        head = FastRCNNConvFCHead((self.channels, S, S), int(cfg_get(bh, "NUM_FC", 0)), int(cfg_get(bh, "FC_DIM", 1024)), int(cfg_get(bh, "NUM_CONV", 0)),
                                  cfg_get(bh, "NORM", ""), int(cfg_get(bh, "CONV_DIM", 256)), convs=self.conv_norm_heads)
        return head, FastRCNNOutputLayers(head.output_size, self.num_classes, bool(cfg_get(bh, "CLS_AGNOSTIC_BBOX_REG", False)))

    def _build_box_branch(self, cfg, bh):
        self.box_weights = _reg_weights("MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS", cfg_get(bh, "BBOX_REG_WEIGHTS", (10.0, 10.0, 5.0, 5.0)))
        self.box_head, self.box_predictor = self._make_box_head(bh)

    # ------------------------------------------------------------------ weights in the kernels' layout
    def _prepare_head(self, head, pr, name):
        """(fc1's weight in [out][S][S][C] order, the predictor's two layers as one [Cpad, D] weight and [Cpad] bias), kept in the slot `name` and
        rebuilt when a parameter changes."""
        fc1 = head.fcs[0]
        ts = [fc1.weight, pr.cls_score.weight, pr.cls_score.bias, pr.bbox_pred.weight, pr.bbox_pred.bias]

        def build():
            C_, S, _ = head.conv_output_shape
            out = fc1.weight.shape[0]
            w1 = fc1.weight.detach().float().view(out, C_, S, S).permute(0, 2, 3, 1).reshape(out, S * S * C_).contiguous()
            nc, nb = pr.cls_score.weight.shape[0], pr.bbox_pred.weight.shape[0]
            cpad = (nc + nb + 3) // 4 * 4
            w = torch.zeros((cpad, pr.cls_score.weight.shape[1]), device=ts[0].device, dtype=torch.float32)
            b = torch.zeros((cpad,), device=ts[0].device, dtype=torch.float32)
            w[:nc], w[nc:nc + nb] = ts[1].detach(), ts[3].detach()
            b[:nc], b[nc:nc + nb] = ts[2].detach(), ts[4].detach()
            return w1, w, b
        return prepared(self, name, ts, build)

    def _prepare_convs(self, head, name):
        """[every conv's (weight in [O][kh][kw][I] memory, bias), its norm folded in (fp64, rounded once)], rebuilt when the conv's weight or
        bias or one of the norm's four tensors changes."""
        ts = [t for l in head.conv_norm_relus for t in _conv_tensors(l)]
        return prepared(self, name, ts, lambda: [fold_conv(l, getattr(l, "norm", None)) for l in head.conv_norm_relus])

    def _prepare(self):
        return self._prepare_head(self.box_head, self.box_predictor, "prep")

    def _prepare_mask(self):
        """([(3x3 weight in [O][kh][kw][I] memory, bias)], (deconv as a [4 Cout, Cin] 1x1 weight, its bias four times), (predictor [Km, C],
        bias)), rebuilt when a parameter changes."""
        mh = self.mask_head
        ts = [t for l in mh.conv_norm_relus + [mh.deconv, mh.predictor] for t in _conv_tensors(l)]

        def build():
            convs = [fold_conv(l, getattr(l, "norm", None)) for l in mh.conv_norm_relus]
            pw = mh.predictor.weight.detach().float().reshape(mh.num_mask_classes, -1).contiguous()
            return convs, deconv_as_conv1x1(mh.deconv.weight, mh.deconv.bias), (pw, mh.predictor.bias.detach().float().contiguous())
        return prepared(self, "mask_prep", ts, build)

    # ------------------------------------------------------------------ checks
    def _check(self, features, boxes=None, counts=None, train=False):
        """train: the call computes losses (targets were given), so gradients may flow; every other call is forward-only."""
        if not train and self.training and torch.is_grad_enabled():
            raise AfiError("roi_heads: the ROI heads are inference-only (frozen): call .eval(), or run them under torch.no_grad(); the detection "
                           "losses and training are out of scope")
        missing = [f for f in self.in_features if f not in features]
        if missing:
            raise AfiError(f"roi_heads: features {missing} are missing (got {sorted(features)})")
        xs = [features[f] for f in self.in_features]
        C_ = self.channels
        for f, x in zip(self.in_features, xs):
            _check_feature("roi_heads", f"feature {f}", x)
            if x.dim() != 4 or x.shape[1] != C_ or x.shape[0] != xs[0].shape[0]:
                raise AfiError(f"roi_heads: feature {f} has shape {tuple(x.shape)}; [N, {C_}, H, W] expected")
            if not train and torch.is_grad_enabled() and x.requires_grad:
                raise AfiError("roi_heads: the ROI heads are forward-only: run them under torch.no_grad() or detach their inputs")
        if boxes is not None:
            _check_feature("roi_heads", "boxes", boxes)
            N = xs[0].shape[0]
            if boxes.dim() != 3 or boxes.shape[0] != N or boxes.shape[2] != 4 or boxes.shape[1] == 0:
                raise AfiError(f"roi_heads: boxes of shape {tuple(boxes.shape)}; [{N}, P >= 1, 4] expected")
            if not torch.is_tensor(counts) or not counts.is_cuda or counts.dtype != torch.int32 or tuple(counts.shape) != (N,):
                raise AfiError(f"roi_heads: counts must be an int32 tensor [{N}] on the GPU")
        return xs

    # ------------------------------------------------------------------ stages
    def box_features(self, features, boxes, counts):
        """The pooled features of the padded box list: pixel-major [N P, C, S, S], rows past counts zero."""
        xs = self._check(features, boxes, counts)
        with torch.no_grad():
            return self.box_pooler(xs, boxes.contiguous(), counts.contiguous())

    def box_head_forward(self, pooled, intermediates=False):
        """pooled [R, C, S, S] pixel-major -> the predictor's output [R, Cpad] (K + 1 logits, the deltas, zero padding); intermediates: the list
        of every FC's output [R, FC_DIM] as well."""
        pred, _, acts = self._run_head(self.box_head, [], self._prepare(), pooled)
        return (pred, acts) if intermediates else pred

    @staticmethod
    def _run_head(head, convs, prep, pooled):
        """One box head and its predictor on pooled [R, C, S, S]: (pred [R, Cpad], every conv's output [R, CONV_DIM, S, S], every FC's [R, FC_DIM]);
        fc1 reads the last conv's (or the pooler's) pixel-major memory in place."""
        w1, wp, bp = prep
        x, cacts, acts = pooled, [], []
        for wb in convs:
            x = conv3x3(x, wb, relu=True)
            cacts.append(x)
        if not ops.is_dense_pm(x):
            raise AfiError("roi_heads: the box head reads dense pixel-major features")
        x = _rows_as_pixels(x.permute(0, 2, 3, 1).reshape(x.shape[0], -1))
        for k, fc in enumerate(head.fcs):
            x = ops.conv1x1_fwd(x, w1 if k == 0 else fc.weight.detach(), fc.bias.detach(), act=2)
            acts.append(_pixels_as_rows(x))
        return _pixels_as_rows(ops.conv1x1_fwd(x, wp, bp)), cacts, acts

    def select(self, pred, boxes, counts, image_hw):
        """scores and boxes, candidates, NMS, pick on the predictor's output; returns every stage's output in a dict."""
        pr = self.box_predictor
        scores, cboxes = ops.roi_scores_boxes(pred, pr.num_classes, pr.cls_agnostic_bbox_reg, boxes, counts, image_hw, self.box_weights, SCALE_CLAMP)
        return self._pick(scores, cboxes)

    def _pick(self, scores, cboxes):
        """fast_rcnn_inference on scores [N, P, K] and boxes [N, P, K or 1, 4]: candidates, NMS, pick."""
        cand = ops.roi_candidates(scores, cboxes, self.test_score_thresh, ROI_MAX_CANDIDATES)
        keep = ops.roi_nms(cand["boxes"], cand["cls"], cand["valid"], self.test_nms_thresh)
        ob, os_, oc, oc_n, trunc = ops.roi_pick(cand, keep, self.test_detections_per_img)
        return {"boxes": ob, "scores": os_, "classes": oc, "counts": oc_n, "truncated": trunc, "class_scores": scores, "class_boxes": cboxes,
                "cand": cand, "keep": keep}

    def mask_features(self, features, boxes, counts):
        """The mask pooler's features of a padded box list: pixel-major [N D, C, S, S], rows past counts zero."""
        if not self.mask_on:
            raise AfiError("roi_heads: the heads were built without the mask branch (build_roi_heads(cfg, input_shape, masks=True))")
        xs = self._check(features, boxes, counts)
        with torch.no_grad():
            return self.mask_pooler(xs, boxes.contiguous(), counts.contiguous())

    def mask_head_forward(self, pooled, classes, counts, intermediates=False):
        """pooled [N D, C, S, S] pixel-major, classes [N, D] int32, counts [N] -> mask probabilities [N, D, 2S, 2S], rows past counts zero;
        intermediates: also (every conv's output [R, CONV_DIM, S, S], the deconv's 4-phase output [R, 4 CONV_DIM, S, S])."""
        if not self.mask_on:
            raise AfiError("roi_heads: the heads were built without the mask branch (build_roi_heads(cfg, input_shape, masks=True))")
        convs, (wd, bd), (wp, bp) = self._prepare_mask()
        N, D = classes.shape
        x, acts = pooled, []
        for wb in convs:
            x = conv3x3(x, wb, relu=True)
            acts.append(x)
        h = ops.conv1x1_fwd(x, wd, bd, act=2)
        probs = ops.roi_mask_probs(h, wp, bp, classes.contiguous(), counts.contiguous())
        probs = probs.view(N, D, probs.shape[1], probs.shape[2])
        return (probs, acts, h) if intermediates else probs

    def _box_branch(self, xs, boxes, counts, image_hw, intermediates):
        """Pooler, head, predictor and selection on the padded proposals: ``select``'s dict plus ``pooled``, ``fc`` and ``pred``."""
        pooled = self.box_pooler(xs, boxes, counts)
        pred, acts = self.box_head_forward(pooled, intermediates=True)
        r = self.select(pred, boxes, counts, image_hw)
        r.update(pooled=pooled, fc=acts, pred=pred)
        return r

    def _mask_branch(self, xs, boxes, classes, counts, r=None):
        pooled = self.mask_pooler(xs, boxes, counts)
        probs, acts, h = self.mask_head_forward(pooled, classes, counts, intermediates=True)
        if r is not None:
            r.update(mask_pooled=pooled, mask_convs=acts, mask_deconv=h, mask_probs=probs)
        return probs

    def forward_padded(self, image_sizes, features, boxes, counts, intermediates=False):
        """(boxes [N, D, 4], scores [N, D], classes [N, D] int32, counts [N] int32, truncated [N] int32) on the device, D =
        TEST.DETECTIONS_PER_IMAGE, rows past counts zero; image_sizes: [N, 2] device tensor (height, width) of the un-padded images; boxes
        [N, P, 4] / counts [N]: the proposals as ``RPN.forward_padded`` returns them.  No host read: capturable in a hipGraph.  intermediates:
        the dict of ``select`` plus ``pooled``, ``fc`` and ``pred`` instead.  With the mask branch a sixth tensor, masks [N, D, 2S, 2S] (rows
        past counts zero), and the intermediates ``mask_pooled``, ``mask_convs``, ``mask_deconv`` and ``mask_probs``."""
        xs = self._check(features, boxes, counts)
        if not torch.is_tensor(image_sizes) or not image_sizes.is_cuda:
            raise AfiError("roi_heads: forward_padded takes the image sizes as an [N, 2] tensor on the GPU (forward() takes a list)")
        if tuple(image_sizes.shape) != (xs[0].shape[0], 2):
            raise AfiError(f"roi_heads: image sizes of shape {tuple(image_sizes.shape)} for a batch of {xs[0].shape[0]}")
        with torch.no_grad():
            boxes, counts = boxes.contiguous(), counts.contiguous()
            r = self._box_branch(xs, boxes, counts, image_sizes.to(torch.float32).contiguous(), intermediates)
            masks = self._mask_branch(xs, r["boxes"], r["classes"], r["counts"], r) if self.mask_on else None
        if intermediates:
            return r
        out = (r["boxes"], r["scores"], r["classes"], r["counts"], r["truncated"])
        return out + (masks,) if self.mask_on else out

    # ------------------------------------------------------------------ training (the box branch)
    @staticmethod
    def _padded_proposals(proposals, N, dev):
        """The images' ``proposal_boxes`` as one padded [N, P, 4] tensor and counts [N] int32; the counts come from the shapes."""
        pbs = []
        for p in proposals:
            b = p.proposal_boxes
            b = b.tensor if hasattr(b, "tensor") else b
            _check_feature("roi_heads", "proposal boxes", b)
            pbs.append(b.reshape(-1, 4))
        P = max(1, max(int(b.shape[0]) for b in pbs))
        boxes = torch.zeros((N, P, 4), device=dev, dtype=torch.float32)
        for n, b in enumerate(pbs):
            boxes[n, :b.shape[0]] = b
        return boxes, torch.tensor([int(b.shape[0]) for b in pbs], dtype=torch.int32).to(dev)

    def _targets(self, targets, N, device):
        """The images' boxes and classes as padded [N, Gmax, 4] fp32 / [N, Gmax] int32 tensors and counts [N] int32 on the device.  Every target
        carries ``gt_boxes`` (a Boxes or a [G, 4] tensor) and ``gt_classes`` [G], as attributes or as dict entries."""
        if len(targets) != N:
            raise AfiError(f"roi_heads: {len(targets)} targets for a batch of {N}")
        boxes, classes = [], []
        for t in targets:
            b, c = _target_field(t, "gt_boxes"), _target_field(t, "gt_classes")
            if not torch.is_tensor(b) or b.dim() != 2 or b.shape[1] != 4 or not torch.is_tensor(c) or c.dim() != 1 or c.shape[0] != b.shape[0]:
                raise AfiError("roi_heads: every target needs gt_boxes (a Boxes or a [G, 4] tensor) and gt_classes [G]")
            if c.is_floating_point() or c.dtype == torch.bool:
                raise AfiError(f"roi_heads: gt_classes must be integers, got {c.dtype}")
            boxes.append(b)
            classes.append(c)
        gmax = max(b.shape[0] for b in boxes)
        if gmax > ops.RPN_MAX_GT:
            raise AfiError(f"roi_heads: {gmax} ground-truth boxes in one image; at most {ops.RPN_MAX_GT} are supported")
        allc = torch.cat([c.reshape(-1).to(torch.int64) for c in classes]) if gmax else None
        if allc is not None and allc.numel():
            lo, hi = torch.stack([allc.min(), allc.max()]).tolist()         # (the one host read of a call whose classes live on the device)
            if lo < 0 or hi >= self.num_classes:
                raise AfiError(f"roi_heads: gt_classes must lie in 0..{self.num_classes - 1} (MODEL.ROI_HEADS.NUM_CLASSES {self.num_classes}), "
                               f"got {lo}..{hi}")
        gt = torch.zeros((N, max(gmax, 1), 4), device=device, dtype=torch.float32)
        gc = torch.zeros((N, max(gmax, 1)), device=device, dtype=torch.int32)
        for n, (b, c) in enumerate(zip(boxes, classes)):
            if b.shape[0]:
                gt[n, :b.shape[0]] = b.detach().to(device=device, dtype=torch.float32)
                gc[n, :b.shape[0]] = c.detach().to(device=device, dtype=torch.int32)
        return gt, gc, torch.tensor([b.shape[0] for b in boxes], dtype=torch.int32).to(device)

    @property
    def mask_batch_per_image(self):
        """Bf: the rows per image the mask branch trains on, the most positives the sampler takes."""
        return int(self.batch_size_per_image * self.positive_fraction)

    @staticmethod
    def _target_polygons(targets):
        """Every image's instances as lists of flat coordinate sequences, from the targets' ``gt_masks``: an object with ``.polygons`` (what the
        dual-scale mapper yields) or a list with one list of polygons per instance.  Host data; nothing touches the device."""
        out = []
        for n, t in enumerate(targets):
            m = t.get("gt_masks") if isinstance(t, dict) else getattr(t, "gt_masks", None)
            if m is None:
                raise AfiError(f"roi_heads: target {n} has no `gt_masks`: these heads were built with masks=True and train the mask branch "
                               "on every instance's polygons; for targets with boxes only the mask loss is not built yet: give every target "
                               "its `gt_masks`, or train heads built without the mask branch (box losses only)")
            if torch.is_tensor(m) or torch.is_tensor(getattr(m, "tensor", None)):
                raise AfiError(f"roi_heads: target {n}'s `gt_masks` is a bitmask ({type(m).__name__}); polygon masks only (an object with "
                               "`.polygons`, or one list of flat coordinate arrays per instance): bitmask targets are out of scope")
            polys = getattr(m, "polygons", m)
            if not isinstance(polys, (list, tuple)) or any(not isinstance(p, (list, tuple)) for p in polys):
                raise AfiError(f"roi_heads: target {n}'s `gt_masks` must be an object with `.polygons` or a list with one list of flat "
                               f"coordinate arrays per instance, got {type(m).__name__}")
            b = _target_field(t, "gt_boxes")
            if torch.is_tensor(b) and len(polys) != b.shape[0]:             # (a target without gt_boxes is _targets' to refuse)
                raise AfiError(f"roi_heads: target {n}'s `gt_masks` has {len(polys)} instances and `gt_boxes` {b.shape[0]}")
            out.append([[p.detach().cpu().numpy() if torch.is_tensor(p) else p for p in inst] for inst in polys])
        return out

    def _refuse_training(self):
        if isinstance(self.box_head, nn.ModuleList):
            raise AfiError("roi_heads: CascadeROIHeads is inference-only (frozen): cascade training is out of scope")

    def losses_padded(self, features, boxes, counts, gt, gt_classes, gt_counts, keys=None, gt_polygons=None):
        """``losses`` on padded device tensors: proposals boxes [N, P, 4] / counts [N] (``RPN.forward_padded``'s layout), ground truth gt
        [N, Gmax, 4] fp32, gt_classes [N, Gmax] int32, gt_counts [N] int32.  Heads built with masks=True also take gt_polygons = the packed
        polygons of the call on the device (``ops.mask_polygons``: xy, vert_off, poly_off, one annotation per (image, ground-truth slot)) and
        return ``loss_mask`` as well.  No host read."""
        self._refuse_training()
        xs = self._check(features, boxes, counts, train=True)
        _check_feature("roi_heads", "gt boxes", gt)
        if self.mask_on:
            if gt_polygons is None or len(gt_polygons) != 3:
                raise AfiError("roi_heads: heads built with masks=True train the mask branch: losses_padded needs gt_polygons = (xy, vert_off, "
                               "poly_off) on the device (ops.mask_polygons)")
            if self.mask_batch_per_image < 1:
                raise AfiError(f"roi_heads: MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE {self.batch_size_per_image} x POSITIVE_FRACTION "
                               f"{self.positive_fraction} leaves the mask branch no foreground row")
        elif gt_polygons is not None:
            raise AfiError("roi_heads: gt_polygons given to heads built without the mask branch (build_roi_heads(cfg, input_shape, masks=True))")
        h, pr = self.box_head, self.box_predictor
        params = [t for fc in h.fcs for t in (fc.weight, fc.bias)] + [pr.cls_score.weight, pr.cls_score.bias, pr.bbox_pred.weight, pr.bbox_pred.bias]
        out = _ROIBoxLossFn.apply(self, boxes.detach().contiguous(), counts.contiguous(), gt.contiguous(), gt_classes.contiguous(),
                                  gt_counts.contiguous(), keys, len(xs), *xs, *params)
        losses = {"loss_cls": out[0], "loss_box_reg": out[1]}
        if self.mask_on:
            mh = self.mask_head
            mparams = [t for l in mh.conv_norm_relus + [mh.deconv, mh.predictor] for t in (l.weight, l.bias)]
            losses["loss_mask"] = _ROIMaskLossFn.apply(self, tuple(gt_polygons), gt_counts.contiguous(), int(gt.shape[1]), len(xs), *xs, *mparams)
        return losses

    def losses(self, images, features, proposals, targets, keys=None):
        """{"loss_cls", "loss_box_reg"} of detectron2's StandardROIHeads in training (box branch), differentiable in the features and, after
        ``trainable_()``, the parameters of the box head and predictor; heads built with masks=True add ``loss_mask`` (differentiable in the
        mask head's parameters too, after ``trainable_(mask_head=True)``) and need ``gt_masks`` on every target: an object with ``.polygons`` or one list of flat coordinate arrays
        per instance.  proposals: one object with ``proposal_boxes`` per image; targets: one
        object (or dict) with ``gt_boxes`` and ``gt_classes`` per image.  keys: [N, P + Gmax] 32-bit integers on the device that decide the
        sample (the candidates with the smallest (key, index) are taken; a candidate is a proposal or, behind them, an appended ground-truth
        box); drawn from torch's generator when None.  The assignment, the sample and the training list of the call stay in
        ``last_assignment``.  Works in either mode."""
        self._refuse_training()
        inst = self._target_polygons(targets) if self.mask_on else None      # host data: refused before anything touches the device
        xs = self._check(features, train=True)
        N, dev = xs[0].shape[0], xs[0].device
        if len(proposals) != N:
            raise AfiError(f"roi_heads: {len(proposals)} proposal lists for a batch of {N}")
        boxes, counts = self._padded_proposals(proposals, N, dev)
        gt, gc, gn = self._targets(targets, N, dev)
        polys = ops.mask_polygons(inst, N, int(gt.shape[1]), dev) if self.mask_on else None
        return self.losses_padded(features, boxes, counts, gt, gc, gn, keys, polys)

    def _forward_train(self, images, features, proposals, targets, keys=None):
        """(the sampled proposals per image with ``gt_classes`` and ``gt_boxes``, losses), as detectron2's StandardROIHeads.forward in training.
        One device-to-host read, of the sample's counts."""
        losses = self.losses(images, features, proposals, targets, keys)
        a = self.last_assignment
        out = []
        for n, (p, c) in enumerate(zip(proposals, a["counts"].tolist())):
            size = tuple(getattr(p, "image_size", None) or images.image_sizes[n])
            out.append(_make_sampled(size, a["boxes"][n, :c], a["gt_classes"][n, :c].to(torch.int64), a["gt_boxes"][n, :c]))
        return out, losses

    def forward(self, images, features, proposals, targets=None, keys=None):
        """detectron2's StandardROIHeads.forward.  At inference: (one result per image -- image_size, pred_boxes, scores, pred_classes (int64),
        sorted by score --, {}); one device-to-host read, of counts and truncated.  In training mode with targets: (the sampled proposals with
        their labels, ``losses()``' dict; keys: as there)."""
        if targets is not None:
            if not self.training:
                raise AfiError("roi_heads: targets given to a module in eval mode -- call .train() for (proposals, losses), or "
                               "StandardROIHeads.losses() for the losses alone")
            return self._forward_train(images, features, proposals, targets, keys)
        xs = self._check(features)
        sizes = [(int(h), int(w)) for h, w in images.image_sizes]
        N, dev = xs[0].shape[0], xs[0].device
        if len(sizes) != N or len(proposals) != N:
            raise AfiError(f"roi_heads: {len(sizes)} image sizes and {len(proposals)} proposal lists for a batch of {N}")
        boxes, counts = self._padded_proposals(proposals, N, dev)
        hw = torch.tensor(sizes, dtype=torch.float32).to(dev)
        ob, os_, oc, cn, trunc, *mk = self.forward_padded(hw, features, boxes, counts)
        host = torch.stack([cn, trunc]).tolist()
        if any(host[1]):
            raise AfiError(f"roi_heads: image(s) {[n for n, t in enumerate(host[1]) if t]} have more than {ROI_MAX_CANDIDATES} class scores above "
                           f"MODEL.ROI_HEADS.SCORE_THRESH_TEST {self.test_score_thresh} and fewer than TEST.DETECTIONS_PER_IMAGE "
                           f"{self.test_detections_per_img} survive NMS among the {ROI_MAX_CANDIDATES} highest (the candidate cap): the result "
                           "could differ from the uncapped one; raise SCORE_THRESH_TEST")
        return [_make_detections(sz, ob[n, :c], os_[n, :c], oc[n, :c].to(torch.int64), mk[0][n, :c].unsqueeze(1) if mk else None)
                for n, (sz, c) in enumerate(zip(sizes, host[0]))], {}

    def forward_with_given_boxes(self, features, instances):
        """detectron2's StandardROIHeads.forward_with_given_boxes: without the mask branch the instances unchanged; with it, ``pred_masks``
        [n, 1, 2S, 2S] set on every instance from its ``pred_boxes`` and ``pred_classes``."""
        if self.training and torch.is_grad_enabled():
            raise AfiError("roi_heads: the ROI heads are inference-only (frozen): call .eval(), or run them under torch.no_grad()")
        if not self.mask_on:
            return instances
        xs = self._check(features)
        N, dev = xs[0].shape[0], xs[0].device
        if len(instances) != N:
            raise AfiError(f"roi_heads: {len(instances)} instance lists for a batch of {N}")
        bs, cs = [], []
        for inst in instances:
            if getattr(inst, "pred_boxes", None) is None or getattr(inst, "pred_classes", None) is None:
                raise AfiError("roi_heads: forward_with_given_boxes needs `pred_boxes` and `pred_classes` on every instance")
            b = inst.pred_boxes.tensor if hasattr(inst.pred_boxes, "tensor") else inst.pred_boxes
            _check_feature("roi_heads", "pred_boxes", b)
            if not inst.pred_classes.is_cuda:
                raise AfiError("roi_heads: pred_classes is a CPU tensor; the ROI heads run on the GPU only, there is no CPU fallback")
            bs.append(b.reshape(-1, 4))
            cs.append(inst.pred_classes.reshape(-1))
            if cs[-1].shape[0] != bs[-1].shape[0]:
                raise AfiError(f"roi_heads: {bs[-1].shape[0]} pred_boxes and {cs[-1].shape[0]} pred_classes")
        # the list length forward_padded uses whenever the boxes fit, so that the same kernels run on the same shapes and the masks agree bit for bit
        D = max(self.test_detections_per_img, max(int(b.shape[0]) for b in bs))
        boxes = torch.zeros((N, D, 4), device=dev, dtype=torch.float32)
        classes = torch.zeros((N, D), device=dev, dtype=torch.int32)
        for n, (b, c) in enumerate(zip(bs, cs)):
            boxes[n, :b.shape[0]] = b
            classes[n, :b.shape[0]] = c.to(torch.int32)
        counts = torch.tensor([int(b.shape[0]) for b in bs], dtype=torch.int32).to(dev)
        with torch.no_grad():
            probs = self._mask_branch(xs, boxes, classes, counts)
        for n, (inst, b) in enumerate(zip(instances, bs)):
            inst.pred_masks = probs[n, :b.shape[0]].unsqueeze(1)
        return instances


@ROI_HEADS_REGISTRY.register()
class CascadeROIHeads(StandardROIHeads):
    """detectron2 v0.1.1's CascadeROIHeads at inference (the module docstring's last part): StandardROIHeads' checks, pooler, selection, mask
    branch, ``forward`` and ``forward_with_given_boxes``; ``box_head`` / ``box_predictor`` are ModuleLists of one head per stage."""
    conv_norm_heads = True
    MAX_STAGES = 8

    def _refuse_name(self, name):
        return AfiError(f"roi_heads: MODEL.ROI_HEADS.NAME {name!r} is not 'CascadeROIHeads', the class that was asked for")

    def _build_box_branch(self, cfg, bh):
        ch = cfg_get(cfg.MODEL, "ROI_BOX_CASCADE_HEAD", None)
        if ch is None:
            raise AfiError("roi_heads: the config has no MODEL.ROI_BOX_CASCADE_HEAD section (afigan_amd.config.get_cfg declares it)")
        ious, weights = tuple(cfg_get(ch, "IOUS", ())), tuple(cfg_get(ch, "BBOX_REG_WEIGHTS", ()))
        if len(ious) != len(weights):
            raise AfiError(f"roi_heads: MODEL.ROI_BOX_CASCADE_HEAD.IOUS has {len(ious)} entries and MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS "
                           f"{len(weights)}: one of each per stage")
        if not 1 <= len(ious) <= self.MAX_STAGES:
            raise AfiError(f"roi_heads: MODEL.ROI_BOX_CASCADE_HEAD.IOUS gives {len(ious)} stages; 1..{self.MAX_STAGES} are supported")
        first = list(cfg_get(cfg.MODEL.ROI_HEADS, "IOU_THRESHOLDS", [0.5]))[0]
        if float(ious[0]) != float(first):
            raise AfiError(f"roi_heads: MODEL.ROI_BOX_CASCADE_HEAD.IOUS[0] {ious[0]} must equal MODEL.ROI_HEADS.IOU_THRESHOLDS[0] {first} (detectron2 "
                           "asserts it)")
        self.num_stages = len(ious)
        self.stage_ious = tuple(float(v) for v in ious)
        self.box_norm = cfg_get(bh, "NORM", "")
        self._train_enabled = False
        self.stage_weights = tuple(_reg_weights(f"MODEL.ROI_BOX_CASCADE_HEAD.BBOX_REG_WEIGHTS[{k}]", w) for k, w in enumerate(weights))
        if not cfg_get(bh, "CLS_AGNOSTIC_BBOX_REG", False):
            raise AfiError("roi_heads: MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG False is not supported by CascadeROIHeads (detectron2 asserts "
                           "class-agnostic box regression)")
        heads = [self._make_box_head(bh) for _ in range(self.num_stages)]
        self.box_head = nn.ModuleList([h for h, _ in heads])
        self.box_predictor = nn.ModuleList([p for _, p in heads])

    def _prepare(self, stage=0):
        """Stage `stage`'s (folded convs, (fc1's weight, the predictor's weight and bias))."""
        return (self._prepare_convs(self.box_head[stage], f"prep_convs{stage}"),
                self._prepare_head(self.box_head[stage], self.box_predictor[stage], f"prep{stage}"))

    def box_head_forward(self, pooled, stage=0, intermediates=False):
        """pooled [R, C, S, S] pixel-major -> stage `stage`'s predictor output [R, Cpad] (K + 1 logits, 4 deltas, zero padding); intermediates:
        also (every conv's output [R, CONV_DIM, S, S], every FC's output [R, FC_DIM])."""
        pred, cacts, acts = self._run_head(self.box_head[stage], *self._prepare(stage), pooled)
        return (pred, cacts, acts) if intermediates else pred

    def select(self, pred, boxes, counts, image_hw):
        raise AfiError("roi_heads: CascadeROIHeads decodes stage by stage (forward_padded); there is no selection on one predictor output")

    # ------------------------------------------------------------------ training (the box branch of every stage)
    def trainable_(self, flag=True, mask_head=False):
        """Enable training of these heads (``losses`` / ``losses_padded`` / ``forward`` with targets refuse until this was called) and make the
        parameters of every stage's box head and predictor trainable (flag=False: frozen, training stays enabled).  The affine of a "BN" /
        "SyncBN" norm of the box heads becomes a pair of parameters under the same keys ``norm.weight`` / ``norm.bias`` (a "FrozenBN" norm
        stays four buffers).  mask_head=True: the mask head's parameters as well (heads built with masks=True), its norms' affine likewise."""
        if mask_head and not self.mask_on:
            raise AfiError("roi_heads: trainable_(mask_head=True) on heads built without the mask branch (build_roi_heads(cfg, input_shape, masks=True))")
        for head in list(self.box_head) + ([self.mask_head] if mask_head else []):
            for conv in head.conv_norm_relus:
                n = getattr(conv, "norm", None)
                if isinstance(n, TrackedFrozenBatchNorm2d) and not isinstance(n.weight, nn.Parameter):
                    w, b = n.weight, n.bias
                    del n._buffers["weight"], n._buffers["bias"]
                    n.weight, n.bias = nn.Parameter(w.detach().clone(), requires_grad=False), nn.Parameter(b.detach().clone(), requires_grad=False)
        self._train_enabled = True
        for mod in (self.box_head, self.box_predictor) + ((self.mask_head,) if mask_head else ()):
            for p in mod.parameters():
                p.requires_grad_(bool(flag))
        return self

    def _refuse_training(self):
        if not self._train_enabled:
            raise AfiError("roi_heads: CascadeROIHeads is inference-only (frozen): cascade training is out of scope until trainable_() enables it "
                           "(CascadeROIHeads.trainable_)")
        # what depends on the module's state alone is refused here, before anything touches the device
        heads = [(h, self.box_norm) for h in self.box_head] + ([(self.mask_head, self.mask_norm)] if self.mask_on else [])
        batch = [norm for h, norm in heads if any(isinstance(getattr(c, "norm", None), TrackedFrozenBatchNorm2d) for c in h.conv_norm_relus)]
        if batch and not self.training:
            raise AfiError("roi_heads: targets given to CascadeROIHeads in eval mode whose heads carry BN / SyncBN: the batch statistics "
                           "are those of training mode -- call .train()")
        if "SyncBN" in batch and torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size() > 1:
            raise AfiError("roi_heads: SyncBN heads under a process group of more than one rank: the exchange of the statistics "
                           "between ranks is not built yet")

    def _train_params(self):
        """(every stage's trainable tensors in one list, per stage the positions of each in it): conv weight, bias (no norm) or the BN affine,
        the FCs, the predictor."""
        plist, layout = [], []

        def add(t):
            plist.append(t)
            return len(plist) - 1
        for head, pr in zip(self.box_head, self.box_predictor):
            start, convs = len(plist), []
            for conv in head.conv_norm_relus:
                n = getattr(conv, "norm", None)
                slot = {"weight": add(conv.weight), "bias": add(conv.bias) if conv.bias is not None else None, "gamma": None, "beta": None}
                if isinstance(n, TrackedFrozenBatchNorm2d):
                    slot["gamma"], slot["beta"] = add(n.weight), add(n.bias)
                convs.append(slot)
            fc = [add(t) for l in head.fcs for t in (l.weight, l.bias)]
            pred = [add(t) for t in (pr.cls_score.weight, pr.cls_score.bias, pr.bbox_pred.weight, pr.bbox_pred.bias)]
            layout.append({"conv": convs, "fc": fc, "pred": pred, "all": list(range(start, len(plist)))})
        return plist, layout

    def _train_conv(self, name, conv, x, counts, folded):
        """One conv-norm-ReLU of a head in training on the padded rows x [N B, C, S, S]: (output, what the backward keeps).  No norm: the
        biased conv with ReLU.  FrozenBN: the folded conv with ReLU (folded(): its prepared weight and bias).  BN / SyncBN: the conv without
        bias, then the statistics over the rows below counts (the running buffers and num_batches_tracked advance) and the list-masked
        normalise + ReLU.  name: the slot the conv's weight in the kernels' memory is kept under.  (Eval mode and more than one rank under
        BN / SyncBN are ``_refuse_training``'s to refuse, before the call reaches the device.)"""
        n = getattr(conv, "norm", None)
        if isinstance(n, TrackedFrozenBatchNorm2d):
            w = prepared(self, f"train_w{name}", [conv.weight], lambda: ops.to_ohwi(conv.weight.detach().float()))
            u = conv3x3(x, (w, None), relu=False)
            mean, invstd = ops.roi_bn_stats(u, counts, n.eps, self.bn_momentum, n.running_mean, n.running_var, n.num_batches_tracked)
            gamma, beta = n.weight.detach().float().contiguous(), n.bias.detach().float().contiguous()
            y = ops.roi_bn_relu_fwd(u, counts, mean, invstd, gamma, beta)
            return y, {"kind": "bn", "tensors": [y, u, mean, invstd, gamma, w]}
        wb = folded()
        y = conv3x3(x, wb, relu=True)
        if n is None:
            return y, {"kind": "relu", "tensors": [y, wb[0]]}
        s = (n.weight.double() * torch.rsqrt(n.running_var.double() + n.eps)).float().contiguous()
        return y, {"kind": "frozen", "tensors": [y, wb[0], s]}

    bn_momentum = 0.1                 # nn.BatchNorm2d's / nn.SyncBatchNorm's default, which detectron2's get_norm keeps

    def losses_padded(self, features, boxes, counts, gt, gt_classes, gt_counts, keys=None, gt_polygons=None, image_sizes=None):
        """``StandardROIHeads.losses_padded`` for the cascade: {"loss_cls_stage{k}", "loss_box_reg_stage{k}"} of every stage (and ``loss_mask``
        on stage 0's training list for heads built with masks=True).  image_sizes: [N, 2] fp32 (height, width) on the device, which the boxes
        a stage hands to the next are clipped to.  No host read."""
        self._refuse_training()
        xs = self._check(features, boxes, counts, train=True)
        _check_feature("roi_heads", "gt boxes", gt)
        N = xs[0].shape[0]
        if not torch.is_tensor(image_sizes) or not image_sizes.is_cuda or tuple(image_sizes.shape) != (N, 2):
            raise AfiError(f"roi_heads: CascadeROIHeads.losses_padded needs image_sizes = an [{N}, 2] tensor (height, width) on the GPU: the boxes "
                           "of a stage are clipped to the image before the next stage is labelled")
        if self.mask_on:
            if gt_polygons is None or len(gt_polygons) != 3:
                raise AfiError("roi_heads: heads built with masks=True train the mask branch: losses_padded needs gt_polygons = (xy, vert_off, "
                               "poly_off) on the device (ops.mask_polygons)")
            if self.mask_batch_per_image < 1:
                raise AfiError(f"roi_heads: MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE {self.batch_size_per_image} x POSITIVE_FRACTION "
                               f"{self.positive_fraction} leaves the mask branch no foreground row")
        elif gt_polygons is not None:
            raise AfiError("roi_heads: gt_polygons given to heads built without the mask branch (build_roi_heads(cfg, input_shape, masks=True))")
        params, self._train_layout = self._train_params()
        out = _CascadeBoxLossFn.apply(self, boxes.detach().contiguous(), counts.contiguous(), gt.contiguous(), gt_classes.contiguous(),
                                      gt_counts.contiguous(), keys, image_sizes.detach().to(torch.float32).contiguous(), len(xs), *xs, *params)
        losses = {}
        for k in range(self.num_stages):
            losses[f"loss_cls_stage{k}"], losses[f"loss_box_reg_stage{k}"] = out[2 * k], out[2 * k + 1]
        if self.mask_on:
            mh = self.mask_head
            if not any(getattr(l, "norm", None) is not None for l in mh.conv_norm_relus):           # without norm: the parent's path
                mparams = [t for l in mh.conv_norm_relus + [mh.deconv, mh.predictor] for t in (l.weight, l.bias)]
                losses["loss_mask"] = _ROIMaskLossFn.apply(self, tuple(gt_polygons), gt_counts.contiguous(), int(gt.shape[1]), len(xs), *xs, *mparams)
                return losses
            mparams, convs = [], []

            def add(t):
                mparams.append(t)
                return len(mparams) - 1
            for conv in mh.conv_norm_relus:
                n = getattr(conv, "norm", None)
                slot = {"weight": add(conv.weight), "bias": add(conv.bias) if conv.bias is not None else None, "gamma": None, "beta": None}
                if isinstance(n, TrackedFrozenBatchNorm2d):
                    slot["gamma"], slot["beta"] = add(n.weight), add(n.bias)
                convs.append(slot)
            self._mask_layout = {"conv": convs, "deconv": [add(mh.deconv.weight), add(mh.deconv.bias)],
                                 "pred": [add(mh.predictor.weight), add(mh.predictor.bias)]}
            losses["loss_mask"] = _CascadeMaskLossFn.apply(self, tuple(gt_polygons), gt_counts.contiguous(), int(gt.shape[1]), len(xs), *xs, *mparams)
        return losses

    def losses(self, images, features, proposals, targets, keys=None):
        """The stage losses of detectron2's CascadeROIHeads in training (``losses_padded``), from per-image proposals and targets as
        ``StandardROIHeads.losses`` takes them; the image sizes come from ``images.image_sizes`` or, without it, the proposals' ``image_size``."""
        self._refuse_training()
        inst = self._target_polygons(targets) if self.mask_on else None
        xs = self._check(features, train=True)
        N, dev = xs[0].shape[0], xs[0].device
        if len(proposals) != N:
            raise AfiError(f"roi_heads: {len(proposals)} proposal lists for a batch of {N}")
        sizes = getattr(images, "image_sizes", None) or [getattr(p, "image_size", None) for p in proposals]
        if len(sizes) != N or any(s is None or len(s) != 2 for s in sizes):
            raise AfiError("roi_heads: CascadeROIHeads.losses needs the image sizes (images.image_sizes, or image_size on every proposal list): the "
                           "boxes of a stage are clipped to the image before the next stage is labelled")
        boxes, counts = self._padded_proposals(proposals, N, dev)
        gt, gc, gn = self._targets(targets, N, dev)
        polys = ops.mask_polygons(inst, N, int(gt.shape[1]), dev) if self.mask_on else None
        hw = torch.tensor([(float(h), float(w)) for h, w in sizes], dtype=torch.float32).to(dev)
        return self.losses_padded(features, boxes, counts, gt, gc, gn, keys, polys, hw)

    def _box_branch(self, xs, boxes, counts, image_hw, intermediates):
        """The S stages and the selection: ``_pick``'s dict, ``class_scores`` the mean scores, ``class_boxes`` the last stage's boxes [N, P, 1, 4],
        ``pooled`` / ``fc`` / ``pred`` the last stage's; intermediates: ``stages``, per stage ``proposals``, ``pooled``, ``convs``, ``fc``, ``pred``,
        ``scores`` (the running score after it) and ``boxes``.  Without intermediates the running score is one buffer, updated in place."""
        N, P = boxes.shape[:2]
        scores, cur, stages = None, boxes, []
        for k in range(self.num_stages):
            pooled = self.box_pooler(xs, cur, counts)
            pred, cacts, acts = self.box_head_forward(pooled, k, intermediates=True)
            last = k == self.num_stages - 1
            scores, nxt = ops.roi_cascade_stage(pred, self.num_classes, cur, counts, image_hw, self.stage_weights[k], prev_scores=scores,
                                                out_scale=1.0 / self.num_stages if last else 1.0, scale_clamp=SCALE_CLAMP,
                                                out=None if intermediates else scores)
            if intermediates:
                stages.append({"proposals": cur, "pooled": pooled, "convs": cacts, "fc": acts, "pred": pred, "scores": scores, "boxes": nxt})
            cur = nxt
        r = self._pick(scores, cur.view(N, P, 1, 4))
        r.update(pooled=pooled, fc=acts, pred=pred)
        if intermediates:
            r["stages"] = stages
        return r


def build_roi_heads(cfg, input_shape, masks=False, cascade=False):
    """detectron2's build_roi_heads: the class registered under MODEL.ROI_HEADS.NAME.  masks=True builds the mask branch as well (it needs
    MODEL.MASK_ON True); without it a MASK_ON config is refused.  cascade=True builds 'CascadeROIHeads' (the NAME must say so); without it a
    Cascade config is refused."""
    name = cfg_get(cfg_get(cfg.MODEL, "ROI_HEADS", None), "NAME", "StandardROIHeads")
    if cascade and name != "CascadeROIHeads":
        raise AfiError(f"roi_heads: cascade=True builds 'CascadeROIHeads' and needs MODEL.ROI_HEADS.NAME 'CascadeROIHeads', got {name!r}")
    if not cascade and name != "StandardROIHeads":
        raise AfiError(f"roi_heads: MODEL.ROI_HEADS.NAME {name!r} is not supported (this package provides the box branch of 'StandardROIHeads')"
                       + ("; 'CascadeROIHeads' is built with build_roi_heads(cfg, input_shape, cascade=True)" if name == "CascadeROIHeads" else ""))
    cls = ROI_HEADS_REGISTRY.get(name)
    return cls(cfg, input_shape, masks=True) if masks else cls(cfg, input_shape)
