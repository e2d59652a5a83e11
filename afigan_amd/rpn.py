"""The frozen RPN proposal generator of the inference configs: detectron2 v0.1.1's ``RPN`` (``StandardRPNHead``, ``DefaultAnchorGenerator``,
``Box2BoxTransform``, ``find_top_rpn_proposals``) at inference, forward only, on this package's HIP kernels.

Per level l of ``MODEL.RPN.IN_FEATURES`` (stride s, map H x W, A anchors per cell):
  - head: t = relu(conv3x3(x)); objectness_logits = conv1x1(t) [A channels], anchor_deltas = conv1x1(t) [4A channels, 4a + c]; one set of weights;
  - anchors: cell anchor a = (-w/2, -h/2, w/2, h/2), w = sqrt(size^2 / ratio), h = ratio w (sizes, then ratios); anchor (y W + x) A + a is the
    cell anchor shifted by (x s, y s).  Never materialised: the kernels form an anchor from its index and the ``cell_anchors`` buffer;
  - the min(PRE_NMS_TOPK_TEST, H W A) highest logits per image, equal logits in ascending anchor index (detectron2's sort leaves ties open;
    this is the rule here), NaN below every number;
  - Box2BoxTransform(BBOX_REG_WEIGHTS).apply_deltas with dw / dh clamped at log(1000 / 16), clip to the image's own un-padded size, drop
    boxes with a side <= PROPOSAL_GENERATOR.MIN_SIZE;
  - greedy NMS per image and level (batched_nms with the level as the category), inter / (area_a + area_b - inter) > NMS_THRESH in fp32;
then the survivors of all levels by logit (ties: level, then rank), the first POST_NMS_TOPK_TEST.

Keys: ``rpn_head.{conv, objectness_logits, anchor_deltas}.{weight, bias}`` and the buffers ``anchor_generator.cell_anchors.{l}`` [A, 4] --
detectron2's, so a detector checkpoint's ``proposal_generator.*`` loads with strict=True.  Every parameter has requires_grad False.

Kernels: the 3x3 conv + ReLU is afi_conv3x3_wino_infer / afi_conv3x3_fwd (the regime rule of frozen.conv3x3), the two 1x1 convs ONE
afi_conv1x1_fwd over their concatenated weights (A + 4A channels, zero-padded to a multiple of 4; rebuilt when a parameter changes:
frozen.prepared); selection afi_rpn_topk, afi_rpn_decode, afi_rpn_nms per level and one afi_rpn_merge (csrc/rpn.hip); a level whose list is
longer than 1024 (training: PRE_NMS_TOPK_TRAIN up to 4096) runs afi_rpn_topk_wide / afi_rpn_nms_wide, and the merge is then
afi_rpn_merge_wide.  No torch sort / topk /
conv, MIOpen or hipBLASLt kernel runs.  ``forward_padded`` has no host read and can be captured in a hipGraph; ``forward`` reads ``counts`` once.

Training (``RPN.losses``, and ``forward`` in training mode with ``gt_instances``): RPNOutputs._get_ground_truth, subsample_labels, get_deltas
and rpn_losses on afi_rpn_match / afi_rpn_sample / afi_rpn_loss (csrc/rpn_loss.hip), the head's backward on the conv kernels' own data- and
weight-gradient entry points (``_RPNLossFn``).  The sample is decided by 32-bit keys (the smallest (key, anchor index) are taken), drawn from
torch's generator unless given: uniform, but not ``randperm``'s stream.  ``trainable_()`` makes the six parameters trainable.

Out of scope (AfiError): a training-mode call without ``gt_instances``, ``gt_instances`` in eval mode, BOUNDARY_THRESH other than -1,
IOU_LABELS other than [0, -1, 1], PRE_NMS_TOPK_TRAIN above 4096 (for proposals; the losses do not need it), more than 1024 ground-truth boxes
per image or 2^22 anchors, rotated anchors, heads other than StandardRPNHead, PRE_NMS_TOPK_TEST above 1024, more than 16 anchors per cell,
more than 8 levels, CPU tensors, 2-byte features."""
import math

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import AfiError
from .frozen import cfg_get, check_feature, conv3x3, prepared
from .registry import detectron2_or_local

SCALE_CLAMP = math.log(1000.0 / 16)                    # Box2BoxTransform's _DEFAULT_SCALE_CLAMP


PROPOSAL_GENERATOR_REGISTRY = detectron2_or_local("detectron2.modeling.proposal_generator", "PROPOSAL_GENERATOR_REGISTRY", "RPN",
                                                  "PROPOSAL_GENERATOR")


def generate_cell_anchors(sizes, aspect_ratios):
    """DefaultAnchorGenerator.generate_cell_anchors: [len(sizes) len(ratios), 4] fp32 (x1, y1, x2, y2) around the origin, sizes then ratios."""
    out = []
    for size in sizes:
        area = float(size) ** 2.0
        for ratio in aspect_ratios:
            w = math.sqrt(area / ratio)
            h = ratio * w
            out.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
    return torch.tensor(out, dtype=torch.float32)


class BufferList(nn.Module):
    """detectron2's BufferList: buffers named "0", "1", ... (the state-dict keys ``cell_anchors.{l}``)."""

    def __init__(self, buffers):
        super().__init__()
        for i, b in enumerate(buffers):
            self.register_buffer(str(i), b)

    def __len__(self):
        return len(self._buffers)

    def __iter__(self):
        return iter(self._buffers.values())

    def __getitem__(self, i):
        return self._buffers[str(i)]


class DefaultAnchorGenerator(nn.Module):
    def __init__(self, sizes, aspect_ratios, strides, offset=0.0):
        super().__init__()
        n = len(strides)
        sizes, aspect_ratios = [list(s) for s in sizes], [list(r) for r in aspect_ratios]
        if len(sizes) == 1:
            sizes = sizes * n
        if len(aspect_ratios) == 1:
            aspect_ratios = aspect_ratios * n
        if len(sizes) != n or len(aspect_ratios) != n:
            raise AfiError(f"rpn: ANCHOR_GENERATOR.SIZES / ASPECT_RATIOS need one entry, or one per input feature ({n}); got {len(sizes)} / "
                           f"{len(aspect_ratios)}")
        if float(offset) != 0.0:
            raise AfiError(f"rpn: ANCHOR_GENERATOR.OFFSET {offset} is not supported (detectron2 v0.1.1 places anchors at offset 0)")
        self.strides = [int(s) for s in strides]
        self.cell_anchors = BufferList([generate_cell_anchors(s, r) for s, r in zip(sizes, aspect_ratios)])

    @property
    def num_cell_anchors(self):
        return [int(c.shape[0]) for c in self.cell_anchors]


class StandardRPNHead(nn.Module):
    def __init__(self, in_channels, num_cell_anchors, box_dim=4):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)
        self.objectness_logits = nn.Conv2d(in_channels, num_cell_anchors, kernel_size=1, stride=1)
        self.anchor_deltas = nn.Conv2d(in_channels, num_cell_anchors * box_dim, kernel_size=1, stride=1)
        for layer in (self.conv, self.objectness_logits, self.anchor_deltas):      # detectron2's initialisation
            nn.init.normal_(layer.weight, std=0.01)
            nn.init.constant_(layer.bias, 0)


class Boxes:
    """The part of detectron2's Boxes the detector path reads: ``.tensor`` [n, 4]."""

    def __init__(self, tensor):
        self.tensor = tensor

    def __len__(self):
        return self.tensor.shape[0]

    def to(self, device):
        return Boxes(self.tensor.to(device))


class Proposals:
    """One image's proposals when detectron2's Instances is not importable: ``image_size``, ``proposal_boxes``, ``objectness_logits``."""

    def __init__(self, image_size, proposal_boxes, objectness_logits):
        self.image_size, self.proposal_boxes, self.objectness_logits = image_size, proposal_boxes, objectness_logits

    def __len__(self):
        return len(self.proposal_boxes)

    def to(self, device):
        return Proposals(self.image_size, self.proposal_boxes.to(device), self.objectness_logits.to(device))


def _make_proposals(image_size, boxes, logits):
    try:
        from detectron2.structures import Boxes as D2Boxes, Instances
    except Exception:
        return Proposals(tuple(image_size), Boxes(boxes), logits)
    r = Instances(tuple(image_size))
    r.proposal_boxes = D2Boxes(boxes)
    r.objectness_logits = logits
    return r


def _wino(x, cout):
    """The regime rule of frozen.conv3x3 (stride 1): the Winograd form for >= 128 channels on both sides and >= 1024 pixels."""
    N, C, H, W = x.shape
    return C >= 128 and cout >= 128 and N * H * W >= 1024


class _RPNLossFn(torch.autograd.Function):
    """(loss_rpn_cls, loss_rpn_loc, head output per level) of the features and the six head parameters.  Forward: the head on the kernels the
    proposals are made from (frozen.conv3x3 + ReLU kept, one afi_conv1x1_fwd), afi_rpn_match / afi_rpn_sample / afi_rpn_loss, which also leave
    d loss / d head output.  Backward, per level: afi_conv1x1_dgrad on the concatenated 1x1 weight, afi_relu_bwd, afi_conv1x1_wgrad and the bias
    column sums (split back into objectness_logits and anchor_deltas), the 3x3 conv's weight and data gradients in the forward's regime; the
    shared head's weight gradients accumulate over the levels inside the kernels' own `dw +=`.  The head outputs are not differentiable here."""

    @staticmethod
    @_lib.ctx_forward
    def forward(ctx, rpn, gt, counts, keys, nlev, *ts):
        xs, A = [ops.pixel_major(x.detach()) for x in ts[:nlev]], rpn.num_anchors
        wcat, bcat, w3, b3 = rpn._prepare()
        acts, heads = [], []
        for x in xs:
            t = conv3x3(x, (w3, b3), relu=True)
            acts.append(t)
            heads.append(ops.conv1x1_fwd(t, wcat, bcat))
        ag, N = rpn.anchor_generator, xs[0].shape[0]
        cell = torch.stack(list(ag.cell_anchors)).contiguous()
        level_hw = [tuple(h.shape[2:]) for h in heads]
        labels, midx = ops.rpn_match(level_hw, ag.strides, cell, A, gt, counts, rpn.iou_thresholds)
        if keys is None:                                     # every 32-bit pattern equally likely, from torch's generator for this device
            keys = torch.randint(-2 ** 31, 2 ** 31, labels.shape, device=labels.device, dtype=torch.int32)
        labels, sidx, n_pos, n_neg = ops.rpn_sample(labels, keys, rpn.batch_size_per_image, rpn.positive_fraction)
        scale = rpn.loss_weight / (rpn.batch_size_per_image * N)
        loss, grads = ops.rpn_loss(heads, ag.strides, cell, A, gt, counts, midx, sidx, n_pos, n_neg, rpn.box_weights, rpn.smooth_l1_beta, scale, scale)
        ctx.save_for_backward(wcat, w3, *xs, *acts, *grads)
        ctx.nlev, ctx.A = nlev, A
        rpn.last_assignment = {"labels": labels, "matched_idx": midx, "sampled_idx": sidx, "n_pos": n_pos, "n_neg": n_neg}
        ctx.mark_non_differentiable(*heads)
        return (loss[0], loss[1], *heads)

    @staticmethod
    @_lib.ctx_backward
    def backward(ctx, dcls, dloc, *_):
        sv, L, A = ctx.saved_tensors, ctx.nlev, ctx.A
        wcat, w3 = sv[0], sv[1]
        xs, acts, grads = sv[2:2 + L], sv[2 + L:2 + 2 * L], sv[2 + 2 * L:2 + 3 * L]
        Cp, C_ = wcat.shape
        dev = wcat.device
        need = ctx.needs_input_grad
        need_w = any(need[5 + L:])
        # the kernel left d loss_cls / d logit in channels 0..A-1 and d loss_loc / d delta in A..5A-1: the two upstream scalars, per channel
        s = torch.zeros(Cp, device=dev, dtype=torch.float32)
        s[:A], s[A:5 * A] = dcls.float(), dloc.float()
        dwcat = torch.zeros((Cp, C_), device=dev, dtype=torch.float32)
        dbcat = torch.zeros((Cp,), device=dev, dtype=torch.float32)
        dw3 = ops.new_ohwi(C_, C_, 3, 3, dev)
        db3 = torch.zeros((C_,), device=dev, dtype=torch.float32)
        dxs = []
        for l in range(L):
            x, t = xs[l], acts[l]
            N, _, H, W = x.shape
            g = (grads[l].permute(0, 2, 3, 1) * s).permute(0, 3, 1, 2)      # on the [N][H][W][Cp] memory: the result is dense pixel-major
            du = ops.relu_bwd(ops.conv1x1_dgrad(g, wcat), t)
            wino = _wino(x, C_)
            if need_w:
                _lib.call("afi_conv1x1_wgrad", ops.view_of(g), ops.view_of(t), N, H, W, Cp, C_, ops._p(dwcat), 1.0, ops.stream_ptr())
                ops.colsum_accum(g.permute(0, 2, 3, 1).reshape(-1, Cp), dbcat)
                (ops.conv3x3_wino_wgrad if wino else ops.conv3x3_wgrad)(du, x, dw3)
                ops.colsum_accum(du.permute(0, 2, 3, 1).reshape(-1, C_), db3)
            dxs.append((ops.conv3x3_wino_dgrad if wino else ops.conv3x3_dgrad)(du, w3) if need[5 + l] else None)
        h = [dwcat[:A].reshape(A, C_, 1, 1), dbcat[:A], dwcat[A:5 * A].reshape(4 * A, C_, 1, 1), dbcat[A:5 * A], dw3, db3]
        return (None, None, None, None, None, *dxs, *[v if n else None for v, n in zip(h, need[5 + L:])])


@PROPOSAL_GENERATOR_REGISTRY.register()
class RPN(nn.Module):
    def __init__(self, cfg, input_shape):
        super().__init__()
        m = cfg.MODEL
        ag, r, pg = cfg_get(m, "ANCHOR_GENERATOR", None), cfg_get(m, "RPN", None), cfg_get(m, "PROPOSAL_GENERATOR", None)
        if r is None or ag is None:
            raise AfiError("rpn: the config has no MODEL.RPN / MODEL.ANCHOR_GENERATOR section (afigan_amd.config.get_cfg declares them)")
        if cfg_get(ag, "NAME", "DefaultAnchorGenerator") != "DefaultAnchorGenerator":
            raise AfiError(f"rpn: MODEL.ANCHOR_GENERATOR.NAME {ag.NAME!r} is not supported (DefaultAnchorGenerator only: rotated anchors are out of scope)")
        if cfg_get(r, "HEAD_NAME", "StandardRPNHead") != "StandardRPNHead":
            raise AfiError(f"rpn: MODEL.RPN.HEAD_NAME {r.HEAD_NAME!r} is not supported (StandardRPNHead only)")
        self.in_features = list(r.IN_FEATURES)
        missing = [f for f in self.in_features if f not in input_shape]
        if missing or not self.in_features:
            raise AfiError(f"rpn: MODEL.RPN.IN_FEATURES {self.in_features} are not all outputs of the backbone ({sorted(input_shape)})")
        if len(self.in_features) > ops.RPN_MAX_LEVELS:
            raise AfiError(f"rpn: at most {ops.RPN_MAX_LEVELS} input features, got {len(self.in_features)}")
        self.pre_nms_topk = int(cfg_get(r, "PRE_NMS_TOPK_TEST", 6000))
        if not 0 < self.pre_nms_topk <= ops.RPN_MAX_TOPK:
            raise AfiError(f"rpn: MODEL.RPN.PRE_NMS_TOPK_TEST {self.pre_nms_topk} is outside 1..{ops.RPN_MAX_TOPK}, the per-level list the selection "
                           f"kernels hold (detectron2's default of 6000 is above it; every reference config sets 1000)")
        self.post_nms_topk = int(cfg_get(r, "POST_NMS_TOPK_TEST", 1000))
        if self.post_nms_topk <= 0:
            raise AfiError(f"rpn: MODEL.RPN.POST_NMS_TOPK_TEST {self.post_nms_topk} must be positive")
        self.nms_thresh = float(cfg_get(r, "NMS_THRESH", 0.7))
        self.min_box_side_len = float(cfg_get(pg, "MIN_SIZE", 0))
        self.box_weights = tuple(float(w) for w in cfg_get(r, "BBOX_REG_WEIGHTS", (1.0, 1.0, 1.0, 1.0)))
        if len(self.box_weights) != 4 or min(self.box_weights) <= 0:
            raise AfiError(f"rpn: MODEL.RPN.BBOX_REG_WEIGHTS {self.box_weights} must be four positive numbers")
        shapes = [input_shape[f] for f in self.in_features]
        channels = {s.channels for s in shapes}
        if len(channels) != 1:
            raise AfiError(f"rpn: every input feature must have one channel count, got {sorted(channels)}")
        self.anchor_generator = DefaultAnchorGenerator(cfg_get(ag, "SIZES", [[32, 64, 128, 256, 512]]), cfg_get(ag, "ASPECT_RATIOS", [[0.5, 1.0, 2.0]]),
                                                       [s.stride for s in shapes], cfg_get(ag, "OFFSET", 0.0))
        na = set(self.anchor_generator.num_cell_anchors)
        if len(na) != 1:
            raise AfiError(f"rpn: every level must have the same number of cell anchors, got {self.anchor_generator.num_cell_anchors}")
        self.num_anchors = na.pop()
        if self.num_anchors > ops.RPN_MAX_ANCHORS:
            raise AfiError(f"rpn: {self.num_anchors} anchors per cell; at most {ops.RPN_MAX_ANCHORS} are supported")
        self.rpn_head = StandardRPNHead(channels.pop(), self.num_anchors)
        for p in self.parameters():
            p.requires_grad_(False)
        # ---- the training side (losses): read here, so that a config it cannot honour fails at construction
        self.pre_nms_topk_train = int(cfg_get(r, "PRE_NMS_TOPK_TRAIN", 12000))
        self.post_nms_topk_train = int(cfg_get(r, "POST_NMS_TOPK_TRAIN", 2000))
        self.iou_thresholds = tuple(float(t) for t in cfg_get(r, "IOU_THRESHOLDS", [0.3, 0.7]))
        if len(self.iou_thresholds) != 2 or not self.iou_thresholds[0] <= self.iou_thresholds[1]:
            raise AfiError(f"rpn: MODEL.RPN.IOU_THRESHOLDS {list(self.iou_thresholds)} must be two ascending numbers")
        if [int(v) for v in cfg_get(r, "IOU_LABELS", [0, -1, 1])] != [0, -1, 1]:
            raise AfiError(f"rpn: MODEL.RPN.IOU_LABELS {list(r.IOU_LABELS)} is not supported ([0, -1, 1] only)")
        if float(cfg_get(r, "BOUNDARY_THRESH", -1)) != -1:
            raise AfiError(f"rpn: MODEL.RPN.BOUNDARY_THRESH {r.BOUNDARY_THRESH} is not supported (-1 only: anchors that leave the image are kept)")
        self.batch_size_per_image = int(cfg_get(r, "BATCH_SIZE_PER_IMAGE", 256))
        self.positive_fraction = float(cfg_get(r, "POSITIVE_FRACTION", 0.5))
        if not 0 < self.batch_size_per_image <= ops.RPN_MAX_BATCH or not 0.0 <= self.positive_fraction <= 1.0:
            raise AfiError(f"rpn: MODEL.RPN.BATCH_SIZE_PER_IMAGE {self.batch_size_per_image} must be in 1..{ops.RPN_MAX_BATCH} and POSITIVE_FRACTION "
                           f"{self.positive_fraction} in 0..1")
        self.smooth_l1_beta = float(cfg_get(r, "SMOOTH_L1_BETA", 0.0))
        self.loss_weight = float(cfg_get(r, "LOSS_WEIGHT", 1.0))
        if self.smooth_l1_beta < 0:
            raise AfiError(f"rpn: MODEL.RPN.SMOOTH_L1_BETA {self.smooth_l1_beta} must not be negative")

    def trainable_(self, flag=True):
        """Turn the six head parameters into trainable ones (or back).  The prepared weights are rebuilt on the next call."""
        for p in self.parameters():
            p.requires_grad_(bool(flag))
        self._cat_key = None
        return self

    # ------------------------------------------------------------------ the head
    def _prepare(self):
        """The two 1x1 convs as one [Cpad, C] weight (logits, then deltas, zero rows up to a multiple of 4) and the 3x3 weight in the kernels'
        layout, rebuilt when a parameter changes."""
        h = self.rpn_head
        ts = [h.objectness_logits.weight, h.objectness_logits.bias, h.anchor_deltas.weight, h.anchor_deltas.bias, h.conv.weight, h.conv.bias]

        def build():
            A, C_ = self.num_anchors, h.conv.weight.shape[0]
            cpad = (5 * A + 3) // 4 * 4
            w = torch.zeros((cpad, C_), device=ts[0].device, dtype=torch.float32)
            b = torch.zeros((cpad,), device=ts[0].device, dtype=torch.float32)
            w[:A], w[A:5 * A] = ts[0].detach().reshape(A, C_), ts[2].detach().reshape(4 * A, C_)
            b[:A], b[A:5 * A] = ts[1].detach(), ts[3].detach()
            return w, b, ops.to_ohwi(ts[4].detach().float()), ts[5].detach().float().contiguous()
        return prepared(self, "cat", ts, build)

    def _check(self, features, train=False):
        """train: the call computes losses (ground truth was given), so gradients may flow; every other call is forward-only."""
        if not train and self.training and torch.is_grad_enabled():
            raise AfiError("rpn: the proposal generator is inference-only (frozen) without ground truth: call .eval(), or run it under "
                           "torch.no_grad(); a training-mode call needs gt_instances (RPN.losses)")
        missing = [f for f in self.in_features if f not in features]
        if missing:
            raise AfiError(f"rpn: features {missing} are missing (got {sorted(features)})")
        xs = [features[f] for f in self.in_features]
        for f, x in zip(self.in_features, xs):
            check_feature("rpn", f"feature {f}", x, "the proposal generator runs", "fp32 features only")
            if x.dim() != 4 or x.shape[1] != self.rpn_head.conv.weight.shape[1] or x.shape[0] != xs[0].shape[0]:
                raise AfiError(f"rpn: feature {f} has shape {tuple(x.shape)}; [N, {self.rpn_head.conv.weight.shape[1]}, H, W] expected")
            if not train and torch.is_grad_enabled() and x.requires_grad:
                raise AfiError("rpn: the proposal generator is forward-only: run it under torch.no_grad() or detach its inputs")
        return xs

    def head(self, features):
        """Per level, the pixel-major head output [N, Cpad, H, W]: channels 0..A-1 the objectness logits, A..5A-1 the anchor deltas."""
        xs = self._check(features)
        with torch.no_grad():
            wcat, bcat, w3, b3 = self._prepare()
            outs = []
            for x in xs:
                t = conv3x3(ops.pixel_major(x), (w3, b3), relu=True)
                outs.append(ops.conv1x1_fwd(t, wcat, bcat))
        return outs

    # ------------------------------------------------------------------ selection
    def select(self, heads, image_hw, pre_k=None, post_k=None):
        """top-k, decode, NMS per level and the merge, on the head outputs; image_hw [N, 2] fp32 on the device.  Returns a dict with the padded
        result (boxes [N, post_k, 4], logits [N, post_k], counts [N] int32) and the stages' own outputs with the levels side by side
        (level_off, vals / idx / valid / keep [N, K], level_boxes [N, K, 4]).  pre_k / post_k: the *_TEST values unless given.  A level whose
        list min(pre_k, H W A) is longer than ops.RPN_MAX_TOPK (up to ops.RPN_MAX_TOPK_WIDE) runs the wide top-k and NMS, and the merge is then
        the wide one; every other level runs the calls it always ran."""
        A, N, dev = self.num_anchors, heads[0].shape[0], heads[0].device
        pre_k, post_k = pre_k or self.pre_nms_topk, post_k or self.post_nms_topk
        ks = [min(pre_k, o.shape[2] * o.shape[3] * A) for o in heads]
        off = [0]
        for k in ks:
            off.append(off[-1] + k)
        K = off[-1]
        vals = torch.empty((N, K), device=dev, dtype=torch.float32)
        idx = torch.empty((N, K), device=dev, dtype=torch.int32)
        boxes = torch.empty((N, K, 4), device=dev, dtype=torch.float32)
        valid = torch.empty((N, K), device=dev, dtype=torch.int32)
        keep = torch.empty((N, K), device=dev, dtype=torch.int32)
        for l, (o, k) in enumerate(zip(heads, ks)):
            s = slice(off[l], off[l + 1])
            wide = k > ops.RPN_MAX_TOPK                      # a list the LDS-resident kernels cannot hold: the wide forms, this level only
            (ops.rpn_topk_wide if wide else ops.rpn_topk)(o, A, k, vals[:, s], idx[:, s])
            ops.rpn_decode(o, A, A, self.anchor_generator.cell_anchors[l], self.anchor_generator.strides[l], idx[:, s], k, image_hw,
                           self.box_weights, SCALE_CLAMP, self.min_box_side_len, boxes[:, s], valid[:, s])
            (ops.rpn_nms_wide if wide else ops.rpn_nms)(boxes[:, s], valid[:, s], self.nms_thresh, keep[:, s])
        merge = ops.rpn_merge_wide if max(ks) > ops.RPN_MAX_TOPK else ops.rpn_merge
        ob, ol, counts = merge(boxes, vals, keep, off, post_k)
        return {"boxes": ob, "logits": ol, "counts": counts, "level_off": off, "vals": vals, "idx": idx, "level_boxes": boxes, "valid": valid,
                "keep": keep}

    def forward_padded(self, image_sizes, features, intermediates=False):
        """(boxes [N, post_k, 4], logits [N, post_k], counts [N] int32) on the device, rows past counts zero; image_sizes: [N, 2] device tensor
        (height, width) of the un-padded images.  No host read: capturable in a hipGraph.  intermediates: the dict of ``select`` instead."""
        heads = self.head(features)
        if not torch.is_tensor(image_sizes) or not image_sizes.is_cuda:
            raise AfiError("rpn: forward_padded takes the image sizes as an [N, 2] tensor on the GPU (forward() takes a list)")
        if tuple(image_sizes.shape) != (heads[0].shape[0], 2):
            raise AfiError(f"rpn: image sizes of shape {tuple(image_sizes.shape)} for a batch of {heads[0].shape[0]}")
        with torch.no_grad():
            r = self.select(heads, image_sizes.to(torch.float32).contiguous())
        return r if intermediates else (r["boxes"], r["logits"], r["counts"])

    # ------------------------------------------------------------------ training
    def _ground_truth(self, gt_instances, N, device):
        """The images' boxes as one padded [N, Gmax, 4] fp32 tensor and counts [N] int32 on the device; the counts come from the shapes."""
        if len(gt_instances) != N:
            raise AfiError(f"rpn: {len(gt_instances)} gt_instances for a batch of {N}")
        boxes = []
        for g in gt_instances:
            b = getattr(g, "gt_boxes", None)
            b = getattr(b, "tensor", b)
            if not torch.is_tensor(b) or b.dim() != 2 or b.shape[1] != 4:
                raise AfiError("rpn: every element of gt_instances needs gt_boxes, a Boxes or an [G, 4] tensor")
            boxes.append(b)
        gmax = max(b.shape[0] for b in boxes)
        if gmax > ops.RPN_MAX_GT:
            raise AfiError(f"rpn: {gmax} ground-truth boxes in one image; at most {ops.RPN_MAX_GT} are supported")
        gt = torch.zeros((N, max(gmax, 1), 4), device=device, dtype=torch.float32)
        for n, b in enumerate(boxes):
            if b.shape[0]:
                gt[n, :b.shape[0]] = b.detach().to(device=device, dtype=torch.float32)
        return gt, torch.tensor([b.shape[0] for b in boxes], dtype=torch.int32).to(device)

    def _losses_and_heads(self, features, gt_instances, keys):
        xs = self._check(features, train=True)
        gt, counts = self._ground_truth(gt_instances, xs[0].shape[0], xs[0].device)
        h = self.rpn_head
        out = _RPNLossFn.apply(self, gt, counts, keys, len(xs), *xs, h.objectness_logits.weight, h.objectness_logits.bias, h.anchor_deltas.weight,
                               h.anchor_deltas.bias, h.conv.weight, h.conv.bias)
        return {"loss_rpn_cls": out[0], "loss_rpn_loc": out[1]}, list(out[2:])

    def losses(self, images, features, gt_instances, keys=None):
        """{"loss_rpn_cls", "loss_rpn_loc"} of detectron2's RPN in training, differentiable in the features and, after ``trainable_()``, the six
        head parameters.  keys: [N, R] 32-bit integers on the device that decide the sample (the anchors with the smallest (key, index) are
        taken); drawn from torch's generator when None.  The label assignment and sample of the call stay in ``last_assignment``.  Works in
        either mode and whatever the *_TOPK_TRAIN values are: no proposal is made.  No host read."""
        return self._losses_and_heads(features, gt_instances, keys)[0]

    def _forward_train(self, images, features, gt_instances, keys=None):
        if self.pre_nms_topk_train > ops.RPN_MAX_TOPK_WIDE:
            raise AfiError(f"rpn: MODEL.RPN.PRE_NMS_TOPK_TRAIN {self.pre_nms_topk_train} is above both {ops.RPN_MAX_TOPK}, the per-level list the "
                           f"selection kernels hold in LDS, and {ops.RPN_MAX_TOPK_WIDE}, the list their wide forms hold through a workspace, so a "
                           "training-mode forward cannot make proposals (the reference's base config sets 2000, which runs; detectron2's default "
                           "is 12000).  RPN.losses() works regardless; lists above "
                           f"{ops.RPN_MAX_TOPK_WIDE} are a separate piece of work")
        if self.post_nms_topk_train <= 0 or self.pre_nms_topk_train <= 0:
            raise AfiError(f"rpn: MODEL.RPN.PRE_NMS_TOPK_TRAIN / POST_NMS_TOPK_TRAIN {self.pre_nms_topk_train} / {self.post_nms_topk_train} must be positive")
        losses, heads = self._losses_and_heads(features, gt_instances, keys)
        sizes = [(int(h), int(w)) for h, w in images.image_sizes]
        if len(sizes) != heads[0].shape[0]:
            raise AfiError(f"rpn: {len(sizes)} image sizes for a batch of {heads[0].shape[0]}")
        with torch.no_grad():                                 # the proposals carry no gradient (detectron2 detaches them too)
            r = self.select([h.detach() for h in heads], torch.tensor(sizes, dtype=torch.float32).to(heads[0].device), self.pre_nms_topk_train,
                            self.post_nms_topk_train)
        props = [_make_proposals(sz, r["boxes"][n, :c], r["logits"][n, :c]) for n, (sz, c) in enumerate(zip(sizes, r["counts"].tolist()))]
        return props, losses

    def forward(self, images, features, gt_instances=None, keys=None):
        """detectron2's RPN.forward: (one proposals object per image -- image_size, proposal_boxes, objectness_logits, sorted by logit --,
        losses).  At inference the losses are {}; in training mode with gt_instances they are ``losses()``' (keys: as there) and the proposals
        come from the same head outputs at the *_TOPK_TRAIN values.  One device-to-host read, of the counts."""
        if gt_instances is not None:
            if not self.training:
                raise AfiError("rpn: gt_instances given to a module in eval mode -- call .train() for (proposals, losses), or RPN.losses() for the "
                               "losses alone")
            return self._forward_train(images, features, gt_instances, keys)
        xs = self._check(features)
        sizes = [(int(h), int(w)) for h, w in images.image_sizes]
        if len(sizes) != xs[0].shape[0] or len(images) != len(sizes):
            raise AfiError(f"rpn: {len(sizes)} image sizes for a batch of {xs[0].shape[0]}")
        hw = torch.tensor(sizes, dtype=torch.float32).to(xs[0].device)
        boxes, logits, counts = self.forward_padded(hw, features)
        return [_make_proposals(sz, boxes[n, :c], logits[n, :c]) for n, (sz, c) in enumerate(zip(sizes, counts.tolist()))], {}


def build_proposal_generator(cfg, input_shape):
    """detectron2's build_proposal_generator: None for precomputed proposals, else the registered class."""
    name = cfg_get(cfg_get(cfg.MODEL, "PROPOSAL_GENERATOR", None), "NAME", "RPN")
    if name == "PrecomputedProposals":
        return None
    try:
        cls = PROPOSAL_GENERATOR_REGISTRY.get(name)
    except KeyError:
        raise AfiError(f"rpn: no proposal generator named {name!r} (this package provides 'RPN')")
    return cls(cfg, input_shape)
