"""The frozen guide network of stages 1 and 2 as detectron2 builds it: ``build_resnet_fpn_backbone`` (a ResNet bottom-up with FrozenBN under an
FPN with LastLevelMaxPool), forward only, on this package's HIP kernels.  ``RCNN_FPN_only`` (rcnn_only.py) looks the builder up by
``cfg.MODEL.GUIDE_BACKBONE.NAME``; the reference loads ``MODEL.GUIDE_WEIGHTS``, a detectron2 model-zoo file, into it
(stage1_trainer.py:62-74: checkpoint.load_guide_weights here).

The parameter tree and key names are detectron2's (``bottom_up.stem.conv1.{weight,norm.*}``, ``bottom_up.res{2..5}.{i}.{conv1..3,shortcut}.*``,
``fpn_lateral{k}.*``, ``fpn_output{k}.*``), so ``RCNN_FPN_only.backbone.*`` takes a model-zoo file's ``backbone.*`` tensors as they are.
Each FrozenBatchNorm2d (eps 1e-5) is folded into its conv once, in fp64, and refolded when a parameter or buffer changes.

Kernels: the stem (7x7/2 conv + ReLU + 3x3/2 max-pool) is afi_resnet_stem_fwd; every 1x1 conv (conv1, conv3 with the residual add + ReLU in its
epilogue, shortcuts, FPN laterals with the top-down addend) afi_conv1x1_fwd, stride 2 read as a strided view; 3x3 convs afi_conv3x3_fwd or, with
>= 128 channels on both sides, afi_conv3x3_wino_infer; the stride-2 3x3 of STRIDE_IN_1X1 = False afi_conv3x3s2_fwd; the x2 nearest top-down
up-sampling and p6 afi_nearest_nhwc.  No MIOpen, hipBLASLt or torch conv / pool / interpolate kernel runs.

Out of scope (AfiError at build time): dilation, groups > 1, deformable convs, norms other than FrozenBN, a normalised FPN, the ResNeSt
options; at call time, a forward that autograd could differentiate."""
import torch
import torch.nn as nn

from . import ops, registry
from ._lib import AfiError
from .fpn_sr import ShapeSpec
from .frozen import FROZEN_BN_EPS, Conv2d, FrozenBatchNorm2d, cfg_get, check_forward_only, conv1x1, conv3x3, prepared  # noqa: F401

_BLOCKS = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3]}


class _Frozen(nn.Module):
    """Folded weights of the convs this module runs itself, rebuilt when a parameter / buffer of them changes (frozen.prepared)."""
    what = "the ResNet-FPN guide"

    def _own_convs(self):
        raise NotImplementedError

    def _fold_own(self, convs):
        return {id(m): m.fold() for m in convs}

    def _prepare(self):
        convs = self._own_convs()
        ts = [t for m in convs for t in list(m.parameters()) + list(m.buffers())]
        return prepared(self, "folded", ts, lambda: self._fold_own(convs))


class BasicStem(nn.Module):
    def __init__(self, in_channels=3, out_channels=64):
        super().__init__()
        self.conv1 = Conv2d(in_channels, out_channels, 7, stride=2)

    def run(self, x, f):
        return ops.resnet_stem(x, *f[id(self.conv1)])


class BottleneckBlock(nn.Module):
    """detectron2's BottleneckBlock (groups 1, dilation 1): relu(conv3(relu(conv2(relu(conv1(x))))) + shortcut(x))."""

    def __init__(self, cin, cout, bottleneck, stride, stride_in_1x1):
        super().__init__()
        self.shortcut = Conv2d(cin, cout, 1, stride=stride) if cin != cout else None
        s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)
        self.conv1 = Conv2d(cin, bottleneck, 1, stride=s1)
        self.conv2 = Conv2d(bottleneck, bottleneck, 3, stride=s3)
        self.conv3 = Conv2d(bottleneck, cout, 1)

    def run(self, x, f):
        s = x if self.shortcut is None else conv1x1(x, f[id(self.shortcut)], self.shortcut.stride)
        y = conv1x1(x, f[id(self.conv1)], self.conv1.stride, relu=True)
        y = conv3x3(y, f[id(self.conv2)], self.conv2.stride, relu=True)
        return conv1x1(y, f[id(self.conv3)], add=s, relu=True)


class ResNetBase(_Frozen):
    """What the ResNet and ResNeSt bottom-ups share: a stem (4x down) and the stages res2.. of bottleneck blocks, each twice as wide and, from
    res3 on, half the size; ``forward(x [N,3,H,W]) -> {name: pixel-major fp32 features}`` for ``out_features`` (subset of stem, res2..res5)."""
    STAGES = ["stem", "res2", "res3", "res4", "res5"]

    @classmethod
    def _num_stages(cls, prefix, out_features):
        if not out_features or any(f not in cls.STAGES for f in out_features):
            raise AfiError(f"{prefix}: unknown RESNETS.OUT_FEATURES {list(out_features)}")
        return max(cls.STAGES.index(f) for f in out_features)

    def _build(self, out_features, stem, stem_channels, counts, res2_out_channels, width, block):
        """`counts` blocks per stage, each ``block(stage, cin, cout, width, stride)``; `width` (the bottleneck's) doubles per stage."""
        self._out_features = list(out_features)
        self.stem = stem
        self._out_feature_channels, self._out_feature_strides = {"stem": stem_channels}, {"stem": 4}
        cin, cout = stem_channels, res2_out_channels
        self.stage_names = []
        for i, n in enumerate(counts):
            name, first = f"res{i + 2}", (1 if i == 0 else 2)
            blocks = [block(i + 2, cin if j == 0 else cout, cout, width, first if j == 0 else 1) for j in range(n)]
            self.add_module(name, nn.Sequential(*blocks))
            self.stage_names.append(name)
            self._out_feature_channels[name], self._out_feature_strides[name] = cout, 4 * 2 ** i
            cin, cout, width = cout, 2 * cout, 2 * width

    @property
    def size_divisibility(self):
        return 0

    def output_shape(self):
        return {n: ShapeSpec(channels=self._out_feature_channels[n], stride=self._out_feature_strides[n]) for n in self._out_features}

    def forward(self, x):
        check_forward_only(self, x, self.what)
        with torch.no_grad():
            f = self._prepare()
            out = {}
            y = self.stem.run(x.float(), f)
            if "stem" in self._out_features:
                out["stem"] = y
            for name in self.stage_names:
                for blk in getattr(self, name):
                    y = blk.run(y, f)
                if name in self._out_features:
                    out[name] = y
        return out


class ResNet(ResNetBase):
    """The bottom-up of detectron2's ResNet-50 / -101 (see ResNetBase for the forward)."""

    def __init__(self, depth=50, out_features=("res2", "res3", "res4", "res5"), stride_in_1x1=True, width_per_group=64,
                 res2_out_channels=256, stem_out_channels=64):
        super().__init__()
        if depth not in _BLOCKS:
            raise AfiError(f"resnet_guide: RESNETS.DEPTH {depth} is not supported (50 or 101)")
        if stem_out_channels != 64:
            raise AfiError(f"resnet_guide: RESNETS.STEM_OUT_CHANNELS {stem_out_channels} is not supported (the stem kernel makes 64)")
        n_stages = self._num_stages("resnet_guide", out_features)
        if (width_per_group % 4) or (res2_out_channels % 4):
            raise AfiError("resnet_guide: channel counts must be multiples of 4")
        self._build(out_features, BasicStem(3, 64), 64, _BLOCKS[depth][:n_stages], res2_out_channels, width_per_group,
                    lambda stage, cin, cout, width, stride: BottleneckBlock(cin, cout, width, stride, stride_in_1x1))

    def _own_convs(self):
        return [m for m in self.modules() if isinstance(m, Conv2d)]


class LastLevelMaxPool(nn.Module):
    """detectron2's top block: p6 = max_pool2d(p5, kernel_size=1, stride=2) (a stride-2 subsampling)."""

    def __init__(self):
        super().__init__()
        self.num_levels, self.in_feature = 1, "p5"


class FPN(_Frozen):
    """detectron2's FPN over a ResNet with LastLevelMaxPool: ``forward(x) -> {"p2".."p6"}`` (pixel-major), fuse "sum" or "avg"."""

    def __init__(self, bottom_up, in_features, out_channels=256, fuse_type="sum"):
        super().__init__()
        if fuse_type not in ("sum", "avg"):
            raise AfiError(f"resnet_guide: FPN.FUSE_TYPE {fuse_type!r} is not supported (sum or avg)")
        shapes = bottom_up.output_shape()
        missing = [f for f in in_features if f not in shapes]
        if missing:
            raise AfiError(f"resnet_guide: FPN.IN_FEATURES {missing} are not among RESNETS.OUT_FEATURES {list(shapes)}")
        strides = [shapes[f].stride for f in in_features]
        if any(b != 2 * a for a, b in zip(strides, strides[1:])):
            raise AfiError(f"resnet_guide: FPN.IN_FEATURES {list(in_features)} are not consecutive stages")
        self.bottom_up, self.in_features, self._fuse_type = bottom_up, list(in_features), fuse_type
        self.lateral_convs, self.output_convs = [], []
        for f in self.in_features:
            k = shapes[f].stride.bit_length() - 1
            lat = Conv2d(shapes[f].channels, out_channels, 1, bias=True, norm=False)
            out = Conv2d(out_channels, out_channels, 3, bias=True, norm=False)
            self.add_module(f"fpn_lateral{k}", lat)
            self.add_module(f"fpn_output{k}", out)
            self.lateral_convs.insert(0, lat)                          # top (coarsest) first, as detectron2 keeps them
            self.output_convs.insert(0, out)
        self.top_block = LastLevelMaxPool()
        top = strides[-1].bit_length() - 1
        self._out_features = [f"p{s.bit_length() - 1}" for s in strides] + [f"p{top + 1}"]
        self._out_feature_strides = {f"p{s.bit_length() - 1}": s for s in strides + [2 * strides[-1]]}
        self._out_feature_channels = {k: out_channels for k in self._out_features}
        self._size_divisibility = strides[-1]

    @property
    def size_divisibility(self):
        return self._size_divisibility

    def output_shape(self):
        return {n: ShapeSpec(channels=self._out_feature_channels[n], stride=self._out_feature_strides[n]) for n in self._out_features}

    def _own_convs(self):
        return self.lateral_convs + self.output_convs

    def _fold_own(self, convs):
        f = super()._fold_own(convs)
        if self._fuse_type == "avg":
            for m in self.lateral_convs[1:]:                               # (lat + top-down) / 2 = 0.5 conv + 0.5 bias + 0.5 top-down
                f[("avg", id(m))] = m.fold(scale=0.5)
        return f

    def forward(self, x):
        check_forward_only(self, x, self.what)
        feats = self.bottom_up(x)
        with torch.no_grad():
            f = self._prepare()
            xs = [feats[k] for k in self.in_features[::-1]]
            prev = conv1x1(xs[0], f[id(self.lateral_convs[0])])
            results = [conv3x3(prev, f[id(self.output_convs[0])])]
            for feat, lat, out in zip(xs[1:], self.lateral_convs[1:], self.output_convs[1:]):
                td = ops.nearest(prev, up=2)
                if self._fuse_type == "avg":
                    prev = conv1x1(feat, f[("avg", id(lat))], add=td, alpha=0.5, add_scale=0.5)
                else:
                    prev = conv1x1(feat, f[id(lat)], add=td)
                results.insert(0, conv3x3(prev, f[id(out)]))
            results.append(ops.nearest(results[-1], up=1, down=2))          # LastLevelMaxPool on the coarsest output
        return dict(zip(self._out_features, results))


def _resnet_from_cfg(cfg, input_shape=None):
    """detectron2's build_resnet_backbone restricted to the frozen, forward-only guide: refuses every option it does not implement."""
    r = cfg_get(cfg.MODEL, "RESNETS", None)
    if input_shape is not None and getattr(input_shape, "channels", 3) not in (None, 3):
        raise AfiError(f"resnet_guide: 3 input channels only, got {input_shape.channels}")
    norm = cfg_get(r, "NORM", "FrozenBN")
    if norm != "FrozenBN":
        raise AfiError(f"resnet_guide: RESNETS.NORM {norm!r} is not supported (the frozen guide folds FrozenBN)")
    if cfg_get(r, "NUM_GROUPS", 1) != 1:
        raise AfiError(f"resnet_guide: RESNETS.NUM_GROUPS {cfg_get(r, 'NUM_GROUPS', 1)} is not supported (groups = 1 only)")
    if cfg_get(r, "RES5_DILATION", 1) != 1:
        raise AfiError(f"resnet_guide: RESNETS.RES5_DILATION {cfg_get(r, 'RES5_DILATION', 1)} is not supported (no dilation)")
    if any(cfg_get(r, "DEFORM_ON_PER_STAGE", [False] * 4)):
        raise AfiError("resnet_guide: deformable convolutions (RESNETS.DEFORM_ON_PER_STAGE) are not supported")
    if cfg_get(r, "RADIX", 1) != 1 or cfg_get(r, "DEEP_STEM", False) or cfg_get(r, "AVD", False) or cfg_get(r, "AVG_DOWN", False):
        raise AfiError("resnet_guide: the ResNeSt options (RESNETS.RADIX / DEEP_STEM / AVD / AVG_DOWN) are not supported")
    return ResNet(depth=cfg_get(r, "DEPTH", 50), out_features=list(cfg_get(r, "OUT_FEATURES", ["res4"])),
                  stride_in_1x1=bool(cfg_get(r, "STRIDE_IN_1X1", True)), width_per_group=cfg_get(r, "WIDTH_PER_GROUP", 64),
                  res2_out_channels=cfg_get(r, "RES2_OUT_CHANNELS", 256), stem_out_channels=cfg_get(r, "STEM_OUT_CHANNELS", 64))


def build_resnet_backbone(cfg, input_shape=None):
    """The frozen ResNet bottom-up alone, for ``registry.set_bottom_up_builder("resnet", build_resnet_backbone)`` (opt-in: see use_as_bottom_up)."""
    return _resnet_from_cfg(cfg, input_shape)


def build_resnet_fpn_backbone(cfg, input_shape=None):
    """detectron2's build_resnet_fpn_backbone (ResNet + FPN + LastLevelMaxPool) as the frozen guide of stages 1 and 2."""
    fpn = cfg_get(cfg.MODEL, "FPN", None)
    if cfg_get(fpn, "NORM", "") != "":
        raise AfiError(f"resnet_guide: FPN.NORM {cfg_get(fpn, 'NORM', '')!r} is not supported (the guide's FPN has biased convs, no norm)")
    return FPN(_resnet_from_cfg(cfg, input_shape), list(cfg_get(fpn, "IN_FEATURES", ["res2", "res3", "res4", "res5"])),
               cfg_get(fpn, "OUT_CHANNELS", 256), cfg_get(fpn, "FUSE_TYPE", "sum"))


def use_as_bottom_up():
    """Opt in: the AFI backbones' "resnet" bottom-up lookup (registry.bottom_up_builder) returns this frozen, forward-only ResNet."""
    registry.set_bottom_up_builder("resnet", build_resnet_backbone)


REGISTERED = registry.register_local_backbone(build_resnet_fpn_backbone)        # (with detectron2 installed the name is detectron2's)
