"""The frozen ResNeSt bottom-up of the reference's best models (detectron2-ResNeSt's ``build_resnest_backbone``: resnest.py, splat.py),
forward only, on this package's HIP kernels -- as the AFI backbone's bottom-up for inference (``use_as_bottom_up``, then
``build_resnest_{fpn,pafpn}_sr_backbone``) and, under resnet_guide's FPN, as a stage-1/2 guide (``build_resnest_fpn_backbone``).

ResNeSt is the ResNet of resnet_guide.py plus four pieces, all forced on by ``RESNETS.RADIX`` 2 (resnest.py:493,523-524):
  - a deep stem: conv 3x3/2 (3 -> sw), conv 3x3 (sw -> sw), conv 3x3 (sw -> 2 sw), each with a norm and a ReLU, then max_pool2d(3, 2, 1);
    sw (the stem width) is 32 for depth 50 and 64 for depth 101, and STEM_OUT_CHANNELS is not read;
  - split-attention 3x3 convs (SplAtConv2d, radix 2, cardinality 1): a 2-group conv (group r reads input channels [r gw/2, (r+1) gw/2) and
    writes split r) + bn0 + ReLU; gap = mean_HW(split0 + split1); fc1 + bn1 + ReLU; fc2; softmax over each pair (c, gw + c);
    out = a0 split0 + a1 split1;
  - AVD: AvgPool2d(3, 2, padding 1) after the split-attention conv of a stride-2 block (whose 3x3 conv then has stride 1);
  - avg_down: the shortcut is AvgPool2d(stride, stride, ceil_mode, count_include_pad=False) followed by the 1x1 conv and its norm.
A block is relu(conv3(avd(splat(relu(conv1(x))))) + shortcut(x)).

The parameter tree and key names are detectron2-ResNeSt's (``stem.conv1_{1,2,3}.{weight,norm.*}``, ``res{k}.{i}.conv1.*``,
``conv2.conv.weight``, ``conv2.bn0.*``, ``conv2.fc1.{weight,bias}``, ``conv2.bn1.*``, ``conv2.fc2.*``, ``conv3.*``, ``shortcut.*``), and so is
the freezing: with ``BACKBONE.FREEZE_AT`` = k the stem (k >= 1) and the stages res2..res{k} carry FrozenBatchNorm2d, later norms the
config's type (BN / SyncBN, with ``num_batches_tracked``), so a trained checkpoint's key set matches exactly.  Every norm is folded into its
conv (fp64, frozen.fold_conv), whatever its type: the module only runs in inference.

Kernels: the stem's first conv afi_resnest_stem_fwd; the other 3x3 convs afi_conv3x3_fwd / afi_conv3x3_wino_infer, chosen as
frozen.conv3x3 chooses (a split-attention conv: one launch per radix group, through channel views of its input, each writing its
own split); every 1x1 conv afi_conv1x1_fwd (conv3 with the shortcut add and the ReLU in its epilogue); the stem pool and the avg_down pool
afi_resnest_pool_nhwc; split attention afi_resnest_splat_gap / _attn / _combine (AVD fused into the combine).  No MIOpen, hipBLASLt or
torch conv / pool kernel runs, and no atomics: the forward is bit-identical from run to run and under hipGraph replay.

Out of scope (AfiError at build time): radix != 2, NUM_GROUPS > 1, dilation, deformable convs, norms other than FrozenBN / BN / SyncBN,
STRIDE_IN_1X1 = True; at call time, a CPU tensor and a forward that autograd could differentiate."""
import torch.nn as nn

from . import frozen, ops, registry
from ._lib import AfiError
from .frozen import FrozenBatchNorm2d, cfg_get, conv1x1, conv3x3, fold_conv
from .resnet_guide import FPN, ResNetBase

_BLOCKS = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3]}
_STEM_WIDTH = {50: 32, 101: 64}
NORMS = ("FrozenBN", "BN", "SyncBN")


def _norm(kind, channels):
    """detectron2's get_norm for the norms this module folds: FrozenBN, or BN / SyncBN (nn.BatchNorm2d / nn.SyncBatchNorm, frozen here)."""
    if kind == "FrozenBN":
        return FrozenBatchNorm2d(channels)
    m = nn.BatchNorm2d(channels) if kind == "BN" else nn.SyncBatchNorm(channels)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


class Conv2d(frozen.Conv2d):
    """frozen.Conv2d with the norm of the given kind ("" / None: no norm)."""

    def __init__(self, cin, cout, k, stride=1, bias=False, norm="FrozenBN"):
        super().__init__(cin, cout, k, stride=stride, bias=bias, norm=False)
        self.norm = _norm(norm, cout) if norm else None


class SplAtConv2d(nn.Module):
    """splat.py's SplAtConv2d for radix 2, cardinality 1, stride 1, no dilation / rectify / DropBlock."""

    def __init__(self, channels, norm):
        super().__init__()
        self.radix, self.channels = 2, channels
        inter = max(channels * self.radix // 4, 32)
        self.conv = Conv2d(channels // 2, channels * self.radix, 3, norm=None)          # groups = radix
        self.bn0 = _norm(norm, channels * self.radix)
        self.fc1 = Conv2d(channels, inter, 1, bias=True, norm=None)
        self.bn1 = _norm(norm, inter)
        self.fc2 = Conv2d(inter, channels * self.radix, 1, bias=True, norm=None)

    def fold(self):
        return fold_conv(self.conv, self.bn0), fold_conv(self.fc1, self.bn1), self.fc2.fold()      # (bn0 / bn1 stand beside their convs)

    def run(self, y, f, avd):
        (wc, bc), (w1, b1), (w2, b2) = f[id(self)]
        g = self.channels
        s0 = conv3x3(y[:, :g // 2], (wc[:g], bc[:g]), relu=True)
        s1 = conv3x3(y[:, g // 2:], (wc[g:], bc[g:]), relu=True)
        return ops.splat_attention(s0, s1, w1, b1, w2, b2, avd=avd)[0]


class DeepStem(nn.Module):
    def __init__(self, stem_width, norm):
        super().__init__()
        self.conv1_1 = Conv2d(3, stem_width, 3, stride=2, norm=norm)
        self.conv1_2 = Conv2d(stem_width, stem_width, 3, norm=norm)
        self.conv1_3 = Conv2d(stem_width, 2 * stem_width, 3, norm=norm)

    def run(self, x, f):
        y = ops.resnest_stem(x, *f[id(self.conv1_1)])
        y = conv3x3(y, f[id(self.conv1_2)], relu=True)
        y = conv3x3(y, f[id(self.conv1_3)], relu=True)
        return ops.resnest_pool(y, "max3s2p1")


class BottleneckBlock(nn.Module):
    """resnest.py's BottleneckBlock with radix 2 (so AVD and avg_down on), STRIDE_IN_1X1 False, groups 1, dilation 1."""

    def __init__(self, cin, cout, group_width, stride, norm):
        super().__init__()
        self.stride, self.avd, self.avg_down, self.radix = stride, stride > 1, True, 2
        self.shortcut = Conv2d(cin, cout, 1, norm=norm) if cin != cout else None
        self.conv1 = Conv2d(cin, group_width, 1, norm=norm)
        self.conv2 = SplAtConv2d(group_width, norm)
        self.conv3 = Conv2d(group_width, cout, 1, norm=norm)

    def run(self, x, f):
        if self.shortcut is None:
            s = x
        else:
            xs = ops.resnest_pool(x, "avg2s2_ceil") if self.stride == 2 else x           # (AvgPool2d(1, 1) is the identity)
            s = conv1x1(xs, f[id(self.shortcut)])
        y = conv1x1(x, f[id(self.conv1)], relu=True)
        y = self.conv2.run(y, f, self.avd)
        return conv1x1(y, f[id(self.conv3)], add=s, relu=True)


class ResNeSt(ResNetBase):
    """The bottom-up of detectron2-ResNeSt's ResNeSt-50 / -101 (see ResNetBase for the forward)."""
    what = "the ResNeSt bottom-up"

    def __init__(self, depth=50, out_features=("res2", "res3", "res4", "res5"), norm="FrozenBN", freeze_at=2, width_per_group=64,
                 bottleneck_width=64, res2_out_channels=256):
        super().__init__()
        if depth not in _BLOCKS:
            raise AfiError(f"resnest_backbone: RESNETS.DEPTH {depth} is not supported (50 or 101)")
        if norm not in NORMS:
            raise AfiError(f"resnest_backbone: RESNETS.NORM {norm!r} is not supported (one of {', '.join(NORMS)}: folded into the convs)")
        n_stages = self._num_stages("resnest_backbone", out_features)
        group_width = int(width_per_group * (bottleneck_width / 64.0))
        if group_width % 8 or group_width * 2 ** (n_stages - 1) > 1024 or res2_out_channels % 4:
            raise AfiError(f"resnest_backbone: group width {group_width} (a multiple of 8, at most 1024 in res5) and RES2_OUT_CHANNELS "
                           f"{res2_out_channels} (a multiple of 4) are required")
        sw = _STEM_WIDTH[depth]
        norm_of = lambda stage: "FrozenBN" if freeze_at >= stage else norm          # noqa: E731  (the stem is stage 1)
        self._build(out_features, DeepStem(sw, norm_of(1)), 2 * sw, _BLOCKS[depth][:n_stages], res2_out_channels, group_width,
                    lambda stage, cin, cout, gw, stride: BottleneckBlock(cin, cout, gw, stride, norm_of(stage)))

    def _own_convs(self):
        convs = [self.stem.conv1_1, self.stem.conv1_2, self.stem.conv1_3]
        for name in self.stage_names:
            for blk in getattr(self, name):
                convs += [m for m in (blk.shortcut, blk.conv1, blk.conv2, blk.conv3) if m is not None]
        return convs


def _resnest_from_cfg(cfg, input_shape=None):
    """build_resnest_backbone (resnest.py:482-620) restricted to the frozen, forward-only module: refuses every option it does not implement."""
    r = cfg_get(cfg.MODEL, "RESNETS", None)
    if input_shape is not None and getattr(input_shape, "channels", 3) not in (None, 3):
        raise AfiError(f"resnest_backbone: 3 input channels only, got {input_shape.channels}")
    radix = cfg_get(r, "RADIX", 1)
    if radix != 2:
        raise AfiError(f"resnest_backbone: RESNETS.RADIX {radix} is not supported (2 only; radix 1 is the plain ResNet of resnet_guide)")
    if cfg_get(r, "NUM_GROUPS", 1) != 1:
        raise AfiError(f"resnest_backbone: RESNETS.NUM_GROUPS {cfg_get(r, 'NUM_GROUPS', 1)} is not supported (cardinality 1 only)")
    if cfg_get(r, "RES5_DILATION", 1) != 1:
        raise AfiError(f"resnest_backbone: RESNETS.RES5_DILATION {cfg_get(r, 'RES5_DILATION', 1)} is not supported (no dilation)")
    if any(cfg_get(r, "DEFORM_ON_PER_STAGE", [False] * 4)):
        raise AfiError("resnest_backbone: deformable convolutions (RESNETS.DEFORM_ON_PER_STAGE) are not supported")
    if cfg_get(r, "STRIDE_IN_1X1", True):
        raise AfiError("resnest_backbone: RESNETS.STRIDE_IN_1X1 True is not supported: with radix 2 the AVD pool already down-samples a "
                       "stride-2 block, so a strided conv1 would down-sample it twice and its residual add would not match the shortcut "
                       "(the published ResNeSt configs set STRIDE_IN_1X1: False)")
    return ResNeSt(depth=cfg_get(r, "DEPTH", 50), out_features=list(cfg_get(r, "OUT_FEATURES", ["res4"])), norm=cfg_get(r, "NORM", "FrozenBN"),
                   freeze_at=int(cfg_get(cfg_get(cfg.MODEL, "BACKBONE", None), "FREEZE_AT", 2)), width_per_group=cfg_get(r, "WIDTH_PER_GROUP", 64),
                   bottleneck_width=cfg_get(r, "BOTTLENECK_WIDTH", 64), res2_out_channels=cfg_get(r, "RES2_OUT_CHANNELS", 256))


def build_resnest_backbone(cfg, input_shape=None):
    """The frozen ResNeSt bottom-up alone, for ``registry.set_bottom_up_builder("resnest", build_resnest_backbone)`` (opt-in: use_as_bottom_up)."""
    return _resnest_from_cfg(cfg, input_shape)


def build_resnest_fpn_backbone(cfg, input_shape=None):
    """detectron2-ResNeSt's build_resnest_fpn_backbone (ResNeSt + FPN + LastLevelMaxPool) as the frozen guide of stages 1 and 2."""
    fpn = cfg_get(cfg.MODEL, "FPN", None)
    if cfg_get(fpn, "NORM", "") != "":
        raise AfiError(f"resnest_backbone: FPN.NORM {cfg_get(fpn, 'NORM', '')!r} is not supported (the guide's FPN has biased convs, no norm)")
    return FPN(_resnest_from_cfg(cfg, input_shape), list(cfg_get(fpn, "IN_FEATURES", ["res2", "res3", "res4", "res5"])),
               cfg_get(fpn, "OUT_CHANNELS", 256), cfg_get(fpn, "FUSE_TYPE", "sum"))


def use_as_bottom_up():
    """Opt in: the AFI backbones' "resnest" bottom-up lookup (registry.bottom_up_builder) returns this frozen, forward-only ResNeSt -- what
    build_resnest_{fpn,pafpn}_sr_backbone then build on.  Not the default: stage 3 trains its bottom-up, which this module cannot."""
    registry.set_bottom_up_builder("resnest", build_resnest_backbone)


REGISTERED = registry.register_local_backbone(build_resnest_fpn_backbone)    # (with detectron2 installed the name is detectron2-ResNeSt's)
