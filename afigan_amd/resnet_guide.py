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

FROZEN_BN_EPS = 1e-5
_BLOCKS = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3]}


class FrozenBatchNorm2d(nn.Module):
    """detectron2.layers.FrozenBatchNorm2d: y = (x - running_mean) / sqrt(running_var + eps) * weight + bias, all four buffers."""

    def __init__(self, num_features, eps=FROZEN_BN_EPS):
        super().__init__()
        self.num_features, self.eps = num_features, eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features) - eps)


class Conv2d(nn.Module):
    """detectron2.layers.Conv2d's parameter tree (weight, optional bias, optional norm child); frozen: requires_grad is off."""

    def __init__(self, cin, cout, k, stride=1, bias=False, norm=True):
        super().__init__()
        self.kernel_size, self.stride = k, stride
        w = torch.randn(cout, cin, k, k) * (2.0 / (cout * k * k)) ** 0.5          # c2_msra_fill's scale (fan_out); a checkpoint replaces it
        self.weight = nn.Parameter(w, requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False) if bias else None
        self.norm = FrozenBatchNorm2d(cout) if norm else None

    def fold(self, scale=1.0):
        """(weight, bias) with the norm folded in, computed in fp64 and rounded once; 3x3 weights in the kernels' [O][kh][kw][I] memory,
        1x1 weights as [Cout, Cin].  `scale` multiplies the bias (the FPN's "avg" fuse halves it)."""
        w = self.weight.detach().double()
        b = self.bias.detach().double() if self.bias is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
        n = self.norm
        if n is not None:
            s = n.weight.double() * torch.rsqrt(n.running_var.double() + n.eps)
            w = w * s.view(-1, 1, 1, 1)
            b = (b - n.running_mean.double()) * s + n.bias.double()
        w, b = w.float(), (b * scale).float().contiguous()
        if self.kernel_size == 1:
            return w.reshape(w.shape[0], w.shape[1]).contiguous(), b
        if self.kernel_size == 3:
            return w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), b
        return w.contiguous(), b


def _conv1x1(x, wb, stride=1, add=None, relu=False, alpha=1.0, add_scale=1.0):
    if stride != 1:
        x = x[:, :, ::stride, ::stride]                                 # (a view: the kernel walks the strides)
    if add is not None and add.shape[-2:] != x.shape[-2:]:
        raise AfiError(f"resnet_guide: addend {tuple(add.shape)} does not match the conv output {tuple(x.shape[-2:])}")
    return ops.conv1x1_fwd(x, wb[0], wb[1], add=add, add_scale=add_scale, alpha=alpha, act=2 if relu else 0)


def _conv3x3(x, wb, stride=1, relu=False):
    act = 2 if relu else 0
    if stride == 2:
        return ops.conv3x3s2_fwd(x, wb[0], wb[1], act=act)
    N, C, H, W = x.shape
    if C >= 128 and wb[0].shape[0] >= 128 and N * H * W >= 1024:      # the Winograd form (F(4x4) tiles on maps of >= 8192 pixels)
        return ops.conv3x3_wino_infer(x, wb[0], wb[1], act=act)
    return ops.conv3x3_fwd(x, wb[0], wb[1], lrelu=act)


class _Frozen(nn.Module):
    """Folded weights of the convs this module runs itself, rebuilt when a parameter / buffer of them changes (version, storage, device)."""

    def _own_convs(self):
        raise NotImplementedError

    def _prepare(self):
        convs = self._own_convs()
        ts = [t for m in convs for t in list(m.parameters()) + list(m.buffers())]
        key = tuple((t._version, t.data_ptr(), str(t.device)) for t in ts)
        if getattr(self, "_folded_key", None) != key:
            self._folded = {id(m): m.fold() for m in convs}
            self._folded_key = key
        return self._folded

    def _check_frozen(self, x):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise AfiError("the ResNet-FPN guide is forward-only (frozen): run it under torch.no_grad() with no parameter or input requiring grad")
        if not x.is_cuda:
            raise AfiError("the ResNet-FPN guide runs on the GPU only (got a CPU tensor); there is no CPU fallback")


class BasicStem(nn.Module):
    def __init__(self, in_channels=3, out_channels=64):
        super().__init__()
        self.conv1 = Conv2d(in_channels, out_channels, 7, stride=2)


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
        s = x if self.shortcut is None else _conv1x1(x, f[id(self.shortcut)], self.shortcut.stride)
        y = _conv1x1(x, f[id(self.conv1)], self.conv1.stride, relu=True)
        y = _conv3x3(y, f[id(self.conv2)], self.conv2.stride, relu=True)
        return _conv1x1(y, f[id(self.conv3)], add=s, relu=True)


class ResNet(_Frozen):
    """The bottom-up: ``forward(x [N,3,H,W]) -> {name: pixel-major features}`` for ``out_features`` (subset of stem, res2..res5)."""

    def __init__(self, depth=50, out_features=("res2", "res3", "res4", "res5"), stride_in_1x1=True, width_per_group=64,
                 res2_out_channels=256, stem_out_channels=64):
        super().__init__()
        if depth not in _BLOCKS:
            raise AfiError(f"resnet_guide: RESNETS.DEPTH {depth} is not supported (50 or 101)")
        if stem_out_channels != 64:
            raise AfiError(f"resnet_guide: RESNETS.STEM_OUT_CHANNELS {stem_out_channels} is not supported (the stem kernel makes 64)")
        names = ["stem", "res2", "res3", "res4", "res5"]
        bad = [f for f in out_features if f not in names]
        if bad or not out_features:
            raise AfiError(f"resnet_guide: unknown RESNETS.OUT_FEATURES {list(out_features)}")
        if (width_per_group % 4) or (res2_out_channels % 4):
            raise AfiError("resnet_guide: channel counts must be multiples of 4")
        self._out_features = list(out_features)
        self.stem = BasicStem(3, 64)
        self._out_feature_channels, self._out_feature_strides = {"stem": 64}, {"stem": 4}
        cin, cout, mid = 64, res2_out_channels, width_per_group
        self.stage_names = []
        for i, n in enumerate(_BLOCKS[depth][:max(names.index(f) for f in out_features)]):
            name, first = f"res{i + 2}", (1 if i == 0 else 2)
            blocks = [BottleneckBlock(cin if j == 0 else cout, cout, mid, first if j == 0 else 1, stride_in_1x1) for j in range(n)]
            self.add_module(name, nn.Sequential(*blocks))
            self.stage_names.append(name)
            self._out_feature_channels[name], self._out_feature_strides[name] = cout, 4 * 2 ** i
            cin, cout, mid = cout, 2 * cout, 2 * mid

    @property
    def size_divisibility(self):
        return 0

    def output_shape(self):
        return {n: ShapeSpec(channels=self._out_feature_channels[n], stride=self._out_feature_strides[n]) for n in self._out_features}

    def _own_convs(self):
        return [m for m in self.modules() if isinstance(m, Conv2d)]

    def forward(self, x):
        self._check_frozen(x)
        with torch.no_grad():
            f = self._prepare()
            out = {}
            y = ops.resnet_stem(x.float(), *f[id(self.stem.conv1)])
            if "stem" in self._out_features:
                out["stem"] = y
            for name in self.stage_names:
                for blk in getattr(self, name):
                    y = blk.run(y, f)
                if name in self._out_features:
                    out[name] = y
        return out


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

    def _prepare(self):
        f = super()._prepare()
        if self._fuse_type == "avg" and getattr(self, "_avg_key", None) != self._folded_key:
            for m in self.lateral_convs[1:]:                               # (lat + top-down) / 2 = 0.5 conv + 0.5 bias + 0.5 top-down
                f[("avg", id(m))] = m.fold(scale=0.5)
            self._avg_key = self._folded_key
        return f

    def forward(self, x):
        self._check_frozen(x)
        feats = self.bottom_up(x)
        with torch.no_grad():
            f = self._prepare()
            xs = [feats[k] for k in self.in_features[::-1]]
            prev = _conv1x1(xs[0], f[id(self.lateral_convs[0])])
            results = [_conv3x3(prev, f[id(self.output_convs[0])])]
            for feat, lat, out in zip(xs[1:], self.lateral_convs[1:], self.output_convs[1:]):
                td = ops.nearest(prev, up=2)
                if self._fuse_type == "avg":
                    prev = _conv1x1(feat, f[("avg", id(lat))], add=td, alpha=0.5, add_scale=0.5)
                else:
                    prev = _conv1x1(feat, f[id(lat)], add=td)
                results.insert(0, _conv3x3(prev, f[id(out)]))
            results.append(ops.nearest(results[-1], up=1, down=2))          # LastLevelMaxPool on the coarsest output
        return dict(zip(self._out_features, results))


def _get(node, key, default):
    return getattr(node, key, default) if node is not None else default


def _resnet_from_cfg(cfg, input_shape=None):
    """detectron2's build_resnet_backbone restricted to the frozen, forward-only guide: refuses every option it does not implement."""
    r = _get(cfg.MODEL, "RESNETS", None)
    if input_shape is not None and getattr(input_shape, "channels", 3) not in (None, 3):
        raise AfiError(f"resnet_guide: 3 input channels only, got {input_shape.channels}")
    norm = _get(r, "NORM", "FrozenBN")
    if norm != "FrozenBN":
        raise AfiError(f"resnet_guide: RESNETS.NORM {norm!r} is not supported (the frozen guide folds FrozenBN)")
    if _get(r, "NUM_GROUPS", 1) != 1:
        raise AfiError(f"resnet_guide: RESNETS.NUM_GROUPS {_get(r, 'NUM_GROUPS', 1)} is not supported (groups = 1 only)")
    if _get(r, "RES5_DILATION", 1) != 1:
        raise AfiError(f"resnet_guide: RESNETS.RES5_DILATION {_get(r, 'RES5_DILATION', 1)} is not supported (no dilation)")
    if any(_get(r, "DEFORM_ON_PER_STAGE", [False] * 4)):
        raise AfiError("resnet_guide: deformable convolutions (RESNETS.DEFORM_ON_PER_STAGE) are not supported")
    if _get(r, "RADIX", 1) != 1 or _get(r, "DEEP_STEM", False) or _get(r, "AVD", False) or _get(r, "AVG_DOWN", False):
        raise AfiError("resnet_guide: the ResNeSt options (RESNETS.RADIX / DEEP_STEM / AVD / AVG_DOWN) are not supported")
    return ResNet(depth=_get(r, "DEPTH", 50), out_features=list(_get(r, "OUT_FEATURES", ["res4"])),
                  stride_in_1x1=bool(_get(r, "STRIDE_IN_1X1", True)), width_per_group=_get(r, "WIDTH_PER_GROUP", 64),
                  res2_out_channels=_get(r, "RES2_OUT_CHANNELS", 256), stem_out_channels=_get(r, "STEM_OUT_CHANNELS", 64))


def build_resnet_backbone(cfg, input_shape=None):
    """The frozen ResNet bottom-up alone, for ``registry.set_bottom_up_builder("resnet", build_resnet_backbone)`` (opt-in: see use_as_bottom_up)."""
    return _resnet_from_cfg(cfg, input_shape)


def build_resnet_fpn_backbone(cfg, input_shape=None):
    """detectron2's build_resnet_fpn_backbone (ResNet + FPN + LastLevelMaxPool) as the frozen guide of stages 1 and 2."""
    fpn = _get(cfg.MODEL, "FPN", None)
    if _get(fpn, "NORM", "") != "":
        raise AfiError(f"resnet_guide: FPN.NORM {_get(fpn, 'NORM', '')!r} is not supported (the guide's FPN has biased convs, no norm)")
    return FPN(_resnet_from_cfg(cfg, input_shape), list(_get(fpn, "IN_FEATURES", ["res2", "res3", "res4", "res5"])),
               _get(fpn, "OUT_CHANNELS", 256), _get(fpn, "FUSE_TYPE", "sum"))


def use_as_bottom_up():
    """Opt in: the AFI backbones' "resnet" bottom-up lookup (registry.bottom_up_builder) returns this frozen, forward-only ResNet."""
    registry.set_bottom_up_builder("resnet", build_resnet_backbone)


def _register():
    """``build_resnet_fpn_backbone`` in the LOCAL registry only: with detectron2 installed the name is detectron2's."""
    if registry.USING_DETECTRON2_REGISTRY:
        return False
    if "build_resnet_fpn_backbone" not in registry.BACKBONE_REGISTRY:
        registry.BACKBONE_REGISTRY.register(build_resnet_fpn_backbone)
    return True


REGISTERED = _register()
