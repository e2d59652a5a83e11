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

Training (``ResNet.trainable_``): the stages behind ``freeze_at`` run as one autograd Function, ``_ResNetTrainFn`` -- forward on the
kernels above, backward on afi_conv1x1_wgrad / afi_conv3x3_wgrad / afi_conv3x3_wino_wgrad / afi_conv3x3s2_wgrad and the data gradients with
the ReLU mask, the residual join and the pyramid's cotangent in their epilogue (afi_conv1x1_dgrad_act, afi_conv3x3_dgrad_act,
afi_conv3x3_wino_dgrad_act), then one afi_frozen_wgrad_unfold launch from the folded weights' gradients to the parameters'.

Out of scope (AfiError at build time): dilation, groups > 1, deformable convs, norms other than FrozenBN, a normalised FPN, the ResNeSt
options; at call time, a forward that autograd could differentiate through a frozen module, the stem's backward (``freeze_at=0``)."""
import torch
import torch.nn as nn

from . import _lib, ops, registry
from ._lib import AfiError
from .fpn_sr import ShapeSpec
from .frozen import FROZEN_BN_EPS, Conv2d, FrozenBatchNorm2d, adopt_prepared, cfg_get, check_forward_only, conv1x1, conv3x3, prepared  # noqa: F401
from .rpn import _wino

_BLOCKS = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3]}


class _Frozen(nn.Module):
    """Folded weights of the convs this module runs itself, rebuilt when a parameter / buffer of them changes (frozen.prepared)."""
    what = "the ResNet-FPN guide"

    def _own_convs(self):
        raise NotImplementedError

    def _fold_own(self, convs):
        return {id(m): m.fold() for m in convs}

    def _prepare_tensors(self, convs):
        return [t for m in convs for t in list(m.parameters()) + list(m.buffers())]

    def _prepare(self):
        convs = self._own_convs()
        return prepared(self, "folded", self._prepare_tensors(convs), lambda: self._fold_own(convs))


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

    def run(self, x, f, route=False):
        """`route`: the forward-only inference path -- large maps take frozen.conv1x1's bf16x6 kernel over each conv's prepared image."""
        own = (lambda m: m) if route else (lambda m: None)
        s = x if self.shortcut is None else conv1x1(x, f[id(self.shortcut)], self.shortcut.stride, owner=own(self.shortcut))
        y = conv1x1(x, f[id(self.conv1)], self.conv1.stride, relu=True, owner=own(self.conv1))
        y = conv3x3(y, f[id(self.conv2)], self.conv2.stride, relu=True)
        return conv1x1(y, f[id(self.conv3)], add=s, relu=True, owner=own(self.conv3))

    def convs(self):
        """The block's convs in the order ``_ResNetTrainFn`` takes their weights: conv1, conv2, conv3, then the shortcut if there is one."""
        return [self.conv1, self.conv2, self.conv3] + ([self.shortcut] if self.shortcut is not None else [])

    def run_keep(self, x, f):
        """`run`, also returning conv1's and conv2's (post-ReLU) outputs: what the backward reads its masks and weight gradients from."""
        s = x if self.shortcut is None else conv1x1(x, f[id(self.shortcut)], self.shortcut.stride)
        a1 = conv1x1(x, f[id(self.conv1)], self.conv1.stride, relu=True)
        a2 = conv3x3(a1, f[id(self.conv2)], self.conv2.stride, relu=True)
        return a1, a2, conv1x1(a2, f[id(self.conv3)], add=s, relu=True)


def _strided(t, stride):
    return t if stride == 1 else t[:, :, ::stride, ::stride]


def _dense_pm(t, like):
    """A cotangent as a dense pixel-major fp32 tensor (None: none arrived for this output)."""
    if t is None:
        return None
    t = ops.pixel_major(t.float())
    if not ops.is_dense_pm(t):
        d = ops.new_pixel_major(*like.shape, like.device)
        d.copy_(t)
        t = d
    return t


dense_cotangent = _dense_pm              # (the name resnest_backbone's _ResNeStTrainFn imports)


class _ResNetTrainFn(torch.autograd.Function):
    """The trainable stages of a ResNet bottom-up as one node: ``(net, fuse_masks, x, *weights) -> out_features of those stages``, x the first
    trainable stage's input (no gradient: the stages below are frozen), weights the conv weights of ``net._train_convs()`` in that order.

    Forward: every block on frozen.conv1x1 / frozen.conv3x3 over the prepared fold (the frozen module's kernels), keeping a1, a2 and y, all
    post-ReLU.  Backward, blocks in reverse; gz = the gradient at a block's pre-activation output, afi_relu_bwd(d_out, y) for the last block:
      conv3  weight gradient, then g2 = (W3'^T gz) * [a2 > 0]                      -- afi_conv1x1_dgrad_act
      conv2  weight gradient and g1 = (W2'^T g2) * [a1 > 0] in the forward's regime  -- afi_conv3x3_dgrad_act / afi_conv3x3_wino_dgrad_act
             (the stride-2 3x3 of STRIDE_IN_1X1 = False: afi_conv3x3s2_dgrad + one afi_relu_bwd)
      conv1  weight gradient, then the data gradient LAST: an identity block writes (W1'^T g1 + gz + cotangent of x) * [x > 0] into the gz
             buffer itself (beta = 1, in place) -- the previous block's gz; a down-sampling block starts a fresh buffer from the cotangent of x
             (afi_relu_bwd) or zeros, and its shortcut's and conv1's data gradients add into the view of the pixels they read (beta = 1, the
             mask again: a 0/1 mask applied twice is the same mask).  The first trainable block computes no dx.
    ``fuse_masks=False``: the same GEMMs through the entry points without the mask, afi_relu_bwd and the adds as passes of their own.
    All dw' (gradients of the FOLDED weights) live in one zero-filled buffer the weight-gradient kernels add into; one afi_frozen_wgrad_unfold
    launch takes them through the fold's scale to the parameters' [O][I][kh][kw] gradients."""

    @staticmethod
    @_lib.ctx_forward
    def forward(ctx, net, fuse, x, *weights):
        f, scales = net._prepare(), net._fold_scales()
        blocks = net._train_blocks()
        saved, outs, y = [x], [], x
        ctx.out_block = {}                                                   # index of the block whose y is output k
        for name in net._train_stages:
            for blk in getattr(net, name):
                a1, a2, y = blk.run_keep(y, f)
                saved += [a1, a2, y]
            if name in net._out_features:
                ctx.out_block[len(saved) // 3 - 1] = len(outs)
                outs.append(y)
        convs = [c for blk in blocks for c in blk.convs()]
        ctx.save_for_backward(*saved, *[f[id(c)][0] for c in convs], *[scales[id(c)] for c in convs])
        ctx.blocks, ctx.fuse = blocks, bool(fuse)
        ctx.wshapes = [tuple(w.shape) for w in weights]
        return tuple(outs)

    @staticmethod
    @_lib.ctx_backward
    def backward(ctx, *douts):
        blocks, fuse, sv = ctx.blocks, ctx.fuse, ctx.saved_tensors
        B = len(blocks)
        nconv = len(ctx.wshapes)
        acts, wf, sc = sv[:1 + 3 * B], sv[1 + 3 * B:1 + 3 * B + nconv], sv[1 + 3 * B + nconv:]
        dev = acts[0].device
        xin = lambda b: acts[3 * b]                                          # block b's input: x, or block b - 1's y
        a1, a2, yb = (lambda b: acts[3 * b + 1]), (lambda b: acts[3 * b + 2]), (lambda b: acts[3 * b + 3])
        cot = {b: _dense_pm(douts[k], yb(b)) for b, k in ctx.out_block.items()}
        # one zero-filled home for every dw' (OHWI / [O][I] memory, each slice a multiple of 16 bytes) and one for the parameters' gradients
        sizes = [int(torch.Size(s_).numel()) for s_ in ctx.wshapes]
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + n)
        dwflat = torch.zeros(offs[-1], device=dev, dtype=torch.float32)
        gflat = torch.zeros(offs[-1], device=dev, dtype=torch.float32)
        dws, grads = [], []
        for (O, I, k, _), o, n in zip(ctx.wshapes, offs, sizes):
            seg = dwflat[o:o + n]
            dws.append(seg.view(O, 3, 3, I).permute(0, 3, 1, 2) if k == 3 else seg.view(O, I))
            grads.append(gflat[o:o + n].view(O, I, k, k))

        def wgrad1x1(dy, x, dw):
            N, Cout, H, W = dy.shape
            _lib.call("afi_conv1x1_wgrad", ops.view_of(dy), ops.view_of(x), N, H, W, Cout, x.shape[1], ops._p(dw), 1.0, ops.stream_ptr())

        ci = nconv
        gz = None
        for b in reversed(range(B)):
            blk = blocks[b]
            n_own = len(blk.convs())
            ci -= n_own
            i1, i2, i3, isc = ci, ci + 1, ci + 2, (ci + 3 if n_own == 4 else None)
            x, A1, A2 = xin(b), a1(b), a2(b)
            if gz is None:                                                   # the last block: everything it gets is its output's cotangent
                c = cot.get(b)
                gz = ops.relu_bwd(c, yb(b)) if c is not None else ops.new_pixel_major(*yb(b).shape, dev, zero=True)
            # conv3
            wgrad1x1(gz, A2, dws[i3])
            g2 = ops.conv1x1_dgrad(gz, wf[i3], z=A2, z_act="relu") if fuse else ops.relu_bwd(ops.conv1x1_dgrad(gz, wf[i3]), A2)
            # conv2, in the regime its forward ran in
            if blk.conv2.stride == 2:
                ops.conv3x3s2_wgrad(g2, A1, dw=dws[i2])
                g1 = ops.relu_bwd(ops.conv3x3s2_dgrad(g2, wf[i2], tuple(A1.shape[2:])), A1)
            else:
                wino = _wino(A1, g2.shape[1])
                (ops.conv3x3_wino_wgrad if wino else ops.conv3x3_wgrad)(g2, A1, dw=dws[i2])
                dgrad = ops.conv3x3_wino_dgrad if wino else ops.conv3x3_dgrad
                g1 = dgrad(g2, wf[i2], z=A1, z_act="relu") if fuse else ops.relu_bwd(dgrad(g2, wf[i2]), A1)
            # conv1 and the shortcut: weight gradients on the pixels they read
            s1 = blk.conv1.stride
            wgrad1x1(g1, _strided(x, s1), dws[i1])
            if isc is not None:
                ss = blk.shortcut.stride
                wgrad1x1(gz, _strided(x, ss), dws[isc])
            if b == 0:
                break                                                        # the stages below are frozen: no dx
            c = cot.get(b - 1)
            if fuse:
                if isc is None:                                              # identity block: join, cotangent and mask in conv1's epilogue, in place
                    gz = ops.conv1x1_dgrad(g1, wf[i1], dx=gz, beta=1.0, z=x, z_act="relu", add=c)
                else:
                    dx = ops.relu_bwd(c, x) if c is not None else ops.new_pixel_major(*x.shape, dev, zero=True)
                    ops.conv1x1_dgrad(gz, wf[isc], dx=_strided(dx, ss), beta=1.0, z=_strided(x, ss), z_act="relu")
                    ops.conv1x1_dgrad(g1, wf[i1], dx=_strided(dx, s1), beta=1.0, z=_strided(x, s1), z_act="relu")
                    gz = dx
            else:                                                            # the unfused baseline: every add and mask a pass of its own
                if s1 == 1:
                    dx = ops.conv1x1_dgrad(g1, wf[i1])
                else:
                    dx = ops.new_pixel_major(*x.shape, dev, zero=True)
                    ops.conv1x1_dgrad(g1, wf[i1], dx=_strided(dx, s1))
                if isc is None:
                    dx = dx + gz
                elif ss == 1:
                    dx = dx + ops.conv1x1_dgrad(gz, wf[isc])
                else:
                    t = ops.new_pixel_major(*x.shape, dev, zero=True)
                    ops.conv1x1_dgrad(gz, wf[isc], dx=_strided(t, ss))
                    dx = dx + t
                if c is not None:
                    dx = dx + c
                gz = ops.relu_bwd(dx, x)
        ops.frozen_wgrad_unfold(list(zip(dws, grads, sc)))
        need = ctx.needs_input_grad[3:]
        return (None, None, None, *[g if n else None for g, n in zip(grads, need)])


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

    _train_stages = ()                   # ResNet.trainable_: the stages that run under autograd
    _fuse_masks = True
    _route_frozen1x1 = False             # the forward-only path hands its blocks `route=True` (ResNet; the ResNeSt blocks are not routed)

    def _wants_graph(self):
        """The differentiable path: grad mode on, ``trainable_`` has named stages and a parameter requires grad (BiFPN_AFIGAN._wants_graph's
        rule).  Everything else is the frozen forward, with its refusals."""
        return bool(self._train_stages) and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def forward(self, x):
        if self._wants_graph():
            return self._forward_train(x)
        check_forward_only(self, x, self.what)
        with torch.no_grad():
            f = self._prepare()
            out = {}
            y = self.stem.run(x.float(), f)
            if "stem" in self._out_features:
                out["stem"] = y
            for name in self.stage_names:
                for blk in getattr(self, name):
                    y = blk.run(y, f, route=True) if self._route_frozen1x1 else blk.run(y, f)
                if name in self._out_features:
                    out[name] = y
        return out


class ResNet(ResNetBase):
    """The bottom-up of detectron2's ResNet-50 / -101 (see ResNetBase for the forward)."""
    _route_frozen1x1 = True

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

    # ---- training
    def trainable_(self, freeze_at=2, fuse_masks=True):
        """detectron2's ``ResNet.freeze(freeze_at)`` read the other way round: the stem and res2..res{freeze_at} stay frozen, the conv weights
        of the later stages get ``requires_grad=True`` (the FrozenBN tensors stay buffers) and ``forward`` runs those stages under autograd
        (``_ResNetTrainFn``).  ``trainable_(False)`` restores the all-frozen, forward-only module.  ``fuse_masks=False``: the unfused backward
        (every ReLU mask and residual add a pass of its own), the baseline the fused one is measured against.  Returns self."""
        if freeze_at is False:
            stages = []
        else:
            if isinstance(freeze_at, bool) or not isinstance(freeze_at, int) or not 0 <= freeze_at <= 5:
                raise AfiError(f"resnet_guide: trainable_(freeze_at={freeze_at!r}): an integer 1..5 (BACKBONE.FREEZE_AT), or False to freeze everything")
            if freeze_at == 0:
                raise AfiError("resnet_guide: BACKBONE.FREEZE_AT 0 trains the stem, which needs the backward of the 7x7 stride-2 conv and of the "
                               "max-pool; neither exists here (freeze_at >= 1 only)")
            stages = [n for n in self.stage_names if int(n[3:]) > freeze_at]
        for name in self.stage_names:
            for blk in getattr(self, name):
                for c in blk.convs():
                    c.weight.requires_grad_(name in stages)
        self._train_stages, self._fuse_masks = tuple(stages), bool(fuse_masks)
        return self

    def _train_blocks(self):
        return [blk for name in self._train_stages for blk in getattr(self, name)]

    def _train_convs(self):
        return [c for blk in self._train_blocks() for c in blk.convs()]

    def _fold_scales(self):
        """s = gamma / sqrt(var + eps) of every trainable conv's FrozenBN, fp64 rounded once: d w / d w' of the fold, per output channel."""
        convs = self._train_convs()
        ts = [t for c in convs for t in c.norm.buffers()]
        return prepared(self, "bn_scales", ts, lambda: {
            id(c): (c.norm.weight.double() * torch.rsqrt(c.norm.running_var.double() + c.norm.eps)).float().contiguous() for c in convs})

    def _fold_scales64(self):
        """`_fold_scales` before its rounding: frozen.fold_conv's own fp64 expression, what the fold multiplies the weight by."""
        convs = self._train_convs()
        ts = [t for c in convs for t in c.norm.buffers()]
        return prepared(self, "bn_scales64", ts, lambda: {
            id(c): (c.norm.weight.double() * torch.rsqrt(c.norm.running_var.double() + c.norm.eps)).contiguous() for c in convs})

    def fold_slots(self):
        """[(weight parameter, fp64 fold scale [O], folded weight)] per trainable conv: the folded weight is the tensor that lives in the
        ``_prepare()`` dict ([O, I] for a 1x1, [O, I, 3, 3] in [O][kh][kw][I] memory for a 3x3), so a writer that keeps it equal to
        ``fold_conv`` of the parameter (afi_detector_sgd_step) and then calls ``adopt_folded`` spares the next forward the refold."""
        f, s = self._prepare(), self._fold_scales64()
        return [(c.weight, s[id(c)], f[id(c)][0]) for c in self._train_convs()]

    def adopt_folded(self):
        """The ``_prepare()`` dict is current for the parameters as they are now (frozen.adopt_prepared): only for the writer `fold_slots` names."""
        adopt_prepared(self, "folded", self._prepare_tensors(self._own_convs()))

    def _forward_train(self, x):
        if not x.is_cuda:
            raise AfiError(f"{self.what} runs on the GPU only (got a CPU tensor); there is no CPU fallback")
        if x.requires_grad:
            raise AfiError(f"{self.what}: the input requires grad, but the stem is frozen (its backward does not exist here)")
        convs = self._train_convs()
        own = {id(c.weight) for c in convs}
        stray = [n for n, p in self.named_parameters() if p.requires_grad and id(p) not in own]
        if stray:
            raise AfiError(f"{self.what}: {stray[:3]} require grad but belong to a frozen stage (trainable_(freeze_at) names the trainable ones)")
        with torch.no_grad():
            f = self._prepare()
            out = {}
            y = self.stem.run(x.float(), f)
            if "stem" in self._out_features:
                out["stem"] = y
            for name in self.stage_names:
                if name in self._train_stages:
                    break
                for blk in getattr(self, name):
                    y = blk.run(y, f)
                if name in self._out_features:
                    out[name] = y
        outs = _ResNetTrainFn.apply(self, self._fuse_masks, y, *[c.weight for c in convs])
        out.update(zip([n for n in self._train_stages if n in self._out_features], outs))
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
            own = (lambda m: m) if getattr(self.bottom_up, "_route_frozen1x1", False) else (lambda m: None)   # (over a ResNeSt: not routed)
            prev = conv1x1(xs[0], f[id(self.lateral_convs[0])], owner=own(self.lateral_convs[0]))
            results = [conv3x3(prev, f[id(self.output_convs[0])])]
            for feat, lat, out in zip(xs[1:], self.lateral_convs[1:], self.output_convs[1:]):
                td = ops.nearest(prev, up=2)
                if self._fuse_type == "avg":
                    prev = conv1x1(feat, f[("avg", id(lat))], add=td, alpha=0.5, add_scale=0.5, owner=own(lat))
                else:
                    prev = conv1x1(feat, f[id(lat)], add=td, owner=own(lat))
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


def build_trainable_resnet_backbone(cfg, input_shape=None):
    """The ResNet bottom-up with the stages behind ``cfg.MODEL.BACKBONE.FREEZE_AT`` trainable (steps 2 and 3: FREEZE_AT 2)."""
    return _resnet_from_cfg(cfg, input_shape).trainable_(int(cfg_get(cfg_get(cfg.MODEL, "BACKBONE", None), "FREEZE_AT", 2)))


def use_as_bottom_up(trainable=False):
    """Opt in: the AFI backbones' "resnet" bottom-up lookup (registry.bottom_up_builder) returns this ResNet -- frozen and forward-only, or
    with ``trainable=True`` the one ``build_trainable_resnet_backbone`` makes (same state-dict keys: a model-zoo file loads as before)."""
    registry.set_bottom_up_builder("resnet", build_trainable_resnet_backbone if trainable else build_resnet_backbone)


REGISTERED = registry.register_local_backbone(build_resnet_fpn_backbone)        # (with detectron2 installed the name is detectron2's)
