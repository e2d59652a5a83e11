"""The ResNeSt bottom-up of the reference's best models (detectron2-ResNeSt's ``build_resnest_backbone``: resnest.py, splat.py) on this
package's HIP kernels -- frozen and forward-only as the AFI backbone's bottom-up for inference (``use_as_bottom_up``, then
``build_resnest_{fpn,pafpn}_sr_backbone``) and, under resnet_guide's FPN, as a stage-1/2 guide (``build_resnest_fpn_backbone``); and, after
``ResNeSt.trainable_``, with the stages behind ``freeze_at`` under autograd for step 3.

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

Training (``ResNeSt.trainable_``): the stages behind ``freeze_at`` run as one autograd Function, ``_ResNeStTrainFn``, under the
folded FrozenBN as the ResNet's do -- the convs' backward on the ResNet's entry points (the grouped 3x3 as two per-group weight
and data gradients through channel views), split attention's on afi_resnest_splat_bwd_dots / _attn / _params / _combine, the avg_down
pool's on afi_resnest_pool_bwd; the AVD pool's transpose is gathered inside the split-attention passes.

Out of scope (AfiError at build time): radix != 2, NUM_GROUPS > 1, dilation, deformable convs, norms other than FrozenBN / BN / SyncBN,
STRIDE_IN_1X1 = True; at call time, a CPU tensor and a forward that autograd could differentiate through a frozen module; in training,
BN / SyncBN in a trainable stage (train-mode BatchNorm) and the stem's backward (``freeze_at=0``)."""
import torch
import torch.nn as nn

from . import _lib, frozen, ops, registry
from ._lib import AfiError
from .frozen import FrozenBatchNorm2d, adopt_prepared, cfg_get, conv1x1, conv3x3, fold_conv, prepared
from .resnet_guide import FPN, ResNetBase, dense_cotangent

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

    def fold_fc(self):
        """The folds of the two tiny biased convs alone: ((w1', b1'), (w2, b2)) -- the only ones whose fold depends on a trainable bias."""
        return frozen.fold_conv(self.fc1, self.bn1), frozen.fold_conv(self.fc2)

    def run(self, y, f, avd):
        (wc, bc), (w1, b1), (w2, b2) = f[id(self)]
        g = self.channels
        s0 = conv3x3(y[:, :g // 2], (wc[:g], bc[:g]), relu=True)
        s1 = conv3x3(y[:, g // 2:], (wc[g:], bc[g:]), relu=True)
        return ops.splat_attention(s0, s1, w1, b1, w2, b2, avd=avd)[0]

    def run_keep(self, y, f, avd):
        """`run`, also returning what the backward reads: the splits, the attention, the pooled mean g and fc1's post-ReLU output h."""
        (wc, bc), (w1, b1), (w2, b2) = f[id(self)]
        g = self.channels
        s0 = conv3x3(y[:, :g // 2], (wc[:g], bc[:g]), relu=True)
        s1 = conv3x3(y[:, g // 2:], (wc[g:], bc[g:]), relu=True)
        u, att, gm, h = ops.splat_attention(s0, s1, w1, b1, w2, b2, avd=avd, keep=True)
        return s0, s1, att, gm, h, u


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

    def convs(self):
        """The block's bias-free convs with their norms, in the order ``_ResNeStTrainFn`` takes their weights: conv1, the grouped 3x3 (its
        norm is bn0), conv3, then the shortcut if there is one."""
        out = [(self.conv1, self.conv1.norm), (self.conv2.conv, self.conv2.bn0), (self.conv3, self.conv3.norm)]
        return out + ([(self.shortcut, self.shortcut.norm)] if self.shortcut is not None else [])

    def fc_params(self):
        return [self.conv2.fc1.weight, self.conv2.fc1.bias, self.conv2.fc2.weight, self.conv2.fc2.bias]

    def run_keep(self, x, f):
        """`run`, also returning conv1's output, the splits, the attention's (att, g, h) and the combine's output u (conv3's input)."""
        if self.shortcut is None:
            s = x
        else:
            xs = ops.resnest_pool(x, "avg2s2_ceil") if self.stride == 2 else x
            s = conv1x1(xs, f[id(self.shortcut)])
        a1 = conv1x1(x, f[id(self.conv1)], relu=True)
        s0, s1, att, g, h, u = self.conv2.run_keep(a1, f, self.avd)
        return [a1, s0, s1, att, g, h, u, conv1x1(u, f[id(self.conv3)], add=s, relu=True)]


_KEPT = 8                                # tensors BottleneckBlock.run_keep returns


def conv2_wino(a1, group_width):
    """Whether the grouped 3x3 of a block with conv1 output `a1` runs in the Winograd form: frozen.conv3x3's rule on ONE radix group
    (group_width / 2 channels in, group_width out), which is how the forward launches it."""
    N, _, H, W = a1.shape
    return group_width // 2 >= 128 and group_width >= 128 and N * H * W >= 1024


class _ResNeStTrainFn(torch.autograd.Function):
    """The trainable stages of a ResNeSt bottom-up as one node, modelled on resnet_guide._ResNetTrainFn: ``(net, x, *weights, *fc) -> out_features
    of those stages``; x the first trainable stage's input (no gradient: the stages below are frozen), `weights` the bias-free conv weights of
    ``net._train_convs()``, `fc` the four fc1 / fc2 tensors of every block (``net._train_fc()``).

    Forward: every block on the frozen module's kernels over the prepared fold, keeping per block a1, s0, s1, att, g, h, u and y.  Backward,
    blocks in reverse; gz = the gradient at a block's pre-activation output:
      conv3    weight gradient, then du = W3'^T gz UNMASKED (u is the combine's output: no ReLU)             -- afi_conv1x1_dgrad
      splat    afi_resnest_splat_bwd_dots / _attn / _params / _combine: fc1 / fc2's gradients straight into the parameters' (bn1's scale
               applied there), ds0 / ds1 with the splits' ReLU masks; with AVD the pool's transpose is gathered inside the passes
      grouped  per radix group r, through channel views: weight gradient of (ds_r, a1 group r) into rows r of dw', data gradient into
               channels r of g1 with conv1's ReLU mask in the epilogue, in the regime the forward ran in
      conv1 and the shortcut as in _ResNetTrainFn; a stride-2 block's shortcut data gradient goes through afi_resnest_pool_bwd (the
               avg_down pool's transpose) into the input's gradient with beta = 1 and the input's ReLU mask.
    One afi_frozen_wgrad_unfold launch takes every dw' through its fold scale to the parameter's gradient."""

    @staticmethod
    @_lib.ctx_forward
    def forward(ctx, net, x, *params):
        f, scales = net._prepare(), net._fold_scales()
        blocks = net._train_blocks()
        saved, outs, y = [x], [], x
        ctx.out_block = {}
        for name in net._train_stages:
            for blk in getattr(net, name):
                kept = blk.run_keep(y, f)
                saved += kept
                y = kept[-1]
            if name in net._out_features:
                ctx.out_block[(len(saved) - 1) // _KEPT - 1] = len(outs)
                outs.append(y)
        convs = [c for blk in blocks for c, _ in blk.convs()]
        wf = [f[id(blk.conv2)][0][0] if c is blk.conv2.conv else f[id(c)][0] for blk in blocks for c, _ in blk.convs()]
        fcw = [t for blk in blocks for t in (f[id(blk.conv2)][1][0], f[id(blk.conv2)][2][0], scales[id(blk.conv2.fc1)])]
        ctx.save_for_backward(*saved, *wf, *[scales[id(c)] for c in convs], *fcw)
        ctx.blocks = blocks
        ctx.wshapes = [tuple(c.weight.shape) for c in convs]
        ctx.fcshapes = [tuple(t.shape) for blk in blocks for t in blk.fc_params()]
        return tuple(outs)

    @staticmethod
    @_lib.ctx_backward
    def backward(ctx, *douts):
        blocks, sv = ctx.blocks, ctx.saved_tensors
        B, nconv = len(blocks), len(ctx.wshapes)
        nact = 1 + _KEPT * B
        acts, wf, sc, fcw = sv[:nact], sv[nact:nact + nconv], sv[nact + nconv:nact + 2 * nconv], sv[nact + 2 * nconv:]
        dev = acts[0].device
        xin = lambda b: acts[_KEPT * b]                                      # block b's input: x, or block b - 1's y
        kept = lambda b: acts[_KEPT * b + 1:_KEPT * b + 1 + _KEPT]
        cot = {b: dense_cotangent(douts[k], kept(b)[-1]) for b, k in ctx.out_block.items()}
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
        fcsizes = [(int(torch.Size(s_).numel()) + 3) // 4 * 4 for s_ in ctx.fcshapes]          # every segment 16-byte aligned
        fcoffs = [0]
        for n in fcsizes:
            fcoffs.append(fcoffs[-1] + n)
        fcflat = torch.zeros(fcoffs[-1], device=dev, dtype=torch.float32)
        fcgrads = [fcflat[o:o + int(torch.Size(s_).numel())].view(s_) for s_, o in zip(ctx.fcshapes, fcoffs)]

        def wgrad1x1(dy, x, dw):
            N, Cout, H, W = dy.shape
            _lib.call("afi_conv1x1_wgrad", ops.view_of(dy), ops.view_of(x), N, H, W, Cout, x.shape[1], ops._p(dw), 1.0, ops.stream_ptr())

        ci, gz = nconv, None
        for b in reversed(range(B)):
            blk = blocks[b]
            n_own = len(blk.convs())
            ci -= n_own
            i1, i2, i3, isc = ci, ci + 1, ci + 2, (ci + 3 if n_own == 4 else None)
            x = xin(b)
            A1, S0, S1, att, gm, h, U, Y = kept(b)
            w1f, w2f, s1 = fcw[3 * b:3 * b + 3]
            dw1, db1, dw2, db2 = fcgrads[4 * b:4 * b + 4]
            if gz is None:                                                   # the last block: everything it gets is its output's cotangent
                c = cot.get(b)
                gz = ops.relu_bwd(c, Y) if c is not None else ops.new_pixel_major(*Y.shape, dev, zero=True)
            # conv3: its input u has no ReLU, so the data gradient is unmasked
            wgrad1x1(gz, U, dws[i3])
            du = ops.conv1x1_dgrad(gz, wf[i3])
            # split attention (with AVD: the pool's transpose gathered inside)
            ds0, ds1 = ops.splat_attention_bwd(du, S0, S1, att, gm, h, w1f, w2f, s1, blk.avd, dw1, db1, dw2, db2)
            # the grouped 3x3: one weight and one data gradient per radix group, through channel views
            gw = blk.conv2.channels
            wino = conv2_wino(A1, gw)
            g1 = ops.new_pixel_major(*A1.shape, dev)
            for r, ds in enumerate((ds0, ds1)):
                a1r, g1r = A1[:, r * gw // 2:(r + 1) * gw // 2], g1[:, r * gw // 2:(r + 1) * gw // 2]
                wr, dwr = wf[i2][r * gw:(r + 1) * gw], dws[i2][r * gw:(r + 1) * gw]
                if wino:
                    ops.conv3x3_wino_wgrad(ds, a1r, dw=dwr)
                    ops.conv3x3_wino_dgrad(ds, wr, z=a1r, z_act="relu", dx=g1r)
                else:
                    ops.conv3x3_wgrad(ds, a1r, dw=dwr)
                    ops.conv3x3_dgrad(ds, wr, dx=g1r, z=a1r, z_act="relu")
            # conv1 and the shortcut: weight gradients on what they read
            wgrad1x1(g1, x, dws[i1])
            if isc is not None:
                xs = ops.resnest_pool(x, "avg2s2_ceil") if blk.stride == 2 else x
                wgrad1x1(gz, xs, dws[isc])
            if b == 0:
                break                                                        # the stages below are frozen: no dx
            c = cot.get(b - 1)
            if isc is None:                                                  # identity block: join, cotangent and mask in conv1's epilogue, in place
                gz = ops.conv1x1_dgrad(g1, wf[i1], dx=gz, beta=1.0, z=x, z_act="relu", add=c)
            else:
                dx = ops.relu_bwd(c, x) if c is not None else ops.new_pixel_major(*x.shape, dev, zero=True)
                if blk.stride == 2:                                          # W_sc^T gz at the pooled size, then the avg_down pool's transpose
                    ops.resnest_pool_bwd(ops.conv1x1_dgrad(gz, wf[isc]), "avg2s2_ceil", dx=dx, beta=1.0, z=x)
                else:
                    ops.conv1x1_dgrad(gz, wf[isc], dx=dx, beta=1.0, z=x, z_act="relu")
                ops.conv1x1_dgrad(g1, wf[i1], dx=dx, beta=1.0, z=x, z_act="relu")
                gz = dx
        ops.frozen_wgrad_unfold(list(zip(dws, grads, sc)))
        need = ctx.needs_input_grad[2:]
        return (None, None, *[g if n else None for g, n in zip(grads + fcgrads, need)])


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

    # ---- the prepared fold, in two slots: "folded" holds every bias-free conv (a split-attention conv's entry is its grouped 3x3 with bn0),
    # "folded_fc" the tiny fc1 / fc2 of every block, whose fold depends on trainable biases.  An optimiser that writes the bias-free folds
    # itself (fold_slots / adopt_folded) leaves the second slot to refold here when fc1 / fc2 move.
    def _fold_own(self, convs):
        return {id(m): (frozen.fold_conv(m.conv, m.bn0) if isinstance(m, SplAtConv2d) else m.fold()) for m in convs}

    def _prepare_tensors(self, convs):
        ts = []
        for m in convs:
            ts += [m.conv.weight] + list(m.bn0.buffers()) if isinstance(m, SplAtConv2d) else list(m.parameters()) + list(m.buffers())
        return ts

    def _prepare(self):
        convs = self._own_convs()
        splats = [m for m in convs if isinstance(m, SplAtConv2d)]
        f = prepared(self, "folded", self._prepare_tensors(convs), lambda: self._fold_own(convs))
        fc_ts = [t for m in splats for t in list(m.fc1.parameters()) + list(m.bn1.buffers()) + list(m.fc2.parameters())]
        fc = prepared(self, "folded_fc", fc_ts, lambda: {id(m): m.fold_fc() for m in splats})
        joined = getattr(self, "_joined", None)
        if joined is None or joined[0] is not f or joined[1] is not fc:
            d = dict(f)
            for m in splats:
                d[id(m)] = (f[id(m)],) + tuple(fc[id(m)])
            joined = self._joined = (f, fc, d)
        return joined[2]

    # ---- training
    def trainable_(self, freeze_at=2):
        """``ResNet.trainable_`` for the ResNeSt: the stem and res2..res{freeze_at} stay frozen; the later stages' conv1 / grouped 3x3 / conv3 /
        shortcut weights and fc1 / fc2 weights and biases get ``requires_grad=True`` (every norm tensor stays a buffer: training runs under
        the folded FrozenBN) and ``forward`` runs those stages under autograd (``_ResNeStTrainFn``).  ``trainable_(False)`` restores the
        all-frozen, forward-only module.  Returns self."""
        if freeze_at is False:
            stages = []
        else:
            if isinstance(freeze_at, bool) or not isinstance(freeze_at, int) or not 0 <= freeze_at <= 5:
                raise AfiError(f"resnest_backbone: trainable_(freeze_at={freeze_at!r}): an integer 1..5 (BACKBONE.FREEZE_AT), or False to freeze everything")
            if freeze_at == 0:
                raise AfiError("resnest_backbone: BACKBONE.FREEZE_AT 0 trains the stem, which needs the backward of the deep stem's 3x3 convs and "
                               "of the max-pool; neither exists here (freeze_at >= 1 only)")
            stages = [n for n in self.stage_names if int(n[3:]) > freeze_at]
            for name in stages:
                for m in getattr(self, name).modules():
                    if isinstance(m, (nn.BatchNorm2d, nn.SyncBatchNorm)):
                        raise AfiError(f"resnest_backbone: {name} carries {type(m).__name__}: train-mode BatchNorm in the bottom-up is out of scope; "
                                       "build with RESNETS.NORM \"FrozenBN\" (training runs under the folded norm)")
        for name in self.stage_names:
            for blk in getattr(self, name):
                for t in [c.weight for c, _ in blk.convs()] + blk.fc_params():
                    t.requires_grad_(name in stages)
        self._train_stages = tuple(stages)
        return self

    def _train_blocks(self):
        return [blk for name in self._train_stages for blk in getattr(self, name)]

    def _train_convs(self):
        """[(conv, its norm)] of the trainable stages' bias-free convs, in ``_ResNeStTrainFn``'s order."""
        return [cn for blk in self._train_blocks() for cn in blk.convs()]

    def _train_fc(self):
        return [t for blk in self._train_blocks() for t in blk.fc_params()]

    def _scale_pairs(self):
        return self._train_convs() + [(blk.conv2.fc1, blk.conv2.bn1) for blk in self._train_blocks()]

    def _fold_scales(self):
        """s = gamma / sqrt(var + eps) per trainable conv (and per fc1, of bn1), fp64 rounded once: d w' / d w of the fold, per output channel."""
        pairs = self._scale_pairs()
        return prepared(self, "bn_scales", [t for _, n in pairs for t in n.buffers()], lambda: {
            id(c): (n.weight.double() * torch.rsqrt(n.running_var.double() + n.eps)).float().contiguous() for c, n in pairs})

    def _fold_scales64(self):
        pairs = self._train_convs()
        return prepared(self, "bn_scales64", [t for _, n in pairs for t in n.buffers()], lambda: {
            id(c): (n.weight.double() * torch.rsqrt(n.running_var.double() + n.eps)).contiguous() for c, n in pairs})

    def fold_slots(self):
        """[(weight parameter, fp64 fold scale [O], folded weight)] per trainable bias-free conv (``ResNet.fold_slots``): the folded weight is
        the tensor in the "folded" slot of ``_prepare()`` -- for the grouped 3x3 the [2C, C/2, 3, 3] weight with bn0, an ordinary k = 3 entry.
        fc1 / fc2 are not here: their slot refolds itself."""
        self._prepare()
        f, s = self._folded, self._fold_scales64()
        splat_of = {id(blk.conv2.conv): blk.conv2 for blk in self._train_blocks()}
        return [(c.weight, s[id(c)], f[id(splat_of.get(id(c), c))][0]) for c, _ in self._train_convs()]

    def adopt_folded(self):
        """The "folded" slot is current for the parameters as they are now (frozen.adopt_prepared): only for the writer `fold_slots` names."""
        adopt_prepared(self, "folded", self._prepare_tensors(self._own_convs()))

    def _forward_train(self, x):
        if not x.is_cuda:
            raise AfiError(f"{self.what} runs on the GPU only (got a CPU tensor); there is no CPU fallback")
        if x.requires_grad:
            raise AfiError(f"{self.what}: the input requires grad, but the stem is frozen (its backward does not exist here)")
        params = [c.weight for c, _ in self._train_convs()] + self._train_fc()
        own = {id(p) for p in params}
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
        outs = _ResNeStTrainFn.apply(self, y, *params)
        out.update(zip([n for n in self._train_stages if n in self._out_features], outs))
        return out


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


def build_trainable_resnest_backbone(cfg, input_shape=None):
    """The ResNeSt bottom-up with the stages behind ``cfg.MODEL.BACKBONE.FREEZE_AT`` trainable (step 3: FREEZE_AT 2); RESNETS.NORM must be
    "FrozenBN" (``ResNeSt.trainable_`` refuses BN / SyncBN stages)."""
    return _resnest_from_cfg(cfg, input_shape).trainable_(int(cfg_get(cfg_get(cfg.MODEL, "BACKBONE", None), "FREEZE_AT", 2)))


def use_as_bottom_up(trainable=False):
    """Opt in: the AFI backbones' "resnest" bottom-up lookup (registry.bottom_up_builder) returns this ResNeSt -- what
    build_resnest_{fpn,pafpn}_sr_backbone then build on: frozen and forward-only, or with ``trainable=True`` the one
    ``build_trainable_resnest_backbone`` makes (same state-dict keys), which stage 3 trains."""
    registry.set_bottom_up_builder("resnest", build_trainable_resnest_backbone if trainable else build_resnest_backbone)


REGISTERED = registry.register_local_backbone(build_resnest_fpn_backbone)    # (with detectron2 installed the name is detectron2-ResNeSt's)
