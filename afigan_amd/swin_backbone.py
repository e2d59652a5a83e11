"""The frozen Swin Transformer bottom-up of the reference's BiFPN inference config (swin_transformer.py's ``build_swint_backbone``), forward
only, on this package's HIP kernels -- as the AFI backbone's bottom-up for inference (``use_as_bottom_up``, then
``build_swint_bifpn_sr_backbone``).

The network (patch size 4, head dim 32, no absolute position embedding):
  - PatchEmbed: the image zero-padded on the right / bottom to multiples of 4, Conv2d(3, C, 4, stride 4) + bias, LayerNorm;
  - per stage i (C_i = EMBED_DIM 2^i), DEPTHS[i] blocks  x = x + proj(attn(pad(norm1(x)))),  x = x + fc2(GELU(fc1(norm2(x)))), every odd
    block shifted by WINDOW_SIZE // 2 (also on a map smaller than the window: the reference does not clamp);
  - stage i's output, stage{i+2}, is norm{i}(x) before its PatchMerging: the 2x2 gather (odd sizes zero-padded), LayerNorm over the 4C
    channels, Linear(4C, 2C, bias=False).
Window attention: the map is zero-padded to multiples of the window AFTER norm1 (a padded token's q / k / v are the qkv bias), rolled by
-shift, partitioned; softmax(q k^T / sqrt(32) + table[relative_position_index] + mask) v, the mask -100 between tokens of different shift
regions (3 x 3 region ids over the padded map) in shifted blocks only; reversed, rolled back and cropped.

The parameter tree, key names and buffers are the reference SwinTransformer's (``patch_embed.proj`` / ``.norm``,
``layers.{i}.blocks.{j}.{norm1, attn.relative_position_bias_table, attn.relative_position_index, attn.qkv, attn.proj, norm2, mlp.fc1,
mlp.fc2}``, ``layers.{i}.downsample.{norm, reduction}``, ``norm{i}`` for the stages in OUT_FEATURES), so a trained checkpoint's
``backbone.bottom_up.*`` loads with strict=True.  Every parameter is created with requires_grad False.

Kernels: the patch embed afi_swin_patch_embed; norm1, norm2 and the output norms afi_swin_layernorm (affine applied, not folded: the
attention kernel synthesises padded tokens from the qkv bias itself); the merge gather + its LayerNorm afi_swin_layernorm (merge); window
attention afi_swin_window_attn (fp32 MFMA); GELU afi_swin_gelu; qkv, proj (+ residual), fc1, fc2 (+ residual) and the reduction
afi_conv1x1_fwd over pixel-major tokens.  No torch matmul / softmax / layer_norm, MIOpen or hipBLASLt kernel runs in the forward, and no
atomics: it is bit-identical from run to run and under hipGraph replay.  The dense relative-position bias images are rebuilt from the table
and the index buffer whenever a parameter or buffer changes (frozen.prepared: version, storage, device).

Out of scope (AfiError at build time): APE, head dims other than 32, windows other than 7 and 12, EMBED_DIM above 192 (the kernels' widths),
input channels other than 3; at call time, a CPU tensor and a forward that autograd could differentiate.  DROP_PATH_RATE and
BACKBONE.FREEZE_AT change neither the key set nor an eval forward: the frozen builder accepts and ignores them.

Training is an opt-in: ``trainable_(freeze_at, drop_path_rate)`` / ``build_trainable_swint_backbone`` /
``use_as_bottom_up(trainable=True)``.  A module on which ``trainable_`` was never called is the frozen one above, kernel for kernel.  The
trainable one runs the same forward kernels inside one autograd Function (``_SwinTrainFn``; bit-identical outputs without DropPath) and its
backward on afi_conv1x1_dgrad / _wgrad / afi_colsum_accum and swin_train.hip's kernels (LayerNorm, GELU, window attention, bias table,
patch gather, DropPath's scale-add): fp32, no atomics, bit-identical from run to run.  Refused: an input that requires grad, a 2-byte
input, a parameter of a frozen part that requires grad.  Out of scope: AdamW, activation checkpointing, APE, AMP."""
import torch
import torch.nn as nn

from . import _lib, ops, registry
from ._lib import AfiError
from .fpn_sr import ShapeSpec
from .frozen import cfg_get, check_forward_only, prepared
from .resnet_guide import dense_cotangent

HEAD_DIM = 32
MAX_EMBED_DIM = 192         # patch embed <= 256 channels; the last merge's LayerNorm 16 EMBED_DIM <= 3072 channels


def _frozen(m):
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def relative_position_index(window):
    """WindowAttention's relative_position_index: [window^2, window^2] int64, (dy + ws - 1) (2 ws - 1) + (dx + ws - 1)."""
    coords = torch.stack(torch.meshgrid(torch.arange(window), torch.arange(window), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += window - 1
    rel[:, :, 1] += window - 1
    rel[:, :, 0] *= 2 * window - 1
    return rel.sum(-1)


class WindowAttention(nn.Module):
    def __init__(self, dim, window, heads):
        super().__init__()
        self.window, self.heads = window, heads
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window - 1) ** 2, heads), requires_grad=False)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        self.register_buffer("relative_position_index", relative_position_index(window))
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def bias_image(self):
        idx, table = self.relative_position_index, self.relative_position_bias_table
        n = self.window * self.window
        if tuple(idx.shape) != (n, n) or int(idx.min()) < 0 or int(idx.max()) >= table.shape[0]:
            raise AfiError(f"swin_backbone: relative_position_index of shape {tuple(idx.shape)} does not index the {table.shape[0]}-row bias table")
        return ops.swin_bias_image(table, idx, self.window)


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, heads, window, shift, mlp_ratio):
        super().__init__()
        self.window, self.shift = window, shift
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, window, heads)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    def run(self, x, bias_img):
        a, m = self.attn, self.mlp
        y = ops.swin_layernorm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        qkv = ops.conv1x1_fwd(y, a.qkv.weight, a.qkv.bias)
        y = ops.swin_window_attn(qkv, a.qkv.bias, bias_img, self.window, self.shift)
        x = ops.conv1x1_fwd(y, a.proj.weight, a.proj.bias, add=x)
        y = ops.swin_layernorm(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        y = ops.swin_gelu_(ops.conv1x1_fwd(y, m.fc1.weight, m.fc1.bias))
        return ops.conv1x1_fwd(y, m.fc2.weight, m.fc2.bias, add=x)

    def run_keep(self, x, bias_img, s_attn=None, s_mlp=None):
        """``run`` keeping what the backward reads: (out, (x, qkv, attention output, x after the attention branch, fc1's pre-activation)).
        The same launches as ``run`` (GELU on a copy of the pre-activation); with the DropPath scales s_attn / s_mlp ([N], 0 or 1 / keep) the
        branch outputs are joined by afi_swin_scale_add instead of the proj / fc2 epilogue."""
        a, m = self.attn, self.mlp
        y = ops.swin_layernorm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        qkv = ops.conv1x1_fwd(y, a.qkv.weight, a.qkv.bias)
        att = ops.swin_window_attn(qkv, a.qkv.bias, bias_img, self.window, self.shift)
        if s_attn is None:
            x1 = ops.conv1x1_fwd(att, a.proj.weight, a.proj.bias, add=x)
        else:
            x1 = ops.swin_scale_add(x, s_attn, ops.conv1x1_fwd(att, a.proj.weight, a.proj.bias))
        y = ops.swin_layernorm(x1, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        h = ops.conv1x1_fwd(y, m.fc1.weight, m.fc1.bias)
        act = ops.swin_gelu_(h.clone())
        if s_mlp is None:
            out = ops.conv1x1_fwd(act, m.fc2.weight, m.fc2.bias, add=x1)
        else:
            out = ops.swin_scale_add(x1, s_mlp, ops.conv1x1_fwd(act, m.fc2.weight, m.fc2.bias))
        return out, (x, qkv, att, x1, h)

    def backward(self, kept, bias_img, csr, g, acc, s_attn=None, s_mlp=None, need_dx=True):
        """The block's backward: g, the gradient at its output (dense, owned by the caller: updated in place), becomes the gradient at its
        input (None without need_dx); acc(parameter, gradient) receives every parameter gradient.  y1, y2 and the GELU output are
        recomputed from what ``run_keep`` kept."""
        x, qkv, att, x1, h = kept
        a, m = self.attn, self.mlp
        H, W = x.shape[2:]
        zeros = lambda p: torch.zeros_like(p, memory_format=torch.contiguous_format)       # noqa: E731
        # MLP: fc2, GELU, fc1, norm2; the stream's gradient meets norm2's input gradient in the LayerNorm backward (beta = 1)
        gs = g if s_mlp is None else ops.swin_scale_add(None, s_mlp, g)
        act = ops.swin_gelu_(h.clone())
        acc(m.fc2.weight, ops.conv1x1_wgrad(gs, act))
        acc(m.fc2.bias, ops.bias_grad(gs))
        del act
        dh = ops.conv1x1_dgrad(gs, m.fc2.weight)
        ops.swin_gelu_bwd(dh, h, out=dh)
        y = ops.swin_layernorm(x1, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        acc(m.fc1.weight, ops.conv1x1_wgrad(dh, y))
        acc(m.fc1.bias, ops.bias_grad(dh))
        dy = ops.conv1x1_dgrad(dh, m.fc1.weight)
        del dh
        dgam, dbet = zeros(self.norm2.weight), zeros(self.norm2.bias)
        ops.swin_layernorm_bwd(dy, x1, self.norm2.weight, self.norm2.eps, dx=g, beta=1.0, dgamma=dgam, dbeta=dbet)
        acc(self.norm2.weight, dgam)
        acc(self.norm2.bias, dbet)
        # attention: proj, the window attention, the bias table, qkv (its bias over the padded map), norm1
        gs = g if s_attn is None else ops.swin_scale_add(None, s_attn, g)
        acc(a.proj.weight, ops.conv1x1_wgrad(gs, att))
        acc(a.proj.bias, ops.bias_grad(gs))
        da = ops.conv1x1_dgrad(gs, a.proj.weight)
        dqkv, ds_part = ops.swin_window_attn_bwd(da, qkv, a.qkv.bias, bias_img, self.window, self.shift)
        acc(a.relative_position_bias_table, ops.swin_bias_table_bwd(ds_part, csr, self.window, zeros(a.relative_position_bias_table)))
        acc(a.qkv.bias, ops.bias_grad(dqkv))
        dqkv = dqkv[:, :, :H, :W]
        y = ops.swin_layernorm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        acc(a.qkv.weight, ops.conv1x1_wgrad(dqkv, y))
        dy = ops.conv1x1_dgrad(dqkv, a.qkv.weight)
        dgam, dbet = zeros(self.norm1.weight), zeros(self.norm1.bias)
        ops.swin_layernorm_bwd(dy, x, self.norm1.weight, self.norm1.eps, dx=g, beta=1.0, dgamma=dgam, dbeta=dbet, want_dx=need_dx)
        acc(self.norm1.weight, dgam)
        acc(self.norm1.bias, dbet)
        return g if need_dx else None


class PatchMerging(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim)

    def run(self, x):
        y = ops.swin_layernorm(x, self.norm.weight, self.norm.bias, self.norm.eps, merge=True)
        return ops.conv1x1_fwd(y, self.reduction.weight)

    def backward(self, x, g, acc):
        """g, the gradient at ``run(x)``'s output -> the gradient at x (fresh): the reduction's 1x1 gradients, then the merge LayerNorm's
        backward, which scatters to the four source pixels."""
        y = ops.swin_layernorm(x, self.norm.weight, self.norm.bias, self.norm.eps, merge=True)
        acc(self.reduction.weight, ops.conv1x1_wgrad(g, y))
        dy = ops.conv1x1_dgrad(g, self.reduction.weight)
        dgam, dbet = torch.zeros_like(self.norm.weight), torch.zeros_like(self.norm.bias)
        dx = ops.swin_layernorm_bwd(dy, x, self.norm.weight, self.norm.eps, merge=True, dgamma=dgam, dbeta=dbet)
        acc(self.norm.weight, dgam)
        acc(self.norm.bias, dbet)
        return dx


class BasicLayer(nn.Module):
    def __init__(self, dim, depth, heads, window, mlp_ratio, downsample):
        super().__init__()
        self.blocks = nn.ModuleList([SwinTransformerBlock(dim, heads, window, 0 if j % 2 == 0 else window // 2, mlp_ratio) for j in range(depth)])
        self.downsample = PatchMerging(dim) if downsample else None


class PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=4, stride=4)
        self.norm = nn.LayerNorm(dim)


class _SwinTrainFn(torch.autograd.Function):
    """A trainable Swin bottom-up as one node, modelled on resnest_backbone._ResNeStTrainFn: ``(net, x, s, *params) -> out_features``; x the
    image batch (no gradient), s the [2 blocks, N] DropPath scales or None, `params` the parameters that require grad.

    Forward: the frozen forward's kernel sequence (``SwinTransformerBlock.run_keep``); the frozen leading parts keep nothing.  Kept per
    trainable block: its input, qkv, the attention output, the stream after the attention branch and fc1's pre-activation; per stage the
    stream before its output norm and before its PatchMerging.  Backward, stages and blocks in reverse: the linears on
    afi_conv1x1_dgrad / _wgrad / afi_colsum_accum, the rest on swin_train.hip's kernels; LayerNorm outputs and the GELU output are recomputed.
    Cotangents may arrive for any subset of the outputs.  Where no gradient is wanted (``torch.no_grad()``) nothing is kept and, without DropPath,
    every block is the frozen ``run``: no copy of fc1's pre-activation."""

    @staticmethod
    @_lib.ctx_forward
    def forward(ctx, net, x, s, *params):
        ctx.set_materialize_grads(False)
        f = net._prepare()
        pe = net.patch_embed
        xf = x.float()
        y = ops.swin_patch_embed(xf, pe.proj.weight, pe.proj.bias, pe.norm.weight, pe.norm.bias, pe.norm.eps)
        last = max(int(n[len("stage"):]) - 2 for n in net._out_features)
        saved, outs = [], []
        ctx.blocks, ctx.stages = [], []                          # (block, index of its 5 kept tensors, index of its s rows); per stage (i, pre-norm, pre-merge)
        keeping = any(ctx.needs_input_grad)                      # False under no_grad: nothing is kept, and without DropPath every block is ``run``
        bi = 0
        for i in range(last + 1):
            layer, train = net.layers[i], i >= net._frozen_layers
            for blk in layer.blocks:
                if train and (keeping or s is not None):
                    y, kept = blk.run_keep(y, f[id(blk)], None if s is None else s[2 * bi], None if s is None else s[2 * bi + 1])
                    if keeping:
                        ctx.blocks.append((i, blk, len(saved), bi))
                        saved += kept
                    del kept
                else:
                    y = blk.run(y, f[id(blk)])
                bi += 1
            name, pre = f"stage{i + 2}", None
            if name in net._out_features:
                norm = getattr(net, f"norm{i}")
                outs.append(ops.swin_layernorm(y, norm.weight, norm.bias, norm.eps))
            if keeping and (name in net._out_features or (train and i < last)):
                pre = len(saved)
                saved.append(y)
            ctx.stages.append((i, pre, name in net._out_features))
            if i < last:
                y = layer.downsample.run(y)
        ctx.image = None
        if keeping and net._train_embed:
            ctx.image = len(saved)
            saved.append(xf)
        ctx.net, ctx.s, ctx.nsaved, ctx.last = net, s, len(saved), last
        ctx.save_for_backward(*saved, *params)
        return tuple(outs)

    @staticmethod
    @_lib.ctx_backward
    def backward(ctx, *douts):
        net, sv, s = ctx.net, ctx.saved_tensors, ctx.s
        saved, params = sv[:ctx.nsaved], sv[ctx.nsaved:]
        f, csr = net._prepare(), net._bias_csr()
        grads = {}

        def acc(p, g):
            grads[id(p)] = g if id(p) not in grads else grads[id(p)] + g

        cots = iter(douts)
        cot = {i: next(cots) for i, _, is_out in ctx.stages if is_out}
        g = None                                                 # the gradient of the stream where the walk stands (None: zero so far)
        for i, pre, is_out in reversed(ctx.stages):
            layer, train = net.layers[i], i >= net._frozen_layers
            if i < ctx.last:                                     # g is the gradient at the PatchMerging's output
                g = layer.downsample.backward(saved[pre], g, acc) if train and g is not None else None
            c = cot.get(i)
            if c is not None:                                    # the output norm: its dx joins the stream's gradient at the stage boundary
                norm, y = getattr(net, f"norm{i}"), saved[pre]
                c = dense_cotangent(c, y)
                dgam, dbet = torch.zeros_like(norm.weight), torch.zeros_like(norm.bias)
                if train:
                    g = ops.swin_layernorm_bwd(c, y, norm.weight, norm.eps, dx=g, beta=0.0 if g is None else 1.0, dgamma=dgam, dbeta=dbet)
                else:
                    ops.swin_layernorm_bwd(c, y, norm.weight, norm.eps, dgamma=dgam, dbeta=dbet, want_dx=False)
                acc(norm.weight, dgam)
                acc(norm.bias, dbet)
            if not train or g is None:
                continue
            mine = [b for b in ctx.blocks if b[0] == i]
            for k, (_, blk, at, bi) in reversed(list(enumerate(mine))):
                below = k > 0 or i > net._frozen_layers or net._train_embed        # something trainable reads this block's input gradient
                g = blk.backward(saved[at:at + 5], f[id(blk)], csr[id(blk)], g, acc, None if s is None else s[2 * bi],
                                 None if s is None else s[2 * bi + 1], need_dx=below)
        if net._train_embed and g is not None:                  # PatchEmbed: the conv as a 1x1 over gathered patches
            pe = net.patch_embed
            C_ = pe.proj.weight.shape[0]
            patches = ops.swin_patch_gather(saved[ctx.image])
            conv = ops.conv1x1_fwd(patches, pe.proj.weight.reshape(C_, 48), pe.proj.bias)
            dgam, dbet = torch.zeros_like(pe.norm.weight), torch.zeros_like(pe.norm.bias)
            dc = ops.swin_layernorm_bwd(g, conv, pe.norm.weight, pe.norm.eps, dgamma=dgam, dbeta=dbet)
            acc(pe.norm.weight, dgam)
            acc(pe.norm.bias, dbet)
            acc(pe.proj.bias, ops.bias_grad(dc))
            acc(pe.proj.weight, ops.conv1x1_wgrad(dc, patches).view(C_, 3, 4, 4))
        by_param = {id(p): k for k, p in enumerate(net._train_params())}
        out = [None] * len(params)
        for pid, gr in grads.items():
            out[by_param[pid]] = gr
        return (None, None, None, *[gr if need else None for gr, need in zip(out, ctx.needs_input_grad[3:])])


class SwinTransformer(nn.Module):
    """The bottom-up: ``forward(x [N,3,H,W]) -> {stage{i+2}: pixel-major fp32 [N, EMBED_DIM 2^i, ceil(H/2^(i+2)), ...]}`` for ``out_features``."""

    def __init__(self, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window_size=7, mlp_ratio=4.0,
                 out_features=("stage2", "stage3", "stage4", "stage5")):
        super().__init__()
        depths, num_heads = list(depths), list(num_heads)
        if len(depths) != len(num_heads) or not depths:
            raise AfiError(f"swin_backbone: SWINT.DEPTHS {depths} and NUM_HEADS {num_heads} must have the same, non-zero length")
        if window_size not in ops.SWIN_WINDOWS:
            raise AfiError(f"swin_backbone: SWINT.WINDOW_SIZE {window_size} is not supported: the attention kernel covers windows "
                           f"{', '.join(map(str, ops.SWIN_WINDOWS))}")
        if embed_dim % 4 or embed_dim > MAX_EMBED_DIM:
            raise AfiError(f"swin_backbone: SWINT.EMBED_DIM {embed_dim} is not supported (a multiple of 4, at most {MAX_EMBED_DIM}: the patch "
                           f"embed and the last patch merging's LayerNorm are held per wave)")
        for i, h in enumerate(num_heads):
            dim = embed_dim * 2 ** i
            if h <= 0 or dim % h or dim // h != HEAD_DIM:
                raise AfiError(f"swin_backbone: stage {i + 2} has head dim {dim}/{h}; the attention kernel needs {HEAD_DIM} (every published "
                               f"Swin T/S/B/L has it)")
            if int(dim * mlp_ratio) % 4:
                raise AfiError(f"swin_backbone: SWINT.MLP_RATIO {mlp_ratio} gives an MLP width {int(dim * mlp_ratio)} that is not a multiple of 4")
        names = [f"stage{i + 2}" for i in range(len(depths))]
        bad = [f for f in out_features if f not in names]
        if bad or not out_features:
            raise AfiError(f"swin_backbone: unknown SWINT.OUT_FEATURES {list(out_features)} (of {names})")
        self._out_features = list(out_features)
        self.num_layers, self.window_size = len(depths), window_size
        self.patch_embed = PatchEmbed(embed_dim)
        self.layers = nn.ModuleList([BasicLayer(embed_dim * 2 ** i, depths[i], num_heads[i], window_size, mlp_ratio, i < len(depths) - 1)
                                     for i in range(len(depths))])
        self.num_features = [embed_dim * 2 ** i for i in range(len(depths))]
        self._out_feature_channels, self._out_feature_strides = {}, {}
        for i, name in enumerate(names):
            if name in self._out_features:
                self._out_feature_channels[name], self._out_feature_strides[name] = self.num_features[i], 4 * 2 ** i
                self.add_module(f"norm{i}", nn.LayerNorm(self.num_features[i]))
        _frozen(self)

    @property
    def size_divisibility(self):
        return 0

    def output_shape(self):
        return {n: ShapeSpec(channels=self._out_feature_channels[n], stride=self._out_feature_strides[n]) for n in self._out_features}

    def _blocks(self):
        return [b for layer in self.layers for b in layer.blocks]

    def _prepare(self):
        """The dense relative-position bias image of every block, rebuilt when a parameter / buffer changes (version, storage, device)."""
        return prepared(self, "bias_images", list(self.parameters()) + list(self.buffers()),
                        lambda: {id(b): b.attn.bias_image() for b in self._blocks()})

    def _check_frozen(self, x):
        check_forward_only(self, x, "the Swin bottom-up")
        if x.dim() != 4 or x.shape[1] != 3:
            raise AfiError(f"the Swin bottom-up takes [N, 3, H, W] images, got {tuple(x.shape)}")

    # ---- training
    _trainable, _frozen_layers, _train_embed, drop_path_rate, _keep_cache = False, 0, False, 0.0, None

    def trainable_(self, freeze_at=-1, drop_path_rate=0.0):
        """Opt in to training, following the reference's ``_freeze_stages``: ``freeze_at >= 0`` keeps ``patch_embed`` frozen, ``freeze_at >= 2``
        also ``layers[0 .. freeze_at - 2]`` (each with its ``downsample``); every other parameter -- the output norms ``norm{i}`` of all
        stages included -- gets ``requires_grad=True`` and ``forward`` runs under autograd (``_SwinTrainFn``).  `drop_path_rate`: stochastic
        depth in ``train()`` mode, block b of sum(depths) at rate ``linspace(0, rate, sum(depths))[b]``.  The state-dict keys do not change.
        Returns self."""
        if isinstance(freeze_at, bool) or not isinstance(freeze_at, int) or not -1 <= freeze_at <= self.num_layers + 1:
            raise AfiError(f"swin_backbone: trainable_(freeze_at={freeze_at!r}): an integer -1 .. {self.num_layers + 1} (BACKBONE.FREEZE_AT)")
        if isinstance(drop_path_rate, bool) or not isinstance(drop_path_rate, (int, float)) or not 0.0 <= drop_path_rate < 1.0:
            raise AfiError(f"swin_backbone: trainable_(drop_path_rate={drop_path_rate!r}): a rate in [0, 1) (SWINT.DROP_PATH_RATE)")
        self._frozen_layers = freeze_at - 1 if freeze_at >= 2 else 0
        self._train_embed = freeze_at < 0
        for p in self.parameters():
            p.requires_grad_(True)
        if not self._train_embed:
            _frozen(self.patch_embed)
        for layer in self.layers[:self._frozen_layers]:
            _frozen(layer)
        self._trainable, self.drop_path_rate = True, float(drop_path_rate)
        return self

    def drop_path_rates(self):
        """The DropPath rate of every block, in ``_blocks()`` order: torch.linspace(0, drop_path_rate, sum(depths)), as the reference builds it."""
        return [float(r) for r in torch.linspace(0, self.drop_path_rate, len(self._blocks()))]

    def _train_params(self):
        return [p for p in self.parameters() if p.requires_grad]

    def _frozen_part_names(self):
        names = ["patch_embed."] if not self._train_embed else []
        return names + [f"layers.{i}." for i in range(self._frozen_layers)]

    def _bias_csr(self):
        """The CSR of every block's relative_position_index (ops.swin_bias_csr), rebuilt when an index buffer changes."""
        blocks = self._blocks()
        return prepared(self, "rel_index_csr", [b.attn.relative_position_index for b in blocks], lambda: {
            id(b): ops.swin_bias_csr(b.attn.relative_position_index, b.window, b.attn.relative_position_bias_table.shape[0]) for b in blocks})

    def _drop_scales(self, N, device, drop_masks):
        """[2 blocks, N]: 0 or 1 / keep per (branch, image) -- row 2 b the attention branch of block b, row 2 b + 1 its MLP -- from
        `drop_masks` (0 / 1, a test's fixed draw) or drawn on the device from torch's generator (floor(keep + U[0, 1)), no host read)."""
        key = (self.drop_path_rate, len(self._blocks()), torch.device(device))
        if self._keep_cache is None or self._keep_cache[0] != key:       # one host-to-device copy per (rate, device), not per forward
            self._keep_cache = (key, 1.0 - torch.tensor(self.drop_path_rates(), dtype=torch.float32).repeat_interleave(2).to(device)[:, None])
        keep = self._keep_cache[1]
        if drop_masks is None:
            mask = torch.floor(keep + torch.rand((keep.shape[0], N), device=device, dtype=torch.float32))
        else:
            if tuple(drop_masks.shape) != (keep.shape[0], N):
                raise AfiError(f"the Swin bottom-up: drop_masks {tuple(drop_masks.shape)} must be [2 blocks, N] = {(keep.shape[0], N)}")
            mask = drop_masks.to(device=device, dtype=torch.float32)
        return (mask / keep).contiguous()

    def _forward_train(self, x, drop_masks):
        what = "the Swin bottom-up"
        if x.dim() != 4 or x.shape[1] != 3:
            raise AfiError(f"{what} takes [N, 3, H, W] images, got {tuple(x.shape)}")
        if x.requires_grad:
            raise AfiError(f"{what}: the input requires grad, but no input gradient exists here (PatchEmbed's backward gives its parameters' only)")
        if x.dtype in (torch.float16, torch.bfloat16):
            raise AfiError(f"{what}: a {x.dtype} input; training runs on fp32 images (AMP / 2-byte activations are out of scope)")
        frozen_parts = self._frozen_part_names()
        stray = [n for n, p in self.named_parameters() if p.requires_grad and n.startswith(tuple(frozen_parts))] if frozen_parts else []
        if stray:
            raise AfiError(f"{what}: {stray[:3]} require grad but belong to a frozen part (trainable_(freeze_at) names the trainable ones)")
        dropping = self.training and self.drop_path_rate > 0.0
        if drop_masks is not None and not dropping:
            raise AfiError(f"{what}: drop_masks given, but DropPath is off (drop_path_rate {self.drop_path_rate}, training {self.training})")
        if not x.is_cuda:
            raise AfiError(f"{what} runs on the GPU only (got a CPU tensor); there is no CPU fallback")
        s = self._drop_scales(x.shape[0], x.device, drop_masks) if dropping else None
        outs = _SwinTrainFn.apply(self, x, s, *self._train_params())
        return dict(zip([f"stage{i + 2}" for i in range(self.num_layers) if f"stage{i + 2}" in self._out_features], outs))

    def forward(self, x, drop_masks=None):
        if self._trainable:
            return self._forward_train(x, drop_masks)
        if drop_masks is not None:
            raise AfiError("the Swin bottom-up: drop_masks belongs to a trainable module (trainable_())")
        self._check_frozen(x)
        with torch.no_grad():
            f = self._prepare()
            pe = self.patch_embed
            y = ops.swin_patch_embed(x.float(), pe.proj.weight, pe.proj.bias, pe.norm.weight, pe.norm.bias, pe.norm.eps)
            last = max(int(n[len("stage"):]) - 2 for n in self._out_features)
            out = {}
            for i in range(last + 1):
                layer = self.layers[i]
                for blk in layer.blocks:
                    y = blk.run(y, f[id(blk)])
                name = f"stage{i + 2}"
                if name in self._out_features:
                    norm = getattr(self, f"norm{i}")
                    out[name] = ops.swin_layernorm(y, norm.weight, norm.bias, norm.eps)
                if i < last:
                    y = layer.downsample.run(y)
        return out


def build_swint_backbone(cfg, input_shape=None):
    """swin_transformer.py's build_swint_backbone restricted to the frozen, forward-only module: refuses every option it does not implement.
    For ``registry.set_bottom_up_builder("swint", build_swint_backbone)`` (opt-in: use_as_bottom_up)."""
    s = cfg_get(cfg.MODEL, "SWINT", None)
    if input_shape is not None and getattr(input_shape, "channels", 3) not in (None, 3):
        raise AfiError(f"swin_backbone: 3 input channels only, got {input_shape.channels}")
    if cfg_get(s, "APE", False):
        raise AfiError("swin_backbone: SWINT.APE True (absolute position embedding) is not supported")
    return SwinTransformer(embed_dim=cfg_get(s, "EMBED_DIM", 96), depths=list(cfg_get(s, "DEPTHS", [2, 2, 6, 2])),
                           num_heads=list(cfg_get(s, "NUM_HEADS", [3, 6, 12, 24])), window_size=cfg_get(s, "WINDOW_SIZE", 7),
                           mlp_ratio=float(cfg_get(s, "MLP_RATIO", 4.0)),
                           out_features=list(cfg_get(s, "OUT_FEATURES", ["stage2", "stage3", "stage4", "stage5"])))


def build_trainable_swint_backbone(cfg, input_shape=None):
    """The Swin bottom-up trainable as the reference's build_swint_backbone leaves it: ``BACKBONE.FREEZE_AT`` (-1 in the BiFPN config: every
    parameter trains) and ``SWINT.DROP_PATH_RATE`` (the reference's default 0.2) through ``SwinTransformer.trainable_``."""
    return build_swint_backbone(cfg, input_shape).trainable_(int(cfg_get(cfg_get(cfg.MODEL, "BACKBONE", None), "FREEZE_AT", -1)),
                                                             float(cfg_get(cfg_get(cfg.MODEL, "SWINT", None), "DROP_PATH_RATE", 0.2)))


def use_as_bottom_up(trainable=False):
    """Opt in: the AFI backbones' "swint" bottom-up lookup (registry.bottom_up_builder) returns this Swin -- what
    build_swint_bifpn_sr_backbone then builds on: frozen and forward-only, or with ``trainable=True`` the one
    ``build_trainable_swint_backbone`` makes (same state-dict keys), which stage 3 trains.  Not the default."""
    registry.set_bottom_up_builder("swint", build_trainable_swint_backbone if trainable else build_swint_backbone)
