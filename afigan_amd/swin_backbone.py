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
BACKBONE.FREEZE_AT change neither the key set nor an eval forward: accepted and ignored."""
import torch
import torch.nn as nn

from . import ops, registry
from ._lib import AfiError
from .fpn_sr import ShapeSpec
from .frozen import cfg_get, check_forward_only, prepared

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


class PatchMerging(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim)

    def run(self, x):
        y = ops.swin_layernorm(x, self.norm.weight, self.norm.bias, self.norm.eps, merge=True)
        return ops.conv1x1_fwd(y, self.reduction.weight)


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

    def forward(self, x):
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


def use_as_bottom_up():
    """Opt in: the AFI backbones' "swint" bottom-up lookup (registry.bottom_up_builder) returns this frozen, forward-only Swin -- what
    build_swint_bifpn_sr_backbone then builds on.  Not the default: stage 3 trains its bottom-up, which this module cannot."""
    registry.set_bottom_up_builder("swint", build_swint_backbone)
