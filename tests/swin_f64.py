"""Test infrastructure: the Swin Transformer bottom-up restated in torch.nn.functional (any dtype, any device), the weight rule of
tests/golden/swin_tiny.npz, and helpers to fill afigan_amd.swin_backbone.SwinTransformer with it.

The restatement is written from the published Swin semantics (pad after norm1, roll(-shift), window partition, relative-position bias,
-100 across shift regions, PatchMerging's cat order), not from the kernels.  test_swin_host.py checks it against the reference's own
outputs in the golden fixture, so the GPU tests can use it as the fp64 yardstick on any size.  Used by tests/test_swin_host.py,
tests/test_gpu_swin.py and tools/swin_bench.py."""
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swin_tiny.npz")
TINY = dict(EMBED_DIM=32, DEPTHS=[2, 2, 2, 2], NUM_HEADS=[1, 2, 4, 8], WINDOW_SIZE=7, MLP_RATIO=4.0, DROP_PATH_RATE=0.2, APE=False,
            OUT_FEATURES=["stage2", "stage3", "stage4", "stage5"])


def weight_rule(key, shape):
    """Legacy RandomState seeded with crc32(key): linear / conv weights N(0, 1) / sqrt(fan-in), biases N(0, 0.2^2), LayerNorm weights
    1 + N(0, 0.1^2), relative-position bias tables N(0, 0.5^2) (the same rule as tests/golden/make_golden_swin.py)."""
    rs = np.random.RandomState(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    z = rs.standard_normal(shape)
    if key.endswith("relative_position_bias_table"):
        return 0.5 * z
    if key.endswith("bias"):
        return 0.2 * z
    if len(shape) == 1:
        return 1.0 + 0.1 * z
    return z / np.sqrt(np.prod(shape[1:]))


def fill(model):
    """Every parameter of `model` from weight_rule (fp32), buffers as built."""
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(weight_rule(k, tuple(p.shape))).to(torch.float32))
    return model


def golden_image():
    g = np.load(GOLDEN)
    return torch.from_numpy(np.random.RandomState(int(g["image_seed"])).standard_normal(tuple(g["image_shape"]))).float()


def layer_norm(x, w, b, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def shift_mask(Hp, Wp, ws, shift, dtype, device):
    """[nW, N, N]: -100 between tokens of different 3x3 shift regions of the padded map, 0 elsewhere."""
    reg = torch.zeros(Hp, Wp, dtype=torch.long, device=device)
    bounds = lambda L: [(0, L - ws), (L - ws, L - shift), (L - shift, L)]
    for a, (h0, h1) in enumerate(bounds(Hp)):
        for c, (w0, w1) in enumerate(bounds(Wp)):
            if h1 > max(h0, 0) and w1 > max(w0, 0):
                reg[max(h0, 0):h1, max(w0, 0):w1] = 3 * a + c
    r = reg.view(Hp // ws, ws, Wp // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    return torch.where(r[:, None, :] != r[:, :, None], -100.0, 0.0).to(dtype)


def attention_from_qkv(qkv, qkv_b, table, index, heads, ws, shift):
    """qkv [B, H, W, 3C] (channel s C + head d_h + d) -> [B, H, W, C]: the map padded to multiples of ws with tokens whose q / k / v are
    qkv_b (what the linear gives a zero-padded norm1 output), rolled by -shift, window attention with the relative-position bias and, when
    shifted, the region mask; reversed, rolled back, cropped."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    x = F.pad(qkv - qkv_b, (0, 0, 0, Wp - W, 0, Hp - H)) + qkv_b
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    win = x.reshape(B, Hp // ws, ws, Wp // ws, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C3)
    n, d = ws * ws, C // heads
    qkv = win.view(-1, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * d ** -0.5, qkv[1], qkv[2]
    att = q @ k.transpose(-2, -1) + table[index.reshape(-1)].view(n, n, heads).permute(2, 0, 1)
    if shift:
        nW = (Hp // ws) * (Wp // ws)
        att = (att.view(B, nW, heads, n, n) + shift_mask(Hp, Wp, ws, shift, att.dtype, att.device)[None, :, None]).view(-1, heads, n, n)
    y = (att.softmax(-1) @ v).transpose(1, 2).reshape(-1, n, C)
    y = y.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift:
        y = torch.roll(y, (shift, shift), (1, 2))
    return y[:, :H, :W]


def window_attention(x, qkv_w, qkv_b, proj_w, proj_b, table, index, heads, ws, shift):
    """x [B, H, W, C] (already norm1'ed, not padded) -> proj(attention) [B, H, W, C]."""
    return F.linear(attention_from_qkv(F.linear(x, qkv_w, qkv_b), qkv_b, table, index, heads, ws, shift), proj_w, proj_b)


def merge_gather(x):
    """PatchMerging's gather of x [B, H, W, C] -> [B, ceil(H/2), ceil(W/2), 4C] (odd sizes zero-padded)."""
    B, H, W, C = x.shape
    x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)


def patch_embed(img, w, b, nw, nb, eps=1e-5):
    """img [B, 3, H, W] -> tokens [B, ceil(H/4), ceil(W/4), C]."""
    H, W = img.shape[-2:]
    img = F.pad(img, (0, (-W) % 4, 0, (-H) % 4))
    return layer_norm(F.conv2d(img, w, b, stride=4).permute(0, 2, 3, 1), nw, nb, eps)


def forward(model, img, dtype=torch.float64, device="cpu"):
    """The bottom-up of `model` (a SwinTransformer: only its weights, config and out_features are read) on `img`, in `dtype` on `device`:
    {stage: [B, C, H, W]} contiguous."""
    sd = {k: v.detach().to(device) for k, v in model.state_dict().items()}
    P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x = patch_embed(img.to(device, dtype), P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], P["patch_embed.norm.weight"],
                    P["patch_embed.norm.bias"])
    ws = model.window_size
    out = {}
    for i, layer in enumerate(model.layers):
        for j, blk in enumerate(layer.blocks):
            p = f"layers.{i}.blocks.{j}."
            heads = blk.attn.heads
            y = layer_norm(x, P[p + "norm1.weight"], P[p + "norm1.bias"])
            x = x + window_attention(y, P[p + "attn.qkv.weight"], P[p + "attn.qkv.bias"], P[p + "attn.proj.weight"], P[p + "attn.proj.bias"],
                                     P[p + "attn.relative_position_bias_table"], P[p + "attn.relative_position_index"], heads, ws,
                                     0 if j % 2 == 0 else ws // 2)
            y = layer_norm(x, P[p + "norm2.weight"], P[p + "norm2.bias"])
            x = x + F.linear(F.gelu(F.linear(y, P[p + "mlp.fc1.weight"], P[p + "mlp.fc1.bias"])), P[p + "mlp.fc2.weight"], P[p + "mlp.fc2.bias"])
        name = f"stage{i + 2}"
        if name in model._out_features:
            out[name] = layer_norm(x, P[f"norm{i}.weight"], P[f"norm{i}.bias"]).permute(0, 3, 1, 2).contiguous()
        if layer.downsample is not None:
            p = f"layers.{i}.downsample."
            x = F.linear(layer_norm(merge_gather(x), P[p + "norm.weight"], P[p + "norm.bias"]), P[p + "reduction.weight"])
    return out


def rel_err(a, ref):
    """(relative L2, max-norm relative to max |ref|) of a against ref, in float64."""
    a, ref = a.double().cpu(), ref.double().cpu()
    return float((a - ref).norm() / ref.norm()), float((a - ref).abs().max() / ref.abs().max())
