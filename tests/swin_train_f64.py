"""Test infrastructure: the backward of the Swin bottom-up in closed form (any dtype; fp64 is the reference), each written out from its
formula and not through autograd, and the whole network's gradients by torch autograd through the restatement of tests/swin_f64.py.

Closed forms: LayerNorm backward with and without PatchMerging's gather, GELU backward, window-attention backward from qkv (dq / dk / dv
over the PADDED map, the sum of dS, the bias-table gradient through the index buffer), the patch gather and DropPath's scale-add.
tests/test_swin_train_host.py holds them to fp64 autograd; tests/test_gpu_swin_train.py holds the kernels to them.

The network: ``forward(model, img, ...)`` is swin_f64.forward's body over a dict of parameter LEAVES (swin_f64.forward detaches what it
reads, so it cannot give parameter gradients itself; the host test holds the two together to fp64 rounding) with DropPath restated beside it:
each branch output times s[n] in {0, 1 / keep} before the residual add.  No package code is used beyond state dicts and the module's
configuration."""
import math

import torch
import torch.nn.functional as F

import swin_f64 as S


# ------------------------------------------------------------------------------------------------ closed forms
def merge_scatter(d, H, W):
    """The transpose of swin_f64.merge_gather: d [B, ceil(H/2), ceil(W/2), 4C] -> [B, H, W, C]; quadrants past an odd edge are dropped."""
    B, Ho, Wo, C4 = d.shape
    C = C4 // 4
    out = d.new_zeros((B, 2 * Ho, 2 * Wo, C))
    out[:, 0::2, 0::2] = d[..., 0:C]
    out[:, 1::2, 0::2] = d[..., C:2 * C]
    out[:, 0::2, 1::2] = d[..., 2 * C:3 * C]
    out[:, 1::2, 1::2] = d[..., 3 * C:]
    return out[:, :H, :W]


def layernorm_bwd(dy, x, gamma, eps=1e-5, merge=False):
    """x [B, H, W, C], dy [B, Ho, Wo, Ct] -> (dx [B, H, W, C], dgamma [Ct], dbeta [Ct], terms of dx in the normalised layout):
    g = dy gamma;  dx = rstd (g - mean(g) - xhat mean(g xhat));  dgamma = sum dy xhat;  dbeta = sum dy."""
    B, H, W, _ = x.shape
    xin = S.merge_gather(x) if merge else x
    mean = xin.mean(-1, keepdim=True)
    rstd = (((xin - mean) ** 2).mean(-1, keepdim=True) + eps) ** -0.5
    xh = (xin - mean) * rstd
    g = dy * gamma
    m1, m2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    dxin = rstd * (g - m1 - xh * m2)
    terms = rstd * (g.abs() + m1.abs() + (xh * m2).abs())
    dx = merge_scatter(dxin, H, W) if merge else dxin
    return dx, (dy * xh).sum((0, 1, 2)), dy.sum((0, 1, 2)), (merge_scatter(terms, H, W) if merge else terms)


def gelu_bwd(dy, x):
    """dy (Phi(x) + x phi(x))"""
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return dy * (cdf + x * pdf)


def _windows(x, ws, shift):
    """[B, Hp, Wp, K] -> rolled by -shift and partitioned: [B nW, ws^2, K]"""
    B, Hp, Wp, K = x.shape
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    return x.reshape(B, Hp // ws, ws, Wp // ws, ws, K).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, K)


def _unwindows(w, B, Hp, Wp, ws, shift):
    K = w.shape[-1]
    x = w.view(B, Hp // ws, Wp // ws, ws, ws, K).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, K)
    return torch.roll(x, (shift, shift), (1, 2)) if shift else x


def attention_probs(qkv, qkv_b, table, index, heads, ws, shift):
    """(q scaled, k, v, P) per window and head, [B nW, heads, n, .], of the padded, rolled map; plus (Hp, Wp)."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    x = F.pad(qkv - qkv_b, (0, 0, 0, Wp - W, 0, Hp - H)) + qkv_b
    n, d = ws * ws, C // heads
    win = _windows(x, ws, shift).view(-1, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = win[0] * d ** -0.5, win[1], win[2]
    att = q @ k.transpose(-2, -1) + table[index.reshape(-1)].view(n, n, heads).permute(2, 0, 1)
    if shift:
        nW = (Hp // ws) * (Wp // ws)
        att = (att.view(B, nW, heads, n, n) + S.shift_mask(Hp, Wp, ws, shift, att.dtype, att.device)[None, :, None]).view(-1, heads, n, n)
    return q, k, v, att.softmax(-1), Hp, Wp


def attention_bwd(dout, qkv, qkv_b, table, index, heads, ws, shift):
    """The backward of swin_f64.attention_from_qkv for dout [B, H, W, C], by the formulas
        dV = P^T dO,  dP = dO V^T,  dS = P (dP - rowsum(dP P)),  dQ = d^-1/2 dS K,  dK = d^-1/2 dS^T Q.
    Returns (dqkv over the PADDED, un-rolled map [B, Hp, Wp, 3C] -- padded positions carry gradients of qkv_b --,
    d bias image [heads, n, n] = the sum of dS over images and windows, d table [R, heads])."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    n, d = ws * ws, C // heads
    q, k, v, P, Hp, Wp = attention_probs(qkv, qkv_b, table, index, heads, ws, shift)
    do = _windows(F.pad(dout, (0, 0, 0, Wp - W, 0, Hp - H)), ws, shift).view(-1, n, heads, d).permute(0, 2, 1, 3)
    dv = P.transpose(-2, -1) @ do
    dP = do @ v.transpose(-2, -1)
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    dq = (dS @ k) * d ** -0.5                                   # k unscaled; q above is already scaled
    dk = dS.transpose(-2, -1) @ q
    dwin = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(-1, n, C3)          # [B nW, n, (s, head, d)]
    dbias = dS.sum(0)
    dtable = torch.zeros_like(table).index_add_(0, index.reshape(-1), dbias.permute(1, 2, 0).reshape(n * n, heads))
    return _unwindows(dwin, B, Hp, Wp, ws, shift), dbias, dtable


def patch_gather(img):
    """img [B, 3, H, W] -> [B, ceil(H/4), ceil(W/4), 48], channel 16 ci + 4 ky + kx, zero past the image: proj.weight.reshape(C, 48)'s order."""
    B, _, H, W = img.shape
    x = F.pad(img, (0, (-W) % 4, 0, (-H) % 4))
    Ho, Wo = x.shape[2] // 4, x.shape[3] // 4
    return x.view(B, 3, Ho, 4, Wo, 4).permute(0, 2, 4, 1, 3, 5).reshape(B, Ho, Wo, 48)


def scale_add(a, s, b):
    """a + s[n] b over [B, ...] tensors (a None: s[n] b)"""
    sb = s.view(-1, *([1] * (b.dim() - 1))) * b
    return sb if a is None else a + sb


# ------------------------------------------------------------------------------------------------ the network
def leaves(model, dtype=torch.float64, device="cpu"):
    """{key: tensor} of model.state_dict() in `dtype` on `device`, floating-point entries as autograd leaves."""
    out = {}
    for k, v in model.state_dict().items():
        v = v.detach().to(device)
        out[k] = v.to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v
    return out


def drop_path_rates(model, rate):
    return [float(r) for r in torch.linspace(0, rate, sum(len(layer.blocks) for layer in model.layers))]


def drop_scales(model, rate, masks, dtype=torch.float64):
    """[2 blocks, B]: masks (0 / 1; row 2 b the attention branch of block b, row 2 b + 1 its MLP) over keep_b = 1 - rate_b."""
    keep = 1.0 - torch.tensor(drop_path_rates(model, rate), dtype=torch.float32).repeat_interleave(2)[:, None]
    return (masks.float() / keep).to(dtype)


def forward(model, P, img, scales=None):
    """swin_f64.forward's body over the parameter dict P (its dtype and device): {stage: [B, C, H, W]}; `scales` [2 blocks, B]: DropPath."""
    x = S.patch_embed(img, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], P["patch_embed.norm.weight"], P["patch_embed.norm.bias"])
    ws = model.window_size
    out = {}
    b = 0
    join = lambda x, y, row: x + y if scales is None else scale_add(x, scales[row].to(y.device), y)      # noqa: E731
    for i, layer in enumerate(model.layers):
        for j, blk in enumerate(layer.blocks):
            p = f"layers.{i}.blocks.{j}."
            heads = blk.attn.heads
            y = S.layer_norm(x, P[p + "norm1.weight"], P[p + "norm1.bias"])
            x = join(x, S.window_attention(y, P[p + "attn.qkv.weight"], P[p + "attn.qkv.bias"], P[p + "attn.proj.weight"], P[p + "attn.proj.bias"],
                                           P[p + "attn.relative_position_bias_table"], P[p + "attn.relative_position_index"], heads, ws,
                                           0 if j % 2 == 0 else ws // 2), 2 * b)
            y = S.layer_norm(x, P[p + "norm2.weight"], P[p + "norm2.bias"])
            x = join(x, F.linear(F.gelu(F.linear(y, P[p + "mlp.fc1.weight"], P[p + "mlp.fc1.bias"])), P[p + "mlp.fc2.weight"], P[p + "mlp.fc2.bias"]),
                     2 * b + 1)
            b += 1
        name = f"stage{i + 2}"
        if name in model._out_features:
            out[name] = S.layer_norm(x, P[f"norm{i}.weight"], P[f"norm{i}.bias"]).permute(0, 3, 1, 2).contiguous()
        if layer.downsample is not None:
            p = f"layers.{i}.downsample."
            x = F.linear(S.layer_norm(S.merge_gather(x), P[p + "norm.weight"], P[p + "norm.bias"]), P[p + "reduction.weight"])
    return out


def network_grads(model, img, cots, dtype=torch.float64, device="cpu", scales=None):
    """(outputs, {key: gradient}) of sum_k <out[k], cots[k]> by autograd through `forward`, in `dtype` on `device`; keys without a path to
    the chosen outputs are absent."""
    P = leaves(model, dtype, device)
    out = forward(model, P, img.to(device, dtype), None if scales is None else scales.to(device, dtype))
    loss = sum((out[k] * c.to(device, dtype)).sum() for k, c in cots.items())
    keys = [k for k, v in P.items() if v.is_floating_point()]
    grads = torch.autograd.grad(loss, [P[k] for k in keys], allow_unused=True)
    return {k: v.detach() for k, v in out.items()}, {k: g for k, g in zip(keys, grads) if g is not None}


# ------------------------------------------------------------------------------------------------ fixture conditions
QKV_SCALE = 0.7         # swin_f64.weight_rule as it stands gives the tiny network a largest softmax logit gap of 9.58 on the golden image; with every
                        # attn.qkv weight and bias times 0.7 it is 5.83 (the bar of test_swin_train_host.py is 8), both measured in fp64 alone


def fill(model):
    """The network fixture of the training tests: swin_f64.fill, then attn.qkv.{weight, bias} times QKV_SCALE (see there)."""
    S.fill(model)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith(("attn.qkv.weight", "attn.qkv.bias")):
                p.mul_(QKV_SCALE)
    return model


def conditioning(model, P, img):
    """(min over LayerNorm input tokens of var / mean square, max over softmax rows of the largest gap between unmasked logits) of the
    network on `img`: what tests/test_swin_train_host.py bounds so that the GPU bars compare code, not conditioning."""
    worst_var, worst_gap = [float("inf")], [0.0]

    def ln(x, w, b):
        var = ((x - x.mean(-1, keepdim=True)) ** 2).mean(-1)
        worst_var[0] = min(worst_var[0], float((var / (x * x).mean(-1)).min()))
        return S.layer_norm(x, w, b)

    x = F.conv2d(F.pad(img, (0, (-img.shape[-1]) % 4, 0, (-img.shape[-2]) % 4)), P["patch_embed.proj.weight"], P["patch_embed.proj.bias"],
                 stride=4).permute(0, 2, 3, 1)
    x = ln(x, P["patch_embed.norm.weight"], P["patch_embed.norm.bias"])
    ws = model.window_size
    for i, layer in enumerate(model.layers):
        for j, blk in enumerate(layer.blocks):
            p = f"layers.{i}.blocks.{j}."
            heads, shift = blk.attn.heads, 0 if j % 2 == 0 else ws // 2
            y = ln(x, P[p + "norm1.weight"], P[p + "norm1.bias"])
            qkv = F.linear(y, P[p + "attn.qkv.weight"], P[p + "attn.qkv.bias"])
            prob = attention_probs(qkv, P[p + "attn.qkv.bias"], P[p + "attn.relative_position_bias_table"], P[p + "attn.relative_position_index"],
                                   heads, ws, shift)[3]
            live = prob > math.exp(-50.0)                         # a masked pair sits 100 below: not part of the row's own spread
            logp = torch.where(live, prob.log(), torch.zeros_like(prob))
            gap = logp.max(-1).values - torch.where(live, logp, torch.full_like(prob, float("inf"))).min(-1).values
            worst_gap[0] = max(worst_gap[0], float(gap.max()))
            x = x + S.window_attention(y, P[p + "attn.qkv.weight"], P[p + "attn.qkv.bias"], P[p + "attn.proj.weight"], P[p + "attn.proj.bias"],
                                       P[p + "attn.relative_position_bias_table"], P[p + "attn.relative_position_index"], heads, ws, shift)
            y = ln(x, P[p + "norm2.weight"], P[p + "norm2.bias"])
            x = x + F.linear(F.gelu(F.linear(y, P[p + "mlp.fc1.weight"], P[p + "mlp.fc1.bias"])), P[p + "mlp.fc2.weight"], P[p + "mlp.fc2.bias"])
        if f"stage{i + 2}" in model._out_features:
            ln(x, P[f"norm{i}.weight"], P[f"norm{i}.bias"])
        if layer.downsample is not None:
            p = f"layers.{i}.downsample."
            x = F.linear(ln(S.merge_gather(x), P[p + "norm.weight"], P[p + "norm.bias"]), P[p + "reduction.weight"])
    return worst_var[0], worst_gap[0]
