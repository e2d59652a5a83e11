"""fp64 restatement of the mask branch of StandardROIHeads at inference (detectron2 v0.1.1 semantics, afigan_amd/roi_heads.py's docstring), the
checker of tests/test_gpu_mask.py and tests/test_mask_host.py: plain numpy / torch on the CPU, stage by stage so that a test can feed each
stage the KERNEL's previous output.  Stages: a 3x3 conv + ReLU, the deconv as the 4-phase layout, the selected logit and its sigmoid, the
paste value with its error bar.

The paste coordinates are written in the order the semantics state them -- gx = (x + 0.5 - x0) / (x1 - x0) 2 - 1, ix = ((gx + 1) M - 1) / 2,
left to right -- which is the order the kernel evaluates them in, in fp64, so tap indices agree bit for bit; the sum is then taken through two
per-axis weight matrices, which is not how the kernel does it."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the head
def conv_relu(x, weight, bias, dtype=torch.float64):
    """relu(conv2d(x, weight [O, I, 3, 3], bias, padding 1)) in `dtype` on the CPU."""
    return torch.relu(F.conv2d(x.detach().cpu().to(dtype), weight.detach().cpu().to(dtype), bias.detach().cpu().to(dtype), padding=1))


def deconv_phases(x, weight, bias, dtype=torch.float64):
    """relu(ConvTranspose2d(kernel 2, stride 2)(x)) as the 4-phase layout [R, 4 Cout, S, S]: channel (2a + b) Cout + co at (y, x) is output
    pixel (2y + a, 2x + b) of channel co.  weight [Cin, Cout, 2, 2]."""
    x, w, b = x.detach().cpu().to(dtype), weight.detach().cpu().to(dtype), bias.detach().cpu().to(dtype)
    up = torch.relu(F.conv_transpose2d(x, w, b, stride=2))                       # [R, Cout, 2S, 2S]
    return torch.cat([up[:, :, a::2, c::2] for a in (0, 1) for c in (0, 1)], 1)


def head_chain(pooled, params, dtype=torch.float64, prefix="mask_head."):
    """([every conv's output], the deconv's 4-phase output) of the whole head from its input, in `dtype`."""
    x, acts, i = pooled, [], 1
    while f"{prefix}mask_fcn{i}.weight" in params:
        x = conv_relu(x, params[f"{prefix}mask_fcn{i}.weight"], params[f"{prefix}mask_fcn{i}.bias"], dtype)
        acts.append(x)
        i += 1
    return acts, deconv_phases(x, params[f"{prefix}deconv.weight"], params[f"{prefix}deconv.bias"], dtype)


def selected_logits(h, weight, bias, classes, counts):
    """h [N D, 4 C, S, S] (the 4-phase layout), weight [Km, C(, 1, 1)], bias [Km], classes [N, D], counts [N].  Returns (z [N D, 2S, 2S] fp64,
    mag [N D, 2S, 2S] = sum |w h| + |b|, live [N D] bool); rows past counts and rows with a class outside 0 .. Km - 1 are not live (z = 0)."""
    h = np.asarray(h, np.float64)
    w = np.asarray(weight, np.float64).reshape(len(bias), -1)
    b = np.asarray(bias, np.float64)
    Km, C = w.shape
    R, _, S, _ = h.shape
    N, D = np.asarray(classes).shape
    z, mag, live = np.zeros((R, 2 * S, 2 * S)), np.zeros((R, 2 * S, 2 * S)), np.zeros(R, bool)
    for r in range(R):
        n, d = divmod(r, D)
        c = 0 if Km == 1 else int(classes[n][d])
        if d >= int(counts[n]) or not 0 <= c < Km:
            continue
        live[r] = True
        for a in (0, 1):
            for e in (0, 1):
                ph = h[r, (2 * a + e) * C:(2 * a + e + 1) * C]                      # [C, S, S]
                z[r, a::2, e::2] = np.einsum("k,kyx->yx", w[c], ph) + b[c]
                mag[r, a::2, e::2] = np.einsum("k,kyx->yx", np.abs(w[c]), np.abs(ph)) + abs(b[c])
    return z, mag, live


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


# ------------------------------------------------------------------------------------------------ the paste
def _axis(lo, hi, size, M):
    """(Wm [size, M] fp64 bilinear weights of every pixel centre on the mask's axis, inside [size] bool)."""
    c = np.arange(size, dtype=np.float64) + 0.5
    g = (c - lo) / (hi - lo) * 2.0 - 1.0
    i = ((g + 1.0) * float(M) - 1.0) / 2.0
    fl = np.floor(i)
    l = i - fl
    Wm = np.zeros((size, M))
    for p in range(size):
        t = int(fl[p]) if np.isfinite(fl[p]) and abs(fl[p]) < 1e9 else -10
        if 0 <= t < M:
            Wm[p, t] += 1.0 - l[p]
        if 0 <= t + 1 < M:
            Wm[p, t + 1] += l[p]
    return Wm, (c >= lo) & (c <= hi)


def paste(probs, boxes, H, W):
    """probs [R, M, M], boxes [R, 4] fp32.  Returns (v [R, H, W] fp64: the bilinear value at EVERY pixel, e [R, H, W] = 8 2^-24 sum |w m|: four
    fp32-rounded weights and four fused multiply-adds, inside [R, H, W] bool: the pixel's centre lies in the box).  A box with a non-positive
    (or NaN) side: v = 0, nothing inside."""
    m = np.asarray(probs, np.float32).astype(np.float64)
    b = np.asarray(boxes, np.float32).astype(np.float64)
    R, M = m.shape[:2]
    v, e, inside = np.zeros((R, H, W)), np.zeros((R, H, W)), np.zeros((R, H, W), bool)
    for r in range(R):
        x0, y0, x1, y1 = b[r]
        if not (x1 - x0 > 0 and y1 - y0 > 0):
            continue
        Wy, iy = _axis(y0, y1, H, M)
        Wx, ix = _axis(x0, x1, W, M)
        v[r] = Wy @ m[r] @ Wx.T
        e[r] = 8 * EPS * (Wy @ np.abs(m[r]) @ Wx.T)
        inside[r] = iy[:, None] & ix[None, :]
    return v, e, inside


def paste_decided(v, e, inside, threshold=0.5):
    """(want [R, H, W] bool = inside and v >= threshold, sure [R, H, W] bool: outside pixels, and inside pixels with |v - threshold| > e)."""
    return inside & (v >= threshold), ~inside | (np.abs(v - threshold) > e)


# ------------------------------------------------------------------------------------------------ paste test inputs
PASTE_CASES = ((37, 53, 28), (37, 53, 7), (16, 32, 28), (16, 32, 7))       # (H, W, M): a row length that is no multiple of 16, and one that is
PASTE_SEED = 3
PASTE_LEFT_OUT = 1e-3                                                    # at most this share of the inside pixels may be undecided


def paste_boxes(H, W):
    """fp32 [R, 4]: inside the image, touching and exceeding each edge, sides below one pixel, zero and negative width, one wider than 56 px."""
    return np.array([
        (5.3, 4.7, 0.6 * W + 0.2, 0.7 * H + 0.4),      # inside
        (0, 0, W, H),                                  # touches every edge
        (0, 2.5, 0.4 * W, H),                          # touches left and bottom
        (0.5 * W, 0, W, 0.5 * H + 0.25),               # touches right and top
        (-7.5, -3.25, W + 9.5, H + 20),                # exceeds every edge
        (-4.2, 3.1, 11.7, H + 2.6),                    # exceeds left and bottom
        (W - 9.3, -2.8, W + 3.9, 9.4),                 # exceeds right and top
        (10.25, 7.5, 10.75, 7.875),                    # sides below one pixel, no centre inside
        (12.3, 5.2, 12.9, 5.9),                        # sides below one pixel around the centre (12.5, 5.5)
        (20, 3, 20, 12),                               # zero width
        (25, 4, 15, 12),                               # negative width
        (3, 9, 14, 9),                                 # zero height
        (-12.6, 1.3, 58.1, H - 1.2),                   # wider than 2 * 28 pixels
        (1.5, 1.5, W - 1.5, H - 1.5),                  # edges exactly on pixel centres
    ], np.float32)


def paste_masks(R, M, seed=PASTE_SEED):
    """fp32 [R, M, M]: row r is a smooth random probability map (r % 4 == 0 or 1), a binary {0, 1} mask (2), all-zero / all-one (3, in turn)."""
    g = torch.Generator().manual_seed(seed + M)
    out = np.zeros((R, M, M), np.float32)
    for r in range(R):
        if r % 4 in (0, 1):
            low = torch.randn((1, 1, 4, 4), generator=g, dtype=torch.float64) * 2.5
            out[r] = torch.sigmoid(F.interpolate(low, size=(M, M), mode="bicubic", align_corners=False))[0, 0].numpy().clip(0, 1)
        elif r % 4 == 2:
            out[r] = (torch.rand((M, M), generator=g) < 0.5).numpy()
        else:
            out[r] = float((r // 4) % 2)
    return out


def paste_case(H, W, M):
    boxes = paste_boxes(H, W)
    boxes = np.concatenate([boxes, boxes[[0, 4, 12, 1, 5, 6]]])          # the large boxes again, so that each meets another kind of mask
    return paste_masks(len(boxes), M), boxes


# ------------------------------------------------------------------------------------------------ predictor test inputs
PROBS_COUNTS = ((5, 0), (3, 5))


def probs_case(C, S, Km, seed=7):
    """(h [10, 4 C, S, S] fp32 >= 0 (a ReLU output), w [Km, C], bias [Km], classes [2, 5] int32 with 0 and Km - 1 among the live rows)."""
    g = torch.Generator().manual_seed(seed + C + 31 * S + 977 * Km)
    h = torch.relu(torch.randn((10, 4 * C, S, S), generator=g)).numpy()
    w = (torch.randn((Km, C), generator=g) * (3.0 / np.sqrt(C))).numpy()
    b = (torch.randn((Km,), generator=g) * 0.5).numpy()
    cls = torch.randint(0, Km, (2, 5), generator=g).numpy().astype(np.int32)
    cls[:, 0], cls[:, 1], cls[:, 2] = 0, Km - 1, Km // 2
    cls[1, 4] = Km - 1
    return h, w, b, cls
