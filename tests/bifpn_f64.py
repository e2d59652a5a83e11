"""float64 yardsticks, launch geometry and case tables of the BiFPN node kernels: fusion + swish and its backward, the depthwise 3x3 and its weight
gradient, the zero-padded 3x3/2 max-pool with its argmax and backward (csrc/elementwise.hip, csrc/bifpn_train.hip), and the pass-through kernels
next to them: afi_relu_bwd, afi_nearest_nhwc and the two layout transposes.  tests/test_bifpn_host.py holds this module to torch's own float64
ops and autograd and to the path every case names; tests/test_gpu_bifpn_kernels.py compares the kernels with it.

Every arithmetic reference takes the kernel's fp32 INPUTS as CPU NCHW tensors, widens them to float64 and returns (result, terms): terms is, per
element, the sum of the magnitudes that the kernel rounds on the way to that element, each weighted by how far its rounding moves the result
(first order).  The selections (max-pool value and tap, nearest, the transposes) are evaluated in the input's own dtype: they copy, so their
bits can be compared.  Nothing here touches a GPU."""
import torch
import torch.nn.functional as F

from elementwise_f64 import BLOCK, C_MAX, EPS, EW_GRID_CAP, d, elementwise_bar, errs, ew_grid, f32, reduction_bars  # noqa: F401 (re-exported)

# ------------------------------------------------------------------------------------------------ launch geometry (pure functions)
BT_GRID_CAP = 1024              # AFI_BT_MAX_BLOCKS (csrc/bifpn_train.hip)
DWW_MAX_CHUNKS = 256            # AFI_DWW_MAX_CHUNKS
NEAREST_GRID_CAP = 8192         # afi_nearest_nhwc (csrc/resnet_guide.hip)
TILE = {"nchw_to_nhwc": (32, 64), "nhwc_to_nchw": (32, 32)}     # (channels, pixels) of a block: afi_widen_nchw_kernel<F32>, afi_nhwc_to_nchw_kernel


def bt_grid(items):
    """csrc/bifpn_train.hip: afi_bt_grid -- blocks of 256 threads, capped at 1024, at least one"""
    return max(1, min(BT_GRID_CAP, (items + 255) // 256))


def nearest_grid(items):
    """csrc/resnet_guide.hip: afi_nearest_nhwc -- ceil(items / 256) blocks, capped at 8192"""
    return min(NEAREST_GRID_CAP, (items + 255) // 256)


def dww_geometry(P):
    """csrc/bifpn_train.hip: afi_dwconv3x3_wgrad -- (chunks, rows_per_chunk) over the P = N*H*W pixels"""
    want = min(DWW_MAX_CHUNKS, (P + 63) // 64)
    rpc = (P + want - 1) // want
    return (P + rpc - 1) // rpc, rpc


def pool_out(h):
    """output extent of MaxPool2d(3, 2, "static_same") along an axis of h >= 2"""
    return (h - 2) // 2 + 1


def nearest_out(h, up, down):
    return (h * up + down - 1) // down


PATHS = {
    "fuse_swish": ("grid_stride", "partial_last_pass"),
    "fuse_swish_bwd": ("grid_stride", "partial_last_pass", "finalize_strided"),
    "dwconv3x3": ("grid_stride", "partial_last_pass"),
    "dwconv3x3_wgrad": ("chunk_cap", "partial_last_chunk", "image_boundary_inside_chunk", "partial_channel_block", "second_channel_block",
                        "finalize_unrolled"),
    "maxpool": ("grid_stride", "partial_last_pass", "pad_row", "pad_col"),
    "maxpool_idx": ("grid_stride", "partial_last_pass", "pad_row", "pad_col"),
    "maxpool_bwd": ("grid_stride", "partial_last_pass", "pad_row", "pad_col"),
    "relu_bwd": ("grid_stride", "partial_last_pass"),
    "nearest": ("grid_stride", "partial_last_pass"),
    "nchw_to_nhwc": ("multi_tile_p", "multi_tile_c", "partial_tile"),
    "nhwc_to_nchw": ("multi_tile_p", "multi_tile_c", "partial_tile"),
}


def _strided(items, blocks):
    """a grid-stride loop of `items` float4 items on `blocks` x 256 threads: some thread takes a second item; the last pass is not full"""
    threads = BLOCK * blocks
    out = set()
    if items > threads:
        out.add("grid_stride")
        if items % threads:
            out.add("partial_last_pass")
    return out


def path_of(op, shape):
    """What the launch of `op` on `shape` exercises, as a frozenset over PATHS[op].  shape is (N, C, H, W) of the op's INPUT (of dy / x for the
    weight gradient, of the pooled map's input for all three max-pool ops), (N, C, H, W, up, down) for nearest and (N, C, P) for the transposes.
      grid_stride / partial_last_pass   the launch is capped and a thread takes a second float4 item / the last pass over the grid is not full
      finalize_strided                  afi_fuse_swish_bwd_finalize_kernel: more than 64 block partials, so a lane sums several, and their count
                                        is no multiple of 64, so the lanes sum unequal numbers of them
      chunk_cap                         N*H*W > 64 * 256: rows_per_chunk > 64
      partial_last_chunk                the last chunk is shorter than the others
      image_boundary_inside_chunk       a chunk holds the last pixel of one image and the first of the next (the row decode must wrap)
      partial_channel_block / second_channel_block      C % 128 != 0 / C > 128
      finalize_unrolled                 afi_dwconv3x3_wgrad_finalize_kernel: the 4-way loop runs and leaves a tail (chunks >= 4, chunks % 4 != 0)
      pad_row / pad_col                 even H / even W: the last window reaches the zero pad row / column
      multi_tile_p / multi_tile_c / partial_tile        more than one tile along the pixels / the channels; a tile cut by either extent"""
    if op in ("nchw_to_nhwc", "nhwc_to_nchw"):
        _, Cc, P = shape
        tc, tp = TILE[op]
        out = set()
        if P > tp:
            out.add("multi_tile_p")
        if Cc > tc:
            out.add("multi_tile_c")
        if P % tp or Cc % tc:
            out.add("partial_tile")
        return frozenset(out)
    if op == "nearest":
        N, Cc, H, W, up, down = shape
        items = N * nearest_out(H, up, down) * nearest_out(W, up, down) * (Cc // 4)
        return frozenset(_strided(items, nearest_grid(items)))
    N, Cc, H, W = shape
    items = N * H * W * (Cc // 4)
    if op in ("fuse_swish", "dwconv3x3", "relu_bwd"):
        return frozenset(_strided(items, ew_grid(items)))
    if op == "fuse_swish_bwd":
        blocks = bt_grid(items)
        out = _strided(items, blocks)
        if blocks > 64 and blocks % 64:
            out.add("finalize_strided")
        return frozenset(out)
    if op in ("maxpool", "maxpool_idx", "maxpool_bwd"):
        oitems = N * pool_out(H) * pool_out(W) * (Cc // 4)
        out = _strided(oitems, ew_grid(oitems)) if op == "maxpool" else _strided(oitems, bt_grid(oitems)) if op == "maxpool_idx" \
            else _strided(items, bt_grid(items))
        if H % 2 == 0:
            out.add("pad_row")
        if W % 2 == 0:
            out.add("pad_col")
        return frozenset(out)
    if op == "dwconv3x3_wgrad":
        P = N * H * W
        chunks, rpc = dww_geometry(P)
        out = set()
        if (P + 63) // 64 > DWW_MAX_CHUNKS:
            out.add("chunk_cap")
        if P % rpc:
            out.add("partial_last_chunk")
        if any((k * H * W) % rpc for k in range(1, N)):
            out.add("image_boundary_inside_chunk")
        if Cc % 128:
            out.add("partial_channel_block")
        if Cc > 128:
            out.add("second_channel_block")
        if chunks >= 4 and chunks % 4:
            out.add("finalize_unrolled")
        return frozenset(out)
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------ case tables
def S(*names):
    return frozenset(names)


_TINY = [(1, 4, 1, 1), (1, 8, 1, 7), (2, 8, 5, 1)]              # a single row or column: centre taps only along the short axis
_TINY_POOL = [(1, 4, 2, 2), (1, 8, 2, 5), (2, 8, 5, 2)]         # the pool needs H, W >= 2
_MID = (2, 132, 7, 9)                                           # C = 128 + 4, 4158 items, 126 pixels
_STRIDED = (1, 132, 23, 29)                                     # 22 011 items: 86 blocks = 64 + 22 partials for the swish finalizer
_BWD_CAP = (2, 132, 67, 63)                                     # 278 586 items = 1.06 x the backward cap; 8442 pixels: 132 chunks of 64, the last of 58
_FWD_CAP = (2, 132, 95, 89)                                     # 558 030 items = 1.06 x the forward cap, 2.13 x the backward cap; 16 910 pixels:
                                                                # rows_per_chunk 67, 253 chunks (252 + a tail of 1), the last of 26, image 0 ends inside chunk 126
_IDX_CAP = (2, 132, 135, 125)                                   # 67 x 62 outputs: 274 164 items = 1.05 x the backward cap; odd H and W
_POOL_CAP = (2, 132, 190, 176)                                  # 95 x 88 outputs: 551 760 items = 1.05 x the forward cap; even H and W

# op -> [(shape, paths)]
CASES = {
    "fuse_swish": [(s, S()) for s in _TINY + [_MID]] + [(_FWD_CAP, S("grid_stride", "partial_last_pass"))],
    "fuse_swish_bwd": [(s, S()) for s in _TINY + [_MID]] + [(_STRIDED, S("finalize_strided")), (_BWD_CAP, S("grid_stride", "partial_last_pass")),
                                                            (_FWD_CAP, S("grid_stride", "partial_last_pass"))],
    "dwconv3x3": [(s, S()) for s in _TINY + [_MID]] + [(_FWD_CAP, S("grid_stride", "partial_last_pass"))],
    "dwconv3x3_wgrad": [
        ((1, 4, 1, 1), S("partial_channel_block")),
        ((1, 8, 1, 7), S("partial_channel_block")),
        ((2, 8, 5, 1), S("partial_channel_block", "image_boundary_inside_chunk")),              # one chunk of 10 rows holds both images
        (_MID, S("partial_channel_block", "second_channel_block")),                             # 2 chunks of 63 = one image each
        ((2, 128, 7, 9), S()),                                                                  # C = 128: one full channel block
        (_BWD_CAP, S("partial_channel_block", "second_channel_block", "partial_last_chunk", "image_boundary_inside_chunk")),
        (_FWD_CAP, S("partial_channel_block", "second_channel_block", "partial_last_chunk", "image_boundary_inside_chunk", "chunk_cap",
                     "finalize_unrolled")),
    ],
    "maxpool": [((1, 4, 2, 2), S("pad_row", "pad_col")), ((1, 8, 2, 5), S("pad_row")), ((2, 8, 5, 2), S("pad_col")), (_MID, S()),
                (_POOL_CAP, S("grid_stride", "partial_last_pass", "pad_row", "pad_col"))],
    "maxpool_idx": [((1, 4, 2, 2), S("pad_row", "pad_col")), ((1, 8, 2, 5), S("pad_row")), ((2, 8, 5, 2), S("pad_col")), (_MID, S()),
                    ((2, 132, 8, 6), S("pad_row", "pad_col")), (_IDX_CAP, S("grid_stride", "partial_last_pass"))],
    "maxpool_bwd": [((1, 4, 2, 2), S("pad_row", "pad_col")), ((1, 8, 2, 5), S("pad_row")), ((2, 8, 5, 2), S("pad_col")), (_MID, S()),
                    ((2, 132, 8, 6), S("pad_row", "pad_col")), (_BWD_CAP, S("grid_stride", "partial_last_pass")),
                    (_IDX_CAP, S("grid_stride", "partial_last_pass"))],
    "relu_bwd": [(s, S()) for s in _TINY + [_MID]] + [(_FWD_CAP, S("grid_stride", "partial_last_pass"))],
    "nearest": [((2, 64, 5, 7, 2, 1), S()), ((2, 64, 5, 7, 1, 2), S()), ((1, 8, 1, 7, 3, 2), S()), ((1, 132, 127, 125, 2, 1), S()),     # 2 095 500 items
                ((1, 132, 128, 125, 2, 1), S("grid_stride", "partial_last_pass"))],                                                     # 2 112 000 > 2 097 152
}
POOL_FAMILIES = ("random", "negative", "zeros", "halves")
TRANSPOSE_N, TRANSPOSE_C, TRANSPOSE_P = (1, 3), (1, 3, 31, 32, 33, 100), (1, 63, 64, 65, 2049)


def rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def pool_input(family, shape, seed=0):
    """the fp32 input of a max-pool case.  negative: every element <= -1, the zero pad wins wherever a window reaches it; zeros: every
    window is one nine-way tie; halves: multiples of 1/2 (-0.0 among them), ties in most windows -- the first maximum in scan order wins"""
    r = rand(shape, 300 + seed)
    if family == "random":
        return r
    if family == "negative":
        return -r.abs() - 1.0
    if family == "zeros":
        return torch.zeros(shape)
    if family == "halves":
        return (r * 2).round() / 2
    raise KeyError(family)


SWISH_W3, SWISH_W2 = (0.4, 1.1, -0.7), (0.9, -1.2)


def swish_bwd_inputs(shape, n_in=3):
    """(w, a, b, c or None, dout) of a fusion-backward case: positive inputs, weights of both signs (s = sum w_k x_k takes both signs, about
    -4 .. 6) and a positive cotangent, so that ds x_k hardly changes sign and |dw_k| is a good fraction of sum |ds x_k| (asserted on the CPU)"""
    w = torch.tensor(SWISH_W3 if n_in == 3 else SWISH_W2)
    xs = [rand(shape, 40 + k).abs() + 0.1 for k in range(n_in)]
    dout = rand(shape, 44).abs() + 0.5
    return w, xs[0], xs[1], (xs[2] if n_in == 3 else None), dout


# ------------------------------------------------------------------------------------------------ float64 references: fusion + swish
def _fusion(w, a, b, c):
    xs = [d(a), d(b)] + ([d(c)] if c is not None else [])
    ws = [float(v) for v in w.detach().double().flatten()]
    assert len(ws) == len(xs)
    s = sum(wk * x for wk, x in zip(ws, xs))
    Ts = sum(abs(wk) * x.abs() for wk, x in zip(ws, xs))
    return ws, xs, s, Ts


def fuse_swish(w, a, b, c=None):
    """(out, terms): s = sum w_k x_k, out = s sigmoid(s).  terms = |f'(s)| sum |w_k x_k| + |out|, f'(s) = sig (1 + s (1 - sig)): the roundings
    of s reach out through f', those of 1 + e and of the division are relative to out"""
    _, _, s, Ts = _fusion(w, a, b, c)
    sg = torch.sigmoid(s)
    out = s * sg
    return out, (sg * (1 + s * (1 - sg))).abs() * Ts + out.abs()


def fuse_swish_exp(w, a, b, c=None):
    """(|s|, gain): a relative error q of the exponential e = exp(-s) moves out by gain * q, gain = |s| e / (1 + e)^2 = |s| sig (1 - sig)"""
    _, _, s, _ = _fusion(w, a, b, c)
    sg = torch.sigmoid(s)
    return s.abs(), s.abs() * sg * (1 - sg)


def fuse_swish_bwd(w, a, b, c, dout):
    """((dw, da, db, dc), (tw, ta, tb, tc)): ds = dout sig (1 + s (1 - sig)), d{a,b,c} = w_k ds, dw_k = sum ds x_k (dc, tc None without c).
    terms of ds, in the kernel's sequence sg = 1 / (1 + e), u = 1 - sg, q = 1 + s u, ds = (dout sg) q:
        |dout| sig (|1 + s - 2 s sig| + |s| (1 - sig) + |q|)  +  |dout f''(s)| sum |w_k x_k|,   f'' = sig (1 - sig) (2 + s (1 - 2 sig))
    (d ds / d sg = dout (1 + s - 2 s sg); d ds / d u = dout sg s; the last three roundings are relative to q and ds); t{a,b,c} = |w_k| times
    that; tw_k = sum |ds x_k|, the denominator of the condition under which dw_k has a relative bar."""
    ws, xs, s, Ts = _fusion(w, a, b, c)
    g = d(dout)
    sg = torch.sigmoid(s)
    q = 1 + s * (1 - sg)
    ds = g * sg * q
    f2 = sg * (1 - sg) * (2 + s * (1 - 2 * sg))
    tds = g.abs() * sg * ((1 + s - 2 * s * sg).abs() + s.abs() * (1 - sg) + q.abs()) + (g * f2).abs() * Ts
    dw = torch.stack([(ds * x).sum() for x in xs])
    tw = torch.stack([(ds * x).abs().sum() for x in xs])
    dx = [wk * ds for wk in ws] + [None] * (3 - len(ws))
    tx = [abs(wk) * tds for wk in ws] + [None] * (3 - len(ws))
    return (dw, dx[0], dx[1], dx[2]), (tw, tx[0], tx[1], tx[2])


def fuse_swish_bwd_exp(w, a, b, c, dout):
    """(|s|, gain of ds): a relative error q of e = exp(-s) moves sig by sig (1 - sig) q and ds by |dout (1 + s - 2 s sig)| sig (1 - sig) q;
    d{a,b,c} by |w_k| times that"""
    _, _, s, _ = _fusion(w, a, b, c)
    sg = torch.sigmoid(s)
    return s.abs(), (d(dout) * (1 + s - 2 * s * sg)).abs() * sg * (1 - sg)


# ------------------------------------------------------------------------------------------------ float64 references: depthwise 3x3
def _taps(xp, H, W):
    """the nine shifted [N, C, H, W] windows of a map padded by 1, tap t = 3 ty + tx reading x[y + ty - 1][x + tx - 1]"""
    return [xp[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9)]


def dwconv3x3(x, w9c):
    """(out, terms): depthwise 3x3, stride 1, zero pad 1, w9c [9][C] tap-major; terms = sum_t |w_t x_t|"""
    H, W = x.shape[2:]
    w = d(w9c)

    def f(xp, wt):
        return sum(wt[t].view(1, -1, 1, 1) * v for t, v in enumerate(_taps(xp, H, W)))
    xp = F.pad(d(x), (1, 1, 1, 1))
    return f(xp, w), f(xp.abs(), w.abs())


def dwconv3x3_wgrad(dy, x):
    """(dw9c, terms), both [9][C]: dw[t][c] = sum over n, y, x of dy x_t; terms = sum |dy x_t|"""
    H, W = x.shape[2:]
    g = d(dy)
    prods = [g * v for v in _taps(F.pad(d(x), (1, 1, 1, 1)), H, W)]
    return torch.stack([p.sum((0, 2, 3)) for p in prods]), torch.stack([p.abs().sum((0, 2, 3)) for p in prods])


# ------------------------------------------------------------------------------------------------ references: max-pool (selections)
def maxpool3s2_same(x, want_taps=True):
    """(value, tap): zero pad right and bottom by 1, 3x3 windows at stride 2; tap = 3 dy + dx of the FIRST maximum in scan order, the pad
    included (uint8; None when not wanted), value = the element at that tap, in x's own dtype (the sign of a zero is the first one's)"""
    xp = F.pad(x, (0, 1, 0, 1))
    if not want_taps and not bool((x == 0).any()):
        return F.max_pool2d(xp, 3, 2), None                     # (no zero among the inputs: no sign to decide, the maximum's bits are unique)
    win = xp.unfold(2, 3, 2).unfold(3, 3, 2).reshape(*x.shape[:2], pool_out(x.shape[2]), pool_out(x.shape[3]), 9)
    m = win.max(-1, keepdim=True).values
    tap = torch.where(win == m, torch.arange(9), torch.tensor(9)).min(-1).values
    return win.gather(-1, tap.unsqueeze(-1)).squeeze(-1), (tap.to(torch.uint8) if want_taps else None)


def maxpool3s2_same_bwd(dout, tap, in_hw):
    """(dx, terms): dx[n][c][y][x] = sum of dout over the windows whose tap points at (y, x); a window won by the pad sends its gradient
    nowhere.  terms = the same gather of |dout|."""
    H, W = in_hw
    N, Cc, Ho, Wo = dout.shape
    g, t = d(dout), tap.long()

    def f(v):
        acc = torch.zeros((N, Cc, 2 * Ho + 1, 2 * Wo + 1), dtype=torch.float64)
        for k in range(9):
            acc[:, :, k // 3:k // 3 + 2 * Ho:2, k % 3:k % 3 + 2 * Wo:2] += torch.where(t == k, v, torch.zeros((), dtype=torch.float64))
        return acc[:, :, :H, :W].clone()
    return f(g), f(g.abs())


# ------------------------------------------------------------------------------------------------ references: the pass-through kernels
def relu_bwd(g, act, scale=1.0):
    """(out, terms): out = scale g where act > 0, else 0; terms = |out| (one product)"""
    out = torch.where(d(act) > 0, f32(scale) * d(g), torch.zeros((), dtype=torch.float64))
    return out, out.abs()


def nearest(x, up, down):
    """out[n][c][oy][ox] = x[n][c][oy down / up][ox down / up], Ho = ceil(H up / down); a copy, in x's own dtype"""
    H, W = x.shape[2:]
    iy = torch.arange(nearest_out(H, up, down)) * down // up
    ix = torch.arange(nearest_out(W, up, down)) * down // up
    return x.index_select(2, iy).index_select(3, ix)


def nchw_to_nhwc(x):
    """[N][C][P] -> [N][P][C], a copy"""
    return x.permute(0, 2, 1).contiguous()


def nhwc_to_nchw(x):
    """[N][P][C] -> [N][C][P], a copy"""
    return x.permute(0, 2, 1).contiguous()


def bits(t):
    """the int32 view of an fp32 tensor: -0.0 and NaN payloads count in a comparison"""
    return t.detach().cpu().contiguous().view(torch.int32)
