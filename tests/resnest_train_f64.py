"""The trainable ResNeSt bottom-up (afigan_amd/resnest_backbone.py) restated plainly: UNFOLDED convs (F.conv2d on the parameters,
groups=2 for the split-attention conv) followed by the norm affine, both average pools (F.avg_pool2d), the pair softmax and
detectron2-ResNeSt's block order, in torch on the CPU, differentiated by autograd; fp64 is the reference, fp32 the yardstick of the bars.
Nothing of the package's kernels, fold or autograd Function is used: only the module's state dict (detectron2-ResNeSt's key names) and its
architecture numbers.

Also here: plain closed forms of what each new kernel writes (split attention's backward, the transposed pools), and the fixtures the host
and GPU tests share, built once per process and never modified by a caller, with the conditions they have to meet
(test_resnest_train_host.py asserts them): every ReLU unit of every trainable block -- conv1's, bn0's, fc1's and the block output's -- has
|pre-activation| > 2^-24 (sum |w x| + |b|) in fp64, so a fp32 evaluation decides the same mask; every conv mask is between 10 % and 90 %
ones; every image has at least one live and one dead fc1 unit in every trainable block; the attention of every trainable block is neither
flat nor saturated (`attention`: max |z0 - z1| <= 8, mean |a0 - 1/2| >= 0.1)."""
import functools

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
BN_EPS = 1e-5
BLOCKS = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3]}


# ------------------------------------------------------------------------------------------------ the restatement
def scale_shift(sd, pre):
    """(s, t) of the norm `pre`: y = s * x + t, s = gamma / sqrt(var + eps)"""
    s = sd[pre + ".weight"] * torch.rsqrt(sd[pre + ".running_var"] + BN_EPS)
    return s, sd[pre + ".bias"] - sd[pre + ".running_mean"] * s


def conv_bn(x, sd, conv, norm, stride=1, pad=0, groups=1, trace=None, add=None, kind="conv"):
    """norm(conv(x) + bias) [+ add], unfolded; with `trace`, appends (name, kind, pre-activation, sum |w' x| + |b'| + |add|)"""
    w, b = sd[conv + ".weight"], sd.get(conv + ".bias")
    one = torch.ones(w.shape[0], dtype=w.dtype)
    s, t = scale_shift(sd, norm) if norm else (one, 0 * one)
    v = lambda a: a.view(1, -1, 1, 1)
    y = F.conv2d(x, w, b, stride, pad, groups=groups) * v(s) + v(t)
    if add is not None:
        y = y + add
    if trace is not None:
        with torch.no_grad():
            bias_mag = (b.abs() * s.abs() if b is not None else 0 * one) + t.abs()
            mag = F.conv2d(x.abs(), w.abs(), None, stride, pad, groups=groups) * v(s.abs()) + v(bias_mag)
            if add is not None:
                mag = mag + add.abs()
            trace.append((conv, kind, y.detach(), mag))
    return y


def splat(x, sd, pre, trace=None):
    """splat.py's SplAtConv2d (radix 2, cardinality 1) and rSoftMax: returns a0 s0 + a1 s1"""
    C = sd[pre + ".conv.weight"].shape[0] // 2
    y = torch.relu(conv_bn(x, sd, pre + ".conv", pre + ".bn0", 1, 1, 2, trace))
    s0, s1 = y[:, :C], y[:, C:]
    g = (s0 + s1).mean((2, 3), keepdim=True)
    h = torch.relu(conv_bn(g, sd, pre + ".fc1", pre + ".bn1", trace=trace, kind="fc1"))
    z = conv_bn(h, sd, pre + ".fc2", None)
    a = torch.softmax(z.view(-1, 2, C), dim=1)
    if trace is not None:
        trace.append((pre, "att", (z.view(-1, 2, C)[:, 0] - z.view(-1, 2, C)[:, 1]).detach(), a[:, 0].detach()))
    return a[:, 0].reshape(-1, C, 1, 1) * s0 + a[:, 1].reshape(-1, C, 1, 1) * s1


def block(x, sd, pre, stride, trace=None):
    """resnest.py's BottleneckBlock (radix 2, AVD, avg_down): relu(conv3(avd(splat(relu(conv1(x))))) + shortcut(x))"""
    if pre + ".shortcut.weight" in sd:
        xs = F.avg_pool2d(x, stride, stride, ceil_mode=True, count_include_pad=False) if stride > 1 else x
        sc = conv_bn(xs, sd, pre + ".shortcut", pre + ".shortcut.norm")
    else:
        sc = x
    y = torch.relu(conv_bn(x, sd, pre + ".conv1", pre + ".conv1.norm", trace=trace))
    y = splat(y, sd, pre + ".conv2", trace)
    if stride > 1:
        y = F.avg_pool2d(y, 3, stride, padding=1)
    return torch.relu(conv_bn(y, sd, pre + ".conv3", pre + ".conv3.norm", trace=trace, add=sc))


def stem(x, sd):
    y = torch.relu(conv_bn(x, sd, "stem.conv1_1", "stem.conv1_1.norm", 2, 1))
    y = torch.relu(conv_bn(y, sd, "stem.conv1_2", "stem.conv1_2.norm", 1, 1))
    y = torch.relu(conv_bn(y, sd, "stem.conv1_3", "stem.conv1_3.norm", 1, 1))
    return F.max_pool2d(y, 3, 2, 1)


def resnest(x, sd, counts, out_features, trace_from=None, trace=None):
    """{name: feature} of the bottom-up; `trace` collects the ReLU units of the stages res{trace_from + 1}.. (the trainable ones)"""
    out, y = {}, stem(x, sd)
    for i, n in enumerate(counts):
        name = f"res{i + 2}"
        tr = trace if trace is not None and i + 2 > trace_from else None
        for j in range(n):
            y = block(y, sd, f"{name}.{j}", (1 if i == 0 else 2) if j == 0 else 1, tr)
        if name in out_features:
            out[name] = y
    return out


# ------------------------------------------------------------------------------------------------ closed forms of the new kernels' outputs
def avg2s2_ceil_T(dy, H, W):
    """transpose of avg_pool2d(2, 2, ceil_mode=True, count_include_pad=False) on an H x W map: every pixel gets dy of its window / the
    pixels that window covered"""
    idx_y, idx_x = torch.arange(H) // 2, torch.arange(W) // 2
    cnt = lambda n: torch.minimum(2 * (torch.arange(n) // 2) + 2, torch.tensor(n)) - 2 * (torch.arange(n) // 2)
    div = (cnt(H).view(-1, 1) * cnt(W).view(1, -1)).to(dy.dtype)
    return dy[:, :, idx_y][:, :, :, idx_x] / div


def avg3s2p1_sources(n):
    """per coordinate 0..n-1: the output coordinates whose 3-wide stride-2 padding-1 window holds it (1 or 2 of them)"""
    no = (n - 1) // 2 + 1
    return [[o for o in range(no) if 2 * o - 1 <= y <= 2 * o + 1] for y in range(n)]


def avg3s2p1_T(dy, H, W):
    """transpose of avg_pool2d(3, 2, padding=1) (divisor 9 everywhere), gather form: a pixel adds the dy of the windows that hold it"""
    sy, sx = avg3s2p1_sources(H), avg3s2p1_sources(W)
    out = torch.zeros(dy.shape[:2] + (H, W), dtype=dy.dtype)
    for y in range(H):
        for x in range(W):
            for oy in sy[y]:
                for ox in sx[x]:
                    out[:, :, y, x] += dy[:, :, oy, ox]
    return out / 9


def splat_forward(s0, s1, w1, b1, w2, b2):
    """(g, h, att) of split attention over the splits: w1 [I, C] / b1 with bn1 folded, w2 [2C, I]"""
    N, C = s0.shape[:2]
    g = (s0 + s1).mean((2, 3))
    h = torch.relu(g @ w1.t() + b1)
    att = torch.softmax((h @ w2.t() + b2).view(N, 2, C), dim=1).reshape(N, 2 * C)
    return g, h, att


def splat_bwd_da(du, s0, s1):
    """[N, 2C]: sum over pixels of du * s0, then of du * s1"""
    return torch.cat([(du * s0).sum((2, 3)), (du * s1).sum((2, 3))], dim=1)


def splat_bwd_dz(da, att):
    C = att.shape[1] // 2
    d = att[:, :C] * att[:, C:] * (da[:, :C] - da[:, C:])
    return torch.cat([d, -d], dim=1)


def splat_bwd_dh(dz, h, w2):
    return (dz @ w2) * (h > 0).to(dz.dtype)


def splat_bwd_dg(dh, w1, hw):
    return (dh @ w1) / hw


def splat_bwd_ds(du, s, a, dg):
    """(a du + dg) [s > 0] for one split: a, dg [N, C]"""
    v = lambda t: t.reshape(t.shape[0], -1, 1, 1)
    return (v(a) * du + v(dg)) * (s > 0).to(du.dtype)


# ------------------------------------------------------------------------------------------------ fixtures
def randomise(module, seed):
    """Norm buffers away from the identity, so the fold and its chain rule matter; fc biases away from zero and fc1's weights large enough
    that the attention leaves 1/2 without saturating (`attention` below); conv3 damped so the residual sum stays O(1) through the stages."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, b in module.named_buffers():
            if k.endswith(".weight") or k.endswith(".running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
            elif k.endswith(".bias") or k.endswith(".running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
        for k, p in module.named_parameters():
            if ".fc1." in k or ".fc2." in k:
                p.copy_(0.3 * torch.randn(p.shape, generator=g) if k.endswith(".bias") else (1.5 if ".fc1." in k else 1.0) * p)
            elif ".conv3." in k:
                p.mul_(0.5)
    return module


NETS = {
    # name: (constructor keywords, input shape, seed); freeze_at 1 and 2 are both run on it
    "small": (dict(depth=50, width_per_group=8, res2_out_channels=16), (2, 3, 64, 96), 5),           # res2 16x24, res3 8x12, res4 4x6, res5 2x3
}
FREEZE_ATS = (1, 2)


def make_net(name):
    """(module on the CPU, input image): the same weights for every caller (seeded)"""
    from afigan_amd import resnest_backbone
    kw, shape, seed = NETS[name]
    torch.manual_seed(seed)
    net = randomise(resnest_backbone.ResNeSt(**kw), seed + 100)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed + 200))
    return net, x


def counts_of(name):
    kw = NETS[name][0]
    outs = kw.get("out_features", ("res2", "res3", "res4", "res5"))
    return BLOCKS[kw["depth"]][:max(int(o[3:]) for o in outs) - 1], list(outs)


def trainable_keys(sd, freeze_at):
    """the state-dict keys ResNeSt.trainable_(freeze_at) makes trainable: conv weights and the fc1 / fc2 weights and biases of the later stages"""
    norm = (".norm.", ".bn0.", ".bn1.")
    return [k for k in sd if k.startswith("res") and int(k[3]) > freeze_at and not any(n in k for n in norm)]


@functools.lru_cache(maxsize=None)
def cotangents(name):
    net, x = make_net(name)
    with torch.no_grad():
        counts, outs = counts_of(name)
        sd = {k: v.double() for k, v in net.state_dict().items()}
        feats = resnest(x.double(), sd, counts, outs)
    g = torch.Generator().manual_seed(NETS[name][2] + 300)
    return {k: torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in feats.items()}


@functools.lru_cache(maxsize=None)
def reference(name, freeze_at, dtype):
    """(outputs, parameter gradients) of sum_k <feature_k, cotangent_k> in `dtype` on the CPU; callers must not modify them"""
    net, x = make_net(name)
    counts, outs = counts_of(name)
    sd = {k: v.to(dtype) for k, v in net.state_dict().items()}
    keys = trainable_keys(sd, freeze_at)
    for k in keys:
        sd[k].requires_grad_(True)
    feats = resnest(x.to(dtype), sd, counts, outs)
    cot = cotangents(name)
    sum((feats[k] * cot[k].to(dtype)).sum() for k in feats).backward()
    return {k: v.detach() for k, v in feats.items()}, {k: sd[k].grad for k in keys}


@functools.lru_cache(maxsize=None)
def margins(name, freeze_at):
    """[(unit name, kind, min |pre| / (2^-24 mag), fraction of ones, min and max live units per image)] over the ReLU units of the trainable
    blocks, fp64"""
    net, x = make_net(name)
    counts, outs = counts_of(name)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    trace = []
    with torch.no_grad():
        resnest(x.double(), sd, counts, outs, trace_from=freeze_at, trace=trace)
    rows = []
    for n, kind, pre, mag in trace:
        if kind == "att":
            continue
        live = (pre > 0).flatten(1).sum(1)
        rows.append((n, kind, (pre.abs() / (EPS * mag)).min().item(), (pre > 0).double().mean().item(), int(live.min()), int(live.max()),
                     pre[0].numel()))
    return rows


@functools.lru_cache(maxsize=None)
def attention(name, freeze_at):
    """[(block, max |z0 - z1|, mean |a0 - 1/2|)] over the trainable blocks, fp64.  The pair softmax turns an ABSOLUTE error of its logits into
    a RELATIVE error of the attention and of dz = a0 a1 (da0 - da1): logits rounded in fp32 carry about 2^-24 |z| sqrt(I), so a fixture with
    |z0 - z1| in the tens (a saturated attention) makes every fp32 evaluation -- torch's on the CPU as much as the kernels' -- differ from
    fp64 by tens of 2^-24 in everything behind the attention, and a comparison of two such evaluations decides nothing.  The fixtures keep
    |z0 - z1| <= 8 (a >= 3e-4) and, so that the attention still matters, mean |a0 - 1/2| >= 0.1."""
    net, x = make_net(name)
    counts, outs = counts_of(name)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    trace = []
    with torch.no_grad():
        resnest(x.double(), sd, counts, outs, trace_from=freeze_at, trace=trace)
    return [(n, d.abs().max().item(), (a0 - 0.5).abs().mean().item()) for n, kind, d, a0 in trace if kind == "att"]


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


# ------------------------------------------------------------------------------------------------ the kernels' inputs and geometry
GAP_BYTES = 65536                # RS_GAP_BYTES of csrc/afi_resnest.h


def gap_chunks(H, W, C):
    """(chunks, pixels per chunk, pixel slots of a block) of the pooled-sum passes for a split of C channels"""
    slots = 256 // (C // 4)
    pix = max(GAP_BYTES // (4 * C), slots)
    return -(-H * W // pix), pix, slots


@functools.lru_cache(maxsize=None)
def splat_case(N, C, I, H, W, avd, seed=0):
    """fp32 inputs of the split-attention backward: post-ReLU splits (about half zeros), fc weights that move the attention off 1/2 and leave
    live and dead fc1 units in every image, bn1's fold scale, and dout at the (pooled, with avd) output size"""
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W + seed)
    r = lambda *s: torch.randn(s, generator=g)
    s0, s1 = torch.relu(r(N, C, H, W)), torch.relu(r(N, C, H, W) + 0.3)
    w1, b1 = r(I, C) * (2.0 / C ** 0.5), 0.05 * r(I)
    gm = (s0 + s1).double().mean((2, 3))
    b1 = (b1.double() - (gm @ w1.double().t()).mean(0)).float()       # centre fc1's pre-activation: units on both sides of zero
    w2, b2 = r(2 * C, I) * (3.0 / I ** 0.5), 0.1 * r(2 * C)
    s1_scale = 0.5 + torch.rand(I, generator=g)
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if avd else (H, W)
    return dict(s0=s0, s1=s1, w1=w1, b1=b1, w2=w2, b2=b2, s1_scale=s1_scale, dout=r(N, C, Ho, Wo))
