"""The trainable ResNet bottom-up (afigan_amd/resnet_guide.py) restated plainly: UNFOLDED convs (F.conv2d on the parameters) followed by
the FrozenBN affine, in torch on the CPU, differentiated by autograd; fp64 is the reference, fp32 the yardstick of the bars.  Nothing of the
package's kernels, fold or autograd Function is used: only the module's state dict (detectron2's key names) and its architecture numbers.

Also here: the fixtures the host and GPU tests share (a small ResNet-50 with all four stages, a full-width one down to res3, single blocks),
built once per process and never modified by a caller, and the conditions they have to meet (test_resnet_train_host.py asserts them):
every ReLU unit of every trainable block has |pre-activation| > 2^-24 (sum |w x| + |b|) in fp64, so a fp32 evaluation decides the same mask,
and every mask is between 10 % and 90 % ones."""
import functools

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
BN_EPS = 1e-5
BLOCKS = {50: [3, 4, 6, 3]}


def scale_shift(sd, pre):
    """(s, t) of the FrozenBN `pre`.norm: y = s * x + t, s = gamma / sqrt(var + eps)"""
    s = sd[pre + ".norm.weight"] * torch.rsqrt(sd[pre + ".norm.running_var"] + BN_EPS)
    return s, sd[pre + ".norm.bias"] - sd[pre + ".norm.running_mean"] * s


def conv_bn(x, sd, pre, stride, pad, trace=None, add=None):
    """FrozenBN(conv(x)) [+ add], unfolded; with `trace`, appends (name, pre-activation, sum |w' x| + |b'| + |add|)"""
    w = sd[pre + ".weight"]
    s, t = scale_shift(sd, pre)
    y = F.conv2d(x, w, None, stride, pad) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)
    if add is not None:
        y = y + add
    if trace is not None:
        with torch.no_grad():
            mag = F.conv2d(x.abs(), w.abs(), None, stride, pad) * s.abs().view(1, -1, 1, 1) + t.abs().view(1, -1, 1, 1)
            if add is not None:
                mag = mag + add.abs()
            trace.append((pre, y.detach(), mag))
    return y


def block(x, sd, pre, stride, stride_in_1x1=True, trace=None):
    """detectron2's BottleneckBlock: relu(conv3(relu(conv2(relu(conv1(x))))) + shortcut(x)); the shortcut conv exists iff its weight does"""
    s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)
    sc = conv_bn(x, sd, pre + ".shortcut", stride, 0) if pre + ".shortcut.weight" in sd else x
    y = torch.relu(conv_bn(x, sd, pre + ".conv1", s1, 0, trace))
    y = torch.relu(conv_bn(y, sd, pre + ".conv2", s3, 1, trace))
    return torch.relu(conv_bn(y, sd, pre + ".conv3", 1, 0, trace, add=sc))


def stem(x, sd):
    return F.max_pool2d(torch.relu(conv_bn(x, sd, "stem.conv1", 2, 3)), 3, 2, 1)


def resnet(x, sd, counts, out_features, stride_in_1x1=True, trace_from=None, trace=None):
    """{name: feature} of the bottom-up; `trace` collects the ReLU units of the stages res{trace_from + 1}.. (the trainable ones)"""
    out, y = {}, stem(x, sd)
    for i, n in enumerate(counts):
        name = f"res{i + 2}"
        tr = trace if trace is not None and i + 2 > trace_from else None
        for j in range(n):
            y = block(y, sd, f"{name}.{j}", (1 if i == 0 else 2) if j == 0 else 1, stride_in_1x1, tr)
        if name in out_features:
            out[name] = y
    return out


def randomise_norms(module, seed):
    """FrozenBN buffers away from the identity, so that the fold and its chain rule matter: gamma in 0.5..1.5, var in 0.5..1.5, small beta / mean"""
    g = torch.Generator().manual_seed(seed)
    for k, b in module.named_buffers():
        if k.endswith("norm.weight") or k.endswith("norm.running_var"):
            b.copy_(0.5 + torch.rand(b.shape, generator=g))
        elif k.endswith("norm.bias") or k.endswith("norm.running_mean"):
            b.copy_(0.1 * torch.randn(b.shape, generator=g))
    return module


# ------------------------------------------------------------------------------------------------ the networks of the tests
NETS = {
    # name: (constructor keywords, freeze_at, input shape, seed)
    "small": (dict(depth=50, width_per_group=8, res2_out_channels=32), 2, (2, 3, 72, 104), 3),                    # res3 9x13, res4 5x7, res5 3x4
    "wide": (dict(depth=50, out_features=("res2", "res3")), 1, (2, 3, 128, 256), 19),                             # res3: Winograd at 1024 pixels
}


def make_net(name):
    """(module on the CPU, freeze_at, input image): the same weights for every caller (seeded)"""
    from afigan_amd import resnet_guide
    kw, freeze_at, shape, seed = NETS[name]
    torch.manual_seed(seed)
    net = randomise_norms(resnet_guide.ResNet(**kw), seed + 100)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed + 200))
    return net, freeze_at, x


def counts_of(name):
    kw = NETS[name][0]
    outs = kw.get("out_features", ("res2", "res3", "res4", "res5"))
    return BLOCKS[kw["depth"]][:max(int(o[3:]) for o in outs) - 1], list(outs)


def trainable_keys(sd, freeze_at):
    return [k for k in sd if k.endswith(".weight") and ".norm." not in k and k.startswith("res") and int(k[3]) > freeze_at]


@functools.lru_cache(maxsize=None)
def cotangents(name):
    net, freeze_at, x = make_net(name)
    with torch.no_grad():
        counts, outs = counts_of(name)
        sd = {k: v.double() for k, v in net.state_dict().items()}
        feats = resnet(x.double(), sd, counts, outs)
    g = torch.Generator().manual_seed(NETS[name][3] + 300)
    return {k: torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in feats.items()}


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """(outputs, weight gradients) of sum_k <feature_k, cotangent_k> in `dtype` on the CPU; callers must not modify them"""
    net, freeze_at, x = make_net(name)
    counts, outs = counts_of(name)
    sd = {k: v.to(dtype) for k, v in net.state_dict().items()}
    keys = trainable_keys(sd, freeze_at)
    for k in keys:
        sd[k].requires_grad_(True)
    feats = resnet(x.to(dtype), sd, counts, outs)
    cot = cotangents(name)
    sum((feats[k] * cot[k].to(dtype)).sum() for k in feats).backward()
    return {k: v.detach() for k, v in feats.items()}, {k: sd[k].grad for k in keys}


@functools.lru_cache(maxsize=None)
def margins(name):
    """[(unit name, min |pre| / (2^-24 mag), fraction of ones)] over the ReLU units of the trainable blocks, fp64"""
    net, freeze_at, x = make_net(name)
    counts, outs = counts_of(name)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    trace = []
    with torch.no_grad():
        resnet(x.double(), sd, counts, outs, trace_from=freeze_at, trace=trace)
    return [(n, (pre.abs() / (EPS * mag)).min().item(), (pre > 0).double().mean().item()) for n, pre, mag in trace]


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()
