"""What the frozen, forward-only networks (resnet_guide, resnest_backbone, swin_backbone, rpn, roi_heads, bifpn_sr's eval path) share: the
frozen conv and its fp64 fold, the 1x1 / 3x3 conv dispatch, the cache of prepared weights, the forward-only / GPU-only checks and the
config lookup.  A new prepared form of a weight is one more `prepared` slot of its module and, if a conv reads it, one more branch here
(so far one: the bf16x6 image of a 1x1 weight, `conv1x1_image`, read by `conv1x1` for the large maps of forward-only callers)."""
import torch
import torch.nn as nn

from . import ops
from ._lib import AfiError

FROZEN_BN_EPS = 1e-5


class FrozenBatchNorm2d(nn.Module):
    """detectron2.layers.FrozenBatchNorm2d: y = (x - running_mean) / sqrt(running_var + eps) * weight + bias, all four buffers."""

    def __init__(self, num_features, eps=FROZEN_BN_EPS):
        super().__init__()
        self.num_features, self.eps = num_features, eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features) - eps)


def fold_conv(conv, norm=None, scale=1.0):
    """(weight, bias) of `conv` with `norm` (its own child or not; any norm with weight / bias / running_mean / running_var / eps) folded in,
    computed in fp64 and rounded once; 3x3 weights in the kernels' [O][kh][kw][I] memory, 1x1 weights as [Cout, Cin].  `scale` multiplies
    the bias (the FPN's "avg" fuse halves it)."""
    w = conv.weight.detach().double()
    b = conv.bias.detach().double() if conv.bias is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
    if norm is not None:
        s = norm.weight.double() * torch.rsqrt(norm.running_var.double() + norm.eps)
        w = w * s.view(-1, 1, 1, 1)
        b = (b - norm.running_mean.double()) * s + norm.bias.double()
    w, b = w.float(), (b * scale).float().contiguous()
    k = conv.kernel_size if isinstance(conv.kernel_size, int) else (conv.kernel_size[0] if len(set(conv.kernel_size)) == 1 else 0)   # nn.Conv2d: a tuple
    if k == 1:
        return w.reshape(w.shape[0], w.shape[1]).contiguous(), b
    if k == 3:
        return ops.to_ohwi(w), b
    return w.contiguous(), b


class Conv2d(nn.Module):
    """detectron2.layers.Conv2d's parameter tree (weight, optional bias, optional norm child); frozen: requires_grad is off."""

    def __init__(self, cin, cout, k, stride=1, bias=False, norm=True):
        super().__init__()
        self.kernel_size, self.stride = k, stride
        w = torch.randn(cout, cin, k, k) * (2.0 / (cout * k * k)) ** 0.5          # c2_msra_fill's scale (fan_out); a checkpoint replaces it
        self.weight = nn.Parameter(w, requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False) if bias else None
        self.norm = FrozenBatchNorm2d(cout) if norm else None

    def fold(self, scale=1.0):
        return fold_conv(self, self.norm, scale)


def conv1x1(x, wb, stride=1, add=None, relu=False, alpha=1.0, add_scale=1.0, owner=None):
    """`owner`: the frozen module the folded (weight, bias) `wb` belongs to, given by forward-only callers: a large map then runs on the
    bf16 matrix cores over the weight's prepared image (conv1x1_image); without it, and for every map the host plan does not route, the
    fp32-MFMA pixel GEMM as before."""
    if stride != 1:
        x = x[:, :, ::stride, ::stride]                                 # (a view: the kernel walks the strides)
    if add is not None and add.shape[-2:] != x.shape[-2:]:
        raise AfiError(f"resnet_guide: addend {tuple(add.shape)} does not match the conv output {tuple(x.shape[-2:])}")
    if owner is not None and ops.conv1x1_frozen_routed(x, wb[0].shape[0], add):
        return ops.conv1x1_frozen_fwd(x, conv1x1_image(owner, wb[0]), wb[1], wb[0].shape[0], add=add, add_scale=add_scale, alpha=alpha,
                                      act=2 if relu else 0)
    return ops.conv1x1_fwd(x, wb[0], wb[1], add=add, add_scale=add_scale, alpha=alpha, act=2 if relu else 0)


def conv1x1_image(module, w, name="image1x1"):
    """The prepared form "1x1 bf16x6 image" of `module`'s folded weight `w` [Cout, Cin]: built by one launch when a parameter or buffer of
    the module -- everything `w` is folded from -- has changed, the same tensor otherwise.  Keyed per conv, so a write to one conv's weight
    rebuilds that conv's image only (the fold of a whole network is one slot and hands out fresh `w` tensors for all of them)."""
    return prepared(module, name, list(module.parameters()) + list(module.buffers()), lambda: ops.conv1x1_frozen_image(w))


def conv3x3(x, wb, stride=1, relu=False):
    act = 2 if relu else 0
    if stride == 2:
        return ops.conv3x3s2_fwd(x, wb[0], wb[1], act=act)
    N, C, H, W = x.shape
    if C >= 128 and wb[0].shape[0] >= 128 and N * H * W >= 1024:      # the Winograd form (F(4x4) tiles on maps of >= 8192 pixels)
        return ops.conv3x3_wino_infer(x, wb[0], wb[1], act=act)
    return ops.conv3x3_fwd(x, wb[0], wb[1], lrelu=act)


def prepared(module, name, tensors, build):
    """`build()`, kept on `module` as ``_<name>`` and rebuilt when one of `tensors` changes (version, storage, device; the key is kept as
    ``_<name>_key``): the one cache of weights in the kernels' form.  Unchanged tensors give the same object back."""
    key = tuple((t._version, t.data_ptr(), str(t.device)) for t in tensors)
    if getattr(module, f"_{name}_key", None) != key:
        setattr(module, f"_{name}", build())
        setattr(module, f"_{name}_key", key)
    return getattr(module, f"_{name}")


def adopt_prepared(module, name, tensors):
    """Re-key the existing ``_<name>`` slot of `module` to the CURRENT versions of `tensors` without rebuilding it: for a caller that has just
    written both sides itself -- the tensors and, consistently, what the slot holds (detector_optim: the update and the refold are one
    kernel).  The slot must exist and have been current before those writes; nothing here can check that."""
    if not hasattr(module, f"_{name}_key"):
        raise AfiError(f"adopt_prepared: {type(module).__name__} has no prepared slot {name!r} to adopt (prepared() builds it first)")
    setattr(module, f"_{name}_key", tuple((t._version, t.data_ptr(), str(t.device)) for t in tensors))


def check_forward_only(module, x, what):
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters())):
        raise AfiError(f"{what} is forward-only (frozen): run it under torch.no_grad() with no parameter or input requiring grad")
    if not x.is_cuda:
        raise AfiError(f"{what} runs on the GPU only (got a CPU tensor); there is no CPU fallback")


def check_feature(where, name, x, runs, only="fp32 only"):
    """An input of a detector head is an fp32 GPU tensor; `runs`: "the ROI heads run", `only`: the words before the reason."""
    if not getattr(x, "is_cuda", False):
        raise AfiError(f"{where}: {name} is a CPU tensor; {runs} on the GPU only, there is no CPU fallback")
    if x.dtype != torch.float32:
        raise AfiError(f"{where}: {name} is {x.dtype}; {only} (2-byte activations stop at the AFI backbone's boundary)")


def cfg_get(node, key, default):
    return getattr(node, key, default) if node is not None else default
