"""CPU-side checks of what the frozen networks share (afigan_amd/frozen.py): the cache of prepared weights -- the same object while no keyed
tensor changes, rebuilt after every way a weight can change (in place, a load, a rebound ``.data``, a dtype round trip) and then equal to a
fresh module's --, fold_conv through a norm that is not the conv's child, and that no module reaches into resnet_guide's private names."""
import ast
import os

import pytest
import torch

import afigan_amd as amd
from afigan_amd import frozen, resnet_guide
from afigan_amd.fpn_sr import ShapeSpec


class _TwoStages(torch.nn.Module):
    """What resnet_guide.FPN reads of its bottom-up."""

    def output_shape(self):
        return {"res2": ShapeSpec(channels=8, stride=4), "res3": ShapeSpec(channels=16, stride=8)}


def _resnet():
    return resnet_guide.ResNet(depth=50, out_features=["res2"])


def _fpn_avg():
    return resnet_guide.FPN(_TwoStages(), ["res2", "res3"], out_channels=8, fuse_type="avg")


def _rpn():
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[32], [64]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]}, "RPN": {"IN_FEATURES": ["p2", "p3"],
                                                                                                                 "PRE_NMS_TOPK_TEST": 1000}})
    return amd.RPN(cfg, {"p2": ShapeSpec(channels=8, stride=4), "p3": ShapeSpec(channels=8, stride=8)})


def _roi_heads():
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": False, "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": ["p2"], "NUM_CLASSES": 3},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "FC_DIM": 8, "POOLER_RESOLUTION": 2}})
    return amd.build_roi_heads(cfg, {"p2": ShapeSpec(channels=4, stride=4)})


# maker, the keyed parameter the single-tensor changes touch (the FPN's: a lateral whose "avg" half-scale form is prepared as well)
MODULES = {"ResNet": (_resnet, lambda m: m.stem.conv1.weight), "FPN-avg": (_fpn_avg, lambda m: m.lateral_convs[1].weight),
           "RPN": (_rpn, lambda m: m.rpn_head.conv.weight), "StandardROIHeads": (_roi_heads, lambda m: m.box_head.fc1.weight)}


def _add_in_place(m, p):
    p.add_(1.0)


def _load_perturbed(m, p):
    m.load_state_dict({k: v + 1.0 for k, v in m.state_dict().items()}, strict=True)


def _rebind_data(m, p):
    version = p._version
    p.data = p.data.clone().add_(1.0)
    assert p._version == version                # the case a key of versions alone misses


def _double_float(m, p):
    held = [t.data for t in m.state_dict().values()]             # (alive across the round trip: the allocator cannot hand a freed address out again)
    m.double().float()
    assert all(t.dtype == torch.float32 and t.data_ptr() != h.data_ptr() for t, h in zip(m.state_dict().values(), held))


CHANGES = {"add_": _add_in_place, "load_state_dict": _load_perturbed, "rebound .data": _rebind_data, ".double().float()": _double_float}


def _flat(o):
    if torch.is_tensor(o):
        return [o]
    return [t for v in (o.values() if isinstance(o, dict) else o) for t in _flat(v)]


def _same(a, b):
    a, b = _flat(a), _flat(b)
    return len(a) == len(b) and all(x.dtype == y.dtype and x.stride() == y.stride() and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(MODULES))
def test_prepare_twice_returns_the_same_object(name):
    m = MODULES[name][0]()
    with torch.no_grad():
        assert m._prepare() is m._prepare()


@pytest.mark.parametrize("change", list(CHANGES))
@pytest.mark.parametrize("name", list(MODULES))
def test_prepared_weights_are_rebuilt_after_a_change(name, change):
    make, param = MODULES[name]
    torch.manual_seed(0)
    m = make()
    with torch.no_grad():
        before = m._prepare()
        kept = [t.clone() for t in _flat(before)]
        CHANGES[change](m, param(m))
        after = m._prepare()
        assert after is not before and m._prepare() is after
        fresh = make()
        fresh.load_state_dict(m.state_dict(), strict=True)
        assert _same(after, fresh._prepare())
        changed = any(not torch.equal(a, b) for a, b in zip(_flat(after), kept))
        assert changed == (change != ".double().float()")           # (a dtype round trip of fp32 values changes storage, not values)


class _BottomUp3(torch.nn.Module):
    _out_feature_strides = {"stage3": 8, "stage4": 16, "stage5": 32}
    _out_feature_channels = {"stage3": 8, "stage4": 12, "stage5": 16}


def _bifpn():
    return amd.BiFPN_AFIGAN(_BottomUp3(), ["stage3", "stage4", "stage5"], 8, 7, norm="BN", top_block=amd.LastLevelP6P7(16, 8, "BN")).eval()


def test_bifpn_refolds_after_a_parameters_data_is_rebound():
    """BiFPN_AFIGAN._prepare is pure torch, so it runs here.  Its key used to hold versions and the device only: a rebound ``.data`` (same
    version count, other storage) left the folded weights stale."""
    torch.manual_seed(0)
    net = _bifpn()
    with torch.no_grad():
        before = net._prepare()
        assert net._prepare() is before
        w_before = before["lateral3"][0].clone()
        _rebind_data(net, net.before_bifpn.lateral3[0].weight)
        after = net._prepare()
        assert after is not before and not torch.equal(after["lateral3"][0], w_before)
        fresh = _bifpn()
        fresh.load_state_dict(net.state_dict(), strict=True)
        assert _same(after, fresh._prepare())


@pytest.mark.parametrize("k,bias,scale", [(1, False, 1.0), (3, False, 1.0), (3, True, 0.5), (7, False, 1.0)])
def test_fold_conv_through_a_norm_that_is_not_a_child(k, bias, scale):
    g = torch.Generator().manual_seed(k)
    own = frozen.Conv2d(8, 16, k, bias=bias)                       # the norm is its child
    bare = frozen.Conv2d(8, 16, k, bias=bias, norm=False)
    beside = frozen.FrozenBatchNorm2d(16)
    with torch.no_grad():
        for t in (own.norm.weight, own.norm.bias, own.norm.running_mean):
            t.copy_(torch.randn(t.shape, generator=g))
        own.norm.running_var.copy_(torch.rand(16, generator=g) + 0.5)
        if bias:
            own.bias.copy_(torch.randn(16, generator=g))
        bare.load_state_dict({n: v for n, v in own.state_dict().items() if not n.startswith("norm.")}, strict=True)
        beside.load_state_dict(own.norm.state_dict(), strict=True)
        assert bare.norm is None and _same(frozen.fold_conv(bare, beside, scale), own.fold(scale))
        assert not _same(frozen.fold_conv(bare), own.fold(scale))   # (the norm does something)
    assert resnet_guide.Conv2d is frozen.Conv2d and resnet_guide.FrozenBatchNorm2d is frozen.FrozenBatchNorm2d


def test_no_module_imports_a_private_name_of_resnet_guide():
    pkg = os.path.dirname(amd.__file__)
    found = []
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py") or fn == "resnet_guide.py":
            continue
        for node in ast.walk(ast.parse(open(os.path.join(pkg, fn)).read(), fn)):
            if isinstance(node, ast.ImportFrom) and (node.module or "").split(".")[-1] == "resnet_guide":
                found += [f"{fn}: from resnet_guide import {a.name}" for a in node.names if a.name.startswith("_")]
            if isinstance(node, ast.Attribute) and node.attr.startswith("_") and isinstance(node.value, ast.Name) and node.value.id == "resnet_guide":
                found.append(f"{fn}: resnet_guide.{node.attr}")
    assert not found, found
