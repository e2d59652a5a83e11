"""The frozen ResNeSt bottom-up (afigan_amd/resnest_backbone.py) on the host: detectron2-ResNeSt's parameter tree, key names and shapes for
R-50 / R-101, its per-stage freezing, loading a model-zoo style checkpoint into the guide built from it, the builders with detectron2
absent, and the options it refuses.  No GPU work: the models are built on the CPU and never run.  The configs restate the values of the
reference's ResNeSt101 inference yamls (RESNETS.DEPTH 101, STRIDE_IN_1X1 False, RADIX 2, NORM SyncBN)."""
import pickle

import pytest
import torch
import torch.nn as nn

import afigan_amd as amd
from afigan_amd import checkpoint, registry, resnest_backbone, resnet_guide

IN_FEATURES = ["res2", "res3", "res4", "res5"]
HEAD_KEYS = {"proposal_generator.rpn_head.conv.weight": (256, 256, 3, 3), "roi_heads.box_predictor.cls_score.weight": (81, 1024)}


def _cfg(depth=101, norm="SyncBN", guide=True, **resnets):
    cfg = amd.get_cfg()
    r = {"DEPTH": depth, "OUT_FEATURES": list(IN_FEATURES), "RADIX": 2, "STRIDE_IN_1X1": False, "NORM": norm}
    r.update(resnets)
    m = {"RESNETS": r, "FPN": {"IN_FEATURES": list(IN_FEATURES)}}
    if guide:
        m.update({"GUIDE_ARCHITECTURE": "RCNN_FPN_only", "GUIDE_BACKBONE": {"NAME": "build_resnest_fpn_backbone"}})
    cfg.merge_from_dict({"MODEL": m})
    cfg.MODEL.DEVICE = "cpu"
    return cfg


@pytest.fixture
def restore_bottom_up():
    old = dict(registry._BOTTOM_UP)
    yield
    registry._BOTTOM_UP.clear()
    registry._BOTTOM_UP.update(old)


@pytest.mark.parametrize("depth", [50, 101])
def test_parameter_tree_and_shapes(depth):
    if registry.USING_DETECTRON2_REGISTRY:
        pytest.skip("with detectron2 installed the name is detectron2-ResNeSt's")
    assert amd.BACKBONE_REGISTRY.get("build_resnest_fpn_backbone") is resnest_backbone.build_resnest_fpn_backbone
    m = amd.build_guide_model(_cfg(depth))
    assert isinstance(m.backbone, resnet_guide.FPN) and isinstance(m.backbone.bottom_up, resnest_backbone.ResNeSt)
    sd = {k[len("backbone.bottom_up."):]: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("backbone.bottom_up.")}
    sw = {50: 32, 101: 64}[depth]
    expect = {"stem.conv1_1.weight": (sw, 3, 3, 3), "stem.conv1_2.weight": (sw, sw, 3, 3), "stem.conv1_3.weight": (2 * sw, sw, 3, 3),
              "stem.conv1_3.norm.running_var": (2 * sw,),
              "res2.0.conv1.weight": (64, 2 * sw, 1, 1), "res2.0.conv2.conv.weight": (128, 32, 3, 3), "res2.0.conv2.bn0.weight": (128,),
              "res2.0.conv2.fc1.weight": (32, 64, 1, 1), "res2.0.conv2.fc1.bias": (32,), "res2.0.conv2.bn1.running_mean": (32,),
              "res2.0.conv2.fc2.weight": (128, 32, 1, 1), "res2.0.conv2.fc2.bias": (128,), "res2.0.conv3.weight": (256, 64, 1, 1),
              "res2.0.shortcut.weight": (256, 2 * sw, 1, 1), "res3.0.conv2.conv.weight": (256, 64, 3, 3),
              "res3.0.conv2.fc1.weight": (64, 128, 1, 1), "res3.0.shortcut.weight": (512, 256, 1, 1),
              "res4.0.conv2.fc2.weight": (512, 128, 1, 1), "res5.2.conv2.fc1.weight": (256, 512, 1, 1),
              "res5.2.conv2.conv.weight": (1024, 256, 3, 3), "res5.0.shortcut.weight": (2048, 1024, 1, 1)}
    if depth == 101:
        expect["res4.22.conv2.fc1.weight"] = (128, 256, 1, 1)
    for k, s in expect.items():
        assert sd.get(k) == s, (k, sd.get(k), s)
    last = {50: 5, 101: 22}[depth]
    assert f"res4.{last}.conv3.weight" in sd and f"res4.{last + 1}.conv3.weight" not in sd
    assert "res2.1.shortcut.weight" not in sd and "stem.conv1.weight" not in sd
    assert not any(".avd_layer" in k or "shortcut_avgpool" in k for k in sd)         # the pools have no parameters
    for k in range(2, 6):
        assert f"backbone.fpn_lateral{k}.bias" in m.state_dict() and f"backbone.fpn_output{k}.weight" in m.state_dict()
    bu = m.backbone.bottom_up
    assert {k: (s.channels, s.stride) for k, s in bu.output_shape().items()} == {"res2": (256, 4), "res3": (512, 8), "res4": (1024, 16),
                                                                                 "res5": (2048, 32)}
    assert m.backbone.size_divisibility == 32
    assert not any(p.requires_grad for p in m.parameters())
    assert [b.avd for b in bu.res3] == [True, False, False, False] and not any(b.avd for b in bu.res2)


def test_freeze_at_makes_stem_and_res2_frozen_bn():
    """FREEZE_AT 2 with NORM SyncBN: FrozenBatchNorm2d (no num_batches_tracked) in the stem and res2, the config's norm after."""
    m = amd.build_guide_model(_cfg(101, "SyncBN"))
    sd = m.state_dict()
    norms = {k.rsplit(".", 1)[0] for k in sd if k.startswith("backbone.bottom_up.") and k.endswith("running_mean")}
    assert len(norms) == 3 + 4 * (3 + 4 + 23 + 3) + 4                      # stem, 4 per block (conv1, bn0, bn1, conv3), a shortcut per stage
    for n in norms:
        frozen = ".stem." in n or ".res2." in n
        assert (n + ".num_batches_tracked" in sd) != frozen, n
    bu = m.backbone.bottom_up
    assert isinstance(bu.stem.conv1_1.norm, resnet_guide.FrozenBatchNorm2d) and isinstance(bu.res2[2].conv2.bn1, resnet_guide.FrozenBatchNorm2d)
    assert isinstance(bu.res3[0].conv2.bn0, nn.SyncBatchNorm) and isinstance(bu.res5[2].conv3.norm, nn.SyncBatchNorm)
    cfg = _cfg(50, "BN")
    cfg.MODEL.BACKBONE.FREEZE_AT = 3
    bu = amd.build_guide_model(cfg).backbone.bottom_up
    assert isinstance(bu.res3[3].conv1.norm, resnet_guide.FrozenBatchNorm2d)
    assert type(bu.res4[0].conv1.norm) is nn.BatchNorm2d
    cfg.MODEL.BACKBONE.FREEZE_AT = 0
    bu = amd.build_guide_model(cfg).backbone.bottom_up
    assert type(bu.stem.conv1_1.norm) is nn.BatchNorm2d


def test_model_zoo_pkl_loads_with_no_missing_keys(tmp_path):
    m = amd.build_guide_model(_cfg(101))
    gen = torch.Generator().manual_seed(0)
    sd = {k: (torch.randn(tuple(v.shape), generator=gen) if v.is_floating_point() else torch.full(tuple(v.shape), 7)).numpy()
          for k, v in m.state_dict().items()}
    for k, s in HEAD_KEYS.items():
        sd[k] = torch.randn(s, generator=gen).numpy()
    p = tmp_path / "model_final.pkl"
    with open(p, "wb") as f:
        pickle.dump({"model": sd, "__author__": "ResNeSt model zoo"}, f)
    missing, unused = checkpoint.load_guide_weights(m, str(p))
    assert missing == [] and unused == sorted(HEAD_KEYS)
    got = m.state_dict()
    for k in ("backbone.bottom_up.res4.22.conv2.fc1.weight", "backbone.bottom_up.stem.conv1_2.norm.running_var",
              "backbone.bottom_up.res3.0.conv2.bn1.num_batches_tracked", "backbone.fpn_output3.bias"):
        assert torch.equal(got[k], torch.as_tensor(sd[k])), k


def test_splat_fold_uses_its_own_norms():
    """bn0 is folded into the grouped conv, bn1 into fc1 (whose bias passes through it); fc2 keeps its bias."""
    sp = resnest_backbone.SplAtConv2d(64, "BN")
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for t in (sp.bn0.weight, sp.bn0.bias, sp.bn0.running_mean, sp.bn1.weight, sp.bn1.bias, sp.bn1.running_mean, sp.fc1.bias, sp.fc2.bias):
            t.copy_(torch.randn(t.shape, generator=g))
        sp.bn0.running_var.copy_(torch.rand(128, generator=g) + 0.5)
        sp.bn1.running_var.copy_(torch.rand(32, generator=g) + 0.5)
    (wc, bc), (w1, b1), (w2, b2) = sp.fold()
    s0 = sp.bn0.weight.double() / (sp.bn0.running_var.double() + 1e-5).sqrt()
    assert torch.allclose(wc.double(), sp.conv.weight.double() * s0.view(-1, 1, 1, 1), rtol=1e-6, atol=0)
    assert torch.allclose(bc.double(), sp.bn0.bias.double() - sp.bn0.running_mean.double() * s0, rtol=1e-6, atol=1e-7)
    s1 = sp.bn1.weight.double() / (sp.bn1.running_var.double() + 1e-5).sqrt()
    assert torch.allclose(w1.double(), sp.fc1.weight.double().view(32, 64) * s1.view(-1, 1), rtol=1e-6, atol=0)
    assert torch.allclose(b1.double(), (sp.fc1.bias.double() - sp.bn1.running_mean.double()) * s1 + sp.bn1.bias.double(), rtol=1e-6,
                          atol=1e-6)
    assert torch.equal(w2, sp.fc2.weight.view(128, 32)) and torch.equal(b2, sp.fc2.bias)
    assert wc.permute(0, 2, 3, 1).is_contiguous() and tuple(wc.shape) == (128, 32, 3, 3)


@pytest.mark.parametrize("section,key,value", [("RESNETS", "RADIX", 1), ("RESNETS", "RADIX", 4), ("RESNETS", "NUM_GROUPS", 2),
                                               ("RESNETS", "RES5_DILATION", 2), ("RESNETS", "DEFORM_ON_PER_STAGE", [False, True, True, True]),
                                               ("RESNETS", "NORM", "GN"), ("RESNETS", "NORM", ""), ("RESNETS", "DEPTH", 152),
                                               ("RESNETS", "DEPTH", 34), ("FPN", "NORM", "SyncBN"), ("RESNETS", "OUT_FEATURES", ["res6"])])
def test_unsupported_options_raise(section, key, value):
    cfg = _cfg()
    setattr(getattr(cfg.MODEL, section), key, value)
    with pytest.raises(amd.AfiError):
        resnest_backbone.build_resnest_fpn_backbone(cfg, None)


def test_stride_in_1x1_is_refused_with_the_reason():
    with pytest.raises(amd.AfiError, match="down-sample it twice"):
        resnest_backbone.build_resnest_backbone(_cfg(STRIDE_IN_1X1=True), None)


def test_forward_refuses_autograd_and_the_cpu():
    bu = resnest_backbone.build_resnest_backbone(_cfg(50), None)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(amd.AfiError, match="forward-only"):
        bu(x.clone().requires_grad_(True))
    bu.res3[0].conv2.fc1.weight.requires_grad_(True)
    with pytest.raises(amd.AfiError, match="forward-only"):
        bu(x)
    bu.res3[0].conv2.fc1.weight.requires_grad_(False)
    with torch.no_grad(), pytest.raises(amd.AfiError, match="GPU only"):
        bu(x)


def test_resnet_guide_still_refuses_radix_2():
    cfg = _cfg(50, "FrozenBN")
    cfg.MODEL.GUIDE_BACKBONE.NAME = "build_resnet_fpn_backbone"
    with pytest.raises(amd.AfiError, match="ResNeSt options"):
        resnet_guide.build_resnet_fpn_backbone(cfg, None)


def test_resnest_bottom_up_is_opt_in(restore_bottom_up):
    registry._BOTTOM_UP.pop("resnest", None)
    try:
        default = registry.bottom_up_builder("resnest")
    except amd.AfiError:
        default = None
    assert default is not resnest_backbone.build_resnest_backbone                 # importing the package does not install it
    cfg = _cfg(101, guide=False)
    cfg.MODEL.BACKBONE.NAME = "build_resnest_pafpn_sr_backbone"
    if default is None:
        with pytest.raises(amd.AfiError, match="resnest"):
            amd.BACKBONE_REGISTRY.get("build_resnest_pafpn_sr_backbone")(cfg, None)
    resnest_backbone.use_as_bottom_up()
    assert registry.bottom_up_builder("resnest") is resnest_backbone.build_resnest_backbone
    for name, cls in (("build_resnest_pafpn_sr_backbone", amd.PAFPN_AFIGAN), ("build_resnest_fpn_sr_backbone", amd.FPN_AFIGAN)):
        bb = amd.BACKBONE_REGISTRY.get(name)(cfg, None)
        assert isinstance(bb, cls) and isinstance(bb.bottom_up, resnest_backbone.ResNeSt)
        assert {k: (s.channels, s.stride) for k, s in bb.output_shape().items()} == {f"p{i}": (256, 2 ** i) for i in range(2, 7)}
        assert "bottom_up.res4.22.conv2.fc2.weight" in bb.state_dict() and "srf_module.Generators.0.0.0.weight" in bb.state_dict()
