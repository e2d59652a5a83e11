"""The frozen ResNet-FPN guide (afigan_amd/resnet_guide.py) on the host: detectron2's parameter tree and key names, loading a detectron2
model-zoo checkpoint (checkpoint.load_guide_weights), the builder behind ``build_resnet_fpn_backbone`` with detectron2 absent, and the options
it refuses.  No GPU work: the models are built on the CPU and never run."""
import pickle

import pytest
import torch

import afigan_amd as amd
from afigan_amd import checkpoint, registry, resnet_guide

IN_FEATURES = ["res2", "res3", "res4", "res5"]
HEAD_KEYS = {"proposal_generator.rpn_head.conv.weight": (256, 256, 3, 3), "roi_heads.box_predictor.cls_score.weight": (81, 1024),
             "roi_heads.mask_head.predictor.bias": (80,)}


def _step1_cfg(**resnets):
    """get_cfg() with what the step-1 yaml (and its Base-RCNN-FPN base) sets under MODEL that the guide reads, on the CPU."""
    cfg = amd.get_cfg()
    r = {"DEPTH": 50, "OUT_FEATURES": list(IN_FEATURES)}
    r.update(resnets)
    cfg.merge_from_dict({"MODEL": {"GUIDE_ARCHITECTURE": "RCNN_FPN_only", "RESNETS": r, "FPN": {"IN_FEATURES": list(IN_FEATURES)}}})
    cfg.MODEL.DEVICE = "cpu"
    return cfg


def _zoo_file(tmp_path, model, extra=None, drop=(), reshape=None):
    """A detectron2 model-zoo style .pkl: {"model": {name: numpy array}, "__author__": ...}, the guide's keys plus detector-head keys."""
    gen = torch.Generator().manual_seed(0)
    sd = {}
    for k, v in model.state_dict().items():
        if k in drop:
            continue
        shape = reshape.get(k, v.shape) if reshape else v.shape
        sd[k] = torch.randn(tuple(shape), generator=gen).numpy()
    for k, s in (extra if extra is not None else HEAD_KEYS).items():
        sd[k] = torch.randn(s, generator=gen).numpy()
    p = tmp_path / "model_final.pkl"
    with open(p, "wb") as f:
        pickle.dump({"model": sd, "__author__": "Detectron2 Model Zoo"}, f)
    return p, sd


def test_builder_is_registered_and_builds_from_the_step1_config():
    if registry.USING_DETECTRON2_REGISTRY:
        pytest.skip("with detectron2 installed the name is detectron2's")
    assert amd.BACKBONE_REGISTRY.get("build_resnet_fpn_backbone") is resnet_guide.build_resnet_fpn_backbone
    cfg = _step1_cfg()
    assert cfg.MODEL.GUIDE_BACKBONE.NAME == "build_resnet_fpn_backbone"
    m = amd.build_guide_model(cfg)
    assert isinstance(m, amd.RCNN_FPN_only) and isinstance(m.backbone, resnet_guide.FPN)
    bb = m.backbone
    assert bb.size_divisibility == 32
    assert {k: (s.channels, s.stride) for k, s in bb.output_shape().items()} == {f"p{i}": (256, 2 ** i) for i in range(2, 7)}
    sd = m.state_dict()
    assert "backbone.bottom_up.stem.conv1.weight" in sd and tuple(sd["backbone.bottom_up.stem.conv1.weight"].shape) == (64, 3, 7, 7)
    for k in ("weight", "bias", "running_mean", "running_var"):
        assert f"backbone.bottom_up.stem.conv1.norm.{k}" in sd
        assert f"backbone.bottom_up.res5.2.conv3.norm.{k}" in sd
    assert "backbone.bottom_up.res2.0.shortcut.weight" in sd and "backbone.bottom_up.res2.1.shortcut.weight" not in sd
    assert tuple(sd["backbone.bottom_up.res3.0.conv1.weight"].shape) == (128, 256, 1, 1)
    assert tuple(sd["backbone.bottom_up.res5.0.shortcut.weight"].shape) == (2048, 1024, 1, 1)
    assert "backbone.bottom_up.res4.5.conv2.weight" in sd and "backbone.bottom_up.res4.6.conv2.weight" not in sd
    for k in range(2, 6):
        assert f"backbone.fpn_lateral{k}.bias" in sd and f"backbone.fpn_output{k}.weight" in sd
    assert not any(p.requires_grad for p in m.parameters())           # frozen
    # STRIDE_IN_1X1 says where a block's stride sits; R-101 has 23 blocks in res4
    assert m.backbone.bottom_up.res3[0].conv1.stride == 2 and m.backbone.bottom_up.res3[0].conv2.stride == 1
    m2 = amd.build_guide_model(_step1_cfg(DEPTH=101, STRIDE_IN_1X1=False))
    assert m2.backbone.bottom_up.res3[0].conv1.stride == 1 and m2.backbone.bottom_up.res3[0].conv2.stride == 2
    assert "backbone.bottom_up.res4.22.conv3.weight" in m2.state_dict() and "backbone.bottom_up.res4.23.conv3.weight" not in m2.state_dict()


def test_model_zoo_pkl_loads_with_no_missing_backbone_keys(tmp_path):
    m = amd.build_guide_model(_step1_cfg())
    p, sd = _zoo_file(tmp_path, m)
    missing, unused = checkpoint.load_guide_weights(m, str(p))
    assert missing == [] and unused == sorted(HEAD_KEYS)
    got = m.state_dict()
    for k in ("backbone.bottom_up.res4.3.conv2.weight", "backbone.bottom_up.stem.conv1.norm.running_var", "backbone.fpn_output3.bias"):
        assert torch.equal(got[k], torch.as_tensor(sd[k])), k
    # a .pth ({"model": tensors}) reads the same way; a key the file lacks is reported, not invented
    sd2 = {k: torch.as_tensor(v) for k, v in sd.items() if k != "backbone.fpn_lateral4.weight"}
    torch.save({"model": sd2}, tmp_path / "guide.pth")
    missing, unused = checkpoint.load_guide_weights(m, str(tmp_path / "guide.pth"))
    assert missing == ["backbone.fpn_lateral4.weight"] and unused == sorted(HEAD_KEYS)


def test_folding_follows_the_buffers():
    """FrozenBN folded into the conv in fp64: w * gamma / sqrt(var + 1e-5), (b - mean) * that + beta; rebuilt after a load changes a buffer."""
    conv = resnet_guide.Conv2d(8, 16, 3)
    g = torch.Generator().manual_seed(1)
    for t in (conv.norm.weight, conv.norm.bias, conv.norm.running_mean):
        t.copy_(torch.randn(t.shape, generator=g))
    conv.norm.running_var.copy_(torch.rand(16, generator=g) + 0.5)
    w, b = conv.fold()
    s = conv.norm.weight.double() / (conv.norm.running_var.double() + 1e-5).sqrt()
    assert torch.allclose(w.double(), conv.weight.double() * s.view(-1, 1, 1, 1), rtol=1e-7, atol=0)
    assert torch.allclose(b.double(), conv.norm.bias.double() - conv.norm.running_mean.double() * s, rtol=1e-6, atol=1e-7)
    assert w.permute(0, 2, 3, 1).is_contiguous()                          # the kernels' [O][kh][kw][I] memory

    class _One(resnet_guide._Frozen):
        def __init__(self):
            super().__init__()
            self.c = conv

        def _own_convs(self):
            return [self.c]
    one = _One()
    f1 = one._prepare()
    assert one._prepare() is f1                                          # unchanged: not refolded
    conv.norm.running_var.mul_(2.0)
    f2 = one._prepare()
    assert f2 is not f1 and not torch.equal(f2[id(conv)][0], f1[id(conv)][0])


def test_wrong_shape_and_caffe2_names_are_refused(tmp_path):
    m = amd.build_guide_model(_step1_cfg())
    p, _ = _zoo_file(tmp_path, m, reshape={"backbone.bottom_up.res3.1.conv2.weight": (128, 128, 1, 1)})
    with pytest.raises(ValueError, match="res3.1.conv2.weight"):
        checkpoint.load_guide_weights(m, str(p))
    c2 = tmp_path / "R-50.pkl"
    with open(c2, "wb") as f:
        pickle.dump({"blobs": {"conv1_w": torch.zeros(64, 3, 7, 7).numpy(), "res2_0_branch1_w": torch.zeros(256, 64, 1, 1).numpy(),
                               "res_conv1_bn_s": torch.ones(64).numpy()}}, f)
    with pytest.raises(ValueError, match="Caffe2"):
        checkpoint.load_guide_weights(m, str(c2))
    with open(c2, "wb") as f:
        pickle.dump({"model": {"res2_0_branch2a_w": torch.zeros(64, 64, 1, 1).numpy()}, "__author__": "Caffe2"}, f)
    with pytest.raises(ValueError, match="Caffe2"):
        checkpoint.load_guide_weights(m, str(c2))


@pytest.mark.parametrize("section,key,value", [("RESNETS", "DEPTH", 34), ("RESNETS", "DEPTH", 152), ("RESNETS", "NUM_GROUPS", 32),
                                               ("RESNETS", "RES5_DILATION", 2), ("RESNETS", "DEFORM_ON_PER_STAGE", [False, True, True, True]),
                                               ("RESNETS", "NORM", "BN"), ("RESNETS", "NORM", "GN"), ("RESNETS", "STEM_OUT_CHANNELS", 32),
                                               ("RESNETS", "RADIX", 2), ("RESNETS", "DEEP_STEM", True), ("FPN", "NORM", "GN"),
                                               ("FPN", "FUSE_TYPE", "max"), ("RESNETS", "OUT_FEATURES", ["res3", "res4", "res5"])])
def test_unsupported_options_raise(section, key, value):
    cfg = _step1_cfg()
    setattr(getattr(cfg.MODEL, section), key, value)
    with pytest.raises(amd.AfiError):
        resnet_guide.build_resnet_fpn_backbone(cfg, None)


def test_forward_refuses_autograd_and_the_cpu():
    m = resnet_guide.build_resnet_fpn_backbone(_step1_cfg(), None)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(amd.AfiError, match="forward-only"):
        m(x.clone().requires_grad_(True))
    m.fpn_output2.weight.requires_grad_(True)
    with pytest.raises(amd.AfiError, match="forward-only"):
        m(x)
    m.fpn_output2.weight.requires_grad_(False)
    with torch.no_grad(), pytest.raises(amd.AfiError, match="GPU only"):
        m(x)


def test_resnet_bottom_up_builder_is_opt_in():
    old = dict(registry._BOTTOM_UP)
    try:
        registry._BOTTOM_UP.pop("resnet", None)
        try:
            default = registry.bottom_up_builder("resnet")
        except amd.AfiError:
            default = None
        assert default is not resnet_guide.build_resnet_backbone            # importing the package does not install it
        resnet_guide.use_as_bottom_up()
        assert registry.bottom_up_builder("resnet") is resnet_guide.build_resnet_backbone
        bu = registry.bottom_up_builder("resnet")(_step1_cfg(), None)
        assert isinstance(bu, resnet_guide.ResNet)
        assert {k: (s.channels, s.stride) for k, s in bu.output_shape().items()} == {"res2": (256, 4), "res3": (512, 8), "res4": (1024, 16),
                                                                                     "res5": (2048, 32)}
    finally:
        registry._BOTTOM_UP.clear()
        registry._BOTTOM_UP.update(old)
