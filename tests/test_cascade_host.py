"""CPU-side checks of the frozen CascadeROIHeads (afigan_amd/roi_heads.py): detectron2's key names, shapes and counts for the reference's
Cascade configs and a strict load of nn.SyncBatchNorm-normed modules' state, the norm fold and its cache, the config defaults and the three
Cascade yamls' sections, every refusal by its message, tests/cascade_f64.py -- the fp64 yardstick of test_gpu_cascade.py -- against restatements
written differently, afi_roi_cascade_stage's argument checks, and the GPU tests' seeded inputs held to the conditions those tests assert."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import afigan_amd as amd
from afigan_amd.fpn_sr import ShapeSpec

import cascade_f64 as Q
import roi_f64 as QB

S101 = {"MASK_ON": True, "ROI_HEADS": {"NAME": "CascadeROIHeads", "IN_FEATURES": ["p2", "p3", "p4", "p5"]},
        "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 1, "NUM_CONV": 4, "NORM": "SyncBN", "POOLER_RESOLUTION": 7, "CLS_AGNOSTIC_BBOX_REG": True},
        "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": 4, "NORM": "SyncBN", "POOLER_RESOLUTION": 14}}
SWIN = dict(S101, MASK_ON=False, ROI_HEADS={"NAME": "CascadeROIHeads", "IN_FEATURES": ["p3", "p4", "p5", "p6"]})
SMALL = {"MASK_ON": True, "ROI_HEADS": {"NAME": "CascadeROIHeads", "IN_FEATURES": ["p2"], "NUM_CLASSES": 3},
         "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 1, "FC_DIM": 8, "NUM_CONV": 2, "CONV_DIM": 8, "NORM": "SyncBN", "POOLER_RESOLUTION": 3,
                          "CLS_AGNOSTIC_BBOX_REG": True},
         "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": 1, "CONV_DIM": 8, "NORM": "SyncBN", "POOLER_RESOLUTION": 4}}


def _cfg(base=S101, model=None):
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict(base)
    for sec, d in (model or {}).items():
        if isinstance(d, dict):
            getattr(cfg.MODEL, sec).merge_from_dict(d)
        else:
            setattr(cfg.MODEL, sec, d)
    return cfg


def _shapes(channels=256, names=("p2", "p3", "p4", "p5", "p6", "p7")):
    return {f: ShapeSpec(channels=channels, stride=2 ** int(f[1:])) for f in names}


def _small(model=None, channels=8):
    return amd.build_roi_heads(_cfg(SMALL, model), _shapes(channels), masks=True, cascade=True)


# ------------------------------------------------------------------------------------------------ keys, shapes, counts
NORM_SHAPES = {"weight": (256,), "bias": (256,), "running_mean": (256,), "running_var": (256,), "num_batches_tracked": ()}


def test_key_names_shapes_and_counts_of_the_reference_heads():
    h = amd.build_roi_heads(_cfg(), _shapes(), masks=True, cascade=True)
    assert isinstance(h, amd.CascadeROIHeads) and isinstance(h, amd.StandardROIHeads) and amd.ROI_HEADS_REGISTRY.get("CascadeROIHeads") is amd.CascadeROIHeads
    want = {}
    for k in range(3):
        for i in range(1, 5):
            want[f"box_head.{k}.conv{i}.weight"] = (256, 256, 3, 3)
            want.update({f"box_head.{k}.conv{i}.norm.{n}": s for n, s in NORM_SHAPES.items()})
        want.update({f"box_head.{k}.fc1.weight": (1024, 256 * 49), f"box_head.{k}.fc1.bias": (1024,),
                     f"box_predictor.{k}.cls_score.weight": (81, 1024), f"box_predictor.{k}.cls_score.bias": (81,),
                     f"box_predictor.{k}.bbox_pred.weight": (4, 1024), f"box_predictor.{k}.bbox_pred.bias": (4,)})
    for i in range(1, 5):
        want[f"mask_head.mask_fcn{i}.weight"] = (256, 256, 3, 3)
        want.update({f"mask_head.mask_fcn{i}.norm.{n}": s for n, s in NORM_SHAPES.items()})
    want.update({"mask_head.deconv.weight": (256, 256, 2, 2), "mask_head.deconv.bias": (256,), "mask_head.predictor.weight": (80, 256, 1, 1),
                 "mask_head.predictor.bias": (80,)})
    assert {k: tuple(v.shape) for k, v in h.state_dict().items()} == want and len(want) == 3 * 30 + 28
    assert all(not p.requires_grad for p in h.parameters()) and len(list(h.parameters())) == 3 * (4 + 2 + 4) + 4 + 4
    assert h.num_stages == 3 and h.stage_weights == ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))
    assert (h.box_pooler.min_level, h.box_pooler.max_level, h.box_pooler.output_size) == (2, 5, 7) and h.mask_pooler.output_size == 14 and h.mask_on
    assert h.num_classes == 80 and all(p.cls_agnostic_bbox_reg for p in h.box_predictor)
    # detectron2's initialisation: msra convs, c2_xavier FCs, std 0.01 / 0.001 predictors, zero biases, unit norms
    assert 0.7 < float(h.box_head[1].conv2.weight.std()) / math.sqrt(2.0 / (256 * 9)) < 1.3
    assert 0.7 < float(h.box_head[2].fc1.weight.std()) / math.sqrt(1.0 / (256 * 49)) < 1.3
    assert 0.005 < float(h.box_predictor[0].cls_score.weight.std()) < 0.02 and 0.0005 < float(h.box_predictor[2].bbox_pred.weight.std()) < 0.002
    assert not any(v.any() for k, v in h.state_dict().items() if k.endswith(".bias"))
    n = h.box_head[0].conv1.norm
    assert bool((n.weight == 1).all()) and bool((n.running_var == 1).all()) and not n.running_mean.any() and n.eps == 1e-5
    assert h.box_head[0].conv1.bias is None and h.mask_head.mask_fcn1.bias is None


def test_swin_config_heads():
    h = amd.build_roi_heads(_cfg(SWIN), _shapes(names=("p3", "p4", "p5", "p6", "p7")), cascade=True)
    assert not h.mask_on and not hasattr(h, "mask_head") and h.in_features == ["p3", "p4", "p5", "p6"]
    assert (h.box_pooler.min_level, h.box_pooler.max_level) == (3, 6)
    assert len(h.state_dict()) == 90 and {k.split(".")[0] for k in h.state_dict()} == {"box_head", "box_predictor"}
    direct = amd.CascadeROIHeads(_cfg(SWIN), _shapes())
    assert set(direct.state_dict()) == set(h.state_dict())


def test_norm_variants_and_bias():
    for norm, tracked in (("BN", True), ("SyncBN", True), ("FrozenBN", False)):
        sd = _small({"ROI_BOX_HEAD": {"NORM": norm}, "ROI_MASK_HEAD": {"NORM": norm}}).state_dict()
        assert ("box_head.0.conv1.norm.num_batches_tracked" in sd) == tracked and ("mask_head.mask_fcn1.norm.num_batches_tracked" in sd) == tracked
        assert "box_head.0.conv1.bias" not in sd and "mask_head.mask_fcn1.bias" not in sd and "box_head.0.conv1.norm.running_var" in sd
    sd = _small({"ROI_BOX_HEAD": {"NORM": ""}, "ROI_MASK_HEAD": {"NORM": ""}}).state_dict()
    assert "box_head.0.conv1.bias" in sd and "mask_head.mask_fcn1.bias" in sd and not any(".norm." in k for k in sd)
    one = _small({"ROI_BOX_CASCADE_HEAD": {"IOUS": (0.5,), "BBOX_REG_WEIGHTS": ((10.0, 10.0, 5.0, 5.0),)}, "ROI_BOX_HEAD": {"NUM_CONV": 0}})
    assert one.num_stages == 1 and tuple(one.state_dict()["box_head.0.fc1.weight"].shape) == (8, 8 * 9) and "box_head.1.fc1.weight" not in one.state_dict()


class _D2Conv(nn.Conv2d):
    """detectron2.layers.Conv2d's parameter tree: an nn.Conv2d with its norm as the child ``norm``."""

    def __init__(self, cin, cout, k, norm, **kw):
        super().__init__(cin, cout, k, bias=norm is None, **kw)
        if norm is not None:
            self.norm = norm


def _torch_heads(C=8, S=3, fc=8, K=3, stages=3, Sm=4):
    """The Cascade heads of SMALL as plain torch modules under detectron2's names, SyncBatchNorm norms."""
    m = nn.Module()
    m.box_head, m.box_predictor = nn.ModuleList(), nn.ModuleList()
    for _ in range(stages):
        hd = nn.Module()
        hd.conv1, hd.conv2 = _D2Conv(C, 8, 3, nn.SyncBatchNorm(8), padding=1), _D2Conv(8, 8, 3, nn.SyncBatchNorm(8), padding=1)
        hd.fc1 = nn.Linear(8 * S * S, fc)
        pr = nn.Module()
        pr.cls_score, pr.bbox_pred = nn.Linear(fc, K + 1), nn.Linear(fc, 4)
        m.box_head.append(hd)
        m.box_predictor.append(pr)
    m.mask_head = nn.Module()
    m.mask_head.mask_fcn1 = _D2Conv(C, 8, 3, nn.SyncBatchNorm(8), padding=1)
    m.mask_head.deconv = nn.ConvTranspose2d(8, 8, 2, stride=2)
    m.mask_head.predictor = nn.Conv2d(8, K, 1)
    return m


def test_syncbatchnorm_checkpoint_loads_strictly():
    src = _torch_heads()
    g = torch.Generator().manual_seed(0)
    ckpt = {}
    for k, v in src.state_dict().items():
        ckpt["roi_heads." + k] = torch.tensor(7) if k.endswith("num_batches_tracked") else torch.rand(v.shape, generator=g) + 0.5
    ckpt["proposal_generator.rpn_head.conv.bias"] = torch.zeros(1)
    assert sum(k.endswith("num_batches_tracked") for k in ckpt) == 3 * 2 + 1
    h = _small()
    res = h.load_state_dict({k[len("roi_heads."):]: v for k, v in ckpt.items() if k.startswith("roi_heads.")}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, ckpt["roi_heads." + k]) for k, v in h.state_dict().items())
    assert all(not p.requires_grad for p in h.parameters())
    # FrozenBN has no num_batches_tracked: the same checkpoint has nowhere to put it
    frozen = _small({"ROI_BOX_HEAD": {"NORM": "FrozenBN"}, "ROI_MASK_HEAD": {"NORM": "FrozenBN"}})
    with pytest.raises(RuntimeError, match="num_batches_tracked"):
        frozen.load_state_dict({k[len("roi_heads."):]: v for k, v in ckpt.items() if k.startswith("roi_heads.")}, strict=True)
    frozen.load_state_dict({k[len("roi_heads."):]: v for k, v in ckpt.items() if k.startswith("roi_heads.") and not k.endswith("num_batches_tracked")},
                           strict=True)
    det = torch.nn.Module()
    det.roi_heads = h
    assert set(det.state_dict()) == {k for k in ckpt if k.startswith("roi_heads.")}


# ------------------------------------------------------------------------------------------------ the fold and its cache
def _randomise(h, seed=1):
    g = torch.Generator().manual_seed(seed)
    for name, t in list(h.named_parameters()) + list(h.named_buffers()):
        if name.endswith("num_batches_tracked"):
            continue
        with torch.no_grad():
            t.copy_(0.5 + 1.5 * torch.rand(t.shape, generator=g) if name.endswith("running_var") else torch.randn(t.shape, generator=g))


def test_fold_equals_the_unfolded_norm_and_is_rounded_once():
    """The fold's formula in fp64 (w s, (b - mean) s + beta with s = gamma / sqrt(var + eps)) applied in fp64 equals norm(conv(x)) in fp64 to
    1e-12 relative; what the heads hold is that fp64 fold rounded to fp32 ONCE, bit for bit (so the held weights themselves are within fp32
    rounding of it, not within 1e-12)."""
    h = _small()
    _randomise(h)
    g = torch.Generator().manual_seed(2)
    for conv, x in ((h.box_head[1].conv1, torch.randn((4, 8, 3, 3), generator=g, dtype=torch.float64)),
                    (h.box_head[2].conv2, torch.randn((4, 8, 3, 3), generator=g, dtype=torch.float64)),
                    (h.mask_head.mask_fcn1, torch.randn((2, 8, 4, 4), generator=g, dtype=torch.float64))):
        n = conv.norm
        assert float(n.running_var.min()) >= 0.5 and float(n.running_var.max()) <= 2.0
        s = n.weight.double() / torch.sqrt(n.running_var.double() + 1e-5)
        w64, b64 = conv.weight.double() * s.view(-1, 1, 1, 1), (0.0 - n.running_mean.double()) * s + n.bias.double()
        want = Q.conv_norm_relu(x, conv.weight, None, {k: getattr(n, k) for k in Q.NORM_KEYS})
        got = torch.relu(F.conv2d(x, w64, b64, padding=1))
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        ref = nn.BatchNorm2d(8).double().eval()
        ref.load_state_dict({k: getattr(n, k).double() for k in Q.NORM_KEYS}, strict=False)
        with torch.no_grad():
            assert float((torch.relu(ref(F.conv2d(x, conv.weight.double(), padding=1))) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    convs, _ = h._prepare(1)
    c1 = h.box_head[1].conv1
    s = c1.norm.weight.double() / torch.sqrt(c1.norm.running_var.double() + 1e-5)
    assert torch.equal(convs[0][0], (c1.weight.double() * s.view(-1, 1, 1, 1)).float()) and convs[0][0].permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(convs[0][1], ((0.0 - c1.norm.running_mean.double()) * s + c1.norm.bias.double()).float())
    mconvs = h._prepare_mask()[0]
    mc = h.mask_head.mask_fcn1
    s = mc.norm.weight.double() / torch.sqrt(mc.norm.running_var.double() + 1e-5)
    assert torch.equal(mconvs[0][0], (mc.weight.double() * s.view(-1, 1, 1, 1)).float())
    # without a norm the held weight is the conv's own and the bias its bias
    plain = _small({"ROI_BOX_HEAD": {"NORM": ""}, "ROI_MASK_HEAD": {"NORM": ""}})
    _randomise(plain)
    pc, _ = plain._prepare(0)
    assert torch.equal(pc[1][0], plain.box_head[0].conv2.weight) and torch.equal(pc[1][1], plain.box_head[0].conv2.bias)


def test_prepared_weights_are_cached_and_rebuilt_on_in_place_edits():
    h = _small()
    _randomise(h)
    convs, fcs = h._prepare(2)
    again = h._prepare(2)
    assert again[0] is convs and again[1] is fcs and h._prepare(1)[0] is not convs
    w0, b0 = convs[0][0].clone(), convs[0][1].clone()
    h.box_head[2].conv1.norm.running_var.mul_(4.0)
    c2 = h._prepare(2)[0]
    assert c2 is not convs and not torch.equal(c2[0][0], w0) and torch.allclose(c2[0][0], w0 * 0.5, rtol=1e-4, atol=0)
    h.box_head[2].conv1.weight.mul_(2.0)
    c3 = h._prepare(2)[0]
    assert c3 is not c2 and torch.allclose(c3[0][0], w0, rtol=1e-4, atol=0) and torch.equal(c3[0][1], c2[0][1])
    h.box_head[2].conv2.norm.running_mean.add_(1.0)
    assert h._prepare(2)[0] is not c3
    assert h._prepare(2)[1] is fcs, "the FC weights do not depend on the convs"
    h.box_head[2].fc1.weight.mul_(2.0)
    f2 = h._prepare(2)[1]
    assert f2 is not fcs and torch.equal(f2[0], 2.0 * fcs[0])
    m0 = h._prepare_mask()
    assert h._prepare_mask() is m0
    h.mask_head.mask_fcn1.norm.running_var.add_(1.0)
    assert h._prepare_mask() is not m0
    # fc1's permuted weight reads the last conv's [S][S][C] memory order
    x = torch.randn((5, 8, 3, 3), generator=torch.Generator().manual_seed(3))
    assert torch.allclose(x.permute(0, 2, 3, 1).reshape(5, -1) @ f2[0].t(), x.flatten(1) @ h.box_head[2].fc1.weight.t(), atol=1e-4)
    assert f2[1].shape == (8, 8) and torch.equal(f2[1][:4], h.box_predictor[2].cls_score.weight) and torch.equal(f2[1][4:8], h.box_predictor[2].bbox_pred.weight)


# ------------------------------------------------------------------------------------------------ config
def test_cascade_head_defaults_are_detectron2s():
    ch = amd.get_cfg().MODEL.ROI_BOX_CASCADE_HEAD
    assert tuple(tuple(w) for w in ch.BBOX_REG_WEIGHTS) == ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))
    assert tuple(ch.IOUS) == (0.5, 0.6, 0.7) and sorted(ch.keys()) == ["BBOX_REG_WEIGHTS", "IOUS"]
    m = amd.get_cfg().MODEL
    assert m.ROI_BOX_HEAD.NUM_CONV == 0 and m.ROI_BOX_HEAD.CONV_DIM == 256 and m.ROI_HEADS.IOU_THRESHOLDS == [0.5] and m.RPN.PRE_NMS_TOPK_TEST == 6000


CASCADE_YAMLS = ("inference/AFI-GAN_cascade_mask_rcnn_ResNeSt101_FPN.yaml", "inference/AFI-GAN_cascade_mask_rcnn_ResNeSt101_PAFPN.yaml",
                 "inference/AFI-GAN_cascade_rcnn_swint_BiFPN_ST.yaml")


@pytest.mark.parametrize("rel", CASCADE_YAMLS)
def test_reference_cascade_yaml_sections_merge_and_build(rel):
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_yaml_keys.json")))
    cfg = amd.get_cfg()
    if not hasattr(cfg, "merge_from_dict"):
        pytest.skip("a yacs CfgNode: detectron2's own defaults apply")
    assert fx[rel]["_BASE_"] == "../Base-RCNN-FPN-AFIGAN.yaml"
    for src in ("Base-RCNN-FPN-AFIGAN.yaml", rel):
        for key, val in fx[src]["keys"].items():
            parts = key.split(".")
            if parts[0] == "MODEL" and (parts[1].startswith("ROI_") or parts[1] == "MASK_ON"):
                d = val
                for p in reversed(parts):
                    d = {p: d}
                cfg.merge_from_dict(d)
    m = cfg.MODEL
    assert (m.ROI_HEADS.NAME, m.ROI_BOX_HEAD.NUM_CONV, m.ROI_BOX_HEAD.NUM_FC, m.ROI_BOX_HEAD.NORM, m.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG,
            m.ROI_MASK_HEAD.NORM) == ("CascadeROIHeads", 4, 1, "SyncBN", True, "SyncBN")
    swin = "swint" in rel
    assert m.MASK_ON is (not swin) and m.ROI_HEADS.IN_FEATURES == (["p3", "p4", "p5", "p6"] if swin else ["p2", "p3", "p4", "p5"])
    h = amd.build_roi_heads(cfg, _shapes(), masks=m.MASK_ON, cascade=True)
    assert isinstance(h, amd.CascadeROIHeads) and h.num_stages == 3 and h.box_pooler.min_level == (3 if swin else 2) and h.mask_on is (not swin)
    assert len(h.state_dict()) == 90 + (0 if swin else 28) and h.box_pooler.output_size == 7


# ------------------------------------------------------------------------------------------------ refusals
def test_the_keyword_and_the_name():
    with pytest.raises(amd.AfiError, match=r"ROI_HEADS\.NAME 'CascadeROIHeads' is not supported.*cascade=True"):
        amd.build_roi_heads(_cfg(), _shapes())
    with pytest.raises(amd.AfiError, match=r"ROI_HEADS\.NAME 'CascadeROIHeads'"):
        amd.build_roi_heads(_cfg(), _shapes(), masks=True)
    with pytest.raises(amd.AfiError, match=r"ROI_HEADS\.NAME 'CascadeROIHeads' is not supported \(StandardROIHeads only"):
        amd.StandardROIHeads(_cfg(), _shapes(), masks=True)
    with pytest.raises(amd.AfiError, match=r"cascade=True.*'CascadeROIHeads'.*got 'StandardROIHeads'"):
        amd.build_roi_heads(_cfg(model={"ROI_HEADS": {"NAME": "StandardROIHeads"}}), _shapes(), masks=True, cascade=True)
    with pytest.raises(amd.AfiError, match=r"ROI_HEADS\.NAME 'StandardROIHeads' is not 'CascadeROIHeads'"):
        amd.CascadeROIHeads(_cfg(model={"ROI_HEADS": {"NAME": "StandardROIHeads"}}), _shapes(), masks=True)
    # the conv head and the normed mask head stay the Cascade class's: StandardROIHeads' refusals are word for word what they were
    std = {"ROI_HEADS": {"NAME": "StandardROIHeads"}}
    with pytest.raises(amd.AfiError, match=r"ROI_BOX_HEAD\.NUM_CONV 4 is not supported \(FC-only box head; the conv head is CascadeROIHeads' and out of scope\)"):
        amd.build_roi_heads(_cfg(model=std), _shapes(), masks=True)
    with pytest.raises(amd.AfiError, match=r"ROI_BOX_HEAD\.NORM 'SyncBN' is not supported \(the FC-only box head has no norm\)"):
        amd.build_roi_heads(_cfg(model=dict(std, ROI_BOX_HEAD={"NUM_CONV": 0})), _shapes(), masks=True)
    with pytest.raises(amd.AfiError, match=r"ROI_MASK_HEAD\.NORM 'SyncBN' is not supported \(the mask head without norm only"):
        amd.build_roi_heads(_cfg(model=dict(std, ROI_BOX_HEAD={"NUM_CONV": 0, "NORM": ""})), _shapes(), masks=True)
    with pytest.raises(amd.AfiError, match=r"box branch only; set MODEL\.MASK_ON False.*masks=True"):
        amd.build_roi_heads(_cfg(), _shapes(), cascade=True)
    with pytest.raises(amd.AfiError, match=r"masks=True.*MODEL\.MASK_ON"):
        amd.build_roi_heads(_cfg(SWIN), _shapes(), masks=True, cascade=True)


W3 = ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))


@pytest.mark.parametrize("model,match", [
    ({"ROI_BOX_HEAD": {"CLS_AGNOSTIC_BBOX_REG": False}}, r"ROI_BOX_HEAD\.CLS_AGNOSTIC_BBOX_REG False"),
    ({"ROI_BOX_CASCADE_HEAD": {"IOUS": (0.5, 0.6)}}, r"ROI_BOX_CASCADE_HEAD\.IOUS has 2 entries and MODEL\.ROI_BOX_CASCADE_HEAD\.BBOX_REG_WEIGHTS 3"),
    ({"ROI_BOX_CASCADE_HEAD": {"IOUS": (), "BBOX_REG_WEIGHTS": ()}}, r"ROI_BOX_CASCADE_HEAD\.IOUS gives 0 stages; 1\.\.8"),
    ({"ROI_BOX_CASCADE_HEAD": {"IOUS": (0.5,) * 9, "BBOX_REG_WEIGHTS": W3 * 3}}, r"ROI_BOX_CASCADE_HEAD\.IOUS gives 9 stages; 1\.\.8"),
    ({"ROI_BOX_CASCADE_HEAD": {"IOUS": (0.6, 0.6, 0.7)}}, r"ROI_BOX_CASCADE_HEAD\.IOUS\[0\] 0\.6 must equal MODEL\.ROI_HEADS\.IOU_THRESHOLDS\[0\] 0\.5"),
    ({"ROI_BOX_CASCADE_HEAD": {"BBOX_REG_WEIGHTS": (W3[0], (20.0, 20.0, 10.0), W3[2])}}, r"ROI_BOX_CASCADE_HEAD\.BBOX_REG_WEIGHTS\[1\] .* must be four positive numbers"),
    ({"ROI_BOX_CASCADE_HEAD": {"BBOX_REG_WEIGHTS": (W3[0], W3[1], (30.0, 30.0, 0.0, 15.0))}}, r"ROI_BOX_CASCADE_HEAD\.BBOX_REG_WEIGHTS\[2\] .* must be four positive numbers"),
    ({"ROI_BOX_HEAD": {"NUM_FC": 0}}, r"ROI_BOX_HEAD\.NUM_FC 0 must be >= 1"),
    ({"ROI_BOX_HEAD": {"CONV_DIM": 0}}, r"ROI_BOX_HEAD\.CONV_DIM 0 must be a positive multiple of 4"),
    ({"ROI_BOX_HEAD": {"CONV_DIM": 130}}, r"ROI_BOX_HEAD\.CONV_DIM 130 must be a positive multiple of 4"),
    ({"ROI_BOX_HEAD": {"NUM_CONV": -1}}, r"ROI_BOX_HEAD\.NUM_CONV -1"),
    ({"ROI_BOX_HEAD": {"NORM": "GN"}}, r"ROI_BOX_HEAD\.NORM 'GN'"),
    ({"ROI_MASK_HEAD": {"NORM": "GN"}}, r"ROI_MASK_HEAD\.NORM 'GN'"),
    ({"ROI_MASK_HEAD": {"NORM": "GN", "NUM_CONV": 0}}, r"ROI_MASK_HEAD\.NORM 'GN'"),
    ({"ROI_MASK_HEAD": {"CONV_DIM": 130}}, r"ROI_MASK_HEAD\.CONV_DIM 130"),
    ({"ROI_BOX_HEAD": {"NAME": "MyHead"}}, r"ROI_BOX_HEAD\.NAME 'MyHead'"),
    ({"ROI_BOX_HEAD": {"POOLER_TYPE": "ROIPool"}}, r"ROI_BOX_HEAD\.POOLER_TYPE 'ROIPool'"),
    ({"KEYPOINT_ON": True}, r"MODEL\.KEYPOINT_ON"),
    ({"ROI_HEADS": {"IN_FEATURES": ["p2", "p9"]}}, r"ROI_HEADS\.IN_FEATURES"),
])
def test_unsupported_cascade_configs_raise(model, match):
    with pytest.raises(amd.AfiError, match=match):
        amd.build_roi_heads(_cfg(model=model), _shapes(), masks=True, cascade=True)


class _FakeCuda:
    is_cuda = True

    def __init__(self, dtype):
        self.dtype = dtype


def test_call_time_refusals():
    h = _small().eval()
    images = type("Images", (), {"image_sizes": [(32, 32)], "__len__": lambda s: 1})()
    x = torch.zeros((1, 8, 8, 8))
    with pytest.raises(amd.AfiError, match="targets given"):
        h(images, {"p2": x}, [], targets=[None])
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        h(images, {"p2": x}, [])
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        h.forward_padded(torch.zeros((1, 2)), {"p2": x}, torch.zeros((1, 1, 4)), torch.ones((1,), dtype=torch.int32))
    with pytest.raises(amd.AfiError, match="features .* are missing"):
        h(images, {"p3": x}, [])
    with pytest.raises(amd.AfiError, match="stage by stage"):
        h.select(None, None, None, None)
    h.train()
    with pytest.raises(amd.AfiError, match="inference-only"):
        h(images, {"p2": x}, [])
    with pytest.raises(amd.AfiError, match="inference-only"):
        h.forward_with_given_boxes({"p2": x}, [])
    from afigan_amd.roi_heads import _check_feature
    with pytest.raises(amd.AfiError, match=r"torch\.float16; fp32 only"):
        _check_feature("roi_heads", "feature p2", _FakeCuda(torch.float16))
    from afigan_amd import ops
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        ops.roi_cascade_stage(torch.zeros((2, 8)), 3, torch.zeros((1, 2, 4)), torch.ones((1,), dtype=torch.int32), torch.zeros((1, 2)), W3[0])


def test_entry_point_checks_its_arguments_without_a_device():
    """AFI_ERR_BAD_ARG / AFI_ERR_UNSUPPORTED come back before anything is launched (fake, never dereferenced pointers): the sibling's checks."""
    from afigan_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.DEFINES["AFI_ERR_BAD_ARG"], _lib.DEFINES["AFI_ERR_UNSUPPORTED"]
    p = 0x1000

    def run(pred=p, ld=85, N=1, P=4, K=80, props=p, counts=p, hw=p, w=(10.0, 10.0, 5.0, 5.0), prev=None, scale=1.0, scores=p, boxes=p):
        return lib.afi_roi_cascade_stage(pred, ld, N, P, K, props, counts, hw, *w, 4.135, prev, scale, scores, boxes, None)
    for kw in ({"pred": None}, {"props": None}, {"counts": None}, {"hw": None}, {"scores": None}, {"boxes": None}, {"N": 0}, {"N": 65536}, {"P": 0},
               {"K": 0}, {"ld": 84}, {"w": (0.0, 10.0, 5.0, 5.0)}, {"w": (10.0, 10.0, 5.0, -1.0)}, {"w": (10.0, float("nan"), 5.0, 5.0)},
               {"scale": 0.0}, {"scale": -1.0}, {"scale": float("nan")}, {"scale": float("inf")}):
        assert run(**kw) == BAD, kw
    assert run(K=1025, ld=1030) == UNS
    assert lib.afi_roi_scores_boxes(p, 84, 1, 4, 80, 1, p, p, p, 10.0, 10.0, 5.0, 5.0, 4.135, p, p, None) == BAD       # the sibling's ld check


# ------------------------------------------------------------------------------------------------ the checker against other restatements
def test_mean_scores_against_a_python_loop():
    r = np.random.RandomState(4)
    for S in (1, 2, 3, 5, 8):
        per = [r.rand(2, 3, 4).astype(np.float32) for _ in range(S)]
        per[0][0, 0, 0], per[-1][1, 2, 3] = -np.inf, np.nan
        got = Q.mean_scores(per)
        assert got.dtype == np.float32
        for idx in np.ndindex(2, 3, 4):
            acc = np.float32(0)
            with np.errstate(invalid="ignore"):
                for s in per:                                    # python's sum(): 0 + s0 + s1 + ...
                    acc = np.float32(acc + s[idx])
                want = np.float32(acc * np.float32(1.0 / S))
            assert (np.isnan(want) and np.isnan(got[idx])) or want == got[idx]
    third = Q.mean_scores([np.float32([0.1]), np.float32([0.7]), np.float32([0.25])])
    assert third[0] == np.float32(np.float32(np.float32(0.1) + np.float32(0.7)) + np.float32(0.25)) * np.float32(1 / 3)


def test_conv_norm_chain_against_batchnorm_eval():
    h = _small()
    _randomise(h, seed=5)
    sd = h.state_dict()
    x = torch.randn((6, 8, 3, 3), generator=torch.Generator().manual_seed(6))
    convs, fcs, logits, deltas = Q.conv_fc_head(x, sd, stage=1)
    y = x.double()
    for i in (1, 2):
        bn = nn.BatchNorm2d(8).double().eval()
        bn.load_state_dict({k: sd[f"box_head.1.conv{i}.norm.{k}"].double() for k in Q.NORM_KEYS + ("num_batches_tracked",)})
        y = torch.relu(bn(F.conv2d(y, sd[f"box_head.1.conv{i}.weight"].double(), padding=1)))
        assert float((convs[i - 1] - y).abs().max()) <= 1e-12 * float(y.abs().max())
    a = torch.relu(F.linear(y.flatten(1), sd["box_head.1.fc1.weight"].double(), sd["box_head.1.fc1.bias"].double()))
    assert torch.allclose(fcs[0], a, rtol=1e-12, atol=1e-12) and logits.shape == (6, 4) and deltas.shape == (6, 4)
    assert torch.allclose(logits, F.linear(a, sd["box_predictor.1.cls_score.weight"].double(), sd["box_predictor.1.cls_score.bias"].double()), rtol=1e-12, atol=1e-12)
    # the folded weights the kernels read give the same chain within fp32 rounding of the weights
    pc, (w1, wp, bp) = h._prepare(1)
    z = x.double()
    for w, b in pc:
        z = torch.relu(F.conv2d(z, w.double(), b.double(), padding=1))
    assert float((z - y).abs().max()) <= 1e-5 * float(y.abs().max())
    pred = torch.relu(z.permute(0, 2, 3, 1).reshape(6, -1) @ w1.double().t() + sd["box_head.1.fc1.bias"].double()) @ wp.double().t() + bp.double()
    assert torch.allclose(pred[:, :4], logits, rtol=0, atol=1e-4 * float(logits.abs().max())) and torch.allclose(pred[:, 4:8], deltas, rtol=0, atol=1e-4)
    # the mask chain: with the norm, and equal to mask_f64's when there is none
    m = torch.randn((2, 8, 4, 4), generator=torch.Generator().manual_seed(7))
    acts, dec = Q.mask_head_chain(m, {"mask_head." + k: v for k, v in h.mask_head.state_dict().items()})
    bn = nn.BatchNorm2d(8).double().eval()
    bn.load_state_dict({k: sd[f"mask_head.mask_fcn1.norm.{k}"].double() for k in Q.NORM_KEYS}, strict=False)
    want = torch.relu(bn(F.conv2d(m.double(), sd["mask_head.mask_fcn1.weight"].double(), padding=1)))
    assert float((acts[0] - want).abs().max()) <= 1e-12 * float(want.abs().max()) and dec.shape == (2, 32, 4, 4)
    import mask_f64 as QM
    plain = _small({"ROI_BOX_HEAD": {"NORM": ""}, "ROI_MASK_HEAD": {"NORM": ""}})
    _randomise(plain, seed=8)
    psd = {"mask_head." + k: v for k, v in plain.mask_head.state_dict().items()}
    a1, d1 = Q.mask_head_chain(m, psd)
    a2, d2 = QM.head_chain(m, psd)
    assert torch.equal(a1[0], a2[0]) and torch.equal(d1, d2)


# ------------------------------------------------------------------------------------------------ the GPU tests' seeded inputs
@pytest.mark.parametrize("K", Q.STAGE_KS)
def test_stage_inputs_meet_the_gpu_tests_conditions(K):
    pred, props = Q.stage_case(K)
    assert pred.shape == (100, (K + 8) // 4 * 4) and props.shape == (2, 50, 4) and np.abs(pred[:, :K + 1][np.isfinite(pred[:, :K + 1])]).max() > 29
    for w in Q.STAGE_WEIGHTS:
        for counts in Q.STAGE_COUNTS:
            s, b, _ = QB.scores_boxes(pred, K, True, props, counts, Q.STAGE_HW, w)
            assert pred[3, K + 3] / w[2] > QB.SCALE_CLAMP and pred[4, K + 4] / w[3] > QB.SCALE_CLAMP, "deltas above the clamp"
            for n, c in enumerate(counts):
                ih, iw = Q.STAGE_HW[n]
                if c > 7:
                    assert (b[n, 5, 0, :2] == 0).all() and b[n, 6, 0, 2] == iw and b[n, 6, 0, 3] == ih, "all four clips"
                    assert np.isnan(s[n, 7]).all() and np.isfinite(s[n, :7]).all()
                assert np.isneginf(s[n, c:]).all() and not b[n, c:].any()
            prev = Q.stage_prev(K, counts)
            assert all(np.isneginf(prev[n, c:]).all() and np.isfinite(prev[n, :c]).all() for n, c in enumerate(counts))
    assert np.float32(1 / 3) != np.float32(1) and np.float32(0.5) * 2 == 1


@pytest.mark.parametrize("layout,stages,K,masks", Q.WHOLE_CASES)
def test_whole_heads_inputs_meet_the_gpu_tests_conditions(layout, stages, K, masks):
    """On the fp64 chain for the chosen seeds: no stage-0 box near a level or grid boundary, at least 3 valid candidates per non-empty image, and
    the greedy NMS keeps between 10 % and 90 % of them."""
    feats, (ih, iw), levels, hw = Q.WHOLE_LAYOUTS[layout]
    ml = int(feats[0][1:])
    assert ml == (3 if layout == "swin" else 2) and [int(f[1:]) for f in feats] == list(range(ml, ml + 4))
    boxes = Q.whole_boxes(layout)
    assert boxes.shape == (2, Q.WHOLE_P, 4) and boxes.min() >= 0 and boxes[..., 0::2].max() <= iw and boxes[..., 1::2].max() <= ih
    assert QB.align_facts(boxes, 7, 0, ml, ml + 3, skip=0) > 1e-6
    h = Q.whole_heads(amd, layout, stages, K, masks)
    assert h.num_stages == stages and h.mask_on == masks and h.box_pooler.min_level == ml
    xs = Q.whole_features(layout)
    mean, last, per = Q.chain(h.state_dict(), [xs[f].numpy() for f in feats], ml, boxes, Q.WHOLE_COUNTS, hw, 7, 0, K, h.stage_weights)
    assert len(per) == stages and np.array_equal(mean, Q.mean_scores(per), equal_nan=True)
    for n, c in enumerate(Q.WHOLE_COUNTS):
        assert np.isneginf(mean[n, c:]).all() and np.isfinite(mean[n, :c]).all() and not last[n, c:].any()
        assert np.abs(mean[n, :c].sum(-1)).max() <= 1 + 1e-5
    moved = np.abs(last - boxes)[0].max()
    assert moved > 0.5, "the stages must move the boxes"
    facts = Q.selection_facts(mean, last, h.test_score_thresh, h.test_nms_thresh)
    print(f"[cascade inputs] {layout} S {stages} K {K}: (valid, kept) per image {facts}, largest box movement {moved:.2f}")
    for valid, kept in facts:
        assert valid >= 3 and 0.1 * valid <= kept <= 0.9 * valid, facts
