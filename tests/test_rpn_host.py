"""CPU-side checks of the frozen RPN proposal generator (afigan_amd/rpn.py): detectron2's key names and shapes and a strict load of a
detector checkpoint's ``proposal_generator.*`` tensors, the cell anchors against their closed form, the config defaults and the reference-style
yaml sections merging, every refusal, and tests/rpn_f64.py -- the fp64 yardstick of test_gpu_rpn.py -- against a brute-force NMS written
differently.  Also the GPU NMS test's inputs, generated here and held to their two conditions, so that a bad seed fails without a GPU."""
import math

import numpy as np
import pytest
import torch

import afigan_amd as amd
from afigan_amd import rpn
from afigan_amd.fpn_sr import ShapeSpec

import rpn_f64 as R

FEATURES = ["p2", "p3", "p4", "p5", "p6"]


def _cfg(**rpn_keys):
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[32], [64], [128], [256], [512]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": FEATURES, "PRE_NMS_TOPK_TEST": 1000, "POST_NMS_TOPK_TEST": 1000, **rpn_keys}})
    return cfg


def _shapes(channels=256, names=FEATURES):
    return {f: ShapeSpec(channels=channels, stride=4 * 2 ** i) for i, f in enumerate(names)}


def test_key_names_shapes_and_frozen_parameters():
    m = amd.RPN(_cfg(), _shapes())
    sd = m.state_dict()
    want = {"rpn_head.conv.weight": (256, 256, 3, 3), "rpn_head.conv.bias": (256,), "rpn_head.objectness_logits.weight": (3, 256, 1, 1),
            "rpn_head.objectness_logits.bias": (3,), "rpn_head.anchor_deltas.weight": (12, 256, 1, 1), "rpn_head.anchor_deltas.bias": (12,)}
    want.update({f"anchor_generator.cell_anchors.{l}": (3, 4) for l in range(5)})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert all(not p.requires_grad for p in m.parameters()) and len(list(m.parameters())) == 6
    assert m.in_features == FEATURES and m.num_anchors == 3 and m.anchor_generator.strides == [4, 8, 16, 32, 64]
    assert (m.pre_nms_topk, m.post_nms_topk, m.nms_thresh, m.min_box_side_len, m.box_weights) == (1000, 1000, 0.7, 0.0, (1.0, 1.0, 1.0, 1.0))


def test_detector_checkpoint_keys_load_strictly():
    """A detectron2 detector checkpoint names these tensors ``proposal_generator.*``: with the prefix stripped they load with strict=True."""
    src = amd.RPN(_cfg(), _shapes())
    g = torch.Generator().manual_seed(0)
    ckpt = {"proposal_generator." + k: torch.randn(v.shape, generator=g) for k, v in src.state_dict().items()}
    ckpt["backbone.fpn_output2.weight"] = torch.zeros(1)
    m = amd.RPN(_cfg(), _shapes())
    own = {k[len("proposal_generator."):]: v for k, v in ckpt.items() if k.startswith("proposal_generator.")}
    res = m.load_state_dict(own, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in m.state_dict().items():
        assert torch.equal(v, ckpt["proposal_generator." + k]), k
    # under a detector module the prefix is the attribute name
    det = torch.nn.Module()
    det.proposal_generator = m
    assert {k for k in det.state_dict()} == {k for k in ckpt if k.startswith("proposal_generator.")}


def test_cell_anchors_match_the_closed_form():
    m = amd.RPN(_cfg(), _shapes())
    for l, size in enumerate((32, 64, 128, 256, 512)):
        got = m.anchor_generator.cell_anchors[l].double().numpy()
        want = R.cell_anchors([size], [0.5, 1.0, 2.0])
        assert got.shape == (3, 4) and np.abs(got - want).max() <= 2.0 ** -24 * 2 * size
        for a, ratio in enumerate((0.5, 1.0, 2.0)):
            w, h = want[a, 2] - want[a, 0], want[a, 3] - want[a, 1]
            assert math.isclose(w * h, size * size, rel_tol=1e-12) and math.isclose(h / w, ratio, rel_tol=1e-12)
    # sizes, then ratios; one shared entry is repeated for every level
    c = rpn.generate_cell_anchors([32, 64], [0.5, 2.0]).double().numpy()
    assert np.allclose(c, R.cell_anchors([32, 64], [0.5, 2.0]), rtol=1e-7) and c[1, 3] > c[0, 3] and c[2, 2] > c[0, 2]
    cfg = _cfg()
    cfg.MODEL.ANCHOR_GENERATOR.SIZES = [[32, 64]]
    m2 = amd.RPN(cfg, _shapes())
    assert m2.num_anchors == 6 and all(torch.equal(b, m2.anchor_generator.cell_anchors[0]) for b in m2.anchor_generator.cell_anchors)
    assert tuple(m2.state_dict()["rpn_head.anchor_deltas.weight"].shape) == (24, 256, 1, 1)


def test_config_defaults_are_detectron2s():
    m = amd.get_cfg().MODEL
    assert (m.PROPOSAL_GENERATOR.NAME, m.PROPOSAL_GENERATOR.MIN_SIZE) == ("RPN", 0)
    ag = m.ANCHOR_GENERATOR
    assert (ag.NAME, ag.SIZES, ag.ASPECT_RATIOS, ag.ANGLES, ag.OFFSET) == ("DefaultAnchorGenerator", [[32, 64, 128, 256, 512]], [[0.5, 1.0, 2.0]],
                                                                        [[-90, 0, 90]], 0.0)
    r = m.RPN
    assert (r.HEAD_NAME, r.IN_FEATURES, r.BOUNDARY_THRESH, r.IOU_THRESHOLDS, r.IOU_LABELS) == ("StandardRPNHead", ["res4"], -1, [0.3, 0.7], [0, -1, 1])
    assert (r.BATCH_SIZE_PER_IMAGE, r.POSITIVE_FRACTION, tuple(r.BBOX_REG_WEIGHTS), r.SMOOTH_L1_BETA, r.LOSS_WEIGHT) == (256, 0.5, (1.0, 1.0, 1.0, 1.0), 0.0, 1.0)
    assert (r.PRE_NMS_TOPK_TRAIN, r.PRE_NMS_TOPK_TEST, r.POST_NMS_TOPK_TRAIN, r.POST_NMS_TOPK_TEST, r.NMS_THRESH) == (12000, 6000, 2000, 1000, 0.7)


def test_reference_style_yaml_sections_merge():
    """The ANCHOR_GENERATOR / RPN sections the reference's base yaml sets (and the inference yamls' overrides) merge under the yacs rule; a
    key that is declared nowhere still raises."""
    cfg = amd.get_cfg()
    if not hasattr(cfg, "merge_from_dict"):
        pytest.skip("a yacs CfgNode: detectron2's own defaults apply")
    cfg.merge_from_dict({"MODEL": {"ANCHOR_GENERATOR": {"SIZES": [[32], [64], [128], [256], [512]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                                   "RPN": {"IN_FEATURES": ["p2", "p3", "p4", "p5", "p6"], "PRE_NMS_TOPK_TRAIN": 2000, "PRE_NMS_TOPK_TEST": 1000,
                                           "POST_NMS_TOPK_TRAIN": 1000, "POST_NMS_TOPK_TEST": 1000}}})
    cfg.merge_from_dict({"MODEL": {"RPN": {"IN_FEATURES": ["p3", "p4", "p5", "p6", "p7"], "POST_NMS_TOPK_TRAIN": 2000}}})
    assert cfg.MODEL.RPN.IN_FEATURES == ["p3", "p4", "p5", "p6", "p7"] and cfg.MODEL.RPN.PRE_NMS_TOPK_TEST == 1000
    assert cfg.MODEL.RPN.NMS_THRESH == 0.7 and cfg.MODEL.ANCHOR_GENERATOR.SIZES[4] == [512]
    m = amd.RPN(cfg, _shapes(names=["p3", "p4", "p5", "p6", "p7"]))
    assert m.pre_nms_topk == 1000 and m.in_features[0] == "p3"
    with pytest.raises(KeyError, match="NO_SUCH_KEY"):
        cfg.merge_from_dict({"MODEL": {"RPN": {"NO_SUCH_KEY": 1}}})


def test_default_pre_nms_topk_is_refused_by_name():
    cfg = amd.get_cfg()
    cfg.MODEL.RPN.IN_FEATURES = ["p2"]
    with pytest.raises(amd.AfiError, match=r"PRE_NMS_TOPK_TEST 6000.*1024"):
        amd.RPN(cfg, _shapes())


@pytest.mark.parametrize("section,key,value,match", [
    ("ANCHOR_GENERATOR", "NAME", "RotatedAnchorGenerator", "rotated"),
    ("RPN", "HEAD_NAME", "MyHead", "StandardRPNHead"),
    ("RPN", "PRE_NMS_TOPK_TEST", 1025, "PRE_NMS_TOPK_TEST"),
    ("ANCHOR_GENERATOR", "ASPECT_RATIOS", [[0.25 * i for i in range(1, 18)]], "anchors per cell"),
    ("ANCHOR_GENERATOR", "OFFSET", 0.5, "OFFSET"),
    ("RPN", "IN_FEATURES", ["p2", "p9"], "IN_FEATURES"),
])
def test_unsupported_configs_raise(section, key, value, match):
    cfg = _cfg()
    setattr(getattr(cfg.MODEL, section), key, value)
    with pytest.raises(amd.AfiError, match=match):
        amd.RPN(cfg, _shapes())


class _Imgs:
    def __init__(self, sizes):
        self.image_sizes = sizes

    def __len__(self):
        return len(self.image_sizes)


def test_forward_refusals_without_a_gpu():
    m = amd.RPN(_cfg(), _shapes()).eval()
    feats = {f: torch.zeros(1, 256, 4, 4) for f in FEATURES}
    imgs = _Imgs([(16, 16)])
    with pytest.raises(amd.AfiError, match="gt_instances"):
        m(imgs, feats, gt_instances=[object()])
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        m(imgs, feats)
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        m.forward_padded(torch.tensor([[16.0, 16.0]]), feats)
    m.train()
    with pytest.raises(amd.AfiError, match="inference-only"):
        m(imgs, feats)
    m.eval()
    with pytest.raises(amd.AfiError, match="missing"):
        m(imgs, {"p2": feats["p2"]})


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_two_byte_features_are_refused(dtype):
    """The dtype check sits behind the device check; a stand-in that says it is on the GPU shows it without one."""
    m = amd.RPN(_cfg(), _shapes()).eval()
    fake = type("T", (), {"is_cuda": True, "dtype": dtype, "dim": lambda s: 4, "shape": (1, 256, 4, 4), "requires_grad": False})()
    with pytest.raises(amd.AfiError, match="fp32 features only"):
        m._check({f: fake for f in FEATURES})


def test_build_proposal_generator_and_registry():
    cfg = _cfg()
    assert isinstance(amd.build_proposal_generator(cfg, _shapes()), amd.RPN)
    assert amd.PROPOSAL_GENERATOR_REGISTRY.get("RPN") is amd.RPN
    cfg.MODEL.PROPOSAL_GENERATOR.NAME = "PrecomputedProposals"
    assert amd.build_proposal_generator(cfg, _shapes()) is None
    cfg.MODEL.PROPOSAL_GENERATOR.NAME = "RRPN"
    with pytest.raises(amd.AfiError, match="RRPN"):
        amd.build_proposal_generator(cfg, _shapes())


def test_detector_from_config_builds_the_rpn_and_stops_at_the_roi_heads(monkeypatch):
    """Without detectron2 ``_build_from_config`` now gets as far as the ROI heads: the proposal generator is built (observed through the
    builder) and the error names the ROI heads only."""
    try:
        import detectron2  # noqa: F401
        pytest.skip("detectron2 builds the ROI heads itself")
    except ImportError:
        pass
    built = []
    real = rpn.build_proposal_generator
    monkeypatch.setattr(rpn, "build_proposal_generator", lambda cfg, shape: built.append(real(cfg, shape)) or built[-1])

    class _BB:
        def output_shape(self):
            return _shapes()
    name = "_rpn_host_test_backbone"
    reg = amd.BACKBONE_REGISTRY
    if name not in reg:
        def _rpn_host_test_backbone(cfg, input_shape):
            return _BB()
        reg.register(_rpn_host_test_backbone)
    cfg = _cfg()
    cfg.MODEL.BACKBONE.NAME = name
    with pytest.raises(amd.AfiError, match="building the ROI heads from a config needs detectron2") as e:
        amd.GeneralizedRCNN_AFExtractor._build_from_config(cfg)
    assert "RPN" not in str(e.value) and len(built) == 1 and isinstance(built[0], amd.RPN)


# ------------------------------------------------------------------------------------------------ the yardstick itself
def _brute_nms(boxes, thresh):
    """Greedy NMS the other way round: a box is kept iff no KEPT earlier box overlaps it -- pairwise, scalar arithmetic, no matrix."""
    kept = []
    for i, (x1, y1, x2, y2) in enumerate(boxes.tolist()):
        ok = True
        for j in kept:
            a1, b1, a2, b2 = boxes[j].tolist()
            iw, ih = min(x2, a2) - max(x1, a1), min(y2, b2) - max(y1, b1)
            inter = iw * ih if iw > 0 and ih > 0 else 0.0
            if inter / ((x2 - x1) * (y2 - y1) + (a2 - a1) * (b2 - b1) - inter) > thresh:
                ok = False
                break
        if ok:
            kept.append(i)
    return kept


@pytest.mark.parametrize("thresh", [0.7, 0.5, 0.3])
def test_fp64_nms_matches_a_brute_force_one(thresh):
    b, _ = R.nms_case(11, 50)
    b = b.astype(np.float64)
    keep = R.nms(b, np.ones(50, bool), thresh)
    assert np.nonzero(keep)[0].tolist() == _brute_nms(b, thresh) and 0 < keep.sum() < 50
    valid = np.ones(50, bool)
    valid[[0, 7, 20]] = False                              # an invalid box is skipped and suppresses nothing
    rest = np.nonzero(valid)[0]
    assert np.nonzero(R.nms(b, valid, thresh))[0].tolist() == rest[_brute_nms(b[rest], thresh)].tolist()


def test_fp64_topk_decode_and_merge_rules():
    x = np.array([1.0, 3.0, np.nan, 3.0, -0.0, 0.0, -np.inf, 2.0], np.float32)
    assert R.topk(x, 8).tolist() == [1, 3, 7, 0, 4, 5, 6, 2] and R.topk(x, 2).tolist() == [1, 3]
    cell = R.cell_anchors([32], [0.5, 1.0, 2.0])
    # zero deltas give the anchor itself, clipped; anchor (y W + x) A + a sits at (x s, y s)
    b, v, _ = R.decode(np.zeros((2, 4)), [0, (2 * 5 + 3) * 3 + 1], cell, 8, 5, 3, (1, 1, 1, 1), (100, 100), 0)
    assert np.allclose(b[0], np.clip(cell[0], 0, 100)) and np.allclose(b[1], cell[1] + [24, 16, 24, 16]) and v.tolist() == [True, True]
    # dw above the clamp is clamped: the width is 1000 / 16 anchor widths before clipping
    _, _, (pcx, pcy, pw, ph) = R.decode(np.array([[0, 0, 10.0, 0]]), [1], cell, 8, 5, 3, (1, 1, 1, 1), (100, 100), 0)
    assert math.isclose(pw[0], 32 * 1000 / 16, rel_tol=1e-12) and math.isclose(ph[0], 32)
    # merge: by value, ties by position (level, then rank)
    vals = np.array([5, 3, 1, 4, 3, 3], np.float32)
    keep = np.array([1, 1, 0, 1, 1, 1], bool)
    assert R.merge(vals, keep, [0, 3, 6], 10).tolist() == [0, 3, 1, 4, 5] and R.merge(vals, keep, [0, 3, 6], 3).tolist() == [0, 3, 1]


@pytest.mark.parametrize("thresh", R.NMS_THRESHOLDS)
@pytest.mark.parametrize("n", [n for n in R.NMS_SIZES if n > 1])
@pytest.mark.parametrize("seed", R.NMS_SEEDS)
def test_gpu_nms_inputs_meet_their_conditions(seed, n, thresh):
    """What tests/test_gpu_rpn.py asserts before any launch, checked where no GPU is needed: no pair's fp64 IoU within 1e-5 of the threshold
    (the fp32 evaluation carries ~1e-6 relative error: such a pair would be decided by rounding), and 10 % .. 90 % of the boxes survive."""
    b, s = R.nms_case(seed, n)
    nonempty, ambiguous, kept = R.nms_case_facts(b, thresh)
    assert b.shape == (n, 4) and b.dtype == np.float32 and np.all(np.diff(s) <= 0)
    assert b[:, 0::2].min() >= 0 and b[:, 0::2].max() <= R.NMS_IMAGE[1] and b[:, 1::2].min() >= 0 and b[:, 1::2].max() <= R.NMS_IMAGE[0]
    assert nonempty and ambiguous == 0 and 0.1 <= kept <= 0.9, (nonempty, ambiguous, kept)


def test_library_answers_the_topk_workspace_query():
    lib = amd._lib.load()
    assert lib.afi_rpn_topk_ws_floats(2, 13, 21, 3) == 0                                  # small maps: the selecting block reads the logits itself
    n = 200 * 336 * 3
    assert lib.afi_rpn_topk_ws_floats(2, 200, 336, 3) == 2 * 4104 + 2 * 2 * n              # the histograms and one 8-byte word per logit
    assert lib.afi_rpn_topk_ws_floats(1, 200, 336, 17) == -1 and lib.afi_rpn_topk_ws_floats(1, 2048, 2048, 1) == -1
    assert lib.afi_rpn_merge(None, None, None, 1, 1, None, 1, None, None, None, None) == 1 and lib.afi_rpn_nms(None, None, 1, 0, 0, 0.7, None, None) == 0
