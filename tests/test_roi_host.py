"""CPU-side checks of the frozen box branch of StandardROIHeads (afigan_amd/roi_heads.py): detectron2's key names and shapes and a strict load
of a detector checkpoint's ``roi_heads.box_*`` tensors, the config defaults and the reference-style yaml sections merging, every refusal by its
message, and tests/roi_f64.py -- the fp64 yardstick of test_gpu_roi.py -- against brute-force scalar restatements written differently.  Also
the GPU tests' seeded inputs, held here to the conditions those tests assert, so that a bad seed fails without a GPU."""
import math

import numpy as np
import pytest
import torch

import afigan_amd as amd
from afigan_amd.fpn_sr import ShapeSpec

import roi_f64 as Q
import rpn_f64 as R

FEATURES = ["p2", "p3", "p4", "p5"]
R50_FPN = {"MASK_ON": False, "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": FEATURES},
           "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "POOLER_RESOLUTION": 7},
           "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": 4, "POOLER_RESOLUTION": 14}}     # the base yaml's sections


def _cfg(model=None, test=None):
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict(R50_FPN)
    for sec, d in (model or {}).items():
        if isinstance(d, dict):
            getattr(cfg.MODEL, sec).merge_from_dict(d)
        else:
            setattr(cfg.MODEL, sec, d)
    if test:
        cfg.TEST.merge_from_dict(test)
    return cfg


def _shapes(channels=256, names=("p2", "p3", "p4", "p5", "p6")):
    return {f: ShapeSpec(channels=channels, stride=2 ** int(f[1:])) for f in names}


# ------------------------------------------------------------------------------------------------ construction, keys, config
def test_fallback_defaults_are_detectron2s():
    cfg = amd.get_cfg()
    m = cfg.MODEL
    assert (m.MASK_ON, m.KEYPOINT_ON, cfg.TEST.DETECTIONS_PER_IMAGE) == (False, False, 100)
    rh, bh = m.ROI_HEADS, m.ROI_BOX_HEAD
    assert (rh.NUM_CLASSES, rh.SCORE_THRESH_TEST, rh.NMS_THRESH_TEST, rh.IN_FEATURES) == (80, 0.05, 0.5, ["res4"])
    assert (bh.NUM_FC, bh.FC_DIM, bh.NUM_CONV, bh.NORM, bh.POOLER_RESOLUTION, bh.POOLER_SAMPLING_RATIO, bh.POOLER_TYPE) == (0, 1024, 0, "", 14, 0, "ROIAlignV2")
    assert (tuple(bh.BBOX_REG_WEIGHTS), bh.CLS_AGNOSTIC_BBOX_REG, bh.SMOOTH_L1_BETA) == ((10.0, 10.0, 5.0, 5.0), False, 0.0)
    assert m.ROI_MASK_HEAD.NAME == "MaskRCNNConvUpsampleHead"
    # the keys of earlier sections are untouched
    assert m.RPN.PRE_NMS_TOPK_TEST == 6000 and m.FPN.OUT_CHANNELS == 256 and cfg.INPUT.FORMAT == "BGR"
    # from the bare fallback config, setting what a user must set
    m.ROI_HEADS.NAME, m.ROI_HEADS.IN_FEATURES, m.ROI_BOX_HEAD.NAME, m.ROI_BOX_HEAD.NUM_FC = "StandardROIHeads", ["p2", "p3"], "FastRCNNConvFCHead", 1
    h = amd.build_roi_heads(cfg, _shapes())
    assert h.box_pooler.output_size == 14 and tuple(h.state_dict()["box_head.fc1.weight"].shape) == (1024, 256 * 14 * 14)


def test_key_names_shapes_and_frozen_parameters():
    h = amd.build_roi_heads(_cfg(), _shapes())
    assert isinstance(h, amd.StandardROIHeads)
    want = {"box_head.fc1.weight": (1024, 12544), "box_head.fc1.bias": (1024,), "box_head.fc2.weight": (1024, 1024), "box_head.fc2.bias": (1024,),
            "box_predictor.cls_score.weight": (81, 1024), "box_predictor.cls_score.bias": (81,),
            "box_predictor.bbox_pred.weight": (320, 1024), "box_predictor.bbox_pred.bias": (320,)}
    assert {k: tuple(v.shape) for k, v in h.state_dict().items()} == want
    assert all(not p.requires_grad for p in h.parameters()) and len(list(h.parameters())) == 8
    assert (h.box_pooler.min_level, h.box_pooler.max_level, h.box_pooler.output_size, h.box_pooler.sampling_ratio) == (2, 5, 7, 0)
    assert (h.num_classes, h.test_score_thresh, h.test_nms_thresh, h.test_detections_per_img, h.box_weights) == (80, 0.05, 0.5, 100, (10.0, 10.0, 5.0, 5.0))
    ag = amd.build_roi_heads(_cfg({"ROI_BOX_HEAD": {"CLS_AGNOSTIC_BBOX_REG": True}, "ROI_HEADS": {"NUM_CLASSES": 3}}), _shapes())
    sd = ag.state_dict()
    assert tuple(sd["box_predictor.bbox_pred.weight"].shape) == (4, 1024) and tuple(sd["box_predictor.cls_score.weight"].shape) == (4, 1024)


def test_detector_checkpoint_keys_load_strictly():
    src = amd.build_roi_heads(_cfg(), _shapes())
    g = torch.Generator().manual_seed(0)
    ckpt = {"roi_heads." + k: torch.randn(v.shape, generator=g) for k, v in src.state_dict().items()}
    ckpt["proposal_generator.rpn_head.conv.bias"] = torch.zeros(1)
    h = amd.build_roi_heads(_cfg(), _shapes())
    own = {k[len("roi_heads."):]: v for k, v in ckpt.items() if k.startswith("roi_heads.box_")}
    res = h.load_state_dict(own, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, ckpt["roi_heads." + k]) for k, v in h.state_dict().items())
    det = torch.nn.Module()
    det.roi_heads = h
    assert set(det.state_dict()) == {k for k in ckpt if k.startswith("roi_heads.")}


def test_registry_and_builder():
    assert "StandardROIHeads" in amd.ROI_HEADS_REGISTRY and amd.ROI_HEADS_REGISTRY.get("StandardROIHeads") is amd.StandardROIHeads
    with pytest.raises(amd.AfiError, match=r"ROI_HEADS\.NAME 'CascadeROIHeads'"):
        amd.build_roi_heads(_cfg({"ROI_HEADS": {"NAME": "CascadeROIHeads"}}), _shapes())
    with pytest.raises(amd.AfiError, match=r"ROI_HEADS\.NAME 'Res5ROIHeads'"):
        amd.StandardROIHeads(_cfg({"ROI_HEADS": {"NAME": "Res5ROIHeads"}}), _shapes())


def test_reference_style_yaml_sections_merge():
    cfg = amd.get_cfg()
    if not hasattr(cfg, "merge_from_dict"):
        pytest.skip("a yacs CfgNode: detectron2's own defaults apply")
    cfg.merge_from_dict({"MODEL": dict(R50_FPN, MASK_ON=True), "TEST": {"DETECTIONS_PER_IMAGE": 100}})
    assert cfg.MODEL.ROI_MASK_HEAD.NUM_CONV == 4 and cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION == 7 and cfg.MODEL.MASK_ON is True
    with pytest.raises(KeyError, match="NO_SUCH_KEY"):
        cfg.merge_from_dict({"MODEL": {"ROI_BOX_HEAD": {"NO_SUCH_KEY": 1}}})


@pytest.mark.parametrize("model,test,match", [
    ({"MASK_ON": True}, None, r"box branch only; set MODEL\.MASK_ON False"),
    ({"KEYPOINT_ON": True}, None, r"MODEL\.KEYPOINT_ON"),
    ({"ROI_BOX_HEAD": {"NUM_CONV": 4}}, None, r"ROI_BOX_HEAD\.NUM_CONV 4"),
    ({"ROI_BOX_HEAD": {"NORM": "SyncBN"}}, None, r"ROI_BOX_HEAD\.NORM 'SyncBN'"),
    ({"ROI_BOX_HEAD": {"NUM_FC": 0}}, None, r"ROI_BOX_HEAD\.NUM_FC 0"),
    ({"ROI_BOX_HEAD": {"POOLER_TYPE": "ROIPool"}}, None, r"ROI_BOX_HEAD\.POOLER_TYPE 'ROIPool'"),
    ({"ROI_BOX_HEAD": {"POOLER_TYPE": "ROIAlign"}}, None, r"POOLER_TYPE 'ROIAlign'"),
    ({"ROI_BOX_HEAD": {"POOLER_RESOLUTION": 15}}, None, r"POOLER_RESOLUTION 15"),
    ({"ROI_BOX_HEAD": {"NAME": "MyHead"}}, None, r"ROI_BOX_HEAD\.NAME 'MyHead'"),
    ({"ROI_HEADS": {"IN_FEATURES": ["p2", "p9"]}}, None, r"ROI_HEADS\.IN_FEATURES"),
    (None, {"DETECTIONS_PER_IMAGE": 1025}, r"TEST\.DETECTIONS_PER_IMAGE 1025.*1024"),
])
def test_unsupported_configs_raise(model, test, match):
    with pytest.raises(amd.AfiError, match=match):
        amd.build_roi_heads(_cfg(model, test), _shapes())


def test_mixed_channels_and_bad_strides_raise():
    sh = _shapes()
    sh["p3"] = ShapeSpec(channels=128, stride=8)
    with pytest.raises(amd.AfiError, match="one channel count"):
        amd.build_roi_heads(_cfg(), sh)
    sh = _shapes()
    sh["p3"] = ShapeSpec(channels=256, stride=16)
    with pytest.raises(amd.AfiError, match="consecutive powers of two"):
        amd.build_roi_heads(_cfg(), sh)


def test_call_time_refusals():
    h = amd.build_roi_heads(_cfg({"ROI_HEADS": {"IN_FEATURES": ["p2"]}}), _shapes(channels=8)).eval()
    images = type("Images", (), {"image_sizes": [(32, 32)], "__len__": lambda s: 1})()
    x = torch.zeros((1, 8, 8, 8))
    with pytest.raises(amd.AfiError, match="targets given"):
        h(images, {"p2": x}, [], targets=[None])
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        h(images, {"p2": x}, [])
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        h.box_features({"p2": x}, torch.zeros((1, 1, 4)), torch.ones((1,), dtype=torch.int32))
    with pytest.raises(amd.AfiError, match="features .* are missing"):
        h(images, {"p3": x}, [])
    h.train()
    with pytest.raises(amd.AfiError, match="inference-only"):
        h(images, {"p2": x}, [])
    with pytest.raises(amd.AfiError, match="inference-only"):
        h.forward_with_given_boxes({"p2": x}, [])
    h.eval()
    inst = [object()]
    assert h.forward_with_given_boxes({"p2": x}, inst) is inst
    from afigan_amd.roi_heads import _check_feature
    with pytest.raises(amd.AfiError, match=r"torch\.bfloat16; fp32 only"):
        _check_feature("roi_heads", "feature p2", _FakeCuda(torch.bfloat16))


class _FakeCuda:
    """What _check_feature reads of a tensor: is_cuda and dtype (a 2-byte GPU tensor cannot be made without a GPU)."""
    is_cuda = True

    def __init__(self, dtype):
        self.dtype = dtype


# ------------------------------------------------------------------------------------------------ the checker against scalar restatements
def test_levels_by_hand():
    b = np.array([[0, 0, 112, 112], [0, 0, 224, 224], [0, 0, 448, 448], [10, 10, 10 + 111.9, 10 + 112], [0, 0, 224, 224.1], [0, 0, 900, 900],
                  [5, 5, 6, 6], [5, 5, 5, 9], [9, 5, 5, 9], [0, 0, 56, 224]], np.float32)
    assert Q.level_of(b, 2, 5).tolist() == [3, 4, 5, 2, 4, 5, 2, 2, 2, 3]
    assert Q.level_of(b, 3, 4).tolist() == [3, 4, 4, 3, 4, 4, 3, 3, 3, 3]
    assert Q.level_of(b[:3], 0, 9).tolist() == [3, 4, 5]


def _bilinear_scalar(f, y, x):
    """detectron2's bilinear_interpolate on one [H, W] map, written out for one point."""
    H, W = f.shape
    if y < -1.0 or y > H or x < -1.0 or x > W:
        return 0.0, 0.0
    y, x = max(y, 0.0), max(x, 0.0)
    y_low, x_low = int(y), int(x)
    if y_low >= H - 1:
        y_high = y_low = H - 1
        y = float(y_low)
    else:
        y_high = y_low + 1
    if x_low >= W - 1:
        x_high = x_low = W - 1
        x = float(x_low)
    else:
        x_high = x_low + 1
    ly, lx = y - y_low, x - x_low
    hy, hx = 1.0 - ly, 1.0 - lx
    terms = (hy * hx * f[y_low, x_low], hy * lx * f[y_low, x_high], ly * hx * f[y_high, x_low], ly * lx * f[y_high, x_high])
    return sum(terms), sum(abs(t) for t in terms)


def _roi_align_scalar(levels, min_level, boxes, counts, S, sr):
    """ROIAlignV2 (aligned) sample by sample: a different program from roi_f64.roi_align's separable matrices."""
    N, P = boxes.shape[:2]
    C = levels[0].shape[1]
    out, ab = np.zeros((N * P, C, S, S)), np.zeros((N * P, C, S, S))
    for n in range(N):
        for j in range(counts[n]):
            x1, y1, x2, y2 = (float(v) for v in boxes[n, j])
            if not (x2 - x1 > 0 and y2 - y1 > 0):
                continue
            lvl = min(max(math.floor(4 + math.log2(math.sqrt((x2 - x1) * (y2 - y1)) / 224)), min_level), min_level + len(levels) - 1)
            f = levels[lvl - min_level][n].astype(np.float64)
            sc = 1.0 / 2 ** lvl
            rw, rh = (x2 - x1) * sc, (y2 - y1) * sc
            gh = sr if sr > 0 else math.ceil(rh / S)
            gw = sr if sr > 0 else math.ceil(rw / S)
            for ph in range(S):
                for pw in range(S):
                    for iy in range(gh):
                        y = y1 * sc - 0.5 + ph * (rh / S) + (iy + 0.5) * (rh / S) / gh
                        for ix in range(gw):
                            x = x1 * sc - 0.5 + pw * (rw / S) + (ix + 0.5) * (rw / S) / gw
                            for c in range(C):
                                v, a = _bilinear_scalar(f[c], y, x)
                                out[n * P + j, c, ph, pw] += v / max(gh * gw, 1)
                                ab[n * P + j, c, ph, pw] += a / max(gh * gw, 1)
    return out, ab


@pytest.mark.parametrize("S,sr", [(7, 0), (2, 0), (2, 2)])
def test_roi_align_checker_against_the_sample_loop(S, sr):
    g = np.random.RandomState(1)
    levels = [g.randn(2, 2, h, w).astype(np.float32) for h, w in Q.ALIGN_LEVELS]
    boxes = Q.align_boxes()[:, :18]
    counts = [18, 15]
    got, gab, terms = Q.roi_align(levels, Q.ALIGN_MIN_LEVEL, boxes, counts, S, sr)
    want, wab = _roi_align_scalar(levels, Q.ALIGN_MIN_LEVEL, boxes, counts, S, sr)
    assert np.abs(got - want).max() <= 1e-12 and np.abs(gab - wab).max() <= 1e-12
    assert not got[15 + 18:].any() and got[:18].any()
    assert not got[7].any() and not got[8].any() and terms[7] == 0, "a zero-width / negative-width box pools to zeros"
    if sr == 0:
        assert terms[9] == 4 * math.ceil(14 / S) * math.ceil(21.5 / 4 / S)


@pytest.mark.parametrize("S,sr", [(7, 0), (2, 0), (7, 2), (2, 2)])
def test_align_inputs_meet_the_gpu_tests_conditions(S, sr):
    """Apart from the exact cases built on purpose, no box has 4 + log2(s / 224) or roi / S within 1e-6 of an integer."""
    b = Q.align_boxes()
    assert Q.align_facts(b, S, sr, Q.ALIGN_MIN_LEVEL, Q.ALIGN_MIN_LEVEL + len(Q.ALIGN_LEVELS) - 1) > 1e-6
    lv = Q.level_of(b.reshape(-1, 4), 2, 5)
    assert set(lv.tolist()) == {2, 3, 4, 5}, "every level is used"
    big = np.array([[[0, 0, 160, 160]]], np.float32)
    assert Q.grid_of(big[0, 0].astype(np.float64), 2, 7, 0)[:2] == (6, 6)


def _nms_pairwise(boxes, cls, valid, thresh):
    keep = []
    for i in range(len(boxes)):
        if not valid[i]:
            continue
        ok = True
        for j in keep:
            if cls[i] != cls[j]:
                continue
            a, b = boxes[i].astype(np.float64), boxes[j].astype(np.float64)
            iw, ih = max(min(a[2], b[2]) - max(a[0], b[0]), 0), max(min(a[3], b[3]) - max(a[1], b[1]), 0)
            u = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - iw * ih
            if u > 0 and iw * ih / u > thresh:
                ok = False
                break
        if ok:
            keep.append(i)
    out = np.zeros(len(boxes), bool)
    out[keep] = True
    return out


@pytest.mark.parametrize("n", Q.NMS_SIZES)
@pytest.mark.parametrize("thresh", Q.NMS_THRESHOLDS)
@pytest.mark.parametrize("nclass", Q.NMS_CLASS_COUNTS)
def test_nms_inputs_and_checker(n, thresh, nclass):
    boxes, cls = Q.nms_class_case(n, nclass)
    valid = np.ones(n, bool)
    valid[3::17] = False
    got = Q.nms_classes(boxes, cls, valid, thresh)
    assert np.array_equal(got, _nms_pairwise(boxes, cls, valid, thresh))
    if n >= 2:
        ambiguous, frac = Q.nms_class_facts(boxes, cls, thresh)
        assert ambiguous == 0 and 0.1 <= frac <= 0.9, (ambiguous, frac)
    if nclass == 1 and n:
        assert np.array_equal(got, R.nms(boxes, valid, thresh)), "one class: the RPN's NMS"


def test_different_classes_do_not_suppress():
    b = np.array([[0, 0, 10, 10], [1, 1, 11, 11], [0, 0, 10, 10]], np.float32)
    assert Q.nms_classes(b, [0, 1, 0], [1, 1, 1], 0.5).tolist() == [True, True, False]


def test_scores_candidates_pick_checkers():
    g = np.random.RandomState(2)
    K, P = 3, 7
    pred = g.randn(2 * P, 16).astype(np.float32) * 3
    pred[4, 1] = np.nan
    props = np.abs(g.randn(2, P, 4)).astype(np.float32) * 10
    props[..., 2:] += props[..., :2] + 1
    sc, bx, _ = Q.scores_boxes(pred, K, False, props, [5, 7], [(40, 50), (30, 30)], (10, 10, 5, 5))
    assert sc.shape == (2, P, K) and bx.shape == (2, P, K, 4)
    t = torch.softmax(torch.from_numpy(pred[:, :K + 1]).double(), 1)[:, :K].numpy().reshape(2, P, K)
    assert np.allclose(sc[0, :4], t[0, :4], rtol=1e-12, atol=0) and np.isnan(sc[0, 4]).all() and np.isinf(sc[0, 5:]).all()
    assert bx[0, :5, :, 0::2].max() <= 50 and bx[0, :5, :, 1::2].max() <= 40 and bx.min() >= 0 and not bx[0, 5:].any()
    q = np.round(sc[1].astype(np.float32) * 8) / 8                                # ties
    idx, valid, n_over = Q.candidates(q, 0.2, 10)
    flat = q.reshape(-1)
    assert len(idx) == 10 and n_over == int((flat > 0.2).sum()) and np.array_equal(valid, flat[idx] > 0.2)
    key = sorted(range(flat.size), key=lambda i: (-flat[i], i))[:10]
    assert idx.tolist() == key
    pos, trunc = Q.pick(np.array([1, 0, 1, 1, 0, 1], bool), 7, 6, 3)
    assert pos.tolist() == [0, 2, 3] and trunc is False
    pos, trunc = Q.pick(np.array([1, 0, 1, 0, 0, 0], bool), 7, 6, 3)
    assert pos.tolist() == [0, 2] and trunc is True
    assert Q.pick(np.array([1, 0, 1, 0, 0, 0], bool), 6, 6, 3)[1] is False


def test_box_head_checker_flattens_in_detectron2s_order():
    h = amd.build_roi_heads(_cfg({"ROI_HEADS": {"IN_FEATURES": ["p2"], "NUM_CLASSES": 3}, "ROI_BOX_HEAD": {"FC_DIM": 8, "POOLER_RESOLUTION": 2}}),
                            _shapes(channels=4))
    g = torch.Generator().manual_seed(3)
    x = torch.randn((5, 4, 2, 2), generator=g)
    acts, logits, deltas = Q.box_head(x, h.state_dict())
    a = torch.relu(h.box_head.fc1(x.flatten(1)))
    a2 = torch.relu(h.box_head.fc2(a))
    assert torch.allclose(acts[1].float(), a2, atol=1e-5) and logits.shape == (5, 4) and deltas.shape == (5, 12)
    assert torch.allclose(logits.float(), h.box_predictor.cls_score(a2), atol=1e-5)
    # the permuted fc1 weight the kernels read gives the same product on the [S][S][C] memory order
    w1, wp, bp = h._prepare()
    assert torch.allclose(x.permute(0, 2, 3, 1).reshape(5, -1) @ w1.t(), x.flatten(1) @ h.box_head.fc1.weight.t(), atol=1e-5)
    assert wp.shape == (16, 8) and torch.equal(wp[:4], h.box_predictor.cls_score.weight) and torch.equal(wp[4:], h.box_predictor.bbox_pred.weight)
    k0 = h._prep_key
    h.box_head.fc1.weight.mul_(2.0)
    w1b, _, _ = h._prepare()
    assert h._prep_key != k0 and torch.equal(w1b, 2.0 * w1)
