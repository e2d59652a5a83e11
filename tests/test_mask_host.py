"""CPU-side checks of the frozen mask branch of StandardROIHeads (afigan_amd/roi_heads.py): detectron2's key names and shapes and a strict load of
a detector checkpoint's ``roi_heads.*`` tensors with box and mask keys, the opt-in keyword and every refusal by its message, tests/mask_f64.py --
the fp64 yardstick of test_gpu_mask.py -- against torch's own fp64 operators and against scalar restatements written differently, the prepared
deconv weight, the extractor's postprocess, and the GPU tests' seeded inputs held to the conditions those tests assert."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import afigan_amd as amd
from afigan_amd.fpn_sr import ShapeSpec

import mask_f64 as Q

FEATURES = ["p2", "p3", "p4", "p5"]
R50_FPN = {"MASK_ON": True, "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": FEATURES},
           "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "POOLER_RESOLUTION": 7},
           "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": 4, "POOLER_RESOLUTION": 14}}     # the base yaml's sections


def _cfg(model=None):
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict(R50_FPN)
    for sec, d in (model or {}).items():
        if isinstance(d, dict):
            getattr(cfg.MODEL, sec).merge_from_dict(d)
        else:
            setattr(cfg.MODEL, sec, d)
    return cfg


def _shapes(channels=256, names=("p2", "p3", "p4", "p5", "p6")):
    return {f: ShapeSpec(channels=channels, stride=2 ** int(f[1:])) for f in names}


# ------------------------------------------------------------------------------------------------ construction and refusals
MASK_KEYS = dict([(f"mask_head.mask_fcn{i}.weight", (256, 256, 3, 3)) for i in range(1, 5)] + [(f"mask_head.mask_fcn{i}.bias", (256,)) for i in range(1, 5)]
                 + [("mask_head.deconv.weight", (256, 256, 2, 2)), ("mask_head.deconv.bias", (256,)),
                    ("mask_head.predictor.weight", (80, 256, 1, 1)), ("mask_head.predictor.bias", (80,))])


def test_key_names_shapes_and_frozen_parameters():
    h = amd.build_roi_heads(_cfg(), _shapes(), masks=True)
    assert isinstance(h, amd.StandardROIHeads) and h.mask_on and isinstance(h.mask_head, amd.MaskRCNNConvUpsampleHead)
    sd = {k: tuple(v.shape) for k, v in h.state_dict().items()}
    assert {k: v for k, v in sd.items() if k.startswith("mask_head.")} == MASK_KEYS
    assert {k.split(".")[0] for k in sd} == {"box_head", "box_predictor", "mask_head"} and len(sd) == 8 + 12
    assert all(not p.requires_grad for p in h.parameters())
    assert (h.mask_pooler.output_size, h.mask_pooler.sampling_ratio, h.mask_pooler.min_level, h.mask_pooler.max_level) == (14, 0, 2, 5)
    assert h.box_pooler.output_size == 7
    # detectron2's initialisation: zero biases, a predictor of std 0.001, msra-filled convs
    assert not any(v.any() for k, v in h.state_dict().items() if k.startswith("mask_head.") and k.endswith("bias"))
    assert 0.0005 < float(h.mask_head.predictor.weight.std()) < 0.002
    assert 0.7 < float(h.mask_head.mask_fcn2.weight.std()) / math.sqrt(2.0 / (256 * 9)) < 1.3
    direct = amd.StandardROIHeads(_cfg(), _shapes(), masks=True)
    assert set(direct.state_dict()) == set(sd)
    ag = amd.build_roi_heads(_cfg({"ROI_MASK_HEAD": {"CLS_AGNOSTIC_MASK": True, "NUM_CONV": 0, "CONV_DIM": 64, "POOLER_RESOLUTION": 7}}), _shapes(),
                             masks=True)
    sda = {k: tuple(v.shape) for k, v in ag.state_dict().items() if k.startswith("mask_head.")}
    assert sda == {"mask_head.deconv.weight": (256, 64, 2, 2), "mask_head.deconv.bias": (64,), "mask_head.predictor.weight": (1, 64, 1, 1),
                   "mask_head.predictor.bias": (1,)}


def test_detector_checkpoint_with_box_and_mask_keys_loads_strictly():
    src = amd.build_roi_heads(_cfg(), _shapes(), masks=True)
    g = torch.Generator().manual_seed(0)
    ckpt = {"roi_heads." + k: torch.randn(v.shape, generator=g) for k, v in src.state_dict().items()}
    ckpt["proposal_generator.rpn_head.conv.bias"] = torch.zeros(1)
    assert any(k.startswith("roi_heads.mask_head.") for k in ckpt) and any(k.startswith("roi_heads.box_head.") for k in ckpt)
    h = amd.build_roi_heads(_cfg(), _shapes(), masks=True)
    res = h.load_state_dict({k[len("roi_heads."):]: v for k, v in ckpt.items() if k.startswith("roi_heads.")}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, ckpt["roi_heads." + k]) for k, v in h.state_dict().items())
    assert all(not p.requires_grad for p in h.parameters())
    # the box-only heads have nowhere to put the mask keys
    box_only = amd.build_roi_heads(_cfg({"MASK_ON": False}), _shapes())
    with pytest.raises(RuntimeError, match="mask_head"):
        box_only.load_state_dict({k[len("roi_heads."):]: v for k, v in ckpt.items() if k.startswith("roi_heads.")}, strict=True)


def test_opt_in_keyword():
    with pytest.raises(amd.AfiError, match=r"box branch only; set MODEL\.MASK_ON False"):
        amd.build_roi_heads(_cfg(), _shapes())
    with pytest.raises(amd.AfiError, match=r"box branch only; set MODEL\.MASK_ON False.*masks=True"):
        amd.StandardROIHeads(_cfg(), _shapes())
    for build in (amd.build_roi_heads, amd.StandardROIHeads):
        with pytest.raises(amd.AfiError, match=r"masks=True.*MODEL\.MASK_ON"):
            build(_cfg({"MASK_ON": False}), _shapes(), masks=True)
    with pytest.raises(amd.AfiError, match=r"MODEL\.KEYPOINT_ON"):
        amd.build_roi_heads(_cfg({"KEYPOINT_ON": True}), _shapes(), masks=True)
    box_only = amd.build_roi_heads(_cfg({"MASK_ON": False}), _shapes(channels=8)).eval()
    assert not box_only.mask_on and not hasattr(box_only, "mask_head")
    inst = [object()]
    assert box_only.forward_with_given_boxes({"p2": torch.zeros((1, 8, 8, 8))}, inst) is inst
    with pytest.raises(amd.AfiError, match="without the mask branch"):
        box_only.mask_head_forward(None, None, None)


@pytest.mark.parametrize("model,match", [
    ({"ROI_MASK_HEAD": {"NAME": "MaskRCNNConvHead"}}, r"ROI_MASK_HEAD\.NAME 'MaskRCNNConvHead'"),
    ({"ROI_MASK_HEAD": {"NORM": "SyncBN"}}, r"ROI_MASK_HEAD\.NORM 'SyncBN'"),
    ({"ROI_MASK_HEAD": {"POOLER_TYPE": "ROIAlign"}}, r"ROI_MASK_HEAD\.POOLER_TYPE 'ROIAlign'"),
    ({"ROI_MASK_HEAD": {"POOLER_TYPE": "ROIPool"}}, r"ROI_MASK_HEAD\.POOLER_TYPE 'ROIPool'"),
    ({"ROI_MASK_HEAD": {"POOLER_RESOLUTION": 15}}, r"ROI_MASK_HEAD\.POOLER_RESOLUTION 15"),
    ({"ROI_MASK_HEAD": {"POOLER_RESOLUTION": 0}}, r"ROI_MASK_HEAD\.POOLER_RESOLUTION 0"),
    ({"ROI_MASK_HEAD": {"POOLER_RESOLUTION": (14, 7)}}, r"ROI_MASK_HEAD\.POOLER_RESOLUTION .* must be square"),
    ({"ROI_MASK_HEAD": {"CONV_DIM": 0}}, r"ROI_MASK_HEAD\.CONV_DIM 0"),
    ({"ROI_MASK_HEAD": {"CONV_DIM": 130}}, r"ROI_MASK_HEAD\.CONV_DIM 130"),
    ({"ROI_MASK_HEAD": {"NUM_CONV": -1}}, r"ROI_MASK_HEAD\.NUM_CONV -1"),
    ({"ROI_BOX_HEAD": {"POOLER_TYPE": "ROIPool"}}, r"ROI_BOX_HEAD\.POOLER_TYPE 'ROIPool'"),
])
def test_unsupported_mask_configs_raise(model, match):
    with pytest.raises(amd.AfiError, match=match):
        amd.build_roi_heads(_cfg(model), _shapes(), masks=True)


def test_wrappers_and_paste_refuse_cpu_tensors():
    from afigan_amd import ops
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        ops.mask_paste(torch.zeros((1, 28, 28)), torch.zeros((1, 4)), (8, 8))
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        ops.roi_mask_probs(torch.zeros((1, 16, 2, 2)), torch.zeros((3, 4)), torch.zeros(3), torch.zeros((1, 1), dtype=torch.int32),
                           torch.ones(1, dtype=torch.int32))
    with pytest.raises(amd.AfiError, match="GPU"):
        amd.paste_masks_in_image(torch.zeros((1, 28, 28)), torch.zeros((1, 4)), (8, 8))


# ------------------------------------------------------------------------------------------------ the checker against other restatements
def test_deconv_checker_and_prepared_weight_against_conv_transpose():
    from afigan_amd.roi_heads import deconv_as_conv1x1
    g = torch.Generator().manual_seed(1)
    R, Cin, Cout, S = 3, 8, 12, 5
    x = torch.randn((R, Cin, S, S), generator=g, dtype=torch.float64)
    w = torch.randn((Cin, Cout, 2, 2), generator=g, dtype=torch.float64)
    b = torch.randn((Cout,), generator=g, dtype=torch.float64)
    up = torch.relu(F.conv_transpose2d(x, w, b, stride=2))
    ph = Q.deconv_phases(x, w, b)
    assert ph.shape == (R, 4 * Cout, S, S)
    for a in (0, 1):
        for c in (0, 1):
            for co in (0, 5, Cout - 1):
                assert torch.equal(ph[:, (2 * a + c) * Cout + co], up[:, co, a::2, c::2])
    # the prepared weight: one 1x1 conv over [4 Cout, Cin] gives that layout
    w1, b1 = deconv_as_conv1x1(w.float(), b.float())
    assert w1.shape == (4 * Cout, Cin) and b1.shape == (4 * Cout,) and w1.is_contiguous()
    for a in (0, 1):
        for c in (0, 1):
            assert torch.equal(w1[(2 * a + c) * Cout:(2 * a + c + 1) * Cout], w.float()[:, :, a, c].t())
    got = torch.relu(F.conv2d(x, w1.double()[:, :, None, None], b1.double()))
    assert torch.allclose(got, Q.deconv_phases(x, w.float(), b.float()), rtol=0, atol=1e-12)


def test_conv_and_logit_checkers_against_scalar_restatements():
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 3, 4, 4), generator=g, dtype=torch.float64)
    w = torch.randn((5, 3, 3, 3), generator=g, dtype=torch.float64)
    b = torch.randn((5,), generator=g, dtype=torch.float64)
    got = Q.conv_relu(x, w, b)
    for r, o, y, xx in ((0, 0, 0, 0), (1, 4, 3, 3), (0, 2, 1, 2), (1, 1, 0, 3)):
        s = float(b[o])
        for ci in range(3):
            for dy in range(3):
                for dx in range(3):
                    yy, xc = y + dy - 1, xx + dx - 1
                    if 0 <= yy < 4 and 0 <= xc < 4:
                        s += float(w[o, ci, dy, dx]) * float(x[r, ci, yy, xc])
        assert abs(float(got[r, o, y, xx]) - max(s, 0.0)) < 1e-12
    C, S, Km = 8, 3, 3
    h, wp, bp, cls = Q.probs_case(C, S, Km)
    cls = cls.copy()
    cls[1, 1] = Km                                           # out of range: not live
    z, mag, live = Q.selected_logits(h, wp, bp, cls, (5, 3))
    assert live.tolist() == [True] * 5 + [True, False, True, False, False]
    assert not z[6].any() and not z[8:].any()
    for r, oy, ox in ((0, 0, 0), (4, 5, 2), (7, 3, 4), (5, 1, 1)):
        c = int(cls[r // 5, r % 5])
        y, a, x, e = oy // 2, oy % 2, ox // 2, ox % 2
        s = float(bp[c]) + sum(float(wp[c, k]) * float(h[r, (2 * a + e) * C + k, y, x]) for k in range(C))
        assert abs(z[r, oy, ox] - s) < 1e-12 and mag[r, oy, ox] >= abs(s) - 1e-12
    assert np.allclose(Q.sigmoid(z), torch.sigmoid(torch.from_numpy(z)).numpy(), rtol=1e-15, atol=0)
    z1, _, live1 = Q.selected_logits(h, wp[:1], bp[:1], cls, (5, 3))          # Km == 1: channel 0 whatever the class says
    assert live1.tolist() == [True] * 8 + [False] * 2 and z1[6].any()


def _grid_sample_value(probs, boxes, H, W):
    """detectron2's paste over the whole image with torch's own operator on double tensors."""
    m = torch.from_numpy(np.asarray(probs, np.float32)).double()
    b = torch.from_numpy(np.asarray(boxes, np.float32)).double()
    ys = torch.arange(H, dtype=torch.float64) + 0.5
    xs = torch.arange(W, dtype=torch.float64) + 0.5
    gy = (ys[None] - b[:, 1:2]) / (b[:, 3:4] - b[:, 1:2]) * 2 - 1
    gx = (xs[None] - b[:, 0:1]) / (b[:, 2:3] - b[:, 0:1]) * 2 - 1
    grid = torch.stack([gx[:, None, :].expand(-1, H, -1), gy[:, :, None].expand(-1, -1, W)], -1)
    return F.grid_sample(m[:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0].numpy()


def _scalar_paste(m, box, y, x):
    """One pixel, written from the semantics with explicit taps."""
    M = m.shape[0]
    x0, y0, x1, y1 = (float(np.float32(t)) for t in box)
    ix = (((x + 0.5 - x0) / (x1 - x0) * 2 - 1 + 1) * M - 1) / 2
    iy = (((y + 0.5 - y0) / (y1 - y0) * 2 - 1 + 1) * M - 1) / 2
    fx, fy = math.floor(ix), math.floor(iy)
    v = 0.0
    for ty, wy in ((fy, 1 - (iy - fy)), (fy + 1, iy - fy)):
        for tx, wx in ((fx, 1 - (ix - fx)), (fx + 1, ix - fx)):
            if 0 <= ty < M and 0 <= tx < M:
                v += wy * wx * float(m[ty, tx])
    return v, (x0 <= x + 0.5 <= x1) and (y0 <= y + 0.5 <= y1)


@pytest.mark.parametrize("H,W,M", Q.PASTE_CASES)
def test_paste_checker_and_seeded_inputs(H, W, M):
    probs, boxes = Q.paste_case(H, W, M)
    R = len(boxes)
    assert probs.shape == (R, M, M) and probs.min() >= 0 and probs.max() <= 1
    v, e, inside = Q.paste(probs, boxes, H, W)
    ok = (boxes[:, 2] - boxes[:, 0] > 0) & (boxes[:, 3] - boxes[:, 1] > 0)
    assert (~ok).sum() == 3 and not v[~ok].any() and not inside[~ok].any()
    ref = _grid_sample_value(probs[ok], boxes[ok], H, W)
    assert np.abs(v[ok] - ref).max() < 1e-12, "the checker differs from grid_sample on double tensors"
    r = np.random.RandomState(0)
    for _ in range(60):
        i, y, x = r.randint(R), r.randint(H), r.randint(W)
        if ok[i]:
            sv, sin = _scalar_paste(probs[i].astype(np.float64), boxes[i], y, x)
            assert abs(sv - v[i, y, x]) < 1e-12 and sin == bool(inside[i, y, x])
    # the conditions the GPU test asserts: the kinds of boxes and masks are all there, and few inside pixels are undecided
    w, hgt = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    assert (w > 2 * 28).any() and ((w > 0) & (w < 1) & (hgt < 1)).sum() >= 2 and (w == 0).any() and (w < 0).any()
    assert (boxes[:, 0] < 0).any() and (boxes[:, 1] < 0).any() and (boxes[:, 2] > W).any() and (boxes[:, 3] > H).any()
    assert ((boxes[:, 0] == 0) & ok).any() and ((boxes[:, 2] == W) & ok).any()
    kinds = [set(np.unique(p)) for p in probs]
    assert any(k == {0.0} for k in kinds) and any(k == {1.0} for k in kinds) and any(k == {0.0, 1.0} for k in kinds) and any(len(k) > M * M // 2 for k in kinds)
    assert not any(k == {0.5} for k in kinds)
    want, sure = Q.paste_decided(v, e, inside)
    left_out = int((~sure).sum())
    assert inside.sum() > 500 and left_out <= Q.PASTE_LEFT_OUT * inside.sum(), (left_out, int(inside.sum()))
    assert want.any() and (inside & ~want).any()
    # a pixel whose centre is outside its box cannot reach 0.5 (the reason the kernel may skip it)
    assert v[~inside].max() <= 0.5 + 1e-12
    print(f"[mask paste inputs] {H}x{W} M {M}: {R} boxes, {int(inside.sum())} inside pixels, {left_out} undecided, {int(want.sum())} set")


@pytest.mark.parametrize("Km", [80, 3, 1])
def test_predictor_seeded_inputs(Km):
    for C, S in ((8, 14), (256, 3)):
        h, w, b, cls = Q.probs_case(C, S, Km)
        assert h.shape == (10, 4 * C, S, S) and w.shape == (Km, C) and cls.shape == (2, 5) and cls.dtype == np.int32
        assert cls.min() == 0 and cls.max() == Km - 1
        for counts in Q.PROBS_COUNTS:
            z, mag, live = Q.selected_logits(h, w, b, cls, counts)
            assert live.sum() == sum(counts) and np.abs(z[live]).max() > 1.0
            seen = {int(cls[r // 5, r % 5]) for r in np.nonzero(live)[0]}
            assert sum(counts) == 5 or {0, Km - 1} <= seen


# ------------------------------------------------------------------------------------------------ the extractor's postprocess
def test_postprocess_without_masks_is_unchanged_and_cpu_masks_raise():
    from afigan_amd.rcnn_extractor import _detector_postprocess_boxes
    from afigan_amd.roi_heads import Detections
    from afigan_amd.rpn import Boxes
    b = torch.tensor([[1.0, 2.0, 11.0, 12.0], [5.0, 5.0, 5.0, 9.0], [30.0, 10.0, 50.0, 40.0]])
    d = Detections((40, 50), Boxes(b), torch.tensor([0.9, 0.8, 0.7]), torch.tensor([1, 2, 3]))
    assert d.pred_masks is None
    r = _detector_postprocess_boxes(d, 80, 100)
    assert r.image_size == (80, 100) and torch.equal(r.pred_boxes.tensor, torch.tensor([[2.0, 4.0, 22.0, 24.0], [60.0, 20.0, 100.0, 80.0]]))
    assert torch.equal(r.scores, torch.tensor([0.9, 0.7])) and torch.equal(r.pred_classes, torch.tensor([1, 3])) and r.pred_masks is None
    assert torch.equal(d.pred_boxes.tensor, b), "the input was modified"
    d.pred_masks = torch.zeros((3, 1, 28, 28))
    with pytest.raises(amd.AfiError, match=r"pred_masks.*GPU only.*CPU tensor"):
        _detector_postprocess_boxes(d, 80, 100)
    d.pred_masks = None
    d.pred_keypoints = torch.zeros((3, 17, 3))
    with pytest.raises(amd.AfiError, match="pred_keypoints"):
        _detector_postprocess_boxes(d, 80, 100)
    moved = Detections((4, 4), Boxes(b), torch.zeros(3), torch.zeros(3), torch.ones((3, 1, 2, 2))).to("cpu")
    assert torch.equal(moved.pred_masks, torch.ones((3, 1, 2, 2)))


def test_entry_points_check_their_arguments_without_a_device():
    """AFI_ERR_BAD_ARG / AFI_ERR_UNSUPPORTED come back before anything is launched (fake, never dereferenced pointers)."""
    from afigan_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.DEFINES["AFI_ERR_BAD_ARG"], _lib.DEFINES["AFI_ERR_UNSUPPORTED"]
    p = 0x1000
    assert lib.afi_roi_mask_probs(None, p, p, p, p, 1, 1, 8, 14, 3, p, None) == BAD
    assert lib.afi_roi_mask_probs(p, p, p, p, p, 0, 1, 8, 14, 3, p, None) == BAD
    assert lib.afi_roi_mask_probs(p, p, p, p, p, 1, 1, 8, 14, 0, p, None) == BAD
    assert lib.afi_roi_mask_probs(p, p, p, p, p, 1, 1, 6, 14, 3, p, None) == UNS          # C % 4
    assert lib.afi_roi_mask_probs(p, p, p, p, p, 1, 1, 8, 15, 3, p, None) == UNS          # S > 14
    assert lib.afi_roi_mask_probs(p + 4, p, p, p, p, 1, 1, 8, 14, 3, p, None) == UNS      # h not 16-byte aligned
    assert lib.afi_mask_paste(None, p, 1, 28, 8, 8, 0.5, p, None) == BAD
    assert lib.afi_mask_paste(p, p, -1, 28, 8, 8, 0.5, p, None) == BAD
    assert lib.afi_mask_paste(p, p, 1, 0, 8, 8, 0.5, p, None) == BAD
    assert lib.afi_mask_paste(p, p, 1, 28, 8, 0, 0.5, p, None) == BAD
    assert lib.afi_mask_paste(p, p, 1, 65, 8, 8, 0.5, p, None) == UNS                     # M > 64
    assert lib.afi_mask_paste(p, p, 1, 28, 32 * 65536, 8, 0.5, p, None) == UNS            # more than 65535 bands
    assert lib.afi_mask_paste(None, None, 0, 28, 8, 8, 0.5, None, None) == 0              # R = 0 launches nothing
