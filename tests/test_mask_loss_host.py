"""The checker of the mask branch's training side (tests/mask_loss_f64.py) held to things that are not this project's, the refusals of the
Python surface, and the conditions the GPU test's fixtures rely on -- all without a GPU.
  1. the loss and its gradient  F.binary_cross_entropy_with_logits(reduction="mean") and conv_transpose2d autograd in float64;
  2. the target rule            a hand-computed case; the float32 / float64 quotient tells two masks apart; the kinds of rows of the case;
  3. the refusals               gt_masks missing, a bitmask, a wrong length; CascadeROIHeads; trainable_(mask_head=True) flips the mask head;
  4. the end-to-end fixture     >= 4 foreground rows per image on >= 2 levels with >= 2 classes, every target between 10 % and 90 % ones."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import afigan_amd as amd
import mask_f64
import mask_loss_f64 as Q
import roi_f64
import roi_loss_f64 as T

F = np.float32


# ------------------------------------------------------------------------------------------------ 1. loss, dz, dh, dW, db against torch autograd
@pytest.mark.parametrize("name", ["C8_S3_K1", "C12_S5_K3", "logits_of_40", "mtot_zero"])
def test_checker_loss_and_gradients_equal_torch_float64_autograd(name):
    C, S, Km, kw = Q.LOSS_CASES[name]
    h, w, b, cls, counts, tg = Q.loss_case(C, S, Km, **kw)
    r = Q.mask_loss(h, w, b, cls[:, :Q.BF], counts, tg)
    # torch: the deconv's output as an image [R, C, 2S, 2S], a 1x1 conv to Km classes, the row's own class, BCE with logits (mean)
    R = h.shape[0]
    up = torch.tensor(h, dtype=torch.float64).view(R, 2, 2, C, S, S).permute(0, 3, 4, 1, 5, 2).reshape(R, C, 2 * S, 2 * S).requires_grad_(True)
    wt = torch.tensor(w, dtype=torch.float64).view(Km, C, 1, 1).requires_grad_(True)
    bt = torch.tensor(b, dtype=torch.float64).requires_grad_(True)
    logits = Fn.conv2d(up, wt, bt)
    rows = [(n, d) for n in range(Q.N) for d in range(int(counts[n]))]
    if not rows:
        assert r["loss"] == 0.0 and not r["dz"].any() and r["mtot"] == 0
        return
    sel = torch.stack([logits[n * Q.BF + d, 0 if Km == 1 else int(cls[n, d])] for n, d in rows])
    sel.retain_grad()
    t = torch.tensor(np.stack([tg[n, d] for n, d in rows]), dtype=torch.float64)
    loss = Fn.binary_cross_entropy_with_logits(sel, t, reduction="mean")
    loss.backward()
    assert r["mtot"] == len(rows) * 4 * S * S and abs(r["loss"] - loss.item()) <= 1e-12 * abs(loss.item())
    dz = np.stack([r["dz"][n * Q.BF + d] for n, d in rows])
    assert np.abs(dz - sel.grad.numpy()).max() <= 1e-15
    if kw.get("big"):
        assert np.abs(r["z"][r["live"]]).max() > 40 and np.isfinite(r["loss"])
    # the predictor's backward, from dz in the kernel's order
    dzk = r["dz"].reshape(R, S, 2, S, 2).transpose(0, 1, 3, 2, 4).reshape(R, S, S, 4)
    assert np.array_equal(Q.image_order(dzk), r["dz"])
    p = Q.pred_bwd(h, dzk, w, cls[:, :Q.BF], counts)
    assert np.abs(p["dW"] - wt.grad.numpy().reshape(Km, C)).max() <= 1e-12 * max(p["dW_abs"].max(), 1e-30)
    assert np.abs(p["db"] - bt.grad.numpy()).max() <= 1e-12 * max(p["db_abs"].max(), 1e-30)
    dh = torch.tensor(p["dh"]).view(R, 2, 2, C, S, S).permute(0, 3, 4, 1, 5, 2).reshape(R, C, 2 * S, 2 * S)
    want = up.grad * (up > 0)                                     # dh carries the deconv's ReLU mask
    assert (dh - want).abs().max().item() <= 1e-15
    assert p["terms"].sum() == r["mtot"] and (p["dh"][h == 0] == 0).all()


def test_torch_restatement_backpropagates_through_the_deconv_like_conv_transpose2d():
    """deconv_as_conv1x1's [4 Cout, Cin] weight and the 4-phase layout against conv_transpose2d: value and weight gradient, whose permutation
    back to [Cin, Cout, 2, 2] is the one the backward uses."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, 8, 5, 5), generator=g, dtype=torch.float64)
    w = torch.randn((8, 4, 2, 2), generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn((4,), generator=g, dtype=torch.float64).requires_grad_(True)
    up = Fn.conv_transpose2d(x, w, b, stride=2)
    gy = torch.randn(up.shape, generator=g, dtype=torch.float64)
    up.backward(gy)
    w1, b1 = amd.roi_heads.deconv_as_conv1x1(w.float(), b.float())
    w1, b1 = w1.double().requires_grad_(True), b1.double().requires_grad_(True)
    ph = Fn.conv2d(x, w1.view(16, 8, 1, 1), b1)                  # [R, 4 Cout, S, S]
    gph = torch.cat([gy[:, :, a::2, c::2] for a in (0, 1) for c in (0, 1)], 1)
    assert (torch.relu(ph) - mask_f64.deconv_phases(x, w, b)).abs().max() < 1e-6        # the layouts agree (the weight went through fp32)
    ph.backward(gph)
    back = w1.grad.view(2, 2, 4, 8).permute(3, 2, 0, 1)
    assert (back - w.grad).abs().max() < 1e-6 and (b1.grad.view(4, 4).sum(0) - b.grad).abs().max() < 1e-9


# ------------------------------------------------------------------------------------------------ 2. the target rule
def test_target_rule_on_a_hand_computed_case():
    """A 2 x 1 box on a 4 x 4 canvas: rw = 2, rh = 4.  The rectangle (10.5, 20.25) .. (12, 21) maps to X in [1, 4], Y in [1, 4]: every pixel
    whose centre lies in it -- columns 1 .. 3 and rows 1 .. 3 -- is one (rleFrPoly fills x in [1, 4) by centres 1.5, 2.5, 3.5; likewise y)."""
    box = np.array([10, 20, 12, 21], F)
    poly = [[10.5, 20.25, 12.0, 20.25, 12.0, 21.0, 10.5, 21.0]]
    assert Q.ratio(F(2), 4) == 2.0 and Q.ratio(F(1), 4) == 4.0
    tp = Q.transformed(poly, box, 4)
    assert tp[0].tolist() == [1.0, 1.0, 4.0, 1.0, 4.0, 4.0, 1.0, 4.0]
    want = np.zeros((4, 4), bool)
    want[1:4, 1:4] = True
    assert np.array_equal(Q.row_target(poly, box, 4), want)
    # a side below 0.1 uses the float64 quotient M / 0.1, a side of exactly fp32(0.1) (above the double 0.1) the float32 one
    assert Q.ratio(F(0.05), 28) == 28 / 0.1 and Q.ratio(F(0), 28) == 280.0 and Q.ratio(F(-3), 28) == 280.0
    assert float(F(0.1)) > 0.1 and Q.ratio(F(0.1), 28) == float(F(28) / F(0.1)) != 28 / float(F(0.1))
    assert np.isnan(Q.ratio(F("nan"), 28))
    # non-finite and out-of-range transformed coordinates, and an instance without polygons: all zero
    assert not Q.row_target(poly, np.array([10, 20, np.nan, 21], F), 4).any()
    assert not Q.row_target([[0.0, 0.0, 1e9, 0.0, 1e9, 1e9]], np.array([0, 0, 0.01, 0.01], F), 28).any()
    assert Q.row_target([[0.0, 0.0, 1.0, 0.0, 1.0, 1.0]], np.array([0, 0, 0.01, 0.01], F), 28).any()
    assert not Q.row_target([], box, 4).any()


@pytest.mark.parametrize("M", [28, 6])
def test_float32_and_float64_quotients_give_different_masks(M):
    polys, box = Q.split_polygon(M, Q.SPLIT_W[M])
    a, b = Q.row_target(polys, box, M), Q.row_target(polys, box, M, "fp64")
    assert a.any() and b.any() and not np.array_equal(a, b), (a.sum(), b.sum())
    assert Q.ratio(F(3), 6) == Q.ratio(F(3), 6, "fp64")          # 6 / 3 is exact: why M = 6 splits at another width


@pytest.mark.parametrize("M", [28, 6])
def test_target_case_holds_the_rows_it_is_for(M):
    c = Q.target_case(M)
    tg, cfg = Q.targets(c["instances"], c["boxes"], c["sidx"], c["midx"], (Q.BF, Q.BF), c["counts_g"], Q.BF, M)
    k = {name: j for j, name in enumerate(c["kinds"])}
    frac = tg.reshape(Q.N, Q.BF, -1).mean(2)
    assert cfg.tolist() == [Q.BF, Q.BF]
    assert frac[0, k["own_box"]] > 0.5 and 0.2 < frac[0, k["half_outside"]] < 0.6 and frac[0, k["three_polygons"]] > 0.3
    assert not tg[0, k["polygon_outside_box"]].any() and tg[0, k["zero_area"]].all()
    assert tg[0, k["side_below_0.1"]].any() and not tg[0, k["side_below_0.1"]].all() if M == 28 else True
    b = c["boxes"][0]
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    assert w[k["side_below_0.1"]] < 0.1 < h[k["side_below_0.1"]] and w[k["zero_area"]] == 0 == h[k["zero_area"]]
    assert Q.ratio(w[k["square_box"]], M) == Q.ratio(h[k["square_box"]], M) and Q.ratio(w[k["own_box"]], M) != Q.ratio(h[k["own_box"]], M)
    other = Q.targets(c["instances"], c["boxes"], c["sidx"], c["midx"], (Q.BF, Q.BF), c["counts_g"], Q.BF, M, "fp64")[0]
    assert not np.array_equal(other[0, k["split_quotient"]], tg[0, k["split_quotient"]])
    # the union of three polygons differs from each of them; image 1's rows use image 1's instances
    one = Q.row_target(c["instances"][0][1][:1], b[k["three_polygons"]], M)
    assert (tg[0, k["three_polygons"]].astype(bool) & ~one).any()
    assert np.array_equal(tg[1, 0].astype(bool), Q.row_target(c["instances"][1][0], c["boxes"][1, 0], M))
    # n_pos is clamped to 0 .. Bf and the rows past it are zero
    tg2, cfg2 = Q.targets(c["instances"], c["boxes"], c["sidx"], c["midx"], Q.N_POS_CASES["above_and_below"], c["counts_g"], Q.BF, M)
    assert cfg2.tolist() == [Q.BF, 0] and not tg2[1].any() and np.array_equal(tg2[0], tg[0])


# ------------------------------------------------------------------------------------------------ 3. the Python surface
def _cfg(extra=None):
    cfg = amd.get_cfg()
    d = {"MASK_ON": True, "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": ["p2", "p3"], "NUM_CLASSES": 5, "BATCH_SIZE_PER_IMAGE": 32},
         "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 1, "FC_DIM": 16, "POOLER_RESOLUTION": 7},
         "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": 1, "CONV_DIM": 8, "POOLER_RESOLUTION": 7}}
    for k, v in (extra or {}).items():
        d[k] = {**d.get(k, {}), **v} if isinstance(v, dict) else v
    cfg.MODEL.merge_from_dict(d)
    return cfg


def _shapes():
    from afigan_amd.fpn_sr import ShapeSpec
    return {f: ShapeSpec(channels=8, stride=2 ** int(f[1:])) for f in ("p2", "p3")}


def test_gt_masks_refusals_name_the_field():
    h = amd.build_roi_heads(_cfg(), _shapes(), masks=True)
    boxes = torch.tensor([[1.0, 1.0, 9.0, 9.0], [2.0, 2.0, 5.0, 5.0]])
    base = {"gt_boxes": boxes, "gt_classes": torch.tensor([2, 1])}
    tri = [np.array([1.0, 1.0, 9.0, 1.0, 9.0, 9.0])]
    with pytest.raises(amd.AfiError, match="no `gt_masks`"):
        h._target_polygons([base])
    with pytest.raises(amd.AfiError, match="`gt_masks` is a bitmask"):
        h._target_polygons([{**base, "gt_masks": torch.zeros((2, 16, 16), dtype=torch.bool)}])
    with pytest.raises(amd.AfiError, match="`gt_masks` is a bitmask"):
        h._target_polygons([{**base, "gt_masks": type("BitMasks", (), {"tensor": torch.zeros((2, 16, 16), dtype=torch.bool)})()}])
    with pytest.raises(amd.AfiError, match="`gt_masks` has 1 instances and `gt_boxes` 2"):
        h._target_polygons([{**base, "gt_masks": [tri]}])
    with pytest.raises(amd.AfiError, match="`gt_masks` must be"):
        h._target_polygons([{**base, "gt_masks": 7}])
    as_list = h._target_polygons([{**base, "gt_masks": [tri, [torch.tensor([2.0, 2.0, 5.0, 2.0, 5.0, 5.0]), tri[0]]]}])
    as_obj = h._target_polygons([type("T", (), {**base, "gt_masks": type("PolygonMasks", (), {"polygons": [tri, tri + tri]})()})()])
    assert len(as_list[0]) == 2 and len(as_list[0][1]) == 2 and isinstance(as_list[0][1][0], np.ndarray) and len(as_obj[0][1]) == 2
    # the packed form: one annotation per (image, ground-truth slot), the slots past an image's instances empty
    xy, voff, poff = amd.ops.mask_polygons(as_list + [[]], 2, 3, "cpu")
    assert poff.tolist() == [0, 1, 3, 3, 3, 3, 3] and voff.tolist() == [0, 3, 6, 9] and tuple(xy.shape) == (9, 2) and xy.dtype == torch.float64
    with pytest.raises(amd.AfiError, match="3 instances for 2 ground-truth slots"):
        amd.ops.mask_polygons([[tri, tri, tri]], 1, 2, "cpu")
    with pytest.raises(amd.AfiError, match="non-finite"):
        amd.ops.mask_polygons([[[np.array([1.0, np.inf, 2.0, 2.0])]]], 1, 1, "cpu")


def test_training_surface_of_heads_with_masks():
    h = amd.build_roi_heads(_cfg(), _shapes(), masks=True)
    assert h.mask_batch_per_image == 8 and not any(p.requires_grad for p in h.parameters())
    assert h.trainable_(mask_head=True) is h and all(p.requires_grad for p in h.parameters())
    assert not any(p.requires_grad for p in h.trainable_(False, mask_head=True).parameters())
    h.trainable_()                                           # without the keyword the mask head stays as it is: frozen
    assert all(p.requires_grad for p in h.box_head.parameters()) and not any(p.requires_grad for p in h.mask_head.parameters())
    h.trainable_(False)
    plain = amd.build_roi_heads(_cfg({"MASK_ON": False}), _shapes()).trainable_()
    with pytest.raises(amd.AfiError, match="built without the mask branch"):
        plain.trainable_(mask_head=True)
    assert all(p.requires_grad for p in plain.parameters()) and not hasattr(plain, "mask_head")
    images = type("Images", (), {"image_sizes": [(32, 32)], "__len__": lambda s: 1})()
    x = {"p2": torch.zeros((1, 8, 8, 8)), "p3": torch.zeros((1, 8, 4, 4))}
    prop = [type("P", (), {"proposal_boxes": torch.zeros((3, 4))})()]
    tgt = [{"gt_boxes": torch.tensor([[1.0, 1.0, 9.0, 9.0]]), "gt_classes": torch.tensor([2]), "gt_masks": [[[1.0, 1.0, 9.0, 1.0, 9.0, 9.0]]]}]
    with pytest.raises(amd.AfiError, match="CPU tensor"):        # a training call of mask heads reaches the device checks: it is no longer refused
        h.train()(images, x, prop, tgt)
    cas =_cfg({"ROI_HEADS": {"NAME": "CascadeROIHeads"}, "ROI_BOX_HEAD": {"CLS_AGNOSTIC_BBOX_REG": True}})
    c = amd.build_roi_heads(cas, _shapes(), masks=True, cascade=True).train()
    with pytest.raises(amd.AfiError, match="cascade training is out of scope"):
        c(images, x, prop, tgt)
    with pytest.raises(amd.AfiError, match="KEYPOINT_ON"):
        amd.build_roi_heads(_cfg({"KEYPOINT_ON": True}), _shapes(), masks=True)


def test_ops_refuse_wrong_shapes_and_devices():
    z = torch.zeros
    with pytest.raises(amd.AfiError, match=r"mask_targets: dense boxes"):
        amd.ops.mask_targets(z((1, 2), dtype=torch.float64), z(2, dtype=torch.int64), z(3, dtype=torch.int64), z((1, 8, 4)), z((1, 4), dtype=torch.int32),
                             z((1, 9), dtype=torch.int32), z(1, dtype=torch.int32), 2, z(1, dtype=torch.int32), 2, 28)
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        amd.ops.mask_targets(z((1, 2), dtype=torch.float64), z(2, dtype=torch.int64), z(3, dtype=torch.int64), z((1, 8, 4)), z((1, 8), dtype=torch.int32),
                             z((1, 9), dtype=torch.int32), z(1, dtype=torch.int32), 2, z(1, dtype=torch.int32), 2, 28)
    with pytest.raises(amd.AfiError, match=r"mask_targets: Bf 9"):
        amd.ops.mask_targets(z((1, 2), dtype=torch.float64), z(2, dtype=torch.int64), z(3, dtype=torch.int64), z((1, 8, 4)), z((1, 8), dtype=torch.int32),
                             z((1, 9), dtype=torch.int32), z(1, dtype=torch.int32), 2, z(1, dtype=torch.int32), 9, 28)
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        amd.ops.mask_loss(z((2, 32, 3, 3)), z((3, 8)), z(3), z((1, 2), dtype=torch.int32), z(1, dtype=torch.int32), z((1, 2, 6, 6), dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ 4. the end-to-end fixture
def test_e2e_fixture_has_foreground_on_two_levels_with_two_classes_and_mixed_targets():
    case = T.e2e_case()
    inst = Q.e2e_polygons(case)
    a = T.assign(case, 5)
    assert a["n_pos"].tolist() == [Q.BF, Q.BF]
    gmax = 10
    tg, cfg = Q.targets(inst, a["boxes"], a["sidx"], a["midx"], a["n_pos"], np.array([10, 10]), Q.BF, 28)
    for n in range(Q.N):
        fg = a["boxes"][n, :Q.BF].astype(np.float64)
        assert cfg[n] >= 4 and len(set(roi_f64.level_of(fg, T.MIN_LEVEL, T.MIN_LEVEL + 3).tolist())) >= 2, n
        assert len(set(a["cls"][n, :Q.BF].tolist())) >= 2 and (a["cls"][n, :Q.BF] < 5).all(), n
        frac = tg[n].reshape(Q.BF, -1).mean(1)
        assert (frac > 0.1).all() and (frac < 0.9).all(), (n, frac)
    assert gmax == max(len(g) for g in case["gts"])


@pytest.mark.parametrize("channels", [8, 128])
def test_e2e_fixture_decides_every_relu_at_fp32_resolution(channels):
    """No ReLU unit of the float64 restatement lies within 2^-24 (sum |w x| + |b|) of zero: below that one fp32 rounding of a partial sum can
    flip the unit, and one flipped unit of the 128-channel chain moves a weight gradient by 1e-4 relative -- the end-to-end
    comparison would measure the flip, not the kernels."""
    case = T.e2e_case()
    a = T.assign(case, 5)
    tg, cfg = Q.targets(Q.e2e_polygons(case), a["boxes"], a["sidx"], a["midx"], a["n_pos"], np.array([10, 10]), Q.BF, 28)
    h = Q.e2e_heads(amd, channels)
    sd = h.state_dict()
    names = [k for k in sd if k.startswith("mask_head.")]
    assert names == [f"mask_head.{l}.{t}" for l in ("mask_fcn1", "mask_fcn2", "deconv", "predictor") for t in ("weight", "bias")]
    margins = []
    with torch.no_grad():
        loss = Q.torch_mask_loss([v.double() for v in Q.e2e_features(channels).values()], [sd[k].double() for k in names], T.MIN_LEVEL, 14, 2,
                                 a["boxes"][:, :Q.BF], cfg, a["cls"], tg, 5, margins)
    assert len(margins) == 3 and min(margins) > 1.0 and 0.3 < loss.item() < 3.0, (margins, loss.item())
    if channels == 128:                                       # the seed it replaced holds a deconv unit at 0.16 of that distance
        m2 = []
        with torch.no_grad():
            Q.torch_mask_loss([v.double() for v in Q.e2e_features(channels, 2).values()], [sd[k].double() for k in names], T.MIN_LEVEL, 14, 2,
                              a["boxes"][:, :Q.BF], cfg, a["cls"], tg, 5, m2)
        assert min(m2) < 1.0
