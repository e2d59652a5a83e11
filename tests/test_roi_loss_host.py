"""CPU-side checks of the training side of the box branch of StandardROIHeads (afigan_amd/roi_heads.py: StandardROIHeads.losses): the plain-loop
checker tests/roi_loss_f64.py against vectorised torch restatements written differently (IoU matrix and argmax; F.cross_entropy and autograd; a
sample-by-sample bilinear ROIAlign and autograd), the GPU tests' fixtures held to their purpose, the module's refusals by their messages, and the
ROIAlign-backward bar: passed by numpy float32 evaluating the kernel's order, failed by two wrong variants."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import afigan_amd as amd
from afigan_amd.fpn_sr import ShapeSpec

import roi_f64 as Q
import roi_loss_f64 as T
import rpn_loss_f64 as RL

F = np.float32
FEATURES = ["p2", "p3", "p4", "p5"]


def _cfg(model=None):
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": False, "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": FEATURES, "NUM_CLASSES": 5,
                                                               "BATCH_SIZE_PER_IMAGE": 32},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "FC_DIM": 32, "POOLER_RESOLUTION": 7},
                               "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": 1, "CONV_DIM": 8, "POOLER_RESOLUTION": 14}})
    for sec, d in (model or {}).items():
        if isinstance(d, dict):
            getattr(cfg.MODEL, sec).merge_from_dict(d)
        else:
            setattr(cfg.MODEL, sec, d)
    return cfg


def _shapes(channels=8):
    return {f: ShapeSpec(channels=channels, stride=2 ** int(f[1:])) for f in FEATURES}


# ------------------------------------------------------------------------------------------------ the checker against vectorised restatements
def _label_vectorised(cand, gt, thresh):
    """pairwise_iou as one fp32 matrix expression and Matcher's max over the boxes (the first maximum)."""
    if len(gt) == 0:
        return np.zeros(len(cand), np.int8), np.zeros(len(cand), np.int32)
    a, b = torch.tensor(gt), torch.tensor(cand)
    area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, None, 2:], b[None, :, 2:]) - torch.max(a[:, None, :2], b[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    iou = torch.where(inter > 0, inter / (area_a[:, None] + area_b[None, :] - inter), torch.zeros_like(inter)).numpy()
    val = iou.max(0)
    idx = (iou == val[None, :]).argmax(0)                  # the lowest index that reaches the maximum
    return (val >= F(thresh)).astype(np.int8), idx.astype(np.int32)


@pytest.mark.parametrize("name", sorted(T.label_cases()))
@pytest.mark.parametrize("append_gt", [True, False])
def test_label_checker_against_iou_matrix(name, append_gt):
    c = T.label_cases()[name]
    gmax = max(1, max(len(g) for g in c["gts"]))
    pmax = max(len(p) for p in c["proposals"])
    for n, (p, g) in enumerate(zip(c["proposals"], c["gts"])):
        labels, midx = T.label(p, len(p), g, pmax + gmax, c["thresh"], append_gt)
        cand = T.candidates(p, len(p), g, append_gt)
        l2, m2 = _label_vectorised(cand, g, c["thresh"])
        assert np.array_equal(labels[:len(cand)], l2) and np.array_equal(midx[:len(cand)], m2)
        assert (labels[len(cand):] == -1).all() and (midx[len(cand):] == 0).all()
        if append_gt and len(g):
            assert (labels[len(p):len(cand)] == 1).all()   # a ground-truth box matches itself


def test_label_cases_hold_what_they_are_for():
    c = T.label_cases()
    e = c["iou_exactly_and_one_ulp_below"]
    labels, midx = T.label(e["proposals"][0], 3, e["gts"][0], 5, 0.5, False)
    assert RL.iou32(e["gts"][0][0], e["proposals"][0][0]) == F(0.5) and labels[0] == 1
    assert RL.iou32(e["gts"][0][1], e["proposals"][0][2]) == np.nextafter(F(0.5), F(0)) and labels[2] == 0 and midx[2] == 1
    i = c["identical_boxes"]
    labels, midx = T.label(i["proposals"][1], len(i["proposals"][1]), i["gts"][1], 50, 0.5, False)
    assert labels[4] == 1 and midx[4] == 0                # two identical boxes: the lowest index wins
    assert len(c["more_than_one_lds_tile"]["gts"][0]) > 256 and len(c["random"]["proposals"][1]) < T.P
    for name, (labels, keys, batch, fraction) in T.sample_cases().items():
        quota = int(batch * fraction)
        npos, nneg = (labels == 1).sum(1), (labels == 0).sum(1)
        if name == "quota_above_both":
            assert (npos < quota).all() and (nneg < batch - quota).all()
        if name == "quota_at_class_sizes":
            assert (npos == quota).all() and (nneg == batch - quota).all()
        if name == "quota_below_both":
            assert (npos > quota).all() and (nneg > batch - quota).all()
        assert (labels[:, -3:] == -1).all()


@pytest.mark.parametrize("name", sorted(T.sample_cases()))
def test_sample_and_gather_checker_against_sorting(name):
    labels, keys, batch, fraction = T.sample_cases()[name]
    rng = np.random.default_rng(5)
    for n in range(labels.shape[0]):
        out, sidx, n_pos, n_neg = RL.sample(labels[n], keys[n], batch, fraction)
        order = np.lexsort((np.arange(labels.shape[1]), keys[n].astype(np.int64)))       # by (key, index)
        pos, neg = [i for i in order if labels[n][i] == 1], [i for i in order if labels[n][i] == 0]
        assert n_pos == min(len(pos), int(batch * fraction)) and n_neg == min(len(neg), batch - n_pos)
        assert sidx == sorted(pos[:n_pos]) + sorted(neg[:n_neg])
        assert (out == 1).sum() == n_pos and (out == 0).sum() == n_neg
        # gather: positives carry their box's class, negatives K, the rest -1
        props, gt, gc = RL._rand_boxes(rng, T.P), RL._rand_boxes(rng, 10), rng.integers(0, 5, 10).astype(np.int32)
        midx = rng.integers(0, 10, labels.shape[1]).astype(np.int32)
        b, cnt, cls, gb = T.gather(props, T.P, gt, gc, midx, sidx, n_pos, n_neg, 5, batch)
        cand = np.concatenate([props, gt])
        assert cnt == n_pos + n_neg and np.array_equal(b[:cnt], cand[sidx]) and np.array_equal(gb[:cnt], gt[midx[sidx]])
        assert np.array_equal(cls[:n_pos], gc[midx[sidx[:n_pos]]]) and (cls[n_pos:cnt] == 5).all() and (cls[cnt:] == -1).all()
        assert not b[cnt:].any() and not gb[cnt:].any()


@pytest.mark.parametrize("K,agnostic,beta", [(5, False, 0.0), (5, True, 0.5), (80, False, 0.5), (80, False, 0.0)])
def test_loss_checker_against_torch_autograd(K, agnostic, beta):
    c = T.loss_case(K, agnostic)
    w = (10.0, 10.0, 5.0, 5.0)
    lc, lb, dpred, ac, al, rtot = T.box_loss(c["pred"], K, agnostic, c["boxes"], c["counts"], c["cls"], c["gboxes"], w, beta)
    rows = [(n, j) for n in range(T.N) for j in range(int(c["counts"][n]))]
    assert rtot == len(rows)
    p = torch.tensor(c["pred"], dtype=torch.float64, requires_grad=True)
    sel = torch.tensor([n * T.B + j for n, j in rows])
    tc = torch.tensor([int(c["cls"][n, j]) for n, j in rows])
    ref_c = Fn.cross_entropy(p[sel, :K + 1], tc, reduction="sum") / rtot
    fg = [i for i, (n, j) in enumerate(rows) if c["cls"][n, j] < K]
    cols = torch.tensor([[K + 1 + (0 if agnostic else 4 * int(c["cls"][rows[i]])) + k for k in range(4)] for i in fg])
    tg = torch.tensor([[float(F(v)) for v in RL.get_deltas(c["boxes"][rows[i]], c["gboxes"][rows[i]], w)] for i in fg], dtype=torch.float64)
    d = p[sel[torch.tensor(fg)]].gather(1, cols) - tg
    ref_b = (d.abs().sum() if beta < 1e-5 else torch.where(d.abs() < beta, 0.5 * d * d / beta, d.abs() - 0.5 * beta).sum()) / rtot
    (ref_c + ref_b).backward()
    assert abs(lc - ref_c.item()) < 1e-12 * max(1, abs(lc)) and abs(lb - ref_b.item()) < 1e-12 * max(1, abs(lb))
    assert np.abs(dpred - p.grad.numpy()).max() < 1e-14
    # the plain fp32 formula passes the stated bars
    lc32, lb32, _, _, _, _ = T.box_loss(c["pred"], K, agnostic, c["boxes"], c["counts"], c["cls"], c["gboxes"], w, beta, dtype=np.float32)
    assert abs(lb32 - lb) <= T.K_LOC * T.EPS * al / rtot


def test_loss_fixtures_hold_what_they_are_for():
    c = T.loss_case(80, False)
    live = np.concatenate([c["cls"][n, :c["counts"][n]] for n in range(T.N)])
    assert len(set(live[live < 80].tolist())) >= 3 and (live == 80).sum() >= 3 and (c["counts"] < T.B).any()
    assert c["pred"].shape[1] > 64
    c = T.loss_case(5, False, no_fg_image=True)
    assert (c["cls"][1, :c["counts"][1]] == 5).all() and (c["cls"][0, :c["counts"][0]] < 5).any()
    assert T.box_loss(**{k: T.loss_case(5, False, empty=True)[k] for k in ("pred", "K", "agnostic", "boxes", "counts", "cls", "gboxes")},
                      weights=(10.0, 10.0, 5.0, 5.0), beta=0.0)[:2] == (0.0, 0.0)


def test_end_to_end_fixture_holds_what_it_is_for():
    case = T.e2e_case()
    a = T.assign(case, 5)
    for n in range(T.N):
        assert a["n_pos"][n] >= 8 and a["n_neg"][n] >= 8
    live = np.concatenate([a["boxes"][n, :a["counts"][n]] for n in range(T.N)])
    live = live[(live[:, 2] > live[:, 0]) & (live[:, 3] > live[:, 1])]
    assert len(set(Q.level_of(live, T.MIN_LEVEL, T.MIN_LEVEL + 3).tolist())) >= 3
    fg = np.concatenate([a["cls"][n, :a["n_pos"][n]] for n in range(T.N)])
    assert len(set(fg.tolist())) >= 3


# ------------------------------------------------------------------------------------------------ ROIAlign backward
def _torch_roi_align(levels, min_level, boxes, counts, S, sr):
    """ROIAlignV2 sample by sample in torch float64 (bilinear_interpolate's rules on index tensors), differentiable in the levels."""
    rows = []
    nb, batch = boxes.shape[:2]
    C = levels[0].shape[1]
    b64 = np.asarray(boxes, F).astype(np.float64)
    for n in range(nb):
        lv = Q.level_of(b64[n], min_level, min_level + len(levels) - 1)
        for j in range(batch):
            bx = b64[n, j]
            if j >= counts[n] or not (bx[2] > bx[0] and bx[3] > bx[1]):
                rows.append(torch.zeros((C, S, S), dtype=torch.float64))
                continue
            f = levels[lv[j] - min_level][n]
            H, W = f.shape[1:]
            gh, gw, rh, rw = Q.grid_of(bx, lv[j], S, sr)
            scale = 1.0 / (1 << int(lv[j]))

            def axis(start, roi, grid, size):
                p, i = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(grid, dtype=np.float64), indexing="ij")
                v = (start + p * (roi / S) + (i + 0.5) * (roi / S) / grid).reshape(-1)
                ok = (v >= -1.0) & (v <= size)
                v = np.maximum(v, 0.0)
                lo = np.floor(v).astype(np.int64)
                last = lo >= size - 1
                lo = np.where(last, size - 1, lo)
                v = np.where(last, lo.astype(np.float64), v)
                hi = np.where(last, size - 1, lo + 1)
                l = v - lo
                return (torch.tensor(np.clip(lo, 0, size - 1)), torch.tensor(np.clip(hi, 0, size - 1)), torch.tensor((1 - l) * ok), torch.tensor(l * ok))
            yl, yh, wyl, wyh = axis(bx[1] * scale - 0.5, rh, gh, H)
            xl, xh, wxl, wxh = axis(bx[0] * scale - 0.5, rw, gw, W)
            rowsum = f[:, yl] * wyl[None, :, None] + f[:, yh] * wyh[None, :, None]                 # [C, S gh, W]
            val = rowsum[:, :, xl] * wxl[None, None, :] + rowsum[:, :, xh] * wxh[None, None, :]  # [C, S gh, S gw]
            rows.append(val.view(C, S, gh, S, gw).sum((2, 4)) / max(gh * gw, 1))
    return torch.stack(rows)


ALIGN_BWD_CASES = [("align_boxes", 7, 0), ("align_boxes", 7, 2), ("special", 7, 0), ("special", 14, 2), ("twenty_identical", 7, 0)]


@pytest.mark.parametrize("name,S,sr", ALIGN_BWD_CASES)
def test_align_bwd_checker_bar_and_wrong_variants(name, S, sr):
    boxes, counts = T.align_bwd_box_sets()[name]
    rng = np.random.default_rng(S + sr)
    C = 4
    g = rng.standard_normal((T.N * T.B, C, S, S)).astype(F)
    ref = T.align_bwd(g, T.LEVELS, T.MIN_LEVEL, boxes, counts, S, sr)
    # the checker is the transpose of the forward: against autograd through a sample-by-sample ROIAlign
    lv = [torch.zeros((T.N, C, H, W), dtype=torch.float64, requires_grad=True) for H, W in T.LEVELS]
    out = _torch_roi_align(lv, T.MIN_LEVEL, boxes, counts, S, sr)
    (out * torch.tensor(g, dtype=torch.float64)).sum().backward()
    for (gr, ab, tm), x in zip(ref, lv):
        auto = x.grad.numpy() if x.grad is not None else np.zeros(gr.shape)         # (a level no box lands on is not in the graph)
        assert np.abs(gr - auto).max() <= 1e-12 * max(1.0, np.abs(gr).max())
        assert (gr[tm[:, None].repeat(C, 1) == 0] == 0).all()
    # the bar: passed by fp32 in the kernel's order, failed by the two wrong variants somewhere
    def worst(variant):
        got = T.align_bwd_f32(g, T.LEVELS, T.MIN_LEVEL, boxes, counts, S, sr, variant)
        return max(float(((np.abs(o.astype(np.float64) - gr) - (tm[:, None] + T.K_ALIGN_BWD) * T.EPS * ab)).max()) for o, (gr, ab, tm) in zip(got, ref))
    assert worst("kernel") <= 0.0
    if name != "twenty_identical":                         # (that box is nowhere near the last row or column: the collapse never acts)
        assert worst("no_collapse") > 0.0
    assert worst("wrong_count") > 0.0


def test_align_bwd_box_sets_hold_what_they_are_for():
    sets = T.align_bwd_box_sets()
    sp, cnt = sets["special"]
    ih, iw = T.IMAGE
    assert sp[0, 0, 2] < 0 and sp[0, 1, 2] == iw and sp[0, 1, 3] == ih and sp[0, 2, 0] == sp[0, 2, 2] and cnt[1] < cnt[0] < T.B
    same, cnt = sets["twenty_identical"]
    assert (same[:, :20] == same[0, 0]).all() and (cnt == 20).all()
    ab, cnt = sets["align_boxes"]
    live = ab[0, :cnt[0]]
    live = live[(live[:, 2] > live[:, 0]) & (live[:, 3] > live[:, 1])]
    assert len(set(Q.level_of(live, T.MIN_LEVEL, T.MIN_LEVEL + 3).tolist())) == 4


# ------------------------------------------------------------------------------------------------ the module's refusals
def test_construction_refusals_name_the_key():
    with pytest.raises(amd.AfiError, match=r"ROI_HEADS\.IOU_THRESHOLDS .*one threshold only"):
        amd.build_roi_heads(_cfg({"ROI_HEADS": {"IOU_THRESHOLDS": [0.3, 0.7], "IOU_LABELS": [0, -1, 1]}}), _shapes())
    with pytest.raises(amd.AfiError, match=r"ROI_HEADS\.IOU_LABELS .*\[0, 1\] only"):
        amd.build_roi_heads(_cfg({"ROI_HEADS": {"IOU_LABELS": [1, 0]}}), _shapes())
    with pytest.raises(amd.AfiError, match=r"ROI_HEADS\.BATCH_SIZE_PER_IMAGE 5000"):
        amd.build_roi_heads(_cfg({"ROI_HEADS": {"BATCH_SIZE_PER_IMAGE": 5000}}), _shapes())
    with pytest.raises(amd.AfiError, match=r"ROI_HEADS\.POSITIVE_FRACTION"):
        amd.build_roi_heads(_cfg({"ROI_HEADS": {"POSITIVE_FRACTION": 1.5}}), _shapes())
    with pytest.raises(amd.AfiError, match=r"ROI_BOX_HEAD\.SMOOTH_L1_BETA"):
        amd.build_roi_heads(_cfg({"ROI_BOX_HEAD": {"SMOOTH_L1_BETA": -1.0}}), _shapes())


def test_trainable_flips_the_box_branch_only_and_config_is_read():
    h = amd.build_roi_heads(_cfg({"ROI_HEADS": {"POSITIVE_FRACTION": 0.5, "PROPOSAL_APPEND_GT": False}, "ROI_BOX_HEAD": {"SMOOTH_L1_BETA": 0.5}}),
                            _shapes())
    assert (h.batch_size_per_image, h.positive_fraction, h.proposal_append_gt, h.smooth_l1_beta, h.iou_threshold) == (32, 0.5, False, 0.5, 0.5)
    assert not any(p.requires_grad for p in h.parameters())
    assert h.trainable_() is h and all(p.requires_grad for p in h.parameters())
    h.trainable_(False)
    assert not any(p.requires_grad for p in h.parameters())
    m = amd.build_roi_heads(_cfg({"MASK_ON": True}), _shapes(), masks=True).trainable_()
    assert all(p.requires_grad for p in m.box_head.parameters()) and not any(p.requires_grad for p in m.mask_head.parameters())


def test_call_time_refusals():
    images = type("Images", (), {"image_sizes": [(32, 32)], "__len__": lambda s: 1})()
    x = torch.zeros((1, 8, 8, 8))
    prop = [type("P", (), {"proposal_boxes": torch.zeros((3, 4))})()]
    tgt = [{"gt_boxes": torch.tensor([[1.0, 1.0, 9.0, 9.0]]), "gt_classes": torch.tensor([2])}]
    h = amd.build_roi_heads(_cfg({"ROI_HEADS": {"IN_FEATURES": ["p2"]}}), _shapes()).train()
    with pytest.raises(amd.AfiError, match="CPU tensor"):                   # a training call reaches the device checks: it is no longer refused
        h(images, {"p2": x}, prop, tgt)
    with pytest.raises(amd.AfiError, match="inference-only"):
        h(images, {"p2": x}, prop)
    h.eval()
    with pytest.raises(amd.AfiError, match="targets given"):
        h(images, {"p2": x}, prop, tgt)
    m = amd.build_roi_heads(_cfg({"MASK_ON": True, "ROI_HEADS": {"IN_FEATURES": ["p2"]}}), _shapes(), masks=True).train()
    with pytest.raises(amd.AfiError, match="mask loss is not built yet"):
        m(images, {"p2": x}, prop, tgt)
    with pytest.raises(amd.AfiError, match="mask loss is not built yet"):
        m.losses(images, {"p2": x}, prop, tgt)
    # the targets: checked before anything touches the device
    for bad, msg in (([{"gt_boxes": torch.zeros((1, 4)), "gt_classes": torch.tensor([5])}], r"gt_classes must lie in 0\.\.4"),
                     ([{"gt_boxes": torch.zeros((1, 4)), "gt_classes": torch.tensor([-1])}], r"gt_classes must lie in 0\.\.4"),
                     ([{"gt_boxes": torch.zeros((1, 4)), "gt_classes": torch.tensor([1.0])}], "must be integers"),
                     ([{"gt_boxes": torch.zeros((2, 4)), "gt_classes": torch.tensor([1])}], "gt_boxes .* and gt_classes"),
                     ([{"gt_boxes": torch.zeros((1, 4))}], "gt_boxes .* and gt_classes"),
                     ([], "0 targets for a batch of 1")):
        with pytest.raises(amd.AfiError, match=msg):
            h._targets(bad, 1, "cpu")
    gt, gc, gn = h._targets([type("T", (), {"gt_boxes": amd.rpn.Boxes(torch.ones((2, 4))), "gt_classes": torch.tensor([0, 4])})()], 1, "cpu")
    assert tuple(gt.shape) == (1, 2, 4) and gc.tolist() == [[0, 4]] and gn.tolist() == [2] and gc.dtype == torch.int32


def test_ops_refuse_wrong_dtypes_and_shapes():
    p, cp = torch.zeros((1, 4, 4)), torch.zeros((1,), dtype=torch.int32)
    g, cg = torch.zeros((1, 2, 4)), torch.zeros((1,), dtype=torch.int32)
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        amd.ops.roi_label(p, cp, g, cg)
    with pytest.raises(amd.AfiError, match=r"roi_label: dense proposals"):
        amd.ops.roi_label(p[0], cp, g, cg)
    with pytest.raises(amd.AfiError, match="at most 1024"):
        amd.ops.roi_label(p, cp, torch.zeros((1, 1025, 4)), cg)
    with pytest.raises(amd.AfiError, match=r"roi_box_loss: pred"):
        amd.ops.roi_box_loss(torch.zeros((4, 8)), 5, False, torch.zeros((1, 4, 4)), cp, torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 4, 4)))
    with pytest.raises(amd.AfiError, match=r"roi_align_bwd: 1\.\.8 levels"):
        amd.ops.roi_align_bwd(torch.zeros((4, 8, 7, 7)), [], 2, torch.zeros((1, 4, 4)), cp)
