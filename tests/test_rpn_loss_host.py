"""CPU-side checks of the RPN's training side: tests/rpn_loss_f64.py -- the plain-loop yardstick of test_gpu_rpn_loss.py -- against a vectorised
torch restatement of the detectron2 formulas (pairwise_iou as a G x R fp32 matrix, max along both axes, the == promotion; the losses through
torch's own binary_cross_entropy_with_logits and autograd); the match cases held to what they are meant to show; the loss bars let the plain
fp32 formula through; the config keys, the refusals, and the parameters staying frozen until ``trainable_()``."""
import numpy as np
import pytest
import torch

import afigan_amd as amd
from afigan_amd import ops
from afigan_amd.fpn_sr import ShapeSpec

import rpn_loss_f64 as O

CASES = O.match_cases()
_ORACLE = {}


def _oracle(name):
    if name not in _ORACLE:
        c = CASES[name]
        anc, _ = O.anchors(c["cells"])
        _ORACLE[name] = (anc, [O.match(anc, g, *c["thresholds"]) for g in c["gts"]])
    return _ORACLE[name]


def _torch_match(anc, gt, t0, t1):
    """detectron2's pairwise_iou + Matcher(allow_low_quality_matches=True), vectorised, fp32."""
    a, g = torch.from_numpy(anc), torch.from_numpy(gt)
    if len(g) == 0:
        return np.zeros(len(a), np.int8), np.zeros(len(a), np.float32), None
    area_g, area_a = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]), (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    wh = (torch.min(g[:, None, 2:], a[:, 2:]) - torch.max(g[:, None, :2], a[:, :2])).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    iou = torch.where(inter > 0, inter / (area_g[:, None] + area_a - inter), torch.zeros(()))
    vals, _ = iou.max(dim=0)
    labels = torch.full((len(a),), 1, dtype=torch.int8)
    labels[vals < np.float32(t1)] = -1
    labels[vals < np.float32(t0)] = 0
    best, _ = iou.max(dim=1)
    labels[(iou == best[:, None]).any(dim=0)] = 1
    return labels.numpy(), vals.numpy(), iou.numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_loop_match_equals_the_vectorised_restatement(name):
    c = CASES[name]
    anc, per_image = _oracle(name)
    assert len(anc) == 912 and len(anc) % 64 and len(c["gts"]) == 2 and (name == "no_gt" or len(c["gts"][0]) != len(c["gts"][1]))
    for gt, (labels, midx, mval) in zip(c["gts"], per_image):
        want, vals, iou = _torch_match(anc, gt, *c["thresholds"])
        assert np.array_equal(labels, want) and np.array_equal(mval, vals)
        if iou is None:
            assert not midx.any()
            continue
        assert np.array_equal(iou[midx, np.arange(len(anc))], vals)                          # the matched box reaches the maximum ...
        first = (iou == vals[None]).argmax(axis=0)
        assert np.array_equal(midx, first)                                                  # ... and is the lowest index that does


def test_match_cases_show_what_they_are_for():
    lab = lambda name, n: _oracle(name)[1][n]
    # exactly t1: 70 / 100 in fp32 is fp32 0.7, label 1 by the threshold; no box has this anchor as its best
    labels, midx, mval = lab("iou_exactly_t1", 1)
    assert mval[0] == np.float32(0.7) and np.float32(70.0) / np.float32(100.0) == np.float32(0.7) and labels[0] == 1 and mval[:3].max() > mval[0]
    # one ulp below each threshold: label 0 under t0, -1 under t1, and each would be one class higher AT the threshold
    t0, t1 = (np.float32(t) for t in CASES["one_ulp_below_thresholds"]["thresholds"])
    labels, midx, mval = lab("one_ulp_below_thresholds", 1)
    assert np.nextafter(mval[0], np.float32(1)) == t0 and labels[0] == 0 and np.nextafter(mval[3], np.float32(1)) == t1 and labels[3] == -1
    anc = _oracle("one_ulp_below_thresholds")[0]
    at = O.match(anc, CASES["one_ulp_below_thresholds"]["gts"][1], float(mval[0]), float(mval[3]))[0]
    assert at[0] == -1 and at[3] == 1
    # several anchors tie for a box's best and all are promoted from below t1
    labels, midx, mval = lab("tied_best", 0)
    tied = np.nonzero((mval == mval[midx == 0].max()) & (midx == 0))[0]
    assert len(tied) == 4 and mval[tied[0]] < 0.7 and (labels[tied] == 1).all()
    # a box that overlaps nothing promotes every anchor; next to it an ordinary image
    assert (lab("box_overlapping_nothing", 0)[0] == 1).all() and 0 < (lab("box_overlapping_nothing", 1)[0] == 1).sum() < 20
    # identical boxes: never the later copy
    labels, midx, _ = lab("identical_boxes", 0)
    assert (midx == 1).any() and not (midx == 2).any() and not (midx == 4).any()
    assert len(CASES["more_than_one_lds_tile"]["gts"][0]) > 256 and (lab("more_than_one_lds_tile", 0)[1] >= 256).any()
    assert not lab("no_gt", 0)[0].any() and not lab("one_box_beside_empty", 1)[0].any() and lab("one_box_beside_empty", 0)[0].any()


@pytest.mark.parametrize("name", list(O.sample_cases()))
def test_sample_rule(name):
    labels, keys, batch, frac = O.sample_cases()[name]
    for n in range(2):
        out, idx, n_pos, n_neg = O.sample(labels[n], keys[n], batch, frac)
        pos, neg = np.nonzero(labels[n] == 1)[0], np.nonzero(labels[n] == 0)[0]
        assert n_pos == min(len(pos), int(batch * frac)) and n_neg == min(len(neg), batch - n_pos) and len(idx) == n_pos + n_neg
        assert (out == 1).sum() == n_pos and (out == 0).sum() == n_neg and np.array_equal(out[idx], [1] * n_pos + [0] * n_neg)
        for cls, members, k, got in ((1, pos, n_pos, idx[:n_pos]), (0, neg, n_neg, idx[n_pos:])):
            order = np.lexsort((members, keys[n][members]))                    # by key, then by index: numpy's stable sort, not the checker's
            assert sorted(members[order[:k]].tolist()) == list(got)
    if name == "more_positives_than_quota":
        assert (labels[0] == 1).sum() > 4 and n_pos == 4
    if name == "fewer_negatives_than_asked":
        assert n_neg == 2 and n_pos == 32


@pytest.mark.parametrize("beta,weights", [(0.0, (1.0, 1.0, 1.0, 1.0)), (0.5, (2.0, 2.0, 1.0, 1.0))])
def test_loop_losses_against_torch_and_the_bars_let_plain_fp32_through(beta, weights):
    """The fp64 loop equals torch's own BCE-with-logits / smooth-L1 and autograd in float64; the same terms evaluated in numpy float32 stay
    within K 2^-24 sum |term| of it (K_CLS = 10, K_LOC = 5: counted in rpn_loss_f64.py) -- a bar the plain fp32 formula failed would be wrong."""
    c = O.loss_case(weights)
    scale = 1.0 / (c["batch"] * c["N"])
    args = (c["anc"], c["where"], c["A"], c["gts"], c["midx"], c["sidx"], c["n_pos"], c["n_neg"], weights, beta, scale)
    lc, ll, grads, ac, al = O.losses(c["heads"], *args)
    A = c["A"]
    th = [(torch.tensor(h[:, :A], dtype=torch.float64, requires_grad=True), torch.tensor(h[:, A:5 * A], dtype=torch.float64, requires_grad=True))
          for h in c["heads"]]
    tc, tl = O.torch_losses(None, None, A, c["anc"], c["where"], c["gts"], c["midx"], c["sidx"], c["n_pos"], c["n_neg"], weights, beta, scale, heads=th)
    (tc + tl).backward()
    assert abs(lc - tc.item()) <= 1e-13 * abs(lc) and abs(ll - tl.item()) <= 1e-13 * abs(ll) and lc > 0 and ll > 0
    for g, (zl, zd) in zip(grads, th):
        gl, gd = (t.grad.numpy() if t.grad is not None else 0.0 for t in (zl, zd))          # (None: no sampled anchor on that level)
        assert np.abs(g[:, :A] - gl).max() <= 1e-15 and np.abs(g[:, A:5 * A] - gd).max() <= 1e-15
        assert not g[:, 5 * A:].any()
    n, i, ch = c["planted_zero"]
    l, y, x, _ = c["where"][i]
    assert grads[l][n, ch, y, x] == 0.0 and np.count_nonzero(grads[l][n, :, y, x]) >= 4       # d = 0 exactly: no gradient, whatever beta
    fc, fl, _, _, _ = O.losses(c["heads"], *args, dtype=np.float32)
    print(f"fp32 formula: cls {abs(fc - lc):.3e} (bar {O.K_CLS * O.EPS * ac * scale:.3e}), loc {abs(fl - ll):.3e} (bar {O.K_LOC * O.EPS * al * scale:.3e})")
    assert abs(fc - lc) <= O.K_CLS * O.EPS * ac * scale and abs(fl - ll) <= O.K_LOC * O.EPS * al * scale


# ------------------------------------------------------------------------------------------------ the module and the ops
FEATURES = ["p3", "p4", "p5"]


def _cfg(**rpn_keys):
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[32], [64], [128]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": FEATURES, "PRE_NMS_TOPK_TEST": 1000, "POST_NMS_TOPK_TEST": 1000, **rpn_keys}})
    return cfg


def _shapes(channels=16):
    return {f: ShapeSpec(channels=channels, stride=8 * 2 ** i) for i, f in enumerate(FEATURES)}


def test_training_keys_are_read_with_detectron2s_defaults():
    m = amd.RPN(_cfg(), _shapes())
    assert (m.iou_thresholds, m.batch_size_per_image, m.positive_fraction, m.smooth_l1_beta, m.loss_weight) == ((0.3, 0.7), 256, 0.5, 0.0, 1.0)
    assert (m.pre_nms_topk_train, m.post_nms_topk_train) == (12000, 2000)
    m = amd.RPN(_cfg(IOU_THRESHOLDS=[0.2, 0.6], BATCH_SIZE_PER_IMAGE=8, POSITIVE_FRACTION=0.25, SMOOTH_L1_BETA=0.11, LOSS_WEIGHT=2.0,
                     PRE_NMS_TOPK_TRAIN=500, POST_NMS_TOPK_TRAIN=100), _shapes())
    assert (m.iou_thresholds, m.batch_size_per_image, m.positive_fraction, m.smooth_l1_beta, m.loss_weight) == ((0.2, 0.6), 8, 0.25, 0.11, 2.0)
    assert (m.pre_nms_topk_train, m.post_nms_topk_train) == (500, 100)
    # the cell anchors of the module are the checker's
    assert np.array_equal(torch.stack(list(m.anchor_generator.cell_anchors)).numpy(), O.cell_anchors())


@pytest.mark.parametrize("key,value,match", [("BOUNDARY_THRESH", 0, "BOUNDARY_THRESH"), ("IOU_LABELS", [0, 1, 1], "IOU_LABELS"),
                                             ("IOU_THRESHOLDS", [0.7, 0.3], "IOU_THRESHOLDS"), ("BATCH_SIZE_PER_IMAGE", 5000, "4096"),
                                             ("SMOOTH_L1_BETA", -1.0, "SMOOTH_L1_BETA")])
def test_unsupported_training_configs_raise_at_construction(key, value, match):
    with pytest.raises(amd.AfiError, match=match):
        amd.RPN(_cfg(**{key: value}), _shapes())


def test_parameters_stay_frozen_until_trainable():
    m = amd.RPN(_cfg(), _shapes())
    assert not any(p.requires_grad for p in m.parameters())
    assert m.trainable_(True) is m and all(p.requires_grad for p in m.parameters()) and len(list(m.parameters())) == 6
    assert not any(p.requires_grad for p in m.trainable_(False).parameters())


class _Imgs:
    def __init__(self, sizes):
        self.image_sizes = sizes

    def __len__(self):
        return len(self.image_sizes)


class _GT:
    def __init__(self, boxes):
        self.gt_boxes = boxes


def test_training_forward_refusals():
    feats = {f: torch.zeros(1, 16, 4, 4) for f in FEATURES}
    gt = [_GT(torch.tensor([[0.0, 0.0, 10.0, 10.0]]))]
    m = amd.RPN(_cfg(), _shapes()).train()                 # PRE_NMS_TOPK_TRAIN 12000, detectron2's default
    with pytest.raises(amd.AfiError, match=r"PRE_NMS_TOPK_TRAIN 12000.*1024.*losses\(\) works regardless.*separate piece of work"):
        m(_Imgs([(32, 32)]), feats, gt)
    m = amd.RPN(_cfg(PRE_NMS_TOPK_TRAIN=1000, POST_NMS_TOPK_TRAIN=500), _shapes()).train()
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        m(_Imgs([(32, 32)]), feats, gt)
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        m.losses(_Imgs([(32, 32)]), feats, gt)
    with pytest.raises(amd.AfiError, match="inference-only"):                  # without ground truth a training-mode call stays refused
        m(_Imgs([(32, 32)]), feats)
    with pytest.raises(amd.AfiError, match="gt_instances"):
        m.eval()(_Imgs([(32, 32)]), feats, gt)


def test_ops_name_their_limits():
    cell = torch.zeros(1, 3, 4)
    gt, counts = torch.zeros(1, 2, 4), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        ops.rpn_match([(4, 4)], [8], cell, 3, gt, counts)
    with pytest.raises(amd.AfiError, match=f"at most {ops.RPN_MAX_GT}"):
        ops.rpn_match([(4, 4)], [8], cell, 3, torch.zeros(1, ops.RPN_MAX_GT + 1, 4), counts)
    assert ops.RPN_MAX_GT >= 512 and ops.RPN_MAX_TOTAL_ANCHORS == 2 ** 22
    with pytest.raises(amd.AfiError, match=rf"{1183 * 1182 * 3} anchors.*4194304 \(2\^22\)"):
        ops.rpn_match([(1183, 1182)], [8], cell, 3, gt, counts)               # just above 2^22
    with pytest.raises(amd.AfiError, match="cell anchors"):
        ops.rpn_match([(4, 4)], [8], torch.zeros(2, 3, 4), 3, gt, counts)
    labels, keys = torch.zeros(1, 48, dtype=torch.int8), torch.zeros(1, 48, dtype=torch.int32)
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        ops.rpn_sample(labels, keys, 8, 0.5)
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        ops.rpn_loss([torch.zeros(1, 16, 4, 4)], [8], cell, 3, gt, counts, keys, keys, counts, counts)
    lib = amd._lib.load()
    assert lib.afi_rpn_match(None, None, 1, 3, None, 1, None, None, 1, 0.3, 0.7, None, None, None, 0, None) == 1      # AFI_ERR_BAD_ARG, no launch
    assert lib.afi_rpn_sample(None, None, 1, 48, 8, 4, None, None, None, None, None) == 1
