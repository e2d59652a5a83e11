"""COCO evaluation without a GPU: the known answers that tie tests/coco_eval_f64.py (the plain-loop checker) to COCO's definition, the host half of
afigan_amd/coco_eval.py (accumulate, summarize) against the checker on the same match tables -- exactly --, COCOEvaluator's construction and error
paths, the entry points' return codes, and the proof that the seeded set of tests/test_gpu_coco_eval.py holds the shapes it is meant to hold."""
import numpy as np
import pytest

import coco_eval_cases as CC
import coco_eval_f64 as Q

# AP, AP50, AP75, APs, APm, APl, AR@1, AR@10, AR@100, ARs, ARm, ARl
KNOWN = {
    "A": [1, 1, 1, -1, 1, -1, 1, 1, 1, -1, 1, -1],
    "B": [.5, .5, .5, -1, .5, -1, 0, 1, 1, -1, 1, -1],
    "C": [.6, 1, 1, -1, -1, .6, .6, .6, .6, -1, -1, .6],
    "D": [1, 1, 1, -1, 1, -1, 0, 1, 1, -1, 1, -1],             # AR@1 = 0: the one detection kept is the one the crowd absorbs
    "D-crowd-only": [-1] * 12,
    "E": [0, 0, 0, -1, 0, -1, 0, 0, 0, -1, 0, -1],
    "F": [1, 1, 1, 1, 1, -1, 1, 1, 1, 1, 1, -1],               # area 1024 counts in small and in medium
}
TASKS = ("bbox", "segm")


@pytest.mark.parametrize("task", TASKS)
@pytest.mark.parametrize("name", sorted(KNOWN))
def test_checker_known_answers(name, task):
    gt, res = CC.hand_case(name)
    e = Q.evaluate(gt, res, task)
    assert np.abs(e["stats"] - np.array(KNOWN[name], np.float64)).max() < 1e-12, e["stats"]
    if name == "B":
        assert (e["precision"][:, :, 0, 0, 2] == 0.5).all() and e["precision"].shape == (10, 101, 1, 4, 3) and e["recall"].shape == (10, 1, 4, 3)
    if name == "D":
        g = e["groups"][0]
        assert (g["dt_match"][0, :, 0] == 1).all() and (g["dt_ignore"][0, :, 0] == 1).all() and g["iou"][0, 1] == 1.0
        assert (g["dt_match"][0, :, 1] == 0).all() and not g["dt_ignore"][0, :, 1].any()
    if name == "E":
        assert len(e["groups"][0]["dts"]) == 100 and not e["groups"][0]["iou"].any()


@pytest.mark.parametrize("task", TASKS)
def test_checker_ties_and_the_exact_threshold(task):
    g = Q.evaluate(*CC.hand_case("G"), task)["groups"][0]
    assert g["iou"].tolist() == [[0.5, 0.5]]
    assert g["dt_match"][:, 0, 0].tolist() == [1, 1, 1, 1] and (g["dt_match"][:, 1:, 0] == -1).all()        # the later GT, among the ignored ones too
    assert g["dt_ignore"][:, 0, 0].tolist() == [0, 0, 1, 1]                                                  # both GTs are small
    h = Q.evaluate(*CC.hand_case("H"), task)["groups"][0]
    assert h["iou"].tolist() == [[0.5]] and h["dt_match"][0, :, 0].tolist() == [0] + [-1] * 9
    f = Q.evaluate(*CC.hand_case("F"), task)["groups"][0]
    assert f["gt_ignore"][:, 0].tolist() == [0, 0, 0, 1]


def test_checker_mask_primitives():
    m = np.zeros((5, 4), bool)
    m[1:4, 1:3] = True
    s = Q.starts_of_mask(m)
    assert s == [6, 9, 11, 14] and Q.starts_of_counts(CC.counts_of(m)) == s and Q.rle_area(s, 20) == 6
    full, empty, last = [0], [], [19]
    assert Q.rle_area(full, 20) == 20 and Q.rle_area(empty, 20) == 0 and Q.rle_area(last, 20) == 1
    assert Q.rle_inter(s, full, 20) == 6 and Q.rle_inter(s, empty, 20) == 0 and Q.rle_inter(full, last, 20) == 1 and Q.rle_inter(s, last, 20) == 0
    assert Q.rle_inter([6, 9, 9, 9, 11, 14], s, 20) == 6                 # an empty run between two equal starts
    rng = np.random.default_rng(3)
    for _ in range(20):
        a, b = rng.random((7, 9)) < 0.5, rng.random((7, 9)) < 0.4
        assert Q.rle_inter(Q.starts_of_mask(a), Q.starts_of_mask(b), 63) == int((a & b).sum()) and Q.rle_area(Q.starts_of_mask(a), 63) == int(a.sum())
    inter, iou = Q.rle_iou([(s, 20), (empty, 20), (s, 21)], [(full, 20), (empty, 20)], [1, 0])
    assert inter.tolist() == [[6, 0], [0, 0], [-1, -1]] and iou.tolist() == [[1.0, 0.0], [0.0, 0.0], [-1.0, -1.0]]


@pytest.mark.parametrize("task", TASKS)
def test_the_synthetic_set_holds_what_the_gpu_tests_need(task):
    gt, res, e = CC.checked_set(task)
    groups = {(g["img"], g["k"]): g for g in e["groups"]}
    ids, n_in = CC.SET_IMAGE_IDS, lambda i, k: sum(r["image_id"] == CC.SET_IMAGE_IDS[i] and r["category_id"] == CC.SET_CAT_IDS[k] for r in res)
    assert all(max(im["height"], im["width"]) <= 130 and min(im["height"], im["width"]) <= 90 for im in gt["images"]) and len(gt["images"]) == 6
    assert any(im["height"] > 64 for im in gt["images"]) and len(gt["categories"]) == 3
    assert n_in(0, 0) == 130 and len(groups[(ids[0], 0)]["dts"]) == 100               # cut
    assert len(groups[(ids[0], 1)]["gts"]) == 70                                       # more than a wave
    assert len(groups[(ids[0], 2)]["dts"]) == 0 and len(groups[(ids[0], 2)]["gts"]) == 2
    assert len(groups[(ids[1], 0)]["gts"]) == 0 and len(groups[(ids[1], 0)]["dts"]) == 4
    assert (ids[1], 1) not in groups and len(groups) == 17
    for key in ((ids[1], 2), (ids[2], 1)):                                            # a crowd matched by several detections at one (a, t)
        g = groups[key]
        c = g["crowd"].index(1)
        assert int((g["dt_match"][0, 0] == c).sum()) >= 3, key
    assert any(len(set(g["scores"])) < len(g["scores"]) for g in groups.values())     # tied scores
    ga = np.array([a for g in groups.values() for a in g["gt_area"]])
    da = np.array([a for g in groups.values() for a in g["dt_area"]])
    for v in (ga, da):
        assert (v < 1024).any() and ((v > 1024) & (v < 9216)).any() and (v > 9216).any()
    assert groups[(ids[5], 0)]["dt_match"][0, 0, 0] == 1 and groups[(ids[5], 0)]["iou"].tolist() == [[0.5, 0.5]]      # G
    assert groups[(ids[5], 1)]["dt_match"][0, :, 0].tolist() == [0] + [-1] * 9                                      # H
    if task == "segm":
        assert any(len(g["dts"]) and max(len(r["segmentation"]["counts"]) for r in g["dts"]) > 64 for g in groups.values())
    assert (e["stats"][:3] > 0).all() and (e["stats"][:3] < 1).all()


@pytest.mark.parametrize("task", TASKS)
def test_accumulate_and_summarize_equal_the_checker_exactly(task):
    from afigan_amd import coco_eval
    assert np.array_equal(coco_eval.IOU_THRS, Q.IOU_THRS) and np.array_equal(coco_eval.REC_THRS, Q.REC_THRS)
    assert tuple(coco_eval.MAX_DETS) == tuple(Q.MAX_DETS) and coco_eval.AREA_RNG == Q.AREA_RNG
    cases = [CC.checked_set(task)[2]] + [Q.evaluate(*CC.hand_case(n), task) for n in sorted(KNOWN)]
    for n, e in enumerate(cases):
        K = 3 if n == 0 else 1
        precision, recall = coco_eval.accumulate(Q.tables_of(e["groups"]), K)
        assert np.array_equal(precision, e["precision"]), n
        assert np.array_equal(recall, e["recall"]), n
        assert np.array_equal(coco_eval.summarize(precision, recall), e["stats"]), n


def test_evaluator_construction_and_error_paths():
    import afigan_amd as amd
    gt, res = CC.hand_case("A")
    ev = amd.COCOEvaluator(gt)
    assert ev.evaluate() == {}                                                     # nothing processed
    ev.process([], [])
    assert ev.evaluate() == {}
    with pytest.raises(amd.AfiError, match="image id"):
        ev.process([{"image_id": 99}], [{"instances": []}])
    ev.process([{"image_id": 1}], [{"instances": [dict(res[0], image_id=98)]}])    # a result's own image id is looked at when the groups are built
    with pytest.raises(amd.AfiError, match="image id 98"):
        ev.evaluate()
    ev.reset()
    ev.process([{"image_id": 1}], [{"instances": []}])                             # an image without detections: every metric is nan
    out = ev.evaluate()
    assert list(out) == ["bbox"] and list(out["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl"] and all(np.isnan(v) for v in out["bbox"].values())
    poly = {"images": gt["images"], "categories": gt["categories"], "annotations": [dict(gt["annotations"][0], segmentation=[[10, 10, 60, 10, 60, 60]])]}
    amd.COCOEvaluator(poly, tasks=("bbox",))                                       # polygons do not matter to bbox
    with pytest.raises(amd.AfiError, match="polygon"):
        amd.COCOEvaluator(poly, tasks=("bbox", "segm"))
    with pytest.raises(amd.AfiError, match="tasks"):
        amd.COCOEvaluator(gt, tasks=("keypoints",))
    with pytest.raises(amd.AfiError, match="annotation dict"):
        amd.COCOEvaluator({"images": []})
    with pytest.raises(amd.AfiError, match="class names"):
        amd.COCOEvaluator(gt, class_names=["a", "b"])


def test_entry_point_return_codes():
    from afigan_amd import _lib
    lib = _lib.load()
    OK, BAD, UNS = 0, _lib.DEFINES["AFI_ERR_BAD_ARG"], _lib.DEFINES["AFI_ERR_UNSUPPORTED"]
    assert _lib.ABI_VERSION == 9 and lib.afi_abi_version() == 9
    p, odd = 0x1000, 0x1001
    box = lib.afi_coco_box_iou
    assert box(p, p, p, p, p, p, 0, 0, p, None) == OK and box(p, p, p, p, p, p, 3, 0, p, None) == OK          # nothing to do
    for i in (0, 1, 2, 3, 4, 5, 8):
        args = [p, p, p, p, p, p, 2, 6, p, None]
        args[i] = None
        assert box(*args) == BAD, i
    assert box(p, p, p, p, p, p, -1, 6, p, None) == BAD and box(p, p, p, p, p, p, 2, -6, p, None) == BAD
    assert box(odd, p, p, p, p, p, 2, 6, p, None) == UNS and box(p, p, p, p, p, odd, 2, 6, p, None) == UNS
    area = lib.afi_coco_rle_area
    assert area(p, p, p, 0, p, None) == OK and area(p, p, p, -1, p, None) == BAD
    for i in (0, 1, 2, 4):
        args = [p, p, p, 3, p, None]
        args[i] = None
        assert area(*args) == BAD, i
    assert area(p + 2, p, p, 3, p, None) == UNS and area(p, p + 4, p, 3, p, None) == UNS
    riou = lib.afi_coco_rle_iou
    good = [p, p, p, p, p, p, p, p, p, p, p, p, 2, 6, p, p, None]
    assert riou(*good[:12], 0, 6, p, p, None) == OK and riou(*good[:12], 2, 0, p, p, None) == OK
    assert riou(*good[:12], -2, 6, p, p, None) == BAD and riou(*good[:12], 2, -1, p, p, None) == BAD
    for i in list(range(12)) + [15]:
        args = list(good)
        args[i] = None
        assert riou(*args) == BAD, i
    assert riou(*good[:14], None, p + 4, None) == UNS                       # inter may be null; iou must be 8-byte aligned
    ws = lib.afi_coco_match_ws_bytes
    assert ws(0, 4, 10) == 0 and ws(75, 4, 10) == 3000 and ws(-1, 4, 10) == -1 and ws(5, 0, 10) == -1 and ws(5, 4, 0) == -1 and ws(5, 65, 64) == -1
    match = lib.afi_coco_match
    good = [p, p, p, p, 2, p, p, p, 7, 5, p, 4, p, 10, 5, p, p, p, p, 200, None]
    assert match(*good[:4], 0, *good[5:]) == OK
    for i in (0, 1, 2, 3, 5, 6, 7, 10, 12, 15, 16, 17, 18):
        args = list(good)
        args[i] = None
        assert match(*args) == BAD, i
    for i, v in ((4, -1), (8, -1), (9, -1), (11, 0), (13, 0), (14, -1), (19, 199)):   # negative counts, no range / threshold, a workspace one byte short
        args = list(good)
        args[i] = v
        assert match(*args) == BAD, (i, v)
    args = list(good)
    args[0] = odd
    assert match(*args) == UNS
    args = list(good)
    args[11], args[13], args[19] = 65, 64, 1 << 30
    assert match(*args) == UNS
    args = list(good)
    args[14] = 1 << 30                                                      # A max_g past 2^31
    assert match(*args) == UNS
