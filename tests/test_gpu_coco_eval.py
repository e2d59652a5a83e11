"""COCO box / mask AP on the GPU (csrc/coco_eval.hip, ops.coco_*, afigan_amd.COCOEvaluator) against the plain-loop fp64 checker
tests/coco_eval_f64.py.  The IoU matrices, intersections, areas and match tables are compared for equality -- the kernels are fp64 with contraction
off, so there is no tolerance -- and precision / recall / stats within 1e-12 (they are sums of at most 1010 such terms; in fact they come out
equal).  tests/test_coco_eval_host.py proves on the checker alone that the seeded set holds what is needed here: a group without detections, one
without GTs, 130 detections cut to 100, 70 GTs, tied scores, two crowds matched several times, areas on both sides of 32^2 and 96^2, the hand
cases G and H."""
import numpy as np
import pytest
import torch

import coco_eval_cases as CC
import coco_eval_f64 as Q

pytestmark = pytest.mark.gpu
TASKS = ("bbox", "segm")


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


_TABLES = {}


def _device_tables(amd, task, fresh=False):
    """COCOEvaluator.match_tables of the synthetic set (once per task unless `fresh`)."""
    if fresh or task not in _TABLES:
        gt, res, _ = CC.checked_set(task)
        t = amd.COCOEvaluator(gt, tasks=(task,)).match_tables(res, task)
        if fresh:
            return t
        _TABLES[task] = t
    return _TABLES[task]


def _evaluate(amd, gt, res, task):
    ev = amd.COCOEvaluator(gt, tasks=(task,), class_names=[c["name"] for c in gt["categories"]])
    by_image = {}
    for r in res:
        by_image.setdefault(r["image_id"], []).append(r)
    ids = [im["id"] for im in gt["images"]]
    ev.process([{"image_id": i} for i in ids], [{"instances": by_image.get(i, [])} for i in ids])
    return ev, ev.evaluate()


@pytest.mark.parametrize("task", TASKS)
def test_iou_matrices_equal_the_checker(amd, task):
    _, _, e = CC.checked_set(task)
    t = _device_tables(amd, task)
    assert len(t["cat"]) == len(e["groups"]) == 17 and t["iou"].dtype == np.float64
    pairs = 0
    for n, g in enumerate(e["groups"]):
        D, G = len(g["dts"]), len(g["gts"])
        assert (t["dt_off"][n + 1] - t["dt_off"][n], t["gt_off"][n + 1] - t["gt_off"][n], t["cat"][n]) == (D, G, g["k"]), n
        got = t["iou"][t["iou_off"][n]:t["iou_off"][n + 1]].reshape(D, G)
        assert np.array_equal(got, g["iou"]), (n, np.abs(got - g["iou"]).max())
        assert np.array_equal(t["dt_area"][t["dt_off"][n]:t["dt_off"][n + 1]], np.array(g["dt_area"], np.float64)), n
        pairs += D * G
    print(f"[coco] {task}: {len(e['groups'])} groups, {pairs} pairs, {int((t['iou'] > 0).sum())} overlapping")
    assert (t["iou"] > 0).sum() > 200 and (t["iou"] == 0).sum() > 200


def _pasted_runs():
    """Run starts of 13 pasted masks on a 130 x 40 canvas from ops.mask_paste_rle (three 64-row words): (starts list per mask, n)."""
    from afigan_amd import ops
    H, W, M = 130, 40, 28
    g = torch.Generator().manual_seed(23)
    b = torch.rand((13, 4), generator=g)
    boxes = torch.stack([b[:, 0] * W * 0.5, b[:, 1] * H * 0.5, W * (0.5 + 0.5 * b[:, 2]), H * (0.5 + 0.5 * b[:, 3])], 1)
    boxes[0] = torch.tensor([0.0, 0.0, W, H])
    low = torch.randn((13, 1, 5, 5), generator=g) * 2.0
    probs = torch.sigmoid(torch.nn.functional.interpolate(low, size=(M, M), mode="bilinear", align_corners=False))[:, 0].contiguous()
    probs[0] = 1.0                                                          # the full mask
    probs[1] = 0.0                                                          # the empty mask
    starts, nstarts = ops.mask_paste_rle(probs.cuda(), boxes.cuda(), (H, W))
    s, k = starts.cpu().numpy().tolist(), np.concatenate(([0], np.cumsum(nstarts.numpy())))
    return [s[k[i]:k[i + 1]] for i in range(13)], H * W


def _random_runs(n, seed):
    rng = np.random.default_rng(seed)
    out = [[], [0], [n - 1], [0, 1, n - 1], [5, 9, 9, 9, 14, 20]]            # empty, full, the last pixel alone / after a first, an empty run
    for k in (1, 2, 7, 40, 41, 300):
        out.append(sorted(rng.choice(n, size=k, replace=False).tolist()))
    return out


def _rle_side(lists, n):
    flat = np.array([v for s in lists for v in s], np.int32)
    off = np.concatenate(([0], np.cumsum([len(s) for s in lists]))).astype(np.int64)
    return torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda(), torch.full((len(lists),), n, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("source", ("pasted", "random"))
def test_rle_area_and_iou_equal_the_checker(amd, source):
    from afigan_amd import ops
    if source == "pasted":
        lists, n = _pasted_runs()
        print(f"[coco] pasted masks: starts per mask {[len(s) for s in lists]}")
        assert lists[0] == [0] and lists[1] == [] and sum(len(s) > 2 for s in lists) >= 6
    else:
        n = 130 * 40
        lists = _random_runs(n, 7)
    dts, gts = lists, lists[::-1]
    crowd = [i % 3 == 0 for i in range(len(gts))]                            # crowd pairs among them
    d, g = _rle_side(dts, n), _rle_side(gts, n)
    da, ga = ops.coco_rle_area(*d), ops.coco_rle_area(*g)
    assert da.dtype == torch.int64 and da.cpu().tolist() == [Q.rle_area(s, n) for s in dts] and ga.cpu().tolist() == [Q.rle_area(s, n) for s in gts]
    D, G = len(dts), len(gts)
    # two groups: rows 0 .. 3 against all GTs, the rest against all GTs but the first two
    off = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")       # noqa: E731
    d_off, g_off, i_off = [0, 4, D], [0, G, G], [0, 4 * G, 4 * G]
    iou, inter = ops.coco_rle_iou(d + (da,), g + (ga,), torch.tensor(crowd, dtype=torch.uint8, device="cuda"), off(d_off), off(g_off), off(i_off),
                                  4 * G, want_inter=True)
    want_i, want_o = Q.rle_iou([(s, n) for s in dts[:4]], [(s, n) for s in gts], crowd)
    assert np.array_equal(inter.cpu().numpy().reshape(4, G), want_i) and np.array_equal(iou.cpu().numpy().reshape(4, G), want_o)
    d_off, g_off = [0, 4, D], [0, 2, G]
    i_off = [0, 8, 8 + (D - 4) * (G - 2)]
    iou, inter = ops.coco_rle_iou(d + (da,), g + (ga,), torch.tensor(crowd, dtype=torch.uint8, device="cuda"), off(d_off), off(g_off), off(i_off),
                                  i_off[-1], want_inter=True)
    a_i, a_o = Q.rle_iou([(s, n) for s in dts[:4]], [(s, n) for s in gts[:2]], crowd[:2])
    b_i, b_o = Q.rle_iou([(s, n) for s in dts[4:]], [(s, n) for s in gts[2:]], crowd[2:])
    assert np.array_equal(inter.cpu().numpy(), np.concatenate((a_i.reshape(-1), b_i.reshape(-1))))
    assert np.array_equal(iou.cpu().numpy(), np.concatenate((a_o.reshape(-1), b_o.reshape(-1))))
    assert (want_i > 0).sum() > 4 and (want_i == 0).sum() > 4
    # masks of different sizes: -1
    g2 = (g[0], g[1], torch.full((G,), n + 1, dtype=torch.int32, device="cuda"))
    iou = ops.coco_rle_iou(d + (da,), g2 + (ga,), torch.zeros((G,), dtype=torch.uint8, device="cuda"), off([0, D]), off([0, G]), off([0, D * G]), D * G)
    assert (iou == -1).all()


@pytest.mark.parametrize("task", TASKS)
def test_match_tables_equal_the_checker(amd, task):
    _, _, e = CC.checked_set(task)
    t = _device_tables(amd, task)
    want = Q.tables_of(e["groups"])
    assert t["dt_match"].dtype == np.int32 and t["dt_ignore"].dtype == np.uint8 and t["gt_ignore"].dtype == np.uint8
    for k in ("dt_match", "dt_ignore", "gt_ignore"):
        assert t[k].shape == want[k].shape, k
        bad = np.argwhere(t[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:5].tolist())
    assert np.array_equal(t["scores"], want["scores"])
    assert (t["dt_match"] >= 0).any() and (t["dt_match"] < 0).any() and t["dt_ignore"].any() and t["gt_ignore"][0].any()


@pytest.mark.parametrize("task", TASKS)
def test_evaluate_equals_the_checker(amd, task):
    gt, res, e = CC.checked_set(task)
    ev, out = _evaluate(amd, gt, res, task)
    for name, got, want in (("precision", ev.precision[task], e["precision"]), ("recall", ev.recall[task], e["recall"]), ("stats", ev.stats[task], e["stats"])):
        err = float(np.abs(got - want).max())
        print(f"[coco] {task} {name}: max abs difference {err:.3e}")
        assert got.shape == want.shape and err <= 1e-12, name
    assert list(out) == [task] and list(out[task])[:6] == ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    for i, m in enumerate(("AP", "AP50", "AP75", "APs", "APm", "APl")):
        assert (np.isnan(out[task][m]) and e["stats"][i] == -1) or abs(out[task][m] - 100 * e["stats"][i]) <= 1e-10
    for k, c in enumerate(gt["categories"]):
        p = e["precision"][:, :, k, 0, -1]
        assert abs(out[task]["AP-" + c["name"]] - 100 * float(np.mean(p[p > -1]))) <= 1e-10


@pytest.mark.parametrize("task", TASKS)
def test_known_answers_from_the_device_path(amd, task):
    from test_coco_eval_host import KNOWN
    from afigan_amd import rle
    for name in ("A", "B", "C", "D", "D-crowd-only", "E"):
        gt, res = CC.hand_case(name)
        if task == "segm":                                                  # the string form, as a detector's results carry it
            for x in gt["annotations"] + res:
                x["segmentation"] = {"size": x["segmentation"]["size"], "counts": rle.to_string(x["segmentation"]["counts"])}
                x.pop("bbox")                                               # not consulted for segm
        ev, out = _evaluate(amd, gt, res, task)
        assert np.abs(ev.stats[task] - np.array(KNOWN[name], np.float64)).max() < 1e-12, (name, ev.stats[task])
        assert "AP-c1" not in out[task]                                     # one class name: no per-category rows


@pytest.mark.parametrize("task", TASKS)
def test_dirty_workspaces_and_two_runs(amd, task, monkeypatch):
    from afigan_amd import ops
    a = _device_tables(amd, task)
    b = _device_tables(amd, task, fresh=True)
    monkeypatch.setattr(ops, "new_workspace", lambda floats, device: torch.full((int(floats) * 4,), 0xFF, dtype=torch.uint8, device=device).view(torch.float32))
    c = _device_tables(amd, task, fresh=True)
    for k in ("iou", "dt_area", "dt_match", "dt_ignore", "gt_ignore", "scores"):
        assert np.array_equal(a[k], b[k]), ("second run", k)
        assert np.array_equal(a[k], c[k]), ("0xFF-filled workspace", k)


def test_coco_match_workspace_argument(amd):
    from afigan_amd import ops
    cu = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")             # noqa: E731
    iou = cu([0.9, 0.6, 0.2, 0.7], torch.float64)                           # one group, D = 2, G = 2
    args = (iou, cu([0, 2], torch.int64), cu([0, 2], torch.int64), cu([0, 4], torch.int64), cu([100.0, 100.0], torch.float64),
            cu([100.0, 100.0], torch.float64), cu([0, 0], torch.uint8), cu(Q.AREA_RNG, torch.float64), cu(Q.IOU_THRS.tolist(), torch.float64))
    n = amd._lib.load().afi_coco_match_ws_bytes(2, 4, 10)
    assert n == 80
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    dtm, dti, gti = ops.coco_match(*args, ws=ws)
    want = Q.match(iou.cpu().numpy().reshape(2, 2), [100.0] * 2, [100.0] * 2, [0, 0])
    assert np.array_equal(dtm.cpu().numpy(), want[0]) and np.array_equal(dti.cpu().numpy(), want[1]) and np.array_equal(gti.cpu().numpy(), want[2])
    assert dtm[0, 0].tolist() == [0, 1] and dtm[0, 5].tolist() == [0, -1]
    with pytest.raises(amd.AfiError, match="ws must be"):
        ops.coco_match(*args, ws=ws[:n - 1])
    with pytest.raises(amd.AfiError, match="GPU"):
        ops.coco_match(iou.cpu(), *args[1:])


@pytest.mark.parametrize("G", (64, 65, 70))
def test_coco_match_on_a_dirty_workspace_across_the_64_gt_edge(amd, G):
    """ops.coco_match itself on one group of G GTs and 9 detections plus a small second group, the workspace full of 0xFF and then reused: G = 64
    is the last group of the register kernel, 65 and 70 go through the workspace."""
    from afigan_amd import ops
    rng = np.random.default_rng(100 + G)
    D, D2, G2 = 9, 3, 2
    iou = [np.round(rng.random((D, G)), 2), np.round(rng.random((D2, G2)), 2)]           # a grid of 0.01: ties among the GTs
    crowd = [(rng.random(G) < 0.1).astype(np.uint8), np.zeros(G2, np.uint8)]
    gt_area = [rng.choice([500.0, 1024.0, 5000.0, 20000.0], G), np.array([100.0, 5000.0])]
    dt_area = [rng.choice([500.0, 5000.0, 20000.0], D), np.array([100.0, 100.0, 5000.0])]
    want = [Q.match(iou[i], dt_area[i], gt_area[i], crowd[i]) for i in range(2)]
    cu = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).cuda()       # noqa: E731
    args = (cu(np.concatenate([m.reshape(-1) for m in iou]), np.float64), cu([0, D, D + D2], np.int64), cu([0, G, G + G2], np.int64),
            cu([0, D * G, D * G + D2 * G2], np.int64), cu(np.concatenate(dt_area), np.float64), cu(np.concatenate(gt_area), np.float64),
            cu(np.concatenate(crowd), np.uint8), cu(Q.AREA_RNG, np.float64), cu(Q.IOU_THRS, np.float64))
    n = amd._lib.load().afi_coco_match_ws_bytes(G + G2, 4, 10)
    assert n == 40 * (G + G2)
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    for round_, max_g in (("0xFF-filled", G), ("reused", None)):
        dtm, dti, gti = (t.cpu().numpy() for t in ops.coco_match(*args, max_g=max_g, ws=ws))
        for k, got in enumerate((dtm, dti, gti)):
            assert np.array_equal(got, np.concatenate([want[0][k], want[1][k]], axis=-1)), (round_, k)
    assert (dtm >= 0).any() and (dtm < 0).any() and bool(ws.ne(0xFF).any()) == (G > 64)     # only groups of more than 64 GTs touch the workspace


def test_detector_outputs_under_both_mask_formats_evaluate_alike(amd):
    """The 64 x 80 toy detector of tests/test_gpu_rle.py, built again here; its own confident detections serve as the ground truth."""
    from afigan_amd import rle
    from afigan_amd.fpn_sr import ShapeSpec
    from test_gpu_mask import LEVELS4, _heads
    from test_gpu_rpn import _rpn

    class Backbone(torch.nn.Module):
        size_divisibility = 32

        def output_shape(self):
            return {f: ShapeSpec(channels=32, stride=2 ** int(f[1:])) for f in LEVELS4}

        def forward(self, x):
            return {f: torch.nn.functional.avg_pool2d(x, 2 ** int(f[1:])).repeat(1, 11, 1, 1)[:, :32].contiguous() for f in LEVELS4}

    rpn = _rpn(amd, LEVELS4, 32, (32, 64, 128, 256), pre_k=300, post_k=100, seed=9)
    heads = _heads(amd, LEVELS4, 32, K=5, S=7, fc=64, Sm=14, num_conv=1, conv_dim=16, seed=61)
    g = torch.Generator().manual_seed(61)
    with torch.no_grad():
        heads.box_predictor.cls_score.weight.copy_(torch.randn(heads.box_predictor.cls_score.weight.shape, generator=g))
        heads.box_predictor.bbox_pred.weight.copy_(torch.randn(heads.box_predictor.bbox_pred.weight.shape, generator=g) * 0.3)
        heads.mask_head.predictor.bias.fill_(0.3)
    det = amd.GeneralizedRCNN_AFExtractor(backbone=Backbone(), proposal_generator=rpn, roi_heads=heads, pixel_mean=[100.0, 110.0, 120.0],
                                          pixel_std=[50.0, 55.0, 60.0]).eval()
    inputs = [{"image_x0.5": torch.rand((3, 64, 80), generator=g) * 255, "height": 128, "width": 160, "image_id": 7},
              {"image_x0.5": torch.rand((3, 57, 71), generator=g) * 255, "height": 114, "width": 142, "image_id": 8}]
    with torch.no_grad():
        bit = det.inference(inputs)
        run = det.inference(inputs, mask_format="rle")
    gt = {"images": [{"id": i["image_id"], "height": i["height"], "width": i["width"]} for i in inputs],
          "categories": [{"id": c, "name": f"k{c}"} for c in range(5)], "annotations": []}
    n_dt = 0
    for inp, o in zip(inputs, bit):
        rs = amd.instances_to_coco_json(o["instances"], inp["image_id"])
        n_dt += len(rs)
        for r in rs[::2]:                                                   # every other detection is "true"
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": r["bbox"],
                                      "iscrowd": 0, "area": float(rle.area(r["segmentation"])), "segmentation": r["segmentation"]})
    assert n_dt >= 4 and len(gt["annotations"]) >= 2, "too few detections: the test would show nothing"
    outs = []
    for o in (bit, run):
        ev = amd.COCOEvaluator(gt, tasks=("bbox", "segm"), class_names=[c["name"] for c in gt["categories"]])
        ev.process(inputs, o)
        outs.append((ev.evaluate(), ev))
    (ra, ea), (rb, eb) = outs
    assert list(ra) == ["bbox", "segm"] and list(ra) == list(rb)
    for task in TASKS:
        assert np.array_equal(ea.precision[task], eb.precision[task]) and np.array_equal(ea.recall[task], eb.recall[task])
        assert np.array_equal(ea.stats[task], eb.stats[task])
        assert {k: v for k, v in ra[task].items() if not np.isnan(v)} == {k: v for k, v in rb[task].items() if not np.isnan(v)}
        assert [k for k, v in ra[task].items() if np.isnan(v)] == [k for k, v in rb[task].items() if np.isnan(v)]
        assert ra[task]["AP50"] > 0, (task, ra[task])                       # every GT is a detection, so some of them match
