"""COCO polygons as run starts on the GPU (csrc/poly_rle.hip, ops.polygons_rle / ops.rle_decode, rle.from_polygons, COCOEvaluator's
rasterize_polygons, DualScaleMapper's bitmask format) against the plain-loop checker tests/poly_f64.py.  Every comparison of starts, counts,
strings and pixels is for equality: after the first step of the algorithm everything is an integer.  tests/test_poly_host.py shows on the checker
alone that the inputs hold what is needed here (among it: at least 3 polygons that a contracted kernel would rasterise differently)."""
import numpy as np
import pytest
import torch

import poly_cases as PC
import poly_f64 as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


def _lists(starts, start_off):
    s, o = starts.cpu().numpy().tolist(), start_off.cpu().numpy().tolist()
    return [s[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def test_random_polygons_equal_the_checker(amd):
    from afigan_amd import ops, rle
    cases, want = PC.random_set(), PC.random_set_starts()
    fused = PC.random_set_starts(fused=True)
    assert sum(a != b for a, b in zip(want, fused)) >= 3, "the set cannot tell a contracted kernel from the stated arithmetic"
    polys, sizes = [[p] for p, _ in cases], [hw for _, hw in cases]
    starts, off, hw = ops.polygons_rle(polys, sizes)
    assert starts.dtype == torch.int32 and off.dtype == torch.int64 and hw.dtype == torch.int32 and starts.is_cuda and off.is_cuda and hw.is_cuda
    assert hw.cpu().tolist() == [h * w for h, w in sizes] and off.shape == (len(cases) + 1,)
    got = _lists(starts, off)
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, (len(bad), bad[:5], cases[bad[0]], got[bad[0]], want[bad[0]])
    # the triple feeds the evaluation kernels as it is
    assert ops.coco_rle_area(starts, off, hw).cpu().tolist() == [int(Q.mask_of_starts(s, h, w).sum()) for s, (h, w) in zip(want, sizes)]
    strings = rle.from_polygons(polys, sizes)
    for i, ((p, (H, W)), r) in enumerate(zip(cases, strings)):
        assert r == rle.to_rle(Q.ann_counts([p], H, W), (H, W)), i
    assert amd.polygons_to_rle(polys[:3], sizes[:3]) == strings[:3]


def test_union_of_an_annotations_polygons(amd):
    from afigan_amd import ops, rle
    cases, want = PC.union_set(), PC.union_set_starts()
    polys, sizes = [ps for ps, _, _ in cases], [hw for _, hw, _ in cases]
    got = _lists(*ops.polygons_rle(polys, sizes)[:2])
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, cases[i][2], a, b)
    for (ps, (H, W), what), r in zip(cases, rle.from_polygons(polys, sizes)):
        assert r == rle.to_rle(Q.ann_counts(ps, H, W), (H, W)), what
    # one common size given once
    same = [ps for ps, hw, _ in cases if hw == (16, 18)]
    assert _lists(*ops.polygons_rle(same, (16, 18))[:2]) == [s for s, (_, hw, _) in zip(want, cases) if hw == (16, 18)]


@pytest.mark.parametrize("delta,extra", ((-2, False), (0, False), (2, False), (2, True)))
def test_both_sort_paths_at_the_lds_capacity(amd, delta, extra):
    """A zigzag whose crossings are the LDS capacity - 2 and the capacity itself (sorted in LDS) and the capacity + 2 (sorted in the workspace), between small masks
    so that the offsets count.  The number of crossings of closed boundaries is even, so +-2 are the nearest neighbours of the capacity.
    extra: a box across the zigzag as a second polygon, so that the workspace path sorts twice and sweeps a union."""
    from afigan_amd import ops
    cap = amd._lib.DEFINES["AFI_POLY_RLE_LDS_CAP"]
    xy, (H, W) = PC.zigzag_case(cap + delta)
    assert len(Q.crossings(xy, H, W)) == cap + delta
    big = [xy, [3.0, 2.0, W - 3.5, 2.0, W - 3.5, 5.0, 3.0, 5.0]] if extra else [xy]
    small = PC.union_set()[:4]
    polys = [ps for ps, _, _ in small[:2]] + [big] + [ps for ps, _, _ in small[2:]]
    sizes = [hw for _, hw, _ in small[:2]] + [(H, W)] + [hw for _, hw, _ in small[2:]]
    want = PC.union_set_starts()[:2] + [Q.ann_starts(big, H, W)] + PC.union_set_starts()[2:4]
    got = _lists(*ops.polygons_rle(polys, sizes)[:2])
    assert [len(g) for g in got] == [len(w) for w in want]
    assert got == want
    assert len(want[2]) > cap // 2


@pytest.mark.parametrize("H,W", ((37, 65), (1, 70), (70, 1), (64, 64), (16, 130)))
def test_decode_equals_the_checker(amd, H, W):
    from afigan_amd import ops
    rng = np.random.default_rng(H * 1000 + W)
    polys = [[PC._polygon(rng, H, W) for _ in range(1 + i % 3)] for i in range(5)] + [[], [[-3.0, -3.0, W + 3.0, -3.0, W + 3.0, H + 3.0, -3.0, H + 3.0]]]
    starts, off, _ = ops.polygons_rle(polys, (H, W))
    out = torch.full((len(polys), H, W), 0xFF, dtype=torch.uint8, device="cuda")                 # every byte is written
    got = ops.rle_decode(starts, off, (H, W), out=out)
    assert got.dtype == torch.bool and tuple(got.shape) == (len(polys), H, W) and got.data_ptr() == out.data_ptr()
    assert set(out.unique().cpu().tolist()) <= {0, 1}
    for i, ps in enumerate(polys):
        assert np.array_equal(got[i].cpu().numpy(), Q.ann_mask(ps, H, W)), i
    assert not got[5].any() and got[6].all()
    # starts that no polygon made: an empty run (equal neighbours) and the last pixel alone
    lists = [[], [0], [H * W - 1], [2, 5, 5, 5, 9, 12] if H * W > 12 else []]
    flat = torch.tensor([v for s in lists for v in s], dtype=torch.int32, device="cuda")
    o = torch.tensor(np.concatenate(([0], np.cumsum([len(s) for s in lists]))), dtype=torch.int64, device="cuda")
    got = ops.rle_decode(flat, o, (H, W)).cpu().numpy()
    for i, s in enumerate(lists):
        assert np.array_equal(got[i], Q.mask_of_starts(s, H, W)), i
    assert not ops.rle_decode(torch.zeros((0,), dtype=torch.int32, device="cuda"), torch.zeros((4,), dtype=torch.int64, device="cuda"), (H, W)).any()
    assert tuple(ops.rle_decode(flat[:0], o[:1], (H, W)).shape) == (0, H, W)


def test_dirty_workspaces_two_runs_and_no_annotation(amd, monkeypatch):
    from afigan_amd import ops
    cap = amd._lib.DEFINES["AFI_POLY_RLE_LDS_CAP"]
    xy, hw = PC.zigzag_case(cap + 2)                                          # both sort paths in the call
    polys = [ps for ps, _, _ in PC.union_set()] + [[xy]]
    sizes = [s for _, s, _ in PC.union_set()] + [hw]
    a = ops.polygons_rle(polys, sizes)
    b = ops.polygons_rle(polys, sizes)
    for fill in (0xFF, 0x7F):
        monkeypatch.setattr(ops, "new_workspace", lambda floats, device: torch.full((int(floats) * 4,), fill, dtype=torch.uint8, device=device).view(torch.float32))
        c = ops.polygons_rle(polys, sizes)
        assert all(torch.equal(x, y) for x, y in zip(a, c)), fill
    monkeypatch.undo()
    nan = torch.full((amd._lib.load().afi_poly_rle_ws_bytes(int(ops.polygons_batch(polys, sizes)[4][-1])) // 4 + 2,), float("nan"), device="cuda")
    d = ops.polygons_rle(polys, sizes, ws=nan)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x, y) for x, y in zip(a, d))
    with pytest.raises(amd.AfiError, match="ws must be"):
        ops.polygons_rle(polys, sizes, ws=nan[:8])
    starts, off, n = ops.polygons_rle([], (8, 8))                             # N = 0
    assert starts.shape == (0,) and off.cpu().tolist() == [0] and n.shape == (0,) and starts.is_cuda
    starts, off, n = ops.polygons_rle([[], []], [(8, 8), (3, 4)])            # annotations without a polygon
    assert starts.shape == (0,) and off.cpu().tolist() == [0, 0, 0] and n.cpu().tolist() == [64, 12]


# ------------------------------------------------------------------------------------------------ the evaluator
EV_SIZES = {3: (40, 37), 5: (33, 50), 8: (64, 48)}
EV_CATS = (1, 4)


def _evaluator_set():
    """A small set whose ground truth is polygons (1 to 3 per annotation, some reaching outside the image), with one crowd given as uncompressed
    RLE; the results are the checker's masks of jittered polygons.  Returns (gt with polygons, results, gt with the checker's RLE)."""
    from coco_eval_cases import counts_of
    rng = np.random.default_rng(77)
    gt = {"images": [{"id": i, "height": h, "width": w} for i, (h, w) in EV_SIZES.items()], "categories": [{"id": c, "name": f"c{c}"} for c in EV_CATS],
          "annotations": []}
    res = []

    def blob(H, W):
        cx, cy, r = rng.uniform(4, W - 4), rng.uniform(4, H - 4), rng.uniform(3, min(H, W) / 2.5)
        k = int(rng.integers(4, 9))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = r * rng.uniform(0.6, 1.0, k)
        return np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).reshape(-1) * 4) / 4

    for img, (H, W) in EV_SIZES.items():
        for cat in EV_CATS:
            for n in range(int(rng.integers(2, 6))):
                ps = [blob(H, W).tolist() for _ in range(int(rng.integers(1, 4)))]
                m = Q.ann_mask(ps, H, W)
                gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": img, "category_id": cat, "iscrowd": 0, "area": float(m.sum()),
                                          "bbox": [0.0, 0.0, 1.0, 1.0], "segmentation": ps, "_mask": m})
                for _ in range(int(rng.integers(0, 4))):
                    qs = [(np.asarray(p) + np.round(rng.normal(0, 1.0, len(p)) * 2) / 2).tolist() for p in ps]
                    dm = Q.ann_mask(qs, H, W)
                    res.append({"image_id": img, "category_id": cat, "score": float(rng.integers(1, 20)) / 20,
                                "segmentation": {"size": [H, W], "counts": counts_of(dm)}})
    H, W = EV_SIZES[5]
    crowd = np.zeros((H, W), bool)
    crowd[5:25, 10:40] = True
    gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": 5, "category_id": 4, "iscrowd": 1, "area": float(crowd.sum()),
                              "bbox": [10.0, 5.0, 30.0, 20.0], "segmentation": {"size": [H, W], "counts": counts_of(crowd)}, "_mask": crowd})
    for n in range(3):
        dm = np.zeros((H, W), bool)
        dm[8 + 4 * n:14 + 4 * n, 12 + 6 * n:22 + 6 * n] = True
        res.append({"image_id": 5, "category_id": 4, "score": 0.5, "segmentation": {"size": [H, W], "counts": counts_of(dm)}})
    as_rle = dict(gt, annotations=[dict(a, segmentation={"size": list(a["_mask"].shape), "counts": counts_of(a["_mask"])}) for a in gt["annotations"]])
    return gt, res, as_rle


def _run(amd, gt, res, **kw):
    ev = amd.COCOEvaluator(gt, tasks=("segm",), **kw)
    by_image = {}
    for r in res:
        by_image.setdefault(r["image_id"], []).append(r)
    ids = [im["id"] for im in gt["images"]]
    ev.process([{"image_id": i} for i in ids], [{"instances": by_image.get(i, [])} for i in ids])
    ev.evaluate()
    return ev


def test_evaluator_on_polygon_ground_truth(amd, monkeypatch):
    import coco_eval_f64 as CQ
    from afigan_amd import ops, rle
    gt, res, as_rle = _evaluator_set()
    assert sum(isinstance(a["segmentation"], list) for a in gt["annotations"]) >= 15 and sum(a["iscrowd"] for a in gt["annotations"]) == 1 and len(res) >= 20
    with pytest.raises(amd.AfiError, match="rasterize_polygons=True"):
        amd.COCOEvaluator(gt, tasks=("segm",))
    calls = []
    real = ops.polygons_rle
    monkeypatch.setattr(ops, "polygons_rle", lambda *a, **k: (calls.append(len(a[0])), real(*a, **k))[1])
    a = _run(amd, gt, res, rasterize_polygons=True)
    assert calls == [len(gt["annotations"]) - 1], "one batched call for all polygon annotations"
    monkeypatch.undo()
    # the same annotations converted beforehand
    pa = [x for x in gt["annotations"] if isinstance(x["segmentation"], list)]
    conv = rle.from_polygons([x["segmentation"] for x in pa], [EV_SIZES[x["image_id"]] for x in pa])
    it = iter(conv)
    gt2 = dict(gt, annotations=[dict(x, segmentation=next(it)) if isinstance(x["segmentation"], list) else x for x in gt["annotations"]])
    b = _run(amd, gt2, res)
    want = CQ.evaluate(as_rle, res, "segm")
    for name, x, y, w in (("precision", a.precision["segm"], b.precision["segm"], want["precision"]), ("recall", a.recall["segm"], b.recall["segm"], want["recall"]),
                          ("stats", a.stats["segm"], b.stats["segm"], want["stats"])):
        assert np.array_equal(x, y), name
        err = float(np.abs(x - w).max())
        print(f"[poly] evaluator {name}: max abs difference from the checker {err:.3e}")
        assert x.shape == w.shape and np.array_equal(x, w), name
    assert 0 < a.stats["segm"][0] < 1 and a.stats["segm"][1] > a.stats["segm"][0]


# ------------------------------------------------------------------------------------------------ the mapper
def _sample():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(60, 84, 3), dtype=np.uint8)
    box = lambda x0, y0, x1, y1: [float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]   # noqa: E731
    segs = [[box(5, 6, 40, 30)], [box(50, 10, 70, 50), [20.0, 40.0, 45.0, 42.5, 30.0, 57.0]], [[60.5, 3.25, 80.0, 8.0, 70.0, 30.75, 55.0, 20.0]],
            [[10.0, 20.0, 10.0, 40.0, 10.0, 30.0]],                            # no width (its box below has one): an empty mask at every scale
            [box(30.0, 30.0, 31.2, 50.0)],                                     # a sliver: whether it holds a pixel-centre column depends on the scale
            [[2.0, 50.0, 20.0, 44.0, 12.0, 58.0]]]
    annos = []
    for i, s in enumerate(segs):
        xs, ys = np.concatenate([np.asarray(p)[0::2] for p in s]), np.concatenate([np.asarray(p)[1::2] for p in s])
        annos.append({"bbox": [float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max())], "bbox_mode": 0, "category_id": i % 3, "iscrowd": 0,
                      "segmentation": s})
    annos[3]["bbox"] = [8.0, 20.0, 12.0, 40.0]
    annos.append({"bbox": [1.0, 1.0, 9.0, 9.0], "bbox_mode": 0, "category_id": 1, "iscrowd": 1, "segmentation": [box(1, 1, 9, 9)]})
    return {"image": img, "annotations": annos}


@pytest.mark.parametrize("seed", (0, 1))
def test_mapper_bitmask_equals_the_checker_on_the_polygon_runs_polygons(amd, seed):
    from afigan_amd.dual_scale import BitMasks, DualScaleMapper
    outs = {}
    for fmt in ("polygon", "bitmask"):
        np.random.seed(seed)
        outs[fmt] = DualScaleMapper((40, 48, 56), 90, "choice", mask_on=True, mask_format=fmt, device="cuda")(_sample())
    dropped = {}
    for key in ("instances", "instances_x0.5"):
        p, b = outs["polygon"][key], outs["bitmask"][key]
        H, W = p.image_size
        assert b.image_size == (H, W) and isinstance(b.gt_masks, BitMasks)
        masks = [Q.ann_mask(inst, H, W) for inst in p.gt_masks.polygons]
        keep = [bool(m.any()) for m in masks]
        dropped[key] = keep.count(False)
        want = np.stack([m for m, k in zip(masks, keep) if k])
        t = b.gt_masks.tensor
        assert t.is_cuda and t.dtype == torch.bool and tuple(t.shape) == want.shape and len(b.gt_masks) == want.shape[0]
        assert np.array_equal(t.cpu().numpy(), want), key
        sel = torch.tensor(keep)
        assert torch.equal(b.gt_boxes.cpu(), p.gt_boxes.cpu()[sel]) and torch.equal(b.gt_classes.cpu(), p.gt_classes.cpu()[sel])
        assert bool(b.gt_masks.nonempty().all()) and len(b.gt_masks[torch.tensor([True] + [False] * (len(b.gt_masks) - 1))]) == 1
    assert torch.equal(outs["polygon"]["image"], outs["bitmask"]["image"]) and torch.equal(outs["polygon"]["image_x0.5"], outs["bitmask"]["image_x0.5"])
    print(f"[poly] mapper seed {seed}: instances dropped for an empty mask {dropped}")
    assert dropped["instances"] >= 1 and dropped["instances_x0.5"] >= 1
