"""Inputs of the COCO evaluation tests (tests/test_coco_eval_host.py, tests/test_gpu_coco_eval.py): the hand cases A to H whose answers are known
without running anything, and a seeded synthetic set of 6 images x 3 categories that holds every shape the kernels can get wrong.  Annotations and
results carry both a ``bbox`` and an uncompressed-RLE ``segmentation``, so one set serves both tasks.  Nothing here imports the package."""
import numpy as np

CANVAS = (300, 300)                                      # of the hand cases


def counts_of(mask):
    """COCO's uncompressed counts (a list of ints) of a [H, W] mask, column-major."""
    f = (np.asarray(mask) != 0).T.reshape(-1)
    starts = np.flatnonzero(f != np.concatenate(([False], f[:-1])))
    return np.diff(np.concatenate(([0], starts, [f.size]))).astype(np.int64).tolist()


def rect_mask(box, hw):
    x, y, w, h = (int(v) for v in box)
    m = np.zeros(hw, bool)
    m[y:y + h, x:x + w] = True
    return m


def _seg(mask):
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": counts_of(mask)}


def dataset(n_images, cats, gts, dts, hw=CANVAS):
    """gts: (image, category, box, iscrowd[, area]); dts: (image, category, box, score).  Integer boxes; the masks are the filled boxes."""
    gt = {"images": [{"id": i, "height": hw[0], "width": hw[1]} for i in range(1, n_images + 1)],
          "categories": [{"id": c, "name": f"c{c}"} for c in cats], "annotations": []}
    for n, g in enumerate(gts):
        img, cat, box, crowd = g[:4]
        gt["annotations"].append({"id": n + 1, "image_id": img, "category_id": cat, "bbox": [float(v) for v in box], "iscrowd": int(crowd),
                                  "area": float(g[4]) if len(g) > 4 else float(box[2] * box[3]), "segmentation": _seg(rect_mask(box, hw))})
    res = [{"image_id": img, "category_id": cat, "bbox": [float(v) for v in box], "score": float(s), "segmentation": _seg(rect_mask(box, hw))}
           for img, cat, box, s in dts]
    return gt, res


def hand_case(name):
    """(gt, results) of the issue's cases; the expected statistics are in tests/test_coco_eval_host.py."""
    G = (10, 10, 50, 50)
    if name == "A":
        return dataset(1, [1], [(1, 1, G, 0)], [(1, 1, G, .9)])
    if name == "B":
        return dataset(1, [1], [(1, 1, G, 0)], [(1, 1, (200, 200, 50, 50), .9), (1, 1, G, .8)])
    if name == "C":
        return dataset(1, [1], [(1, 1, (0, 0, 100, 100), 0)], [(1, 1, (0, 0, 100, 77), .9)])
    if name == "D":
        return dataset(1, [1], [(1, 1, (0, 0, 50, 50), 0), (1, 1, (100, 100, 100, 100), 1)],
                       [(1, 1, (110, 110, 20, 20), .9), (1, 1, (0, 0, 50, 50), .8)])
    if name == "D-crowd-only":
        return dataset(1, [1], [(1, 1, (100, 100, 100, 100), 1)], [(1, 1, (110, 110, 20, 20), .9), (1, 1, (0, 0, 50, 50), .8)])
    if name == "E":                                      # 100 detections elsewhere score above the only overlapping one
        far = [(1, 1, (100 + (i % 10) * 12, 100 + (i // 10) * 12, 10, 10), .99 - .001 * i) for i in range(100)]
        return dataset(1, [1], [(1, 1, G, 0)], far + [(1, 1, G, .01)])
    if name == "F":                                      # area exactly 32^2: inside small and inside medium
        return dataset(1, [1], [(1, 1, (5, 5, 32, 32), 0)], [(1, 1, (5, 5, 32, 32), .9)])
    if name == "G":                                      # two GTs, IoU 0.5 each with the one detection
        return dataset(1, [1], [(1, 1, (0, 0, 10, 5), 0), (1, 1, (0, 5, 10, 5), 0)], [(1, 1, (0, 0, 10, 10), .9)])
    if name == "H":                                      # IoU exactly 0.5
        return dataset(1, [1], [(1, 1, (0, 0, 1, 1), 0)], [(1, 1, (0, 0, 2, 1), .9)])
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ the synthetic set
SET_SIZES = ((130, 90), (65, 40), (130, 88), (64, 50), (129, 77), (96, 64))    # (H, W): rows 63 | 64 | 65 are crossed
SET_IMAGE_IDS = (11, 14, 17, 20, 23, 26)
SET_CAT_IDS = (2, 5, 9)
SET_SEED = 5


def _mask(rng, box, hw, style):
    """A mask inside `box`: the filled box or the inscribed ellipse, with a tenth of its pixels cleared."""
    H, W = hw
    x, y, w, h = box
    ys, xs = np.mgrid[0:H, 0:W]
    cx, cy = xs + 0.5, ys + 0.5
    inside = (cx >= x) & (cx <= x + w) & (cy >= y) & (cy <= y + h)
    if style == "ellipse":
        inside &= ((cx - (x + w / 2)) / (w / 2)) ** 2 + ((cy - (y + h / 2)) / (h / 2)) ** 2 <= 1.0
    if style != "solid":
        inside &= rng.random((H, W)) < 0.9
    return inside


def _rand_box(rng, hw, lo, hi):
    H, W = hw
    w = min(float(rng.integers(lo * 4, hi * 4 + 1)) / 4, W - 1.0)
    h = min(float(rng.integers(lo * 4, hi * 4 + 1)) / 4, H - 1.0)
    x = float(rng.integers(0, int((W - w) * 4) + 1)) / 4
    y = float(rng.integers(0, int((H - h) * 4) + 1)) / 4
    return (x, y, w, h)


def _jitter(rng, box, hw, amount):
    H, W = hw
    x, y, w, h = box
    d = rng.integers(-amount * 4, amount * 4 + 1, 4) / 4.0
    w2, h2 = max(1.0, w + d[2]), max(1.0, h + d[3])
    x2, y2 = min(max(0.0, x + d[0]), W - w2), min(max(0.0, y + d[1]), H - h2)
    return (float(max(x2, 0.0)), float(max(y2, 0.0)), float(min(w2, W)), float(min(h2, H)))


def synthetic_set(seed=SET_SEED):
    """(gt, results).  By construction (tests/test_coco_eval_host.py checks each on the checker): image 0 holds a group of 130 detections, a group
    of 70 GTs and a group of GTs without detections; image 1 a group of detections without GTs, an empty group and a crowd GT with several
    detections inside; image 2 boxes above 96^2 and a second such crowd; image 5 the hand cases G and H; scores come from a grid of 0.05, so
    they tie."""
    rng = np.random.default_rng(seed)
    gt = {"images": [{"id": i, "height": h, "width": w} for i, (h, w) in zip(SET_IMAGE_IDS, SET_SIZES)],
          "categories": [{"id": c, "name": f"c{c}"} for c in SET_CAT_IDS], "annotations": []}
    res = []

    def add_gt(i, k, box, crowd=0, style=None):
        m = _mask(rng, box, SET_SIZES[i], style or ("ellipse", "rect")[int(rng.integers(2))])
        gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": SET_IMAGE_IDS[i], "category_id": SET_CAT_IDS[k],
                                  "bbox": list(box), "iscrowd": crowd, "area": float(m.sum()), "segmentation": _seg(m)})

    def add_dt(i, k, box, score=None, style=None):
        m = _mask(rng, box, SET_SIZES[i], style or ("ellipse", "rect")[int(rng.integers(2))])
        res.append({"image_id": SET_IMAGE_IDS[i], "category_id": SET_CAT_IDS[k], "bbox": list(box),
                    "score": float(rng.integers(1, 20)) / 20 if score is None else score, "segmentation": _seg(m)})

    def group(i, k, n_gt, n_dt, lo, hi, crowds=()):
        hw = SET_SIZES[i]
        boxes = [_rand_box(rng, hw, lo, hi) for _ in range(n_gt)]
        for n, b in enumerate(boxes):
            add_gt(i, k, b, int(n in crowds))
        for _ in range(n_dt):
            if boxes and rng.random() < 0.7:
                add_dt(i, k, _jitter(rng, boxes[int(rng.integers(len(boxes)))], hw, 3))
            else:
                add_dt(i, k, _rand_box(rng, hw, lo, hi))

    group(0, 0, 3, 130, 20, 60)                          # 130 detections: cut to 100
    group(0, 1, 70, 5, 5, 12)                            # 70 GTs: more than a wave
    group(0, 2, 2, 0, 10, 40)                            # GTs only
    group(1, 0, 0, 4, 8, 30)                             # detections only; (1, 1) stays empty
    add_gt(1, 2, (4.0, 6.0, 30.0, 50.0), 1, "rect")      # a crowd with five detections inside, and one ordinary GT
    add_gt(1, 2, (20.0, 2.0, 15.0, 20.0), 0)
    for n in range(5):
        add_dt(1, 2, (6.0 + 4 * n, 10.0 + 7 * n, 8.0, 10.0), 0.9 - 0.1 * (n // 2))
    add_dt(1, 2, (20.0, 2.0, 15.0, 20.0), 0.9)
    add_gt(2, 0, (1.0, 2.0, 85.0, 120.0), 0, "solid")    # above 96^2 as a box and as a mask
    add_gt(2, 0, (10.0, 10.0, 40.0, 50.0), 0)            # medium
    add_gt(2, 0, (50.0, 80.0, 20.0, 20.0), 0)            # small
    add_dt(2, 0, (2.0, 3.0, 84.0, 119.0), 0.8, "rect")
    add_dt(2, 0, (0.0, 0.0, 88.0, 130.0), 0.8, "solid")
    add_dt(2, 0, (11.0, 9.0, 40.0, 52.0), 0.7)
    add_dt(2, 0, (50.0, 80.0, 20.0, 21.0), 0.7)
    add_dt(2, 0, (60.0, 5.0, 8.0, 8.0), 0.95)
    add_gt(2, 1, (30.0, 40.0, 50.0, 70.0), 1, "rect")    # the second crowd: four detections inside, two GTs beside it
    add_gt(2, 1, (2.0, 2.0, 25.0, 30.0), 0)
    add_gt(2, 1, (5.0, 90.0, 20.0, 30.0), 0)
    for n in range(4):
        add_dt(2, 1, (32.0 + 10 * n, 45.0 + 12 * n, 12.0, 14.0), 0.6)
    add_dt(2, 1, (3.0, 2.0, 24.0, 30.0), 0.6)
    add_dt(2, 1, (60.0, 2.0, 20.0, 20.0), 0.3)
    group(2, 2, 4, 12, 10, 50)
    for k in range(3):
        group(3, k, 3, 9, 6, 40, crowds=(1,) if k == 1 else ())
        group(4, k, 5, 14, 8, 70)
    for b in ((0.0, 0.0, 10.0, 5.0), (0.0, 5.0, 10.0, 5.0)):              # G: equal IoU with one detection
        add_gt(5, 0, b, 0, "solid")
    add_dt(5, 0, (0.0, 0.0, 10.0, 10.0), 0.9, "solid")
    add_gt(5, 1, (0.0, 0.0, 1.0, 1.0), 0, "solid")                          # H: IoU exactly 0.5
    add_dt(5, 1, (0.0, 0.0, 2.0, 1.0), 0.9, "solid")
    group(5, 2, 6, 20, 5, 45)
    return gt, res


_CHECKED = {}


def checked_set(task):
    """(gt, results, the checker's evaluation) of the synthetic set, computed once per session and task; treat as read-only."""
    if task not in _CHECKED:
        import coco_eval_f64 as Q
        gt, res = synthetic_set()
        _CHECKED[task] = (gt, res, Q.evaluate(gt, res, task))
    return _CHECKED[task]
