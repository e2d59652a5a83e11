"""COCO box / mask AP at a validation-set size: a seeded synthetic set of 500 images x 80 categories, about 7 GTs and 100 detections per image
(a detection is a jittered GT of its image or a random box, in the GT's or a random category), masks on 480 x 640 = the ellipse inscribed in the
box, a few hundred runs each.  Median (min / max) of 9 calls after warm-up:

  the three device stages, per task    areas (segm only), IoU, greedy matching, on inputs already uploaded          device events
  evaluate(), per task                 COCOEvaluator.evaluate(): group / sort / upload, the stages, read-back,       host clock, synchronised
                                       accumulate, summarize
  the checker                          tests/coco_eval_f64.py evaluate() on the same input, once, on the CPU         host clock

The checker is interpreted Python loops: its ratio to evaluate() says how slow plain Python is, and nothing about pycocotools (C for the IoU,
numpy for the rest), which is not available here and was not measured.  The statistics of evaluate() and of the checker are compared.

    python tools/coco_eval_bench.py --rounds 9 [--images 500] [--no-checker]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rpn_bench import _time  # noqa: E402
from rle_bench import _host_time  # noqa: E402

H, W, K = 480, 640, 80


def ellipse_counts(box):
    """Uncompressed COCO counts of the ellipse inscribed in `box` (x, y, w, h) on the H x W canvas: one run per column."""
    x, y, w, h = box
    cols = np.arange(max(0, int(np.ceil(x - 0.5))), min(W - 1, int(np.floor(x + w - 0.5))) + 1)
    t = 1.0 - ((cols + 0.5 - (x + w / 2)) / (w / 2)) ** 2
    half = (h / 2) * np.sqrt(np.clip(t, 0.0, None))
    ya = np.clip(np.ceil(y + h / 2 - half - 0.5), 0, H).astype(np.int64)
    yb = np.clip(np.floor(y + h / 2 + half - 0.5) + 1, 0, H).astype(np.int64)
    ok = yb > ya
    starts = np.stack([cols[ok] * H + ya[ok], cols[ok] * H + yb[ok]], 1).reshape(-1)
    keep = np.ones(starts.size, bool)                    # a run that ends at the bottom where the next begins at the top: one run
    same = np.flatnonzero(starts[1:] == starts[:-1])
    keep[same], keep[same + 1] = False, False
    starts = starts[keep]
    return np.diff(np.concatenate(([0], starts, [H * W]))).tolist()


def make_set(n_images, seed=0):
    rng = np.random.default_rng(seed)
    gt = {"images": [{"id": i + 1, "height": H, "width": W} for i in range(n_images)], "categories": [{"id": c + 1, "name": f"c{c + 1}"} for c in range(K)],
          "annotations": []}
    res = []

    def rand_box():
        w, h = rng.uniform(12, 300), rng.uniform(12, 300)
        return [float(rng.uniform(0, W - w)), float(rng.uniform(0, H - h)), float(w), float(h)]

    def seg(box):
        return {"size": [H, W], "counts": ellipse_counts(box)}

    for i in range(n_images):
        boxes = []
        for _ in range(int(rng.integers(3, 12))):
            b, c = rand_box(), int(rng.integers(1, K + 1)) if rng.random() < 0.5 else int(rng.integers(1, 6))
            s = seg(b)
            boxes.append((b, c))
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": i + 1, "category_id": c, "bbox": b, "iscrowd": int(rng.random() < 0.05),
                                      "area": float(sum(s["counts"][1::2])), "segmentation": s})
        for _ in range(100):
            if rng.random() < 0.7:
                b, c = boxes[int(rng.integers(len(boxes)))]
                j = rng.normal(0, 6, 4)
                w, h = max(4.0, b[2] + j[2]), max(4.0, b[3] + j[3])
                b = [float(np.clip(b[0] + j[0], 0, W - w)), float(np.clip(b[1] + j[1], 0, H - h)), float(w), float(h)]
                if rng.random() < 0.2:
                    c = int(rng.integers(1, K + 1))
            else:
                b, c = rand_box(), int(rng.integers(1, K + 1))
            res.append({"image_id": i + 1, "category_id": c, "bbox": b, "score": float(np.round(rng.random(), 3)), "segmentation": seg(b)})
    return gt, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--no-checker", action="store_true")
    args = ap.parse_args()
    import afigan_amd as amd
    gt, res = make_set(args.images)
    runs = [len(r["segmentation"]["counts"]) - 1 for r in res]
    print(f"{args.images} images x {K} categories: {len(gt['annotations'])} GTs, {len(res)} detections, runs per detection mask: mean "
          f"{np.mean(runs):.0f}, max {max(runs)}", flush=True)
    out = {"images": args.images, "rounds": args.rounds, "median_ms": {}, "min_ms": {}, "max_ms": {}}

    def report(name, ts):
        out["median_ms"][name], out["min_ms"][name], out["max_ms"][name] = statistics.median(ts), min(ts), max(ts)
        print(f"{name:34s}: median {statistics.median(ts):10.3f} ms  min {min(ts):10.3f}  max {max(ts):10.3f}  ({len(ts)} rounds)", flush=True)

    stats = {}
    for task in ("bbox", "segm"):
        ev = amd.COCOEvaluator(gt, tasks=(task,))
        p = ev.prepare(res, task)
        ev.stage_area(p)
        ev.stage_iou(p)
        ev.stage_match(p)
        print(f"{task}: {len(p['cat'])} groups, {p['total']} pairs, {int((p['iou'] > 0).sum())} overlapping, {len(p['scores'])} detections kept",
              flush=True)
        if task == "segm":
            report(f"{task} afi_coco_rle_area (both)", _time(lambda: ev.stage_area(p), args.rounds))
        report(f"{task} IoU", _time(lambda: ev.stage_iou(p), args.rounds))
        report(f"{task} afi_coco_match", _time(lambda: ev.stage_match(p), args.rounds))
        ids = [im["id"] for im in gt["images"]]
        by_image = {}
        for r in res:
            by_image.setdefault(r["image_id"], []).append(r)
        ev.process([{"image_id": i} for i in ids], [{"instances": by_image.get(i, [])} for i in ids])
        report(f"{task} evaluate()", _host_time(ev.evaluate, args.rounds))
        stats[task] = ev.stats[task]
        print(f"{task} stats: {np.round(stats[task], 4).tolist()}", flush=True)
    if not args.no_checker:
        import coco_eval_f64 as Q
        for task in ("bbox", "segm"):
            t0 = time.perf_counter()
            e = Q.evaluate(gt, res, task)
            ms = (time.perf_counter() - t0) * 1e3
            err = float(np.abs(e["stats"] - stats[task]).max())
            out["median_ms"][f"{task} checker (one run, CPU)"] = ms
            out[f"{task}_stats_max_abs_diff"] = err
            print(f"{task} checker (interpreted loops, CPU, one run): {ms:10.1f} ms = {ms / out['median_ms'][task + ' evaluate()']:.0f} x evaluate(); "
                  f"stats max abs difference {err:.2e}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
