"""COCO box / mask AP with this package alone: the reference's ``COCOEvaluator`` (afigan/evaluation/coco_evaluation.py) without pycocotools.

``COCOEvaluator(gt, tasks)`` takes an already-loaded COCO annotation dict; ``process(inputs, outputs)`` collects what
``GeneralizedRCNN_AFExtractor.inference()`` returns (either mask format) through ``instances_to_coco_json``; ``evaluate()`` runs pycocotools'
COCOeval restated: the per-(image, category) IoU matrices and the greedy matching on the GPU (csrc/coco_eval.hip: afi_coco_box_iou,
afi_coco_rle_area, afi_coco_rle_iou, afi_coco_match), the precision / recall accumulation and the twelve statistics here in numpy.  There is no
CPU fallback for the device stages.  DESIGN.md section 19 states the semantics; tests/coco_eval_f64.py is the plain-loop checker.

Polygon ground truth for ``segm`` (what every COCO instances file holds) is rasterised on the GPU with ``rasterize_polygons=True``
(ops.polygons_rle, csrc/poly_rle.hip: pycocotools' annToRLE restated), all annotations in one batched call at construction.

Not here: keypoints (OKS), proposal AR, polygon segmentations in the RESULTS (they must be RLE), gathering predictions across processes, result files."""
from collections import OrderedDict

import numpy as np
import torch

from . import ops, rle
from ._lib import AfiError

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, small, medium, large
METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl")


# ------------------------------------------------------------------------------------------------ accumulate and summarize (host)
def accumulate(tables, n_cats, rec_thrs=REC_THRS, max_dets=MAX_DETS):
    """pycocotools' accumulate over the match tables of every (image, category) group, the groups in (image, category) order:
    ``cat`` [ng] (category index), ``dt_off`` / ``gt_off`` [ng + 1], ``scores`` [total_d], ``dt_match`` int [A, T, total_d] (-1: unmatched),
    ``dt_ignore`` [A, T, total_d], ``gt_ignore`` [A, total_g].  Returns (precision [T, R, K, A, M], recall [T, K, A, M]); -1 where a
    (category, area range) has no non-ignored ground truth."""
    cat, dt_off, gt_off = (np.asarray(tables[k]).astype(np.int64) for k in ("cat", "dt_off", "gt_off"))
    scores = np.asarray(tables["scores"], np.float64)
    dtm, dti, gti = np.asarray(tables["dt_match"]), np.asarray(tables["dt_ignore"]), np.asarray(tables["gt_ignore"])
    A, T = dtm.shape[:2]
    R, M = len(rec_thrs), len(max_dets)
    precision = -np.ones((T, R, n_cats, A, M))
    recall = -np.ones((T, n_cats, A, M))
    nd = np.diff(dt_off)
    rank = np.arange(scores.size) - np.repeat(dt_off[:-1], nd)                   # a detection's place in its group's sorted list
    dcat, gcat = np.repeat(cat, nd), np.repeat(cat, np.diff(gt_off))
    for k in range(n_cats):
        if not (cat == k).any():
            continue
        dk, gk = np.flatnonzero(dcat == k), np.flatnonzero(gcat == k)            # image after image
        for mi, md in enumerate(max_dets):
            sel = dk[rank[dk] < md]
            sel = sel[np.argsort(-scores[sel], kind="mergesort")]
            for a in range(A):
                npig = int(np.count_nonzero(gti[a, gk] == 0))
                if npig == 0:
                    continue
                matched, ign = dtm[a][:, sel] >= 0, dti[a][:, sel] != 0
                tp = np.cumsum(matched & ~ign, axis=1).astype(np.float64)
                fp = np.cumsum(~matched & ~ign, axis=1).astype(np.float64)
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                if sel.size == 0:
                    recall[:, k, a, mi] = 0
                    precision[:, :, k, a, mi] = 0
                    continue
                recall[:, k, a, mi] = rc[:, -1]
                pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]         # non-increasing, from the back
                for t in range(T):
                    idx = np.searchsorted(rc[t], rec_thrs, side="left")
                    ok = idx < sel.size
                    q = np.zeros(R)
                    q[ok] = pr[t, idx[ok]]
                    precision[t, :, k, a, mi] = q
    return precision, recall


def summarize(precision, recall):
    """The twelve COCO statistics: AP, AP50, AP75, APs, APm, APl (at the last maxDet), AR@1, AR@10, AR@100, ARs, ARm, ARl; -1 where nothing counts."""
    M = precision.shape[4]

    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    ap = lambda a, ts=slice(None): mean(precision[ts, :, :, a, M - 1])          # noqa: E731
    ar = lambda a, m: mean(recall[:, :, a, m])                                   # noqa: E731
    return np.array([ap(0), ap(0, slice(0, 1)), ap(0, slice(5, 6)), ap(1), ap(2), ap(3), ar(0, 0), ar(0, 1), ar(0, M - 1), ar(1, M - 1), ar(2, M - 1),
                     ar(3, M - 1)])


# ------------------------------------------------------------------------------------------------ the evaluator
def _starts(seg, what):
    """(ascending run starts int32, H W) of an RLE segmentation: a compressed string, or an uncompressed counts list, with ``size``."""
    if not isinstance(seg, dict) or "counts" not in seg or "size" not in seg:
        raise AfiError(f"COCOEvaluator: {what}: the `segm` task needs an RLE segmentation ({{'size': [H, W], 'counts': str or list}}); a polygon "
                       "is not rasterised here -- pass rasterize_polygons=True to COCOEvaluator for polygon ground truth, or convert it to RLE "
                       "first (afigan_amd.polygons_to_rle)")
    c = seg["counts"]
    c = rle.from_string(c) if isinstance(c, (str, bytes)) else np.asarray(c, dtype=np.int64).reshape(-1)
    n = int(seg["size"][0]) * int(seg["size"][1])
    if n >= 1 << 31 or (c < 0).any() or int(c.sum()) != n:
        raise AfiError(f"COCOEvaluator: {what}: RLE counts summing to {int(c.sum())} for a mask of size {list(seg['size'])} (H W < 2^31)")
    return np.cumsum(c)[:-1].astype(np.int32), n


class COCOEvaluator:
    """``gt``: a COCO annotation dict (``images``, ``annotations``, ``categories``).  ``tasks``: of "bbox", "segm".  ``class_names``: with more than
    one entry (one per category, in category-id order), ``evaluate()`` adds ``AP-<name>`` per category.  After ``evaluate()``, ``self.stats[task]``
    [12], ``self.precision[task]`` [T, R, K, A, M] and ``self.recall[task]`` [T, K, A, M] hold what pycocotools' ``COCOeval.stats`` / ``.eval`` hold.
    ``rasterize_polygons``: for ``segm``, a ground truth whose ``segmentation`` is a polygon list is rasterised on the GPU at the ``height`` /
    ``width`` of its image entry (pycocotools' annToRLE), all of them in one batched call here; RLE ground truth (crowds) is taken as it is.
    False (the default) refuses a polygon."""

    def __init__(self, gt, tasks=("bbox",), class_names=None, rasterize_polygons=False):
        for k in ("images", "annotations", "categories"):
            if k not in gt:
                raise AfiError(f"COCOEvaluator: the annotation dict has no `{k}`")
        tasks = tuple(tasks)
        if not tasks or any(t not in ("bbox", "segm") for t in tasks):
            raise AfiError(f"COCOEvaluator: tasks of ('bbox', 'segm') expected, got {tasks} (keypoints and proposals are out of scope)")
        self._tasks = tasks
        self._img_ids = sorted(im["id"] for im in gt["images"])
        self._cat_ids = sorted(c["id"] for c in gt["categories"])
        self._img_index = {v: i for i, v in enumerate(self._img_ids)}
        self._cat_index = {v: i for i, v in enumerate(self._cat_ids)}
        if class_names is not None and len(class_names) > 1 and len(class_names) != len(self._cat_ids):
            raise AfiError(f"COCOEvaluator: {len(class_names)} class names for {len(self._cat_ids)} categories")
        self._class_names = class_names
        anns = [a for a in gt["annotations"] if a["image_id"] in self._img_index and a["category_id"] in self._cat_index]
        K = len(self._cat_ids)
        key = np.array([self._img_index[a["image_id"]] * K + self._cat_index[a["category_id"]] for a in anns], np.int64)
        order = np.argsort(key, kind="mergesort")                               # annotation order inside a group
        self._gt = [anns[i] for i in order]
        self._gt_key = key[order]
        # segm: the ground truth's run starts, once (a polygon is refused by _starts unless rasterize_polygons)
        self._gt_starts = None
        if "segm" in tasks:
            is_poly = [rasterize_polygons and isinstance(a.get("segmentation"), (list, tuple)) for a in self._gt]
            self._gt_starts = [None if p else _starts(a.get("segmentation"), f"annotation {a.get('id')}") for a, p in zip(self._gt, is_poly)]
            if any(is_poly):
                self._rasterize([i for i, p in enumerate(is_poly) if p], {im["id"]: im for im in gt["images"]})
        self.reset()

    def _rasterize(self, idx, images):
        """The run starts of the polygon ground truths ``idx`` of self._gt: one batched ops.polygons_rle call and one read back."""
        polys, sizes = [], []
        for i in idx:
            a = self._gt[i]
            im = images[a["image_id"]]
            if "height" not in im or "width" not in im:
                raise AfiError(f"COCOEvaluator: annotation {a.get('id')}: image {a['image_id']!r} has no `height` / `width`, which a polygon is rasterised at")
            polys.append(a["segmentation"])
            sizes.append((int(im["height"]), int(im["width"])))
        sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
        ops.polygons_batch(polys, sizes)                                        # every refusal before the device is touched
        starts, off, hw = ops.polygons_rle(polys, sizes)
        starts, off, hw = starts.cpu().numpy(), off.cpu().numpy(), hw.cpu().numpy()
        for k, i in enumerate(idx):
            self._gt_starts[i] = (starts[off[k]:off[k + 1]].astype(np.int32), int(hw[k]))

    def reset(self):
        self._predictions = []
        self.stats, self.precision, self.recall = {}, {}, {}

    def process(self, inputs, outputs):
        """``inputs``: dicts with ``image_id``; ``outputs``: dicts with ``instances`` = what ``inference()`` returns for the image (pasted bool masks or
        ``pred_masks_rle``), or a ready-made list of COCO result dicts."""
        from .roi_heads import instances_to_coco_json
        for inp, out in zip(inputs, outputs):
            img = inp["image_id"]
            if img not in self._img_index:
                raise AfiError(f"COCOEvaluator: image id {img!r} is not in the annotations")
            pred = {"image_id": img}
            if isinstance(out, dict) and "instances" in out:
                inst = out["instances"]
                pred["instances"] = list(inst) if isinstance(inst, (list, tuple)) else instances_to_coco_json(inst, img)
            elif isinstance(out, (list, tuple)):
                pred["instances"] = list(out)
            self._predictions.append(pred)

    def evaluate(self):
        if len(self._predictions) == 0:
            return {}
        results = OrderedDict()
        if "instances" not in self._predictions[0]:
            return results
        coco = [r for p in self._predictions for r in p.get("instances", ())]
        for task in sorted(self._tasks):
            if len(coco) == 0:                                                  # the reference: "No predictions from the model!"
                results[task] = OrderedDict((m, float("nan")) for m in METRICS)
                continue
            tables = self.match_tables(coco, task)
            self.precision[task], self.recall[task] = accumulate(tables, len(self._cat_ids))
            self.stats[task] = summarize(self.precision[task], self.recall[task])
            results[task] = self._derive(task)
        return results

    def _derive(self, task):
        s = self.stats[task]
        res = OrderedDict((m, float(s[i] * 100 if s[i] >= 0 else "nan")) for i, m in enumerate(METRICS))
        if self._class_names is None or len(self._class_names) <= 1:
            return res
        for k, name in enumerate(self._class_names):
            p = self.precision[task][:, :, k, 0, -1]
            p = p[p > -1]
            res["AP-" + str(name)] = float(np.mean(p) * 100) if p.size else float("nan")
        return res

    # -------------------------------------------------------------------------------------------- the device part
    def match_tables(self, coco_results, task):
        """The (image, category) groups of `coco_results` and the ground truth, their IoU matrices and greedy matches (on the GPU), as the tables
        ``accumulate`` reads (numpy, plus ``iou`` and ``iou_off``: the packed matrices, and ``dt_area``)."""
        p = self.prepare(coco_results, task)
        self.stage_area(p)
        self.stage_iou(p)
        self.stage_match(p)
        dtm, dti, gti = p["match"]
        return {"cat": p["cat"], "img": p["img"], "dt_off": p["dt_off"], "gt_off": p["gt_off"], "iou_off": p["iou_off"], "scores": p["scores"],
                "dt_match": dtm.cpu().numpy(), "dt_ignore": dti.cpu().numpy(), "gt_ignore": gti.cpu().numpy(), "iou": p["iou"].cpu().numpy(),
                "dt_area": p["dt_area"].cpu().numpy()}

    def prepare(self, coco_results, task):
        """The host part before the kernels: group, sort and cut the results, and upload boxes or run starts once.  Returns the dict the three
        stages below work on (tools/coco_eval_bench.py times them one by one)."""
        K, dev, cut = len(self._cat_ids), "cuda", MAX_DETS[-1]
        for r in coco_results:
            if r["image_id"] not in self._img_index:
                raise AfiError(f"COCOEvaluator: a result with image id {r['image_id']!r}, which is not in the annotations")
        res = [r for r in coco_results if r["category_id"] in self._cat_index]  # other categories are never evaluated, as in pycocotools
        key = np.array([self._img_index[r["image_id"]] * K + self._cat_index[r["category_id"]] for r in res], np.int64)
        score = np.array([r["score"] for r in res], np.float64)
        order = np.lexsort((np.arange(key.size), -score, key))                  # by group, inside it by descending score, ties in input order
        key_s = key[order]
        first = np.searchsorted(key_s, key_s, side="left")
        order = order[np.arange(key_s.size) - first < cut]                      # the top 100 of every group
        dts, dkey = [res[i] for i in order], key[order]
        gts, gkey = self._gt, self._gt_key
        groups = np.union1d(dkey, gkey)                                         # a group with neither is not there
        dt_off = np.searchsorted(dkey, np.append(groups, np.iinfo(np.int64).max), side="left").astype(np.int64)
        gt_off = np.searchsorted(gkey, np.append(groups, np.iinfo(np.int64).max), side="left").astype(np.int64)
        iou_off = np.concatenate(([0], np.cumsum(np.diff(dt_off) * np.diff(gt_off)))).astype(np.int64)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
        p = {"task": task, "cat": groups % K, "img": groups // K, "dt_off": dt_off, "gt_off": gt_off, "iou_off": iou_off, "scores": score[order],
             "total": int(iou_off[-1]), "max_g": int(np.diff(gt_off).max()) if groups.size else 0, "offs": (up(dt_off, np.int64), up(gt_off, np.int64), up(iou_off, np.int64)),
             "crowd": up([1 if a.get("iscrowd", 0) else 0 for a in gts], np.uint8), "gt_area": up([a["area"] for a in gts], np.float64),
             "area_rng": up(AREA_RNG, np.float64), "iou_thr": up(IOU_THRS, np.float64)}
        if task == "bbox":
            dbox = np.array([r["bbox"] for r in dts], np.float64).reshape(-1, 4)
            p["dt_box"], p["gt_box"] = up(dbox, np.float64), up(np.array([a["bbox"] for a in gts], np.float64).reshape(-1, 4), np.float64)
            p["dt_area"] = up(dbox[:, 2] * dbox[:, 3], np.float64)
        else:
            if self._gt_starts is None:
                raise AfiError("COCOEvaluator: the `segm` task was not among this evaluator's tasks")
            # (a result's `bbox` is not consulted for segm)
            for side, sn in (("dt_rle", [_starts(r.get("segmentation"), "a result") for r in dts]), ("gt_rle", self._gt_starts)):
                starts = np.concatenate([s for s, _ in sn]) if sn else np.zeros(0, np.int32)
                soff = np.concatenate(([0], np.cumsum([s.size for s, _ in sn]))).astype(np.int64)
                p[side] = (up(starts, np.int32), up(soff, np.int64), up([n for _, n in sn], np.int32))
        return p

    def stage_area(self, p):
        """segm: the mask areas (afi_coco_rle_area); the detection's area for the area ranges is its mask's."""
        if p["task"] == "segm":
            p["rle_area"] = (ops.coco_rle_area(*p["dt_rle"]), ops.coco_rle_area(*p["gt_rle"]))
            p["dt_area"] = p["rle_area"][0].to(torch.float64)

    def stage_iou(self, p):
        if p["task"] == "bbox":
            p["iou"] = ops.coco_box_iou(p["dt_box"], p["gt_box"], p["crowd"], *p["offs"], p["total"])
        else:
            p["iou"] = ops.coco_rle_iou(p["dt_rle"] + (p["rle_area"][0],), p["gt_rle"] + (p["rle_area"][1],), p["crowd"], *p["offs"], p["total"])

    def stage_match(self, p):
        p["match"] = ops.coco_match(p["iou"], *p["offs"], p["dt_area"], p["gt_area"], p["crowd"], p["area_rng"], p["iou_thr"], max_g=p["max_g"])
