"""COCO box / mask AP restated in plain Python loops and fp64: the checker of csrc/coco_eval.hip and afigan_amd/coco_eval.py (the role roi_f64.py
and mask_f64.py play for their kernels).  It is pycocotools' COCOeval (computeIoU, evaluateImg, accumulate, summarize) for iouType bbox and segm,
written from the algorithm: pycocotools is not available where this runs, so its fidelity rests on the known answers asserted in
tests/test_coco_eval_host.py.  Nothing here imports the package under test.

Masks are ascending run *starts* on n = H W pixels read column-major (afigan_amd/rle.py): pixels from an even-indexed start up to the next start
(or n) are set.  A result's / annotation's ``segmentation`` is ``{"size": [H, W], "counts": [ints]}`` (uncompressed) here."""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, small, medium, large
EPS = float(np.spacing(1))


# ------------------------------------------------------------------------------------------------ IoU
def box_iou(dt, gt, crowd):
    """[D, G] fp64 from xywh boxes, operation by operation as afi_coco_box_iou."""
    out = np.zeros((len(dt), len(gt)), np.float64)
    for d, (dx, dy, dw, dh) in enumerate(dt):
        dx, dy, dw, dh = float(dx), float(dy), float(dw), float(dh)
        for g, (gx, gy, gw, gh) in enumerate(gt):
            gx, gy, gw, gh = float(gx), float(gy), float(gw), float(gh)
            w = min(dx + dw, gx + gw) - max(dx, gx)
            h = min(dy + dh, gy + gh) - max(dy, gy)
            if w <= 0 or h <= 0:
                continue
            i = w * h
            u = dw * dh if crowd[g] else dw * dh + gw * gh - i
            out[d, g] = i / u
    return out


def starts_of_counts(counts):
    s, acc = [], 0
    for c in list(counts)[:-1]:
        acc += int(c)
        s.append(acc)
    return s


def starts_of_mask(mask):
    """The starts of a [H, W] mask, pixel by pixel."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    s, prev = [], False
    for x in range(W):
        for y in range(H):
            if bool(m[y, x]) != prev:
                s.append(x * H + y)
                prev = not prev
    return s


def rle_area(starts, n):
    a = 0
    for i in range(0, len(starts), 2):
        a += (starts[i + 1] if i + 1 < len(starts) else n) - starts[i]
    return a


def rle_inter(a, b, n):
    """Pixels set in both: the plain two-pointer merge over the whole of both lists (no short cuts)."""
    ia = ib = pos = inter = 0
    va = vb = False
    while ia < len(a) or ib < len(b):
        pa = a[ia] if ia < len(a) else n
        pb = b[ib] if ib < len(b) else n
        p = min(pa, pb)
        if va and vb:
            inter += p - pos
        pos = p
        if pa <= pb:
            va, ia = not va, ia + 1
        else:
            vb, ib = not vb, ib + 1
    if va and vb:
        inter += n - pos
    return inter


def rle_iou(dt, gt, crowd):
    """dt, gt: lists of (starts, n).  (inter int64 [D, G], iou fp64 [D, G]); a pair of different n gives -1 in both."""
    inter = np.zeros((len(dt), len(gt)), np.int64)
    iou = np.zeros((len(dt), len(gt)), np.float64)
    da, ga = [rle_area(a, n) for a, n in dt], [rle_area(b, n) for b, n in gt]
    for d, (a, na) in enumerate(dt):
        for g, (b, nb) in enumerate(gt):
            if na != nb:
                inter[d, g], iou[d, g] = -1, -1.0
                continue
            i = rle_inter(a, b, na)
            u = da[d] if crowd[g] else da[d] + ga[g] - i
            inter[d, g] = i
            iou[d, g] = 0.0 if u == 0 else float(i) / float(u)
    return inter, iou


# ------------------------------------------------------------------------------------------------ greedy matching
def match(iou, dt_area, gt_area, crowd, area_rng=AREA_RNG, thrs=IOU_THRS):
    """(dt_match int32 [A, T, D] (GT index or -1), dt_ignore uint8 [A, T, D], gt_ignore uint8 [A, G])."""
    D, G, A, T = len(dt_area), len(gt_area), len(area_rng), len(thrs)
    dtm = np.full((A, T, D), -1, np.int32)
    dti = np.zeros((A, T, D), np.uint8)
    gti = np.zeros((A, G), np.uint8)
    for a, (lo, hi) in enumerate(area_rng):
        for g in range(G):
            gti[a, g] = 1 if (crowd[g] or gt_area[g] < lo or gt_area[g] > hi) else 0
        order = [g for g in range(G) if not gti[a, g]] + [g for g in range(G) if gti[a, g]]      # the stable sort by the ignore flag
        for t, thr in enumerate(thrs):
            matched = [False] * G
            for d in range(D):
                best, m = min(float(thr), 1 - 1e-10), -1
                for g in order:
                    if matched[g] and not crowd[g]:
                        continue
                    if m > -1 and not gti[a, m] and gti[a, g]:
                        break
                    if iou[d, g] < best:
                        continue
                    best, m = iou[d, g], g
                if m >= 0:
                    dtm[a, t, d], dti[a, t, d], matched[m] = m, gti[a, m], True
                elif dt_area[d] < lo or dt_area[d] > hi:
                    dti[a, t, d] = 1
    return dtm, dti, gti


# ------------------------------------------------------------------------------------------------ groups
def groups_of(gt, results, task, max_det=MAX_DETS[-1]):
    """The (image, category) groups in (image id, category id) order, groups with neither detections nor GTs left out.  Each is a dict: img, k
    (category index), dts (sorted by descending score, stably, cut to max_det), gts (annotation order), scores, dt_area, gt_area, crowd, iou,
    inter (segm), dt_match, dt_ignore, gt_ignore."""
    img_ids = sorted(im["id"] for im in gt["images"])
    cat_ids = sorted(c["id"] for c in gt["categories"])
    out, gt_of, dt_of = [], {}, {}
    for a in gt["annotations"]:
        gt_of.setdefault((a["image_id"], a["category_id"]), []).append(a)
    for r in results:
        dt_of.setdefault((r["image_id"], r["category_id"]), []).append(r)
    for img in img_ids:
        for k, cat in enumerate(cat_ids):
            gts, dts = gt_of.get((img, cat), []), dt_of.get((img, cat), [])
            if not gts and not dts:
                continue
            dts = sorted(dts, key=lambda r: -r["score"])[:max_det]               # sorted() is stable
            crowd = [1 if a.get("iscrowd", 0) else 0 for a in gts]
            g = {"img": img, "k": k, "dts": dts, "gts": gts, "scores": [float(r["score"]) for r in dts], "crowd": crowd,
                 "gt_area": [float(a["area"]) for a in gts], "inter": None}
            if task == "bbox":
                g["dt_area"] = [float(r["bbox"][2]) * float(r["bbox"][3]) for r in dts]
                g["iou"] = box_iou([r["bbox"] for r in dts], [a["bbox"] for a in gts], crowd)
            else:
                dm = [(starts_of_counts(r["segmentation"]["counts"]), int(r["segmentation"]["size"][0]) * int(r["segmentation"]["size"][1])) for r in dts]
                gm = [(starts_of_counts(a["segmentation"]["counts"]), int(a["segmentation"]["size"][0]) * int(a["segmentation"]["size"][1])) for a in gts]
                g["dt_area"] = [float(rle_area(s, n)) for s, n in dm]
                g["inter"], g["iou"] = rle_iou(dm, gm, crowd)
            g["dt_match"], g["dt_ignore"], g["gt_ignore"] = match(g["iou"], g["dt_area"], g["gt_area"], crowd)
            out.append(g)
    return out


def tables_of(groups):
    """The groups' match tables as the flat arrays afigan_amd.coco_eval.accumulate reads."""
    A, T = len(AREA_RNG), len(IOU_THRS)
    dt_off = np.cumsum([0] + [len(g["dts"]) for g in groups]).astype(np.int64)
    gt_off = np.cumsum([0] + [len(g["gts"]) for g in groups]).astype(np.int64)
    cat = lambda key, shape, dtype, axis: (np.concatenate([np.asarray(g[key], dtype).reshape(shape) for g in groups], axis)  # noqa: E731
                                           if groups else np.zeros([0 if s == -1 else s for s in shape], dtype))
    return {"cat": np.array([g["k"] for g in groups], np.int64), "dt_off": dt_off, "gt_off": gt_off, "scores": cat("scores", (-1,), np.float64, 0),
            "dt_match": cat("dt_match", (A, T, -1), np.int32, 2), "dt_ignore": cat("dt_ignore", (A, T, -1), np.uint8, 2),
            "gt_ignore": cat("gt_ignore", (A, -1), np.uint8, 1)}


# ------------------------------------------------------------------------------------------------ accumulate and summarize
def accumulate(groups, n_cats):
    """(precision [T, R, K, A, M], recall [T, K, A, M]), -1 where a (category, area range) has no non-ignored GT."""
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, n_cats, A, M))
    recall = -np.ones((T, n_cats, A, M))
    for k in range(n_cats):
        E = [g for g in groups if g["k"] == k]
        if not E:
            continue
        for a in range(A):
            npig = sum(1 for g in E for v in g["gt_ignore"][a] if not v)
            if npig == 0:
                continue
            for mi, md in enumerate(MAX_DETS):
                rows = [(-g["scores"][d], gi, d) for gi, g in enumerate(E) for d in range(min(md, len(g["scores"])))]
                rows.sort(key=lambda r: r[0])                                      # stable: ties keep (image, rank) order
                for t in range(T):
                    tp = fp = 0
                    rc, pr = [], []
                    for _, gi, d in rows:
                        g = E[gi]
                        if not g["dt_ignore"][a, t, d]:
                            if g["dt_match"][a, t, d] >= 0:
                                tp += 1
                            else:
                                fp += 1
                        rc.append(float(tp) / npig)
                        pr.append(float(tp) / (float(fp) + float(tp) + EPS))
                    recall[t, k, a, mi] = rc[-1] if rc else 0.0
                    for i in range(len(pr) - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    i = 0
                    for r, thr in enumerate(REC_THRS):                             # searchsorted(rc, thr, "left"): the first i with rc[i] >= thr
                        while i < len(rc) and rc[i] < thr:
                            i += 1
                        precision[t, r, k, a, mi] = pr[i] if i < len(pr) else 0.0
    return precision, recall


def _mean(values):
    # np.mean, not a running sum: the evaluator (like pycocotools) takes np.mean of the same entries in the same order, and the comparison of the
    # two is exact only if both sum pairwise
    return float(np.mean(np.array(values, np.float64))) if values else -1.0


def summarize(precision, recall):
    """The twelve COCO statistics."""
    T, R, K, A, M = precision.shape

    def ap(a, ts):
        return _mean([precision[t, r, k, a, M - 1] for t in ts for r in range(R) for k in range(K) if precision[t, r, k, a, M - 1] > -1])

    def ar(a, m):
        return _mean([recall[t, k, a, m] for t in range(T) for k in range(K) if recall[t, k, a, m] > -1])

    every = range(T)
    return np.array([ap(0, every), ap(0, [0]), ap(0, [5]), ap(1, every), ap(2, every), ap(3, every),
                     ar(0, 0), ar(0, 1), ar(0, 2), ar(1, 2), ar(2, 2), ar(3, 2)])


def evaluate(gt, results, task="bbox"):
    groups = groups_of(gt, results, task)
    K = len(gt["categories"])
    precision, recall = accumulate(groups, K)
    return {"groups": groups, "precision": precision, "recall": recall, "stats": summarize(precision, recall)}
