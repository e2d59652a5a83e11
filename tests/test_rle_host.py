"""CPU-side checks of the COCO RLE path: afigan_amd/rle.py against the format's known answers and against scalar restatements written here,
instances_to_coco_json on CPU detections, the new entry points' argument checks, and the seeded inputs of tests/test_gpu_rle.py held -- on the
fp64 checker tests/mask_f64.py alone -- to the run shapes that file's equality tests rely on."""
import types

import numpy as np
import pytest
import torch

import afigan_amd as amd
from afigan_amd import rle

import mask_f64 as Q
import test_gpu_rle as G


# ------------------------------------------------------------------------------------------------ scalar restatements
def _encode_scalar(mask):
    H, W = mask.shape
    counts, prev, run = [], 0, 0
    for x in range(W):
        for y in range(H):
            v = int(bool(mask[y, x]))
            if v != prev:
                counts.append(run)
                run, prev = 0, v
            run += 1
    counts.append(run)
    return counts


def _to_string_scalar(counts):
    out = []
    for i, c in enumerate(counts):
        x = int(c) - (int(counts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            g = x & 31
            x >>= 5
            more = (x != -1) if g & 16 else (x != 0)
            if more:
                g |= 32
            out.append(chr(g + 48))
    return "".join(out)


def _from_string_scalar(s):
    counts, i = [], 0
    while i < len(s):
        x, k, more = 0, 0, True
        while more:
            g = ord(s[i]) - 48
            x |= (g & 31) << (5 * k)
            more = bool(g & 32)
            i += 1
            k += 1
            if not more and g & 16:
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def _known_mask():
    m = np.zeros((40, 30), bool)
    m[3:37, 2:5] = True
    m[39, 7] = True
    m[0, 8] = True
    m[10:12, 20] = True
    return m


KNOWN = [
    (lambda: np.pad(np.ones((2, 1), bool), ((1, 1), (1, 1))), [5, 2, 5], "525"),          # 4 x 3, rows 1..2 of column 1
    (lambda: np.ones((2, 2), np.uint8), [0, 4], "04"),
    (lambda: np.zeros((2, 2), np.uint8), [4], "4"),
    (_known_mask, [83, 34, 6, 34, 6, 34, 122, 2, 489, 2, 388], "c2R16000d3PO_;0kL"),
]
LONG_COUNTS, LONG_STRING = [1000, 1, 70000, 5, 3, 2000000], "Xo01`[T24cdkMkSQm1"


# ------------------------------------------------------------------------------------------------ the format
@pytest.mark.parametrize("make,counts,string", KNOWN)
def test_known_answers(make, counts, string):
    m = make()
    c = rle.encode(m)
    assert c.dtype == np.int64 and c.tolist() == counts == _encode_scalar(m)
    assert rle.to_string(c) == string == _to_string_scalar(counts)
    assert rle.from_string(string).tolist() == counts == _from_string_scalar(string)
    d = {"size": list(m.shape), "counts": string}
    assert np.array_equal(rle.decode(d), m.astype(bool)) and rle.area(d) == int(m.sum())
    assert rle.to_rle(c, m.shape) == d


def test_known_long_counts():
    assert rle.to_string(LONG_COUNTS) == LONG_STRING == _to_string_scalar(LONG_COUNTS)
    assert rle.from_string(LONG_STRING).tolist() == LONG_COUNTS == _from_string_scalar(LONG_STRING)


def test_column_wrap_is_one_run():
    m = np.zeros((40, 30), bool)
    m[39, 7] = m[0, 8] = True                           # the bottom of column 7 and the top of column 8: one run of 2
    assert rle.encode(m).tolist() == [7 * 40 + 39, 2, 30 * 40 - 7 * 40 - 41]


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 3), (64, 3), (65, 4), (130, 7)])
@pytest.mark.parametrize("density", [0.0, 0.3, 0.5, 1.0])
def test_mask_round_trips(H, W, density):
    g = np.random.default_rng(1000 * H + W + int(10 * density))
    m = g.random((H, W)) < density
    c = rle.encode(m)
    assert c.tolist() == _encode_scalar(m) and int(c.sum()) == H * W
    s = rle.to_string(c)
    assert s == _to_string_scalar(c.tolist())
    assert rle.from_string(s).tolist() == c.tolist()
    for d in ({"size": [H, W], "counts": s}, {"size": [H, W], "counts": c.tolist()}, {"size": [H, W], "counts": s.encode()}):
        back = rle.decode(d)
        assert back.dtype == bool and back.shape == (H, W) and np.array_equal(back, m)
        assert rle.area(d) == int(m.sum())
    assert rle.encode(m.astype(np.uint8)).tolist() == c.tolist()


def test_count_sequences_with_negative_differences_and_large_values():
    g = np.random.default_rng(5)
    seqs = [[0], [31], [15], [16], [1 << 20], [(1 << 31) - 1], [5, 1 << 20, 3, 1, (1 << 20) + 7, 2, 1 << 24, 1],
            [1 << 25, 1 << 25, 1, 1, 1 << 25, 1 << 25, 0, 0, 15, 16, 17, 1 << 30],
            g.integers(0, 1 << 22, size=301).tolist(), g.integers(0, 40, size=64).tolist(), (g.integers(0, 2, size=50) * (1 << 21)).tolist()]
    assert any(c[i] < c[i - 2] for c in seqs for i in range(3, len(c))) and any(v >= 1 << 20 for c in seqs for v in c)
    for c in seqs:
        s = rle.to_string(c)
        assert s == _to_string_scalar(c), c[:8]
        assert rle.from_string(s).tolist() == c == _from_string_scalar(s)
    # many sequences in one vectorised pass = each alone
    assert rle.to_strings(seqs) == [_to_string_scalar(c) for c in seqs]
    assert rle.to_strings([]) == []
    with pytest.raises(ValueError):
        rle.from_string("0~")
    with pytest.raises(ValueError):
        rle.from_string("P")                            # a continuation bit on the last character
    with pytest.raises(ValueError):
        rle.decode({"size": [2, 2], "counts": "3"})


def test_counts_from_starts():
    assert rle.counts_from_starts([], [], (4, 5)) == []
    got = rle.counts_from_starts(np.zeros(0, np.int32), [0, 0], (4, 5))
    assert [c.tolist() for c in got] == [[20], [20]]
    assert [c.tolist() for c in rle.counts_from_starts([5, 7], [2], (4, 3))] == [[5, 2, 5]]
    assert [c.tolist() for c in rle.counts_from_starts([0], [1], (2, 2))] == [[0, 4]]
    packed = np.array([5, 7, 0, 83, 117, 123], np.int32)
    got = rle.counts_from_starts(packed, np.array([2, 0, 1, 3]), (40, 30))
    assert [c.tolist() for c in got] == [[5, 2, 1193], [1200], [0, 1200], [83, 34, 6, 1077]] and all(c.dtype == np.int64 for c in got)
    assert [c.tolist() for c in rle.counts_from_starts(torch.tensor(packed).numpy(), torch.tensor([2, 0, 1, 3]).numpy(), (40, 30))] \
        == [c.tolist() for c in got]
    with pytest.raises(ValueError):
        rle.counts_from_starts([1, 2, 3], [2], (4, 4))
    # the starts of a mask are what encode differences
    m = _known_mask()
    f = m.T.reshape(-1)
    st = np.flatnonzero(f != np.concatenate(([False], f[:-1])))
    assert rle.counts_from_starts(st, [len(st)], m.shape)[0].tolist() == rle.encode(m).tolist()


# ------------------------------------------------------------------------------------------------ instances_to_coco_json
def _detections(n=3, H=12, W=10, masks=True):
    from afigan_amd.roi_heads import Detections
    from afigan_amd.rpn import Boxes
    g = torch.Generator().manual_seed(3)
    b = torch.tensor([(1.5, 2.0, 7.25, 9.0), (0.0, 0.0, 10.0, 12.0), (3.0, 4.5, 4.0, 6.0)])[:n]
    m = (torch.rand((n, H, W), generator=g) < 0.4) if masks else None
    return Detections((H, W), Boxes(b), torch.tensor([0.9, 0.75, 0.5])[:n], torch.tensor([1, 0, 4])[:n], m)


def test_instances_to_coco_json_on_cpu_detections():
    d = _detections()
    out = amd.instances_to_coco_json(d, 42)
    assert len(out) == 3
    for k, r in enumerate(out):
        assert set(r) == {"image_id", "category_id", "bbox", "score", "segmentation"}
        x0, y0, x1, y1 = d.pred_boxes.tensor[k].tolist()
        assert r["image_id"] == 42 and r["category_id"] == int(d.pred_classes[k]) and isinstance(r["category_id"], int)
        assert r["bbox"] == [x0, y0, x1 - x0, y1 - y0] and all(isinstance(v, float) for v in r["bbox"]) and isinstance(r["score"], float)
        assert r["score"] == float(d.scores[k])
        m = d.pred_masks[k].numpy()
        assert r["segmentation"] == {"size": [12, 10], "counts": rle.to_string(rle.encode(m))} and isinstance(r["segmentation"]["counts"], str)
        assert np.array_equal(rle.decode(r["segmentation"]), m)
    import json
    json.dumps(out)
    # pred_masks_rle is taken as it is, and wins over pred_masks
    given = [{"size": [12, 10], "counts": s} for s in ("a", "b", "c")]
    d.pred_masks_rle = given
    assert [r["segmentation"] for r in amd.instances_to_coco_json(d, 1)] == given
    d.pred_masks = None
    assert [r["segmentation"] for r in amd.instances_to_coco_json(d, 1)] == given
    assert d.to("cpu").pred_masks_rle == given
    # boxes only
    assert all(set(r) == {"image_id", "category_id", "bbox", "score"} for r in amd.instances_to_coco_json(_detections(masks=False), 0))
    # the empty case, keypoints, raw (not pasted) masks
    assert amd.instances_to_coco_json(_detections(n=0), 5) == []
    k = _detections()
    k.pred_keypoints = torch.zeros((3, 17, 3))
    with pytest.raises(amd.AfiError, match="pred_keypoints"):
        amd.instances_to_coco_json(k, 0)
    raw = _detections()
    raw.pred_masks = torch.zeros((3, 1, 28, 28))
    with pytest.raises(amd.AfiError, match="bool `pred_masks`"):
        amd.instances_to_coco_json(raw, 0)


class _Instances:
    """A stand-in with the interface of detectron2's Instances that the package relies on: a read-only image_size, fields of one length."""

    def __init__(self, image_size, **kw):
        self._image_size, self._fields = image_size, {}
        for k, v in kw.items():
            self.set(k, v)

    image_size = property(lambda self: self._image_size)

    def __setattr__(self, name, value):
        if name.startswith("_"):
            super().__setattr__(name, value)
        else:
            self.set(name, value)

    def __getattr__(self, name):
        if name == "_fields" or name not in self._fields:
            raise AttributeError(name)
        return self._fields[name]

    def set(self, name, value):
        assert all(len(v) == len(value) for v in self._fields.values()), "fields of one length"
        self._fields[name] = value

    def has(self, name):
        return name in self._fields

    def get(self, name):
        return self._fields[name]

    def get_fields(self):
        return self._fields

    def __len__(self):
        return len(next(iter(self._fields.values()))) if self._fields else 0


def test_instances_like_objects():
    from afigan_amd.rcnn_extractor import _detector_postprocess_boxes
    from afigan_amd.rpn import Boxes
    d = _detections()
    inst = _Instances((12, 10), pred_boxes=d.pred_boxes, scores=d.scores, pred_classes=d.pred_classes, pred_masks=d.pred_masks)
    assert amd.instances_to_coco_json(inst, 9) == amd.instances_to_coco_json(d, 9)
    # the box part of the postprocess on such an object: a new object at the output size with the kept rows, the input untouched
    b = torch.tensor([(1.0, 2.0, 6.0, 8.0), (20.0, 2.0, 30.0, 8.0), (2.0, 3.0, 4.0, 5.0)])       # the second is clipped to nothing
    src = _Instances((12, 10), pred_boxes=Boxes(b), scores=torch.tensor([0.9, 0.8, 0.7]), pred_classes=torch.tensor([1, 2, 3]))
    r = _detector_postprocess_boxes(src, 24, 20, mask_format="rle")
    assert r is not src and r.image_size == (24, 20) and src.image_size == (12, 10) and len(src) == 3 and len(r) == 2
    assert torch.equal(r.pred_boxes.tensor, torch.tensor([(2.0, 4.0, 12.0, 16.0), (4.0, 6.0, 8.0, 10.0)]))
    assert torch.equal(r.scores, torch.tensor([0.9, 0.7])) and torch.equal(r.pred_classes, torch.tensor([1, 3])) and not r.has("pred_masks_rle")
    assert torch.equal(src.pred_boxes.tensor, b)


def test_mask_format_is_checked_before_anything_runs():
    from afigan_amd.rcnn_extractor import _detector_postprocess_boxes
    stub = types.SimpleNamespace(training=False)
    with pytest.raises(amd.AfiError, match="mask_format must be 'bitmask' or 'rle', got 'polygon'"):
        amd.GeneralizedRCNN_AFExtractor.inference(stub, [], mask_format="polygon")
    with pytest.raises(amd.AfiError, match="mask_format"):
        _detector_postprocess_boxes(_detections(masks=False), 24, 20, mask_format="polygon")
    d = _detections()                                   # CPU masks: refused under either format, as before
    d.pred_masks = torch.zeros((3, 1, 28, 28))
    for fmt in ("bitmask", "rle"):
        with pytest.raises(amd.AfiError, match=r"pred_masks.*GPU only.*CPU tensor"):
            _detector_postprocess_boxes(d, 24, 20, mask_format=fmt)
    r = _detector_postprocess_boxes(_detections(masks=False), 24, 20, mask_format="rle")
    assert r.image_size == (24, 20) and r.pred_masks is None and r.pred_masks_rle is None


def test_wrappers_refuse_cpu_tensors():
    from afigan_amd import ops
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        ops.mask_paste_rle(torch.zeros((1, 28, 28)), torch.zeros((1, 4)), (8, 8))
    with pytest.raises(amd.AfiError, match="GPU"):
        amd.paste_masks_rle(torch.zeros((1, 28, 28)), torch.zeros((1, 4)), (8, 8))


# ------------------------------------------------------------------------------------------------ the C-ABI without a device
def test_entry_points_check_their_arguments_without_a_device():
    """AFI_ERR_BAD_ARG / AFI_ERR_UNSUPPORTED come back before anything is launched (fake, never dereferenced pointers)."""
    from afigan_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.DEFINES["AFI_ERR_BAD_ARG"], _lib.DEFINES["AFI_ERR_UNSUPPORTED"]
    assert _lib.ABI_VERSION == 9 and lib.afi_abi_version() == 9
    ws = lib.afi_mask_rle_ws_bytes
    assert ws(1, 8, 8) == 8 * 8 + 32 and ws(1, 1, 9) == 9 * 8 + 40 and ws(3, 65, 5) == 3 * 2 * 5 * 8 + 64 and ws(0, 8, 8) == 0
    assert ws(200, 800, 1333) == 200 * 13 * 1333 * 8 + 200 * 1333 * 4
    assert ws(-1, 8, 8) == -1 and ws(1, 0, 8) == -1 and ws(1, 8, 0) == -1
    assert ws(1, 65536, 32768) == -1 and ws(1, 65536, 32767) > 0           # H W < 2^31
    assert ws(1, 2097121, 1) == -1 and ws(1, 2097120, 1) > 0               # afi_mask_paste's bound on H
    p, n = 0x1000, ws(1, 8, 8)
    cnt, emit = lib.afi_mask_rle_count, lib.afi_mask_rle_emit
    for args in ((None, p, 1, 28, 8, 8, 0.5, p, n, p), (p, None, 1, 28, 8, 8, 0.5, p, n, p), (p, p, 1, 28, 8, 8, 0.5, None, n, p),
                 (p, p, 1, 28, 8, 8, 0.5, p, n, None), (p, p, -1, 28, 8, 8, 0.5, p, n, p), (p, p, 1, 0, 8, 8, 0.5, p, n, p),
                 (p, p, 1, 28, 0, 8, 0.5, p, n, p), (p, p, 1, 28, 8, 0, 0.5, p, n, p), (p, p, 1, 28, 8, 8, 0.5, p, n - 1, p)):
        assert cnt(*args, None) == BAD, args
    for args in ((p, p, 1, 65, 8, 8, 0.5, p, n, p), (p, p, 1, 28, 65536, 32768, 0.5, p, 1 << 40, p), (p, p, 1, 28, 2097121, 1, 0.5, p, 1 << 40, p),
                 (p, p, 1, 28, 8, 8, 0.5, p + 4, n, p), (p + 2, p, 1, 28, 8, 8, 0.5, p, n, p)):
        assert cnt(*args, None) == UNS, args
    assert cnt(None, None, 0, 28, 8, 8, 0.5, None, 0, None, None) == 0                     # R = 0 launches nothing
    for args in ((None, 1, 8, 8, p, n, p, p), (p, 1, 8, 8, None, n, p, p), (p, 1, 8, 8, p, n, None, p), (p, 1, 8, 8, p, n, p, None),
                 (p, -1, 8, 8, p, n, p, p), (p, 1, 0, 8, p, n, p, p), (p, 1, 8, 8, p, n - 1, p, p)):
        assert emit(*args, None) == BAD, args
    for args in ((p, 1, 65536, 32768, p, 1 << 40, p, p), (p, 1, 8, 8, p + 4, n, p, p), (p, 1, 8, 8, p, n, p + 4, p)):
        assert emit(*args, None) == UNS, args
    assert emit(None, 0, 8, 8, None, 0, None, None, None) == 0


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def _decided(H, W, M):
    probs, boxes = G.case(H, W, M)
    v, e, inside = Q.paste(probs, boxes, H, W)
    want, sure = Q.paste_decided(v, e, inside)
    return probs, boxes, want, sure


def test_gpu_cases_hold_the_run_shapes_on_the_checker_alone():
    """Conditions on the inputs, decided by the fp64 checker on pixels it is sure of -- not measurements of the kernels."""
    assert G.OLD_CASES[0] in Q.PASTE_CASES and G.OLD_CASES[1] in Q.PASTE_CASES
    seen = {k: [] for k in ("wrap", "ends at the bottom", "last pixel", "first pixel", "empty", "more than 64 starts")}
    for H, W, M in G.NEW_CASES:
        probs, boxes, want, sure = _decided(H, W, M)
        assert len(boxes) == 13 and probs.shape == (13, M, M) and probs.dtype == np.float32 and boxes.dtype == np.float32
        finite = np.isfinite(boxes).all(1)
        assert finite.sum() == 12 and np.isnan(boxes[10]).any() and not np.isinf(boxes).any()
        # the two fixed answers, and the boxes that must give nothing
        assert sure[G.ALL_ONES].all() and want[G.ALL_ONES].all(), "the all-ones mask in the whole-image box must set every pixel"
        assert not want[G.ALL_ZEROS].any() and sure[G.ALL_ZEROS].all()
        for r in (6, 8, 9, 10):
            assert sure[r].all() and not want[r].any(), r
        assert want[7].sum() == 1 and sure[7].all(), "the sub-pixel box around one centre sets that pixel"
        assert (want & sure).any(axis=(1, 2)).sum() >= 6, "most boxes of the case must set pixels"
        for r in range(13):
            w, s = want[r], sure[r]
            if W > 1:
                bot, top, sb = w[H - 1, :-1], w[0, 1:], s[H - 1, :-1] & s[0, 1:]
                if (bot & top & sb).any():
                    seen["wrap"].append((H, W, r))
                if (bot & ~top & sb).any():
                    seen["ends at the bottom"].append((H, W, r))
            if w[H - 1, W - 1] and s[H - 1, W - 1]:
                seen["last pixel"].append((H, W, r))
            if w[0, 0] and s[0, 0]:
                seen["first pixel"].append((H, W, r))
            if s.all() and not w.any():
                seen["empty"].append((H, W, r))
            if s.all() and len(rle.encode(w)) - 1 > 64:
                seen["more than 64 starts"].append((H, W, r))
    for k, v in seen.items():
        print(f"[rle cases] {k}: {len(v)} detections, e.g. {v[:4]}")
        assert v, k
    # on the cases that have more than one row and word: every shape but the trivial ones shows in a random mask, not only in the all-ones one
    for k in ("wrap", "ends at the bottom", "more than 64 starts"):
        assert any(r not in (G.ALL_ONES, G.ALL_ZEROS) for _, _, r in seen[k]), k
    assert any(r not in (G.ALL_ONES,) for _, _, r in seen["last pixel"]) and any(r not in (G.ALL_ONES,) for _, _, r in seen["first pixel"])
    # a run that wraps and a word edge: some sure, set pixel pair (63, x), (64, x) and some set (63, x) with (64, x) clear
    for H, W, M in ((65, 5, 7), (130, 40, 28), (300, 20, 28)):
        _, _, want, sure = _decided(H, W, M)
        pair = sure[:, 63] & sure[:, 64]
        assert (want[:, 63] & want[:, 64] & pair).any() and (want[:, 63] & ~want[:, 64] & pair)[2:].any(), (H, W)
