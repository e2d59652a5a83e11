"""The polygon rasteriser without a GPU: the plain-loop checker tests/poly_f64.py on the cases whose answers are known, the conditions the GPU
tests' inputs must meet (decided by the checker alone), the argument checks of the entry points, the workspace query and the host refusals."""
import numpy as np
import pytest

import poly_cases as PC
import poly_f64 as Q

import afigan_amd as amd
from afigan_amd import _lib, ops, rle


# ------------------------------------------------------------------------------------------------ the checker
@pytest.mark.parametrize("case", range(len(PC.HAND)))
def test_checker_reproduces_the_hand_cases(case):
    xy, (H, W), ncross, nstarts, area, extent = PC.HAND[case]
    starts = Q.poly_starts(xy, H, W)
    m = Q.poly_mask(xy, H, W)
    assert len(Q.crossings(xy, H, W)) == ncross and len(starts) == nstarts and int(m.sum()) == area
    assert starts == sorted(set(starts)) and all(0 <= a < H * W for a in starts)
    assert Q.ann_starts([xy], H, W) == starts                               # the union of one polygon is the polygon
    assert rle.area(rle.to_rle(Q.ann_counts([xy], H, W), (H, W))) == area
    if extent is not None:
        x0, x1, y0, y1 = extent
        want = np.zeros((H, W), bool)
        want[y0:y1 + 1, x0:x1 + 1] = True
        assert np.array_equal(m, want)


def test_checker_on_degenerate_polygons_and_the_union():
    seen = {}
    for xy, (H, W), what in PC.special_polygons():
        cr, st = Q.crossings(xy, H, W), Q.poly_starts(xy, H, W)
        assert all(0 <= a <= H * W for a in cr), what
        seen[what] = (cr, st)
    assert seen["one vertex"] == ([], []) and seen["two vertices"][1] == [] and len(seen["two vertices"][0]) > 0   # out and back: every crossing twice
    assert seen["left of and above the canvas"] == ([], []) and seen["right of the canvas"] == ([], [])
    assert seen["below the canvas"][1] == [] and len(seen["below the canvas"][0]) > 0                              # clamped to the column ends: pairs
    for what in ("covers the whole canvas", "the canvas itself"):
        assert seen[what][1] == [0] and 72 in seen[what][0], what             # crossings land at a = H W and are dropped
    assert len(seen["repeated consecutive vertices"][1]) > 0
    cases, starts = PC.union_set(), PC.union_set_starts()
    by = {what: (ps, hw, st) for (ps, hw, what), st in zip(cases, starts)}
    ps, (H, W), st = by["identical twice"]
    assert st == Q.poly_starts(ps[0], H, W) and len(st) == 20
    assert by["no polygon"][2] == []
    ps, (H, W), st = by["nested"]
    assert st == Q.poly_starts(ps[0], H, W)
    ps, (H, W), st = by["disjoint"]
    assert sorted(st) == sorted(Q.poly_starts(ps[0], H, W) + Q.poly_starts(ps[1], H, W))
    ps, (H, W), st = by["overlapping"]
    assert len(st) < len(Q.poly_starts(ps[0], H, W)) + len(Q.poly_starts(ps[1], H, W))
    assert len({hw for _, hw, _ in cases}) >= 6 and {len(ps) for ps, _, _ in cases} >= {0, 1, 2, 3, 4}


def test_gpu_inputs_meet_their_conditions_on_the_checker_alone():
    """What tests/test_gpu_poly.py needs of its inputs, none of it a measurement of the kernels: the random set reaches every kind of polygon and
    canvas, at least 3 of its polygons get other starts from the fused form fma(s, t, ys) of step 2 (so a contracted kernel cannot pass), and
    the zigzags have exactly the crossings that put them on either side of the LDS capacity."""
    cases, plain, fused = PC.random_set(), PC.random_set_starts(), PC.random_set_starts(fused=True)
    assert len(cases) == PC.RANDOM_N + len(PC.special_polygons()) and 300 <= PC.RANDOM_N <= 500
    differ = [i for i, (a, b) in enumerate(zip(plain, fused)) if a != b]
    print(f"[poly] fused form changes the starts of polygons {differ}")
    assert len(differ) >= 3
    sizes = {hw for _, hw in cases}
    assert (5, 5) in sizes and (40, 37) in sizes and any(h == 1 for h, _ in sizes) and any(w == 1 for _, w in sizes)
    assert {len(p) // 2 for p, _ in cases} >= set(range(1, 13))
    kinds = set()
    for p, _ in cases[:PC.RANDOM_N]:
        kinds.add("integer" if all(float(v).is_integer() for v in p) else "half" if all(float(2 * v).is_integer() for v in p) else "arbitrary")
        assert min(p) >= -6 and max(p) <= 46
    assert kinds == {"integer", "half", "arbitrary"}
    assert sum(len(s) == 0 for s in plain) >= 5 and max(len(s) for s in plain) > 64
    cap = _lib.DEFINES["AFI_POLY_RLE_LDS_CAP"]
    assert cap % 4 == 0
    for n in (cap - 2, cap, cap + 2):                                        # (a closed boundary has an even number of crossings: see zigzag_case)
        xy, (H, W) = PC.zigzag_case(n)
        assert len(Q.crossings(xy, H, W)) == n and H == 8


# ------------------------------------------------------------------------------------------------ the host side of ops.polygons_rle
def test_batch_layout_and_capacity_bound():
    polys = [[[2, 2, 8, 2, 8, 7, 2, 7]], [], [[1, 1, 12, 3, 6, 10], [3.0, 4.0]]]
    xy, voff, poff, hw, cap = ops.polygons_batch(polys, [(12, 14), (5, 5), (12, 14)])
    assert xy.dtype == np.float64 and xy.shape == (8, 2) and voff.tolist() == [0, 4, 7, 8] and poff.tolist() == [0, 1, 1, 3]
    assert hw.dtype == np.int32 and hw.tolist() == [[12, 14], [5, 5], [12, 14]]
    # sum over edges of (dx / 5 + 2), dx in upsampled units: the box 30 / 5 + 2 twice and 0 / 5 + 2 twice; the triangle 55, 30, 25; the point 0
    assert cap.dtype == np.int64 and cap.tolist() == [0, 20, 20 + 13 + 8 + 7, 50]
    assert ops.polygons_batch(polys, (12, 14))[3].tolist() == [[12, 14]] * 3
    # the bound holds for every polygon of the GPU tests (the kernel refuses a mask whose crossings exceed it)
    for p, (H, W) in PC.random_set():
        c = ops.polygons_batch([[p]], (H, W))[4]
        assert len(Q.crossings(p, H, W)) <= int(c[-1])
    xy, voff, poff, hw, cap = ops.polygons_batch([], (4, 4))
    assert xy.shape == (0, 2) and voff.tolist() == [0] and poff.tolist() == [0] and hw.shape == (0, 2) and cap.tolist() == [0]


def test_host_refusals_before_anything_is_uploaded():
    box = [1.0, 1.0, 5.0, 1.0, 5.0, 5.0]
    for bad, match in (([[[1.0, float("nan"), 2.0, 2.0]]], "non-finite"), ([[[1.0, float("inf"), 2.0, 2.0]]], "non-finite"),
                       ([[[1.0, 1.0, float(2 ** 30) / 5, 2.0]]], r"2\^30"), ([[[1.0, 1.0, -float(2 ** 30) / 5 - 1, 2.0]]], r"2\^30"),
                       ([[[]]], "0 coordinates"), ([[[1.0, 2.0, 3.0]]], "3 coordinates"), ([{"size": [4, 4], "counts": [16]}], "not a list of polygons")):
        for fn in (ops.polygons_batch, ops.polygons_rle, rle.from_polygons, amd.polygons_to_rle):
            with pytest.raises(amd.AfiError, match=match):
                fn(bad, (8, 8))
    ops.polygons_batch([[[1.0, 1.0, float(2 ** 30 - 1) / 5, 2.0]]], (8, 8))                   # below the bound: accepted
    for sizes, match in (((65536, 32768), r"H W < 2\^31"), ((0, 8), "H, W > 0"), ([(8, 8), (8, 8)], "one pair per annotation"), ((8, 8, 8), "one pair per annotation")):
        with pytest.raises(amd.AfiError, match=match):
            ops.polygons_batch([[box]], sizes)
    ops.polygons_batch([[box]], (65536, 32767))
    with pytest.raises(amd.AfiError, match="GPU only"):
        ops.polygons_rle([[box]], (8, 8), device="cpu")
    assert amd.polygons_to_rle is rle.from_polygons


def test_wrappers_refuse_cpu_tensors():
    import torch
    with pytest.raises(amd.AfiError, match="GPU"):
        ops.rle_decode(torch.zeros((0,), dtype=torch.int32), torch.zeros((2,), dtype=torch.int64), (4, 4))
    with pytest.raises(amd.AfiError, match="H W < 2"):
        ops.rle_decode(torch.zeros((0,), dtype=torch.int32), torch.zeros((2,), dtype=torch.int64), (65536, 32768))


# ------------------------------------------------------------------------------------------------ the C-ABI without a device
def test_entry_points_check_their_arguments_without_a_device():
    """AFI_ERR_BAD_ARG / AFI_ERR_UNSUPPORTED come back before anything is launched (fake, never dereferenced pointers)."""
    lib = _lib.load()
    BAD, UNS = _lib.DEFINES["AFI_ERR_BAD_ARG"], _lib.DEFINES["AFI_ERR_UNSUPPORTED"]
    assert _lib.ABI_VERSION == 9 and lib.afi_abi_version() == 9              # additive: the ABI stays
    assert _lib.DEFINES["AFI_POLY_RLE_LDS_CAP"] == 4096
    ws = lib.afi_poly_rle_ws_bytes
    assert ws(0) == 0 and ws(1) == 8 + 8 and ws(2) == 16 + 8 and ws(3) == 24 + 16 and ws(1000) == 12000
    assert ws(-1) == -1 and ws(1 << 31) == -1 and ws((1 << 31) - 1) > 0
    p, n = 0x1000, ws(100)
    cnt, emit, dec = lib.afi_poly_rle_count, lib.afi_poly_rle_emit, lib.afi_rle_decode
    good = (p, p, p, p, p, 1, 100, p, n, p)
    for i in (0, 1, 2, 3, 4, 7, 9):                                           # every pointer null in turn
        assert cnt(*(None if j == i else v for j, v in enumerate(good)), None) == BAD, i
    for args in ((p, p, p, p, p, -1, 100, p, n, p), (p, p, p, p, p, 1, -1, p, n, p), (p, p, p, p, p, 1, 100, p, n - 1, p)):
        assert cnt(*args, None) == BAD, args
    for i, off in ((0, 4), (1, 4), (2, 4), (3, 2), (4, 4), (7, 4), (9, 2)):  # every pointer off its alignment in turn
        assert cnt(*(v + off if j == i else v for j, v in enumerate(good)), None) == UNS, i
    assert cnt(p, p, p, p, p, 1, 1 << 31, p, 1 << 40, p, None) == UNS
    assert cnt(None, None, None, None, None, 0, 0, None, 0, None, None) == 0  # N = 0 launches nothing
    good = (p, p, 1, 100, p, n, p, p)
    for i in (0, 1, 4, 6, 7):
        assert emit(*(None if j == i else v for j, v in enumerate(good)), None) == BAD, i
    for args in ((p, p, -1, 100, p, n, p, p), (p, p, 1, -1, p, n, p, p), (p, p, 1, 100, p, n - 1, p, p)):
        assert emit(*args, None) == BAD, args
    for i, off in ((0, 4), (1, 4), (4, 4), (6, 4), (7, 2)):
        assert emit(*(v + off if j == i else v for j, v in enumerate(good)), None) == UNS, i
    assert emit(None, None, 0, 0, None, 0, None, None, None) == 0
    good = (p, p, 1, 8, 8, p)
    for i in (0, 1, 5):
        assert dec(*(None if j == i else v for j, v in enumerate(good)), None) == BAD, i
    for args in ((p, p, -1, 8, 8, p), (p, p, 1, 0, 8, p), (p, p, 1, 8, 0, p)):
        assert dec(*args, None) == BAD, args
    for args in ((p + 2, p, 1, 8, 8, p), (p, p + 4, 1, 8, 8, p), (p, p, 1, 65536, 32768, p), (p, p, 1 << 30, 1, 129, p)):
        assert dec(*args, None) == UNS, args
    assert dec(None, None, 0, 8, 8, None, None) == 0


# ------------------------------------------------------------------------------------------------ the evaluator
def _polygon_gt(images=True):
    gt = {"images": [{"id": 1, "height": 20, "width": 30}], "categories": [{"id": 1, "name": "a"}],
          "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "bbox": [2, 2, 6, 5], "area": 30.0, "iscrowd": 0,
                           "segmentation": [[2, 2, 8, 2, 8, 7, 2, 7]]}]}
    if not images:
        gt["images"] = [{"id": 1, "width": 30}]
    return gt


def test_evaluator_refuses_polygons_by_default_and_a_missing_image_size():
    with pytest.raises(amd.AfiError, match="rasterize_polygons=True"):        # the default keeps refusing, and names the keyword
        amd.COCOEvaluator(_polygon_gt(), tasks=("segm",))
    with pytest.raises(amd.AfiError, match="height"):                         # before the device is touched
        amd.COCOEvaluator(_polygon_gt(images=False), tasks=("segm",), rasterize_polygons=True)
    bad = _polygon_gt()
    bad["annotations"][0]["segmentation"] = [[2, 2, 8]]
    with pytest.raises(amd.AfiError, match="3 coordinates"):
        amd.COCOEvaluator(bad, tasks=("segm",), rasterize_polygons=True)
    amd.COCOEvaluator(_polygon_gt(), tasks=("bbox",), rasterize_polygons=True)  # polygons do not matter to bbox


def test_mapper_bitmask_refusals():
    from afigan_amd.dual_scale import DualScaleMapper
    with pytest.raises(amd.AfiError, match="GPU"):
        DualScaleMapper(mask_on=True, mask_format="bitmask", device="cpu")
    with pytest.raises(amd.AfiError, match="INPUT.CROP"):
        DualScaleMapper(mask_on=True, mask_format="bitmask", device="cuda", crop=("relative", (0.8, 0.8)))
    with pytest.raises(amd.AfiError, match="MASK_FORMAT"):
        DualScaleMapper(mask_on=True, mask_format="rle", device="cuda")
