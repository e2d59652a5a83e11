"""Pasted masks as COCO run-length starts on the GPU (csrc/mask_rle.hip, ops.mask_paste_rle, roi_heads.paste_masks_rle, the extractor's
``mask_format="rle"``) against afi_mask_paste's own bytes: the counts of every detection equal rle.encode of the pasted mask, exactly -- there is
no tolerance anywhere in this file.  tests/test_rle_host.py proves without a GPU, on the fp64 checker, that the seeded cases built here hold the
run shapes the kernels can get wrong (a run that wraps from the bottom of a column into the next, one that ends there, a set last pixel, a set
first pixel, an empty mask, more than 64 starts)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mask_f64 as Q

pytestmark = pytest.mark.gpu

# (H, W, M): one row; the 64-row word edge from both sides; three words, the last partial; two row bands; two column chunks
NEW_CASES = ((1, 9, 7), (64, 5, 7), (65, 5, 7), (130, 40, 28), (300, 20, 28), (20, 300, 28))
OLD_CASES = ((37, 53, 28), (16, 32, 7))                 # mask_f64.paste_case, as test_gpu_mask.py runs it
RLE_SEED = 11
ALL_ONES, ALL_ZEROS = 0, 1                              # rows of rle_case: counts [0, H W] and [H W]


def rle_case(H, W, M, seed=RLE_SEED):
    """(probs [13, M, M], boxes [13, 4]) fp32.  No box has a non-finite coordinate but the NaN side of row 10."""
    nan = float("nan")
    boxes = np.array([
        (0, 0, W, H),                                               # 0 whole image, all-ones mask
        (0, 0, W, H),                                               # 1 whole image, all-zero mask
        (0, 0, W, H),                                               # 2 whole image, binary random mask
        (0.2 * W, 0.3 * H, 0.8 * W + 0.3, H),                       # 3 touches the bottom, binary random
        (-3.5, -2.25, 0.6 * W, 0.7 * H),                            # 4 exceeds left and top, smooth
        (0.3 * W, 0.4 * H, W + 4.5, H + 7.25),                      # 5 exceeds right and bottom, binary random
        (0.5 * W + 0.25, 0.5 * H + 0.5625, 0.5 * W + 0.75, 0.5 * H + 0.875),      # 6 sides below one pixel, no row centre inside
        (int(0.4 * W) + 0.3, int(0.4 * H) + 0.2, int(0.4 * W) + 0.9, int(0.4 * H) + 0.9),     # 7 sides below one pixel around one centre
        (0.5 * W, 0, 0.5 * W, H),                                   # 8 zero width
        (0.7 * W, 0, 0.2 * W, H),                                   # 9 negative width
        (1, 0, nan, H),                                             # 10 a NaN side
        (0.1 * W, 0.15 * H, 0.9 * W, 0.85 * H),                     # 11 inside, smooth
        (-6.5, -4.75, W + 5.25, H + 3.5),                           # 12 exceeds every edge, smooth
    ], np.float32)
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    probs = np.zeros((len(boxes), M, M), np.float32)
    for r in range(len(boxes)):
        if r == ALL_ONES:
            probs[r] = 1.0
        elif r == ALL_ZEROS:
            probs[r] = 0.0
        elif r in (2, 3, 5, 7):
            probs[r] = (torch.rand((M, M), generator=g) < 0.5).numpy()
        else:
            low = torch.randn((1, 1, 4, 4), generator=g, dtype=torch.float64) * 2.5
            probs[r] = torch.sigmoid(F.interpolate(low, size=(M, M), mode="bicubic", align_corners=False))[0, 0].numpy().clip(0, 1)
    probs[7] = 1.0                                                  # the one pixel is set
    return probs, boxes


def case(H, W, M):
    return Q.paste_case(H, W, M) if (H, W, M) in OLD_CASES else rle_case(H, W, M)


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


_PASTED = {}


def _pasted_counts(H, W, M):
    """The oracle, computed once per case: afi_mask_paste's masks (bool numpy) and rle.encode of each."""
    if (H, W, M) not in _PASTED:
        from afigan_amd import ops, rle
        probs, boxes = case(H, W, M)
        masks = ops.mask_paste(torch.from_numpy(probs).cuda(), torch.from_numpy(boxes).cuda(), (H, W)).cpu().numpy()
        masks.setflags(write=False)
        _PASTED[(H, W, M)] = (masks, [rle.encode(m) for m in masks])
    return _PASTED[(H, W, M)]


def _run(H, W, M, ws=None):
    from afigan_amd import ops
    probs, boxes = case(H, W, M)
    starts, nstarts = ops.mask_paste_rle(torch.from_numpy(probs).cuda(), torch.from_numpy(boxes).cuda(), (H, W), 0.5, ws=ws)
    assert starts.dtype == torch.int32 and starts.is_cuda and nstarts.dtype == torch.int64 and not nstarts.is_cuda
    return starts.cpu().numpy(), nstarts.numpy()


@pytest.mark.parametrize("H,W,M", OLD_CASES + NEW_CASES)
def test_counts_equal_the_pasted_masks(amd, H, W, M):
    from afigan_amd import rle
    masks, want = _pasted_counts(H, W, M)
    starts, nstarts = _run(H, W, M)
    got = rle.counts_from_starts(starts, nstarts, (H, W))
    print(f"[rle] {H}x{W} M {M}: {len(want)} detections, starts per detection {nstarts.tolist()}, {int(masks.sum())} pixels set")
    assert nstarts.tolist() == [len(c) - 1 for c in want]
    for r, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (r, g[:12], w[:12])
    if (H, W, M) in NEW_CASES:
        assert got[ALL_ONES].tolist() == [0, H * W] and got[ALL_ZEROS].tolist() == [H * W]


@pytest.mark.parametrize("H,W,M", [(130, 40, 28), (300, 20, 28), (20, 300, 28)])
def test_workspace_content_does_not_matter(amd, H, W, M):
    """The same call on a workspace full of 0xFF bytes, and again after another case has used that workspace."""
    other = (65, 5, 7) if (H, W, M) != (300, 20, 28) else (20, 300, 28)
    lib = amd._lib.load()
    n = max(lib.afi_mask_rle_ws_bytes(13, H, W), lib.afi_mask_rle_ws_bytes(13, other[0], other[1]))
    fresh = _run(H, W, M)
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    dirty = _run(H, W, M, ws=ws)
    _run(*other, ws=ws)
    again = _run(H, W, M, ws=ws)
    for name, (s, k) in (("0xFF-filled", dirty), ("used by another case", again)):
        assert np.array_equal(k, fresh[1]) and np.array_equal(s, fresh[0]), name
    with pytest.raises(amd.AfiError, match="ws must be"):
        _run(H, W, M, ws=ws[:lib.afi_mask_rle_ws_bytes(13, H, W) - 1])


def test_two_runs_are_bit_identical_and_non_finite_boxes_are_empty(amd):
    from afigan_amd import ops
    a, b = _run(130, 40, 28), _run(130, 40, 28)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    inf, nan = float("inf"), float("nan")
    boxes = torch.tensor([(-inf, 0, 20, 100), (0, -inf, 20, 100), (3, 0, inf, 100), (3, 2, 20, inf), (-inf, -inf, inf, inf), (nan, 0, 20, 100),
                          (0, 0, 20, nan), (inf, inf, inf, inf)], dtype=torch.float32, device="cuda")
    starts, nstarts = ops.mask_paste_rle(torch.ones((len(boxes), 28, 28), device="cuda"), boxes, (130, 40))
    assert nstarts.tolist() == [0] * len(boxes) and starts.numel() == 0


def test_mask_paste_rle_refusals_and_the_empty_list(amd):
    from afigan_amd import ops
    p, b = torch.zeros((2, 28, 28), device="cuda"), torch.zeros((2, 4), device="cuda")
    with pytest.raises(amd.AfiError):
        ops.mask_paste_rle(torch.zeros((2, 65, 65), device="cuda"), b, (8, 8))
    with pytest.raises(amd.AfiError):
        ops.mask_paste_rle(p, b[:1], (8, 8))
    with pytest.raises(amd.AfiError):
        ops.mask_paste_rle(p, b, (0, 8))
    with pytest.raises(amd.AfiError):
        ops.mask_paste_rle(p, b, (65536, 32768))
    starts, nstarts = ops.mask_paste_rle(p[:0], b[:0], (8, 8))
    assert starts.shape == (0,) and starts.dtype == torch.int32 and nstarts.shape == (0,)
    starts, nstarts = ops.mask_paste_rle(p, b, (8, 8))                  # zero boxes: no start at all, the emit is skipped
    assert starts.numel() == 0 and nstarts.tolist() == [0, 0]


@pytest.mark.parametrize("H,W,M", [(37, 53, 28), (130, 40, 28)])
def test_paste_masks_rle_equals_the_encoded_bitmasks(amd, H, W, M):
    from afigan_amd import rle
    probs, boxes = case(H, W, M)
    p, b = torch.from_numpy(probs).cuda(), torch.from_numpy(boxes).cuda()
    masks = amd.paste_masks_in_image(p[:, None], b, (H, W)).cpu().numpy()
    got = amd.paste_masks_rle(p[:, None], b, (H, W))
    assert len(got) == len(boxes)
    for r, d in enumerate(got):
        assert d["size"] == [H, W] and isinstance(d["counts"], str)
        assert d["counts"] == rle.to_string(rle.encode(masks[r])), r
        assert np.array_equal(rle.decode(d), masks[r]) and rle.area(d) == int(masks[r].sum())
    assert amd.paste_masks_rle(p[:0], b[:0], (H, W)) == []
    with pytest.raises(amd.AfiError, match="GPU"):
        amd.paste_masks_rle(p.cpu(), b.cpu(), (H, W))


def test_detector_inference_with_rle_masks(amd):
    """The 64 x 80 detector of test_gpu_mask.py::test_detector_inference_returns_pasted_masks, once per mask format."""
    from afigan_amd import rle
    from afigan_amd.fpn_sr import ShapeSpec
    from test_gpu_mask import LEVELS4, _gpu_kernel_names, _heads
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
        heads.mask_head.predictor.bias.fill_(0.3)              # so that some pixels are set
    det = amd.GeneralizedRCNN_AFExtractor(backbone=Backbone(), proposal_generator=rpn, roi_heads=heads, pixel_mean=[100.0, 110.0, 120.0],
                                          pixel_std=[50.0, 55.0, 60.0]).eval()
    inputs = [{"image_x0.5": torch.rand((3, 64, 80), generator=g) * 255, "height": 128, "width": 160},
              {"image_x0.5": torch.rand((3, 57, 71), generator=g) * 255, "height": 114, "width": 142}]
    with torch.no_grad():
        ref = det.inference(inputs)
        kernels, _ = _gpu_kernel_names(lambda: det.inference(inputs, mask_format="rle"))
        out = det.inference(inputs, mask_format="rle")
    assert not any("afi_mask_paste" in k for k in kernels) and any("afi_mask_rle_bits" in k for k in kernels) \
        and any("afi_mask_rle_starts" in k for k in kernels), sorted(set(kernels))
    total = 0
    for i, (o, rf, inp) in enumerate(zip(out, ref, inputs)):
        r, q = o["instances"], rf["instances"]
        n = len(q)
        assert len(r) == n and torch.equal(r.pred_boxes.tensor, q.pred_boxes.tensor) and torch.equal(r.scores, q.scores) \
            and torch.equal(r.pred_classes, q.pred_classes)
        assert getattr(r, "pred_masks", None) is None and len(r.pred_masks_rle) == n
        for d, m in zip(r.pred_masks_rle, q.pred_masks.cpu().numpy()):
            assert d["size"] == [inp["height"], inp["width"]] and np.array_equal(rle.decode(d), m)
            total += int(m.sum())
        a, b = amd.instances_to_coco_json(r, 7 + i), amd.instances_to_coco_json(q, 7 + i)
        assert len(a) == n and a == b
        assert all(isinstance(d["segmentation"]["counts"], str) and d["image_id"] == 7 + i for d in a)
    assert total > 0, "no mask pixel at all: the test would show nothing"
    with pytest.raises(amd.AfiError, match="mask_format"):
        det.inference(inputs, mask_format="polygon")
