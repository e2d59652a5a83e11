"""The wide forms of the RPN's selection stages on the GPU (csrc/rpn.hip: afi_rpn_topk_wide, afi_rpn_nms_wide, afi_rpn_merge_wide) --
per-level lists of 1025 .. 4096 entries, PRE_NMS_TOPK_TRAIN = 2000 of the reference's base config among them -- against tests/rpn_f64.py.  Every
comparison is equality; the scheme is tests/test_gpu_rpn.py's (each stage's checker consumes the KERNEL's previous stage output):
  1. top-k      indices and values equal the stable descending sort; direct and filtered maps, k = n, ties / equal / +-0 / NaN logits, column slices;
  2. NMS        the exact keep set on lists held to the two conditions first (no pair's fp64 IoU within 1e-5 of the threshold, 10 % .. 90 % kept;
                tests/test_rpn_wide_host.py asserts them without a GPU); invalid boxes, n = 1 and 0, ld > k, a NaN-filled workspace; on lists of
                <= 1024 the keep array of afi_rpn_nms, bit for bit;
  3. merge      five levels (2000, 2000, 2000, 2000, 819) with ties across levels and the cut, a level with nothing kept;
  4. selection  stage by stage over a filtered wide, a direct wide and a narrow level; the narrow level's outputs equal the narrow calls';
  5. RPN        in training mode with PRE_NMS_TOPK_TRAIN 2000 / POST_NMS_TOPK_TRAIN 1000: (proposals, losses), deterministic, poisoned workspaces;
  6. detector   five finite losses whose sum reaches every trainable parameter, with those RPN values."""
import functools
import math

import numpy as np
import pytest
import torch

import rpn_f64 as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


def _pm(x):
    """CPU NCHW -> GPU tensor whose memory is [N][H][W][C], with those strides spelled out"""
    N, C_, H, W = x.shape
    flat = x.permute(0, 2, 3, 1).reshape(-1).cuda()
    return flat.as_strided((N, C_, H, W), (H * W * C_, 1, W * C_, C_))


def _flat(x):
    """[C, H, W] logits -> anchor order (y W + x) A + a"""
    return x.permute(1, 2, 0).reshape(-1)


# ------------------------------------------------------------------------------------------------ 1. top-k
def _logit_case(kind, N, A, H, W, seed):
    """the logit kinds of tests/test_gpu_rpn.py's TOPK_CASES"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, A, H, W), generator=g)
    if kind == "ties":                                     # 64 distinct values: ties span the cut
        x = torch.round(x * 8).clamp(-32, 31) / 8
    elif kind == "equal":
        x = torch.full((N, A, H, W), 0.25)
    elif kind == "nan":
        f = x.view(-1)
        f[torch.randperm(f.numel(), generator=g)[:max(3, f.numel() // 50)]] = float("nan")
    elif kind == "zeros":                                  # -0 and +0 compare equal: index order decides
        x = torch.where(torch.rand((N, A, H, W), generator=g) < 0.5, torch.zeros(()), -torch.zeros(()))
        x.view(-1)[::7] = 1.0
    return x


TOPK_WIDE_CASES = [  # kind, N, A, H, W, k, Cpad
    # direct read (H W A <= 16384)
    ("rand", 2, 3, 40, 40, 1025, 16), ("rand", 2, 3, 40, 40, 4096, 16), ("ties", 2, 3, 40, 40, 2000, 16), ("nan", 2, 3, 40, 40, 4096, 16),
    ("rand", 2, 3, 37, 37, 4096, 16), ("ties", 2, 3, 37, 37, 4096, 16),                       # n = 4107: almost the whole map
    ("rand", 2, 4, 32, 32, 4096, 16), ("nan", 2, 4, 32, 32, 4096, 16), ("equal", 2, 4, 32, 32, 4096, 16),     # k = n: everything, sorted
    ("zeros", 2, 3, 40, 40, 2049, 16), ("equal", 2, 3, 40, 40, 2048, 16),
    ("rand", 2, 2, 32, 32, 2048, 8),                                                          # k = n = 2048: the 2048-sort without padding
    # through the grid histogram and the filter (n = 23 040)
    ("rand", 2, 3, 80, 96, 2000, 16), ("rand", 2, 3, 80, 96, 4096, 16), ("ties", 2, 3, 80, 96, 2000, 16), ("ties", 2, 3, 80, 96, 4096, 16),
    ("equal", 2, 3, 80, 96, 4096, 16), ("zeros", 2, 3, 80, 96, 2000, 16), ("nan", 2, 3, 80, 96, 4096, 16),
]


@pytest.mark.parametrize("kind,N,A,H,W,k,Cpad", TOPK_WIDE_CASES)
def test_wide_topk_is_the_stable_descending_sort(amd, kind, N, A, H, W, k, Cpad):
    x = _logit_case(kind, N, A, H, W, seed=H * W + A)
    head = torch.full((N, Cpad, H, W), float("nan"))        # the other channels of the head output must not matter
    head[:, :A] = x
    hg = _pm(head)
    vals, idx = amd.ops.rpn_topk_wide(hg, A, k)
    torch.cuda.synchronize()
    vals, idx = vals.cpu().numpy(), idx.cpu().numpy()
    for n in range(N):
        flat = _flat(x[n]).numpy()
        want = R.topk(flat, k)
        assert idx[n].min() >= 0 and idx[n].max() < flat.size
        assert np.array_equal(idx[n], want), (kind, n, np.nonzero(idx[n] != want)[0][:5])
        assert np.array_equal(vals[n], flat[want], equal_nan=True)
    # into column slices of a wider buffer (the layout the levels of an image share), neighbours untouched
    wide_v = torch.full((N, k + 9), -7.0, device="cuda")
    wide_i = torch.full((N, k + 9), -7, device="cuda", dtype=torch.int32)
    amd.ops.rpn_topk_wide(hg, A, k, wide_v[:, 4:4 + k], wide_i[:, 4:4 + k])
    assert np.array_equal(wide_i[:, 4:4 + k].cpu().numpy(), idx) and bool((wide_i[:, :4] == -7).all()) and bool((wide_i[:, 4 + k:] == -7).all())
    assert bool((wide_v[:, :4] == -7).all()) and bool((wide_v[:, 4 + k:] == -7).all())


def test_wide_topk_refusals_and_the_narrow_limit_stays(amd):
    hg = _pm(torch.zeros(1, 16, 40, 40))
    for A, k in ((3, 4097), (3, 1024), (3, 0), (17, 2000)):   # k <= 1024 is rpn_topk's
        with pytest.raises(amd.AfiError):
            amd.ops.rpn_topk_wide(hg, A, k)
    with pytest.raises(amd.AfiError):
        amd.ops.rpn_topk_wide(_pm(torch.zeros(1, 4, 20, 20)), 3, 1201)    # k above H W A = 1200
    with pytest.raises(amd.AfiError):
        amd.ops.rpn_topk(hg, 3, 1025)                                     # the narrow op keeps its limit


# ------------------------------------------------------------------------------------------------ 2. NMS
# seeds per (n, threshold), two for a batch of 2: found on the CPU with rpn_f64.nms_case_facts (no pair within 1e-5, every box non-empty).  At 4096
# most seeds have a few such pairs at 0.5 and none found serves both thresholds, so the seeds are chosen per threshold there.
NMS_WIDE_SEEDS = {
    (4096, 0.7): (0, 5), (4096, 0.5): (49, 59),
    (4033, 0.7): (28, 64), (4033, 0.5): (28, 64),
    (2000, 0.7): (0, 1), (2000, 0.5): (0, 1),
    (1025, 0.7): (0, 2), (1025, 0.5): (0, 2),
    (65, 0.7): (0, 1), (65, 0.5): (0, 1),
}


@functools.lru_cache(maxsize=None)
def nms_fixture(seed, n, thresh):
    """(boxes fp32 [n, 4], all non-empty, pairs whose fp64 IoU is within 1e-5 of thresh, the fp64 greedy keep set): computed once per process and
    shared by the tests here and in tests/test_rpn_wide_host.py, which also holds the three facts to rpn_f64.nms_case_facts."""
    b, _ = R.nms_case(seed, n)
    b64 = b.astype(np.float64)
    nonempty = bool((((b64[:, 2] - b64[:, 0]) > 0) & ((b64[:, 3] - b64[:, 1]) > 0)).all())
    near = np.abs(R.iou_matrix(b64) - thresh) < 1e-5
    ambiguous = int(np.triu(near, 1).sum())
    want = R.nms(b64, np.ones(n, bool), thresh)
    return b, nonempty, ambiguous, want


def _nms_batch(n, thresh):
    cases = [nms_fixture(seed, n, thresh) for seed in NMS_WIDE_SEEDS[(n, thresh)]]
    for b, nonempty, ambiguous, want in cases:              # the conditions, before any launch
        assert nonempty and ambiguous == 0 and 0.1 <= want.mean() <= 0.9, (n, thresh, nonempty, ambiguous, want.mean())
    boxes = torch.tensor(np.stack([c[0] for c in cases]), dtype=torch.float32).cuda()
    return cases, boxes


@pytest.mark.parametrize("thresh", R.NMS_THRESHOLDS)
@pytest.mark.parametrize("n", [4096, 4033, 2000, 1025, 65])
def test_wide_nms_keep_set_is_exact(amd, n, thresh, monkeypatch):
    cases, boxes = _nms_batch(n, thresh)
    valid = torch.ones((2, n), dtype=torch.int32, device="cuda")
    keep = amd.ops.rpn_nms_wide(boxes, valid, thresh)
    torch.cuda.synchronize()
    assert tuple(keep.shape) == (2, n)
    for i, c in enumerate(cases):
        got = keep[i].cpu().numpy()
        assert set(np.unique(got)) <= {0, 1} and np.array_equal(got != 0, c[3]), (n, thresh, i, np.nonzero((got != 0) != c[3])[0][:5])
    monkeypatch.setattr(amd.ops, "_POISON", True)           # a NaN-filled workspace: only words the build wrote may be read
    assert torch.equal(amd.ops.rpn_nms_wide(boxes, valid, thresh), keep)


@pytest.mark.parametrize("n,thresh", [(2000, 0.7), (1025, 0.5), (65, 0.7)])
def test_wide_nms_invalid_boxes_and_a_wider_buffer(amd, n, thresh):
    cases, boxes = _nms_batch(n, thresh)
    valid = torch.ones((2, n), dtype=torch.int32, device="cuda")
    valid[:, ::7] = 0                                       # invalid boxes are skipped and suppress nothing
    keep = amd.ops.rpn_nms_wide(boxes, valid, thresh).cpu().numpy()
    vh = valid.cpu().numpy() != 0
    for i, c in enumerate(cases):
        assert np.array_equal(keep[i] != 0, R.nms(c[0].astype(np.float64), vh[i], thresh)) and not (keep[i] != 0)[~vh[i]].any()
    # ld > k: column slices of wider buffers whose neighbours keep a sentinel
    wb = torch.full((2, n + 9, 4), -7.0, device="cuda")
    wv = torch.full((2, n + 9), -7, device="cuda", dtype=torch.int32)
    wk = torch.full((2, n + 9), -7, device="cuda", dtype=torch.int32)
    wb[:, 5:5 + n], wv[:, 5:5 + n] = boxes, valid
    amd.ops.rpn_nms_wide(wb[:, 5:5 + n], wv[:, 5:5 + n], thresh, wk[:, 5:5 + n])
    assert np.array_equal(wk[:, 5:5 + n].cpu().numpy(), keep) and bool((wk[:, :5] == -7).all()) and bool((wk[:, 5 + n:] == -7).all())


def test_wide_nms_of_one_box_and_of_none(amd):
    b = torch.tensor([[[1.0, 2.0, 30.0, 40.0]], [[0.0, 0.0, 5.0, 5.0]]], device="cuda")
    v = torch.tensor([[1], [0]], dtype=torch.int32, device="cuda")
    assert amd.ops.rpn_nms_wide(b, v, 0.7).cpu().tolist() == [[1], [0]]
    keep = amd.ops.rpn_nms_wide(torch.zeros((2, 0, 4), device="cuda"), torch.zeros((2, 0), dtype=torch.int32, device="cuda"), 0.7)
    assert tuple(keep.shape) == (2, 0)
    with pytest.raises(amd.AfiError, match="4096"):
        amd.ops.rpn_nms_wide(torch.zeros((1, 4097, 4), device="cuda"), torch.ones((1, 4097), dtype=torch.int32, device="cuda"), 0.7)


@pytest.mark.parametrize("thresh", R.NMS_THRESHOLDS)
@pytest.mark.parametrize("n", [1000, 333, 64])
def test_wide_nms_equals_the_narrow_kernel_on_its_lists(amd, n, thresh):
    """tests/test_gpu_rpn.py's own lists (R.NMS_SIZES / R.NMS_SEEDS), all valid and with every fifth box invalid: the same keep array, bit for bit."""
    boxes = torch.tensor(np.stack([R.nms_case(seed, n)[0] for seed in R.NMS_SEEDS]), dtype=torch.float32).cuda()
    valid = torch.ones((2, n), dtype=torch.int32, device="cuda")
    for _ in range(2):
        assert torch.equal(amd.ops.rpn_nms_wide(boxes, valid, thresh), amd.ops.rpn_nms(boxes, valid, thresh))
        valid[:, ::5] = 0


# ------------------------------------------------------------------------------------------------ 3. merge
REF_LEVELS = [0, 2000, 4000, 6000, 8000, 8819]             # the reference at 800 x 1344 with PRE_NMS_TOPK_TRAIN 2000: p6 has 13 x 21 x 3 = 819 anchors


def _check_merge(amd, vals, keep, boxes, off, post_k):
    ob, ol, counts = amd.ops.rpn_merge_wide(boxes.cuda(), vals.cuda(), keep.cuda(), off, post_k)
    torch.cuda.synchronize()
    assert tuple(ob.shape) == (vals.shape[0], post_k, 4)
    for n in range(vals.shape[0]):
        order = R.merge(vals[n].numpy(), keep[n].numpy() != 0, off, post_k)
        c = len(order)
        assert int(counts[n]) == c == min(int((keep[n] != 0).sum()), post_k)
        assert np.array_equal(ol[n, :c].cpu().numpy(), vals[n].numpy()[order]) and np.array_equal(ob[n, :c].cpu().numpy(), boxes[n].numpy()[order])
        assert not ob[n, c:].any() and not ol[n, c:].any()
    return counts.cpu().tolist()


def _merge_inputs(off, seed, quant=4):
    g = torch.Generator().manual_seed(seed)
    N, K = 2, off[-1]
    vals = torch.empty((N, K))
    for l in range(len(off) - 1):
        v = torch.round(torch.randn((N, off[l + 1] - off[l]), generator=g) * quant) / quant       # quantised: ties across levels and at the cut
        vals[:, off[l]:off[l + 1]] = torch.sort(v, dim=1, descending=True).values
    keep = (torch.rand((N, K), generator=g) < 0.6).to(torch.int32)
    return vals, keep, torch.rand((N, K, 4), generator=g)


@pytest.mark.parametrize("post_k", [1000, 2000])
def test_wide_merge_of_the_references_five_levels(amd, post_k):
    vals, keep, boxes = _merge_inputs(REF_LEVELS, 3)
    assert _check_merge(amd, vals, keep, boxes, REF_LEVELS, post_k) == [post_k, post_k]
    cut = np.sort(vals[0].numpy()[keep[0].numpy() != 0])[::-1]
    assert cut[post_k - 1] == cut[post_k], "no tie at the cut"
    keep[:, 2000:4000] = 0                                   # a level with nothing kept
    keep[1, 4000:] = 0                                       # and an image with fewer than post_k kept: rows past counts are zero
    assert _check_merge(amd, vals, keep, boxes, REF_LEVELS, post_k)[1] == min(int(keep[1].sum()), post_k)


def test_wide_merge_at_its_stated_total_and_with_short_levels(amd):
    off = [0, 4096, 8192, 12288, 16384, 20480]               # 5 x 4096: the total the kernel holds
    vals, keep, boxes = _merge_inputs(off, 4, quant=16)
    _check_merge(amd, vals, keep, boxes, off, 3000)
    off = [0, 1025, 1025, 1026, 3000, 3007, 3010]            # an empty level, levels of 1, 7 and 3, six levels
    vals, keep, boxes = _merge_inputs(off, 5)
    for post_k in (137, 5000):
        _check_merge(amd, vals, keep, boxes, off, post_k)
    with pytest.raises(amd.AfiError, match="20480"):
        amd.ops.rpn_merge_wide(torch.zeros((1, 20481, 4), device="cuda"), torch.zeros((1, 20481), device="cuda"),
                               torch.zeros((1, 20481), dtype=torch.int32, device="cuda"), [0, 4096, 8192, 12288, 16384, 20480, 20481], 10)


# ------------------------------------------------------------------------------------------------ 4. the whole selection
LEVELS3 = ["p3", "p4", "p5"]


class _Imgs:
    def __init__(self, sizes):
        self.image_sizes = sizes

    def __len__(self):
        return len(self.image_sizes)


class _GT:
    def __init__(self, boxes):
        self.gt_boxes = boxes


def _rpn(amd, channels, sizes, seed=0, features=LEVELS3, **keys):
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[s] for s in sizes], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": list(features), "PRE_NMS_TOPK_TEST": 1000, "POST_NMS_TOPK_TEST": 1000, "PRE_NMS_TOPK_TRAIN": 2000,
                                       "POST_NMS_TOPK_TRAIN": 1000, "BATCH_SIZE_PER_IMAGE": 32, **keys}})
    m = amd.RPN(cfg, {f: ShapeSpec(channels=channels, stride=2 ** int(f[1:])) for f in features})
    g = torch.Generator().manual_seed(seed)
    std = {"conv": (1.0 / math.sqrt(9 * channels)), "objectness_logits": 1.0 / math.sqrt(channels), "anchor_deltas": 0.6 / math.sqrt(channels)}
    with torch.no_grad():
        for name, s in std.items():
            layer = getattr(m.rpn_head, name)
            layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * s)
            layer.bias.copy_(torch.randn(layer.bias.shape, generator=g) * 0.1)
    return m.cuda()


def _check_selection(m, r, sizes, heads, post_k):
    """tests/test_gpu_rpn.py's scheme: the checker run stage by stage on the kernels' own intermediates, the decode left to that file (its kernel
    is the same for every list length: here its boxes must only be the ones the validity flags and the NMS were computed from)."""
    A, off = m.num_anchors, r["level_off"]
    N = r["vals"].shape[0]
    vals, idx, lb, valid, keep = (r[k].cpu().numpy() for k in ("vals", "idx", "level_boxes", "valid", "keep"))
    ob, ol, counts = r["boxes"].cpu().numpy(), r["logits"].cpu().numpy(), r["counts"].cpu().numpy()
    EPS = 2.0 ** -24
    for n in range(N):
        for l, hd in enumerate(heads):
            s = slice(off[l], off[l + 1])
            k = off[l + 1] - off[l]
            H, W = hd.shape[2:]
            h = hd[n].cpu()
            flat = _flat(h[:A]).numpy()
            want = R.topk(flat, k)
            assert np.array_equal(idx[n, s], want) and np.array_equal(vals[n, s], flat[want])
            dn = h[A:5 * A].reshape(A, 4, H, W).permute(2, 3, 0, 1).reshape(-1, 4)[torch.tensor(idx[n, s]).long()].numpy()
            cell = m.anchor_generator.cell_anchors[l].cpu().double().numpy()
            ref, v, (pcx, pcy, pw, ph) = R.decode(dn, idx[n, s], cell, m.anchor_generator.strides[l], W, A, m.box_weights, sizes[n], m.min_box_side_len)
            bound = 16 * EPS * np.stack([np.abs(pcx) + pw, np.abs(pcy) + ph, np.abs(pcx) + pw, np.abs(pcy) + ph], 1)      # test_gpu_rpn.py's, derived there
            assert (np.abs(lb[n, s] - ref) <= bound).all()
            b32 = lb[n, s]
            v = ((b32[:, 2] - b32[:, 0]) > np.float32(m.min_box_side_len)) & ((b32[:, 3] - b32[:, 1]) > np.float32(m.min_box_side_len))
            assert np.array_equal(valid[n, s] != 0, v)
            assert np.array_equal(keep[n, s] != 0, R.nms(b32.astype(np.float64), v, m.nms_thresh, rounding_pairs_in_fp32=True))
        order = R.merge(vals[n], keep[n] != 0, off, post_k)
        c = len(order)
        assert counts[n] == c == min(int((keep[n] != 0).sum()), post_k)
        assert np.array_equal(ob[n, :c], lb[n][order]) and np.array_equal(ol[n, :c], vals[n][order])
        assert not ob[n, c:].any() and not ol[n, c:].any()
        assert np.all(np.diff(ol[n, :c]) <= 0)
        ties = np.nonzero(np.diff(ol[n, :c]) == 0)[0]
        assert np.all(order[ties] < order[ties + 1])
    return counts


SEL_SHAPES = [(80, 96), (40, 48), (10, 12)]                # 23 040 (filtered, wide), 5760 (direct, wide), 360 entries (narrow)
SEL_SIZES = [(640, 768), (611, 739)]


TRAIN_LEVELS = ["p2", "p3", "p4"]
TRAIN_SHAPES = [(80, 96), (40, 48), (20, 24)]              # a 320 x 384 batch at strides 4, 8, 16: 23 040, 5760 and 1440 entries, all wide at 2000


def _selection_inputs(amd, seed=1, features=LEVELS3, shapes=SEL_SHAPES):
    m = _rpn(amd, 16, (32, 64, 128), seed=seed, features=features)
    g = torch.Generator().manual_seed(seed + 1)
    feats = {f: _pm(torch.randn((2, 16, h, w), generator=g)) for f, (h, w) in zip(features, shapes)}
    return m, feats


def test_wide_selection_stage_by_stage(amd):
    m, feats = _selection_inputs(amd)
    m.eval()
    hw = torch.tensor(SEL_SIZES, dtype=torch.float32, device="cuda")
    ops = amd.ops
    with torch.no_grad():
        heads = m.head(feats)
        r = m.select(heads, hw, 2000, 1000)
        torch.cuda.synchronize()
        assert r["level_off"] == [0, 2000, 4000, 4360]
        counts = _check_selection(m, r, SEL_SIZES, heads, 1000)
        assert counts.max() <= 1000 and counts.min() > 0
        # the narrow level ran the kernels it runs today: the same bits as those calls made directly
        s, A, ag = slice(4000, 4360), m.num_anchors, m.anchor_generator
        v, i = ops.rpn_topk(heads[2], A, 360)
        b, vd = ops.rpn_decode(heads[2], A, A, ag.cell_anchors[2], ag.strides[2], i, 360, hw, m.box_weights, R.SCALE_CLAMP, m.min_box_side_len)
        kp = ops.rpn_nms(b, vd, m.nms_thresh)
        assert torch.equal(r["vals"][:, s], v) and torch.equal(r["idx"][:, s], i) and torch.equal(r["keep"][:, s], kp)
        assert torch.equal(r["level_boxes"][:, s], b) and torch.equal(r["valid"][:, s], vd)
        # and a selection without a wide level is today's, merge included
        r2 = m.select(heads, hw, 360, 300)
        ob, ol, cn = ops.rpn_merge(r2["level_boxes"], r2["vals"], r2["keep"], r2["level_off"], 300)
        assert r2["level_off"] == [0, 360, 720, 1080] and torch.equal(r2["boxes"], ob) and torch.equal(r2["logits"], ol) and torch.equal(r2["counts"], cn)


# ------------------------------------------------------------------------------------------------ 5. the RPN in training mode
def test_rpn_training_forward_with_the_references_values(amd, monkeypatch):
    m, feats = _selection_inputs(amd, seed=3, features=TRAIN_LEVELS, shapes=TRAIN_SHAPES)
    m.trainable_(True).train()
    assert (m.pre_nms_topk_train, m.post_nms_topk_train) == (2000, 1000)
    sizes = [(320, 384), (301, 377)]                        # the image pair inside its 320 x 384 batch
    gts = [_GT(torch.tensor([[20.0, 30.0, 200.0, 180.0], [150.0, 100.0, 380.0, 300.0], [5.0, 200.0, 90.0, 310.0]]).cuda()),
           _GT(torch.tensor([[40.0, 40.0, 300.0, 280.0], [200.0, 10.0, 370.0, 120.0]]).cuda())]
    R_ = sum(h * w * 3 for h, w in TRAIN_SHAPES)
    keys = torch.randint(-2 ** 31, 2 ** 31, (2, R_), generator=torch.Generator().manual_seed(9), dtype=torch.int64).to(torch.int32).cuda()
    imgs = _Imgs(sizes)

    def run():
        props, losses = m(imgs, feats, gts, keys=keys)
        torch.cuda.synchronize()
        return props, losses
    props, losses = run()
    alone = m.losses(imgs, feats, gts, keys)
    assert set(losses) == {"loss_rpn_cls", "loss_rpn_loc"} and all(torch.equal(losses[k], alone[k]) for k in losses)
    assert losses["loss_rpn_cls"].requires_grad and all(bool(torch.isfinite(v)) for v in losses.values())
    # the proposals: the staged checker's, on the same head outputs
    with torch.no_grad():
        heads = m.eval().head(feats)
        m.train()
        r = m.select(heads, torch.tensor(sizes, dtype=torch.float32, device="cuda"), 2000, 1000)
    assert r["level_off"] == [0, 2000, 4000, 5440]
    counts = _check_selection(m, r, sizes, heads, 1000)
    assert len(props) == 2
    for n, p in enumerate(props):
        c, t, lg = int(counts[n]), p.proposal_boxes.tensor, p.objectness_logits
        assert tuple(p.image_size) == sizes[n] and 0 < len(p) == c <= 1000 and not t.requires_grad
        assert torch.equal(t, r["boxes"][n, :c]) and torch.equal(lg, r["logits"][n, :c])
        assert bool((lg[1:] <= lg[:-1]).all())
        assert bool((t >= 0).all()) and bool((t[:, 0::2] <= sizes[n][1]).all()) and bool((t[:, 1::2] <= sizes[n][0]).all())
    # two runs bit-identical, and again with NaN-poisoned workspaces and fresh outputs
    again = [run()]
    monkeypatch.setattr(amd.ops, "_POISON", True)
    again.append(run())
    for p2, l2 in again:
        assert all(torch.equal(losses[k], l2[k]) for k in losses)
        assert all(torch.equal(a.proposal_boxes.tensor, b.proposal_boxes.tensor) and torch.equal(a.objectness_logits, b.objectness_logits)
                   for a, b in zip(props, p2))


# ------------------------------------------------------------------------------------------------ 6. under the detector
def test_detector_trains_with_the_references_rpn_values(amd):
    """tests/test_gpu_resnet_train.py's detector (FPN_AFIGAN over the small trainable ResNet, trainable RPN, box + mask heads) with
    PRE_NMS_TOPK_TRAIN 2000 / POST_NMS_TOPK_TRAIN 1000, at 96 x 128 so that p2 (24 x 32 x 3 = 2304 anchors) is a wide level."""
    import mask_loss_f64 as Q
    import resnet_train_f64 as RT
    features = ["p2", "p3", "p4", "p5"]
    net, freeze_at, _ = RT.make_net("small")
    backbone = amd.FPN_AFIGAN(bottom_up=net.trainable_(freeze_at), in_features=["res2", "res3", "res4", "res5"], out_channels=16, norm="",
                              top_block=amd.LastLevelMaxPool(), fuse_type="sum").cuda()
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[16], [32], [64], [128]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": features, "PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 50, "PRE_NMS_TOPK_TRAIN": 2000,
                                       "POST_NMS_TOPK_TRAIN": 1000, "BATCH_SIZE_PER_IMAGE": 32}})
    rpn = amd.RPN(cfg, {f: backbone.output_shape()[f] for f in features}).cuda().trainable_()
    heads = Q.e2e_heads(amd, 16).cuda().trainable_(mask_head=True)
    model = amd.GeneralizedRCNN_AFExtractor(backbone=backbone, proposal_generator=rpn, roi_heads=heads, pixel_mean=[0.0, 0.0, 0.0],
                                            pixel_std=[1.0, 1.0, 1.0], device="cuda").train()
    ih, iw = 96, 128
    gts = [np.array([[4, 6, 60, 80], [50, 20, 120, 90], [10, 30, 40, 64]], np.float32), np.array([[8, 8, 100, 60], [60, 34, 110, 92]], np.float32)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g = torch.Generator().manual_seed(4)
    batch = []
    for b in gts:
        polys = [[Q._ngon((x0 + x1) / 2, (y0 + y1) / 2, 0.45 * (x1 - x0), 0.45 * (y1 - y0), 9)] for x0, y0, x1, y1 in b.astype(np.float64)]
        tg = type("GT", (), {})()
        tg.gt_boxes, tg.gt_classes = dev(b), dev(np.arange(len(b), dtype=np.int64) % 5)
        tg.gt_masks = type("PolygonMasks", (), {"polygons": polys})()
        batch.append({"image_x0.5": torch.randn((3, ih, iw), generator=g), "targets": tg})
    seen = {}
    select = rpn.select
    rpn.select = lambda *a, **k: seen.setdefault("r", select(*a, **k))
    losses, _ = model(batch)
    assert seen["r"]["level_off"][:2] == [0, 2000], "p2 did not run as a wide level"
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_mask", "loss_rpn_cls", "loss_rpn_loc"}
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for k, p in list(net.named_parameters()) + list(rpn.named_parameters()) + list(heads.named_parameters()):
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0), k
        else:
            assert p.grad is None, k
