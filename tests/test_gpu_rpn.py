"""The frozen RPN proposal generator on the GPU (afigan_amd/rpn.py, csrc/rpn.hip) against tests/rpn_f64.py, staged so that each stage's
checker consumes the KERNEL's previous stage output -- no rounding difference leaks into a discrete decision:
  1. top-k      exact: indices and values equal a stable descending sort of the same fp32 logits (ties in ascending anchor index, NaN last);
  2. decode     per coordinate |err| <= 16 * 2^-24 * (|pcx| + pw) against the fp64 formula on the same fp32 deltas and indices -- about eight
                fp32 operations and one expf, each within an ulp or two of values no larger than |pcx| + pw: derived, not measured (the
                measured maximum is printed beside it) -- and the validity flags equal;
  3. NMS        exact keep set on inputs that the test first holds to two conditions (no pair's fp64 IoU within 1e-5 of the threshold,
                10 % .. 90 % kept; tests/test_rpn_host.py checks the same inputs without a GPU);
  4. selection  the padded result equals the checker run stage by stage on the kernels' own intermediates; forward() = forward_padded();
  5. head       logits and deltas against fp64 at test_gpu_pixgemm.py's bars (max-norm 2 sqrt(Ktot) 2^-24 with its caps, rel. L2 4x the larger
                of CPU fp32's error and sqrt(Ktot) 2^-24 / 8), Ktot = 9 C + C: the two reductions an output passes through, whose rounding
                errors add in variance.  CPU fp32's error printed beside; no torch / MIOpen / hipBLASLt kernel in the trace.  Measured on
                MI355X, C = 256 at 50 x 84 (Winograd F(4x4), f16x3 arithmetic): rel. L2 1.47e-6 of a 1.51e-6 bar -- Ktot = 9 C alone would put
                the bar at 1.43e-6, which that case misses by 2.6 %; every direct-conv case sits below 3.7e-7;
  6. full size  properties that tolerate a box moving across the top-k cut, checked in fp64 on the kernels' output and intermediates; two eager
                runs and a hipGraph replay bit-identical;
  7. the detector's inference() with this RPN and a stand-in for the ROI heads."""
import math

import numpy as np
import pytest
import torch

import rpn_f64 as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


def _pm(x):
    """CPU NCHW -> GPU tensor whose memory is [N][H][W][C], with those strides spelled out (torch leaves the strides of size-1 dimensions open)"""
    N, C_, H, W = x.shape
    flat = x.permute(0, 2, 3, 1).reshape(-1).cuda()
    return flat.as_strided((N, C_, H, W), (H * W * C_, 1, W * C_, C_))


def _flat(x):
    """[C, H, W] logits -> anchor order (y W + x) A + a"""
    return x.permute(1, 2, 0).reshape(-1)


# ------------------------------------------------------------------------------------------------ 1. top-k
def _logit_case(kind, N, A, H, W, seed):
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


TOPK_CASES = [  # kind, N, A, H, W, k, Cpad
    ("rand", 2, 3, 200, 336, 1000, 16), ("ties", 2, 3, 200, 336, 1000, 16), ("equal", 1, 3, 200, 336, 1000, 16), ("nan", 2, 3, 100, 168, 1000, 16),
    ("rand", 2, 3, 13, 21, 819, 16), ("ties", 2, 3, 13, 21, 500, 16), ("nan", 2, 3, 13, 21, 819, 16), ("nan", 1, 1, 5, 4, 20, 8),
    ("rand", 1, 3, 1, 1, 3, 16), ("rand", 2, 1, 1, 1, 1, 8), ("rand", 2, 3, 7, 9, 189, 16),       # H W A < PRE_NMS_TOPK: all of them, sorted
    ("rand", 2, 1, 50, 84, 1000, 8), ("ties", 2, 1, 200, 336, 1024, 8), ("zeros", 2, 3, 25, 42, 700, 16), ("equal", 2, 3, 50, 84, 1000, 16),
    ("rand", 2, 16, 40, 40, 1000, 80),
    ("rand", 2, 4, 16, 16, 1024, 8), ("nan", 2, 4, 16, 16, 1023, 8),       # k = n = 1024: the sort is full, no padding word; and one short of it
    ("ties", 2, 1, 200, 336, 1, 8),                                        # k = 1 through the filter
]


@pytest.mark.parametrize("kind,N,A,H,W,k,Cpad", TOPK_CASES)
def test_topk_is_the_stable_descending_sort(amd, kind, N, A, H, W, k, Cpad):
    x = _logit_case(kind, N, A, H, W, seed=H * W + A)
    head = torch.full((N, Cpad, H, W), float("nan"))        # the other channels of the head output must not matter
    head[:, :A] = x
    hg = _pm(head)
    assert hg.stride(3) == Cpad                              # a strided view: A of Cpad channels
    vals, idx = amd.ops.rpn_topk(hg, A, k)
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
    amd.ops.rpn_topk(hg, A, k, wide_v[:, 4:4 + k], wide_i[:, 4:4 + k])
    assert np.array_equal(wide_i[:, 4:4 + k].cpu().numpy(), idx) and bool((wide_i[:, :4] == -7).all()) and bool((wide_i[:, 4 + k:] == -7).all())
    assert bool((wide_v[:, :4] == -7).all()) and bool((wide_v[:, 4 + k:] == -7).all())


def test_topk_refuses_what_it_cannot_hold(amd):
    hg = _pm(torch.zeros(1, 16, 40, 40))
    for A, k in ((3, 1025), (3, 0), (17, 10)):
        with pytest.raises(amd.AfiError):
            amd.ops.rpn_topk(hg, A, k)
    with pytest.raises(amd.AfiError):
        amd.ops.rpn_topk(_pm(torch.zeros(1, 4, 2, 2)), 3, 13)           # k above H W A


# ------------------------------------------------------------------------------------------------ 2. decode
@pytest.mark.parametrize("min_size,weights", [(0.0, (1.0, 1.0, 1.0, 1.0)), (4.0, (1.0, 1.0, 1.0, 1.0)), (0.0, (10.0, 10.0, 5.0, 5.0))])
def test_decode_against_fp64(amd, min_size, weights):
    N, A, H, W, stride, k = 2, 3, 50, 84, 16, 1000
    g = torch.Generator().manual_seed(5)
    head = torch.randn((N, 16, H, W), generator=g)
    d = head[:, A:5 * A]
    d[:, 0::4] *= 1.5                                       # dx, dy: centres leave the image on every side
    d[:, 1::4] *= 1.5
    d[:, 2::4] = d[:, 2::4] * 2.5 - 1.0                     # dw, dh from tiny boxes up to 10: the clamp is hit
    d[:, 3::4] = d[:, 3::4] * 2.5 - 1.0
    big = torch.zeros((N, A, H, W), dtype=torch.bool)
    big.view(-1)[::97] = True
    d[:, 2::4][big] = 10.0
    d[:, 3::4][big.flip(3)] = 10.0
    d *= torch.tensor(weights).repeat(A).view(1, 4 * A, 1, 1)
    hg = _pm(head)
    cell = R.cell_anchors([128], [0.5, 1.0, 2.0])
    cell32 = torch.tensor(cell, dtype=torch.float32)
    sizes = [(800, 1344), (731, 1203)]
    hw = torch.tensor(sizes, dtype=torch.float32, device="cuda")
    idx = torch.stack([torch.randperm(H * W * A, generator=g)[:k] for _ in range(N)]).to(torch.int32)
    boxes, valid = amd.ops.rpn_decode(hg, A, A, cell32.cuda(), stride, idx.cuda(), k, hw, weights, R.SCALE_CLAMP, min_size)
    torch.cuda.synchronize()
    boxes, valid = boxes.cpu().double().numpy(), valid.cpu().numpy()
    worst, clamped, clipped, dropped = 0.0, 0, np.zeros(4, int), 0
    for n in range(N):
        dn = d[n].reshape(A, 4, H, W).permute(2, 3, 0, 1).reshape(-1, 4)[idx[n].long()].numpy()
        ref, v, (pcx, pcy, pw, ph) = R.decode(dn, idx[n].numpy(), cell32.double().numpy(), stride, W, A, weights, sizes[n], min_size)
        bound = 16 * EPS * np.stack([np.abs(pcx) + pw, np.abs(pcy) + ph, np.abs(pcx) + pw, np.abs(pcy) + ph], 1)
        err = np.abs(boxes[n] - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"decode error {err.max():.3e}, worst err / bound {float((err / bound).max()):.3f}"
        # the flags: the size test on the kernel's own stored fp32 boxes, exactly -- and equal to the fp64 checker's
        b32 = boxes[n].astype(np.float32)
        assert np.array_equal(valid[n] != 0, ((b32[:, 2] - b32[:, 0]) > np.float32(min_size)) & ((b32[:, 3] - b32[:, 1]) > np.float32(min_size)))
        assert np.array_equal(valid[n] != 0, v), np.nonzero((valid[n] != 0) != v)[0]
        clamped += int((dn[:, 2] / weights[2] > R.SCALE_CLAMP).sum() + (dn[:, 3] / weights[3] > R.SCALE_CLAMP).sum())
        ih, iw = sizes[n]
        clipped += [(ref[:, 0] == 0).sum(), (ref[:, 1] == 0).sum(), (ref[:, 2] == iw).sum(), (ref[:, 3] == ih).sum()]
        dropped += int((~v).sum())
        assert boxes[n][:, 0::2].min() >= 0 and boxes[n][:, 0::2].max() <= iw and boxes[n][:, 1::2].min() >= 0 and boxes[n][:, 1::2].max() <= ih
    print(f"[rpn decode] min_size {min_size} weights {weights}: worst |err| / (16 eps (|pc| + p)) = {worst:.3f}; clamped {clamped}, "
          f"clipped (x1, y1, x2, y2) {clipped.tolist()}, dropped {dropped}")
    assert clamped > 0 and (clipped > 0).all() and dropped > 0
    # an index outside the map: a zero box, flagged invalid -- never a fault
    bad = torch.tensor([[-1, H * W * A, 2 ** 30, 0]] * N, dtype=torch.int32, device="cuda")
    b2, v2 = amd.ops.rpn_decode(hg, A, A, cell32.cuda(), stride, bad, 4, hw, weights, R.SCALE_CLAMP, min_size)
    assert bool((b2[:, :3] == 0).all()) and bool((v2[:, :3] == 0).all())


# ------------------------------------------------------------------------------------------------ 3. NMS
@pytest.mark.parametrize("thresh", R.NMS_THRESHOLDS)
@pytest.mark.parametrize("n", R.NMS_SIZES)
def test_nms_keep_set_is_exact(amd, n, thresh):
    cases = [R.nms_case(seed, n) for seed in R.NMS_SEEDS]
    for b, _ in cases:                                      # the two input conditions, before any launch
        if n > 1:
            nonempty, ambiguous, kept = R.nms_case_facts(b, thresh)
            assert nonempty and ambiguous == 0 and 0.1 <= kept <= 0.9, (n, thresh, nonempty, ambiguous, kept)
    boxes = torch.tensor(np.stack([b for b, _ in cases]), dtype=torch.float32).reshape(len(cases), n, 4).cuda()
    valid = torch.ones((len(cases), n), dtype=torch.int32, device="cuda")
    keep = amd.ops.rpn_nms(boxes, valid, thresh)
    torch.cuda.synchronize()
    assert tuple(keep.shape) == (len(cases), n)
    for i, (b, _) in enumerate(cases):
        want = R.nms(b.astype(np.float64), np.ones(n, bool), thresh)
        assert np.array_equal(keep[i].cpu().numpy() != 0, want), (n, thresh, i)
    if n >= 64:                                             # invalid boxes are skipped and suppress nothing
        valid[:, ::5] = 0
        keep = amd.ops.rpn_nms(boxes, valid, thresh).cpu().numpy()
        for i, (b, _) in enumerate(cases):
            assert np.array_equal(keep[i] != 0, R.nms(b.astype(np.float64), valid[i].cpu().numpy() != 0, thresh))


# ------------------------------------------------------------------------------------------------ 4. the whole selection
LEVELS3 = ["p3", "p4", "p5"]


def _rpn(amd, features, channels, sizes, pre_k, post_k, min_size=0, seed=0, std=None, thresh=0.7):
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[s] for s in sizes], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": list(features), "PRE_NMS_TOPK_TEST": pre_k, "POST_NMS_TOPK_TEST": post_k, "NMS_THRESH": thresh},
                               "PROPOSAL_GENERATOR": {"MIN_SIZE": min_size}})
    strides = {f: 2 ** int(f[1:]) for f in features}
    m = amd.RPN(cfg, {f: ShapeSpec(channels=channels, stride=strides[f]) for f in features})
    g = torch.Generator().manual_seed(seed)
    std = std or {"conv": (1.0 / math.sqrt(9 * channels)), "objectness_logits": 1.0 / math.sqrt(channels), "anchor_deltas": 0.6 / math.sqrt(channels)}
    for name, s in std.items():
        layer = getattr(m.rpn_head, name)
        layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * s)
        layer.bias.copy_(torch.randn(layer.bias.shape, generator=g) * 0.1)
    return m.cuda().eval()


def _check_selection(m, r, sizes, heads):
    """The checker run stage by stage on the kernels' own intermediates: each stage's output must equal the checker's on the stage's input."""
    A, off = m.num_anchors, r["level_off"]
    N = r["vals"].shape[0]
    vals, idx, lb, valid, keep = (r[k].cpu().numpy() for k in ("vals", "idx", "level_boxes", "valid", "keep"))
    ob, ol, counts = r["boxes"].cpu().numpy(), r["logits"].cpu().numpy(), r["counts"].cpu().numpy()
    post_k = m.post_nms_topk
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
            bound = 16 * EPS * np.stack([np.abs(pcx) + pw, np.abs(pcy) + ph, np.abs(pcx) + pw, np.abs(pcy) + ph], 1)
            assert (np.abs(lb[n, s] - ref) <= bound).all()
            # validity and NMS: the checker on the KERNEL's boxes (these come out of kernels, so no seed can rule out a pair whose IoU is
            # within 1e-5 of the threshold: such a pair is decided by the fp32 statement of the formula, every other pair in fp64)
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
        # the stated tie rule: among equal logits, ascending concatenated position (level, then rank)
        ties = np.nonzero(np.diff(ol[n, :c]) == 0)[0]
        assert np.all(order[ties] < order[ties + 1])
    return counts


@pytest.mark.parametrize("min_size", [0, 6])
def test_selection_stage_by_stage(amd, min_size):
    m = _rpn(amd, LEVELS3, 32, (32, 64, 128), pre_k=200, post_k=300, min_size=min_size, seed=1)
    g = torch.Generator().manual_seed(2)
    shapes = [(25, 34), (13, 17), (7, 9)]
    feats = {f: _pm(torch.randn((2, 32, h, w), generator=g)) for f, (h, w) in zip(LEVELS3, shapes)}
    sizes = [(200, 272), (187, 251)]
    hw = torch.tensor(sizes, dtype=torch.float32, device="cuda")
    with torch.no_grad():
        heads = m.head(feats)
        r = m.forward_padded(hw, feats, intermediates=True)
        torch.cuda.synchronize()
        assert r["level_off"] == [0, 200, 400, 400 + 7 * 9 * 3]
        counts = _check_selection(m, r, sizes, heads)
        assert counts.max() <= 300 and counts.min() > 0
        # forward() = forward_padded(), one proposals object per image

        class Imgs:
            image_sizes = sizes

            def __len__(self):
                return 2
        props, losses = m(Imgs(), feats)
        b, lg, c = m.forward_padded(hw, feats)
    assert losses == {} and len(props) == 2
    for n, p in enumerate(props):
        assert tuple(p.image_size) == sizes[n] and len(p) == int(c[n])
        assert torch.equal(p.proposal_boxes.tensor, b[n, :int(c[n])]) and torch.equal(p.objectness_logits, lg[n, :int(c[n])])
        assert torch.equal(b[n], r["boxes"][n]) and torch.equal(lg[n], r["logits"][n])


def test_merge_ties_across_levels_and_the_cut(amd):
    """afi_rpn_merge alone: quantised logits, so equal values meet across levels and at the post_k cut."""
    g = torch.Generator().manual_seed(3)
    N, off = 2, [0, 1000, 1700, 1701, 2300]
    K = off[-1]
    vals = torch.empty((N, K))
    for l in range(4):
        v = torch.round(torch.randn((N, off[l + 1] - off[l]), generator=g) * 4) / 4
        vals[:, off[l]:off[l + 1]] = torch.sort(v, dim=1, descending=True).values
    keep = (torch.rand((N, K), generator=g) < 0.6).to(torch.int32)
    boxes = torch.rand((N, K, 4), generator=g)
    for post_k in (1000, 137, 3000):
        ob, ol, counts = amd.ops.rpn_merge(boxes.cuda(), vals.cuda(), keep.cuda(), off, post_k)
        torch.cuda.synchronize()
        for n in range(N):
            order = R.merge(vals[n].numpy(), keep[n].numpy() != 0, off, post_k)
            c = len(order)
            assert int(counts[n]) == c
            assert np.array_equal(ol[n, :c].cpu().numpy(), vals[n].numpy()[order]) and np.array_equal(ob[n, :c].cpu().numpy(), boxes[n].numpy()[order])
            assert not ob[n, c:].any() and not ol[n, c:].any()


def test_merge_at_its_bound_and_what_it_refuses(amd):
    """afi_rpn_merge with all it holds: eight levels of 1024, ties across levels and at the cut, one level with nothing kept."""
    g = torch.Generator().manual_seed(6)
    N, off = 2, [1024 * l for l in range(9)]
    K = off[-1]
    vals = torch.empty((N, K))
    for l in range(8):
        v = torch.round(torch.randn((N, 1024), generator=g) * 4) / 4
        vals[:, off[l]:off[l + 1]] = torch.sort(v, dim=1, descending=True).values
    keep = (torch.rand((N, K), generator=g) < 0.6).to(torch.int32)
    keep[:, off[5]:off[6]] = 0
    boxes = torch.rand((N, K, 4), generator=g)
    ob, ol, counts = amd.ops.rpn_merge(boxes.cuda(), vals.cuda(), keep.cuda(), off, 1000)
    torch.cuda.synchronize()
    for n in range(N):
        order = R.merge(vals[n].numpy(), keep[n].numpy() != 0, off, 1000)
        assert int(counts[n]) == len(order) == 1000
        assert np.array_equal(ol[n].cpu().numpy(), vals[n].numpy()[order]) and np.array_equal(ob[n].cpu().numpy(), boxes[n].numpy()[order])
        cut = np.sort(vals[n].numpy()[keep[n].numpy() != 0])[::-1]
        assert cut[999] == cut[1000], "no tie at the cut"

    def lists(K):
        return torch.zeros((1, K, 4), device="cuda"), torch.zeros((1, K), device="cuda"), torch.ones((1, K), dtype=torch.int32, device="cuda")
    with pytest.raises(amd.AfiError):
        amd.ops.rpn_merge(*lists(9), list(range(10)), 5)                # a ninth level
    with pytest.raises(amd.AfiError):
        amd.ops.rpn_merge(*lists(1025), [0, 1025], 5)                   # a level of 1025 is rpn_merge_wide's
    _, _, c = amd.ops.rpn_merge_wide(*lists(1025), [0, 1025], 5)
    assert c.tolist() == [5]


# ------------------------------------------------------------------------------------------------ 5. the head
def _gpu_kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")], [e.key for e in prof.key_averages()]


@pytest.mark.parametrize("channels,shapes", [(256, [(50, 84), (13, 21), (4, 6)]), (64, [(25, 42), (7, 11)])])
def test_head_against_fp64(amd, channels, shapes):
    feats_names = ["p2", "p3", "p4"][:len(shapes)]
    m = _rpn(amd, feats_names, channels, (32, 64, 128)[:len(shapes)], pre_k=100, post_k=100, seed=4)
    g = torch.Generator().manual_seed(6)
    xs = {f: torch.randn((2, channels, h, w), generator=g) for f, (h, w) in zip(feats_names, shapes)}
    feats = {f: _pm(x) for f, x in xs.items()}
    A = m.num_anchors
    with torch.no_grad():
        m.head(feats)                                       # warm-up: scratch registration, the concatenated weights
        from test_gpu_pixgemm import _profiled
        heads, ran = _profiled(lambda: m.head(feats))
        assert ran, "the head did not run on the library's pixel GEMMs"
        kernels, ops_seen = _gpu_kernel_names(lambda: m.head(feats))
    bad = [k for k in kernels + ops_seen if any(s in k.lower() for s in ("miopen", "cijk", "hipblas", "rocblas", "aten::conv", "aten::_conv",
                                                                          "aten::mm", "aten::addmm", "aten::sort", "aten::topk"))]
    assert not bad, bad
    print(f"[rpn head] C {channels}: library launch kinds {ran}; {len(kernels)} GPU kernels in the trace: {sorted(set(kernels))[:12]}")
    params = {k[len("rpn_head."):]: v for k, v in m.state_dict().items() if k.startswith("rpn_head.")}
    from test_gpu_pixgemm import R_L2, _bar, _errs
    for f, hd in zip(feats_names, heads):
        assert hd.shape[1] == 16 and not hd[:, 5 * A:].any()
        ref_l, ref_d = R.head(xs[f], params, torch.float64)
        c32_l, c32_d = R.head(xs[f], params, torch.float32)
        # the bars of test_gpu_pixgemm.py for these kernels.  Ktot: an output of the head is a sum over C products of values that are
        # themselves sums over 9 C products; the rounding errors of both reductions add in variance, so the chain's length is 9 C + C.
        ktot = 10 * channels
        for tag, got, ref, c32 in (("logits", hd[:, :A].cpu(), ref_l, c32_l), ("deltas", hd[:, A:5 * A].cpu(), ref_d, c32_d)):
            em, el = _errs(got, ref)
            cm, cl = _errs(c32, ref)
            bar, l2bar = _bar(ktot), R_L2 * max(cl, math.sqrt(ktot) * EPS / 8)
            print(f"[rpn head] C {channels} {f} {tag}: max-norm {em:.2e} (cpu fp32 {cm:.2e}, bar {bar:.2e})  rel-L2 {el:.2e} (cpu fp32 {cl:.2e}, bar {l2bar:.2e})")
            assert em <= bar and el <= l2bar, (f, tag, em, bar, el, l2bar)
    # a parameter change rebuilds the concatenated weights
    with torch.no_grad():
        m.rpn_head.objectness_logits.bias.add_(1.0)
        h2 = m.head(feats)
    assert torch.allclose(h2[0][:, :A], heads[0][:, :A] + 1.0, atol=1e-5) and torch.equal(h2[0][:, A:], heads[0][:, A:])
    # NCHW-contiguous features go through ops.pixel_major
    with torch.no_grad():
        h3 = m.head({f: x.cuda() for f, x in xs.items()})
    assert all(torch.equal(a, b) for a, b in zip(h2, h3))


# ------------------------------------------------------------------------------------------------ 6. full size
FULL = [("p2", 200, 336), ("p3", 100, 168), ("p4", 50, 84), ("p5", 25, 42), ("p6", 13, 21)]


def test_full_size_properties_and_determinism(amd):
    names = [f for f, _, _ in FULL]
    m = _rpn(amd, names, 256, (32, 64, 128, 256, 512), pre_k=1000, post_k=1000, seed=7)
    g = torch.Generator().manual_seed(8)
    feats = {f: _pm(torch.randn((2, 256, h, w), generator=g)) for f, h, w in FULL}
    sizes = [(800, 1344), (768, 1290)]
    hw = torch.tensor(sizes, dtype=torch.float32, device="cuda")
    with torch.no_grad():
        r = m.forward_padded(hw, feats, intermediates=True)
        b2, l2, c2 = m.forward_padded(hw, feats)
        torch.cuda.synchronize()
    assert torch.equal(r["boxes"], b2) and torch.equal(r["logits"], l2) and torch.equal(r["counts"], c2), "two eager runs differ"
    off, thr = r["level_off"], m.nms_thresh
    assert off == [0, 1000, 2000, 3000, 4000, 4000 + 13 * 21 * 3]
    ob, ol, counts = r["boxes"].cpu().double().numpy(), r["logits"].cpu().numpy(), r["counts"].cpu().numpy()
    lb, valid, keep, vals = r["level_boxes"].cpu().double().numpy(), r["valid"].cpu().numpy() != 0, r["keep"].cpu().numpy() != 0, r["vals"].cpu().numpy()
    assert not np.isnan(ob).any() and not np.isnan(ol).any() and not np.isnan(lb).any()
    for n in range(2):
        c = int(counts[n])
        assert 0 < c <= 1000 and np.all(np.diff(ol[n, :c]) <= 0) and not ob[n, c:].any()
        ih, iw = sizes[n]
        bx = ob[n, :c]
        assert bx[:, 0::2].min() >= 0 and bx[:, 0::2].max() <= iw and bx[:, 1::2].min() >= 0 and bx[:, 1::2].max() <= ih
        assert ((bx[:, 2] - bx[:, 0]) > 0).all() and ((bx[:, 3] - bx[:, 1]) > 0).all()
        kept_total = 0
        for l in range(5):
            s = slice(off[l], off[l + 1])
            assert np.all(np.diff(vals[n, s]) <= 0)
            I = R.iou_matrix(lb[n, s])
            kp, vd = keep[n, s], valid[n, s]
            assert not (kp & ~vd).any()
            ki = np.nonzero(kp)[0]
            Ik = I[np.ix_(ki, ki)]
            assert (Ik[np.triu_indices(len(ki), 1)] <= thr + 1e-5).all(), "two kept boxes of one level overlap by more than the threshold"
            for j in np.nonzero(vd & ~kp)[0]:
                earlier = ki[ki < j]
                assert len(earlier) and I[earlier, j].max() > thr - 1e-5, "a suppressed box without an earlier kept box above the threshold"
            kept_total += len(ki)
        assert c == min(kept_total, 1000)
        print(f"[rpn full] image {n}: kept per level {[int(keep[n, off[l]:off[l + 1]].sum()) for l in range(5)]}, proposals {c}")
    # a captured hipGraph of forward_padded replays bit-identically
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(stream):
        for _ in range(2):
            m.forward_padded(hw, feats)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        gr = m.forward_padded(hw, feats, intermediates=True)
    stages = ("vals", "idx", "level_boxes", "valid", "keep", "boxes", "logits", "counts")
    for _ in range(2):
        for k in stages:
            gr[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        differ = [k for k in stages if not torch.equal(gr[k], r[k])]
        assert not differ, f"the hipGraph replay differs from the eager run in {differ}"


# ------------------------------------------------------------------------------------------------ 7. under the detector
def test_detector_inference_hands_the_roi_heads_proposals(amd):
    from afigan_amd.fpn_sr import ShapeSpec

    class Backbone(torch.nn.Module):
        size_divisibility = 32

        def output_shape(self):
            return {f: ShapeSpec(channels=32, stride=2 ** int(f[1:])) for f in LEVELS3}

        def forward(self, x):
            return {f: torch.nn.functional.avg_pool2d(x, 2 ** int(f[1:])).repeat(1, 11, 1, 1)[:, :32].contiguous() for f in LEVELS3}

    seen = {}

    class RoiHeads(torch.nn.Module):
        def forward(self, images, features, proposals, targets=None):
            seen["proposals"] = proposals
            out = []
            for p in proposals:
                r = type("Result", (), {})()
                r.image_size, r.pred_boxes, r.scores = p.image_size, p.proposal_boxes.tensor[:5], p.objectness_logits[:5]
                out.append(r)
            return out, {}

    bb = Backbone()
    rpn = _rpn(amd, LEVELS3, 32, (32, 64, 128), pre_k=300, post_k=100, seed=9)
    det = amd.GeneralizedRCNN_AFExtractor(backbone=bb, proposal_generator=rpn, roi_heads=RoiHeads(), pixel_mean=[100.0, 110.0, 120.0],
                                          pixel_std=[50.0, 55.0, 60.0]).eval()
    assert {k for k in det.state_dict() if k.startswith("proposal_generator.")} == {"proposal_generator." + k for k in rpn.state_dict()}
    g = torch.Generator().manual_seed(10)
    inputs = [{"image_x0.5": torch.rand((3, 160, 224), generator=g) * 255, "height": 320, "width": 448},
              {"image_x0.5": torch.rand((3, 131, 203), generator=g) * 255, "height": 262, "width": 406}]
    with torch.no_grad():
        out = det.inference(inputs)
    props = seen["proposals"]
    assert len(props) == 2 and [tuple(p.image_size) for p in props] == [(160, 224), (131, 203)]
    for p in props:
        t = p.proposal_boxes.tensor
        assert t.is_cuda and t.shape[1] == 4 and 0 < len(p) <= 100 and p.objectness_logits.shape == (len(p),)
        assert bool((t[:, 0::2] <= p.image_size[1]).all()) and bool((t[:, 1::2] <= p.image_size[0]).all()) and bool((t >= 0).all())
    assert len(out) == 2 and tuple(out[0]["instances"].image_size) == (320, 448)
