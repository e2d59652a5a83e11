"""The frozen box branch of StandardROIHeads on the GPU (afigan_amd/roi_heads.py, csrc/roi.hip) against tests/roi_f64.py, stage by stage: every
stage's checker consumes the KERNEL's previous output, so discrete stages (candidates, NMS, pick) are held to exact equality and the
arithmetic ones (ROIAlign, scores / boxes, the box head) to derived bars.  tests/test_roi_host.py proves the seeded inputs' conditions
without a GPU; they are asserted again here before each launch.
"""
import math

import numpy as np
import pytest
import torch

import roi_f64 as Q

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


def _pm(x):
    """CPU NCHW -> GPU tensor whose memory is [N][H][W][C], with those strides spelled out"""
    N, C_, H, W = x.shape
    flat = x.permute(0, 2, 3, 1).reshape(-1).cuda()
    return flat.as_strided((N, C_, H, W), (H * W * C_, 1, W * C_, C_))


def _heads(amd, features, channels, K=80, S=7, fc=1024, num_fc=2, agnostic=False, thresh=0.05, nms=0.5, D=100, sr=0, seed=0):
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": list(features), "NUM_CLASSES": K, "SCORE_THRESH_TEST": thresh,
                                             "NMS_THRESH_TEST": nms},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": num_fc, "FC_DIM": fc, "POOLER_RESOLUTION": S,
                                                "POOLER_SAMPLING_RATIO": sr, "CLS_AGNOSTIC_BBOX_REG": agnostic}})
    cfg.TEST.DETECTIONS_PER_IMAGE = D
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=2 ** int(f[1:])) for f in features})
    g = torch.Generator().manual_seed(seed)
    for name, p in h.named_parameters():
        if name.endswith("weight"):
            scale = {"cls_score": 3.0, "bbox_pred": 2.0}.get(name.split(".")[-2], 1.0)
            p.copy_(torch.randn(p.shape, generator=g) * scale / math.sqrt(p.shape[1]))
        else:
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return h.cuda().eval()


# ------------------------------------------------------------------------------------------------ 1. ROIAlign
_ALIGN_REF = {}


def _align_inputs(C):
    g = torch.Generator().manual_seed(11)
    return [torch.randn((2, C, h, w), generator=g) for h, w in Q.ALIGN_LEVELS]


def _check_align(amd, levels_gpu, levels_cpu, min_level, boxes, counts, S, sr, tag):
    from afigan_amd import ops
    N, P = boxes.shape[:2]
    C = levels_cpu[0].shape[1]
    key = (tag, C, S, sr, tuple(counts))
    if key not in _ALIGN_REF:
        _ALIGN_REF[key] = Q.roi_align([x.numpy() for x in levels_cpu], min_level, boxes, counts, S, sr)
    ref, absum, terms = _ALIGN_REF[key]
    out = torch.full((N * P, S, S, C), float("nan"), device="cuda").permute(0, 3, 1, 2)          # a NaN-filled output buffer must not matter
    got = ops.roi_align(levels_gpu, min_level, torch.from_numpy(boxes).cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda"), S, sr, out=out)
    assert got is out
    got = got.cpu().double().numpy()
    assert not np.isnan(got).any()
    bar = (terms[:, None, None, None] + 4) * EPS * absum
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bar, 1e-300)).max()) if (bar > 0).any() else 0.0
    print(f"[roi align] {tag} C {C} S {S} sampling {sr} counts {counts}: max |err| {err.max():.3e}, max |err| / bar {worst:.3f}")
    assert (err <= bar).all(), (tag, float(err.max()), worst)
    for n in range(N):
        assert not got[n * P + counts[n]:(n + 1) * P].any(), "padding rows must be exactly zero"
    return got


@pytest.mark.parametrize("counts", Q.ALIGN_COUNTS)
@pytest.mark.parametrize("sr", [0, 2])
@pytest.mark.parametrize("C,S", [(4, 7), (12, 7), (256, 7), (12, 2), (256, 2)])
def test_roi_align_against_fp64(amd, C, S, sr, counts):
    boxes = Q.align_boxes()
    max_level = Q.ALIGN_MIN_LEVEL + len(Q.ALIGN_LEVELS) - 1
    assert Q.align_facts(boxes, S, sr, Q.ALIGN_MIN_LEVEL, max_level) > 1e-6
    xs = _align_inputs(C)
    got = _check_align(amd, [_pm(x) for x in xs], xs, Q.ALIGN_MIN_LEVEL, boxes, list(counts), S, sr, "pyramid")
    if counts[0] >= Q.ALIGN_EXACT:
        assert not got[7].any() and not got[8].any(), "a zero-width / negative-width box pools to zeros"
        assert got[:7].any(axis=(1, 2, 3)).all()
    if C == 12:
        # the same levels as channel slices of wider buffers (strided views)
        wide = [_pm(torch.cat([torch.full_like(x[:, :4], 7.0), x, torch.full_like(x[:, :8], -3.0)], 1)) for x in xs]
        views = [w[:, 4:4 + C] for w in wide]
        assert views[0].stride(3) == C + 12
        got2 = _check_align(amd, views, xs, Q.ALIGN_MIN_LEVEL, boxes, list(counts), S, sr, "pyramid")
        assert np.array_equal(got, got2), "strided input views give another result"


def test_roi_align_large_adaptive_grid(amd):
    g = torch.Generator().manual_seed(12)
    x = torch.randn((1, 8, 40, 40), generator=g)
    boxes = np.array([[[0, 0, 160, 160], [-3.3, 1.7, 170.2, 158.9], [20.5, 30.25, 150.75, 101.5]]], np.float32)
    assert Q.grid_of(boxes[0, 0].astype(np.float64), 2, 7, 0)[:2] == (6, 6)
    assert Q.align_facts(boxes, 7, 0, 2, 2, skip=1) > 1e-6
    _check_align(amd, [_pm(x)], [x], 2, boxes, [3], 7, 0, "single 40x40")


def test_roi_align_refusals(amd):
    from afigan_amd import ops
    x = _pm(torch.zeros((1, 8, 4, 4)))
    b, c = torch.zeros((1, 2, 4), device="cuda"), torch.ones((1,), dtype=torch.int32, device="cuda")
    with pytest.raises(amd.AfiError):
        ops.roi_align([x], 2, b, c, 15)
    with pytest.raises(amd.AfiError):
        ops.roi_align([x] * 9, 2, b, c, 7)
    with pytest.raises(amd.AfiError):
        ops.roi_align([_pm(torch.zeros((1, 6, 4, 4)))], 2, b, c, 7)
    with pytest.raises(amd.AfiError):
        ops.roi_align([x], 2, b, c, 7, sampling_ratio=-1)


# ------------------------------------------------------------------------------------------------ 2. scores and boxes
def _pred_case(K, agnostic, seed=21, N=2, P=50):
    r = np.random.RandomState(seed)
    Kb = 1 if agnostic else K
    cpad = (K + 1 + 4 * Kb + 3) // 4 * 4
    pred = np.zeros((N * P, cpad), np.float32)
    pred[:, :K + 1] = r.uniform(-30, 30, (N * P, K + 1))
    pred[:, K + 1:K + 1 + 4 * Kb] = r.randn(N * P, 4 * Kb) * 4
    pred[3, K + 1 + 2] = 60.0                              # dw above the clamp (weight 5: 12 > log(1000 / 16))
    pred[4, K + 1 + 3] = 45.0
    pred[5, K + 1:K + 5] = (-800, -800, 0, 0)                # clips at 0
    pred[6, K + 1:K + 5] = (800, 800, 0, 0)                  # clips at the image size
    pred[7, 0] = np.nan                                    # a NaN row
    hw = [(60.0, 90.0), (75.0, 50.0)]
    props = np.zeros((N, P, 4), np.float32)
    for n in range(N):
        ctr = r.rand(P, 2) * [hw[n][1], hw[n][0]]
        wh = np.exp(r.uniform(np.log(2), np.log(40), (P, 2)))
        props[n] = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)
    return pred, props, [43, 50], hw


@pytest.mark.parametrize("K,agnostic", [(80, False), (80, True), (3, False), (3, True), (1, False)])
def test_scores_and_boxes_against_fp64(amd, K, agnostic):
    from afigan_amd import ops
    pred, props, counts, hw = _pred_case(K, agnostic)
    w = (10.0, 10.0, 5.0, 5.0)
    ref_s, ref_b, (pcx, pcy, pw, ph) = Q.scores_boxes(pred, K, agnostic, props, counts, hw, w)
    sc, bx = ops.roi_scores_boxes(torch.from_numpy(pred).cuda(), K, agnostic, torch.from_numpy(props).cuda(),
                                  torch.tensor(counts, dtype=torch.int32, device="cuda"), torch.tensor(hw, device="cuda"), w)
    sc, bx = sc.cpu().double().numpy(), bx.cpu().double().numpy()
    assert np.isneginf(sc[0, 43:]).all() and not bx[0, 43:].any(), "padded rows score -inf"
    assert np.isnan(sc[0, 7]).all() and np.isnan(ref_s[0, 7]).all()
    live = np.isfinite(ref_s)
    assert live.sum() == (93 - 1) * K and np.isfinite(sc[live]).all()
    es = np.abs(sc - ref_s)[live] / (2.0 ** -23 * ref_s[live] + 1e-300)
    real = np.zeros(ref_b.shape[:3], bool)
    real[0, :43], real[1] = True, True
    bar = 16 * EPS * np.stack([np.abs(pcx) + pw, np.abs(pcy) + ph, np.abs(pcx) + pw, np.abs(pcy) + ph], -1)
    eb = np.abs(bx - ref_b)[real] / bar[real]
    print(f"[roi scores] K {K} agnostic {agnostic}: max |err| / (2^-23 score) {es.max():.3f}; boxes max |err| / bar {eb.max():.3f}")
    assert es.max() <= 1.0 and eb.max() <= 1.0
    # the clamp and all four clips are hit
    Kb = 1 if agnostic else K
    assert pred[3, K + 3] / 5 > Q.SCALE_CLAMP and (bx[0, 5, 0, :2] == 0).all() and bx[0, 6, 0, 2] == hw[0][1] and bx[0, 6, 0, 3] == hw[0][0]
    assert bx.shape == (2, 50, Kb, 4) and bx[..., 0::2].max() <= 90 and bx.min() >= 0


# ------------------------------------------------------------------------------------------------ 3. candidates, NMS, pick
def _check_selection(amd, scores, cboxes, thresh, nms_thresh, D, M=1024):
    """candidates -> NMS -> pick on the GPU, each stage against the checker on the kernel's own previous output; returns the pick."""
    from afigan_amd import ops
    cand = ops.roi_candidates(scores, cboxes, thresh, M)
    keep = ops.roi_nms(cand["boxes"], cand["cls"], cand["valid"], nms_thresh)
    ob, os_, oc, cn, tr = ops.roi_pick(cand, keep, D)
    torch.cuda.synchronize()
    N, P, K = scores.shape
    s_np, b_np = scores.cpu().numpy(), cboxes.cpu().numpy()
    out = []
    for n in range(N):
        idx, valid, n_over = Q.candidates(s_np[n], thresh, M)
        m = len(idx)
        assert np.array_equal(cand["idx"][n, :m].cpu().numpy(), idx), "candidate order"
        assert np.array_equal(cand["valid"][n, :m].cpu().numpy() != 0, valid) and int(cand["n_over"][n]) == n_over
        assert not cand["valid"][n, m:].any() and (cand["idx"][n, m:] == -1).all()
        r, c = idx // K, idx % K
        assert np.array_equal(cand["cls"][n, :m].cpu().numpy(), c)
        assert np.array_equal(cand["scores"][n, :m].cpu().numpy(), s_np[n].reshape(-1)[idx], equal_nan=True)
        assert np.array_equal(cand["boxes"][n, :m].cpu().numpy(), b_np[n, r, c if b_np.shape[2] > 1 else 0])
        kb, kc, kv = cand["boxes"][n].cpu().numpy(), cand["cls"][n].cpu().numpy(), cand["valid"][n].cpu().numpy() != 0
        want = Q.nms_classes(kb, kc, kv, nms_thresh, rounding_pairs_in_fp32=True)
        assert np.array_equal(keep[n].cpu().numpy() != 0, want), "NMS keep set"
        pos, trunc = Q.pick(want, n_over, M, D)
        cnt = len(pos)
        assert int(cn[n]) == cnt and bool(tr[n]) == trunc
        assert np.array_equal(ob[n, :cnt].cpu().numpy(), kb[pos]) and np.array_equal(oc[n, :cnt].cpu().numpy(), kc[pos])
        assert np.array_equal(os_[n, :cnt].cpu().numpy(), cand["scores"][n].cpu().numpy()[pos])
        assert not ob[n, cnt:].any() and not os_[n, cnt:].any() and not oc[n, cnt:].any()
        out.append((cnt, trunc, n_over, int(want.sum())))
    return out


def _score_case(P, K, seed, quant):
    r = np.random.RandomState(seed)
    s = r.rand(2, P, K).astype(np.float32) ** 6
    s = np.round(s * quant) / quant                        # quantised: many ties, also across the cut at M
    s[0, P - 2:] = -np.inf
    s[1, 0, 0] = np.nan
    ctr = r.rand(2, P, K, 2) * [300, 200]
    wh = np.exp(r.uniform(np.log(8), np.log(120), (2, P, K, 2)))
    b = np.concatenate([ctr - wh / 2, ctr + wh / 2], -1).astype(np.float32)
    return torch.from_numpy(s.astype(np.float32)).cuda(), torch.from_numpy(b).cuda()


@pytest.mark.parametrize("P,K,quant", [(1000, 80, 64), (7, 3, 8)])
@pytest.mark.parametrize("thresh", [0.05, 0.0])
def test_candidates_nms_pick_are_exact(amd, P, K, quant, thresh):
    scores, boxes = _score_case(P, K, 31, quant)
    res = _check_selection(amd, scores, boxes, thresh, 0.5, 100)
    if P == 1000:
        flat = np.sort(scores[1].cpu().numpy().reshape(-1))[::-1]
        assert flat[1023] == flat[1024], "the inputs must tie across the cut at M"
        assert all(r[2] > 1024 for r in res)
    print(f"[roi select] P {P} K {K} thresh {thresh}: (count, truncated, n_over, kept) {res}")
    # agnostic boxes [N, P, 1, 4]
    _check_selection(amd, scores, boxes[:, :, :1].contiguous(), thresh, 0.5, 100)


@pytest.mark.parametrize("n", Q.NMS_SIZES)
@pytest.mark.parametrize("thresh", Q.NMS_THRESHOLDS)
@pytest.mark.parametrize("nclass", Q.NMS_CLASS_COUNTS)
def test_class_nms_keep_set_is_exact(amd, n, thresh, nclass):
    from afigan_amd import ops
    boxes, cls = Q.nms_class_case(n, nclass)
    if n >= 2:
        ambiguous, frac = Q.nms_class_facts(boxes, cls, thresh)
        assert ambiguous == 0 and 0.1 <= frac <= 0.9
    valid = np.ones(n, np.int32)
    valid[3::17] = 0
    b2 = np.stack([boxes, boxes[::-1]]) if n else np.zeros((2, 0, 4), np.float32)
    c2 = np.stack([cls, cls[::-1]]) if n else np.zeros((2, 0), np.int32)
    v2 = np.stack([valid, valid])
    keep = ops.roi_nms(torch.from_numpy(np.ascontiguousarray(b2)).cuda(), torch.from_numpy(np.ascontiguousarray(c2)).cuda(),
                       torch.from_numpy(v2).cuda(), thresh).cpu().numpy() != 0
    for i in range(2):
        assert np.array_equal(keep[i], Q.nms_classes(b2[i], c2[i], v2[i], thresh, rounding_pairs_in_fp32=(i == 1)))


def test_different_classes_overlap_and_both_survive(amd):
    from afigan_amd import ops
    b = torch.tensor([[[0, 0, 10, 10], [1, 1, 11, 11], [0, 0, 10, 10]]], dtype=torch.float32, device="cuda")
    assert Q._iou(b[0].cpu().numpy())[0, 1] > 0.5
    keep = ops.roi_nms(b, torch.tensor([[0, 1, 0]], dtype=torch.int32, device="cuda"), torch.ones((1, 3), dtype=torch.int32, device="cuda"), 0.5)
    assert keep.cpu().tolist() == [[1, 1, 0]]
    same = ops.roi_nms(b, torch.zeros((1, 3), dtype=torch.int32, device="cuda"), torch.ones((1, 3), dtype=torch.int32, device="cuda"), 0.5)
    assert same.cpu().tolist() == [[1, 0, 0]]


def test_truncated_flag(amd):
    """n_over > M with fewer than D kept: truncated; n_over > M with D kept: clear and exact."""
    P, K = 400, 4
    s = torch.full((2, P, K), 0.5, device="cuda")
    s += torch.arange(P * K, device="cuda").reshape(P, K) * -1e-5
    # image 0: every box the same -> one kept per class; image 1: disjoint boxes -> everything kept
    b = torch.zeros((2, P, K, 4), device="cuda")
    b[0] = torch.tensor([5.0, 5.0, 50.0, 60.0], device="cuda")
    i = torch.arange(P * K, device="cuda", dtype=torch.float32).reshape(P, K)
    b[1] = torch.stack([(i % 40) * 10, (i // 40) * 10, (i % 40) * 10 + 8, (i // 40) * 10 + 8], -1)
    res = _check_selection(amd, s, b, 0.05, 0.5, 100)
    assert res[0] == (K, True, P * K, K) and res[1][:3] == (100, False, P * K)


# ------------------------------------------------------------------------------------------------ 4. the box head
def _gpu_kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")], [e.key for e in prof.key_averages()]


@pytest.mark.parametrize("C,S,fc,P", [(256, 7, 1024, 24), (16, 7, 64, 24)])
def test_box_head_against_fp64(amd, C, S, fc, P):
    from test_gpu_pixgemm import R_L2, _bar, _errs, _profiled
    h = _heads(amd, ["p2"], C, K=80, S=S, fc=fc, seed=41)
    g = torch.Generator().manual_seed(42)
    pooled_cpu = torch.randn((2 * P, C, S, S), generator=g)
    pooled = _pm(pooled_cpu)
    with torch.no_grad():
        h.box_head_forward(pooled)                          # warm-up: scratch registration, the prepared weights
        (pred, acts), ran = _profiled(lambda: h.box_head_forward(pooled, intermediates=True))
        assert ran, "the box head did not run on the library's pixel GEMMs"
        kernels, ops_seen = _gpu_kernel_names(lambda: h.box_head_forward(pooled))
    bad = [k for k in kernels + ops_seen if any(s in k.lower() for s in ("miopen", "cijk", "hipblas", "rocblas", "aten::mm", "aten::addmm", "aten::linear",
                                                                          "aten::matmul", "softmax", "aten::sort", "aten::topk"))]
    assert not bad, bad
    print(f"[roi head] C {C}: library launch kinds {ran}; GPU kernels in the trace: {sorted(set(kernels))[:8]}")
    sd = h.state_dict()
    r_acts, r_log, r_del = Q.box_head(pooled_cpu, sd, torch.float64)
    c_acts, c_log, c_del = Q.box_head(pooled_cpu, sd, torch.float32)
    K = 80
    k1 = C * S * S
    assert k1 == (12544 if C == 256 else 784)
    pred = pred.cpu()
    assert pred.shape[1] == (K + 1 + 4 * K + 3) // 4 * 4 and not pred[:, 5 * K + 1:].any()
    # Ktot accumulates through the chain: fc1's K, then + FC_DIM for every further layer
    rows = [("fc1", acts[0].cpu(), r_acts[0], c_acts[0], k1), ("fc2", acts[1].cpu(), r_acts[1], c_acts[1], k1 + fc),
            ("cls_score", pred[:, :K + 1], r_log, c_log, k1 + 2 * fc), ("bbox_pred", pred[:, K + 1:5 * K + 1], r_del, c_del, k1 + 2 * fc)]
    fails = []
    for tag, got, ref, c32, ktot in rows:
        em, el = _errs(got, ref)
        cm, cl = _errs(c32, ref)
        bar, l2bar = _bar(ktot), R_L2 * max(cl, math.sqrt(ktot) * EPS / 8)
        print(f"[roi head] C {C} {tag} Ktot {ktot}: max-norm {em:.2e} (cpu fp32 {cm:.2e}, bar {bar:.2e})  rel-L2 {el:.2e} (cpu fp32 {cl:.2e}, bar {l2bar:.2e})")
        if not (em <= bar and el <= l2bar):
            fails.append((tag, em, bar, el, l2bar))
    assert not fails, fails
    # an in-place parameter change rebuilds the prepared weights
    with torch.no_grad():
        h.box_predictor.cls_score.bias.add_(1.0)
        p2 = h.box_head_forward(pooled).cpu()
        assert torch.allclose(p2[:, :K + 1], pred[:, :K + 1] + 1.0, atol=1e-5) and torch.equal(p2[:, K + 1:], pred[:, K + 1:])
        h.box_head.fc1.weight.zero_()
        p3 = h.box_head_forward(pooled)
        a1 = torch.relu(h.box_head.fc1.bias)
        assert not torch.equal(p3.cpu(), p2) and torch.equal(p3[0], p3[-1]) and a1.shape == (fc,)


# ------------------------------------------------------------------------------------------------ 5. whole heads
LEVELS4 = ["p2", "p3", "p4", "p5"]


def _whole_case(amd, thresh=0.05, D=20):
    h = _heads(amd, LEVELS4, 16, K=5, S=7, fc=64, thresh=thresh, D=D, seed=51)
    g = torch.Generator().manual_seed(52)
    xs = {f: torch.randn((2, 16, hh, ww), generator=g) for f, (hh, ww) in zip(LEVELS4, Q.ALIGN_LEVELS)}
    boxes = torch.from_numpy(Q.align_boxes(seed=6)).cuda()
    boxes[..., 0::2] = boxes[..., 0::2].clamp(0, 80)
    boxes[..., 1::2] = boxes[..., 1::2].clamp(0, 64)
    counts = torch.tensor([37, 40], dtype=torch.int32, device="cuda")
    hw = torch.tensor([(64.0, 80.0), (60.0, 77.0)], device="cuda")
    return h, xs, {f: _pm(x) for f, x in xs.items()}, boxes, counts, hw


def test_forward_padded_equals_the_staged_checker_and_is_deterministic(amd):
    h, xs, feats, boxes, counts, hw = _whole_case(amd)
    with torch.no_grad():
        r = h.forward_padded(hw, feats, boxes, counts, intermediates=True)
        out2 = h.forward_padded(hw, feats, boxes, counts)
        torch.cuda.synchronize()
    names = ("boxes", "scores", "classes", "counts", "truncated")
    assert all(torch.equal(r[k], o) for k, o in zip(names, out2)), "two eager runs differ"
    assert torch.equal(h.box_features(feats, boxes, counts), r["pooled"])
    # stage by stage on the kernels' intermediates
    ref, absum, terms = Q.roi_align([xs[f].numpy() for f in LEVELS4], 2, boxes.cpu().numpy(), counts.tolist(), 7, 0)
    assert (np.abs(r["pooled"].cpu().double().numpy() - ref) <= (terms[:, None, None, None] + 4) * EPS * absum).all()
    K = 5
    s_ref, b_ref, _ = Q.scores_boxes(r["pred"].cpu().numpy(), K, False, boxes.cpu().numpy(), counts.tolist(), hw.cpu().numpy(), h.box_weights)
    live = np.isfinite(s_ref)
    assert (np.abs(r["class_scores"].cpu().double().numpy() - s_ref)[live] <= 2.0 ** -23 * s_ref[live]).all()
    assert np.isneginf(r["class_scores"][0, 37:].cpu().numpy()).all()
    res = _check_selection(amd, r["class_scores"], r["class_boxes"], h.test_score_thresh, h.test_nms_thresh, h.test_detections_per_img)
    assert [c for c, *_ in res] == r["counts"].tolist() and all(c > 0 for c, *_ in res)
    # forward == forward_padded
    from afigan_amd.rpn import Boxes, Proposals
    images = type("Images", (), {"image_sizes": [(64, 80), (60, 77)], "__len__": lambda s: 2})()
    props = [Proposals(sz, Boxes(boxes[n, :c]), torch.zeros(c, device="cuda")) for n, (sz, c) in enumerate(zip(images.image_sizes, counts.tolist()))]
    with torch.no_grad():
        results, losses = h(images, feats, props)
    assert losses == {} and len(results) == 2
    for n, d in enumerate(results):
        c = int(r["counts"][n])
        assert len(d) == c and d.pred_classes.dtype == torch.int64 and tuple(d.image_size) == images.image_sizes[n]
        assert torch.equal(d.pred_boxes.tensor, r["boxes"][n, :c]) and torch.equal(d.scores, r["scores"][n, :c])
        assert torch.equal(d.pred_classes, r["classes"][n, :c].long())
    # a captured hipGraph of forward_padded replays bit-identically
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(stream):
        for _ in range(2):
            h.forward_padded(hw, feats, boxes, counts)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        gr = h.forward_padded(hw, feats, boxes, counts)
    for _ in range(2):
        for t in gr:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        differ = [k for k, t in zip(names, gr) if not torch.equal(t, r[k])]
        assert not differ, f"the hipGraph replay differs from the eager run in {differ}"


def test_forward_raises_when_truncated(amd):
    """More than M = 1024 class scores above the threshold and fewer than D kept: forward refuses by name."""
    h, xs, feats, boxes, counts, hw = _whole_case(amd, thresh=0.0, D=1000)
    P, K = 300, 5
    big = boxes[:, :1].repeat(1, P, 1).contiguous()
    big[:] = torch.tensor([10.0, 10.0, 50.0, 50.0], device="cuda")
    cnt = torch.tensor([P, P], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        h.box_predictor.bbox_pred.weight.zero_()
        h.box_predictor.bbox_pred.bias.zero_()
        out = h.forward_padded(hw, feats, big, cnt)
    assert out[4].tolist() == [1, 1] and max(out[3].tolist()) <= K
    from afigan_amd.rpn import Boxes, Proposals
    images = type("Images", (), {"image_sizes": [(64, 80), (60, 77)], "__len__": lambda s: 2})()
    props = [Proposals(sz, Boxes(big[n]), torch.zeros(P, device="cuda")) for n, sz in enumerate(images.image_sizes)]
    with torch.no_grad(), pytest.raises(amd.AfiError, match=r"SCORE_THRESH_TEST.*1024|1024.*SCORE_THRESH_TEST"):
        h(images, feats, props)


def test_detector_inference_returns_instances(amd):
    from afigan_amd.fpn_sr import ShapeSpec
    from test_gpu_rpn import _rpn

    class Backbone(torch.nn.Module):
        size_divisibility = 32

        def output_shape(self):
            return {f: ShapeSpec(channels=32, stride=2 ** int(f[1:])) for f in LEVELS4}

        def forward(self, x):
            return {f: torch.nn.functional.avg_pool2d(x, 2 ** int(f[1:])).repeat(1, 11, 1, 1)[:, :32].contiguous() for f in LEVELS4}

    bb = Backbone()
    rpn = _rpn(amd, LEVELS4, 32, (32, 64, 128, 256), pre_k=300, post_k=100, seed=9)
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": LEVELS4, "NUM_CLASSES": 5, "SCORE_THRESH_TEST": 0.05},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "FC_DIM": 64, "POOLER_RESOLUTION": 7}})
    heads = amd.build_roi_heads(cfg, bb.output_shape())
    g = torch.Generator().manual_seed(61)
    with torch.no_grad():
        heads.box_predictor.cls_score.weight.copy_(torch.randn(heads.box_predictor.cls_score.weight.shape, generator=g))
        heads.box_predictor.bbox_pred.weight.copy_(torch.randn(heads.box_predictor.bbox_pred.weight.shape, generator=g) * 0.3)
    det = amd.GeneralizedRCNN_AFExtractor(backbone=bb, proposal_generator=rpn, roi_heads=heads, pixel_mean=[100.0, 110.0, 120.0],
                                          pixel_std=[50.0, 55.0, 60.0]).eval()
    assert {k for k in det.state_dict() if k.startswith("roi_heads.")} == {"roi_heads." + k for k in heads.state_dict()}
    inputs = [{"image_x0.5": torch.rand((3, 64, 80), generator=g) * 255, "height": 128, "width": 160},
              {"image_x0.5": torch.rand((3, 57, 71), generator=g) * 255, "height": 114, "width": 142}]
    with torch.no_grad():
        out = det.inference(inputs)
        raw = det.inference(inputs, do_postprocess=False)
    assert len(out) == 2 and all(set(o) == {"instances"} for o in out)
    total = 0
    for o, rw, inp in zip(out, raw, inputs):
        r = o["instances"]
        t = r.pred_boxes.tensor
        assert tuple(r.image_size) == (inp["height"], inp["width"]) and t.is_cuda and t.shape[1] == 4
        assert r.scores.shape == (len(t),) and r.pred_classes.dtype == torch.int64 and len(r.pred_classes) == len(t)
        assert bool((t >= 0).all()) and bool((t[:, 0::2] <= inp["width"]).all()) and bool((t[:, 1::2] <= inp["height"]).all())
        assert len(t) <= len(rw.pred_boxes.tensor) <= 100
        if len(t) == len(rw.pred_boxes.tensor):                 # no box became empty: the boxes are the raw ones times 2, clipped
            want = rw.pred_boxes.tensor * 2.0
            want[:, 0::2].clamp_(0, inp["width"])
            want[:, 1::2].clamp_(0, inp["height"])
            assert torch.allclose(t, want, rtol=1e-6, atol=1e-4)
        total += len(t)
    assert total > 0, "no detection at all: the test would show nothing"
