"""The frozen CascadeROIHeads on the GPU (afigan_amd/roi_heads.py, afi_roi_cascade_stage in csrc/roi.hip) against tests/cascade_f64.py, stage by
stage: every stage's checker consumes the KERNEL's previous output, so the discrete stages (candidates, NMS, pick) and the running score are
held to exact equality and the arithmetic ones (ROIAlign, the conv-FC head, the normed mask head) to derived bars.  tests/test_cascade_host.py
proves the seeded inputs' conditions without a GPU; they are asserted again here.

Bars.  afi_roi_cascade_stage: none -- stage 0 is afi_roi_scores_boxes(agnostic = 1) bit for bit, and the accumulation is (prev + s) * scale in
numpy fp32, exactly.  ROIAlign: test_gpu_roi.py's (terms + 4) 2^-24 sum |w f|.  The heads: test_gpu_pixgemm.py's _bar / R_L2 with Ktot
accumulating through the chain (9 C per conv, + S^2 CONV_DIM for fc1, + FC_DIM for the predictor; + C for the mask head's deconv).
"""
import math

import numpy as np
import pytest
import torch

import cascade_f64 as Q
import roi_f64 as QB

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
VENDOR = ("miopen", "cijk", "hipblas", "rocblas", "aten::mm", "aten::addmm", "aten::linear", "aten::matmul", "aten::conv", "aten::_conv", "aten::cudnn",
          "aten::miopen", "softmax", "aten::sort", "aten::topk", "aten::sigmoid", "conv_transpose", "batch_norm")


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


def _pm(x):
    """CPU NCHW -> GPU tensor whose memory is [N][H][W][C]"""
    N, C_, H, W = x.shape
    flat = x.permute(0, 2, 3, 1).reshape(-1).cuda()
    return flat.as_strided((N, C_, H, W), (H * W * C_, 1, W * C_, C_))


def _gpu_kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")], [e.key for e in prof.key_averages()]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """fp32 arrays equal element by element, NaN matching NaN and -inf matching -inf."""
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


# ------------------------------------------------------------------------------------------------ 1. afi_roi_cascade_stage
def _stage_inputs(K, counts, seed=21):
    pred, props = Q.stage_case(K, seed)
    return (torch.from_numpy(pred).cuda(), torch.from_numpy(props).cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda"),
            torch.tensor(Q.STAGE_HW, device="cuda"))


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


@pytest.mark.parametrize("counts", Q.STAGE_COUNTS)
@pytest.mark.parametrize("w", Q.STAGE_WEIGHTS)
@pytest.mark.parametrize("K", Q.STAGE_KS)
def test_stage_is_scores_boxes_and_an_exact_fp32_accumulation(amd, K, w, counts):
    from afigan_amd import ops
    N, P = Q.STAGE_N, Q.STAGE_P
    pred, props, cnt, hw = _stage_inputs(K, counts)
    s0, b0 = ops.roi_scores_boxes(pred, K, True, props, cnt, hw, w)
    out, ob = _nan(N, P, K), _nan(N, P, 4)
    s, b = ops.roi_cascade_stage(pred, K, props, cnt, hw, w, out=out, out_boxes=ob)
    assert s is out and b is ob and tuple(b0.shape) == (N, P, 1, 4)
    assert torch.equal(_bits(s), _bits(s0)) and torch.equal(_bits(b), _bits(b0[:, :, 0])), "stage 0 differs from afi_roi_scores_boxes(agnostic = 1)"
    s_np, b_np = s.cpu().numpy(), b.cpu().numpy()
    for n, c in enumerate(counts):
        assert np.isneginf(s_np[n, c:]).all() and not b_np[n, c:].any()
        if c > 7:
            ih, iw = Q.STAGE_HW[n]
            assert np.isnan(s_np[n, 7]).all() and np.isfinite(s_np[n, :7]).all() and np.isfinite(b_np[n]).all()
            assert (b_np[n, 5, :2] == 0).all() and b_np[n, 6, 2] == iw and b_np[n, 6, 3] == ih
    prev = Q.stage_prev(K, counts)
    for scale in (1.0, float(np.float32(1.0 / 3)), 0.5):
        with np.errstate(invalid="ignore"):
            want = (prev + s_np) * np.float32(scale)
        got, gb = ops.roi_cascade_stage(pred, K, props, cnt, hw, w, prev_scores=torch.from_numpy(prev).cuda(), out_scale=scale, out=_nan(N, P, K))
        assert _same(got.cpu().numpy(), want), f"(prev + s) * {scale} is not the fp32 result"
        assert torch.equal(gb, b)
        for n, c in enumerate(counts):
            assert np.isneginf(got[n, c:].cpu().numpy()).all()
        buf = torch.from_numpy(prev).cuda()
        inplace, _ = ops.roi_cascade_stage(pred, K, props, cnt, hw, w, prev_scores=buf, out_scale=scale, out=buf)
        assert inplace is buf and _same(buf.cpu().numpy(), want), "in place (scores is prev_scores) differs"
    fresh, _ = ops.roi_cascade_stage(pred, K, props, cnt, hw, w, prev_scores=torch.from_numpy(prev).cuda())
    assert _same(fresh.cpu().numpy(), prev + s_np)


@pytest.mark.parametrize("K", Q.STAGE_KS)
def test_three_chained_stages_equal_the_mean_of_three_stage0_calls(amd, K):
    from afigan_amd import ops
    counts = Q.STAGE_COUNTS[0]
    _, props, cnt, hw = _stage_inputs(K, counts)
    preds = [torch.from_numpy(Q.stage_case(K, seed)[0]).cuda() for seed in (21, 31, 41)]
    ws = ((10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0))
    run, cur, per = None, props, []
    for k in range(3):
        s0, b0 = ops.roi_scores_boxes(preds[k], K, True, cur, cnt, hw, ws[k])
        per.append(s0.cpu().numpy())
        run, nxt = ops.roi_cascade_stage(preds[k], K, cur, cnt, hw, ws[k], prev_scores=run, out_scale=1.0 / 3 if k == 2 else 1.0, out=run)
        assert torch.equal(_bits(nxt), _bits(b0[:, :, 0]))
        cur = nxt
    assert _same(run.cpu().numpy(), Q.mean_scores(per))
    assert np.isnan(run[0, 7].cpu().numpy()).all() and np.isneginf(run[1, 17:].cpu().numpy()).all()


def test_stage_refusals_and_return_codes(amd):
    from afigan_amd import _lib, ops
    K = 3
    pred, props, cnt, hw = _stage_inputs(K, Q.STAGE_COUNTS[0])
    w = Q.STAGE_WEIGHTS[0]
    for kw in ({"prev_scores": torch.zeros((2, 50, 4), device="cuda")}, {"out": torch.zeros((2, 49, 3), device="cuda")},
               {"out_boxes": torch.zeros((2, 50, 1, 4), device="cuda")}, {"out_scale": 0.0}, {"out_scale": float("inf")},
               {"prev_scores": torch.zeros((2, 50, 3))}):
        with pytest.raises(amd.AfiError):
            ops.roi_cascade_stage(pred, K, props, cnt, hw, w, **kw)
    with pytest.raises(amd.AfiError, match="roi_cascade_stage: pred"):
        ops.roi_cascade_stage(pred[:, :7], K, props, cnt, hw, w)
    with pytest.raises(amd.AfiError):
        ops.roi_cascade_stage(pred, K, props, cnt.long(), hw, w)
    lib = _lib.load()
    BAD, UNS = _lib.DEFINES["AFI_ERR_BAD_ARG"], _lib.DEFINES["AFI_ERR_UNSUPPORTED"]
    s, b = torch.empty((2, 50, K), device="cuda"), torch.empty((2, 50, 4), device="cuda")
    args = lambda ld=8, N=2, K_=K, wx=10.0, sc=1.0, out=s: (pred.data_ptr(), ld, N, 50, K_, props.data_ptr(), cnt.data_ptr(), hw.data_ptr(), wx, 10.0,  # noqa: E731
                                                             5.0, 5.0, 4.135, None, sc, out.data_ptr() if out is not None else None, b.data_ptr(), None)
    assert lib.afi_roi_cascade_stage(*args(ld=7)) == BAD and lib.afi_roi_cascade_stage(*args(N=0)) == BAD
    assert lib.afi_roi_cascade_stage(*args(wx=0.0)) == BAD and lib.afi_roi_cascade_stage(*args(sc=0.0)) == BAD
    assert lib.afi_roi_cascade_stage(*args(out=None)) == BAD and lib.afi_roi_cascade_stage(*args(K_=1025, ld=1030)) == UNS
    assert lib.afi_roi_cascade_stage(*args()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the conv-FC head
def _chain_rows(C, S, num_conv, conv_dim, fc, K, convs, fcs, pred, ref, c32):
    """(tag, got, fp64, cpu fp32, Ktot) of every layer of one head, Ktot accumulating through the chain."""
    rows, ktot, cin = [], 0, C
    for i in range(num_conv):
        ktot += 9 * cin
        rows.append((f"conv{i + 1}", convs[i].cpu(), ref[0][i], c32[0][i], ktot))
        cin = conv_dim
    ktot += S * S * cin
    rows.append(("fc1", fcs[0].cpu(), ref[1][0], c32[1][0], ktot))
    ktot += fc
    p = pred.cpu()
    rows.append(("cls_score", p[:, :K + 1], ref[2], c32[2], ktot))
    rows.append(("bbox_pred", p[:, K + 1:K + 5], ref[3], c32[3], ktot))
    return rows


def _check_rows(tag, rows):
    from test_gpu_pixgemm import R_L2, _bar, _errs
    fails = []
    for name, got, ref, c32, ktot in rows:
        assert not torch.isnan(got).any()
        em, el = _errs(got, ref)
        cm, cl = _errs(c32, ref)
        bar, l2bar = _bar(ktot), R_L2 * max(cl, math.sqrt(ktot) * EPS / 8)
        print(f"[cascade head] {tag} {name} Ktot {ktot}: max-norm {em:.2e} (cpu fp32 {cm:.2e}, bar {bar:.2e})  rel-L2 {el:.2e} (cpu fp32 {cl:.2e}, bar {l2bar:.2e})")
        if not (em <= bar and el <= l2bar):
            fails.append((name, em, bar, el, l2bar))
    assert not fails, (tag, fails)


@pytest.mark.parametrize("norm", Q.HEAD_NORMS)
@pytest.mark.parametrize("case", sorted(Q.HEAD_CASES))
def test_conv_fc_head_against_fp64(amd, case, norm):
    from test_gpu_pixgemm import _profiled
    C, S, num_conv, conv_dim, fc, half = Q.HEAD_CASES[case]
    K, R = 80, 2 * half
    stages = 2 if C < 128 else 1
    k = stages - 1
    h = Q.build_heads(amd, ["p2"], C, K=K, S=S, fc=fc, num_conv=num_conv, conv_dim=conv_dim, norm=norm, stages=stages, seed=41).cuda()
    pooled_cpu = torch.randn((R, C, S, S), generator=torch.Generator().manual_seed(42 + R))
    pooled = _pm(pooled_cpu)
    wino = C >= 128 and conv_dim >= 128 and R * S * S >= 1024
    assert wino == (case == "a") and R * S * S == {"a": 2352, "b": 490, "c": 2352}[case]
    with torch.no_grad():
        h.box_head_forward(pooled, k)                             # warm-up: scratch registration, the prepared weights
        (pred, convs, fcs), ran = _profiled(lambda: h.box_head_forward(pooled, k, intermediates=True))
        assert ran, "the head did not run on the library's pixel GEMMs"
        kernels, ops_seen = _gpu_kernel_names(lambda: h.box_head_forward(pooled, k))
    bad = [x for x in kernels + ops_seen if any(s in x.lower() for s in VENDOR)]
    assert not bad, bad
    assert any("afi_wino" in x for x in kernels) == wino, sorted(set(kernels))
    print(f"[cascade head] case {case} norm {norm!r} {'winograd' if wino else 'direct'}: library launch kinds {ran}; kernels {sorted(set(kernels))[:8]}")
    assert len(convs) == num_conv and tuple(convs[-1].shape) == (R, conv_dim, S, S) and tuple(fcs[0].shape) == (R, fc)
    assert pred.shape[1] == (K + 5 + 3) // 4 * 4 and not pred[:, K + 5:].any()
    sd = h.state_dict()
    assert (f"box_head.{k}.conv1.bias" in sd) == (norm == "") and (f"box_head.{k}.conv1.norm.running_var" in sd) == (norm != "")
    ref, c32 = Q.conv_fc_head(pooled_cpu, sd, k, torch.float64), Q.conv_fc_head(pooled_cpu, sd, k, torch.float32)
    _check_rows(f"case {case} norm {norm!r}", _chain_rows(C, S, num_conv, conv_dim, fc, K, convs, fcs, pred, ref, c32))
    # an in-place change of a running statistic (or of the bias) rebuilds the folded weights
    with torch.no_grad():
        c1 = h.box_head[k].conv1
        if norm:
            c1.norm.running_mean.add_(1000.0)                      # far below zero after the norm: conv1's ReLU output is all zero
        else:
            c1.bias.sub_(1000.0)
        _, convs2, _ = h.box_head_forward(pooled, k, intermediates=True)
        assert not convs2[0].any() and convs[0].any(), "conv1's prepared weights were not rebuilt"


# ------------------------------------------------------------------------------------------------ 3. the normed mask head
def test_normed_mask_head_against_fp64(amd):
    from test_gpu_pixgemm import _profiled
    C, S, R = 256, 14, 6
    h = Q.build_heads(amd, ["p2"], C, K=5, S=7, fc=64, num_conv=0, norm="SyncBN", stages=1, masks=True, Sm=S, mask_conv=4, seed=43).cuda()
    pooled_cpu = torch.randn((R, C, S, S), generator=torch.Generator().manual_seed(48))
    pooled = _pm(pooled_cpu)
    cls = torch.zeros((1, R), dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), R, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        h.mask_head_forward(pooled, cls, cnt)
        (probs, acts, dec), ran = _profiled(lambda: h.mask_head_forward(pooled, cls, cnt, intermediates=True))
        kernels, ops_seen = _gpu_kernel_names(lambda: h.mask_head_forward(pooled, cls, cnt))
    bad = [x for x in kernels + ops_seen if any(s in x.lower() for s in VENDOR)]
    assert not bad and ran and any("afi_wino" in x for x in kernels), (bad, ran)
    sd = {"mask_head." + k: v for k, v in h.mask_head.state_dict().items()}
    assert "mask_head.mask_fcn1.bias" not in sd and "mask_head.mask_fcn4.norm.num_batches_tracked" in sd
    (r_acts, r_dec), (c_acts, c_dec) = Q.mask_head_chain(pooled_cpu, sd, torch.float64), Q.mask_head_chain(pooled_cpu, sd, torch.float32)
    rows = [(f"mask_fcn{i + 1}", acts[i].cpu(), r_acts[i], c_acts[i], 9 * C * (i + 1)) for i in range(4)]
    rows.append(("deconv", dec.cpu(), r_dec, c_dec, 9 * C * 4 + C))
    _check_rows("normed mask head", rows)
    assert tuple(probs.shape) == (1, R, 2 * S, 2 * S) and not torch.isnan(probs).any()


# ------------------------------------------------------------------------------------------------ 4. whole heads
_WHOLE = {}


def _whole(amd, layout, stages, K, masks):
    key = (layout, stages, K, masks)
    if key not in _WHOLE:
        feats, _, _, hw = Q.WHOLE_LAYOUTS[layout]
        xs = Q.whole_features(layout)
        _WHOLE[key] = (Q.whole_heads(amd, layout, stages, K, masks).cuda(), xs, {f: _pm(x) for f, x in xs.items()},
                       torch.from_numpy(Q.whole_boxes(layout)).cuda(), torch.tensor(Q.WHOLE_COUNTS, dtype=torch.int32, device="cuda"),
                       torch.tensor(hw, device="cuda"))
    return _WHOLE[key]


def _names(masks):
    return ("boxes", "scores", "classes", "counts", "truncated") + (("mask_probs",) if masks else ())


@pytest.mark.parametrize("layout,stages,K,masks", Q.WHOLE_CASES)
def test_forward_padded_equals_the_staged_checker(amd, layout, stages, K, masks):
    from afigan_amd import ops
    from test_gpu_pixgemm import _bar, _errs
    from test_gpu_roi import _check_selection
    h, xs, feats, boxes, counts, hw = _whole(amd, layout, stages, K, masks)
    names, (fnames, _, _, _) = _names(masks), Q.WHOLE_LAYOUTS[layout]
    ml, cn, C, FC = h.box_pooler.min_level, list(Q.WHOLE_COUNTS), Q.WHOLE_C, Q.WHOLE_FC
    assert QB.align_facts(boxes.cpu().numpy(), 7, 0, ml, ml + 3, skip=0) > 1e-6
    with torch.no_grad():
        r = h.forward_padded(hw, feats, boxes, counts, intermediates=True)
        out2 = h.forward_padded(hw, feats, boxes, counts)              # (the running score updated in place here, fresh per stage above)
        torch.cuda.synchronize()
    assert len(out2) == len(names) and all(torch.equal(r[k], o) for k, o in zip(names, out2)), "two eager runs differ"
    assert len(r["stages"]) == stages and set(r["stages"][0]) == {"proposals", "pooled", "convs", "fc", "pred", "scores", "boxes"}
    sd, levels = h.state_dict(), [xs[f].numpy() for f in fnames]
    per, cur = [], boxes
    for k, st in enumerate(r["stages"]):
        assert torch.equal(st["proposals"], cur), "stage k + 1 reads stage k's clipped boxes, none dropped"
        ref, absum, terms = QB.roi_align(levels, ml, st["proposals"].cpu().numpy(), cn, 7, 0)
        err = np.abs(st["pooled"].cpu().double().numpy() - ref)
        bar = (terms[:, None, None, None] + 4) * EPS * absum
        print(f"[cascade whole] {layout} S {stages} K {K} stage {k} ROIAlign: max |err| {err.max():.3e}, max |err| / bar {float((err / np.maximum(bar, 1e-300)).max()):.3f}")
        assert (err <= bar).all()
        ref_h = Q.conv_fc_head(st["pooled"].cpu(), sd, k, torch.float64)
        for tag, got, want, ktot in [(f"conv{i + 1}", st["convs"][i], ref_h[0][i], 9 * C * (i + 1)) for i in range(2)] + \
                [("fc1", st["fc"][0], ref_h[1][0], 18 * C + 49 * C), ("cls_score", st["pred"][:, :K + 1], ref_h[2], 67 * C + FC),
                 ("bbox_pred", st["pred"][:, K + 1:K + 5], ref_h[3], 67 * C + FC)]:
            em, _ = _errs(got.cpu(), want)
            print(f"[cascade whole] {layout} S {stages} K {K} stage {k} {tag} Ktot {ktot}: max-norm {em:.2e} (bar {_bar(ktot):.2e})")
            assert em <= _bar(ktot), (k, tag, em)
        # the running score and the boxes: exact on the kernel's pred
        s_k, b_k = ops.roi_scores_boxes(st["pred"], K, True, st["proposals"], counts, hw, h.stage_weights[k])
        per.append(s_k.cpu().numpy())
        assert torch.equal(_bits(st["boxes"]), _bits(b_k[:, :, 0]))
        want = per[0]
        with np.errstate(invalid="ignore"):
            for s in per[1:]:
                want = want + s
        if k == stages - 1:
            want = Q.mean_scores(per)
        assert _same(st["scores"].cpu().numpy(), want), f"running score after stage {k}"
        s64, b64, (pcx, pcy, pw, ph) = QB.scores_boxes(st["pred"].cpu().numpy(), K, True, st["proposals"].cpu().numpy(), cn, hw.cpu().numpy(), h.stage_weights[k])
        live = np.isfinite(s64)
        assert (np.abs(per[-1].astype(np.float64)[live] - s64[live]) <= 2.0 ** -23 * s64[live]).all()
        bbar = 16 * EPS * np.stack([np.abs(pcx) + pw, np.abs(pcy) + ph, np.abs(pcx) + pw, np.abs(pcy) + ph], -1)
        assert (np.abs(b_k.cpu().double().numpy() - b64) <= bbar).all()
        cur = st["boxes"]
    assert torch.equal(_bits(r["class_scores"]), _bits(r["stages"][-1]["scores"])) and torch.equal(r["class_boxes"].reshape(2, -1, 4), cur)
    assert _same(r["class_scores"].cpu().numpy(), Q.mean_scores(per))
    for n, c in enumerate(cn):
        assert np.isneginf(r["class_scores"][n, c:].cpu().numpy()).all() and not cur[n, c:].any()
    res = _check_selection(amd, r["class_scores"], r["class_boxes"], h.test_score_thresh, h.test_nms_thresh, h.test_detections_per_img)
    assert [c for c, *_ in res] == r["counts"].tolist() and not any(t for _, t, *_ in res)
    valid, kept = (r["cand"]["valid"] != 0).sum(1).tolist(), (r["keep"] != 0).sum(1).tolist()
    print(f"[cascade whole] {layout} S {stages} K {K}: valid candidates {valid}, kept {kept}, detections {r['counts'].tolist()}")
    for v, kp in zip(valid, kept):
        assert v >= 3 and 0.1 * v <= kp <= 0.9 * v, (valid, kept)
    # forward == forward_padded; forward_with_given_boxes on the same boxes and classes gives the same masks bit for bit
    from afigan_amd.roi_heads import Detections
    from afigan_amd.rpn import Boxes, Proposals
    sizes = [(int(a), int(b)) for a, b in hw.tolist()]
    images = type("Images", (), {"image_sizes": sizes, "__len__": lambda s: 2})()
    props = [Proposals(sz, Boxes(boxes[n, :c]), torch.zeros(c, device="cuda")) for n, (sz, c) in enumerate(zip(sizes, cn))]
    with torch.no_grad():
        results, losses = h(images, feats, props)
    assert losses == {} and len(results) == 2
    for n, d in enumerate(results):
        c = int(r["counts"][n])
        assert len(d) == c and c > 0 and d.pred_classes.dtype == torch.int64 and tuple(d.image_size) == sizes[n]
        assert torch.equal(d.pred_boxes.tensor, r["boxes"][n, :c]) and torch.equal(d.scores, r["scores"][n, :c])
        assert torch.equal(d.pred_classes, r["classes"][n, :c].long())
    if masks:
        Sm = h.mask_pooler.output_size
        with torch.no_grad():
            given = [Detections(d.image_size, d.pred_boxes, d.scores, d.pred_classes) for d in results]
            assert h.forward_with_given_boxes(feats, given) is given
        for n, (d, gv) in enumerate(zip(results, given)):
            c = int(r["counts"][n])
            assert tuple(d.pred_masks.shape) == (c, 1, 2 * Sm, 2 * Sm) and torch.equal(d.pred_masks[:, 0], out2[5][n, :c])
            assert torch.equal(gv.pred_masks, d.pred_masks), "forward_with_given_boxes differs from forward_padded on the same boxes and classes"
            assert bool(d.pred_masks.flatten(1).any(1).all()) and not out2[5][n, c:].any()
        # the normed mask head on the kernel's pooled features, conv by conv
        import mask_f64 as QM
        msd = h.mask_head.state_dict()
        x = r["mask_pooled"]
        for i, a in enumerate(r["mask_convs"]):
            q = f"mask_fcn{i + 1}"
            em, _ = _errs(a.cpu(), Q.conv_norm_relu(x.cpu(), msd[q + ".weight"], None, Q.norm_of(msd, q)))
            assert em <= _bar(9 * C), (i, em)
            x = a
        em, _ = _errs(r["mask_deconv"].cpu(), QM.deconv_phases(x, msd["deconv.weight"], msd["deconv.bias"]))
        assert em <= _bar(C), em


@pytest.mark.parametrize("layout,stages,K,masks", Q.WHOLE_CASES[:2])
def test_hipgraph_replay_is_bit_identical_and_no_vendor_kernel_runs(amd, layout, stages, K, masks):
    h, xs, feats, boxes, counts, hw = _whole(amd, layout, stages, K, masks)
    names = _names(masks)
    with torch.no_grad():
        eager = h.forward_padded(hw, feats, boxes, counts)
        again = h.forward_padded(hw, feats, boxes, counts)
    assert all(torch.equal(a, b) for a, b in zip(eager, again)), "two eager runs differ"
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
        differ = [k for k, t, e in zip(names, gr, eager) if not torch.equal(t, e)]
        assert not differ, f"the hipGraph replay differs from the eager run in {differ}"
    with torch.no_grad():
        kernels, ops_seen = _gpu_kernel_names(lambda: h.forward_padded(hw, feats, boxes, counts))
    bad = [x for x in kernels + ops_seen if any(s in x.lower() for s in VENDOR)]
    assert not bad, bad
    assert sum("afi_roi_cascade_stage" in x for x in kernels) == stages and not any("afi_roi_scores_boxes" in x for x in kernels), sorted(set(kernels))


def test_forward_raises_when_truncated(amd):
    """More than M = 1024 class scores above the threshold and fewer than D kept: forward refuses by name, as StandardROIHeads' does."""
    feats_n = Q.WHOLE_LAYOUTS["fpn"][0]
    h = Q.build_heads(amd, feats_n, Q.WHOLE_C, K=3, S=7, fc=Q.WHOLE_FC, num_conv=2, norm="SyncBN", stages=3, thresh=0.0, D=1000, seed=51).cuda()
    feats = {f: _pm(x) for f, x in Q.whole_features("fpn").items()}
    P, K = 400, 3
    big = torch.zeros((2, P, 4), device="cuda")
    big[:] = torch.tensor([10.0, 10.0, 50.0, 50.0], device="cuda")
    cnt = torch.tensor([P, P], dtype=torch.int32, device="cuda")
    hw = torch.tensor(Q.WHOLE_LAYOUTS["fpn"][3], device="cuda")
    with torch.no_grad():
        for pr in h.box_predictor:
            pr.bbox_pred.weight.zero_()
            pr.bbox_pred.bias.zero_()
        out = h.forward_padded(hw, feats, big, cnt)
    assert out[4].tolist() == [1, 1] and max(out[3].tolist()) <= K
    from afigan_amd.rpn import Boxes, Proposals
    images = type("Images", (), {"image_sizes": [(64, 80), (60, 77)], "__len__": lambda s: 2})()
    props = [Proposals(sz, Boxes(big[n]), torch.zeros(P, device="cuda")) for n, sz in enumerate(images.image_sizes)]
    with torch.no_grad(), pytest.raises(amd.AfiError, match=r"SCORE_THRESH_TEST.*1024|1024.*SCORE_THRESH_TEST"):
        h(images, feats, props)


@pytest.mark.parametrize("masks", [False, True])
def test_detector_inference_returns_instances(amd, masks):
    from afigan_amd.fpn_sr import ShapeSpec
    from test_gpu_rpn import _rpn
    levels4 = ["p2", "p3", "p4", "p5"]

    class Backbone(torch.nn.Module):
        size_divisibility = 32

        def output_shape(self):
            return {f: ShapeSpec(channels=32, stride=2 ** int(f[1:])) for f in levels4}

        def forward(self, x):
            return {f: torch.nn.functional.avg_pool2d(x, 2 ** int(f[1:])).repeat(1, 11, 1, 1)[:, :32].contiguous() for f in levels4}

    bb = Backbone()
    rpn = _rpn(amd, levels4, 32, (32, 64, 128, 256), pre_k=300, post_k=100, seed=9)
    heads = Q.build_heads(amd, levels4, 32, K=5, S=7, fc=64, num_conv=1, conv_dim=16, norm="SyncBN", stages=3, masks=masks, mask_conv=1, D=100,
                          seed=61, box_scale=1.0).cuda()
    if masks:
        with torch.no_grad():
            heads.mask_head.predictor.bias.fill_(0.3)             # so that some pixels are set
    det = amd.GeneralizedRCNN_AFExtractor(backbone=bb, proposal_generator=rpn, roi_heads=heads, pixel_mean=[100.0, 110.0, 120.0],
                                          pixel_std=[50.0, 55.0, 60.0]).eval()
    assert {k for k in det.state_dict() if k.startswith("roi_heads.")} == {"roi_heads." + k for k in heads.state_dict()}
    g = torch.Generator().manual_seed(61)
    inputs = [{"image_x0.5": torch.rand((3, 64, 80), generator=g) * 255, "height": 128, "width": 160},
              {"image_x0.5": torch.rand((3, 57, 71), generator=g) * 255, "height": 114, "width": 142}]
    with torch.no_grad():
        out = det.inference(inputs)
    assert len(out) == 2 and all(set(o) == {"instances"} for o in out)
    total = pixels = 0
    for o, inp in zip(out, inputs):
        r = o["instances"]
        t = r.pred_boxes.tensor
        n = len(t)
        assert tuple(r.image_size) == (inp["height"], inp["width"]) and t.is_cuda and t.shape[1] == 4 and n <= 100
        assert r.scores.shape == (n,) and r.pred_classes.dtype == torch.int64 and len(r.pred_classes) == n
        assert bool((t >= 0).all()) and bool((t[:, 0::2] <= inp["width"]).all()) and bool((t[:, 1::2] <= inp["height"]).all())
        if masks:
            m = r.pred_masks
            assert m.dtype == torch.bool and m.is_cuda and tuple(m.shape) == (n, inp["height"], inp["width"])
            pixels += int(m.sum())
        else:
            assert getattr(r, "pred_masks", None) is None
        total += n
    assert total > 0, "no detection at all: the test would show nothing"
    assert not masks or pixels > 0, "no mask pixel at all: the test would show nothing"
