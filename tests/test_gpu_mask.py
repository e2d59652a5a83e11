"""The frozen mask branch of StandardROIHeads on the GPU (afigan_amd/roi_heads.py, csrc/mask.hip) against tests/mask_f64.py, stage by stage: every
stage's checker consumes the KERNEL's previous output.  tests/test_mask_host.py proves the seeded inputs' conditions without a GPU; they are
asserted again here.  Float outputs start NaN-filled and the paste's output 0xFF-filled: every element has to be written.

Bars.  afi_roi_mask_probs: the logit is C products summed in fp32 in any order plus the bias add, each operation within 2^-24 relative of its
running magnitude <= sum |w h| + |b|, so |err| <= (C + 6) 2^-24 (sum |w h| + |b|); the sigmoid's slope is at most 1/4 and it is rounded once:
0.25 (logit bar) + 2^-24.  The convs and the deconv: test_gpu_pixgemm.py's _bar / R_L2 with Ktot accumulating through the chain.  The paste:
exact equality of every pixel the checker decides (|v - 0.5| > e = 8 2^-24 sum |w m|), and of every pixel whose centre is outside its box.
"""
import math

import numpy as np
import pytest
import torch

import mask_f64 as Q
import roi_f64 as QB

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
LEVELS4 = ["p2", "p3", "p4", "p5"]


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


def _pm(x):
    """CPU NCHW -> GPU tensor whose memory is [N][H][W][C]"""
    N, C_, H, W = x.shape
    flat = x.permute(0, 2, 3, 1).reshape(-1).cuda()
    return flat.as_strided((N, C_, H, W), (H * W * C_, 1, W * C_, C_))


def _heads(amd, features, channels, K=80, S=7, fc=64, Sm=14, num_conv=4, conv_dim=None, agnostic_mask=False, thresh=0.05, D=100, seed=0):
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": True,
                               "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": list(features), "NUM_CLASSES": K, "SCORE_THRESH_TEST": thresh},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "FC_DIM": fc, "POOLER_RESOLUTION": S},
                               "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": num_conv, "CONV_DIM": conv_dim or channels,
                                                 "POOLER_RESOLUTION": Sm, "CLS_AGNOSTIC_MASK": agnostic_mask}})
    cfg.TEST.DETECTIONS_PER_IMAGE = D
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=2 ** int(f[1:])) for f in features}, masks=True)
    g = torch.Generator().manual_seed(seed)
    for name, p in h.named_parameters():
        if name.endswith("weight"):
            fan_in = p[0].numel() if "deconv" not in name else p.shape[0]
            scale = {"cls_score": 3.0, "bbox_pred": 2.0, "predictor": 3.0}.get(name.split(".")[-2], 1.4)
            p.copy_(torch.randn(p.shape, generator=g) * scale / math.sqrt(fan_in))
        else:
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return h.cuda().eval()


def _gpu_kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")], [e.key for e in prof.key_averages()]


VENDOR = ("miopen", "cijk", "hipblas", "rocblas", "aten::mm", "aten::addmm", "aten::linear", "aten::matmul", "aten::conv", "aten::_conv",
          "aten::cudnn", "aten::miopen", "grid_sample", "grid_sampler", "aten::sigmoid", "conv_transpose")


# ------------------------------------------------------------------------------------------------ 1. afi_roi_mask_probs
def _check_probs(h_np, w, b, cls, counts, got):
    """got [10, 2S, 2S] against the checker on the same h; returns (worst logit-bar ratio seen through the sigmoid, max |err|)."""
    z, mag, live = Q.selected_logits(h_np, w, b, cls, counts)
    C = w.shape[1]
    bar = 0.25 * (C + 6) * EPS * mag + EPS
    err = np.abs(got.astype(np.float64) - Q.sigmoid(z))
    assert not np.isnan(got).any() and not got[~live].any(), "rows past counts must be exactly zero"
    assert (err[live] <= bar[live]).all(), float((err[live] / bar[live]).max())
    return float((err[live] / bar[live]).max()) if live.any() else 0.0, float(err[live].max()) if live.any() else 0.0


@pytest.mark.parametrize("counts", Q.PROBS_COUNTS)
@pytest.mark.parametrize("Km", [80, 3, 1])
@pytest.mark.parametrize("C,S", [(8, 14), (256, 14), (8, 3), (256, 3)])
def test_mask_probs_against_fp64(amd, C, S, Km, counts):
    from afigan_amd import ops
    h_np, w, b, cls = Q.probs_case(C, S, Km)
    assert cls.min() == 0 and cls.max() == Km - 1
    h = _pm(torch.from_numpy(h_np))
    out = torch.full((10, 2 * S, 2 * S), float("nan"), device="cuda")
    got = ops.roi_mask_probs(h, torch.from_numpy(w).cuda().view(Km, C, 1, 1), torch.from_numpy(b).cuda(), torch.from_numpy(cls).cuda(),
                             torch.tensor(counts, dtype=torch.int32, device="cuda"), out=out)
    assert got is out
    worst, emax = _check_probs(h_np, w, b, cls, counts, got.cpu().numpy())
    print(f"[mask probs] C {C} S {S} Km {Km} counts {counts}: max |err| {emax:.3e}, max |err| / bar {worst:.3f}")


def test_mask_probs_class_out_of_range_and_refusals(amd):
    from afigan_amd import ops
    C, S, Km = 8, 3, 3
    h_np, w, b, cls = Q.probs_case(C, S, Km)
    cls = cls.copy()
    cls[0, 1], cls[0, 3], cls[1, 0] = -1, Km, 2 ** 30
    out = torch.full((10, 2 * S, 2 * S), float("nan"), device="cuda")
    got = ops.roi_mask_probs(_pm(torch.from_numpy(h_np)), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(cls).cuda(),
                             torch.tensor([5, 5], dtype=torch.int32, device="cuda"), out=out).cpu().numpy()
    _check_probs(h_np, w, b, cls, (5, 5), got)
    assert not got[1].any() and not got[3].any() and not got[5].any() and got[0].any() and got[6].any()
    hh, cc, cn = _pm(torch.zeros((2, 16, 2, 2))), torch.zeros((1, 2), dtype=torch.int32, device="cuda"), torch.ones((1,), dtype=torch.int32, device="cuda")
    with pytest.raises(amd.AfiError):
        ops.roi_mask_probs(hh, torch.zeros((3, 8), device="cuda"), torch.zeros(3, device="cuda"), cc, cn)            # 4 C != 16
    with pytest.raises(amd.AfiError):
        ops.roi_mask_probs(hh, torch.zeros((3, 4), device="cuda"), torch.zeros(2, device="cuda"), cc, cn)            # bias length
    with pytest.raises(amd.AfiError):
        ops.roi_mask_probs(_pm(torch.zeros((2, 16, 15, 15))), torch.zeros((3, 4), device="cuda"), torch.zeros(3, device="cuda"), cc, cn)
    with pytest.raises(amd.AfiError):
        ops.roi_mask_probs(hh, torch.zeros((3, 4), device="cuda"), torch.zeros(3, device="cuda"), cc.long(), cn)


# ------------------------------------------------------------------------------------------------ 2. the convs and the deconv
@pytest.mark.parametrize("C,R", [(256, 6), (256, 2), (16, 6)])
def test_convs_and_deconv_against_fp64(amd, C, R):
    from test_gpu_pixgemm import R_L2, _bar, _errs, _profiled
    S = 14
    h = _heads(amd, ["p2"], C, K=5, Sm=S, num_conv=4, seed=41)
    g = torch.Generator().manual_seed(42 + R)
    pooled_cpu = torch.randn((R, C, S, S), generator=g)
    pooled = _pm(pooled_cpu)
    cls = torch.zeros((1, R), dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), R, dtype=torch.int32, device="cuda")
    wino = C >= 128 and R * S * S >= 1024
    assert wino == (C == 256 and R == 6), "R = 6 at C = 256 takes the Winograd form, the other cases the direct form"
    with torch.no_grad():
        h.mask_head_forward(pooled, cls, cnt)                  # warm-up: scratch registration, the prepared weights
        (probs, acts, dec), ran = _profiled(lambda: h.mask_head_forward(pooled, cls, cnt, intermediates=True))
        assert ran, "the mask head did not run on the library's pixel GEMMs"
        kernels, ops_seen = _gpu_kernel_names(lambda: h.mask_head_forward(pooled, cls, cnt))
    bad = [k for k in kernels + ops_seen if any(s in k.lower() for s in VENDOR)]
    assert not bad, bad
    print(f"[mask head] C {C} R {R}: library launch kinds {ran}; GPU kernels in the trace: {sorted(set(kernels))[:8]}")
    sd = {"mask_head." + k: v for k, v in h.mask_head.state_dict().items()}
    r_acts, r_dec = Q.head_chain(pooled_cpu, sd, torch.float64)
    c_acts, c_dec = Q.head_chain(pooled_cpu, sd, torch.float32)
    assert len(acts) == 4 and tuple(dec.shape) == (R, 4 * C, S, S) and dec.permute(0, 2, 3, 1).is_contiguous()
    rows = [(f"mask_fcn{i + 1}", acts[i].cpu(), r_acts[i], c_acts[i], 9 * C * (i + 1)) for i in range(4)]
    rows.append(("deconv", dec.cpu(), r_dec, c_dec, 9 * C * 4 + C))
    fails = []
    for tag, got, ref, c32, ktot in rows:
        assert not torch.isnan(got).any()
        em, el = _errs(got, ref)
        cm, cl = _errs(c32, ref)
        bar, l2bar = _bar(ktot), R_L2 * max(cl, math.sqrt(ktot) * EPS / 8)
        print(f"[mask head] C {C} R {R} {'winograd' if wino else 'direct'} {tag} Ktot {ktot}: max-norm {em:.2e} (cpu fp32 {cm:.2e}, bar {bar:.2e})  "
              f"rel-L2 {el:.2e} (cpu fp32 {cl:.2e}, bar {l2bar:.2e})")
        if not (em <= bar and el <= l2bar):
            fails.append((tag, em, bar, el, l2bar))
    assert not fails, fails
    # the deconv alone on the kernel's own input: Ktot = C
    d_ref = Q.deconv_phases(acts[-1].cpu(), sd["mask_head.deconv.weight"], sd["mask_head.deconv.bias"])
    em, el = _errs(dec.cpu(), d_ref)
    print(f"[mask head] C {C} R {R} deconv on the kernel's input, Ktot {C}: max-norm {em:.2e} (bar {_bar(C):.2e})")
    assert em <= _bar(C)
    # an in-place parameter change rebuilds the prepared weights
    with torch.no_grad():
        h.mask_head.deconv.bias.add_(1.0)
        _, _, d2 = h.mask_head_forward(pooled, cls, cnt, intermediates=True)
        assert torch.allclose(d2[dec > 0].cpu(), dec[dec > 0].cpu() + 1.0, atol=1e-4)
        h.mask_head.mask_fcn1.weight.zero_()
        _, a3, _ = h.mask_head_forward(pooled, cls, cnt, intermediates=True)
        want = torch.relu(h.mask_head.mask_fcn1.bias).view(1, C, 1, 1).expand(R, C, S, S)
        assert torch.equal(a3[0], want), "mask_fcn1's prepared weight was not rebuilt"


# ------------------------------------------------------------------------------------------------ 3. the paste
@pytest.mark.parametrize("H,W,M", Q.PASTE_CASES)
def test_paste_against_fp64(amd, H, W, M):
    from afigan_amd import ops
    probs, boxes = Q.paste_case(H, W, M)
    R = len(boxes)
    v, e, inside = Q.paste(probs, boxes, H, W)
    want, sure = Q.paste_decided(v, e, inside)
    left_out = int((~sure).sum())
    assert left_out <= Q.PASTE_LEFT_OUT * inside.sum(), (left_out, int(inside.sum()))
    assert not any(set(np.unique(p)) == {0.5} for p in probs)
    # the output sits one byte into a 0xFF-filled buffer: rows start at odd addresses, and the bytes around it must stay
    buf = torch.full((R * H * W + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    for off in (0, 1):
        buf.fill_(0xFF)
        out = buf[32 + off:32 + off + R * H * W].view(R, H, W)
        got = ops.mask_paste(torch.from_numpy(probs).cuda(), torch.from_numpy(boxes).cuda(), (H, W), 0.5, out=out)
        assert got.dtype == torch.bool and got.data_ptr() == out.data_ptr()
        raw = out.cpu().numpy()
        assert set(np.unique(raw)) <= {0, 1}, "every byte is written, as 0 or 1"
        assert bool((buf[:32 + off] == 0xFF).all()) and bool((buf[32 + off + R * H * W:] == 0xFF).all()), "bytes outside the output were written"
        g = raw.astype(bool)
        assert not g[~inside].any(), "a pixel whose centre is outside its box is set"
        wrong = int((g != want)[sure].sum())
        print(f"[mask paste] {H}x{W} M {M} offset {off}: {int(inside.sum())} inside pixels, {left_out} undecided, {int(g.sum())} set, {wrong} wrong")
        assert wrong == 0
    fresh = ops.mask_paste(torch.from_numpy(probs).cuda(), torch.from_numpy(boxes).cuda(), (H, W))
    assert np.array_equal(fresh.cpu().numpy(), g) and fresh.dtype == torch.bool
    assert amd.paste_masks_in_image(torch.from_numpy(probs).cuda()[:, None], torch.from_numpy(boxes).cuda(), (H, W)).equal(fresh)
    assert ops.mask_paste(torch.zeros((0, M, M), device="cuda"), torch.zeros((0, 4), device="cuda"), (H, W)).shape == (0, H, W)


def test_paste_refusals(amd):
    from afigan_amd import ops
    p, b = torch.zeros((2, 28, 28), device="cuda"), torch.zeros((2, 4), device="cuda")
    with pytest.raises(amd.AfiError):
        ops.mask_paste(torch.zeros((2, 65, 65), device="cuda"), b, (8, 8))
    with pytest.raises(amd.AfiError):
        ops.mask_paste(p, b[:1], (8, 8))
    with pytest.raises(amd.AfiError):
        ops.mask_paste(p, b, (0, 8))
    with pytest.raises(amd.AfiError):
        ops.mask_paste(p, b, (8, 8), out=torch.zeros((2, 8, 8), device="cuda"))


# ------------------------------------------------------------------------------------------------ 4. the whole branch
def _whole_case(amd):
    h = _heads(amd, LEVELS4, 16, K=5, S=7, fc=64, Sm=14, num_conv=2, D=20, seed=51)
    g = torch.Generator().manual_seed(52)
    xs = {f: torch.randn((2, 16, hh, ww), generator=g) for f, (hh, ww) in zip(LEVELS4, QB.ALIGN_LEVELS)}
    boxes = torch.from_numpy(QB.align_boxes(seed=6)).cuda()
    boxes[..., 0::2] = boxes[..., 0::2].clamp(0, 80)
    boxes[..., 1::2] = boxes[..., 1::2].clamp(0, 64)
    counts = torch.tensor([37, 40], dtype=torch.int32, device="cuda")
    hw = torch.tensor([(64.0, 80.0), (60.0, 77.0)], device="cuda")
    return h, xs, {f: _pm(x) for f, x in xs.items()}, boxes, counts, hw


def test_forward_padded_with_masks_equals_the_staged_checker_and_is_deterministic(amd):
    from test_gpu_pixgemm import _bar, _errs
    h, xs, feats, boxes, counts, hw = _whole_case(amd)
    with torch.no_grad():
        r = h.forward_padded(hw, feats, boxes, counts, intermediates=True)
        out2 = h.forward_padded(hw, feats, boxes, counts)
        torch.cuda.synchronize()
    names = ("boxes", "scores", "classes", "counts", "truncated", "mask_probs")
    assert len(out2) == 6 and all(torch.equal(r[k], o) for k, o in zip(names, out2)), "two eager runs differ"
    N, D, S, C = 2, 20, 14, 16
    masks = out2[5]
    assert tuple(masks.shape) == (N, D, 2 * S, 2 * S)
    cn = r["counts"].tolist()
    assert all(c > 0 for c in cn)
    for n in range(N):
        assert not masks[n, cn[n]:].any() and bool(masks[n, :cn[n]].flatten(1).any(1).all())
    # stage by stage on the kernels' intermediates
    ref, absum, terms = QB.roi_align([xs[f].numpy() for f in LEVELS4], 2, r["boxes"].cpu().numpy(), cn, S, 0)
    assert torch.equal(h.mask_features(feats, r["boxes"], r["counts"]), r["mask_pooled"])
    assert (np.abs(r["mask_pooled"].cpu().double().numpy() - ref) <= (terms[:, None, None, None] + 4) * EPS * absum).all()
    sd = h.mask_head.state_dict()
    x = r["mask_pooled"]
    for i, a in enumerate(r["mask_convs"]):
        em, _ = _errs(a.cpu(), Q.conv_relu(x, sd[f"mask_fcn{i + 1}.weight"], sd[f"mask_fcn{i + 1}.bias"]))
        assert em <= _bar(9 * C), (i, em)
        x = a
    em, _ = _errs(r["mask_deconv"].cpu(), Q.deconv_phases(x, sd["deconv.weight"], sd["deconv.bias"]))
    assert em <= _bar(C), em
    _check_probs(r["mask_deconv"].cpu().numpy(), sd["predictor.weight"].cpu().numpy().reshape(5, C), sd["predictor.bias"].cpu().numpy(),
                 r["classes"].cpu().numpy(), cn, masks.reshape(N * D, 2 * S, 2 * S).cpu().numpy())
    # forward's pred_masks, and forward_with_given_boxes on the same boxes and classes
    from afigan_amd.roi_heads import Detections
    from afigan_amd.rpn import Boxes, Proposals
    images = type("Images", (), {"image_sizes": [(64, 80), (60, 77)], "__len__": lambda s: 2})()
    props = [Proposals(sz, Boxes(boxes[n, :c]), torch.zeros(c, device="cuda")) for n, (sz, c) in enumerate(zip(images.image_sizes, counts.tolist()))]
    with torch.no_grad():
        results, losses = h(images, feats, props)
        given = [Detections(d.image_size, d.pred_boxes, d.scores, d.pred_classes) for d in results]
        back = h.forward_with_given_boxes(feats, given)
    assert losses == {} and back is given
    for n, (d, gv) in enumerate(zip(results, given)):
        assert len(d) == cn[n] and tuple(d.pred_masks.shape) == (cn[n], 1, 2 * S, 2 * S) and d.pred_masks.dtype == torch.float32
        assert torch.equal(d.pred_masks[:, 0], masks[n, :cn[n]]) and torch.equal(d.pred_boxes.tensor, r["boxes"][n, :cn[n]])
        assert torch.equal(gv.pred_masks, d.pred_masks), "forward_with_given_boxes differs from forward on the same boxes and classes"
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
    # no torch or vendor conv, GEMM or grid-sample kernel
    with torch.no_grad():
        kernels, ops_seen = _gpu_kernel_names(lambda: (h.forward_padded(hw, feats, boxes, counts),
                                                       amd.paste_masks_in_image(masks[0, :cn[0]], r["boxes"][0, :cn[0]], (64, 80))))
    bad = [k for k in kernels + ops_seen if any(s in k.lower() for s in VENDOR + ("softmax", "aten::sort", "aten::topk"))]
    assert not bad, bad
    assert any("afi_roi_mask_probs" in k for k in kernels) and any("afi_mask_paste" in k for k in kernels), sorted(set(kernels))


def test_detector_inference_returns_pasted_masks(amd):
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
    heads = _heads(amd, LEVELS4, 32, K=5, S=7, fc=64, Sm=14, num_conv=1, conv_dim=16, seed=61)
    g = torch.Generator().manual_seed(61)
    with torch.no_grad():
        heads.box_predictor.cls_score.weight.copy_(torch.randn(heads.box_predictor.cls_score.weight.shape, generator=g))
        heads.box_predictor.bbox_pred.weight.copy_(torch.randn(heads.box_predictor.bbox_pred.weight.shape, generator=g) * 0.3)
        heads.mask_head.predictor.bias.fill_(0.3)              # so that some pixels are set
    det = amd.GeneralizedRCNN_AFExtractor(backbone=bb, proposal_generator=rpn, roi_heads=heads, pixel_mean=[100.0, 110.0, 120.0],
                                          pixel_std=[50.0, 55.0, 60.0]).eval()
    assert {k for k in det.state_dict() if k.startswith("roi_heads.mask_head.")} == {"roi_heads.mask_head." + k for k in heads.mask_head.state_dict()}
    inputs = [{"image_x0.5": torch.rand((3, 64, 80), generator=g) * 255, "height": 128, "width": 160},
              {"image_x0.5": torch.rand((3, 57, 71), generator=g) * 255, "height": 114, "width": 142}]
    with torch.no_grad():
        out = det.inference(inputs)
        raw = det.inference(inputs, do_postprocess=False)
    total = 0
    for o, rw, inp in zip(out, raw, inputs):
        r = o["instances"]
        t, m = r.pred_boxes.tensor, r.pred_masks
        n = len(t)
        assert m.dtype == torch.bool and m.is_cuda and tuple(m.shape) == (n, inp["height"], inp["width"])
        assert tuple(rw.pred_masks.shape) == (len(rw.pred_boxes.tensor), 1, 28, 28) and rw.pred_masks.dtype == torch.float32
        assert r.scores.shape == (n,) and len(r.pred_classes) == n
        ys = torch.arange(inp["height"], device="cuda").view(1, -1, 1) + 0.5
        xs = torch.arange(inp["width"], device="cuda").view(1, 1, -1) + 0.5
        b = t.view(n, 4, 1, 1)
        inbox = (xs >= b[:, 0]) & (xs <= b[:, 2]) & (ys >= b[:, 1]) & (ys <= b[:, 3])
        assert not bool((m & ~inbox).any()), "a mask pixel is set outside its box"
        total += int(m.sum())
    assert total > 0, "no mask pixel at all: the test would show nothing"
