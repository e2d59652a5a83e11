"""The frozen ResNet-FPN guide (afigan_amd/resnet_guide.py) on the GPU against fp64 CPU restatements written here with torch.nn.functional:
F.conv2d, the FrozenBN affine, F.max_pool2d(3, 2, 1), nearest F.interpolate and detectron2's block order.  Weights are random, scaled so the
activations stay O(1) (each block's conv3 damped, as guide.py does).  Every guide figure is also taken for a CPU fp32 run of the same
restatement, and the ratio of the two errors is printed."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

IN_FEATURES = ["res2", "res3", "res4", "res5"]


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _fill(model, seed):
    """Random weights and FrozenBN statistics with O(1) activations through the whole network."""
    from afigan_amd import resnet_guide
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in model.named_modules():
            if not isinstance(m, resnet_guide.Conv2d):
                continue
            cout, cin, k, _ = m.weight.shape
            gain = 0.25 if name.endswith("conv3") else (0.5 if "fpn_" in name else 1.0)
            if name.endswith("stem.conv1"):
                gain = 1.0 / 58.0                                  # the input is (pixel - mean) / 1: the 0..255 range
            m.weight.copy_(torch.randn(m.weight.shape, generator=g) * gain * math.sqrt(2.0 / (cin * k * k)))
            if m.bias is not None:
                m.bias.copy_(torch.randn(cout, generator=g) * 0.1)
            if m.norm is not None:
                n = m.norm
                n.weight.copy_(torch.rand(cout, generator=g) * 0.4 + 0.8)
                n.bias.copy_(torch.randn(cout, generator=g) * 0.1)
                n.running_mean.copy_(torch.randn(cout, generator=g) * 0.1)
                n.running_var.copy_(torch.rand(cout, generator=g) * 0.5 + 0.75)


def _conv(m, x, stride=1, padding=0):
    d = x.dtype
    y = F.conv2d(x, m.weight.detach().cpu().to(d), None if m.bias is None else m.bias.detach().cpu().to(d), stride=stride, padding=padding)
    if m.norm is not None:
        n = m.norm
        s = n.weight.cpu().to(d) / torch.sqrt(n.running_var.cpu().to(d) + n.eps)
        y = y * s.view(1, -1, 1, 1) + (n.bias.cpu().to(d) - n.running_mean.cpu().to(d) * s).view(1, -1, 1, 1)
    return y


def _ref_stem(stem, x):
    return F.max_pool2d(F.relu(_conv(stem.conv1, x, stride=2, padding=3)), 3, 2, 1)


def _ref_backbone(bb, x):
    """detectron2's ResNet + FPN + LastLevelMaxPool, restated; x is the normalised, padded NCHW batch (dtype decides the arithmetic)."""
    bu = bb.bottom_up
    y = _ref_stem(bu.stem, x)
    feats = {}
    for name in bu.stage_names:
        for blk in getattr(bu, name):
            s = y if blk.shortcut is None else _conv(blk.shortcut, y, stride=blk.shortcut.stride)
            t = F.relu(_conv(blk.conv1, y, stride=blk.conv1.stride))
            t = F.relu(_conv(blk.conv2, t, stride=blk.conv2.stride, padding=1))
            y = F.relu(_conv(blk.conv3, t) + s)
        feats[name] = y
    xs = [feats[k] for k in bb.in_features[::-1]]
    prev = _conv(bb.lateral_convs[0], xs[0])
    outs = [_conv(bb.output_convs[0], prev, padding=1)]
    for f, lat, out in zip(xs[1:], bb.lateral_convs[1:], bb.output_convs[1:]):
        prev = _conv(lat, f) + F.interpolate(prev, scale_factor=2.0, mode="nearest")
        if bb._fuse_type == "avg":
            prev = prev / 2
        outs.insert(0, _conv(out, prev, padding=1))
    outs.append(F.max_pool2d(outs[-1], kernel_size=1, stride=2, padding=0))
    return dict(zip([f"p{i}" for i in range(2, 7)], outs))


def _guide(amd, depth=50, stride_in_1x1=True, fuse="sum", seed=0):
    cfg = amd.get_cfg()
    cfg.merge_from_dict({"MODEL": {"GUIDE_ARCHITECTURE": "RCNN_FPN_only", "RESNETS": {"DEPTH": depth, "OUT_FEATURES": list(IN_FEATURES),
                                                                                       "STRIDE_IN_1X1": stride_in_1x1},
                                   "FPN": {"IN_FEATURES": list(IN_FEATURES), "FUSE_TYPE": fuse}}})
    torch.manual_seed(seed)
    m = amd.build_guide_model(cfg)                                   # (MODEL.DEVICE "cuda": RCNN_FPN_only moves itself there)
    _fill(m.backbone, seed)
    return m.eval(), m


def _batch(guide, images):
    from afigan_amd.rcnn_only import pad_to_batch
    return pad_to_batch([(t.double() - guide.pixel_mean.cpu().double()) / guide.pixel_std.cpu().double() for t in images], 32)


@pytest.mark.parametrize("shape", [(1, 3, 37, 53), (2, 3, 64, 96)])
def test_stem_kernel_vs_fp64(amd, shape):
    """afi_resnet_stem_fwd: conv 7x7/2 + FrozenBN + ReLU + max-pool 3x3/2 in one kernel, odd and even sizes, to fp32 rounding."""
    from afigan_amd import ops, resnet_guide
    stem = resnet_guide.BasicStem()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        stem.conv1.weight.copy_(torch.randn(64, 3, 7, 7, generator=g) * 0.1)
        stem.conv1.norm.weight.copy_(torch.rand(64, generator=g) + 0.5)
        stem.conv1.norm.bias.copy_(torch.randn(64, generator=g) * 0.3)
        stem.conv1.norm.running_mean.copy_(torch.randn(64, generator=g) * 0.3)
        stem.conv1.norm.running_var.copy_(torch.rand(64, generator=g) + 0.5)
    x = torch.randn(shape, generator=g)
    ref = _ref_stem(stem, x.double())
    w, b = stem.conv1.fold()
    got = ops.resnet_stem(x.cuda(), w.cuda(), b.cuda())
    assert got.shape == ref.shape and ops.is_dense_pm(got)
    err = ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()
    print(f"stem {shape}: max rel err {err:.2e}")
    assert err <= 1e-5, err


def test_nearest_resampling_is_exact(amd):
    from afigan_amd import ops
    x = torch.randn(2, 5, 7, 64, device="cuda").permute(0, 3, 1, 2)          # pixel-major [2, 64, 5, 7]
    assert torch.equal(ops.nearest(x, up=2).cpu(), F.interpolate(x.cpu(), scale_factor=2.0, mode="nearest"))
    assert torch.equal(ops.nearest(x, up=1, down=2).cpu(), F.max_pool2d(x.cpu(), kernel_size=1, stride=2))
    assert torch.equal(ops.nearest(x[:, 8:40, 1:, :5], up=2).cpu(), F.interpolate(x[:, 8:40, 1:, :5].cpu(), scale_factor=2.0, mode="nearest"))


@pytest.mark.parametrize("depth,stride_in_1x1,fuse", [(50, True, "sum"), (50, False, "avg"), (101, True, "avg"), (101, False, "sum")])
def test_guide_vs_fp64_ragged(amd, depth, stride_in_1x1, fuse):
    """RCNN_FPN_only over the guide on two ragged images: p2..p6 within 1e-3 relative L2 of fp64."""
    guide, _ = _guide(amd, depth, stride_in_1x1, fuse, seed=depth + int(stride_in_1x1))
    g = torch.Generator().manual_seed(5)
    images = [torch.rand((3, 100, 150), generator=g) * 255.0, torch.rand((3, 90, 170), generator=g) * 255.0]
    with torch.no_grad():
        got = guide([{"image": t} for t in images])[0]["features"]
        x = _batch(guide, images)
        ref = _ref_backbone(guide.backbone, x)
        ref32 = _ref_backbone(guide.backbone, x.float())
    for k in ("p2", "p3", "p4", "p5", "p6"):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        e, e32 = _rel_l2(got[k], ref[k]), _rel_l2(ref32[k], ref[k])
        print(f"R-{depth} stride_in_1x1={stride_in_1x1} {fuse} {k}: rel L2 {e:.2e} (CPU fp32 {e32:.2e}, ratio {e / max(e32, 1e-30):.1f}); "
              f"|ref| rms {ref[k].pow(2).mean().sqrt().item():.3f}")
        assert e <= 1e-3, (k, e)


def test_guide_vs_fp64_full_size(amd):
    """2 x 3 x 800 x 1344, the stage-1 training size: p2..p6 within 1e-3 relative L2 of fp64."""
    guide, _ = _guide(amd, 50, True, "sum", seed=11)
    g = torch.Generator().manual_seed(6)
    images = [torch.rand((3, 800, 1344), generator=g) * 255.0 for _ in range(2)]
    with torch.no_grad():
        got = guide([{"image": t} for t in images])[0]["features"]
        got = {k: v.cpu() for k, v in got.items()}
        x = _batch(guide, images)
        ref = _ref_backbone(guide.backbone, x)
        ref32 = _ref_backbone(guide.backbone, x.float())
    for k in ("p2", "p3", "p4", "p5", "p6"):
        e, e32 = _rel_l2(got[k], ref[k]), _rel_l2(ref32[k], ref[k])
        print(f"800x1344 {k}: rel L2 {e:.2e} (CPU fp32 {e32:.2e}, ratio {e / max(e32, 1e-30):.1f})")
        assert e <= 1e-3, (k, e)


def test_guide_hipgraph_capture(amd):
    """The eval forward has no host synchronisation: it captures into a hipGraph and replays bit-identically on new input values."""
    guide, _ = _guide(amd, 50, True, "sum", seed=2)
    bb = guide.backbone
    x = torch.randn((2, 3, 128, 192), device="cuda")
    with torch.no_grad():
        eager = bb(x)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = bb(x)
        x.mul_(0.5).add_(0.25)                                     # new input values in the same buffer
        graph.replay()
        torch.cuda.synchronize()
        eager2 = bb(x)
    for k in eager:
        assert torch.equal(captured[k], eager2[k]), k
        assert not torch.equal(captured[k], eager[k]), k


def test_guide_pyramids_feed_a_stage1_step(amd):
    """stage1_trainer.py:320-327: the guide's pyramids for `image` and `image_x0.5` feed one Stage1Step iteration; the losses are finite."""
    guide, _ = _guide(amd, 50, True, "sum", seed=4)
    g = torch.Generator().manual_seed(8)
    data = [{"image": torch.rand((3, 128, 192), generator=g) * 255.0, "image_x0.5": torch.rand((3, 64, 96), generator=g) * 255.0},
            {"image": torch.rand((3, 120, 180), generator=g) * 255.0, "image_x0.5": torch.rand((3, 60, 90), generator=g) * 255.0}]
    with torch.no_grad():
        hr = guide(data, img_dict_name="image")[0]["features"]
        lr = guide(data, img_dict_name="image_x0.5")[0]["features"]
    levels = [f"p{i}" for i in range(2, 7)]
    torch.manual_seed(0)
    G = amd.Generator(n_residual_dense_blocks=3).cuda()
    D = amd.Discriminator().cuda()
    step = amd.Stage1Step(G, D, base_lr=1e-3, warmup_iters=0)
    step.run_step([lr[k] for k in levels], [hr[k] for k in levels])
    m = step.metrics()
    assert all(math.isfinite(v) for v in m.values()), m
    assert set(f"content_loss_p{i}" for i in range(2, 7)) <= set(m)
