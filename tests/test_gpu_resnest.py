"""The frozen ResNeSt bottom-up (afigan_amd/resnest_backbone.py) and its kernels on the GPU, against fp64 CPU restatements written here with
torch.nn.functional: F.conv2d (groups=2 for the split-attention conv), the norm affine, F.avg_pool2d (3, 2, 1 for AVD; 2, 2, ceil_mode,
count_include_pad=False for avg_down), F.max_pool2d(3, 2, 1), F.softmax over the radix pair, and detectron2-ResNeSt's block order.  Weights
are random, scaled so the activations stay O(1) (each block's conv3 damped).  Every network figure is also taken for a CPU fp32 run of the
same restatement, and the ratio of the two errors is printed."""
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


def _max_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def _pm(t):
    """a CPU NCHW tensor as a pixel-major fp32 GPU tensor"""
    return t.float().cuda().contiguous(memory_format=torch.channels_last)


def _fill(model, seed):
    """Random weights, biases and norm statistics with O(1) activations through the whole network."""
    from afigan_amd import resnet_guide
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, resnet_guide.Conv2d):
                cout, cin, k, _ = m.weight.shape
                gain = 0.25 if name.endswith("conv3") else (0.5 if "fpn_" in name else 1.0)
                if name.endswith("stem.conv1_1"):
                    gain = 1.0 / 58.0                              # the input is (pixel - mean) / 1: the 0..255 range
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * gain * math.sqrt(2.0 / (cin * k * k)))
                if m.bias is not None:
                    m.bias.copy_(torch.randn(cout, generator=g) * 0.1)
            elif hasattr(m, "running_var"):
                c = m.running_var.shape[0]
                m.weight.copy_(torch.rand(c, generator=g) * 0.4 + 0.8)
                m.bias.copy_(torch.randn(c, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(c, generator=g) * 0.5 + 0.75)


def _t(p, d):
    return None if p is None else p.detach().cpu().to(d)


def _bn(n, y):
    d = y.dtype
    s = _t(n.weight, d) / torch.sqrt(_t(n.running_var, d) + n.eps)
    return y * s.view(1, -1, 1, 1) + (_t(n.bias, d) - _t(n.running_mean, d) * s).view(1, -1, 1, 1)


def _conv(m, x, stride=1, padding=0, groups=1, norm=None):
    y = F.conv2d(x, _t(m.weight, x.dtype), _t(m.bias, x.dtype), stride=stride, padding=padding, groups=groups)
    n = norm if norm is not None else m.norm
    return _bn(n, y) if n is not None else y


def _ref_splat(sp, x):
    """splat.py SplAtConv2d.forward (radix 2, cardinality 1) and rSoftMax."""
    y = F.relu(_conv(sp.conv, x, padding=1, groups=2, norm=sp.bn0))
    N, C = y.shape[0], sp.channels
    s0, s1 = torch.split(y, C, dim=1)
    gap = F.adaptive_avg_pool2d(s0 + s1, 1)
    h = F.relu(_conv(sp.fc1, gap, norm=sp.bn1))
    z = _conv(sp.fc2, h)
    a = F.softmax(z.view(N, 1, 2, -1).transpose(1, 2), dim=1).reshape(N, -1).view(N, -1, 1, 1)
    a0, a1 = torch.split(a, C, dim=1)
    return a0 * s0 + a1 * s1


def _ref_bottom_up(bu, x):
    """detectron2-ResNeSt's ResNet(BasicStem(deep_stem), BottleneckBlock(radix 2, avd, avg_down)) restated; dtype decides the arithmetic."""
    st = bu.stem
    y = F.relu(_conv(st.conv1_1, x, stride=2, padding=1))
    y = F.relu(_conv(st.conv1_2, y, padding=1))
    y = F.relu(_conv(st.conv1_3, y, padding=1))
    y = F.max_pool2d(y, kernel_size=3, stride=2, padding=1)
    feats = {}
    for name in bu.stage_names:
        for blk in getattr(bu, name):
            t = F.relu(_conv(blk.conv1, y))
            t = _ref_splat(blk.conv2, t)
            if blk.avd:
                t = F.avg_pool2d(t, 3, blk.stride, padding=1)
            t = _conv(blk.conv3, t)
            if blk.shortcut is not None:
                s = F.avg_pool2d(y, blk.stride, blk.stride, ceil_mode=True, count_include_pad=False)
                s = _conv(blk.shortcut, s)
            else:
                s = y
            y = F.relu(t + s)
        feats[name] = y
    return feats


def _ref_fpn(bb, feats):
    xs = [feats[k] for k in bb.in_features[::-1]]
    prev = _conv(bb.lateral_convs[0], xs[0])
    outs = [_conv(bb.output_convs[0], prev, padding=1)]
    for f, lat, out in zip(xs[1:], bb.lateral_convs[1:], bb.output_convs[1:]):
        prev = _conv(lat, f) + F.interpolate(prev, scale_factor=2.0, mode="nearest")
        outs.insert(0, _conv(out, prev, padding=1))
    outs.append(F.max_pool2d(outs[-1], kernel_size=1, stride=2, padding=0))
    return dict(zip([f"p{i}" for i in range(2, 7)], outs))


def _cfg(amd, depth, norm, guide=True):
    cfg = amd.get_cfg()
    m = {"RESNETS": {"DEPTH": depth, "OUT_FEATURES": list(IN_FEATURES), "RADIX": 2, "STRIDE_IN_1X1": False, "NORM": norm},
         "FPN": {"IN_FEATURES": list(IN_FEATURES)}}
    if guide:
        m.update({"GUIDE_ARCHITECTURE": "RCNN_FPN_only", "GUIDE_BACKBONE": {"NAME": "build_resnest_fpn_backbone"}})
    cfg.merge_from_dict({"MODEL": m})
    return cfg


def _guide(amd, depth, norm, seed):
    torch.manual_seed(seed)
    m = amd.build_guide_model(_cfg(amd, depth, norm))              # (MODEL.DEVICE "cuda": RCNN_FPN_only moves itself there)
    _fill(m.backbone, seed)
    return m.eval()


def _batch(guide, images):
    from afigan_amd.rcnn_only import pad_to_batch
    return pad_to_batch([(t.double() - guide.pixel_mean.cpu().double()) / guide.pixel_std.cpu().double() for t in images], 32)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape,cout", [((1, 3, 37, 53), 32), ((2, 3, 64, 96), 64)])
def test_stem_conv_vs_fp64(amd, shape, cout):
    """afi_resnest_stem_fwd: conv 3x3/2 pad 1 (Cin 3) + folded norm + ReLU from the NCHW batch, odd and even sizes."""
    from afigan_amd import ops, resnest_backbone
    conv = resnest_backbone.Conv2d(3, cout, 3, stride=2, norm="BN")
    _fill(conv, 3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(shape, generator=g) * 3.0
    ref = F.relu(_conv(conv, x.double(), stride=2, padding=1))
    w, b = conv.fold()
    got = ops.resnest_stem(x.cuda(), w.cuda(), b.cuda())
    assert got.shape == ref.shape and ops.is_dense_pm(got)
    err = _max_rel(got, ref)
    print(f"stem conv {shape} -> {cout}: max rel err {err:.2e}")
    assert err <= 1e-5, err


@pytest.mark.parametrize("hw", [(37, 53), (64, 96), (1, 2)])
def test_pooling_modes_vs_fp64(amd, hw):
    from afigan_amd import ops
    g = torch.Generator().manual_seed(hw[0])
    x = torch.randn((2, 72) + hw, generator=g)
    xg = _pm(x)[:, 4:68]                                            # a channel view of a wider pixel-major buffer
    xd = x[:, 4:68].double()
    refs = {"max3s2p1": F.max_pool2d(xd, 3, 2, 1), "avg3s2p1": F.avg_pool2d(xd, 3, 2, 1),
            "avg2s2_ceil": F.avg_pool2d(xd, 2, 2, ceil_mode=True, count_include_pad=False)}
    for mode, ref in refs.items():
        got = ops.resnest_pool(xg, mode)
        assert got.shape == ref.shape, (mode, got.shape, ref.shape)
        err = _max_rel(got, ref)
        print(f"pool {mode} {hw}: max rel err {err:.2e}")
        assert err <= 1e-5, (mode, err)
    assert torch.equal(ops.resnest_pool(xg, "max3s2p1").cpu(), refs["max3s2p1"].float())


@pytest.mark.parametrize("hw", [(37, 53), (64, 96)])
def test_avg_pools_are_exact_on_representable_inputs(amd, hw):
    """Multiples of 1/16 in [-4, 4): every window sum is exact in fp32, so the one rounding left is the division -- as in fp64 rounded."""
    from afigan_amd import ops
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-64, 64, (2, 32) + hw, generator=g).double() / 16.0
    for mode, ref in (("avg3s2p1", F.avg_pool2d(x, 3, 2, 1)),
                      ("avg2s2_ceil", F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False))):
        assert torch.equal(ops.resnest_pool(_pm(x), mode).cpu(), ref.float()), mode


@pytest.mark.parametrize("avd", [False, True])
@pytest.mark.parametrize("C", [64, 256])
def test_split_attention_vs_fp64(amd, C, avd):
    """afi_resnest_splat_gap / _attn / _combine on an odd map, with and without the fused AVD pool, against splat.py restated in fp64."""
    from afigan_amd import ops, resnest_backbone
    sp = resnest_backbone.SplAtConv2d(C, "BN")
    _fill(sp, C)
    with torch.no_grad():
        sp.fc1.weight.mul_(3.0)                                      # attention weights well away from 1/2
        sp.fc2.weight.mul_(3.0)
    g = torch.Generator().manual_seed(C + int(avd))
    s0, s1 = torch.relu(torch.randn((2, C, 37, 29), generator=g)), torch.relu(torch.randn((2, C, 37, 29), generator=g) + 0.3)
    (_, _), (w1, b1), (w2, b2) = sp.fold()
    got, att = ops.splat_attention(_pm(s0), _pm(s1), w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda(), avd=avd)
    a0, a1 = s0.double(), s1.double()
    gap = F.adaptive_avg_pool2d(a0 + a1, 1)
    h = F.relu(_conv(sp.fc1, gap, norm=sp.bn1))
    z = _conv(sp.fc2, h).view(2, 2, C)
    a = F.softmax(z, dim=1)
    ref = a[:, 0].view(2, C, 1, 1) * a0 + a[:, 1].view(2, C, 1, 1) * a1
    if avd:
        ref = F.avg_pool2d(ref, 3, 2, 1)
    assert got.shape == ref.shape and ops.is_dense_pm(got)
    e_att, e = _rel_l2(att, a.reshape(2, 2 * C)), _rel_l2(got, ref)
    print(f"split attention C={C} avd={avd}: att rel L2 {e_att:.2e}, out rel L2 {e:.2e}; att range {a.min().item():.3f}..{a.max().item():.3f}")
    assert e_att <= 1e-5 and e <= 1e-5, (e_att, e)


# ------------------------------------------------------------------------------------------------ network
@pytest.mark.parametrize("depth,norm", [(50, "FrozenBN"), (101, "SyncBN")])
def test_guide_vs_fp64_ragged(amd, depth, norm):
    """RCNN_FPN_only over build_resnest_fpn_backbone on two ragged images: p2..p6 within 1e-3 relative L2 of fp64."""
    guide = _guide(amd, depth, norm, seed=depth)
    g = torch.Generator().manual_seed(5)
    images = [torch.rand((3, 100, 150), generator=g) * 255.0, torch.rand((3, 90, 170), generator=g) * 255.0]
    with torch.no_grad():
        got = guide([{"image": t} for t in images])[0]["features"]
        x = _batch(guide, images)
        ref = _ref_fpn(guide.backbone, _ref_bottom_up(guide.backbone.bottom_up, x))
        ref32 = _ref_fpn(guide.backbone, _ref_bottom_up(guide.backbone.bottom_up, x.float()))
    for k in ("p2", "p3", "p4", "p5", "p6"):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        e, e32 = _rel_l2(got[k], ref[k]), _rel_l2(ref32[k], ref[k])
        print(f"ResNeSt-{depth} {norm} {k}: rel L2 {e:.2e} (CPU fp32 {e32:.2e}, ratio {e / max(e32, 1e-30):.1f}); "
              f"|ref| rms {ref[k].pow(2).mean().sqrt().item():.3f}")
        assert e <= 1e-3, (k, e)


def test_guide_vs_fp64_full_size(amd):
    """ResNeSt-101 at 1 x 3 x 800 x 1344: p2..p6 within 1e-3 relative L2 of fp64."""
    guide = _guide(amd, 101, "SyncBN", seed=11)
    g = torch.Generator().manual_seed(6)
    images = [torch.rand((3, 800, 1344), generator=g) * 255.0]
    with torch.no_grad():
        got = {k: v.cpu() for k, v in guide([{"image": t} for t in images])[0]["features"].items()}
        x = _batch(guide, images)
        ref = _ref_fpn(guide.backbone, _ref_bottom_up(guide.backbone.bottom_up, x))
        ref32 = _ref_fpn(guide.backbone, _ref_bottom_up(guide.backbone.bottom_up, x.float()))
    for k in ("p2", "p3", "p4", "p5", "p6"):
        e, e32 = _rel_l2(got[k], ref[k]), _rel_l2(ref32[k], ref[k])
        print(f"800x1344 {k}: rel L2 {e:.2e} (CPU fp32 {e32:.2e}, ratio {e / max(e32, 1e-30):.1f})")
        assert e <= 1e-3, (k, e)


def test_hipgraph_capture_replays_bit_identically(amd):
    """The forward has no host synchronisation and no atomics: it captures into a hipGraph and replays bit-identically on new inputs."""
    guide = _guide(amd, 50, "BN", seed=2)
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
        again = bb(x)
    for k in eager:
        assert torch.equal(captured[k], eager2[k]), k
        assert torch.equal(again[k], eager2[k]), k
        assert not torch.equal(captured[k], eager[k]), k


def test_resnest101_pafpn_inference_backbone(amd):
    """build_resnest_pafpn_sr_backbone with the ResNeSt101-PAFPN inference config values (RESNETS.NORM and FPN.NORM SyncBN, eval, no_grad):
    p2..p6 within 1e-3 relative L2 of the same PAFPN_AFIGAN module fed the fp64 restated bottom-up's features rounded to fp32."""
    from afigan_amd import registry, resnest_backbone
    old = dict(registry._BOTTOM_UP)
    try:
        resnest_backbone.use_as_bottom_up()
        cfg = _cfg(amd, 101, "SyncBN", guide=False)
        cfg.MODEL.FPN.NORM = "SyncBN"
        cfg.MODEL.BACKBONE.NAME = "build_resnest_pafpn_sr_backbone"
        torch.manual_seed(9)
        bb = amd.BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, None)
    finally:
        registry._BOTTOM_UP.clear()
        registry._BOTTOM_UP.update(old)
    assert isinstance(bb, amd.PAFPN_AFIGAN) and isinstance(bb.bottom_up, resnest_backbone.ResNeSt)
    _fill(bb.bottom_up, 9)
    bb = bb.cuda().eval()
    g = torch.Generator().manual_seed(10)
    x = (torch.rand((2, 3, 160, 224), generator=g) * 255.0 - 120.0) / 58.0
    with torch.no_grad():
        got = bb(x.cuda())
        feats = {k: _pm(v) for k, v in _ref_bottom_up(bb.bottom_up, x.double()).items()}
        bb.bottom_up.forward = lambda _x: feats                    # the same PAFPN fed the restated features
        try:
            ref = bb(x.cuda())
        finally:
            del bb.bottom_up.forward
    for k in ("p2", "p3", "p4", "p5", "p6"):
        assert got[k].shape == ref[k].shape, k
        e = _rel_l2(got[k], ref[k])
        print(f"ResNeSt101-PAFPN {k}: rel L2 {e:.2e} against the PAFPN over the fp64 bottom-up")
        assert e <= 1e-3, (k, e)
