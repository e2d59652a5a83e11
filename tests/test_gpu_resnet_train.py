"""The trainable ResNet bottom-up on the GPU against float64: the data gradients with the ReLU form of the mask (every epilogue body),
afi_frozen_wgrad_unfold, single blocks, whole networks with fused and unfused masks, determinism, and the bottom-up under the AFI FPN and the
detector.  Reference and fixtures: tests/resnet_train_f64.py (their conditions are asserted on the CPU by test_resnet_train_host.py).

Bars.  The masked data gradients: those of tests/test_gpu_pixgemm.py for the unmasked ops (max-norm 2 sqrt(Ktot) eps, capped; rel. L2 4 x max(torch
CPU fp32's, sqrt(Ktot) eps / 8)) on the live elements, exact zeros elsewhere; the Winograd form: tests/wino_f64.py's.  The unfold: 2^-24 (|s dw'| +
|grad|) per element.  Blocks and networks: 4 x the relative-L2 deviation of torch CPU fp32 autograd from fp64, per tensor."""
import math

import pytest
import torch
import torch.nn.functional as F

import resnet_train_f64 as R
import wino_f64 as wf

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
NAN = float("nan")


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _pm(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _mask_values(shape, seed):
    """an activation with +0.0, -0.0, negatives and a positive subnormal among ordinary values"""
    z = _rand(shape, seed)
    f = z.flatten()
    f[0::7], f[1::7], f[2::7] = 0.0, -0.0, 1e-40
    return z


def _bar(ktot):
    return min(2.0 * math.sqrt(ktot) * EPS, 1e-5 if ktot <= 2304 else 5e-5)


def _hold(tag, got, ref64, ref32, live, ktot):
    """the pixel-GEMM tests' two bars on the live elements, exact zeros on the others"""
    got = got.cpu()
    assert bool((got[~live] == 0).all()), f"{tag}: a masked element is not exactly zero"
    assert bool(torch.isfinite(got).all()), tag
    def err(a):
        d, r = (a.double() - ref64)[live], ref64[live]
        return (d.abs().max() / r.abs().max()).item(), (d.norm() / r.norm()).item()
    (em, el), (cm, cl) = err(got), err(ref32)
    bar, l2bar = _bar(ktot), 4.0 * max(cl, math.sqrt(ktot) * EPS / 8)
    print(f"[resnet-train] {tag:52s} Ktot {ktot:5d}  max-norm {em:.2e} (cpu {cm:.2e}, bar {bar:.2e})  rel-L2 {el:.2e} (cpu {cl:.2e}, bar {l2bar:.2e})")
    assert em <= bar and el <= l2bar, (tag, em, bar, el, l2bar)


# ------------------------------------------------------------------------------------------------ 1. conv1x1_dgrad with the ReLU mask
def _dgrad1_ref(dy, w, dx0, add, z, alpha, beta, dtype):
    v = alpha * torch.einsum("nohw,oi->nihw", dy.to(dtype), w.to(dtype))
    if beta:
        v = v + beta * dx0.to(dtype)
    if add is not None:
        v = v + add.to(dtype)
    return v * (z > 0).to(dtype)


@pytest.mark.parametrize("N,H,W,Cout,Cin,alpha,beta,with_add", [(2, 5, 7, 8, 12, 1.0, 0.0, False), (2, 5, 7, 8, 12, 0.5, 1.0, True),
                                                              (1, 16, 20, 64, 256, 1.0, 0.0, True), (1, 16, 20, 256, 64, 1.0, 1.0, False)])
def test_conv1x1_dgrad_relu_mask(amd, N, H, W, Cout, Cin, alpha, beta, with_add):
    """Shapes 12 -> 8, 256 -> 64 and 64 -> 256 (conv Cin -> Cout; the data gradient's K is Cout).  beta = 0: dx is NaN-filled before the call;
    beta = 1: dx is updated in place (it supplied nothing to the GEMM)."""
    ops = amd.ops
    dy, w = _rand((N, Cout, H, W), 1), _rand((Cout, Cin), 2) / math.sqrt(Cout)
    z, dx0 = _mask_values((N, Cin, H, W), 3), (_rand((N, Cin, H, W), 4) if beta else torch.full((N, Cin, H, W), NAN))
    add = _rand((N, Cin, H, W), 5) if with_add else None
    dx = _pm(dx0)
    out = ops.conv1x1_dgrad(_pm(dy), w.cuda(), dx=dx, alpha=alpha, beta=beta, z=_pm(z), z_act="relu", add=_pm(add) if with_add else None)
    assert out is dx
    ref = lambda dt: _dgrad1_ref(dy, w, dx0, add, z, alpha, beta, dt)
    _hold(f"dgrad1 relu N{N} {H}x{W} {Cin}<-{Cout} a{alpha} b{beta} add{int(with_add)}", dx, ref(torch.float64), ref(torch.float32), z > 0, Cout)


def test_conv1x1_dgrad_relu_mask_strided_view(amd):
    """dx and z are [:, :, ::2, ::2] of 9 x 13 maps; dx's map is pre-filled with a sentinel: the pixels in between stay bit-equal."""
    ops = amd.ops
    N, Cout, Cin = 2, 8, 12
    dy, w = _rand((N, Cout, 5, 7), 1), _rand((Cout, Cin), 2)
    zfull, sentinel = _mask_values((N, Cin, 9, 13), 3), 12345.678
    full0 = torch.full((N, Cin, 9, 13), sentinel)
    full0[:, :, ::2, ::2] = _rand((N, Cin, 5, 7), 4)
    full = _pm(full0)
    ops.conv1x1_dgrad(_pm(dy), w.cuda(), dx=full[:, :, ::2, ::2], beta=1.0, z=_pm(zfull)[:, :, ::2, ::2], z_act="relu")
    got = full.cpu()
    keep = torch.ones(9, 13, dtype=torch.bool)
    keep[::2, ::2] = False
    assert torch.equal(got[:, :, keep], full0[:, :, keep])
    z = zfull[:, :, ::2, ::2]
    ref = lambda dt: _dgrad1_ref(dy, w, full0[:, :, ::2, ::2], None, z, 1.0, 1.0, dt)
    _hold("dgrad1 relu strided 9x13 -> 5x7", got[:, :, ::2, ::2], ref(torch.float64), ref(torch.float32), z > 0, Cout)


def test_lrelu_through_the_new_entry_points_is_bit_equal_to_the_old(amd):
    ops = amd.ops
    dy, w, z = _pm(_rand((2, 8, 6, 10), 1)), _rand((8, 12, 3, 3), 2).cuda(), _pm(_mask_values((2, 12, 6, 10), 3))
    assert torch.equal(ops.conv3x3_dgrad(dy, w, z=z), ops.conv3x3_dgrad(dy, w, z=z, z_act="lrelu"))
    dy, w, z = _pm(_rand((2, 128, 16, 32), 1)), (_rand((128, 128, 3, 3), 2) / 34).cuda(), _pm(_mask_values((2, 128, 16, 32), 3))
    assert torch.equal(ops.conv3x3_wino_dgrad(dy, w, z=z), ops.conv3x3_wino_dgrad(dy, w, z=z, z_act="lrelu"))
    # 1x1: the old entry point has no mask; with an all-positive z the new one is the same GEMM and epilogue
    dy, w = _pm(_rand((1, 64, 16, 20), 1)), _rand((64, 256), 2).cuda()
    ones = _pm(torch.ones(1, 256, 16, 20))
    assert torch.equal(ops.conv1x1_dgrad(dy, w), ops.conv1x1_dgrad(dy, w, z=ones, z_act="lrelu"))
    with pytest.raises(amd.AfiError, match="z_act"):
        ops.conv1x1_dgrad(dy, w, z=ones, z_act="gelu")


# ------------------------------------------------------------------------------------------------ 2. 3x3 data gradients with the ReLU mask
@pytest.mark.parametrize("N,H,W,Cin,Cout,what", [(2, 6, 10, 12, 8, "small map: smallmap.hip's afi_epilogue_finish"),
                                                 (2, 96, 96, 12, 8, "tiled kernel: afi_epilogue_store")])
def test_conv3x3_dgrad_relu_mask(amd, N, H, W, Cin, Cout, what):
    """12 -> 8 on 6 x 10 is a small map (< 128 tiles of 128 x 128): under the default options it runs pix_gemm_wk, whose epilogue is
    smallmap.hip's; 2 x 96 x 96 pixels are 144 tiles, the tiled kernel with afi_epilogue_store."""
    ops = amd.ops
    dy, w, z = _rand((N, Cout, H, W), 1), _rand((Cout, Cin, 3, 3), 2) / math.sqrt(9 * Cout), _mask_values((N, Cin, H, W), 3)
    dx = _pm(torch.full((N, Cin, H, W), NAN))
    ops.conv3x3_dgrad(_pm(dy), w.cuda(), dx=dx, z=_pm(z), z_act="relu")
    ref = lambda dt: F.conv_transpose2d(dy.to(dt), w.to(dt), padding=1) * (z > 0).to(dt)
    _hold(f"dgrad3 relu N{N} {H}x{W} {Cin}<-{Cout} ({what})", dx, ref(torch.float64), ref(torch.float32), z > 0, 9 * Cout)


def test_conv3x3_wino_dgrad_relu_mask(amd):
    N, H, W, C_ = 2, 16, 32, 128
    dy, w, ref64, rest32 = wf.yardstick("dgrad", 2, N, C_, C_, H, W)
    z = _mask_values((N, C_, H, W), 3)
    live = z > 0
    got = amd.ops.conv3x3_wino_dgrad(_pm(dy), w.cuda(), z=_pm(z), z_act="relu").cpu()
    assert bool((got[~live] == 0).all()) and bool(torch.isfinite(got).all())
    m = live.double()
    e, r = wf.errors(got.double() * m, ref64 * m), wf.errors(rest32.double() * m, ref64 * m)
    bm, bl = wf.bars(r, wf.ktot("dgrad", 2, N, C_, C_, H, W))
    print(f"[resnet-train] wino dgrad relu: max-norm {e[0]:.2e} (restated {r[0]:.2e}, bar {bm:.2e})  rel-L2 {e[1]:.2e} (restated {r[1]:.2e}, bar {bl:.2e})")
    assert e[0] <= bm and e[1] <= bl


# ------------------------------------------------------------------------------------------------ 3. afi_frozen_wgrad_unfold
def test_frozen_wgrad_unfold(amd):
    """k in {1, 3} x (O, I) in {(8, 12), (128, 64)}, all four tensors in one launch, a non-zero grad going in; two runs bit-identical."""
    ops = amd.ops
    cases = [(k, O, I) for k in (1, 3) for O, I in ((8, 12), (128, 64))]
    host = []
    for n, (k, O, I) in enumerate(cases):
        host.append((_rand((O, I, k, k), 10 + n), _rand((O, I, k, k), 20 + n), 0.5 + torch.rand(O, generator=torch.Generator().manual_seed(30 + n))))

    def run():
        descs = []
        for (k, O, I), (dw, g0, s) in zip(cases, host):
            dwd = ops.to_ohwi(dw.cuda()) if k == 3 else dw.reshape(O, I).cuda()
            descs.append((dwd, g0.cuda().contiguous(), s.cuda()))
        ops.frozen_wgrad_unfold(descs)
        return [d[1].cpu() for d in descs]
    a, b = run(), run()
    for (k, O, I), (dw, g0, s), ga, gb in zip(cases, host, a, b):
        assert torch.equal(ga, gb)
        prod = s.double().view(-1, 1, 1, 1) * dw.double()
        ref = prod + g0.double()
        assert bool(((ga.double() - ref).abs() <= EPS * (prod.abs() + g0.double().abs())).all()), (k, O, I)


# ------------------------------------------------------------------------------------------------ 4. single blocks
class _Mini:
    """Stages of BottleneckBlocks as a ResNet that has only them (no stem): what _ResNetTrainFn needs of a network."""

    @staticmethod
    def build(amd, stages, stride_in_1x1, seed):
        rg = amd.resnet_guide

        class Mini(rg.ResNet):
            def __init__(self):
                torch.nn.Module.__init__(self)
                self.stage_names, self._out_features = list(stages), list(stages)
                for name, blocks in stages.items():
                    self.add_module(name, torch.nn.Sequential(*[rg.BottleneckBlock(cin, cout, mid, stride, stride_in_1x1)
                                                                for cin, cout, mid, stride in blocks]))
                self._train_stages = tuple(stages)
                for c in self._train_convs():
                    c.weight.requires_grad_(True)
        torch.manual_seed(seed)
        return R.randomise_norms(Mini(), seed + 1)


BLOCK_CASES = {
    # stages {name: [(cin, cout, bottleneck, stride)]}, stride_in_1x1; the first block of the first stage computes no dx
    "first-trainable-block-alone": ({"res3": [(16, 32, 8, 2)]}, True),
    "identity-after-downsampling": ({"res3": [(16, 32, 8, 2), (32, 32, 8, 1)]}, True),
    "downsampling-stride-in-1x1": ({"res3": [(16, 16, 8, 1)], "res4": [(16, 32, 8, 2)]}, True),
    "downsampling-stride-in-3x3": ({"res3": [(16, 16, 8, 1)], "res4": [(16, 32, 8, 2)]}, False),
    "identity-whose-input-is-an-output": ({"res3": [(16, 16, 8, 1)], "res4": [(16, 16, 8, 1)]}, True),
}


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", sorted(BLOCK_CASES))
def test_blocks_against_fp64_autograd(amd, case, fuse):
    stages, s1x1 = BLOCK_CASES[case]
    net = _Mini.build(amd, stages, s1x1, 7)
    cin = next(iter(stages.values()))[0][0]
    x = torch.relu(_rand((2, cin, 9, 13), 8))                                  # a block's input is a ReLU's output

    def ref(dt):
        sd = {k: v.detach().to(dt) for k, v in net.state_dict().items()}
        keys = [k for k in sd if k.endswith(".weight") and ".norm." not in k]
        for k in keys:
            sd[k].requires_grad_(True)
        y, feats = x.to(dt), {}
        for name, blocks in stages.items():
            for j, (_, _, _, stride) in enumerate(blocks):
                y = R.block(y, sd, f"{name}.{j}", stride, s1x1)
            feats[name] = y
        cot = {k: _rand(v.shape, 9 + i).to(dt) for i, (k, v) in enumerate(feats.items())}
        sum((feats[k] * cot[k]).sum() for k in feats).backward()
        return {k: v.detach() for k, v in feats.items()}, {k: sd[k].grad for k in keys}, cot
    f64, g64, cot = ref(torch.float64)
    f32, g32, _ = ref(torch.float32)
    net = net.cuda()
    convs = net._train_convs()
    outs = amd.resnet_guide._ResNetTrainFn.apply(net, fuse, _pm(x), *[c.weight for c in convs])
    sum((o * cot[k].float().cuda()).sum() for k, o in zip(stages, outs)).backward()
    bad = []
    for k, o in zip(stages, outs):
        e, c = R.rel_l2(o, f64[k]), R.rel_l2(f32[k], f64[k])
        print(f"[resnet-train] {case:36s} {k:24s} rel L2 gpu {e:.3e}  cpu fp32 {c:.3e}")
        bad += [(k, e, c)] if not e <= 4 * c else []
    for k, p in net.named_parameters():
        e, c = R.rel_l2(p.grad, g64[k]), R.rel_l2(g32[k], g64[k])
        print(f"[resnet-train] {case:36s} {k:24s} rel L2 gpu {e:.3e}  cpu fp32 {c:.3e}")
        assert g64[k].norm() > 0
        bad += [(k, e, c)] if not e <= 4 * c else []
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 5. whole networks
def _run_net(amd, name, fuse):
    net, freeze_at, x = R.make_net(name)
    net = net.cuda().trainable_(freeze_at, fuse_masks=fuse)
    out = net(x.cuda())
    cot = R.cotangents(name)
    sum((out[k] * cot[k].float().cuda()).sum() for k in out).backward()
    torch.cuda.synchronize()
    return net, out


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", sorted(R.NETS))
def test_network_against_fp64_autograd(amd, name, fuse):
    net, out = _run_net(amd, name, fuse)
    (f64, g64), (f32, g32) = R.reference(name, torch.float64), R.reference(name, torch.float32)
    assert list(out) == list(f64)
    bad, worst = [], 0.0
    for k in f64:
        assert not out[k].requires_grad or out[k].grad_fn is not None
        e, c = R.rel_l2(out[k], f64[k]), R.rel_l2(f32[k], f64[k])
        print(f"[resnet-train] {name} {k:28s} rel L2 gpu {e:.3e}  cpu fp32 {c:.3e}  bar {4 * c:.3e}")
        bad += [(k, e, c)] if not e <= 4 * c else []
    for k, p in net.named_parameters():
        if k not in g64:
            assert p.grad is None and not p.requires_grad, k                  # frozen parameters keep grad None
            continue
        assert p.grad is not None and tuple(p.grad.shape) == tuple(g64[k].shape), k
        e, c = R.rel_l2(p.grad, g64[k]), R.rel_l2(g32[k], g64[k])
        worst = max(worst, e / c)
        print(f"[resnet-train] {name} {k:28s} rel L2 gpu {e:.3e}  cpu fp32 {c:.3e}  bar {4 * c:.3e}")
        bad += [(k, e, c)] if not e <= 4 * c else []
    print(f"[resnet-train] {name} fuse={fuse}: worst gradient at {worst:.2f} x cpu fp32's deviation")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_determinism_and_poisoned_workspaces(amd, monkeypatch):
    cx = amd._lib.current_ctx()
    prev = cx.get_option("deterministic")
    cx.set_option("deterministic", 1)
    try:
        runs = []
        for poison in (False, False, True):
            if poison:
                monkeypatch.setattr(amd.ops, "_POISON", True)
            net, out = _run_net(amd, "small", True)
            runs.append(({k: v.detach().clone() for k, v in out.items()}, {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}))
    finally:
        cx.set_option("deterministic", prev)
    (o1, g1) = runs[0]
    assert len(g1) == 42 and all(bool(torch.isfinite(v).all()) for v in g1.values())
    for o, g in runs[1:]:
        assert all(torch.equal(o1[k], o[k]) for k in o1)
        assert all(torch.equal(g1[k], g[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g[k])]


# ------------------------------------------------------------------------------------------------ 7. integration
def test_fpn_afigan_over_the_trainable_bottom_up(amd):
    net, freeze_at, _ = R.make_net("small")
    x = _rand((2, 3, 64, 96), 11)                                              # a multiple of 32: the AFI x2 maps meet the laterals
    bottom_up = net.trainable_(freeze_at)
    fpn = amd.FPN_AFIGAN(bottom_up=bottom_up, in_features=["res2", "res3", "res4", "res5"], out_channels=32, norm="", top_block=amd.LastLevelMaxPool(),
                         fuse_type="sum").cuda()
    out = fpn(x.cuda())
    sum(p.sum() for p in out.values()).backward()
    torch.cuda.synchronize()
    for k, p in bottom_up.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0), k
        else:
            assert p.grad is None, k
    assert bottom_up.res3[0].conv1.weight.grad is not None and bottom_up.res5[2].conv3.weight.grad is not None


def test_detector_losses_reach_the_bottom_up(amd):
    """GeneralizedRCNN_AFExtractor over FPN_AFIGAN over the small trainable ResNet, a trainable RPN and box + mask heads at 64 x 80: five losses
    whose sum back-propagates into the bottom-up (tests/test_gpu_mask_loss.py runs the same detector over a torch conv pyramid)."""
    import numpy as np
    import mask_loss_f64 as Q
    features = ["p2", "p3", "p4", "p5"]
    net, freeze_at, _ = R.make_net("small")
    backbone = amd.FPN_AFIGAN(bottom_up=net.trainable_(freeze_at), in_features=["res2", "res3", "res4", "res5"], out_channels=16, norm="",
                              top_block=amd.LastLevelMaxPool(), fuse_type="sum").cuda()
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[16], [32], [64], [128]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": features, "PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 50, "PRE_NMS_TOPK_TRAIN": 200,
                                       "POST_NMS_TOPK_TRAIN": 50, "BATCH_SIZE_PER_IMAGE": 32}})
    shapes = {f: backbone.output_shape()[f] for f in features}
    rpn = amd.RPN(cfg, shapes).cuda().trainable_()
    heads = Q.e2e_heads(amd, 16).cuda().trainable_(mask_head=True)
    model = amd.GeneralizedRCNN_AFExtractor(backbone=backbone, proposal_generator=rpn, roi_heads=heads, pixel_mean=[0.0, 0.0, 0.0],
                                            pixel_std=[1.0, 1.0, 1.0], device="cuda").train()
    ih, iw = 64, 80
    gts = [np.array([[4, 6, 40, 50], [30, 20, 76, 60], [10, 30, 30, 44]], np.float32), np.array([[8, 8, 60, 40], [40, 34, 70, 62]], np.float32)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g = torch.Generator().manual_seed(4)
    batch = []
    for b in gts:
        polys = [[Q._ngon((x0 + x1) / 2, (y0 + y1) / 2, 0.45 * (x1 - x0), 0.45 * (y1 - y0), 9)] for x0, y0, x1, y1 in b.astype(np.float64)]
        tg = type("GT", (), {})()
        tg.gt_boxes, tg.gt_classes = dev(b), dev(np.arange(len(b), dtype=np.int64) % 5)
        tg.gt_masks = type("PolygonMasks", (), {"polygons": polys})()
        batch.append({"image_x0.5": torch.randn((3, ih, iw), generator=g), "targets": tg})
    losses, _ = model(batch)
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_mask", "loss_rpn_cls", "loss_rpn_loc"}
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for k, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0), k
        else:
            assert p.grad is None, k
