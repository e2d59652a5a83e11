"""CPU-side checks of the trainable ResNeSt bottom-up: the conditions tests/resnest_train_f64.py's fixtures promise, its closed
forms against fp64 autograd, the transposed pools against autograd of F.avg_pool2d, the refusals that need no device, and that every shape
tests/test_gpu_resnest_train.py runs takes the branch it is there for."""
import pytest
import torch
import torch.nn.functional as F

import resnest_train_f64 as R

import afigan_amd as amd
from afigan_amd import resnest_backbone


# ------------------------------------------------------------------------------------------------ fixture conditions
@pytest.mark.parametrize("freeze_at", R.FREEZE_ATS)
def test_fixture_conditions(freeze_at):
    rows = R.margins("small", freeze_at)
    blocks = sum(R.BLOCKS[50][freeze_at - 1:])
    assert len(rows) == 4 * blocks                                             # conv1, bn0, fc1 and the output of every trainable block
    for name, kind, margin, ones, live_min, live_max, units in rows:
        assert margin > 1.0, (name, margin)                                    # |pre| > 2^-24 (sum |w x| + |b|): fp32 decides the same mask
        if kind == "fc1":
            assert 1 <= live_min and live_max <= units - 1, (name, live_min, live_max, units)      # a live and a dead unit in every image
        else:
            assert 0.1 <= ones <= 0.9, (name, ones)


@pytest.mark.parametrize("freeze_at", R.FREEZE_ATS)
def test_fixture_attention_is_neither_flat_nor_saturated(freeze_at):
    rows = R.attention("small", freeze_at)
    assert len(rows) == sum(R.BLOCKS[50][freeze_at - 1:])
    for name, zmax, off in rows:
        assert zmax <= 8.0 and off >= 0.1, (name, zmax, off)


def test_trainable_keys_are_the_modules_trainable_parameters():
    net, _ = R.make_net("small")
    for freeze_at in R.FREEZE_ATS:
        net.trainable_(freeze_at)
        assert sorted(R.trainable_keys(net.state_dict(), freeze_at)) == sorted(k for k, p in net.named_parameters() if p.requires_grad)
    before = list(net.state_dict())
    assert list(net.trainable_(False).state_dict()) == before and not any(p.requires_grad for p in net.parameters())


# ------------------------------------------------------------------------------------------------ closed forms against autograd
@pytest.mark.parametrize("avd", [False, True])
@pytest.mark.parametrize("H,W", [(7, 9), (8, 10)])
def test_split_attention_closed_forms_against_autograd(H, W, avd):
    N, C, I = 3, 8, 32
    c = {k: v.double() for k, v in R.splat_case(N, C, I, H, W, avd).items()}
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("s0", "s1", "w1", "b1", "w2", "b2")}
    pre0, pre1 = leaves["s0"], leaves["s1"]                                    # the splits' pre-activations: positive where the split is
    s0, s1 = torch.relu(pre0), torch.relu(pre1)
    g, h, att = R.splat_forward(s0, s1, leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"])
    u = att[:, :C].reshape(N, C, 1, 1) * s0 + att[:, C:].reshape(N, C, 1, 1) * s1
    out = F.avg_pool2d(u, 3, 2, padding=1) if avd else u
    (out * c["dout"]).sum().backward()
    du = R.avg3s2p1_T(c["dout"], H, W) if avd else c["dout"]
    with torch.no_grad():
        da = R.splat_bwd_da(du, s0, s1)
        dz = R.splat_bwd_dz(da, att)
        dh = R.splat_bwd_dh(dz, h, c["w2"])
        dg = R.splat_bwd_dg(dh, c["w1"], H * W)
        close = lambda a, b: torch.allclose(a, b, rtol=1e-11, atol=1e-13)
        assert close(dz.t() @ h, leaves["w2"].grad) and close(dz.sum(0), leaves["b2"].grad)
        assert close(dh.t() @ g, leaves["w1"].grad) and close(dh.sum(0), leaves["b1"].grad)         # of the FOLDED fc1: the scale is the kernel's
        assert close(R.splat_bwd_ds(du, s0, att[:, :C], dg), pre0.grad) and close(R.splat_bwd_ds(du, s1, att[:, C:], dg), pre1.grad)
        assert bool(((h > 0).sum(1) > 0).all()) and bool(((h > 0).sum(1) < I).all())


@pytest.mark.parametrize("H,W", [(7, 9), (8, 10), (1, 2), (2, 1)])
def test_transposed_pools_against_autograd(H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn((2, 3, H, W), generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn((2, 3, (H + 1) // 2, (W + 1) // 2), generator=g, dtype=torch.float64)
    for pool, T in ((lambda t: F.avg_pool2d(t, 2, 2, ceil_mode=True, count_include_pad=False), R.avg2s2_ceil_T),
                    (lambda t: F.avg_pool2d(t, 3, 2, padding=1), R.avg3s2p1_T)):
        x.grad = None
        (pool(x) * dy).sum().backward()
        assert torch.allclose(T(dy, H, W), x.grad, rtol=1e-13, atol=1e-15)


# ------------------------------------------------------------------------------------------------ refusals that need no device
@pytest.mark.parametrize("norm", ["BN", "SyncBN"])
def test_trainable_refuses_batchnorm_stages(norm):
    net = resnest_backbone.ResNeSt(depth=50, norm=norm, freeze_at=2, width_per_group=8, res2_out_channels=16)
    with pytest.raises(amd.AfiError, match=r'train-mode BatchNorm in the bottom-up is out of scope; build with RESNETS.NORM "FrozenBN"'):
        net.trainable_(2)
    assert not any(p.requires_grad for p in net.parameters()) and net._train_stages == ()
    # (all of its stages frozen by the config carry FrozenBN: those can train)
    resnest_backbone.ResNeSt(depth=50, norm=norm, freeze_at=5, width_per_group=8, res2_out_channels=16).trainable_(2)


def test_trainable_refuses_the_stem_and_a_bad_freeze_at():
    net, _ = R.make_net("small")
    with pytest.raises(amd.AfiError, match="FREEZE_AT 0 trains the stem"):
        net.trainable_(0)
    for bad in (-1, 6, 2.0, True, "2", None):
        with pytest.raises(amd.AfiError, match="an integer 1..5"):
            net.trainable_(bad)
    assert net._train_stages == ()


def test_builders_and_the_registry_hook():
    from afigan_amd import registry
    cfg = amd.get_cfg()
    cfg.merge_from_dict({"MODEL": {"RESNETS": {"DEPTH": 50, "OUT_FEATURES": ["res2", "res3"], "RADIX": 2, "STRIDE_IN_1X1": False, "NORM": "FrozenBN",
                                               "WIDTH_PER_GROUP": 8, "RES2_OUT_CHANNELS": 16}, "BACKBONE": {"FREEZE_AT": 2}}})
    net = resnest_backbone.build_trainable_resnest_backbone(cfg)
    assert net._train_stages == ("res3",) and net.res3[0].conv2.fc1.bias.requires_grad and not net.res2[0].conv1.weight.requires_grad
    old = dict(registry._BOTTOM_UP)
    try:
        resnest_backbone.use_as_bottom_up(trainable=True)
        assert registry.bottom_up_builder("resnest") is resnest_backbone.build_trainable_resnest_backbone
        resnest_backbone.use_as_bottom_up()
        assert registry.bottom_up_builder("resnest") is resnest_backbone.build_resnest_backbone
    finally:
        registry._BOTTOM_UP.clear()
        registry._BOTTOM_UP.update(old)


def test_prepared_slots_and_fold_slots():
    """The joined dict is one object while nothing changes; a change of fc1's bias rebuilds the fc slot alone (the bias-free folds keep their
    tensors); fold_slots names the tensors of the "folded" slot, the grouped 3x3 as a k = 3 entry of [2C, C/2, 3, 3]."""
    net, _ = R.make_net("small")
    net.trainable_(2)
    with torch.no_grad():
        d = net._prepare()
        assert net._prepare() is d
        slots = net.fold_slots()
        assert len(slots) == len(net._train_convs()) == 13 * 3 + 3
        blk = net.res3[0]
        by_param = {id(w): fw for w, _, fw in slots}
        fw = by_param[id(blk.conv2.conv.weight)]
        assert fw is d[id(blk.conv2)][0][0] and tuple(fw.shape) == (16 * 2, 16 // 2, 3, 3) and fw.permute(0, 2, 3, 1).is_contiguous()
        assert by_param[id(blk.conv1.weight)] is d[id(blk.conv1)][0]
        blk.conv2.fc1.bias.add_(1.0)
        d2 = net._prepare()
        assert d2 is not d and d2[id(blk.conv2)][0][0] is fw and d2[id(blk.conv1)][0] is d[id(blk.conv1)][0]
        assert not torch.equal(d2[id(blk.conv2)][1][1], d[id(blk.conv2)][1][1])
        for m in net._own_convs():
            fresh = m.fold()
            flat = lambda o: [o] if torch.is_tensor(o) else [t for v in o for t in flat(v)]
            assert all(torch.equal(a, b) and a.stride() == b.stride() for a, b in zip(flat(d2[id(m)]), flat(fresh)))


# ------------------------------------------------------------------------------------------------ the GPU shapes take their branches
def test_gpu_shapes_take_the_branches_they_are_there_for():
    # dots: two chunks with a short last one; four pixel slots; one slot and 16-pixel chunks
    assert R.gap_chunks(48, 44, 8) == (2, 2048, 128) and 48 * 44 - 2048 == 64
    assert R.gap_chunks(7, 10, 256) == (2, 64, 4)
    assert R.gap_chunks(3, 6, 1024) == (2, 16, 1)
    # the attention test's 5 x 6 maps: one chunk, one chunk, two chunks
    assert [R.gap_chunks(5, 6, C)[0] for C in (8, 256, 1024)] == [1, 1, 2]
    # the gathered AVD transpose: pixels with 1, 2 and 4 sources on both maps; the even map's last row / column has one source (no window below)
    for H, W in ((7, 9), (8, 10)):
        sy, sx = R.avg3s2p1_sources(H), R.avg3s2p1_sources(W)
        counts = {len(a) * len(b) for a in sy for b in sx}
        assert counts == {1, 2, 4}, (H, W, counts)
    assert len(R.avg3s2p1_sources(8)[7]) == 1 and len(R.avg3s2p1_sources(7)[5]) == 2 and len(R.avg3s2p1_sources(7)[6]) == 1
    # the grouped conv: Winograd for group width 256 on 1 x 32 x 32 (128 -> 256 per group, 1024 pixels), direct for the C = 8 blocks
    assert resnest_backbone.conv2_wino(torch.empty(1, 256, 32, 32), 256)
    assert not resnest_backbone.conv2_wino(torch.empty(1, 256, 31, 32), 256) and not resnest_backbone.conv2_wino(torch.empty(2, 8, 9, 13), 8)
    # ... and the predicate is the forward's: frozen.conv3x3's rule on one group's channel counts
    from afigan_amd.rpn import _wino
    for gw, shape in ((256, (1, 128, 32, 32)), (128, (4, 64, 32, 32)), (512, (1, 256, 8, 8))):
        assert resnest_backbone.conv2_wino(torch.empty(shape[0], gw, *shape[2:]), gw) == _wino(torch.empty(shape), gw)
