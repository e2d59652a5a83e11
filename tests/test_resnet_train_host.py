"""Host side of the trainable ResNet bottom-up: the fp64 restatement (tests/resnet_train_f64.py) held to things that are not this
project's, ``ResNet.trainable_``'s flags and refusals, and the conditions of the fixtures the GPU tests use.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import resnet_train_f64 as R


def _block_sd(cin, cout, mid, seed, shortcut=True):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    sd = {}
    for name, (o, i, k) in {"conv1": (mid, cin, 1), "conv2": (mid, mid, 3), "conv3": (cout, mid, 1), "shortcut": (cout, cin, 1)}.items():
        if name == "shortcut" and not shortcut:
            continue
        sd[f"b.{name}.weight"] = r(o, i, k, k) / (i * k * k) ** 0.5
        sd[f"b.{name}.norm.weight"] = 0.5 + torch.rand(o, generator=g, dtype=torch.float64)
        sd[f"b.{name}.norm.running_var"] = 0.5 + torch.rand(o, generator=g, dtype=torch.float64)
        sd[f"b.{name}.norm.bias"], sd[f"b.{name}.norm.running_mean"] = 0.1 * r(o), 0.1 * r(o)
    return sd


@pytest.mark.parametrize("stride,s1x1", [(1, True), (2, True), (2, False)])
def test_restatement_equals_conv2d_on_folded_weights_and_the_chain_rule(stride, s1x1):
    """The unfolded block equals F.conv2d on w' = w s[o] with bias b' (what the kernels run), and d loss / d w = s[o] d loss / d w' to 1e-12."""
    sd = _block_sd(8, 16, 4, 1)
    x = torch.randn((2, 8, 9, 13), generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    ws = [k for k in sd if k.endswith("weight") and ".norm." not in k]
    for k in ws:
        sd[k].requires_grad_(True)
    y = R.block(x, sd, "b", stride, s1x1)
    cot = torch.randn(y.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (y * cot).sum().backward()

    fold = {}
    for k in ws:
        s, t = R.scale_shift(sd, k[:-7])
        fold[k] = ((sd[k].detach() * s.view(-1, 1, 1, 1)).requires_grad_(True), t, s)
    s1, s3 = (stride, 1) if s1x1 else (1, stride)
    cv = lambda v, k, st, pad: F.conv2d(v, fold[k][0], fold[k][1], st, pad)
    a1 = torch.relu(cv(x, "b.conv1.weight", s1, 0))
    a2 = torch.relu(cv(a1, "b.conv2.weight", s3, 1))
    y2 = torch.relu(cv(a2, "b.conv3.weight", 1, 0) + cv(x, "b.shortcut.weight", stride, 0))
    (y2 * cot).sum().backward()
    assert (y - y2).abs().max() <= 1e-12 * y.abs().max()
    for k in ws:
        w2, _, s = fold[k]
        want = s.view(-1, 1, 1, 1) * w2.grad
        assert (sd[k].grad - want).abs().max() <= 1e-12 * want.abs().max(), k


def test_trainable_flags_follow_freeze_at():
    from afigan_amd import AfiError, resnet_guide
    net = resnet_guide.ResNet(50, width_per_group=8, res2_out_channels=32)
    frozen_keys = list(net.state_dict())
    assert not any(p.requires_grad for p in net.parameters())
    for freeze_at in (1, 2, 3, 4, 5):
        assert net.trainable_(freeze_at) is net
        for k, p in net.named_parameters():
            stage = int(k[3]) if k.startswith("res") else 1
            assert p.requires_grad == (k.startswith("res") and stage > freeze_at and k.endswith(".weight")), (freeze_at, k)
        assert all(".norm." not in k for k, _ in net.named_parameters())          # the FrozenBN tensors stay buffers
        assert net._train_stages == tuple(f"res{i}" for i in range(freeze_at + 1, 6))
    with pytest.raises(AfiError, match="7x7.*max-pool"):
        net.trainable_(0)
    with pytest.raises(AfiError, match="freeze_at"):
        net.trainable_(6)
    net.trainable_(2)
    net.trainable_(False)
    assert not any(p.requires_grad for p in net.parameters()) and net._train_stages == ()
    assert list(net.state_dict()) == frozen_keys == list(resnet_guide.ResNet(50, width_per_group=8, res2_out_channels=32).state_dict())


def test_cpu_tensor_is_refused_before_anything_touches_the_device():
    from afigan_amd import AfiError, resnet_guide
    net = resnet_guide.ResNet(50, width_per_group=8, res2_out_channels=32).trainable_(2)
    with pytest.raises(AfiError, match="GPU only"):
        net(torch.zeros(1, 3, 32, 32))
    with pytest.raises(AfiError, match="GPU only"):                                  # and the frozen path's refusal is what it was
        with torch.no_grad():
            net(torch.zeros(1, 3, 32, 32))
    net.trainable_(False)
    net.res3[0].conv1.weight.requires_grad_(True)                                    # not through trainable_: still the forward-only module
    with pytest.raises(AfiError, match="forward-only"):
        net(torch.zeros(1, 3, 32, 32))


def test_builders():
    from afigan_amd import get_cfg, registry, resnet_guide
    cfg = get_cfg()
    cfg.MODEL.RESNETS.OUT_FEATURES = ["res2", "res3", "res4", "res5"]
    cfg.MODEL.BACKBONE.FREEZE_AT = 3
    net = resnet_guide.build_trainable_resnet_backbone(cfg, None)
    assert net._train_stages == ("res4", "res5") and not net.res3[0].conv1.weight.requires_grad and net.res4[0].conv1.weight.requires_grad
    prev = dict(registry._BOTTOM_UP)
    try:
        resnet_guide.use_as_bottom_up()
        assert registry.bottom_up_builder("resnet") is resnet_guide.build_resnet_backbone
        resnet_guide.use_as_bottom_up(trainable=True)
        assert registry.bottom_up_builder("resnet") is resnet_guide.build_trainable_resnet_backbone
    finally:
        registry._BOTTOM_UP.clear()
        registry._BOTTOM_UP.update(prev)


@pytest.mark.parametrize("name", sorted(R.NETS))
def test_fixture_conditions(name):
    """Caps, not measurements: every ReLU unit of every trainable block is decided with margin (|pre| > 2^-24 (sum |w x| + |b|)), every mask has
    between 10 % and 90 % ones, and no gradient of the reference is zero or non-finite."""
    m = R.margins(name)
    counts, _ = R.counts_of(name)
    freeze_at = R.NETS[name][1]
    assert len(m) == 3 * sum(counts[freeze_at - 1:])
    worst = min(m, key=lambda t: t[1])
    lo, hi = min(t[2] for t in m), max(t[2] for t in m)
    print(f"\n{name}: {len(m)} ReLU layers; smallest margin {worst[1]:.3g} x the rule's threshold ({worst[0]}); ones {lo:.3f} .. {hi:.3f}")
    assert worst[1] > 1.0, worst
    assert 0.10 <= lo and hi <= 0.90, (lo, hi)
    _, g64 = R.reference(name, torch.float64)
    assert all(bool(torch.isfinite(g).all()) and g.norm() > 0 for g in g64.values())
