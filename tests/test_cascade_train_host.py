"""CascadeROIHeads' training passes without a GPU: the checker tests/cascade_train_f64.py against torch's own float64 BatchNorm and
hand-computed relabel cases, the conditions the GPU fixtures must meet -- the relabel fixtures' and, on the float64 chain of the whole heads,
every whole-head variant's --, the wrappers' refusals, the heads' surviving refusal and the two refusals that depend on the module's state.  Every test needs the feature's names (``feature``): on a tree without csrc/cascade_train.hip they all fail on the missing name."""
import numpy as np
import pytest
import torch

import cascade_f64 as QC
import cascade_train_f64 as T
import elementwise_f64 as E

F = np.float32


@pytest.fixture(autouse=True)
def feature():
    from afigan_amd import _lib, ops
    for name in ("roi_cascade_relabel", "roi_bn_stats", "roi_bn_relu_fwd", "roi_bn_relu_bwd_sums", "roi_bn_relu_bwd_apply"):
        getattr(ops, name)
        assert "afi_" + name in _lib.SIGNATURES
    return ops


# ------------------------------------------------------------------------------------------------ the checker's BatchNorm is torch's
@pytest.mark.parametrize("name", ["mixed", "full", "clamped"])
@pytest.mark.parametrize("shape", T.BN_SHAPES[:2], ids=str)
def test_masked_bn_checker_is_torch_batchnorm_on_compacted_rows(shape, name):
    """forward, running buffers and all three gradients of nn.BatchNorm2d (float64, train mode) + ReLU on the valid rows taken out by index
    selection equal the checker's masked passes to float64 rounding"""
    N, B, P1, C = shape
    counts = T.bn_counts(N, B)[name]
    x = T.bn_input("unit", N, B, P1, C, counts)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    v = T.valid_rows(counts, B)
    bn = torch.nn.BatchNorm2d(C, eps=E.f32(T.BN_EPS), momentum=E.f32(T.BN_MOMENTUM)).double()
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.5 * torch.randn(C, generator=gen))
        bn.bias.copy_(0.3 * torch.randn(C, generator=gen))
        bn.running_mean.copy_(0.2 * torch.randn(C, generator=gen))
        bn.running_var.copy_(1 + torch.rand(C, generator=gen))
    rm0, rv0 = bn.running_mean.clone().float(), bn.running_var.clone().float()
    bn.weight.data, bn.bias.data = bn.weight.data.float().double(), bn.bias.data.float().double()
    bn.running_mean.data, bn.running_var.data = rm0.double(), rv0.double()
    xc = x[v].double().permute(2, 0, 1).unsqueeze(0).requires_grad_(True)            # [1, C, rows, P1]
    y = torch.relu(bn(xc))
    y.backward(g[v].double().permute(2, 0, 1).unsqueeze(0))
    st = T.masked_stats(x, counts, B, T.BN_EPS, T.BN_MOMENTUM, rm0, rv0)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-11, atol=1e-12)
    assert close(st["running_mean"], bn.running_mean) and close(st["running_var"], bn.running_var) and int(bn.num_batches_tracked) == 1
    mean, invstd, gamma, beta = st["mean"], st["invstd"], bn.weight.detach(), bn.bias.detach()
    yref, _ = T.masked_relu_fwd(x, counts, B, mean, invstd, gamma, beta)
    assert close(yref[v], y[0].permute(1, 2, 0).detach()) and not bool(yref[~v].any())
    s0, s1 = T.masked_bwd_sums(g, x, yref, counts, B, mean, invstd)
    assert close(s0, bn.bias.grad) and close(s1, bn.weight.grad)
    dx, _ = T.masked_bwd_dx(g, x, yref, counts, B, mean, invstd, gamma, s0, s1)
    assert close(dx[v], xc.grad[0].permute(1, 2, 0)) and not bool(dx[~v].any())


def test_masked_bn_checker_without_a_valid_row():
    N, B, P1, C = T.BN_SHAPES[0]
    counts = T.bn_counts(N, B)["zero"]
    x = T.bn_input("unit", N, B, P1, C, counts)
    rm, rv = torch.ones(C), torch.full((C,), 2.0)
    st = T.masked_stats(x, counts, B, T.BN_EPS, T.BN_MOMENTUM, rm, rv)
    assert not bool(st["mean"].any()) and torch.equal(st["running_mean"], rm.double()) and torch.equal(st["running_var"], rv.double())
    assert abs(float(st["invstd"][0]) - 1 / np.sqrt(float(F(T.BN_EPS)))) < 1e-9
    z = torch.zeros(C)
    assert not bool(T.masked_bwd_dx(x, x, x, counts, B, z, z, z, z, z)[0].any())


# ------------------------------------------------------------------------------------------------ the relabel rule
def test_relabel_rule_on_hand_computed_cases():
    K = 3
    props = np.array([[[0, 0, 10, 10], [5, 5, 5, 9], [50, 50, 60, 60], [0, 0, 10, 5], [1, 1, 2, 2]]], F)
    pred = np.zeros((5, 8), F)
    pred[4] = np.nan                                                                 # past counts: never read
    gt, gc = np.array([[[0, 0, 10, 5], [9, 9, 9, 9]]], F), np.array([[2, 7]], np.int32)
    r = T.relabel(pred, K, props, [4], np.array([[64, 80]], F), (10, 10, 5, 5), gt, gc, [1], 0.5)
    assert r["counts"].tolist() == [3] and r["src"][0].tolist() == [0, 2, 3, -1, -1]
    assert r["gt_classes"][0].tolist() == [2, K, 2, -1, -1]                          # IoU exactly 0.5: foreground; no overlap: K; IoU 1
    assert np.array_equal(r["boxes"][0, :3], props[0, [0, 2, 3]]) and not r["boxes"][0, 3:].any()
    assert np.array_equal(r["gt_boxes"][0, :3], np.tile(gt[0, 0], (3, 1))) and not r["gt_boxes"][0, 3:].any()       # background rows too
    assert r["matched_idx"][0].tolist() == [0] * 5
    r = T.relabel(pred, K, props, [4], np.array([[64, 80]], F), (10, 10, 5, 5), gt, gc, [0], 0.5)                  # an image without ground truth
    assert r["counts"].tolist() == [3] and r["gt_classes"][0].tolist() == [K, K, K, -1, -1] and not r["gt_boxes"].any()
    r = T.relabel(pred, K, props, [4], np.array([[64, 80]], F), (10, 10, 5, 5), gt, gc, [1], 0.6)
    assert r["gt_classes"][0].tolist() == [K, K, 2, -1, -1]


@pytest.mark.parametrize("K", T.RELABEL_KS)
@pytest.mark.parametrize("case", range(len(T.RELABEL_CASES)))
def test_relabel_fixture_conditions(case, K):
    """What the GPU fixtures must hold: between 10 % and 90 % of the main image's rows dropped, both labels among its kept rows, the pushed-out
    and the NaN rows dropped, the tie won by the lower index, IoU exactly at the threshold foreground, one ulp below it background; the other
    image of case 0 loses every row."""
    c = T.relabel_case(case, K)
    r = T.relabel(c["pred"], K, c["proposals"], c["counts"], c["image_hw"], T.RELABEL_WEIGHTS, c["gt"], c["gt_classes"], c["counts_g"], T.RELABEL_THRESH)
    m, B = c["main"], T.RELABEL_B
    kept = int(r["counts"][m])
    assert 0.1 * B <= B - kept <= 0.9 * B
    src = r["src"][m, :kept].tolist()
    assert not set(src) & (set(T.PUSHED_OUT) | {T.NAN_ROW}) and src == sorted(src)
    cls = r["gt_classes"][m, :kept]
    assert (cls == K).any() and (cls < K).any()
    at = lambda row: src.index(row)
    assert r["matched_idx"][m, at(T.TIE_ROW)] == 1 and cls[at(T.TIE_ROW)] == c["gt_classes"][m, 1]
    assert r["matched_idx"][m, at(T.EXACT_ROW)] == 0 and cls[at(T.EXACT_ROW)] == c["gt_classes"][m, 0]
    if c["counts_g"][m] == 6:
        assert cls[at(T.BELOW_ROW)] == K and r["matched_idx"][m, at(T.BELOW_ROW)] == 5
    other = 1 - m
    assert r["counts"][other] == 0 and (case == 1 or c["counts"][other] == 17)
    assert (r["gt_classes"][other] == -1).all()


# ------------------------------------------------------------------------------------------------ refusals, keys
def test_wrappers_refuse_what_the_kernels_cannot_take(feature):
    from afigan_amd._lib import AfiError
    ops = feature
    x, counts = torch.zeros(10, 49, 12), torch.tensor([5, 5], dtype=torch.int32)
    v = torch.zeros(12)
    for call in (lambda: ops.roi_bn_stats(x, counts, 1e-5, 0.1), lambda: ops.roi_bn_relu_fwd(x, counts, v, v, v, v),
                 lambda: ops.roi_bn_relu_bwd_sums(x, x, x, counts, v, v), lambda: ops.roi_bn_relu_bwd_apply(x, x, x, counts, v, v, v, torch.zeros(2, 12)),
                 lambda: ops.roi_cascade_relabel(torch.zeros(10, 8), 3, torch.zeros(2, 5, 4), counts, torch.zeros(2, 2), (10, 10, 5, 5), torch.zeros(2, 1, 4),
                                                 torch.zeros(2, 1, dtype=torch.int32), counts, 0.5)):
        with pytest.raises(AfiError, match="GPU only"):
            call()
    with pytest.raises(AfiError, match="stored y"):
        ops.roi_bn_relu_bwd_sums(x, x, None, counts, v, v)


def test_heads_without_trainable_still_refuse_and_keep_their_keys():
    import afigan_amd as amd
    h = QC.build_heads(amd, ("p2", "p3"), 8, K=3, S=7, fc=16, num_conv=1, norm="SyncBN", stages=2)
    keys = set(h.state_dict())
    assert {"box_head.0.conv1.weight", "box_head.0.conv1.norm.weight", "box_head.0.conv1.norm.running_var", "box_head.0.conv1.norm.num_batches_tracked",
            "box_head.1.fc1.bias", "box_predictor.1.bbox_pred.weight"} <= keys and len(keys) == 2 * (1 + 5 + 2 + 4)
    with pytest.raises(amd.AfiError, match="cascade training is out of scope"):
        h.losses(None, {}, [], [])
    with pytest.raises(amd.AfiError, match=r"trainable_\(mask_head=True\) on heads built without the mask branch"):
        h.trainable_(mask_head=True)
    assert not h._train_enabled
    h.trainable_(False)                                                               # frozen parameters, training enabled; the keys stay
    assert h._train_enabled and set(h.state_dict()) == keys and not any(p.requires_grad for p in h.parameters())
    assert isinstance(h.box_head[0].conv1.norm.weight, torch.nn.Parameter) and "box_head.0.conv1.norm.weight" not in dict(h.named_buffers())
    with pytest.raises(amd.AfiError, match="GPU"):                                    # past the opt-in (and in training mode): the device's refusal
        h.train().losses(None, {"p2": torch.zeros(1, 8, 4, 4), "p3": torch.zeros(1, 8, 2, 2)}, [], [])


def test_state_refusals_come_before_any_device_work(monkeypatch):
    """BN / SyncBN heads in eval mode with targets, and SyncBN under more than one rank, are refused on the module's state alone: the calls
    below carry no features at all.  A "BN" head under two ranks, and a FrozenBN head in eval mode, pass on to the next check."""
    import afigan_amd as amd
    build = lambda norm: QC.build_heads(amd, ("p2", "p3"), 8, K=3, S=7, fc=16, num_conv=1, norm=norm, stages=2).trainable_()
    call = lambda h: h.losses(None, {}, [], [])
    h = build("SyncBN")                                                               # build_heads leaves the module in eval mode
    with pytest.raises(amd.AfiError, match=r"call \.train\(\)"):
        call(h)
    with pytest.raises(amd.AfiError, match=r"call \.train\(\)"):
        h.losses_padded({}, None, None, None, None, None)
    h.train()
    with pytest.raises(amd.AfiError, match="features .* are missing"):                # one rank: past both refusals
        call(h)
    for name, value in (("is_available", True), ("is_initialized", True), ("get_world_size", 2)):
        monkeypatch.setattr(torch.distributed, name, lambda *a, _v=value, **k: _v)
    with pytest.raises(amd.AfiError, match="more than one rank"):
        call(h)
    with pytest.raises(amd.AfiError, match="more than one rank"):
        h.losses_padded({}, None, None, None, None, None)
    with pytest.raises(amd.AfiError, match="features .* are missing"):                # plain BN keeps per-rank statistics, as torch's does
        call(build("BN").train())
    with pytest.raises(amd.AfiError, match="features .* are missing"):                # FrozenBN has no batch statistics: either mode
        call(build("FrozenBN").eval())
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 1)
    with pytest.raises(amd.AfiError, match="features .* are missing"):
        call(h)


def test_masked_bn_wrappers_cap_the_image_count(feature):
    from afigan_amd._lib import AfiError
    n = feature.ROI_BN_MAX_IMAGES + 1                                                  # every thread walks the counts: a longer list is refused
    with pytest.raises(AfiError, match=f"{n} images"):
        feature.roi_bn_stats(torch.zeros(n, 1, 4), torch.zeros(n, dtype=torch.int32), 1e-5, 0.1)
    with pytest.raises(AfiError, match="GPU only"):
        feature.roi_bn_stats(torch.zeros(n - 1, 1, 4), torch.zeros(n - 1, dtype=torch.int32), 1e-5, 0.1)


@pytest.mark.parametrize("variant", list(T.HEAD_VARIANTS))
def test_whole_head_fixture_conditions_on_the_float64_chain(variant):
    """What tests/test_gpu_cascade_train.py's whole-head cases need, proven on ``chain_train`` (float64 heads, the checker's label / sample /
    gather and relabel): every stage of every image keeps at least 8 foreground and 8 background rows, and with more than one stage at
    least one row is dropped somewhere (the two zero-width background proposals, by the first relabel)."""
    import afigan_amd as amd
    C, norm, S = T.HEAD_VARIANTS[variant]
    h = T.build_train_heads(amd, C, norm, S)
    st = T.chain_train(h.state_dict(), T.head_features(C), T.head_case(), norm, S)
    assert len(st) == S
    for k, s in enumerate(st):
        for n in range(T.HEAD_N):
            cls = s["gt_classes"][n, :s["counts"][n]]
            assert (cls < T.HEAD_K).sum() >= 8 and (cls == T.HEAD_K).sum() >= 8, (variant, k, n)
            assert (s["gt_classes"][n, s["counts"][n]:] == -1).all()
    assert st[0]["counts"].tolist() == [T.HEAD_BATCH] * T.HEAD_N
    if S > 1:
        assert int(st[0]["counts"].sum() - st[1]["counts"].sum()) >= 1
        assert all(int(st[k]["counts"].sum()) <= int(st[k - 1]["counts"].sum()) for k in range(1, S))
