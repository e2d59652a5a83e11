"""The trainable Swin bottom-up without a GPU: the closed-form backward of tests/swin_train_f64.py against fp64 autograd, the refusals that
need no device, the freeze table, the DropPath rates, the optimiser groups, the branches the GPU shapes are listed for, and the conditioning
of the network fixture (so that the GPU bars compare code and not conditioning).  Worst margins are printed."""
import pytest
import torch
import torch.nn.functional as F

import swin_f64 as S
import swin_train_f64 as T

CLOSE = 1e-12           # fp64 rounding of sums of at most a few thousand terms of unit scale, relative to the largest entry


def _r(g, *shape, scale=1.0):
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def _close(name, got, ref):
    err = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
    print(f"{name}: max-norm {err:.2e}")
    assert got.shape == ref.shape and err <= CLOSE, (name, err)


def _model(cfg=S.TINY):
    from afigan_amd import swin_backbone
    return S.fill(swin_backbone.SwinTransformer(cfg["EMBED_DIM"], cfg["DEPTHS"], cfg["NUM_HEADS"], cfg["WINDOW_SIZE"], 4.0, cfg["OUT_FEATURES"]))


# ------------------------------------------------------------------------------------------------ closed forms against autograd
@pytest.mark.parametrize("C,H,W,merge", [(8, 5, 7, False), (8, 5, 3, True), (12, 7, 10, True), (8, 4, 6, True)])
def test_layernorm_bwd_closed_form(C, H, W, merge):
    g = torch.Generator().manual_seed(C + H)
    x = _r(g, 2, H, W, C, scale=3.0).requires_grad_(True)
    Ct = 4 * C if merge else C
    gamma, beta = (1 + 0.1 * _r(g, Ct)).requires_grad_(True), _r(g, Ct).requires_grad_(True)
    y = S.layer_norm(S.merge_gather(x) if merge else x, gamma, beta)
    dy = _r(g, *y.shape)
    ref = torch.autograd.grad((y * dy).sum(), [x, gamma, beta])
    dx, dgam, dbet, _ = T.layernorm_bwd(dy, x.detach(), gamma.detach(), merge=merge)
    for n, a, b in zip(("dx", "dgamma", "dbeta"), (dx, dgam, dbet), ref):
        _close(f"layernorm merge {merge} {H}x{W} {n}", a, b)


def test_gelu_bwd_closed_form():
    g = torch.Generator().manual_seed(1)
    x = _r(g, 3, 50, scale=3.0).requires_grad_(True)
    dy = _r(g, 3, 50)
    _close("gelu", T.gelu_bwd(dy, x.detach()), torch.autograd.grad((F.gelu(x) * dy).sum(), x)[0])


# a map that pads (17x23 under 7), a shifted window on a map smaller than the window (4x6 under 7 and 12), a map of whole windows
@pytest.mark.parametrize("ws,shifted,B,C,H,W", [(7, False, 2, 64, 17, 23), (7, True, 2, 64, 17, 23), (7, True, 2, 32, 4, 6), (12, True, 1, 32, 4, 6),
                                                (7, True, 1, 32, 14, 7), (12, False, 1, 32, 13, 12)])
def test_attention_bwd_closed_form(ws, shifted, B, C, H, W):
    from afigan_amd import swin_backbone
    g = torch.Generator().manual_seed(ws + H)
    heads, shift = C // 32, ws // 2 if shifted else 0
    qkv, qkv_b = _r(g, B, H, W, 3 * C).requires_grad_(True), _r(g, 3 * C).requires_grad_(True)
    table = _r(g, (2 * ws - 1) ** 2, heads, scale=0.5).requires_grad_(True)
    index = swin_backbone.relative_position_index(ws)
    out = S.attention_from_qkv(qkv, qkv_b, table, index, heads, ws, shift)
    dout = _r(g, *out.shape)
    ref = torch.autograd.grad((out * dout).sum(), [qkv, qkv_b, table])
    dpad, dbias, dtable = T.attention_bwd(dout, qkv.detach(), qkv_b.detach(), table.detach(), index, heads, ws, shift)
    assert tuple(dpad.shape) == (B, -(-H // ws) * ws, -(-W // ws) * ws, 3 * C)
    _close(f"attention ws {ws} shift {shift} dqkv (the crop)", dpad[:, :H, :W], ref[0])
    _close(f"attention ws {ws} shift {shift} dqkv_bias (the padded positions)", dpad.sum((0, 1, 2)) - dpad[:, :H, :W].sum((0, 1, 2)), ref[1])
    _close(f"attention ws {ws} shift {shift} dtable", dtable, ref[2])
    assert tuple(dbias.shape) == (heads, ws * ws, ws * ws)


def test_patch_gather_and_scale_add_closed_forms():
    g = torch.Generator().manual_seed(2)
    img = _r(g, 2, 3, 29, 43)
    w = _r(g, 16, 3, 4, 4)
    conv = F.conv2d(F.pad(img, (0, 1, 0, 3)), w, stride=4).permute(0, 2, 3, 1)
    _close("patch gather as a 1x1", F.linear(T.patch_gather(img), w.reshape(16, 48)), conv)
    assert float(T.patch_gather(img)[:, -1, :, 4:16].abs().max()) == 0.0        # rows 29 .. 31 of the last patch row: ky = 1, 2, 3 of channel 0
    a, b, s = _r(g, 2, 4, 5), _r(g, 2, 4, 5), torch.tensor([0.0, 1.25], dtype=torch.float64)
    out = T.scale_add(a, s, b)
    assert torch.equal(out[0], a[0]) and torch.equal(out[1], a[1] + 1.25 * b[1]) and torch.equal(T.scale_add(None, s, b)[1], 1.25 * b[1])


def test_network_restatement_is_swin_f64_forward_and_drop_path_is_restated():
    m = _model()
    img = S.golden_image().double()
    ref = S.forward(m, img)
    nb = len(m._blocks())
    ones = T.drop_scales(m, 0.0, torch.ones(2 * nb, img.shape[0]))
    got, kept = T.forward(m, T.leaves(m), img), T.forward(m, T.leaves(m), img, ones)
    for k in ref:                                               # (to fp64 rounding: torch's CPU GEMMs do not promise the same bits for the same call)
        _close(f"restatement {k}", got[k].detach(), ref[k])
        _close(f"restatement with all-ones DropPath scales {k}", kept[k].detach(), ref[k])
    masks = torch.ones(2 * nb, img.shape[0])
    masks[3, 0] = 0                                             # block 1's MLP branch of image 0 dropped
    dropped = T.forward(m, T.leaves(m), img, T.drop_scales(m, 0.2, masks))
    assert not torch.equal(dropped["stage2"].detach(), ref["stage2"])


# ------------------------------------------------------------------------------------------------ the public surface without a device
def test_freeze_table():
    for freeze_at in (-1, 0, 1, 2, 3):
        m = _model().trainable_(freeze_at)
        frozen_layers = freeze_at - 1 if freeze_at >= 2 else 0
        for n, p in m.named_parameters():
            want = not (n.startswith("patch_embed.") and freeze_at >= 0) and not any(n.startswith(f"layers.{i}.") for i in range(frozen_layers))
            assert p.requires_grad == want, (freeze_at, n)
        assert all(getattr(m, f"norm{i}").weight.requires_grad for i in range(4))
    m = _model()
    keys = sorted(m.state_dict())
    assert m.trainable_() is m and sorted(m.state_dict()) == keys
    assert all(not p.requires_grad for p in _model().parameters())


def test_refusals_without_a_device():
    from afigan_amd import AfiError
    for bad in (-2, 6, 1.0, True, None):
        with pytest.raises(AfiError, match="freeze_at"):
            _model().trainable_(bad)
    for bad in (-0.1, 1.0, 2, "0.2"):
        with pytest.raises(AfiError, match="drop_path_rate"):
            _model().trainable_(-1, bad)
    m = _model().trainable_(2)
    img = torch.zeros(1, 3, 32, 32)
    with pytest.raises(AfiError, match="input requires grad"):
        m(img.clone().requires_grad_(True))
    with pytest.raises(AfiError, match="2-byte"):
        m(img.half())
    m.layers[0].blocks[0].norm1.weight.requires_grad_(True)
    with pytest.raises(AfiError, match="frozen part"):
        m(img)
    with pytest.raises(AfiError, match="drop_masks"):
        _model().trainable_(-1, 0.0)(img, drop_masks=torch.ones(16, 1))
    with pytest.raises(AfiError, match="GPU only"):
        _model().trainable_()(img)
    # the module trainable_() was never called on refuses a differentiable forward in the frozen module's words
    m = _model()
    m.norm0.weight.requires_grad_(True)
    with pytest.raises(AfiError, match=r"^the Swin bottom-up is forward-only \(frozen\): run it under torch.no_grad\(\) with no parameter or input "
                                       r"requiring grad$"):
        m(img)


def test_drop_path_rates_and_builder():
    import afigan_amd
    from afigan_amd import registry, swin_backbone
    m = _model().trainable_(-1, 0.2)
    assert m.drop_path_rates() == [float(r) for r in torch.linspace(0, 0.2, 8)]
    assert _model().trainable_().drop_path_rates() == [0.0] * 8
    cfg = afigan_amd.get_cfg()
    cfg.merge_from_dict({"MODEL": {"BACKBONE": {"FREEZE_AT": 2}, "SWINT": dict(S.TINY)}})
    b = swin_backbone.build_trainable_swint_backbone(cfg)
    assert b.drop_path_rate == pytest.approx(0.2) and b._frozen_layers == 1 and not b._train_embed
    assert not any(p.requires_grad for p in swin_backbone.build_swint_backbone(cfg).parameters())
    old = dict(registry._BOTTOM_UP)
    try:
        swin_backbone.use_as_bottom_up(trainable=True)
        assert registry._BOTTOM_UP["swint"] is swin_backbone.build_trainable_swint_backbone
        swin_backbone.use_as_bottom_up()
        assert registry._BOTTOM_UP["swint"] is swin_backbone.build_swint_backbone
    finally:
        registry._BOTTOM_UP.clear()
        registry._BOTTOM_UP.update(old)


def test_optimizer_groups_by_module_type():
    """Every nn.LayerNorm parameter takes WEIGHT_DECAY_NORM (detectron2's build_optimizer decides by module type); param_group's results for
    keys are what they were."""
    from afigan_amd import detector_optim as D
    m = _model().trainable_()
    norm = {id(p) for p in D.norm_module_params(m)}
    names = {n for n, p in m.named_parameters() if id(p) in norm}
    assert "layers.0.blocks.0.norm1.weight" in names and "norm3.bias" in names and "layers.1.downsample.norm.weight" in names
    assert names == {n for n, _ in m.named_parameters() if ".norm" in "." + n.rsplit(".", 1)[0]}

    named = list(m.named_parameters())
    groups = dict(zip([n for n, _ in named], D.param_groups(named, D.norm_module_params(m), 0.02, 1e-4, 0.0, 2.0, 3e-4)))
    assert groups["layers.0.blocks.0.norm1.weight"] == (0.02, 0.0) and groups["norm2.bias"] == (0.02, 0.0)
    assert groups["layers.0.blocks.0.attn.qkv.bias"] == (0.04, 3e-4) and groups["layers.0.blocks.0.attn.qkv.weight"] == (0.02, 1e-4)
    by_key = dict(zip([n for n, _ in named], D.param_groups(named, (), 0.02, 1e-4, 0.0, 2.0, 3e-4)))
    assert all(by_key[n] == D.param_group(n, 0.02, 1e-4, 0.0, 2.0, 3e-4) for n in by_key)          # without the module list: the key rule, unchanged
    assert D.param_group("layers.0.blocks.0.norm1.weight", 0.02, 1e-4, 0.0) == (0.02, 1e-4)
    assert D.param_group("backbone.fpn_output2.norm.weight", 0.02, 1e-4, 0.0) == (0.02, 0.0)


# ------------------------------------------------------------------------------------------------ the GPU shapes take the branches they are listed for
def _strips_without_a_pixel(ws, shift, H, W):
    """(16-token strips of some window that hold no pixel of the H x W map, strips in all, windows): the index arithmetic of the module's
    docstring -- window token t of the window at (wy0, wx0) of the rolled, padded map is pixel ((wy0 + t // ws + shift) % Hp, ...)."""
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    t = torch.arange(ws * ws)
    empty = strips = 0
    for wy0 in range(0, Hp, ws):
        for wx0 in range(0, Wp, ws):
            real = ((wy0 + t // ws + shift) % Hp < H) & ((wx0 + t % ws + shift) % Wp < W)
            for t0 in range(0, ws * ws, 16):
                strips += 1
                empty += not bool(real[t0:t0 + 16].any())
    return empty, strips, (Hp // ws) * (Wp // ws)


def test_gpu_shapes_take_their_branches():
    """What tests/test_gpu_swin_train.py's shapes are listed for, derived from its own lists and asked of the library where the library decides."""
    import test_gpu_swin_train as G
    from afigan_amd import _lib, swin_backbone
    lib = _lib.load()
    # LayerNorm: every instantiation runs; one case has a single block of partials, one several blocks with several tokens per wave
    N, vecs, rows = 2, set(), {}                                                     # (the GPU tests' LayerNorm batch is 2)
    for C, H, W, merge in G.LN_CASES:
        Ct, Ho, Wo = (4 * C, (H + 1) // 2, (W + 1) // 2) if merge else (C, H, W)
        vecs.add(int(lib.afi_swin_layernorm_bwd_vecs(Ct)))
        floats = int(lib.afi_swin_layernorm_bwd_ws_floats(N, H, W, C, int(merge)))
        assert floats > 0 and floats % (2 * Ct) == 0
        rows[(C, H, W, merge)] = (floats // (2 * Ct), N * Ho * Wo)                   # partial rows (4 per block: one per wave), tokens
    print(f"LayerNorm instantiations {sorted(vecs)}, (partial rows, tokens) {rows}")
    assert vecs == {2, 6, 12}
    assert any(r == 4 for r, _ in rows.values())                                     # one block
    assert any(r > 4 and tokens > r for r, tokens in rows.values())                  # several blocks, and a wave's loop over tokens runs more than once
    assert any((H % 2 or W % 2) and merge for _, H, W, merge in G.LN_CASES)          # a merge that drops quadrants
    # attention: per case, padded tokens, all-padding query strips, windows per table row
    with_empty, without_empty = set(), set()
    for ws, shifted, B, C, H, W in G.ATTN_GRID:
        shift = ws // 2 if shifted else 0
        empty, strips, nW = _strips_without_a_pixel(ws, shift, H, W)
        groups = int(lib.afi_swin_window_attn_bwd_groups(B, H, W, C, ws))
        print(f"window {ws} shift {shift} {B}x{C}x{H}x{W}: {empty} of {strips} strips without a pixel, {nW} windows in {groups} groups")
        assert (-(-H // ws) * ws, -(-W // ws) * ws) != (H, W)                        # padded tokens present in every case
        assert 1 <= groups <= nW
        (with_empty if empty else without_empty).add((ws, shifted))
        assert empty < strips                                                        # never a map without pixels
    both = {(ws, sh) for ws in (7, 12) for sh in (False, True)}
    assert with_empty == both                                                        # every kernel variant meets a strip the forward returns early on
    assert without_empty                                                             # ... and a case where every strip holds a pixel
    for ws in (7, 12):
        assert any(B * _strips_without_a_pixel(w, 0, H, W)[2] > 1 for w, _, B, _, H, W in G.ATTN_GRID if w == ws)    # several windows add into one table row
        count = torch.bincount(swin_backbone.relative_position_index(ws).reshape(-1))
        assert int(count.max()) == ws * ws and int(count.min()) == 1                 # several pairs per table row, and a row of one pair


# ------------------------------------------------------------------------------------------------ fixture conditions
def test_network_fixture_is_well_conditioned():
    """The GPU network test's fixture (swin_f64.TINY, swin_train_f64.fill, the golden image): every LayerNorm input token has variance at least
    1e-2 x its mean square, and every softmax row's largest gap between unmasked logits is at most 8 (DESIGN 28's lesson: a saturated
    softmax makes the fp32 yardstick itself ill-conditioned)."""
    m = T.fill(_model())
    with torch.no_grad():
        var, gap = T.conditioning(m, T.leaves(m), S.golden_image().double())
    print(f"network fixture: min var / mean square {var:.3e} (bar 1e-2), max softmax logit gap {gap:.2f} (bar 8)")
    assert var >= 1e-2, var
    assert gap <= 8.0, gap
