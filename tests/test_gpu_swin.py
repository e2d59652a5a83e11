"""The frozen Swin bottom-up (afigan_amd/swin_backbone.py) and its kernels on the GPU.

Each kernel is held to 1e-6 relative L2 and max-norm against an fp64 restatement in torch.nn.functional (tests/swin_f64.py, itself checked
against the reference's outputs by test_swin_host.py).  The whole network: the tiny config against the reference's own fp64 outputs
(tests/golden/swin_tiny.npz), and Swin-T against the fp64 restatement, each stage within 2x the error of the same restatement run in fp32 on
the CPU.  The BiFPN inference config over the HIP Swin-L is compared with the same BiFPN fed the fp64 Swin-L's features.  Measured values
are printed."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import swin_f64 as S

pytestmark = pytest.mark.gpu

SWIN_T = dict(EMBED_DIM=96, DEPTHS=[2, 2, 6, 2], NUM_HEADS=[3, 6, 12, 24], WINDOW_SIZE=7, OUT_FEATURES=["stage2", "stage3", "stage4", "stage5"])
# the Swin-L and BiFPN values of configs/inference/AFI-GAN_cascade_rcnn_swint_BiFPN_ST.yaml
SWIN_L = dict(EMBED_DIM=192, DEPTHS=[2, 2, 18, 2], NUM_HEADS=[6, 12, 24, 48], WINDOW_SIZE=12, OUT_FEATURES=["stage3", "stage4", "stage5"])
KERNEL_BAR = 1e-6


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


def _pm(t):
    """a CPU [N, H, W, C] / NCHW tensor as a pixel-major fp32 GPU tensor"""
    return t.float().cuda().contiguous(memory_format=torch.channels_last)


def _model(cfg):
    from afigan_amd import swin_backbone
    m = swin_backbone.SwinTransformer(cfg["EMBED_DIM"], cfg["DEPTHS"], cfg["NUM_HEADS"], cfg["WINDOW_SIZE"], 4.0, cfg["OUT_FEATURES"])
    return S.fill(m)


def _check(name, got, ref, bar=KERNEL_BAR):
    l2, mx = S.rel_err(got, ref)
    print(f"{name}: rel L2 {l2:.2e}, max {mx:.2e}")
    assert l2 <= bar and mx <= bar, (name, l2, mx)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("ws", [7, 12])
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("B,C,H,W", [(2, 64, 17, 23), (1, 96, 5, 9), (2, 32, 4, 6), (1, 64, 2 * 12 + 1, 3 * 12)])
def test_window_attention_vs_fp64(amd, ws, shifted, B, C, H, W):
    from afigan_amd import ops, swin_backbone
    g = torch.Generator().manual_seed(ws * 1000 + H * 10 + W + shifted)
    heads = C // 32
    qkv = torch.randn((B, H, W, 3 * C), generator=g, dtype=torch.float64).float().double()
    qkv_b = torch.randn(3 * C, generator=g, dtype=torch.float64).float().double()
    table = (torch.randn(((2 * ws - 1) ** 2, heads), generator=g, dtype=torch.float64) * 0.5).float().double()
    index = swin_backbone.relative_position_index(ws)
    shift = ws // 2 if shifted else 0
    ref = S.attention_from_qkv(qkv, qkv_b, table, index, heads, ws, shift)
    img = ops.swin_bias_image(table.float().cuda(), index.cuda(), ws)
    got = ops.swin_window_attn(_pm(qkv.permute(0, 3, 1, 2)), qkv_b.float().cuda(), img, ws, shift)
    _check(f"attention ws {ws} shift {shift} {B}x{C}x{H}x{W}", got.permute(0, 2, 3, 1), ref)


@pytest.mark.parametrize("C", [96, 192, 384, 768, 1536])
def test_layernorm_vs_fp64(amd, C):
    from afigan_amd import ops
    g = torch.Generator().manual_seed(C)
    x = (torch.randn((2, 7, 9, C), generator=g, dtype=torch.float64) * 3 + 1).float().double()
    w = (1 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)).float().double()
    b = (0.2 * torch.randn(C, generator=g, dtype=torch.float64)).float().double()
    got = ops.swin_layernorm(_pm(x.permute(0, 3, 1, 2)), w.float().cuda(), b.float().cuda())
    _check(f"layernorm C {C}", got.permute(0, 2, 3, 1), S.layer_norm(x, w, b))


@pytest.mark.parametrize("C,H,W", [(96, 7, 10), (192, 8, 8), (384, 5, 3), (768, 3, 4), (768, 2, 2)])
def test_patch_merging_vs_fp64(amd, C, H, W):
    """The 2x2 gather (odd sizes zero-padded) + LayerNorm over 4C (up to 3072), and the reduction on the 1x1 launcher."""
    from afigan_amd import ops
    g = torch.Generator().manual_seed(C + H * W)
    x = torch.randn((2, H, W, C), generator=g, dtype=torch.float64).float().double()
    w = (1 + 0.1 * torch.randn(4 * C, generator=g, dtype=torch.float64)).float().double()
    b = (0.2 * torch.randn(4 * C, generator=g, dtype=torch.float64)).float().double()
    red = (torch.randn((2 * C, 4 * C), generator=g, dtype=torch.float64) / (4 * C) ** 0.5).float().double()
    ref = S.layer_norm(S.merge_gather(x), w, b)
    got = ops.swin_layernorm(_pm(x.permute(0, 3, 1, 2)), w.float().cuda(), b.float().cuda(), merge=True)
    assert tuple(got.shape) == (2, 4 * C, (H + 1) // 2, (W + 1) // 2)
    _check(f"merge layernorm C {C} {H}x{W}", got.permute(0, 2, 3, 1), ref)
    out = ops.conv1x1_fwd(got, red.float().cuda())
    l2, mx = S.rel_err(out.permute(0, 2, 3, 1), F.linear(ref, red))
    print(f"merge + reduction C {C} {H}x{W}: rel L2 {l2:.2e}, max {mx:.2e}")
    assert l2 <= 2e-6 and mx <= 2e-6


@pytest.mark.parametrize("shape,C", [((2, 3, 30, 45), 96), ((1, 3, 29, 43), 128), ((1, 3, 64, 36), 192)])
def test_patch_embed_vs_fp64(amd, shape, C):
    from afigan_amd import ops
    g = torch.Generator().manual_seed(C)
    img = torch.randn(shape, generator=g, dtype=torch.float64).float().double()
    w = (torch.randn((C, 3, 4, 4), generator=g, dtype=torch.float64) / 48 ** 0.5).float().double()
    b, nw, nb = [(s * torch.randn(C, generator=g, dtype=torch.float64) + o).float().double() for s, o in ((0.2, 0), (0.1, 1), (0.2, 0))]
    got = ops.swin_patch_embed(img.float().cuda(), w.float().cuda(), b.float().cuda(), nw.float().cuda(), nb.float().cuda())
    _check(f"patch embed {shape} C {C}", got.permute(0, 2, 3, 1), S.patch_embed(img, w, b, nw, nb))


def test_gelu_vs_fp64(amd):
    from afigan_amd import ops
    x = (torch.randn((2, 5, 7, 384), generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 3).float().double()
    got = ops.swin_gelu_(_pm(x.permute(0, 3, 1, 2)))
    _check("gelu", got.permute(0, 2, 3, 1), F.gelu(x))


# ------------------------------------------------------------------------------------------------ the whole Swin
def test_tiny_swin_vs_reference_golden(amd):
    """The reference's own fp64 outputs for the tiny config: window padding, merge padding, a shift on maps smaller than the window."""
    g = np.load(S.GOLDEN)
    m = _model(S.TINY)
    assert sorted(m.state_dict()) == list(g["keys"])
    img = S.golden_image()
    cpu32 = S.forward(m, img, torch.float32)
    with torch.no_grad():
        got = m.cuda()(img.cuda())
    for k in S.TINY["OUT_FEATURES"]:
        ref = torch.from_numpy(g[k])
        assert got[k].shape == ref.shape and got[k].is_contiguous(memory_format=torch.channels_last), k
        e, e32 = S.rel_err(got[k], ref)[0], S.rel_err(cpu32[k], ref)[0]
        print(f"tiny {k}: rel L2 {e:.2e} against the reference (CPU fp32 {e32:.2e}, ratio {e / e32:.2f})")
        assert e <= 2 * e32, (k, e, e32)


@pytest.mark.parametrize("shape", [(2, 3, 123, 77), (1, 3, 200, 150), (1, 3, 896, 1408)])
def test_swin_t_vs_fp64(amd, shape):
    m = _model(SWIN_T)
    img = torch.randn(shape, generator=torch.Generator().manual_seed(shape[2]))
    ref = S.forward(m, img.cuda(), torch.float64, "cuda")
    cpu32 = S.forward(m, img, torch.float32)
    with torch.no_grad():
        got = m.cuda()(img.cuda())
    for k in SWIN_T["OUT_FEATURES"]:
        e, e32 = S.rel_err(got[k], ref[k])[0], S.rel_err(cpu32[k], ref[k])[0]
        print(f"Swin-T {shape} {k}: rel L2 {e:.2e} (CPU fp32 {e32:.2e}, ratio {e / e32:.2f})")
        assert e <= 2 * e32, (k, e, e32)


def test_hipgraph_capture_replays_bit_identically(amd):
    """No host synchronisation and no atomics in the forward: it captures into a hipGraph and replays bit-identically on new inputs; two
    eager runs are bit-identical."""
    m = _model(SWIN_L).cuda()
    x = torch.randn((1, 3, 200, 264), device="cuda")
    with torch.no_grad():
        eager = m(x)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = m(x)
        x.mul_(0.5).add_(0.25)
        graph.replay()
        torch.cuda.synchronize()
        eager2 = m(x)
        again = m(x)
    for k in eager:
        assert torch.equal(captured[k], eager2[k]), k
        assert torch.equal(again[k], eager2[k]), k
        assert not torch.equal(captured[k], eager[k]), k


def test_prepared_state_follows_the_weights(amd):
    """A changed bias table (in place) reaches the next forward: the dense bias images are rebuilt."""
    m = _model(S.TINY).cuda()
    x = torch.randn((1, 3, 64, 96), device="cuda")
    with torch.no_grad():
        a = m(x)["stage5"].clone()
        m.layers[3].blocks[1].attn.relative_position_bias_table.mul_(2.0)
        b = m(x)["stage5"]
        ref = S.forward(m, x, torch.float64, "cuda")["stage5"]
    assert not torch.equal(a, b)
    assert S.rel_err(b, ref)[0] <= 1e-5


def test_bifpn_inference_config_over_hip_swin(amd):
    """build_swint_bifpn_sr_backbone with the inference yaml's values (Swin-L, window 12, FPN_REPEAT 7, eval, no_grad) at 1x3x384x512:
    p3..p7 against the same BiFPN_AFIGAN fed the fp64 Swin-L's features rounded to fp32."""
    from afigan_amd import registry, swin_backbone
    cfg = amd.get_cfg()
    cfg.merge_from_dict({"MODEL": {"BACKBONE": {"NAME": "build_swint_bifpn_sr_backbone", "FREEZE_AT": -1},
                                   "SWINT": dict(SWIN_L), "BIFPN": {"IN_FEATURES": ["stage3", "stage4", "stage5"], "FPN_REPEAT": 7}}})
    old = dict(registry._BOTTOM_UP)
    try:
        swin_backbone.use_as_bottom_up()
        torch.manual_seed(11)
        bb = amd.BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, None)
    finally:
        registry._BOTTOM_UP.clear()
        registry._BOTTOM_UP.update(old)
    assert isinstance(bb, amd.BiFPN_AFIGAN) and isinstance(bb.bottom_up, swin_backbone.SwinTransformer)
    S.fill(bb.bottom_up)
    bb = bb.cuda().eval()
    x = torch.randn((1, 3, 384, 512), generator=torch.Generator().manual_seed(12)).cuda()
    with torch.no_grad():
        got = bb(x)
        feats = {k: v.float().contiguous(memory_format=torch.channels_last) for k, v in S.forward(bb.bottom_up, x, torch.float64, "cuda").items()}
        bb.bottom_up.forward = lambda _x: feats
        try:
            ref = bb(x)
        finally:
            del bb.bottom_up.forward
    for k in ("p3", "p4", "p5", "p6", "p7"):
        assert got[k].shape == ref[k].shape, k
        e = S.rel_err(got[k], ref[k])[0]
        print(f"Swin-L BiFPN {k}: rel L2 {e:.2e} against the BiFPN over the fp64 Swin-L")
        assert e <= 1e-4, (k, e)
