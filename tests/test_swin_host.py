"""The frozen Swin bottom-up (afigan_amd/swin_backbone.py) on the host: the reference SwinTransformer's key set and shapes (from the golden
fixture), the tree of the BiFPN inference config's Swin-L, the relative-position index, the options it refuses, the opt-in "swint" lookup
and a strict state_dict round trip of the whole BiFPN backbone.  Also checks tests/swin_f64.py -- the fp64 yardstick of test_gpu_swin.py --
against the reference's own outputs, and the weight rule against the fixture's checksums.  No GPU work: models are built on the CPU."""
import numpy as np
import pytest
import torch

import afigan_amd as amd
from afigan_amd import registry
import swin_f64 as S

# the Swin-L and BiFPN values of configs/inference/AFI-GAN_cascade_rcnn_swint_BiFPN_ST.yaml
YAML = {"BACKBONE": {"NAME": "build_swint_bifpn_sr_backbone", "FREEZE_AT": -1},
        "SWINT": {"OUT_FEATURES": ["stage3", "stage4", "stage5"], "EMBED_DIM": 192, "DEPTHS": [2, 2, 18, 2], "NUM_HEADS": [6, 12, 24, 48],
                  "WINDOW_SIZE": 12},
        "BIFPN": {"IN_FEATURES": ["stage3", "stage4", "stage5"], "FPN_REPEAT": 7}}


def _swin():
    from afigan_amd import swin_backbone
    return swin_backbone


def _cfg(**swint):
    cfg = amd.get_cfg()
    cfg.merge_from_dict({"MODEL": YAML})
    cfg.merge_from_dict({"MODEL": {"SWINT": swint}})
    return cfg


def _tiny():
    sb = _swin()
    T = S.TINY
    return sb.SwinTransformer(T["EMBED_DIM"], T["DEPTHS"], T["NUM_HEADS"], T["WINDOW_SIZE"], T["MLP_RATIO"], T["OUT_FEATURES"])


@pytest.fixture
def restore_bottom_up():
    old = dict(registry._BOTTOM_UP)
    yield
    registry._BOTTOM_UP.clear()
    registry._BOTTOM_UP.update(old)


def test_key_set_and_shapes_equal_the_reference():
    g = np.load(S.GOLDEN)
    sd = _tiny().state_dict()
    assert sorted(sd) == list(g["keys"])
    for k, s in zip(g["keys"], g["shapes"]):
        assert ",".join(map(str, sd[k].shape)) == s, k
    assert not any("absolute_pos_embed" in k for k in sd)


def test_weight_rule_matches_the_fixture_checksums():
    g = np.load(S.GOLDEN)
    sd = S.fill(_tiny()).state_dict()
    for k, (s, a) in zip(g["keys"], g["checksums"]):
        v = sd[k].double()
        assert np.isclose(float(v.sum()), s, rtol=1e-9, atol=1e-9) and np.isclose(float(v.abs().sum()), a, rtol=1e-9), k


def test_fp64_restatement_matches_the_reference_outputs():
    """The yardstick of the GPU tests equals the reference's own fp64 forward on the golden input (padding, merge padding, small-map shift)."""
    g = np.load(S.GOLDEN)
    out = S.forward(S.fill(_tiny()), S.golden_image())
    for k in S.TINY["OUT_FEATURES"]:
        ref = torch.from_numpy(g[k])
        assert out[k].shape == ref.shape
        assert S.rel_err(out[k], ref)[0] <= 1e-13, k


def test_inference_yaml_swin_l_tree():
    m = _swin().build_swint_backbone(_cfg(), None)
    assert [len(layer.blocks) for layer in m.layers] == [2, 2, 18, 2]
    sd = m.state_dict()
    assert {k.split(".")[0] for k in sd if k.startswith("norm")} == {"norm1", "norm2", "norm3"}
    assert tuple(sd["layers.2.blocks.17.attn.relative_position_bias_table"].shape) == (23 * 23, 24)
    assert tuple(sd["layers.2.downsample.reduction.weight"].shape) == (1536, 3072)
    assert tuple(sd["layers.3.blocks.1.mlp.fc1.weight"].shape) == (6144, 1536)
    assert "layers.3.downsample.norm.weight" not in sd and "layers.2.downsample.norm.weight" in sd
    assert [b.shift for b in m.layers[2].blocks[:4]] == [0, 6, 0, 6]
    assert {k: (s.channels, s.stride) for k, s in m.output_shape().items()} == {"stage3": (384, 8), "stage4": (768, 16), "stage5": (1536, 32)}
    assert m.size_divisibility == 0
    assert not any(p.requires_grad for p in m.parameters())


@pytest.mark.parametrize("ws", [7, 12])
def test_relative_position_index_is_canonical(ws):
    sb = _swin()
    idx = sb.SwinTransformer(96, [2], [3], ws, 4.0, ["stage2"]).layers[0].blocks[0].attn.relative_position_index
    n = ws * ws
    y, x = torch.arange(n) // ws, torch.arange(n) % ws
    ref = (y[:, None] - y[None, :] + ws - 1) * (2 * ws - 1) + (x[:, None] - x[None, :] + ws - 1)
    assert idx.dtype == torch.long and torch.equal(idx, ref)


@pytest.mark.parametrize("swint,match", [
    ({"APE": True}, "APE"),
    ({"EMBED_DIM": 96, "NUM_HEADS": [4, 8, 16, 32], "DEPTHS": [2, 2, 6, 2]}, "head dim"),
    ({"EMBED_DIM": 128, "NUM_HEADS": [4, 8, 16, 16], "DEPTHS": [2, 2, 18, 2]}, "head dim"),
    ({"WINDOW_SIZE": 8}, "WINDOW_SIZE"),
    ({"WINDOW_SIZE": 14}, "WINDOW_SIZE"),
    ({"EMBED_DIM": 256, "NUM_HEADS": [8, 16, 32, 64]}, "EMBED_DIM"),
    ({"OUT_FEATURES": ["stage6"]}, "OUT_FEATURES"),
])
def test_unsupported_options_raise(swint, match):
    with pytest.raises(amd.AfiError, match=match):
        _swin().build_swint_backbone(_cfg(**swint), None)


def test_input_channels_other_than_3_raise():
    from afigan_amd.fpn_sr import ShapeSpec
    with pytest.raises(amd.AfiError, match="3 input channels"):
        _swin().build_swint_backbone(_cfg(), ShapeSpec(channels=1, stride=1))


def test_drop_path_and_freeze_at_are_ignored():
    a = _swin().build_swint_backbone(_cfg(DROP_PATH_RATE=0.0), None)
    cfg = _cfg(DROP_PATH_RATE=0.5)
    cfg.MODEL.BACKBONE.FREEZE_AT = 2
    b = _swin().build_swint_backbone(cfg, None)
    assert {k: v.shape for k, v in a.state_dict().items()} == {k: v.shape for k, v in b.state_dict().items()}


def test_forward_refuses_autograd_and_the_cpu():
    m = _tiny()
    with pytest.raises(amd.AfiError, match="GPU only"):
        with torch.no_grad():
            m(torch.zeros(1, 3, 32, 32))
    m.patch_embed.proj.weight.requires_grad_(True)
    with pytest.raises(amd.AfiError, match="forward-only"):
        m(torch.zeros(1, 3, 32, 32))


def test_swint_bottom_up_is_opt_in(restore_bottom_up):
    """The default "swint" lookup is unchanged (no builder: AfiError); after use_as_bottom_up() the registered BiFPN builder builds the
    inference yaml's whole backbone on the CPU, and its state_dict loads back strictly."""
    if registry.USING_DETECTRON2_REGISTRY:
        pytest.skip("with detectron2 installed the default lookup is the reference's")
    sb = _swin()
    with pytest.raises(amd.AfiError, match="no 'swint' bottom-up builder"):
        registry.bottom_up_builder("swint")
    with pytest.raises(amd.AfiError, match="bottom-up"):
        amd.BACKBONE_REGISTRY.get("build_swint_bifpn_sr_backbone")(_cfg(), None)
    sb.use_as_bottom_up()
    assert registry.bottom_up_builder("swint") is sb.build_swint_backbone
    bb = amd.BACKBONE_REGISTRY.get("build_swint_bifpn_sr_backbone")(_cfg(), None)
    assert isinstance(bb, amd.BiFPN_AFIGAN) and isinstance(bb.bottom_up, sb.SwinTransformer)
    assert set(bb.output_shape()) == {"p3", "p4", "p5", "p6", "p7"}
    sd = bb.state_dict()
    assert "bottom_up.layers.2.blocks.17.attn.relative_position_index" in sd and "bottom_up.norm3.weight" in sd
    bb.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
