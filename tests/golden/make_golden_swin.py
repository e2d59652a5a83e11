#!/usr/bin/env python3
"""Generate tests/golden/swin_tiny.npz from the REAL reference Swin Transformer (afigan/modeling/backbone/swin_transformer.py).

Run on the CPU of a machine that has the reference checkout:

    python tests/golden/make_golden_swin.py --reference PATH_TO_REFERENCE_CHECKOUT

The reference module is loaded BY PATH with importlib.  Its module-top imports need timm, detectron2 and fvcore, which are not installed,
so exactly those names are provided as stand-in modules in sys.modules:
  timm.models.layers: DropPath -> identity (eval: drop path is the identity anyway), to_2tuple, trunc_normal_ -> nn.init.trunc_normal_
  detectron2.layers: Conv2d, DeformConv, FrozenBatchNorm2d, ModulatedDeformConv, get_norm (never used by the Swin), ShapeSpec
  detectron2.modeling.backbone.Backbone -> nn.Module; detectron2.modeling.backbone.build.BACKBONE_REGISTRY.register -> identity
  fvcore.nn.weight_init -> an empty module (imported, never used)
The config is a tiny head-dim-32 Swin (EMBED_DIM 32, DEPTHS [2,2,2,2], NUM_HEADS [1,2,4,8], window 7, all four outputs).  Its weights follow
swin_weight_rule() below, which tests/test_gpu_swin.py restates; the fixture stores per-key checksums so drift in either copy is caught.
The input 1x3x116x172 forces window padding (29x43 tokens in stage 2), merge padding (29 and 43 are odd, 15 and 11 too) and a shift on
maps smaller than the window (stage 5 is 4x6).  The reference runs in float64.  Only arrays are written: the state_dict key list and shapes,
the checksums and the four outputs; no reference source or bytecode is copied."""
import argparse
import importlib.util
import os
import sys
import types
import zlib

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = dict(EMBED_DIM=32, DEPTHS=[2, 2, 2, 2], NUM_HEADS=[1, 2, 4, 8], WINDOW_SIZE=7, MLP_RATIO=4.0, DROP_PATH_RATE=0.2, APE=False,
           OUT_FEATURES=["stage2", "stage3", "stage4", "stage5"])
IMAGE = (1, 3, 116, 172)
IMAGE_SEED = 7


def swin_weight_rule(key, shape):
    """The value of parameter `key` (float64): legacy RandomState seeded with crc32(key); weights of linears / convs N(0, 1) / sqrt(fan-in),
    biases N(0, 0.2^2), LayerNorm weights 1 + N(0, 0.1^2) (a 1-D ``weight``), relative-position bias tables N(0, 0.5^2)."""
    rs = np.random.RandomState(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    z = rs.standard_normal(shape)
    if key.endswith("relative_position_bias_table"):
        return 0.5 * z
    if key.endswith("bias"):
        return 0.2 * z
    if len(shape) == 1:
        return 1.0 + 0.1 * z
    return z / np.sqrt(np.prod(shape[1:]))


def image():
    return np.random.RandomState(IMAGE_SEED).standard_normal(IMAGE)


def _stubs():
    timm = types.ModuleType("timm")
    tm = types.ModuleType("timm.models")
    tl = types.ModuleType("timm.models.layers")

    class DropPath(nn.Identity):
        def __init__(self, *a, **k):
            super().__init__()

    tl.DropPath = DropPath
    tl.to_2tuple = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    tl.trunc_normal_ = lambda t, std=1.0, **k: nn.init.trunc_normal_(t, std=std)
    d2 = types.ModuleType("detectron2")
    layers = types.ModuleType("detectron2.layers")
    for n in ("Conv2d", "DeformConv", "FrozenBatchNorm2d", "ModulatedDeformConv"):
        setattr(layers, n, type(n, (nn.Module,), {}))
    layers.get_norm = lambda *a, **k: None
    layers.ShapeSpec = lambda **k: types.SimpleNamespace(**k)
    modeling = types.ModuleType("detectron2.modeling")
    backbone = types.ModuleType("detectron2.modeling.backbone")
    backbone.Backbone = nn.Module
    build = types.ModuleType("detectron2.modeling.backbone.build")
    build.BACKBONE_REGISTRY = types.SimpleNamespace(register=lambda *a: (lambda f: f) if not a else a[0])
    fv = types.ModuleType("fvcore")
    fvnn = types.ModuleType("fvcore.nn")
    wi = types.ModuleType("fvcore.nn.weight_init")
    for name, mod in {"timm": timm, "timm.models": tm, "timm.models.layers": tl, "detectron2": d2, "detectron2.layers": layers,
                      "detectron2.modeling": modeling, "detectron2.modeling.backbone": backbone,
                      "detectron2.modeling.backbone.build": build, "fvcore": fv, "fvcore.nn": fvnn, "fvcore.nn.weight_init": wi}.items():
        sys.modules[name] = mod


def _load(ref):
    _stubs()
    spec = importlib.util.spec_from_file_location("ref_swin_transformer", os.path.join(ref, "afigan/modeling/backbone/swin_transformer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(HERE, "swin_tiny.npz"))
    args = ap.parse_args()
    mod = _load(args.reference)
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(SWINT=types.SimpleNamespace(**CFG), BACKBONE=types.SimpleNamespace(FREEZE_AT=-1)))
    torch.manual_seed(0)
    m = mod.build_swint_backbone(cfg, types.SimpleNamespace(channels=3))
    m.eval()                                    # (its train() returns None)
    sd = m.state_dict()
    keys = sorted(sd)
    params = {k for k, _ in m.named_parameters()}
    new, sums = {}, []
    for k in keys:
        if k in params:
            v = swin_weight_rule(k, tuple(sd[k].shape))
            new[k] = torch.from_numpy(v).to(torch.float32)
            f = new[k].double().numpy()
            sums.append((f.sum(), np.abs(f).sum()))
        else:
            new[k] = sd[k]
            sums.append((float(sd[k].double().sum()), float(sd[k].double().abs().sum())))
    m.load_state_dict(new, strict=True)
    m.double()
    with torch.no_grad():
        out = m(torch.from_numpy(image()).float().double())          # the fp32 image the GPU test feeds
    arrays = {"keys": np.array(keys), "is_param": np.array([k in params for k in keys]),
              "shapes": np.array([",".join(map(str, sd[k].shape)) for k in keys]), "checksums": np.array(sums, dtype=np.float64),
              "image_shape": np.array(IMAGE), "image_seed": np.array(IMAGE_SEED)}
    for name, v in out.items():
        arrays[name] = v.numpy()
    np.savez_compressed(args.out, **arrays)
    print(args.out, os.path.getsize(args.out), "bytes;", {k: tuple(v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main()
