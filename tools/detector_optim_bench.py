"""Time of the detector's optimiser step (afigan_amd/detector_optim.py) at the reference's workload: R-50 Mask R-CNN over FPN_AFIGAN,
full width, BACKBONE.FREEZE_AT 2, every gradient filled with random values.  Median (min / max) of device-event-timed runs after a warm-up.

    python tools/detector_optim_bench.py [--rounds 20] [--warmup 3]

Rows, alternated round by round in one session:
  DetectorOptim.step()          the table, its upload, one afi_detector_sgd_step launch with the fold, the version bumps and adopt_folded;
  + next _prepare()             what the next forward then pays for the bottom-up's prepared weights (a cache hit);
  torch.optim.SGD.step()        torch's optimiser over the same per-parameter groups (what Stage2Step was handed before);
  + next _prepare()             the refold of all 53 convs in torch fp64 that the next forward then pays;
  kernel, flat grid / (512, T)  the launch alone over an uploaded table, both grid shapes, with the bytes it moves (5 streams of 4 bytes per
                                element, 6 on a fold entry) as a fraction of the 6.29 TB/s float4 copy rate measured on an MI355X.
No figure here is a pass criterion."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12


def build_detector(amd):
    from afigan_amd import resnet_guide
    features = ["p2", "p3", "p4", "p5", "p6"]
    torch.manual_seed(0)
    net = resnet_guide.ResNet(depth=50, out_features=["res2", "res3", "res4", "res5"]).trainable_(2)
    backbone = amd.FPN_AFIGAN(bottom_up=net, in_features=["res2", "res3", "res4", "res5"], out_channels=256, norm="", top_block=amd.LastLevelMaxPool(),
                              fuse_type="sum").cuda()
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": True, "RPN": {"IN_FEATURES": features, "PRE_NMS_TOPK_TRAIN": 2000, "PRE_NMS_TOPK_TEST": 1000,
                                                        "POST_NMS_TOPK_TRAIN": 1000, "POST_NMS_TOPK_TEST": 1000},
                               "ANCHOR_GENERATOR": {"SIZES": [[32], [64], [128], [256], [512]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": features[:4], "NUM_CLASSES": 80},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "FC_DIM": 1024, "POOLER_RESOLUTION": 7, "POOLER_SAMPLING_RATIO": 0},
                               "ROI_MASK_HEAD": {"NAME": "MaskRCNNConvUpsampleHead", "NUM_CONV": 4, "CONV_DIM": 256, "POOLER_RESOLUTION": 14,
                                                 "POOLER_SAMPLING_RATIO": 0}})
    shapes = backbone.output_shape()
    rpn = amd.RPN(cfg, {f: shapes[f] for f in features}).cuda().trainable_()
    heads = amd.build_roi_heads(cfg, {f: shapes[f] for f in features[:4]}, masks=True).cuda().trainable_(mask_head=True)
    model = amd.GeneralizedRCNN(backbone=backbone, proposal_generator=rpn, roi_heads=heads, pixel_mean=[103.53, 116.28, 123.675],
                                pixel_std=[1.0, 1.0, 1.0], device="cuda").train()
    return model, net


def _row(name, ts, extra=""):
    print(f"  {name:34s} {statistics.median(ts):9.3f} ms  ({min(ts):.3f} / {max(ts):.3f}){extra}", flush=True)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "detector_optim_bench needs a GPU"
    import afigan_amd as amd
    from afigan_amd import _lib, ops
    model, net = build_detector(amd)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    for _, p in named:
        p.grad = torch.randn_like(p)                                            # (preserve_format: the parameter's own strides)
    mine = amd.DetectorOptim(named, modules=[net])
    theirs = torch.optim.SGD([{"params": [p], "lr": lr, "weight_decay": wd} for (_, p), (lr, wd) in zip(named, mine.groups)], lr=0.001, momentum=0.9)
    total = sum(p.numel() for _, p in named)
    folded = sum(w.numel() for w, _, _ in net.fold_slots())
    nbytes = 4 * (5 * total + folded)
    print(f"R-50 Mask R-CNN over FPN_AFIGAN, FREEZE_AT 2: {len(named)} trainable tensors, {total / 1e6:.1f} M elements ({folded / 1e6:.1f} M under a fold), "
          f"{nbytes / 1e6:.0f} MB moved per step; median (min / max) of {args.rounds} runs")

    # the launch alone: one uploaded table, both grids
    table = (_lib.DetSgdDesc * len(named))()
    folds = {id(w): (s, f) for w, s, f in net.fold_slots()}
    mom = torch.zeros(total + 4 * len(named), device="cuda")
    units, off = [], 0
    for d, (_, p) in zip(table, named):
        d.p, d.g, d.m, d.n, d.lr, d.wd = p.data_ptr(), p.grad.data_ptr(), mom.data_ptr() + 4 * off, p.numel(), 1e-6, 1e-4
        off += (p.numel() + 3) // 4 * 4
        if id(p) in folds:
            s, f = folds[id(p)]
            d.fold_out, d.s64, d.O, d.I, d.k = f.data_ptr(), s.data_ptr(), p.shape[0], p.shape[1], p.shape[2]
        units.append(ops.detector_sgd_units(d.n, d.O, d.I, d.k, bool(d.fold_out)))
    prefix = torch.tensor([0] + list(torch.tensor(units).cumsum(0)), dtype=torch.int32, device="cuda")
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()

    def launch(flat):
        _lib.call("afi_detector_sgd_step", table, ops._p(table_dev), len(named), max(units), ops._p(prefix) if flat else C.c_void_p(None), sum(units),
                  0.9, 1.0, ops.stream_ptr())

    rows = {k: [] for k in ("mine", "mine_prepare", "theirs", "theirs_prepare", "flat", "grid")}
    for i in range(args.warmup + args.rounds):
        t = {"mine": _timed(mine.step), "mine_prepare": _timed(net._prepare), "theirs": _timed(theirs.step), "theirs_prepare": _timed(net._prepare),
             "flat": _timed(lambda: launch(True)), "grid": _timed(lambda: launch(False))}
        if i >= args.warmup:
            for k, v in t.items():
                rows[k].append(v)
    res = {"tensors": len(named), "elements": total, "fold_elements": folded, "bytes": nbytes, "rounds": args.rounds}
    res["DetectorOptim.step"] = _row("DetectorOptim.step()", rows["mine"])
    res["DetectorOptim.step + _prepare"] = _row("  + next _prepare()", [a + b for a, b in zip(rows["mine"], rows["mine_prepare"])])
    res["torch.optim.SGD.step"] = _row("torch.optim.SGD.step()", rows["theirs"])
    res["torch.optim.SGD.step + _prepare"] = _row("  + next _prepare() (the refold)", [a + b for a, b in zip(rows["theirs"], rows["theirs_prepare"])])
    for k, name in (("flat", "kernel, flat grid"), ("grid", f"kernel, (512, {len(named)}) grid")):
        rate = nbytes / (statistics.median(rows[k]) * 1e-3)
        res[name] = _row(name, rows[k], f"   {rate / 1e12:.2f} TB/s = {100 * rate / COPY_RATE:.0f} % of the copy rate")
        res[name]["fraction_of_copy_rate"] = rate / COPY_RATE
    print(json.dumps(res))


if __name__ == "__main__":
    main()
