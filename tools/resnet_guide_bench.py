"""Forward time of the frozen ResNet-FPN guide (afigan_amd/resnet_guide.py) next to bench.py's harness guide (guide.GuideR50FPN) on the same
batch shapes: median (and min / max) over rounds of CUDA-event-timed forwards, after warm-up.  Random weights: the arithmetic is the same for
trained ones.  Prints one line per network and shape, and a JSON summary line.

    python tools/resnet_guide_bench.py --shapes 2x800x1344 2x400x672 --rounds 9 [--depth 50] [--trace-only]

--trace-only: one warm-up forward and three timed forwards of the new guide at the first shape, nothing else (for a rocprofv3 kernel trace)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, rounds, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["2x800x1344", "2x400x672"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import afigan_amd as amd
    from afigan_amd.guide import GuideR50FPN
    cfg = amd.get_cfg()
    cfg.merge_from_dict({"MODEL": {"RESNETS": {"DEPTH": args.depth, "OUT_FEATURES": ["res2", "res3", "res4", "res5"]},
                                   "FPN": {"IN_FEATURES": ["res2", "res3", "res4", "res5"]}}})
    new = amd.resnet_guide.build_resnet_fpn_backbone(cfg).cuda().eval()
    results = {}
    for s in args.shapes:
        N, H, W = (int(v) for v in s.split("x"))
        x = torch.randn((N, 3, -(-H // 32) * 32, -(-W // 32) * 32), device="cuda")     # the batch RCNN_FPN_only hands over: padded to 32
        with torch.no_grad():
            if args.trace_only:
                _time(lambda: new(x), 3, warmup=1)
                print(f"[trace] resnet_guide R-{args.depth} {s}: 1 warm-up + 3 forwards", flush=True)
                return
            t_new = _time(lambda: new(x), args.rounds)
            old = GuideR50FPN().cuda()
            img = torch.rand((N, 3, H, W), device="cuda") * 255.0
            t_old = _time(lambda: old(img), args.rounds)
            del old
        for name, ts in ((f"resnet_guide R-{args.depth}", t_new), ("GuideR50FPN", t_old)):
            print(f"{name:20s} {s:>12s}: median {statistics.median(ts):8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  ({len(ts)} rounds)",
                  flush=True)
        results[s] = {"resnet_guide_ms": statistics.median(t_new), "GuideR50FPN_ms": statistics.median(t_old)}
    print(json.dumps({"depth": args.depth, "rounds": args.rounds, "median_ms": results}))


if __name__ == "__main__":
    main()
