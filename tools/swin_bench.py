"""Forward time of the frozen Swin bottom-up (afigan_amd/swin_backbone.py) next to the same network written with torch.nn.functional on the
GPU in fp32 (tests/swin_f64.py's restatement: F.linear / F.layer_norm / softmax / roll / pad, torch and hipBLASLt kernels), with identical
weights: median (and min / max) over rounds of CUDA-event-timed forwards, after warm-up.  Weights follow the test weight rule: the arithmetic
is the same for trained ones.  Prints one line per network and shape, and a JSON summary line.

    python tools/swin_bench.py --shapes 2x896x1408 2x448x704 --rounds 9 [--nets T L] [--trace-only]

T is Swin-T (window 7, all four stages), L the BiFPN inference config's Swin-L (window 12, stage3..stage5).
--trace-only: one warm-up forward and three timed forwards of the HIP bottom-up of the first net at the first shape, nothing else (for a
rocprofv3 kernel trace)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NETS = {"T": dict(EMBED_DIM=96, DEPTHS=[2, 2, 6, 2], NUM_HEADS=[3, 6, 12, 24], WINDOW_SIZE=7, OUT_FEATURES=["stage2", "stage3", "stage4", "stage5"]),
        "L": dict(EMBED_DIM=192, DEPTHS=[2, 2, 18, 2], NUM_HEADS=[6, 12, 24, 48], WINDOW_SIZE=12, OUT_FEATURES=["stage3", "stage4", "stage5"])}


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
    ap.add_argument("--shapes", nargs="+", default=["2x896x1408", "2x448x704"])
    ap.add_argument("--nets", nargs="+", default=["T", "L"], choices=sorted(NETS))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import afigan_amd  # noqa: F401
    from afigan_amd import swin_backbone
    import swin_f64 as S
    results = {}
    for net in args.nets:
        c = NETS[net]
        m = S.fill(swin_backbone.SwinTransformer(c["EMBED_DIM"], c["DEPTHS"], c["NUM_HEADS"], c["WINDOW_SIZE"], 4.0, c["OUT_FEATURES"])).cuda()
        for s in args.shapes:
            N, H, W = (int(v) for v in s.split("x"))
            x = torch.randn((N, 3, H, W), device="cuda")
            with torch.no_grad():
                if args.trace_only:
                    _time(lambda: m(x), 3, warmup=1)
                    print(f"[trace] Swin-{net} {s}: 1 warm-up + 3 forwards", flush=True)
                    return
                t_hip = _time(lambda: m(x), args.rounds)
                t_torch = _time(lambda: S.forward(m, x, torch.float32, "cuda"), args.rounds)
            for name, ts in ((f"HIP Swin-{net}", t_hip), (f"torch Swin-{net}", t_torch)):
                print(f"{name:14s} {s:>12s}: median {statistics.median(ts):8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  ({len(ts)} rounds)",
                      flush=True)
            results[f"{net} {s}"] = {"hip_ms": statistics.median(t_hip), "torch_ms": statistics.median(t_torch)}
        del m
        torch.cuda.empty_cache()
    if not args.trace_only:
        results["bandwidth"] = bandwidth(args.shapes[0], args.rounds)
    print(json.dumps({"rounds": args.rounds, "median_ms": results}))


def bandwidth(shape, rounds):
    """Achieved GB/s (bytes read + written once / median time) of the LayerNorm and patch-merging passes on Swin-L's maps at `shape`."""
    from afigan_amd import ops
    N, H, W = (int(v) for v in shape.split("x"))
    h, w, C, out = -(-H // 4), -(-W // 4), 192, {}
    for stage in range(4):
        x = torch.randn((N, C, h, w), device="cuda").contiguous(memory_format=torch.channels_last)
        g, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        t = statistics.median(_time(lambda: ops.swin_layernorm(x, g, b), rounds))
        out[f"layernorm C {C} {h}x{w}"] = 2 * x.numel() * 4 / t / 1e6
        if stage < 3:
            g4, b4 = torch.ones(4 * C, device="cuda"), torch.zeros(4 * C, device="cuda")
            t = statistics.median(_time(lambda: ops.swin_layernorm(x, g4, b4, merge=True), rounds))
            out[f"merge C {C} {h}x{w}"] = (x.numel() + N * 4 * C * -(-h // 2) * -(-w // 2)) * 4 / t / 1e6
        h, w, C = -(-h // 2), -(-w // 2), 2 * C
    for k, v in out.items():
        print(f"{k:28s}: {v:7.0f} GB/s", flush=True)
    return out


if __name__ == "__main__":
    main()
