"""Per-shape A/B of the frozen guides' 1x1 convs: ops.conv1x1_fwd (the fp32-MFMA pixel GEMM) against ops.conv1x1_frozen_fwd (bf16x6 over a weight
image built once) on every 1x1 conv shape of GuideR50FPN at the given image sizes, each launch alone on the chip.  For each shape: `--rounds`
rounds alternating the two kernels, each round `--reps` launches between two events over `--bufs` rotating input / output sets (so a launch does
not find its own operands in the caches); the median per-launch time of each, their ratio, and the floor max(bytes / 5 TB/s, FLOP / 417 TFLOP/s)
with bytes = x once + out once + add once + image once.  The table decides ops.FROZEN1X1_MIN_PIXELS.

    python tools/frozen1x1_bench.py --images 2x800x1333 2x400x667 --rounds 5 --reps 10
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def guide_shapes(N, Himg, Wimg):
    """(name, Cin, Cout, H, W, stride, add, relu, count) of the distinct 1x1 convs of GuideR50FPN on an N x 3 x Himg x Wimg batch"""
    H, W = -(-Himg // 32) * 32 // 4, -(-Wimg // 32) * 32 // 4
    out = []
    for i, (cin, mid, cout, n, stride) in enumerate([(64, 64, 256, 3, 1), (256, 128, 512, 4, 2), (512, 256, 1024, 6, 2), (1024, 512, 2048, 3, 2)]):
        H, W = H // stride, W // stride
        s = f"res{i + 2}"
        out.append((f"{s}.0.c1", cin, mid, H, W, stride, False, True, 1))
        out.append((f"{s}.0.short", cin, cout, H, W, stride, False, False, 1))
        out.append((f"{s}.c3", mid, cout, H, W, 1, True, True, n))
        out.append((f"{s}.c1", cout, mid, H, W, 1, False, True, n - 1))
        out.append((f"{s}.lateral", cout, 256, H, W, 1, cout != 2048, False, 1))
    return out


def time_pair(fns, rounds, reps):
    for f in fns:
        f(0)
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for r in range(reps):
                f(r)
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3 / reps)
    return [statistics.median(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", nargs="+", default=["2x800x1333", "2x400x667"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bufs", type=int, default=3)
    args = ap.parse_args()
    from afigan_amd import ops
    rows = []
    print(f"{'conv':14s} {'shape':>28s} {'n':>2s} {'tile':>10s} {'old us':>9s} {'new us':>9s} {'old/new':>8s} {'floor us':>9s}", flush=True)
    for im in args.images:
        N, Himg, Wimg = (int(v) for v in im.split("x"))
        for name, cin, cout, H, W, stride, has_add, relu, count in guide_shapes(N, Himg, Wimg):
            if count == 0:
                continue
            M = N * H * W
            nb = args.bufs
            xs = [torch.randn((N, H * stride, W * stride, cin), device="cuda").permute(0, 3, 1, 2)[:, :, ::stride, ::stride] for _ in range(nb)]
            outs = [ops.new_pixel_major(N, cout, H, W, "cuda") for _ in range(nb)]
            adds = [torch.randn((N, H, W, cout), device="cuda").permute(0, 3, 1, 2) if has_add else None for _ in range(nb)]
            w = torch.randn(cout, cin, device="cuda") / cin ** 0.5
            b = torch.randn(cout, device="cuda")
            act = 2 if relu else 0
            x0 = xs[0]
            plan = ops.conv1x1_frozen_plan(N, H, W, cin, cout, (x0.stride(0), x0.stride(2), x0.stride(3)),
                                           add_strides=(adds[0].stride(0), adds[0].stride(2), adds[0].stride(3)) if has_add else None)
            old = lambda r: ops.conv1x1_fwd(xs[r % nb], w, b, add=adds[r % nb], out=outs[r % nb], act=act)
            if plan is None:
                t_old, = time_pair([old], args.rounds, args.reps)
                t_new, tile = float("nan"), "refused"
            else:
                image = ops.conv1x1_frozen_image(w)
                new = lambda r: ops.conv1x1_frozen_fwd(xs[r % nb], image, b, cout, add=adds[r % nb], out=outs[r % nb], act=act)
                t_old, t_new = time_pair([old, new], args.rounds, args.reps)
                tile = f"64x{plan['BN']}k{plan['KC']}"
            nbytes = 4 * M * (cin + cout * (2 if has_add else 1)) + 6 * cin * cout
            floor = max(nbytes / 5e12, 2.0 * M * cin * cout / 417e12) * 1e6
            shape = f"{M}px {cin}->{cout}{' s2' if stride == 2 else ''}{' +add' if has_add else ''}"
            print(f"{name:14s} {shape:>28s} {count:2d} {tile:>10s} {t_old:9.1f} {t_new:9.1f} {t_old / t_new:8.2f} {floor:9.1f}", flush=True)
            rows.append({"image": im, "conv": name, "M": M, "Cin": cin, "Cout": cout, "stride": stride, "add": has_add, "count": count, "tile": tile,
                         "old_us": t_old, "new_us": t_new, "floor_us": floor})
            del xs, outs, adds
    tot_old = sum(r["old_us"] * r["count"] for r in rows) / 1e3
    tot_best = sum(min(r["old_us"], r["new_us"] if r["new_us"] == r["new_us"] else r["old_us"]) * r["count"] for r in rows) / 1e3
    print(json.dumps({"sum_old_ms": tot_old, "sum_best_of_both_ms": tot_best, "rows": rows}))


if __name__ == "__main__":
    main()
