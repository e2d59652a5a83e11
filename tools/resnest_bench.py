"""Forward time of the frozen ResNeSt bottom-up (afigan_amd/resnest_backbone.py) next to the same network written with torch.nn.functional on
the GPU (F.conv2d / F.batch_norm / F.avg_pool2d / F.max_pool2d / F.softmax: MIOpen and torch kernels), with identical weights: median (and
min / max) over rounds of CUDA-event-timed forwards, after warm-up.  Random weights: the arithmetic is the same for trained ones.  Prints one
line per network and shape, and a JSON summary line.

    python tools/resnest_bench.py --shapes 2x800x1344 2x400x672 --rounds 9 [--depth 101] [--trace-only]

--trace-only: one warm-up forward and three timed forwards of the HIP bottom-up at the first shape, nothing else (for a rocprofv3 kernel trace)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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


def _bn(n, y):
    return F.batch_norm(y, n.running_mean, n.running_var, n.weight, n.bias, False, 0.0, n.eps)


def _conv(m, x, stride=1, padding=0, groups=1, norm=None):
    y = F.conv2d(x, m.weight, m.bias, stride=stride, padding=padding, groups=groups)
    n = norm if norm is not None else m.norm
    return _bn(n, y) if n is not None else y


def torch_resnest(bu, x):
    """The bottom-up restated with torch.nn.functional (NCHW, fp32, on the module's own parameters)."""
    st = bu.stem
    y = F.relu(_conv(st.conv1_1, x, stride=2, padding=1))
    y = F.relu(_conv(st.conv1_2, y, padding=1))
    y = F.max_pool2d(F.relu(_conv(st.conv1_3, y, padding=1)), 3, 2, 1)
    out = {}
    for name in bu.stage_names:
        for blk in getattr(bu, name):
            sp = blk.conv2
            t = F.relu(_conv(blk.conv1, y))
            t = F.relu(_conv(sp.conv, t, padding=1, groups=2, norm=sp.bn0))
            s0, s1 = torch.split(t, sp.channels, dim=1)
            h = F.relu(_conv(sp.fc1, F.adaptive_avg_pool2d(s0 + s1, 1), norm=sp.bn1))
            a = F.softmax(_conv(sp.fc2, h).view(t.shape[0], 2, sp.channels, 1, 1), dim=1)
            t = a[:, 0] * s0 + a[:, 1] * s1
            if blk.avd:
                t = F.avg_pool2d(t, 3, blk.stride, padding=1)
            t = _conv(blk.conv3, t)
            if blk.shortcut is not None:
                s = _conv(blk.shortcut, F.avg_pool2d(y, blk.stride, blk.stride, ceil_mode=True, count_include_pad=False))
            else:
                s = y
            y = F.relu(t + s)
        out[name] = y
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["2x800x1344", "2x400x672"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--depth", type=int, default=101)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import afigan_amd as amd
    cfg = amd.get_cfg()
    cfg.merge_from_dict({"MODEL": {"RESNETS": {"DEPTH": args.depth, "OUT_FEATURES": ["res2", "res3", "res4", "res5"], "RADIX": 2,
                                               "STRIDE_IN_1X1": False, "NORM": "SyncBN"}}})
    torch.manual_seed(0)
    bu = amd.resnest_backbone.build_resnest_backbone(cfg).cuda().eval()
    results = {}
    for s in args.shapes:
        N, H, W = (int(v) for v in s.split("x"))
        x = torch.randn((N, 3, -(-H // 32) * 32, -(-W // 32) * 32), device="cuda")     # the batch a detector hands over: padded to 32
        with torch.no_grad():
            if args.trace_only:
                _time(lambda: bu(x), 3, warmup=1)
                print(f"[trace] resnest R-{args.depth} {s}: 1 warm-up + 3 forwards", flush=True)
                return
            t_hip = _time(lambda: bu(x), args.rounds)
            t_torch = _time(lambda: torch_resnest(bu, x), args.rounds)
        for name, ts in ((f"HIP ResNeSt-{args.depth}", t_hip), (f"torch ResNeSt-{args.depth}", t_torch)):
            print(f"{name:20s} {s:>12s}: median {statistics.median(ts):8.3f} ms  min {min(ts):8.3f}  max {max(ts):8.3f}  ({len(ts)} rounds)",
                  flush=True)
        results[s] = {"hip_ms": statistics.median(t_hip), "torch_ms": statistics.median(t_torch)}
    print(json.dumps({"depth": args.depth, "rounds": args.rounds, "median_ms": results}))


if __name__ == "__main__":
    main()
