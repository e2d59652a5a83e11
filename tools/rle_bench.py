"""Pasted masks to COCO RLE strings, two ways, at the Mask R-CNN R50-FPN inference settings: 2 images x 100 detections, M = 28, paste at
800 x 1333, boxes drawn as tools/mask_bench.py draws them (tools/roi_bench.py make_boxes), masks smooth random blobs (a 4 x 4 normal field,
bicubic to 28 x 28, sigmoid).  Median (min / max) of 9 calls after warm-up:

  (a) afi_mask_paste alone             ops.mask_paste on all 200 detections                                      device events
  (b) count + emit                     afi_mask_rle_count, afi_mask_rle_emit back to back on all 200, the        device events
                                       offsets prepared beforehand (no host read inside the timed region)
  (c) bitmask path to RLE strings      per image: ops.mask_paste, .cpu(), rle.encode per mask, rle.to_strings    host clock, synchronised
  (d) RLE path to RLE strings          per image: paste_masks_rle                                                host clock, synchronised

then the bytes each path writes on the device and copies to the host, the mean and max starts per detection, the per-kernel device time of
(b) from one profiled pass, and a JSON summary line.  (c) and (d) are checked to give the same strings.

    python tools/rle_bench.py --rounds 9"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from roi_bench import make_boxes  # noqa: E402
from rpn_bench import _time  # noqa: E402


def make_probs(R, M, seed=1):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn((R, 1, 4, 4), generator=g) * 2.5
    return torch.sigmoid(F.interpolate(low, size=(M, M), mode="bicubic", align_corners=False))[:, 0].clamp(0, 1).contiguous().cuda()


def _host_time(fn, rounds, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def extent_words(boxes, H, W):
    """(64-row words, columns) of every box's pixel extent: what afi_mask_rle_count writes of its workspace."""
    b = boxes.double().cpu().numpy()
    xa, xb = np.clip(np.ceil(b[:, 0] - 0.5), 0, W), np.clip(np.floor(b[:, 2] - 0.5), -1, W - 1)
    ya, yb = np.clip(np.ceil(b[:, 1] - 0.5), 0, H), np.clip(np.floor(b[:, 3] - 0.5), -1, H - 1)
    ok = (b[:, 2] - b[:, 0] > 0) & (b[:, 3] - b[:, 1] > 0) & (xa <= xb) & (ya <= yb)
    cols = np.where(ok, xb - xa + 1, 0)
    words = np.where(ok, yb // 64 - ya // 64 + 1, 0)
    return int((cols * words).sum()), int(cols.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    import afigan_amd as amd
    from afigan_amd import _lib, ops, rle
    from afigan_amd.ops import _p, stream_ptr
    N, D, M, H, W = 2, 100, 28, 800, 1333
    R = N * D
    boxes = make_boxes(N, D, H, W)
    flat_boxes = boxes.reshape(-1, 4).contiguous()
    probs = make_probs(R, M)
    hw = (H, W)

    # (b)'s buffers: one untimed call gives the counts; the timed region is the two entry points with everything prepared
    starts0, nstarts = ops.mask_paste_rle(probs, flat_boxes, hw)
    nws = _lib.load().afi_mask_rle_ws_bytes(R, H, W)
    ws = ops.new_workspace((nws + 3) // 4, probs.device)
    nst = torch.empty((R,), device="cuda", dtype=torch.int32)
    offsets = (torch.cumsum(nstarts, 0) - nstarts).cuda()
    starts = torch.empty_like(starts0)

    def count():
        _lib.call("afi_mask_rle_count", _p(probs), _p(flat_boxes), R, M, H, W, 0.5, _p(ws), nws, _p(nst), stream_ptr())

    def emit():
        _lib.call("afi_mask_rle_emit", _p(flat_boxes), R, H, W, _p(ws), nws, _p(offsets), _p(starts), stream_ptr())

    def count_emit():
        count()
        emit()

    def bitmask_path():
        out = []
        for n in range(N):
            m = ops.mask_paste(probs[n * D:(n + 1) * D], boxes[n], hw).cpu().numpy()
            out += rle.to_strings([rle.encode(x) for x in m])
        return out

    def rle_path():
        out = []
        for n in range(N):
            out += [d["counts"] for d in amd.paste_masks_rle(probs[n * D:(n + 1) * D], boxes[n], hw)]
        return out

    count_emit()
    torch.cuda.synchronize()
    assert torch.equal(starts, starts0) and torch.equal(nst.cpu().long(), nstarts)
    same = bitmask_path() == rle_path()
    print(f"(c) and (d) give the same {R} strings: {same}", flush=True)

    parts = [("(a) afi_mask_paste", lambda: ops.mask_paste(probs, flat_boxes, hw), _time),
             ("(b) count + emit", count_emit, _time),
             ("    count alone (bits + count kernels)", count, _time),
             ("    emit alone", emit, _time),
             ("(c) bitmask path to strings", bitmask_path, _host_time),
             ("(d) RLE path to strings", rle_path, _host_time)]
    r = {}
    for name, fn, timer in parts:
        ts = timer(fn, args.rounds)
        r[name.strip()] = statistics.median(ts)
        print(f"{name:40s}: median {statistics.median(ts):9.3f} ms  min {min(ts):9.3f}  max {max(ts):9.3f}  ({len(ts)} rounds)", flush=True)
    a, b, c, d = (r[k] for k in ("(a) afi_mask_paste", "(b) count + emit", "(c) bitmask path to strings", "(d) RLE path to strings"))
    print(f"(b) / (a) = {b / a:.3f}   (d) / (c) = {d / c:.4f}", flush=True)

    words, cols = extent_words(flat_boxes, H, W)
    total = int(nstarts.sum())
    dev_a, dev_b = R * H * W, words * 8 + cols * 4 + R * 4 + total * 4
    print(f"bytes written on the device: bitmask {dev_a / 1e6:.1f} MB; RLE {dev_b / 1e6:.3f} MB (bits {words * 8 / 1e6:.3f}, column counts "
          f"{cols * 4 / 1e6:.3f}, starts {total * 4 / 1e6:.3f}); workspace allocated {nws / 1e6:.1f} MB", flush=True)
    print(f"bytes copied to the host: bitmask {dev_a / 1e6:.1f} MB; RLE {(R * 4 + total * 4) / 1e6:.3f} MB", flush=True)
    print(f"starts per detection: mean {total / R:.1f}, max {int(nstarts.max())}", flush=True)

    # per-kernel device time of (b): one profiled pass of 5 calls, apart from the timed rounds
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(5):
            count_emit()
        torch.cuda.synchronize()
    split = {}
    for e in prof.events():
        if "afi_mask_rle" in e.name:
            t = getattr(e, "device_time", None)
            t = e.cuda_time if t is None else t
            key = "bits" if "bits" in e.name else ("emit" if "Lb1" in e.name or "<true>" in e.name else "count")
            split.setdefault(key, []).append(t)
    split = {k: statistics.median(v) / 1e3 for k, v in split.items()}
    print("per-kernel device time of (b), median of 5 profiled launches (ms): " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(split.items())),
          flush=True)
    print(json.dumps({"rounds": args.rounds, "median_ms": r, "b_over_a": b / a, "d_over_c": d / c, "kernel_ms": split,
                      "device_bytes": {"bitmask": dev_a, "rle": dev_b}, "starts_mean": total / R, "starts_max": int(nstarts.max()),
                      "same_strings": same}))


if __name__ == "__main__":
    main()
