"""The polygon rasteriser at a validation-set size: a seeded synthetic set shaped like COCO val2017's ground truth -- about 37k annotations of 1 to
3 polygons with 10 to 200 vertices each (star-shaped outlines of 5 to 150 px radius), canvases around 480 x 640 (a few sizes, so masks of one call
differ).  Median (min / max) of the rounds after warm-up, device events around each entry point on inputs already uploaded:

  afi_poly_rle_count     every mask's crossings, both sorts, the sweep; starts into the workspace
  afi_poly_rle_emit      the copy to the caller's offsets
  afi_rle_decode         --decode masks of the most common size into bytes
  polygons_rle()         the whole op on the host clock, synchronised: checks, packing, upload, count, the one read-back, emit

Bytes are what each stage must move at least (inputs read once, outputs written once); the count kernel reads the vertices twice and sorts in
LDS or in the workspace on top of that.  There is no bar: nothing else on the machine rasterises polygons, so the numbers are reported as they are.

    python tools/poly_rle_bench.py --rounds 9 [--annotations 37000] [--decode 256]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rpn_bench import _time  # noqa: E402
from rle_bench import _host_time  # noqa: E402

SIZES = ((480, 640), (640, 480), (427, 640), (480, 500), (375, 500))


def make_set(n, seed=0):
    rng = np.random.default_rng(seed)
    polys, sizes = [], []
    for _ in range(n):
        H, W = SIZES[int(rng.choice(len(SIZES), p=(0.5, 0.15, 0.15, 0.1, 0.1)))]
        ann = []
        for _ in range(int(rng.choice((1, 2, 3), p=(0.85, 0.1, 0.05)))):
            k = int(np.clip(rng.lognormal(3.3, 0.7), 10, 200))
            r = float(np.clip(rng.lognormal(3.3, 0.8), 5, 150))
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            rad = r * rng.uniform(0.7, 1.0, k)
            xy = np.stack([np.clip(cx + rad * np.cos(ang), 0, W), np.clip(cy + rad * np.sin(ang), 0, H)], 1)
            ann.append(np.round(xy * 100) / 100)                 # COCO stores two decimals
        polys.append([a.reshape(-1) for a in ann])
        sizes.append((H, W))
    return polys, sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--annotations", type=int, default=37000)
    ap.add_argument("--decode", type=int, default=256)
    args = ap.parse_args()
    from afigan_amd import _lib, ops
    from afigan_amd.ops import _p, call, stream_ptr
    polys, sizes = make_set(args.annotations)
    xy, voff, poff, hw2, cap = ops.polygons_batch(polys, sizes)
    N, cap_total = len(polys), int(cap[-1])
    print(f"{N} annotations, {poff[-1]} polygons, {xy.shape[0]} vertices, crossing capacity {cap_total}", flush=True)
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(a).to(dev)                # noqa: E731
    d_xy, d_voff, d_poff, d_hw2, d_cap = up(xy), up(voff), up(poff), up(hw2), up(cap)
    wsb = _lib.load().afi_poly_rle_ws_bytes(cap_total)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.int64, device=dev)
    nst = torch.empty((N,), dtype=torch.int32, device=dev)
    count = lambda: call("afi_poly_rle_count", _p(d_xy), _p(d_voff), _p(d_poff), _p(d_hw2), _p(d_cap), N, cap_total, _p(ws), wsb, _p(nst), stream_ptr())   # noqa: E731
    count()
    n = nst.cpu().to(torch.int64)
    assert int(n.min()) >= 0
    off = torch.cat((torch.zeros(1, dtype=torch.int64), torch.cumsum(n, 0))).to(dev)
    total = int(off[-1])
    starts = torch.empty((total,), dtype=torch.int32, device=dev)
    emit = lambda: call("afi_poly_rle_emit", _p(d_poff), _p(d_cap), N, cap_total, _p(ws), wsb, _p(off), _p(starts), stream_ptr())   # noqa: E731
    emit()
    cap_lds = _lib.DEFINES["AFI_POLY_RLE_LDS_CAP"]
    print(f"{total} starts (mean {total / N:.0f}, max {int(n.max())} per mask); workspace {wsb / 1e6:.1f} MB; LDS capacity {cap_lds} crossings", flush=True)
    out = {"annotations": N, "polygons": int(poff[-1]), "vertices": int(xy.shape[0]), "starts": total, "rounds": args.rounds, "median_ms": {}, "min_ms": {},
           "max_ms": {}, "bytes": {}}

    def report(name, ts, nbytes=None):
        out["median_ms"][name], out["min_ms"][name], out["max_ms"][name] = statistics.median(ts), min(ts), max(ts)
        extra = ""
        if nbytes is not None:
            out["bytes"][name] = int(nbytes)
            extra = f"  {nbytes / 1e6:9.1f} MB at least = {nbytes / statistics.median(ts) / 1e6:8.1f} GB/s"
        print(f"{name:22s}: median {statistics.median(ts):9.3f} ms  min {min(ts):9.3f}  max {max(ts):9.3f}  ({len(ts)} rounds){extra}", flush=True)

    in_bytes = xy.nbytes + voff.nbytes + poff.nbytes + hw2.nbytes + cap.nbytes
    report("afi_poly_rle_count", _time(count, args.rounds), in_bytes + 4 * total + 4 * N)
    report("afi_poly_rle_emit", _time(emit, args.rounds), 8 * total + 8 * (N + 1))
    H, W = SIZES[0]
    idx = [i for i, s in enumerate(sizes) if s == (H, W)][:args.decode]
    n_np, off_np, st_np = n.numpy(), off.cpu().numpy(), starts.cpu().numpy()
    sub = torch.from_numpy(np.concatenate([st_np[off_np[i]:off_np[i + 1]] for i in idx])).to(dev)
    sub_off = torch.from_numpy(np.concatenate(([0], np.cumsum(n_np[idx])))).to(dev)
    masks = torch.empty((len(idx), H, W), dtype=torch.uint8, device=dev)
    report(f"afi_rle_decode x{len(idx)}", _time(lambda: ops.rle_decode(sub, sub_off, (H, W), out=masks), args.rounds), masks.numel() + 4 * sub.numel())
    area = ops.coco_rle_area(sub, sub_off, torch.full((len(idx),), H * W, dtype=torch.int32, device=dev))
    assert torch.equal(area, masks.view(len(idx), -1).sum(1)), "decode and afi_coco_rle_area disagree"
    report("polygons_rle()", _host_time(lambda: ops.polygons_rle(polys, sizes), max(3, args.rounds // 3)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
