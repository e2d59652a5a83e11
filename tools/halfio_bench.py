"""Cost of bf16 / fp16 activations at the AFI boundary, against the fp32 path on the same shapes:

  fpn   FPN_AFIGAN fwd+bwd on one 800x1344 image (res2..res5 = 256/512/1024/2048 channels at strides 4..32, C = 256), bottom-up
        features in fp32, or in bf16 / fp16 with the module run under torch.autocast
  gen   Generator fwd+bwd at 1x256x25x34 and at P2 scale (1x256x100x168 -> 200x336)
  cast  the widening transpose (NCHW and channels_last sources) and the narrowing pass at P2 scale (1x256x200x336), in GB/s

Each number is the median of --repeats timed rounds of --iters calls (CUDA events around the round, after --warmup calls); the spread
printed beside it is min .. max over the rounds.  One JSON line per measurement; run alone on the GPU.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def timed(fn, warmup, iters, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return statistics.median(ms), min(ms), max(ms)


def emit(**kw):
    print(json.dumps(kw), flush=True)


class _BottomUp(nn.Module):
    def __init__(self, chans, strides):
        super().__init__()
        self.chans, self.strides = chans, strides

    def output_shape(self):
        from afigan_amd.fpn_sr import ShapeSpec
        return {f"res{i + 2}": ShapeSpec(c, s) for i, (c, s) in enumerate(zip(self.chans, self.strides))}

    def forward(self, feats):
        return feats


def bench_fpn(amd, args):
    chans, strides = [256, 512, 1024, 2048], [4, 8, 16, 32]
    net = amd.FPN_AFIGAN(_BottomUp(chans, strides), ["res2", "res3", "res4", "res5"], 256, top_block=amd.LastLevelMaxPool()).cuda()
    g = torch.Generator().manual_seed(0)
    base = {f"res{i + 2}": torch.randn((1, c, 800 // s, 1344 // s), generator=g).cuda() for i, (c, s) in enumerate(zip(chans, strides))}
    for name, dt in DT.items():
        feats = {k: v.to(dt).requires_grad_(True) for k, v in base.items()}

        def step():
            with torch.autocast("cuda", dtype=dt, enabled=dt != torch.float32):
                out = net(feats)
            sum(o.float().sum() for o in out.values()).backward()
        med, lo, hi = timed(step, args.warmup, args.iters, args.repeats)
        emit(bench="fpn_fwd_bwd_800x1344", dtype=name, ms=round(med, 3), min=round(lo, 3), max=round(hi, 3))


def bench_gen(amd, args):
    G = amd.Generator(in_channels=256, n_residual_dense_blocks=3).cuda()
    g = torch.Generator().manual_seed(1)
    for (H, W) in ((25, 34), (100, 168)):
        x0 = torch.randn((1, 256, H, W), generator=g).cuda()
        for name, dt in DT.items():
            x = x0.to(dt).requires_grad_(True)

            def step():
                with torch.autocast("cuda", dtype=dt, enabled=dt != torch.float32):
                    y = G(x)
                y.float().sum().backward()
            med, lo, hi = timed(step, args.warmup, args.iters, args.repeats)
            emit(bench=f"generator_fwd_bwd_1x256x{H}x{W}", dtype=name, ms=round(med, 3), min=round(lo, 3), max=round(hi, 3))


def bench_cast(amd, args):
    from afigan_amd import ops
    N, C_, H, W = 1, 256, 200, 336
    n = N * C_ * H * W
    src = torch.randn((N, C_, H, W), device="cuda")
    for name in ("bf16", "fp16"):
        dt = DT[name]
        for layout, t in (("nchw", src.to(dt).contiguous()), ("channels_last", src.to(dt).contiguous(memory_format=torch.channels_last))):
            med, lo, hi = timed(lambda: ops.ingest(t), args.warmup, args.iters, args.repeats)
            emit(bench=f"widen_{layout}_1x256x200x336", dtype=name, ms=round(med, 4), GBps=round(6 * n / med / 1e6, 1),
                 GBps_range=[round(6 * n / hi / 1e6, 1), round(6 * n / lo / 1e6, 1)])
        p = ops.pixel_major(src)
        med, lo, hi = timed(lambda: ops.narrow(p, dt), args.warmup, args.iters, args.repeats)
        emit(bench="narrow_1x256x200x336", dtype=name, ms=round(med, 4), GBps=round(6 * n / med / 1e6, 1),
             GBps_range=[round(6 * n / hi / 1e6, 1), round(6 * n / lo / 1e6, 1)])
    med, lo, hi = timed(lambda: ops.pixel_major(src), args.warmup, args.iters, args.repeats)
    emit(bench="nchw_to_nhwc_fp32_1x256x200x336", dtype="fp32", ms=round(med, 4), GBps=round(8 * n / med / 1e6, 1),
         GBps_range=[round(8 * n / hi / 1e6, 1), round(8 * n / lo / 1e6, 1)])
    med, lo, hi = timed(lambda: src.clone(), args.warmup, args.iters, args.repeats)
    emit(bench="torch_copy_fp32_1x256x200x336 (copy roof on this box)", dtype="fp32", ms=round(med, 4), GBps=round(8 * n / med / 1e6, 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", default="fpn,gen,cast")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(verbose=False)
    import afigan_amd as amd
    for w in args.what.split(","):
        {"fpn": bench_fpn, "gen": bench_gen, "cast": bench_cast}[w](amd, args)


if __name__ == "__main__":
    main()
