"""Time of the trainable ResNet bottom-up (afigan_amd/resnet_guide.py: ResNet.trainable_, _ResNetTrainFn) at the training configs' size
-- R-50, N = 2 at 800 x 1344, BACKBONE.FREEZE_AT 2, out_features res2 .. res5 -- next to a torch-ROCm restatement (F.conv2d on the unfolded
weights plus the FrozenBN affine, autograd) on the same GPU with the same weights: median (min / max) of device-event-timed runs after a warm-up.

    python tools/resnet_train_bench.py [--rounds 20] [--warmup 3] [--batch 2] [--height 800] [--width 1344] [--deviation]

Rows:
  forward               the whole bottom-up with the trainable stages under autograd (stem and res2 frozen);
  backward, fused       _ResNetTrainFn.backward with fuse_masks=True: the ReLU masks, residual joins and cotangents in the data gradients' epilogues;
  backward, unfused     the same GEMMs with afi_relu_bwd and the adds as passes of their own (fuse_masks=False);
  unfold                the one afi_frozen_wgrad_unfold launch over the 43 trainable convs (descriptor table included);
  refold                the fp64 fold of every conv after a parameter changed (what the first forward after an optimiser step pays);
  torch forward / backward   the restatement.
A random cotangent per output stands for the pyramid's gradient.  --deviation: also the relative-L2 deviation from a float64 CPU evaluation of
outputs and weight gradients on a res2 / res3 network at 1 x 3 x 512 x 1024 (res3: 8192 pixels, where the training forward's 3x3 convs take the
F(4x4) inference tiling), next to torch CPU fp32's.  No figure here is a pass criterion."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BN_EPS = 1e-5


def _time(fn, rounds, warmup, before=None):
    ts = []
    for i in range(warmup + rounds):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b))
    return ts


def _row(name, ts):
    print(f"  {name:28s} {statistics.median(ts):9.3f} ms  ({min(ts):.3f} / {max(ts):.3f})", flush=True)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def make_net(seed=0, **kw):
    from afigan_amd import resnet_guide
    torch.manual_seed(seed)
    net = resnet_guide.ResNet(**kw)
    g = torch.Generator().manual_seed(seed + 1)
    for k, b in net.named_buffers():
        if k.endswith("norm.weight") or k.endswith("norm.running_var"):
            b.copy_(0.5 + torch.rand(b.shape, generator=g))
        else:
            b.copy_(0.1 * torch.randn(b.shape, generator=g))
    return net


# ------------------------------------------------------------------------------------------------ the restatement
def _conv_bn(x, sd, pre, stride, pad):
    s = sd[pre + ".norm.weight"] * torch.rsqrt(sd[pre + ".norm.running_var"] + BN_EPS)
    t = sd[pre + ".norm.bias"] - sd[pre + ".norm.running_mean"] * s
    return F.conv2d(x, sd[pre + ".weight"], None, stride, pad) * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1)


def torch_resnet(x, sd, counts, outs):
    y = F.max_pool2d(torch.relu(_conv_bn(x, sd, "stem.conv1", 2, 3)), 3, 2, 1)
    out = {}
    for i, n in enumerate(counts):
        for j in range(n):
            pre, stride = f"res{i + 2}.{j}", (2 if i > 0 and j == 0 else 1)
            sc = _conv_bn(y, sd, pre + ".shortcut", stride, 0) if pre + ".shortcut.weight" in sd else y
            a = torch.relu(_conv_bn(y, sd, pre + ".conv1", stride, 0))
            a = torch.relu(_conv_bn(a, sd, pre + ".conv2", 1, 1))
            y = torch.relu(_conv_bn(a, sd, pre + ".conv3", 1, 0) + sc)
        if f"res{i + 2}" in outs:
            out[f"res{i + 2}"] = y
    return out


def _state(net, dtype, device, freeze_at):
    sd = {k: v.detach().to(device=device, dtype=dtype) for k, v in net.state_dict().items()}
    keys = [k for k in sd if k.endswith(".weight") and ".norm." not in k and k.startswith("res") and int(k[3]) > freeze_at]
    for k in keys:
        sd[k].requires_grad_(True)
    return sd, keys


# ------------------------------------------------------------------------------------------------ timing
def bench(args):
    from afigan_amd import ops
    outs, counts, freeze_at = ["res2", "res3", "res4", "res5"], [3, 4, 6, 3], 2
    net = make_net(depth=50, out_features=outs).cuda()
    x = torch.randn((args.batch, 3, args.height, args.width), generator=torch.Generator().manual_seed(2)).cuda()
    res = {"shape": [args.batch, 3, args.height, args.width], "freeze_at": freeze_at, "rounds": args.rounds}
    print(f"R-50 bottom-up, N = {args.batch} at {args.height} x {args.width}, FREEZE_AT {freeze_at}; median (min / max) of {args.rounds} runs")
    cots = None
    for fuse in (True, False):
        net.trainable_(freeze_at, fuse_masks=fuse)
        params = [p for p in net.parameters() if p.requires_grad]
        if fuse:
            res["forward"] = _row("forward", _time(lambda: net(x), args.rounds, args.warmup))
        out = net(x)
        feats = [out[k] for k in outs if out[k].requires_grad]
        if cots is None:
            cots = [torch.randn_like(f) for f in feats]

        def clear():
            for p in params:
                p.grad = None
        name = "backward, fused" if fuse else "backward, unfused"
        res[name] = _row(name, _time(lambda: torch.autograd.backward(feats, cots, retain_graph=True), args.rounds, args.warmup, before=clear))
        del out, feats
    convs = net._train_convs()
    scales = net._fold_scales()
    descs = []
    for c in convs:
        O, I, k, _ = c.weight.shape
        dw = torch.randn((O, k, k, I), device="cuda").permute(0, 3, 1, 2) if k == 3 else torch.randn((O, I), device="cuda")
        descs.append((dw, torch.zeros_like(c.weight), scales[id(c)]))
    res["unfold"] = _row(f"unfold ({len(descs)} convs)", _time(lambda: ops.frozen_wgrad_unfold(descs), args.rounds, args.warmup))

    def touch():
        with torch.no_grad():
            for c in convs:
                c.weight.mul_(1.0)                                      # a new version, as an optimiser step leaves
    res["refold"] = _row("refold", _time(lambda: net._prepare(), args.rounds, args.warmup, before=touch))

    sd, keys = _state(net, torch.float32, "cuda", freeze_at)
    res["torch forward"] = _row("torch forward", _time(lambda: torch_resnet(x, sd, counts, outs), args.rounds, args.warmup))
    tout = torch_resnet(x, sd, counts, outs)
    tfeats = [tout[k] for k in outs if tout[k].requires_grad]

    def tclear():
        for k in keys:
            sd[k].grad = None
    res["torch backward"] = _row("torch backward", _time(lambda: torch.autograd.backward(tfeats, cots, retain_graph=True), args.rounds, args.warmup,
                                                         before=tclear))
    return res


# ------------------------------------------------------------------------------------------------ deviation at >= 8192 pixels
def deviation():
    outs, counts, freeze_at = ["res2", "res3"], [3, 4], 1
    net = make_net(seed=5, depth=50, out_features=outs)
    x = torch.randn((1, 3, 512, 1024), generator=torch.Generator().manual_seed(6))
    g = torch.Generator().manual_seed(7)
    cot = {"res2": torch.randn((1, 256, 128, 256), generator=g), "res3": torch.randn((1, 512, 64, 128), generator=g)}

    def ref(dtype):
        sd, keys = _state(net, dtype, "cpu", freeze_at)
        f = torch_resnet(x.to(dtype), sd, counts, outs)
        sum((f[k] * cot[k].to(dtype)).sum() for k in outs).backward()
        return {k: v.detach() for k, v in f.items()}, {k: sd[k].grad for k in keys}
    f64, g64 = ref(torch.float64)
    f32, g32 = ref(torch.float32)
    gnet = net.cuda().trainable_(freeze_at)
    out = gnet(x.cuda())
    sum((out[k] * cot[k].cuda()).sum() for k in outs).backward()
    rel = lambda a, b: ((a.detach().double().cpu() - b).norm() / b.norm()).item()
    rows = {}
    print("deviation from float64 (relative L2), res3 at 8192 pixels: HIP  |  torch CPU fp32")
    for k in outs:
        rows[k] = (rel(out[k], f64[k]), rel(f32[k], f64[k]))
    for k, p in gnet.named_parameters():
        if p.grad is not None:
            rows[k] = (rel(p.grad, g64[k]), rel(g32[k], g64[k]))
    for k, (a, b) in rows.items():
        print(f"  {k:28s} {a:.3e}  |  {b:.3e}", flush=True)
    worst = max(rows, key=lambda k: rows[k][0] / rows[k][1])
    print(f"  largest ratio: {rows[worst][0] / rows[worst][1]:.2f} x ({worst})")
    return {k: {"hip": a, "cpu_fp32": b} for k, (a, b) in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1344)
    ap.add_argument("--deviation", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resnet_train_bench needs a GPU"
    import afigan_amd  # noqa: F401
    res = {}
    if not args.no_timing:
        res["timing"] = bench(args)
    if args.deviation:
        res["deviation"] = deviation()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
