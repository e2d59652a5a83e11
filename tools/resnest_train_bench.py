"""Times the trainable ResNeSt bottom-up: forward + backward of res3..res5 of ResNeSt-50 and -101 at the pyramid of a
2 x 800 x 1344 input (res2's output, 2 x 256 x 200 x 336, goes in), against a torch-eager restatement on the same GPU (grouped F.conv2d on the
folded weights, F.avg_pool2d, softmax; autograd's backward), and each new kernel alone against the 6.29 TB/s copy rate DESIGN 26 measured.

Device events, the median of 20 runs after 3 warm-ups (min / max beside it).  No figure is a pass criterion: the table goes into DESIGN 28.

    python tools/resnest_train_bench.py [--depths 50 101] [--runs 20] [--warmup 3] [--no-eager]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import afigan_amd as amd  # noqa: E402
from afigan_amd import ops, resnest_backbone  # noqa: E402

COPY_RATE = 6.29e12                      # bytes / s: DESIGN 26's float4 copy on this GPU


def timed(fn, runs, warmup):
    """(median, min, max) milliseconds of fn() by device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def fill(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, b in net.named_buffers():
            if k.endswith(".weight") or k.endswith(".running_var"):
                b.copy_(0.75 + 0.5 * torch.rand(b.shape, generator=g))
            elif k.endswith(".bias") or k.endswith(".running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=g))
        for k, p in net.named_parameters():
            if ".conv3." in k:
                p.mul_(0.25)


# ---- the torch-eager restatement on the module's own folded weights (leaves of their own, so autograd computes every gradient the HIP path does)
def eager_block(x, w, blk):
    cv = lambda t, name, **kw: F.conv2d(t, w[name + ".w"], w[name + ".b"], **kw)
    if blk.shortcut is not None:
        xs = F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False) if blk.stride == 2 else x
        sc = cv(xs, "shortcut")
    else:
        sc = x
    y = torch.relu(cv(x, "conv1"))
    y = torch.relu(cv(y, "conv", padding=1, groups=2))
    C = y.shape[1] // 2
    s0, s1 = y[:, :C], y[:, C:]
    g = (s0 + s1).mean((2, 3), keepdim=True)
    z = cv(torch.relu(cv(g, "fc1")), "fc2")
    a = torch.softmax(z.view(-1, 2, C), dim=1)
    y = a[:, 0].reshape(-1, C, 1, 1) * s0 + a[:, 1].reshape(-1, C, 1, 1) * s1
    if blk.avd:
        y = F.avg_pool2d(y, 3, 2, padding=1)
    return torch.relu(cv(y, "conv3") + sc)


def eager_weights(net):
    f = net._prepare()
    out = []
    for blk in net._train_blocks():
        (wc, bc), (w1, b1), (w2, b2) = f[id(blk.conv2)]
        w = {"conv.w": wc, "conv.b": bc, "fc1.w": w1[:, :, None, None], "fc1.b": b1, "fc2.w": w2[:, :, None, None], "fc2.b": b2}
        for name in ("conv1", "conv3", "shortcut"):
            m = getattr(blk, name)
            if m is not None:
                w[name + ".w"], w[name + ".b"] = f[id(m)][0][:, :, None, None], f[id(m)][1]
        out.append({k: v.detach().clone().contiguous(memory_format=torch.channels_last if v.dim() == 4 else torch.contiguous_format)
                    .requires_grad_(not k.endswith(".b") or k.startswith("fc")) for k, v in w.items()})
    return out


def bench_depth(depth, runs, warmup, eager):
    torch.manual_seed(depth)
    net = resnest_backbone.ResNeSt(depth=depth, out_features=("res3", "res4", "res5"), norm="FrozenBN", freeze_at=2)
    fill(net, depth)
    net = net.cuda().trainable_(2)
    params = [c.weight for c, _ in net._train_convs()] + net._train_fc()
    g = torch.Generator().manual_seed(1)
    x = torch.relu(torch.randn((2, 256, 200, 336), generator=g)).cuda().contiguous(memory_format=torch.channels_last)
    shapes = [(2, 512, 100, 168), (2, 1024, 50, 84), (2, 2048, 25, 42)]
    cots = [torch.randn(s, generator=g).cuda().contiguous(memory_format=torch.channels_last) for s in shapes]

    def hip():
        for p in params:
            p.grad = None
        outs = resnest_backbone._ResNeStTrainFn.apply(net, x, *params)
        torch.autograd.backward(outs, cots)

    def hip_fwd():
        with torch.no_grad():
            resnest_backbone._ResNeStTrainFn.apply(net, x, *params)
    rows = [(f"ResNeSt-{depth} res3..res5 forward + backward, HIP", timed(hip, runs, warmup)),
            (f"ResNeSt-{depth} res3..res5 forward alone (keeping activations), HIP", timed(hip_fwd, runs, warmup))]
    if eager:
        ws = eager_weights(net)
        blocks = net._train_blocks()
        ends = set()
        n = 0
        for name in net._train_stages:
            n += len(getattr(net, name))
            ends.add(n - 1)

        def torch_eager():
            for w in ws:
                for t in w.values():
                    t.grad = None
            y, outs = x, []
            for i, (blk, w) in enumerate(zip(blocks, ws)):
                y = eager_block(y, w, blk)
                if i in ends:
                    outs.append(y)
            torch.autograd.backward(outs, cots)
        rows.append((f"ResNeSt-{depth} res3..res5 forward + backward, torch eager (folded weights)", timed(torch_eager, runs, warmup)))
    return rows


def bench_kernels(runs, warmup):
    """each new kernel alone at res3's split-attention shape (N 2, C 128, 100 x 168; with AVD the first block's), bytes = what it must move"""
    N, C, I, H, W = 2, 128, 64, 100, 168
    g = torch.Generator().manual_seed(2)
    pm = lambda *s: torch.randn(s, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    s0, s1 = torch.relu(pm(N, C, H, W)), torch.relu(pm(N, C, H, W))
    w1, b1, w2, b2 = [torch.randn(s, generator=g).cuda() * 0.1 for s in ((I, C), (I,), (2 * C, I), (2 * C,))]
    s1s = torch.ones(I).cuda()
    rows = []
    split = N * C * H * W * 4
    for avd in (False, True):
        Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if avd else (H, W)
        dout = pm(N, C, Ho, Wo)
        _, att, gm, h = ops.splat_attention(s0, s1, w1, b1, w2, b2, avd=avd, keep=True)
        part = ops.splat_bwd_dots(dout, s0, s1, avd)
        dz, dh, dg = ops.splat_bwd_attn(part, (H, W), att, h, w1, w2)
        ds0, ds1 = ops.new_pixel_major(N, C, H, W, "cuda"), ops.new_pixel_major(N, C, H, W, "cuda")
        dbytes = dout.numel() * 4
        rows.append((f"afi_resnest_splat_bwd_dots avd={int(avd)}", timed(lambda: ops.splat_bwd_dots(dout, s0, s1, avd), runs, warmup), 2 * split + dbytes))
        rows.append((f"afi_resnest_splat_bwd_combine avd={int(avd)}",
                     timed(lambda: ops.splat_bwd_combine(dout, s0, s1, att, dg, avd, ds0, ds1), runs, warmup), 4 * split + dbytes))
    rows.append(("afi_resnest_splat_bwd_attn (one block per image)", timed(lambda: ops.splat_bwd_attn(part, (H, W), att, h, w1, w2), runs, warmup),
                 (w1.numel() + w2.numel()) * 4 * N + part.numel() * 4))
    grads = [torch.zeros_like(t) for t in (w1, b1, w2, b2)]
    rows.append(("afi_resnest_splat_bwd_params", timed(lambda: ops.splat_bwd_params(dz, dh, gm, h, s1s, *grads), runs, warmup),
                 2 * (w1.numel() + w2.numel()) * 4))
    x = torch.relu(pm(N, 256, 2 * H, 2 * W))
    dy, dx = pm(N, 256, H, W), pm(N, 256, 2 * H, 2 * W)
    for mode in ("avg2s2_ceil", "avg3s2p1"):
        rows.append((f"afi_resnest_pool_bwd {mode} beta=1 with mask (2 x 256 x 200 x 336)",
                     timed(lambda: ops.resnest_pool_bwd(dy, mode, dx=dx, beta=1.0, z=x), runs, warmup), (3 * dx.numel() + dy.numel()) * 4))
    big = torch.empty(64 * 1024 * 1024, device="cuda")
    dst = torch.empty_like(big)
    rows.append(("torch copy of 256 MiB (the yardstick, read + write)", timed(lambda: dst.copy_(big), runs, warmup), 2 * big.numel() * 4))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", type=int, nargs="*", default=[50, 101])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times kernels on the GPU"
    print(f"library build {amd._lib.build_id()[:16]}, {torch.cuda.get_device_name(0)}, median of {a.runs} after {a.warmup} warm-ups (min / max)")
    print("| what | ms, median (min / max) | |")
    print("|---|---|---|")
    for name, (med, lo, hi), nbytes in bench_kernels(a.runs, a.warmup):
        rate = nbytes / (med * 1e-3)
        print(f"| {name} | {med:.4f} ({lo:.4f} / {hi:.4f}) | {rate / 1e9:.0f} GB/s, {100 * rate / COPY_RATE:.0f} % of the copy rate |")
    for depth in a.depths:
        rows = bench_depth(depth, a.runs, a.warmup, not a.no_eager)
        for name, (med, lo, hi) in rows:
            print(f"| {name} | {med:.2f} ({lo:.2f} / {hi:.2f}) | |", flush=True)
        if len(rows) == 3:
            print(f"| ResNeSt-{depth}: torch eager / HIP | {rows[2][1][0] / rows[0][1][0]:.2f} x | |", flush=True)


if __name__ == "__main__":
    main()
