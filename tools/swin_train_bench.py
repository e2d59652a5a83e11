"""Times the trainable Swin bottom-up: forward + backward of Swin-T and of the BiFPN config's Swin-L (every parameter trainable,
freeze_at -1, DropPath off so both sides compute the same thing) against the same network in torch.nn.functional with autograd on the same GPU
(tests/swin_train_f64.forward, the restatement of tests/swin_f64.py over parameter leaves, in fp32), and each new kernel alone at Swin-L's
stage-3 shape (N 2, C 384, 112 x 176, window 12, 12 heads: the map of a 2 x 3 x 896 x 1408 batch) against the bytes it must move and the
6.29 TB/s copy rate DESIGN 26 measured.  The kernel rows time the ops.* wrappers as the module calls them (output and workspace allocation
from torch's caching allocator included; the rows named "clone" include the clone): upper bounds for the kernels themselves.

Device events, the median of 20 runs after 3 warm-ups (min / max beside it).  No figure is a pass criterion: the tables go into DESIGN 29.

    python tools/swin_train_bench.py [--nets T L] [--shapes 2x896x1408 2x448x704] [--runs 20] [--warmup 3] [--no-torch] [--no-kernels]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import afigan_amd as amd  # noqa: E402
from afigan_amd import ops, swin_backbone  # noqa: E402
from tools.swin_bench import NETS  # noqa: E402

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


def pm(g, *shape):
    return torch.randn(shape, generator=g).cuda().contiguous(memory_format=torch.channels_last)


def bench_net(net, shape, runs, warmup, with_torch):
    """rows (name, (median, min, max)) of one network at one N x H x W"""
    import swin_f64 as S
    import swin_train_f64 as T
    c = NETS[net]
    N, H, W = (int(v) for v in shape.split("x"))
    m = S.fill(swin_backbone.SwinTransformer(c["EMBED_DIM"], c["DEPTHS"], c["NUM_HEADS"], c["WINDOW_SIZE"], 4.0, c["OUT_FEATURES"])).cuda()
    g = torch.Generator().manual_seed(1)
    x = torch.randn((N, 3, H, W), generator=g).cuda()
    with torch.no_grad():
        shapes = {k: tuple(v.shape) for k, v in m(x).items()}
    cots = {k: pm(g, *s) for k, s in shapes.items()}
    rows = [(f"Swin-{net} {shape} frozen forward, HIP", timed(lambda: m(x), runs, warmup))]
    m.trainable_(-1, 0.0)
    params = m._train_params()

    def hip():
        for p in params:
            p.grad = None
        out = m(x)
        torch.autograd.backward([out[k] for k in cots], [cots[k] for k in cots])

    def hip_fwd():
        m(x)
    rows.append((f"Swin-{net} {shape} forward + backward, HIP", timed(hip, runs, warmup)))
    rows.append((f"Swin-{net} {shape} forward alone (keeping activations), HIP", timed(hip_fwd, runs, warmup)))
    m.trainable_(-1, 0.2).train()
    rows.append((f"Swin-{net} {shape} forward + backward with DropPath 0.2, HIP", timed(hip, runs, warmup)))
    m.trainable_(-1, 0.0)
    if with_torch:
        P = T.leaves(m, torch.float32, "cuda")
        leaves = [v for v in P.values() if v.is_floating_point()]
        tcots = {k: v.contiguous() for k, v in cots.items()}

        def torch_autograd():
            for v in leaves:
                v.grad = None
            out = T.forward(m, P, x)
            torch.autograd.backward([out[k] for k in tcots], [tcots[k] for k in tcots])
        rows.append((f"Swin-{net} {shape} forward + backward, torch autograd", timed(torch_autograd, runs, warmup)))
    return rows


def bench_kernels(runs, warmup):
    """rows (name, (median, min, max), bytes it must move) of each new kernel alone at Swin-L's stage-3 shape"""
    N, C, H, W, ws, heads = 2, 384, 112, 176, 12, 12
    g = torch.Generator().manual_seed(2)
    tok = N * H * W * 4                                     # bytes of one channel over the map
    rows = []
    # LayerNorm backward: <2> at C 384 (norm1 / norm2), <6> the merge of C 384 to 1536, <12> the merge of C 768 to 3072 one stage down
    x, dy, dx = pm(g, N, C, H, W), pm(g, N, C, H, W), pm(g, N, C, H, W)
    gam, dgam, dbet = torch.ones(C).cuda(), torch.zeros(C).cuda(), torch.zeros(C).cuda()
    rows.append(("afi_swin_layernorm_bwd <2> C 384, beta 1, dgamma / dbeta",
                 timed(lambda: ops.swin_layernorm_bwd(dy, x, gam, dx=dx, beta=1.0, dgamma=dgam, dbeta=dbet), runs, warmup), 4 * C * tok))
    rows.append(("afi_swin_layernorm_bwd <2> C 384, dx alone, beta 0", timed(lambda: ops.swin_layernorm_bwd(dy, x, gam, dx=dx), runs, warmup),
                 3 * C * tok))
    for Cm, Hm, Wm in ((C, H, W), (2 * C, H // 2, W // 2)):
        xm, dym = pm(g, N, Cm, Hm, Wm), pm(g, N, 4 * Cm, Hm // 2, Wm // 2)
        gm, dgm, dbm = torch.ones(4 * Cm).cuda(), torch.zeros(4 * Cm).cuda(), torch.zeros(4 * Cm).cuda()
        rows.append((f"afi_swin_layernorm_bwd <{6 if Cm == C else 12}> merge C {Cm} to {4 * Cm} on {Hm} x {Wm}, dgamma / dbeta",
                     timed(lambda: ops.swin_layernorm_bwd(dym, xm, gm, merge=True, dgamma=dgm, dbeta=dbm), runs, warmup), 3 * xm.numel() * 4))
        del xm, dym
    # GELU backward in place on the gradient, the MLP's 4 C channels
    h, dh = pm(g, N, 4 * C, H, W), pm(g, N, 4 * C, H, W)
    rows.append(("afi_swin_gelu_bwd in place, 4 C = 1536", timed(lambda: ops.swin_gelu_bwd(dh, h, out=dh), runs, warmup), 3 * 4 * C * tok))
    del h, dh
    # window attention backward, shifted (the mask's branch) and not; then the table's gradient from its partials
    qkv, da, qb = pm(g, N, 3 * C, H, W), pm(g, N, C, H, W), 0.2 * torch.randn(3 * C, generator=g).cuda()
    table = 0.5 * torch.randn(((2 * ws - 1) ** 2, heads), generator=g).cuda()
    index = swin_backbone.relative_position_index(ws).cuda()
    img = ops.swin_bias_image(table, index, ws)
    csr = ops.swin_bias_csr(index, ws, table.shape[0])
    for shift in (0, ws // 2):
        dqkv, part = ops.swin_window_attn_bwd(da, qkv, qb, img, ws, shift)
        rows.append((f"afi_swin_window_attn_bwd window 12, shift {shift} ({part.shape[0] // N} groups of windows)",
                     timed(lambda: ops.swin_window_attn_bwd(da, qkv, qb, img, ws, shift), runs, warmup),
                     (qkv.numel() + da.numel() + dqkv.numel() + part.numel()) * 4))
    rows.append((f"afi_swin_window_attn (the forward, shift {ws // 2}, for scale)", timed(lambda: ops.swin_window_attn(qkv, qb, img, ws, ws // 2), runs, warmup),
                 (qkv.numel() + da.numel()) * 4))
    dtab = torch.zeros_like(table)
    rows.append((f"afi_swin_bias_table_bwd ({part.shape[0]} partials of 12 x 144 x 144)", timed(lambda: ops.swin_bias_table_bwd(part, csr, ws, dtab), runs, warmup),
                 part.numel() * 4))
    del qkv, da, dqkv, part
    # DropPath's join and the patch gather of the 2 x 3 x 896 x 1408 batch
    a, b, s = pm(g, N, C, H, W), pm(g, N, C, H, W), torch.tensor([0.0, 1.25]).cuda()
    rows.append(("afi_swin_scale_add C 384", timed(lambda: ops.swin_scale_add(a, s, b), runs, warmup), 3 * C * tok))
    image = torch.randn((N, 3, 8 * H, 8 * W), generator=g).cuda()
    rows.append(("afi_swin_patch_gather 2 x 3 x 896 x 1408", timed(lambda: ops.swin_patch_gather(image), runs, warmup), 2 * image.numel() * 4))
    # what the training forward adds to the frozen one, and what the backward recomputes, per block at this shape
    hh = pm(g, N, 4 * C, H, W)
    rows.append(("torch clone of fc1's pre-activation (run_keep)", timed(lambda: hh.clone(), runs, warmup), 2 * hh.numel() * 4))
    rows.append(("afi_swin_gelu on a clone (the backward's recompute)", timed(lambda: ops.swin_gelu_(hh.clone()), runs, warmup), 4 * hh.numel() * 4))
    rows.append(("afi_swin_layernorm C 384 (the backward's recompute of y1 / y2)", timed(lambda: ops.swin_layernorm(x, gam, dbet), runs, warmup), 2 * C * tok))
    del hh
    big = torch.empty(64 * 1024 * 1024, device="cuda")
    dst = torch.empty_like(big)
    rows.append(("torch copy of 256 MiB (the yardstick, read + write)", timed(lambda: dst.copy_(big), runs, warmup), 2 * big.numel() * 4))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="*", default=["T", "L"], choices=sorted(NETS))
    ap.add_argument("--shapes", nargs="*", default=["2x896x1408", "2x448x704"])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times kernels on the GPU"
    print(f"library build {amd._lib.build_id()[:16]}, {torch.cuda.get_device_name(0)}, median of {a.runs} after {a.warmup} warm-ups (min / max)")
    print("| what | ms, median (min / max) | |")
    print("|---|---|---|")
    if not a.no_kernels:
        for name, (med, lo, hi), nbytes in bench_kernels(a.runs, a.warmup):
            rate = nbytes / (med * 1e-3)
            print(f"| {name} | {med:.4f} ({lo:.4f} / {hi:.4f}) | {nbytes / 1e6:.1f} MB, {rate / 1e9:.0f} GB/s, {100 * rate / COPY_RATE:.0f} % of the copy rate |",
                  flush=True)
        torch.cuda.empty_cache()
    for net in a.nets:
        for shape in a.shapes:
            rows = bench_net(net, shape, a.runs, a.warmup, not a.no_torch)
            for name, (med, lo, hi) in rows:
                print(f"| {name} | {med:.2f} ({lo:.2f} / {hi:.2f}) | |", flush=True)
            if not a.no_torch:
                print(f"| Swin-{net} {shape}: torch autograd / HIP | {rows[-1][1][0] / rows[1][1][0]:.2f} x | |", flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
