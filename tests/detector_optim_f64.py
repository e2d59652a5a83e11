"""The detector's optimiser step restated in fp64 (the yardstick of test_gpu_detector_optim.py, itself held to torch.optim.SGD in
test_detector_optim_host.py): detectron2 v0.1.1's build_optimizer groups, WarmupMultiStepLR, and torch.optim.SGD's update evaluated in
double from the fp32 inputs -- parameter, gradient, momentum buffer and the fp32-rounded scalars the kernel receives."""
from bisect import bisect_right

import numpy as np
import torch

U = 2.0 ** -24                         # fp32 unit roundoff
SLACK = 1.0 + 2.0 ** -20               # second-order terms of the bounds below


def group(name, base_lr=0.001, weight_decay=1e-4, weight_decay_norm=0.0, bias_lr_factor=1.0, weight_decay_bias=1e-4):
    """(lr, weight_decay) of a parameter by its key (solver/build.py: build_optimizer)."""
    lr, wd = base_lr, weight_decay
    if name.endswith("norm.weight") or name.endswith("norm.bias"):
        wd = weight_decay_norm
    elif name.endswith(".bias"):
        lr, wd = base_lr * bias_lr_factor, weight_decay_bias
    return lr, wd


def schedule(it, steps=(30000,), gamma=0.1, warmup_factor=1e-3, warmup_iters=1000):
    """WarmupMultiStepLR.get_lr() / base_lr at iteration `it` (solver/lr_scheduler.py, linear warm-up)."""
    w = 1.0
    if it < warmup_iters:
        alpha = it / warmup_iters
        w = warmup_factor * (1 - alpha) + alpha
    return w * gamma ** bisect_right(sorted(steps), it)


def f32(x):
    return float(np.float32(x))


def sgd(p, g, m, lr, wd, momentum, gscale=1.0):
    """One torch.optim.SGD update in double: d = g gscale + wd p; m' = momentum m + d; p' = p - lr m'.  p, g, m: fp32 tensors (m None: zeros);
    the scalars are rounded to fp32 first, as the kernel's arguments are.  Returns (p', m', M), M = |momentum m| + |gscale g| + |wd p|."""
    lr, wd, momentum, gscale = f32(lr), f32(wd), f32(momentum), f32(gscale)
    p, g = p.detach().double().cpu(), g.detach().double().cpu()
    m = torch.zeros_like(p) if m is None else m.detach().double().cpu()
    d = g * gscale + wd * p
    m1 = momentum * m + d
    return p - lr * m1, m1, (momentum * m).abs() + (gscale * g).abs() + (wd * p).abs()


def bounds(p0, m1, lr, M):
    """(bound on |m - m64|, bound on |p - p64|) of one fp32 step: the count of roundings, with or without contraction.  m: the product
    g gscale, the sum d and the sum m', each relative to at most M: 3u M, taken as 4u M.  p: the rounding of p' itself, u |p'| <=
    u (|p0| + lr |m'|), taken twice for the product lr m' without contraction, plus lr times m's error."""
    lr = f32(lr)
    bm = 4 * U * M
    bp = (2 * U * (p0.detach().double().cpu().abs() + lr * m1.abs()) + 4 * U * lr * M) * SLACK
    return bm, bp


def trajectory(p0, grads, lrs, wd, momentum, gscale=1.0):
    """`len(grads)` steps in double from the fp32 p0 and m = 0, with the bounds of one step accumulated: an error of p or m that a step inherits
    goes through the step's own linear map (m' = momentum m + wd p + .., p' = p - lr m').  Returns (p, m, bound_p, bound_m)."""
    p, m = p0.detach().double().cpu(), torch.zeros_like(p0, dtype=torch.float64, device="cpu")
    ep, em = torch.zeros_like(p), torch.zeros_like(p)
    mo, w = f32(momentum), f32(wd)
    for g, lr in zip(grads, lrs):
        l, gs = f32(lr), f32(gscale)
        M = (mo * m).abs() + (gs * g.detach().double().cpu()).abs() + (w * p).abs()
        m1 = mo * m + gs * g.detach().double().cpu() + w * p
        em = (mo * em + w * ep + 4 * U * M) * SLACK
        ep = (ep + l * em + 2 * U * (p.abs() + l * m1.abs())) * SLACK
        p, m = p - l * m1, m1
    return p, m, ep, em
