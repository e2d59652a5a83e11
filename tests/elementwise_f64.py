"""float64 yardsticks, launch geometry and case tables of the bandwidth passes in afigan_amd/csrc/elementwise.hip: BatchNorm statistics, apply
and backward, column sums, BCE, L1, bilinear x2 and the SGD step.  tests/test_elementwise_host.py holds this module to torch's own float64
ops and to the branch every case names; tests/test_gpu_elementwise.py compares the kernels with it.

Every reference takes the kernel's fp32 INPUTS (tensors and scalars: a scalar is rounded to fp32 first, as the C-ABI's `float` arguments are)
and evaluates the operation in float64.  Nothing here touches a GPU."""
import math

import numpy as np
import torch

from oracle import afigan_oracle as orc

EPS = 2.0 ** -24                # unit roundoff of fp32
F32_MIN_NORMAL = 2.0 ** -126    # below it a result is rounded to the subnormal grid (or flushed): the absolute floor of every elementwise bar


def f32(v):
    """a python scalar as the kernel receives it: rounded to fp32, held in a python float"""
    return float(np.float32(v))


def d(t):
    return t.detach().double()


# ------------------------------------------------------------------------------------------------ launch geometry (pure functions)
EW_GRID_CAP = 2048              # afi_ew_grid: 256 CUs x 8 blocks
RED_MAX_CHUNKS = 256            # AFI_RED_MAX_CHUNKS
BCE_GRID_CAP = 256              # afi_launch_bce_logits
SGD_GRID_CAP = 512              # afi_launch_sgd (x ntensors in grid.y)
BLOCK = 256


def ew_grid(work_items):
    """csrc/elementwise.hip: afi_ew_grid -- blocks of 256 threads, capped, at least one"""
    return max(1, min(EW_GRID_CAP, (work_items + 255) // 256))


def red_geometry(P):
    """csrc/elementwise.hip: afi_red_geometry -- (chunks, rows_per_chunk) of the per-channel reductions"""
    want = max(1, min(RED_MAX_CHUNKS, (P + 63) // 64))
    rpc = (P + want - 1) // want
    return (P + rpc - 1) // rpc, rpc


def bce_grid(n):
    """csrc/elementwise.hip: afi_launch_bce_logits -- ceil(n / 256) blocks, capped at 256"""
    return min(BCE_GRID_CAP, (n + 255) // 256)


def sgd_grid(max_n, ntensors):
    """csrc/elementwise.hip: afi_launch_sgd -- (ceil(max_n / 256) capped at 512, one row of blocks per tensor)"""
    return max(1, min(SGD_GRID_CAP, (max_n + 255) // 256)), ntensors


BRANCHES = ("hoisted", "fallback", "main_loop", "grid_stride")
UNROLL = {"bn_apply": 4, "bn_bwd_apply": 2}      # afi_bn_apply_lrelu_kernel: four loads in flight; afi_bn_bwd_apply_kernel: two pairs


def branch_of(op, P, C):
    """Which of BRANCHES the launch of `op` on P rows of C channels takes, as a frozenset.
    bn_apply / bn_bwd_apply (afi_bn_apply_lrelu_kernel / afi_bn_bwd_apply_kernel): total4 = P*C/4 float4 items on ew_grid(total4) blocks;
    `hoisted` where stride % (C/4) == 0, else `fallback`; `grid_stride` where some thread takes a second item; `main_loop` where the hoisted
    branch's unrolled loop runs at least once (thread 0: i + (U-1)*stride < total4).
    The flat ops have one loop: `grid_stride` or nothing.  Their work items, as their launchers count them --
    bce: P = n, C = 1;  sgd: P = max_n, C = 1;  l1: P = N*Ha*Wa, C (float4 items);  bilinear_fwd: P = N*H*W INPUT pixels, C (the launcher sizes
    the grid by N*H*W*C, which is the number of OUTPUT float4 items);  bilinear_bwd: P = N*H*W input pixels, C (float4 items)."""
    if op in UNROLL:
        total4 = P * C // 4
        stride = BLOCK * ew_grid(total4)
        out = set()
        hoisted = stride % (C // 4) == 0
        out.add("hoisted" if hoisted else "fallback")
        if total4 > stride:
            out.add("grid_stride")
        if hoisted and total4 > (UNROLL[op] - 1) * stride:
            out.add("main_loop")
        return frozenset(out)
    if op == "bce":
        items, threads = P, BLOCK * bce_grid(P)
    elif op == "sgd":
        items, threads = P, BLOCK * sgd_grid(P, 1)[0]
    elif op in ("l1", "bilinear_bwd"):
        items = P * C // 4
        threads = BLOCK * ew_grid(items)
    elif op == "bilinear_fwd":
        items = 4 * P * C // 4
        threads = BLOCK * ew_grid(P * C)
    else:
        raise KeyError(op)
    return frozenset({"grid_stride"}) if items > threads else frozenset()


RED_PATHS = ("one_chunk", "multi_chunk", "partial_last_chunk", "chunk_cap", "finalize_unrolled", "idle_lanes", "partial_channel_block")


def red_path_of(P, C):
    """What a [P][C] per-channel reduction exercises (afi_bn_stats_partial_kernel / afi_colred_partial_kernel + their finalizers):
    one chunk or several; a last chunk shorter than the others; the want > 256 cap; more than 24 chunks, where the fp64 finalizer's
    4-in-flight loop runs (8 lanes per channel: i + 24 < chunks); fewer rows in a chunk than its 8 row lanes; C % 128 != 0 (channel quads
    of the last block masked off)."""
    chunks, rpc = red_geometry(P)
    out = {"one_chunk" if chunks == 1 else "multi_chunk"}
    if P % rpc:
        out.add("partial_last_chunk")
    if (P + 63) // 64 > RED_MAX_CHUNKS:
        out.add("chunk_cap")
    if chunks > 24:
        out.add("finalize_unrolled")
    if min(rpc, P - (chunks - 1) * rpc) < 8:
        out.add("idle_lanes")
    if C % 128:
        out.add("partial_channel_block")
    return frozenset(out)


def add_chain_depth(P):
    """the longest chain of additions a reduction over P rows runs through: rows per lane + 8 lanes + chunks / 8 + 8 -- the worst-case
    bound of a reduction is depth * 2^-24 * sum|terms|, which no bar here may exceed"""
    chunks, rpc = red_geometry(P)
    return (rpc + 7) // 8 + 8 + (chunks + 7) // 8 + 8


# ------------------------------------------------------------------------------------------------ case tables
def S(*names):
    return frozenset(names)


# BatchNorm statistics / backward sums / column sums: (P, C, what the case is there for)
STATS_SHAPES = [
    (1, 4, S("one_chunk", "idle_lanes", "partial_channel_block")),                              # P = 1: var = 0, unbiased factor 1 / max(P-1, 1)
    (7, 8, S("one_chunk", "idle_lanes", "partial_channel_block")),                              # P < 8: a row lane without rows
    (77, 132, S("multi_chunk", "partial_last_chunk", "partial_channel_block")),                 # 2 chunks (39 + 38), C = 128 + 4: a second channel block
    (1537, 64, S("multi_chunk", "partial_last_chunk", "finalize_unrolled", "partial_channel_block")),   # 25 chunks: the 4-in-flight finalize loop
    (16385, 16, S("multi_chunk", "partial_last_chunk", "chunk_cap", "finalize_unrolled", "idle_lanes", "partial_channel_block")),  # want 257 -> 256:
                                                                                                # 253 chunks of 65 rows, the last of 5
]
STATS_FAMILIES = ("unit", "offset_1e4", "offset_5e3", "tiny", "row0_outlier", "const_channel")
CONST_VALUE = 3.25


def stats_input(family, P, C, seed=0):
    """the fp32 [P][C] input of a statistics case.  const_channel: channel 1 is 3.25 in every row (var == 0 exactly: K = x[0][c] = 3.25)"""
    g = torch.Generator().manual_seed(1000 + seed)
    r = torch.randn((P, C), generator=g)
    if family == "unit":
        return r
    if family == "offset_1e4":
        return (1e4 + 0.1 * r).float()
    if family == "offset_5e3":
        return (5e3 + 1e3 * r).float()
    if family == "tiny":
        return (1e-3 * r).float()
    if family == "row0_outlier":
        r[0] = 1e3
        return r
    if family == "const_channel":
        r[:, 1] = CONST_VALUE
        return r
    raise KeyError(family)


# BatchNorm apply and backward apply: (P, C, branches of bn_apply, branches of bn_bwd_apply)
APPLY_SHAPES = [
    (77, 12, S("fallback"), S("fallback")),                                                     # C/4 = 3, one block
    (100, 96, S("fallback"), S("fallback")),                                                    # C/4 = 24, 10 blocks: stride 2560 % 24 != 0
    (4100, 512, S("hoisted", "grid_stride"), S("hoisted", "grid_stride", "main_loop")),         # 524800 float4 on 524288 threads: 512 threads take two
    (5500, 384, S("fallback", "grid_stride"), S("fallback", "grid_stride")),                    # C/4 = 96 does not divide 524288
    (16500, 512, S("hoisted", "grid_stride", "main_loop"), S("hoisted", "grid_stride", "main_loop")),   # 2112000 float4: every thread runs apply's
                                                                                                # 4-way loop once, the first 14848 also its tail
]

# flat ops: (op, P, C as branch_of counts them, branch)
BCE_N = [(1, S()), (255, S()), (70001, S("grid_stride"))]                                     # 70001 > 256 blocks x 256
L1_SHAPES = [((2, 16, 14, 22), S()), ((2, 128, 96, 96), S("grid_stride"))]                      # a's full extent (N, C, Ha, Wa)
BILINEAR_FWD_SHAPES = [((1, 4, 1, 1), S()), ((2, 8, 1, 7), S()), ((2, 8, 5, 1), S()), ((1, 12, 5, 7), S()), ((1, 64, 96, 96), S("grid_stride"))]
BILINEAR_BWD_SHAPES = [((1, 4, 1, 1), S()), ((2, 8, 1, 7), S()), ((2, 8, 5, 1), S()), ((1, 12, 5, 7), S()), ((1, 256, 96, 96), S("grid_stride"))]
SGD_SIZES = (1, 1000, 131077)                                                                   # 131077 > 512 x 256: grid-stride on the last tensor
SGD_BRANCH = S("grid_stride")


# ------------------------------------------------------------------------------------------------ float64 references
def bn_stats(x, eps, momentum=None, running_mean=None, running_var=None):
    """x [P][C] fp32 -> dict of float64 mean, var (biased), invstd and, given the running buffers, their updates (unbiased variance with
    P / max(P - 1, 1), torch.nn.BatchNorm2d's train mode)"""
    x = d(x)
    P = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    out = {"mean": mean, "var": var, "invstd": 1.0 / torch.sqrt(var + f32(eps))}
    if running_mean is not None:
        m = f32(momentum)
        out["running_mean"] = (1.0 - m) * d(running_mean) + m * mean
        out["running_var"] = (1.0 - m) * d(running_var) + m * var * (P / max(P - 1, 1))
    return out


def bn_stats_shifted_one_pass(x, order="plain"):
    """float64 emulation of the kernel's form: K = row 0, s0 = sum (x - K), s1 = sum (x - K)^2, mean = K + s0/P, var = max(s1/P - (s0/P)^2, 0).
    order: `plain` (torch's pairwise sum), `serial` (row after row), `kernel` (8 row lanes per chunk, then chunks: afi_bn_stats_partial_kernel)"""
    x = d(x)
    P = x.shape[0]
    K = x[0]
    dd = x - K
    if order == "plain":
        s0, s1 = dd.sum(0), (dd * dd).sum(0)
    elif order == "serial":
        s0, s1 = torch.zeros_like(K), torch.zeros_like(K)
        for r in range(P):
            s0 = s0 + dd[r]; s1 = s1 + dd[r] * dd[r]
    elif order == "kernel":
        chunks, rpc = red_geometry(P)
        s0, s1 = torch.zeros_like(K), torch.zeros_like(K)
        for ch in range(chunks):
            blk = dd[ch * rpc:min((ch + 1) * rpc, P)]
            c0, c1 = torch.zeros_like(K), torch.zeros_like(K)
            for lane in range(8):
                rows = blk[lane::8]
                c0 = c0 + rows.sum(0); c1 = c1 + (rows * rows).sum(0)
            s0 = s0 + c0; s1 = s1 + c1
    else:
        raise KeyError(order)
    dm = s0 / P
    return K + dm, torch.clamp(s1 / P - dm * dm, min=0.0)


def bn_apply(x, mean, invstd, gamma, beta, slope):
    """(y, terms): y = lrelu_slope((x - mean) * invstd * gamma + beta); terms = |x - mean| * invstd * |gamma| + |beta| per element"""
    t = (d(x) - d(mean)) * d(invstd) * d(gamma)
    z = t + d(beta)
    s = f32(slope)
    return torch.where(z > 0, z, z * s), t.abs() + d(beta).abs()


def bn_bwd_sums(g, x, mean, invstd):
    """(sum g, sum g * xhat) over the rows, xhat = (x - mean) * invstd with the KERNEL's fp32 mean / invstd"""
    xh = (d(x) - d(mean)) * d(invstd)
    return d(g).sum(0), (d(g) * xh).sum(0)


def bn_bwd_dx(g, x, mean, invstd, gamma, s0, s1, Pn):
    """(dx, terms): dx = gamma * invstd * (g - s0/Pn - xhat * s1/Pn); terms = |gamma invstd| * (|g| + |s0/Pn| + |xhat s1/Pn|)"""
    xh = (d(x) - d(mean)) * d(invstd)
    a, b, c = d(g), d(s0) / Pn, xh * (d(s1) / Pn)
    k = d(gamma) * d(invstd)
    return k * (a - b - c), k.abs() * (a.abs() + b.abs() + c.abs())


def colsum(g):
    """column sums of a [P][C] matrix (any row stride)"""
    return d(g).sum(0)


def bce_logits(z, target):
    """(loss, dz, terms of dz): BCE-with-logits (mean) against the constant target; dz = (sigmoid(z) - t) / n"""
    z = d(z).flatten()
    t = f32(target)
    n = z.numel()
    per = torch.clamp(z, min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
    sig = torch.sigmoid(z)
    return per.sum() / n, (sig - t) / n, (sig + abs(t)) / n


def l1_crop(a, b):
    """(loss, da): mean |a - b| over the common crop [N, C, h, w] from the origin; da = sign(a - b) / n inside it, 0 over the rest of a's extent"""
    h, w = min(a.shape[2], b.shape[2]), min(a.shape[3], b.shape[3])
    df = d(a)[:, :, :h, :w] - d(b)[:, :, :h, :w]
    n = df.numel()
    da = torch.zeros(a.shape, dtype=torch.float64)
    da[:, :, :h, :w] = torch.sign(df) / n
    return df.abs().sum() / n, da


def _bil_axis(v, dim):
    """the x2 bilinear map along one axis: out[o] = v[i0[o]] * (1 - lam[o]) + v[i1[o]] * lam[o]  (orc.bilinear2x_index_map)"""
    i0, i1, lam = orc.bilinear2x_index_map(v.shape[dim])
    shape = [1] * v.dim()
    shape[dim] = -1
    lam = lam.double().view(shape)
    return v.index_select(dim, i0) * (1.0 - lam) + v.index_select(dim, i1) * lam


def _bil_axis_T(v, dim):
    """its transpose: in[i] = sum over o of ((i0[o] == i) * (1 - lam[o]) + (i1[o] == i) * lam[o]) * v[o]"""
    L = v.shape[dim] // 2
    i0, i1, lam = orc.bilinear2x_index_map(L)
    shape = [1] * v.dim()
    shape[dim] = -1
    lam = lam.double().view(shape)
    size = list(v.shape)
    size[dim] = L
    out = torch.zeros(size, dtype=torch.float64)
    out.index_add_(dim, i0, v * (1.0 - lam))
    out.index_add_(dim, i1, v * lam)
    return out


def bilinear2x(x):
    """(out, terms): F.interpolate(scale_factor=2, mode="bilinear") of NCHW x; terms = the same map of |x|"""
    f = lambda v: _bil_axis(_bil_axis(v, 2), 3)
    return f(d(x)), f(d(x).abs())


def bilinear2x_T(dout):
    """(dx, terms): the transpose of bilinear2x applied to NCHW dout [N, C, 2H, 2W]"""
    f = lambda v: _bil_axis_T(_bil_axis_T(v, 3), 2)
    return f(d(dout)), f(d(dout).abs())


def sgd_step(p, g, m, lr, momentum, wd, gscale):
    """torch.optim.SGD with momentum and weight decay on existing buffers: dd = g*gscale + wd*p; m' = momentum*m + dd; p' = p - lr*m'.
    Returns (p', m', terms of p', terms of m')."""
    lr, momentum, wd, gscale = f32(lr), f32(momentum), f32(wd), f32(gscale)
    p, g, m = d(p), d(g), d(m)
    m2 = momentum * m + (g * gscale + wd * p)
    tm = (momentum * m).abs() + (g * gscale).abs() + (wd * p).abs()
    return p - lr * m2, m2, p.abs() + lr * tm, tm


# ------------------------------------------------------------------------------------------------ bars
def ulps_from(got, ref64):
    """distance of fp32 `got` from the fp32 rounding of float64 `ref64`, in fp32 ulps of that rounding (0: equal, 1: its neighbour)"""
    r = ref64.float()
    got = got.detach().float().cpu()
    up, dn = torch.nextafter(r, torch.full_like(r, math.inf)), torch.nextafter(r, torch.full_like(r, -math.inf))
    ulp = torch.maximum(up - r, r - dn).double()              # (the wider side at a power of two: a neighbour on either side counts as 1)
    return ((got.double() - r.double()).abs() / ulp)


def elementwise_bar(terms, r):
    """(r + 1) * 2^-24 * sum|terms| per element: r roundings, each bounded by 2^-24 of the magnitude it rounds, plus one for the second-order
    terms; never below (r + 1) * 2^-126, the smallest normal fp32 (a result below it is rounded to the subnormal grid or flushed to zero)"""
    return (r + 1) * (EPS * terms + F32_MIN_NORMAL)


C_MAX = 2.0     # tests/test_gpu_pixgemm.py: max-norm bar C_MAX * sqrt(Ktot) * 2^-24 * max|ref|
R_L2 = 4.0      # rel. L2 bar R_L2 * max(torch CPU fp32's, sqrt(Ktot) * 2^-24 / 8)


def reduction_bars(ktot, cpu_l2):
    return C_MAX * math.sqrt(ktot) * EPS, R_L2 * max(cpu_l2, math.sqrt(ktot) * EPS / 8)


def errs(got, ref64):
    """(max-norm, relative L2) of got against the float64 reference, as tests/test_gpu_pixgemm.py measures them"""
    df = (got.detach().double().cpu() - ref64).flatten()
    r = ref64.flatten()
    return (df.abs().max() / r.abs().max().clamp_min(1e-300)).item(), (df.norm() / r.norm().clamp_min(1e-300)).item()
