"""Float64 reference and fp32 yardstick for the Winograd conv forms (csrc/winograd.hip), shared by tests/test_wino_host.py and
tests/test_gpu_wino.py.  Nothing here touches the library.

restate(op, tiling, x, w_or_dy, dtype) evaluates the 3x3 / stride-1 / pad-1 conv the way the library does -- transform, one batched
channel mix per transform point, inverse transform -- with the matrices of the comments in csrc/winograd.hip (F(4x4): the
interpolation points {0, 1, -1, 1/2, -2, inf}, AFI_WINO4_POINTS == 1), in a torch dtype of the caller's choice:
  float64   a check of the algebra: it must reproduce F.conv2d / autograd in float64 to rounding (test_wino_host.py: 1e-12);
  float32   the yardstick: fp32 transforms around torch.bmm, i.e. what a CORRECT fp32 evaluation of this form loses against fp64.
            The transforms' rounding dominates it (a strictly sequential fp32 sum over k gives the same figures to three digits at
            K = 128 .. 256), so it does not depend on the summation order of the GEMM it is compared with.
reference(op, ...) is F.conv2d / its gradients in float64 on the same fp32 inputs; errors(got, ref) the two norms every bar is stated in.

The bar of the fp32-grade arithmetics (fp32, f16x3, bf16x6), per case and per norm:
    kernel error <= R_WINO * max(error of the fp32 restatement of the case's own tiling, sqrt(Ktot) * 2^-24 / 8)
Ktot = the reduction length (Cin forward, Cout data gradient, tiles for a weight gradient).  R_WINO = 4 is R_L2 of
tests/test_gpu_pixgemm.py: the same yardstick (a correct CPU fp32 evaluation, whose blocked sums round less than an MFMA chain) and the
same floor; the direct kernels measured <= 2.4x there.
"""
import math

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
R_WINO = 4.0
FP32_GRADE = ("fp32", "f16x3", "bf16x6")
TOL_CONV = {"bf16x3": 2e-4, "bf16": 2e-2}          # tests/test_gpu_bf16.py: the two reduced arithmetics keep their own bars
OPS = ("fwd", "dgrad", "wgrad")

_T = 1.0 / 3.0
_F = 1.0 / 15.0
# F(2x2,3x3) / F(3x3,2x2): points {0, 1, -1, inf}; F(4x4,3x3) / F(3x3,4x4): points {0, 1, -1, 1/2, -2, inf}
MATRICES = {
    2: {
        "BT": [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
        "G": [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]],
        "AT": [[1, 1, 1, 0], [0, 1, -1, -1]],
        "Gp": [[1, 0], [0.5, 0.5], [0.5, -0.5], [0, 1]],
        "ApT": [[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, -1]],
    },
    4: {
        "BT": [[1, -1.5, -2, 1.5, 1, 0], [0, -1, 0.5, 2.5, 1, 0], [0, 1, -2.5, 0.5, 1, 0], [0, -2, -1, 2, 1, 0], [0, 0.5, -1, -0.5, 1, 0],
               [0, 1, -1.5, -2, 1.5, 1]],
        "G": [[1, 0, 0], [_T, _T, _T], [-_T, _T, -_T], [-16 * _F, -8 * _F, -4 * _F], [_F, -2 * _F, 4 * _F], [0, 0, 1]],
        "AT": [[1, 1, 1, 1, 1, 0], [0, 1, -1, 0.5, -2, 0], [0, 1, 1, 0.25, 4, 0], [0, 1, -1, 0.125, -8, 1]],
        "Gp": [[1, 0, 0, 0], [_T, _T, _T, _T], [-_T, _T, -_T, _T], [-16 * _F, -8 * _F, -4 * _F, -2 * _F], [_F, -2 * _F, 4 * _F, -8 * _F],
               [0, 0, 0, 1]],
        "ApT": [[1, 1, 1, 1, 1, 0], [0, 1, -1, 0.5, -2, 0], [0, 1, 1, 0.25, 4, 1]],
    },
}


def matrix(tiling, name, dtype=torch.float64):
    """B^T ("BT"), G, A^T ("AT"), G' ("Gp") or A'^T ("ApT") of F(tiling x tiling, 3x3) as a tensor (built in float64, rounded once to dtype)"""
    return torch.tensor(MATRICES[tiling][name], dtype=torch.float64).to(dtype)


def tiles(tiling, N, H, W):
    """tiles of an N x H x W map: the reduction length of a weight gradient in this tiling"""
    return N * ((H + tiling - 1) // tiling) * ((W + tiling - 1) // tiling)


def _patches(x, m):
    """x [N,C,H,W] -> the (m+2) x (m+2) input patches [N,C,Th,Tw,m+2,m+2] of its m x m output tiles; the patch of tile (ty, tx) starts at
    (m ty - 1, m tx - 1), zeros outside the map (the conv's padding, and the empty part of the last tile row / column)"""
    H, W = x.shape[2:]
    Th, Tw = (H + m - 1) // m, (W + m - 1) // m
    xp = F.pad(x, (1, Tw * m + 1 - W, 1, Th * m + 1 - H))
    return xp.unfold(2, m + 2, m).unfold(3, m + 2, m)


def _blocks(y, m):
    """y [N,C,H,W] -> its m x m blocks [N,C,Th,Tw,m,m], zero-padded at the right and bottom edges"""
    H, W = y.shape[2:]
    Th, Tw = (H + m - 1) // m, (W + m - 1) // m
    yp = F.pad(y, (0, Tw * m - W, 0, Th * m - H))
    return yp.unfold(2, m, m).unfold(3, m, m)


def _planes(t):
    """[N,C,Th,Tw,a,b] -> [a*b, N*Th*Tw, C]: one (tiles x channels) matrix per transform point"""
    N, C, Th, Tw, a, b = t.shape
    return t.permute(4, 5, 0, 2, 3, 1).reshape(a * b, N * Th * Tw, C)


def _sandwich(L, t, R):
    """L t R^T on the last two dimensions"""
    return torch.einsum("ij,...jk,lk->...il", L, t, R)


def _forward(m, x, w, dtype):
    N, _, H, W = x.shape
    Cout = w.shape[0]
    BT, G, AT = (matrix(m, k, dtype) for k in ("BT", "G", "AT"))
    d = _patches(x.to(dtype), m)
    Th, Tw = d.shape[2:4]
    V = _planes(_sandwich(BT, d, BT))                                    # [P, T, Cin]
    U = _sandwich(G, w.to(dtype), G).permute(2, 3, 1, 0).reshape((m + 2) ** 2, w.shape[1], Cout)     # [P, Cin, Cout]
    M = torch.bmm(V, U)                                                  # [P, T, Cout]
    M = M.reshape(m + 2, m + 2, N, Th, Tw, Cout).permute(2, 5, 3, 4, 0, 1)
    Y = _sandwich(AT, M, AT)                                             # [N, Cout, Th, Tw, m, m]
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(N, Cout, Th * m, Tw * m)[:, :, :H, :W].contiguous()


def restate(op, tiling, x, w_or_dy, dtype):
    """The Winograd evaluation of `op` on tiling x tiling tiles in `dtype` (CPU tensors in, a `dtype` tensor out):
       "fwd"    x [N,Cin,H,W],  w  [Cout,Cin,3,3]  ->  conv(x, w)                 [N,Cout,H,W]
       "dgrad"  dy [N,Cout,H,W], w  [Cout,Cin,3,3]  ->  d conv / d x  (dy)         [N,Cin,H,W]    flipped taps, swapped roles
       "wgrad"  x [N,Cin,H,W],  dy [N,Cout,H,W]    ->  d <dy, conv(x, w)> / d w   [Cout,Cin,3,3]
                dU = sum_tiles (G' dy G'^T) (x) (B^T d B),  dW = A'^T dU A'"""
    m = tiling
    if op == "fwd":
        return _forward(m, x, w_or_dy, dtype)
    if op == "dgrad":
        return _forward(m, x, w_or_dy.flip(2, 3).transpose(0, 1), dtype)
    if op != "wgrad":
        raise ValueError(op)
    BT, Gp, ApT = (matrix(m, k, dtype) for k in ("BT", "Gp", "ApT"))
    V = _planes(_sandwich(BT, _patches(x.to(dtype), m), BT))             # [P, T, Cin]
    Q = _planes(_sandwich(Gp, _blocks(w_or_dy.to(dtype), m), Gp))        # [P, T, Cout]
    dU = torch.bmm(Q.transpose(1, 2), V)                                 # [P, Cout, Cin]
    dU = dU.reshape(m + 2, m + 2, Q.shape[2], V.shape[2]).permute(2, 3, 0, 1)
    return _sandwich(ApT, dU, ApT).contiguous()


def reference(op, x, w_or_dy):
    """F.conv2d / its gradients in float64 on the same fp32 inputs (arguments as restate's)"""
    a, b = x.double(), w_or_dy.double()
    if op == "fwd":
        return F.conv2d(a, b, None, 1, 1)
    if op == "dgrad":
        return F.conv_transpose2d(a, b, None, 1, 1)
    if op == "wgrad":
        return torch.nn.grad.conv2d_weight(a, (b.shape[1], a.shape[1], 3, 3), b, 1, 1)
    raise ValueError(op)


def errors(got, ref):
    """(max|d| / max|ref|, ||d|| / ||ref||) in float64"""
    d = (got.double() - ref.double()).flatten()
    r = ref.double().flatten()
    return (d.abs().max() / r.abs().max().clamp_min(1e-300)).item(), (d.norm() / r.norm().clamp_min(1e-300)).item()


def ktot(op, tiling, N, Cin, Cout, H, W):
    """the reduction length of the op's batched GEMM"""
    return Cin if op == "fwd" else (Cout if op == "dgrad" else tiles(tiling, N, H, W))


def floor(k):
    return math.sqrt(k) * EPS / 8


def bars(rest_errs, k):
    """(max-norm bar, rel. L2 bar) of a fp32-grade case from its restatement's two errors and its reduction length"""
    return tuple(R_WINO * max(e, floor(k)) for e in rest_errs)


def inputs(op, N, Cin, Cout, H, W, seed=1):
    """the fp32 operands of a case: x = randn, w = randn / sqrt(9 Cin), dy = randn (one generator per tensor: a shape's x is the same for every op)"""
    def r(shape, s):
        return torch.randn(shape, generator=torch.Generator().manual_seed(s))
    if op == "fwd":
        return r((N, Cin, H, W), seed), r((Cout, Cin, 3, 3), seed + 1) / math.sqrt(9 * Cin)
    if op == "dgrad":
        return r((N, Cout, H, W), seed + 2), r((Cout, Cin, 3, 3), seed + 1) / math.sqrt(9 * Cin)
    return r((N, Cin, H, W), seed), r((N, Cout, H, W), seed + 2)


_cache = {}


def yardstick(op, tiling, N, Cin, Cout, H, W, seed=1):
    """(a, b, ref64, rest32) of a case, computed once per process and never modified by a caller: the operands of `inputs`, the float64
    reference and the fp32 restatement of the plain linear op (epilogue terms are applied by the caller to both)"""
    key = (op, tiling, N, Cin, Cout, H, W, seed)
    if key not in _cache:
        rkey = (op, 0, N, Cin, Cout, H, W, seed)
        if rkey not in _cache:
            a, b = inputs(op, N, Cin, Cout, H, W, seed)
            _cache[rkey] = (a, b, reference(op, a, b))
        a, b, ref = _cache[rkey]
        _cache[key] = (a, b, ref, restate(op, tiling, a, b, torch.float32))
    return _cache[key]
