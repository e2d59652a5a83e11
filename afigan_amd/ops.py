"""Tensor-level wrappers over the per-op C-ABI entry points (used by the modules, the stage-1 engine and the tests).

All tensors are logically NCHW (what detectron2 hands around) but must be *pixel-major* in memory:
``stride(1) == 1`` (torch.channels_last, or any crop / channel slice of such a tensor).  ``pixel_major`` converts an
NCHW-contiguous tensor with the library's own transpose kernel.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import View, call

_NULL_VIEW = View(None, 0, 0, 0)


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_cuda(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.AfiError("the AFI-GAN hot path runs on the GPU only (got a CPU tensor); there is no CPU fallback")
        if t.dtype != torch.float32:
            raise _lib.AfiError(f"fp32 only on this path, got {t.dtype}")


def is_pixel_major(t: torch.Tensor) -> bool:
    return t.dim() == 4 and (t.stride(1) == 1 or t.size(1) == 1) and all(s % 4 == 0 for s in (t.stride(0), t.stride(2), t.stride(3))) \
        and t.data_ptr() % 16 == 0


_POISON = os.environ.get("AFI_POISON_WS", "0") != "0"     # debugging aid: workspaces start as NaN, so a read of memory the library did not
                                                            # write first shows up in the results instead of depending on what the allocator recycled


def new_workspace(floats: int, device) -> torch.Tensor:
    """Uninitialised fp32 scratch for a library call (NaN-filled under AFI_POISON_WS=1)."""
    if _POISON:
        return torch.full((int(floats),), float("nan"), device=device, dtype=torch.float32)
    return torch.empty(int(floats), device=device, dtype=torch.float32)


def new_pixel_major(N, C_, H, W, device, zero=False, dtype=torch.float32) -> torch.Tensor:
    """Fresh [N,C,H,W] tensor whose memory is [N][H][W][C]."""
    if _POISON and not zero:
        return torch.full((N, H, W, C_), float("nan"), device=device, dtype=dtype).permute(0, 3, 1, 2)
    f = torch.zeros if zero else torch.empty
    return f((N, H, W, C_), device=device, dtype=dtype).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ storage dtype at the module boundary
# The interpolator and the AFI FPN / PAFPN accept bf16 / fp16 activations (torch.autocast): they are widened to fp32 on the way in, every
# kernel computes in fp32 under the context's compute dtype, and the module's outputs (and its inputs' gradients) are rounded back ONCE, by
# the epilogue that stores them.  Only the helpers below let a 2-byte tensor in; _check_cuda keeps refusing it everywhere else.
STORE_DTYPES = {torch.float32: _lib.DEFINES["AFI_STORE_F32"], torch.bfloat16: _lib.DEFINES["AFI_STORE_BF16"], torch.float16: _lib.DEFINES["AFI_STORE_F16"]}


def boundary_dtype(*ts) -> torch.dtype:
    """The storage dtype of the tensors a module receives: fp32, bf16 or fp16, on the GPU, one dtype for all of them (AfiError otherwise)."""
    dts = {t.dtype for t in ts if t is not None}
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.AfiError("the AFI-GAN hot path runs on the GPU only (got a CPU tensor); there is no CPU fallback")
    if len(dts) > 1:
        raise _lib.AfiError(f"the inputs of one module must share one dtype, got {sorted(str(d) for d in dts)}")
    dt = dts.pop() if dts else torch.float32
    if dt not in STORE_DTYPES:
        raise _lib.AfiError(f"fp32, bf16 or fp16 activations only at this boundary, got {dt}")
    return dt


def _autocast_on() -> bool:
    try:
        return torch.is_autocast_enabled("cuda")
    except TypeError:                                       # (torch < 2.4: the CUDA flag takes no argument)
        return torch.is_autocast_enabled()


def generator_input_dtype(t) -> torch.dtype:
    """boundary_dtype of the interpolator's own input (Generator.forward).  A 2-byte map reaches a stand-alone interpolator from the reference's
    FPN code run under torch.autocast("cuda"), and is taken there; outside an autocast region the stand-alone module keeps the fp32-only
    contract tests/test_gpu_modules.py::test_error_paths pins (an fp16 input raises).  FPN_AFIGAN / PAFPN_AFIGAN take 2-byte bottom-up
    features with or without autocast (boundary_dtype alone): they never hand the interpolator anything but their fp32 top-down chain."""
    dt = boundary_dtype(t)
    if dt != torch.float32 and not _autocast_on():
        raise _lib.AfiError(f"Generator: fp32 only outside torch.autocast, got {dt} (a 2-byte map is taken under torch.autocast(\"cuda\"))")
    return dt


def ingest(t: torch.Tensor):
    """(fp32 pixel-major tensor, storage dtype of t): fp32 goes through pixel_major as always; a bf16 / fp16 tensor (NCHW, channels_last
    or any strided view) is widened into a fresh dense fp32 [N][H][W][C] by afi_cast_to_f32_nhwc (exact)."""
    dt = boundary_dtype(t)
    if dt == torch.float32:
        return pixel_major(t), dt
    N, C_, H, W = t.shape
    out = new_pixel_major(N, C_, H, W, t.device)
    sN, sC, sH, sW = t.stride()
    call("afi_cast_to_f32_nhwc", C.c_void_p(t.data_ptr()), STORE_DTYPES[dt], N, C_, H, W, sN, sC, sH, sW, C.c_void_p(out.data_ptr()), stream_ptr())
    return out, dt


def narrow(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """A pixel-major fp32 tensor stored as `dtype`: itself for fp32, else a dense channels_last bf16 / fp16 copy rounded to nearest even
    (afi_cast_from_f32_nhwc; for gradients that no GEMM epilogue writes)."""
    _check_cuda(t)
    if dtype == torch.float32:
        return t
    if dtype not in (torch.bfloat16, torch.float16):
        raise _lib.AfiError(f"narrow: fp32, bf16 or fp16 only, got {dtype}")
    N, C_, H, W = t.shape
    out = new_pixel_major(N, C_, H, W, t.device, dtype=dtype)
    call("afi_cast_from_f32_nhwc", view_of(t), N, H, W, C_, C.c_void_p(out.data_ptr()), STORE_DTYPES[dtype], stream_ptr())
    return out


def pixel_major(t: torch.Tensor) -> torch.Tensor:
    """Return `t` itself when it is already pixel-major, else an NHWC copy made by afi_nchw_to_nhwc."""
    _check_cuda(t)
    if is_pixel_major(t):
        return t
    src = t if t.is_contiguous() else t.contiguous()
    N, C_, H, W = src.shape
    out = new_pixel_major(N, C_, H, W, t.device)
    call("afi_nchw_to_nhwc", C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), N, C_, H * W, stream_ptr())
    return out


def to_nchw_contiguous(t: torch.Tensor) -> torch.Tensor:
    """Dense pixel-major tensor -> NCHW-contiguous copy (afi_nhwc_to_nchw)."""
    _check_cuda(t)
    N, C_, H, W = t.shape
    assert t.permute(0, 2, 3, 1).is_contiguous()
    out = torch.empty((N, C_, H, W), device=t.device, dtype=torch.float32)
    call("afi_nhwc_to_nchw", C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()), N, C_, H * W, stream_ptr())
    return out


def view_of(t: torch.Tensor, c0: int = 0) -> View:
    """afi_view_t of a pixel-major tensor (optionally starting at channel c0)."""
    if not is_pixel_major(t):
        raise _lib.AfiError(f"tensor is not pixel-major: shape {tuple(t.shape)} strides {t.stride()}")
    return View(t.data_ptr() + t.element_size() * c0, t.stride(0), t.stride(2), t.stride(3))


def is_dense_pm(t: torch.Tensor) -> bool:
    return t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous()


def to_ohwi(w: torch.Tensor) -> torch.Tensor:
    """[O,I,kh,kw] weight with its memory made [O][kh][kw][I] (what the conv kernels read)."""
    return w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def ohwi(w: torch.Tensor) -> torch.Tensor:
    """[O,I,kh,kw] weight whose memory is [O][kh][kw][I]; copies only if it is not already."""
    if w.permute(0, 2, 3, 1).is_contiguous():
        return w
    return keep_alive(to_ohwi(w))


def new_ohwi(O, I, kh, kw, device, zero=True) -> torch.Tensor:
    f = torch.zeros if zero else torch.empty
    return f((O, kh, kw, I), device=device, dtype=torch.float32).permute(0, 3, 1, 2)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _dense(t):
    """sizes/strides describe a permutation of a contiguous block (what zeros_like can reproduce exactly)"""
    expect = 1
    for size, stride in sorted(((sz, st) for sz, st in zip(t.size(), t.stride()) if sz != 1), key=lambda p: p[1]):
        if stride != expect:
            return False
        expect *= size
    return True


@contextlib.contextmanager
def weight_transform_cache(device, floats=32 * 1024 * 1024):
    """Register a buffer for transformed / packed conv weights (afi_ctx_set_wino_weight_cache) with the active context for the duration
    of a block in which weight VALUES do not change -- e.g. one backbone forward, where the interpolator runs 3 (FPN) to 28 (BiFPN) times
    on one set of weights.  The cache is keyed by weight ADDRESS, so every temporary weight copy made inside the block (``ohwi`` of a
    parameter that is not stored in the kernels' layout, ``.contiguous()`` of a bias) is kept alive until the block exits: a freed
    temporary's address could otherwise be handed to another same-shaped weight and hit the first one's transform.  Not re-entrant."""
    cx = _lib.current_ctx()
    buf = cx.bufs.get("wcache")
    if buf is None or buf.numel() < floats:
        buf = cx.bufs["wcache"] = new_workspace(floats, device)
    if cx.keep is not None:
        raise _lib.AfiError("weight_transform_cache is not re-entrant")
    cx.keep = []
    call("afi_ctx_set_wino_weight_cache", cx.handle, _p(buf), floats)
    try:
        yield
    finally:
        call("afi_ctx_set_wino_weight_cache", cx.handle, C.c_void_p(None), 0)
        cx.keep = None


def keep_alive(t: torch.Tensor) -> torch.Tensor:
    """Hold a temporary until the open weight_transform_cache block (if any) exits; returns it."""
    cx = _lib.current_ctx()
    if cx.keep is not None:
        cx.keep.append(t)
    return t


def zeros_like_many(tensors, need):
    """``[torch.zeros_like(t) if n else None ...]`` out of ONE zero-filled allocation (one fill kernel instead of one per
    tensor: 23 launches per interpolator backward otherwise).  Each result keeps its tensor's sizes and strides (the
    [O][kh][kw][I] weight layout) and starts 16-byte aligned."""
    offs, total = [], 0
    for t, n in zip(tensors, need):
        if n:
            assert t.dtype == torch.float32 and _dense(t), (t.dtype, t.size(), t.stride())
            offs.append(total)
            total += (t.numel() + 3) & ~3
        else:
            offs.append(None)
    if total == 0:
        return [None] * len(offs)
    ref = next(t for t, n in zip(tensors, need) if n)
    flat = torch.zeros(total, device=ref.device, dtype=torch.float32)
    return [flat.as_strided(t.size(), t.stride(), o) if o is not None else None for t, o in zip(tensors, offs)]


def gemm_nt(A, B, dtype, out=None):
    """afi_gemm_nt for tests and micro-benchmarks: C[g] = A[g] @ B[g]^T over the planes of dense [planes, rows, K] / [planes, N, K] tensors,
    in the arithmetic `dtype` ("fp32", "f16x3", "bf16x6", "bf16x3", "bf16"); allocates the split-operand scratch the emulated settings need."""
    _check_cuda(A, B)
    planes, rows, K = A.shape
    N = B.shape[1]
    lib = _lib.load()
    dt = _lib.DTYPES[dtype]
    nb = lib.afi_gemm_nt_scratch_bytes(planes, N, K, dt)
    scratch = torch.empty(max(int(nb), 16), device=A.device, dtype=torch.uint8)
    if out is None:
        out = torch.empty((planes, rows, N), device=A.device, dtype=torch.float32)
    _lib.check(lib.afi_gemm_nt(_p(A), _p(B), _p(out), planes, rows, N, K, dt, _p(scratch), nb, stream_ptr()), "afi_gemm_nt")
    return out


def gemm_tn(Q, V, dtype, out=None):
    """afi_gemm_tn for tests and micro-benchmarks: dU[g] += Q[g]^T @ V[g] over the planes of dense [planes, rows, M] / [planes, rows, N]
    tensors in the arithmetic `dtype`; `out` ([planes, M, N], zero-filled when omitted) is accumulated into, as the weight gradient is."""
    _check_cuda(Q, V)
    planes, rows, M = Q.shape
    N = V.shape[2]
    if out is None:
        out = torch.zeros((planes, M, N), device=Q.device, dtype=torch.float32)
    lib, dt = _lib.load(), _lib.DTYPES[dtype]
    nb = lib.afi_gemm_tn_scratch_bytes(planes, dt)
    scratch = torch.empty(max(int(nb), 16), device=Q.device, dtype=torch.uint8)
    _lib.check(lib.afi_gemm_tn(_p(Q), _p(V), _p(out), planes, rows, M, N, dt, _p(scratch), nb, stream_ptr()), "afi_gemm_tn")
    return out


# ------------------------------------------------------------------------------------------------ convs
OP_SCRATCH_FLOATS = 100 * 1024 * 1024          # 400 MB: 4 slabs of the largest map that is split (1536 tiles of 128x128)


def _ensure_op_scratch(device):
    """Split-K scratch for the per-op conv calls (include/afigan_hip.h: afi_ctx_set_op_scratch): one buffer per context, registered
    once; all per-op calls of a context are issued on one stream, one after the other."""
    cx = _lib.current_ctx()
    buf = cx.bufs.get("op_scratch")
    if buf is None:
        buf = cx.bufs["op_scratch"] = new_workspace(OP_SCRATCH_FLOATS, device)
        call("afi_ctx_set_op_scratch", cx.handle, C.c_void_p(buf.data_ptr()), buf.numel())
    return buf


def conv3x3_fwd(x, w, bias=None, lrelu=False, out=None, alpha=1.0, beta=0.0, out_dtype=torch.float32):
    """out_dtype bf16 / fp16: a fresh 2-byte output rounded by the epilogue (afi_conv3x3_fwd_out16; write-only: beta must be 0)."""
    _check_cuda(x, w, bias, out)
    _ensure_op_scratch(x.device)
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    w = ohwi(w)
    if out_dtype != torch.float32:
        if out is not None:
            raise _lib.AfiError("conv3x3_fwd: a 2-byte output is always a fresh tensor")
        out = new_pixel_major(N, Cout, H, W, x.device, dtype=out_dtype)
        call("afi_conv3x3_fwd_out16", view_of(x), N, H, W, Cin, _p(w), _p(bias), Cout, view_of(out), STORE_DTYPES[out_dtype], float(alpha),
             float(beta), int(lrelu), stream_ptr())
        return out
    if out is None:
        out = new_pixel_major(N, Cout, H, W, x.device)
    call("afi_conv3x3_fwd", view_of(x), N, H, W, Cin, _p(w), _p(bias), Cout, view_of(out), float(alpha), float(beta), int(lrelu),
         stream_ptr())
    return out


Z_ACTS = {"lrelu": 1, "relu": 2}           # the activation whose derivative a data gradient's z mask applies (the numbering of lrelu= / act=)


def _z_act(where, z, z_act):
    if z_act not in Z_ACTS:
        raise _lib.AfiError(f"{where}: z_act must be one of {sorted(Z_ACTS)}, got {z_act!r}")
    if z is None:
        raise _lib.AfiError(f"{where}: z_act={z_act!r} needs z=, the activation the mask is read from")
    return Z_ACTS[z_act]


def conv3x3_dgrad(dy, w, dx=None, alpha=1.0, beta=0.0, z=None, *, z_act=None):
    """dx = (alpha*conv3x3^T(dy, w) + beta*dx) * act'(z).  Without z_act: the LeakyReLU(0.2) mask of afi_conv3x3_dgrad; z_act "lrelu" /
    "relu": afi_conv3x3_dgrad_act."""
    _check_cuda(dy, w, dx, z)
    _ensure_op_scratch(dy.device)
    N, Cout, H, W = dy.shape
    Cin = w.shape[1]
    w = ohwi(w)
    if dx is None:
        dx = new_pixel_major(N, Cin, H, W, dy.device)
    if z_act is not None:
        call("afi_conv3x3_dgrad_act", view_of(dy), N, H, W, Cout, _p(w), Cin, view_of(dx), float(alpha), float(beta), view_of(z),
             _z_act("conv3x3_dgrad", z, z_act), stream_ptr())
        return dx
    call("afi_conv3x3_dgrad", view_of(dy), N, H, W, Cout, _p(w), Cin, view_of(dx), float(alpha), float(beta),
         view_of(z) if z is not None else _NULL_VIEW, stream_ptr())
    return dx


def conv3x3_wgrad(dy, x, dw=None, alpha=1.0):
    _check_cuda(dy, x, dw)
    N, Cout, H, W = dy.shape
    Cin = x.shape[1]
    if dw is None:
        dw = new_ohwi(Cout, Cin, 3, 3, dy.device)
    assert dw.permute(0, 2, 3, 1).is_contiguous()
    call("afi_conv3x3_wgrad", view_of(dy), view_of(x), N, H, W, Cout, Cin, _p(dw), float(alpha), stream_ptr())
    return dw


def conv3x3_wino_fwd(x, w, bias=None, out_dtype=torch.float32):
    """3x3 conv in Winograd F(2x2,3x3) form (large maps, many channels): out = conv(x, w) + bias, stored as out_dtype (fp32, bf16 or fp16:
    the output transform rounds)."""
    _check_cuda(x, w, bias)
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    w = ohwi(w)
    n = _lib.load().afi_conv3x3_wino_ws_floats(N, H, W, Cin, Cout)
    ws = new_workspace(n, x.device)
    out = new_pixel_major(N, Cout, H, W, x.device, dtype=out_dtype)
    if out_dtype != torch.float32:
        call("afi_conv3x3_wino_fwd_out16", view_of(x), N, H, W, Cin, _p(w), _p(bias), Cout, view_of(out), STORE_DTYPES[out_dtype], _p(ws), n,
             stream_ptr())
        return out
    call("afi_conv3x3_wino_fwd", view_of(x), N, H, W, Cin, _p(w), _p(bias), Cout, view_of(out), _p(ws), n, stream_ptr())
    return out


def conv3x3_wino_infer(x, w, bias=None, act=0):
    """act(conv3x3(x, w) + bias) for inference (no backward): Winograd, F(4x4) tiles on maps of >= 8192 pixels.  act: 0 / 1 LeakyReLU / 2 ReLU."""
    _check_cuda(x, w, bias)
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    w = ohwi(w)
    n = _lib.load().afi_conv3x3_wino_ws_floats(N, H, W, Cin, Cout)
    ws = new_workspace(n, x.device)
    out = new_pixel_major(N, Cout, H, W, x.device)
    call("afi_conv3x3_wino_infer", view_of(x), N, H, W, Cin, _p(w), _p(bias), Cout, view_of(out), int(act), _p(ws), n, stream_ptr())
    return out


def conv3x3_wino_dgrad(dy, w, z=None, *, z_act=None, dx=None):
    """Data gradient of the 3x3 conv in Winograd form: dx = conv^T(dy) [* lrelu'(z)]; z_act "lrelu" / "relu": afi_conv3x3_wino_dgrad_act.
    dx=: the (pixel-major, possibly channel-sliced) tensor to write instead of a fresh one."""
    _check_cuda(dy, w, z, dx)
    N, Cout, H, W = dy.shape
    Cin = w.shape[1]
    w = ohwi(w)
    n = _lib.load().afi_conv3x3_wino_ws_floats(N, H, W, Cin, Cout)
    ws = new_workspace(n, dy.device)
    if dx is None:
        dx = new_pixel_major(N, Cin, H, W, dy.device)
    elif tuple(dx.shape) != (N, Cin, H, W):
        raise _lib.AfiError(f"conv3x3_wino_dgrad: dx {tuple(dx.shape)} is not the conv's input shape {(N, Cin, H, W)}")
    if z_act is not None:
        call("afi_conv3x3_wino_dgrad_act", view_of(dy), N, H, W, Cout, _p(w), Cin, view_of(dx), view_of(z), _z_act("conv3x3_wino_dgrad", z, z_act),
             _p(ws), n, stream_ptr())
        return dx
    call("afi_conv3x3_wino_dgrad", view_of(dy), N, H, W, Cout, _p(w), Cin, view_of(dx), view_of(z) if z is not None else _NULL_VIEW,
         _p(ws), n, stream_ptr())
    return dx


def conv3x3_wino_wgrad(dy, x, dw=None, alpha=1.0):
    """Weight gradient of the 3x3 conv in Winograd F(3x3,2x2) form; accumulates into dw ([Cout,Cin,3,3] with OHWI memory)."""
    _check_cuda(dy, x, dw)
    N, Cout, H, W = dy.shape
    Cin = x.shape[1]
    if dw is None:
        dw = new_ohwi(Cout, Cin, 3, 3, dy.device)
    assert dw.permute(0, 2, 3, 1).is_contiguous()
    n = _lib.load().afi_conv3x3_wino_ws_floats(N, H, W, Cin, Cout)
    ws = new_workspace(n, dy.device)
    call("afi_conv3x3_wino_wgrad", view_of(dy), view_of(x), N, H, W, Cout, Cin, _p(dw), float(alpha), _p(ws), n, stream_ptr())
    return dw


def conv3x3s2_fwd(x, w, bias=None, act=0, add=None, add_scale=1.0, post_scale=1.0, keep_act=False):
    """Conv2d(k3, s2, p1) with the fused PAFPN merge:  a = act(conv(x, w) + bias);  out = post_scale*a + add_scale*add.
    act: 0 none, 1 LeakyReLU(0.2), 2 ReLU.  Returns out, or (out, a) with keep_act (a is what the ReLU backward needs)."""
    _check_cuda(x, w, bias, add)
    _ensure_op_scratch(x.device)
    N, Cin, Hi, Wi = x.shape
    Cout = w.shape[0]
    w = ohwi(w)
    Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
    if add is not None and tuple(add.shape) != (N, Cout, Ho, Wo):
        raise _lib.AfiError(f"conv3x3s2_fwd: residual shape {tuple(add.shape)} != {(N, Cout, Ho, Wo)}")
    out = new_pixel_major(N, Cout, Ho, Wo, x.device)
    a = new_pixel_major(N, Cout, Ho, Wo, x.device) if keep_act else None
    call("afi_conv3x3s2_fwd", view_of(x), N, Hi, Wi, Cin, _p(w), _p(bias), Cout, view_of(out), int(act),
         view_of(a) if a is not None else _NULL_VIEW, float(post_scale), view_of(add) if add is not None else _NULL_VIEW,
         float(add_scale), stream_ptr())
    return (out, a) if keep_act else out


def conv3x3s2_dgrad(dy, w, in_hw, dx=None, alpha=1.0, beta=0.0):
    """dx [N,Cin,Hi,Wi] = alpha * (data gradient of Conv2d(k3,s2,p1)) + beta*dx;  in_hw = (Hi, Wi) of the conv's input."""
    _check_cuda(dy, w, dx)
    _ensure_op_scratch(dy.device)
    N, Cout, Ho, Wo = dy.shape
    Hi, Wi = in_hw
    if ((Hi + 1) // 2, (Wi + 1) // 2) != (Ho, Wo):
        raise _lib.AfiError(f"conv3x3s2_dgrad: dy {Ho}x{Wo} is not the stride-2 output of {Hi}x{Wi}")
    Cin = w.shape[1]
    w = ohwi(w)
    if dx is None:
        dx = new_pixel_major(N, Cin, Hi, Wi, dy.device)
    call("afi_conv3x3s2_dgrad", view_of(dy), N, Hi, Wi, Cout, _p(w), Cin, view_of(dx), float(alpha), float(beta), stream_ptr())
    return dx


def conv3x3s2_wgrad(dy, x, dw=None, alpha=1.0):
    _check_cuda(dy, x, dw)
    N, Cout, Ho, Wo = dy.shape
    _, Cin, Hi, Wi = x.shape
    if ((Hi + 1) // 2, (Wi + 1) // 2) != (Ho, Wo):
        raise _lib.AfiError(f"conv3x3s2_wgrad: dy {Ho}x{Wo} is not the stride-2 output of {Hi}x{Wi}")
    if dw is None:
        dw = new_ohwi(Cout, Cin, 3, 3, dy.device)
    assert dw.permute(0, 2, 3, 1).is_contiguous()
    call("afi_conv3x3s2_wgrad", view_of(dy), view_of(x), N, Hi, Wi, Cout, Cin, _p(dw), float(alpha), stream_ptr())
    return dw


def relu_bwd(g, act, scale=1.0):
    """scale * g * (act > 0) for dense pixel-major g / act of the same shape."""
    _check_cuda(g, act)
    assert is_dense_pm(g) and is_dense_pm(act) and g.shape == act.shape
    out = new_pixel_major(*g.shape, g.device)
    call("afi_relu_bwd", _p(g), _p(act), _p(out), g.numel(), float(scale), stream_ptr())
    return out


def conv1x1_fwd(x, w, bias=None, add=None, add_scale=1.0, alpha=1.0, out=None, act=0):
    """out = act(alpha*conv1x1(x, w) + bias + add_scale*add);  w: [Cout, Cin] or [Cout, Cin, 1, 1];  act: 0 none, 1 LeakyReLU(0.2), 2 ReLU.
    ``x`` may be a strided view of a pixel-major tensor (a crop, or every second pixel: a stride-2 1x1 conv reads it in place)."""
    _check_cuda(x, w, bias, add, out)
    _ensure_op_scratch(x.device)
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    w2 = w.reshape(Cout, Cin).contiguous()
    if out is None:
        out = new_pixel_major(N, Cout, H, W, x.device)
    call("afi_conv1x1_fwd", view_of(x), N, H, W, Cin, _p(w2), _p(bias), Cout, view_of(out), float(alpha), 0.0,
         view_of(add) if add is not None else _NULL_VIEW, float(add_scale), int(act), stream_ptr())
    return out


# ---- the 1x1 conv of FROZEN weights on the bf16 matrix cores (csrc/frozen1x1.hip): the weight is turned into a pre-split image once
# (frozen.conv1x1_image keeps it per module), large maps then run afi_conv1x1_frozen_fwd instead of the fp32-MFMA pixel GEMM.
FROZEN1X1_MIN_PIXELS = 8192          # maps below it stay on conv1x1_fwd (the per-shape table that decided it) ...
FROZEN1X1_MIN_PIXELS_EXPANDING = 2048   # ... but for the convs with Cout >= 2 Cin (conv3, shortcuts): enough column tiles to fill the chip from here on
frozen1x1_route = True               # False: every caller takes conv1x1_fwd (A/B runs, and the route test's reference)
frozen1x1_images_built = 0           # image launches so far (an unchanged weight must not add to it)
_F1_PLAN = ("M", "BM", "BN", "KC", "ntile_m", "ntile_n", "grid", "lds_bytes", "x_bytes", "out_bytes", "image_bytes", "x_dense")


def conv1x1_frozen_plan(N, H, W, Cin, Cout, x_strides, out_strides=None, add_strides=None):
    """The host plan of afi_conv1x1_frozen_fwd for x [N, Cin, H, W] with element strides (sN, sH, sW), a dense output unless `out_strides`
    says otherwise and an optional addend: a dict (M, BM, BN, KC, ntile_m, ntile_n, grid, lds_bytes, x_bytes, out_bytes, image_bytes,
    x_dense), or None when the kernel does not take the problem.  Pure host code: no device, no launch."""
    o = out_strides if out_strides is not None else (H * W * Cout, W * Cout, Cout)
    a = add_strides if add_strides is not None else (0, 0, 0)
    plan = (C.c_longlong * len(_F1_PLAN))()
    st = _lib.load().afi_frozen1x1_plan(N, H, W, Cin, Cout, *[int(s) for s in x_strides], *[int(s) for s in o], int(add_strides is not None),
                                        *[int(s) for s in a], plan)
    if st == _lib.DEFINES["AFI_ERR_UNSUPPORTED"]:
        return None
    _lib.check(st, "afi_frozen1x1_plan")
    return dict(zip(_F1_PLAN, plan))


def conv1x1_frozen_routed(x, Cout, add=None):
    """True when a frozen 1x1 conv of `x` to `Cout` channels goes to the bf16x6 kernel: the route is on, the map has at least
    FROZEN1X1_MIN_PIXELS pixels (FROZEN1X1_MIN_PIXELS_EXPANDING when Cout >= 2 Cin) and the host plan takes the views."""
    N, Cin, H, W = x.shape
    least = min(FROZEN1X1_MIN_PIXELS, FROZEN1X1_MIN_PIXELS_EXPANDING) if Cout >= 2 * Cin else FROZEN1X1_MIN_PIXELS
    if not frozen1x1_route or N * H * W < least or x.stride(1) != 1 or (add is not None and not is_dense_pm(add)):
        return False
    return conv1x1_frozen_plan(N, H, W, Cin, Cout, (x.stride(0), x.stride(2), x.stride(3)),
                               add_strides=(add.stride(0), add.stride(2), add.stride(3)) if add is not None else None) is not None


def conv1x1_frozen_image(w):
    """The bf16x6 fragment image of w [Cout, Cin] (or [Cout, Cin, 1, 1]), both multiples of 32: a uint8 tensor afi_conv1x1_frozen_fwd reads."""
    global frozen1x1_images_built
    _check_cuda(w)
    Cout, Cin = w.shape[0], w.shape[1]
    w2 = w.reshape(Cout, Cin).contiguous()
    nbytes = _lib.load().afi_frozen1x1_image_bytes(Cout, Cin)
    if nbytes <= 0:
        raise _lib.AfiError(f"conv1x1_frozen_image: Cout {Cout} and Cin {Cin} must be positive multiples of 32")
    image = torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    call("afi_conv1x1_frozen_image", _p(w2), Cout, Cin, _p(image), nbytes, stream_ptr())
    frozen1x1_images_built += 1
    return image


def conv1x1_frozen_fwd(x, image, bias, Cout, add=None, add_scale=1.0, alpha=1.0, out=None, act=0):
    """out = act(alpha*conv1x1(x, w) + bias + add_scale*add) with w given as its conv1x1_frozen_image; what conv1x1_frozen_plan refuses
    raises AfiError (callers ask conv1x1_frozen_routed first and take conv1x1_fwd otherwise)."""
    _check_cuda(x, bias, add, out)
    N, Cin, H, W = x.shape
    if out is None:
        out = new_pixel_major(N, Cout, H, W, x.device)
    call("afi_conv1x1_frozen_fwd", view_of(x), N, H, W, Cin, _p(image), _p(bias), Cout, view_of(out), float(alpha),
         view_of(add) if add is not None else _NULL_VIEW, float(add_scale), int(act), stream_ptr())
    return out


def conv1x1_dgrad(dy, w, dx=None, alpha=1.0, beta=0.0, out_dtype=torch.float32, *, z=None, z_act="lrelu", add=None, add_scale=1.0):
    """out_dtype bf16 / fp16: a fresh 2-byte dx rounded by the epilogue (afi_conv1x1_dgrad_out16; beta must be 0).
    With z= and / or add= (afi_conv1x1_dgrad_act): dx = (alpha*W^T dy + beta*dx + add_scale*add) * act'(z), z_act "lrelu" or "relu"; dx, add
    and z may be strided views of pixel-major tensors (every second pixel), and beta = 1 may update dx in place."""
    _check_cuda(dy, w, dx, z, add)
    _ensure_op_scratch(dy.device)
    N, Cout, H, W = dy.shape
    Cin = w.shape[1]
    w2 = w.reshape(Cout, Cin).contiguous()
    if z is not None or add is not None:
        if out_dtype != torch.float32:
            raise _lib.AfiError("conv1x1_dgrad: z= / add= go with an fp32 dx")
        if dx is None:
            dx = new_pixel_major(N, Cin, H, W, dy.device)
        for name, t in (("dx", dx), ("z", z), ("add", add)):
            if t is not None and tuple(t.shape) != (N, Cin, H, W):
                raise _lib.AfiError(f"conv1x1_dgrad: {name} {tuple(t.shape)} is not the conv's input shape {(N, Cin, H, W)}")
        call("afi_conv1x1_dgrad_act", view_of(dy), N, H, W, Cout, _p(w2), Cin, view_of(dx), float(alpha), float(beta),
             view_of(add) if add is not None else _NULL_VIEW, float(add_scale), view_of(z) if z is not None else _NULL_VIEW,
             _z_act("conv1x1_dgrad", z, z_act) if z is not None else 0, stream_ptr())
        return dx
    if out_dtype != torch.float32:
        if dx is not None:
            raise _lib.AfiError("conv1x1_dgrad: a 2-byte output is always a fresh tensor")
        dx = new_pixel_major(N, Cin, H, W, dy.device, dtype=out_dtype)
        call("afi_conv1x1_dgrad_out16", view_of(dy), N, H, W, Cout, _p(w2), Cin, view_of(dx), STORE_DTYPES[out_dtype], float(alpha), float(beta),
             stream_ptr())
        return dx
    if dx is None:
        dx = new_pixel_major(N, Cin, H, W, dy.device)
    call("afi_conv1x1_dgrad", view_of(dy), N, H, W, Cout, _p(w2), Cin, view_of(dx), float(alpha), float(beta), stream_ptr())
    return dx


def conv1x1_wgrad(dy, x, alpha=1.0):
    _check_cuda(dy, x)
    N, Cout, H, W = dy.shape
    Cin = x.shape[1]
    dw = torch.zeros((Cout, Cin), device=dy.device, dtype=torch.float32)
    call("afi_conv1x1_wgrad", view_of(dy), view_of(x), N, H, W, Cout, Cin, _p(dw), float(alpha), stream_ptr())
    return dw


def frozen_wgrad_unfold(descs):
    """grad[o][i][kh][kw] += s[o] * dw[o][kh][kw][i] for every (dw, grad, s) of `descs` in one launch (afi_frozen_wgrad_unfold): dw the
    gradient of a weight folded with its FrozenBN, in the kernels' memory ([O, I, k, k] with OHWI memory, or [O, I] for k = 1), grad a
    contiguous [O, I, k, k] tensor, s the fold's [O] scale."""
    if not descs:
        return
    table = (_lib.UnfoldDesc * len(descs))()
    max_oi = 0
    for d, (dw, grad, s_) in zip(table, descs):
        _check_cuda(dw, grad, s_)
        O, I = grad.shape[:2]
        k = grad.shape[2] if grad.dim() == 4 else 1
        ok = grad.is_contiguous() and k in (1, 3) and dw.numel() == grad.numel() == O * I * k * k and s_.numel() == O and s_.is_contiguous() \
            and dw.shape[:2] == grad.shape[:2] and (dw.permute(0, 2, 3, 1).is_contiguous() if dw.dim() == 4 else dw.is_contiguous())
        if not ok:
            raise _lib.AfiError(f"frozen_wgrad_unfold: dw {tuple(dw.shape)} / grad {tuple(grad.shape)} / s {tuple(s_.shape)}: grad must be a "
                                "contiguous [O, I, k, k] (k 1 or 3), dw the same shape in OHWI memory, s [O]")
        d.dw, d.grad, d.s, d.O, d.I, d.k = dw.data_ptr(), grad.data_ptr(), s_.data_ptr(), O, I, k
        max_oi = max(max_oi, O * ((I + 31) // 32))
    dev = descs[0][0].device
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    call("afi_frozen_wgrad_unfold", _p(table_dev), len(descs), max_oi, stream_ptr())


def detector_sgd_units(n, O=0, I=0, k=0, fold=False):
    """The number of work units afi_detector_sgd_step cuts a tensor into (afi_detector_sgd_units)."""
    return int(_lib.load().afi_detector_sgd_units(int(n), int(O), int(I), int(k), int(bool(fold))))


def detector_sgd_step(table, device, momentum, gscale=1.0, flat=False, units=None):
    """One afi_detector_sgd_step launch over `table`, a ctypes array of _lib.DetSgdDesc (device pointers; see include/afigan_hip.h): SGD with
    momentum and per-tensor lr / weight decay, and the FrozenBN refold of the entries with a ``fold_out``.  `flat`: the flat grid over all work
    units, else the (<= 512, ntensors) grid.  `units`: the entries' unit counts if the caller keeps them (detector_sgd_units otherwise).
    The table (and the flat grid's unit prefix behind it) goes to the device in one copy."""
    nt = len(table)
    if nt == 0:
        return
    if units is None:
        units = [detector_sgd_units(d.n, d.O, d.I, d.k, bool(d.fold_out)) if d.n > 0 else 0 for d in table]
    raw = bytes(table)
    if flat:
        raw += b"\0" * (-len(raw) % 16)
        prefix = len(raw)
        raw += np.concatenate([[0], np.cumsum(units)]).astype(np.int32).tobytes()
    buf = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
    unit_off = C.c_void_p(buf.data_ptr() + prefix) if flat else C.c_void_p(None)
    call("afi_detector_sgd_step", table, _p(buf), nt, max(units), unit_off, sum(units), float(momentum), float(gscale), stream_ptr())


def bias_grad(dy):
    """Column sums of a dense pixel-major gradient: d/d bias of a conv."""
    assert is_dense_pm(dy)
    N, C_, H, W = dy.shape
    db = torch.zeros(C_, device=dy.device, dtype=torch.float32)
    colsum_accum(dy.permute(0, 2, 3, 1).reshape(-1, C_), db)
    return db


def convT_pack(w_iohw):
    Cin, Cout = w_iohw.shape[:2]
    w_iohw = w_iohw.contiguous()
    wp = torch.empty((4 * Cout, 3, 3, Cin), device=w_iohw.device, dtype=torch.float32)
    call("afi_convT6s2_pack_weight", _p(w_iohw), _p(wp), Cin, Cout, stream_ptr())
    return wp


def convT_fwd(x, wp, bias, Cout, lrelu=False):
    _ensure_op_scratch(x.device)
    N, Cin, H, W = x.shape
    out = new_pixel_major(N, Cout, 2 * H, 2 * W, x.device)
    call("afi_convT6s2_fwd", view_of(x), N, H, W, Cin, _p(wp), _p(bias), Cout, view_of(out), int(lrelu), stream_ptr())
    return out


def convT_dgrad(dy, wp, Cin, z=None):
    _ensure_op_scratch(dy.device)
    N, Cout, H2, W2 = dy.shape
    H, W = H2 // 2, W2 // 2
    dx = new_pixel_major(N, Cin, H, W, dy.device)
    call("afi_convT6s2_dgrad", view_of(dy), N, H, W, Cout, _p(wp), Cin, view_of(dx), view_of(z) if z is not None else _NULL_VIEW,
         stream_ptr())
    return dx


def convT_wgrad(dy, x):
    """Returns the gradient in torch's [Cin][Cout][6][6] layout."""
    N, Cout, H2, W2 = dy.shape
    _, Cin, H, W = x.shape
    dwp = torch.zeros((4 * Cout, 3, 3, Cin), device=dy.device, dtype=torch.float32)
    call("afi_convT6s2_wgrad", view_of(dy), view_of(x), N, H, W, Cout, Cin, _p(dwp), 1.0, stream_ptr())
    dw = torch.zeros((Cin, Cout, 6, 6), device=dy.device, dtype=torch.float32)
    call("afi_convT6s2_unpack_wgrad", _p(dwp), _p(dw), Cin, Cout, stream_ptr())
    return dw


# ------------------------------------------------------------------------------------------------ BiFPN inference pieces
def dwconv3x3(x, w9c):
    """Depthwise 3x3 (stride 1, zero pad 1, no bias); w9c: [9, C] tap-major weights (see bifpn_sr.pack_depthwise)."""
    _check_cuda(x, w9c)
    N, C_, H, W = x.shape
    assert tuple(w9c.shape) == (9, C_) and w9c.is_contiguous()
    out = new_pixel_major(N, C_, H, W, x.device)
    call("afi_dwconv3x3_fwd", view_of(x), N, H, W, C_, _p(w9c), _p(out), stream_ptr())
    return out


def maxpool3s2_same(x):
    """MaxPool2d(3, 2, padding_mode="static_same") of bifpn_layers/wrappers.py (zero pad right/bottom)."""
    _check_cuda(x)
    N, C_, H, W = x.shape
    out = new_pixel_major(N, C_, (H - 2) // 2 + 1, (W - 2) // 2 + 1, x.device)
    call("afi_maxpool3s2_same_fwd", view_of(x), N, H, W, C_, _p(out), stream_ptr())
    return out


def fuse_swish(w, a, b, c=None):
    """swish(w[0]*a + w[1]*b (+ w[2]*c)) for dense pixel-major tensors of one shape; w: device tensor with 2 or 3 weights."""
    _check_cuda(w, a, b, c)
    assert is_dense_pm(a) and is_dense_pm(b) and a.shape == b.shape and (c is None or (is_dense_pm(c) and c.shape == a.shape))
    assert w.numel() == (2 if c is None else 3) and w.is_contiguous()
    out = new_pixel_major(*a.shape, a.device)
    call("afi_fuse_swish_fwd", _p(a), _p(b), _p(c), _p(w), _p(out), a.numel(), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ BiFPN node backward (training mode)
def fuse_swish_bwd(w, a, b, c, dout, need=(True, True, True, True)):
    """Backward of fuse_swish: returns (dw, da, db, dc); entries not in `need` (w, a, b, c) come back None."""
    _check_cuda(w, a, b, c, dout)
    assert is_dense_pm(dout) and dout.shape == a.shape
    dev = a.device
    da = new_pixel_major(*a.shape, dev) if need[1] else None
    db = new_pixel_major(*a.shape, dev) if need[2] else None
    dc = new_pixel_major(*a.shape, dev) if (c is not None and need[3]) else None
    dw = torch.empty_like(w) if need[0] else None
    scratch = new_workspace(_lib.load().afi_fuse_swish_bwd_scratch_floats(), dev)
    call("afi_fuse_swish_bwd", _p(a), _p(b), _p(c), _p(w), _p(dout), _p(da), _p(db), _p(dc), _p(dw), a.numel(), _p(scratch), stream_ptr())
    return dw, da, db, dc


def dwconv3x3_wgrad(dy, x):
    """[9, C] tap-major weight gradient of dwconv3x3 from dense pixel-major dy and x."""
    _check_cuda(dy, x)
    assert is_dense_pm(dy) and is_dense_pm(x) and dy.shape == x.shape
    N, C_, H, W = x.shape
    dw = torch.empty((9, C_), device=x.device, dtype=torch.float32)
    scratch = new_workspace(_lib.load().afi_dwconv3x3_wgrad_scratch_floats(C_), x.device)
    call("afi_dwconv3x3_wgrad", _p(dy), _p(x), N, H, W, C_, _p(dw), _p(scratch), stream_ptr())
    return dw


def maxpool3s2_same_idx(x):
    """maxpool3s2_same keeping the argmax taps (uint8, [N, Ho, Wo, C]) for maxpool3s2_same_bwd."""
    _check_cuda(x)
    N, C_, H, W = x.shape
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    out = new_pixel_major(N, C_, Ho, Wo, x.device)
    idx = torch.empty((N, Ho, Wo, C_), device=x.device, dtype=torch.uint8)
    call("afi_maxpool3s2_same_fwd_idx", view_of(x), N, H, W, C_, _p(out), _p(idx), stream_ptr())
    return out, idx


def maxpool3s2_same_bwd(dout, idx, in_hw):
    _check_cuda(dout)
    if not idx.is_cuda or idx.dtype != torch.uint8 or not idx.is_contiguous():
        raise _lib.AfiError("idx must be the contiguous uint8 CUDA tensor maxpool3s2_same_idx returned")
    N, C_ = dout.shape[:2]
    H, W = in_hw
    assert is_dense_pm(dout) and tuple(idx.shape) == (N, (H - 2) // 2 + 1, (W - 2) // 2 + 1, C_) and tuple(dout.shape[2:]) == tuple(idx.shape[1:3])
    dx = new_pixel_major(N, C_, H, W, dout.device)
    call("afi_maxpool3s2_same_bwd", _p(dout), _p(idx), N, H, W, C_, _p(dx), stream_ptr())
    return dx


def bn_stats_ex(x2d, eps, momentum, running_mean=None, running_var=None, num_batches_tracked=None, want_var=False):
    """Train-mode statistics of a dense [P, C] matrix with the norm's own eps / momentum; updates the running buffers in place.
    want_var: also the biased batch variance (for a caller that combines the statistics of several ranks)."""
    P, C_ = x2d.shape
    mean, invstd = torch.empty(C_, device=x2d.device), torch.empty(C_, device=x2d.device)
    var = torch.empty(C_, device=x2d.device) if want_var else None
    call("afi_bn_stats_ex", _p(x2d), P, C_, float(eps), float(momentum), _p(mean), _p(invstd), _p(var), _p(running_mean), _p(running_var),
         _p(num_batches_tracked), _p(reduce_scratch(C_, x2d.device)), stream_ptr())
    return (mean, invstd, var) if want_var else (mean, invstd)


def bn_apply(x2d, mean, invstd, gamma, beta, slope=1.0):
    P, C_ = x2d.shape
    y = torch.empty_like(x2d)
    call("afi_bn_apply_fwd", _p(x2d), _p(y), _p(mean), _p(invstd), _p(gamma), _p(beta), P, C_, float(slope), stream_ptr())
    return y


# ------------------------------------------------------------------------------------------------ dual-scale data path
def _check_u8(t):
    if not t.is_cuda:
        raise _lib.AfiError("the dual-scale data path runs on the GPU only (got a CPU tensor); there is no CPU fallback")
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise _lib.AfiError(f"expected a contiguous uint8 tensor, got {t.dtype}, contiguous={t.is_contiguous()}")


def resize_bilinear_u8(img_hwc, new_h, new_w, hflip=False, chw=True):
    """ResizeTransform.apply_image (Pillow BILINEAR, bit-exact) + the shared HFlipTransform for a uint8 [H,W,C] or [H,W]
    device tensor; returns uint8 [C,new_h,new_w] (chw, the DatasetMapper tensor layout) or [new_h,new_w,C]."""
    _check_u8(img_hwc)
    squeeze = img_hwc.dim() == 2
    H0, W0 = img_hwc.shape[:2]
    Cn = 1 if squeeze else img_hwc.shape[2]
    new_h, new_w = int(new_h), int(new_w)
    lib = _lib.load()
    ws_bytes = lib.afi_resize_bilinear_u8_ws_bytes(H0, W0, Cn, new_h, new_w)
    if ws_bytes < 0:
        raise _lib.AfiError(f"afi_resize_bilinear_u8: unsupported shape {tuple(img_hwc.shape)} -> {(new_h, new_w)}")
    ws = torch.empty(ws_bytes, device=img_hwc.device, dtype=torch.uint8)
    out = torch.empty((Cn, new_h, new_w) if chw else (new_h, new_w, Cn), device=img_hwc.device, dtype=torch.uint8)
    call("afi_resize_bilinear_u8", _p(img_hwc), H0, W0, Cn, _p(out), new_h, new_w, int(bool(hflip)), int(bool(chw)), _p(ws), ws_bytes,
         stream_ptr())
    if squeeze:
        out = out[0] if chw else out[..., 0]
    return out


def dual_scale_u8(img_hwc, size, size_r, hflip=False, hflip_r=False, chw=True):
    """Both images of one DatasetMapper sample in two launches: `image` = resize(img, size) and `image_x0.5` =
    resize(img, size_r), each from the ORIGINAL uint8 [H,W,3] device tensor (dataset_mapper.py:103-105), each with its flip flag."""
    _check_u8(img_hwc)
    if img_hwc.dim() != 3:
        raise _lib.AfiError(f"expected a uint8 HWC image, got shape {tuple(img_hwc.shape)}")
    H0, W0, Cn = img_hwc.shape
    (H1, W1), (H2, W2) = (int(v) for v in size), (int(v) for v in size_r)
    lib = _lib.load()
    ws_bytes = lib.afi_dual_scale_u8_ws_bytes(H0, W0, Cn, H1, W1, H2, W2)
    if ws_bytes < 0:
        raise _lib.AfiError(f"afi_dual_scale_u8: unsupported shape {tuple(img_hwc.shape)} -> {(H1, W1)}, {(H2, W2)}")
    ws = torch.empty(ws_bytes, device=img_hwc.device, dtype=torch.uint8)
    out = torch.empty((Cn, H1, W1) if chw else (H1, W1, Cn), device=img_hwc.device, dtype=torch.uint8)
    out_r = torch.empty((Cn, H2, W2) if chw else (H2, W2, Cn), device=img_hwc.device, dtype=torch.uint8)
    call("afi_dual_scale_u8", _p(img_hwc), H0, W0, Cn, _p(out), H1, W1, int(bool(hflip)), _p(out_r), H2, W2, int(bool(hflip_r)),
         int(bool(chw)), _p(ws), ws_bytes, stream_ptr())
    return out, out_r


def normalize_pad(images_chw, pixel_mean, pixel_std, size_divisibility=0):
    """RCNN_FPN_only.forward's `(x - mean) / std` per image + ImageList.from_tensors (rcnn_only.py:36-39): a list of uint8
    [C,H,W] device tensors -> fp32 [N,C,Hp,Wp], zero-padded bottom/right to the batch maximum rounded up to size_divisibility."""
    assert len(images_chw) > 0
    for t in images_chw:
        _check_u8(t)
    Cn = images_chw[0].shape[0]
    hm = max(t.shape[1] for t in images_chw)
    wm = max(t.shape[2] for t in images_chw)
    if size_divisibility > 0:
        hm = -(-hm // size_divisibility) * size_divisibility
        wm = -(-wm // size_divisibility) * size_divisibility
    mean = (C.c_float * Cn)(*[float(v) for v in pixel_mean])
    std = (C.c_float * Cn)(*[float(v) for v in pixel_std])
    out = torch.empty((len(images_chw), Cn, hm, wm), device=images_chw[0].device, dtype=torch.float32)
    for n, t in enumerate(images_chw):
        assert t.shape[0] == Cn
        call("afi_normalize_pad_u8", _p(t), Cn, t.shape[1], t.shape[2], mean, std, _p(out[n]), hm, wm, stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ frozen ResNet-FPN guide (resnet_guide.py)
def resnet_stem(x, w, bias):
    """detectron2's BasicStem with its FrozenBN folded into (w [64,3,7,7], bias [64]): max_pool2d(relu(conv7x7/2(x)), 3, 2, 1) in one kernel.
    x: the NCHW fp32 batch [N,3,H,W]; returns pixel-major [N,64,ceil(H/4),ceil(W/4)] (afi_resnet_stem_fwd)."""
    _check_cuda(x, w, bias)
    N, Cin, H, W = x.shape
    if Cin != 3 or tuple(w.shape) != (64, 3, 7, 7) or tuple(bias.shape) != (64,):
        raise _lib.AfiError(f"resnet_stem: a 3 -> 64 channel 7x7 stem only, got x {tuple(x.shape)}, w {tuple(w.shape)}")
    x, w, bias = x.contiguous(), w.contiguous(), bias.contiguous()
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = new_pixel_major(N, 64, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1, x.device)
    call("afi_resnet_stem_fwd", _p(x), N, H, W, _p(w), _p(bias), _p(out), stream_ptr())
    return out


def nearest(x, up=2, down=1):
    """Nearest resampling of a pixel-major tensor by up / down: F.interpolate(x, scale_factor=2, mode="nearest") (up=2), or the stride-2
    subsampling max_pool2d(x, 1, 2) of LastLevelMaxPool (down=2).  Returns a dense pixel-major tensor (afi_nearest_nhwc)."""
    _check_cuda(x)
    N, C_, H, W = x.shape
    out = new_pixel_major(N, C_, -(-H * up // down), -(-W * up // down), x.device)
    call("afi_nearest_nhwc", view_of(x), N, H, W, C_, int(up), int(down), _p(out), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ frozen ResNeSt bottom-up (resnest_backbone.py)
POOL_MODES = {m: _lib.DEFINES["AFI_POOL_" + m.upper()] for m in ("max3s2p1", "avg3s2p1", "avg2s2_ceil")}


def resnest_stem(x, w, bias):
    """The deep stem's first conv with its norm folded into (w [Cout,3,3,3], bias [Cout]): relu(conv2d(x, w, bias, stride 2, padding 1)).
    x: the NCHW fp32 batch [N,3,H,W]; returns pixel-major [N,Cout,ceil(H/2),ceil(W/2)] (afi_resnest_stem_fwd)."""
    _check_cuda(x, w, bias)
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    if Cin != 3 or tuple(w.shape) != (Cout, 3, 3, 3) or tuple(bias.shape) != (Cout,):
        raise _lib.AfiError(f"resnest_stem: a 3-channel 3x3 conv only, got x {tuple(x.shape)}, w {tuple(w.shape)}")
    x, w, bias = x.contiguous(), ohwi(w), bias.contiguous()
    out = new_pixel_major(N, Cout, (H + 1) // 2, (W + 1) // 2, x.device)
    call("afi_resnest_stem_fwd", _p(x), N, H, W, _p(w), _p(bias), Cout, _p(out), stream_ptr())
    return out


def resnest_pool(x, mode):
    """Pooling of a pixel-major tensor (afi_resnest_pool_nhwc); every mode gives [N,C,ceil(H/2),ceil(W/2)]:
    "max3s2p1" max_pool2d(3, 2, 1); "avg3s2p1" avg_pool2d(3, 2, 1) (count_include_pad: / 9); "avg2s2_ceil" avg_pool2d(2, 2, ceil_mode=True,
    count_include_pad=False)."""
    _check_cuda(x)
    N, C_, H, W = x.shape
    out = new_pixel_major(N, C_, (H + 1) // 2, (W + 1) // 2, x.device)
    call("afi_resnest_pool_nhwc", view_of(x), N, H, W, C_, POOL_MODES[mode], _p(out), stream_ptr())
    return out


def splat_attention(s0, s1, w1, b1, w2, b2, avd=False, keep=False):
    """Split attention (radix 2) over two pixel-major splits [N,C,H,W] (bn0 + ReLU already applied), in three passes: per-chunk channel sums
    of s0 + s1, the per-image attention att = rsoftmax(fc2(relu(fc1(mean)))) with w1 [I,C] (bn1 folded) and w2 [2C,I], and the combine
    att0 * s0 + att1 * s1 -- with avd, its avg_pool2d(3, 2, 1) in the same pass.  Returns (out, att [N, 2C]); with `keep` (the training
    forward, afi_resnest_splat_attn_keep: the same kernel) (out, att, g [N, C], h [N, I]), the pooled mean and fc1's post-ReLU output."""
    _check_cuda(s0, s1, w1, b1, w2, b2)
    N, C_, H, W = s0.shape
    I = w1.shape[0]
    if tuple(s1.shape) != tuple(s0.shape) or tuple(w1.shape[:2]) != (I, C_) or tuple(w2.shape[:2]) != (2 * C_, I):
        raise _lib.AfiError(f"splat_attention: splits {tuple(s0.shape)} / {tuple(s1.shape)}, fc1 {tuple(w1.shape)}, fc2 {tuple(w2.shape)}")
    w1, w2 = w1.reshape(I, C_).contiguous(), w2.reshape(2 * C_, I).contiguous()
    n = _lib.load().afi_resnest_splat_ws_floats(N, H, W, C_)
    if n <= 0:
        raise _lib.AfiError(f"splat_attention: unsupported split width {C_}")
    part = new_workspace(n, s0.device)
    att = torch.empty((N, 2 * C_), device=s0.device, dtype=torch.float32)
    call("afi_resnest_splat_gap", view_of(s0), view_of(s1), N, H, W, C_, _p(part), n, stream_ptr())
    if keep:
        g, h = torch.empty((N, C_), device=s0.device, dtype=torch.float32), torch.empty((N, I), device=s0.device, dtype=torch.float32)
        call("afi_resnest_splat_attn_keep", _p(part), N, H, W, C_, I, _p(w1), _p(b1.contiguous()), _p(w2), _p(b2.contiguous()), _p(att), _p(g),
             _p(h), stream_ptr())
    else:
        call("afi_resnest_splat_attn", _p(part), N, H, W, C_, I, _p(w1), _p(b1.contiguous()), _p(w2), _p(b2.contiguous()), _p(att), stream_ptr())
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if avd else (H, W)
    out = new_pixel_major(N, C_, Ho, Wo, s0.device)
    call("afi_resnest_splat_combine", view_of(s0), view_of(s1), N, H, W, C_, _p(att), int(bool(avd)), _p(out), stream_ptr())
    return (out, att, g, h) if keep else (out, att)


def _splat_bwd_shapes(name, dout, s0, s1, att, avd):
    N, C_, H, W = s0.shape
    want = (N, C_, (H + 1) // 2, (W + 1) // 2) if avd else (N, C_, H, W)
    if tuple(s1.shape) != (N, C_, H, W) or tuple(dout.shape) != want or tuple(att.shape) != (N, 2 * C_):
        raise _lib.AfiError(f"{name}: splits {tuple(s0.shape)} / {tuple(s1.shape)}, dout {tuple(dout.shape)} (expected {want}), att {tuple(att.shape)}")
    return N, C_, H, W


def splat_bwd_dots(dout, s0, s1, avd=False):
    """part [N, chunks, 2, C]: per-chunk sums over the pixels of du * s0 and du * s1 (afi_resnest_splat_bwd_dots), du the cotangent of the
    combine's un-pooled output: `dout` itself, or with avd the transposed avg_pool2d(3, 2, 1) of dout, gathered and never stored."""
    _check_cuda(dout, s0, s1)
    N, C_, H, W = s0.shape
    n = _lib.load().afi_resnest_splat_bwd_ws_floats(N, H, W, C_)
    if n <= 0:
        raise _lib.AfiError(f"splat_bwd_dots: unsupported split width {C_}")
    part = new_workspace(n, s0.device)
    call("afi_resnest_splat_bwd_dots", view_of(dout), view_of(s0), view_of(s1), N, H, W, C_, int(bool(avd)), _p(part), n, stream_ptr())
    return part.view(N, -1, 2, C_)


def splat_bwd_attn(part, hw, att, h, w1, w2):
    """(dz [N,2C], dh [N,I], dg [N,C]) from the partials of splat_bwd_dots (afi_resnest_splat_bwd_attn): dz0 = a0 a1 (da0 - da1), dz1 = -dz0,
    dh = (w2^T dz) [h > 0], dg = w1^T dh / (H W); w1 [I,C] with bn1 folded, hw = (H, W) of the splits."""
    _check_cuda(part, att, h, w1, w2)
    N, C_, I = att.shape[0], att.shape[1] // 2, h.shape[1]
    w1, w2 = w1.reshape(I, C_).contiguous(), w2.reshape(2 * C_, I).contiguous()
    if tuple(part.shape) != (N, part.shape[1], 2, C_) or not part.is_contiguous() or tuple(h.shape) != (N, I):
        raise _lib.AfiError(f"splat_bwd_attn: part {tuple(part.shape)}, att {tuple(att.shape)}, h {tuple(h.shape)}")
    if part.numel() != _lib.load().afi_resnest_splat_bwd_ws_floats(N, hw[0], hw[1], C_):
        raise _lib.AfiError(f"splat_bwd_attn: part {tuple(part.shape)} is not the partials of a {hw[0]}x{hw[1]} map of {C_} channels")
    dz, dh, dg = (torch.empty((N, k), device=att.device, dtype=torch.float32) for k in (2 * C_, I, C_))
    call("afi_resnest_splat_bwd_attn", _p(part), N, hw[0], hw[1], C_, I, _p(att.contiguous()), _p(h.contiguous()), _p(w1), _p(w2), _p(dz), _p(dh),
         _p(dg), stream_ptr())
    return dz, dh, dg


def splat_bwd_params(dz, dh, g, h, s1_scale, dw1, db1, dw2, db2):
    """dw2 += sum_n dz_n (x) h_n, db2 += sum_n dz_n, dw1 += s1 * sum_n dh_n (x) g_n, db1 += s1 * sum_n dh_n (afi_resnest_splat_bwd_params):
    straight into the gradients of fc1.{weight,bias} / fc2.{weight,bias} (contiguous), s1_scale [I] the fold scale of bn1."""
    _check_cuda(dz, dh, g, h, s1_scale, dw1, db1, dw2, db2)
    N, C_, I = g.shape[0], g.shape[1], h.shape[1]
    for name, t, n in (("dw1", dw1, I * C_), ("db1", db1, I), ("dw2", dw2, 2 * C_ * I), ("db2", db2, 2 * C_), ("s1_scale", s1_scale, I),
                       ("dz", dz, N * 2 * C_), ("dh", dh, N * I)):
        if t.numel() != n or not t.is_contiguous():
            raise _lib.AfiError(f"splat_bwd_params: {name} {tuple(t.shape)} is not a contiguous tensor of {n} elements")
    call("afi_resnest_splat_bwd_params", _p(dz), _p(dh), _p(g.contiguous()), _p(h.contiguous()), _p(s1_scale), N, C_, I, _p(dw1), _p(db1), _p(dw2),
         _p(db2), stream_ptr())


def splat_bwd_combine(dout, s0, s1, att, dg, avd=False, ds0=None, ds1=None):
    """ds_r = (att_r du + dg) * [s_r > 0] for r = 0, 1 (afi_resnest_splat_bwd_combine); ds0 / ds1 may be views, e.g. the halves of one
    [N,2C,H,W] tensor.  Masked elements are exact zeros."""
    _check_cuda(dout, s0, s1, att, dg, ds0, ds1)
    N, C_, H, W = _splat_bwd_shapes("splat_bwd_combine", dout, s0, s1, att, avd)
    if ds0 is None:
        ds0 = new_pixel_major(N, C_, H, W, s0.device)
    if ds1 is None:
        ds1 = new_pixel_major(N, C_, H, W, s0.device)
    if tuple(ds0.shape) != (N, C_, H, W) or tuple(ds1.shape) != (N, C_, H, W) or tuple(dg.shape) != (N, C_):
        raise _lib.AfiError(f"splat_bwd_combine: ds0 {tuple(ds0.shape)} / ds1 {tuple(ds1.shape)} / dg {tuple(dg.shape)} for splits {tuple(s0.shape)}")
    call("afi_resnest_splat_bwd_combine", view_of(dout), view_of(s0), view_of(s1), N, H, W, C_, _p(att.contiguous()), _p(dg.contiguous()),
         int(bool(avd)), view_of(ds0), view_of(ds1), stream_ptr())
    return ds0, ds1


def splat_attention_bwd(dout, s0, s1, att, g, h, w1, w2, s1_scale, avd, dw1, db1, dw2, db2, ds0=None, ds1=None):
    """The backward of `splat_attention` in four passes: splat_bwd_dots, splat_bwd_attn, splat_bwd_params (adding into the
    gradients dw1, db1, dw2, db2 of fc1 / fc2's PARAMETERS) and splat_bwd_combine.  Returns (ds0, ds1), the gradients of the two splits'
    pre-activations."""
    N, C_, H, W = _splat_bwd_shapes("splat_attention_bwd", dout, s0, s1, att, avd)
    part = splat_bwd_dots(dout, s0, s1, avd)
    dz, dh, dg = splat_bwd_attn(part, (H, W), att, h, w1, w2)
    splat_bwd_params(dz, dh, g, h, s1_scale, dw1, db1, dw2, db2)
    return splat_bwd_combine(dout, s0, s1, att, dg, avd, ds0, ds1)


def resnest_pool_bwd(dy, mode, dx=None, beta=0.0, z=None, in_hw=None):
    """dx = (beta * dx + pool^T(dy)) [* (z > 0)] (afi_resnest_pool_bwd) for "avg2s2_ceil" / "avg3s2p1" of `resnest_pool`; dx and z may be
    views of pixel-major tensors; without dx, in_hw = (H, W) of the pool's input names its size.  "max3s2p1" is refused by the library."""
    _check_cuda(dy, dx, z)
    N, C_, Ho, Wo = dy.shape
    if dx is None:
        if in_hw is None:
            raise _lib.AfiError("resnest_pool_bwd: dx= or in_hw= names the size of the pool's input")
        dx = new_pixel_major(N, C_, in_hw[0], in_hw[1], dy.device)
    H, W = dx.shape[2:]
    if tuple(dx.shape[:2]) != (N, C_) or ((H + 1) // 2, (W + 1) // 2) != (Ho, Wo) or (z is not None and z.shape != dx.shape):
        raise _lib.AfiError(f"resnest_pool_bwd: dy {tuple(dy.shape)} is not the pooled size of dx {tuple(dx.shape)}"
                            + (f" / z {tuple(z.shape)}" if z is not None else ""))
    if not is_dense_pm(dy):
        raise _lib.AfiError("resnest_pool_bwd: dy must be a dense pixel-major tensor")
    call("afi_resnest_pool_bwd", _p(dy), N, H, W, C_, POOL_MODES[mode], view_of(dx), float(beta), view_of(z) if z is not None else _NULL_VIEW,
         stream_ptr())
    return dx


# ------------------------------------------------------------------------------------------------ frozen Swin bottom-up (swin_backbone.py)
SWIN_WINDOWS = (7, 12)                      # window sizes afi_swin_window_attn covers


def swin_patch_embed(x, w, bias, gamma, beta, eps=1e-5):
    """PatchEmbed: LayerNorm(conv2d(x zero-padded to multiples of 4, w [C,3,4,4], bias, stride 4)) with (gamma, beta, eps).
    x: the NCHW fp32 batch [N,3,H,W]; returns pixel-major [N,C,ceil(H/4),ceil(W/4)] (afi_swin_patch_embed)."""
    _check_cuda(x, w, bias, gamma, beta)
    N, Cin, H, W = x.shape
    C_ = w.shape[0]
    if Cin != 3 or tuple(w.shape) != (C_, 3, 4, 4):
        raise _lib.AfiError(f"swin_patch_embed: a 3-channel 4x4 conv only, got x {tuple(x.shape)}, w {tuple(w.shape)}")
    out = new_pixel_major(N, C_, (H + 3) // 4, (W + 3) // 4, x.device)
    call("afi_swin_patch_embed", _p(x.contiguous()), N, H, W, _p(w.contiguous()), _p(bias.contiguous()), _p(gamma.contiguous()),
         _p(beta.contiguous()), float(eps), C_, _p(out), stream_ptr())
    return out


def swin_layernorm(x, gamma, beta, eps=1e-5, merge=False):
    """LayerNorm over the channels of a pixel-major [N,C,H,W] -> pixel-major [N,C,H,W]; merge: PatchMerging's 2x2 gather (odd H / W
    zero-padded, torch.cat([x0, x1, x2, x3]) order) and its LayerNorm over the 4C channels -> [N,4C,ceil(H/2),ceil(W/2)] (afi_swin_layernorm)."""
    _check_cuda(x, gamma, beta)
    N, C_, H, W = x.shape
    Ct, Ho, Wo = (4 * C_, (H + 1) // 2, (W + 1) // 2) if merge else (C_, H, W)
    if tuple(gamma.shape) != (Ct,) or tuple(beta.shape) != (Ct,):
        raise _lib.AfiError(f"swin_layernorm: affine of {Ct} channels expected, got {tuple(gamma.shape)} / {tuple(beta.shape)}")
    out = new_pixel_major(N, Ct, Ho, Wo, x.device)
    call("afi_swin_layernorm", view_of(x), N, H, W, C_, _p(gamma.contiguous()), _p(beta.contiguous()), float(eps), int(bool(merge)), _p(out),
         stream_ptr())
    return out


def swin_gelu_(x):
    """Exact (erf) GELU of a dense pixel-major tensor, in place (afi_swin_gelu)."""
    _check_cuda(x)
    if not is_dense_pm(x):
        raise _lib.AfiError("swin_gelu_: a dense pixel-major tensor is required")
    call("afi_swin_gelu", _p(x), x.numel(), stream_ptr())
    return x


def swin_bias_image(table, index, window):
    """The dense relative-position bias afi_swin_window_attn reads: [heads, NP, NP] with [h, i, j] = table[index[i, j], h] for i, j < window^2,
    zero elsewhere (NP = window^2 rounded up to 16)."""
    n = window * window
    NP = (n + 15) // 16 * 16
    heads = table.shape[1]
    img = torch.zeros((heads, NP, NP), device=table.device, dtype=torch.float32)
    img[:, :n, :n] = table.float()[index.reshape(-1).long()].reshape(n, n, heads).permute(2, 0, 1)
    return img


def swin_window_attn(qkv, qkv_bias, bias_img, window, shift):
    """(Shifted) window attention of a pixel-major qkv [N,3C,H,W] (head dim 32) -> pixel-major [N,C,H,W], the reference's
    pad / roll(-shift) / window_partition / WindowAttention (mask -100 across shift regions when shift > 0) / window_reverse / roll / crop
    in one pass; padded tokens' q / k / v are qkv_bias.  bias_img: swin_bias_image (afi_swin_window_attn)."""
    _check_cuda(qkv, qkv_bias, bias_img)
    N, C3, H, W = qkv.shape
    C_ = C3 // 3
    if C3 % 3 or C_ % 32 or window not in SWIN_WINDOWS or not 0 <= shift < window or tuple(qkv_bias.shape) != (C3,):
        raise _lib.AfiError(f"swin_window_attn: qkv {tuple(qkv.shape)} (head dim 32), window {window} (one of {SWIN_WINDOWS}), shift {shift}")
    NP = (window * window + 15) // 16 * 16
    if tuple(bias_img.shape) != (C_ // 32, NP, NP) or not bias_img.is_contiguous():
        raise _lib.AfiError(f"swin_window_attn: bias image {tuple(bias_img.shape)}, expected dense {(C_ // 32, NP, NP)}")
    out = new_pixel_major(N, C_, H, W, qkv.device)
    call("afi_swin_window_attn", view_of(qkv), N, H, W, C_, _p(qkv_bias.contiguous()), _p(bias_img), int(window), int(shift), _p(out),
         stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ training the Swin bottom-up
def swin_layernorm_bwd(dy, x, gamma, eps=1e-5, merge=False, dx=None, beta=0.0, dgamma=None, dbeta=None, want_dx=True):
    """The backward of ``swin_layernorm(x, gamma, ., eps, merge)`` for the dense pixel-major dy (afi_swin_layernorm_bwd): x-hat and rstd are
    recomputed from x.  Returns dx = beta * dx + the input gradient, a pixel-major tensor of x's shape or the view given as ``dx=`` (with
    merge: scattered to the four source pixels; every pixel of x receives exactly one store); ``want_dx=False``: None, only the parameter
    gradients.  dgamma / dbeta (both or neither, contiguous [Ct]) += the sums over tokens of dy * x-hat / dy."""
    _check_cuda(dy, x, gamma, dx, dgamma, dbeta)
    N, C_, H, W = x.shape
    Ct, Ho, Wo = (4 * C_, (H + 1) // 2, (W + 1) // 2) if merge else (C_, H, W)
    if tuple(dy.shape) != (N, Ct, Ho, Wo) or not is_dense_pm(dy) or tuple(gamma.shape) != (Ct,):
        raise _lib.AfiError(f"swin_layernorm_bwd: dy {tuple(dy.shape)} must be the dense pixel-major {(N, Ct, Ho, Wo)} and gamma [{Ct}] "
                            f"(got {tuple(gamma.shape)})")
    if (dgamma is None) != (dbeta is None):
        raise _lib.AfiError("swin_layernorm_bwd: dgamma and dbeta go together")
    for name, t in (("dgamma", dgamma), ("dbeta", dbeta)):
        if t is not None and (tuple(t.shape) != (Ct,) or not t.is_contiguous()):
            raise _lib.AfiError(f"swin_layernorm_bwd: {name} {tuple(t.shape)} must be a contiguous [{Ct}]")
    if want_dx:
        if dx is None:
            if beta != 0.0:
                raise _lib.AfiError("swin_layernorm_bwd: beta != 0 needs the dx= to add into")
            dx = new_pixel_major(N, C_, H, W, x.device)
        elif tuple(dx.shape) != (N, C_, H, W):
            raise _lib.AfiError(f"swin_layernorm_bwd: dx {tuple(dx.shape)} is not x's shape {(N, C_, H, W)}")
    elif dgamma is None:
        raise _lib.AfiError("swin_layernorm_bwd: nothing to compute (no dx, no parameter gradients)")
    ws, need = None, 0
    if dgamma is not None:
        need = int(_lib.load().afi_swin_layernorm_bwd_ws_floats(N, H, W, C_, int(bool(merge))))
        ws = new_workspace(need, x.device)
    call("afi_swin_layernorm_bwd", view_of(x), N, H, W, C_, _p(gamma.contiguous()), float(eps), int(bool(merge)), _p(dy),
         view_of(dx) if want_dx else _NULL_VIEW, float(beta), _p(dgamma), _p(dbeta), _p(ws), need, stream_ptr())
    return dx if want_dx else None


def swin_gelu_bwd(dy, x, out=None):
    """dy * (Phi(x) + x phi(x)), x the GELU's input; dense pixel-major tensors of one shape; ``out=dy`` runs in place (afi_swin_gelu_bwd)."""
    _check_cuda(dy, x, out)
    if out is None:
        out = new_pixel_major(*x.shape, x.device)
    if dy.shape != x.shape or out.shape != x.shape or not (is_dense_pm(x) and is_dense_pm(dy) and is_dense_pm(out)):
        raise _lib.AfiError(f"swin_gelu_bwd: dense pixel-major tensors of one shape are required (x {tuple(x.shape)}, dy {tuple(dy.shape)})")
    call("afi_swin_gelu_bwd", _p(x), _p(dy), _p(out), x.numel(), stream_ptr())
    return out


def swin_window_attn_bwd(dout, qkv, qkv_bias, bias_img, window, shift):
    """The backward of ``swin_window_attn(qkv, qkv_bias, bias_img, window, shift)`` for dout [N,C,H,W] (afi_swin_window_attn_bwd).
    Returns (dqkv_padded, ds_part):
      dqkv_padded  pixel-major [N,3C,Hp,Wp] over the PADDED map: ``[:, :, :H, :W]`` is the gradient of qkv, the sum over every position (the
                   padded ones too: their q / k / v are the bias) the gradient of qkv_bias;
      ds_part      [N * groups, heads, NP, NP]: the sums of dS over groups of windows, what ``swin_bias_table_bwd`` reduces."""
    _check_cuda(dout, qkv, qkv_bias, bias_img)
    N, C3, H, W = qkv.shape
    C_ = C3 // 3
    if C3 % 3 or C_ % 32 or window not in SWIN_WINDOWS or not 0 <= shift < window or tuple(qkv_bias.shape) != (C3,) \
            or tuple(dout.shape) != (N, C_, H, W):
        raise _lib.AfiError(f"swin_window_attn_bwd: qkv {tuple(qkv.shape)} (head dim 32), dout {tuple(dout.shape)}, window {window} "
                            f"(one of {SWIN_WINDOWS}), shift {shift}")
    NP = (window * window + 15) // 16 * 16
    heads = C_ // 32
    if tuple(bias_img.shape) != (heads, NP, NP) or not bias_img.is_contiguous():
        raise _lib.AfiError(f"swin_window_attn_bwd: bias image {tuple(bias_img.shape)}, expected dense {(heads, NP, NP)}")
    Hp, Wp = -(-H // window) * window, -(-W // window) * window
    lib = _lib.load()
    groups = int(lib.afi_swin_window_attn_bwd_groups(N, H, W, C_, int(window)))
    floats = int(lib.afi_swin_window_attn_bwd_ws_floats(N, H, W, C_, int(window)))
    if groups <= 0 or floats != N * groups * heads * NP * NP:
        raise _lib.AfiError(f"swin_window_attn_bwd: the library sizes the dS workspace as {floats} floats in {groups} groups")
    dqkv = new_pixel_major(N, C3, Hp, Wp, qkv.device)
    ds_part = new_workspace(floats, qkv.device).view(N * groups, heads, NP, NP)
    call("afi_swin_window_attn_bwd", view_of(qkv), view_of(dout), N, H, W, C_, _p(qkv_bias.contiguous()), _p(bias_img), int(window), int(shift),
         _p(dqkv), _p(ds_part), floats, stream_ptr())
    return dqkv, ds_part


def swin_bias_csr(index, window, rows):
    """The CSR of a relative_position_index buffer as loaded, for ``swin_bias_table_bwd``: (row_off int32 [rows + 1], pairs int32 [window^4])
    on the index's device, pairs = i * NP + j of the (i, j) with index[i, j] = r, ascending within each row.  Built on the host, once per
    buffer (the caller caches it)."""
    n = window * window
    NP = (n + 15) // 16 * 16
    idx = index.detach().reshape(-1).cpu().long()
    if idx.numel() != n * n or int(idx.min()) < 0 or int(idx.max()) >= rows:
        raise _lib.AfiError(f"swin_bias_csr: relative_position_index of {idx.numel()} entries does not index a {rows}-row table over window {window}")
    order = torch.sort(idx, stable=True).indices                            # ascending r, then ascending (i, j)
    pairs = ((order // n) * NP + order % n).to(torch.int32)
    row_off = torch.zeros(rows + 1, dtype=torch.int64)
    row_off[1:] = torch.cumsum(torch.bincount(idx, minlength=rows), 0)
    return row_off.to(torch.int32).to(index.device), pairs.to(index.device)


def swin_bias_table_bwd(ds_part, csr, window, dtable):
    """dtable [R, heads] += the sum over ds_part's partials and the pairs of each table row (afi_swin_bias_table_bwd: fp64, one fixed order);
    csr: ``swin_bias_csr``."""
    _check_cuda(ds_part, dtable)
    row_off, pairs = csr
    NP = (window * window + 15) // 16 * 16
    R, heads = dtable.shape
    if ds_part.dim() != 4 or tuple(ds_part.shape[1:]) != (heads, NP, NP) or not ds_part.is_contiguous() or not dtable.is_contiguous() \
            or row_off.numel() != R + 1 or pairs.numel() != (window * window) ** 2 or row_off.dtype != torch.int32 or pairs.dtype != torch.int32 \
            or not (row_off.is_cuda and pairs.is_cuda):
        raise _lib.AfiError(f"swin_bias_table_bwd: ds_part {tuple(ds_part.shape)} / dtable {tuple(dtable.shape)} / csr ({row_off.numel()}, "
                            f"{pairs.numel()}) do not fit window {window} (partials [P, heads, {NP}, {NP}], int32 CSR on the GPU)")
    need = int(_lib.load().afi_swin_bias_table_bwd_ws_floats(heads, int(window)))
    ws = new_workspace(need, ds_part.device)
    call("afi_swin_bias_table_bwd", _p(ds_part), ds_part.shape[0], heads, int(window), _p(row_off), _p(pairs), R, _p(dtable), _p(ws), need,
         stream_ptr())
    return dtable


def swin_patch_gather(x):
    """The zero-padded 4x4x3 patches of the NCHW batch x [N,3,H,W] as pixel-major [N,48,ceil(H/4),ceil(W/4)], channel 16 ci + 4 ky + kx: the
    order of ``proj.weight.reshape(C, 48)``, so PatchEmbed's conv is a 1x1 over it (afi_swin_patch_gather)."""
    _check_cuda(x)
    N, Cin, H, W = x.shape
    if Cin != 3:
        raise _lib.AfiError(f"swin_patch_gather: a 3-channel batch only, got {tuple(x.shape)}")
    out = new_pixel_major(N, 48, (H + 3) // 4, (W + 3) // 4, x.device)
    call("afi_swin_patch_gather", _p(x.contiguous()), N, H, W, _p(out), stream_ptr())
    return out


def swin_scale_add(a, s, b, out=None):
    """out = a + s[n] * b over dense pixel-major tensors (DropPath; a None: out = s[n] * b); s a [N] fp32 vector on the device
    (afi_swin_scale_add).  ``out`` may be a or b."""
    _check_cuda(a, s, b, out)
    if out is None:
        out = new_pixel_major(*b.shape, b.device)
    N = b.shape[0]
    if tuple(s.shape) != (N,) or not s.is_contiguous() or any(t is not None and (t.shape != b.shape or not is_dense_pm(t)) for t in (a, b, out)):
        raise _lib.AfiError(f"swin_scale_add: dense pixel-major tensors of one shape and s [{N}] are required (b {tuple(b.shape)}, s {tuple(s.shape)})")
    call("afi_swin_scale_add", _p(a), _p(b), _p(s), N, b.numel() // N, _p(out), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ RPN selection (rpn.py)
RPN_MAX_TOPK = 1024                         # per-level list length the selection kernels hold in LDS
RPN_MAX_ANCHORS = 16
RPN_MAX_LEVELS = 8


def _check_i32(*ts):
    for t in ts:
        if not t.is_cuda:
            raise _lib.AfiError("the RPN selection runs on the GPU only (got a CPU tensor); there is no CPU fallback")
        if t.dtype != torch.int32:
            raise _lib.AfiError(f"int32 expected, got {t.dtype}")


def _rpn_rows(t, k, inner=()):
    """`t` is rows of one level's list: [N, >= k, *inner], dense inside a row; returns the row stride in list elements."""
    per = 1
    for s in inner:
        per *= s
    if t.dim() != 2 + len(inner) or t.shape[1] < k or tuple(t.shape[2:]) != tuple(inner) or not t[0].is_contiguous() or t.stride(0) % per:
        raise _lib.AfiError(f"rpn: a list buffer [N, >= {k}{''.join(', ' + str(s) for s in inner)}] with dense rows expected, got shape "
                            f"{tuple(t.shape)} strides {t.stride()}")
    return t.stride(0) // per


def _rpn_topk(name, k_lo, k_hi, head, A, k, vals, idx):
    """The body of rpn_topk / rpn_topk_wide: k_lo <= k <= k_hi, the entry points afi_<name> and afi_<name>_ws_floats."""
    _check_cuda(head)
    N, Cp, H, W = head.shape
    if not 0 < A <= min(Cp, RPN_MAX_ANCHORS) or not k_lo <= k <= min(k_hi, H * W * A):
        raise _lib.AfiError(f"{name}: A {A} (1..{min(Cp, RPN_MAX_ANCHORS)}), k {k} ({k_lo}..{min(k_hi, H * W * A)}) for a head of shape {tuple(head.shape)}")
    if vals is None:
        vals = torch.empty((N, k), device=head.device, dtype=torch.float32)
        idx = torch.empty((N, k), device=head.device, dtype=torch.int32)
    _check_cuda(vals)
    _check_i32(idx)
    ld = _rpn_rows(vals, k)
    if vals.shape[0] != N or idx.shape[0] != N or _rpn_rows(idx, k) != ld:
        raise _lib.AfiError(f"{name}: vals and idx must be [N, >= k] with one row stride")
    n = getattr(_lib.load(), f"afi_{name}_ws_floats")(N, H, W, A)
    if n < 0:
        raise _lib.AfiError(f"{name}: unsupported map {H}x{W}x{A}")
    ws = new_workspace(n, head.device) if n else None
    call(f"afi_{name}", view_of(head), N, H, W, A, k, _p(vals), _p(idx), ld, _p(ws), n, stream_ptr())
    return vals, idx


def rpn_topk(head, A, k, vals=None, idx=None):
    """The k highest of channels 0..A-1 of the pixel-major head output [N, Cpad, H, W], per image: (vals [N, k] fp32, idx [N, k] int32), sorted
    by (logit descending, anchor index (y W + x) A + a ascending); NaN below every number (afi_rpn_topk).  vals / idx may be column slices of wider
    [N, K] buffers (the levels of an image side by side)."""
    return _rpn_topk("rpn_topk", 1, RPN_MAX_TOPK, head, A, k, vals, idx)


def rpn_decode(head, c0, A, cell_anchors, stride, idx, k, image_hw, weights=(1.0, 1.0, 1.0, 1.0), scale_clamp=4.135166556742356, min_size=0.0,
               boxes=None, valid=None):
    """Boxes of the anchors idx [N, k] of one level: deltas = channels c0 + 4 a + c of the pixel-major head output, anchors from the index and
    cell_anchors [A, 4], Box2BoxTransform(weights) with dw / dh clamped at scale_clamp, clipped to image_hw [N, 2] (device fp32: height, width);
    returns (boxes [N, k, 4], valid [N, k] int32 = both sides > min_size) (afi_rpn_decode)."""
    _check_cuda(head, cell_anchors, image_hw)
    _check_i32(idx)
    N, Cp, H, W = head.shape
    if not 0 < A <= RPN_MAX_ANCHORS or c0 < 0 or c0 + 4 * A > Cp or tuple(cell_anchors.shape) != (A, 4) or tuple(image_hw.shape) != (N, 2):
        raise _lib.AfiError(f"rpn_decode: head {tuple(head.shape)}, deltas at channel {c0}, A {A}, cell anchors {tuple(cell_anchors.shape)}, "
                            f"image sizes {tuple(image_hw.shape)}")
    if boxes is None:
        boxes = torch.empty((N, k, 4), device=head.device, dtype=torch.float32)
        valid = torch.empty((N, k), device=head.device, dtype=torch.int32)
    _check_cuda(boxes)
    _check_i32(valid)
    ld = _rpn_rows(idx, k)
    if _rpn_rows(boxes, k, (4,)) != ld or _rpn_rows(valid, k) != ld or not (idx.shape[0] == boxes.shape[0] == valid.shape[0] == N):
        raise _lib.AfiError("rpn_decode: idx, boxes and valid must be lists of one row stride")
    v = view_of(head)
    v.p += 4 * c0
    call("afi_rpn_decode", v, N, H, W, A, _p(cell_anchors.contiguous()), int(stride), _p(idx), k, ld, _p(image_hw.contiguous()),
         *[float(w) for w in weights], float(scale_clamp), float(min_size), _p(boxes), _p(valid), stream_ptr())
    return boxes, valid


def _rpn_nms(name, k_max, ws_query, boxes, valid, thresh, keep):
    """The body of rpn_nms / rpn_nms_wide: lists of at most k_max boxes; ws_query (N, k) -> floats of workspace, None for the form without one."""
    _check_cuda(boxes)
    _check_i32(valid)
    N, k = valid.shape
    if keep is None:
        keep = torch.empty((N, k), device=boxes.device, dtype=torch.int32)
    _check_i32(keep)
    if k > k_max:
        raise _lib.AfiError(f"{name}: lists of at most {k_max} boxes, got {k}")
    if k == 0:
        return keep
    ld = _rpn_rows(valid, k)
    if _rpn_rows(boxes, k, (4,)) != ld or _rpn_rows(keep, k) != ld or not (boxes.shape[0] == keep.shape[0] == N):
        raise _lib.AfiError(f"{name}: boxes, valid and keep must be lists of one row stride")
    if ws_query is None:
        call(f"afi_{name}", _p(boxes), _p(valid), N, k, ld, float(thresh), _p(keep), stream_ptr())
        return keep
    n = ws_query(N, k)
    ws = new_workspace(n, boxes.device)                      # held until after the launch
    call(f"afi_{name}", _p(boxes), _p(valid), N, k, ld, float(thresh), _p(keep), _p(ws), n, stream_ptr())
    return keep


def rpn_nms(boxes, valid, thresh, keep=None):
    """Greedy NMS of the lists boxes [N, k, 4] (k <= 1024, in score order), valid [N, k] int32: keep [N, k] int32 (afi_rpn_nms)."""
    return _rpn_nms("rpn_nms", RPN_MAX_TOPK, None, boxes, valid, thresh, keep)


def _rpn_merge(name, level_max, total_max, boxes, vals, keep, level_off, post_k):
    """The body of rpn_merge / rpn_merge_wide.  level_max None: the level and total bounds are left to afi_rpn_merge (RPN_MAX_TOPK a level)."""
    _check_cuda(boxes, vals)
    _check_i32(keep)
    N, K = vals.shape
    L = len(level_off) - 1
    if not (boxes.is_contiguous() and vals.is_contiguous() and keep.is_contiguous()) or tuple(boxes.shape) != (N, K, 4) or tuple(keep.shape) != (N, K) \
            or level_off[0] != 0 or level_off[-1] != K or not 0 < L <= RPN_MAX_LEVELS or post_k <= 0:
        raise _lib.AfiError(f"{name}: dense boxes [N, K, 4], vals / keep [N, K] and 1..{RPN_MAX_LEVELS} levels ending at K expected, got "
                            f"{tuple(boxes.shape)}, {tuple(vals.shape)}, {tuple(keep.shape)}, offsets {list(level_off)}")
    if level_max is not None and (K > total_max or any(level_off[l + 1] - level_off[l] > level_max for l in range(L))):
        raise _lib.AfiError(f"{name}: levels of at most {level_max} entries, {total_max} in all; got offsets {list(level_off)}")
    ob = torch.empty((N, post_k, 4), device=boxes.device, dtype=torch.float32)
    ol = torch.empty((N, post_k), device=boxes.device, dtype=torch.float32)
    counts = torch.empty((N,), device=boxes.device, dtype=torch.int32)
    off = (C.c_int * (L + 1))(*[int(o) for o in level_off])
    call(f"afi_{name}", _p(boxes), _p(vals), _p(keep), N, L, off, int(post_k), _p(ob), _p(ol), _p(counts), stream_ptr())
    return ob, ol, counts


def rpn_merge(boxes, vals, keep, level_off, post_k):
    """The kept entries of every level of an image in (logit descending, level, rank) order, the first post_k: boxes [N, K, 4], vals / keep
    [N, K] dense with level l in columns [level_off[l], level_off[l + 1]); returns (boxes [N, post_k, 4], logits [N, post_k], counts [N] int32),
    rows past counts zero (afi_rpn_merge)."""
    # no bounds here: a level above RPN_MAX_TOPK has always been refused by afi_rpn_merge itself, with the library's status message
    return _rpn_merge("rpn_merge", None, None, boxes, vals, keep, level_off, post_k)


# The wide forms: per-level lists of 1025 .. 4096 (PRE_NMS_TOPK_TRAIN of the reference's base config is 2000).  RPN.select uses them for the
# levels whose list is longer than RPN_MAX_TOPK; the functions above keep their limits.
RPN_MAX_TOPK_WIDE = 4096                    # 64 x 64: the suppressed set of the NMS sweep is one 64-bit word per lane of a wave
RPN_MAX_MERGE_WIDE = 5 * RPN_MAX_TOPK_WIDE  # entries of all levels of an image rpn_merge_wide holds


def rpn_topk_wide(head, A, k, vals=None, idx=None):
    """rpn_topk for RPN_MAX_TOPK < k <= RPN_MAX_TOPK_WIDE: the same order, tie rule, NaN rule and output layout (afi_rpn_topk_wide).  A k of
    at most RPN_MAX_TOPK is rpn_topk's and is refused here."""
    return _rpn_topk("rpn_topk_wide", RPN_MAX_TOPK + 1, RPN_MAX_TOPK_WIDE, head, A, k, vals, idx)


def rpn_nms_wide(boxes, valid, thresh, keep=None):
    """rpn_nms for lists of up to RPN_MAX_TOPK_WIDE boxes, the suppression bit matrix in a workspace (afi_rpn_nms_wide).  For k <= RPN_MAX_TOPK
    the keep set is rpn_nms's."""
    return _rpn_nms("rpn_nms_wide", RPN_MAX_TOPK_WIDE, lambda N, k: _lib.load().afi_rpn_nms_wide_ws_floats(N, k), boxes, valid, thresh, keep)


def rpn_merge_wide(boxes, vals, keep, level_off, post_k):
    """rpn_merge with levels of up to RPN_MAX_TOPK_WIDE entries, at most RPN_MAX_MERGE_WIDE over all levels (afi_rpn_merge_wide)."""
    return _rpn_merge("rpn_merge_wide", RPN_MAX_TOPK_WIDE, RPN_MAX_MERGE_WIDE, boxes, vals, keep, level_off, post_k)


# ------------------------------------------------------------------------------------------------ RPN training (rpn.py: RPN.losses)
RPN_MAX_TOTAL_ANCHORS = 1 << 22             # anchors of one image over all levels: an index is 22 bits of a select word
RPN_MAX_GT = 1024                           # ground-truth boxes per image (four LDS tiles of 256)
RPN_MAX_BATCH = 4096                        # BATCH_SIZE_PER_IMAGE


def _rpn_train_levels(name, level_hw, strides, cell_anchors, A):
    """The checks rpn_match and rpn_loss share; returns (L, R, host level_hw array, host strides array, dense cell anchors)."""
    L = len(level_hw)
    if not 0 < L <= RPN_MAX_LEVELS or len(strides) != L:
        raise _lib.AfiError(f"{name}: 1..{RPN_MAX_LEVELS} levels with one stride each, got {L} maps and {len(strides)} strides")
    if not 0 < A <= RPN_MAX_ANCHORS or any(int(h) <= 0 or int(w) <= 0 for h, w in level_hw) or any(int(s) <= 0 for s in strides):
        raise _lib.AfiError(f"{name}: A {A} (1..{RPN_MAX_ANCHORS}), positive map sizes and strides expected, got {list(level_hw)}, {list(strides)}")
    R = sum(int(h) * int(w) * A for h, w in level_hw)
    if R > RPN_MAX_TOTAL_ANCHORS:
        raise _lib.AfiError(f"{name}: {R} anchors per image; at most {RPN_MAX_TOTAL_ANCHORS} (2^22) are supported")
    if tuple(cell_anchors.shape) != (L, A, 4):
        raise _lib.AfiError(f"{name}: cell anchors [{L}, {A}, 4] expected, got {tuple(cell_anchors.shape)}")
    hw = (C.c_int * (2 * L))(*[int(s) for p in level_hw for s in p])
    st = (C.c_int * L)(*[int(s) for s in strides])
    return L, R, hw, st


def _rpn_gt(name, gt, counts, cell_anchors):
    """Shapes and limits first, then devices and dtypes (so that a limit is named whatever the tensors live on); returns (N, Gmax)."""
    if gt.dim() != 3 or gt.shape[2] != 4 or gt.shape[1] < 1 or not gt.is_contiguous() or tuple(counts.shape) != (gt.shape[0],) or not counts.is_contiguous():
        raise _lib.AfiError(f"{name}: dense ground truth [N, Gmax >= 1, 4] and counts [N] expected, got {tuple(gt.shape)} and {tuple(counts.shape)}")
    if gt.shape[1] > RPN_MAX_GT:
        raise _lib.AfiError(f"{name}: {gt.shape[1]} ground-truth boxes per image; at most {RPN_MAX_GT} are supported")
    _check_cuda(gt, cell_anchors)
    _check_i32(counts)
    return gt.shape[0], gt.shape[1]


def rpn_match(level_hw, strides, cell_anchors, A, gt, counts, thresholds=(0.3, 0.7)):
    """Anchor labels of detectron2's RPN (Matcher with IOU_LABELS [0, -1, 1] and low-quality matches) over all levels: level_hw = [(H, W), ...],
    cell_anchors [L, A, 4], gt [N, Gmax, 4] fp32 with counts [N] int32.  Returns (labels [N, R] int8, matched_idx [N, R] int32), R the anchors
    of an image in level order, index (y W + x) A + a inside a level (afi_rpn_match)."""
    L, R, hw, st = _rpn_train_levels("rpn_match", level_hw, strides, cell_anchors, A)
    N, Gmax = _rpn_gt("rpn_match", gt, counts, cell_anchors)
    cell = cell_anchors.contiguous()
    t0, t1 = (float(t) for t in thresholds)
    if not t0 <= t1:
        raise _lib.AfiError(f"rpn_match: thresholds {thresholds} must ascend")
    labels = torch.empty((N, R), device=gt.device, dtype=torch.int8)
    midx = torch.empty((N, R), device=gt.device, dtype=torch.int32)
    ws = new_workspace(N * Gmax, gt.device)
    call("afi_rpn_match", hw, st, L, int(A), _p(cell), N, _p(gt), _p(counts), Gmax, t0, t1, _p(labels), _p(midx), _p(ws), N * Gmax, stream_ptr())
    return labels, midx


def rpn_sample(labels, keys, batch_per_image, positive_fraction):
    """subsample_labels with caller-supplied randomness: of labels [N, R] int8, the min(#positives, int(batch_per_image positive_fraction))
    positives and the min(#negatives, batch_per_image - num_pos) negatives with the smallest (key, anchor index) stay, every other label
    becomes -1.  keys [N, R]: 32 bits per anchor (int32 or uint32 storage), compared unsigned.  Returns (labels [N, R] int8 -- a new tensor --,
    sampled_idx [N, batch_per_image] int32: positives in ascending index, then negatives, then -1; n_pos [N], n_neg [N] int32) (afi_rpn_sample)."""
    for t in (labels, keys):
        if not t.is_cuda:
            raise _lib.AfiError("the RPN sampling runs on the GPU only (got a CPU tensor); there is no CPU fallback")
    if labels.dtype != torch.int8 or keys.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
        raise _lib.AfiError(f"rpn_sample: int8 labels and 32-bit integer keys expected, got {labels.dtype} and {keys.dtype}")
    if labels.dim() != 2 or keys.shape != labels.shape or not labels.is_contiguous() or not keys.is_contiguous():
        raise _lib.AfiError(f"rpn_sample: dense labels and keys [N, R] expected, got {tuple(labels.shape)} and {tuple(keys.shape)}")
    N, R = labels.shape
    B = int(batch_per_image)
    if R > RPN_MAX_TOTAL_ANCHORS:
        raise _lib.AfiError(f"rpn_sample: {R} anchors per image; at most {RPN_MAX_TOTAL_ANCHORS} (2^22) are supported")
    if not 0 < B <= RPN_MAX_BATCH or not 0.0 <= float(positive_fraction) <= 1.0:
        raise _lib.AfiError(f"rpn_sample: batch size per image {batch_per_image} (1..{RPN_MAX_BATCH}), positive fraction {positive_fraction} (0..1)")
    out = torch.empty_like(labels)
    sidx = torch.empty((N, B), device=labels.device, dtype=torch.int32)
    n_pos = torch.empty((N,), device=labels.device, dtype=torch.int32)
    n_neg = torch.empty((N,), device=labels.device, dtype=torch.int32)
    call("afi_rpn_sample", _p(labels), _p(keys), N, R, B, int(B * float(positive_fraction)), _p(out), _p(sidx), _p(n_pos), _p(n_neg), stream_ptr())
    return out, sidx, n_pos, n_neg


def rpn_loss(heads, strides, cell_anchors, A, gt, counts, matched_idx, sampled_idx, n_pos, n_neg, weights=(1.0, 1.0, 1.0, 1.0), beta=0.0,
             scale_cls=1.0, scale_loc=1.0):
    """rpn_losses over the sampled anchors: heads = the pixel-major head outputs [N, Cpad, H_l, W_l] (channel a the logit, A + 4 a + c the
    deltas).  Returns (loss [2] fp32 on the device: scale_cls * sum of the objectness terms, scale_loc * sum of the smooth-L1 terms of the
    positives; grads: per level a dense pixel-major tensor like the head output holding d loss[0] / d logit and d loss[1] / d delta, exactly
    zero outside the sample) (afi_rpn_loss)."""
    L, R, hw, st = _rpn_train_levels("rpn_loss", [tuple(h.shape[2:]) for h in heads], strides, cell_anchors, A)
    N, Gmax = _rpn_gt("rpn_loss", gt, counts, cell_anchors)
    _check_cuda(*heads)
    cell = cell_anchors.contiguous()
    _check_i32(matched_idx, sampled_idx, n_pos, n_neg)
    if any(h.dim() != 4 or h.shape[0] != N or h.shape[1] < 5 * A for h in heads):
        raise _lib.AfiError(f"rpn_loss: every head output must be [N = {N}, >= {5 * A}, H, W], got {[tuple(h.shape) for h in heads]}")
    B = sampled_idx.shape[1] if sampled_idx.dim() == 2 else 0
    if tuple(matched_idx.shape) != (N, R) or tuple(sampled_idx.shape) != (N, B) or tuple(n_pos.shape) != (N,) or tuple(n_neg.shape) != (N,) \
            or not (matched_idx.is_contiguous() and sampled_idx.is_contiguous() and n_pos.is_contiguous() and n_neg.is_contiguous()):
        raise _lib.AfiError(f"rpn_loss: dense matched_idx [{N}, {R}], sampled_idx [{N}, B], n_pos / n_neg [{N}] expected, got "
                            f"{tuple(matched_idx.shape)}, {tuple(sampled_idx.shape)}, {tuple(n_pos.shape)}, {tuple(n_neg.shape)}")
    if not 0 < B <= RPN_MAX_BATCH or len(weights) != 4 or min(weights) <= 0 or not beta >= 0:
        raise _lib.AfiError(f"rpn_loss: batch size per image {B} (1..{RPN_MAX_BATCH}), four positive weights and beta >= 0 expected")
    grads = [new_pixel_major(*h.shape, h.device, zero=True) for h in heads]
    loss = torch.empty((2,), device=gt.device, dtype=torch.float32)
    hv = (View * L)(*[view_of(h) for h in heads])
    gv = (View * L)(*[view_of(g) for g in grads])
    call("afi_rpn_loss", hv, gv, hw, st, L, int(A), _p(cell), N, _p(gt), Gmax, _p(matched_idx), _p(sampled_idx), B, _p(n_pos), _p(n_neg),
         *[float(w) for w in weights], float(beta), float(scale_cls), float(scale_loc), _p(loss), stream_ptr())
    return loss, grads


# ------------------------------------------------------------------------------------------------ ROI heads, box branch (roi_heads.py)
ROI_MAX_CANDIDATES = 1024                   # M: the per-image candidate list afi_roi_nms holds in LDS
ROI_MAX_POOLED = 14
ROI_MAX_CLASSES = 1024


def roi_align(levels, min_level, boxes, counts, S, sampling_ratio=0, out=None):
    """Multi-level ROIAlignV2 (aligned): levels = pixel-major [N, C, H_l, W_l] views with strides 2^(min_level + l), boxes [N, P, 4] with
    counts [N] int32 (RPN.forward_padded's layout); returns the pixel-major [N P, C, S, S] pooled features, rows past counts zero
    (afi_roi_align)."""
    _check_cuda(boxes, out, *levels)
    _check_i32(counts)
    L = len(levels)
    if not 0 < L <= RPN_MAX_LEVELS:
        raise _lib.AfiError(f"roi_align: 1..{RPN_MAX_LEVELS} levels, got {L}")
    N, C_ = levels[0].shape[:2]
    if boxes.dim() != 3 or boxes.shape[0] != N or boxes.shape[2] != 4 or not boxes.is_contiguous() or tuple(counts.shape) != (N,) \
            or not counts.is_contiguous():
        raise _lib.AfiError(f"roi_align: dense boxes [{N}, P, 4] and counts [{N}] expected, got {tuple(boxes.shape)} and {tuple(counts.shape)}")
    if any(x.dim() != 4 or x.shape[0] != N or x.shape[1] != C_ for x in levels) or C_ % 4:
        raise _lib.AfiError(f"roi_align: every level must be [N, C, H, W] with one N and one C % 4 == 0, got {[tuple(x.shape) for x in levels]}")
    if not 0 < S <= ROI_MAX_POOLED or sampling_ratio < 0:
        raise _lib.AfiError(f"roi_align: pooled size {S} (1..{ROI_MAX_POOLED}), sampling_ratio {sampling_ratio} (>= 0)")
    P = boxes.shape[1]
    if out is None:
        out = new_pixel_major(N * P, C_, S, S, boxes.device)
    elif tuple(out.shape) != (N * P, C_, S, S) or not is_dense_pm(out):
        raise _lib.AfiError(f"roi_align: out must be a dense pixel-major [{N * P}, {C_}, {S}, {S}] tensor")
    views = (View * L)(*[view_of(x) for x in levels])
    hw = (C.c_int * (2 * L))(*[int(s) for x in levels for s in x.shape[2:]])
    call("afi_roi_align", views, hw, L, int(min_level), N, C_, _p(boxes), _p(counts), P, int(S), int(sampling_ratio), _p(out), stream_ptr())
    return out


def _roi_pred_rows(name, pred, K, Kb, proposals, counts, image_hw):
    """The checks roi_scores_boxes and roi_cascade_stage share; returns (pred as its [N P, Cpad] matrix, N, P)."""
    _check_cuda(pred, proposals, image_hw)
    _check_i32(counts)
    N, P = proposals.shape[:2]
    p2 = pred.reshape(pred.shape[0], -1) if pred.dim() == 4 and pred.shape[2:] == (1, 1) and pred.stride(1) == 1 else pred
    if p2.dim() != 2 or p2.shape[0] != N * P or p2.shape[1] < K + 1 + 4 * Kb or p2.stride(1) != 1 or not 0 < K <= ROI_MAX_CLASSES \
            or tuple(proposals.shape) != (N, P, 4) or tuple(image_hw.shape) != (N, 2) or tuple(counts.shape) != (N,):
        raise _lib.AfiError(f"{name}: pred [{N * P}, >= {K + 1 + 4 * Kb}] with dense rows, proposals [N, P, 4], image sizes [N, 2], "
                            f"counts [N] and 1 <= K <= {ROI_MAX_CLASSES} expected, got {tuple(pred.shape)}, {tuple(proposals.shape)}, "
                            f"{tuple(image_hw.shape)}, {tuple(counts.shape)}, K {K}")
    return p2, N, P


def roi_scores_boxes(pred, K, agnostic, proposals, counts, image_hw, weights, scale_clamp=4.135166556742356):
    """pred: the predictor's output, pixel-major [N P, Cpad, 1, 1] (or [N P, Cpad]): K + 1 class logits (background last), then 4 K (or 4,
    agnostic) deltas.  Returns (scores [N, P, K] fp32 = softmax without the background column, -inf past counts; boxes [N, P, K or 1, 4] decoded
    from proposals [N, P, 4] and clipped to image_hw [N, 2]) (afi_roi_scores_boxes)."""
    Kb = 1 if agnostic else K
    p2, N, P = _roi_pred_rows("roi_scores_boxes", pred, K, Kb, proposals, counts, image_hw)
    scores = torch.empty((N, P, K), device=pred.device, dtype=torch.float32)
    boxes = torch.empty((N, P, Kb, 4), device=pred.device, dtype=torch.float32)
    call("afi_roi_scores_boxes", _p(p2), p2.stride(0), N, P, int(K), int(bool(agnostic)), _p(proposals.contiguous()), _p(counts.contiguous()),
         _p(image_hw.contiguous()), *[float(w) for w in weights], float(scale_clamp), _p(scores), _p(boxes), stream_ptr())
    return scores, boxes


def roi_cascade_stage(pred, K, proposals, counts, image_hw, weights, prev_scores=None, out_scale=1.0, scale_clamp=4.135166556742356, out=None,
                      out_boxes=None):
    """One stage of CascadeROIHeads on the predictor's output pred [N P, Cpad] (K + 1 class logits, 4 class-agnostic deltas): returns (scores
    [N, P, K] = (prev_scores + s) out_scale with s roi_scores_boxes' scores -- one fp32 operation each, the product only when out_scale != 1;
    boxes [N, P, 4] = the clipped decode, the next stage's proposals).  prev_scores None: the first stage.  out: where the scores go; it may be
    prev_scores itself; out_boxes: where the boxes go (afi_roi_cascade_stage)."""
    p2, N, P = _roi_pred_rows("roi_cascade_stage", pred, K, 1, proposals, counts, image_hw)
    for name, t in (("prev_scores", prev_scores), ("out", out)):
        if t is not None:
            _check_cuda(t)
            if tuple(t.shape) != (N, P, K) or not t.is_contiguous():
                raise _lib.AfiError(f"roi_cascade_stage: {name} must be a dense [{N}, {P}, {K}] tensor, got {tuple(t.shape)}")
    if not 0.0 < float(out_scale) < float("inf"):
        raise _lib.AfiError(f"roi_cascade_stage: out_scale {out_scale} must be a positive number")
    scores = out if out is not None else torch.empty((N, P, K), device=pred.device, dtype=torch.float32)
    if out_boxes is not None:
        _check_cuda(out_boxes)
        if tuple(out_boxes.shape) != (N, P, 4) or not out_boxes.is_contiguous():
            raise _lib.AfiError(f"roi_cascade_stage: out_boxes must be a dense [{N}, {P}, 4] tensor, got {tuple(out_boxes.shape)}")
    boxes = out_boxes if out_boxes is not None else torch.empty((N, P, 4), device=pred.device, dtype=torch.float32)
    call("afi_roi_cascade_stage", _p(p2), p2.stride(0), N, P, int(K), _p(proposals.contiguous()), _p(counts.contiguous()), _p(image_hw.contiguous()),
         *[float(w) for w in weights], float(scale_clamp), _p(prev_scores), float(out_scale), _p(scores), _p(boxes), stream_ptr())
    return scores, boxes


def roi_candidates(scores, boxes, score_thresh, M=ROI_MAX_CANDIDATES):
    """The min(M, P K) highest of scores [N, P, K] per image by (score descending, index r K + c ascending), NaN last; boxes [N, P, K or 1, 4].
    Returns a dict: scores / idx / cls / valid [N, M], boxes [N, M, 4], n_over [N] (all scores above score_thresh) (afi_roi_candidates)."""
    _check_cuda(scores, boxes)
    N, P, K = scores.shape
    if boxes.dim() != 4 or boxes.shape[:2] != (N, P) or boxes.shape[2] not in (1, K) or boxes.shape[3] != 4 or not scores.is_contiguous() \
            or not boxes.is_contiguous() or not 0 < M <= ROI_MAX_CANDIDATES:
        raise _lib.AfiError(f"roi_candidates: dense scores [N, P, K] and boxes [N, P, K or 1, 4], 1 <= M <= {ROI_MAX_CANDIDATES} expected, got "
                            f"{tuple(scores.shape)}, {tuple(boxes.shape)}, M {M}")
    # (K == 1: a [N, P, 1, 4] box list reads the same either way)
    agnostic = int(boxes.shape[2] == 1)
    n = _lib.load().afi_roi_candidates_ws_floats(N, P, K)
    if n < 0:
        raise _lib.AfiError(f"roi_candidates: unsupported score list {P} x {K}")
    ws = new_workspace(n, scores.device) if n else None
    dev = scores.device
    r = {"scores": torch.empty((N, M), device=dev, dtype=torch.float32), "idx": torch.empty((N, M), device=dev, dtype=torch.int32),
         "boxes": torch.empty((N, M, 4), device=dev, dtype=torch.float32), "cls": torch.empty((N, M), device=dev, dtype=torch.int32),
         "valid": torch.empty((N, M), device=dev, dtype=torch.int32), "n_over": torch.empty((N,), device=dev, dtype=torch.int32)}
    call("afi_roi_candidates", _p(scores), _p(boxes), N, P, K, agnostic, float(score_thresh), int(M), _p(r["scores"]), _p(r["idx"]), _p(r["boxes"]),
         _p(r["cls"]), _p(r["valid"]), _p(r["n_over"]), _p(ws), n, stream_ptr())
    return r


def roi_nms(boxes, cls, valid, thresh, keep=None):
    """Class-aware greedy NMS of the lists boxes [N, k, 4] (k <= 1024, in score order), cls / valid [N, k] int32: keep [N, k] int32.  The IoU is
    taken on the boxes as they are, not on torchvision's class-offset copies (afi_roi_nms)."""
    _check_cuda(boxes)
    _check_i32(cls, valid)
    N, k = valid.shape
    if keep is None:
        keep = torch.empty((N, k), device=boxes.device, dtype=torch.int32)
    _check_i32(keep)
    if k > RPN_MAX_TOPK:
        raise _lib.AfiError(f"roi_nms: lists of at most {RPN_MAX_TOPK} boxes, got {k}")
    if k == 0:
        return keep
    ld = _rpn_rows(valid, k)
    if _rpn_rows(boxes, k, (4,)) != ld or _rpn_rows(keep, k) != ld or _rpn_rows(cls, k) != ld or not (boxes.shape[0] == keep.shape[0] == cls.shape[0] == N):
        raise _lib.AfiError("roi_nms: boxes, cls, valid and keep must be lists of one row stride")
    call("afi_roi_nms", _p(boxes), _p(cls), _p(valid), N, k, ld, float(thresh), _p(keep), stream_ptr())
    return keep


def roi_pick(cand, keep, D):
    """The first D kept candidates of roi_candidates' dict in list order: (boxes [N, D, 4], scores [N, D], classes [N, D] int32, counts [N],
    truncated [N] = (n_over > M and kept < D)), zero past counts (afi_roi_pick)."""
    _check_i32(keep, cand["cls"], cand["n_over"])
    N, M = cand["scores"].shape
    if tuple(keep.shape) != (N, M) or not keep.is_contiguous() or not 0 < D <= ROI_MAX_CANDIDATES:
        raise _lib.AfiError(f"roi_pick: dense keep [{N}, {M}] and 1 <= D <= {ROI_MAX_CANDIDATES} expected, got {tuple(keep.shape)}, D {D}")
    dev = keep.device
    ob = torch.empty((N, D, 4), device=dev, dtype=torch.float32)
    os_ = torch.empty((N, D), device=dev, dtype=torch.float32)
    oc = torch.empty((N, D), device=dev, dtype=torch.int32)
    counts = torch.empty((N,), device=dev, dtype=torch.int32)
    trunc = torch.empty((N,), device=dev, dtype=torch.int32)
    call("afi_roi_pick", _p(cand["boxes"]), _p(cand["scores"]), _p(cand["cls"]), _p(keep), _p(cand["n_over"]), N, M, int(D), _p(ob), _p(os_), _p(oc),
         _p(counts), _p(trunc), stream_ptr())
    return ob, os_, oc, counts, trunc


# ------------------------------------------------------------------------------------------------ ROI heads, box branch in training (roi_heads.py)
def _roi_train_lists(name, proposals, counts_p, gt, counts_g):
    """Shapes and limits first, then devices and dtypes (as _rpn_gt does); returns (N, P, Gmax)."""
    if proposals.dim() != 3 or proposals.shape[2] != 4 or proposals.shape[1] < 1 or not proposals.is_contiguous() or gt.dim() != 3 \
            or gt.shape[2] != 4 or gt.shape[1] < 1 or gt.shape[0] != proposals.shape[0] or not gt.is_contiguous() \
            or tuple(counts_p.shape) != (gt.shape[0],) or tuple(counts_g.shape) != (gt.shape[0],) or not counts_p.is_contiguous() \
            or not counts_g.is_contiguous():
        raise _lib.AfiError(f"{name}: dense proposals [N, P >= 1, 4], ground truth [N, Gmax >= 1, 4] and two counts [N] expected, got "
                            f"{tuple(proposals.shape)}, {tuple(gt.shape)}, {tuple(counts_p.shape)}, {tuple(counts_g.shape)}")
    if gt.shape[1] > RPN_MAX_GT:
        raise _lib.AfiError(f"{name}: {gt.shape[1]} ground-truth boxes per image; at most {RPN_MAX_GT} are supported")
    if proposals.shape[1] + gt.shape[1] > RPN_MAX_TOTAL_ANCHORS:
        raise _lib.AfiError(f"{name}: {proposals.shape[1] + gt.shape[1]} candidates per image; at most {RPN_MAX_TOTAL_ANCHORS} (2^22) are supported")
    _check_cuda(proposals, gt)
    _check_i32(counts_p, counts_g)
    return proposals.shape[0], proposals.shape[1], gt.shape[1]


def roi_label(proposals, counts_p, gt, counts_g, iou_thresh=0.5, append_gt=True):
    """Proposal labels of detectron2's ROIHeads (Matcher with one threshold and IOU_LABELS [0, 1], no low-quality matches) over the padded
    candidate list of every image: its counts_p proposals, then (append_gt) its counts_g ground-truth boxes.  proposals [N, P, 4], gt
    [N, Gmax, 4] fp32, counts int32.  Returns (labels [N, P + Gmax] int8: 1 / 0 / -1 for padding, matched_idx [N, P + Gmax] int32)
    (afi_roi_label)."""
    N, P, Gmax = _roi_train_lists("roi_label", proposals, counts_p, gt, counts_g)
    labels = torch.empty((N, P + Gmax), device=gt.device, dtype=torch.int8)
    midx = torch.empty((N, P + Gmax), device=gt.device, dtype=torch.int32)
    call("afi_roi_label", _p(proposals), _p(counts_p), N, P, _p(gt), _p(counts_g), Gmax, int(bool(append_gt)), float(iou_thresh), _p(labels),
         _p(midx), stream_ptr())
    return labels, midx


def roi_gather_samples(proposals, counts_p, gt, gt_classes, counts_g, matched_idx, sampled_idx, n_pos, n_neg, K, append_gt=True):
    """The padded training list of rpn_sample's sample of roi_label's candidates: (boxes [N, B, 4], counts [N] = n_pos + n_neg, gt_classes
    [N, B] int32 -- the matched box's class for the n_pos first rows, K (background) for the other sampled rows, -1 past the count --,
    gt_boxes [N, B, 4]: the matched box, zeros when the image has none) (afi_roi_gather_samples)."""
    N, P, Gmax = _roi_train_lists("roi_gather_samples", proposals, counts_p, gt, counts_g)
    _check_i32(gt_classes, matched_idx, sampled_idx, n_pos, n_neg)
    B = sampled_idx.shape[1] if sampled_idx.dim() == 2 else 0
    if tuple(gt_classes.shape) != (N, Gmax) or tuple(matched_idx.shape) != (N, P + Gmax) or tuple(sampled_idx.shape) != (N, B) \
            or tuple(n_pos.shape) != (N,) or tuple(n_neg.shape) != (N,) \
            or not all(t.is_contiguous() for t in (gt_classes, matched_idx, sampled_idx, n_pos, n_neg)):
        raise _lib.AfiError(f"roi_gather_samples: dense gt_classes [{N}, {Gmax}], matched_idx [{N}, {P + Gmax}], sampled_idx [{N}, B], n_pos / "
                            f"n_neg [{N}] expected, got {tuple(gt_classes.shape)}, {tuple(matched_idx.shape)}, {tuple(sampled_idx.shape)}, "
                            f"{tuple(n_pos.shape)}, {tuple(n_neg.shape)}")
    if not 0 < B <= RPN_MAX_BATCH or not 0 < int(K) <= ROI_MAX_CLASSES:
        raise _lib.AfiError(f"roi_gather_samples: batch size per image {B} (1..{RPN_MAX_BATCH}) and K {K} (1..{ROI_MAX_CLASSES}) expected")
    dev = gt.device
    boxes = torch.empty((N, B, 4), device=dev, dtype=torch.float32)
    gboxes = torch.empty((N, B, 4), device=dev, dtype=torch.float32)
    counts = torch.empty((N,), device=dev, dtype=torch.int32)
    cls = torch.empty((N, B), device=dev, dtype=torch.int32)
    call("afi_roi_gather_samples", _p(proposals), _p(counts_p), N, P, _p(gt), _p(gt_classes), _p(counts_g), Gmax, int(bool(append_gt)),
         _p(matched_idx), _p(sampled_idx), _p(n_pos), _p(n_neg), B, int(K), _p(boxes), _p(counts), _p(cls), _p(gboxes), stream_ptr())
    return boxes, counts, cls, gboxes


def roi_box_loss(pred, K, agnostic, boxes, counts, gt_classes, gt_boxes, weights=(10.0, 10.0, 5.0, 5.0), beta=0.0):
    """FastRCNNOutputs' two losses over the padded training list: pred = the predictor's output [N B, >= K + 1 + 4 Kb] with dense rows (K + 1
    logits, background at K, then the deltas), boxes / gt_boxes [N, B, 4], counts [N], gt_classes [N, B] int32.  Returns (loss [2] fp32 on the
    device: cross-entropy and smooth L1, each divided by Rtot = sum(counts); dpred like pred: d loss[0] / d logit and d loss[1] / d delta, every
    other entry zero) (afi_roi_box_loss)."""
    K, Kb = int(K), 1 if agnostic else int(K)
    N, B = boxes.shape[:2] if boxes.dim() == 3 else (0, 0)
    p2 = pred.reshape(pred.shape[0], -1) if pred.dim() == 4 and pred.shape[2:] == (1, 1) and pred.stride(1) == 1 else pred
    if p2.dim() != 2 or p2.shape[0] != N * B or p2.shape[1] < K + 1 + 4 * Kb or p2.stride(1) != 1 or not 0 < K <= ROI_MAX_CLASSES \
            or tuple(boxes.shape) != (N, B, 4) or tuple(gt_boxes.shape) != (N, B, 4) or tuple(counts.shape) != (N,) \
            or tuple(gt_classes.shape) != (N, B) or not all(t.is_contiguous() for t in (boxes, gt_boxes, counts, gt_classes)):
        raise _lib.AfiError(f"roi_box_loss: pred [{N * B}, >= {K + 1 + 4 * Kb}] with dense rows, dense boxes and gt_boxes [N, B, 4], counts [N], "
                            f"gt_classes [N, B] and 1 <= K <= {ROI_MAX_CLASSES} expected, got {tuple(pred.shape)}, {tuple(boxes.shape)}, "
                            f"{tuple(gt_boxes.shape)}, {tuple(counts.shape)}, {tuple(gt_classes.shape)}, K {K}")
    if not 0 < B <= RPN_MAX_BATCH or len(weights) != 4 or min(weights) <= 0 or not beta >= 0:
        raise _lib.AfiError(f"roi_box_loss: batch size per image {B} (1..{RPN_MAX_BATCH}), four positive weights and beta >= 0 expected")
    _check_cuda(pred, boxes, gt_boxes)
    _check_i32(counts, gt_classes)
    ld = p2.stride(0)
    dpred = new_workspace(N * B * ld, pred.device).view(N * B, ld)
    loss = torch.empty((2,), device=pred.device, dtype=torch.float32)
    nws = int(_lib.load().afi_roi_box_loss_ws_floats())
    ws = new_workspace(nws, pred.device)
    call("afi_roi_box_loss", _p(p2), ld, N, B, K, int(bool(agnostic)), _p(boxes), _p(counts), _p(gt_classes), _p(gt_boxes),
         *[float(w) for w in weights], float(beta), _p(loss), _p(dpred), _p(ws), nws, stream_ptr())
    return loss, dpred[:, :p2.shape[1]]


def roi_align_bwd(dpooled, level_shapes, min_level, boxes, counts, sampling_ratio=0):
    """The backward of roi_align: dpooled = dense pixel-major [N B, C, S, S], level_shapes = [(H_l, W_l), ...], boxes [N, B, 4] with counts [N]
    int32.  Returns one dense pixel-major gradient [N, C, H_l, W_l] per level, every element written (zero where no box reaches)
    (afi_roi_align_bwd: one block per 8 x 8 tile of a level, no atomics)."""
    L = len(level_shapes)
    if not 0 < L <= RPN_MAX_LEVELS or any(int(h) <= 0 or int(w) <= 0 for h, w in level_shapes):
        raise _lib.AfiError(f"roi_align_bwd: 1..{RPN_MAX_LEVELS} levels of positive size, got {list(level_shapes)}")
    N, B = boxes.shape[:2] if boxes.dim() == 3 else (0, 0)
    if boxes.dim() != 3 or boxes.shape[2] != 4 or B < 1 or not boxes.is_contiguous() or tuple(counts.shape) != (N,) or not counts.is_contiguous():
        raise _lib.AfiError(f"roi_align_bwd: dense boxes [N, B, 4] and counts [N] expected, got {tuple(boxes.shape)} and {tuple(counts.shape)}")
    if dpooled.dim() != 4 or dpooled.shape[0] != N * B or dpooled.shape[2] != dpooled.shape[3] or not is_dense_pm(dpooled) or dpooled.shape[1] % 4:
        raise _lib.AfiError(f"roi_align_bwd: a dense pixel-major [{N * B}, C % 4 == 0, S, S] gradient expected, got {tuple(dpooled.shape)}")
    C_, S = dpooled.shape[1:3]
    if not 0 < S <= ROI_MAX_POOLED or sampling_ratio < 0:
        raise _lib.AfiError(f"roi_align_bwd: pooled size {S} (1..{ROI_MAX_POOLED}), sampling_ratio {sampling_ratio} (>= 0)")
    _check_cuda(dpooled, boxes)
    _check_i32(counts)
    grads = [new_pixel_major(N, C_, int(h), int(w), boxes.device) for h, w in level_shapes]
    views = (View * L)(*[view_of(g) for g in grads])
    hw = (C.c_int * (2 * L))(*[int(s) for p in level_shapes for s in p])
    nws = int(_lib.load().afi_roi_align_bwd_ws_floats(N, B))
    ws = new_workspace(nws, boxes.device)
    call("afi_roi_align_bwd", _p(dpooled), views, hw, L, int(min_level), N, C_, _p(boxes), _p(counts), B, int(S), int(sampling_ratio), _p(ws), nws,
         stream_ptr())
    return grads


# ------------------------------------------------------------------------------------------------ ROI heads, mask branch (roi_heads.py)
MASK_MAX_SIDE = 64                          # M: the mask afi_mask_paste holds in LDS


def roi_mask_probs(h, w, bias, classes, counts, out=None):
    """The class-selected mask predictor and sigmoid on the deconv's 4-phase output: h pixel-major [N D, 4 C, S, S] dense (memory
    [R][S][S][4][C], phase 2a + b of input pixel (y, x) = output pixel (2y + a, 2x + b)), w [Km, C] (or [Km, C, 1, 1]), bias [Km], classes
    [N, D] int32, counts [N] int32; returns probs [N D, 2S, 2S], rows past counts (and rows with a class outside 0..Km-1) zero
    (afi_roi_mask_probs)."""
    _check_cuda(h, w, bias, out)
    _check_i32(classes, counts)
    if classes.dim() != 2 or counts.dim() != 1 or counts.shape[0] != classes.shape[0] or not classes.is_contiguous() or not counts.is_contiguous():
        raise _lib.AfiError(f"roi_mask_probs: dense classes [N, D] and counts [N] expected, got {tuple(classes.shape)} and {tuple(counts.shape)}")
    N, D = classes.shape
    Km = w.shape[0]
    w2 = w.reshape(Km, -1).contiguous()
    C_ = w2.shape[1]
    if h.dim() != 4 or h.shape[0] != N * D or h.shape[1] != 4 * C_ or h.shape[2] != h.shape[3] or not is_dense_pm(h) or C_ % 4 \
            or tuple(bias.shape) != (Km,) or not bias.is_contiguous():
        raise _lib.AfiError(f"roi_mask_probs: a dense pixel-major h [{N * D}, 4 C, S, S] with C = {C_} (a multiple of 4) and a bias [{Km}] "
                            f"expected, got {tuple(h.shape)} and {tuple(bias.shape)}")
    S = h.shape[2]
    if not 0 < S <= ROI_MAX_POOLED:
        raise _lib.AfiError(f"roi_mask_probs: pooled size {S} (1..{ROI_MAX_POOLED})")
    if out is None:
        out = torch.empty((N * D, 2 * S, 2 * S), device=h.device, dtype=torch.float32)
    elif tuple(out.shape) != (N * D, 2 * S, 2 * S) or not out.is_contiguous():
        raise _lib.AfiError(f"roi_mask_probs: out must be a dense [{N * D}, {2 * S}, {2 * S}] tensor")
    call("afi_roi_mask_probs", _p(h), _p(w2), _p(bias), _p(classes), _p(counts), N, D, C_, S, Km, _p(out), stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ ROI heads, mask branch in training (roi_heads.py)
def mask_polygons(instances, N, Gmax, device):
    """The polygons of a training call as afi_mask_targets reads them: ``instances[n]`` = image n's list of instances, each a list of flat
    coordinate sequences; one annotation per (image, ground-truth slot), the slots past an image's instances empty.  Checked on the host
    (polygons_batch), uploaded once: (xy float64 [V, 2], vert_off int64 [P + 1], poly_off int64 [N Gmax + 1]) on the device."""
    anns = []
    for n in range(N):
        inst = list(instances[n])
        if len(inst) > Gmax:
            raise _lib.AfiError(f"mask_polygons: image {n} has {len(inst)} instances for {Gmax} ground-truth slots")
        anns.extend(inst + [[]] * (Gmax - len(inst)))
    xy, vert_off, poly_off, _, _ = polygons_batch(anns, (1, 1))
    up = lambda a: torch.from_numpy(a if a.size else np.zeros((1,) + a.shape[1:], a.dtype)).to(device)      # noqa: E731  (no null pointer)
    return up(xy), torch.from_numpy(vert_off).to(device), torch.from_numpy(poly_off).to(device)


def mask_targets(xy, vert_off, poly_off, boxes, sampled_idx, matched_idx, counts_g, Gmax, n_pos, Bf, M, out=None):
    """detectron2's mask targets of the foreground prefix of a training list (PolygonMasks.crop_and_resize restated): xy / vert_off / poly_off
    = mask_polygons' tensors, boxes [N, B, 4] / sampled_idx [N, B] / matched_idx [N, P + Gmax] / n_pos [N] = the box branch's training list
    (roi_gather_samples' inputs and output), counts_g [N].  Returns (targets uint8 [N, Bf, M, M], every byte written, rows past the count
    zero; counts_fg [N] int32 = n_pos clamped to 0..Bf) (afi_mask_targets)."""
    N, B = boxes.shape[:2] if boxes.dim() == 3 else (0, 0)
    Bf, M, Gmax = int(Bf), int(M), int(Gmax)
    if boxes.dim() != 3 or boxes.shape[2] != 4 or not boxes.is_contiguous() or tuple(sampled_idx.shape) != (N, B) or matched_idx.dim() != 2 \
            or matched_idx.shape[0] != N or tuple(counts_g.shape) != (N,) or tuple(n_pos.shape) != (N,) \
            or not all(t.is_contiguous() for t in (sampled_idx, matched_idx, counts_g, n_pos)):
        raise _lib.AfiError(f"mask_targets: dense boxes [N, B, 4], sampled_idx [N, B], matched_idx [N, R], counts_g [N] and n_pos [N] expected, got "
                            f"{tuple(boxes.shape)}, {tuple(sampled_idx.shape)}, {tuple(matched_idx.shape)}, {tuple(counts_g.shape)}, {tuple(n_pos.shape)}")
    if not 0 < Bf <= B or not 0 < B <= RPN_MAX_BATCH or not 0 < M <= 2 * ROI_MAX_POOLED or Gmax < 1:
        raise _lib.AfiError(f"mask_targets: Bf {Bf} (1..B = {B} <= {RPN_MAX_BATCH}), M {M} (1..{2 * ROI_MAX_POOLED}) and Gmax {Gmax} (>= 1) expected")
    _check_cuda(boxes)
    _check_i32(sampled_idx, matched_idx, counts_g, n_pos)
    for name, t, dt in (("xy", xy, torch.float64), ("vert_off", vert_off, torch.int64), ("poly_off", poly_off, torch.int64)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise _lib.AfiError(f"mask_targets: {name} must be a dense {dt} tensor on the GPU (ops.mask_polygons)")
    if poly_off.numel() != N * Gmax + 1 or vert_off.numel() < 1 or xy.dim() != 2 or xy.shape[1] != 2:
        raise _lib.AfiError(f"mask_targets: poly_off must hold {N} x {Gmax} + 1 offsets (one annotation per image and ground-truth slot), "
                            f"got {poly_off.numel()}; xy [V, 2], got {tuple(xy.shape)}")
    if out is None:
        out = torch.empty((N, Bf, M, M), device=boxes.device, dtype=torch.uint8)
    elif tuple(out.shape) != (N, Bf, M, M) or out.dtype != torch.uint8 or not out.is_contiguous() or not out.is_cuda:
        raise _lib.AfiError(f"mask_targets: out must be a dense uint8 [{N}, {Bf}, {M}, {M}] tensor on the GPU")
    counts_fg = torch.empty((N,), device=boxes.device, dtype=torch.int32)
    call("afi_mask_targets", _p(xy), _p(vert_off), _p(poly_off), vert_off.numel() - 1, xy.shape[0], _p(boxes), _p(sampled_idx), N, B,
         _p(matched_idx), matched_idx.shape[1], _p(counts_g), Gmax, _p(n_pos), Bf, M, _p(out), _p(counts_fg), stream_ptr())
    return out, counts_fg


def _mask_loss_rows(name, h, w, classes, counts_fg):
    """The shapes shared by mask_loss and mask_pred_bwd: returns (N, D, C, S, Km, w as [Km, C])."""
    _check_i32(classes, counts_fg)
    if classes.dim() != 2 or counts_fg.dim() != 1 or counts_fg.shape[0] != classes.shape[0] or classes.stride(1) != 1 or not counts_fg.is_contiguous():
        raise _lib.AfiError(f"{name}: classes [N, D] with dense rows and counts_fg [N] expected, got {tuple(classes.shape)} and {tuple(counts_fg.shape)}")
    N, D = classes.shape
    Km = w.shape[0]
    w2 = w.reshape(Km, -1).contiguous()
    C_ = w2.shape[1]
    if h.dim() != 4 or h.shape[0] != N * D or h.shape[1] != 4 * C_ or h.shape[2] != h.shape[3] or not is_dense_pm(h) or C_ % 4 \
            or not 0 < h.shape[2] <= ROI_MAX_POOLED:
        raise _lib.AfiError(f"{name}: a dense pixel-major h [{N * D}, 4 C, S, S] with C = {C_} (a multiple of 4) and S in 1..{ROI_MAX_POOLED} "
                            f"expected, got {tuple(h.shape)}")
    return N, D, C_, h.shape[2], Km, w2


def mask_loss(h, w, bias, classes, counts_fg, targets):
    """mask_rcnn_loss on the deconv's 4-phase output: h as in roi_mask_probs with D = Bf rows per image, classes [N, Bf] int32 (a view of the
    training list's [N, B] classes will do), counts_fg [N], targets uint8 [N, Bf, 2S, 2S].  Returns (loss [1] fp32 on the device = the mean
    binary cross-entropy with logits over the counts_fg rows' selected-class pixels, dz [N Bf, S, S, 4] = d loss / d logit in h's pixel order,
    zero on the other rows) (afi_mask_loss)."""
    _check_cuda(h, w, bias)
    N, D, C_, S, Km, w2 = _mask_loss_rows("mask_loss", h, w, classes, counts_fg)
    if tuple(bias.shape) != (Km,) or not bias.is_contiguous() or tuple(targets.shape) != (N, D, 2 * S, 2 * S) or targets.dtype != torch.uint8 \
            or not targets.is_contiguous() or not targets.is_cuda:
        raise _lib.AfiError(f"mask_loss: a bias [{Km}] and dense uint8 targets [{N}, {D}, {2 * S}, {2 * S}] on the GPU expected, got "
                            f"{tuple(bias.shape)} and {targets.dtype} {tuple(targets.shape)}")
    loss = torch.empty((1,), device=h.device, dtype=torch.float32)
    dz = new_workspace(N * D * 4 * S * S, h.device).view(N * D, S, S, 4)
    nws = int(_lib.load().afi_mask_loss_ws_floats(N, D, C_, S))
    ws = new_workspace(max(nws, 2), h.device)
    call("afi_mask_loss", _p(h), _p(w2), _p(bias), _p(classes), classes.stride(0), _p(counts_fg), _p(targets), N, D, C_, S, Km, _p(loss), _p(dz),
         _p(ws), nws, stream_ptr())
    return loss, dz


def mask_pred_bwd(h, dz, w, classes, counts_fg):
    """The backward of the class-selected mask predictor: h, w, classes, counts_fg as in mask_loss, dz [N Bf, S, S, 4] (mask_loss', possibly
    scaled).  Returns (dh like h = dz w[class] (h > 0), zero on rows past the count; dW [Km, C]; db [Km]) (afi_mask_pred_bwd)."""
    _check_cuda(h, w, dz)
    N, D, C_, S, Km, w2 = _mask_loss_rows("mask_pred_bwd", h, w, classes, counts_fg)
    if tuple(dz.shape) != (N * D, S, S, 4) or not dz.is_contiguous():
        raise _lib.AfiError(f"mask_pred_bwd: a dense dz [{N * D}, {S}, {S}, 4] expected, got {tuple(dz.shape)}")
    nws = int(_lib.load().afi_mask_pred_bwd_ws_floats(N, D, C_))
    if nws < 0 or N * D > 65535:
        raise _lib.AfiError(f"mask_pred_bwd: unsupported shape (C {C_} <= 1024 and N Bf {N * D} <= 65535 expected)")
    dh = new_pixel_major(N * D, 4 * C_, S, S, h.device)
    dW = torch.empty((Km, C_), device=h.device, dtype=torch.float32)
    db = torch.empty((Km,), device=h.device, dtype=torch.float32)
    ws = new_workspace(nws, h.device)
    call("afi_mask_pred_bwd", _p(h), _p(dz), _p(w2), _p(classes), classes.stride(0), _p(counts_fg), N, D, C_, S, Km, _p(dh), _p(dW), _p(db),
         _p(ws), nws, stream_ptr())
    return dh, dW, db


def mask_paste(probs, boxes, hw, threshold=0.5, out=None):
    """detectron2's paste_masks_in_image: probs [R, M, M] pasted into boxes [R, 4] (x0, y0, x1, y1) of an image of hw = (H, W), compared with
    ``>= threshold``: bool [R, H, W].  Pixels whose centre is outside their box are False; a box with a non-positive side gives all False
    (afi_mask_paste).  out: a uint8 or bool [R, H, W] buffer."""
    _check_cuda(probs, boxes)
    H, W = int(hw[0]), int(hw[1])
    if probs.dim() != 3 or probs.shape[1] != probs.shape[2] or tuple(boxes.shape) != (probs.shape[0], 4) or H <= 0 or W <= 0:
        raise _lib.AfiError(f"mask_paste: probs [R, M, M], boxes [R, 4] and a positive output size expected, got {tuple(probs.shape)}, "
                            f"{tuple(boxes.shape)}, {(H, W)}")
    R, M = probs.shape[:2]
    if not 0 < M <= MASK_MAX_SIDE:
        raise _lib.AfiError(f"mask_paste: mask side {M} (1..{MASK_MAX_SIDE})")
    if out is None:
        out = torch.empty((R, H, W), device=probs.device, dtype=torch.uint8)
    elif not out.is_cuda or out.dtype not in (torch.uint8, torch.bool) or tuple(out.shape) != (R, H, W) or not out.is_contiguous():
        raise _lib.AfiError(f"mask_paste: out must be a dense uint8 / bool [{R}, {H}, {W}] tensor on the GPU")
    if R:
        call("afi_mask_paste", _p(probs.contiguous()), _p(boxes.contiguous()), R, M, H, W, float(threshold), _p(out), stream_ptr())
    return out.view(torch.bool)


def mask_paste_rle(probs, boxes, hw, threshold=0.5, ws=None):
    """mask_paste's masks as COCO run-length starts, without the image-size masks: (starts int32 [T] on the GPU, detection after detection,
    ascending; nstarts int64 [R] on the CPU).  A mask is read column-major (j = x H + y) and a start is a j whose pixel differs from pixel
    j - 1; rle.counts_from_starts turns them into counts.  The pixels are mask_paste's, bit for bit; a box with a non-finite coordinate gives
    an empty mask.  Count, ONE host read of the R counts, their running sum, emit (afi_mask_rle_count, afi_mask_rle_emit).  ws: a dense GPU
    buffer of at least afi_mask_rle_ws_bytes(R, H, W) bytes to use instead of a fresh workspace."""
    _check_cuda(probs, boxes)
    H, W = int(hw[0]), int(hw[1])
    if probs.dim() != 3 or probs.shape[1] != probs.shape[2] or tuple(boxes.shape) != (probs.shape[0], 4) or H <= 0 or W <= 0:
        raise _lib.AfiError(f"mask_paste_rle: probs [R, M, M], boxes [R, 4] and a positive output size expected, got {tuple(probs.shape)}, "
                            f"{tuple(boxes.shape)}, {(H, W)}")
    R, M = probs.shape[:2]
    if not 0 < M <= MASK_MAX_SIDE:
        raise _lib.AfiError(f"mask_paste_rle: mask side {M} (1..{MASK_MAX_SIDE})")
    dev = probs.device
    if R == 0:
        return torch.empty((0,), device=dev, dtype=torch.int32), torch.zeros((0,), dtype=torch.int64)
    n = _lib.load().afi_mask_rle_ws_bytes(R, H, W)
    if n < 0:
        raise _lib.AfiError(f"mask_paste_rle: unsupported output size {H} x {W} (H W < 2^31)")
    if ws is None:
        ws = new_workspace((n + 3) // 4, dev)
    elif not ws.is_cuda or not ws.is_contiguous() or ws.numel() * ws.element_size() < n:
        raise _lib.AfiError(f"mask_paste_rle: ws must be a dense GPU buffer of at least {n} bytes")
    wsb = ws.numel() * ws.element_size()
    boxes = boxes.contiguous()
    nst = torch.empty((R,), device=dev, dtype=torch.int32)
    call("afi_mask_rle_count", _p(probs.contiguous()), _p(boxes), R, M, H, W, float(threshold), _p(ws), wsb, _p(nst), stream_ptr())
    nstarts = nst.cpu().to(torch.int64)                     # the one host read
    ends = torch.cumsum(nstarts, 0)
    total = int(ends[-1])
    starts = torch.empty((total,), device=dev, dtype=torch.int32)
    if total:
        offsets = (ends - nstarts).to(dev)
        call("afi_mask_rle_emit", _p(boxes), R, H, W, _p(ws), wsb, _p(offsets), _p(starts), stream_ptr())
    return starts, nstarts


# ------------------------------------------------------------------------------------------------ COCO evaluation (coco_eval.py)
def _coco_arg(name, t, dtype, numel=None):
    """A dense GPU tensor of `dtype` (and, when given, of `numel` elements); an empty one becomes one zero element, so that no pointer is null."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.AfiError(f"coco: `{name}` must be a GPU tensor (the evaluation kernels run on the GPU only; there is no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise _lib.AfiError(f"coco: `{name}` must be a dense {dtype} tensor" + (f" of {numel} elements" if numel is not None else "")
                            + f", got {t.dtype} {tuple(t.shape)}")
    return t if t.numel() else torch.zeros((1,), device=t.device, dtype=dtype)


def _coco_groups(dt_off, gt_off, iou_off):
    ng = dt_off.numel() - 1
    if ng < 0:
        raise _lib.AfiError("coco: offsets of ngroups + 1 elements expected, got an empty tensor")
    return ng, [_coco_arg(n, t, torch.int64, ng + 1) for n, t in (("dt_off", dt_off), ("gt_off", gt_off), ("iou_off", iou_off))]


def coco_box_iou(dt, gt, iscrowd, dt_off, gt_off, iou_off, total):
    """The packed IoU matrices [total] (fp64) of every (image, category) group: dt [total_d, 4], gt [total_g, 4] xywh fp64, iscrowd [total_g] uint8,
    dt_off / gt_off / iou_off [ngroups + 1] int64 on the GPU, total = iou_off[-1] (known to the caller) (afi_coco_box_iou)."""
    ng, offs = _coco_groups(dt_off, gt_off, iou_off)
    if dt.dim() != 2 or dt.shape[1] != 4 or gt.dim() != 2 or gt.shape[1] != 4:
        raise _lib.AfiError(f"coco_box_iou: boxes [n, 4] expected, got {tuple(dt.shape)} and {tuple(gt.shape)}")
    out = torch.empty((int(total),), device=dt.device, dtype=torch.float64)
    call("afi_coco_box_iou", _p(_coco_arg("dt", dt, torch.float64)), _p(_coco_arg("gt", gt, torch.float64)),
         _p(_coco_arg("iscrowd", iscrowd, torch.uint8, gt.shape[0])), _p(offs[0]), _p(offs[1]), _p(offs[2]), ng, int(total), _p(_coco_arg("iou", out, torch.float64)),
         stream_ptr())
    return out


def coco_rle_area(starts, start_off, hw):
    """The set pixels (int64 [nmask]) of masks given as ascending run starts: starts int32 [S], start_off int64 [nmask + 1], hw int32 [nmask] = H W
    of every mask (afi_coco_rle_area)."""
    nmask = hw.numel()
    out = torch.empty((nmask,), device=hw.device, dtype=torch.int64)
    if nmask:
        call("afi_coco_rle_area", _p(_coco_arg("starts", starts, torch.int32)), _p(_coco_arg("start_off", start_off, torch.int64, nmask + 1)),
             _p(_coco_arg("hw", hw, torch.int32)), nmask, _p(out), stream_ptr())
    return out


def coco_rle_iou(dt, gt, iscrowd, dt_off, gt_off, iou_off, total, want_inter=False):
    """The packed mask IoU matrices [total] (fp64; with want_inter also the intersections, int64): dt and gt are (starts, start_off, hw, area) with
    area = coco_rle_area's; a pair of masks with different H W gives -1 (afi_coco_rle_iou)."""
    ng, offs = _coco_groups(dt_off, gt_off, iou_off)
    args = []
    for side, (starts, soff, hw, area) in (("dt", dt), ("gt", gt)):
        n = hw.numel()
        args += [_p(_coco_arg(f"{side} starts", starts, torch.int32)), _p(_coco_arg(f"{side} start_off", soff, torch.int64, n + 1)),
                 _p(_coco_arg(f"{side} hw", hw, torch.int32)), _p(_coco_arg(f"{side} area", area, torch.int64, n))]
    dev = dt[2].device
    out = torch.empty((int(total),), device=dev, dtype=torch.float64)
    inter = torch.empty((int(total),), device=dev, dtype=torch.int64) if want_inter else None
    call("afi_coco_rle_iou", *args, _p(_coco_arg("iscrowd", iscrowd, torch.uint8, gt[2].numel())), _p(offs[0]), _p(offs[1]), _p(offs[2]), ng, int(total),
         _p(_coco_arg("inter", inter, torch.int64)) if want_inter else _p(None), _p(_coco_arg("iou", out, torch.float64)), stream_ptr())
    return (out, inter) if want_inter else out


def coco_match(iou, dt_off, gt_off, iou_off, dt_area, gt_area, iscrowd, area_rng, iou_thr, max_g=None, ws=None):
    """pycocotools' greedy matching of every group for A area ranges (area_rng [A, 2] fp64) x T thresholds (iou_thr [T] fp64): (dt_match int32
    [A, T, total_d] = the matched GT's index inside its group or -1, dt_ignore uint8 [A, T, total_d], gt_ignore uint8 [A, total_g]).  dt_area
    [total_d], gt_area [total_g] fp64, iscrowd [total_g] uint8.  max_g: an upper bound on the GTs of any group, when the caller knows one
    (None: total_g); the kernel for groups of more than 64 GTs is launched only if it exceeds 64.  ws: a dense GPU buffer of at least afi_coco_match_ws_bytes(total_g, A, T) bytes
    to use instead of a fresh workspace (afi_coco_match)."""
    ng, offs = _coco_groups(dt_off, gt_off, iou_off)
    if area_rng.dim() != 2 or area_rng.shape[1] != 2 or iou_thr.dim() != 1 or not area_rng.shape[0] or not iou_thr.shape[0]:
        raise _lib.AfiError(f"coco_match: area_rng [A, 2] and iou_thr [T] expected, got {tuple(area_rng.shape)} and {tuple(iou_thr.shape)}")
    A, T, nd, ngt, dev = area_rng.shape[0], iou_thr.shape[0], dt_area.numel(), gt_area.numel(), dt_area.device
    n = _lib.load().afi_coco_match_ws_bytes(ngt, A, T)
    if n < 0:
        raise _lib.AfiError(f"coco_match: {A} area ranges x {T} thresholds are not supported (A T <= 4096)")
    if ws is None:
        ws = new_workspace((n + 3) // 4 + 1, dev)
    elif not ws.is_cuda or not ws.is_contiguous() or ws.numel() * ws.element_size() < n:
        raise _lib.AfiError(f"coco_match: ws must be a dense GPU buffer of at least {n} bytes")
    dtm = torch.empty((A, T, nd), device=dev, dtype=torch.int32)
    dti = torch.empty((A, T, nd), device=dev, dtype=torch.uint8)
    gti = torch.empty((A, ngt), device=dev, dtype=torch.uint8)
    call("afi_coco_match", _p(_coco_arg("iou", iou, torch.float64)), _p(offs[0]), _p(offs[1]), _p(offs[2]), ng,
         _p(_coco_arg("dt_area", dt_area, torch.float64)), _p(_coco_arg("gt_area", gt_area, torch.float64)),
         _p(_coco_arg("iscrowd", iscrowd, torch.uint8, ngt)), nd, ngt, _p(_coco_arg("area_rng", area_rng, torch.float64)), A,
         _p(_coco_arg("iou_thr", iou_thr, torch.float64)), T, ngt if max_g is None else int(max_g), _p(_coco_arg("dt_match", dtm, torch.int32)), _p(_coco_arg("dt_ignore", dti, torch.uint8)),
         _p(_coco_arg("gt_ignore", gti, torch.uint8)), _p(ws), ws.numel() * ws.element_size(), stream_ptr())
    return dtm, dti, gti


# ------------------------------------------------------------------------------------------------ COCO polygons as run starts (rle.py, coco_eval.py)
def polygons_batch(polygons, sizes):
    """The host side of polygons_rle: checks the annotations (AfiError before anything is uploaded) and packs them as afi_poly_rle_count reads
    them.  Returns numpy arrays (xy float64 [V, 2], vert_off int64 [P + 1], poly_off int64 [N + 1], hw int32 [N, 2], cap_off int64 [P + 1])."""
    N = len(polygons)
    sz = np.asarray(sizes, dtype=np.int64)
    if sz.ndim == 1 and sz.size == 2:
        sz = np.broadcast_to(sz, (N, 2))
    if sz.ndim != 2 or sz.shape != (N, 2):
        raise _lib.AfiError(f"polygons_rle: sizes must be (H, W) or one pair per annotation, got shape {tuple(np.shape(sizes))} for {N} annotations")
    if N and ((sz <= 0).any() or (sz[:, 0] * sz[:, 1] >= 1 << 31).any()):
        raise _lib.AfiError("polygons_rle: every canvas needs H, W > 0 and H W < 2^31")
    flat, nvert, npoly = [], [], []
    for i, ann in enumerate(polygons):
        if isinstance(ann, dict) or isinstance(ann, (str, bytes)):
            raise _lib.AfiError(f"polygons_rle: annotation {i} is not a list of polygons (an RLE is not rasterised)")
        npoly.append(len(ann))
        for poly in ann:
            c = np.asarray(poly, dtype=np.float64).reshape(-1)
            if c.size == 0 or c.size & 1:
                raise _lib.AfiError(f"polygons_rle: annotation {i}: a polygon of {c.size} coordinates (a non-empty list of x, y pairs expected)")
            flat.append(c)
            nvert.append(c.size // 2)
    xy = np.concatenate(flat).reshape(-1, 2) if flat else np.zeros((0, 2), np.float64)
    if not np.isfinite(xy).all():
        raise _lib.AfiError("polygons_rle: a non-finite coordinate")
    if (np.abs(5 * xy + .5) >= float(1 << 30)).any():
        raise _lib.AfiError("polygons_rle: a coordinate c with |5 c + .5| >= 2^30")
    vert_off = np.concatenate(([0], np.cumsum(nvert))).astype(np.int64)
    poly_off = np.concatenate(([0], np.cumsum(npoly))).astype(np.int64)
    # the capacity of a polygon: sum over its edges of (dx / 5 + 2), dx in upsampled units (the kernel's X = (int)(5 x + .5), same fp64 steps)
    X = np.trunc(5 * xy[:, 0] + .5).astype(np.int64)
    nxt = np.arange(1, X.size + 1, dtype=np.int64)
    if X.size:
        nxt[vert_off[1:] - 1] = vert_off[:-1]                                   # the last vertex of a polygon is followed by its first
    cap_edge = np.abs(X[nxt] - X) // 5 + 2 if X.size else np.zeros(0, np.int64)
    cap_off = np.concatenate(([0], np.cumsum(cap_edge)))[vert_off].astype(np.int64)
    if int(cap_off[-1]) >= 1 << 31:
        raise _lib.AfiError(f"polygons_rle: {int(cap_off[-1])} crossings at most in one call (< 2^31): split the batch")
    return xy, vert_off, poly_off, np.ascontiguousarray(sz, dtype=np.int32), cap_off


def polygons_rle(polygons, sizes, device="cuda", ws=None):
    """COCO polygon annotations as run starts (pycocotools' frPyObjects + merge): ``polygons`` a list of N annotations, each a list of flat
    coordinate sequences [x0, y0, x1, y1, ...]; ``sizes`` (H, W) or one pair per annotation.  Returns (starts int32 [S], start_off int64 [N + 1],
    hw int32 [N] = H W) on the GPU: the (starts, start_off, hw) of coco_rle_area / coco_rle_iou.  An annotation without a polygon, or whose
    polygons cover no pixel centre column, is an empty mask.  Count, ONE host read of the N counts, their running sum, emit (afi_poly_rle_count,
    afi_poly_rle_emit).  ws: a dense GPU buffer to use instead of a fresh workspace."""
    xy, vert_off, poly_off, hw2, cap_off = polygons_batch(polygons, sizes)
    N, cap_total = len(polygons), int(cap_off[-1])
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.AfiError("polygons_rle: the rasteriser runs on the GPU only; there is no CPU fallback")
    hw = torch.from_numpy(hw2[:, 0] * hw2[:, 1]).to(dev)
    if N == 0:
        return torch.empty((0,), device=dev, dtype=torch.int32), torch.zeros((1,), device=dev, dtype=torch.int64), hw
    n = _lib.load().afi_poly_rle_ws_bytes(cap_total)
    if n < 0:
        raise _lib.AfiError(f"polygons_rle: unsupported capacity {cap_total}")
    if ws is None:
        ws = new_workspace((n + 3) // 4 + 2, dev)
    elif not ws.is_cuda or not ws.is_contiguous() or ws.numel() * ws.element_size() < n or ws.data_ptr() % 8:
        raise _lib.AfiError(f"polygons_rle: ws must be a dense, 8-byte aligned GPU buffer of at least {n} bytes")
    wsb = ws.numel() * ws.element_size()
    up = lambda a: torch.from_numpy(a if a.size else np.zeros((1,) + a.shape[1:], a.dtype)).to(dev)      # noqa: E731  (no null pointer)
    d_xy, d_voff, d_poff, d_hw2, d_cap = up(xy), up(vert_off), up(poly_off), up(hw2), up(cap_off)
    nst = torch.empty((N,), device=dev, dtype=torch.int32)
    call("afi_poly_rle_count", _p(d_xy), _p(d_voff), _p(d_poff), _p(d_hw2), _p(d_cap), N, cap_total, _p(ws), wsb, _p(nst), stream_ptr())
    nstarts = nst.cpu().to(torch.int64)                     # the one host read
    if bool((nstarts < 0).any()):
        raise _lib.AfiError("polygons_rle: a mask's crossings exceeded its capacity bound (internal error: the bound is sum of dx / 5 + 2 per edge)")
    start_off = torch.cat((torch.zeros((1,), dtype=torch.int64), torch.cumsum(nstarts, 0)))
    total = int(start_off[-1])
    starts = torch.empty((total,), device=dev, dtype=torch.int32)
    start_off = start_off.to(dev)
    if total:
        call("afi_poly_rle_emit", _p(d_poff), _p(d_cap), N, cap_total, _p(ws), wsb, _p(start_off), _p(starts), stream_ptr())
    return starts, start_off, hw


def rle_decode(starts, start_off, hw, out=None):
    """The bool [N, H, W] masks of N run-start lists on one common canvas ``hw`` = (H, W): starts int32 [S], start_off int64 [N + 1] on the GPU
    (polygons_rle's, mask_paste_rle's after a running sum); pixel (y, x) is set iff the number of starts <= x H + y is odd (afi_rle_decode)."""
    H, W = int(hw[0]), int(hw[1])
    if H <= 0 or W <= 0 or H * W >= 1 << 31:
        raise _lib.AfiError(f"rle_decode: a canvas with H, W > 0 and H W < 2^31 expected, got {(H, W)}")
    N = start_off.numel() - 1
    if N < 0:
        raise _lib.AfiError("rle_decode: start_off of N + 1 elements expected, got an empty tensor")
    so = _coco_arg("start_off", start_off, torch.int64)
    st = _coco_arg("starts", starts, torch.int32)
    if out is None:
        out = torch.empty((N, H, W), device=so.device, dtype=torch.uint8)
    elif not out.is_cuda or out.dtype not in (torch.uint8, torch.bool) or tuple(out.shape) != (N, H, W) or not out.is_contiguous():
        raise _lib.AfiError(f"rle_decode: out must be a dense uint8 / bool [{N}, {H}, {W}] tensor on the GPU")
    if N:
        call("afi_rle_decode", _p(st), _p(so), N, H, W, _p(out), stream_ptr())
    return out.view(torch.bool)


# ------------------------------------------------------------------------------------------------ bandwidth ops
def bilinear2x(x, out=None, beta=0.0):
    N, C_, H, W = x.shape
    if out is None:
        out = new_pixel_major(N, C_, 2 * H, 2 * W, x.device)
    assert is_dense_pm(out)
    call("afi_bilinear2x_add_fwd", view_of(x), N, H, W, C_, float(beta), _p(out), stream_ptr())
    return out


def bilinear2x_bwd(dout, dx=None, beta=0.0):
    N, C_, H2, W2 = dout.shape
    assert is_dense_pm(dout)
    if dx is None:
        dx = new_pixel_major(N, C_, H2 // 2, W2 // 2, dout.device)
    call("afi_bilinear2x_add_bwd", _p(dout), N, H2 // 2, W2 // 2, C_, float(beta), _p(dx), stream_ptr())
    return dx


def reduce_scratch(C_, device):
    return new_workspace(_lib.load().afi_reduce_scratch_floats(C_), device)


def bn_stats(x2d, running_mean=None, running_var=None):
    """x2d: dense [P, C].  Returns (mean, invstd, var_biased)."""
    P, C_ = x2d.shape
    mean, invstd, var = (torch.empty(C_, device=x2d.device) for _ in range(3))
    call("afi_bn_stats", _p(x2d), P, C_, _p(mean), _p(invstd), _p(var), _p(running_mean), _p(running_var),
         _p(reduce_scratch(C_, x2d.device)), stream_ptr())
    return mean, invstd, var


def bn_apply_lrelu(x2d, mean, invstd, gamma, beta):
    P, C_ = x2d.shape
    y = torch.empty_like(x2d)
    call("afi_bn_apply_lrelu_fwd", _p(x2d), _p(y), _p(mean), _p(invstd), _p(gamma), _p(beta), P, C_, stream_ptr())
    return y


def bn_bwd(g2d, x2d, mean, invstd, gamma, dgamma, dbeta):
    P, C_ = x2d.shape
    dx = torch.empty_like(x2d)
    call("afi_bn_bwd", _p(g2d), _p(x2d), _p(dx), _p(mean), _p(invstd), _p(gamma), _p(dgamma), _p(dbeta), P, C_,
         _p(reduce_scratch(C_, x2d.device)), stream_ptr())
    return dx


def bn_bwd_sums(g2d, x2d, mean, invstd, dgamma, dbeta):
    """First half of bn_bwd (afi_bn_bwd_sums): [2, C] = (sum g, sum g * xhat) over this tensor's rows; dbeta / dgamma += them."""
    P, C_ = x2d.shape
    sums = torch.empty((2, C_), device=x2d.device)
    call("afi_bn_bwd_sums", _p(g2d), _p(x2d), _p(mean), _p(invstd), _p(dgamma), _p(dbeta), _p(sums), P, C_, _p(reduce_scratch(C_, x2d.device)), stream_ptr())
    return sums


def bn_bwd_apply(g2d, x2d, mean, invstd, gamma, sums, P_total):
    """Second half (afi_bn_bwd_apply): dx from sums taken over P_total rows in all (the caller's all-reduce of bn_bwd_sums)."""
    P, C_ = x2d.shape
    dx = torch.empty_like(x2d)
    call("afi_bn_bwd_apply", _p(g2d), _p(x2d), _p(dx), _p(mean), _p(invstd), _p(gamma), _p(sums), P, int(P_total), C_, stream_ptr())
    return dx


def colsum_accum(g2d, db, alpha=1.0):
    P, C_ = g2d.shape
    call("afi_colsum_accum", _p(g2d), P, C_, g2d.stride(0), float(alpha), _p(db), _p(reduce_scratch(C_, g2d.device)), stream_ptr())
    return db


def bce_logits(z, target, loss, lscale=1.0, gscale=1.0, want_grad=True):
    """*loss += lscale * BCEWithLogits(z, target).mean(); returns dz (or None)."""
    z = z.contiguous()
    dz = torch.empty_like(z) if want_grad else None
    call("afi_bce_logits_fwd_bwd", _p(z), z.numel(), float(target), float(lscale), _p(loss), float(gscale), _p(dz), stream_ptr())
    return dz


def l1_crop(a, b, loss, lscale=1.0, gscale=1.0, want_grad=True):
    """*loss += lscale * l1(a[:, :, :h, :w], b[:, :, :h, :w]) with h, w the common extent; returns da (dense, full extent of a)."""
    N, C_, Ha, Wa = a.shape
    h, w = min(Ha, b.shape[2]), min(Wa, b.shape[3])
    da = new_pixel_major(N, C_, Ha, Wa, a.device) if want_grad else None
    call("afi_l1_fwd_bwd", view_of(a), view_of(b), N, h, w, C_, Ha, Wa, float(lscale), _p(loss), float(gscale), _p(da), stream_ptr())
    return da


# ------------------------------------------------------------------------------------------------ CascadeROIHeads in training (roi_heads.py)
def roi_cascade_relabel(pred, K, proposals, counts, image_hw, weights, gt, gt_classes, counts_g, iou_thresh, scale_clamp=4.135166556742356):
    """The next cascade stage's training list from stage k's predictor output pred [N B, Cpad] and its boxes proposals [N, B, 4] / counts [N]
    (detectron2's _create_proposals_from_boxes + _match_and_label_boxes): decode and clip as roi_cascade_stage does, drop the boxes that
    clipped to empty keeping the order, match the rest to gt [N, Gmax, 4] / gt_classes [N, Gmax] / counts_g [N] at iou_thresh.  Returns a
    dict: boxes [N, B, 4], counts [N], gt_classes [N, B] int32 (K = background, -1 past counts), gt_boxes [N, B, 4], src [N, B] int32 (the
    input row, -1 past counts), matched_idx [N, B] int32 (afi_roi_cascade_relabel)."""
    p2, N, B = _roi_pred_rows("roi_cascade_relabel", pred, K, 1, proposals, counts, image_hw)
    if gt.dim() != 3 or gt.shape[0] != N or gt.shape[2] != 4 or gt.shape[1] < 1 or not gt.is_contiguous() \
            or tuple(gt_classes.shape) != tuple(gt.shape[:2]) or not gt_classes.is_contiguous() or tuple(counts_g.shape) != (N,) \
            or not counts_g.is_contiguous():
        raise _lib.AfiError(f"roi_cascade_relabel: dense ground truth [{N}, Gmax >= 1, 4], gt_classes [{N}, Gmax] and counts_g [{N}] expected, "
                            f"got {tuple(gt.shape)}, {tuple(gt_classes.shape)}, {tuple(counts_g.shape)}")
    if gt.shape[1] > RPN_MAX_GT:
        raise _lib.AfiError(f"roi_cascade_relabel: {gt.shape[1]} ground-truth boxes per image; at most {RPN_MAX_GT} are supported")
    if B > RPN_MAX_BATCH:
        raise _lib.AfiError(f"roi_cascade_relabel: lists of {B} rows per image; at most {RPN_MAX_BATCH} are supported")
    _check_cuda(gt)
    _check_i32(gt_classes, counts_g)
    if not float(iou_thresh) == float(iou_thresh):
        raise _lib.AfiError("roi_cascade_relabel: the IoU threshold is NaN")
    dev, Gmax = pred.device, gt.shape[1]
    r = {"boxes": torch.empty((N, B, 4), device=dev, dtype=torch.float32), "counts": torch.empty((N,), device=dev, dtype=torch.int32),
         "gt_classes": torch.empty((N, B), device=dev, dtype=torch.int32), "gt_boxes": torch.empty((N, B, 4), device=dev, dtype=torch.float32),
         "src": torch.empty((N, B), device=dev, dtype=torch.int32), "matched_idx": torch.empty((N, B), device=dev, dtype=torch.int32)}
    call("afi_roi_cascade_relabel", _p(p2), p2.stride(0), N, B, int(K), _p(proposals.contiguous()), _p(counts.contiguous()),
         _p(image_hw.contiguous()), *[float(w) for w in weights], float(scale_clamp), _p(gt), _p(gt_classes), _p(counts_g), Gmax, float(iou_thresh),
         _p(r["boxes"]), _p(r["counts"]), _p(r["gt_classes"]), _p(r["gt_boxes"]), _p(r["src"]), _p(r["matched_idx"]), stream_ptr())
    return r


ROI_BN_MAX_IMAGES = 1024                    # CT_MAX_N: the list-masked passes walk the counts of every image in every thread


def _roi_bn_list(name, x, counts, *same, vectors=()):
    """The checks of the list-masked BatchNorm passes: x (and every tensor of `same`) is the dense rows [N B, P1, C] or their pixel-major
    form [N B, C, S, S]; counts [N] int32; `vectors` are dense fp32 [C].  Shapes and limits first, then devices and dtypes.  Returns
    (N, B, P1, C)."""
    dense = x.is_contiguous() if x.dim() == 3 else is_dense_pm(x)
    if x.dim() not in (3, 4) or not dense or counts.dim() != 1 or counts.shape[0] < 1 or x.shape[0] % counts.shape[0] or x.shape[0] == 0 \
            or not counts.is_contiguous():
        raise _lib.AfiError(f"{name}: dense rows [N B, P1, C] (or pixel-major [N B, C, S, S]) and counts [N] with N dividing the rows expected, "
                            f"got {tuple(x.shape)} and {tuple(counts.shape)}")
    N, B = counts.shape[0], x.shape[0] // counts.shape[0]
    P1, C_ = (x.shape[1], x.shape[2]) if x.dim() == 3 else (x.shape[2] * x.shape[3], x.shape[1])
    if C_ % 4 or P1 < 1 or B > RPN_MAX_BATCH or N > ROI_BN_MAX_IMAGES:
        raise _lib.AfiError(f"{name}: {C_} channels (a multiple of 4 is needed), {P1} pixels per row, {B} rows per image (at most {RPN_MAX_BATCH}), "
                            f"{N} images (at most {ROI_BN_MAX_IMAGES})")
    for t in same:
        if t is not None and (t.shape != x.shape or t.stride() != x.stride()):
            raise _lib.AfiError(f"{name}: every row tensor must have x's shape and memory layout, got {tuple(t.shape)} for {tuple(x.shape)}")
    for v in vectors:
        if v is not None and (tuple(v.shape) != (C_,) or not v.is_contiguous()):
            raise _lib.AfiError(f"{name}: dense per-channel vectors [{C_}] expected, got {tuple(v.shape)}")
    _check_cuda(x, *same, *[v for v in vectors if v is not None])
    _check_i32(counts)
    return N, B, P1, C_


def roi_bn_stats(x, counts, eps, momentum, running_mean=None, running_var=None, num_batches_tracked=None, want_var=False):
    """Train-mode BatchNorm statistics over the valid rows (j < counts[n]) of the padded list x [N B, P1, C] (or pixel-major [N B, C, S, S]):
    (mean, invstd[, biased var]); the running buffers and the counter are updated in place, and left alone when no row is valid
    (afi_roi_bn_stats)."""
    N, B, P1, C_ = _roi_bn_list("roi_bn_stats", x, counts, vectors=(running_mean, running_var))
    if (running_mean is None) != (running_var is None):
        raise _lib.AfiError("roi_bn_stats: running_mean and running_var come together")
    if num_batches_tracked is not None and (not num_batches_tracked.is_cuda or num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1):
        raise _lib.AfiError("roi_bn_stats: num_batches_tracked must be one int64 on the GPU")
    mean, invstd = torch.empty(C_, device=x.device), torch.empty(C_, device=x.device)
    var = torch.empty(C_, device=x.device) if want_var else None
    call("afi_roi_bn_stats", _p(x), _p(counts), N, B, P1, C_, float(eps), float(momentum), _p(mean), _p(invstd), _p(var), _p(running_mean),
         _p(running_var), _p(num_batches_tracked), _p(reduce_scratch(C_, x.device)), stream_ptr())
    return (mean, invstd, var) if want_var else (mean, invstd)


def roi_bn_relu_fwd(x, counts, mean, invstd, gamma, beta, relu=True):
    """y = max(0, (x - mean) invstd gamma + beta) on the valid rows of the padded list (relu=False: the plain affine), exactly 0 on its
    padding rows, in x's layout (afi_roi_bn_relu_fwd)."""
    N, B, P1, C_ = _roi_bn_list("roi_bn_relu_fwd", x, counts, vectors=(mean, invstd, gamma, beta))
    y = torch.empty_like(x)
    call("afi_roi_bn_relu_fwd", _p(x), _p(counts), N, B, P1, C_, _p(mean), _p(invstd), _p(gamma), _p(beta), int(bool(relu)), _p(y), stream_ptr())
    return y


def roi_bn_relu_bwd_sums(g, x, y, counts, mean, invstd, dgamma=None, dbeta=None, relu=True):
    """[2, C] = (sum g', sum g' xhat) over the valid rows, g' = g [y > 0] from the stored y (relu=False: g' = g, y may be None); dbeta /
    dgamma += them (afi_roi_bn_relu_bwd_sums)."""
    if relu and y is None:
        raise _lib.AfiError("roi_bn_relu_bwd_sums: relu=True needs the forward's stored y (the mask is the forward's)")
    N, B, P1, C_ = _roi_bn_list("roi_bn_relu_bwd_sums", x, counts, g, y if relu else None, vectors=(mean, invstd, dgamma, dbeta))
    sums = torch.empty((2, C_), device=x.device)
    call("afi_roi_bn_relu_bwd_sums", _p(g), _p(x), _p(y if relu else None), _p(counts), N, B, P1, C_, _p(mean), _p(invstd), int(bool(relu)),
         _p(dgamma), _p(dbeta), _p(sums), _p(reduce_scratch(C_, x.device)), stream_ptr())
    return sums


def roi_bn_relu_bwd_apply(g, x, y, counts, mean, invstd, gamma, sums, relu=True):
    """dx = gamma invstd (g' - s0 / Pn - xhat s1 / Pn) on the valid rows, 0 on the padding rows, Pn formed from counts on the device
    (afi_roi_bn_relu_bwd_apply)."""
    if relu and y is None:
        raise _lib.AfiError("roi_bn_relu_bwd_apply: relu=True needs the forward's stored y (the mask is the forward's)")
    N, B, P1, C_ = _roi_bn_list("roi_bn_relu_bwd_apply", x, counts, g, y if relu else None, vectors=(mean, invstd, gamma))
    _check_cuda(sums)
    if tuple(sums.shape) != (2, C_) or not sums.is_contiguous():
        raise _lib.AfiError(f"roi_bn_relu_bwd_apply: dense sums [2, {C_}] expected, got {tuple(sums.shape)}")
    dx = torch.empty_like(x)
    call("afi_roi_bn_relu_bwd_apply", _p(g), _p(x), _p(y if relu else None), _p(counts), N, B, P1, C_, _p(mean), _p(invstd), _p(gamma), _p(sums),
         int(bool(relu)), _p(dx), stream_ptr())
    return dx
