"""afi_conv1x1_frozen_fwd (csrc/frozen1x1.hip: the 1x1 conv of frozen weights on the bf16 matrix cores, bf16x6 operands over a weight image
built once) called directly, against torch CPU float64 on the same fp32 inputs.

Bars: those of tests/test_gpu_pixgemm.py for this operation, restated (eps = 2^-24, K = Cin):
  max-norm   max|got - ref| / max|ref|   <= min(2 sqrt(K) eps, 1e-5)
  rel. L2    ||got - ref|| / ||ref||     <= 4 max(torch CPU fp32's rel. L2, sqrt(K) eps / 8)
Every case prints the kernel's error, torch CPU fp32's and the bar, and asserts besides: profiler kind 23 ran and no pixel-GEMM kind did; two
runs are bit-identical; an output placed in the middle of a NaN-filled buffer leaves its neighbours NaN.  Unsupported views (Cin = 36, a
channel slice of a wider tensor) return AFI_ERR_UNSUPPORTED and launch nothing.

Shapes, the smallest at which each mechanism can go wrong: one K step and one partial row tile (32 -> 32 @ 5x7); row tiles that straddle the
image boundary and a ragged last tile (64 -> 256 @ 65x67); two K chunks of 128 with an addend, alpha and LeakyReLU (256 -> 64); every second
pixel of an odd-height map (the stride-2 read in place); long K and several column tiles (2048 <-> 512); channel counts that are no multiple
of 64 or 128 (96 -> 160: K chunks of 32, a ragged last column tile); several column tiles per row tile (256 -> 1024, the 128-column tile);
a shape above the routing threshold (64 -> 256 @ 96x96: 288 row tiles, the 128-column tile); and, beyond the issue's list, the 256-column
tile the largest maps run (from 512 row tiles on), once with a ragged second column tile.  TILE_BN pins the tile form of each case.

Measured on MI355X (kernel error / bar; torch CPU fp32's error): max-norm 7.3e-8 / 6.7e-7 (1.8e-7) at K = 32, 1.6e-7 .. 1.9e-7 / 9.5e-7
(2.3e-7 .. 3.1e-7) at K = 64, 2.5e-7 .. 4.0e-7 / 1.9e-6 (1.5e-7 .. 5.9e-7) at K = 256, 6.0e-7 / 2.7e-6 (7.7e-7) at K = 512, 1.1e-6 / 5.4e-6
(2.9e-7) at K = 2048; rel. L2 0.10 .. 0.37 of its bar.  The kernel sits below torch CPU fp32's error up to K = 512 and at 3.9x (max-norm) /
2.4x (rel. L2) of it at K = 2048: bf16x6 drops the three smallest of the nine partial products and accumulates 64 K steps in order.
What the bars catch (scratch builds, never committed; this file's eleven fp64 cases run against each): the image builder storing zeros for
the third (lo) plane -- all eleven cases fail, the smallest (K = 32) at max-norm 2.7e-6 against its bar of 6.7e-7 (4.0x) and rel. L2 2.5e-6
against 3.9e-7 (6.3x); the kernel skipping the last K step of a tile -- all eleven fail (K = 32: the whole product is missing, error 1.0).
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
PIX_KINDS = (0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 15, 20)       # tests/test_gpu_pixgemm.py
KIND = 23
UNSUPPORTED = 2
NAN = float("nan")

# (N, Cin, Cout, H, W, view, epilogue)
CASES = [
    (1, 32, 32, 5, 7, "dense", dict()),
    (2, 64, 256, 65, 67, "dense", dict(bias=1, act=2)),
    (2, 256, 64, 33, 35, "dense", dict(add=1, add_scale=-0.5, alpha=0.5, act=1)),
    (2, 64, 128, 37, 41, "s2", dict(bias=1)),
    (1, 2048, 512, 9, 11, "dense", dict(bias=1)),
    (1, 512, 2048, 9, 11, "dense", dict(bias=1, act=2)),
    (1, 96, 160, 40, 40, "dense", dict(bias=1, add=1)),
    (1, 256, 1024, 70, 60, "dense", dict(bias=1)),
    (2, 64, 256, 96, 96, "dense", dict(bias=1, add=1, act=2)),
    # beyond the issue's list: the 256-column tile (the plan takes it from 512 row tiles on), once as the large 64 -> 256 maps run it and once
    # with two K chunks and a ragged second column tile (Cout = 320: three of its four waves own no column)
    (2, 64, 256, 128, 128, "dense", dict(bias=1, act=2)),
    (1, 256, 320, 128, 128, "dense", dict(bias=1, add=1)),
]
TILE_BN = {(2, 64, 256, 96, 96): 128, (1, 256, 1024, 70, 60): 128, (2, 64, 256, 128, 128): 256, (1, 256, 320, 128, 128): 256}   # every other case: 64


def _id(c):
    N, Cin, Cout, H, W, view, ep = c
    return f"{N}x{Cin}to{Cout}@{H}x{W}-{view}" + "".join(f"-{k}{v}" for k, v in sorted(ep.items()))


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _pm(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _profiled(fn):
    from afigan_amd import _lib
    lib = _lib.load()
    _lib.check(lib.afi_profile_enable(1), "afi_profile_enable")
    try:
        out = fn()
        torch.cuda.synchronize()
        ran, buf = {}, (C.c_double * 3)()
        for k in range(lib.afi_profile_num_kinds()):
            _lib.check(lib.afi_profile_get(k, buf), "afi_profile_get")
            if buf[0]:
                ran[k] = int(buf[0])
    finally:
        lib.afi_profile_enable(0)
    return out, ran


def _errs(got, ref):
    d = (got.double() - ref).flatten()
    r = ref.flatten()
    return (d.abs().max() / r.abs().max().clamp_min(1e-300)).item(), (d.norm() / r.norm().clamp_min(1e-300)).item()


def test_kind_23_is_appended_and_priced_as_bf16x6(amd):
    lib = amd._lib.load()
    assert lib.afi_profile_num_kinds() == 24
    name = lib.afi_profile_kind_name(KIND).decode()
    assert "bf16x6 operands" in name and name not in {lib.afi_profile_kind_name(k).decode() for k in range(KIND)}


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_frozen_1x1_vs_fp64(amd, case):
    ops = amd.ops
    N, Cin, Cout, H, W, view, ep = case
    X = _rand((N, Cin, H, W), 1)
    Wt = _rand((Cout, Cin), 2) / math.sqrt(Cin)
    b = _rand((Cout,), 3) if ep.get("bias") else None
    add = _rand((N, Cout, H, W), 4) if ep.get("add") else None
    alpha, add_scale, act = ep.get("alpha", 1.0), ep.get("add_scale", 1.0), ep.get("act", 0)
    if view == "s2":                                       # every second pixel of a (2H - 1) x 2W map (odd height), read in place
        big = _rand((N, Cin, 2 * H - 1, 2 * W), 5)
        big[:, :, ::2, ::2] = X
        keep = _pm(big)
        xg = keep[:, :, ::2, ::2]
    else:
        xg = _pm(X)

    def ref(dt):
        y = alpha * F.conv2d(X.to(dt), Wt.to(dt)[:, :, None, None])
        if b is not None:
            y = y + b.to(dt).view(1, -1, 1, 1)
        if add is not None:
            y = y + add_scale * add.to(dt)
        return y if act == 0 else (F.leaky_relu(y, 0.2) if act == 1 else F.relu(y))

    ref64, ref32 = ref(torch.float64), ref(torch.float32)
    wg, bg, addg = Wt.cuda(), (b.cuda() if b is not None else None), (_pm(add) if add is not None else None)
    plan = ops.conv1x1_frozen_plan(N, H, W, Cin, Cout, (xg.stride(0), xg.stride(2), xg.stride(3)),
                                   add_strides=(addg.stride(0), addg.stride(2), addg.stride(3)) if addg is not None else None)
    assert plan is not None and plan["BN"] == TILE_BN.get((N, Cin, Cout, H, W), 64), plan      # the tile form the case is here for
    image = ops.conv1x1_frozen_image(wg)
    # the output in the middle of a NaN-filled buffer: its neighbours must stay NaN
    pad = 1024
    buf = torch.full((2 * pad + N * H * W * Cout,), NAN, device="cuda")
    out = buf[pad:pad + N * H * W * Cout].view(N, H, W, Cout).permute(0, 3, 1, 2)
    got, ran = _profiled(lambda: ops.conv1x1_frozen_fwd(xg, image, bg, Cout, add=addg, add_scale=add_scale, alpha=alpha, out=out, act=act))
    assert ran.get(KIND) == 1 and not any(k in ran for k in PIX_KINDS), f"expected kind {KIND} alone, the profiler saw {ran}"
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + N * H * W * Cout:]).all(), "the kernel wrote outside its output"
    assert not torch.isnan(got).any()
    again = ops.conv1x1_frozen_fwd(xg, image, bg, Cout, add=addg, add_scale=add_scale, alpha=alpha, act=act)
    assert torch.equal(again, got), "two runs differ"
    em, el = _errs(got.cpu(), ref64)
    cm, cl = _errs(ref32, ref64)
    bar, l2bar = min(2.0 * math.sqrt(Cin) * EPS, 1e-5), 4.0 * max(cl, math.sqrt(Cin) * EPS / 8)
    print(f"[frozen1x1] {_id(case):58s} max-norm {em:.2e} (cpu fp32 {cm:.2e}, bar {bar:.2e})  rel-L2 {el:.2e} (cpu fp32 {cl:.2e}, bar {l2bar:.2e})")
    assert em <= bar, f"max-norm rel error {em:.3e} > bar {bar:.3e} (cpu fp32 {cm:.3e})"
    assert el <= l2bar, f"rel-L2 error {el:.3e} > bar {l2bar:.3e} (cpu fp32 {cl:.3e})"


def test_unsupported_views_launch_nothing(amd):
    ops, _lib = amd.ops, amd._lib
    lib = _lib.load()
    image = ops.conv1x1_frozen_image(torch.randn(64, 32, device="cuda"))
    out = ops.new_pixel_major(1, 64, 9, 9, "cuda")

    def raw(x, Cin):
        N, _, H, W = x.shape
        return lib.afi_conv1x1_frozen_fwd(_lib.current_ctx().handle, ops.view_of(x), N, H, W, Cin, ops._p(image), None, 64, ops.view_of(out), 1.0,
                                          _lib.View(None, 0, 0, 0), 1.0, 0, ops.stream_ptr())

    x36 = _pm(torch.randn(1, 36, 9, 9))
    wide = _pm(torch.randn(1, 64, 9, 9))
    for x, Cin in ((x36, 36), (wide[:, :32], 32), (wide[:, 32:], 32)):
        st, ran = _profiled(lambda: raw(x, Cin))
        assert st == UNSUPPORTED and not ran, (Cin, st, ran)
        assert ops.conv1x1_frozen_plan(1, 9, 9, Cin, 64, (x.stride(0), x.stride(2), x.stride(3))) is None
    with pytest.raises(_lib.AfiError):
        ops.conv1x1_frozen_fwd(x36, image, None, 64)
