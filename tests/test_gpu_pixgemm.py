"""Every pixel-GEMM kernel variant against a float64 reference, at fp32-grade bars, with proof of which kernel ran.

The direct convolutions (everything that does not run in Winograd form) go through one dispatcher, afi_launch_pix_gemm
(csrc/igemm.hip), and its weight-gradient counterpart afi_launch_wgrad_gemm.  Each case below names the entry point, the shape,
the input and output views, the epilogue and the profiler kind it must run on (kKindNames in csrc/igemm.hip):

   0 / 4   pix_gemm<128x128, KC / RC>        linear tiles; mid-size maps split K over 3-4 blocks (slab reduction)
   1 / 5   pix_gemm<128x64,  KC / RC>        Ncols <= 64, >= 128 tiles of 128x128
   2 / 6   pix_gemm<128x32,  KC / RC>        Ncols <= 32, >= 128 tiles of 128x128
   3 / 7   pix_gemm<64x64,   KC / RC>        generic-tap (stride-2) convs with M <= 64*256 or Ncols <= 64
  11 / 12  pix_gemm<128x128, KC / RC, halo>  3x3 stride-1 on maps whose 8x16 patch grid wastes <= 12 %
   8 9 10  wgrad_gemm<128 / 64 / 32 x 128>   weight gradients, by Mrows (Cout, 4*Cout for the conv-transpose)
  15       small-map pixel GEMM (< 128 tiles of 128x128): pix_gemm_wk (K split inside the block), or -- where wk_prepare
           refuses the problem (operand byte extents >= 2 GB) -- the stream-K kernel launch_sk with its slab-reduction pass.
           Both record as kind 15; the stream-K cases assert the byte extent that forces the fallback.
  16 19 20 the grouped weight gradients and the bf16x6 small-map kernel on weight images: only a whole interpolator call reaches them; held by
           tests/test_gpu_smallmap.py.

The profiler (afi_profile_enable / afi_profile_get) shows every launch of the call: a case passes only if its named kind ran and no
other pixel-GEMM or weight-gradient kind did, so a change of the dispatch cannot quietly move a case off its kernel.

Reference: torch CPU float64 on the same fp32 inputs.  Torch CPU fp32's own error against it is printed next to the kernel's.
Bars (Ktot = the reduction length: taps * channels, or pixels for a weight gradient; eps = 2^-24):
  max-norm   max|got - ref| / max|ref|              <= C_MAX * sqrt(Ktot) * eps    (never above 1e-5 for Ktot <= 2304, 5e-5 else)
  rel. L2    ||got - ref|| / ||ref||                 <= R_L2 * max(cpu fp32 rel. L2, sqrt(Ktot) * eps / 8)
2-byte outputs (the _out16 forms) must equal the same kernel's fp32 output rounded once, bit for bit.  Weight gradients run under
AFI_OPT_DETERMINISTIC 0 (atomics over pixel splits: within the bar) and 1 (two runs bit-identical, and within the bar).

Measured on MI355X: the case of each kind that comes closest to its max-norm bar (kernel error / bar, Ktot, torch CPU fp32's error).
Over all cases the kernels sit at 0.04 .. 1.06 sqrt(Ktot) eps (forward and data-gradient kinds <= 0.82; the largest, 1.06, is a
deterministic weight gradient, whose single block sums all pixels in order) and at <= 2.4x the L2 reference.
   0  3.0e-07 / 9.5e-07  (Ktot   64, cpu 4.8e-07)        8  1.7e-06 / 3.2e-06  (Ktot 714, cpu 5.1e-07)
   1  2.9e-07 / 9.5e-07  (Ktot   64, cpu 4.8e-07)        9  8.4e-07 / 2.8e-06  (Ktot 546, cpu 5.9e-07)
   2  1.8e-07 / 6.7e-07  (Ktot   32, cpu 1.8e-07)       10  9.0e-07 / 2.8e-06  (Ktot 546, cpu 4.5e-07)
   3  5.4e-07 / 2.0e-06  (Ktot  288, cpu 3.1e-07)       11  7.7e-07 / 2.0e-06  (Ktot 288, cpu 3.6e-07)
   4  5.5e-07 / 1.3e-06  (Ktot  128, cpu 6.2e-07)       12  7.0e-07 / 2.9e-06  (Ktot 576, cpu 3.3e-07)
   5  3.6e-07 / 3.5e-06  (Ktot  864, cpu 3.1e-07)       15  1.8e-07 / 6.7e-07  (Ktot  32, cpu 1.5e-07)
   6  3.8e-07 / 9.5e-07  (Ktot   64, cpu 4.5e-07)
   7  5.0e-07 / 1.3e-06  (Ktot  128, cpu 5.0e-07)
What the bars catch (scratch builds, never committed): the tiled kernel's A operand rounded to bf16 at the tile load (every
tiled case: ~1.5e-3), the tile's last K stage of pix_gemm_wk skipped (every wk case), the stream-K kernel addressing its A
operand with 32-bit byte offsets (the stream-K case past element 2^31).
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
C_MAX = 2.0            # max-norm bar: C_MAX * sqrt(Ktot) * eps (measured: <= 1.06)
R_L2 = 4.0             # rel. L2 bar: R_L2 * max(cpu fp32's, sqrt(Ktot) * eps / 8) (measured: <= 2.4)
PIX_KINDS = (0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 15, 20)
WGRAD_KINDS = (8, 9, 10, 16, 19)
LRELU = 0.2
NAN = float("nan")


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _pm(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------ case table
class Case:
    """op: fwd3 / dgrad3 / wgrad3 (conv3x3), fwd1 / dgrad1 / wgrad1 (conv1x1), fwd3s2 / dgrad3s2 / wgrad3s2 (Conv2d k3 s2 p1),
    fwdT / dgradT / wgradT (ConvTranspose2d k6 s2 p2 in four phases).  H, W: the map the op's input lives on (the conv's input for
    forwards and weight gradients, dy's map for data gradients of stride-1 convs; the conv's input map for every stride-2 op).
    view: how the GEMM's A operand is handed over -- dense, crop (a corner of a larger map), cslice (channels 4.. of a wider
    buffer), s2 (every second pixel of a larger map: resnet_guide._conv1x1), far (images `gap` floats apart in one buffer).
    out: fresh, or slice (channels 4.. of a wider buffer that holds other data: written with beta, neighbours must stay bit-identical).
    ep: epilogue terms (bias, alpha, beta, act, add, add_scale, post_scale, keep_act, z); o16: 2-byte output dtype."""

    def __init__(self, op, N, Cin, Cout, H, W, kind, view="dense", out="fresh", o16=None, gap=0, **ep):
        self.op, self.N, self.Cin, self.Cout, self.H, self.W, self.kind = op, N, Cin, Cout, H, W, kind
        self.view, self.out, self.o16, self.gap, self.ep = view, out, o16, gap, ep

    def __repr__(self):
        e = ",".join(f"{k}={v}" for k, v in sorted(self.ep.items()))
        o16 = f",{str(self.o16)[6:]}" if self.o16 else ""
        return f"{self.op}-N{self.N}-{self.Cin}to{self.Cout}-{self.H}x{self.W}-k{self.kind}-{self.view}-{self.out}{o16}{',' + e if e else ''}"


GAP_2GB = 280_000_000          # floats between the two images of a `far` view: 1.12 GB, so the view spans 2.24 GB
GAP_2P31 = (1 << 31) + 1024    # floats: element offsets past 2^31 (an 8.6 GB buffer)

CASES = [
    # ---- small maps (< 128 tiles of 128x128): pix_gemm_wk
    Case("fwd3", 1, 4, 4, 5, 7, 15, bias=1),                                        # smallest channel counts
    Case("fwd3", 2, 28, 36, 7, 11, 15, bias=1, act=1),                              # K tail: Cin % 32 = 28
    Case("fwd3", 3, 36, 12, 6, 5, 15, act=2),                                       # K tail: Cin % 32 = 4
    Case("fwd3", 1, 1024, 64, 9, 10, 15, bias=1),                                   # long K: 3x3 over 1024 channels
    Case("fwd3", 1, 32, 40, 1, 37, 15, bias=1),                                     # one row
    Case("fwd3", 2, 32, 40, 29, 1, 15, bias=1),                                     # one column
    Case("fwd3", 2, 64, 32, 13, 21, 15, out="slice", bias=1, alpha=0.7, beta=0.5, act=2),
    Case("fwd3", 2, 16, 12, 9, 12, 15, view="crop", act=1),
    Case("fwd3", 2, 24, 16, 9, 12, 15, view="cslice", bias=1),
    Case("fwd3", 1, 32, 32, 13, 21, 15, o16=torch.bfloat16, bias=1, act=1),
    Case("fwd3", 1, 32, 32, 13, 21, 15, o16=torch.float16, bias=1),
    Case("fwd3", 1, 32, 128, 127, 128, 15),                                         # 127 tiles: the last small map
    Case("fwd3", 1, 32, 128, 64, 128, 15),                                          # 64 tiles at Ncols 128 (see 132 below)
    Case("dgrad3", 2, 32, 256, 25, 34, 15, z=1),
    Case("dgrad3", 1, 4, 4, 5, 7, 15),
    Case("dgrad3", 2, 36, 28, 9, 13, 15, out="slice", alpha=0.5, beta=1.0),
    Case("fwd1", 1, 2048, 256, 13, 17, 15, bias=1),                                 # long K: 1x1 over 2048 channels
    Case("fwd1", 2, 64, 128, 17, 21, 15, view="s2", bias=1, alpha=0.5, add=1, add_scale=0.25, act=1),
    Case("fwd1", 1, 32, 36, 11, 13, 15, out="slice", bias=1, act=2),
    Case("dgrad1", 2, 64, 512, 7, 9, 15),
    Case("dgrad1", 1, 64, 128, 9, 11, 15, o16=torch.float16),
    Case("dgrad1", 1, 64, 128, 9, 11, 15, o16=torch.bfloat16, alpha=0.5),
    Case("fwdT", 1, 32, 32, 7, 9, 15, bias=1, act=1),
    Case("dgradT", 1, 32, 32, 7, 9, 15, z=1),
    # ---- small maps, stream-K fallback: the view spans >= 2 GB, which wk_prepare refuses
    Case("fwd1", 2, 128, 32, 9, 11, 15, view="far", gap=GAP_2GB, bias=1, act=1),              # short K: whole tiles, no second pass
    Case("dgrad3", 3, 32, 64, 9, 11, 15, view="far", gap=GAP_2GB, z=1),                      # 128x32 RC form, 18 stages; image 2 past 2 GiB
    Case("fwd3", 2, 256, 64, 13, 17, 15, view="far", gap=GAP_2P31, out="slice", bias=1),     # long K: stream-K partition + reduce pass;
                                                                                              # element offsets past 2^31
    # ---- tiled kernels
    Case("fwd3", 1, 32, 132, 64, 128, 11),                                          # Ncols 132: 128 tiles, exact patch grid -> halo
    Case("fwd3", 2, 32, 128, 65, 256, 11, bias=1, act=1),                           # patch waste 10.8 %: halo
    Case("fwd3", 2, 32, 128, 57, 256, 0, bias=1, act=1),                            # patch waste 12.3 %: linear tiles
    Case("fwd3", 1, 16, 128, 1, 16257, 0, bias=1),                                  # one row, 128 tiles: the first map off the small-map path
    Case("fwd3", 1, 16, 32, 16257, 1, 2),                                           # one column
    Case("fwd3", 2, 4, 32, 96, 96, 2, bias=1, act=2),                               # Cin = 4 on the 128x32 tile
    Case("fwd3", 1, 28, 64, 130, 127, 1, out="slice", bias=1, alpha=0.7, beta=0.5),
    Case("fwd3", 2, 32, 32, 96, 96, 2, o16=torch.bfloat16, bias=1),
    Case("fwd3", 2, 32, 136, 96, 96, 11, o16=torch.float16, act=1),                 # exact patch grid, two N tiles of the 128-column halo kernel
    Case("fwd3", 1, 16, 128, 1, 16257, 0, o16=torch.float16, act=1),
    Case("fwd1", 1, 2048, 256, 64, 128, 0, bias=1),                                 # long K 1x1 on linear tiles (mid-size split-K)
    Case("fwd1", 1, 64, 32, 128, 130, 2, bias=1),                                   # Ncols 32 | 36
    Case("fwd1", 1, 64, 36, 128, 130, 1, bias=1),
    Case("fwd1", 1, 64, 64, 128, 130, 1, act=1),                                    # Ncols 64 | 68
    Case("fwd1", 1, 64, 68, 128, 130, 0, act=1),
    Case("fwd1", 2, 64, 128, 75, 111, 0, view="s2", bias=1, add=1, add_scale=-0.5, act=2),   # tiles straddle images; stride-2 view
    Case("fwd1", 2, 32, 32, 96, 96, 2, view="far", gap=GAP_2P31, bias=1),            # element offsets past 2^31
    Case("dgrad3", 2, 128, 64, 64, 128, 12, z=1),                                   # halo RC
    Case("dgrad3", 3, 64, 96, 73, 75, 5),                                           # Ncols 64, tiles straddle images
    Case("dgrad1", 2, 128, 256, 75, 111, 4),
    Case("dgrad1", 1, 32, 64, 128, 129, 6, alpha=2.0),
    Case("dgrad1", 1, 32, 64, 128, 129, 6, o16=torch.float16),
    Case("fwdT", 1, 32, 32, 128, 128, 11, bias=1),                                  # halo with the pixel-shuffle store (o_up = 2)
    Case("dgradT", 1, 32, 32, 128, 128, 6, z=1),                                    # four K phases (nKphase = 4, a_up = 2)
    # ---- generic-tap (stride-2) forms: small = M <= 64*256 or Ncols <= 64
    Case("fwd3s2", 1, 32, 128, 256, 256, 3, bias=1),                                # M = 16384: 64x64
    Case("fwd3s2", 1, 32, 128, 258, 256, 0, bias=1),                                # M = 16512: 128x128
    Case("fwd3s2", 1, 28, 64, 259, 257, 3, act=1),                                  # Ncols 64 | 68, odd sizes
    Case("fwd3s2", 1, 28, 68, 259, 257, 0, act=2, add=1, add_scale=0.5, post_scale=2.0, keep_act=1),
    Case("fwd3s2", 2, 16, 32, 25, 33, 3, bias=1, act=1, add=1, add_scale=1.0, post_scale=0.5, keep_act=1),
    Case("fwd3s2", 1, 4, 4, 3, 1, 3),
    Case("dgrad3s2", 2, 32, 64, 25, 33, 7),
    Case("dgrad3s2", 1, 4, 4, 1, 3, 7),
    Case("dgrad3s2", 1, 128, 32, 259, 257, 4, alpha=0.5),
    Case("dgrad3s2", 1, 64, 32, 259, 257, 7),                                       # Ncols 64 at the large M: 64x64
]

WGRAD_CASES = [
    Case("wgrad3", 1, 4, 4, 5, 7, 10),
    Case("wgrad3", 2, 36, 32, 13, 21, 10, alpha=0.5),                               # Mrows 32 | 36
    Case("wgrad3", 2, 28, 36, 13, 21, 9, alpha=0.5),
    Case("wgrad3", 2, 32, 64, 13, 21, 9, view="crop"),                               # Mrows 64 | 68
    Case("wgrad3", 2, 32, 68, 13, 21, 8, view="cslice"),
    Case("wgrad3", 2, 64, 128, 96, 96, 8, alpha=0.25),                               # 18432 pixels: split over blocks under det 0
    Case("wgrad3", 1, 32, 32, 1, 37, 10),                                            # one row
    Case("wgrad1", 2, 2048, 256, 9, 11, 8),
    Case("wgrad1", 2, 64, 128, 17, 21, 8, view="s2"),
    Case("wgrad1", 1, 64, 32, 128, 130, 10),
    Case("wgrad3s2", 2, 32, 64, 25, 33, 9, alpha=0.5),
    Case("wgrad3s2", 1, 16, 128, 259, 257, 8),
    Case("wgradT", 1, 32, 32, 7, 9, 8),
    Case("wgradT", 1, 32, 8, 64, 64, 10),                                            # Mrows = 4 * 8
]


# ------------------------------------------------------------------------------------------------ references
def _act(v, a):
    if a == 1:
        return torch.where(v > 0, v, v * LRELU)
    if a == 2:
        return torch.clamp_min(v, 0)
    return v


def _zmask(v, z):
    return v * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, LRELU))


def _conv(op, dt, X, Wt, in_hw=None):
    """the plain linear operation of `op` on CPU tensors cast to dt: forward, data gradient (X = dy) or weight gradient (X = (dy, x))"""
    g = torch.nn.grad
    if op == "fwd3":
        return F.conv2d(X.to(dt), Wt.to(dt), None, 1, 1)
    if op == "fwd1":
        return F.conv2d(X.to(dt), Wt.to(dt))
    if op == "fwd3s2":
        return F.conv2d(X.to(dt), Wt.to(dt), None, 2, 1)
    if op == "fwdT":
        return F.conv_transpose2d(X.to(dt), Wt.to(dt), None, 2, 2)
    if op == "dgrad3":
        return F.conv_transpose2d(X.to(dt), Wt.to(dt), None, 1, 1)
    if op == "dgrad1":
        return F.conv_transpose2d(X.to(dt), Wt.to(dt))
    if op == "dgrad3s2":
        N = X.shape[0]
        return g.conv2d_input((N, Wt.shape[1]) + tuple(in_hw), Wt.to(dt), X.to(dt), 2, 1)
    if op == "dgradT":
        return F.conv2d(X.to(dt), Wt.to(dt), None, 2, 2)
    dy, x = X[0].to(dt), X[1].to(dt)
    if op == "wgrad3":
        return g.conv2d_weight(x, (dy.shape[1], x.shape[1], 3, 3), dy, 1, 1)
    if op == "wgrad1":
        return g.conv2d_weight(x, (dy.shape[1], x.shape[1], 1, 1), dy)
    if op == "wgrad3s2":
        return g.conv2d_weight(x, (dy.shape[1], x.shape[1], 3, 3), dy, 2, 1)
    if op == "wgradT":       # weight [Cin][Cout][6][6] of conv_transpose2d(x): the gradient of <dy, convT(x, w)>
        w = torch.zeros((x.shape[1], dy.shape[1], 6, 6), dtype=dt, requires_grad=True)
        F.conv_transpose2d(x, w, None, 2, 2).backward(dy)
        return w.grad
    raise ValueError(op)


def _ktot(c):
    if c.op in ("fwd3", "fwd3s2", "fwdT"):
        return 9 * c.Cin
    if c.op == "fwd1":
        return c.Cin
    if c.op == "dgrad3":
        return 9 * c.Cout
    if c.op == "dgrad1":
        return c.Cout
    if c.op == "dgrad3s2":
        return 4 * c.Cout
    if c.op == "dgradT":
        return 36 * c.Cout
    if c.op == "wgrad3s2":
        return c.N * ((c.H + 1) // 2) * ((c.W + 1) // 2)
    return c.N * c.H * c.W                       # wgrad3 / wgrad1 / wgradT: pixels of the (low-res) map


def _bar(ktot):
    cap = 1e-5 if ktot <= 2304 else 5e-5
    return min(C_MAX * math.sqrt(ktot) * EPS, cap)


def _errs(got, ref):
    d = (got.double() - ref).flatten()
    r = ref.flatten()
    return (d.abs().max() / r.abs().max().clamp_min(1e-300)).item(), (d.norm() / r.norm().clamp_min(1e-300)).item()


# ------------------------------------------------------------------------------------------------ GPU side
def _profiled(fn):
    """run fn() with the library's launch profiler on; returns (fn's result, {kind: launches})"""
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


def _check_kind(c, ran):
    fam = PIX_KINDS if not c.op.startswith("wgrad") else WGRAD_KINDS
    got = {k for k in ran if k in fam}
    assert got == {c.kind}, f"{c}: expected kind {c.kind} alone, the profiler saw {ran}"


def _far(X, gap):
    """X [N,C,H,W] (CPU) placed on the GPU as a pixel-major view whose images start `gap` floats apart in one NaN-filled buffer"""
    N, C_, H, W = X.shape
    assert gap % 4 == 0 and gap >= C_ * H * W
    buf = torch.full(((N - 1) * gap + C_ * H * W,), NAN, device="cuda")
    v = buf.as_strided((N, C_, H, W), (gap, 1, W * C_, C_))
    v.copy_(X.cuda())
    return v, buf


def _wk_a_extent_bytes(v, N, H, W, Ck, a_up=1):
    """the A-operand byte extent wk_prepare (csrc/smallmap.hip) computes for a view; >= 0x7FFFFFF0 sends the problem to stream-K"""
    sN, sH, sW = v.stride(0), v.stride(2), v.stride(3)
    return (abs(sN) * N + abs(sH) * (H * a_up + 2) + abs(sW) * (W * a_up + 2) + Ck + 64) * 4


def _operand(c, X, seed):
    """(GPU view handed to the op, CPU fp32 tensor it holds, keep-alive): the case's A-operand view of the logical tensor X"""
    N, C_, H, W = X.shape
    if c.view == "dense":
        return _pm(X), X, None
    if c.view == "crop":
        big = _rand((N, C_, H + 3, W + 2), seed)
        big[:, :, :H, :W] = X
        g = _pm(big)
        return g[:, :, :H, :W], X, g
    if c.view == "cslice":
        big = _rand((N, C_ + 8, H, W), seed)
        big[:, 4:4 + C_] = X
        g = _pm(big)
        return g[:, 4:4 + C_], X, g
    if c.view == "s2":
        big = _rand((N, C_, 2 * H - 1, 2 * W), seed)
        big[:, :, ::2, ::2] = X
        g = _pm(big)
        return g[:, :, ::2, ::2], X, g
    if c.view == "far":
        v, buf = _far(X, c.gap)
        return v, X, buf
    raise ValueError(c.view)


def _report(c, tag, em, el, cm, cl, ktot, bar, l2bar):
    print(f"[pixgemm] kind {c.kind:2d} {tag:5s} {c!r:75s} Ktot {ktot:6d}  max-norm {em:.2e} (cpu fp32 {cm:.2e}, bar {bar:.2e})"
          f"  rel-L2 {el:.2e} (cpu fp32 {cl:.2e}, bar {l2bar:.2e})")


def _assert_close(c, tag, got, ref64, ref32, ktot):
    em, el = _errs(got, ref64)
    cm, cl = _errs(ref32, ref64)
    bar = _bar(ktot)
    l2bar = R_L2 * max(cl, math.sqrt(ktot) * EPS / 8)
    _report(c, tag, em, el, cm, cl, ktot, bar, l2bar)
    assert em <= bar, f"{c} {tag}: max-norm rel error {em:.3e} > bar {bar:.3e} (cpu fp32 {cm:.3e})"
    assert el <= l2bar, f"{c} {tag}: rel-L2 error {el:.3e} > bar {l2bar:.3e} (cpu fp32 {cl:.3e})"


def _fwd_like(amd, c):
    """forward and data-gradient ops: GPU result (CPU fp32), float64 and fp32 references, the kinds that ran, extra checks"""
    ops, ep = amd.ops, c.ep
    N, Cin, Cout, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    fwd = c.op.startswith("fwd")
    # logical shapes: A operand, weight, output
    if c.op in ("fwd3", "fwd1"):
        a_shape, o_shape = (N, Cin, H, W), (N, Cout, H, W)
    elif c.op == "fwd3s2":
        a_shape, o_shape = (N, Cin, H, W), (N, Cout, (H + 1) // 2, (W + 1) // 2)
    elif c.op == "fwdT":
        a_shape, o_shape = (N, Cin, H, W), (N, Cout, 2 * H, 2 * W)
    elif c.op in ("dgrad3", "dgrad1"):
        a_shape, o_shape = (N, Cout, H, W), (N, Cin, H, W)
    elif c.op == "dgrad3s2":
        a_shape, o_shape = (N, Cout, (H + 1) // 2, (W + 1) // 2), (N, Cin, H, W)
    else:                                        # dgradT: dy on the 2x map
        a_shape, o_shape = (N, Cout, 2 * H, 2 * W), (N, Cin, H, W)
    k = 1 if c.op.endswith("1") else (6 if c.op.endswith("T") else 3)
    w_shape = (Cin, Cout, 6, 6) if c.op.endswith("T") else (Cout, Cin, k, k)
    X = _rand(a_shape, 1)
    Wt = _rand(w_shape, 2) / math.sqrt(w_shape[1] * k * k)
    b = _rand((Cout,), 3) if ep.get("bias") else None
    add = _rand(o_shape, 4) if ep.get("add") else None
    z = _rand(o_shape, 5) if ep.get("z") else None
    alpha, beta, act = ep.get("alpha", 1.0), ep.get("beta", 0.0), ep.get("act", 0)
    add_scale, post_scale = ep.get("add_scale", 1.0), ep.get("post_scale", 1.0)
    C_o = o_shape[1]
    old = _rand(o_shape, 6) if c.out == "slice" else None

    # references: alpha * op + bias + beta * old + add; act; z mask; (stride-2 forward: post_scale * a + add_scale * add)
    def ref(dt):
        v = _conv(c.op, dt, X, Wt, in_hw=(H, W)) * alpha
        if b is not None:
            v = v + b.to(dt).view(1, -1, 1, 1)
        if old is not None:
            v = v + beta * old.to(dt)
        if add is not None and c.op != "fwd3s2":
            v = v + add_scale * add.to(dt)
        v = _act(v, act)
        if z is not None:
            v = _zmask(v, z.to(dt))
        a = v
        if c.op == "fwd3s2":
            v = post_scale * v + (add_scale * add.to(dt) if add is not None else 0)
        return v, a

    keep = []
    xa, _, hold = _operand(c, X, 7)
    keep.append(hold)
    wd = Wt.cuda()
    if c.op in ("fwd3", "dgrad3", "fwd3s2", "dgrad3s2"):
        wd = ops.ohwi(wd)
    elif c.op.endswith("T"):
        wd = ops.convT_pack(wd)
    bd = b.cuda() if b is not None else None
    addd = _pm(add) if add is not None else None
    zd = _pm(z) if z is not None else None
    obuf = None
    if c.out == "slice":
        full = _rand((o_shape[0], C_o + 8) + o_shape[2:], 8)
        full[:, 4:4 + C_o] = old
        obuf = _pm(full)
        ref_full = obuf.clone()

    def out_arg():
        return obuf[:, 4:4 + C_o] if obuf is not None else None

    def run(o16=None):
        if c.op == "fwd3":
            if o16 is not None:
                return ops.conv3x3_fwd(xa, wd, bd, lrelu=act, alpha=alpha, out_dtype=o16)
            return ops.conv3x3_fwd(xa, wd, bd, lrelu=act, out=out_arg(), alpha=alpha, beta=beta)
        if c.op == "fwd1":
            assert beta == 0.0 or c.out == "fresh"
            return ops.conv1x1_fwd(xa, wd, bd, add=addd, add_scale=add_scale, alpha=alpha, out=out_arg(), act=act)
        if c.op == "fwd3s2":
            return ops.conv3x3s2_fwd(xa, wd, bd, act=act, add=addd, add_scale=add_scale, post_scale=post_scale, keep_act=bool(ep.get("keep_act")))
        if c.op == "fwdT":
            return ops.convT_fwd(xa, wd, bd, Cout, lrelu=act)
        if c.op == "dgrad3":
            return ops.conv3x3_dgrad(xa, wd, dx=out_arg(), alpha=alpha, beta=beta, z=zd)
        if c.op == "dgrad1":
            if o16 is not None:
                return ops.conv1x1_dgrad(xa, wd, alpha=alpha, out_dtype=o16)
            return ops.conv1x1_dgrad(xa, wd, dx=out_arg(), alpha=alpha, beta=beta)
        if c.op == "dgrad3s2":
            return ops.conv3x3s2_dgrad(xa, wd, (H, W), dx=out_arg(), alpha=alpha, beta=beta)
        if c.op == "dgradT":
            return ops.convT_dgrad(xa, wd, Cin, z=zd)
        raise ValueError(c.op)

    if c.view == "far":
        ext = _wk_a_extent_bytes(xa, a_shape[0], a_shape[2], a_shape[3], a_shape[1])
        if c.kind == 15:
            assert ext >= 0x7FFFFFF0, ext                               # wk_prepare refuses: the stream-K kernel runs
        if c.gap == GAP_2P31:
            assert xa.stride(0) * (a_shape[0] - 1) >= 1 << 31           # the last image lies past element 2^31
        print(f"[pixgemm] {c!r}: A view spans {ext / 2 ** 30:.2f} GiB (wk_prepare's limit: 2 GiB), "
              f"last image starts at element {xa.stride(0) * (a_shape[0] - 1)} (2^31 = {1 << 31})")
    res, ran = _profiled(run)
    _check_kind(c, ran)
    got, act_got = (res if isinstance(res, tuple) else (res, None))
    r64, a64 = ref(torch.float64)
    r32, a32 = ref(torch.float32)
    ktot = _ktot(c)
    _assert_close(c, "out", got.float().cpu(), r64, r32, ktot)
    if act_got is not None:
        _assert_close(c, "act", act_got.cpu(), a64, a32, ktot)
    if obuf is not None:                          # the channels on either side of the slice: bit-identical
        assert torch.equal(obuf[:, :4], ref_full[:, :4]) and torch.equal(obuf[:, 4 + C_o:], ref_full[:, 4 + C_o:]), f"{c}: neighbours written"
    if c.o16 is not None:                         # 2-byte output: the fp32 result of the same kernel, rounded once
        h, ran16 = _profiled(lambda: run(c.o16))
        _check_kind(c, ran16)
        assert h.dtype == c.o16
        assert torch.equal(h.cpu(), got.cpu().to(c.o16)), f"{c}: the 2-byte output is not the fp32 result rounded once"
    del keep


def _wgrad(amd, c, det):
    ops, ep = amd.ops, c.ep
    from afigan_amd import _lib
    N, Cin, Cout, H, W = c.N, c.Cin, c.Cout, c.H, c.W
    alpha = ep.get("alpha", 1.0)
    if c.op in ("wgrad3", "wgrad1"):
        x_shape, dy_shape = (N, Cin, H, W), (N, Cout, H, W)
    elif c.op == "wgrad3s2":
        x_shape, dy_shape = (N, Cin, H, W), (N, Cout, (H + 1) // 2, (W + 1) // 2)
    else:
        x_shape, dy_shape = (N, Cin, H, W), (N, Cout, 2 * H, 2 * W)
    x, dy = _rand(x_shape, 1), _rand(dy_shape, 2)
    xa, _, hold = _operand(c, x, 7)
    dyd = _pm(dy)
    dw0 = _rand((Cout, Cin, 3, 3), 3) if c.op in ("wgrad3", "wgrad3s2") else None

    def run():
        if c.op == "wgrad3":
            return ops.conv3x3_wgrad(dyd, xa, dw=ops.ohwi(dw0.cuda()).clone(memory_format=torch.preserve_format), alpha=alpha)
        if c.op == "wgrad3s2":
            return ops.conv3x3s2_wgrad(dyd, xa, dw=ops.ohwi(dw0.cuda()).clone(memory_format=torch.preserve_format), alpha=alpha)
        if c.op == "wgrad1":
            return ops.conv1x1_wgrad(dyd, xa, alpha=alpha).view(Cout, Cin, 1, 1)
        return ops.convT_wgrad(dyd, xa)

    def ref(dt):
        v = _conv(c.op, dt, (dy, x), None) * alpha
        return v + dw0.to(dt) if dw0 is not None else v

    cx = _lib.current_ctx()
    prev = cx.get_option("deterministic")
    cx.set_option("deterministic", det)
    try:
        got, ran = _profiled(run)
        _check_kind(c, ran)
        got = got.cpu()
        if det:
            again = run().cpu()
            assert torch.equal(got, again), f"{c}: two runs under deterministic = 1 differ"
    finally:
        cx.set_option("deterministic", prev)
    _assert_close(c, f"det{det}", got, ref(torch.float64), ref(torch.float32), _ktot(c))
    del hold


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_pix_gemm_kernel_vs_fp64(amd, case):
    _fwd_like(amd, case)


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=repr)
def test_wgrad_gemm_kernel_vs_fp64(amd, case, det):
    _wgrad(amd, case, det)


def test_table_covers_every_kind():
    """every pixel-GEMM and weight-gradient kind of the fp32 MFMA family is named by at least one case (host-only)"""
    named = {c.kind for c in CASES} | {c.kind for c in WGRAD_CASES}
    assert named >= {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15}, sorted(named)
    far = [c for c in CASES if c.view == "far"]
    assert any(c.kind == 15 and c.N == 2 and c.gap == GAP_2GB for c in far) and any(c.kind == 15 and c.gap == GAP_2P31 for c in far)
    assert any(c.kind != 15 and c.gap == GAP_2P31 for c in far)
