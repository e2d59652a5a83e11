"""Every Winograd conv form against a float64 reference, at bars derived from an fp32 restatement of the same form, with proof of which
GEMM ran.

The 3x3 / stride-1 convs with >= 128 channels on both sides run as  transform -> one batched GEMM over the transform points -> inverse
transform  (csrc/winograd.hip, the batched GEMMs of csrc/igemm.hip, afi_gemm_f16.h, afi_gemm_bf16.h; the form is decided by wino_form in
csrc/nets.hip).  Each case below names the entry point (afi_conv3x3_wino_fwd / _fwd_out16 / _infer / _dgrad / _wgrad), the shape, the
context's arithmetic and options, the views, the tiling it must take and the profiler kind its GEMM must run on (kKindNames, csrc/igemm.hip):

  13 / 17 / 21   batched NT GEMM (forward, data gradient): fp32 MFMA / bf16 MFMA (bf16x6, bf16x3, bf16) / f16x3.  Kind 21 holds two tile
                 sizes, told apart by the `split` column of afi_profile_dump: 2 = 128 x 128, 3 = 256 x 256 (AFI_OPT_F16_NT256_MIN_TILES)
  14 / 18 / 22   batched TN GEMM (weight gradient): fp32 / bf16 MFMA / f16x3 (f16x3 only where Cout % 128 == 0 and Cin % 128 == 0)
  0 / 2 / 3      shapes the batched NT GEMMs refuse (columns % 128 != 0 or K % 32 != 0) under EVERY arithmetic: the fp32 pixel GEMM over the
                 transform points as images, always in its KC form (U is transformed per direction, so a data gradient never takes the RC
                 kinds 4 .. 7): 128x32 tiles up to 32 columns (2), 64x64 tiles below 128 tiles of 128x128 (3), 128x128 linear tiles (0)
  8 / 9 / 10     shapes the batched TN GEMMs refuse (Cout % 128 != 0 or Cin % 128 != 0): the direct weight-gradient kernel with the
                 transform points as taps, by Cout: > 64 (8), <= 64 (9), <= 32 (10)
A case passes only if its named kind ran and no other GEMM kind did, and if the dump shows the tiling it names (16 or 36 planes).  The
expectations are stated in the table from wino_form and the launchers; nothing here mirrors their logic.

Every call goes through the C-ABI directly with a NaN-filled workspace and a NaN-filled output (weight gradients: a dw that holds other
data), so a padded tile row (T < Tpad), the K padding or a pixel that is read or left unwritten shows as a non-finite result.

Reference and bars: tests/wino_f64.py.  fp32, f16x3 and bf16x6 are held, per case and per norm (max-norm and relative L2), to
R_WINO = 4 x max(error of the fp32 restatement of the case's own tiling, sqrt(Ktot) 2^-24 / 8); bf16x3 and bf16 run the same code paths for
shape and edge coverage at the TOL_CONV of tests/test_gpu_bf16.py.

Exact properties: 2-byte outputs equal the fp32 output rounded once; deterministic weight gradients repeat bit for bit; scaling the
operands by 2^40 and 2^-30 scales the result by exactly 2^10 (the f16x3 scales and their exact inverses far from unit scale).

Not reached from here (they run only inside afi_discriminator_* / afi_generator_*): planes pre-split with a known maximum, the
k-step-local sums, kept input planes (tests/test_gpu_d_parity.py); the conv-transpose's four-phase gradients and the non-simple output
epilogue (the interpolator tests).

Exception, derived: kinds 14 and 18 under deterministic = 1.  With the strict bar these two failed at the two largest F(3x3,2x2) reductions of
the table (1x128->128x91x91 with winograd_f4_backward = 0, Ktot = 2116, and 1x128->128x90x91, Ktot = 2070): max-norm 2.08e-6 / 2.14e-6 (fp32)
and 2.30e-6 / 1.99e-6 (bf16x6) against a restatement at 5.07e-7 / 4.87e-7, i.e. x4.1 .. x4.5 where R_WINO allows x4; rel. L2 x2.7 .. x3.1, inside
its bar.  Cause, from afi_launch_gemm_tn / afi_launch_gemm_tn_bf16 (csrc/igemm.hip): deterministic = 1 sets splitK = 1, so one block sums ALL
Ktot tiles of a dU element in ONE sequential fp32 accumulator chain (the fp32 MFMA is an fmaf chain; bf16x6 adds its six products per k-step
to the same accumulator).  A chain of K roundings at the accumulator's magnitude walks ~ c sqrt(K) 2^-24 of it: sqrt(2116) 2^-24 = 2.7e-6, the
kernels sit at 0.75 .. 0.85 of that -- where the deterministic direct weight gradient of tests/test_gpu_pixgemm.py sits (1.06).  The yardstick
does not grow with it: torch.bmm sums in blocks and stays at 5e-7 for every Ktot, so the ratio grows like sqrt(Ktot) (x1.6 at 272, x4.5 at
2116) with nothing wrong in the kernel; under deterministic = 0 the same shapes split Ktot over blocks and measure x1.2 .. x1.5.  These two
kinds under deterministic = 1 are therefore held in MAX-NORM to max(R_WINO x restatement, C_MAX_CHAIN sqrt(Ktot) 2^-24) with C_MAX_CHAIN = 2 =
C_MAX of test_gpu_pixgemm.py (5.5e-6 at Ktot = 2116; today's bar there: 1e-4), and in rel. L2 to the strict bar.  Every other form -- kind 22
(f16x3: x3.3 at most), the fallbacks 8 / 9 / 10, and everything under deterministic = 0 -- stays on the strict bar.

Measured on MI355X, per kind the case closest to its max-norm bar: kernel error / fp32 restatement's (ratio), Ktot.  Over all fp32-grade cases
the kernels sit at 0.5 .. 2.5x the restatement in max-norm (but the exception above: 4.5x) and at <= 3.1x in rel. L2 (that maximum: kind 14,
deterministic = 1, Ktot = 2116; every forward and data gradient <= 1.4x).
  forward / inference / data gradient                          weight gradient        deterministic = 0              deterministic = 1
  13     F2 4.78e-7 / 4.31e-7 (1.11)  F4 4.85e-6 / 2.63e-6 (1.85, K 256)    14  F2 8.15e-7 / 5.05e-7 (1.61)    2.14e-6 / 4.87e-7 (4.40, K 2070)
  17     F2 3.53e-7 / 3.59e-7 (0.98)  F4 4.16e-6 / 2.74e-6 (1.52, K 256)        F4 3.77e-6 / 2.39e-6 (1.58)    6.08e-6 / 2.61e-6 (2.33, K 700)
  21/s2  F2 3.49e-7 / 4.36e-7 (0.80)  F4 3.21e-6 / 2.74e-6 (1.17, K 256)    18  F2 8.59e-7 / 4.64e-7 (1.85)    2.30e-6 / 5.07e-7 (4.53, K 2116)
  21/s3  F2 2.61e-7 / 3.30e-7 (0.79)  F4 1.38e-6 / 2.65e-6 (0.52)               F4 5.85e-6 / 2.39e-6 (2.45)    5.85e-6 / 2.39e-6 (2.45, K 529)
  0      F2 5.80e-7 / 5.36e-7 (1.08)  F4 2.76e-6 / 2.45e-6 (1.13)           22  F2 7.53e-7 / 5.07e-7 (1.49)    1.68e-6 / 5.07e-7 (3.32, K 2116)
  2      F2 1.70e-7 / 1.86e-7 (0.92)                                            F4 3.39e-6 / 2.39e-6 (1.42)    3.39e-6 / 2.39e-6 (1.42, K 529)
  3      F2 7.23e-7 / 4.32e-7 (1.67, K 256)                                 8   F2 5.58e-7 / 5.83e-7 (0.96)    8.60e-7 / 5.83e-7 (1.47)
  one dominant element (f16x3, F2): all pixels 7.43e-7 / 7.65e-7 (0.97);        F4 2.82e-6 / 4.63e-6 (0.61)    4.54e-6 / 4.63e-6 (0.98)
    outside its footprint 2.94e-7 / 4.51e-7 (0.65): inside the bar          9   F2 5.00e-7 / 5.45e-7 (0.92)    7.10e-7 / 5.45e-7 (1.30)
  weight cache, every step <= 1.1x; accumulator sums <= 1.84x (bf16x6, F4)  10  F2 1.96e-7 / 1.88e-7 (1.04)    1.96e-7 / 1.88e-7 (1.04)
So F(4x4) rounds at 3e-6 .. 6e-6 of the output scale (not the ~3e-5 once quoted), F(2x2) at 3e-7 .. 9e-7.

What the bars catch (scratch builds of the library with ONE arithmetic value changed, never committed; the whole file run against each):
  the lo_a x hi_b MFMA of the 128 x 128 f16x3 NT kernel left out   every fp64 case on kind 21 / split 2 (33 of 33: errors 1.4e-4 .. 2.3e-3),
                                                                   the dominant-element test, the weight-cache sequence; nothing else
  G of F(4x4): 1/15 -> 1/16 (wino4_g3, row 4)                      every F(4x4) inference and data-gradient case under every arithmetic, both
                                                                   tile sizes and the fallback (42 of 42: 2.5e-2 .. 4.8e-2), the weight-cache
                                                                   sequence (G' of the weight gradient is a separate function: untouched)
  A^T of F(4x4): y3's 0.125 -> 0.25 (wino4_at)                     the same 42 cases (2.3e-1 .. 3.8e-1) and the weight-cache sequence
  bf16x6 NT kernel: its lo_a x hi_b term left out                  every fp64 case on kind 17 under bf16x6 (31 of 31: 1.7e-6 .. 2.8e-5: the
                                                                   smallest 1.5x over its bar, which today's 1e-4 passed), the weight-cache sequence
The 2-byte and power-of-two tests compare a kernel with itself and pass under all four, as they must; no defect passed every case.
"""
import csv
import ctypes as C
import math

import pytest
import torch

import wino_f64 as wf

pytestmark = pytest.mark.gpu

NAN = float("nan")
LRELU = 0.2
NT_BATCHED, TN_BATCHED = (13, 17, 21), (14, 18, 22)
NT_FALLBACK, TN_FALLBACK = (0, 2, 3), (8, 9, 10)
ENTRY = {"fwd": "afi_conv3x3_wino_fwd", "fwd16": "afi_conv3x3_wino_fwd_out16", "infer": "afi_conv3x3_wino_infer",
         "dgrad": "afi_conv3x3_wino_dgrad", "wgrad": "afi_conv3x3_wino_wgrad"}
OP_OF = {"fwd": "fwd", "fwd16": "fwd", "infer": "fwd", "dgrad": "dgrad", "wgrad": "wgrad"}
C_MAX_CHAIN = 2.0               # C_MAX of tests/test_gpu_pixgemm.py: the max-norm bar of ONE sequential fp32 chain of Ktot terms (module docstring)
CHAIN_KINDS = (14, 18)          # ... which only the fp32 and bf16 batched TN GEMMs under deterministic = 1 are held to (module docstring)
NEVER = 10 ** 9                 # f16_nt256_min_tiles: a tile count no shape reaches


# ------------------------------------------------------------------------------------------------ case table
class Case:
    """ep: the entry point (ENTRY).  N, Cin, Cout, H, W: the conv (every op lives on the H x W map).  dtype: the context's arithmetic.
    tiling: 2 = F(2x2,3x3) / F(3x3,2x2), 4 = F(4x4,3x3) / F(3x3,4x4).  kind: the profiler kind of the GEMM; split: for kind 21, the tile
    form afi_profile_dump must show.  opts: context options for the call (names of afigan_amd/_lib.py).
    view: how the operand is handed over -- dense, crop (a corner of a larger map), cslice (channels 4.. of a wider buffer), and for weight
    gradients crop_slice (a cropped x together with a sliced dy).  out: fresh, or slice (channels 4.. of a wider buffer that holds other data:
    the neighbours must stay bit-identical).  bias / act / z / alpha: epilogue terms; o16: the 2-byte dtype of _fwd_out16."""

    def __init__(self, ep, N, Cin, Cout, H, W, dtype, tiling, kind, split=None, opts=None, view="dense", out="fresh", o16=None, bias=0, act=0,
                 z=0, alpha=1.0):
        self.ep, self.N, self.Cin, self.Cout, self.H, self.W = ep, N, Cin, Cout, H, W
        self.dtype, self.tiling, self.kind, self.split, self.opts = dtype, tiling, kind, split, dict(opts or {})
        self.view, self.out, self.o16, self.bias, self.act, self.z, self.alpha = view, out, o16, bias, act, z, alpha

    @property
    def op(self):
        return OP_OF[self.ep]

    @property
    def shape(self):
        return (self.N, self.Cin, self.Cout, self.H, self.W)

    def __repr__(self):
        e = "".join(f",{k}={v}" for k, v in (("bias", self.bias), ("act", self.act), ("z", self.z)) if v)
        e += f",alpha={self.alpha}" if self.alpha != 1.0 else ""
        e += "".join(f",{k}={v}" for k, v in sorted(self.opts.items()))
        e += f",{str(self.o16)[6:]}" if self.o16 else ""
        s = f"/s{self.split}" if self.split is not None else ""
        return (f"{self.ep}-{self.dtype}-N{self.N}-{self.Cin}to{self.Cout}-{self.H}x{self.W}-F{self.tiling}-k{self.kind}{s}-{self.view}-{self.out}{e}")


def _x3(ep, N, Cin, Cout, H, W, tiling, kinds, **kw):
    """one case per fp32-grade arithmetic; kinds = the expected profiler kinds under (fp32, f16x3, bf16x6).  Kind 21 runs on its 128 x 128
    tile (split 2) unless the case says otherwise: no shape of this file reaches the default AFI_OPT_F16_NT256_MIN_TILES = 512"""
    out = []
    for dt, k in zip(wf.FP32_GRADE, kinds):
        kk = dict(kw)
        if k == 21:
            kk.setdefault("split", 2)
        out.append(Case(ep, N, Cin, Cout, H, W, dt, tiling, k, **kk))
    return out


A1 = (1, 128, 128, 33, 31)      # F(2x2) aligned: T = 272, Tpad = 384
A2 = (2, 160, 256, 21, 27)      # F(2x2) aligned, K % 32 == 0 only, columns % 256 == 0: T = 308, Tpad = 384; a 128-row GEMM tile straddles the images
A2T = (2, 256, 160, 21, 27)     # its data gradient is the aligned one (K = 160, columns 256); that of A2 has 160 columns: fallback
NA1 = (1, 132, 160, 33, 31)     # columns % 128 != 0: 96 tiles of 128x128 -> the 64x64 pixel GEMM
NA2 = (2, 20, 8, 8, 6)          # the smallest: <= 32 columns -> the 128x32 pixel GEMM
NA3 = (1, 132, 160, 45, 45)     # T = 529, Tpad = 640: 160 tiles of 128x128 -> the linear 128x128 pixel GEMM
NA4 = (1, 132, 64, 33, 31)      # weight gradient with Cout = 64 rows
F4A = (1, 128, 128, 91, 91)     # 8281 pixels: F(4x4), last tile row and column three-quarters empty, T = 529, Tpad = 640
F4B = (2, 128, 256, 64, 65)     # 8320 pixels: F(4x4), columns % 256 == 0, T = 544, Tpad = 640, tiles straddle the images
F4N = (1, 132, 160, 91, 91)     # F(4x4) on the non-aligned fallbacks: 36 x 640 rows -> the linear 128x128 pixel GEMM
UND = (1, 128, 128, 90, 91)     # 8190 pixels: just under the F(4x4) threshold
D1 = (1, 128, 128, 3, 400)      # degenerate maps: two tile rows, the second half empty
D2 = (1, 128, 128, 1100, 1)     # one column
D3 = (1, 128, 128, 3, 2800)     # 8400 pixels: F(4x4) with a single tile row
NT, TN = (13, 21, 17), (14, 22, 18)
F2_ONLY = {"winograd_f4_backward": 0}

FWD_CASES = (
    _x3("fwd", *A1, 2, NT, bias=1) + _x3("fwd", *A1, 2, NT, view="crop") + _x3("fwd", *A2, 2, NT, bias=1, view="cslice")
    + _x3("fwd", *A2, 2, NT, out="slice") + _x3("fwd", *NA1, 2, (3, 3, 3), bias=1) + _x3("fwd", *NA2, 2, (2, 2, 2), bias=1, view="crop")
    + _x3("fwd", *NA3, 2, (0, 0, 0), out="slice") + _x3("fwd", *D1, 2, NT, bias=1) + _x3("fwd", *D2, 2, NT)
    + _x3("fwd", *F4A, 2, NT, bias=1)                                       # a forward a backward may follow never takes F(4x4)
    + [Case("fwd", *A1, "bf16x3", 2, 17, bias=1), Case("fwd", *A1, "bf16", 2, 17, bias=1)]
    # f16x3 NT tile choice at a 256-column shape: the 256 x 256 tile when asked for, the 128 x 128 tile otherwise
    + [Case("fwd", *A2, "f16x3", 2, 21, split=3, opts={"f16_nt256_min_tiles": 1}, bias=1),
       Case("fwd", *A2, "f16x3", 2, 21, split=2, opts={"f16_nt256_min_tiles": NEVER}, bias=1)]
)
INFER_CASES = (
    _x3("infer", *F4A, 4, NT, bias=1, act=0) + _x3("infer", *F4A, 4, NT, bias=1, act=1) + _x3("infer", *F4A, 4, NT, act=2)
    + _x3("infer", *F4B, 4, NT, bias=1, act=1, view="crop") + _x3("infer", *F4B, 4, NT, act=2, out="slice", view="cslice")
    + _x3("infer", *F4N, 4, (0, 0, 0), bias=1, act=1)
    + _x3("infer", *A1, 2, NT, bias=1, act=2) + _x3("infer", *A1, 2, NT, bias=1, act=1) + _x3("infer", *A2, 2, NT, act=0)
    + _x3("infer", *NA1, 2, (3, 3, 3), bias=1, act=1)
    + _x3("infer", *UND, 2, NT, bias=1, act=1) + _x3("infer", *D1, 2, NT, act=1) + _x3("infer", *D2, 2, NT, bias=1) + _x3("infer", *D3, 4, NT, bias=1, act=2)
    + _x3("infer", *F4A, 2, NT, opts=F2_ONLY, bias=1, act=1)
    + [Case("infer", *F4A, "bf16x3", 4, 17, bias=1, act=1),
       Case("infer", *F4A, "bf16", 2, 17, bias=1, act=1)]                   # 8-bit operands cannot carry the F(4x4) transforms: stays on F(2x2)
    + [Case("infer", *F4B, "f16x3", 4, 21, split=3, opts={"f16_nt256_min_tiles": 1}, bias=1, act=1),
       Case("infer", *F4B, "f16x3", 4, 21, split=2, opts={"f16_nt256_min_tiles": NEVER}, bias=1, act=1)]
)
DGRAD_CASES = (
    _x3("dgrad", *F4A, 4, NT) + _x3("dgrad", *F4A, 4, NT, z=1) + _x3("dgrad", *F4A, 2, NT, opts=F2_ONLY, z=1)
    + _x3("dgrad", *F4B, 4, NT, z=1, view="cslice") + _x3("dgrad", *F4B, 4, NT, out="slice") + _x3("dgrad", *F4N, 4, (0, 0, 0), z=1)
    + _x3("dgrad", *A1, 2, NT, z=1) + _x3("dgrad", *A2, 2, (3, 3, 3), view="crop") + _x3("dgrad", *A2T, 2, NT, view="crop") + _x3("dgrad", *NA1, 2, (3, 3, 3), z=1)
    + _x3("dgrad", *NA2, 2, (2, 2, 2)) + _x3("dgrad", *NA3, 2, (0, 0, 0), z=1)
    + _x3("dgrad", *UND, 2, NT) + _x3("dgrad", *D1, 2, NT, z=1) + _x3("dgrad", *D2, 2, NT) + _x3("dgrad", *D3, 4, NT, z=1)
    + [Case("dgrad", *A1, "bf16x3", 2, 17, z=1), Case("dgrad", *A1, "bf16", 2, 17, z=1)]
)
WGRAD_CASES = (
    _x3("wgrad", *A1, 2, TN, alpha=0.5) + _x3("wgrad", *A1, 2, TN, view="crop_slice") + _x3("wgrad", *A2, 2, (8, 8, 8), alpha=0.5)
    + _x3("wgrad", *NA1, 2, (8, 8, 8), alpha=2.0) + _x3("wgrad", *NA2, 2, (10, 10, 10), alpha=0.5) + _x3("wgrad", *NA4, 2, (9, 9, 9))
    + _x3("wgrad", *F4A, 4, TN, alpha=0.5) + _x3("wgrad", *F4A, 4, TN) + _x3("wgrad", *NA2, 2, (10, 10, 10)) + _x3("wgrad", *F4A, 2, TN, opts=F2_ONLY, alpha=0.5)
    + _x3("wgrad", *F4B, 4, TN, alpha=0.25, view="crop_slice") + _x3("wgrad", *F4N, 4, (8, 8, 8), alpha=0.5)
    + _x3("wgrad", *UND, 2, TN) + _x3("wgrad", *D1, 2, TN, alpha=0.5) + _x3("wgrad", *D2, 2, TN) + _x3("wgrad", *D3, 4, TN, alpha=0.5)
    + [Case("wgrad", *A1, "bf16x3", 2, 18, alpha=0.5), Case("wgrad", *A1, "bf16", 2, 18, alpha=0.5)]
)
O16_CASES = [
    Case("fwd16", *A1, "f16x3", 2, 21, split=2, o16=torch.bfloat16, bias=1), Case("fwd16", *A1, "f16x3", 2, 21, split=2, o16=torch.float16, bias=1),
    Case("fwd16", *A1, "bf16x6", 2, 17, o16=torch.float16), Case("fwd16", *A1, "fp32", 2, 13, o16=torch.bfloat16, bias=1),
    Case("fwd16", *NA1, "f16x3", 2, 3, o16=torch.bfloat16, bias=1), Case("fwd16", *NA1, "bf16x6", 2, 3, o16=torch.float16, bias=1),
]
ALL_CASES = FWD_CASES + INFER_CASES + DGRAD_CASES + WGRAD_CASES + O16_CASES
# the forms of the issue's list: (entry point, tiling, aligned / fallback GEMM), each under every fp32-grade arithmetic
FORMS = [(ep, t, fam) for ep in ("fwd", "infer", "dgrad", "wgrad") for t in (2, 4) for fam in ("batched", "fallback") if not (ep == "fwd" and t == 4)]


def form_of(c):
    return (c.ep, c.tiling, "batched" if c.kind in NT_BATCHED + TN_BATCHED else "fallback")


# ------------------------------------------------------------------------------------------------ GPU side
@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _pm(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _operand(view, X, seed):
    """(GPU view handed to the op, keep-alive) of the logical CPU tensor X"""
    N, C_, H, W = X.shape
    if view == "dense":
        return _pm(X), None
    if view == "crop":
        big = _rand((N, C_, H + 3, W + 2), seed)
        big[:, :, :H, :W] = X
        g = _pm(big)
        return g[:, :, :H, :W], g
    if view == "cslice":
        big = _rand((N, C_ + 8, H, W), seed)
        big[:, 4:4 + C_] = X
        g = _pm(big)
        return g[:, 4:4 + C_], g
    raise ValueError(view)


def _profiled(fn, dump_path):
    """run fn() with the launch profiler on: ({kind: launches}, [(kind, rows, cols, k, split, planes)] of afi_profile_dump)"""
    from afigan_amd import _lib
    lib = _lib.load()
    names = {lib.afi_profile_kind_name(k).decode(): k for k in range(lib.afi_profile_num_kinds())}
    _lib.check(lib.afi_profile_enable(1), "afi_profile_enable")
    try:
        fn()
        torch.cuda.synchronize()
        ran, buf = {}, (C.c_double * 3)()
        for k in range(lib.afi_profile_num_kinds()):
            _lib.check(lib.afi_profile_get(k, buf), "afi_profile_get")
            if buf[0]:
                ran[k] = int(buf[0])
        _lib.check(lib.afi_profile_dump(str(dump_path).encode()), "afi_profile_dump")
    finally:
        lib.afi_profile_enable(0)
    with open(dump_path, newline="") as f:
        rows = [(names[r["kind"]], int(r["rows"]), int(r["cols"]), int(r["k"]), int(r["split"]), int(r["planes"])) for r in csv.DictReader(f)]
    return ran, rows


def _check_form(c, ran, rows):
    """the named kind ran alone, on the tiling and (kind 21) the tile form the case names"""
    assert set(ran) == {c.kind} and ran[c.kind] == 1, f"{c}: expected one launch of kind {c.kind} alone, the profiler saw {ran}"
    (kind, m, n, k, split, planes), = rows
    np_ = (c.tiling + 2) ** 2
    tpad = (wf.tiles(c.tiling, c.N, c.H, c.W) + 127) // 128 * 128
    if c.kind in NT_BATCHED + TN_BATCHED:
        assert planes == np_, f"{c}: expected {np_} transform points, the dump shows {planes}"
    elif c.kind in NT_FALLBACK:
        assert m == np_ * tpad, f"{c}: expected {np_} x {tpad} GEMM rows, the dump shows {m}"
    else:
        assert m == np_ * c.Cout, f"{c}: expected {np_} taps x {c.Cout} rows, the dump shows {m}"
    if c.kind == 21:
        assert c.split is not None and split == c.split, f"{c}: expected tile form {c.split}, the dump shows {split}"


class _Options:
    """the context's arithmetic and options for a block, restored on exit"""

    def __init__(self, amd, dtype, opts):
        self.amd, self.dtype, self.opts = amd, dtype, opts

    def __enter__(self):
        from afigan_amd import _lib
        self.cd = self.amd.compute_dtype(self.dtype)
        self.cx = self.cd.__enter__()
        assert self.cx is _lib.current_ctx()
        self.prev = {k: self.cx.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.cx.set_option(k, v)
        return self.cx

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.cx.set_option(k, v)
        return self.cd.__exit__(*exc)


def _act(v, a):
    if a == 1:
        return torch.where(v > 0, v, v * LRELU)
    if a == 2:
        return torch.clamp_min(v, 0)
    return v


def _workspace(lib, c):
    n = lib.afi_conv3x3_wino_ws_floats(c.N, c.H, c.W, c.Cin, c.Cout)
    return torch.full((int(n),), NAN, device="cuda"), n


def _expected(c, lin, terms):
    """the case's epilogue on a linear result `lin` (the float64 reference or the fp32 restatement), in lin's dtype"""
    dt = lin.dtype
    v = lin
    if c.op == "wgrad":
        return terms["dw0"].to(dt) + c.alpha * v
    if terms.get("bias") is not None:
        v = v + terms["bias"].to(dt).view(1, -1, 1, 1)
    v = _act(v, c.act)
    if terms.get("z") is not None:
        zz = terms["z"].to(dt)
        v = v * torch.where(zz > 0, torch.ones_like(zz), torch.full_like(zz, LRELU))
    return v


def _launch(amd, c, a, b, terms, keep):
    """a callable that issues the case's one library call on fresh NaN-filled scratch, and a callable that returns its result (GPU tensor)"""
    from afigan_amd import _lib
    ops, lib = amd.ops, _lib.load()
    N, Cin, Cout, H, W = c.shape
    ws, n = _workspace(lib, c)
    st = ops.stream_ptr
    if c.op == "wgrad":
        xv, k1 = _operand("crop" if c.view == "crop_slice" else c.view, a, 7)
        dyv, k2 = _operand("cslice" if c.view == "crop_slice" else "dense", b, 8)
        keep += [k1, k2]
        dw0 = ops.ohwi(terms["dw0"].cuda()).clone(memory_format=torch.preserve_format)
        state = {"dw": None}

        def run():
            state["dw"] = dw0.clone(memory_format=torch.preserve_format)
            ws.fill_(NAN)
            _lib.call(ENTRY[c.ep], ops.view_of(dyv), ops.view_of(xv), N, H, W, Cout, Cin, ops._p(state["dw"]), float(c.alpha), ops._p(ws), n, st())
        return run, lambda: state["dw"]
    C_o = Cin if c.op == "dgrad" else Cout
    av, k1 = _operand(c.view, a, 7)
    keep.append(k1)
    wd = ops.ohwi(b.cuda())
    bd = terms["bias"].cuda() if terms.get("bias") is not None else None
    zd = _pm(terms["z"]) if terms.get("z") is not None else None
    full = None
    if c.out == "slice":
        full = _pm(_rand((N, C_o + 8, H, W), 9))
        ref_full = full.clone()
        out = full[:, 4:4 + C_o]
    else:
        out = ops.new_pixel_major(N, C_o, H, W, "cuda", dtype=c.o16 or torch.float32)
    out.fill_(NAN)
    keep += [wd, bd, zd, full]

    def run():
        ws.fill_(NAN)
        if c.ep == "fwd":
            _lib.call(ENTRY[c.ep], ops.view_of(av), N, H, W, Cin, ops._p(wd), ops._p(bd), Cout, ops.view_of(out), ops._p(ws), n, st())
        elif c.ep == "fwd16":
            _lib.call(ENTRY[c.ep], ops.view_of(av), N, H, W, Cin, ops._p(wd), ops._p(bd), Cout, ops.view_of(out), ops.STORE_DTYPES[c.o16], ops._p(ws), n, st())
        elif c.ep == "infer":
            _lib.call(ENTRY[c.ep], ops.view_of(av), N, H, W, Cin, ops._p(wd), ops._p(bd), Cout, ops.view_of(out), int(c.act), ops._p(ws), n, st())
        else:
            _lib.call(ENTRY[c.ep], ops.view_of(av), N, H, W, Cout, ops._p(wd), Cin, ops.view_of(out),
                      ops.view_of(zd) if zd is not None else ops._NULL_VIEW, ops._p(ws), n, st())

    def result():
        if full is not None:                      # the channels on either side of the slice: bit-identical
            assert torch.equal(full[:, :4], ref_full[:, :4]) and torch.equal(full[:, 4 + C_o:], ref_full[:, 4 + C_o:]), f"{c}: neighbours written"
        return out
    return run, result


def _terms(c):
    N, Cin, Cout, H, W = c.shape
    if c.op == "wgrad":
        # alpha == 1: into a zeroed dw (the error is that of the gradient alone); alpha != 1: added into a dw that holds other data
        return {"dw0": torch.zeros((Cout, Cin, 3, 3)) if c.alpha == 1.0 else _rand((Cout, Cin, 3, 3), 5)}
    C_o = Cin if c.op == "dgrad" else Cout
    return {"bias": _rand((Cout,), 3) if c.bias else None, "z": _rand((N, C_o, H, W), 4) if c.z else None}


def _report(c, tag, em, el, rm, rl, k, bm, bl):
    print(f"[wino] {c!r:100s} {tag:5s} Ktot {k:5d}  max-norm {em:.2e} (restated {rm:.2e}, x{em / max(rm, 1e-300):.2f}, bar {bm:.2e})"
          f"  rel-L2 {el:.2e} (restated {rl:.2e}, x{el / max(rl, 1e-300):.2f}, bar {bl:.2e})")


def _assert_close(c, tag, got, ref64, rest32, k, chain=False):
    """got (CPU) against the float64 reference at the case's bar; rest32: the fp32 restatement of the same expression.
    chain: kinds 14 / 18 under deterministic = 1 (the exception derived in the module docstring: max-norm only, rel. L2 stays at R_WINO)"""
    assert torch.isfinite(got).all(), f"{c} {tag}: non-finite values in the result (something unwritten was read, or a pixel was left unwritten)"
    em, el = wf.errors(got, ref64)
    rm, rl = wf.errors(rest32, ref64)
    if c.dtype in wf.FP32_GRADE:
        bm, bl = wf.bars((rm, rl), k)
        if chain:
            bm = max(bm, C_MAX_CHAIN * math.sqrt(k) * wf.EPS)
    else:
        bm = bl = wf.TOL_CONV[c.dtype]
    _report(c, tag, em, el, rm, rl, k, bm, bl)
    assert em <= bm, f"{c} {tag}: max-norm rel error {em:.3e} > bar {bm:.3e} (fp32 restatement {rm:.3e})"
    assert el <= bl, f"{c} {tag}: rel-L2 error {el:.3e} > bar {bl:.3e} (fp32 restatement {rl:.3e})"
    return em, el


def _run_case(amd, c, tmp_path, det=0):
    a, b, ref, rest = wf.yardstick(c.op, c.tiling, *c.shape)
    terms, keep = _terms(c), []
    k = wf.ktot(c.op, c.tiling, *c.shape)
    opts = dict(c.opts, deterministic=det) if c.op == "wgrad" else c.opts
    with _Options(amd, c.dtype, opts):
        run, result = _launch(amd, c, a, b, terms, keep)
        ran, rows = _profiled(run, tmp_path / "dump.csv")
        _check_form(c, ran, rows)
        got = result().float().cpu()
        if c.op == "wgrad" and det:
            run()
            assert torch.equal(result().cpu(), got), f"{c}: two runs under deterministic = 1 differ"
    _assert_close(c, f"det{det}" if c.op == "wgrad" else "out", got, _expected(c, ref, terms), _expected(c, rest, terms), k, chain=det == 1 and c.kind in CHAIN_KINDS)
    del keep


@pytest.mark.parametrize("case", FWD_CASES + INFER_CASES + DGRAD_CASES, ids=repr)
def test_wino_conv_vs_fp64(amd, case, tmp_path):
    _run_case(amd, case, tmp_path)


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=repr)
def test_wino_wgrad_vs_fp64(amd, case, det, tmp_path):
    _run_case(amd, case, tmp_path, det)


@pytest.mark.parametrize("case", O16_CASES, ids=repr)
def test_wino_fwd_out16_is_the_fp32_output_rounded_once(amd, case, tmp_path):
    c = case
    a, b, _, _ = wf.yardstick("fwd", 2, *c.shape)
    terms, keep = _terms(c), []
    c32 = Case("fwd", *c.shape, c.dtype, c.tiling, c.kind, split=c.split, bias=c.bias)
    with _Options(amd, c.dtype, {}):
        run32, res32 = _launch(amd, c32, a, b, terms, keep)
        run32()
        run16, res16 = _launch(amd, c, a, b, terms, keep)
        ran, rows = _profiled(run16, tmp_path / "dump.csv")
        _check_form(c, ran, rows)
        y32, y16 = res32().cpu(), res16().cpu()
    assert y16.dtype == c.o16 and torch.isfinite(y32).all()
    assert torch.equal(y16, y32.to(c.o16)), f"{c}: the 2-byte output is not the fp32 result rounded once"


# ------------------------------------------------------------------------------------------------ exact properties
SCALE_CASES = (_x3("fwd", *A1, 2, NT) + _x3("fwd", *NA1, 2, (3, 3, 3)) + _x3("infer", *F4A, 4, NT) + _x3("dgrad", *A2T, 2, NT) + _x3("dgrad", *F4A, 4, NT)
               + _x3("wgrad", *A1, 2, TN) + _x3("wgrad", *F4A, 4, TN) + _x3("wgrad", *NA1, 2, (8, 8, 8)))


@pytest.mark.parametrize("case", SCALE_CASES, ids=repr)
def test_wino_power_of_two_scaling_is_exact(amd, case):
    """x 2^40 and w 2^-30 (dy and w; dy and x): the result is the unscaled result times 2^10, bit for bit -- every transform constant, every
    rounding and the f16x3 operand scales (afi_f16_scale from afi_f16_bound, and the exact 1 / s of the epilogue) commute with a power of two
    while nothing leaves fp32's normal range.  No bias; weight gradients into a zeroed dw under deterministic = 1."""
    c = case
    a, b, _, _ = wf.yardstick(c.op, c.tiling, *c.shape)
    terms = {"dw0": torch.zeros((c.Cout, c.Cin, 3, 3))} if c.op == "wgrad" else {}
    sa, sb = (2.0 ** -30, 2.0 ** 40) if c.op == "wgrad" else (2.0 ** 40, 2.0 ** -30)      # (wgrad operands: a = x, b = dy)
    keep = []
    with _Options(amd, c.dtype, {"deterministic": 1} if c.op == "wgrad" else {}):
        run1, res1 = _launch(amd, c, a, b, terms, keep)
        run1()
        y1 = res1().cpu().clone()
        run2, res2 = _launch(amd, c, a * sa, b * sb, terms, keep)
        run2()
        y2 = res2().cpu()
    assert torch.isfinite(y1).all() and torch.isfinite(y2).all()
    same = torch.equal(y2, y1 * 2.0 ** 10)
    if not same:
        print(f"[wino] {c!r}: scaled / unscaled differ, max-norm {wf.errors(y2, y1.double() * 2.0 ** 10)[0]:.3e}")
    assert same, f"{c}: the result of the scaled operands is not 2^10 times the unscaled result bit for bit"


def test_wino_one_dominant_element(amd, tmp_path):
    """x = randn with ONE element of 1e4, F(2x2) under f16x3 (the plane-wide operand scale follows that element: the case the design
    accepts).  The whole output holds the max-norm bar against max|ref|; the pixels outside the element's 3x3 footprint, whose
    values the element does not enter, hold R_WINO x the restatement's error on those pixels (both norms)."""
    c = Case("fwd", *A1, "f16x3", 2, 21, split=2)
    N, Cin, Cout, H, W = c.shape
    x, w = wf.inputs("fwd", *c.shape)
    x = x.clone()
    y0, x0 = 10, 11
    x[0, 5, y0, x0] = 1e4
    ref, rest = wf.reference("fwd", x, w), wf.restate("fwd", 2, x, w, torch.float32)
    keep = []
    with _Options(amd, c.dtype, {}):
        run, result = _launch(amd, c, x, w, {}, keep)
        ran, rows = _profiled(run, tmp_path / "dump.csv")
        _check_form(c, ran, rows)
        got = result().cpu()
    assert torch.isfinite(got).all()
    em, el = wf.errors(got, ref)
    rm, rl = wf.errors(rest, ref)
    print(f"[wino] dominant element, all pixels: max-norm {em:.2e} (restated {rm:.2e}, x{em / rm:.2f})  rel-L2 {el:.2e} (restated {rl:.2e}, x{el / rl:.2f})")
    assert em <= wf.bars((rm, rl), Cin)[0]
    outside = torch.ones((H, W), dtype=torch.bool)
    outside[y0 - 1:y0 + 2, x0 - 1:x0 + 2] = False
    eo, ro = wf.errors(got[:, :, outside], ref[:, :, outside]), wf.errors(rest[:, :, outside], ref[:, :, outside])
    bo = wf.bars(ro, Cin)
    print(f"[wino] dominant element, outside its footprint: max-norm {eo[0]:.2e} (restated {ro[0]:.2e}, x{eo[0] / ro[0]:.2f}, bar {bo[0]:.2e})"
          f"  rel-L2 {eo[1]:.2e} (restated {ro[1]:.2e}, x{eo[1] / ro[1]:.2f}, bar {bo[1]:.2e})")
    assert eo[0] <= bo[0] and eo[1] <= bo[1], f"outside the footprint: {eo} > {bo}"


def test_wino_weight_cache_across_arithmetics_and_tilings(amd):
    """One weight buffer (Cin == Cout: the two directions differ in nothing but the key) through f16x3, bf16x6, fp32 and f16x3 forwards, an
    F(4x4) inference call and a data gradient with a cache registered, each within its bar; then invalidate, other weights, and all of it
    again: a transform or pre-split image served under the wrong key, or a stale one, misses every bar."""
    from afigan_amd import _lib
    ops, lib = amd.ops, _lib.load()
    cache = torch.full((16 * 1024 * 1024,), NAN, device="cuda")
    steps = [("fwd", A1, 2, "f16x3"), ("fwd", A1, 2, "bf16x6"), ("fwd", A1, 2, "fp32"), ("fwd", A1, 2, "f16x3")]
    steps += [(ep, F4A, 4, dt) for dt in wf.FP32_GRADE for ep in ("infer", "dgrad")] + [("dgrad", A1, 2, "f16x3"), ("fwd", A1, 2, "bf16x6")]
    wd = ops.ohwi(torch.zeros((128, 128, 3, 3), device="cuda")).clone(memory_format=torch.preserve_format)       # one device buffer = one cache key
    cx = _lib.current_ctx()
    _lib.call("afi_ctx_set_wino_weight_cache", cx.handle, C.c_void_p(cache.data_ptr()), cache.numel())
    try:
        for rnd, wseed in enumerate((2, 52)):
            w = _rand((128, 128, 3, 3), wseed) / math.sqrt(9 * 128)
            wd.copy_(w.cuda())
            for i, (ep, shape, tiling, dt) in enumerate(steps):
                c = Case(ep, *shape, dt, tiling, 0)
                a, _ = wf.inputs(c.op, *shape)
                ref, rest = wf.reference(c.op, a, w), wf.restate(c.op, tiling, a, w, torch.float32)
                ws, n = _workspace(lib, c)
                out = ops.new_pixel_major(c.N, 128, c.H, c.W, "cuda")
                out.fill_(NAN)
                av = _pm(a)
                with _Options(amd, dt, {}):
                    if ep == "fwd":
                        _lib.call(ENTRY[ep], ops.view_of(av), c.N, c.H, c.W, 128, ops._p(wd), ops._p(None), 128, ops.view_of(out), ops._p(ws), n, ops.stream_ptr())
                    elif ep == "infer":
                        _lib.call(ENTRY[ep], ops.view_of(av), c.N, c.H, c.W, 128, ops._p(wd), ops._p(None), 128, ops.view_of(out), 0, ops._p(ws), n, ops.stream_ptr())
                    else:
                        _lib.call(ENTRY[ep], ops.view_of(av), c.N, c.H, c.W, 128, ops._p(wd), 128, ops.view_of(out), ops._NULL_VIEW, ops._p(ws), n,
                                  ops.stream_ptr())
                _assert_close(c, f"r{rnd}s{i}", out.cpu(), ref, rest, 128)
                if rnd == 0 and i == 0:                     # the transform went INTO the registered buffer (it started as NaN everywhere)
                    assert torch.isfinite(cache).any(), "the registered weight cache was not written"
            _lib.call("afi_ctx_wino_weight_cache_invalidate", cx.handle)
    finally:
        _lib.call("afi_ctx_set_wino_weight_cache", cx.handle, C.c_void_p(None), 0)


@pytest.mark.parametrize("dtype", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("shape,tiling", [(A1, 2), (F4A, 4)], ids=["F2", "F4"])
def test_wino_wgrad_accumulator_sum(amd, dtype, shape, tiling):
    """Three calls into one dw with an accumulator registered: nothing lands before the flush; after it dw holds the sum of the three
    float64 references at the bar of the summed problem (the three fp32 restatements added in fp32, Ktot = 3 T)."""
    from afigan_amd import _lib
    ops, lib = amd.ops, _lib.load()
    N, Cin, Cout, H, W = shape
    c = Case("wgrad", *shape, dtype, tiling, 0)
    acc = torch.full((8 * 1024 * 1024,), NAN, device="cuda")
    dw = ops.new_ohwi(Cout, Cin, 3, 3, "cuda", zero=True)
    ref, rest = 0, 0
    cx = _lib.current_ctx()
    with _Options(amd, dtype, {}):
        _lib.call("afi_ctx_set_wino_wgrad_accum", cx.handle, C.c_void_p(acc.data_ptr()), acc.numel())
        try:
            for seed in (1, 11, 21):
                x, dy = wf.inputs("wgrad", *shape, seed=seed)
                ref = ref + wf.reference("wgrad", x, dy)
                rest = rest + wf.restate("wgrad", tiling, x, dy, torch.float32)
                ws, n = _workspace(lib, c)
                dyd, xd = _pm(dy), _pm(x)                   # (both alive across the call: a dropped temporary's block goes to the next allocation)
                _lib.call(ENTRY["wgrad"], ops.view_of(dyd), ops.view_of(xd), N, H, W, Cout, Cin, ops._p(dw), 1.0, ops._p(ws), n, ops.stream_ptr())
            assert torch.isfinite(acc).any(), "the registered accumulator was not written"        # (it started as NaN everywhere)
            assert float(dw.abs().max()) == 0.0         # nothing lands in dw (zero-filled above) before the flush
        finally:
            _lib.call("afi_ctx_wino_wgrad_flush", cx.handle, ops.stream_ptr())
            _lib.call("afi_ctx_set_wino_wgrad_accum", cx.handle, C.c_void_p(None), 0)
    _assert_close(c, "sum3", dw.cpu(), ref, rest, 3 * wf.tiles(tiling, N, H, W))
