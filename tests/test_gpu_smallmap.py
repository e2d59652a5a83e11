"""The interpolator's small-map schedule against float64 with resolved LeakyReLU masks, with proof of which kernels ran.

The interpolator call the project is tuned for (1 x 256 x 25 x 34, and every call of up to 4096 low-res pixels) runs on kernels of
csrc/smallmap.hip that only a whole call reaches, driven by gen_plan() (csrc/nets.hip); tests/test_gpu_pixgemm.py holds the per-op kinds:
  20  pix_gemm_wk6     afi_pix_gemm_wk6_kernel / its 32x64 form afi_pix_gemm_wk6w_kernel (each with a _group_kernel) on the weight images of
                       afi_wk6_image_kernel (KC / RC jobs, the two conv-transpose modes, the zero fill and the bilinear skip gradient riding along)
  19  wgrad_group6     afi_wgrad6_group_sk_kernel: stream-K runs over up to 20 problems, every tile added by fp32 atomics; packed growth gradients
  16  wgrad_group      the fp32 stream-K groups, 32x128 (rows <= 32) and 128x128 tiles: tiles one run owns stored, shared tiles added by atomics
  15  (grouped)        afi_pix_gemm_wk_group_kernel, and the per-problem pix_gemm_wk where a pass has no image for a conv
Every case runs amd.Generator under a fresh context on reference_init_generator_params weights and the loss (out * R).sum(), forward and
backward each inside the launch profiler, and states the exact set of kinds from {0-12, 15, 16, 19, 20} each pass must record -- derived by
reading gen_plan(), gen_fwd_image_reqs / gen_bwd_image_reqs, GenPix, afi_launch_pix_gemm and the refusals of afi_launch_wgrad6_group:
  * a pass on images (Fwd::six / Bwd::images: bf16x6 or f16x3, C % 32 == G % 32 == 0) records 20 for every conv that has an image; the final
    conv on the 4x map has one only while 4 P <= 4096 (GenPlan::hires_wk6), else it runs without (kind 15; C < 128 keeps it off Winograd).
  * a grouped backward under the six-product arithmetics packs the growth gradients (4G rows) and sends every problem of more than 32 rows
    to wgrad_group6 (19); problems of <= 32 rows (C = 32: head, trunk, final conv, conv5) go to the fp32 32x128 group (16).  With C = 64 or
    128 nothing is that narrow: 19 alone.  Under fp32 both the wide and the narrow group are kind 16.
  * channels that are no multiples of 32 get no images (wk6_shapes_ok) but the backward is still `six`: 15 for every pixel GEMM, 19 for the
    weight gradients (48 and 64 rows, all above 32).
  * deterministic = 1: the forward does not look at it (images, 20); the backward runs per layer without images (15) and its weight
    gradients one by one on the per-op kernels: 64 rows -> kind 9, the conv-transpose (4C = 256 rows) and the packed growth gradient
    (4G = 128 rows, Bwd::batch_growth: n_wino == 0 below 128 channels) -> kind 8.

Reference and bars: tests/smallmap_f64.py (float64, masks resolved per run; |S| <= 64 asserted on the reference before the kernel's result
is looked at).  Further checks: b twice (atomics: each run within the bar), b-nodx (dx == NULL, the stage-1 production call: parameter
gradients within the bar of case b's), j twice bit-identical, and shape b under ops.weight_transform_cache (first call builds the images in
cache slots, the second finds them: out and dx bit-identical between the calls, the parameter gradients -- all added by atomics at this
shape -- within the bar, and the forward bit-identical to the call without a cache).

Measured on MI355X (error / (sqrt(K) eps) with K as in the bars: forward 9 (C + 4G), gradients max(9 (C + 4G), 4 N H W); the larger of
max-norm and rel-L2; |S|, flips; torch CPU fp32's forward max-norm beside the kernel's):
  case     kinds fwd / bwd              forward max-norm (ratio; torch cpu fp32)   worst gradient: max-norm / rel-L2 (ratio)                  |S|  flips
  a        20 / 16 19 20                7.5e-08 (0.03; 7.5e-08)                    Generators.0.4.0.weight          5.2e-07 / 2.3e-07 (0.23)    0    0
  b        20 / 19 20                   8.1e-08 (0.03; 1.1e-07)                    Generators.0.0.0.bias            6.6e-07 / 8.3e-07 (0.34)    3    0
  b-nodx   20 / 19 20                   8.1e-08 (0.03; 1.1e-07)                    Generators.0.0.0.bias            6.6e-07 / 8.3e-07 (0.34)    3    0
  c        20 / 19 20                   1.0e-07 (0.04; 1.3e-07)                    Generators.0.0.0.bias            2.9e-06 / 1.8e-06 (0.86)    7    0
  d        20 / 19 20                   1.4e-07 (0.05; 1.4e-07)                    Generators.0.0.0.bias            2.5e-06 / 2.7e-06 (0.95)   13    0
  e        15 20 / 15 16 19 20          9.2e-08 (0.04; 1.0e-07)                    Generators.0.0.0.bias            1.0e-06 / 1.2e-06 (0.31)    1    0
  f        15 20 / 15 16 19 20          9.7e-08 (0.04; 1.3e-07)                    Generators.0.0.0.bias            1.1e-06 / 1.7e-06 (0.26)   17    0
  g        15 / 15 19                   6.8e-08 (0.04; 1.2e-07)                    ...RDBs.0.conv1.0.weight         6.6e-07 / 4.3e-07 (0.35)    0    0
  h        15 / 15 16                   8.1e-08 (0.03; 1.1e-07)                    ...RDBs.0.conv2.0.weight         6.7e-07 / 5.2e-07 (0.27)    3    0
  i        20 / 16 19 20                7.5e-08 (0.03; 7.5e-08)                    Generators.0.4.0.weight          5.2e-07 / 2.3e-07 (0.23)    0    0
  j        20 / 8 9 15                  8.1e-08 (0.03; 1.1e-07)                    Generators.0.2.0.weight          9.3e-07 / 4.4e-07 (0.37)    3    0
The forward figures sit at the fp32 rounding of the output itself (the bilinear skip dominates its magnitude): the kernels and torch CPU fp32
are alike there.  The worst gradient is the head conv's bias (a column sum over all pixels behind the whole chain) from 800 pixels on.
C_F = 1 and C_G = 2: twice the worst ratio (0.05, 0.95), rounded up.  The largest bars of the table: forward 2.9e-6 (case d), gradients
1.3e-5 (case f); the condition is <= 1e-4.

What the bars catch (scratch builds, never committed):
  the image kernel storing zeros for the second residual plane (both the matrix jobs and the conv-transpose modes): a, b, b-nodx, d, i and
    the cache case fail, by gradients at 1.02 .. 1.1 x their bar (the third bf16 plane carries 2^-17 of a weight: this is as small as a real
    error of these kernels gets); c, e and f, whose bars are wider by sqrt(4 N H W), pass.  The forward bar does not see it.
  afi_wk6_body skipping a tile's last K stage: every case that runs kind 20 fails on the forward output (4e-5 .. 7e-5 against 2.3e-6 .. 2.9e-6;
    the whole-call tests' 1e-3 passes it), j included (its forward is on images); g and h (no images) pass.
  the 32x64 form reading its second N tile from the first tile's image offset: exactly c (the group launch) and d (the single launch) fail.
  the stream-K walk of the six-product weight gradients treating a shared tile as owned: no case fails, and none can -- afi_wgrad6_gemm_range
    ignores the flag and adds every element atomically, owned tile or not.  The same mutation in the fp32 group kernel (kind 16), which does
    store the tiles a run owns: every case that records kind 16 fails (a, e, f, h, i; gradients off by 4e-3 .. 0.9), the others pass.
  the packed growth gradient unpacked with the row blocks of conv1 and conv2 swapped (the tail launch): every case whose backward packs it
    fails (a .. g, i and the cache case); h (fp32: the growth convs one by one) and j (deterministic: the per-layer unpack kernel) pass.
"""
import pytest
import torch

import smallmap_f64 as sm
import test_gpu_pixgemm as PG
from oracle import afigan_oracle as orc

pytestmark = pytest.mark.gpu

FAMILY = frozenset(range(13)) | {15, 16, 19, 20}


class Case:
    """One interpolator call: channels C, growth G, R dense blocks on N x H x W; ctx dtype (None: the default, f16x3), ctx options,
    whether x requires a gradient, and the kinds of FAMILY the forward and the backward must record (exactly)."""

    def __init__(self, id, C, G, R, N, H, W, fwd, bwd, dtype=None, options=None, want_dx=True, seed=0, runs=1):
        self.id, self.C, self.G, self.R, self.N, self.H, self.W = id, C, G, R, N, H, W
        self.fwd, self.bwd, self.dtype, self.options, self.want_dx, self.seed, self.runs = set(fwd), set(bwd), dtype, options or {}, want_dx, seed, runs

    @property
    def P(self):
        return self.N * self.H * self.W

    @property
    def shape_key(self):
        return (self.C, self.G, self.R, self.N, self.H, self.W, self.seed)

    def __repr__(self):
        return self.id


CASES = [
    # one full pixel tile + a 3-pixel tail; weight-gradient tiles of 2 stages stored whole; hi-res map 140 px.  C = 32: the 32-row problems
    # (head, trunk, final conv, conv5) on the fp32 narrow group, the packed growth and conv-transpose gradients (128 rows) on wgrad_group6
    Case("a", 32, 32, 1, 1, 5, 7, fwd={20}, bwd={20, 16, 19}),
    # a pixel tile straddles the image boundary at pixel 99; 7-stage weight-gradient tiles cut by runs (shared tiles, atomics); two dense
    # blocks chained.  Run twice: each run within the bar
    Case("b", 64, 32, 2, 2, 9, 11, fwd={20}, bwd={20, 19}, runs=2),
    Case("b-nodx", 64, 32, 2, 2, 9, 11, fwd={20}, bwd={20, 19}, want_dx=False),      # dx == NULL: no head image, no skip gradient in the image launch
    # the dense block's first grouped step: 26 x (4 + 1) = 130 tiles -> the 32x64 group kernel; 25-pixel tail
    Case("c", 64, 32, 1, 1, 25, 33, fwd={20}, bwd={20, 19}),
    # the hi-res conv at 2048 px: 64 x 2 = 128 wide tiles -> the 32x64 single-launch kernel; 4G == C
    Case("d", 128, 32, 1, 1, 16, 32, fwd={20}, bwd={20, 19}),
    # 4 P = 4224 > 4096: hires_wk6 off while the images are on; the hi-res pair runs without an image
    Case("e", 32, 32, 1, 1, 33, 32, fwd={20, 15}, bwd={20, 15, 16, 19}),
    # P = 3008 > 2048 and > 3000: forward batched and backward grouped only through the six-product rule
    Case("f", 32, 32, 1, 1, 47, 64, fwd={20, 15}, bwd={20, 15, 16, 19}),
    # channels not multiples of 32: no images
    Case("g", 48, 16, 1, 1, 7, 9, fwd={15}, bwd={15, 19}),
    # fp32: kind 15 grouped, kind 16 narrow (the growth convs one by one, 32 rows) and wide
    Case("h", 64, 32, 2, 2, 9, 11, fwd={15}, bwd={15, 16}, dtype="fp32"),
    # bf16x6: the same kernels as f16x3 (afi_dtype_smallmap6)
    Case("i", 32, 32, 1, 1, 5, 7, fwd={20}, bwd={20, 16, 19}, dtype="bf16x6"),
    # deterministic: forward on images, backward per layer; two runs bit-identical
    Case("j", 64, 32, 2, 2, 9, 11, fwd={20}, bwd={15, 8, 9}, options={"deterministic": 1}, runs=2),
]
BY_ID = {c.id: c for c in CASES}


def inputs(c):
    """(parameters, x, R) of a case: CPU fp32, from the case's seed (cases of one shape share them)"""
    g = torch.Generator().manual_seed(c.seed)
    p = orc.reference_init_generator_params(c.C, c.R, c.G, generator=g)
    x = torch.randn((c.N, c.C, c.H, c.W), generator=g)
    Rw = torch.randn((c.N, c.C, 2 * c.H, 2 * c.W), generator=g)
    return p, x, Rw


_refs = {}


def reference(c, device):
    """the case's float64 reference (shared by the cases of one shape; with dx, which a case without it simply does not compare)"""
    key = c.shape_key + (str(device),)
    if key not in _refs:
        p, x, Rw = inputs(c)
        _refs[key] = sm.Reference(x.to(device), {k: v.to(device) for k, v in p.items()}, Rw.to(device), c.C, c.G, c.R, want_dx=True, device=device)
    return _refs[key]


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return afigan_amd


def _kernel_run(amd, c, G, cx, x, Rw):
    """one forward + backward of G under cx, each inside the profiler: (out, {name: gradient}, kinds of the forward, kinds of the backward)"""
    from afigan_amd import _lib
    for q in G.parameters():
        q.grad = None
    xg = x.cuda().requires_grad_(c.want_dx)
    with _lib.use_ctx(cx):
        out, ran_f = PG._profiled(lambda: G(xg))
        loss = (out * Rw.cuda()).sum()
        _, ran_b = PG._profiled(lambda: loss.backward())
    grads = {k: q.grad.detach().clone() for k, q in G.named_parameters()}
    if c.want_dx:
        grads["dx"] = xg.grad.detach().clone()
    return out.detach().clone(), grads, ran_f, ran_b


def _model(amd, c):
    from afigan_amd import _lib
    cx = _lib.Ctx(c.dtype)
    for k, v in c.options.items():
        cx.set_option(k, v)
    G = amd.Generator(in_channels=c.C, n_residual_dense_blocks=c.R, growth_rate=c.G).cuda()
    p, x, Rw = inputs(c)
    G.load_state_dict(p)
    return cx, G, p, x, Rw


_results = {}


def _case_runs(amd, c):
    """the case's kernel runs [(out, grads, kinds fwd, kinds bwd)], once per session"""
    if c.id not in _results:
        cx, G, p, x, Rw = _model(amd, c)
        _results[c.id] = [_kernel_run(amd, c, G, cx, x, Rw) for _ in range(c.runs)]
    return _results[c.id]


def _check_kinds(c, ran_f, ran_b):
    f, b = {k for k in ran_f if k in FAMILY}, {k for k in ran_b if k in FAMILY}
    print(f"[smallmap] case {c.id}: forward recorded {ran_f}, backward recorded {ran_b}")
    assert f == c.fwd, f"case {c.id}: the forward must record kinds {sorted(c.fwd)}, the profiler saw {ran_f}"
    assert b == c.bwd, f"case {c.id}: the backward must record kinds {sorted(c.bwd)}, the profiler saw {ran_b}"


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_smallmap_schedule_vs_fp64(amd, case):
    c = case
    ref = reference(c, "cuda")                             # (|S| <= CAP is asserted in there, on the reference alone)
    p, x, Rw = inputs(c)
    cpu32 = sm.generator_forward(x, p, c.R)
    runs = _case_runs(amd, c)
    for i, (out, grads, ran_f, ran_b) in enumerate(runs):
        tag = f"case {c.id} run {i}"
        _check_kinds(c, ran_f, ran_b)
        ref.check_out(out, tag, cpu32=cpu32)
        ref.check_grads(grads, tag)
    if c.id == "b-nodx":                                   # the parameter gradients of the dx == NULL call against case b's own
        gb = _case_runs(amd, BY_ID["b"])[0][1]
        assert "dx" not in runs[0][1] and set(runs[0][1]) == set(gb) - {"dx"}
        for k, g in runs[0][1].items():
            em, el = sm.errs(g, gb[k].double())
            assert max(em, el) <= ref.bar_g, f"b-nodx {k}: {em:.3e} / {el:.3e} from case b's gradient (bar {ref.bar_g:.3e})"
    if c.id == "j":
        for k in runs[0][1]:
            assert torch.equal(runs[0][1][k], runs[1][1][k]), f"case j {k}: two runs under deterministic = 1 differ"
        assert torch.equal(runs[0][0], runs[1][0])


def test_smallmap_weight_cache_builds_then_hits(amd):
    """Shape b under ops.weight_transform_cache: the first call builds the weight images in cache slots, the second finds them.  Out and dx
    (computed without atomics) are bit-identical between the two calls.  Every parameter gradient of this shape is added by fp32 atomics --
    the stream-K runs are 4 stages long and cut every 7- and 25-stage weight-gradient tile (tests/test_smallmap_host.py asserts that plan),
    the grouped bias sums add one partial per 128 rows -- so those agree within the bar, and each is within the bar of float64.  The forward
    output is bit-identical to the call without a cache."""
    from afigan_amd import _lib, ops
    c = BY_ID["b"]
    ref = reference(c, "cuda")
    cx, G, p, x, Rw = _model(amd, c)
    with _lib.use_ctx(cx), ops.weight_transform_cache("cuda"):
        runs = [_kernel_run(amd, c, G, cx, x, Rw) for _ in range(2)]
    for i, (out, grads, ran_f, ran_b) in enumerate(runs):
        _check_kinds(c, ran_f, ran_b)
        ref.check_out(out, f"cache call {i}")
        ref.check_grads(grads, f"cache call {i}")
    (o0, g0, _, _), (o1, g1, _, _) = runs
    assert torch.equal(o0, o1), "the forward on cached images differs from the forward that built them"
    assert torch.equal(g0["dx"], g1["dx"]), "dx on cached images differs"
    for k in g0:
        em, el = sm.errs(g1[k], g0[k].double())
        assert max(em, el) <= ref.bar_g, (k, em, el)
    assert torch.equal(o0, _case_runs(amd, c)[0][0]), "the forward under a weight cache differs from the forward without one"
