"""The BiFPN node kernels against float64 past every launch cap: fusion + swish forward and backward, the depthwise 3x3, its input and weight
gradients, the zero-padded 3x3/2 max-pool (plain, with argmax, backward), and the pass-through kernels next to them -- afi_relu_bwd,
afi_nearest_nhwc, afi_nchw_to_nhwc / afi_nhwc_to_nchw.

Reference: tests/bifpn_f64.py on the same fp32 inputs (held to torch's float64 ops and autograd by tests/test_bifpn_host.py, which also asserts
that every shape below takes the paths it is here for and that the shapes of an op reach every path it has).  Every output is written into the
middle of a buffer filled with one NaN bit pattern: the bands on both sides must keep it, and no element of the output may (a pass that
never ran leaves it behind).

Bars (eps = 2^-24; terms in float64 per element, tests/bifpn_f64.py):
  depthwise 3x3, and its input gradient (the forward on dy with rows 8..0 of w9c)
               |got - ref| <= (r + 1) eps sum_t |w_t x_t|,  r = 18: nine products and nine additions (an fma contraction only lowers it)
  fuse + swish |got - ref| <= (r + 1) eps terms + (|s| + 2 k_exp) eps gain, per element.
               forward   r = 3   s = w0 a + w1 b + w2 c: three products and two additions, each bounded by eps sum |w_k x_k| in all, reach out
                                 through f'(s); 1 + e and the division are relative to out.  terms = |f'(s)| sum |w_k x_k| + |out|
               d{a,b,c}  r = 4   the same three on s, reaching ds through dout f''(s); sg = 1 / (1 + e) two roundings through
                                 d ds / d sg; u = 1 - sg and s u through d ds / d u; 1 + s u, dout sg and the last product relative to
                                 ds (at most three on any one magnitude); then w_k ds
               the fast exponential is counted apart: __expf(-s) = exp2(-s log2 e) has the relative error (|s| + k_exp) eps -- the
               rounded argument moves it by |s| eps, the hardware exponential by k_exp eps -- and reaches out through
               gain = |s| e / (1 + e)^2, ds through |dout (1 + s - 2 s sig)| e / (1 + e)^2: it matters near s = 0 and vanishes in both tails.
               k_exp: neither the guides nor anything else at hand states the accuracy of v_exp_f32, so it is MEASURED here, by the
               fixture k_exp, through the forward kernel itself: with w = (1, 0) and b = 0, s = a exactly and e = s / out - 1 in float64,
               on 65 536 values of s in [-8, -2] (e in 7 .. 2981, where 1 + e and the division blur e by at most 2.3 eps, which the
               measurement includes).  k_exp = max(1, max over the probe of rel. error / eps - |s|); the bars use twice that for the
               arguments the probe did not visit (s > 0 in the first place: e < 1 cannot be read back from out).  Measured: see below.
  dw9c         reduction_bars(Ktot = N H W, torch CPU fp32's rel. L2): max-norm <= 2 sqrt(Ktot) eps, rel. L2 <= 4 max(cpu fp32's, sqrt(Ktot) eps / 8)
  dw_k         one number each: relative error <= 2 sqrt(n) eps, n = the elements summed, under |dw_k| >= 0.1 sum |ds x_k| (host test)
  max-pool     values and argmax taps bit-equal (int32 view: the sign of a zero counts).  Backward: at most four addends, compared with the
               float64 gather at r = 3 on the sum of |dout| over the contributing windows (the choice between the issue's two forms)
  relu_bwd     the zeros where act <= 0 are +0.0 exactly; elsewhere r = 1, and bit-equal to g with scale = 1
  nearest, transposes      bit-equal through an int32 view, on inputs holding -0.0, inf, a subnormal and NaNs of two payloads

Shapes: tests/bifpn_f64.py CASES.  Three come on top of the issue's table: (1, 132, 23, 29) for the fusion backward -- its 86 block partials
are the only count between 64 and the cap that is no multiple of 64 (finalize_strided; the capped shapes have 1024 = 16 x 64);
(2, 128, 7, 9) for the weight gradient (one FULL channel block) and (2, 132, 8, 6) for the pool with argmax (even H and W, several channel
quads).  (2, 132, 7, 9) runs the weight gradient in two chunks of 63 rows, one image each, not three.

134 tests, 4 s.  Measured on MI355X: k_exp = 2.71 (worst relative error of e over the probe: 8.81 eps, at |s| near 8), so the bars use 5.42.
The worst error / bar of each op and the case it came from (no bar was widened):
  fuse_swish               0.43  (2, 132, 95, 89), 3 inputs        dwconv3x3                0.22  (2, 132, 95, 89)
  fuse_swish_bwd d{a,b,c}  0.43  (2, 132, 67, 63), 3 inputs, dc    dwconv3x3 input grad     0.21  (2, 132, 95, 89)
  fuse_swish_bwd dw_k      0.17  (1, 4, 1, 1), 3 inputs            dw9c max-norm / rel. L2  0.24 / 0.33  (2, 8, 5, 1)
  maxpool3s2_same_bwd      0.55  (2, 132, 135, 125), negative      relu_bwd, scale 1/3      0.42  (2, 132, 95, 89)
  dw_k: relative errors 1e-9 .. 1e-7 at every n from 4 to 2.2 M (bars 2.4e-7 .. 1.8e-4).  dw9c: 9e-8 max-norm and rel. L2 at every Ktot from
  1 to 16 910; torch CPU fp32's own are 2e-8 .. 1.7e-7, within 2x of the kernel's either way.
  max-pool values and taps, nearest, both transposes and their round trip, relu_bwd at scale 1, every view: 0 elements differ.
What the tests found: afi_maxpool3s2_same_kernel took its maximum with fmaxf, which orders -0.0 below +0.0, so a window whose first maximum
was -0.0 came out as +0.0 where afi_maxpool3s2_same_idx_kernel and torch keep -0.0 (test_maxpool3s2_same[*-halves]: 7 of 3168 and 7490 of
2 207 040 elements, all of them in the sign of a zero alone).  It now scans with '>' as the other kernel does.  The depthwise and max-pool
launchers took any view; they now refuse one their 16-byte loads cannot take, as afi_nearest_nhwc does (tests/test_bifpn_host.py).

What the bars catch (scratch builds with one value fault each, never committed; every case not named passed):
  (a) a grid-stride loop stops after its first pass
        afi_fuse_swish_kernel                   test_fuse_swish at (2, 132, 95, 89) alone, by the fill pattern left behind
        afi_fuse_swish_bwd_kernel               test_fuse_swish_bwd at (2, 132, 67, 63) and (2, 132, 95, 89), and the optional-output and
                                                poisoned-scratch tests at those shapes
  (b) afi_dwconv3x3_wgrad drops its last chunk  test_dwconv3x3_wgrad at (2, 132, 67, 63) and (2, 132, 95, 89): the two with a short last chunk
  (c) its row decode is r / W without % H       test_dwconv3x3_wgrad at every shape with N = 2
  (d) the argmax takes '>=' for '>'             test_maxpool3s2_same_idx and _bwd (which compares the taps first) on zeros and halves at every
                                                shape, on negative at every shape with an even H or W and on random at all of those but
                                                (1, 8, 2, 5): there the pad wins a window and the tie is between two pad zeros, which the taps
                                                tell apart although the gradient does not
  (e) the pad counts as -3.4e38, not 0          all three pool tests on negative at every shape with an even H or W, on random and halves at
                                                all of those but (1, 8, 2, 5); no odd shape and no zeros case (a window of zeros keeps tap 0)
  (f) the swish finalizer sums 64 partials      test_fuse_swish_bwd at (1, 132, 23, 29), (2, 132, 67, 63), (2, 132, 95, 89): more than 64 blocks
  (g) __expf(s) for __expf(-s) in the backward  every test_fuse_swish_bwd case
"""
import ctypes as C
import functools
import math

import pytest
import torch

import bifpn_f64 as B

pytestmark = pytest.mark.gpu

FILL = 0x7FC0DEAD               # the NaN every output buffer starts as
PAD = 1024                      # elements of guard band on either side
WORST = {}                      # op -> (worst error / bar, case): printed when the module is done


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    yield afigan_amd
    for op, (ratio, case) in sorted(WORST.items()):
        print(f"[bifpn-kernels] worst error / bar  {op:28s} {ratio:8.3f}   {case}")


def _note(op, ratio, case):
    if not (ratio <= WORST.get(op, (-1.0, ""))[0]):
        WORST[op] = (ratio, case)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _pm(t):
    """CPU NCHW tensor -> GPU pixel-major tensor with the strides of a dense [N][H][W][C] block"""
    from afigan_amd import ops
    out = ops.new_pixel_major(*t.shape, "cuda")
    out.copy_(t)
    return out


class _Out:
    """n elements in the middle of a buffer of one bit pattern (fp32: the NaN FILL; uint8: 0xFF, which no tap is)"""

    def __init__(self, n, dtype=torch.float32):
        self.n, self.f32 = int(n), dtype == torch.float32
        if self.f32:
            self.raw = torch.full((self.n + 2 * PAD,), FILL, dtype=torch.int32, device="cuda")
            self.buf = self.raw.view(torch.float32)
        else:
            self.raw = self.buf = torch.full((self.n + 2 * PAD,), 0xFF, dtype=torch.uint8, device="cuda")
        self.t = self.buf[PAD:PAD + self.n]

    def nchw(self, N, Cc, H, W):
        return self.t.view(N, H, W, Cc).permute(0, 3, 1, 2)

    def check(self, what):
        fill = FILL if self.f32 else 0xFF
        assert bool((self.raw[:PAD] == fill).all()) and bool((self.raw[PAD + self.n:] == fill).all()), f"{what}: wrote outside its output"
        left = int((self.raw[PAD:PAD + self.n] == fill).sum())
        assert left == 0, f"{what}: {left} of {self.n} output elements were never written"
        return self


def _call(name, *args):
    from afigan_amd import _lib, ops
    _lib.call(name, *args, ops.stream_ptr())


# ------------------------------------------------------------------------------------------------ the kernels, on guarded outputs
def k_fuse_swish(w, a, b, c):
    o = _Out(a.numel())
    _call("afi_fuse_swish_fwd", _p(a), _p(b), _p(c), _p(w), _p(o.t), a.numel())
    return o.check("fuse_swish").nchw(*a.shape)


def k_fuse_swish_bwd(w, a, b, c, dout):
    """(dw, da, db, dc or None), every output requested"""
    from afigan_amd import _lib, ops
    n = a.numel()
    outs = [_Out(w.numel()), _Out(n), _Out(n), _Out(n) if c is not None else None]
    scratch = ops.new_workspace(_lib.load().afi_fuse_swish_bwd_scratch_floats(), a.device)
    _call("afi_fuse_swish_bwd", _p(a), _p(b), _p(c), _p(w), _p(dout), _p(outs[1].t), _p(outs[2].t), _p(outs[3].t) if outs[3] else None, _p(outs[0].t),
          n, _p(scratch))
    for o in outs:
        if o is not None:
            o.check("fuse_swish_bwd")
    return (outs[0].t,) + tuple(o.nchw(*a.shape) if o is not None else None for o in outs[1:])


def k_dwconv3x3(x, w9c):
    from afigan_amd import ops
    N, Cc, H, W = x.shape
    o = _Out(x.numel())
    _call("afi_dwconv3x3_fwd", ops.view_of(x), N, H, W, Cc, _p(w9c), _p(o.t))
    return o.check("dwconv3x3").nchw(N, Cc, H, W)


def k_dwconv3x3_wgrad(dy, x):
    from afigan_amd import _lib, ops
    N, Cc, H, W = x.shape
    o = _Out(9 * Cc)
    scratch = ops.new_workspace(_lib.load().afi_dwconv3x3_wgrad_scratch_floats(Cc), x.device)
    _call("afi_dwconv3x3_wgrad", _p(dy), _p(x), N, H, W, Cc, _p(o.t), _p(scratch))
    return o.check("dwconv3x3_wgrad").t.view(9, Cc)


def k_maxpool(x):
    from afigan_amd import ops
    N, Cc, H, W = x.shape
    Ho, Wo = B.pool_out(H), B.pool_out(W)
    o = _Out(N * Ho * Wo * Cc)
    _call("afi_maxpool3s2_same_fwd", ops.view_of(x), N, H, W, Cc, _p(o.t))
    return o.check("maxpool3s2_same").nchw(N, Cc, Ho, Wo)


def k_maxpool_idx(x):
    """(out NCHW, idx as [N][C][Ho][Wo] uint8)"""
    from afigan_amd import ops
    N, Cc, H, W = x.shape
    Ho, Wo = B.pool_out(H), B.pool_out(W)
    o, ix = _Out(N * Ho * Wo * Cc), _Out(N * Ho * Wo * Cc, torch.uint8)
    _call("afi_maxpool3s2_same_fwd_idx", ops.view_of(x), N, H, W, Cc, _p(o.t), _p(ix.t))
    return o.check("maxpool3s2_same_idx").nchw(N, Cc, Ho, Wo), ix.check("maxpool3s2_same_idx taps").nchw(N, Cc, Ho, Wo)


def k_maxpool_bwd(dout, idx_nhwc, in_hw):
    N, Cc = dout.shape[:2]
    H, W = in_hw
    o = _Out(N * H * W * Cc)
    _call("afi_maxpool3s2_same_bwd", _p(dout), _p(idx_nhwc), N, H, W, Cc, _p(o.t))
    return o.check("maxpool3s2_same_bwd").nchw(N, Cc, H, W)


def k_relu_bwd(g, act, scale):
    o = _Out(g.numel())
    _call("afi_relu_bwd", _p(g), _p(act), _p(o.t), g.numel(), float(scale))
    return o.check("relu_bwd").nchw(*g.shape)


def k_nearest(x, up, down):
    from afigan_amd import ops
    N, Cc, H, W = x.shape
    Ho, Wo = B.nearest_out(H, up, down), B.nearest_out(W, up, down)
    o = _Out(N * Ho * Wo * Cc)
    _call("afi_nearest_nhwc", ops.view_of(x), N, H, W, Cc, int(up), int(down), _p(o.t))
    return o.check("nearest").nchw(N, Cc, Ho, Wo)


# ------------------------------------------------------------------------------------------------ the checks
def _check_elem(op, case, got, ref, terms, r, extra=None):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (op, case, got.shape, ref.shape)
    bar = B.elementwise_bar(terms, r)
    if extra is not None:
        bar = bar + extra
    ratio = float(((got.double() - ref).abs() / bar).max())
    _note(op, ratio, case)
    print(f"[bifpn-kernels] {op:22s} {case:44s} worst |err| / bar = {ratio:.3f}   (r = {r})")
    assert ratio <= 1.0, f"{op} {case}: an element misses its bar by {ratio:.3f}x"


def _check_red(op, case, got, ref, cpu32, ktot):
    got = got.detach().cpu().reshape(ref.shape)
    em, el = B.errs(got, ref)
    cm, cl = B.errs(cpu32.reshape(ref.shape), ref)
    bar, l2bar = B.reduction_bars(ktot, cl)
    _note(op + " max-norm", em / bar, case)
    _note(op + " rel-L2", el / l2bar, case)
    print(f"[bifpn-kernels] {op:22s} {case:44s} Ktot {ktot:7d}  max-norm {em:.2e} (cpu fp32 {cm:.2e}, bar {bar:.2e})"
          f"  rel-L2 {el:.2e} (cpu fp32 {cl:.2e}, bar {l2bar:.2e})")
    assert em <= bar, f"{op} {case}: max-norm rel error {em:.3e} > bar {bar:.3e} (cpu fp32 {cm:.3e})"
    assert el <= l2bar, f"{op} {case}: rel-L2 error {el:.3e} > bar {l2bar:.3e} (cpu fp32 {cl:.3e})"


def _check_bits(op, case, got, ref):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (op, case, got.shape, ref.shape)
    only_bits = 0
    if got.dtype == torch.float32:
        only_bits = int(((B.bits(got) != B.bits(ref)) & ((got == ref) | (got.isnan() & ref.isnan()))).sum())
        got, ref = B.bits(got), B.bits(ref)
    bad = int((got.contiguous() != ref.contiguous()).sum())
    _note(op + " (elements that differ)", float(bad), case)
    assert bad == 0, (f"{op} {case}: {bad} of {ref.numel()} elements differ from the reference bit for bit"
                      f" ({only_bits} of them in the sign of a zero or a NaN's payload alone)")


def _specials(t):
    """every 7th element replaced, in turn, by -0.0, a quiet NaN with a payload, a negative NaN, +inf and a subnormal"""
    flat = t.clone().contiguous().view(-1).view(torch.int32)
    pats = torch.tensor([-0x80000000, 0x7FC12345, -0x3FFFFF, 0x7F800000, 0x00012345], dtype=torch.int32)     # (-0x3FFFFF = 0xFFC00001)
    pos = torch.arange(0, flat.numel(), 7)
    flat[pos] = pats[torch.arange(pos.numel()) % 5]
    return flat.view(torch.float32).view(t.shape)


def _ids(cases):
    return ["x".join(str(v) for v in s) for s in cases]


def _shapes(op):
    return [s for s, _ in B.CASES[op]]


# ------------------------------------------------------------------------------------------------ the fast exponential
@pytest.fixture(scope="module")
def k_exp(amd):
    """the accuracy of __expf as the swish kernels use it, read back through afi_fuse_swish_fwd (module docstring)"""
    g = torch.Generator().manual_seed(77)
    s = -(2.0 + 6.0 * torch.rand((1, 4, 128, 128), generator=g))
    out = k_fuse_swish(torch.tensor([1.0, 0.0]).cuda(), _pm(s), _pm(torch.zeros_like(s)), None).cpu()
    s64 = s.double()
    e_hat, e = s64 / out.double() - 1.0, torch.exp(-s64)
    rel = (e_hat / e - 1.0).abs() / B.EPS
    k = max(1.0, float((rel - s64.abs()).max()))
    print(f"[bifpn-kernels] k_exp measured {k:.3f}  (worst rel. error of e {float(rel.max()):.3f} eps on s in [-8, -2]); the bars use {2 * k:.3f}")
    return k


# ------------------------------------------------------------------------------------------------ fusion + swish
@functools.lru_cache(maxsize=2)
def _swish_fwd_inputs(shape):
    return tuple(B.rand(shape, 20 + k) for k in range(3))


@pytest.mark.parametrize("n_in", [3, 2])
@pytest.mark.parametrize("shape", _shapes("fuse_swish"), ids=_ids(_shapes("fuse_swish")))
def test_fuse_swish(amd, k_exp, shape, n_in):
    xs = _swish_fwd_inputs(shape)[:n_in]
    c = xs[2] if n_in == 3 else None
    w = torch.tensor(B.SWISH_W3[:n_in])
    got = k_fuse_swish(w.cuda(), *[_pm(x) for x in xs], *([None] if c is None else []))
    ref, terms = B.fuse_swish(w, xs[0], xs[1], c)
    a_s, gain = B.fuse_swish_exp(w, xs[0], xs[1], c)
    _check_elem("fuse_swish", f"{shape} {n_in} inputs", got, ref, terms, 3, extra=B.EPS * (a_s + 2 * k_exp) * gain)


@pytest.mark.parametrize("n_in", [3, 2])
@pytest.mark.parametrize("shape", _shapes("fuse_swish_bwd"), ids=_ids(_shapes("fuse_swish_bwd")))
def test_fuse_swish_bwd(amd, k_exp, shape, n_in):
    w, a, b, c, dout = B.swish_bwd_inputs(shape, n_in)
    dev = [w.cuda(), _pm(a), _pm(b), _pm(c) if c is not None else None, _pm(dout)]
    got = k_fuse_swish_bwd(*dev)
    (dw, *dx), (tw, *tx) = B.fuse_swish_bwd(w, a, b, c, dout)
    a_s, gain = B.fuse_swish_bwd_exp(w, a, b, c, dout)
    case = f"{shape} {n_in} inputs"
    for k in range(n_in):
        _check_elem("fuse_swish_bwd d{a,b,c}", case + f" d{'abc'[k]}", got[1 + k], dx[k], tx[k], 4,
                    extra=B.EPS * (a_s + 2 * k_exp) * abs(float(w[k])) * gain)
    assert n_in == 3 or got[3] is None
    n = a.numel()
    rel = ((got[0].cpu().double() - dw).abs() / dw.abs())
    bar = B.C_MAX * math.sqrt(n) * B.EPS
    assert bool((dw.abs() >= 0.1 * tw).all())
    _note("fuse_swish_bwd dw_k", float(rel.max()) / bar, case)
    print(f"[bifpn-kernels] fuse_swish_bwd dw_k    {case:44s} rel. errors {[f'{v:.2e}' for v in rel.tolist()]}  bar {bar:.2e}  (n = {n})")
    assert float(rel.max()) <= bar, f"dw {case}: relative errors {rel.tolist()} > {bar:.3e}"
    again = k_fuse_swish_bwd(*dev)
    assert all(torch.equal(B.bits(x), B.bits(y)) for x, y in zip(got, again) if x is not None), "two runs differ"


NEEDS = [(1, 1, 0, 0), (0, 0, 1, 1), (1, 0, 0, 0), (0, 1, 1, 1)]


@pytest.mark.parametrize("shape", [B._MID, B._STRIDED, B._BWD_CAP], ids=_ids([B._MID, B._STRIDED, B._BWD_CAP]))
def test_fuse_swish_bwd_optional_outputs(amd, shape):
    """need = what _FuseSwishFn.backward passes on from ctx.needs_input_grad: a requested output is bit-identical to the all-requested run,
    the others come back None (their pointers are NULL in the call)"""
    ops = amd.ops
    for n_in in (3, 2):
        w, a, b, c, dout = B.swish_bwd_inputs(shape, n_in)
        dev = [w.cuda(), _pm(a), _pm(b), _pm(c) if c is not None else None, _pm(dout)]
        full = ops.fuse_swish_bwd(*dev)
        assert all((full[i] is not None) == (i < 1 + n_in) for i in range(4))
        for need in NEEDS:
            got = ops.fuse_swish_bwd(*dev, need=tuple(bool(v) for v in need))
            for i in range(4):
                if need[i] and full[i] is not None:
                    assert got[i] is not None and torch.equal(B.bits(got[i]), B.bits(full[i])), (shape, n_in, need, i)
                else:
                    assert got[i] is None, (shape, n_in, need, i)


# ------------------------------------------------------------------------------------------------ depthwise 3x3
@functools.lru_cache(maxsize=2)
def _dw_inputs(shape):
    Cc = shape[1]
    return B.rand(shape, 1), B.rand(shape, 2), B.rand((Cc, 9), 3).t().contiguous()       # x, dy, w9c [9][C]


@pytest.mark.parametrize("shape", _shapes("dwconv3x3"), ids=_ids(_shapes("dwconv3x3")))
def test_dwconv3x3_and_input_gradient(amd, shape):
    x, dy, w9c = _dw_inputs(shape)
    ref, terms = B.dwconv3x3(x, w9c)
    _check_elem("dwconv3x3", f"{shape}", k_dwconv3x3(_pm(x), w9c.cuda()), ref, terms, 18)
    wr = w9c.flip(0).contiguous()
    ref, terms = B.dwconv3x3(dy, wr)
    _check_elem("dwconv3x3 input grad", f"{shape}", k_dwconv3x3(_pm(dy), wr.cuda()), ref, terms, 18)


def _wgrad32(dy, x):
    """torch CPU fp32's own weight gradient, by the same nine products"""
    H, W = x.shape[2:]
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    return torch.stack([(dy * xp[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W]).sum((0, 2, 3)) for t in range(9)])


@pytest.mark.parametrize("shape", _shapes("dwconv3x3_wgrad"), ids=_ids(_shapes("dwconv3x3_wgrad")))
def test_dwconv3x3_wgrad(amd, shape):
    x, dy, _ = _dw_inputs(shape)
    N, Cc, H, W = shape
    xd, dyd = _pm(x), _pm(dy)
    got = k_dwconv3x3_wgrad(dyd, xd)
    ref, _ = B.dwconv3x3_wgrad(dy, x)
    if H == 1 or W == 1:                                       # taps that only ever meet the zero pad: exactly zero, not merely small
        dead = [t for t in range(9) if (H == 1 and t // 3 != 1) or (W == 1 and t % 3 != 1)]
        assert float(got[dead].abs().max()) == 0.0 and float(ref[dead].abs().max()) == 0.0
    _check_red("dwconv3x3_wgrad", f"{shape}", got, ref, _wgrad32(dy, x), N * H * W)
    assert torch.equal(B.bits(k_dwconv3x3_wgrad(dyd, xd)), B.bits(got)), "two runs differ"


# ------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("family", B.POOL_FAMILIES)
@pytest.mark.parametrize("shape", _shapes("maxpool"), ids=_ids(_shapes("maxpool")))
def test_maxpool3s2_same(amd, shape, family):
    x = B.pool_input(family, shape)
    ref, _ = B.maxpool3s2_same(x, want_taps=False)
    _check_bits("maxpool3s2_same", f"{shape} {family}", k_maxpool(_pm(x)), ref)


@pytest.mark.parametrize("family", B.POOL_FAMILIES)
@pytest.mark.parametrize("shape", _shapes("maxpool_idx"), ids=_ids(_shapes("maxpool_idx")))
def test_maxpool3s2_same_idx(amd, shape, family):
    x = B.pool_input(family, shape)
    ref, tap = B.maxpool3s2_same(x)
    out, idx = k_maxpool_idx(_pm(x))
    _check_bits("maxpool3s2_same_idx value", f"{shape} {family}", out, ref)
    _check_bits("maxpool3s2_same_idx tap", f"{shape} {family}", idx, tap)


@pytest.mark.parametrize("family", B.POOL_FAMILIES)
@pytest.mark.parametrize("shape", _shapes("maxpool_bwd"), ids=_ids(_shapes("maxpool_bwd")))
def test_maxpool3s2_same_bwd(amd, shape, family):
    """the backward on the KERNEL's own taps (checked against the reference's first), as the node runs it"""
    x = B.pool_input(family, shape)
    N, Cc, H, W = shape
    _, tap = B.maxpool3s2_same(x)
    dout = B.rand(tap.shape, 9)
    _, idx = k_maxpool_idx(_pm(x))
    _check_bits("maxpool3s2_same_idx tap", f"{shape} {family}", idx, tap)
    got = k_maxpool_bwd(_pm(dout), idx, (H, W))                 # idx: a [N][Ho][Wo][C] block, viewed as NCHW
    ref, terms = B.maxpool3s2_same_bwd(dout, tap, (H, W))
    assert bool(((got.cpu() == 0) | (terms > 0)).all()), "a gradient where no window points"
    _check_elem("maxpool3s2_same_bwd", f"{shape} {family}", got, ref, terms, 3)


# ------------------------------------------------------------------------------------------------ the pass-through kernels
@pytest.mark.parametrize("shape", _shapes("relu_bwd"), ids=_ids(_shapes("relu_bwd")))
def test_relu_bwd(amd, shape):
    g, act = B.rand(shape, 5), torch.relu(B.rand(shape, 6))
    act.view(-1)[::5] = 0.0                                     # (exact zeros, and -0.0 below, are not > 0)
    act.view(-1)[::11] = -0.0
    gd, ad = _pm(g), _pm(act)
    for scale in (1.0, 1.0 / 3):
        got = k_relu_bwd(gd, ad, scale)
        ref, terms = B.relu_bwd(g, act, scale)
        off = act <= 0
        assert bool((B.bits(got)[off] == 0).all()), "the masked elements are not +0.0"
        if scale == 1.0:
            _check_bits("relu_bwd scale 1", f"{shape}", got, torch.where(off, torch.zeros(()), g))
        else:
            _check_elem("relu_bwd", f"{shape} scale 1/3", got, ref, terms, 1)


@pytest.mark.parametrize("shape", _shapes("nearest"), ids=_ids(_shapes("nearest")))
def test_nearest(amd, shape):
    N, Cc, H, W, up, down = shape
    x = _specials(B.rand((N, Cc, H, W), 7))
    _check_bits("nearest", f"{shape}", k_nearest(_pm(x), up, down), B.nearest(x, up, down))


@pytest.mark.parametrize("Cc", B.TRANSPOSE_C)
def test_layout_transposes(amd, Cc):
    """each direction alone against permute, and the round trip, bit for bit"""
    for N in B.TRANSPOSE_N:
        for P in B.TRANSPOSE_P:
            x = _specials(B.rand((N, Cc, P), 8))                # [N][C][P]
            xd = x.cuda()
            o = _Out(x.numel())
            _call("afi_nchw_to_nhwc", _p(xd), _p(o.t), N, Cc, P)
            nhwc = o.check("nchw_to_nhwc").t.view(N, P, Cc)
            _check_bits("nchw_to_nhwc", f"({N}, {Cc}, {P})", nhwc, B.nchw_to_nhwc(x))
            y = _specials(B.rand((N, P, Cc), 9))                # [N][P][C]
            o2 = _Out(y.numel())
            _call("afi_nhwc_to_nchw", _p(y.cuda()), _p(o2.t), N, Cc, P)
            _check_bits("nhwc_to_nchw", f"({N}, {Cc}, {P})", o2.check("nhwc_to_nchw").t.view(N, Cc, P), B.nhwc_to_nchw(y))
            o3 = _Out(x.numel())
            _call("afi_nhwc_to_nchw", _p(nhwc.contiguous()), _p(o3.t), N, Cc, P)
            _check_bits("transpose round trip", f"({N}, {Cc}, {P})", o3.check("round trip").t.view(N, Cc, P), x)


# ------------------------------------------------------------------------------------------------ views
def _view_of_kind(kind, x):
    """x as a view of a wider GPU tensor whose other elements are 1e30: a spatial crop (offset (1, 2)) or a channel slice (offset 4 of C + 8).
    Offsets and strides stay multiples of 4 floats, which afigan_amd.ops.view_of requires."""
    N, Cc, H, W = x.shape
    if kind == "crop":
        big = torch.full((N, Cc, H + 3, W + 2), 1e30)
        big[:, :, 1:1 + H, 2:2 + W] = x
        return _pm(big)[:, :, 1:1 + H, 2:2 + W]
    big = torch.full((N, Cc + 8, H, W), 1e30)
    big[:, 4:4 + Cc] = x
    return _pm(big)[:, 4:4 + Cc]


@pytest.mark.parametrize("kind", ["crop", "slice"])
@pytest.mark.parametrize("shape", [(2, 12, 6, 5), B._MID], ids=_ids([(2, 12, 6, 5), B._MID]))
def test_views(amd, shape, kind):
    """dwconv3x3, both max-pool forwards and nearest on a crop / a channel slice: the dense result, bit for bit"""
    x = B.pool_input("halves", shape, seed=3) + 0.25 * B.rand(shape, 4).round()
    w9c = B.rand((shape[1], 9), 3).t().contiguous().cuda()
    dense, view = _pm(x), _view_of_kind(kind, x)
    assert not view.permute(0, 2, 3, 1).is_contiguous() and torch.equal(view.cpu(), x)
    assert torch.equal(B.bits(k_dwconv3x3(view, w9c)), B.bits(k_dwconv3x3(dense, w9c)))
    assert torch.equal(B.bits(k_maxpool(view)), B.bits(k_maxpool(dense)))
    (ov, iv), (od, idn) = k_maxpool_idx(view), k_maxpool_idx(dense)
    assert torch.equal(B.bits(ov), B.bits(od)) and torch.equal(iv.cpu(), idn.cpu())
    for up, down in ((2, 1), (1, 2)):
        assert torch.equal(B.bits(k_nearest(view, up, down)), B.bits(k_nearest(dense, up, down)))
    _check_bits("views: dwconv3x3 / pools / nearest", f"{shape} {kind}", k_maxpool(view), B.maxpool3s2_same(x, want_taps=False)[0])


# ------------------------------------------------------------------------------------------------ scratch
@pytest.mark.parametrize("shape", [B._MID, B._STRIDED, B._FWD_CAP], ids=_ids([B._MID, B._STRIDED, B._FWD_CAP]))
def test_no_result_reads_scratch_it_did_not_write(amd, shape, monkeypatch):
    """both two-stage reductions with their scratch poisoned: the same bits as on fresh scratch, and no NaN"""
    ops = amd.ops
    w, a, b, c, dout = B.swish_bwd_inputs(shape, 3)
    dev = [w.cuda(), _pm(a), _pm(b), _pm(c), _pm(dout)]
    w2 = w[:2].contiguous().cuda()
    run = lambda: (k_fuse_swish_bwd(*dev), k_fuse_swish_bwd(w2, dev[1], dev[2], None, dev[4]), k_dwconv3x3_wgrad(dev[4], dev[1]))
    plain = run()
    asked = []

    def poisoned(floats, device):
        asked.append(int(floats))
        return torch.full((int(floats),), float("nan"), device=device, dtype=torch.float32)
    monkeypatch.setattr(ops, "new_workspace", poisoned)
    again = run()
    assert asked == [4 * B.BT_GRID_CAP, 4 * B.BT_GRID_CAP, B.DWW_MAX_CHUNKS * 9 * shape[1]]
    flat = lambda r: [t for t in (r if isinstance(r, tuple) else (r,)) if t is not None]
    for p, q in zip(plain, again):
        for x, y in zip(flat(p), flat(q)):
            assert not bool(torch.isnan(y).any()) and torch.equal(B.bits(x), B.bits(y))
