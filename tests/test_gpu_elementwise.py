"""The bandwidth passes of csrc/elementwise.hip against float64: BatchNorm statistics, apply and backward, column sums, BCE, L1, bilinear x2
and the SGD step, each at the smallest shapes that reach every branch of its kernel.

Reference: tests/elementwise_f64.py on the same fp32 inputs (held to torch's float64 ops by tests/test_elementwise_host.py, which also
asserts that every shape below takes the branch it is here for).  Torch CPU fp32's own error is printed next to the kernel's.

Bars (eps = 2^-24):
  statistics   mean, var, invstd and both running buffers equal the fp32 rounding of the reference or its neighbour (<= 1 ulp): the
               kernel accumulates in fp64 and rounds once, and the host test shows that every input family admits it
  apply        |got - ref| <= 5 eps (|x - mu| invstd |gamma| + |beta|) per element: four roundings (afi_bn_affine, contraction off) plus one
  elementwise  |got - ref| <= (r + 1) eps sum|terms| per element (+ (r + 1) 2^-126, the subnormal range), terms in float64 per element.
               r = the most fp32 roundings any one term passes through on its way to the result:
                 dx given the sums   r = 8   xhat (sub, mul), 1/Pn, s1/Pn, their product, the subtraction, gamma*invstd, the last product
                 BCE dz              r = 7   expf (<= 1 ulp = 2 roundings), 1 + e, the division, sig - t, two products, 1/n
                 L1 gradient         r = 2   1/n and gscale/n (the products of the four extents are exact below 2^24); the SIGN, and the
                                             zeros at ties and outside the crop, must match exactly
                 bilinear x2         r = 4   mul, add, mul, add (the weights .25 / .75 / 1 are exact); + 1 with beta
                 bilinear x2^T       r = 17  up to 16 taps per input pixel: one product and up to 16 additions; + 1 with beta
                 SGD m / p           r = 3 / 5   g*gscale, + wd*p, + momentum*m  /  then lr*m and p - .
  reductions   sum g, sum g*xhat, dgamma, dbeta, column sums, both losses -- the form and constants of tests/test_gpu_pixgemm.py with
               Ktot = P (or n):  max|got - ref| <= C_MAX sqrt(Ktot) eps max|ref|,  rel. L2 <= R_L2 max(cpu fp32's, sqrt(Ktot) eps / 8),
               C_MAX = 2, R_L2 = 4; for a loss (one number) both are its relative error, the saturated BCE cases included.
86 tests.  Measured on MI355X: the worst error / bar of each op and the case it came from (no bar was widened):
  statistics (afi_bn_stats, afi_bn_stats_ex)   0 ulp on all 30 shape x family cases, every vector
  bn_apply                 0.69  5500x384, slope 1          bilinear x2        0.61  (1, 64, 96, 96)
  bn_bwd_apply             0.43  16500x512, P_total 3 P     bilinear x2^T      0.26  (1, 256, 96, 96)
  BCE dz                   0.50  n 70001, t 0               SGD m / p          0.46 / 0.31  n 131077, wd 1e-4
  L1 gradient              0.12  (2, 128, 96, 96)
  reductions, max-norm / rel. L2 (torch CPU fp32's own errors are within 2x of the kernels' either way; the kernels sit at 1-3e-7 at every P):
  sum g                    0.16 / 0.22  7x8                 column sums        0.12  1x4 / 0.47  7x8
  sum g xhat               0.34 / 0.28  7x8                 BCE loss           0.22  n 1, t 0.9 / 0.29  n 255, t 0
  dgamma += / dbeta +=     0.34 / 0.26, 0.11 / 0.25         L1 loss            0.006 / 0.026
tests/test_gpu_d_parity.py::test_batch_statistics_in_both_accumulation_types at P = 546: option 1 0 ulp; option 0 mean <= 2.2e-7 std, var <= 6.4e-7
relative (bar 2.8e-6).

What the bars catch (scratch builds of csrc/elementwise.hip with one fault each, never committed; every case not named passed):
  (a) bn_apply takes the hoisted branch unconditionally      test_bn_apply[5500-384] alone.  The 77x12 and 100x96 cases run the fallback
                                                             branch with ONE item per thread, where the two branches compute the same
                                                             thing: only a fallback shape that also grid-strides can tell them apart
  (b) the fourth slot of apply's 4-way loop reuses v[0]      test_bn_apply[16500-512] alone
  (c) the fp64 statistics are not shifted by K = row 0       test_bn_stats[*-offset_1e4] at P = 7, 77, 1537, 16385, and [77-132-const_channel]
                                                             (var != 0 on a constant channel)
  (d) afi_red_geometry drops the last partial chunk          every test_bn_stats, test_bn_bwd_sums and test_colsum_accum case at P = 77, 1537
                                                             and 16385 (all three have a short last chunk), test_bn_bwd_sums_far_from_zero
  (e) BCE sums logf(1.f + e) instead of log1pf(e)            test_bce_logits[n-1.0] at n = 1, 255, 70001 (the saturated logits) and [1-0.0]
  (f) the SGD step leaves out gscale                         test_sgd_momentum_step
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import elementwise_f64 as E
from oracle import afigan_oracle as orc

pytestmark = pytest.mark.gpu

NAN = float("nan")
WORST = {}                      # op -> (worst error / bar, case): printed when the module is done


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    yield afigan_amd
    for op, (ratio, case) in sorted(WORST.items()):
        print(f"[elementwise] worst error / bar  {op:28s} {ratio:8.3f}   {case}")


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _pm(t):
    """CPU NCHW tensor -> GPU pixel-major tensor with the strides of a dense [N][H][W][C] block (channels_last leaves the strides of an extent
    of 1 unnormalised, which ops.view_of refuses)"""
    from afigan_amd import ops
    out = ops.new_pixel_major(*t.shape, "cuda")
    out.copy_(t)
    return out


def _note(op, ratio, case):
    if not (ratio <= WORST.get(op, (-1.0, ""))[0]):
        WORST[op] = (ratio, case)


def _check_elem(op, case, got, ref, terms, r):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (op, case, got.shape, ref.shape)
    ratio = float(((got.double() - ref).abs() / E.elementwise_bar(terms, r)).max())
    _note(op, ratio, case)
    print(f"[elementwise] {op:20s} {case:44s} worst |err| / ((r+1) eps terms) = {ratio:.3f}   (r = {r})")
    assert ratio <= 1.0, f"{op} {case}: an element misses its bar by {ratio:.3f}x"


def _check_red(op, case, got, ref, cpu32, ktot):
    got = got.detach().cpu().reshape(ref.shape)
    em, el = E.errs(got, ref)
    cm, cl = E.errs(cpu32.reshape(ref.shape), ref)
    bar, l2bar = E.reduction_bars(ktot, cl)
    _note(op + " max-norm", em / bar, case)
    _note(op + " rel-L2", el / l2bar, case)
    print(f"[elementwise] {op:20s} {case:44s} Ktot {ktot:7d}  max-norm {em:.2e} (cpu fp32 {cm:.2e}, bar {bar:.2e})"
          f"  rel-L2 {el:.2e} (cpu fp32 {cl:.2e}, bar {l2bar:.2e})  depth {E.add_chain_depth(ktot)}")
    assert em <= bar, f"{op} {case}: max-norm rel error {em:.3e} > bar {bar:.3e} (cpu fp32 {cm:.3e})"
    assert el <= l2bar, f"{op} {case}: rel-L2 error {el:.3e} > bar {l2bar:.3e} (cpu fp32 {cl:.3e})"


def _check_ulp(op, case, got, ref):
    u = float(E.ulps_from(got, ref).max())
    _note(op + " (ulp)", u, case)
    assert u <= 1.0, f"{op} {case}: {u} ulp from the rounded float64 reference"
    return u


# ------------------------------------------------------------------------------------------------ BatchNorm statistics
STATS_PC = [(P, Cc) for P, Cc, _ in E.STATS_SHAPES]


@pytest.mark.parametrize("family", E.STATS_FAMILIES)
@pytest.mark.parametrize("P,Cc", STATS_PC)
def test_bn_stats(amd, P, Cc, family):
    """afi_bn_stats (the discriminator's eps / momentum, var requested) and afi_bn_stats_ex (eps 1e-3, momentum 0.01, the counter, var
    requested and not) on every shape x input family: <= 1 ulp on mean, var, invstd and both running buffers."""
    ops = amd.ops
    x = E.stats_input(family, P, Cc)
    rm0, rv0 = 0.3 * _rand((Cc,), 4) + 0.1, 1 + 0.5 * _rand((Cc,), 5).abs()
    xd = x.cuda()
    case = f"{P}x{Cc} {family}"
    ref = E.bn_stats(x, orc.BN_EPS, orc.BN_MOMENTUM, rm0, rv0)
    rm, rv = rm0.cuda(), rv0.cuda()
    mean, invstd, var = ops.bn_stats(xd, rm, rv)
    us = [_check_ulp("bn_stats " + k, case, v, ref[k]) for k, v in (("mean", mean), ("var", var), ("invstd", invstd), ("running_mean", rm), ("running_var", rv))]
    ref = E.bn_stats(x, 1e-3, 0.01, rm0, rv0)
    for want_var in (True, False):
        rm, rv, nbt = rm0.cuda(), rv0.cuda(), torch.tensor([41], dtype=torch.int64, device="cuda")
        out = ops.bn_stats_ex(xd, 1e-3, 0.01, rm, rv, nbt, want_var=want_var)
        assert int(nbt) == 42
        got = {"mean": out[0], "invstd": out[1], "running_mean": rm, "running_var": rv}
        if want_var:
            got["var"] = out[2]
        us += [_check_ulp("bn_stats_ex " + k, case, v, ref[k]) for k, v in got.items()]
    if family == "const_channel":
        assert float(var[1]) == 0.0 and float(out[0][1]) == E.CONST_VALUE
        assert float(E.ulps_from(invstd[1:2], torch.tensor([1.0 / math.sqrt(E.f32(orc.BN_EPS))], dtype=torch.float64))) <= 1.0
    mean, invstd = ops.bn_stats_ex(xd, 1e-3, 0.01)              # no running buffers, no counter
    us += [_check_ulp("bn_stats_ex mean", case, mean, ref["mean"]), _check_ulp("bn_stats_ex invstd", case, invstd, ref["invstd"])]
    print(f"[elementwise] bn_stats             {case:44s} worst {max(us)} ulp over {len(us)} vectors")


# ------------------------------------------------------------------------------------------------ BatchNorm apply
APPLY_PC = [(P, Cc) for P, Cc, _, _ in E.APPLY_SHAPES]


@functools.lru_cache(maxsize=2)
def _apply_inputs(P, Cc):
    """x, g and parameter vectors of an apply / backward-apply case (CPU fp32), shared by the tests of that shape"""
    x = _rand((P, Cc), 1) * 1.7 + 0.3
    g = _rand((P, Cc), 6)
    mean, invstd = 0.3 + 0.2 * _rand((Cc,), 7), 0.6 + 0.3 * _rand((Cc,), 8).abs()
    gamma, beta = 1 + 0.5 * _rand((Cc,), 2), 0.3 * _rand((Cc,), 3)      # (some gammas near zero, a few negative at the wide shapes)
    return x, g, mean, invstd, gamma, beta


@pytest.mark.parametrize("P,Cc", APPLY_PC)
def test_bn_apply(amd, P, Cc):
    """afi_bn_apply_lrelu_fwd (slope 0.2) and afi_bn_apply_fwd at slope 1 and 0.01: the per-element four-roundings bar."""
    ops = amd.ops
    x, _, mean, invstd, gamma, beta = _apply_inputs(P, Cc)
    dev = [t.cuda() for t in (x, mean, invstd, gamma, beta)]
    runs = (("lrelu_fwd 0.2", 0.2, lambda: ops.bn_apply_lrelu(*dev)), ("apply_fwd 1", 1.0, lambda: ops.bn_apply(*dev, slope=1.0)),
            ("apply_fwd 0.01", 0.01, lambda: ops.bn_apply(*dev, slope=0.01)))
    for name, slope, run in runs:
        ref, terms = E.bn_apply(x, mean, invstd, gamma, beta, slope)
        _check_elem("bn_apply", f"{P}x{Cc} {name}", run(), ref, terms, 4)


# ------------------------------------------------------------------------------------------------ BatchNorm backward
@pytest.mark.parametrize("P,Cc", APPLY_PC)
def test_bn_bwd_apply_given_sums(amd, P, Cc):
    """afi_bn_bwd_apply with the float64 sums rounded to fp32, P_total = P and 3 P (SyncBatchNorm: sums over all ranks' rows), out of place
    and in place on g (as nets.hip calls it)."""
    from afigan_amd import _lib, ops
    x, g, _, _, gamma, _ = _apply_inputs(P, Cc)
    xd, gd, gad = x.cuda(), g.cuda(), gamma.cuda()
    md, isd, _ = ops.bn_stats(xd)
    mean, invstd = md.cpu(), isd.cpu()
    s0, s1 = E.bn_bwd_sums(g, x, mean, invstd)
    sums = torch.stack([s0, s1]).float()
    for Pn in (P, 3 * P):
        ref, terms = E.bn_bwd_dx(g, x, mean, invstd, gamma, sums[0], sums[1], Pn)
        _check_elem("bn_bwd_apply", f"{P}x{Cc} P_total {Pn}", ops.bn_bwd_apply(gd, xd, md, isd, gad, sums.cuda(), Pn), ref, terms, 8)
        gi = gd.clone()
        p = lambda t: C.c_void_p(t.data_ptr())
        _lib.call("afi_bn_bwd_apply", p(gi), p(xd), p(gi), p(md), p(isd), p(gad), p(sums.cuda()), P, Pn, Cc, ops.stream_ptr())
        _check_elem("bn_bwd_apply", f"{P}x{Cc} P_total {Pn} in place", gi, ref, terms, 8)


def _bwd_sums_case(ops, x, g, case):
    P, Cc = x.shape
    xd, gd = x.cuda(), g.cuda()
    md, isd, _ = ops.bn_stats(xd)
    mean, invstd = md.cpu(), isd.cpu()
    s0, s1 = E.bn_bwd_sums(g, x, mean, invstd)
    xh32 = (x - mean) * invstd
    c0, c1 = g.sum(0), (g * xh32).sum(0)                       # torch CPU fp32
    dg0, db0 = _rand((Cc,), 11) * 3, _rand((Cc,), 12) * 3
    dg, db = dg0.cuda(), db0.cuda()
    sums = ops.bn_bwd_sums(gd, xd, md, isd, dg, db)
    _check_red("bn_bwd_sums sum g", case, sums[0], s0, c0, P)
    _check_red("bn_bwd_sums sum g xhat", case, sums[1], s1, c1, P)
    _check_red("bn_bwd_sums dbeta +=", case, db, db0.double() + s0, db0 + c0, P)
    _check_red("bn_bwd_sums dgamma +=", case, dg, dg0.double() + s1, dg0 + c1, P)
    again = ops.bn_bwd_sums(gd, xd, md, isd, None, None)        # NULL dgamma / dbeta: the same sums, bit for bit
    assert torch.equal(again, sums)


@pytest.mark.parametrize("P,Cc", STATS_PC)
def test_bn_bwd_sums(amd, P, Cc):
    """afi_bn_bwd_sums on the statistics shapes: the two sums, dgamma / dbeta accumulating onto non-zero values, and both passed as NULL."""
    _bwd_sums_case(amd.ops, _rand((P, Cc), 1) * 1.7 + 0.3, _rand((P, Cc), 6), f"{P}x{Cc}")


def test_bn_bwd_sums_far_from_zero(amd):
    """the same with a mean far from zero: x - mean is exact in fp32 (the reference takes the kernel's fp32 mean)"""
    _bwd_sums_case(amd.ops, E.stats_input("offset_1e4", 77, 132), _rand((77, 132), 6), "77x132 offset_1e4")


@pytest.mark.parametrize("P,Cc", STATS_PC + APPLY_PC)
def test_bn_bwd_is_its_two_halves(amd, P, Cc):
    """afi_bn_bwd = afi_bn_bwd_sums then afi_bn_bwd_apply(P_total = P), bit for bit: the same kernels in a fixed order."""
    ops = amd.ops
    xd, gd = (_rand((P, Cc), 1) * 1.7 + 0.3).cuda(), _rand((P, Cc), 6).cuda()
    gad = (1 + 0.5 * _rand((Cc,), 2)).cuda()
    md, isd, _ = ops.bn_stats(xd)
    dg0, db0 = (_rand((Cc,), 11) * 3).cuda(), (_rand((Cc,), 12) * 3).cuda()
    dg1, db1 = dg0.clone(), db0.clone()
    dx0 = ops.bn_bwd(gd, xd, md, isd, gad, dg0, db0)
    sums = ops.bn_bwd_sums(gd, xd, md, isd, dg1, db1)
    dx1 = ops.bn_bwd_apply(gd, xd, md, isd, gad, sums, P)
    assert torch.equal(dx0, dx1) and torch.equal(dg0, dg1) and torch.equal(db0, db1)
    assert bool(torch.isfinite(dx0).all())


@pytest.mark.parametrize("P,Cc", STATS_PC)
def test_colsum_accum(amd, P, Cc):
    """afi_colsum_accum on a channel slice of a wider matrix (ld = C + 8 > C), alpha = 0.5, onto a non-zero db."""
    wide = _rand((P, Cc + 8), 7)
    db0 = _rand((Cc,), 8) * 3
    db = db0.cuda()
    amd.ops.colsum_accum(wide.cuda()[:, 4:4 + Cc], db, alpha=0.5)
    g = wide[:, 4:4 + Cc]
    _check_red("colsum_accum", f"{P}x{Cc} ld {Cc + 8}", db, db0.double() + 0.5 * E.colsum(g), db0 + 0.5 * g.sum(0), P)


# ------------------------------------------------------------------------------------------------ BCE
def _bce_logits(family, n):
    g = torch.Generator().manual_seed(20 + n % 97)
    if family == "normal5":
        return torch.randn((n,), generator=g) * 5
    if family == "saturated":
        return 20 + 60 * torch.rand((n,), generator=g)
    raise KeyError(family)


def _bce_case(ops, z, target, case, lscale=1.0, loss0=0.0, gscale=1.0):
    n = z.numel()
    loss_ref, dz_ref, terms = E.bce_logits(z, target)
    zg = z.clone().requires_grad_(True)
    cpu = F.binary_cross_entropy_with_logits(zg, torch.full_like(z, target))
    loss = torch.full((1,), loss0, device="cuda")
    dz = ops.bce_logits(z.cuda(), target, loss, lscale=lscale, gscale=gscale)
    _check_red("bce loss", case, loss, (loss0 + lscale * loss_ref).reshape(1), (loss0 + lscale * cpu.detach()).reshape(1), n)
    _check_elem("bce dz", case, dz, gscale * dz_ref, gscale * terms, 7)


@pytest.mark.parametrize("target", [0.0, 1.0, 0.9])
@pytest.mark.parametrize("n", [n for n, _ in E.BCE_N])
def test_bce_logits(amd, n, target):
    """N(0, 5) logits at every n x target; logits all in +[20, 80] (target 1: the loss is ~1e-9 and every term is log1p of a tiny number;
    target 0: the loss is the mean logit) -- the loss is one number, compared relative to itself."""
    _bce_case(amd.ops, _bce_logits("normal5", n), target, f"n {n} t {target} N(0,5)")
    if target != 0.9:
        _bce_case(amd.ops, _bce_logits("saturated", n), target, f"n {n} t {target} +U(20,80)")


@pytest.mark.parametrize("target", [0.0, 1.0, 0.9])
def test_bce_logits_extremes_scales_and_null_gradient(amd, target):
    """0, +-100 and +-88.7 (exp(-|z|) underflows or lands in the subnormals); lscale = 0.5 onto *loss = 3.0 with gscale = 2; dz = NULL."""
    ops = amd.ops
    z = torch.tensor([0.0, 100.0, -100.0, 88.7, -88.7])
    _bce_case(ops, z, target, f"n 5 t {target} extremes")
    _bce_case(ops, _bce_logits("normal5", 70001), target, f"n 70001 t {target} lscale .5 onto 3, gscale 2", lscale=0.5, loss0=3.0, gscale=2.0)
    z = _bce_logits("normal5", 255)
    guard = torch.full((255,), NAN, device="cuda")
    loss = torch.zeros(1, device="cuda")
    assert ops.bce_logits(z.cuda(), target, loss, want_grad=False) is None
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard).all())
    assert abs(float(loss) - float(E.bce_logits(z, target)[0])) <= E.C_MAX * math.sqrt(255) * E.EPS * float(E.bce_logits(z, target)[0])


# ------------------------------------------------------------------------------------------------ L1
def _l1_case(ops, a, b, ad, bd, case, lscale=1.0, loss0=0.0, gscale=1.0, want_grad=True):
    """a, b: CPU NCHW values; ad, bd: the pixel-major GPU tensors (possibly views) holding them"""
    loss_ref, da_ref = E.l1_crop(a, b)
    h, w = min(a.shape[2], b.shape[2]), min(a.shape[3], b.shape[3])
    n = a.shape[0] * a.shape[1] * h * w
    cpu = F.l1_loss(a[:, :, :h, :w], b[:, :, :h, :w])
    loss = torch.full((1,), loss0, device="cuda")
    da = ops.l1_crop(ad, bd, loss, lscale=lscale, gscale=gscale, want_grad=want_grad)
    _check_red("l1 loss", case, loss, (loss0 + lscale * loss_ref).reshape(1), (loss0 + lscale * cpu).reshape(1), n)
    if not want_grad:
        assert da is None
        return
    da = da.cpu()
    assert torch.equal(torch.sign(da).double(), torch.sign(da_ref)), f"{case}: a gradient's sign (or a zero) differs"
    _check_elem("l1 da", case, da, gscale * da_ref, torch.full_like(da_ref, E.f32(gscale) / n), 2)


def test_l1_crop(amd):
    """a larger than b, b larger than a, each larger along one axis; a quarter of the elements tied; lscale onto a non-zero loss; da = NULL."""
    ops = amd.ops
    big, small = (2, 16, 14, 22), (2, 16, 13, 21)
    for sa, sb in ((big, small), (small, big), ((2, 16, 14, 21), (2, 16, 13, 22))):
        a, b = _rand(sa, 2), _rand(sb, 3)
        _l1_case(ops, a, b, _pm(a), _pm(b), f"a {sa[2]}x{sa[3]} b {sb[2]}x{sb[3]}")
    a, b = _rand(big, 2), _rand(small, 3)
    a[:, :, :13, :21][..., ::4] = b[..., ::4]
    assert int((a[:, :, :13, :21] == b).sum()) >= b.numel() // 4
    _l1_case(ops, a, b, _pm(a), _pm(b), "a quarter tied")
    _l1_case(ops, a, b, _pm(a), _pm(b), "lscale .5 onto 3, gscale 2", lscale=0.5, loss0=3.0, gscale=2.0)
    _l1_case(ops, a, b, _pm(a), _pm(b), "da NULL", want_grad=False)


def test_l1_crop_views_and_grid_stride(amd):
    """a and b as crops and channel slices of larger buffers (pixel strides that are not the extents); (2, 128, 96, 96): grid-stride."""
    ops = amd.ops
    A, B = _rand((2, 24, 16, 25), 4), _rand((2, 28, 15, 24), 5)
    Ad, Bd = _pm(A), _pm(B)
    sa = (slice(None), slice(4, 20), slice(1, 15), slice(2, 24))
    sb = (slice(None), slice(8, 24), slice(0, 13), slice(3, 24))
    _l1_case(ops, A[sa].contiguous(), B[sb].contiguous(), Ad[sa], Bd[sb], "views a 14x22 b 13x21")
    shape = [s for s, w in E.L1_SHAPES if w][0]
    a, b = _rand(shape, 6), _rand((shape[0], shape[1], shape[2] - 1, shape[3]), 7)
    _l1_case(ops, a, b, _pm(a), _pm(b), f"a {shape[2]}x{shape[3]} x{shape[1]} grid-stride")


# ------------------------------------------------------------------------------------------------ bilinear x2
@pytest.mark.parametrize("shape", [s for s, _ in E.BILINEAR_FWD_SHAPES], ids=str)
def test_bilinear2x_fwd(amd, shape):
    """out = beta * out + bilinear2x(x): H = 1, W = 1, both; (1, 12, 5, 7) as a crop and channel slice of a larger buffer; beta = 0 and 0.5."""
    ops = amd.ops
    x = _rand(shape, 3)
    if shape == (1, 12, 5, 7):
        big = _rand((1, 20, 8, 9), 5)
        sl = (slice(None), slice(4, 16), slice(1, 6), slice(2, 9))
        big[sl] = x
        xd = _pm(big)[sl]
    else:
        xd = _pm(x)
    ref, terms = E.bilinear2x(x)
    _check_elem("bilinear2x fwd", f"{shape} beta 0", ops.bilinear2x(xd).cpu(), ref, terms, 4)
    out0 = _rand(tuple(ref.shape), 9)
    out = _pm(out0)
    assert ops.bilinear2x(xd, out=out, beta=0.5) is out
    _check_elem("bilinear2x fwd", f"{shape} beta .5", out.cpu(), ref + 0.5 * out0.double(), terms + 0.5 * out0.double().abs(), 5)


@pytest.mark.parametrize("shape", [s for s, _ in E.BILINEAR_BWD_SHAPES], ids=str)
def test_bilinear2x_bwd(amd, shape):
    """dx = beta * dx + bilinear2x^T(dout), beta = 0 and 0.5; `shape` is dx's."""
    ops = amd.ops
    N, Cc, H, W = shape
    dout = _rand((N, Cc, 2 * H, 2 * W), 4)
    ref, terms = E.bilinear2x_T(dout)
    dd = _pm(dout)
    _check_elem("bilinear2x bwd", f"{shape} beta 0", ops.bilinear2x_bwd(dd).cpu(), ref, terms, 17)
    dx0 = _rand(shape, 9)
    dx = _pm(dx0)
    assert ops.bilinear2x_bwd(dd, dx=dx, beta=0.5) is dx
    _check_elem("bilinear2x bwd", f"{shape} beta .5", dx.cpu(), ref + 0.5 * dx0.double(), terms + 0.5 * dx0.double().abs(), 18)


# ------------------------------------------------------------------------------------------------ SGD
def test_sgd_momentum_step(amd):
    """afi_sgd_momentum_step on three tensors (1, 1000 and 131077 elements: the last one is max_n and past 512 x 256 threads) cut from flat
    buffers at odd float offsets, weight decay 0 and 1e-4, non-zero momentum buffers, gscale = 0.5; the floats between the tensors stay."""
    from afigan_amd import _lib, ops
    sizes, wds = E.SGD_SIZES, (1e-4, 0.0, 1e-4)
    offs = [1, 5, 1007]
    total = offs[-1] + sizes[-1] + 3
    assert all(o % 2 == 1 for o in offs) and all(offs[i] + sizes[i] < offs[i + 1] for i in range(2))
    lr, mom, gscale = 0.02, 0.9, 0.5
    flat = {k: _rand((total,), s) for k, s in (("p", 1), ("g", 2), ("m", 3))}
    dev = {k: v.cuda() for k, v in flat.items()}
    descs = (_lib.SgdDesc * 3)()
    for i, (o, n) in enumerate(zip(offs, sizes)):
        d = descs[i]
        d.p, d.g, d.m, d.n, d.wd = dev["p"].data_ptr() + 4 * o, dev["g"].data_ptr() + 4 * o, dev["m"].data_ptr() + 4 * o, n, wds[i]
    assert C.sizeof(_lib.SgdDesc) == 40
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
    _lib.call("afi_sgd_momentum_step", C.c_void_p(table.data_ptr()), 3, sizes[-1], lr, mom, gscale, ops.stream_ptr())
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in dev.items()}
    assert torch.equal(got["g"], flat["g"])
    inside = torch.zeros(total, dtype=torch.bool)
    for i, (o, n) in enumerate(zip(offs, sizes)):
        inside[o:o + n] = True
        sl = slice(o, o + n)
        p2, m2, tp, tm = E.sgd_step(flat["p"][sl], flat["g"][sl], flat["m"][sl], lr, mom, wds[i], gscale)
        _check_elem("sgd m", f"n {n} wd {wds[i]}", got["m"][sl], m2, tm, 3)
        _check_elem("sgd p", f"n {n} wd {wds[i]}", got["p"][sl], p2, tp, 5)
    assert torch.equal(got["p"][~inside], flat["p"][~inside]) and torch.equal(got["m"][~inside], flat["m"][~inside])
