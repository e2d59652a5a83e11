"""CPU-side checks of tests/elementwise_f64.py, the float64 yardstick of test_gpu_elementwise.py: (a) every reference against torch's own
float64 ops and autograd to 1e-12; (b) every case of the tables lands on the branch it names, and the cases of an op together reach every
branch that op has -- a retuned grid cap or an edited shape fails here, without a GPU; (c) the shifted one-pass form of the statistics
kernels, emulated in float64 in three summation orders, stays within one fp32 ulp of the two-pass reference on every hard input."""
import pytest
import torch
import torch.nn.functional as F

import elementwise_f64 as E

TOL = 1e-12


def _rand(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _same(got, ref, what):
    scale = max(float(ref.abs().max()), 1e-300)
    err = float((got - ref).abs().max())
    assert got.shape == ref.shape and err <= TOL * scale, f"{what}: {err:.3e} against scale {scale:.3e}"


# ------------------------------------------------------------------------------------------------ (a) the references are the operations
@pytest.mark.parametrize("P,C", [(1, 4), (7, 8), (77, 132)])
def test_batchnorm_references_are_torchs(P, C):
    x = _rand((P, C), 1) * 1.7 + 0.3
    gamma, beta = 1 + 0.2 * _rand((C,), 2), 0.1 * _rand((C,), 3)
    rm, rv = 0.1 * _rand((C,), 4), 1 + 0.1 * _rand((C,), 5).abs()
    eps, mom = 1e-3, 0.01
    ref = E.bn_stats(x, eps, mom, rm, rv)
    x64 = x.double().t().reshape(1, C, P, 1).clone().requires_grad_(True)
    ga64, be64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    trm, trv = rm.double().clone(), rv.double().clone()
    if P > 1:                                                  # (torch refuses one value per channel in training mode)
        y = F.batch_norm(x64, trm, trv, ga64, be64, training=True, momentum=E.f32(mom), eps=E.f32(eps))
        _same(ref["running_mean"], trm, "running_mean")
        _same(ref["running_var"], trv, "running_var")
    else:
        y = (x64 - x64) * ga64.view(1, C, 1, 1) + be64.view(1, C, 1, 1)
        assert float(ref["var"].abs().max()) == 0.0 and torch.equal(ref["running_var"], (1.0 - E.f32(mom)) * rv.double())
    got, _ = E.bn_apply(x, ref["mean"], ref["invstd"], gamma, beta, 1.0)
    _same(got, y.detach().reshape(C, P).t(), "affine")
    for slope in (0.2, 0.01):
        got, terms = E.bn_apply(x, ref["mean"], ref["invstd"], gamma, beta, slope)
        _same(got, F.leaky_relu(y.detach(), E.f32(slope)).reshape(C, P).t(), f"lrelu {slope}")
        assert bool((terms >= got.abs() * (1 - 1e-12)).all())
    g = _rand((P, C), 6)
    y.backward(g.double().t().reshape(1, C, P, 1))
    s0, s1 = E.bn_bwd_sums(g, x, ref["mean"], ref["invstd"])
    _same(s0, be64.grad, "sum g = dbeta")
    _same(s1, ga64.grad, "sum g xhat = dgamma")
    dx, terms = E.bn_bwd_dx(g, x, ref["mean"], ref["invstd"], gamma, s0, s1, P)
    if P > 1:
        _same(dx, x64.grad.reshape(C, P).t(), "dx")
    assert bool((terms >= dx.abs() * (1 - 1e-12)).all())
    wide = _rand((P, C + 8), 7)
    _same(E.colsum(wide[:, 4:4 + C]), wide.double()[:, 4:4 + C].sum(0), "column sums of a slice")


@pytest.mark.parametrize("target", [0.0, 1.0, 0.9])
def test_bce_reference_is_torchs(target):
    z = torch.cat([_rand((546,), 1) * 5, torch.tensor([0.0, 100.0, -100.0, 88.7, -88.7])])
    zg = z.double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(zg, torch.full_like(zg, E.f32(target)))
    ref.backward()
    loss, dz, terms = E.bce_logits(z, target)
    _same(loss, ref.detach(), "bce")
    _same(dz, zg.grad, "bce gradient")
    assert bool((terms >= dz.abs()).all())


def test_l1_reference_is_torchs():
    for sa, sb in (((2, 16, 14, 22), (2, 16, 13, 21)), ((2, 16, 13, 21), (2, 16, 14, 22)), ((1, 4, 5, 9), (1, 4, 7, 6))):
        a, b = _rand(sa, 2), _rand(sb, 3)
        h, w = min(sa[2], sb[2]), min(sa[3], sb[3])
        a[:, :, :h, :w][..., ::4] = b[:, :, :h, :w][..., ::4]          # ties: gradient exactly 0
        ag = a.double().requires_grad_(True)
        ref = F.l1_loss(ag[:, :, :h, :w], b.double()[:, :, :h, :w])
        ref.backward()
        loss, da = E.l1_crop(a, b)
        _same(loss, ref.detach(), "l1")
        _same(da, ag.grad, "l1 gradient")
        assert int((da[:, :, :h, :w] == 0).sum()) >= a[:, :, :h, :w].numel() // 4


@pytest.mark.parametrize("shape", [(1, 4, 1, 1), (2, 8, 1, 7), (2, 8, 5, 1), (1, 12, 5, 7)])
def test_bilinear_references_are_torchs(shape):
    x = _rand(shape, 3)
    xg = x.double().requires_grad_(True)
    ref = F.interpolate(xg, scale_factor=2, mode="bilinear")
    dout = _rand(tuple(ref.shape), 4)
    ref.backward(dout.double())
    out, terms = E.bilinear2x(x)
    _same(out, ref.detach(), "bilinear x2")
    assert bool((terms >= out.abs() * (1 - 1e-12)).all())
    dx, terms = E.bilinear2x_T(dout)
    _same(dx, xg.grad, "bilinear x2 transposed")
    assert bool((terms >= dx.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_sgd_reference_is_torchs(wd):
    lr, mom = 0.02, 0.9
    p = torch.nn.Parameter(_rand((1000,), 1, torch.float64))
    opt = torch.optim.SGD([p], lr=E.f32(lr), momentum=E.f32(mom), weight_decay=E.f32(wd))
    p.grad = _rand((1000,), 2, torch.float64)
    opt.step()                                                 # the first step creates the momentum buffers
    m = opt.state[p]["momentum_buffer"].clone()
    p0 = p.detach().clone()
    g = _rand((1000,), 3)
    p.grad = g.double() * 0.5                                  # gscale = 0.5 folded into the gradient
    opt.step()
    p2, m2, tp, tm = E.sgd_step(p0, g, m, lr, mom, wd, 0.5)
    _same(p2, p.detach(), "parameter")
    _same(m2, opt.state[p]["momentum_buffer"], "momentum buffer")
    assert bool((tp >= p2.abs() * (1 - 1e-12)).all()) and bool((tm >= m2.abs() * (1 - 1e-12)).all())


# ------------------------------------------------------------------------------------------------ (b) every case is on the branch it names
def test_launch_geometry():
    assert [E.ew_grid(n) for n in (0, 1, 256, 257, 2048 * 256, 2048 * 256 + 1)] == [1, 1, 1, 2, 2048, 2048]
    assert [E.red_geometry(P) for P in (1, 7, 64, 65, 77, 1537, 16384, 16385)] == [(1, 1), (1, 7), (1, 64), (2, 33), (2, 39), (25, 62), (256, 64), (253, 65)]
    assert [E.bce_grid(n) for n in (1, 255, 65536, 70001)] == [1, 1, 256, 256]
    assert E.sgd_grid(131077, 3) == (512, 3) and E.sgd_grid(1000, 3) == (4, 3) and E.sgd_grid(0, 1) == (1, 1)
    for P in (1, 7, 77, 1537, 16385):
        chunks, rpc = E.red_geometry(P)
        assert (chunks - 1) * rpc < P <= chunks * rpc and chunks <= E.RED_MAX_CHUNKS
        assert E.add_chain_depth(P) >= 18


def test_every_case_is_on_its_branch_and_every_branch_has_a_case():
    for P, C, want in E.STATS_SHAPES:
        assert E.red_path_of(P, C) == want, (P, C, sorted(E.red_path_of(P, C)))
    assert frozenset().union(*(w for _, _, w in E.STATS_SHAPES)) == frozenset(E.RED_PATHS)
    for P, C, want_apply, want_bwd in E.APPLY_SHAPES:
        assert E.branch_of("bn_apply", P, C) == want_apply, (P, C, sorted(E.branch_of("bn_apply", P, C)))
        assert E.branch_of("bn_bwd_apply", P, C) == want_bwd, (P, C, sorted(E.branch_of("bn_bwd_apply", P, C)))
    for col in (2, 3):
        seen = [row[col] for row in E.APPLY_SHAPES]
        assert frozenset().union(*seen) == frozenset(E.BRANCHES)
        assert any("fallback" in s and "grid_stride" in s for s in seen) and any("fallback" in s and "grid_stride" not in s for s in seen)
    # the largest case: all 524288 threads run apply's 4-way loop once, the first 14848 also its tail
    P, C = 16500, 512
    total4, stride = P * C // 4, 256 * E.ew_grid(P * C // 4)
    assert stride == 524288 and total4 - 3 * stride > stride and total4 - 4 * stride == 14848
    # flat ops: one case per op takes a second item per thread, one does not
    flat = [("bce", n, 1, w) for n, w in E.BCE_N]
    flat += [("l1", s[0] * s[2] * s[3], s[1], w) for s, w in E.L1_SHAPES]
    flat += [("bilinear_fwd", s[0] * s[2] * s[3], s[1], w) for s, w in E.BILINEAR_FWD_SHAPES]
    flat += [("bilinear_bwd", s[0] * s[2] * s[3], s[1], w) for s, w in E.BILINEAR_BWD_SHAPES]
    flat += [("sgd", max(E.SGD_SIZES), 1, E.SGD_BRANCH), ("sgd", 1000, 1, E.S())]
    for op, P, C, want in flat:
        assert E.branch_of(op, P, C) == want, (op, P, C)
    for op in ("bce", "l1", "bilinear_fwd", "bilinear_bwd", "sgd"):
        assert {w for o, _, _, w in flat if o == op} == {E.S(), E.S("grid_stride")}, op
    assert E.SGD_SIZES[-1] == max(E.SGD_SIZES)                # max_n belongs to the last tensor


# ------------------------------------------------------------------------------------------------ (c) the inputs admit the 1-ulp bar
@pytest.mark.parametrize("family", E.STATS_FAMILIES)
def test_shifted_one_pass_statistics_admit_the_one_ulp_bar(family):
    for P, C, _ in E.STATS_SHAPES:
        x = E.stats_input(family, P, C)
        ref = E.bn_stats(x, 1e-5)
        for order in ("plain", "kernel") + (("serial",) if P <= 1537 else ()):
            mean, var = E.bn_stats_shifted_one_pass(x, order)
            invstd = 1.0 / torch.sqrt(var + E.f32(1e-5))
            for name, got in (("mean", mean), ("var", var), ("invstd", invstd)):
                u = float(E.ulps_from(got.float(), ref[name]).max())
                assert u <= 1.0, f"{family} {P}x{C} {order} {name}: {u} ulp"
        if family == "const_channel":
            assert float(ref["var"][1]) == 0.0 and float(ref["mean"][1]) == E.CONST_VALUE
