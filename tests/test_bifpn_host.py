"""CPU-side checks of tests/bifpn_f64.py, the float64 yardstick of test_gpu_bifpn_kernels.py: (a) every reference against torch's own float64
ops and autograd to 1e-12, the max-pool taps against the routing of torch.autograd on random, all-negative, all-zero and tied inputs; (b) every
case of the tables takes the paths it names, the cases of an op together reach every path that op has, and the caps the C-ABI exposes equal
their mirrors -- a retuned cap or an edited shape fails here, without a GPU; (c) every fusion-backward case leaves |dw_k| at least a tenth of
sum |ds x_k|, so its relative bar means something; (d) terms bound the result element by element; (e) the depthwise and max-pool entry points
refuse a view their 16-byte loads cannot take before anything is launched."""
import pytest
import torch
import torch.nn.functional as F

import bifpn_f64 as B
from oracle import afigan_oracle as orc

TOL = 1e-12
SMALL = [(1, 4, 1, 1), (1, 8, 1, 7), (2, 8, 5, 1), (2, 12, 6, 5), (2, 132, 7, 9)]
SMALL_POOL = [(1, 4, 2, 2), (1, 8, 2, 5), (2, 8, 5, 2), (2, 12, 6, 5), (2, 12, 8, 6), (2, 132, 7, 9)]


def _same(got, ref, what):
    scale = max(float(ref.abs().max()), 1e-300)
    err = float((got - ref).abs().max())
    assert got.shape == ref.shape and err <= TOL * scale, f"{what}: {err:.3e} against scale {scale:.3e}"


def _bounded(terms, result, what):
    assert terms.shape == result.shape and bool((terms >= result.abs() * (1 - 1e-12)).all()), f"{what}: terms below |result|"   # (d)


# ------------------------------------------------------------------------------------------------ (a) the references are the operations
@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("n_in", [3, 2])
def test_fusion_references_are_torchs(shape, n_in):
    w = torch.tensor(B.SWISH_W3[:n_in])
    xs = [B.rand(shape, 10 + k) for k in range(n_in)]
    c = xs[2] if n_in == 3 else None
    dout = B.rand(shape, 14)
    w64 = w.double().requires_grad_(True)
    x64 = [x.double().requires_grad_(True) for x in xs]
    ref = orc.swish(sum(w64[k] * x for k, x in enumerate(x64)))
    grads = torch.autograd.grad((ref * dout.double()).sum(), [w64] + x64)
    out, terms = B.fuse_swish(w, xs[0], xs[1], c)
    _same(out, ref.detach(), "fuse_swish")
    _bounded(terms, out, "fuse_swish")
    (dw, *dx), (tw, *tx) = B.fuse_swish_bwd(w, xs[0], xs[1], c, dout)
    _same(dw, grads[0], "dw")
    _bounded(tw, dw, "dw")
    for k in range(n_in):
        _same(dx[k], grads[1 + k], f"d input {k}")
        _bounded(tx[k], dx[k], f"d input {k}")
    assert n_in == 3 or (dx[2] is None and tx[2] is None)
    # the gains of the exponential are the derivatives with respect to ln e: a central difference in float64
    s = sum(float(w[k]) * xs[k].double() for k in range(n_in))
    h = 1e-6
    sw = lambda q: s / (1 + torch.exp(-s) * (1 + q))
    a_s, gain = B.fuse_swish_exp(w, xs[0], xs[1], c)
    assert torch.equal(a_s, s.abs())
    assert float(((sw(h) - sw(-h)).abs() / (2 * h) - gain).abs().max()) <= 1e-8 * max(1.0, float(gain.max()))

    def dsw(q):
        sg = 1 / (1 + torch.exp(-s) * (1 + q))
        return dout.double() * sg * (1 + s * (1 - sg))
    _, gain = B.fuse_swish_bwd_exp(w, xs[0], xs[1], c, dout)
    assert float(((dsw(h) - dsw(-h)).abs() / (2 * h) - gain).abs().max()) <= 1e-8 * max(1.0, float(gain.max()))


@pytest.mark.parametrize("shape", SMALL)
def test_depthwise_references_are_torchs(shape):
    N, Cc, H, W = shape
    x, dy = B.rand(shape, 1), B.rand(shape, 2)
    wdw = B.rand((Cc, 1, 3, 3), 3)
    w9c = wdw.reshape(Cc, 9).t().contiguous()
    x64, w64 = x.double().requires_grad_(True), wdw.double().requires_grad_(True)
    ref = F.conv2d(F.pad(x64, (1, 1, 1, 1)), w64, None, 1, 0, 1, Cc)
    gx, gw = torch.autograd.grad((ref * dy.double()).sum(), (x64, w64))
    out, terms = B.dwconv3x3(x, w9c)
    _same(out, ref.detach(), "dwconv3x3")
    _bounded(terms, out, "dwconv3x3")
    dx, terms = B.dwconv3x3(dy, w9c.flip(0).contiguous())       # the input gradient: the forward on dy with rows 8..0
    _same(dx, gx, "dwconv3x3 input gradient")
    _bounded(terms, dx, "dwconv3x3 input gradient")
    dw, terms = B.dwconv3x3_wgrad(dy, x)
    _same(dw, gw.reshape(Cc, 9).t(), "dwconv3x3 weight gradient")
    _bounded(terms, dw, "dwconv3x3 weight gradient")


@pytest.mark.parametrize("family", B.POOL_FAMILIES)
@pytest.mark.parametrize("shape", SMALL_POOL)
def test_maxpool_taps_route_as_autograd(shape, family):
    x = B.pool_input(family, shape)
    for dt in (torch.float32, torch.float64):
        xs = x.to(dt).clone().requires_grad_(True)
        ref = orc.maxpool3s2_same(xs)
        assert torch.equal(ref, F.max_pool2d(F.pad(xs, (0, 1, 0, 1)), 3, 2))
        dout = B.rand(ref.shape, 5)
        (gx,) = torch.autograd.grad((ref * dout.to(dt)).sum(), xs)
        val, tap = B.maxpool3s2_same(x.to(dt))
        assert val.dtype == dt and tap.dtype == torch.uint8 and int(tap.max()) <= 8
        assert torch.equal(val, ref.detach())
        dx, terms = B.maxpool3s2_same_bwd(dout, tap, shape[2:])
        _same(dx, gx.double(), f"max-pool backward ({family})") if dt == torch.float64 else None
        assert bool((dx - gx.double()).abs().max() <= 4 * B.EPS * terms.max().clamp_min(1e-300))          # (fp32 autograd adds in fp32)
        _bounded(terms, dx, "max-pool backward")
    v2, none = B.maxpool3s2_same(x, want_taps=False)
    assert none is None and torch.equal(B.bits(v2), B.bits(val.float()))
    if family == "zeros":
        assert int(tap.max()) == 0 and float(dx.abs().sum()) == float(dout.double().abs().sum() - _pad_won(dout, tap, shape).abs().sum())
    if family == "negative" and shape[2] % 2 == 0 and shape[3] % 2 == 0:
        assert float(val[:, :, -1, :].abs().max()) == 0.0 and float(val[:, :, :, -1].abs().max()) == 0.0         # the pad won the border


def _pad_won(dout, tap, shape):
    """the cotangents of the windows whose tap lies in the pad row / column"""
    H, W = shape[2:]
    oy = torch.arange(tap.shape[2]).view(1, 1, -1, 1)
    ox = torch.arange(tap.shape[3]).view(1, 1, 1, -1)
    t = tap.long()
    pad = (2 * oy + t // 3 >= H) | (2 * ox + t % 3 >= W)
    return dout.double() * pad


@pytest.mark.parametrize("shape", SMALL)
def test_pass_through_references_are_torchs(shape):
    N, Cc, H, W = shape
    x, g = B.rand(shape, 1), B.rand(shape, 2)
    for scale in (1.0, 0.25, 1.0 / 3):
        a64 = x.double().requires_grad_(True)
        (gx,) = torch.autograd.grad((F.relu(a64) * g.double()).sum(), a64)
        out, terms = B.relu_bwd(g, F.relu(x), scale)
        _same(out, B.f32(scale) * gx, "relu_bwd")
        _bounded(terms, out, "relu_bwd")
    assert torch.equal(B.nearest(x, 2, 1), F.interpolate(x, scale_factor=2, mode="nearest"))
    assert torch.equal(B.nearest(x, 1, 2), F.max_pool2d(x, 1, 2, ceil_mode=True))
    assert B.nearest(x, 3, 2).shape == (N, Cc, B.nearest_out(H, 3, 2), B.nearest_out(W, 3, 2))
    x3 = x.reshape(N, Cc, H * W)
    assert torch.equal(B.nhwc_to_nchw(B.nchw_to_nhwc(x3)), x3) and B.nchw_to_nhwc(x3).shape == (N, H * W, Cc)
    assert torch.equal(B.nchw_to_nhwc(x3)[:, :, 0], x3[:, 0, :])


# ------------------------------------------------------------------------------------------------ (b) every case takes the paths it is there for
ALL_CASES = [(op, shape, paths) for op, cases in B.CASES.items() for shape, paths in cases]


@pytest.mark.parametrize("op,shape,paths", ALL_CASES, ids=lambda v: str(v) if not isinstance(v, frozenset) else "")
def test_cases_take_their_paths(op, shape, paths):
    assert B.path_of(op, shape) == paths, (op, shape, sorted(B.path_of(op, shape)), sorted(paths))
    assert paths <= set(B.PATHS[op])


@pytest.mark.parametrize("op", sorted(B.PATHS))
def test_cases_reach_every_path(op):
    if op in B.TILE:
        shapes = [(n, c, p) for n in B.TRANSPOSE_N for c in B.TRANSPOSE_C for p in B.TRANSPOSE_P]
    else:
        shapes = [s for s, _ in B.CASES[op]]
    reached = frozenset().union(*(B.path_of(op, s) for s in shapes))
    assert reached == frozenset(B.PATHS[op]), (op, sorted(set(B.PATHS[op]) - reached))


def test_geometry_of_the_large_shapes():
    """the figures the case tables are built on, spelled out"""
    assert B.bt_grid(1) == 1 and B.bt_grid(262144) == 1024 and B.bt_grid(262145) == 1024 and B.bt_grid(0) == 1
    assert B.ew_grid(558030) == B.EW_GRID_CAP == 2048 and 558030 > 2048 * 256 and 558030 > 2 * 1024 * 256
    assert 2 * 33 * 67 * 63 == 278586 and 278586 - 1024 * 256 == 16442
    assert B.dww_geometry(2 * 67 * 63) == (132, 64) and 2 * 67 * 63 - 131 * 64 == 58
    assert B.dww_geometry(2 * 95 * 89) == (253, 67) and 2 * 95 * 89 - 252 * 67 == 26 and (95 * 89) // 67 == 126 and (95 * 89) % 67
    assert B.dww_geometry(126) == (2, 63) and B.dww_geometry(16384) == (256, 64) and B.dww_geometry(16385)[1] == 65 and B.dww_geometry(1) == (1, 1)
    assert 2 * 67 * 62 * 33 == 274164 > 1024 * 256 and 2 * 95 * 88 * 33 == 551760 > 2048 * 256
    assert B.nearest_grid(254 * 250 * 33) == 8186 and 256 * 250 * 33 > 8192 * 256 and B.nearest_grid(256 * 250 * 33) == 8192


def _lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from afigan_amd import _lib
    return _lib, _lib.load()


def test_caps_equal_the_librarys():
    """the two caps the C-ABI states through its scratch sizes (host-only functions)"""
    _, lib = _lib()
    assert lib.afi_fuse_swish_bwd_scratch_floats() == 4 * B.BT_GRID_CAP
    for Cc in (4, 132, 256):
        assert lib.afi_dwconv3x3_wgrad_scratch_floats(Cc) == B.DWW_MAX_CHUNKS * 9 * Cc


# ------------------------------------------------------------------------------------------------ (c) dw_k is well conditioned in every case
@pytest.mark.parametrize("shape", [s for s, _ in B.CASES["fuse_swish_bwd"]], ids=str)
@pytest.mark.parametrize("n_in", [3, 2])
def test_fusion_weight_gradient_is_well_conditioned(shape, n_in):
    w, a, b, c, dout = B.swish_bwd_inputs(shape, n_in)
    (dw, *dx), (tw, *tx) = B.fuse_swish_bwd(w, a, b, c, dout)
    assert bool((dw.abs() >= 0.1 * tw).all()), (dw / tw).tolist()
    for k in range(n_in):
        _bounded(tx[k], dx[k], f"d input {k}")
    s = sum(float(w[k]) * t.double() for k, t in enumerate((a, b, c)[:n_in]))
    assert float(s.min()) < -1.5 and float(s.max()) > 1.5 or s.numel() < 1000      # both tails of the swish, where there are elements enough


# ------------------------------------------------------------------------------------------------ (e) views the 16-byte loads cannot take
def test_depthwise_and_maxpool_refuse_a_misaligned_view():
    """AFI_ERR_UNSUPPORTED (2), decided on the host before any launch: the pointers are made up, so every call here must be refused.
    Each call has exactly one thing wrong."""
    L, lib = _lib()
    UNSUPPORTED, BAD_ARG = L.DEFINES["AFI_ERR_UNSUPPORTED"], L.DEFINES["AFI_ERR_BAD_ARG"]
    N, H, W, Cc, Cw = 1, 4, 6, 8, 16
    base, w, out, idx = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    good = (base, H * W * Cw, W * Cw, Cw)
    bad_views = [(base + 4, *good[1:]), (base + 8, *good[1:]), (base, good[1] + 2, good[2], good[3]), (base, good[1], good[2] + 1, good[3]),
                 (base, good[1], good[2], good[3] + 3)]
    for p, sN, sH, sW in bad_views:
        v = L.View(p, sN, sH, sW)
        assert lib.afi_dwconv3x3_fwd(v, N, H, W, Cc, w, out, None) == UNSUPPORTED
        assert lib.afi_maxpool3s2_same_fwd(v, N, H, W, Cc, out, None) == UNSUPPORTED
        assert lib.afi_maxpool3s2_same_fwd_idx(v, N, H, W, Cc, out, idx, None) == UNSUPPORTED
    v = L.View(*good)
    assert lib.afi_dwconv3x3_fwd(v, N, H, W, Cc, w + 4, out, None) == UNSUPPORTED
    assert lib.afi_dwconv3x3_fwd(v, N, H, W, Cc, w, out + 8, None) == UNSUPPORTED
    assert lib.afi_maxpool3s2_same_fwd(v, N, H, W, Cc, out + 4, None) == UNSUPPORTED
    assert lib.afi_maxpool3s2_same_fwd_idx(v, N, H, W, Cc, out + 4, idx, None) == UNSUPPORTED
    assert lib.afi_maxpool3s2_same_fwd_idx(v, N, H, W, Cc, out, idx + 2, None) == UNSUPPORTED
    assert lib.afi_dwconv3x3_fwd(v, N, H, W, Cc + 2, w, out, None) == UNSUPPORTED
    null = L.View(None, *good[1:])
    assert lib.afi_dwconv3x3_fwd(null, N, H, W, Cc, w, out, None) == BAD_ARG and lib.afi_dwconv3x3_fwd(v, N, H, W, Cc, None, out, None) == BAD_ARG
    assert lib.afi_maxpool3s2_same_fwd(null, N, H, W, Cc, out, None) == BAD_ARG and lib.afi_maxpool3s2_same_fwd(v, N, H, W, Cc, None, None) == BAD_ARG
    assert lib.afi_maxpool3s2_same_fwd_idx(null, N, H, W, Cc, out, idx, None) == BAD_ARG
    assert lib.afi_nearest_nhwc(L.View(base + 4, *good[1:]), N, H, W, Cc, 2, 1, out, None) == UNSUPPORTED          # the model of these refusals
