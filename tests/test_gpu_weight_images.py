"""The f16x3 weight images of the Winograd convs, built straight from w (the default: the grouped builder of csrc/winograd.hip -- maxima pass,
transform + split in registers, header written by the kernel) against the three-launch path they replace (bit 1 of option f16_presplit,
value 3: header fill, fp32 weight transform, split; the planes of the activations are pre-split as under the default 1 either way).  The two must produce the same BYTES: every comparison here is on
integers, with no tolerance.

Each side runs on a context of its own with a caller-owned weight cache that starts as one NaN bit pattern everywhere, so the cache bytes
compare whole: the images, their headers, where each image sits and every byte neither path may touch.

  per-op       afi_conv3x3_wino_fwd / _infer / _dgrad, weights (Cout, Cin) = (128,128), (256,128), (128,384), (512,256) -- the smallest
               tile-aligned shapes, a non-square pair each way and the K = 384 of the dense blocks' last conv -- on 1x32x32 (F(2x2)) and
               2x64x64 (8192 pixels: F(4x4) for _infer and _dgrad).  One weight element is 2^6 above the rest: a wrong maximum moves every
               plane's scale.
  whole nets   under deterministic = 1: Discriminator(in_filters=128) forward (training) + backward at 2x64x64 and 1x32x32 -- its three
               convs are three jobs of different size in one builder launch -- and the interpolator forward + backward at 1x256x48x48.
               Outputs, every gradient and the cache bytes are equal; a second call changes no cache byte (the interpolator: a third -- its
               second small-map forward still adds the packed conv-transpose weight, which is no Winograd image; the two sides are compared
               after that call too); after an invalidate and changed weights both sides follow the new weights (they equal a context that
               has no cache at all).  The calls of one side reuse one workspace per size, as an engine does: the interpolator keys one
               image by an address inside its forward workspace.
  table edges  one image of the call already in the cache (a hit among misses); a cache with room for the first two images of the call only.
"""
import ctypes as C
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
CACHE_FLOATS = 48 * 1024 * 1024          # D(128) at 2x64x64: 22.1 M floats of forward images + 23.0 M of data-gradient images


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


class _Side:
    """a context whose weight images are built the old way (build = 0: f16_presplit = 3) or directly (1: the default), with its own NaN-filled
    weight cache; None: the default context settings and no cache"""

    def __init__(self, build, floats=CACHE_FLOATS, deterministic=True):
        from afigan_amd import _lib
        self.lib = _lib
        self.cx = _lib.Ctx("f16x3")
        if deterministic:
            self.cx.set_option("deterministic", 1)
        self.cache = None
        self.pool = {}                   # workspaces of this side's whole-net calls, by size (_fwd_bwd)
        if build is not None:
            self.cx.set_option("f16_presplit", 1 if build else 3)
            self.cache = torch.full((floats,), NAN, device="cuda")
            _lib.call("afi_ctx_set_wino_weight_cache", self.cx.handle, C.c_void_p(self.cache.data_ptr()), floats)

    def bits(self):
        return self.cache.view(torch.int32)

    def invalidate(self):
        self.lib.call("afi_ctx_wino_weight_cache_invalidate", self.cx.handle)

    def close(self):
        if self.cache is not None:
            self.lib.call("afi_ctx_set_wino_weight_cache", self.cx.handle, C.c_void_p(None), 0)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ per-op
def _planted_weight(ops, Cout, Cin, seed):
    w = _rand((Cout, Cin, 3, 3), seed) / (9 * Cin) ** 0.5
    w[Cout // 3, Cin // 5, 1, 2] = float(w.abs().max()) * 64.0
    return ops.ohwi(w.cuda()).clone(memory_format=torch.preserve_format)


def _conv_once(amd, side, ep, x, wd, N, H, W, Cin, Cout):
    from afigan_amd import _lib
    ops, lib = amd.ops, _lib.load()
    n = lib.afi_conv3x3_wino_ws_floats(N, H, W, Cin, Cout)
    ws = torch.full((int(n),), NAN, device="cuda")
    out = ops.new_pixel_major(N, Cin if ep == "dgrad" else Cout, H, W, "cuda")
    out.fill_(NAN)
    with _lib.use_ctx(side.cx):
        if ep == "fwd":
            _lib.call("afi_conv3x3_wino_fwd", ops.view_of(x), N, H, W, Cin, ops._p(wd), ops._p(None), Cout, ops.view_of(out), ops._p(ws), n, ops.stream_ptr())
        elif ep == "infer":
            _lib.call("afi_conv3x3_wino_infer", ops.view_of(x), N, H, W, Cin, ops._p(wd), ops._p(None), Cout, ops.view_of(out), 0, ops._p(ws), n, ops.stream_ptr())
        else:
            _lib.call("afi_conv3x3_wino_dgrad", ops.view_of(x), N, H, W, Cout, ops._p(wd), Cin, ops.view_of(out), ops._NULL_VIEW, ops._p(ws), n, ops.stream_ptr())
    return out


@pytest.fixture(scope="module")
def op_sides(amd):
    sides = (_Side(0, 8 * 1024 * 1024, deterministic=False), _Side(1, 8 * 1024 * 1024, deterministic=False))
    yield sides
    for s in sides:
        s.close()


@pytest.mark.parametrize("N,H,W", [(1, 32, 32), (2, 64, 64)], ids=["1x32x32", "2x64x64"])
@pytest.mark.parametrize("Cout,Cin", [(128, 128), (256, 128), (128, 384), (512, 256)])
@pytest.mark.parametrize("ep", ["fwd", "infer", "dgrad"])
def test_conv_image_and_output_bits(amd, op_sides, ep, Cout, Cin, N, H, W):
    ops = amd.ops
    wd = _planted_weight(ops, Cout, Cin, 3)
    x = _rand((N, Cout if ep == "dgrad" else Cin, H, W), 5).cuda().contiguous(memory_format=torch.channels_last)
    outs = []
    for s in op_sides:
        s.invalidate()
        s.cache.fill_(NAN)
        outs.append(_conv_once(amd, s, ep, x, wd, N, H, W, Cin, Cout))
    assert torch.isfinite(outs[0]).all()
    assert not torch.isnan(op_sides[0].cache).all(), "the registered cache was not written"
    assert _same_bits(outs[0], outs[1]), "conv outputs differ between the two builds of the images"
    assert torch.equal(op_sides[0].bits(), op_sides[1].bits()), "cache bytes differ between the two builds of the images"


# ------------------------------------------------------------------------------------------------ whole nets
def _twin(make, seed):
    """two modules with the same values (each keeps its own buffers: BatchNorm statistics move in a training forward)"""
    torch.manual_seed(seed)
    a = make().cuda()
    b = make().cuda()
    b.load_state_dict(a.state_dict())
    return a.train(), b.train()


def _fwd_bwd(side, net, x, dy):
    """forward + backward of `net` on side's context: (output, dx, parameter gradients by name)"""
    for p in net.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    import afigan_amd.ops as ops
    fresh = ops.new_workspace

    def pooled(floats, device):
        # one workspace per size and side, as an engine keeps them: the interpolator keys the image of its packed conv-transpose weight by
        # the address of that weight INSIDE the forward workspace, so only a call on the same workspace can find it again
        if int(floats) not in side.pool:
            side.pool[int(floats)] = fresh(floats, device)
        return side.pool[int(floats)]

    with side.lib.use_ctx(side.cx), mock.patch.object(ops, "new_workspace", pooled):
        out = net(xg)
        out.backward(dy)
    torch.cuda.synchronize()
    return out.detach(), xg.grad.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def _assert_runs_equal(a, b, what):
    assert _same_bits(a[0], b[0]), f"{what}: outputs differ"
    assert _same_bits(a[1], b[1]), f"{what}: input gradients differ"
    assert set(a[2]) == set(b[2]) and a[2], what
    for k in a[2]:
        assert _same_bits(a[2][k], b[2][k]), f"{what}: gradient of {k} differs"


def _net_case(amd, make, x, dy, seed, settle=0):
    sides = (_Side(0), _Side(1), _Side(None))
    try:
        na, nb = _twin(make, seed)
        _, nc = _twin(make, seed)
        nc.load_state_dict(na.state_dict())
        r0, r1 = _fwd_bwd(sides[0], na, x, dy), _fwd_bwd(sides[1], nb, x, dy)
        assert all(torch.isfinite(t).all() for t in (r0[0], r0[1]))
        assert not torch.isnan(sides[0].cache).all(), "the registered cache was not written"
        _assert_runs_equal(r0, r1, "first call")
        assert torch.equal(sides[0].bits(), sides[1].bits()), "cache bytes differ between the two builds of the images"
        # a further call finds every image: no cache byte moves.  `settle` calls come first where a call on a filled cache still adds an entry
        # that is no Winograd image (the interpolator's small-map forward: once its conv-transpose image is a hit it asks for the packed
        # fp32 conv-transpose weight, which the launch that built the image had written as a by-product); the two sides stay equal through them
        for _ in range(settle):
            _fwd_bwd(sides[0], na, x, dy), _fwd_bwd(sides[1], nb, x, dy)
            assert torch.equal(sides[0].bits(), sides[1].bits()), "cache bytes differ between the two builds of the images"
        snap = sides[1].cache.clone()
        _fwd_bwd(sides[1], nb, x, dy)
        assert torch.equal(snap.view(torch.int32), sides[1].bits()), "a call on a filled cache changed cache bytes"
        # changed weights behind an invalidate: both sides follow them, as a context without a cache does
        with torch.no_grad():
            for n_ in (na, nb, nc):
                g = torch.Generator().manual_seed(77)
                for p in n_.parameters():
                    if p.dim() == 4:
                        p.mul_(1.0 + 0.25 * torch.rand(p.shape, generator=g).to(p.device))
        for s in sides[:2]:
            s.invalidate()
        q0, q1, qc = _fwd_bwd(sides[0], na, x, dy), _fwd_bwd(sides[1], nb, x, dy), _fwd_bwd(sides[2], nc, x, dy)
        assert not _same_bits(q0[0], r0[0]), "the changed weights changed nothing"
        _assert_runs_equal(q0, q1, "after invalidate")
        _assert_runs_equal(qc, q1, "after invalidate, against a context without a cache")
        assert torch.equal(sides[0].bits(), sides[1].bits()), "cache bytes differ after the invalidate"
    finally:
        for s in sides:
            s.close()


@pytest.mark.parametrize("N,H,W", [(2, 64, 64), (1, 32, 32)], ids=["2x64x64", "1x32x32"])
def test_discriminator_bits(amd, N, H, W):
    x = _rand((N, 128, H, W), 11).cuda()
    dy = _rand((N, 1, H, W), 12).cuda()
    _net_case(amd, lambda: amd.Discriminator(in_filters=128), x, dy, 21)


def test_interpolator_bits(amd):
    x = _rand((1, 256, 48, 48), 13).cuda()
    dy = _rand((1, 256, 96, 96), 14).cuda()
    _net_case(amd, lambda: amd.Generator(n_residual_dense_blocks=1), x, dy, 22, settle=1)


# ------------------------------------------------------------------------------------------------ job-table edges
def _d_case(amd, floats, prime):
    """D(128) forward + backward at 1x32x32 (every conv on F(2x2)) on both sides with caches of `floats`; prime: first run block 1's conv
    alone through afi_conv3x3_wino_fwd, so that the forward's table holds one hit between two misses"""
    N, H, W = 1, 32, 32
    x = _rand((N, 128, H, W), 31).cuda()
    dy = _rand((N, 1, H, W), 32).cuda()
    sides = (_Side(0, floats), _Side(1, floats), _Side(None))
    try:
        na, nb = _twin(lambda: amd.Discriminator(in_filters=128), 41)
        _, nc = _twin(lambda: amd.Discriminator(in_filters=128), 41)
        nc.load_state_dict(na.state_dict())
        if prime:
            y0 = _rand((N, 256, H, W), 33).cuda().contiguous(memory_format=torch.channels_last)
            for s, n_ in zip(sides[:2], (na, nb)):
                _conv_once(amd, s, "fwd", y0, n_.Discriminators[0][1][0].weight.detach(), N, H, W, 256, 512)
            assert torch.equal(sides[0].bits(), sides[1].bits())
        r0, r1, rc = _fwd_bwd(sides[0], na, x, dy), _fwd_bwd(sides[1], nb, x, dy), _fwd_bwd(sides[2], nc, x, dy)
        _assert_runs_equal(r0, r1, "option 0 against option 1")
        _assert_runs_equal(rc, r1, "against a context without a cache")
        assert torch.equal(sides[0].bits(), sides[1].bits()), "cache bytes differ between the two builds of the images"
        return sides[1].cache.clone()
    finally:
        for s in sides:
            s.close()


def test_one_hit_among_misses(amd):
    cache = _d_case(amd, CACHE_FLOATS, prime=True)
    assert not torch.isnan(cache).all()


def test_cache_with_room_for_part_of_a_call(amd):
    # F(2x2) forward images of D(128): 1.5 x 16 x K x Nc floats each: 128x256 and 256x512 fit, 512x512 (6.3 M floats) does not, and
    # nothing of the backward's does
    room = 24 * (128 * 256 + 256 * 512) + 4096
    cache = _d_case(amd, room, prime=False)
    used = (~torch.isnan(cache)).nonzero().max().item()
    assert 24 * 128 * 256 < used < room, "the cache holds the first two images of the call and no more"
