"""The trainable ResNeSt bottom-up on the GPU against float64: the split-attention backward pass by pass, the transposed average
pools, single blocks, a small whole ResNeSt-50, determinism, the untouched frozen module, and the bottom-up under the AFI FPN and the detector
step.  Reference, closed forms and fixtures: tests/resnest_train_f64.py (their conditions are asserted on the CPU by
test_resnest_train_host.py).

Bars.  Sums over pixels / matrix-vector sums: elementwise_f64.reduction_bars with Ktot = their length (max-norm 2 sqrt(Ktot) 2^-24, rel. L2
4 x max(torch CPU fp32's, sqrt(Ktot) 2^-24 / 8)).  Element-wise results: elementwise_f64.elementwise_bar(terms, r), r the number of
roundings, counted beside each call.  Blocks and networks: every parameter gradient within 4 x the relative-L2 deviation of torch CPU fp32
autograd from fp64, per tensor (tests/test_gpu_resnet_train.py's rule); outputs within tests/test_gpu_resnest.py's 1e-3 relative L2."""
import numpy as np
import pytest
import torch

import elementwise_f64 as E
import resnest_train_f64 as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
FWD_BAR = 1e-3                           # tests/test_gpu_resnest.py: a network's features against fp64, relative L2


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _pm(t):
    return t.float().cuda().contiguous(memory_format=torch.channels_last)


def _du(dout, avd, H, W, dtype):
    return R.avg3s2p1_T(dout.to(dtype), H, W) if avd else dout.to(dtype)


def _hold_reduction(tag, got, ref64, ref32, ktot):
    (em, el), (_, cl) = E.errs(got, ref64), E.errs(ref32, ref64)
    bm, bl = E.reduction_bars(ktot, cl)
    print(f"[resnest-train] {tag:56s} Ktot {ktot:5d}  max-norm {em:.2e} (bar {bm:.2e})  rel-L2 {el:.2e} (cpu {cl:.2e}, bar {bl:.2e})")
    assert bool(torch.isfinite(got).all()) and em <= bm and el <= bl, (tag, em, bm, el, bl)


def _hold_elementwise(tag, got, ref64, terms, r):
    got = got.detach().double().cpu()
    bar = E.elementwise_bar(terms, r)
    worst = ((got - ref64).abs() / bar).max().item()
    print(f"[resnest-train] {tag:56s} r {r:2d}  worst error / bar {worst:.3f}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, (tag, worst)


def _forward_kept(amd, c):
    """the GPU forward's own (att, g, h) for a splat_case: what the backward passes are given"""
    ops = amd.ops
    out, att, g, h = ops.splat_attention(_pm(c["s0"]), _pm(c["s1"]), c["w1"].cuda(), c["b1"].cuda(), c["w2"].cuda(), c["b2"].cuda(),
                                         avd=c["dout"].shape[2] != c["s0"].shape[2], keep=True)
    return out, att, g, h


# ------------------------------------------------------------------------------------------------ 1. dots
DOT_SHAPES = [(8, 48, 44, False), (8, 48, 44, True), (256, 7, 10, False), (256, 7, 10, True), (1024, 3, 6, False), (1024, 3, 6, True),
              (8, 7, 9, True), (8, 8, 10, True)]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C,H,W,avd", DOT_SHAPES)
def test_dots_against_fp64(amd, C, H, W, avd, N):
    c = R.splat_case(N, C, max(C // 2, 32), H, W, avd)
    part = amd.ops.splat_bwd_dots(_pm(c["dout"]), _pm(c["s0"]), _pm(c["s1"]), avd)
    assert tuple(part.shape) == (N, R.gap_chunks(H, W, C)[0], 2, C)
    got = part.double().cpu().sum(1).reshape(N, 2 * C)                       # the chunks added in fp64: the kernel's own sums alone are judged
    ref = lambda dt: R.splat_bwd_da(_du(c["dout"], avd, H, W, dt), c["s0"].to(dt), c["s1"].to(dt))
    _hold_reduction(f"dots C{C} {H}x{W} avd{int(avd)} N{N}", got, ref(torch.float64), ref(torch.float32), H * W)


def test_dots_refuses_a_short_workspace(amd):
    ops, lib = amd.ops, amd._lib
    c = R.splat_case(1, 8, 32, 48, 44, False)
    d, s0, s1 = _pm(c["dout"]), _pm(c["s0"]), _pm(c["s1"])
    n = lib.load().afi_resnest_splat_bwd_ws_floats(1, 48, 44, 8)
    assert n == 2 * 2 * 8
    part = torch.zeros(n, device="cuda")
    with pytest.raises(amd.AfiError, match="status 4"):
        lib.call("afi_resnest_splat_bwd_dots", ops.view_of(d), ops.view_of(s0), ops.view_of(s1), 1, 48, 44, 8, 0, ops._p(part), n - 1, ops.stream_ptr())
    assert not bool(part.any())


# ------------------------------------------------------------------------------------------------ 2. attention backward and parameters
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C,I", [(8, 32), (256, 128), (1024, 512)])
def test_attention_backward_and_params_against_fp64(amd, C, I, N):
    """On the dots kernel's own sums (a cancellation in da0 - da1 is charged once), and each later quantity on the kernel's own earlier
    outputs.  5 x 6 maps: one chunk for C = 8 and 256, two for C = 1024."""
    ops = amd.ops
    H, W = 5, 6
    c = R.splat_case(N, C, I, H, W, False)
    _, att, g, h = _forward_kept(amd, c)
    part = ops.splat_bwd_dots(_pm(c["dout"]), _pm(c["s0"]), _pm(c["s1"]), False)
    dz, dh, dg = ops.splat_bwd_attn(part, (H, W), att, h, c["w1"].cuda(), c["w2"].cuda())
    d = lambda t: t.detach().double().cpu()
    tag = f"C{C} I{I} N{N}"
    # the live / dead fc1 units the fixture promises, in the kernel's own h
    assert bool(((h > 0).sum(1) > 0).all()) and bool(((h > 0).sum(1) < I).all())
    # dz: the chunk sums (at most 1 add each: 2 chunks), the subtraction, two products: r = 1 + 1 + 2 = 4
    chunks = d(part)
    da, mag = chunks.sum(1).reshape(N, 2 * C), chunks.abs().sum(1).reshape(N, 2 * C)
    a = d(att)
    terms = a[:, :C] * a[:, C:] * (mag[:, :C] + mag[:, C:])
    _hold_elementwise("dz " + tag, dz, R.splat_bwd_dz(da, a), torch.cat([terms, terms], 1), 4)
    assert torch.equal(dz[:, C:], -dz[:, :C])
    # dh: a sum of 2C products per unit on the kernel's dz; exact zeros at dead units
    ref = lambda dt: R.splat_bwd_dh(dz.cpu().to(dt), h.cpu().to(dt), c["w2"].to(dt))
    assert bool((dh[h <= 0] == 0).all())
    _hold_reduction("dh " + tag, dh, ref(torch.float64), ref(torch.float32), 2 * C)
    # dg: a sum of I products per channel on the kernel's dh, divided by HW
    ref = lambda dt: R.splat_bwd_dg(dh.cpu().to(dt), c["w1"].to(dt), H * W)
    _hold_reduction("dg " + tag, dg, ref(torch.float64), ref(torch.float32), I)
    # parameters, into non-zero gradients (+=)
    g0 = [_rand(s, 40 + i) for i, s in enumerate([(I, C), (I,), (2 * C, I), (2 * C,)])]
    dw1, db1, dw2, db2 = [t.clone().cuda() for t in g0]
    ops.splat_bwd_params(dz, dh, g, h, c["s1_scale"].cuda(), dw1, db1, dw2, db2)
    s1 = c["s1_scale"].double()
    p2, p1 = torch.einsum("no,nj->noj", d(dz), d(h)), torch.einsum("nj,nc->njc", d(dh), d(g))
    # dw2: N products and N adds (the last into the gradient): r = 2N
    _hold_elementwise("dw2 " + tag, dw2, g0[2].double() + p2.sum(0), g0[2].double().abs() + p2.abs().sum(0), 2 * N)
    # db2: N adds: r = N
    _hold_elementwise("db2 " + tag, db2, g0[3].double() + d(dz).sum(0), g0[3].double().abs() + d(dz).abs().sum(0), N)
    # dw1: N products, N - 1 adds, the scale, the add into the gradient: r = 2N + 1
    _hold_elementwise("dw1 " + tag, dw1, g0[0].double() + s1.view(-1, 1) * p1.sum(0), g0[0].double().abs() + s1.view(-1, 1) * p1.abs().sum(0),
                      2 * N + 1)
    # db1: N - 1 adds, the scale, the add into the gradient: r = N + 1
    _hold_elementwise("db1 " + tag, db1, g0[1].double() + s1 * d(dh).sum(0), g0[1].double().abs() + s1 * d(dh).abs().sum(0), N + 1)


# ------------------------------------------------------------------------------------------------ 3. combine backward and the transposed pools
@pytest.mark.parametrize("C,H,W,avd", [(8, 7, 9, False), (8, 7, 9, True), (8, 8, 10, True), (256, 7, 10, True), (1024, 3, 6, False)])
def test_combine_backward_against_fp64(amd, C, H, W, avd):
    """ds0 / ds1 are the two halves of one NaN-filled [N, 2C, H, W] tensor.  Without AVD: a product and a sum, r = 2; with AVD du is up to 3
    adds and a division first: r = 6."""
    N = 2
    c = R.splat_case(N, C, max(C // 2, 32), H, W, avd)
    att, dg = torch.softmax(_rand((N, 2, C), 1), 1).reshape(N, 2 * C), _rand((N, C), 2)
    both = _pm(torch.full((N, 2 * C, H, W), NAN))
    amd.ops.splat_bwd_combine(_pm(c["dout"]), _pm(c["s0"]), _pm(c["s1"]), att.cuda(), dg.cuda(), avd, ds0=both[:, :C], ds1=both[:, C:])
    du, dumag = _du(c["dout"], avd, H, W, torch.float64), _du(c["dout"].abs(), avd, H, W, torch.float64)
    for r, s in enumerate((c["s0"], c["s1"])):
        a, got = att[:, r * C:(r + 1) * C].double(), both[:, r * C:(r + 1) * C].cpu()
        assert bool((got[s <= 0] == 0).all()), "a masked element is not exactly zero"
        terms = (a.view(N, C, 1, 1) * dumag + dg.double().abs().view(N, C, 1, 1)) * (s > 0)
        _hold_elementwise(f"combine C{C} {H}x{W} avd{int(avd)} split {r}", got, R.splat_bwd_ds(du, s.double(), a, dg.double()), terms, 6 if avd else 2)


@pytest.mark.parametrize("H,W", [(7, 9), (8, 10), (1, 2)])
@pytest.mark.parametrize("mode", ["avg2s2_ceil", "avg3s2p1"])
def test_pool_backward_into_a_strided_view(amd, mode, H, W):
    """beta = 1 into every second pixel of a sentinel-filled map, with the ReLU mask; the pixels in between stay bit-equal.  avg2s2_ceil: a
    division and the add, r = 2; avg3s2p1: up to 3 adds, the division, the add, r = 5."""
    N, C = 2, 12
    dy, z, dx0 = _rand((N, C, (H + 1) // 2, (W + 1) // 2), 1), _rand((N, C, H, W), 2), _rand((N, C, H, W), 3)
    sentinel = 12345.678
    full0 = torch.full((N, C, 2 * H, 2 * W), sentinel)
    full0[:, :, ::2, ::2] = dx0
    full, zfull = _pm(full0), _pm(torch.zeros(N, C, 2 * H, 2 * W))
    zfull[:, :, ::2, ::2] = z.cuda()
    out = amd.ops.resnest_pool_bwd(_pm(dy), mode, dx=full[:, :, ::2, ::2], beta=1.0, z=zfull[:, :, ::2, ::2])
    assert out.data_ptr() == full.data_ptr()
    got = full.cpu()
    keep = torch.ones(2 * H, 2 * W, dtype=torch.bool)
    keep[::2, ::2] = False
    assert torch.equal(got[:, :, keep], full0[:, :, keep])
    T = R.avg2s2_ceil_T if mode == "avg2s2_ceil" else R.avg3s2p1_T
    live = z > 0
    ref, terms = (dx0.double() + T(dy.double(), H, W)) * live, (dx0.double().abs() + T(dy.double().abs(), H, W)) * live
    got = got[:, :, ::2, ::2]
    assert bool((got[~live] == 0).all())
    _hold_elementwise(f"pool_bwd {mode} {H}x{W}", got, ref, terms, 2 if mode == "avg2s2_ceil" else 5)


def test_pool_backward_beta_zero_and_the_refused_mode(amd):
    """beta = 0 never reads dx (NaN-filled going in), no mask; the max mode is refused by the library (status 2: unsupported)."""
    ops = amd.ops
    dy = _rand((1, 8, 4, 5), 1)
    for mode, T in (("avg2s2_ceil", R.avg2s2_ceil_T), ("avg3s2p1", R.avg3s2p1_T)):
        dx = _pm(torch.full((1, 8, 7, 9), NAN))
        ops.resnest_pool_bwd(_pm(dy), mode, dx=dx)
        _hold_elementwise(f"pool_bwd {mode} beta 0", dx, T(dy.double(), 7, 9), T(dy.double().abs(), 7, 9), 1 if mode == "avg2s2_ceil" else 4)
        assert torch.equal(ops.resnest_pool_bwd(_pm(dy), mode, in_hw=(7, 9)), dx)
    with pytest.raises(amd.AfiError, match="status 2"):
        ops.resnest_pool_bwd(_pm(dy), "max3s2p1", in_hw=(7, 9))


@pytest.mark.parametrize("H,W", [(7, 9), (8, 10)])
def test_fused_avd_gather_is_the_transposed_pool_pass(amd, H, W):
    """The du the split-attention passes gather is what afi_resnest_pool_bwd's avg3s2p1 mode writes: that pass is held to its bar (r = 4),
    and the combine with att = 1, dg = 0 and all-positive splits (1 * du + 0, both exact) is bit-equal to it."""
    ops = amd.ops
    N, C = 2, 8
    dout = _rand((N, C, (H + 1) // 2, (W + 1) // 2), 5)
    du = ops.resnest_pool_bwd(_pm(dout), "avg3s2p1", in_hw=(H, W))
    _hold_elementwise(f"avg3s2p1 transposed {H}x{W}", du, R.avg3s2p1_T(dout.double(), H, W), R.avg3s2p1_T(dout.double().abs(), H, W), 4)
    ones = _pm(torch.ones(N, C, H, W))
    ds0, ds1 = ops.splat_bwd_combine(_pm(dout), ones, ones, torch.ones(N, 2 * C).cuda(), torch.zeros(N, C).cuda(), True)
    assert torch.equal(ds0, du) and torch.equal(ds1, du)


# ------------------------------------------------------------------------------------------------ 4. single blocks
class _Mini:
    """Stages of ResNeSt BottleneckBlocks as a ResNeSt that has only them (no stem): what _ResNeStTrainFn needs of a network."""

    @staticmethod
    def build(amd, stages, seed):
        rb = amd.resnest_backbone

        class Mini(rb.ResNeSt):
            def __init__(self):
                torch.nn.Module.__init__(self)
                self.stage_names, self._out_features = list(stages), list(stages)
                for name, blocks in stages.items():
                    self.add_module(name, torch.nn.Sequential(*[rb.BottleneckBlock(cin, cout, gw, stride, "FrozenBN") for cin, cout, gw, stride in blocks]))

            def _own_convs(self):
                return [m for name in self.stage_names for blk in getattr(self, name) for m in (blk.shortcut, blk.conv1, blk.conv2, blk.conv3)
                        if m is not None]
        torch.manual_seed(seed)
        net = R.randomise(Mini(), seed + 1)
        net._train_stages = tuple(stages)
        for p in [c.weight for c, _ in net._train_convs()] + net._train_fc():
            p.requires_grad_(True)
        return net


BLOCK_CASES = {
    # stages {name: [(cin, cout, group width, stride)]}, input (N, H, W); the first block of the first stage computes no dx
    "identity": ({"res3": [(16, 16, 8, 1)], "res4": [(16, 16, 8, 1)]}, (2, 9, 13)),
    "stride-2-avd-shortcut": ({"res3": [(16, 16, 8, 1)], "res4": [(16, 32, 8, 2)]}, (2, 9, 13)),
    "stride-2-avd-shortcut-even": ({"res3": [(16, 16, 8, 1)], "res4": [(16, 32, 8, 2)]}, (2, 8, 10)),
    "stride-1-shortcut": ({"res3": [(16, 16, 8, 1)], "res4": [(16, 32, 8, 1)]}, (2, 9, 13)),
    "winograd-grouped-conv": ({"res3": [(64, 64, 256, 1)]}, (1, 32, 32)),
}


@pytest.mark.parametrize("case", sorted(BLOCK_CASES))
def test_blocks_against_fp64_autograd(amd, case):
    stages, (N, H, W) = BLOCK_CASES[case]
    net = _Mini.build(amd, stages, 7)
    cin = next(iter(stages.values()))[0][0]
    x = torch.relu(_rand((N, cin, H, W), 8))                                  # a block's input is a ReLU's output
    last = list(stages.values())[-1][0]
    a1 = torch.empty(N, last[2], H, W)
    assert amd.resnest_backbone.conv2_wino(a1, last[2]) == (case == "winograd-grouped-conv")       # the module's own predicate

    def ref(dt):
        sd = {k: v.detach().to(dt) for k, v in net.state_dict().items()}
        keys = R.trainable_keys(sd, 0)
        for k in keys:
            sd[k].requires_grad_(True)
        y, feats = x.to(dt), {}
        for name, blocks in stages.items():
            for j, (_, _, _, stride) in enumerate(blocks):
                y = R.block(y, sd, f"{name}.{j}", stride)
            feats[name] = y
        cot = {k: _rand(v.shape, 9 + i).to(dt) for i, (k, v) in enumerate(feats.items())}
        sum((feats[k] * cot[k]).sum() for k in feats).backward()
        return {k: v.detach() for k, v in feats.items()}, {k: sd[k].grad for k in keys}, cot
    f64, g64, cot = ref(torch.float64)
    f32, g32, _ = ref(torch.float32)
    net = net.cuda()
    params = [c.weight for c, _ in net._train_convs()] + net._train_fc()
    outs = amd.resnest_backbone._ResNeStTrainFn.apply(net, _pm(x), *params)
    sum((o * cot[k].float().cuda()).sum() for k, o in zip(stages, outs)).backward()
    bad = []
    for k, o in zip(stages, outs):
        e = R.rel_l2(o, f64[k])
        print(f"[resnest-train] {case:28s} {k:28s} rel L2 gpu {e:.3e}  cpu fp32 {R.rel_l2(f32[k], f64[k]):.3e}  bar {FWD_BAR:.0e}")
        bad += [(k, e)] if not e <= FWD_BAR else []
    assert set(g64) == {k for k, p in net.named_parameters()}
    for k, p in net.named_parameters():
        e, c = R.rel_l2(p.grad, g64[k]), R.rel_l2(g32[k], g64[k])
        print(f"[resnest-train] {case:28s} {k:28s} rel L2 gpu {e:.3e}  cpu fp32 {c:.3e}  bar {4 * c:.3e}")
        assert g64[k].norm() > 0 and tuple(p.grad.shape) == tuple(g64[k].shape)
        bad += [(k, e, c)] if not e <= 4 * c else []
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 5. a small whole ResNeSt-50
def _run_net(amd, name, freeze_at):
    net, x = R.make_net(name)
    net = net.cuda().trainable_(freeze_at)
    out = net(x.cuda())
    cot = R.cotangents(name)
    sum((out[k] * cot[k].float().cuda()).sum() for k in out).backward()
    torch.cuda.synchronize()
    return net, out


@pytest.mark.parametrize("freeze_at", R.FREEZE_ATS)
def test_network_against_fp64_autograd(amd, freeze_at):
    name = "small"
    net, out = _run_net(amd, name, freeze_at)
    (f64, g64), (f32, g32) = R.reference(name, freeze_at, torch.float64), R.reference(name, freeze_at, torch.float32)
    assert list(out) == list(f64)
    bad, worst = [], 0.0
    for k in f64:
        e = R.rel_l2(out[k], f64[k])
        print(f"[resnest-train] {name} freeze_at {freeze_at} {k:28s} rel L2 gpu {e:.3e}  cpu fp32 {R.rel_l2(f32[k], f64[k]):.3e}  bar {FWD_BAR:.0e}")
        bad += [(k, e)] if not e <= FWD_BAR else []
    for k, p in net.named_parameters():
        if k not in g64:
            assert p.grad is None and not p.requires_grad, k                  # frozen parameters keep grad None
            continue
        assert p.grad is not None and tuple(p.grad.shape) == tuple(g64[k].shape), k
        e, c = R.rel_l2(p.grad, g64[k]), R.rel_l2(g32[k], g64[k])
        worst = max(worst, e / c)
        print(f"[resnest-train] {name} freeze_at {freeze_at} {k:28s} rel L2 gpu {e:.3e}  cpu fp32 {c:.3e}  bar {4 * c:.3e}")
        bad += [(k, e, c)] if not e <= 4 * c else []
    print(f"[resnest-train] {name} freeze_at {freeze_at}: worst gradient at {worst:.2f} x cpu fp32's deviation")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 6. determinism and workspaces
def test_determinism_and_poisoned_workspaces(amd, monkeypatch):
    cx = amd._lib.current_ctx()
    prev = cx.get_option("deterministic")
    cx.set_option("deterministic", 1)
    try:
        runs = []
        for poison in (False, False, True):
            if poison:
                monkeypatch.setattr(amd.ops, "_POISON", True)
            net, out = _run_net(amd, "small", 2)
            runs.append(({k: v.detach().clone() for k, v in out.items()}, {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}))
    finally:
        cx.set_option("deterministic", prev)
    (o1, g1) = runs[0]
    assert len(g1) == 13 * 7 + 3 and all(bool(torch.isfinite(v).all()) for v in g1.values())       # res3..res5: 13 blocks, 3 shortcuts
    for o, g in runs[1:]:
        assert all(torch.equal(o1[k], o[k]) for k in o1)
        assert all(torch.equal(g1[k], g[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g[k])]


# ------------------------------------------------------------------------------------------------ 7. the untouched frozen module
def test_keep_leaves_the_frozen_attention_bit_identical(amd):
    for C, avd in ((8, False), (256, True)):
        c = R.splat_case(2, C, max(C // 2, 32), 7, 10, avd)
        args = (_pm(c["s0"]), _pm(c["s1"]), c["w1"].cuda(), c["b1"].cuda(), c["w2"].cuda(), c["b2"].cuda())
        out, att = amd.ops.splat_attention(*args, avd=avd)
        out_k, att_k, g, h = amd.ops.splat_attention(*args, avd=avd, keep=True)
        assert torch.equal(out, out_k) and torch.equal(att, att_k)
        g64, h64, _ = R.splat_forward(c["s0"].double(), c["s1"].double(), c["w1"].double(), c["b1"].double(), c["w2"].double(), c["b2"].double())
        assert R.rel_l2(g, g64) <= 1e-5 and R.rel_l2(h, h64) <= 1e-5 and bool(((h.cpu() > 0) == (h64 > 0)).all())


def test_a_resnest_never_made_trainable_is_the_frozen_module(amd):
    net, x = R.make_net("small")
    net = net.cuda()
    with torch.no_grad():
        frozen_out = net(x.cuda())
    with pytest.raises(amd.AfiError, match=r"the ResNeSt bottom-up is forward-only \(frozen\): run it under torch.no_grad\(\) with no parameter or input "
                                           "requiring grad"):
        net(x.cuda().requires_grad_(True))
    net.res5[0].conv1.weight.requires_grad_(True)
    with pytest.raises(amd.AfiError, match="forward-only"):
        net(x.cuda())
    net.res5[0].conv1.weight.requires_grad_(False)
    train_out = net.trainable_(2)(x.cuda())                                    # the training forward runs the same kernels on the same fold
    assert all(torch.equal(frozen_out[k], train_out[k]) for k in frozen_out)
    with pytest.raises(amd.AfiError, match="the input requires grad"):
        net(x.cuda().requires_grad_(True))
    net.res2[0].conv1.weight.requires_grad_(True)
    with pytest.raises(amd.AfiError, match="belong to a frozen stage"):
        net(x.cuda())
    net.res2[0].conv1.weight.requires_grad_(False)
    with torch.no_grad():
        back = net.trainable_(False)(x.cuda())
    assert all(torch.equal(frozen_out[k], back[k]) for k in frozen_out) and not any(p.requires_grad for p in net.parameters())


# ------------------------------------------------------------------------------------------------ 8. integration
def test_fpn_afigan_over_the_trainable_bottom_up(amd):
    net, x = R.make_net("small")
    bottom_up = net.trainable_(2)
    fpn = amd.FPN_AFIGAN(bottom_up=bottom_up, in_features=["res2", "res3", "res4", "res5"], out_channels=32, norm="", top_block=amd.LastLevelMaxPool(),
                         fuse_type="sum").cuda()
    out = fpn(x.cuda())
    sum(p.sum() for p in out.values()).backward()
    torch.cuda.synchronize()
    for k, p in bottom_up.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0), k
        else:
            assert p.grad is None, k
    assert bottom_up.res3[0].conv2.fc1.bias.grad is not None and bottom_up.res5[2].conv3.weight.grad is not None


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and a.stride() == b.stride() and torch.equal(a, b)
    return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def test_detector_step_over_the_trainable_resnest(amd):
    """GeneralizedRCNN over FPN_AFIGAN over the small FrozenBN ResNeSt, a trainable RPN and CascadeROIHeads.trainable_(), two DetectorStep steps
    at 64 x 80.  After each step: the bottom-up's _prepare() is bit-equal to a fresh fold, no bias-free conv was refolded (frozen.fold_conv
    calls, counted by conv), and the frozen parameters are bit-unchanged."""
    import cascade_train_f64 as K
    from afigan_amd import frozen
    features = ["p2", "p3", "p4", "p5"]
    net, _ = R.make_net("small")
    backbone = amd.FPN_AFIGAN(bottom_up=net.trainable_(2), in_features=["res2", "res3", "res4", "res5"], out_channels=16, norm="",
                              top_block=amd.LastLevelMaxPool(), fuse_type="sum").cuda()
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[16], [32], [64], [128]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": features, "PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 50, "PRE_NMS_TOPK_TRAIN": 200,
                                       "POST_NMS_TOPK_TRAIN": 50, "BATCH_SIZE_PER_IMAGE": 32}})
    rpn = amd.RPN(cfg, {f: backbone.output_shape()[f] for f in features}).cuda().trainable_()
    heads = K.build_train_heads(amd, 16, "SyncBN", 3).cuda().trainable_()
    model = amd.GeneralizedRCNN(backbone=backbone, proposal_generator=rpn, roi_heads=heads, pixel_mean=[0.0, 0.0, 0.0], pixel_std=[1.0, 1.0, 1.0],
                                device="cuda").train()
    gts = [np.array([[4, 6, 40, 50], [30, 20, 76, 60], [10, 30, 30, 44]], np.float32), np.array([[8, 8, 60, 40], [40, 34, 70, 62]], np.float32)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g = torch.Generator().manual_seed(4)
    batch = []
    for b in gts:
        tg = type("GT", (), {})()
        tg.gt_boxes, tg.gt_classes = dev(b), dev(np.arange(len(b), dtype=np.int64) % 5)
        batch.append({"image": torch.randn((3, 64, 80), generator=g), "targets": tg})
    init = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    opt = amd.DetectorOptim(list(model.named_parameters()), modules=list(model.modules()), base_lr=1e-6, momentum=0.9, weight_decay=1e-3,
                            bias_lr_factor=2.0, weight_decay_bias=0.0, lr_steps=(2,), warmup_factor=0.5, warmup_iters=2)
    assert len(opt.modules) == 1 and opt.modules[0] is net
    bias_free = {id(c) for c in net.modules() if isinstance(c, frozen.Conv2d) and c.bias is None}
    assert len(net.fold_slots()) == len(net._train_convs()) == 13 * 3 + 3
    runner = amd.DetectorStep(model, opt)
    for step in range(2):
        losses = runner.run_step(batch)
        assert all(np.isfinite(v) for v in losses.values()), losses
        folded, real = [], frozen.fold_conv
        frozen.fold_conv = lambda conv, *a, **k: (folded.append(id(conv)), real(conv, *a, **k))[1]
        try:
            d = net._prepare()
        finally:
            frozen.fold_conv = real
        assert not bias_free & set(folded), f"step {step}: {len(bias_free & set(folded))} bias-free convs were refolded"
        assert len(folded) == 2 * 16, (step, len(folded))                       # fc1 and fc2 of all 16 blocks: their slot refolds itself
        for m in net._own_convs():
            fresh = m.fold()
            assert _same(d[id(m)], fresh), (step, type(m).__name__)
    now = {n: p.detach().cpu() for n, p in model.named_parameters()}
    frozen_names = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert frozen_names and all(torch.equal(now[n], init[n]) for n in frozen_names)
    moved = sum(int(not torch.equal(now[n], init[n])) for n in opt.names)
    assert moved >= 0.9 * len(opt.names), (moved, len(opt.names))
