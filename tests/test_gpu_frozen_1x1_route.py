"""The route of the frozen guides' 1x1 convs to afi_conv1x1_frozen_fwd (bf16x6 on weight images built once): GuideR50FPN (afigan_amd/guide.py,
what bench.py runs) and the forward-only ResNet-FPN guide (afigan_amd/resnet_guide.py).

Size.  In production a conv takes the route from ops.FROZEN1X1_MIN_PIXELS = 8192 pixels on; a conv of EVERY stage reaches that only from a
2 x 3 x 2048 x 2048 batch on (res5: 2 x 64 x 64 pixels), whose fp64 CPU restatement takes minutes.  The tests therefore run 2 x 3 x 128 x 192
images -- maps of 3072, 768, 192 and 48 pixels -- and lower the threshold to 32 pixels, so that the same plan, images and kernel serve every
1x1 conv of every stage (K chunks of 64 and 128, K up to 2048, stride-2 views, residual and top-down addends); thresholds of 200 and 8192
pixels (the latter with the production rule that convs with Cout >= 2 Cin move from 2048 pixels on) check that exactly the convs the host
plan names move and the others stay.

Bar: each pyramid level of the routed forward is within 4 x the un-routed forward's own rel. L2 error against the fp64 restatement (the
restatements of tests/test_gpu_guide.py and tests/test_gpu_resnet_guide.py)."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

KIND = 23
SHAPE = (2, 3, 128, 192)
HERE = os.path.dirname(os.path.abspath(__file__))


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


@pytest.fixture()
def route(amd, monkeypatch):
    """set(threshold, on): the routing threshold and switch of afigan_amd.ops for this test"""
    def set_(threshold=32, on=True):
        monkeypatch.setattr(amd.ops, "FROZEN1X1_MIN_PIXELS", threshold)
        monkeypatch.setattr(amd.ops, "frozen1x1_route", on)
    return set_


def _kind23_launches(fn):
    from afigan_amd import _lib
    lib = _lib.load()
    _lib.check(lib.afi_profile_enable(1), "afi_profile_enable")
    try:
        out = fn()
        torch.cuda.synchronize()
        buf = (C.c_double * 3)()
        _lib.check(lib.afi_profile_get(KIND, buf), "afi_profile_get")
    finally:
        lib.afi_profile_enable(0)
    return out, int(buf[0])


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _planned(ops, calls, threshold):
    """how many of the recorded 1x1 convs (x view, Cout, add) the host plan sends to the new kernel at `threshold`"""
    n = 0
    for x, cout, add in calls:
        N, Cin, H, W = x.shape
        plan = ops.conv1x1_frozen_plan(N, H, W, Cin, cout, (x.stride(0), x.stride(2), x.stride(3)),
                                       add_strides=(add.stride(0), add.stride(2), add.stride(3)) if add is not None else None)
        least = min(threshold, 2048) if cout >= 2 * Cin else threshold          # ops.FROZEN1X1_MIN_PIXELS_EXPANDING: convs with Cout >= 2 Cin
        n += int(N * H * W >= least and plan is not None)
    return n


# ------------------------------------------------------------------------------------------------ GuideR50FPN
@pytest.fixture(scope="module")
def harness(amd):
    """(model, image batch, fp64 pyramid, the 1x1 convs one forward runs as (x view, Cout, add))"""
    from afigan_amd.guide import GuideR50FPN, _Conv1x1
    torch.manual_seed(0)
    g = GuideR50FPN().cuda()
    img = torch.rand(SHAPE, generator=torch.Generator().manual_seed(1)) * 255.0
    ref = _sibling("test_gpu_guide")._ref_forward(g, img)
    calls = []

    def hook(m, args, kwargs):
        x = args[0] if m.stride == 1 else args[0][:, :, ::m.stride, ::m.stride]
        calls.append((x, m.w.shape[0], kwargs.get("add", args[1] if len(args) > 1 else None)))

    hs = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in g.modules() if isinstance(m, _Conv1x1)]
    amd.ops.frozen1x1_route, keep = False, amd.ops.frozen1x1_route
    try:
        g(img.cuda())
    finally:
        amd.ops.frozen1x1_route = keep
        for h in hs:
            h.remove()
    assert len(calls) == 16 * 2 + 4 + 4                                 # conv1 + conv3 per block, four shortcuts, four laterals
    return g, img.cuda(), ref, calls


def test_harness_guide_pyramid_and_kinds(amd, harness, route):
    g, img, ref, calls = harness
    ops = amd.ops
    route(on=False)
    off, n_off = _kind23_launches(lambda: g(img))
    assert n_off == 0
    route(32)
    assert _planned(ops, calls, 32) == len(calls)                      # every stage, every 1x1 conv
    on, n_on = _kind23_launches(lambda: g(img))
    assert n_on == len(calls), (n_on, len(calls))
    for i, r in enumerate(ref):
        k = f"p{i + 2}"
        e_on, e_off = _rel_l2(on[k], r), _rel_l2(off[k], r)
        print(f"[route] GuideR50FPN {k}: rel-L2 vs fp64 routed {e_on:.2e}, un-routed {e_off:.2e} (bar {4 * e_off:.2e}); routed vs un-routed {_rel_l2(on[k], off[k]):.2e}")
        assert e_on <= 4 * e_off, (k, e_on, e_off)
    for thr in (200, 8192):                                            # only the maps at or above the threshold move
        route(thr)
        want = _planned(ops, calls, thr)
        _, n = _kind23_launches(lambda: g(img))
        assert n == want and 0 < want < len(calls), (thr, n, want)         # (at 8192: the Cout >= 2 Cin convs of the 3072-pixel map)


def test_images_are_built_once_and_follow_their_weight(amd, harness, route):
    g, img, _, calls = harness
    ops = amd.ops
    route(32)
    first = g(img)
    built = ops.frozen1x1_images_built
    again = g(img)
    assert ops.frozen1x1_images_built == built, "a second forward of unchanged weights built an image"
    assert all(torch.equal(first[k], again[k]) for k in first)
    conv = g.stages[1][0].c3
    with torch.no_grad():
        conv.w.mul_(2.0)
    try:
        changed = g(img)
        assert ops.frozen1x1_images_built == built + 1, "one changed weight must rebuild exactly its own image"
        route(on=False)
        want = g(img)
        for k in changed:
            assert not torch.equal(changed[k], first[k]), k
            assert _rel_l2(changed[k], want[k]) <= 1e-5, (k, _rel_l2(changed[k], want[k]))
    finally:
        with torch.no_grad():
            conv.w.mul_(0.5)


# ------------------------------------------------------------------------------------------------ resnet_guide, forward only
def _resnet_calls(bb, x):
    """the 1x1 convs of one forward-only R-50-FPN forward on the padded batch x, as (x view, Cout, add) over empty tensors of the right strides"""
    N, _, H, W = x.shape
    calls, bu = [], bb.bottom_up
    H, W, cin = (H + 3) // 4, (W + 3) // 4, 64
    pm = lambda c, h, w: torch.empty((N, h, w, c), device="meta").permute(0, 3, 1, 2)
    feats = []
    for name in bu.stage_names:
        for blk in getattr(bu, name):
            s1 = blk.conv1.stride
            xin = pm(cin, H, W)
            mid, cout = blk.conv1.weight.shape[0], blk.conv3.weight.shape[0]
            if blk.shortcut is not None:
                ss = blk.shortcut.stride
                calls.append((xin[:, :, ::ss, ::ss], cout, None))
            calls.append((xin[:, :, ::s1, ::s1], mid, None))
            st = s1 * blk.conv2.stride
            H, W = (H + st - 1) // st, (W + st - 1) // st
            calls.append((pm(mid, H, W), cout, pm(cout, H, W)))
            cin = cout
        feats.append((cin, H, W))
    for i, (c, h, w) in enumerate(feats[::-1]):
        calls.append((pm(c, h, w), 256, None if i == 0 else pm(256, h, w)))
    return calls


@pytest.fixture(scope="module")
def resnet(amd):
    t = _sibling("test_gpu_resnet_guide")
    guide, _ = t._guide(amd, 50, True, "sum", seed=3)
    g = torch.Generator().manual_seed(7)
    images = [torch.rand(SHAPE[1:], generator=g) * 255.0 for _ in range(SHAPE[0])]
    x = t._batch(guide, images)
    with torch.no_grad():
        ref = t._ref_backbone(guide.backbone, x)
    return guide.backbone, x.float().cuda(), ref


def test_resnet_guide_pyramid_and_kinds(amd, resnet, route):
    bb, x, ref = resnet
    ops = amd.ops
    calls = _resnet_calls(bb, x)
    assert len(calls) == 16 * 2 + 4 + 4
    with torch.no_grad():
        route(on=False)
        off, n_off = _kind23_launches(lambda: bb(x))
        assert n_off == 0
        route(32)
        assert _planned(ops, calls, 32) == len(calls)
        on, n_on = _kind23_launches(lambda: bb(x))
        assert n_on == len(calls), (n_on, len(calls))
        for k in ref:
            e_on, e_off = _rel_l2(on[k], ref[k]), _rel_l2(off[k], ref[k])
            print(f"[route] resnet_guide {k}: rel-L2 vs fp64 routed {e_on:.2e}, un-routed {e_off:.2e} (bar {4 * e_off:.2e}); routed vs un-routed {_rel_l2(on[k], off[k]):.2e}")
            assert e_on <= 4 * e_off, (k, e_on, e_off)
        for thr in (200, 8192):
            route(thr)
            want = _planned(ops, calls, thr)
            _, n = _kind23_launches(lambda: bb(x))
            assert n == want and 0 < want < len(calls), (thr, n, want)


def test_resnet_guide_rebuilds_one_image_and_replays_from_a_graph(amd, resnet, route):
    bb, x, _ = resnet
    ops = amd.ops
    route(32)
    with torch.no_grad():
        first = bb(x)
        built = ops.frozen1x1_images_built
        bb(x)
        assert ops.frozen1x1_images_built == built
        conv = bb.bottom_up.res3[1].conv1
        conv.weight.mul_(2.0)
        try:
            changed = bb(x)
            assert ops.frozen1x1_images_built == built + 1
            route(on=False)
            want = bb(x)
            for k in changed:
                assert not torch.equal(changed[k], first[k])
                assert _rel_l2(changed[k], want[k]) <= 1e-5, (k, _rel_l2(changed[k], want[k]))
        finally:
            conv.weight.mul_(0.5)
        # every image exists after an eager forward (and _prepare()): a captured forward launches no builder and replays bit-identically
        route(32)
        x = x.clone()
        bb._prepare()
        eager = bb(x)
        built = ops.frozen1x1_images_built
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = bb(x)
        assert ops.frozen1x1_images_built == built
        x.mul_(0.5).add_(0.25)                                          # new input values in the same buffer
        graph.replay()
        torch.cuda.synchronize()
        eager2 = bb(x)
        for k in eager:
            assert torch.equal(captured[k], eager2[k]), k
            assert not torch.equal(captured[k], eager[k]), k
