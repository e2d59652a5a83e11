"""GPU parity of the drop-in modules (one HIP forward / backward each) against the golden fixtures captured from the
reference modules (tests/golden/make_golden.py) and against the CPU oracle.  Bar: 1e-3 relative fp32."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import afigan_oracle as orc  # noqa: E402

# Discriminator gradients on the library's OWN forward: a LeakyReLU-mask element that flips under fp32 rounding moves a gradient tensor
# by ~1e-3 relative L2 / ~1e-2 max-norm (torch's own fp32 CPU evaluation of the reference does the same against fp64), so these get
# their own bars; tests/test_gpu_d_parity.py holds the full backward to 1e-4 max-norm with the reference's masks and bounds the flips.
D_GRAD_L2_TOL = 3e-3
D_GRAD_MAXNORM_TOL = 3e-2


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


def _load(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name)))


def _rel(got, ref):
    got, ref = torch.as_tensor(got).detach().float().cpu(), torch.as_tensor(ref).detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def _digest(t, nsample=64):
    f = t.detach().reshape(-1).double().cpu()
    stride = max(1, f.numel() // nsample)
    return np.array([f.sum().item(), f.norm().item(), f.abs().max().item()]), f[::stride][:nsample].float().numpy()


def _logical(p_grad):
    """grad tensor in logical (NCHW / OIHW) element order regardless of its memory layout."""
    return p_grad.detach().contiguous()


def _check_digest(fx, key, g, prefix="", tol=1e-3):
    d, s = _digest(_logical(g))
    rd, rs = fx[prefix + "gd/" + key], fx[prefix + "gs/" + key]
    assert abs(d[1] - rd[1]) <= tol * rd[1] + 1e-12, (key, d, rd)
    np.testing.assert_allclose(s, rs, rtol=0, atol=tol * rd[2] + 1e-12, err_msg=key)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_generator_small_vs_reference(amd, golden_dir, tag):
    fx = _load(golden_dir, f"g_small_{tag}.npz")
    G = amd.Generator(in_channels=16, n_residual_dense_blocks=3, growth_rate=4).cuda()
    sd = {k[2:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("w/")}
    assert set(sd) == set(G.state_dict()), set(sd) ^ set(G.state_dict())
    G.load_state_dict(sd, strict=True)
    x = torch.from_numpy(fx["x"]).cuda().requires_grad_(True)           # NCHW-contiguous input, like detectron2 hands over
    out = G(x)
    assert tuple(out.shape) == fx["out"].shape
    assert _rel(out, fx["out"]) < 1e-3
    (out * torch.from_numpy(fx["R"]).cuda()).sum().backward()
    assert _rel(x.grad, fx["dx"]) < 1e-3
    for k, p in G.named_parameters():
        assert _rel(_logical(p.grad), fx["g/" + k]) < 1e-3, k


def test_generator_full_cfg1_vs_reference_and_oracle(amd, golden_dir):
    fx = _load(golden_dir, "g_full_cfg1.npz")
    gp = orc.closed_form_generator_params()
    G = amd.Generator(n_residual_dense_blocks=3).cuda()
    G.load_state_dict(gp, strict=True)
    x_cpu = torch.randn(tuple(fx["x_shape"]), generator=torch.Generator().manual_seed(int(fx["x_seed"][0])))
    x = x_cpu.cuda().requires_grad_(True)
    out = G(x)
    assert tuple(out.shape) == (1, 256, 50, 68)
    scale = float(fx["out_absmax"][0])
    o = out.detach().cpu()
    assert np.abs(o[0, ::16, ::5, ::7].numpy() - fx["out_slice"]).max() < 1e-3 * scale
    assert np.abs(o[0, :, 17, :].numpy() - fx["out_row"]).max() < 1e-3 * scale
    out.sum().backward()
    assert np.abs(x.grad.cpu()[0, ::16, ::5, ::7].numpy() - fx["dx_slice"]).max() < 1e-3 * fx["gd/x"][2]
    for k, p in G.named_parameters():
        _check_digest(fx, k, p.grad)
    # full-tensor comparison against the CPU oracle on the same input
    pr = {k: v.clone().requires_grad_(True) for k, v in gp.items()}
    xr = x_cpu.clone().requires_grad_(True)
    ref = orc.generator_forward(xr, pr)
    ref.sum().backward()
    assert _rel(out, ref) < 1e-3
    assert _rel(x.grad, xr.grad) < 1e-3
    for k, p in G.named_parameters():
        assert _rel(_logical(p.grad), pr[k].grad) < 1e-3, k
    # inference path (no grad) and channels_last input give the same values
    with torch.no_grad():
        out2 = G(x.detach().contiguous(memory_format=torch.channels_last))
    assert torch.equal(out2, out.detach())


@pytest.mark.parametrize("tag", ["a", "b"])
def test_discriminator_vs_reference(amd, golden_dir, tag):
    fx = _load(golden_dir, f"d_{tag}.npz")
    D = amd.Discriminator().cuda()
    dp = orc.closed_form_discriminator_params()
    assert set(dp) == set(D.state_dict())
    D.load_state_dict(dp, strict=True)
    D.train()
    x = torch.randn(tuple(fx["x_shape"]), generator=torch.Generator().manual_seed(int(fx["x_seed"][0]))).cuda().requires_grad_(True)
    logits = D.Discriminators[0](x)                  # called the way stage1_trainer.py:349 calls it
    assert _rel(logits, fx["logits"]) < 1e-3
    sd = D.state_dict()
    for k in sd:
        if "running" in k:
            assert _rel(sd[k], fx["buf/" + k]) < 1e-3, k
        if "num_batches" in k:
            assert int(sd[k]) == int(fx["buf/" + k]) == 1
    (logits * torch.from_numpy(fx["R"]).cuda()).sum().backward()
    # Gradients through LeakyReLU are DISCONTINUOUS in the pre-activation sign: an element whose BN output lies within
    # fp32 rounding (~1e-6) of zero gets slope 1 in one fp32 evaluation and 0.2 in another.  With 546 pixels one such flip
    # moves a whole gradient tensor by ~1e-3 in relative L2 (measured: torch-CPU fp32 vs the fp64 oracle differ by 7e-4 L2 /
    # 1.4e-2 max-norm on this very fixture).  So D gradients are held to 3e-3 relative L2 (plus a loose max-norm bound);
    # the mask-free pieces (BN backward, dgrad, wgrad with explicit masks) are held to 1e-3 max-norm in test_gpu_ops.py.
    ref_dx = fx["dx_slice"]
    got_dx = x.grad.cpu()[0, ::16].numpy()
    assert np.linalg.norm(got_dx - ref_dx) <= D_GRAD_L2_TOL * np.linalg.norm(ref_dx)
    assert np.abs(got_dx - ref_dx).max() < D_GRAD_MAXNORM_TOL * fx["gd/x"][2]
    for k, p in D.named_parameters():
        if k.endswith(".0.bias") and not k.startswith("Discriminators.0.3"):
            # bias feeding a train-mode BN: zero gradient up to rounding noise, in the reference too
            wn = fx["gd/" + k.replace(".bias", ".weight")][1]
            assert p.grad.abs().max().item() < 1e-3 * wn, k
            continue
        d, s = _digest(_logical(p.grad))
        rd, rs = fx["gd/" + k], fx["gs/" + k]
        assert abs(d[1] - rd[1]) <= D_GRAD_L2_TOL * rd[1], (k, d, rd)
        np.testing.assert_allclose(s, rs, rtol=0, atol=D_GRAD_MAXNORM_TOL * rd[2], err_msg=k)
    # full tensors against the fp32 CPU oracle, relative L2
    pr = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone()) for k, v in dp.items()}
    xr = x.detach().cpu().clone().requires_grad_(True)
    lref, _ = orc.discriminator_forward(xr, pr, training=True)
    (lref * torch.from_numpy(fx["R"])).sum().backward()

    def l2(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return ((a - b).norm() / b.norm()).item()
    assert l2(x.grad, xr.grad) < D_GRAD_L2_TOL
    for k, p in D.named_parameters():
        if k.endswith(".0.bias") and not k.startswith("Discriminators.0.3"):
            continue
        assert l2(_logical(p.grad), pr[k].grad) < D_GRAD_L2_TOL, k


def test_discriminator_eval_mode_and_buffers(amd):
    D = amd.Discriminator(in_filters=16).cuda()
    dp = orc.closed_form_discriminator_params(16)
    D.load_state_dict(dp, strict=True)
    x = torch.randn((2, 16, 9, 11), generator=torch.Generator().manual_seed(5))
    D.eval()
    with torch.no_grad():
        got = D(x.cuda())
    ref, _ = orc.discriminator_forward(x, dp, training=False)
    assert _rel(got, ref) < 1e-3
    assert int(D.state_dict()["Discriminators.0.0.0.norm.num_batches_tracked"]) == 0
    D.train()
    p = {k: v.clone() for k, v in dp.items()}
    for _ in range(3):                                # running stats advance once per call
        with torch.no_grad():
            got = D(x.cuda())
        ref, upd = orc.discriminator_forward(x, p, training=True)
        p.update(upd)
    assert _rel(got, ref) < 1e-3
    sd = D.state_dict()
    for k, v in p.items():
        if "running" in k:
            assert _rel(sd[k], v) < 1e-3, k
        if "num_batches" in k:
            assert int(sd[k]) == 3


def test_discriminator_large_map_halo_path(amd):
    """A map large enough for the halo-staged conv kernels (18,432 pixels), small channel counts to keep the oracle cheap."""
    Cin = 64
    dp = orc.closed_form_discriminator_params(Cin)
    D = amd.Discriminator(in_filters=Cin).cuda()
    D.load_state_dict(dp)
    D.train()
    x = torch.randn((1, Cin, 72, 256), generator=torch.Generator().manual_seed(9))
    xg = x.cuda().requires_grad_(True)
    logits = D(xg)
    (logits * logits).mean().backward()
    pr = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone()) for k, v in dp.items()}
    xr = x.clone().requires_grad_(True)
    lref, _ = orc.discriminator_forward(xr, pr, training=True)
    (lref * lref).mean().backward()
    assert _rel(logits, lref) < 1e-3

    def l2(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return ((a - b).norm() / b.norm()).item()
    assert l2(xg.grad, xr.grad) < D_GRAD_L2_TOL
    for k, p in D.named_parameters():
        if k.endswith(".0.bias") and not k.startswith("Discriminators.0.3"):
            continue
        assert l2(_logical(p.grad), pr[k].grad) < D_GRAD_L2_TOL, k


def test_mid_size_maps_split_k_paths_full_channels(amd):
    """Real channel counts on a mid-size ragged map (1x256x50x84 for D, 1x256x26x42 -> 52x84 for G): the 128x128 tiles with
    the mid-size split-K rule (linear and halo variants, dgrad included) and the balanced wgrad split, against the oracle."""
    dp = orc.closed_form_discriminator_params()
    D = amd.Discriminator().cuda()
    D.load_state_dict(dp)
    D.train()
    x = torch.randn((1, 256, 50, 84), generator=torch.Generator().manual_seed(12))
    xg = x.cuda().requires_grad_(True)
    logits = D(xg)
    (logits * logits).mean().backward()
    pr = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone()) for k, v in dp.items()}
    xr = x.clone().requires_grad_(True)
    lref, _ = orc.discriminator_forward(xr, pr, training=True)
    (lref * lref).mean().backward()
    assert _rel(logits, lref) < 1e-3

    def l2(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return ((a - b).norm() / b.norm()).item()
    assert l2(xg.grad, xr.grad) < D_GRAD_L2_TOL
    for k, p in D.named_parameters():
        if k.endswith(".0.bias") and not k.startswith("Discriminators.0.3"):
            continue
        assert l2(_logical(p.grad), pr[k].grad) < D_GRAD_L2_TOL, k

    gp = orc.closed_form_generator_params()
    G = amd.Generator(n_residual_dense_blocks=3).cuda()
    G.load_state_dict(gp)
    z = torch.randn((1, 256, 26, 42), generator=torch.Generator().manual_seed(13))
    zg = z.cuda().requires_grad_(True)
    out = G(zg)
    out.sum().backward()
    qr = {k: v.clone().requires_grad_(True) for k, v in gp.items()}
    zr = z.clone().requires_grad_(True)
    ref = orc.generator_forward(zr, qr)
    ref.sum().backward()
    assert _rel(out, ref) < 1e-3 and _rel(zg.grad, zr.grad) < 1e-3
    for k, p in G.named_parameters():
        assert _rel(_logical(p.grad), qr[k].grad) < 1e-3, k


def test_generator_large_map_halo_path(amd):
    C, g = 128, 32
    gp = orc.closed_form_generator_params(C, 2, g)
    G = amd.Generator(in_channels=C, n_residual_dense_blocks=2, growth_rate=g).cuda()
    G.load_state_dict(gp)
    x = torch.randn((1, C, 72, 256), generator=torch.Generator().manual_seed(4))
    xg = x.cuda().requires_grad_(True)
    out = G(xg)
    out.sum().backward()
    pr = {k: v.clone().requires_grad_(True) for k, v in gp.items()}
    xr = x.clone().requires_grad_(True)
    ref = orc.generator_forward(xr, pr, n_rdb=2)
    ref.sum().backward()
    assert _rel(out, ref) < 1e-3 and _rel(xg.grad, xr.grad) < 1e-3
    for k, p in G.named_parameters():
        assert _rel(_logical(p.grad), pr[k].grad) < 1e-3, k


def test_frozen_generator_inside_a_graph(amd):
    """MODEL.AFI_FREEZE (fpn_sr.py:67-69): every G parameter has requires_grad=False but the input still needs its gradient
    (stage 3: prev_features come from the trainable FPN).  Also a partially frozen generator."""
    C, g = 16, 4
    gp = orc.closed_form_generator_params(C, 3, g)
    G = amd.Generator(in_channels=C, n_residual_dense_blocks=3, growth_rate=g).cuda()
    G.load_state_dict(gp)
    for p in G.parameters():
        p.requires_grad = False
    x = torch.randn((2, C, 6, 9), generator=torch.Generator().manual_seed(2))
    xg = x.cuda().requires_grad_(True)
    (G(xg * 1.5) ** 2).sum().backward()
    xr = x.clone().requires_grad_(True)
    (orc.generator_forward(xr * 1.5, gp) ** 2).sum().backward()
    assert _rel(xg.grad, xr.grad) < 1e-3
    assert all(p.grad is None for p in G.parameters())
    # un-freeze only the last conv
    w9 = G.Generators[0][4][0].weight
    w9.requires_grad = True
    xg.grad = None
    (G(xg) ** 2).sum().backward()
    pr = {k: v.clone().requires_grad_(k == "Generators.0.4.0.weight") for k, v in gp.items()}
    xr2 = x.clone().requires_grad_(True)
    (orc.generator_forward(xr2, pr) ** 2).sum().backward()
    assert _rel(_logical(w9.grad), pr["Generators.0.4.0.weight"].grad) < 1e-3
    assert _rel(xg.grad, xr2.grad) < 1e-3
    assert sum(p.grad is not None for p in G.parameters()) == 1


def test_generator_empty_batch(amd):
    """N = 0 (a rank whose shard has no image / an empty proposal-level map): an empty output of the right shape, no launch,
    zero gradients for every parameter (what the reference's conv stack returns for empty inputs)."""
    G = amd.Generator(in_channels=16, n_residual_dense_blocks=2, growth_rate=4).cuda()
    x = torch.zeros((0, 16, 5, 7), device="cuda", requires_grad=True)
    out = G(x)
    assert tuple(out.shape) == (0, 16, 10, 14)
    out.sum().backward()
    assert x.grad is not None and tuple(x.grad.shape) == (0, 16, 5, 7)
    for k, p in G.named_parameters():
        assert p.grad is not None and float(p.grad.abs().sum()) == 0.0, k
    with torch.no_grad():
        assert tuple(G(torch.zeros((2, 16, 0, 7), device="cuda")).shape) == (2, 16, 0, 14)


def test_error_paths(amd):
    G = amd.Generator(in_channels=16, growth_rate=4).cuda()
    with pytest.raises(amd.AfiError):
        G(torch.zeros(1, 8, 4, 4, device="cuda"))                 # wrong channel count
    with pytest.raises(amd.AfiError):
        G(torch.zeros(1, 16, 4, 4, device="cuda", dtype=torch.float16))
    D = amd.Discriminator(in_filters=16).cuda().eval()
    x = torch.randn(1, 16, 5, 5, device="cuda", requires_grad=True)
    with pytest.raises(amd.AfiError, match="train-mode"):
        D(x).sum().backward()                                     # eval-mode backward is not part of the path
    # degenerate spatial sizes still work (1x1 map -> 2x2)
    out = G(torch.randn(1, 16, 1, 1, device="cuda"))
    assert tuple(out.shape) == (1, 16, 2, 2) and torch.isfinite(out).all()


def test_weight_cache_with_weights_that_need_a_layout_copy(amd):
    """the transform cache is keyed by weight ADDRESS.  With parameters that are NOT stored in the kernels' [O][kh][kw][I]
    layout every call makes temporary copies; under no_grad they used to be freed after the call, and the allocator hands the same
    address to the next same-shaped weight (w0 / w7 / w9 are all [256,256,3,3]) -- a cache hit on another layer's transform.  Inside a
    weight_transform_cache block the temporaries are now kept alive until the block exits."""
    ops = amd.ops
    torch.manual_seed(3)
    G = amd.Generator(n_residual_dense_blocks=3).cuda().eval()
    x = torch.randn((1, 256, 32, 32), generator=torch.Generator().manual_seed(4)).cuda()     # 1024 px: the Winograd path with its cache
    with torch.no_grad():
        ref = G(x).clone()
        G2 = amd.Generator(n_residual_dense_blocks=3).cuda().eval()
        G2.load_state_dict(G.state_dict())
        for p in G2.parameters():
            if p.dim() == 4:
                p.data = p.data.contiguous()                     # NCHW-contiguous storage: ohwi() has to copy on every call
        assert not G2.Generators[0][0][0].weight.permute(0, 2, 3, 1).is_contiguous()
        with ops.weight_transform_cache(x.device):
            outs = [G2(x).clone() for _ in range(3)]             # FPN / PAFPN run the interpolator 3x inside one block
    for o in outs:
        assert _rel(o, ref) < 1e-6


def test_two_contexts_keep_their_own_state(amd):
    """Two engines in one process: each afi_ctx_t has its own weight-transform cache.  Changing a weight's VALUES in place makes the
    cache of the context that transformed it stale (the documented contract: the caller invalidates) and leaves the other one fresh."""
    import ctypes as C
    ops, _lib = amd.ops, amd._lib
    x = torch.randn((1, 128, 32, 32), generator=torch.Generator().manual_seed(1)).cuda().contiguous(memory_format=torch.channels_last)
    w = ops.new_ohwi(128, 128, 3, 3, "cuda", zero=False)
    w.normal_(0, 0.05)
    a, b = _lib.Ctx(), _lib.Ctx()
    bufs = [torch.empty(8 * 1024 * 1024, device="cuda") for _ in range(2)]
    for cx, buf in zip((a, b), bufs):
        _lib.call("afi_ctx_set_wino_weight_cache", cx.handle, C.c_void_p(buf.data_ptr()), buf.numel())
    with _lib.use_ctx(a):
        y_a0 = ops.conv3x3_wino_fwd(x, w, None).clone()          # context a transforms and caches w
    w.mul_(2.0)                                                  # values change, address does not
    with _lib.use_ctx(a):
        y_a1 = ops.conv3x3_wino_fwd(x, w, None).clone()          # stale by contract (no invalidate)
    with _lib.use_ctx(b):
        y_b = ops.conv3x3_wino_fwd(x, w, None).clone()           # context b never saw the old values
    assert torch.equal(y_a1, y_a0)
    assert _rel(y_b, 2.0 * y_a0) < 1e-5
    _lib.call("afi_ctx_wino_weight_cache_invalidate", a.handle)
    with _lib.use_ctx(a):
        assert _rel(ops.conv3x3_wino_fwd(x, w, None), y_b) < 1e-6
    for cx in (a, b):
        _lib.call("afi_ctx_set_wino_weight_cache", cx.handle, C.c_void_p(None), 0)


def test_results_do_not_depend_on_uninitialised_memory(amd, monkeypatch):
    """Every workspace and output buffer the Python side hands to the library pre-filled with NaN (ops._POISON, = AFI_POISON_WS=1):
    generator and discriminator forward + backward and one stage-1 step give the same finite results as with recycled memory."""
    import copy
    from afigan_amd import ops
    torch.manual_seed(5)
    G0 = amd.Generator(in_channels=32, n_residual_dense_blocks=3).cuda()
    D0 = amd.Discriminator(in_filters=32).cuda()
    g = torch.Generator().manual_seed(6)
    x = torch.randn((2, 32, 9, 13), generator=g).cuda()
    h = torch.randn((2, 32, 18, 26), generator=g).cuda()
    R = torch.randn((2, 32, 18, 26), generator=g).cuda()

    def run():
        G, D = copy.deepcopy(G0), copy.deepcopy(D0)
        xg = x.clone().requires_grad_(True)
        out = G(xg)
        (out * R).sum().backward()
        hg = h.clone().requires_grad_(True)
        logits = D(hg)
        logits.square().mean().backward()
        res = [out.detach(), xg.grad, logits.detach(), hg.grad] + [q.grad for q in list(G.parameters()) + list(D.parameters())]
        step = amd.Stage1Step(copy.deepcopy(G0), copy.deepcopy(D0), base_lr=0.01, warmup_iters=0)
        step.run_step([x], [h])
        res += [torch.tensor(sorted(step.metrics().values()))]
        return [t.detach().float().cpu().clone() for t in res]

    clean = run()
    monkeypatch.setattr(ops, "_POISON", True)
    poisoned = run()
    for a, b in zip(clean, poisoned):
        assert torch.isfinite(b).all()
        assert ((a - b).abs().max() / (a.abs().max() + 1e-30)).item() < 1e-4      # (fp32 atomics of the split weight gradients only)


@pytest.mark.parametrize("C,g,hw", [(128, 32, (72, 64)), (32, 8, (80, 64)), (64, 32, (60, 56))])
def test_generator_batched_growth_gradients_match_the_per_conv_form(amd, C, g, hw):
    """AFI_OPT_G_BATCH_GROWTH_GRADS (larger maps: what a dense block's four growth convs take from the block input as one packed conv, their data
    gradients onto it as one packed data gradient, their weight gradients as one packed GEMM; Winograd form at 128 channels) against the
    per-conv form of generator_rdb.py:64-71, and both against the oracle: outputs, input gradient, every parameter gradient."""
    from afigan_amd import _lib
    gp = orc.closed_form_generator_params(C, 2, g)
    x = torch.randn((1, C, *hw), generator=torch.Generator().manual_seed(21))
    res = {}
    for flag in (1, 0):
        cx = _lib.Ctx()
        cx.set_option("g_batch_growth_grads", flag)
        G = amd.Generator(in_channels=C, n_residual_dense_blocks=2, growth_rate=g).cuda()
        G.load_state_dict(gp)
        xg = x.cuda().requires_grad_(True)
        with _lib.use_ctx(cx):
            out = G(xg)
            (out * torch.linspace(-1, 1, out.numel(), device="cuda").view_as(out)).sum().backward()
        res[flag] = (xg.grad.clone(), {k: _logical(p.grad).clone() for k, p in G.named_parameters()}, out.detach().clone())
    pr = {k: v.clone().requires_grad_(True) for k, v in gp.items()}
    xr = x.clone().requires_grad_(True)
    ref = orc.generator_forward(xr, pr, n_rdb=2)
    (ref * torch.linspace(-1, 1, ref.numel()).view_as(ref)).sum().backward()
    for flag in (1, 0):
        assert _rel(res[flag][2], ref) < 1e-3, flag
        assert _rel(res[flag][0], xr.grad) < 1e-3, flag
        for k in pr:
            assert _rel(res[flag][1][k], pr[k].grad) < 1e-3, (flag, k)
    assert _rel(res[1][2], res[0][2]) < 2e-5 and _rel(res[1][0], res[0][0]) < 2e-5
    for k in pr:
        assert _rel(res[1][1][k], res[0][1][k]) < 2e-5, k


@pytest.fixture(scope="module")
def schedule_case():
    """One small interpolator for test_generator_every_schedule_matches_the_oracle and its CPU-oracle results, computed once: C = 128, growth 32, two
    dense blocks on 1 x 128 x 36 x 32 -- 1152 low-res pixels, the smallest map above the 1024-pixel floor of the Winograd scratch sizing with C and
    G still multiples of 32 (the weight images' rule)."""
    C, g = 128, 32
    gp = orc.closed_form_generator_params(C, 2, g)
    x = torch.randn((1, C, 36, 32), generator=torch.Generator().manual_seed(22))
    pr = {k: v.clone().requires_grad_(True) for k, v in gp.items()}
    xr = x.clone().requires_grad_(True)
    ref = orc.generator_forward(xr, pr, n_rdb=2)
    (ref * torch.linspace(-1, 1, ref.numel()).view_as(ref)).sum().backward()
    return gp, x, ref.detach(), xr.grad, {k: v.grad for k, v in pr.items()}


_LARGE_MAP_FORMS = dict(g_smallmap6_max_pixels=0, g_smallmap_max_pixels=0, g_grouped_wgrad_max_pixels=0, g_winograd_min_pixels=1024)


@pytest.mark.parametrize("dtype,options", [
    (None, {}),                                                                 # (a) defaults: batched forward on weight images, grouped backward
    (None, _LARGE_MAP_FORMS),                                                   # (b) batched-growth forms with Winograd, side stream on
    (None, dict(_LARGE_MAP_FORMS, g_batch_growth_grads=0)),                     # (c) conv by conv
    (None, dict(_LARGE_MAP_FORMS, g_batch_growth_grads=0, winograd=0)),         # (d) direct kernels only
    (None, dict(deterministic=1)),                                              # (e) forward on images, backward per layer
    ("fp32", {}),                                                               # (f) the small-map schedule without images
], ids=["defaults", "batched_growth_winograd", "conv_by_conv", "direct_only", "deterministic", "fp32_small_map"])
def test_generator_every_schedule_matches_the_oracle(amd, schedule_case, dtype, options):
    """Every schedule gen_plan() (csrc/nets.hip; table in DESIGN.md 4) can choose for one interpolator call, each under a fresh context, against
    the CPU oracle: output, input gradient, every parameter gradient."""
    from afigan_amd import _lib
    gp, x, ref, dx_ref, grads_ref = schedule_case
    cx = _lib.Ctx(dtype)
    for k, v in options.items():
        cx.set_option(k, v)
    G = amd.Generator(in_channels=128, n_residual_dense_blocks=2, growth_rate=32).cuda()
    G.load_state_dict(gp)
    xg = x.cuda().requires_grad_(True)
    with _lib.use_ctx(cx):
        out = G(xg)
        (out * torch.linspace(-1, 1, out.numel(), device="cuda").view_as(out)).sum().backward()
    errs = {"out": _rel(out, ref), "dx": _rel(xg.grad, dx_ref)}
    errs.update({k: _rel(_logical(p.grad), grads_ref[k]) for k, p in G.named_parameters()})
    print(f"schedule {dtype} {options}: worst {max(errs, key=errs.get)} {max(errs.values()):.2e}")
    assert set(grads_ref) <= set(errs)
    for k, e in errs.items():
        assert e < 1e-3, (k, e)


@pytest.mark.parametrize("shape", [(2, 26, 42), (1, 13, 21)])
def test_discriminator_stats_only_forward_has_the_same_side_effects(amd, shape):
    """afi_discriminator_fwd(training = 3) -- the G phase's D(real) call of stage1_trainer.py:401-403, whose logits nothing reads -- leaves the
    BatchNorm running statistics and counters bit-identical to the full forward-only call (training = 2) and writes no logits."""
    import ctypes as C
    from afigan_amd import _lib, ops
    N, H, W = shape
    dp = orc.closed_form_discriminator_params()
    x = ops.pixel_major(torch.randn((N, 256, H, W), generator=torch.Generator().manual_seed(31)).cuda())
    states = {}
    for mode in (2, 3):
        D = amd.Discriminator().cuda()
        D.load_state_dict(dp)
        D.train()
        net = D.Discriminators[0]
        prm, keep = net._param_struct(net._ordered_params())
        F = (C.c_int * 4)(*net.F)
        n = _lib.load().afi_discriminator_fwd_ws_floats(F, N, H, W)
        ws = torch.empty(n, device="cuda")
        logits = torch.full((N, 1, H, W), 7.0, device="cuda")
        _lib.call("afi_discriminator_fwd", C.byref(prm), ops.view_of(x), N, H, W, C.c_void_p(logits.data_ptr()), mode, C.c_void_p(ws.data_ptr()), n,
                  ops.stream_ptr())
        torch.cuda.synchronize()
        states[mode] = ({k: v.clone() for k, v in D.state_dict().items() if "running" in k or "num_batches" in k}, logits.clone())
    assert states[2][0].keys() == states[3][0].keys() and len(states[2][0]) == 9
    for k in states[2][0]:
        assert torch.equal(states[2][0][k], states[3][0][k]), k
    assert not torch.equal(states[2][1], torch.full_like(states[2][1], 7.0)) and torch.equal(states[3][1], torch.full_like(states[3][1], 7.0))


@pytest.mark.parametrize("F0,N,H,W,train", [(256, 2, 13, 21, 1), (256, 2, 50, 84, 1), (256, 1, 32, 40, 0), (16, 2, 9, 11, 1), (96, 1, 17, 5, 1),
                                            # the forward's channel loop (batches of four 16-channel steps, then a remainder loop): F3 = 48 is three
                                            # remainder steps and no batch, 80 one batch + one step, 112 one batch + three; P = 50400 is 788 row tiles
                                            # (> 768 blocks: a block walks two) and the backward sums at their 512-chunk cap
                                            (12, 2, 9, 11, 1), (20, 1, 17, 5, 1), (28, 2, 9, 11, 1), (16, 1, 224, 225, 1)])
def test_discriminator_fused_tail_is_the_same_network(amd, F0, N, H, W, train):
    """Option d_fuse_tail (default on): block 2's BatchNorm apply + LeakyReLU, the last conv and their backward without y[2] and without the
    gradient w.r.t. it in memory (feature_patch_discriminator.py:38-41; csrc/elementwise.hip, afi_launch_disc_tail_*).  Against the separate
    passes (option off) on the same inputs: the same LeakyReLU decisions (the pinned affine on the same conv output), sums in another order --
    logits, input gradient and every parameter gradient to fp32 rounding; y[2] is not even reserved (the context's workspace is P x F3 floats
    smaller, and the call stays inside it) and the mask of afi_discriminator_saved_activations says so.  Channel counts that fill a wave's 256 channels (1024), a part of one (64: masked lanes)
    and one and a half (384); batch statistics and running statistics (eval)."""
    import ctypes as C
    from afigan_amd import _lib, ops
    lib = _lib.load()
    torch.manual_seed(11)
    D = amd.Discriminator(in_filters=F0).cuda()
    D.train(bool(train))
    net = D.Discriminators[0]
    if not train:                                           # running statistics that are not the initial (0, 1)
        for m in net.modules():
            if hasattr(m, "running_mean") and m.running_mean is not None:
                m.running_mean.normal_(0, 0.3); m.running_var.uniform_(0.5, 2.0)
    x = ops.pixel_major(torch.randn(N, F0, H, W).cuda())
    dl = torch.randn(N * H * W, device="cuda")
    params = net._ordered_params()
    Fa = (C.c_int * 4)(*net.F)
    nf, nb = lib.afi_discriminator_fwd_ws_floats(Fa, N, H, W), lib.afi_discriminator_bwd_ws_floats(Fa, N, H, W)
    off = (C.c_longlong * 12)()
    _lib.call("afi_discriminator_ws_layout", Fa, N, H, W, off)
    res, nfx = {}, {}
    for flag in (0, 1):
        cx = _lib.Ctx()
        cx.set_option("d_fuse_tail", flag)
        cx.set_option("deterministic", 1)
        assert lib.afi_discriminator_saved_activations(cx.handle, Fa, N, H, W) == (3 if flag else 7)
        nfx[flag] = lib.afi_discriminator_fwd_ws_floats_ex(cx.handle, Fa, N, H, W, 1 if train else 0)     # what THIS context's call needs
        with _lib.use_ctx(cx):
            prm, keep = net._param_struct(params)
            grads = [torch.zeros_like(t) for t in keep]
            gst, _k2 = net._param_struct(grads, already_packed=True, grads=True)
            ws, sc = torch.full((nfx[flag] + 4096,), float("nan"), device="cuda"), torch.zeros(nb, device="cuda")      # (+ a guard behind it)
            logits = torch.empty(N * H * W, device="cuda")
            dx = ops.new_pixel_major(N, F0, H, W, "cuda")
            st = ops.stream_ptr()
            _lib.call("afi_discriminator_fwd", C.byref(prm), ops.view_of(x), N, H, W, C.c_void_p(logits.data_ptr()), 1 if train else 0, C.c_void_p(ws.data_ptr()), nfx[flag], st)
            y2_written = flag == 0 and not bool(torch.isnan(ws[off[5]:off[5] + 8]).any())
            if train:
                _lib.call("afi_discriminator_bwd", C.byref(prm), C.byref(gst), ops.view_of(x), N, H, W, C.c_void_p(ws.data_ptr()), C.c_void_p(dl.data_ptr()),
                          C.c_void_p(dx.data_ptr()), C.c_void_p(sc.data_ptr()), nb, st)
            torch.cuda.synchronize()
        assert y2_written == (flag == 0)
        assert bool(torch.isnan(ws[nfx[flag]:]).all()), "the call wrote behind the workspace its context asked for"
        res[flag] = (logits.clone(), dx.clone(), [g.clone() for g in grads])
    assert nfx[0] - nfx[1] == N * H * W * net.F[3] and nfx[0] <= nf
    assert _rel(res[1][0], res[0][0]) < 2e-6, "logits"
    if train:
        assert _rel(res[1][1], res[0][1]) < 1e-5, "input gradient"
        for i, (a, b) in enumerate(zip(res[1][2], res[0][2])):
            if float(b.abs().max()) == 0.0:
                assert float(a.abs().max()) == 0.0, i
            else:
                assert _rel(a, b) < 2e-5, i


@pytest.mark.parametrize("N,H,W", [(2, 50, 84), (1, 40, 36)])
def test_discriminator_winograd_forward_backward_reads_nothing_it_did_not_write(amd, N, H, W):
    """The default Winograd forward + backward of the discriminator (feature_patch_discriminator.py:35-41) on a forward workspace AND a backward
    scratch filled with NaN: whatever a pass reads of either, it wrote before -- logits, the input gradient and every parameter gradient come
    out finite, and the gradients of the conv biases that feed a train-mode BatchNorm are exactly zero (nets.hip: disc_bwd adds nothing to
    them).  The forward writes the activations of blocks 0 and 1 (afi_discriminator_saved_activations: 3; y[2] is the fused tail's) and the
    context's own workspace query stays inside the context-free one.  8400 pixels: F(4x4) gradients, block 2's forward planes kept for the
    backward; 1440: F(2x2)."""
    import ctypes as C
    from afigan_amd import _lib, ops
    lib = _lib.load()
    torch.manual_seed(12)
    D = amd.Discriminator(in_filters=256).cuda()
    D.train()
    net = D.Discriminators[0]
    x = ops.pixel_major(torch.randn(N, 256, H, W).cuda())
    dl = torch.randn(N * H * W, device="cuda")
    params = net._ordered_params()
    Fa = (C.c_int * 4)(*net.F)
    nf, nb = lib.afi_discriminator_fwd_ws_floats(Fa, N, H, W), lib.afi_discriminator_bwd_ws_floats(Fa, N, H, W)
    off = (C.c_longlong * 12)()
    _lib.call("afi_discriminator_ws_layout", Fa, N, H, W, off)
    cx = _lib.Ctx()
    cx.set_option("deterministic", 1)
    assert lib.afi_discriminator_saved_activations(None, Fa, N, H, W) == 3                              # (bit 2: never, d_fuse_tail)
    assert lib.afi_discriminator_saved_activations(cx.handle, Fa, N, H, W) == 3
    assert lib.afi_discriminator_fwd_ws_floats_ex(cx.handle, Fa, N, H, W, 1) <= nf
    with _lib.use_ctx(cx):
        prm, keep = net._param_struct(params)
        grads = [torch.zeros_like(t) for t in keep]
        gst, _k2 = net._param_struct(grads, already_packed=True, grads=True)
        ws, sc = torch.full((nf,), float("nan"), device="cuda"), torch.full((nb,), float("nan"), device="cuda")
        logits = torch.empty(N * H * W, device="cuda")
        dx = ops.new_pixel_major(N, 256, H, W, "cuda")
        st = ops.stream_ptr()
        _lib.call("afi_discriminator_fwd", C.byref(prm), ops.view_of(x), N, H, W, C.c_void_p(logits.data_ptr()), 1, C.c_void_p(ws.data_ptr()), nf, st)
        y0_written = not bool(torch.isnan(ws[off[3]:off[3] + 8]).any())
        _lib.call("afi_discriminator_bwd", C.byref(prm), C.byref(gst), ops.view_of(x), N, H, W, C.c_void_p(ws.data_ptr()), C.c_void_p(dl.data_ptr()),
                  C.c_void_p(dx.data_ptr()), C.c_void_p(sc.data_ptr()), nb, st)
        torch.cuda.synchronize()
    assert y0_written
    assert bool(torch.isfinite(logits).all()), "logits"
    assert bool(torch.isfinite(dx).all()), "input gradient"
    for i, g in enumerate(grads):                           # (w, b, gamma, beta) x 3 blocks, then w3, b3
        assert bool(torch.isfinite(g).all()), i
        if i in (1, 5, 9):
            assert float(g.abs().max()) == 0.0, i
        else:
            assert float(g.abs().max()) > 0.0, i


def test_interpolator_default_gradient_deviation_not_above_torch_fp32(amd):
    """The interpolator's counterpart of tests/test_gpu_d_parity.py::test_default_forward_gradient_deviation_not_above_torch_fp32:
    its LeakyReLUs sit behind 32-channel growth convs, whose masks an fp32 implementation decides by its conv rounding.  Forward + backward at
    2x256x52x84 (the P3 call of the stage-1 step) under the library's DEFAULT options against an fp64 evaluation of the oracle's op sequence
    (torch ops on the GPU), beside torch's own fp32 ops on the same inputs: the worst parameter gradient's relative-L2 deviation must not exceed
    torch fp32's (profiles/r05/gflip_interpolator_forwards.txt: 2.2e-4 against 4.4e-4), dx -- no mask in front of it that the loss weights
    reach with more than rounding -- stays at the 1e-6 level.  What this bar excludes, and why the non-default paths are where they are:
    the F(4x4) forwards (winograd_f4_forward bit 16: 3.4e-3) and the exact-fp32 DIRECT kernels (winograd = 0: 1.9e-3) -- an fp32 MFMA chain of
    K / 2 = 1152+ dependent additions per output rounds more than torch's blocked sums or the 16-plane Winograd form, and every flipped mask of
    a growth conv moves its (small) weight-gradient tensor by ~1e-3; the direct kernels are the fallback for ragged / small maps, where the
    masks per tensor are few, and are held to the 1e-3 forward bar by the module fixtures."""
    from oracle import afigan_oracle as orc
    torch.backends.cudnn.allow_tf32 = False
    torch.manual_seed(0)
    G = amd.Generator(n_residual_dense_blocks=3).cuda().train()
    x0 = torch.randn(2, 256, 52, 84, device="cuda")
    r = torch.randn(2, 256, 104, 168, device="cuda")
    names = [n for n, _ in G.named_parameters()]
    sd = {k: v.detach().clone() for k, v in G.state_dict().items()}

    def torch_run(dt):
        p = {k: v.detach().clone().to(dt).contiguous().requires_grad_(True) for k, v in sd.items()}       # (clone: .to(same dtype) is the tensor itself)
        xx = x0.detach().clone().to(dt).requires_grad_(True)
        (orc.generator_forward(xx, p, n_rdb=3) * r.to(dt)).sum().backward()
        return {"dx": xx.grad.double(), **{n: p[n].grad.double() for n in names}}

    ref, t32 = torch_run(torch.float64), torch_run(torch.float32)
    x = x0.detach().clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    (G(x) * r).sum().backward()
    lib = {"dx": x.grad.double(), **{n: q.grad.double() for n, q in G.named_parameters()}}
    live = [k for k in ref if ref[k].norm() > 1e-9 * ref[k].numel() ** 0.5]
    dev = lambda o: (((o["dx"] - ref["dx"]).norm() / ref["dx"].norm()).item(), max(((o[k] - ref[k]).norm() / ref[k].norm()).item() for k in live))   # noqa: E731
    (ldx, lw), (tdx, tw) = dev(lib), dev(t32)
    print(f"interpolator default: dx {ldx:.3e} worst {lw:.3e}; torch fp32: dx {tdx:.3e} worst {tw:.3e}")
    assert lw <= tw, (lw, tw)
    assert ldx < 1e-6 and ldx <= 3.0 * tdx, (ldx, tdx)
