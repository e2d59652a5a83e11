"""bf16 / fp16 activations at the boundary of the AF interpolator and the AFI FPN / PAFPN (torch.autocast).

The contract: a 2-byte input runs the fp32 computation on its widened values, and every 2-byte result is the fp32 result rounded ONCE
(torch's .to(dtype)).  So each check here is bit equality against the fp32 path, not a tolerance:
  casts       widen == t.float(); narrow == t.to(dtype) on ties, +-0, subnormals, NaN, +-inf and fp16 overflow
  Generator   output and input gradient == the fp32 run's rounded, parameter gradients == the fp32 run's, on each final-conv route
  FPN/PAFPN   p2..p6 and the bottom-up gradients == the fp32 module's rounded, parameter gradients equal; and closer to the fp64 oracle
              than the oracle itself run under torch.autocast (what the reference does under AMP)
  FPN/PAFPN   also without torch.autocast: the same bits as inside it
  Winograd    the 3x3 output conv's Winograd route (p2 / p3 at detector sizes): 2-byte store, and the backward from a 2-byte gradient
  refusals    mixed levels, fp64, and the modules outside the feature keep rejecting 2-byte tensors; a stand-alone Generator takes a 2-byte
              map under torch.autocast only (tests/test_gpu_modules.py::test_error_paths pins the fp16 refusal outside it)
Contexts run with deterministic = 1 (no fp32 atomics in the weight gradients), so two runs can agree bit for bit."""
import ctypes as C
import csv

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from oracle import afigan_oracle as orc  # noqa: E402

HALF = [torch.bfloat16, torch.float16]
_I16 = torch.int16


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


def _same_bits(a, b):
    """bit equality of two 2-byte tensors, any NaN matching any NaN (NaN stays NaN; its payload is not part of the contract)"""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return torch.equal(a.contiguous().view(_I16)[~na.contiguous()], b.contiguous().view(_I16)[~nb.contiguous()])


def _layouts(t):
    """(name, view) of one [N,C,H,W] source: NCHW-contiguous, channels_last, a channel slice of a wider channels_last tensor, and one
    that starts at an odd element (2-byte aligned only: the one-element-per-thread form)"""
    N, C_, H, W = t.shape
    wide = torch.zeros((N, C_ + 8, H, W), device=t.device, dtype=t.dtype).contiguous(memory_format=torch.channels_last)
    wide[:, 4:4 + C_] = t
    odd = torch.zeros((N, C_ + 8, H, W), device=t.device, dtype=t.dtype).contiguous(memory_format=torch.channels_last)
    odd[:, 1:1 + C_] = t
    return [("nchw", t.contiguous()), ("channels_last", t.contiguous(memory_format=torch.channels_last)), ("slice", wide[:, 4:4 + C_]),
            ("odd_slice", odd[:, 1:1 + C_])]


# ------------------------------------------------------------------------------------------------ casts
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("C_", [3, 4, 6, 36, 256])
@pytest.mark.parametrize("shape", [(1, 13, 21), (2, 25, 34)])
def test_widen_is_exact(amd, dtype, C_, shape):
    from afigan_amd import ops
    N, H, W = shape
    g = torch.Generator().manual_seed(C_ + H)
    t = (torch.randn((N, C_, H, W), generator=g) * 3).to(dtype).cuda()
    for name, v in _layouts(t):
        w, dt = ops.ingest(v)
        assert dt == dtype and w.dtype == torch.float32 and ops.is_dense_pm(w), name
        assert torch.equal(w, v.float()), name


def _crafted(dtype, n):
    """fp32 values whose rounding to `dtype` is decided by the rule: exact ties (both parities), +-0, subnormals of both formats, NaN,
    +-inf, fp16 overflow and its boundary; the rest random normal"""
    if dtype == torch.bfloat16:
        u = 2.0 ** -7                                   # ulp of bf16 at 1
        special = [1 + u / 2, 1 + 3 * u / 2, -(1 + u / 2), -(1 + 3 * u / 2), 2.0 ** -130, -3 * 2.0 ** -134, 2.0 ** -126 * (1 + 2.0 ** -8),
                   3.3895e38, 3.4e38]
    else:
        u = 2.0 ** -10
        special = [1 + u / 2, 1 + 3 * u / 2, -(1 + u / 2), -(1 + 3 * u / 2), 2.0 ** -20, 3 * 2.0 ** -25, 2.0 ** -25, -2.0 ** -26,
                   65504.0, 65519.0, 65520.0, 70000.0, -1e6]
    special += [0.0, -0.0, float("nan"), float("inf"), float("-inf")]
    v = torch.randn(n, generator=torch.Generator().manual_seed(n))
    s = torch.tensor(special, dtype=torch.float32)
    reps = (n // 4) // len(s)
    v[: reps * len(s)] = s.repeat(reps)
    return v[torch.randperm(n, generator=torch.Generator().manual_seed(1))]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("C_", [4, 36, 256])
@pytest.mark.parametrize("shape", [(1, 13, 21), (2, 25, 34)])
def test_narrow_rounds_like_torch(amd, dtype, C_, shape):
    from afigan_amd import ops
    N, H, W = shape
    t = _crafted(dtype, N * C_ * H * W).reshape(N, H, W, C_).cuda().permute(0, 3, 1, 2)        # dense pixel-major fp32
    wide = torch.zeros((N, H, W, C_ + 8), device="cuda").permute(0, 3, 1, 2)
    wide[:, 4:4 + C_] = t
    for name, v in (("dense", t), ("slice", wide[:, 4:4 + C_])):
        n = ops.narrow(v, dtype)
        assert n.dtype == dtype and ops.is_dense_pm(n), name
        assert _same_bits(n, v.to(dtype)), name


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("C_", [3, 6, 36])
def test_narrow_one_element_per_thread(amd, dtype, C_):
    """afi_cast_from_f32_nhwc where no vector access is allowed: C not a multiple of 4 (source strides of C floats), or a destination that
    is 2-byte aligned only (one element into its buffer)"""
    from afigan_amd import _lib, ops
    N, H, W = 2, 13, 21
    n = N * H * W * C_
    src = _crafted(dtype, n).reshape(N, H, W, C_).cuda()                      # dense [N][H][W][C] fp32
    ref = src.to(dtype)
    for off in (0, 1):
        buf = torch.zeros(n + 8, device="cuda", dtype=dtype)
        v = _lib.View(src.data_ptr(), H * W * C_, W * C_, C_)
        _lib.call("afi_cast_from_f32_nhwc", v, N, H, W, C_, C.c_void_p(buf.data_ptr() + 2 * off), ops.STORE_DTYPES[dtype], ops.stream_ptr())
        torch.cuda.synchronize()
        got = buf[off:off + n].reshape(N, H, W, C_)
        assert _same_bits(got, ref), off
        assert float(buf[:off].float().abs().sum()) == 0.0 and float(buf[off + n:].float().abs().sum()) == 0.0, "wrote outside dst"


# ------------------------------------------------------------------------------------------------ Generator
def _ctx(amd, dtype, winograd=1):
    from afigan_amd import _lib
    cx = _lib.Ctx(dtype)
    cx.set_option("deterministic", 1)
    cx.set_option("winograd", winograd)
    return cx


def _final_conv_route(path, N, C_, H, W):
    """which kernel stored the final conv's [N, C, 2H, 2W] output, from an afi_profile_dump of one forward"""
    pix = {0, 1, 2, 3, 4, 5, 6, 7, 11, 12}
    with open(path) as f:
        rows = [(r["kind"], int(r["rows"]), int(r["cols"]), int(r["planes"])) for r in csv.DictReader(f)]
    names = {k: _kind_name(k) for k in range(23)}
    at_hi = [k for k, m, n, pl in rows if m == 4 * N * H * W and n == C_]
    if any(k == names[20] for k in at_hi):
        return "wk6"
    if any(k == names[15] for k in at_hi):
        return "smallmap"
    if any(k in (names[i] for i in pix) for k in at_hi):
        return "direct"
    if not at_hi and any(m >= 16 * N * H * W and n == C_ for k, m, n, pl in rows):     # the 16 transform planes of the hi-res map
        return "winograd"
    return f"unknown: {rows}"


def _kind_name(k):
    from afigan_amd import _lib
    return _lib.load().afi_profile_kind_name(k).decode()


# (shape, context option winograd, the route the final conv must take under f16x3 / under fp32)
G_CASES = [((1, 256, 13, 21), 1, "wk6", "smallmap"), ((1, 256, 25, 34), 1, "wk6", "winograd"),
           ((2, 256, 50, 84), 1, "winograd", "winograd"), ((2, 256, 50, 84), 0, "direct", "direct")]


@pytest.mark.parametrize("case", range(len(G_CASES)))
@pytest.mark.parametrize("cdt", ["f16x3", "fp32"])
@pytest.mark.parametrize("dtype", HALF)
def test_generator_is_fp32_path_rounded_once(amd, tmp_path, case, cdt, dtype):
    from afigan_amd import _lib
    shape, wino, route16, route32 = G_CASES[case]
    N, C_, H, W = shape
    G = amd.Generator(in_channels=C_, n_residual_dense_blocks=3).cuda()
    G.load_state_dict(orc.closed_form_generator_params(C_, 3, 32))
    gen = torch.Generator().manual_seed(H * W + N)
    x16 = torch.randn(shape, generator=gen).to(dtype).cuda()
    if case % 2:
        x16 = x16.contiguous(memory_format=torch.channels_last)
    dout16 = torch.randn((N, C_, 2 * H, 2 * W), generator=gen).to(dtype).cuda()
    if case % 2 == 0:
        dout16 = dout16.contiguous(memory_format=torch.channels_last)
    cx = _ctx(amd, cdt, wino)
    lib = _lib.load()
    res = {}
    with _lib.use_ctx(cx):
        for kind in ("fp32", "half"):
            for p in G.parameters():
                p.grad = None
            x = (x16.float() if kind == "fp32" else x16).clone().requires_grad_(True)
            if kind == "half":
                lib.afi_profile_enable(1)
            with torch.autocast("cuda", dtype=dtype):           # (2-byte activations are taken under autocast; the fp32 run is unaffected by it)
                y = G(x)
            if kind == "half":
                torch.cuda.synchronize()
                path = str(tmp_path / "prof.csv")
                assert lib.afi_profile_dump(path.encode()) == 0
                lib.afi_profile_enable(0)
                route = _final_conv_route(path, N, C_, H, W)
            y.backward(dout16.float() if kind == "fp32" else dout16)
            torch.cuda.synchronize()
            res[kind] = (y.detach(), x.grad.detach(), {k: p.grad.detach().clone() for k, p in G.named_parameters()})
    assert route == (route16 if cdt == "f16x3" else route32), route
    y32, dx32, pg32 = res["fp32"]
    y16, dx16, pg16 = res["half"]
    assert y16.dtype == dtype and y16.is_contiguous(memory_format=torch.channels_last)
    assert dx16.dtype == dtype
    assert _same_bits(y16, y32.to(dtype)), "output"
    assert _same_bits(dx16, dx32.to(dtype)), "input gradient"
    for k in pg32:
        assert pg16[k].dtype == torch.float32 and torch.equal(pg16[k], pg32[k]), k


# ------------------------------------------------------------------------------------------------ FPN / PAFPN under autocast
class _BottomUp(nn.Module):
    """Stand-in bottom-up network (tests/test_gpu_fpn.py): hands back the feature maps it is given (res2..res5)."""

    def __init__(self, chans, strides):
        super().__init__()
        self.chans, self.strides = chans, strides

    def output_shape(self):
        from afigan_amd.fpn_sr import ShapeSpec
        return {f"res{i + 2}": ShapeSpec(c, s) for i, (c, s) in enumerate(zip(self.chans, self.strides))}

    def forward(self, feats):
        return feats


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


@pytest.mark.parametrize("kind", ["fpn", "pafpn"])
@pytest.mark.parametrize("fuse_type", ["sum", "avg"])
@pytest.mark.parametrize("top", [True, False])
@pytest.mark.parametrize("dtype", HALF)
def test_pyramid_under_autocast(amd, kind, fuse_type, top, dtype):
    from afigan_amd import _lib
    chans, strides, C_ = [8, 12, 16, 20], [4, 8, 16, 32], 32
    N, H5, W5 = 2, 2, 3
    bu = _BottomUp(chans, strides)
    cls = amd.FPN_AFIGAN if kind == "fpn" else amd.PAFPN_AFIGAN
    net = cls(bu, ["res2", "res3", "res4", "res5"], C_, norm="", top_block=amd.LastLevelMaxPool() if top else None, fuse_type=fuse_type).cuda()
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if k.endswith("bias"):
                v.copy_(orc.closed_form_tensor(k, v.shape, 0.05))
        net.srf_module.load_state_dict(orc.closed_form_generator_params(C_, 3, 32))
    feats = {f"res{i + 2}": torch.randn((N, c, H5 * 2 ** (3 - i), W5 * 2 ** (3 - i)), generator=gen).to(dtype).cuda()
             for i, c in enumerate(chans)}
    names = ["p2", "p3", "p4", "p5"] + (["p6"] if top else [])
    R = {k: torch.randn((N, C_, H5 * 2 ** (3 - i), W5 * 2 ** (3 - i)), generator=gen).to(dtype).cuda() for i, k in enumerate(names[:4])}
    if top:
        R["p6"] = torch.randn((N, C_, H5 // 2 + H5 % 2, W5 // 2 + W5 % 2), generator=gen).to(dtype).cuda()
    cx = _ctx(amd, "f16x3")
    res = {}
    with _lib.use_ctx(cx):
        for run in ("fp32", "half", "half_no_autocast"):        # (a backbone cast to 2 bytes hands over the same maps without autocast)
            for p in net.parameters():
                p.grad = None
            fg = {k: (v.float() if run == "fp32" else v).clone().requires_grad_(True) for k, v in feats.items()}
            if run == "half":
                with torch.autocast("cuda", dtype=dtype):
                    out = net(fg)
            elif run == "half_no_autocast":
                out = net(fg)
            else:
                out = net(fg)
                for o in out.values():                 # the gradient reaching a 2-byte level is 2-byte (autograd sums p5's and p6's in it)
                    o.register_hook(lambda g: g.to(dtype).float())
            assert list(out) == names
            loss = sum((o.float() * R[k].float()).sum() for k, o in out.items())
            loss.backward()
            torch.cuda.synchronize()
            res[run] = ({k: o.detach() for k, o in out.items()}, {k: v.grad for k, v in fg.items()},
                        {k: p.grad.clone() for k, p in net.named_parameters()})
    o32, g32, p32 = res["fp32"]
    o16, g16, p16 = res["half"]
    for k in names:
        assert o16[k].dtype == dtype and _same_bits(o16[k], o32[k].to(dtype)), k
    for k in feats:
        assert g16[k].dtype == dtype and _same_bits(g16[k], g32[k].to(dtype)), k
    for k in p32:
        assert p16[k].dtype == torch.float32 and torch.equal(p16[k], p32[k]), k
    on, gn, pn = res["half_no_autocast"]
    for k in names:
        assert on[k].dtype == dtype and _same_bits(on[k], o16[k]), k
    for k in feats:
        assert gn[k].dtype == dtype and _same_bits(gn[k], g16[k]), k
    for k in p32:
        assert torch.equal(pn[k], p16[k]), k

    # against the fp64 oracle: rounding once beats the reference's own autocast run, which rounds after every layer
    fwd = orc.fpn_afigan_forward if kind == "fpn" else orc.pafpn_afigan_forward
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    order = [feats[f"res{i + 2}"] for i in range(4)]
    ref = fwd([f.double().cpu() for f in order], [2, 3, 4, 5], {k: v.double().cpu() for k, v in sd.items()}, fuse_type=fuse_type,
              last_level_maxpool=top)
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        amp = fwd(order, [2, 3, 4, 5], sd, fuse_type=fuse_type, last_level_maxpool=top)
    ours = max(_rel(o16[k], ref[k]) for k in names)
    theirs = max(_rel(amp[k], ref[k]) for k in names)
    assert ours <= theirs, (ours, theirs)


@pytest.mark.parametrize("dtype", HALF)
def test_output_conv_winograd_route(amd, dtype):
    """The pyramid's 3x3 output conv on a map large enough for its Winograd route (fpn_sr._winograd_pays: p2 / p3 at detector sizes):
    afi_conv3x3_wino_fwd_out16 stores the fp32 result rounded once, and the backward from a 2-byte gradient (widened, then the Winograd
    data / weight gradients) equals the fp32 backward from that gradient's fp32 values."""
    from afigan_amd import _lib, fpn_sr
    N, C_, H, W = 1, 256, 64, 64
    gen = torch.Generator().manual_seed(11)
    x0 = torch.randn((N, C_, H, W), generator=gen).cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn((C_, C_, 3, 3), generator=gen) / 48).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    b = (torch.randn(C_, generator=gen) * 0.1).cuda().requires_grad_(True)
    dy16 = torch.randn((N, C_, H, W), generator=gen).to(dtype).cuda()
    assert fpn_sr._winograd_pays(x0, C_)
    res = {}
    with _lib.use_ctx(_ctx(amd, "f16x3")):
        for run, odt in (("fp32", torch.float32), ("half", dtype)):
            w.grad = b.grad = None
            x = x0.clone().requires_grad_(True)
            y = fpn_sr._Conv3x3Fn.apply(x, w, b, odt)
            y.backward(dy16 if run == "half" else dy16.float())
            torch.cuda.synchronize()
            res[run] = (y.detach(), x.grad.clone(), w.grad.clone(), b.grad.clone())
    y32, dx32, dw32, db32 = res["fp32"]
    y16, dx16, dw16, db16 = res["half"]
    assert y16.dtype == dtype and y16.is_contiguous(memory_format=torch.channels_last)
    assert _same_bits(y16, y32.to(dtype))
    assert dx16.dtype == torch.float32 and torch.equal(dx16, dx32)            # (prev, the conv's input, is the fp32 top-down chain)
    assert torch.equal(dw16, dw32) and torch.equal(db16, db32)


# ------------------------------------------------------------------------------------------------ refusals
def test_mixed_levels_and_fp64_are_refused(amd):
    from afigan_amd import _lib
    bu = _BottomUp([8, 8], [4, 8])
    for cls in (amd.FPN_AFIGAN, amd.PAFPN_AFIGAN):
        net = cls(bu, ["res2", "res3"], 32, top_block=None).cuda()
        mixed = {"res2": torch.randn(1, 8, 8, 12, device="cuda").bfloat16(), "res3": torch.randn(1, 8, 4, 6, device="cuda").half()}
        with pytest.raises(_lib.AfiError, match="one dtype"), torch.autocast("cuda", dtype=torch.bfloat16):
            net(mixed)
        f64 = {"res2": torch.randn(1, 8, 8, 12, device="cuda").double(), "res3": torch.randn(1, 8, 4, 6, device="cuda").double()}
        with pytest.raises(_lib.AfiError):
            net(f64)
    G = amd.Generator(in_channels=32, n_residual_dense_blocks=1).cuda()
    with pytest.raises(_lib.AfiError), torch.autocast("cuda", dtype=torch.float16):
        G(torch.randn(1, 32, 4, 6, device="cuda").double())
    with pytest.raises(_lib.AfiError, match="outside torch.autocast"):    # (the stand-alone interpolator: tests/test_gpu_modules.py pins it)
        G(torch.randn(1, 32, 4, 6, device="cuda").half())


@pytest.mark.parametrize("dtype", HALF)
def test_modules_outside_the_feature_still_reject_2byte_input(amd, dtype):
    from afigan_amd import _lib, ops
    D = amd.Discriminator(in_filters=32).cuda()
    with pytest.raises(_lib.AfiError, match="fp32 only"), torch.autocast("cuda", dtype=dtype):
        D(torch.randn(1, 32, 8, 12, device="cuda").to(dtype))

    class _BottomUp3(nn.Module):                       # (tests/test_gpu_bifpn.py)
        _out_feature_strides = {"stage3": 8, "stage4": 16, "stage5": 32}
        _out_feature_channels = {"stage3": 8, "stage4": 12, "stage5": 16}

        def forward(self, feats):
            return feats

    bif = amd.BiFPN_AFIGAN(_BottomUp3(), ["stage3", "stage4", "stage5"], 32, 7, norm="BN", top_block=amd.LastLevelP6P7(16, 32, "BN")).cuda()
    feats = {f"stage{i + 3}": torch.randn(1, c, 16 >> i, 16 >> i, device="cuda").to(dtype) for i, c in enumerate((8, 12, 16))}
    for train in (False, True):
        bif.train(train)
        with pytest.raises(_lib.AfiError, match="fp32 only"), torch.autocast("cuda", dtype=dtype):
            bif(feats)
    with pytest.raises(_lib.AfiError, match="fp32 only"):
        ops.conv3x3_fwd(ops.pixel_major(torch.randn(1, 8, 4, 4, device="cuda").to(dtype)), torch.randn(8, 8, 3, 3, device="cuda"))


def test_2byte_epilogue_refuses_reading_its_output(amd):
    """A 2-byte output is write-only: beta != 0 (the epilogue would read O_old as fp32) is AFI_ERR_UNSUPPORTED, on real device buffers."""
    from afigan_amd import _lib, ops
    lib = _lib.load()
    x = ops.new_pixel_major(1, 32, 8, 8, "cuda")
    x.zero_()
    w = torch.zeros(32, 3, 3, 32, device="cuda")
    out = ops.new_pixel_major(1, 32, 8, 8, "cuda", dtype=torch.bfloat16)
    cx = _lib.current_ctx()
    st = ops.stream_ptr()
    assert lib.afi_conv3x3_fwd_out16(cx.handle, ops.view_of(x), 1, 8, 8, 32, C.c_void_p(w.data_ptr()), None, 32, ops.view_of(out), 1,
                                     1.0, 1.0, 0, st) == 2
    assert lib.afi_conv1x1_dgrad_out16(cx.handle, ops.view_of(x), 1, 8, 8, 32, C.c_void_p(w.data_ptr()), 32, ops.view_of(out), 2,
                                       1.0, 0.5, st) == 2
    assert lib.afi_conv3x3_fwd_out16(cx.handle, ops.view_of(x), 1, 8, 8, 32, C.c_void_p(w.data_ptr()), None, 32, ops.view_of(out), 1,
                                     1.0, 0.0, 0, st) == 0
    torch.cuda.synchronize()
    assert float(out.float().abs().max()) == 0.0
