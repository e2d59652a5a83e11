"""Training the Swin bottom-up on the GPU (afigan_amd/swin_backbone.py trainable_, csrc/swin_train.hip).

Every new kernel against its fp64 closed form (tests/swin_train_f64.py, held to fp64 autograd by test_swin_train_host.py), one block and the
tiny network against fp64 autograd through the restatement of tests/swin_f64.py, determinism, the untouched frozen module, and the detector
around it.  Bars: sums over tokens / pairs and the attention products elementwise_f64.reduction_bars(Ktot, cpu fp32's rel-L2), element-wise
results elementwise_f64.elementwise_bar(terms, r), blocks and networks 4 x torch-CPU-fp32's relative-L2 deviation from fp64 per tensor.
Inputs lie on fp32 grids; measured values are printed."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_f64 as E
import swin_f64 as S
import swin_train_f64 as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


def _r(g, *shape, scale=1.0, offset=0.0):
    """fp64 values on the fp32 grid"""
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale + offset).float().double()


def _pm(t):
    """a CPU [N, H, W, C] tensor as a pixel-major fp32 GPU tensor [N, C, H, W]"""
    return t.permute(0, 3, 1, 2).float().cuda().contiguous(memory_format=torch.channels_last)


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).double().cpu()


def _hold_reduction(tag, got, ref64, ref32, ktot):
    (em, el), (_, cl) = E.errs(got, ref64), E.errs(ref32, ref64)
    bm, bl = E.reduction_bars(ktot, cl)
    print(f"[swin-train] {tag:60s} Ktot {ktot:6d}  max-norm {em:.2e} (bar {bm:.2e})  rel-L2 {el:.2e} (cpu {cl:.2e}, bar {bl:.2e})")
    assert bool(torch.isfinite(got).all()) and em <= bm and el <= bl, (tag, em, bm, el, bl)


def _hold_elementwise(tag, got, ref64, terms, r):
    got = got.detach().double().cpu()
    worst = ((got - ref64).abs() / E.elementwise_bar(terms, r)).max().item()
    print(f"[swin-train] {tag:60s} r {r:3d}  worst error / bar {worst:.3f}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, (tag, worst)


def _hold_gradient(k, got, g64, g32):
    """4 x torch-CPU-fp32's relative-L2 deviation from fp64; a gradient that is exactly zero in fp64 (a branch dropped for every image) must
    be exactly zero.  Returns error / cpu's."""
    if float(g64.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, k
        return 0.0
    e, c = S.rel_err(got.detach(), g64)[0], S.rel_err(g32, g64)[0]
    assert e <= 4 * c, (k, e, c)
    return e / c


def _f32(fn, *args, **kw):
    """the closed form `fn` evaluated in fp32 on the CPU: the yardstick of reduction_bars"""
    return fn(*[a.float() if torch.is_tensor(a) and a.is_floating_point() else a for a in args], **kw)


# ------------------------------------------------------------------------------------------------ 1. LayerNorm backward
# (C, H, W, merge): 2 / 6 / 12 float4 per lane by the normalised width; merges with odd edges; 2 x 40 x 52 tokens: 130 blocks of partials
LN_CASES = [(96, 7, 9, False), (768, 3, 4, False), (768, 3, 4, True), (96, 5, 3, True), (96, 7, 10, True), (96, 40, 52, False)]


def _ln_r(Ct):
    """roundings of one dx element: 8 of its own expression (dy gamma, x - mean, * rstd, g - m1, xhat m2, the second difference, * rstd, the
    beta = 1 add) plus the three wave sums it reads (mean, variance -> rstd, and the larger of m1 / m2), each a chain of 3 adds per float4 of
    the lane and a 6-step tree"""
    return 8 + 3 * (3 * -(-Ct // 256) + 6)


@pytest.mark.parametrize("C,H,W,merge", LN_CASES)
def test_layernorm_backward_vs_fp64(amd, C, H, W, merge):
    from afigan_amd import ops
    g = torch.Generator().manual_seed(C + H * W + merge)
    Ct, Ho, Wo = (4 * C, (H + 1) // 2, (W + 1) // 2) if merge else (C, H, W)
    x, dy = _r(g, 2, H, W, C, scale=3.0, offset=1.0), _r(g, 2, Ho, Wo, Ct)
    gamma = _r(g, Ct, scale=0.1, offset=1.0)
    dx64, dg64, db64, terms = T.layernorm_bwd(dy, x, gamma, merge=merge)
    _, dg32, db32, _ = _f32(T.layernorm_bwd, dy, x, gamma, merge=merge)
    dgam, dbet = torch.full((Ct,), 0.5, device="cuda"), torch.full((Ct,), -0.25, device="cuda")       # += into non-zero gradients
    dx = ops.swin_layernorm_bwd(_pm(dy), _pm(x), gamma.float().cuda(), merge=merge, dgamma=dgam, dbeta=dbet)
    _hold_elementwise(f"layernorm dx C {C} {H}x{W} merge {merge}", _nhwc(dx), dx64, terms, _ln_r(Ct))
    tokens = 2 * Ho * Wo
    _hold_reduction(f"layernorm dgamma C {C} {H}x{W} merge {merge}", dgam.cpu() - 0.5, dg64, dg32, tokens)      # Ktot: the token count
    _hold_reduction(f"layernorm dbeta C {C} {H}x{W} merge {merge}", dbet.cpu() + 0.25, db64, db32, tokens)
    # beta = 1 into a strided view (every second pixel of a larger, sentinel-filled gradient): the pixels in between are bit-unchanged
    big = torch.randn((2, 2 * H, 2 * W, C), generator=torch.Generator().manual_seed(7)).cuda().permute(0, 3, 1, 2)
    before = big.clone()
    view = big[:, :, ::2, ::2]
    base = _nhwc(view)
    ops.swin_layernorm_bwd(_pm(dy), _pm(x), gamma.float().cuda(), merge=merge, dx=view, beta=1.0)
    _hold_elementwise(f"layernorm dx beta 1 C {C} {H}x{W} merge {merge}", _nhwc(view), base + dx64, terms + base.abs(), _ln_r(Ct))
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, :, ::2, ::2] = False
    assert torch.equal(big[mask], before[mask])
    # parameter gradients alone
    dgam2, dbet2 = torch.zeros(Ct, device="cuda"), torch.zeros(Ct, device="cuda")
    assert ops.swin_layernorm_bwd(_pm(dy), _pm(x), gamma.float().cuda(), merge=merge, dgamma=dgam2, dbeta=dbet2, want_dx=False) is None
    _hold_reduction(f"layernorm dgamma alone C {C} {H}x{W} merge {merge}", dgam2.cpu(), dg64, dg32, tokens)


def test_layernorm_backward_refuses_a_short_workspace(amd):
    import ctypes as C
    from afigan_amd import _lib, ops
    x, dy, gamma = torch.zeros(1, 8, 2, 2).cuda().contiguous(memory_format=torch.channels_last), torch.zeros(1, 8, 2, 2).cuda().contiguous(
        memory_format=torch.channels_last), torch.ones(8).cuda()
    need = int(_lib.load().afi_swin_layernorm_bwd_ws_floats(1, 2, 2, 8, 0))
    assert need == 4 * 2 * 8
    ws, dgam, dbet = torch.zeros(need, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    with pytest.raises(amd.AfiError, match="workspace"):
        _lib.call("afi_swin_layernorm_bwd", ops.view_of(x), 1, 2, 2, 8, ops._p(gamma), 1e-5, 0, ops._p(dy), ops._NULL_VIEW, 0.0, ops._p(dgam),
                  ops._p(dbet), ops._p(ws), need - 1, C.c_void_p(0))


# ------------------------------------------------------------------------------------------------ 2. GELU backward
def test_gelu_backward_vs_fp64(amd):
    from afigan_amd import ops
    g = torch.Generator().manual_seed(3)
    x, dy = _r(g, 2, 5, 7, 384, scale=3.0), _r(g, 2, 5, 7, 384)
    ref = T.gelu_bwd(dy, x)
    # the operands' magnitudes: Phi = (1 + erf) / 2 is a sum of terms of size (1 + |erf|) / 2, and the exponent -x^2 / 2 carries its own rounding
    # into phi times x^2 / 2.  r = 12: x / sqrt 2, erf (2 ulp), 1 +, x x, exp (2 ulp), the constant, x phi, the sum, dy *
    terms = dy.abs() * (0.5 * (1 + torch.erf(x / math.sqrt(2.0)).abs()) + x.abs() * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi) * (1 + 0.5 * x * x))
    out = ops.swin_gelu_bwd(_pm(dy), _pm(x))
    _hold_elementwise("gelu backward", _nhwc(out), ref, terms, 12)
    dyg = _pm(dy)
    assert ops.swin_gelu_bwd(dyg, _pm(x), out=dyg) is dyg and torch.equal(dyg, out)                  # in place


# ------------------------------------------------------------------------------------------------ 3. window attention backward, table gradient
ATTN_GRID = [(ws, sh, *s) for ws in (7, 12) for sh in (False, True) for s in [(2, 64, 17, 23), (1, 96, 5, 9), (2, 32, 4, 6), (1, 64, 25, 36)]]


def _attn_case(ws, shifted, B, C, H, W):
    from afigan_amd import swin_backbone
    g = torch.Generator().manual_seed(ws * 1000 + H * 10 + W + shifted)
    heads = C // 32
    qkv, qkv_b = _r(g, B, H, W, 3 * C), _r(g, 3 * C)
    table = _r(g, (2 * ws - 1) ** 2, heads, scale=0.5)
    dout = _r(g, B, H, W, C)
    return qkv, qkv_b, table, swin_backbone.relative_position_index(ws), heads, ws // 2 if shifted else 0, dout


@pytest.mark.parametrize("ws,shifted,B,C,H,W", ATTN_GRID)
def test_window_attention_backward_vs_fp64(amd, ws, shifted, B, C, H, W):
    from afigan_amd import ops
    qkv, qkv_b, table, index, heads, shift, dout = _attn_case(ws, shifted, B, C, H, W)
    ref, _, _ = T.attention_bwd(dout, qkv, qkv_b, table, index, heads, ws, shift)
    ref32, _, _ = _f32(T.attention_bwd, dout, qkv, qkv_b, table, index, heads, ws, shift)
    img = ops.swin_bias_image(table.float().cuda(), index.cuda(), ws)
    dqkv, _ = ops.swin_window_attn_bwd(_pm(dout), _pm(qkv), qkv_b.float().cuda(), img, ws, shift)
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    assert tuple(dqkv.shape) == (B, 3 * C, Hp, Wp)
    got = _nhwc(dqkv)
    real = torch.zeros(Hp, Wp, dtype=torch.bool)
    real[:H, :W] = True
    tag = f"attention ws {ws} shift {shift} {B}x{C}x{H}x{W}"
    for s, name in enumerate(("dq", "dk", "dv")):               # Ktot = ws^2: the window's tokens each product sums over
        sl = slice(s * C, (s + 1) * C)
        _hold_reduction(f"{tag} {name} real", got[:, real][..., sl], ref[:, real][..., sl], ref32[:, real][..., sl], ws * ws)
        _hold_reduction(f"{tag} {name} padded", got[:, ~real][..., sl], ref[:, ~real][..., sl], ref32[:, ~real][..., sl], ws * ws)
    db = ops.bias_grad(dqkv)                                    # d qkv.bias: the column sum over the whole padded buffer (Ktot: its positions)
    _hold_reduction(f"{tag} dqkv_bias", db.cpu(), ref.sum((0, 1, 2)), ref32.sum((0, 1, 2)), B * Hp * Wp)


@pytest.mark.parametrize("ws,shifted,B,C,H,W", ATTN_GRID)
def test_bias_table_gradient_vs_fp64(amd, ws, shifted, B, C, H, W):
    from afigan_amd import ops
    C = max(C, 64)                                              # two heads or more
    qkv, qkv_b, table, index, heads, shift, dout = _attn_case(ws, shifted, B, C, H, W)
    _, dbias, dtable = T.attention_bwd(dout, qkv, qkv_b, table, index, heads, ws, shift)
    _, dbias32, dtable32 = _f32(T.attention_bwd, dout, qkv, qkv_b, table, index, heads, ws, shift)
    img = ops.swin_bias_image(table.float().cuda(), index.cuda(), ws)
    _, ds_part = ops.swin_window_attn_bwd(_pm(dout), _pm(qkv), qkv_b.float().cuda(), img, ws, shift)
    n = ws * ws
    nW = (-(-H // ws)) * (-(-W // ws))
    tag = f"table ws {ws} shift {shift} {B}x{C}x{H}x{W}"
    # an entry of dS = P (dP - rowsum(dP P)) is itself a 32-term dot (dP) less a ws^2-term row sum; B nW of them are added: Ktot = (32 + ws^2) B nW
    _hold_reduction(f"{tag} sum of dS", ds_part.sum(0)[:, :n, :n].cpu(), dbias, dbias32, (32 + n) * B * nW)
    start = _r(torch.Generator().manual_seed(5), *table.shape)
    grad = start.float().cuda()
    ops.swin_bias_table_bwd(ds_part, ops.swin_bias_csr(index.cuda(), ws, table.shape[0]), ws, grad)          # += into a non-zero gradient
    pairs = int(torch.bincount(index.reshape(-1)).max())
    _hold_reduction(f"{tag} dtable", grad.cpu().double() - start, dtable, dtable32, pairs * nW * B)          # Ktot: pairs x windows x images of a row


# Above 2048 blocks a block takes several consecutive windows and adds their dS into one slice (afi_swin_window_attn_bwd_groups); the grid
# above stays at one window per block.  The smallest maps past that threshold with an odd window count, so the last group is ragged:
# 17 x 17 windows of 7 (2 images, 4 heads: 2312 blocks), 11 x 13 windows of 12 (2 images, 8 heads: 2288 blocks); two windows per block.
GROUPED = [(7, 2, 128, 113, 115), (12, 2, 256, 125, 150)]


@pytest.mark.parametrize("ws,B,C,H,W", GROUPED)
def test_window_attention_backward_in_groups_of_windows(amd, ws, B, C, H, W):
    from afigan_amd import _lib, ops
    qkv, qkv_b, table, index, heads, shift, dout = _attn_case(ws, True, B, C, H, W)
    nW = (-(-H // ws)) * (-(-W // ws))
    groups = int(_lib.load().afi_swin_window_attn_bwd_groups(B, H, W, C, ws))
    assert nW % 2 == 1 and groups == (nW + 1) // 2
    ref, dbias, dtable = T.attention_bwd(dout, qkv, qkv_b, table, index, heads, ws, shift)
    ref32, dbias32, dtable32 = _f32(T.attention_bwd, dout, qkv, qkv_b, table, index, heads, ws, shift)
    img = ops.swin_bias_image(table.float().cuda(), index.cuda(), ws)
    dqkv, ds_part = ops.swin_window_attn_bwd(_pm(dout), _pm(qkv), qkv_b.float().cuda(), img, ws, shift)
    assert ds_part.shape[0] == B * groups
    n, tag = ws * ws, f"grouped attention ws {ws} {B}x{C}x{H}x{W}"
    _hold_reduction(f"{tag} dqkv", _nhwc(dqkv), ref, ref32, n)                                               # Ktot = ws^2, as above
    _hold_reduction(f"{tag} sum of dS", ds_part.sum(0)[:, :n, :n].cpu(), dbias, dbias32, (32 + n) * B * nW)
    grad = torch.zeros(table.shape, device="cuda")
    ops.swin_bias_table_bwd(ds_part, ops.swin_bias_csr(index.cuda(), ws, table.shape[0]), ws, grad)
    _hold_reduction(f"{tag} dtable", grad.cpu(), dtable, dtable32, int(torch.bincount(index.reshape(-1)).max()) * nW * B)


# ------------------------------------------------------------------------------------------------ 4. patch gather, scale-add
@pytest.mark.parametrize("shape", [(2, 3, 30, 45), (1, 3, 29, 43)])
def test_patch_gather_is_exact(amd, shape):
    from afigan_amd import ops
    img = _r(torch.Generator().manual_seed(shape[2]), *shape)
    got = ops.swin_patch_gather(img.float().cuda())
    assert torch.equal(_nhwc(got), T.patch_gather(img))         # a copy: ragged right and bottom edges are zero
    w = _r(torch.Generator().manual_seed(1), 32, 3, 4, 4)
    conv = F.conv2d(F.pad(img, (0, (-shape[3]) % 4, 0, (-shape[2]) % 4)), w, stride=4).permute(0, 2, 3, 1)
    out = ops.conv1x1_fwd(got, w.float().cuda().reshape(32, 48))
    assert S.rel_err(_nhwc(out), conv)[0] <= 2e-6               # the channel order is proj.weight.reshape(C, 48)'s


def test_scale_add(amd):
    from afigan_amd import ops
    g = torch.Generator().manual_seed(9)
    a, b = _r(g, 3, 5, 7, 64), _r(g, 3, 5, 7, 64)
    s = torch.tensor([0.0, 1.0 / 0.8, 1.0])
    out = ops.swin_scale_add(_pm(a), s.cuda(), _pm(b))
    assert torch.equal(out[0], _pm(a)[0])                       # the dropped image: bit-equal to a
    sd = s.double()
    _hold_elementwise("scale-add", _nhwc(out), T.scale_add(a, sd, b), a.abs() + (sd.view(-1, 1, 1, 1) * b).abs(), 1)     # one fma
    _hold_elementwise("scale (a = None)", _nhwc(ops.swin_scale_add(None, s.cuda(), _pm(b))), T.scale_add(None, sd, b), (sd.view(-1, 1, 1, 1) * b).abs(), 1)
    bg = _pm(b)
    assert ops.swin_scale_add(None, s.cuda(), bg, out=bg) is bg and float(bg[0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 5. one block
def _block_ref(P, x, heads, ws, shift, s, dtype):
    P = {k: (v.to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in P.items()}
    x = x.to(dtype).clone().requires_grad_(True)
    join = (lambda a, b, row: a + b) if s is None else (lambda a, b, row: T.scale_add(a, s[row].to(dtype), b))
    y = S.layer_norm(x, P["norm1.weight"], P["norm1.bias"])
    x1 = join(x, S.window_attention(y, P["attn.qkv.weight"], P["attn.qkv.bias"], P["attn.proj.weight"], P["attn.proj.bias"],
                                    P["attn.relative_position_bias_table"], P["attn.relative_position_index"], heads, ws, shift), 0)
    y = S.layer_norm(x1, P["norm2.weight"], P["norm2.bias"])
    out = join(x1, F.linear(F.gelu(F.linear(y, P["mlp.fc1.weight"], P["mlp.fc1.bias"])), P["mlp.fc2.weight"], P["mlp.fc2.bias"]), 1)
    return P, x, out


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("shifted", [False, True])
def test_block_against_fp64_autograd(amd, shifted, masks):
    """C 64 on 17 x 23 (pads under window 7): every parameter gradient and the input gradient."""
    from afigan_amd import ops, swin_backbone
    torch.manual_seed(0)
    blk = swin_backbone.SwinTransformerBlock(64, 2, 7, 3 if shifted else 0, 4.0)
    with torch.no_grad():
        for k, p in blk.named_parameters():
            p.copy_(torch.from_numpy(S.weight_rule("layers.0.blocks.0." + k, tuple(p.shape))).float())
            if k.startswith("attn.qkv"):
                p.mul_(T.QKV_SCALE)
    g = torch.Generator().manual_seed(11 + shifted)
    x, dout = _r(g, 2, 17, 23, 64), _r(g, 2, 17, 23, 64)
    s = torch.tensor([[0.0, 1.25], [1.25, 0.0]]) if masks else None
    P = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    refs = {}
    for dtype in (torch.float64, torch.float32):
        Pl, xl, out = _block_ref(P, x, 2, 7, blk.shift, s, dtype)
        keys = [k for k, v in Pl.items() if v.is_floating_point()]
        grads = torch.autograd.grad((out * dout.to(dtype)).sum(), [xl] + [Pl[k] for k in keys])
        refs[dtype] = (out.detach(), dict(zip(["input"] + keys, grads)))
    blk = blk.cuda()
    sg = None if s is None else s.cuda()
    with torch.no_grad():
        out, kept = blk.run_keep(_pm(x), blk.attn.bias_image(), None if sg is None else sg[0], None if sg is None else sg[1])
        if not masks:
            assert torch.equal(out, blk.run(_pm(x), blk.attn.bias_image()))
        got = {}
        csr = ops.swin_bias_csr(blk.attn.relative_position_index, 7, blk.attn.relative_position_bias_table.shape[0])
        names = {id(p): k for k, p in blk.named_parameters()}
        gin = blk.backward(kept, blk.attn.bias_image(), csr, _pm(dout), lambda p, gr: got.__setitem__(names[id(p)], gr),
                           None if sg is None else sg[0], None if sg is None else sg[1])
    got["input"] = gin.permute(0, 2, 3, 1)
    e, e32 = S.rel_err(_nhwc(out), refs[torch.float64][0])[0], S.rel_err(refs[torch.float32][0], refs[torch.float64][0])[0]
    print(f"[swin-train] block shift {blk.shift} masks {masks} output: rel L2 {e:.2e} (cpu fp32 {e32:.2e})")
    assert e <= 2 * e32
    worst = 0.0
    assert set(got) == set(refs[torch.float64][1])
    for k, ref in refs[torch.float64][1].items():
        e, c = S.rel_err(got[k], ref)[0], S.rel_err(refs[torch.float32][1][k], ref)[0]
        worst = max(worst, e / c)
        print(f"[swin-train] block shift {blk.shift} masks {masks} {k:40s} rel L2 {e:.2e} (cpu fp32 {c:.2e}, ratio {e / c:.2f})")
        assert e <= 4 * c, (k, e, c)
    print(f"[swin-train] block shift {blk.shift} masks {masks}: worst gradient at {worst:.2f} x cpu fp32's deviation")


# ------------------------------------------------------------------------------------------------ 6. the tiny network
def _tiny():
    from afigan_amd import swin_backbone
    c = S.TINY
    return T.fill(swin_backbone.SwinTransformer(c["EMBED_DIM"], c["DEPTHS"], c["NUM_HEADS"], c["WINDOW_SIZE"], 4.0, c["OUT_FEATURES"]))


def _cots(out, seed=21):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g).double() for k, v in out.items()}


_REF = {}


def _tiny_reference():
    """fp64 and CPU-fp32 autograd through the restatement, computed once: every gradient of the all-trainable network."""
    if not _REF:
        m, img = _tiny(), S.golden_image()
        with torch.no_grad():
            shapes = S.forward(m, img.double())
        cots = _cots(shapes)
        _REF["cots"] = cots
        _REF[64] = T.network_grads(m, img, cots, torch.float64)
        _REF[32] = T.network_grads(m, img, cots, torch.float32)
    return _REF


def _run_tiny(freeze_at, cots, keys=None):
    m = _tiny().cuda()
    img = S.golden_image().cuda()
    with torch.no_grad():
        frozen_out = {k: v.clone() for k, v in m(img).items()}
    m.trainable_(freeze_at)
    out = m(img)
    sum((out[k] * cots[k].float().cuda()).sum() for k in (keys or out)).backward()
    torch.cuda.synchronize()
    return m, frozen_out, out


@pytest.mark.parametrize("freeze_at", [-1, 0, 3])
def test_tiny_network_against_fp64_autograd(amd, freeze_at):
    ref = _tiny_reference()
    m, frozen_out, out = _run_tiny(freeze_at, ref["cots"])
    for k in frozen_out:
        assert torch.equal(out[k], frozen_out[k]), k            # the training forward is the frozen module's kernel sequence
    worst, seen = 0.0, 0
    for k, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, k
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        g64, g32 = ref[64][1][k], ref[32][1][k]
        e, c = S.rel_err(p.grad, g64)[0], S.rel_err(g32, g64)[0]
        worst, seen = max(worst, e / c), seen + 1
        assert e <= 4 * c, (k, e, c)
    print(f"[swin-train] tiny network freeze_at {freeze_at}: {seen} gradients, worst at {worst:.2f} x cpu fp32's deviation")
    assert seen == len([1 for _, p in m.named_parameters() if p.requires_grad]) > 0


def test_tiny_network_takes_cotangents_on_a_subset(amd):
    m = _tiny()
    img = S.golden_image()
    with torch.no_grad():
        cots = _cots(S.forward(m, img.double()))
    sub = {k: cots[k] for k in ("stage3",)}
    _, g64 = T.network_grads(m, img, sub, torch.float64)
    _, g32 = T.network_grads(m, img, sub, torch.float32)
    net, _, _ = _run_tiny(-1, cots, keys=["stage3"])
    for k, p in net.named_parameters():
        if k in g64:
            assert S.rel_err(p.grad, g64[k])[0] <= 4 * S.rel_err(g32[k], g64[k])[0], k
        else:
            assert p.grad is None, k                            # stages 4 and 5 and their norms: no path to stage3


def test_drop_path_masks_against_fp64_autograd(amd):
    m, img = _tiny(), S.golden_image()
    nb = len(m._blocks())
    masks = (torch.rand((2 * nb, img.shape[0]), generator=torch.Generator().manual_seed(2)) > 0.3).float()
    masks[0, :] = 1
    with torch.no_grad():
        cots = _cots(S.forward(m, img.double()))
    sc = T.drop_scales(m, 0.2, masks)
    o64, g64 = T.network_grads(m, img, cots, torch.float64, scales=sc)
    o32, g32 = T.network_grads(m, img, cots, torch.float32, scales=sc)
    net = _tiny().cuda().trainable_(-1, 0.2).train()
    out = net(img.cuda(), drop_masks=masks.cuda())
    for k in out:
        assert S.rel_err(out[k].detach(), o64[k])[0] <= 2 * S.rel_err(o32[k], o64[k])[0], k
    sum((out[k] * cots[k].float().cuda()).sum() for k in out).backward()
    worst = 0.0
    for k, p in net.named_parameters():
        worst = max(worst, _hold_gradient(k, p.grad, g64[k], g32[k]))
    print(f"[swin-train] tiny network with DropPath masks: worst gradient at {worst:.2f} x cpu fp32's deviation")
    with torch.no_grad():                                       # eval(): the identity, bit-equal to the frozen module
        ev = net.eval()(img.cuda())
        fr = _tiny().cuda()(img.cuda())
    assert all(torch.equal(ev[k], fr[k]) for k in fr)
    drawn = net.train()(img.cuda())                             # masks drawn on the device from torch's generator
    assert all(bool(torch.isfinite(v).all()) for v in drawn.values())


# ------------------------------------------------------------------------------------------------ 7. determinism, the untouched module
def test_determinism_and_poisoned_workspaces(amd, monkeypatch):
    cots = _tiny_reference()["cots"]
    cx = amd._lib.current_ctx()
    prev = cx.get_option("deterministic")
    cx.set_option("deterministic", 1)                           # the weight-gradient GEMM's fixed-order form, as every determinism test here
    try:
        runs = []
        for poison in (False, False, True):
            if poison:
                monkeypatch.setattr(amd.ops, "_POISON", True)
            net, _, out = _run_tiny(-1, cots)
            runs.append(({k: v.detach().clone() for k, v in out.items()}, {k: p.grad.clone() for k, p in net.named_parameters()}))
    finally:
        cx.set_option("deterministic", prev)
    o1, g1 = runs[0]
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())
    for o, g in runs[1:]:
        assert all(torch.equal(o1[k], o[k]) for k in o1)
        assert all(torch.equal(g1[k], g[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g[k])]


def test_a_swin_never_made_trainable_is_the_frozen_module(amd):
    m = _tiny().cuda()
    img = S.golden_image().cuda()
    with torch.no_grad():
        a = m(img)
        y = amd.ops.swin_patch_embed(img, m.patch_embed.proj.weight, m.patch_embed.proj.bias, m.patch_embed.norm.weight, m.patch_embed.norm.bias)
        f = m._prepare()
        for blk in m.layers[0].blocks:
            y = blk.run(y, f[id(blk)])
        assert torch.equal(a["stage2"], amd.ops.swin_layernorm(y, m.norm0.weight, m.norm0.bias))     # today's kernel sequence
    assert not m._trainable and not any(p.requires_grad for p in m.parameters())
    with pytest.raises(amd.AfiError, match=r"^the Swin bottom-up is forward-only \(frozen\): run it under torch.no_grad\(\) with no parameter or input "
                                           r"requiring grad$"):
        m(img.clone().requires_grad_(True))
    with pytest.raises(amd.AfiError, match="drop_masks"):
        m(img, drop_masks=torch.ones(16, 1))


def test_bias_images_follow_an_optimiser_step_and_nothing_else_rebuilds(amd):
    m = _tiny().cuda().trainable_()
    img = S.golden_image().cuda()
    f0 = m._prepare()
    m(img)["stage5"].sum().backward()
    assert m._prepare() is f0                                   # a forward and a backward rebuild nothing
    csr = m._bias_csr()
    opt = amd.DetectorOptim(list(m.named_parameters()), base_lr=1e-3, momentum=0.9)
    opt.step()
    f1 = m._prepare()
    assert f1 is not f0 and m._bias_csr() is csr                # the step moved the tables: new images; the index buffers did not move
    for blk in m._blocks():
        assert torch.equal(f1[id(blk)], blk.attn.bias_image())
    assert not torch.equal(f1[id(m._blocks()[0])], f0[id(m._blocks()[0])])


# ------------------------------------------------------------------------------------------------ 8. the detector around it
def _tiny_bifpn(amd, stages=("stage3", "stage4", "stage5")):
    from afigan_amd import registry, swin_backbone
    cfg = amd.get_cfg()
    cfg.merge_from_dict({"MODEL": {"BACKBONE": {"NAME": "build_swint_bifpn_sr_backbone", "FREEZE_AT": -1}, "SWINT": dict(S.TINY, DROP_PATH_RATE=0.0, OUT_FEATURES=list(stages)),
                                   "BIFPN": {"IN_FEATURES": list(stages), "FPN_REPEAT": 1, "OUT_CHANNELS": 16}}})
    old = dict(registry._BOTTOM_UP)
    try:
        swin_backbone.use_as_bottom_up(trainable=True)
        torch.manual_seed(11)
        bb = amd.BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, None)
    finally:
        registry._BOTTOM_UP.clear()
        registry._BOTTOM_UP.update(old)
    T.fill(bb.bottom_up)
    return bb.cuda()


def test_bifpn_afigan_over_the_trainable_swin(amd):
    bb = _tiny_bifpn(amd).train()
    out = bb(torch.randn((2, 3, 256, 256), generator=torch.Generator().manual_seed(3)).cuda())    # (a multiple of the BiFPN's size divisibility, 128)
    sum(p.sum() for p in out.values()).backward()
    torch.cuda.synchronize()
    swin = bb.bottom_up
    for k, p in swin.named_parameters():
        if k.startswith("norm0."):                              # stage2 is not computed as an output: no gradient
            assert p.grad is None, k
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0), k


def test_detector_step_over_the_trainable_swin(amd):
    """GeneralizedRCNN over BiFPN_AFIGAN over the trainable tiny Swin, a trainable RPN and CascadeROIHeads.trainable_(): two DetectorStep steps
    at 64 x 80.  Frozen parameters are bit-unchanged, the bias images equal a fresh bias_image() after each step."""
    import cascade_train_f64 as K
    features = ["p2", "p3", "p4", "p5", "p6"]                  # stages 2 .. 4 into the BiFPN: the heads of cascade_train_f64 read p2 .. p5
    backbone = _tiny_bifpn(amd, ("stage2", "stage3", "stage4"))
    assert list(backbone.output_shape()) == features
    swin = backbone.bottom_up
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[16], [32], [64], [128], [256]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": features, "PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 50, "PRE_NMS_TOPK_TRAIN": 200,
                                       "POST_NMS_TOPK_TRAIN": 50, "BATCH_SIZE_PER_IMAGE": 32}})
    rpn = amd.RPN(cfg, {f: backbone.output_shape()[f] for f in features}).cuda().trainable_()
    heads = K.build_train_heads(amd, 16, "SyncBN", 3).cuda().trainable_()
    model = amd.GeneralizedRCNN(backbone=backbone, proposal_generator=rpn, roi_heads=heads, pixel_mean=[0.0, 0.0, 0.0], pixel_std=[1.0, 1.0, 1.0],
                                device="cuda").train()
    gts = [np.array([[4, 6, 40, 50], [30, 20, 76, 60], [10, 30, 30, 44]], np.float32), np.array([[8, 8, 60, 40], [40, 34, 70, 62]], np.float32)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()        # noqa: E731
    g = torch.Generator().manual_seed(4)
    batch = []
    for b in gts:
        tg = type("GT", (), {})()
        tg.gt_boxes, tg.gt_classes = dev(b), dev(np.arange(len(b), dtype=np.int64) % 5)
        batch.append({"image": torch.randn((3, 64, 80), generator=g), "targets": tg})
    init = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    opt = amd.DetectorOptim(list(model.named_parameters()), modules=list(model.modules()), base_lr=1e-6, momentum=0.9, weight_decay=1e-3,
                            bias_lr_factor=2.0, weight_decay_bias=0.0, lr_steps=(2,), warmup_factor=0.5, warmup_iters=2,
                            norm_params=amd.detector_optim.norm_module_params(model))
    by_name = dict(zip(opt.names, opt.groups))
    assert by_name["backbone.bottom_up.layers.0.blocks.0.norm1.weight"][1] == 0.0 and by_name["backbone.bottom_up.layers.0.blocks.0.attn.qkv.weight"][1] == 1e-3
    runner = amd.DetectorStep(model, opt)
    for step in range(2):
        losses = runner.run_step(batch)
        assert all(np.isfinite(v) for v in losses.values()), losses
        f = swin._prepare()
        for blk in swin._blocks():
            assert torch.equal(f[id(blk)], blk.attn.bias_image()), step
    now = {n: p.detach().cpu() for n, p in model.named_parameters()}
    frozen_names = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert all(torch.equal(now[n], init[n]) for n in frozen_names)
    swin_names = [n for n in opt.names if n.startswith("backbone.bottom_up.") and ".layers.3." not in n]          # stage 5 is not computed
    moved = sum(int(not torch.equal(now[n], init[n])) for n in swin_names)
    assert moved >= 0.9 * len(swin_names), (moved, len(swin_names))
