"""csrc/cascade_train.hip on the GPU against tests/cascade_train_f64.py (held to torch's float64 BatchNorm and to hand-computed relabel cases
by tests/test_cascade_train_host.py, which also proves the conditions of the fixtures used here).

Relabel: every output EQUALS the checker's on the same fp32 inputs, and the kept boxes equal ops.roi_cascade_stage's boxes at ``src`` bit for
bit; test_relabel_writes_every_output_element repeats every case on NaN- / -7-filled outputs, so an element the kernel does not write shows.
List-masked BatchNorm + ReLU: the bars of tests/test_gpu_elementwise.py, taken from elementwise_f64 unchanged (derived counts, not
measurements; eps = 2^-24):
  statistics, running buffers   <= 1 ulp of the float64 reference's fp32 rounding
  apply                         |got - ref| <= 5 eps (|x - mu| invstd |gamma| + |beta|); zeros at masked-off elements and padding rows exact
  dx given the sums             the r = 8 elementwise form, from the kernel's own sums and y
  sums, dgamma +=, dbeta +=     the reduction form with Ktot = Pn: max-norm <= 2 sqrt(Pn) eps max|ref|, rel. L2 <= 4 max(cpu fp32's, sqrt(Pn) eps / 8)
Padding rows of x, g and y are NaN in every case.  With every row valid the same results meet the same bars against the references of the
dense passes (afi_bn_stats_ex / afi_bn_bwd), and the dense kernels' statistics are reproduced to <= 1 ulp.
The worst error / bar of every op is printed when the module is done."""
import numpy as np
import pytest
import torch

import cascade_train_f64 as T
import elementwise_f64 as E

pytestmark = pytest.mark.gpu

NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module")
def ops():
    import afigan_amd
    assert torch.cuda.is_available()
    yield afigan_amd.ops
    for op, (ratio, case) in sorted(WORST.items()):
        print(f"[cascade_train] worst error / bar  {op:32s} {ratio:8.3f}   {case}")


def _note(op, ratio, case):
    if not (ratio <= WORST.get(op, (-1.0, ""))[0]):
        WORST[op] = (ratio, case)


def _check_elem(op, case, got, ref, terms, r):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (op, case, got.shape, ref.shape)
    ratio = float(((got.double() - ref).abs() / E.elementwise_bar(terms, r)).max())
    _note(op, ratio, case)
    print(f"[cascade_train] {op:24s} {case:40s} worst |err| / ((r+1) eps terms) = {ratio:.3f}   (r = {r})")
    assert ratio <= 1.0, f"{op} {case}: an element misses its bar by {ratio:.3f}x"


def _check_red(op, case, got, ref, cpu32, ktot):
    got = got.detach().cpu().reshape(ref.shape)
    em, el = E.errs(got, ref)
    cm, cl = E.errs(cpu32.reshape(ref.shape), ref)
    bar, l2bar = E.reduction_bars(ktot, cl)
    _note(op + " max-norm", em / bar, case)
    _note(op + " rel-L2", el / l2bar, case)
    print(f"[cascade_train] {op:24s} {case:40s} Ktot {ktot:7d}  max-norm {em:.2e} (cpu fp32 {cm:.2e}, bar {bar:.2e})"
          f"  rel-L2 {el:.2e} (cpu fp32 {cl:.2e}, bar {l2bar:.2e})")
    assert em <= bar, f"{op} {case}: max-norm rel error {em:.3e} > bar {bar:.3e} (cpu fp32 {cm:.3e})"
    assert el <= l2bar, f"{op} {case}: rel-L2 error {el:.3e} > bar {l2bar:.3e} (cpu fp32 {cl:.3e})"


def _check_ulp(op, case, got, ref):
    u = float(E.ulps_from(got, ref).max())
    _note(op + " (ulp)", u, case)
    assert u <= 1.0, f"{op} {case}: {u} ulp from the rounded float64 reference"
    return u


# ------------------------------------------------------------------------------------------------ relabel
@pytest.mark.parametrize("K", T.RELABEL_KS)
@pytest.mark.parametrize("case", range(len(T.RELABEL_CASES)))
def test_relabel_equals_the_checker(ops, case, K):
    c = T.relabel_case(case, K)
    dev = {k: torch.from_numpy(v).cuda() for k, v in c.items() if k != "main"}
    got = ops.roi_cascade_relabel(dev["pred"], K, dev["proposals"], dev["counts"], dev["image_hw"], T.RELABEL_WEIGHTS, dev["gt"], dev["gt_classes"],
                                  dev["counts_g"], T.RELABEL_THRESH)
    # the decode is afi_roi_cascade_stage's, bit for bit: the checker's rule on THAT kernel's boxes must give every output exactly
    _, sb = ops.roi_cascade_stage(dev["pred"], K, dev["proposals"], dev["counts"], dev["image_hw"], T.RELABEL_WEIGHTS)
    ref = T.relabel_boxes(sb.cpu().numpy(), K, c["counts"], c["gt"], c["gt_classes"], c["counts_g"], T.RELABEL_THRESH)
    for k, v in ref.items():
        assert np.array_equal(got[k].cpu().numpy(), v), (k, np.argwhere(got[k].cpu().numpy() != v)[:5])
    for n in range(T.RELABEL_N):
        k = int(got["counts"][n])
        src = got["src"][n, :k].long()
        assert torch.equal(got["boxes"][n, :k].view(torch.int32), sb[n][src].view(torch.int32))
    # the fixture's conditions hold on the kernel's boxes as they do on the float64 decode (tests/test_cascade_train_host.py)
    host = T.relabel(c["pred"], K, c["proposals"], c["counts"], c["image_hw"], T.RELABEL_WEIGHTS, c["gt"], c["gt_classes"], c["counts_g"], T.RELABEL_THRESH)
    for k in ("counts", "src", "gt_classes", "matched_idx"):
        assert np.array_equal(host[k], ref[k]), k
    # the same from run to run: a second call, into fresh buffers, gives the same bits (outputs filled with NaN first: the next test)
    again = ops.roi_cascade_relabel(dev["pred"], K, dev["proposals"], dev["counts"], dev["image_hw"], T.RELABEL_WEIGHTS, dev["gt"], dev["gt_classes"],
                                    dev["counts_g"], T.RELABEL_THRESH)
    assert all(torch.equal(again[k].view(torch.int32), got[k].view(torch.int32)) for k in got)


@pytest.mark.parametrize("K", T.RELABEL_KS)
@pytest.mark.parametrize("case", range(len(T.RELABEL_CASES)))
def test_relabel_writes_every_output_element(ops, case, K):
    """the C entry point on outputs filled with NaN / -7 first, on every case"""
    import ctypes as C
    from afigan_amd import _lib
    c = T.relabel_case(case, K)
    dev = {k: torch.from_numpy(v).cuda() for k, v in c.items() if k != "main"}
    N, B, G = T.RELABEL_N, T.RELABEL_B, T.RELABEL_GMAX
    fb = lambda *s: torch.full(s, NAN, device="cuda")
    ib = lambda *s: torch.full(s, -7, device="cuda", dtype=torch.int32)
    out = {"boxes": fb(N, B, 4), "counts": ib(N), "gt_classes": ib(N, B), "gt_boxes": fb(N, B, 4), "src": ib(N, B), "matched_idx": ib(N, B)}
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.call("afi_roi_cascade_relabel", p(dev["pred"]), dev["pred"].stride(0), N, B, K, p(dev["proposals"]), p(dev["counts"]), p(dev["image_hw"]),
              *T.RELABEL_WEIGHTS, float(np.log(1000.0 / 16)), p(dev["gt"]), p(dev["gt_classes"]), p(dev["counts_g"]), G, T.RELABEL_THRESH,
              p(out["boxes"]), p(out["counts"]), p(out["gt_classes"]), p(out["gt_boxes"]), p(out["src"]), p(out["matched_idx"]), ops.stream_ptr())
    _, sb = ops.roi_cascade_stage(dev["pred"], K, dev["proposals"], dev["counts"], dev["image_hw"], T.RELABEL_WEIGHTS)
    ref = T.relabel_boxes(sb.cpu().numpy(), K, c["counts"], c["gt"], c["gt_classes"], c["counts_g"], T.RELABEL_THRESH)
    for k, v in ref.items():
        assert np.array_equal(out[k].cpu().numpy(), v), k


# ------------------------------------------------------------------------------------------------ list-masked BatchNorm + ReLU
def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _bn_case(N, B, P1, C, counts, family):
    x = T.bn_input(family, N, B, P1, C, counts)
    v = T.valid_rows(counts, B)
    g = _rand(x.shape, 6)
    g[~v] = NAN
    gamma, beta = 1 + 0.5 * _rand((C,), 2), 0.3 * _rand((C,), 3)
    return counts, x, g, v, gamma, beta


@pytest.mark.parametrize("family", T.BN_FAMILIES)
@pytest.mark.parametrize("name", ["mixed", "full", "zero", "clamped"])
@pytest.mark.parametrize("shape", T.BN_SHAPES, ids=str)
def test_masked_bn_relu(ops, shape, name, family):
    _masked_bn_relu(ops, shape, T.bn_counts(shape[0], shape[1])[name], f"{shape} {name} {family}", family)


def test_masked_bn_relu_more_rows_than_blocks(ops):
    """2100 list rows on the apply passes' 2048 blocks (the grid-stride step) and 33 reduction chunks of 64 list rows"""
    _masked_bn_relu(ops, (1, 2100, 1, 4), [1500], "(1, 2100, 1, 4) 1500 unit", "unit")


def _masked_bn_relu(ops, shape, counts, case, family):
    N, B, P1, C = shape
    counts, x, g, v, gamma, beta = _bn_case(N, B, P1, C, counts, family)
    cd = torch.tensor(counts, dtype=torch.int32, device="cuda")
    xd, gd, gad, bed = x.cuda(), g.cuda(), gamma.cuda(), beta.cuda()
    Pn = int(v.sum()) * P1
    # ---- statistics and running buffers: <= 1 ulp
    rm0, rv0 = 0.3 * _rand((C,), 4) + 0.1, 1 + 0.5 * _rand((C,), 5).abs()
    ref = T.masked_stats(x, counts, B, T.BN_EPS, T.BN_MOMENTUM, rm0, rv0)
    rm, rv, nbt = rm0.cuda(), rv0.cuda(), torch.tensor([41], dtype=torch.int64, device="cuda")
    mean, invstd, var = ops.roi_bn_stats(xd, cd, T.BN_EPS, T.BN_MOMENTUM, rm, rv, nbt, want_var=True)
    assert int(nbt) == (42 if Pn else 41)
    us = [_check_ulp("roi_bn_stats " + k, case, t, ref[k]) for k, t in (("mean", mean), ("var", var), ("invstd", invstd), ("running_mean", rm), ("running_var", rv))]
    if Pn == 0:
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and not bool(mean.any())
    m2, i2 = ops.roi_bn_stats(xd, cd, T.BN_EPS, T.BN_MOMENTUM)                        # no buffers, no counter, no variance: the same bits
    assert torch.equal(m2, mean) and torch.equal(i2, invstd)
    if family == "const_channel" and Pn:
        assert float(var[1]) == 0.0 and float(mean[1]) == E.CONST_VALUE
    print(f"[cascade_train] roi_bn_stats             {case:40s} worst {max(us)} ulp")
    mc, ic = mean.cpu(), invstd.cpu()
    # ---- apply: the five-eps form; exact zeros
    for relu in (True, False):
        y = ops.roi_bn_relu_fwd(xd, cd, mean, invstd, gad, bed, relu=relu)
        yref, terms = T.masked_relu_fwd(x, counts, B, mc, ic, gamma, beta, relu)
        yc = y.cpu()
        assert not bool(yc[~v].any()) and bool(torch.isfinite(yc).all())
        if Pn:
            _check_elem("roi_bn_relu_fwd", f"{case} relu {int(relu)}", yc[v], yref[v], terms[v], 4)
            assert not relu or bool((yc >= 0).all())
        if relu:
            ykeep = y
    # ---- backward: the sums (reduction form, Ktot = Pn), dgamma / dbeta accumulate; dx from the kernel's own sums and y (r = 8)
    yk = ykeep.cpu()
    ynan = ykeep.clone()
    ynan[~v.cuda()] = NAN                                                              # padding rows of y are NaN for the backward
    dg0, db0 = _rand((C,), 11) * 3, _rand((C,), 12) * 3
    dg, db = dg0.cuda(), db0.cuda()
    sums = ops.roi_bn_relu_bwd_sums(gd, xd, ynan, cd, mean, invstd, dg, db)
    assert torch.equal(ops.roi_bn_relu_bwd_sums(gd, xd, ynan, cd, mean, invstd), sums)
    s0, s1 = T.masked_bwd_sums(g, x, yk, counts, B, mc, ic)
    if Pn:
        gp = T.masked_gprime(g, yk, counts, B)
        xh32 = (x[v].reshape(-1, C) - mc) * ic
        c0, c1 = gp.sum(0), (gp * xh32).sum(0)                                        # torch CPU fp32
        _check_red("roi_bn_bwd_sums sum g'", case, sums[0], s0, c0, Pn)
        _check_red("roi_bn_bwd_sums sum g' xhat", case, sums[1], s1, c1, Pn)
        _check_red("roi_bn_bwd_sums dbeta +=", case, db, db0.double() + s0, db0 + c0, Pn)
        _check_red("roi_bn_bwd_sums dgamma +=", case, dg, dg0.double() + s1, dg0 + c1, Pn)
    else:
        assert not bool(sums.any()) and torch.equal(dg.cpu(), dg0) and torch.equal(db.cpu(), db0)
    dx = ops.roi_bn_relu_bwd_apply(gd, xd, ynan, cd, mean, invstd, gad, sums).cpu()
    assert not bool(dx[~v].any()) and bool(torch.isfinite(dx).all())
    if Pn:
        sc = sums.cpu()
        dref, terms = T.masked_bwd_dx(g, x, yk, counts, B, mc, ic, gamma, sc[0], sc[1])
        _check_elem("roi_bn_relu_bwd_apply", case, dx[v], dref[v], terms[v], 8)
    gi = gd.clone()                                                                    # in place on g, as the dense pass allows
    import ctypes as C_
    from afigan_amd import _lib
    p = lambda t: C_.c_void_p(t.data_ptr())
    _lib.call("afi_roi_bn_relu_bwd_apply", p(gi), p(xd), p(ynan), p(cd), N, B, P1, C, p(mean), p(invstd), p(gad), p(sums), 1, p(gi), ops.stream_ptr())
    assert torch.equal(gi.cpu(), dx)


@pytest.mark.parametrize("shape", T.BN_SHAPES, ids=str)
def test_masked_bn_with_every_row_valid_is_the_dense_pass(ops, shape):
    """counts = B everywhere: statistics, apply (plain affine) and the backward halves (no ReLU) meet the dense passes' bars against THEIR
    references (elementwise_f64 on the [N B P1, C] matrix), and afi_bn_stats_ex / afi_bn_bwd_sums give the same numbers to <= 1 ulp / the
    reduction bar."""
    N, B, P1, C = shape
    case = f"{shape} dense"
    x2 = E.stats_input("offset_1e4", N * B * P1, C)
    g2 = _rand(x2.shape, 6)
    gamma, beta = 1 + 0.5 * _rand((C,), 2), 0.3 * _rand((C,), 3)
    cd = torch.full((N,), B, dtype=torch.int32, device="cuda")
    xd, gd, gad, bed = x2.cuda().view(N * B, P1, C), g2.cuda().view(N * B, P1, C), gamma.cuda(), beta.cuda()
    P = x2.shape[0]
    rm0, rv0 = 0.3 * _rand((C,), 4) + 0.1, 1 + 0.5 * _rand((C,), 5).abs()
    ref = E.bn_stats(x2, T.BN_EPS, T.BN_MOMENTUM, rm0, rv0)
    rm, rv = rm0.cuda(), rv0.cuda()
    mean, invstd, var = ops.roi_bn_stats(xd, cd, T.BN_EPS, T.BN_MOMENTUM, rm, rv, want_var=True)
    rmd, rvd = rm0.cuda(), rv0.cuda()
    dense = ops.bn_stats_ex(xd.view(P, C), T.BN_EPS, T.BN_MOMENTUM, rmd, rvd, want_var=True)
    for k, t, dn in (("mean", mean, dense[0]), ("invstd", invstd, dense[1]), ("var", var, dense[2]), ("running_mean", rm, rmd), ("running_var", rv, rvd)):
        _check_ulp("roi_bn_stats dense " + k, case, t, ref[k])
        _check_ulp("roi_bn_stats vs afi_bn_stats_ex " + k, case, t, dn.double().cpu())
    mc, ic = mean.cpu(), invstd.cpu()
    y = ops.roi_bn_relu_fwd(xd, cd, mean, invstd, gad, bed, relu=False)
    yref, terms = E.bn_apply(x2, mc, ic, gamma, beta, 1.0)
    _check_elem("roi_bn_relu_fwd dense", case, y.cpu().view(P, C), yref, terms, 4)
    assert torch.equal(y.view(P, C), ops.bn_apply(xd.view(P, C), mean, invstd, gad, bed, slope=1.0))          # afi_bn_affine both: the same bits
    sums = ops.roi_bn_relu_bwd_sums(gd, xd, None, cd, mean, invstd, relu=False)
    s0, s1 = E.bn_bwd_sums(g2, x2, mc, ic)
    xh32 = (x2 - mc) * ic
    _check_red("roi_bn_bwd_sums dense sum g", case, sums[0], s0, g2.sum(0), P)
    _check_red("roi_bn_bwd_sums dense sum g xhat", case, sums[1], s1, (g2 * xh32).sum(0), P)
    sc = sums.cpu()
    dx = ops.roi_bn_relu_bwd_apply(gd, xd, None, cd, mean, invstd, gad, sums, relu=False)
    dref, terms = E.bn_bwd_dx(g2, x2, mc, ic, gamma, sc[0], sc[1], P)
    _check_elem("roi_bn_relu_bwd_apply dense", case, dx.cpu().view(P, C), dref, terms, 8)


# ------------------------------------------------------------------------------------------------ whole heads
import roi_loss_f64 as RL


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


class _Prop:
    def __init__(self, boxes, image_size):
        self.proposal_boxes, self.image_size = boxes, image_size


class _Imgs:
    def __init__(self, sizes):
        self.image_sizes = sizes


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _keys(k):
    return torch.from_numpy(np.ascontiguousarray(k).view(np.int32)).cuda()


def _loss_weights(out):
    return {k: (0.5 if "box_reg" in k else 0.25 if k == "loss_mask" else 1.0) for k in out}


def _run(h, feats, case, keys=True, polys=None, weights=None):
    xs = {f: v.cuda().requires_grad_(True) for f, v in feats.items()}
    h.zero_grad(set_to_none=True)
    props = [_Prop(_dev(case["proposals"][n, :case["counts_p"][n]]), T.HEAD_IMAGE) for n in range(T.HEAD_N)]
    tg = [{"gt_boxes": _dev(case["gts"][n]), "gt_classes": _dev(case["gt_classes"][n])} for n in range(T.HEAD_N)]
    if polys is not None:
        for t, p in zip(tg, polys):
            t["gt_masks"] = p
    out = h.losses(None, xs, props, tg, _keys(case["keys"]) if keys else None)
    sum(w * out[k] for k, w in (weights or _loss_weights(out)).items()).backward()
    torch.cuda.synchronize()
    grads = {f: x.grad for f, x in xs.items()}
    grads.update({k: p.grad for k, p in h.named_parameters()})
    return out, grads, h.last_assignment


@pytest.mark.parametrize("variant", list(T.HEAD_VARIANTS))
def test_whole_heads_against_fp64_autograd(amd, variant):
    """Every stage's assignment EQUALS the checker's (stage 0: roi_loss_f64.assign; stage k: the relabel rule on afi_roi_cascade_stage's boxes
    of stage k - 1's own predictor output).  Per tensor -- the features, every parameter, gamma and beta -- the relative L2 error against
    float64 autograd on the GPU's assignment is <= 4 x torch-CPU-float32 autograd's own deviation; the losses by test_gpu_roi_loss.py's rule.
    The upstream gradients differ (1 for loss_cls, 0.5 for loss_box_reg).  The measured values are recorded in DESIGN 27."""
    ops = amd.ops
    C, norm, S = T.HEAD_VARIANTS[variant]
    K = T.HEAD_K
    h = T.build_train_heads(amd, C, norm, S).cuda().trainable_().train()
    sd = {k: v.detach().cpu().clone() for k, v in h.state_dict().items()}
    feats, case = T.head_features(C), T.head_case()
    out, grads, asg = _run(h, feats, case)
    assert list(out) == [f"loss_{q}_stage{k}" for k in range(S) for q in ("cls", "box_reg")]
    assert all(v.dim() == 0 and v.requires_grad for v in out.values())
    # ---- the assignment
    want = RL.assign(case, K, T.HEAD_BATCH, T.HEAD_FRACTION, T.HEAD_IOUS[0])
    st = asg["stages"]
    assert len(st) == S and all(set(s) == {"boxes", "counts", "gt_classes", "gt_boxes", "src", "matched_idx", "pred"} for s in st)
    for k, w in (("boxes", "boxes"), ("counts", "counts"), ("gt_classes", "cls"), ("gt_boxes", "gboxes")):
        assert np.array_equal(st[0][k].cpu().numpy(), want[w]) and torch.equal(asg[k], st[0][k]), k
    gt, gc, cg = RL.pad_lists([np.zeros((0, 4), np.float32)] * T.HEAD_N, case["gts"], case["gt_classes"])[2:]
    hw = torch.tensor([T.HEAD_IMAGE] * T.HEAD_N, dtype=torch.float32, device="cuda")
    dropped = 0
    for k in range(1, S):
        p = st[k - 1]
        _, sb = ops.roi_cascade_stage(p["pred"], K, p["boxes"], p["counts"], hw, T.HEAD_WEIGHTS[k - 1])
        ref = T.relabel_boxes(sb.cpu().numpy(), K, p["counts"].cpu().numpy(), gt, gc, cg, T.HEAD_IOUS[k])
        for q, v in ref.items():
            assert np.array_equal(st[k][q].cpu().numpy(), v), (k, q)
        dropped += int(p["counts"].sum() - st[k]["counts"].sum())
    for k, s in enumerate(st):
        cls, cn = s["gt_classes"].cpu().numpy(), s["counts"].cpu().numpy()
        for n in range(T.HEAD_N):
            assert (cls[n, :cn[n]] < K).sum() >= 8 and (cls[n, :cn[n]] == K).sum() >= 8, (k, n)
    assert S == 1 or dropped > 0
    # ---- gradients and losses
    names = [k for k, _ in h.named_parameters()]
    assert (f"box_head.{S - 1}.conv2.norm.weight" in names) == (norm == "SyncBN") and all(g is not None for g in grads.values())
    stages = [{q: s[q].cpu().numpy() for q in ("boxes", "counts", "gt_classes", "gt_boxes")} for s in st]

    def ref(dtype):
        xs = [feats[f].to(dtype).requires_grad_(True) for f in T.HEAD_FEATURES]
        ps = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
        for k in names:
            ps[k].requires_grad_(True)
        bufs = {k: v.clone() for k, v in ps.items() if "running_" in k}
        ls = T.torch_cascade_losses(xs, ps, stages, T.HEAD_MIN_LEVEL, T.HEAD_S, 2, K, T.HEAD_WEIGHTS, 0.0, norm, bufs)
        sum(lc + 0.5 * lb for lc, lb in ls).backward()
        g = {f: x.grad for f, x in zip(T.HEAD_FEATURES, xs)}
        g.update({k: ps[k].grad for k in names})
        return [v.item() for pair in ls for v in pair], g, bufs
    l64, g64, b64 = ref(torch.float64)
    l32, g32, b32 = ref(torch.float32)
    rel = lambda a, b: ((a.double().cpu() - b).norm() / b.norm()).item()
    got = [v.item() for v in out.values()]
    print(f"\n[cascade_train] {variant}: losses gpu {got}\n   fp64 {l64}\n   cpu fp32 {l32}")
    bad, worst = [], (0.0, "")
    for k in list(T.HEAD_FEATURES) + names:
        if k in T.HEAD_FEATURES[1:]:                 # every box of a 64 x 80 image pools from p2 (level 3 starts at sqrt(area) 112): no term, exact zeros
            assert (g64[k] is None or not bool(g64[k].any())) and not bool(grads[k].any()), k
            continue
        assert g64[k] is not None and g64[k].norm() > 0, k
        e_gpu, e_cpu = rel(grads[k].contiguous(), g64[k]), rel(g32[k], g64[k])
        print(f"  {k:40s} rel L2: gpu {e_gpu:.3e}   cpu fp32 {e_cpu:.3e}   bar {4 * e_cpu:.3e}")
        assert tuple(grads[k].shape) == tuple(g64[k].shape)
        worst = max(worst, (e_gpu / (4 * e_cpu), k))
        if not e_gpu <= 4 * e_cpu:
            bad.append((k, e_gpu, e_cpu))
    print(f"[cascade_train] {variant}: worst gradient error / bar {worst[0]:.3f} ({worst[1]})")
    _note("whole heads gradient rel-L2", worst[0], f"{variant} {worst[1]}")
    for gv, w64, w32 in zip(got, l64, l32):
        assert abs(gv - w64) <= 4 * max(abs(w32 - w64), 2.0 ** -24 * abs(w64)), (gv, w64, w32)
    assert not bad, bad
    # ---- the running buffers and the counter advanced once per call and stage, to float64's values
    if norm == "SyncBN":
        now = h.state_dict()
        for k in b64:
            e_gpu, e_cpu = rel(now[k], b64[k]), rel(b32[k], b64[k])
            assert e_gpu <= 4 * max(e_cpu, 2.0 ** -24), (k, e_gpu, e_cpu)
            assert not torch.equal(now[k].cpu(), sd[k])
        assert all(int(v) == 1 for k, v in now.items() if k.endswith("num_batches_tracked") and k.startswith("box_head"))
    elif norm == "FrozenBN":
        assert all(torch.equal(v.cpu(), sd[k]) for k, v in h.state_dict().items() if "running_" in k)


def test_normed_mask_head_against_fp64_autograd(amd):
    """Heads with masks=True and ROI_MASK_HEAD.NORM "SyncBN" (mask pooler 14, 16 channels): loss_mask on the foreground prefix of stage 0's
    list and its gradients -- features, convs, gamma, beta, deconv, predictor -- at the 4 x bar; the running buffers advance."""
    import mask_loss_f64 as Q
    C, K = 16, T.HEAD_K
    h = T.build_train_heads(amd, C, "", 1, masks=True, mask_norm="SyncBN").cuda().trainable_(mask_head=True).train()
    sd = {k: v.detach().cpu().clone() for k, v in h.state_dict().items()}
    feats, case = T.head_features(C), T.head_case()
    out, grads, asg = _run(h, feats, case, polys=Q.e2e_polygons(case), weights={"loss_mask": 0.25})
    assert list(out) == ["loss_cls_stage0", "loss_box_reg_stage0", "loss_mask"]
    names = [k for k, _ in h.named_parameters() if k.startswith("mask_head.")]
    assert "mask_head.mask_fcn2.norm.bias" in names and "mask_head.mask_fcn1.bias" not in names
    boxes, cfg, cls, tg = (asg[k].cpu().numpy() for k in ("mask_boxes", "counts_fg", "gt_classes", "mask_targets"))
    assert cfg.tolist() == [12, 12] and 0.05 < tg.mean() < 0.95

    def ref(dtype):
        xs = [feats[f].to(dtype).requires_grad_(True) for f in T.HEAD_FEATURES]
        ps = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
        for k in names:
            ps[k].requires_grad_(True)
        bufs = {k: v.clone() for k, v in ps.items() if "running_" in k}
        loss = T.torch_normed_mask_loss(xs, ps, "SyncBN", T.HEAD_MIN_LEVEL, 14, 2, boxes, cfg, cls, tg, K, bufs)
        (0.25 * loss).backward()
        g = {f: x.grad for f, x in zip(T.HEAD_FEATURES, xs)}
        g.update({k: ps[k].grad for k in names})
        return loss.item(), g, bufs
    l64, g64, b64 = ref(torch.float64)
    l32, g32, b32 = ref(torch.float32)
    rel = lambda a, b: ((a.double().cpu() - b).norm() / b.norm()).item()
    got = out["loss_mask"].item()
    print(f"\n[cascade_train] normed mask head: loss_mask gpu {got:.8g} fp64 {l64:.8g} cpu fp32 {l32:.8g}")
    bad, worst = [], (0.0, "")
    for k in ["p2"] + names:
        e_gpu, e_cpu = rel(grads[k].contiguous(), g64[k]), rel(g32[k], g64[k])
        print(f"  {k:40s} rel L2: gpu {e_gpu:.3e}   cpu fp32 {e_cpu:.3e}   bar {4 * e_cpu:.3e}")
        worst = max(worst, (e_gpu / (4 * e_cpu), k))
        if not e_gpu <= 4 * e_cpu:
            bad.append((k, e_gpu, e_cpu))
    _note("normed mask head gradient rel-L2", worst[0], worst[1])
    assert abs(got - l64) <= 4 * max(abs(l32 - l64), 2.0 ** -24 * abs(l64))
    assert not bad, bad
    now = h.state_dict()
    for k in b64:
        if k.startswith("mask_head."):
            assert rel(now[k], b64[k]) <= 4 * max(rel(b32[k], b64[k]), 2.0 ** -24) and not torch.equal(now[k].cpu(), sd[k]), k
    assert all(int(v) == 1 for k, v in now.items() if k.endswith("num_batches_tracked") and k.startswith("mask_head"))


def test_training_forward_determinism_frozen_parameters_and_refusals(amd, monkeypatch):
    C, norm, S = T.HEAD_VARIANTS["c8_syncbn"]
    feats, case = T.head_features(C), T.head_case()
    h = T.build_train_heads(amd, C, norm, S).cuda()
    xs = {f: v.cuda() for f, v in feats.items()}
    props = [_Prop(_dev(case["proposals"][n, :case["counts_p"][n]]), T.HEAD_IMAGE) for n in range(T.HEAD_N)]
    tg = [{"gt_boxes": _dev(case["gts"][n]), "gt_classes": _dev(case["gt_classes"][n])} for n in range(T.HEAD_N)]
    with pytest.raises(amd.AfiError, match="cascade training is out of scope"):      # never enabled: the refusal of before
        h.losses(None, xs, props, tg)
    state = {k: v.clone() for k, v in h.state_dict().items()}
    h.trainable_().train()
    runs = []
    cx = amd._lib.current_ctx()
    prev = cx.get_option("deterministic")
    cx.set_option("deterministic", 1)
    try:
        for poison in (False, False, True):
            h.load_state_dict(state)                                                   # the running buffers back to where they were
            if poison:
                monkeypatch.setattr(amd.ops, "_POISON", True)
            runs.append(_run(h, feats, case))
    finally:
        cx.set_option("deterministic", prev)
        monkeypatch.setattr(amd.ops, "_POISON", False)
    (o1, g1, a1) = runs[0]
    for o, g, a in runs[1:]:
        assert all(torch.equal(o1[k], o[k]) for k in o1) and all(torch.equal(g1[k], g[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g[k])]
        assert all(torch.equal(s1[q], s[q]) for s1, s in zip(a1["stages"], a["stages"]) for q in ("boxes", "counts", "gt_classes", "pred"))
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())
    # forward in training mode: stage 0's sampled proposals with their labels, and the same losses
    h.load_state_dict(state)
    sampled, losses = h(_Imgs([T.HEAD_IMAGE] * T.HEAD_N), xs, props, tg, keys=_keys(case["keys"]))
    want = RL.assign(case, T.HEAD_K, T.HEAD_BATCH, T.HEAD_FRACTION, T.HEAD_IOUS[0])
    assert set(losses) == set(o1) and all(torch.equal(losses[k], o1[k]) for k in o1)
    for n, s in enumerate(sampled):
        c = want["counts"][n]
        assert len(s) == c and np.array_equal(s.proposal_boxes.tensor.cpu().numpy(), want["boxes"][n, :c])
        assert s.gt_classes.dtype == torch.int64 and np.array_equal(s.gt_classes.cpu().numpy(), want["cls"][n, :c])
    # eval mode with targets under BN: refused in words; frozen parameters: no gradient, the features still get theirs
    with pytest.raises(amd.AfiError, match=r"call \.train\(\)"):
        h.eval().losses(None, xs, props, tg)
    h.train().trainable_(False)
    _, g, _ = _run(h, feats, case)
    assert all(g[k] is None for k, _ in h.named_parameters()) and all(g[f] is not None for f in T.HEAD_FEATURES) and bool(g["p2"].abs().sum() > 0)
    with pytest.raises(amd.AfiError, match="image_sizes"):
        h.losses_padded(xs, torch.zeros(2, 4, 4, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, 1, 4, device="cuda"),
                        torch.zeros(2, 1, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"))


class _Pyramid(torch.nn.Module):
    """A small torch conv pyramid with the backbone's contract: p2 .. p5 at strides 4 .. 32."""
    size_divisibility = 32

    def __init__(self, channels=8):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, channels, 4, stride=4)
        self.down = torch.nn.ModuleList([torch.nn.Conv2d(channels, channels, 3, stride=2, padding=1) for _ in range(3)])
        self.channels = channels

    def output_shape(self):
        from afigan_amd.fpn_sr import ShapeSpec
        return {f: ShapeSpec(channels=self.channels, stride=2 ** int(f[1:])) for f in T.HEAD_FEATURES}

    def forward(self, x):
        out = {"p2": torch.tanh(self.stem(x))}
        for a, b, conv in zip(T.HEAD_FEATURES, T.HEAD_FEATURES[1:], self.down):
            out[b] = torch.tanh(conv(out[a]))
        return out


def test_detector_with_cascade_heads_trains_two_steps(amd):
    """A GeneralizedRCNN with Cascade heads returns the RPN's two losses plus the 2 S stage losses; two DetectorStep.run_step calls at a base
    rate of 1e-6 stay finite, the norms' affine sits in the WEIGHT_DECAY_NORM group, and after each step the heads' prepared weights equal
    those of a freshly built module with the same state dict."""
    torch.manual_seed(0)
    C, norm, S = T.HEAD_VARIANTS["c8_syncbn"]
    backbone = _Pyramid(C).cuda()
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[16], [32], [64], [128]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": list(T.HEAD_FEATURES), "PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 50, "PRE_NMS_TOPK_TRAIN": 200,
                                       "POST_NMS_TOPK_TRAIN": 50, "BATCH_SIZE_PER_IMAGE": 32}})
    rpn = amd.RPN(cfg, backbone.output_shape()).cuda().trainable_()
    new_heads = lambda: T.build_train_heads(amd, C, norm, S).cuda().trainable_()
    heads = new_heads()
    model = amd.GeneralizedRCNN(backbone=backbone, proposal_generator=rpn, roi_heads=heads, pixel_mean=[0.0, 0.0, 0.0], pixel_std=[1.0, 1.0, 1.0],
                                device="cuda").train()
    case = T.head_case()
    g = torch.Generator().manual_seed(4)
    batch = []
    for n in range(T.HEAD_N):
        tg = type("GT", (), {})()
        tg.gt_boxes, tg.gt_classes = _dev(case["gts"][n]), _dev(case["gt_classes"][n].astype(np.int64))
        batch.append({"image": torch.randn((3,) + tuple(T.HEAD_IMAGE), generator=g), "targets": tg})
    losses = model(batch)
    losses = losses[0] if isinstance(losses, tuple) else losses
    assert set(losses) == {"loss_rpn_cls", "loss_rpn_loc"} | {f"loss_{q}_stage{k}" for k in range(S) for q in ("cls", "box_reg")}
    opt = amd.DetectorOptim(list(model.named_parameters()), modules=list(model.modules()), base_lr=1e-6, momentum=0.9, weight_decay=1e-3,
                            weight_decay_norm=0.0, bias_lr_factor=2.0, weight_decay_bias=0.0, lr_steps=(5,), lr_gamma=0.1, warmup_factor=0.5, warmup_iters=2)
    by_name = dict(zip(opt.names, opt.groups))                                        # (lr, weight decay) per parameter
    affine = [n for n in opt.names if ".box_head." in n and n.endswith(("norm.weight", "norm.bias"))]
    assert len(affine) == 2 * 2 * S and all(by_name[n] == (1e-6, 0.0) for n in affine)                       # WEIGHT_DECAY_NORM 0, no bias rate
    one = lambda tail: [v for n, v in by_name.items() if n.endswith(tail)]
    assert one("box_head.0.conv1.weight") == [(1e-6, 1e-3)] and one("box_head.0.fc1.bias") == [(2e-6, 0.0)]
    step = amd.DetectorStep(model, opt)
    before = {k: v.detach().clone() for k, v in heads.named_parameters()}
    for _ in range(2):
        rec = step.run_step(batch)
        assert all(np.isfinite(v) for v in rec.values()), rec
        fresh = new_heads()
        fresh.load_state_dict(heads.state_dict())
        for k in range(S):
            a, b = heads._prepare(k), fresh._prepare(k)
            assert all(torch.equal(x, y) for x, y in zip([t for wb in a[0] for t in wb] + list(a[1]), [t for wb in b[0] for t in wb] + list(b[1])))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    moved = [k for k, v in heads.named_parameters() if not torch.equal(v, before[k])]
    assert any(k.endswith("norm.weight") for k in moved) and any(k.endswith("conv1.weight") for k in moved) and any("bbox_pred" in k for k in moved)
