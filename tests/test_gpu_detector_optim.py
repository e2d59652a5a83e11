"""The detector's optimiser step on the GPU (afigan_amd/detector_optim.py, csrc/detector_optim.hip):
  1. afi_detector_sgd_step against the fp64 restatement (tests/detector_optim_f64.py) at the bounds the count of roundings gives;
  2. its FrozenBN fold, bit-equal to frozen.fold_conv of the updated parameter;
  3. DetectorOptim / DetectorStep / GeneralizedRCNN on the small detector of test_gpu_resnet_train.py: no refold, no stale cache, the
     three-step trajectory against fp64;
  4. Stage2Step with a DetectorOptim, the state dict, the scheduler check."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import detector_optim_f64 as F  # noqa: E402

SENT = -7.25                       # what surrounds every buffer of tests 1 and 2
MOM, GSCALE = 0.9, 0.5
KW = dict(base_lr=0.05, momentum=MOM, weight_decay=1e-2, weight_decay_norm=0.0, bias_lr_factor=2.0, weight_decay_bias=5e-3,
          lr_steps=(1,), lr_gamma=0.5, warmup_factor=0.25, warmup_iters=1)


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    assert torch.cuda.is_available()
    return afigan_amd


def _fenced(vals, front=4):
    """(whole buffer, the view holding `vals`): `front` sentinels before it (4: the view is 16-byte aligned; 5: it is not) and 4 after."""
    n = vals.numel()
    whole = torch.full((front + n + 4,), SENT, device="cuda")
    whole[front:front + n] = vals.reshape(-1).cuda()
    return whole, whole[front:front + n].view(vals.shape)


def _fence_ok(whole, front, n):
    return bool((whole[:front] == SENT).all()) and bool((whole[front + n:] == SENT).all())


# ------------------------------------------------------------------------------------------------ 1. the kernel against the restatement
#        name                  n        front (5: starts at element 1 of a 16-byte line)
PLAIN = [("a.weight", 1, 4), ("b.bias", 3, 4), ("c.norm.weight", 5, 4), ("d.weight", 4099, 4), ("e.weight", 600001, 4), ("f.bias", 0, 4),
         ("g.weight", 37, 5), ("h.norm.bias", 1030, 5), ("idle.weight", 9, 4),
         ("i.weight", 2200003, 4), ("j.bias", 2100001, 5)]  # 538 and 513 units of 4096: the 512 blocks of the per-tensor grid sweep twice
_RUNS = {}


def _plain_run(amd, flat):
    """Two steps of a DetectorOptim over PLAIN (step 1 from m = 0); everything the checks need, on the CPU.  Computed once per grid."""
    if flat in _RUNS:
        return _RUNS[flat]
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(n, generator=g) for _, n, _ in PLAIN]
    grads = [[torch.randn(n, generator=g) * 3 for _, n, _ in PLAIN] for _ in range(2)]
    fenced = [_fenced(v, front) for v, (_, _, front) in zip(init, PLAIN)]
    params = [torch.nn.Parameter(view) for _, view in fenced]
    opt = amd.DetectorOptim([(name, p) for (name, _, _), p in zip(PLAIN, params)], **KW)
    opt.FLAT_GRID = flat
    pad = torch.ones_like(opt.flat_mom, dtype=torch.bool)                      # the momentum buffer's fences: the padding between segments
    for i, p in enumerate(opt.params):
        pad[opt._offs[i]:opt._offs[i] + p.numel()] = False
    opt.flat_mom[pad] = SENT
    out = {"init": init, "grads": grads, "steps": [], "lrs": [], "opt": opt}
    for step in range(2):
        gf = [_fenced(v, front) for v, (_, _, front) in zip(grads[step], PLAIN)]
        for (name, _, _), p, (_, gv) in zip(PLAIN, params, gf):
            p.grad = None if name.startswith("idle") else gv
        before = [p._version for p in params]
        out["lrs"].append(opt.group_lrs())
        opt.step(gscale=GSCALE)
        torch.cuda.synchronize()
        out["steps"].append({"p": [p.detach().cpu().clone() for p in params], "m": [opt._logical(i).cpu().clone() for i in range(len(params))],
                             "bumped": [p._version > v for p, v in zip(params, before)],
                             "fences": all(_fence_ok(w, front, n) for (w, _), (_, n, front) in zip(fenced, PLAIN))
                             and all(_fence_ok(w, front, n) for (w, _), (_, n, front) in zip(gf, PLAIN)) and bool((opt.flat_mom[pad] == SENT).all()),
                             "grads_kept": all(torch.equal(gv.cpu(), v) for (_, gv), v in zip(gf, grads[step]))})
    _RUNS[flat] = out
    return out


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("flat", [True, False])
def test_kernel_against_the_fp64_restatement(amd, flat, poison, monkeypatch):
    """|m - m64| <= 4u M and |p - p64| <= 2u (|p0| + lr |m64|) + 4u lr M per step (detector_optim_f64.bounds), each step restated from the
    kernel's own fp32 state before it.  Worst observed ratio to the bound on an MI355X: 0.477 (m), 0.497 (p), either grid."""
    if poison:
        monkeypatch.setattr(amd.ops, "_POISON", True)
        _RUNS.pop(flat, None)
    r = _plain_run(amd, flat)
    assert r["opt"].relayouts == 0 and r["opt"].iter == 2
    assert r["lrs"][0] != r["lrs"][1] and len({(lr, wd) for lr, (_, wd) in zip(r["lrs"][0], r["opt"].groups)}) == 3      # three distinct groups, a moving schedule
    worst_m = worst_p = 0.0
    for step in range(2):
        s = r["steps"][step]
        assert s["fences"] and s["grads_kept"]
        for i, (name, n, _) in enumerate(PLAIN):
            p0 = r["init"][i] if step == 0 else r["steps"][0]["p"][i]
            m0 = None if step == 0 else r["steps"][0]["m"][i]
            if name.startswith("idle") or n == 0:
                assert torch.equal(s["p"][i], r["init"][i]) and not bool(s["m"][i].any()) and (n == 0 or not s["bumped"][i]), name
                continue
            assert s["bumped"][i], name
            p64, m64, M = F.sgd(p0, r["grads"][step][i], m0, r["lrs"][step][i], r["opt"].groups[i][1], MOM, GSCALE)
            bm, bp = F.bounds(p0, m64, r["lrs"][step][i], M)
            em, ep = (s["m"][i].double() - m64).abs(), (s["p"][i].double() - p64).abs()
            worst_m, worst_p = max(worst_m, float((em / bm).max())), max(worst_p, float((ep / bp).max()))
            assert bool((em <= bm).all()) and bool((ep <= bp).all()), (name, step, float((em / bm).max()), float((ep / bp).max()))
    print(f"[detector_sgd flat={flat}] worst error / bound: m {worst_m:.3f}, p {worst_p:.3f}")
    assert worst_p > 0                                                          # (fp32 arithmetic did run: the bound is not met by an fp64 copy)


def test_two_runs_and_the_two_grids_are_bit_identical(amd):
    a = _plain_run(amd, True)
    _RUNS.pop(True)
    b, c = _plain_run(amd, True), _plain_run(amd, False)
    for other in (b, c):
        for s, t in zip(a["steps"], other["steps"]):
            assert all(torch.equal(x, y) for x, y in zip(s["p"], t["p"])) and all(torch.equal(x, y) for x, y in zip(s["m"], t["m"]))


# ------------------------------------------------------------------------------------------------ 2. the fold
# (k, O, I, front of p / g / m, front of fold_out); 4: 16-byte aligned, 5: not.  In table order: the two large k = 3 entries come first
# and hold 640 + 1920 = 2560 units, so on the flat grid (2048 blocks) everything behind them is reached in a block's second sweep, and on
# the per-tensor grid (512 blocks) their own blocks sweep twice and four times over one LDS tile.
FOLDS = [(3, 512, 160, 4, 4), (3, 512, 480, 4, 4),
         (1, 8, 12, 4, 4), (1, 64, 256, 4, 4),                                 # k = 1: float4s that span two rows; whole rows
         (3, 8, 12, 4, 4), (3, 4, 80, 4, 4), (3, 128, 64, 4, 4),               # k = 3: a chunk tail, more than one 32-channel chunk, full lines
         (1, 6, 3, 4, 4), (1, 8, 12, 4, 5), (3, 5, 7, 5, 5), (3, 3, 64, 5, 4)]  # the scalar branches: I < 4, an unaligned fold_out, I % 4 != 0 and
                                                                               # unaligned p / g / m, unaligned p / g / m under full 128-byte rows


def _fold_convs(amd, seed):
    """(conv, the fenced buffer its weight lives in) per FOLDS entry."""
    from afigan_amd import frozen
    g = torch.Generator().manual_seed(seed)
    convs = []
    for k, O, I, front, _ in FOLDS:
        c = frozen.Conv2d(I, O, k, bias=True, norm=True)
        with torch.no_grad():
            c.bias.copy_(torch.randn(O, generator=g))
            c.norm.weight.copy_(torch.randn(O, generator=g))
            c.norm.weight[0] = -1.5                                            # a negative gamma
            c.norm.bias.copy_(torch.randn(O, generator=g))
            c.norm.running_mean.copy_(torch.randn(O, generator=g))
            c.norm.running_var.copy_(torch.rand(O, generator=g) + 0.1)
            c.norm.running_var[1] = 1e-12                                      # a tiny variance: s = gamma / sqrt(var + eps) near 316 gamma
        c = c.cuda()
        whole, view = _fenced(torch.randn(c.weight.shape, generator=g), front)
        c.weight = torch.nn.Parameter(view, requires_grad=False)
        convs.append((c, whole))
    return convs


@pytest.mark.parametrize("flat", [True, False])
def test_fold_is_fold_conv_of_the_updated_parameter(amd, flat):
    from afigan_amd import _lib
    units = [amd.ops.detector_sgd_units(O * I * k * k, O, I, k, True) for k, O, I, _, _ in FOLDS]
    assert units[0] > 512 and units[1] > 3 * 512 and units[0] + units[1] > 2048 and sum(units) < 2 * 2048      # what the order above claims
    convs = _fold_convs(amd, 9)
    g = torch.Generator().manual_seed(10)
    table = (_lib.DetSgdDesc * len(convs))()
    keep, lr, wd = [], 0.1, 1e-2
    for d, (c, pw), (k, O, I, front, ffront) in zip(table, convs, FOLDS):
        n = O * I * k * k
        p0 = c.weight.detach().cpu().clone()
        grad, m0 = torch.randn(c.weight.shape, generator=g), torch.randn(c.weight.shape, generator=g)
        gw, gv = _fenced(grad, front)
        mw, mv = _fenced(m0, front)
        fw, fv = _fenced(torch.zeros(n), ffront)
        assert all((t.data_ptr() % 16 == 0) == (f == 4) for t, f in ((c.weight, front), (gv, front), (mv, front), (fv, ffront)))
        s64 = (c.norm.weight.double() * torch.rsqrt(c.norm.running_var.double() + c.norm.eps)).contiguous()
        d.p, d.g, d.m, d.n, d.lr, d.wd = c.weight.data_ptr(), gv.data_ptr(), mv.data_ptr(), n, lr, wd
        d.fold_out, d.s64, d.O, d.I, d.k = fv.data_ptr(), s64.data_ptr(), O, I, k
        bias_before = (c.bias.detach().clone(), c.fold()[1].clone())
        keep.append((p0, grad, m0, gw, gv, mw, mv, fw, fv, s64, bias_before))
    amd.ops.detector_sgd_step(table, torch.device("cuda"), MOM, GSCALE, flat=flat)
    torch.cuda.synchronize()
    for (c, pw), (k, O, I, front, ffront), (p0, grad, m0, gw, gv, mw, mv, fw, fv, s64, bias_before) in zip(convs, FOLDS, keep):
        n, case = O * I * k * k, (k, O, I, front, ffront)
        assert _fence_ok(pw, front, n) and _fence_ok(gw, front, n) and _fence_ok(mw, front, n) and _fence_ok(fw, ffront, n), case
        assert torch.equal(gv.cpu(), grad), case
        p64, m64, M = F.sgd(p0, grad, m0, lr, wd, MOM, GSCALE)
        bm, bp = F.bounds(p0, m64, lr, M)
        assert bool(((mv.cpu().double() - m64).abs() <= bm).all()) and bool(((c.weight.detach().cpu().double() - p64).abs() <= bp).all()), case
        w, b = c.fold()                                                        # fold_conv of the kernel's own updated parameter
        mine = fv.view(O, I) if k == 1 else fv.view(O, 3, 3, I).permute(0, 3, 1, 2)
        assert mine.stride() == w.stride() and torch.equal(mine, w), (case, int((mine != w).sum()))
        assert torch.equal(c.bias.detach(), bias_before[0]) and torch.equal(b, bias_before[1]), case


# ------------------------------------------------------------------------------------------------ 3. DetectorOptim on the small detector
def _detector(amd):
    import mask_loss_f64 as Q
    import resnet_train_f64 as R
    features = ["p2", "p3", "p4", "p5"]
    net, freeze_at, _ = R.make_net("small")
    backbone = amd.FPN_AFIGAN(bottom_up=net.trainable_(freeze_at), in_features=["res2", "res3", "res4", "res5"], out_channels=16, norm="",
                              top_block=amd.LastLevelMaxPool(), fuse_type="sum").cuda()
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[16], [32], [64], [128]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": features, "PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 50, "PRE_NMS_TOPK_TRAIN": 200,
                                       "POST_NMS_TOPK_TRAIN": 50, "BATCH_SIZE_PER_IMAGE": 32}})
    shapes = {f: backbone.output_shape()[f] for f in features}
    new_rpn = lambda: amd.RPN(cfg, shapes).cuda().trainable_()
    new_heads = lambda: Q.e2e_heads(amd, 16).cuda().trainable_(mask_head=True)
    model = amd.GeneralizedRCNN(backbone=backbone, proposal_generator=new_rpn(), roi_heads=new_heads(), pixel_mean=[0.0, 0.0, 0.0],
                                pixel_std=[1.0, 1.0, 1.0], device="cuda").train()
    ih, iw = 64, 80
    gts = [np.array([[4, 6, 40, 50], [30, 20, 76, 60], [10, 30, 30, 44]], np.float32), np.array([[8, 8, 60, 40], [40, 34, 70, 62]], np.float32)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g = torch.Generator().manual_seed(4)
    batch = []
    for b in gts:
        polys = [[Q._ngon((x0 + x1) / 2, (y0 + y1) / 2, 0.45 * (x1 - x0), 0.45 * (y1 - y0), 9)] for x0, y0, x1, y1 in b.astype(np.float64)]
        tg = type("GT", (), {})()
        tg.gt_boxes, tg.gt_classes = dev(b), dev(np.arange(len(b), dtype=np.int64) % 5)
        tg.gt_masks = type("PolygonMasks", (), {"polygons": polys})()
        batch.append({"image": torch.randn((3, ih, iw), generator=g), "targets": tg})
    return model, net, batch, new_rpn, new_heads


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b)
    return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


# (the small detector's weights are random draws: its losses start in the hundreds and a rate of 1e-3 already diverges, under torch.optim.SGD too)
DET_KW = dict(base_lr=1e-6, momentum=0.9, weight_decay=1e-3, weight_decay_norm=0.0, bias_lr_factor=2.0, weight_decay_bias=0.0,
              lr_steps=(2,), lr_gamma=0.1, warmup_factor=0.5, warmup_iters=2)


@pytest.fixture(scope="module")
def trained(amd):
    """Three DetectorStep.run_step calls on the small detector; after every step() the checks that need the state of that moment."""
    from afigan_amd import frozen
    model, net, batch, new_rpn, new_heads = _detector(amd)
    init = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    opt = amd.DetectorOptim(list(model.named_parameters()), modules=list(model.modules()), **DET_KW)
    rec = {"model": model, "net": net, "opt": opt, "batch": batch, "init": init, "grads": [], "lrs": [], "losses": [], "after_step": []}
    inner = opt.step

    def step():
        rec["grads"].append({n: (None if p.grad is None else p.grad.detach().cpu().clone()) for n, p in zip(opt.names, opt.params)})
        rec["lrs"].append(opt.group_lrs())
        before = net._prepare() if rec["after_step"] else None                 # (the first forward built it)
        inner()
        calls = []
        real = frozen.fold_conv
        frozen.fold_conv = lambda *a, **k: (calls.append(1), real(*a, **k))[1]   # Conv2d.fold goes through it too
        try:
            d = net._prepare()
        finally:
            frozen.fold_conv = real
        fresh_ok = all(_same(d[id(c)], c.fold()) and d[id(c)][0].stride() == c.fold()[0].stride() for c in net._own_convs())
        rpn2, heads2 = new_rpn(), new_heads()
        rpn2.load_state_dict(model.proposal_generator.state_dict())
        heads2.load_state_dict(model.roi_heads.state_dict())
        rec["after_step"].append({
            "same_dict": before is None or d is before, "fold_calls": len(calls), "fresh_ok": fresh_ok,
            "rpn_ok": _same(model.proposal_generator._prepare(), rpn2._prepare()),
            "heads_ok": _same(model.roi_heads._prepare(), heads2._prepare()) and _same(model.roi_heads._prepare_mask(), heads2._prepare_mask())})
    opt.step = step
    runner = amd.DetectorStep(model, opt)
    for _ in range(3):
        rec["losses"].append(runner.run_step(batch))
    torch.cuda.synchronize()
    return rec


def test_generalized_rcnn_returns_the_five_losses(amd, trained):
    for losses in trained["losses"]:
        assert set(losses) == {"loss_cls", "loss_box_reg", "loss_mask", "loss_rpn_cls", "loss_rpn_loc"}
        assert all(isinstance(v, float) and np.isfinite(v) for v in losses.values())
    assert "GeneralizedRCNN" in amd.META_ARCH_REGISTRY or amd.registry.USING_DETECTRON2_REGISTRY
    assert trained["losses"][0] != trained["losses"][2]                         # the weights moved


def test_step_leaves_the_prepared_weights_current(trained):
    """After each step() the bottom-up's _prepare() is a cache hit (the same dict, no fold_conv call) whose every entry is bit-equal to a
    fresh conv.fold(); the RPN's and the heads' prepared weights are those of freshly built modules with the same state dict."""
    assert len(trained["after_step"]) == 3 and trained["opt"].relayouts == 0
    for i, s in enumerate(trained["after_step"]):
        assert s["same_dict"] and s["fold_calls"] == 0 and s["fresh_ok"] and s["rpn_ok"] and s["heads_ok"], (i, s)
    assert len(trained["opt"].modules) == 1 and len(trained["net"].fold_slots()) == len(trained["net"]._train_convs()) > 0


def test_three_steps_against_the_fp64_trajectory(trained):
    """Parameters and momentum after three steps against detector_optim_f64.trajectory driven by the gradients each step() saw: test 1's
    bound accumulated per step (observed on an MI355X: 0.48 of it).  Frozen parameters: unchanged bit for bit, no momentum entry."""
    opt, model = trained["opt"], trained["model"]
    mom = opt.state_dict()["optimizer"]["momentum_buffer"]
    now = {n: p.detach().cpu() for n, p in model.named_parameters()}
    frozen_names = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert frozen_names and all(torch.equal(now[n], trained["init"][n]) and n not in mom for n in frozen_names)
    assert list(mom) == opt.names and len(opt.names) + len(frozen_names) == len(now)
    worst, moved = 0.0, 0
    for i, n in enumerate(opt.names):
        grads = [g[n] for g in trained["grads"]]
        assert all(g is not None for g in grads), n
        p64, m64, ep, em = F.trajectory(trained["init"][n], grads, [lrs[i] for lrs in trained["lrs"]], opt.groups[i][1], DET_KW["momentum"])
        dp, dm = (now[n].double() - p64).abs(), (mom[n].cpu().double() - m64).abs()
        ok = ep > 0
        worst = max(worst, float((dp[ok] / ep[ok]).max()) if bool(ok.any()) else 0.0)
        assert bool((dp <= ep).all()) and bool((dm <= em).all()), (n, float((dp - ep).max()), float((dm - em).max()))
        assert bool(mom[n].any()), n
        moved += int(not torch.equal(now[n], trained["init"][n]))
    assert moved >= 0.9 * len(opt.names), (moved, len(opt.names))                 # (an update below half an ulp of every element leaves a tensor as it was)
    print(f"[detector_optim] three steps: worst parameter error / accumulated bound {worst:.3f}")


def test_step_between_forward_and_backward_is_refused(trained):
    """The version bumps keep torch's saved-tensor check alive: a step() after a forward invalidates that forward's graph."""
    model, opt = trained["model"], trained["opt"]
    losses = model(trained["batch"])
    type(opt).step(opt)                                                         # (the gradients of the third step are still there)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        sum(losses.values()).backward()


# ------------------------------------------------------------------------------------------------ 4. trainers and state
class _TinyBottomUp(torch.nn.Module):
    """test_gpu_stage2.py's stand-in bottom-up: average pooling to strides 4..32 and a 1x1 conv per level (plain torch ops)."""

    def __init__(self, chans=(8, 12, 16, 20)):
        super().__init__()
        self.chans = chans
        self.proj = torch.nn.ModuleList([torch.nn.Conv2d(3, c, 1) for c in chans])

    def output_shape(self):
        from afigan_amd.fpn_sr import ShapeSpec
        return {f"res{i + 2}": ShapeSpec(c, 4 * 2 ** i) for i, c in enumerate(self.chans)}

    def forward(self, x):
        return {f"res{i + 2}": p(torch.nn.functional.avg_pool2d(x, 4 * 2 ** i)) for i, p in enumerate(self.proj)}


class _FakeRPN(torch.nn.Module):
    def forward(self, images, features, gt):
        return [None] * len(images), {"loss_rpn_cls": 0.1 * features["p3"].square().mean(), "loss_rpn_loc": 0.05 * features["p6"].abs().mean()}


class _FakeHeads(torch.nn.Module):
    def forward(self, images, features, proposals, gt):
        return None, {"loss_cls": 0.2 * features["p2"].square().mean(), "loss_box_reg": 0.1 * features["p4"].abs().mean()}


def _stage2_models(amd, C_, seed):
    from oracle import afigan_oracle as orc
    torch.manual_seed(seed)

    def fpn():
        f = amd.FPN_AFIGAN(_TinyBottomUp(), ["res2", "res3", "res4", "res5"], C_, top_block=amd.LastLevelMaxPool())
        f.srf_module.load_state_dict(orc.closed_form_generator_params(C_, 3, 32))
        return f
    det = amd.GeneralizedRCNN_AFExtractor(backbone=fpn(), proposal_generator=_FakeRPN(), roi_heads=_FakeHeads(),
                                          pixel_mean=[0.4, 0.5, 0.6], pixel_std=[1.0, 1.1, 0.9], device="cuda")

    class Cfg:
        class MODEL:
            DEVICE, PIXEL_MEAN, PIXEL_STD = "cuda", [0.4, 0.5, 0.6], [1.0, 1.1, 0.9]

            class GUIDE_BACKBONE:
                NAME = "_test_detector_optim_guide_backbone"

        class INPUT:
            FORMAT = "BGR"
    guide_fpn = fpn()
    if Cfg.MODEL.GUIDE_BACKBONE.NAME not in amd.BACKBONE_REGISTRY:
        def _test_detector_optim_guide_backbone(cfg, shape):
            return _stage2_models.guide_fpn
        amd.BACKBONE_REGISTRY.register(_test_detector_optim_guide_backbone)
    _stage2_models.guide_fpn = guide_fpn
    guide = amd.RCNN_FPN_only(Cfg).eval()
    D = amd.Discriminator(in_filters=C_).cuda()
    D.load_state_dict(orc.closed_form_discriminator_params(C_))
    return det, guide, D


def test_stage2_step_with_a_detector_optim(amd):
    """Stage2Step(optimizer=DetectorOptim) beside the same step with torch.optim.SGD over identical groups, two iterations each.
    Iteration 1: its losses are computed before the detector's first update, so the optimiser cannot move them; the bar only says that the
    two runs are the same computation.  The update: both optimisers sit within one step's bound (test 1) of the fp64 update of the same
    gradients, so they differ by at most twice that bound.  Iteration 2 is where the optimiser shows in the losses: the four detector losses
    are functions of the updated parameters alone (D feeds the detector no gradient: the adversarial term is detached, the content term does
    not read D), held to test_gpu_stage2.py's bar for these losses computed twice on the kernels, 1e-5 relative + 1e-7; the D- and G-side
    terms also carry D's own update and get that file's 1e-3.  The update must be visible at a hundred times the bar, or the comparison says
    nothing.  Observed on an MI355X: iteration-1 gap 1.1e-7 relative, parameters bit-identical to torch's, iteration-2
    detector losses equal after a move of 0.44 of their sum."""
    kw = dict(base_lr=0.05, momentum=0.9, weight_decay=1e-3, weight_decay_norm=0.0, bias_lr_factor=2.0, weight_decay_bias=0.0)
    det, guide, D = _stage2_models(amd, 32, 3)
    det2, D2 = copy.deepcopy(det), copy.deepcopy(D)
    gen = torch.Generator().manual_seed(21)
    data = [{"image": torch.rand((3, 128, 192), generator=gen), "image_x0.5": torch.rand((3, 64, 96), generator=gen)},
            {"image": torch.rand((3, 120, 180), generator=gen), "image_x0.5": torch.rand((3, 60, 90), generator=gen)}]
    opt = amd.DetectorOptim(list(det.named_parameters()), warmup_iters=0, lr_steps=(), **kw)
    init = [p.detach().clone() for p in opt.params]
    grads = []
    inner = opt.step
    opt.step = lambda: (grads.extend(p.grad.detach().clone() for p in opt.params), inner())[1]
    step = amd.Stage2Step(det.train(), guide, D, opt, base_lr=0.01, warmup_iters=0, lr_steps=())
    step.adv.set_option("deterministic", 1)
    out = step.run_step(data)
    assert opt.iter == 1 and opt.relayouts == 0 and len(grads) == len(opt.params) > 20

    named2 = [(n, p) for n, p in det2.named_parameters() if p.requires_grad]
    assert [n for n, _ in named2] == opt.names
    groups = [{"params": [p], "lr": F.f32(lr), "weight_decay": F.f32(wd)} for (_, p), (lr, wd) in zip(named2, opt.groups)]
    opt2 = torch.optim.SGD(groups, lr=kw["base_lr"], momentum=F.f32(kw["momentum"]))
    step2 = amd.Stage2Step(det2.train(), guide, D2, opt2, base_lr=0.01, warmup_iters=0, lr_steps=())
    step2.adv.set_option("deterministic", 1)
    out2 = step2.run_step(data)
    assert set(out) == set(out2) and len(out) == 14
    gap = max(abs(out[k] - out2[k]) / (abs(out2[k]) + 1e-30) for k in out)
    assert gap <= 1e-5, {k: (out[k], out2[k]) for k in out}
    after = [p.detach().clone() for p in opt.params]                            # (the update of iteration 1, checked below)
    nxt, nxt2 = step.run_step(data), step2.run_step(data)
    det_keys = ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc")
    for k in nxt:
        bar = 1e-5 * abs(nxt2[k]) + 1e-7 if k in det_keys else 1e-3 * abs(nxt2[k])
        assert abs(nxt[k] - nxt2[k]) <= bar, (k, nxt[k], nxt2[k])
    moved = abs(sum(nxt[k] for k in det_keys) - sum(out[k] for k in det_keys)) / sum(out[k] for k in det_keys)
    assert moved >= 1e-3, moved
    gap2 = max(abs(nxt[k] - nxt2[k]) / (abs(nxt2[k]) + 1e-30) for k in det_keys)

    # torch.optim.SGD fed the very gradients the DetectorOptim saw, from the same start
    twins = [torch.nn.Parameter(p.clone()) for p in init]
    opt3 = torch.optim.SGD([{"params": [t], "lr": F.f32(lr), "weight_decay": F.f32(wd)} for t, (lr, wd) in zip(twins, opt.groups)],
                           lr=kw["base_lr"], momentum=F.f32(kw["momentum"]))
    for t, g in zip(twins, grads):
        t.grad = g.clone()
    opt3.step()
    worst = 0.0
    for i, (p, t) in enumerate(zip(after, twins)):
        p64, m64, M = F.sgd(init[i], grads[i], None, opt.groups[i][0], opt.groups[i][1], kw["momentum"])
        _, bp = F.bounds(init[i], m64, opt.groups[i][0], M)
        d = (p.detach().cpu().double() - t.detach().cpu().double()).abs()
        assert bool((d <= 2 * bp).all()), opt.names[i]
        assert bool(((p.detach().cpu().double() - p64).abs() <= bp).all()), opt.names[i]
        worst = max(worst, float((d / (2 * bp).clamp_min(1e-300)).max()))
    print(f"[detector_optim] Stage2Step: loss gap {gap:.2e}, iteration 2: detector-loss gap {gap2:.2e} after a move of {moved:.2e}; "
          f"worst parameter gap / (2 x bound) {worst:.3f}")


def test_state_dict_round_trip_and_scheduler_check(amd):
    """Two steps -> state_dict -> a new optimiser over copies of the parameters -> load -> the third step lands bit for bit where three
    uninterrupted steps land (momentum and iteration travelled); another schedule is refused."""
    g = torch.Generator().manual_seed(6)
    names = ["a.weight", "a.bias", "b.norm.weight", "c.weight"]
    shapes = [(6, 5, 3, 3), (6,), (6,), (1000, 7)]
    init = [torch.randn(s, generator=g) for s in shapes]
    init[0] = init[0].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)       # a conv weight in [O][kh][kw][I] memory, as fpn_sr keeps them
    grads = [[torch.randn(s, generator=g) for s in shapes] for _ in range(3)]

    def fresh(values):
        ps = [torch.nn.Parameter(v.clone().cuda() if v.is_contiguous() else v.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)) for v in values]
        return ps, amd.DetectorOptim(list(zip(names, ps)), **KW)

    def run(ps, opt, steps):
        for gs in steps:
            for p, gr in zip(ps, gs):
                p.grad = gr.cuda()                                              # (contiguous: the conv weight's gradient is re-laid out)
            opt.step()
    pa, oa = fresh(init)
    run(pa, oa, grads)
    assert oa.relayouts == 3 and oa.iter == 3
    pb, ob = fresh(init)
    run(pb, ob, grads[:2])
    sd = copy.deepcopy(ob.state_dict())
    assert sd["iteration"] == 2 and list(sd["optimizer"]["momentum_buffer"]) == names and sd["scheduler"]["steps"] == [1]
    assert [tuple(v.shape) for v in sd["optimizer"]["momentum_buffer"].values()] == shapes
    pc, oc = fresh([p.detach().cpu() for p in pb])
    oc.load_state_dict(sd)
    assert oc.iter == 2
    run(pc, oc, grads[2:])
    torch.cuda.synchronize()
    for a, c in zip(pa, pc):
        assert torch.equal(a, c)
    assert all(torch.equal(x, y) for x, y in zip(oa.state_dict()["optimizer"]["momentum_buffer"].values(), oc.state_dict()["optimizer"]["momentum_buffer"].values()))
    other = amd.DetectorOptim(list(zip(names, pc)), **{**KW, "lr_steps": (5,)})
    with pytest.raises(ValueError, match="scheduler steps"):
        other.load_state_dict(sd)
    with pytest.raises(KeyError, match="missing"):
        oc.load_state_dict({**sd, "optimizer": {"momentum_buffer": {}}})
