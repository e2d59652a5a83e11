"""CPU-side checks of the detector's optimiser step: tests/detector_optim_f64.py -- the yardstick of test_gpu_detector_optim.py -- against
torch.optim.SGD in fp64; the parameter groups and the schedule at their edges; the refusals; the launcher's argument checks (host code)."""
import ctypes as C
import types

import pytest
import torch

import afigan_amd as amd
from afigan_amd import _lib, detector_optim

import detector_optim_f64 as F

# keys of GeneralizedRCNN over FPN_AFIGAN over the small trainable ResNet, an RPN and box + mask heads (test_gpu_detector_optim.py builds it)
NAMES = {
    "backbone.bottom_up.res3.0.shortcut.weight": "w", "backbone.bottom_up.res4.1.conv2.weight": "w",
    "backbone.fpn_lateral2.weight": "w", "backbone.fpn_lateral2.bias": "b", "backbone.fpn_output5.bias": "b",
    "backbone.srf_module.conv1.0.weight": "w", "backbone.srf_module.conv1.0.bias": "b",
    "proposal_generator.rpn_head.conv.weight": "w", "proposal_generator.rpn_head.objectness_logits.bias": "b",
    "roi_heads.box_head.fc1.weight": "w", "roi_heads.box_predictor.bbox_pred.bias": "b",
    "roi_heads.mask_head.mask_fcn1.norm.weight": "n", "roi_heads.mask_head.mask_fcn1.norm.bias": "n", "roi_heads.mask_head.deconv.bias": "b",
    "roi_heads.mask_head.prenorm.weight": "n", "bias": "w", "x.bias_scale": "w",
}


def test_restatement_equals_torch_sgd_in_fp64():
    """3 steps, mixed groups, gscale folded into the gradients torch sees, one parameter that never gets a gradient: 1e-15 relative."""
    g = torch.Generator().manual_seed(0)
    kw = dict(base_lr=0.02, weight_decay=1e-2, weight_decay_norm=0.0, bias_lr_factor=2.0, weight_decay_bias=5e-3)
    names = ["a.weight", "a.bias", "a.norm.weight", "b.weight", "idle.weight"]
    shapes = [(5, 3), (5,), (5,), (4, 3, 3, 3), (2, 2)]
    p32 = [torch.randn(s, generator=g) for s in shapes]
    params = [torch.nn.Parameter(t.double()) for t in p32]
    groups = [F.group(n, **kw) for n in names]
    assert groups == [(0.02, 1e-2), (0.04, 5e-3), (0.02, 0.0), (0.02, 1e-2), (0.02, 1e-2)]
    mom, gscale = 0.9, 0.5
    opt = torch.optim.SGD([{"params": [p], "lr": F.f32(lr), "weight_decay": F.f32(wd)} for p, (lr, wd) in zip(params, groups)], lr=0.02, momentum=F.f32(mom))
    mine_p, mine_m = [t.clone() for t in p32], [None] * len(names)
    for step in range(3):
        fac = F.schedule(step, steps=(2,), gamma=0.5, warmup_factor=0.1, warmup_iters=2)
        assert fac == [0.1, 0.55, 0.5][step]
        grads = [torch.randn(s, generator=g) for s in shapes]
        for i, (p, gr, grp) in enumerate(zip(params, grads, opt.param_groups)):
            grp["lr"] = F.f32(groups[i][0] * fac)
            p.grad = None if names[i].startswith("idle") else gr.double() * F.f32(gscale)
        opt.step()
        for i in range(len(names)):
            if names[i].startswith("idle"):
                continue
            mine_p[i], mine_m[i], _ = F.sgd(mine_p[i], grads[i], mine_m[i], groups[i][0] * fac, groups[i][1], mom, gscale)
    for i, (p, n) in enumerate(zip(params, names)):
        assert float((p.detach() - mine_p[i].double()).abs().max()) <= 1e-15 * float(p.detach().abs().max()), n
        if n.startswith("idle"):
            assert p not in opt.state or "momentum_buffer" not in opt.state[p]
            assert torch.equal(p.detach(), p32[i].double())
        else:
            buf = opt.state[p]["momentum_buffer"]
            assert float((buf - mine_m[i]).abs().max()) <= 1e-15 * float(buf.abs().max()), n


def test_sgd_carries_fp32_inputs_exactly():
    """The restatement's inputs are the fp32 values themselves (nothing is re-rounded on the way in), and the trajectory is `sgd` repeated."""
    g = torch.Generator().manual_seed(1)
    p0, gs = torch.randn(7, generator=g), [torch.randn(7, generator=g) for _ in range(2)]
    p1, m1, M = F.sgd(p0, gs[0], None, 0.1, 0.01, 0.9, 2.0)
    assert torch.equal(m1, gs[0].double() * 2.0 + F.f32(0.01) * p0.double()) and torch.equal(M, (2.0 * gs[0].double()).abs() + (F.f32(0.01) * p0.double()).abs())
    p2, m2, _ = F.sgd(p1, gs[1], m1, 0.1, 0.01, 0.9, 2.0)                                   # (fp64 tensors pass through .double() unchanged)
    tp, tm, ep, em = F.trajectory(p0, gs, [0.1, 0.1], 0.01, 0.9, 2.0)
    assert torch.equal(tp, p2) and torch.equal(tm, m2)
    bm, bp = F.bounds(p0, m1, 0.1, M)
    assert bool((em >= bm).all()) and bool((ep >= bp).all()) and bool((bp > 0).all())        # two steps' bound is no tighter than one step's


def test_groups_by_key():
    kw = dict(base_lr=0.02, weight_decay=1e-4, weight_decay_norm=0.25, bias_lr_factor=2.0, weight_decay_bias=0.5)
    want = {"w": (0.02, 1e-4), "b": (0.04, 0.5), "n": (0.02, 0.25)}
    for name, kind in NAMES.items():
        assert F.group(name, **kw) == want[kind] == detector_optim.param_group(name, **kw), name
    assert F.group("any.bias") == (0.001, 1e-4) and F.group("any.norm.bias") == (0.001, 0.0) and F.group("any.weight") == (0.001, 1e-4)


def test_schedule_at_its_edges():
    kw = dict(steps=(210000, 250000), gamma=0.1, warmup_factor=1e-3, warmup_iters=1000)
    assert F.schedule(0, **kw) == 1e-3
    assert F.schedule(999, **kw) == 1e-3 * (1 - 0.999) + 0.999
    assert F.schedule(1000, **kw) == 1.0 == F.schedule(209999, **kw)
    assert F.schedule(210000, **kw) == 0.1 and F.schedule(249999, **kw) == 0.1
    assert F.schedule(250000, **kw) == pytest.approx(0.01, rel=1e-15) and F.schedule(10 ** 6, **kw) == F.schedule(250000, **kw)
    for it in (0, 1, 999, 1000, 1001, 209999, 210000, 250000, 300000):                       # the package's schedule is the same function
        assert amd.warmup_multistep_lr(0.02, it, kw["steps"], 0.1, 1e-3, 1000) == pytest.approx(0.02 * F.schedule(it, **kw), rel=1e-15), it


def _cfg(**solver):
    return types.SimpleNamespace(SOLVER=types.SimpleNamespace(**solver))


def test_refusals():
    model = torch.nn.Linear(2, 2)
    with pytest.raises(amd.AfiError, match="NESTEROV"):
        amd.build_detector_optimizer(_cfg(NESTEROV=True), model)
    with pytest.raises(amd.AfiError, match="CLIP_GRADIENTS"):
        amd.build_detector_optimizer(_cfg(CLIP_GRADIENTS=types.SimpleNamespace(ENABLED=True)), model)
    with pytest.raises(amd.AfiError, match="LR_SCHEDULER_NAME"):
        amd.build_detector_optimizer(_cfg(LR_SCHEDULER_NAME="WarmupCosineLR"), model)
    with pytest.raises(amd.AfiError, match="no CPU fallback"):                               # a disabled CLIP_GRADIENTS passes; CPU parameters do not
        amd.build_detector_optimizer(_cfg(CLIP_GRADIENTS=types.SimpleNamespace(ENABLED=False)), model)
    with pytest.raises(amd.AfiError, match="requires grad"):
        amd.DetectorOptim([("w", torch.nn.Parameter(torch.zeros(2), requires_grad=False))])
    step = amd.DetectorStep(model.eval(), None)
    with pytest.raises(AssertionError, match="eval mode"):
        step.run_step([])


def test_launcher_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    bad = _lib.DEFINES["AFI_ERR_BAD_ARG"]
    t = (_lib.DetSgdDesc * 2)()                                                              # two n = 0 entries: valid, nothing to launch

    def go(host, dev, nt, max_units=0, unit_off=None, total=0):
        return lib.afi_detector_sgd_step(host, dev, nt, max_units, unit_off, total, 0.9, 1.0, None)
    assert go(t, t, 2) == 0 and go(t, t, 2, unit_off=C.c_void_p(16)) == 0
    assert go(None, t, 2) == bad and go(t, None, 2) == bad
    assert go(t, t, 0) == bad and go(t, t, -1) == bad and go(t, t, 65536) == bad
    assert go(t, t, 2, max_units=-1) == bad and go(t, t, 2, unit_off=C.c_void_p(16), total=-1) == bad
    d = t[1]
    d.p = d.g = d.m = 256
    d.n, d.O, d.I, d.k, d.fold_out, d.s64 = 36, 2, 2, 3, 256, 256
    for field, value in (("k", 2), ("k", 0), ("s64", None), ("n", 35), ("O", 0), ("p", None), ("n", -1)):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert go(t, t, 2, max_units=1) == bad, (field, value)
        setattr(d, field, keep)
    assert C.sizeof(_lib.DetSgdDesc) == 72
    units = amd.ops.detector_sgd_units
    assert [units(n) for n in (0, 1, 4096, 4097, 600001)] == [0, 1, 1, 2, 147]
    assert units(4 * 80 * 9, 4, 80, 3, True) == 3 and units(128 * 64 * 9, 128, 64, 3, True) == 64 and units(64 * 256, 64, 256, 1, True) == 4
