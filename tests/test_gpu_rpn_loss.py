"""The RPN's training side on the GPU (afigan_amd/rpn.py: RPN.losses, csrc/rpn_loss.hip) against tests/rpn_loss_f64.py, staged like
test_gpu_rpn.py so that no rounding difference leaks into a discrete decision:
  1. match      labels and matched_idx EQUAL the plain-loop checker (its IoU is numpy float32 in the kernel's order) on the cases
                tests/test_rpn_host.py's sibling test_rpn_loss_host.py holds to their purpose: no box, one box, an empty image beside a full one,
                identical boxes, an IoU exactly at t1 and one ulp below each threshold, tied low-quality matches, a box that overlaps nothing,
                more boxes than one LDS tile.  Three levels 13 x 17 / 7 x 9 / 4 x 5, A = 3: 912 anchors, four blocks, the last one ragged;
  2. sample     equal to the checker for given keys (quota above, at and below the class sizes, duplicate, constant and extreme keys);
  3. loss       against fp64 on the checker's labels and sample: |loss - ref| <= K 2^-24 sum |term| with K_CLS = 10 and K_LOC = 5 counted
                from the formulas (rpn_loss_f64.py; numpy float32 passes them on the CPU: test_rpn_loss_host.py); the logit gradient element-wise
                within 9 x 2^-24 scale, the delta gradient exactly +-scale / 0 for beta = 0 and within 4 x 2^-24 scale for beta > 0; every element
                outside the sample bit-zero; logits of +-30 and a delta equal to its target among the sampled anchors;
  4. end to end RPN.losses' gradients of the six parameters and of every feature map against float64 CPU autograd of the restated head and
                losses, fed the GPU's own labels and sample.  The per-op bars of test_gpu_pixgemm.py / test_gpu_wino.py are stated in different
                norms (a capped max-norm, a relative L2 tied to one reduction length) and do not compose over conv3x3 -> ReLU -> conv1x1 ->
                a sparse gradient, so the bar is the stated alternative: the relative L2 deviation of torch-CPU float32 autograd of the same
                restatement from float64, times 4 (another summation order, f16x3 pieces).  Measured values: see the test's docstring;
  5. determinism  labels, sample, losses and the head-output gradient bit-identical over two runs, the parameter gradients under
                set_option("deterministic", 1); NaN-poisoned workspaces change nothing;
  6. forward    in training mode with ground truth: the proposals of the eval-mode selection at the same top-k, the losses of losses()."""
import numpy as np
import pytest
import torch

import rpn_loss_f64 as O

pytestmark = pytest.mark.gpu

CASES = O.match_cases()
SAMPLES = O.sample_cases()
FEATURES = ["p3", "p4", "p5"]
_ORACLE = {}


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


def _oracle(name):
    if name not in _ORACLE:
        c = CASES[name]
        anc, _ = O.anchors(c["cells"])
        _ORACLE[name] = [O.match(anc, g, *c["thresholds"]) for g in c["gts"]]
    return _ORACLE[name]


def _pm(x):
    """CPU NCHW -> GPU tensor whose memory is [N][H][W][C], with those strides spelled out"""
    N, C_, H, W = x.shape
    flat = x.permute(0, 2, 3, 1).reshape(-1).cuda()
    return flat.as_strided((N, C_, H, W), (H * W * C_, 1, W * C_, C_))


def _gpu_match(amd, c):
    gt, counts = O.pad_gt(c["gts"])
    return amd.ops.rpn_match(O.LEVEL_HW, O.STRIDES, torch.from_numpy(c["cells"]).cuda(), c["cells"].shape[1], torch.from_numpy(gt).cuda(),
                             torch.from_numpy(counts).cuda(), c["thresholds"])


# ------------------------------------------------------------------------------------------------ 1. match
@pytest.mark.parametrize("name", list(CASES))
def test_match_equals_the_oracle(amd, name):
    c = CASES[name]
    labels, midx = _gpu_match(amd, c)
    again = _gpu_match(amd, c)
    assert labels.dtype == torch.int8 and midx.dtype == torch.int32 and tuple(labels.shape) == (2, 912)
    assert torch.equal(labels, again[0]) and torch.equal(midx, again[1])
    labels, midx = labels.cpu().numpy(), midx.cpu().numpy()
    for n, (want_l, want_m, _) in enumerate(_oracle(name)):
        assert np.array_equal(labels[n], want_l), (name, n, np.nonzero(labels[n] != want_l)[0][:8])
        assert np.array_equal(midx[n], want_m), (name, n, np.nonzero(midx[n] != want_m)[0][:8])


def test_match_and_sample_refuse_wrong_dtypes(amd):
    cell = torch.from_numpy(O.cell_anchors()).cuda()
    gt, counts = torch.zeros(2, 3, 4, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(amd.AfiError, match="int32"):
        amd.ops.rpn_match(O.LEVEL_HW, O.STRIDES, cell, 3, gt, counts.long())
    with pytest.raises(amd.AfiError, match="fp32"):
        amd.ops.rpn_match(O.LEVEL_HW, O.STRIDES, cell, 3, gt.double(), counts)
    labels = torch.zeros(2, 912, dtype=torch.int8, device="cuda")
    with pytest.raises(amd.AfiError, match="int8 labels"):
        amd.ops.rpn_sample(labels.int(), labels.int(), 8, 0.5)
    with pytest.raises(amd.AfiError, match="32-bit integer keys"):
        amd.ops.rpn_sample(labels, labels.long(), 8, 0.5)
    with pytest.raises(amd.AfiError, match="4096"):
        amd.ops.rpn_sample(labels, labels.int(), 5000, 0.5)


# ------------------------------------------------------------------------------------------------ 2. sample
def _keys(k):
    return torch.from_numpy(k.view(np.int32)).cuda()          # the same 32 bits: the kernel compares them unsigned


@pytest.mark.parametrize("name", list(SAMPLES))
def test_sample_equals_the_oracle(amd, name):
    labels, keys, batch, frac = SAMPLES[name]
    lg = torch.from_numpy(labels).cuda()
    out, sidx, n_pos, n_neg = amd.ops.rpn_sample(lg, _keys(keys), batch, frac)
    again = amd.ops.rpn_sample(lg, _keys(keys), batch, frac)
    assert all(torch.equal(a, b) for a, b in zip((out, sidx, n_pos, n_neg), again)) and torch.equal(lg.cpu(), torch.from_numpy(labels))
    out, sidx, n_pos, n_neg = out.cpu().numpy(), sidx.cpu().numpy(), n_pos.cpu().numpy(), n_neg.cpu().numpy()
    assert sidx.shape == (2, batch)
    for n in range(2):
        want, idx, p, q = O.sample(labels[n], keys[n], batch, frac)
        assert (n_pos[n], n_neg[n]) == (p, q) and np.array_equal(out[n], want), (name, n, n_pos[n], n_neg[n], p, q)
        assert sidx[n, :p + q].tolist() == idx and (sidx[n, p + q:] == -1).all()
        # the relabelling and the list say the same thing
        assert np.array_equal(np.sort(sidx[n, :p]), np.nonzero(out[n] == 1)[0]) and np.array_equal(np.sort(sidx[n, p:p + q]), np.nonzero(out[n] == 0)[0])


# ------------------------------------------------------------------------------------------------ 3. loss
def _loss_inputs(c):
    N, B, R = c["N"], c["batch"], len(c["anc"])
    sidx = np.full((N, B), -1, np.int32)
    for n in range(N):
        sidx[n, :len(c["sidx"][n])] = c["sidx"][n]
    gt, counts = O.pad_gt(c["gts"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(heads=[_pm(torch.from_numpy(h)) for h in c["heads"]], cell=dev(c["cells"]), gt=dev(gt), counts=dev(counts),
                midx=dev(np.stack(c["midx"]).astype(np.int32)), sidx=dev(sidx), n_pos=dev(np.array(c["n_pos"], np.int32)),
                n_neg=dev(np.array(c["n_neg"], np.int32)))


@pytest.mark.parametrize("beta,weights", [(0.0, (1.0, 1.0, 1.0, 1.0)), (0.5, (2.0, 2.0, 1.0, 1.0))])
def test_losses_and_head_gradient_against_fp64(amd, beta, weights):
    """K_CLS = 10 and K_LOC = 5 roundings of 2^-24 per term (counted in rpn_loss_f64.py), relative to sum |term|: the sums are fp64."""
    c = O.loss_case(weights)
    g = _loss_inputs(c)
    A, scale = c["A"], 2.0 / (c["batch"] * c["N"])           # LOSS_WEIGHT 2
    run = lambda: amd.ops.rpn_loss(g["heads"], O.STRIDES, g["cell"], A, g["gt"], g["counts"], g["midx"], g["sidx"], g["n_pos"], g["n_neg"],
                                   weights, beta, scale, scale)
    loss, grads = run()
    loss2, grads2 = run()
    assert torch.equal(loss, loss2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    lc, ll, want, ac, al = O.losses(c["heads"], c["anc"], c["where"], A, c["gts"], c["midx"], c["sidx"], c["n_pos"], c["n_neg"], weights, beta, scale)
    loss = loss.double().cpu().numpy()
    bar_c, bar_l = O.K_CLS * O.EPS * ac * scale, O.K_LOC * O.EPS * al * scale
    print(f"\nbeta {beta}: loss_cls {loss[0]:.9g} err {abs(loss[0] - lc):.3e} (bar {bar_c:.3e}); loss_loc {loss[1]:.9g} err {abs(loss[1] - ll):.3e} (bar {bar_l:.3e})")
    assert abs(loss[0] - lc) <= bar_c and abs(loss[1] - ll) <= bar_l
    s32 = float(np.float32(scale))
    worst_z = worst_d = 0.0
    for got, ref in zip(grads, want):
        assert ops_dense(got) and got.shape == ref.shape
        got = got.cpu().numpy()
        # bit-zero (+0) wherever the reference is zero: everything outside the sample, and the planted d = 0.  (Inside the sample fp32 may
        # round a gradient to 0 that fp64 does not: sigmoid(30) - 1.)
        assert not got[ref == 0].any() and not np.signbit(got[ref == 0]).any() and (ref == 0).sum() > ref.size - 5 * 64
        ez, ed = np.abs(got[:, :A] - ref[:, :A]).max(), np.abs(got[:, A:5 * A] - ref[:, A:5 * A])
        worst_z, worst_d = max(worst_z, ez), max(worst_d, ed.max())
        assert ez <= O.K_GRAD_LOGIT * O.EPS * scale
        if beta == 0.0:
            assert np.isin(got[:, A:5 * A], [0.0, s32, -s32]).all() and np.array_equal(np.sign(got[:, A:5 * A]), np.sign(ref[:, A:5 * A]))
        else:
            assert ed.max() <= O.K_GRAD_DELTA * O.EPS * scale
    print(f"worst logit-gradient error {worst_z:.3e} (bar {O.K_GRAD_LOGIT * O.EPS * scale:.3e}), delta-gradient error {worst_d:.3e}")
    n, i, ch = c["planted_zero"]                                                            # the delta equal to its target: d = 0, gradient 0
    l, y, x, _ = c["where"][i]
    assert grads[l][n, ch, y, x].item() == 0.0 and grads[l][n, ch + 1, y, x].item() != 0.0


def ops_dense(t):
    return t.permute(0, 2, 3, 1).is_contiguous()


# ------------------------------------------------------------------------------------------------ 4 - 6. the module
class _GT:
    def __init__(self, boxes):
        self.gt_boxes = boxes


class _Imgs:
    def __init__(self, sizes):
        self.image_sizes = sizes

    def __len__(self):
        return len(self.image_sizes)


WINO = dict(channels=128, level_hw=[(24, 24), (7, 9)], strides=[8, 16], sizes=[32, 64])      # 2 x 24 x 24 = 1152 pixels of 128 channels: the Winograd regime


def _module(amd, beta=0.0, channels=16, level_hw=O.LEVEL_HW, strides=O.STRIDES, sizes=O.SIZES, **keys):
    from afigan_amd.fpn_sr import ShapeSpec
    names = FEATURES[:len(strides)]
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[s] for s in sizes], "ASPECT_RATIOS": [O.RATIOS]},
                               "RPN": {"IN_FEATURES": names, "PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 50, "PRE_NMS_TOPK_TRAIN": 200,
                                       "POST_NMS_TOPK_TRAIN": 50, "BATCH_SIZE_PER_IMAGE": 32, "SMOOTH_L1_BETA": beta, "LOSS_WEIGHT": 2.0, **keys}})
    m = amd.RPN(cfg, {f: ShapeSpec(channels=channels, stride=s) for f, s in zip(names, strides)})
    g = torch.Generator().manual_seed(1)
    k = (16.0 / channels) ** 0.5                              # the outputs keep their size when the channel count grows
    with torch.no_grad():                                    # detectron2's std 0.01 would leave every logit near 0
        for p, std in zip(m.parameters(), (0.08 * k, 0.1, 0.25 * k, 0.3, 0.25 * k, 0.3)):
            p.copy_(torch.randn(p.shape, generator=g) * std)
    return m.cuda()


def _inputs(seed=2, channels=16, level_hw=O.LEVEL_HW, **_):
    g = torch.Generator().manual_seed(seed)
    feats = {f: torch.randn((2, channels, H, W), generator=g) for f, (H, W) in zip(FEATURES, level_hw)}
    gts = [_GT(torch.from_numpy(b)) for b in CASES["random"]["gts"]]
    R = sum(H * W * 3 for H, W in level_hw)
    keys = torch.randint(-2 ** 31, 2 ** 31, (2, R), generator=g, dtype=torch.int64).to(torch.int32)
    return feats, gts, keys


def _run(m, feats, gts, keys, wc=1.0, wl=1.0):
    xs = {f: v.cuda().requires_grad_(True) for f, v in feats.items()}
    m.zero_grad(set_to_none=True)
    out = m.losses(None, xs, [_GT(g.gt_boxes.cuda()) for g in gts], None if keys is None else keys.cuda())
    (wc * out["loss_rpn_cls"] + wl * out["loss_rpn_loc"]).backward()
    torch.cuda.synchronize()
    grads = {f: x.grad for f, x in xs.items()}
    grads.update({k: p.grad for k, p in m.named_parameters()})
    return out, grads, m.last_assignment


@pytest.mark.parametrize("beta,shape", [(0.0, {}), (0.5, {}), (0.0, WINO)], ids=["beta0", "beta0.5", "winograd"])
def test_rpn_losses_end_to_end_against_fp64_autograd(amd, beta, shape):
    """Bar per tensor: 4 x the relative L2 deviation of torch-CPU float32 autograd from float64 on the same inputs, labels and sample
    (another summation order and f16x3 pieces on the GPU side).  The upstream gradients of the two losses differ (1 and 0.5): each reaches its own
    channels.  Measured on MI355X, relative L2 (GPU / CPU fp32 -> bar = 4 x CPU fp32), worst tensor of each kind:
      16 channels, direct convs, beta 0 / 0.5:  feature maps 8.1e-8 / 1.0e-7 and 1.2e-7 / 2.1e-7; conv.weight 8.7e-8 / 9.7e-8 and 1.2e-7 / 1.7e-7;
                the 1x1 weights 9.5e-8 / 1.8e-7 and 1.2e-7 / 2.7e-7; biases 6.9e-8 / 6.9e-8 and 9.2e-8 / 1.2e-7 (anchor_deltas.bias at beta 0
                is a sum of +-scale: exact on both sides, 0 / 0);
      128 channels at 2 x 24 x 24 (Winograd forms, f16x3): that level's feature map 2.4e-7 / 1.2e-7 (bar 4.6e-7), conv.weight 2.4e-7 / 1.2e-7
                (bar 4.8e-7), everything else at or below CPU fp32's own deviation.
    The losses themselves: within 4 x the CPU-fp32 deviation, which is floored at one fp32 rounding of the value."""
    m = _module(amd, beta, **shape).trainable_(True)
    feats, gts, keys = _inputs(**shape)
    FEATS = list(feats)
    out, grads, asg = _run(m, feats, gts, keys, 1.0, 0.5)
    assert set(out) == {"loss_rpn_cls", "loss_rpn_loc"} and all(v.dim() == 0 and v.requires_grad for v in out.values())
    n_pos, n_neg = asg["n_pos"].tolist(), asg["n_neg"].tolist()
    sidx = [asg["sampled_idx"][n, :n_pos[n] + n_neg[n]].tolist() for n in range(2)]
    midx = asg["matched_idx"].cpu().numpy()
    assert min(n_pos) >= 1 and all(p + q == 32 for p, q in zip(n_pos, n_neg))
    anc, where = O.anchors(O.cell_anchors(shape.get("sizes", O.SIZES)), shape.get("level_hw", O.LEVEL_HW), shape.get("strides", O.STRIDES))
    names = ["rpn_head.conv.weight", "rpn_head.conv.bias", "rpn_head.objectness_logits.weight", "rpn_head.objectness_logits.bias",
             "rpn_head.anchor_deltas.weight", "rpn_head.anchor_deltas.bias"]
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    scale = 2.0 / (32 * 2)

    def ref(dtype):
        xs = [feats[f].to(dtype).requires_grad_(True) for f in FEATS]
        ps = [sd[k].to(dtype).requires_grad_(True) for k in names]
        lc, ll = O.torch_losses(xs, ps, 3, anc, where, CASES["random"]["gts"], midx, sidx, n_pos, n_neg, (1.0, 1.0, 1.0, 1.0), beta, scale)
        (lc + 0.5 * ll).backward()
        g = {f: x.grad for f, x in zip(FEATS, xs)}
        g.update({k: p.grad for k, p in zip(names, ps)})
        return (lc.item(), ll.item()), g
    (lc64, ll64), g64 = ref(torch.float64)
    (lc32, ll32), g32 = ref(torch.float32)
    rel = lambda a, b: ((a.double().cpu() - b).norm() / b.norm()).item()
    print(f"\nbeta {beta}: losses gpu {out['loss_rpn_cls'].item():.8g} {out['loss_rpn_loc'].item():.8g}; fp64 {lc64:.8g} {ll64:.8g}; cpu fp32 {lc32:.8g} {ll32:.8g}")
    bad = []
    for k in FEATS + names:
        e_gpu, e_cpu = rel(grads[k].contiguous(), g64[k]), rel(g32[k], g64[k])
        print(f"  {k:36s} rel L2: gpu {e_gpu:.3e}   cpu fp32 {e_cpu:.3e}   bar {4 * e_cpu:.3e}")
        assert tuple(grads[k].shape) == tuple(g64[k].shape)
        if not e_gpu <= 4 * e_cpu:
            bad.append((k, e_gpu, e_cpu))
    for got, want, w32 in ((out["loss_rpn_cls"].item(), lc64, lc32), (out["loss_rpn_loc"].item(), ll64, ll32)):
        assert abs(got - want) <= 4 * max(abs(w32 - want), 2.0 ** -24 * abs(want))             # (one fp32 rounding of the result itself at least)
    assert not bad, bad


def test_determinism_and_poisoned_workspaces(amd, monkeypatch):
    m = _module(amd).trainable_(True)
    feats, gts, keys = _inputs()
    cx = amd._lib.current_ctx()
    prev = cx.get_option("deterministic")
    cx.set_option("deterministic", 1)
    try:
        out1, g1, a1 = _run(m, feats, gts, keys)
        out2, g2, a2 = _run(m, feats, gts, keys)
        monkeypatch.setattr(amd.ops, "_POISON", True)        # workspaces and fresh outputs start as NaN: nothing may be read before it is written
        out3, g3, a3 = _run(m, feats, gts, keys)
    finally:
        cx.set_option("deterministic", prev)
    for o, g, a in ((out2, g2, a2), (out3, g3, a3)):
        assert all(torch.equal(a1[k], a[k]) for k in a1) and all(torch.equal(out1[k], o[k]) for k in out1)
        assert all(torch.equal(g1[k], g[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g[k])]
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())


def test_default_keys_come_from_torchs_generator(amd):
    m = _module(amd)
    feats, gts, _ = _inputs()
    runs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        with torch.no_grad():
            out = m.losses(None, {f: v.cuda() for f, v in feats.items()}, [_GT(g.gt_boxes.cuda()) for g in gts])
        runs.append((m.last_assignment["sampled_idx"].clone(), out["loss_rpn_cls"].item()))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and not torch.equal(runs[0][0], runs[2][0])
    assert not any(p.requires_grad for p in m.parameters())


def test_training_forward_returns_the_eval_proposals_and_the_losses(amd):
    m = _module(amd).trainable_(True).train()
    feats, gts, keys = _inputs()
    xs = {f: v.cuda() for f, v in feats.items()}
    gtc = [_GT(g.gt_boxes.cuda()) for g in gts]
    imgs = _Imgs([(104, 136), (100, 130)])
    props, losses = m(imgs, xs, gtc, keys=keys.cuda())
    alone = m.losses(imgs, xs, gtc, keys.cuda())
    assert all(torch.equal(losses[k], alone[k]) for k in ("loss_rpn_cls", "loss_rpn_loc")) and losses["loss_rpn_cls"].requires_grad
    m.eval()
    with torch.no_grad():
        want, empty = m(imgs, xs)                            # *_TOPK_TEST = *_TOPK_TRAIN in this config
    assert empty == {} and len(props) == len(want) == 2
    for p, w in zip(props, want):
        assert 0 < len(p) <= 50 and torch.equal(p.proposal_boxes.tensor, w.proposal_boxes.tensor) and torch.equal(p.objectness_logits, w.objectness_logits)
        assert not p.proposal_boxes.tensor.requires_grad
    with pytest.raises(amd.AfiError, match="gt_instances"):
        m(imgs, xs, gtc)
