"""The training side of the box branch of StandardROIHeads on the GPU (afigan_amd/roi_heads.py: StandardROIHeads.losses, csrc/roi_loss.hip)
against tests/roi_loss_f64.py, staged like test_gpu_rpn_loss.py so that no rounding difference leaks into a discrete decision.  N = 2, P = 40,
B = 32; levels 32 x 40, 16 x 20, 8 x 10, 4 x 5 (strides 4 .. 32); box sets from roi_f64.align_boxes (doubled for the 128 x 160 image).
  1. label / sample / gather   EQUAL the plain-loop checker on the cases test_roi_loss_host.py holds to their purpose;
  2. losses and dpred           against fp64 at the bars of DESIGN 22 (cross-entropy 2, smooth L1 5, logit gradient 2, delta gradient 0 / 4 units
                                of 2^-24); every other entry bit-zero;
  3. ROIAlign backward          |dF - ref| <= (t + 4) 2^-24 A per element, t and A from the checker; pixels no box reaches bit-zero, also with
                                NaN-poisoned fresh tensors;
  4. end to end                 gradients of every feature map and head parameter against float64 CPU autograd of the restated pooler, head and
                                losses on the GPU's own assignment: 4 x the deviation of CPU float32 autograd from float64;
  5. determinism                bit-identical over two runs, the parameter gradients under set_option("deterministic", 1);
  6. detector                   a GeneralizedRCNN_AFExtractor with a torch backbone, a trainable RPN and trainable ROI heads returns the four
                                losses, and their sum reaches every part."""
import numpy as np
import pytest
import torch

import roi_loss_f64 as T
import rpn_loss_f64 as RL

pytestmark = pytest.mark.gpu

F = np.float32
LABELS = T.label_cases()
SAMPLES = T.sample_cases()
FEATURES = ["p2", "p3", "p4", "p5"]
WEIGHTS = (10.0, 10.0, 5.0, 5.0)


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _keys(k):
    return torch.from_numpy(np.ascontiguousarray(k).view(np.int32)).cuda()      # the same 32 bits: the kernel compares them unsigned


def _pm(x):
    """CPU NCHW -> GPU tensor whose memory is [N][H][W][C], with those strides spelled out"""
    N, C_, H, W = x.shape
    flat = x.permute(0, 2, 3, 1).reshape(-1).cuda()
    return flat.as_strided((N, C_, H, W), (H * W * C_, 1, W * C_, C_))


# ------------------------------------------------------------------------------------------------ 1. label, sample, gather
@pytest.mark.parametrize("append_gt", [True, False], ids=["append_gt", "proposals_only"])
@pytest.mark.parametrize("name", list(LABELS))
def test_label_sample_gather_equal_the_checker(amd, name, append_gt):
    c = LABELS[name]
    K, batch, frac = 3, T.B, 0.25
    gcls = [(np.arange(len(g)) % K).astype(np.int32) for g in c["gts"]]
    pp, cp, gt, gc, cg = T.pad_lists(c["proposals"], c["gts"], gcls)
    R = pp.shape[1] + gt.shape[1]
    args = (_dev(pp), _dev(cp), _dev(gt), _dev(cg))
    labels, midx = amd.ops.roi_label(*args, c["thresh"], append_gt)
    again = amd.ops.roi_label(*args, c["thresh"], append_gt)
    assert labels.dtype == torch.int8 and midx.dtype == torch.int32 and tuple(labels.shape) == (T.N, R)
    assert torch.equal(labels, again[0]) and torch.equal(midx, again[1])
    keys = np.random.default_rng(23).integers(0, 2 ** 32, size=(T.N, R), dtype=np.uint64).astype(np.uint32)
    l2, sidx, n_pos, n_neg = amd.ops.rpn_sample(labels, _keys(keys), batch, frac)
    got = amd.ops.roi_gather_samples(args[0], args[1], args[2], _dev(gc), args[3], midx, sidx, n_pos, n_neg, K, append_gt)
    labels, midx, l2, sidx = labels.cpu().numpy(), midx.cpu().numpy(), l2.cpu().numpy(), sidx.cpu().numpy()
    boxes, counts, cls, gboxes = (t.cpu().numpy() for t in got)
    assert cls.dtype == np.int32 and counts.dtype == np.int32 and boxes.shape == (T.N, batch, 4) and gboxes.shape == (T.N, batch, 4)
    for n in range(T.N):
        want_l, want_m = T.label(c["proposals"][n], len(c["proposals"][n]), c["gts"][n], R, c["thresh"], append_gt)
        assert np.array_equal(labels[n], want_l), (name, n, np.nonzero(labels[n] != want_l)[0][:8])
        assert np.array_equal(midx[n], want_m), (name, n, np.nonzero(midx[n] != want_m)[0][:8])
        want_l2, idx, p, q = RL.sample(want_l, keys[n], batch, frac)
        assert (int(n_pos[n]), int(n_neg[n])) == (p, q) and np.array_equal(l2[n], want_l2) and sidx[n, :p + q].tolist() == idx
        b, cnt, k, gb = T.gather(c["proposals"][n], len(c["proposals"][n]), c["gts"][n], gcls[n], want_m, idx, p, q, K, batch, append_gt)
        assert counts[n] == cnt and np.array_equal(boxes[n], b) and np.array_equal(cls[n], k) and np.array_equal(gboxes[n], gb)
    if name == "no_boxes":
        assert (labels[:, :T.P][:, :29] == 0).all() and (midx == 0).all() and (gboxes == 0).all() and (cls[cls >= 0] == K).all()


@pytest.mark.parametrize("name", list(SAMPLES))
def test_sample_quotas_and_the_training_list(amd, name):
    """Given labels over the [N, P + 10] candidate list (the last three entries padding): afi_rpn_sample's sample, and the training list
    afi_roi_gather_samples makes of it with given matches."""
    labels, keys, batch, frac = SAMPLES[name]
    rng = np.random.default_rng(29)
    K, G = 5, 10
    props = [RL._rand_boxes(rng, T.P) for _ in range(T.N)]
    gts = [RL._rand_boxes(rng, G) for _ in range(T.N)]
    gcls = [rng.integers(0, K, G).astype(np.int32) for _ in range(T.N)]
    midx = rng.integers(0, G, labels.shape).astype(np.int32)
    pp, cp, gt, gc, cg = T.pad_lists(props, gts, gcls)
    out, sidx, n_pos, n_neg = amd.ops.rpn_sample(_dev(labels), _keys(keys), batch, frac)
    got = amd.ops.roi_gather_samples(_dev(pp), _dev(cp), _dev(gt), _dev(gc), _dev(cg), _dev(midx), sidx, n_pos, n_neg, K)
    boxes, counts, cls, gboxes = (t.cpu().numpy() for t in got)
    out, sidx = out.cpu().numpy(), sidx.cpu().numpy()
    for n in range(T.N):
        want, idx, p, q = RL.sample(labels[n], keys[n], batch, frac)
        assert (int(n_pos[n]), int(n_neg[n])) == (p, q) and np.array_equal(out[n], want)
        assert sidx[n, :p + q].tolist() == idx and (sidx[n, p + q:] == -1).all()
        b, cnt, k, gb = T.gather(props[n], T.P, gts[n], gcls[n], midx[n], idx, p, q, K, batch)
        assert counts[n] == cnt and np.array_equal(boxes[n], b) and np.array_equal(cls[n], k) and np.array_equal(gboxes[n], gb)


def test_ops_refuse_wrong_dtypes(amd):
    p, cp = torch.zeros(2, 4, 4, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    g = torch.zeros(2, 3, 4, device="cuda")
    with pytest.raises(amd.AfiError, match="int32"):
        amd.ops.roi_label(p, cp.long(), g, cp)
    with pytest.raises(amd.AfiError, match="fp32"):
        amd.ops.roi_label(p.double(), cp, g, cp)
    labels, midx = amd.ops.roi_label(p, cp, g, cp)
    l2, sidx, n_pos, n_neg = amd.ops.rpn_sample(labels, torch.zeros_like(midx), 8, 0.25)
    with pytest.raises(amd.AfiError, match="int32"):
        amd.ops.roi_gather_samples(p, cp, g, torch.zeros(2, 3, device="cuda"), cp, midx, sidx, n_pos, n_neg, 3)
    with pytest.raises(amd.AfiError, match="int32"):
        amd.ops.roi_box_loss(torch.zeros(16, 16, device="cuda"), 3, False, torch.zeros(2, 8, 4, device="cuda"), cp,
                             torch.zeros(2, 8, device="cuda"), torch.zeros(2, 8, 4, device="cuda"))
    with pytest.raises(amd.AfiError, match="fp32"):
        amd.ops.roi_align_bwd(torch.zeros(16, 7, 7, 8, device="cuda", dtype=torch.float64).permute(0, 3, 1, 2), [(8, 8)], 2,
                              torch.zeros(2, 8, 4, device="cuda"), cp)


# ------------------------------------------------------------------------------------------------ 2. losses and dpred
LOSS_CASES = {"K5": (5, False, 0.0, {}), "K5_beta0.5": (5, False, 0.5, {}), "K5_agnostic": (5, True, 0.5, {}), "K80": (80, False, 0.5, {}),
              "K80_beta0": (80, False, 0.0, {}), "no_foreground_image": (5, False, 0.0, {"no_fg_image": True}), "rtot_zero": (5, False, 0.5, {"empty": True})}


@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_losses_and_dpred_against_fp64(amd, name, monkeypatch):
    K, agnostic, beta, kw = LOSS_CASES[name]
    c = T.loss_case(K, agnostic, **kw)
    monkeypatch.setattr(amd.ops, "_POISON", True)             # the kernel owns the whole of dpred: NaN-filled before the call
    args = (_dev(c["pred"]), K, agnostic, _dev(c["boxes"]), _dev(c["counts"]), _dev(c["cls"]), _dev(c["gboxes"]), WEIGHTS, beta)
    loss, dpred = amd.ops.roi_box_loss(*args)
    loss2, dpred2 = amd.ops.roi_box_loss(*args)
    assert torch.equal(loss, loss2) and torch.equal(dpred, dpred2) and loss.dtype == torch.float32 and tuple(dpred.shape) == c["pred"].shape
    loss, dpred = loss.cpu().numpy().astype(np.float64), dpred.cpu().numpy()
    lc, lb, ref, ac, al, rtot = T.box_loss(c["pred"], K, agnostic, c["boxes"], c["counts"], c["cls"], c["gboxes"], WEIGHTS, beta)
    print(f"\n{name}: gpu {loss[0]:.9g} {loss[1]:.9g}  fp64 {lc:.9g} {lb:.9g}  Rtot {rtot}  bars {T.K_CLS * T.EPS * ac / max(rtot, 1):.3e} "
          f"{T.K_LOC * T.EPS * al / max(rtot, 1):.3e}")
    if rtot == 0:
        assert loss[0] == 0 and loss[1] == 0 and not dpred.any()
        return
    assert abs(loss[0] - lc) <= T.K_CLS * T.EPS * ac / rtot and abs(loss[1] - lb) <= T.K_LOC * T.EPS * al / rtot
    logit = np.zeros(ref.shape, bool)
    logit[:, :K + 1] = True
    delta = (ref != 0) & ~logit
    live = np.zeros(ref.shape[0], bool)
    for n in range(T.N):
        live[n * T.B:n * T.B + c["counts"][n]] = True
    err = np.abs(dpred.astype(np.float64) - ref)
    assert err[logit].max() <= T.K_GRAD_LOGIT * T.EPS / rtot
    if beta < 1e-5:
        assert np.array_equal(dpred[delta], (np.sign(ref[delta]).astype(F) * F(1.0 / rtot)))
    elif delta.any():
        assert err[delta].max() <= T.K_GRAD_DELTA * T.EPS / rtot
    # everything else is bit-zero: the other classes' deltas, the padding columns, the padding rows, a delta equal to its target (beta 0)
    rest = ~(logit & live[:, None]) & ~delta
    assert not dpred[rest].any() and not np.signbit(dpred[rest]).any()
    fg_rows = np.nonzero(delta.any(1))[0]
    assert name in ("rtot_zero",) or len(fg_rows) >= 3
    if name == "no_foreground_image":
        assert (fg_rows < T.B).all()


# ------------------------------------------------------------------------------------------------ 3. ROIAlign backward
ALIGN_CASES = {"C8_S7_adaptive": (8, T.LEVELS, T.MIN_LEVEL, 7, 0, "align_boxes"), "C8_S14_ratio2": (8, T.LEVELS, T.MIN_LEVEL, 14, 2, "align_boxes"),
               "C8_identical": (8, T.LEVELS, T.MIN_LEVEL, 7, 2, "twenty_identical"), "C8_special": (8, T.LEVELS, T.MIN_LEVEL, 7, 0, "special"),
               "C256_one_level": (256, (T.LEVELS[2],), 4, 7, 0, "align_boxes"), "C260_ratio2": (260, T.LEVELS, T.MIN_LEVEL, 7, 2, "special")}
_ALIGN_REF = {}


def _align_ref(name):
    if name not in _ALIGN_REF:
        C, levels, min_level, S, sr, boxset = ALIGN_CASES[name]
        boxes, counts = T.align_bwd_box_sets()[boxset]
        g = np.random.default_rng(len(name)).standard_normal((T.N * T.B, C, S, S)).astype(F)
        _ALIGN_REF[name] = (g, boxes, counts, T.align_bwd(g, levels, min_level, boxes, counts, S, sr))
    return _ALIGN_REF[name]


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
@pytest.mark.parametrize("name", list(ALIGN_CASES))
def test_roi_align_bwd_against_fp64(amd, name, poison, monkeypatch):
    C, levels, min_level, S, sr, _ = ALIGN_CASES[name]
    g, boxes, counts, ref = _align_ref(name)
    if poison:
        monkeypatch.setattr(amd.ops, "_POISON", True)         # fresh outputs and workspaces start as NaN
    gg = _pm(torch.from_numpy(g))
    got = amd.ops.roi_align_bwd(gg, levels, min_level, _dev(boxes), _dev(counts), sr)
    again = amd.ops.roi_align_bwd(gg, levels, min_level, _dev(boxes), _dev(counts), sr)
    assert len(got) == len(levels)
    for l, (o, o2, (gr, ab, tm)) in enumerate(zip(got, again, ref)):
        assert tuple(o.shape) == gr.shape and amd.ops.is_dense_pm(o) and torch.equal(o, o2)
        o = o.cpu().numpy()
        slack = np.abs(o.astype(np.float64) - gr) - (tm[:, None] + T.K_ALIGN_BWD) * T.EPS * ab
        print(f"\n{name} level {l}: max |err| {np.abs(o - gr).max():.3e}, max terms {tm.max()}, worst err - bar {slack.max():.3e}, reached "
              f"{(tm > 0).mean():.2f}")
        assert slack.max() <= 0.0
        unreached = np.broadcast_to((tm == 0)[:, None], o.shape)
        assert not o[unreached].any() and not np.signbit(o[unreached]).any()
    assert sum(int((tm > 0).sum()) for _, _, tm in ref) > 0


# ------------------------------------------------------------------------------------------------ 4. end to end
class _GT:
    def __init__(self, boxes, classes):
        self.gt_boxes, self.gt_classes = boxes, classes


class _Prop:
    def __init__(self, boxes):
        self.proposal_boxes = boxes


class _Imgs:
    def __init__(self, sizes):
        self.image_sizes = sizes

    def __len__(self):
        return len(self.image_sizes)


def _heads(amd, channels=8, fc_dim=32, beta=0.0, ratio=0, K=5, agnostic=False):
    from afigan_amd.fpn_sr import ShapeSpec
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"MASK_ON": False, "ROI_HEADS": {"NAME": "StandardROIHeads", "IN_FEATURES": FEATURES, "NUM_CLASSES": K,
                                                               "BATCH_SIZE_PER_IMAGE": T.B},
                               "ROI_BOX_HEAD": {"NAME": "FastRCNNConvFCHead", "NUM_FC": 2, "FC_DIM": fc_dim, "POOLER_RESOLUTION": 7,
                                                "POOLER_SAMPLING_RATIO": ratio, "SMOOTH_L1_BETA": beta, "CLS_AGNOSTIC_BBOX_REG": agnostic}})
    h = amd.build_roi_heads(cfg, {f: ShapeSpec(channels=channels, stride=2 ** int(f[1:])) for f in FEATURES})
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                                    # detectron2's std 0.01 / 0.001 would leave every logit and delta near 0
        for k, p in h.named_parameters():
            std = 0.2 if k.endswith("bias") else (2.0 / p.shape[1]) ** 0.5 * (3.0 if "box_predictor" in k else 1.0)
            p.copy_(torch.randn(p.shape, generator=g) * std)
    return h.cuda()


def _inputs(channels=8, seed=2):
    g = torch.Generator().manual_seed(seed)
    feats = {f: torch.randn((T.N, channels, H, W), generator=g) for f, (H, W) in zip(FEATURES, T.LEVELS)}
    return feats, T.e2e_case()


def _run(h, feats, case, wc=1.0, wb=1.0, keys=True):
    xs = {f: v.cuda().requires_grad_(True) for f, v in feats.items()}
    h.zero_grad(set_to_none=True)
    props = [_Prop(_dev(case["proposals"][n, :case["counts_p"][n]])) for n in range(T.N)]
    tg = [_GT(_dev(case["gts"][n]), _dev(case["gt_classes"][n])) for n in range(T.N)]
    out = h.losses(None, xs, props, tg, _keys(case["keys"]) if keys else None)
    (wc * out["loss_cls"] + wb * out["loss_box_reg"]).backward()
    torch.cuda.synchronize()
    grads = {f: x.grad for f, x in xs.items()}
    grads.update({k: p.grad for k, p in h.named_parameters()})
    return out, grads, h.last_assignment


@pytest.mark.parametrize("channels,fc_dim,beta,ratio", [(8, 32, 0.0, 0), (8, 32, 0.5, 2), (128, 64, 0.0, 2)], ids=["c8", "c8_beta0.5", "c128"])
def test_losses_end_to_end_against_fp64_autograd(amd, channels, fc_dim, beta, ratio):
    """Bar per tensor: 4 x the relative L2 deviation of torch-CPU float32 autograd from float64 on the same inputs and the GPU's own
    assignment.  The upstream gradients of the two losses differ (1 and 0.5).  The measured values are recorded in DESIGN 22."""
    K = 5
    h = _heads(amd, channels, fc_dim, beta, ratio, K).trainable_()
    feats, case = _inputs(channels)
    out, grads, asg = _run(h, feats, case, 1.0, 0.5)
    assert set(out) == {"loss_cls", "loss_box_reg"} and all(v.dim() == 0 and v.requires_grad for v in out.values())
    want = T.assign(case, K)                                  # the GPU's assignment IS the checker's
    for k, w in (("boxes", "boxes"), ("counts", "counts"), ("gt_classes", "cls"), ("gt_boxes", "gboxes")):
        assert np.array_equal(asg[k].cpu().numpy(), want[w]), k
    n_pos, n_neg = asg["n_pos"].tolist(), asg["n_neg"].tolist()
    assert min(n_pos) >= 8 and min(n_neg) >= 8
    names = [k for k, _ in h.named_parameters()]
    assert names == ["box_head.fc1.weight", "box_head.fc1.bias", "box_head.fc2.weight", "box_head.fc2.bias", "box_predictor.cls_score.weight",
                     "box_predictor.cls_score.bias", "box_predictor.bbox_pred.weight", "box_predictor.bbox_pred.bias"]
    sd = {k: v.detach().cpu() for k, v in h.state_dict().items()}

    def ref(dtype):
        xs = [feats[f].to(dtype).requires_grad_(True) for f in FEATURES]
        ps = [sd[k].to(dtype).requires_grad_(True) for k in names]
        lc, lb = T.torch_losses(xs, ps, T.MIN_LEVEL, 7, ratio, want["boxes"], want["counts"], want["cls"], want["gboxes"], K, False, WEIGHTS, beta)
        (lc + 0.5 * lb).backward()
        g = {f: x.grad for f, x in zip(FEATURES, xs)}
        g.update({k: p.grad for k, p in zip(names, ps)})
        return (lc.item(), lb.item()), g
    (lc64, lb64), g64 = ref(torch.float64)
    (lc32, lb32), g32 = ref(torch.float32)
    rel = lambda a, b: ((a.double().cpu() - b).norm() / b.norm()).item()
    print(f"\n{channels} channels, beta {beta}: losses gpu {out['loss_cls'].item():.8g} {out['loss_box_reg'].item():.8g}; fp64 {lc64:.8g} {lb64:.8g}; "
          f"cpu fp32 {lc32:.8g} {lb32:.8g}")
    bad = []
    for k in FEATURES + names:
        assert g64[k] is not None and g64[k].norm() > 0, k
        e_gpu, e_cpu = rel(grads[k].contiguous(), g64[k]), rel(g32[k], g64[k])
        print(f"  {k:36s} rel L2: gpu {e_gpu:.3e}   cpu fp32 {e_cpu:.3e}   bar {4 * e_cpu:.3e}")
        assert tuple(grads[k].shape) == tuple(g64[k].shape)
        if not e_gpu <= 4 * e_cpu:
            bad.append((k, e_gpu, e_cpu))
    for got, w64, w32 in ((out["loss_cls"].item(), lc64, lc32), (out["loss_box_reg"].item(), lb64, lb32)):
        assert abs(got - w64) <= 4 * max(abs(w32 - w64), 2.0 ** -24 * abs(w64))                # (one fp32 rounding of the result itself at least)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 5. determinism, keys, frozen parameters
def test_determinism_and_poisoned_workspaces(amd, monkeypatch):
    h = _heads(amd).trainable_()
    feats, case = _inputs()
    cx = amd._lib.current_ctx()
    prev = cx.get_option("deterministic")
    cx.set_option("deterministic", 1)
    try:
        out1, g1, a1 = _run(h, feats, case)
        out2, g2, a2 = _run(h, feats, case)
        monkeypatch.setattr(amd.ops, "_POISON", True)
        out3, g3, a3 = _run(h, feats, case)
    finally:
        cx.set_option("deterministic", prev)
    for o, g, a in ((out2, g2, a2), (out3, g3, a3)):
        assert all(torch.equal(a1[k], a[k]) for k in a1) and all(torch.equal(out1[k], o[k]) for k in out1)
        assert all(torch.equal(g1[k], g[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g[k])]
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())


def test_default_keys_and_frozen_parameters(amd):
    h = _heads(amd)
    feats, case = _inputs()
    runs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        out, grads, asg = _run(h, feats, case, keys=False)
        runs.append((asg["sampled_idx"].clone(), out["loss_cls"].item()))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and not torch.equal(runs[0][0], runs[2][0])
    # frozen at construction: the features get their gradient, the parameters none
    assert not any(p.requires_grad for p in h.parameters()) and all(grads[k] is None for k, _ in h.named_parameters())
    assert all(grads[f] is not None and bool(grads[f].abs().sum() > 0) for f in FEATURES)


def test_training_forward_returns_the_sampled_proposals_and_the_losses(amd):
    h = _heads(amd).trainable_().train()
    feats, case = _inputs()
    xs = {f: v.cuda() for f, v in feats.items()}
    props = [_Prop(_dev(case["proposals"][n, :case["counts_p"][n]])) for n in range(T.N)]
    tg = [{"gt_boxes": _dev(case["gts"][n]), "gt_classes": _dev(case["gt_classes"][n])} for n in range(T.N)]     # the dict form
    imgs = _Imgs([T.IMAGE, T.IMAGE])
    sampled, losses = h(imgs, xs, props, tg, keys=_keys(case["keys"]))
    alone = h.losses(imgs, xs, props, tg, _keys(case["keys"]))
    assert all(torch.equal(losses[k], alone[k]) for k in ("loss_cls", "loss_box_reg")) and losses["loss_cls"].requires_grad
    want = T.assign(case, 5)
    for n, s in enumerate(sampled):
        c = want["counts"][n]
        assert len(s) == c and np.array_equal(s.proposal_boxes.tensor.cpu().numpy(), want["boxes"][n, :c])
        assert s.gt_classes.dtype == torch.int64 and np.array_equal(s.gt_classes.cpu().numpy(), want["cls"][n, :c])
        assert np.array_equal(s.gt_boxes.tensor.cpu().numpy(), want["gboxes"][n, :c])
    assert all(torch.equal(h.last_assignment[k].cpu(), torch.from_numpy(want[w])) for k, w in (("n_pos", "n_pos"), ("n_neg", "n_neg")))
    with pytest.raises(amd.AfiError, match="inference-only"):
        h(imgs, xs, props)
    with pytest.raises(amd.AfiError, match=r"gt_classes must lie in 0\.\.4"):
        h.losses(imgs, xs, props, [{"gt_boxes": t["gt_boxes"], "gt_classes": t["gt_classes"] + 3} for t in tg])


# ------------------------------------------------------------------------------------------------ 6. the detector
class _Pyramid(torch.nn.Module):
    """A small torch conv pyramid with the backbone's contract: p2 .. p5 at strides 4 .. 32."""
    size_divisibility = 32

    def __init__(self, channels=16):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, channels, 4, stride=4)
        self.down = torch.nn.ModuleList([torch.nn.Conv2d(channels, channels, 3, stride=2, padding=1) for _ in range(3)])
        self.channels = channels

    def output_shape(self):
        from afigan_amd.fpn_sr import ShapeSpec
        return {f: ShapeSpec(channels=self.channels, stride=2 ** int(f[1:])) for f in FEATURES}

    def forward(self, x):
        out = {"p2": torch.tanh(self.stem(x))}
        for f, conv in zip(FEATURES[1:], self.down):
            out[f] = torch.tanh(conv(out[FEATURES[FEATURES.index(f) - 1]]))
        return out


def test_detector_returns_four_losses_that_reach_every_part(amd):
    torch.manual_seed(0)
    backbone = _Pyramid().cuda()
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[16], [32], [64], [128]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": FEATURES, "PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 50, "PRE_NMS_TOPK_TRAIN": 200,
                                       "POST_NMS_TOPK_TRAIN": 50, "BATCH_SIZE_PER_IMAGE": 32}})
    rpn = amd.RPN(cfg, backbone.output_shape()).cuda().trainable_()
    heads = _heads(amd, channels=16).trainable_()
    model = amd.GeneralizedRCNN_AFExtractor(backbone=backbone, proposal_generator=rpn, roi_heads=heads, pixel_mean=[0.0, 0.0, 0.0],
                                            pixel_std=[1.0, 1.0, 1.0], device="cuda").train()
    case = T.e2e_case()
    g = torch.Generator().manual_seed(4)
    batch = [{"image_x0.5": torch.randn((3,) + T.IMAGE, generator=g), "targets": _GT(_dev(case["gts"][n]), _dev(case["gt_classes"][n]))}
             for n in range(T.N)]
    losses, _ = model(batch)
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"}
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for part in (backbone, rpn.rpn_head, heads.box_head, heads.box_predictor):
        for k, p in part.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0), (type(part).__name__, k)
