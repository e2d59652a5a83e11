"""The training side of the mask branch of StandardROIHeads on the GPU (afigan_amd/roi_heads.py: _ROIMaskLossFn, csrc/mask_loss.hip) against
tests/mask_loss_f64.py.  N = 2, P = 40, B = 32, fraction 0.25 (Bf = 8); levels 32 x 40 .. 4 x 5 (test_gpu_roi_loss.py's shapes).
  1. targets        EQUAL the checker at M = 28 and M = 6 on the rows tests/test_mask_loss_host.py holds to their purpose, for every n_pos;
  2. loss and dz    against fp64 at the bars of DESIGN 23; padding rows bit-zero;
  3. dh, dW, db     dh from the kernel's own dz within one fp32 product; dW / db within (t + 2) 2^-24 sum |dz h|;
  4. end to end     gradients of every feature map and mask-head parameter (and, in the same call, the box branch's) against float64 CPU
                    autograd of the restatement on the GPU's own assignment and targets: 4 x the deviation of CPU float32 from float64;
  5. determinism    bit-identical over two runs and under NaN-poisoned workspaces, the parameter gradients under set_option("deterministic", 1);
  6. detector       a GeneralizedRCNN_AFExtractor with trainable mask heads returns five losses whose sum reaches every part."""
import numpy as np
import pytest
import torch

import mask_loss_f64 as Q
import roi_loss_f64 as T

pytestmark = pytest.mark.gpu

F = np.float32
EPS = Q.EPS
FEATURES = ["p2", "p3", "p4", "p5"]
WEIGHTS = (10.0, 10.0, 5.0, 5.0)


@pytest.fixture(scope="module")
def amd():
    import afigan_amd
    return afigan_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _keys(k):
    return torch.from_numpy(np.ascontiguousarray(k).view(np.int32)).cuda()


def _pm(x):
    """numpy NCHW -> GPU tensor whose memory is [N][H][W][C]"""
    x = torch.from_numpy(np.ascontiguousarray(x))
    N, C_, H, W = x.shape
    flat = x.permute(0, 2, 3, 1).reshape(-1).cuda()
    return flat.as_strided((N, C_, H, W), (H * W * C_, 1, W * C_, C_))


# ------------------------------------------------------------------------------------------------ 1. targets
_TARGET_REF = {}


def _target_ref(M, name):
    if (M, name) not in _TARGET_REF:
        c = Q.target_case(M)
        _TARGET_REF[(M, name)] = (c, Q.targets(c["instances"], c["boxes"], c["sidx"], c["midx"], Q.N_POS_CASES[name], c["counts_g"], Q.BF, M))
    return _TARGET_REF[(M, name)]


@pytest.mark.parametrize("name", list(Q.N_POS_CASES))
@pytest.mark.parametrize("M", [28, 6])
def test_targets_equal_the_checker(amd, M, name):
    c, (want, want_cfg) = _target_ref(M, name)
    polys = amd.ops.mask_polygons(c["instances"], Q.N, c["Gmax"], "cuda")
    out = torch.full((Q.N, Q.BF, M, M), 0xA5, dtype=torch.uint8, device="cuda")                # the kernel owns every byte
    args = (*polys, _dev(c["boxes"]), _dev(c["sidx"]), _dev(c["midx"]), _dev(c["counts_g"]), c["Gmax"],
            _dev(np.array(Q.N_POS_CASES[name], np.int32)), Q.BF, M)
    tg, cfg = amd.ops.mask_targets(*args, out=out)
    tg2, cfg2 = amd.ops.mask_targets(*args)
    assert tg.data_ptr() == out.data_ptr() and torch.equal(tg, tg2) and torch.equal(cfg, cfg2) and cfg.dtype == torch.int32
    got = tg.cpu().numpy()
    assert cfg.tolist() == want_cfg.tolist()
    assert set(np.unique(got).tolist()) <= {0, 1}
    for n in range(Q.N):
        for j in range(Q.BF):
            assert np.array_equal(got[n, j], want[n, j]), (M, name, n, j, c["kinds"][j] if n == 0 else "", int((got[n, j] != want[n, j]).sum()))
        assert not got[n, want_cfg[n]:].any()
    if name == "all":                                         # the float64 quotient would have given another mask for the row built to tell
        other = Q.targets(c["instances"], c["boxes"], c["sidx"], c["midx"], Q.N_POS_CASES[name], c["counts_g"], Q.BF, M, "fp64")[0]
        j = c["kinds"].index("split_quotient")
        assert not np.array_equal(other[0, j], got[0, j])


def test_targets_of_an_image_without_instances_beside_a_full_one(amd):
    M = 28
    c = Q.target_case(M)
    inst = [[], c["instances"][1]]                            # image 0 has no instance: its poly_off entries repeat 0
    counts_g = np.array([0, len(inst[1])], np.int32)
    polys = amd.ops.mask_polygons(inst, Q.N, c["Gmax"], "cuda")
    n_pos = np.array([3, Q.BF], np.int32)                     # (the sampler gives an empty image no positive; the kernel must not need that)
    tg, cfg = amd.ops.mask_targets(*polys, _dev(c["boxes"]), _dev(c["sidx"]), _dev(c["midx"]), _dev(counts_g), c["Gmax"], _dev(n_pos), Q.BF, M)
    want, want_cfg = Q.targets(inst, c["boxes"], c["sidx"], c["midx"], n_pos, counts_g, Q.BF, M)
    assert cfg.tolist() == want_cfg.tolist() == [3, Q.BF]
    assert np.array_equal(tg.cpu().numpy(), want) and not want[0].any() and want[1].any()


# ------------------------------------------------------------------------------------------------ 2. loss and dz, 3. dh, dW, db
_LOSS_REF = {}


def _loss_ref(name):
    if name not in _LOSS_REF:
        C, S, Km, kw = Q.LOSS_CASES[name]
        case = Q.loss_case(C, S, Km, **kw)
        h, w, b, cls, counts, tg = case
        _LOSS_REF[name] = (case, Q.mask_loss(h, w, b, cls[:, :Q.BF], counts, tg))
    return _LOSS_REF[name]


@pytest.mark.parametrize("name", list(Q.LOSS_CASES))
def test_loss_dz_and_predictor_backward_against_fp64(amd, name, monkeypatch):
    C, S, Km, kw = Q.LOSS_CASES[name]
    (h, w, b, cls, counts, tg), r = _loss_ref(name)
    monkeypatch.setattr(amd.ops, "_POISON", True)             # dz, dh and the workspaces are NaN-filled before the call
    hg, wg, bg = _pm(h), _dev(w), _dev(b)
    clsg = _dev(cls)[:, :Q.BF]                                # a view of the training list's classes: row stride B
    args = (hg, wg, bg, clsg, _dev(counts), _dev(tg))
    loss, dz = amd.ops.mask_loss(*args)
    loss2, dz2 = amd.ops.mask_loss(*args)
    assert torch.equal(loss, loss2) and torch.equal(dz, dz2) and tuple(dz.shape) == (Q.N * Q.BF, S, S, 4) and loss.dtype == torch.float32
    got, dzk = float(loss.cpu().numpy().astype(np.float64)[0]), dz.cpu().numpy()
    mtot = r["mtot"]
    live = np.repeat(r["live"], 1)
    if mtot == 0:
        assert got == 0.0 and not dzk.any() and not np.signbit(dzk).any()
    else:
        bar = (r["ez"].sum() + 2 * EPS * r["absterm"]) / mtot
        print(f"\n{name}: loss gpu {got:.9g} fp64 {r['loss']:.9g} |err| {abs(got - r['loss']):.3e} bar {bar:.3e}  Mtot {mtot}  max |z| "
              f"{np.abs(r['z']).max():.3g}")
        assert abs(got - r["loss"]) <= bar
        err = np.abs(Q.image_order(dzk).astype(np.float64) - r["dz"])
        dbar = (0.25 * r["ez"] + 2 * EPS) / mtot
        print(f"  dz: max |err| {err.max():.3e}, worst err / bar {(err / dbar)[live].max():.3f}")
        assert (err <= dbar)[live].all()
        assert not dzk[~live].any() and not np.signbit(dzk[~live]).any() and (~live).any()
    # the predictor's backward from the kernel's own dz (scaled, as the upstream gradient scales it)
    dzs = dz * 0.5
    dh, dW, db = amd.ops.mask_pred_bwd(hg, dzs, wg, clsg, args[4])
    dh2, dW2, db2 = amd.ops.mask_pred_bwd(hg, dzs, wg, clsg, args[4])
    assert torch.equal(dh, dh2) and torch.equal(dW, dW2) and torch.equal(db, db2)
    assert amd.ops.is_dense_pm(dh) and tuple(dh.shape) == h.shape and tuple(dW.shape) == (Km, C) and tuple(db.shape) == (Km,)
    p = Q.pred_bwd(h, dzs.cpu().numpy(), w, cls[:, :Q.BF], counts)
    dh, dW, db = dh.cpu().numpy(), dW.cpu().numpy().astype(np.float64), db.cpu().numpy().astype(np.float64)
    # one fp32 product: half an ulp, 2^-24 |dz w| on a normal result and 2^-150 on a subnormal one (|z| = 40 leaves dz near 1e-20)
    edh = np.abs(dh.astype(np.float64) - p["dh"])
    print(f"  dh: worst err / (2^-24 |dz w|) {(edh / np.maximum(EPS * p['dh_mag'], 1e-300))[p['dh_mag'] >= 2.0 ** -126].max(initial=0):.3f} on normal "
          f"results; {int(((p['dh_mag'] < 2.0 ** -126) & (p['dh_mag'] > 0)).sum())} subnormal products, max err there "
          f"{edh[p['dh_mag'] < 2.0 ** -126].max(initial=0):.3e}")
    assert (edh <= np.maximum(EPS * p["dh_mag"], 2.0 ** -150)).all()
    assert not dh[h == 0].any() and not dh[~live].any() and np.isfinite(dh).all()
    tW, tb = (p["terms"][:, None] + 2) * EPS * p["dW_abs"], (p["terms"] + 2) * EPS * p["db_abs"]
    eW, eb = np.abs(dW - p["dW"]), np.abs(db - p["db"])
    if mtot:
        print(f"  dW: worst err / bar {(eW / np.maximum(tW, 1e-300)).max():.4f}; db: {(eb / np.maximum(tb, 1e-300)).max():.4f}; classes with rows "
              f"{int((p['terms'] > 0).sum())} of {Km}")
    assert (eW <= tW).all() and (eb <= tb).all()
    none = p["terms"] == 0
    assert not dW[none].any() and not db[none].any()          # classes without a row: zeros, written


# ------------------------------------------------------------------------------------------------ 4. end to end
class _GT:
    def __init__(self, boxes, classes, polygons):
        self.gt_boxes, self.gt_classes = boxes, classes
        self.gt_masks = type("PolygonMasks", (), {"polygons": polygons})()


class _Prop:
    def __init__(self, boxes):
        self.proposal_boxes = boxes


def _heads(amd, channels=8, **kw):
    return Q.e2e_heads(amd, channels, **kw).cuda()


def _inputs(channels=8):
    case = T.e2e_case()
    return Q.e2e_features(channels), case, Q.e2e_polygons(case)


def _run(h, feats, case, inst, wm=1.0, wc=1.0, wb=1.0):
    xs = {f: v.cuda().requires_grad_(True) for f, v in feats.items()}
    h.zero_grad(set_to_none=True)
    props = [_Prop(_dev(case["proposals"][n, :case["counts_p"][n]])) for n in range(T.N)]
    tg = [_GT(_dev(case["gts"][n]), _dev(case["gt_classes"][n]), inst[n]) for n in range(T.N)]
    out = h.losses(None, xs, props, tg, _keys(case["keys"]))
    (wm * out["loss_mask"] + wc * out["loss_cls"] + wb * out["loss_box_reg"]).backward()
    torch.cuda.synchronize()
    grads = {f: x.grad for f, x in xs.items()}
    grads.update({k: p.grad for k, p in h.named_parameters()})
    return out, grads, h.last_assignment


@pytest.mark.parametrize("channels", [8, 128], ids=["c8_direct", "c128_winograd"])
def test_three_losses_end_to_end_against_fp64_autograd(amd, channels):
    """One call with all three losses: the feature gradient is the sum of both poolers' backward.  Bar per tensor: 4 x the relative L2
    deviation of torch-CPU float32 autograd from float64 on the same inputs, the GPU's own assignment and targets.  The measured values are
    recorded in DESIGN 23."""
    K, S = 5, 14
    h = _heads(amd, channels).trainable_(mask_head=True)
    feats, case, inst = _inputs(channels)
    out, grads, asg = _run(h, feats, case, inst, 0.75, 1.0, 0.5)
    assert set(out) == {"loss_cls", "loss_box_reg", "loss_mask"} and all(v.dim() == 0 and v.requires_grad for v in out.values())
    want = T.assign(case, K)
    for k, w in (("boxes", "boxes"), ("counts", "counts"), ("gt_classes", "cls"), ("gt_boxes", "gboxes")):
        assert np.array_equal(asg[k].cpu().numpy(), want[w]), k
    tg, cfg = asg["mask_targets"].cpu().numpy(), asg["counts_fg"].cpu().numpy()
    wtg, wcfg = Q.targets(inst, want["boxes"], want["sidx"], want["midx"], want["n_pos"], np.array([10, 10]), Q.BF, 2 * S)
    assert np.array_equal(tg, wtg) and cfg.tolist() == wcfg.tolist() == [Q.BF, Q.BF]                 # the GPU's targets ARE the checker's
    names = [k for k, _ in h.named_parameters()]
    mnames = [k for k in names if k.startswith("mask_head.")]
    bnames = [k for k in names if not k.startswith("mask_head.")]
    assert mnames == [f"mask_head.{l}.{t}" for l in ("mask_fcn1", "mask_fcn2", "deconv", "predictor") for t in ("weight", "bias")]
    sd = {k: v.detach().cpu() for k, v in h.state_dict().items()}
    fgb = want["boxes"][:, :Q.BF]

    def ref(dtype):
        xs = [feats[f].to(dtype).requires_grad_(True) for f in FEATURES]
        pm = [sd[k].to(dtype).requires_grad_(True) for k in mnames]
        pb = [sd[k].to(dtype).requires_grad_(True) for k in bnames]
        margins = []
        lm = Q.torch_mask_loss(xs, pm, T.MIN_LEVEL, S, 2, fgb, cfg, want["cls"], tg, K, margins)
        assert min(margins) > 1.0, margins                    # every ReLU decision of the fixture is made at fp32 resolution
        lc, lb = T.torch_losses(xs, pb, T.MIN_LEVEL, 7, 2, want["boxes"], want["counts"], want["cls"], want["gboxes"], K, False, WEIGHTS, 0.0)
        (0.75 * lm + lc + 0.5 * lb).backward()
        g = {f: x.grad for f, x in zip(FEATURES, xs)}
        g.update({k: p.grad for k, p in zip(mnames + bnames, pm + pb)})
        return lm.item(), g
    lm64, g64 = ref(torch.float64)
    lm32, g32 = ref(torch.float32)
    rel = lambda a, b: ((a.double().cpu() - b).norm() / b.norm()).item()
    print(f"\n{channels} channels: loss_mask gpu {out['loss_mask'].item():.8g}; fp64 {lm64:.8g}; cpu fp32 {lm32:.8g}")
    bad = []
    for k in FEATURES + mnames + bnames:
        assert g64[k] is not None and g64[k].norm() > 0, k
        assert tuple(grads[k].shape) == tuple(g64[k].shape), k
        e_gpu, e_cpu = rel(grads[k].contiguous(), g64[k]), rel(g32[k], g64[k])
        print(f"  {k:36s} rel L2: gpu {e_gpu:.3e}   cpu fp32 {e_cpu:.3e}   bar {4 * e_cpu:.3e}")
        if not e_gpu <= 4 * e_cpu:
            bad.append((k, e_gpu, e_cpu))
    assert abs(out["loss_mask"].item() - lm64) <= 4 * max(abs(lm32 - lm64), EPS * abs(lm64))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_determinism_and_poisoned_workspaces(amd, monkeypatch):
    h = _heads(amd).trainable_(mask_head=True)
    feats, case, inst = _inputs()
    cx = amd._lib.current_ctx()
    prev = cx.get_option("deterministic")
    cx.set_option("deterministic", 1)
    try:
        out1, g1, a1 = _run(h, feats, case, inst)
        a1 = dict(a1)
        out2, g2, a2 = _run(h, feats, case, inst)
        a2 = dict(a2)
        monkeypatch.setattr(amd.ops, "_POISON", True)
        out3, g3, a3 = _run(h, feats, case, inst)
    finally:
        cx.set_option("deterministic", prev)
    assert {"mask_targets", "counts_fg", "mask_dz", "mask_deconv"} <= set(a1)
    for o, g, a in ((out2, g2, a2), (out3, g3, a3)):
        assert all(torch.equal(a1[k], a[k]) for k in a1), [k for k in a1 if not torch.equal(a1[k], a[k])]
        assert all(torch.equal(out1[k], o[k]) for k in out1)
        assert all(torch.equal(g1[k], g[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g[k])]
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())


def test_frozen_mask_head_and_agnostic_predictor(amd):
    h = _heads(amd, agnostic=True)                            # frozen at construction: the features get their gradient, the parameters none
    feats, case, inst = _inputs()
    out, grads, asg = _run(h, feats, case, inst)
    assert h.mask_head.predictor.weight.shape[0] == 1 and bool(torch.isfinite(out["loss_mask"])) and out["loss_mask"].item() > 0
    assert all(grads[k] is None for k, _ in h.named_parameters()) and all(bool(grads[f].abs().sum() > 0) for f in FEATURES)
    with pytest.raises(amd.AfiError, match="no `gt_masks`"):
        h.losses(None, {f: v.cuda() for f, v in feats.items()}, [_Prop(_dev(case["proposals"][n])) for n in range(T.N)],
                 [{"gt_boxes": _dev(case["gts"][n]), "gt_classes": _dev(case["gt_classes"][n])} for n in range(T.N)])


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


def test_detector_returns_five_losses_that_reach_every_part(amd):
    torch.manual_seed(0)
    backbone = _Pyramid().cuda()
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[16], [32], [64], [128]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": FEATURES, "PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 50, "PRE_NMS_TOPK_TRAIN": 200,
                                       "POST_NMS_TOPK_TRAIN": 50, "BATCH_SIZE_PER_IMAGE": 32}})
    rpn = amd.RPN(cfg, backbone.output_shape()).cuda().trainable_()
    heads = _heads(amd, channels=16).trainable_(mask_head=True)
    model = amd.GeneralizedRCNN_AFExtractor(backbone=backbone, proposal_generator=rpn, roi_heads=heads, pixel_mean=[0.0, 0.0, 0.0],
                                            pixel_std=[1.0, 1.0, 1.0], device="cuda").train()
    ih, iw = 64, 80
    gts = [np.array([[4, 6, 40, 50], [30, 20, 76, 60], [10, 30, 30, 44]], F), np.array([[8, 8, 60, 40], [40, 34, 70, 62]], F)]
    g = torch.Generator().manual_seed(4)
    batch = []
    for n, b in enumerate(gts):
        polys = [[Q._ngon((x0 + x1) / 2, (y0 + y1) / 2, 0.45 * (x1 - x0), 0.45 * (y1 - y0), 9)] for x0, y0, x1, y1 in b.astype(np.float64)]
        batch.append({"image_x0.5": torch.randn((3, ih, iw), generator=g),
                      "targets": _GT(_dev(b), _dev(np.arange(len(b), dtype=np.int64) % 5), polys)})
    losses, _ = model(batch)
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_mask", "loss_rpn_cls", "loss_rpn_loc"}
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    mh = heads.mask_head
    for part in (backbone, rpn.rpn_head, heads.box_head, heads.box_predictor, mh.mask_fcn1, mh.deconv, mh.predictor):
        for k, p in part.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.abs().sum() > 0), (type(part).__name__, k)
