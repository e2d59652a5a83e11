"""CPU-side checks of the wide RPN selection: the training-mode limit and its messages, the argument checks of the new entry
points through the library (fake, never dereferenced pointers: every status below comes back before anything is launched), the workspace
sizes, and the conditions tests/test_gpu_rpn_wide.py puts on its NMS lists, held to rpn_f64.nms_case_facts."""
import numpy as np
import pytest
import torch

import afigan_amd as amd
from afigan_amd import _lib, ops
from afigan_amd.fpn_sr import ShapeSpec

import rpn_f64 as R
from test_gpu_rpn_wide import NMS_WIDE_SEEDS, REF_LEVELS, nms_fixture

FEATURES = ["p3", "p4", "p5"]


def _cfg(**rpn_keys):
    cfg = amd.get_cfg()
    cfg.MODEL.merge_from_dict({"ANCHOR_GENERATOR": {"SIZES": [[32], [64], [128]], "ASPECT_RATIOS": [[0.5, 1.0, 2.0]]},
                               "RPN": {"IN_FEATURES": FEATURES, "PRE_NMS_TOPK_TEST": 1000, "POST_NMS_TOPK_TEST": 1000, **rpn_keys}})
    return cfg


def _shapes(channels=16):
    return {f: ShapeSpec(channels=channels, stride=8 * 2 ** i) for i, f in enumerate(FEATURES)}


class _Imgs:
    def __init__(self, sizes):
        self.image_sizes = sizes

    def __len__(self):
        return len(self.image_sizes)


class _GT:
    def __init__(self, boxes):
        self.gt_boxes = boxes


FEATS = {f: torch.zeros(1, 16, 4, 4) for f in FEATURES}
GT = [_GT(torch.tensor([[0.0, 0.0, 10.0, 10.0]]))]


def test_the_references_training_values_pass_the_topk_limit():
    """PRE_NMS_TOPK_TRAIN 2000 / POST_NMS_TOPK_TRAIN 1000 (Base-RCNN-FPN-AFIGAN.yaml): the training-mode forward gets as far as the first kernel,
    which refuses CPU features.  (Before the wide selection it raised the top-k refusal.)"""
    m = amd.RPN(_cfg(PRE_NMS_TOPK_TRAIN=2000, POST_NMS_TOPK_TRAIN=1000), _shapes()).train()
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        m(_Imgs([(32, 32)]), FEATS, GT)
    m = amd.RPN(_cfg(PRE_NMS_TOPK_TRAIN=4096, POST_NMS_TOPK_TRAIN=4000), _shapes()).train()
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        m(_Imgs([(32, 32)]), FEATS, GT)


def test_limits_that_stay():
    assert (ops.RPN_MAX_TOPK, ops.RPN_MAX_TOPK_WIDE, ops.RPN_MAX_MERGE_WIDE) == (1024, 4096, 5 * 4096) and sum(np.diff(REF_LEVELS)) <= ops.RPN_MAX_MERGE_WIDE
    m = amd.RPN(_cfg(PRE_NMS_TOPK_TRAIN=4097, POST_NMS_TOPK_TRAIN=1000), _shapes()).train()
    with pytest.raises(amd.AfiError, match=r"PRE_NMS_TOPK_TRAIN 4097.*1024.*4096.*losses\(\) works regardless"):
        m(_Imgs([(32, 32)]), FEATS, GT)
    m = amd.RPN(_cfg(), _shapes()).train()                 # 12000, detectron2's default: the message tests/test_rpn_loss_host.py pins
    with pytest.raises(amd.AfiError, match=r"PRE_NMS_TOPK_TRAIN 12000.*1024.*losses\(\) works regardless.*separate piece of work"):
        m(_Imgs([(32, 32)]), FEATS, GT)
    for k in (1025, 2000, 6000):                            # inference keeps the LDS-resident list
        with pytest.raises(amd.AfiError, match=rf"PRE_NMS_TOPK_TEST {k}.*1024"):
            amd.RPN(_cfg(PRE_NMS_TOPK_TEST=k), _shapes())


def test_wide_ops_refuse_cpu_tensors_and_name_their_limits():
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        ops.rpn_topk_wide(torch.zeros(1, 16, 40, 40), 3, 2000)
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        ops.rpn_nms_wide(torch.zeros(1, 2000, 4), torch.ones(1, 2000, dtype=torch.int32), 0.7)
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        ops.rpn_merge_wide(torch.zeros(1, 2000, 4), torch.zeros(1, 2000), torch.ones(1, 2000, dtype=torch.int32), [0, 2000], 100)
    with pytest.raises(amd.AfiError, match="CPU tensor"):
        ops.rpn_topk(torch.zeros(1, 16, 40, 40), 3, 1025)   # the device check comes first there too


def test_entry_points_check_their_arguments_without_a_device():
    lib = _lib.load()
    BAD, UNS, WS = (_lib.DEFINES[k] for k in ("AFI_ERR_BAD_ARG", "AFI_ERR_UNSUPPORTED", "AFI_ERR_WORKSPACE"))
    p = 0x1000

    def topk(view_p=p, N=1, H=80, W=96, A=3, k=2000, vals=p, idx=p, ld=None, ws=p, short=0):
        need = lib.afi_rpn_topk_wide_ws_floats(N, H, W, A) if 0 < A <= 16 and N > 0 else 0
        return lib.afi_rpn_topk_wide(_lib.View(view_p, H * W * 16, W * 16, 16), N, H, W, A, k, vals, idx, k if ld is None else ld, ws, need - short, None)
    for kw in ({"view_p": None}, {"vals": None}, {"idx": None}, {"N": 0}, {"N": 65536}, {"k": 0}, {"ld": 1999}, {"H": 0}, {"A": 0}):
        assert topk(**kw) == BAD, kw
    assert topk(H=30, W=30, k=2701) == BAD                  # k above H W A
    for kw in ({"k": 4097}, {"k": 1024}, {"k": 1}, {"A": 17}, {"H": 2048, "W": 2048, "A": 1}):      # k <= 1024 is afi_rpn_topk's: unsupported here
        assert topk(**kw) == UNS, kw
    for kw in ({"ws": None}, {"short": 1}, {"ws": p + 4}):
        assert topk(**kw) == WS, kw
    assert lib.afi_rpn_topk_wide_ws_floats(2, 40, 40, 3) == 0 == lib.afi_rpn_topk_ws_floats(2, 40, 40, 3)
    n = 80 * 96 * 3
    assert lib.afi_rpn_topk_wide_ws_floats(2, 80, 96, 3) == 2 * 4104 + 2 * 2 * n == lib.afi_rpn_topk_ws_floats(2, 80, 96, 3)
    assert lib.afi_rpn_topk_wide_ws_floats(1, 200, 336, 17) == -1 and lib.afi_rpn_topk_wide_ws_floats(1, 2048, 2048, 1) == -1

    def nms(boxes=p, valid=p, N=1, k=2000, ld=None, keep=p, ws=p, short=0):
        need = max(lib.afi_rpn_nms_wide_ws_floats(N, k), 0)
        return lib.afi_rpn_nms_wide(boxes, valid, N, k, k if ld is None else ld, 0.7, keep, ws, need - short, None)
    for kw in ({"boxes": None}, {"valid": None}, {"keep": None}, {"N": 0}, {"N": 65536}, {"k": -1}, {"ld": 1999}):
        assert nms(**kw) == BAD, kw
    assert nms(k=4097) == UNS
    assert nms(k=0) == 0 and nms(k=0, boxes=None, valid=None, keep=None, ws=None) == 0          # as afi_rpn_nms: nothing to do
    for kw in ({"ws": None}, {"short": 1}, {"ws": p + 4}):
        assert nms(**kw) == WS, kw
    assert lib.afi_rpn_nms_wide_ws_floats(2, 2000) == 2 * 2 * 2000 * 32 and lib.afi_rpn_nms_wide_ws_floats(1, 4096) == 2 * 4096 * 64
    assert lib.afi_rpn_nms_wide_ws_floats(3, 65) == 2 * 3 * 65 * 2 and lib.afi_rpn_nms_wide_ws_floats(1, 0) == 0
    assert lib.afi_rpn_nms_wide_ws_floats(1, 4097) == -1 and lib.afi_rpn_nms_wide_ws_floats(0, 10) == -1

    import ctypes as C

    def merge(off, boxes=p, vals=p, keep=p, N=1, L=None, post_k=1000, ob=p, ol=p, counts=p, no_off=False):
        L = len(off) - 1 if L is None else L
        arr = None if no_off else (C.c_int * len(off))(*off)
        return lib.afi_rpn_merge_wide(boxes, vals, keep, N, L, arr, post_k, ob, ol, counts, None)
    ok = list(REF_LEVELS)
    for kw in ({"boxes": None}, {"vals": None}, {"keep": None}, {"ob": None}, {"ol": None}, {"counts": None}, {"N": 0}, {"N": 65536}, {"post_k": 0},
               {"L": 0}, {"no_off": True}):
        assert merge(ok, **kw) == BAD, kw
    assert merge([1, 2000]) == BAD and merge([0, 2000, 1000]) == BAD and merge([0, 0]) == BAD
    assert merge([0, 4097]) == UNS and merge(list(range(0, 10 * 100, 100))) == UNS                 # a level above 4096; nine levels
    assert merge([0, 4096, 8192, 12288, 16384, 20480, 20481]) == UNS                                # the stated total is 5 x 4096
    # the narrow entry points keep their answers
    assert lib.afi_rpn_topk(_lib.View(p, 80 * 96 * 16, 96 * 16, 16), 1, 80, 96, 3, 1025, p, p, 1025, p, 1 << 30, None) == UNS
    assert lib.afi_rpn_nms(p, p, 1, 1025, 1025, 0.7, p, None) == UNS
    assert lib.afi_rpn_merge(p, p, p, 1, 1, (C.c_int * 2)(0, 1025), 10, p, p, p, None) == UNS


@pytest.mark.parametrize("n,thresh", sorted(NMS_WIDE_SEEDS))
def test_gpu_nms_lists_meet_their_conditions(n, thresh):
    """What tests/test_gpu_rpn_wide.py asserts before every launch, and that its shared fixture states what rpn_f64.nms_case_facts states."""
    seeds = NMS_WIDE_SEEDS[(n, thresh)]
    assert len(seeds) == 2 and seeds[0] != seeds[1]
    for seed in seeds:
        b, nonempty, ambiguous, want = nms_fixture(seed, n, thresh)
        assert b.shape == (n, 4) and b.dtype == np.float32
        assert b[:, 0::2].min() >= 0 and b[:, 0::2].max() <= R.NMS_IMAGE[1] and b[:, 1::2].min() >= 0 and b[:, 1::2].max() <= R.NMS_IMAGE[0]
        assert nonempty and ambiguous == 0 and 0.1 <= want.mean() <= 0.9, (seed, nonempty, ambiguous, want.mean())
        if n <= 2000 or ((n, thresh) == (4096, 0.7) and seed == seeds[0]):      # (the large lists cost seconds each: one of them is enough here)
            assert R.nms_case_facts(b, thresh) == (nonempty, ambiguous, want.sum() / n)
