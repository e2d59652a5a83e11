"""Host-side checks of the Winograd reference (tests/wino_f64.py) and of the case table of tests/test_gpu_wino.py: no GPU.

The float64 restatement must BE the convolution (the matrices copied from csrc/winograd.hip are right, the tiling and padding are right);
the fp32 restatement, which sets every bar of the GPU file, must sit where a correct fp32 Winograd evaluation sits -- a broken yardstick
would silently loosen every bar; and the table must name what the GPU file then proves."""
import math

import pytest
import torch

import test_gpu_wino as G
import wino_f64 as wf

ALGEBRA_SHAPES = [(2, 8, 12, 33, 31), (1, 4, 8, 3, 40), (1, 8, 4, 40, 1), (2, 4, 4, 5, 2), (1, 4, 4, 1, 1)]


@pytest.mark.parametrize("tiling", [2, 4])
@pytest.mark.parametrize("op", wf.OPS)
@pytest.mark.parametrize("shape", ALGEBRA_SHAPES, ids=str)
def test_float64_restatement_is_the_convolution(shape, op, tiling):
    """odd sizes, H or W smaller than a tile, N = 2: restate(..., float64) == F.conv2d / autograd in float64 to 1e-12 in both norms"""
    a, b = wf.inputs(op, *shape)
    em, el = wf.errors(wf.restate(op, tiling, a, b, torch.float64), wf.reference(op, a, b))
    assert em <= 1e-12 and el <= 1e-12, (em, el)


def test_matrices_interpolate_the_stated_points():
    """B^T, G, A^T are a Toom-Cook triple of the points {0, 1, -1, inf} / {0, 1, -1, 1/2, -2, inf}: for polynomials d, g the identity
    A^T [(G g) . (B^T d)] == correlation(d, g) holds exactly (float64, small integers scaled), and G' / A'^T are the triple of the
    transposed problem; a single wrong constant breaks it"""
    for m in (2, 4):
        BT, Gm, AT, Gp, ApT = (wf.matrix(m, k) for k in ("BT", "G", "AT", "Gp", "ApT"))
        gen = torch.Generator().manual_seed(m)
        d = torch.randint(-8, 9, (m + 2,), generator=gen).double()
        g = torch.randint(-8, 9, (3,), generator=gen).double()
        e = torch.randint(-8, 9, (m,), generator=gen).double()
        y = torch.stack([sum(d[i + k] * g[k] for k in range(3)) for i in range(m)])
        assert torch.allclose(AT @ ((Gm @ g) * (BT @ d)), y, rtol=0, atol=1e-11)
        dw = torch.stack([sum(d[i + k] * e[i] for i in range(m)) for k in range(3)])
        assert torch.allclose(ApT @ ((Gp @ e) * (BT @ d)), dw, rtol=0, atol=1e-11)


# the figures of the fp32 restatement at 1 x K -> K x 91 x 91 (randn, w / sqrt(9 Cin)): (max-norm, rel. L2)
QUOTED = {(2, 128): (4.7e-7, 3.5e-7), (4, 128): (3.3e-6, 1.5e-6), (2, 256): (7.7e-7, 4.9e-7), (4, 256): (5.5e-6, 2.0e-6)}


@pytest.mark.parametrize("tiling,K", sorted(QUOTED))
def test_fp32_restatement_sits_at_the_quoted_figures(tiling, K):
    _, _, ref, rest = wf.yardstick("fwd", tiling, 1, K, K, 91, 91)
    em, el = wf.errors(rest, ref)
    qm, ql = QUOTED[(tiling, K)]
    print(f"[wino-host] F({tiling}x{tiling}) K = {K}: max-norm {em:.2e} (quoted {qm:.1e})  rel-L2 {el:.2e} (quoted {ql:.1e})")
    assert qm / 2 <= em <= qm * 2 and ql / 2 <= el <= ql * 2, (em, el)


def _shapes():
    seen = {}
    for c in G.ALL_CASES + G.SCALE_CASES:
        seen.setdefault((c.op, c.tiling) + c.shape, c)
    return sorted(seen)


@pytest.mark.parametrize("key", _shapes(), ids=str)
def test_fp32_restatement_at_the_gpu_shapes(key):
    """every (op, tiling, shape) the GPU file holds a kernel to: the yardstick is finite, is not zero, and stays below 2e-5 (max-norm) and
    1e-5 (rel. L2) -- far inside today's 1e-4 / 3e-4, so no bar of the GPU file can be looser than the bars it replaces"""
    op, tiling, *shape = key
    _, _, ref, rest = wf.yardstick(op, tiling, *shape)
    assert torch.isfinite(ref).all() and torch.isfinite(rest).all() and ref.abs().max() > 0
    em, el = wf.errors(rest, ref)
    bm, bl = wf.bars((em, el), wf.ktot(op, tiling, *shape))
    print(f"[wino-host] {op} F{tiling} {tuple(shape)}: max-norm {em:.2e}  rel-L2 {el:.2e}  bars {bm:.2e} / {bl:.2e}")
    assert 0 < em <= 2e-5 and 0 < el <= 1e-5, (em, el)
    assert math.isfinite(bm) and bm <= 1e-4 and bl <= 1e-4


def test_case_table_is_well_formed():
    kinds_nt = set(G.NT_BATCHED + G.NT_FALLBACK)
    kinds_tn = set(G.TN_BATCHED + G.TN_FALLBACK)
    for c in G.ALL_CASES + G.SCALE_CASES:
        assert c.ep in G.ENTRY and c.dtype in wf.FP32_GRADE + tuple(wf.TOL_CONV), c
        assert c.tiling in (2, 4) and c.kind in (kinds_tn if c.op == "wgrad" else kinds_nt), c
        assert (c.split in (2, 3)) == (c.kind == 21), c
        assert c.view in ("dense", "crop", "cslice", "crop_slice") and (c.view == "crop_slice") <= (c.op == "wgrad") and c.out in ("fresh", "slice"), c
        assert (c.o16 is not None) == (c.ep == "fwd16"), c
        assert c.Cin % 4 == 0 and c.Cout % 4 == 0, c
        if c.tiling == 4:                                   # F(4x4) only from 8192 pixels on, never for a forward a backward may follow
            assert c.N * c.H * c.W >= 8192 and c.ep not in ("fwd", "fwd16") and c.dtype != "bf16", c
    ids = [repr(c) for c in G.ALL_CASES]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]


def test_case_table_covers_every_form():
    grade = [c for c in G.ALL_CASES if c.dtype in wf.FP32_GRADE]
    for form in G.FORMS:
        for dt in wf.FP32_GRADE:
            assert any(G.form_of(c) == form and c.dtype == dt for c in grade), (form, dt)
    named = {c.kind for c in G.ALL_CASES}
    assert named >= {13, 17, 21, 14, 18, 22, 0, 2, 3, 8, 9, 10}, sorted(named)

    def has(pred):
        return any(pred(c) for c in G.ALL_CASES)
    for dt in wf.FP32_GRADE:
        assert has(lambda c: c.ep == "fwd" and c.dtype == dt and c.bias) and has(lambda c: c.ep == "fwd" and c.dtype == dt and not c.bias)
        for t in (2, 4):
            assert {c.act for c in G.ALL_CASES if c.ep == "infer" and c.dtype == dt and c.tiling == t} == {0, 1, 2}, (dt, t)
            assert {c.z for c in G.ALL_CASES if c.ep == "dgrad" and c.dtype == dt and c.tiling == t} == {0, 1}, (dt, t)
            assert has(lambda c: c.ep == "wgrad" and c.dtype == dt and c.tiling == t and c.alpha != 1.0)
        # the same shape on F(4x4) and, with winograd_f4_backward = 0, on F(2x2)
        for ep in ("dgrad", "wgrad"):
            assert has(lambda c: c.ep == ep and c.dtype == dt and c.shape == G.F4A and c.tiling == 4 and not c.opts)
            assert has(lambda c: c.ep == ep and c.dtype == dt and c.shape == G.F4A and c.tiling == 2 and c.opts == G.F2_ONLY)
        # just under the threshold: F(2x2) under _infer, _dgrad and _wgrad
        for ep in ("infer", "dgrad", "wgrad"):
            assert has(lambda c: c.ep == ep and c.dtype == dt and c.shape == G.UND and c.tiling == 2)
        for view in ("crop", "cslice"):
            assert has(lambda c: c.dtype == dt and c.view == view)
        assert has(lambda c: c.dtype == dt and c.view == "crop_slice") and has(lambda c: c.dtype == dt and c.out == "slice")
    for dt in wf.TOL_CONV:
        assert {c.ep for c in G.ALL_CASES if c.dtype == dt} >= {"fwd", "infer", "dgrad", "wgrad"}, dt
    assert has(lambda c: c.ep == "infer" and c.dtype == "bf16" and c.N * c.H * c.W >= 8192 and c.tiling == 2)
    for t in (2, 4):                                        # both f16x3 NT tile sizes at a 256-column shape
        assert {c.split for c in G.ALL_CASES if c.kind == 21 and c.tiling == t and "f16_nt256_min_tiles" in c.opts} == {2, 3}, t
    assert {c.o16 for c in G.O16_CASES} == {torch.bfloat16, torch.float16}
    assert {"batched", "fallback"} == {G.form_of(c)[2] for c in G.O16_CASES}
