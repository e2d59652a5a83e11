"""CPU tests of tests/smallmap_f64.py (the float64 reference with resolved LeakyReLU masks) and of the case table of
tests/test_gpu_smallmap.py: the recording forward is the oracle's, a planted mask flip is named and explained away, planted errors that are
no flips are rejected, every case's candidate set is within the cap, and the table covers what it says it covers."""
import ctypes

import pytest
import torch

import smallmap_f64 as sm
import test_gpu_smallmap as T
from oracle import afigan_oracle as orc


@pytest.fixture(scope="module")
def ref_b():
    """case b's reference on the CPU (shared; never modified)"""
    return T.reference(T.BY_ID["b"], "cpu")


@pytest.mark.parametrize("cid", ["a", "b", "g"])
def test_recording_forward_is_the_oracles_bit_for_bit(cid):
    c = T.BY_ID[cid]
    p, x, _ = T.inputs(c)
    p64, x64 = {k: v.double() for k, v in p.items()}, x.double()
    rec = {}
    got = sm.generator_forward(x64, p64, c.R, record=rec)
    assert torch.equal(got, orc.generator_forward(x64, p64, n_rdb=c.R))
    assert list(rec) == sm.act_names(c.R)
    assert sum(z.numel() for z in rec.values()) == c.P * (2 * c.C + 4 * c.G * c.R) + 4 * c.P * c.C
    # a forced mask changes exactly that element's activation, to the other branch of the LeakyReLU
    z = rec["a0"].reshape(-1)
    i = int(z.abs().argmin())
    rec2 = {}
    sm.generator_forward(x64, p64, c.R, flips={"a0": [i]}, record=rec2)
    assert torch.equal(rec2["a0"], rec["a0"])
    d = (rec2["rdb0.conv1"] - rec["rdb0.conv1"]).abs().max().item()
    assert 0 < d <= abs(z[i].item()), (d, z[i].item())


@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_candidate_set_within_cap(case):
    """|S| <= 64 for every case, on the reference alone (the condition of the resolution: at most 64 extra float64 passes per case)"""
    p, x, _ = T.inputs(case)
    rec = {}
    sm.generator_forward(x.double(), {k: v.double() for k, v in p.items()}, case.R, record=rec)
    S = sm.candidates(rec, case.C, case.G)
    n = sum(z.numel() for z in rec.values())
    print(f"[smallmap] case {case.id}: |S| = {len(S)} of {n} activations")
    assert len(S) <= sm.CAP
    assert max(sm.bar_fwd(case.C, case.G), sm.bar_grad(case.C, case.G, case.N, case.H, case.W)) <= sm.MAX_BAR


def _fp32_grads(c, flips=None):
    p, x, Rw = T.inputs(c)
    return sm.run(x, p, Rw, c.R, flips=flips, dtype=torch.float32)[1]


def test_planted_flip_is_recovered(ref_b):
    """torch fp32's backward with one element of S forced to the other side: the resolver names exactly that element, and against the
    reference evaluated with that flip the remainder passes the bar"""
    c = T.BY_ID["b"]
    assert len(ref_b.S) >= 1, "case b's reference has no candidate: the planted-flip test needs one"
    plain = _fp32_grads(c)
    own = ref_b.resolve(plain)                              # the sides torch fp32 itself took
    for e in ref_b.S[:3]:
        got = _fp32_grads(c, flips={e[0]: [e[1]]})
        flipped, worst = ref_b.check_grads(got, f"planted {e}")
        assert set(flipped) == set(own) ^ {e}, (e, flipped, own)
        assert worst <= 1.0


def test_planted_errors_that_are_no_flips_are_rejected(ref_b):
    c = T.BY_ID["b"]
    good = _fp32_grads(c)
    ref_b.check_grads(good, "torch fp32")                   # (the unplanted result passes)
    k5 = "Generators.0.1.RDBs.1.conv5.weight"
    bad = dict(good)
    bad[k5] = good[k5].clone()
    bad[k5][32:64] = 0.0                                    # one 32-row block of a conv5 gradient zeroed
    with pytest.raises(AssertionError):
        ref_b.check_grads(bad, "zeroed row block")
    for k in ("Generators.0.2.0.weight", "Generators.0.1.RDBs.0.conv2.0.weight", "dx"):
        bad = dict(good)
        bad[k] = good[k] * (1.0 + 1e-4)                     # one gradient tensor scaled by 1 + 1e-4
        with pytest.raises(AssertionError):
            ref_b.check_grads(bad, f"scaled {k}")


def test_table_covers_the_schedule():
    """the case table names each of kinds 15, 16, 19 and 20, both tile forms of kind 20 (by the mirrored rule: wk6_tile_forms mirrors
    wk6_wide_candidate and the >= 128-tile rules of the launchers, it does not observe a launch), N = 2, a pixel tail, dx == NULL,
    hires_wk6 off, P > 3000 and channel counts that are no multiples of 32"""
    by = T.BY_ID
    assert [c.id for c in T.CASES] == ["a", "b", "b-nodx", "c", "d", "e", "f", "g", "h", "i", "j"]
    named = set().union(*[c.fwd | c.bwd for c in T.CASES])
    assert named >= {15, 16, 19, 20} and named <= T.FAMILY
    forms = {cid: sm.wk6_tile_forms(by[cid].C, by[cid].G, by[cid].R, by[cid].N, by[cid].H, by[cid].W) for cid in "abcd"}
    assert forms["c"]["group_wide"] == ["rdb0.step0"] and not forms["c"]["single_wide"]          # 26 x (4 + 1) = 130 tiles
    # the hi-res pair: 64 x 2 = 128 tiles; the conv-transpose's 4C = 512 columns: 16 x 8 = 128 tiles
    assert set(forms["d"]["single_wide"]) == {"convT", "final", "final.dgrad"} and not forms["d"]["group_wide"]
    for cid in "ab":
        assert not forms[cid]["single_wide"] and not forms[cid]["group_wide"], cid
        assert forms[cid]["single_narrow"] and forms[cid]["group_narrow"]
    assert any(c.N == 2 for c in T.CASES)
    assert by["b"].H * by["b"].W == 99 and 99 % 32 != 0                       # a pixel tile straddles the image boundary at pixel 99
    assert by["a"].P % 32 == 3 and by["c"].P % 32 == 25                         # pixel tails
    assert not by["b-nodx"].want_dx and by["b-nodx"].shape_key == by["b"].shape_key
    assert 1024 < by["e"].P <= 4096 and 4 * by["e"].P > 4096 and 15 in by["e"].fwd and 20 in by["e"].fwd       # hires_wk6 off, images on
    assert 3000 < by["f"].P <= 4096 and by["f"].dtype is None
    assert by["g"].C % 32 and by["g"].G % 32 and 20 not in (by["g"].fwd | by["g"].bwd)
    assert by["h"].dtype == "fp32" and by["h"].bwd == {15, 16} and by["i"].dtype == "bf16x6" and by["j"].options == {"deterministic": 1}
    for c in T.CASES:                                                         # images: exactly where the shapes and the arithmetic take them
        images = c.dtype != "fp32" and c.C % 32 == 0 and c.G % 32 == 0
        assert (20 in c.fwd) == images, c.id


def _wgrad_groups(c):
    """(pixels, 128x128 tiles) of the wide and (pixels, 32x128 tiles) of the narrow weight-gradient group of a grouped six-product backward,
    in the order csrc/nets.hip defers them: final conv, conv-transpose, trunk, per block (last first) conv5 + the packed growth gradient, head"""
    P, L, cd = c.P, c.C + 4 * c.G, lambda a, b: -(-a // b)
    probs = [(4 * P, c.C, c.C), (P, 4 * c.C, c.C), (P, c.C, c.C)]
    for _ in range(c.R):
        probs += [(P, c.C, L), (P, 4 * c.G, L)]
    probs.append((P, c.C, c.C))
    wide = [(p, cd(m, 128) * cd(n, 128) * 9) for p, m, n in probs if m > 32]
    narrow = [(p, cd(m, 32) * cd(n, 128) * 9) for p, m, n in probs if m <= 32]
    return wide, narrow


def _sk_plan(group):
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from afigan_amd import _lib
    lib = _lib.load()
    n, tiles = len(group), sum(t for _, t in group)
    px, tl = (ctypes.c_longlong * n)(*[p for p, _ in group]), (ctypes.c_int * n)(*[t for _, t in group])
    stored, added, stages = ((ctypes.c_int * tiles)() for _ in range(3))
    assert lib.afi_debug_wgrad_sk_plan(px, tl, n, 3, stored, added, stages) == 0
    return list(stored), list(added)


def test_stream_k_plans_of_cases_a_and_b():
    """What the table says of the weight-gradient tiles, from the kernel's own walk run on the host (afi_debug_wgrad_sk_plan): case a's
    wgrad_group6 tiles (2 stages each) are all stored whole by one run; case b's (7 and 25 stages, runs of 4) are all shared between runs
    and added by atomics."""
    wide_a, narrow_a = _wgrad_groups(T.BY_ID["a"])
    assert len(wide_a) == 2 and len(narrow_a) == 4          # C = 32: only the conv-transpose and the packed growth gradient have > 32 rows
    stored, added = _sk_plan(wide_a)
    assert all(s == 1 for s in stored) and not any(added)
    wide_b, narrow_b = _wgrad_groups(T.BY_ID["b"])
    assert len(wide_b) == 8 and not narrow_b
    stored, added = _sk_plan(wide_b)
    assert not any(stored) and all(a >= 2 for a in added)
