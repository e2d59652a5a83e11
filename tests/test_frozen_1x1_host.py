"""The host plan of afi_conv1x1_frozen_fwd (csrc/frozen1x1.hip: afi_frozen1x1_plan, pure host code) without a device: eligibility exactly
where the header says, every output row and column covered by exactly one (block, wave, n half), the grid and the LDS within the limits of a
launch, every byte offset the kernel forms inside the extent its buffer descriptor is given, and the image size the builder writes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT = 0x7FFFFFF0
STAGE_BYTES = 6144                    # AFI_WK6_STAGE_BYTES: one (32 columns, 32 channels) unit of the image


def _ops():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from afigan_amd import ops
    return ops


def _dense(N, H, W, C):
    return (H * W * C, W * C, C)


def _s2(N, H, W, C, Hf=None, Wf=None):
    """every second pixel of a dense [N][Hf][Wf][C] map"""
    Hf, Wf = Hf or 2 * H, Wf or 2 * W
    return (Hf * Wf * C, 2 * Wf * C, 2 * C)


def _guide_shapes(Himg, Wimg, N=2):
    """(N, H, W, Cin, Cout, x strides, has_add) of every 1x1 conv of GuideR50FPN on an N x 3 x Himg x Wimg batch (padded to a multiple of 32)"""
    H, W = -(-Himg // 32) * 32 // 4, -(-Wimg // 32) * 32 // 4
    out = []
    cfg = [(64, 64, 256, 3, 1), (256, 128, 512, 4, 2), (512, 256, 1024, 6, 2), (1024, 512, 2048, 3, 2)]
    for cin, mid, cout, n, stride in cfg:
        Ho, Wo = H // stride, W // stride
        xs = _dense(N, H, W, cin) if stride == 1 else _s2(N, Ho, Wo, cin, H, W)
        out.append((N, Ho, Wo, cin, mid, xs, False))                        # first block: c1 (strided), shortcut (strided), c3 with the addend
        out.append((N, Ho, Wo, cin, cout, xs, False))
        out.append((N, Ho, Wo, mid, cout, _dense(N, Ho, Wo, mid), True))
        for _ in range(n - 1):
            out.append((N, Ho, Wo, cout, mid, _dense(N, Ho, Wo, cout), False))
            out.append((N, Ho, Wo, mid, cout, _dense(N, Ho, Wo, mid), True))
        out.append((N, Ho, Wo, cout, 256, _dense(N, Ho, Wo, cout), cout != 2048))   # lateral (top-down addend below the top level)
        H, W = Ho, Wo
    return out


def _check_plan(ops, N, H, W, Cin, Cout, xs, has_add):
    """the kernel's own index math (csrc/frozen1x1.hip) replayed on the host for one plan"""
    add = _dense(N, H, W, Cout) if has_add else None
    p = ops.conv1x1_frozen_plan(N, H, W, Cin, Cout, xs, add_strides=add)
    assert p is not None, (N, H, W, Cin, Cout, xs)
    M = N * H * W
    assert p["M"] == M and p["BM"] == 64 and p["BN"] in (64, 128, 256) and p["KC"] in (32, 64, 128) and Cin % p["KC"] == 0
    assert p["ntile_m"] == -(-M // 64) and p["ntile_n"] == -(-Cout // p["BN"]) and p["grid"] == p["ntile_m"] * p["ntile_n"]
    assert 1 <= p["grid"] < 2 ** 31 and p["lds_bytes"] == 3 * 64 * p["KC"] * 2 <= 64 * 1024
    assert p["image_bytes"] == Cout * Cin * 6 == ops._lib.load().afi_frozen1x1_image_bytes(Cout, Cin)
    assert p["out_bytes"] == M * Cout * 4 < LIMIT and p["x_bytes"] < LIMIT
    # rows: tile t covers [64 t, 64 t + 64) below M; columns: (column tile, wave, j) -> n half (tile * 4 + wave) * NJ + j, 16 columns each
    nj = p["BN"] // 64
    halves = [(tn * 4 + w) * nj + j for tn in range(p["ntile_n"]) for w in range(4) for j in range(nj)]
    valid = [h for h in halves if h * 16 < Cout]
    assert sorted(valid) == list(range(Cout // 16)) and len(set(halves)) == len(halves)
    assert (p["ntile_m"] - 1) * 64 < M <= p["ntile_m"] * 64
    # the largest byte offsets: x (last row, last chunk, last 16 bytes), out / add (last row, last four columns), image (last half, last stage, lo part, lane 63)
    sN, sH, sW = xs
    dense = sH == W * sW and sN == H * sH
    assert p["x_dense"] == int(dense)
    last_row = (M - 1) * sW if dense else (N - 1) * sN + (H - 1) * sH + (W - 1) * sW
    assert 4 * last_row + 4 * (Cin - 4) + 16 <= p["x_bytes"]
    assert 4 * ((M - 1) * Cout + Cout - 4) + 16 <= p["out_bytes"]
    h = Cout // 16 - 1
    assert ((h >> 1) * (Cin // 32) + Cin // 32 - 1) * STAGE_BYTES + 3 * (h & 1) * 1024 + 2 * 1024 + 16 * 63 + 16 <= p["image_bytes"]
    return p


def test_plan_over_the_benchmarks_guide_shapes():
    """both image sizes of a stage-1 step (2 x 3 x 800 x 1333 and its half), every stage, the stride-2 views"""
    ops = _ops()
    seen = set()
    for Himg, Wimg in ((800, 1333), (400, 667)):
        for N, H, W, Cin, Cout, xs, has_add in _guide_shapes(Himg, Wimg):
            p = _check_plan(ops, N, H, W, Cin, Cout, xs, has_add)
            seen.add((p["BN"], p["KC"], p["x_dense"]))
    assert {bn for bn, _, _ in seen} == {64, 128, 256} and {kc for _, kc, _ in seen} == {64, 128} and {d for _, _, d in seen} == {0, 1}


def test_plan_degenerate_shapes():
    ops = _ops()
    for N, H, W, Cin, Cout in ((1, 1, 1, 32, 32), (1, 1, 1, 2048, 2048), (1, 1, 65, 32, 96), (3, 7, 1, 96, 32), (1, 64, 1, 160, 288)):
        _check_plan(ops, N, H, W, Cin, Cout, _dense(N, H, W, Cin), False)
        _check_plan(ops, N, H, W, Cin, Cout, _dense(N, H, W, Cin), True)
    _check_plan(ops, 2, 37, 41, 64, 128, _s2(2, 37, 41, 64, 73, 82), False)           # odd full height
    _check_plan(ops, 2, 5, 6, 32, 32, (7 * 9 * 32 + 64, 9 * 32, 32), False)            # a crop of a larger map, images further apart


def test_plan_refuses_exactly_what_the_header_says():
    ops = _ops()
    ok = lambda *a, **k: ops.conv1x1_frozen_plan(*a, **k) is not None
    d = _dense(1, 9, 9, 64)
    assert ok(1, 9, 9, 64, 64, d)
    assert not ok(1, 9, 9, 36, 64, _dense(1, 9, 9, 36)) and not ok(1, 9, 9, 64, 48, d) and not ok(1, 9, 9, 16, 64, _dense(1, 9, 9, 16))
    assert not ok(1, 9, 9, 32, 64, d)                                                  # a channel slice: 32 of 64 channels
    assert not ok(1, 9, 9, 64, 64, (9 * 9 * 64 + 2, 9 * 64, 64))                      # strides that break the 16-byte loads
    assert not ok(1, 9, 9, 64, 64, d, out_strides=(9 * 9 * 128, 9 * 128, 128))        # out is not dense
    assert not ok(1, 9, 9, 64, 64, d, add_strides=(9 * 9 * 128, 9 * 128, 128))        # add is not dense
    assert ok(1, 9, 9, 64, 64, d, add_strides=_dense(1, 9, 9, 64))
    assert not ok(1, 9, 9, 64, 64, (9 * 9 * 64, 8 * 64, 64))                          # rows that overlap
    import pytest
    with pytest.raises(ops._lib.AfiError):
        ops.conv1x1_frozen_plan(0, 9, 9, 64, 64, d)
    assert ops._lib.load().afi_frozen1x1_image_bytes(48, 64) == 0


def test_plan_at_the_2gb_boundary():
    """x, out and the image: the largest extent below 2 GB is taken, the next one refused"""
    ops = _ops()
    ok = lambda *a, **k: ops.conv1x1_frozen_plan(*a, **k) is not None
    # out: M * Cout * 4 against 0x7FFFFFF0
    W = LIMIT // (4 * 2048)                                                            # 262143: 2048 W 4 = LIMIT - 8176
    assert ok(1, 1, W, 32, 2048, _dense(1, 1, W, 32)) and not ok(1, 1, W + 1, 32, 2048, _dense(1, 1, W + 1, 32))
    _check_plan(ops, 1, 1, W, 32, 2048, _dense(1, 1, W, 32), True)
    # x: a far-apart pair of images
    gap = (LIMIT - 4 * 64 * 81) // 4 // 4 * 4
    assert ok(2, 9, 9, 64, 64, (gap - 4, 9 * 64, 64)) and not ok(2, 9, 9, 64, 64, (gap + 64, 9 * 64, 64))
    _check_plan(ops, 2, 9, 9, 64, 64, (gap - 4, 9 * 64, 64), False)
    # the image: Cout * Cin * 6
    assert ok(1, 1, 1, 8192, 32768, _dense(1, 1, 1, 8192)) and not ok(1, 1, 1, 16384, 32768, _dense(1, 1, 1, 16384))
