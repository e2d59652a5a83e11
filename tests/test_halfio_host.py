"""CPU-side checks of the 2-byte boundary (no GPU): the new C-ABI entry points refuse an unknown storage dtype before anything else, and
the Python boundary helpers decide the storage dtype in one place."""
import pytest
import torch


def _lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from afigan_amd import _lib
    return _lib, _lib.load()


def test_store_dtype_codes_match_the_header():
    import os
    import re
    from afigan_amd import ops
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "afigan_hip.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define AFI_STORE_(\w+) (\d+)", hdr)}
    assert codes == {"F32": 0, "BF16": 1, "F16": 2}
    assert ops.STORE_DTYPES == {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def test_new_entry_points_refuse_unknown_storage_dtypes():
    """An unknown storage dtype is AFI_ERR_BAD_ARG (1), decided before anything else: every buffer here is NULL, so nothing could be
    launched on it.  No context (NULL): the library's defaults, nothing device-side is created.  (The beta != 0 refusal of a 2-byte output
    is checked on real device buffers, tests/test_gpu_halfio.py::test_2byte_epilogue_refuses_reading_its_output.)"""
    L, lib = _lib()
    v = L.View(None, 64 * 32, 8 * 32, 32)
    for bad in (0, 3, -1):                                   # the fp32 store has its own entry points; nothing else exists
        assert lib.afi_conv3x3_fwd_out16(None, v, 1, 8, 8, 32, None, None, 32, v, bad, 1.0, 0.0, 0, None) == 1
        assert lib.afi_conv1x1_dgrad_out16(None, v, 1, 8, 8, 32, None, 32, v, bad, 1.0, 0.0, None) == 1
        assert lib.afi_conv3x3_wino_fwd_out16(None, v, 1, 8, 8, 32, None, None, 32, v, bad, None, 0, None) == 1
        assert lib.afi_generator_fwd_out16(None, None, v, 1, 8, 8, v, bad, None, 0, None) == 1
        assert lib.afi_cast_to_f32_nhwc(None, bad + 4, 1, 4, 2, 2, 16, 4, 8, 1, None, None) == 1
        assert lib.afi_cast_from_f32_nhwc(v, 1, 8, 8, 32, None, bad, None) == 1


def test_boundary_dtype_is_decided_in_one_place():
    from afigan_amd import _lib, ops
    with pytest.raises(_lib.AfiError, match="GPU only"):
        ops.boundary_dtype(torch.zeros(1, 4, 2, 2, dtype=torch.bfloat16))
    with pytest.raises(_lib.AfiError, match="GPU only"):
        ops.ingest(torch.zeros(1, 4, 2, 2, dtype=torch.float16))
    with pytest.raises(_lib.AfiError, match="fp32 only"):               # the per-op check is unchanged: 2-byte tensors enter only here
        ops._check_cuda(_FakeCuda())


class _FakeCuda:                                                        # (a GPU tensor's attributes, on a machine without one)
    is_cuda = True
    dtype = torch.bfloat16
