"""CPU: the C-ABI shared library loads and exports every symbol include/r3d_hip.h declares; argument
validation (which runs before any HIP call) reports errors through return codes + r3d_last_error."""
import ctypes
import os
import re
import subprocess

import pytest

from abi import C_RETURNS, HEADERS, entry_matches, header_constants, header_declarations, header_source
from conftest import ROOT

COMPANIONS = [h for h in HEADERS if h != "r3d_hip.h"]
# the constants of each header that real3dportrait_amd/_lib.py mirrors, by _lib's name: _lib.X is R3D_X.  Listed here, so that a constant
# deleted from _lib (or from its header) fails test_constants_mirror_the_headers
MIRRORED = {"r3d_hip.h": ["CHAIN_SR_BLOCK", "CHAIN_CONV", "CHAIN_SR_BLOCK_TAIL", "CHAIN_SRC_NONE", "CHAIN_MAX_OPS", "CHAIN_MAX_EXT", "CHAIN_MAX_ZERO"],
            "r3d_hip_clip.h": [],
            "r3d_hip_video.h": ["VIDEO_STATE_WORDS", "VIDEO_PANELS_ALL", "VIDEO_PANEL_DEPTH"],
            "r3d_hip_source.h": ["SOURCE_MAX_SIDE", "SOURCE_STATUS_WORDS", "SOURCE_DARKEN", "SOURCE_HEAD_CLASSES"],
            "r3d_hip_audio.h": ["A2M_WN_ROWS"],
            "r3d_hip_fit.h": ["FIT_LOSS_WORDS", "FIT_LAUNCHES"]}
LLVM = "/opt/rocm/lib/llvm/bin"          # csrc/Makefile's LLVM


def declared_symbols():
    return sorted(set(s for h in HEADERS for s in re.findall(r"\b(r3d_[a-z0-9_]+)\s*\(", header_source(h))))


def test_every_declared_symbol_is_exported_and_bound():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    syms = declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), "libr3d_hip.so does not export %s" % s
        assert s in _lib.SIGNATURES, "python binding table misses %s" % s
    assert set(_lib.SIGNATURES) == set(syms)


def test_table_mirrors_every_header_declaration():
    """Every declaration of include/r3d_hip.h and of the five companion headers it includes (each exactly once) -- 92 in all -- is bound
    in the one table with the same parameter count, the exact ctypes type of every scalar, the header's element type of every pointer
    (device pointers by their marker, host pointers by their ctypes.POINTER) and the same return type; the stream is the last parameter
    and no other (and every status-returning entry point of a companion header has one); and load() derives each function's argtypes and
    call()'s plan from that line."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    per_header = {h: header_declarations(h) for h in HEADERS}
    assert {h: len(d) for h, d in per_header.items()} == HEADERS and len(HEADERS) == 6 and sum(HEADERS.values()) == 92
    main = open(os.path.join(ROOT, "include", "r3d_hip.h")).read()
    assert len(COMPANIONS) == 5 and re.findall(r'#include "(\w+\.h)"', main) == COMPANIONS
    decls = {}
    for h, d in per_header.items():
        assert h == "r3d_hip.h" or main.count('#include "%s"' % h) == 1, h
        assert not set(d) & (set(decls) | set(_lib.OPTIONAL_SIGNATURES)), h
        decls.update(d)
    assert set(decls) == set(_lib.SIGNATURES) == set(declared_symbols()) and len(decls) == 92
    for name, (ret, types) in decls.items():
        res, entries = _lib.SIGNATURES[name]
        assert res is C_RETURNS[ret], (name, ret, res)
        assert len(entries) == len(types), (name, len(entries), len(types))
        for i, (e, t) in enumerate(zip(entries, types)):
            assert entry_matches(e, t, _lib), "%s: parameter %d is %s in the header, %r in the table" % (name, i, t, e)
        assert all(isinstance(e, _lib.Stream) is (i == len(entries) - 1) for i, e in enumerate(entries) if isinstance(e, _lib.Stream)), name
        if name not in per_header["r3d_hip.h"] and res is ctypes.c_int:
            assert isinstance(entries[-1], _lib.Stream), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == [getattr(e, "ctype", e) for e in entries], name
        assert name in _lib._plans, name
    assert _lib.F.ctype is ctypes.c_void_p and _lib.S.ctype is ctypes.c_void_p


def test_abi_number_is_pinned_once():
    """The ABI number: the library's, the package's and this literal agree, and csrc/r3d_api.hip holds the one definition (functions are
    added without a new number: the per-unit host tests compare the first two and leave the literal to this test)."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION == 80
    csrc = os.path.join(ROOT, "real3dportrait_amd", "csrc")
    defs = {f: re.findall(r"\bint\s+r3d_version\s*\(\s*(?:void)?\s*\)\s*\{([^}]*)\}", open(os.path.join(csrc, f)).read())
            for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    assert {f: [b.strip() for b in d] for f, d in defs.items() if d} == {"r3d_api.hip": ["return 80;"]}


def test_constants_mirror_the_headers():
    """_lib.X mirrors R3D_X: every constant of a header that _lib holds under that name has the header's value, every name of MIRRORED is
    in both, and a companion header defines no constant that _lib does not mirror."""
    from real3dportrait_amd import _lib
    assert set(MIRRORED) == set(HEADERS) and [len(MIRRORED[h]) for h in HEADERS] == [7, 0, 3, 4, 1, 2]
    for h in HEADERS:
        consts = header_constants(h)
        for name in MIRRORED[h]:
            assert "R3D_" + name in consts, "%s does not define R3D_%s" % (h, name)
            assert hasattr(_lib, name), "_lib.%s (R3D_%s of %s) is gone" % (name, name, h)
        for rname, value in consts.items():
            if hasattr(_lib, rname[4:]):
                assert getattr(_lib, rname[4:]) == value and type(getattr(_lib, rname[4:])) is int, (h, rname, value)
                assert rname[4:] in MIRRORED[h], "_lib.%s mirrors %s of %s: list it in MIRRORED" % (rname[4:], rname, h)
        if h != "r3d_hip.h":
            assert set(consts) == {"R3D_" + n for n in MIRRORED[h]}, h
    main = header_constants("r3d_hip.h")
    assert main["R3D_CHAIN_SRC_NONE"] == -1000 and main["R3D_ERR_WORKSPACE"] == -2 and main["R3D_PROF_COUNT"] == 7 and len(main) >= 25


@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_headers_stand_alone(lang, tmp_path):
    """Each of the six headers compiles as the only line of a translation unit, as C99 and as C++17 (-Wall -Werror, host only), and so do
    all six in the reverse of the order r3d_hip.h includes them in."""
    clang = os.path.join(LLVM, "clang")
    if not os.path.exists(clang):
        pytest.skip("no %s: the headers are not compiled here" % clang)
    flags = ["-x", "c", "-std=c99"] if lang == "c99" else ["-x", "c++", "-std=c++17"]
    units = [[h] for h in HEADERS] + [list(HEADERS)[::-1]]
    for i, unit in enumerate(units):
        src = tmp_path / ("unit%d.%s" % (i, "c" if lang == "c99" else "cpp"))
        src.write_text("".join('#include "%s"\n' % h for h in unit))
        r = subprocess.run([clang] + flags + ["-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, "%s as %s:\n%s" % (" + ".join(unit), lang, r.stderr)


def test_debug_twins_extend_their_product_function():
    """An OPTIONAL_SIGNATURES twin of a product function takes the product's parameters, then the documented extras, then the stream."""
    from real3dportrait_amd import _lib
    extras = {"r3d_debug_raster_forward": ("r3d_raster_forward", [ctypes.c_int, ctypes.c_int]),          # large-face threshold, stage mask
              "r3d_debug_secc_blink": ("r3d_secc_blink", [ctypes.c_int])}                                 # stage mask
    plans = {"r3d_debug_fit_plan", "r3d_debug_face_plan"}                                                 # host arithmetic, no product twin
    assert set(_lib.OPTIONAL_SIGNATURES) == set(extras) | {"r3d_debug_merge_fallbacks"} | plans
    for name in plans:
        assert name not in header_declarations()
        assert _lib.OPTIONAL_SIGNATURES[name] == (ctypes.c_int, [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int32)]), name
    header = header_declarations()
    for twin, (product, extra) in extras.items():
        assert twin not in header
        (res, got), (pres, want) = _lib.OPTIONAL_SIGNATURES[twin], _lib.SIGNATURES[product]
        assert res is pres and isinstance(want[-1], _lib.Stream)
        assert got[:len(want) - 1] == want[:-1] and got[len(want) - 1:-1] == extra and got[-1] is want[-1], twin
    assert _lib.OPTIONAL_SIGNATURES["r3d_debug_merge_fallbacks"] == (ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int])


def test_version_and_sizes():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    assert lib.r3d_version() >= 10
    assert lib.r3d_render_workspace_bytes(1, 16384, 48, 48) >= 2 * 16384 * 4
    assert lib.r3d_sr_block_prepacked_bytes(32, 256) == (4 * 9 * 32 * 256 + 9 * 256 * 256 + 4 * 256 + 12 * 256 * 256) * 4   # conv0 in four layouts (plain, up, up with fp8 records, plain with fp8 records) + conv1 + 2 weight-row tails + conv1's 12 Winograd F(2,3) tap matrices
    assert lib.r3d_conv_prepacked_bytes(3, 64, 3) == (2 * 9 * 16 * 128 + 2 * 128 + 12 * 16 * 128) * 4        # padded to 16 x 128, twice (the f16x3 layout and, for 3x3 convs, the layout with fp8 records) + tail + (3x3) the 12 Winograd tap matrices
    assert lib.r3d_conv_scales_bytes(2, 3, 64) >= 2 * (16 + 128 + 3) * 4
    assert lib.r3d_sr_block_bound_offset(32, 256) * 4 < lib.r3d_sr_block_styles_bytes(1, 32, 256)
    assert lib.r3d_sr_block_styles_bytes(2, 32, 256) > 2 * (32 + 4 * 256) * 4
    assert lib.r3d_sr_block_workspace_bytes(1, 32, 256, 128, 128) > 256 * 257 * 257 * 4


def test_pack_and_workspace_sizes_are_pinned():
    """The sizes SrPackLayout / ConvPackLayout / SrWorkspaceLayout (csrc/r3d_sr_common.h) add up to, at shapes that pad both channel counts and
    have every region; the numbers are those of the library before the layouts were named (formulas in the comments)."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    assert lib.r3d_sr_block_prepacked_bytes(16, 128) == 1673216          # (4 * 9 * 16 * 128 + 9 * 128^2 + 2 * 2 * 128 + 12 * 128^2) * 4
    assert lib.r3d_conv_prepacked_bytes(65, 3, 1) == 41984               # 1x1, padded to 80 x 128: (80 * 128 + 2 * 128) * 4
    assert lib.r3d_conv_prepacked_bytes(20, 132, 3) == 985088            # padded to 32 x 256: (2 * 9 * 32 * 256 + 2 * 256 + 12 * 32 * 256) * 4
    assert lib.r3d_sr_block_workspace_bytes(1, 16, 128, 8, 8) == 438272  # xin 4096 + T 165888 + y0 131072 + xo 131072 + rgbp 6144
    assert lib.r3d_sr_block_workspace_bytes(2, 16, 128, 5, 7) == 494848  # every slot rounded up to 256 bytes: 4608 + 196608 + 2 * 143360 + 6912
    assert lib.r3d_conv_scales_bytes(1, 65, 3) == 848 and lib.r3d_conv_scales_bytes(2, 65, 3) == 1696        # (80 + 128 + 4) * 4 per sample
    assert lib.r3d_conv_scales_bytes(1, 20, 132) == 1168 and lib.r3d_conv_scales_bytes(3, 20, 132) == 3504   # (32 + 256 + 4) * 4
    assert lib.r3d_conv_scales_bound_offset(65, 3) == 209 and lib.r3d_conv_scales_bound_offset(20, 132) == 289
    assert lib.r3d_conv_workspace_bytes(1, 17, 5, 7) == 4864             # Cin padded to 32: 32 * 35 * 4 rounded up to 256, + 256


def test_argument_errors_are_reported_not_thrown():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    rc = lib.r3d_raygen(None, None, 1, 16, None, None, None)
    assert rc == -1 and b"raygen" in lib.r3d_last_error()
    one = ctypes.c_void_p(64)      # never dereferenced: validation fails first
    rc = lib.r3d_render_forward(one, 1, 32, 32, 1, one, one, one, one, one, one, 256, 200, 0, 1.0, 0, None, None, 0,
                                one, 0, one, one, one, None, 0, None, None, None, None, 0, one, 1 << 20, None)
    assert rc == -1 and b"depth_resolution" in lib.r3d_last_error()
    rc = lib.r3d_render_forward(one, 1, 32, 32, 1, one, one, one, one, one, one, 256, 48, 48, 1.0, 0, None, None, 0,
                                one, 1, None, one, one, None, 0, None, None, None, None, 0, one, 8, None)
    assert rc == -2 and b"workspace" in lib.r3d_last_error()
    rc = lib.r3d_render_forward(one, 1, 32, 32, 1, one, one, one, one, None, None, 250, 48, 48, 1.0, 0, None, None, 0,
                                one, 1, None, one, one, None, 0, one, one, None, None, 0, one, 1 << 20, None)
    assert rc == -1 and b"camera mode" in lib.r3d_last_error()       # camera mode needs a square ray count
    rc = lib.r3d_render_forward(one, 1, 32, 32, 1, one, one, one, one, None, None, 256, 48, 48, 1.0, 0, None, None, 0,
                                one, 1, None, one, one, None, 0, None, None, None, None, 0, one, 1 << 20, None)
    assert rc == -1 and b"NULL pointer" in lib.r3d_last_error()      # neither rays nor a camera
    rc = lib.r3d_render_forward(one, 1, 32, 32, 1, one, one, one, one, one, one, 256, 48, 48, 1.0, 0, None, None, 0,
                                one, 1, None, one, one, None, 0, None, None, one, None, 0, one, 1 << 20, None)
    assert rc == -1 and b"split_scale" in lib.r3d_last_error()
    rc = lib.r3d_run_model(one, 1, 32, 32, 1, one, one, one, one, one, 16, 1.0, one, one, None, 0, one, 8, None)
    assert rc == -2 and b"workspace" in lib.r3d_last_error()
    n = ctypes.c_int(0)
    rc = lib.r3d_planes_to_nhwc(one, None, one, 1, 32, 8, 8, 1, 0, one, None, None)
    assert rc == -1 and b"n_partials" in lib.r3d_last_error()
    assert lib.r3d_planes_absmax_partials(1, 32, 256, 256, 1) >= 3 * 256 * 256 // 64
    rc = lib.r3d_sr_block_prepack(30, 256, one, one, one, 1, None)
    assert rc == -1 and b"multiple of 8" in lib.r3d_last_error()
    rc2 = lib.r3d_sr_block_forward(one, one, 1, 32, 256, 16, 16, 1, one, 2, one, -1.0, None, -1, None, 0, one, None, None, 0, one, 1 << 40, None)
    assert rc2 == -1 and b"format" in lib.r3d_last_error()      # SPLIT input needs the f16x3 precision
    rc2 = lib.r3d_sr_block_forward(one, one, 1, 32, 256, 16, 16, 0, one, 0, one, -1.0, None, -1, None, 0, one, None, None, 0, one, 1 << 40, None)
    assert rc2 == -1 and b"up=0" in lib.r3d_last_error()        # SynthesisBlockNoUp is f16x3 only
    rc2 = lib.r3d_sr_block_forward(one, one, 1, 32, 256, 16, 16, 1, one, 0, one, -1.0, None, -1, None, 0, one, one, None, 0, one, 1 << 40, None)
    assert rc2 == -1 and b"uint8" in lib.r3d_last_error()       # the fused uint8 output is f16x3 only
    rc2 = lib.r3d_conv_forward(one, one, None, 1, 64, 30, 16, 16, 3, one, 0, 0, 0.0, 1.0, -1.0, one, 0, None, 0, None, one, 1 << 40, None)
    assert rc2 == -1 and b"multiple of 4" in lib.r3d_last_error()
    rc2 = lib.r3d_conv_forward(one, one, None, 1, 64, 32, 16, 16, 5, one, 0, 0, 0.0, 1.0, -1.0, one, 0, None, 0, None, one, 1 << 40, None)
    assert rc2 == -1 and b"bad argument" in lib.r3d_last_error()
    rc2 = lib.r3d_conv_forward(one, one, None, 1, 64, 32, 16, 16, 3, one, 0, 0, 0.0, 1.0, -1.0, one, 0, None, 0, None, one, 8, None)
    assert rc2 == -2 and b"workspace" in lib.r3d_last_error()
    # the round-6 entry points: the fused blend conv and the conv that writes one part of a concatenation
    rc2 = lib.r3d_conv_forward_blend(one, one, None, 1, 8, 40, 64, 4, 4, one, one, one, 0, 0.0, 1.0, -1.0, one, 0, None, 0, None, None)
    assert rc2 == -1 and b"multiple of 64" in lib.r3d_last_error()
    rc2 = lib.r3d_conv_forward_blend(one, one, None, 1, 32, 32, 64, 4, 4, one, None, one, 0, 0.0, 1.0, -1.0, one, 0, None, 0, None, None)
    assert rc2 == -1 and b"bad argument" in lib.r3d_last_error()
    rc2 = lib.r3d_conv_forward_blend(one, one, None, 1, 32, 32, 24, 4, 4, one, one, one, 0, 0.0, 1.0, -1.0, one, 3, None, 0, None, None)
    assert rc2 == -1 and b"unsupported output" in lib.r3d_last_error()        # SPLIT_MX needs Cout % 16 == 0
    rc2 = lib.r3d_conv_forward_cat(one, one, None, 1, 64, 256, 16, 16, 3, one, 0, 0, 0.0, 1.0, -1.0, one, 2, 512, 256, one, 1, None, 0, one, 1 << 40, None)
    assert rc2 == -1 and b"1x1" in lib.r3d_last_error()
    rc2 = lib.r3d_conv_forward_cat(one, one, None, 1, 64, 256, 16, 16, 1, one, 0, 0, 0.0, 1.0, -1.0, one, 2, 512, 264, one, 1, None, 0, one, 1 << 40, None)
    assert rc2 == -1 and b"multiples of 16" in lib.r3d_last_error()
    rc2 = lib.r3d_conv_forward_cat(one, one, None, 1, 64, 256, 16, 16, 1, one, 0, 0, 0.0, 1.0, -1.0, one, 0, 512, 256, one, 1, None, 0, one, 1 << 40, None)
    assert rc2 == -1 and b"SPLIT" in lib.r3d_last_error()                     # the concatenated operand is SPLIT or SPLIT_MX
    rc2 = lib.r3d_conv_forward_cat(one, one, None, 1, 64, 256, 16, 16, 1, one, 0, 0, 0.0, 1.0, -1.0, one, 2, 512, 256, one, 1, None, 0, one, 8, None)
    assert rc2 == -2 and b"workspace" in lib.r3d_last_error()
    rc2 = lib.r3d_blend_cat_to_split(one, 1, 8, None, 1, 8, one, 1, 4, 4, one, 2, None, 0, None)
    assert rc2 == -1 and b"b = NULL" in lib.r3d_last_error()                  # writing only the `a` part needs whole 16-channel record groups
    # chain fold: a layer may only read the bound of an EARLIER op or of an external slot that exists
    op = _lib.ChainOp(kind=_lib.CHAIN_CONV, Cin=16, Cout=128, ksize=3, act=0, gain=1.0, clamp=-1.0, src_a=0, src_b=_lib.CHAIN_SRC_NONE,
                      scales=64, prepacked=64, bias=None)
    arr = (_lib.ChainOp * 1)(op)
    rc2 = lib.r3d_chain_fold(ctypes.cast(arr, ctypes.c_void_p), 1, 1, None, 0, None, 0, None)
    assert rc2 == -1 and b"bound source" in lib.r3d_last_error()
    arr[0].src_a = -1
    rc2 = lib.r3d_chain_fold(ctypes.cast(arr, ctypes.c_void_p), 1, 1, None, 0, None, 0, None)
    assert rc2 == -1 and b"bound source" in lib.r3d_last_error()
    rc2 = lib.r3d_absmax(None, 16, 1, one, None, None)
    assert rc2 == -1 and b"absmax" in lib.r3d_last_error()
    rc = lib.r3d_sr_block_prepack(30, 256, one, one, one, 1, None)
    try:
        _lib.check(rc, "prepack")
        assert False
    except RuntimeError as e:
        assert "multiple of 8" in str(e)


def test_sr_resampling_and_image_op_argument_errors():
    """The small kernels around the SR convs refuse what they do not cover before any launch (tests/test_gpu_sr_ops.py runs them)."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)      # never dereferenced: validation fails first
    CB8, SPLIT, SPLIT_MX = 1, 2, 3
    rc = lib.r3d_upsample2x_bilinear(one, 1, 12, 4, 4, one, CB8, None, 0, None)
    assert rc == -1 and b"multiple of 8" in lib.r3d_last_error()
    rc = lib.r3d_upsample2x_bilinear(one, 1, 16, 4, 4, one, 0, None, 0, None)
    assert rc == -1 and b"y_format" in lib.r3d_last_error()                    # NCHW is not an output format of this kernel
    rc = lib.r3d_upsample2x_bilinear(one, 1, 16, 4, 4, one, 4, None, 0, None)
    assert rc == -1 and b"y_format" in lib.r3d_last_error()
    rc = lib.r3d_upsample2x_bilinear(one, 1, 24, 4, 4, one, SPLIT_MX, None, 0, None)
    assert rc == -1 and b"SPLIT_MX needs C % 16" in lib.r3d_last_error()      # whole 16-channel record groups
    assert lib.r3d_upsample2x_bilinear(None, 1, 16, 4, 4, one, SPLIT, None, 0, None) == -1 and b"upsample2x_bilinear" in lib.r3d_last_error()
    assert lib.r3d_upsample2x_bilinear(one, 1, 16, 4, 4, None, SPLIT, None, 0, None) == -1 and b"upsample2x_bilinear" in lib.r3d_last_error()
    assert lib.r3d_upsample2x_bilinear(one, 1, 16, 0, 4, one, CB8, None, 0, None) == -1
    for args in ((0, 4, 4, 2, 2), (1, 0, 4, 2, 2), (1, 4, 0, 2, 2), (1, 4, 4, 0, 2), (1, 4, 4, 2, 0)):          # planes, H, W, OH, OW
        rc = lib.r3d_resize_bilinear(one, args[0], args[1], args[2], one, args[3], args[4], 1, None)
        assert rc == -1 and b"resize_bilinear" in lib.r3d_last_error(), args
    assert lib.r3d_resize_bilinear(None, 1, 4, 4, one, 2, 2, 0, None) == -1
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):       # a, b, mask, out
        rc = lib.r3d_blend(args[0], args[1], args[2], 1, 3, 4, 4, args[3], None)
        assert rc == -1 and b"blend" in lib.r3d_last_error()
    assert lib.r3d_blend(one, one, one, 1, 0, 4, 4, one, None) == -1
    rc = lib.r3d_person_occlusion(one, one, 0.5, 0, one, None)
    assert rc == -1 and b"person_occlusion" in lib.r3d_last_error()
    assert lib.r3d_person_occlusion(one, None, 0.5, 16, one, None) == -1


def test_torso_conv_argument_errors():
    """What the seven torso conv entry points refuse before any launch: rc -1 and a message with the entry point's name (the _prec
    variants report the base name) and the rule.  Every call has exactly one defect; the pointers are fake, 1 TiB apart and never
    dereferenced.  Rejected calls only: a valid one would launch (tests/test_gpu_torso_*_ops.py run those)."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    X, W, BIAS, Y, YN, PS, PT, RES = (i << 40 for i in range(1, 9))
    base = dict(x=X, B=1, D=2, Hs=4, Ws=4, Cin=8, in_nchw=0, up=0, ps=None, pt=None, w=W, bias=BIAS, Cout=8, k=3, full=0, act=1, pool=0,
                depth=1, res=None, y=Y, ycs=None, yco=0, yn=None, prec=0)

    def call(fn, **over):
        a = dict(base, **over)
        ycs = a["Cout"] if a["ycs"] is None else a["ycs"]
        conv = (a["x"], a["B"], a["Hs"], a["Ws"], a["Cin"], a["in_nchw"], a["up"], a["ps"], a["pt"], 0.0, a["w"], a["bias"], a["Cout"], a["k"],
                a["act"], 0.0, a["res"], a["y"], a["yn"])
        conv3d = (a["x"], a["B"], a["D"], a["Hs"], a["Ws"], a["Cin"], a["up"], a["w"], a["bias"], a["Cout"], a["k"], a["full"], a["act"], 0.0,
                  a["pool"], a["y"], ycs, a["yco"], a["yn"])
        flat = (a["x"], a["B"], a["Hs"], a["Ws"], a["Cin"], a["in_nchw"], a["w"], a["bias"], a["Cout"], a["k"], a["act"], 0.0)
        args = {"conv": conv + (None,), "conv_prec": conv + (a["prec"], None), "conv3d": conv3d + (None,), "conv3d_prec": conv3d + (a["prec"], None),
                "conv_pool": flat + (a["pool"], a["y"], a["prec"], None), "conv_split": flat + (a["depth"], a["y"], a["prec"], None),
                "conv3d_res": (a["x"], a["B"], a["D"], a["Hs"], a["Ws"], a["Cin"], a["ps"], a["pt"], 0.0, a["w"], a["bias"], a["Cout"], a["k"],
                               a["act"], 0.0, a["res"], a["y"], a["yn"], a["prec"], None)}[fn]
        rc = getattr(lib, "r3d_torso_" + fn)(*args)
        return rc, lib.r3d_last_error()

    def refused(fns, quote, **over):
        for fn in fns.split():
            rc, msg = call(fn, **over)
            name = ("torso_" + fn[:-5] if fn.endswith("_prec") else "torso_" + fn).encode()
            assert rc == -1 and name + b":" in msg and quote in msg, (fn, over, rc, msg)
        return msg

    ALL = "conv conv_prec conv3d conv3d_prec conv_pool conv_split conv3d_res"
    TWO_OUT, D3, PREC = "conv conv_prec conv3d conv3d_prec conv3d_res", "conv3d conv3d_prec conv3d_res", "conv_prec conv3d_prec conv_pool conv_split conv3d_res"
    refused(ALL, b"NULL pointer", x=None)
    refused(ALL, b"NULL pointer", w=None)
    refused(ALL, b"NULL pointer", y=None)                                       # no output pointer at all
    refused("conv conv_prec conv3d_res", b"NULL pointer", ps=PS)                # pro_scale without pro_shift
    refused("conv conv_prec conv3d_res", b"NULL pointer", pt=PT)
    refused(ALL, b"bad argument", B=0)
    refused(ALL, b"bad argument", Cin=0)
    refused(ALL, b"bad argument", Cout=4097)
    refused(D3, b"bad argument", D=1025)
    refused(ALL, b"ksize 5", k=5)
    refused("conv conv_prec conv3d conv3d_prec", b"upsample 2", up=2)
    refused(ALL, b"act 3", act=3)
    refused(PREC, b"precision 2", prec=2)
    refused("conv3d conv3d_prec conv_pool", b"pool", pool=2)
    refused("conv3d conv3d_prec", b"pool", full=2)
    refused("conv3d conv3d_prec conv_pool", b"odd size", pool=1, Hs=3)          # a 3 x 4 grid
    refused("conv3d conv3d_prec", b"channel-last only", pool=1, yn=YN)
    refused("conv3d conv3d_prec", b"channel-last only", pool=1, y=None, yn=YN)
    refused("conv3d conv3d_prec", b"channel slice", yco=-1)
    refused("conv3d conv3d_prec", b"channel slice", ycs=11, yco=4)
    refused("conv_split", b"multiple of depth", Cout=10, depth=4)
    refused("conv_split", b"multiple of depth", depth=0)
    refused(ALL, b"2^31", B=32768, D=1, Hs=256, Ws=256, Cin=1, Cout=1)          # 2^31 output positions
    refused(ALL, b"overlap", y=X)
    refused(ALL, b"overlap", y=W)
    refused(TWO_OUT, b"overlap", yn=Y + 4)
    refused(TWO_OUT, b"overlap", y=None, yn=X)
    refused("conv conv_prec conv3d_res", b"residual", res=Y + 4)                # overlaps y without being y
    # a rule that does not apply to an entry point stays not applying: the call is refused for its one defect, which is checked later
    refused("conv conv_prec conv_pool conv_split", b"act 3", Hs=1025, D=1025, act=3)            # the 2-D entry points have no D to limit
    refused("conv_split", b"act 3", Cout=2050, depth=1025, act=3)                               # nor does the split's depth have that limit
    refused("conv3d conv3d_prec conv_pool", b"overlap", pool=0, Hs=3, y=X)                     # odd sizes are fine without the pool
    refused("conv3d conv3d_prec", b"overlap", y=None, yco=-1, yn=X)                             # no y: no channel slice
    assert b"residual" not in refused("conv conv_prec conv3d_res", b"overlap", res=Y, yn=Y + 4)  # the residual may be y itself
    refused("conv3d conv3d_prec", b"overlap", full=1, D=1024, y=None, yn=X)                     # full depth: D depth taps, one output depth


def test_sr_conv_argument_errors():
    """What r3d_conv_forward / _cat / _blend and r3d_sr_block_forward refuse before any launch: rc -1 (-2 for the workspace) and a message with the
    entry point's name and the rule.  Every call has exactly one defect unless its comment says otherwise; the pointers are fake, 1 TiB apart and
    never dereferenced.  Rejected calls only: a valid one would launch (tests/test_gpu_blend_conv.py, test_gpu_sr_ops.py, test_gpu_raw_abi.py
    run those), which is also why "no workspace is asked for a SPLIT input" cannot be shown here -- the workspace is the last rule."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    PRE, SC, X, Y, MASK, A, B, NS, WS, IMG, IMGO, U8, AM = (i << 40 for i in range(1, 14))
    NCHW, CB8, SPLIT, SPLIT_MX, BIG = 0, 1, 2, 3, 1 << 60
    base = {
        "conv_forward": dict(pre=PRE, sc=SC, N=1, Cin=64, Cout=128, H=16, W=16, k=3, x=X, xf=NCHW, y=Y, yf=NCHW, ns=None, ws=WS, wsb=BIG),
        "conv_forward_cat": dict(pre=PRE, sc=SC, N=1, Cin=64, Cout=128, H=16, W=16, k=1, x=X, xf=NCHW, y=Y, yf=SPLIT, Ct=256, off=128, mask=MASK,
                                 ns=NS, ws=WS, wsb=BIG),
        "conv_forward_blend": dict(pre=PRE, sc=SC, N=1, Ca=32, Cb=32, Cout=128, H=16, W=16, a=A, b=B, mask=MASK, y=Y, yf=NCHW, ns=None),
        "sr_block_forward": dict(pre=PRE, sc=SC, N=1, Cin=16, Cout=128, H=8, W=8, up=1, x=X, xf=NCHW, img=IMG, y=Y, yf=NCHW, ns=None, imgo=IMGO,
                                 u8=None, am=None, prec=1, ws=WS, wsb=BIG)}

    def call(fn, **over):
        assert set(over) <= set(base[fn]), (fn, over)          # an override the entry point has no argument for would leave a valid call
        a = dict(base[fn], **over)
        args = {"conv_forward": lambda: (a["pre"], a["sc"], None, a["N"], a["Cin"], a["Cout"], a["H"], a["W"], a["k"], a["x"], a["xf"], 0, 0.0, 1.0, -1.0,
                                         a["y"], a["yf"], a["ns"], 0, None, a["ws"], a["wsb"], None),
                "conv_forward_cat": lambda: (a["pre"], a["sc"], None, a["N"], a["Cin"], a["Cout"], a["H"], a["W"], a["k"], a["x"], a["xf"], 0, 0.0, 1.0, -1.0,
                                             a["y"], a["yf"], a["Ct"], a["off"], a["mask"], 1, a["ns"], 0, a["ws"], a["wsb"], None),
                "conv_forward_blend": lambda: (a["pre"], a["sc"], None, a["N"], a["Ca"], a["Cb"], a["Cout"], a["H"], a["W"], a["a"], a["b"], a["mask"],
                                               0, 0.0, 1.0, -1.0, a["y"], a["yf"], a["ns"], 0, None, None),
                "sr_block_forward": lambda: (a["pre"], a["sc"], a["N"], a["Cin"], a["Cout"], a["H"], a["W"], a["up"], a["x"], a["xf"], a["img"], -1.0,
                                             a["y"], a["yf"], a["ns"], 0, a["imgo"], a["u8"], a["am"], a["prec"], a["ws"], a["wsb"], None)}[fn]()
        rc = getattr(lib, "r3d_" + fn)(*args)
        return rc, lib.r3d_last_error()

    def refused(fns, quote, rc=-1, **over):
        for fn in fns.split():
            got, msg = call(fn, **over)
            assert got == rc and fn.encode() + b":" in msg and quote in msg, (fn, over, got, msg)

    CONV, CAT, BLEND, BLOCK = "conv_forward", "conv_forward_cat", "conv_forward_blend", "sr_block_forward"
    PLAIN, LAYERS = CONV + " " + CAT, " ".join((CONV, CAT, BLEND))
    EVERY = LAYERS + " " + BLOCK
    # ---- NULL pointers and non-positive sizes ---------------------------------------------------------------------------------------------
    for key in ("pre", "sc"):
        refused(EVERY, b"bad argument", **{key: None})
    refused(PLAIN + " " + BLOCK, b"bad argument", x=None)
    refused(LAYERS, b"bad argument", y=None)
    refused(CAT + " " + BLEND, b"bad argument", mask=None)
    refused(BLEND, b"bad argument", a=None)
    refused(BLEND, b"bad argument", b=None)
    refused(BLOCK, b"bad argument", img=None)
    refused(BLOCK, b"bad argument", imgo=None)                                  # neither the fp32 nor the uint8 image
    for key in ("N", "H", "W"):
        refused(EVERY, b"bad argument", **{key: 0})
        refused(EVERY, b"bad argument", **{key: -1})
    refused(LAYERS, b"bad argument", Cout=0)
    refused(PLAIN, b"bad argument", Cin=0)
    refused(BLEND, b"bad argument", Ca=0)
    refused(BLEND, b"bad argument", Cb=-8)
    refused(BLOCK, b"bad argument", Cin=24)                                     # the block: Cin % 16, Cout % 128, up 0 | 1
    refused(BLOCK, b"bad argument", Cout=64)
    refused(BLOCK, b"bad argument", up=2)
    # ---- kernel size ------------------------------------------------------------------------------------------------------------------------
    for k in (0, 2, 5):
        refused(CONV, b"bad argument", k=k)
    refused(CAT, b"1x1", k=3)
    # ---- activation formats -----------------------------------------------------------------------------------------------------------------
    for f in (-1, 4):
        refused(CONV, b"unsupported", xf=f)
        refused(CONV, b"unsupported", yf=f)
        refused(CAT, b"unsupported input", xf=f)
        refused(BLEND, b"unsupported output", yf=f)
        refused(BLOCK, b"unsupported activation format", xf=f)
    for f in (NCHW, CB8, -1, 4):
        refused(CAT, b"must be SPLIT or SPLIT_MX", yf=f)
    refused(BLOCK, b"unsupported activation format", yf=4)
    refused(BLOCK, b"unsupported activation format", yf=-2)
    refused(CONV, b"unsupported", xf=SPLIT_MX, k=1)                             # fp8 records: the 3x3 kernels only
    refused(CAT, b"unsupported input", xf=SPLIT_MX)                             # (so never for the 1x1 conv of _cat)
    refused(CONV, b"unsupported", xf=SPLIT_MX, Cin=24)                          # ... in whole 16-channel groups
    refused(CONV, b"unsupported", yf=SPLIT_MX, Cout=24)
    refused(BLEND, b"unsupported output", yf=SPLIT_MX, Cout=24)
    for f in (CB8, SPLIT):
        refused(CONV, b"blocked formats", xf=f, Cin=24)
        refused(CAT, b"unsupported input", xf=f, Cin=24)
        refused(CONV, b"blocked formats", yf=f, Cout=12)
        refused(BLEND, b"unsupported output", yf=f, Cout=12)
    refused(CONV, b"multiple of 4", Cout=30)
    refused(BLEND, b"unsupported output", Cout=30)                              # Cout % 4 for an NCHW output too
    # ---- the concatenation part and the blend operand -----------------------------------------------------------------------------------------
    refused(CAT, b"multiples of 16", Cout=24)
    refused(CAT, b"multiples of 16", off=120)
    refused(CAT, b"multiples of 16", Ct=264)
    refused(CAT, b"chan_off + Cout <= C_total", off=-16)
    refused(CAT, b"chan_off + Cout <= C_total", off=144)
    refused(CAT, b"chan_off + Cout <= C_total", Ct=240)
    refused(BLEND, b"multiples of 8", Ca=36, Cb=28)
    refused(BLEND, b"multiples of 8", Ca=28, Cb=36)
    refused(BLEND, b"multiple of 64", Ca=8, Cb=40)
    # ---- 2^32 elements per sample, through each entry point's own channel term; one channel group less passes (two defects: the workspace is next) ----
    refused(CONV, b"32-bit index", H=4096, W=4096)                              # (max(Cin, Cout) + 128) H W = 2^32
    refused(CONV, b"workspace", rc=-2, H=4096, W=4096, Cout=124, wsb=8)
    refused(CONV, b"32-bit index", H=4096, W=4096, Cin=128, Cout=4)             # ... through Cin
    refused(CAT, b"32-bit index", H=2048, W=2048, Ct=896, off=0)                # (max(Cin, C_total) + 128) H W = 2^32; Cout + 128 stays at 2^30
    refused(CAT, b"workspace", rc=-2, H=2048, W=2048, Ct=880, off=0, wsb=8)
    refused(BLEND, b"32-bit index", H=2048, W=2048, Ca=448, Cb=448, Cout=64)    # (max(Ca + Cb, Cout) + 128) H W = 2^32
    refused(BLOCK, b"32-bit index", H=2048, W=2048, Cout=256)                   # max(Cin, Cout) (up ? 4 : 1) H W = 2^32
    refused(BLOCK, b"workspace", rc=-2, H=2048, W=2048, Cout=256, up=0, wsb=8)
    # ---- workspace ------------------------------------------------------------------------------------------------------------------------------
    for f in (NCHW, CB8):
        refused(PLAIN, b"workspace too small", rc=-2, xf=f, wsb=8)
        refused(PLAIN, b"workspace too small", rc=-2, xf=f, ws=None)
    refused(BLOCK, b"workspace too small", rc=-2, wsb=8)
    refused(BLOCK, b"workspace too small", rc=-2, ws=None)
    # ---- the block's precisions ---------------------------------------------------------------------------------------------------------------
    refused(BLOCK, b"unknown precision", prec=3)
    refused(BLOCK, b"unknown precision", prec=-1)
    refused(BLOCK, b"uint8", prec=0, u8=U8)                                     # R3D_SR_F32: no fused uint8 image, no max|x|, no up = 0, no SPLIT
    refused(BLOCK, b"x_absmax", prec=0, am=AM)
    refused(BLOCK, b"up=0", prec=0, up=0)
    refused(BLOCK, b"unsupported activation format", prec=0, xf=SPLIT)
    refused(BLOCK, b"unsupported activation format", prec=0, yf=SPLIT, ns=NS)
    refused(BLOCK, b"unsupported activation format", prec=1, xf=SPLIT_MX)        # fp8 records: R3D_SR_F16MX only
    refused(BLOCK, b"unsupported activation format", prec=1, yf=SPLIT_MX, ns=NS)
    for prec, f in ((1, SPLIT), (2, SPLIT), (2, SPLIT_MX)):
        refused(BLOCK, b"unsupported activation format", prec=prec, yf=f)       # a SPLIT output without next_scale


def test_product_has_no_oracle_dependency():
    """The oracle is test infrastructure: nothing under real3dportrait_amd/ may import or load it."""
    pkg = os.path.join(ROOT, "real3dportrait_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "r3d_oracle" not in txt and "from oracle" not in txt and "import oracle" not in txt, f


# The kernel sources carry no experiment switches (DESIGN "Retired experiment switches"): a build option or an environment variable read inside the library
# is a deliberate addition to one of these two lists, with its test, not a silent #ifndef.
CSRC_CONDITIONAL_MACROS = {"R3D_STAMPS"}          # the instrumented build (scripts/gpu_stamps.py)
CSRC_GETENV_NAMES = {"R3D_CONV_WINO"}             # include/r3d_hip.h; tests/test_gpu_wino.py


def test_kernel_sources_carry_no_experiment_switches():
    csrc = os.path.join(ROOT, "real3dportrait_amd", "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    assert len(files) >= 10
    for f in files:
        src = open(os.path.join(csrc, f)).read()
        lines = src.split("\n")
        for i, ln in enumerate(lines):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b([^/]*)", ln)           # (#else / #endif belong to one of these)
            if not m:
                continue
            names = set(re.findall(r"[A-Za-z_]\w*", m.group(2))) - {"defined"}
            include_guard = m.group(1) == "ifndef" and len(names) == 1 and re.match(r"\s*#\s*define\s+%s\s*$" % min(names), lines[i + 1]) is not None
            assert include_guard or (names and names <= CSRC_CONDITIONAL_MACROS), "%s:%d: %s" % (f, i + 1, ln.strip())
        for m in re.finditer(r"getenv\s*\(([^)]*)\)", src):
            assert m.group(1).strip().strip('"') in CSRC_GETENV_NAMES, "%s: getenv(%s)" % (f, m.group(1))


def test_render_workspace_grows_for_the_shapes_that_park_colours():
    """r3d_render_workspace_bytes: per-ray limits + the fold record, plus -- when Nc or Nf exceeds 48 AND there is a fine pass, i.e. the kernel shapes that
    park a ray's colours -- grid x 4 waves x 2 (6 + 6) tiles x 1 KB, with the grid the launch really uses (round 6, ADVICE r5: a fixed 48 MB before)."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    base = lib.r3d_render_workspace_bytes(1, 128 * 128, 48, 48)
    park = 512 * 4 * 24 * 64 * 16                                                       # 16 384 rays = 4 096 blocks of 4 waves: the grid is capped at 512
    assert lib.r3d_render_workspace_bytes(1, 128 * 128, 96, 96) == base + park
    assert lib.r3d_render_workspace_bytes(1, 128 * 128, 40, 60) == base + park          # <4,4> is dispatched for Nf > 48 too
    assert lib.r3d_render_workspace_bytes(1, 128 * 128, 96, 0) == base                  # a coarse-only call never parks (<6,0>)
    assert lib.r3d_render_workspace_bytes(1, 128 * 128, 16, 16) == base
    small = lib.r3d_render_workspace_bytes(1, 32 * 32, 96, 96) - lib.r3d_render_workspace_bytes(1, 32 * 32, 48, 48)
    assert small == 256 * 4 * 24 * 64 * 16                                              # 1 024 rays = 256 blocks: half the parking of a full grid


def test_render_workspace_sizes_are_pinned():
    """The totals RenderWorkspaceLayout (csrc/r3d_render.hip) adds up to; the numbers are those of the library before the layout was named:
    gstate (8 + 3 per 256 rays ints, rounded up to 64 bytes) + ray_start + ray_end + 64 + the fold record with its partials (64 + 512 * 4) +,
    for the calls that park, grid x 4 waves x 24 tiles x 1 KB."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    assert lib.r3d_render_workspace_bytes(1, 16384, 48, 48) == 134080          # 832 + 131072 + 64 + 2112
    assert lib.r3d_render_workspace_bytes(1, 16384, 96, 96) == 50465728        # + 512 * 4 * 24 * 64 * 16
    assert lib.r3d_render_workspace_bytes(2, 1000, 16, 16) == 18304            # 128 + 16000 + 64 + 2112
    assert lib.r3d_render_workspace_bytes(1, 1024, 96, 96) == 25176320         # 128 + 8192 + 64 + 2112 + 256 * 4 * 24 * 64 * 16
    assert lib.r3d_render_workspace_bytes(1, 1, 4, 0) == 2248                  # 64 + 8 + 64 + 2112
    assert lib.r3d_render_workspace_bytes(1, 64, 64, 20) == 1575616            # 64 + 512 + 64 + 2112 + 16 * 4 * 24 * 64 * 16: <4,4> gets <6,6>'s room
    assert lib.r3d_render_workspace_bytes(1, 64, 96, 0) == 2752
    assert lib.r3d_run_model_workspace_bytes() == 2112


def test_render_argument_errors():
    """What r3d_planes_to_nhwc, r3d_raygen, r3d_render_forward and r3d_run_model refuse before any HIP call: rc -1 (-2 for the workspace) and a
    message with the entry point's name and the rule.  Every call has exactly one defect; the pointers are fake, 64-byte aligned, 1 TiB apart and
    never dereferenced.  The rules about planes, decoder, N, triplane_depth and box_warp are the same for r3d_render_forward and r3d_run_model,
    but their wording is only pinned where both have always said the same ("bad shape" for H, W)."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    P, W1, B1, W2, B2, O, D, RGB, DEP, WS, V, WK, C2W, K, SPO, SPS, CO, SIG, ADD, OUT, PART = (i << 40 for i in range(1, 22))
    BIG = 1 << 60
    base = {
        "planes_to_nhwc": dict(src=P, add=None, dst=OUT, N=1, C=32, H=8, W=8, depth=1, flip=0, part=None, npart=None),
        "raygen": dict(c2w=C2W, K=K, N=1, R=16, o=O, d=D),
        "render_forward": dict(planes=P, N=1, H=32, W=32, depth=1, w1=W1, b1=B1, w2=W2, b2=B2, o=O, d=D, M=256, Nc=48, Nf=48, box=1.0, rgb=RGB,
                               dep=DEP, wsum=WS, valid=V, c2w=None, K=None, spo=None, sps=None, stride=0, ws=WK, wsb=BIG),
        "run_model": dict(planes=P, N=1, H=32, W=32, depth=1, w1=W1, b1=B1, w2=W2, b2=B2, co=CO, npts=16, box=1.0, rgb=RGB, sig=SIG, ws=WK, wsb=BIG)}

    def call(fn, **over):
        assert set(over) <= set(base[fn]), (fn, over)          # an override the entry point has no argument for would leave a valid call
        a = dict(base[fn], **over)
        args = {"planes_to_nhwc": lambda: (a["src"], a["add"], a["dst"], a["N"], a["C"], a["H"], a["W"], a["depth"], a["flip"], a["part"], a["npart"], None),
                "raygen": lambda: (a["c2w"], a["K"], a["N"], a["R"], a["o"], a["d"], None),
                "render_forward": lambda: (a["planes"], a["N"], a["H"], a["W"], a["depth"], a["w1"], a["b1"], a["w2"], a["b2"], a["o"], a["d"], a["M"],
                                           a["Nc"], a["Nf"], a["box"], 0, None, None, 0, a["rgb"], 1, a["dep"], a["wsum"], a["valid"], None, 0,
                                           a["c2w"], a["K"], a["spo"], a["sps"], a["stride"], a["ws"], a["wsb"], None),
                "run_model": lambda: (a["planes"], a["N"], a["H"], a["W"], a["depth"], a["w1"], a["b1"], a["w2"], a["b2"], a["co"], a["npts"], a["box"],
                                      a["rgb"], a["sig"], None, 0, a["ws"], a["wsb"], None)}[fn]()
        rc = getattr(lib, "r3d_" + fn)(*args)
        return rc, lib.r3d_last_error()

    def refused(fn, quote, rc=-1, **over):
        got, msg = call(fn, **over)
        assert got == rc and fn.encode() + b":" in msg and quote in msg, (fn, over, got, msg)

    NHWC, RAYGEN, RENDER, MODEL = "planes_to_nhwc", "raygen", "render_forward", "run_model"
    # ---- r3d_planes_to_nhwc -------------------------------------------------------------------------------------------------------------------
    refused(NHWC, b"n_partials", part=PART)                                     # partials without the count's address
    refused(NHWC, b"bad argument", src=None)
    refused(NHWC, b"bad argument", dst=None)
    for key in ("N", "C", "H", "W"):
        refused(NHWC, b"bad argument", **{key: 0})
        refused(NHWC, b"bad argument", **{key: -1})
    for depth in (0, -1, 17):
        refused(NHWC, b"bad argument", depth=depth)
    for flip in (-1, 64):
        refused(NHWC, b"bad argument", flip=flip)
    # ---- r3d_raygen ---------------------------------------------------------------------------------------------------------------------------
    for key in ("c2w", "K", "o", "d"):
        refused(RAYGEN, b"bad argument", **{key: None})
    for key in ("N", "R"):
        refused(RAYGEN, b"bad argument", **{key: 0})
        refused(RAYGEN, b"bad argument", **{key: -1})
    # ---- planes, decoder, N, triplane_depth, box_warp: both forwards ----------------------------------------------------------------------------
    for key in ("planes", "w1", "b1", "w2", "b2"):
        refused(RENDER, b"NULL pointer", **{key: None})
        refused(MODEL, b"", **{key: None})
    for over in (dict(N=0), dict(N=-1), dict(depth=0), dict(depth=-1), dict(depth=17), dict(box=0.0), dict(box=-1.0), dict(box=float("nan"))):
        refused(RENDER, b"bad shape", **over)
        refused(MODEL, b"", **over)
    for over in (dict(H=1), dict(W=1), dict(H=0), dict(W=-1)):
        refused(RENDER, b"bad shape", **over)
        refused(MODEL, b"bad shape", **over)
    # ---- r3d_render_forward's own ---------------------------------------------------------------------------------------------------------------
    for key in ("o", "d", "rgb", "wsum", "valid"):                              # one ray array without the other: neither explicit rays nor camera mode
        refused(RENDER, b"NULL pointer", **{key: None})
    refused(RENDER, b"NULL pointer", o=None, d=None)                            # no rays and no camera
    refused(RENDER, b"NULL pointer", o=None, d=None, c2w=C2W)                   # half a camera
    refused(RENDER, b"bad shape", M=0)
    refused(RENDER, b"bad shape", M=-4)
    for over in (dict(Nc=3), dict(Nc=97), dict(Nf=-1), dict(Nf=97)):
        refused(RENDER, b"depth_resolution", **over)
    refused(RENDER, b"32-bit tap offsets", H=4096, W=4096)                      # 3 * 4096^2 * 128 = 6 GiB of planes per image
    refused(RENDER, b"32-bit tap offsets", H=1024, W=1024, depth=16)
    refused(RENDER, b"workspace", rc=-2, ws=None)
    refused(RENDER, b"workspace", rc=-2, wsb=lib.r3d_render_workspace_bytes(1, 256, 48, 48) - 1)
    refused(RENDER, b"camera mode", o=None, d=None, c2w=C2W, K=K, M=250)        # camera mode renders an R x R image
    refused(RENDER, b"split_scale", spo=SPO)                                    # split_out without its scales
    refused(RENDER, b"split_scale", spo=SPO + 8, sps=SPS)                       # 16-byte alignment of both, a stride in whole float4s
    refused(RENDER, b"split_scale", spo=SPO, sps=SPS + 4)
    refused(RENDER, b"split_scale", spo=SPO, sps=SPS, stride=6)
    # ---- r3d_run_model's own --------------------------------------------------------------------------------------------------------------------
    for key in ("co", "rgb", "sig"):
        refused(MODEL, b"bad argument", **{key: None})
    refused(MODEL, b"bad argument", npts=0)
    refused(MODEL, b"bad argument", npts=-1)
    refused(MODEL, b"workspace", rc=-2, ws=None)
    refused(MODEL, b"workspace", rc=-2, wsb=lib.r3d_run_model_workspace_bytes() - 1)
    refused(MODEL, b"workspace", rc=-2, ws=WK + 8)                              # 16-byte alignment


def test_render_index_range_errors():
    """Sizes whose indices would leave the kernels' ints are refused by name of the limit, before any HIP call (no GPU here: a launch would
    come back as -3): r3d_run_model's gather is an int in float4 units with 24-bit row products, the ray kernels carry the ray in an int,
    the layout kernels H * W, the ray generator R * R.  Fake pointers, never dereferenced; one limit per call."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    p = [ctypes.c_void_p(i << 40) for i in range(1, 12)]

    def run_model(H, W, depth):
        return lib.r3d_run_model(p[0], 1, H, W, depth, p[1], p[2], p[3], p[4], p[5], 16, 1.0, p[6], p[7], None, 0, p[8], 1 << 60, None)

    for H, W, depth in ((16384, 16384, 1), (8192, 2048, 16), (4096, 4096, 6)):          # 3 * depth * H * W * 8 = 3 * 2^31, 3 * 2^31, 1.125 * 2^31
        assert run_model(H, W, depth) == -1 and b"run_model:" in lib.r3d_last_error() and b"2^31" in lib.r3d_last_error(), (H, W, depth)
    for H, W in ((1 << 24, 2), (2, 1 << 24)):                                           # 3 * 2^25 * 8 < 2^31, but the row product is 24-bit
        assert run_model(H, W, 1) == -1 and b"run_model:" in lib.r3d_last_error() and b"2^24" in lib.r3d_last_error(), (H, W)
    for N, M in ((2, 1 << 30), (3, 715827883), (1 << 16, 1 << 15)):                     # N * M = 2^31, 2^31 + 1, 2^31
        rc = lib.r3d_render_forward(p[0], N, 32, 32, 1, p[1], p[2], p[3], p[4], p[5], p[6], M, 48, 48, 1.0, 0, None, None, 0,
                                    p[7], 1, None, p[8], p[9], None, 0, None, None, None, None, 0, p[10], 1 << 62, None)
        assert rc == -1 and b"render_forward:" in lib.r3d_last_error() and b"2^31 - 1" in lib.r3d_last_error(), (N, M)
    for H, W in ((65536, 32768), (46341, 46341)):                                       # H * W = 2^31, 2^31 + 50 633
        rc = lib.r3d_planes_to_nhwc(p[0], None, p[1], 1, 32, H, W, 1, 0, None, None, None)
        assert rc == -1 and b"planes_to_nhwc:" in lib.r3d_last_error() and b"2^31 - 1" in lib.r3d_last_error(), (H, W)
    for R in (46341, 65536, 2147483647):                                                # 46340^2 = 2^31 - 88 047 is the largest image
        rc = lib.r3d_raygen(p[0], p[1], 1, R, p[2], p[3], None)
        assert rc == -1 and b"raygen:" in lib.r3d_last_error() and b"2^31 - 1" in lib.r3d_last_error(), R


def test_no_hazardous_packed_f32_forms(tmp_path):
    """gfx950 erratum found in round 3: a packed-f32 instruction whose src1 / src2 op_sel bit is set returns a wrong low half
    in lanes 48-63 while another wave of the SIMD executes MFMAs.  The library is compiled WITHOUT packed-f32 instructions (they buy
    nothing next to MFMAs: csrc/Makefile); this test disassembles the device code objects that are actually inside the shipped libr3d_hip.so and
    checks that no line matches the pattern the Makefile refuses, crossed operands or not -- plus the barrier / fp16-rounding lints of the SR kernels."""
    import shutil
    import subprocess
    from real3dportrait_amd import _lib
    packed = r"^\s*v_pk_(mul|add|fma)_f32|^\s*v_pk_mov_b32"
    assert packed in open(os.path.join(ROOT, "real3dportrait_amd", "csrc", "Makefile")).read(), "csrc/Makefile refuses another pattern than this test counts"
    llvm = "/opt/rocm/lib/llvm/bin"
    so = str(tmp_path / "lib.so")
    shutil.copy(_lib.LIB_PATH, so)
    subprocess.check_call([llvm + "/llvm-objdump", "--offloading", so], stdout=subprocess.DEVNULL)      # writes lib.so.<k>.hipv4-...-gfx950
    objs = [str(tmp_path / f) for f in sorted(os.listdir(tmp_path)) if "amdgcn" in f]
    assert len(objs) >= 4, objs
    n_pk = n_mix = n_bar = 0
    bare_barriers = []
    for o in objs:
        dis = subprocess.run([llvm + "/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        sym, reads_in_flight = "", 0
        for line in dis.splitlines():
            # in the DMA-pipelined SR loops a wave must not pass a barrier with LDS reads in flight (the buffer they read is
            # refilled right after it).  Straight-line model of lgkmcnt for ds_read*: a barrier of those kernels with a read issued and
            # not yet waited for is the race that put 55 of 1 920 pipelined frames off by one count.
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                sym, reads_in_flight = m.group(1), 0
                continue
            ins = re.sub(r"\s*//.*", "", line).strip()
            if ins.startswith("ds_read"):
                reads_in_flight += 1
            elif ins.startswith("s_waitcnt"):
                w = re.search(r"lgkmcnt\((\d+)\)", ins)
                if w:
                    reads_in_flight = min(reads_in_flight, int(w.group(1)))
            elif ins.startswith("s_barrier") and ("conv_mfma_f16x3" in sym or "upconv_fir_f16x3" in sym or "conv1x1_mfma_f16x3" in sym):
                n_bar += 1
                if reads_in_flight:
                    bare_barriers.append(sym[:60])
            # fp16(a * b) fused into one rounding (v_fma_mixlo/hi_f16 a, b, 0): hipcc derives `hi` of an fp16 hi/lo split this way at one
            # use and by fl32 + v_cvt at another, so hi + lo misses the value by an ulp of hi where the roundings differ
            # (csrc/r3d_common.h as_rounded()); no split in this library may compile to it
            if re.search(r"v_fma_mix(lo|hi)_f16 v\d+, [^,]+, [^,]+, 0\b", line):
                n_mix += 1
            n_pk += int(re.search(packed, line) is not None)
    assert n_pk == 0, "%d packed-f32 instructions in libr3d_hip.so: the library is built without them (csrc/Makefile)" % n_pk
    assert n_bar >= 30, "only %d barriers seen in the SR conv kernels: is the symbol tracking broken?" % n_bar
    assert not bare_barriers, "s_barrier passed with ds_reads in flight in: %s" % sorted(set(bare_barriers))
    assert n_mix == 0, "%d fp16 roundings fused into their product (v_fma_mix*_f16 a, b, 0): a hi/lo split is missing as_rounded()" % n_mix
