"""CPU: _lib.call, the one way from the package into libr3d_hip.so: what it refuses before the library is entered, what
it passes through, and what it returns.  Needs the built library, no GPU."""
import ctypes

import pytest
import torch

from real3dportrait_amd import _lib

A = [i << 40 for i in range(1, 8)]          # fake device addresses, never dereferenced: the C validation fails first


def refused(exc, match, name, *args):
    """call(name, *args) raises `exc` matching `match` and the library is not entered."""
    with _lib.counting() as calls:
        with pytest.raises(exc, match=match):
            _lib.call(name, *args)
    assert calls == []


def layernorm_args(x=A[0], g=A[1], b=A[2], y=A[3]):
    return (x, 4, 32, g, b, 1e-5, y, None)


def test_wrong_dtype_at_a_typed_pointer():
    for t in (torch.zeros(4, 32, dtype=torch.float64), torch.zeros(4, 32, dtype=torch.int64)):
        refused(TypeError, r"r3d_secc_layernorm: argument 0 is a float\*, got a %s tensor" % t.dtype, "r3d_secc_layernorm", *layernorm_args(x=t))
    refused(TypeError, r"r3d_secc_layernorm: argument 6 is a float\*", "r3d_secc_layernorm", *layernorm_args(y=torch.zeros(4, 32, dtype=torch.float16)))
    f32 = torch.zeros(6, 3)
    raster = [A[0], None, f32, 0, 1, 8, 6, 0, 16, 12.0, 5.0, 1, 1, 1.0, 0.0, None, A[1], A[2], None, A[3], 1 << 20, None]
    refused(TypeError, r"r3d_raster_forward: argument 2 is a int32_t\*, got a torch.float32", "r3d_raster_forward", *raster)
    raster[2], raster[15] = A[4], torch.zeros(1, 16, 16, dtype=torch.int32)
    refused(TypeError, r"r3d_raster_forward: argument 15 is a int64_t\*, got a torch.int32", "r3d_raster_forward", *raster)
    blink = [A[0], 2, 64, 64, A[1], torch.zeros(1), 1, A[0], A[2], A[3], 1 << 20, None]
    refused(TypeError, r"r3d_secc_blink: argument 5 is a double\*, got a torch.float32", "r3d_secc_blink", *blink)
    blink[4], blink[5] = torch.zeros(1, dtype=torch.int64), A[4]
    refused(TypeError, r"r3d_secc_blink: argument 4 is a int32_t\*, got a torch.int64", "r3d_secc_blink", *blink)


def test_contiguity_then_device():
    """The order is dtype, contiguity, device: the first two show on a CPU tensor."""
    strided = torch.zeros(4, 64)[:, ::2]
    refused(ValueError, "r3d_secc_layernorm: argument 0 .* not contiguous", "r3d_secc_layernorm", *layernorm_args(x=strided))
    refused(TypeError, "argument 0 is a float", "r3d_secc_layernorm", *layernorm_args(x=strided.double()))          # dtype comes first
    refused(ValueError, "r3d_secc_layernorm: argument 3 .* not on a GPU", "r3d_secc_layernorm", *layernorm_args(g=torch.ones(32)))
    refused(ValueError, "not on a GPU", "r3d_secc_layernorm", *layernorm_args(g=torch.nn.Parameter(torch.ones(32))))
    refused(ValueError, "argument 0 .* not on a GPU", "r3d_secc_layernorm", *layernorm_args(x=torch.zeros(4, 32))[:-1])   # the stream left out


def test_types_with_the_same_bit_pattern_pass_the_dtype_stage():
    """bool at uint8_t*, bfloat16 and int16 at uint16_t*, anything at void*: on a CPU tensor they fail only at the device stage."""
    for valid in (torch.zeros(8, dtype=torch.bool), torch.zeros(8, dtype=torch.uint8)):
        args = [A[0], 1, 32, 32, 1, A[1], A[1], A[1], A[1], A[2], A[2], 8, 48, 48, 1.0, 0, None, None, 0, A[3], 1, None, A[4], valid, None, 0,
                None, None, None, None, 0, A[5], 1 << 30, None]
        refused(ValueError, "r3d_render_forward: argument 23 .*uint8_t.* not on a GPU", "r3d_render_forward", *args)
    for piece in (torch.zeros(8, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.int16)):
        refused(ValueError, "r3d_torso_split_bf16x3: argument 2 .*uint16_t.* not on a GPU", "r3d_torso_split_bf16x3", A[0], 8, piece, A[1], A[2], None)
    refused(TypeError, r"argument 2 is a uint16_t\*, got a torch.float32", "r3d_torso_split_bf16x3", A[0], 8, torch.zeros(8), A[1], A[2], None)
    for any_dtype in (torch.uint8, torch.float16, torch.float64):
        refused(ValueError, r"r3d_conv_prepack: argument 4 \(void\*\) is not on a GPU", "r3d_conv_prepack", A[0], 16, 128, 3,
                torch.zeros(64, dtype=any_dtype), None)


def test_argument_count():
    refused(TypeError, "r3d_secc_layernorm takes 8 arguments .*stream may be left out.*, got 9", "r3d_secc_layernorm", *layernorm_args(), None)
    refused(TypeError, "r3d_secc_layernorm takes 8 arguments .*, got 6", "r3d_secc_layernorm", *layernorm_args()[:6])
    refused(TypeError, "r3d_raster_workspace_bytes takes 3 arguments, got 2", "r3d_raster_workspace_bytes", 1, 512)          # no stream to leave out
    refused(TypeError, "r3d_version takes 0 arguments, got 1", "r3d_version", None)


def test_addresses_pass_through_to_the_c_validation():
    """None (NULL), an int address and a ctypes pointer go to the library as they are, and its refusal comes back as check() words it.
    A status of 0 is not reachable without a GPU (a call the C validation accepts launches): tests/test_gpu_secc_ops.py has that path."""
    for x in (A[0], ctypes.c_void_p(A[0]), ctypes.cast(ctypes.c_void_p(A[0]), ctypes.POINTER(ctypes.c_float))):
        with _lib.counting() as calls:
            with pytest.raises(RuntimeError, match=r"^libr3d_hip secc_layernorm failed \(-1\): secc_layernorm: bad argument"):
                _lib.call("r3d_secc_layernorm", x, 4, 32, A[1], A[2], 0.0, A[3], None)          # eps = 0
        assert [n for n, _ in calls] == ["r3d_secc_layernorm"] and calls[0][1][1:] == (4, 32, A[1], A[2], 0.0, A[3], None)
    with pytest.raises(RuntimeError, match="secc_layernorm failed"):
        _lib.call("r3d_secc_layernorm", None, 4, 32, A[1], A[2], 1e-5, A[3], None)          # x = NULL


def test_value_returning_entry_points_return_the_value():
    assert _lib.call("r3d_raster_workspace_bytes", 1, 512, 70000) == 512 * 512 * 8 + 256 + (70000 * 4 + 255) // 256 * 256
    assert _lib.call("r3d_version") == _lib.ABI_VERSION == 80
    assert _lib.call("r3d_sr_block_bound_offset", 32, 256) == _lib.load().r3d_sr_block_bound_offset(32, 256)
    with pytest.raises(RuntimeError):
        _lib.call("r3d_raygen", None, None, 1, 16, None, None, None)
    assert b"raygen" in _lib.call("r3d_last_error")


def test_counting_nests_and_sees_a_substituted_library():
    """counting() records per block; call() looks the function up through load(), so a stand-in in _lib._lib is what gets called."""
    with _lib.counting() as outer:
        _lib.call("r3d_version")
        with _lib.counting() as inner:
            _lib.call("r3d_run_model_workspace_bytes")
        _lib.call("r3d_version")
    assert [n for n, _ in outer] == ["r3d_version", "r3d_version"] and inner == [("r3d_run_model_workspace_bytes", ())]
    real = _lib.load()

    class StandIn:
        def __getattr__(self, name):
            return (lambda *a: 81) if name == "r3d_version" else getattr(real, name)

    _lib._lib = StandIn()
    try:
        assert _lib.call("r3d_version") == 81
    finally:
        _lib._lib = real
    assert _lib.call("r3d_version") == 80


def test_ptr_raises_instead_of_asserting():
    assert _lib.ptr(None) is None
    with pytest.raises(ValueError, match="device tensors only"):
        _lib.ptr(torch.zeros(4))
