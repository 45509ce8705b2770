"""ctypes binding of libr3d_hip.so (the C ABI declared in include/r3d_hip.h and the five companion headers it includes, and in the
extension headers of EXTENSION_SIGNATURES, the feature headers of FEATURE_SIGNATURES and the module headers of MODULE_SIGNATURES, which
include r3d_hip.h).

The product path has NO fallback: if the HIP library is missing or fails to load, importing an
operator raises.  Build it with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C real3dportrait_amd/csrc`.
"""
import contextlib
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("R3D_LIB") or os.path.join(_HERE, "lib", "libr3d_hip.so")     # R3D_LIB: an experiment build (scripts/)
CSRC = os.path.join(_HERE, "csrc")

c_void_p, c_int, c_float, c_size_t, c_uint64 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                                ctypes.c_size_t, ctypes.c_uint64)
H = c_void_p          # an untyped HOST pointer: an opaque handle (event, communicator), the 128-byte id, an array of structs or of addresses


class DevPtr:
    """A DEVICE pointer parameter.  elem: the C element type the header declares; call() accepts the torch dtypes with that bit pattern
    (DTYPES, resolved in load(): importing this module does not import torch)."""
    DTYPES = {"float": ("float32",), "double": ("float64",), "int32_t": ("int32",), "int64_t": ("int64",), "uint8_t": ("uint8", "bool"),
              "uint16_t": ("bfloat16", "int16", "uint16"), "void": None}      # uint16_t: what the package keeps bf16 pieces in; void: any
    ctype = c_void_p

    def __init__(self, elem):
        self.elem = elem

    def __repr__(self):
        return "DevPtr(%r)" % self.elem


class Stream:
    """r3d_stream_t: a hipStream_t passed as void*.  As the last parameter it may be left out of a call(): the current stream is passed."""
    ctype = c_void_p


F, F64, I32, I64, U8, U16, V = (DevPtr(e) for e in ("float", "double", "int32_t", "int64_t", "uint8_t", "uint16_t", "void"))
S = Stream()
# what the two r3d_fit_landmark_* entry points begin with; `lambdas` is a HOST array of six floats
_FIT_COMMON = [F, F, F, c_int, c_int, c_int, F, F, c_int, c_int, c_float, c_float, c_float, ctypes.POINTER(c_float)]

# name -> (restype, [one entry per parameter]); mirrors include/r3d_hip.h and the five companion headers it includes one to one
# (tests/test_abi.py compares every declaration of the six).  A library that lacks one of them does not load.
# An entry is a ctypes type (scalars; host pointers as ctypes.POINTER(...) or, untyped, H), a device pointer named by the header's element
# type (F float*, F64 double*, I32 int32_t*, I64 int64_t*, U8 uint8_t*, U16 uint16_t*, V void*), or S, the trailing r3d_stream_t.
SIGNATURES = {
    "r3d_version": (c_int, []),
    "r3d_last_error": (ctypes.c_char_p, []),
    "r3d_planes_to_nhwc": (c_int, [F, F, F, c_int, c_int, c_int, c_int, c_int, c_int, F, ctypes.POINTER(c_int), S]),
    "r3d_planes_absmax_partials": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "r3d_raygen": (c_int, [F, F, c_int, c_int, F, F, S]),
    "r3d_render_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "r3d_render_forward": (c_int, [F, c_int, c_int, c_int, c_int, F, F, F, F, F, F, c_int, c_int, c_int, c_float, c_int, F, F, c_uint64, F, c_int, F,
                                   F, U8, F, c_int, F, F, V, F, c_size_t, V, c_size_t, S]),
    "r3d_run_model": (c_int, [F, c_int, c_int, c_int, c_int, F, F, F, F, F, c_int, c_float, F, F, F, c_int, V, c_size_t, S]),
    "r3d_run_model_workspace_bytes": (c_size_t, []),
    "r3d_sr_block_prepacked_bytes": (c_size_t, [c_int, c_int]),
    "r3d_sr_block_styles_bytes": (c_size_t, [c_int, c_int, c_int]),
    "r3d_sr_block_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "r3d_sr_block_prepack": (c_int, [c_int, c_int, F, F, V, c_int, S]),
    "r3d_sr_block_styles": (c_int, [F, c_int, c_int, c_int, c_int, F, F, F, F, F, F, F, F, F, F, F, F, V, S]),
    "r3d_sr_block_forward": (c_int, [V, V, c_int, c_int, c_int, c_int, c_int, c_int, V, c_int, F, c_float, V, c_int, F, c_size_t, F, U8, F, c_int, V,
                                     c_size_t, S]),
    "r3d_chain_fold": (c_int, [H, c_int, c_int, H, c_int, H, c_int, S]),
    "r3d_sr_block_bound_offset": (c_size_t, [c_int, c_int]),
    "r3d_conv_scales_bound_offset": (c_size_t, [c_int, c_int]),
    "r3d_absmax": (c_int, [F, c_size_t, c_int, F, F, S]),
    "r3d_conv_prepacked_bytes": (c_size_t, [c_int, c_int, c_int]),
    "r3d_conv_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "r3d_conv_scales_bytes": (c_size_t, [c_int, c_int, c_int]),
    "r3d_conv_prepack": (c_int, [F, c_int, c_int, c_int, V, S]),
    "r3d_conv_forward": (c_int, [V, V, F, c_int, c_int, c_int, c_int, c_int, c_int, V, c_int, c_int, c_float, c_float, c_float, V, c_int, F,
                                 c_size_t, F, V, c_size_t, S]),
    "r3d_blend_cat_to_split": (c_int, [F, c_int, c_int, F, c_int, c_int, F, c_int, c_int, c_int, V, c_int, F, c_size_t, S]),
    "r3d_conv_forward_cat": (c_int, [V, V, F, c_int, c_int, c_int, c_int, c_int, c_int, V, c_int, c_int, c_float, c_float, c_float, V, c_int, c_int,
                                     c_int, F, c_int, F, c_size_t, V, c_size_t, S]),
    "r3d_conv_forward_blend": (c_int, [V, V, F, c_int, c_int, c_int, c_int, c_int, c_int, F, F, F, c_int, c_float, c_float, c_float, V, c_int, F,
                                       c_size_t, F, S]),
    "r3d_debug_conv_variant": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "r3d_debug_sr_block_variants": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, ctypes.POINTER(c_int)]),
    "r3d_upsample2x_bilinear": (c_int, [F, c_int, c_int, c_int, c_int, V, c_int, F, c_size_t, S]),
    "r3d_resize_bilinear": (c_int, [F, c_int, c_int, c_int, F, c_int, c_int, c_int, S]),
    "r3d_blend": (c_int, [F, F, F, c_int, c_int, c_int, c_int, F, S]),
    "r3d_person_occlusion": (c_int, [F, F, c_float, c_size_t, F, S]),
    "r3d_frames_to_u8": (c_int, [F, c_int, c_int, c_int, U8, S]),
    "r3d_comm_unique_id": (c_int, [H]),
    "r3d_comm_init": (c_int, [H, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "r3d_comm_destroy": (c_int, [H]),
    "r3d_gather_frames": (c_int, [H, U8, c_size_t, U8, c_int, S]),
    "r3d_event_create": (c_int, [ctypes.POINTER(c_void_p)]),
    "r3d_event_record": (c_int, [H, S]),
    "r3d_event_elapsed_ms": (c_int, [H, H, ctypes.POINTER(c_float)]),
    "r3d_event_destroy": (c_int, [H]),
    "r3d_profile_configure": (c_int, [ctypes.c_uint32]),
    "r3d_profile_reset": (c_int, []),
    "r3d_profile_read": (c_int, [c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int)]),
    "r3d_profile_clock": (c_int, [c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ulonglong)]),
    "r3d_secc_embed1": (c_int, [F, c_int, c_int, c_int, c_int, F, F, F, F, F, F, F, S]),
    "r3d_secc_conv": (c_int, [F, c_int, c_int, c_int, c_int, F, F, c_int, c_int, c_int, c_int, F, F, c_float, F, S]),
    "r3d_secc_linear": (c_int, [F, c_int, c_int, F, F, c_float, F, F, c_int, c_int, F, F, S]),
    "r3d_secc_layernorm": (c_int, [F, c_int, c_int, F, F, c_float, F, S]),
    "r3d_secc_attention": (c_int, [F, F, c_int, c_int, c_int, c_int, c_int, c_float, F, S]),
    "r3d_secc_dwconv_gelu": (c_int, [F, c_int, c_int, c_int, c_int, F, F, F, S]),
    "r3d_secc_head": (c_int, [F, c_int, c_int, c_int, F, F, F, F, F, F, F, F, S]),
    "r3d_torso_volume_to_cl": (c_int, [F, c_int, c_int, c_int, c_int, c_int, F, S]),
    "r3d_torso_warp": (c_int, [F, c_int, c_int, c_int, c_int, c_int, F, c_int, c_int, c_int, F, c_int, S]),
    "r3d_torso_conv": (c_int, [F, c_int, c_int, c_int, c_int, c_int, c_int, F, F, c_float, F, F, c_int, c_int, c_int, c_float, F, F, F, S]),
    "r3d_torso_conv3d": (c_int, [F, c_int, c_int, c_int, c_int, c_int, c_int, F, F, c_int, c_int, c_int, c_int, c_float, c_int, F, c_int, c_int, F,
                                 S]),
    "r3d_torso_motion_input": (c_int, [F, c_int, c_int, c_int, c_int, c_int, F, F, F, F, F, c_int, F, c_int, F, c_int, S]),
    "r3d_torso_motion_deform": (c_int, [F, c_int, c_int, c_int, c_int, c_int, F, F, F, F, S]),
    "r3d_torso_motion_broadcast": (c_int, [F, c_int, c_int, c_int, c_int, c_int, F, c_int, c_int, S]),
    "r3d_torso_conv_prec": (c_int, [F, c_int, c_int, c_int, c_int, c_int, c_int, F, F, c_float, F, F, c_int, c_int, c_int, c_float, F, F, F, c_int,
                                    S]),
    "r3d_torso_conv3d_prec": (c_int, [F, c_int, c_int, c_int, c_int, c_int, c_int, F, F, c_int, c_int, c_int, c_int, c_float, c_int, F, c_int, c_int,
                                      F, c_int, S]),
    "r3d_torso_split_bf16x3": (c_int, [F, c_size_t, U16, U16, U16, S]),
    "r3d_torso_conv_pool": (c_int, [F, c_int, c_int, c_int, c_int, c_int, F, F, c_int, c_int, c_int, c_float, c_int, F, c_int, S]),
    "r3d_torso_conv_split": (c_int, [F, c_int, c_int, c_int, c_int, c_int, F, F, c_int, c_int, c_int, c_float, c_int, F, c_int, S]),
    "r3d_torso_conv3d_res": (c_int, [F, c_int, c_int, c_int, c_int, c_int, F, F, c_float, F, F, c_int, c_int, c_int, c_float, F, F, F, c_int, S]),
    "r3d_torso_seg_input": (c_int, [F, c_int, c_int, F, c_int, c_int, c_int, c_int, c_int, F, c_int, c_int, S]),
    "r3d_torso_mask_volume": (c_int, [F, c_int, c_int, c_int, c_int, c_int, F, c_int, c_int, c_int, c_int, c_int, c_int, c_int, F, F, S]),
    "r3d_raster_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "r3d_raster_forward": (c_int, [F, F, I32, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_int, c_float, c_float, I64, F, F,
                                   F, V, c_size_t, S]),
    "r3d_secc_blink_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "r3d_secc_blink": (c_int, [F, c_int, c_int, c_int, I32, F64, c_int, F, I32, V, c_size_t, S]),
    "r3d_face_vertex": (c_int, [F, F, F, c_int, c_int, c_int, F, F, F, F, c_int, c_float, c_int, F, S]),
    "r3d_face_landmarks": (c_int, [F, F, F, c_int, c_int, c_int, F, F, F, F, c_int, c_float, c_int, c_float, c_float, c_float, F, S]),
    # include/r3d_hip_clip.h
    "r3d_clip_camera": (c_int, [F, F, c_int, c_int, ctypes.c_double, F, S]),
    "r3d_camera_smooth": (c_int, [F, c_int, c_int, c_int, F, S]),
    "r3d_smooth_features": (c_int, [F, c_int, c_int, c_int, c_int, F, S]),
    # include/r3d_hip_video.h
    "r3d_video_depth_range": (c_int, [F, c_size_t, c_int, I32, S]),
    "r3d_video_compose_debug": (c_int, [F, F, c_int, c_int, F, c_int, c_int, F, c_int, c_int, F, c_int, c_int, c_int, c_int, I32, U8, S]),
    # include/r3d_hip_source.h; the darkening table and the blur weights of r3d_source_torso are HOST arrays
    "r3d_source_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "r3d_source_nearest": (c_int, [U8, c_int, c_int, c_int, I32, I32, I32, V, c_size_t, S]),
    "r3d_source_background": (c_int, [U8, U8, c_int, c_int, c_int, U8, I32, V, c_size_t, S]),
    "r3d_source_torso": (c_int, [U8, U8, c_int, c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int), U8, U8, U8, U8, V, c_size_t, S]),
    "r3d_source_select": (c_int, [U8, U8, c_int, c_int, c_int, U8, U8, S]),
    "r3d_source_to_planes": (c_int, [U8, U8, c_int, c_int, c_int, F, S]),
    # include/r3d_hip_audio.h
    "r3d_a2m_conv1d": (c_int, [F, c_int, c_int, c_int, c_int, c_int, c_int, F, F, c_int, c_int, c_int, c_int, c_int, F, F, I64, c_int, c_int, F, F, F, F, F, F,
                               c_int, c_int, c_int, S]),
    "r3d_a2m_wn_layer": (c_int, [F, F, c_int, c_int, c_int, c_int, c_int, F, F, F, F, F, c_int, c_int, F, F, S]),
    "r3d_a2m_pitch_embed": (c_int, [F, c_int, c_int, F, c_int, c_int, I32, F, S]),
    # include/r3d_hip_fit.h
    "r3d_fit_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "r3d_fit_state_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "r3d_fit_landmark_grad": (c_int, _FIT_COMMON + [F, F, F, F, F, F, F, F, F, V, c_size_t, S]),
    "r3d_fit_landmark_run": (c_int, _FIT_COMMON + [c_float, c_float, c_int, c_int, c_int, c_int, F, V, c_size_t, S]),
}

# Headers that r3d_hip.h does not include (each includes r3d_hip.h instead): header -> its table, lines as in SIGNATURES.  load() binds them
# the same way, and a library that lacks one of these functions does not load either; call() finds a name in whichever table holds it.
EXTENSION_SIGNATURES = {
    "r3d_hip_img2plane.h": {
        "r3d_i2p_attention": (c_int, [F, F, c_int, c_int, c_int, c_int, c_int, c_float, F, S]),
        "r3d_i2p_upsample2x": (c_int, [F, c_int, c_int, c_int, c_int, F, S]),
        "r3d_i2p_pixel_shuffle": (c_int, [F, c_int, c_int, c_int, c_int, F, c_int, c_int, S]),
        "r3d_i2p_copy_channels": (c_int, [F, c_size_t, c_int, F, c_int, c_int, S]),
        "r3d_i2p_nchw_to_cl": (c_int, [F, c_int, c_int, c_int, c_int, F, S]),
        "r3d_i2p_planes_out": (c_int, [F, c_int, c_int, c_int, c_int, F, S]),
    },
}

# Feature headers, each a stage of the pipeline of its own that includes r3d_hip.h: header -> its table, bound and found exactly as the
# extension tables are (required; same _bind).
FEATURE_SIGNATURES = {
    "r3d_hip_hubert.h": {
        "r3d_hubert_wave_stats": (c_int, [F, c_size_t, F64, S]),
        "r3d_hubert_conv0": (c_int, [F, F64, c_int, c_size_t, c_size_t, c_int, F, F, F, F, c_float, c_int, c_int, c_int, F, S]),
        "r3d_hubert_conv_ln_gelu": (c_int, [F, F, F, F, F, c_float, c_int, c_int, c_int, c_int, c_int, c_int, F, S]),
        "r3d_hubert_pos_conv": (c_int, [F, F, F, c_int, c_int, c_int, c_int, c_int, F, S]),
    },
    "r3d_hip_deeplab.h": {
        "r3d_dl_conv": (c_int, [F, c_int, c_int, c_int, c_int, F, F, c_int, c_int, c_int, c_int, c_int, c_int, F, c_int, F, c_int, c_int, S]),
        "r3d_dl_maxpool": (c_int, [F, c_int, c_int, c_int, c_int, F, S]),
        "r3d_dl_global_mean": (c_int, [F, c_int, c_int, c_int, F, S]),
        "r3d_dl_assemble_input": (c_int, [F, F, F, c_int, c_int, c_int, F, S]),
    },
}

# Module headers, each one torch module of a model restated (it includes r3d_hip.h): header -> its table, bound and found exactly as the
# extension and feature tables are (required; same _bind).
MODULE_SIGNATURES = {
    "r3d_hip_plane2grid.h": {
        "r3d_p2g_groupnorm_stats_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
        "r3d_p2g_groupnorm_stats": (c_int, [F, c_int, c_int, c_int, c_int, c_int, c_int, F, F, c_float, F, F, V, c_size_t, S]),
        "r3d_p2g_conv3d": (c_int, [F, c_int, c_int, c_int, c_int, c_int, F, F, F, F, c_int, F, F, F, S]),
    },
}

# The headers' constants the package uses: _lib.X mirrors R3D_X of the header named (tests/test_abi.py compares every one).
CHAIN_SR_BLOCK, CHAIN_CONV, CHAIN_SR_BLOCK_TAIL, CHAIN_SRC_NONE, CHAIN_MAX_OPS, CHAIN_MAX_EXT, CHAIN_MAX_ZERO = 0, 1, 2, -1000, 12, 4, 4      # r3d_hip.h
VIDEO_STATE_WORDS, VIDEO_PANELS_ALL, VIDEO_PANEL_DEPTH = 8, 31, 8                                           # r3d_hip_video.h
SOURCE_MAX_SIDE, SOURCE_STATUS_WORDS, SOURCE_DARKEN, SOURCE_HEAD_CLASSES = 2048, 2, 53, 42                  # r3d_hip_source.h
A2M_WN_ROWS = 16                                          # r3d_hip_audio.h: the time rows one block of r3d_a2m_wn_layer owns
FIT_LOSS_WORDS, FIT_LAUNCHES = 8, 2                       # r3d_hip_fit.h

# test hooks outside the C ABI of include/r3d_hip.h: bound when the library exports them, absent otherwise (nothing in the product calls
# them, and a library built from older sources -- the other side of a scripts/ab.py comparison, say -- must keep loading)
OPTIONAL_SIGNATURES = {
    "r3d_debug_merge_fallbacks": (c_int, [ctypes.POINTER(ctypes.c_ulonglong), c_int]),
    # r3d_raster_forward with the large-face threshold and a stage mask (1 clear, 2 scatter, 4 large_faces, 8 resolve) in front of the stream
    "r3d_debug_raster_forward": (c_int, [F, F, I32, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_int, c_float, c_float,
                                         I64, F, F, F, V, c_size_t, c_int, c_int, S]),
    # r3d_secc_blink with a stage mask (1 clear, 2 quantise_bounds, 4 erode, 8 columns, 16 fill) in front of the stream
    "r3d_debug_secc_blink": (c_int, [F, c_int, c_int, c_int, I32, F64, c_int, F, I32, V, c_size_t, c_int, S]),
    # the launch plans of the clip stage's two frame-walking kernels, host arithmetic only (no HIP call): (L, Ki, Ke, T) -> V, slabs, chunk,
    # ychunks, nsplit, Kc, lds_bytes, ws_floats of fit_grad; (N, Ki, Ke, T) -> V, xblocks, chunk, yblocks, lds_bytes of face_model
    "r3d_debug_fit_plan": (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int32)]),
    "r3d_debug_face_plan": (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int32)]),
}


class ChainOp(ctypes.Structure):
    """r3d_chain_op of include/r3d_hip.h (one layer of an r3d_chain_fold chain)."""
    _fields_ = [("kind", c_int), ("Cin", c_int), ("Cout", c_int), ("ksize", c_int), ("act", c_int),
                ("gain", c_float), ("clamp", c_float), ("src_a", c_int), ("src_b", c_int),
                ("scales", c_void_p), ("prepacked", c_void_p), ("bias", c_void_p)]


ABI_VERSION = 80          # r3d_version() of the library this table mirrors (include/r3d_hip.h)
_lib = None
_torch = None             # the torch module, from load() on (this module does not import it)
_Tensor = ()
_plans = {}               # name -> (parameter count, ends with the stream, ((position, element, dtypes or None) per device pointer), returns a status)
_calls = None             # the list of the innermost counting() block


def build(force=False):
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-s", "-C", CSRC, "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


def _bind(fn, name, res, params, torch):
    """ctypes types of one table line onto `fn`, and call()'s plan for it."""
    fn.restype, fn.argtypes = res, [getattr(p, "ctype", p) for p in params]
    dtypes = lambda names: names and tuple(getattr(torch, d) for d in names if hasattr(torch, d))        # (torch.uint16: newer versions only)
    dev = tuple((i, p.elem, dtypes(DevPtr.DTYPES[p.elem])) for i, p in enumerate(params) if isinstance(p, DevPtr))
    # every int-returning entry point returns an r3d_status, except r3d_version
    _plans[name] = (len(params), bool(params) and isinstance(params[-1], Stream), dev, res is c_int and name != "r3d_version")


def load():
    """Load libr3d_hip.so; raises RuntimeError (never falls back) when it is absent."""
    global _lib, _torch, _Tensor
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64.so.7; it must be the HIP runtime of the process (one runtime, one
    # set of streams/devices), so make sure it is mapped before our library asks the loader for that SONAME.
    import torch
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "real3dportrait_amd: HIP extension %s not built -- run `make -C %s` (there is no CPU/eager fallback)"
            % (LIB_PATH, CSRC))
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise RuntimeError("real3dportrait_amd: cannot load %s: %s" % (LIB_PATH, e))
    required = dict(SIGNATURES)
    for table in list(EXTENSION_SIGNATURES.values()) + list(FEATURE_SIGNATURES.values()) + list(MODULE_SIGNATURES.values()):
        required.update(table)
    for name, (res, params) in required.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:       # functions are added without a new ABI number: a stale in-tree build lacks them
            raise RuntimeError("real3dportrait_amd: %s does not export %s, which this package binds -- rebuild it (`make -C %s`)"
                               % (LIB_PATH, name, CSRC))
        _bind(fn, name, res, params, torch)
    for name, (res, params) in OPTIONAL_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            _bind(fn, name, res, params, torch)
    if lib.r3d_version() != ABI_VERSION:      # a stale in-tree build (real3dportrait_amd/lib/ is not tracked): arguments would be shifted silently
        raise RuntimeError("real3dportrait_amd: %s reports ABI %d, this package binds ABI %d -- rebuild it (`make -C %s`)"
                           % (LIB_PATH, lib.r3d_version(), ABI_VERSION, CSRC))
    _torch, _Tensor = torch, torch.Tensor
    _lib = lib
    return lib


def call(name, *args):
    """The one way from the package into the library: lib.<name>(*args) with every device pointer checked.

    A device-pointer parameter (DevPtr in the table) takes None (NULL), an int (an address), a ctypes object, or a tensor, which must have
    a dtype of the declared element type, be contiguous and live on a GPU -- checked in that order, each failure a TypeError / ValueError
    naming the function and the parameter's position (from 0), raised before the library is entered.  When the table line ends with the
    stream and the caller gave one argument fewer, the current stream is passed.  A status other than 0 raises as check() does; entry
    points that return a value (*_bytes, *_offset, r3d_version, r3d_last_error) return it."""
    lib = load()
    n, stream, dev, status = _plans[name]
    args = list(args)
    add_stream = stream and len(args) == n - 1
    if len(args) != n and not add_stream:
        raise TypeError("libr3d_hip %s takes %d arguments%s, got %d" % (name, n, " (the stream may be left out)" if stream else "", len(args)))
    for i, elem, dtypes in dev:
        t = args[i]
        if isinstance(t, _Tensor):
            if dtypes is not None and t.dtype not in dtypes:
                raise TypeError("libr3d_hip %s: argument %d is a %s*, got a %s tensor" % (name, i, elem, t.dtype))
            if not t.is_contiguous():
                raise ValueError("libr3d_hip %s: argument %d (%s*) is not contiguous" % (name, i, elem))
            if not t.is_cuda:
                raise ValueError("libr3d_hip %s: argument %d (%s*) is not on a GPU: the library operates on device tensors only" % (name, i, elem))
            args[i] = t.data_ptr()
    if add_stream:
        args.append(_torch.cuda.current_stream().cuda_stream)
    if _calls is not None:
        _calls.append((name, tuple(args)))
    rc = getattr(lib, name)(*args)
    if not status:
        return rc
    if rc != 0:
        check(rc, name[4:])


@contextlib.contextmanager
def counting():
    """Records (entry point, marshalled arguments) of every call() made inside the block, in order, just before the library is entered;
    yields the list.  A call refused by call()'s own checks is not recorded."""
    global _calls
    outer, _calls = _calls, []
    try:
        yield _calls
    finally:
        _calls = outer


def check(rc, what=""):
    if rc != 0:
        msg = load().r3d_last_error()
        raise RuntimeError("libr3d_hip %s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def ptr(t):
    """Raw device pointer of a contiguous CUDA(HIP) tensor (or None): for code that drives the raw C ABI (tests, bench.py)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("libr3d_hip operates on device tensors only")
    if not t.is_contiguous():
        raise ValueError("libr3d_hip takes contiguous tensors")
    return t.data_ptr()


def stream_ptr():
    load()
    return _torch.cuda.current_stream().cuda_stream
