"""CPU: the host side of the HIP mesh rasteriser (real3dportrait_amd/mesh_renderer.py, r3d_raster_forward of include/r3d_hip.h,
DESIGN 4.14).

The symbols, the argument check of the C entry point (which runs before any HIP call), the restatement of the rule
(tests/raster_ref64.py) on cases computed by hand, the fp32 restatement's own distance from fp64 on the GPU tests' inputs, and the
kernels' scratch use."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
import raster_ref64 as R64
from real3dportrait_amd import synth

FOV90 = 90.0                    # s = 1: NDC = (x, y) / z
FACE_CASES = [(64, 24), (96, 40), (128, 64)]          # (S, G), seed 0


def face_case(S, G, seeds=(0,)):
    """B = len(seeds) face-like meshes with one shared tri: (vertex [B, N, 3], tri [M, 3], feat [B, N, 3])."""
    m = [synth.synth_face_mesh(G, s) for s in seeds]
    return np.stack([k["vertex"] for k in m]), m[0]["tri"], np.stack([k["feat"] for k in m])


def cap(S):
    """pix_to_face may differ from fp64 in at most 0.1 % of an image's pixels."""
    return (S * S) // 1000


def test_symbols_are_declared_exported_and_bound():
    from real3dportrait_amd import _lib
    import real3dportrait_amd
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "r3d_hip.h")).read()
    for name in ("r3d_raster_workspace_bytes", "r3d_raster_forward"):          # (header against table: tests/test_abi.py)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "r3d_debug_raster_forward" in _lib.OPTIONAL_SIGNATURES and "r3d_debug_raster_forward" not in header
    assert len(_lib.OPTIONAL_SIGNATURES["r3d_debug_raster_forward"][1]) == len(_lib.SIGNATURES["r3d_raster_forward"][1]) + 2
    from real3dportrait_amd import mesh_renderer
    assert real3dportrait_amd.MeshRenderer is mesh_renderer.MeshRenderer and real3dportrait_amd.rasterize is mesh_renderer.rasterize
    assert real3dportrait_amd.patch_secc_renderer is mesh_renderer.patch_secc_renderer


def test_workspace_bytes():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    # 8-byte keys in tiles of 4 x 2 pixels, 256 bytes for the list length, one 4-byte list slot per face rounded up to 256 bytes
    assert lib.r3d_raster_workspace_bytes(1, 512, 70000) == 512 * 512 * 8 + 256 + (70000 * 4 + 255) // 256 * 256
    assert lib.r3d_raster_workspace_bytes(2, 5, 3) == 2 * (2 * 3 * 8) * 8 + 256 + 256          # 5 x 5 pixels: 2 x 3 tiles
    assert lib.r3d_raster_workspace_bytes(50, 512, 141376) < 1 << 28
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 16385, 4), (1 << 16, 4, 1 << 15), (1 << 12, 1024, 4)):
        assert lib.r3d_raster_workspace_bytes(*bad) == 0, bad


def test_c_entry_point_rejects_bad_arguments_without_a_gpu():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)              # never dereferenced: validation fails first
    err = lambda: lib.r3d_last_error()
    need = lib.r3d_raster_workspace_bytes(2, 64, 100)

    def call(vertex=P(1), feat=P(2), tri=P(3), B=2, N=50, M=100, C=3, S=64, fov=12.6, znear=5.0, p2f=P(4), mask=P(5), depth=P(6),
             image=P(7), ws=P(8), ws_bytes=need):
        return lib.r3d_raster_forward(vertex, feat, tri, 0, B, N, M, C, S, fov, znear, 1, 1, 1.0, 0.0, p2f, mask, depth, image, ws, ws_bytes, None)

    for k in ("vertex", "tri", "mask", "depth"):
        assert call(**{k: None}) == -1 and b"NULL pointer" in err(), k
    assert call(feat=None) == -1 and b"feat and image" in err()
    assert call(image=None) == -1 and b"feat and image" in err()
    for S in (0, -3, 16385):
        assert call(S=S) == -1 and b"image size S" in err(), S
    for C in (0, 5, -1):
        assert call(C=C) == -1 and b"attribute channels" in err(), C
    assert call(B=0) == -1 and b"must be positive" in err()
    assert call(M=0) == -1 and b"must be positive" in err()
    assert call(N=0) == -1 and b"must be positive" in err()
    assert call(B=1 << 16, M=1 << 15, S=1, ws_bytes=1 << 62) == -1 and b"31-bit face index" in err()
    assert call(B=1 << 12, S=1024, ws_bytes=1 << 62) == -1 and b"2^31" in err()
    for fov in (0.0, 180.0, -10.0, 200.0, float("nan"), float("inf")):
        assert call(fov=fov) == -1 and b"fov_deg" in err(), fov
    assert call(znear=float("nan")) == -1 and b"NaN" in err()
    assert call(ws=None) == -2 and b"NULL workspace" in err()
    assert call(ws_bytes=need - 1) == -2 and b"needed" in err()
    assert call(ws_bytes=0) == -2 and b"needed" in err()
    assert call(ws=ctypes.c_void_p((8 << 32) + 4)) == -2 and b"aligned" in err()
    dbg = lib.r3d_debug_raster_forward
    args = (P(1), P(2), P(3), 0, 2, 50, 100, 3, 64, 12.6, 5.0, 1, 1, 1.0, 0.0, P(4), P(5), P(6), P(7), P(8), need)
    assert dbg(*args, -1, 15, None) == -1 and b"test-hook" in err()
    assert dbg(*args, 64, 16, None) == -1 and b"test-hook" in err()


def test_python_wrapper_refuses_malformed_input_before_the_library():
    import torch
    from real3dportrait_amd import rasterize
    v, t = torch.zeros(1, 4, 3), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="vertex must be"):
        rasterize(torch.zeros(4, 3), t, 8, 30.0, 0.1)
    with pytest.raises(ValueError, match="tri must be"):
        rasterize(v, torch.zeros(2, 4, dtype=torch.int64), 8, 30.0, 0.1)
    with pytest.raises(ValueError, match="differ in B"):
        rasterize(v, torch.zeros(2, 2, 3, dtype=torch.int64), 8, 30.0, 0.1)
    with pytest.raises(ValueError, match="feat must be"):
        rasterize(v, t, 8, 30.0, 0.1, feat=torch.zeros(1, 5, 3))
    with pytest.raises(ValueError, match="empty input"):
        rasterize(v, torch.zeros(0, 3, dtype=torch.int64), 8, 30.0, 0.1)


def one_triangle():
    """Camera-space corners (-0.875, 0.875), (-0.875, -0.375), (0.375, 0.875) at z = 1 under s = 1.  The reference negates x: NDC
    (0.875, 0.875), (0.875, -0.375), (-0.375, 0.875), the right angle at the image's TOP LEFT (+x is left, +y is up), the hypotenuse
    on x + y = 1/2.  Every number is dyadic: the arithmetic of the rule is exact in both formats."""
    v = np.array([[[-0.875, 0.875, 1.0], [-0.875, -0.375, 1.0], [0.375, 0.875, 1.0]]], np.float32)
    return v, np.array([[0, 1, 2]])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_on_one_triangle_by_hand(dtype):
    """S = 4: centres at NDC 0.75, 0.25, -0.25, -0.75 for columns 0 .. 3 (and rows 0 .. 3).  Strictly inside x < 0.875, y < 0.875,
    x + y > 0.5: (0.75, 0.75), (0.75, 0.25), (0.25, 0.75) = (row, column) (0, 0), (1, 0), (0, 1).  The centres (0.25, 0.25),
    (0.75, -0.25) and (-0.25, 0.75) lie exactly ON the hypotenuse and are not covered."""
    v, tri = one_triangle()
    feat = np.array([[[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]], np.float32)
    r = R64.rasterize(v, tri, feat, 4, FOV90, 0.1, dtype, first_face_is_background=False)
    want = np.full((4, 4), -1)
    want[0, 0] = want[1, 0] = want[0, 1] = 0
    assert np.array_equal(r["pix_to_face"][0], want)
    assert np.array_equal(r["mask"][0, 0], (want == 0).astype(dtype))
    assert np.array_equal(r["depth"][0, 0], (want == 0).astype(dtype))          # every corner at z = 1
    # barycentrics at the centre (0.75, 0.75) by areas: w1 (towards the lower corner) = 0.125 / 1.25 = 0.1, w2 = 0.1, w0 = 0.8
    assert np.allclose(r["bary"][0, 0, 0], [0.8, 0.1, 0.1], rtol=0, atol=1e-6)
    assert np.allclose(r["image"][0, :, 0, 0], [0.8, 0.1], rtol=0, atol=1e-6) and r["image"][0, 0, 3, 3] == 0
    # the reference's mask: pix_to_face > 0 makes face 0 of the first mesh background, everywhere
    q = R64.rasterize(v, tri, feat, 4, FOV90, 0.1, dtype)
    assert np.array_equal(q["pix_to_face"], r["pix_to_face"]) and not q["mask"].any() and not q["depth"].any() and not q["image"].any()
    # without the negation the triangle sits at the top RIGHT
    n = R64.rasterize(v, tri, None, 4, FOV90, 0.1, dtype, negate_x=False)
    assert np.array_equal(n["pix_to_face"][0], want[:, ::-1]) and n["image"] is None
    # the other winding draws the same pixels
    w = R64.rasterize(v, tri[:, ::-1], None, 4, FOV90, 0.1, dtype)
    assert np.array_equal(w["pix_to_face"][0], want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_depth_test_and_tie(dtype):
    """Face 0 far (z = 4, the same NDC triangle), faces 1 and 2 the SAME corners at z = 2, face 3 nearer (z = 1.5) over a part: the tie of 1
    and 2 goes to the lower index; 3 wins where it covers; 0 never shows.  Perspective: a face across depths 1 and 3 reads
    pz = 1 / ((1 - t) / 1 + t / 3) at screen fraction t, not 1 + 2 t."""
    v0, _ = one_triangle()
    corner = v0[0]
    v = np.concatenate([corner * 4, corner * 2, corner * 1.5])[None].astype(np.float32)
    v[0, 6:9, :2] = np.array([[-0.875, 0.875], [-0.875, 0.375], [-0.375, 0.875]]) * 1.5          # NDC (0.875, 0.875), (0.875, 0.375), (0.375, 0.875)
    tri = np.array([[0, 1, 2], [3, 4, 5], [3, 4, 5], [6, 7, 8]])
    r = R64.rasterize(v, tri, None, 4, FOV90, 0.1, dtype)
    want = np.full((4, 4), -1)
    want[1, 0] = want[0, 1] = 1
    want[0, 0] = 3                    # (0.75, 0.75): x + y = 1.5 > 1.25 inside face 3
    assert np.array_equal(r["pix_to_face"][0], want)
    assert np.allclose(r["depth"][0, 0], np.where(want == 1, 2.0, np.where(want == 3, 1.5, 0.0)), rtol=0, atol=1e-6)
    # a long thin face along the top row from depth 1 (left) to depth 3 (right)
    v = np.array([[[-0.99 * 1, 0.99 * 1, 1.0], [-0.99 * 1, 0.51 * 1, 1.0], [0.99 * 3, 0.75 * 3, 3.0]]], np.float32)
    r = R64.rasterize(v, np.array([[0, 1, 2]]), None, 4, FOV90, 0.1, dtype, first_face_is_background=False)
    for j, x in enumerate((0.75, 0.25, -0.25, -0.75)):
        if r["pix_to_face"][0, 0, j] < 0:
            continue
        t = (0.99 - x) / 1.98
        assert abs(r["depth"][0, 0, 0, j] - 1.0 / ((1 - t) + t / 3.0)) < 1e-5, j
    assert (r["pix_to_face"][0, 0] >= 0).sum() >= 2


def test_restatement_drops_the_faces_of_rule_7():
    v0, tri = one_triangle()
    base = R64.rasterize(v0 * 8, tri, None, 4, FOV90, 5.0, first_face_is_background=False)          # z = 8 >= znear / 2
    assert (base["pix_to_face"] >= 0).sum() == 3
    near = v0 * 2                                                                                  # z = 2 < 2.5
    assert (R64.rasterize(near, tri, None, 4, FOV90, 5.0)["pix_to_face"] == -1).all()
    for bad in (np.nan, np.inf):
        w = (v0 * 8).copy()
        w[0, 1, 0] = bad
        assert (R64.rasterize(w, tri, None, 4, FOV90, 5.0)["pix_to_face"] == -1).all()
    assert (R64.rasterize(v0 * 8, np.array([[0, 1, 3]]), None, 4, FOV90, 5.0)["pix_to_face"] == -1).all()          # an index past N
    assert (R64.rasterize(v0 * 8, np.array([[0, -1, 2]]), None, 4, FOV90, 5.0)["pix_to_face"] == -1).all()
    assert (R64.rasterize(v0 * 8, np.array([[0, 1, 1]]), None, 4, FOV90, 5.0)["pix_to_face"] == -1).all()          # zero area


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_boxes_lose_no_pixel(dtype):
    """The per-face pixel boxes of the restatement against testing every face at every pixel."""
    v, tri, feat = face_case(24, 6, seeds=(3, 4))
    a = R64.rasterize(v, tri, feat, 24, synth.BFM_FOV_DEG, 5.0, dtype)
    b = R64.rasterize(v, tri, feat, 24, synth.BFM_FOV_DEG, 5.0, dtype, brute=True)
    for k in ("pix_to_face", "mask", "depth", "image", "bary"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["pix_to_face"] >= 0).mean() > 0.8


def test_synth_face_mesh():
    m = synth.synth_face_mesh(24, 0)
    assert m["vertex"].shape == (2 * 25 * 25, 3) and m["tri"].shape == (4 * 24 * 24, 3) and m["feat"].shape == (2 * 25 * 25, 3)
    assert m["vertex"].dtype == np.float32 and m["tri"].dtype == np.int64 and m["tri"].min() == 0 and m["tri"].max() == 2 * 25 * 25 - 1
    assert 8.4 < m["vertex"][:, 2].min() and m["vertex"][:, 2].max() < 10.5
    assert synth.synth_face_mesh(188, 0)["tri"].shape[0] == 141376 and synth.synth_face_mesh(132, 0)["tri"].shape[0] == 69696
    assert not np.array_equal(m["vertex"], synth.synth_face_mesh(24, 1)["vertex"])
    r = R64.rasterize(m["vertex"][None], m["tri"], None, 64, synth.BFM_FOV_DEG, 5.0)
    cover = (r["pix_to_face"] >= 0).mean()
    front = (r["pix_to_face"] >= 2 * 24 * 24).mean()                    # the nearer layer wins its pixels
    print("coverage %.3f, nearer layer %.3f" % (cover, front))
    assert 0.88 < cover < 0.99 and 0.05 < front < 0.2


@pytest.mark.parametrize("S,G", FACE_CASES)
def test_fp32_restatement_meets_the_cap_on_the_test_inputs(S, G):
    """The condition the GPU tests hold the kernel to, met by an fp32 evaluation of the rule itself: measured here 0 differing pixels at
    all three sizes."""
    v, tri, feat = face_case(S, G)
    r64 = R64.rasterize(v, tri, feat, S, synth.BFM_FOV_DEG, 5.0, np.float64)
    r32 = R64.rasterize(v, tri, feat, S, synth.BFM_FOV_DEG, 5.0, np.float32)
    c = R64.compare(r32, r64)
    print("S %d G %d: fp32 restatement against fp64: %d differing pixels of %d, max |d depth| %.2e, max |d image| %.2e"
          % (S, G, c["differing"], c["pixels"], c["depth"], c["image"]))
    assert c["differing"] <= cap(S)
    assert c["depth"] < 1e-4 and c["image"] < 1e-4          # fp32 at depth 10 and attributes below 1: far inside this


def test_raster_kernels_do_not_use_scratch():
    from test_render_kernel_resources import _kernel_metadata
    from real3dportrait_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    names = sorted(k for k in meta if "6raster" in k)
    assert len(names) == 3 and [n for n in names if "scatter" in n] and [n for n in names if "large_faces" in n] and \
        [n for n in names if "resolve" in n], names
    for k in names:
        assert int(meta[k]["private_segment_fixed_size"]) == 0, (k, meta[k])
        assert int(meta[k]["vgpr_spill_count"]) == 0 and int(meta[k]["sgpr_spill_count"]) == 0, (k, meta[k])
