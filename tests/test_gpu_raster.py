"""GPU: the HIP mesh rasteriser (real3dportrait_amd/mesh_renderer.py, r3d_raster_forward) against the fp64 restatement of
the rule (tests/raster_ref64.py).

The conditions, none of them derived from the kernel's output:
  * pix_to_face may differ from fp64 in at most 0.1 % of the pixels of an image (cap(S) = S S // 1000 pixels: 4 at S = 64, 0 below
    S = 32).  The fp32 restatement of the rule meets it with 0 (tests/test_raster_host.py).
  * on the pixels where the faces agree, the errors of depth and image are at most 4 x the fp32 restatement's own largest error against
    fp64 on the same input, computed here (the GPU contracts to fma and divides differently from NumPy).  For the images of fewer than
    1 000 pixels (S = 1, S = 5) that largest error is taken to be at least FLOORS, from the number formats (see there).
Measured on an MI355X (pytest -s prints them): DESIGN 4.14.
"""
import functools

import numpy as np
import pytest
import torch

import raster_ref64 as R64
from test_raster_host import cap, face_case
from real3dportrait_amd import synth

pytestmark = pytest.mark.gpu
FOV, ZNEAR = synth.BFM_FOV_DEG, 5.0
DEV = "cuda:0"


def run(v, tri, feat, S, fov=FOV, znear=ZNEAR, **kw):
    """rasterize on the GPU from NumPy inputs, as NumPy."""
    from real3dportrait_amd import rasterize
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    p2f, mask, depth, image = rasterize(T(v), T(tri), S, fov, znear, feat=T(feat), **kw)
    assert p2f.dtype == torch.int64 and tuple(p2f.shape) == (v.shape[0], S, S)
    assert mask.dtype == depth.dtype == torch.float32 and tuple(mask.shape) == tuple(depth.shape) == (v.shape[0], 1, S, S)
    return {"pix_to_face": p2f.cpu().numpy(), "mask": mask.cpu().numpy(), "depth": depth.cpu().numpy(),
            "image": None if image is None else image.cpu().numpy()}


# Where an image has too few pixels for the fp32 restatement's largest error to mean much (S = 1: one pixel, whose fp32 error can be 0 by
# luck), the bound does not go below what the formats give on small_mesh: a barycentric carries about 2^-23 / l of absolute error from
# the rounding of the coordinate differences of a face whose shortest NDC extent is l (>= 1/16 there, so 16 x 2^-23 for an attribute
# in [0, 1)), and the depth, whose range within a face is small, one rounding of a number in [8, 16): 2^-20.
FLOORS = {"depth": 2.0 ** -20, "image": 16 * 2.0 ** -23}


def check(got, v, tri, feat, S, what, fov=FOV, znear=ZNEAR, floors=None, **kw):
    """The two conditions of the module docstring (floors: FLOORS for the images of a few pixels); returns the fp64 result."""
    r64 = R64.rasterize(v, tri, feat, S, fov, znear, np.float64, **kw)
    own = R64.compare(R64.rasterize(v, tri, feat, S, fov, znear, np.float32, **kw), r64)
    c = R64.compare(got, r64)
    keys = ("depth",) + (("image",) if feat is not None else ())
    if floors:
        own = dict(own, **{k: max(own[k], floors[k]) for k in keys})
    print("%s: %d differing pixels of %d (cap %d; the fp32 restatement %d); " % (what, c["differing"], c["pixels"], cap(S), own["differing"])
          + "; ".join("%s error %.2e, bound 4 x %.2e" % (k, c[k], own[k]) for k in keys))
    assert c["differing"] <= cap(S), (what, c)
    for k in keys:
        assert c[k] <= 4.0 * own[k], (what, k, c[k], own[k])
    same = got["pix_to_face"] == r64["pix_to_face"]
    assert np.array_equal(got["mask"][:, 0][same], r64["mask"][:, 0][same].astype(np.float32))
    return r64


def equal(a, b, keys=("pix_to_face", "mask", "depth", "image")):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k], b[k]), k


@functools.lru_cache(maxsize=None)
def small_mesh(G=8, seed=5):
    m = synth.synth_face_mesh(G, seed)
    return m["vertex"][None], m["tri"], m["feat"][None]


@pytest.mark.parametrize("S,G", [(64, 24), (96, 40)])
def test_face_like_mesh(S, G):
    v, tri, feat = face_case(S, G, seeds=(0, 1))
    assert not np.array_equal(v[0], v[1])
    got = run(v, tri, feat, S)
    r64 = check(got, v, tri, feat, S, "face-like mesh S %d G %d B 2" % (S, G))
    assert (r64["pix_to_face"] >= 0).mean() > 0.9
    assert got["pix_to_face"][1].max() >= tri.shape[0] and got["pix_to_face"][0].max() < tri.shape[0]
    # empty pixels are 0 in all three
    empty = got["pix_to_face"] == -1
    assert empty.any() and not got["mask"][:, 0][empty].any() and not got["depth"][:, 0][empty].any()
    assert not got["image"][np.broadcast_to(empty[:, None], got["image"].shape)].any()


def test_packed_index_and_the_first_face_quirk():
    v1, tri, f1 = small_mesh()
    v, feat, M, S = np.concatenate([v1, v1]), np.concatenate([f1, f1]), tri.shape[0], 33
    got = run(v, tri, feat, S)
    r64 = check(got, v, tri, feat, S, "packed index, first face background")
    assert (r64["pix_to_face"][0] == 0).sum() >= 4                           # face 0 is visible
    zero = got["pix_to_face"][0] == 0
    assert zero.sum() >= 4 and np.array_equal(got["pix_to_face"][1] == M, zero)
    assert not got["mask"][0, 0][zero].any() and not got["depth"][0, 0][zero].any() and not got["image"][0][:, zero].any()
    assert got["mask"][1, 0][zero].all() and (got["depth"][1, 0][zero] > 8).all() and got["image"][1][:, zero].any()
    hit = got["pix_to_face"][0] >= 0
    assert np.array_equal(got["pix_to_face"][1][hit], got["pix_to_face"][0][hit] + M) and (got["pix_to_face"][1][~hit] == -1).all()
    drawn = run(v, tri, feat, S, first_face_is_background=False)
    check(drawn, v, tri, feat, S, "packed index, first face drawn", first_face_is_background=False)
    assert drawn["mask"][0, 0][zero].all() and (drawn["depth"][0, 0][zero] > 8).all() and drawn["image"][0][:, zero].any()
    equal(drawn, got, keys=("pix_to_face",))
    for k in ("mask", "depth", "image"):
        assert np.array_equal(drawn[k][1], got[k][1]), k
        assert np.array_equal(drawn[k][0][..., ~zero], got[k][0][..., ~zero]), k


def test_batched_tri_equals_per_mesh_calls():
    va, tri, fa = small_mesh()
    vb, _, fb = small_mesh(8, 6)
    M = tri.shape[0]
    tri_b = np.stack([tri, np.roll(tri[::-1], 1, axis=1)])                  # the second mesh: faces in reverse order, corners rotated
    v, feat, S = np.concatenate([va, vb]), np.concatenate([fa, fb]), 33
    got = run(v, tri_b, feat, S, first_face_is_background=False)
    check(got, v, tri_b, feat, S, "batched tri", first_face_is_background=False)
    for b in range(2):
        one = run(v[b:b + 1], tri_b[b], feat[b:b + 1], S, first_face_is_background=False)
        assert np.array_equal(np.where(one["pix_to_face"] >= 0, one["pix_to_face"] + b * M, -1)[0], got["pix_to_face"][b])
        for k in ("mask", "depth", "image"):
            assert np.array_equal(one[k][0], got[k][b]), (b, k)
    # int32 indices and an [M, 3] tri repeated over the batch give the same
    rep = run(np.concatenate([va, va]), np.stack([tri, tri]).astype(np.int32), np.concatenate([fa, fa]), S)
    equal(rep, run(np.concatenate([va, va]), tri, np.concatenate([fa, fa]), S))


@pytest.mark.parametrize("S", [1, 5, 33])
def test_sizes_that_fit_no_tile(S):
    v, tri, feat = small_mesh()
    got = run(v, tri, feat, S)
    r64 = check(got, v, tri, feat, S, "S %d" % S, floors=FLOORS if S * S < 1000 else None)
    assert (r64["pix_to_face"] >= 0).any()


def test_large_face_path():
    """One triangle over the whole image behind a small mesh at S = 128: its box holds 16 384 pixels, far above the threshold of 64, so
    it takes the wave-per-face kernel.  The result must be the restatement's, and the same bits as with the threshold raised so that
    the same face is walked by one lane, and as with the threshold at 0 (every face through the wave-per-face kernel)."""
    v1, tri1, f1 = small_mesh(16, 7)
    N = v1.shape[1]
    big = np.array([[-3.8, -1.9, 11.5], [3.8, -1.9, 11.5], [0.0, 5.1, 11.5]], np.float32)          # NDC (-3, -1.5), (3, -1.5), (0, 4)
    v = np.concatenate([v1, big[None]], axis=1)
    feat = np.concatenate([f1, np.array([[[0.25, 0.5, 0.75]] * 3], np.float32)], axis=1)
    tri = np.concatenate([tri1[:100], [[N, N + 1, N + 2]], tri1[100:]])
    S = 128
    got = run(v, tri, feat, S)
    r64 = check(got, v, tri, feat, S, "large face")
    assert (r64["pix_to_face"] == 100).mean() > 0.03 and (r64["pix_to_face"] >= 0).all()
    assert ((got["pix_to_face"] == 100) != (r64["pix_to_face"] == 100)).sum() <= cap(S) and (got["pix_to_face"] >= 0).all()
    equal(run(v, tri, feat, S, _large_box=1 << 30), got)
    equal(run(v, tri, feat, S, _large_box=0), got)


def test_large_face_path_with_more_faces_than_waves():
    """large_faces has a fixed grid of 2048 waves, a face per wave and step.  With the threshold at 0 every face of a face-like mesh is
    listed, and the fp64 restatement alone shows more than 2048 distinct faces winning a pixel: waves have to take a second step
    (`e += waves`), and what they draw there is seen.  The result must be the restatement's, and the same bits as with the default
    threshold and with the threshold raised so that no face is listed."""
    S, G = 128, 40
    v, tri, feat = face_case(S, G)
    got = run(v, tri, feat, S, _large_box=0)
    r64 = check(got, v, tri, feat, S, "every face through large_faces, S %d G %d" % (S, G))
    winners = np.unique(r64["pix_to_face"][r64["pix_to_face"] >= 0])
    print("distinct winning faces in fp64: %d of %d faces (large_faces has 2048 waves)" % (len(winners), tri.shape[0]))
    assert len(winners) > 2048
    equal(run(v, tri, feat, S), got)
    equal(run(v, tri, feat, S, _large_box=1 << 30), got)


def test_winding_changes_nothing():
    """Every triangle reversed: the same pixels, depths and attributes (to the rounding of another order of the same sums)."""
    v, tri, feat = face_case(64, 24, seeds=(0, 1))
    S = 64
    rev = np.ascontiguousarray(tri[:, ::-1])
    got = run(v, rev, feat, S)
    r64 = R64.rasterize(v, tri, feat, S, FOV, ZNEAR)
    own = R64.compare(R64.rasterize(v, rev, feat, S, FOV, ZNEAR, np.float32), r64)
    c = R64.compare(got, r64)
    print("reversed winding against the fp64 result of the original: %d differing pixels; depth %.2e (bound 4 x %.2e), image %.2e (4 x %.2e)"
          % (c["differing"], c["depth"], own["depth"], c["image"], own["image"]))
    assert c["differing"] <= cap(S) and c["depth"] <= 4 * own["depth"] and c["image"] <= 4 * own["image"]


def test_dropped_faces_contribute_nothing():
    v1, tri1, f1 = small_mesh()
    N, S = v1.shape[1], 33
    extra = np.array([[0.0, 0.0, 1.0], [0.3, 0.2, np.nan], [0.1, 0.1, 9.0]], np.float32)          # z = 1 < znear / 2; NaN; a point for the zero area
    v = np.concatenate([v1, extra[None]], axis=1)
    feat = np.concatenate([f1, np.ones((1, 3, 3), np.float32)], axis=1)
    c0, c1 = int(tri1[10, 0]), int(tri1[40, 1])
    bad = np.array([[N, c0, c1], [c0, N + 1, c1], [N + 2, N + 2, c0], [c0, c1, c1]])
    tri = np.concatenate([tri1, bad])
    base = run(v, tri1, feat, S)
    got = run(v, tri, feat, S)
    equal(got, base)
    check(got, v, tri, feat, S, "dropped faces")
    # the same faces in front of the list shift the indices and nothing else
    front = run(v, np.concatenate([bad, tri1]), feat, S, first_face_is_background=False)
    plain = run(v, tri1, feat, S, first_face_is_background=False)
    assert np.array_equal(front["pix_to_face"], np.where(plain["pix_to_face"] >= 0, plain["pix_to_face"] + 4, -1))
    equal(front, plain, keys=("mask", "depth", "image"))
    # an index past N is refused on the host
    from real3dportrait_amd import rasterize
    with pytest.raises(ValueError, match="vertex indices"):
        rasterize(torch.from_numpy(v).to(DEV), torch.from_numpy(np.concatenate([tri1, [[0, 1, N + 3]]])).to(DEV), S, FOV, ZNEAR)
    with pytest.raises(ValueError, match="vertex indices"):
        rasterize(torch.from_numpy(v).to(DEV), torch.from_numpy(np.concatenate([tri1, [[0, -1, 2]]])).to(DEV), S, FOV, ZNEAR)


def test_caller_tensors_are_left_alone():
    from real3dportrait_amd import rasterize
    v1, tri1, f1 = small_mesh()
    v, t, f = torch.from_numpy(v1).to(DEV), torch.from_numpy(tri1).to(DEV), torch.from_numpy(f1).to(DEV)
    v0, t0, f0 = v.clone(), t.clone(), f.clone()
    rasterize(v, t, 33, FOV, ZNEAR, feat=f)
    assert torch.equal(v, v0) and torch.equal(t, t0) and torch.equal(f, f0)
    no_flip = run(v1, tri1, f1, 33, negate_x=False)
    flipped = run(v1 * np.array([-1, 1, 1], np.float32), tri1, f1, 33)
    equal(no_flip, flipped)


def test_determinism_and_side_stream():
    from real3dportrait_amd import rasterize
    vn, trin, fn = face_case(64, 24, seeds=(0, 1))
    v, t, f = torch.from_numpy(vn).to(DEV), torch.from_numpy(trin).to(DEV), torch.from_numpy(fn).to(DEV)
    a = rasterize(v, t, 64, FOV, ZNEAR, feat=f)
    b = rasterize(v, t, 64, FOV, ZNEAR, feat=f)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = rasterize(v, t, 64, FOV, ZNEAR, feat=f)
    side.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_feat_none_and_channel_counts():
    from real3dportrait_amd import MeshRenderer, rasterize
    v, tri, f3 = small_mesh()
    S = 33
    none = run(v, tri, None, S)
    assert none["image"] is None
    check(none, v, tri, None, S, "feat None")
    ren = MeshRenderer(FOV, znear=ZNEAR, zfar=15.0, rasterize_size=S, use_opengl=False)
    mask, depth, image = ren(torch.from_numpy(v).to(DEV), torch.from_numpy(tri).to(DEV))
    assert image is None and np.array_equal(mask.cpu().numpy(), none["mask"]) and np.array_equal(depth.cpu().numpy(), none["depth"])
    for C in (1, 4):
        feat = synth.hash_uniform(11, v.shape[1] * C, stream=C).reshape(1, -1, C)
        got = run(v, tri, feat, S)
        assert got["image"].shape == (1, C, S, S)
        check(got, v, tri, feat, S, "C %d" % C)
        equal(got, none, keys=("pix_to_face", "mask", "depth"))
    p2f, _, _, _ = rasterize(torch.from_numpy(v).to(DEV), torch.from_numpy(tri).to(DEV), S, FOV, ZNEAR, want_pix_to_face=False)
    assert p2f is None
    with pytest.raises(RuntimeError, match="attribute channels"):
        run(v, tri, np.zeros((1, v.shape[1], 5), np.float32), S)


class StubFaceModel:
    """compute_face_vertex of ParametricFaceModel, stood in for: a fixed mesh moved by the coefficients (BFM data does not exist here)."""

    def __init__(self, vertex):
        self.vertex = vertex

    def compute_face_vertex(self, id, exp, euler, trans):
        return self.vertex[None] + 0.02 * torch.stack([id[:, 0], exp[:, 0], euler[:, 0] + trans[:, 0]], dim=1)[:, None, :]


class StubSECCRenderer(torch.nn.Module):
    """The attributes and the forward of SECC_Renderer (deep_3drecon/secc_renderer.py:10-58) over a synthetic mesh."""

    def __init__(self, S):
        super().__init__()
        m = synth.synth_face_mesh(12, 21)
        self.face_model = StubFaceModel(torch.from_numpy(m["vertex"]).to(DEV))
        self.fov, self.znear, self.zfar = FOV, 5.0, 15.0
        self.face_renderer = torch.nn.Identity()          # the reference's MeshRenderer would need pytorch3d
        self.face_renderer.rasterize_size = S
        self.face_feat = torch.from_numpy(m["feat"]).to(DEV).unsqueeze(0)
        self.face_buf = torch.from_numpy(m["tri"]).to(DEV)

    def forward(self, id, exp, euler, trans):
        bs, btc = id.shape[0], id.ndim == 3
        if btc:
            t = id.shape[1]
            bs = bs * t
            id, exp, euler, trans = (x.reshape(bs, -1) for x in (id, exp, euler, trans))
        vertex = self.face_model.compute_face_vertex(id, exp, euler, trans)
        mask, _, secc = self.face_renderer(vertex, self.face_buf.unsqueeze(0).repeat([bs, 1, 1]), feat=self.face_feat.repeat([bs, 1, 1]))
        secc = (secc - 0.5) / 0.5
        if btc:
            mask, secc = (x.reshape(bs // t, t, *x.shape[1:]).permute(0, 2, 1, 3, 4) for x in (mask, secc))
        return mask, secc


def test_patch_secc_renderer():
    from real3dportrait_amd import MeshRenderer, patch_secc_renderer, rasterize
    S, bs = 48, 3
    coef = [torch.from_numpy(synth.hash_unitvar(30 + k, (bs, 4))).to(DEV) for k in range(4)]
    r = StubSECCRenderer(S)
    fwd = r.forward
    assert patch_secc_renderer(r) is r
    assert isinstance(r.face_renderer, MeshRenderer) and r.face_renderer.rasterize_size == S and r.face_renderer.fov == FOV
    assert (r.face_renderer.znear, r.face_renderer.zfar) == (5.0, 15.0) and r.forward == fwd and not hasattr(r, "_r3d_reference_forward")
    mask, secc = r(*coef)
    vertex = r.face_model.compute_face_vertex(*coef)
    p0, m0, d0, image = rasterize(vertex, r.face_buf, S, FOV, 5.0, feat=r.face_feat.repeat(bs, 1, 1))
    assert tuple(mask.shape) == (bs, 1, S, S) and tuple(secc.shape) == (bs, 3, S, S)
    assert torch.equal(mask, m0) and torch.equal(secc, (image - 0.5) / 0.5) and torch.equal(secc, 2 * image - 1)
    assert 0.5 < float(mask.mean()) < 1 and bool((secc[(mask == 0).expand_as(secc)] == -1).all())          # background: (0 - 0.5) / 0.5
    # against the restatement, through the class
    v_np, f_np = vertex.cpu().numpy(), r.face_feat.repeat(bs, 1, 1).cpu().numpy()
    check({"pix_to_face": p0.cpu().numpy(), "mask": mask.cpu().numpy(), "depth": d0.cpu().numpy(), "image": image.cpu().numpy()},
          v_np, r.face_buf.cpu().numpy(), f_np, S, "SECC stub")
    # the affine folded into the resolve kernel: the same map to 1 ulp (of values in [-1, 1])
    f = patch_secc_renderer(StubSECCRenderer(S), fold_affine=True)
    assert f.forward.__func__.__name__ == "_secc_forward_folded" and (f.face_renderer.out_scale, f.face_renderer.out_shift) == (2.0, -1.0)
    mask_f, secc_f = f(*coef)
    print("folded affine against (x - 0.5) / 0.5 in torch: max |difference| %.2e (1 ulp of 1 = %.2e)" % (float((secc_f - secc).abs().max()), 2.0 ** -23))
    assert torch.equal(mask_f, mask) and float((secc_f - secc).abs().max()) <= 2.0 ** -23
    # [B, T, C] coefficients come back as [B, C, T, H, W], from both forwards
    btc = [c.reshape(1, bs, 4) for c in coef]
    for ren, want in ((r, secc), (f, secc_f)):
        mk, sc = ren(*btc)
        assert tuple(mk.shape) == (1, 1, bs, S, S) and tuple(sc.shape) == (1, 3, bs, S, S)
        assert torch.equal(sc[0].transpose(0, 1), want) and torch.equal(mk[0].transpose(0, 1), mask)
