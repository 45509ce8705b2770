"""GPU: get_driving_motion (real3dportrait_amd/driving_motion.py) on stub SECC_Renderer / Face3DHelper / infer objects over
synth_face_model: bit-identical to the same steps written out from the package's public parts with the reference's host round trip, for
every chunk size; the identities the reference's function has; the maps against the fp64 rasteriser on fp64 vertices.

T = 131: three chunks of 50 with a ragged last one, two blink periods (the second cut off by the clip's end)."""
import random

import numpy as np
import pytest
import torch

import face_model_ref64 as F64
import raster_ref64 as R64
from real3dportrait_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 131
CASES = [(64, 24), (96, 40)]          # (S, G)
FP64_FRAMES = (0, 1, 49, 50, 130)     # the frames compared with the fp64 rasteriser: chunk starts and ends, the clip's last
_RUNS = {}


class _FaceModel:
    def __init__(self, m):
        self.mean_shape, self.id_base, self.exp_base, self.camera_distance = m["mean_shape"], m["id_base"], m["exp_base"], m["camera_distance"]


class _Rasterizer:
    def __init__(self, S):
        self.rasterize_size = S


class _SeccRenderer:
    """The attributes of SECC_Renderer (deep_3drecon/secc_renderer.py:10-32) that the package reads."""

    def __init__(self, m, S):
        self.face_model = _FaceModel(m)
        self.fov, self.znear, self.zfar = synth.BFM_FOV_DEG, 5.0, 15.0
        self.face_renderer = _Rasterizer(S)
        self.face_feat = torch.from_numpy(m["feat"])[None].to(DEV)
        self.face_buf = torch.from_numpy(m["tri"]).to(DEV)

    def forward(self, id, exp, euler, trans):
        raise AssertionError("the reference's forward is not part of this path")


class _Helper(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        for k in ("key_mean_shape", "key_id_base", "key_exp_base"):
            self.register_buffer(k, torch.from_numpy(m[k]))


class _Infer:
    def __init__(self, m, S):
        self.secc_renderer, self.face3d_helper = _SeccRenderer(m, S), _Helper(m).to(DEV)

    def get_driving_motion(self, id, exp, euler, trans, batch, inp):
        return "reference"


def composition(m, S, coeffs, seed):
    """The loop of real3d_infer.py:391-433 written from the package's public parts, with the reference's chunks of 50 and its .cpu() /
    cat / .cuda(): (un-blinked clip, blinked clip, src, cano, drv_kp, edits, status)."""
    from real3dportrait_amd import apply_periodic_blink, patch_face3d_helper, patch_face_model, rasterize
    idc, expc, euler, trans = coeffs
    fm, helper = patch_face_model(_FaceModel(m)), patch_face3d_helper(_Helper(m).to(DEV))
    tri, feat = torch.from_numpy(m["tri"]).to(DEV), torch.from_numpy(m["feat"])[None].to(DEV)
    zeros = torch.zeros(T, 3, device=DEV)

    def render(i, e, z):
        v = fm.compute_face_vertex(i, e, z, z)
        return rasterize(v, tri, S, synth.BFM_FOV_DEG, 5.0, feat=feat.expand(len(i), -1, -1), out_scale=2.0, out_shift=-1.0,
                         want_pix_to_face=False)[3]

    parts = [render(idc[i:i + 50], expc[i:i + 50], zeros[i:i + 50]).cpu() for i in range(0, T, 50)]
    plain = torch.cat(parts, dim=0).cuda()
    src = render(idc[0:1], expc[0:1], zeros[0:1])
    cano = render(idc[0:1], torch.zeros_like(expc[0:1]), zeros[0:1])
    drv = plain.clone()
    edits, status = apply_periodic_blink(drv, random.Random(seed))
    kp = torch.clamp((helper.reconstruct_lm2d(idc, expc, euler, trans) - 0.5) / 0.5, -1, 1)
    return plain, drv, src, cano, kp, edits, status


def run(S, G):
    """Everything the tests of one size share, computed once."""
    if (S, G) not in _RUNS:
        from real3dportrait_amd import get_driving_motion
        m = synth.synth_face_model(G, 0)
        host = F64.coefficients(40 + G, T)
        coeffs = tuple(torch.from_numpy(a).to(DEV) for a in host)
        infer = _Infer(m, S)
        out = get_driving_motion(infer.secc_renderer, infer.face3d_helper, *coeffs, rng=random.Random(9))
        plain = get_driving_motion(infer.secc_renderer, infer.face3d_helper, *coeffs, blink_mode="none")
        _RUNS[(S, G)] = {"m": m, "host": host, "coeffs": coeffs, "infer": infer, "out": out, "plain": plain,
                         "parts": composition(m, S, coeffs, 9)}
    return _RUNS[(S, G)]


@pytest.mark.parametrize("S,G", CASES)
def test_bit_identical_to_the_composition_of_the_parts(S, G):
    r = run(S, G)
    plain, drv, src, cano, kp, edits, status = r["parts"]
    out = r["out"]
    assert out["drv_secc"].shape == (T, 3, S, S) and out["src_secc"].shape == (1, 3, S, S) and out["cano_secc"].shape == (1, 3, S, S)
    assert out["drv_kp"].shape == (T, 68, 2) and all(out[k].device == torch.device(DEV) for k in ("drv_secc", "src_secc", "cano_secc", "drv_kp"))
    assert torch.equal(out["drv_secc"], drv)
    assert torch.equal(out["src_secc"], src) and torch.equal(out["cano_secc"], cano)
    assert torch.equal(out["drv_kp"], kp) and float(out["drv_kp"].abs().max()) <= 1.0
    assert out["blink_edits"] == edits and torch.equal(out["blink_status"], status)
    assert [j for j, _ in edits][:8] == list(range(8)) and max(j for j, _ in edits) == T - 2


@pytest.mark.parametrize("chunk_size", [1, 7, 50, 131])
@pytest.mark.parametrize("S,G", CASES[:1])
def test_bit_identical_for_every_chunk_size(S, G, chunk_size):
    from real3dportrait_amd import get_driving_motion
    r = run(S, G)
    out = get_driving_motion(r["infer"].secc_renderer, r["infer"].face3d_helper, *r["coeffs"], rng=random.Random(9), chunk_size=chunk_size)
    for k in ("drv_secc", "src_secc", "cano_secc", "drv_kp"):
        assert torch.equal(out[k], r["out"][k]), k


@pytest.mark.parametrize("S,G", CASES)
def test_identities(S, G):
    r = run(S, G)
    out, plain = r["out"], r["plain"]
    assert torch.equal(out["src_secc"][0], plain["drv_secc"][0])                       # the un-blinked frame 0, bit for bit
    assert not torch.equal(out["src_secc"][0], out["drv_secc"][0])                     # frame 0 of the clip is quantised (blink at 0 %)
    q = (out["drv_secc"][0] + 1) * 127.5
    assert float((q - q.round()).abs().max()) < 1e-3
    assert not torch.equal(out["cano_secc"], out["src_secc"])
    assert torch.equal(out["cano_secc"], r["parts"][3])                                # a render with exp = 0
    assert bool((out["blink_status"] == 0).all()) and len(out["blink_status"]) == len(out["blink_edits"])
    assert torch.equal(out["drv_secc"][T - 1], plain["drv_secc"][T - 1])               # the clip's last frame is never edited
    edited = sorted(j for j, _ in out["blink_edits"])
    untouched = [t for t in range(T) if t not in edited]
    assert torch.equal(out["drv_secc"][untouched], plain["drv_secc"][untouched])
    for j, p in out["blink_edits"]:
        if p > 0.5:
            assert not torch.equal(out["drv_secc"][j], plain["drv_secc"][j]), j


@pytest.mark.parametrize("S,G", CASES[:1])
def test_other_blink_modes_leave_the_maps_unquantised(S, G):
    r = run(S, G)
    plain = r["plain"]
    assert plain["blink_edits"] == [] and plain["blink_status"] is None
    assert torch.equal(plain["drv_secc"], r["parts"][0]) and torch.equal(plain["drv_kp"], r["out"]["drv_kp"])
    q = (plain["drv_secc"] + 1) * 127.5
    assert float((q - q.round()).abs().max()) > 0.4                                    # off the 8-bit grid


@pytest.mark.parametrize("S,G", CASES)
def test_maps_against_the_fp64_rasteriser_on_fp64_vertices(S, G):
    from real3dportrait_amd import face_model as FM, rasterize
    r = run(S, G)
    m, (idc, expc, _, _) = r["m"], r["host"]
    fr = list(FP64_FRAMES)
    v64 = F64.face_vertex(m["mean_shape"], m["id_base"], m["exp_base"], idc[fr], expc[fr])
    feat = np.broadcast_to(m["feat"], (len(fr),) + m["feat"].shape)
    ref = R64.rasterize(v64, m["tri"], feat, S, synth.BFM_FOV_DEG, 5.0)
    sr = r["infer"].secc_renderer
    v = FM.compute_face_vertex(sr.face_model, r["coeffs"][0][fr], r["coeffs"][1][fr], torch.zeros(len(fr), 3, device=DEV), torch.zeros(len(fr), 3, device=DEV))
    p2f = rasterize(v, sr.face_buf, S, synth.BFM_FOV_DEG, 5.0)[0].cpu().numpy()
    same = p2f == ref["pix_to_face"]
    differing = int((~same).reshape(len(fr), -1).sum(axis=1).max())
    # frames after the first of the call are not first in THEIR chunk of the clip: compare the images where face 0, which covers nothing, plays no part
    img = r["plain"]["drv_secc"][fr].cpu().numpy().astype(np.float64)
    d = np.abs(img - (2.0 * ref["image"] - 1.0))
    e = float(d[np.broadcast_to(same[:, None], d.shape)].max())
    print("S %d G %d: %d differing pixels of %d (cap %d), max |image - fp64| %.2e where the faces agree" % (S, G, differing, S * S, S * S // 1000, e))
    assert differing <= (S * S) // 1000 and e <= 2e-4
    assert (ref["pix_to_face"] >= 0).mean() > 0.9


def test_a_face_0_with_area_is_background_where_a_call_starts():
    """synth_face_model's face 0 has no area, so the tests above never see the reference's mask, pix_to_face > 0.  Here a visible triangle
    of the lower face is moved to index 0.  Expected, from the rule alone: in the first frame of every chunk and in src_secc the pixels of
    face 0 are background (-1 after the affine), every other pixel of every frame is the render that keeps face 0, bit for bit; and
    cano_secc, the second mesh of its call, keeps face 0."""
    from real3dportrait_amd import face_model as FM, get_driving_motion, rasterize
    S, G, frames = 64, 24, 15
    m = dict(synth.synth_face_model(G, 0))
    coeffs = tuple(torch.from_numpy(a).to(DEV) for a in F64.coefficients(77, frames))
    idc, expc = coeffs[:2]
    arrays = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (m["mean_shape"].reshape(-1), m["id_base"], m["exp_base"]))
    feat = torch.from_numpy(m["feat"])[None].to(DEV)

    def keep_all(tri, i, e):
        """(pix_to_face per mesh, image) of a render in which no face is background."""
        p2f, _, _, image = rasterize(FM.face_vertex(arrays, i, e), tri, S, synth.BFM_FOV_DEG, 5.0, feat=feat.expand(len(i), -1, -1),
                                     first_face_is_background=False, out_scale=2.0, out_shift=-1.0)
        own = torch.where(p2f >= 0, p2f - torch.arange(len(i), device=DEV)[:, None, None] * len(tri), p2f)
        return own, image

    tri = torch.from_numpy(m["tri"]).to(DEV)
    f = int(keep_all(tri, idc[:1], expc[:1])[0][0, 3 * S // 4, S // 2])          # a face of the lower half, away from the eyes
    assert f > 0
    m["tri"] = np.concatenate([m["tri"][f:f + 1], m["tri"][1:f], m["tri"][f + 1:]])
    tri = torch.from_numpy(m["tri"]).to(DEV)
    own, kept = keep_all(tri, idc, expc)
    first = own == 0                                                             # [frames, S, S]: the pixels of face 0
    assert int(first.reshape(frames, -1).sum(dim=1).min()) >= 1
    infer = _Infer(m, S)
    for chunk_size in (7, 15):
        out = get_driving_motion(infer.secc_renderer, infer.face3d_helper, *coeffs, blink_mode="none", chunk_size=chunk_size)
        for t in range(frames):
            got, hole = out["drv_secc"][t], first[t][None].expand(3, -1, -1)
            if t % chunk_size == 0:
                assert bool((got[hole] == -1.0).all()) and torch.equal(got[~hole], kept[t][~hole]), (chunk_size, t)
            else:
                assert torch.equal(got, kept[t]), (chunk_size, t)
        assert torch.equal(out["src_secc"][0], out["drv_secc"][0])
        cano_own, cano_kept = keep_all(tri, idc[:1], torch.zeros_like(expc[:1]))
        assert int((cano_own == 0).sum()) >= 1 and torch.equal(out["cano_secc"], cano_kept)


def test_patch_driving_motion():
    from real3dportrait_amd import MeshRenderer, patch_driving_motion
    S, G = CASES[0]
    r = run(S, G)
    infer = _Infer(r["m"], S)
    assert patch_driving_motion(infer) is infer and infer._r3d_reference_get_driving_motion(*[None] * 6) == "reference"
    assert isinstance(infer.secc_renderer.face_renderer, MeshRenderer) and infer.secc_renderer.face_renderer.rasterize_size == S
    batch = {"keep": 1}
    random.seed(9)
    assert infer.get_driving_motion(*r["coeffs"], batch, {"blink_mode": "period"}) is batch and batch["keep"] == 1
    for k in ("drv_secc", "src_secc", "cano_secc", "drv_kp"):
        assert batch[k].is_cuda and torch.equal(batch[k], r["out"][k]), k
    assert batch["drv_secc"].shape == (T, 3, S, S) and batch["src_secc"].shape == (1, 3, S, S) and batch["cano_secc"].shape == (1, 3, S, S)
    assert batch["drv_kp"].shape == (T, 68, 2) and float(batch["drv_kp"].min()) >= -1.0 and float(batch["drv_kp"].max()) <= 1.0
    assert patch_driving_motion(infer) is infer and infer._r3d_reference_get_driving_motion(*[None] * 6) == "reference"
