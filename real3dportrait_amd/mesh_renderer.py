"""HIP mesh rasteriser for the SECC map: MeshRenderer of deep_3drecon/util/mesh_renderer.py:35-130 without pytorch3d (r3d_raster_forward
of include/r3d_hip.h).

    MeshRenderer            the reference's class: __init__(rasterize_fov, znear, zfar, rasterize_size, **args),
                            forward(vertex, tri, feat=None) -> (mask, depth, image)
    rasterize               the functional form, which also returns pix_to_face
    patch_secc_renderer     swaps SECC_Renderer.face_renderer (deep_3drecon/secc_renderer.py:19) for the class above

The reference rasterises with pytorch3d (image_size = S, blur_radius = 0, faces_per_pixel = 1, cull_backfaces = False,
FoVPerspectiveCameras(fov, znear, zfar)).  The rule those settings give is restated from pytorch3d's naive rasteriser (the header and
tests/raster_ref64.py); equality with pytorch3d rests on that restatement and has not been measured against pytorch3d.  One documented
difference: a face with a vertex at z < znear / 2 is dropped, not clipped (SECC_Renderer's faces sit at z = 10 +- 1.5 with znear = 5).
zfar takes no part: nothing is culled at the far plane, as in the reference.

INFERENCE ONLY: inputs are detached and no autograd graph is built.  There is no fallback: without the library, importing this raises.
"""
import weakref

import torch
import torch.nn as nn

from . import _lib
from ._state import StreamBuffers

_TRI = {}              # id(tri) -> (weak reference to tri, its version, N checked against, the int32 copy the kernels read or None)


def _checked_tri(tri, N):
    """tri as the contiguous int32 tensor the kernels read, its indices checked against [0, N) once per distinct tensor (and version of
    it): one device-to-host sync at first use, none afterwards.  The cache holds tri weakly and dies with it."""
    key = id(tri)
    hit = _TRI.get(key)
    if hit is not None and hit[0]() is tri and hit[1] == tri._version and hit[2] == N:
        return tri if hit[3] is None else hit[3]
    t = tri.detach()
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError("rasterize: tri must be an integer tensor, got %s" % (tri.dtype,))
    lo, hi = torch.stack([t.min(), t.max()]).tolist()          # the one sync; before the narrowing, so that no index wraps into range
    if lo < 0 or hi >= N:
        raise ValueError("rasterize: tri holds vertex indices %d .. %d, the mesh has %d vertices" % (lo, hi, N))
    narrow = t.dtype != torch.int32 or not t.is_contiguous()
    t32 = t.to(torch.int32).contiguous() if narrow else t
    # never a strong reference to tri's own storage: the entry must die with tri
    _TRI[key] = (weakref.ref(tri, lambda _, k=key: _TRI.pop(k, None)), tri._version, N, t32 if narrow else None)
    return t32


def _new_workspace(dev, B, S, M):
    nbytes = _lib.call("r3d_raster_workspace_bytes", B, S, M)
    if nbytes == 0:
        raise ValueError("rasterize: B = %d meshes of M = %d faces at S = %d are outside what r3d_raster_forward accepts" % (B, M, S))
    return torch.empty(nbytes, device=dev, dtype=torch.uint8)


_WORKSPACE = StreamBuffers(_new_workspace, cap=8)          # a clip uses one or two shapes


@torch.no_grad()
def rasterize(vertex, tri, S, fov, znear, feat=None, negate_x=True, first_face_is_background=True, out_scale=1.0, out_shift=0.0,
              want_pix_to_face=True, _large_box=None):
    """Rasterise B meshes: vertex [B, N, 3] camera space, tri [M, 3] or [B, M, 3] integer, feat [B, N, C] (1 <= C <= 4) or None, S the
    image size, fov in degrees.  Returns (pix_to_face, mask, depth, image):

        pix_to_face [B, S, S] int64   the packed face index b M + f, or -1 (None with want_pix_to_face=False)
        mask  [B, 1, S, S]            pix_to_face > 0.  The strict > 0 is the reference's (mesh_renderer.py:116): it turns face 0 of the
                                      batch's FIRST mesh into background.  first_face_is_background=False gives pix_to_face >= 0.
        depth [B, 1, S, S]            mask x camera-space depth
        image [B, C, S, S]            (mask x the perspective-corrected interpolation of feat) x out_scale + out_shift, or None

    The perspective-corrected barycentrics are used, not stored (pytorch3d's Fragments.bary_coords has no counterpart here).  negate_x:
    x is negated as the reference does (mesh_renderer.py:69-71), on the fly: the caller's tensor is never written.  tri is checked on the
    host once per distinct tensor (ValueError for an index outside [0, N)).  _large_box is a test hook: the pixel count of a face's
    clamped box above which it takes the wave-per-face kernel (None: the library's 64)."""
    if not torch.is_tensor(vertex) or vertex.dim() != 3 or vertex.shape[-1] != 3:
        raise ValueError("rasterize: vertex must be [B, N, 3]")
    if not torch.is_tensor(tri) or tri.dim() not in (2, 3) or tri.shape[-1] != 3:
        raise ValueError("rasterize: tri must be [M, 3] or [B, M, 3]")
    v = vertex.detach().float().contiguous()
    B, N = v.shape[:2]
    if tri.dim() == 3 and tri.shape[0] != B:
        raise ValueError("rasterize: tri %s and vertex %s differ in B" % (tuple(tri.shape), tuple(v.shape)))
    if tri.device != v.device:
        raise ValueError("rasterize: tri is on %s, vertex on %s" % (tri.device, v.device))
    M, S = tri.shape[-2], int(S)
    if B < 1 or N < 1 or M < 1:
        raise ValueError("rasterize: empty input (vertex %s, tri %s)" % (tuple(v.shape), tuple(tri.shape)))
    C = 0
    if feat is not None:
        if not torch.is_tensor(feat) or feat.dim() != 3 or feat.shape[:2] != v.shape[:2]:
            raise ValueError("rasterize: feat must be [B, N, C] with vertex's B and N")
        feat = feat.detach().float().contiguous()
        C = feat.shape[2]
    t32 = _checked_tri(tri, N)
    ws = _WORKSPACE.get(v.device, B, S, M)
    e = lambda c: torch.empty(B, c, S, S, device=v.device, dtype=torch.float32)
    p2f = torch.empty(B, S, S, device=v.device, dtype=torch.int64) if want_pix_to_face else None
    mask, depth, image = e(1), e(1), (e(C) if feat is not None else None)
    args = (v, feat, t32, int(tri.dim() == 3), B, N, M, C, S, float(fov), float(znear), int(bool(negate_x)), int(bool(first_face_is_background)),
            float(out_scale), float(out_shift), p2f, mask, depth, image, ws, ws.numel())
    if _large_box is None:
        _lib.call("r3d_raster_forward", *args)
    else:
        _lib.call("r3d_debug_raster_forward", *args, int(_large_box), 15)
    return p2f, mask, depth, image


@torch.no_grad()
def _rasterize_into(vertex, tri, S, fov, znear, feat, image, mask, depth, out_scale=1.0, out_shift=0.0):
    """rasterize's call with every output given (driving_motion.py): vertex [B, N, 3], feat [B, N, C] and the outputs image [B, C, S, S],
    mask and depth [B, 1, S, S] are contiguous fp32 tensors on one GPU, tri [M, 3] or [B, M, 3] integer; the reference's settings
    (x negated, face 0 of the first mesh is background), no pix_to_face.  The same launches as rasterize, so the same bits."""
    B, N = vertex.shape[:2]
    M, S = tri.shape[-2], int(S)
    C = feat.shape[2]
    for t, shape, what in ((vertex, (B, N, 3), "vertex"), (feat, (B, N, C), "feat"), (image, (B, C, S, S), "image"),
                           (mask, (B, 1, S, S), "mask"), (depth, (B, 1, S, S), "depth")):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != vertex.device:
            raise ValueError("_rasterize_into: %s must be a contiguous float32 %s tensor on %s" % (what, shape, vertex.device))
    t32 = _checked_tri(tri, N)
    ws = _WORKSPACE.get(vertex.device, B, S, M)
    _lib.call("r3d_raster_forward", vertex, feat, t32, int(tri.dim() == 3), B, N, M, C, S, float(fov), float(znear), 1, 1, float(out_scale),
              float(out_shift), None, mask, depth, image, ws, ws.numel())


class MeshRenderer(nn.Module):
    """deep_3drecon/util/mesh_renderer.py:35-130 on the HIP rasteriser: the same constructor, forward(vertex, tri, feat=None) ->
    (mask [B, 1, S, S], depth [B, 1, S, S], image [B, C, S, S] or None), fp32, x negated as the reference negates it (on its copy, never
    on the caller's tensor).  mask is the reference's pix_to_face > 0 (face 0 of the first mesh is background); out_scale / out_shift
    (1, 0) apply image x out_scale + out_shift after the mask multiply, inside the resolve kernel.  Inference only."""

    def __init__(self, rasterize_fov, znear=0.1, zfar=10, rasterize_size=224, **args):
        super().__init__()
        self.rasterize_size = rasterize_size
        self.fov = rasterize_fov
        self.znear = znear
        self.zfar = zfar
        self.out_scale, self.out_shift = 1.0, 0.0

    def forward(self, vertex, tri, feat=None):
        _, mask, depth, image = rasterize(vertex, tri, int(self.rasterize_size), self.fov, self.znear, feat=feat, out_scale=self.out_scale,
                                          out_shift=self.out_shift, want_pix_to_face=False)
        return mask, depth, image


def _secc_forward_folded(self, id, exp, euler, trans):
    """SECC_Renderer.forward (deep_3drecon/secc_renderer.py:34-58) with its line 52, (secc_face - 0.5) / 0.5, done by the rasteriser's
    output affine (2 x - 1): bound by patch_secc_renderer(fold_affine=True)."""
    bs = id.shape[0]
    is_btc_flag = id.ndim == 3
    if is_btc_flag:
        t = id.shape[1]
        bs = bs * t
        id, exp, euler, trans = id.reshape([bs, -1]), exp.reshape([bs, -1]), euler.reshape([bs, -1]), trans.reshape([bs, -1])
    face_vertex = self.face_model.compute_face_vertex(id, exp, euler, trans)
    face_mask, _, secc_face = self.face_renderer(face_vertex, self.face_buf, feat=self.face_feat.expand(bs, -1, -1))
    if is_btc_flag:
        unfold = lambda x: x.reshape(bs // t, t, *x.shape[1:]).permute(0, 2, 1, 3, 4)          # "(n t) c h w -> n c t h w"
        face_mask, secc_face = unfold(face_mask), unfold(secc_face)
    return face_mask, secc_face


def patch_secc_renderer(secc_renderer, fold_affine=False):
    """Swap secc_renderer.face_renderer (SECC_Renderer of deep_3drecon/secc_renderer.py:10-58) for the HIP MeshRenderer built from its
    fov, znear, zfar and the old renderer's rasterize_size (in place; returns secc_renderer).  By default the object's own forward is
    left alone, so the map keeps the reference's order of operations (interpolate, mask, then (x - 0.5) / 0.5 in torch).
    fold_affine=True also binds a forward that leaves that line to the resolve kernel (image x 2 - 1 after the mask multiply: the
    same value to 1 ulp), passes face_buf [M, 3] once instead of a repeat per call, and keeps the old one as _r3d_reference_forward."""
    old = secc_renderer.face_renderer
    new = MeshRenderer(rasterize_fov=float(secc_renderer.fov), znear=float(secc_renderer.znear), zfar=float(secc_renderer.zfar),
                       rasterize_size=int(old.rasterize_size))
    if fold_affine:
        new.out_scale, new.out_shift = 2.0, -1.0
        secc_renderer._r3d_reference_forward = secc_renderer.forward
        secc_renderer.forward = _secc_forward_folded.__get__(secc_renderer)
    secc_renderer.face_renderer = new
    return secc_renderer
