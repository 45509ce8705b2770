"""get_driving_motion of inference/real3d_infer.py:391-433 on the device: face model -> rasteriser -> blink edit -> landmarks, chained
without a device-to-host copy of a map.

    get_driving_motion      (secc_renderer, face3d_helper, id, exp, euler, trans, ...) -> dict of drv_secc, src_secc, cano_secc, drv_kp, ...
    patch_driving_motion    binds it as infer.get_driving_motion(id, exp, euler, trans, batch, inp), the reference's signature

The reference renders the clip in chunks of 50 maps, copies every chunk to the host, concatenates there and copies the clip back; then it
edits the blink frames one by one through the host.  Here each chunk's vertices come from r3d_face_vertex (zero pose: NULL euler and
trans), r3d_raster_forward writes the chunk's maps straight into its slice of the clip's drv_secc with SECC_Renderer's (x - 0.5) / 0.5
folded in (the arithmetic of patch_secc_renderer(fold_affine=True)), and apply_periodic_blink edits the clip in place.  The only
synchronisation is the rasteriser's index check of face_buf, once per distinct face_buf tensor.

A map does not depend on chunk_size, with one exception inherited from the reference: its mask, pix_to_face > 0, turns face 0 of the
FIRST mesh of every rasteriser call into background, so the pixels of face 0 are background in the first frame of each chunk and in
src_secc.  cano_secc is the second mesh of its call and keeps face 0, where the reference, which renders it alone, drops it.

INFERENCE ONLY.  There is no fallback: without the library, importing this raises.
"""
import random

import torch

from . import edit_secc, face_model, mesh_renderer


@torch.no_grad()
def get_driving_motion(secc_renderer, face3d_helper, id, exp, euler, trans, blink_mode="period", rng=random, chunk_size=50,
                       period_frames=125):
    """id [T, Ki], exp [T, Ke], euler [T, 3], trans [T, 3] on the GPU; secc_renderer an object with SECC_Renderer's attributes
    (face_model, face_buf [M, 3] and face_feat [1, N, 3] on that GPU, fov, znear, face_renderer.rasterize_size), face3d_helper one with
    Face3DHelper's key_* arrays.  Returns a dict, everything on the device:

        drv_secc [T, 3, S, S]     the driving maps in [-1, 1] at zero pose, blink frames edited when blink_mode == 'period'
        src_secc, cano_secc [1, 3, S, S]   frame 0 before the blink, and frame 0 with exp = 0
        drv_kp [T, L, 2]          clamp((reconstruct_lm2d(id, exp, euler, trans) - 0.5) / 0.5, -1, 1)
        blink_edits, blink_status the (frame, percent) list and apply_periodic_blink's device status tensor (None: nothing edited)

    rng is consumed exactly as the reference's loop consumes `random`."""
    if not torch.is_tensor(id) or id.dim() != 2 or not id.is_cuda:
        raise ValueError("get_driving_motion: id must be a [T, Ki] tensor on the GPU")
    chunk_size = int(chunk_size)
    if chunk_size < 1:
        raise ValueError("get_driving_motion: chunk_size = %d" % chunk_size)
    dev, T = id.device, id.shape[0]
    fm = secc_renderer.face_model
    arrays = face_model.model_arrays(fm, dev)
    N = arrays[0].numel() // 3
    S = int(secc_renderer.face_renderer.rasterize_size)
    fov, znear, distance = float(secc_renderer.fov), float(secc_renderer.znear), float(fm.camera_distance)
    tri, feat1 = secc_renderer.face_buf, secc_renderer.face_feat
    if tri.device != dev or feat1.device != dev:
        raise ValueError("get_driving_motion: face_buf is on %s and face_feat on %s, the coefficients on %s" % (tri.device, feat1.device, dev))
    idc, expc = (x.detach().to(device=dev, dtype=torch.float32).contiguous() for x in (id, exp))
    with torch.cuda.device(dev):
        Bmax = max(min(chunk_size, T), 2)
        feat = feat1.detach().float().reshape(1, N, -1).expand(Bmax, -1, -1).contiguous()
        C = feat.shape[2]
        vertex = torch.empty(Bmax, N, 3, device=dev, dtype=torch.float32)
        mask, depth = (torch.empty(Bmax, 1, S, S, device=dev, dtype=torch.float32) for _ in range(2))
        drv_secc = torch.empty(T, C, S, S, device=dev, dtype=torch.float32)
        for i in range(0, T, chunk_size):
            B = min(chunk_size, T - i)
            face_model.face_vertex(arrays, idc[i:i + B], expc[i:i + B], None, None, camera_distance=distance, out=vertex[:B])
            mesh_renderer._rasterize_into(vertex[:B], tri, S, fov, znear, feat[:B], drv_secc[i:i + B], mask[:B], depth[:B], 2.0, -1.0)
        pair = torch.empty(2, C, S, S, device=dev, dtype=torch.float32)
        face_model.face_vertex(arrays, idc[0:1], expc[0:1], None, None, camera_distance=distance, out=vertex[0:1])
        face_model.face_vertex(arrays, idc[0:1], None, None, None, camera_distance=distance, out=vertex[1:2])
        mesh_renderer._rasterize_into(vertex[:2], tri, S, fov, znear, feat[:2], pair, mask[:2], depth[:2], 2.0, -1.0)
        edits, status = [], None
        if blink_mode == "period":
            edits, status = edit_secc.apply_periodic_blink(drv_secc, rng, period_frames)
        lm2d = face_model.reconstruct_lm2d(face3d_helper, idc, expc, euler, trans)
        drv_kp = torch.clamp((lm2d - 0.5) / 0.5, -1, 1)
    return {"drv_secc": drv_secc, "src_secc": pair[0:1], "cano_secc": pair[1:2], "drv_kp": drv_kp, "blink_edits": edits,
            "blink_status": status}


def _infer_get_driving_motion(self, id, exp, euler, trans, batch, inp):
    """real3d_infer.py:391-433 with its signature: fills batch['drv_secc' | 'src_secc' | 'cano_secc' | 'drv_kp'] and returns batch."""
    out = get_driving_motion(self.secc_renderer, self.face3d_helper, id, exp, euler, trans, blink_mode=inp["blink_mode"])
    for k in ("drv_secc", "src_secc", "cano_secc", "drv_kp"):
        batch[k] = out[k]
    return batch


def patch_driving_motion(infer):
    """Patch infer.secc_renderer (patch_secc_renderer with fold_affine=True, unless it already carries the HIP renderer) and bind
    infer.get_driving_motion(id, exp, euler, trans, batch, inp) to the function above, which reads inp['blink_mode'] and uses
    infer.secc_renderer and infer.face3d_helper; the old method stays as infer._r3d_reference_get_driving_motion.  Returns infer."""
    if not isinstance(infer.secc_renderer.face_renderer, mesh_renderer.MeshRenderer):
        mesh_renderer.patch_secc_renderer(infer.secc_renderer, fold_affine=True)
    if not hasattr(infer, "_r3d_reference_get_driving_motion"):
        object.__setattr__(infer, "_r3d_reference_get_driving_motion", getattr(infer, "get_driving_motion", None))
    object.__setattr__(infer, "get_driving_motion", _infer_get_driving_motion.__get__(infer))
    return infer
