"""Time the HIP face model and get_driving_motion on a 250-frame clip at 512 x 512 over synth_face_model(188, 0)
(N = 35 721 vertices, the BFM's size; Ki + Ke = 144) and print one JSON line:

  * r3d_face_vertex alone on one chunk of 50 frames at zero pose, device events around every call, `calls` calls per block, `blocks`
    blocks after a warm-up; reported: the median of the block medians and their spread.  Beside it, in alternating blocks of the same
    run, the torch operations of compute_face_vertex (bfm.py:332-347: two einsums, two adds, the rotation from six sines and cosines,
    a batched product, the depth flip) on the same tensors, and the time that reading the bases and writing the vertices once takes at
    the 8 TB/s HBM figure of DESIGN 5;
  * get_driving_motion whole against the route the package offered before it: the torch face model, patch_secc_renderer(fold_affine=True),
    the reference's chunk loop with its copy of every chunk to the host, its concatenation there and its copy back, apply_periodic_blink
    and the torch landmarks.  Host wall clock around a call that ends in a synchronise, the two routes in alternating blocks.

    python scripts/prof_driving_motion.py [--calls 20] [--blocks 5] [--clip-calls 3] [--frames 250] [--size 512] [--grid 188] [--out DIR]
"""
import random
import statistics

import _prof

_prof.paths()
HBM_TBPS = 8.0


def main():
    ap = _prof.parser(__doc__, calls=20)
    ap.add_argument("--clip-calls", type=int, default=3)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--grid", type=int, default=188)
    a = ap.parse_args()
    import numpy as np
    import torch

    from real3dportrait_amd import apply_periodic_blink, face_model as FM, get_driving_motion, patch_secc_renderer, synth

    assert torch.cuda.is_available(), "timings need the GPU"
    dev, S, T, CH = "cuda:0", a.size, a.frames, 50
    m = synth.synth_face_model(a.grid, 0)
    N, Ki, Ke = m["feat"].shape[0], m["id_base"].shape[1], m["exp_base"].shape[1]
    D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    idc, expc = D(synth.hash_unitvar(1, (T, Ki), stream=80)), D(synth.hash_unitvar(1, (T, Ke), stream=81))
    euler, trans = D(0.3 * synth.hash_unitvar(1, (T, 3), stream=82)), D(0.2 * synth.hash_unitvar(1, (T, 3), stream=83))

    def rotation(e):
        x, y, z = e[:, :1], e[:, 1:2], e[:, 2:]
        one, zero = torch.ones_like(x), torch.zeros_like(x)
        rx = torch.cat([one, zero, zero, zero, torch.cos(x), -torch.sin(x), zero, torch.sin(x), torch.cos(x)], dim=1).reshape(-1, 3, 3)
        ry = torch.cat([torch.cos(y), zero, torch.sin(y), zero, one, zero, -torch.sin(y), zero, torch.cos(y)], dim=1).reshape(-1, 3, 3)
        rz = torch.cat([torch.cos(z), -torch.sin(z), zero, torch.sin(z), torch.cos(z), zero, zero, zero, one], dim=1).reshape(-1, 3, 3)
        return (rz @ ry @ rx).permute(0, 2, 1)

    class TorchFaceModel:
        """The torch operations of ParametricFaceModel.compute_face_vertex on device tensors."""
        mean_shape, id_base, exp_base, camera_distance = D(m["mean_shape"]), D(m["id_base"]), D(m["exp_base"]), 10.0

        def compute_face_vertex(self, id, exp, angle, trans):
            shape = torch.einsum("ij,aj->ai", self.id_base, id) + torch.einsum("ij,aj->ai", self.exp_base, exp) + self.mean_shape.reshape(1, -1)
            v = shape.reshape(id.shape[0], -1, 3) @ rotation(angle) + trans.unsqueeze(1)
            v[..., -1] = self.camera_distance - v[..., -1]
            return v

    class Rasterizer:
        rasterize_size = S

    class Secc:
        face_model = TorchFaceModel()
        fov, znear, zfar = synth.BFM_FOV_DEG, 5.0, 15.0
        face_renderer = Rasterizer()
        face_feat, face_buf = D(m["feat"])[None], D(m["tri"])

        def forward(self, id, exp, euler, trans):
            raise AssertionError

    class Helper:
        key_mean_shape, key_id_base, key_exp_base = D(m["key_mean_shape"]), D(m["key_id_base"]), D(m["key_exp_base"])

    secc, helper = Secc(), Helper()
    arrays = FM.model_arrays(secc.face_model, torch.device(dev))
    vertex = torch.empty(CH, N, 3, device=dev)
    zeros = torch.zeros(T, 3, device=dev)

    def wall(fn, calls):
        """The median of `calls` calls, each alone between two synchronises on the host clock."""
        return statistics.median(_prof.by_host_clock(fn, 1) for _ in range(calls))

    def measure(fns, timer, calls):
        samples = _prof.alternate(_prof.routes(fns, timer, calls), a.blocks, warmup=2)
        return {t: _prof.ms_spread(v, keep_blocks=True) for t, v in samples.items()}

    hip_chunk = lambda: FM.face_vertex(arrays, idc[:CH], expc[:CH], None, None, out=vertex)
    torch_chunk = lambda: secc.face_model.compute_face_vertex(idc[:CH], expc[:CH], zeros[:CH], zeros[:CH])
    kernel = measure({"r3d_face_vertex": hip_chunk, "torch_ops": torch_chunk}, _prof.block_median, a.calls)
    err = float((hip_chunk() - torch_chunk()).abs().max())
    base_bytes, out_bytes = 3 * N * (Ki + Ke) * 4, CH * N * 3 * 4
    kernel["bytes"] = {"bases_read_once": base_bytes, "vertices_written": out_bytes,
                       "ms_at_%g_TBps" % HBM_TBPS: round((base_bytes + out_bytes) / (HBM_TBPS * 1e12) * 1e3, 4)}
    kernel["max_abs_difference_hip_vs_torch"] = err

    # the package's route before get_driving_motion existed: the reference's loop (real3d_infer.py:391-433) over the patched renderer
    patched = patch_secc_renderer(Secc(), fold_affine=True)

    def lm2d_torch(idc, expc, euler, trans):
        face = (idc @ helper.key_id_base.T + expc @ helper.key_exp_base.T + helper.key_mean_shape.reshape(1, -1)).reshape(idc.shape[0], -1, 3)
        lm3d = face @ rotation(euler) + trans.unsqueeze(1)
        lm3d[..., -1] = 10 - lm3d[..., -1]
        proj = torch.tensor([[1015.0, 0, 0], [0, 1015.0, 0], [112.0, 112.0, 1]], device=dev)
        p = lm3d @ proj
        lm2d = p[..., :2] / p[..., 2:]
        lm2d[..., 1] = 224 - lm2d[..., 1]
        return lm2d / 224

    def parent_route():
        parts = []
        for i in range(0, T, CH):
            _, c = patched.forward(idc[i:i + CH], expc[i:i + CH], zeros[i:i + CH], zeros[i:i + CH])
            parts.append(c.cpu())
        drv = torch.cat(parts, dim=0).cuda()
        _, src = patched.forward(idc[0:1], expc[0:1], zeros[0:1], zeros[0:1])
        _, cano = patched.forward(idc[0:1], expc[0:1] * 0, zeros[0:1], zeros[0:1])
        apply_periodic_blink(drv, random.Random(5))
        kp = torch.clamp((lm2d_torch(idc, expc, euler, trans) - 0.5) / 0.5, -1, 1)
        return drv, src.cuda(), cano.cuda(), kp

    new_route = lambda: get_driving_motion(secc, helper, idc, expc, euler, trans, rng=random.Random(5))
    whole = measure({"get_driving_motion": new_route, "parent_route": parent_route}, wall, a.clip_calls)
    got, old = new_route(), parent_route()
    # the two face models agree to a few ulp, not bit for bit, so the interpolated colours differ in their last bits almost everywhere:
    # counted are the pixels that differ by more than half an 8-bit step (a face or a blink source chosen differently)
    diff = (got["drv_secc"] - old[0]).abs().amax(dim=1)
    whole["drv_secc_pixels"] = int(diff.numel())
    whole["drv_secc_pixels_differing_in_any_bit"] = int((diff > 0).sum())
    whole["drv_secc_pixels_differing_by_more_than_half_an_8_bit_step"] = int((diff > 1.0 / 255.0).sum())
    whole["drv_secc_max_abs_difference"] = float(diff.max())
    whole["drv_kp_max_abs_difference"] = float((got["drv_kp"] - old[3]).abs().max())
    whole["blink_status"] = got["blink_status"].cpu().tolist()
    faster_by = whole["parent_route"]["ms"] - whole["get_driving_motion"]["ms"]
    whole["faster_by_ms"] = round(faster_by, 3)
    whole["faster_by_more_than_both_spreads"] = bool(faster_by > max(whole["parent_route"]["spread_ms"], whole["get_driving_motion"]["spread_ms"]))

    out = {"metric": "driving_motion_%d_frames_s%d" % (T, S), "S": S, "frames": T, "chunk": CH, "N": N, "Ki": Ki, "Ke": Ke, "faces": int(m["tri"].shape[0]),
           "calls_per_block": a.calls, "clip_calls_per_block": a.clip_calls, "blocks": a.blocks, "shader_clock": "not measured",
           "face_vertex_chunk_of_50_device_events": kernel, "whole_function_wall_with_sync": whole}
    _prof.emit(out, a.out, "prof_driving_motion")


if __name__ == "__main__":
    main()
