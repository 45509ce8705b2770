"""Time the HIP mesh rasteriser on a chunk of 50 frames at S = 512, the shape SECC_Renderer is called with
(inference/real3d_infer.py:396-405), on synth_face_mesh(G = 188) (141 376 faces, twice BFM's layer count) and G = 132 (69 696 faces),
and print one JSON line:

  * MeshRenderer.forward on the chunk (one library call: a memset and three kernels), device events around every call, `calls` calls per
    block, `blocks` blocks after a warm-up; reported: the median of the block medians and their spread, in ms per chunk and per frame;
  * the memset and each of the three kernels, the same way, through the stage mask of the test hook r3d_debug_raster_forward: the call
    cut off after the clear, after scatter, after large_faces and complete, each kernel's time being the difference of two such
    medians (every timed call starts from its own clear, so each kernel sees the input the whole call gives it);
  * the same math in plain torch on the same GPU as a sanity baseline (one frame at a time: every face's pixel box of at most
    WINDOW x WINDOW pixels evaluated densely, a scatter_reduce 'amin' of the same 64-bit keys, a gather for the attributes), with the
    number of pixels on which its pix_to_face differs from the library's;
  * the bytes a frame must move (keys written and read, outputs, vertices and indices) and what they would take at a nominal 4 TB/s.

    python scripts/prof_raster.py [--calls 20] [--blocks 5] [--frames 50] [--out DIR]     (writes DIR/prof_raster.json)
"""
import json
import math
import sys

import _prof

_prof.paths()

WINDOW = 16
STAGES = (("clear", 1), ("scatter", 3), ("large_faces", 7), ("resolve", 15))          # cumulative stage masks: every timed call starts from its own clear


def torch_rasterize(v, tri, feat, S, fov_deg, znear, window=WINDOW):
    """One frame of the rule in plain torch (fp32, on v's device): (pix_to_face [S, S], mask, depth [S, S], image [C, S, S], the number
    of faces whose pixel box exceeds the window and is therefore cut).  v [N, 3] with x already negated."""
    import torch
    s = 1.0 / math.tan(math.radians(fov_deg) * 0.5)
    P = v[tri]                                                # [M, 3, 3]
    z = P[:, :, 2]
    xn, yn = (s * P[:, :, 0]) / z, (s * P[:, :, 1]) / z
    edge = lambda px, py, ax, ay, bx, by: (px - ax) * (by - ay) - (py - ay) * (bx - ax)
    area = edge(xn[:, 2], yn[:, 2], xn[:, 0], yn[:, 0], xn[:, 1], yn[:, 1])
    ok = (z >= 0.5 * znear).all(dim=1) & torch.isfinite(P).all(dim=2).all(dim=1) & (area.abs() > 1e-8)
    A = area + 1e-8
    pos = lambda c: S - 0.5 - (c + 1.0) * (0.5 * S)
    j0 = torch.ceil(pos(xn.max(dim=1).values) - 0.01).clamp(0, S).long()
    j1 = torch.floor(pos(xn.min(dim=1).values) + 0.01).clamp(-1, S - 1).long()
    i0 = torch.ceil(pos(yn.max(dim=1).values) - 0.01).clamp(0, S).long()
    i1 = torch.floor(pos(yn.min(dim=1).values) + 0.01).clamp(-1, S - 1).long()
    cut = int((ok & ((j1 - j0 >= window) | (i1 - i0 >= window))).sum())
    o = torch.arange(window, device=v.device)
    oi, oj = (t.reshape(1, -1) for t in torch.meshgrid(o, o, indexing="ij"))
    pi, pj = i0[:, None] + oi, j0[:, None] + oj               # [M, window^2]
    inside = ok[:, None] & (pi <= i1[:, None]) & (pj <= j1[:, None])
    centre = -1.0 + (2 * (S - 1 - torch.arange(S, device=v.device)) + 1).float() / float(S)
    px, py = centre[pj.clamp(max=S - 1)], centre[pi.clamp(max=S - 1)]
    c = lambda t, k: t[:, k:k + 1]

    def bary(px, py, xn, yn, z, A):
        w0 = edge(px, py, c(xn, 1), c(yn, 1), c(xn, 2), c(yn, 2)) / A
        w1 = edge(px, py, c(xn, 2), c(yn, 2), c(xn, 0), c(yn, 0)) / A
        w2 = edge(px, py, c(xn, 0), c(yn, 0), c(xn, 1), c(yn, 1)) / A
        t0, t1, t2 = w0 * c(z, 1) * c(z, 2), c(z, 0) * w1 * c(z, 2), c(z, 0) * c(z, 1) * w2
        den = (t0 + t1 + t2).clamp(min=1e-8)
        b0, b1, b2 = t0 / den, t1 / den, t2 / den
        return (w0 > 0) & (w1 > 0) & (w2 > 0), b0, b1, b2, b0 * c(z, 0) + b1 * c(z, 1) + b2 * c(z, 2)

    cov, _, _, _, pz = bary(px, py, xn, yn, z, A[:, None])
    cov &= inside & (pz >= 0)
    f = torch.arange(tri.shape[0], device=v.device)[:, None].expand_as(cov)
    key = (pz[cov].contiguous().view(torch.int32).long() << 32) | f[cov]
    empty = torch.iinfo(torch.int64).max
    keys = torch.full((S * S,), empty, dtype=torch.int64, device=v.device)
    keys.scatter_reduce_(0, (pi * S + pj)[cov], key, "amin", include_self=True)
    hit = keys != empty
    face = torch.where(hit, keys & 0xFFFFFFFF, torch.zeros_like(keys))
    depth = torch.where(hit, (keys >> 32).int().view(torch.float32), torch.zeros(S * S, device=v.device))
    p2f = torch.where(hit, face, torch.full_like(face, -1))
    mask = (p2f > 0).float()
    rows, cols = torch.arange(S * S, device=v.device) // S, torch.arange(S * S, device=v.device) % S
    _, b0, b1, b2, _ = bary(centre[cols][:, None], centre[rows][:, None], xn[face], yn[face], z[face], A[face][:, None])
    a = feat[tri[face]]                                       # [S S, 3, C]
    image = mask[:, None] * (b0 * a[:, 0] + b1 * a[:, 1] + b2 * a[:, 2])
    return p2f.view(S, S), mask.view(S, S), (mask * depth).view(S, S), image.t().reshape(-1, S, S), cut


def main():
    ap = _prof.parser(__doc__, calls=20)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    import torch

    from real3dportrait_amd import MeshRenderer, _lib, rasterize, synth

    dev, S, B = "cuda:0", a.size, a.frames
    lib = _lib.load()

    def measure(fns):
        samples = _prof.alternate(_prof.routes(fns, _prof.block_median, a.calls), a.blocks, warmup=3)
        return {t: _prof.ms_spread(v) for t, v in samples.items()}

    out = {"metric": "raster_chunk_s%d_b%d" % (S, B), "S": S, "frames": B, "calls_per_block": a.calls, "blocks": a.blocks,
           "fov_deg": synth.BFM_FOV_DEG, "shader_clock": "not measured", "cases": {}}
    for G in (188, 132):
        m = synth.synth_face_mesh(G, 0)
        N, M = m["vertex"].shape[0], m["tri"].shape[0]
        shift = 0.03 * synth.hash_unitvar(1, (B, 1, 3))                  # a head that moves a little from frame to frame
        shift[..., 2] *= 3.0
        vertex = torch.from_numpy(m["vertex"][None] + shift).to(dev)
        tri = torch.from_numpy(m["tri"]).to(dev)
        feat = torch.from_numpy(m["feat"]).to(dev)[None].expand(B, -1, -1).contiguous()
        ren = MeshRenderer(synth.BFM_FOV_DEG, znear=5.0, zfar=15.0, rasterize_size=S)
        p2f, mask, depth, image = rasterize(vertex, tri, S, synth.BFM_FOV_DEG, 5.0, feat=feat)
        tri32 = tri.to(torch.int32)
        ws = torch.empty(lib.r3d_raster_workspace_bytes(B, S, M), device=dev, dtype=torch.uint8)
        P = _lib.ptr

        def stage(mask_bits):
            _lib.check(lib.r3d_debug_raster_forward(P(vertex), P(feat), P(tri32), 0, B, N, M, 3, S, synth.BFM_FOV_DEG, 5.0, 1, 1, 1.0, 0.0,
                                                    None, P(mask), P(depth), P(image), P(ws), ws.numel(), 64, mask_bits, _lib.stream_ptr()),
                       "raster stage %d" % mask_bits)

        fns = {"forward": lambda: ren(vertex, tri, feat)}
        for name, bits in STAGES:
            fns["up_to_" + name] = lambda bits=bits: stage(bits)
        res = measure(fns)
        before = 0.0
        for name, _ in STAGES:
            upto = res.pop("up_to_" + name)
            res[name] = {"ms": round(upto["ms"] - before, 4), "spread_ms_of_the_cumulative_call": upto["spread_ms"]}
            before = upto["ms"]
        for t in res:
            res[t]["ms_per_frame"] = round(res[t]["ms"] / B, 5)
        large = int(ws[B * S * S * 8:B * S * S * 8 + 4].view(torch.int32).item()) + 1 if S % 4 == 0 else None
        vneg = vertex[0] * torch.tensor([-1.0, 1.0, 1.0], device=dev)
        tp2f, tmask, tdepth, timage, cut = torch_rasterize(vneg, tri, feat[0], S, synth.BFM_FOV_DEG, 5.0)
        base = measure({"torch_one_frame": lambda: torch_rasterize(vneg, tri, feat[0], S, synth.BFM_FOV_DEG, 5.0)})
        same = tp2f == p2f[0]
        bytes_frame = {"keys_written_and_read": S * S * 8, "outputs": S * S * 4 * 5, "vertices_and_indices": N * 3 * 4 * 2 + M * 3 * 4}
        total = sum(bytes_frame.values())
        out["cases"]["G%d" % G] = {
            "faces": M, "vertices": N, "coverage": round(float((p2f >= 0).float().mean()), 4), "faces_on_the_large_path_per_chunk": large,
            "hip": res, "torch_baseline_one_frame": base["torch_one_frame"], "torch_window": WINDOW, "torch_faces_cut_by_the_window": cut,
            "torch_pix_to_face_differs_on_pixels": int((~same).sum()),
            "torch_max_abs_diff_where_same": {"depth": float((tdepth - depth[0, 0])[same].abs().max()),
                                              "image": float((timage - image[0])[:, same].abs().max())},
            "bytes_per_frame": bytes_frame, "bytes_per_frame_total": total, "ms_per_frame_at_4TBps": round(total / 4e12 * 1e3, 5)}
        print("G %d: %s" % (G, json.dumps(out["cases"]["G%d" % G])), file=sys.stderr, flush=True)
    _prof.emit(out, a.out, "prof_raster")


if __name__ == "__main__":
    main()
