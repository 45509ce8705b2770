"""Time the HIP blink edit on the blink of one period of the reference's loop (inference/real3d_infer.py:411-426): the 10
frames 0 .. 9 of a 125-frame clip at 512 x 512, closing percentages -4/100 k^2 + 4/10 k, on synth_secc_eyes(512, 512, seed k), and print
one JSON line:

  * one batched r3d_secc_blink call over the 10 frames (a memset and four kernels), device events around every call, `calls` calls per
    block, `blocks` blocks after a warm-up; reported: the median of the block medians and their spread.  The timed calls read the
    pristine clip and write a second buffer (out != secc: the same reads and writes as in place), so every call sees the same input;
  * the memset and each kernel, the same way, through the stage mask of the test hook r3d_debug_secc_blink: the call cut off after the
    clear, after quantise_bounds, after erode, after columns and complete, each kernel's time being the difference of two such medians;
  * one blink_eye_for_secc call on one frame at p = 0.64 with the synchronisation its status read costs (host wall clock);
  * where sklearn imports: the reference's route on the same maps -- the frame copied to the host, the rule with two kd-trees (this
    script's own NumPy + sklearn code, not the reference's), the result copied back -- per frame, host wall clock, and the number of
    pixels on which the two results differ (the documented choice among equidistant face pixels).  Where it does not import, the JSON
    says so and quotes the figure measured elsewhere.

    python scripts/prof_blink.py [--calls 20] [--blocks 5] [--size 512] [--out DIR]     (writes DIR/prof_blink.json)
"""
import os
import statistics
import time

import _prof

_prof.paths()

STAGES = (("clear", 1), ("quantise_bounds", 3), ("erode", 7), ("columns", 15), ("fill", 31))          # cumulative stage masks
HOST_FIGURE = "41 to 51 ms per frame at p > 0 and 6 ms at p = 0 for the reference function with sklearn 1.7.2, measured on a CPU-only machine"


def kdtree_blink(img, p):
    """The rule of DESIGN 4.15 on the host with sklearn's kd-trees for its two nearest-neighbour queries: img [3, h, w] float32 ->
    (out [3, h, w] float32, the number of edited pixels)."""
    import numpy as np
    from sklearn.neighbors import NearestNeighbors
    q = ((np.transpose(img, (1, 2, 0)) + 1) / 2 * 255).astype(np.int64)
    back = lambda q: np.ascontiguousarray(np.transpose(q.astype(np.float32) / 127.5 - 1, (2, 0, 1)))
    if p == 0:
        return back(q), 0
    h, w = q.shape[:2]
    face = (q != 0).all(axis=-1)
    L, R = np.zeros((h, w), bool), np.zeros((h, w), bool)
    L[h // 4:h // 2, w // 4:w // 2] = True
    R[h // 4:h // 2, w // 2:w // 4 * 3] = True
    E = ~face & (L | R)
    exy = np.stack(np.nonzero(E), 1)
    lc, rc = np.nonzero(~face & L)[1], np.nonzero(~face & R)[1]
    P = np.zeros((h, w), bool)
    r0, r1 = exy[:, 0].min() - 4, exy[:, 0].max() + 4
    P[r0:r1, lc.min() - 4:lc.max() + 4] = True
    P[r0:r1, rc.min() - 4:rc.max() + 4] = True
    F = face & P
    fxy = np.stack(np.nonzero(F), 1)
    d, _ = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(exy).kneighbors(fxy)
    near = fxy[d[:, 0] <= 5]
    F[near[:, 0], near[:, 1]] = False
    M = ~F & P
    rows = np.mgrid[0:h, 0:w][0]
    cnt = M.sum(axis=0)
    mean = np.where(M, rows, 0).sum(axis=0) / np.clip(cnt, 1, h)
    lo = p * mean + (1 - p) * np.where(M, rows, 99999).min(axis=0)
    hi = p * mean + (1 - p) * np.where(M, rows, -99999).max(axis=0)
    B = M & ((rows <= lo) | (rows >= hi))
    fxy, bxy = np.stack(np.nonzero(F), 1), np.stack(np.nonzero(B), 1)
    _, ind = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(fxy).kneighbors(bxy)
    src = fxy[ind[:, 0]]
    q[bxy[:, 0], bxy[:, 1]] = q[src[:, 0], src[:, 1]]
    return back(q), int(bxy.shape[0])


def main():
    ap = _prof.parser(__doc__, calls=20)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    import numpy as np
    import torch

    from real3dportrait_amd import _lib, blink_eye_for_secc, blink_frames, synth

    dev, S, T, F = "cuda:0", a.size, 125, 10
    lib = _lib.load()
    frames = [j for j in range(F)]
    percents = [-4 / F ** 2 * k ** 2 + 4 / F * k for k in range(F)]
    maps = np.stack([synth.synth_secc_eyes(S, S, k) for k in range(F)])
    clip = torch.from_numpy(maps[0])[None].repeat(T, 1, 1, 1)
    clip[:F] = torch.from_numpy(maps)
    clip = clip.to(dev)
    out_buf = torch.empty_like(clip)
    d_idx = torch.tensor(frames, dtype=torch.int32, device=dev)
    d_pct = torch.tensor(percents, dtype=torch.float64, device=dev)
    status = torch.empty(F, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.r3d_secc_blink_workspace_bytes(F, S, S), device=dev, dtype=torch.uint8)
    P = _lib.ptr

    def call():
        _lib.check(lib.r3d_secc_blink(P(clip), T, S, S, P(d_idx), P(d_pct), F, P(out_buf), P(status), P(ws), ws.numel(), _lib.stream_ptr()),
                   "secc_blink")

    def stage(bits):
        _lib.check(lib.r3d_debug_secc_blink(P(clip), T, S, S, P(d_idx), P(d_pct), F, P(out_buf), P(status), P(ws), ws.numel(), bits,
                                            _lib.stream_ptr()), "secc_blink stage %d" % bits)

    fns = {"call": call}
    for name, bits in STAGES:
        fns["up_to_" + name] = lambda bits=bits: stage(bits)
    samples = _prof.alternate(_prof.routes(fns, _prof.block_median, a.calls), a.blocks, warmup=3)
    res = {t: _prof.ms_spread(v) for t, v in samples.items()}
    before = 0.0
    for name, _ in STAGES:
        upto = res.pop("up_to_" + name)
        res[name] = {"ms": round(upto["ms"] - before, 4), "spread_ms_of_the_cumulative_call": upto["spread_ms"]}
        before = upto["ms"]
    for t in res:
        res[t]["ms_per_frame"] = round(res[t]["ms"] / F, 5)
    call()
    torch.cuda.synchronize()
    head = ws[:F * 256].view(torch.int32).view(F, 64).cpu()
    gpu = out_buf[:F].cpu().numpy()

    one = clip[6].clone()
    one_frame = lambda: blink_eye_for_secc(one, 0.64)          # ends in its status read, a synchronisation
    _prof.by_host_clock(one_frame, 3)
    walls = [_prof.by_host_clock(one_frame, 1) for _ in range(a.calls)]

    def batched_in_place():
        work = clip[:F + 1].clone()
        return _prof.by_host_clock(lambda: blink_frames(work, frames, percents), 1)
    batched_in_place()
    batched = [batched_in_place() for _ in range(a.calls)]

    out = {"metric": "secc_blink_%d_frames_s%d" % (F, S), "S": S, "clip_frames": T, "blink_frames": F, "percents": [round(p, 4) for p in percents],
           "calls_per_block": a.calls, "blocks": a.blocks, "shader_clock": "not measured", "status": status.cpu().tolist(),
           "face_pixels_per_frame": head[:, 6].tolist(), "blink_pixels_per_frame": head[:, 7].tolist(), "hip": res,
           "blink_frames_in_place_with_its_uploads_and_a_sync_wall_ms": {"median": round(statistics.median(batched), 4), "min": round(min(batched), 4)},
           "blink_eye_for_secc_one_frame_with_its_sync_wall_ms": {"median": round(statistics.median(walls), 4), "min": round(min(walls), 4)}}
    try:
        import sklearn
        have = True
    except ImportError:
        have = False
    if have:
        per_frame, differ, edited = [], [], []
        for k in range(F):
            best = None
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = clip[k].cpu().numpy()
                edit, n = kdtree_blink(host, percents[k])
                back = torch.from_numpy(edit).to(dev)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None else min(best, dt)
            per_frame.append(round(best, 3))
            edited.append(n)
            differ.append(int((back.cpu().numpy() != gpu[k]).any(axis=0).sum()))
        out["host_kdtree_path"] = {"sklearn": sklearn.__version__, "cpus": os.cpu_count(), "ms_per_frame_best_of_3": per_frame,
                                   "ms_for_the_blink": round(sum(per_frame), 3), "edited_pixels": edited,
                                   "pixels_differing_from_the_hip_result": differ}
    else:
        out["host_kdtree_path"] = {"sklearn": "does not import on this machine", "quoted": HOST_FIGURE}
    _prof.emit(out, a.out, "prof_blink")


if __name__ == "__main__":
    main()
