"""Time the HIP source-image conditions on one synthetic portrait, synth_portrait_segmap / synth_portrait_image at 512 x 512,
B = 1, what prepare_batch_from_inp does once per clip (inference/real3d_infer.py:247-260), and print one JSON line:

  * source_conditions(img, segmap) with the image and the segmap already on the device: warm, `calls` back-to-back calls per block, host
    clock around the block (every call ends in the 8-byte status read, a synchronisation), `blocks` blocks; the median and the spread of
    the blocks' per-call times;
  * each entry point alone, the same way but with one synchronisation at the block's end: r3d_source_nearest on the person mask (d2 and
    index), r3d_source_background, r3d_source_torso, r3d_source_to_planes;
  * the row pass's distance from its integer-issue floor: H W W key evaluations of 5 vector instructions (add, 24-bit multiply-add,
    64-bit compare, two selects), 2 cycles each per wave of 64 on the 1024 SIMDs, at the 2.4 GHz peak clock (the clock during the run is
    not measured); the nearest-seed time also holds the column pass and a launch boundary, so this is an upper bound of the distance;
  * where sklearn and scipy import: the host route of the same three functions on this machine's CPU -- this script's own NumPy code
    with two sklearn kd-trees, scipy's binary_dilation and the fixed-point blur model -- with the upload of its results, host wall clock,
    best of 3; and on how many pixels the two routes differ (the background: the documented choice among equidistant sure pixels; the
    torso and the head: none).  Where they do not import, the JSON says so and quotes the figure measured elsewhere.

    python scripts/prof_source_conditions.py [--calls 20] [--blocks 5] [--size 512] [--out DIR]     (writes DIR/prof_source_conditions.json)
"""
import ctypes
import os
import time

import _prof

_prof.paths()

HOST_FIGURE = "1.2 s for the two kd-tree stages at 512 x 512 with sklearn 1.7.2, one run on a CPU-only machine: a stand-in from another host"
BLUR = (48, 53, 54, 53, 48)


def host_background(img, seg):
    """extract_background([img], [seg], 'knn')'s rule with sklearn's kd-trees."""
    import numpy as np
    from sklearn.neighbors import NearestNeighbors
    h, w = img.shape[:2]
    grid = np.mgrid[0:h, 0:w].reshape(2, -1).T
    person = np.stack(np.nonzero(seg[0] == 0), 1)
    dist, _ = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(person).kneighbors(grid)
    sure = dist.reshape(h, w) > 10
    out = np.where(sure[..., None], img, 0).astype(np.uint8)
    known, fill = np.stack(np.nonzero(sure), 1), np.stack(np.nonzero(~sure), 1)
    _, ind = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(known).kneighbors(fill)
    src = known[ind[:, 0]]
    out[fill[:, 0], fill[:, 1]] = out[src[:, 0], src[:, 1]]
    return out


def host_blur(img):
    import numpy as np
    h, w = img.shape[:2]
    x = np.pad(img.astype(np.uint32), ((0, 0), (2, 2), (0, 0)), mode="reflect")
    hor = sum(BLUR[i] * x[:, i:i + w] for i in range(5))
    y = np.pad(hor, ((2, 2), (0, 0), (0, 0)), mode="reflect")
    return ((sum(BLUR[k] * y[k:k + h] for k in range(5)) + 32768) >> 16).astype(np.uint8)


def host_torso(img, seg):
    """inpaint_torso_job's rule, vectorised over the columns, with scipy's dilation and the blur model; paint above row 0 is dropped."""
    import numpy as np
    from scipy.ndimage import binary_dilation
    h, w = img.shape[:2]
    s = seg != 0
    head, torso = s[1] | s[3] | s[5], s[4]
    neck = binary_dilation(s[2], structure=np.array([[0, 1, 0]] * 3, dtype=bool), iterations=3)
    work = img.copy()
    work[head] = 0
    darken = 0.98 ** np.arange(53)
    paints = []
    for mask, L, push in ((torso, 9, 0), (neck, 53, 4)):
        cols = np.nonzero(mask.any(axis=0))[0]
        top, count = mask.argmax(axis=0)[cols], mask.sum(axis=0)[cols]
        keep = (top >= 1) & head[np.maximum(top - 1, 0), cols]
        cols, start = cols[keep], (top + (np.minimum(count - 1, push) if push else 0))[keep]
        rows = start[None] - np.arange(L)[:, None]
        ok = rows >= 0
        colour = (img[start, cols][None] * darken[:L, None, None]).astype(np.uint8)
        cc = np.broadcast_to(cols[None], rows.shape)
        work[rows[ok], cc[ok]] = colour[ok]
        painted = np.zeros((h, w), bool)
        painted[rows[ok], cc[ok]] = True
        paints.append(painted)
    work[paints[1]] = host_blur(work)[paints[1]]
    torso_mask = neck | torso | paints[0] | paints[1]
    out = work.copy()
    out[~torso_mask] = 0
    return out, torso_mask, work, s[0] | torso_mask


def main():
    ap = _prof.parser(__doc__, calls=20)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    import numpy as np
    import torch

    from real3dportrait_amd import _lib, synth
    from real3dportrait_amd import source_conditions as S

    dev, N = "cuda:0", a.size
    img_np, seg_np = synth.synth_portrait_image(N, N, 1), synth.synth_portrait_segmap(N, N, 1)
    img, seg = torch.from_numpy(img_np).to(dev), torch.from_numpy(seg_np).to(dev)
    person = (seg[0] == 0).to(torch.uint8)[None].contiguous()
    ws = torch.empty(_lib.call("r3d_source_workspace_bytes", 1, N, N), dtype=torch.uint8, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    d2, index = (torch.empty(1, N, N, dtype=torch.int32, device=dev) for _ in range(2))
    outs = [torch.empty(N, N, 3, dtype=torch.uint8, device=dev) for _ in range(3)]
    masks = [torch.empty(N, N, dtype=torch.uint8, device=dev) for _ in range(2)]
    planes = torch.empty(1, 3, N, N, dtype=torch.float32, device=dev)
    darken = (ctypes.c_double * 53)(*(0.98 ** np.arange(53)).tolist())
    weights = (ctypes.c_int * 5)(*BLUR)
    fns = {
        "source_conditions": lambda: S.source_conditions(img, seg),
        "nearest": lambda: _lib.call("r3d_source_nearest", person, 1, N, N, d2, index, status, ws, ws.numel()),
        "background": lambda: _lib.call("r3d_source_background", img[None], seg[:1], 1, N, N, outs[0], status, ws, ws.numel()),
        "torso": lambda: _lib.call("r3d_source_torso", img, seg, N, N, darken, weights, outs[1], masks[0], outs[2], masks[1], ws, ws.numel()),
        "to_planes": lambda: _lib.call("r3d_source_to_planes", img, seg, S.HEAD_CLASSES, N, N, planes),
    }
    per_call = _prof.alternate(_prof.routes(fns, _prof.by_host_clock, a.calls), a.blocks, warmup=3)
    hip = {t: _prof.ms_spread(v) for t, v in per_call.items()}
    evaluations = N * N * N
    floor_ms = evaluations / 64 * 5 * 2 / 1024 / 2.4e9 * 1e3
    out = {"metric": "source_conditions_s%d" % N, "S": N, "B": 1, "calls_per_block": a.calls, "blocks": a.blocks, "shader_clock": "not measured",
           "timing": "host clock around back-to-back calls ending in a synchronise, per call", "hip": hip,
           "row_pass_floor": {"key_evaluations": evaluations, "vector_instructions_per_evaluation": 5, "floor_ms_at_2.4_GHz": round(floor_ms, 4),
                              "nearest_ms_over_floor": round(hip["nearest"]["ms"] / floor_ms, 2),
                              "note": "the nearest time holds the column pass, a memset and two launch boundaries as well"}}
    got = S.source_conditions(img, seg)
    dev_bg, dev_torso = outs[0].cpu().numpy(), S.inpaint_torso_job(img, seg)
    try:
        import scipy
        import sklearn
        have = True
    except ImportError:
        have = False
    if have:
        stages = {}

        def best_of_3(name, fn):
            best = None
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None else min(best, dt)
            stages[name] = round(best, 3)
            return res
        to_dev = lambda x: ((torch.tensor(x) - 127.5) / 127.5).float().unsqueeze(0).permute(0, 3, 1, 2).to(dev)
        bg = best_of_3("background_two_kd_trees", lambda: host_background(img_np, seg_np))
        torso = best_of_3("torso_job", lambda: host_torso(img_np, seg_np))
        head = best_of_3("head_image", lambda: np.where((seg_np[[1, 3, 5]].sum(0) > 0)[..., None], img_np, 0).astype(np.uint8))
        best_of_3("normalise_and_upload_three_images", lambda: [to_dev(x) for x in (head, torso[0], bg)])
        out["host_route"] = {"sklearn": sklearn.__version__, "scipy": scipy.__version__, "cpus": os.cpu_count(), "ms_best_of_3": stages,
                             "ms_total": round(sum(stages.values()), 3),
                             "background_pixels_differing_from_the_hip_result": int((bg != dev_bg).any(axis=-1).sum()),
                             "torso_pixels_differing_from_the_hip_result": int(sum((x != y.cpu().numpy()).sum() for x, y in zip(torso, dev_torso))),
                             "head_values_differing_from_the_hip_result": int((to_dev(head) != got["ref_head_img"]).sum())}
    else:
        out["host_route"] = {"sklearn_or_scipy": "does not import on this machine", "quoted": HOST_FIGURE}
    _prof.emit(out, a.out, "prof_source_conditions")


if __name__ == "__main__":
    main()
