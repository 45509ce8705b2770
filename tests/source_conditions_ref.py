"""NumPy restatement of the source-image conditions (real3dportrait_amd/source_conditions.py, include/r3d_hip_source.h): the
rules of extract_background(..., 'knn') and inpaint_torso_job (data_gen/utils/process_video/extract_segment_imgs.py:63-239) written out
per pixel and per column, by another route than the kernels take.

    nearest_brute     every pixel against every seed in int64; the lowest (row, col) among equidistant seeds, and where there is a tie
    background        the whole of extract_background for already selected frames; `tie` marks the filled pixels with several candidates
    matches_up_to_ties   a recorded reference result against it: differences outside the ties, tie pixels off every candidate's colour
    inpaint_torso     inpaint_torso_job column by column, with the fixed-point blur; wrap=True is the reference's NumPy indexing (paint
                      above row 0 lands at the bottom of the image, a top pixel in row 0 looks at the bottom row), wrap=False what the
                      kernels do (such rows are dropped, such a column is not under head)
    blur_fixed        the model of cv2.GaussianBlur(img, (5, 5), 4)'s 8-bit path: separable, 8 fractional bits, reflect-101
    blur_fp64         the same blur with the exact weights in fp64, rounded
"""
import numpy as np

BLUR_WEIGHTS = (48, 53, 54, 53, 48)
TORSO_L, NECK_L, PUSH_DOWN, DILATE = 9, 53, 4, 3


def nearest_brute(mask, chunk=256):
    """mask [H, W] (a seed where not 0) -> (d2 [H, W] int64, index [H, W] int64 = row * W + col of the nearest seed with the lowest
    (row, col), tie [H, W] bool: more than one seed at that distance)."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    sr, sc = np.nonzero(mask)                     # row-major: ascending (row, col)
    assert len(sr) > 0, "no seed"
    sr, sc = sr.astype(np.int64), sc.astype(np.int64)
    pr, pc = (a.reshape(-1).astype(np.int64) for a in np.mgrid[0:H, 0:W])
    d2, index, tie = np.empty(H * W, np.int64), np.empty(H * W, np.int64), np.empty(H * W, bool)
    for lo in range(0, H * W, chunk):
        D = (pr[lo:lo + chunk, None] - sr[None]) ** 2 + (pc[lo:lo + chunk, None] - sc[None]) ** 2
        m = D.min(axis=1)
        first = (D == m[:, None]).argmax(axis=1)          # the first seed in (row, col) order at the minimum
        d2[lo:lo + chunk], index[lo:lo + chunk] = m, sr[first] * W + sc[first]
        tie[lo:lo + chunk] = (D == m[:, None]).sum(axis=1) > 1
    return d2.reshape(H, W), index.reshape(H, W), tie.reshape(H, W)


def background(imgs, bgs):
    """imgs [B, H, W, 3] uint8, bgs [B, H, W] (segmap plane 0 of each frame) -> dict: out [H, W, 3], sure [H, W], frame [H, W] (the first
    frame with the largest distance), d2max [H, W], index [H, W] (the sure pixel a filled pixel copies), tie [H, W] (a filled pixel with
    several equidistant sure pixels)."""
    imgs, bgs = np.asarray(imgs), np.asarray(bgs) != 0
    B, H, W = bgs.shape
    d2 = np.stack([nearest_brute(~bgs[b])[0] for b in range(B)])
    d2max, frame = d2.max(axis=0), d2.argmax(axis=0)
    sure = d2max > 100                            # max_dist > 10
    assert sure.any(), "no sure pixel"
    stage = np.zeros((H, W, 3), np.uint8)
    rr, cc = np.nonzero(sure)
    stage[rr, cc] = imgs[frame[rr, cc], rr, cc]
    _, index, tie = nearest_brute(sure)
    out = stage.copy()
    fr, fc = np.nonzero(~sure)
    src = index[fr, fc]
    out[fr, fc] = stage[src // W, src % W]
    return {"out": out, "sure": sure, "frame": frame, "d2max": d2max, "index": index, "tie": tie & ~sure, "stage": stage}


def matches_up_to_ties(res, reference_out):
    """-> (pixels outside the tie mask where reference_out differs from res['out'], tie pixels whose reference colour is the colour of
    none of their equidistant sure pixels)."""
    out, tie, sure, stage = res["out"], res["tie"], res["sure"], res["stage"]
    differ = (out != reference_out).any(axis=-1)
    outside = int((differ & ~tie).sum())
    H, W = tie.shape
    sr, sc = (a.astype(np.int64) for a in np.nonzero(sure))
    bad = 0
    for r, c in zip(*np.nonzero(tie)):
        D = (sr - r) ** 2 + (sc - c) ** 2
        cand = D == D.min()
        bad += int(not (stage[sr[cand], sc[cand]] == reference_out[r, c]).all(axis=-1).any())
    return outside, bad


def _reflect101(x, pad, axis):
    width = [(0, 0)] * x.ndim
    width[axis] = (pad, pad)
    return np.pad(x, width, mode="reflect")       # NumPy's 'reflect' does not repeat the edge: OpenCV's BORDER_REFLECT_101


def blur_fixed(img, weights=BLUR_WEIGHTS):
    """img [H, W, 3] uint8 -> the 5 x 5 blur: a 16-bit horizontal sum of weights with 8 fractional bits, then the vertical sum rounded half
    up, (v + 2^15) >> 16."""
    w = [int(v) for v in weights]
    H, W = img.shape[:2]
    x = _reflect101(img.astype(np.uint32), 2, 1)
    h = sum(w[i] * x[:, i:i + W] for i in range(5))
    assert h.max() < 65536
    y = _reflect101(h, 2, 0)
    v = sum(w[k] * y[k:k + H] for k in range(5))
    return np.minimum((v + 32768) >> 16, 255).astype(np.uint8)


def gaussian_weights(sigma=4.0):
    g = np.exp(-np.arange(-2, 3, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return g / g.sum()


def blur_fp64(img, sigma=4.0):
    g = gaussian_weights(sigma)
    H, W = img.shape[:2]
    x = _reflect101(img.astype(np.float64), 2, 1)
    h = sum(g[i] * x[:, i:i + W] for i in range(5))
    y = _reflect101(h, 2, 0)
    v = sum(g[k] * y[k:k + H] for k in range(5))
    return np.floor(v + 0.5)


def blur_bound(weights=BLUR_WEIGHTS, sigma=4.0):
    """The largest difference, in counts, between blur_fixed and blur_fp64.  Both weigh the same 25 bytes, with Q[i][j] = q_i q_j / 2^16
    and G[i][j] = g_i g_j; the fixed-point sums are exact until the final shift, so the two real numbers before rounding differ by at
    most 255 sum |Q - G|, and each is rounded once, by at most 1 / 2: two integers that differ by at most 255 sum |Q - G| + 1.  (With
    |Q - G| <= e_i g_j + (q_i / 256) e_j, e_i = |q_i / 256 - g_i|, the sum is at most 2 sum e_i = 0.0077, times 255: 1.97.)"""
    q, g = np.asarray(weights, np.float64) / 256.0, gaussian_weights(sigma)
    return int(np.floor(255.0 * np.abs(np.outer(q, q) - np.outer(g, g)).sum() + 1.0))


def inpaint_torso(img, segmap, weights=BLUR_WEIGHTS, wrap=False):
    """img [H, W, 3] uint8, segmap [6, H, W] -> (torso_img, torso_img_mask, torso_with_bg_img, torso_with_bg_img_mask, info).  info counts
    what the synthetic portraits must contain: torso_cols (clothes directly under head), neck_cols_lt5 / neck_cols_gt5 (kept neck columns
    by their pixel count), dilated_only (pixels the dilation adds), and `wraps`: whether wrap=True and wrap=False differ on this input."""
    img = np.asarray(img)
    seg = np.asarray(segmap) != 0
    H, W = img.shape[:2]
    bg, neck, torso = seg[0], seg[2], seg[4]
    head = seg[1] | seg[3] | seg[5]
    darken = 0.98 ** np.arange(NECK_L)
    work = img.copy()
    work[head] = 0
    info = {"torso_cols": 0, "neck_cols_lt5": 0, "neck_cols_gt5": 0, "wraps": False}

    dilated = neck.copy()                         # 3 iterations of a 3 x 1 structure with a zero border: 3 rows up and down
    for k in range(1, DILATE + 1):
        dilated[k:] |= neck[:-k]
        dilated[:-k] |= neck[k:]
    info["dilated_only"] = int((dilated & ~neck).sum())

    def paint(mask2d, L, push):
        """The columns of mask2d whose top pixel lies under head, painted L rows upward from the (pushed-down) top; returns the paint mask."""
        painted = np.zeros((H, W), bool)
        jobs = []
        for c in range(W):
            rows = np.nonzero(mask2d[:, c])[0]
            if len(rows) == 0:
                continue
            top, count = int(rows[0]), len(rows)
            if top == 0:
                info["wraps"] = True
                if not wrap or not head[H - 1, c]:
                    continue
            elif not head[top - 1, c]:
                continue
            start = top + (min(count - 1, push) if push else 0)
            jobs.append((c, start, count))
        for c, start, count in jobs:              # every colour is read from the unedited image
            for k in range(L):
                r = start - k
                if r < 0:
                    info["wraps"] = True
                    if not wrap:
                        break
                    r += H
                work[r, c] = (img[start, c] * darken[k]).astype(np.uint8)          # fp64 product, truncated
                painted[r, c] = True
        return painted, jobs

    torso_paint, jobs = paint(torso, TORSO_L, 0)
    info["torso_cols"] = len(jobs)
    neck_paint, jobs = paint(dilated, NECK_L, PUSH_DOWN)
    info["neck_cols_lt5"] = sum(1 for _, _, n in jobs if n < 5)
    info["neck_cols_gt5"] = sum(1 for _, _, n in jobs if n > 5)

    info["painted"] = work.copy()                 # the image the blur reads
    blurred = blur_fixed(work, weights)
    work[neck_paint] = blurred[neck_paint]
    torso_mask = dilated | torso | neck_paint | torso_paint
    with_bg_mask = bg | torso_mask
    torso_img = work.copy()
    torso_img[~torso_mask] = 0
    return torso_img, torso_mask, work.copy(), with_bg_mask, dict(info, neck_paint=neck_paint)


def head_image(img, segmap):
    seg = np.asarray(segmap) != 0
    sel = seg[1] | seg[3] | seg[5]
    out = np.asarray(img).copy()
    out[~sel] = 0
    return out, sel[None]


def frames_of(g):
    """A source_cond_* fixture -> (imgs [B, H, W, 3] uint8, segmaps [B, 6, H, W] uint8 one-hot).  With B = 3 the file holds frames 0 and 2;
    frame 1 has frame 0's segmap and the image 255 - frame 0 (identical masks, another image: np.argmax's first-frame rule shows)."""
    B = int(g["spec"][3])
    img = g["img"]
    imgs = img if B == 1 else np.stack([img[0], 255 - img[0], img[1]])
    segs = (g["label"][:, None] == np.arange(6, dtype=np.uint8)[None, :, None, None]).astype(np.uint8)
    return np.ascontiguousarray(imgs), segs
