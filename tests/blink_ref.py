"""The blink edit's rule (inference/edit_secc.py:47-129) in NumPy with brute-force nearest neighbours: no sklearn, no torch.

blink(img, p) restates the reference function line by line except for its two kd-tree queries, which become exhaustive searches over
exact integer squared distances.  Where a pixel to close has several nearest face pixels at the same distance the reference takes
whatever its kd-tree returns; this takes the one with the lowest (row, col) -- r3d_secc_blink's rule -- and reports the pixel in
`tie` with the colours of all its candidates in `cands`.  Maps on which the reference raises come back quantised with a status."""
import numpy as np


def quantise(img):
    """[3, h, w] float32 in [-1, 1] -> q [h, w, 3] int64, the reference's ((img + 1) / 2 * 255).astype(np.uint) (fp32 arithmetic)."""
    x = np.ascontiguousarray(np.transpose(np.asarray(img, np.float32), (1, 2, 0)))
    return np.clip(np.nan_to_num((x + 1) / 2 * 255, nan=0.0), 0, 255).astype(np.int64)


def dequantise(q):
    """q [h, w, 3] -> [3, h, w] float32, the reference's img.astype(np.float32) / 127.5 - 1."""
    return np.ascontiguousarray(np.transpose(q.astype(np.float32) / 127.5 - 1, (2, 0, 1)))


def regions(h, w):
    L, R = np.zeros((h, w), bool), np.zeros((h, w), bool)
    L[h // 4:h // 2, w // 4:w // 2] = True
    R[h // 4:h // 2, w // 2:w // 4 * 3] = True
    return L, R


def min_d2(a, b):
    """For every point of a [n, 2] the smallest squared distance to b [m, 2] (exact integers) -> [n], and the full matrix."""
    d = a[:, None, :] - b[None, :, :]
    d2 = (d * d).sum(-1)
    return d2.min(axis=1), d2


def blink(img, p):
    """-> dict(out [3, h, w] float32, status, tie [h, w] bool, cands {(row, col): [k, 3] colours of the equidistant candidates},
    q [h, w, 3] the edited 8-bit map, masks E, P, F, M, B [h, w] bool (None where the rule stops before them))."""
    assert 0.0 <= p <= 1.0
    q = quantise(img)
    h, w = q.shape[:2]
    if h < 16 or w < 16 or h > 4096 or w > 4096:
        raise ValueError("blink: map size %d x %d is not in 16 .. 4096" % (h, w))
    res = {"status": 0, "tie": np.zeros((h, w), bool), "cands": {}, "E": None, "P": None, "F": None, "M": None, "B": None}

    def done(status):
        res.update(status=status, q=q, out=dequantise(q))
        return res

    if p == 0:
        return done(0)
    face = (q[..., 0] != 0) & (q[..., 1] != 0) & (q[..., 2] != 0)
    L, R = regions(h, w)
    E = ~face & (L | R)
    res["E"] = E
    lc, rc = np.nonzero(~face & L)[1], np.nonzero(~face & R)[1]
    if lc.size == 0 or rc.size == 0:
        return done(1)
    er = np.nonzero(E)[0]
    min_h, max_h = er.min(), er.max()
    P = np.zeros((h, w), bool)
    P[min_h - 4:max_h + 4, lc.min() - 4:lc.max() + 4] = True
    P[min_h - 4:max_h + 4, rc.min() - 4:rc.max() + 4] = True
    F = face & P
    fxy, exy = np.stack(np.nonzero(F), 1), np.stack(np.nonzero(E), 1)
    if fxy.shape[0]:
        near = min_d2(fxy, exy)[0] <= 25
        F[fxy[near, 0], fxy[near, 1]] = False
    M = ~F & P
    res.update(P=P, F=F, M=M)
    fxy = np.stack(np.nonzero(F), 1)          # row-major: the first of equal distances is the lowest (row, col)
    if fxy.shape[0] == 0:
        return done(2)
    rows = np.mgrid[0:h, 0:w][0]
    cnt = M.sum(axis=0)
    mean = np.where(M, rows, 0).sum(axis=0) / np.clip(cnt, 1, h)
    mn, mx = np.where(M, rows, 99999).min(axis=0), np.where(M, rows, -99999).max(axis=0)
    lo, hi = p * mean + (1 - p) * mn, p * mean + (1 - p) * mx
    B = M & ((rows <= lo) | (rows >= hi)) & (cnt != 0)
    res["B"] = B
    bxy = np.stack(np.nonzero(B), 1)
    if bxy.shape[0]:
        best, d2 = min_d2(bxy, fxy)
        src = fxy[d2.argmin(axis=1)]
        colours = q[fxy[:, 0], fxy[:, 1]]
        for k in np.nonzero((d2 == best[:, None]).sum(axis=1) > 1)[0]:
            res["tie"][bxy[k, 0], bxy[k, 1]] = True
            res["cands"][(int(bxy[k, 0]), int(bxy[k, 1]))] = colours[d2[k] == best[k]]
        q = q.copy()
        q[bxy[:, 0], bxy[:, 1]] = q[src[:, 0], src[:, 1]]
    return done(0)


def matches_up_to_ties(res, ref_q):
    """The rule of comparison with the reference: ref_q [h, w, 3] equals res['q'] at every pixel outside the tie mask, and inside it
    carries the colour of one of the pixel's equidistant candidates.  -> (pixels differing outside the ties, tie pixels whose colour is
    none of the candidates')."""
    ref_q = np.asarray(ref_q).astype(np.int64)
    diff = (ref_q != res["q"]).any(axis=-1)
    outside = int((diff & ~res["tie"]).sum())
    bad = sum(1 for (r, c), cand in res["cands"].items() if not (cand == ref_q[r, c]).all(axis=1).any())
    return outside, bad


def transcribed_loop(clip, rng, period_frames=125):
    """inference/real3d_infer.py:411-426 transcribed, over blink() instead of the reference function: clip [T, 3, h, w] -> the edited
    copy.  Consumes rng as the reference consumes `random`."""
    out = np.array(clip, np.float32, copy=True)
    T = out.shape[0]
    for i in range(T):
        if i % period_frames == 0:
            blink_dur_frames = rng.randint(8, 12)
            for offset in range(blink_dur_frames):
                j = offset + i
                close_percent = -4 / blink_dur_frames ** 2 * offset ** 2 + 4 / blink_dur_frames * offset
                if j >= T - 1:
                    break
                out[j] = blink(out[j], close_percent)["out"]
    return out


def hand_map(h, w, eyes, seed=0):
    """A map for cases worked out by hand: face everywhere, every channel's 8-bit value drawn from 26 .. 229 (a pixel's colour tells
    where it came from), and single eye pixels (-1 in all channels) at the (row, col) positions `eyes`."""
    from real3dportrait_amd import synth
    x = 0.1 + 0.8 * synth.hash_uniform(seed, 3 * h * w, stream=60).reshape(3, h, w).astype(np.float64)
    img = (2.0 * x - 1.0).astype(np.float32)
    for r, c in eyes:
        img[:, r, c] = -1.0
    return img
