"""The yardstick of the HIP mesh rasteriser (real3dportrait_amd/mesh_renderer.py, r3d_raster_forward of include/r3d_hip.h):
the rasterisation rule of MeshRenderer.forward (deep_3drecon/util/mesh_renderer.py:53-130: pytorch3d with image_size = S,
blur_radius = 0, faces_per_pixel = 1, cull_backfaces = False, FoVPerspectiveCameras(fov, znear, zfar)) restated in NumPy with the number
format as an argument.  float64 is the reference; the float32 instance, with every operation rounded to fp32 in the order written here,
gives the error an fp32 evaluation of the rule makes.  NumPy only: no torch operator that could hide a convention.

pytorch3d is not installed anywhere this suite runs: the rule is restated from its naive rasteriser, and equality with pytorch3d itself
has not been measured.

  1. vertex [B, N, 3] camera space (x negated first, as the reference does on its copy), tri [M, 3] or [B, M, 3], feat [B, N, C]
  2. x_ndc = s x / z, y_ndc = s y / z, s = 1 / tan(fov / 2) (fov as the fp32 number of degrees the C entry point receives)
  3. pixel (row i, column j): y_ndc = -1 + (2 (S - 1 - i) + 1) / S, x_ndc = -1 + (2 (S - 1 - j) + 1) / S
  4. edge(p, a, b) = (p.x - a.x)(b.y - a.y) - (p.y - a.y)(b.x - a.x); area = edge(v2, v0, v1), skipped when |area| <= 1e-8;
     A = area + 1e-8; w0 = edge(p, v1, v2) / A, w1 = edge(p, v2, v0) / A, w2 = edge(p, v0, v1) / A; covered iff all > 0;
     t0 = w0 z1 z2, t1 = z0 w1 z2, t2 = z0 z1 w2; b_k = t_k / max(t0 + t1 + t2, 1e-8); pz = b0 z0 + b1 z1 + b2 z2, rejected when < 0
  5. the smallest pz wins, the lower face index on an exact tie
  6. pix_to_face = b M + f or -1; mask = pix_to_face > 0 (>= 0 with first_face_is_background = False); depth = mask pz;
     image = mask sum_k b_k feat[tri[f, k]]; empty pixels are 0
  7. dropped: a face with a vertex at z < znear / 2 or z <= 0, a non-finite vertex or projection, or an index outside [0, N)
"""
import numpy as np

EPS = 1e-8
SMALL = 8          # faces whose pixel box is at most SMALL x SMALL are evaluated together, the others one by one


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def pixel_ndc(S, dtype):
    """NDC coordinate of the pixel centres 0 .. S - 1 of either axis (rule 3)."""
    i = np.arange(S)
    return dtype(-1.0) + (2 * (S - 1 - i) + 1).astype(dtype) / dtype(S)


def _evaluate(F, px, py, dtype):
    """Rule 4 for faces F (a tuple of arrays that broadcast against the pixel centres px, py): covered, b0, b1, b2, pz."""
    x0, y0, x1, y1, x2, y2, z0, z1, z2, A = F
    eps = dtype(EPS)
    w0 = _edge(px, py, x1, y1, x2, y2) / A
    w1 = _edge(px, py, x2, y2, x0, y0) / A
    w2 = _edge(px, py, x0, y0, x1, y1) / A
    t0, t1, t2 = w0 * z1 * z2, z0 * w1 * z2, z0 * z1 * w2
    den = np.maximum(t0 + t1 + t2, eps)
    b0, b1, b2 = t0 / den, t1 / den, t2 / den
    pz = b0 * z0 + b1 * z1 + b2 * z2
    return (w0 > 0) & (w1 > 0) & (w2 > 0) & (pz >= 0), b0, b1, b2, pz


def _one_mesh(v, tri, S, s, zmin, dtype, brute):
    """Candidates of one mesh: (pixel = i S + j, face, b0, b1, b2, pz) of every covered (face, pixel) pair."""
    N = v.shape[0]
    ok = ((tri >= 0) & (tri < N)).all(axis=1)
    t = np.where(ok[:, None], tri, 0)
    with np.errstate(all="ignore"):
        P = v[t]                                                           # [M, 3 corners, 3]
        z = P[:, :, 2]
        ok &= (z >= dtype(zmin)).all(axis=1) & (z > 0).all(axis=1) & np.isfinite(P).all(axis=(1, 2))
        zs = np.where(ok[:, None], z, dtype(1.0))
        xn, yn = (s * P[:, :, 0]) / zs, (s * P[:, :, 1]) / zs
        ok &= np.isfinite(xn).all(axis=1) & np.isfinite(yn).all(axis=1)
        area = _edge(xn[:, 2], yn[:, 2], xn[:, 0], yn[:, 0], xn[:, 1], yn[:, 1])
        ok &= np.abs(area) > dtype(EPS)
    faces = np.nonzero(ok)[0]
    xn, yn, z, A = xn[faces], yn[faces], z[faces], (area + dtype(EPS))[faces]
    # the box of pixel centres that can lie inside, half a pixel wider than the triangle's (in fp64 whatever dtype: it decides nothing)
    pos = lambda c: S - 0.5 - (c.astype(np.float64) + 1.0) * (0.5 * S)
    if brute:
        j0 = i0 = np.zeros(len(faces), np.int64)
        j1 = i1 = np.full(len(faces), S - 1, np.int64)
    else:
        j0 = np.clip(np.ceil(pos(xn.max(axis=1)) - 0.5), 0, S).astype(np.int64)
        j1 = np.clip(np.floor(pos(xn.min(axis=1)) + 0.5), -1, S - 1).astype(np.int64)
        i0 = np.clip(np.ceil(pos(yn.max(axis=1)) - 0.5), 0, S).astype(np.int64)
        i1 = np.clip(np.floor(pos(yn.min(axis=1)) + 0.5), -1, S - 1).astype(np.int64)
    w, h = j1 - j0 + 1, i1 - i0 + 1
    centre = pixel_ndc(S, dtype)
    col = lambda sel: tuple(a[sel][:, None] for a in (xn[:, 0], yn[:, 0], xn[:, 1], yn[:, 1], xn[:, 2], yn[:, 2], z[:, 0], z[:, 1], z[:, 2], A))
    out = []
    small = (w > 0) & (h > 0) & (w <= SMALL) & (h <= SMALL)
    if small.any():
        oi, oj = (o.reshape(-1) for o in np.meshgrid(np.arange(SMALL), np.arange(SMALL), indexing="ij"))
        inside = (oj[None, :] < w[small][:, None]) & (oi[None, :] < h[small][:, None])
        pj = np.minimum(j0[small][:, None] + oj[None, :], S - 1)
        pi = np.minimum(i0[small][:, None] + oi[None, :], S - 1)
        cov, b0, b1, b2, pz = _evaluate(col(small), centre[pj], centre[pi], dtype)
        cov &= inside
        fid = np.broadcast_to(faces[small][:, None], cov.shape)
        out.append((pi[cov] * S + pj[cov], fid[cov], b0[cov], b1[cov], b2[cov], pz[cov]))
    for k in np.nonzero((w > 0) & (h > 0) & ~small)[0]:
        pi, pj = (o.reshape(1, -1) for o in np.meshgrid(np.arange(i0[k], i1[k] + 1), np.arange(j0[k], j1[k] + 1), indexing="ij"))
        cov, b0, b1, b2, pz = _evaluate(col([k]), centre[pj], centre[pi], dtype)
        out.append(((pi * S + pj)[cov], np.full(int(cov.sum()), faces[k]), b0[cov], b1[cov], b2[cov], pz[cov]))
    if not out:
        return tuple(np.zeros(0, d) for d in (np.int64, np.int64, dtype, dtype, dtype, dtype))
    return tuple(np.concatenate(c) for c in zip(*out))


def rasterize(vertex, tri, feat, S, fov_deg, znear, dtype=np.float64, negate_x=True, first_face_is_background=True, brute=False):
    """Rules 1-7 in `dtype`.  {pix_to_face [B, S, S] int64, mask, depth [B, 1, S, S], image [B, C, S, S] or None, bary [B, S, S, 3]}, the
    floating ones in `dtype`.  brute: every face is tested at every pixel (no boxes; small sizes only)."""
    dtype = np.dtype(dtype).type
    vertex, tri = np.asarray(vertex), np.asarray(tri).astype(np.int64)
    B, N = vertex.shape[:2]
    M = tri.shape[-2]
    v = vertex.astype(dtype)
    if negate_x:
        v = v.copy()
        v[..., 0] = -v[..., 0]
    s = dtype(1.0 / np.tan(np.radians(float(np.float32(fov_deg))) * 0.5))
    C = None if feat is None else np.asarray(feat).shape[-1]
    p2f = np.full((B, S * S), -1, np.int64)
    depth, mask, bary = np.zeros((B, S * S), dtype), np.zeros((B, S * S), dtype), np.zeros((B, S * S, 3), dtype)
    image = None if feat is None else np.zeros((B, C, S * S), dtype)
    for b in range(B):
        tb = tri[b] if tri.ndim == 3 else tri
        pix, f, b0, b1, b2, pz = _one_mesh(v[b], tb, S, s, 0.5 * znear, dtype, brute)
        order = np.lexsort((f, pz, pix))                    # by pixel, then depth, then face index: rule 5
        pix, f, b0, b1, b2, pz = (a[order] for a in (pix, f, b0, b1, b2, pz))
        first = np.ones(len(pix), bool)
        first[1:] = pix[1:] != pix[:-1]
        pix, f, b0, b1, b2, pz = (a[first] for a in (pix, f, b0, b1, b2, pz))
        p2f[b, pix] = b * M + f
        m = (p2f[b, pix] > 0) if first_face_is_background else np.ones(len(pix), bool)
        mask[b, pix] = m.astype(dtype)
        depth[b, pix] = m.astype(dtype) * pz
        bary[b, pix] = np.stack([b0, b1, b2], axis=1)
        if feat is not None:
            a = np.asarray(feat)[b].astype(dtype)[tb[f]]          # [pixels, 3 corners, C]
            val = b0[:, None] * a[:, 0] + b1[:, None] * a[:, 1] + b2[:, None] * a[:, 2]
            image[b][:, pix] = (m.astype(dtype)[:, None] * val).T
    return {"pix_to_face": p2f.reshape(B, S, S), "mask": mask.reshape(B, 1, S, S), "depth": depth.reshape(B, 1, S, S),
            "image": None if image is None else image.reshape(B, C, S, S), "bary": bary.reshape(B, S, S, 3)}


def compare(got, ref):
    """A result against the fp64 one: the share of pixels whose face differs per image (its maximum over the batch), and the largest
    absolute errors of depth and image over the pixels where the faces agree."""
    same = np.asarray(got["pix_to_face"]) == ref["pix_to_face"]
    out = {"differing": int((~same).reshape(same.shape[0], -1).sum(axis=1).max()), "pixels": int(same[0].size)}
    out["depth"] = float(np.abs(np.asarray(got["depth"], np.float64) - ref["depth"])[same[:, None]].max(initial=0.0))
    if ref["image"] is not None:
        C = ref["image"].shape[1]
        d = np.abs(np.asarray(got["image"], np.float64) - ref["image"])
        out["image"] = float(d[np.broadcast_to(same[:, None], d.shape)].max(initial=0.0)) if C else 0.0
    return out
