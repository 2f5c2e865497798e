"""TEST INFRASTRUCTURE ONLY: a float64 numpy restatement of the depth rasterizer (csrc/ncw_raster.hip, reproj.render_depth)
with the same conventions -- OpenCV camera, pixel (r, c) samples (c + 0.5, r + 0.5), faces entirely in front of znear or
beyond zfar dropped, near-plane clipping into 1 or 2 sub-triangles, back faces (signed pixel area > 0) culled with
cull='back', zero-area triangles dropped, inclusive coverage (all edge functions >= 0), perspective-correct depth, samples
outside [znear, zfar] dropped, the nearest sample wins and equal depth goes to the smaller face.  Brute force over
pixels x triangles: small sizes only.

`rasterize` also says which pixels are ROBUST: the winner covers the sample with every edge at least `margin` pixels
away, and every other triangle that covers the sample within `margin` lies at least `gap` (relative) deeper.  There the
GPU must give the same face and a depth within fp32 rounding; elsewhere its face must be one of `near_cover[pixel]`."""
import numpy as np


def _project(p, K):
    return np.array([K[0, 0] * p[0] / p[2] + K[0, 2], K[1, 1] * p[1] / p[2] + K[1, 2]])


def sub_triangles(verts, faces, K, view, znear=0.05, zfar=100.0, cull="back"):
    """[(face, xy [3,2] pixel coordinates wound so that the covered side is >= 0, z [3])] after clipping and culling."""
    V = np.asarray(view, dtype=np.float64)[:3, :4]
    K = np.asarray(K, dtype=np.float64)
    cam = np.asarray(verts, dtype=np.float64) @ V[:, :3].T + V[:, 3]
    out = []
    for f, idx in enumerate(np.asarray(faces, dtype=np.int64)):
        p = cam[idx]
        inside = p[:, 2] >= znear
        if not inside.any() or (p[:, 2] > zfar).all():
            continue
        if inside.all():
            polys = [(p[0], p[1], p[2])]
        else:
            n_in = int(inside.sum())
            k = int(np.flatnonzero(inside)[0]) if n_in == 1 else int(np.flatnonzero(~inside)[0])
            a, b, c = p[k], p[(k + 1) % 3], p[(k + 2) % 3]

            def clip(o, i):
                t = (znear - o[2]) / (i[2] - o[2])
                q = o + t * (i - o)
                q[2] = znear
                return q

            if n_in == 1:
                polys = [(a, clip(b, a), clip(c, a))]
            else:
                ab, ca = clip(a, b), clip(a, c)
                polys = [(b, c, ca), (b, ca, ab)]
        for tri in polys:
            xy = np.stack([_project(q, K) for q in tri])
            z = np.array([q[2] for q in tri])
            area = (xy[1, 0] - xy[0, 0]) * (xy[2, 1] - xy[0, 1]) - (xy[1, 1] - xy[0, 1]) * (xy[2, 0] - xy[0, 0])
            if area == 0 or not np.isfinite(area):
                continue
            if area > 0:
                if cull == "back":
                    continue
            else:
                xy, z = xy[[0, 2, 1]], z[[0, 2, 1]]
            out.append((f, xy, z))
    return out


def rasterize(verts, faces, K, view, height, width, znear=0.05, zfar=100.0, cull="back", margin=1e-3, gap=1e-4):
    """-> dict(depth [H,W] float64 (0 = empty), face [H,W] int64 (-1), robust [H,W] bool, near_cover: list (per pixel, flat)
    of the set of faces covering the sample within `margin` pixels with a depth in [znear, zfar])."""
    H, W = int(height), int(width)
    px = (np.arange(W, dtype=np.float64) + 0.5)[None, :]
    py = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    best = np.full((H, W), np.inf)
    best_f = np.full((H, W), -1, dtype=np.int64)
    best_m = np.full((H, W), -np.inf)  # winner's smallest edge distance (pixels)
    near = [set() for _ in range(H * W)]
    hits = []  # (face, z, covered-within-margin mask)
    for f, xy, z in sub_triangles(verts, faces, K, view, znear, zfar, cull):
        e, dist = [], []
        for i in range(3):
            a, b = xy[(i + 1) % 3], xy[(i + 2) % 3]  # edge opposite vertex i
            ei = (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])
            e.append(ei)
            dist.append(ei / np.hypot(b[0] - a[0], b[1] - a[1]))
        s = e[0] + e[1] + e[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            zz = s / (e[0] / z[0] + e[1] / z[1] + e[2] / z[2])
        dmin = np.minimum(np.minimum(dist[0], dist[1]), dist[2])
        inz = (zz >= znear) & (zz <= zfar)
        cov = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0) & inz
        nc = (dmin >= -margin) & np.isfinite(zz) & (zz >= znear * (1 - 1e-6)) & (zz <= zfar * (1 + 1e-6))
        win = cov & ((zz < best) | ((zz == best) & (f < best_f)))
        best = np.where(win, zz, best)
        best_f = np.where(win, f, best_f)
        best_m = np.where(win, dmin, best_m)
        for q in np.flatnonzero(nc):
            near[q].add(f)
        hits.append((f, np.where(nc, zz, np.inf)))
    robust = (best_f >= 0) & (best_m > margin)
    for f, zz in hits:  # runner-up gap
        other = (best_f != f) & np.isfinite(zz)
        robust &= ~(other & (zz <= best * (1 + gap)))
    depth = np.where(best_f >= 0, best, 0.0)
    # a pixel with no winner is robust when nothing covers it within the margin
    empty = best_f < 0
    robust |= empty & np.array([len(s) == 0 for s in near]).reshape(H, W)
    return {"depth": depth, "face": best_f, "robust": robust, "near_cover": near}


def backproject(depth, K, pose):
    """utils/reproj_filter.py:133-152 in float64: points [N,3] of the pixels with depth > 0 (pixel order), integer pixel
    coordinates."""
    H, W = depth.shape
    r, c = np.nonzero(depth > 0)
    d = depth[r, c]
    cam = np.linalg.inv(np.asarray(K, dtype=np.float64)) @ np.stack([c, r, np.ones_like(c)]).astype(np.float64) * d
    pose = np.asarray(pose, dtype=np.float64)
    return (pose[:3, :3] @ cam + pose[:3, 3:4]).T


def nearest(ref, q, chunk=2048):
    """Brute-force 1-NN in float64: (distance [N], index [N], runner-up distance [N]); ties to the smaller index."""
    ref = np.asarray(ref, dtype=np.float64)
    d_out, i_out, d2_out = [], [], []
    for s in range(0, len(q), chunk):
        d = np.sqrt(((q[s:s + chunk, None, :] - ref[None]) ** 2).sum(-1))
        i = np.argmin(d, 1)
        srt = np.sort(d, 1)
        d_out.append(srt[:, 0])
        i_out.append(i)
        d2_out.append(srt[:, 1] if ref.shape[0] > 1 else np.full(len(i), np.inf))
    if not d_out:
        return np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0)
    return np.concatenate(d_out), np.concatenate(i_out), np.concatenate(d2_out)
