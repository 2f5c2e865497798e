"""Restatements of csrc/ncw_gtreproj.hip in numpy, for the tests and for tests/golden/make_golden_gtreproj.py.  No GPU in here.

  pixel_nearest_f32 / reproj_errors_f32   the kernels' contracts in float32, every product and sum rounded in the order the
                                          header writes them: the kernels must agree with these BITWISE
  pixel_nearest_f64 / reproj_errors_f64   the same in float64, which arbitrates, with the band: the distance of every projection
                                          from the rounding boundaries of the query's pixel
"""
import numpy as np

NO_POINT = np.uint64(0xFFFFFFFFFFFFFFFF)
BAND = 1e-3      # px: no point of a band-free fixture projects this close to a boundary of a query pixel
MIN_DEPTH = 1e-6  # and none has |c_2| below this

f32 = np.float32


def _rows(table):
    w = np.asarray(table["w2c"], dtype=f32).reshape(-1, 3, 4)
    k = np.asarray(table["intr"], dtype=f32).reshape(-1, 4)
    xy = np.asarray(table["xy"], dtype=f32).reshape(-1, 2)
    return w, k, xy


def project_f32(w, k, xyz):
    """(u, v, c2) float32 [N] of one query (w [3,4], k = fx, fy, cx, cy) in the contract's order."""
    x, y, z = (np.ascontiguousarray(xyz[:, i], dtype=f32) for i in range(3))
    with np.errstate(all="ignore"):
        c = [((w[r, 0] * x + w[r, 1] * y) + w[r, 2] * z) + w[r, 3] for r in range(3)]
        u = (k[0] * c[0] + k[2] * c[2]) / c[2]
        v = (k[1] * c[1] + k[3] * c[2]) / c[2]
    assert u.dtype == f32 and c[2].dtype == f32
    return u, v, c[2]


def pixel_nearest_f32(table, xyz, p0=0, best=None):
    """ncw_pixel_nearest's contract: keys uint64 [Q].  table: the structured query table (gtreproj.query_table); xyz float32 [N,3].
    best: the keys so far (a later launch of a split cloud), or None for all-ones."""
    w, k, xy = _rows(table)
    xyz = np.asarray(xyz, dtype=f32).reshape(-1, 3)
    out = np.full(len(w), NO_POINT, dtype=np.uint64) if best is None else np.array(best, dtype=np.uint64)
    idx = (np.arange(len(xyz), dtype=np.uint64) + np.uint64(p0))
    for q in range(len(w)):
        if len(xyz) == 0:
            break
        u, v, c2 = project_f32(w[q], k[q], xyz)
        with np.errstate(invalid="ignore"):
            hit = (np.rint(u) == np.rint(xy[q, 0])) & (np.rint(v) == np.rint(xy[q, 1])) & (c2 >= 0)
        if hit.any():
            bits = (c2[hit] + f32(0.0)).view(np.uint32).astype(np.uint64)
            out[q] = min(out[q], ((bits << np.uint64(32)) | idx[hit]).min())
    return out


def pixel_nearest_f64(w2c, intr, xy, cloud):
    """The float64 answer: (index int64 [Q], -1 for none; band_hits int64 [Q] = the number of points that project within BAND of
    a rounding boundary of the query's pixel while within BAND of the pixel in the other coordinate, or have |c_2| < MIN_DEPTH;
    gap float64 [Q] = (second nearest hit's depth - nearest's) / nearest's, inf with fewer than two hits; second int64 [Q] = that
    second nearest hit, -1 without one).  The key-point is
    rounded as float32, as the kernel sees it."""
    w2c = np.asarray(w2c, dtype=np.float64).reshape(-1, 3, 4)
    intr = np.asarray(intr, dtype=np.float64).reshape(-1, 4)
    cloud = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    X = np.rint(np.asarray(xy, dtype=f32).reshape(-1, 2)).astype(np.float64)
    idx = np.full(len(w2c), -1, dtype=np.int64)
    band = np.zeros(len(w2c), dtype=np.int64)
    gap = np.full(len(w2c), np.inf)
    second = np.full(len(w2c), -1, dtype=np.int64)
    for q in range(len(w2c)):
        c = cloud @ w2c[q, :, :3].T + w2c[q, :, 3]
        with np.errstate(all="ignore"):
            u = (intr[q, 0] * c[:, 0] + intr[q, 2] * c[:, 2]) / c[:, 2]
            v = (intr[q, 1] * c[:, 1] + intr[q, 3] * c[:, 2]) / c[:, 2]
        du, dv = np.abs(u - X[q, 0]), np.abs(v - X[q, 1])
        hit = (du < 0.5) & (dv < 0.5) & (c[:, 2] > 0)
        near = (du < 0.5 + BAND) & (dv < 0.5 + BAND)
        band[q] = int((near & ((np.abs(du - 0.5) < BAND) | (np.abs(dv - 0.5) < BAND))).sum() + (np.abs(c[:, 2]) < MIN_DEPTH).sum())
        if hit.any():
            d = np.where(hit, c[:, 2], np.inf)
            idx[q] = int(np.argmin(d))
            if hit.sum() > 1:
                two = np.argsort(d, kind="stable")[:2]
                second[q] = int(two[1])
                gap[q] = (d[two[1]] - d[two[0]]) / d[two[0]]
    return idx, band, gap, second


def reproj_errors_f32(proj, xyz, cam_idx, pt_idx, xy):
    """ncw_reproj_errors' err in float32, the contract's order."""
    P = np.asarray(proj, dtype=f32).reshape(-1, 3, 4)[np.asarray(cam_idx)]
    p = np.asarray(xyz, dtype=f32).reshape(-1, 3)[np.asarray(pt_idx)]
    xy = np.asarray(xy, dtype=f32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        h = [((P[:, r, 0] * p[:, 0] + P[:, r, 1] * p[:, 1]) + P[:, r, 2] * p[:, 2]) + P[:, r, 3] for r in range(3)]
        dx, dy = h[0] / h[2] - xy[:, 0], h[1] / h[2] - xy[:, 1]
        e = np.sqrt(dx * dx + dy * dy)
    assert e.dtype == f32
    return e


def reproj_errors_f64(proj, xyz, cam_idx, pt_idx, xy):
    """The same on the same (float32-valued) inputs in float64."""
    P = np.asarray(proj, dtype=np.float64).reshape(-1, 3, 4)[np.asarray(cam_idx)]
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)[np.asarray(pt_idx)]
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    h = np.einsum("nij,nj->ni", P[:, :, :3], p) + P[:, :, 3]
    return np.hypot(h[:, 0] / h[:, 2] - xy[:, 0], h[:, 1] / h[:, 2] - xy[:, 1])


def seg_sums_f64(err, seg_start):
    """float64 sum of err per segment (np.sum's pairwise order: the comparison allows 1e-12 relative)."""
    return np.array([np.sum(np.asarray(err[a:b], dtype=np.float64)) for a, b in zip(seg_start[:-1], seg_start[1:])], dtype=np.float64)


def seg_sums_wave(err, seg_start):
    """The kernel's order exactly: lane l adds elements l, l + 64, .. in sequence, then the xor butterfly 32, 16, .. 1."""
    out = np.zeros(len(seg_start) - 1, dtype=np.float64)
    for s, (a, b) in enumerate(zip(seg_start[:-1], seg_start[1:])):
        part = np.zeros(64, dtype=np.float64)
        e = np.asarray(err[a:b], dtype=np.float64)
        for l in range(64):
            for x in e[l::64]:
                part[l] += x
        m = 32
        while m >= 1:
            part = part + part[np.arange(64) ^ m]
            m >>= 1
        out[s] = part[0]
    return out
