"""numpy restatement of the point-to-triangle distance contract of include/neuconw_hip.h (csrc/ncw_ptm.hip): the same rules
and the same arithmetic -- products and sums rounded one by one, in the kernel's order -- as a chunked brute force over all
(query, triangle) pairs, in float64 or, with dtype=np.longdouble, in extended precision on the same float64 inputs (the
coordinates are recentred in float64 first, as the kernel does).  No temporary holds more than CHUNK_PAIRS elements
(32 MB in float64, 64 MB in longdouble)."""
import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
CHUNK_PAIRS = 1 << 22


def _seg(P, A, B, d2m, M):
    """One segment term, endpoints in canonical order; updates (d2m, M) where it is strictly smaller."""
    (px, py, pz), (ax, ay, az), (bx, by, bz) = P, A, B
    sw = (bx < ax) | ((bx == ax) & ((by < ay) | ((by == ay) & (bz < az))))
    ux, uy, uz = np.where(sw, bx, ax), np.where(sw, by, ay), np.where(sw, bz, az)
    vx, vy, vz = np.where(sw, ax, bx), np.where(sw, ay, by), np.where(sw, az, bz)
    wx, wy, wz = vx - ux, vy - uy, vz - uz
    l = wx * wx + wy * wy + wz * wz
    with np.errstate(all="ignore"):
        s = ((px - ux) * wx + (py - uy) * wy + (pz - uz) * wz) / l
        s = np.where(l > 0, np.clip(s, 0, 1), 0)
        at_u, at_v = s <= 0, s >= 1
        cx = np.where(at_u, ux, np.where(at_v, vx, ux + s * wx))
        cy = np.where(at_u, uy, np.where(at_v, vy, uy + s * wy))
        cz = np.where(at_u, uz, np.where(at_v, vz, uz + s * wz))
        dx, dy, dz = px - cx, py - cy, pz - cz
        d2 = dx * dx + dy * dy + dz * dz
        upd = d2 < d2m
    d2m = np.where(upd, d2, d2m)
    if M is not None:
        M = (np.where(upd, cx, M[0]), np.where(upd, cy, M[1]), np.where(upd, cz, M[2]))
    return d2m, M


def tri_d2(P, A, B, C, closest=False):
    """d^2 of points P to triangles (A, B, C): each a tuple (x, y, z) of broadcastable arrays of ONE float dtype.  +inf where
    no term answers.  With `closest` also the closest point (x, y, z) of the first minimal term (face, AB, BC, CA)."""
    (px, py, pz), (ax, ay, az), (bx, by, bz), (cx, cy, cz) = P, A, B, C
    dt = np.result_type(px, ax)
    inf = np.array(np.inf, dtype=dt)
    e1x, e1y, e1z = bx - ax, by - ay, bz - az
    e2x, e2y, e2z = cx - ax, cy - ay, cz - az
    nx, ny, nz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
    nn = nx * nx + ny * ny + nz * nz
    pax, pay, paz = px - ax, py - ay, pz - az
    pbx, pby, pbz = px - bx, py - by, pz - bz
    pcx, pcy, pcz = px - cx, py - cy, pz - cz
    e3x, e3y, e3z = cx - bx, cy - by, cz - bz
    e4x, e4y, e4z = ax - cx, ay - cy, az - cz
    with np.errstate(all="ignore"):
        f1 = (e1y * paz - e1z * pay) * nx + (e1z * pax - e1x * paz) * ny + (e1x * pay - e1y * pax) * nz
        f2 = (e3y * pbz - e3z * pby) * nx + (e3z * pbx - e3x * pbz) * ny + (e3x * pby - e3y * pbx) * nz
        f3 = (e4y * pcz - e4z * pcy) * nx + (e4z * pcx - e4x * pcz) * ny + (e4x * pcy - e4y * pcx) * nz
        face = (nn > 0) & np.isfinite(nn) & (f1 >= 0) & (f2 >= 0) & (f3 >= 0)
        tt = nx * pax + ny * pay + nz * paz
        d2f = tt * tt / nn
        face = face & (d2f < inf)
        d2m = np.where(face, d2f, inf)
        M = None
        if closest:
            k = tt / nn
            nan = np.array(np.nan, dtype=dt)
            M = (np.where(face, px - k * nx, nan), np.where(face, py - k * ny, nan), np.where(face, pz - k * nz, nan))
    del f1, f2, f3, tt
    d2m, M = _seg(P, A, B, d2m, M)
    d2m, M = _seg(P, B, C, d2m, M)
    d2m, M = _seg(P, C, A, d2m, M)
    return (d2m, M) if closest else d2m


def pack(verts, faces, centre, box=None, dtype=np.float64):
    """(tri [F,9] of `dtype`: the corners recentred in float64, zero rows for invalid triangles; valid [F] bool): the
    validity rule of the contract -- indices in [0, V), nine finite coordinates, all corners inside the closed box."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    ok = ((faces >= 0) & (faces < verts.shape[0])).all(1)
    f = np.where(ok[:, None], faces, 0)
    c = verts[f] if verts.shape[0] else np.zeros((faces.shape[0], 3, 3))  # [F,3,3]
    ok &= np.isfinite(c).all((1, 2))
    if box is not None:
        lo, hi = np.asarray(box[0], dtype=np.float64), np.asarray(box[1], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            ok &= ((c >= lo) & (c <= hi)).all((1, 2))
    with np.errstate(invalid="ignore"):
        t = c - np.asarray(centre, dtype=np.float64)
    ok &= np.isfinite(t).all((1, 2))
    t = np.where(ok[:, None, None], t, 0.0).reshape(-1, 9)
    return t.astype(dtype), ok


def _cols(a):
    return a[..., 0], a[..., 1], a[..., 2]


def mesh_ref(verts, faces, query, centre, box=None, dtype=np.float64, chunk_pairs=CHUNK_PAIRS):
    """Brute force over all pairs.  Returns a dict: d2 [N] (dtype), dist [N] = sqrt(d2), idx [N] int64 = the FIRST argmin over
    the valid triangles, tie [N] bool (more than one valid triangle at exactly the minimal d^2), next [N] = the smallest
    distance strictly above the minimum (inf if none), closest [N,3] in the caller's coordinates (float64 centre added
    back), valid [F].  ValueError when no triangle is valid."""
    tri, ok = pack(verts, faces, centre, box, dtype)
    if not ok.any():
        raise ValueError("no valid triangle")
    q = (np.asarray(query, dtype=np.float64).reshape(-1, 3) - np.asarray(centre, dtype=np.float64)).astype(dtype)
    n, F = q.shape[0], tri.shape[0]
    A, B, C = (tuple(tri[None, :, 3 * k + a] for a in range(3)) for k in range(3))
    out = dict(d2=np.empty(n, dtype), idx=np.empty(n, np.int64), tie=np.empty(n, bool), next=np.empty(n, dtype),
               closest=np.empty((n, 3), dtype), valid=ok)
    step = max(1, chunk_pairs // max(F, 1))
    inf = np.array(np.inf, dtype=dtype)
    for i0 in range(0, n, step):
        qc = q[i0:i0 + step]
        P = tuple(qc[:, a, None] for a in range(3))
        d2 = np.where(ok[None, :], tri_d2(P, A, B, C), inf)  # [nq, F]
        idx = d2.argmin(1)  # numpy: the first minimal entry
        m = d2[np.arange(qc.shape[0]), idx]
        out["d2"][i0:i0 + step], out["idx"][i0:i0 + step] = m, idx
        out["tie"][i0:i0 + step] = (d2 == m[:, None]).sum(1) > 1
        out["next"][i0:i0 + step] = np.sqrt(np.where(d2 > m[:, None], d2, inf).min(1))
        del d2
        t = tri[idx]
        _, M = tri_d2(_cols(qc), _cols(t[:, 0:3]), _cols(t[:, 3:6]), _cols(t[:, 6:9]), closest=True)
        out["closest"][i0:i0 + step] = np.stack(M, -1)
    out["dist"] = np.sqrt(out["d2"])
    out["closest"] = out["closest"] + np.asarray(centre, dtype=np.float64).astype(dtype)
    return out


def pair_dist(verts, faces, query, idx, centre, dtype=np.float64):
    """Reference distance of query i to triangle idx[i] (no validity test: the caller checks that separately)."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(centre, dtype=np.float64)
    t = (verts[np.asarray(faces).reshape(-1, 3)[np.asarray(idx)]] - c).astype(dtype)  # [N,3,3]
    q = (np.asarray(query, dtype=np.float64).reshape(-1, 3) - c).astype(dtype)
    return np.sqrt(tri_d2(_cols(q), _cols(t[:, 0]), _cols(t[:, 1]), _cols(t[:, 2])))


def coord_scale(verts, query, centre):
    """C of the bounds: the largest |recentred coordinate| over the finite vertices and the queries."""
    c = np.asarray(centre, dtype=np.float64)
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    q = np.asarray(query, dtype=np.float64).reshape(-1, 3)
    return float(max(np.abs(v - c).max() if v.size else 0.0, np.abs(q - c).max() if q.size else 0.0))


def centre_of(verts, query):
    """evalmesh.ptm_centre in numpy: the centre of the common box of the finite vertices and queries."""
    sets = [np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in (verts, query)]
    sets = [a[np.isfinite(a).all(1)] for a in sets]
    sets = [a for a in sets if a.shape[0]]
    lo = np.min([a.min(0) for a in sets], 0)
    hi = np.max([a.max(0) for a in sets], 0)
    return (lo + hi) / 2.0


# ---------------------------------------------------------------------------------------------------
# the meshes and queries of the cases
# ---------------------------------------------------------------------------------------------------
def height_field(n=24, seed=1, jitter=0.25, quantum=None):
    """A jittered n x n height field over [0, 1]^2: (verts float64 [n*n,3], faces int64 [2 (n-1)^2, 3]); 1058 triangles at
    n = 24.  `quantum` rounds the coordinates to multiples of it (so that adding an offset stays exact)."""
    rng = np.random.RandomState(seed)
    g = np.arange(n) / (n - 1.0)
    x, y = np.meshgrid(g, g, indexing="ij")
    x = x + rng.uniform(-jitter, jitter, x.shape) / (n - 1.0)
    y = y + rng.uniform(-jitter, jitter, y.shape) / (n - 1.0)
    z = 0.15 * np.sin(5 * x) * np.cos(4 * y) + rng.uniform(-0.002, 0.002, x.shape)
    v = np.stack([x, y, z], -1).reshape(-1, 3)
    if quantum:
        v = np.round(v / quantum) * quantum
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1)
    f = np.concatenate([np.stack([a, a + n, a + 1], -1), np.stack([a + 1, a + n, a + n + 1], -1)])
    return v, f.astype(np.int64)


def min_angle_deg(verts, faces):
    t = verts[faces]
    out = []
    for k in range(3):
        u, w = t[:, (k + 1) % 3] - t[:, k], t[:, (k + 2) % 3] - t[:, k]
        c = (u * w).sum(1) / np.sqrt((u * u).sum(1) * (w * w).sum(1))
        out.append(np.degrees(np.arccos(np.clip(c, -1, 1))))
    return float(np.min(out))


def interior_queries(verts, faces, n, seed=1, lift=0.01):
    """n points over triangle interiors (barycentric weights >= 0.2), lifted +-lift along the normal; returns (points,
    source triangle)."""
    rng = np.random.RandomState(seed)
    src = rng.randint(0, faces.shape[0], n)
    w = rng.dirichlet([1.0, 1.0, 1.0], n) * 0.4 + 0.2
    t = verts[faces[src]]
    p = (w[:, :, None] * t).sum(1)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return p + nrm * (lift * rng.choice([-1.0, 1.0], n))[:, None], src


def uniform_queries(verts, n, seed=2, pad=0.2):
    rng = np.random.RandomState(seed)
    lo, hi = verts.min(0) - pad, verts.max(0) + pad
    return lo + rng.rand(n, 3) * (hi - lo)
