"""numpy restatement of ncw_imls_values (csrc/ncw_imls.hip; the contract is in include/neuconw_hip.h) and of the support rule of
cloudmesh.mesh_cloud, plus the clouds the IMLS tests share.

`imls_ref` is a brute force over ALL of pts_sorted, in its order: the float32 admission test d2 <= r2 with the 1-NN kernels'
d2 expression, then float64 sums taken sequentially over the admitted points.  numpy rounds every float32 / float64 operation
once, and np.add.accumulate adds strictly left to right, so the result is what the kernel must give bit for bit.  A point that
is not admitted enters the running sums as +0.0, which changes nothing: S and W start at +0.0, and a sum in round-to-nearest
is -0.0 only when both terms are, so neither is ever -0.0 and x + 0.0 == x holds for every value they take."""
import numpy as np

INF32 = np.float32(np.inf)
NAN32 = np.float32(np.nan)


def block_rows(blocks):
    """[nb*64,3] int64 lattice indices in the row order of the kernel: block-major, then local x, y, z with z fastest."""
    blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 3)
    a, c, e = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    loc = np.stack([a, c, e], -1).reshape(1, 64, 3)
    return (blocks[:, None, :] * 4 + loc).reshape(-1, 3)


def lattice_points(idx, lat_lo, voxel):
    """float32 [L,3]: x_a = lat_lo_a + float(i_a) * voxel, every operation in float32."""
    lo = np.asarray(lat_lo, dtype=np.float32)
    return lo[None, :] + np.asarray(idx).astype(np.float32) * np.float32(voxel)


def imls_ref(ps, ns, idx, lat_lo, voxel, side, radius, chunk_elems=1 << 22):
    """(value f32 [L], count int32 [L], d2min f32 [L]) of the lattice points idx [L,3] over ps [m,>=3] f32 (pts_sorted) and ns
    [m,>=3] f32 (its normals, same rows).  A lattice index outside [0, side) gives NaN / 0 / +inf."""
    ps = np.asarray(ps, dtype=np.float32)
    ns = np.asarray(ns, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 3)
    Ln, m = idx.shape[0], ps.shape[0]
    r2 = np.float32(radius) * np.float32(radius)
    inv_r2 = 1.0 / np.float64(r2)
    X = lattice_points(idx, lat_lo, voxel)
    inside = ((idx >= 0) & (idx < np.asarray(side, dtype=np.int64)[None, :])).all(1)
    value = np.full(Ln, NAN32, dtype=np.float32)
    count = np.zeros(Ln, dtype=np.int32)
    d2min = np.full(Ln, INF32, dtype=np.float32)
    n64 = ns[:, :3].astype(np.float64)
    step = max(1, chunk_elems // max(1, m))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for s in range(0, Ln, step):
            x = X[s:s + step]
            dx = ps[None, :, 0] - x[:, None, 0]
            dy = ps[None, :, 1] - x[:, None, 1]
            dz = ps[None, :, 2] - x[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz                        # float32, left to right
            adm = d2 <= r2                                            # false for a NaN
            t = 1.0 - d2.astype(np.float64) * inv_r2
            w = (t * t) * (t * t)
            g = -((dx.astype(np.float64) * n64[None, :, 0] + dy.astype(np.float64) * n64[None, :, 1])
                  + dz.astype(np.float64) * n64[None, :, 2])
            wg = np.where(adm, w * g, 0.0)
            w = np.where(adm, w, 0.0)
            S = np.add.accumulate(wg, axis=1)[:, -1]
            W = np.add.accumulate(w, axis=1)[:, -1]
            cnt = adm.sum(1).astype(np.int32)
            ok = (cnt > 0) & (W > 0.0) & inside[s:s + step]
            v = np.full(x.shape[0], NAN32, dtype=np.float32)
            v[ok] = (S[ok] / W[ok]).astype(np.float32)
            value[s:s + step] = v
            count[s:s + step] = np.where(inside[s:s + step], cnt, 0)
            dm = np.where(adm, d2, INF32).min(1)
            d2min[s:s + step] = np.where(inside[s:s + step], dm, INF32)
    return value, count, d2min


def support_rule(value, count, d2min, voxel, near, min_count):
    """The sparse points of cloudmesh.mesh_cloud: count >= min_count, a finite value, d2min <= float32(near * voxel)^2."""
    nv = np.float32(near * voxel)
    return (count >= min_count) & np.isfinite(value) & (d2min <= nv * nv)


# ---------------------------------------------------------------------------------------------------
# the shared clouds
# ---------------------------------------------------------------------------------------------------
def icosphere(levels):
    """(vertices [V,3] on the unit sphere, faces [F,3]) of an icosahedron subdivided `levels` times."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.stack(v), np.array(f, dtype=np.int64)


SPHERE_R = 1.0
SPHERE_VOXEL = 0.08     # about 1.6 x the mean spacing of the samples (sqrt(4 pi / 5120) = 0.0495)
SPHERE_SUPPORT = 3.0
SPHERE_NEAR = 2.0
SPHERE_MIN_COUNT = 3


def sphere_cloud():
    """Stratified samples of an icosphere: one sample per face of the level-3 icosphere's 4-way split (5120 faces), at the
    centroid, pushed out onto the unit sphere.  (points float64 [5120,3], normals float64 [5120,3] = the radial direction)."""
    v, f = icosphere(4)
    c = v[f].mean(1)
    n = c / np.linalg.norm(c, axis=1, keepdims=True)
    return n * SPHERE_R, n


def plane_cloud(n_side=24, spacing=0.05, normal=(0.3, -0.2, 0.9327379053088815), origin=(0.1, -0.2, 0.05)):
    """A square patch of n_side^2 points on the plane through `origin` with unit `normal`, on a regular net with a fixed
    sub-spacing jitter.  (points float64, normals float64, unit normal, origin)."""
    nrm = np.asarray(normal, dtype=np.float64)
    nrm = nrm / np.linalg.norm(nrm)
    a = np.cross(nrm, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    u, v = np.meshgrid(np.arange(n_side, dtype=np.float64), np.arange(n_side, dtype=np.float64), indexing="ij")
    rs = np.random.RandomState(7)
    u = (u + 0.3 * rs.rand(*u.shape) - n_side / 2.0) * spacing
    v = (v + 0.3 * rs.rand(*v.shape) - n_side / 2.0) * spacing
    P = np.asarray(origin, dtype=np.float64) + u.reshape(-1, 1) * a + v.reshape(-1, 1) * b
    return P, np.repeat(nrm[None, :], P.shape[0], 0), nrm, np.asarray(origin, dtype=np.float64)


def lattice_for(lo, hi, voxel, support):
    """cloudmesh.lattice_for restated: lat_lo = lo - (ceil(support) + 1) voxels, and the sides that reach as far beyond hi."""
    pad = int(np.ceil(support)) + 1
    lat_lo = [float(a) - pad * voxel for a in lo]
    side = [int(np.ceil((float(b) - float(a)) / voxel)) + 2 * pad + 1 for a, b in zip(lo, hi)]
    return lat_lo, side


_SPHERE = {}


def sphere_reference():
    """The restatement on the sphere fixture, computed once: every lattice point of the cloud's own lattice within
    SPHERE_NEAR + 1 voxels of the sphere.  dict: P, N (float64), ps, ns (float32 [m,4], cloud order), lat_lo (float32 values),
    side, idx [L,3], x (float32 lattice points), true = |x| - r (float64), value, count, d2min, sparse (the support rule)."""
    if _SPHERE:
        return _SPHERE
    P, N = sphere_cloud()
    lo, hi = P.min(0), P.max(0)
    centre = (lo + hi) / 2.0
    lat_lo, side = lattice_for(lo - centre, hi - centre, SPHERE_VOXEL, SPHERE_SUPPORT)
    lat_lo = [float(np.float32(v)) for v in lat_lo]
    p32 = (P - centre).astype(np.float32)
    ps = np.concatenate([p32, np.arange(P.shape[0], dtype=np.int32).view(np.float32)[:, None]], 1)
    ns = np.concatenate([N.astype(np.float32), np.zeros((P.shape[0], 1), np.float32)], 1)
    ii = np.stack(np.meshgrid(*[np.arange(s) for s in side], indexing="ij"), -1).reshape(-1, 3)
    x = lattice_points(ii, lat_lo, SPHERE_VOXEL)
    true = np.linalg.norm(x.astype(np.float64) + centre, axis=1) - SPHERE_R
    keep = np.abs(true) <= (SPHERE_NEAR + 1.0) * SPHERE_VOXEL
    ii, x, true = ii[keep], x[keep], true[keep]
    value, count, d2min = imls_ref(ps, ns, ii, lat_lo, SPHERE_VOXEL, side, SPHERE_SUPPORT * SPHERE_VOXEL)
    _SPHERE.update(P=P, N=N, centre=centre, ps=ps, ns=ns, lat_lo=lat_lo, side=side, idx=ii, x=x, true=true, value=value, count=count,
                   d2min=d2min, sparse=support_rule(value, count, d2min, SPHERE_VOXEL, SPHERE_NEAR, SPHERE_MIN_COUNT))
    return _SPHERE
