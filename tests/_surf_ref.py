"""numpy restatement of csrc/ncw_surf.hip (area weights, the search of the area table, the Philox4x32-10 stream and the
point formula) for tests/test_surf_host.py and tests/test_gpu_surf.py.  float64 throughout, products and sums rounded one by
one in the kernel's order."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
M32 = np.uint64(MASK)


def philox4x32_10(counter, key):
    """counter [n,4], key (k0, k1): uint32 words -> [n,4] uint32 (Salmon et al., SC'11)."""
    c = [np.asarray(counter, dtype=np.uint64)[:, j] & M32 for j in range(4)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, -1).astype(np.uint32)


def stream(i, seed, mode=0, n_total=1):
    """(u, r1, r2, xi) float64 of the sample indices i (ncw_surf_sample's rules)."""
    i = np.asarray(i, dtype=np.uint64)
    ctr = np.stack([i & M32, i >> np.uint64(32), np.zeros_like(i), np.zeros_like(i)], -1)
    w = philox4x32_10(ctr, (seed & MASK, (seed >> 32) & MASK)).astype(np.uint64)
    xi = (((w[:, 0] << np.uint64(32)) | w[:, 1]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    r1 = (w[:, 2].astype(np.float64) + 0.5) * 2.0 ** -32
    r2 = (w[:, 3].astype(np.float64) + 0.5) * 2.0 ** -32
    u = (i.astype(np.float64) + xi) / float(n_total) if mode == 1 else xi
    return u, r1, r2, xi


def weights(verts, faces, box=None):
    """0.5 |(B - A) x (C - A)|; 0 for an index outside [0, V), a non-finite area, a corner outside the closed box."""
    verts, faces = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    ok = ((faces >= 0) & (faces < len(verts))).all(-1)
    f = np.where(ok[:, None], faces, 0)
    A, B, Cc = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    with np.errstate(all="ignore"):
        u, v = B - A, Cc - A
        nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        area = 0.5 * np.sqrt(nx * nx + ny * ny + nz * nz)
        ok &= np.isfinite(area)
        if box is not None:
            lo, hi = np.asarray(box[0], dtype=np.float64), np.asarray(box[1], dtype=np.float64)
            for P in (A, B, Cc):
                ok &= ((P >= lo) & (P <= hi)).all(-1)
    return np.where(ok, area, 0.0)


def pick(cdf, x):
    """The smallest k with cdf[k] > x, else the smallest k with cdf[k] == cdf[-1]; NaN / negative x counts as 0."""
    cdf, x = np.asarray(cdf, dtype=np.float64), np.asarray(x, dtype=np.float64)
    x = np.where(x > 0, x, 0.0)
    k = np.searchsorted(cdf, x, "right")
    return np.where(k < len(cdf), k, np.searchsorted(cdf, cdf[-1], "left")).astype(np.int64)


def points(verts, faces, tri, r1, r2):
    """(1 - s) A + s (1 - r2) B + s r2 C, s = sqrt(r1)."""
    verts, f = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)[np.asarray(tri, dtype=np.int64)]
    s = np.sqrt(r1)
    wa, wb, wc = 1.0 - s, s * (1.0 - r2), s * r2
    return wa[:, None] * verts[f[:, 0]] + wb[:, None] * verts[f[:, 1]] + wc[:, None] * verts[f[:, 2]]
