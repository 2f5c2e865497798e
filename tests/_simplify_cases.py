"""Meshes shared by tests/test_simplify_host.py and tests/test_gpu_simplify.py: the two quality fixtures (offset unit cube,
UV sphere) and the small shapes of the GPU cases."""
import numpy as np


def cube(q, offset=0.013):
    """The surface of the unit cube, `q` x `q` quads per side, welded (one vertex per lattice point of the boundary), every quad
    split in two triangles, outward orientation, shifted by `offset`.  Returns (verts float64 [V,3], faces int64 [F,3],
    on_edge bool [V]: at least two lattice coordinates in {0, q})."""
    ids = -np.ones((q + 1, q + 1, q + 1), dtype=np.int64)
    g = np.arange(q + 1)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    border = (X == 0) | (X == q) | (Y == 0) | (Y == q) | (Z == 0) | (Z == q)
    ids[border] = np.arange(border.sum())
    lattice = np.stack([X[border], Y[border], Z[border]], -1)
    faces = []
    i, j = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")
    i, j = i.reshape(-1), j.reshape(-1)
    for axis in range(3):
        for side in (0, q):
            def at(di, dj):
                c = [None, None, None]
                c[axis] = np.full_like(i, side)
                c[(axis + 1) % 3] = i + di
                c[(axis + 2) % 3] = j + dj
                return ids[c[0], c[1], c[2]]

            a, b, c, d = at(0, 0), at(1, 0), at(1, 1), at(0, 1)         # counter-clockwise seen from +axis
            t = np.concatenate([np.stack([a, b, c], -1), np.stack([a, c, d], -1)])
            faces.append(t if side == q else t[:, ::-1])
    on_edge = ((lattice == 0) | (lattice == q)).sum(1) >= 2
    return lattice / float(q) + offset, np.concatenate(faces).astype(np.int64), on_edge


def cube_edge_distance(p, offset=0.013):
    """Distance of every row of p to the nearest of the 12 edges of the unit cube shifted by `offset`."""
    p = np.asarray(p, dtype=np.float64) - offset
    best = np.full(len(p), np.inf)
    for axis in range(3):
        o1, o2 = (axis + 1) % 3, (axis + 2) % 3
        along = p[:, axis] - np.clip(p[:, axis], 0.0, 1.0)
        for s1 in (0.0, 1.0):
            for s2 in (0.0, 1.0):
                best = np.minimum(best, np.sqrt(along ** 2 + (p[:, o1] - s1) ** 2 + (p[:, o2] - s2) ** 2))
    return best


def uv_sphere(stacks, slices, radius=1.0):
    """UV sphere: `stacks` x `slices` segments, one vertex per pole, outward orientation."""
    th = np.pi * np.arange(1, stacks) / stacks
    ph = 2 * np.pi * np.arange(slices) / slices
    ring = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(slices))], -1)
    verts = np.concatenate([[[0, 0, 1.0]], ring.reshape(-1, 3), [[0, 0, -1.0]]]) * radius
    south = len(verts) - 1
    s = np.arange(slices)
    s1 = (s + 1) % slices
    faces = [np.stack([np.zeros(slices, dtype=np.int64), 1 + s, 1 + s1], -1)]
    for r in range(stacks - 2):
        a, b = 1 + r * slices, 1 + (r + 1) * slices
        faces.append(np.stack([a + s, b + s, b + s1], -1))
        faces.append(np.stack([a + s, b + s1, a + s1], -1))
    a = 1 + (stacks - 2) * slices
    faces.append(np.stack([np.full(slices, south), a + s1, a + s], -1))
    return verts, np.concatenate(faces).astype(np.int64)


def plane(q, z=0.25):
    """q x q quads of side 1 / q in the plane z = const: every cluster's quadric has rank 1."""
    g = np.arange(q + 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    verts = np.stack([X.reshape(-1) / q, Y.reshape(-1) / q, np.full(X.size, z)], -1)
    i, j = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")
    a = (i * (q + 1) + j).reshape(-1)
    b, c, d = a + (q + 1), a + (q + 1) + 1, a + 1
    return verts, np.concatenate([np.stack([a, b, c], -1), np.stack([a, c, d], -1)]).astype(np.int64)
