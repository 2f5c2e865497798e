"""float64 restatement of the voxel first-hit views (csrc/ncw_voxview.hip, reproj.VoxelCloud): the rays of
utils/kaolin_renderer.py:33-51 (`gen_rays`), the first crossing per ray from the brute-force slab oracle
(oracle.neuconw_oracle.ray_voxel_nuggets), the validity rule of generate_voxel.py:397-400 and the kept-vertex rule.

A float32 DDA and a float64 slab test may disagree on a voxel a ray merely grazes, so every ray is answered twice: counting
grazing contacts (margin -eps) and discounting them (+eps), eps = 2e-3 voxel (the band tests/test_gpu_voxel.py uses).  A pixel
is ROBUST when both margins give the same first voxel and neither entry depth lies within 1e-5 of the validity threshold
1e-4; a pixel that is not may come out as either margin's answer."""
import numpy as np
import torch

from oracle import neuconw_oracle as O

NEAR_MIN = 1e-4  # generate_voxel.py:397
NEAR_BAND = 1e-5
DEPTH_BIAS = 0.02  # kaolin_renderer.py:141


def look_at(C, T, scale=1.0):
    """4x4 camera -> world (OpenCV axes: z forward, y down; world z up) of a camera at C looking at T, rotation scaled."""
    C = np.asarray(C, dtype=np.float64)
    z = np.asarray(T, dtype=np.float64) - C
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 0.0, -1.0]), z)
    x /= np.linalg.norm(x)
    P = np.eye(4)
    P[:3, :3] = scale * np.stack([x, np.cross(z, x), z], 1)
    P[:3, 3] = C
    return P


def gen_rays(K, pose, height, width):
    """(d [H*W,3] = dir / |dir| + 1e-7, dir_norm [H*W]) of the pixels in row-major order: integer pixel coordinates,
    dir = pose[:3,:3] ((i - cx) / fx, (j - cy) / fy, 1) (kaolin_renderer.py:33-51, generate_voxel.py:332)."""
    K = np.asarray(K, dtype=np.float64)
    j, i = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    cam = np.stack([(i - K[0, 2]) / K[0, 0], (j - K[1, 2]) / K[1, 1], np.ones_like(i)], -1).reshape(-1, 3)
    dirs = cam @ np.asarray(pose, dtype=np.float64)[:3, :3].T
    dir_norm = np.linalg.norm(dirs, axis=-1)
    return dirs / dir_norm[:, None] + 1e-7, dir_norm


def origin_norm(pose, origin, scale):
    """generate_voxel.py:333, :345: the camera centre in the cube."""
    return (np.asarray(pose, dtype=np.float64)[:3, 3] + 1e-7 - np.asarray(origin, dtype=np.float64)) / float(scale)


def first_hits(on, d, idx, G, margin, chunk=1024):
    """Per ray: (linear index (x G + y) G + z of the first crossed voxel of idx [V,3] in depth order, -1 for none; its entry
    depth, clamped at 0)."""
    R = d.shape[0]
    vox = np.full(R, -1, dtype=np.int64)
    near = np.zeros(R)
    idx = torch.as_tensor(idx, dtype=torch.int64)
    lin = ((idx[:, 0] * G + idx[:, 1]) * G + idx[:, 2]).numpy()
    o = torch.as_tensor(on, dtype=torch.float64).reshape(1, 3)
    for s in range(0, R, chunk):
        dd = torch.as_tensor(d[s:s + chunk], dtype=torch.float64)
        r, v, dep = O.ray_voxel_nuggets(o.expand(dd.shape[0], 3), dd, idx, G, margin=margin)
        r, v, dep = r.numpy(), v.numpy(), dep.numpy()
        first = np.ones(r.shape[0], dtype=bool)
        first[1:] = r[1:] != r[:-1]  # ordered by ray, then by entry depth
        vox[s + r[first]] = lin[v[first]]
        near[s + r[first]] = dep[first, 0]
    return vox, near


def view(K, pose, height, width, idx, G, origin, scale):
    """The restated view.  dict of [H*W] arrays: for each margin m in ('lo', 'hi') (with / without grazing contacts)
    voxel_m (-1 where the ray is not valid) and depth_m (0 there); robust; valid (of the robust pixels' common answer)."""
    d, dir_norm = gen_rays(K, pose, height, width)
    on = origin_norm(pose, origin, scale)
    eps = 2e-3 * (2.0 / G)
    out = {}
    raw = {}
    for name, m in (("lo", -eps), ("hi", eps)):
        vox, near = first_hits(on, d, idx, G, m)
        raw[name] = (vox, near)
        ok = (vox >= 0) & (near > NEAR_MIN)
        out["voxel_" + name] = np.where(ok, vox, -1)
        out["depth_" + name] = np.where(ok, near * float(scale) / dir_norm + DEPTH_BIAS, 0.0)
    edge = [(v >= 0) & (np.abs(n - NEAR_MIN) <= NEAR_BAND) for v, n in raw.values()]
    out["robust"] = (raw["lo"][0] == raw["hi"][0]) & ~edge[0] & ~edge[1]
    out["valid"] = out["voxel_lo"] >= 0
    return out


def point_voxels(pn32, G):
    """ncw_voxel_build's arithmetic in f32 on normalised f32 points [N,3] (torch, CPU): linear voxel index, -1 for a point
    outside the cube or NaN."""
    p = torch.as_tensor(pn32, dtype=torch.float32).reshape(-1, 3)
    u = (p + 1.0) * (0.5 * float(G))  # f32 throughout
    inside = ((u >= 0) & (u < float(G))).all(-1)
    c = torch.where(inside[:, None], u, torch.zeros_like(u)).to(torch.int64)  # truncation, like (int)u
    return torch.where(inside, (c[:, 0] * G + c[:, 1]) * G + c[:, 2], torch.full_like(c[:, 0], -1)).numpy()


def normalise32(points, origin, scale):
    """reproj.VoxelCloud.normalise: float64, then cast."""
    return ((np.asarray(points, dtype=np.float64).reshape(-1, 3) - np.asarray(origin, dtype=np.float64)) / float(scale)).astype(np.float32)


def kept(point_vox, seen_voxels):
    """The kept-vertex rule: a vertex is kept iff the voxel that contains it (point_vox, -1 = none) was some pixel's first
    hit (seen_voxels: linear indices)."""
    seen = np.unique(np.asarray(seen_voxels, dtype=np.int64))
    return (point_vox >= 0) & np.isin(point_vox, seen[seen >= 0])


def unpack_bits(words, n_voxels=None):
    """Linear indices of the set bits of a bit grid (int32 / uint32 words, numpy)."""
    w = np.asarray(words).view(np.uint32)
    nz = np.flatnonzero(w)
    bits = (w[nz, None] >> np.arange(32, dtype=np.uint32)[None]) & 1
    r, b = np.nonzero(bits)
    return np.sort(nz[r].astype(np.int64) * 32 + b)
