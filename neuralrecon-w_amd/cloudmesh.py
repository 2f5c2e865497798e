"""Mesh an oriented point cloud on the GPU: implicit-moving-least-squares (IMLS) values on a sparse lattice around the cloud
(csrc/ncw_imls.hip, `imls_values`), then the sparse marching cubes of `mesh.isosurface_sparse` on the supported lattice points.

    f(x) = sum_i w_i n_i.(x - p_i) / sum_i w_i,   w_i = (1 - |x - p_i|^2 / R^2)^4 for |x - p_i| <= R = support * voxel

is the signed distance of x to the planes through its neighbours, blended; the surface is f = 0 and the normals point to f > 0.
The reference has no such step (it only ever meshes its own network); what users know it from is open3d's
`create_from_point_cloud_*`.  The weight, the support rule and the defaults are THIS PROJECT'S choice: no parity with open3d's
Poisson or ball pivoting, nor with any published IMLS code, is claimed or measured.

A lattice point is a sparse point -- it takes part in marching cubes -- iff
    count >= min_count   and   value is finite   and   d2min <= float32(near * voxel)^2
(count = the cloud points within R, d2min = the squared distance to the nearest of them).  The rule does not depend on how the
candidate lattice points are enumerated: any superset of the points that can pass it gives the same mesh.  A cube with an
unsupported corner yields no triangle, so a hole in the cloud wider than about 2 near voxels stays a hole in the mesh.

Limitations: two sheets closer than support * voxel with opposite normals mix (their planes are blended); the input normals must
be consistently oriented -- nothing here propagates orientation.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import evalmesh, mesh, meshops
from . import lib as L

MAX_SIDE = mesh.SPARSE_MC_MAX_DIM  # 16384 lattice points per axis
MAX_SPARSE = 2 ** 31 - 1
BLOCK_CHUNK = 1 << 15              # blocks of 64 lattice points per launch of mesh_cloud: 2 M rows, 24 MB of planes


def _need_gpu(what, *tensors):
    for t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise L.NeuconwHipError("cloudmesh.%s: the input is not on a GPU; there is no CPU fallback" % what)


def gather_normals(grid, normals):
    """nrm_sorted [m,4] float32: row i holds the normal of grid.pts[i] (through the index in its .w), .w = 0."""
    idx = grid.pts[:, 3].contiguous().view(torch.int32).long()
    out = torch.zeros(grid.m, 4, dtype=torch.float32, device=grid.dev)
    out[:, :3] = normals.to(torch.float32)[idx]
    return out


@torch.no_grad()
def imls_values(grid, normals, blocks, lat_lo, voxel, side, radius, stats=None, sorted_normals=None):
    """One launch of `ncw_imls_values` (include/neuconw_hip.h states the contract): grid = a built `evalmesh.NNGrid` over the
    cloud, normals [m,3] in the cloud's own order (or sorted_normals = `gather_normals(grid, normals)`, if the caller kept
    it), blocks [nb,3] int32 coordinates of 4 x 4 x 4 blocks of lattice points, the lattice x = lat_lo + index * voxel with
    `side` points per axis, radius = the support.  Returns (value f32, count int32, d2min f32), each [nb * 64]: row
    b * 64 + ((a * 4 + c) * 4 + e) is lattice point (4 bx + a, 4 by + c, 4 bz + e).  stats (dict) gets `staged` (points staged
    through LDS, summed over the blocks).  NeuconwHipError for CPU tensors and for the arguments the entry refuses."""
    _need_gpu("imls_values", grid.pts, normals, blocks, sorted_normals)
    dev = grid.dev
    if sorted_normals is None:
        if normals.shape != (grid.m, 3):
            raise ValueError("cloudmesh.imls_values: normals must be [%d,3]" % grid.m)
        sorted_normals = gather_normals(grid, normals)
    blocks = blocks.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    nb = int(blocks.shape[0])
    value = torch.empty(nb * 64, dtype=torch.float32, device=dev)
    count = torch.empty(nb * 64, dtype=torch.int32, device=dev)
    d2min = torch.empty(nb * 64, dtype=torch.float32, device=dev)
    work = torch.empty(nb, dtype=torch.int32, device=dev) if stats is not None else None
    lo3 = (C.c_float * 3)(*[float(v) for v in lat_lo])
    side3 = (C.c_int32 * 3)(*[int(v) for v in side])
    if nb:
        L.check(L.get_lib().ncw_imls_values(L.ptr(grid.pts), L.ptr(sorted_normals.contiguous()), L.ptr(grid.range), grid.m,
                                            C.byref(grid.cgrid), float(grid.margin), L.ptr(blocks), nb, lo3, float(voxel), side3,
                                            float(radius), L.ptr(value), L.ptr(count), L.ptr(d2min), L.ptr(work),
                                            L.stream_ptr(dev)), "ncw_imls_values")
    if stats is not None:
        stats["staged"] = stats.get("staged", 0) + (int(work.long().sum()) if nb else 0)
    return value, count, d2min


def lattice_for(lo, hi, voxel, support):
    """(lat_lo [3] float, side [3] int) of the lattice over the box lo .. hi: lat_lo = lo - (ceil(support) + 1) voxels, and as
    many points as reach hi + (ceil(support) + 1) voxels."""
    pad = int(math.ceil(support)) + 1
    lat_lo = [float(a) - pad * voxel for a in lo]
    side = [int(math.ceil((float(b) - float(a)) / voxel)) + 2 * pad + 1 for a, b in zip(lo, hi)]
    return lat_lo, side


def candidate_blocks(p32, lat_lo, voxel, side, near):
    """[nb,3] int32, ascending: the 4^3 blocks of lattice points that hold a cloud point, dilated by ceil((near + 0.01) / 4)
    blocks (the 0.01 voxel covers the float32 rounding of a point's lattice index, at most 16384 * 2^-23 voxel), inside the
    lattice.  A superset of the blocks with a lattice point within near voxels of the cloud."""
    dev = p32.device
    lo = torch.tensor(lat_lo, dtype=torch.float32, device=dev)
    li = torch.floor((p32 - lo) / float(voxel))
    sd = torch.tensor(side, dtype=torch.float32, device=dev)
    ok = ((li >= 0) & (li < sd)).all(-1)  # false for a NaN
    b = (li[ok].long() // 4)
    nbs = [(s + 3) // 4 for s in side]
    NB = max(nbs)
    keys = torch.unique((b[:, 0] * NB + b[:, 1]) * NB + b[:, 2])
    d = int(math.ceil((float(near) + 0.01) / 4.0))
    r = torch.arange(-d, d + 1, device=dev, dtype=torch.int64)
    off = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    lim = torch.tensor(nbs, dtype=torch.int64, device=dev)
    out = []
    step = max(1, (1 << 22) // off.shape[0])  # bounded temporaries: 4 M keys at a time
    for s in range(0, keys.shape[0], step):
        k = keys[s:s + step]
        c = torch.stack((k // (NB * NB), (k // NB) % NB, k % NB), -1)[:, None, :] + off[None, :, :]
        c = c.reshape(-1, 3)
        c = c[((c >= 0) & (c < lim)).all(-1)]
        out.append(torch.unique((c[:, 0] * NB + c[:, 1]) * NB + c[:, 2]))
    if not out:
        return torch.zeros(0, 3, dtype=torch.int32, device=dev)
    k = torch.unique(torch.cat(out))
    return torch.stack((k // (NB * NB), (k // NB) % NB, k % NB), -1).to(torch.int32).contiguous()


def _block_points(blocks):
    """[nb*64,3] int64 lattice indices in the row order of `imls_values`."""
    dev = blocks.device
    r = torch.arange(4, device=dev, dtype=torch.int64)
    loc = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(1, 64, 3)
    return (blocks.long()[:, None, :] * 4 + loc).reshape(-1, 3)


def _check_args(points, normals, voxel, support, near, min_count):
    if normals is None:
        raise ValueError("cloudmesh.mesh_cloud: the cloud has no normals (cloudops.estimate_normals gives it some)")
    if points.dim() != 2 or points.shape[1] != 3 or tuple(normals.shape) != tuple(points.shape):
        raise ValueError("cloudmesh.mesh_cloud: points and normals must both be [N,3]")
    if points.shape[0] < 1:
        raise ValueError("cloudmesh.mesh_cloud: the cloud is empty")
    if not (float(voxel) > 0 and math.isfinite(float(voxel))):
        raise ValueError("cloudmesh.mesh_cloud: voxel must be > 0, got %r" % (voxel,))
    if not float(near) >= math.sqrt(3.0):
        raise ValueError("cloudmesh.mesh_cloud: near = %r < sqrt(3): a cube the surface crosses could lack a corner" % (near,))
    if not (float(support) >= float(near) and math.isfinite(float(support))):
        raise ValueError("cloudmesh.mesh_cloud: support = %r must be finite and at least near = %r" % (support, near))
    if int(min_count) < 1:
        raise ValueError("cloudmesh.mesh_cloud: min_count must be at least 1")


@torch.no_grad()
def mesh_cloud(points, normals, voxel, support=3.0, near=2.0, min_count=3, box=None, colors=None, min_component_faces=0,
               stats=None):
    """The surface of an oriented cloud as a triangle mesh.  points [N,3], normals [N,3] (unit, consistently oriented; the
    mesh's face normals follow them), colors [N,...] or None: GPU tensors.  voxel: the lattice spacing; support, near in voxels,
    min_count: see the module text.  box [[x0, y0, z0], [x1, y1, z1]]: the lattice covers this box instead of the cloud's own (the
    surface is only extracted where lattice points exist).  Returns (verts float64 [V,3] in the cloud's coordinates, faces
    [F,3] integer) and, with colors, the colour of every vertex's nearest cloud point.  min_component_faces > 0: components
    with fewer faces are dropped (`meshops.clean`).  stats (dict): points, candidates, sparse, staged, vertices, faces.
    ValueError, before anything is launched: missing, non-finite or non-unit (beyond 1e-3) normals, non-finite points,
    near < sqrt(3), support < near, a lattice side above 16384, more than 2^31 - 1 sparse points.  NeuconwHipError for CPU
    tensors: there is no fallback."""
    _check_args(points, normals, voxel, support, near, min_count)
    voxel, support, near = float(voxel), float(support), float(near)
    dev = points.device
    p64, n32 = points.double(), normals.float()
    if not bool(torch.isfinite(p64).all()):
        raise ValueError("cloudmesh.mesh_cloud: the points are not all finite")
    nlen = n32.double().norm(dim=-1)
    if not bool(torch.isfinite(n32).all()) or not bool(((nlen - 1.0).abs() <= 1e-3).all()):
        raise ValueError("cloudmesh.mesh_cloud: the normals are not all finite and of unit length (within 1e-3)")
    if colors is not None and colors.shape[0] != points.shape[0]:
        raise ValueError("cloudmesh.mesh_cloud: one colour per point")
    if box is None:
        blo, bhi = p64.amin(0).tolist(), p64.amax(0).tolist()
    else:
        blo, bhi = [float(v) for v in box[0]][:3], [float(v) for v in box[1]][:3]
        if len(blo) != 3 or len(bhi) != 3 or not all(math.isfinite(a) and math.isfinite(b) and b >= a for a, b in zip(blo, bhi)):
            raise ValueError("cloudmesh.mesh_cloud: box must be [[x0, y0, z0], [x1, y1, z1]] with finite lo <= hi")
    centre = [(a + b) / 2.0 for a, b in zip(blo, bhi)]
    lat_lo, side = lattice_for([a - c for a, c in zip(blo, centre)], [b - c for b, c in zip(bhi, centre)], voxel, support)
    if max(side) > MAX_SIDE:
        raise ValueError("cloudmesh.mesh_cloud: a lattice of %s points per axis, more than %d: use a larger voxel" % (side, MAX_SIDE))
    _need_gpu("mesh_cloud", points, normals, colors)  # every ValueError above comes first, whatever the device
    lat_lo = [float(np.float32(v)) for v in lat_lo]  # the float32 values the kernel adds to
    c64 = torch.tensor(centre, dtype=torch.float64, device=dev)
    p32 = (p64 - c64).float().contiguous()
    cmax = max(float(p32.abs().amax()), max(abs(v) for v in lat_lo), max(abs(l + s * voxel) for l, s in zip(lat_lo, side)))
    grid = evalmesh.NNGrid(p32, cmax)
    nrm_sorted = gather_normals(grid, n32)
    blocks = candidate_blocks(p32, lat_lo, voxel, side, near)
    near2 = float(np.float32(near * voxel) * np.float32(near * voxel))
    G = max(side)
    st = {} if stats is not None else None
    keys, vals = [], []
    n_sparse = 0
    for s in range(0, blocks.shape[0], BLOCK_CHUNK):
        bl = blocks[s:s + BLOCK_CHUNK]
        value, count, d2min = imls_values(grid, None, bl, lat_lo, voxel, side, support * voxel, stats=st, sorted_normals=nrm_sorted)
        sel = torch.nonzero((count >= int(min_count)) & torch.isfinite(value) & (d2min <= near2)).reshape(-1)
        li = _block_points(bl)[sel]
        keys.append((li[:, 0] * G + li[:, 1]) * G + li[:, 2])
        vals.append(value[sel])
        n_sparse += int(sel.shape[0])
        if n_sparse > MAX_SPARSE:
            raise ValueError("cloudmesh.mesh_cloud: more than 2^31 - 1 sparse lattice points: use a larger voxel")
    if keys:
        keys, order = torch.sort(torch.cat(keys))  # the keys are distinct: blocks and their points are
        vals = torch.cat(vals)[order].contiguous()
    else:
        keys, vals = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float32, device=dev)
    bricks = torch.stack((keys // (G * G), (keys // G) % G, keys % G), -1).to(torch.int32).contiguous()
    verts_i, faces = mesh.isosurface_sparse(bricks, 1, vals, 0.0, G=G)
    lo64 = torch.tensor(lat_lo, dtype=torch.float64, device=dev)
    verts = c64 + lo64 + voxel * verts_i.double()
    vcol = None
    if colors is not None:
        if verts.shape[0]:
            _, idx = grid.query((verts - c64).float().contiguous())
            vcol = colors[idx]
        else:
            vcol = colors[:0]
    if int(min_component_faces) > 0 and faces.shape[0]:
        verts, faces, vcol, _ = meshops.clean(verts, faces, vcol, min_component_faces=int(min_component_faces))
    if stats is not None:
        stats.update(points=int(points.shape[0]), candidates=int(blocks.shape[0]) * 64, sparse=n_sparse, staged=st.get("staged", 0),
                     vertices=int(verts.shape[0]), faces=int(faces.shape[0]), side=list(side))
    return (verts, faces) if colors is None else (verts, faces, vcol)
