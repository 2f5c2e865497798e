"""Mesh extraction on the GPU: the steps after the SDF grid sweep of config 5.

Reference: utils/visualization.py:37-159 `extract_mesh` (rank-0 CPU `skimage.measure.marching_cubes`, vertex
colours through `renderer.rgb`, trimesh export) driven by tools/extract_mesh.py:104-168.  Here the SDF grid never
leaves the GPU: `grid.sdf_grid` -> `isosurface` (marching cubes, csrc/ncw_mesh.hip + the generated case tables of
mc_tables.py) -> vertex welding with torch.unique -> optional colour pass -> binary PLY.  The VERTEX SET is the reference's
(one linear zero crossing per sign-changing grid edge of the enabled cubes: tests/test_gpu_mesh.py checks it edge by
edge); skimage's triangulation of the ambiguous cube configurations (Lewiner) is not reproducible without skimage, which
is neither in the reference tree nor installable: **triangulation parity is unpinned** there.  Also kept: the `mask`
semantics, the sparse mode (`gen_grid_spc`, tools/extract_mesh.py:60-102: SDF only inside the occupied octree voxels, cubes with
all 8 corners evaluated) and the coordinate chain `verts * voxel_size + vol_origin`, `* scene_radius + scene_origin` (:116-117).
Normals / winding point towards increasing SDF (outwards).
Not in the reference: `isosurface_sparse` (csrc/ncw_mc_sparse.hip) runs the same marching cubes on the sparse mode's values as
they are blocked by octree voxel, without the [dim]^3 volume and mask -- the same mesh bit for bit, at lattices the dense path
cannot hold (`extract_mesh(sparse_mc=...)`).
"""
import numpy as np
import torch

from . import grid as _grid
from . import lib as L
from . import ply


_TABLES = {}


def _mc_tables(dev):
    """The generated marching-cubes case tables (mc_tables.py) on `dev`."""
    t = _TABLES.get(str(dev))
    if t is None:
        from . import mc_tables

        tri, ntri, edges = mc_tables.tables()
        t = _TABLES[str(dev)] = (torch.from_numpy(tri).to(dev).contiguous(), torch.from_numpy(ntri).to(dev).contiguous(),
                                 torch.from_numpy(edges).to(dev).contiguous())
    return t


@torch.no_grad()
def isosurface(sdf, level=0.0, mask=None):
    """sdf [Dx,Dy,Dz] float32 on the GPU (x slowest) -> (verts [V,3] float32 in grid-index coordinates,
    faces [F,3] int64).  mask: bool [Dx,Dy,Dz] or None -- cube (i,j,k) is used iff mask[i+1,j+1,k+1]."""
    if not sdf.is_cuda:
        raise L.NeuconwHipError("mesh.isosurface: the SDF grid is not on a GPU; there is no CPU fallback")
    sdf = sdf.contiguous().float()
    Dx, Dy, Dz = sdf.shape
    dev = sdf.device
    m8 = None if mask is None else mask.to(device=dev, dtype=torch.uint8).contiguous()
    ncubes = (Dx - 1) * (Dy - 1) * (Dz - 1)
    counts = torch.empty(ncubes, dtype=torch.int32, device=dev)
    tri, ntri, edges = _mc_tables(dev)
    lib = L.get_lib()
    L.check(lib.ncw_mc_count(L.ptr(sdf), L.ptr(m8), Dx, Dy, Dz, float(level), L.ptr(ntri), L.ptr(counts), L.stream_ptr(dev)),
            "ncw_mc_count")
    incl = torch.cumsum(counts, 0, dtype=torch.int64)
    T = int(incl[-1])  # one device->host read: the mesh size
    if T == 0:
        return torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev)
    offsets = (incl - counts).contiguous()
    pos = torch.empty(T, 3, 3, device=dev, dtype=torch.float32)
    key = torch.empty(T, 3, device=dev, dtype=torch.int64)
    L.check(lib.ncw_mc_emit(L.ptr(sdf), L.ptr(m8), Dx, Dy, Dz, float(level), L.ptr(tri), L.ptr(ntri), L.ptr(edges),
                            L.ptr(offsets), L.ptr(pos), L.ptr(key), L.stream_ptr(dev)), "ncw_mc_emit")
    uniq, inv = torch.unique(key.reshape(-1), return_inverse=True)  # weld: one vertex per grid edge
    verts = torch.empty(uniq.shape[0], 3, device=dev, dtype=torch.float32)
    verts[inv] = pos.reshape(-1, 3)  # all copies of a vertex are bit-identical (interpolated lo -> hi)
    faces = inv.reshape(T, 3)
    ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    return verts, faces[ok]  # a value exactly on the level collapses an edge: drop the degenerate faces


DENSE_MC_MAX_DIM = 1024  # the reference's level 10: the largest lattice the dense path (sparse_volume + isosurface) is used on
SPARSE_MC_MAX_DIM = 16384  # G * up of isosurface_sparse


def _check_bricks(bricks, up, values, G):
    """The refusals of isosurface_sparse (ValueError, before anything is launched on the values).  Returns (n, K)."""
    up, G = int(up), int(G)
    if up < 1 or up > 32 or up & (up - 1):
        raise ValueError("isosurface_sparse: up = %d is not a power of two in 1..32" % up)
    if bricks.dim() != 2 or bricks.shape[1] != 3 or bricks.dtype.is_floating_point or bricks.dtype == torch.bool:
        raise ValueError("isosurface_sparse: bricks must be [n,3] integer coarse-voxel indices")
    n = bricks.shape[0]
    K = n * up ** 3
    if values.numel() != K:
        raise ValueError("isosurface_sparse: %d values for %d bricks of %d^3 sub-voxels (%d expected)" % (values.numel(), n, up, K))
    if K > 2 ** 31 - 1:
        raise ValueError("isosurface_sparse: K = %d sparse points, more than 2^31 - 1" % K)
    if G < 1 or G * up > SPARSE_MC_MAX_DIM:
        raise ValueError("isosurface_sparse: lattice side G * up = %d * %d outside 1..%d" % (G, up, SPARSE_MC_MAX_DIM))
    if n:
        b = bricks.long()
        if bool((b < 0).any()) or bool((b >= G).any()):
            raise ValueError("isosurface_sparse: bricks outside [0, %d)" % G)
        key = (b[:, 0] * G + b[:, 1]) * G + b[:, 2]
        if bool((key[1:] <= key[:-1]).any()):
            raise ValueError("isosurface_sparse: bricks are not strictly ascending in (x, y, z) (the order of torch.nonzero)")
    return n, K


@torch.no_grad()
def brick_neighbors(bricks, G):
    """bricks [n,3] int32 on the GPU (ascending) -> [n,7] int32: the index of the brick at offset o = 1..7 (bit0 = +x, bit1 = +y,
    bit2 = +z), -1 where there is none (ncw_mcs_neighbors)."""
    nbr = torch.empty(bricks.shape[0], 7, dtype=torch.int32, device=bricks.device)
    L.check(L.get_lib().ncw_mcs_neighbors(L.ptr(bricks), bricks.shape[0], int(G), L.ptr(nbr), L.stream_ptr(bricks.device)),
            "ncw_mcs_neighbors")
    return nbr


def _mcs_count(values, bricks, nbr, up, G, level):
    """counts [K] uint8: triangles of the cube at every sub-voxel (ncw_mcs_count)."""
    dev = values.device
    counts = torch.empty(values.shape[0], dtype=torch.uint8, device=dev)
    L.check(L.get_lib().ncw_mcs_count(L.ptr(values), values.shape[0], L.ptr(bricks), L.ptr(nbr), bricks.shape[0], up, G, float(level),
                                      L.ptr(_mc_tables(dev)[1]), L.ptr(counts), L.stream_ptr(dev)), "ncw_mcs_count")
    return counts


def _mcs_compact(counts, bricks, up, G):
    """The non-empty cubes in the dense path's cube order: (sub [M] int64 indices into counts, offsets [M] int64 exclusive scan
    of their counts, T).  One device->host read: the mesh size."""
    dev = counts.device
    sub = torch.nonzero(counts).reshape(-1)
    M = sub.shape[0]
    if M == 0:
        return sub, sub, 0
    ids = torch.empty(M, dtype=torch.int64, device=dev)
    L.check(L.get_lib().ncw_mcs_cube_ids(L.ptr(bricks), bricks.shape[0], up, G, L.ptr(sub), M, L.ptr(ids), L.stream_ptr(dev)),
            "ncw_mcs_cube_ids")
    sub = sub[torch.argsort(ids)].contiguous()  # the ids are distinct: no tie to break
    cnt = counts[sub]
    incl = torch.cumsum(cnt, 0, dtype=torch.int64)
    return sub, (incl - cnt).contiguous(), int(incl[-1])


def _mcs_emit(values, bricks, nbr, up, G, level, sub, offsets, T):
    """tri_pos [T,3,3] float32, tri_key [T,3] int64 (ncw_mcs_emit)."""
    dev = values.device
    tri, ntri, edges = _mc_tables(dev)
    pos = torch.empty(T, 3, 3, device=dev, dtype=torch.float32)
    key = torch.empty(T, 3, device=dev, dtype=torch.int64)
    L.check(L.get_lib().ncw_mcs_emit(L.ptr(values), values.shape[0], L.ptr(bricks), L.ptr(nbr), bricks.shape[0], up, G, float(level),
                                     L.ptr(tri), L.ptr(ntri), L.ptr(edges), L.ptr(sub), L.ptr(offsets), sub.shape[0], T, L.ptr(pos),
                                     L.ptr(key), L.stream_ptr(dev)), "ncw_mcs_emit")
    return pos, key


def _weld(pos, key):
    """One vertex per grid edge, in ascending key order, and the faces without the degenerate ones: the tail of `isosurface`."""
    T = key.shape[0]
    uniq, inv = torch.unique(key.reshape(-1), return_inverse=True)
    verts = torch.empty(uniq.shape[0], 3, device=pos.device, dtype=torch.float32)
    verts[inv] = pos.reshape(-1, 3)  # all copies of a vertex are bit-identical (interpolated lo -> hi)
    faces = inv.reshape(T, 3)
    ok = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    return verts, faces[ok]


@torch.no_grad()
def isosurface_sparse(bricks, up, values, level=0.0, *, G, neighbors=None):
    """Marching cubes on the brick-blocked sparse values of `gen_grid_spc`, with no allocation of the size of the lattice
    (csrc/ncw_mc_sparse.hip).  bricks [n,3] integer coarse-voxel indices of a [G]^3 lattice, strictly ascending in (x, y, z)
    (the order of torch.nonzero); up sub-voxels per side (a power of two, 1..32); values [n * up^3] float32, brick-major, then
    local x, y, z with z fastest.  A cube is used iff all 8 of its corners are sparse points.  Returns (verts [V,3] float32 in
    fine grid-index coordinates, faces [F,3] int64): wherever the dense path can run, exactly what
    `isosurface(*sparse_volume(sd, values)[:2], level)` returns, order included -- vertices by (lower grid point, axis z < y < x),
    faces by cube (x slowest), then by table order.  neighbors: the table of `brick_neighbors`, if the caller kept it.
    ValueError for a bad up, a wrong number of values, K > 2^31 - 1, G * up > 16384, bricks out of order or outside [0, G)."""
    if G is None:
        raise ValueError("isosurface_sparse: the coarse lattice side G is required")
    n, K = _check_bricks(bricks, up, values, G)
    up, G = int(up), int(G)
    if not values.is_cuda:
        raise L.NeuconwHipError("mesh.isosurface_sparse: the values are not on a GPU; there is no CPU fallback")
    dev = values.device
    empty = (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev))
    if n == 0:
        return empty
    values = values.reshape(-1).contiguous().float()
    b32 = bricks.to(device=dev, dtype=torch.int32).contiguous()
    nbr = brick_neighbors(b32, G) if neighbors is None else neighbors.to(device=dev, dtype=torch.int32).contiguous()
    if tuple(nbr.shape) != (n, 7):
        raise ValueError("isosurface_sparse: neighbors must be [n,7]")
    counts = _mcs_count(values, b32, nbr, up, G, level)
    sub, offsets, T = _mcs_compact(counts, b32, up, G)
    if T == 0:
        return empty
    pos, key = _mcs_emit(values, b32, nbr, up, G, level, sub, offsets, T)
    return _weld(pos, key)


@torch.no_grad()
def vertex_colors(renderer, verts_training, embedding_a, chunk=1 << 16):
    """utils/visualization.py:124-150: rgb at the vertices, viewed along +z, one appearance code for all."""
    V = verts_training.shape[0]
    dev = verts_training.device
    out = torch.empty(V, 3, device=dev)
    a = embedding_a.reshape(1, -1).to(dev).float()
    for i in range(0, V, chunk):
        p = verts_training[i:i + chunk].float()
        d = torch.zeros_like(p)
        d[:, 2] = 1
        with torch.enable_grad():  # renderer.rgb runs NeuconW.forward, which needs the SDF gradient
            out[i:i + chunk] = renderer.rgb(p.unsqueeze(1), d.unsqueeze(1), a.expand(p.shape[0], -1).unsqueeze(1)).detach()
    return out * 255


@torch.no_grad()
def gen_grid_spc(octree_data, eval_level):
    """tools/extract_mesh.py:60-102 `gen_grid_spc` on the device: the lower corners of the level-`eval_level` sub-voxels of
    the occupied voxels of the training octree (`voxel.octree_from_sfm`), in SfM coordinates.  Same arithmetic and dtypes as the
    reference: index * voxel in float32, + float64 volume origin, (float32 downstream).  Returns the reference's `sparse_data`
    dict (sparse_vol [K,3] float64 tensor on the GPU, voxel_size / vol_origin as numpy float64, dim), plus the blocking of its
    rows: bricks [n,3] int64 (the occupied voxels, ascending) and up (sub-voxels per side), K = n * up^3."""
    from . import voxel

    level = int(octree_data["level"])
    dense = voxel.dense_from_occupancy(octree_data)           # convert_to_dense(octree, level)
    dev = dense.device
    low_dim = dense.shape[0]
    sparse_ind = torch.nonzero(dense)                         # [n,3], lexicographic in (x,y,z)
    up_level = int(eval_level) - level
    if up_level < 0:
        raise ValueError("eval_level %d below the octree level %d" % (eval_level, level))
    up_times = 2 ** up_level
    eval_dim = int(low_dim * up_times)
    k = torch.arange(0, up_times, device=dev)
    up_kernel = torch.stack(torch.meshgrid(k, k, k, indexing="ij"), dim=-1).reshape(-1, 3)
    ind_up = sparse_ind.repeat_interleave(up_times ** 3, dim=0) * up_times + up_kernel.repeat([sparse_ind.shape[0], 1])
    octree_scale = np.float64(octree_data["scale"])
    so = octree_data["scene_origin"]
    octree_origin = np.asarray(so.detach().cpu().numpy() if torch.is_tensor(so) else so, dtype=np.float64).reshape(3)
    eval_voxel_size = 2 / (2 ** int(eval_level)) * octree_scale                       # :91
    vol_origin = octree_origin - octree_scale                                         # :92
    xyz_sfm = (ind_up * float(eval_voxel_size)).double() + torch.from_numpy(vol_origin).to(dev)  # :94 (f32 product, f64 sum)
    # bricks / up (not in the reference): the blocking of sparse_vol -- row (b * up^3 + (lx * up + ly) * up + lz) is sub-voxel
    # (lx, ly, lz) of occupied voxel bricks[b] -- which isosurface_sparse meshes without the dense lattice
    return {"sparse_vol": xyz_sfm, "voxel_size": eval_voxel_size, "dim": eval_dim, "vol_origin": vol_origin,
            "bricks": sparse_ind, "up": up_times}


@torch.no_grad()
def sparse_volume(sparse_data, sdf_values):
    """utils/visualization.py:51-56,91-110: scatter the SDF of the sparse points into a dense [dim]^3 volume of ones and build
    the cube mask -- a grid point is valid iff it and its 7 lower neighbours were evaluated (the reference's rolls, wrap-around
    included).  Returns (sdf_dense, mask, ind)."""
    sparse_vol = sparse_data["sparse_vol"].float()
    dev = sparse_vol.device
    dim = int(sparse_data["dim"])
    vo64 = torch.from_numpy(np.asarray(sparse_data["vol_origin"], dtype=np.float64)).to(dev)
    ind = torch.round((sparse_vol - vo64) / float(sparse_data["voxel_size"])).long()  # :51 (float64 like the reference)
    sdf_dense = torch.ones(dim, dim, dim, device=dev, dtype=torch.float32)
    sdf_dense[ind[:, 0], ind[:, 1], ind[:, 2]] = sdf_values.reshape(-1).float()
    m = torch.zeros(dim, dim, dim, device=dev, dtype=torch.bool)
    m[ind[:, 0], ind[:, 1], ind[:, 2]] = True
    m = (m & torch.roll(m, shifts=1, dims=0) & torch.roll(m, shifts=1, dims=1) & torch.roll(m, shifts=1, dims=2)
         & torch.roll(m, shifts=[1, 1], dims=[0, 1]) & torch.roll(m, shifts=[1, 1], dims=[0, 2])
         & torch.roll(m, shifts=[1, 1], dims=[1, 2]) & torch.roll(m, shifts=[1, 1, 1], dims=[0, 1, 2]))
    return sdf_dense, m, ind


@torch.no_grad()
def extract_mesh(renderer, dim, scene_radius, scene_origin, origin=None, radius=1.0, with_color=False, embedding_a=None,
                 level=0.0, chunk_rgb=1 << 16, sparse_data=None, chunk=1 << 22, group=None, min_component_faces=0,
                 largest_components=None, simplify_cells=0, sparse_mc="auto"):
    """utils/visualization.py:37-159.  Dense path: the [dim]^3 lattice over `origin` +- `radius` (training coordinates), swept
    on chip and sharded over the ranks (grid.sdf_grid).  Sparse path (`sparse_data` from gen_grid_spc): the SDF only at the
    sub-voxels of the occupied octree voxels (sharded like neuconw_system.py:236-256), marching cubes under the all-8-corners
    mask.  Returns dict(vertices [V,3] world coordinates, faces [F,3], vertices_training, colors [V,3] uint8 or None) as GPU
    tensors, on every rank (the reference returns the mesh on rank 0 only).
    min_component_faces > 0 / largest_components = K (not in the reference; both off: this path is not taken): after marching
    cubes and BEFORE the colour pass, only the connected components (by shared vertex index, meshops.clean) of at least that
    many faces / the K with the most faces are kept, so the colour network never runs on floaters.
    simplify_cells > 0 (not in the reference; 0: this path is not taken): after that clean-up and before the colour pass,
    meshops.simplify with a cell of `simplify_cells` voxels (grid-index units): vertex clustering with a quadric-optimal vertex
    per cell, so the colour network runs on far fewer vertices.
    sparse_mc (sparse path only): "dense" scatters the values into the [dim]^3 lattice (sparse_volume + isosurface: the path up
    to dim = 1024, the reference's level 10; ValueError above that); "bricks" runs isosurface_sparse on the blocked values
    (needs the keys bricks / up of gen_grid_spc; no lattice, dim up to 16384), the same mesh bit for bit; "auto" takes the
    dense path up to dim = 1024 and the bricks above."""
    if sparse_mc not in ("auto", "dense", "bricks"):
        raise ValueError("extract_mesh: sparse_mc = %r, not one of auto / dense / bricks" % (sparse_mc,))
    dev = next(renderer.neuconw.parameters()).device
    so = torch.as_tensor(np.asarray(scene_origin, dtype=np.float32), device=dev).reshape(3)
    if sparse_data is None:
        origin = [0.0, 0.0, 0.0] if origin is None else [float(v) for v in origin]
        lo = tuple(o - radius for o in origin)
        hi = tuple(o + radius for o in origin)
        sdf = _grid.sdf_grid(renderer.neuconw.sdf_net, dim, lo, hi, prec=renderer.infer_prec, group=group).view(dim, dim, dim)
        verts, faces = isosurface(sdf, level)
        voxel_size = 2 * radius / (dim - 1)                                      # :44
        vol_origin = torch.tensor(lo, device=dev, dtype=torch.float32)           # :43
    else:
        from . import voxel

        sdim = int(sparse_data["dim"])
        bricks_mc = sparse_mc == "bricks" or (sparse_mc == "auto" and sdim > DENSE_MC_MAX_DIM)
        if not bricks_mc and sdim > DENSE_MC_MAX_DIM:
            raise ValueError("extract_mesh: sparse_mc = 'dense' at dim = %d: the dense lattice path stops at %d (its weld key "
                             "overflows int64 from 1449); use sparse_mc = 'bricks' or 'auto'" % (sdim, DENSE_MC_MAX_DIM))
        if bricks_mc and ("bricks" not in sparse_data or "up" not in sparse_data):
            raise ValueError("extract_mesh: the brick path needs the keys 'bricks' and 'up' of gen_grid_spc in sparse_data")
        sparse_vol = sparse_data["sparse_vol"].to(dev).float()
        xyz = ((sparse_vol - so) / float(scene_radius)).contiguous()             # :58
        sdf_sparse = voxel._sdf_sharded(renderer, xyz, int(chunk), group)
        if bricks_mc:
            del xyz, sparse_vol
            up = int(sparse_data["up"])
            verts, faces = isosurface_sparse(sparse_data["bricks"], up, sdf_sparse.reshape(-1), level, G=sdim // up)
        else:
            sdf, mask, _ = sparse_volume(dict(sparse_data, sparse_vol=sparse_vol), sdf_sparse)
            verts, faces = isosurface(sdf, level, mask)
        vo_sfm = torch.from_numpy(np.asarray(sparse_data["vol_origin"], dtype=np.float64)).float().to(dev)  # :53
        vol_origin = (vo_sfm - so) / float(scene_radius)                         # :59
        voxel_size = float(sparse_data["voxel_size"]) / float(scene_radius)      # :61
    if (int(min_component_faces) > 0 or largest_components is not None) and faces.shape[0] > 0:
        from . import meshops

        verts, faces, _, _ = meshops.clean(verts, faces, None, min_component_faces, largest_components)
        faces = faces.long()
    if float(simplify_cells) > 0 and faces.shape[0] > 0:
        from . import meshops

        verts, faces, _, _ = meshops.simplify(verts, faces, float(simplify_cells))
        faces = faces.long()
    verts_t = verts * voxel_size + vol_origin                                    # :116
    verts_w = verts_t * float(scene_radius) + so                                 # :117
    colors = None
    if with_color:
        colors = vertex_colors(renderer, verts_t, embedding_a, chunk_rgb).clamp(0, 255).to(torch.uint8)
    return {"vertices": verts_w, "faces": faces, "vertices_training": verts_t, "colors": colors}


def write_ply(path, vertices, faces, colors=None):
    """Binary little-endian PLY of device tensors (what trimesh's export writes for tools/extract_mesh.py:160-168): float
    coordinates, uchar colours, always a face element."""
    ply.write(path, vertices.detach().cpu().numpy(), faces.detach().cpu().numpy(),
              None if colors is None else colors.detach().cpu().numpy(), coord="f4")
