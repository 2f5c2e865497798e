"""Mesh evaluation on the GPU: precision / recall / F-score of a predicted surface against the
ground-truth point cloud.

Reference: utils/eval_mesh.py:48-123 `eval_mesh` with its use_o3d=False branch (`trimesh_load`, utils/eval_utils.py:61-84)
and the helpers of utils/eval_utils.py (`_compute` :87-100, `bbx_crop` :103-113, `nn_correspondance` :126-154,
`filtered_sfm` :157-173, `point_crop` :176-216).  The reference needs kaolin, trimesh and matplotlib to import and answers
the nearest-neighbour queries with one scipy KDTree query per point; here:
  * nearest neighbours: exact 1-NN over a uniform grid (csrc/ncw_nn.hip, `nn_distances`) -- same distances, no
    approximation, ties to the smaller index;
  * PLY input without trimesh (`ply.read_points`); the ONLY difference from trimesh's vertex array: trimesh merges duplicate
    vertices when it loads a MESH, and `ply.read_points` removes exact-coordinate duplicates only (our own meshes are already
    welded, so the step does nothing on them);
  * the SfM crop with sorted unique cell keys + searchsorted instead of the O(N M) Morton-code compare (`sfm_crop`);
  * all thresholds from one sort per distance vector (`metrics`).
File layout and JSON keys are the reference's.

`eval_mesh(surface=k)` is the reference's OTHER branch (`o3d_load` with is_mesh, utils/eval_utils.py:20-61): the predicted
mesh is scored by k |GT| points drawn uniformly by area from its triangles inside the evaluation box (csrc/ncw_surf.hip,
`sample_surface`), not by its vertices; `error_clouds` writes the error-coloured clouds of utils/eval_mesh.py:96-98
(`visualize_error`, eval_utils.py:116-123).  Unpinned against open3d, whose source is not at hand: its crop rule (taken from
its documentation), its Mersenne-twister stream (unseeded in the reference: not reproducible there either; ours is
Philox4x32-10 of (sample index, seed)) and its double -> uchar colour rounding.

`eval_mesh(exact_recall=True)` measures the recall side -- GT point to prediction -- to the predicted SURFACE itself: exact
point-to-triangle distances in float64 over a uniform grid of triangles (csrc/ncw_ptm.hip, `TriGrid`, `mesh_distances`),
instead of the distance to the nearest vertex or sample, which is always too large.  The reference has no such mode; what
users know it from is trimesh `proximity`, kaolin `point_to_mesh_distance` or open3d `RaycastingScene`, none of which is at
hand: parity with them is unpinned.
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from . import colmap, ply
from . import lib as L
from .ply import read_points as read_ply_points  # noqa: F401  (a binding only: the name the earlier test suites call)

F32_EPS = float(np.finfo(np.float32).eps)
MAX_CELLS = 1 << 24  # cap of the dense cell table (two int32 per cell)
MAX_SHELL = 8        # Chebyshev shells a query walks before it is handed to the brute-force kernel
COARSE_MAX_BLOCKS = 1 << 16  # cap of the coarse occupancy table of NNGrid.query_within (one int32 per block of cells)


# ---------------------------------------------------------------------------------------------------
# exact 1-NN (csrc/ncw_nn.hip)
# ---------------------------------------------------------------------------------------------------
def _grid_dims(ext, h):
    return [max(1, int(np.ceil(e / h))) for e in ext]


def _grid_for(ext, target_cells):
    """Cubic cells of side h over a box of extents `ext` with about `target_cells` cells (at most MAX_CELLS)."""
    ext = [max(float(e), 0.0) for e in ext]
    emax = max(ext)
    if emax <= 0.0:
        return 1.0, [1, 1, 1]
    target = max(1, min(int(target_cells), MAX_CELLS))
    lo_h, hi_h = emax * 1e-7, emax * 1.0001  # hi_h: one cell along the longest edge
    for _ in range(60):  # geometric bisection: the smallest h whose table fits the target
        mid = (lo_h * hi_h) ** 0.5
        n = np.prod(_grid_dims(ext, mid), dtype=np.float64)
        if n > target:
            lo_h = mid
        else:
            hi_h = mid
    return hi_h, _grid_dims(ext, hi_h)


class NNGrid:
    """The reference cloud P (f32, recentred) bucketed on a uniform grid.  The grid box is P's own box with its 0.1 % tails on
    every axis cut off (far outliers would otherwise stretch the cells over the whole scene); points and queries outside it
    are clamped into the boundary cells.  That keeps the search exact: a point in a cell below the block's lower face lies
    below that face whether it was clamped or not, and the faces on the grid boundary never enter the stop bound.
    `coord_max`: the largest |coordinate| of P and the queries (sets the rounding margin of the stop test).  Built once,
    queried with `query` (every query answered; the far ones by a brute-force pass) or `query_within` (the nearest point within a
    radius, or nothing: one launch over a second, coarse occupancy level, no brute-force pass)."""

    def __init__(self, ref32, coord_max, max_shell=MAX_SHELL, target_cells=None):
        if not ref32.is_cuda:
            raise L.NeuconwHipError("evalmesh.NNGrid: the reference cloud is not on a GPU; there is no CPU fallback")
        self.dev = ref32.device
        self.ref = ref32.contiguous()
        self.m = int(ref32.shape[0])
        sample = self.ref[:: max(1, self.m // 65536)]
        if sample.shape[0] >= 1000:
            q = torch.quantile(sample, torch.tensor([1e-3, 1 - 1e-3], device=self.dev), dim=0)
            lo, hi = q[0].tolist(), q[1].tolist()
        else:
            lo, hi = self.ref.amin(0).tolist(), self.ref.amax(0).tolist()
        self.lo = [float(v) for v in lo]
        self.ext = [float(b) - float(a) for a, b in zip(lo, hi)]
        self.max_shell = int(max_shell)
        # rounding of the cell assignment and of the face distances is of order eps * (|x| + extent): the stop test keeps
        # that much in hand
        self.margin = 16 * F32_EPS * (float(coord_max) + max(self.ext) + 1e-30)
        self.refined = False
        self._build(self.m if target_cells is None else target_cells)
        if target_cells is None:
            # surface clouds leave most cells empty and crowd a few: when the fullest cell is far above the mean of the
            # table, refine once so that the non-empty cells hold about 2 points (area scales as h^-2)
            counts = self._counts()
            mean_all = self.m / float(self.ncells)
            occ = self.m / float(max(1, int((counts > 0).sum())))
            if int(counts.max()) > 32 * max(mean_all, 1.0) and occ > 4 and self.ncells < MAX_CELLS:
                self._build(int(min(MAX_CELLS, self.ncells * (occ / 2.0) ** 1.5)))
                self.refined = True

    def _build(self, target_cells):
        lib = L.get_lib()
        h, dims = _grid_for(self.ext, target_cells)
        self.h, self.dims = h, dims
        self.ncells = int(dims[0] * dims[1] * dims[2])
        self.coarse = None  # the coarse level of query_within: built on its first call
        g = L.NcwNnGrid()
        for a in range(3):
            g.lo[a], g.dim[a] = self.lo[a], dims[a]
        g.h, g.inv_h = h, 1.0 / h
        self.cgrid = g
        keys = torch.empty(self.m, dtype=torch.int32, device=self.dev)
        L.check(lib.ncw_nn_cell_keys(L.ptr(self.ref), self.m, C.byref(g), L.ptr(keys), L.stream_ptr(self.dev)), "ncw_nn_cell_keys")
        skeys, order = torch.sort(keys, stable=True)
        self.sorted_keys = skeys.contiguous()
        self.range = torch.zeros(self.ncells, 2, dtype=torch.int32, device=self.dev)
        self.pts = torch.empty(self.m, 4, dtype=torch.float32, device=self.dev)
        L.check(lib.ncw_nn_cell_ranges(L.ptr(self.ref), L.ptr(self.sorted_keys), L.ptr(order.contiguous()), self.m,
                                       L.ptr(self.range), L.ptr(self.pts), L.stream_ptr(self.dev)), "ncw_nn_cell_ranges")

    def _counts(self):
        return self.range[:, 1] - self.range[:, 0]

    def query(self, q32, stats=None):
        """(dist [N] f32, idx [N] int64) of every query's nearest point of P; stats (dict) gets `escaped`."""
        lib = L.get_lib()
        n = int(q32.shape[0])
        q32 = q32.contiguous()
        dist = torch.empty(n, dtype=torch.float32, device=self.dev)
        idx = torch.empty(n, dtype=torch.int64, device=self.dev)
        keys = torch.empty(n, dtype=torch.int32, device=self.dev)
        s = L.stream_ptr(self.dev)
        L.check(lib.ncw_nn_cell_keys(L.ptr(q32), n, C.byref(self.cgrid), L.ptr(keys), s), "ncw_nn_cell_keys")
        q_order = torch.sort(keys, stable=True)[1].contiguous()
        escaped = torch.empty(n, dtype=torch.int32, device=self.dev)
        n_esc = torch.zeros(1, dtype=torch.int32, device=self.dev)
        L.check(lib.ncw_nn_query(L.ptr(self.pts), L.ptr(self.range), L.ptr(q32), L.ptr(q_order), n, C.byref(self.cgrid),
                                 self.max_shell, float(self.margin), L.ptr(dist), L.ptr(idx), L.ptr(escaped), L.ptr(n_esc), s),
                "ncw_nn_query")
        ne = int(n_esc.item())  # one device->host read: the size of the escape launch
        if ne:
            scratch = torch.empty(ne, dtype=torch.int64, device=self.dev)
            L.check(lib.ncw_nn_brute(L.ptr(self.pts), self.m, L.ptr(q32), L.ptr(escaped), ne, L.ptr(scratch), L.ptr(dist),
                                     L.ptr(idx), s), "ncw_nn_brute")
        if stats is not None:
            stats["escaped"] = stats.get("escaped", 0) + ne
        return dist, idx

    def build_coarse(self, block=None):
        """The coarse occupancy level of `query_within`: the number of points per block of `block`^3 fine cells (int32,
        ceil(dim / block) entries per axis), built by `ncw_nn_coarse` and kept with the grid.  The rule for `block` when none
        is given: the smallest power of two >= 4 whose table has at most COARSE_MAX_BLOCKS entries -- small enough that an empty
        region costs few lookups, and a table (256 KiB at the most) that stays in the caches."""
        if block is None:
            block = 4
            while np.prod([-(-d // block) for d in self.dims], dtype=np.float64) > COARSE_MAX_BLOCKS:
                block *= 2
        block = int(block)
        if block < 1 or block > 65536 or block & (block - 1):
            raise ValueError("evalmesh.NNGrid.build_coarse: block must be a power of two in [1, 65536], got %r" % (block,))
        cdims = [-(-d // block) for d in self.dims]
        coarse = torch.empty(cdims[0] * cdims[1] * cdims[2], dtype=torch.int32, device=self.dev)
        L.check(L.get_lib().ncw_nn_coarse(L.ptr(self.range), C.byref(self.cgrid), block, L.ptr(coarse), L.stream_ptr(self.dev)),
                "ncw_nn_coarse")
        self.coarse, self.coarse_block, self.coarse_dims = coarse, block, cdims
        return coarse

    def query_within(self, q32, max_dist, stats=None):
        """(dist [N] f32, idx [N] int64): every query's nearest point of P if it lies within `max_dist` (d^2 <= float32(max_dist)^2,
        inclusive), else dist = +inf and idx = -1.  Exact, ties to the smaller index; where a query qualifies, the bits are
        those of `query`'s shell walk.  One launch answers every query (`ncw_nn_query_within`): no escape list, no brute-force
        pass; max_dist = inf gives the unbounded answer.  The coarse level is built on the first call (`build_coarse`).
        stats (dict) gets `beyond` (the queries answered -1).  ValueError unless max_dist > 0."""
        max_dist = float(max_dist)
        if not max_dist > 0:
            raise ValueError("evalmesh.NNGrid.query_within: max_dist must be > 0, got %r" % (max_dist,))
        if not q32.is_cuda:
            raise L.NeuconwHipError("evalmesh.NNGrid.query_within: the queries are not on a GPU; there is no CPU fallback")
        lib = L.get_lib()
        if self.coarse is None:
            self.build_coarse()
        n = int(q32.shape[0])
        q32 = q32.contiguous()
        dist = torch.empty(n, dtype=torch.float32, device=self.dev)
        idx = torch.empty(n, dtype=torch.int64, device=self.dev)
        if n:
            keys = torch.empty(n, dtype=torch.int32, device=self.dev)
            s = L.stream_ptr(self.dev)
            L.check(lib.ncw_nn_cell_keys(L.ptr(q32), n, C.byref(self.cgrid), L.ptr(keys), s), "ncw_nn_cell_keys")
            q_order = torch.sort(keys, stable=True)[1].contiguous()
            L.check(lib.ncw_nn_query_within(L.ptr(self.pts), L.ptr(self.range), L.ptr(self.coarse), self.coarse_block, L.ptr(q32),
                                            L.ptr(q_order), n, C.byref(self.cgrid), float(self.margin), max_dist, L.ptr(dist),
                                            L.ptr(idx), s), "ncw_nn_query_within")
        if stats is not None:
            stats["beyond"] = stats.get("beyond", 0) + (int((idx < 0).sum()) if n else 0)
        return dist, idx

    def query_k(self, q32, k, max_dist=None, exclude=None, stats=None, wg=0):
        """(dist [N,k] f32, idx [N,k] int32, count [N] int32): every query's k nearest points of P (`ncw_knn_query`): the k
        smallest (d^2, index) pairs in lexicographic order -- a tie on d^2 goes to the smaller index -- ascending; with
        `max_dist` only points with d^2 <= float32(max_dist)^2 (inclusive); rows beyond `count` hold +inf / -1.  `exclude`
        [N] int32 (or None): an index into P, or -1, that is never reported for that query (a cloud querying itself: only
        that index, a duplicate of the point stays).  A NaN or infinite query gets count 0.  One launch over the coarse level
        (built on the first call, as `query_within`): exact, no brute-force pass.  stats (dict) gets `evals` and `inserts`
        (distance evaluations and list insertions, summed over the queries).  `wg`: the workgroup size (0 = the default).
        ValueError unless 1 <= k <= 32 and max_dist > 0."""
        _check_k("evalmesh.NNGrid.query_k", k, max_dist)
        if not q32.is_cuda or (exclude is not None and not exclude.is_cuda):
            raise L.NeuconwHipError("evalmesh.NNGrid.query_k: the queries are not on a GPU; there is no CPU fallback")
        lib = L.get_lib()
        if self.coarse is None:
            self.build_coarse()
        k = int(k)
        n = int(q32.shape[0])
        q32 = q32.contiguous()
        dist = torch.empty(n, k, dtype=torch.float32, device=self.dev)
        idx = torch.empty(n, k, dtype=torch.int32, device=self.dev)
        count = torch.empty(n, dtype=torch.int32, device=self.dev)
        work = torch.empty(n, 2, dtype=torch.int32, device=self.dev) if stats is not None else None
        if exclude is not None:
            exclude = exclude.to(torch.int32).contiguous()
            if exclude.shape != (n,):
                raise ValueError("evalmesh.NNGrid.query_k: exclude must have one entry per query")
        if n:
            keys = torch.empty(n, dtype=torch.int32, device=self.dev)
            s = L.stream_ptr(self.dev)
            L.check(lib.ncw_nn_cell_keys(L.ptr(q32), n, C.byref(self.cgrid), L.ptr(keys), s), "ncw_nn_cell_keys")
            q_order = torch.sort(keys, stable=True)[1].contiguous()
            L.check(lib.ncw_knn_query(L.ptr(self.pts), L.ptr(self.range), L.ptr(self.coarse), self.coarse_block, L.ptr(q32),
                                      L.ptr(q_order), L.ptr(exclude) if exclude is not None else None, n, C.byref(self.cgrid),
                                      float(self.margin), float("inf") if max_dist is None else float(max_dist), k, int(wg),
                                      L.ptr(idx), L.ptr(dist), L.ptr(count), L.ptr(work) if work is not None else None, s),
                    "ncw_knn_query")
        if stats is not None:
            tot = work.long().sum(0).tolist() if n else [0, 0]
            stats["evals"] = stats.get("evals", 0) + int(tot[0])
            stats["inserts"] = stats.get("inserts", 0) + int(tot[1])
        return dist, idx, count


KNN_MAX_K = 32


def _check_k(what, k, max_dist):
    if not (isinstance(k, (int, np.integer)) and 1 <= int(k) <= KNN_MAX_K):
        raise ValueError("%s: k must be an integer in [1, %d], got %r" % (what, KNN_MAX_K, k))
    if max_dist is not None and not float(max_dist) > 0:
        raise ValueError("%s: max_dist must be > 0, got %r" % (what, max_dist))


def recentre(ref, query):
    """Both clouds moved to their common box centre in float64, then cast to f32 (scene coordinates are metres and may be
    far from the origin).  Returns (ref32, query32, largest |recentred coordinate|, centre float64 numpy)."""
    both = [t for t in (ref, query) if t.shape[0] > 0]
    lo = torch.stack([t.double().amin(0) for t in both]).amin(0).cpu().numpy()
    hi = torch.stack([t.double().amax(0) for t in both]).amax(0).cpu().numpy()
    centre = (lo + hi) / 2.0
    c = torch.from_numpy(centre).to(ref.device)
    r32 = (ref.double() - c).float().contiguous()
    q32 = (query.double() - c).float().contiguous()
    cmax = float(torch.maximum(r32.abs().amax(), q32.abs().amax()))
    return r32, q32, cmax, centre


@torch.no_grad()
def nn_distances(ref, query, max_shell=MAX_SHELL, stats=None, max_dist=None):
    """For every query point its Euclidean distance to the nearest point of `ref` and that point's index -- exact, ties to the
    smaller index (utils/eval_utils.py:126-154 `nn_correspondance(ref, query)`).  ref [M,3], query [N,3]: GPU tensors (any
    float dtype).  Returns (dist [N] float32, idx [N] int64); empty results when either side is empty (as the reference).
    stats (dict, optional) gets the grid shape and the number of queries that took the brute-force path (`escaped`).
    max_dist (a number > 0, default None = no bound, the path above unchanged): only a nearest point within max_dist is
    reported, dist = +inf and idx = -1 otherwise (`NNGrid.query_within`: one launch, no brute-force pass; stats gets `beyond`
    instead of `escaped`).  ValueError unless max_dist > 0."""
    if max_dist is not None and not float(max_dist) > 0:
        raise ValueError("evalmesh.nn_distances: max_dist must be > 0, got %r" % (max_dist,))
    if not (ref.is_cuda and query.is_cuda):
        raise L.NeuconwHipError("evalmesh.nn_distances: the clouds are not on a GPU; there is no CPU fallback")
    dev = ref.device
    ref, query = ref.reshape(-1, 3), query.reshape(-1, 3)
    if ref.shape[0] == 0 or query.shape[0] == 0:
        return torch.zeros(0, dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
    r32, q32, cmax, _ = recentre(ref, query)
    grid = NNGrid(r32, cmax, max_shell=max_shell)
    if stats is not None:
        stats.update(dims=list(grid.dims), cells=grid.ncells, refined=grid.refined)
    if max_dist is not None:
        return grid.query_within(q32, max_dist, stats)
    return grid.query(q32, stats)


@torch.no_grad()
def knn(ref, query, k, max_dist=None, exclude_self=False, stats=None):
    """For every query point its k nearest points of `ref`: (dist [N,k] float32, idx [N,k] int32, count [N] int32), exact,
    ascending, ties on equal d^2 to the smaller index, rows beyond `count` +inf / -1 (`NNGrid.query_k`; the clouds are
    recentred as in `nn_distances`).  max_dist: only points within it (inclusive).  exclude_self: `query` is `ref` itself
    (the same number of points) and point i is never its own neighbour (a duplicate of it is).  Empty results when either
    side is empty.  ValueError unless 1 <= k <= 32 and max_dist > 0; NeuconwHipError for CPU tensors."""
    _check_k("evalmesh.knn", k, max_dist)
    if not (ref.is_cuda and query.is_cuda):
        raise L.NeuconwHipError("evalmesh.knn: the clouds are not on a GPU; there is no CPU fallback")
    dev = ref.device
    ref, query = ref.reshape(-1, 3), query.reshape(-1, 3)
    n, k = int(query.shape[0]), int(k)
    if exclude_self and ref.shape[0] != n:
        raise ValueError("evalmesh.knn: exclude_self needs query to be ref itself (%d != %d points)" % (n, ref.shape[0]))
    if ref.shape[0] == 0 or n == 0:
        return (torch.full((n, k), float("inf"), dtype=torch.float32, device=dev),
                torch.full((n, k), -1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    r32, q32, cmax, _ = recentre(ref, query)
    grid = NNGrid(r32, cmax)
    if stats is not None:
        stats.update(dims=list(grid.dims), cells=grid.ncells, refined=grid.refined)
    exclude = torch.arange(n, dtype=torch.int32, device=dev) if exclude_self else None
    return grid.query_k(q32, k, max_dist=max_dist, exclude=exclude, stats=stats)


# ---------------------------------------------------------------------------------------------------
# PLY / COLMAP input
# ---------------------------------------------------------------------------------------------------
def apply_transform(points, T):
    """(T[:3] @ [p, 1]^T)^T in float64: the reference's homogeneous product (eval_utils.py:70-71, :167-168)."""
    T = np.asarray(T, dtype=np.float64)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    ph = np.concatenate((p, np.ones((p.shape[0], 1))), axis=-1)
    return (T[:3] @ ph.T).T


def read_points3d_filtered(path, track_length, reproj_error, sfm_to_gt=None):
    """utils/eval_utils.py:157-173 `filtered_sfm`: COLMAP points with a track STRICTLY longer than `track_length` and a mean
    reprojection error STRICTLY below `reproj_error`, carried to GT coordinates by `sfm_to_gt` (4x4; None = identity).
    `path`: points3D.bin or the directory holding it.  float64 [K,3] ([0,3] when none passes; the reference raises there)."""
    if os.path.isdir(path):
        path = os.path.join(path, "points3D.bin")
    _, xyz, err, track = colmap.read_points3d(path)
    keep = (track > track_length) & (err < reproj_error)
    pts = xyz[keep]
    return pts if sfm_to_gt is None else apply_transform(pts, sfm_to_gt)


# ---------------------------------------------------------------------------------------------------
# crops and metrics
# ---------------------------------------------------------------------------------------------------
def bbx_crop(points, bbx):
    """utils/eval_utils.py:103-113: the points strictly inside the box (normalised coordinates in the open (-1, 1)^3).
    A torch tensor (any device) is cropped on its device with the same float64 arithmetic and returned as a float64 tensor
    there; anything else goes through numpy."""
    if torch.is_tensor(points):
        p = points.reshape(-1, 3).double()
        bmin = torch.tensor([float(v) for v in bbx[0]], dtype=torch.float64, device=p.device)
        bmax = torch.tensor([float(v) for v in bbx[1]], dtype=torch.float64, device=p.device)
        origin = bmin + (bmax - bmin) / 2
        scale = (bmax - bmin) / 2
        pn = (p - origin) / scale
        return p[(pn > -1).all(-1) & (pn < 1).all(-1)]
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    bmin, bmax = np.array(bbx[0], dtype=np.float64), np.array(bbx[1], dtype=np.float64)
    origin = bmin + (bmax - bmin) / 2
    scale = (bmax - bmin) / 2
    pn = (points - origin) / scale
    return points[(pn > -1).all(-1) & (pn < 1).all(-1)]


def _sfm_crop_torch(points, sfm_points, voxel_size, bbx):
    """`sfm_crop` for a tensor: the same float64 operations in the same order, on the tensor's device."""
    p = points.reshape(-1, 3).double()
    dev = p.device
    if torch.is_tensor(sfm_points):
        sp = sfm_points.reshape(-1, 3).double().to(dev)
    else:
        sp = torch.from_numpy(np.ascontiguousarray(sfm_points, dtype=np.float64).reshape(-1, 3)).to(dev)
    bmin, bmax = np.array(bbx[0], dtype=np.float64), np.array(bbx[1], dtype=np.float64)
    dim = np.max(bmax - bmin)
    origin = torch.from_numpy(bmin + (bmax - bmin) / 2).to(dev)
    scale = float(dim / 2)
    res = int(np.floor(2 * scale / voxel_size))

    def cells(x):
        q = torch.floor(res * ((x - origin) / scale + 1.0) / 2.0)
        ok = ((q >= 0) & (q < res)).all(-1)
        qi = torch.where(ok[:, None], q, torch.zeros_like(q)).long()
        return (qi[:, 0] * res + qi[:, 1]) * res + qi[:, 2], ok

    if p.shape[0] == 0 or sp.shape[0] == 0:
        return p[:0]
    sk, sok = cells(sp)
    sk = torch.unique(sk[sok])
    pk, pok = cells(p)
    if sk.shape[0] == 0:
        return p[:0]
    pos = torch.clamp(torch.searchsorted(sk, pk), 0, sk.shape[0] - 1)
    return p[pok & (sk[pos] == pk)]


def sfm_crop(points, sfm_points, voxel_size, bbx):
    """utils/eval_utils.py:176-216 `point_crop`: keep the points whose voxel holds an SfM point.  Cube of half-size
    (longest box edge) / 2 around the box centre, res = floor(2 scale / voxel_size), cell = floor(res (x + 1) / 2) per axis
    with NO clamp.  The reference compares every point's kaolin Morton code against every SfM code (O(N M)); here sorted
    unique cell keys + searchsorted.  One difference: SfM cells outside [0, res)^3 are dropped.  In the reference such a cell
    could only match through kaolin's Morton code of negative / overflowing int16 coordinates, which cannot be pinned
    without kaolin; points outside the cube therefore never survive the crop here.
    `points` as a torch tensor (any device) is cropped on its device -- same float64 arithmetic, same comparisons -- and
    returned as a float64 tensor there (`sfm_points` may be numpy or a tensor)."""
    if torch.is_tensor(points):
        return _sfm_crop_torch(points, sfm_points, voxel_size, bbx)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    sfm_points = np.asarray(sfm_points, dtype=np.float64).reshape(-1, 3)
    bmin, bmax = np.array(bbx[0], dtype=np.float64), np.array(bbx[1], dtype=np.float64)
    dim = np.max(bmax - bmin)
    origin = bmin + (bmax - bmin) / 2
    scale = dim / 2
    res = int(np.floor(2 * scale / voxel_size))

    def cells(p):
        q = np.floor(res * ((p - origin) / scale + 1.0) / 2.0)
        ok = ((q >= 0) & (q < res)).all(-1)
        qi = np.where(ok[:, None], q, 0).astype(np.int64)
        return (qi[:, 0] * res + qi[:, 1]) * res + qi[:, 2], ok

    if points.shape[0] == 0 or sfm_points.shape[0] == 0:
        return points[:0]
    sk, sok = cells(sfm_points)
    sk = np.unique(sk[sok])
    pk, pok = cells(points)
    if sk.shape[0] == 0:
        return points[:0]
    pos = np.clip(np.searchsorted(sk, pk), 0, sk.shape[0] - 1)
    return points[pok & (sk[pos] == pk)]


def _as_f64(d, dev=None):
    if torch.is_tensor(d):
        return d.reshape(-1).double()
    return torch.as_tensor(np.asarray(d, dtype=np.float64).reshape(-1), device=dev)


@torch.no_grad()
def metrics(d_gt_to_pred, d_pred_to_gt, thresholds):
    """utils/eval_utils.py:87-100 `_compute` for every threshold (list of dicts, the reference's keys): `dist1` = mean
    pred->gt distance, `dist2` = mean gt->pred distance, `prec` = fraction of pred->gt distances < t, `recal` = fraction of
    gt->pred distances < t (both floored at 1e-6), `fscore` = 2 prec recal / (prec + recal).  Each distance vector is sorted
    once (float64, on its device) and counted with searchsorted.  Empty vectors give NaN, as numpy's mean does."""
    single = not isinstance(thresholds, (list, tuple, np.ndarray))
    ts = [float(thresholds)] if single else [float(t) for t in thresholds]
    dev = d_gt_to_pred.device if torch.is_tensor(d_gt_to_pred) else None
    a = _as_f64(d_gt_to_pred, dev)    # reference dist1
    b = _as_f64(d_pred_to_gt, a.device)  # reference dist2
    t = torch.tensor(ts, dtype=torch.float64, device=a.device)

    def frac_below(d):
        if d.numel() == 0:
            return [float("nan")] * len(ts)
        cnt = torch.searchsorted(torch.sort(d)[0], t, right=False)  # number of entries strictly below t
        n = d.numel()
        return [c / n for c in cnt.cpu().tolist()]  # correctly rounded on the host, as numpy's mean of the 0/1 vector

    def mean(d):
        return float(d.mean()) if d.numel() else float("nan")

    pa, pb = frac_below(a), frac_below(b)
    m1, m2 = mean(b), mean(a)
    out = []
    for i in range(len(ts)):
        precision = max(pb[i], 1e-6)  # Python's max keeps a NaN first argument, like the reference
        recal = max(pa[i], 1e-6)
        fscore = 2 * precision * recal / (precision + recal)
        out.append({"dist1": m1, "dist2": m2, "prec": precision, "recal": recal, "fscore": fscore})
    return out


# ---------------------------------------------------------------------------------------------------
# area-weighted surface samples (csrc/ncw_surf.hip; utils/eval_utils.py:39-43)
# ---------------------------------------------------------------------------------------------------
SURFACE_MODES = {"iid": 0, "stratified": 1}


def _cuda_device(device, what):
    if device is None:
        if not torch.cuda.is_available():
            raise L.NeuconwHipError("evalmesh.%s: no GPU; there is no CPU fallback" % what)
        return torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.NeuconwHipError("evalmesh.%s runs on a GPU only; there is no CPU fallback" % what)
    return dev


def _box6(box):
    if box is None:
        return None
    lo, hi = [float(v) for v in box[0]][:3], [float(v) for v in box[1]][:3]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("box: [[x0, y0, z0], [x1, y1, z1]]")
    return (C.c_double * 6)(*(lo + hi))


@torch.no_grad()
def surface_weights(verts, faces, box=None):
    """ncw_surf_weights: float64 [F] triangle areas of faces (int32 [F,3], device) over verts (float64 [V,3], device);
    exactly 0 for a corner index outside [0, V), a non-finite area, or -- with `box` = [lo, hi] -- a corner outside the
    closed box (open3d's documented `TriangleMesh.crop` rule; unpinned)."""
    if not (verts.is_cuda and faces.is_cuda):
        raise L.NeuconwHipError("evalmesh.surface_weights: the mesh is not on a GPU; there is no CPU fallback")
    assert verts.dtype == torch.float64 and faces.dtype == torch.int32
    verts, faces = verts.reshape(-1, 3).contiguous(), faces.reshape(-1, 3).contiguous()
    w = torch.empty(faces.shape[0], dtype=torch.float64, device=verts.device)
    L.check(L.get_lib().ncw_surf_weights(L.ptr(verts), verts.shape[0], L.ptr(faces), faces.shape[0], _box6(box), L.ptr(w),
                                         L.stream_ptr(verts.device)), "ncw_surf_weights")
    return w


@torch.no_grad()
def surface_cdf(weight):
    """The table ncw_surf_pick / ncw_surf_sample search: the inclusive prefix sum of the weights in float64
    (torch.cumsum), made safe against the scan's rounding.  A parallel prefix sum adds in a different order at every
    position, so next to a triangle of weight 0 it may differ from its neighbour in the last bit, and such a triangle could
    then be drawn (its corners may be out of range).  Here an entry of weight 0 is replaced by the running maximum of the
    entries before it, and the whole table is made non-decreasing by that running maximum: a zero-weight triangle repeats
    its predecessor exactly and can never be returned."""
    cdf = torch.cumsum(weight.double(), 0)
    if cdf.numel() == 0:
        return cdf
    return torch.cummax(torch.where(weight > 0, cdf, torch.zeros_like(cdf)), 0).values.contiguous()


@torch.no_grad()
def sample_surface(verts, faces, n, seed=0, mode="stratified", box=None, return_index=False, chunk=None, device=None):
    """`n` points drawn uniformly by area from the triangles of a mesh (open3d's `sample_points_uniformly`,
    utils/eval_utils.py:42, after `crop(box)`, :39) on the GPU: float64 [n,3] on the device, and with `return_index` the
    int32 [n] triangle of every point.  verts [V,3] (numpy or tensor; used as float64), faces [F,3] (numpy or tensor of an
    INTEGER dtype, checked here; corner indices outside [0, V) give the triangle weight 0).  `box` = [lo, hi] keeps the
    triangles with all three corners inside the closed box.  mode "stratified" (default): sample i searches
    u = (i + xi_i) / n of the area table, so every triangle gets floor or ceil of its share and a wavefront's searches stay
    together; "iid": u = xi_i, independent draws (the reference's distribution).  Either way each point is uniform over
    the surface.  The stream is Philox4x32-10 of (i, seed): the same (seed, n, mode) gives the same points bit for bit, for
    any `chunk` (samples per launch; None = one launch).  An empty mesh or a total weight of 0 returns [0,3].  No CPU
    fallback: NeuconwHipError without a GPU."""
    if mode not in SURFACE_MODES:
        raise ValueError("mode: one of %s (got %r)" % (", ".join(sorted(SURFACE_MODES)), mode))
    f = faces if torch.is_tensor(faces) else torch.as_tensor(np.asarray(faces))
    if f.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError("faces: an integer array of shape [F,3] (got %s %s)" % (f.dtype, tuple(f.shape)))
    n = int(n)
    if n < 0:
        raise ValueError("n must not be negative")
    if device is None and torch.is_tensor(verts) and verts.is_cuda:
        device = verts.device
    dev = _cuda_device(device, "sample_surface")
    v = verts if torch.is_tensor(verts) else torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float64))
    v = v.detach().reshape(-1, 3).to(dev).double().contiguous()
    f = f.detach().to(dev).long()
    if f.shape[0] >= (1 << 31):
        raise ValueError("at most 2^31 - 1 faces")
    # an index that does not fit int32 must stay out of range after the cast
    f = torch.where((f < 0) | (f >= v.shape[0]), torch.full_like(f, -1), f).int().contiguous()
    pts = torch.empty(n, 3, dtype=torch.float64, device=dev)
    tri = torch.empty(n, dtype=torch.int32, device=dev) if return_index else None
    total = 0.0
    if f.shape[0] and v.shape[0] and n:
        cdf = surface_cdf(surface_weights(v, f, box))
        total = float(cdf[-1])  # one device -> host read
    if not (total > 0.0):
        return (pts[:0], tri[:0]) if return_index else pts[:0]
    lib, s = L.get_lib(), L.stream_ptr(dev)
    step = n if chunk is None else max(1, int(chunk))
    for i0 in range(0, n, step):
        c = min(step, n - i0)
        L.check(lib.ncw_surf_sample(L.ptr(v), L.ptr(f), L.ptr(cdf), f.shape[0], int(seed) & 0xFFFFFFFFFFFFFFFF, i0, c, n,
                                    SURFACE_MODES[mode], L.ptr(pts[i0:i0 + c]), L.ptr(tri[i0:i0 + c]) if return_index else None,
                                    None, s), "ncw_surf_sample")
    return (pts, tri) if return_index else pts


# ---------------------------------------------------------------------------------------------------
# exact point-to-mesh distances (csrc/ncw_ptm.hip)
# ---------------------------------------------------------------------------------------------------
F64_EPS = float(np.finfo(np.float64).eps)
PTM_MAX_PAIRS = (1 << 31) - 1      # (cell, triangle) pairs of one grid: int32 positions in the cell table
PTM_MAX_CELLS_PER_TRI = 512        # a triangle whose box covers more cells goes to the large list
PTM_NO_LARGE = 1 << 30             # max_cells_per_tri that keeps every triangle in the grid (a grid has at most 2^24 cells)


def ptm_centre(verts, query):
    """The centre `mesh_distances` recentres by: `recentre`'s -- the centre of the common box of both point sets, in float64
    -- over the rows that are finite (a NaN vertex makes its triangles invalid, it must not poison the centre), and without
    the cast to f32.  Tensors on any device.  Returns (centre float64 numpy [3], largest |recentred coordinate|)."""
    sets = []
    for t in (verts, query):
        t = t.reshape(-1, 3).double()
        t = t[torch.isfinite(t).all(-1)]
        if t.shape[0]:
            sets.append(t)
    if not sets:
        return np.zeros(3), 0.0
    lo = torch.stack([t.amin(0) for t in sets]).amin(0).cpu().numpy()
    hi = torch.stack([t.amax(0) for t in sets]).amax(0).cpu().numpy()
    centre = (lo + hi) / 2.0
    c = torch.from_numpy(centre).to(sets[0].device)
    return centre, max(float((t - c).abs().amax()) for t in sets)


class TriGrid:
    """The triangles of a mesh (verts float64 [V,3], faces int32 [F,3], device tensors, in the caller's coordinates) packed,
    recentred by `centre` (float64 [3]) and binned on a uniform grid of cubic cells over the box of the valid triangles: a
    triangle belongs to every cell its axis-aligned box overlaps; one over more than `max_cells_per_tri` cells goes to the
    large list that every query tests first.  Validity as ncw_ptm_pack: corner indices in range, finite corners, and with
    `box` all three corners inside the closed box.  The cell side is twice the median box size of the triangles, raised
    until the table has at most MAX_CELLS cells, and doubled (rebuild) while the pair count would pass 2^31 - 1;
    `target_cells` fixes the table size instead (tests).  `coord_max`: the largest |recentred coordinate| of the mesh and
    the queries (sets the rounding margin of the stop test).  Built once, queried with `query`.  ValueError when no
    triangle is valid."""

    def __init__(self, verts, faces, centre, coord_max, box=None, max_shell=MAX_SHELL, target_cells=None, max_cells_per_tri=None):
        if not (verts.is_cuda and faces.is_cuda):
            raise L.NeuconwHipError("evalmesh.TriGrid: the mesh is not on a GPU; there is no CPU fallback")
        assert verts.dtype == torch.float64 and faces.dtype == torch.int32
        lib = L.get_lib()
        self.dev = verts.device
        verts, faces = verts.reshape(-1, 3).contiguous(), faces.reshape(-1, 3).contiguous()
        self.n_faces = int(faces.shape[0])
        if self.n_faces >= (1 << 31):
            raise ValueError("at most 2^31 - 1 faces")
        self.centre = np.ascontiguousarray(centre, dtype=np.float64).reshape(3)
        self.centre_t = torch.from_numpy(self.centre).to(self.dev)
        self.max_shell = int(max_shell)
        self.max_cells_per_tri = PTM_MAX_CELLS_PER_TRI if max_cells_per_tri is None else int(max_cells_per_tri)
        self.tri = torch.empty(self.n_faces, 9, dtype=torch.float64, device=self.dev)
        self.valid = torch.empty(self.n_faces, dtype=torch.uint8, device=self.dev)
        s = L.stream_ptr(self.dev)
        L.check(lib.ncw_ptm_pack(L.ptr(verts), verts.shape[0], L.ptr(faces), self.n_faces, (C.c_double * 3)(*self.centre.tolist()),
                                 _box6(box), L.ptr(self.tri), L.ptr(self.valid), s), "ncw_ptm_pack")
        ok = self.valid.bool()
        self.n_valid = int(ok.sum()) if self.n_faces else 0
        if self.n_valid == 0:
            raise ValueError("no valid triangle (corner indices in range, finite corners, all three corners inside the box)")
        t3 = self.tri.view(-1, 3, 3)[ok]
        tmin, tmax = t3.amin(1), t3.amax(1)
        lo, hi = tmin.amin(0), tmax.amax(0)
        self.lo = [float(v) for v in lo.tolist()]
        self.ext = [float(b) - float(a) for a, b in zip(lo.tolist(), hi.tolist())]
        size = (tmax - tmin).amax(1)
        size = size[:: max(1, size.shape[0] // 65536)]
        h_tri = 2.0 * float(size.median())
        # rounding of the cell assignment, of the face distances and of d^2 is of order eps * (|x| + extent): the stop test
        # keeps that much in hand
        self.margin = 16 * F64_EPS * (float(coord_max) + max(self.ext) + 1e-300)
        if target_cells is not None:
            h = _grid_for(self.ext, target_cells)[0]
        else:
            h = max(_grid_for(self.ext, MAX_CELLS)[0], h_tri) if h_tri > 0.0 else _grid_for(self.ext, self.n_valid)[0]
        while not self._build(h):
            h *= 2.0

    def _build(self, h):
        """Bins the triangles on cells of side h; False (nothing kept) when the pair count passes PTM_MAX_PAIRS."""
        lib, s = L.get_lib(), L.stream_ptr(self.dev)
        dims = _grid_dims(self.ext, h)
        g = L.NcwPtmGrid()
        for a in range(3):
            g.lo[a], g.dim[a] = self.lo[a], dims[a]
        g.h, g.inv_h = h, 1.0 / h
        count = torch.empty(self.n_faces, dtype=torch.int32, device=self.dev)
        large = torch.empty(self.n_faces, dtype=torch.uint8, device=self.dev)
        L.check(lib.ncw_ptm_count(L.ptr(self.tri), L.ptr(self.valid), self.n_faces, C.byref(g), self.max_cells_per_tri,
                                  L.ptr(count), L.ptr(large), s), "ncw_ptm_count")
        cum = torch.cumsum(count, 0, dtype=torch.int64).contiguous()
        pairs = int(cum[-1])  # one device -> host read: the size of the pair list
        if pairs > PTM_MAX_PAIRS:
            return False
        self.h, self.dims, self.cgrid, self.pairs = h, dims, g, pairs
        self.ncells = int(dims[0] * dims[1] * dims[2])
        self.large_ids = torch.nonzero(large).reshape(-1).int().contiguous()
        self.n_large = int(self.large_ids.shape[0])
        self.range = torch.zeros(self.ncells, 2, dtype=torch.int32, device=self.dev)
        self.ids = torch.empty(pairs, dtype=torch.int32, device=self.dev)
        if pairs:
            keys = torch.empty(pairs, dtype=torch.int32, device=self.dev)
            ids = torch.empty(pairs, dtype=torch.int32, device=self.dev)
            L.check(lib.ncw_ptm_emit(L.ptr(self.tri), L.ptr(count), L.ptr(cum), self.n_faces, C.byref(g), pairs, L.ptr(keys),
                                     L.ptr(ids), s), "ncw_ptm_emit")
            skeys, order = torch.sort(keys, stable=True)
            L.check(lib.ncw_ptm_ranges(L.ptr(skeys.contiguous()), L.ptr(order.contiguous()), L.ptr(ids), pairs, self.ncells,
                                       L.ptr(self.range), L.ptr(self.ids), s), "ncw_ptm_ranges")
        return True

    def query(self, points64, return_closest=False, stats=None):
        """(dist [N] float64, tri [N] int64[, closest [N,3] float64]) of every point (float64 [N,3] on the device, in the
        caller's coordinates) to the surface; closest points come back in the caller's coordinates.  stats (dict) gets
        `dims`, `cells`, `pairs`, `large` and adds up `escaped`."""
        lib, s = L.get_lib(), L.stream_ptr(self.dev)
        n = int(points64.shape[0])
        q = (points64.reshape(-1, 3).double() - self.centre_t).contiguous()
        dist = torch.empty(n, dtype=torch.float64, device=self.dev)
        idx = torch.empty(n, dtype=torch.int64, device=self.dev)
        closest = torch.empty(n, 3, dtype=torch.float64, device=self.dev) if return_closest else None
        ne = 0
        if n:
            keys = torch.empty(n, dtype=torch.int32, device=self.dev)
            L.check(lib.ncw_ptm_cell_keys(L.ptr(q), n, C.byref(self.cgrid), L.ptr(keys), s), "ncw_ptm_cell_keys")
            q_order = torch.sort(keys, stable=True)[1].contiguous()
            escaped = torch.empty(n, dtype=torch.int32, device=self.dev)
            n_esc = torch.zeros(1, dtype=torch.int32, device=self.dev)
            L.check(lib.ncw_ptm_query(L.ptr(self.tri), self.n_faces, L.ptr(self.range), L.ptr(self.ids), L.ptr(self.large_ids),
                                      self.n_large, L.ptr(q), L.ptr(q_order), n, C.byref(self.cgrid), self.max_shell,
                                      float(self.margin), L.ptr(dist), L.ptr(idx), L.ptr(closest), L.ptr(escaped), L.ptr(n_esc),
                                      s), "ncw_ptm_query")
            ne = int(n_esc.item())  # one device -> host read: the size of the escape launch
            if ne:
                scratch = torch.empty(2 * ne, dtype=torch.int64, device=self.dev)
                L.check(lib.ncw_ptm_brute(L.ptr(self.tri), L.ptr(self.valid), self.n_faces, L.ptr(q), n, L.ptr(escaped), ne,
                                          L.ptr(scratch), L.ptr(dist), L.ptr(idx), L.ptr(closest), s), "ncw_ptm_brute")
        if stats is not None:
            stats.update(dims=list(self.dims), cells=self.ncells, pairs=self.pairs, large=self.n_large)
            stats["escaped"] = stats.get("escaped", 0) + ne
        if return_closest:
            return dist, idx, closest + self.centre_t
        return dist, idx


def _mesh_tensors(verts, faces, dev):
    """(float64 [V,3], int32 [F,3]) on the device; faces of an INTEGER dtype, indices that do not fit stay out of range."""
    f = faces if torch.is_tensor(faces) else torch.as_tensor(np.asarray(faces))
    if f.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError("faces: an integer array of shape [F,3] (got %s %s)" % (f.dtype, tuple(f.shape)))
    v = verts if torch.is_tensor(verts) else torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float64))
    v = v.detach().reshape(-1, 3).to(dev).double().contiguous()
    f = f.detach().to(dev).long()
    if f.shape[0] >= (1 << 31):
        raise ValueError("at most 2^31 - 1 faces")
    f = torch.where((f < 0) | (f >= v.shape[0]), torch.full_like(f, -1), f).int().contiguous()
    return v, f


@torch.no_grad()
def mesh_distances(verts, faces, query, box=None, return_closest=False, chunk=None, stats=None, max_shell=MAX_SHELL,
                   target_cells=None, max_cells_per_tri=None):
    """For every query point its exact Euclidean distance to the SURFACE of a triangle mesh, the triangle that realises it
    and, with `return_closest`, the closest point on it -- float64, ties on equal d^2 to the smaller triangle index (the
    distance contract of include/neuconw_hip.h; what trimesh `proximity`, kaolin `point_to_mesh_distance` or open3d
    `RaycastingScene` answer, none of them pinned).  verts [V,3] and query [N,3] (numpy or tensor; used as float64), faces
    [F,3] of an integer dtype.  A triangle counts when its corner indices lie in [0, V), its corners are finite and -- with
    `box` = [lo, hi] -- all three corners are inside the closed box (`surface_weights`' rule: the sampled precision side and
    the exact recall side see the same surface).  Returns (dist [N] float64, tri [N] int64[, closest [N,3] float64]) on the
    device; empty results for an empty query; ValueError when no triangle is valid.  `chunk`: queries per launch (None =
    one launch); results are bit-identical for any chunk.  stats (dict) gets `dims`, `cells`, `pairs`, `large`, `escaped`.
    max_shell / target_cells / max_cells_per_tri: see `TriGrid`.  No CPU fallback: NeuconwHipError without a GPU."""
    dev = None
    for t in (verts, query):
        if dev is None and torch.is_tensor(t) and t.is_cuda:
            dev = t.device
    dev = _cuda_device(dev, "mesh_distances")
    v, f = _mesh_tensors(verts, faces, dev)
    q = query if torch.is_tensor(query) else torch.from_numpy(np.ascontiguousarray(query, dtype=np.float64))
    q = q.detach().reshape(-1, 3).to(dev).double().contiguous()
    n = int(q.shape[0])
    if n == 0:
        out = (torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev))
        return out + (torch.zeros(0, 3, dtype=torch.float64, device=dev),) if return_closest else out
    centre, cmax = ptm_centre(v, q)
    grid = TriGrid(v, f, centre, cmax, box=box, max_shell=max_shell, target_cells=target_cells,
                   max_cells_per_tri=max_cells_per_tri)
    step = n if chunk is None else max(1, int(chunk))
    parts = [grid.query(q[i0:i0 + step], return_closest, stats) for i0 in range(0, n, step)]
    if len(parts) == 1:
        return parts[0]
    return tuple(torch.cat([p[k] for p in parts]) for k in range(len(parts[0])))


# ---------------------------------------------------------------------------------------------------
# error-coloured clouds (utils/eval_utils.py:116-123 `visualize_error`)
# ---------------------------------------------------------------------------------------------------
# matplotlib's "jet": piecewise-linear (x, y) nodes per channel
_JET_NODES = {
    0: ((0.00, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.00, 0.5)),
    1: ((0.000, 0.0), (0.125, 0.0), (0.375, 1.0), (0.640, 1.0), (0.910, 0.0), (1.000, 0.0)),
    2: ((0.00, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.00, 0.0)),
}


def _jet_table(n=256):
    """The n-entry table matplotlib samples from jet's piecewise-linear definition: entry j is the interpolant at j of the
    nodes stretched to [0, n - 1] (first and last entries are the end nodes), clipped to [0, 1].  float64 [n,3]."""
    out = np.empty((n, 3), dtype=np.float64)
    xi = (n - 1) * np.linspace(0, 1, n)
    for ch, nodes in _JET_NODES.items():
        a = np.array(nodes, dtype=np.float64)
        x, y = a[:, 0] * (n - 1), a[:, 1]
        ind = np.searchsorted(x, xi)[1:-1]
        t = (xi[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        out[:, ch] = np.clip(np.concatenate([[y[0]], t * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]]), 0.0, 1.0)
    return out


JET = _jet_table()
JET_U8 = np.round(255.0 * JET).astype(np.uint8)


@torch.no_grad()
def error_colours(dists, threshold):
    """uint8 [n,3] colours of `visualize_error`: v = min(d, 3 t) / (3 t) in float64, looked up in the 256-entry jet table
    at min(int(256 v), 255) (what matplotlib's colormap call does with a float), channel = round(255 c).  open3d's own
    double -> uchar conversion when it writes the cloud is unpinned; round-to-nearest is our choice.  Runs on the device
    of `dists` (tensor) or on the host (numpy)."""
    d = _as_f64(dists)
    max_dist = float(threshold) * 3
    v = torch.clamp(d, max=max_dist) / max_dist
    idx = torch.clamp((v * 256).long(), 0, 255)
    return torch.from_numpy(JET_U8).to(d.device)[idx]


def _write_error_cloud(path, pts, dists, threshold):
    xyz = pts.detach().cpu().numpy() if torch.is_tensor(pts) else pts
    ply.write(path, xyz, rgb=error_colours(dists, threshold).cpu().numpy())


# ---------------------------------------------------------------------------------------------------
# the evaluation (utils/eval_mesh.py:48-123, both branches)
# ---------------------------------------------------------------------------------------------------
def _write_points(path, pts):
    """The clouds of the vertex scoring, as trimesh exports them: float coordinates and an empty face element."""
    ply.write(path, pts, faces=np.zeros((0, 3), dtype=np.int64), coord="f4")


def eval_mesh(file_pred, file_trgt, scene_config, is_mesh, threshold=.1, bbx_name="eval_bbx", save_name="eval", sfm=None,
              device=None, verbose=True, surface=None, surface_seed=0, surface_mode="stratified", error_clouds=None,
              exact_recall=False, normals=None):
    """utils/eval_mesh.py:48-123 with use_o3d=False: load both PLYs (ply.read_points; `is_mesh` is accepted and, as in the
    reference's trimesh branch, not used), carry the prediction to GT coordinates by scene_config['sfm2gt'], crop both to
    scene_config[bbx_name], optionally crop both to the voxels of the filtered SfM points, nearest neighbours in both
    directions on the GPU, metrics per threshold.  `sfm`: dict(path, track_length, reproj_error, voxel_size), or the
    reference's scene_config keys sfm_path / eval_tl / eval_error / eval_voxel.  Writes under
    <dir of file_pred>/eval_<save_name>/: down_gt.ply, down_pred_in_gt.ply, [sfm_points.ply, pred_filtered.ply,
    target_filtered.ply], visualize/<t:.2f>/metrics.json and metrics.json (thresholds, fscores, precs, recals).  Returns the
    last threshold's metrics dict.

    `surface` = k (a number; the reference's value is 10) scores the prediction by its SURFACE, as the reference's open3d
    branch does with is_mesh (utils/eval_utils.py:30-43): file_pred must have faces (ply.read_mesh, vertices as
    stored); its vertices are carried to GT coordinates, the triangles with all three corners inside the closed box are kept
    (open3d's documented crop rule; unpinned), int(|cropped GT|) * k points are drawn uniformly by area on the GPU
    (`sample_surface` with surface_seed / surface_mode) and written to down_pred_in_gt.ply as doubles (open3d's
    write_point_cloud); as in the reference no point-wise box crop follows.  The SfM crop of the samples runs on the device
    (pred_filtered.ply: doubles too).  surface=None is the vertex scoring described above, whatever `is_mesh` is.

    `error_clouds`: None, True (every threshold) or a list of thresholds: writes visualize/<t:.2f>/error_pred_precision.ply
    (the predicted points coloured by their distance to GT) and error_gt_recal.ply (the GT points by their distance to the
    prediction), colours by `error_colours` (utils/eval_mesh.py:96-98).

    `exact_recall` (default off) measures the recall side to the predicted SURFACE: file_pred must have faces, and the GT ->
    prediction distances (`dist2`, `recal`, error_gt_recal.ply) are exact point-to-triangle distances (`mesh_distances`) to
    the triangles with all three corners inside the closed box -- the surface the samples of `surface=k` are drawn from.
    The precision side is unchanged (samples with `surface=k`, vertices otherwise).  One difference from the sampled path
    under the SfM crop: the GT queries are cropped to the SfM voxels as always, the triangles are NOT clipped to them (a
    triangle is not a point: it may cross voxels), so a GT point may be matched to surface that the sampled path would have
    cropped away.  metrics.json then carries "recal_mode": "exact"; with the option off every written byte is as before.

    `normals` = K (an integer in [1, 32]; default None) adds the NORMAL CONSISTENCY of the two scored clouds: after all
    crops the normals of the scored prediction points and of the scored GT points are estimated, each from its own K
    nearest neighbours (`cloudops.estimate_normals`; unoriented), and over the nearest-neighbour pairs the distances
    already use the mean of |n_a . n_b| is formed in float64 where both normals are valid.  The summary metrics.json gets
    `normal_consistency_pred2gt` (every predicted point with its nearest GT point), `normal_consistency_gt2pred`, their mean
    `normal_consistency`, `normals_k`, and per threshold the lists `normal_consistencies_pred2gt` / `_gt2pred` /
    `normal_consistencies`: the same means over the pairs closer than the threshold (strictly, as `prec` / `recal`).  The
    returned dict carries the three overall values too.  Refused together with `exact_recall` (ValueError, before anything
    is written): there the GT side is paired with a triangle, not with a point that has an estimated normal.  With
    normals=None every written byte is as before."""
    if normals is not None:
        _check_k("evalmesh.eval_mesh(normals=)", normals, None)
        if exact_recall:
            raise ValueError("evalmesh.eval_mesh: normals= and exact_recall=True cannot be combined (the exact recall pairs "
                             "a GT point with a triangle, not with a point of the scored cloud)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    save_dir = os.path.join(os.path.dirname(file_pred), "eval_" + str(save_name))
    os.makedirs(save_dir, exist_ok=True)
    log = print if verbose else (lambda *a, **k: None)
    log("results will save in %s" % save_dir)
    sfm_to_gt = np.array(scene_config["sfm2gt"], dtype=np.float64)

    verts_trgt = bbx_crop(ply.read_points(file_trgt), scene_config[bbx_name])
    _write_points(os.path.join(save_dir, "down_gt.ply"), verts_trgt)
    if surface is None:
        verts_pred = bbx_crop(apply_transform(ply.read_points(file_pred), sfm_to_gt), scene_config[bbx_name])
        _write_points(os.path.join(save_dir, "down_pred_in_gt.ply"), verts_pred)
    else:
        m_verts, m_faces, _ = ply.read_mesh(file_pred)
        if m_faces.shape[0] == 0:
            raise ValueError("%s has no faces: surface sampling needs a triangle mesh (surface=None scores points)" % file_pred)
        n_samples = int(int(verts_trgt.shape[0]) * surface)
        verts_pred = sample_surface(apply_transform(m_verts, sfm_to_gt), m_faces, n_samples, seed=surface_seed,
                                    mode=surface_mode, box=scene_config[bbx_name], device=dev)
        log("surface samples: %d" % verts_pred.shape[0])
        ply.write(os.path.join(save_dir, "down_pred_in_gt.ply"), verts_pred.cpu().numpy())
    if exact_recall:
        if surface is None:
            m_verts, m_faces, _ = ply.read_mesh(file_pred)
        if m_faces.shape[0] == 0:
            raise ValueError("%s has no faces: exact recall needs a triangle mesh (exact_recall=False scores points)" % file_pred)

    if sfm is None and "sfm_path" in scene_config:
        sfm = {"path": scene_config["sfm_path"], "track_length": scene_config["eval_tl"],
               "reproj_error": scene_config["eval_error"], "voxel_size": scene_config["eval_voxel"]}
    if sfm is not None:
        sfm_pts = read_points3d_filtered(sfm["path"], sfm["track_length"], sfm["reproj_error"], sfm_to_gt)
        _write_points(os.path.join(save_dir, "sfm_points.ply"), sfm_pts)
        log("filtered points: %d" % sfm_pts.shape[0])
        verts_pred = sfm_crop(verts_pred, sfm_pts, sfm["voxel_size"], scene_config[bbx_name])
        if torch.is_tensor(verts_pred):
            ply.write(os.path.join(save_dir, "pred_filtered.ply"), verts_pred.cpu().numpy())
        else:
            _write_points(os.path.join(save_dir, "pred_filtered.ply"), verts_pred)
        verts_trgt = sfm_crop(verts_trgt, sfm_pts, sfm["voxel_size"], scene_config[bbx_name])
        _write_points(os.path.join(save_dir, "target_filtered.ply"), verts_trgt)

    p = verts_pred if torch.is_tensor(verts_pred) else torch.from_numpy(verts_pred).to(dev)
    g = torch.from_numpy(verts_trgt).to(dev)
    if exact_recall:  # for every GT point the predicted surface itself
        dist1 = mesh_distances(apply_transform(m_verts, sfm_to_gt), m_faces, g, box=scene_config[bbx_name])[0]
    else:
        dist1, idx1 = nn_distances(p, g)  # for every GT point its nearest prediction (eval_mesh.py:88)
    dist2, idx2 = nn_distances(g, p)  # for every predicted point its nearest GT point (:89)

    thresholds = list(threshold) if isinstance(threshold, (list, tuple, np.ndarray)) else [threshold]
    all_m = metrics(dist1, dist2, thresholds)
    fscores, precs, recals = [], [], []
    for t, m in zip(thresholds, all_m):
        save_path = os.path.join(save_dir, "visualize", "%.2f" % t)
        os.makedirs(save_path, exist_ok=True)
        with open(os.path.join(save_path, "metrics.json"), "w") as fh:
            json.dump(m, fh)
        fscores.append(m["fscore"])
        precs.append(m["prec"])
        recals.append(m["recal"])
    if error_clouds is not None and error_clouds is not False:
        for t in (thresholds if error_clouds is True else list(error_clouds)):
            save_path = os.path.join(save_dir, "visualize", "%.2f" % t)
            os.makedirs(save_path, exist_ok=True)
            _write_error_cloud(os.path.join(save_path, "error_pred_precision.ply"), p, dist2, t)
            _write_error_cloud(os.path.join(save_path, "error_gt_recal.ply"), g, dist1, t)
    summary = {"thresholds": [float(t) for t in thresholds], "fscores": fscores, "precs": precs, "recals": recals}
    if exact_recall:
        summary["recal_mode"] = "exact"
    nc = None
    if normals is not None:
        nc = _normal_consistency(p, g, dist1, idx1, dist2, idx2, int(normals), thresholds)
        summary.update(nc)
    with open(os.path.join(save_dir, "metrics.json"), "w") as fh:
        json.dump(summary, fh)
    log("fscores: %s" % fscores)
    log("precs: %s" % precs)
    log("recals: %s" % recals)
    if nc is not None:
        log("normal consistency (k = %d): %s" % (nc["normals_k"], nc["normal_consistency"]))
        return dict(all_m[-1], **{key: nc[key] for key in ("normal_consistency", "normal_consistency_pred2gt",
                                                           "normal_consistency_gt2pred")})
    return all_m[-1]


def _normal_consistency(p, g, dist1, idx1, dist2, idx2, k, thresholds):
    """The normal-consistency keys of eval_mesh's summary: p / g the scored prediction / GT points, (dist1, idx1) for every
    GT point its nearest prediction, (dist2, idx2) for every predicted point its nearest GT point."""
    from . import cloudops

    def half(a, b):
        return (a + b) / 2.0

    n_p, _, v_p = cloudops.estimate_normals(p, k=k)
    n_g, _, v_g = cloudops.estimate_normals(g, k=k)
    p2g = cloudops.normal_consistency(n_p, v_p, n_g, v_g, idx2)[0]
    g2p = cloudops.normal_consistency(n_g, v_g, n_p, v_p, idx1)[0]
    out = {"normal_consistency_pred2gt": p2g, "normal_consistency_gt2pred": g2p, "normal_consistency": half(p2g, g2p),
           "normals_k": int(k), "normal_consistencies_pred2gt": [], "normal_consistencies_gt2pred": [],
           "normal_consistencies": []}
    for t in thresholds:
        a = cloudops.normal_consistency(n_p, v_p, n_g, v_g, torch.where(dist2.double() < float(t), idx2, -1))[0]
        b = cloudops.normal_consistency(n_g, v_g, n_p, v_p, torch.where(dist1.double() < float(t), idx1, -1))[0]
        out["normal_consistencies_pred2gt"].append(a)
        out["normal_consistencies_gt2pred"].append(b)
        out["normal_consistencies"].append(half(a, b))
    return out


def parse_thresholds(text):
    """utils/eval_mesh.py:127-129: "start,end,interval" -> list(np.arange(start, end, interval)); a single value "0.1" ->
    [0.1]."""
    vals = [float(v.strip()) for v in str(text).split(",") if v.strip()]
    if len(vals) == 1:
        return vals
    if len(vals) != 3:
        raise ValueError("--threshold takes one value or start,end,interval (got %r)" % text)
    return [float(v) for v in np.arange(vals[0], vals[1], vals[2])]
