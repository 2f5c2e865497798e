"""Estimating a scene's `sfm2gt` on the GPU: gated point-to-point ICP with a similarity transform (Umeyama) of the filtered SfM
points onto the ground-truth cloud.

    T, report = estimate_sfm2gt("scene", "gt.ply", init="config")          # refines the matrix of scene/config.yaml
    T0 = similarity_from_pairs(sfm_landmarks, gt_landmarks)                   # a coarse start for a scene that has none

Every tool of the evaluation chain multiplies by `sfm2gt` (eval_mesh, the SfM crop, the reprojection filter, the validation
meshes, voxel.py's scene cube) and `gtreproj` CHECKS it; this module PRODUCES it.  The reference has no such tool: heritage-recon
ships the matrices.  Nothing here is pinned against open3d / CloudCompare registration (neither is at hand).

ICP is LOCAL: it refines an initial matrix (the scene's config.yaml, a matrix file, or three or more landmark pairs solved in
closed form by `similarity_from_pairs`) and converges to the nearest minimum.  Run scripts/reproj_error.py on the result: that
remains the check.

The loop (`icp_similarity`).  The target cloud is bucketed ONCE (`AlignTarget`: evalmesh.NNGrid over float32(Q - centre)); per
iteration the SOURCE is transformed (`ncw_align_transform`: float64, the float32 query and the flag "inside the target's box
grown by the gate"), the inside points are compacted with torch and queried (`NNGrid.query`: exact 1-NN, ties to the smaller
index), `ncw_align_sums` reduces the pairs within the gate to a count and 20 float64 sums in a fixed order (no float atomics:
the same bits on every run), and the host solves the similarity from those 22 numbers (`similarity_from_sums`).  The gate shrinks
by `shrink` per iteration down to `gate_min`; the loop stops when the matrix repeats bit for bit or at `max_iter`.
There is no CPU fallback: tensors that are not on a GPU raise NeuconwHipError.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import evalmesh, ply
from . import lib as L

RANK_TOL = 1e-9           # second singular value of the cross-covariance relative to the first: below = collinear pairs
DEFAULT_GATE0 = 0.2       # x the longest edge of the target's box
DEFAULT_GATE_MIN = 4.0    # x the median nearest-neighbour spacing of the target
SPACING_SAMPLES = 16384   # about this many target points measure the spacing
MIN_PAIRS_SHARE = 0.1     # default min_pairs = max(3, ceil(share x source points))


# ---------------------------------------------------------------------------------------------------
# the closed-form solve (host, numpy)
# ---------------------------------------------------------------------------------------------------
def similarity_from_sums(count, sums, cp, cq, with_scale=True):
    """4x4 float64 similarity [sR t; 0 1] minimising sum |sR P_i + t - Q_i|^2 (Umeyama 1991) from the pair count and the sums of
    `ncw_align_sums` (include/neuconw_hip.h: with p = P - cp, q = Q - cq: sums[0:3] = sum p, [3:6] = sum q, [6:15] = sum p_a q_b
    row-major, [15] = sum |p|^2, [16] = sum |q|^2; the rest is not read).  The centred cross-covariance
    Sigma = (sum q p^T - (sum q)(sum p)^T / n) / n = U D V^T, S = diag(1, 1, det(U) det(V)) (the reflection guard),
    R = U S V^T, s = trace(D S) / sigma_p^2 (1 without scale), t = mu_q - s R mu_p.
    Raises ValueError for fewer than 3 pairs and for a cross-covariance of rank below 2 (collinear pairs)."""
    n = int(count)
    if n < 3:
        raise ValueError("a similarity needs at least 3 pairs, got %d" % n)
    s = np.asarray(sums, dtype=np.float64).reshape(-1)
    cp, cq = np.asarray(cp, dtype=np.float64).reshape(3), np.asarray(cq, dtype=np.float64).reshape(3)
    sp, sq, spq = s[0:3], s[3:6], s[6:15].reshape(3, 3)
    sigma = (spq.T - np.outer(sq, sp) / n) / n
    var_p = (s[15] - sp.dot(sp) / n) / n
    if not np.isfinite(sigma).all() or not np.isfinite(var_p):
        raise ValueError("the pairs hold non-finite coordinates")
    U, D, Vt = np.linalg.svd(sigma)
    if not (D[0] > 0 and D[1] > RANK_TOL * D[0] and var_p > 0):
        raise ValueError("the pairs are collinear (cross-covariance of rank below 2): no unique similarity")
    det = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0
    S = np.array([1.0, 1.0, det])
    R = (U * S) @ Vt
    scale = float((D * S).sum() / var_p) if with_scale else 1.0
    mu_p, mu_q = cp + sp / n, cq + sq / n
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = mu_q - T[:3, :3] @ mu_p
    return T


def pair_sums(src, dst, cp, cq):
    """(count, the first 17 sums of include/neuconw_hip.h's rule 5) of explicit pairs, on the host (any order: numpy's sums)."""
    p = np.asarray(src, dtype=np.float64).reshape(-1, 3) - cp
    q = np.asarray(dst, dtype=np.float64).reshape(-1, 3) - cq
    s = np.zeros(L.ALIGN_SUMS)
    s[0:3], s[3:6] = p.sum(0), q.sum(0)
    s[6:15] = (p[:, :, None] * q[:, None, :]).sum(0).reshape(-1)
    s[15], s[16] = (p * p).sum(), (q * q).sum()
    return p.shape[0], s


def similarity_from_pairs(src, dst, with_scale=True):
    """The same solve for explicit landmark pairs src [K,3] -> dst [K,3] (K >= 3, not collinear), on the host: the coarse initial
    matrix of a scene that has none."""
    src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    if src.shape != dst.shape:
        raise ValueError("similarity_from_pairs: %d source points for %d target points" % (src.shape[0], dst.shape[0]))
    if src.shape[0] < 3:
        raise ValueError("a similarity needs at least 3 pairs, got %d" % src.shape[0])
    cp, cq = src.mean(0), dst.mean(0)
    n, s = pair_sums(src, dst, cp, cq)
    return similarity_from_sums(n, s, cp, cq, with_scale)


def decompose_similarity(T):
    """(scale, rotation angle in degrees, translation length) of a 4x4 similarity."""
    T = np.asarray(T, dtype=np.float64)
    A = T[:3, :3]
    scale = float(abs(np.linalg.det(A)) ** (1.0 / 3.0))
    c = (np.trace(A / scale) - 1.0) / 2.0 if scale > 0 else 1.0
    return scale, float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), float(np.linalg.norm(T[:3, 3]))


# ---------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------
def _gpu_points(x, device, what):
    """float64 [K,3] contiguous on a GPU.  numpy goes to `device`; a tensor must already be on one."""
    if torch.is_tensor(x):
        if not x.is_cuda:
            raise L.NeuconwHipError("align.%s: the points are not on a GPU; there is no CPU fallback" % what)
        return x.reshape(-1, 3).double().contiguous()
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise L.NeuconwHipError("align.%s needs a GPU (device %s); there is no CPU fallback" % (what, device))
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)).to(dev)


def _f64x(values):
    return (C.c_double * len(values))(*[float(v) for v in values])


def _f32x(values):
    return (C.c_float * len(values))(*[float(v) for v in values])


class AlignTarget:
    """The ground-truth cloud Q on the device, bucketed once: `points` float64 [M,3] (kept for the sums), `centre` = the centre of
    its box (float64 numpy; also the `cq` of the sums), `box_lo` / `box_hi` = the box of float32(Q - centre) and `grid` =
    evalmesh.NNGrid over it.  `gate_max`: the largest gate a loop may start from (default 0.2 x the longest edge of the box): a
    queried point lies in the box grown by the gate, which bounds the `coord_max` the grid is built with.  `max_shell`: NNGrid's
    (the shells a query walks before it takes the brute-force path; the result does not depend on it)."""

    def __init__(self, gt_points, device="cuda:0", gate_max=None, max_shell=evalmesh.MAX_SHELL):
        q = _gpu_points(gt_points, device, "AlignTarget")
        if q.shape[0] < 3:
            raise ValueError("the target cloud holds %d points" % q.shape[0])
        self.dev, self.points, self.m = q.device, q, int(q.shape[0])
        lo, hi = q.amin(0).cpu().numpy(), q.amax(0).cpu().numpy()
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError("the target cloud holds non-finite coordinates")
        self.lo, self.hi = lo, hi
        self.centre = (lo + hi) / 2.0
        self.longest_edge = float((hi - lo).max())
        self.gate_max = float(DEFAULT_GATE0 * self.longest_edge if gate_max is None else gate_max)
        self.ref32 = (q - torch.from_numpy(self.centre).to(self.dev)).float().contiguous()
        self.box_lo = self.ref32.amin(0).cpu().numpy()
        self.box_hi = self.ref32.amax(0).cpu().numpy()
        coord_max = float(max(np.abs(self.box_lo).max(), np.abs(self.box_hi).max())) + self.gate_max
        self.grid = evalmesh.NNGrid(self.ref32, coord_max, max_shell=max_shell)
        self._spacing = None

    def spacing(self):
        """Median nearest-neighbour spacing of the cloud, measured on a subsample S = every k-th point (k = max(8, M // 16384)) as
        the distance from each point of S to the nearest point of the cloud WITHOUT S (one NNGrid over the rest, one query).
        Equivalent to a self-query that skips the point itself, up to the thinning by 1 / k of the cloud searched."""
        if self._spacing is None:
            k = max(8, self.m // SPACING_SAMPLES)
            pick = torch.zeros(self.m, dtype=torch.bool, device=self.dev)
            pick[::k] = True
            rest, sub = self.ref32[~pick].contiguous(), self.ref32[pick].contiguous()
            if rest.shape[0] < 1 or sub.shape[0] < 1:
                raise ValueError("the target cloud is too small to measure its spacing: pass gate_min")
            cmax = float(max(np.abs(self.box_lo).max(), np.abs(self.box_hi).max()))
            d, _ = evalmesh.NNGrid(rest, cmax).query(sub)
            self._spacing = float(d.double().median())
        return self._spacing


def transform_points(src, T, target, gate):
    """`ncw_align_transform`: (q32 [N,3] float32 = float32(T [p, 1] - target.centre), inside [N] uint8)."""
    n = int(src.shape[0])
    q32 = torch.empty(n, 3, dtype=torch.float32, device=src.device)
    inside = torch.empty(n, dtype=torch.uint8, device=src.device)
    T = np.asarray(T, dtype=np.float64)
    L.check(L.get_lib().ncw_align_transform(L.ptr(src), n, _f64x(T[:3].reshape(-1)), _f64x(target.centre), _f32x(target.box_lo),
                                            _f32x(target.box_hi), float(gate), L.ptr(q32), L.ptr(inside), L.stream_ptr(src.device)),
            "ncw_align_transform")
    return q32, inside


def far_reach(grid):
    """A distance below which an ESCAPED query of `grid` (evalmesh.NNGrid) provably has no point.  ncw_nn_query hands a query to
    the escape list when, after its last shell r = max_shell, the best visited point is not closer than b - margin, b = its
    distance to the faces of the visited block that are not on the grid boundary; every unvisited point lies beyond such a face
    (that is the kernel's own stop argument), and b >= r h because the query lies in the block's centre cell (clamped queries: the
    faces left are the far ones).  So every point is at least r h - margin away; one more margin covers the rounding of b."""
    return grid.max_shell * grid.h - 2.0 * grid.margin


def gate_bound(gate):
    """The radius `correspondences(bounded=True)` asks for at the float32 gate `gate`: gate (1 + 4 eps32), rounded to float32.
    ncw_align_sums admits a pair when sqrtf(d2) <= gate, which implies d2 <= gate^2 (1 + eps)^2; the bound's float32 square is,
    after its two roundings, still >= gate^2 (1 + 5 eps): every pair the sums admit is within the bound."""
    return float(np.float32(float(gate) * (1.0 + 4.0 * evalmesh.F32_EPS)))


def correspondences(q32, inside, target, skip_beyond=None, stats=None, bounded=False, gate=None):
    """(idx [N] int64, dist [N] float32): the nearest target point of every inside query (exact, ties to the smaller index);
    idx = -1 and dist = +inf for the others, which are not queried.
    skip_beyond (a gate, or None): the queries that `NNGrid` would hand to its brute-force pass over the whole cloud are left at
    idx = -1 / dist = +inf instead when the gate is below `far_reach(grid)`: they have no partner within the gate, so the pairs,
    the sums and the matrix are the same bits, and only the idx / dist reported for sources that take no part differ.  The
    grid kernels are NNGrid.query's, called in its order; stats (dict) gets `escaped` and `skipped_far`.
    bounded=True (with `gate`, the float32 gate of the iteration; skip_beyond is not read): the inside queries go to
    `NNGrid.query_within` at `gate_bound(gate)` -- one launch, no escape list and no brute-force pass at ANY gate.  A query
    with no target point within the bound is left at idx = -1 / dist = +inf; every pair within the gate has the idx and the
    dist bits of the unbounded query.  stats gets `beyond` (those left at -1); `escaped` and `skipped_far` stay 0."""
    n = int(q32.shape[0])
    idx = torch.full((n,), -1, dtype=torch.int64, device=q32.device)
    dist = torch.full((n,), float("inf"), dtype=torch.float32, device=q32.device)
    sel = torch.nonzero(inside, as_tuple=False).reshape(-1)
    if not sel.numel():
        return idx, dist
    q = q32.index_select(0, sel).contiguous()
    g = target.grid
    if bounded:
        if gate is None:
            raise ValueError("align.correspondences: bounded=True needs the gate")
        d, i = g.query_within(q, gate_bound(gate), stats)
        idx[sel], dist[sel] = i, d
        return idx, dist
    if skip_beyond is None or not (float(skip_beyond) < far_reach(g)):
        d, i = g.query(q, stats)
        idx[sel], dist[sel] = i, d
        return idx, dist
    lib, k, s = L.get_lib(), int(q.shape[0]), L.stream_ptr(q.device)
    d = torch.full((k,), float("inf"), dtype=torch.float32, device=q.device)   # an escaped query is left unwritten: stays +inf / -1
    i = torch.full((k,), -1, dtype=torch.int64, device=q.device)
    keys = torch.empty(k, dtype=torch.int32, device=q.device)
    L.check(lib.ncw_nn_cell_keys(L.ptr(q), k, C.byref(g.cgrid), L.ptr(keys), s), "ncw_nn_cell_keys")
    q_order = torch.sort(keys, stable=True)[1].contiguous()
    escaped = torch.empty(k, dtype=torch.int32, device=q.device)
    n_esc = torch.zeros(1, dtype=torch.int32, device=q.device)
    L.check(lib.ncw_nn_query(L.ptr(g.pts), L.ptr(g.range), L.ptr(q), L.ptr(q_order), k, C.byref(g.cgrid), g.max_shell, float(g.margin),
                             L.ptr(d), L.ptr(i), L.ptr(escaped), L.ptr(n_esc), s), "ncw_nn_query")
    if stats is not None:
        ne = int(n_esc.item())
        stats["escaped"] = stats.get("escaped", 0) + ne
        stats["skipped_far"] = stats.get("skipped_far", 0) + ne
    idx[sel], dist[sel] = i, d
    return idx, dist


def correspondence_sums(src, cp, target, idx, dist, gate, T):
    """`ncw_align_sums`: (sums [20] float64, counts [2] int64) as device tensors; cq = target.centre."""
    lib = L.get_lib()
    n = int(src.shape[0])
    nb = int(lib.ncw_align_sums_blocks(n))
    part = torch.empty(max(nb, 1), L.ALIGN_SUMS, dtype=torch.float64, device=src.device)
    ipart = torch.empty(max(nb, 1), 2, dtype=torch.int64, device=src.device)
    sums = torch.empty(L.ALIGN_SUMS, dtype=torch.float64, device=src.device)
    counts = torch.empty(2, dtype=torch.int64, device=src.device)
    T = np.asarray(T, dtype=np.float64)
    L.check(lib.ncw_align_sums(L.ptr(src), n, _f64x(cp), L.ptr(target.points), target.m, _f64x(target.centre), L.ptr(idx.contiguous()),
                               L.ptr(dist.contiguous()), float(gate), _f64x(T[:3].reshape(-1)), L.ptr(part), L.ptr(ipart), L.ptr(sums),
                               L.ptr(counts), L.stream_ptr(src.device)), "ncw_align_sums")
    return sums, counts


def default_min_pairs(n):
    return max(3, int(np.ceil(MIN_PAIRS_SHARE * n)))


@torch.no_grad()
def icp_similarity(src, target, init, gate0=None, shrink=0.85, gate_min=None, max_iter=60, with_scale=True, min_pairs=None,
                   stats=None, skip_far=False, bounded=False):
    """Refines the 4x4 `init` so that it carries `src` [N,3] (a GPU tensor, or numpy moved to the target's device) onto `target`
    (AlignTarget).  Per iteration k with matrix T_k and gate g_k: transform, compact, NNGrid.query, sums over the pairs with
    dist <= g_k, T_{k+1} = the similarity of those pairs, g_{k+1} = max(g_k shrink, gate_min).  Stops when T_{k+1} equals T_k bit
    for bit, or after max_iter solves.  Raises ValueError when fewer than `min_pairs` pairs lie within the gate (default
    max(3, 10 % of the source): the initial matrix is too far off).  Defaults from the data: gate0 = 0.2 x the longest edge of
    the target's box, gate_min = 4 x target.spacing().  The gates are rounded to float32 (what the kernels compare against).
    skip_far=True does not send a query that the grid cannot resolve to the brute-force pass once the gate is below
    `far_reach` (see `correspondences`): the same pairs, sums and matrices bit for bit, idx = -1 for those sources.
    bounded=True asks `NNGrid.query_within` at a bound just above the gate (`gate_bound`) in EVERY iteration, also while the gate
    is above `far_reach`, so no iteration runs the brute-force pass (skip_far is then not read).  The matrix, and every
    iteration's pairs, rms and matrix, are the same bits as without it; in the history `escaped` and `skipped_far` read 0 and
    `beyond` counts the inside sources left at idx = -1 (no target point within the bound); idx differs from the plain run
    only on sources outside the mask, and only towards -1.
    Returns the 4x4 float64 matrix.  stats (dict) gets gate0 / gate_min / shrink / min_pairs, `iterations` (the solves made),
    `converged`, `history` (per iteration: gate, pairs, rms and max residual under T_k, mean pair distance, the matrix T_{k+1})
    and the last iteration's `idx` / `mask` (device tensors); with stats["keep_pairs"] set, every iteration's idx / mask as numpy
    in its history entry."""
    if not isinstance(target, AlignTarget):
        raise TypeError("icp_similarity: target must be an AlignTarget")
    src = _gpu_points(src, target.dev, "icp_similarity")
    n = int(src.shape[0])
    T = np.array(init, dtype=np.float64).reshape(4, 4)
    gate0 = DEFAULT_GATE0 * target.longest_edge if gate0 is None else float(gate0)
    if gate0 > target.gate_max * (1 + 1e-6):
        raise ValueError("gate0 %g exceeds the AlignTarget's gate_max %g: build the target with gate_max >= gate0" % (gate0, target.gate_max))
    gate_min = DEFAULT_GATE_MIN * target.spacing() if gate_min is None else float(gate_min)
    min_pairs = default_min_pairs(n) if min_pairs is None else int(min_pairs)
    if not (0 < shrink <= 1 and gate0 > 0 and gate_min >= 0):
        raise ValueError("icp_similarity: gate0 > 0, gate_min >= 0 and 0 < shrink <= 1 are required")
    cp = src.cpu().numpy().mean(0) if n else np.zeros(3)  # any fixed point near the source conditions the sums: numpy's mean, once
    gate = float(np.float32(gate0))
    history, converged, idx, mask = [], False, None, None
    keep = bool(stats is not None and stats.get("keep_pairs"))
    for _ in range(int(max_iter)):
        q32, inside = transform_points(src, T, target, gate)
        qst = {}
        idx, dist = correspondences(q32, inside, target, gate if skip_far else None, qst, bounded=bounded, gate=gate)
        sums, counts = correspondence_sums(src, cp, target, idx, dist, gate, T)
        s, c = sums.cpu().numpy(), counts.cpu().numpy()  # the read-back: 22 numbers
        pairs = int(c[0])
        if pairs < max(min_pairs, 3):
            raise ValueError("only %d of %d source points have a partner within the gate %g at iteration %d (min_pairs %d): the "
                             "initial matrix is too far off for a local method" % (pairs, n, gate, len(history), min_pairs))
        T_new = similarity_from_sums(pairs, s, cp, target.centre, with_scale)
        mask = (idx >= 0) & (dist <= gate)
        entry = {"gate": gate, "pairs": pairs, "rms": float(np.sqrt(s[17] / pairs)),
                 "max_residual": float(np.sqrt(np.array(c[1], dtype=np.int64).view(np.float64))),
                 "mean_distance": float(s[18] / pairs), "matrix": T_new.tolist(), "escaped": qst.get("escaped", 0),
                 "skipped_far": qst.get("skipped_far", 0), "beyond": qst.get("beyond", 0)}
        if keep:
            entry["idx"], entry["mask"] = idx.cpu().numpy(), mask.cpu().numpy()
        history.append(entry)
        same = np.array_equal(T_new, T)
        T = T_new
        if same:
            converged = True
            break
        gate = float(np.float32(max(gate * shrink, gate_min)))
    if stats is not None:
        stats.update(gate0=float(np.float32(gate0)), gate_min=float(gate_min), shrink=float(shrink), min_pairs=min_pairs,
                     max_iter=int(max_iter), iterations=len(history), converged=converged, history=history, idx=idx, mask=mask,
                     source_points=n)
    return T


def _read_matrix(path):
    """4x4 from a text file of 16 (or 12: 3x4) numbers, a .npy, or a yaml / json file holding `sfm2gt` or a bare matrix."""
    if path.endswith(".npy"):
        m = np.load(path)
    elif path.endswith((".yaml", ".yml", ".json")):
        import yaml

        with open(path, "r") as fh:
            doc = yaml.safe_load(fh)
        m = np.array(doc["sfm2gt"] if isinstance(doc, dict) else doc, dtype=np.float64)
    else:
        m = np.loadtxt(path, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    if m.size == 12:
        m = np.concatenate([m, [0.0, 0.0, 0.0, 1.0]])
    if m.size != 16:
        raise ValueError("%s holds %d numbers, not a 3x4 or 4x4 matrix" % (path, m.size))
    return m.reshape(4, 4)


def initial_matrix(data_dir, init="config", pairs=None, with_scale=True):
    """The matrix the loop starts from: `pairs` ([K,6] rows x y z X Y Z, K >= 3: solved by similarity_from_pairs) wins; else
    init = "config" (sfm2gt of <data_dir>/config.yaml), "identity", a path (see _read_matrix) or a 4x4."""
    if pairs is not None:
        pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 6)
        return similarity_from_pairs(pairs[:, :3], pairs[:, 3:], with_scale)
    if isinstance(init, str):
        if init == "identity":
            return np.eye(4)
        if init == "config":
            return _read_matrix(os.path.join(data_dir, "config.yaml"))
        return _read_matrix(init)
    return np.array(init, dtype=np.float64).reshape(4, 4)


def estimate_sfm2gt(data_dir, gt_pcd_path, sfm_path="dense/sparse", init="config", pairs=None, track_length=8, reproj_error=1.0,
                    device="cuda:0", **icp):
    """sfm2gt of the scene `data_dir`: the COLMAP points of <data_dir>/<sfm_path> with a track longer than `track_length` and a
    mean reprojection error below `reproj_error` (evalmesh.read_points3d_filtered), aligned to the cloud `gt_pcd_path`
    (ply.read_points) by `icp_similarity` from `initial_matrix(data_dir, init, pairs)`; **icp are icp_similarity's options.
    Returns (4x4 float64, report).  report: initial_matrix, matrix, correction (matrix inv(initial): scale, rotation_deg,
    translation), iterations, converged, source_points, pairs, inlier_share, rms, max_residual, gate0 / gate_min / shrink /
    min_pairs / with_scale, matched_bbx (the GT-frame box of the matched GT points: a suggestion for eval_bbx), history.
    `bounded` defaults to True here (icp_similarity's own default stays False): the matrix, sfm2gt.yaml and every iteration's
    pairs, rms and matrix are the same bits as with bounded=False; in the report's history `escaped` and `skipped_far` read 0
    and `beyond` counts the sources left at idx = -1."""
    src = evalmesh.read_points3d_filtered(os.path.join(data_dir, sfm_path), track_length, reproj_error)
    if src.shape[0] < 3:
        raise ValueError("%d SfM points pass track_length > %s and reproj_error < %s" % (src.shape[0], track_length, reproj_error))
    gt = ply.read_points(gt_pcd_path)
    T0 = initial_matrix(data_dir, init, pairs, icp.get("with_scale", True))
    target = AlignTarget(gt, device, gate_max=icp.get("gate0"))
    st = {}
    icp.setdefault("skip_far", True)  # the matrix and the report are the same bits either way; only unpaired sources' idx differ
    # the radius-bounded query: the same matrix and the same pairs, rms and matrix in every iteration, and no brute-force pass at
    # the early gates (profiles/align/README.md: faster at every gate measured); the history then reports `beyond`
    icp.setdefault("bounded", True)
    T = icp_similarity(src, target, T0, stats=st, **icp)
    last = st["history"][-1]
    matched = target.points[st["idx"][st["mask"]]]
    scale, angle, shift = decompose_similarity(T @ np.linalg.inv(T0))
    history = [{k: v for k, v in h.items() if k not in ("idx", "mask")} for h in st["history"]]
    report = {"initial_matrix": T0.tolist(), "matrix": T.tolist(),
              "correction": {"scale": scale, "rotation_deg": angle, "translation": shift},
              "iterations": st["iterations"], "converged": st["converged"], "source_points": st["source_points"],
              "target_points": target.m, "pairs": last["pairs"], "inlier_share": last["pairs"] / float(st["source_points"]),
              "rms": last["rms"], "max_residual": last["max_residual"], "gate0": st["gate0"], "gate_min": st["gate_min"],
              "shrink": st["shrink"], "min_pairs": st["min_pairs"], "with_scale": bool(icp.get("with_scale", True)),
              "track_length": track_length, "reproj_error": reproj_error,
              "matched_bbx": [matched.amin(0).cpu().tolist(), matched.amax(0).cpu().tolist()], "history": history}
    return T, report
