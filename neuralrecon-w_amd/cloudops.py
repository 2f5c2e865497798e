"""What a point cloud needs before it is scored or shown, on the exact k-NN grid of csrc/ncw_knn.hip: normals from the PCA of
every point's neighbourhood, statistical outlier removal, and the normal consistency of two oriented clouds.

No parity is claimed with open3d (`estimate_normals`, `remove_statistical_outlier`), whose source is not at hand: the
neighbourhoods here are the exact k nearest OTHER points plus the point itself, ties to the smaller index; open3d's
KD-tree returns the point itself among its k and resolves ties in tree order.  Normals are unoriented by nature: the sign
rule below is a convention, nothing propagates orientation over the cloud.
"""
import ctypes as C

import numpy as np
import torch

from . import evalmesh
from . import lib as L


def _need_gpu(what, *tensors):
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise L.NeuconwHipError("cloudops.%s: the cloud is not on a GPU; there is no CPU fallback" % what)


@torch.no_grad()
def pca(pts32, ref32, idx, count, with_query=True, toward=None):
    """`ncw_knn_pca`: per point of pts32 [N,3] f32 the PCA of its members -- itself first when `with_query`, then
    ref32[idx[j, :count[j]]] in list order -- in float64 with a fixed operation sequence.  Returns (normal [N,3] f32,
    eig [N,3] f64 ascending, curvature [N] f32, valid [N] bool).  valid = at least 3 members and l1 > 1e-10 l2; an invalid
    point has a zero normal.  `toward` (3 numbers in the coordinates of pts32, or None): the normal is flipped to face it;
    without one its component of largest magnitude is made positive."""
    _need_gpu("pca", pts32, ref32, idx, count)
    n, k = int(idx.shape[0]), int(idx.shape[1])
    dev = pts32.device
    pts32, ref32 = pts32.float().contiguous(), ref32.float().contiguous()
    idx, count = idx.to(torch.int32).contiguous(), count.to(torch.int32).contiguous()
    normal = torch.empty(n, 3, dtype=torch.float32, device=dev)
    eig = torch.empty(n, 3, dtype=torch.float64, device=dev)
    curv = torch.empty(n, dtype=torch.float32, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    tw = None if toward is None else (C.c_float * 3)(*[float(np.float32(v)) for v in toward])
    L.check(L.get_lib().ncw_knn_pca(L.ptr(pts32), L.ptr(ref32), int(ref32.shape[0]), L.ptr(idx), L.ptr(count), n, k,
                                    1 if with_query else 0, tw, L.ptr(normal), L.ptr(eig), L.ptr(curv), L.ptr(valid),
                                    L.stream_ptr(dev)), "ncw_knn_pca")
    return normal, eig, curv, valid.bool()


@torch.no_grad()
def estimate_normals(points, k=16, toward=None, max_dist=None):
    """(normals [N,3] f32, curvature [N] f32, valid [N] bool) of a cloud [N,3] on the GPU: every point's members are itself
    and its k nearest OTHER points (within `max_dist`, if given); the normal is the eigenvector of the smallest eigenvalue
    of their covariance, curvature = l0 / (l0 + l1 + l2).  `toward` (x, y, z in the cloud's coordinates): normals face that
    viewpoint; otherwise the component of largest magnitude is positive.  Points whose members are collinear, coincident or
    fewer than 3 are invalid and get a zero normal.  ValueError unless 1 <= k <= 32 and max_dist > 0."""
    evalmesh._check_k("cloudops.estimate_normals", k, max_dist)
    _need_gpu("estimate_normals", points)
    points = points.reshape(-1, 3)
    n = int(points.shape[0])
    if n == 0:
        dev = points.device
        return (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
                torch.zeros(0, dtype=torch.bool, device=dev))
    p32, _, cmax, centre = evalmesh.recentre(points, points)
    grid = evalmesh.NNGrid(p32, cmax)
    own = torch.arange(n, dtype=torch.int32, device=points.device)
    _, idx, count = grid.query_k(p32, k, max_dist=max_dist, exclude=own)
    tw = None if toward is None else (np.asarray(toward, dtype=np.float64).reshape(3) - centre)
    normal, _, curv, valid = pca(p32, p32, idx, count, with_query=True, toward=tw)
    return normal, curv, valid


@torch.no_grad()
def remove_statistical_outliers(points, k=16, ratio=2.0):
    """(keep [N] bool, mean_dist [N] f64): m_i = the mean distance of point i to its k nearest other points; with mu and
    sigma the float64 mean and population standard deviation of m, keep = m <= mu + ratio * sigma (the rule of open3d's
    `remove_statistical_outlier`; unpinned against it).  ValueError if the cloud has no more than k points."""
    evalmesh._check_k("cloudops.remove_statistical_outliers", k, None)
    _need_gpu("remove_statistical_outliers", points)
    points = points.reshape(-1, 3)
    if int(points.shape[0]) <= int(k):
        raise ValueError("cloudops.remove_statistical_outliers: %d points are no more than k = %d" % (points.shape[0], k))
    dist, _, _ = evalmesh.knn(points, points, k, exclude_self=True)
    m = dist.double().sum(1) / float(k)
    mu = m.mean()
    sigma = m.std(unbiased=False)
    return m <= mu + float(ratio) * sigma, m


@torch.no_grad()
def normal_consistency(n_a, valid_a, n_b, valid_b, idx_ab):
    """(mean of |n_a[i] . n_b[idx_ab[i]]| in float64 over the pairs where both normals are valid, the number of such pairs).
    idx_ab [Na]: for every point of a its partner in b (negative = none).  nan when no pair qualifies."""
    idx_ab = idx_ab.long()
    has = idx_ab >= 0
    j = idx_ab.clamp(min=0)
    ok = valid_a.bool() & has & valid_b.bool()[j]
    dots = (n_a.double() * n_b.double()[j]).sum(1).abs()[ok]
    cnt = int(ok.sum())
    return (float(dots.mean()) if cnt else float("nan")), cnt
