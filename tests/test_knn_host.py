"""Host side of the k-NN grid walk and the cloud operations on it (csrc/ncw_knn.hip, evalmesh.NNGrid.query_k, evalmesh.knn,
cloudops): the binding, the refusals that need no GPU, the command lines, and -- in numpy -- that the restatements of
tests/_knn_ref.py, to which the GPU tests hold the kernels bit for bit, are themselves right against independent references."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import _knn_ref as K
from tests import _nn_within_cases as W
from tests._util import ROOT

from neuralrecon_w_amd import evalmesh
from neuralrecon_w_amd import lib as L

KS = (1, 8, 16, 32)


def _script(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        return __import__(name)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))


# ---------------------------------------------------------------------------------------------------
# binding, refusals, command lines
# ---------------------------------------------------------------------------------------------------
def test_binding_and_header_declare_the_entry_points():
    assert {"ncw_knn_query", "ncw_knn_pca"} <= set(L.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "neuconw_hip.h")).read()
    assert "int ncw_knn_query(" in hdr and "int ncw_knn_pca(" in hdr
    assert L.ABI_VERSION >= 38


@pytest.mark.parametrize("k", [0, -1, 33, 2.5, None])
def test_k_outside_1_to_32_is_refused(k):
    from neuralrecon_w_amd import cloudops

    grid = evalmesh.NNGrid.__new__(evalmesh.NNGrid)  # the check comes before anything of the grid is read
    pts = torch.zeros(40, 3)
    with pytest.raises(ValueError):
        grid.query_k(pts, k)
    with pytest.raises(ValueError):
        evalmesh.knn(pts, pts, k)
    with pytest.raises(ValueError):
        cloudops.estimate_normals(pts, k=k)
    with pytest.raises(ValueError):
        cloudops.remove_statistical_outliers(pts, k=k)


@pytest.mark.parametrize("bad", [0, -1, float("nan")])
def test_max_dist_must_be_positive(bad):
    from neuralrecon_w_amd import cloudops

    grid = evalmesh.NNGrid.__new__(evalmesh.NNGrid)
    pts = torch.zeros(4, 3)
    with pytest.raises(ValueError):
        grid.query_k(pts, 4, max_dist=bad)
    with pytest.raises(ValueError):
        evalmesh.knn(pts, pts, 4, max_dist=bad)
    with pytest.raises(ValueError):
        cloudops.estimate_normals(pts, k=4, max_dist=bad)


def test_cpu_tensors_raise():
    from neuralrecon_w_amd import cloudops

    grid = evalmesh.NNGrid.__new__(evalmesh.NNGrid)
    pts = torch.zeros(40, 3)
    with pytest.raises(L.NeuconwHipError):
        grid.query_k(pts, 4)
    with pytest.raises(L.NeuconwHipError):
        evalmesh.knn(pts, pts, 4, max_dist=1.0)
    with pytest.raises(L.NeuconwHipError):
        cloudops.estimate_normals(pts, k=4)
    with pytest.raises(L.NeuconwHipError):
        cloudops.remove_statistical_outliers(pts, k=4)


def test_eval_mesh_refuses_normals_with_exact_recall_before_any_work(tmp_path):
    with pytest.raises(ValueError):
        evalmesh.eval_mesh(str(tmp_path / "none.ply"), str(tmp_path / "none_gt.ply"), {}, True, exact_recall=True, normals=16)
    with pytest.raises(ValueError):
        evalmesh.eval_mesh(str(tmp_path / "none.ply"), str(tmp_path / "none_gt.ply"), {}, True, normals=40)
    assert not os.listdir(str(tmp_path))


def test_command_lines_parse():
    em = _script("eval_mesh")
    base = ["--file_pred", "p.ply", "--file_trgt", "g.ply", "--scene_config_path", "c.yaml"]
    assert em.get_opts(base).normal_consistency is None
    assert em.get_opts(base + ["--normal_consistency"]).normal_consistency == 16
    assert em.get_opts(base + ["--normal_consistency", "8"]).normal_consistency == 8
    cc = _script("clean_cloud")
    a = cc.build_parser().parse_args(["--file_in", "a.ply", "--file_out", "b.ply"])
    assert (a.outlier_k, a.outlier_ratio, a.normals_k, a.toward) == (16, 2.0, 16, None)
    a = cc.build_parser().parse_args(["--file_in", "a.ply", "--file_out", "b.ply", "--outlier_k", "8", "--outlier_ratio", "1.5",
                                      "--normals_k", "12", "--toward", "1,-2.5,3"])
    assert (a.outlier_k, a.outlier_ratio, a.normals_k, a.toward) == (8, 1.5, 12, [1.0, -2.5, 3.0])


# ---------------------------------------------------------------------------------------------------
# knn32 against an independent float64 brute force
# ---------------------------------------------------------------------------------------------------
def _dist64(P, Q):
    return np.sqrt(((Q[:, None, :] - P[None, :, :]) ** 2).sum(-1))


@pytest.mark.parametrize("name", W.NAMES)
def test_knn32_against_float64_brute_force(name):
    c = W.case(name)
    P, Q = c["P"], c["Q"]
    b = W.bound(P, Q)
    (p32, q32), _ = K.recentre32(P, Q)
    D = _dist64(P, Q)
    Ds = np.sort(np.partition(D, 33, axis=1)[:, :34], axis=1)        # the 34 smallest float64 distances of every query
    d2 = K.d2_matrix(p32, q32)
    rows = np.arange(Q.shape[0])[:, None]
    for k in KS:
        dist, idx, count = K.knn32(p32, q32, k, d2=d2)
        assert (count == k).all() and dist.dtype == np.float32 and idx.dtype == np.int32
        assert (np.abs(dist.astype(np.float64) - Ds[:, :k]) <= b).all()                  # every rank, no query left out
        assert (np.abs(D[rows, idx] - dist) <= b).all()                                  # every index's own distance
        assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all() if k > 1 else True      # distinct
        assert (np.diff(dist, axis=1) >= 0).all() if k > 1 else True
        clear = Ds[:, k] - Ds[:, k - 1] > 2 * b
        want = np.sort(np.argpartition(D, k - 1, axis=1)[:, :k], axis=1)
        assert (np.sort(idx, axis=1)[clear] == want[clear]).all()
        print("%s k = %d: %.2f %% of the queries unclear" % (name, k, 100.0 * (1 - clear.mean())))
        assert clear.mean() >= 0.97, (name, k, clear.mean())
    for R in c["radii"]:
        dist, idx, count = K.knn32(p32, q32, 32, r=R, d2=d2)
        lo = np.minimum((D < R - b).sum(1), 32)
        hi = np.minimum((D <= R + b).sum(1), 32)
        assert ((lo <= count) & (count <= hi)).all(), (name, R)
        assert (np.isinf(dist) == (idx < 0)).all() and ((idx >= 0).sum(1) == count).all()
        inside = idx >= 0
        assert (D[rows, np.where(inside, idx, 0)][inside] <= R + b).all()


@pytest.mark.parametrize("k", [8, 32])
@pytest.mark.parametrize("R", [None, 3.0])
def test_knn32_on_the_lattice_follows_the_d2_index_rule(k, R):
    """Every d2 is an exact float32, so the rows must equal np.lexsort on the exact integers: the (d2, index) rule decides."""
    P, Q, _, _ = W.lattice_case()
    (p32, q32), _ = K.recentre32(P, Q)
    dd = ((Q[:, None, :] - P[None, :, :]) ** 2).sum(-1)               # exact (multiples of 0.25)
    assert (K.d2_matrix(p32, q32).astype(np.float64) == dd).all()
    dist, idx, count = K.knn32(p32, q32, k, r=np.inf if R is None else R)
    ids = np.arange(P.shape[0])
    ties = 0
    for j in range(Q.shape[0]):
        order = np.lexsort((ids, dd[j]))
        if R is not None:
            order = order[dd[j][order] <= R * R]                      # d2 = 9 is inclusive
        want = order[:k]
        assert count[j] == want.size and (idx[j, :want.size] == want).all() and (idx[j, want.size:] == -1).all()
        assert (dist[j, :want.size] == np.sqrt(dd[j][want]).astype(np.float32)).all()
        if order.size > k:
            ties += dd[j][order[k - 1]] == dd[j][order[k]]
    if R is None and k == 8:
        assert ties >= 0.5 * Q.shape[0], ties                         # half of the queries have a tie at the boundary
    if R is not None:
        assert (dd == 9.0).any() and (count < k).any() and (count > 0).any()


def test_knn32_nan_inf_exclude_and_short_rows():
    rng = np.random.RandomState(2)
    P = rng.uniform(-1, 1, (5, 3)).astype(np.float32)
    P[4] = P[1]                                                      # a duplicate
    Q = P.copy()
    dist, idx, count = K.knn32(P, Q, 8, exclude=np.arange(5))
    assert (count == 4).all() and (idx[:, 4:] == -1).all() and np.isinf(dist[:, 4:]).all()
    assert not (idx == np.arange(5)[:, None]).any()
    assert idx[1, 0] == 4 and dist[1, 0] == 0 and idx[4, 0] == 1       # the duplicate stays at d = 0
    Q[0, 1], Q[2, 0] = np.nan, np.inf
    dist, idx, count = K.knn32(P, Q, 3)
    assert count[0] == 0 and count[2] == 0 and (idx[0] == -1).all() and (count[[1, 3, 4]] == 3).all()


# ---------------------------------------------------------------------------------------------------
# pca_ref against numpy.linalg.eigh; outliers_ref on its fixture
# ---------------------------------------------------------------------------------------------------
def plane_patch(n=2000, sigma=0.002, seed=5):
    """A noisy patch of the plane through the origin with normal (1, 2, 2) / 3, mean spacing about 1 / sqrt(n)."""
    rng = np.random.RandomState(seed)
    nrm = np.array([1.0, 2.0, 2.0]) / 3.0
    u = np.cross(nrm, [1.0, 0, 0])
    u /= np.linalg.norm(u)
    v = np.cross(nrm, u)
    ab = rng.uniform(0, 1, (n, 2))
    return ab[:, :1] * u + ab[:, 1:] * v + rng.randn(n, 1) * sigma * nrm, nrm


def test_pca_ref_against_eigh():
    """Davis-Kahan: sin(angle) <= 2 |E| / gap with |E| of order k eps64 l2 is about 1e-13 at a gap of 0.06 l2, so 1e-9 rad leaves
    four orders.  The angle is taken on the float64 eigenvector, as its sine (the cross product; acos cannot resolve 1e-9);
    the float32 normal is that vector cast."""
    P, _ = plane_patch()
    (p32,), _ = K.recentre32(P)
    _, idx, count = K.knn32(p32, p32, 16, exclude=np.arange(p32.shape[0]))
    normal, eig, curv, valid, normal64 = K.pca_ref(p32, p32, idx, count, with_query=True, return_normal64=True)
    assert valid.all() and normal.dtype == np.float32 and eig.dtype == np.float64
    assert (normal == normal64.astype(np.float32)).all()
    assert (np.abs(np.linalg.norm(normal64, axis=1) - 1) <= 4e-16).all()
    assert (np.diff(eig, axis=1) >= 0).all()
    p64 = p32.astype(np.float64)
    worst_sin, worst_eig, min_gap = 0.0, 0.0, np.inf
    for j in range(p32.shape[0]):
        mem = np.concatenate([p64[j:j + 1], p64[idx[j]]])
        w, v = np.linalg.eigh(np.cov(mem.T, bias=True))
        min_gap = min(min_gap, (w[1] - w[0]) / w[2])
        worst_eig = max(worst_eig, np.abs(eig[j] - w).max() / w[2])
        worst_sin = max(worst_sin, float(np.linalg.norm(np.cross(normal64[j], v[:, 0]))))
        assert abs(float(curv[j]) - w[0] / w.sum()) <= 1e-7
    print("pca_ref vs eigh: sin(angle) %.3g, eigenvalues %.3g l2, smallest gap %.3g l2" % (worst_sin, worst_eig, min_gap))
    assert min_gap >= 0.06
    assert worst_eig <= 1e-12
    assert worst_sin <= 1e-9


def test_pca_ref_sign_rule_and_invalid_sets():
    P, nrm = plane_patch()
    (p32,), centre = K.recentre32(P)
    _, idx, count = K.knn32(p32, p32, 16, exclude=np.arange(p32.shape[0]))
    normal = K.pca_ref(p32, p32, idx, count)[0]
    big = np.abs(normal).argmax(1)
    assert (normal[np.arange(normal.shape[0]), big] > 0).all()        # the component of largest magnitude is positive
    assert (np.abs(normal.astype(np.float64) @ nrm) > 0.95).all()
    for view in (nrm * 5.0, -nrm * 5.0):
        tw = view - centre
        n2 = K.pca_ref(p32, p32, idx, count, toward=tw)[0]
        assert ((n2.astype(np.float64) * (tw.astype(np.float32).astype(np.float64) - p32)).sum(1) >= 0).all()
        assert (np.abs(n2) == np.abs(normal)).all()                  # the sign alone differs
        assert (np.sign(n2.astype(np.float64) @ nrm) == np.sign(view @ nrm)).all()
    # collinear members, coincident members, two members, none
    line = (np.arange(6, dtype=np.float32)[:, None] * np.array([[0.5, 0.25, -1.0]], dtype=np.float32))
    ii = np.tile(np.arange(1, 6, dtype=np.int32), (1, 1))
    n, e, cv, ok = K.pca_ref(line[:1], line, ii, np.array([5]))
    assert not ok[0] and (n == 0).all() and e[0, 2] > 0 and e[0, 1] <= 1e-10 * e[0, 2]
    same = np.ones((4, 3), dtype=np.float32)
    n, e, cv, ok = K.pca_ref(same[:1], same, np.array([[1, 2, 3]], dtype=np.int32), np.array([3]))
    assert not ok[0] and (e == 0).all() and cv[0] == 0 and (n == 0).all()
    n, e, cv, ok = K.pca_ref(p32[:1], p32, idx[:1], np.array([1]))    # n = 2
    assert not ok[0] and (n == 0).all() and e[0, 2] > 0
    n, e, cv, ok = K.pca_ref(p32[:1], p32, idx[:1], np.array([2]))    # n = 3: a triangle has a normal
    assert ok[0]
    n, e, cv, ok = K.pca_ref(p32[:1], p32, idx[:1], np.array([0]), with_query=False)
    assert not ok[0] and (e == 0).all() and (n == 0).all() and cv[0] == 0


# ---------------------------------------------------------------------------------------------------
# outliers_ref
# ---------------------------------------------------------------------------------------------------
def outlier_fixture():
    """The 2000-point plane patch plus 40 points on a coarse lattice 30 to 50 mean spacings off the plane: each at least 20
    mean spacings (1 / sqrt(2000)) from every other point."""
    P, nrm = plane_patch()
    sp = 1.0 / np.sqrt(2000.0)
    u = np.cross(nrm, [1.0, 0, 0])
    u /= np.linalg.norm(u)
    v = np.cross(nrm, u)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(5), indexing="ij"), -1).reshape(-1, 2)
    far = (g[:, :1] * u + g[:, 1:] * v) * 25 * sp + (30 + 20 * (g.sum(1) % 2))[:, None] * sp * nrm
    return np.concatenate([P, far]), sp


def test_outliers_ref_drops_the_far_points_and_keeps_the_patch():
    P, sp = outlier_fixture()
    D = _dist64(P, P[2000:])
    D[np.arange(40), 2000 + np.arange(40)] = np.inf
    assert D.min() >= 20 * sp
    keep, m = K.outliers_ref(P, k=16, ratio=2.0)
    assert not keep[2000:].any()
    assert (~keep[:2000]).sum() <= 20
    D = _dist64(P, P[:50])
    D[np.arange(50), np.arange(50)] = np.inf
    assert np.allclose(m[:50], np.sort(D, axis=1)[:, :16].mean(1), rtol=1e-5)
    with pytest.raises(ValueError):
        K.outliers_ref(P[:16], k=16)
