"""GPU: exact 1-NN of the mesh evaluation (csrc/ncw_nn.hip through evalmesh.nn_distances) against a chunked float64 brute
force over the ORIGINAL float64 coordinates, on the distributions that stress a uniform grid: uniform, planar (mostly empty
cells), 1e5 duplicates (the tie rule), queries far outside P's box and far outliers (the escape path), M = 1, empty sides,
non-square extents, coordinates 1e3 m from the origin (the recentring); and one larger case against scipy's cKDTree."""
import numpy as np
import pytest
import torch

from neuralrecon_w_amd import evalmesh

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
DEV = "cuda:0"


def _brute64(P, Q, chunk=1 << 24):
    """(d [N], first argmin [N], runner-up distance [N]) in float64 on the GPU, differences squared (no expansion)."""
    p = torch.from_numpy(P).to(DEV)
    q = torch.from_numpy(Q).to(DEV)
    rows = max(1, chunk // max(1, p.shape[0]))
    d, i, d2nd = [], [], []
    for s in range(0, q.shape[0], rows):
        dd = ((q[s:s + rows, None, :] - p[None, :, :]) ** 2).sum(-1)
        i.append(torch.argmin(dd, 1))  # first index of the minimum
        k = min(2, p.shape[0])
        v = torch.topk(dd, k, 1, largest=False).values
        d.append(v[:, 0].sqrt())
        d2nd.append(v[:, 1].sqrt() if k == 2 else torch.full_like(v[:, 0], float("inf")))
    return torch.cat(d).cpu().numpy(), torch.cat(i).cpu().numpy(), torch.cat(d2nd).cpu().numpy()


def _bound(P, Q):
    both = np.concatenate([P, Q])
    c = (both.min(0) + both.max(0)) / 2
    return 8 * EPS32 * float(np.abs(both - c).max())


def _check(P, Q, expect_escape=None):
    st = {}
    d, i = evalmesh.nn_distances(torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV), stats=st)
    assert d.dtype == torch.float32 and i.dtype == torch.int64 and d.shape == (Q.shape[0],) and i.shape == (Q.shape[0],)
    d2, i2 = evalmesh.nn_distances(torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV))
    assert torch.equal(d, d2) and torch.equal(i, i2), "repeated calls differ"
    d, i = d.double().cpu().numpy(), i.cpu().numpy()
    e, ei, e2 = _brute64(P, Q)
    b = _bound(P, Q)
    err = np.abs(d - e)
    assert err.max() <= b, (err.max(), b)
    clear = e2 - e > b
    assert (i[clear] == ei[clear]).all(), int((i[clear] != ei[clear]).sum())
    # where the runner-up is within the bound the returned point must still be one of the nearest within it
    dd = np.linalg.norm(P[i] - Q, axis=1)
    assert (dd <= e + 2 * b).all()
    if expect_escape is not None:
        assert (st["escaped"] > 0) == expect_escape, st
    return st


def test_uniform():
    rng = np.random.RandomState(0)
    _check(rng.uniform(-1, 1, (20000, 3)), rng.uniform(-1, 1, (30000, 3)))


def test_plane_surface_like():
    rng = np.random.RandomState(1)
    P = np.c_[rng.uniform(-5, 5, (50000, 2)), np.zeros(50000)]
    Q = np.c_[rng.uniform(-5, 5, (20000, 2)), rng.randn(20000) * 0.01]
    st = _check(P, Q)
    assert st["cells"] > 1


def test_duplicates_tie_to_the_first_index():
    rng = np.random.RandomState(2)
    X = np.array([0.3, -0.2, 0.1])
    P = np.concatenate([rng.uniform(-1, 1, (50, 3)) * 5 + 20, np.repeat(X[None], 100000, 0), rng.uniform(-1, 1, (50, 3)) * 5 + 20])
    Q = X + rng.randn(500, 3) * 1e-2
    d, i = evalmesh.nn_distances(torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV))
    assert (i.cpu().numpy() == 50).all()  # the first of the 1e5 copies
    _check(P, Q)


def test_far_queries_and_outliers_take_the_escape_path():
    rng = np.random.RandomState(3)
    d = rng.randn(20000, 3)
    P = d / np.linalg.norm(d, axis=1, keepdims=True)
    Q = np.concatenate([P[:5000] + rng.randn(5000, 3) * 1e-3, rng.uniform(-1, 1, (200, 3)) + [1000.0, 0, 0],
                        rng.randn(20, 3) * 300.0])
    _check(P, Q, expect_escape=True)


def test_single_point_and_empty_sides():
    rng = np.random.RandomState(4)
    _check(np.array([[0.5, -1.0, 2.0]]), rng.uniform(-3, 3, (1000, 3)))
    _check(rng.uniform(-3, 3, (1000, 3)), np.array([[0.5, -1.0, 2.0]]))
    for P, Q in ((np.zeros((0, 3)), rng.rand(10, 3)), (rng.rand(10, 3), np.zeros((0, 3))), (np.zeros((0, 3)), np.zeros((0, 3)))):
        d, i = evalmesh.nn_distances(torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV))
        assert d.shape == (0,) and i.shape == (0,)


def test_non_square_extents():
    rng = np.random.RandomState(5)
    P = rng.uniform(0, 1, (40000, 3)) * [100.0, 1.0, 0.01]
    Q = rng.uniform(0, 1, (20000, 3)) * [100.0, 1.0, 0.01]
    _check(P, Q)


def test_offset_coordinates_are_recentred():
    rng = np.random.RandomState(6)
    off = np.array([1000.0, -2000.0, 1500.0])
    P = rng.uniform(-1, 1, (20000, 3)) + off
    Q = rng.uniform(-1, 1, (20000, 3)) + off
    _check(P, Q)
    assert _bound(P, Q) < 1e-5  # the bound is set by the recentred coordinates, not by the 1e3 m offset


@pytest.mark.slow
def test_large_against_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.RandomState(7)
    d = rng.randn(1000000, 3)
    r = 10 * (1 + 0.1 * np.sin(3 * d[:, 0] / np.linalg.norm(d, axis=1)))
    P = d / np.linalg.norm(d, axis=1, keepdims=True) * r[:, None] + rng.randn(1000000, 3) * 1e-3
    Q = P[rng.choice(1000000, 200000, replace=False)] + rng.randn(200000, 3) * 0.02
    dist, idx = evalmesh.nn_distances(torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV))
    kd, ki = spatial.cKDTree(P).query(Q, k=1, workers=16)
    assert np.abs(dist.double().cpu().numpy() - kd).max() <= _bound(P, Q)
    assert (idx.cpu().numpy() == ki).mean() > 0.999
