"""The clouds, queries and radii of the radius-bounded 1-NN tests (tests/test_nn_within_host.py checks in numpy that the
reference alone satisfies what the GPU cases rest on; tests/test_gpu_nn_within.py runs them).  numpy only."""
import numpy as np

from neuralrecon_w_amd import evalmesh

EPS32 = float(np.finfo(np.float32).eps)
RADII_H = (0.25, 2.0, 11.0, 40.0)  # x the cell side h; +inf is added by the GPU test (there every query qualifies)
NAMES = ("uniform", "plane", "clusters", "outliers", "outside", "offset")


def bound(P, Q):
    """8 eps32 x the largest recentred |coordinate|: the bound of tests/test_gpu_nn.py."""
    both = np.concatenate([P, Q])
    c = (both.min(0) + both.max(0)) / 2
    return 8 * EPS32 * float(np.abs(both - c).max())


def nominal_grid(P, Q, target_cells):
    """(h, dims) that evalmesh.NNGrid(recentre(P, Q), target_cells=...) gets, restated in numpy (the 0.1 % tails cut off from
    1000 points on; float64 here, float32 there: the radii are multiples of THIS h, whatever the last digits of the other)."""
    both = np.concatenate([P, Q])
    c = (both.min(0) + both.max(0)) / 2
    p = P - c
    if p.shape[0] >= 1000:
        lo, hi = np.quantile(p, 1e-3, axis=0), np.quantile(p, 1 - 1e-3, axis=0)
    else:
        lo, hi = p.min(0), p.max(0)
    return evalmesh._grid_for(list(hi - lo), target_cells)


def _queries(rng, P, h, lo, hi, n_near, n_uni, n_far):
    """Queries of three kinds: jittered copies of points of P (sigma 0.15 h: the small radii have both outcomes), uniform in
    the box [lo, hi], and far ones 45 h to 60 h outside the sphere around that box (beyond every finite radius)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    near = P[rng.choice(P.shape[0], n_near)] + rng.randn(n_near, 3) * 0.15 * h
    uni = rng.uniform(lo, hi, (n_uni, 3))
    d = rng.randn(n_far, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = (lo + hi) / 2 + d * (np.linalg.norm(hi - lo) / 2 + rng.uniform(45, 60, (n_far, 1)) * h)
    return np.concatenate([near, uni, far])


def case(name):
    """dict(P, Q float64, target_cells, h, dims, radii): every grid side is at most 64 cells, so NNGrid(max_shell=64).query
    resolves every query in its shells."""
    rng = np.random.RandomState(NAMES.index(name) + 100)
    if name == "uniform":
        P, tc, lo, hi = rng.uniform(-1, 1, (2000, 3)), 48 ** 3, [-1] * 3, [1] * 3
    elif name == "plane":      # a plane in a box: one layer of cells, queries up to 14 h off it
        P, tc, lo, hi = np.c_[rng.uniform(-5, 5, (3000, 2)), np.zeros(3000)], 48 * 48, [-5, -5, -3], [5, 5, 3]
    elif name == "clusters":   # two clusters more than 50 h apart, queries between them
        P = np.concatenate([rng.randn(800, 3) * 0.03 + [-1, 0, 0], rng.randn(800, 3) * 0.03 + [1, 0, 0]])
        tc, lo, hi = 60 * 6 * 6, [-1, -0.1, -0.1], [1, 0.1, 0.1]
    elif name == "outliers":   # six far points, one beyond each face: inside the 0.1 % tails, clamped into boundary cells
        out = np.concatenate([np.eye(3), -np.eye(3)]) * 30.0 + rng.randn(6, 3) * 0.01
        P, tc, lo, hi = np.concatenate([rng.uniform(-1, 1, (4000, 3)), out]), 48 ** 3, [-1] * 3, [1] * 3
    elif name == "outside":    # queries up to 30 h outside the grid box (h = 2 / 40)
        P, tc, lo, hi = rng.uniform(-1, 1, (2000, 3)), 40 ** 3, [-2.45] * 3, [2.45] * 3
    elif name == "offset":
        off = np.array([1000.0, -2000.0, 1500.0])
        P, tc, lo, hi = rng.uniform(-1, 1, (2000, 3)) + off, 48 ** 3, off - 1, off + 1
    else:
        raise KeyError(name)
    # the queries need h, h needs the common box of P and the queries: one fixed-point step from P's own box is enough,
    # because the box only moves the centre and the cells are sized from P alone
    h, _ = nominal_grid(P, P, tc)
    Q = _queries(rng, P, h, lo, hi, 1000, 1900, 100)
    if name == "outliers":     # and queries next to the clamped outliers: their partner sits in a boundary cell, 700 h away
        Q = np.concatenate([Q, P[-6:].repeat(10, 0) + rng.randn(60, 3) * 0.15 * h])
    h, dims = nominal_grid(P, Q, tc)
    return {"P": P, "Q": Q, "target_cells": tc, "h": h, "dims": dims, "radii": [k * h for k in RADII_H]}


def brute64_numpy(P, Q):
    """(nearest distance [N], first argmin [N]) in float64 on the host, chunked."""
    d, i = np.empty(Q.shape[0]), np.empty(Q.shape[0], dtype=np.int64)
    for s in range(0, Q.shape[0], 512):
        dd = ((Q[s:s + 512, None, :] - P[None, :, :]) ** 2).sum(-1)
        i[s:s + 512] = dd.argmin(1)
        d[s:s + 512] = np.sqrt(dd.min(1))
    return d, i


def lattice_case():
    """The exact-boundary case: P = the integer lattice {0..7}^3 in shuffled order with 64 duplicates appended, Q on
    coordinates from {-4, -3.5, -3, -1, 0, 3, 7, 8, 10, 10.5, 11}: the common box is [-4, 11]^3, its centre 3.5, so every
    recentred coordinate is a multiple of 0.5 and every d^2 an exact float32.  (P, Q, exact d^2 [N] float64, expected index
    [N] = the smallest index at that d^2.)"""
    rng = np.random.RandomState(7)
    g = np.arange(8.0)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    lat = lat[rng.permutation(512)]
    P = np.concatenate([lat, lat[rng.choice(512, 64, replace=False)]])
    v = np.array([-4, -3.5, -3, -1, 0, 3, 7, 8, 10, 10.5, 11.0])
    Q = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    dd = ((Q[:, None, :] - P[None, :, :]) ** 2).sum(-1)
    return P, Q, dd.min(1), dd.argmin(1)
