"""GPU: the reprojection filter's marking with the radius-bounded query (reproj.Target(bounded=True)) against the earlier path
(bounded=False): equal flags on a target whose queries are half beyond the threshold, the threshold itself decided the same
way on exact coordinates, and reprojected.ply byte for byte on the golden scene."""
import os

import numpy as np
import pytest
import torch

from tests._util import GOLDEN

from neuralrecon_w_amd import reproj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR = 0.25


def _case():
    """3000 vertices on multiples of 2^-10 (the corners (-8,-8,-8) and (8,8,8) among them: the centre is the origin, recentring
    changes nothing), vertex A = (6, 0, 0) with a query at exactly THR from it, vertex B = (-6, 0, 0) with a query one float32
    step inside THR; 6000 queries, half of them further than THR from every vertex."""
    rng = np.random.RandomState(21)
    body = np.round(rng.uniform(-4, 4, (2996, 3)) * 1024) / 1024
    xyz = np.concatenate([body, [[-8, -8, -8], [8, 8, 8], [6, 0, 0], [-6, 0, 0]]]).astype(np.float64)
    near = body[rng.choice(2996, 2998)] + rng.randn(2998, 3) * 0.1 * THR
    far = np.c_[rng.uniform(-7.5, 7.5, 3000), rng.uniform(5, 7.5, 3000), rng.uniform(-7.5, 7.5, 3000)]
    at = np.array([[6.25, 0, 0]])
    inside = np.array([[-float(np.nextafter(np.float32(6.25), np.float32(0))), 0, 0]])
    q = np.concatenate([near, far, at, inside]).astype(np.float32)
    return xyz, q


def test_mark_gives_equal_flags_with_and_without_the_bound():
    xyz, q = _case()
    dev = torch.device(DEV)
    q32 = torch.from_numpy(q).to(dev)
    flags = {}
    for bounded in (True, False):
        t = reproj.Target(xyz, None, THR, dev, bounded=bounded)
        assert (t.centre == 0).all() and t.bounded == bounded
        t.mark(q32)
        flags[bounded] = t.flags[: t.m].clone()
    d, _ = t.grid.query(q32)
    assert int((d > THR).sum()) >= 3000 and int((d < THR).sum()) >= 2000   # half of the queries lie beyond the threshold
    assert float(d[-2]) == THR and float(d[-1]) < THR                     # the query AT the threshold, and the one a step inside
    assert torch.equal(flags[True], flags[False])
    A, B = xyz.shape[0] - 2, xyz.shape[0] - 1
    assert int(flags[True][A]) == 0 and int(flags[True][B]) == 1
    assert 0 < int(flags[True].sum()) < xyz.shape[0]


def test_reproj_filter_writes_the_same_file(tmp_path):
    g = np.load(os.path.join(GOLDEN, "reproj_golden.npz"))
    scene = os.path.join(GOLDEN, "reproj_scene")
    mesh = os.path.join(scene, "mesh.ply")
    out = {}
    for bounded in (True, False):
        out[bounded] = str(tmp_path / ("bounded" if bounded else "plain"))
        reproj.reproj_filter(mesh, mesh, scene, out[bounded], voxel_size=float(g["voxel_size"]), verbose=False, bounded=bounded)
    a = open(os.path.join(out[True], "reprojected.ply"), "rb").read()
    b = open(os.path.join(out[False], "reprojected.ply"), "rb").read()
    assert a == b and len(a) > 200
