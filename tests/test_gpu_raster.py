"""GPU: the triangle depth rasterizer (csrc/ncw_raster.hip via reproj.render_depth) against the float64 test rasterizer
(tests/_raster_oracle.py).  At ROBUST pixels (the winner clear of its edges by MARGIN pixels, every other candidate at least
GAP deeper, relative) the face must be equal and the depth within DEPTH_TOL (relative: fp32 setup + interpolation); at the
others the GPU's face must be one the oracle says covers the sample within MARGIN."""
import math

import numpy as np
import pytest
import torch

from tests import _raster_oracle as O

from neuralrecon_w_amd import mesh, reproj

pytestmark = pytest.mark.gpu

MARGIN, GAP, DEPTH_TOL = 1e-3, 1e-4, 2e-5


def _check(verts, faces, K, view, H, W, cull="back", znear=0.05, zfar=100.0, stats=None):
    d, f = reproj.render_depth(verts, faces, K, view, H, W, znear, zfar, cull, stats=stats)
    d, f = d.cpu().numpy(), f.cpu().numpy()
    o = O.rasterize(verts, faces, K, view, H, W, znear, zfar, cull, margin=MARGIN, gap=GAP)
    rob = o["robust"]
    assert np.array_equal(f[rob], o["face"][rob]), np.argwhere(rob & (f != o["face"]))[:5]
    hit = rob & (o["face"] >= 0)
    err = np.abs(d[hit] - o["depth"][hit]) / o["depth"][hit]
    assert err.size == 0 or err.max() <= DEPTH_TOL, err.max()
    assert ((d > 0) == (f >= 0)).all()
    for q in np.flatnonzero(~rob.reshape(-1) & (f.reshape(-1) >= 0)):
        assert f.reshape(-1)[q] in o["near_cover"][q], (q, f.reshape(-1)[q], o["near_cover"][q])
    return d, f, o


K0 = np.array([[40.0, 0, 16.0], [0, 40.0, 12.0], [0, 0, 1]])


def test_single_triangle_windings_and_culling():
    v = np.array([[-0.3, -0.2, 2.0], [-0.2, 0.25, 2.2], [0.35, -0.1, 1.8]])  # towards the camera: negative pixel area
    front, back = [[0, 1, 2]], [[0, 2, 1]]
    d, f, _ = _check(v, front, K0, np.eye(4), 24, 32)
    n = int((f == 0).sum())
    assert n > 50
    d2, f2, _ = _check(v, back, K0, np.eye(4), 24, 32)
    assert (f2 < 0).all() and (d2 == 0).all()  # culled
    d3, f3, _ = _check(v, back, K0, np.eye(4), 24, 32, cull="none")
    assert np.array_equal(d3, d) and np.array_equal(f3, f)
    _check(v, front, K0, np.eye(4), 24, 32, cull="none")


def test_occlusion_is_independent_of_face_order():
    rng = np.random.RandomState(0)
    tris = []
    for k, z in enumerate((2.0, 2.5, 3.0, 3.5)):
        c = np.array([0.25 * math.cos(2.1 * k), 0.2 * math.sin(2.1 * k)]) + rng.uniform(-0.05, 0.05, 2)
        tris.append([[c[0] - 0.5, c[1] - 0.4, z], [c[0] - 0.3, c[1] + 0.5, z + 0.3], [c[0] + 0.6, c[1] - 0.1, z - 0.2]])
    v = np.array(tris).reshape(-1, 3)
    faces = np.arange(12).reshape(4, 3)
    d, f, o = _check(v, faces, K0, np.eye(4), 24, 32)
    assert len(set(f[f >= 0].tolist())) >= 3  # overlapping, several visible
    for perm in (np.array([3, 2, 1, 0]), np.array([2, 0, 3, 1])):
        dp, fp = reproj.render_depth(v, faces[perm], K0, np.eye(4), 24, 32)
        dp, fp = dp.cpu().numpy(), fp.cpu().numpy()
        assert np.array_equal(dp, d)
        assert np.array_equal(np.where(fp >= 0, perm[np.maximum(fp, 0)], -1), f)


def test_fan_has_no_holes_and_no_overdraw():
    """Edges through pixel centres exactly (vertices on half-integer pixel coordinates, z = 1, unit focal length): every
    sample inside the union is covered, none outside."""
    K = np.eye(3)
    c = np.array([16.5, 15.5, 1.0])
    ring = [np.array([16.5 + 10 * math.cos(a), 15.5 + 10 * math.sin(a), 1.0]) for a in np.linspace(0, 2 * math.pi, 9)[:-1]]
    ring = [np.array([np.round(p[0] - 0.5) + 0.5, np.round(p[1] - 0.5) + 0.5, 1.0]) for p in ring]
    v = np.array([c] + ring)
    faces = np.array([[0, 1 + (i + 1) % 8, 1 + i] for i in range(8)])  # negative pixel area: front facing
    d, f, o = _check(v, faces, K, np.eye(4), 32, 33)
    inside = o["face"] >= 0
    assert inside.sum() > 250
    assert ((f >= 0) == inside).all()  # no holes, no pixel outside the union
    assert (d[inside] == 1.0).all()
    # a sample on a shared edge goes to the smaller face id (equal depth)
    assert np.array_equal(f, o["face"])


def test_triangle_larger_than_the_image_takes_the_large_path():
    v = np.array([[-50.0, -50.0, 4.0], [-50.0, 80.0, 5.0], [80.0, -50.0, 6.0]])
    st = {}
    d, f, o = _check(v, [[0, 1, 2]], K0, np.eye(4), 24, 32, stats=st)
    assert st["large"] == 1 and (f == 0).all()


def test_near_plane_clipping_and_vertices_behind_the_camera():
    # one vertex in front of znear = 0.5 (not behind the camera), and one behind the camera (z < 0): both are clipped
    for z_bad in (0.3, -1.0):
        v = np.array([[-0.4, -0.3, z_bad], [-0.3, 0.6, 3.0], [0.7, -0.2, 2.5]])
        d, f, o = _check(v, [[0, 1, 2]], K0, np.eye(4), 24, 32, znear=0.5)
        assert (f == 0).sum() > 20 and (d[f == 0] >= 0.5 * (1 - 1e-6)).all()
        assert (o["face"] == 0).sum() > 20
    # two vertices in front of znear: the clip gives a quad (two sub-triangles)
    v = np.array([[-0.4, -0.3, 0.2], [0.5, 0.6, 0.1], [0.3, -0.5, 3.0]])
    d, f, o = _check(v, [[0, 1, 2]], K0, np.eye(4), 24, 32, znear=0.5, cull="none")
    assert (f == 0).sum() > 20


def test_far_plane_degenerate_and_sub_pixel_triangles():
    # crossing zfar = 3: the part beyond it is dropped; a face entirely beyond is dropped
    v = np.array([[-0.5, -0.4, 2.0], [-0.4, 0.5, 4.0], [0.6, -0.2, 2.5], [-0.5, -0.5, 5.0], [-0.5, 0.5, 5.0], [0.5, 0.0, 5.0]])
    d, f, o = _check(v, [[0, 1, 2], [3, 4, 5]], K0, np.eye(4), 24, 32, zfar=3.0, cull="none")
    assert (f == 0).sum() > 10 and (d <= 3.0).all() and (f != 1).all()
    # degenerate: a repeated index, collinear vertices
    v = np.array([[0.0, 0.0, 2.0], [0.3, 0.3, 2.0], [0.6, 0.6, 2.0], [-0.2, 0.1, 2.0]])
    d, f, _ = _check(v, [[0, 1, 2], [0, 3, 3], [1, 1, 1]], K0, np.eye(4), 24, 32, cull="none")
    assert (f < 0).all()
    # tiny triangles between pixel centres (pixel coordinates (c + 0.1 .. c + 0.4)): nothing covered
    K = np.eye(3)
    tris = [[[x + 0.1, y + 0.1, 1.0], [x + 0.4, y + 0.1, 1.0], [x + 0.1, y + 0.4, 1.0]] for x in range(4, 12) for y in range(3, 9)]
    v = np.array(tris).reshape(-1, 3)
    faces = np.arange(len(v)).reshape(-1, 3)
    d, f, _ = _check(v, faces, K, np.eye(4), 16, 16, cull="none")
    assert (f < 0).all()


def test_random_overlapping_triangles_non_square_image_deterministic():
    rng = np.random.RandomState(7)
    n = 3000
    K = np.array([[31.0, 0, 17.3], [0, 19.0, 12.6], [0, 0, 1]])  # fx != fy, odd, non-square (37 x 23)
    ctr = np.c_[rng.uniform(-0.8, 0.8, (n, 2)), rng.uniform(1.0, 4.0, n)]
    v = (ctr[:, None, :] + rng.normal(0, 0.12, (n, 3, 3)) * np.array([1, 1, 0.5])).reshape(-1, 3)
    v[: 60 * 3] = (ctr[:60, None, :] + rng.normal(0, 0.8, (60, 3, 3)) * np.array([1, 1, 0.2])).reshape(-1, 3)  # big ones
    faces = np.arange(3 * n).reshape(n, 3)
    st = {}
    d, f, o = _check(v, faces, K, np.eye(4), 23, 37, cull="none", stats=st)
    assert st["large"] > 0 and (o["robust"] & (o["face"] >= 0)).sum() > 400
    d2, f2 = reproj.render_depth(v, faces, K, np.eye(4), 23, 37, cull="none")
    assert np.array_equal(d2.cpu().numpy(), d) and np.array_equal(f2.cpu().numpy(), f)
    # a general view matrix (rotation + translation) and back faces culled
    R = np.linalg.qr(rng.randn(3, 3))[0]
    R *= np.sign(np.linalg.det(R))
    view = np.eye(4)
    view[:3, :3] = R
    view[:3, 3] = [0.1, -0.2, 0.5]
    vw = (v - view[:3, 3]) @ R  # camera = R world + t: the soup sits where it sat in front of the camera
    _check(vw, faces, K, view, 23, 37, cull="back")


def test_closed_sphere_from_isosurface():
    D = 64
    g = torch.linspace(-1, 1, D, device="cuda:0")
    X, Y, Z = torch.meshgrid(g, g, g, indexing="ij")
    sdf = (torch.sqrt(X * X + Y * Y + Z * Z) - 0.6).contiguous()
    verts, faces = mesh.isosurface(sdf)
    verts = verts * (2.0 / (D - 1)) - 1.0
    H, W = 60, 80
    K = np.array([[70.0, 0, 40.3], [0, 72.0, 29.6], [0, 0, 1]])
    view = np.eye(4)
    view[2, 3] = 3.0  # sphere centre at camera z = 3
    d, f = reproj.render_depth(verts, faces, K, view, H, W)
    dn, fn = reproj.render_depth(verts, faces, K, view, H, W, cull="none")
    assert np.array_equal(d.cpu().numpy(), dn.cpu().numpy())
    assert (f == fn).float().mean().item() > 0.999
    d = d.cpu().numpy()
    # analytic ray / sphere hit along (x, y, 1) through the pixel centre: depth = t
    c, r = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    x, y = (c - K[0, 2]) / K[0, 0], (r - K[1, 2]) / K[1, 1]
    a, b, cc = x * x + y * y + 1, -2 * 3.0, 9.0 - 0.36
    disc = b * b - 4 * a * cc
    t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0)
    clear = disc > 0.4  # away from the silhouette (disc = 1.44 at the centre, 0 on the silhouette)
    assert clear.sum() > 300
    assert (d[clear] > 0).all() and np.abs(d[clear] - t[clear]).max() < 4e-3
    assert (d[disc < -0.5] == 0).all() and (d[disc > 0] > 0).mean() > 0.95
