"""GPU: `ncw_view_rays` (csrc/ncw_view.hip) -- the rays of a pixel range of a camera view, generated on the device -- against the
float64 restatement of datasets/ray_utils.py:18-52 + datasets/phototourism.py:769-782 (tests/_view_ref.py) and the golden rays
recorded from the reference itself (tests/golden/view_golden.npz)."""
import os

import numpy as np
import pytest
import torch

from tests import _view_ref as VR
from tests._util import GOLDEN

pytestmark = pytest.mark.gpu


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def _cameras():
    from neuralrecon_w_amd.views import Camera

    g = np.load(os.path.join(GOLDEN, "view_golden.npz"))
    W, H = [int(v) for v in g["rays_wh"]]
    c2w = np.concatenate([_rot((1.0, 0.4, -0.7), 63.0), [[0.3], [1.7], [-0.9]]], 1)
    return {"7x5": (Camera(g["rays_K"], g["rays_c2w"], W, H, 0.25, 7.5), g),
            "37x23": (Camera([[41.3, 0, 17.2], [0, 39.8, 12.9], [0, 0, 1]], c2w, 37, 23, 0.0947, 9.479), None),
            "1x1": (Camera([[1.5, 0, 0.2], [0, 1.25, -0.4], [0, 0, 1]], c2w, 1, 1, 1.0, 3.0), None)}


@pytest.mark.parametrize("name", ["7x5", "37x23", "1x1"])
def test_view_rays_match_the_restatement(name):
    """o, near and far are bitwise the camera's float32 values; d is within 1e-6 absolute of the float64 restatement (each
    component of a unit vector sees about ten float32 roundings of <= 6e-8)."""
    from neuralrecon_w_amd import views

    cam, gold = _cameras()[name]
    hw = cam.width * cam.height
    rays = views.view_rays(cam)
    assert rays.shape == (hw, 8)
    ref = VR.view_rays(cam.K, cam.c2w, cam.width, cam.height, cam.near, cam.far)
    got = rays.cpu()
    assert torch.equal(got[:, :3], ref[:, :3].float()) and torch.equal(got[:, 6:], ref[:, 6:].float())
    assert torch.equal(got[:, :3], torch.from_numpy(cam.c2w[:, 3]).expand(hw, 3))
    err = float((got[:, 3:6].double() - ref[:, 3:6]).abs().max())
    print("%s: max |d - d64| = %.3g" % (name, err))
    assert err <= 1e-6
    if gold is not None:  # the reference's own float32 rays
        assert torch.equal(got[:, :3], torch.from_numpy(gold["rays_o"]))
        assert float((got[:, 3:6] - torch.from_numpy(gold["rays_d"])).abs().max()) <= 1e-6


@pytest.mark.parametrize("name", ["7x5", "37x23"])
def test_chunks_equal_the_full_launch_bitwise(name):
    """Chunks that start mid-row and end ragged (p0 = 11, n = 100 of the 37-wide view; 3-pixel chunks of the 7-wide one): the
    union of chunks is bitwise the single full launch, and a chunk writes nothing outside its rows."""
    from neuralrecon_w_amd import views

    cam, _ = _cameras()[name]
    hw = cam.width * cam.height
    full = views.view_rays(cam)
    if name == "37x23":
        part = views.view_rays(cam, p0=11, n=100)
        assert torch.equal(part, full[11:111])
        bounds = [0, 11, 111, 400, 401, hw]
    else:
        bounds = list(range(0, hw, 3)) + [hw]
    buf = torch.full((hw + 2, 8), -7.0, device="cuda")
    for a, b in zip(bounds[:-1], bounds[1:]):
        views.view_rays(cam, p0=a, n=b - a, out=buf[1 + a:1 + b])
    assert torch.equal(buf[1:-1], full) and bool((buf[0] == -7).all()) and bool((buf[-1] == -7).all())


def test_pixel_ranges_outside_the_view_are_refused():
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import views

    cam, _ = _cameras()["7x5"]
    for p0, n in ((30, 6), (-1, 3), (36, 1)):
        with pytest.raises(L.NeuconwHipError):
            views.view_rays(cam, p0=p0, n=n, out=torch.empty(n, 8, device="cuda"))
    assert views.view_rays(cam, p0=35, n=0).shape == (0, 8)


def test_bad_ray_buffers_are_refused_before_the_launch():
    """A buffer of the wrong shape or dtype is a ValueError, a host buffer and a buffer that is not 16-byte aligned (rows are
    written as two 16-byte stores) are refused by the binding: nothing is written."""
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import views

    cam, _ = _cameras()["7x5"]
    for bad in (torch.empty(10, 7, device="cuda"), torch.empty(9, 8, device="cuda"), torch.empty(10, 8, device="cuda", dtype=torch.float64),
                torch.empty(8, 10, device="cuda").T):
        with pytest.raises(ValueError):
            views.view_rays(cam, p0=0, n=10, out=bad)
    with pytest.raises(L.NeuconwHipError):
        views.view_rays(cam, p0=0, n=10, out=torch.empty(10, 8))
    flat = torch.full((81,), -7.0, device="cuda")
    with pytest.raises(L.NeuconwHipError):
        views.view_rays(cam, p0=0, n=10, out=flat[1:].view(10, 8))  # 4 bytes past a 16-byte boundary
    assert bool((flat == -7).all())
