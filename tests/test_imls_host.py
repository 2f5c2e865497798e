"""No GPU: the numpy restatement of the IMLS values (tests/_imls_ref.py) against closed forms, the sphere fixture the GPU mesh
tests stand on, the binding, and every refusal of cloudmesh.mesh_cloud that comes before a launch."""
import numpy as np
import pytest
import torch

from tests import _imls_ref as R

from neuralrecon_w_amd import cloudmesh
from neuralrecon_w_amd import lib as L

EPS32 = float(np.finfo(np.float32).eps)


def test_plane_cloud_gives_the_signed_distance():
    """Every term n.(x - p_i) of a plane cloud IS the signed distance of x, so the weighted mean is too, whatever the weights:
    what is left is the float32 rounding of x, of p_i and of x - p_i, each at most eps32 / 2 of a coordinate below `extent`."""
    P, N, n, o = R.plane_cloud()
    voxel, support = 0.06, 3.0
    lat_lo, side = R.lattice_for(P.min(0), P.max(0), voxel, support)
    lat_lo = [float(np.float32(v)) for v in lat_lo]
    ps = np.concatenate([P.astype(np.float32), np.zeros((P.shape[0], 1), np.float32)], 1)
    ns = np.concatenate([N.astype(np.float32), np.zeros((P.shape[0], 1), np.float32)], 1)
    idx = np.stack(np.meshgrid(*[np.arange(s) for s in side], indexing="ij"), -1).reshape(-1, 3)
    value, count, d2min = R.imls_ref(ps, ns, idx, lat_lo, voxel, side, support * voxel)
    x = R.lattice_points(idx, lat_lo, voxel).astype(np.float64)
    true = (x - o) @ n
    got = count > 0
    assert got.sum() > 1000 and np.isfinite(value[got]).all()
    extent = max(np.abs(x).max(), np.abs(P).max())
    assert np.abs(value[got].astype(np.float64) - true[got]).max() <= 4 * EPS32 * extent
    assert (np.isnan(value[~got])).all() and (d2min[~got] == np.inf).all()
    # d2min is the brute-force nearest squared distance, where there is one within the support
    d2 = ((x[:, None, :] - ps[None, :, :3].astype(np.float64)) ** 2).sum(-1).min(1)
    assert np.abs(d2min[got] - d2[got]).max() <= 8 * EPS32 * (support * voxel) ** 2 + 8 * EPS32 * extent * support * voxel


def test_sphere_fixture_values_and_support():
    """On a sphere of radius r the term of a sample at angle theta from x (|x| = rho) is rho cos(theta) - r, so
    f - (rho - r) = -rho * <1 - cos(theta)> <= 0, and |x - p|^2 = rho^2 + r^2 - 2 rho r cos(theta) <= R^2 gives
    1 - cos(theta) <= (R^2 - (rho - r)^2) / (2 rho r):   0 <= (rho - r) - f <= (R^2 - (rho - r)^2) / (2 r)   for ANY sampling --
    at R = 3 voxels of 0.08 that is at most 0.36 voxel.  Measured on this fixture: max 0.0613 voxel, mean 0.0512 voxel over the
    7894 supported points (the weight favours the near samples, whose angle is small).  The fixture leaves no lattice point within
    sqrt(3) voxels of the sphere unsupported (6811 such points; the fewest samples in range there is 37, the farthest nearest
    sample 1.78 voxels): a closed mesh is a fair demand of it."""
    s = R.sphere_reference()
    sp, true, f = s["sparse"], s["true"], s["value"].astype(np.float64)
    R2 = (R.SPHERE_SUPPORT * R.SPHERE_VOXEL) ** 2
    slack = 64 * EPS32
    gap = true[sp] - f[sp]
    assert sp.sum() > 5000
    assert (gap >= -slack).all()
    assert (gap <= (R2 - true[sp] ** 2) / (2 * R.SPHERE_R) + slack).all()
    assert gap.max() <= 0.07 * R.SPHERE_VOXEL                             # the measured 0.0613, so that a drift of the fixture shows
    close = np.abs(true) <= np.sqrt(3.0) * R.SPHERE_VOXEL
    assert close.sum() > 5000 and not (close & ~sp).any()
    far = np.abs(true) > 0.5 * R.SPHERE_VOXEL
    assert not (sp & far & (np.sign(f) != np.sign(true))).any()


def test_rows_tie_and_outside():
    """The row order, an exact d2 == r2 tie (w = 0: NaN with count 1), and a lattice index outside `side`."""
    assert R.block_rows([[1, 2, 3]])[[0, 1, 4, 16, 63]].tolist() == [[4, 8, 12], [4, 8, 13], [4, 9, 12], [5, 8, 12], [7, 11, 15]]
    ps = np.array([[0.75, 0.0, 0.0, 0.0]], np.float32)
    ns = np.array([[1.0, 0.0, 0.0, 0.0]], np.float32)
    v, c, d = R.imls_ref(ps, ns, [[0, 0, 0], [1, 0, 0], [4, 0, 0], [-1, 0, 0]], [0.0, 0.0, 0.0], 0.25, [4, 4, 4], 0.75)
    assert c.tolist() == [1, 1, 0, 0] and np.isnan(v[0]) and v[1] == np.float32(-0.5) and np.isnan(v[2:]).all()
    assert d.tolist()[:2] == [0.5625, 0.25] and (d[2:] == np.inf).all()


def test_symbol_and_abi():
    assert "ncw_imls_values" in L.exported_symbols() and L.ABI_VERSION >= 41


def _cloud():
    P, N, _, _ = R.plane_cloud(8)
    return torch.from_numpy(P), torch.from_numpy(N)


@pytest.mark.parametrize("case", ["no_normals", "nan_normal", "short_normal", "long_normal", "shape", "near", "support", "side",
                                  "voxel", "nan_point", "min_count", "box"])
def test_mesh_cloud_refusals(case):
    """Every ValueError mesh_cloud raises before a launch, on CPU tensors (the refusal of more than 2^31 - 1 sparse points can only
    follow the launches that count them, and needs a lattice no test can hold).  A valid call on CPU tensors reaches the device
    check instead: there is no fallback."""
    P, N = _cloud()
    kw = dict(voxel=0.05)
    if case == "no_normals":
        N = None
    elif case == "nan_normal":
        N = N.clone(); N[3, 1] = float("nan")
    elif case == "short_normal":
        N = N * 0.998
    elif case == "long_normal":
        N = N.clone(); N[5] *= 1.002
    elif case == "shape":
        N = N[:-1]
    elif case == "near":
        kw.update(near=1.7)
    elif case == "support":
        kw.update(support=2.5, near=2.6)
    elif case == "side":
        kw.update(voxel=1e-5)
    elif case == "voxel":
        kw.update(voxel=0.0)
    elif case == "nan_point":
        P = P.clone(); P[0, 0] = float("inf")
    elif case == "min_count":
        kw.update(min_count=0)
    elif case == "box":
        kw.update(box=[[0, 0, 0], [1, -1, 1]])
    with pytest.raises(ValueError):
        cloudmesh.mesh_cloud(P, N, **kw)


def test_mesh_cloud_has_no_cpu_fallback():
    P, N = _cloud()
    with pytest.raises(L.NeuconwHipError):
        cloudmesh.mesh_cloud(P, N, 0.05)
    with pytest.raises(L.NeuconwHipError):
        cloudmesh.mesh_cloud(P, N * 0.9995, 0.05, near=1.7320508075688772, support=1.7320508075688772)  # the limits themselves pass
