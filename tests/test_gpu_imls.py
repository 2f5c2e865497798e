"""GPU: the IMLS values kernel (ncw_imls_values of csrc/ncw_imls.hip through cloudmesh.imls_values), the meshes
cloudmesh.mesh_cloud makes of them, and scripts/mesh_cloud.py.

The three output planes are compared BIT FOR BIT -- the value as its bits, NaNs included -- with the numpy restatement of
tests/_imls_ref.py, a brute force over ALL of pts_sorted: a cell the walk leaves out shows as a missing point.
tests/test_imls_host.py checks that restatement against closed forms without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import _imls_ref as R
from tests._util import ROOT

from neuralrecon_w_amd import cloudmesh, evalmesh, meshops, ply
from neuralrecon_w_amd import lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS32 = float(np.finfo(np.float32).eps)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _grid(P32, target_cells, cmax=None):
    p = torch.from_numpy(np.ascontiguousarray(P32, dtype=np.float32)).to(DEV)
    return evalmesh.NNGrid(p, float(np.abs(P32).max()) if cmax is None else cmax, target_cells=target_cells)


def _tables(grid, N):
    """(ps, ns) as numpy: pts_sorted and the normals gathered into its order, as the kernel reads them."""
    ns = cloudmesh.gather_normals(grid, torch.from_numpy(np.ascontiguousarray(N, dtype=np.float32)).to(DEV))
    return grid.pts.cpu().numpy(), ns.cpu().numpy(), ns


def _run(grid, ns_t, blocks, lat_lo, voxel, side, radius, stats=None):
    b = torch.from_numpy(np.ascontiguousarray(blocks, dtype=np.int32)).to(DEV)
    return cloudmesh.imls_values(grid, None, b, lat_lo, voxel, side, radius, stats=stats, sorted_normals=ns_t)


def _same(got, want, what=""):
    v, c, d = (t.cpu().numpy() for t in got)
    wv, wc, wd = want
    assert v.dtype == np.float32 and c.dtype == np.int32 and d.dtype == np.float32 and v.shape == wv.shape
    assert np.array_equal(c, wc), (what, "count", int((c != wc).sum()))
    assert np.array_equal(d, wd), (what, "d2min", int((d != wd).sum()))
    assert np.array_equal(v.view(np.uint32), wv.view(np.uint32)), (what, "value", int((v.view(np.uint32) != wv.view(np.uint32)).sum()))


def _check(P32, N, target_cells, blocks, lat_lo, voxel, side, radius, what="", grid=None):
    grid = _grid(P32, target_cells) if grid is None else grid
    ps, ns, ns_t = _tables(grid, N)
    want = R.imls_ref(ps, ns, R.block_rows(blocks), lat_lo, voxel, side, radius)
    got = _run(grid, ns_t, blocks, lat_lo, voxel, side, radius)
    _same(got, want, what)
    return grid, want


def _all_blocks(side):
    nb = [(s + 3) // 4 for s in side]
    return np.stack(np.meshgrid(*[np.arange(n) for n in nb], indexing="ij"), -1).reshape(-1, 3)


def _cube_cloud(n, seed):
    rs = np.random.RandomState(seed)
    return rs.rand(n, 3).astype(np.float32), _unit(rs.randn(n, 3)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# 1. bit for bit
# ---------------------------------------------------------------------------------------------------
def test_one_point():
    P = np.array([[0.3, -0.2, 0.1]], np.float32)
    N = np.array([[0.6, 0.0, 0.8]], np.float32)
    side = [9, 9, 9]
    _, want = _check(P, N, None, _all_blocks(side), [-0.2, -0.7, -0.4], 0.125, side, 0.3, "m = 1")
    assert (want[1] == 1).sum() > 10 and (want[1] == 0).sum() > 10


@pytest.mark.parametrize("m", [255, 256, 257])
def test_duplicates_in_one_cell_cross_a_tile(m):
    """m copies of one point (one cell, m staged points: a tile holds 256), each with its own normal: the float64 sums depend on
    the order, so a point staged twice, dropped or out of order shows."""
    P = np.repeat(np.array([[0.5, 0.25, -0.125]], np.float32), m, 0)
    N = _unit(np.random.RandomState(m).randn(m, 3)).astype(np.float32)
    side = [8, 8, 8]
    _, want = _check(P, N, None, _all_blocks(side), [0.0, -0.25, -0.625], 0.125, side, 0.4, "m = %d" % m)
    assert set(np.unique(want[1]).tolist()) == {0, m}


def test_side_not_a_multiple_of_four_and_blocks_beyond_it():
    P, N = _cube_cloud(300, 1)
    side = [5, 6, 7]
    blocks = np.concatenate([_all_blocks(side), [[2, 0, 0], [0, 2, 1], [-1, 0, 0], [0, 0, 5000], [2 ** 29, 0, 0], [0, -2 ** 31, 0]]])
    _, want = _check(P, N, None, blocks, [0.1, 0.0, -0.1], 0.15, side, 0.3, "side 5 6 7")
    rows = R.block_rows(blocks)
    out = ~((rows >= 0) & (rows < np.array(side))).all(1)
    assert out.sum() >= 6 * 64 and np.isnan(want[0][out]).all() and (want[1][out] == 0).all() and (want[2][out] == np.inf).all()
    assert (want[1][~out] > 0).sum() > 100


@pytest.mark.parametrize("nb", [1, 63, 64, 65])
def test_block_counts(nb):
    P, N = _cube_cloud(400, 2)
    side = [20, 20, 20]
    blocks = _all_blocks(side)[np.random.RandomState(nb).permutation(125)[:nb]]
    _check(P, N, None, blocks, [0.0, 0.0, 0.0], 0.05, side, 0.12, "%d blocks" % nb)


@pytest.mark.parametrize("target_cells,what", [(1, "radius below h: one cell"), (32768, "radius of several h")])
def test_radius_against_the_cell_size(target_cells, what):
    P, N = _cube_cloud(600, 3)
    side = [12, 12, 12]
    grid = _grid(P, target_cells)
    radius = 0.2
    assert (radius < grid.h) if target_cells == 1 else (radius > 5 * grid.h)
    _, want = _check(P, N, target_cells, _all_blocks(side), [-0.05, -0.05, -0.05], 0.1, side, radius, what, grid=grid)
    assert want[1].max() > 5


def test_lattice_ties_and_zero_weight():
    """Cloud points ON lattice positions, voxel = 2^-2, radius = 3 voxels: every coordinate, d2 and r2 = 0.5625 is exact, so points
    at exactly d2 == r2 are admitted (inclusive) with w = 0; the lone far point gives count 1, W = 0, value NaN."""
    voxel, side, lat_lo = 0.25, [24, 12, 12], [-1.0, -1.0, -1.0]
    i = np.stack(np.meshgrid(np.arange(4, 8), np.arange(4, 8), np.arange(4, 8), indexing="ij"), -1).reshape(-1, 3)
    i = np.concatenate([i, [[18, 5, 5]]])
    P = (np.array(lat_lo) + i * voxel).astype(np.float32)
    N = _unit(np.random.RandomState(4).randn(P.shape[0], 3)).astype(np.float32)
    blocks = _all_blocks(side)
    _, (v, c, d) = _check(P, N, 64, blocks, lat_lo, voxel, side, 3 * voxel, "ties")
    rows = R.block_rows(blocks)
    lone = (rows == [21, 5, 5]).all(1) | (rows == [18, 8, 5]).all(1) | (rows == [18, 5, 2]).all(1)
    assert lone.sum() == 3 and (c[lone] == 1).all() and np.isnan(v[lone]).all() and (d[lone] == np.float32(0.5625)).all()
    tie = (d == np.float32(0.5625)) & (c == 1)
    assert tie.sum() >= 6
    assert ((c > 1) & np.isfinite(v)).sum() > 400


def _outlier_case():
    rs = np.random.RandomState(5)
    P = rs.rand(2000, 3).astype(np.float32)
    # far outliers, one beyond each end of each axis: the grid box (the 0.1 % .. 99.9 % quantiles of 2000 points) stays the unit cube
    P[:3] = np.array([[-50.0, -40.0, 0.5], [48.0, 0.3, -45.0], [0.6, 52.0, 41.0]], np.float32)
    N = _unit(rs.randn(2000, 3)).astype(np.float32)
    voxel, lat_lo, side = 0.1, [-52.0, -52.0, -52.0], [1050, 1050, 1050]
    li = np.floor((P - np.array(lat_lo, np.float32)) / voxel).astype(np.int64) // 4
    near = np.unique(np.concatenate([li[:3] + o for o in ([0, 0, 0], [1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, 1, 0], [-1, -1, -1])]), axis=0)
    inl = np.unique(li[3:67], axis=0)
    edge = np.array([[129, 129, 129], [133, 131, 130], [130, 133, 129], [0, 0, 0], [262, 262, 262]])  # just outside the grid box; corners
    return P, N, voxel, lat_lo, side, np.concatenate([near, inl, edge])


def test_outliers_clamped_into_boundary_cells():
    P, N, voxel, lat_lo, side, blocks = _outlier_case()
    grid = _grid(P, None, cmax=60.0)
    lo, hi = np.array(grid.lo), np.array(grid.lo) + np.array(grid.ext)
    assert ((P[:3] < lo - 30) | (P[:3] > hi + 30)).any(1).all() and (hi - lo).max() < 1.01   # far outside the box the cells cover
    _, (v, c, d) = _check(P, N, None, blocks, lat_lo, voxel, side, 0.35, "outliers", grid=grid)
    rows = R.lattice_points(R.block_rows(blocks), lat_lo, voxel)
    beyond = ((rows < lo - 1.0) | (rows > hi + 1.0)).any(1)
    assert (c[beyond] > 0).sum() >= 100                                # lattice points far outside the grid box found their outlier
    assert (c[~beyond] > 3).sum() > 1000


def test_non_finite_points_are_never_admitted():
    P, N = _cube_cloud(500, 6)
    grid = _grid(P, None)
    ps0 = grid.pts.cpu().numpy()
    grid.pts[7, 0] = float("nan")
    grid.pts[100, 2] = float("inf")
    grid.pts[301, 1] = float("-inf")
    side = [12, 12, 12]
    blocks = _all_blocks(side)
    _, (v, c, d) = _check(P, N, None, blocks, [-0.05, -0.05, -0.05], 0.1, side, 0.25, "nan point", grid=grid)
    ps, ns, _ = _tables(grid, N)
    clean = R.imls_ref(np.delete(ps, [7, 100, 301], 0), np.delete(ns, [7, 100, 301], 0), R.block_rows(blocks), [-0.05, -0.05, -0.05], 0.1,
                       side, 0.25)
    assert np.array_equal(c, clean[1]) and np.array_equal(v.view(np.uint32), clean[0].view(np.uint32))
    full = R.imls_ref(ps0, ns, R.block_rows(blocks), [-0.05, -0.05, -0.05], 0.1, side, 0.25)
    assert (full[1] != c).any()                                        # the three points did count before


def test_order_split_and_repeat():
    P, N, voxel, lat_lo, side, blocks = _outlier_case()
    grid = _grid(P, None, cmax=60.0)
    _, _, ns_t = _tables(grid, N)
    st = {}
    a = [t.cpu().numpy() for t in _run(grid, ns_t, blocks, lat_lo, voxel, side, 0.35, stats=st)]
    b = [t.cpu().numpy() for t in _run(grid, ns_t, blocks, lat_lo, voxel, side, 0.35)]
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))          # two runs
    assert st["staged"] >= int(a[1].max())
    perm = np.random.RandomState(8).permutation(blocks.shape[0])
    p = [t.cpu().numpy() for t in _run(grid, ns_t, blocks[perm], lat_lo, voxel, side, 0.35)]
    for x, y in zip(a, p):
        assert np.array_equal(x.reshape(-1, 64)[perm].view(np.uint32), y.reshape(-1, 64).view(np.uint32))
    k = blocks.shape[0] // 3
    s1 = [t.cpu().numpy() for t in _run(grid, ns_t, blocks[:k], lat_lo, voxel, side, 0.35)]
    s2 = [t.cpu().numpy() for t in _run(grid, ns_t, blocks[k:], lat_lo, voxel, side, 0.35)]
    for x, y1, y2 in zip(a, s1, s2):
        assert np.array_equal(x.view(np.uint32), np.concatenate([y1, y2]).view(np.uint32))
    empty = _run(grid, ns_t, blocks[:0], lat_lo, voxel, side, 0.35)
    assert all(t.numel() == 0 for t in empty)


def test_badarg():
    P, N = _cube_cloud(100, 9)
    grid = _grid(P, None)
    _, _, ns_t = _tables(grid, N)
    lib, st = L.get_lib(), L.stream_ptr(torch.device(DEV))
    blocks = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    out = [torch.full((128,), 7.0, device=DEV), torch.full((128,), 7, dtype=torch.int32, device=DEV), torch.full((128,), 7.0, device=DEV)]
    nan = float("nan")

    def call(pts=grid.pts, nrm=ns_t, rng=grid.range, m=grid.m, g=grid.cgrid, margin=grid.margin, bl=blocks, nb=2, lo=(0.0, 0.0, 0.0),
             voxel=0.1, side=(8, 8, 8), radius=0.3, o=out):
        return lib.ncw_imls_values(L.ptr(pts), L.ptr(nrm), L.ptr(rng), m, C.byref(g) if g is not None else None, float(margin),
                                   L.ptr(bl), nb, (C.c_float * 3)(*lo) if lo is not None else None, float(voxel),
                                   (C.c_int32 * 3)(*side) if side is not None else None, float(radius), L.ptr(o[0]), L.ptr(o[1]),
                                   L.ptr(o[2]), None, st)

    bad = L.NcwNnGrid()
    C.memmove(C.byref(bad), C.byref(grid.cgrid), C.sizeof(bad))
    bad.dim[1] = 0
    for kw in (dict(pts=None), dict(nrm=None), dict(rng=None), dict(bl=None), dict(lo=None), dict(side=None), dict(g=None), dict(g=bad),
               dict(o=[None, out[1], out[2]]), dict(o=[out[0], None, out[2]]), dict(o=[out[0], out[1], None]),
               dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=nan), dict(radius=0.0), dict(radius=-0.3), dict(radius=nan),
               dict(margin=-1e-6), dict(margin=nan), dict(side=(0, 8, 8)), dict(side=(8, 16385, 8)), dict(side=(8, 8, -4)), dict(m=0)):
        assert call(**kw) == -1, kw                             # NCW_E_BADARG
    assert call(nb=0) == 0 and call(nb=-5) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)                      # nothing was launched
    assert call() == 0 and call(side=(16384, 1, 1)) == 0
    torch.cuda.synchronize()
    assert not bool((out[0] == 7).any())


# ---------------------------------------------------------------------------------------------------
# 2. meshes
# ---------------------------------------------------------------------------------------------------
def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _edges(faces):
    f = faces.cpu().numpy().astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return np.unique(e, axis=0, return_counts=True)


def _face_normals(v, f):
    v, f = v.cpu().numpy(), f.cpu().numpy().astype(np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return np.cross(b - a, c - a), (a + b + c) / 3.0


def test_plane_patch():
    """Every term of a plane cloud is the signed distance itself, so the values are exact to float32 rounding and so is every
    crossing: the vertices lie on the plane to a few float32 roundings of the coordinates, and the faces look along the normal."""
    P, N, n, o = R.plane_cloud()
    voxel = 0.06
    st = {}
    v, f = cloudmesh.mesh_cloud(_t(P), _t(N), voxel, stats=st)
    assert f.shape[0] > 500 and st["sparse"] > 1000 and st["candidates"] >= st["sparse"]
    off = np.abs((v.cpu().numpy() - o) @ n)
    extent = float(np.abs(P).max()) + voxel * max(st["side"])
    print("plane: %d vertices, %d faces, max |offset| %.3e (bound %.3e)" % (v.shape[0], f.shape[0], off.max(), 16 * EPS32 * extent))
    assert off.max() <= 16 * EPS32 * extent
    fn, _ = _face_normals(v, f)
    assert ((fn @ n) > 0).all()


@pytest.fixture(scope="module")
def sphere():
    s = R.sphere_reference()
    st = {}
    v, f = cloudmesh.mesh_cloud(_t(s["P"]), _t(s["N"]), R.SPHERE_VOXEL, support=R.SPHERE_SUPPORT, near=R.SPHERE_NEAR,
                                min_count=R.SPHERE_MIN_COUNT, stats=st)
    return s, v, f, st


def test_sphere_is_closed_and_outward(sphere):
    s, v, f, st = sphere
    # the restatement holds every lattice point within near + 1 voxels of the sphere: all that can pass the support rule
    assert st["side"] == s["side"] and st["sparse"] == int(s["sparse"].sum())
    _, sizes = meshops.components(f, int(v.shape[0]))
    assert int((sizes > 0).sum()) == 1
    e, cnt = _edges(f)
    assert (cnt == 2).all()
    assert int(v.shape[0]) - e.shape[0] + int(f.shape[0]) == 2
    fn, cen = _face_normals(v, f)
    assert ((fn * cen).sum(1) > 0).all()


def test_sphere_radial_error(sphere):
    """A vertex is the zero of the linear interpolant of f along a lattice edge of length v: f is off the true distance by at most
    e = the restatement's own maximum |f - true| over the supported points, and the true distance |x| - r has second derivative at
    most 1 / (r - v) along an edge near the surface, so its interpolant is off by at most v^2 / (8 (r - v)).  The factor 1.5 covers
    the welded vertices' float32 positions."""
    s, v, f, _ = sphere
    e = np.abs(s["value"].astype(np.float64) - s["true"])[s["sparse"]].max()
    bound = 1.5 * (e + R.SPHERE_VOXEL ** 2 / (8 * (R.SPHERE_R - R.SPHERE_VOXEL)))
    err = np.abs(np.linalg.norm(v.cpu().numpy(), axis=1) - R.SPHERE_R)
    print("sphere: %d vertices, radial error max %.5f mean %.5f (bound %.5f, e %.5f)" % (v.shape[0], err.max(), err.mean(), bound, e))
    assert err.max() <= bound


def test_sphere_without_a_cap_stays_open():
    s = R.sphere_reference()
    keep = s["P"][:, 2] < 0.75
    P, N = s["P"][keep], s["N"][keep]
    v, f = cloudmesh.mesh_cloud(_t(P), _t(N), R.SPHERE_VOXEL, near=R.SPHERE_NEAR)
    e, cnt = _edges(f)
    assert (cnt <= 2).all() and (cnt == 1).sum() > 10                  # a boundary: the mesh is open
    d, _ = evalmesh.nn_distances(_t(P), v)
    print("open sphere: %d boundary edges, farthest vertex %.4f voxels from a sample" % ((cnt == 1).sum(), float(d.max()) / R.SPHERE_VOXEL))
    assert float(d.max()) <= R.SPHERE_NEAR * R.SPHERE_VOXEL
    assert float(v[:, 2].max()) < 0.75 + R.SPHERE_NEAR * R.SPHERE_VOXEL


# ---------------------------------------------------------------------------------------------------
# 3. the tool
# ---------------------------------------------------------------------------------------------------
def _tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "mesh_cloud.py")] + list(args), capture_output=True, text=True,
                          cwd=ROOT, timeout=600)


def test_tool_round_trip(tmp_path):
    """An icosphere sampled by area, with its face normals and a colour per sample, through scripts/mesh_cloud.py and back
    against the samples with scripts/eval_mesh.py --exact_recall: every sample within one voxel of the new surface."""
    voxel = 0.08
    vs, fs = R.icosphere(3)
    pts, tri = evalmesh.sample_surface(vs, fs, 6000, seed=1, return_index=True, device=DEV)
    fn = np.cross(vs[fs[:, 1]] - vs[fs[:, 0]], vs[fs[:, 2]] - vs[fs[:, 0]])
    nrm = _unit(fn)[tri.cpu().numpy()]
    rgb = np.random.RandomState(0).randint(0, 256, (6000, 3)).astype(np.uint8)
    rgb[:, 2] = np.arange(6000) % 251                                 # every colour in the cloud is known
    cloud, bare, out = str(tmp_path / "cloud.ply"), str(tmp_path / "bare.ply"), str(tmp_path / "mesh.ply")
    ply.write(cloud, pts.cpu().numpy(), rgb=rgb, normals=nrm)
    ply.write(bare, pts.cpu().numpy(), rgb=rgb)
    r = _tool("--file_in", bare, "--file_out", out, "--voxel", str(voxel))
    assert r.returncode != 0 and "clean_cloud.py --toward" in r.stderr and not os.path.exists(out)
    r = _tool("--file_in", cloud, "--file_out", out, "--voxel", str(voxel), "--color", "--min_component_faces", "10")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout)
    for word in ("points: 6000", "candidate lattice points", "sparse points", "vertices", "faces", "components:", "boundary edges:"):
        assert word in r.stdout, word
    v, f, c = ply.read_mesh(out)
    assert f.shape[0] > 1000 and c is not None and c.shape == (v.shape[0], 3)
    known = set(map(tuple, rgb.tolist()))
    assert all(tuple(x) in known for x in c.tolist())
    cfg = str(tmp_path / "config.yaml")
    yaml.safe_dump({"sfm2gt": np.eye(4).tolist(), "eval_bbx": [[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]]}, open(cfg, "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_mesh.py"), "--file_pred", out, "--file_trgt", cloud,
                        "--scene_config_path", cfg, "--mesh", "--threshold", str(voxel), "--exact_recall", "--sample_surface"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    import json

    m = json.load(open(str(tmp_path / "eval_eval" / "metrics.json")))
    print("tool: recall %s precision %s at %s" % (m["recals"], m["precs"], m["thresholds"]))
    assert m["recals"] == [1.0]
