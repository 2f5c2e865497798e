"""Depth / normal scores on the GPU (csrc/ncw_depthmetrics.hip, neuralrecon_w_amd/depthmetrics.py, scripts/eval_depth.py):
  1 the kernel bit for bit against the numpy restatement (tests/_depthmetrics_ref.py): row, histograms and the three planes,
    over the sizes where the lane / wave / block layout changes, both modes, every NULL input, degenerate and edge content;
  2 planes from the rasteriser: a mesh against itself, a plane against the same plane moved along the optical axis, and against
    the same plane tilted;
  3 a sphere-traced analytic sphere against a rasterised icosphere (the t -> z conversion and `scale`);
  4 the tool on a generated scene."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from neuralrecon_w_amd import depthmetrics as DM
from neuralrecon_w_amd import ply, reproj, synth, views
from tests import _depthmetrics_ref as R
from tests._build import build_system
from tests._util import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32

SIZES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (1, 256), (1, 257), (13, 17), (48, 64)]   # (H, W); 48 x 64 = 2 blocks
REL_EDGES = np.unique(np.concatenate([np.geomspace(1e-3, 4.0, 200), [0.25]]))
ANGLE_STEP = 0.5


def _camera(H, W):
    a, b = 0.3, -0.2
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    c2w = np.concatenate([Rx @ Ry, [[0.1], [0.2], [0.3]]], 1)
    return views.Camera([[41.3, 0, W / 2 - 0.3], [0, 39.8, H / 2 + 0.2], [0, 0, 1]], c2w, W, H, 0.1, 10.0)


def _content(H, W, seed, mode, cam, scale, cos_e):
    """Planes with every kind of pixel: valid pairs, empty / NaN / inf / negative / zero values in each input, zero and NaN
    normals, z_p == z_g, and (mode z) r on a table edge, q on a delta threshold, c on a table edge and on a threshold."""
    n = H * W
    g = np.random.RandomState(seed)
    zg = g.uniform(0.5, 4.0, n).astype(f32)
    zp = (zg * g.uniform(0.7, 1.4, n)).astype(f32)
    gn = g.normal(size=(3, n))
    gn = (gn / np.linalg.norm(gn, axis=0)).astype(f32)
    pn = gn + 0.2 * g.normal(size=(3, n))
    pn = (pn / np.linalg.norm(pn, axis=0)).astype(f32)
    dt, ct = R.thresholds()
    special = [(2.0, 2.5, 1.0), (1.0, dt[0], cos_e[3]), (1.0, dt[1], ct[0]), (1.0, dt[2], ct[1]), (3.0, 3.0, ct[2]), (1.0, 1.0, cos_e[0]),
               (2.0, 1.5, -1.0), (1.0, 1e-3, 0.0), (1e-3, 1.0, cos_e[-1])]
    for k, (a, b, c) in enumerate(special):
        i = (7 * k + 3) % n
        zg[i], zp[i] = a, b
        gn[:, i], pn[:, i] = (0, 0, 1), (0.25, 0, c)
    for k, (arr, val) in enumerate([(zg, 0), (zp, 0), (zg, np.nan), (zp, np.nan), (zg, np.inf), (zp, np.inf), (zg, -1), (zp, -2),
                                    (zg, -np.inf), (zp, -0.0)]):
        arr[(11 * k + 5) % n::23] = val
    pn[:, (4 % n)::29] = 0
    gn[:, (6 % n)::31] = 0
    gn[1, (8 % n)::37] = np.nan
    pn[2, (9 % n)::41] = np.inf
    mask = (g.rand(n) < 0.2).astype(np.uint8)
    mask[(10 % n)::43] = 200
    pred, pred_n, nrm = zp, pn, None
    if mode == R.PRED_T:
        nrm = R.ray_norm(cam.K, cam.c2w, H, W)
        with np.errstate(all="ignore"):
            pred = (zp * nrm / f32(scale)).astype(f32)
            pred_n = (pn / 2 + f32(0.5)).astype(f32)
    return zg, pred, gn, pred_n, mask, nrm


def _dev(a, shape):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).reshape(shape).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _check(sc, v, H, W, zg, pred, gn, pn, mask, mode, cam, scale, nrm):
    planes = sc.score(v, _dev(zg, (H, W)), _dev(pred, (H, W)), gt_n=_dev(gn, (3, H, W)), pred_n=_dev(pn, (3, H, W)),
                      mask=_dev(mask, (H, W)), mode="t" if mode == R.PRED_T else "z", camera=cam, scale=scale, want_planes=True)
    row, ref = R.compare(zg, pred, sc.cos_edges_host, sc.rel_edges_host, gt_n=gn, pred_n=pn, mask=mask, mode=mode, nrm=nrm, scale=scale)
    want = torch.from_numpy(R.words(row, sc.nr, sc.na))
    got = sc.table[v].cpu()
    assert torch.equal(got, want), [(i, int(got[i]), int(want[i])) for i in torch.nonzero(got != want).reshape(-1)[:8].tolist()]
    for k in ("err_rel", "err_cos", "z_pred"):
        assert torch.equal(_bits(planes[k]).reshape(-1), torch.from_numpy(ref[k].view(np.int32))), k
    return row


@pytest.mark.parametrize("H,W", SIZES)
def test_kernel_against_the_restatement(H, W):
    sc = DM.ViewScorer(1, ANGLE_STEP, REL_EDGES, DEV)
    cam, scale = _camera(H, W), 2.5
    scored = 0
    for mode in (R.PRED_Z, R.PRED_T):
        zg, pred, gn, pn, mask, nrm = _content(H, W, 100 * H + W, mode, cam, scale, sc.cos_edges_host)
        for with_gn in (True, False):
            for with_pn in (True, False):
                for with_mask in (True, False):
                    row = _check(sc, 0, H, W, zg, pred, gn if with_gn else None, pn if with_pn else None, mask if with_mask else None,
                                 mode, cam, scale, nrm)
                    assert with_gn and with_pn or row["normals"] == 0
                    scored += row["normals"]
    assert H * W < 64 or scored > 0


@pytest.mark.parametrize("mode", [R.PRED_Z, R.PRED_T])
def test_kernel_against_the_restatement_many_blocks(mode):
    """1024 x 768 = 384 workgroups: more rows of partials than the fold has lanes, so lanes 0 .. 127 add two rows each before the
    tree -- the second level of the order."""
    H, W = 768, 1024
    assert (H * W + R.BLOCK - 1) // R.BLOCK > R.LANES
    sc = DM.ViewScorer(1, ANGLE_STEP, REL_EDGES, DEV)
    cam, scale = _camera(H, W), 2.5
    zg, pred, gn, pn, mask, nrm = _content(H, W, 77, mode, cam, scale, sc.cos_edges_host)
    row = _check(sc, 0, H, W, zg, pred, gn, pn, mask, mode, cam, scale, nrm)
    assert row["both"] > 300000 and row["normals"] > 250000


@pytest.mark.parametrize("mode", [R.PRED_Z, R.PRED_T])
def test_degenerate_views(mode):
    H, W = 13, 17
    sc = DM.ViewScorer(1, ANGLE_STEP, REL_EDGES, DEV)
    cam, scale = _camera(H, W), 2.5
    zg, pred, gn, pn, mask, nrm = _content(H, W, 5, mode, cam, scale, sc.cos_edges_host)
    zero = np.zeros(H * W, dtype=f32)
    r = _check(sc, 0, H, W, zero, pred, gn, pn, mask, mode, cam, scale, nrm)             # all-empty GT
    assert r["both"] == r["gt_only"] == 0 and r["pred_only"] > 0
    r = _check(sc, 0, H, W, zg, zero, gn, pn, mask, mode, cam, scale, nrm)               # all-empty prediction
    assert r["both"] == r["pred_only"] == 0 and r["gt_only"] > 0
    r = _check(sc, 0, H, W, zg, pred, gn, pn, np.ones(H * W, np.uint8), mode, cam, scale, nrm)   # everything masked
    assert r["masked"] == H * W and r["both"] + r["gt_only"] + r["pred_only"] + r["neither"] == 0
    same = np.where(np.isfinite(zg) & (zg > 0), zg, f32(1)).astype(f32)                  # z_p == z_g everywhere: q = 1, e = 0
    if mode == R.PRED_Z:
        r = _check(sc, 0, H, W, same, same, gn, gn, None, mode, cam, scale, nrm)
        assert r["both"] == r["delta1"] == H * W and r["sum_abs"] == 0.0 and r["sum_sq"] == 0.0 and r["hist_rel"][0] == H * W


@pytest.mark.parametrize("angle_step,rel_edges", [(90.0, [0.1]), (180.0 / 2049, np.geomspace(1e-4, 10, 2048)), (90.0, np.geomspace(1e-4, 10, 2048)),
                                                  (180.0 / 2049, [0.1])])
def test_table_sizes(angle_step, rel_edges):
    H, W = 48, 64
    sc = DM.ViewScorer(1, angle_step, rel_edges, DEV)
    assert (sc.na, sc.nr) == (1 if angle_step == 90.0 else 2048, len(rel_edges))
    cam = _camera(H, W)
    zg, pred, gn, pn, mask, nrm = _content(H, W, 9, R.PRED_Z, cam, 1.0, sc.cos_edges_host if sc.na > 3 else np.zeros(4, f32))
    r = _check(sc, 0, H, W, zg, pred, gn, pn, mask, R.PRED_Z, cam, 1.0, nrm)
    assert r["hist_rel"].sum() == r["both"] > 1000 and r["hist_cos"].sum() == r["normals"] > 1000


def test_repeatable_and_rows_apart():
    H, W = 48, 64
    sc = DM.ViewScorer(3, ANGLE_STEP, REL_EDGES, DEV)
    cam = _camera(H, W)
    zg, pred, gn, pn, mask, nrm = _content(H, W, 3, R.PRED_T, cam, 2.5, sc.cos_edges_host)
    sentinel = torch.arange(3 * sc.K, dtype=torch.int64, device=DEV).reshape(3, sc.K) * 7919 + 13
    sc.table.copy_(sentinel)
    _check(sc, 1, H, W, zg, pred, gn, pn, mask, R.PRED_T, cam, 2.5, nrm)   # row 1 is what the restatement gives, whatever it held
    first = sc.table.clone()
    assert torch.equal(first[0], sentinel[0]) and torch.equal(first[2], sentinel[2])
    for _ in range(2):
        _check(sc, 1, H, W, zg, pred, gn, pn, mask, R.PRED_T, cam, 2.5, nrm)
        assert torch.equal(sc.table, first)
    rows = sc.rows()
    assert rows[1]["both"] > 1000 and rows[1]["sum_rel"] > 0


def test_bad_arguments():
    z = torch.ones(4, 5, device=DEV)
    with pytest.raises(DM.L.NeuconwHipError):
        DM.compare_planes(z.cpu(), z.cpu())
    with pytest.raises(ValueError):
        DM.compare_planes(z, z[:3])
    with pytest.raises(ValueError):
        DM.compare_planes(z, z, mode="t")                      # no camera
    with pytest.raises(ValueError):
        DM.compare_planes(z, z, mode="t", camera=_camera(5, 4))   # another size
    with pytest.raises(ValueError):
        DM.compare_planes(z, z, scale=0.0)
    row, planes = DM.compare_planes(z, z, want_planes=True)
    assert row["both"] == 20 and row["sum_abs"] == 0.0 and tuple(planes["z_pred"].shape) == (4, 5)


# ---------------------------------------------------------------------------------------------------
# 2. planes from the rasteriser
# ---------------------------------------------------------------------------------------------------
def _icosphere(sub, radius, centre):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(sub):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(centre, dtype=np.float64), np.array(f, dtype=np.int64)


K0 = np.array([[40.0, 0, 16.0], [0, 40.0, 12.0], [0, 0, 1]])
H0, W0 = 24, 32


def _quad(z0, alpha=0.0):
    """A 20 x 20 quad through (0, 0, z0), facing the camera at the origin, tilted by alpha about the image's x axis."""
    c, s = math.cos(alpha), math.sin(alpha)
    v = np.array([[x, y * c, z0 + y * s] for x, y in ((-10, -10), (10, -10), (10, 10), (-10, 10))], dtype=np.float64)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    n = np.tile(np.array([[0.0, s, -c]]), (2, 1))
    return v, f, n


def _quad_planes(z0, alpha=0.0):
    v, f, n = _quad(z0, alpha)
    return DM.gt_planes_from_mesh(reproj.RasterMesh(v, f, DEV), n, K0, np.eye(4), H0, W0, cull="none", znear=0.01, zfar=100.0)


def test_a_mesh_against_itself():
    v, f = _icosphere(2, 1.0, (0.1, -0.05, 4.0))
    n, _ = synth.face_normals(v, f)
    gz, gn = DM.gt_planes_from_mesh(reproj.RasterMesh(v, f, DEV), n, K0, np.eye(4), H0, W0, znear=0.01, zfar=100.0)
    row = DM.compare_planes(gz, gz, gt_n=gn, pred_n=gn)
    s = DM.summarise([row])["pooled"]
    assert 100 < row["both"] < H0 * W0 and row["gt_only"] == row["pred_only"] == 0 and row["neither"] == H0 * W0 - row["both"]
    assert all(row[k] == 0.0 for k in ("sum_abs", "sum_err", "sum_sq", "sum_rel", "sum_sq_rel"))
    assert row["hist_rel"][0] == row["both"] == row["delta1"] and row["normals"] == row["both"] == row["hist_cos"][0] == row["ang1"]
    assert s["completeness"] == 1.0 and s["extra"] == 0.0 and s["abs_rel"] == 0.0 and s["rmse"] == 0.0
    # the normals look at the camera under either culling
    gz2, gn2 = DM.gt_planes_from_mesh(reproj.RasterMesh(v, f[:, ::-1].copy(), DEV), -n, K0, np.eye(4), H0, W0, cull="none", znear=0.01,
                                      zfar=100.0)
    r2 = DM.compare_planes(gz, gz2, gt_n=gn, pred_n=gn2)
    assert r2["normals"] == r2["both"] > 100 and r2["hist_cos"][0] == r2["normals"]


def test_a_plane_moved_along_the_optical_axis():
    """bias = d and abs-rel = d / z.  A rasterised depth carries at most 16 float32 roundings (vertex transform, edge functions,
    interpolation): relative error 16 * 2^-24 per plane; e = z_p - z_g adds one more rounding of d."""
    z0, d = 4.0, 0.5
    (gz, gn), (pz, pn) = _quad_planes(z0), _quad_planes(z0 + d)
    row = DM.compare_planes(gz, pz, gt_n=gn, pred_n=pn)
    s = DM.summarise([row])["pooled"]
    tol = 16 * 2.0 ** -24 * (2 * z0 + d) + 2.0 ** -24 * d
    print("moved plane: bias %.9g (d %.9g), abs_rel %.9g (d / z %.9g), tol %.3g" % (s["bias"], d, s["abs_rel"], d / z0, tol))
    assert row["both"] == H0 * W0 and s["completeness"] == 1.0
    assert abs(s["bias"] - d) <= tol and abs(s["mae"] - d) <= tol and abs(s["abs_rel"] - d / z0) <= tol / z0 * (1 + 2.0 ** -20)
    assert row["delta1"] == H0 * W0 and row["hist_cos"][0] == row["normals"] == H0 * W0


def test_a_tilted_plane():
    alpha = 10.05   # the middle of angle bin 100 of the default 0.1 degree table
    (gz, gn), (pz, pn) = _quad_planes(4.0), _quad_planes(4.0, math.radians(alpha))
    row = DM.compare_planes(gz, pz, gt_n=gn, pred_n=pn)
    b = int(math.ceil(alpha / 0.1)) - 1
    assert b == 100 and row["normals"] == row["both"] == H0 * W0
    assert row["hist_cos"][b - 1:b + 2].sum() == H0 * W0
    s = DM.summarise([row])["pooled"]
    assert abs(s["median_angle"] - alpha) <= 0.15 and s["angle_within_11.25"] == 1.0


# ---------------------------------------------------------------------------------------------------
# 3. a traced analytic sphere against a rasterised icosphere
# ---------------------------------------------------------------------------------------------------
def test_traced_sphere_against_icosphere():
    """|z_p - z_g| <= 2 (radius - smallest face-plane distance) + eps in SfM units where the incidence cosine exceeds 0.5: the
    icosphere lies inside the sphere by at most that deficiency along the normal, at most twice that along such a ray."""
    origin, radius, rho, eps = np.array([0.3, -0.2, 0.1]), 2.0, 0.5, 1e-4
    rdr = build_system(W=64, origin=origin.tolist(), radius=radius)[3]
    Rs = rho * radius
    H, W = 48, 64
    K = np.array([[90.0, 0, 31.5], [0, 90.0, 23.5], [0, 0, 1]])
    # OpenCV camera 4 SfM units from the sphere's centre, looking at it, slightly rolled
    fwd = np.array([0.2, 1.0, -0.1])
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.05, 0.0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c2w_cv = np.concatenate([np.stack([right, down, fwd], 1), (origin - 4.0 * fwd)[:, None]], 1)
    w2c = np.linalg.inv(np.concatenate([c2w_cv, [[0, 0, 0, 1]]], 0))
    c2w = c2w_cv.copy()
    c2w[:, 1:3] *= -1
    cam = views.Camera(K, c2w, W, H, 1.0, 8.0)
    sdf = lambda p: p.norm(dim=1) - rho  # noqa: E731  (unit-sphere frame: the sphere |x| = rho)
    pz, pn, out = DM.pred_planes_from_trace(rdr, cam, 0, sdf_fn=sdf, shade=False, eps=eps, max_iter=64)
    assert pn is None and out["stats"]["hit"] > 500
    v, f = _icosphere(3, Rs, origin)
    n, _ = synth.face_normals(v, f)
    deficiency = Rs - float(np.abs((n * (v[f[:, 0]] - origin)).sum(1)).min())   # float64
    assert 0 < deficiency < 0.01 * Rs
    gz, gn = DM.gt_planes_from_mesh(reproj.RasterMesh(v, f, DEV), n, K, w2c, H, W, znear=0.01, zfar=100.0)
    row, planes = DM.compare_planes(gz, pz, mode="t", camera=cam, scale=radius, want_planes=True)
    zp, zg, gnh = planes["z_pred"].cpu().numpy().astype(np.float64), gz.cpu().numpy().astype(np.float64), gn.cpu().numpy().astype(np.float64)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(c - K[0, 2]) / K[0, 0], (r - K[1, 2]) / K[1, 1], np.ones_like(c, dtype=np.float64)], 0)
    d /= np.linalg.norm(d, axis=0)
    cos_inc = np.abs((np.einsum("ij,jhw->ihw", w2c[:3, :3], gnh) * d).sum(0))
    both = (zp > 0) & (zg > 0)
    sel = both & (cos_inc > 0.5)
    bound = 2 * deficiency + eps * radius
    err = np.abs(zp - zg)[sel]
    print("traced sphere: %d pixels, max |z_p - z_g| %.3e, bound %.3e (deficiency %.3e)" % (sel.sum(), err.max(), bound, deficiency))
    assert sel.sum() > 500 and row["both"] == both.sum() and err.max() <= bound
    # gt_only / pred_only only within one pixel of the silhouette (a 3 x 3 neighbourhood holding both kinds of GT pixel)
    g = np.pad(zg > 0, 1, mode="edge")
    nb = np.stack([g[i:i + H, j:j + W] for i in range(3) for j in range(3)], 0)
    edge = nb.any(0) & ~nb.all(0)
    odd = (zp > 0) != (zg > 0)
    assert row["gt_only"] + row["pred_only"] == odd.sum() and not (odd & ~edge).any()
    # the conversion is what is pinned: a scale off by the radius, or t taken for z, is far outside the bound
    for kw in (dict(mode="t", camera=cam, scale=1.0), dict(mode="z")):
        _, p2 = DM.compare_planes(gz, pz if "camera" in kw else pz * radius, want_planes=True, **kw)
        assert np.abs(p2["z_pred"].cpu().numpy().astype(np.float64) - zg)[sel].max() > bound


# ---------------------------------------------------------------------------------------------------
# 4. the tool
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("depthmetrics") / "facade")
    synth.generate(root, seed=0, n_views=4, size=(64, 48), n_points=2000, n_gt=20000, ss=2, max_edge=2.0, num_test=1, pixel_sigma=0.5,
                   device=DEV)
    return root


def test_the_tool(scene_root, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import eval_depth
    import yaml

    root = scene_root
    mesh = os.path.join(root, "mesh.ply")
    out = str(tmp_path / "out")
    res = eval_depth.main(["--root_dir", root, "--pred_mesh", mesh, "--gt_mesh", mesh, "--split", "all", "--out", out, "--panels",
                           "--write_planes", "--device", DEV])
    saved = json.load(open(os.path.join(out, "metrics.json")))
    p = res["pooled"]
    assert len(saved["views"]) == 4 and saved["pooled"]["both"] == p["both"] > 1000 and set(saved["classes"]) == {
        "both", "gt_only", "pred_only", "neither", "masked"}
    assert p["abs_rel"] == 0.0 and p["rmse"] == 0.0 and p["mae"] == 0.0 and p["bias"] == 0.0 and p["sq_rel"] == 0.0
    assert p["completeness"] == 1.0 and p["extra"] == 0.0 and p["delta1"] == 1.0 and p["angle_within_11.25"] == 1.0
    person, n_person, n_pix = synth.labels.label_id("person"), 0, 0
    for v in saved["views"]:
        stem = os.path.splitext(v["name"])[0]
        lab = np.load(os.path.join(root, "semantic_maps", stem + ".npz"))["arr_0"]
        assert lab.shape == (v["height"], v["width"]) and v["row"]["masked"] == int((lab == person).sum())
        n_person += int((lab == person).sum())
        n_pix += lab.size
        z = np.load(os.path.join(out, stem + ".npz"))
        assert z["z_pred"].dtype == np.float32 and z["z_pred"].shape == lab.shape and np.array_equal(z["z_pred"], z["z_gt"])
        assert os.path.getsize(os.path.join(out, stem + ".png")) > 100
    assert p["masked"] == n_person > 0 and p["both"] + p["gt_only"] + p["pred_only"] + p["neither"] + p["masked"] == n_pix
    # the predicted mesh 0.05 GT units toward the cameras (they stand in front of the facade, at -y of the GT frame)
    S = np.array(yaml.safe_load(open(os.path.join(root, "config.yaml")))["sfm2gt"])
    v, f, _ = ply.read_mesh(mesh)
    shifted = str(tmp_path / "shifted.ply")
    ply.write(shifted, v + np.linalg.inv(S[:3, :3]) @ np.array([0.0, -0.05, 0.0]), faces=f)
    res2 = eval_depth.main(["--root_dir", root, "--pred_mesh", shifted, "--gt_mesh", mesh, "--split", "all", "--out", str(tmp_path / "out2"),
                            "--device", DEV])
    q = res2["pooled"]
    print("shifted mesh: bias %.5f  abs_rel %.5f  completeness %.4f" % (q["bias"], q["abs_rel"], q["completeness"]))
    assert q["bias"] < 0 and q["completeness"] >= 0.9 and q["masked"] == n_person


def test_truth_in_the_gt_frame_and_a_cloud_as_truth(scene_root, tmp_path):
    """eval_scene with the truth carried through sfm2gt (a similarity with a rotation and a scale of 3 .. 8).
    A GT-FRAME MESH, cull='none': the same views as the SfM-frame run.  The vertices go through float64 and are rounded to
    float32 in another frame, so depths agree to float32 rounding, far inside relative-error bin 0 (< 1e-4), except where a
    sample lies within rounding of a triangle edge at a depth discontinuity: at most 1 % of the pixels is allowed for that.
    Every normal is in angle bin 0 likewise -- with the normals oriented in a wrongly rotated frame a share of them flips to
    180 degrees.  Lengths are multiplied by the sfm2gt scale.
    A CLOUD (gt.ply), both frames: no normals; the voxel first hit precedes the surface by at most a voxel diagonal along the
    normal, twice that along a ray whose incidence cosine is >= 0.5 as it is for the median facade pixel, plus the 0.02 camera
    units the cloud renderer adds: the median |z_p - z_g| in GT units is within 2 sqrt(3) v + 0.02 s."""
    import yaml

    from neuralrecon_w_amd import evalmesh

    root = scene_root
    S = np.array(yaml.safe_load(open(os.path.join(root, "config.yaml")))["sfm2gt"])
    s_ = float(np.sqrt((S[0, :3] ** 2).sum()))
    assert 3 <= s_ <= 8 and np.abs(S[:3, :3] / s_ - np.eye(3)).max() > 0.1
    mesh = os.path.join(root, "mesh.ply")
    v, f, _ = ply.read_mesh(mesh)
    gt_mesh = str(tmp_path / "mesh_gt.ply")
    ply.write(gt_mesh, evalmesh.apply_transform(v, S), faces=f)
    kw = dict(pred="mesh", pred_mesh=mesh, split="all", cull="none", device=DEV)
    a = DM.eval_scene(root, gt_mesh=mesh, gt_frame="sfm", **kw)
    b = DM.eval_scene(root, gt_mesh=gt_mesh, gt_frame="gt", **kw)
    pa, pb = DM.pool_rows(a["rows"]), DM.pool_rows(b["rows"])
    assert a["unit_scale"] == 1.0 and b["unit_scale"] == pytest.approx(s_, rel=1e-12)
    assert pa["sum_abs"] == 0.0 and pa["hist_rel"][0] == pa["both"] > 1000 and pa["hist_cos"][0] == pa["normals"] == pa["both"]
    print("gt frame: both %d / %d, rel bin 0 %d, angle bin 0 %d of %d, masked %d / %d"
          % (pb["both"], pa["both"], pb["hist_rel"][0], pb["hist_cos"][0], pb["normals"], pb["masked"], pa["masked"]))
    assert pb["masked"] == pa["masked"] and abs(pb["both"] - pa["both"]) <= 0.01 * pa["both"] and pb["normals"] == pb["both"]
    assert pb["hist_rel"][0] >= 0.99 * pb["both"] and pb["hist_cos"][0] >= 0.99 * pb["normals"]
    sb = b["summary"]["pooled"]
    assert sb["mae"] == pytest.approx(s_ * pb["sum_abs"] / pb["both"], rel=1e-12) and sb["abs_rel"] == pytest.approx(pb["sum_rel"] / pb["both"], rel=1e-12)
    assert sb["completeness"] >= 0.99 and sb["angle_within_11.25"] >= 0.99

    vox = 0.25
    cloud_gt = os.path.join(root, "gt.ply")
    pts, _, _ = ply.read_mesh(cloud_gt)
    cloud_sfm = str(tmp_path / "gt_sfm.ply")
    ply.write(cloud_sfm, evalmesh.apply_transform(pts, np.linalg.inv(S)))
    both = {}
    for frame, path in (("gt", cloud_gt), ("sfm", cloud_sfm)):
        diffs = []

        def on_view(info):
            zp, zg = info["planes"]["z_pred"], info["gt_z"]
            m = torch.isfinite(info["planes"]["err_rel"])
            diffs.append((zp - zg).abs()[m].cpu().numpy())
        c = DM.eval_scene(root, gt_cloud=path, gt_frame=frame, voxel_size=vox, on_view=on_view, **kw)
        pc = DM.pool_rows(c["rows"])
        d = np.concatenate(diffs).astype(np.float64) * s_
        bound = 2 * math.sqrt(3.0) * vox + 0.02 * s_
        print("cloud as truth (%s frame): both %d gt_only %d pred_only %d, median |dz| %.4f GT units (bound %.4f)"
              % (frame, pc["both"], pc["gt_only"], pc["pred_only"], float(np.median(d)), bound))
        assert pc["normals"] == 0 and pc["hist_cos"].sum() == 0 and len(d) == pc["both"] > 1000 and pc["masked"] == pa["masked"]
        assert c["unit_scale"] == (pytest.approx(s_, rel=1e-12) if frame == "gt" else 1.0)
        assert float(np.median(d)) <= bound
        both[frame] = pc["both"]
    assert abs(both["gt"] - both["sfm"]) <= 0.02 * both["gt"]   # the same cloud up to a float64 round trip through sfm2gt
