"""GPU: the reprojection visibility filter (neuralrecon_w_amd.reproj, scripts/reproj_filter.py, scripts/eval_pipeline.py).
(a) the golden depth maps of tests/golden/reproj_scene through our back-projection and marking give the reference's rows;
(b) end to end on a scene with surfaces no camera sees (an object on a ground plane seen from above, a sphere hidden behind
    a wall), against a float64 restatement (tests/_raster_oracle.py depth + float64 back-projection + brute-force 1-NN);
(c) the evaluation pipeline on that scene laid out as a Heritage-Recon scene.
Marking is exact up to fp32 rounding: vertices whose best distance lies within BAND of 2 sqrt(2) voxel_size, or that tie
with another vertex within BAND, may go either way; in (b) pixels the oracle does not call robust may too."""
import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import _raster_oracle as O
from tests._util import GOLDEN, ROOT

from neuralrecon_w_amd import evalmesh, reproj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 1e-5


def _marks(points, xyz, thr, band=BAND, slack=None):
    """(must, may) bool [V]: must = the nearest vertex of a point, closer than thr - band and clear of the runner-up by band;
    may = any vertex within thr + band of a point and within band of its nearest (slack[i] widens both for point i)."""
    must = np.zeros(len(xyz), bool)
    may = np.zeros(len(xyz), bool)
    if len(points) == 0:
        return must, may
    sl = np.zeros(len(points)) if slack is None else slack
    for s in range(0, len(points), 1024):
        p = points[s:s + 1024]
        d = np.sqrt(((p[:, None] - xyz[None]) ** 2).sum(-1))
        srt = np.sort(d, 1)
        i = np.argmin(d, 1)
        ok = (srt[:, 0] < thr - band) & (srt[:, 1] - srt[:, 0] > band) & (sl[s:s + 1024] == 0)
        must[i[ok]] = True
        cand = (d < thr + band + sl[s:s + 1024, None]) & (d <= srt[:, :1] + band + 2 * sl[s:s + 1024, None])
        may |= cand.any(0)
    return must, may


def _row_index(xyz, rows):
    """Indices of the vertices (xyz) equal to the rows' coordinates."""
    d = np.abs(rows[:, None, :3] - xyz[None]).max(-1)
    j = np.argmin(d, 1)
    assert (d[np.arange(len(rows)), j] <= 1e-12).all()
    return j


def test_golden_depths_through_our_backprojection_and_marking():
    g = np.load(os.path.join(GOLDEN, "reproj_golden.npz"))
    scene = os.path.join(GOLDEN, "reproj_scene")
    dz = np.load(os.path.join(scene, "depth.npz"))
    S = reproj.read_sfm2gt(scene)
    views = reproj.load_views(scene, S)
    verts, _, rgb = reproj.read_ply_mesh(os.path.join(scene, "mesh.ply"))
    xyz = evalmesh.apply_transform(verts, S)
    thr = 2 * math.sqrt(2) * float(g["voxel_size"])
    tgt = reproj.Target(xyz, rgb, thr, torch.device(DEV))
    pts64 = []
    for v in views:
        depth = dz["view_%d" % v["id"]]
        pts, pix = reproj.backproject(torch.from_numpy(depth).to(DEV), reproj.backproject_matrix(v["K"], v["pose"], tgt.centre))
        ref = O.backproject(depth.astype(np.float64), v["K"], v["pose"])
        assert pts.shape[0] == ref.shape[0] > 100
        assert np.abs(pts.double().cpu().numpy() + tgt.centre - ref).max() < 1e-5
        pts64.append(ref)
        tgt.mark(pts)
    got_xyz, got_rgb = tgt.rows()
    rows = g["rows"]
    assert np.array_equal(np.round(rows[:, 3:] * 255).astype(np.uint8), rgb[_row_index(xyz, rows)])
    got = np.zeros(len(xyz), bool)
    got[_row_index(xyz, np.c_[got_xyz, got_rgb])] = True
    ref = np.zeros(len(xyz), bool)
    ref[_row_index(xyz, rows)] = True
    must, may = _marks(np.concatenate(pts64), xyz, thr)
    assert (must <= ref).all() and (ref <= may).all()  # the restatement agrees with the reference
    assert np.array_equal(got | (may & ~must), ref | (may & ~must)), np.flatnonzero(got != ref)
    assert 0 < got.sum() < len(xyz)
    # the rows come out sorted and unique, as np.unique(axis=0)
    out = np.c_[got_xyz, got_rgb.astype(np.float64)]
    assert np.array_equal(out, np.unique(out, axis=0))
    if np.array_equal(got, ref):
        assert np.array_equal(got_xyz, rows[:, :3])


# ---------------------------------------------------------------------------------------------------
# (b) / (c): a scene with hidden surfaces
# ---------------------------------------------------------------------------------------------------
def _grid(verts, faces, origin, u, v, n):
    base = len(verts)
    for i in range(n + 1):
        for j in range(n + 1):
            verts.append(origin + u * (i / n) + v * (j / n))
    for i in range(n):
        for j in range(n):
            a, b, c, d = base + i * (n + 1) + j, base + (i + 1) * (n + 1) + j, base + (i + 1) * (n + 1) + j + 1, base + i * (n + 1) + j + 1
            faces += [(a, b, c), (a, c, d)]  # normal = u x v


def _hidden_scene():
    """SfM frame: ground z = 0 over [-2, 2]^2, a box on it, a wall y = 1 facing -y, a sphere behind the wall.  Returns
    (verts float32, faces, labels: 0 ground, 1 box, 2 wall, 3 sphere)."""
    verts, faces, lab = [], [], []
    e = np.eye(3)

    def add(fn, label):
        n0 = len(verts)
        fn()
        lab.extend([label] * (len(verts) - n0))

    add(lambda: _grid(verts, faces, np.array([-2.0, -2.0, 0.0]), 4 * e[0], 4 * e[1], 16), 0)
    b, h, lo = 0.4, 0.5, np.array([-0.4, -0.9, 0.0])
    add(lambda: (_grid(verts, faces, lo + [0, 0, h], 2 * b * e[0], 2 * b * e[1], 3),
                 _grid(verts, faces, lo, 2 * b * e[1], 2 * b * e[0], 3),
                 _grid(verts, faces, lo, 2 * b * e[0], h * e[2], 3),
                 _grid(verts, faces, lo + [0, 2 * b, 0], h * e[2], 2 * b * e[0], 3),
                 _grid(verts, faces, lo, h * e[2], 2 * b * e[1], 3),
                 _grid(verts, faces, lo + [2 * b, 0, 0], 2 * b * e[1], h * e[2], 3)), 1)
    add(lambda: _grid(verts, faces, np.array([-1.4, 1.0, 0.0]), 2.8 * e[0], 1.6 * e[2], 6), 2)  # normal -y
    n0 = len(verts)
    nu, nv, c, r = 16, 10, np.array([0.0, 1.5, 0.45]), 0.3
    for i in range(nv + 1):
        th = math.pi * i / nv
        for j in range(nu):
            ph = 2 * math.pi * j / nu
            verts.append(c + r * np.array([math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)]))
    for i in range(nv):
        for j in range(nu):
            a, b2, cc, d = n0 + i * nu + j, n0 + i * nu + (j + 1) % nu, n0 + (i + 1) * nu + (j + 1) % nu, n0 + (i + 1) * nu + j
            faces += [(a, d, cc), (a, cc, b2)]  # outward
    lab.extend([3] * (len(verts) - n0))
    return np.array(verts, np.float32), np.array(faces), np.array(lab)


SFM2GT = np.eye(4)
SFM2GT[:3, :3] = 1.5 * np.array([[math.cos(0.4), -math.sin(0.4), 0], [math.sin(0.4), math.cos(0.4), 0], [0, 0, 1]])
SFM2GT[:3, 3] = [3.0, -1.0, 0.5]
CAMS = [(160, 120, [150.0, 152.0, 81.3, 58.7], (0.6, -3.0, 3.6)), (128, 128, [120.0, 118.0, 62.2, 66.1], (-0.8, -2.6, 3.9)),
        (160, 120, [150.0, 152.0, 81.3, 58.7], (0.0, -2.2, 4.2))]


def _look_at(C, T):
    """World -> camera (OpenCV axes) of a camera at C looking at T, z up."""
    z = np.asarray(T, dtype=np.float64) - C
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 0.0, -1.0]), z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ np.asarray(C, dtype=np.float64)


def _qvec(R):
    """(w, x, y, z) of a rotation with trace > -1 (all cameras here)."""
    w = math.sqrt(max(0.0, 1.0 + np.trace(R))) / 2
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def _write_workspace(root, S):
    sp = os.path.join(root, "dense", "sparse")
    os.makedirs(sp, exist_ok=True)
    views = []
    with open(os.path.join(sp, "cameras.bin"), "wb") as fc, open(os.path.join(sp, "images.bin"), "wb") as fi:
        fc.write(struct.pack("<Q", len(CAMS)))
        fi.write(struct.pack("<Q", len(CAMS)))
        for k, (w, h, p, C) in enumerate(CAMS):
            fc.write(struct.pack("<iiQQ4d", k + 1, 1, w, h, *p))
            R, t = _look_at(np.array(C), (0.0, 0.2, 0.0))
            fi.write(struct.pack("<i7di", k + 1, *_qvec(R), *t, k + 1) + ("v%d.jpg" % k).encode() + b"\0" + struct.pack("<Q", 0))
    with open(os.path.join(root, "scene.tsv"), "w") as fh:
        fh.write("filename\tid\tsplit\n" + "".join("v%d.jpg\t%d\ttrain\n" % (k, k) for k in range(len(CAMS))))
    with open(os.path.join(root, "config.yaml"), "w") as fh:
        yaml.safe_dump({"sfm2gt": np.asarray(S).tolist(), "eval_bbx": [[-10.0, -10.0, -3.0], [10.0, 10.0, 6.0]]}, fh)
    return reproj.load_views(root, S)


def _restatement(verts, faces, views, xyz, thr):
    """float64: oracle depth per view, back-projection, (must, may) marks; non-robust pixels only widen `may`."""
    pts, slack = [], []
    for v in views:
        w, h = v["wh"]
        o = O.rasterize(verts, faces, v["K"].astype(np.float64), v["E"], h, w)
        p = O.backproject(o["depth"], v["K"], v["pose"])
        rob = o["robust"][o["depth"] > 0]
        pts.append(p)
        slack.append(np.where(rob, 0.0, 0.2))  # a non-robust pixel may land on a neighbouring face: widen by its footprint
    return _marks(np.concatenate(pts), xyz, thr, slack=np.concatenate(slack))


def test_filter_end_to_end_removes_hidden_surfaces(tmp_path):
    verts, faces, lab = _hidden_scene()
    root = str(tmp_path / "scene")
    views = _write_workspace(root, SFM2GT)
    mesh_file = str(tmp_path / "mesh.ply")
    rgb = (np.arange(len(verts))[:, None] * np.array([7, 13, 29]) % 256).astype(np.uint8)
    from neuralrecon_w_amd import mesh as M

    M.write_ply(mesh_file, torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(rgb))
    voxel = 0.02
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "reproj_filter.py"), "--src_file", mesh_file, "--target_file",
                        mesh_file, "--data_path", root, "--output_path", out, "--voxel_size", str(voxel), "--visualize",
                        "--n_cpus", "4", "--n_gpus", "4"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    gx, _, gc = reproj.read_ply_mesh(os.path.join(out, "reprojected.ply"))
    xyz = evalmesh.apply_transform(verts.astype(np.float64), SFM2GT)
    got = np.zeros(len(xyz), bool)
    j = _row_index(xyz, gx)
    got[j] = True
    assert np.array_equal(gc, rgb[j])
    must, may = _restatement(verts, faces, views, xyz, 2 * math.sqrt(2) * voxel)
    assert (got <= may).all(), np.flatnonzero(got & ~may)
    assert (must <= got).all(), np.flatnonzero(must & ~got)
    assert not got[lab == 3].any()  # the sphere behind the wall
    assert got[lab == 0].sum() > 100 and got[lab == 2].sum() > 10 and got.sum() < len(xyz)
    for k in range(len(CAMS)):
        d = np.load(os.path.join(out, "render", "depth", "v%d.npy" % k))
        assert d.shape == (CAMS[k][1], CAMS[k][0]) and (d > 0).mean() > 0.5
        assert os.path.isfile(os.path.join(out, "render", "reprojects", "v%d.ply" % k))


def test_eval_pipeline_on_a_heritage_layout(tmp_path):
    verts, faces, lab = _hidden_scene()
    scene = "brandenburg_gate"  # its SfM crop voxel (2) keeps the hidden surfaces in the unfiltered score
    root = str(tmp_path / "data")
    sdir = os.path.join(root, scene)
    _write_workspace(sdir, np.eye(4))  # identity sfm2gt: the two steps chain only then (eval_mesh applies sfm2gt again)
    from neuralrecon_w_amd import mesh as M

    pred = str(tmp_path / "run")
    os.makedirs(os.path.join(pred, "mesh"))
    M.write_ply(os.path.join(pred, "mesh", "extracted_mesh_level_10_colored.ply"), torch.from_numpy(verts),
                torch.from_numpy(faces), torch.zeros(len(verts), 3, dtype=torch.uint8))
    # GT: points sampled on the visible surfaces only (ground outside the box's footprint, box top, wall front)
    rng = np.random.RandomState(4)
    g = rng.uniform(-2, 2, (30000, 2))
    g = g[~((np.abs(g[:, 0]) < 0.4) & (g[:, 1] > -0.9) & (g[:, 1] < -0.1)) & (g[:, 1] < 1.0)]
    top = np.c_[rng.uniform(-0.4, 0.4, (3000, 2)) + [0, -0.5], np.full(3000, 0.5)]
    wall = np.c_[rng.uniform(-1.4, 1.4, 4000), np.full(4000, 1.0), rng.uniform(0, 1.6, 4000)]
    gt = np.concatenate([np.c_[g, np.zeros(len(g))], top, wall])
    M.write_ply(os.path.join(sdir, scene + ".ply"), torch.from_numpy(gt), torch.zeros(0, 3, dtype=torch.int64))
    os.makedirs(os.path.join(sdir, "neuralsfm"))
    sfm = gt[rng.choice(len(gt), 400, replace=False)]
    with open(os.path.join(sdir, "neuralsfm", "points3D.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(sfm)))
        for i, p in enumerate(sfm):
            fh.write(struct.pack("<QdddBBBd", i + 1, *p, 1, 2, 3, 0.5) + struct.pack("<Q", 20) + struct.pack("<40i", *([1, i] * 20)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_pipeline.py"), "--scene_name", scene, "--pred_dir", pred,
                        "--data_root", root], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.path.isfile(os.path.join(pred, "mesh", "reprojected.ply"))
    filt = json.load(open(os.path.join(pred, "mesh", "eval_%s_reprojected.ply" % scene, "metrics.json")))
    assert filt["thresholds"] == evalmesh.parse_thresholds(reproj.SCENES[scene]["thresholds"])
    with open(os.path.join(sdir, "config.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    sc = reproj.SCENES[scene]
    evalmesh.eval_mesh(os.path.join(pred, "mesh", "extracted_mesh_level_10_colored.ply"), os.path.join(sdir, scene + ".ply"), cfg,
                       True, threshold=filt["thresholds"], save_name="unfiltered", verbose=False,
                       sfm={"path": os.path.join(sdir, "neuralsfm"), "track_length": sc["track_length"],
                            "reproj_error": sc["reproj_error"], "voxel_size": sc["voxel_size"]})
    raw = json.load(open(os.path.join(pred, "mesh", "eval_unfiltered", "metrics.json")))
    k = int(np.argmin(np.abs(np.array(filt["thresholds"]) - 0.05)))
    assert filt["precs"][k] > raw["precs"][k] + 0.02, (filt["precs"][k], raw["precs"][k])
