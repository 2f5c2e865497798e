"""GPU: the mesh evaluation end to end (evalmesh.eval_mesh, scripts/eval_mesh.py, scripts/train.py --val_mesh_every) on a
predicted mesh from marching cubes of an analytic SDF and a GT cloud sampled from a slightly different surface, with a
non-identity sfm2gt (rotation, scale, translation), an eval box that cuts the surface, and an SfM crop from a COLMAP
points3D.bin written here.  Expected values: a float64 restatement (numpy crops + float64 brute-force distances)."""
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

from tests._util import ROOT

from neuralrecon_w_amd import evalmesh, mesh

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
DEV = "cuda:0"
C30, S30 = math.cos(math.pi / 6), math.sin(math.pi / 6)
SFM2GT = np.array([[2 * C30, -2 * S30, 0, 100.0], [2 * S30, 2 * C30, 0, -50.0], [0, 0, 2.0, 10.0], [0, 0, 0, 1]])


def _sphere(n, r, seed):
    rng = np.random.RandomState(seed)
    d = rng.randn(n, 3)
    return d / np.linalg.norm(d, axis=1, keepdims=True) * r


def _to_gt(p):
    return p @ SFM2GT[:3, :3].T + SFM2GT[:3, 3]


def _write_points3d(path, pts, tracks, errs):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(pts)))
        for i, (p, t, e) in enumerate(zip(pts, tracks, errs)):
            f.write(struct.pack("<QdddBBBd", i + 1, *p, 1, 2, 3, e))
            f.write(struct.pack("<Q", int(t)))
            f.write(struct.pack("<" + "ii" * int(t), *([1, i] * int(t))))


def _make_case(tmp):
    # predicted surface: marching cubes of a sphere of radius 0.5 (SfM units) on a 96^3 lattice over [-1, 1]^3
    D = 96
    g = torch.linspace(-1, 1, D, device=DEV)
    X, Y, Z = torch.meshgrid(g, g, g, indexing="ij")
    sdf = (torch.sqrt(X * X + Y * Y + Z * Z) - 0.5).contiguous()
    verts, faces = mesh.isosurface(sdf)
    verts_w = verts * (2.0 / (D - 1)) - 1.0
    pred = str(tmp / "pred" / "mesh.ply")
    os.makedirs(os.path.dirname(pred), exist_ok=True)
    mesh.write_ply(pred, verts_w, faces)
    # GT: a slightly larger sphere sampled in SfM units, carried to GT coordinates
    gt = str(tmp / "gt.ply")
    mesh.write_ply(gt, torch.from_numpy(_to_gt(_sphere(30000, 0.52, 1))), torch.zeros(0, 3, dtype=torch.int64))
    # SfM points near the surface with varied track length / error
    rng = np.random.RandomState(2)
    sp = _sphere(300, 0.5, 3) + rng.randn(300, 3) * 0.01
    _write_points3d(str(tmp / "sparse" / "points3D.bin"), sp, rng.randint(1, 8, 300), rng.uniform(0, 2, 300))
    c = SFM2GT[:3, 3]
    scene = {"sfm2gt": SFM2GT.tolist(), "eval_bbx": [(c - 1.3).tolist(), (c + [1.3, 1.3, 0.4]).tolist()]}
    return pred, gt, scene


def _expected(pred, gt, scene, ts, sfm=None):
    """float64 restatement of utils/eval_mesh.py:48-123 (use_o3d=False)."""
    lo, hi = np.array(scene["eval_bbx"][0]), np.array(scene["eval_bbx"][1])

    def crop(p):
        pn = (p - (lo + (hi - lo) / 2)) / ((hi - lo) / 2)
        return p[((pn > -1) & (pn < 1)).all(-1)]

    vt = crop(evalmesh.read_ply_points(gt))
    vp = evalmesh.read_ply_points(pred)
    vp = crop((SFM2GT[:3] @ np.c_[vp, np.ones(len(vp))].T).T)
    if sfm is not None:
        xyz, err, tr = [], [], []
        with open(os.path.join(sfm["path"], "points3D.bin"), "rb") as f:
            n = struct.unpack("<Q", f.read(8))[0]
            for _ in range(n):
                rec = struct.unpack("<QdddBBBd", f.read(43))
                t = struct.unpack("<Q", f.read(8))[0]
                f.read(8 * t)
                xyz.append(rec[1:4])
                err.append(rec[7])
                tr.append(t)
        xyz, err, tr = np.array(xyz), np.array(err), np.array(tr)
        s = xyz[(tr > sfm["track_length"]) & (err < sfm["reproj_error"])]
        s = (SFM2GT[:3] @ np.c_[s, np.ones(len(s))].T).T
        half = np.max(hi - lo) / 2
        ctr = lo + (hi - lo) / 2
        res = int(np.floor(2 * half / sfm["voxel_size"]))
        cell = lambda p: np.floor(res * ((p - ctr) / half + 1.0) / 2.0).astype(np.int64)  # noqa: E731
        cs = cell(s)
        occ = {tuple(c) for c in cs[((cs >= 0) & (cs < res)).all(-1)]}
        vp = vp[np.array([tuple(c) in occ for c in cell(vp)], dtype=bool)]
        vt = vt[np.array([tuple(c) in occ for c in cell(vt)], dtype=bool)]

    def nn(a, b):  # for every point of b its distance to a
        A, B = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        return torch.cat([((B[i:i + 512, None] - A[None]) ** 2).sum(-1).min(1).values.sqrt() for i in range(0, len(B), 512)]).cpu().numpy()

    d1, d2 = nn(vp, vt), nn(vt, vp)
    both = np.concatenate([vp, vt])
    bound = 8 * EPS32 * float(np.abs(both - (both.min(0) + both.max(0)) / 2).max())
    return d1, d2, bound, len(vp), len(vt)


def _compare(got_all, d1, d2, bound, ts):
    for t, got in zip(ts, got_all):
        for key, d in (("prec", d2), ("recal", d1)):
            lo_c, hi_c = int((d < t - bound).sum()), int((d < t + bound).sum())
            v = got[key] * len(d)
            assert lo_c - 1e-6 <= v <= hi_c + 1e-6 or (got[key] == 1e-6 and lo_c == 0), (t, key, v, lo_c, hi_c)
            if lo_c == hi_c:
                assert got[key] == max(lo_c / len(d), 1e-6), (t, key)
        if all(int((d < t - bound).sum()) == int((d < t + bound).sum()) for d in (d1, d2)):
            p, r = max((d2 < t).mean(), 1e-6), max((d1 < t).mean(), 1e-6)
            assert got["fscore"] == 2 * p * r / (p + r)
        assert abs(got["dist1"] - d2.mean()) <= 1e-6 * d2.mean() and abs(got["dist2"] - d1.mean()) <= 1e-6 * d1.mean()


def test_eval_mesh_matches_the_restatement(tmp_path):
    pred, gt, scene = _make_case(tmp_path)
    ts = [0.02, 0.04, 0.05, 0.08, 0.1, 0.2]
    m = evalmesh.eval_mesh(pred, gt, scene, is_mesh=True, threshold=ts, save_name="plain", verbose=False)
    d1, d2, bound, npred, ngt = _expected(pred, gt, scene, ts)
    assert 1000 < npred and 1000 < ngt
    out = os.path.join(os.path.dirname(pred), "eval_plain")
    allm = json.load(open(os.path.join(out, "metrics.json")))
    assert list(allm) == ["thresholds", "fscores", "precs", "recals"] and allm["thresholds"] == ts
    per = [json.load(open(os.path.join(out, "visualize", "%.2f" % t, "metrics.json"))) for t in ts]
    assert all(list(p) == ["dist1", "dist2", "prec", "recal", "fscore"] for p in per)
    assert [p["fscore"] for p in per] == allm["fscores"] and m == per[-1]
    _compare(per, d1, d2, bound, ts)
    assert 0.0 < per[0]["fscore"] < per[-1]["fscore"] and per[-1]["fscore"] > 0.9
    assert sorted(os.listdir(out)) == ["down_gt.ply", "down_pred_in_gt.ply", "metrics.json", "visualize"]
    assert evalmesh.read_ply_points(os.path.join(out, "down_gt.ply")).shape == (ngt, 3)
    assert evalmesh.read_ply_points(os.path.join(out, "down_pred_in_gt.ply")).shape == (npred, 3)


def test_eval_mesh_with_the_sfm_crop_and_the_command_line(tmp_path):
    pred, gt, scene = _make_case(tmp_path)
    ts = [0.03, 0.06, 0.1]
    sfm = {"path": str(tmp_path / "sparse"), "track_length": 3, "reproj_error": 1.0, "voxel_size": 0.3}
    evalmesh.eval_mesh(pred, gt, scene, is_mesh=True, threshold=ts, save_name="sfm", sfm=sfm, verbose=False)
    d1, d2, bound, npred, ngt = _expected(pred, gt, scene, ts, sfm)
    out = os.path.join(os.path.dirname(pred), "eval_sfm")
    assert sorted(os.listdir(out)) == ["down_gt.ply", "down_pred_in_gt.ply", "metrics.json", "pred_filtered.ply", "sfm_points.ply",
                                       "target_filtered.ply", "visualize"]
    assert evalmesh.read_ply_points(os.path.join(out, "pred_filtered.ply")).shape == (npred, 3)
    assert evalmesh.read_ply_points(os.path.join(out, "target_filtered.ply")).shape == (ngt, 3)
    assert 100 < npred and 100 < ngt
    per = [json.load(open(os.path.join(out, "visualize", "%.2f" % t, "metrics.json"))) for t in ts]
    _compare(per, d1, d2, bound, ts)
    cfg = str(tmp_path / "config.yaml")
    yaml.safe_dump(scene, open(cfg, "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_mesh.py"), "--file_pred", pred, "--file_trgt", gt,
                        "--scene_config_path", cfg, "--mesh", "--threshold", "0.03,0.11,0.03", "--sfm_path", sfm["path"],
                        "--track_lenth", "3", "--reproj_error", "1.0", "--voxel_size", "0.3", "--save_name", "cli"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    cli = json.load(open(os.path.join(os.path.dirname(pred), "eval_cli", "metrics.json")))
    assert cli["thresholds"] == [float(v) for v in np.arange(0.03, 0.11, 0.03)]
    ref = json.load(open(os.path.join(out, "metrics.json")))
    assert cli["fscores"][:2] == ref["fscores"][:2] and cli["precs"][:2] == ref["precs"][:2]  # 0.03, 0.06 in both runs


def _write_scene(root, n_chunks=2):
    """The synthetic Heritage-Recon scene directory of the training-driver test, plus eval_bbx_detail and gt.ply."""
    sys.path.insert(0, ROOT)
    import bench

    os.makedirs(os.path.join(root, "dense", "sparse"), exist_ok=True)
    rng = np.random.RandomState(0)
    d = rng.randn(400, 3)
    pts = d / np.linalg.norm(d, axis=1, keepdims=True) * 0.5
    with open(os.path.join(root, "dense", "sparse", "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(pts)))
        for i, p in enumerate(pts):
            f.write(struct.pack("<QdddBBBd", i + 1, *p, 1, 2, 3, 0.1))
            f.write(struct.pack("<Q", 3))
            f.write(struct.pack("<iiiiii", 1, i, 2, i, 3, i))
    yaml.safe_dump({"origin": [0.0, 0.0, 0.0], "radius": 1.0, "sfm2gt": np.eye(4).tolist(),
                    "eval_bbx": [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], "voxel_size": 0.125, "min_track_length": 2,
                    "eval_bbx_detail": [[-0.7, -0.7, -0.7], [0.7, 0.7, 0.7]]},
                   open(os.path.join(root, "config.yaml"), "w"))
    mesh.write_ply(os.path.join(root, "gt.ply"), torch.from_numpy(_sphere(5000, 0.5, 9)), torch.zeros(0, 3, dtype=torch.int64))
    labels = np.array([0, 1, 2, 4, 12, 20], dtype=np.float32)
    for i in range(n_chunks):
        rays, ts, label, rgbs = bench.synth_batch(300 + 40 * i, 50 + i, "cpu")
        n = rays.shape[0]
        row = np.zeros((n, 13), dtype=np.float32)
        row[:, :8] = rays[:, :8].numpy()
        row[:, 8] = (ts.numpy() % 64)
        row[:, 9] = labels[rng.randint(0, len(labels), n)]
        row[:, 10:12] = rays[:, 8:10].numpy()
        sd = os.path.join(root, "cache", "splits", "split_%d" % i)
        os.makedirs(sd, exist_ok=True)
        np.savez_compressed(os.path.join(sd, "rays1.npz"), row)
        np.savez_compressed(os.path.join(sd, "rgbs1.npz"), rgbs.numpy())
    exp = {"NEUCONW": {"N_SAMPLES": 8, "N_IMPORTANCE": 8, "UP_SAMPLE_STEP": 2, "N_OUTSIDE": 4, "NEAR_FAR_OVERRIDE": True,
                       "DEPTH_LOSS": True, "S_VAL_BASE": 3, "BOUNDARY_SAMPLES": 4, "SAMPLE_RANGE": 16, "SDF_THRESHOLD": 0.05,
                       "TRAIN_VOXEL_SIZE": 0.06, "UPDATE_FREQ": 3, "N_VOCAB": 64, "N_A": 16, "ANNEAL_END": 100,
                       "MESH_MASK_LIST": ["sky"], "RAY_MASK_LIST": ["person", "car"],
                       "SDF_CONFIG": {"d_out": 65, "d_hidden": 64, "skip_in": "(4,)"},
                       "COLOR_CONFIG": {"d_feature": 64, "d_hidden": 64, "head_channels": 32},
                       "S_CONFIG": {"init_val": 0.3}, "LOSS": {"igr_weight": 0.0001}},
           "DATASET": {"ROOT_DIR": root, "DATASET_NAME": "phototourism", "PHOTOTOURISM": {"CACHE_DIR": "cache"}},
           "TRAINER": {"CANONICAL_BS": 4096, "CANONICAL_LR": "1e-4", "LR_SCHEDULER": "none", "SAVE_DIR": os.path.join(root, "ckpts"),
                       "SAVE_FREQ": 4}}
    cfg = os.path.join(root, "train_synth.yaml")
    yaml.safe_dump(exp, open(cfg, "w"))
    return cfg


def test_train_driver_validation_meshes_and_fscore(tmp_path):
    root = str(tmp_path / "scene")
    cfg = _write_scene(root)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--cfg_path", cfg, "--batch_size", "64", "--num_epochs", "1",
           "--max_steps", "2", "--exp_name", "v", "--prec", "f32", "--log_every", "1", "--val_mesh_every", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    md = os.path.join(root, "ckpts", "v", "meshes")
    for s in (1, 2):
        for name in ("%08d.ply" % s, "%08d_detail.ply" % s):
            assert evalmesh.read_ply_points(os.path.join(md, name)).shape[0] > 100, name
    val = [l for l in r.stdout.splitlines() if l.startswith("[val] step")]
    assert len(val) == 2, r.stdout[-2000:]
    f = float(val[-1].split("fscore")[1].split()[0])
    assert math.isfinite(f) and 0.0 <= f <= 1.0
    assert os.path.isfile(os.path.join(md, "eval_eval", "metrics.json"))
