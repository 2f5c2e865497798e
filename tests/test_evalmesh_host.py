"""CPU: the host side of the mesh evaluation (neuralrecon_w_amd.evalmesh) -- PLY reading, the COLMAP filter, the box and SfM
crops, the metrics and the --threshold parsing -- against float64 numpy restatements written here from the reference's
documented behaviour (utils/eval_utils.py:87-216, utils/eval_mesh.py:126-129).  No GPU, no HIP library."""
import math
import os
import struct

import numpy as np
import pytest
import torch

from tests._util import ROOT

from neuralrecon_w_amd import evalmesh, mesh


# ---------------------------------------------------------------- PLY
def _ascii_ply(path, verts, faces):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment made by a test\nelement vertex %d\n" % len(verts))
        f.write("property double x\nproperty double y\nproperty double z\nproperty float nx\nproperty uchar red\n")
        f.write("element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(faces))
        for v in verts:
            f.write("%r %r %r 0.5 7\n" % tuple(float(c) for c in v))
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(t))


def _binary_ply(path, verts, faces, face_first=False):
    vrec = np.zeros(len(verts), dtype=[("nx", "<f4"), ("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("c", "u1"), ("q", "<i4")])
    vrec["x"], vrec["y"], vrec["z"] = verts[:, 0], verts[:, 1], verts[:, 2]
    vrec["nx"], vrec["c"], vrec["q"] = 1.0, 3, -5
    vhdr = ("element vertex %d\nproperty float nx\nproperty double x\nproperty double y\nproperty double z\n"
            "property uchar red\nproperty int quality\n" % len(verts))
    fhdr = "element face %d\nproperty list uchar int vertex_indices\nproperty uchar flags\n" % len(faces)
    fbody = b"".join(struct.pack("<B3iB", 3, *t, 1) for t in faces)
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\n" + (fhdr + vhdr if face_first else vhdr + fhdr) + "end_header\n").encode())
        if face_first:
            f.write(fbody + vrec.tobytes())
        else:
            f.write(vrec.tobytes() + fbody)


def test_ply_reader_ascii_and_binary(tmp_path):
    rng = np.random.RandomState(0)
    v = rng.randn(50, 3) * 1e3 + 0.123456789012345
    f = rng.randint(0, 50, (20, 3))
    for name, writer in (("a.ply", _ascii_ply), ("b.ply", _binary_ply)):
        p = str(tmp_path / name)
        writer(p, v, f)
        got = evalmesh.read_ply_points(p)
        assert got.dtype == np.float64 and got.shape == (50, 3)
        np.testing.assert_array_equal(got, v)  # doubles round-trip exactly
    p = str(tmp_path / "c.ply")
    _binary_ply(p, v, f, face_first=True)  # the face element before the vertices: walked, not misread
    np.testing.assert_array_equal(evalmesh.read_ply_points(p), v)


def test_ply_reader_welds_exact_duplicates_of_meshes_only(tmp_path):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [1, 0, 0], [1e-12, 0, 0]], dtype=np.float64)
    p = str(tmp_path / "m.ply")
    _binary_ply(p, v, np.array([[0, 1, 3]]))
    np.testing.assert_array_equal(evalmesh.read_ply_points(p), v[[0, 1, 3, 5]])  # first occurrences, order kept
    p2 = str(tmp_path / "pc.ply")
    _binary_ply(p2, v, np.zeros((0, 3), dtype=np.int64))  # a point cloud: stored vertices as they are
    np.testing.assert_array_equal(evalmesh.read_ply_points(p2), v)


def test_ply_reader_reads_write_ply_output(tmp_path):
    rng = np.random.RandomState(1)
    v = torch.from_numpy(rng.randn(40, 3).astype(np.float32))
    faces = torch.from_numpy(np.stack([np.arange(0, 36, 3), np.arange(1, 37, 3), np.arange(2, 38, 3)], -1))
    for colors in (None, torch.randint(0, 255, (40, 3), dtype=torch.uint8)):
        p = str(tmp_path / "w.ply")
        mesh.write_ply(p, v, faces, colors)
        np.testing.assert_array_equal(evalmesh.read_ply_points(p), v.numpy().astype(np.float64))
    mesh.write_ply(p, v, torch.zeros(0, 3, dtype=torch.int64))  # the vertex-only files eval_mesh writes
    np.testing.assert_array_equal(evalmesh.read_ply_points(p), v.numpy().astype(np.float64))


# ---------------------------------------------------------------- COLMAP filter
def _parse_points3d(path):
    """Independent parse: whole records with struct, no offsets shared with the package."""
    out = []
    with open(path, "rb") as f:
        n = struct.unpack("<Q", f.read(8))[0]
        for _ in range(n):
            pid, x, y, z, r, g, b, err = struct.unpack("<QdddBBBd", f.read(43))
            tl = struct.unpack("<Q", f.read(8))[0]
            f.read(8 * tl)
            out.append((x, y, z, err, tl))
    return np.array(out, dtype=np.float64).reshape(-1, 5)


def test_read_points3d_filtered_matches_an_independent_parse():
    path = os.path.join(ROOT, "tests", "golden", "sfm_scene", "dense", "sparse", "points3D.bin")
    rec = _parse_points3d(path)
    assert rec.shape[0] > 10
    T = np.array([[0.0, -2.0, 0.0, 5.0], [2.0, 0.0, 0.0, -1.0], [0.0, 0.0, 2.0, 0.25], [0, 0, 0, 1]])
    tls = np.unique(rec[:, 4])
    errs = np.unique(rec[:, 3])
    cases = [(tls[0], errs[-1] + 1), (tls[len(tls) // 2], errs[len(errs) // 2]), (-1, errs[0]), (tls[-1], 1e9)]
    for tl, er in cases:  # thresholds ON data values: the strict inequalities decide
        keep = (rec[:, 4] > tl) & (rec[:, 3] < er)
        exp = rec[keep, :3] @ T[:3, :3].T + T[:3, 3]
        got = evalmesh.read_points3d_filtered(path, tl, er, T)
        assert got.shape == exp.shape
        np.testing.assert_allclose(got, exp, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(evalmesh.read_points3d_filtered(os.path.dirname(path), tl, er), rec[keep, :3])
    assert evalmesh.read_points3d_filtered(path, tls[-1], 1e9).shape == (0, 3)


# ---------------------------------------------------------------- crops
def _bbx_ref(points, bbx):
    lo, hi = np.asarray(bbx[0], np.float64), np.asarray(bbx[1], np.float64)
    c, s = (lo + hi) / 2, (hi - lo) / 2
    keep = [all(-1 < (p[a] - c[a]) / s[a] < 1 for a in range(3)) for p in points]
    return points[np.array(keep, dtype=bool)] if len(points) else points


def test_bbx_crop_is_the_open_box():
    bbx = [[-1.0, -2.0, 0.0], [3.0, 2.0, 0.5]]
    rng = np.random.RandomState(2)
    pts = np.concatenate([rng.uniform(-3, 4, (500, 3)),
                          np.array([[-1.0, 0, 0.25], [3.0, 0, 0.25], [0, -2.0, 0.25], [0, 2.0, 0.25], [0, 0, 0.0], [0, 0, 0.5],
                                    [1.0, 0.0, 0.25]])])  # on the faces: out; the centre: in
    got = evalmesh.bbx_crop(pts, bbx)
    np.testing.assert_array_equal(got, _bbx_ref(pts, bbx))
    assert not (got == np.array([3.0, 0, 0.25])).all(-1).any() and (got == np.array([1.0, 0.0, 0.25])).all(-1).any()
    assert evalmesh.bbx_crop(np.zeros((0, 3)), bbx).shape == (0, 3)


def _sfm_crop_ref(points, sfm, voxel, bbx):
    lo, hi = np.asarray(bbx[0], np.float64), np.asarray(bbx[1], np.float64)
    half = np.max(hi - lo) / 2
    c = lo + (hi - lo) / 2
    res = int(math.floor(2 * half / voxel))

    def cell(p):
        return tuple(int(math.floor(res * ((p[a] - c[a]) / half + 1.0) / 2.0)) for a in range(3))

    occupied = {cell(s) for s in sfm if all(0 <= k < res for k in cell(s))}
    keep = [cell(p) in occupied for p in points]
    return points[np.array(keep, dtype=bool)] if len(points) else points


def test_sfm_crop_matches_the_voxel_rule():
    bbx = [[0.0, 0.0, 0.0], [4.0, 2.0, 1.0]]
    rng = np.random.RandomState(3)
    sfm = np.concatenate([rng.uniform(0, 4, (40, 3)) * [1, 0.5, 0.25],
                          np.array([[9.0, 9.0, 9.0], [-3.0, 1.0, 0.5], [4.0, 1.0, 0.5]])])  # outside the cube / on its face
    pts = np.concatenate([rng.uniform(-1, 5, (4000, 3)), sfm + 1e-9, np.array([[9.0, 9.0, 9.0], [4.0, 1.0, 0.5]])])
    got = evalmesh.sfm_crop(pts, sfm, 0.3, bbx)
    exp = _sfm_crop_ref(pts, sfm, 0.3, bbx)
    assert got.shape[0] > 40
    np.testing.assert_array_equal(got, exp)
    assert not (got == 9.0).all(-1).any()  # the SfM point outside the cube keeps nothing
    assert evalmesh.sfm_crop(np.zeros((0, 3)), sfm, 0.3, bbx).shape == (0, 3)
    assert evalmesh.sfm_crop(pts, np.zeros((0, 3)), 0.3, bbx).shape == (0, 3)


# ---------------------------------------------------------------- metrics
def _metrics_ref(d_gt_to_pred, d_pred_to_gt, t):
    a = np.asarray(d_gt_to_pred, np.float64)
    b = np.asarray(d_pred_to_gt, np.float64)
    nan = float("nan")
    prec = sum(1 for x in b if x < t) / len(b) if len(b) else nan
    rec = sum(1 for x in a if x < t) / len(a) if len(a) else nan
    prec = prec if prec != prec else max(prec, 1e-6)
    rec = rec if rec != rec else max(rec, 1e-6)
    return {"dist1": float(np.mean(b)) if len(b) else nan, "dist2": float(np.mean(a)) if len(a) else nan,
            "prec": prec, "recal": rec, "fscore": 2 * prec * rec / (prec + rec)}


def test_metrics_against_a_restatement():
    rng = np.random.RandomState(4)
    a = rng.exponential(0.1, 3001).astype(np.float32)
    b = rng.exponential(0.2, 1999).astype(np.float32)
    b[:5] = 0.1  # exactly on a threshold: not below it
    ts = [float(t) for t in np.arange(0.01, 1, 0.01)] + [0.1, 1e-9, 50.0]
    got = evalmesh.metrics(torch.from_numpy(a), torch.from_numpy(b), ts)
    for t, g in zip(ts, got):
        e = _metrics_ref(a, b, t)
        assert set(g) == {"dist1", "dist2", "prec", "recal", "fscore"}
        for k in ("prec", "recal", "fscore"):
            assert g[k] == e[k], (t, k, g[k], e[k])
        for k in ("dist1", "dist2"):
            assert abs(g[k] - e[k]) <= 1e-12 * abs(e[k])
    assert got[-2]["prec"] == 1e-6 and got[-2]["recal"] == 1e-6  # the floors
    one = evalmesh.metrics(torch.from_numpy(a), torch.from_numpy(b), 0.1)
    assert len(one) == 1 and one[0]["prec"] == _metrics_ref(a, b, 0.1)["prec"]


def test_metrics_of_empty_clouds_are_nan():
    e = torch.zeros(0)
    x = torch.rand(10)
    for da, db in ((e, e), (e, x), (x, e)):
        m = evalmesh.metrics(da, db, [0.1, 0.2])
        assert all(math.isnan(v["fscore"]) for v in m)
    m = evalmesh.metrics(e, x, [0.5])[0]
    assert math.isnan(m["recal"]) and math.isnan(m["dist2"]) and not math.isnan(m["prec"])


# ---------------------------------------------------------------- command line
def test_threshold_parsing():
    assert evalmesh.parse_thresholds("0.1") == [0.1]
    got = evalmesh.parse_thresholds("0.01,1,0.01")
    assert got == [float(v) for v in np.arange(0.01, 1, 0.01)] and len(got) == 99
    assert evalmesh.parse_thresholds(" 0.5, 0.8 ,0.1") == [float(v) for v in np.arange(0.5, 0.8, 0.1)]
    with pytest.raises(ValueError):
        evalmesh.parse_thresholds("0.1,0.2")


def test_nn_distances_refuses_cpu_tensors():
    with pytest.raises(evalmesh.L.NeuconwHipError, match="no CPU fallback"):
        evalmesh.nn_distances(torch.zeros(4, 3), torch.zeros(2, 3))
