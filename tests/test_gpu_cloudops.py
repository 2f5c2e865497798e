"""GPU: the cloud operations on the k-NN grid (neuralrecon_w_amd.cloudops), the normal consistency of evalmesh.eval_mesh and
scripts/clean_cloud.py, against the numpy restatements of tests/_knn_ref.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import _knn_ref as K
from tests._util import ROOT
from tests.test_knn_host import outlier_fixture

from neuralrecon_w_amd import cloudops, evalmesh, ply

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _sphere_points(n, seed, radius=1.0, centre=(0.0, 0.0, 0.0)):
    v = np.random.RandomState(seed).randn(n, 3)
    return v / np.linalg.norm(v, axis=1, keepdims=True) * radius + np.asarray(centre, dtype=np.float64)


def _icosphere(levels):
    """(vertices [V,3] on the unit sphere, faces [F,3]) of an icosahedron subdivided `levels` times."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(levels):
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
    return np.stack(v), np.array(f, dtype=np.int64)


def _angle(n, radial):
    return np.arccos(np.clip(np.abs((n.astype(np.float64) * radial).sum(1)), 0.0, 1.0))


def test_estimate_normals_on_a_sphere():
    P = _sphere_points(4000, 1) * 2.0 + [5.0, -3.0, 1.0]
    radial = (P - [5.0, -3.0, 1.0]) / 2.0
    (p32,), centre = K.recentre32(P)
    _, idx, cnt = K.knn32(p32, p32, 16, exclude=np.arange(4000))
    rn, _, rc, rv = K.pca_ref(p32, p32, idx, cnt)
    bound = float(_angle(rn, radial).max())                            # what a k = 16 patch of this curvature allows
    assert rv.all() and bound < 0.2
    normal, curv, valid = cloudops.estimate_normals(torch.from_numpy(P).to(DEV), k=16)
    assert normal.dtype == torch.float32 and normal.shape == (4000, 3) and valid.dtype == torch.bool and bool(valid.all())
    got = float(_angle(normal.cpu().numpy(), radial).max())
    print("sphere normals: %.4g rad off the radial direction at the worst point (reference %.4g)" % (got, bound))
    assert got <= bound + 1e-6
    assert np.abs(curv.cpu().numpy() - rc).max() <= 1e-6 and float(curv.max()) < 0.05
    # facing a viewpoint: the centre sees every normal pointing inwards, a far point splits the sphere
    inward = cloudops.estimate_normals(torch.from_numpy(P).to(DEV), k=16, toward=[5.0, -3.0, 1.0])[0].double().cpu().numpy()
    assert ((inward * radial).sum(1) < 0).all()
    want = K.pca_ref(p32, p32, idx, cnt, toward=np.array([5.0, -3.0, 1.0]) - centre)[0]
    assert np.abs(inward - want).max() <= 1e-6
    n8, _, v8 = cloudops.estimate_normals(torch.from_numpy(P).to(DEV), k=16, max_dist=1e-3)     # nobody that close
    assert not bool(v8.any()) and bool((n8 == 0).all())


def test_remove_statistical_outliers_equals_the_restatement():
    P, _ = outlier_fixture()
    rk, rm = K.outliers_ref(P, k=16, ratio=2.0)
    keep, m = cloudops.remove_statistical_outliers(torch.from_numpy(P).to(DEV), k=16, ratio=2.0)
    assert keep.dtype == torch.bool and m.dtype == torch.float64
    assert np.array_equal(m.cpu().numpy(), rm)                        # 16 float32 distances sum exactly in float64
    assert np.array_equal(keep.cpu().numpy(), rk)
    assert not rk[2000:].any() and (~rk[:2000]).sum() <= 20
    with pytest.raises(ValueError):
        cloudops.remove_statistical_outliers(torch.from_numpy(P[:16]).to(DEV), k=16)


def test_normal_consistency_is_the_masked_mean():
    rng = np.random.RandomState(3)
    a, b = rng.randn(50, 3), rng.randn(40, 3)
    va, vb = rng.rand(50) > 0.2, rng.rand(40) > 0.2
    idx = rng.randint(-1, 40, 50)
    ok = va & (idx >= 0) & vb[np.clip(idx, 0, None)]
    want = np.abs((a * b[np.clip(idx, 0, None)]).sum(1))[ok].mean()
    t = lambda x: torch.from_numpy(x).to(DEV)
    got, cnt = cloudops.normal_consistency(t(a), t(va), t(b), t(vb), t(idx))
    assert cnt == int(ok.sum()) and abs(got - want) <= 1e-12
    got, cnt = cloudops.normal_consistency(t(a), t(va), t(b), t(vb), t(np.full(50, -1)))
    assert cnt == 0 and np.isnan(got)


# ---------------------------------------------------------------------------------------------------
# eval_mesh(normals=K)
# ---------------------------------------------------------------------------------------------------
SCENE = {"sfm2gt": np.eye(4).tolist(), "eval_bbx": [[-3.0, -3.0, -3.0], [3.0, 3.0, 3.0]]}
TS = [0.02, 0.05, 0.5]


def _ref_normals(P):
    (p32,), _ = K.recentre32(P)
    _, idx, cnt = K.knn32(p32, p32, 16, exclude=np.arange(P.shape[0]))
    n, _, _, v = K.pca_ref(p32, p32, idx, cnt)
    return n.astype(np.float64), v


def _nn64(A, B):
    """for every point of A its nearest point of B (float64 brute force): (distance, index)"""
    D = np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2).sum(-1))
    return D.min(1), D.argmin(1)


def _nc64(na, va, nb, vb, idx, mask):
    ok = va & vb[idx] & mask
    return float(np.abs((na * nb[idx]).sum(1))[ok].mean())


def test_eval_mesh_normal_consistency(tmp_path):
    verts, faces = _icosphere(4)                                       # 2562 vertices
    pred = str(tmp_path / "pred.ply")
    ply.write(pred, verts, faces=faces)
    gt_same, gt_off = str(tmp_path / "gt_same.ply"), str(tmp_path / "gt_off.ply")
    G1 = _sphere_points(3000, 2)
    G2 = _sphere_points(3000, 3, centre=(0.35, 0.0, 0.1))
    ply.write(gt_same, G1)
    ply.write(gt_off, G2)

    # normals=None: the files of today
    evalmesh.eval_mesh(pred, gt_same, SCENE, True, threshold=TS, save_name="plain", verbose=False)
    plain = open(str(tmp_path / "eval_plain" / "metrics.json"), "rb").read()
    old = json.loads(plain)
    assert sorted(old) == ["fscores", "precs", "recals", "thresholds"]
    assert plain == json.dumps({key: old[key] for key in ("thresholds", "fscores", "precs", "recals")}).encode()

    # its own samples
    m = evalmesh.eval_mesh(pred, gt_same, SCENE, True, threshold=TS, save_name="same", verbose=False, normals=16)
    s = json.load(open(str(tmp_path / "eval_same" / "metrics.json")))
    assert s["normals_k"] == 16 and s["normal_consistency"] > 0.99
    assert s["normal_consistency_pred2gt"] > 0.99 and s["normal_consistency_gt2pred"] > 0.99
    assert s["normal_consistency"] == (s["normal_consistency_pred2gt"] + s["normal_consistency_gt2pred"]) / 2
    assert m["normal_consistency"] == s["normal_consistency"] and m["fscore"] == old["fscores"][-1]
    assert {key: s[key] for key in old} == old                           # the old keys carry the old values
    for t in TS:                                                       # and the per-threshold files are byte for byte the same
        a = open(str(tmp_path / "eval_plain" / "visualize" / ("%.2f" % t) / "metrics.json"), "rb").read()
        assert a == open(str(tmp_path / "eval_same" / "visualize" / ("%.2f" % t) / "metrics.json"), "rb").read()
    assert len(s["normal_consistencies"]) == len(TS) and s["normal_consistencies"][-1] == s["normal_consistency"]

    # another sphere: the float64 numpy composition
    evalmesh.eval_mesh(pred, gt_off, SCENE, True, threshold=TS, save_name="off", verbose=False, normals=16)
    s = json.load(open(str(tmp_path / "eval_off" / "metrics.json")))
    P = ply.read_points(pred)
    n_p, v_p = _ref_normals(P)
    n_g, v_g = _ref_normals(G2)
    d_pg, i_pg = _nn64(P, G2)
    d_gp, i_gp = _nn64(G2, P)
    every_p, every_g = np.ones(P.shape[0], dtype=bool), np.ones(G2.shape[0], dtype=bool)
    p2g, g2p = _nc64(n_p, v_p, n_g, v_g, i_pg, every_p), _nc64(n_g, v_g, n_p, v_p, i_gp, every_g)
    print("offset sphere: pred2gt %.6f (numpy %.6f), gt2pred %.6f (numpy %.6f)" %
          (s["normal_consistency_pred2gt"], p2g, s["normal_consistency_gt2pred"], g2p))
    assert abs(s["normal_consistency_pred2gt"] - p2g) <= 1e-6 and abs(s["normal_consistency_gt2pred"] - g2p) <= 1e-6
    assert abs(s["normal_consistency"] - (p2g + g2p) / 2) <= 1e-6 and s["normal_consistency"] < 0.99
    for j, t in enumerate(TS):
        assert abs(s["normal_consistencies_pred2gt"][j] - _nc64(n_p, v_p, n_g, v_g, i_pg, d_pg < t)) <= 1e-6
        assert abs(s["normal_consistencies_gt2pred"][j] - _nc64(n_g, v_g, n_p, v_p, i_gp, d_gp < t)) <= 1e-6
    with pytest.raises(ValueError):
        evalmesh.eval_mesh(pred, gt_off, SCENE, True, threshold=TS, save_name="no", verbose=False, normals=16, exact_recall=True)
    assert not os.path.exists(str(tmp_path / "eval_no"))


# ---------------------------------------------------------------------------------------------------
# scripts/clean_cloud.py
# ---------------------------------------------------------------------------------------------------
def test_clean_cloud_end_to_end(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import clean_cloud
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    P, _ = outlier_fixture()
    rgb = np.random.RandomState(0).randint(0, 256, (P.shape[0], 3)).astype(np.uint8)
    src, dst = str(tmp_path / "cloud.ply"), str(tmp_path / "clean.ply")
    ply.write(src, P, rgb=rgb)
    view = np.array([1.0, 2.0, 2.0]) / 3.0 * 5.0                        # on the side the plane's normal points to
    n_in, n_out, bad = clean_cloud.main(["--file_in", src, "--file_out", dst, "--toward", "%r,%r,%r" % tuple(view.tolist())])
    keep, _ = K.outliers_ref(P, k=16, ratio=2.0)
    assert (n_in, n_out, bad) == (P.shape[0], int(keep.sum()), 0)
    verts, faces, cols = ply.read_mesh(dst)
    assert np.array_equal(verts, P[keep]) and faces.shape[0] == 0 and np.array_equal(cols, rgb[keep])
    normals = ply.read_normals(dst)
    assert normals.shape == (n_out, 3)
    want = cloudops.estimate_normals(torch.from_numpy(P[keep]).to(DEV), k=16, toward=view)[0].cpu().numpy()
    assert np.array_equal(normals, want)
    assert ((normals.astype(np.float64) @ (np.array([1.0, 2.0, 2.0]) / 3.0)) > 0.95).all()
    out = capsys.readouterr().out
    assert "points: %d -> %d" % (n_in, n_out) in out and "invalid normals: 0" in out
    # without colours, and without the outlier step
    ply.write(src, P)
    n_in, n_out, _ = clean_cloud.main(["--file_in", src, "--file_out", dst, "--outlier_k", "0", "--normals_k", "8"])
    assert n_in == n_out == P.shape[0] and ply.read_mesh(dst)[2] is None and ply.read_normals(dst).shape == (n_in, 3)
