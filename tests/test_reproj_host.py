"""CPU: the host side of the reprojection filter (neuralrecon_w_amd.reproj) -- COLMAP readers, the tsv train split and the
composed cameras against the golden of the reference's own code (tests/golden/make_golden_reproj.py), the PLY mesh reader,
the refusal of non-PINHOLE cameras, the command lines' argument parsing, and the float64 test rasterizer's conventions."""
import os
import struct
import sys

import numpy as np
import pytest

from tests import _raster_oracle as O
from tests._util import GOLDEN, ROOT

from neuralrecon_w_amd import evalmesh, reproj

SCENE = os.path.join(GOLDEN, "reproj_scene")


def _golden():
    return np.load(os.path.join(GOLDEN, "reproj_golden.npz"))


def test_views_match_the_reference():
    g = _golden()
    S = reproj.read_sfm2gt(SCENE)
    assert np.array_equal(S, g["sfm2gt"])
    views = reproj.load_views(SCENE, S)
    assert [v["id"] for v in views] == g["train_ids"].tolist()
    assert [v["name"] for v in views] == g["names"].tolist()
    for i, v in enumerate(views):
        np.testing.assert_allclose(v["E"], g["E"][i], rtol=0, atol=1e-15)
        assert v["K"].dtype == np.float32 and np.array_equal(v["K"], g["K"][i])
        assert tuple(v["wh"]) == tuple(g["wh"][i])
        np.testing.assert_allclose(v["E_gt"], g["E_gt"][i], rtol=0, atol=1e-14)
        np.testing.assert_allclose(v["pose"], np.linalg.inv(g["E_gt"][i]), rtol=0, atol=1e-13)
    assert len({tuple(v["wh"]) for v in views}) == 2  # two cameras of different size


def test_colmap_readers_and_split():
    sp = os.path.join(SCENE, "dense", "sparse")
    cams = reproj.read_cameras_binary(os.path.join(sp, "cameras.bin"))
    assert sorted(cams) == [4, 9] and cams[4]["width"] == 40 and cams[4]["height"] == 30
    assert cams[9]["params"].tolist() == [30.5, 29.0, 15.1, 18.9]
    imgs = reproj.read_images_binary(os.path.join(sp, "images.bin"))
    assert sorted(imgs) == [1, 2, 3, 7] and imgs[3]["name"] == "a.jpg" and imgs[1]["camera_id"] == 9
    for im in imgs.values():
        R = reproj.qvec2rotmat(im["qvec"])
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
    # tsv order, train only, the id-less row skipped even though its image is not registered
    assert reproj.read_train_split(SCENE, imgs) == [2, 3, 1]


def test_split_refuses_an_unregistered_image(tmp_path):
    imgs = reproj.read_images_binary(os.path.join(SCENE, "dense", "sparse", "images.bin"))
    (tmp_path / "x.tsv").write_text("filename\tid\tsplit\na.jpg\t1\ttrain\nz.jpg\t2\ttest\n")
    with pytest.raises(KeyError, match="z.jpg"):
        reproj.read_train_split(str(tmp_path), imgs)
    (tmp_path / "x.tsv").write_text("filename\tid\tsplit\na.jpg\t1\ttrain\nz.jpg\tnan\ttest\nb.jpg\t4\ttest\n")
    assert reproj.read_train_split(str(tmp_path), imgs) == [3]


@pytest.mark.parametrize("model,nparams", [(0, 3), (2, 4), (4, 8), (42, 4)])
def test_non_pinhole_cameras_are_refused(tmp_path, model, nparams):
    p = tmp_path / "cameras.bin"
    p.write_bytes(struct.pack("<Q", 1) + struct.pack("<iiQQ", 1, model, 64, 48) + struct.pack("<%dd" % nparams, *range(nparams)))
    with pytest.raises(ValueError, match="only PINHOLE"):
        reproj.read_cameras_binary(str(p))


def _ply(path, fmt, v, f, rgb):
    hdr = ["ply", "format %s 1.0" % fmt, "comment test", "element vertex %d" % len(v), "property float x", "property float y",
           "property float z", "property float nx"]
    if rgb is not None:
        hdr += ["property uchar red", "property uchar green", "property uchar blue"]
    hdr += ["element face %d" % len(f), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(hdr) + "\n").encode())
        if fmt == "ascii":
            for i, p in enumerate(v):
                fh.write((" ".join(["%r" % float(x) for x in p] + ["0.5"] + ([str(int(c)) for c in rgb[i]] if rgb is not None else []))
                          + "\n").encode())
            for poly in f:
                fh.write((" ".join(str(x) for x in [len(poly)] + list(poly)) + "\n").encode())
        else:
            bo = "<" if fmt == "binary_little_endian" else ">"
            dt = [("p", bo + "f4", 3), ("n", bo + "f4")] + ([("c", "u1", 3)] if rgb is not None else [])
            rec = np.zeros(len(v), dtype=dt)
            rec["p"] = v
            if rgb is not None:
                rec["c"] = rgb
            fh.write(rec.tobytes())
            for poly in f:
                fh.write(struct.pack(bo + "B%di" % len(poly), len(poly), *poly))


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("colours", [True, False])
def test_read_ply_mesh(tmp_path, fmt, colours):
    rng = np.random.RandomState(3)
    v = rng.rand(7, 3).astype(np.float32)
    v[5] = v[2]  # a duplicate vertex stays (no welding)
    rgb = rng.randint(0, 256, (7, 3)).astype(np.uint8) if colours else None
    f = [(0, 1, 2), (2, 3, 4), (1, 4, 5, 6)]  # a quad is fanned
    p = str(tmp_path / "m.ply")
    _ply(p, fmt, v, f, rgb)
    vv, ff, cc = reproj.read_ply_mesh(p)
    assert vv.dtype == np.float64 and np.array_equal(vv, v.astype(np.float64))
    assert ff.tolist() == [[0, 1, 2], [2, 3, 4], [1, 4, 5], [1, 5, 6]]
    if colours:
        assert cc.dtype == np.uint8 and np.array_equal(cc, rgb)
    else:
        assert cc is None


def test_write_ply_points_round_trip(tmp_path):
    xyz = np.array([[1e-3, 2.5, -3.25], [100.0 + 1e-9, 0, 1]])
    rgb = np.array([[1, 2, 3], [250, 128, 0]], dtype=np.uint8)
    p = str(tmp_path / "r.ply")
    reproj.write_ply_points(p, xyz, rgb)
    v, f, c = reproj.read_ply_mesh(p)
    assert np.array_equal(v, xyz) and f.shape == (0, 3) and np.array_equal(c, rgb)
    assert b"property double x" in open(p, "rb").read(300)
    assert np.array_equal(evalmesh.read_ply_points(p, weld=False), xyz)


def test_backprojection_matrix_is_the_references_reproject():
    g = _golden()
    K, pose = g["K"][0], np.linalg.inv(g["E_gt"][0])
    d = np.zeros((5, 7))
    d[1, 2], d[4, 6], d[0, 0] = 1.25, 3.5, 0.75
    ref = O.backproject(d, K, pose)
    M = reproj.backproject_matrix(K, pose)
    r, c = np.nonzero(d > 0)
    got = (M[:, :3] @ np.stack([c * d[r, c], r * d[r, c], d[r, c]]) + M[:, 3:4]).T
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)


def test_oracle_conventions():
    """The test rasterizer itself: a front-facing triangle (negative signed pixel area) is drawn, its reverse is culled,
    pixel centres are sampled, the depth is the plane's camera z."""
    K = np.array([[10.0, 0, 5.0], [0, 10.0, 5.0], [0, 0, 1]])
    v = np.array([[-0.5, -0.5, 2.0], [-0.5, 0.5, 2.0], [0.5, -0.5, 2.0]])  # normal -z: towards the camera
    r = O.rasterize(v, [[0, 1, 2]], K, np.eye(4), 10, 10)
    assert (r["face"] == 0).sum() > 0 and np.allclose(r["depth"][r["face"] == 0], 2.0)
    assert (O.rasterize(v, [[0, 2, 1]], K, np.eye(4), 10, 10)["face"] >= 0).sum() == 0
    assert (O.rasterize(v, [[0, 2, 1]], K, np.eye(4), 10, 10, cull="none")["face"] == 0).sum() == (r["face"] == 0).sum()
    # the covered samples: pixel x = c + 0.5 in [2.5, 7.5] and the triangle's half below the diagonal
    rr, cc = np.nonzero(r["face"] == 0)
    assert cc.min() == 2 and rr.min() == 2 and ((cc + 0.5) + (rr + 0.5) <= 10 + 1e-9).all()


def test_command_lines_parse():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import eval_pipeline
        import reproj_filter
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    a = reproj_filter.parse_args(["--src_file", "m.ply", "--data_path", "d", "--output_path", "o", "--n_cpus", "8",
                                  "--n_gpus", "2", "--gt", "--visualize", "--voxel_size", "0.02"])
    assert (a.src_file, a.target_file, a.data_path, a.output_path, a.gt, a.visualize, a.voxel_size) == \
        ("m.ply", None, "d", "o", True, True, 0.02)
    assert (a.znear, a.zfar, a.cull, a.n_cpus, a.n_gpus) == (0.05, 100.0, "back", 8, 2)
    b = reproj_filter.parse_args(["--src_file", "m.ply", "--target_file", "t.ply", "--data_path", "d", "--output_path", "o"])
    assert (b.target_file, b.gt, b.visualize, b.voxel_size) == ("t.ply", False, False, 0.01)
    e = eval_pipeline.parse_args(["--scene_name", "lincoln_memorial", "--pred_dir", "p"])
    assert (e.scene_name, e.pred_dir, e.data_root) == ("lincoln_memorial", "p", "data/heritage-recon")
    with pytest.raises(SystemExit):
        eval_pipeline.parse_args(["--scene_name", "nowhere", "--pred_dir", "p"])
    assert reproj.SCENES["brandenburg_gate"] == {"thresholds": "0.01,1,0.01", "track_length": 14, "reproj_error": 2.0,
                                                 "voxel_size": 2.0}
