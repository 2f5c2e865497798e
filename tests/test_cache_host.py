"""CPU: the host half of the ray-cache writer (neuralrecon_w_amd.cachebuild) -- the COLMAP readers against the tables the
reference's own readers produced, the chunk writer bit for bit against the reference's `split_to_chunks`
(tests/golden/make_golden_cache.py), and the argument errors."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "golden", "cache_scene")
SPARSE = os.path.join(SCENE, "dense", "sparse")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "cache_golden.npz"))


def test_scene_lists_are_the_datasets(g):
    """The tsv's registered images in file order; c.jpg is 'test', e.jpg is not in images.bin."""
    from neuralrecon_w_amd import views

    scene = views.read_scene(SCENE, "sparse")
    assert scene["ids"] == g["ids"].tolist() and scene["ids_train"] == g["train_ids"].tolist()
    assert [scene["images"][i]["name"] for i in scene["ids"]] == g["names"].tolist()
    assert "e.jpg" not in scene["by_name"]


def test_readers_match_the_reference_tables(g):
    from neuralrecon_w_amd import cachebuild, colmap

    xyz_t, err_t = cachebuild.read_points3d_table(os.path.join(SPARSE, "points3D.bin"))
    assert xyz_t.dtype == np.float32 and np.array_equal(xyz_t, g["xyz_table"]) and np.array_equal(err_t, g["err_table"])
    pts = {i: (im["xys"], im["point3d_ids"]) for i, im in colmap.read_images(os.path.join(SPARSE, "images.bin"), True).items()}
    assert sorted(pts) == sorted(g["ids"].tolist())
    for iid in g["ids"].tolist():
        t = "im%d_" % iid
        xys, p3d = pts[iid]
        assert xys.dtype == np.float64 and np.array_equal(xys, g[t + "xys"]) and np.array_equal(p3d, g[t + "point3d_ids"])
        w, h = g[t + "wh"].tolist()
        xyz, err, px, err_mean = cachebuild.image_keypoints(xys, p3d, xyz_t, err_t, w, h, 1)
        assert np.array_equal(xyz, g[t + "kp_xyz"]) and np.array_equal(err, g[t + "kp_err"])
        assert px.dtype == np.int32 and np.array_equal(px, g[t + "kp_px"])  # torch.round of float64: halves go to even
        assert err_mean == float(g[t + "err_mean"])
        assert (p3d == -1).any() and len(px) == int((p3d != -1).sum())


def test_keypoint_rounding_and_downscale():
    from neuralrecon_w_amd import cachebuild

    xyz_t, err_t = np.arange(12, dtype=np.float32).reshape(4, 3), np.array([1, 2, 3, 4], dtype=np.float32)
    xys = np.array([[10.5, 7.5], [11.5, 8.5], [3.0, 5.0], [-0.6, 2.0], [21.0, 1.0], [5.0, 5.0]])
    ids = np.array([1, 2, 3, 0, 1, -1])
    xyz, err, px, err_mean = cachebuild.image_keypoints(xys, ids, xyz_t, err_t, 12, 9, 1)
    assert px.tolist() == [[10, 8], [12, 8], [3, 5], [-1, 2], [21, 1]]
    assert err.tolist() == [2, 3, 4, 1, 2] and err_mean == 3.0  # the mean runs over the in-image key-points only
    assert np.array_equal(xyz, xyz_t[[1, 2, 3, 0, 1]])
    _, _, px2, _ = cachebuild.image_keypoints(xys, ids, xyz_t, err_t, 6, 4, 2)
    assert px2.tolist() == [[5, 4], [6, 4], [2, 2], [0, 1], [10, 0]]  # 5.25 -> 5, 5.75 -> 6, 1.5 -> 2, 2.5 -> 2, -0.3 -> -0
    assert np.isnan(cachebuild.image_keypoints(xys[3:5], ids[3:5], xyz_t, err_t, 12, 9, 1)[3])


def test_chunk_writer_is_the_references_bit_for_bit(g, tmp_path):
    from neuralrecon_w_amd import cachebuild

    train = g["train_ids"].tolist()
    pad, n = g["chunk_padding"], int(g["n_chunks"])
    for arr, key in (("rgbs", "rgbs"), ("rays", "rows13")):
        lists = [torch.from_numpy(g["im%d_%s" % (i, key)]) for i in train]
        cachebuild.write_chunks(lists, str(tmp_path), n, 1, pad, arr)
        assert len(lists) == len(train)  # the caller's list is not extended by the padding
    assert sorted(os.listdir(tmp_path)) == ["rays1_meta_info.json", "rgbs1_meta_info.json"] + ["split_%d" % i for i in range(n)]
    for i in range(n):
        assert sorted(os.listdir(tmp_path / ("split_%d" % i))) == ["rays1.npz", "rgbs1.npz"]
        for arr in ("rays", "rgbs"):
            z = np.load(tmp_path / ("split_%d" % i) / ("%s1.npz" % arr))
            assert z.files == ["arr_0"]
            want = g["chunk%d_%s" % (i, arr)]
            assert z["arr_0"].dtype == want.dtype and z["arr_0"].shape == want.shape and z["arr_0"].tobytes() == want.tobytes()
    meta = json.load(open(tmp_path / "rays1_meta_info.json"))
    assert meta == json.loads(str(g["chunk_meta"])) == json.load(open(tmp_path / "rgbs1_meta_info.json"))


def test_chunk_padding_lengths():
    from neuralrecon_w_amd import cachebuild

    assert len(cachebuild.chunk_padding(3114, 3, 0)) == 0  # divisible: the reference pads nothing
    p = cachebuild.chunk_padding(3115, 4, 5)
    assert len(p) == 1 and 0 <= p[0] < 3115
    p = cachebuild.chunk_padding(1003, 7, 5)
    assert len(p) == 7 - 1003 % 7 and len(set(p.tolist())) == len(p)  # without replacement
    assert np.array_equal(p, cachebuild.chunk_padding(1003, 7, 5)) and not np.array_equal(p, cachebuild.chunk_padding(1003, 7, 6))


def test_unchunked_files(g, tmp_path):
    from neuralrecon_w_amd import cachebuild

    train = g["train_ids"].tolist()
    rays = [torch.from_numpy(g["im%d_rows12" % i]) for i in train]
    rgbs = [torch.from_numpy(g["im%d_rgbs" % i]) for i in train]
    files = cachebuild.write_cache(rays, rgbs, str(tmp_path), "cache", 2, -1)
    assert [os.path.relpath(f, tmp_path) for f in files] == ["cache/rays2.npz", "cache/rgbs2.npz"]
    assert np.array_equal(np.load(files[0])["arr_0"], np.concatenate([r.numpy() for r in rays]))
    assert np.array_equal(np.load(files[1])["arr_0"], np.concatenate([r.numpy() for r in rgbs]))


def test_argument_errors(tmp_path):
    from neuralrecon_w_amd import cachebuild

    with pytest.raises(NotImplementedError, match="npz"):
        cachebuild.build_cache(SCENE, cache_type="h5")
    with pytest.raises(FileNotFoundError, match="COLMAP"):  # no model under dense/<sfm_path>
        cachebuild.build_cache(str(tmp_path), sfm_path="sparse")
    with pytest.raises(FileNotFoundError, match="COLMAP"):
        cachebuild.build_cache(SCENE, sfm_path="../neuralsfm")
    with pytest.raises(ValueError, match="img_downscale"):
        cachebuild.build_cache(SCENE, img_downscale=0)
    # a label map whose size // downscale is not the image's
    assert cachebuild.load_label_map(SCENE, "semantic_maps", "a.jpg", 42, 27, 1).shape == (27, 42)
    with pytest.raises(ValueError, match="42 x 27.*but the image is 21 x 14"):
        cachebuild.load_label_map(SCENE, "semantic_maps", "a.jpg", 21, 14, 1)
    with pytest.raises(ValueError, match="21 x 13"):
        cachebuild.load_label_map(SCENE, "semantic_maps", "a.jpg", 21, 14, 2)
    with pytest.raises(L_error()):
        cachebuild.build_image(None, None, 0, None, None, device="cpu")


def L_error():
    from neuralrecon_w_amd import lib as L

    return L.NeuconwHipError


def test_cache_octree_struct_layout():
    """sizeof / field offsets of the ctypes mirror of NcwCacheOctree equal what the C compiler lays out."""
    from neuralrecon_w_amd import lib as L

    cc = "gcc"  # as tests/test_view_host.py does: a missing compiler fails the test, it does not hide the ABI mirror
    fields = ["origin", "scale", "level", "occ", "brick"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "neuconw_hip.h"\nint main(){printf("%zu", sizeof(NcwCacheOctree));'
            + "".join('printf(" %%zu", offsetof(NcwCacheOctree, %s));' % f for f in fields) + "return 0;}")
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.run([cc, "-I", os.path.join(os.path.dirname(HERE), "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(L.NcwCacheOctree)] + [getattr(L.NcwCacheOctree, f).offset for f in fields]


def test_command_line_hands_its_flags_to_build_cache(monkeypatch):
    """scripts/prepare_data_cache.py: the reference's flags plus --sfm_path / --seed / --device reach build_cache under the
    right names (the script passes most of them by position)."""
    import importlib.util
    import inspect

    from neuralrecon_w_amd import cachebuild

    spec = importlib.util.spec_from_file_location("prepare_data_cache_cli", os.path.join(os.path.dirname(HERE), "scripts", "prepare_data_cache.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    sig = inspect.signature(cachebuild.build_cache)
    seen = {}

    def fake(*a, **k):
        seen.update(sig.bind(*a, **k).arguments)
        k["stats"].update(n_images=1, n_rays=2, n_pixels=3, d2h_bytes=4, t_decode=0.0, t_device=0.0, t_write=0.0)
        return ["f"]

    monkeypatch.setattr(cachebuild, "build_cache", fake)
    cli.main(["--root_dir", "/scene", "--dataset_name", "phototourism", "--cache_dir", "cc", "--cache_type", "npz", "--img_downscale", "2",
              "--split_to_chunks", "5", "--semantic_map_path", "sem", "--sfm_path", "sparse", "--seed", "9", "--device", "cuda:1"])
    seen.pop("stats")
    assert seen == {"root_dir": "/scene", "cache_dir": "cc", "img_downscale": 2, "semantic_map_path": "sem", "split_to_chunks": 5,
                    "sfm_path": "sparse", "seed": 9, "device": "cuda:1", "cache_type": "npz", "depth_percent": None}
    d = vars(cli.build_parser().parse_args(["--root_dir", "x"]))
    assert (d["cache_dir"], d["img_downscale"], d["split_to_chunks"], d["semantic_map_path"], d["sfm_path"], d["seed"]) == ("cache", 1, -1, None, None, 0)
    with pytest.raises(NotImplementedError, match="npz"):  # the reference's default type is refused by build_cache itself
        monkeypatch.undo()
        cli.main(["--root_dir", SCENE, "--cache_type", "h5"])
