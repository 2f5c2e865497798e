"""Host side of the scene preparation (neuralrecon_w_amd.sceneprep): the scene config against the reference's `generate_config`,
the tsv writer, the selection rules on the golden shares, the refusals, the static shares, and the three conditions the
fixture tests/golden/split_scene (tests/golden/make_golden_split.py) must meet for the GPU tests to be exact.  No GPU."""
import json
import os
import shutil

import numpy as np
import pytest

from tests import _roi_ref as RR
from tests._util import GOLDEN

SCENE = os.path.join(GOLDEN, "split_scene")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "split_golden.npz"))


def _flat(x):
    return np.asarray(x, dtype=np.float64).reshape(-1)


def test_scene_config_equals_generate_config(gold):
    """Key order as the reference writes it, every value to 1e-12 (np.percentile in float64 on the same points)."""
    from neuralrecon_w_amd import sceneprep

    ref = json.loads(str(gold["config_json"]))
    cfg = sceneprep.scene_config_from_sfm(os.path.join(SCENE, "dense", "sparse", "points3D.bin"), "split_scene")
    assert list(cfg) == list(ref) == list(sceneprep.CONFIG_KEYS) == [str(k) for k in gold["config_yaml_keys"]]
    assert cfg["name"] == ref["name"] and cfg["min_track_length"] == ref["min_track_length"] == 2
    for k in ("origin", "radius", "eval_bbx", "sfm2gt", "eval_bbx_detail", "voxel_size"):
        a, b = _flat(cfg[k]), _flat(ref[k])
        assert a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-12, k
    assert cfg["eval_bbx"] == cfg["eval_bbx_detail"]
    # points with 2 or fewer observations are in the file and do not count
    from neuralrecon_w_amd import colmap

    track = colmap.read_points3d(os.path.join(SCENE, "dense", "sparse", "points3D.bin"))[3]
    assert int((track > 2).sum()) == int(gold["config_n_points"]) < len(track)


def test_write_scene_config_round_trip_and_refusal(tmp_path, gold):
    import yaml

    from neuralrecon_w_amd import sceneprep

    root = tmp_path / "my_scene"
    shutil.copytree(os.path.join(SCENE, "dense", "sparse"), root / "dense" / "sparse")
    path = sceneprep.write_scene_config(str(root))
    text = open(path).read()
    assert [ln.split(":")[0] for ln in text.splitlines() if ln and ln[0] not in " -"] == list(sceneprep.CONFIG_KEYS)
    back = yaml.safe_load(text)
    ref = json.loads(str(gold["config_json"]))
    assert back["name"] == "my_scene" and back["origin"] == pytest.approx(ref["origin"], abs=1e-12)
    with pytest.raises(FileExistsError):
        sceneprep.write_scene_config(str(root))
    assert open(path).read() == text
    sceneprep.write_scene_config(str(root), name="other", overwrite=True)
    assert yaml.safe_load(open(path))["name"] == "other"


EXPECTED_TSV = ("filename\tid\tsplit\tdataset\n"
                "b.jpg\t0\ttest\tmy_scene\n"
                "sub/a 1.jpg\t1\ttest\tmy_scene\n"
                "c.png\t2\ttrain\tmy_scene\n"
                "d.jpg\t3\ttrain\tmy_scene\n")


def test_write_split_bytes_and_readers(tmp_path):
    import pandas

    from neuralrecon_w_amd import colmap, sceneprep

    root = tmp_path / "my_scene"
    root.mkdir()
    names = ["b.jpg", "sub/a 1.jpg", "c.png", "d.jpg"]
    path = sceneprep.write_split(str(root) + os.sep, names, 2)  # a trailing separator does not empty the dataset name
    assert os.path.basename(path) == "my_scene.tsv"
    assert open(path, "rb").read() == EXPECTED_TSV.encode()
    tsv, rows = colmap.split_rows(str(root))
    assert tsv == path and [r["filename"] for r in rows] == names and [r["id"] for r in rows] == ["0", "1", "2", "3"]
    assert [r["split"] for r in rows] == ["test", "test", "train", "train"] and {r["dataset"] for r in rows} == {"my_scene"}
    df = pandas.read_csv(path, sep="\t")
    assert list(df.columns) == ["filename", "id", "split", "dataset"] and list(df["filename"]) == names
    assert list(df["id"]) == [0, 1, 2, 3] and list(df["split"]) == ["test", "test", "train", "train"]
    # what pandas itself writes for the same table (prepare_data_split.py:61-62)
    ref = pandas.DataFrame(np.array([[n, str(i), "test" if i < 2 else "train", "my_scene"] for i, n in enumerate(names)]),
                           columns=["filename", "id", "split", "dataset"]).to_csv(sep="\t", index=False)
    assert ref == EXPECTED_TSV


def test_write_split_refusals(tmp_path):
    from neuralrecon_w_amd import sceneprep

    root = tmp_path / "s"
    root.mkdir()
    with pytest.raises(ValueError, match="remain"):
        sceneprep.write_split(str(root), ["a.jpg", "b.jpg"], 2)  # no training image would be left
    with pytest.raises(ValueError):
        sceneprep.write_split(str(root), ["a\tb.jpg", "c.jpg"], 1)
    assert os.listdir(root) == []
    (root / "old.tsv").write_text("filename\tid\tsplit\tdataset\n")
    with pytest.raises(FileExistsError, match="old.tsv"):
        sceneprep.write_split(str(root), ["a.jpg", "b.jpg"], 1)
    assert sorted(os.listdir(root)) == ["old.tsv"]
    path = sceneprep.write_split(str(root), ["a.jpg", "b.jpg"], 1, overwrite=True)
    assert os.path.basename(path) == "s.tsv" and open(path).read().count("\n") == 3
    with pytest.raises(FileExistsError):
        sceneprep.write_split(str(root), ["a.jpg", "b.jpg"], 1)


def test_select_views_on_the_golden_shares(gold):
    """The reference's returned names at (0.5, 0.6) and (0, 0): view_selection on the float64 shares, then the transient filter
    on its survivors (the filter judges every image by itself, so the composition is the intersection)."""
    from neuralrecon_w_amd import sceneprep

    names = [str(n) for n in gold["names"]]
    roi = gold["count64"] / np.diff(gold["prefix"])
    static = gold["static_share"]
    for rt, st in ((0.5, 0.6), (0.0, 0.0)):
        roi_ref = [str(n) for n in gold["roi_kept_%03d" % round(100 * rt)]]
        static_ref = [str(n) for n in gold["static_kept_%03d" % round(100 * st)]]
        kept, reasons = sceneprep.select_views(names, roi, None, rt, st)
        assert kept == roi_ref and set(reasons.values()) <= {"less_ROI"}
        kept, reasons = sceneprep.select_views(names, None, static, rt, st)
        assert kept == static_ref and set(reasons.values()) <= {"transient_much"}
        kept, reasons = sceneprep.select_views(names, roi, static, rt, st)
        assert kept == [n for n in roi_ref if n in static_ref]
        assert set(kept) | set(reasons) == set(names) and not set(kept) & set(reasons)
        for n, why in reasons.items():
            assert why == ("less_ROI" if n not in roi_ref else "transient_much")
    # the image EXACTLY at the static threshold is dropped (the rule is >), at both thresholds
    assert static[names.index("col.jpg")] == 0.6 and "col.jpg" not in gold["static_kept_060"]
    assert static[names.index("away.jpg")] == 0.0 and "away.jpg" not in gold["static_kept_000"]
    assert len(gold["roi_kept_000"]) == len(names)  # `share < 0` rejects nothing


def test_select_views_min_observation_rule(gold):
    """dataset_filter_utils.py:137-155 against the reference's own run with dense/sparse_filtered_3, and the focal exception
    with one synthetic camera row: fx AND fy above 2000 rescues an image the filtered model lacks; one of them does not."""
    from neuralrecon_w_amd import sceneprep

    names = [str(n) for n in gold["names"]]
    roi = gold["count64"] / np.diff(gold["prefix"])
    focal = np.stack([gold["K"][:, 0, 0], gold["K"][:, 1, 1]], 1)
    cov = [str(n) for n in gold["filtered_3"]]
    kept, reasons = sceneprep.select_views(names, roi, None, 0.5, 0.6, 3, cov, focal)
    assert sorted(kept) == sorted(str(n) for n in gold["roi_kept_050_minobs3"])
    assert reasons["col.jpg"] == "less_covis" and reasons["graze.jpg"] == "less_ROI"
    names2, roi2 = names + ["long.jpg", "wide.jpg"], np.concatenate([roi, [0.9, 0.9]])
    focal2 = np.concatenate([focal, [[2000.5, 2100.0], [2500.0, 2000.0]]])
    kept, reasons = sceneprep.select_views(names2, roi2, None, 0.5, 0.6, 3, cov, focal2)
    assert "long.jpg" in kept and reasons["wide.jpg"] == "less_covis"
    kept0, _ = sceneprep.select_views(names2, roi2, None, 0.5, 0.6, -1)
    assert "wide.jpg" in kept0 and "col.jpg" in kept0
    with pytest.raises(ValueError):
        sceneprep.select_views(names, roi, None, 0.5, 0.6, 3)
    with pytest.raises(ValueError):
        sceneprep.select_views(names, roi[:-1], None, 0.5, 0.6)


def test_static_shares_match_the_reference(gold):
    from neuralrecon_w_amd import sceneprep

    names = [str(n) for n in gold["names"]]
    got = sceneprep.static_shares(SCENE, "semantic_maps", names)
    assert got.dtype == np.float64 and np.array_equal(got, gold["static_share"])
    assert str(gold["static_missing_map"]) == "FileNotFoundError"  # what the reference does without a map file
    with pytest.raises(FileNotFoundError, match="nomap.jpg"):
        sceneprep.static_shares(SCENE, "semantic_maps", ["centre.jpg", "nomap.jpg"])


def test_static_shares_of_a_wide_dtype(tmp_path, gold):
    """A map that is not uint8 takes the other counting path and gives the same share."""
    from neuralrecon_w_amd import sceneprep

    (tmp_path / "maps").mkdir()
    lab = np.load(os.path.join(SCENE, "semantic_maps", "tele.npz"))["arr_0"]
    np.savez_compressed(tmp_path / "maps" / "tele.npz", lab.astype(np.int64))
    got = sceneprep.static_shares(str(tmp_path), "maps", ["tele.jpg"])
    assert got[0] == gold["static_share"][[str(n) for n in gold["names"]].index("tele.jpg")]


def test_scene_cameras_read_headers_only(tmp_path, gold):
    """One camera per registered image, file order; K unrescaled, pose as the dataset's, size from the file's header; a
    registered image without a file is named."""
    from neuralrecon_w_amd import sceneprep

    cams = sceneprep.scene_cameras(SCENE)
    assert [c.name for c in cams] == [str(n) for n in gold["names"]] and [c.image_id for c in cams] == gold["ids"].tolist()
    # against what the reference's view_selection itself handed to get_ray_directions / get_rays (recorded by the generator):
    # K is a float32 copy of the same four doubles, so it is exact; the pose is float32(inv(w2c)), where the reference inverts
    # all matrices in one batched call and views.image_pose one by one -- the float64 inverses may differ in their last bits,
    # which can move a float32 rounding by at most one ulp of the largest entry here (|x| < 8: 2^-21 = 4.8e-7)
    assert np.array_equal(np.stack([c.K for c in cams]), gold["ref_K"])
    err = float(np.abs(np.stack([c.c2w for c in cams]).astype(np.float64) - gold["ref_c2w"]).max())
    print("max |c2w - reference c2w| = %.3g" % err)
    assert float(np.abs(gold["ref_c2w"]).max()) < 8 and err <= 2.0 ** -21
    assert [[c.width, c.height] for c in cams] == gold["ref_wh"].tolist() == gold["wh"].tolist()
    assert np.array_equal(gold["K"], gold["ref_K"]) and float(np.abs(gold["c2w"].astype(np.float64) - gold["ref_c2w"]).max()) <= 2.0 ** -21
    assert np.array_equal(sceneprep.pixel_prefix(cams), gold["prefix"])
    root = tmp_path / "split_scene"
    shutil.copytree(SCENE, root)
    os.remove(root / "dense" / "images" / "graze.jpg")
    with pytest.raises(FileNotFoundError, match="graze.jpg"):
        sceneprep.scene_cameras(str(root))


def test_no_cpu_fallback(gold):
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import sceneprep

    cams = sceneprep.scene_cameras(SCENE)
    with pytest.raises(L.NeuconwHipError, match="no CPU fallback"):
        sceneprep.roi_shares(cams, gold["origin"], float(gold["radius"]), device="cpu")
    assert "ncw_views_roi" in L.exported_symbols() and L.ABI_VERSION >= 25


def test_fixture_conditions(gold):
    """What makes the GPU comparisons exact: (1) the ambiguous band holds at most 1 % of any view's pixels; (2) the reference's
    float32 mask equals the float64 predicate on every pixel outside the band; (3) no view's float64 count lies within its band
    count of threshold x pixels for the positive ROI threshold the tests use (`share < 0` holds for no count, so threshold 0
    cannot flip a view).  The restatement is recomputed here from the recorded cameras and must equal the recorded one."""
    prefix, wh = gold["prefix"], gold["wh"]
    npix = np.diff(prefix)
    assert np.array_equal(npix, wh[:, 0] * wh[:, 1]) and sum(int(p) % 64 != 0 for p in prefix[1:-1]) >= 6  # views meet inside waves
    band_count = np.zeros(len(npix), dtype=np.int64)
    for v in range(len(npix)):
        f = RR.roi_f64(gold["K"][v], gold["c2w"][v], int(wh[v, 0]), int(wh[v, 1]), gold["origin"], float(gold["radius"]))
        s = slice(int(prefix[v]), int(prefix[v + 1]))
        for k in ("dist_ray", "dist_cam", "dot"):
            assert np.allclose(f[k], gold[k][s], rtol=1e-12, atol=1e-12), (v, k)
        assert np.array_equal(f["roi"], gold["roi64"][s] != 0) and np.array_equal(f["band"], gold["band"][s] != 0)
        band_count[v] = int(f["band"].sum())
        assert int(f["roi"].sum()) == int(gold["count64"][v])
    assert np.array_equal(band_count, gold["band_count"])
    assert float((band_count / npix).max()) <= 0.01
    out = gold["band"] == 0
    assert np.array_equal(gold["ref_mask"][out], gold["roi64"][out])
    assert (np.abs(gold["count64"] - 0.5 * npix) > band_count).all()
    assert (np.abs(gold["ref_count"] - gold["count64"]) <= band_count).all()
    # the table of the fixture: shares of the nine views to four places
    assert np.round(gold["count64"] / npix, 4).tolist() == [0.6533, 0.0, 1.0, 0.4155, 1.0, 0.7031, 0.68, 0.4147, 0.0]


def test_command_lines_parse():
    import importlib.util

    def load(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(GOLDEN), "..", "scripts", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    a = load("prepare_data_split").build_parser().parse_args(["--root_dir", "x"])
    assert (a.num_test, a.min_observation, a.roi_threshold, a.static_threshold, a.semantic_map_path) == (10, -1, 0.5, 0.6, "semantic_maps")
    assert a.nima_ckpt_path == "weights/nima_epoch-34.pth" and a.seed == 0 and a.sfm_path == "sparse" and not a.overwrite and not a.visualize
    b = load("prepare_scene_config").build_parser().parse_args(["--root_dir", "x", "--name", "n", "--overwrite"])
    assert b.name == "n" and b.overwrite
    c = load("bench_split").build_parser().parse_args([])
    assert (c.views, c.width, c.height) == (1500, 1024, 768)
