"""GPU: the alignment check end to end (neuralrecon_w_amd.gtreproj, scripts/reproj_error.py) on tests/golden/gtreproj_scene,
against what the reference's own functions gave on CPU (tests/golden/gtreproj_golden.npz, tests/golden/make_golden_gtreproj.py).

Figures on one MI355X, as the tests print them (the kernels equal the float32 restatement of tests/_gtreproj_ref.py bit for bit, so
the restatement gives the same on a CPU): per-image means in reference mode 2.7e-8 of the largest mean off the reference's numbers,
bound 4 x 1.03e-8 = 4.1e-8 (the reference itself is 2.8e-8 off float64); mean error 0.76905821 px against the reference's
0.76906630: 1.05e-5 relative, bound 336 x 2^-24 = 2.0e-5 -- the reference's float32 projection of un-recentred coordinates of about
100 units is itself 1.04e-5 off float64, the recentred one 6e-8."""
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import _gtreproj_ref as GR
from tests._util import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SCENE = os.path.join(GOLDEN, "gtreproj_scene")
SCRIPT = os.path.join(ROOT, "scripts", "reproj_error.py")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gtreproj_golden.npz"))


def _run(gold, data_dir=SCENE, **kw):
    from neuralrecon_w_amd import gtreproj

    return gtreproj.gt_reprojection_error(data_dir, None, gold["sfm_to_gt"], "dense/sparse", int(gold["track_length"]), float(gold["reproj_error"]),
                                          float(gold["img_reproj_error"]), gt_points=gold["cloud"].astype(np.float64), **kw)


@pytest.fixture(scope="module")
def report(gold):
    """The tool on the fixture, once: shared by the tests below and left unchanged."""
    return _run(gold)


def test_image_errors(gold):
    """reference_unmatched: against the reference's per-image means.  Both the kernel and the float32 restatement of its contract
    are measured against float64 on the launch's own arrays, relative to the largest mean; the kernel gets 4 x the restatement's
    error (tests/_ray_cases.py), against float64 and against the reference's own float32 means alike.  Default mode: the same
    against the float64 restatement."""
    from neuralrecon_w_amd import gtreproj

    scene = gtreproj.read_scene(SCENE)
    results = {}
    for mode, ref in ((True, gold["ref_image_error"].astype(np.float64)), (False, None)):
        obs = gtreproj.image_observations(scene, reference_unmatched=mode)
        seg = obs[5]
        m64 = GR.seg_sums_f64(GR.reproj_errors_f64(*obs[:5]), seg) / np.diff(seg)
        m32 = GR.seg_sums_f64(GR.reproj_errors_f32(*obs[:5]), seg) / np.diff(seg)
        got = gtreproj.image_errors(scene, "cuda:0", reference_unmatched=mode)
        scale = np.abs(m64).max()
        e32, e_k = np.abs(m32 - m64).max() / scale, np.abs(got - m64).max() / scale
        print("image errors (reference_unmatched=%s): kernel %.3e, restatement %.3e" % (mode, e_k, e32))
        assert e32 > 0 and e_k <= 4 * e32
        assert np.array_equal(got, m32) or np.abs(got - m32).max() <= 1e-12 * scale  # the same float32 errors, summed in float64
        if ref is not None:
            e_ref = np.abs(ref - m64).max() / scale
            print("   against the reference's means: %.3e (the reference's own error %.3e)" % (np.abs(got - ref).max() / scale, e_ref))
            assert np.abs(got - ref).max() / scale <= 4 * e32
            assert np.array_equal(got < float(gold["img_reproj_error"]), gold["kept"])
        else:
            assert np.abs(m64 - gold["image_error_f64_default"]).max() <= 1e-12 * scale
            k = gold["kept"]  # on the well-registered images the unmatched key-points of the reference's rule are most of its error
            assert (got[k] < 0.5 * results[True][k]).all() and np.array_equal(got < float(gold["img_reproj_error"]), k)
        results[mode] = got


def test_chosen_points_and_mean(report, gold):
    rep = report
    n = len(rep["errors"])
    assert rep["n_images"] == 10 and rep["n_images_kept"] == 9 and rep["n_tracks_no_gt"] == 0
    assert rep["n_tracks"] == rep["n_tracks_selected"] == len(gold["ref_gt_index"])
    assert np.array_equal(rep["track_point_id"], gold["sel_point_id"]) and np.array_equal(rep["seg_start"], gold["sel_seg_start"])
    assert np.array_equal(rep["gt_index"], gold["ref_gt_index"])  # the chosen ground-truth point of EVERY selected track
    assert np.array_equal(rep["gt_points"], gold["cloud"][gold["ref_gt_index"]].astype(np.float64))
    assert n == len(gold["ref_errors"]) == rep["seg_start"][-1]
    ref = float(gold["ref_loss"])
    rel = abs(rep["mean_error"] - ref) / ref
    print("mean error %.8f px, reference %.8f: relative %.3e, bound %d x 2^-24 = %.3e" % (rep["mean_error"], ref, rel, n, n * 2.0 ** -24))
    assert rel <= n * 2.0 ** -24
    assert abs(rep["mean_error"] - np.sum(rep["errors"].astype(np.float64)) / n) <= 1e-12 * ref  # the mean of the errors reported
    # per element the reference's float32 projection of un-recentred coordinates ~ 100 is good to a few 1e-4 px
    assert np.abs(rep["errors"] - gold["ref_errors"]).max() < 1e-3
    # the points in SfM coordinates lie where the SfM points are, to the few pixels the tool measures
    assert np.abs(rep["gt_points_sfm"] - rep["sfm_points"]).max() < 0.1


def test_streamed_equals_unstreamed(report, gold):
    rep = _run(gold, chunk=1000)
    assert np.array_equal(rep["gt_index"], report["gt_index"]) and np.array_equal(rep["errors"].view(np.uint32), report["errors"].view(np.uint32))
    assert rep["mean_error"] == report["mean_error"]


def _move_keypoint(images_bin, image_id, point2d_idx, xy):
    """Overwrites one key-point of images.bin in place."""
    buf = bytearray(open(images_bin, "rb").read())
    (n,) = struct.unpack_from("<Q", buf, 0)
    off = 8
    for _ in range(n):
        (iid,) = struct.unpack_from("<i", buf, off)
        end = buf.index(b"\x00", off + 64)
        (n2d,) = struct.unpack_from("<Q", buf, end + 1)
        off = end + 9
        if iid == image_id:
            struct.pack_into("<dd", buf, off + 24 * point2d_idx, float(xy[0]), float(xy[1]))
        off += 24 * n2d
    open(images_bin, "wb").write(bytes(buf))


def test_track_without_gt_point_is_dropped_and_counted(tmp_path, report, gold):
    """The reference key-point of one track moved to a pixel that no ground-truth point projects onto (decided in float64, with
    a pixel of margin): the track is dropped and counted, every other track keeps its point, and the mean is the mean of the
    others' elements (the moved key-point is no element any more)."""
    t = 5
    seg = gold["sel_seg_start"]
    image_id, p2d = int(gold["sel_obs_image_id"][seg[t]]), int(gold["sel_obs_point2d_idx"][seg[t]])
    w, k = gold["query_w2c"][t], gold["query_intr"][t]
    c = gold["cloud"].astype(np.float64) @ w[:, :3].T + w[:, 3]
    u, v = (k[0] * c[:, 0] + k[2] * c[:, 2]) / c[:, 2], (k[1] * c[:, 1] + k[3] * c[:, 2]) / c[:, 2]
    free = [(x, y) for y in range(2, 40) for x in range(2, 58) if not ((np.abs(u - x) < 1.5) & (np.abs(v - y) < 1.5)).any()]
    assert free
    root = tmp_path / "gtreproj_scene"
    shutil.copytree(SCENE, root)
    _move_keypoint(str(root / "dense" / "sparse" / "images.bin"), image_id, p2d, free[0])
    rep = _run(gold, data_dir=str(root))
    assert rep["n_tracks_no_gt"] == 1 and rep["no_gt_point_id"].tolist() == [int(gold["sel_point_id"][t])]
    assert rep["n_tracks_selected"] == len(seg) - 1 and rep["n_tracks"] == len(seg) - 2
    others = np.arange(len(seg) - 1) != t
    assert np.array_equal(rep["track_point_id"], gold["sel_point_id"][others]) and np.array_equal(rep["gt_index"], report["gt_index"][others])
    keep = np.repeat(others, np.diff(seg))
    assert np.array_equal(rep["errors"].view(np.uint32), report["errors"][keep].view(np.uint32))
    assert np.array_equal(np.diff(rep["seg_start"]), np.diff(seg)[others])


def test_script_as_a_child_process(tmp_path, report, gold):
    from neuralrecon_w_amd import ply

    gt = str(tmp_path / "gt_cloud.ply")
    ply.write(gt, gold["cloud"].astype(np.float64))
    out = str(tmp_path / "out")
    cmd = [sys.executable, SCRIPT, "--data_dir", SCENE, "--gt_pcd_path", gt, "--track_length", "3", "--img_reproj_error", "20", "--batch_size", "2",
           "--out_dir", out, "--visualize", "--chunk", "2000"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert "avg re-projection error" in r.stdout and "selected 9 view" in r.stdout
    doc = json.load(open(os.path.join(out, "report.json")))
    assert doc["mean_error"] == report["mean_error"] and doc["n_tracks"] == report["n_tracks"] and doc["n_tracks_no_gt"] == 0
    assert doc["n_images_kept"] == 9 and doc["gt_index"] == report["gt_index"].tolist() and len(doc["errors"]) == doc["n_elements"] == len(report["errors"])
    assert np.array_equal(np.array(doc["errors"], dtype=np.float32), report["errors"])
    assert [n for n, e in doc["images"].items() if not e["kept"]] == ["bad.jpg"]
    sfm, gtp = ply.read_points(os.path.join(out, "colmap_sfm.ply")), ply.read_points(os.path.join(out, "gt.ply"))
    assert np.array_equal(sfm, report["sfm_points"]) and np.array_equal(gtp, report["gt_points_sfm"]) and len(sfm) == doc["n_tracks"]
    pngs = sorted(os.listdir(os.path.join(out, "reprojects")))
    assert len(pngs) == 9 and "bad.jpg.png" not in pngs and all(open(os.path.join(out, "reprojects", p), "rb").read(8) == b"\x89PNG\r\n\x1a\n" for p in pngs)
    assert not os.path.exists(str(tmp_path / "samples"))  # nothing lands in the working directory
