"""Host side of the alignment check (neuralrecon_w_amd.gtreproj), no GPU: the track reader, the selection against what the
reference's own run selected (tests/golden/gtreproj_golden.npz, recorded by tests/golden/make_golden_gtreproj.py), the fixture's
conditions, the float32 restatement against the reference's chosen points, the command line and the binding."""
import importlib.util
import os
import struct

import numpy as np
import pytest

from tests import _gtreproj_ref as GR
from tests._util import GOLDEN, ROOT

SCENE = os.path.join(GOLDEN, "gtreproj_scene")
SPARSE = os.path.join(SCENE, "dense", "sparse")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gtreproj_golden.npz"))


@pytest.fixture(scope="module")
def scene():
    from neuralrecon_w_amd import gtreproj

    return gtreproj.read_scene(SCENE)


@pytest.fixture(scope="module")
def selection(scene, gold):
    from neuralrecon_w_amd import gtreproj

    kept_ids = [iid for iid, k in zip(scene["image_ids"], gold["kept"]) if k]
    return gtreproj.select_tracks(scene, kept_ids, int(gold["track_length"]), float(gold["reproj_error"]))


def _walk_points3d(path):
    """points3D.bin parsed here, independently of the reader: [(id, xyz, error, [(image id, point2D idx)])]."""
    buf = open(path, "rb").read()
    (n,) = struct.unpack_from("<Q", buf, 0)
    off, out = 8, []
    for _ in range(n):
        pid, x, y, z, _, _, _, err = struct.unpack_from("<QdddBBBd", buf, off)
        (m,) = struct.unpack_from("<Q", buf, off + 43)
        el = [struct.unpack_from("<ii", buf, off + 51 + 8 * k) for k in range(m)]
        out.append((pid, (x, y, z), err, el))
        off += 51 + 8 * m
    assert off == len(buf)
    return out


def test_read_points3d_with_tracks():
    from neuralrecon_w_amd import colmap

    path = os.path.join(SPARSE, "points3D.bin")
    plain = colmap.read_points3d(path)
    assert len(plain) == 4  # the default return value is unchanged
    full = colmap.read_points3d(path, with_tracks=True)
    assert len(full) == 7
    for a, b in zip(plain, full[:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    ids, xyz, err, track, start, t_img, t_p2d = full
    assert start.dtype == np.int64 and t_img.dtype == np.int32 and t_p2d.dtype == np.int32
    truth = _walk_points3d(path)
    assert len(truth) == len(ids) and 1 == min(len(t[3]) for t in truth) and max(len(t[3]) for t in truth) == 8
    assert np.array_equal(start, np.concatenate([[0], np.cumsum([len(t[3]) for t in truth])])) and np.array_equal(np.diff(start), track)
    for i, (pid, p, e, el) in enumerate(truth):
        assert ids[i] == pid and tuple(xyz[i]) == p and err[i] == e
        assert [(int(a), int(b)) for a, b in zip(t_img[start[i]:start[i + 1]], t_p2d[start[i]:start[i + 1]])] == el
    # the other fixture scenes still read, tracks included
    for other in ("sfm_scene", "split_scene"):
        p = os.path.join(GOLDEN, other, "dense", "sparse", "points3D.bin")
        if os.path.isfile(p):
            o = colmap.read_points3d(p, with_tracks=True)
            assert o[4][-1] == len(o[5]) == len(o[6]) == o[3].sum()


def test_scene_matches_the_reference_cameras(scene, gold):
    assert scene["image_ids"] == [int(i) for i in gold["image_ids"]] and scene["names"] == [str(n) for n in gold["image_names"]]
    assert np.array_equal(scene["E"], gold["ref_E"])  # get_entrinsics, float64, bit for bit
    assert scene["K"].dtype == np.float32 and np.array_equal(scene["K"], gold["ref_K"])  # get_intrinsic
    assert any((im["point3d_ids"] < 0).any() for im in scene["images"].values())  # key-points without a 3-D point exist
    assert scene["wh"].max(0).tolist() == [131, 71]


def test_select_tracks_equals_the_reference_selection(scene, selection, gold):
    seg = selection["seg_start"]
    n = len(selection["point_row"])
    assert 24 <= n <= 80
    # the golden selection: order, lengths, every element
    assert np.array_equal(selection["point_id"], gold["sel_point_id"]) and np.array_equal(seg, gold["sel_seg_start"])
    assert np.array_equal(selection["obs_image_id"], gold["sel_obs_image_id"]) and np.array_equal(selection["obs_point2d_idx"], gold["sel_obs_point2d_idx"])
    assert np.array_equal(selection["obs_xy"], gold["sel_obs_xy"])
    # what the reference handed to get_gt_point for every track, in its order: the reference observation
    ref = gold["ref_pts2d"]
    assert len(ref) == n
    assert np.array_equal(ref[:, 0], selection["obs_image_id"][seg[:-1]]) and np.array_equal(ref[:, 1], selection["obs_point2d_idx"][seg[:-1]])
    assert np.array_equal(ref[:, 2:], selection["obs_xy"][seg[:-1]].astype(np.float32))
    assert len(gold["ref_errors"]) == seg[-1]  # the reference measured as many elements
    # file order; more than track_length observations in the file; the dropped image contributes nothing
    assert (np.diff(selection["point_row"]) > 0).all()
    assert (scene["track_len"][selection["point_row"]] > int(gold["track_length"])).all()
    assert (scene["error"][selection["point_row"]] < float(gold["reproj_error"])).all()
    bad = [iid for iid, k in zip(scene["image_ids"], gold["kept"]) if not k]
    assert len(bad) == 1 and not np.isin(selection["obs_image_id"], bad).any()
    assert (np.diff(seg) < scene["track_len"][selection["point_row"]]).any()  # some track lost elements to the dropped image
    assert (np.diff(seg) >= 1).all()


def test_select_tracks_rules(scene):
    from neuralrecon_w_amd import gtreproj

    all_ids = scene["image_ids"]
    none = gtreproj.select_tracks(scene, [], 0, 1e9)
    assert len(none["point_row"]) == 0 and none["seg_start"].tolist() == [0] and none["obs_xy"].shape == (0, 2)
    every = gtreproj.select_tracks(scene, all_ids, 0, 1e9)
    assert np.array_equal(every["point_row"], np.arange(len(scene["point_ids"])))  # length > 0: every point
    assert np.array_equal(np.diff(every["seg_start"]), scene["track_len"])
    strict = gtreproj.select_tracks(scene, all_ids, 8, 1e9)
    assert len(strict["point_row"]) == 0  # "more than": the longest track has 8
    one = gtreproj.select_tracks(scene, all_ids[:1], 0, 1e9)
    assert set(one["obs_image_id"].tolist()) == {all_ids[0]} and (np.diff(one["seg_start"]) == 1).all()


def _queries(scene, selection, gold):
    from neuralrecon_w_amd import gtreproj

    index_of = {iid: k for k, iid in enumerate(scene["image_ids"])}
    ref = selection["seg_start"][:-1]
    cam = np.array([index_of[int(g)] for g in selection["obs_image_id"][ref]])
    w2c = (scene["E"] @ np.linalg.inv(gold["sfm_to_gt"]))[cam, :3, :]
    intr = np.stack([scene["K"][cam, 0, 0], scene["K"][cam, 1, 1], scene["K"][cam, 0, 2], scene["K"][cam, 1, 2]], -1)
    return gtreproj, w2c, intr, selection["obs_xy"][ref]


def test_fixture_conditions(scene, selection, gold):
    """What make_golden_gtreproj.py asserted when it wrote the fixture, checked again on the files."""
    gtreproj, w2c, intr, xy = _queries(scene, selection, gold)
    assert np.array_equal(w2c, gold["query_w2c"]) and np.array_equal(intr, gold["query_intr"])
    cloud = gold["cloud"].astype(np.float64)
    assert gold["cloud"].dtype == np.float32 and len(cloud) <= 8192
    M = gold["sfm_to_gt"]
    assert np.abs(M[:3, 3]).max() >= 100 and abs(np.cbrt(np.linalg.det(M[:3, :3])) - 1.7) < 1e-12 and abs(M[0, 1]) > 0.1  # large translation, scale, rotation
    idx, band, gap, _ = GR.pixel_nearest_f64(w2c, intr, xy, cloud)
    assert (idx >= 0).all()        # every selected track's reference pixel is hit
    assert not band.any()          # nothing within 1e-3 px of a rounding boundary, no |c_2| < 1e-6
    assert gap.min() > 1e-4        # the nearest hit is nearest by more than float32 can blur
    assert np.array_equal(idx, gold["index_f64"])
    # the reference's own float32 choice equals the float64 choice on EVERY query: none is left out
    assert np.array_equal(gold["ref_gt_index"], idx)
    # key-points at k + 0.5 are among the queries (round: ties to even)
    assert (np.modf(xy)[0] == 0.5).any()
    # points behind the camera that project onto a query pixel are in the cloud
    c = np.einsum("qij,nj->qni", w2c[:, :, :3], cloud) + w2c[:, None, :, 3]
    u = (intr[:, None, 0] * c[..., 0] + intr[:, None, 2] * c[..., 2]) / c[..., 2]
    v = (intr[:, None, 1] * c[..., 1] + intr[:, None, 3] * c[..., 2]) / c[..., 2]
    X = np.rint(xy.astype(np.float32)).astype(np.float64)
    on = (np.abs(u - X[:, None, 0]) < 0.5) & (np.abs(v - X[:, None, 1]) < 0.5)
    assert (on & (c[..., 2] < 0)).any(1).all()
    assert ((on & (c[..., 2] > 0)).sum(1) >= 2).all()  # and a farther point on the same pixel
    # the marked band points really sit at a boundary of their query's pixel: they are stored as float32 at |coordinate| ~ 100
    # (quantum 2^-17 = 7.6e-6 units, times focal / depth ~ 100 / 5 px per unit: up to 1.5e-4 px off where they were aimed)
    bp, bq = gold["band_points"].astype(np.float64), gold["band_query"]
    cb = np.einsum("nij,nj->ni", w2c[bq][:, :, :3], bp) + w2c[bq][:, :, 3]
    ub = (intr[bq, 0] * cb[:, 0] + intr[bq, 2] * cb[:, 2]) / cb[:, 2]
    vb = (intr[bq, 1] * cb[:, 1] + intr[bq, 3] * cb[:, 2]) / cb[:, 2]
    d = np.minimum(np.abs(np.abs(ub - X[bq, 0]) - 0.5), np.abs(np.abs(vb - X[bq, 1]) - 0.5))
    assert len(bp) >= 100 and d.max() < 2e-4 and (d < 1e-5).sum() >= 20


def test_float32_restatement_reproduces_the_reference_choice(scene, selection, gold):
    gtreproj, w2c, intr, xy = _queries(scene, selection, gold)
    cloud = gold["cloud"].astype(np.float64)
    for centre in (gtreproj.cloud_centre(cloud), np.zeros(3)):  # as the host module feeds the kernel, and not recentred
        table = gtreproj.query_table(w2c, intr, xy, centre)
        keys = GR.pixel_nearest_f32(table, (cloud - centre).astype(np.float32))
        idx, depth = gtreproj.split_keys(keys)
        assert np.array_equal(idx, gold["ref_gt_index"])
        assert (depth > 0).all() and np.isfinite(depth).all()
    # a split of the cloud gives the same keys, and all-ones reads as "no point"
    a = GR.pixel_nearest_f32(table, cloud[:1000].astype(np.float32))
    b = GR.pixel_nearest_f32(table, cloud[1000:].astype(np.float32), p0=1000, best=a)
    assert np.array_equal(b, keys)
    idx, depth = gtreproj.split_keys(np.array([GR.NO_POINT, np.uint64((0x3F800000 << 32) | 7)], dtype=np.uint64))
    assert idx.tolist() == [-1, 7] and depth[1] == 1.0 and np.isinf(depth[0])


def test_image_errors_restated_against_the_reference(scene, gold):
    """The per-image means of the two modes from the launch's own arrays, restated: reference_unmatched reproduces the
    reference's numbers (its float32 matmul and ours differ in the last bits), the default leaves the unmatched key-points out."""
    from neuralrecon_w_amd import gtreproj

    for mode, want in ((True, gold["ref_image_error"].astype(np.float64)), (False, gold["image_error_f64_default"])):
        proj, xyz, cam_idx, pt_idx, xy, seg = gtreproj.image_observations(scene, reference_unmatched=mode)
        assert seg[-1] == len(cam_idx) == len(pt_idx) == len(xy) and proj.dtype == np.float32 and xyz.dtype == np.float32
        e = GR.reproj_errors_f32(proj, xyz, cam_idx, pt_idx, xy)
        means = GR.seg_sums_f64(e, seg) / np.diff(seg)
        assert np.abs(means - want).max() <= 1e-5 * want.max()
    n_all = sum(len(im["point3d_ids"]) for im in scene["images"].values())
    n_matched = sum(int((im["point3d_ids"] >= 0).sum()) for im in scene["images"].values())
    assert gtreproj.image_observations(scene, True)[5][-1] == n_all > n_matched == gtreproj.image_observations(scene, False)[5][-1]
    # the two modes keep the same images at the fixture's threshold, and drop exactly one
    thr = float(gold["img_reproj_error"])
    assert np.array_equal(gold["ref_image_error"] < thr, gold["kept"]) and np.array_equal(gold["image_error_f64_default"] < thr, gold["kept"])
    assert (~gold["kept"]).sum() == 1


def test_command_line_parses():
    spec = importlib.util.spec_from_file_location("reproj_error_cli", os.path.join(ROOT, "scripts", "reproj_error.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    a = ap.parse_args(["--data_dir", "d", "--gt_pcd_path", "g.ply"])
    # the reference's flags and defaults (tools/reproj_error.py:249-269)
    assert (a.reconstuct_path, a.track_length, a.reproj_error, a.batch_size, a.img_reproj_error) == ("dense/sparse", 200, 0.4, 2, 300)
    assert a.out_dir == os.path.join("samples", "reproject") and not a.reference_unmatched and not a.visualize and a.chunk is None
    b = ap.parse_args(["--data_dir", "d", "--gt_pcd_path", "g.ply", "--reconstuct_path", "x", "--track_length", "3", "--reproj_error", "0.5",
                       "--batch_size", "8", "--img_reproj_error", "20", "--out_dir", "o", "--reference_unmatched", "--visualize", "--chunk", "1000"])
    assert (b.reconstuct_path, b.track_length, b.reproj_error, b.batch_size, b.img_reproj_error, b.out_dir, b.chunk) == ("x", 3, 0.5, 8, 20, "o", 1000)
    assert b.reference_unmatched and b.visualize
    with pytest.raises(SystemExit):
        ap.parse_args(["--gt_pcd_path", "g.ply"])


def test_binding_declares_the_entry_points():
    import ctypes as C

    from neuralrecon_w_amd import lib as L

    assert {"ncw_pixel_nearest", "ncw_reproj_errors"} <= set(L.exported_symbols()) and L.ABI_VERSION >= 26
    assert C.sizeof(L.NcwPixelQuery) == 72
    src = open(os.path.join(ROOT, "include", "neuconw_hip.h")).read()
    assert "#define NCW_PIXNN_WG_POINTS %d\n" % L.PIXNN_WG_POINTS in src and "#define NCW_PIXNN_QUERY_TILE %d\n" % L.PIXNN_QUERY_TILE in src


def test_no_cpu_fallback():
    from neuralrecon_w_amd import gtreproj
    from neuralrecon_w_amd import lib as L

    with pytest.raises(L.NeuconwHipError, match="no CPU fallback"):
        gtreproj.nearest_on_pixel(np.zeros((1, 3, 4)), np.ones((1, 4)), np.zeros((1, 2)), np.zeros((4, 3)), device="cpu")
    with pytest.raises(L.NeuconwHipError, match="no CPU fallback"):
        gtreproj.reproj_errors(np.zeros((1, 3, 4)), np.zeros((1, 3)), [0], [0], np.zeros((1, 2)), [0, 1], device="cpu")
