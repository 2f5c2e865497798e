"""Golden scene and vectors for the ground-truth reprojection error (neuralrecon_w_amd.gtreproj, csrc/ncw_gtreproj.hip).

Writes the scene tests/golden/gtreproj_scene/ --
  dense/sparse/{cameras,images,points3D}.bin : ten registered PINHOLE images of ragged sizes (VIEWS below; the largest 131 x 71)
                  that look at a bumpy sheet from one side, and 300 SfM points on it whose tracks run from 1 to 8 observations
                  (thresholds 3 / 0.4 select a few dozen).  Key-points = the float64 projection + noise; some sit at k + 0.5
                  exactly (round: ties to even); every image also holds key-points WITHOUT a 3-D point (id -1); the key-points of
                  `bad` are off by 25 px, so that its mean error puts it above img_reproj_error = 20 in both modes;
  dense/images/*.jpg : the images, stored as PNG bytes (only their names are read);
  config.yaml        : sfm2gt with rotation, scale 1.7 and the translation (100, -60, 30)
-- and tests/golden/gtreproj_golden.npz: the ground-truth cloud (float32-valued, as a PLY stores it: per selected track a point
on the reference pixel near the SfM point, one behind it on the same pixel, one BEHIND THE CAMERA that projects onto it, and a
few thousand points of the sheet), the marked band points (placed within a few float32 ulp of a query pixel's 0.5 boundary; never
part of the cloud the references see), and the golden recorded by RUNNING the reference's own functions on CPU:
  * tools/reproj_error.py `get_entrinsics`, `get_intrinsic`, `image_reproj_error` on the scene;
  * `gt_reproject_error` as a whole (track_length 3, reproj_error 0.4, batch_size 2, img_reproj_error 20): the returned mean, the
    per-element errors (its plt.plot call), every `get_gt_point` call's arguments and result (a spy in its namespace), from
    which the chosen indices, the selection (track_pts2D: image id, point2D idx, x, y) and the reference views follow.
Seams: `Tensor.cuda` is the identity; open3d (read_point_cloud returns the cloud; the writers do nothing), imageio.imwrite and
matplotlib.pyplot are stubs installed here; the scene is copied to a temporary directory whose dense/images gets two extra
entries that sort first, because `get_image_id` drops the first two entries of the sorted directory.
The script ASSERTS the fixture's conditions, which tests/test_gtreproj_host.py checks again:
  * every selected track's reference pixel is hit by a ground-truth point (the reference cannot say "none");
  * no point of the cloud projects, in float64, within 1e-3 px of a rounding boundary of any query pixel or has |c_2| < 1e-6,
    and the two nearest hits of a query differ in depth by more than 1e-4 relative;
  * the reference's float32 choice equals the float64 choice on EVERY query: no query is left out.
No reference text is stored, only data.   Run:  python tests/golden/make_golden_gtreproj.py
"""
import importlib
import os
import shutil
import struct
import sys
import tempfile
import types
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_golden_cache as MC  # noqa: E402
from make_golden_view import write_png  # noqa: E402
from oracle import ref_import  # noqa: E402
from tests import _gtreproj_ref as GR  # noqa: E402

SCENE = os.path.join(HERE, "gtreproj_scene")
VIEWS = [  # name, image id, pos, target, (w, h), focal / width
    ("a", 4, (0.2, -3.0, 0.4), (0.0, 0.0, 0.0), (131, 71), 1.1),
    ("b", 9, (1.2, -2.8, 0.1), (0.1, 0.0, 0.1), (97, 61), 1.0),
    ("c", 2, (-1.1, -2.9, 0.6), (-0.1, 0.0, 0.0), (83, 67), 0.9),
    ("d", 15, (0.6, -3.3, -0.5), (0.0, 0.0, -0.1), (101, 53), 1.2),
    ("e", 7, (-0.5, -2.6, -0.3), (0.0, 0.0, 0.1), (64, 64), 0.8),
    ("bad", 11, (0.9, -3.1, 0.8), (0.1, 0.0, 0.0), (89, 59), 1.0),
    ("f", 21, (-1.4, -3.0, -0.2), (0.0, 0.0, 0.0), (127, 70), 1.3),
    ("g", 5, (0.0, -2.7, 0.9), (0.0, 0.0, 0.1), (75, 71), 0.85),
    ("h", 30, (1.6, -2.9, -0.4), (0.2, 0.0, 0.0), (113, 47), 1.15),
    ("i", 12, (-0.3, -3.4, 0.2), (0.0, 0.0, -0.05), (59, 41), 0.75),
]
TRACK_LENGTH, REPROJ_ERROR, IMG_REPROJ_ERROR = 3, 0.4, 20.0
N_SFM, N_SHEET = 300, 5000


def sfm_to_gt():
    a = np.array([0.3, -0.5, 0.8])
    a /= np.linalg.norm(a)
    t = 0.7
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = 1.7 * R, (100.0, -60.0, 30.0)
    return M


def sheet(x, z):
    return 0.25 * np.sin(1.7 * x) * np.cos(1.3 * z) + 0.1 * x  # y of the surface over (x, z); the cameras sit at y ~ -3


def cameras():
    cams = []
    for k, (name, iid, pos, target, (w, h), f) in enumerate(VIEWS):
        q, t = MC.look_at(np.array(pos, dtype=np.float64), np.array(target, dtype=np.float64), 3.0 * k)
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = MC.qvec2rotmat(q), t
        K = np.array([[f * w, 0, w / 2 + 0.25], [0, f * w * 1.02, h / 2 - 0.5], [0, 0, 1]])
        cams.append(dict(name=name + ".jpg", id=iid, cam_id=k + 1, q=q, t=t, E=E, K=K, w=w, h=h))
    return cams


def project(E, K, p):
    c = p @ E[:3, :3].T + E[:3, 3]
    return np.stack([K[0, 0] * c[:, 0] / c[:, 2] + K[0, 2], K[1, 1] * c[:, 1] / c[:, 2] + K[1, 2]], -1), c[:, 2]


def write_scene():
    rs = np.random.RandomState(77)
    cams = cameras()
    for sub in ("dense/sparse", "dense/images"):
        os.makedirs(os.path.join(SCENE, sub), exist_ok=True)
    xz = rs.uniform(-0.8, 0.8, size=(N_SFM, 2))
    xyz = np.stack([xz[:, 0], sheet(xz[:, 0], xz[:, 1]), xz[:, 1]], -1)
    kps = {c["id"]: [] for c in cams}  # per image: (x, y, point3D id)
    points = []
    for i, p in enumerate(xyz):
        pid = 2 + 3 * i  # ids with gaps
        want = 1 + i % 8
        order = [(i + 3 * j) % len(cams) for j in range(len(cams))]
        track = []
        for k in order:
            c = cams[k]
            uv, depth = project(c["E"], c["K"], p[None])
            if not (depth[0] > 0 and 2 < uv[0, 0] < c["w"] - 3 and 2 < uv[0, 1] < c["h"] - 3):
                continue
            xy = uv[0] + rs.normal(0, 0.25, 2) + (25.0 if c["name"] == "bad.jpg" else 0.0)
            if i % 11 == 0 and not track:
                xy = np.floor(xy) + 0.5  # a reference key-point at k + 0.5: ties to even
            track.append((c["id"], len(kps[c["id"]])))
            kps[c["id"]].append((xy[0], xy[1], pid))
            if len(track) == want:
                break
        if track:
            points.append((pid, p, 0.2 + 0.6 * rs.rand(), track))
    for c in cams:  # key-points without a 3-D point, in between the others
        for _ in range(6):
            kps[c["id"]].insert(rs.randint(0, len(kps[c["id"]]) + 1), (rs.uniform(0, c["w"]), rs.uniform(0, c["h"]), -1))
    # the inserts moved the point2D indices: rebuild them from the lists
    where = {}
    for iid, lst in kps.items():
        seen = {}
        for j, (_, _, pid) in enumerate(lst):
            if pid >= 0:
                seen[pid] = j
        where[iid] = seen
    with open(os.path.join(SCENE, "dense", "sparse", "points3D.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(points)))
        for pid, p, err, track in points:
            fh.write(struct.pack("<QdddBBBd", pid, *p, *rs.randint(0, 256, 3).tolist(), err))
            fh.write(struct.pack("<Q", len(track)) + b"".join(struct.pack("<ii", iid, where[iid][pid]) for iid, _ in track))
    with open(os.path.join(SCENE, "dense", "sparse", "cameras.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(cams)))
        for c in cams:
            fh.write(struct.pack("<iiQQdddd", c["cam_id"], 1, c["w"], c["h"], c["K"][0, 0], c["K"][1, 1], c["K"][0, 2], c["K"][1, 2]))
    with open(os.path.join(SCENE, "dense", "sparse", "images.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(cams)))
        for k, c in enumerate(cams):
            fh.write(struct.pack("<i7di", c["id"], *c["q"], *c["t"], c["cam_id"]) + c["name"].encode() + b"\x00")
            fh.write(struct.pack("<Q", len(kps[c["id"]])) + b"".join(struct.pack("<ddq", *kp) for kp in kps[c["id"]]))
            yy, xx = np.mgrid[0:c["h"], 0:c["w"]]
            img = np.stack([255 * xx / (c["w"] - 1), 255 * yy / (c["h"] - 1), 0 * xx + 20 * k], -1)
            write_png(os.path.join(SCENE, "dense", "images", c["name"]), np.clip(img, 0, 255).astype(np.uint8))
    import yaml

    with open(os.path.join(SCENE, "config.yaml"), "w") as fh:
        yaml.safe_dump({"name": "gtreproj_scene", "origin": [0.0, 0.0, 0.0], "radius": 1.5, "eval_bbx": [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]],
                        "sfm2gt": sfm_to_gt().tolist(), "min_track_length": 2, "voxel_size": 0.1}, fh, sort_keys=False)


def back_project(E, K, uv, depth):
    cam = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * depth, (uv[:, 1] - K[1, 2]) / K[1, 1] * depth, depth], -1)
    return (cam - E[:3, 3]) @ np.linalg.inv(E[:3, :3]).T  # A^-1 (c - t); A is a rotation, or a scaled one for a view of the cloud


def make_cloud(scene, sel, M):
    """The ground-truth cloud (GT coordinates, float32-valued float64) for the selection `sel`, free of band points."""
    from neuralrecon_w_amd import gtreproj as G

    rs = np.random.RandomState(5)
    index_of = {iid: k for k, iid in enumerate(scene["image_ids"])}
    ref = sel["seg_start"][:-1]
    cam = np.array([index_of[int(g)] for g in sel["obs_image_id"][ref]])
    pts = []
    for t, k in enumerate(cam):
        E, K = scene["E"][k], scene["K"][k].astype(np.float64)
        X = np.rint(sel["obs_xy"][ref[t]].astype(np.float32)).astype(np.float64)
        p = scene["xyz"][sel["point_row"][t]]
        depth = (E[:3, :3] @ p + E[:3, 3])[2]
        uv = (X + rs.uniform(-0.3, 0.3, 2))[None]
        pts.append(back_project(E, K, uv, np.array([depth * (1 + rs.normal(0, 0.004))])))
        pts.append(back_project(E, K, (X + rs.uniform(-0.3, 0.3, 2))[None], np.array([depth * 1.3])))   # behind it, same pixel
        pts.append(back_project(E, K, (X + rs.uniform(-0.3, 0.3, 2))[None], np.array([-depth * 0.4])))  # behind the camera
    xz = rs.uniform(-1.0, 1.0, size=(N_SHEET, 2))
    pts.append(np.stack([xz[:, 0], sheet(xz[:, 0], xz[:, 1]) + rs.normal(0, 0.01, N_SHEET), xz[:, 1]], -1))
    sfm = np.concatenate(pts)
    gt = (sfm @ M[:3, :3].T + M[:3, 3]).astype(np.float32).astype(np.float64)
    # drop the sheet points that fall into a band or tie a depth (the designed points are checked, not dropped)
    w2c = (scene["E"] @ np.linalg.inv(M))[cam, :3, :]
    intr = np.stack([scene["K"][cam, 0, 0], scene["K"][cam, 1, 1], scene["K"][cam, 0, 2], scene["K"][cam, 1, 2]], -1)
    n_design = len(gt) - N_SHEET
    keep = np.ones(len(gt), dtype=bool)
    for j in range(n_design, len(gt)):
        _, band, _, _ = GR.pixel_nearest_f64(w2c, intr, sel["obs_xy"][ref], gt[j:j + 1])
        keep[j] = not band.any()
    gt = gt[keep]
    for _ in range(20):  # depth near-ties: drop the farther sheet point of the pair
        idx, band, gap, second = GR.pixel_nearest_f64(w2c, intr, sel["obs_xy"][ref], gt)
        bad = np.flatnonzero(gap <= 1e-4)
        if not len(bad):
            break
        gt = np.delete(gt, [s if s >= n_design else i for i, s in zip(idx[bad], second[bad])], axis=0)
    return gt, w2c, intr, G


def make_band_points(w2c, intr, xy, M):
    """Points within a few float32 ulp of the 0.5 boundaries of the first queries' pixels, in u and in v, on both sides."""
    out, of_query = [], []
    for q in range(min(6, len(w2c))):
        W = np.eye(4)
        W[:3] = w2c[q]
        K = np.array([[intr[q, 0], 0, intr[q, 2]], [0, intr[q, 1], intr[q, 3]], [0, 0, 1]], dtype=np.float64)
        X = np.rint(xy[q].astype(np.float32)).astype(np.float64)
        for axis in (0, 1):
            for side in (-0.5, 0.5):
                for e in (-2e-5, -6e-6, -1e-6, 0.0, 1e-6, 6e-6, 2e-5):
                    uv = X.copy()
                    uv[axis] += side + e
                    uv[1 - axis] += 0.1
                    out.append(back_project(W, K, uv[None], np.array([2.0 + 0.01 * len(out)])))
                    of_query.append(q)
    return np.concatenate(out).astype(np.float32).astype(np.float64), np.array(of_query)


def install_stubs(cloud):
    MC.install_stubs()
    o3d = types.ModuleType("open3d")
    o3d.io = types.SimpleNamespace(read_point_cloud=lambda path: types.SimpleNamespace(points=cloud), write_point_cloud=lambda *a, **k: True)
    o3d.geometry = types.SimpleNamespace(PointCloud=lambda: types.SimpleNamespace(points=None))
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: a)
    plots = []
    plt = types.ModuleType("matplotlib.pyplot")
    plt.plot = lambda *a, **k: plots.append([np.array(x) for x in a])
    plt.savefig = lambda *a, **k: None
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = plt
    imageio = types.ModuleType("imageio")
    imageio.imwrite = lambda *a, **k: None
    sys.modules.update({"open3d": o3d, "matplotlib": mpl, "matplotlib.pyplot": plt, "imageio": imageio})
    return plots


def main():
    write_scene()
    from neuralrecon_w_amd import gtreproj as G

    M = sfm_to_gt()
    scene = G.read_scene(SCENE)
    # the kept images and the selection come from the float64 restatement here; the reference's own run below must agree
    obs = G.image_observations(scene, reference_unmatched=True)
    e64 = GR.reproj_errors_f64(*obs[:5])
    img64_ref_mode = np.array([e64[a:b].mean() for a, b in zip(obs[5][:-1], obs[5][1:])])
    obs_d = G.image_observations(scene, reference_unmatched=False)
    e64d = GR.reproj_errors_f64(*obs_d[:5])
    img64_default = np.array([e64d[a:b].mean() for a, b in zip(obs_d[5][:-1], obs_d[5][1:])])
    kept = img64_ref_mode < IMG_REPROJ_ERROR
    assert np.array_equal(kept, img64_default < IMG_REPROJ_ERROR) and kept.sum() == len(kept) - 1, (img64_ref_mode, img64_default)
    assert np.abs(img64_ref_mode - IMG_REPROJ_ERROR).min() > 1.0 and np.abs(img64_default - IMG_REPROJ_ERROR).min() > 1.0
    kept_ids = [iid for iid, k in zip(scene["image_ids"], kept) if k]
    sel = G.select_tracks(scene, kept_ids, TRACK_LENGTH, REPROJ_ERROR)
    n_sel = len(sel["point_row"])
    assert 24 <= n_sel <= 80, n_sel
    cloud, w2c, intr, _ = make_cloud(scene, sel, M)
    ref_obs = sel["seg_start"][:-1]
    qxy = sel["obs_xy"][ref_obs]
    idx64, band, gap, _ = GR.pixel_nearest_f64(w2c, intr, qxy, cloud)
    assert (idx64 >= 0).all() and not band.any() and gap.min() > 1e-4, (idx64.min(), band.sum(), gap.min())
    assert len(cloud) <= 8192, len(cloud)
    band_pts, band_query = make_band_points(w2c, intr, qxy, M)
    # ---- the reference
    plots = install_stubs(cloud)
    sys.path.insert(0, ref_import.REFERENCE_ROOT)
    try:
        rp = importlib.import_module("tools.reproj_error")
        cu = importlib.import_module("utils.colmap_utils")
    finally:
        sys.path.remove(ref_import.REFERENCE_ROOT)
    rec = {}
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    try:
        root = os.path.join(tmp, "gtreproj_scene")
        shutil.copytree(SCENE, root)
        for extra in ("!0", "!1"):  # get_image_id drops the first two entries of the sorted directory
            open(os.path.join(root, "dense", "images", extra), "w").close()
        os.chdir(tmp)  # the reference writes samples/, reprojects/ and a plot into the working directory
        calls = []
        real_get = rp.get_gt_point

        def spy(pcd, cam_pose, cam_intrinsic, track_pts2D):
            out = real_get(pcd, cam_pose, cam_intrinsic, track_pts2D)
            calls.append((cam_pose.numpy().copy(), cam_intrinsic.numpy().copy(), track_pts2D.numpy().copy(), out.numpy().copy().reshape(-1, 4)))
            return out

        with mock.patch.object(torch.Tensor, "cuda", lambda self, *a, **k: self), mock.patch.object(rp, "get_gt_point", spy):
            imdata = cu.read_images_binary(os.path.join(root, "dense/sparse/images.bin"))
            camdata = cu.read_cameras_binary(os.path.join(root, "dense/sparse/cameras.bin"))
            pts3d = cu.read_points3d_binary(os.path.join(root, "dense/sparse/points3D.bin"))
            img_ids, _ = rp.get_image_id(imdata, root)
            ent = rp.get_entrinsics(imdata, img_ids)
            Ks, whs = rp.get_intrinsic(camdata, img_ids, imdata)
            img_err = rp.image_reproj_error(imdata, pts3d, img_ids, {i: ent[k] for k, i in enumerate(img_ids)}, Ks)
            loss = rp.gt_reproject_error(root, "gt.ply", M, "dense/sparse", TRACK_LENGTH, REPROJ_ERROR, 2, IMG_REPROJ_ERROR)
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)
    assert list(img_ids) == list(scene["image_ids"]), (img_ids, scene["image_ids"])
    assert np.array_equal(ent, scene["E"]) and np.array_equal(np.stack([Ks[i] for i in img_ids]), scene["K"])
    rec["ref_image_error"] = img_err.numpy().reshape(-1).astype(np.float32)
    assert np.array_equal(rec["ref_image_error"] < IMG_REPROJ_ERROR, kept)
    ref_pts2d = np.concatenate([c[2] for c in calls])            # [T, 4] float32: image id, point2D idx, x, y of the reference views
    ref_chosen = np.concatenate([c[3] for c in calls])[:, :3]    # [T, 3] float32: the chosen cloud points
    assert len(ref_pts2d) == n_sel, (len(ref_pts2d), n_sel)
    assert np.array_equal(ref_pts2d[:, 0], sel["obs_image_id"][ref_obs]) and np.array_equal(ref_pts2d[:, 1], sel["obs_point2d_idx"][ref_obs])
    assert np.array_equal(ref_pts2d[:, 2:], qxy.astype(np.float32))
    c32 = cloud.astype(np.float32)
    ref_index = np.array([int(np.flatnonzero((c32 == p).all(1))[0]) for p in ref_chosen])
    n_left_out = int((ref_index != idx64).sum())
    assert n_left_out == 0, (n_left_out, np.flatnonzero(ref_index != idx64))  # the cap on left-out queries is 0
    ref_errors = plots[-1][1].astype(np.float64)
    assert len(ref_errors) == sel["seg_start"][-1]
    # ---- the float32 restatement on the same queries (recentred, as the host module feeds the kernel)
    centre = G.cloud_centre(cloud)
    table = G.query_table(w2c, intr, qxy, centre)
    keys32 = GR.pixel_nearest_f32(table, (cloud - centre).astype(np.float32))
    idx32, _ = G.split_keys(keys32)
    assert np.array_equal(idx32, idx64)
    rec.update(sfm_to_gt=M, cloud=cloud.astype(np.float32), band_points=band_pts.astype(np.float32), band_query=band_query,
               image_ids=np.array(scene["image_ids"]), image_names=np.array(scene["names"]), ref_E=ent, ref_K=np.stack([Ks[i] for i in img_ids]),
               image_error_f64_reference_mode=img64_ref_mode, image_error_f64_default=img64_default, kept=kept,
               track_length=np.int64(TRACK_LENGTH), reproj_error=np.float64(REPROJ_ERROR), img_reproj_error=np.float64(IMG_REPROJ_ERROR),
               sel_point_id=sel["point_id"], sel_seg_start=sel["seg_start"], sel_obs_image_id=sel["obs_image_id"],
               sel_obs_point2d_idx=sel["obs_point2d_idx"], sel_obs_xy=sel["obs_xy"], ref_pts2d=ref_pts2d, ref_gt_index=ref_index,
               index_f64=idx64, ref_errors=ref_errors, ref_loss=np.float64(float(loss)), query_w2c=w2c, query_intr=intr)
    path = os.path.join(HERE, "gtreproj_golden.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes;", n_sel, "tracks,", len(ref_errors), "elements,", len(cloud), "cloud points,",
          len(band_pts), "band points; reference mean", float(loss), "image errors", np.round(rec["ref_image_error"], 3).tolist())


if __name__ == "__main__":
    main()
