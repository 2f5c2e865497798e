"""Golden scene and vectors for the scene preparation (neuralrecon_w_amd.sceneprep, csrc/ncw_roi.hip).

Writes the scene tests/golden/split_scene/ --
  dense/sparse/{cameras,images,points3D}.bin : nine registered PINHOLE images (VIEWS below: look-at from `pos` to `target`, up =
                  +z, fx = fy = f * width, cx = w / 2, cy = h / 2) around the sphere of config.yaml, origin (0.1, -0.1, 0.2),
                  radius 1.2, and 320 SfM points whose track lengths run 1 .. 4 (those with 2 or fewer do not count for the box);
                  the sizes are ragged on purpose: `big` spans many workgroups, `row` and `col` are one pixel thin and
                  consecutive views meet inside a wave;
  dense/sparse_filtered_3/images.bin : a subset of the images (the min_observation rule);
  dense/images/*.jpg : the images, stored as PNG bytes (lossless; PIL reads by content);
  semantic_maps/*.npz : label maps -- `col` sits EXACTLY at static share 0.6 (dropped: the rule is >), `away` at exactly 0
                  (dropped at threshold 0 too), `tele` well below (0.2), the others well above; `nomap.jpg`, which is neither
                  registered nor has a map, stands for an image without a map file;
  config.yaml        : written by hand here (origin, radius and the keys the other tools read)
-- and records tests/golden/split_golden.npz by RUNNING the reference's own functions on CPU against a temporary copy of the
scene (view_selection deletes and recreates trash_images/):
  * tools/prepare_data/dataset_filter_utils.py `view_selection` at roi_threshold 0.5 and 0 (min_observation -1, and 3 at 0.5):
    the returned names; the per-view float32 ROI mask and count, captured by wrapping torch.count_nonzero; the K, pose and
    size it hands to get_ray_directions / get_rays for every image, captured by wrapping those two in its namespace;
  * `filter_image_based_on_transient_percent` at 0.6 and 0 on all nine names: the returned names, the static shares (captured
    by wrapping np.count_nonzero), and what it does with `nomap.jpg` (the exception's type);
  * tools/pre_process.py `generate_config` on the scene's points with more than 2 observations (:102-108), read back from
    the yaml it writes;
  * the float64 restatement of the predicate (tests/_roi_ref.py) with, per pixel, dist_ray, dist_cam and dot.
Seams: `Tensor.cuda` is the identity, torchvision / kornia as in make_golden_view.py, `torchvision.models` a MagicMock.
The script ASSERTS the three fixture conditions tests/test_split_host.py checks again: the ambiguous band holds at most 1 % of
any view's pixels, the reference's float32 mask equals float64 on every pixel outside the band, and no view's float64 count lies
within its band count of threshold x pixels for the positive thresholds the tests use.
No reference text is stored, only data.   Run:  python tests/golden/make_golden_split.py
"""
import importlib
import json
import os
import shutil
import struct
import sys
import tempfile
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
from tests import _roi_ref as RR  # noqa: E402

SCENE = os.path.join(HERE, "split_scene")
ORIGIN, RADIUS = np.array([0.1, -0.1, 0.2]), 1.2
VIEWS = [  # name, image id, pos, target, (w, h), focal / width
    ("centre", 7, (3.1, 0.3, 1.0), ORIGIN, (37, 23), 0.9),
    ("away", 3, (3.1, 0.3, 1.0), (6.0, 0.6, 2.0), (37, 23), 0.9),
    ("inside", 11, (0.4, 0.2, 0.5), (5.0, 5.0, 5.0), (33, 21), 0.8),
    ("graze", 5, (2.6, -1.9, 0.4), ORIGIN + [0.9, 1.1, 0.0], (41, 29), 1.1),
    ("tele", 2, (-5.0, 2.0, 1.5), ORIGIN, (29, 31), 4.0),
    ("row", 13, (0.2, 3.3, -0.8), ORIGIN + [0.5, 0.0, 0.0], (64, 1), 1.0),
    ("col", 17, (0.2, -3.3, 0.8), ORIGIN + [0.0, 0.0, 0.6], (1, 50), 50.0),
    ("big", 19, (-2.0, -2.2, 1.9), ORIGIN + [0.3, -0.6, 0.2], (131, 71), 0.7),
    ("behind", 23, (1.5, 0.2, 0.3), (4.0, 0.5, 0.4), (35, 25), 0.6),
]
FILTERED_3 = ["centre", "inside", "graze", "tele", "row"]
STATIC = {"centre": 0.9, "away": 0.0, "inside": 0.85, "graze": 0.95, "tele": 0.2, "row": 0.75, "col": 0.6, "big": 0.9, "behind": 0.8}
TRANSIENT = ["person", "car", "bicycle", "minibike", "tree"]  # prepare_data_split.py:44
TRANSIENT_IDS = [12, 20, 127, 116, 4]
THRESHOLDS_ROI, THRESHOLDS_STATIC = (0.5, 0.0), (0.6, 0.0)


def write_scene():
    rs = np.random.RandomState(31)
    for sub in ("dense/sparse", "dense/sparse_filtered_3", "dense/images", "semantic_maps"):
        os.makedirs(os.path.join(SCENE, sub), exist_ok=True)
    xyz = ORIGIN + rs.normal(size=(320, 3)) * [0.7, 0.5, 0.4]
    with open(os.path.join(SCENE, "dense", "sparse", "points3D.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(xyz)))
        for i, p in enumerate(xyz):
            track = 1 + i % 4
            fh.write(struct.pack("<QdddBBBd", 1 + 3 * i, *p, *rs.randint(0, 256, 3).tolist(), 0.4 + 0.003 * i))
            fh.write(struct.pack("<Q", track) + b"".join(struct.pack("<ii", VIEWS[(i + t) % len(VIEWS)][1], t) for t in range(track)))
    with open(os.path.join(SCENE, "dense", "sparse", "cameras.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(VIEWS)))
        for k, (_, _, _, _, (w, h), f) in enumerate(VIEWS):
            fh.write(struct.pack("<iiQQdddd", k + 1, 1, w, h, f * w, f * w, w / 2, h / 2))
    rows = []
    for k, (name, iid, pos, target, (w, h), f) in enumerate(VIEWS):
        q, t = MC.look_at(np.array(pos, dtype=np.float64), np.array(target, dtype=np.float64), 0.0)
        rows.append((name, struct.pack("<i7di", iid, *q, *t, k + 1) + (name + ".jpg").encode() + b"\x00" + struct.pack("<Q", 0)))
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([255 * xx / max(w - 1, 1), 255 * yy / max(h - 1, 1), 127 + 100 * np.sin(0.3 * xx + 0.2 * yy + k)], -1)
        write_png(os.path.join(SCENE, "dense", "images", name + ".jpg"), np.clip(img, 0, 255).astype(np.uint8))
        # the label map: the first round(share * h * w) pixels (row-major) static (building / sky / road), the rest transient
        n_static = int(round(STATIC[name] * h * w))
        assert n_static / (h * w) == STATIC[name] or name not in ("col", "away"), name
        lab = np.empty(h * w, dtype=np.uint8)
        lab[:n_static] = np.array([1, 2, 6], dtype=np.uint8)[np.arange(n_static) % 3]
        lab[n_static:] = np.array(TRANSIENT_IDS, dtype=np.uint8)[np.arange(h * w - n_static) % 5]
        np.savez_compressed(os.path.join(SCENE, "semantic_maps", name + ".npz"), lab.reshape(h, w))
    for sub, keep in (("sparse", [v[0] for v in VIEWS]), ("sparse_filtered_3", FILTERED_3)):
        with open(os.path.join(SCENE, "dense", sub, "images.bin"), "wb") as fh:
            fh.write(struct.pack("<Q", len(keep)) + b"".join(r for n, r in rows if n in keep))
    import yaml

    lo, hi = ORIGIN - [1.0, 0.8, 0.7], ORIGIN + [1.0, 0.8, 0.7]
    with open(os.path.join(SCENE, "config.yaml"), "w") as fh:
        yaml.safe_dump({"name": "split_scene", "origin": ORIGIN.tolist(), "radius": RADIUS, "eval_bbx": [lo.tolist(), hi.tolist()],
                        "sfm2gt": np.eye(4).tolist(), "min_track_length": 2, "voxel_size": 0.1}, fh, sort_keys=False)


def install_stubs():
    MC.install_stubs()
    sys.modules["torchvision"].models = mock.MagicMock()
    sys.modules["torchvision.models"] = sys.modules["torchvision"].models


def main():
    write_scene()
    install_stubs()
    sys.path.insert(0, ref_import.REFERENCE_ROOT)
    try:
        dfu = importlib.import_module("tools.prepare_data.dataset_filter_utils")
        pre = importlib.import_module("tools.pre_process")
        cu = importlib.import_module("utils.colmap_utils")
    finally:
        sys.path.remove(ref_import.REFERENCE_ROOT)
    from neuralrecon_w_amd import sceneprep

    rec = {}
    names = [v[0] + ".jpg" for v in VIEWS]
    tmp = tempfile.mkdtemp()
    try:
        root = os.path.join(tmp, "split_scene")
        shutil.copytree(SCENE, root)
        # ---- view_selection; the mask of every view through torch.count_nonzero
        masks = []
        real_count = torch.count_nonzero

        def spy(x, *a, **k):
            masks.append(x.detach().clone())
            return real_count(x, *a, **k)

        # the K and the pose the reference hands to its ray functions for every image (names it star-imports: patched in its namespace)
        ref_cams = []
        real_dirs, real_rays = dfu.get_ray_directions, dfu.get_rays

        def dirs_spy(h, w, K):
            ref_cams.append({"wh": (int(w), int(h)), "K": np.array(K, dtype=np.float32)})
            return real_dirs(h, w, K)

        def rays_spy(directions, c2w):
            ref_cams[-1]["c2w"] = c2w.detach().numpy().astype(np.float32).copy()
            return real_rays(directions, c2w)

        with mock.patch.object(torch.Tensor, "cuda", lambda self, *a, **k: self), mock.patch.object(torch, "count_nonzero", spy), \
                mock.patch.object(dfu, "get_ray_directions", dirs_spy), mock.patch.object(dfu, "get_rays", rays_spy):
            for thr in THRESHOLDS_ROI:
                del masks[:]
                kept = dfu.view_selection(root, ORIGIN.tolist(), RADIUS, -1, thr)
                rec["roi_kept_%03d" % round(100 * thr)] = np.array([str(k) for k in kept])
                if thr == THRESHOLDS_ROI[0]:
                    assert len(masks) == len(VIEWS) and all(m.dtype == torch.bool for m in masks)
                    ref_masks = [m.numpy().astype(np.uint8) for m in masks]
                    rec.update(ref_K=np.stack([c["K"] for c in ref_cams[:len(VIEWS)]]), ref_c2w=np.stack([c["c2w"] for c in ref_cams[:len(VIEWS)]]),
                               ref_wh=np.array([c["wh"] for c in ref_cams[:len(VIEWS)]]))
            kept = dfu.view_selection(root, ORIGIN.tolist(), RADIUS, 3, THRESHOLDS_ROI[0])
            rec["roi_kept_050_minobs3"] = np.array([str(k) for k in kept])
        # ---- the transient filter on all nine names; the shares through np.count_nonzero
        shares = []
        real_np_count = np.count_nonzero

        def np_spy(x, *a, **k):
            r = real_np_count(x, *a, **k)
            if getattr(x, "ndim", 0) == 2:
                shares.append(r / (x.shape[0] * x.shape[1]))
            return r

        paths = np.array(names)[:, np.newaxis]
        for thr in THRESHOLDS_STATIC:
            del shares[:]
            with mock.patch.object(np, "count_nonzero", np_spy):
                kept = dfu.filter_image_based_on_transient_percent(root, "semantic_maps", paths, TRANSIENT, thr)
            rec["static_kept_%03d" % round(100 * thr)] = np.array([str(k) for k in kept[:, 0]])
            rec["static_share"] = np.array(shares, dtype=np.float64)
        assert len(rec["static_share"]) == len(names)
        try:
            dfu.filter_image_based_on_transient_percent(root, "semantic_maps", np.array(["nomap.jpg"])[:, np.newaxis], TRANSIENT, 0.6)
            rec["static_missing_map"] = np.array("returned")
        except Exception as e:  # noqa: BLE001  (the type is what is recorded)
            rec["static_missing_map"] = np.array(type(e).__name__)
        # ---- generate_config on the points with more than 2 observations (pre_process.py:102-108)
        pts3d = cu.read_points3d_binary(os.path.join(root, "dense", "sparse", "points3D.bin"))
        pts = np.array([p.xyz for p in pts3d.values() if p.point2D_idxs.shape[0] > 2])
        assert 0 < len(pts) < len(pts3d)
        out = os.path.join(tmp, "cfg")
        os.makedirs(out)
        pre.generate_config("split_scene", out, pts)
        import yaml

        with open(os.path.join(out, "config.yaml")) as fh:
            text = fh.read()
        cfg = yaml.safe_load(text)
        rec["config_json"] = np.array(json.dumps(cfg))  # json keeps the key order and float64 values exactly (repr round trip)
        rec["config_yaml_keys"] = np.array([ln.split(":")[0] for ln in text.splitlines() if ln and ln[0] not in " -"])
        rec["config_n_points"] = np.array(len(pts))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    # ---- the views as sceneprep builds them, the float64 restatement, the band, the three conditions
    cams = sceneprep.scene_cameras(SCENE)
    assert [c.name for c in cams] == names
    assert np.array_equal(rec["ref_wh"], [[c.width, c.height] for c in cams]) and np.array_equal(rec["ref_K"], np.stack([c.K for c in cams]))
    prefix = sceneprep.pixel_prefix(cams)
    ref_mask = np.concatenate([m.reshape(-1) for m in ref_masks])
    assert len(ref_mask) == prefix[-1]
    f64 = [RR.roi_f64(c.K, c.c2w, c.width, c.height, ORIGIN, RADIUS) for c in cams]
    cat = {k: np.concatenate([f[k] for f in f64]) for k in ("dist_ray", "dist_cam", "dot", "roi", "band")}
    band_count = np.array([int(f["band"].sum()) for f in f64])
    count64 = np.array([int(f["roi"].sum()) for f in f64])
    count32 = np.array([int(m.sum()) for m in ref_masks])
    npix = np.diff(prefix)
    worst = float((band_count / npix).max())
    assert worst <= 0.01, worst
    out_band = ~cat["band"]
    n_diff_out = int((ref_mask[out_band] != cat["roi"][out_band]).sum())
    assert n_diff_out == 0, n_diff_out
    for thr in THRESHOLDS_ROI:
        if thr > 0:  # `share < 0` holds for no count: threshold 0 cannot flip a view
            assert (np.abs(count64 - thr * npix) > band_count).all(), (thr, count64, npix, band_count)
    rec.update(names=np.array(names), ids=np.array([c.image_id for c in cams]), prefix=prefix, wh=np.array([[c.width, c.height] for c in cams]),
               K=np.stack([c.K for c in cams]), c2w=np.stack([c.c2w for c in cams]), origin=ORIGIN, radius=np.float64(RADIUS),
               ref_mask=ref_mask, ref_count=count32, count64=count64, band_count=band_count, roi64=cat["roi"].astype(np.uint8),
               band=cat["band"].astype(np.uint8), dist_ray=cat["dist_ray"], dist_cam=cat["dist_cam"], dot=cat["dot"],
               filtered_3=np.array([n + ".jpg" for n in FILTERED_3]))
    path = os.path.join(HERE, "split_golden.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")
    print("shares fp64", np.round(count64 / npix, 4).tolist(), "fp32 == fp64 on", int((ref_mask == cat["roi"]).sum()), "of", len(ref_mask),
          "pixels; worst band share %.4f" % worst)
    print({k: rec[k].tolist() for k in ("roi_kept_050", "roi_kept_000", "roi_kept_050_minobs3", "static_kept_060", "static_kept_000",
                                        "static_share", "static_missing_map")})


if __name__ == "__main__":
    main()
