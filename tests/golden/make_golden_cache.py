"""Golden scene and vectors for the ray-cache writer (neuralrecon_w_amd.cachebuild, csrc/ncw_cache.hip).

Writes the scene tests/golden/cache_scene/ --
  dense/sparse/{cameras,images,points3D}.bin : four registered PINHOLE images a..d of 42x27, 36x30, 40x24, 30x30 pixels around an
                  OPEN ellipsoid shell of 400 SfM points plus 24 strays (some behind the cameras); the key-points of every image
                  include point ids of -1, points outside the image, points behind the camera, pixel coordinates at exact halves
                  (round half to even) and four pixel COLLISIONS (two key-points of different depth on one pixel);
  dense/images/*.jpg : the images, stored as PNG bytes (lossless; PIL reads by content), semantic_maps/*.npz : small label maps;
  cache_scene.tsv    : a, b, d train, c test, and e.jpg, which images.bin does not register (last, see below);
  config.yaml        : eval_bbx, sfm2gt, voxel_size 0.1 (octree level 4 for both octrees), min_track_length, origin, radius
-- and records tests/golden/cache_golden.npz by RUNNING the reference's own code on CPU:
  * datasets/phototourism.py `PhototourismDataset.read_meta` for split 'train' (a, b, d) and 'eval' (c: the same per-image rows),
    use_voxel False, with and without semantics.  The constructor cannot run for this scene: it leaves `sfm_path` or
    `depth_percent` unbound for every directory name but brandenburg_gate / palacio_de_bellas_artes (phototourism.py:81-93, whose
    depth padding is random), so the object is made with __new__, given the attributes the constructor would set
    (depth_percent 0, sfm_path 'sparse') and read_meta() is called -- everything from the tsv to `all_rays` is the reference's.
    Seams: `gen_octree_from_sfm` patched out of the dataset's namespace (kaolin), `Tensor.cuda` the identity, `get_colmap_depth`
    called with device='cpu', `cv2.resize(..., INTER_NEAREST)` restated as map[floor(row hs / h), floor(col ws / w)] (cv2 is not
    installed), kornia / torchvision as in make_golden_view.py.
    (The reference pairs tsv ROW i with the i-th REGISTERED image (phototourism.py:453-462), so an unregistered name in the
    middle of the tsv shifts its splits; the unregistered row is the last one here, where that cannot happen.)
  * tools/prepare_data/prepare_data_cache.py `split_to_chunks` on the resulting lists (4 chunks, two fixed padding indices, h5py
    stubbed, cache_type npz);
  * the depth / weight formula of get_colmap_depth evaluated in float64 with the last key-point winning a collision; the script
    ASSERTS that the reference's CPU run resolves every collision that way, that the fp64 slab oracle finds kept and dropped
    pixels in every view and that at most 1 % of the rays hinge on a grazing contact (tests/test_gpu_cache.py excludes those).
No reference text is stored, only data.   Run:  python tests/golden/make_golden_cache.py
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
from make_golden_view import ToTensor, create_meshgrid, write_png  # noqa: E402
from oracle import ref_import  # noqa: E402

SCENE = os.path.join(HERE, "cache_scene")
CENTRE = np.array([0.1, -0.1, 0.2])
VOXEL_SIZE, MIN_TRACK = 0.1, 2
IMAGES = [  # name, id, (w, h), camera position, focal / w
    ("a.jpg", 7, (42, 27), (3.0, 0.4, 0.9), 0.95),
    ("b.jpg", 3, (36, 30), (-0.6, -3.1, 0.5), 0.90),
    ("c.jpg", 11, (40, 24), (-2.2, 1.8, -1.4), 1.00),
    ("d.jpg", 5, (30, 30), (0.8, 2.4, 2.2), 0.85),
]
TSV = [("a.jpg", "train"), ("b.jpg", "train"), ("c.jpg", "test"), ("d.jpg", "train"), ("e.jpg", "train")]
N_CHUNKS, PADDING = 4, [7, 2000]


def rot_to_qvec(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def qvec2rotmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def look_at(pos, target, roll_deg):
    z = target - pos
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    a = np.deg2rad(roll_deg)
    x, y = np.cos(a) * x + np.sin(a) * y, -np.sin(a) * x + np.cos(a) * y
    R = np.stack([x, y, z])  # world -> camera: right, down, front
    q = rot_to_qvec(R)
    return q, -qvec2rotmat(q) @ pos


def make_points(rs):
    u = rs.normal(size=(4000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u = u[u[:, 2] < 0.55][:400]  # the cap is left open
    shell = CENTRE + u * [0.7, 0.55, 0.45]
    strays = CENTRE + rs.uniform(-4.0, 4.0, size=(24, 3))
    xyz = np.concatenate([shell, strays])
    ids = 1 + 2 * np.arange(len(xyz))  # ids with gaps: the reference's table is indexed by id
    err = 0.3 + 1.5 * rs.rand(len(xyz))
    return ids, xyz, err


def write_scene():
    rs = np.random.RandomState(20)
    for sub in ("dense/sparse", "dense/images", "semantic_maps"):
        os.makedirs(os.path.join(SCENE, sub), exist_ok=True)
    ids, xyz, err = make_points(rs)
    with open(os.path.join(SCENE, "dense", "sparse", "points3D.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(xyz)))
        for i, p in enumerate(xyz):
            track = 2 + i % 3
            fh.write(struct.pack("<QdddBBBd", int(ids[i]), *p, *rs.randint(0, 256, 3).tolist(), float(err[i])))
            fh.write(struct.pack("<Q", track) + b"".join(struct.pack("<ii", IMAGES[(i + t) % 4][1], t) for t in range(track)))
    with open(os.path.join(SCENE, "dense", "sparse", "cameras.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(IMAGES)))
        for k, (_, _, (w, h), _, f) in enumerate(IMAGES):
            fh.write(struct.pack("<iiQQdddd", k + 1, 1, w, h, f * w, f * w * 1.03, w / 2 + 0.3, h / 2 + 0.2))
    with open(os.path.join(SCENE, "dense", "sparse", "images.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(IMAGES)))
        for k, (name, iid, (w, h), pos, f) in enumerate(IMAGES):
            q, t = look_at(np.array(pos, dtype=np.float64), CENTRE + rs.uniform(-0.15, 0.15, 3), 10.0 * k - 12.0)
            R = qvec2rotmat(q)
            cam = xyz @ R.T + t
            fx, fy, cx, cy = f * w, f * w * 1.03, w / 2 + 0.3, h / 2 + 0.2
            uv = np.stack([fx * cam[:, 0] / cam[:, 2] + cx, fy * cam[:, 1] / cam[:, 2] + cy], -1)
            front = cam[:, 2] > 0
            inside = front & (uv[:, 0] > 0.6) & (uv[:, 0] < w - 1.6) & (uv[:, 1] > 0.6) & (uv[:, 1] < h - 1.6)
            seen = np.flatnonzero(inside & (rs.rand(len(xyz)) < 0.3))
            kp = [(uv[j] + rs.normal(0, 0.3, 2), ids[j]) for j in seen]
            behind = np.flatnonzero(~front)[:5]  # behind the camera, yet registered at a pixel inside the image
            kp += [(np.array([rs.uniform(1, w - 2), rs.uniform(1, h - 2)]), ids[j]) for j in behind]
            kp += [(np.array([rs.uniform(0, w), rs.uniform(0, h)]), -1) for _ in range(6)]
            kp += [(np.array(p), ids[seen[n]]) for n, p in enumerate([(-3.2, 4.0), (w + 2.7, 5.1), (6.0, -1.4), (9.2, h + 0.7),
                                                                      (w - 0.4, 3.0), (-0.6, 2.0)])]  # the last two round out
            kp += [(np.array([10.5, 7.5]), ids[seen[7]]), (np.array([11.5, 8.5]), ids[seen[8]]), (np.array([12.5, 9.5]), ids[seen[9]])]
            order = rs.permutation(len(kp))
            kp = [kp[j] for j in order]
            first = [j for j, (_, pid) in enumerate(kp) if pid != -1 and 0 <= round(kp[j][0][0]) < w and 0 <= round(kp[j][0][1]) < h][:4]
            others = [pid for (_, pid) in kp if pid != -1]
            for n, j in enumerate(first):  # collisions: a LATER key-point of another 3-D point on the pixel of an earlier one
                kp.append((kp[j][0] + [0.1, -0.1], others[-(n + 3)]))
            fh.write(struct.pack("<i7di", iid, *q, *t, k + 1) + name.encode() + b"\x00" + struct.pack("<Q", len(kp)))
            for p, pid in kp:
                fh.write(struct.pack("<ddq", float(p[0]), float(p[1]), int(pid)))
            yy, xx = np.mgrid[0:h, 0:w]
            img = np.stack([255 * xx / (w - 1), 255 * yy / (h - 1), 127 + 100 * np.sin(0.7 * xx + 0.4 * yy + k)], -1) + rs.normal(0, 12, (h, w, 3))
            write_png(os.path.join(SCENE, "dense", "images", name), np.clip(img, 0, 255).astype(np.uint8))
            lab = (rs.randint(0, 6, size=((h + 5) // 6, (w + 6) // 7)).repeat(6, 0).repeat(7, 1)[:h, :w]).astype(np.uint8)
            np.savez_compressed(os.path.join(SCENE, "semantic_maps", name.split(".")[0] + ".npz"), lab)
    with open(os.path.join(SCENE, "cache_scene.tsv"), "w") as fh:
        fh.write("filename\tid\tsplit\tdataset\n" + "".join("%s\t%d\t%s\tsynthetic\n" % (n, i, s) for i, (n, s) in enumerate(TSV)))
    # the evaluation box is the SfM box CENTRE + (-1, -0.8, -0.7) .. (1, 0.8, 0.7) carried to the GT frame: scale 1 (hit octree) and
    # 1.5 (range octree), 2 scale / voxel_size = 20 / 30 -> level 4 for both, far from a power of two
    a = np.deg2rad(20.0)
    sfm2gt = np.eye(4)
    sfm2gt[:3, :3] = 1.7 * np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    sfm2gt[:3, 3] = [0.4, -0.1, 0.25]
    lo, hi = CENTRE + [-1.0, -0.8, -0.7], CENTRE + [1.0, 0.8, 0.7]
    bbx = [(sfm2gt[:3, :3] @ v + sfm2gt[:3, 3]).tolist() for v in (lo, hi)]
    import yaml

    with open(os.path.join(SCENE, "config.yaml"), "w") as fh:
        yaml.safe_dump({"name": "cache_scene", "origin": CENTRE.tolist(), "radius": 1.2, "eval_bbx": bbx, "voxel_size": VOXEL_SIZE,
                        "min_track_length": MIN_TRACK, "sfm2gt": sfm2gt.tolist()}, fh)


def nearest_resize(src, dsize, interpolation=None):
    """The rule csrc/ncw_cache.hip applies in place of cv2.resize(..., INTER_NEAREST)."""
    ws, hs = dsize
    h, w = src.shape[:2]
    r = np.minimum((np.arange(hs) * h) // hs, h - 1)
    c = np.minimum((np.arange(ws) * w) // ws, w - 1)
    return src[r][:, c]


def install_stubs():
    for name in ref_import._STUBS + ["kaolin.rep", "kaolin.rep.spc"]:
        sys.modules.setdefault(name, mock.MagicMock())
    ref_import._install_yacs()
    if "pytorch_lightning" not in sys.modules:
        pl = types.ModuleType("pytorch_lightning")
        pl.LightningModule, pl.LightningDataModule = torch.nn.Module, object
        sys.modules["pytorch_lightning"] = pl
    kornia = types.ModuleType("kornia")
    kornia.create_meshgrid = lambda h, w, normalized_coordinates=True, device=None: create_meshgrid(h, w, normalized_coordinates)
    kornia.losses = mock.MagicMock()
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tvt.ToTensor = ToTensor
    tv.transforms = tvt
    sys.modules.update({"kornia": kornia, "kornia.losses": kornia.losses, "torchvision": tv, "torchvision.transforms": tvt})


def make_dataset(pt, root, split, with_semantics):
    ds = pt.PhototourismDataset.__new__(pt.PhototourismDataset)
    ds.split_path, ds.root_dir, ds.split, ds.img_downscale, ds.val_num = "", root, split, 1, 1
    ds.define_transforms()
    ds.white_back, ds.semantic_map_path, ds.with_semantics = False, "semantic_maps", with_semantics
    ds.scene_origin = ds.scene_radius = None
    ds.depth_percent, ds.sfm_path = 0, "sparse"
    ds.use_cache, ds.octree_data, ds.use_voxel, ds.cache_paths, ds.shared_cache = False, None, False, ["cache"], False
    ds.read_meta()
    return ds


def cpu_octree(expand, radius):
    """voxel.octree_from_sfm's host half (the device half only sets bits): dense bool [G,G,G], origin f64, scale."""
    import yaml

    from neuralrecon_w_amd import voxel

    with open(os.path.join(SCENE, "config.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    pts = voxel.read_points3d_xyz(os.path.join(SCENE, "dense", "sparse", "points3D.bin"), cfg["min_track_length"])
    for _ in range(expand):
        pts = voxel.dilate_points(pts, cfg["voxel_size"])
    origin, scale = voxel.sfm_cube(cfg, radius)
    q, level = voxel.quantise_points(torch.from_numpy(pts), cfg["voxel_size"], origin, scale)
    G = 1 << level
    occ = torch.zeros(G, G, G, dtype=torch.bool)
    occ[q[:, 0], q[:, 1], q[:, 2]] = True
    return occ, torch.from_numpy(origin), scale, level


def main():
    write_scene()
    install_stubs()
    sys.path.insert(0, ref_import.REFERENCE_ROOT)
    try:
        pt = importlib.import_module("datasets.phototourism")
        pdc = importlib.import_module("tools.prepare_data.prepare_data_cache")
        cu = importlib.import_module("datasets.colmap_utils")
    finally:
        sys.path.remove(ref_import.REFERENCE_ROOT)
    pt.gen_octree_from_sfm = lambda *a, **k: (None, np.zeros(3), 1.0, 4)
    pt.cv2.resize, pt.cv2.INTER_NEAREST = nearest_resize, 0
    orig_depth = pt.PhototourismDataset.get_colmap_depth
    pt.PhototourismDataset.get_colmap_depth = lambda self, *a, **k: orig_depth(self, *a, **dict(k, device="cpu"))
    from neuralrecon_w_amd import cachebuild, views
    from oracle import neuconw_oracle as O

    rec = {}
    tmp = tempfile.mkdtemp()
    try:
        root = os.path.join(tmp, "cache_scene")
        shutil.copytree(SCENE, root)
        with mock.patch.object(torch.Tensor, "cuda", lambda self, *a, **k: self):
            sets = {(split, sem): make_dataset(pt, root, split, sem) for split in ("train", "eval") for sem in (True, False)}
        tr = sets[("train", True)]
        rec.update(ids=np.array(tr.img_ids), train_ids=np.array(tr.img_ids_train), test_ids=np.array(tr.img_ids_test),
                   names=np.array([tr.image_paths[i] for i in tr.img_ids]))
        assert list(rec["names"]) == ["a.jpg", "b.jpg", "c.jpg", "d.jpg"] and list(rec["test_ids"]) == [11], rec
        scene = views.read_scene(SCENE, "sparse")
        assert scene["ids"] == list(rec["ids"]) and scene["ids_train"] == list(rec["train_ids"])
        # the COLMAP tables through the reference's readers, held as phototourism.py:530-534 / :566-575 holds them
        imdata = cu.read_images_binary(os.path.join(SCENE, "dense", "sparse", "images.bin"))
        pts3d = cu.read_points3d_binary(os.path.join(SCENE, "dense", "sparse", "points3D.bin"))
        pts3d_array, error_array = torch.ones(max(pts3d.keys()) + 1, 4), torch.ones(max(pts3d.keys()) + 1, 1)
        for pid, p in pts3d.items():
            pts3d_array[pid, :3] = torch.from_numpy(p.xyz)
            error_array[pid, 0] = torch.from_numpy(p.error)
        xyz_t, err_t = pts3d_array[:, :3].numpy().copy(), error_array[:, 0].numpy().copy()
        points2d = {i: (im.xys, im.point3D_ids) for i, im in imdata.items()}
        n_coll = 0
        for iid in rec["ids"]:
            iid = int(iid)
            split = "eval" if iid in rec["test_ids"] else "train"
            ds13, ds12 = sets[(split, True)], sets[(split, False)]
            k = (ds13.img_ids_test if split == "eval" else ds13.img_ids_train).index(iid)
            rows13, rows12, rgbs = ds13.all_rays[k].numpy(), ds12.all_rays[k].numpy(), ds13.all_rgbs[k].numpy()
            assert rows13.shape[1] == 12 and rows12.shape[1] == 11  # the reference's widths (its comment says 13)
            K, w2c, c2w, w, h = views.image_pose(scene, iid, 1)
            img = views._decode_image(os.path.join(SCENE, "dense", "images", scene["images"][iid]["name"]), 1)
            assert img.shape == (h, w, 3) and rows13.shape[0] == h * w
            assert np.array_equal(K, ds13.Ks[iid]) and np.array_equal(c2w, ds13.poses_dict[iid])
            lab = cachebuild.load_label_map(SCENE, "semantic_maps", scene["images"][iid]["name"], w, h, 1)
            xys, p3d = points2d[iid]
            ok = p3d != -1
            xyz, err = xyz_t[p3d[ok]], err_t[p3d[ok]]
            px = torch.round(torch.from_numpy(xys)[ok] / 1).long().numpy()  # :575 + :185
            ins = (px[:, 0] >= 0) & (px[:, 0] < w) & (px[:, 1] >= 0) & (px[:, 1] < h)
            err_mean = float(np.mean(err[ins].astype(np.float64)))
            assert abs(float(torch.mean(torch.from_numpy(err[ins]))) - err_mean) < 1e-6 * err_mean  # the reference's float32 mean
            # the formula in float64, the LAST key-point winning
            z64 = xyz.astype(np.float64) @ w2c[2, :3] + w2c[2, 3]
            w64 = 2 * np.exp(-(err.astype(np.float64) / err_mean) ** 2)
            col, row = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
            norm = np.sqrt(((col - np.float64(K[0, 2])) / np.float64(K[0, 0])) ** 2 + ((row - np.float64(K[1, 2])) / np.float64(K[1, 1])) ** 2 + 1)
            d64, wt64, cnt = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w), dtype=int)
            for j in range(len(px)):
                c, r = px[j]
                if 0 <= c < w and 0 <= r < h:
                    d64[r, c], wt64[r, c] = z64[j] * norm[r, c], w64[j]
                    cnt[r, c] += 1
            ref_d, ref_w = rows13[:, 10].reshape(h, w).astype(np.float64), rows13[:, 11].reshape(h, w).astype(np.float64)
            assert np.array_equal(ref_w != 0, wt64 != 0) and np.array_equal(rows12[:, 9:11], rows13[:, 10:12])
            coll = cnt > 1
            n_coll += int(coll.sum())
            assert np.allclose(ref_d[coll], d64[coll], rtol=1e-5, atol=0) and np.allclose(ref_w[coll], wt64[coll], rtol=1e-5, atol=0), \
                "the reference's CPU run does not resolve a collision with the last key-point"
            assert (z64 < 0).any() and (p3d == -1).any() and ((px[:, 0] < 0) | (px[:, 0] >= w) | (px[:, 1] < 0) | (px[:, 1] >= h)).any()
            t = "im%d_" % iid
            rec.update({t + "rows13": rows13, t + "rows12": rows12, t + "rgbs": rgbs, t + "image": img, t + "label": lab,
                        t + "xys": xys, t + "point3d_ids": p3d, t + "kp_xyz": xyz, t + "kp_err": err, t + "kp_px": px,
                        t + "err_mean": np.float64(err_mean), t + "K": K, t + "c2w": c2w.astype(np.float32), t + "w2c": w2c,
                        t + "wh": np.array([w, h]), t + "near64": np.float64(ds13.nears[iid]), t + "far64": np.float64(ds13.fars[iid]),
                        t + "depth64": d64.reshape(-1), t + "weight64": wt64.reshape(-1), t + "collisions": coll.reshape(-1)})
        assert n_coll >= 12, n_coll  # at least three per image
        rec.update(xyz_table=xyz_t, err_table=err_t)
        # ---- the chunk writer on the training lists
        args = types.SimpleNamespace(split_to_chunks=N_CHUNKS, img_downscale=1, cache_type="npz")
        rays_l, rgbs_l = list(tr.all_rays), list(tr.all_rgbs)
        total = sum(r.shape[0] for r in rgbs_l)
        assert N_CHUNKS - total % N_CHUNKS == len(PADDING), total
        chunk_length = (total + len(PADDING)) // N_CHUNKS
        sp = os.path.join(tmp, "splits")
        os.makedirs(sp)
        pdc.split_to_chunks(list(rgbs_l), total, chunk_length, sp, args, np.array(PADDING), "rgbs")
        pdc.split_to_chunks(list(rays_l), total, chunk_length, sp, args, np.array(PADDING), "rays")
        assert sorted(os.listdir(sp)) == ["rays1_meta_info.json", "rgbs1_meta_info.json"] + ["split_%d" % i for i in range(N_CHUNKS)]
        for i in range(N_CHUNKS):
            for a in ("rays", "rgbs"):
                rec["chunk%d_%s" % (i, a)] = np.load(os.path.join(sp, "split_%d" % i, "%s1.npz" % a))["arr_0"]
        import json

        rec["chunk_meta"] = np.array(json.dumps(json.load(open(os.path.join(sp, "rays1_meta_info.json")))))
        rec.update(chunk_padding=np.array(PADDING), n_chunks=np.array(N_CHUNKS))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    # ---- the octree walk of the committed scene under the fp64 slab oracle: kept and dropped pixels in every view, grazing cap
    graze, n_rays = 0, 0
    for expand, radius in ((1, 1.0), (2, 1.5)):
        occ, origin, scale, level = cpu_octree(expand, radius)
        assert level == 4, level
        eps = 2e-3 * (2.0 / (1 << level))
        for iid in rec["ids"]:
            rows = torch.from_numpy(rec["im%d_rows12" % iid]).double()
            o, d = rows[:, 0:3], rows[:, 3:6]
            lo = O.ray_voxel_near_far(o, d, occ, origin, scale, margin=-eps)[0] > 0
            hi = O.ray_voxel_near_far(o, d, occ, origin, scale, margin=eps)[0] > 0
            graze += int((lo != hi).sum())
            n_rays += len(o)
            assert int(hi.sum()) > 50 and int((~lo).sum()) > 50, (expand, int(iid), int(hi.sum()), int((~lo).sum()))
    assert graze <= 0.01 * n_rays / 2, (graze, n_rays)  # 1 % of the PIXELS (n_rays counts every pixel once per octree)
    rec["grazing"] = np.array([graze, n_rays])
    out = os.path.join(HERE, "cache_golden.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes; collisions", n_coll, "grazing", graze, "of", n_rays)


if __name__ == "__main__":
    main()
