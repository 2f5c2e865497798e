"""Golden vectors for the camera-view path (neuralrecon_w_amd.views, csrc/ncw_view.hip), produced by RUNNING the reference's
own code on CPU:
  * datasets/ray_utils.py `get_ray_directions` + `get_rays` for a 7 x 5 view with an off-centre principal point and a
    non-trivial rotation (float32, as the dataset runs them);
  * metrics.py `mse` / `psnr` with and without a mask;
  * datasets/phototourism.py `PhototourismDataset` itself, splits 'val' (downscale clamped to 8) and 'test_train' (downscale 2,
    with and without a scene origin), on tests/golden/reproj_scene -- to which this script adds
      dense/sparse/points3D.bin : 240 seeded COLMAP points around the box, some behind the cameras;
      dense/images/d.jpg        : the first training image, 42 x 27 RGB, stored as PNG bytes (lossless, so the decoded pixels
                                  are the same everywhere; PIL reads by content -- the name is the one images.bin registers).
    The dataset hard-codes its COLMAP directory per scene name (phototourism.py:82-93), so the scene is copied to a temporary
    `brandenburg_gate/` with the model under `neuralsfm/`.
The seams (none of these libraries is installed): `kornia.create_meshgrid` is restated here (pixel-coordinate grid [1, H, W, 2],
x first); `torchvision.transforms.ToTensor` is uint8 HWC -> float CHW / 255; `kornia.losses`, `lpips`, open3d, cv2, h5py, kaolin
and the voxel tools are MagicMocks (never called on this path).
Records tests/golden/view_golden.npz.   Run:  python tests/golden/make_golden_view.py
"""
import importlib
import os
import shutil
import struct
import sys
import tempfile
import types
import zlib
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

SCENE = os.path.join(HERE, "reproj_scene")
IMAGE_NAME, IMAGE_WH = "d.jpg", (42, 27)  # int(2 cx) x int(2 cy) of camera 4 (make_golden_reproj.py: cx 21.3, cy 13.7)
SCENE_ORIGIN, SCENE_RADIUS = [0.1, -0.2, 0.3], 1.25


def write_points3d(path):
    rs = np.random.RandomState(11)
    xyz = np.concatenate([rs.uniform(-1.0, 1.0, size=(200, 3)) * [1.0, 1.0, 0.5] + [0, 0, 0.4],
                          rs.uniform(-6.0, 6.0, size=(40, 3))])  # the wide ones fall behind some cameras
    with open(path, "wb") as fh:
        fh.write(struct.pack("<Q", len(xyz)))
        for i, p in enumerate(xyz):
            track = 2 + i % 3
            fh.write(struct.pack("<QdddBBBd", i + 1, *p, *rs.randint(0, 256, 3).tolist(), 0.5 + 0.01 * i))
            fh.write(struct.pack("<Q", track) + b"".join(struct.pack("<ii", 1 + (i + t) % 4, t) for t in range(track)))
    return xyz


def write_png(path, rgb):
    h, w = rgb.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, 3 * w)], 1).tobytes()
    blk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)  # noqa: E731
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + blk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + blk(b"IDAT", zlib.compress(raw, 9))
                 + blk(b"IEND", b""))


def write_image(path):
    w, h = IMAGE_WH
    rs = np.random.RandomState(3)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([255 * xx / (w - 1), 255 * yy / (h - 1), 127 + 100 * np.sin(0.7 * xx + 0.4 * yy)], -1) + rs.normal(0, 12, (h, w, 3))
    write_png(path, np.clip(img, 0, 255).astype(np.uint8))


def create_meshgrid(height, width, normalized_coordinates=True, device=None):
    assert not normalized_coordinates
    xs, ys = torch.linspace(0, width - 1, width), torch.linspace(0, height - 1, height)
    return torch.stack(torch.meshgrid([xs, ys], indexing="ij"), -1).permute(1, 0, 2).unsqueeze(0)


class ToTensor:
    def __call__(self, img):
        return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255)


def install_stubs():
    for name in ref_import._STUBS + ["pytorch_lightning", "kaolin.rep", "kaolin.rep.spc"]:
        sys.modules.setdefault(name, mock.MagicMock())
    kornia = types.ModuleType("kornia")
    kornia.create_meshgrid = create_meshgrid
    kornia.losses = mock.MagicMock()
    tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tvt.ToTensor = ToTensor
    tv.transforms = tvt
    sys.modules.update({"kornia": kornia, "kornia.losses": kornia.losses, "torchvision": tv, "torchvision.transforms": tvt})


def rotmat(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def main():
    os.makedirs(os.path.join(SCENE, "dense", "images"), exist_ok=True)
    write_points3d(os.path.join(SCENE, "dense", "sparse", "points3D.bin"))
    write_image(os.path.join(SCENE, "dense", "images", IMAGE_NAME))
    install_stubs()
    sys.path.insert(0, ref_import.REFERENCE_ROOT)
    try:
        ru = importlib.import_module("datasets.ray_utils")
        met = importlib.import_module("metrics")
        pt = importlib.import_module("datasets.phototourism")
    finally:
        sys.path.remove(ref_import.REFERENCE_ROOT)
    rec = {}
    # ---- rays of a 7 x 5 view
    W, H = 7, 5
    K = np.array([[6.3, 0, 2.7], [0, 5.9, 3.1], [0, 0, 1]], dtype=np.float32)
    c2w = np.concatenate([rotmat((0.3, -1.0, 0.5), 37.0), np.array([[0.4], [-1.3], [2.2]])], 1).astype(np.float32)
    dirs = ru.get_ray_directions(H, W, K)
    o, d = ru.get_rays(dirs, torch.FloatTensor(c2w))
    rec.update(rays_K=K, rays_c2w=c2w, rays_wh=np.array([W, H]), rays_directions=dirs.numpy(), rays_o=o.numpy(), rays_d=d.numpy())
    # ---- psnr / mse
    g = torch.Generator().manual_seed(5)
    pred, gt = torch.rand(63, 3, generator=g), torch.rand(63, 3, generator=g)
    mask = (torch.rand(63, generator=g) < 0.6)[:, None].expand(63, 3)  # metrics.py indexes value[valid_mask]: same shape as value
    rec.update(met_pred=pred.numpy(), met_gt=gt.numpy(), met_mask=mask[:, 0].numpy(),
               met_mse=met.mse(pred, gt).numpy(), met_psnr=met.psnr(pred, gt).numpy(),
               met_mse_masked=met.mse(pred, gt, mask).numpy(), met_psnr_masked=met.psnr(pred, gt, mask).numpy())
    # ---- the dataset's items
    tmp = tempfile.mkdtemp()
    try:
        root = os.path.join(tmp, "brandenburg_gate")
        shutil.copytree(os.path.join(SCENE, "dense", "images"), os.path.join(root, "dense", "images"))
        shutil.copytree(os.path.join(SCENE, "dense", "sparse"), os.path.join(root, "neuralsfm"))
        shutil.copy(os.path.join(SCENE, "split.tsv"), os.path.join(root, "split.tsv"))
        cases = {"val": dict(split="val", img_downscale=1), "tt2": dict(split="test_train", img_downscale=2),
                 "tt1o": dict(split="test_train", img_downscale=1, scene_origin=np.array(SCENE_ORIGIN), scene_radius=SCENE_RADIUS)}
        for tag, kw in cases.items():
            ds = pt.PhototourismDataset(root, with_semantics=False, use_voxel=False, **kw)
            it = ds[0]
            rays = it["rays"].numpy()
            rec.update({"%s_id" % tag: np.array(int(it["ts"][0])), "%s_K" % tag: np.asarray(it["K"]), "%s_c2w" % tag: it["c2w"].numpy(),
                        "%s_wh" % tag: it["img_wh"].numpy(), "%s_near" % tag: rays[0, 6], "%s_far" % tag: rays[0, 7],
                        "%s_rays" % tag: rays, "%s_rgbs" % tag: it["rgbs"].numpy(), "%s_downscale" % tag: np.array(ds.img_downscale),
                        "%s_near64" % tag: np.float64(ds.nears[int(it["ts"][0])]), "%s_far64" % tag: np.float64(ds.fars[int(it["ts"][0])])})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rec.update(scene_origin=np.array(SCENE_ORIGIN), scene_radius=np.float64(SCENE_RADIUS))
    out = os.path.join(HERE, "view_golden.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes;", {k: rec[k].tolist() for k in ("val_id", "val_wh", "tt2_wh", "val_near", "val_far")})


if __name__ == "__main__":
    main()
