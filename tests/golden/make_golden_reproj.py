"""Golden vector for the reprojection visibility filter (neuralrecon_w_amd.reproj), produced by RUNNING the reference's own
utils/reproj_filter.py (its `get_train_ids`, `reprojection_worker`, `reproject`, `sfm2gt` and the `__main__` steps) with
tools/reproj_error.py's `get_entrinsics` / `get_intrinsic` and utils/colmap_utils.py's readers, on a small synthetic
workspace written here (tests/golden/reproj_scene/):
  dense/sparse/{cameras.bin, images.bin}: two PINHOLE cameras of different size with off-centre principal points, four
      registered images (three train, one test);
  split.tsv: train and test rows in an order unlike images.bin's, and one row without an id (whose image is not even
      registered: it must be skipped before the lookup);
  config.yaml: a similarity sfm2gt (rotation, scale 1.7, translation);
  mesh.ply: a coloured box on a ground grid (SfM frame), float32 vertices, faces wound with outward normals;
  depth.npz: per train view the depth map of tests/_raster_oracle.py (float64 rasterizer, stored as float32 as pyrender
      returns it) -- the reference's renderer stub returns these.
The seams (none of these libraries is installed): `ray.remote` is the identity decorator; open3d is a float64 brute-force
KD-tree / the arrays this script wrote / a recorder for write_point_cloud; `trimesh.load` returns the PLY's arrays; the
pyrender renderer returns the stored depth maps (and checks the pose it is given); pyrender, imageio, cv2,
pytorch_lightning and the reference's other imports are MagicMocks; sys.argv is set for the module-level parse_args.
Records reproj_golden.npz: the train ids in order, E, K, (w, h), E inv(sfm2gt), the reference's final rows [xyz, rgb].
Run:  python tests/golden/make_golden_reproj.py
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
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from tests import _raster_oracle as O  # noqa: E402

SCENE = os.path.join(HERE, "reproj_scene")
VOXEL = 0.05  # thr = 2 sqrt(2) 0.05 = 0.141 GT units; vertex spacing ~0.25 SfM units x 1.7


def rotmat(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def rotmat2qvec(R):
    """(w, x, y, z) of a rotation matrix (Shepperd's method, w >= 0)."""
    tr = np.trace(R)
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = np.array(q)
    return q if q[0] >= 0 else -q


def look_at(C, T, up=(0.0, 0.0, 1.0)):
    """World -> camera (OpenCV: x right, y down, z forward) of a camera at C looking at T."""
    z = np.asarray(T, dtype=np.float64) - C
    z /= np.linalg.norm(z)
    x = np.cross(-np.asarray(up, dtype=np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ np.asarray(C, dtype=np.float64)


def box_on_ground(n_ground=8, half=1.0, box=(0.3, 0.6), n_box=2):
    """Ground grid z = 0 over [-half, half]^2 (normals +z) + a box [-b, b]^2 x [0, h] (outward normals, the bottom face
    included: it is never seen)."""
    verts, faces = [], []

    def quad_grid(origin, u, v, n):
        base = len(verts)
        for i in range(n + 1):
            for j in range(n + 1):
                verts.append(origin + u * (i / n) + v * (j / n))
        for i in range(n):
            for j in range(n):
                a, b, c, d = base + i * (n + 1) + j, base + (i + 1) * (n + 1) + j, base + (i + 1) * (n + 1) + j + 1, base + i * (n + 1) + j + 1
                faces.append((a, b, c))  # normal = u x v
                faces.append((a, c, d))

    e = np.eye(3)
    quad_grid(np.array([-half, -half, 0.0]), 2 * half * e[0], 2 * half * e[1], n_ground)
    b, h = box
    lo = np.array([-b, -b, 0.0])
    quad_grid(lo + np.array([0, 0, h]), 2 * b * e[0], 2 * b * e[1], n_box)          # top, +z
    quad_grid(lo, 2 * b * e[1], 2 * b * e[0], n_box)                                # bottom, -z
    quad_grid(lo, 2 * b * e[0], h * e[2], n_box)                                    # y = -b, normal -y
    quad_grid(lo + np.array([0, 2 * b, 0]), h * e[2], 2 * b * e[0], n_box)         # y = +b, normal +y
    quad_grid(lo, h * e[2], 2 * b * e[1], n_box)                                    # x = -b, normal -x
    quad_grid(lo + np.array([2 * b, 0, 0]), 2 * b * e[1], h * e[2], n_box)         # x = +b, normal +x
    return np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int64)


def write_ply(path, v, f, rgb):
    hdr = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v), "property float x", "property float y",
           "property float z", "property uchar red", "property uchar green", "property uchar blue",
           "element face %d" % len(f), "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(len(v), dtype=[("p", "<f4", 3), ("c", "u1", 3)])
    rec["p"], rec["c"] = v, rgb
    fr = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", 3)])
    fr["n"], fr["i"] = 3, f
    with open(path, "wb") as fh:
        fh.write(("\n".join(hdr) + "\n").encode())
        fh.write(rec.tobytes())
        fh.write(fr.tobytes())


CAMERAS = {4: (40, 30, [38.0, 41.5, 21.3, 13.7]), 9: (32, 36, [30.5, 29.0, 15.1, 18.9])}
# image id -> (name, camera id, centre, target)
IMAGES = {3: ("a.jpg", 4, (-1.5, -1.7, 1.4), (0.1, 0.0, 0.2)), 1: ("b.jpg", 9, (0.3, 2.0, 1.8), (0.0, 0.1, 0.1)),
          7: ("c.jpg", 4, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0)), 2: ("d.jpg", 4, (1.8, -1.2, 1.6), (0.0, 0.0, 0.2))}
TSV = [("d.jpg", "12", "train"), ("a.jpg", "5", "train"), ("c.jpg", "6", "test"), ("e.jpg", "", "train"), ("b.jpg", "3", "train")]


def sfm2gt():
    T = np.eye(4)
    T[:3, :3] = rotmat((1.0, 2.0, 3.0), 25.0) * 1.7
    T[:3, 3] = [0.4, -0.1, 0.25]
    return T


def write_scene():
    sp = os.path.join(SCENE, "dense", "sparse")
    os.makedirs(sp, exist_ok=True)
    with open(os.path.join(sp, "cameras.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(CAMERAS)))
        for cid, (w, h, p) in CAMERAS.items():
            fh.write(struct.pack("<iiQQ", cid, 1, w, h) + struct.pack("<4d", *p))
    Es = {}
    with open(os.path.join(sp, "images.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(IMAGES)))
        for iid, (name, cid, C, T) in IMAGES.items():
            R, t = look_at(np.array(C), T)
            q = rotmat2qvec(R)
            fh.write(struct.pack("<i7di", iid, *q, *t, cid) + name.encode() + b"\x00")
            fh.write(struct.pack("<Q", 2) + struct.pack("<ddq", 1.5, 2.5, -1) + struct.pack("<ddq", 3.5, 4.5, 17))
            Es[iid] = (q, t)
    with open(os.path.join(SCENE, "split.tsv"), "w") as fh:
        fh.write("filename\tid\tsplit\tdataset\n")
        for name, i, s in TSV:
            fh.write("%s\t%s\t%s\tsynthetic\n" % (name, i, s))
    with open(os.path.join(SCENE, "config.yaml"), "w") as fh:
        yaml.safe_dump({"sfm2gt": sfm2gt().tolist()}, fh)
    v, f = box_on_ground()
    rgb = np.random.RandomState(5).randint(0, 256, size=(len(v), 3)).astype(np.uint8)
    write_ply(os.path.join(SCENE, "mesh.ply"), v, f, rgb)
    return v, f, rgb, Es


def qvec2rotmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def main():
    v, f, rgb, Es = write_scene()
    train = [iid for name, i, s in TSV if i and s == "train" for iid, im in IMAGES.items() if im[0] == name]
    depths = {}
    for iid in train:
        name, cid, _, _ = IMAGES[iid]
        w, h, p = CAMERAS[cid]
        q, t = Es[iid]
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = qvec2rotmat(q), t
        K = np.array([[p[0], 0, p[2]], [0, p[1], p[3]], [0, 0, 1]], dtype=np.float32)
        depths[iid] = O.rasterize(v, f, K, E, h, w)["depth"].astype(np.float32)
    np.savez_compressed(os.path.join(SCENE, "depth.npz"), **{"view_%d" % k: d for k, d in depths.items()})

    # ---- the reference, with its seams stubbed
    mesh_path = os.path.join(SCENE, "mesh.ply")
    out_dir = tempfile.mkdtemp()
    captured = {}

    class PointCloud:
        def __init__(self):
            self.points = np.zeros((0, 3))
            self.colors = np.zeros((0, 3))

    def read_point_cloud(path):
        assert os.path.abspath(path) == mesh_path, path
        pc = PointCloud()
        pc.points = v.astype(np.float64)
        pc.colors = rgb.astype(np.float64) / 255.0
        return pc

    class KDTreeFlann:
        def __init__(self, pcd):
            self.p = np.asarray(pcd.points, dtype=np.float64)

        def search_knn_vector_3d(self, q, k):
            d2 = ((self.p - np.asarray(q, dtype=np.float64)) ** 2).sum(-1)
            i = int(np.argmin(d2))
            return 1, [i], [float(d2[i])]

    def write_point_cloud(path, pcd):
        captured["rows"] = np.concatenate([np.asarray(pcd.points), np.asarray(pcd.colors)], 1)

    o3d = types.ModuleType("open3d")
    o3d.io = types.SimpleNamespace(read_point_cloud=read_point_cloud, write_point_cloud=write_point_cloud)
    o3d.geometry = types.SimpleNamespace(KDTreeFlann=KDTreeFlann, PointCloud=PointCloud)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda x: np.asarray(x, dtype=np.float64))
    trimesh = types.ModuleType("trimesh")
    trimesh.load = lambda path, process=True: types.SimpleNamespace(vertices=v.astype(np.float64), faces=f.copy())
    ray = types.ModuleType("ray")
    ray.remote = lambda *a, **k: (lambda fn: fn)
    for name in ref_import._STUBS + ["pytorch_lightning", "pyrender", "imageio", "cv2"]:
        sys.modules.setdefault(name, mock.MagicMock())
    sys.modules["open3d"], sys.modules["trimesh"], sys.modules["ray"] = o3d, trimesh, ray
    sys.argv = ["reproj_filter.py", "--src_file", mesh_path, "--target_file", mesh_path, "--data_path", SCENE,
                "--output_path", out_dir, "--voxel_size", str(VOXEL)]
    sys.path.insert(0, ref_import.REFERENCE_ROOT)
    try:
        rf = importlib.import_module("utils.reproj_filter")
        cu = importlib.import_module("utils.colmap_utils")
        re_ = importlib.import_module("tools.reproj_error")
    finally:
        sys.path.remove(ref_import.REFERENCE_ROOT)

    poses = []

    class Renderer:
        def __init__(self, mesh, height=480, width=640):
            self.n = 0

        def __call__(self, height, width, intrinsics, pose):
            iid = ids[self.n]
            self.n += 1
            poses.append(np.array(pose))
            d = depths[iid]
            assert d.shape == (height, width)
            return np.zeros((height, width, 3), np.uint8), d

    rf.pyrender_renderer = Renderer
    # utils/reproj_filter.py `__main__` (:255-291) with one worker
    imdata = cu.read_images_binary(os.path.join(SCENE, "dense/sparse", "images.bin"))
    camdata = cu.read_cameras_binary(os.path.join(SCENE, "dense/sparse", "cameras.bin"))
    img_ids_all, img_id_to_name, img_path_to_id = rf.get_image_id(imdata, SCENE)
    ids = rf.get_train_ids(SCENE, img_ids_all, img_path_to_id)
    assert list(ids) == train, (ids, train)
    ext = re_.get_entrinsics(imdata, ids)
    ext_d = {id_: ext[i] for i, id_ in enumerate(ids)}
    K_d, wh_d = re_.get_intrinsic(camdata, ids, imdata)
    E_list = [ext_d[k] for k in ids]
    points_all = rf.reprojection_worker([K_d[k] for k in ids], E_list, [wh_d[k] for k in ids], [img_id_to_name[k] for k in ids])
    pc_colored = np.unique(np.vstack([np.zeros((0, 6)), points_all]), axis=0)
    rf.o3d.io.write_point_cloud(os.path.join(out_dir, "reprojected.ply"), types.SimpleNamespace(points=pc_colored[:, :3],
                                                                                                colors=pc_colored[:, 3:]))
    shutil.rmtree(out_dir, ignore_errors=True)
    S = sfm2gt()
    E_gt = np.stack([E @ np.linalg.inv(S) for E in E_list])
    assert np.allclose(np.stack(poses), np.linalg.inv(E_gt), rtol=0, atol=1e-12)
    rows = captured["rows"]
    out = os.path.join(HERE, "reproj_golden.npz")
    np.savez_compressed(out, train_ids=np.array(ids), names=np.array([img_id_to_name[k] for k in ids]), E=np.stack(E_list),
                        K=np.stack([K_d[k] for k in ids]), wh=np.array([wh_d[k] for k in ids]), E_gt=E_gt, sfm2gt=S, rows=rows,
                        voxel_size=np.float64(VOXEL))
    print("wrote", out, "rows", rows.shape, "of", len(v), "vertices;", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
