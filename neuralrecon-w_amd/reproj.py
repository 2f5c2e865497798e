"""Reprojection visibility filter on the GPU: the first step of the reference's evaluation pipeline
(scripts/eval_pipeline.sh), which keeps only the mesh vertices some training camera sees before the F-score is taken.

Reference: utils/reproj_filter.py (`get_train_ids` :70-83, `sfm2gt` :85-92, `load_mesh_to_render` :101-130, `reproject`
:133-152, `reprojection_worker` :172-243, `__main__` :254-300), utils/pyrender_renderer.py and tools/reproj_error.py:68-91
(`get_entrinsics`, `get_intrinsic`).  The reference renders every training view with pyrender (OpenGL / EGL), back-projects
every valid pixel and runs one open3d KD-tree query per pixel in a Python loop; here:
  * depth: the triangle rasterizer of csrc/ncw_raster.hip (`render_depth`), pyrender's conventions;
  * back-projection and marking: ncw_raster_backproject / ncw_raster_mark, nearest neighbours by evalmesh.NNGrid (exact,
    ties to the smaller index);
  * COLMAP cameras.bin / images.bin, the tsv split and PLY files read by colmap.py / ply.py (no pandas, no open3d, no trimesh);
    PINHOLE cameras only;
  * one process, one GPU: the views are independent and run one after another;
  * a source WITHOUT faces (a point cloud: utils/reproj_filter.py:110-115, utils/kaolin_renderer.py) is voxelised over the
    evaluation box (`VoxelCloud`) and every view is traced to the first occupied voxel by csrc/ncw_voxview.hip.
"""
import ctypes as C
import os

import numpy as np
import torch
import yaml

from . import colmap, evalmesh, meshops, ply
from . import lib as L
# The names the test suites of the earlier commits call (tests/test_reproj_host.py, tests/test_gpu_reproj*.py, tests/test_gpu_surf.py):
# bindings only -- the functions live in colmap.py / ply.py, and the package's own code calls them there.
from .colmap import qvec2rotmat, read_cameras as read_cameras_binary, read_images as read_images_binary  # noqa: F401
from .ply import read_mesh as read_ply_mesh  # noqa: F401

ZNEAR, ZFAR = 0.05, 100.0  # pyrender.IntrinsicsCamera's defaults (in the units of the rendered frame)
SMALL_MAX = 32  # sub-triangles whose pixel box holds more samples go to the workgroup-per-triangle kernel
CULL = {"back": 1, "none": 0}

# what pandas.read_csv reads as a missing value (its default na_values): such an `id` is null
_NA = {"", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>", "N/A", "NA", "NULL",
       "NaN", "None", "n/a", "nan", "null"}


# ---------------------------------------------------------------------------------------------------
# COLMAP model and the train split
# ---------------------------------------------------------------------------------------------------
def read_train_split(data_path, images):
    """utils/reproj_filter.py:70-83 `get_train_ids`: the rows of the first <data_path>/*.tsv (sorted by name) with a non-null
    `id` and split == 'train', in file order, as COLMAP image ids (through the image names).  A filename of a row with an
    id that is not in images.bin is an error, as in the reference."""
    tsv, rows = colmap.split_rows(data_path)
    by_name = {im["name"]: iid for iid, im in images.items()}
    ids = []
    for row in rows:
        if (row.get("id") or "").strip() in _NA:
            continue
        name = row["filename"]
        if name not in by_name:
            raise KeyError("%s: image %r is not in images.bin" % (tsv, name))
        if row.get("split") == "train":
            ids.append(by_name[name])
    return ids


def load_views(data_path, sfm2gt=None):
    """The training views of <data_path>: list of dict(id, name, E 4x4 world -> camera (SfM frame, float64), K 3x3 (float32
    values, as tools/reproj_error.py:84-88 builds it), wh (width, height), E_gt = E inv(sfm2gt) (utils/reproj_filter.py:175),
    pose = inv(E_gt))."""
    sp = os.path.join(data_path, "dense", "sparse")
    images = colmap.read_images(os.path.join(sp, "images.bin"))
    cams = colmap.read_cameras(os.path.join(sp, "cameras.bin"))
    S = np.eye(4) if sfm2gt is None else np.asarray(sfm2gt, dtype=np.float64)
    S_inv = np.linalg.inv(S)
    views = []
    for iid in read_train_split(data_path, images):
        im = images[iid]
        cam = cams[im["camera_id"]]
        E = np.eye(4)
        E[:3, :3] = colmap.qvec2rotmat(im["qvec"])
        E[:3, 3] = im["tvec"]
        p = cam["params"]
        K = np.array([[p[0], 0, p[2]], [0, p[1], p[3]], [0, 0, 1]], dtype=np.float32)
        E_gt = E @ S_inv
        views.append({"id": iid, "name": im["name"], "E": E, "K": K, "wh": (cam["width"], cam["height"]), "E_gt": E_gt,
                      "pose": np.linalg.inv(E_gt)})
    return views


def read_sfm2gt(data_path):
    with open(os.path.join(data_path, "config.yaml")) as fh:
        return np.array(yaml.safe_load(fh)["sfm2gt"], dtype=np.float64)


def write_ply_points(path, xyz, rgb=None):
    """ply.write's point-cloud form (double coordinates, optional uchar colours, no face element) under the name the earlier
    test suites call; the package itself calls ply.write."""
    ply.write(path, xyz, rgb=rgb)


# ---------------------------------------------------------------------------------------------------
# the rasterizer (csrc/ncw_raster.hip)
# ---------------------------------------------------------------------------------------------------
class RasterMesh:
    """A triangle mesh on the device, ready for `render`: vertices recentred in float64 and cast to f32 (the view's
    translation absorbs the centre), faces int32, and the large-triangle list (2 entries per face: a face clipped by the
    near plane has two sub-triangles)."""

    def __init__(self, verts, faces, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise L.NeuconwHipError("reproj.RasterMesh: the rasterizer runs on a GPU only; there is no CPU fallback")
        v = torch.as_tensor(np.asarray(verts.detach().cpu() if torch.is_tensor(verts) else verts, dtype=np.float64)).reshape(-1, 3)
        f = torch.as_tensor(np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces, dtype=np.int64)).reshape(-1, 3)
        if f.shape[0] >= (1 << 30):
            raise ValueError("reproj.RasterMesh: at most 2^30 - 1 faces")
        self.centre = ((v.amin(0) + v.amax(0)) / 2).numpy() if v.shape[0] else np.zeros(3)
        self.dev = dev
        self.nv, self.nf = int(v.shape[0]), int(f.shape[0])
        self.verts = (v - torch.from_numpy(self.centre)).float().contiguous().to(dev)
        self.faces = f.to(torch.int32).contiguous().to(dev)
        self.large = torch.empty(max(1, 2 * self.nf), dtype=torch.int32, device=dev)
        self.n_large = torch.zeros(1, dtype=torch.int32, device=dev)

    def view_struct(self, K, view, height, width, znear=ZNEAR, zfar=ZFAR, cull="back", small_max=SMALL_MAX):
        """NcwRasterView of a 3x4 / 4x4 world -> camera matrix `view` (float64, applied to the mesh's own frame): the centre
        moves into the translation in float64, then everything is rounded to f32."""
        if cull not in CULL:
            raise ValueError("cull must be 'back' or 'none' (got %r)" % (cull,))
        V = np.asarray(view, dtype=np.float64)[:3, :4].copy()
        V[:, 3] = V[:, :3] @ self.centre + V[:, 3]
        K = np.asarray(K, dtype=np.float64)
        s = L.NcwRasterView()
        for i, x in enumerate(V.reshape(-1)):
            s.view[i] = float(x)
        s.fx, s.fy, s.cx, s.cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
        s.znear, s.zfar = float(znear), float(zfar)
        s.height, s.width = int(height), int(width)
        s.cull = CULL[cull]
        s.small_max = int(small_max)
        return s

    def rasterize(self, s, zbuf, timer=None):
        """The z-buffer of one view into zbuf (int64 [H*W], overwritten).  timer: optional callable(stage) bracketing the
        two raster kernels (scripts/bench_reproj.py)."""
        lib = L.get_lib()
        st = L.stream_ptr(self.dev)
        zbuf.fill_(-1)  # all ones = empty
        self.n_large.zero_()
        if self.nf == 0:
            return
        if timer:
            timer("small")
        L.check(lib.ncw_raster_small(L.ptr(self.verts), self.nv, L.ptr(self.faces), self.nf, C.byref(s), L.ptr(zbuf),
                                     L.ptr(self.large), L.ptr(self.n_large), st), "ncw_raster_small")
        if timer:
            timer("large")
        L.check(lib.ncw_raster_large(L.ptr(self.verts), self.nv, L.ptr(self.faces), C.byref(s), L.ptr(self.large),
                                     L.ptr(self.n_large), int(self.large.shape[0]), L.ptr(zbuf), st), "ncw_raster_large")
        if timer:
            timer("end")


def resolve(zbuf, height, width, with_face=True):
    """(depth [H,W] f32, 0 = empty; face [H,W] int32, -1 = empty, or None) of a z-buffer."""
    lib = L.get_lib()
    n = int(height) * int(width)
    depth = torch.empty(n, dtype=torch.float32, device=zbuf.device)
    face = torch.empty(n, dtype=torch.int32, device=zbuf.device) if with_face else None
    L.check(lib.ncw_raster_resolve(L.ptr(zbuf), n, L.ptr(depth), L.ptr(face), L.stream_ptr(zbuf.device)), "ncw_raster_resolve")
    return depth.view(height, width), (face.view(height, width) if with_face else None)


@torch.no_grad()
def render_depth(verts, faces, K, view, height, width, znear=ZNEAR, zfar=ZFAR, cull="back", device=None, small_max=SMALL_MAX,
                 stats=None):
    """Linear eye-space depth of the mesh (verts [V,3], faces [F,3]; numpy or torch) seen by the pinhole camera K (3x3:
    fx, fy, cx, cy) at world -> camera `view` (3x4 or 4x4, OpenCV axes), as pyrender renders it for
    utils/pyrender_renderer.py: pixel (r, c) samples the image point (c + 0.5, r + 0.5), near-plane clipping, samples beyond
    zfar dropped, back faces culled (cull='back') or not ('none').  Returns (depth [H,W] f32, 0 where nothing is hit;
    face [H,W] int32, -1 there) on the device.  stats (dict): `large` = sub-triangles that took the workgroup path."""
    m = RasterMesh(verts, faces, device)
    s = m.view_struct(K, view, height, width, znear, zfar, cull, small_max)
    zbuf = torch.empty(int(height) * int(width), dtype=torch.int64, device=m.dev)
    m.rasterize(s, zbuf)
    if stats is not None:
        stats["large"] = int(m.n_large.item())
    return resolve(zbuf, int(height), int(width))


def backproject(depth, M):
    """Points [N,3] f32 of the pixels with depth > 0, in pixel order: M[:, :3] (c d, r d, d) + M[:, 3] (M 3x4 on the host,
    rounded to f32), and their linear pixel indices [N] int64."""
    lib = L.get_lib()
    h, w = depth.shape
    flat = depth.reshape(-1).contiguous()
    pix = torch.nonzero(flat > 0).reshape(-1).contiguous()  # pixel order; one device -> host read (the count)
    n = int(pix.shape[0])
    pts = torch.empty(n, 3, dtype=torch.float32, device=depth.device)
    Mf = (C.c_float * 12)(*[float(x) for x in np.asarray(M, dtype=np.float64)[:3, :4].reshape(-1)])
    L.check(lib.ncw_raster_backproject(L.ptr(flat), L.ptr(pix), n, int(w), Mf, L.ptr(pts), L.stream_ptr(depth.device)),
            "ncw_raster_backproject")
    return pts, pix


def backproject_matrix(K, pose, centre=None):
    """3x4 float64 M with M[:, :3] (c d, r d, d) + M[:, 3] = pose[:3] [K^-1 (c, r, 1) d; 1] - centre
    (utils/reproj_filter.py:133-152)."""
    pose = np.asarray(pose, dtype=np.float64)
    M = np.zeros((3, 4))
    M[:, :3] = pose[:3, :3] @ np.linalg.inv(np.asarray(K, dtype=np.float64))
    M[:, 3] = pose[:3, 3] - (0.0 if centre is None else np.asarray(centre, dtype=np.float64))
    return M


# ---------------------------------------------------------------------------------------------------
# the filter (utils/reproj_filter.py)
# ---------------------------------------------------------------------------------------------------
class Target:
    """The cloud to filter (utils/reproj_filter.py:177-189): every vertex of target_file (no welding) in GT coordinates,
    its colours (zeros without), and one NNGrid over it (recentred on its box centre in float64, as nn_distances does).
    bounded (default True): `mark` asks for the nearest vertex WITHIN the threshold only (NNGrid.query_within: one launch, no
    brute-force pass for back-projected points that have no vertex nearby); the flags are the same either way, bounded=False is
    the earlier path, kept for the comparison."""

    def __init__(self, xyz, rgb, thr, device, bounded=True):
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.rgb = np.zeros(self.xyz.shape, dtype=np.uint8) if rgb is None else np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
        self.m = self.xyz.shape[0]
        self.dev = device
        self.thr = float(thr)
        self.bounded = bool(bounded)
        self.flags = torch.zeros(max(1, self.m), dtype=torch.uint8, device=device)
        self.centre = (self.xyz.min(0) + self.xyz.max(0)) / 2 if self.m else np.zeros(3)
        self.grid = None
        if self.m:
            r32 = torch.from_numpy(self.xyz - self.centre).float().to(device).contiguous()
            # queries further than thr outside the cloud's box can mark nothing: the stop test's rounding margin needs to
            # cover the coordinates of the cloud and of the queries that can
            cmax = float(r32.abs().max()) + self.thr
            self.grid = evalmesh.NNGrid(r32, cmax)

    def mark(self, pts32):
        """Marks the nearest target vertex of every query closer than thr (queries: recentred f32 [N,3])."""
        n = int(pts32.shape[0])
        if n == 0 or self.grid is None:
            return
        if self.bounded:
            # ncw_raster_mark marks where sqrtf(d2) < thr (float32), which implies d2 < thr^2 (1 + eps)^2; the float32 square of
            # thr (1 + 4 eps) is, after its two roundings, still >= thr^2 (1 + 5 eps): every vertex it marks is within the bound
            dist, idx = self.grid.query_within(pts32, float(np.float32(self.thr)) * (1.0 + 4.0 * evalmesh.F32_EPS))
        else:
            dist, idx = self.grid.query(pts32)
        L.check(L.get_lib().ncw_raster_mark(L.ptr(dist), L.ptr(idx), n, self.thr, self.m, L.ptr(self.flags),
                                            L.stream_ptr(self.dev)), "ncw_raster_mark")

    def rows(self):
        """np.unique over the rows [xyz, rgb] of the marked vertices (lexicographic): (xyz float64, rgb uint8)."""
        return unique_rows(self.xyz, self.rgb, self.flags[: self.m], self.dev)


def unique_rows(xyz, rgb, flags, device):
    """np.unique over the rows [xyz, rgb] of the vertices whose flag is set (lexicographic): (xyz float64, rgb uint8)."""
    keep = torch.nonzero(flags).reshape(-1).cpu().numpy()
    if keep.shape[0] == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.uint8)
    rows = np.concatenate([xyz[keep], rgb[keep].astype(np.float64)], 1)
    u = torch.unique(torch.from_numpy(rows).to(device), dim=0).cpu().numpy()  # sorted rows, as np.unique(axis=0)
    return u[:, :3].copy(), u[:, 3:].astype(np.uint8)


# ---------------------------------------------------------------------------------------------------
# the point-cloud source (utils/kaolin_renderer.py; csrc/ncw_voxview.hip)
# ---------------------------------------------------------------------------------------------------
def cloud_cube(scene_config, voxel_size):
    """generate_voxel.py:104-118, 146 for gen_octree(..., expand=0, radius=1, in_sfm=False): the evaluation box `eval_bbx` AS
    GIVEN (GT frame; its two corners are not sorted, as in the reference), origin = its centre, scale = longest edge / 2,
    level = floor(log2(2 scale / voxel_size)).  Returns (origin float64 [3], scale, level).  ValueError for a config without
    eval_bbx or a level outside the 3..10 of the bit grids."""
    if not isinstance(scene_config, dict) or scene_config.get("eval_bbx") is None:
        raise ValueError("the scene's config.yaml has no eval_bbx: a point-cloud source is voxelised over the evaluation box")
    lo = np.array(scene_config["eval_bbx"][0], dtype=np.float64)
    hi = np.array(scene_config["eval_bbx"][1], dtype=np.float64)
    origin = lo + (hi - lo) / 2
    scale = float(np.max(hi - lo) / 2)
    if not (scale > 0 and float(voxel_size) > 0):
        raise ValueError("eval_bbx %r / voxel_size %r span no volume" % (scene_config["eval_bbx"], voxel_size))
    level = int(np.floor(np.log2(2 * scale / float(voxel_size))))
    if level > 10:
        raise ValueError("voxel_size %g gives octree level %d over this evaluation box (longest edge %g); the bit grid goes up to "
                         "level 10: the smallest voxel_size that fits is above %.9g" % (voxel_size, level, 2 * scale, 2 * scale / 2048))
    if level < 3:
        raise ValueError("voxel_size %g gives octree level %d over this evaluation box (longest edge %g); the bit grid starts at "
                         "level 3: the largest voxel_size that fits is %.9g" % (voxel_size, level, 2 * scale, 2 * scale / 8))
    return origin, scale, level


class VoxelCloud:
    """utils/kaolin_renderer.py's renderer for a point-cloud source: gen_octree(data_path, points, voxel_size, expand=0,
    in_sfm=False) (generate_voxel.py:75-150) as a bit-packed occupancy over the evaluation box (`cloud_cube`), and a `seen`
    grid of the same layout that the views accumulate their first-hit voxels into.  points_gt: [N,3] in the frame of
    eval_bbx (GT), normalised in float64 and then cast to f32; the occupied voxels are those ncw_voxel_build finds a point
    in (a point outside the cube, or on its upper faces, has none)."""

    def __init__(self, points_gt, scene_config, voxel_size, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise L.NeuconwHipError("reproj.VoxelCloud: the voxel views run on a GPU only; there is no CPU fallback")
        if dev.index is None:  # 'cuda' -> the current device, so that tensors' devices compare equal to it
            dev = torch.device("cuda", torch.cuda.current_device())
        self.origin, self.scale, self.level = cloud_cube(scene_config, voxel_size)
        self.dev = dev
        self.voxel_size = float(voxel_size)
        G = self.G = 1 << self.level
        self.occ = torch.zeros(G * G * G // 32, dtype=torch.int32, device=dev)
        self.brick = torch.zeros((max(G // 8, 1) ** 3 + 31) // 32, dtype=torch.int32, device=dev)
        self.seen = torch.zeros_like(self.occ)
        pn = self.normalise(points_gt)
        L.check(L.get_lib().ncw_voxel_build(L.ptr(pn), int(pn.shape[0]), self.level, L.ptr(self.occ), L.ptr(self.brick),
                                            L.stream_ptr(dev)), "ncw_voxel_build")
        g = self.grid = L.NcwCacheOctree()
        for a in range(3):
            g.origin[a] = float(self.origin[a])
        g.scale, g.level = self.scale, self.level
        g.occ, g.brick = self.occ.data_ptr(), self.brick.data_ptr()

    def normalise(self, points_gt):
        """f32 [N,3] on the device: (points - origin) / scale in float64, then cast."""
        p = points_gt.detach().cpu().numpy() if torch.is_tensor(points_gt) else points_gt
        p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
        return torch.from_numpy(((p - self.origin) / self.scale).astype(np.float32)).to(self.dev).contiguous()

    def view_struct(self, K, pose, height, width):
        """NcwVoxelView of the camera K (3x3) at camera -> world `pose` (3x4 / 4x4, GT frame, scale included): the camera
        centre is normalised to the cube in float64 (generate_voxel.py:333, :345), then everything is rounded to f32."""
        K = np.asarray(K, dtype=np.float64)
        P = np.asarray(pose, dtype=np.float64)[:3, :4]
        s = L.NcwVoxelView()
        s.fx, s.fy, s.cx, s.cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
        for i, x in enumerate(P[:, :3].reshape(-1)):
            s.pose[i] = float(x)
        for i, x in enumerate((P[:, 3] + 1e-7 - self.origin) / self.scale):
            s.o_norm[i] = float(x)
        s.width, s.height = int(width), int(height)
        return s

    def trace(self, K, pose, height, width, depth=None, voxel=None):
        """One view, one launch, no host synchronisation: every pixel's first occupied voxel is marked in `seen`.  depth
        (f32) / voxel (int32): optional contiguous device tensors of height * width elements that receive the planes."""
        n = int(height) * int(width)
        for t, dt in ((depth, torch.float32), (voxel, torch.int32)):
            if t is not None and (t.dtype != dt or t.numel() != n or t.device != self.dev or not t.is_contiguous()):
                raise ValueError("reproj.VoxelCloud.trace: planes are contiguous %d-element f32 (depth) / int32 (voxel) tensors on %s" % (n, self.dev))
        s = self.view_struct(K, pose, height, width)
        L.check(L.get_lib().ncw_voxel_view_seen(C.byref(s), C.byref(self.grid), 0, n, L.ptr(self.seen), L.ptr(depth), L.ptr(voxel),
                                                L.stream_ptr(self.dev)), "ncw_voxel_view_seen")

    def select(self, points_gt):
        """bool [N] on the device: point i lies in a voxel of THIS grid that some traced pixel hit first."""
        pn = self.normalise(points_gt)
        n = int(pn.shape[0])
        flags = torch.zeros(n, dtype=torch.uint8, device=self.dev)
        if n == 0:
            return flags.bool()
        L.check(L.get_lib().ncw_voxel_points_seen(L.ptr(pn), n, self.level, L.ptr(self.seen), L.ptr(flags), L.stream_ptr(self.dev)),
                "ncw_voxel_points_seen")
        return flags.bool()

    def clear(self):
        self.seen.zero_()


@torch.no_grad()
def render_cloud_depth(points, scene_config, voxel_size, K, pose, height, width, device=None):
    """The counterpart of `render_depth` for a point cloud (utils/kaolin_renderer.py:110-141): points [N,3] in the frame of
    scene_config's eval_bbx, voxelised at voxel_size (`VoxelCloud`), seen by the pinhole camera K at camera -> world `pose`;
    pixel (r, c) casts its ray through the INTEGER image point (c, r).  Returns (depth [H,W] f32: camera-space z of the entry
    into the first occupied voxel + 0.02, 0 where nothing is hit or the camera stands inside that voxel; voxel [H,W] int32:
    its linear index (x G + y) G + z, -1 there) on the device."""
    cloud = VoxelCloud(points, scene_config, voxel_size, device)
    depth = torch.empty(int(height) * int(width), dtype=torch.float32, device=cloud.dev)
    voxel = torch.empty(int(height) * int(width), dtype=torch.int32, device=cloud.dev)
    cloud.trace(K, pose, height, width, depth, voxel)
    return depth.view(int(height), int(width)), voxel.view(int(height), int(width))


@torch.no_grad()
def reproj_filter(src_file, target_file, data_path, output_path, gt=False, voxel_size=0.01, visualize=False, znear=ZNEAR,
                  zfar=ZFAR, cull="back", device=None, verbose=True, keep_faces=False, min_corners=1, min_component_faces=0, bounded=True):
    """utils/reproj_filter.py: keep the vertices of target_file that a training view of data_path sees on src_file.
    A source WITH faces (a mesh).  Per view: render the depth of the source mesh, back-project every pixel with depth > 0
    at its integer pixel coordinates, mark the nearest target vertex when it is closer than 2 sqrt(2) voxel_size (GT units).
    Both files are carried to GT coordinates by config.yaml's sfm2gt unless `gt`.  Writes <output_path>/reprojected.ply (np.unique of the marked rows
    [xyz, rgb], double xyz + uchar colours); `visualize` also writes render/depth/<name>.npy and render/reprojects/<name>.ply.
    A source WITHOUT faces (a point cloud; :110-115, utils/kaolin_renderer.py).  Source and target go to GT coordinates; the
    source is voxelised over config.yaml's eval_bbx at level floor(log2(longest edge / voxel_size)) (`VoxelCloud`); every
    pixel of every view is traced to the first occupied voxel (csrc/ncw_voxview.hip).  A target vertex is kept iff the voxel
    of the SOURCE's grid that contains it was the first hit of some training-view pixel (the reference indexes the target by
    the source's point -> voxel table, which is this rule when the two files hold the same points -- its one use -- and is
    undefined otherwise).  The nearest-neighbour marking and its 2 sqrt(2) voxel_size are not used on this path (:224-225);
    znear / zfar / cull do not apply.  A pixel that misses marks nothing and has depth 0 (the reference's wrap-around of
    pid = -1 and its depth of 0.02 there are not reproduced).
    `keep_faces` (default off; the reference has no such mode, the rule is this project's): the TARGET file must have faces
    (ValueError before any view is rendered otherwise), and <output_path>/reprojected_mesh.ply is written IN ADDITION to
    reprojected.ply, which stays byte for byte what it is without the option.  After all views are marked, from the same
    per-vertex flags reprojected.ply is written from (mesh source: Target.flags; point-cloud source: VoxelCloud.select):
    meshops.face_select keeps a target face iff at least `min_corners` (1..3) of its corners are marked, then -- with
    min_component_faces > 0 -- only the faces of connected components (by shared vertex index, over the kept faces) of at
    least that many faces, then meshops.submesh compacts: the vertices some kept face uses, in FILE ORDER (no np.unique, no
    welding), GT coordinates as doubles, uchar colours (zeros without), faces remapped.
    Why min_corners = 1 is the default: every back-projected pixel marks ONE nearest vertex, so where the mesh is finer than
    the pixels a visible triangle rarely has all three corners marked; a strict rule would punch holes that a surface-based
    recall then counts against the model.  The one-ring rule admits at most one triangle's width of surface beyond the marked
    vertices.  min_corners = 3 is for whoever wants "nothing the reference would drop": its vertex set is a subset of the
    rows of reprojected.ply.
    `bounded` (mesh source only; default True): the marking asks for the nearest target vertex within the threshold only
    (`Target`): reprojected.ply and reprojected_mesh.ply are byte for byte what bounded=False, the earlier path, writes.
    Returns (xyz float64 [K,3], rgb uint8 [K,3]) -- the rows of reprojected.ply, whatever keep_faces is."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    log = print if verbose else (lambda *a, **k: None)
    os.makedirs(output_path, exist_ok=True)
    log("result will be saved to %s" % output_path)
    with open(os.path.join(data_path, "config.yaml")) as fh:
        scene_config = yaml.safe_load(fh)
    S = np.array(scene_config["sfm2gt"], dtype=np.float64)
    views = load_views(data_path, S)
    log("views to process: %d" % len(views))

    t_xyz, t_faces, t_rgb = ply.read_mesh(target_file)
    if keep_faces:
        if int(min_corners) not in (1, 2, 3):
            raise ValueError("reproj_filter: min_corners must be 1, 2 or 3 (got %r)" % (min_corners,))
        if t_faces.shape[0] == 0:
            raise ValueError("reproj_filter: keep_faces needs a target with faces; %s has none" % target_file)
    if not gt:
        t_xyz = evalmesh.apply_transform(t_xyz, S)
    if t_rgb is None:
        log("No color found in target point cloud")

    s_verts, s_faces, _ = ply.read_mesh(src_file)
    if s_faces.shape[0] == 0:
        log("reproject point cloud")
        xyz, rgb, flags = _filter_cloud(s_verts if gt else evalmesh.apply_transform(s_verts, S), t_xyz, t_rgb, views, scene_config,
                                        output_path, voxel_size, visualize, dev, with_flags=True)
        ply.write(os.path.join(output_path, "reprojected.ply"), xyz, rgb=rgb)
        log("kept %d of %d vertices" % (xyz.shape[0], t_xyz.shape[0]))
        if keep_faces:
            _write_filtered_mesh(output_path, t_xyz, t_faces, t_rgb, flags, min_corners, min_component_faces, dev, log)
        return xyz, rgb
    target = Target(t_xyz, t_rgb, 2 * np.sqrt(2) * voxel_size, dev, bounded=bounded)
    mesh = RasterMesh(s_verts, s_faces, dev)
    zbuf = None
    for v in views:
        w, h = v["wh"]
        # the source mesh is rasterized in its file's frame: with E (SfM frame) unless gt, else with E inv(sfm2gt) -- the
        # reference's render of the GT-frame mesh with E inv(sfm2gt) in both cases, up to rounding
        s = mesh.view_struct(v["K"], v["E_gt"] if gt else v["E"], h, w, znear, zfar, cull)
        if zbuf is None or zbuf.numel() != h * w:
            zbuf = torch.empty(h * w, dtype=torch.int64, device=dev)
        mesh.rasterize(s, zbuf)
        depth, _ = resolve(zbuf, h, w, with_face=False)
        pts, _ = backproject(depth, backproject_matrix(v["K"], v["pose"], target.centre))
        target.mark(pts)
        if pts.shape[0] < 10:
            log("[WARNING] invalid view at %s" % v["name"])
        if visualize:
            stem = os.path.splitext(v["name"])[0]
            for sub in ("depth", "reprojects"):
                os.makedirs(os.path.join(output_path, "render", sub), exist_ok=True)
            np.save(os.path.join(output_path, "render", "depth", stem + ".npy"), depth.cpu().numpy())
            ply.write(os.path.join(output_path, "render", "reprojects", stem + ".ply"),
                      pts.double().cpu().numpy() + target.centre)
    xyz, rgb = target.rows()
    ply.write(os.path.join(output_path, "reprojected.ply"), xyz, rgb=rgb)
    log("kept %d of %d vertices" % (xyz.shape[0], target.m))
    if keep_faces:
        _write_filtered_mesh(output_path, target.xyz, t_faces, target.rgb, target.flags[: target.m], min_corners,
                             min_component_faces, dev, log)
    return xyz, rgb


def _write_filtered_mesh(output_path, xyz, faces, rgb, flags, min_corners, min_component_faces, dev, log):
    """reprojected_mesh.ply of reproj_filter(keep_faces=True): the target's faces (xyz [V,3] float64 in GT coordinates, faces
    [F,3], rgb uint8 [V,3] or None, numpy) with at least min_corners corners set in flags ([V] on the device), optionally only
    the components of at least min_component_faces kept faces, compacted in file order."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    V = xyz.shape[0]
    rgb = np.zeros((V, 3), dtype=np.uint8) if rgb is None else np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    f = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int64)).to(dev)
    flags = (flags != 0).to(torch.uint8)
    keep = meshops.face_select(f, V, vflags=flags, min_corners=min_corners)
    if int(min_component_faces) > 0:
        labels, sizes = meshops.components(f, V, keep)
        ok = meshops.select_components(sizes, min_faces=int(min_component_faces))
        keep = meshops.face_select(f, V, vflags=flags, min_corners=min_corners, labels=labels, comp_ok=ok)
    v, fo, c, _ = meshops.submesh(torch.from_numpy(xyz).to(dev), f, keep, torch.from_numpy(rgb).to(dev))
    ply.write(os.path.join(output_path, "reprojected_mesh.ply"), v.cpu().numpy(), fo.cpu().numpy(), rgb=c.cpu().numpy())
    log("kept %d of %d faces (%d vertices)" % (fo.shape[0], f.shape[0], v.shape[0]))


def _filter_cloud(s_xyz, t_xyz, t_rgb, views, scene_config, output_path, voxel_size, visualize, dev, with_flags=False):
    """The point-cloud source of reproj_filter (source and target already in GT coordinates; scene_config: the parsed
    config.yaml): one trace per view with the pose inv(E inv(sfm2gt)), one select over the target at the end; the unique
    rows of the kept vertices (with_flags: and the per-vertex flags they were taken from, bool [N] on the device)."""
    cloud = VoxelCloud(s_xyz, scene_config, voxel_size, dev)
    depth = None
    for v in views:
        w, h = v["wh"]
        if visualize and (depth is None or depth.numel() != h * w):
            depth = torch.empty(h * w, dtype=torch.float32, device=dev)
        cloud.trace(v["K"], v["pose"], h, w, depth=depth if visualize else None)
        if visualize:
            stem = os.path.splitext(v["name"])[0]
            for sub in ("depth", "reprojects"):
                os.makedirs(os.path.join(output_path, "render", sub), exist_ok=True)
            np.save(os.path.join(output_path, "render", "depth", stem + ".npy"), depth.view(h, w).cpu().numpy())
            pts, _ = backproject(depth.view(h, w), backproject_matrix(v["K"], v["pose"], cloud.origin))
            ply.write(os.path.join(output_path, "render", "reprojects", stem + ".ply"),
                      pts.double().cpu().numpy() + cloud.origin)
    t_xyz = np.ascontiguousarray(t_xyz, dtype=np.float64).reshape(-1, 3)
    rgb = np.zeros(t_xyz.shape, dtype=np.uint8) if t_rgb is None else np.asarray(t_rgb, dtype=np.uint8).reshape(-1, 3)
    flags = cloud.select(t_xyz)
    rows = unique_rows(t_xyz, rgb, flags, dev)
    return rows + (flags,) if with_flags else rows


# ---------------------------------------------------------------------------------------------------
# scripts/eval_pipeline.sh
# ---------------------------------------------------------------------------------------------------
# per scene: F-score thresholds, SfM crop track length / reprojection error / voxel size (scripts/eval_pipeline.sh:22-53)
SCENES = {
    "brandenburg_gate": {"thresholds": "0.01,1,0.01", "track_length": 14, "reproj_error": 2.0, "voxel_size": 2.0},
    "lincoln_memorial": {"thresholds": "0.005,0.3,0.005", "track_length": 12, "reproj_error": 1.6, "voxel_size": 0.04},
    "palacio_de_bellas_artes": {"thresholds": "0.01,1,0.01", "track_length": 12, "reproj_error": 1.5, "voxel_size": 2.0},
    "pantheon_exterior": {"thresholds": "0.01,1,0.01", "track_length": 12, "reproj_error": 1.4, "voxel_size": 0.1},
}


def eval_pipeline(scene_name, pred_dir, data_root="data/heritage-recon", verbose=True, surface=None, surface_seed=0,
                  surface_mode="stratified", error_clouds=None, keep_faces=False, min_corners=1, min_component_faces=0,
                  exact_recall=False, normals=None):
    """scripts/eval_pipeline.sh in one process: the reprojection filter of <pred_dir>/mesh/extracted_mesh_level_10_colored.ply
    against itself (written to <pred_dir>/mesh/reprojected.ply), then evalmesh.eval_mesh of that file against
    <data_root>/<scene>/<scene>.ply with the scene's thresholds and the SfM crop of <data_root>/<scene>/neuralsfm, results in
    <pred_dir>/mesh/eval_<scene>_reprojected.ply/.  surface / surface_seed / surface_mode / error_clouds go to eval_mesh as
    they are (reprojected.ply is a point cloud, so `surface` is refused there).  Returns the last threshold's metrics.
    keep_faces (default off; not in the reference): filter with reproj_filter(keep_faces=True, min_corners,
    min_component_faces) and score <pred_dir>/mesh/reprojected_mesh.ply instead, results in eval_<scene>_reprojected_mesh.ply/;
    `surface` and `exact_recall` then go to eval_mesh and work, because that file has faces.  Without keep_faces
    exact_recall is refused (ValueError): reprojected.ply is a point cloud.  `normals` = K goes to eval_mesh (normal
    consistency of the scored clouds)."""
    if scene_name not in SCENES:
        raise ValueError("Not supported scene: %s (one of %s)" % (scene_name, ", ".join(sorted(SCENES))))
    if exact_recall and not keep_faces:
        raise ValueError("--exact_recall needs a triangle mesh: without --keep_faces the pipeline scores mesh/reprojected.ply, "
                         "a point cloud")
    sc = SCENES[scene_name]
    pred_path = os.path.join(pred_dir, "mesh")
    scene_dir = os.path.join(data_root, scene_name)
    mesh_file = os.path.join(pred_path, "extracted_mesh_level_10_colored.ply")
    if not os.path.isfile(mesh_file):  # before anything is created or a GPU is touched
        raise FileNotFoundError("No such file: %s (the run directory holds no extracted mesh)" % mesh_file)
    reproj_filter(mesh_file, mesh_file, scene_dir, pred_path, verbose=verbose, keep_faces=keep_faces, min_corners=min_corners,
                  min_component_faces=min_component_faces)
    with open(os.path.join(scene_dir, "config.yaml")) as fh:
        scene_config = yaml.safe_load(fh)
    sfm = {"path": os.path.join(scene_dir, "neuralsfm"), "track_length": sc["track_length"],
           "reproj_error": sc["reproj_error"], "voxel_size": sc["voxel_size"]}
    scored = "reprojected_mesh.ply" if keep_faces else "reprojected.ply"
    return evalmesh.eval_mesh(os.path.join(pred_path, scored), os.path.join(scene_dir, scene_name + ".ply"),
                              scene_config, False, threshold=evalmesh.parse_thresholds(sc["thresholds"]), bbx_name="eval_bbx",
                              save_name=scene_name + "_" + scored, sfm=sfm, verbose=verbose, surface=surface,
                              surface_seed=surface_seed, surface_mode=surface_mode, error_clouds=error_clouds,
                              exact_recall=exact_recall, **({} if normals is None else {"normals": normals}))
