"""The training ray cache writer: `<root_dir>/<cache_dir>/splits/split_*/{rays,rgbs}N.npz`, the files scripts/train.py and
`raycache.RayCache` start from, built from a scene directory on the GPU.

    build_cache("data/heritage-recon/brandenburg_gate", semantic_map_path="semantic_maps", split_to_chunks=64)

Replaces the reference's tools/prepare_data/prepare_data_cache.py:78-239 over `PhototourismDataset(split="train")`
(datasets/phototourism.py:150-209, 316-681), which needs CUDA, kaolin, open3d, cv2, kornia and h5py.  There every image goes
through the host several times (kaolin trace in 100 k-ray chunks with a .cpu() each, a torch.cat of 13 columns, boolean
indexing).  Here, per image: the key-points become two planes (`ncw_sfm_depth_splat`), ONE launch writes the finished rows of all
pixels (`ncw_cache_rows`: rays, both octree walks, label, depth, weight, rgb, keep), `keep.nonzero()` + `ncw_batch_assemble`
compact them, and only the surviving rows leave the device.

Row layout: o(3) d(3) near far ts [label] depth weight 0 -- 13 columns with labels, 12 without, what `ncw_batch_assemble` and
`RayCache` read.  The reference's code concatenates the same columns WITHOUT the last (12 / 11) although its comment says 13 and
its reader slices [10:13] (phototourism.py:611-636, 716-724); the zero column is never read.

Not pinned against the reference: its `cv2.resize(..., INTER_NEAREST)` of the label maps (cv2 is not a dependency; the kernel
samples floor(row hs / h), floor(col ws / w)) and its unseeded random draws (`depth_percent` padding, chunk padding: drawn here
from seeded generators, same lengths and semantics).  Only npz output; h5 is refused (h5py is not a dependency, RayCache reads npz).
"""
import ctypes as C
import json
import os
import time

import numpy as np
import torch

from . import lib as L
from . import colmap, views, voxel

# datasets/phototourism.py:81-92: the share of rays with a key-point depth each image is padded up to
DEPTH_PERCENT = {"brandenburg_gate": 0.2, "palacio_de_bellas_artes": 0.4}


# ---------------------------------------------------------------------------------------------------
# the SfM points as the dataset holds them
# ---------------------------------------------------------------------------------------------------
def read_points3d_table(path):
    """COLMAP `points3D.bin` by point id, as phototourism.py:530-534 holds it: (xyz float32 [max_id + 1, 3], error float32
    [max_id + 1]); rows of ids the file does not list are ones, as `torch.ones` leaves them there."""
    ids, xyz, err, _ = colmap.read_points3d(path)
    size = int(ids.max()) + 1 if len(ids) else 1
    xyz_t = np.ones((size, 3), dtype=np.float32)
    err_t = np.ones(size, dtype=np.float32)
    xyz_t[ids] = xyz.astype(np.float32)
    err_t[ids] = err.astype(np.float32)
    return xyz_t, err_t


def image_keypoints(xys, point3d_ids, xyz_table, err_table, width, height, img_downscale=1):
    """phototourism.py:566-578 + :185-201 for one image: the key-points with a 3-D point, as (xyz float32 [m,3], err float32
    [m], px int32 [m,2] = (col, row) = round_half_even(xys / img_downscale) in float64, err_mean = the mean error of the
    key-points that land inside the width x height image, float64; nan when none does)."""
    ok = point3d_ids != -1
    ids = point3d_ids[ok]
    px = np.rint(xys[ok] / img_downscale).astype(np.int64)  # torch.round of the float64 tensor: half to even
    inside = (px[:, 0] >= 0) & (px[:, 0] < width) & (px[:, 1] >= 0) & (px[:, 1] < height)
    err = err_table[ids]
    err_mean = float(np.mean(err[inside].astype(np.float64))) if inside.any() else float("nan")
    px = np.clip(px, -2 ** 31, 2 ** 31 - 1).astype(np.int32)  # the kernel takes int32; what is clipped is far outside any image
    return np.ascontiguousarray(xyz_table[ids]), np.ascontiguousarray(err), np.ascontiguousarray(px), err_mean


def load_label_map(root_dir, semantic_map_path, image_name, width, height, img_downscale=1):
    """<root>/<semantic_map_path>/<stem>.npz["arr_0"] at its own size, uint8 (phototourism.py:594-609).  The reference resizes
    it to (ws // downscale, hs // downscale) and concatenates it to the rays: a map whose resized size is not the image's is an
    error there too (a shape mismatch in torch.cat), reported here by name."""
    path = os.path.join(root_dir, semantic_map_path, image_name.split(".")[0] + ".npz")
    m = np.load(path)["arr_0"]
    if m.ndim != 2:
        raise ValueError("label map %s: expected [h, w], got %s" % (path, m.shape))
    if (m.shape[1] // img_downscale, m.shape[0] // img_downscale) != (width, height):
        raise ValueError("label map %s is %d x %d (// %d = %d x %d) but the image is %d x %d"
                         % (path, m.shape[1], m.shape[0], img_downscale, m.shape[1] // img_downscale,
                            m.shape[0] // img_downscale, width, height))
    if m.dtype != np.uint8:
        if m.size and (m.min() < 0 or m.max() > 255):
            raise ValueError("label map %s holds labels outside 0..255" % path)
        m = m.astype(np.uint8)
    return np.ascontiguousarray(m)


# ---------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------
def _octree_struct(octree_data):
    """NcwCacheOctree of a voxel.OctreeData, built per call: it holds raw `occ` / `brick` pointers, which must not outlive the
    dictionary's tensors (an octree refresh replaces them) nor be stored in a dictionary that gets checkpointed."""
    voxel.ensure_occupancy(octree_data)
    so = octree_data.get("_scene_origin_host")  # voxel.get_near_far's cache: plain floats, one device -> host read per octree
    if so is None:
        o = octree_data["scene_origin"]
        so = (C.c_float * 3)(*[float(v) for v in (o.tolist() if hasattr(o, "tolist") else o)])
        octree_data["_scene_origin_host"] = so
    return L.NcwCacheOctree((C.c_float * 3)(*so), float(octree_data["scale"]), int(octree_data["level"]), 0,
                            octree_data["occ"].data_ptr(), octree_data["brick"].data_ptr())


def _dev_u8(a, device):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.uint8:
        raise ValueError("expected uint8, got %s" % t.dtype)
    return t.to(device).contiguous()


def sfm_depth_planes(xyz, err, px, err_mean, w2c, width, height, device):
    """`ncw_sfm_depth_splat`: (depth_z [h*w], weight [h*w]) f32 on the device of the key-points xyz [n,3] / err [n] / px [n,2]
    (col, row); w2c: the COLMAP world -> camera matrix (its first three rows).  Zero planes when n == 0."""
    device = torch.device(device)
    if device.type != "cuda":
        raise L.NeuconwHipError("cachebuild.sfm_depth_planes: not a GPU device; there is no CPU fallback")
    hw = int(width) * int(height)
    n = int(len(px))
    winner = torch.empty(hw, device=device, dtype=torch.int32)
    depth_z = torch.empty(hw, device=device, dtype=torch.float32)
    weight = torch.empty(hw, device=device, dtype=torch.float32)
    xyz_d = err_d = px_d = None
    if n:
        xyz_d = torch.as_tensor(xyz, dtype=torch.float32).reshape(n, 3).to(device).contiguous()
        err_d = torch.as_tensor(err, dtype=torch.float32).reshape(n).to(device).contiguous()
        px_d = torch.as_tensor(px, dtype=torch.int32).reshape(n, 2).to(device).contiguous()
        if not err_mean > 0:  # no key-point inside the image: nothing can land (and the mean of nothing is nan)
            n = 0
    w2c_h = (C.c_float * 12)(*[float(v) for v in np.asarray(w2c, dtype=np.float64)[:3].reshape(-1)])
    L.check(L.get_lib().ncw_sfm_depth_splat(L.ptr(xyz_d), L.ptr(err_d), L.ptr(px_d), n, float(err_mean) if n else 1.0, w2c_h,
                                            int(width), int(height), L.ptr(winner), L.ptr(depth_z), L.ptr(weight),
                                            L.stream_ptr(device)), "ncw_sfm_depth_splat")
    return depth_z, weight


def cache_rows(camera, image, image_id, depth_z, weight, label_map=None, hit_octree=None, range_octree=None, voxel_size=0.0,
               p0=0, n=None):
    """`ncw_cache_rows` for the pixels [p0, p0 + n) of the view: (rows [n, 13 | 12], rgbs [n, 3], keep [n] uint8) on the device
    of `image` ([h, w, 3] uint8 device tensor)."""
    if not (torch.is_tensor(image) and image.is_cuda):
        raise L.NeuconwHipError("cachebuild.cache_rows: the image is not on a GPU; there is no CPU fallback")
    dev = image.device
    hw = camera.width * camera.height
    if tuple(image.shape) != (camera.height, camera.width, 3) or image.dtype != torch.uint8:
        raise ValueError("cache_rows: image must be uint8 [%d, %d, 3], got %s %s" % (camera.height, camera.width, image.dtype,
                                                                                     tuple(image.shape)))
    if depth_z.numel() != hw or weight.numel() != hw:
        raise ValueError("cache_rows: the depth / weight planes hold %d / %d entries for %d pixels" % (depth_z.numel(), weight.numel(), hw))
    n = hw - p0 if n is None else int(n)
    ncols = 13 if label_map is not None else 12
    rows = torch.empty(n, ncols, device=dev, dtype=torch.float32)
    rgbs = torch.empty(n, 3, device=dev, dtype=torch.float32)
    keep = torch.empty(n, device=dev, dtype=torch.uint8)
    lh, lw = (int(label_map.shape[0]), int(label_map.shape[1])) if label_map is not None else (0, 0)
    hit_s = _octree_struct(hit_octree) if hit_octree is not None else None
    rng_s = _octree_struct(range_octree) if range_octree is not None else None
    hit = C.byref(hit_s) if hit_s is not None else None
    rng = C.byref(rng_s) if rng_s is not None else None
    L.check(L.get_lib().ncw_cache_rows(C.byref(camera.struct()), L.ptr(image.contiguous()), L.ptr(label_map), lh, lw,
                                       L.ptr(depth_z.contiguous()), L.ptr(weight.contiguous()), int(image_id), float(voxel_size),
                                       hit, rng, int(p0), n, ncols, L.ptr(rows), L.ptr(rgbs), L.ptr(keep), L.stream_ptr(dev)),
            "ncw_cache_rows")
    return rows, rgbs, keep


def compact(rows, rgbs, keep):
    """`rays[valid_mask]`, `img[valid_mask]` (phototourism.py:656-657) on the device: the kept rows in pixel order, gathered by
    `ncw_batch_assemble` from `keep.nonzero()`."""
    dev = rows.device
    ncols = rows.shape[1]
    idx = keep.nonzero().reshape(-1)
    m = int(idx.shape[0])  # the one device -> host sync per image (a data-dependent shape)
    if m == 0:
        return rows.new_empty(0, ncols), rgbs.new_empty(0, 3)
    sem = ncols == 13
    r11 = torch.empty(m, 11, device=dev, dtype=torch.float32)
    ts = torch.empty(m, device=dev, dtype=torch.int64)
    label = torch.empty(m, device=dev, dtype=torch.int64) if sem else None
    out_rgb = torch.empty(m, 3, device=dev, dtype=torch.float32)
    L.check(L.get_lib().ncw_batch_assemble(L.ptr(rows), ncols, L.ptr(rgbs), L.ptr(idx), rows.shape[0], m, int(sem), L.ptr(r11),
                                           L.ptr(ts), L.ptr(label), L.ptr(out_rgb), None, 0, None, L.stream_ptr(dev)),
            "ncw_batch_assemble")
    # the batch layout back to the cache's: image ids and labels are small integers, exact in float32
    cols = [r11[:, :8], ts.float()[:, None]] + ([label.float()[:, None]] if sem else []) + [r11[:, 8:]]
    return torch.cat(cols, 1), out_rgb


def pad_depth_percent(rays, rgbs, depth_percent, generator):
    """phototourism.py:659-675: pad the image's rows with random copies of rows that have a key-point depth until those make
    up `depth_percent` of them, then ONE random permutation of rays and rgbs alike.  Same padding length as the reference
    (which cannot run when the share is already reached -- its torch.rand of a negative length raises; here nothing is padded
    then, and nothing when no row has a depth).  Draws come from `generator` (a CPU torch.Generator)."""
    valid = rays[:, rays.shape[1] - 3] > 0  # the key-point depth column (the reference's rays[:, -2])
    valid_num = int(valid.sum())
    cur = int(rays.shape[0])
    pad = int(np.ceil((depth_percent * cur - valid_num) / (1 - depth_percent)))
    pad = max(pad, 0) if valid_num > 0 else 0
    pad_ind = torch.floor(torch.rand(pad, generator=generator) * valid_num).long().to(rays.device)
    perm = torch.randperm(cur + pad, generator=generator).to(rays.device)
    rays = torch.cat([rays, rays[valid][pad_ind]], 0)[perm]
    rgbs = torch.cat([rgbs, rgbs[valid][pad_ind]], 0)[perm]
    return rays, rgbs


def build_image(camera, image, image_id, keypoints, w2c, label_map=None, hit_octree=None, range_octree=None, voxel_size=0.0,
                depth_percent=0.0, generator=None, device=None):
    """The cache rows of one training image: (rays [m, 13 | 12], rgbs [m, 3]) on the device, rows in pixel order.
    camera: views.Camera with the image's near / far; image: decoded [h, w, 3] uint8 (numpy or tensor); keypoints:
    `image_keypoints`' tuple; w2c: COLMAP's world -> camera matrix; label_map: uint8 [hs, ws] or None (12 columns);
    hit_octree / range_octree: voxel.octree_from_sfm(expand=1, radius=1) / (expand=2, radius=1.5), or None (use_voxel False)."""
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise L.NeuconwHipError("cachebuild.build_image: not a GPU device; the ray cache has no CPU fallback")
    xyz, err, px, err_mean = keypoints
    depth_z, weight = sfm_depth_planes(xyz, err, px, err_mean, w2c, camera.width, camera.height, device)
    img = _dev_u8(image, device)
    lab = _dev_u8(label_map, device) if label_map is not None else None
    rows, rgbs, keep = cache_rows(camera, img, image_id, depth_z, weight, lab, hit_octree, range_octree, voxel_size)
    if hit_octree is not None and range_octree is not None:
        rows, rgbs = compact(rows, rgbs, keep)
    if depth_percent > 0 and rows.shape[0] > 0:
        rows, rgbs = pad_depth_percent(rows, rgbs, float(depth_percent), generator or torch.Generator().manual_seed(0))
    return rows, rgbs


# ---------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------
def _take(arrays, offsets, start, stop):
    """Rows [start, stop) of the concatenation of `arrays` (offsets = their cumulative starts), without concatenating all."""
    out = []
    k = int(np.searchsorted(offsets, start, side="right")) - 1
    while start < stop:
        a = arrays[k]
        lo = start - int(offsets[k])
        hi = min(a.shape[0], lo + (stop - start))
        if hi > lo:
            out.append(a[lo:hi])
            start += hi - lo
        k += 1
    return torch.cat(out, 0)


def write_chunks(arrays, split_path, n_chunks, img_downscale, padding_index, arr_type):
    """prepare_data_cache.py:78-160 `split_to_chunks` for npz: the list's rows followed by the rows `padding_index` picks from
    them, cut into chunks of (total // n_chunks) rows -> split_path/split_i/<arr_type><N>.npz (`arr_0`) and
    <arr_type><N>_meta_info.json.  Returns the chunk length."""
    arrays = [torch.as_tensor(a) for a in arrays]
    all_lengths = int(sum(a.shape[0] for a in arrays))
    offsets = np.concatenate([[0], np.cumsum([a.shape[0] for a in arrays])])[:-1] if arrays else np.zeros(0, dtype=np.int64)
    padding_index = np.asarray(padding_index, dtype=np.int64).reshape(-1)
    if len(padding_index):
        pad = torch.cat([_take(arrays, offsets, int(i), int(i) + 1) for i in padding_index], 0)
        offsets = np.concatenate([offsets, [all_lengths]])
        arrays = arrays + [pad]
    total = all_lengths + len(padding_index)
    chunk_length = total // n_chunks
    if chunk_length < 1:
        raise ValueError("write_chunks: %d rows cannot fill %d chunks" % (total, n_chunks))
    for i, c in enumerate(range(0, total, chunk_length)):
        os.makedirs(os.path.join(split_path, "split_%d" % i), exist_ok=True)
        chunk = _take(arrays, offsets, c, min(total, c + chunk_length)).numpy()
        np.savez_compressed(os.path.join(split_path, "split_%d" % i, "%s%d.npz" % (arr_type, img_downscale)), chunk)
    with open(os.path.join(split_path, "%s%d_meta_info.json" % (arr_type, img_downscale)), "w") as fh:
        json.dump({"data_length": total, "chunk_length": chunk_length, "n_trunks": n_chunks}, fh)
    return chunk_length


def chunk_padding(all_lengths, n_chunks, seed):
    """prepare_data_cache.py:189-196: the rows repeated so that the total divides by n_chunks -- n_chunks - all % n_chunks of
    them (none when it divides already), drawn without replacement; seeded here."""
    padding_size = n_chunks - all_lengths % n_chunks
    if padding_size == n_chunks:
        return np.zeros(0, dtype=np.int64)
    return np.random.RandomState(seed).choice(all_lengths, padding_size, replace=False).astype(np.int64)


def write_cache(all_rays, all_rgbs, root_dir, cache_dir="cache", img_downscale=1, split_to_chunks=-1, seed=0):
    """prepare_data_cache.py:178-239 for npz: the per-image lists -> the cache files.  The SAME padding indices go to rays and
    rgbs.  Returns the list of files written."""
    out_dir = os.path.join(root_dir, cache_dir)
    os.makedirs(out_dir, exist_ok=True)
    if split_to_chunks > 0:
        split_path = os.path.join(out_dir, "splits")
        os.makedirs(split_path, exist_ok=True)
        all_lengths = int(sum(r.shape[0] for r in all_rgbs))
        padding_index = chunk_padding(all_lengths, split_to_chunks, seed)
        write_chunks(all_rgbs, split_path, split_to_chunks, img_downscale, padding_index, "rgbs")
        write_chunks(all_rays, split_path, split_to_chunks, img_downscale, padding_index, "rays")
        return sorted(os.path.join(dp, f) for dp, _, fs in os.walk(split_path) for f in fs)
    files = []
    for name, arrs in (("rays", all_rays), ("rgbs", all_rgbs)):
        files.append(os.path.join(out_dir, "%s%d.npz" % (name, img_downscale)))
        np.savez_compressed(files[-1], torch.cat([torch.as_tensor(a) for a in arrs], 0).numpy())
    return files


def open_scene(root_dir, img_downscale=1, sfm_path=None, device=None, depth_percent=None, use_voxel=True, who="build_cache"):
    """What `build_cache` reads and builds ONCE per scene, before its loop over the training images -- shared with
    raysource.RaySource.from_scene, so both start from the same readers, octrees and defaults.  Returns a dict: `root_dir`
    (normalised), `img_downscale`, `device`, `scene` (views.read_scene), `depth_percent` (None resolved to the reference's
    per-scene value), `xyz_table` / `err_table`, `hit` / `range` (the two SfM octrees, None without use_voxel), `voxel_size`."""
    import yaml

    img_downscale = int(img_downscale)
    if img_downscale < 1:
        raise ValueError("image can only be downsampled, please set img_downscale>=1!")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise L.NeuconwHipError("cachebuild.%s: not a GPU device; the ray cache has no CPU fallback" % who)
    root_dir = os.path.normpath(root_dir)
    scene = views.read_scene(root_dir, sfm_path, with_points=True)
    if depth_percent is None:
        depth_percent = DEPTH_PERCENT.get(os.path.basename(root_dir), 0.0)
    xyz_table, err_table = read_points3d_table(os.path.join(scene["sp"], "points3D.bin"))
    hit = rng = None
    voxel_size = 0.0
    if use_voxel:
        with open(os.path.join(root_dir, "config.yaml"), "r") as fh:
            cfg = yaml.load(fh, Loader=yaml.FullLoader)
        voxel_size = float(cfg["voxel_size"])
        hit = voxel.octree_from_sfm(root_dir, cfg["min_track_length"], voxel_size, device, sfm_path=scene["sfm_path"], expand=1,
                                    radius=1)
        rng = voxel.octree_from_sfm(root_dir, cfg["min_track_length"], voxel_size, device, sfm_path=scene["sfm_path"], expand=2,
                                    radius=1.5)
    return {"root_dir": root_dir, "img_downscale": img_downscale, "device": device, "scene": scene, "depth_percent": depth_percent,
            "xyz_table": xyz_table, "err_table": err_table, "hit": hit, "range": rng, "voxel_size": voxel_size}


def scene_items(sc, semantic_map_path=None, scene_origin=None, scene_radius=None, stats=None):
    """The loop of `build_cache` over the training images (`split != "test"`) of an `open_scene` dict, up to the device work:
    yields `build_image`'s arguments per image -- (camera, decoded uint8 image, image id, key-point tuple, w2c, label map or
    None).  stats: a dict whose `t_decode` receives the host decode time."""
    root_dir, scene, img_downscale = sc["root_dir"], sc["scene"], sc["img_downscale"]
    for image_id in scene["ids_train"]:
        name = scene["images"][image_id]["name"]
        t0 = time.perf_counter()
        img = views._decode_image(os.path.join(root_dir, "dense", "images", name), img_downscale)
        h, w = img.shape[:2]
        lab = load_label_map(root_dir, semantic_map_path, name, w, h, img_downscale) if semantic_map_path is not None else None
        if stats is not None:
            stats["t_decode"] = stats.get("t_decode", 0.0) + time.perf_counter() - t0
        K, w2c, c2w, _, _ = views.image_pose(scene, image_id, img_downscale)
        near, far = views.image_near_far(scene, w2c, scene_origin, scene_radius)
        cam = views.Camera(K, c2w, w, h, near, far)
        im = scene["images"][image_id]
        kp = image_keypoints(im["xys"], im["point3d_ids"], sc["xyz_table"], sc["err_table"], w, h, img_downscale)
        yield cam, img, image_id, kp, w2c, lab


def build_cache(root_dir, cache_dir="cache", img_downscale=1, semantic_map_path=None, split_to_chunks=-1, sfm_path=None, seed=0,
                device=None, cache_type="npz", depth_percent=None, use_voxel=True, scene_origin=None, scene_radius=None,
                stats=None):
    """tools/prepare_data/prepare_data_cache.py for the training images (`split != "test"`) of the scene at root_dir: writes
    <root_dir>/<cache_dir>/splits/split_i/{rays,rgbs}N.npz + {rays,rgbs}N_meta_info.json (split_to_chunks > 0) or one
    raysN.npz / rgbsN.npz.  Returns the files written.
      * sfm_path: the COLMAP model under dense/ (None: the reference's per-scene choice, views.reference_sfm_path);
      * semantic_map_path: directory (under root_dir) of the per-image label maps; None = 12-column rows without labels;
      * depth_percent: None = the reference's per-scene value (`DEPTH_PERCENT`, else 0);
      * use_voxel: near / far and the ray selection from the two SfM octrees of config.yaml (the reference's default);
      * seed: every random draw (depth padding per image, chunk padding) comes from generators seeded with it;
      * stats: an optional dict that receives timings (host decode, device, device -> host bytes, file writing)."""
    if cache_type != "npz":
        raise NotImplementedError("cache_type %r: only npz is written (h5py is not a dependency, and raycache.RayCache and the "
                                  "reference's config/defaults.py read npz); pass cache_type='npz'" % (cache_type,))
    sc = open_scene(root_dir, img_downscale, sfm_path, device, depth_percent, use_voxel)
    root_dir, img_downscale, device, scene = sc["root_dir"], sc["img_downscale"], sc["device"], sc["scene"]
    gen = torch.Generator().manual_seed(int(seed))
    all_rays, all_rgbs = [], []
    st = {"n_images": 0, "n_pixels": 0, "n_rays": 0, "d2h_bytes": 0, "t_decode": 0.0, "t_device": 0.0, "t_write": 0.0}
    t_loop = time.perf_counter()
    for cam, img, image_id, kp, w2c, lab in scene_items(sc, semantic_map_path, scene_origin, scene_radius, st):
        rays, rgbs = build_image(cam, img, image_id, kp, w2c, lab, sc["hit"], sc["range"], sc["voxel_size"], sc["depth_percent"], gen,
                                 device)
        all_rays.append(rays.cpu())
        all_rgbs.append(rgbs.cpu())
        st["n_images"] += 1
        st["n_pixels"] += cam.width * cam.height
        st["n_rays"] += int(rays.shape[0])
        st["d2h_bytes"] += 4 * (rays.numel() + rgbs.numel())
    st["t_device"] = time.perf_counter() - t_loop - st["t_decode"]  # everything in the loop that is not the host decode
    if not all_rays:
        raise ValueError("%s lists no training image registered in images.bin" % scene["tsv"])
    t0 = time.perf_counter()
    files = write_cache(all_rays, all_rgbs, root_dir, cache_dir, img_downscale, split_to_chunks, seed)
    st["t_write"] = time.perf_counter() - t0
    if stats is not None:
        stats.update(st)
    return files
