"""Preparing a scene from its COLMAP model: the two files every other tool starts from, `<scene>/config.yaml` and
`<scene>/<scene>.tsv`.

    cfg = scene_config_from_sfm("scene/dense/sparse/points3D.bin", "scene")     # tools/pre_process.py:35-46, 102-108, 135-158
    write_scene_config("scene", cfg)
    prepare_split("scene", num_test=10)                                         # tools/prepare_data/prepare_data_split.py

The split is the reference's `view_selection` (dataset_filter_utils.py:98-184: a per-pixel geometric test of every registered
image against the scene sphere), a permutation, and `filter_image_based_on_transient_percent` (:186-205: a label histogram per
image).  The per-pixel test is the only hot path: about 1.2 G rays for 1500 images of 1024 x 768, which the reference makes per
image after decoding the image only to learn its size.  Here the camera table of ALL views goes to the device once and ONE
`ncw_views_roi` launch (csrc/ncw_roi.hip) returns the count of region-of-interest pixels per view; image files are opened for
their header only.  The NIMA filter is dead in the reference (prepare_data_split.py:41 is commented out) and is not restated.
"""
import ctypes as C
import glob
import json
import os

import numpy as np

from . import colmap, labels
from . import lib as L

TRANSIENT_OBJECTS = ("person", "car", "bicycle", "minibike", "tree")  # prepare_data_split.py:44
CONFIG_KEYS = ("name", "origin", "radius", "eval_bbx", "sfm2gt", "min_track_length", "eval_bbx_detail", "voxel_size")
TSV_COLUMNS = ("filename", "id", "split", "dataset")
# the reference's prefixes of the copies it puts into trash_images/ (dataset_filter_utils.py:152, 180, 201)
REASON_COVIS, REASON_ROI, REASON_TRANSIENT = "less_covis", "less_ROI", "transient_much"


# ---------------------------------------------------------------------------------------------------
# config.yaml
# ---------------------------------------------------------------------------------------------------
def scene_config_from_sfm(points3d_path, name):
    """tools/pre_process.py:102-108 + 35-46 + 135-152 (`bbx_selection`, `generate_config`) as a dict, keys in the reference's
    order: from the SfM points with MORE THAN 2 observations, eval_bbx = eval_bbx_detail = the 4th and 96th percentile per axis
    (np.percentile, float64), origin = the centre of that box, scale = max(extent) / 2, radius = 2 scale, sfm2gt = identity,
    min_track_length = 2, voxel_size = 2 / 2**5 * scale - 1e-4.  Host numpy over `colmap.read_points3d`."""
    _, xyz, _, track = colmap.read_points3d(points3d_path)
    pts = xyz[track > 2]
    if len(pts) == 0:
        raise ValueError("%s holds no point with more than 2 observations: nothing to fit the scene box to" % points3d_path)
    lo, hi = np.percentile(pts, [4, 96], axis=0)
    half = float((hi - lo).max()) / 2  # half the longest edge of the box: the scale of an octree of level 5 with voxel_size below
    box = [lo.tolist(), hi.tolist()]
    values = {"name": name, "origin": ((lo + hi) / 2).tolist(), "radius": 2 * half, "eval_bbx": box,
              "sfm2gt": [[float(i == j) for j in range(4)] for i in range(4)], "min_track_length": 2,
              "eval_bbx_detail": [list(lo.tolist()), list(hi.tolist())], "voxel_size": half / 16 - 1e-4}
    return {k: values[k] for k in CONFIG_KEYS}


def _scene_name(root_dir):
    return os.path.basename(os.path.normpath(os.path.abspath(root_dir)))


def write_scene_config(root_dir, config=None, name=None, sfm_path="sparse", overwrite=False):
    """Writes <root_dir>/config.yaml as pre_process.py:156-158 does (block style, keys in the order given).  config: the dict to
    write; None = `scene_config_from_sfm` of <root_dir>/dense/<sfm_path>/points3D.bin under `name` (default: the directory
    name).  An existing config.yaml is refused with FileExistsError unless overwrite.  Returns the path."""
    import yaml

    path = os.path.join(root_dir, "config.yaml")
    if os.path.exists(path) and not overwrite:
        raise FileExistsError("%s exists: pass overwrite=True (--overwrite) to replace it" % path)
    if config is None:
        config = scene_config_from_sfm(os.path.join(root_dir, "dense", sfm_path, "points3D.bin"), name or _scene_name(root_dir))
    with open(path, "w") as fh:
        yaml.dump(dict(config), fh, default_flow_style=False, sort_keys=False)
    return path


# ---------------------------------------------------------------------------------------------------
# the cameras of the registered images
# ---------------------------------------------------------------------------------------------------
def scene_cameras(root_dir, sfm_path="sparse"):
    """One views.Camera per image registered in <root_dir>/dense/<sfm_path>/images.bin, file order, as
    dataset_filter_utils.py:101-133 + 161-169 builds them: K = the camera's fx, fy, cx, cy UNRESCALED (float32), c2w =
    inv(w2c)[:3] with columns 1, 2 negated (`views.image_pose`), and the size of the image FILE, read from its header with
    PIL.Image.open(path).size -- nothing is decoded (the reference decodes every image and uses only its size).  Every camera
    also carries `name`, `image_id`.  A registered image whose file is missing is a FileNotFoundError that names it."""
    from PIL import Image

    from . import views

    sp = os.path.normpath(os.path.join(root_dir, "dense", sfm_path))
    if not os.path.isfile(os.path.join(sp, "images.bin")):
        raise FileNotFoundError("no COLMAP model in %s (sfm_path %r)" % (sp, sfm_path))
    scene = {"images": colmap.read_images(os.path.join(sp, "images.bin")), "cams": colmap.read_cameras(os.path.join(sp, "cameras.bin"))}
    cams = []
    for iid, im in scene["images"].items():
        path = os.path.join(root_dir, "dense", "images", im["name"])
        if not os.path.isfile(path):
            raise FileNotFoundError("image %r (id %d) is registered in %s but %s does not exist"
                                    % (im["name"], iid, os.path.join(sp, "images.bin"), path))
        with Image.open(path) as img:
            w, h = img.size
        p = scene["cams"][im["camera_id"]]["params"]
        K = np.zeros((3, 3), dtype=np.float32)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[2, 2] = p[0], p[1], p[2], p[3], 1
        _, _, c2w, _, _ = views.image_pose(scene, iid, 1)
        cam = views.Camera(K, c2w, w, h, 0.0, 1.0)  # near / far: not part of the test
        cam.name, cam.image_id = im["name"], int(iid)
        cams.append(cam)
    return cams


# ---------------------------------------------------------------------------------------------------
# region-of-interest shares: the one launch
# ---------------------------------------------------------------------------------------------------
def pixel_prefix(cameras):
    """int64 [n + 1]: pixel (row, col) of view v is global pixel prefix[v] + row * width + col."""
    return np.concatenate([[0], np.cumsum([c.width * c.height for c in cameras], dtype=np.int64)]).astype(np.int64)


def roi_shares(cameras, origin, radius, device="cuda:0", with_mask=False):
    """dataset_filter_utils.py:161-178 for all `cameras` at once: uploads the camera table and the int64 pixel prefix and makes
    ONE `ncw_views_roi` launch.  Returns (shares float64 [n] = count / (w h), counts int64 [n]), and with_mask also the 0 / 1
    mask of every pixel as a device uint8 tensor [prefix[n]] (`pixel_prefix` locates a view in it).  Production passes no
    mask.  Raises NeuconwHipError without a GPU: there is no CPU fallback."""
    import torch

    cameras = list(cameras)
    if not cameras:
        raise ValueError("roi_shares: no camera")
    origin = [float(v) for v in np.asarray(origin, dtype=np.float64).reshape(-1)]
    if len(origin) != 3:
        raise ValueError("roi_shares: origin holds %d values, not 3" % len(origin))
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise L.NeuconwHipError("sceneprep.roi_shares: device %s is not a GPU; there is no CPU fallback" % (device,))
    n = len(cameras)
    table = (L.NcwViewCamera * n)(*[c.struct() for c in cameras])
    prefix = pixel_prefix(cameras)
    if int(np.diff(prefix).min()) < 1:  # views.Camera refuses an empty image; any other object with struct() is checked here
        raise ValueError("roi_shares: view %d has no pixel (its share would be 0 / 0)" % int(np.diff(prefix).argmin()))
    cams_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(device)
    prefix_d = torch.from_numpy(prefix).to(device)
    count_d = torch.empty(n, device=device, dtype=torch.int32)  # the entry point clears it
    mask_d = torch.empty(int(prefix[-1]), device=device, dtype=torch.uint8) if with_mask else None
    with torch.cuda.device(device):
        L.check(L.get_lib().ncw_views_roi(L.ptr(cams_d), L.ptr(prefix_d), n, (C.c_float * 3)(*origin), float(radius), L.ptr(count_d),
                                          L.ptr(mask_d), L.stream_ptr(device)), "ncw_views_roi")
    counts = count_d.cpu().numpy().view(np.uint32).astype(np.int64)
    shares = counts.astype(np.float64) / np.diff(prefix).astype(np.float64)
    return (shares, counts, mask_d) if with_mask else (shares, counts)


# ---------------------------------------------------------------------------------------------------
# static shares: the label histogram
# ---------------------------------------------------------------------------------------------------
def static_shares(root_dir, semantic_map_path, names, transient=TRANSIENT_OBJECTS):
    """dataset_filter_utils.py:186-195 per image name: the share of the pixels of <root_dir>/<semantic_map_path>/<stem>.npz
    ['arr_0'] (stem = the name up to its first '.') whose label is none of the `transient` ids (`labels.label_id`).  float64 [n].
    This runs on the HOST in numpy on purpose: the maps live on disk as compressed npz, and one histogram of a uint8 map is
    cheaper than its upload, so a launch would only add a copy.  A missing map is a FileNotFoundError that names the image (the
    reference stops there too, inside np.load)."""
    ids = sorted({labels.label_id(t) for t in transient})
    out = np.empty(len(names), dtype=np.float64)
    for k, name in enumerate(names):
        path = os.path.join(root_dir, semantic_map_path, str(name).split(".")[0] + ".npz")
        if not os.path.isfile(path):
            raise FileNotFoundError("no semantic map for image %r: %s does not exist" % (str(name), path))
        lab = np.load(path)["arr_0"]
        if lab.dtype == np.uint8:
            hist = np.bincount(lab.reshape(-1), minlength=256)
            moving = int(hist[ids].sum())
        else:
            moving = int(np.isin(lab, ids).sum())
        out[k] = (lab.size - moving) / (lab.shape[0] * lab.shape[1])
    return out


# ---------------------------------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------------------------------
def select_views(names, roi, static, roi_threshold, static_threshold, min_observation=-1, covisible=None, focal=None):
    """The reference's rules, as a pure function.  names [n]; roi / static: shares [n], or None to leave that rule out.
      * min_observation > 0 (dataset_filter_utils.py:137-155): keep the names in `covisible` (the images of
        dense/sparse_filtered_<n>/images.bin), and any other whose fx and fy (`focal` [n, 2]) BOTH exceed 2000;
      * drop where roi < roi_threshold (:179);
      * keep where static > static_threshold (:196), so a share equal to the threshold is dropped.
    The rules apply in that order and an image carries the reason of the first rule that rejects it.  Returns (kept names in the
    order given, {rejected name: reason})."""
    names = [str(n) for n in names]
    n = len(names)
    for what, arr in (("roi", roi), ("static", static)):
        if arr is not None and len(arr) != n:
            raise ValueError("select_views: %d %s shares for %d names" % (len(arr), what, n))
    reasons = {}
    if min_observation > 0:
        if covisible is None or focal is None:
            raise ValueError("select_views: min_observation > 0 needs the covisible names and the focal lengths")
        covisible = set(str(c) for c in covisible)
        focal = np.asarray(focal, dtype=np.float64).reshape(n, 2)
        for k, name in enumerate(names):
            if name not in covisible and not (focal[k, 0] > 2000 and focal[k, 1] > 2000):
                reasons[name] = REASON_COVIS
    if roi is not None:
        for k, name in enumerate(names):
            if name not in reasons and roi[k] < roi_threshold:
                reasons[name] = REASON_ROI
    if static is not None:
        for k, name in enumerate(names):
            if name not in reasons and not static[k] > static_threshold:
                reasons[name] = REASON_TRANSIENT
    return [name for name in names if name not in reasons], reasons


# ---------------------------------------------------------------------------------------------------
# the tsv
# ---------------------------------------------------------------------------------------------------
def write_split(root_dir, names, num_test, overwrite=False):
    """prepare_data_split.py:54-62 without pandas: <root_dir>/<dirname>.tsv with the header `filename id split dataset`, tab
    separated; id runs 0 .. n - 1, the first num_test rows are `test`, the rest `train`, dataset is the directory name.
    ValueError when fewer than num_test + 1 images remain (no training image).  Any existing *.tsv in root_dir is refused with
    FileExistsError unless overwrite (scripts/data_generation.sh only writes a split when there is none; the readers take the
    FIRST *.tsv by name).  Returns the path."""
    names = [str(n) for n in names]
    num_test = int(num_test)
    if num_test < 0:
        raise ValueError("write_split: num_test %d" % num_test)
    if len(names) < num_test + 1:
        raise ValueError("write_split: %d images remain, %d test images and at least one training image are needed"
                         % (len(names), num_test))
    for name in names:
        if any(ch in name for ch in "\t\n\r\""):
            raise ValueError("write_split: the file name %r cannot be written to a tsv row" % name)
    dataset = _scene_name(root_dir)
    path = os.path.join(root_dir, dataset + ".tsv")
    existing = sorted(glob.glob(os.path.join(root_dir, "*.tsv")))
    if existing and not overwrite:
        raise FileExistsError("%s already holds a split (%s): pass overwrite=True (--overwrite) to write %s"
                              % (root_dir, ", ".join(os.path.basename(e) for e in existing), os.path.basename(path)))
    with open(path, "w", newline="") as fh:
        fh.write("\t".join(TSV_COLUMNS) + "\n")
        for k, name in enumerate(names):
            fh.write("%s\t%d\t%s\t%s\n" % (name, k, "test" if k < num_test else "train", dataset))
    first = sorted(glob.glob(os.path.join(root_dir, "*.tsv")))[0]
    if first != path:
        print("note: %s sorts before %s: the readers take the first *.tsv by name" % (os.path.basename(first), os.path.basename(path)))
    return path


# ---------------------------------------------------------------------------------------------------
# the whole tool
# ---------------------------------------------------------------------------------------------------
def prepare_split(root_dir, num_test=10, min_observation=-1, roi_threshold=0.5, static_threshold=0.6,
                  semantic_map_path="semantic_maps", seed=0, device="cuda:0", sfm_path="sparse", overwrite=False, visualize=None):
    """tools/prepare_data/prepare_data_split.py: view selection (covisibility when min_observation > 0, then the ROI share of
    every registered image against the sphere of config.yaml: ONE `ncw_views_roi` launch), a permutation of the survivors, the
    transient filter on the permuted survivors, and the tsv.  Differences from the reference:
      * its permutation is unseeded; this one is np.random.default_rng(seed).permutation;
      * rejected images are not re-encoded into trash_images/: <root_dir>/split_report.json lists, per image, the ROI share,
        the static share (null where the transient filter did not see the image) and kept / reason;
      * images are opened for their header only.
    semantic_map_path None, or a directory that does not exist: the transient filter is skipped with a printed note.
    visualize: a directory that receives the ROI mask of every view the ROI rule rejected, as <stem>_roi.png.
    Returns a dict: tsv, report (paths), names (the rows), reasons, roi, static ({name: share})."""
    import yaml

    existing = sorted(glob.glob(os.path.join(root_dir, "*.tsv")))
    if existing and not overwrite:  # before any work: the refusal write_split would end with
        raise FileExistsError("%s already holds a split (%s): pass overwrite=True (--overwrite)"
                              % (root_dir, ", ".join(os.path.basename(e) for e in existing)))
    with open(os.path.join(root_dir, "config.yaml"), "r") as fh:
        cfg = yaml.safe_load(fh)
    cams = scene_cameras(root_dir, sfm_path)
    names = [c.name for c in cams]
    res = roi_shares(cams, cfg["origin"], cfg["radius"], device, with_mask=visualize is not None)
    roi, counts = res[0], res[1]
    covisible = None
    if min_observation > 0:
        fpath = os.path.join(root_dir, "dense", "sparse_filtered_%d" % min_observation, "images.bin")
        covisible = [im["name"] for im in colmap.read_images(fpath).values()]
    focal = np.array([[c.K[0, 0], c.K[1, 1]] for c in cams], dtype=np.float64)
    survivors, reasons = select_views(names, roi, None, roi_threshold, static_threshold, min_observation, covisible, focal)
    print("filter %d images in view selection (%d by covisibility, %d by ROI)"
          % (len(names) - len(survivors), sum(r == REASON_COVIS for r in reasons.values()), sum(r == REASON_ROI for r in reasons.values())))
    if visualize is not None:
        from . import views

        prefix = pixel_prefix(cams)
        for k, c in enumerate(cams):
            if reasons.get(c.name) == REASON_ROI:
                m = res[2][int(prefix[k]):int(prefix[k + 1])].reshape(c.height, c.width).cpu().numpy()
                views.write_png(os.path.join(visualize, c.name.split(".")[0] + "_roi.png"), np.repeat((m * 255)[:, :, None], 3, 2))
    order = np.random.default_rng(seed).permutation(len(survivors))
    survivors = [survivors[i] for i in order]
    static = {}
    if semantic_map_path is None or not os.path.isdir(os.path.join(root_dir, semantic_map_path)):
        print("note: no semantic maps (%s): the transient filter is skipped"
              % ("semantic_map_path is None" if semantic_map_path is None else os.path.join(root_dir, semantic_map_path) + " does not exist"))
        kept = survivors
    else:
        sh = static_shares(root_dir, semantic_map_path, survivors)
        static = {n: float(s) for n, s in zip(survivors, sh)}
        kept, late = select_views(survivors, None, sh, roi_threshold, static_threshold)
        reasons.update(late)
        print("filter %d images in transient filtering process" % len(late))
    tsv = write_split(root_dir, kept, num_test, overwrite)
    report = {"root_dir": _scene_name(root_dir), "num_test": int(num_test), "min_observation": int(min_observation),
              "roi_threshold": float(roi_threshold), "static_threshold": float(static_threshold), "seed": int(seed),
              "origin": [float(v) for v in cfg["origin"]], "radius": float(cfg["radius"]),
              "images": {n: {"roi_share": float(roi[k]), "roi_pixels": int(counts[k]), "width": cams[k].width, "height": cams[k].height,
                             "static_share": static.get(n), "kept": n not in reasons, "reason": reasons.get(n)}
                         for k, n in enumerate(names)}}
    rpath = os.path.join(root_dir, "split_report.json")
    with open(rpath, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    return {"tsv": tsv, "report": rpath, "names": kept, "reasons": reasons, "roi": {n: float(roi[k]) for k, n in enumerate(names)},
            "static": static}
