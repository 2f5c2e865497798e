"""Checking the alignment: the ground-truth reprojection error of SfM tracks (tools/reproj_error.py).

    rep = gt_reprojection_error("scene", "gt.ply", cfg["sfm2gt"], "dense/sparse", track_length=200)
    rep["mean_error"]          # pixels: small when sfm2gt is right

`eval_mesh`, the SfM crop and the reprojection filter all multiply by the scene's `sfm2gt`; this is the one tool that says whether
that matrix is right.  Per image it takes the mean reprojection error of the SfM observations (images above a threshold drop
out); per long, low-error track it takes the first observation as the reference view, projects the WHOLE ground-truth cloud into
that view, keeps the points that land on the observation's pixel, takes the nearest, reprojects it into every view of the track
and measures the pixel distance to the SfM key-point.  The mean of those distances is the answer.

The hot part -- whole cloud x every track -- is ONE pass over the cloud for all tracks (`ncw_pixel_nearest`, csrc/ncw_gtreproj.hip;
the reference makes about 15 torch ops over [2, N_gt, 4] tensors per PAIR of tracks); the per-observation errors and their sums are
one `ncw_reproj_errors` launch each for the image filter and for the answer.  numpy for the host logic, torch for device memory.
There is no CPU fallback.  Differences from the reference: INTEGRATION.md ("reproj_error.py").
"""
import ctypes as C
import os

import numpy as np

from . import colmap
from . import lib as L

NO_POINT = 0xFFFFFFFFFFFFFFFF  # ncw_pixel_nearest: no point hit the pixel
DEFAULT_CHUNK = 1 << 24        # cloud points per launch of the streamed pass (192 MB of float32 xyz)


# ---------------------------------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------------------------------
def read_scene(data_dir, reconstruct_path="dense/sparse"):
    """The COLMAP model <data_dir>/<reconstruct_path> as the tool needs it (reproj_error.py:147-157).  Returns a dict:
      images, cams        colmap.read_images(with_points=True) / colmap.read_cameras
      image_ids [n]       every registered image whose file exists in <data_dir>/dense/images, sorted by file name (the
                          reference sorts the directory and drops its first two entries; difference (b))
      names [n], wh [n,2], E float64 [n,4,4] (world -> camera, get_entrinsics), K float32 [n,3,3] (get_intrinsic)
      point_ids, xyz, error, track_len, track_start, track_image_id, track_point2d_idx   colmap.read_points3d(with_tracks=True)"""
    sp = os.path.join(data_dir, reconstruct_path)
    images = colmap.read_images(os.path.join(sp, "images.bin"), with_points=True)
    cams = colmap.read_cameras(os.path.join(sp, "cameras.bin"))
    ids, xyz, err, track, start, t_img, t_p2d = colmap.read_points3d(os.path.join(sp, "points3D.bin"), with_tracks=True)
    img_dir = os.path.join(data_dir, "dense", "images")
    files = set(os.listdir(img_dir)) if os.path.isdir(img_dir) else set()
    order = sorted((im["name"], iid) for iid, im in images.items() if im["name"] in files)
    if not order:
        raise FileNotFoundError("none of the %d images registered in %s has its file in %s" % (len(images), sp, img_dir))
    image_ids = [iid for _, iid in order]
    n = len(image_ids)
    E = np.zeros((n, 4, 4), dtype=np.float64)
    K = np.zeros((n, 3, 3), dtype=np.float32)
    wh = np.zeros((n, 2), dtype=np.int64)
    for k, iid in enumerate(image_ids):
        im = images[iid]
        cam = cams[im["camera_id"]]
        E[k, :3, :3], E[k, :3, 3], E[k, 3, 3] = colmap.qvec2rotmat(im["qvec"]), im["tvec"], 1.0
        p = cam["params"]
        K[k, 0, 0], K[k, 1, 1], K[k, 0, 2], K[k, 1, 2], K[k, 2, 2] = p[0], p[1], p[2], p[3], 1
        wh[k] = cam["width"], cam["height"]
    return {"images": images, "cams": cams, "image_ids": image_ids, "names": [nm for nm, _ in order], "wh": wh, "E": E, "K": K,
            "point_ids": ids, "xyz": xyz, "error": err, "track_len": track, "track_start": start, "track_image_id": t_img,
            "track_point2d_idx": t_p2d}


def _device(device, what):
    import torch

    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise L.NeuconwHipError("gtreproj.%s: device %s is not a GPU; there is no CPU fallback" % (what, device))
    return device


# ---------------------------------------------------------------------------------------------------
# per-observation reprojection errors and their per-segment sums: one launch
# ---------------------------------------------------------------------------------------------------
def reproj_errors(proj, xyz, cam_idx, pt_idx, xy, seg_start, device="cuda:0"):
    """One `ncw_reproj_errors` launch.  proj [n_cams,3,4], xyz [n_pts,3], xy [n_obs,2] (cast to float32), cam_idx / pt_idx
    [n_obs] (int32), seg_start [n_seg + 1] (int64).  Returns (err float32 [n_obs], seg_sum float64 [n_seg]) as numpy."""
    import torch

    device = _device(device, "reproj_errors")
    proj = np.ascontiguousarray(proj, dtype=np.float32).reshape(-1, 12)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    cam_idx = np.ascontiguousarray(cam_idx, dtype=np.int32).reshape(-1)
    pt_idx = np.ascontiguousarray(pt_idx, dtype=np.int32).reshape(-1)
    seg_start = np.ascontiguousarray(seg_start, dtype=np.int64).reshape(-1)
    n_obs, n_seg = len(cam_idx), len(seg_start) - 1
    if len(pt_idx) != n_obs or len(xy) != n_obs or n_seg < 0:
        raise ValueError("reproj_errors: %d cameras, %d points, %d key-points, %d segment bounds" % (n_obs, len(pt_idx), len(xy), n_seg + 1))
    if n_seg == 0 or n_obs == 0:
        return np.zeros(n_obs, dtype=np.float32), np.zeros(max(n_seg, 0), dtype=np.float64)
    if seg_start[0] != 0 or seg_start[-1] != n_obs or (np.diff(seg_start) < 0).any():
        raise ValueError("reproj_errors: the segments do not tile the %d observations" % n_obs)
    d = [torch.from_numpy(a).to(device) for a in (proj, xyz, cam_idx, pt_idx, xy, seg_start)]
    err = torch.empty(n_obs, device=device, dtype=torch.float32)
    seg_sum = torch.empty(n_seg, device=device, dtype=torch.float64)
    with torch.cuda.device(device):
        L.check(L.get_lib().ncw_reproj_errors(L.ptr(d[0]), len(proj), L.ptr(d[1]), len(xyz), L.ptr(d[2]), L.ptr(d[3]), L.ptr(d[4]), n_obs,
                                              L.ptr(d[5]), n_seg, L.ptr(err), L.ptr(seg_sum), L.stream_ptr(device)), "ncw_reproj_errors")
    return err.cpu().numpy(), seg_sum.cpu().numpy()


def image_observations(scene, reference_unmatched=False):
    """The observations the per-image error is taken over, as the arrays of one launch: (proj float32 [n,3,4] = K [R|t] formed in
    float64, xyz float32 [N,3] (file order), cam_idx, pt_idx, xy float64 [n_obs,2], seg_start [n + 1]).  Default: the key-points
    that have a 3-D point.  reference_unmatched: ALL key-points, one without a 3-D point measured against the point of the
    highest id (reproj_error.py:130 indexes its table with -1, which torch reads as the last row; difference (a))."""
    ids = scene["point_ids"]
    order = np.argsort(ids, kind="stable")
    last = int(order[-1]) if len(ids) else 0
    proj = (scene["K"].astype(np.float64) @ scene["E"][:, :3, :]).astype(np.float32)
    cam_idx, pt_idx, xy, seg = [], [], [], [0]
    for k, iid in enumerate(scene["image_ids"]):
        im = scene["images"][iid]
        p3 = im["point3d_ids"]
        has = p3 >= 0
        pos = np.searchsorted(ids[order], np.where(has, p3, ids[order[0]] if len(ids) else 0))
        pos = np.minimum(pos, len(ids) - 1)
        if not (ids[order][pos][has] == p3[has]).all():
            raise ValueError("image %r observes a 3-D point that points3D.bin does not hold" % im["name"])
        row = np.where(has, order[pos], last)
        keep = np.ones(len(p3), dtype=bool) if reference_unmatched else has
        cam_idx.append(np.full(int(keep.sum()), k, dtype=np.int32))
        pt_idx.append(row[keep].astype(np.int32))
        xy.append(im["xys"][keep])
        seg.append(seg[-1] + int(keep.sum()))
    return (proj, scene["xyz"].astype(np.float32), np.concatenate(cam_idx), np.concatenate(pt_idx),
            np.concatenate(xy).reshape(-1, 2), np.array(seg, dtype=np.int64))


def image_errors(scene, device="cuda:0", reference_unmatched=False):
    """reproj_error.py:120-138 (`image_reproj_error`) for every image of the scene in ONE `ncw_reproj_errors` launch: float64 [n]
    = the mean reprojection error of each image's observations (NaN for an image without one, which is then not kept)."""
    proj, xyz, cam_idx, pt_idx, xy, seg = image_observations(scene, reference_unmatched)
    _, seg_sum = reproj_errors(proj, xyz, cam_idx, pt_idx, xy, seg, device)
    count = np.diff(seg).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(count > 0, seg_sum / count, np.nan)


# ---------------------------------------------------------------------------------------------------
# the tracks
# ---------------------------------------------------------------------------------------------------
def select_tracks(scene, kept_image_ids, track_length=200, reproj_error=0.4):
    """reproj_error.py:163-211 as a pure host function: a track is kept if it has MORE THAN track_length observations, its error
    is BELOW reproj_error and at least one observation lies in a kept image; only the observations in kept images count, in file
    order, and the first of them is the reference view.  Order: file order of points3D.bin.  Returns a dict: point_row [T]
    (index into the scene's point arrays), point_id [T], seg_start [T + 1], obs_image_id / obs_point2d_idx [n], obs_xy float64
    [n,2]; the reference observation of track t is element seg_start[t]."""
    kept = np.zeros(int(max(scene["images"]) + 1) if scene["images"] else 1, dtype=bool)
    kept[np.asarray(list(kept_image_ids), dtype=np.int64)] = True
    start, t_img, t_p2d = scene["track_start"], scene["track_image_id"], scene["track_point2d_idx"]
    rows, seg, o_img, o_p2d, o_xy = [], [0], [], [], []
    for i in np.flatnonzero((scene["track_len"] > track_length) & (scene["error"] < reproj_error)):
        a, b = int(start[i]), int(start[i + 1])
        img = t_img[a:b]
        ok = (img >= 0) & (img < len(kept))
        ok[ok] = kept[img[ok]]
        if not ok.any():
            continue
        rows.append(int(i))
        o_img.append(img[ok])
        o_p2d.append(t_p2d[a:b][ok])
        o_xy.append(np.stack([scene["images"][int(g)]["xys"][int(p)] for g, p in zip(o_img[-1], o_p2d[-1])]))
        seg.append(seg[-1] + int(ok.sum()))
    rows = np.array(rows, dtype=np.int64)
    def cat(xs, dt, shape):
        return np.concatenate(xs).astype(dt).reshape(shape) if xs else np.zeros([0 if d < 0 else d for d in shape], dtype=dt)

    return {"point_row": rows, "point_id": scene["point_ids"][rows], "seg_start": np.array(seg, dtype=np.int64),
            "obs_image_id": cat(o_img, np.int32, (-1,)), "obs_point2d_idx": cat(o_p2d, np.int32, (-1,)),
            "obs_xy": cat(o_xy, np.float64, (-1, 2))}


# ---------------------------------------------------------------------------------------------------
# nearest ground-truth point on a pixel: one pass over the cloud for all queries
# ---------------------------------------------------------------------------------------------------
def cloud_centre(cloud):
    """Centre of the cloud's box, float64 [3] (evalmesh.recentre's idea: coordinates are moved there in float64 BEFORE they
    become float32, so that float32 spends its bits on the scene and not on its distance from the origin)."""
    cloud = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    return (cloud.min(0) + cloud.max(0)) / 2.0


def query_table(w2c, intr, xy, centre):
    """The NcwPixelQuery table (float32) of views w2c float64 [Q,3,4] (cloud coordinates -> camera), intr [Q,4] = fx, fy, cx, cy,
    key-points xy [Q,2], for a cloud recentred by `centre`: the shift is folded into each translation in float64,
    t' = W[:, :3] centre + W[:, 3].  Returns a numpy structured array that mirrors the struct."""
    w2c = np.asarray(w2c, dtype=np.float64).reshape(-1, 3, 4).copy()
    w2c[:, :, 3] += w2c[:, :, :3] @ np.asarray(centre, dtype=np.float64)
    q = np.zeros(len(w2c), dtype=np.dtype([("w2c", "<f4", 12), ("intr", "<f4", 4), ("xy", "<f4", 2)]))
    assert q.dtype.itemsize == C.sizeof(L.NcwPixelQuery)
    q["w2c"], q["intr"], q["xy"] = w2c.reshape(-1, 12), np.asarray(intr).reshape(-1, 4), np.asarray(xy).reshape(-1, 2)
    return q


def nearest_on_pixel(w2c, intr, xy, cloud, chunk=None, device="cuda:0", centre=None):
    """reproj_error.py:21-51 (`get_gt_point`) for all queries: index int64 [Q] of the cloud point nearest to the camera among
    those that project onto pixel round(xy) of the view, -1 where none does, and its depth float32 [Q].  cloud: float64 numpy
    [N,3]; it is recentred in float64, cast to float32 and streamed through `ncw_pixel_nearest` `chunk` points at a time (the
    result does not depend on the chunk size, bit for bit, so a cloud larger than the device goes through in pieces)."""
    import torch

    device = _device(device, "nearest_on_pixel")
    cloud = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    n = len(cloud)
    if n > 0xFFFFFFFE:
        raise ValueError("nearest_on_pixel: %d points; the key holds a 32-bit index" % n)
    centre = cloud_centre(cloud) if centre is None else np.asarray(centre, dtype=np.float64)
    table = query_table(w2c, intr, xy, centre)
    nq = len(table)
    if nq == 0 or n == 0:
        return np.full(nq, -1, dtype=np.int64), np.full(nq, np.inf, dtype=np.float32)
    chunk = DEFAULT_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("nearest_on_pixel: chunk %d" % chunk)
    q_d = torch.frombuffer(bytearray(table.tobytes()), dtype=torch.uint8).to(device)
    best = torch.empty(nq, device=device, dtype=torch.int64)
    lib = L.get_lib()
    with torch.cuda.device(device):
        for p0 in range(0, n, chunk):  # the first launch clears `best`, the others go on from it
            pts = torch.from_numpy((cloud[p0:p0 + chunk] - centre).astype(np.float32)).to(device)
            L.check(lib.ncw_pixel_nearest(L.ptr(q_d), nq, L.ptr(pts), p0, len(pts), int(p0 == 0), L.ptr(best), L.stream_ptr(device)),
                    "ncw_pixel_nearest")
    keys = best.cpu().numpy().view(np.uint64)
    return split_keys(keys)


def split_keys(keys):
    """(index int64, -1 for all-ones; depth float32) of ncw_pixel_nearest's keys."""
    keys = np.asarray(keys, dtype=np.uint64)
    none = keys == np.uint64(NO_POINT)
    idx = np.where(none, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64))
    depth = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, np.where(none, np.float32(np.inf), depth).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# the whole tool
# ---------------------------------------------------------------------------------------------------
def gt_reprojection_error(data_dir, gt_pcd_path, sfm_to_gt, reconstruct_path="dense/sparse", track_length=200, reproj_error=0.4,
                          img_reproj_error=300, batch_size=None, reference_unmatched=False, chunk=None, device="cuda:0",
                          gt_points=None):
    """tools/reproj_error.py `gt_reproject_error`.  gt_points: the ground-truth cloud as float64 [N,3] instead of the PLY at
    gt_pcd_path.  batch_size is accepted and ignored (all tracks go through one pass).  Returns the report, a dict:
      mean_error                          the answer, pixels (float; NaN when no element is left)
      errors float32 [n]                  per track element, tracks in file order, elements in track order
      element_image_id [n], seg_start [T + 1], track_point_id [T]
      image_names, image_ids, image_wh, image_error float64    per image of the scene (mean error of its observations), image_kept bool
      n_images, n_images_kept, n_tracks_selected, n_tracks, n_tracks_no_gt
      gt_index int64 [T]                  the chosen point of the cloud per kept track;  gt_points float64 [T,3]
      sfm_points float64 [T,3]            the tracks' SfM points;  gt_points_sfm: gt_points moved by inv(sfm_to_gt)
      no_gt_point_id                      the tracks dropped because no ground-truth point hits their reference pixel
      element_xy, element_proj, centre    per element the key-point and K [R|t] into its view for points given relative to `centre`"""
    from . import ply

    sfm_to_gt = np.asarray(sfm_to_gt, dtype=np.float64).reshape(4, 4)
    gt_to_sfm = np.linalg.inv(sfm_to_gt)
    scene = read_scene(data_dir, reconstruct_path)
    cloud = ply.read_points(gt_pcd_path, weld=False) if gt_points is None else np.asarray(gt_points, dtype=np.float64).reshape(-1, 3)
    if len(cloud) == 0:
        raise ValueError("the ground-truth cloud is empty")
    img_err = image_errors(scene, device, reference_unmatched)
    kept = img_err < img_reproj_error
    kept_ids = [iid for iid, k in zip(scene["image_ids"], kept) if k]
    print("selected %d view for testing." % len(kept_ids))
    tr = select_tracks(scene, kept_ids, track_length, reproj_error)
    seg = tr["seg_start"]
    n_sel = len(tr["point_row"])
    index_of = {iid: k for k, iid in enumerate(scene["image_ids"])}
    obs_cam = np.array([index_of[int(g)] for g in tr["obs_image_id"]], dtype=np.int64)
    w2c_gt = scene["E"] @ gt_to_sfm  # ground-truth coordinates -> camera (SfM units), float64 [n,4,4]
    centre = cloud_centre(cloud)
    ref = seg[:-1]
    intr = np.stack([scene["K"][:, 0, 0], scene["K"][:, 1, 1], scene["K"][:, 0, 2], scene["K"][:, 1, 2]], -1)
    if n_sel:
        gt_index, _ = nearest_on_pixel(w2c_gt[obs_cam[ref], :3, :], intr[obs_cam[ref]], tr["obs_xy"][ref], cloud, chunk, device, centre)
    else:
        gt_index = np.zeros(0, dtype=np.int64)
    hit = gt_index >= 0
    # the tracks whose reference pixel a ground-truth point hits; the others are dropped and counted (difference (c))
    t_of_obs = np.repeat(np.arange(n_sel), np.diff(seg))
    obs_keep = hit[t_of_obs] if n_sel else np.zeros(0, dtype=bool)
    new_t = np.cumsum(hit) - 1
    seg_kept = np.concatenate([[0], np.cumsum(np.diff(seg)[hit])]).astype(np.int64)
    gt_pts = cloud[gt_index[hit]]
    proj = scene["K"].astype(np.float64) @ w2c_gt[:, :3, :]
    proj[:, :, 3] += proj[:, :, :3] @ centre
    err, seg_sum = reproj_errors(proj, gt_pts - centre, obs_cam[obs_keep], new_t[t_of_obs[obs_keep]] if n_sel else [], tr["obs_xy"][obs_keep],
                                 seg_kept, device)
    n = len(err)
    mean = float(np.sum(seg_sum) / n) if n else float("nan")
    print("avg re-projection error %s, %d/%d" % (mean, n, n))
    return {"mean_error": mean, "errors": err, "element_image_id": tr["obs_image_id"][obs_keep], "element_xy": tr["obs_xy"][obs_keep],
            "seg_start": seg_kept, "track_point_id": tr["point_id"][hit], "image_names": list(scene["names"]), "image_error": img_err,
            "image_kept": kept, "n_images": len(kept), "n_images_kept": int(kept.sum()), "n_tracks_selected": int(n_sel),
            "n_tracks": int(hit.sum()), "n_tracks_no_gt": int((~hit).sum()), "no_gt_point_id": tr["point_id"][~hit],
            "gt_index": gt_index[hit], "gt_points": gt_pts, "sfm_points": scene["xyz"][tr["point_row"][hit]],
            "gt_points_sfm": gt_pts @ gt_to_sfm[:3, :3].T + gt_to_sfm[:3, 3], "element_proj": proj[obs_cam[obs_keep]], "centre": centre, "image_ids": list(scene["image_ids"]), "image_wh": scene["wh"]}


def write_outputs(report, out_dir, visualize=False):
    """report.json, colmap_sfm.ply and gt.ply (reproj_error.py:223-231: the tracks' SfM points, and the
    chosen ground-truth points in SfM coordinates, row for row), and with visualize one PNG per image under reprojects/ (:93-118:
    black, the reprojected ground-truth points green, the SfM key-points red on top).  Returns the path of report.json."""
    import json

    from . import ply, views

    os.makedirs(out_dir, exist_ok=True)
    ply.write(os.path.join(out_dir, "colmap_sfm.ply"), report["sfm_points"])
    ply.write(os.path.join(out_dir, "gt.ply"), report["gt_points_sfm"])
    nan = lambda v: None if v != v else float(v)  # noqa: E731
    doc = {"mean_error": nan(report["mean_error"]), "n_elements": int(len(report["errors"])),
           **{k: int(report[k]) for k in ("n_images", "n_images_kept", "n_tracks_selected", "n_tracks", "n_tracks_no_gt")},
           "images": {n: {"error": nan(e), "kept": bool(k)} for n, e, k in zip(report["image_names"], report["image_error"], report["image_kept"])},
           "track_point_id": [int(v) for v in report["track_point_id"]], "no_gt_point_id": [int(v) for v in report["no_gt_point_id"]],
           "seg_start": [int(v) for v in report["seg_start"]], "gt_index": [int(v) for v in report["gt_index"]],
           "element_image_id": [int(v) for v in report["element_image_id"]], "errors": [nan(v) for v in report["errors"]]}
    path = os.path.join(out_dir, "report.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    if visualize:
        t_of = np.repeat(np.arange(len(report["seg_start"]) - 1), np.diff(report["seg_start"]))
        h = np.einsum("nij,nj->ni", report["element_proj"][:, :, :3], (report["gt_points"] - report["centre"])[t_of]) + report["element_proj"][:, :, 3]
        gt2d = h[:, :2] / h[:, 2:3]
        for k, iid in enumerate(report["image_ids"]):
            m = report["element_image_id"] == iid
            if not m.any():
                continue
            w, hh = [int(v) for v in report["image_wh"][k]]
            img = np.zeros((hh, w, 3), dtype=np.uint8)
            for pts, colour in ((gt2d[m], (0, 255, 0)), (report["element_xy"][m], (255, 0, 0))):
                px = np.clip(np.nan_to_num(pts, nan=0.0, posinf=1e9, neginf=-1e9).astype(np.int64), 0, [w - 1, hh - 1])
                img[px[:, 1], px[:, 0]] = colour
            views.write_png(os.path.join(out_dir, "reprojects", report["image_names"][k] + ".png"), img)
    return path

