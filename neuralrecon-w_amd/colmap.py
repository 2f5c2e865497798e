"""The scene files every tool at the edge of the renderer reads: a COLMAP binary model (cameras.bin, images.bin, points3D.bin;
utils/colmap_utils.py) and the tsv split file of a scene directory.  One parser per format; numpy and the standard library only,
so that reading a scene needs neither torch nor the HIP library.
"""
import csv
import glob
import os
import struct

import numpy as np

# COLMAP camera models: id -> (name, number of parameters)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
PINHOLE = 1


def read_cameras(path):
    """COLMAP cameras.bin: {camera_id: dict(id, model, width, height, params float64)}.  Layout (little-endian): uint64
    count, then per camera int32 id, int32 model id, uint64 width, uint64 height, float64 params[n(model)].  Only PINHOLE
    cameras (fx, fy, cx, cy) are accepted: any other model is refused with a ValueError (the reference would read the
    first four parameters of any model as fx, fy, cx, cy)."""
    cams = {}
    with open(path, "rb") as fh:
        (n,) = struct.unpack("<Q", fh.read(8))
        for _ in range(n):
            cid, model, width, height = struct.unpack("<iiQQ", fh.read(24))
            if model != PINHOLE:
                name = CAMERA_MODELS.get(model, ("unknown model id %d" % model,))[0]
                raise ValueError("%s: camera %d is %s; only PINHOLE cameras (undistorted images) are supported" % (path, cid, name))
            params = np.frombuffer(fh.read(8 * 4), dtype="<f8").astype(np.float64)
            cams[cid] = {"id": cid, "model": model, "width": int(width), "height": int(height), "params": params}
    return cams


def read_images(path, with_points=False):
    """COLMAP images.bin: {image_id: dict(id, qvec, tvec, camera_id, name)}, file order.  Layout: uint64 count, then per image
    int32 id, float64 qvec[4] (w, x, y, z), float64 tvec[3], int32 camera id, the name as NUL-terminated UTF-8 bytes, uint64 n2d,
    n2d x (float64 x, float64 y, int64 point3D id; -1 = no 3-D point).  with_points: every dict also carries the 2-D points,
    `xys` float64 [n2d, 2] and `point3d_ids` int64 [n2d] (utils/colmap_utils.py:214-247).  A file that ends early or goes on after
    its last image is refused with a ValueError."""
    with open(path, "rb") as fh:
        buf = fh.read()
    (n,) = struct.unpack_from("<Q", buf, 0)

    def short(k):
        return ValueError("%s: the file ends inside image %d of %d (not a COLMAP images.bin?)" % (path, k + 1, n))

    pt = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
    imgs = {}
    off = 8
    for k in range(n):
        try:
            rec = struct.unpack_from("<i7di", buf, off)
            end = buf.index(b"\x00", off + 64)
            (n2d,) = struct.unpack_from("<Q", buf, end + 1)
        except (struct.error, ValueError):
            raise short(k) from None
        name = buf[off + 64:end].decode("utf-8")
        off = end + 9
        if off + 24 * n2d > len(buf):
            raise short(k)
        im = {"id": rec[0], "qvec": np.array(rec[1:5]), "tvec": np.array(rec[5:8]), "camera_id": rec[8], "name": name}
        if with_points:
            pts = np.frombuffer(buf, dtype=pt, count=n2d, offset=off)
            im["xys"] = np.stack([pts["x"], pts["y"]], -1).astype(np.float64).reshape(-1, 2)
            im["point3d_ids"] = pts["id"].astype(np.int64)
        imgs[rec[0]] = im
        off += 24 * n2d
    if off != len(buf):
        raise ValueError("%s: %d trailing bytes after %d images (not a COLMAP images.bin?)" % (path, len(buf) - off, n))
    return imgs


def read_points3d(path, with_tracks=False):
    """COLMAP points3D.bin (utils/colmap_utils.py:264-291: uint64 count, then per point `<QdddBBBd` + uint64 track length + that
    many `<ii` track elements) -> (ids int64 [N], xyz float64 [N,3], reprojection error float64 [N], track length int64 [N]),
    file order.  The one walk of the file: voxel.read_points3d_xyz, evalmesh.read_points3d_filtered and
    cachebuild.read_points3d_table are views of what it returns.  with_tracks: the tuple also carries the track elements as CSR
    arrays, (.., track_start int64 [N + 1], track_image_id int32 [T], track_point2d_idx int32 [T]): the elements of point i are
    track_start[i] .. track_start[i + 1] - 1, in file order (gtreproj.select_tracks)."""
    with open(path, "rb") as fh:
        buf = fh.read()
    (n,) = struct.unpack_from("<Q", buf, 0)
    off = 8
    ids = np.empty(n, dtype=np.int64)
    xyz = np.empty((n, 3), dtype=np.float64)
    err = np.empty(n, dtype=np.float64)
    track = np.empty(n, dtype=np.int64)
    elems = []
    for i in range(n):
        ids[i], xyz[i, 0], xyz[i, 1], xyz[i, 2] = struct.unpack_from("<Qddd", buf, off)
        (err[i],) = struct.unpack_from("<d", buf, off + 35)
        (track[i],) = struct.unpack_from("<Q", buf, off + 43)
        elems.append((off + 51, 2 * int(track[i])))
        off += 51 + 8 * int(track[i])
    if off != len(buf):
        raise ValueError("%s: %d trailing bytes after %d points (not a COLMAP points3D.bin?)" % (path, len(buf) - off, n))
    if not with_tracks:
        return ids, xyz, err, track
    flat = np.concatenate([np.frombuffer(buf, dtype="<i4", count=c, offset=o) for o, c in elems] + [np.empty(0, dtype="<i4")])
    flat = flat.astype(np.int32).reshape(-1, 2)
    start = np.concatenate([[0], np.cumsum(track)]).astype(np.int64)
    return ids, xyz, err, track, start, np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])


# ---------------------------------------------------------------------------------------------------
# writers: exactly the layouts the three readers document (synth.py writes its scenes with them)
# ---------------------------------------------------------------------------------------------------
def write_cameras(path, cams):
    """cameras.bin from {camera_id: dict(model, width, height, params)} or an iterable of such dicts carrying `id`, in the order
    given.  Only PINHOLE (model id 1, four parameters fx, fy, cx, cy) is written: anything else is a ValueError."""
    items = [(int(k), c) for k, c in cams.items()] if isinstance(cams, dict) else [(int(c["id"]), c) for c in cams]
    out = [struct.pack("<Q", len(items))]
    for cid, c in items:
        params = np.asarray(c["params"], dtype=np.float64).reshape(-1)
        if int(c.get("model", PINHOLE)) != PINHOLE or params.size != 4:
            raise ValueError("write_cameras: camera %d is not PINHOLE (model id %r, %d parameters)"
                             % (cid, c.get("model", PINHOLE), params.size))
        out.append(struct.pack("<iiQQ", cid, PINHOLE, int(c["width"]), int(c["height"])) + params.astype("<f8").tobytes())
    with open(path, "wb") as fh:
        fh.write(b"".join(out))


def write_images(path, images):
    """images.bin from {image_id: dict(qvec, tvec, camera_id, name[, xys, point3d_ids])} or an iterable of such dicts carrying
    `id`, in the order given.  Without `xys` an image has no 2-D point.  A name that holds NUL (the terminator of the name
    field) and xys / point3d_ids of different lengths are ValueErrors."""
    items = [(int(k), im) for k, im in images.items()] if isinstance(images, dict) else [(int(im["id"]), im) for im in images]
    pt = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
    out = [struct.pack("<Q", len(items))]
    for iid, im in items:
        name = str(im["name"]).encode("utf-8")
        if b"\x00" in name:
            raise ValueError("write_images: the name of image %d holds NUL, which ends the name field" % iid)
        xys = np.asarray(im.get("xys", np.empty((0, 2))), dtype=np.float64).reshape(-1, 2)
        ids = np.asarray(im.get("point3d_ids", np.full(len(xys), -1)), dtype=np.int64).reshape(-1)
        if len(ids) != len(xys):
            raise ValueError("write_images: image %d has %d 2-D points and %d point3D ids" % (iid, len(xys), len(ids)))
        q, t = np.asarray(im["qvec"], dtype=np.float64).reshape(4), np.asarray(im["tvec"], dtype=np.float64).reshape(3)
        rec = np.empty(len(xys), dtype=pt)
        rec["x"], rec["y"], rec["id"] = xys[:, 0], xys[:, 1], ids
        out.append(struct.pack("<i7di", iid, *q, *t, int(im["camera_id"])) + name + b"\x00" + struct.pack("<Q", len(xys))
                   + rec.tobytes())
    with open(path, "wb") as fh:
        fh.write(b"".join(out))


def write_points3d(path, ids, xyz, rgb, err, track_start, track_image_id, track_point2d_idx):
    """points3D.bin from the arrays `read_points3d(.., with_tracks=True)` returns plus the colours: ids [N], xyz [N, 3], rgb uint8
    [N, 3], err [N], and the tracks as CSR arrays (track_start [N + 1], track_image_id [T], track_point2d_idx [T]).  Arrays whose
    lengths disagree (N, or T against track_start[-1]) are a ValueError."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    n = len(ids)
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    err = np.asarray(err, dtype=np.float64).reshape(-1)
    start = np.asarray(track_start, dtype=np.int64).reshape(-1)
    t_img = np.asarray(track_image_id, dtype=np.int32).reshape(-1)
    t_idx = np.asarray(track_point2d_idx, dtype=np.int32).reshape(-1)
    if not (len(xyz) == len(rgb) == len(err) == n and len(start) == n + 1):
        raise ValueError("write_points3d: %d ids, %d xyz, %d rgb, %d err, %d track_start (N + 1 expected)"
                         % (n, len(xyz), len(rgb), len(err), len(start)))
    if len(t_img) != len(t_idx) or int(start[0]) != 0 or int(start[-1]) != len(t_img) or (np.diff(start) < 0).any():
        raise ValueError("write_points3d: %d track image ids, %d 2-D point indices, track_start runs %d .. %d"
                         % (len(t_img), len(t_idx), int(start[0]), int(start[-1])))
    elems = np.stack([t_img, t_idx], -1).astype("<i4")
    out = [struct.pack("<Q", n)]
    for i in range(n):
        a, b = int(start[i]), int(start[i + 1])
        out.append(struct.pack("<QdddBBBdQ", int(ids[i]), *xyz[i], *rgb[i], err[i], b - a) + elems[a:b].tobytes())
    with open(path, "wb") as fh:
        fh.write(b"".join(out))


def rotmat2qvec(R):
    """The unit quaternion (w, x, y, z), w >= 0, of a rotation matrix: the inverse of `qvec2rotmat` (the largest of the four
    candidate divisors, so that no case divides by a small number)."""
    R = np.asarray(R, dtype=np.float64)
    t = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
                  1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(t))
    s = 2 * np.sqrt(t[k])
    q = [np.array([s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]),
         np.array([(R[2, 1] - R[1, 2]) / s, s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]),
         np.array([(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s]),
         np.array([(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4])][k]
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def qvec2rotmat(q):
    """Rotation of the unit quaternion (w, x, y, z) (COLMAP's convention: world -> camera)."""
    w, x, y, z = [float(v) for v in q]
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def split_rows(root_dir):
    """(path, rows) of the scene's split file: the first <root_dir>/*.tsv sorted by name and its rows as dicts, file order.
    FileNotFoundError without one.  Which rows count is the caller's rule (reproj.read_train_split, views.read_scene)."""
    tsvs = sorted(glob.glob(os.path.join(root_dir, "*.tsv")))
    if not tsvs:
        raise FileNotFoundError("no *.tsv split file in %s" % root_dir)
    with open(tsvs[0], newline="") as fh:
        return tsvs[0], list(csv.DictReader(fh, delimiter="\t"))
