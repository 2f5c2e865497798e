"""CPU: the scene-file readers and the PLY writer (neuralrecon_w_amd.colmap, neuralrecon_w_amd.ply) against files built by hand
with struct.pack and literal header text -- never by the writer under test."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests._util import ROOT

from neuralrecon_w_amd import cachebuild, colmap, evalmesh, ply, voxel


# ---------------------------------------------------------------------------------------------------
# points3D.bin
# ---------------------------------------------------------------------------------------------------
# id, xyz, rgb, error, track length: ids unsorted and with gaps
POINTS = [(9, (1.5, -2.25, 3.0), (1, 2, 3), 0.5, 0), (2, (0.1, 0.2, 0.3), (4, 5, 6), 1.75, 1), (14, (-7.0, 8.0, 9.5), (7, 8, 9), 0.25, 3),
          (5, (4.0, 5.0, 6.0), (0, 0, 0), 3.0, 0), (11, (1e-3, 2e3, -3.5), (255, 254, 253), 1.0, 7)]


def _points3d_bytes():
    out = struct.pack("<Q", len(POINTS))
    for pid, xyz, rgb, err, track in POINTS:
        out += struct.pack("<QdddBBBd", pid, *xyz, *rgb, err) + struct.pack("<Q", track)
        for k in range(track):
            out += struct.pack("<ii", 100 + k, 7 * k)
    return out


@pytest.fixture()
def points3d(tmp_path):
    p = tmp_path / "points3D.bin"
    p.write_bytes(_points3d_bytes())
    return str(p)


def test_read_points3d_is_the_hand_packed_file(points3d):
    ids, xyz, err, track = colmap.read_points3d(points3d)
    assert (ids.dtype, xyz.dtype, err.dtype, track.dtype) == (np.int64, np.float64, np.float64, np.int64)
    assert ids.tolist() == [p[0] for p in POINTS] and track.tolist() == [p[4] for p in POINTS]
    assert xyz.shape == (5, 3) and xyz.tolist() == [list(p[1]) for p in POINTS]
    assert err.tolist() == [p[3] for p in POINTS]


def test_the_three_views_of_points3d(points3d, tmp_path):
    all_xyz = np.array([p[1] for p in POINTS])
    # voxel: track > min_track_length
    assert np.array_equal(voxel.read_points3d_xyz(points3d, 0), all_xyz[[1, 2, 4]])
    assert np.array_equal(voxel.read_points3d_xyz(points3d, 3), all_xyz[[4]])
    assert voxel.read_points3d_xyz(points3d, 7).shape == (0, 3)
    # evalmesh: track > L and err < E, the optional transform, a directory as path
    assert np.array_equal(evalmesh.read_points3d_filtered(points3d, 0, 1.5), all_xyz[[2, 4]])
    assert np.array_equal(evalmesh.read_points3d_filtered(str(tmp_path), 0, 1.0), all_xyz[[2]])  # err < E is strict
    T = np.array([[0.0, 2.0, 0.0, 1.0], [-2.0, 0.0, 0.0, 0.5], [0.0, 0.0, 2.0, -4.0], [0.0, 0.0, 0.0, 1.0]])
    want = np.array([[2 * y + 1.0, -2 * x + 0.5, 2 * z - 4.0] for x, y, z in all_xyz[[2, 4]]])
    assert np.array_equal(evalmesh.read_points3d_filtered(points3d, 0, 1.5, T), want)
    got = evalmesh.read_points3d_filtered(points3d, 7, 9.0)
    assert got.shape == (0, 3) and got.dtype == np.float64
    # cachebuild: float32 by id, ones for the ids the file does not list, max_id + 1 rows
    xyz_t, err_t = cachebuild.read_points3d_table(points3d)
    assert xyz_t.dtype == np.float32 and err_t.dtype == np.float32 and xyz_t.shape == (15, 3) and err_t.shape == (15,)
    want_xyz, want_err = np.ones((15, 3), dtype=np.float32), np.ones(15, dtype=np.float32)
    for pid, xyz, _, err, _ in POINTS:
        want_xyz[pid], want_err[pid] = np.array(xyz, dtype=np.float32), np.float32(err)
    assert np.array_equal(xyz_t, want_xyz) and np.array_equal(err_t, want_err)
    empty = tmp_path / "empty.bin"
    empty.write_bytes(struct.pack("<Q", 0))
    xyz_t, err_t = cachebuild.read_points3d_table(str(empty))
    assert xyz_t.tolist() == [[1.0, 1.0, 1.0]] and err_t.tolist() == [1.0]


def test_points3d_with_a_trailing_byte_is_refused(tmp_path):
    p = tmp_path / "points3D.bin"
    p.write_bytes(_points3d_bytes() + b"\x00")
    with pytest.raises(ValueError, match="1 trailing bytes after 5 points"):
        colmap.read_points3d(str(p))


# ---------------------------------------------------------------------------------------------------
# images.bin
# ---------------------------------------------------------------------------------------------------
# id, qvec, tvec, camera id, name, 2-D points (x, y, point3D id): file order is not id order
IMAGES = [(7, (0.5, -0.5, 0.5, 0.5), (1.0, 2.0, 3.0), 2, "b/second.jpg", [(10.5, 20.25, 9), (0.0, -1.5, -1), (640.0, 480.0, 14)]),
          (3, (1.0, 0.0, 0.0, 0.0), (-4.0, 5.5, 6.0), 1, "no_points.png", []),
          (12, (0.0, 0.6, 0.0, 0.8), (0.125, 0.25, 0.5), 2, "café_東京.jpg", [(3.5, 4.5, 2)])]


def _images_bytes():
    out = struct.pack("<Q", len(IMAGES))
    for iid, q, t, cam, name, pts in IMAGES:
        out += struct.pack("<i7di", iid, *q, *t, cam) + name.encode("utf-8") + b"\x00" + struct.pack("<Q", len(pts))
        for x, y, pid in pts:
            out += struct.pack("<ddq", x, y, pid)
    return out


def test_read_images_with_and_without_points(tmp_path):
    p = tmp_path / "images.bin"
    p.write_bytes(_images_bytes())
    plain, full = colmap.read_images(str(p)), colmap.read_images(str(p), with_points=True)
    assert list(plain) == list(full) == [7, 3, 12]  # file order
    for iid, q, t, cam, name, pts in IMAGES:
        for im in (plain[iid], full[iid]):
            assert im["id"] == iid and im["camera_id"] == cam and im["name"] == name
            assert im["qvec"].dtype == np.float64 and im["qvec"].tolist() == list(q) and im["tvec"].tolist() == list(t)
        assert set(plain[iid]) == {"id", "qvec", "tvec", "camera_id", "name"}
        assert set(full[iid]) == set(plain[iid]) | {"xys", "point3d_ids"}
        xys, ids = full[iid]["xys"], full[iid]["point3d_ids"]
        assert xys.dtype == np.float64 and xys.shape == (len(pts), 2) and xys.tolist() == [[x, y] for x, y, _ in pts]
        assert ids.dtype == np.int64 and ids.shape == (len(pts),) and ids.tolist() == [k for _, _, k in pts]


@pytest.mark.parametrize("with_points", [False, True])
@pytest.mark.parametrize("cut", [1, 24, 30, 70])  # inside the last 2-D point, at its start, inside the count, inside the name
def test_truncated_or_overlong_images_bin_is_refused(tmp_path, with_points, cut):
    data = _images_bytes()
    p = tmp_path / "images.bin"
    p.write_bytes(data[:-cut])
    with pytest.raises(ValueError, match="not a COLMAP images.bin"):
        colmap.read_images(str(p), with_points)
    p.write_bytes(data + b"\x00")
    with pytest.raises(ValueError, match="1 trailing bytes after 3 images"):
        colmap.read_images(str(p), with_points)


# ---------------------------------------------------------------------------------------------------
# PLY reading: 5 vertices (vertex 3 repeats vertex 0), a triangle and a quad
# ---------------------------------------------------------------------------------------------------
VERTS = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.5), (1.0, 1.0, -2.0), (0.0, 0.0, 0.0), (0.25, 1.0, 3.0)]
RGB = [(255, 0, 0), (0, 254, 0), (1, 2, 3), (9, 8, 7), (128, 64, 32)]
FACES = [(0, 1, 2), (1, 2, 4, 3)]
TRIANGLES = [[0, 1, 2], [1, 2, 4], [1, 4, 3]]  # the quad fanned (0, i, i + 1)
WELDED = [VERTS[i] for i in (0, 1, 2, 4)]


def _ply_bytes(fmt, colours, faces=True, extra=True, cut_faces=0):
    """The mesh as a PLY: `extra` puts a float property `quality` before x; coordinates are doubles, indices ints."""
    hdr = ["ply", "format %s 1.0" % fmt, "comment made by hand", "element vertex %d" % len(VERTS)]
    hdr += (["property float quality"] if extra else []) + ["property double x", "property double y", "property double z"]
    hdr += ["property uchar red", "property uchar green", "property uchar blue"] if colours else []
    hdr += ["element face %d" % len(FACES), "property list uchar int vertex_indices"] if faces else []
    out = ("\n".join(hdr + ["end_header"]) + "\n").encode("ascii")
    if fmt == "ascii":
        for k, v in enumerate(VERTS):
            row = (["0.5"] if extra else []) + [repr(c) for c in v] + ([str(c) for c in RGB[k]] if colours else [])
            out += (" ".join(row) + "\n").encode("ascii")
        for f in FACES if faces else []:
            out += (" ".join(str(c) for c in (len(f),) + f) + "\n").encode("ascii")
        return out
    bo = "<" if fmt == "binary_little_endian" else ">"
    for k, v in enumerate(VERTS):
        out += (struct.pack(bo + "f", 0.5) if extra else b"") + struct.pack(bo + "3d", *v)
        out += struct.pack("3B", *RGB[k]) if colours else b""
    body = b"".join(struct.pack(bo + "B%di" % len(f), len(f), *f) for f in FACES) if faces else b""
    return out + body[:len(body) - cut_faces]


@pytest.mark.parametrize("colours", [False, True])
@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_read_mesh_and_read_points_in_every_form(tmp_path, fmt, colours):
    p = str(tmp_path / "m.ply")
    with open(p, "wb") as fh:
        fh.write(_ply_bytes(fmt, colours))
    v, f, c = ply.read_mesh(p)
    assert v.dtype == np.float64 and v.tolist() == [list(x) for x in VERTS]
    assert f.dtype == np.int64 and f.tolist() == TRIANGLES
    if colours:
        assert c.dtype == np.uint8 and c.tolist() == [list(x) for x in RGB]
    else:
        assert c is None
    assert ply.read_points(p).tolist() == [list(x) for x in WELDED]           # a mesh: welded, first occurrence kept
    assert ply.read_points(p, weld=False).tolist() == [list(x) for x in VERTS]
    with open(p, "wb") as fh:
        fh.write(_ply_bytes(fmt, colours, faces=False))
    got = ply.read_points(p)
    assert got.dtype == np.float64 and got.tolist() == [list(x) for x in VERTS]  # a cloud: as stored
    assert ply.read_points(p, weld=True).tolist() == [list(x) for x in WELDED]
    v, f, c = ply.read_mesh(p)
    assert v.tolist() == [list(x) for x in VERTS] and f.shape == (0, 3) and f.dtype == np.int64


def test_read_points_never_walks_the_faces(tmp_path):
    """The face element is cut short after the vertex element: read_points does not notice, read_mesh does."""
    p = str(tmp_path / "cut.ply")
    with open(p, "wb") as fh:
        fh.write(_ply_bytes("binary_little_endian", True, cut_faces=9))
    assert ply.read_points(p).tolist() == [list(x) for x in WELDED]
    with pytest.raises(ValueError):
        ply.read_mesh(p)


def test_a_list_property_in_the_vertex_element_is_refused(tmp_path):
    p = str(tmp_path / "bad.ply")
    hdr = "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nproperty list uchar int n\nend_header\n"
    with open(p, "wb") as fh:
        fh.write(hdr.encode("ascii") + b"0 0 0 1 5\n")
    with pytest.raises(ValueError, match="list property in the vertex element"):
        ply.read_points(p)
    empty = str(tmp_path / "empty.ply")
    with open(empty, "wb") as fh:
        fh.write(b"ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    v, f, c = ply.read_mesh(empty)
    assert v.shape == (0, 3) and v.dtype == np.float64 and f.shape == (0, 3) and f.dtype == np.int64 and c is None
    assert ply.read_points(empty).shape == (0, 3)


# ---------------------------------------------------------------------------------------------------
# PLY writing: the three forms the tools write, byte for byte
# ---------------------------------------------------------------------------------------------------
XYZ = [(0.1, -2.5, 3.0), (1e-3, 7.0, 8.25), (-1.0, 0.0, 1.0 / 3.0)]
COLOURS = [(1, 2, 3), (250, 128, 0), (7, 7, 255)]
TRI = [(0, 1, 2), (2, 1, 0)]


def _written(tmp_path, *args, **kw):
    p = str(tmp_path / "w.ply")
    ply.write(p, *args, **kw)
    with open(p, "rb") as fh:
        return fh.read()


def test_write_the_extracted_mesh_form(tmp_path):
    """mesh.write_ply: float coordinates, uchar colours, always a face element."""
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
           "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 2\nproperty list uchar int vertex_indices\n"
           "end_header\n")
    want = hdr.encode("ascii") + b"".join(struct.pack("<3f3B", *v, *c) for v, c in zip(XYZ, COLOURS))
    want += b"".join(struct.pack("<B3i", 3, *t) for t in TRI)
    assert _written(tmp_path, np.array(XYZ), np.array(TRI), np.array(COLOURS, dtype=np.uint8), coord="f4") == want
    import torch

    from neuralrecon_w_amd import mesh

    p = str(tmp_path / "shim.ply")
    mesh.write_ply(p, torch.tensor(XYZ, dtype=torch.float64), torch.tensor(TRI), torch.tensor(COLOURS, dtype=torch.uint8))
    with open(p, "rb") as fh:
        assert fh.read() == want


def test_write_the_point_cloud_form(tmp_path):
    """The reprojection filter's clouds: double coordinates, no face element; with and without colours."""
    hdr = "ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty double x\nproperty double y\nproperty double z\n"
    rgb = "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    want = (hdr + rgb + "end_header\n").encode("ascii") + b"".join(struct.pack("<3d3B", *v, *c) for v, c in zip(XYZ, COLOURS))
    assert _written(tmp_path, np.array(XYZ), rgb=np.array(COLOURS)) == want
    want = (hdr + "end_header\n").encode("ascii") + b"".join(struct.pack("<3d", *v) for v in XYZ)
    assert _written(tmp_path, XYZ) == want


def test_write_the_evaluation_cloud_form(tmp_path):
    """eval_mesh's down_gt.ply and its like: float coordinates and `element face 0`."""
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
           "element face 0\nproperty list uchar int vertex_indices\nend_header\n")
    want = hdr.encode("ascii") + b"".join(struct.pack("<3f", *v) for v in XYZ)
    assert _written(tmp_path, np.array(XYZ), faces=np.zeros((0, 3), dtype=np.int64), coord="f4") == want
    p = str(tmp_path / "e.ply")
    evalmesh._write_points(p, np.array(XYZ))
    with open(p, "rb") as fh:
        assert fh.read() == want


# ---------------------------------------------------------------------------------------------------
# the split file and the imports
# ---------------------------------------------------------------------------------------------------
def test_split_rows_takes_the_first_tsv_by_name(tmp_path):
    with pytest.raises(FileNotFoundError, match=r"no \*.tsv split file in"):
        colmap.split_rows(str(tmp_path))
    (tmp_path / "b.tsv").write_text("filename\tid\tsplit\nz.jpg\t1\ttrain\n")
    (tmp_path / "a.tsv").write_text("filename\tid\tsplit\nx.jpg\t4\ttrain\ny.jpg\t\ttest\n")
    path, rows = colmap.split_rows(str(tmp_path))
    assert path == os.path.join(str(tmp_path), "a.tsv")
    assert [dict(r) for r in rows] == [{"filename": "x.jpg", "id": "4", "split": "train"}, {"filename": "y.jpg", "id": "", "split": "test"}]


def test_the_readers_import_without_torch():
    code = ("import sys; import neuralrecon_w_amd.colmap, neuralrecon_w_amd.ply; "
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('neuralrecon_w_amd.') and "
            "m not in ('neuralrecon_w_amd.colmap', 'neuralrecon_w_amd.ply')]; print(bad); sys.exit(1 if 'torch' in bad else 0)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
