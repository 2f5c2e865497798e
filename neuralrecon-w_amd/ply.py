"""PLY files: one reader (ascii, binary little- and big-endian) and one writer (binary little-endian) for the meshes and point
clouds the tools exchange (tools/extract_mesh.py, utils/eval_mesh.py, utils/reproj_filter.py read and write theirs with trimesh
and open3d).  numpy and the standard library only.
"""
import numpy as np

TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
         "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
         "double": "f8", "float64": "f8"}
FACE_LISTS = ("vertex_indices", "vertex_index")


def read_header(fh):
    """(format, elements) of the PLY open at its first byte; fh is left at the first byte of the body.  An element is
    dict(name, count, props); a property is (name, numpy type, None, None), a list property (name, 'list', count type, item
    type)."""
    if fh.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    fmt, elements = None, []
    while True:
        line = fh.readline()
        if not line:
            raise ValueError("PLY header without end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append({"name": tok[1], "count": int(tok[2]), "props": []})
        elif tok[0] == "property":
            if tok[1] == "list":
                elements[-1]["props"].append((tok[4], "list", TYPES[tok[2]], TYPES[tok[3]]))
            else:
                elements[-1]["props"].append((tok[2], TYPES[tok[1]], None, None))
        elif tok[0] == "end_header":
            return fmt, elements


def _load(path):
    with open(path, "rb") as fh:
        fmt, elements = read_header(fh)
        return fmt, elements, fh.read()


def _walk(fmt, elements, body):
    """The element walker: yields (element, columns) in file order.  columns = {property name: array [count]} for an element of
    scalar properties (ascii values come back as float64); for an element with list properties {list property name: list of
    `count` arrays}, its scalar properties skipped.  Lazy: an element is parsed when the caller asks for it, so a reader that
    stops after the vertex element never walks the faces behind it."""
    if fmt == "ascii":
        lines, bo = body.decode("ascii").splitlines(), None
    elif fmt in ("binary_little_endian", "binary_big_endian"):
        bo = "<" if fmt == "binary_little_endian" else ">"
    else:
        raise ValueError("unknown PLY format %r" % fmt)
    at = 0  # where the next element starts: a line (ascii) or a byte (binary)
    for e in elements:
        props, count = e["props"], e["count"]
        if not any(p[1] == "list" for p in props):  # fixed-size rows: one array
            if bo is None:
                data = np.array([ln.split() for ln in lines[at:at + count]], dtype=np.float64).reshape(-1, len(props))
                cols = {p[0]: data[:, i] for i, p in enumerate(props)}
                at += count
            else:
                dt = np.dtype([(p[0], bo + p[1]) for p in props])
                rec = np.frombuffer(body, dt, count, at)
                cols = {p[0]: rec[p[0]] for p in props}
                at += dt.itemsize * count
        elif e["name"] == "vertex":
            raise ValueError("list property in the vertex element")
        else:  # variable-length rows: walk them
            cols = {p[0]: [] for p in props if p[1] == "list"}
            for _ in range(count):
                if bo is None:
                    tok, t, at = lines[at].split(), 0, at + 1
                    for name, kind, _, _ in props:
                        if kind == "list":
                            n = int(tok[t])
                            cols[name].append(np.array(tok[t + 1:t + 1 + n], dtype=np.int64))
                            t += n
                        t += 1
                else:
                    for name, kind, ct, it in props:
                        if kind == "list":
                            n = int(np.frombuffer(body, bo + ct, 1, at)[0])
                            at += np.dtype(ct).itemsize
                            cols[name].append(np.frombuffer(body, bo + it, n, at))
                            at += n * np.dtype(it).itemsize
                        else:
                            at += np.dtype(kind).itemsize
        yield e, cols


def _xyz(cols):
    return np.stack([cols[c].astype(np.float64) for c in ("x", "y", "z")], -1).reshape(-1, 3)


def read_points(path, weld=None):
    """float64 [V,3] vertex coordinates (x, y, z) of an ascii / binary_little_endian / binary_big_endian PLY with any vertex
    property list; the walk stops after the vertex element.  What trimesh.load(...).vertices gives (utils/eval_utils.py:65,71),
    except for one thing: trimesh merges duplicate vertices when it loads a MESH -- here a file with faces (weld=None) or
    weld=True drops exact-coordinate duplicates, first occurrence kept, order preserved.  mesh.write_ply's files are welded
    already, so this changes nothing on them."""
    fmt, elements, body = _load(path)
    n_faces = sum(e["count"] for e in elements if e["name"] == "face")
    verts = np.zeros((0, 3), dtype=np.float64)
    for e, cols in _walk(fmt, elements, body):
        if e["name"] == "vertex":
            verts = np.ascontiguousarray(_xyz(cols))
            break
    if (n_faces > 0 if weld is None else weld) and verts.shape[0]:
        _, first = np.unique(verts, axis=0, return_index=True)
        verts = verts[np.sort(first)]
    return verts


def read_mesh(path):
    """(vertices float64 [V,3], faces int64 [F,3], colours uint8 [V,3] or None) of an ascii / binary PLY, vertices as stored
    (no welding: trimesh.load(process=False) and open3d.io.read_point_cloud read them so).  Colours: the vertex properties
    red / green / blue (uchar; other types are cast).  Faces: the `vertex_indices` / `vertex_index` list of the face
    element; polygons with more than three corners are fanned (0, i, i + 1) as trimesh does."""
    verts, cols, faces = np.zeros((0, 3)), None, np.zeros((0, 3), dtype=np.int64)
    for e, c in _walk(*_load(path)):
        if e["name"] == "vertex":
            verts = _xyz(c)
            if all(k in c for k in ("red", "green", "blue")):
                cols = np.stack([c[k] for k in ("red", "green", "blue")], -1).astype(np.uint8).reshape(-1, 3)
        elif e["name"] == "face":
            polys = next((c[k] for k in FACE_LISTS if k in c), [])
            tri = [np.stack([p[0].repeat(len(p) - 2), p[1:-1], p[2:]], -1) for p in polys if len(p) >= 3]
            faces = np.concatenate(tri).astype(np.int64) if tri else np.zeros((0, 3), dtype=np.int64)
    return np.ascontiguousarray(verts, dtype=np.float64), np.ascontiguousarray(faces, dtype=np.int64), cols


def read_normals(path):
    """float32 [V,3] vertex normals (the vertex properties nx / ny / nz; other types are cast) of an ascii / binary PLY, vertices
    as stored (no welding: row i belongs to row i of read_mesh's vertices); None when the file has none."""
    for e, c in _walk(*_load(path)):
        if e["name"] == "vertex":
            if not all(k in c for k in ("nx", "ny", "nz")):
                return None
            return np.ascontiguousarray(np.stack([c[k] for k in ("nx", "ny", "nz")], -1).astype(np.float32).reshape(-1, 3))
    return None


def write(path, xyz, faces=None, rgb=None, coord="f8", normals=None):
    """Binary little-endian PLY of the points xyz [V,3]: `coord` = 'f8' writes double x / y / z (open3d's write_point_cloud,
    utils/reproj_filter.py:293-300), 'f4' float (trimesh's export, tools/extract_mesh.py:160-168); normals [V,3]: float nx /
    ny / nz behind the coordinates (where open3d and meshlab write them); rgb [V,3]: uchar red / green / blue; faces [F,3]
    (None = a point cloud without a face element; an empty array = `element face 0`): `property list uchar int
    vertex_indices`."""
    hdr = ["ply", "format binary_little_endian 1.0"]
    xyz = np.ascontiguousarray(xyz, dtype="<" + coord).reshape(-1, 3)
    hdr.append("element vertex %d" % xyz.shape[0])
    hdr += ["property %s %s" % ({"f4": "float", "f8": "double"}[coord], c) for c in "xyz"]
    vrec = np.empty(xyz.shape[0], dtype=[("p", "<" + coord, 3)] + ([("n", "<f4", 3)] if normals is not None else [])
                    + ([("c", "u1", 3)] if rgb is not None else []))
    vrec["p"] = xyz
    if normals is not None:
        hdr += ["property float nx", "property float ny", "property float nz"]
        vrec["n"] = np.asarray(normals).reshape(-1, 3)
    if rgb is not None:
        hdr += ["property uchar red", "property uchar green", "property uchar blue"]
        vrec["c"] = np.asarray(rgb).reshape(-1, 3)
    body = vrec.tobytes()
    if faces is not None:
        faces = np.asarray(faces).reshape(-1, 3)
        hdr += ["element face %d" % faces.shape[0], "property list uchar int vertex_indices"]
        frec = np.empty(faces.shape[0], dtype=[("n", "u1"), ("i", "<i4", 3)])
        frec["n"], frec["i"] = 3, faces
        body += frec.tobytes()
    hdr.append("end_header")
    with open(path, "wb") as fh:
        fh.write(("\n".join(hdr) + "\n").encode("ascii"))
        fh.write(body)
