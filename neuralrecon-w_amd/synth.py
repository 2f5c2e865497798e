"""Synthetic phototourism scenes with known ground truth: from a triangle mesh and a seed, a complete scene directory that every
tool of this package reads unchanged -- in-the-wild images (per-image exposure, tint, light and sky, transient occluders with their
semantic label), a COLMAP model with noisy tracks, semantic maps, the split file, config.yaml with the TRUE sfm2gt, gt.ply -- and
`truth.json` with what a real scene never tells.  The reference has no counterpart: its scenes are downloaded.

    mesh = facade_mesh(seed=0, max_edge=0.5)
    info = generate("data/synth_facade", mesh, seed=0, n_views=60, size=(512, 384))

Frames: the mesh lives in the GT frame (z up, metres).  A seeded similarity X_gt = s R X_sfm + t (s in 3..8) is `sfm2gt`; the SfM
model and the images see the mesh through its inverse, as COLMAP would.  Per image: `reproj.RasterMesh` over static + occluder faces
-> `rasterize` -> `resolve` at ss x ss samples per pixel -> `ncw_synth_shade` (image, label map, depth) -> `ncw_synth_observe`
(key-points of the surface samples) -- csrc/ncw_synth.hip, restated bit for bit by tests/_synth_ref.py.  Meshes, cameras, tracks
and files are host numpy.  Everything is a function of the arguments: the same call writes the same bytes.  Key-points are
projected surface samples, not detected corners; there are no shadows; cameras are PINHOLE.
"""
import ctypes as C
import io
import json
import os
import shutil
import zipfile

import numpy as np

from . import colmap, labels, ply
from . import lib as L

SKY_LABEL = "sky"
OCCLUDER_MATERIAL = "person"
# name -> base colour, lattice cells per metre of the first octave, texture amplitude, ADE20K label
MATERIALS = (("ground", (0.42, 0.41, 0.40), 1.5, 0.5, "road"), ("wall", (0.80, 0.74, 0.64), 1.0, 0.4, "building"),
             ("column", (0.88, 0.86, 0.80), 3.0, 0.3, "column"), ("steps", (0.62, 0.60, 0.58), 2.0, 0.4, "stairs"),
             ("roof", (0.55, 0.30, 0.24), 2.0, 0.5, "building"), ("person", (0.25, 0.22, 0.45), 6.0, 0.8, "person"))
MATERIAL_ID = {m[0]: i for i, m in enumerate(MATERIALS)}
DEPTH_TOL = 5e-3   # a key-point is seen where the shaded depth agrees with its own to this share of the depth
MIN_OBS = 3        # views a surface sample must be seen in to become a points3D entry (scene_config_from_sfm counts tracks > 2)


class Mesh:
    """verts float64 [V, 3], faces int64 [F, 3] (outward, counter-clockwise), material uint8 [F] (index into `materials`), and
    the material table: a list of dicts base [3], freq, amp, label (ADE20K id)."""

    def __init__(self, verts, faces, material, materials):
        self.verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
        self.material = np.ascontiguousarray(material, dtype=np.uint8).reshape(-1)
        self.materials = list(materials)
        if len(self.material) != len(self.faces) or (len(self.faces) and int(self.material.max()) >= len(self.materials)):
            raise ValueError("synth.Mesh: %d faces, %d material ids, %d materials" % (len(self.faces), len(self.material), len(self.materials)))


def default_materials():
    return [{"name": n, "base": [float(v) for v in b], "freq": float(f), "amp": float(a), "label": labels.label_id(lab)}
            for n, b, f, a, lab in MATERIALS]


def face_normals(verts, faces):
    """Unit normals float64 [F, 3] of counter-clockwise faces, and twice the areas [F]."""
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    n = np.cross(b - a, c - a)
    l = np.linalg.norm(n, axis=1)
    return n / np.where(l > 0, l, 1.0)[:, None], l


# ---------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------
class _Builder:
    def __init__(self, max_edge):
        self.max_edge, self.v, self.f, self.m, self.nv = float(max_edge), [], [], [], 0

    def tri(self, a, b, c, mat):
        """Triangle (a, b, c) split uniformly into k^2 similar triangles of the same orientation, k = the smallest integer that
        brings the longest edge under max_edge."""
        a, b, c = [np.asarray(p, dtype=np.float64) for p in (a, b, c)]
        longest = max(np.linalg.norm(b - a), np.linalg.norm(c - b), np.linalg.norm(a - c))
        k = max(1, int(np.ceil(longest / self.max_edge - 1e-9)))
        ii, jj = np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing="ij")
        keep = ii + jj <= k
        idx = np.full((k + 2, k + 2), -1, dtype=np.int64)
        idx[:k + 1, :k + 1][keep] = np.arange(int(keep.sum())) + self.nv
        i, j = ii[keep], jj[keep]
        self.v.append(a + (i / k)[:, None] * (b - a) + (j / k)[:, None] * (c - a))
        up = ii + jj < k
        dn = ii + jj < k - 1
        iu, ju, id_, jd = ii[up], jj[up], ii[dn], jj[dn]
        f = np.concatenate([np.stack([idx[iu, ju], idx[iu + 1, ju], idx[iu, ju + 1]], -1),
                            np.stack([idx[id_ + 1, jd], idx[id_ + 1, jd + 1], idx[id_, jd + 1]], -1)])
        self.f.append(f)
        self.m.append(np.full(len(f), mat, dtype=np.uint8))
        self.nv += int(keep.sum())

    def quad(self, p0, p1, p2, p3, mat):
        """Counter-clockwise seen from outside."""
        self.tri(p0, p1, p2, mat)
        self.tri(p0, p2, p3, mat)

    def box(self, lo, hi, mat, bottom=True):
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        self.quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0), mat)
        self.quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1), mat)
        self.quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1), mat)
        self.quad((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0), mat)
        if bottom:
            self.quad((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0), mat)
        self.quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1), mat)

    def cylinder(self, cx, cy, z0, z1, radius, mat):
        n = max(8, int(np.ceil(2 * np.pi * radius / (self.max_edge / np.sqrt(2)))))
        ang = 2 * np.pi * np.arange(n) / n
        for k in range(n):
            a0, a1 = ang[k], ang[(k + 1) % n]
            p0 = (cx + radius * np.cos(a0), cy + radius * np.sin(a0))
            p1 = (cx + radius * np.cos(a1), cy + radius * np.sin(a1))
            self.quad((p0[0], p0[1], z0), (p1[0], p1[1], z0), (p1[0], p1[1], z1), (p0[0], p0[1], z1), mat)

    def mesh(self, materials):
        return Mesh(np.concatenate(self.v), np.concatenate(self.f), np.concatenate(self.m), materials)


def facade_mesh(seed=0, max_edge=0.5):
    """A temple-like facade in the GT frame (z up, metres, the front looks along -y): a ground grid labelled `road`, a main
    block, a colonnade of cylinders under an architrave, steps, a gable prism and two wings, with seeded proportions.  Every
    face is tessellated so that no edge exceeds max_edge; faces are outward and counter-clockwise, none has zero area; a
    per-face material id indexes `default_materials()`.  The same (seed, max_edge) gives the same arrays."""
    rng = np.random.default_rng([int(seed), 0x6d657368])
    b = _Builder(max_edge)
    G, W, C_, S, R = [MATERIAL_ID[k] for k in ("ground", "wall", "column", "steps", "roof")]
    half = 5.0 + rng.uniform(0, 1.5)        # half width of the main block
    depth = 5.0 + rng.uniform(0, 1.5)
    height = 5.5 + rng.uniform(0, 1.0)
    porch = 2.2 + rng.uniform(0, 0.6)       # the colonnade stands this far in front
    n_col = int(rng.integers(5, 8))
    n_steps = 3
    rise, tread = 0.25, 0.45
    base = n_steps * rise
    # ground: one big quad at z = 0 (tessellated), wide enough for every camera of `make_cameras` to stand on
    b.quad((-32.0, -40.0, 0.0), (32.0, -40.0, 0.0), (32.0, 10.0, 0.0), (-32.0, 10.0, 0.0), G)
    # steps: stacked slabs, the widest at the bottom
    for k in range(n_steps):
        out = (n_steps - 1 - k) * tread
        b.box((-half - 0.4 - out, -porch - 0.6 - out, k * rise), (half + 0.4 + out, 0.0, (k + 1) * rise), S, bottom=False)
    # main block and wings
    b.box((-half, 0.0, 0.0), (half, depth, base + height), W, bottom=False)
    wing = 3.0 + rng.uniform(0, 1.0)
    wh = 3.2 + rng.uniform(0, 0.8)
    b.box((-half - wing, 0.8, 0.0), (-half, depth - 0.5, wh), W, bottom=False)
    b.box((half, 0.8, 0.0), (half + wing, depth - 0.5, wh), W, bottom=False)
    # colonnade and architrave
    col_h = height - 0.9
    for k in range(n_col):
        x = -half + 0.5 + (2 * half - 1.0) * k / (n_col - 1)
        b.cylinder(x, -porch, base, base + col_h, 0.32, C_)
    b.box((-half, -porch - 0.5, base + col_h), (half, 0.0, base + height), W)
    # gable prism over the porch and the block: ridge along y
    z0, ridge = base + height, base + height + 1.6 + rng.uniform(0, 0.6)
    y0, y1 = -porch - 0.5, depth
    A, B_, T0 = (-half, y0, z0), (half, y0, z0), (0.0, y0, ridge)
    A1, B1, T1 = (-half, y1, z0), (half, y1, z0), (0.0, y1, ridge)
    b.tri(A, B_, T0, W)            # front pediment (looks along -y)
    b.tri(B1, A1, T1, W)           # back
    b.quad(B_, B1, T1, T0, R)      # +x slope
    b.quad(A1, A, T0, T1, R)       # -x slope
    return b.mesh(default_materials())


def load_mesh(path):
    """Any triangle PLY as a scene mesh in the GT frame: one material (`wall`), or -- when the file carries vertex colours -- one
    material per distinct face colour (the mean of the three corner colours, at most 255 of them; the rest share the nearest)."""
    verts, faces, cols = ply.read_mesh(path)
    if len(faces) == 0:
        raise ValueError("%s has no faces" % path)
    _, area2 = face_normals(verts, faces)
    faces = faces[area2 > 0]
    wall = default_materials()[MATERIAL_ID["wall"]]
    if cols is None:
        return Mesh(verts, faces, np.zeros(len(faces), dtype=np.uint8), [wall])
    fc = (cols[faces].astype(np.float64).mean(1) / 255.0)
    q = np.round(fc * 15).astype(np.int64)  # 16 levels per channel
    keys, inv = np.unique(q[:, 0] * 256 + q[:, 1] * 16 + q[:, 2], return_inverse=True)
    if len(keys) > 255:  # keep the 255 most frequent, the rest go to the nearest kept colour
        cnt = np.bincount(inv)
        top = np.sort(np.argsort(-cnt, kind="stable")[:255])
        pal = np.stack([keys[top] // 256, keys[top] // 16 % 16, keys[top] % 16], -1)
        inv = np.argmin(((q[:, None, :] - pal[None]) ** 2).sum(-1), 1)
        keys = keys[top]
    mats = [dict(wall, name="colour%d" % i, base=[(k // 256) / 15.0, (k // 16 % 16) / 15.0, (k % 16) / 15.0]) for i, k in enumerate(keys)]
    return Mesh(verts, faces, inv.astype(np.uint8), mats)


# ---------------------------------------------------------------------------------------------------
# frames and cameras
# ---------------------------------------------------------------------------------------------------
def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return colmap.qvec2rotmat(q)


def random_sfm2gt(seed, centre, extent):
    """4x4 float64 similarity X_gt = s R X_sfm + t: s in 3..8, a random rotation, and t so that the SfM origin lies within one
    extent of the mesh centre."""
    rng = np.random.default_rng([int(seed), 0x73326774])
    T = np.eye(4)
    T[:3, :3] = rng.uniform(3.0, 8.0) * random_rotation(rng)
    T[:3, 3] = np.asarray(centre) + rng.uniform(-1, 1, 3) * extent
    return T


def invert_similarity(T):
    """The inverse of [s R | t] without a general matrix inverse: [R^T / s | -R^T t / s]."""
    A = T[:3, :3]
    s2 = float((A[0] ** 2).sum())
    inv = np.eye(4)
    inv[:3, :3] = A.T / s2
    inv[:3, 3] = -inv[:3, :3] @ T[:3, 3]
    return inv


def look_at(pos, target, up=(0.0, 0.0, 1.0)):
    """World -> camera (OpenCV axes: x right, y down, z forward) 4x4 of a camera at pos looking at target."""
    pos, target = np.asarray(pos, dtype=np.float64), np.asarray(target, dtype=np.float64)
    f = (target - pos) / np.linalg.norm(target - pos)
    r = np.cross(f, np.asarray(up, dtype=np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    M = np.eye(4)
    M[:3, :3] = np.stack([r, d, f])
    M[:3, 3] = -M[:3, :3] @ pos
    return M


def make_cameras(seed, n_views, size, lo, hi):
    """n_views PINHOLE cameras in the GT frame on a jittered arc in front of the building's box [lo, hi] (front = -y), at eye
    height and above, each looking at a jittered target on the front; seeded focal lengths and image sizes (even, at most
    `size` = (W, H)); cx = W / 2, cy = H / 2 exactly.  Returns a list of dicts w2c [4, 4], K (fx, fy, cx, cy), width, height."""
    rng = np.random.default_rng([int(seed), 0x63616d73])
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    cen = (lo + hi) / 2
    wid, hgt = hi[0] - lo[0], hi[2] - lo[2]
    cams = []
    for k in range(n_views):
        ang = np.deg2rad(-55 + 110 * (k + 0.5) / n_views + rng.uniform(-6, 6))
        dist = max(wid, hgt) * rng.uniform(0.95, 1.35)
        pos = np.array([cen[0] + dist * np.sin(ang), lo[1] - dist * np.cos(ang), rng.uniform(1.6, 4.5)])
        tgt = np.array([cen[0] + rng.uniform(-0.2, 0.2) * wid, lo[1], lo[2] + rng.uniform(0.35, 0.6) * hgt])
        W = 2 * int(round(size[0] * rng.uniform(0.85, 1.0) / 2))
        H = 2 * int(round(size[1] * rng.uniform(0.85, 1.0) / 2))
        W, H = max(2, min(W, size[0] // 2 * 2)), max(2, min(H, size[1] // 2 * 2))
        # focal length so that the building spans about 60 .. 90 % of the smaller field
        span = 1.25 * max(wid / W, hgt / H) * rng.uniform(1.1, 1.6)
        f = float(np.linalg.norm(tgt - pos) / span)
        cams.append({"w2c": look_at(pos, tgt), "K": (f, f * rng.uniform(0.995, 1.005), W / 2.0, H / 2.0), "width": W, "height": H})
    return cams


def to_sfm_pose(w2c_gt, sfm2gt):
    """The COLMAP pose (R, t: camera = R X_sfm + t, in SfM units) of a camera given as world -> camera in the GT frame."""
    A, t = sfm2gt[:3, :3], sfm2gt[:3, 3]
    s = float(np.sqrt((A[0] ** 2).sum()))
    Rc, tc = w2c_gt[:3, :3], w2c_gt[:3, 3]
    return Rc @ (A / s), (Rc @ t + tc) / s


# ---------------------------------------------------------------------------------------------------
# the two launches
# ---------------------------------------------------------------------------------------------------
def _floats(n, values):
    return (C.c_float * n)(*[float(v) for v in np.asarray(values, dtype=np.float64).reshape(-1)])


def image_struct(K, c2w, sfm2gt, height, width, ss, app, tex_seed, sky_label):
    """NcwSynthImage.  K = (fx, fy, cx, cy) of the height x width image; c2w: camera (OpenCV axes) -> world 3x4; sfm2gt 3x4;
    app: dict light [3] (unit), ambient, diffuse, gain [3], bias [3], sky_top [3], sky_bottom [3]."""
    s = L.NcwSynthImage()
    s.fx, s.fy, s.cx, s.cy = [float(v) for v in K]
    s.c2w, s.sfm2gt = _floats(12, np.asarray(c2w)[:3, :4]), _floats(12, np.asarray(sfm2gt)[:3, :4])
    s.light, s.gain, s.bias = _floats(3, app["light"]), _floats(3, app["gain"]), _floats(3, app["bias"])
    s.sky_top, s.sky_bottom = _floats(3, app["sky_top"]), _floats(3, app["sky_bottom"])
    s.ambient, s.diffuse = float(app["ambient"]), float(app["diffuse"])
    s.height, s.width, s.ss, s.sky_label, s.tex_seed = int(height), int(width), int(ss), int(sky_label), int(tex_seed) & 0xFFFFFFFF
    return s


def material_table(materials, device):
    import torch

    tab = (L.NcwSynthMaterial * len(materials))()
    for t, m in zip(tab, materials):
        t.base, t.freq, t.amp, t.label = _floats(3, m["base"]), float(m["freq"]), float(m["amp"]), int(m["label"])
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(device)


def shade(depth_ss, face_ss, img, face_normal, face_material, materials_dev, n_materials):
    """One `ncw_synth_shade` launch: (rgb uint8 [h, w, 3], label uint8 [h, w], depth float32 [h, w]) on the device of depth_ss.
    depth_ss / face_ss: the planes of `reproj.resolve` at (h ss) x (w ss); face_normal float32 [F, 3], face_material uint8 [F]."""
    import torch

    dev = depth_ss.device
    if dev.type != "cuda":
        raise L.NeuconwHipError("synth.shade: the planes are not on a GPU; there is no CPU fallback")
    h, w, ss = img.height, img.width, img.ss
    if tuple(depth_ss.shape) != (h * ss, w * ss) or tuple(face_ss.shape) != (h * ss, w * ss):
        raise ValueError("synth.shade: planes %s / %s for a %d x %d image at ss = %d" % (tuple(depth_ss.shape), tuple(face_ss.shape), h, w, ss))
    if depth_ss.dtype != torch.float32 or face_ss.dtype != torch.int32 or face_normal.dtype != torch.float32 or face_material.dtype != torch.uint8:
        raise ValueError("synth.shade: depth float32, face int32, normals float32, materials uint8 expected")
    nf = int(face_material.shape[0])
    if tuple(face_normal.shape) != (nf, 3):
        raise ValueError("synth.shade: %d materials for normals %s" % (nf, tuple(face_normal.shape)))
    rgb = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
    label = torch.empty(h, w, dtype=torch.uint8, device=dev)
    depth = torch.empty(h, w, dtype=torch.float32, device=dev)
    L.check(L.get_lib().ncw_synth_shade(L.ptr(depth_ss.contiguous()), L.ptr(face_ss.contiguous()), C.byref(img), L.ptr(face_normal.contiguous()),
                                        L.ptr(face_material.contiguous()), nf, L.ptr(materials_dev), int(n_materials), L.ptr(rgb),
                                        L.ptr(label), L.ptr(depth), L.stream_ptr(dev)), "ncw_synth_shade")
    return rgb, label, depth


def view_struct(w2c, K, height, width, znear, sigma, depth_tol, seed, serial):
    """NcwSynthView of a world -> camera matrix (3x4 / 4x4 float64, OpenCV axes) whose rotation part is orthonormal."""
    M = np.asarray(w2c, dtype=np.float64)[:3, :4]
    s = L.NcwSynthView()
    s.w2c = (C.c_double * 12)(*M.reshape(-1))
    s.centre = (C.c_double * 3)(*(-M[:, :3].T @ M[:, 3]))
    s.fx, s.fy, s.cx, s.cy = [float(v) for v in K]
    s.znear, s.sigma_r3, s.depth_tol = float(znear), float(sigma) * float(np.sqrt(3.0)), float(depth_tol)
    s.seed, s.height, s.width, s.serial = int(seed) & 0xFFFFFFFFFFFFFFFF, int(height), int(width), int(serial) & 0xFFFFFFFF
    return s


def observe(pts, nrm, index, view, depth, chunk=None):
    """`ncw_synth_observe` over n points (device float64 [n, 3] x 2, int64 [n]) against the shaded depth plane: (xy float64
    [n, 2], err float64 [n] = the pixel distance of the noisy from the true projection, vis uint8 [n]) on the device.  The
    kernel writes the squared distance; the root is taken here.  chunk: points per launch (None = one launch); the result
    does not depend on it."""
    import torch

    dev = pts.device
    if dev.type != "cuda":
        raise L.NeuconwHipError("synth.observe: the points are not on a GPU; there is no CPU fallback")
    n = int(pts.shape[0])
    if pts.dtype != torch.float64 or nrm.dtype != torch.float64 or index.dtype != torch.int64 or tuple(nrm.shape) != (n, 3) or \
            tuple(pts.shape) != (n, 3) or tuple(index.shape) != (n,) or depth.dtype != torch.float32 or \
            tuple(depth.shape) != (view.height, view.width):
        raise ValueError("synth.observe: float64 [n, 3] points and normals, int64 [n] indices and a float32 [h, w] depth plane expected")
    pts, nrm, index, depth = pts.contiguous(), nrm.contiguous(), index.contiguous(), depth.contiguous()
    xy = torch.empty(n, 2, dtype=torch.float64, device=dev)
    err = torch.empty(n, dtype=torch.float64, device=dev)
    vis = torch.empty(n, dtype=torch.uint8, device=dev)
    step = max(1, n if chunk is None else int(chunk))
    for i0 in range(0, n, step):
        c = min(step, n - i0)
        L.check(L.get_lib().ncw_synth_observe(L.ptr(pts[i0:i0 + c]), L.ptr(nrm[i0:i0 + c]), L.ptr(index[i0:i0 + c]), c, C.byref(view),
                                              L.ptr(depth), L.ptr(xy[i0:i0 + c]), L.ptr(err[i0:i0 + c]), L.ptr(vis[i0:i0 + c]),
                                              L.stream_ptr(dev)), "ncw_synth_observe")
    return xy, torch.sqrt(err), vis


def raster_K(K, ss):
    """The intrinsics handed to the rasterizer for the (h ss) x (w ss) planes: it samples at (c + 0.5, r + 0.5), the project's
    rays go through integer pixels, so cx and cy move by half a pixel before the scale."""
    fx, fy, cx, cy = [float(v) for v in K]
    return np.array([[fx * ss, 0, cx * ss + 0.5 * ss], [0, fy * ss, cy * ss + 0.5 * ss], [0, 0, 1]], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------
# per-image draws
# ---------------------------------------------------------------------------------------------------
def draw_appearance(rng):
    """Exposure, tint, bias, light (unit, GT frame, from above and in front), ambient / diffuse and the two sky colours."""
    expo = rng.uniform(0.75, 1.3)
    tint = 1.0 + rng.uniform(-0.08, 0.08, 3)
    az, el = np.deg2rad(rng.uniform(-70, 70)), np.deg2rad(rng.uniform(25, 70))
    light = np.array([np.cos(el) * np.sin(az), -np.cos(el) * np.cos(az), np.sin(el)])
    ambient = rng.uniform(0.35, 0.55)
    sky_top = np.array([0.30, 0.50, 0.85]) + rng.uniform(-0.1, 0.1, 3)
    sky_bottom = np.array([0.75, 0.82, 0.92]) + rng.uniform(-0.08, 0.08, 3)
    return {"gain": (expo * tint).tolist(), "bias": rng.uniform(-0.03, 0.03, 3).tolist(), "light": (light / np.linalg.norm(light)).tolist(),
            "ambient": float(ambient), "diffuse": float(1.05 - ambient + rng.uniform(0, 0.2)), "sky_top": sky_top.tolist(),
            "sky_bottom": sky_bottom.tolist()}


def draw_occluders(rng, n, cam_pos, lo, hi):
    """n person-sized boxes standing on the ground between the camera and the building's front (GT frame): list of [lo, hi]."""
    out = []
    front = np.array([(lo[0] + hi[0]) / 2, lo[1], 0.0])
    for _ in range(n):
        a = rng.uniform(0.25, 0.7)
        foot = cam_pos * (1 - a) + front * a
        foot = foot + np.array([rng.uniform(-0.25, 0.25) * (hi[0] - lo[0]), rng.uniform(-0.5, 0.5), 0.0])
        w, d, h = rng.uniform(0.45, 0.65), rng.uniform(0.3, 0.45), rng.uniform(1.55, 1.9)
        out.append([[float(foot[0] - w / 2), float(foot[1] - d / 2), 0.0], [float(foot[0] + w / 2), float(foot[1] + d / 2), float(h)]])
    return out


def occluder_mesh(boxes, mat):
    b = _Builder(1e9)
    for lo, hi in boxes:
        b.box(lo, hi, mat, bottom=False)
    if not boxes:
        return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.uint8)
    return np.concatenate(b.v), np.concatenate(b.f), np.concatenate(b.m)


def write_npz(path, arr):
    """<path> = a zip with the one member arr_0.npy, as np.savez_compressed writes it -- but with a fixed member time, so that
    the same array gives the same bytes."""
    buf = io.BytesIO()
    np.lib.format.write_array(buf, np.ascontiguousarray(arr), allow_pickle=False)
    info = zipfile.ZipInfo("arr_0.npy", date_time=(1980, 1, 1, 0, 0, 0))
    info.compress_type = zipfile.ZIP_DEFLATED
    info.external_attr = 0o644 << 16
    with zipfile.ZipFile(path, "w") as z:
        z.writestr(info, buf.getvalue())


# ---------------------------------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------------------------------
def building_box(mesh):
    """[lo, hi] of every face that is not ground (material label `road`), GT frame; the whole mesh when nothing else is left."""
    road = labels.label_id("road")
    keep = np.array([mesh.materials[m]["label"] != road for m in mesh.material], dtype=bool)
    v = mesh.verts[np.unique(mesh.faces[keep])] if keep.any() else mesh.verts
    return v.min(0), v.max(0)


def train_overrides(root, n_vocab):
    """The overrides of config.DEFAULTS a synthetic scene trains with: W = 256 networks, 64 + 64 samples, the scene's vocabulary,
    semantics on, `person` rays masked.  NEAR_FAR_OVERRIDE is on as in the reference's scene yamls: the renderer keeps the path of
    the SfM model only then (its coupling, rendering/renderer.py:96-99), and the octree refresh every UPDATE_FREQ steps needs it."""
    return {"DATASET": {"ROOT_DIR": str(root), "DATASET_NAME": "phototourism", "PHOTOTOURISM": {"WITH_SEMANTICS": True}},
            "NEUCONW": {"N_SAMPLES": 64, "N_IMPORTANCE": 64, "N_VOCAB": int(n_vocab), "RAY_MASK_LIST": [OCCLUDER_MATERIAL],
                        "NEAR_FAR_OVERRIDE": True,
                        "SDF_CONFIG": {"d_hidden": 256, "d_out": 257}, "COLOR_CONFIG": {"d_feature": 256, "d_hidden": 256}}}


def generate(root, mesh=None, seed=0, n_views=60, size=(512, 384), n_points=40000, n_gt=2000000, pixel_sigma=0.5, n_occluders=2, ss=2,
             max_edge=0.5, min_obs=MIN_OBS, unmatched_share=0.3, outlier_share=0.02, point_sigma=0.0, num_test=None, jpeg=False,
             overwrite=False, device="cuda:0", verbose=False):
    """Writes the scene directory `root` (an existing one is refused with FileExistsError unless overwrite, which removes it
    first) and returns a dict of what it wrote.  mesh: a `Mesh` in the GT frame (None = facade_mesh(seed, max_edge)).  See the
    module text for the frames; files: dense/images/<name>, dense/sparse/{cameras,images,points3D}.bin, semantic_maps/<stem>.npz,
    <dirname>.tsv, config.yaml, gt.ply, mesh.ply, train.yaml, truth.json."""
    import torch
    import yaml

    from . import evalmesh, reproj, sceneprep, views

    if not 1 <= int(ss) <= L.SYNTH_MAX_SS:
        raise ValueError("synth.generate: ss must be 1 .. %d" % L.SYNTH_MAX_SS)
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise L.NeuconwHipError("synth.generate: device %s is not a GPU; there is no CPU fallback" % (dev,))
    if os.path.exists(root):
        if not overwrite:
            raise FileExistsError("%s exists: pass overwrite=True (--overwrite) to replace it" % root)
        shutil.rmtree(root)
    seed, n_views, ss = int(seed), int(n_views), int(ss)
    num_test = max(1, n_views // 10) if num_test is None else int(num_test)
    mesh = facade_mesh(seed, max_edge) if mesh is None else mesh
    log = print if verbose else (lambda *a: None)
    for d in ("dense/images", "dense/sparse", "semantic_maps"):
        os.makedirs(os.path.join(root, d))

    # frames
    lo, hi = building_box(mesh)
    extent = float(np.linalg.norm(mesh.verts.max(0) - mesh.verts.min(0)))
    sfm2gt = random_sfm2gt(seed, (lo + hi) / 2, float(np.linalg.norm(hi - lo)))
    gt2sfm = invert_similarity(sfm2gt)
    scale = float(np.sqrt((sfm2gt[0, :3] ** 2).sum()))
    Rs = sfm2gt[:3, :3] / scale
    to_sfm = lambda X: X @ gt2sfm[:3, :3].T + gt2sfm[:3, 3]
    verts_sfm = to_sfm(mesh.verts)
    nrm_gt, _ = face_normals(mesh.verts, mesh.faces)
    sky, person = labels.label_id(SKY_LABEL), labels.label_id(OCCLUDER_MATERIAL)
    materials = list(mesh.materials)
    occ_mat = next((i for i, m in enumerate(materials) if m["label"] == person), None)
    if occ_mat is None:
        materials.append(default_materials()[MATERIAL_ID[OCCLUDER_MATERIAL]])
        occ_mat = len(materials) - 1
    if len(materials) > 256:
        raise ValueError("synth.generate: at most 256 materials")
    mats_dev = material_table(materials, dev)

    # surface samples: the candidates of the SfM tracks (GT frame), their normals in the SfM frame
    # (drawn from the building and the ground around it, a quarter of its width on every side: SfM points gather on the subject)
    cen = mesh.verts[mesh.faces].mean(1)
    pad_xy = 0.25 * float(max(hi[0] - lo[0], hi[1] - lo[1]))
    cand = np.nonzero(((cen[:, :2] >= lo[:2] - pad_xy) & (cen[:, :2] <= hi[:2] + pad_xy)).all(1))[0]
    pts_gt, tri = evalmesh.sample_surface(mesh.verts, mesh.faces[cand], int(n_points), seed=seed, return_index=True, device=dev)
    tri_h = cand[tri.cpu().numpy().astype(np.int64)]
    pts_sfm_h = to_sfm(pts_gt.cpu().numpy())
    n_pts = len(pts_sfm_h)
    pts_d = torch.from_numpy(pts_sfm_h).to(dev)
    nrm_d = torch.from_numpy(np.ascontiguousarray(nrm_gt[tri_h] @ Rs)).to(dev)  # R^T n as rows
    idx_d = torch.arange(n_pts, dtype=torch.int64, device=dev)

    cams = make_cameras(seed, n_views, size, lo, hi)
    rng = np.random.default_rng([seed, 0x696d6773])
    names, per_image, truth_images = [], [], []
    vis_all = np.zeros((n_views, n_pts), dtype=bool)
    xy_all = np.zeros((n_views, n_pts, 2))
    err_all = np.zeros((n_views, n_pts))
    seen_faces = np.zeros(len(mesh.faces), dtype=bool)
    first_rgb = np.zeros((n_pts, 3), dtype=np.uint8)
    have_rgb = np.zeros(n_pts, dtype=bool)
    for k, cam in enumerate(cams):
        image_id = k + 1
        name = "%04d.%s" % (image_id, "jpg" if jpeg else "png")
        app = draw_appearance(rng)
        cam_pos = -cam["w2c"][:3, :3].T @ cam["w2c"][:3, 3]
        boxes = draw_occluders(rng, int(n_occluders), cam_pos, lo, hi)
        ov, of, om = occluder_mesh(boxes, occ_mat)
        v_all = np.concatenate([verts_sfm, to_sfm(ov)]) if len(ov) else verts_sfm
        f_all = np.concatenate([mesh.faces, of + len(verts_sfm)]) if len(of) else mesh.faces
        m_all = np.concatenate([mesh.material, om])
        n_all = np.concatenate([nrm_gt, face_normals(ov, of)[0]]) if len(of) else nrm_gt
        R, t = to_sfm_pose(cam["w2c"], sfm2gt)
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = R, t
        c2w = np.linalg.inv(w2c)
        H, W = cam["height"], cam["width"]
        rm = reproj.RasterMesh(v_all, f_all, dev)
        rs = rm.view_struct(raster_K(cam["K"], ss), w2c, H * ss, W * ss, znear=0.002 * extent / scale, zfar=100.0 * extent / scale)
        zbuf = torch.empty(H * ss * W * ss, dtype=torch.int64, device=dev)
        rm.rasterize(rs, zbuf)
        depth_ss, face_ss = reproj.resolve(zbuf, H * ss, W * ss)
        img = image_struct(cam["K"], c2w, sfm2gt, H, W, ss, app, seed, sky)
        rgb, label, depth = shade(depth_ss, face_ss, img, torch.from_numpy(n_all.astype(np.float32)).to(dev),
                                  torch.from_numpy(m_all).to(dev), mats_dev, len(materials))
        vs = view_struct(w2c, cam["K"], H, W, 0.002 * extent / scale, pixel_sigma, DEPTH_TOL, seed, image_id)
        xy, err, vis = observe(pts_d, nrm_d, idx_d, vs, depth)
        rgb_h, label_h = rgb.cpu().numpy(), label.cpu().numpy()
        vis_all[k], xy_all[k], err_all[k] = vis.cpu().numpy().astype(bool), xy.cpu().numpy(), err.cpu().numpy()
        fs = torch.unique(face_ss[face_ss >= 0]).cpu().numpy()
        seen_faces[fs[fs < len(mesh.faces)]] = True
        # colour of a point: the pixel of its first observation
        new = vis_all[k] & ~have_rgb
        if new.any():
            Kf = cam["K"]
            cam_pts = pts_sfm_h[new] @ R.T + t
            col = np.clip(np.floor(Kf[0] * cam_pts[:, 0] / cam_pts[:, 2] + Kf[2] + 0.5).astype(np.int64), 0, W - 1)
            row = np.clip(np.floor(Kf[1] * cam_pts[:, 1] / cam_pts[:, 2] + Kf[3] + 0.5).astype(np.int64), 0, H - 1)
            first_rgb[new] = rgb_h[row, col]
            have_rgb |= new
        path = os.path.join(root, "dense", "images", name)
        if jpeg:
            from PIL import Image

            Image.fromarray(rgb_h).save(path, quality=95)
        else:
            views.write_png(path, rgb_h)
        write_npz(os.path.join(root, "semantic_maps", name.split(".")[0] + ".npz"), label_h)
        names.append(name)
        per_image.append({"id": image_id, "qvec": colmap.rotmat2qvec(R), "tvec": t, "camera_id": image_id, "name": name})
        truth_images.append({"name": name, "image_id": image_id, "appearance": app, "occluders": boxes, "visible_points": int(vis_all[k].sum()),
                             "width": W, "height": H})
        log("image %s: %d x %d, %d visible points" % (name, W, H, int(vis_all[k].sum())))

    # tracks
    n_obs = vis_all.sum(0)
    is_point = n_obs >= int(min_obs)
    point_idx = np.nonzero(is_point)[0]
    trng = np.random.default_rng([seed, 0x74726b73])
    outlier = np.zeros(n_pts, dtype=bool)
    n_out = int(round(float(outlier_share) * len(point_idx)))
    if n_out:
        outlier[trng.choice(point_idx, n_out, replace=False)] = True
    in_track = vis_all & is_point[None]
    for i in np.nonzero(outlier)[0]:  # short tracks: the first two views only
        vk = np.nonzero(in_track[:, i])[0]
        in_track[vk[2:], i] = False
    xyz = pts_sfm_h.copy()
    if point_sigma > 0:
        xyz += trng.normal(size=xyz.shape) * float(point_sigma) / scale
    disp = trng.normal(size=(n_pts, 3))
    disp *= (trng.uniform(0.05, 0.3, n_pts) * extent / scale / np.linalg.norm(disp, axis=1))[:, None]
    xyz[outlier] += disp[outlier]
    out_err = trng.uniform(5.0, 20.0, n_pts)
    # 2-D points per image: the visible samples in point order, then the unmatched extras
    kp_index = np.full((n_views, n_pts), -1, dtype=np.int64)
    images = []
    for k, im in enumerate(per_image):
        vk = np.nonzero(vis_all[k])[0]
        kp_index[k, vk] = np.arange(len(vk))
        ids = np.where(in_track[k, vk], vk + 1, -1)
        n_extra = int(round(float(unmatched_share) * len(vk)))
        extra = trng.uniform(0, 1, (n_extra, 2)) * np.array([cams[k]["width"] - 1, cams[k]["height"] - 1])
        images.append(dict(im, xys=np.concatenate([xy_all[k, vk], extra]), point3d_ids=np.concatenate([ids, np.full(n_extra, -1)])))
    t_len = in_track[:, point_idx].sum(0)
    start = np.concatenate([[0], np.cumsum(t_len)]).astype(np.int64)
    vv, pp = np.nonzero(in_track[:, point_idx].T)[::-1]  # point-major, view order inside a point
    t_img, t_idx = (vv + 1).astype(np.int32), kp_index[vv, point_idx[pp]].astype(np.int32)
    err_sum = np.where(in_track, err_all, 0.0).sum(0)[point_idx]
    p_err = np.where(outlier[point_idx], out_err[point_idx], err_sum / np.maximum(t_len, 1))
    sp = os.path.join(root, "dense", "sparse")
    colmap.write_cameras(os.path.join(sp, "cameras.bin"), [{"id": k + 1, "model": colmap.PINHOLE, "width": c["width"], "height": c["height"],
                                                           "params": c["K"]} for k, c in enumerate(cams)])
    colmap.write_images(os.path.join(sp, "images.bin"), images)
    colmap.write_points3d(os.path.join(sp, "points3D.bin"), point_idx + 1, xyz[point_idx], first_rgb[point_idx], p_err, start, t_img, t_idx)

    # split, config, ground truth
    sceneprep.write_split(root, names, num_test)
    cfg = sceneprep.scene_config_from_sfm(os.path.join(sp, "points3D.bin"), os.path.basename(os.path.normpath(os.path.abspath(root))))
    pad = 0.02 * float(np.linalg.norm(hi - lo))
    box_lo, box_hi = lo - pad, hi + pad
    box_lo[2] = max(box_lo[2], lo[2] + 0.05 * (hi[2] - lo[2]))  # above the ground
    box = [box_lo.tolist(), box_hi.tolist()]
    cfg["sfm2gt"] = sfm2gt.tolist()
    cfg["eval_bbx"], cfg["eval_bbx_detail"] = box, [list(box[0]), list(box[1])]
    sceneprep.write_scene_config(root, cfg)
    gt = evalmesh.sample_surface(mesh.verts, mesh.faces, int(n_gt), seed=seed + 1, box=box, device=dev).cpu().numpy()
    ply.write(os.path.join(root, "gt.ply"), gt)
    ply.write(os.path.join(root, "mesh.ply"), verts_sfm, faces=mesh.faces)
    with open(os.path.join(root, "train.yaml"), "w") as fh:
        yaml.dump(train_overrides(root, n_views + 1), fh, default_flow_style=False, sort_keys=False)
    truth = {"seed": seed, "sfm2gt": sfm2gt.tolist(), "scale": scale, "pixel_sigma": float(pixel_sigma), "point_sigma": float(point_sigma),
             "ss": ss, "min_obs": int(min_obs), "images": truth_images, "outlier_point_ids": (np.nonzero(outlier)[0] + 1).tolist(),
             "n_points3d": int(len(point_idx)), "labels": sorted({int(m["label"]) for m in materials} | {sky}),
             "seen_faces": np.nonzero(seen_faces)[0].tolist(), "n_faces": int(len(mesh.faces)), "eval_bbx": box, "n_gt": int(len(gt))}
    with open(os.path.join(root, "truth.json"), "w") as fh:
        json.dump(truth, fh, sort_keys=True)
        fh.write("\n")
    return {"root": root, "names": names, "n_points3d": int(len(point_idx)), "n_gt": int(len(gt)), "sfm2gt": sfm2gt, "truth": truth}
