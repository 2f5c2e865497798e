"""GPU: the synthetic-scene kernels (csrc/ncw_synth.hip) bit for bit against tests/_synth_ref.py, the pixel convention against
the project's own rays, and one small generated scene read back by the package's readers, scored against its known answers and
trained on for one step."""
import ctypes as C
import filecmp
import json
import os
import shutil

import numpy as np
import pytest
import torch
import yaml

from neuralrecon_w_amd import colmap, evalmesh, lib as L, ply, reproj, sceneprep, synth, views
from tests import _synth_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MATS = [{"base": [0.8, 0.7, 0.6], "freq": 1.5, "amp": 0.5, "label": 1}, {"base": [0.3, 0.9, 0.2], "freq": 3.0, "amp": 0.25, "label": 42},
        {"base": [0.25, 0.25, 0.5], "freq": 6.0, "amp": 0.75, "label": 12}]
SKY = 2


def f32(v):
    """Python floats that float32 holds exactly: the structs then carry what the restatement computes with."""
    return np.asarray(v, dtype=np.float32).astype(np.float64).tolist()


def _rot(rng):
    q = rng.normal(size=4)
    return colmap.qvec2rotmat(q / np.linalg.norm(q))


def _img(rng, h, w, ss, **over):
    c2w = np.concatenate([_rot(rng), rng.uniform(-2, 2, (3, 1))], 1)
    s2g = np.concatenate([4.5 * _rot(rng), rng.uniform(-20, 20, (3, 1))], 1)
    light = rng.normal(size=3)
    d = {"fx": 37.5, "fy": 38.25, "cx": w / 2.0, "cy": h / 2.0, "c2w": f32(c2w.reshape(-1)), "sfm2gt": f32(s2g.reshape(-1)),
         "light": f32(light / np.linalg.norm(light)), "ambient": 0.4375, "diffuse": 0.75, "gain": f32([1.1, 0.9, 1.0]),
         "bias": f32([0.01, -0.02, 0.0]), "sky_top": f32([0.3, 0.5, 0.85]), "sky_bottom": f32([0.8, 0.85, 0.9]), "height": h,
         "width": w, "ss": ss, "sky_label": SKY, "tex_seed": 12345}
    d.update(over)
    return d


def _struct(d):
    app = {k: d[k] for k in ("light", "ambient", "diffuse", "gain", "bias", "sky_top", "sky_bottom")}
    return synth.image_struct((d["fx"], d["fy"], d["cx"], d["cy"]), np.array(d["c2w"]).reshape(3, 4), np.array(d["sfm2gt"]).reshape(3, 4),
                              d["height"], d["width"], d["ss"], app, d["tex_seed"], d["sky_label"])


def _shade_both(depth_ss, face_ss, d, normals, mat_ids, mats=MATS):
    tab = synth.material_table(mats, DEV)
    got = synth.shade(torch.from_numpy(depth_ss).to(DEV), torch.from_numpy(face_ss).to(DEV), _struct(d),
                      torch.from_numpy(normals).to(DEV), torch.from_numpy(mat_ids).to(DEV), tab, len(mats))
    want = R.shade(depth_ss, face_ss, d, normals, mat_ids, mats)
    for g, w_, name in zip(got, want, ("rgb", "label", "depth")):
        assert g.dtype == torch.from_numpy(w_).dtype and torch.equal(g.cpu(), torch.from_numpy(w_)), name
    return want


def _planes(rng, h, w, ss, nf, holes=0.3):
    face = rng.integers(0, nf, (h * ss, w * ss)).astype(np.int32)
    face[rng.uniform(size=face.shape) < holes] = -1
    depth = np.where(face >= 0, rng.uniform(1.0, 3.0, face.shape), 0.0).astype(np.float32)
    return depth, face


def _faces(rng, nf):
    n = rng.normal(size=(nf, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32), rng.integers(0, len(MATS), nf).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------
# 1. shade
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", [1, 2, 3])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (2, 63), (2, 64), (2, 65)])
def test_shade_bit_for_bit_on_handcrafted_planes(hw, ss):
    h, w = hw
    rng = np.random.default_rng(100 * h + w + ss)
    normals, mat_ids = _faces(rng, 7)
    mat_ids[:3] = [0, 1, 2]
    depth, face = _planes(rng, h, w, ss, 7)
    rgb, label, _ = _shade_both(depth, face, _img(rng, h, w, ss), normals, mat_ids)
    if h * w > 100:
        assert {1, 42, 12, SKY} == set(np.unique(label).tolist())  # two materials with different labels, the occluder's, and sky
    # gains and biases that clamp at both ends: channel 0 saturates, channel 1 goes under 0, channel 2 stays inside
    rgb, _, _ = _shade_both(depth, face, _img(rng, h, w, ss, gain=f32([40.0, 0.5, 1.0]), bias=f32([0.5, -2.0, 0.1])), normals, mat_ids)
    hit = face.reshape(h, ss, w, ss).transpose(0, 2, 1, 3).reshape(h, w, -1).min(-1) >= 0  # pixels without a sky sample
    if hit.any():
        assert (rgb[hit][:, 0] == 255).all() and (rgb[hit][:, 1] == 0).all()


def test_shade_all_sky_and_the_rounding_tie():
    rng = np.random.default_rng(5)
    normals, mat_ids = _faces(rng, 3)
    for ss in (1, 2, 3):
        h, w = 4, 9
        depth, face = np.zeros((h * ss, w * ss), dtype=np.float32), np.full((h * ss, w * ss), -1, dtype=np.int32)
        rgb, label, dep = _shade_both(depth, face, _img(rng, h, w, ss), normals, mat_ids)
        assert (label == SKY).all() and (dep == 0).all() and (rgb[0] != rgb[-1]).any()  # the vertical blend
        # 0.5 * 255 + 0.5 = 128 exactly: the tie goes up
        rgb, _, _ = _shade_both(depth, face, _img(rng, h, w, ss, sky_top=[0.5] * 3, sky_bottom=[0.5] * 3), normals, mat_ids)
        assert (rgb == 128).all()
    # a face index past the table, and a face with depth 0, are sky; a material id past the table takes the last material
    depth, face = _planes(rng, 3, 4, 2, 3, holes=0.0)
    face[0, 0], face[0, 1], depth[1, 1] = 3, 2 ** 31 - 1, 0.0
    mat_ids[0] = 200
    _shade_both(depth, face, _img(rng, 3, 4, 2), normals, mat_ids)


def _box(lo=(-1.0, -0.6, -0.8), hi=(1.0, 0.6, 0.8)):
    b = synth._Builder(1e9)
    b.box(lo, hi, 0)
    return np.concatenate(b.v), np.concatenate(b.f)


def _look(pos, target):
    return synth.look_at(pos, target, up=(0.0, 0.0, 1.0))


@pytest.fixture(scope="module")
def box_view():
    """The 12-triangle box with a two-triangle occluder in front, seen by the real rasterizer once at ss = 1 and ss = 2."""
    v, f = _box()
    ov = np.array([[-0.3, -1.5, -0.5], [0.2, -1.5, -0.5], [0.2, -1.5, 0.4], [-0.3, -1.5, 0.4]])  # looks along -y, at the camera
    verts = np.concatenate([v, ov])
    faces = np.concatenate([f, np.array([[0, 1, 2], [0, 2, 3]]) + len(v)])
    mat_ids = np.array([0] * 4 + [1] * 8 + [2] * 2, dtype=np.uint8)
    normals = synth.face_normals(verts, faces)[0].astype(np.float32)
    w2c = _look((1.7, -4.0, 1.4), (0.0, 0.0, 0.0))
    h, w = 16, 24
    K = (f32(30.5), f32(29.75), w / 2.0, h / 2.0)
    out = {"verts": verts, "faces": faces, "mat_ids": mat_ids, "normals": normals, "w2c": w2c, "K": K, "h": h, "w": w}
    rm = reproj.RasterMesh(verts, faces, DEV)
    for ss in (1, 2):
        s = rm.view_struct(synth.raster_K(K, ss), w2c, h * ss, w * ss, znear=0.05, zfar=100.0)
        zbuf = torch.empty(h * ss * w * ss, dtype=torch.int64, device=DEV)
        rm.rasterize(s, zbuf)
        d, fc = reproj.resolve(zbuf, h * ss, w * ss)
        out[ss] = (d.cpu().numpy(), fc.cpu().numpy())
    return out


def _box_img(bv, ss, **over):
    rng = np.random.default_rng(8)
    d = _img(rng, bv["h"], bv["w"], ss, fx=bv["K"][0], fy=bv["K"][1], cx=bv["K"][2], cy=bv["K"][3],
             c2w=f32(np.linalg.inv(bv["w2c"])[:3].reshape(-1)), sfm2gt=[1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], light=f32([0.48, -0.64, 0.6]))
    d.update(over)
    return d


def test_shade_bit_for_bit_on_the_rasterized_box(box_view):
    for ss in (1, 2):
        depth, face = box_view[ss]
        rgb, label, dep = _shade_both(depth, face, _box_img(box_view, ss), box_view["normals"], box_view["mat_ids"])
        assert {1, 42, 12, SKY} == set(np.unique(label).tolist())
        assert (dep > 0).sum() > 40 and ((label == 12) == np.isin(face[ss // 2::ss, ss // 2::ss], (12, 13))).all()


# ---------------------------------------------------------------------------------------------------
# 2. observe
# ---------------------------------------------------------------------------------------------------
H_, W_ = 48, 64
KO = (50.0, 52.0, W_ / 2.0, H_ / 2.0)
TOL, ZN, SIG = 1e-3, 0.25, 0.6


def _obs_case():
    """Camera at the world's origin looking along +z (camera = world: the edge cases are exact), a depth plane of 5 with holes
    and a nearer occluder block."""
    rng = np.random.default_rng(11)
    depth = np.full((H_, W_), 5.0, dtype=np.float32)
    depth[10:14, 20:30] = 0.0
    depth[30:40, 40:50] = 2.0  # an occluder
    fx, fy, cx, cy = KO
    pts, nrm = [], []

    def add(u, v, z, n=(0.0, 0.0, -1.0)):
        pts.append([(u - cx) * z / fx, (v - cy) * z / fy, z])
        nrm.append(list(n))

    for z in (-1.0, 0.0, ZN, np.nextafter(ZN, 1.0), np.nextafter(ZN, 0.0)):  # behind, in the plane, exactly at znear, either side
        add(30.0, 20.0, z)
    for e in (-1e-6, 1e-6, 0.0):  # either side of half a pixel outside each border, then the border itself
        for u, v in ((-0.5 + e, 20.0), (W_ - 0.5 + e, 20.0), (30.0, -0.5 + e), (30.0, H_ - 0.5 + e), (-0.5 + e, -0.5 + e),
                     (W_ - 0.5 + e, H_ - 0.5 + e)):
            add(u, v, 5.0)
    add(25.0, 12.0, 5.0)                      # over a hole
    add(45.0, 35.0, 5.0)                      # behind the occluder
    add(45.0, 35.0, 2.0)                      # on it
    add(30.0, 20.0, 5.0, (0.0, 0.0, 1.0))     # back-facing
    add(32.0, 20.0, 5.0, (1.0, 0.0, 0.0))     # edge-on, on the axis: n . (c - p) = -x = 0 exactly, which is not facing
    for k in (0.5, 0.999, 1.0, 1.001, 2.0):   # |z - d| on either side of depth_tol z
        for sgn in (-1, 1):
            add(30.0, 20.0, 5.0 / (1.0 - sgn * k * TOL))
    m = 1000 - len(pts)
    u, v = rng.uniform(-4, W_ + 4, m), rng.uniform(-4, H_ + 4, m)
    z = np.where(rng.uniform(size=m) < 0.7, 5.0 * (1 + rng.uniform(-2, 2, m) * TOL), rng.uniform(-1, 8, m))
    for a, b, c in zip(u, v, z):
        n = rng.normal(size=3)
        add(a, b, c, n / np.linalg.norm(n))
    return np.array(pts), np.array(nrm), depth


def _observe_both(pts, nrm, index, w2c, depth, serial=3, seed=(7 << 32) | 9, chunk=None):
    vs = synth.view_struct(w2c, KO, H_, W_, ZN, SIG, TOL, seed, serial)
    got = synth.observe(torch.from_numpy(pts).to(DEV), torch.from_numpy(nrm).to(DEV), torch.from_numpy(index).to(DEV), vs,
                        torch.from_numpy(depth).to(DEV), chunk=chunk)
    M = np.asarray(w2c, dtype=np.float64)[:3, :4]
    view = {"w2c": M.reshape(-1).tolist(), "centre": (-M[:, :3].T @ M[:, 3]).tolist(), "fx": KO[0], "fy": KO[1], "cx": KO[2],
            "cy": KO[3], "znear": ZN, "sigma_r3": SIG * float(np.sqrt(3.0)), "depth_tol": TOL, "seed": seed, "serial": serial,
            "height": H_, "width": W_}
    xy, err2, vis = R.observe(pts, nrm, index, view, depth)
    want = (xy, np.sqrt(err2), vis)
    for g, w_, name in zip(got, want, ("xy", "err", "vis")):
        assert torch.equal(g.cpu(), torch.from_numpy(w_)), name
    return want


def test_observe_bit_for_bit_edges_and_sizes():
    pts, nrm, depth = _obs_case()
    index = np.arange(len(pts), dtype=np.int64) + (1 << 33)  # indices past 32 bits reach the second counter word
    eye = np.eye(4)
    xy, err, vis = _observe_both(pts, nrm, index, eye, depth)
    front = pts[:, 2] > ZN
    assert front[:5].tolist() == [False, False, False, True, False]  # z > znear, strictly: only the fourth is projected at all
    assert (xy[~front] == 0).all() and (err[~front] == 0).all() and (vis[~front] == 0).all() and (xy[front] != 0).all()
    assert err[front].max() <= 2 * np.sqrt(6.0) * SIG and err[front].min() > 0
    assert vis[5:17].tolist() == [0, 1, 0, 1, 0, 1] + [1, 0, 1, 0, 1, 0]  # floor(u + 0.5) on both sides of every border
    assert vis[23:28].tolist() == [0, 0, 1, 0, 0]                          # hole, occluded, on the occluder, back-facing, edge-on
    assert vis[28:32].tolist() == [1, 1, 1, 1] and vis[34:38].tolist() == [0, 0, 0, 0] and 0 < vis[38:].mean() < 1
    for n in (1, 63, 64, 65):
        _observe_both(pts[:n], nrm[:n], index[:n], eye, depth)
    # a general pose, and independence of the split into calls and of the run
    w2c = _look((0.3, -0.2, 0.1), (0.1, 0.2, 5.0))
    base = _observe_both(pts, nrm, index, w2c, depth)
    again = _observe_both(pts, nrm, index, w2c, depth, chunk=7)
    for a, b in zip(base, again):
        assert np.array_equal(a, b)
    _observe_both(pts[:65], nrm[:65], index[:65], w2c, depth, chunk=1)
    other = _observe_both(pts, nrm, index, w2c, depth, serial=4)
    assert not np.array_equal(other[0], base[0]) and np.array_equal(other[2], base[2])  # another view serial: other noise, same visibility
    lib = L.get_lib()
    vs = synth.view_struct(eye, KO, H_, W_, ZN, SIG, TOL, 1, 1)
    t = torch.zeros(8, dtype=torch.float64, device=DEV)
    assert lib.ncw_synth_observe(None, None, None, 0, None, None, None, None, None, None) == 0
    assert lib.ncw_synth_observe(L.ptr(t), L.ptr(t), L.ptr(t), 1, C.byref(vs), None, L.ptr(t), L.ptr(t), L.ptr(t), None) == -1
    vs.znear = 0.0
    assert lib.ncw_synth_observe(L.ptr(t), L.ptr(t), L.ptr(t), 1, C.byref(vs), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), None) == -1
    img = _struct(_img(np.random.default_rng(0), 2, 2, 5))
    assert lib.ncw_synth_shade(L.ptr(t), L.ptr(t), C.byref(img), L.ptr(t), L.ptr(t), 1, L.ptr(t), 1, L.ptr(t), L.ptr(t), L.ptr(t), None) == -1


# ---------------------------------------------------------------------------------------------------
# 3. the image is the one the project's rays see
# ---------------------------------------------------------------------------------------------------
def test_the_image_is_the_one_view_rays_sees(box_view):
    """Every covered pixel's ray of views.view_rays, scaled to the shaded depth, lands on the plane of the face the pixel shows.
    The yardstick is the float32 restatement's own point (camera point -> world, sfm2gt = identity) for the same depth plane:
    its residual against the plane is what float32 and the rasterizer's depth leave (the float64 run of the restatement shows
    the depth's share alone); the rays may use 4 x that.  With cx, cy NOT shifted for the rasterizer -- the restatement fed
    the image point of the raster sample, half a pixel further -- the residual is far beyond the bound: the test sees the
    half pixel."""
    bv = box_view
    depth_ss, face_ss = bv[1]
    d = _box_img(bv, 1)
    tab = synth.material_table(MATS, DEV)
    _, _, depth = synth.shade(torch.from_numpy(depth_ss).to(DEV), torch.from_numpy(face_ss).to(DEV), _struct(d),
                              torch.from_numpy(bv["normals"]).to(DEV), torch.from_numpy(bv["mat_ids"]).to(DEV), tab, len(MATS))
    depth = depth.cpu().numpy().astype(np.float64)
    cov = depth > 0
    assert cov.sum() > 40
    fc = face_ss[cov]
    n, _ = synth.face_normals(bv["verts"], bv["faces"])
    v0 = bv["verts"][bv["faces"][:, 0]]
    resid = lambda p: np.abs((n[fc] * (p - v0[fc])).sum(1))
    c2w_cv = np.linalg.inv(bv["w2c"])[:3]
    c2w = c2w_cv.copy()
    c2w[:, 1:3] *= -1  # the renderer's "right up back" axes (views.image_pose)
    Kc = np.array([[bv["K"][0], 0, bv["K"][2]], [0, bv["K"][1], bv["K"][3]], [0, 0, 1]])
    rays = views.view_rays(views.Camera(Kc, c2w, bv["w"], bv["h"], 0.1, 10.0), device=DEV).cpu().numpy().astype(np.float64)
    o, dr = rays[:, :3].reshape(bv["h"], bv["w"], 3)[cov], rays[:, 3:6].reshape(bv["h"], bv["w"], 3)[cov]
    fwd = c2w_cv[:, 2]
    p_ray = o + dr * (depth[cov] / (dr @ fwd))[:, None]
    p32 = R.shade(depth_ss, face_ss, d, bv["normals"], bv["mat_ids"], MATS, np.float32, with_points=True)[3][cov].astype(np.float64)
    p64 = R.shade(depth_ss, face_ss, d, bv["normals"], bv["mat_ids"], MATS, np.float64, with_points=True)[3][cov]
    wrong = dict(d, cx=d["cx"] - 0.5, cy=d["cy"] - 0.5)
    p_wrong = R.shade(depth_ss, face_ss, wrong, bv["normals"], bv["mat_ids"], MATS, np.float32, with_points=True)[3][cov].astype(np.float64)
    r_ray, r32, r64, r_wrong = resid(p_ray).max(), resid(p32).max(), resid(p64).max(), resid(p_wrong).max()
    print("plane residuals: rays %.3e, restatement f32 %.3e, f64 %.3e, without the half pixel %.3e" % (r_ray, r32, r64, r_wrong))
    assert r_wrong > 1000 * r32  # on the host: the restatement alone shows that half a pixel is visible
    assert r_ray <= 4 * r32


# ---------------------------------------------------------------------------------------------------
# 4 - 6. one generated scene
# ---------------------------------------------------------------------------------------------------
GEN = dict(seed=0, n_views=6, size=(96, 72), n_points=2000, n_gt=20000, ss=2, max_edge=2.0, num_test=1, pixel_sigma=0.5)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("synth") / "facade")
    info = synth.generate(root, device=DEV, **GEN)
    return {"root": root, "info": info, "truth": json.load(open(os.path.join(root, "truth.json")))}


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_the_scene_is_one(scene, tmp_path):
    root = scene["root"]
    from PIL import Image

    sc = views.read_scene(root, "sparse", with_points=True)
    assert len(sc["ids"]) == GEN["n_views"] and len(sc["ids_train"]) == GEN["n_views"] - GEN["num_test"]
    cams = sceneprep.scene_cameras(root)
    assert len(cams) == GEN["n_views"]
    allowed = set(scene["truth"]["labels"])
    assert {synth.labels.label_id("sky"), synth.labels.label_id("person"), synth.labels.label_id("road")} <= allowed
    seen = set()
    for iid in sc["ids"]:
        im = sc["images"][iid]
        p = sc["cams"][im["camera_id"]]["params"]
        with Image.open(os.path.join(root, "dense", "images", im["name"])) as img:
            assert img.size == (int(2 * p[2]), int(2 * p[3])) and img.size[0] <= 96 and img.size[1] <= 72
            size = img.size
        lab = np.load(os.path.join(root, "semantic_maps", im["name"].split(".")[0] + ".npz"))["arr_0"]
        assert lab.dtype == np.uint8 and lab.shape == (size[1], size[0]) and set(np.unique(lab).tolist()) <= allowed
        seen |= set(np.unique(lab).tolist())
        K, w2c, c2w, w_, h_ = views.image_pose(sc, iid, 1)
        assert (w_, h_) == size
    assert synth.labels.label_id("person") in seen and synth.labels.label_id("sky") in seen
    tsv, rows = colmap.split_rows(root)
    assert sum(r["split"] == "test" for r in rows) == GEN["num_test"] and len(rows) == GEN["n_views"]
    ids, xyz, err, track = colmap.read_points3d(os.path.join(root, "dense", "sparse", "points3D.bin"))
    assert len(ids) == scene["truth"]["n_points3d"] > 100 and track.min() >= 2
    cfg = yaml.safe_load(open(os.path.join(root, "config.yaml")))
    assert np.allclose(np.array(cfg["sfm2gt"]), np.array(scene["truth"]["sfm2gt"]), rtol=0, atol=0)
    tr = yaml.safe_load(open(os.path.join(root, "train.yaml")))
    assert tr["NEUCONW"]["N_VOCAB"] >= max(sc["ids"]) + 1 and tr["DATASET"]["ROOT_DIR"] == root
    with pytest.raises(FileExistsError):
        synth.generate(root, device=DEV, **GEN)
    # the same arguments give the same bytes: generate again at the same path, beside a copy of the first
    first = str(tmp_path / "first")
    shutil.copytree(root, first)
    synth.generate(root, device=DEV, overwrite=True, **GEN)
    names = _files(first)
    assert names == _files(root) and len(names) == 2 * GEN["n_views"] + 3 + 6
    match, mismatch, errors = filecmp.cmpfiles(first, root, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


def test_known_answers(scene, tmp_path):
    root, truth = scene["root"], scene["truth"]
    sp = os.path.join(root, "dense", "sparse")
    images = colmap.read_images(os.path.join(sp, "images.bin"), with_points=True)
    cams = colmap.read_cameras(os.path.join(sp, "cameras.bin"))
    ids, xyz, err, track, start, t_img, t_idx = colmap.read_points3d(os.path.join(sp, "points3D.bin"), with_tracks=True)
    outl = set(truth["outlier_point_ids"])
    assert outl and outl <= set(ids.tolist())
    bound = 2 * np.sqrt(6.0) * GEN["pixel_sigma"] + 1e-9
    worst, tracked = 0.0, set()
    for i in range(len(ids)):
        for e in range(int(start[i]), int(start[i + 1])):
            im = images[int(t_img[e])]
            assert im["point3d_ids"][t_idx[e]] == ids[i]
            tracked.add(int(t_img[e]))
            if int(ids[i]) in outl:
                continue
            p = cams[im["camera_id"]]["params"]
            c = colmap.qvec2rotmat(im["qvec"]) @ xyz[i] + im["tvec"]
            uv = np.array([p[0] * c[0] / c[2] + p[2], p[1] * c[1] / c[2] + p[3]])
            worst = max(worst, float(np.linalg.norm(uv - im["xys"][t_idx[e]])))
    print("worst reprojection distance %.4f px (bound %.4f)" % (worst, bound))
    assert worst <= bound and tracked == set(images)
    inl = np.array([int(i) not in outl for i in ids])
    assert track[~inl].max() <= 2 and err[~inl].min() >= 5.0 and err[inl].max() <= bound and (np.diff(start) == track).all()
    # a property of the rig: every view looks at the scene's sphere
    cfg = yaml.safe_load(open(os.path.join(root, "config.yaml")))
    shares, _ = sceneprep.roi_shares(sceneprep.scene_cameras(root), cfg["origin"], cfg["radius"], DEV)
    print("roi shares", np.round(shares, 3).tolist())
    assert shares.min() >= 0.5  # prepare_split's default roi_threshold
    # GT points lie on the mesh: exact recall 1 at 1e-3 GT units (float32 rounding of the written clouds is about 1e-5) ...
    work = str(tmp_path / "eval")
    os.makedirs(work)
    pred = os.path.join(work, "mesh.ply")
    shutil.copy(os.path.join(root, "mesh.ply"), pred)
    m = evalmesh.eval_mesh(pred, os.path.join(root, "gt.ply"), cfg, True, threshold=1e-3, exact_recall=True, device=DEV, verbose=False)
    assert m["recal"] == 1.0
    # ... and the same mesh 0.05 off along (1, 1, 1) / sqrt(3) loses more than half of it
    v, f, _ = ply.read_mesh(pred)
    T = np.array(cfg["sfm2gt"])
    shift = np.linalg.inv(T[:3, :3]) @ (0.05 * np.ones(3) / np.sqrt(3.0))
    off = os.path.join(work, "shifted.ply")
    ply.write(off, v + shift, faces=f)
    m2 = evalmesh.eval_mesh(off, os.path.join(root, "gt.ply"), cfg, True, threshold=1e-3, exact_recall=True, save_name="shifted",
                            device=DEV, verbose=False)
    print("recall: on the mesh %.4f, shifted %.4f" % (m["recal"], m2["recal"]))
    assert m2["recal"] < 0.5


def test_it_trains(scene):
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import config, raysource
    from PIL import Image

    root = scene["root"]
    src = raysource.RaySource.from_scene(root, 1, "semantic_maps", "sparse", ray_mask_list=["person"], prefilter=True, device=DEV)
    assert len(src) > 1000
    b = src.batch(None)
    sc = views.read_scene(root, "sparse")
    assert set(b["ts"].unique().tolist()) == set(sc["ids_train"])
    pix = raysource.unpack_records(src.recs.cpu())[0].numpy()
    ts, rgbs, sem = b["ts"].cpu().numpy(), b["rgbs"].cpu().numpy(), b["semantics"].cpu().numpy()
    person = synth.labels.label_id("person")
    assert bool(b["keep"].all()) and person not in set(np.unique(sem).tolist()) and set(np.unique(sem).tolist()) <= set(scene["truth"]["labels"])
    for iid in sc["ids_train"]:
        name = sc["images"][iid]["name"]
        img = np.asarray(Image.open(os.path.join(root, "dense", "images", name)).convert("RGB"))
        lab = np.load(os.path.join(root, "semantic_maps", name.split(".")[0] + ".npz"))["arr_0"]
        rows = ts == iid
        assert rows.any()
        assert np.array_equal(np.rint(rgbs[rows] * 255.0).astype(np.uint8), img.reshape(-1, 3)[pix[rows]])
        assert np.array_equal(sem[rows], lab.reshape(-1)[pix[rows]].astype(np.int64))
    over = {"NEUCONW": {"N_SAMPLES": 8, "N_IMPORTANCE": 8, "UP_SAMPLE_STEP": 2, "N_OUTSIDE": 4, "N_A": 16, "ANNEAL_END": 100,
                        "SDF_CONFIG": {"d_out": 65, "d_hidden": 64}, "COLOR_CONFIG": {"d_feature": 64, "d_hidden": 64, "head_channels": 32},
                        "S_CONFIG": {"init_val": 0.3}}}
    cfg = config.load_config(os.path.join(root, "train.yaml"), over)
    torch.manual_seed(0)
    emb, neuconw, nerf, rdr, _ = config.build_system(cfg, torch.device(DEV), nw.PREC_F32)
    step = nw.TrainStep(rdr, [emb, neuconw, nerf], config.neuconw_loss(cfg), lr=1e-4, eps=1e-7, clip=0.99)
    idx = torch.arange(0, len(src), max(1, len(src) // 256), device=DEV)[:256]
    bb = src.batch(idx)
    loss, _ = step(bb["rays"], bb["ts"], bb["semantics"], bb["rgbs"], background_rgb=torch.zeros(1, 3, device=DEV), cos_anneal_ratio=0.0)
    assert np.isfinite(float(loss.detach()))
