"""Host side of the synthetic scenes (no GPU): the COLMAP writers against the readers, the restatement's value noise and pixel
noise, the facade mesh, the similarity, and the ABI step."""
import os

import numpy as np
import pytest

from neuralrecon_w_amd import colmap, synth
from tests import _synth_ref as R


# ---------------------------------------------------------------------------------------------------
# writers -> readers
# ---------------------------------------------------------------------------------------------------
def test_cameras_round_trip_and_size(tmp_path):
    cams = {7: {"model": 1, "width": 1024, "height": 768, "params": np.array([800.25, 801.5, 512.0, 384.0])},
            1: {"model": 1, "width": 2, "height": 2, "params": np.array([1.0, 1.0, 1.0, 1.0])},
            2 ** 31 - 1: {"model": 1, "width": 2 ** 40, "height": 3, "params": np.array([1e-300, 1e300, -0.0, np.pi])}}
    p = str(tmp_path / "cameras.bin")
    colmap.write_cameras(p, cams)
    assert os.path.getsize(p) == 8 + len(cams) * (24 + 32)
    back = colmap.read_cameras(p)
    assert list(back) == list(cams)
    for k, c in cams.items():
        assert (back[k]["id"], back[k]["model"], back[k]["width"], back[k]["height"]) == (k, 1, c["width"], c["height"])
        assert back[k]["params"].tobytes() == c["params"].tobytes()
    colmap.write_cameras(p, [dict(c, id=k) for k, c in cams.items()])  # the list form writes the same file
    assert list(colmap.read_cameras(p)) == list(cams)


def test_images_round_trip_and_size(tmp_path):
    rng = np.random.default_rng(0)
    q = rng.normal(size=4)
    imgs = {3: {"qvec": q / np.linalg.norm(q), "tvec": rng.normal(size=3), "camera_id": 9, "name": "a.png"},
            1: {"qvec": np.array([1.0, 0, 0, 0]), "tvec": np.zeros(3), "camera_id": 1, "name": "Zwölf Säulen 柱.jpg",
                "xys": rng.uniform(0, 100, (257, 2)), "point3d_ids": rng.integers(-1, 2 ** 40, 257)},
            2: {"qvec": np.array([0.0, 1, 0, 0]), "tvec": np.ones(3), "camera_id": 2, "name": "", "xys": np.zeros((0, 2)),
                "point3d_ids": np.zeros(0, dtype=np.int64)}}
    p = str(tmp_path / "images.bin")
    colmap.write_images(p, imgs)
    size = 8 + sum(64 + len(im["name"].encode("utf-8")) + 1 + 8 + 24 * len(im.get("xys", ())) for im in imgs.values())
    assert os.path.getsize(p) == size
    back = colmap.read_images(p, with_points=True)
    assert list(back) == list(imgs)
    for k, im in imgs.items():
        b = back[k]
        assert (b["id"], b["camera_id"], b["name"]) == (k, im["camera_id"], im["name"])
        assert b["qvec"].tobytes() == np.asarray(im["qvec"], dtype=np.float64).tobytes() and b["tvec"].tobytes() == im["tvec"].tobytes()
        xys = np.asarray(im.get("xys", np.zeros((0, 2))))
        assert b["xys"].shape == xys.shape and b["xys"].tobytes() == xys.tobytes()
        assert np.array_equal(b["point3d_ids"], np.asarray(im.get("point3d_ids", np.zeros(0)), dtype=np.int64))
    assert [im["name"] for im in colmap.read_images(p).values()] == [im["name"] for im in imgs.values()]


def test_points3d_round_trip_and_size(tmp_path):
    rng = np.random.default_rng(1)
    lens = np.array([0, 1, 300, 2, 0])
    n, T = len(lens), int(lens.sum())
    ids = np.array([5, 2 ** 40, 1, 7, 3])
    xyz, err = rng.normal(size=(n, 3)), rng.uniform(0, 3, n)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    start = np.concatenate([[0], np.cumsum(lens)])
    t_img, t_idx = rng.integers(1, 1000, T).astype(np.int32), rng.integers(0, 5000, T).astype(np.int32)
    p = str(tmp_path / "points3D.bin")
    colmap.write_points3d(p, ids, xyz, rgb, err, start, t_img, t_idx)
    assert os.path.getsize(p) == 8 + 51 * n + 8 * T
    b = colmap.read_points3d(p, with_tracks=True)
    assert np.array_equal(b[0], ids) and b[1].tobytes() == xyz.tobytes() and b[2].tobytes() == err.tobytes()
    assert np.array_equal(b[3], lens) and np.array_equal(b[4], start) and np.array_equal(b[5], t_img) and np.array_equal(b[6], t_idx)
    raw = open(p, "rb").read()
    assert raw[8 + 32:8 + 35] == rgb[0].tobytes()  # the colour bytes sit between xyz and the error


def test_writers_refuse(tmp_path):
    p = str(tmp_path / "x.bin")
    with pytest.raises(ValueError, match="NUL"):
        colmap.write_images(p, {1: {"qvec": [1, 0, 0, 0], "tvec": [0, 0, 0], "camera_id": 1, "name": "a\x00b.png"}})
    with pytest.raises(ValueError, match="PINHOLE"):
        colmap.write_cameras(p, {1: {"model": 2, "width": 4, "height": 4, "params": [1.0, 2.0, 2.0, 0.1]}})
    with pytest.raises(ValueError, match="PINHOLE"):
        colmap.write_cameras(p, {1: {"model": 1, "width": 4, "height": 4, "params": [1.0, 2.0, 2.0]}})
    z3, c3 = np.zeros((2, 3)), np.zeros((2, 3), dtype=np.uint8)
    for bad in (dict(start=[0, 1, 2], img=[1, 2, 3], idx=[0, 0]), dict(start=[0, 1, 2], img=[1, 2], idx=[0, 0, 0]),
                dict(start=[0, 1], img=[1], idx=[0]), dict(start=[0, 1, 3], img=[1, 2], idx=[0, 0])):
        with pytest.raises(ValueError, match="write_points3d"):
            colmap.write_points3d(p, [1, 2], z3, c3, [0.0, 0.0], bad["start"], bad["img"], bad["idx"])
    with pytest.raises(ValueError, match="write_points3d"):
        colmap.write_points3d(p, [1, 2], np.zeros((3, 3)), c3, [0.0, 0.0], [0, 0, 0], [], [])
    with pytest.raises(ValueError, match="2-D points"):
        colmap.write_images(p, {1: {"qvec": [1, 0, 0, 0], "tvec": [0, 0, 0], "camera_id": 1, "name": "a", "xys": np.zeros((2, 2)),
                                    "point3d_ids": [1]}})


def test_rotmat2qvec_inverts_qvec2rotmat():
    rng = np.random.default_rng(2)
    for q in list(rng.normal(size=(50, 4))) + [np.array([0.0, 1, 0, 0]), np.array([0, 0, 1.0, 0]), np.array([0, 0, 0, 1.0]), np.array([1e-9, 1, 1, 1])]:
        q = q / np.linalg.norm(q)
        Rm = colmap.qvec2rotmat(q)
        assert np.abs(colmap.qvec2rotmat(colmap.rotmat2qvec(Rm)) - Rm).max() < 1e-14


# ---------------------------------------------------------------------------------------------------
# the restatement's noise
# ---------------------------------------------------------------------------------------------------
def test_value_noise_hits_the_hash_and_is_continuous():
    rng = np.random.default_rng(3)
    for F in (np.float32, np.float64):
        i = rng.integers(-1000, 1000, (200, 3))
        at = R.value_noise(i.astype(F), seed=5, octave=1, dtype=F)
        assert np.array_equal(at, R.lattice(i[:, 0], i[:, 1], i[:, 2], 5, 1, F))  # t = 0: the lattice value itself
        assert (at >= 0).all() and (at < 1).all()
        # across a cell face: t -> 1 of one cell equals t = 0 of the next, in every axis
        for ax in range(3):
            q = (i + rng.uniform(0, 1, i.shape)).astype(F)
            q[:, ax] = i[:, ax]
            below = q.copy()
            below[:, ax] = np.nextafter(q[:, ax], F(-np.inf))  # the last float of the cell below
            a, b = R.value_noise(q, 5, 1, F), R.value_noise(below, 5, 1, F)
            assert np.abs(a - b).max() <= 1000 * np.finfo(F).eps * 4, (F, ax)  # |coordinate| <= 1000: t is 1 - O(1000 eps)
    assert not np.array_equal(R.value_noise(i.astype(np.float32), 5, 1), R.value_noise(i.astype(np.float32), 6, 1))
    assert not np.array_equal(R.value_noise(i.astype(np.float32), 5, 1), R.value_noise(i.astype(np.float32), 5, 2))


def test_uniform_sum_noise_moments_and_bound():
    n, sigma = 100000, 0.7
    s3 = sigma * np.sqrt(3.0)
    for call in (0, 1):
        x = s3 * R.usum4(np.arange(n), serial=3, call=call, seed=(9 << 32) | 11)
        # standard errors: of the mean sigma / sqrt(n); of the variance sqrt((m4 - sigma^4) / n) with the uniform sum's
        # fourth moment m4 = sigma^4 (3 - 6 / (5 * 4)) = 2.7 sigma^4
        assert abs(x.mean()) <= 5 * sigma / np.sqrt(n)
        assert abs(x.var() - sigma ** 2) <= 5 * np.sqrt(1.7 * sigma ** 4 / n)
        assert np.abs(x).max() <= 2 * np.sqrt(3.0) * sigma
    a = R.usum4(np.arange(100), 3, 0, 1)
    assert np.array_equal(a[10:20], R.usum4(np.arange(10, 20), 3, 0, 1))  # keyed by the index alone
    assert not np.array_equal(a, R.usum4(np.arange(100), 4, 0, 1)) and not np.array_equal(a, R.usum4(np.arange(100), 3, 1, 1))


# ---------------------------------------------------------------------------------------------------
# mesh and frames
# ---------------------------------------------------------------------------------------------------
def test_facade_mesh():
    for seed, max_edge in ((0, 2.0), (3, 0.9)):
        m = synth.facade_mesh(seed, max_edge)
        assert m.faces.min() >= 0 and m.faces.max() < len(m.verts) and len(m.material) == len(m.faces)
        assert m.material.max() < len(m.materials)
        n, area2 = synth.face_normals(m.verts, m.faces)
        assert area2.min() > 1e-9
        edges = np.concatenate([np.linalg.norm(m.verts[m.faces[:, i]] - m.verts[m.faces[:, (i + 1) % 3]], axis=1) for i in range(3)])
        assert edges.max() <= max_edge * (1 + 1e-12)
        ground = m.material == synth.MATERIAL_ID["ground"]
        assert ground.any() and (n[ground, 2] > 0.999999).all()
        assert m.materials[synth.MATERIAL_ID["ground"]]["label"] == synth.labels.label_id("road")
        # outward: seen from far away along its normal's side, no face of the closed parts points back at the building's axis
        lo, hi = synth.building_box(m)
        assert lo[2] == 0.0 and hi[2] > 5.0
        m2 = synth.facade_mesh(seed, max_edge)
        assert np.array_equal(m.verts, m2.verts) and np.array_equal(m.faces, m2.faces) and np.array_equal(m.material, m2.material)
    assert not np.array_equal(synth.facade_mesh(0, 2.0).verts, synth.facade_mesh(1, 2.0).verts)


def test_box_and_cylinder_faces_look_outward():
    b = synth._Builder(0.7)
    b.box((1.0, 2.0, 3.0), (2.0, 4.0, 6.0), 0)
    v, f = np.concatenate(b.v), np.concatenate(b.f)
    n, _ = synth.face_normals(v, f)
    assert ((n * (v[f].mean(1) - np.array([1.5, 3.0, 4.5]))).sum(1) > 0).all()
    c = synth._Builder(0.3)
    c.cylinder(1.0, -2.0, 0.0, 2.0, 0.4, 0)
    v, f = np.concatenate(c.v), np.concatenate(c.f)
    n, _ = synth.face_normals(v, f)
    out = v[f].mean(1) - np.array([1.0, -2.0, 0.0])
    out[:, 2] = 0
    assert ((n * out).sum(1) > 0).all() and np.abs(n[:, 2]).max() < 1e-12


def test_load_mesh_materials(tmp_path):
    from neuralrecon_w_amd import ply

    b = synth._Builder(1e9)
    b.box((0.0, 0.0, 0.0), (1.0, 2.0, 3.0), 0)
    v, f = np.concatenate(b.v), np.concatenate(b.f)
    f = np.concatenate([f, [[0, 0, 1]]])  # a zero-area face is dropped
    p = str(tmp_path / "m.ply")
    ply.write(p, v, faces=f)
    m = synth.load_mesh(p)
    assert len(m.faces) == 12 and len(m.materials) == 1 and (m.material == 0).all() and m.materials[0]["label"] == synth.labels.label_id("building")
    rgb = np.zeros((len(v), 3), dtype=np.uint8)
    rgb[f[:4].reshape(-1)] = [255, 0, 0]  # the first two quads red, the rest black
    ply.write(p, v, faces=f, rgb=rgb)
    m = synth.load_mesh(p)
    assert len(m.materials) == 2 and sorted(np.bincount(m.material).tolist()) == [4, 8]
    assert sorted(tuple(x["base"]) for x in m.materials) == [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0)]
    with pytest.raises(ValueError, match="no faces"):
        ply.write(p, v)
        synth.load_mesh(p)


def test_sfm2gt_is_a_similarity_and_inverts():
    m = synth.facade_mesh(0, 2.0)
    lo, hi = synth.building_box(m)
    ext = float(np.linalg.norm(m.verts.max(0) - m.verts.min(0)))
    for seed in range(5):
        T = synth.random_sfm2gt(seed, (lo + hi) / 2, float(np.linalg.norm(hi - lo)))
        A = T[:3, :3]
        s = np.sqrt((A[0] ** 2).sum())
        assert 3.0 <= s <= 8.0 and np.abs(A @ A.T / s ** 2 - np.eye(3)).max() < 1e-14 and np.linalg.det(A) > 0
        inv = synth.invert_similarity(T)
        x_sfm = m.verts @ inv[:3, :3].T + inv[:3, 3]
        back = x_sfm @ T[:3, :3].T + T[:3, 3]
        assert np.abs(back - m.verts).max() <= 1e-12 * ext
    assert np.array_equal(synth.random_sfm2gt(1, lo, 1.0), synth.random_sfm2gt(1, lo, 1.0))


def test_cameras_keep_the_principal_point_at_the_centre():
    m = synth.facade_mesh(0, 2.0)
    lo, hi = synth.building_box(m)
    T = synth.random_sfm2gt(0, (lo + hi) / 2, 1.0)
    for c in synth.make_cameras(0, 12, (96, 72), lo, hi):
        fx, fy, cx, cy = c["K"]
        assert c["width"] % 2 == 0 and c["height"] % 2 == 0 and c["width"] <= 96 and c["height"] <= 72
        assert int(2 * cx) == c["width"] and int(2 * cy) == c["height"] and cx == c["width"] / 2 and cy == c["height"] / 2
        Rm, t = synth.to_sfm_pose(c["w2c"], T)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14
        # the same camera point, by the GT pose and by the SfM pose, differs by the scale alone
        x_gt = (lo + hi) / 2
        inv = synth.invert_similarity(T)
        x_sfm = inv[:3, :3] @ x_gt + inv[:3, 3]
        s = np.sqrt((T[0, :3] ** 2).sum())
        assert np.abs((Rm @ x_sfm + t) * s - (c["w2c"][:3, :3] @ x_gt + c["w2c"][:3, 3])).max() < 1e-10


def test_train_overrides_are_keys_of_the_defaults():
    from neuralrecon_w_amd import config

    def walk(over, base, path=""):
        for k, v in over.items():
            assert k in base, path + k
            if isinstance(v, dict):
                walk(v, base[k], path + k + ".")

    o = synth.train_overrides("some/scene", 7)
    walk(o, config.DEFAULTS)
    assert o["NEUCONW"]["N_VOCAB"] == 7 and o["NEUCONW"]["RAY_MASK_LIST"] == ["person"]
    assert (o["NEUCONW"]["N_SAMPLES"], o["NEUCONW"]["N_IMPORTANCE"], o["NEUCONW"]["SDF_CONFIG"]["d_hidden"]) == (64, 64, 256)


def test_abi_has_the_synth_entry_points():
    from neuralrecon_w_amd import lib as L

    assert {"ncw_synth_shade", "ncw_synth_observe"} <= set(L.exported_symbols()) and L.ABI_VERSION >= 39
