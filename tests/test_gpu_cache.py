"""GPU: the ray-cache writer -- `ncw_sfm_depth_splat`, `ncw_cache_rows` (csrc/ncw_cache.hip) and neuralrecon_w_amd.cachebuild --
against the rows the reference's own dataset produced on CPU for tests/golden/cache_scene (tests/golden/make_golden_cache.py),
the fp64 slab oracle for the octree columns, today's separate launches, and end to end into files that RayCache reads back.

Row layout here: o(3) d(3) near far ts [label] depth weight 0 (13 / 12 columns); the reference's rows are the same without the
last column (12 / 11), so they are compared column by column."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "golden", "cache_scene")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(HERE, "golden", "cache_golden.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def octrees():
    """The two SfM octrees of the scene's config.yaml, as build_cache makes them."""
    import yaml

    from neuralrecon_w_amd import voxel

    with open(os.path.join(SCENE, "config.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    hit = voxel.octree_from_sfm(SCENE, cfg["min_track_length"], cfg["voxel_size"], DEV, sfm_path="sparse", expand=1, radius=1)
    rng = voxel.octree_from_sfm(SCENE, cfg["min_track_length"], cfg["voxel_size"], DEV, sfm_path="sparse", expand=2, radius=1.5)
    assert hit["level"] == 4 and rng["level"] == 4
    return hit, rng, float(cfg["voxel_size"])


def _camera(g, iid):
    from neuralrecon_w_amd import views

    t = "im%d_" % iid
    w, h = g[t + "wh"].tolist()
    return views.Camera(g[t + "K"], g[t + "c2w"], w, h, float(g[t + "near64"]), float(g[t + "far64"]))


def _planes(g, iid):
    from neuralrecon_w_amd import cachebuild

    t = "im%d_" % iid
    w, h = g[t + "wh"].tolist()
    return cachebuild.sfm_depth_planes(g[t + "kp_xyz"], g[t + "kp_err"], g[t + "kp_px"], float(g[t + "err_mean"]), g[t + "w2c"], w, h, DEV)


def _rows(g, iid, with_label=True, hit=None, rng=None, voxel_size=0.0, **kw):
    from neuralrecon_w_amd import cachebuild

    t = "im%d_" % iid
    dz, wt = _planes(g, iid)
    img = torch.from_numpy(g[t + "image"]).to(DEV)
    lab = torch.from_numpy(g[t + "label"]).to(DEV) if with_label else None
    return cachebuild.cache_rows(_camera(g, iid), img, iid, dz, wt, lab, hit, rng, voxel_size, **kw)


# ---------------------------------------------------------------------------------------------------
# 1. the columns that do not depend on the octrees, against the reference's rows
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_label", [True, False])
@pytest.mark.parametrize("iid", [7, 3, 11, 5])
def test_non_voxel_columns_vs_reference(g, iid, with_label):
    t = "im%d_" % iid
    ref = g[t + ("rows13" if with_label else "rows12")]  # the reference's 12 / 11 columns
    rows, rgbs, keep = [x.cpu().numpy() for x in _rows(g, iid, with_label)]
    nc = 13 if with_label else 12
    assert rows.shape == (ref.shape[0], nc) and ref.shape[1] == nc - 1 and rgbs.shape == (ref.shape[0], 3)
    assert keep.all()  # no octrees: use_voxel = False keeps every pixel
    assert np.array_equal(rows[:, 0:3], ref[:, 0:3])  # origins
    assert np.array_equal(rgbs, g[t + "rgbs"])
    assert np.array_equal(rows[:, 6:9], ref[:, 6:9])  # near, far (float32 of the percentiles), ts
    assert np.array_equal(rows[:, 8], np.full(len(rows), float(iid), dtype=np.float32))
    if with_label:
        assert np.array_equal(rows[:, 9], ref[:, 9]) and len(np.unique(rows[:, 9])) > 2
    e_d = np.abs(rows[:, 3:6] - ref[:, 3:6]).max()
    print("image %d: directions max abs err %.2e" % (iid, e_d))
    assert e_d <= 1e-6  # the bound tests/test_gpu_view_rays.py holds for the same arithmetic
    assert np.array_equal(rows[:, nc - 1], np.zeros(len(rows), dtype=np.float32))  # the column nothing reads
    # key-point depth and weight: no further from the float64 evaluation than twice the reference's own float32 rows are (we
    # round in a different order, not with more error)
    d, w, rd, rw = rows[:, nc - 3].astype(np.float64), rows[:, nc - 2].astype(np.float64), ref[:, nc - 3].astype(np.float64), ref[:, nc - 2].astype(np.float64)
    d64, w64 = g[t + "depth64"], g[t + "weight64"]
    assert np.array_equal(w != 0, w64 != 0) and np.array_equal(w != 0, rw != 0) and int((w != 0).sum()) > 20
    assert np.array_equal(d != 0, d64 != 0)
    assert (d64 < 0).any()  # a key-point behind the camera is written with its negative depth
    e_ours, e_ref = (np.abs(d - d64).max(), np.abs(w - w64).max()), (np.abs(rd - d64).max(), np.abs(rw - w64).max())
    print("image %d: depth err %.2e (reference %.2e), weight err %.2e (reference %.2e)" % (iid, e_ours[0], e_ref[0], e_ours[1], e_ref[1]))
    assert e_ours[0] <= 2 * e_ref[0] and e_ours[1] <= 2 * e_ref[1]
    # collisions: the last key-point's value (the float64 planes hold it; the generator asserted the reference's CPU run agrees)
    c = g[t + "collisions"]
    assert int(c.sum()) >= 3
    assert np.abs(d[c] - d64[c]).max() <= 2 * e_ref[0] and np.abs(w[c] - w64[c]).max() <= 2 * e_ref[1]


# ---------------------------------------------------------------------------------------------------
# 2. / 3. the octree columns
# ---------------------------------------------------------------------------------------------------
def _oracle(o, d, od, eps):
    from neuralrecon_w_amd import voxel
    from oracle import neuconw_oracle as O

    occ = voxel.dense_from_occupancy(od).cpu()
    origin, scale = od["scene_origin"].double().cpu(), float(od["scale"])
    return [O.ray_voxel_near_far(o, d, occ, origin, scale, margin=m) for m in (0.0, -eps, eps)]  # exact, with grazing, without


@pytest.mark.parametrize("iid", [7, 3, 11, 5])
def test_voxel_columns_vs_slab_oracle_and_separate_launches(g, octrees, iid):
    """The sandwich of tests/test_gpu_voxel.py:92-108 (eps = 2e-3 voxel, tol = 1e-5 scale 5) for keep, near and far of the fused
    rows; then the same rays through views.view_rays + voxel.get_near_far."""
    from neuralrecon_w_amd import views, voxel

    hit, rng, vs = octrees
    rows, _, keep = _rows(g, iid, True, hit, rng, vs)
    base, _, _ = _rows(g, iid, True)
    rows, keep, base = rows.cpu().double(), keep.cpu().bool(), base.cpu().double()
    assert torch.equal(rows[:, :6], base[:, :6]) and torch.equal(rows[:, 8:], base[:, 8:])  # only near / far depend on the octrees
    o, d = rows[:, 0:3], rows[:, 3:6]
    n = len(o)
    eps = 2e-3 * (2.0 / 16)
    ex_h, lo_h, hi_h = _oracle(o, d, hit, eps)
    ex_r, lo_r, hi_r = _oracle(o, d, rng, eps)
    sure_h = ((lo_h[0] > 0) == (hi_h[0] > 0)).reshape(-1)
    sure_r = ((lo_r[0] > 0) == (hi_r[0] > 0)).reshape(-1)
    grazing = ~(sure_h & sure_r)
    print("image %d: %d / %d kept, %d rays decided by a grazing contact" % (iid, int(keep.sum()), n, int(grazing.sum())))
    assert int(grazing.sum()) <= 0.01 * n
    assert torch.equal(keep[sure_h], (ex_h[0] > 0).reshape(-1)[sure_h])
    assert int(keep.sum()) > 50 and int((~keep).sum()) > 50  # the view has kept and dropped pixels
    near, far = rows[:, 6], rows[:, 7]
    # dropped pixels keep the camera's near / far
    assert torch.equal(near[~keep], base[:, 6][~keep]) and torch.equal(far[~keep], base[:, 7][~keep])
    tol = 1e-5 * float(rng["scale"]) * 5.0
    r_hit = (ex_r[0] > 0).reshape(-1)
    k_sure = keep & sure_r
    assert torch.equal((near > 0)[k_sure], r_hit[k_sure])
    assert int((k_sure & ~r_hit).sum()) == 0  # the dilated range octree covers the hit octree: the 0 / 0 rows are tested below
    both = keep & (near > 0) & (lo_r[0] > 0).reshape(-1) & (hi_r[0] > 0).reshape(-1)
    assert int(both.sum()) > 50
    lo_n, hi_n, lo_f, hi_f = [x.reshape(-1)[both] for x in (lo_r[0], hi_r[0], lo_r[1], hi_r[1])]
    assert bool((near[both] >= lo_n - tol).all()) and bool((near[both] <= hi_n + tol).all())
    far_wo = far[both] - vs  # far carries + voxel_size where the range octree hits
    assert bool((far_wo <= lo_f + tol).all()) and bool((far_wo >= hi_f - tol).all())
    miss = keep & ~(near > 0)
    assert bool((far[miss] == 0).all())  # ... and nothing where it misses
    assert bool((far[both] >= near[both]).all())
    # ---- 3. today's launches on the same rays
    cam = _camera(g, iid)
    r8 = views.view_rays(cam, device=DEV)
    hn, _ = voxel.get_near_far(r8[:, 0:3], r8[:, 3:6], hit)
    rn, rf = voxel.get_near_far(r8[:, 0:3], r8[:, 3:6], rng)
    hn, rn, rf = hn.cpu().double().reshape(-1), rn.cpu().double().reshape(-1), rf.cpu().double().reshape(-1)
    e_rays = float((r8[:, :6].cpu().double() - rows[:, :6]).abs().max())  # one shared device function: expected 0
    print("image %d: fused vs view_rays o / d max abs diff %.1e" % (iid, e_rays))
    assert e_rays <= 1e-6
    dis = (hn > 0) != keep
    assert not bool((dis & ~grazing).any())
    bh = keep & (hn > 0) & (near > 0) & (rn > 0)
    assert int(bh.sum()) > 50
    assert bool(((near[bh] - rn[bh]).abs() <= tol).all()) and bool(((far[bh] - (rf[bh] + vs)).abs() <= tol).all())


def test_range_octree_miss_gives_zero_near_far():
    """A kept ray (the hit octree hits) that the range octree misses gets near = far = 0 and NO voxel_size: a dilated octree
    never produces this, so two hand-made occupancies do."""
    from neuralrecon_w_amd import cachebuild, views, voxel

    G = 16
    hit_occ = torch.zeros(G, G, G, dtype=torch.bool)
    hit_occ[6:10, 6:10, 6:10] = True
    rng_occ = torch.zeros(G, G, G, dtype=torch.bool)
    rng_occ[6:10, 6:8, 6:10] = True  # only the lower-y half: rays through the upper half miss it
    origin = [0.0, 0.0, 0.0]
    hit = voxel.occupancy_from_dense(hit_occ.to(DEV), origin, 1.0)
    rng = voxel.occupancy_from_dense(rng_occ.to(DEV), origin, 1.0)
    w, h = 24, 20
    K = np.array([[120.0, 0, 12.0], [0, 120.0, 10.0], [0, 0, 1]])  # the hit cube fills all but three columns
    c2w = np.array([[1.0, 0, 0, 0.0], [0, 1.0, 0, 0.0], [0, 0, 1.0, 3.0]])  # at z = 3 looking down -z ("right up back")
    cam = views.Camera(K, c2w, w, h, 0.5, 6.0)
    img = torch.zeros(h, w, 3, dtype=torch.uint8, device=DEV)
    dz, wt = cachebuild.sfm_depth_planes(None, None, np.zeros((0, 2), np.int32), float("nan"), np.eye(4), w, h, DEV)
    assert not bool(dz.any()) and not bool(wt.any())
    rows, _, keep = cachebuild.cache_rows(cam, img, 4, dz, wt, None, hit, rng, 0.25)
    rows, keep = rows.cpu(), keep.cpu().bool()
    zero = keep & (rows[:, 6] == 0)
    assert int(zero.sum()) > 20 and int((keep & (rows[:, 6] > 0)).sum()) > 20 and int((~keep).sum()) > 20
    assert bool((rows[zero][:, 7] == 0).all())
    hitting = keep & (rows[:, 6] > 0)
    rn, rf = voxel.get_near_far(rows[:, 0:3].to(DEV), rows[:, 3:6].to(DEV), rng)
    tol = 1e-5 * 1.0 * 5.0  # the tolerance of the sandwich above, for this cube of scale 1
    assert bool(((rows[hitting][:, 6] - rn.cpu().reshape(-1)[hitting]).abs() <= tol).all())
    assert bool(((rows[hitting][:, 7] - (rf.cpu().reshape(-1)[hitting] + 0.25)).abs() <= tol).all())  # far carries + voxel_size
    # the upper-y pixels (rows above the centre: y up in the camera) are the zero ones
    assert bool((zero.reshape(h, w)[:8].sum() > 0)) and int(zero.reshape(h, w)[12:].sum()) == 0
    # either octree missing: use_voxel = False
    r1, _, k1 = cachebuild.cache_rows(cam, img, 4, dz, wt, None, hit, None, 0.25)
    assert bool(k1.all()) and bool((r1[:, 6] == 0.5).all()) and bool((r1[:, 7] == 6.0).all())


# ---------------------------------------------------------------------------------------------------
# 4. the splat alone
# ---------------------------------------------------------------------------------------------------
def _splat_numpy(xyz, err, px, err_mean, w2c, w, h):
    dz, wt = np.zeros(h * w, np.float32), np.zeros(h * w, np.float32)
    row = np.asarray(w2c, np.float64)[2].astype(np.float32).astype(np.float64)  # the entry point takes the matrix as float32
    for i in range(len(px)):  # in order: the last key-point on a pixel stays
        c, r = int(px[i, 0]), int(px[i, 1])
        if 0 <= c < w and 0 <= r < h:
            dz[r * w + c] = np.float32(row[:3] @ xyz[i].astype(np.float64) + row[3])
            wt[r * w + c] = np.float32(2.0 * np.exp(-(np.float64(err[i]) / err_mean) ** 2))
    return dz, wt


def test_splat_alone():
    from neuralrecon_w_amd import cachebuild

    w, h = 9, 7
    rs = np.random.RandomState(4)
    n = 300  # more than one workgroup; 63 pixels: nearly every pixel is a collision
    xyz = rs.uniform(-2, 2, (n, 3)).astype(np.float32)
    err = rs.uniform(0.2, 2.0, n).astype(np.float32)
    px = np.stack([rs.randint(-3, w + 3, n), rs.randint(-3, h + 3, n)], -1).astype(np.int32)
    px[:5] = [[4, 3]] * 5  # five key-points on one pixel ...
    px[-1] = [4, 3]        # ... and the very last one too: it wins
    px[10] = [-1, 0]
    px[11] = [w, 0]
    px[12] = [0, h]
    px[13] = [-2 ** 31, 2 ** 31 - 1]
    w2c = np.array([[0.36, 0.48, -0.8, 0.1], [-0.8, 0.6, 0.0, -0.2], [0.48, 0.64, 0.6, 1.5], [0, 0, 0, 1]])
    em = float(np.mean(err.astype(np.float64)))
    want_d, want_w = _splat_numpy(xyz, err, px, em, w2c, w, h)
    a = cachebuild.sfm_depth_planes(xyz, err, px, em, w2c, w, h, DEV)
    b = cachebuild.sfm_depth_planes(xyz, err, px, em, w2c, w, h, DEV)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])  # bitwise reproducible
    d, wt = a[0].cpu().numpy(), a[1].cpu().numpy()
    assert np.array_equal(d != 0, want_d != 0) and np.array_equal(wt != 0, want_w != 0)
    np.testing.assert_allclose(d, want_d, rtol=2e-7, atol=0)   # one float32 rounding of a float64 value on either side
    np.testing.assert_allclose(wt, want_w, rtol=2e-7, atol=0)
    z_first = xyz[:5].astype(np.float64) @ w2c[2, :3] + w2c[2, 3]
    assert np.abs(z_first - d[3 * w + 4]).min() > 1e-3 and (want_d < 0).any()  # not one of the earlier five on that pixel
    # n = 0: zero planes, no launch error
    z = cachebuild.sfm_depth_planes(np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros((0, 2), np.int32), float("nan"), w2c, w, h, DEV)
    assert not bool(z[0].any()) and not bool(z[1].any()) and z[0].shape == (h * w,)
    # every key-point outside: zero planes
    z = cachebuild.sfm_depth_planes(xyz[10:14], err[10:14], px[10:14], 1.0, w2c, w, h, DEV)
    assert not bool(z[0].any()) and not bool(z[1].any())


def test_entry_point_argument_checks(g):
    from neuralrecon_w_amd import lib as L

    lib = L.get_lib()
    cam = _camera(g, 7).struct()
    s = L.stream_ptr(torch.device(DEV))
    hw = 42 * 27
    buf, rgb, plane = torch.zeros(hw * 13 + 4, device=DEV), torch.zeros(hw * 3, device=DEV), torch.zeros(hw, device=DEV)
    img = torch.zeros(hw * 3, dtype=torch.uint8, device=DEV)
    keep = torch.zeros(hw, dtype=torch.uint8, device=DEV)
    P = L.ptr
    ok = lambda **k: lib.ncw_cache_rows(C.byref(cam), P(img), None, 0, 0, k.get("dz", P(plane)), P(plane), 7, 0.1, None, None,  # noqa: E731
                                        k.get("p0", 0), k.get("n", hw), k.get("ncols", 12), k.get("rows", P(buf)), P(rgb), P(keep), s)
    assert ok() == 0
    assert ok(n=0, rows=None) == 0  # n == 0: success without a launch, whatever the pointers
    assert ok(rows=None) == -1 and ok(dz=None) == -1
    assert ok(rows=C.c_void_p(buf.data_ptr() + 4)) == -1  # rows are written as 16-byte stores
    assert ok(ncols=13) == -1 and ok(p0=1) == -1 and ok(n=-1) == -1
    w2c = (C.c_float * 12)(*([0.0] * 12))
    i32 = torch.zeros(hw, dtype=torch.int32, device=DEV)
    assert lib.ncw_sfm_depth_splat(None, None, None, 0, 1.0, w2c, 42, 27, P(i32), P(plane), P(buf), s) == 0
    assert lib.ncw_sfm_depth_splat(None, None, None, 5, 1.0, w2c, 42, 27, P(i32), P(plane), P(buf), s) == -1
    assert lib.ncw_sfm_depth_splat(None, None, None, 0, 1.0, w2c, 42, 27, None, P(plane), P(buf), s) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# 5. compaction and edges
# ---------------------------------------------------------------------------------------------------
def _keypoints(g, iid):
    t = "im%d_" % iid
    return g[t + "kp_xyz"], g[t + "kp_err"], g[t + "kp_px"], float(g[t + "err_mean"])


def test_compaction_keeps_pixel_order_and_ranges(g, octrees):
    from neuralrecon_w_amd import cachebuild

    hit, rng, vs = octrees
    iid = 3
    t = "im%d_" % iid
    rows, rgbs, keep = _rows(g, iid, True, hit, rng, vs)
    for lab in (g[t + "label"], None):
        rays, out_rgb = cachebuild.build_image(_camera(g, iid), g[t + "image"], iid, _keypoints(g, iid), g[t + "w2c"], lab, hit, rng, vs,
                                               device=DEV)
        k = keep.bool()
        if lab is not None:
            assert torch.equal(rays, rows[k])  # `rays[valid_mask]`: the kept rows, in pixel order
        else:
            assert rays.shape[1] == 12 and torch.equal(rays, torch.cat([rows[k][:, :9], rows[k][:, 10:]], 1))
        assert torch.equal(out_rgb, rgbs[k]) and 0 < rays.shape[0] < rows.shape[0]
    # a pixel range that starts inside the image and is no multiple of 64 (two workgroups, a ragged one)
    p0, n = 37, 333
    part = _rows(g, iid, True, hit, rng, vs, p0=p0, n=n)
    for a, b in zip(part, (rows, rgbs, keep)):
        assert a.shape[0] == n and torch.equal(a, b[p0:p0 + n])
    part = _rows(g, iid, False, hit, rng, vs, p0=1079, n=1)  # the last pixel alone
    assert torch.equal(part[0][:, :9], rows[1079:, :9]) and torch.equal(part[1], rgbs[1079:])
    e = _rows(g, iid, True, hit, rng, vs, p0=5, n=0)
    assert e[0].shape == (0, 13) and e[1].shape == (0, 3) and e[2].shape == (0,)


def test_one_pixel_image_and_camera_turned_away(g, octrees):
    from neuralrecon_w_amd import cachebuild, views

    hit, rng, vs = octrees
    cam0 = _camera(g, 7)
    one = views.Camera(np.array([[1.0, 0, 0.5], [0, 1.0, 0.5], [0, 0, 1]]), cam0.c2w, 1, 1, cam0.near, cam0.far)
    img = np.array([[[255, 0, 128]]], dtype=np.uint8)
    kp = (np.array([[0.1, -0.1, 0.2]], np.float32), np.array([0.7], np.float32), np.array([[0, 0]], np.int32), 0.7)
    rays, rgbs = cachebuild.build_image(one, img, 9, kp, g["im7_w2c"], np.array([[3]], np.uint8), None, None, device=DEV)
    assert rays.shape == (1, 13) and rgbs.cpu().tolist() == [[1.0, 0.0, float(np.float32(128) / np.float32(255))]]  # float(u8) / 255.f in float32
    r = rays.cpu()[0]
    assert r[8] == 9 and r[9] == 3 and r[10] > 0 and abs(float(r[11]) - 2 * np.exp(-1.0)) < 1e-6 and r[12] == 0
    rays, rgbs = cachebuild.build_image(one, img, 9, kp, g["im7_w2c"], None, hit, rng, vs, device=DEV)
    assert rays.shape[1] == 12 and rays.shape[0] in (0, 1) and rgbs.shape[0] == rays.shape[0]
    # a camera turned away from the scene: every ray misses, the result is empty
    c2w = cam0.c2w.copy()
    c2w[:, 0] *= -1
    c2w[:, 2] *= -1
    away = views.Camera(cam0.K, c2w, cam0.width, cam0.height, cam0.near, cam0.far)
    for lab, nc in ((g["im7_label"], 13), (None, 12)):
        rays, rgbs = cachebuild.build_image(away, g["im7_image"], 7, _keypoints(g, 7), g["im7_w2c"], lab, hit, rng, vs, device=DEV)
        assert rays.shape == (0, nc) and rgbs.shape == (0, 3)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# 6. build_cache end to end
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kept(g, octrees):
    """Per training image: the kept rows [m, 13] and rgbs as the row kernel gives them (the multiset the files must hold)."""
    hit, rng, vs = octrees
    out = {}
    for iid in g["train_ids"].tolist():
        rows, rgbs, keep = _rows(g, iid, True, hit, rng, vs)
        k = keep.bool()
        out[iid] = (rows[k].cpu().numpy(), rgbs[k].cpu().numpy())
    return out


def _rgb_of_rows(g, rays):
    """The image pixel every row's direction points through (rows of one image share the origin), as float rgb."""
    out = np.zeros((len(rays), 3), np.float32)
    for iid in np.unique(rays[:, 8]).astype(int).tolist():
        t = "im%d_" % iid
        sel = rays[:, 8] == iid
        dirs = g[t + "rows12"][:, 3:6]
        pix = np.argmin(((rays[sel][:, None, 3:6] - dirs[None]) ** 2).sum(-1), 1)
        out[sel] = g[t + "image"].reshape(-1, 3)[pix].astype(np.float32) / np.float32(255)
    return out


@pytest.mark.parametrize("nch", [3, 7])
def test_build_cache_end_to_end(g, kept, tmp_path, nch):
    """split_to_chunks = 3 (the kept rows of this scene, 759, divide by it: no padding) and 7 (four padding rows)."""
    from neuralrecon_w_amd import cachebuild, raycache

    root = str(tmp_path / "cache_scene")
    shutil.copytree(SCENE, root)
    stats = {}
    files = cachebuild.build_cache(root, "cache", 1, "semantic_maps", nch, "sparse", seed=3, device=DEV, stats=stats)
    sp = os.path.join(root, "cache", "splits")
    assert sorted(os.listdir(os.path.join(root, "cache"))) == ["splits"]
    assert sorted(os.listdir(sp)) == ["rays1_meta_info.json", "rgbs1_meta_info.json"] + ["split_%d" % i for i in range(nch)]
    assert sorted(os.path.relpath(f, sp) for f in files) == sorted(
        ["rays1_meta_info.json", "rgbs1_meta_info.json"] + ["split_%d/%s1.npz" % (i, a) for i in range(nch) for a in ("rays", "rgbs")])
    rays = [np.load(os.path.join(sp, "split_%d" % i, "rays1.npz"))["arr_0"] for i in range(nch)]
    rgbs = [np.load(os.path.join(sp, "split_%d" % i, "rgbs1.npz"))["arr_0"] for i in range(nch)]
    n_kept = sum(v[0].shape[0] for v in kept.values())
    n_pad = (nch - n_kept % nch) % nch
    assert (n_pad > 0) == (nch == 7)  # the second case really pads
    meta = json.load(open(os.path.join(sp, "rays1_meta_info.json")))
    assert meta == {"data_length": n_kept + n_pad, "chunk_length": (n_kept + n_pad) // nch, "n_trunks": nch}
    assert meta == json.load(open(os.path.join(sp, "rgbs1_meta_info.json")))
    assert all(r.shape == (meta["chunk_length"], 13) and r.dtype == np.float32 for r in rays)
    assert all(r.shape == (meta["chunk_length"], 3) and r.dtype == np.float32 for r in rgbs)
    assert stats["n_images"] == 3 and stats["n_rays"] == n_kept and stats["d2h_bytes"] == 4 * 16 * n_kept
    all_rays, all_rgbs = np.concatenate(rays), np.concatenate(rgbs)
    # the kept rows of the training images a, b, d in order (the test image c is not there), then the padding
    want_rays = np.concatenate([kept[i][0] for i in g["train_ids"].tolist()])
    want_rgbs = np.concatenate([kept[i][1] for i in g["train_ids"].tolist()])
    assert np.array_equal(all_rays[:n_kept], want_rays) and np.array_equal(all_rgbs[:n_kept], want_rgbs)
    assert 11 not in all_rays[:, 8]
    assert len(all_rays) == n_kept + n_pad
    both = np.concatenate([want_rays, want_rgbs], 1)
    for r in np.concatenate([all_rays, all_rgbs], 1)[n_kept:]:  # every padding row is a copy of a kept row, rgb included
        assert (both == r).all(1).any()
    # rays and rgbs were padded and split with the same indices: each row's rgb is the pixel its direction points through
    assert np.array_equal(all_rgbs, _rgb_of_rows(g, all_rays))
    # RayCache loads it and batch() returns the rows unchanged
    rc = raycache.RayCache(root, "cache", ["split_%d" % i for i in range(nch)], DEV, 1, with_semantics=True)
    b = rc.batch(None)
    assert np.array_equal(b["rays"].cpu().numpy(), np.concatenate([all_rays[:, :8], all_rays[:, 10:13]], 1))
    assert np.array_equal(b["ts"].cpu().numpy(), all_rays[:, 8].astype(np.int64))
    assert np.array_equal(b["semantics"].cpu().numpy(), all_rays[:, 9].astype(np.int64))
    assert np.array_equal(b["rgbs"].cpu().numpy(), all_rgbs)


def _nearest(lab, h, w):
    """The kernel's rule in numpy: map[floor(row hs / h), floor(col ws / w)], clamped."""
    hs, ws = lab.shape
    r = np.minimum((np.arange(h) * hs) // h, hs - 1)
    c = np.minimum((np.arange(w) * ws) // w, ws - 1)
    return lab[r][:, c]


@pytest.mark.parametrize("hs,ws", [(54, 84), (61, 97), (13, 21), (27, 42), (1, 1)])
def test_label_map_of_another_size(g, hs, ws):
    """The label column for maps that are not the image's size (every --img_downscale > 1 run): twice the size, a non-integer
    ratio with hs != ws and h != w (42 x 27 image), smaller than the image, equal, a single label."""
    from neuralrecon_w_amd import cachebuild

    t = "im7_"
    w, h = g[t + "wh"].tolist()
    lab = np.random.RandomState(hs * 100 + ws).randint(0, 200, size=(hs, ws)).astype(np.uint8)
    dz, wt = _planes(g, 7)
    rows, _, _ = cachebuild.cache_rows(_camera(g, 7), torch.from_numpy(g[t + "image"]).to(DEV), 7, dz, wt, torch.from_numpy(lab).to(DEV))
    assert np.array_equal(rows[:, 9].cpu().numpy().reshape(h, w), _nearest(lab, h, w).astype(np.float32))


def test_build_cache_downscaled(g, tmp_path):
    """img_downscale = 2 end to end without octrees (every pixel kept, so rows compare position by position): image sizes
    // 2, K rescaled, LANCZOS pixels, key-points at round_half_even(xy / 2), labels by the nearest rule from the full-size maps."""
    from PIL import Image

    from neuralrecon_w_amd import cachebuild, views

    root = str(tmp_path / "cache_scene")
    shutil.copytree(SCENE, root)
    files = cachebuild.build_cache(root, "cache2", 2, "semantic_maps", -1, "sparse", device=DEV, use_voxel=False)
    assert [os.path.relpath(f, root) for f in files] == ["cache2/rays2.npz", "cache2/rgbs2.npz"]
    rays, rgbs = np.load(files[0])["arr_0"], np.load(files[1])["arr_0"]
    scene = views.read_scene(root, "sparse")
    at = 0
    for iid in g["train_ids"].tolist():
        t = "im%d_" % iid
        w0, h0 = g[t + "wh"].tolist()
        w, h = w0 // 2, h0 // 2
        part, prgb = rays[at:at + w * h], rgbs[at:at + w * h]
        at += w * h
        K, w2c, c2w, kw, kh = views.image_pose(scene, iid, 2)
        assert (kw, kh) == (w, h) and bool((part[:, 8] == iid).all())
        want = np.asarray(Image.fromarray(g[t + "image"]).resize((w, h), Image.LANCZOS), dtype=np.uint8)
        assert np.array_equal(prgb, want.reshape(-1, 3).astype(np.float32) / np.float32(255))
        assert np.array_equal(part[:, 9].reshape(h, w), _nearest(g[t + "label"], h, w).astype(np.float32))
        cam = views.Camera(K, c2w, w, h, float(g[t + "near64"]), float(g[t + "far64"]))
        r8 = views.view_rays(cam, device=DEV).cpu().numpy()
        assert np.abs(part[:, :8] - r8).max() <= 1e-6 and np.array_equal(part[:, 6:8], r8[:, 6:8])
        px = np.rint(g[t + "xys"][g[t + "point3d_ids"] != -1] / 2).astype(np.int64)
        ok = (px[:, 0] >= 0) & (px[:, 0] < w) & (px[:, 1] >= 0) & (px[:, 1] < h)
        hitpix = np.zeros(h * w, bool)
        hitpix[px[ok, 1] * w + px[ok, 0]] = True
        assert np.array_equal(part[:, 11] != 0, hitpix) and int(hitpix.sum()) > 20
    assert at == len(rays) == len(rgbs)


@pytest.mark.parametrize("dp", [0.2, 0.6])
def test_build_cache_depth_percent(g, kept, tmp_path, dp):
    """depth_percent: the reference's padding length per image, the original rows all still there, every added row a copy of a
    row with a key-point depth; one permutation for rays and rgbs.  In this scene 22 .. 42 % of an image's kept rays carry a
    key-point depth already, so at 0.2 the reference's length is <= 0 (where its torch.rand(negative) raises and nothing is padded
    here); 0.6 pads every image."""
    from neuralrecon_w_amd import cachebuild

    root = str(tmp_path / "cache_scene")
    shutil.copytree(SCENE, root)
    files = cachebuild.build_cache(root, "cache_dp", 1, "semantic_maps", -1, "sparse", seed=1, device=DEV, depth_percent=dp)
    assert [os.path.relpath(f, root) for f in files] == ["cache_dp/rays1.npz", "cache_dp/rgbs1.npz"]
    rays, rgbs = np.load(files[0])["arr_0"], np.load(files[1])["arr_0"]
    at = 0
    for iid in g["train_ids"].tolist():
        rows0, _ = kept[iid]
        cur, valid = len(rows0), int((rows0[:, 10] > 0).sum())
        pad = max(0, int(np.ceil((dp * cur - valid) / (1 - dp))))  # phototourism.py:664
        assert valid > 0 and (pad > 0) == (dp > 0.5)
        part = rays[at:at + cur + pad]
        assert bool((part[:, 8] == iid).all())
        assert not np.array_equal(part[:cur], rows0)  # permuted
        u, cnt = np.unique(np.concatenate([rows0, part]), axis=0, return_counts=True)
        u0, cnt0 = np.unique(rows0, axis=0, return_counts=True)
        assert len(u) == len(u0) and bool((cnt0 == 1).all())  # no row that is not an original
        extra = cnt - 2  # copies beyond the original
        assert bool((extra >= 0).all()) and int(extra.sum()) == pad
        assert bool((u[extra > 0][:, 10] > 0).all())  # the added rows all have a key-point depth
        at += cur + pad
    assert at == len(rays) == len(rgbs)
    assert np.array_equal(rgbs, _rgb_of_rows(g, rays))
    again = cachebuild.build_cache(root, "cache_dp2", 1, "semantic_maps", -1, "sparse", seed=1, device=DEV, depth_percent=dp)
    assert np.array_equal(np.load(again[0])["arr_0"], rays)  # seeded: the same draws
