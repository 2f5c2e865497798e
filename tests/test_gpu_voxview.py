"""GPU: the voxel first-hit views of the reprojection filter's point-cloud source (csrc/ncw_voxview.hip through
reproj.VoxelCloud): ncw_voxel_view_seen per pixel against the float64 slab restatement (tests/_voxview_ref.py) at levels 3, 5
and 10, the validity rule, the `seen` grid, ragged sizes, NULL planes, ncw_voxel_points_seen, reproducibility, bad arguments.

Bounds: a robust pixel's voxel is the oracle's exactly; its depth is within 5e-5 scale (tests/test_gpu_voxel.py's bound on
fp32 depths of up to ~5 cube units, in the units of the box); a pixel the restatement does not call robust may come out as
either margin's answer.  At least 98 % of the pixels of every view here are robust (the restatement alone, on the CPU: level 5
outside 100 %, inside 99.9 %, camera inside a voxel 100 %, level 3 99.9 %, level 10 99.9 %)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import neuconw_oracle as O
from tests import _voxview_ref as R

from neuralrecon_w_amd import lib as L
from neuralrecon_w_amd import reproj, voxel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NCW_E_BADARG = -1
# an evaluation box far from the origin whose longest edge is x: origin (120, -205, 46), scale 20
BOX = {"eval_bbx": [[100.0, -220.0, 30.0], [140.0, -190.0, 62.0]]}
ORIGIN, SCALE = np.array([120.0, -205.0, 46.0]), 20.0


def _voxel_size(level):
    return 2 * SCALE / (1.25 * (1 << level))  # 2 scale / voxel_size = 1.25 2^level


def _lin(idx, G):
    idx = np.asarray(idx, dtype=np.int64)
    return (idx[:, 0] * G + idx[:, 1]) * G + idx[:, 2]


def _box_idx(xs, ys, zs):
    return np.stack(np.meshgrid(np.arange(*xs), np.arange(*ys), np.arange(*zs), indexing="ij"), -1).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def _grid(level):
    """(idx int64 [V,3] unique lexicographic, G, dict of named parts)."""
    G = 1 << level
    rng = np.random.RandomState(level)
    parts = {}
    if level == 5:
        parts["wall"] = _box_idx((G // 4, 3 * G // 4), (G // 2, G // 2 + 1), (G // 4, 3 * G // 4))
        parts["block"] = _box_idx((3 * G // 8, 5 * G // 8), (5 * G // 8, 3 * G // 4), (3 * G // 8, 5 * G // 8))
        parts["random"] = rng.randint(0, G, (128, 3))
    elif level == 3:
        parts["wall"] = _box_idx((2, 6), (4, 5), (2, 6))
        parts["block"] = _box_idx((3, 5), (6, 7), (3, 5))
        parts["random"] = rng.randint(0, G, (6, 3))
    else:  # level 10: a 16 x 16 patch in the middle, clutter around it, the two extreme voxels
        parts["wall"] = _box_idx((G // 2 - 8, G // 2 + 8), (G // 2, G // 2 + 1), (G // 2 - 8, G // 2 + 8))
        parts["random"] = G // 2 + rng.randint(-24, 24, (42, 3))
        parts["corners"] = np.array([[0, 0, 0], [G - 1, G - 1, G - 1]])
    idx = np.unique(np.concatenate(list(parts.values())).astype(np.int64), axis=0)
    return idx, G, parts


@functools.lru_cache(maxsize=None)
def _cloud(level):
    idx, G, _ = _grid(level)
    centres = (idx + 0.5) * (2.0 / G) - 1.0
    cloud = reproj.VoxelCloud(centres * SCALE + ORIGIN, BOX, _voxel_size(level), DEV)
    assert cloud.level == level and cloud.scale == SCALE and np.array_equal(cloud.origin, ORIGIN)
    got = voxel.voxels_from_occupancy({"occ": cloud.occ, "level": level}).cpu().numpy()
    assert np.array_equal(got, idx)  # the bit grid holds exactly the listed voxels
    return cloud


def _camera(w, h, c_norm, t_norm):
    """K (f32 values) and the camera -> world pose in the box's frame: a look-at rotation scaled by 1.7."""
    K = np.array([[0.9 * w, 0, w / 2 + 0.3], [0, 0.92 * w, h / 2 - 0.4], [0, 0, 1]], dtype=np.float32)
    pose = R.look_at(np.asarray(c_norm) * SCALE + ORIGIN, np.asarray(t_norm) * SCALE + ORIGIN, 1.7)
    return K, pose


# name -> (level, width, height, camera centre and target in cube units)
VIEWS = {
    "outside": (5, 48, 36, (0.3, -2.4, 0.5), (0.0, 0.0, 0.0)),
    "inside": (5, 48, 36, (0.1, -0.8, 0.2), (0.05, 0.0, 0.03)),
    "behind": (5, 48, 36, (-0.2, 2.4, -0.3), (0.0, 0.0, 0.0)),  # sees the block and the wall's other side
    "in_voxel": (5, 37, 23, (0.03125, 0.03125, 0.03125), (0.0, 1.0, 0.0)),  # the centre of wall voxel (16, 16, 16)
    "ragged": (5, 37, 23, (0.3, -2.4, 0.5), (0.0, 0.0, 0.0)),
    "level3": (3, 48, 36, (0.3, -2.4, 0.5), (0.0, 0.0, 0.0)),
    "level10": (10, 32, 24, (0.004, -0.03, 0.006), (0.0, 0.0, 0.0)),
}


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The float64 restatement of a view, computed once and shared."""
    level, w, h, c, t = VIEWS[name]
    idx, G, _ = _grid(level)
    K, pose = _camera(w, h, c, t)
    ref = R.view(K, pose, h, w, idx, G, ORIGIN, SCALE)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _trace(name, cloud=None, planes=True):
    level, w, h, c, t = VIEWS[name]
    cloud = _cloud(level) if cloud is None else cloud
    K, pose = _camera(w, h, c, t)
    depth = torch.full((h * w,), -7.0, device=DEV) if planes else None
    vox = torch.full((h * w,), -7, dtype=torch.int32, device=DEV) if planes else None
    cloud.trace(K, pose, h, w, depth, vox)
    return (depth.cpu().numpy(), vox.cpu().numpy()) if planes else (None, None)


def _check_against_ref(name, depth, vox):
    ref = _ref(name)
    rob = ref["robust"]
    frac = rob.mean()
    hit = (ref["voxel_lo"] >= 0)[rob].mean()
    print("%s: %.2f %% robust, %.1f %% of the robust pixels valid" % (name, 100 * frac, 100 * hit))
    assert frac >= 0.98
    assert np.array_equal(vox[rob], ref["voxel_lo"][rob])
    err = np.abs(depth[rob].astype(np.float64) - ref["depth_lo"][rob])
    print("%s: max depth error %.3g (bound %.3g)" % (name, err.max(), 5e-5 * SCALE))
    assert err.max() <= 5e-5 * SCALE
    assert (depth[vox < 0] == 0).all() and (depth[vox >= 0] > 0.02).all()
    # a pixel that is not robust comes out as one of the two margins' answers
    either = (vox == ref["voxel_lo"]) | (vox == ref["voxel_hi"])
    assert either.all(), np.flatnonzero(~either)
    return ref


def _seen(cloud):
    return cloud.seen.cpu().numpy()


def test_per_pixel_parity_level_5():
    cloud = _cloud(5)
    idx, G, parts = _grid(5)
    block = _lin(parts["block"], G)
    for name, lo, hi in (("outside", 0.2, 0.35), ("inside", 0.99, 1.0)):
        cloud.clear()
        depth, vox = _trace(name)
        ref = _check_against_ref(name, depth, vox)
        valid = (ref["voxel_lo"] >= 0)[ref["robust"]].mean()
        assert lo <= valid <= hi, valid  # about a quarter of the rays hit from outside; from inside the cube all but one or two (99.9 %)
        if name == "outside":  # the block stands behind the wall
            assert not np.isin(vox, block).any()
            assert not np.isin(ref["voxel_lo"], block).any() and not np.isin(ref["voxel_hi"], block).any()
            assert np.isin(vox, _lin(parts["wall"], G)).sum() > 100
    cloud.clear()


def test_camera_inside_an_occupied_voxel_sees_nothing():
    cloud = _cloud(5)
    idx, G, parts = _grid(5)
    cloud.clear()
    depth, vox = _trace("in_voxel")
    ref = _check_against_ref("in_voxel", depth, vox)
    rob = ref["robust"]
    assert (vox[rob] == -1).all() and (depth[rob] == 0).all()
    # ... though the rays cross other occupied voxels: the block stands in front of the camera
    level, w, h, c, t = VIEWS["in_voxel"]
    K, pose = _camera(w, h, c, t)
    d, _ = R.gen_rays(K, pose, h, w)
    on = torch.from_numpy(R.origin_norm(pose, ORIGIN, SCALE)).expand(d.shape[0], 3)
    r, _, _ = O.ray_voxel_nuggets(on, torch.from_numpy(d), torch.from_numpy(parts["block"]), G)
    assert np.unique(r.numpy()).shape[0] > 0.3 * d.shape[0]
    # seen gains no bit from an invalid ray
    assert np.array_equal(R.unpack_bits(_seen(cloud)), np.unique(vox[vox >= 0]))
    assert (vox >= 0).sum() <= (~rob).sum()
    cloud.clear()


def _split_trace(cloud, name):
    """The view in three pixel ranges [p0, p0 + n), straight through the entry point: (depth, voxel)."""
    level, w, h, c, t = VIEWS[name]
    s = cloud.view_struct(*_camera(w, h, c, t), h, w)
    depth = torch.full((h * w,), -7.0, device=DEV)
    vox = torch.full((h * w,), -7, dtype=torch.int32, device=DEV)
    cuts = [0, 7 * w + 5, 20 * w + 63, h * w]
    for p0, p1 in zip(cuts[:-1], cuts[1:]):
        L.check(L.get_lib().ncw_voxel_view_seen(C.byref(s), C.byref(cloud.grid), p0, p1 - p0, L.ptr(cloud.seen), L.ptr(depth[p0:p1]),
                                                L.ptr(vox[p0:p1]), L.stream_ptr(cloud.dev)), "ncw_voxel_view_seen")
    return depth.cpu().numpy(), vox.cpu().numpy()


def test_seen_is_the_or_of_the_voxel_plane():
    cloud = _cloud(5)
    cloud.clear()
    occ = R.unpack_bits(cloud.occ.cpu().numpy())
    depth_a, vox_a = _trace("outside")
    seen_a = R.unpack_bits(_seen(cloud))
    assert np.array_equal(seen_a, np.unique(vox_a[vox_a >= 0])) and seen_a.shape[0] > 20
    assert np.isin(seen_a, occ).all() and not (cloud.seen & ~cloud.occ).any()  # seen & ~occ == 0
    depth_b, vox_b = _trace("behind")  # a second view accumulates: the bits of the first survive
    seen_ab = R.unpack_bits(_seen(cloud))
    assert np.array_equal(seen_ab, np.union1d(seen_a, np.unique(vox_b[vox_b >= 0])))
    assert seen_ab.shape[0] > seen_a.shape[0] and np.setdiff1d(seen_a, np.unique(vox_b)).shape[0] > 0
    words_ab = _seen(cloud).copy()
    cloud.clear()
    assert not cloud.seen.any()
    # three pixel ranges give the planes and the bits of one launch
    for name, one in (("outside", (depth_a, vox_a)), ("behind", (depth_b, vox_b))):
        d3, v3 = _split_trace(cloud, name)
        assert np.array_equal(v3, one[1]) and np.array_equal(d3.view(np.int32), one[0].view(np.int32))
    assert np.array_equal(_seen(cloud), words_ab)
    cloud.clear()


def test_ragged_size_and_null_planes():
    """37 x 23 = 851 pixels = 13 workgroups of 64 + 19: the padded lanes write nothing."""
    cloud = _cloud(5)
    cloud.clear()
    level, w, h, c, t = VIEWS["ragged"]
    n = w * h
    s = cloud.view_struct(*_camera(w, h, c, t), h, w)
    depth = torch.full((n + 64,), -7.0, device=DEV)
    vox = torch.full((n + 64,), -7, dtype=torch.int32, device=DEV)
    L.check(L.get_lib().ncw_voxel_view_seen(C.byref(s), C.byref(cloud.grid), 0, n, L.ptr(cloud.seen), L.ptr(depth), L.ptr(vox),
                                            L.stream_ptr(cloud.dev)), "ncw_voxel_view_seen")
    depth, vox = depth.cpu().numpy(), vox.cpu().numpy()
    assert (depth[n:] == -7.0).all() and (vox[n:] == -7).all()
    assert (vox[:n] != -7).all() and (depth[:n] != -7.0).all()
    _check_against_ref("ragged", depth[:n], vox[:n])
    with_planes = _seen(cloud).copy()
    assert with_planes.any()
    for planes in ((True, False), (False, True), (False, False)):
        cloud.clear()
        d = torch.empty(n, device=DEV) if planes[0] else None
        v = torch.empty(n, dtype=torch.int32, device=DEV) if planes[1] else None
        cloud.trace(*_camera(w, h, c, t), h, w, d, v)
        assert np.array_equal(_seen(cloud), with_planes)
        if v is not None:
            assert np.array_equal(v.cpu().numpy(), vox[:n])
        if d is not None:
            assert np.array_equal(d.cpu().numpy(), depth[:n])
    # n == 0 launches nothing
    assert L.get_lib().ncw_voxel_view_seen(C.byref(s), C.byref(cloud.grid), n, 0, L.ptr(cloud.seen), None, None,
                                           L.stream_ptr(cloud.dev)) == 0
    cloud.clear()


@pytest.mark.parametrize("name", ["level3", "level10"])
def test_levels_3_and_10(name):
    """Level 3: G = 8, a single brick (Gb = 1).  Level 10: 2^30 voxels, linear indices up to 2^30 - 1."""
    level = VIEWS[name][0]
    idx, G, parts = _grid(level)
    if level == 10:
        assert 250 <= idx.shape[0] <= 320 and _lin(idx, G).min() == 0 and _lin(idx, G).max() == 2 ** 30 - 1
    cloud = _cloud(level)
    cloud.clear()
    depth, vox = _trace(name)
    ref = _check_against_ref(name, depth, vox)
    assert 0.1 < (ref["voxel_lo"] >= 0).mean()
    assert np.array_equal(R.unpack_bits(_seen(cloud)), np.unique(vox[vox >= 0]))
    # the extreme voxels through the point lookup: the first and the last bit of the grid
    cloud.seen[0] |= 1
    cloud.seen[-1] |= -(2 ** 31)
    c = (np.array([[0, 0, 0], [G - 1, G - 1, G - 1], [1, 0, 0]]) + 0.5) * (2.0 / G) - 1.0
    assert cloud.select(c * SCALE + ORIGIN).cpu().tolist() == [True, True, False]
    cloud.clear()
    if level == 10:
        _cloud.cache_clear()  # 2 x 128 MB of bit grids


def test_points_seen_equals_the_f32_restatement():
    cloud = _cloud(5)
    idx, G, _ = _grid(5)
    cloud.clear()
    _, vox = _trace("outside")
    _trace("inside", planes=False)
    seen = R.unpack_bits(_seen(cloud))
    rng = np.random.RandomState(3)
    src = (idx + 0.5) * (2.0 / G) - 1.0
    edge = np.array([[1.0, 0.0, 0.0], [-1.0, -1.0, -1.0], [0.0, 1.0, 0.0], [0.2, 0.3, -1.0], [1.0, 1.0, 1.0], [-1.0, 0.5, 0.99999994]])
    out = np.array([[1.5, 0.0, 0.0], [0.0, -1.0000001, 0.0], [np.nan, 0.0, 0.0], [0.0, 0.0, np.inf], [0.1, np.nan, 2.0]])
    fill = rng.uniform(-1.1, 1.1, (4096 - len(src) - len(edge) - len(out), 3))
    on_faces = np.round(rng.uniform(-1, 1, (64, 3)) * (G / 2)) / (G / 2)  # exactly on voxel faces
    fill[:64] = on_faces
    pn = np.concatenate([src, edge, out, fill])
    assert pn.shape[0] == 4096
    pts = pn * SCALE + ORIGIN
    pn32 = R.normalise32(pts, ORIGIN, SCALE)
    want = R.kept(R.point_voxels(pn32, G), seen)
    got = cloud.select(pts).cpu().numpy()
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    # every source point whose voxel is in seen is flagged, and no other source point
    assert np.array_equal(got[: len(src)], np.isin(_lin(idx, G), seen))
    assert 20 < got[: len(src)].sum() < len(src)
    assert not got[len(src) + len(edge): len(src) + len(edge) + len(out)].any()
    # the entry point itself, on the f32 points
    p32 = torch.from_numpy(pn32).to(DEV)
    flags = torch.full((4096 + 64,), 9, dtype=torch.uint8, device=DEV)
    L.check(L.get_lib().ncw_voxel_points_seen(L.ptr(p32), 4096, 5, L.ptr(cloud.seen), L.ptr(flags), L.stream_ptr(cloud.dev)), "points")
    assert np.array_equal(flags[:4096].cpu().numpy(), want.astype(np.uint8)) and (flags[4096:] == 9).all()
    cloud.clear()


def test_two_runs_are_bitwise_equal():
    cloud = _cloud(5)
    runs = []
    for _ in range(2):
        cloud.clear()
        a = _trace("outside")
        b = _trace("inside")
        runs.append((a, b, _seen(cloud).copy()))
    for x, y in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    assert np.array_equal(runs[0][2], runs[1][2])
    cloud.clear()


def test_bad_arguments_are_refused_without_a_launch():
    cloud = _cloud(5)
    cloud.clear()
    lib = L.get_lib()
    level, w, h, c, t = VIEWS["outside"]
    n = w * h
    s = cloud.view_struct(*_camera(w, h, c, t), h, w)
    depth = torch.full((n,), -7.0, device=DEV)
    st = L.stream_ptr(cloud.dev)

    def grid(level=5, occ=True, brick=True):
        g = L.NcwCacheOctree()
        g.scale, g.level = SCALE, level
        g.occ = cloud.occ.data_ptr() if occ else None
        g.brick = cloud.brick.data_ptr() if brick else None
        return g

    call = lambda g, p0, m, seen=cloud.seen: lib.ncw_voxel_view_seen(C.byref(s), C.byref(g), p0, m, L.ptr(seen), L.ptr(depth), None, st)  # noqa: E731
    assert call(grid(level=2), 0, n) == NCW_E_BADARG
    assert call(grid(level=11), 0, n) == NCW_E_BADARG
    assert call(grid(), 1, n) == NCW_E_BADARG  # one pixel past the view
    assert call(grid(), n, 1) == NCW_E_BADARG
    assert call(grid(), -1, 4) == NCW_E_BADARG
    assert call(grid(occ=False), 0, n) == NCW_E_BADARG
    assert call(grid(brick=False), 0, n) == NCW_E_BADARG
    assert call(grid(), 0, n, seen=None) == NCW_E_BADARG
    assert lib.ncw_voxel_view_seen(None, C.byref(grid()), 0, n, L.ptr(cloud.seen), None, None, st) == NCW_E_BADARG
    flags = torch.zeros(4, dtype=torch.uint8, device=DEV)
    p = torch.zeros(4, 3, device=DEV)
    for lv in (2, 11):
        assert lib.ncw_voxel_points_seen(L.ptr(p), 4, lv, L.ptr(cloud.seen), L.ptr(flags), st) == NCW_E_BADARG
    assert lib.ncw_voxel_points_seen(L.ptr(p), 4, 5, None, L.ptr(flags), st) == NCW_E_BADARG
    assert lib.ncw_voxel_points_seen(L.ptr(p), 0, 5, L.ptr(cloud.seen), L.ptr(flags), st) == 0
    torch.cuda.synchronize()
    assert (depth == -7.0).all() and not cloud.seen.any()  # nothing ran
    assert call(grid(), 0, n) == 0  # and the good call does
    assert cloud.seen.any()
    cloud.clear()
