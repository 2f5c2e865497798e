"""The inputs and calls of the voxel-walk fixture tests/golden/dda_parent.npz: every kernel built on csrc/ncw_dda.h's dda_walk
(ncw_ray_voxel_near_far, both passes of ncw_ray_voxel_trace, ncw_voxel_view_seen, ncw_cache_rows with use_voxel) over seeded
inputs, called through the C ABI so that nothing of the Python layer takes part.  tests/golden/make_golden_dda_parent.py runs
`compute` on the build whose outputs are the reference, tests/test_gpu_dda_parent.py on the build under test.

Inputs are made with numpy's RandomState (a frozen stream) and float64 +, -, *, /, sqrt only, then rounded to f32: the same bytes
on every machine; `inputs_digest` is stored beside the outputs and checked before anything is compared.

The cloud of a level is two parallel tilted walls of random points, 48 voxels of that level wide (at most 1.2), the second three
voxels behind the first: dense enough that a ray aimed at it hits at level 10, thin enough that it has few crossings.
No direction component is exactly 0 (asserted): the walk's zero-direction axis is a separate, open matter.
"""
import ctypes as C
import hashlib

import numpy as np
import torch

from neuralrecon_w_amd import lib as L

LEVELS = (3, 5, 10)
N_POINTS = 4096
N_RAYS = 257
W, H = 67, 45          # 3015 pixels: 47 waves of 64 and 7 lanes, 11 workgroups of 256 and 199 rows
FOCAL = 60.0
CACHE_LEVELS = (5, 7)  # hit octree, range octree
SFM_ORIGIN = (0.3, -0.2, 0.1)
SFM_SCALE = 1.7

_CENTRE = np.array([0.11, -0.07, 0.05])


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


_N = _unit(np.array([0.35, 0.25, 0.9]))
_E1 = _unit(np.cross(_N, np.array([0.0, 1.0, 0.0])))
_E2 = np.cross(_N, _E1)


def wall_side(level):
    return min(1.2, 48 * 2.0 / (1 << level))


def cloud(level):
    """float64 [4096, 3] in the cube's normalised coordinates: 3072 points on the front wall, 1024 three voxels behind it."""
    rs = np.random.RandomState(1000 + level)
    ab = rs.uniform(-0.5, 0.5, (N_POINTS, 2)) * wall_side(level)
    back = (np.arange(N_POINTS) >= 3072).astype(np.float64)[:, None]
    return _CENTRE + ab[:, :1] * _E1 + ab[:, 1:] * _E2 + back * (3.0 * 2.0 / (1 << level)) * _N


def rays(level):
    """(o, d) f32 [257, 3], normalised coordinates.  By index modulo 20: 0-6 start outside the cube and aim at a cloud point
    (un-normalised direction), 7-10 start inside the cube and aim at one, 11-13 start AT a cloud point (inside an occupied voxel),
    14-16 start outside and fly away from the cube, 17-19 start outside and cross the cube towards a random point."""
    pts = cloud(level)
    rs = np.random.RandomState(2000 + level)
    kind = np.arange(N_RAYS) % 20
    target = pts[rs.randint(0, N_POINTS, N_RAYS)]
    rnd = rs.uniform(-1, 1, (N_RAYS, 3))
    o_out = 2.5 * _unit(rs.uniform(-1, 1, (N_RAYS, 3)) + 1e-3)
    o_in = rs.uniform(-0.9, 0.9, (N_RAYS, 3))
    through = rs.uniform(-0.8, 0.8, (N_RAYS, 3))
    o = np.where((kind < 7)[:, None], o_out, o_in)
    d = np.where((kind < 7)[:, None], target - o_out, _unit(target - o_in))
    at = (kind >= 11) & (kind < 14)
    o, d = np.where(at[:, None], target, o), np.where(at[:, None], _unit(rnd), d)
    away = (kind >= 14) & (kind < 17)
    o, d = np.where(away[:, None], o_out, o), np.where(away[:, None], _unit(o_out + 0.3 * rnd), d)
    thr = kind >= 17
    o, d = np.where(thr[:, None], o_out, o), np.where(thr[:, None], through - o_out, d)
    o, d = o.astype(np.float32), d.astype(np.float32)
    assert (d != 0).all() and (d + np.float32(1e-7) != 0).all(), "a direction component is exactly 0"
    return o, d


def view_camera(level):
    """The pinhole camera of the 67 x 45 view: on the walls' normal, at the distance where the front wall is 48 pixels wide, the
    principal point off-centre so that the columns right of the wall see nothing.  (K, rotation [3,3] camera -> cube, centre)."""
    K = np.array([[FOCAL, 0, 18.3], [0, FOCAL, 22.4], [0, 0, 1]])
    return K, np.stack([_E1, _E2, _N], -1), _CENTRE - (FOCAL * wall_side(level) / 48) * _N


def cache_image():
    """(image uint8 [45, 67, 3], depth_z f32 [3015], weight f32 [3015]) of the cache-row case."""
    rs = np.random.RandomState(3000)
    image = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    depth_z = np.where(rs.uniform(0, 1, W * H) < 0.05, rs.uniform(0.5, 3.0, W * H), 0.0).astype(np.float32)
    weight = (depth_z != 0) * rs.uniform(0.1, 2.0, W * H).astype(np.float32)
    return image, depth_z, weight.astype(np.float32)


def inputs_digest():
    h = hashlib.sha256()
    for level in LEVELS + CACHE_LEVELS[1:]:
        h.update(cloud(level).astype(np.float32).tobytes())
    for level in LEVELS:
        o, d = rays(level)
        h.update(o.tobytes() + d.tobytes())
        K, R, c = view_camera(level)
        h.update(np.concatenate([K.reshape(-1), R.reshape(-1), c]).astype(np.float32).tobytes())
    for a in cache_image():
        h.update(a.tobytes())
    return h.hexdigest()


def _grid(points_norm, level, dev):
    """(occ, brick) int32 bit masks of ncw_voxel_build over normalised f64 points."""
    G = 1 << level
    pn = torch.from_numpy(points_norm.astype(np.float32)).to(dev).contiguous()
    occ = torch.zeros(G * G * G // 32, dtype=torch.int32, device=dev)
    brick = torch.zeros((max(G // 8, 1) ** 3 + 31) // 32, dtype=torch.int32, device=dev)
    L.check(L.get_lib().ncw_voxel_build(L.ptr(pn), int(pn.shape[0]), level, L.ptr(occ), L.ptr(brick), L.stream_ptr(dev)), "build")
    return occ, brick


def _octree(origin, scale, level, occ, brick):
    return L.NcwCacheOctree((C.c_float * 3)(*origin), float(scale), int(level), 0, occ.data_ptr(), brick.data_ptr())


def _level(level, dev, out):
    lib, st = L.get_lib(), L.stream_ptr(dev)
    occ, brick = _grid(cloud(level), level, dev)
    o_np, d_np = rays(level)
    o, d = torch.from_numpy(o_np).to(dev), torch.from_numpy(d_np).to(dev)
    R = N_RAYS
    # ncw_ray_voxel_near_far: the same rays carried to an SfM frame
    so = np.array(SFM_ORIGIN, dtype=np.float32)
    o_sfm = torch.from_numpy(o_np * np.float32(SFM_SCALE) + so).to(dev).contiguous()
    near = torch.empty(R, dtype=torch.float32, device=dev)
    far = torch.empty(R, dtype=torch.float32, device=dev)
    L.check(lib.ncw_ray_voxel_near_far(L.ptr(o_sfm), L.ptr(d), R, (C.c_float * 3)(*SFM_ORIGIN), SFM_SCALE, level, L.ptr(occ),
                                       L.ptr(brick), L.ptr(near), L.ptr(far), st), "ncw_ray_voxel_near_far")
    # ncw_ray_voxel_trace: the count pass, then the write pass
    counts = torch.zeros(R, dtype=torch.int32, device=dev)
    L.check(lib.ncw_ray_voxel_trace(L.ptr(o), L.ptr(d), R, level, L.ptr(occ), L.ptr(brick), None, L.ptr(counts), None, None, None,
                                    st), "ncw_ray_voxel_trace (count)")
    incl = torch.cumsum(counts, 0)
    n = int(incl[-1])
    offsets = (incl - counts).to(torch.int32)
    nug_ray = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    nug_voxel = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    nug_depth = torch.zeros(max(n, 1), 2, dtype=torch.float32, device=dev)
    if n:
        L.check(lib.ncw_ray_voxel_trace(L.ptr(o), L.ptr(d), R, level, L.ptr(occ), L.ptr(brick), L.ptr(offsets), None,
                                        L.ptr(nug_ray), L.ptr(nug_voxel), L.ptr(nug_depth), st), "ncw_ray_voxel_trace (write)")
    # ncw_voxel_view_seen: one 67 x 45 view
    K, rot, centre = view_camera(level)
    s = L.NcwVoxelView()
    s.fx, s.fy, s.cx, s.cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    for i, x in enumerate(rot.reshape(-1)):
        s.pose[i] = float(x)
    for i, x in enumerate(centre):
        s.o_norm[i] = float(x)
    s.width, s.height = W, H
    grid = _octree((0.0, 0.0, 0.0), 1.0, level, occ, brick)
    seen = torch.zeros_like(occ)
    depth = torch.empty(W * H, dtype=torch.float32, device=dev)
    voxel = torch.empty(W * H, dtype=torch.int32, device=dev)
    L.check(lib.ncw_voxel_view_seen(C.byref(s), C.byref(grid), 0, W * H, L.ptr(seen), L.ptr(depth), L.ptr(voxel), st),
            "ncw_voxel_view_seen")
    words = seen.nonzero().reshape(-1)
    p = "L%d_" % level
    out.update({p + "near": near, p + "far": far, p + "counts": counts, p + "nug_ray": nug_ray[:n], p + "nug_voxel": nug_voxel[:n],
                p + "nug_depth": nug_depth[:n], p + "view_voxel": voxel, p + "view_depth": depth,
                p + "seen_index": words.to(torch.int32), p + "seen_word": seen[words]})


def _cache(dev, out):
    """ncw_cache_rows with use_voxel over the walls of level 7 in an SfM frame: hit octree at level 5, range octree at 7."""
    lib, st = L.get_lib(), L.stream_ptr(dev)
    pts = cloud(CACHE_LEVELS[1])
    grids = [_grid(pts, lv, dev) for lv in CACHE_LEVELS]
    trees = [_octree(SFM_ORIGIN, SFM_SCALE, lv, *g) for lv, g in zip(CACHE_LEVELS, grids)]
    K, rot, centre = view_camera(CACHE_LEVELS[1])
    so = np.array(SFM_ORIGIN)
    c2w = np.concatenate([np.stack([_E1, -_E2, -_N], -1), (centre * SFM_SCALE + so)[:, None]], -1)  # "right up back" axes
    cam = L.NcwViewCamera(float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]),
                          (C.c_float * 12)(*[float(v) for v in c2w.reshape(-1)]), W, H, 0.1, 5.0)
    image, depth_z, weight = (torch.from_numpy(a).to(dev).contiguous() for a in cache_image())
    rows = torch.empty(W * H, 12, dtype=torch.float32, device=dev)
    rgbs = torch.empty(W * H, 3, dtype=torch.float32, device=dev)
    keep = torch.empty(W * H, dtype=torch.uint8, device=dev)
    L.check(lib.ncw_cache_rows(C.byref(cam), L.ptr(image), None, 0, 0, L.ptr(depth_z), L.ptr(weight), 7, 0.03, C.byref(trees[0]),
                               C.byref(trees[1]), 0, W * H, 12, L.ptr(rows), L.ptr(rgbs), L.ptr(keep), st), "ncw_cache_rows")
    out.update({"cache_rows": rows, "cache_rgbs": rgbs, "cache_keep": keep})


def packed(out):
    """The outputs as the fixture stores them.  Everything the walk decides is kept word for word; of the cache rows that is the
    near / far columns and `keep`.  Their other columns and the rgb rows (ray origin and direction, image id, key-point depth and
    weight, pixel / 255: the same kernel, but nothing the walk touches, and 150 kB of it) are kept as the SHA-256 of their
    bytes, which is as exact a comparison and keeps the file small."""
    out = dict(out)
    rows, rgbs = out.pop("cache_rows"), out.pop("cache_rgbs")
    rest = torch.cat([rows[:, :6], rows[:, 8:], rgbs], 1).contiguous().numpy().tobytes()
    out["cache_near_far"] = rows[:, 6:8].contiguous()
    out["cache_rest_sha256"] = torch.from_numpy(np.frombuffer(hashlib.sha256(rest).hexdigest().encode("ascii"), dtype=np.uint8).copy())
    return out


def compute(device="cuda:0"):
    """{name: tensor on the host} of every output of the calls above."""
    dev = torch.device(device)
    out = {}
    for level in LEVELS:
        _level(level, dev, out)
    _cache(dev, out)
    torch.cuda.synchronize(dev)
    return {k: v.cpu() for k, v in out.items()}
