"""GPU: the reprojection filter with a point-cloud source (reproj.reproj_filter -> reproj.VoxelCloud, csrc/ncw_voxview.hip;
utils/reproj_filter.py:110-115 over utils/kaolin_renderer.py), through the command line and in process, against the float64
restatement of tests/_voxview_ref.py.

The rule under test: a target vertex is kept iff the voxel of the SOURCE's grid that contains it was the first hit of some
training-view pixel.  Pixels the restatement does not call robust may go either way, so the kept set is sandwiched: it holds
every vertex whose voxel a robust pixel sees and only vertices whose voxel some pixel sees under either grazing margin."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import _voxview_ref as R
from tests._util import GOLDEN, ROOT

from neuralrecon_w_amd import evalmesh, reproj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SFM2GT = np.eye(4)
SFM2GT[:3, :3] = 1.5 * np.array([[math.cos(0.4), -math.sin(0.4), 0], [math.sin(0.4), math.cos(0.4), 0], [0, 0, 1]])
SFM2GT[:3, 3] = [3.0, -1.0, 0.5]
# GT frame: the scene spans x [-1.3, 7.3], y [-5.3, 3.3], z [0.5, 2.9]; longest edge 10 -> origin (3, -1, 2), scale 5
EVAL_BBX = [[-2.0, -6.0, 0.0], [8.0, 4.0, 4.0]]
VOXEL_SIZE = 0.12  # 10 / 0.12 = 83.3 -> level 6 (GT voxels of 0.156 = 0.104 in the SfM frame)
LEVEL, G = 6, 64
ORIGIN, SCALE = np.array([3.0, -1.0, 2.0]), 5.0
# (width, height, (fx, fy, cx, cy), centre) of three small cameras that look down at the scene from y < 0
CAMS = [(64, 48, [60.0, 61.0, 32.3, 23.7], (0.6, -3.0, 3.6)), (48, 48, [45.0, 44.0, 23.2, 25.1], (-0.8, -2.6, 3.9)),
        (64, 48, [60.0, 61.0, 32.3, 23.7], (0.0, -2.2, 4.2))]


def _lattice(o, u, v, nu, nv):
    a, b = np.meshgrid(np.linspace(0, 1, nu), np.linspace(0, 1, nv), indexing="ij")
    return np.asarray(o, dtype=np.float64) + a.reshape(-1, 1) * np.asarray(u, dtype=np.float64) + b.reshape(-1, 1) * np.asarray(v, dtype=np.float64)


def _hidden_cloud():
    """SfM frame, points every 0.05 (half a voxel): a ground z = 0 over [-2, 2]^2, a box on it, a wall y in [1, 1.1] (three
    layers: a voxel thick, so no ray slips through the staircase its voxels make in the rotated GT grid), a ball of points
    behind the wall.  Returns (points float64 [N,3], labels: 0 ground, 1 box, 2 wall, 3 ball)."""
    parts = [(_lattice([-2, -2, 0], [4, 0, 0], [0, 4, 0], 81, 81), 0)]
    lo, b, h = np.array([-0.4, -0.9, 0.0]), 0.8, 0.5
    box = [_lattice(lo + [0, 0, h], [b, 0, 0], [0, b, 0], 17, 17), _lattice(lo, [b, 0, 0], [0, 0, h], 17, 11),
           _lattice(lo + [0, b, 0], [b, 0, 0], [0, 0, h], 17, 11), _lattice(lo, [0, b, 0], [0, 0, h], 17, 11),
           _lattice(lo + [b, 0, 0], [0, b, 0], [0, 0, h], 17, 11)]
    parts.append((np.concatenate(box), 1))
    parts.append((np.concatenate([_lattice([-1.4, y, 0], [2.8, 0, 0], [0, 0, 1.6], 57, 33) for y in (1.0, 1.05, 1.1)]), 2))
    rng = np.random.RandomState(2)
    s = rng.randn(600, 3)
    parts.append((np.array([0.0, 1.7, 0.6]) + 0.3 * s / np.linalg.norm(s, axis=1, keepdims=True), 3))
    pts, lab = np.concatenate([p for p, _ in parts]), np.concatenate([np.full(len(p), k) for p, k in parts])
    _, first = np.unique(pts.astype(np.float32), axis=0, return_index=True)  # the box's faces share their edges
    first.sort()
    return pts[first], lab[first]


def _look_at(C, T):
    z = np.asarray(T, dtype=np.float64) - C
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 0.0, -1.0]), z)
    x /= np.linalg.norm(x)
    Rm = np.stack([x, np.cross(z, x), z])
    return Rm, -Rm @ np.asarray(C, dtype=np.float64)


def _qvec(Rm):
    w = math.sqrt(max(0.0, 1.0 + np.trace(Rm))) / 2
    return np.array([w, (Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w)])


def _write_workspace(root, eval_bbx=EVAL_BBX):
    """A COLMAP workspace (dense/sparse/{cameras,images}.bin, the tsv split, config.yaml) of CAMS; the loaded views."""
    sp = os.path.join(root, "dense", "sparse")
    os.makedirs(sp, exist_ok=True)
    with open(os.path.join(sp, "cameras.bin"), "wb") as fc, open(os.path.join(sp, "images.bin"), "wb") as fi:
        fc.write(struct.pack("<Q", len(CAMS)))
        fi.write(struct.pack("<Q", len(CAMS)))
        for k, (w, h, p, Cc) in enumerate(CAMS):
            fc.write(struct.pack("<iiQQ4d", k + 1, 1, w, h, *p))
            Rm, t = _look_at(np.array(Cc), (0.0, 0.2, 0.0))
            fi.write(struct.pack("<i7di", k + 1, *_qvec(Rm), *t, k + 1) + ("v%d.jpg" % k).encode() + b"\0" + struct.pack("<Q", 0))
    with open(os.path.join(root, "scene.tsv"), "w") as fh:
        fh.write("filename\tid\tsplit\n" + "".join("v%d.jpg\t%d\ttrain\n" % (k, k) for k in range(len(CAMS))))
    cfg = {"sfm2gt": SFM2GT.tolist()}
    if eval_bbx is not None:
        cfg["eval_bbx"] = eval_bbx
    with open(os.path.join(root, "config.yaml"), "w") as fh:
        yaml.safe_dump(cfg, fh)
    return reproj.load_views(root, SFM2GT)


def _rgb(n):
    return (np.arange(n)[:, None] * np.array([7, 13, 29]) % 256).astype(np.uint8)


def _row_index(xyz, rows):
    """Indices of the vertices (xyz, all different) whose coordinates the rows hold, bit for bit."""
    at = {p.tobytes(): i for i, p in enumerate(np.ascontiguousarray(xyz, dtype=np.float64))}
    assert len(at) == len(xyz)
    return np.array([at[p.tobytes()] for p in np.ascontiguousarray(rows[:, :3], dtype=np.float64)], dtype=np.int64)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """The workspace, the cloud file and the restatement's two sets of seen voxels (computed once, shared)."""
    tmp = tmp_path_factory.mktemp("cloud_scene")
    pts, lab = _hidden_cloud()
    root = str(tmp / "scene")
    views = _write_workspace(root)
    cloud_file = str(tmp / "cloud.ply")
    pts = pts.astype(np.float32).astype(np.float64)  # as a float PLY stores them
    rec = np.empty(len(pts), dtype=[("p", "<f4", 3), ("c", "u1", 3)])
    rec["p"], rec["c"] = pts, _rgb(len(pts))
    with open(cloud_file, "wb") as fh:  # float x / y / z + uchar colours, no face element
        fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(pts)).encode("ascii"))
        fh.write(rec.tobytes())
    xyz = evalmesh.apply_transform(pts, SFM2GT)
    assert (xyz > np.array(EVAL_BBX[0])).all() and (xyz < np.array(EVAL_BBX[1])).all()
    vox = R.point_voxels(R.normalise32(xyz, ORIGIN, SCALE), G)
    assert (vox >= 0).all()
    occ = np.unique(vox)
    idx = np.stack([occ // (G * G), (occ // G) % G, occ % G], -1)
    must, may = [], []
    for v in views:
        w, h = v["wh"]
        ref = R.view(v["K"], v["pose"], h, w, idx, G, ORIGIN, SCALE)
        assert ref["robust"].mean() > 0.95
        must.append(ref["voxel_lo"][ref["robust"]])
        may += [ref["voxel_lo"], ref["voxel_hi"]]
    return {"root": root, "views": views, "file": cloud_file, "xyz": xyz, "lab": lab, "rgb": _rgb(len(pts)), "vox": vox,
            "must": np.unique(np.concatenate(must)), "may": np.unique(np.concatenate(may))}


def test_command_line_end_to_end_on_a_cloud(scene, tmp_path):
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "reproj_filter.py"), "--src_file", scene["file"], "--target_file",
                        scene["file"], "--data_path", scene["root"], "--output_path", out, "--voxel_size", str(VOXEL_SIZE),
                        "--visualize", "--n_cpus", "4", "--n_gpus", "4"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    gx, gf, gc = reproj.read_ply_mesh(os.path.join(out, "reprojected.ply"))
    assert gf.shape[0] == 0
    xyz, lab = scene["xyz"], scene["lab"]
    j = _row_index(xyz, gx)
    got = np.zeros(len(xyz), bool)
    got[j] = True
    assert np.array_equal(gc, scene["rgb"][j])  # colours follow their vertices
    rows = np.c_[gx, gc.astype(np.float64)]
    assert np.array_equal(rows, np.unique(rows, axis=0))  # sorted and unique
    must, may = R.kept(scene["vox"], scene["must"]), R.kept(scene["vox"], scene["may"])
    print("kept %d of %d (must %d, may %d)" % (got.sum(), len(xyz), must.sum(), may.sum()))
    assert (must <= got).all(), np.flatnonzero(must & ~got)
    assert (got <= may).all(), np.flatnonzero(got & ~may)
    assert not got[lab == 3].any() and not may[lab == 3].any()  # the ball behind the wall
    assert got[lab == 0].sum() > 100 and got[lab == 2].sum() > 100 and 0 < got.sum() < len(xyz)
    for k, (w, h, _, _) in enumerate(CAMS):
        d = np.load(os.path.join(out, "render", "depth", "v%d.npy" % k))
        assert d.shape == (h, w) and d.dtype == np.float32 and (d > 0).mean() > 0.5 and (d[d > 0] > 0.02).all()
        px, _, _ = reproj.read_ply_mesh(os.path.join(out, "render", "reprojects", "v%d.ply" % k))
        assert px.shape[0] == int((d > 0).sum())
        # a back-projected pixel lies at its first-hit voxel: inside the cube, within a voxel diagonal of an occupied one
        pv = R.point_voxels(R.normalise32(px, ORIGIN, SCALE), G)
        assert (pv >= 0).all()


def test_target_different_from_the_source(scene, tmp_path):
    """The source plus jittered copies plus points outside the box: the kept set follows the voxel rule."""
    rng = np.random.RandomState(5)
    src_sfm, _, _ = reproj.read_ply_mesh(scene["file"])
    pick = rng.choice(len(src_sfm), 3000, replace=False)
    jit = src_sfm[pick] + rng.uniform(-0.15, 0.15, (3000, 3))  # up to a voxel and a half away (SfM units)
    gt_out = np.array([[3.0, -1.0, 5.0], [3.0, -1.0, 6.9], [3.0, -1.0, 7.5], [9.0, -1.0, 2.0], [-2.5, -1.0, 2.0], [3.0, 30.0, 2.0]])
    S_inv = np.linalg.inv(SFM2GT)
    tgt_sfm = np.concatenate([src_sfm, jit, evalmesh.apply_transform(gt_out, S_inv)]).astype(np.float32).astype(np.float64)
    tfile = str(tmp_path / "target.ply")
    reproj.write_ply_points(tfile, tgt_sfm, _rgb(len(tgt_sfm)))  # double coordinates
    out = str(tmp_path / "out")
    gx, gc = reproj.reproj_filter(scene["file"], tfile, scene["root"], out, voxel_size=VOXEL_SIZE, verbose=False)
    fx, _, fc = reproj.read_ply_mesh(os.path.join(out, "reprojected.ply"))
    assert np.array_equal(fx, gx) and np.array_equal(fc, gc)
    assert not os.path.exists(os.path.join(out, "render"))
    xyz = evalmesh.apply_transform(tgt_sfm, SFM2GT)
    vox = R.point_voxels(R.normalise32(xyz, ORIGIN, SCALE), G)
    must, may = R.kept(vox, scene["must"]), R.kept(vox, scene["may"])
    rows = np.c_[xyz, _rgb(len(xyz)).astype(np.float64)]
    got_rows = np.c_[gx, gc.astype(np.float64)]
    assert np.array_equal(got_rows, np.unique(got_rows, axis=0))
    lo = np.unique(rows[must], axis=0)
    hi = np.unique(rows[may], axis=0)

    def contains(big, small):
        both = np.concatenate([big, small])
        return np.unique(both, axis=0).shape[0] == big.shape[0]

    assert contains(got_rows, lo) and contains(hi, got_rows)
    n_src = len(src_sfm)
    print("kept %d rows of %d vertices; jittered copies kept %d .. %d" % (len(gx), len(xyz), must[n_src:n_src + 3000].sum(), may[n_src:n_src + 3000].sum()))
    assert 100 < must[n_src:n_src + 3000].sum() < 3000  # some jittered copies stay in a seen voxel, some leave
    assert not may[-len(gt_out):].any()  # outside the box (empty voxels) and outside the cube (no voxel)
    # with --gt the files are taken as GT coordinates already: the same cloud carried to GT gives the same rows
    sfile, t2 = str(tmp_path / "src_gt.ply"), str(tmp_path / "tgt_gt.ply")
    reproj.write_ply_points(sfile, scene["xyz"])
    reproj.write_ply_points(t2, xyz, _rgb(len(xyz)))
    g2x, g2c = reproj.reproj_filter(sfile, t2, scene["root"], str(tmp_path / "out_gt"), gt=True, voxel_size=VOXEL_SIZE, verbose=False)
    assert np.array_equal(g2x, gx) and np.array_equal(g2c, gc)


def test_refusals(scene, tmp_path):
    # level 11: 10 / voxel_size >= 2048
    with pytest.raises(ValueError, match=r"level 11.*smallest voxel_size that fits is above 0\.0048828125"):
        reproj.reproj_filter(scene["file"], scene["file"], scene["root"], str(tmp_path / "o1"), voxel_size=0.004, verbose=False)
    with pytest.raises(ValueError, match="level 2"):
        reproj.reproj_filter(scene["file"], scene["file"], scene["root"], str(tmp_path / "o2"), voxel_size=2.0, verbose=False)
    root = str(tmp_path / "no_box")
    _write_workspace(root, eval_bbx=None)
    with pytest.raises(ValueError, match="eval_bbx"):
        reproj.reproj_filter(scene["file"], scene["file"], root, str(tmp_path / "o3"), voxel_size=VOXEL_SIZE, verbose=False)
    for o in ("o1", "o2", "o3"):
        assert not os.path.exists(str(tmp_path / o / "reprojected.ply"))


def test_render_cloud_depth_matches_the_restatement(scene):
    v = scene["views"][1]
    w, h = v["wh"]
    cfg = {"eval_bbx": EVAL_BBX}
    depth, vox = reproj.render_cloud_depth(scene["xyz"], cfg, VOXEL_SIZE, v["K"], v["pose"], h, w, device=DEV)
    assert depth.shape == vox.shape == (h, w) and depth.dtype == torch.float32 and vox.dtype == torch.int32
    occ = np.unique(scene["vox"])
    idx = np.stack([occ // (G * G), (occ // G) % G, occ % G], -1)
    ref = R.view(v["K"], v["pose"], h, w, idx, G, ORIGIN, SCALE)
    rob = ref["robust"]
    depth, vox = depth.reshape(-1).cpu().numpy(), vox.reshape(-1).cpu().numpy()
    assert np.array_equal(vox[rob], ref["voxel_lo"][rob])
    assert np.abs(depth[rob] - ref["depth_lo"][rob]).max() <= 5e-5 * SCALE
    # depth is camera-space z in SfM units: back-projected with the SfM-scaled pose it lands on the first-hit voxel
    pts, pix = reproj.backproject(torch.from_numpy((depth - np.where(depth > 0, 0.02, 0)).astype(np.float32)).to(DEV).view(h, w),
                                  reproj.backproject_matrix(v["K"], v["pose"], ORIGIN))
    pix = pix.cpu().numpy()
    c = ((pts.double().cpu().numpy() / SCALE + 1.0) * (G / 2))  # grid coordinates of the entry points
    lin = vox[pix]
    centre = np.stack([lin // (G * G), (lin // G) % G, lin % G], -1) + 0.5
    assert np.abs(c - centre).max() < 0.5 + 1e-2  # on the voxel's surface


def test_mesh_source_takes_the_rasterizer_path_unchanged(tmp_path):
    """A source with faces: reproj_filter writes, row for row, what the commit before the point-cloud path wrote for the
    golden scene's mesh (tests/golden/reproj_scene_parent_rows.npz: its reprojected.ply, recorded on an MI355X; the
    rasterizer's 64-bit atomicMin and the exact 1-NN make the rows bitwise reproducible)."""
    want = np.load(os.path.join(GOLDEN, "reproj_scene_parent_rows.npz"))
    root = os.path.join(GOLDEN, "reproj_scene")
    mesh_file = os.path.join(root, "mesh.ply")
    _, faces, _ = reproj.read_ply_mesh(mesh_file)
    assert faces.shape[0] > 0
    gx, gc = reproj.reproj_filter(mesh_file, mesh_file, root, str(tmp_path / "out"), voxel_size=float(want["voxel_size"]), verbose=False)
    assert want["xyz"].shape[0] > 50
    assert np.array_equal(gx, want["xyz"]) and np.array_equal(gc, want["rgb"])
    fx, _, fc = reproj.read_ply_mesh(str(tmp_path / "out" / "reprojected.ply"))
    assert np.array_equal(fx, want["xyz"]) and np.array_equal(fc, want["rgb"])


def test_planes_are_checked_and_any_cuda_device_name_works(scene):
    v = scene["views"][0]
    w, h = v["wh"]
    cloud = reproj.VoxelCloud(scene["xyz"], {"eval_bbx": EVAL_BBX}, VOXEL_SIZE, "cuda")  # no index: the current device
    depth = torch.empty(h * w, device=DEV)
    vox = torch.empty(h * w, dtype=torch.int32, device=DEV)
    cloud.trace(v["K"], v["pose"], h, w, depth, vox)
    assert cloud.seen.any() and (vox >= 0).any()
    for bad in (dict(depth=torch.empty(h * w + 1, device=DEV)), dict(depth=torch.empty(h * w, dtype=torch.float64, device=DEV)),
                dict(voxel=torch.empty(2 * h * w, dtype=torch.int32, device=DEV)[::2]), dict(voxel=torch.empty(h * w, dtype=torch.int32))):
        with pytest.raises(ValueError, match="planes are contiguous"):
            cloud.trace(v["K"], v["pose"], h, w, **bad)
    assert cloud.select(np.zeros((0, 3))).shape == (0,)
