"""GPU: the face-preserving reprojection filter (reproj.reproj_filter keep_faces, scripts/eval_pipeline.py --keep_faces) and the
component clean-up of the extraction (mesh.extract_mesh largest_components).  The scene is the one of tests/test_gpu_reproj.py --
a box on a ground plane, a wall, a sphere hidden behind the wall, three views -- plus a visible three-triangle island.  The
marks themselves are pinned there; here the mesh is checked against the per-vertex flags that reprojected.ply was written
from (recovered from its rows: no two vertices of the scene share coordinates AND colour), with the numpy restatement of the face
rule, the component filter and the compaction (tests/_meshops_ref.py): exact equality."""
import json
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import _meshops_ref as R
from tests._util import ROOT
from tests.test_gpu_reproj import SFM2GT, _hidden_scene, _write_workspace

from neuralrecon_w_amd import evalmesh, mesh, ply, reproj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL = 0.02
ISLAND = 4  # its label


def _scene_with_island():
    """The hidden scene and a fan of three triangles floating 0.1 above the ground, facing up, in plain view of every camera:
    its own five vertices, so a component of three faces."""
    verts, faces, lab = _hidden_scene()
    n0 = len(verts)
    c = np.array([0.9, -0.3, 0.1])  # beside the box, clear of its shadow
    rim = [c + 0.15 * np.array([np.cos(t), np.sin(t), 0.0]) for t in (0.0, 1.2, 2.4, 3.6)]
    verts = np.concatenate([verts, np.array([c] + rim, np.float32)]).astype(np.float32)
    faces = np.concatenate([faces, np.array([[n0, n0 + 1 + k, n0 + 2 + k] for k in range(3)])])
    return verts, faces, np.concatenate([lab, np.full(5, ISLAND)])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("reproj_faces")
    verts, faces, lab = _scene_with_island()
    root = str(tmp / "scene")
    _write_workspace(root, SFM2GT)
    mesh_file = str(tmp / "mesh.ply")
    rgb = (np.arange(len(verts))[:, None] * np.array([7, 13, 29]) % 256).astype(np.uint8)
    mesh.write_ply(mesh_file, torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(rgb))
    xyz = evalmesh.apply_transform(verts.astype(np.float64), SFM2GT)
    out = {"verts": verts, "faces": faces, "lab": lab, "rgb": rgb, "xyz": xyz, "root": root, "mesh_file": mesh_file, "tmp": tmp}
    for name, kw in (("plain", {}), ("mc1", {"keep_faces": True}), ("mc3", {"keep_faces": True, "min_corners": 3}),
                     ("comp", {"keep_faces": True, "min_component_faces": 4})):
        d = str(tmp / name)
        rows = reproj.reproj_filter(mesh_file, mesh_file, root, d, voxel_size=VOXEL, verbose=False, **kw)
        out[name] = {"dir": d, "rows": rows}
    return out


def _flags(s, d):
    """The per-vertex flags reprojected.ply of directory d was written from."""
    gx, _, gc = ply.read_mesh(os.path.join(d, "reprojected.ply"))
    m = (np.abs(gx[:, None] - s["xyz"][None]).max(-1) <= 1e-12) & (gc[:, None] == s["rgb"][None]).all(-1)
    assert (m.sum(1) == 1).all()  # a row is one vertex: coincident vertices (shared edges, the sphere's poles) differ in colour
    flags = np.zeros(len(s["xyz"]), dtype=np.uint8)
    flags[m.argmax(1)] = 1
    return flags


def _check_mesh_file(s, d, flags, min_corners, min_component_faces=0):
    """reprojected_mesh.ply of d equals the restatement from the flags, bit for bit; returns (kept faces in old indices, old
    vertex index of every written vertex)."""
    V = len(s["xyz"])
    keep = R.face_select(s["faces"], V, flags, min_corners)
    if min_component_faces:
        labels, sizes = R.components(s["faces"], V, keep)
        keep = R.face_select(s["faces"], V, flags, min_corners, labels, R.select_components(sizes, min_component_faces))
    rv, rf, rc, ridx = R.submesh(s["xyz"], s["faces"], keep, s["rgb"])
    gv, gf, gc = ply.read_mesh(os.path.join(d, "reprojected_mesh.ply"))
    assert gf.shape[0] == int(keep.sum()) > 0                             # the face count is the reference's count from the flags
    assert np.array_equal(gf, rf) and np.array_equal(gv, rv) and np.array_equal(gc, rc)  # file order, doubles, colours
    head = open(os.path.join(d, "reprojected_mesh.ply"), "rb").read(400)
    assert b"property double x" in head and b"property uchar red" in head and b"element face %d" % gf.shape[0] in head
    return s["faces"][keep != 0], ridx


@pytest.mark.parametrize("name,min_corners", [("mc1", 1), ("mc3", 3)])
def test_kept_faces_follow_the_flags(runs, name, min_corners):
    d = runs[name]["dir"]
    flags = _flags(runs, d)
    kept, idx = _check_mesh_file(runs, d, flags, min_corners)
    assert (flags[kept].sum(1) >= min_corners).all()                       # every kept face has its marked corners
    assert not (runs["lab"][kept] == 3).any() and not (runs["lab"][idx] == 3).any()  # nothing of the sphere behind the wall
    if min_corners == 3:
        assert flags[idx].all()                                            # the vertex set is a subset of reprojected.ply's rows
    else:
        assert (runs["lab"][kept[:, 0]] == 0).sum() > 100 and (runs["lab"][kept[:, 0]] == 2).sum() > 5
        assert not flags[idx].all()                                        # the one-ring rule admits unmarked corners


def test_min_corners_orders_the_results(runs):
    n1 = ply.read_mesh(os.path.join(runs["mc1"]["dir"], "reprojected_mesh.ply"))[1].shape[0]
    n3 = ply.read_mesh(os.path.join(runs["mc3"]["dir"], "reprojected_mesh.ply"))[1].shape[0]
    assert 0 < n3 < n1 < len(runs["faces"])


def test_reprojected_ply_is_byte_identical_and_the_return_value_unchanged(runs):
    want = open(os.path.join(runs["plain"]["dir"], "reprojected.ply"), "rb").read()
    assert not os.path.exists(os.path.join(runs["plain"]["dir"], "reprojected_mesh.ply"))
    for name in ("mc1", "mc3", "comp"):
        assert open(os.path.join(runs[name]["dir"], "reprojected.ply"), "rb").read() == want, name
        for a, b in zip(runs[name]["rows"], runs["plain"]["rows"]):
            assert np.array_equal(a, b) and a.dtype == b.dtype


def test_min_component_faces_removes_the_visible_island(runs):
    flags = _flags(runs, runs["comp"]["dir"])
    with_island, _ = _check_mesh_file(runs, runs["mc1"]["dir"], flags, 1)
    assert (runs["lab"][with_island[:, 0]] == ISLAND).any()                # it is visible: the plain rule keeps some of it
    kept, idx = _check_mesh_file(runs, runs["comp"]["dir"], flags, 1, 4)
    assert not (runs["lab"][kept] == ISLAND).any() and not (runs["lab"][idx] == ISLAND).any()
    assert (runs["lab"][kept[:, 0]] == 0).sum() > 100


def test_point_cloud_source_yields_a_mesh_when_the_target_has_faces(runs):
    cloud = str(runs["tmp"] / "cloud.ply")
    g = np.linspace(-2, 2, 161)
    ground = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    ply.write(cloud, np.c_[ground, np.zeros(len(ground))])                 # a dense ground plane, SfM frame, no faces
    d = str(runs["tmp"] / "from_cloud")
    reproj.reproj_filter(cloud, runs["mesh_file"], runs["root"], d, voxel_size=0.1, verbose=False, keep_faces=True, min_corners=2)
    flags = _flags(runs, d)
    assert 0 < flags.sum() < len(flags)
    kept, _ = _check_mesh_file(runs, d, flags, 2)
    assert (runs["lab"][kept[:, 0]] == 0).any()
    plain = str(runs["tmp"] / "from_cloud_plain")
    reproj.reproj_filter(cloud, runs["mesh_file"], runs["root"], plain, voxel_size=0.1, verbose=False)
    assert open(os.path.join(plain, "reprojected.ply"), "rb").read() == open(os.path.join(d, "reprojected.ply"), "rb").read()


def test_keep_faces_refuses_a_target_without_faces(runs):
    cloud = str(runs["tmp"] / "target_cloud.ply")
    ply.write(cloud, runs["xyz"])
    d = str(runs["tmp"] / "refused")
    with pytest.raises(ValueError, match="keep_faces needs a target with faces"):
        reproj.reproj_filter(runs["mesh_file"], cloud, runs["root"], d, voxel_size=VOXEL, verbose=False, keep_faces=True)
    assert not os.path.exists(os.path.join(d, "reprojected.ply"))


def test_eval_pipeline_scores_the_filtered_mesh_by_its_surface(tmp_path):
    """scripts/eval_pipeline.py --keep_faces --sample_surface --exact_recall runs to the end on a Heritage-Recon layout."""
    verts, faces, _ = _scene_with_island()
    scene = "brandenburg_gate"
    root = str(tmp_path / "data")
    sdir = os.path.join(root, scene)
    _write_workspace(sdir, np.eye(4))  # identity sfm2gt: the two steps chain only then
    pred = str(tmp_path / "run")
    os.makedirs(os.path.join(pred, "mesh"))
    mesh.write_ply(os.path.join(pred, "mesh", "extracted_mesh_level_10_colored.ply"), torch.from_numpy(verts),
                   torch.from_numpy(faces), torch.zeros(len(verts), 3, dtype=torch.uint8))
    rng = np.random.RandomState(4)
    g = rng.uniform(-2, 2, (6000, 2))
    g = g[~((np.abs(g[:, 0]) < 0.4) & (g[:, 1] > -0.9) & (g[:, 1] < -0.1)) & (g[:, 1] < 1.0)]
    top = np.c_[rng.uniform(-0.4, 0.4, (600, 2)) + [0, -0.5], np.full(600, 0.5)]
    wall = np.c_[rng.uniform(-1.4, 1.4, 800), np.full(800, 1.0), rng.uniform(0, 1.6, 800)]
    gt = np.concatenate([np.c_[g, np.zeros(len(g))], top, wall])
    mesh.write_ply(os.path.join(sdir, scene + ".ply"), torch.from_numpy(gt), torch.zeros(0, 3, dtype=torch.int64))
    os.makedirs(os.path.join(sdir, "neuralsfm"))
    sfm = gt[rng.choice(len(gt), 400, replace=False)]
    with open(os.path.join(sdir, "neuralsfm", "points3D.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(sfm)))
        for i, p in enumerate(sfm):
            fh.write(struct.pack("<QdddBBBd", i + 1, *p, 1, 2, 3, 0.5) + struct.pack("<Q", 20) + struct.pack("<40i", *([1, i] * 20)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_pipeline.py"), "--scene_name", scene, "--pred_dir", pred,
                        "--data_root", root, "--keep_faces", "--sample_surface", "--exact_recall"], capture_output=True, text=True,
                       cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.path.isfile(os.path.join(pred, "mesh", "reprojected.ply"))
    assert ply.read_mesh(os.path.join(pred, "mesh", "reprojected_mesh.ply"))[1].shape[0] > 100
    m = json.load(open(os.path.join(pred, "mesh", "eval_%s_reprojected_mesh.ply" % scene, "metrics.json")))
    assert m["recal_mode"] == "exact"
    assert m["thresholds"] == evalmesh.parse_thresholds(reproj.SCENES[scene]["thresholds"])
    assert not os.path.exists(os.path.join(pred, "mesh", "eval_%s_reprojected.ply" % scene))
    assert len(m["recals"]) == len(m["precs"]) == len(m["thresholds"]) and 0 < m["recals"][-1] <= 1 and 0 < m["precs"][-1] <= 1


class _AnalyticRenderer:
    """What mesh.extract_mesh touches of a renderer, over an analytic SDF; records the points the colour pass sees."""
    infer_prec = 0

    def __init__(self):
        self.neuconw = types.SimpleNamespace(parameters=lambda: iter([torch.zeros(1, device=DEV)]), sdf_net=None)
        self.seen = []

    def rgb(self, p, d, a):
        self.seen.append(p.reshape(-1, 3).clone())
        return torch.full((p.shape[0], 3), 0.5, device=p.device)


def test_extract_mesh_keeps_the_larger_sphere_and_colours_only_it(monkeypatch):
    dim = 48
    ca, ra, cb, rb = torch.tensor([-0.3, 0.0, 0.0], device=DEV), 0.5, torch.tensor([0.6, 0.1, 0.0], device=DEV), 0.2

    def sdf_grid(net, dim, lo, hi, prec=None, group=None):
        ax = [torch.linspace(lo[k], hi[k], dim, device=DEV) for k in range(3)]
        P = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1)
        return torch.minimum((P - ca).norm(dim=-1) - ra, (P - cb).norm(dim=-1) - rb).reshape(-1)

    monkeypatch.setattr(mesh._grid, "sdf_grid", sdf_grid)
    a = torch.zeros(4, device=DEV)
    rdr = _AnalyticRenderer()
    both = mesh.extract_mesh(rdr, dim, 2.0, [1.0, 2.0, 3.0], with_color=True, embedding_a=a)
    vt = both["vertices_training"]
    on_a = ((vt - ca).norm(dim=-1) - ra).abs() < 0.02
    on_b = ((vt - cb).norm(dim=-1) - rb).abs() < 0.02
    assert int(on_a.sum()) > 500 and int(on_b.sum()) > 50 and bool((on_a ^ on_b).all())
    assert sum(p.shape[0] for p in rdr.seen) == vt.shape[0]
    rdr = _AnalyticRenderer()
    one = mesh.extract_mesh(rdr, dim, 2.0, [1.0, 2.0, 3.0], with_color=True, embedding_a=a, largest_components=1)
    assert torch.equal(one["vertices_training"], vt[on_a]) and torch.equal(one["vertices"], both["vertices"][on_a])  # order kept
    fa = both["faces"][on_a[both["faces"][:, 0]]]
    remap = torch.cumsum(on_a.long(), 0) - 1
    assert one["faces"].dtype == both["faces"].dtype and torch.equal(one["faces"], remap[fa])
    seen = torch.cat(rdr.seen)
    assert torch.equal(seen, one["vertices_training"])                      # the colour pass saw that sphere's vertices only
    assert one["colors"].shape == (int(on_a.sum()), 3) and one["colors"].dtype == torch.uint8
    many = mesh.extract_mesh(_AnalyticRenderer(), dim, 2.0, [1.0, 2.0, 3.0], min_component_faces=10)
    assert torch.equal(many["vertices"], both["vertices"]) and torch.equal(many["faces"], both["faces"])  # both are large
