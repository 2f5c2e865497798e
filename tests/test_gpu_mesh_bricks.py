"""GPU: marching cubes on the octree bricks (mesh.isosurface_sparse, csrc/ncw_mc_sparse.hip).

Wherever the dense path can run the result must EQUAL `isosurface(*sparse_volume(sd, values)[:2], level)` -- vertices and faces,
order included (torch.equal): G = 8 with up = 1 .. 16 over six occupancies and three kinds of values.  Above the dense ceiling
(dim 4096 and 8192) the reference is the dense path on the cut-out window: equal faces, and coordinates within the rounding of
the one addition that differs.  Then extract_mesh and scripts/extract_mesh.py end to end, and reproducibility."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)
G = 8


def _points(bricks, up):
    """gen_grid_spc's rows: fine grid index of every sub-voxel, brick-major, then local x, y, z (z fastest)."""
    k = torch.arange(up, device=bricks.device)
    kern = torch.stack(torch.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    return bricks.repeat_interleave(up ** 3, dim=0) * up + kern.repeat(bricks.shape[0], 1)


def _sparse_data(bricks, up, side):
    return {"sparse_vol": _points(bricks, up).double(), "voxel_size": 1.0, "dim": side * up, "vol_origin": np.zeros(3)}


def _dense(bricks, up, side, values, level):
    from neuralrecon_w_amd import mesh

    vol, mask, _ = mesh.sparse_volume(_sparse_data(bricks, up, side), values)
    return mesh.isosurface(vol, level, mask)


def _occupancy(kind):
    occ = torch.zeros(G, G, G, dtype=torch.bool)
    if kind == "random":
        occ = torch.rand(G, G, G, generator=torch.Generator().manual_seed(11)) < 0.4
    elif kind == "full":
        occ[:] = True
    elif kind == "isolated":
        occ[3, 4, 2] = True
    elif kind == "faces":  # the neighbours of these lie outside the lattice
        occ[G - 1, 2:5, 1:4] = True
        occ[1:4, G - 1, 3:6] = True
        occ[2:6, 0:3, G - 1] = True
        occ[G - 1, G - 1, G - 1] = True
    elif kind == "edge":  # two bricks touching along an edge only
        occ[2, 3, 4] = occ[3, 4, 4] = True
    elif kind == "corner":  # ... and two at a corner only
        occ[2, 3, 4] = occ[3, 4, 5] = True
    return torch.nonzero(occ).cuda()


def _values(kind, bricks, up, seed):
    """(values [K], level)"""
    K = bricks.shape[0] * up ** 3
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":  # every configuration, the ambiguous ones included
        return torch.randn(K, generator=g).cuda(), 0.0
    if kind == "on_level":  # values exactly on the level: zero-length edges, degenerate faces
        v = torch.randn(K, generator=g)
        v[torch.rand(K, generator=g) < 0.15] = 0.25
        return v.cuda(), 0.25
    p = _points(bricks, up).float() - (G * up - 1) / 2.0
    return (p.norm(dim=1) - 0.33 * G * up).contiguous(), 0.0


@pytest.mark.parametrize("occupancy", ["random", "full", "isolated", "faces", "edge", "corner"])
@pytest.mark.parametrize("up", [1, 2, 4, 8, 16])
def test_equals_the_dense_path(up, occupancy):
    from neuralrecon_w_amd import mesh

    bricks = _occupancy(occupancy)
    total = 0
    for i, kind in enumerate(("noise", "on_level", "sphere")):
        values, level = _values(kind, bricks, up, 100 * up + i)
        v, f = mesh.isosurface_sparse(bricks, up, values, level, G=G)
        v2, f2 = _dense(bricks, up, G, values, level)
        assert v.dtype == torch.float32 and f.dtype == torch.int64 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
        assert v.shape == v2.shape and f.shape == f2.shape, (kind, v.shape, v2.shape, f.shape, f2.shape)
        assert torch.equal(f, f2), kind
        assert torch.equal(v, v2), kind
        total += f.shape[0]
        if occupancy == "isolated" and kind == "noise" and up >= 4:
            # the only cubes of a brick on its own are its interior (up - 1)^3: no vertex on or beyond its last layer
            lo = bricks[0].float() * up
            assert bool((v >= lo).all()) and bool((v <= lo + (up - 1)).all()) and f.shape[0] > 0
    if up == 1 and occupancy in ("isolated", "edge", "corner"):
        assert total == 0  # no cube has all 8 corners
    if occupancy in ("random", "full", "faces") and up >= 2:
        assert total > 100


def test_empty_results_are_well_formed():
    from neuralrecon_w_amd import mesh

    one = torch.tensor([[3, 4, 2]], device="cuda")
    for bricks, up, values in ((one, 1, torch.randn(1, device="cuda")),                     # one point: no cube
                               (one, 8, torch.rand(512, device="cuda") + 0.5),              # all values positive
                               (_occupancy("random"), 4, torch.rand(_occupancy("random").shape[0] * 64, device="cuda") + 0.5),
                               (torch.zeros(0, 3, dtype=torch.int64, device="cuda"), 4, torch.zeros(0, device="cuda"))):
        v, f = mesh.isosurface_sparse(bricks, up, values, 0.0, G=G)
        assert v.shape == (0, 3) and v.dtype == torch.float32 and f.shape == (0, 3) and f.dtype == torch.int64
        assert v.is_cuda and f.is_cuda
        if bricks.shape[0]:
            v2, f2 = _dense(bricks, up, G, values, 0.0)
            assert torch.equal(v, v2) and torch.equal(f, f2)


def test_neighbour_table_against_a_lookup():
    from neuralrecon_w_amd import mesh

    for kind in ("random", "full", "faces", "corner"):
        bricks = _occupancy(kind)
        got = mesh.brick_neighbors(bricks.int().contiguous(), G).cpu().numpy()
        rows = [tuple(r) for r in bricks.cpu().tolist()]
        index = {r: i for i, r in enumerate(rows)}
        want = np.array([[index.get((x + (o & 1), y + ((o >> 1) & 1), z + ((o >> 2) & 1)), -1) for o in range(1, 8)]
                         for x, y, z in rows], dtype=np.int32)
        assert np.array_equal(got, want), kind


def _ulp32(x64):
    """Spacing of float32 at |x| (x given in float64 holding float32 values)."""
    a = x64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


@pytest.mark.parametrize("up", [16, 32])
def test_above_the_dense_ceiling(up):
    """G = 256: dim 4096 and 8192, lattices the dense path cannot hold (and whose weld key would overflow).  A 2 x 2 x 2 group
    of bricks at the far corner and one brick at the origin, noise values.  Reference: the dense path on each cut-out window (a
    (2 up)^3 lattice, the window's own mask), shifted back by the window's origin.  Both orders are lexicographic in (x, y, z)
    and the origin brick comes first in both, so the faces are EQUAL; `t` has the same bits on both paths and the lower grid
    point differs by the window's origin exactly, so only the final addition rounds differently:
    |global - (window + origin)| <= ulp32(global) / 2 + ulp32(window) / 2, evaluated in float64."""
    from neuralrecon_w_amd import mesh

    GG = 256
    far = torch.tensor([[x, y, z] for x in (253, 254) for y in (253, 254) for z in (253, 254)])
    bricks = torch.cat([torch.zeros(1, 3, dtype=torch.int64), far]).cuda()
    values = torch.randn(9 * up ** 3, generator=torch.Generator().manual_seed(up)).cuda()
    v, f = mesh.isosurface_sparse(bricks, up, values, 0.0, G=GG)
    verts, faces, nv = [], [], 0
    for sel, org in ((slice(0, 1), 0), (slice(1, 9), 253)):
        wv, wf = _dense(bricks[sel] - org, up, 2, values[sel.start * up ** 3:sel.stop * up ** 3], 0.0)
        assert wf.shape[0] > 1000
        verts.append((wv.double().cpu(), float(org * up)))
        faces.append(wf + nv)
        nv += wv.shape[0]
    assert v.shape[0] == nv
    assert torch.equal(f, torch.cat(faces))
    got = v.double().cpu()
    window = torch.cat([w for w, _ in verts])
    origin = torch.cat([torch.full_like(w, o) for w, o in verts])
    err = (got - (window + origin)).abs()
    bound = _ulp32(got) / 2 + _ulp32(window) / 2
    print("up %d: %d vertices, %d faces, max |global - (window + origin)| %.3e, least slack %.3e"
          % (up, nv, f.shape[0], float(err.max()), float((bound - err).min())))
    assert bool((err <= bound).all())
    assert float(got[:, 0].max()) > 254 * up  # the far group is where it belongs


def _shell_system():
    """The sphere-shell fixture of tests/test_gpu_mesh_sparse.py: G = 16, evaluation level 6."""
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import mesh, voxel
    from tests._build import build_system

    emb, neuconw, nerf, rdr = build_system(seed=2, prec=nw.PREC_F32)  # geometric init: a sphere of radius ~0.5
    side = 16
    ax = (torch.arange(side, device="cuda").float() + 0.5) * (2.0 / side) - 1.0
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt(X * X + Y * Y + Z * Z)
    shell = (r > 0.3) & (r < 0.72)
    scene_origin, scene_radius = [0.3, -0.2, 0.1], 1.7
    od = voxel.occupancy_from_dense(shell, scene_origin, scene_radius)
    od["scene_origin"] = torch.tensor(scene_origin, dtype=torch.float64, device="cuda")
    return emb, rdr, mesh.gen_grid_spc(od, eval_level=6), scene_origin, scene_radius


def test_extract_mesh_bricks_equals_dense():
    from neuralrecon_w_amd import mesh

    emb, rdr, sd, scene_origin, scene_radius = _shell_system()
    assert sd["up"] == 4 and sd["dim"] == 64
    out = {mode: mesh.extract_mesh(rdr, 0, scene_radius, scene_origin, sparse_data=sd, with_color=True,
                                   embedding_a=emb.weight[3].detach(), sparse_mc=mode) for mode in ("dense", "bricks", "auto")}
    assert out["dense"]["vertices"].shape[0] > 2000 and out["dense"]["faces"].shape[0] > 4000
    for key in ("vertices", "faces", "vertices_training", "colors"):
        assert torch.equal(out["bricks"][key], out["dense"][key]), key
        assert torch.equal(out["auto"][key], out["dense"][key]), key  # dim <= 1024: auto is the dense path


def test_reproducible_and_independent_of_the_table():
    from neuralrecon_w_amd import mesh

    bricks = _occupancy("random")
    values, level = _values("noise", bricks, 8, 5)
    first = mesh.isosurface_sparse(bricks, 8, values, level, G=G)
    again = mesh.isosurface_sparse(bricks, 8, values, level, G=G)
    table = mesh.brick_neighbors(bricks.int().contiguous(), G)
    kept = mesh.isosurface_sparse(bricks, 8, values, level, G=G, neighbors=table)
    rebuilt = mesh.isosurface_sparse(bricks, 8, values, level, G=G, neighbors=mesh.brick_neighbors(bricks.int().contiguous(), G))
    assert first[1].shape[0] > 10000
    for other in (again, kept, rebuilt):
        assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])


def test_extract_mesh_script_bricks_file_equals_dense(tmp_path):
    """scripts/extract_mesh.py on the golden COLMAP scene, two levels above its octree: the PLY of --sparse_mc bricks is the
    PLY of --sparse_mc dense, byte for byte."""
    import yaml

    from neuralrecon_w_amd import config as C
    from neuralrecon_w_amd import trainer

    scene = os.path.join(GOLDEN, "sfm_scene")
    cfg_path = str(tmp_path / "exp.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump({"DATASET": {"ROOT_DIR": scene},
                        "NEUCONW": {"SDF_CONFIG": {"d_hidden": 64, "n_layers": 4, "skip_in": "(2,)", "d_out": 65},
                                    "COLOR_CONFIG": {"d_hidden": 64, "d_feature": 64, "n_layers": 2, "head_channels": 32},
                                    "N_VOCAB": 1200, "N_SAMPLES": 8, "N_IMPORTANCE": 16}}, f)
    cfg = C.load_config(cfg_path)
    torch.manual_seed(5)
    emb, neuconw, nerf, rdr, sc = C.build_system(cfg, torch.device("cuda"))
    ckpt = str(tmp_path / "exp" / "last.ckpt")
    os.makedirs(os.path.dirname(ckpt))
    trainer.save_checkpoint(ckpt, emb, neuconw, nerf)
    lvl = int(np.load(os.path.join(GOLDEN, "sfm_octree.npz"))["level"]) + 2
    env = dict(os.environ, PYTHONPATH=ROOT)
    files = {}
    for mode in ("dense", "bricks"):
        out_dir = tmp_path / mode
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "extract_mesh.py"), "--cfg_path", cfg_path, "--ckpt_path",
                            ckpt, "--out_dir", str(out_dir), "--eval_level", str(lvl), "--sparse_mc", mode],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        files[mode] = open(out_dir / ("extracted_mesh_level_%d.ply" % lvl), "rb").read()
    head = files["dense"][:200]
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex ")
    nv = int(head.split(b"element vertex ")[1].split(b"\n")[0])
    print("level %d: %d vertices, %d bytes" % (lvl, nv, len(files["dense"])))
    assert nv > 0
    assert files["bricks"] == files["dense"]
