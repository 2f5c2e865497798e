"""surfcloud.fuse_views end to end on the GPU: four small traced views of a network at geometric initialisation (the surface of
tests/test_gpu_trace.py's fixture A) fused into one cloud, bit for bit against the numpy restatement (tests/_fuse_ref.py) fed
with the samples captured through trace_view's `on_hits`; the hook leaves the planes alone; the written PLY is scored by
evalmesh.eval_mesh as it stands."""
import functools

import numpy as np
import pytest
import torch

from tests import _fuse_ref as FR
from tests import _trace_ref as TR
from tests._build import build_system

pytestmark = pytest.mark.gpu

W, H, FOCAL = 48, 32, 40.0
EYES = ((0.1, -0.05, 1.6), (1.6, 0.1, 0.05), (-0.1, 0.3, -1.6), (-1.2, 0.5, -1.0))
TS = (3, 7, 7, 11)
CHUNK = 500  # four chunks per view, the last one short
# the cloud's frame: x = 3 p + offset (a scene radius and origin), 0.25-unit cells over offset +- 2.4
SCALE, OFFSET, CELL, COS = 3.0, (10.0, -5.0, 2.0), 0.25, 0.1
LO, HI = tuple(o - 2.4 for o in OFFSET), tuple(o + 2.4 for o in OFFSET)
OUT_KEYS = ("positions", "normals", "colours", "count", "views", "keys")


@functools.lru_cache(maxsize=None)
def _system():
    emb, neuconw, nerf, rdr = build_system(W=64)
    fx = TR.FIXTURES["A"]
    neuconw.sdf_net = TR.mk_net(fx["W"], fx["n_layers"], fx["skip"], jitter=fx["jitter"]).cuda()
    return emb, neuconw, rdr


def _cameras():
    from neuralrecon_w_amd import views

    K = np.array([[FOCAL, 0, W / 2.0], [0, FOCAL, H / 2.0], [0, 0, 1]], dtype=np.float32)
    return [(views.Camera(K, TR.look_at(eye).astype(np.float32), W, H, TR.VIEW_NEAR, TR.VIEW_FAR), ts)
            for eye, ts in zip(EYES, TS)]


def _cloud(**kw):
    from neuralrecon_w_amd import surfcloud

    return surfcloud.SurfaceCloud(LO, HI, CELL, scale=SCALE, offset=OFFSET, cos_min=COS, **kw)


@functools.lru_cache(maxsize=None)
def _captured(appearance):
    """[(points, grads, dirs, colours, serial)] per chunk, captured through on_hits from trace_view runs of the four views, and
    the number of hits."""
    from neuralrecon_w_amd import surfcloud, views

    emb, _, rdr = _system()
    a_code = surfcloud.mean_appearance(rdr) if appearance == "mean" else None
    batches = []
    for serial, (cam, ts) in enumerate(_cameras()):
        def grab(p0, hit, pts, dirs, rgb, grad, serial=serial):
            assert hit.dtype == torch.int64 and bool((hit[1:] > hit[:-1]).all()) and 0 <= int(hit[0]) and int(hit[-1]) < CHUNK
            assert pts.shape == dirs.shape == rgb.shape == grad.shape == (hit.numel(), 3)
            batches.append(tuple(t.detach().float().cpu().numpy().copy() for t in (pts, grad, dirs, rgb)) + (serial,))

        views.trace_view(rdr, cam, ts, a_code=a_code, chunk=CHUNK, on_hits=grab)
    return batches, sum(len(b[0]) for b in batches)


@pytest.mark.parametrize("appearance", ["mean", "view"])
def test_fuse_views_equals_the_restatement_of_the_captured_samples(appearance):
    """Pins the frame (scale / offset), the serials (the view's position in the list), the facing test and the filters."""
    from neuralrecon_w_amd import surfcloud

    rdr = _system()[2]
    batches, hits = _captured(appearance)
    assert hits > 1500 and len({b[4] for b in batches}) == 4
    grid = FR.grid_of(LO, HI, CELL, SCALE, OFFSET, COS)
    ref = FR.accumulate(batches, grid)
    # the fixture's surface is bumpy (|p| from 0.29 to 1.11): part of it lies outside the box, a few hits graze -- both filters act
    assert ref["keys"].shape[0] > 150 and ref["views"].max() >= 2 and hits // 2 < ref["valid"] < hits
    cloud = _cloud(capacity=256)
    seen = []
    tot = surfcloud.fuse_views(rdr, _cameras(), cloud, appearance=appearance, chunk=CHUNK,
                               on_view=lambda serial, out: seen.append((serial, out["stats"]["hit"])))
    assert tot["views"] == 4 and tot["samples"] == tot["hit"] == hits and tot["rays"] == 4 * W * H
    assert [s for s, _ in seen] == [0, 1, 2, 3] and sum(h for _, h in seen) == hits
    tab = cloud.table()
    for k in ("keys", "acc", "views"):
        assert np.array_equal(tab[k].cpu().numpy(), ref[k]), k
    for filters in (dict(), dict(min_views=2), dict(min_views=2, min_count=3)):
        out, want = cloud.finish(**filters), FR.resolve(ref, grid, **filters)
        for k in OUT_KEYS:
            got = out[k].cpu().numpy()
            assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), (k, filters)
        assert FR.inside_cells(out["positions"].cpu().numpy(), out["keys"].cpu().numpy(), grid)
        assert out["keys"].numel() > 0
    st = cloud.stats()
    assert (st["offered"], st["valid"], st["cells"], st["overflow"]) == (hits, ref["valid"], ref["keys"].shape[0], 0)
    assert st["growths"] >= 1


def test_appearance_choices_differ_only_in_colour():
    (ma, _), (vi, _) = _captured("mean"), _captured("view")
    assert len(ma) == len(vi)
    for a, b in zip(ma, vi):
        assert all(np.array_equal(a[i], b[i]) for i in (0, 1, 2)) and a[4] == b[4]
    assert any(not np.array_equal(a[3], b[3]) for a, b in zip(ma, vi))


def test_on_hits_leaves_the_planes_alone():
    from neuralrecon_w_amd import views

    rdr = _system()[2]
    cam, ts = _cameras()[3]
    bg = [0.25, 0.5, 0.75]
    plain = views.trace_view(rdr, cam, ts, chunk=CHUNK, background_rgb=bg)
    calls = []
    hooked = views.trace_view(rdr, cam, ts, chunk=CHUNK, background_rgb=bg, on_hits=lambda *a: calls.append(a[0]))
    assert calls == sorted(calls) and 1 <= len(calls) <= 4 and plain["stats"] == hooked["stats"]
    for k in ("color", "depth", "normal", "state", "iters", "depth_vis"):
        assert torch.equal(plain[k], hooked[k]), k
    with pytest.raises(ValueError):
        views.trace_view(rdr, cam, ts, shade=False, on_hits=lambda *a: None)


def test_written_ply_is_scored_by_eval_mesh(tmp_path):
    """The PLY (double xyz, float normals, uchar rgb) goes through evalmesh.eval_mesh's point branch against a synthetic target:
    the cloud itself carried to the GT frame, so every distance is zero and the score is 1."""
    from neuralrecon_w_amd import evalmesh, ply, surfcloud

    rdr = _system()[2]
    cloud = _cloud()
    surfcloud.fuse_views(rdr, _cameras(), cloud, chunk=CHUNK)
    out = cloud.finish(min_views=2)
    pos, nrm, rgb = (out[k].cpu().numpy() for k in ("positions", "normals", "colours"))
    pred = str(tmp_path / "surface_cloud.ply")
    ply.write(pred, pos, rgb=rgb, normals=nrm)
    assert np.array_equal(ply.read_points(pred), pos) and np.array_equal(ply.read_normals(pred), nrm)
    assert np.array_equal(ply.read_mesh(pred)[2], rgb)
    sfm2gt = np.eye(4)
    sfm2gt[:3, :3] *= 2.0
    sfm2gt[:3, 3] = (1.0, 2.0, 3.0)
    gt = pos[::-1] * 2.0 + sfm2gt[:3, 3]
    trgt = str(tmp_path / "gt.ply")
    ply.write(trgt, gt)
    cfg = {"sfm2gt": sfm2gt.tolist(), "eval_bbx": [(gt.min(0) - 1.0).tolist(), (gt.max(0) + 1.0).tolist()]}
    m = evalmesh.eval_mesh(pred, trgt, cfg, is_mesh=False, threshold=0.1, verbose=False, surface=None)
    assert m["fscore"] == 1.0 and m["prec"] == 1.0 and m["recal"] == 1.0
    assert ply.read_points(str(tmp_path / "eval_eval" / "down_pred_in_gt.ply")).shape == pos.shape


def test_surface_cloud_script_on_the_synthetic_scene(tmp_path):
    """scripts/surface_cloud.py end to end on the synthetic scene directory of tests/test_gpu_train_driver.py: three registered
    images, weights at initialisation; the PLY and the report agree with each other."""
    import json
    import os
    import struct
    import subprocess
    import sys

    from neuralrecon_w_amd import config as Cfg
    from neuralrecon_w_amd import ply, trainer
    from tests._util import ROOT
    from tests.test_gpu_train_driver import _write_scene

    root = str(tmp_path / "scene")
    cfg_path = _write_scene(root, n_chunks=1)
    sp = os.path.join(root, "dense", "sparse")
    iw, ih = 40, 24
    with open(os.path.join(sp, "cameras.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", 1) + struct.pack("<iiQQ", 1, 1, iw, ih) + struct.pack("<4d", 52.0, 52.0, iw / 2, ih / 2))
    names = [(5, "a.png", "train"), (6, "b.png", "train"), (7, "t.png", "test")]
    with open(os.path.join(sp, "images.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(names)))
        for iid, name, _ in names:
            fh.write(struct.pack("<i7di", iid, 1.0, 0.0, 0.0, 0.0, 0.02 * iid, 0.0, 2.0, 1) + name.encode() + b"\x00" + struct.pack("<Q", 0))
    with open(os.path.join(root, "synth.tsv"), "w") as fh:
        fh.write("filename\tid\tsplit\tdataset\n" + "".join("%s\t%d\t%s\tsynthetic\n" % (n, i, s) for i, n, s in names))
    torch.manual_seed(0)
    emb, neuconw, nerf, _, _ = Cfg.build_system(Cfg.load_config(cfg_path), torch.device("cuda"), None)
    ckpt = os.path.join(root, "w.ckpt")
    trainer.save_checkpoint(ckpt, emb, neuconw, nerf)
    out = str(tmp_path / "out" / "surface_cloud.ply")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "surface_cloud.py"), "--cfg_path", cfg_path, "--ckpt_path", ckpt,
                        "--root_dir", root, "--img_downscale", "1", "--cell", "0.05", "--box", "eval_bbx", "--min_views", "2",
                        "--chunk", "500", "--prec", "f32", "--out", out], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rep = json.load(open(out + ".report.json"))
    assert rep["views"] == 2 and rep["image_ids"] == [5, 6] and rep["rays"] == 2 * iw * ih and rep["dims"] == [40, 40, 40]
    # most intervals of this scene start below the untrained surface (INSIDE): the SfM octree's near / far, not the tracer's
    assert abs(sum(rep["state_share"].values()) - 1.0) < 1e-12 and rep["state_share"]["hit"] > 0
    assert rep["samples"] == rep["samples_valid"] + rep["samples_invalid"] and rep["samples_valid"] > 0
    assert 0 < rep["cells_kept"] <= rep["cells"] and set(rep["ms"]) >= {"device_trace", "device_networks", "device_fuse"}
    v, f, c = ply.read_mesh(out)
    n = ply.read_normals(out)
    assert v.shape == (rep["cells_kept"], 3) and f.shape[0] == 0 and c.shape == v.shape and n.shape == v.shape
    assert np.allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1.0, atol=1e-6) and (np.abs(v) <= 1.0).all()
