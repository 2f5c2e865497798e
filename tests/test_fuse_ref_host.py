"""Surface-cloud fusion without a GPU: properties of the numpy restatement (tests/_fuse_ref.py), the refusals of
surfcloud.SurfaceCloud and of the entry points (before any launch), the binding, the PLY normals and the script's flags."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from tests import _fuse_ref as FR
from tests._util import ROOT

NAMES = ("ncw_fuse_insert", "ncw_fuse_move", "ncw_fuse_resolve")


def _samples(m, seed, spread=0.4):
    g = np.random.RandomState(seed)
    p = g.uniform(-spread, spread, (m, 3)).astype(np.float32)
    n = g.normal(size=(m, 3)).astype(np.float32)
    d = -n / np.linalg.norm(n, axis=1, keepdims=True) + 0.3 * g.normal(size=(m, 3)).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    c = g.uniform(-0.2, 1.2, (m, 3)).astype(np.float32)
    return p, n, d, c


GRID = FR.make_grid((-0.5, -0.5, -0.5), 0.125, (8, 8, 8), scale=1.0, off=(0, 0, 0), cos_min=0.1)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("keys", "acc", "views")) and a["valid"] == b["valid"]


def test_restatement_is_invariant_under_permutation_and_splitting():
    p, n, d, c = _samples(3000, 0)
    whole = FR.accumulate([(p, n, d, c, 0)], GRID)
    assert whole["keys"].shape[0] > 100 and (np.diff(whole["keys"]) > 0).all() and 0 < whole["valid"] < 3000
    perm = np.random.RandomState(1).permutation(3000)
    assert _same(whole, FR.accumulate([(p[perm], n[perm], d[perm], c[perm], 0)], GRID))
    cuts = [0, 1, 500, 501, 2999, 3000]
    parts = [(p[a:b], n[a:b], d[a:b], c[a:b], 0) for a, b in zip(cuts[:-1], cuts[1:])]
    assert _same(whole, FR.accumulate(parts, GRID))
    assert _same(whole, FR.accumulate(parts[::-1], GRID))
    assert (whole["acc"][:, 0] >= 1).all() and whole["acc"][:, 0].sum() == whole["valid"] and (whole["views"] == 1).all()


def test_restatement_counts_distinct_serials():
    p, n, d, c = _samples(600, 2, spread=0.1)  # 2 x 2 x 2 cells, many samples in each
    t = FR.accumulate([(p[:200], n[:200], d[:200], c[:200], 0), (p[200:400], n[200:400], d[200:400], c[200:400], 3),
                       (p[400:500], n[400:500], d[400:500], c[400:500], 3), (p[500:], n[500:], d[500:], c[500:], 7)], GRID)
    assert t["keys"].shape[0] == 8 and (t["views"] == 3).all() and t["views"].dtype == np.int32
    one = FR.accumulate([(p, n, d, c, 5)], GRID)
    assert (one["views"] == 1).all() and np.array_equal(one["acc"], t["acc"])


def test_restatement_positions_lie_inside_their_cells_and_filters():
    p, n, d, c = _samples(4000, 3)
    p[:7] = np.float32(-0.5) + np.arange(7, dtype=np.float32)[:, None] * np.float32(0.125)  # exactly on cell boundaries
    grid = FR.make_grid((-0.5, -0.5, -0.5), 0.125, (8, 8, 8), cos_min=None)
    t = FR.accumulate([(p[:2000], n[:2000], d[:2000], c[:2000], 0), (p[2000:], n[2000:], d[2000:], c[2000:], 1)], grid)
    r = FR.resolve(t, grid)
    assert r["positions"].dtype == np.float64 and r["normals"].dtype == np.float32 and r["colours"].dtype == np.uint8
    assert FR.inside_cells(r["positions"], r["keys"], grid) and r["cells"] == t["keys"].shape[0]
    assert np.allclose(np.linalg.norm(r["normals"].astype(np.float64), axis=1), 1.0, atol=1e-6)
    r2 = FR.resolve(t, grid, min_views=2, min_count=3)
    assert 0 < r2["keys"].shape[0] < r["keys"].shape[0] and (r2["views"] >= 2).all() and (r2["count"] >= 3).all()
    # opposite normals cancel: the cell is degenerate and dropped
    one = np.float32([[0.01, 0.01, 0.01]] * 2)
    nn = np.float32([[0, 0, 1], [0, 0, -1]])
    t = FR.accumulate([(one, nn, -nn, one, 0)], grid)
    r = FR.resolve(t, grid)
    assert t["keys"].shape[0] == 1 and r["cells"] == 1 and r["degenerate"] == 1 and r["keys"].shape[0] == 0


def test_restatement_quantiser_edges():
    grid = FR.make_grid((0.0, 0.0, 0.0), 0.25, (4, 4, 4), cos_min=0.5)
    n = np.float32([[0, 0, 2.0]])
    d = np.float32([[0, 0, -1.0]])
    col = np.float32([[-1.0, 0.5, 2.0]])
    k, pay = FR.quantise(np.float32([[0.0, 0.25, 0.99999994]]), n, d, col, grid)
    assert k.tolist() == [(3 * 4 + 1) * 4 + 0] and pay[0].tolist()[:4] == [1, 0, 0, 65535]
    assert pay[0].tolist()[4:7] == [0, 0, 32767] and pay[0].tolist()[7:] == [0, 128, 255]  # 127.5 ties to even: 128
    for bad in ([1.0, 0.1, 0.1], [-1e-9, 0.1, 0.1], [np.nan, 0.1, 0.1], [np.inf, 0.1, 0.1]):  # lo + dims h is excluded
        assert FR.quantise(np.float32([bad]), n, d, col, grid)[0].tolist() == [-1]
    pt = np.float32([[0.1, 0.1, 0.1]])
    assert FR.quantise(pt, np.float32([[0, 0, 0]]), d, col, grid)[0].tolist() == [-1]
    assert FR.quantise(pt, -n, d, col, grid)[0].tolist() == [-1]  # back-facing
    half = np.float32([[0.0, np.sqrt(0.75), -0.5]])  # -n.d = 1.0 = cos_min |n| exactly: kept
    assert FR.quantise(pt, n, half, col, grid)[0].tolist() == [0]
    grid_hi = dict(grid, cos_min=np.nextafter(np.float64(0.5), 1.0))
    assert FR.quantise(pt, n, half, col, grid_hi)[0].tolist() == [-1]
    assert FR.quantise(pt, -n, d, col, dict(grid, cos_min=None))[0].tolist() == [0]  # the test switched off
    assert FR.quantise(pt, n, d, np.float32([[np.nan, np.inf, -np.inf]]), grid)[1][0].tolist()[7:] == [0, 255, 0]


def test_surface_cloud_refuses_before_any_launch(monkeypatch):
    from neuralrecon_w_amd import lib as L, surfcloud

    calls = []
    monkeypatch.setattr(L, "get_lib", lambda: calls.append(1))
    for kw in (dict(cell=0.0), dict(cell=float("nan")), dict(cell=-1.0), dict(hi=(1, 1, -1)), dict(cos_min=2.0), dict(scale=0.0),
               dict(capacity=1000), dict(capacity=0), dict(cell=1e-7), dict(capacity=64, max_capacity=32), dict(lo=(0, 0)),
               dict(offset=(0, float("inf"), 0))):
        args = dict(lo=(-1, -1, -1), hi=(1, 1, 1), cell=0.01)
        args.update(kw)
        with pytest.raises(ValueError):
            surfcloud.SurfaceCloud(**args)
    with pytest.raises(L.NeuconwHipError):
        surfcloud.SurfaceCloud(-1, 1, 0.01, device="cpu")
    cloud = surfcloud.SurfaceCloud(-1, 1, 0.01, scale=2.0, offset=(1, 2, 3), cos_min=0.1, capacity=16)
    assert cloud.dims.tolist() == [200, 200, 200] and cloud.capacity == 16
    z = torch.zeros(4, 3)
    with pytest.raises(L.NeuconwHipError):  # host tensors: no CPU fallback
        cloud.add(z, z, z, z, 0)
    with pytest.raises(L.NeuconwHipError):
        cloud.add(z.numpy(), z, z, z, 0)
    for view in (-1, 2 ** 31 - 1, 1.5):
        with pytest.raises(ValueError):
            cloud.add(z, z, z, z, view)
    cloud._last_view = 5
    with pytest.raises(ValueError, match="decrease"):
        cloud.add(z, z, z, z, 4)
    assert not calls and cloud._table is None and cloud.stats()["offered"] == 0
    with pytest.raises(ValueError):
        surfcloud.fuse_views(None, [], cloud, appearance="median")


def test_binding_matches_header():
    from neuralrecon_w_amd import lib as L

    assert set(NAMES) <= set(L.exported_symbols()) and L.ABI_VERSION >= 37
    hdr = open(os.path.join(ROOT, "include", "neuconw_hip.h")).read()
    for n in NAMES:
        assert n + "(" in hdr
    for name, val in (("ACC", L.FUSE_ACC), ("COUNTERS", L.FUSE_COUNTERS), ("EMPTY", "(%d)" % L.FUSE_EMPTY),
                      ("MAX_SERIAL", hex(L.FUSE_MAX_SERIAL))):
        assert "#define NCW_FUSE_%s %s\n" % (name, val) in hdr
    assert "#define NCW_FUSE_MAX_DIM_LOG2 %d\n" % (L.FUSE_MAX_DIM.bit_length() - 1) in hdr
    assert "#define NCW_FUSE_MAX_CAPACITY_LOG2 %d\n" % (L.FUSE_MAX_CAPACITY.bit_length() - 1) in hdr
    assert FR.ACC == L.FUSE_ACC
    import subprocess
    import tempfile

    prog = ('#include <stdio.h>\n#include "neuconw_hip.h"\nint main(){printf("%zu %zu\\n", sizeof(NcwFuseGrid), '
            'sizeof(NcwFuseTable));return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        sizes = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert sizes == [ctypes.sizeof(L.NcwFuseGrid), ctypes.sizeof(L.NcwFuseTable)]


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """Missing / misaligned pointers, counts and serials out of range, a capacity that is no power of two, h <= 0 and values
    that are not finite give NCW_E_BADARG; an empty range gives 0.  Neither launches (the pointers are never dereferenced)."""
    from neuralrecon_w_amd import lib as L

    lib = L.get_lib()
    p, q, odd = 4096, 8192, 4100

    def grid(**kw):
        v = dict(lo=(0.0, 0.0, 0.0), h=0.1, dims=(10, 10, 10), scale=1.0, off=(0.0, 0.0, 0.0), cos_min=0.1, facing=1)
        v.update(kw)
        return L.NcwFuseGrid((ctypes.c_double * 3)(*v["lo"]), v["h"], (ctypes.c_int64 * 3)(*v["dims"]), v["scale"],
                             (ctypes.c_double * 3)(*v["off"]), v["cos_min"], v["facing"], 0)

    def table(cap=1024, keys=p, acc=p, stamp=p, views=p, counters=p):
        return L.NcwFuseTable(keys, acc, stamp, views, counters, cap)

    def insert(n=16, x=p, serial=0, g=None, t=None):
        return lib.ncw_fuse_insert(x, p, p, p, n, serial, ctypes.byref(g or grid()), ctypes.byref(t or table()), None)

    def resolve(n=16, rows=p, g=None, t=None, pos=p):
        return lib.ncw_fuse_resolve(ctypes.byref(t or table()), rows, n, ctypes.byref(g or grid()), pos, p, p, p, p, p, p, None)

    def move(s, t):
        return lib.ncw_fuse_move(ctypes.byref(s), ctypes.byref(t), None)

    nan, inf = float("nan"), float("inf")
    assert insert(0) == 0 and resolve(0) == 0
    bad_grids = [grid(h=0.0), grid(h=-1.0), grid(h=nan), grid(h=inf), grid(lo=(0.0, nan, 0.0)), grid(scale=inf),
                 grid(off=(0.0, 0.0, nan)), grid(cos_min=nan), grid(dims=(0, 1, 1)), grid(dims=(1, 1, 2 ** 20 + 1))]
    bad_tables = [table(cap=0), table(cap=1000), table(cap=2 ** 37), table(keys=None), table(acc=odd), table(stamp=4098),
                  table(views=None), table(counters=odd)]
    for f in (insert, resolve):
        assert f(-1) == -1 and f(2 ** 31) == -1
        for g in bad_grids:
            assert f(g=g) == -1 and f(0, g=g) == -1
        for t in bad_tables:
            assert f(t=t) == -1
    assert insert(g=grid(cos_min=nan, facing=0), n=0) == 0  # cos_min is not read when the test is off
    assert insert(x=None) == -1 and insert(x=4098) == -1 and insert(serial=-1) == -1 and insert(serial=2 ** 31 - 1) == -1
    assert resolve(rows=None) == -1 and resolve(rows=odd) == -1 and resolve(pos=odd) == -1 and resolve(n=2048) == -1
    for t in bad_tables:
        assert move(t, table(keys=q, acc=q, stamp=q, views=q)) == -1 and move(table(), t) == -1
    assert move(table(), table()) == -1  # the same storage
    assert move(table(cap=2048), table(cap=1024, keys=q, acc=q, stamp=q, views=q)) == -1  # a smaller destination


def test_ply_normals_round_trip(tmp_path):
    from neuralrecon_w_amd import ply

    g = np.random.RandomState(0)
    xyz = g.normal(size=(50, 3)) * 1e3 + 1e-9
    nrm = g.normal(size=(50, 3)).astype(np.float32)
    rgb = g.randint(0, 256, (50, 3)).astype(np.uint8)
    path = str(tmp_path / "n.ply")
    ply.write(path, xyz, rgb=rgb, normals=nrm)
    hdr = open(path, "rb").read().split(b"end_header\n")[0].decode().split("\n")
    props = [ln.split()[-1] for ln in hdr if ln.startswith("property")]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert [ln.split()[1] for ln in hdr if ln.startswith("property")] == ["double"] * 3 + ["float"] * 3 + ["uchar"] * 3
    assert np.array_equal(ply.read_points(path), xyz)  # bit for bit
    v, f, c = ply.read_mesh(path)
    assert np.array_equal(v, xyz) and f.shape == (0, 3) and np.array_equal(c, rgb)
    assert np.array_equal(ply.read_normals(path), nrm) and ply.read_normals(path).dtype == np.float32
    # without normals the writer's bytes are what they were, and the reader says so
    plain, plain2 = str(tmp_path / "p.ply"), str(tmp_path / "p2.ply")
    ply.write(plain, xyz, rgb=rgb)
    ply.write(plain2, xyz, None, rgb, "f8", None)
    body = np.empty(50, dtype=[("p", "<f8", 3), ("c", "u1", 3)])
    body["p"], body["c"] = xyz, rgb
    want = ("ply\nformat binary_little_endian 1.0\nelement vertex 50\nproperty double x\nproperty double y\nproperty double z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode() + body.tobytes()
    assert open(plain, "rb").read() == want == open(plain2, "rb").read()
    assert ply.read_normals(plain) is None
    ply.write(path, xyz[:5], faces=np.array([[0, 1, 2]]), normals=nrm[:5], coord="f4")
    v, f, c = ply.read_mesh(path)
    assert f.tolist() == [[0, 1, 2]] and c is None and np.array_equal(ply.read_normals(path), nrm[:5])


def test_script_parses_its_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import surface_cloud as S
    finally:
        sys.path.pop(0)
    ap = S.build_parser()
    a = ap.parse_args(["--cfg_path", "c.yaml", "--ckpt_path", "k.ckpt"])
    assert (a.split, a.max_views, a.view_stride, a.cell, a.box, a.min_views, a.cos_min, a.appearance, a.out) == \
        ("train", None, 1, None, "sphere", 2, 0.1, "mean", "surface_cloud.ply")
    assert (a.trace_eps, a.trace_iters, a.trace_step, a.img_downscale, a.root_dir) == (1e-3, 64, 1.0, None, None)
    a = ap.parse_args(["--cfg_path", "c", "--ckpt_path", "k", "--root_dir", "r", "--split", "all", "--max_views", "7",
                       "--view_stride", "3", "--img_downscale", "4", "--cell", "0.02", "--box", "eval_bbx", "--min_views", "3",
                       "--cos_min", "-1", "--appearance", "12", "--trace_eps", "1e-4", "--trace_iters", "32", "--trace_step",
                       "0.5", "--out", "o.ply"])
    assert (a.split, a.max_views, a.view_stride, a.img_downscale, a.cell, a.box, a.min_views, a.cos_min) == \
        ("all", 7, 3, 4, 0.02, "eval_bbx", 3, -1.0)
    assert S.appearance_of(a.appearance) == 12 and S.appearance_of("mean") == "mean" and S.appearance_of("view") == "view"
    with pytest.raises(SystemExit):
        ap.parse_args(["--cfg_path", "c", "--ckpt_path", "k", "--box", "cube"])
    scene = {"ids": [5, 6, 7, 8, 9, 10], "ids_train": [5, 7, 8, 10]}
    assert S.select_ids(scene, "train", 1, None) == [5, 7, 8, 10] and S.select_ids(scene, "test", 1, None) == [6, 9]
    assert S.select_ids(scene, "all", 2, 2) == [5, 7] and S.select_ids(scene, "train", 3, None) == [5, 10]
    cfg = {"origin": [1.0, 2.0, 3.0], "radius": 2.0, "eval_bbx": [[0, 0, 0], [2, 4, 6]],
           "sfm2gt": [[2.0, 0, 0, 1.0], [0, 2.0, 0, 0], [0, 0, 2.0, 0], [0, 0, 0, 1]]}
    lo, hi = S.grid_box(cfg, "sphere")
    assert lo.tolist() == [-1.0, 0.0, 1.0] and hi.tolist() == [3.0, 4.0, 5.0]
    lo, hi = S.grid_box(cfg, "eval_bbx")
    assert lo.tolist() == [-0.5, 0.0, 0.0] and hi.tolist() == [0.5, 2.0, 3.0]
