"""CPU: the brick-sparse marching cubes (mesh.isosurface_sparse, csrc/ncw_mc_sparse.hip) as far as it goes without a GPU: the
binding, the command-line flag, every refusal (ValueError in Python, NCW_E_BADARG from the entry points, both before any launch)
and the two keys gen_grid_spc adds.  The kernels are compared with the dense path in tests/test_gpu_mesh_bricks.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from tests._util import ROOT

from neuralrecon_w_amd import lib as L
from neuralrecon_w_amd import mesh

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("ncw_mcs_neighbors", "ncw_mcs_count", "ncw_mcs_cube_ids", "ncw_mcs_emit")


def test_new_symbols_are_bound_and_declared():
    assert set(NAMES) <= set(L.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "neuconw_hip.h")).read()
    for n in NAMES:
        assert n + "(" in hdr, n
    assert L.ABI_VERSION >= 34
    lib = L.get_lib()
    for n in NAMES:
        assert hasattr(lib, n)


def test_the_flag_parses():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import extract_mesh
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    base = ["--cfg_path", "a.yaml", "--ckpt_path", "b.ckpt"]
    assert extract_mesh.parse_args(base).sparse_mc == "auto"
    for mode in ("auto", "dense", "bricks"):
        assert extract_mesh.parse_args(base + ["--sparse_mc", mode]).sparse_mc == mode
    with pytest.raises(SystemExit):
        extract_mesh.parse_args(base + ["--sparse_mc", "lattice"])


def _bricks(rows):
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)


def test_python_refusals():
    """Each raises ValueError before the device is looked at (the tensors here are on the CPU); a well-formed call then fails
    because there is no CPU fallback."""
    b = _bricks([[0, 0, 1], [0, 1, 0], [2, 0, 0]])
    for up in (0, -2, 3, 6, 12, 64):
        with pytest.raises(ValueError, match="power of two"):
            mesh.isosurface_sparse(b, up, torch.zeros(3 * abs(up) ** 3), G=4)
    with pytest.raises(ValueError, match="values"):
        mesh.isosurface_sparse(b, 2, torch.zeros(23), G=4)
    with pytest.raises(ValueError, match="values"):
        mesh.isosurface_sparse(b, 2, torch.zeros(25), G=4)
    # K = 65537 * 32^3 = 2^31 + 32768: the values are one element seen K times, nothing of that size is allocated
    n = 65537
    many = torch.stack([torch.zeros(n, dtype=torch.int64), torch.arange(n) // 512, torch.arange(n) % 512], 1)
    with pytest.raises(ValueError, match="2\\^31"):
        mesh.isosurface_sparse(many, 32, torch.zeros(1).expand(n * 32 ** 3), G=512)
    with pytest.raises(ValueError, match="16384"):
        mesh.isosurface_sparse(b, 2, torch.zeros(24), G=8193)
    with pytest.raises(ValueError, match="16384"):
        mesh.isosurface_sparse(b, 32, torch.zeros(3 * 32 ** 3), G=513)
    for rows, what in (([[0, 1, 0], [0, 0, 1], [2, 0, 0]], "ascending"), ([[0, 0, 1], [0, 0, 1], [2, 0, 0]], "ascending"),
                       ([[2, 0, 0], [0, 1, 0], [0, 0, 1]], "ascending"), ([[0, 0, 1], [0, 1, 0], [4, 0, 0]], "outside"),
                       ([[0, 0, -1], [0, 1, 0], [2, 0, 0]], "outside"), ([[0, 0, 1], [0, 4, 0], [2, 0, 0]], "outside")):
        with pytest.raises(ValueError, match=what):
            mesh.isosurface_sparse(_bricks(rows), 2, torch.zeros(24), G=4)
    with pytest.raises(ValueError, match="integer"):
        mesh.isosurface_sparse(b.float(), 2, torch.zeros(24), G=4)
    with pytest.raises(ValueError, match="G is required"):
        mesh.isosurface_sparse(b, 2, torch.zeros(24), G=None)
    with pytest.raises(L.NeuconwHipError, match="no CPU fallback"):
        mesh.isosurface_sparse(b, 2, torch.zeros(24), G=4)


def test_extract_mesh_refuses_its_modes_before_the_sweep():
    class R:  # extract_mesh reads the device off the renderer first; nothing else of it is reached
        class neuconw:
            @staticmethod
            def parameters():
                return iter([torch.zeros(1)])

    sd = {"sparse_vol": torch.zeros(8, 3, dtype=torch.float64), "voxel_size": 1.0, "dim": 2048, "vol_origin": np.zeros(3)}
    with pytest.raises(ValueError, match="auto / dense / bricks"):
        mesh.extract_mesh(R, 0, 1.0, [0, 0, 0], sparse_data=sd, sparse_mc="lattice")
    with pytest.raises(ValueError, match="stops at 1024"):
        mesh.extract_mesh(R, 0, 1.0, [0, 0, 0], sparse_data=sd, sparse_mc="dense")
    for mode in ("auto", "bricks"):  # above 1024 auto is the brick path: it needs the two keys
        with pytest.raises(ValueError, match="'bricks' and 'up'"):
            mesh.extract_mesh(R, 0, 1.0, [0, 0, 0], sparse_data=sd, sparse_mc=mode)
    with pytest.raises(ValueError, match="'bricks' and 'up'"):
        mesh.extract_mesh(R, 0, 1.0, [0, 0, 0], sparse_data=dict(sd, dim=64), sparse_mc="bricks")


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """NCW_E_BADARG (-1) for every shape the header lists, 0 for an empty range; neither launches, so this runs without a GPU
    (the pointers handed in are never dereferenced)."""
    lib = L.get_lib()
    p = ctypes.c_void_p(4096)  # non-NULL, never read

    def count(n=3, up=2, G=4, nv=None, x=p):
        return lib.ncw_mcs_count(x, n * up ** 3 if nv is None else nv, p, p, n, up, G, 0.0, p, p, None)

    def emit(n=3, up=2, G=4, nv=None, M=1, T=1, x=p):
        return lib.ncw_mcs_emit(x, n * up ** 3 if nv is None else nv, p, p, n, up, G, 0.0, p, p, p, p, p, M, T, p, p, None)

    def ids(n=3, up=2, G=4, M=1, x=p):
        return lib.ncw_mcs_cube_ids(x, n, up, G, p, M, p, None)

    for fn in (count, emit, ids):
        for up in (0, -1, 3, 6, 24, 64):
            assert fn(up=up) == -1, (fn.__name__, up)
        assert fn(n=-1) == -1 and fn(G=0) == -1
        assert fn(up=2, G=8193) == -1 and fn(up=32, G=513) == -1          # G * up > 16384
        assert fn(n=65537, up=32, G=512) == -1                            # K = 2^31 + 32768
        assert fn(x=None) == -1                                           # a missing pointer
    for fn in (count, emit):
        assert fn(nv=23) == -1 and fn(nv=25) == -1                        # len(values) != n * up^3
    assert count(n=0) == 0 and emit(M=0, T=0) == 0 and ids(M=0) == 0      # nothing to do: 0 without a launch
    assert emit(M=-1) == -1 and emit(M=25) == -1 and ids(M=25) == -1      # more cubes than sub-voxels
    assert emit(M=2, T=11) == -1 and emit(M=2, T=-1) == -1                # more than 5 triangles per cube
    nb = lib.ncw_mcs_neighbors
    assert nb(p, 0, 4, p, None) == 0
    assert nb(p, -1, 4, p, None) == -1 and nb(p, 1 << 31, 4, p, None) == -1
    assert nb(p, 3, 0, p, None) == -1 and nb(p, 3, 16385, p, None) == -1
    assert nb(None, 3, 4, p, None) == -1 and nb(p, 3, 4, None, None) == -1


def test_gen_grid_spc_blocking_keys():
    """bricks / up describe the rows of sparse_vol: row b * up^3 + (lx * up + ly) * up + lz is sub-voxel (lx, ly, lz) of
    bricks[b].  Restated on the CPU from the points themselves; every key the reference's dict has is untouched (the golden
    comparison of tests/test_grid_spc.py covers their values)."""
    z = np.load(os.path.join(GOLDEN, "grid_spc.npz"))
    zo = np.load(os.path.join(GOLDEN, "sfm_octree.npz"))
    dense = torch.from_numpy(z["dense"]).bool()
    bits = dense.reshape(-1, 32).to(torch.int64)
    occ = (bits << torch.arange(32).view(1, 32)).sum(1)
    occ = torch.where(occ >= 2 ** 31, occ - 2 ** 32, occ).to(torch.int32)
    od = {"occ": occ, "level": int(z["level"]), "scale": float(zo["scale"]), "scene_origin": torch.from_numpy(zo["scene_origin"])}
    for eval_level in (int(z["level"]), int(z["level"]) + 1, int(z["eval_level"])):
        sd = mesh.gen_grid_spc(od, eval_level)
        assert set(sd) == {"sparse_vol", "voxel_size", "dim", "vol_origin", "bricks", "up"}
        up, bricks = sd["up"], sd["bricks"]
        assert up == 2 ** (eval_level - int(z["level"])) and sd["dim"] == dense.shape[0] * up
        assert torch.equal(bricks, torch.nonzero(dense)) and bricks.dtype == torch.int64
        K = sd["sparse_vol"].shape[0]
        assert K == bricks.shape[0] * up ** 3
        ind = np.round((sd["sparse_vol"].float().double().numpy() - sd["vol_origin"]) / float(sd["voxel_size"])).astype(np.int64)
        assert np.array_equal(ind // up, np.repeat(bricks.numpy(), up ** 3, axis=0))
        local = ind % up
        r = np.arange(K) % up ** 3
        assert np.array_equal(local, np.stack([r // (up * up), (r // up) % up, r % up], 1))
        mesh._check_bricks(bricks, up, torch.zeros(1).expand(K), sd["dim"] // up)  # the order isosurface_sparse asks for
