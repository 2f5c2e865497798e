"""Host side of the surface scoring of evalmesh (no GPU): the Philox4x32-10 restatement the GPU tests compare the kernel
with reproduces the published known-answer vectors; the module's jet table is matplotlib's; bbx_crop / sfm_crop on CPU torch
tensors select exactly the rows the numpy path selects; sample_surface validates its faces on the host and has no CPU
fallback; the command line parses the new flags; the binding declares the new entry points."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import _surf_ref as R
from tests._util import ROOT

from neuralrecon_w_amd import evalmesh, lib as L


@pytest.mark.parametrize("counter, key, out", [
    ([0, 0, 0, 0], (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xffffffff] * 4, (0xffffffff, 0xffffffff), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_restatement_reproduces_the_known_answers(counter, key, out):
    got = R.philox4x32_10(np.array([counter, counter]), key)
    assert [" ".join("%08x" % v for v in row) for row in got] == [out, out]


def test_stream_restatement_scales_the_words_exactly():
    i = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1], dtype=np.uint64)
    u, r1, r2, xi = R.stream(i, 0x1234567890abcdef)
    w = R.philox4x32_10(np.stack([i & np.uint64(0xffffffff), i >> np.uint64(32), 0 * i, 0 * i], -1), (0x90abcdef, 0x12345678))
    assert [int(v * 2 ** 53) for v in xi] == [((int(a) << 32) | int(b)) >> 11 for a, b in w[:, :2]]
    assert [int(v * 2 ** 33) for v in r1] == [2 * int(a) + 1 for a in w[:, 2]] and np.array_equal(u, xi)
    assert [int(v * 2 ** 33) for v in r2] == [2 * int(a) + 1 for a in w[:, 3]]
    assert (xi >= 0).all() and (xi < 1).all() and (r1 > 0).all() and (r1 < 1).all()
    assert len({tuple(r) for r in w}) == 5  # the carry into the second counter word gives new blocks


def test_jet_table_is_matplotlibs():
    plt = pytest.importorskip("matplotlib.pyplot")
    lut = plt.get_cmap("jet")(np.arange(256) / 255.0)[:, :3]
    assert evalmesh.JET.shape == (256, 3) and evalmesh.JET_U8.dtype == np.uint8
    want = np.round(255.0 * lut).astype(np.uint8)
    for j in range(256):
        assert tuple(evalmesh.JET_U8[j]) == tuple(want[j]), j
    assert np.abs(evalmesh.JET - lut).max() <= 1e-12


def test_error_colours_index_rule():
    t = 0.03
    d = np.array([0.0, 3 * t, 10.0, 3 * t * 0.5, 3 * t * (255.0 / 256), np.nextafter(3 * t * (255.0 / 256), 0)])
    got = evalmesh.error_colours(d, t).numpy()
    v = np.minimum(d, 3 * t) / (3 * t)
    idx = np.minimum((v * 256).astype(np.int64), 255)
    assert list(idx[:4]) == [0, 255, 255, 128]  # v = 1.0 -> entry 255
    assert got.dtype == np.uint8 and np.array_equal(got, evalmesh.JET_U8[idx])
    got32 = evalmesh.error_colours(torch.from_numpy(d.astype(np.float32)), t).numpy()  # f32 distances are widened first
    v32 = np.minimum(d.astype(np.float32).astype(np.float64), 3 * t) / (3 * t)
    assert np.array_equal(got32, evalmesh.JET_U8[np.minimum((v32 * 256).astype(np.int64), 255)])


def _cloud():
    rng = np.random.RandomState(0)
    p = rng.uniform(-1.5, 1.5, (5000, 3)) + np.array([10.0, -20.0, 5.0])
    box = [[9.0, -21.0, 4.25], [11.0, -19.5, 5.5]]
    # points exactly on the faces of the box (strictly-inside rule: dropped), and one ulp inside (kept)
    p[0] = [9.0, -20.0, 5.0]
    p[1] = [10.0, -19.5, 5.0]
    p[2] = [10.0, -20.0, 5.5]
    p[3] = [np.nextafter(9.0, 10), -20.0, 5.0]
    p[4] = [11.0, -21.0, 4.25]
    return p, box


def test_bbx_crop_on_tensors_selects_the_numpy_rows():
    p, box = _cloud()
    want = evalmesh.bbx_crop(p, box)
    assert isinstance(want, np.ndarray) and 500 < len(want) < 4500
    assert not any((want == p[i]).all(-1).any() for i in (0, 1, 2, 4)) and (want == p[3]).all(-1).any()
    got = evalmesh.bbx_crop(torch.from_numpy(p), box)
    assert torch.is_tensor(got) and got.dtype == torch.float64 and got.device.type == "cpu"
    assert np.array_equal(got.numpy(), want)
    got32 = evalmesh.bbx_crop(torch.from_numpy(p.astype(np.float32)), box)  # widened like np.asarray(..., float64)
    assert np.array_equal(got32.numpy(), evalmesh.bbx_crop(p.astype(np.float32), box))
    assert evalmesh.bbx_crop(torch.zeros(0, 3), box).shape == (0, 3)


def test_sfm_crop_on_tensors_selects_the_numpy_rows():
    p, box = _cloud()
    rng = np.random.RandomState(1)
    sfm = rng.uniform(-1.2, 1.2, (300, 3)) + np.array([10.0, -20.0, 5.0])
    sfm[0] = [10.0, -20.0, 50.0]   # a cell outside [0, res)^3: dropped
    sfm[1] = [8.0, -20.0, 5.0]     # outside the cube on the low side
    p[5] = [10.0, -20.0, 50.0]     # a point in that outside cell never survives
    voxel = 0.21
    want = evalmesh.sfm_crop(p, sfm, voxel, box)
    assert 100 < len(want) < 4900 and not (want == p[5]).all(-1).any()
    for s in (sfm, torch.from_numpy(sfm)):
        got = evalmesh.sfm_crop(torch.from_numpy(p), s, voxel, box)
        assert torch.is_tensor(got) and got.dtype == torch.float64 and np.array_equal(got.numpy(), want)
    assert evalmesh.sfm_crop(torch.from_numpy(p), sfm[:0], voxel, box).shape == (0, 3)
    assert evalmesh.sfm_crop(torch.from_numpy(p), sfm[:1], voxel, box).shape == (0, 3)  # only the outside cell
    assert evalmesh.sfm_crop(torch.from_numpy(p[:0]), sfm, voxel, box).shape == (0, 3)


def test_sample_surface_checks_faces_on_the_host_and_has_no_cpu_fallback():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    with pytest.raises(ValueError, match="integer"):
        evalmesh.sample_surface(v, np.array([[0.0, 1.0, 2.0]]), 4, device="cpu")
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        evalmesh.sample_surface(v, np.array([0, 1, 2]), 4, device="cpu")
    with pytest.raises(ValueError, match="mode"):
        evalmesh.sample_surface(v, np.array([[0, 1, 2]]), 4, mode="sobol", device="cpu")
    with pytest.raises(L.NeuconwHipError, match="no CPU fallback"):
        evalmesh.sample_surface(v, np.array([[0, 1, 2]]), 4, device="cpu")
    with pytest.raises(L.NeuconwHipError, match="no CPU fallback"):
        evalmesh.surface_weights(torch.from_numpy(v), torch.tensor([[0, 1, 2]], dtype=torch.int32))


def test_command_lines_parse_the_surface_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import eval_mesh as cli
        import eval_pipeline as pipe
    finally:
        sys.path.pop(0)
    base = ["--file_pred", "a.ply", "--file_trgt", "b.ply", "--scene_config_path", "c.yaml"]
    a = cli.get_opts(base + ["--mesh"])
    assert a.mesh and a.sample_surface is None and a.surface_seed == 0 and a.surface_mode == "stratified" and not a.error_clouds
    a = cli.get_opts(base + ["--sample_surface", "--surface_mode", "iid", "--surface_seed", "7", "--error_clouds"])
    assert a.sample_surface == 10 and a.surface_mode == "iid" and a.surface_seed == 7 and a.error_clouds and not a.mesh
    assert cli.get_opts(base + ["--sample_surface", "4"]).sample_surface == 4
    b = pipe.parse_args(["--scene_name", "brandenburg_gate", "--pred_dir", "x", "--sample_surface", "--error_clouds"])
    assert b.sample_surface == 10 and b.surface_seed == 0 and b.surface_mode == "stratified" and b.error_clouds


def test_binding_declares_the_surface_entry_points():
    assert {"ncw_surf_weights", "ncw_surf_pick", "ncw_surf_sample"} <= set(L.exported_symbols())
    assert L.ABI_VERSION >= 23
