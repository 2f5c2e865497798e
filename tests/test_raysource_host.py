"""CPU side of the ray source (neuralrecon_w_amd.raysource, scripts/train.py --ray_source): the driver's options, the rank-share
rule, the 8-byte record against a numpy restatement of NcwSourceRec, the refusal of a non-GPU device, and nbytes()."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests._util import ROOT


def _train_module():
    spec = importlib.util.spec_from_file_location("ncw_train_script", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parser_defaults():
    ap = _train_module().build_parser()
    a = ap.parse_args(["--cfg_path", "x.yaml"])
    assert a.ray_source == "cache"
    assert a.semantic_map_path is None and a.sfm_path is None and a.depth_percent is None and a.source_seed == 0
    a = ap.parse_args(["--cfg_path", "x.yaml", "--ray_source", "scene", "--semantic_map_path", "sm", "--sfm_path", "sparse",
                       "--depth_percent", "0.2", "--source_seed", "5"])
    assert (a.ray_source, a.semantic_map_path, a.sfm_path, a.depth_percent, a.source_seed) == ("scene", "sm", "sparse", 0.2, 5)
    with pytest.raises(SystemExit):
        ap.parse_args(["--cfg_path", "x.yaml", "--ray_source", "files"])


@pytest.mark.parametrize("n,world", [(0, 1), (10, 1), (12, 3), (13, 3), (14, 3), (2, 4), (759, 2), (1000, 7)])
def test_rank_share(n, world):
    from neuralrecon_w_amd import raysource

    shares = []
    for rank in range(world):
        first, step, count = raysource.rank_share(n, world, rank)
        mine = list(range(n))[first::step]
        assert len(mine) == count and all(g % world == rank for g in mine)
        shares.append(mine)
    assert sorted(g for s in shares for g in s) == list(range(n))  # disjoint, and the union is everything
    assert max(map(len, shares)) - min(map(len, shares)) <= 1
    with pytest.raises(ValueError):
        raysource.rank_share(n, world, world)
    with pytest.raises(ValueError):
        raysource.rank_share(n, 0, 0)


def test_record_layout_against_numpy_and_the_c_struct():
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import raysource

    assert C.sizeof(L.NcwSourceRec) == 8 and C.sizeof(L.NcwSourceImage) == C.sizeof(L.NcwViewCamera) + 8
    rs = np.random.RandomState(0)
    n = 500
    pix = rs.randint(0, 2 ** 31 - 1, n).astype(np.int64)
    pix[:3] = [0, 2 ** 31 - 2, 1]  # the ends of the range
    rgb = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    rgb[0], rgb[1] = 255, 0
    lab = rs.randint(0, 256, n).astype(np.int64)
    lab[:2] = [255, 0]
    kp = rs.rand(n) < 0.5
    kp[:2] = [True, False]
    words = raysource.pack_records(torch.from_numpy(pix), torch.from_numpy(rgb), torch.from_numpy(lab), torch.from_numpy(kp))
    assert words.dtype == torch.int32 and tuple(words.shape) == (n, 2)
    # numpy restatement: the struct {uint32 pix; uint8 r, g, b, label;} in memory
    want = np.zeros(n, dtype=np.dtype([("pix", "<u4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("label", "u1")]))
    want["pix"] = pix.astype(np.uint32) | (kp.astype(np.uint32) << np.uint32(31))
    want["r"], want["g"], want["b"], want["label"] = rgb[:, 0], rgb[:, 1], rgb[:, 2], lab
    assert words.numpy().tobytes() == want.tobytes()
    rec = L.NcwSourceRec.from_buffer_copy(words.numpy().tobytes()[:8])
    assert rec.pix == (1 << 31) and (rec.r, rec.g, rec.b, rec.label) == (255, 255, 255, 255)  # bit 31 alone: pixel 0 with a key-point
    p2, rgb2, lab2, kp2 = raysource.unpack_records(words)
    assert np.array_equal(p2.numpy(), pix) and np.array_equal(rgb2.numpy(), rgb) and np.array_equal(lab2.numpy(), lab)
    assert np.array_equal(kp2.numpy(), kp)
    # no label maps: the byte is 0
    w0 = raysource.pack_records(torch.from_numpy(pix), torch.from_numpy(rgb), None, torch.from_numpy(kp))
    assert not bool(raysource.unpack_records(w0)[2].any())
    # 31 bits: 2^31 - 1 and anything negative are refused
    for bad in (2 ** 31 - 1, 2 ** 31, -1):
        with pytest.raises(ValueError):
            raysource.pack_records(torch.tensor([bad]), torch.zeros(1, 3, dtype=torch.uint8), None, torch.tensor([False]))
    with pytest.raises(ValueError):
        raysource.pack_records(torch.tensor([1]), torch.zeros(1, 3, dtype=torch.uint8), torch.tensor([256]), torch.tensor([False]))
    e = raysource.pack_records(torch.zeros(0, dtype=torch.int64), torch.zeros(0, 3, dtype=torch.uint8), None, torch.zeros(0, dtype=torch.bool))
    assert tuple(e.shape) == (0, 2)


def test_depth_padding_draws_what_pad_depth_percent_draws():
    """The same indices in the same order, and the generator left where `pad_depth_percent` leaves it."""
    from neuralrecon_w_amd import cachebuild, raysource

    rs = np.random.RandomState(1)
    rays = torch.from_numpy(rs.rand(40, 13).astype(np.float32))
    rays[:, 10] = torch.from_numpy((rs.rand(40) < 0.2) * rs.rand(40)).float()
    rays[:, 0] = torch.arange(40).float()  # the row's number
    rgbs = torch.zeros(40, 3)
    for dp in (0.1, 0.4, 0.7):
        g1, g2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
        out, _ = cachebuild.pad_depth_percent(rays, rgbs, dp, g1)
        extra = raysource.depth_padding(rays[:, 10], dp, g2)
        assert torch.equal(g1.get_state(), g2.get_state())
        got = torch.cat([rays[:, 0], rays[extra][:, 0]]).sort().values
        assert torch.equal(out[:, 0].sort().values, got) and (len(extra) > 0) == (dp > 0.3)


def test_cpu_device_is_refused():
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import raysource

    with pytest.raises(L.NeuconwHipError):
        raysource.RaySource.from_images([], device="cpu")
    with pytest.raises(L.NeuconwHipError):
        raysource.RaySource.from_scene(os.path.join(ROOT, "tests", "golden", "cache_scene"), device="cpu")
    src = _host_source(5, 2)
    with pytest.raises(L.NeuconwHipError):
        src.batch(None)


def _host_source(n, n_kp):
    from neuralrecon_w_amd import raysource, views

    cams = [views.Camera(np.eye(3), np.eye(4)[:3], 4, 3, 0.1, 2.0)] * 2
    return raysource.RaySource(torch.zeros(n, 2, dtype=torch.int32), raysource.image_table(cams, [3, 9]),
                               torch.tensor([0, 2, n]), torch.tensor([0, 0, n_kp]), torch.zeros(n_kp, dtype=torch.int32),
                               torch.zeros(n_kp), torch.zeros(n_kp), None, 0.0, True, ["person"])


def test_nbytes_is_computed_from_shapes_and_the_surface_matches_raycache():
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import raycache, raysource
    from neuralrecon_w_amd.labels import label_id

    src = _host_source(7, 3)
    assert len(src) == 7 and src.n_img == 2
    assert src.nbytes() == 7 * 8 + 2 * C.sizeof(L.NcwSourceImage) + 2 * 3 * 8 + 3 * 12
    assert src.mask_ids == [label_id("person")] and src.prefiltered is False
    tab = (L.NcwSourceImage * 2).from_buffer_copy(src.images.numpy().tobytes())
    assert (tab[0].ts, tab[1].ts) == (3, 9) and tab[1].cam.width == 4 and tab[1].cam.far == 2.0
    for name in ("__len__", "batch", "filtered", "epoch"):
        assert callable(getattr(raysource.RaySource, name)) and callable(getattr(raycache.RayCache, name))
    with pytest.raises(NotImplementedError):
        raysource.RaySource(src.recs, src.images, src.row_start, src.kp_start, src.kp_pix, src.kp_depth, src.kp_weight, None, 0.0,
                            True, ["person", "car", "sky", "tree", "bus"])
