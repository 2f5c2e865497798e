"""GPU: the ray source -- `ncw_source_batch` (csrc/ncw_source.hip), neuralrecon_w_amd.raysource.RaySource and
scripts/train.py --ray_source scene -- against what the cache path gives for the same rays: `cachebuild.build_cache` files read
back by `raycache.RayCache`, `cachebuild.build_image` rows, and the reference's own rows of tests/golden/cache_golden.npz.
Everything that has a cached counterpart is compared BIT FOR BIT: the kernel calls the device functions `ncw_cache_rows` calls."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests._util import ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "golden", "cache_scene")
DEV = "cuda:0"
KEYS = ("rays", "ts", "semantics", "rgbs", "keep")


@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(HERE, "golden", "cache_golden.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def octrees():
    from neuralrecon_w_amd import voxel

    with open(os.path.join(SCENE, "config.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    hit = voxel.octree_from_sfm(SCENE, cfg["min_track_length"], cfg["voxel_size"], DEV, sfm_path="sparse", expand=1, radius=1)
    rng = voxel.octree_from_sfm(SCENE, cfg["min_track_length"], cfg["voxel_size"], DEV, sfm_path="sparse", expand=2, radius=1.5)
    return hit, rng, float(cfg["voxel_size"])


@pytest.fixture(scope="module")
def cached(tmp_path_factory):
    """The fixture scene through the cache path, once: build_cache(split_to_chunks=3) of a copy, read back by RayCache."""
    from neuralrecon_w_amd import cachebuild, raycache

    root = str(tmp_path_factory.mktemp("src") / "cache_scene")
    shutil.copytree(SCENE, root)
    cachebuild.build_cache(root, "cache", 1, "semantic_maps", 3, "sparse", seed=3, device=DEV)
    names = ["split_%d" % i for i in range(3)]
    rc = raycache.RayCache(root, "cache", names, DEV, 1, with_semantics=True)
    return {"root": root, "names": names, "all": rc.batch(None)}


@pytest.fixture(scope="module")
def source():
    from neuralrecon_w_amd import raysource

    return raysource.RaySource.from_scene(SCENE, 1, "semantic_maps", "sparse", seed=3, device=DEV)


@pytest.fixture(scope="module")
def whole(source):
    return source.batch(None)


def _same(a, b, keys=KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def _camera(g, iid):
    from neuralrecon_w_amd import views

    t = "im%d_" % iid
    w, h = g[t + "wh"].tolist()
    return views.Camera(g[t + "K"], g[t + "c2w"], w, h, float(g[t + "near64"]), float(g[t + "far64"]))


def _item(g, iid, with_label=True, cam=None, image_id=None, kp=None):
    t = "im%d_" % iid
    kp = kp if kp is not None else (g[t + "kp_xyz"], g[t + "kp_err"], g[t + "kp_px"], float(g[t + "err_mean"]))
    return (cam or _camera(g, iid), g[t + "image"], iid if image_id is None else image_id, kp, g[t + "w2c"],
            g[t + "label"] if with_label else None)


def _away(g, iid=7):
    """The camera of test_one_pixel_image_and_camera_turned_away: every ray misses the octrees."""
    from neuralrecon_w_amd import views

    cam0 = _camera(g, iid)
    c2w = cam0.c2w.copy()
    c2w[:, 0] *= -1
    c2w[:, 2] *= -1
    return views.Camera(cam0.K, c2w, cam0.width, cam0.height, cam0.near, cam0.far)


def _as_batch(rows, rgbs):
    """Cache rows [m, 13 | 12] + rgbs -> the batch dictionary ncw_batch_assemble makes of them (torch's float -> int64)."""
    rows, rgbs = torch.as_tensor(rows).to(DEV), torch.as_tensor(rgbs).to(DEV)
    nc = rows.shape[1]
    out = {"rays": torch.cat([rows[:, :8], rows[:, nc - 3:]], 1), "ts": rows[:, 8].long(), "rgbs": rgbs}
    if nc == 13:
        out["semantics"] = rows[:, 9].long()
    return out


def _built(items, hit, rng, vs):
    """`build_image` per item, concatenated, as a batch."""
    from neuralrecon_w_amd import cachebuild

    parts = [cachebuild.build_image(*it, hit, rng, vs, device=DEV) for it in items]
    return _as_batch(torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0)), [int(p[0].shape[0]) for p in parts]


def _table(b):
    """A batch as one float64 row per ray (for multiset comparisons), sorted."""
    cols = [b["rays"].double(), b["ts"].double()[:, None], b["rgbs"].double()]
    if "semantics" in b:
        cols.append(b["semantics"].double()[:, None])
    t = torch.cat(cols, 1).cpu().numpy()
    return t[np.lexsort(t.T[::-1])]


# ---------------------------------------------------------------------------------------------------
# 1. / 2. / 12. the whole fixture against the cache path; splits, clamps, shape edges; reproducibility
# ---------------------------------------------------------------------------------------------------
def test_whole_source_equals_the_cache_bit_for_bit(cached, source, whole):
    assert len(source) == 759 and source.prefiltered is False and source.n_img == 3
    _same(whole, cached["all"])
    assert whole["rays"].shape == (759, 11) and whole["keep"].dtype == torch.bool and bool(whole["keep"].all())
    assert 11 not in whole["ts"].tolist() and sorted(set(whole["ts"].tolist())) == [3, 5, 7]  # the test image is absent
    assert int((whole["rays"][:, 8] != 0).sum()) > 20  # key-point rows are there
    assert source.nbytes() < 16 * len(source)  # 8 B records + tables + key-points, against 64 B of dense rows


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_split_independence_and_shape_edges(source, whole, B):
    idx = torch.from_numpy(np.random.RandomState(B).randint(0, 759, B)).to(DEV)
    if B > 2:
        idx[1] = idx[0]  # a repeat for certain
        idx[-1] = 758
    b = source.batch(idx)
    _same(b, {k: v[idx] for k, v in whole.items()})


def test_indices_clamp_and_empty_batch(source, whole, cached):
    from neuralrecon_w_amd import raycache

    idx = torch.tensor([-5, -1, 0, 758, 759, 900, 2 ** 40, -2 ** 40], device=DEV)
    b = source.batch(idx)
    _same(b, {k: v[idx.clamp(0, 758)] for k, v in whole.items()})
    rc = raycache.RayCache(cached["root"], "cache", cached["names"], DEV, 1, with_semantics=True)
    _same(b, rc.batch(idx))  # ncw_batch_assemble's clamp
    e = source.batch(torch.zeros(0, dtype=torch.int64, device=DEV))
    assert e["rays"].shape == (0, 11) and e["ts"].shape == (0,) and e["rgbs"].shape == (0, 3) and e["keep"].shape == (0,)
    assert e["semantics"].shape == (0,)


def test_reproducible(source):
    idx = torch.from_numpy(np.random.RandomState(9).randint(0, 759, 700)).to(DEV)
    _same(source.batch(idx), source.batch(idx))


# ---------------------------------------------------------------------------------------------------
# 3. images without a kept pixel, a 1-pixel image, the last pixel of an image
# ---------------------------------------------------------------------------------------------------
def test_empty_images_first_middle_last(g, octrees):
    from neuralrecon_w_amd import raysource, views

    hit, rng, vs = octrees
    cam0 = _camera(g, 7)
    one = views.Camera(np.array([[1.0, 0, 0.5], [0, 1.0, 0.5], [0, 0, 1]]), cam0.c2w, 1, 1, cam0.near, cam0.far)
    kp1 = (np.array([[0.1, -0.1, 0.2]], np.float32), np.array([0.7], np.float32), np.array([[0, 0]], np.int32), 0.7)
    one_item = (one, np.array([[[255, 0, 128]]], dtype=np.uint8), 9, kp1, g["im7_w2c"], np.array([[3]], np.uint8))
    items = [_item(g, 7, cam=_away(g), image_id=21), _item(g, 7), _item(g, 7, cam=_away(g), image_id=22),
             _item(g, 7, cam=_away(g), image_id=24), _item(g, 3), one_item, _item(g, 5), _item(g, 7, cam=_away(g), image_id=23)]
    want, counts = _built(items, hit, rng, vs)
    assert counts[0] == counts[2] == counts[3] == counts[7] == 0 and min(counts[1], counts[4], counts[6]) > 50
    src = raysource.RaySource.from_images(items, hit, rng, vs, device=DEV)
    assert src.row_start.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist() and src.n_img == 8
    b = src.batch(None)
    _same(b, want, ("rays", "ts", "semantics", "rgbs"))
    assert not {21, 22, 23, 24} & set(b["ts"].tolist())
    idx = torch.from_numpy(np.random.RandomState(2).randint(0, len(src), 300)).to(DEV)
    _same(src.batch(idx), {k: v[idx] for k, v in b.items()})
    # without octrees every pixel is a row: the 1-pixel image gives one, and each image's last pixel (p = w h - 1) is there
    items = [one_item, _item(g, 3), one_item[:2] + (10,) + one_item[3:], _item(g, 5)]
    want, counts = _built(items, None, None, 0.0)
    assert counts == [1, 36 * 30, 1, 30 * 30]
    src = raysource.RaySource.from_images(items, None, None, 0.0, device=DEV)
    b = src.batch(None)
    _same(b, want, ("rays", "ts", "semantics", "rgbs"))
    last = raysource.unpack_records(src.recs.cpu())[0][[0, 1080, 1081, 1981]].tolist()
    assert last == [0, 36 * 30 - 1, 0, 30 * 30 - 1] and b["ts"][[0, 1080, 1081, 1981]].tolist() == [9, 3, 10, 5]
    assert b["rgbs"][1080].tolist() == (torch.from_numpy(g["im3_image"].reshape(-1, 3)[-1].astype(np.float32)) / 255.0).tolist()


# ---------------------------------------------------------------------------------------------------
# 4. key-points
# ---------------------------------------------------------------------------------------------------
def test_key_points_segment_bounds(g, octrees):
    from neuralrecon_w_amd import cachebuild, raysource

    hit, rng, vs = octrees
    cam = _camera(g, 3)
    w = cam.width
    dz, wt = cachebuild.sfm_depth_planes(None, None, np.zeros((0, 2), np.int32), float("nan"), g["im3_w2c"], w, cam.height, DEV)
    keep = cachebuild.cache_rows(cam, torch.from_numpy(g["im3_image"]).to(DEV), 3, dz, wt, None, hit, rng, vs)[2].cpu().numpy() > 0
    kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
    p_first, p_last, q, q2, p_drop = int(kept[0]), int(kept[-1]), int(kept[len(kept) // 2]), int(kept[len(kept) // 3]), int(dropped[0])

    def kps(pixels, seed):
        rs = np.random.RandomState(seed)
        m = len(pixels)
        px = np.array([[p % w, p // w] for p in pixels], np.int32).reshape(m, 2)
        return (rs.uniform(-1, 1, (m, 3)).astype(np.float32), rs.uniform(0.3, 1.5, m).astype(np.float32), px, 0.9)

    items = [_item(g, 3, image_id=30, kp=kps([q, p_last, p_drop, p_first], 1)),  # first + last kept pixel, a dropped one
             _item(g, 3, image_id=31, kp=kps([q2], 2)),                          # the same pixels, a key-point on another one only
             _item(g, 3, image_id=32, kp=kps([], 3)),                             # none
             _item(g, 3, image_id=33, kp=kps([q], 4))]
    want, counts = _built(items, hit, rng, vs)
    m = counts[0]
    assert counts == [m] * 4
    src = raysource.RaySource.from_images(items, hit, rng, vs, device=DEV)
    assert src.kp_start.tolist() == [0, 3, 4, 4, 5]  # the key-point on the dropped pixel has no entry
    b = src.batch(None)
    _same(b, want, ("rays", "ts", "semantics", "rgbs"))  # depth and weight: cache_rows' columns bit for bit
    has = ((b["rays"][:, 8] != 0) | (b["rays"][:, 9] != 0)).cpu().numpy()
    pos = {p: i for i, p in enumerate(kept.tolist())}
    expect = np.zeros(4 * m, bool)
    expect[[pos[p_first], pos[p_last], pos[q], m + pos[q2], 3 * m + pos[q]]] = True
    assert np.array_equal(has, expect) and pos[p_first] == 0 and pos[p_last] == m - 1
    assert bool((b["rays"][:, 9][torch.from_numpy(expect).to(DEV)] > 0).all())  # weights of real key-points
    idx = torch.tensor([0, m - 1, m, 2 * m - 1, m + pos[q], pos[q], 3 * m + pos[q], 2 * m + pos[q]], device=DEV)
    _same(src.batch(idx), {k: v[idx] for k, v in b.items()})


# ---------------------------------------------------------------------------------------------------
# 5. / 6. no label maps; no octrees against the reference's rows
# ---------------------------------------------------------------------------------------------------
def test_no_label_maps(g, octrees):
    from neuralrecon_w_amd import raysource

    hit, rng, vs = octrees
    items = [_item(g, i, with_label=False) for i in (7, 3, 5)]
    want, counts = _built(items, hit, rng, vs)
    assert "semantics" not in want and sum(counts) == 759
    src = raysource.RaySource.from_images(items, hit, rng, vs, ray_mask_list=["wall", "sky"], prefilter=True, device=DEV)
    b = src.batch(None)
    assert "semantics" not in b and bool(b["keep"].all()) and len(src) == 759 and src.prefiltered is False
    _same(b, want, ("rays", "ts", "rgbs"))
    with pytest.raises(ValueError):
        raysource.RaySource.from_images([_item(g, 7), _item(g, 3, with_label=False)], hit, rng, vs, device=DEV)


def test_use_voxel_false_vs_reference_rows(g):
    """Every pixel is a row with the camera's near / far; the bounds are test_non_voxel_columns_vs_reference's."""
    from neuralrecon_w_amd import raysource

    src = raysource.RaySource.from_scene(SCENE, 1, "semantic_maps", "sparse", use_voxel=False, device=DEV)
    b = {k: v.cpu().numpy() for k, v in src.batch(None).items()}
    at = 0
    for iid in g["train_ids"].tolist():
        t = "im%d_" % iid
        ref = g[t + "rows13"]
        n = ref.shape[0]
        rays, ts, lab, rgbs = b["rays"][at:at + n], b["ts"][at:at + n], b["semantics"][at:at + n], b["rgbs"][at:at + n]
        at += n
        assert np.array_equal(rays[:, 0:3], ref[:, 0:3]) and np.array_equal(rgbs, g[t + "rgbs"])
        assert np.array_equal(rays[:, 6:8], ref[:, 6:8]) and np.array_equal(ts, np.full(n, iid, np.int64))
        assert np.array_equal(lab, ref[:, 9].astype(np.int64)) and len(np.unique(lab)) > 2
        assert np.abs(rays[:, 3:6] - ref[:, 3:6]).max() <= 1e-6
        assert np.array_equal(rays[:, 10], np.zeros(n, np.float32))
        d, w, rd, rw = rays[:, 8].astype(np.float64), rays[:, 9].astype(np.float64), ref[:, 10].astype(np.float64), ref[:, 11].astype(np.float64)
        d64, w64 = g[t + "depth64"], g[t + "weight64"]
        assert np.array_equal(w != 0, w64 != 0) and np.array_equal(w != 0, rw != 0) and int((w != 0).sum()) > 20
        assert np.array_equal(d != 0, d64 != 0) and (d64 < 0).any()
        assert np.abs(d - d64).max() <= 2 * np.abs(rd - d64).max() and np.abs(w - w64).max() <= 2 * np.abs(rw - w64).max()
    assert at == len(src) == 42 * 27 + 36 * 30 + 30 * 30 and src.range_octree is None


# ---------------------------------------------------------------------------------------------------
# 7. / 8. / 9. / 10. depth padding, prefilter, downscale, ranks
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dp", [0.2, 0.4])
def test_depth_percent_multiset_equals_build_cache(tmp_path, dp):
    from neuralrecon_w_amd import cachebuild, raysource

    root = str(tmp_path / "cache_scene")
    shutil.copytree(SCENE, root)
    files = cachebuild.build_cache(root, "c", 1, "semantic_maps", -1, "sparse", seed=1, device=DEV, depth_percent=dp)
    want = _as_batch(np.load(files[0])["arr_0"], np.load(files[1])["arr_0"])
    src = raysource.RaySource.from_scene(SCENE, 1, "semantic_maps", "sparse", seed=1, depth_percent=dp, device=DEV)
    b = src.batch(None)
    assert len(src) == want["rays"].shape[0] and (len(src) > 759) == (dp > 0.3)
    assert np.array_equal(_table(b), _table(want))
    for iid in (7, 3, 5):
        sel = b["ts"] == iid
        share = float((b["rays"][sel][:, 8] > 0).double().mean())
        print("depth_percent %.1f image %d: %d rows, share with a key-point depth %.4f" % (dp, iid, int(sel.sum()), share))
        assert share >= dp - 1e-12
    rs = src.row_start.tolist()  # copies stay inside their image's range
    assert all(bool((b["ts"][rs[k]:rs[k + 1]] == iid).all()) for k, iid in enumerate((7, 3, 5)))


def test_prefilter_equals_raycache_prefilter(cached, source):
    from neuralrecon_w_amd import raycache, raysource

    mask = ["sky", "tree"]  # labels 2 and 4 of the fixture's maps
    rc = raycache.RayCache(cached["root"], "cache", cached["names"], DEV, 1, with_semantics=True, ray_mask_list=mask, prefilter=True)
    src = raysource.RaySource.from_scene(SCENE, 1, "semantic_maps", "sparse", seed=3, ray_mask_list=mask, prefilter=True, device=DEV)
    assert src.prefiltered and rc.prefiltered and src.mask_ids == rc.mask_ids == [2, 4]
    assert 0 < len(src) == len(rc) < 759
    b = src.batch(None)
    _same(b, rc.batch(None))
    assert bool(b["keep"].all()) and not {2, 4} & set(b["semantics"].tolist())
    gen = torch.Generator(device=DEV).manual_seed(5)
    sizes = [x["rays"].shape[0] for x in src.epoch(16, generator=gen, drop_last=True)]
    assert sizes == [16] * (len(src) // 16)
    # without prefilter the batch carries the flags instead, as RayCache's does
    flagged = raysource.RaySource.from_scene(SCENE, 1, "semantic_maps", "sparse", seed=3, ray_mask_list=mask, device=DEV).batch(None)
    rc2 = raycache.RayCache(cached["root"], "cache", cached["names"], DEV, 1, with_semantics=True, ray_mask_list=mask)
    _same(flagged, rc2.batch(None))
    assert int(flagged["keep"].sum()) == len(src) and len(flagged["keep"]) == 759
    _same(dict(zip(("rays", "ts", "semantics", "rgbs"), raysource.RaySource.filtered(flagged))), b, ("rays", "ts", "semantics", "rgbs"))
    # the shared epoch loop draws one permutation from the generator, as RayCache.epoch does
    g1, g2 = torch.Generator(device=DEV).manual_seed(8), torch.Generator(device=DEV).manual_seed(8)
    for x, y in zip(src.epoch(100, generator=g1, max_batches=3, skip_batches=1), rc.epoch(100, generator=g2, max_batches=3, skip_batches=1)):
        _same(x, y)
    assert torch.equal(g1.get_state(), g2.get_state())


def test_downscale_2_equals_build_cache(tmp_path):
    from neuralrecon_w_amd import cachebuild, raysource

    root = str(tmp_path / "cache_scene")
    shutil.copytree(SCENE, root)
    files = cachebuild.build_cache(root, "c2", 2, "semantic_maps", -1, "sparse", seed=0, device=DEV)
    want = _as_batch(np.load(files[0])["arr_0"], np.load(files[1])["arr_0"])
    src = raysource.RaySource.from_scene(SCENE, 2, "semantic_maps", "sparse", device=DEV)
    assert 20 < len(src) < 759
    _same(src.batch(None), want, ("rays", "ts", "semantics", "rgbs"))


def test_two_ranks_share_the_records():
    from neuralrecon_w_amd import raysource

    kw = dict(seed=2, depth_percent=0.4, ray_mask_list=["sky"], prefilter=True, device=DEV)
    one = raysource.RaySource.from_scene(SCENE, 1, "semantic_maps", "sparse", **kw)
    ranks = [raysource.RaySource.from_scene(SCENE, 1, "semantic_maps", "sparse", world_size=2, rank=r, **kw) for r in (0, 1)]
    all_b = one.batch(None)
    n = len(one)
    assert len(ranks[0]) + len(ranks[1]) == n and abs(len(ranks[0]) - len(ranks[1])) <= 1
    assert [len(r) for r in ranks] == [raysource.rank_share(n, 2, r)[2] for r in (0, 1)]
    for r in (0, 1):  # global record g (numbered after padding and prefilter) goes to rank g % 2
        _same(ranks[r].batch(None), {k: v[r::2] for k, v in all_b.items()})
    # disjoint as records (image, pixel), apart from the copies depth_percent makes
    plain = [raysource.RaySource.from_scene(SCENE, 1, "semantic_maps", "sparse", world_size=2, rank=r, device=DEV) for r in (0, 1)]
    keys = []
    for s in plain:
        pix = raysource.unpack_records(s.recs.cpu())[0]
        img = torch.searchsorted(s.row_start.cpu(), torch.arange(len(s)), right=True) - 1
        keys.append(set(zip(img.tolist(), pix.tolist())))
    assert len(keys[0]) == 380 and len(keys[1]) == 379 and not keys[0] & keys[1]


# ---------------------------------------------------------------------------------------------------
# 11. the entry point's argument checks
# ---------------------------------------------------------------------------------------------------
def test_entry_point_argument_checks(source, octrees):
    from neuralrecon_w_amd import cachebuild
    from neuralrecon_w_amd import lib as L

    lib, P, s = L.get_lib(), L.ptr, L.stream_ptr(torch.device(DEV))
    src, B = source, 300
    rays = torch.zeros(B * 11 + 4, device=DEV)
    rgbs = torch.zeros(B * 3 + 4, device=DEV)
    ts, lab = torch.zeros(B + 1, dtype=torch.int64, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    keep = torch.zeros(B, dtype=torch.uint8, device=DEV)
    idx = torch.arange(B + 1, device=DEV)
    ids = (C.c_int * 5)(2, 4, 0, 0, 0)
    tree = cachebuild._octree_struct(octrees[1])
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)  # noqa: E731

    def call(**k):
        return lib.ncw_source_batch(k.get("recs", P(src.recs)), k.get("n_rows", len(src)), k.get("images", P(src.images)),
                                    k.get("row_start", P(src.row_start)), P(src.kp_start), k.get("n_img", src.n_img),
                                    k.get("kp_pix", P(src.kp_pix)), P(src.kp_depth), P(src.kp_weight), C.byref(k.get("tree", tree)),
                                    0.1, k.get("idx", P(idx)), k.get("B", B), 1, k.get("rays", P(rays)), k.get("ts", P(ts)), P(lab),
                                    k.get("rgbs", P(rgbs)), ids, k.get("n_ids", 2), P(keep), s)

    assert call() == 0
    assert call(B=0, rays=None, recs=None) == 0 and call(B=-3) == 0  # no launch, whatever the pointers
    assert call(recs=None) == -1 and call(images=None) == -1 and call(row_start=None) == -1 and call(rays=None) == -1
    assert call(ts=None) == -1 and call(kp_pix=None) == -1  # depth / weight without pixels
    assert call(rays=off(rays, 4)) == -1 and call(rgbs=off(rgbs, 4)) == -1  # 16-byte row stores
    assert call(recs=off(src.recs, 4)) == -1 and call(idx=off(idx, 4)) == -1 and call(ts=off(ts, 4)) == -1
    assert call(n_ids=5) == -1 and call(n_ids=-1) == -1 and call(n_rows=0) == -1 and call(n_img=0) == -1
    for level in (2, 11):
        bad = L.NcwCacheOctree(tree.origin, tree.scale, level, 0, tree.occ, tree.brick)
        assert call(tree=bad) == -1
    assert call(tree=L.NcwCacheOctree(tree.origin, tree.scale, tree.level, 0, None, tree.brick)) == -1
    assert call(idx=None, rgbs=None) == 0  # the identity; rgbs are optional as in ncw_batch_assemble
    torch.cuda.synchronize()
    assert torch.equal(rays[:B * 11].reshape(B, 11), src.batch(torch.arange(B, device=DEV))["rays"])


# ---------------------------------------------------------------------------------------------------
# 13. the driver
# ---------------------------------------------------------------------------------------------------
def test_train_driver_from_a_scene_directory(tmp_path):
    """scripts/train.py --ray_source scene on a scene directory with no cache: 5 steps, a checkpoint, a resume to step 7; the
    checkpoint is refused under --ray_source cache."""
    from PIL import Image

    root = str(tmp_path / "scene")
    shutil.copytree(SCENE, root)
    rs = np.random.RandomState(0)
    for name in sorted(os.listdir(os.path.join(root, "dense", "images"))):  # images the test writes, at the fixture's sizes
        p = os.path.join(root, "dense", "images", name)
        w, h = Image.open(p).size
        Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(p)
    exp = {"NEUCONW": {"N_SAMPLES": 8, "N_IMPORTANCE": 8, "UP_SAMPLE_STEP": 2, "N_OUTSIDE": 4, "NEAR_FAR_OVERRIDE": True,
                       "DEPTH_LOSS": True, "S_VAL_BASE": 3, "BOUNDARY_SAMPLES": 4, "SAMPLE_RANGE": 16, "SDF_THRESHOLD": 0.05,
                       "TRAIN_VOXEL_SIZE": 0.06, "UPDATE_FREQ": 0, "N_VOCAB": 64, "N_A": 16, "ANNEAL_END": 100,
                       "MESH_MASK_LIST": ["sky"], "RAY_MASK_LIST": ["tree"],
                       "SDF_CONFIG": {"d_out": 65, "d_hidden": 64, "skip_in": "(4,)"},
                       "COLOR_CONFIG": {"d_feature": 64, "d_hidden": 64, "head_channels": 32},
                       "S_CONFIG": {"init_val": 0.3}, "LOSS": {"igr_weight": 0.0001}},
           "DATASET": {"ROOT_DIR": root, "DATASET_NAME": "phototourism", "PHOTOTOURISM": {"CACHE_DIR": "cache"}},
           "TRAINER": {"CANONICAL_BS": 4096, "CANONICAL_LR": "1e-4", "LR_SCHEDULER": "none", "SAVE_DIR": os.path.join(root, "ckpts"),
                       "SAVE_FREQ": 4}}
    cfg = os.path.join(root, "train_scene.yaml")
    yaml.safe_dump(exp, open(cfg, "w"))
    base = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--cfg_path", cfg, "--batch_size", "64", "--num_epochs", "3",
            "--prec", "f32", "--log_every", "1", "--sfm_path", "sparse"]
    assert not os.path.exists(os.path.join(root, "cache"))
    r = subprocess.run(base + ["--ray_source", "scene", "--max_steps", "5", "--exp_name", "s"], capture_output=True, text=True,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("epoch")]
    assert len(lines) == 5 and all(np.isfinite([float(l.split("loss")[1].split()[0]) for l in lines]))
    assert "ray source: scene (3 images)" in r.stdout and "B/ray" in r.stdout
    n_res = int(r.stdout.split("images), ")[1].split(" rays")[0])
    assert 64 <= n_res < 759  # the black-listed label was removed at build time
    last = os.path.join(root, "ckpts", "s", "last.ckpt")
    ck = torch.load(last, map_location="cpu")
    assert ck["global_step"] == 5 and ck["ncw_resume"]["ray_source"] == "scene"
    r2 = subprocess.run(base + ["--ray_source", "scene", "--max_steps", "7", "--exp_name", "s2", "--ckpt_path", last],
                        capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-3000:]
    assert "step 5 " in r2.stdout and "step 6 " in r2.stdout and "step 4 " not in r2.stdout
    assert torch.load(os.path.join(root, "ckpts", "s2", "last.ckpt"), map_location="cpu")["global_step"] == 7
    # the other source holds another row set: refused, with the message, before anything is read or built
    r3 = subprocess.run(base + ["--max_steps", "7", "--exp_name", "s3", "--ckpt_path", last], capture_output=True, text=True,
                        cwd=ROOT, timeout=600)
    assert r3.returncode != 0 and "was written with --ray_source scene" in r3.stderr and "--ray_source cache" in r3.stderr
    assert not os.path.exists(os.path.join(root, "ckpts", "s3"))
