"""CPU side of the camera-view path (neuralrecon_w_amd.views): the float64 restatement tests/_view_ref.py against the golden
file recorded from the reference's own code (tests/golden/make_golden_view.py), `scene_view` on tests/golden/reproj_scene
against the reference dataset's recorded items, the JET table, the PNG writer, the command lines' arguments, and the refusal to
run without a GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import _view_ref as VR
from tests._util import GOLDEN, ROOT

SCENE = os.path.join(GOLDEN, "reproj_scene")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "view_golden.npz"))


def _script(name):
    spec = importlib.util.spec_from_file_location("_script_" + name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_reproduces_the_reference_rays(gold):
    """get_ray_directions + get_rays of the reference (float32) against the restatement: in float32 the same operations give
    the same directions bitwise and the same rays to an ulp; in float64 within float32 rounding (1e-6)."""
    W, H = [int(v) for v in gold["rays_wh"]]
    K, c2w = gold["rays_K"], gold["rays_c2w"]
    d32 = VR.ray_directions(H, W, K, torch.float32)
    assert torch.equal(d32, torch.from_numpy(gold["rays_directions"]))
    o32, r32 = VR.rays_of(d32, c2w, torch.float32)
    assert torch.equal(o32, torch.from_numpy(gold["rays_o"]))
    assert float((r32 - torch.from_numpy(gold["rays_d"])).abs().max()) <= 2.4e-7  # 2 ulp of a component <= 1
    rays = VR.view_rays(K, c2w, W, H, 0.5, 4.0)
    assert rays.shape == (W * H, 8) and rays.dtype == torch.float64
    assert float((rays[:, 3:6] - torch.from_numpy(gold["rays_d"]).double()).abs().max()) < 1e-6
    assert torch.equal(rays[:, :3].float(), torch.from_numpy(gold["rays_o"]))
    assert float(rays[:, 6].min()) == 0.5 and float(rays[:, 7].max()) == 4.0
    assert float((rays[:, 3:6].norm(dim=-1) - 1).abs().max()) < 1e-12


def test_restatement_reproduces_the_reference_psnr(gold):
    pred, gt, mask = [torch.from_numpy(gold[k]) for k in ("met_pred", "met_gt", "met_mask")]
    m3 = mask[:, None].expand(-1, 3)
    for got, key in ((VR.mse(pred, gt), "met_mse"), (VR.psnr(pred, gt), "met_psnr"), (VR.mse(pred, gt, m3), "met_mse_masked"),
                     (VR.psnr(pred, gt, m3), "met_psnr_masked")):
        assert abs(float(got) - float(gold[key])) <= 2e-6 * abs(float(gold[key])), key
    assert float(gold["met_psnr"]) != float(gold["met_psnr_masked"])


def test_ssim_oracle_properties():
    """The SSIM oracle itself, pinned to values worked out by hand: the sigma-1.5 window of size 3 is
    (e, 1, e) / (1 + 2 e) with e = exp(-1 / 4.5); two constant images a, b have mu = a, b and every variance 0, so the map is
    (2 a b + C1) / (a^2 + b^2 + C1) everywhere, whatever the window; a single bright pixel on black against black has
    mu_y = sigma_y = sigma_xy = 0, so the map is C1 C2 / ((mu_x^2 + C1)(sigma_x^2 + C2)) with mu_x = g_i g_j v and
    E[x^2] = g_i g_j v^2 at offset (i, j) from the pixel.  Then: 1 for identical images, symmetric."""
    e = float(np.exp(-1 / 4.5))
    assert np.allclose(VR.gaussian_window(3).numpy(), np.array([e, 1, e]) / (1 + 2 * e), rtol=0, atol=1e-15)
    assert np.allclose(VR.gaussian_window(3).numpy(), [0.30780133, 0.38439734, 0.30780133], rtol=0, atol=5e-9)
    a, b, C1, C2 = 0.5, 0.25, 1e-4, 9e-4
    for w in (3, 11):
        got = float(VR.ssim(torch.full((3, 12, 13), a), torch.full((3, 12, 13), b), w))
        assert abs(got - 0.2501 / 0.3126) < 1e-12 and abs(got - (2 * a * b + C1) / (a * a + b * b + C1)) < 1e-12
    x = torch.zeros(1, 7, 7, dtype=torch.float64)
    x[0, 3, 3] = v = 0.8
    g = np.array([e, 1, e]) / (1 + 2 * e)
    want = np.ones((7, 7))
    for i in range(3):
        for j in range(3):
            mu, ex2 = g[i] * g[j] * v, g[i] * g[j] * v * v
            want[2 + i, 2 + j] = C1 * C2 / ((mu * mu + C1) * (ex2 - mu * mu + C2))
    assert abs(float(VR.ssim(x, torch.zeros_like(x), 3)) - want.mean()) < 1e-12 and want.min() < 0.01
    g = torch.Generator().manual_seed(2)
    x, y = torch.rand(3, 9, 14, generator=g), torch.rand(3, 9, 14, generator=g)
    for w in (3, 11):
        if w == 11:
            x, y = torch.rand(3, 12, 17, generator=g), torch.rand(3, 12, 17, generator=g)
        assert abs(float(VR.ssim(x, x, w)) - 1) < 1e-12
        a, b = float(VR.ssim(x, y, w)), float(VR.ssim(y, x, w))
        assert abs(a - b) < 1e-12 and 0 <= a < 0.9
    assert abs(float(VR.gaussian_window(11).sum()) - 1) < 1e-12


@pytest.mark.parametrize("tag,kw", [("val", dict(split="val", img_downscale=1)), ("tt2", dict(split="test_train", img_downscale=2)),
                                    ("tt1o", dict(split="test_train", img_downscale=1, with_origin=True))])
def test_scene_view_matches_the_reference_dataset(gold, tag, kw):
    """`scene_view` against the items the reference's PhototourismDataset returned for the same scene: K rescale (with its
    int(2 cx) size), the "right up back" pose flip, near / far (SfM percentiles, or origin_z -+ 1.5 radius), the `val`
    downscale clamp, the default id (first training image of the tsv) and -- where PIL is present -- the decoded image."""
    from neuralrecon_w_amd import views

    kw = dict(kw)
    if kw.pop("with_origin", False):
        kw.update(scene_origin=gold["scene_origin"].tolist(), scene_radius=float(gold["scene_radius"]))
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    cam, gt, image_id = views.scene_view(SCENE, load_image=have_pil, **kw)
    assert image_id == int(gold[tag + "_id"]) == 2  # d.jpg: the first `train` row of split.tsv
    assert int(gold[tag + "_downscale"]) == (8 if tag == "val" else kw["img_downscale"])
    assert (cam.width, cam.height) == tuple(int(v) for v in gold[tag + "_wh"])
    assert cam.K.dtype == np.float32 and np.array_equal(cam.K, gold[tag + "_K"])
    assert cam.c2w.dtype == np.float32 and np.abs(cam.c2w - gold[tag + "_c2w"]).max() <= 1e-6
    assert abs(cam.near - float(gold[tag + "_near64"])) <= 1e-9 * abs(cam.near) + 1e-12
    assert abs(cam.far - float(gold[tag + "_far64"])) <= 1e-9 * abs(cam.far)
    assert cam.near < cam.far
    if have_pil:
        assert gt.shape == (3, cam.height, cam.width)
        assert torch.equal(gt.reshape(3, -1).T, torch.from_numpy(gold[tag + "_rgbs"]))
    # the dataset's rays of that item against the restatement fed with scene_view's camera (float64 vs the float32 reference)
    rays = VR.view_rays(cam.K, cam.c2w, cam.width, cam.height, cam.near, cam.far)
    ref = torch.from_numpy(gold[tag + "_rays"]).double()
    assert float((rays[:, :6] - ref[:, :6]).abs().max()) < 2e-6
    assert torch.equal(rays[:, 6:].float(), ref[:, 6:].float())
    # ... and the independent restatement of the dataset's steps from the raw COLMAP records
    from neuralrecon_w_amd import colmap

    sp = os.path.join(SCENE, "dense", "sparse")
    im = colmap.read_images(os.path.join(sp, "images.bin"))[image_id]
    camrec = colmap.read_cameras(os.path.join(sp, "cameras.bin"))[im["camera_id"]]
    _, xyz, _, _ = colmap.read_points3d(os.path.join(sp, "points3D.bin"))
    K, c2w, near, far = VR.scene_item(camrec["params"], im["qvec"], im["tvec"], xyz, int(gold[tag + "_downscale"]),
                                      kw.get("scene_origin"), kw.get("scene_radius"))
    assert np.array_equal(K, cam.K) and np.abs(c2w - cam.c2w).max() <= 1e-6
    assert abs(near - cam.near) <= 1e-12 + 1e-9 * abs(near) and abs(far - cam.far) <= 1e-9 * abs(far)


def test_scene_view_selects_by_name_and_refuses_unknown_images():
    from neuralrecon_w_amd import views

    cam, gt, image_id = views.scene_view(SCENE, image_name="b.jpg", split="test_train", load_image=False)
    assert image_id == 1 and gt is None and (cam.width, cam.height) == (30, 37)  # int(2 * 15.1), int(2 * 18.9)
    cam3, _, id3 = views.scene_view(SCENE, image_id=3, split="test_train", img_downscale=3, load_image=False)
    assert id3 == 3 and (cam3.width, cam3.height) == (14, 9)
    assert abs(float(cam3.K[0, 0]) - float(np.float32(38.0 * 14 / 42))) == 0
    with pytest.raises(KeyError):
        views.scene_view(SCENE, image_name="e.jpg", load_image=False)
    with pytest.raises(KeyError):
        views.scene_view(SCENE, image_id=99, load_image=False)


def test_jet_table_knots():
    """MATLAB jet(256) in closed form, as RGB: end points and the knots where a channel saturates."""
    from neuralrecon_w_amd.views import JET

    assert JET.shape == (256, 3) and JET.dtype == np.uint8
    assert tuple(JET[0]) == (0, 0, 131) and tuple(JET[255]) == (128, 0, 0)
    assert tuple(JET[95]) == (0, 255, 255) and tuple(JET[159]) == (255, 255, 0) and tuple(JET[223]) == (255, 0, 0)
    assert tuple(JET[31]) == (0, 0, 255) and tuple(JET[127]) == (128, 255, 128)
    i = np.arange(256)
    # the closed form of the issue, channel by channel
    for ch, (a, b) in enumerate(((-95, 287), (-31, 223), (33, 159))):
        v = np.clip(np.minimum((i + a) / 64.0, (b - i) / 64.0), 0, 1)
        assert np.array_equal(JET[:, ch], np.floor(255 * v + 0.5).astype(np.uint8))
    assert (np.diff(JET[:96, 2].astype(int)) >= 0).all() and (np.diff(JET[159:, 0].astype(int)) <= 0).all()


def test_png_writer_round_trips_through_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from neuralrecon_w_amd import views

    rs = np.random.RandomState(0)
    rgb = rs.randint(0, 256, size=(13, 29, 3)).astype(np.uint8)
    p = str(tmp_path / "sub" / "a.png")
    views.write_png(p, rgb)
    back = np.asarray(Image.open(p).convert("RGB"))
    assert np.array_equal(back, rgb)
    planes = [torch.from_numpy(rs.rand(3, 5, 7).astype(np.float32)) for _ in range(4)]
    planes[3][0, 1, 2] = float("nan")  # 0 / 0 normals stay NaN on the device: written as 0
    planes[2][1, 0, 0] = 1.7           # clamped
    w, h = views.write_panel(str(tmp_path / "panel.png"), planes[0], planes[1], None, planes[2], planes[3])
    assert (w, h) == (28, 5)
    img = np.asarray(Image.open(str(tmp_path / "panel.png")).convert("RGB"))
    assert img.shape == (5, 28, 3)
    for k, pl in enumerate(planes):
        want = np.floor(np.clip(np.nan_to_num(pl.numpy().astype(np.float64), nan=0.0), 0, 1).astype(np.float32) * np.float32(255) + np.float32(0.5))
        assert np.array_equal(img[:, 7 * k:7 * k + 7], want.astype(np.uint8).transpose(1, 2, 0)), k
    assert img[1, 21 + 2, 0] == 0 and img[0, 14, 1] == 255
    with pytest.raises(ValueError):
        views.write_panel(str(tmp_path / "bad.png"), planes[0], torch.zeros(3, 4, 7))


def test_command_line_arguments():
    rv = _script("render_view").build_parser()
    a = rv.parse_args(["--cfg_path", "c.yaml", "--ckpt_path", "x/last.ckpt", "--root_dir", "r"])
    assert a.image_id is None and a.image_name is None and a.img_downscale is None and a.chunk is None and a.out is None
    assert a.split == "test_train" and a.ssim_window == 3
    a = rv.parse_args(["--cfg_path", "c", "--ckpt_path", "k", "--image_id", "12", "--img_downscale", "2", "--chunk", "1024", "--out", "o.png"])
    assert (a.image_id, a.img_downscale, a.chunk, a.out) == (12, 2, 1024, "o.png")
    with pytest.raises(SystemExit):
        rv.parse_args(["--cfg_path", "c", "--ckpt_path", "k", "--image_id", "1", "--image_name", "a.jpg"])
    with pytest.raises(SystemExit):
        rv.parse_args(["--cfg_path", "c"])
    tr = _script("train").build_parser()
    a = tr.parse_args(["--cfg_path", "c.yaml"])
    assert a.val_every == 0 and a.val_mesh_every == 0 and a.val_chunk == 0  # both validation hooks are opt-in
    a = tr.parse_args(["--cfg_path", "c.yaml", "--val_every", "500", "--val_chunk", "2048"])
    assert a.val_every == 500 and a.val_chunk == 2048 and a.batch_size == 2048 and a.val_sfm_path is None
    assert tr.parse_args(["--cfg_path", "c.yaml", "--val_sfm_path", "../neuralsfm"]).val_sfm_path == "../neuralsfm"
    assert rv.parse_args(["--cfg_path", "c", "--ckpt_path", "k"]).sfm_path is None
    bv = _script("bench_view").build_parser().parse_args([])
    assert (bv.width, bv.height, bv.chunks) == (1024, 768, "1024,4096,16384")


def test_view_entry_points_refuse_the_cpu():
    """No CPU fallback: images on the host are an error, and the small-image / bad-window cases are refused before any launch."""
    from neuralrecon_w_amd import lib as L
    from neuralrecon_w_amd import views

    x = torch.rand(3, 8, 8)
    for call in (lambda: views.psnr(x, x), lambda: views.ssim(x, x), lambda: views.depth_colormap(x[0])):
        with pytest.raises(L.NeuconwHipError):
            call()
    with pytest.raises(ValueError):
        views.ssim(torch.rand(3, 5, 9), torch.rand(3, 5, 9), window=11)  # a side <= (11 - 1) / 2
    with pytest.raises(ValueError):
        views.ssim(x, x, window=4)
    assert views.Camera(np.eye(3), np.zeros((3, 4)), 4, 3, 0.1, 2.0).struct().width == 4
    assert views.DEFAULT_CHUNK in (1024, 4096, 16384)


def test_camera_struct_matches_the_c_layout(tmp_path):
    """sizeof / field offsets of the ctypes mirror of NcwViewCamera equal what the C compiler lays out."""
    import ctypes
    import subprocess

    from neuralrecon_w_amd import lib as L

    fields = ["fx", "c2w", "width", "height", "near", "far"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "neuconw_hip.h"\nint main(){printf("%zu", sizeof(NcwViewCamera));'
            + "".join('printf(" %%zu", offsetof(NcwViewCamera, %s));' % f for f in fields) + "return 0;}")
    c = tmp_path / "s.c"
    c.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).decode().split()]
    assert got == [ctypes.sizeof(L.NcwViewCamera)] + [getattr(L.NcwViewCamera, f).offset for f in fields]


def test_scene_view_reads_the_colmap_model_the_reference_reads(tmp_path):
    """datasets/phototourism.py:82-93: brandenburg_gate and palacio_de_bellas_artes read <root>/neuralsfm (`../neuralsfm` under
    dense/), every other scene dense/sparse.  scene_view's default follows that choice by directory name; sfm_path overrides
    it; a missing model is an error that names the switch.  (The golden items were recorded from the reference's dataset on
    exactly this layout: tests/golden/make_golden_view.py.)"""
    import shutil

    from neuralrecon_w_amd import views

    assert views.reference_sfm_path("data/heritage-recon/brandenburg_gate") == "../neuralsfm"
    assert views.reference_sfm_path("/x/palacio_de_bellas_artes/") == "../neuralsfm"
    assert views.reference_sfm_path("data/heritage-recon/lincoln_memorial") == "sparse"
    assert views.reference_sfm_path(SCENE) == "sparse"
    gold = np.load(os.path.join(GOLDEN, "view_golden.npz"))
    root = str(tmp_path / "brandenburg_gate")
    shutil.copytree(os.path.join(SCENE, "dense", "sparse"), os.path.join(root, "neuralsfm"))
    shutil.copy(os.path.join(SCENE, "split.tsv"), os.path.join(root, "split.tsv"))
    cam, gt, image_id = views.scene_view(root, split="test_train", img_downscale=2, load_image=False)
    assert image_id == int(gold["tt2_id"]) and np.array_equal(cam.K, gold["tt2_K"])
    assert np.abs(cam.c2w - gold["tt2_c2w"]).max() <= 1e-6 and abs(cam.near - float(gold["tt2_near64"])) <= 1e-9
    with pytest.raises(FileNotFoundError, match="sfm_path"):
        views.scene_view(root, sfm_path="sparse", load_image=False)
    other = str(tmp_path / "some_scene")
    shutil.copytree(root, other)
    with pytest.raises(FileNotFoundError, match="sfm_path"):
        views.scene_view(other, load_image=False)  # not one of the two scenes: dense/sparse, which is absent
    cam2, _, _ = views.scene_view(other, sfm_path="../neuralsfm", split="test_train", img_downscale=2, load_image=False)
    assert np.array_equal(cam2.c2w, cam.c2w)
