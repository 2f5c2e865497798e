"""Host side of the held-out-view evaluation (neuralrecon_w_amd/appfit.py, scripts/eval_views.py): which pixels are fitted and
which are scored, which images are held out, argument parsing, the no-CPU-fallback refusals and the ABI.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests._util import ROOT


@pytest.mark.parametrize("w,h", [(4, 3), (5, 3), (1, 2)])
def test_left_right_indices_are_the_references_slicing(w, h):
    """datasets/phototourism.py:728-733 restated: reshape(h, w, -1), [:, : w // 2] and [:, w // 2 :], reshape(-1, C)."""
    from neuralrecon_w_amd import appfit

    rows = np.arange(w * h * 2).reshape(w * h, 2)  # a payload per pixel, row-major like all_rays[idx]
    img = rows.reshape(h, w, -1)
    want_l, want_r = img[:, : w // 2].reshape(-1, 2), img[:, w // 2:].reshape(-1, 2)
    left, right = appfit.half_pixel_indices(w, h)
    assert np.array_equal(rows[left], want_l) and np.array_equal(rows[right], want_r)
    assert left.size == (w // 2) * h and right.size == (w - w // 2) * h  # an odd width gives the right half the extra column
    assert np.array_equal(np.sort(np.concatenate([left, right])), np.arange(w * h))


def test_ray_subset_is_seeded_and_stays_in_the_left_half():
    from neuralrecon_w_amd import appfit

    w, h = 37, 23
    left, _ = appfit.half_pixel_indices(w, h)
    a, b, c = appfit.ray_subset(w, h, 100, 7), appfit.ray_subset(w, h, 100, 7), appfit.ray_subset(w, h, 100, 8)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert a.size == 100 and len(set(a.tolist())) == 100 and np.all(np.diff(a) > 0)
    assert set(a.tolist()) <= set(left.tolist()) and np.all(a % w < w // 2)
    assert np.array_equal(appfit.ray_subset(w, h, 10 ** 6, 0), left)  # fewer pixels than asked for: all of them


def test_held_out_rows_are_the_test_rows_of_the_tsv(tmp_path):
    from neuralrecon_w_amd import appfit

    with open(tmp_path / "scene.tsv", "w") as fh:
        fh.write("filename\tid\tsplit\tdataset\na.jpg\t1\ttrain\ts\nb.jpg\t2\ttest\ts\nc.jpg\t3\ttrain\ts\nd.jpg\t4\ttest\ts\n")
    assert appfit.held_out_rows(str(tmp_path)) == ["b.jpg", "d.jpg"]
    with pytest.raises(FileNotFoundError):
        appfit.held_out_rows(str(tmp_path / "nowhere"))


def _script():
    spec = importlib.util.spec_from_file_location("eval_views_script", os.path.join(ROOT, "scripts", "eval_views.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_arguments():
    from neuralrecon_w_amd import appfit

    ap = _script().build_parser()
    a = ap.parse_args(["--cfg_path", "c.yaml", "--ckpt_path", "k.ckpt", "--root_dir", "r"])
    assert (a.n_rays, a.steps, a.lr, a.seed, a.init, a.chunk, a.out_dir, a.img_downscale) == (
        appfit.DEFAULT_N_RAYS, appfit.DEFAULT_STEPS, appfit.DEFAULT_LR, 0, "mean", 1024, None, None)
    a = ap.parse_args(["--cfg_path", "c", "--ckpt_path", "k", "--root_dir", "r", "--img_downscale", "4", "--n_rays", "99", "--steps", "7",
                       "--lr", "0.5", "--seed", "3", "--init", "zeros", "--chunk", "64", "--out_dir", "o"])
    assert (a.img_downscale, a.n_rays, a.steps, a.lr, a.seed, a.init, a.chunk, a.out_dir) == (4, 99, 7, 0.5, 3, "zeros", 64, "o")
    for bad in (["--cfg_path", "c", "--ckpt_path", "k"], ["--cfg_path", "c", "--ckpt_path", "k", "--root_dir", "r", "--init", "ones"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_cpu_tensors_are_refused():
    import neuralrecon_w_amd as nw
    from neuralrecon_w_amd import appfit
    from tests._build import build_system

    emb, neuconw, nerf, rdr = build_system(device="cpu", n_samples=8, n_importance=8)
    with pytest.raises(nw.NeuconwHipError, match="no CPU fallback"):
        appfit.freeze_rays(rdr, torch.zeros(4, 8))
    with pytest.raises(nw.NeuconwHipError, match="no CPU fallback"):
        appfit.AppearanceFit(rdr, [object()], torch.zeros(4, 3), torch.zeros(16))
    with pytest.raises(nw.NeuconwHipError, match="no CPU fallback"):
        appfit.fit_view(rdr, nw.Camera(np.eye(3), np.eye(4)[:3], 4, 2, 1.0, 3.0), torch.zeros(3, 2, 4))
    with pytest.raises(nw.NeuconwHipError, match="no CPU fallback"):
        rdr._render_with_normals(torch.zeros(4, 8), torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long),
                                 a_code=torch.zeros(16))
    with pytest.raises(ValueError):
        appfit.AppearanceFit(rdr, [], torch.zeros(4, 3), torch.zeros(16))


def test_initial_code():
    from neuralrecon_w_amd import appfit
    from tests._build import build_system

    emb, neuconw, nerf, rdr = build_system(device="cpu")
    w = emb.weight.detach()
    assert torch.equal(appfit.initial_code(rdr, "zeros"), torch.zeros(16))
    assert torch.allclose(appfit.initial_code(rdr, "mean"), w.mean(0))
    assert torch.allclose(appfit.initial_code(rdr, "mean", [3, 5, 9999]), w[[3, 5]].mean(0))  # ids past the vocabulary are left out
    assert torch.equal(appfit.initial_code(rdr, torch.arange(16.0)), torch.arange(16.0))
    with pytest.raises(ValueError):
        appfit.initial_code(rdr, "ones")


def test_new_symbols_are_bound_and_declared():
    from neuralrecon_w_amd import lib as L

    names = {"ncw_appfit_loss", "ncw_appfit_step", "ncw_appfit_step_scratch_floats"}
    assert names <= set(L.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "neuconw_hip.h")).read()
    for n in names:
        assert n + "(" in hdr, n
    assert L.ABI_VERSION >= 29
