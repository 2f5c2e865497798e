"""GPU: the `--val_every` hook of scripts/train.py -- every N steps rank 0 renders the dataset's validation view, prints
val/psnr and writes the GT | prediction | depth | normal panel (lightning_modules/neuconw_system.py:404-464, 533-546) -- on the
synthetic scene of tests/test_gpu_train_driver.py, to which a COLMAP camera, one registered image and its PNG are added.  The
hook must not change what the training stream computes: the parameters after 4 steps are bitwise those of a run without it."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._util import ROOT

pytestmark = pytest.mark.gpu

IMG_W, IMG_H = 256, 192  # the `val` split clamps the downscale to 8: a 32 x 24 view


def _add_view(root):
    """cameras.bin / images.bin (one PINHOLE camera at (0, 0, -2) looking along +z, COLMAP axes), a split file and the image."""
    from neuralrecon_w_amd import views

    sp = os.path.join(root, "dense", "sparse")
    with open(os.path.join(sp, "cameras.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", 1) + struct.pack("<iiQQ", 1, 1, IMG_W, IMG_H) + struct.pack("<4d", 330.0, 330.0, IMG_W / 2, IMG_H / 2))
    with open(os.path.join(sp, "images.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", 1) + struct.pack("<i7di", 5, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 1) + b"v.png\x00" + struct.pack("<Q", 0))
    with open(os.path.join(root, "synth.tsv"), "w") as fh:
        fh.write("filename\tid\tsplit\tdataset\nv.png\t5\ttrain\tsynthetic\n")
    yy, xx = np.mgrid[0:IMG_H, 0:IMG_W]
    img = np.stack([255 * xx / (IMG_W - 1), 255 * yy / (IMG_H - 1), 127 + 100 * np.sin(0.05 * xx + 0.08 * yy)], -1)
    views.write_png(os.path.join(root, "dense", "images", "v.png"), np.clip(img, 0, 255).astype(np.uint8))


def test_val_every_writes_panels_prints_psnr_and_leaves_training_bitwise(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from tests.test_gpu_train_driver import _write_scene

    root = str(tmp_path / "scene")
    cfg = _write_scene(root)
    _add_view(root)
    base = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--cfg_path", cfg, "--batch_size", "64", "--num_epochs", "3",
            "--max_steps", "4", "--prec", "f32", "--log_every", "1"]

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return r.stdout

    out = run(["--exp_name", "v", "--val_every", "2", "--val_chunk", "500"])  # 768 rays: one full and one ragged chunk
    val = [l for l in out.splitlines() if l.startswith("[val]") and "val/psnr" in l]
    assert len(val) == 2 and "step 2:" in val[0] and "step 4:" in val[1], out[-2000:]
    for l in val:
        p = float(l.split("val/psnr")[1].split()[0])
        assert np.isfinite(p) and 0 < p < 60, l
    for step in (2, 4):
        path = os.path.join(root, "ckpts", "v", "val", "%08d.png" % step)
        assert os.path.isfile(path), path
        im = Image.open(path)
        assert im.size == (4 * (IMG_W // 8), IMG_H // 8) and im.mode == "RGB"
        a = np.asarray(im)
        w = IMG_W // 8
        assert a[:, :w].std() > 10          # the GT tile is the image
        assert a[:, 2 * w:3 * w].max() > 0  # the depth tile went through the colour map
    plain = run(["--exp_name", "b"])
    assert "[val]" not in plain
    losses = lambda o: [l.split("loss")[1].split()[0] for l in o.splitlines() if l.startswith("epoch")]  # noqa: E731
    assert losses(out) == losses(plain) and len(losses(out)) == 4
    a = torch.load(os.path.join(root, "ckpts", "v", "last.ckpt"), map_location="cpu")
    b = torch.load(os.path.join(root, "ckpts", "b", "last.ckpt"), map_location="cpu")
    assert a["global_step"] == b["global_step"] == 4
    for k in a["state_dict"]:
        assert torch.equal(a["state_dict"][k], b["state_dict"][k]), k
