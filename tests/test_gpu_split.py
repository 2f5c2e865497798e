"""GPU: scripts/prepare_data_split.py end to end on a temporary copy of tests/golden/split_scene, at the reference's default
thresholds and at `--roi_threshold 0 --static_threshold 0` (what its scripts/data_generation.sh passes): the kept set against
what the reference's own functions returned (tests/golden/split_golden.npz), the seeded row order, the report, the masks."""
import importlib.util
import json
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests._util import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SCENE = os.path.join(GOLDEN, "split_scene")
SCRIPT = os.path.join(ROOT, "scripts", "prepare_data_split.py")
CASES = {"default": ([], 0.5, 0.6, 1), "zero": (["--roi_threshold", "0", "--static_threshold", "0"], 0.0, 0.0, 2)}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "split_golden.npz"))


def _main():
    spec = importlib.util.spec_from_file_location("prepare_data_split", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.main


def _copy(tmp_path, tag):
    root = tmp_path / tag / "split_scene"
    shutil.copytree(SCENE, root)
    return str(root)


def _expected_rows(gold, rt, st, seed):
    """The reference's sets, in the order sceneprep documents: the ROI survivors (images.bin order) permuted by
    default_rng(seed), then the transient filter, which keeps the order."""
    roi_ref = [str(n) for n in gold["roi_kept_%03d" % round(100 * rt)]]
    static_ref = {str(n) for n in gold["static_kept_%03d" % round(100 * st)]}
    perm = [roi_ref[i] for i in np.random.default_rng(seed).permutation(len(roi_ref))]
    return roi_ref, [n for n in perm if n in static_ref]


def _read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    w, h = struct.unpack(">II", data[16:24])
    off, idat = 8, b""
    while off < len(data):
        (ln,) = struct.unpack(">I", data[off:off + 4])
        if data[off + 4:off + 8] == b"IDAT":
            idat += data[off + 8:off + 8 + ln]
        off += 12 + ln
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()  # filter type 0, as views.write_png writes
    return raw[:, 1:].reshape(h, w, 3)


@pytest.mark.parametrize("case", ["default", "zero"])
def test_split_equals_the_reference_sets(tmp_path, gold, case):
    from neuralrecon_w_amd import views

    flags, rt, st, num_test = CASES[case]
    main = _main()
    texts = []
    for run in ("a", "b"):
        root = _copy(tmp_path, run)
        main(["--root_dir", root, "--num_test", str(num_test), "--seed", "3"] + flags)
        tsv = os.path.join(root, "split_scene.tsv")
        texts.append(open(tsv, "rb").read())
    assert texts[0] == texts[1]  # the same rows in the same order on two runs
    roi_ref, rows_ref = _expected_rows(gold, rt, st, 3)
    lines = texts[0].decode().splitlines()
    assert lines[0] == "filename\tid\tsplit\tdataset"
    rows = [ln.split("\t") for ln in lines[1:]]
    assert sorted(r[0] for r in rows) == sorted(rows_ref)  # the reference's kept set
    assert [r[0] for r in rows] == rows_ref  # in the seeded order
    assert [r[1] for r in rows] == [str(i) for i in range(len(rows))]
    assert [r[2] for r in rows] == ["test"] * num_test + ["train"] * (len(rows) - num_test) and {r[3] for r in rows} == {"split_scene"}
    # the dataset's reader lists the same images
    scene = views.read_scene(root, "sparse")
    by_name = {str(n): int(i) for n, i in zip(gold["names"], gold["ids"])}
    assert scene["ids"] == [by_name[r[0]] for r in rows] and scene["ids_train"] == [by_name[r[0]] for r in rows[num_test:]]
    # the report: every image, a reason for every rejected one, the shares the GPU counted
    rep = json.load(open(os.path.join(root, "split_report.json")))
    names = [str(n) for n in gold["names"]]
    assert list(rep["images"]) == names and rep["seed"] == 3 and rep["roi_threshold"] == rt and rep["static_threshold"] == st
    npix = np.diff(gold["prefix"])
    for v, n in enumerate(names):
        e = rep["images"][n]
        assert e["kept"] == (n in rows_ref) and (e["reason"] is None) == e["kept"]
        if not e["kept"]:
            assert e["reason"] == ("less_ROI" if n not in roi_ref else "transient_much")
        assert abs(e["roi_pixels"] - int(gold["count64"][v])) <= int(gold["band_count"][v]) and e["roi_share"] == e["roi_pixels"] / int(npix[v])
        if n in roi_ref:
            assert e["static_share"] == float(gold["static_share"][v])
        else:
            assert e["static_share"] is None  # the transient filter never saw it
    assert not os.path.exists(os.path.join(root, "trash_images"))
    # another seed gives the same set
    root = _copy(tmp_path, "c")
    main(["--root_dir", root, "--num_test", str(num_test), "--seed", "4"] + flags)
    other = [ln.split("\t")[0] for ln in open(os.path.join(root, "split_scene.tsv")).read().splitlines()[1:]]
    assert other == _expected_rows(gold, rt, st, 4)[1]


def test_command_line_with_masks_and_refusals(tmp_path, gold):
    """The tool as a user starts it, default thresholds: --visualize writes one PNG per ROI-rejected view, holding that view's
    mask; a second start is refused (a split exists) and leaves the files as they are; --overwrite replaces them; too few
    images is an error that writes nothing."""
    root = _copy(tmp_path, "cli")
    cmd = [sys.executable, SCRIPT, "--root_dir", root, "--num_test", "1", "--visualize", "--nima_ckpt_path", "x.pth"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert "nima" in r.stdout.lower() and "ignored" in r.stdout
    roi_ref, rows_ref = _expected_rows(gold, 0.5, 0.6, 0)
    tsv = os.path.join(root, "split_scene.tsv")
    text = open(tsv).read()
    assert [ln.split("\t")[0] for ln in text.splitlines()[1:]] == rows_ref
    names = [str(n) for n in gold["names"]]
    rejected = [n for n in names if n not in roi_ref]
    pngs = sorted(os.listdir(os.path.join(root, "split_roi_masks")))
    assert pngs == sorted(n.split(".")[0] + "_roi.png" for n in rejected) and len(pngs) == 4
    prefix = gold["prefix"]
    for n in rejected:
        v = names.index(n)
        img = _read_png(os.path.join(root, "split_roi_masks", n.split(".")[0] + "_roi.png"))
        w, h = [int(x) for x in gold["wh"][v]]
        assert img.shape == (h, w, 3) and set(np.unique(img)) <= {0, 255}
        m = (img[:, :, 0] != 0).reshape(-1)
        out = gold["band"][int(prefix[v]):int(prefix[v + 1])] == 0
        assert np.array_equal(m[out], gold["roi64"][int(prefix[v]):int(prefix[v + 1])][out] != 0)
    r2 = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r2.returncode != 0 and "overwrite" in r2.stderr and open(tsv).read() == text
    main = _main()
    with pytest.raises(ValueError, match="remain"):
        main(["--root_dir", root, "--num_test", "3", "--overwrite"])  # three images remain: no training image would be left
    assert open(tsv).read() == text
    main(["--root_dir", root, "--num_test", "2", "--overwrite", "--seed", "9"])
    assert open(tsv).read() != text and open(tsv).read().count("test") == 2


def test_without_semantic_maps_and_with_min_observation(tmp_path, gold, capsys):
    main = _main()
    root = _copy(tmp_path, "nomaps")
    shutil.rmtree(os.path.join(root, "semantic_maps"))
    main(["--root_dir", root, "--num_test", "1"])
    assert "transient filter is skipped" in capsys.readouterr().out
    rows = [ln.split("\t")[0] for ln in open(os.path.join(root, "split_scene.tsv")).read().splitlines()[1:]]
    assert sorted(rows) == sorted(str(n) for n in gold["roi_kept_050"])
    root = _copy(tmp_path, "minobs")
    main(["--root_dir", root, "--num_test", "1", "--min_observation", "3", "--static_threshold", "0"])
    rows = [ln.split("\t")[0] for ln in open(os.path.join(root, "split_scene.tsv")).read().splitlines()[1:]]
    assert sorted(rows) == sorted(str(n) for n in gold["roi_kept_050_minobs3"])  # all four have static pixels
    rep = json.load(open(os.path.join(root, "split_report.json")))
    assert rep["images"]["col.jpg"]["reason"] == "less_covis" and rep["images"]["big.jpg"]["reason"] == "less_covis"
