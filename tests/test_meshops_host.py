"""CPU: the numpy restatement of the mesh operations (tests/_meshops_ref.py) against hand-written cases, the refusals of
neuralrecon_w_amd.meshops, the binding, and the command lines that carry the new options."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests import _meshops_ref as R
from tests._util import ROOT

from neuralrecon_w_amd import lib as L
from neuralrecon_w_amd import meshops


# two triangles sharing an edge (0-1-2, 1-2-3), a third touching them in vertex 3 only, a detached one, vertex 9 unused
FACES = np.array([[2, 1, 0], [1, 2, 3], [3, 4, 5], [8, 7, 6]])
V = 10


def test_reference_components_by_shared_vertex():
    labels, sizes = R.components(FACES, V)
    assert labels.tolist() == [0, 0, 0, 0, 0, 0, 6, 6, 6, 9]          # touching in ONE vertex joins; label = smallest index
    assert sizes.tolist() == [3, 0, 0, 0, 0, 0, 1, 0, 0, 0]
    labels, sizes = R.components(FACES, V, keep=[1, 0, 1, 1])          # the mask cuts the first component at vertex 3
    assert labels.tolist() == [0, 0, 0, 3, 3, 3, 6, 6, 6, 9]
    assert sizes.tolist() == [1, 0, 0, 1, 0, 0, 1, 0, 0, 0]


def test_reference_invalid_faces_take_no_part():
    f = np.array([[0, 1, 2], [2, 3, 10], [3, 3, 4], [-1, 4, 5], [5, 6, 7]])
    assert R.valid(f, 10).tolist() == [True, False, False, False, True]
    labels, sizes = R.components(f, 10)
    assert labels.tolist() == [0, 0, 0, 3, 4, 5, 5, 5, 8, 9]
    assert sizes.sum() == 2 and sizes[0] == 1 and sizes[5] == 1
    assert R.face_select(f, 10).tolist() == [1, 0, 0, 0, 1]


def test_reference_selection_ties_go_to_the_smaller_label():
    sizes = np.array([0, 4, 0, 7, 4, 0, 4, 1], dtype=np.int32)
    assert R.select_components(sizes, largest=1).tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert R.select_components(sizes, largest=2).tolist() == [0, 1, 0, 1, 0, 0, 0, 0]
    assert R.select_components(sizes, largest=3).tolist() == [0, 1, 0, 1, 1, 0, 0, 0]
    assert R.select_components(sizes, min_faces=4).tolist() == [0, 1, 0, 1, 1, 0, 1, 0]
    assert R.select_components(sizes, min_faces=5, largest=2).tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert R.select_components(sizes).tolist() == [1] * 8
    assert R.select_components(sizes, largest=0).sum() == 0


def test_reference_face_rule_and_compaction():
    flags = np.zeros(V, dtype=np.uint8)
    flags[[1, 2, 3, 6]] = 1
    assert R.face_select(FACES, V, flags, 1).tolist() == [1, 1, 1, 1]
    assert R.face_select(FACES, V, flags, 2).tolist() == [1, 1, 0, 0]
    assert R.face_select(FACES, V, flags, 3).tolist() == [0, 1, 0, 0]
    labels, sizes = R.components(FACES, V)
    ok = R.select_components(sizes, largest=1)
    assert R.face_select(FACES, V, flags, 1, labels, ok).tolist() == [1, 1, 1, 0]
    verts = np.arange(V * 3, dtype=np.float64).reshape(V, 3)
    cols = np.arange(V * 3, dtype=np.uint8).reshape(V, 3)
    v, f, c, idx = R.submesh(verts, FACES, [0, 1, 0, 1], cols)
    assert idx.tolist() == [1, 2, 3, 6, 7, 8]                          # ascending old indices
    assert f.tolist() == [[0, 1, 2], [5, 4, 3]] and f.dtype == np.int32  # face order and corner order kept
    assert np.array_equal(v, verts[idx]) and np.array_equal(c, cols[idx])
    v, f, c, idx = R.submesh(verts, FACES, [0, 0, 0, 0])
    assert v.shape == (0, 3) and f.shape == (0, 3) and c is None and idx.shape == (0,)


def test_refusals():
    f = torch.from_numpy(FACES)
    verts = torch.zeros(V, 3)
    for call in (lambda: meshops.components(f, V), lambda: meshops.face_select(f, V),
                 lambda: meshops.submesh(verts, f, torch.ones(4, dtype=torch.uint8)), lambda: meshops.clean(verts, f),
                 lambda: meshops.select_components(torch.zeros(V, dtype=torch.int32))):
        with pytest.raises(L.NeuconwHipError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="F == 0"):
        meshops.components(torch.zeros(0, 3, dtype=torch.int64), V)
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        meshops.components(torch.zeros(4, 4, dtype=torch.int64), V)
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        meshops.components(torch.zeros(4, 3), V)                        # float faces
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        meshops.face_select(FACES, V)                                    # not a tensor
    for mc in (0, 4, -1):
        with pytest.raises(ValueError, match="min_corners"):
            meshops.face_select(f, V, min_corners=mc)
    with pytest.raises(ValueError, match="2\\^31"):
        meshops.components(f, 1 << 31)
    with pytest.raises(ValueError, match="labels and comp_ok"):
        meshops.face_select(f, V, labels=torch.zeros(V, dtype=torch.int32))
    with pytest.raises(ValueError):
        meshops.select_components(torch.zeros(V, dtype=torch.int32), min_faces=-1)


def test_new_symbols_are_bound_and_declared():
    names = {"ncw_mesh_cc_hook", "ncw_mesh_cc_flatten", "ncw_mesh_cc_sizes", "ncw_mesh_face_select", "ncw_mesh_compact_mark",
             "ncw_mesh_compact_faces"}
    assert names <= set(L.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "neuconw_hip.h")).read()
    for n in names:
        assert n + "(" in hdr, n
    assert L.ABI_VERSION >= 30


def test_command_lines_parse_the_new_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import clean_mesh
        import eval_pipeline
        import reproj_filter
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    base = ["--src_file", "m.ply", "--data_path", "d", "--output_path", "o"]
    a = reproj_filter.parse_args(base)
    assert (a.keep_faces, a.min_corners, a.min_component_faces) == (False, 1, 0)
    a = reproj_filter.parse_args(base + ["--keep_faces", "--min_corners", "3", "--min_component_faces", "20"])
    assert (a.keep_faces, a.min_corners, a.min_component_faces) == (True, 3, 20)
    with pytest.raises(SystemExit):
        reproj_filter.parse_args(base + ["--min_corners", "4"])
    e = eval_pipeline.parse_args(["--scene_name", "lincoln_memorial", "--pred_dir", "p"])
    assert (e.keep_faces, e.min_corners, e.min_component_faces, e.exact_recall) == (False, 1, 0, False)
    e = eval_pipeline.parse_args(["--scene_name", "lincoln_memorial", "--pred_dir", "p", "--keep_faces", "--min_corners", "2",
                                  "--min_component_faces", "5", "--exact_recall", "--sample_surface"])
    assert (e.keep_faces, e.min_corners, e.min_component_faces, e.exact_recall, e.sample_surface) == (True, 2, 5, True, 10)
    c = clean_mesh.parse_args(["--file_in", "a.ply", "--file_out", "b.ply"])
    assert (c.file_in, c.file_out, c.min_component_faces, c.largest_components) == ("a.ply", "b.ply", 0, None)
    c = clean_mesh.parse_args(["--file_in", "a.ply", "--file_out", "b.ply", "--min_component_faces", "9", "--largest_components", "2"])
    assert (c.min_component_faces, c.largest_components) == (9, 2)
    # extract_mesh.py parses inside main(): its two options are read from the source
    src = open(os.path.join(ROOT, "scripts", "extract_mesh.py")).read()
    assert '"--min_component_faces", type=int, default=0' in src and '"--largest_components", type=int, default=None' in src


def test_eval_pipeline_keep_faces_passes_argument_checking():
    """--keep_faces --exact_recall is no longer refused: the run then fails only on the missing run directory."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_pipeline.py"), "--scene_name", "brandenburg_gate",
                        "--pred_dir", os.path.join(tempfile.gettempdir(), "no_such_run"), "--data_root",
                        os.path.join(tempfile.gettempdir(), "no_such_data"), "--keep_faces", "--exact_recall"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0
    assert "point cloud" not in r.stderr
    assert "no_such_" in r.stderr and ("FileNotFoundError" in r.stderr or "No such file" in r.stderr)


def test_keep_faces_needs_a_target_with_faces(tmp_path):
    """ValueError before any view is rendered (and before a GPU is needed)."""
    import yaml

    from neuralrecon_w_amd import ply, reproj
    from tests._util import GOLDEN

    scene = os.path.join(GOLDEN, "reproj_scene")
    cloud = str(tmp_path / "cloud.ply")
    ply.write(cloud, np.zeros((5, 3)))
    with open(os.path.join(scene, "config.yaml")) as fh:
        assert "sfm2gt" in yaml.safe_load(fh)
    with pytest.raises(ValueError, match="keep_faces needs a target with faces"):
        reproj.reproj_filter(os.path.join(scene, "mesh.ply"), cloud, scene, str(tmp_path / "out"), keep_faces=True,
                             device="cpu", verbose=False)
