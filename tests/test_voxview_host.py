"""CPU side of the point-cloud source of the reprojection filter: the cube and level of reproj.cloud_cube against
tools/prepare_data/generate_voxel.py:104-118, 146 restated, its refusals, the binding of the two entry points of
csrc/ncw_voxview.hip against the header, and the command line."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests._util import ROOT

from neuralrecon_w_amd import lib as L
from neuralrecon_w_amd import reproj


# (eval_bbx, voxel_size) -> the centre, half the longest edge and the level, worked out by hand
@pytest.mark.parametrize("bbx,voxel_size,origin,scale,level", [
    ([[100.0, -220.0, 30.0], [140.0, -190.0, 62.0]], 1.0, (120.0, -205.0, 46.0), 20.0, 5),      # longest edge x: 40 / 1 -> 2^5.3
    ([[-2.0, -6.0, 0.5], [3.0, 9.5, 4.0]], 0.12, (0.5, 1.75, 2.25), 7.75, 7),                   # longest edge y: 15.5 / 0.12 = 129.2
    ([[0.0, 0.0, -40.0], [1.0, 2.0, 24.0]], 0.07, (0.5, 1.0, -8.0), 32.0, 9),                   # longest edge z: 64 / 0.07 = 914
    ([[0.0, 0.0, -40.0], [1.0, 2.0, 24.0]], 0.125, (0.5, 1.0, -8.0), 32.0, 9),                  # 64 / 0.125 = 512 exactly: level 9
    ([[0.0, 0.0, -40.0], [1.0, 2.0, 24.0]], 0.12500001, (0.5, 1.0, -8.0), 32.0, 8),             # just above the boundary
    ([[0.0, 0.0, -40.0], [1.0, 2.0, 24.0]], 8.0, (0.5, 1.0, -8.0), 32.0, 3),                    # the lowest level, at its boundary
    ([[0.0, 0.0, -40.0], [1.0, 2.0, 24.0]], 64.0 / 2047.5, (0.5, 1.0, -8.0), 32.0, 10),         # the highest
])
def test_cube_and_level_follow_gen_octree(bbx, voxel_size, origin, scale, level):
    """generate_voxel.py:104-118, 146 with in_sfm=False: the box as given, its centre, half its longest edge, the level."""
    o, s, lv = reproj.cloud_cube({"eval_bbx": bbx, "sfm2gt": np.eye(4).tolist()}, voxel_size)
    assert o.dtype == np.float64 and np.array_equal(o, np.array(origin))
    assert s == scale and lv == level
    assert 2.0 ** lv <= 2 * s / voxel_size < 2.0 ** (lv + 1)


def test_cube_refusals_name_the_level_and_the_size_that_fits():
    bbx = [[0.0, 0.0, -40.0], [1.0, 2.0, 24.0]]
    with pytest.raises(ValueError, match=r"level 11 .*smallest voxel_size that fits is above 0\.03125"):
        reproj.cloud_cube({"eval_bbx": bbx}, 64.0 / 2048)  # exactly 2^11
    assert reproj.cloud_cube({"eval_bbx": bbx}, 0.03125 * (1 + 1e-9))[2] == 10  # and just above the named size fits
    with pytest.raises(ValueError, match=r"level 2 .*largest voxel_size that fits is 8"):
        reproj.cloud_cube({"eval_bbx": bbx}, 8.000001)
    with pytest.raises(ValueError, match="eval_bbx"):
        reproj.cloud_cube({"sfm2gt": np.eye(4).tolist()}, 0.1)
    with pytest.raises(ValueError, match="span no volume"):
        reproj.cloud_cube({"eval_bbx": [[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]}, 0.1)


def test_voxel_cloud_refuses_the_cpu():
    with pytest.raises(L.NeuconwHipError, match="GPU only"):
        reproj.VoxelCloud(np.zeros((4, 3)), {"eval_bbx": [[0, 0, 0], [1, 1, 1]]}, 0.01, device="cpu")


_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "void*": C.c_void_p, "const float*": C.c_void_p,
           "float*": C.c_void_p, "int32_t*": C.c_void_p, "uint32_t*": C.c_void_p, "const uint32_t*": C.c_void_p,
           "uint8_t*": C.c_void_p, "const NcwVoxelView*": C.POINTER(L.NcwVoxelView),
           "const NcwCacheOctree*": C.POINTER(L.NcwCacheOctree)}


def _header_args(name):
    src = open(os.path.join(ROOT, "include", "neuconw_hip.h")).read()
    m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, src, flags=re.M | re.S)
    assert m, name
    args = []
    for a in m.group(1).replace("\n", " ").split(","):
        typ = re.sub(r"\s*\w+\s*$", "", a.strip())  # drop the parameter's name
        args.append(re.sub(r"\s*\*", "*", typ))
    return args


@pytest.mark.parametrize("name,n_args", [("ncw_voxel_view_seen", 8), ("ncw_voxel_points_seen", 6)])
def test_binding_declares_the_header_argument_lists(name, n_args):
    args = _header_args(name)
    assert len(args) == n_args
    res, proto = L._PROTOS[name]
    assert res is C.c_int and proto == [_CTYPES[a] for a in args], (args, proto)
    assert L.ABI_VERSION >= 24


def test_view_struct_matches_the_c_layout(tmp_path):
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "neuconw_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", '
            "sizeof(NcwVoxelView), offsetof(NcwVoxelView, pose), offsetof(NcwVoxelView, o_norm), offsetof(NcwVoxelView, width));return 0;}")
    c = tmp_path / "s.c"
    c.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "s")])
    size, pose, o_norm, width = map(int, subprocess.check_output([str(tmp_path / "s")]).decode().split())
    V = L.NcwVoxelView
    assert (C.sizeof(V), V.pose.offset, V.o_norm.offset, V.width.offset) == (size, pose, o_norm, width)


def test_command_line_help_still_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "reproj_filter.py"), "--help"], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--src_file", "--target_file", "--data_path", "--output_path", "--gt", "--visualize", "--voxel_size", "--n_cpus",
                 "--n_gpus"):
        assert flag in r.stdout
