"""GPU: the one voxel walk (csrc/ncw_dda.h: dda_walk with a stop, voxel_of_point, NcwCacheOctree through ray_voxel_near_far)
computes what the commit before the merge computed, bit for bit: ncw_ray_voxel_near_far, both passes of ncw_ray_voxel_trace,
ncw_voxel_view_seen (voxel plane, depth plane, `seen` words) at levels 3, 5 and 10 and ncw_cache_rows with use_voxel, against
tests/golden/dda_parent.npz, which tests/golden/make_golden_dda_parent.py recorded on that commit's build
(tests/_dda_cases.py holds the seeded inputs and the calls both share).  Every output is compared as raw 32-bit patterns; the
columns of the cache rows that the walk does not touch through the SHA-256 of their bytes (_dda_cases.packed)."""
import os

import numpy as np
import pytest
import torch

from tests import _dda_cases as D
from tests._util import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    z = np.load(os.path.join(GOLDEN, "dda_parent.npz"))
    assert bytes(z["inputs_digest"]).decode("ascii") == D.inputs_digest(), "the seeded inputs are not the recorded ones"
    return {k: torch.from_numpy(z[k]) for k in z.files if k != "inputs_digest"}


@pytest.fixture(scope="module")
def ours():
    return D.packed(D.compute("cuda:0"))


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _names(prefix):
    return [prefix + k for k in ("near", "far", "counts", "nug_ray", "nug_voxel", "nug_depth", "view_voxel", "view_depth",
                                 "seen_index", "seen_word")]


def test_the_fixture_holds_every_output(parent, ours):
    assert sorted(parent) == sorted(ours) == sorted(sum((_names("L%d_" % lv) for lv in D.LEVELS), []) +
                                                    ["cache_near_far", "cache_keep", "cache_rest_sha256"])


@pytest.mark.parametrize("level", D.LEVELS)
def test_walk_outputs_are_the_parents(parent, ours, level):
    for name in _names("L%d_" % level):
        a, b = ours[name], parent[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(_bits(a), _bits(b)), "%s: %d of %d words differ" % (name, int((_bits(a) != _bits(b)).sum()), a.numel())


def test_cache_rows_are_the_parents(parent, ours):
    for name in ("cache_near_far", "cache_keep", "cache_rest_sha256"):
        a, b = ours[name], parent[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(_bits(a), _bits(b)), "%s: %d of %d words differ" % (name, int((_bits(a) != _bits(b)).sum()), a.numel())
