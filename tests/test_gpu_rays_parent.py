"""GPU: csrc/ncw_rays.hip as one object -- the four LDS kernels as templates on the capacity (512 / 1088), the compositor
kernels on the ABI structs themselves, the section / NeuS alpha / background alpha formulas stated once -- computes what the
commit before computed, bit for bit: ncw_composite_fwd / _bwd over every shape and option case of tests/_ray_cases.py (1, 63, 64,
65, 512 and 513 columns, 1056 + 32, 1088, no background, trim_sphere off, no background_rgb, the value switches, inv_s 20 / 403 /
3000), with cos_anneal as a device scalar and with grad_scale 8 and a device scale, ncw_upsample at n = 2 .. 1087, ncw_sort_merge
at 512 / 513 / 1088, ncw_sample_coarse, ncw_boundary and ncw_bg_select, against tests/golden/rays_parent.npz, which
tests/golden/make_golden_rays_parent.py recorded on that commit's build (tests/_rays_parent.py holds the seeded inputs and the
calls both share).  Per-ray outputs are compared as raw 32-bit patterns, per-sample outputs through the SHA-256 of their bytes.
No tolerance: a helper that reassociates one sum or moves one FMA fusion fails here."""
import os

import numpy as np
import pytest
import torch

from tests import _ray_cases as C
from tests import _rays_parent as P
from tests._util import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    z = np.load(os.path.join(GOLDEN, "rays_parent.npz"))
    assert bytes(z["inputs_digest"]).decode("ascii") == P.inputs_digest(), "the seeded inputs are not the recorded ones"
    return {k: torch.from_numpy(z[k]) for k in z.files if k != "inputs_digest"}


@pytest.fixture(scope="module")
def ours():
    return P.packed(P.compute("cuda:0"))


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(parent, ours, prefix):
    names = [k for k in parent if k.startswith(prefix)]
    assert names, prefix
    bad = []
    for name in names:
        a, b = ours[name], parent[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        if not torch.equal(_bits(a), _bits(b)):
            bad.append(name if not P.per_ray(name) else "%s: %d of %d words" % (name, int((_bits(a) != _bits(b)).sum()), a.numel()))
    assert not bad, "differ from the parent's: %s" % bad


def test_the_fixture_holds_every_output(parent, ours):
    assert sorted(parent) == sorted(ours)
    per_case = len(C.FWD_KEYS) - 2 + 1 + len(C.ADJ_KEYS)  # eik_num / eik_den are one array; weights_max is among FWD_KEYS
    assert sum(k.startswith("comp.S61_O4_R5.") for k in ours) == per_case


@pytest.mark.parametrize("c", P.comp_cases(), ids=C.case_id)
def test_compositor_is_the_parents(parent, ours, c):
    _same(parent, ours, "comp.%s." % C.case_id(c))


@pytest.mark.parametrize("tag", ["comp_cos_dev", "comp_scale8_dev", "comp_scale0"])
def test_compositor_scalars_are_the_parents(parent, ours, tag):
    """cos_anneal read from the device; grad_scale 8 times a device scale of 0.5; grad_scale 0, which the entry point turns into 1
    (the only field it edits) -- so its adjoints are those of the plain call."""
    _same(parent, ours, tag + ".")
    if tag != "comp_scale8_dev":
        for k in ours:
            if k.startswith(tag + "."):
                assert torch.equal(_bits(ours[k]), _bits(ours["comp." + k[len(tag) + 1:]])), k


@pytest.mark.parametrize("prefix", ["upsample.%d." % n for n, _, _ in P.UPSAMPLE] + ["merge.%d." % (a + b) for a, b, _ in P.MERGE] +
                         ["coarse.%d.%s." % (n, "jitter" if p else "plain") for n, _, p in P.COARSE] + ["boundary.", "bg_select."])
def test_sampler_is_the_parents(parent, ours, prefix):
    _same(parent, ours, prefix)
