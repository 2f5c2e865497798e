"""Writes tests/golden/rays_parent.npz: the outputs of the per-ray sampler and compositor kernels (tests/_rays_parent.py) as the
build of the commit BEFORE csrc/ncw_rays.hip became one object with templated capacities and shared section / alpha helpers
computes them.  Run once, on a GPU, in a checkout of that commit with this file and tests/_rays_parent.py copied in:

    python tests/golden/make_golden_rays_parent.py [output.npz]

tests/test_gpu_rays_parent.py compares the current build with the file bit for bit.  Re-running it on a later build would make
the fixture that build's own output and the test vacuous.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import _rays_parent as P  # noqa: E402


# a ray of one sample has one section, and it is sample_dist = 2 / S long on every ray
CONSTANT_BY_DESIGN = ("comp.S1_O0_R5.dists", "comp.S1_O1_R5.dists")


def main():
    raw_t = P.compute()
    raw = {k: v.numpy() for k, v in raw_t.items()}
    inside = np.concatenate([v.reshape(-1) for k, v in raw.items() if k.startswith("comp.") and k.endswith(".inside")])
    print("compositor: %d cases, inside fraction %.2f" % (len(P.comp_cases()), float(inside.mean())))
    assert set(np.unique(inside)) == {0.0, 1.0}, "inside does not take both values"
    n, _, S, O_ = P.BG_SELECT
    kept = raw["bg_select.idx"].size
    print("bg_select: %d of %d samples kept" % (kept, n * (S + O_)))
    assert 0 < kept < n * (S + O_), "the bg_select list is empty or complete"
    out = {k: v.numpy() for k, v in P.packed(raw_t).items()}
    again = {k: v.numpy() for k, v in P.packed(P.compute()).items()}
    assert sorted(out) == sorted(raw) == sorted(again)
    bad = []
    for k, v in raw.items():  # every output, before it is hashed
        if not np.isfinite(v).all():
            bad.append("%s is not finite" % k)
        if k not in CONSTANT_BY_DESIGN and not (v.size > 1 and (v != v.reshape(-1)[0]).any()):
            bad.append("%s is constant" % k)
        if not np.array_equal(out[k], again[k]):
            bad.append("%s: a second run differs from the first" % k)
    assert not bad, bad
    out["inputs_digest"] = np.frombuffer(P.inputs_digest().encode("ascii"), dtype=np.uint8)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "rays_parent.npz")
    np.savez_compressed(path, **out)
    print("%s: %d outputs, %d bytes" % (path, len(out) - 1, os.path.getsize(path)))


if __name__ == "__main__":
    main()
