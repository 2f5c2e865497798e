"""Writes tests/golden/dda_parent.npz: the outputs of every kernel built on the voxel DDA walk (tests/_dda_cases.py) as the
build of the commit BEFORE the walks were merged into one computes them.  Run once, on a GPU, in a checkout of that commit with
this file and tests/_dda_cases.py copied in:

    python tests/golden/make_golden_dda_parent.py [output.npz]

tests/test_gpu_dda_parent.py compares the current build with the file bit for bit.  Re-running it on a later build would make
the fixture that build's own output and the test vacuous.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import _dda_cases as D  # noqa: E402


def main():
    out = {k: v.numpy() for k, v in D.packed(D.compute()).items()}
    frac = lambda m: float(np.mean(m))  # noqa: E731
    multi = 0
    for level in D.LEVELS:
        p = "L%d_" % level
        near, counts, vox = out[p + "near"], out[p + "counts"], out[p + "view_voxel"]
        figures = (frac(near > 0), frac(near == 0), frac(counts > 0), frac(counts == 0), frac(vox >= 0), frac(vox < 0))
        print("level %2d: near-far hit %.2f miss %.2f | trace hit %.2f miss %.2f | pixels hit %.2f miss %.2f | nuggets %d, most per "
              "ray %d" % ((level,) + figures + (int(counts.sum()), int(counts.max()))))
        for hit, miss in (figures[0:2], figures[2:4], figures[4:6]):
            assert hit >= 0.25 and miss >= 0.10, (level, figures)
        assert (out[p + "far"][near > 0] >= near[near > 0]).all()
        multi += int((counts > 1).sum())
    assert multi >= 1, "no ray has more than one nugget"
    keep = out["cache_keep"]
    print("cache rows: kept %.2f dropped %.2f" % (frac(keep == 1), frac(keep == 0)))
    assert frac(keep == 1) >= 0.25 and frac(keep == 0) >= 0.10
    out["inputs_digest"] = np.frombuffer(D.inputs_digest().encode("ascii"), dtype=np.uint8)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "dda_parent.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
