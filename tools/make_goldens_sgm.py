"""Writes tests/golden/sgm_disparity.npz: the maps of the loop reference tests/sgm_ref.py (the pixel-by-pixel statement of K35's
matcher) for ``sgm_ref.golden_cases()`` -- the four shapes, with and without ``reverse``, at three speckle
windows -- as int16 [H, W] under the case's key.  A few tens of KB.

    python tools/make_goldens_sgm.py [--check]

``--check`` recomputes and compares instead of writing.  tests/test_sgm_ref.py holds both the loop reference and the host twin
``ops.sgm_disparity_host`` to the file; tests/test_gpu_sgm.py holds the kernel to the loop reference.  Also prints the shares
that tests/test_sgm_ref.py and DESIGN.md record (valid share of the matched columns, share of the valid pixels within one
disparity of the truth).
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import sgm_ref as R  # noqa: E402


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    maps = {}
    for key, H, W, p, reverse, seed in R.golden_cases():
        base, lookup, truth = R.make_pair(H, W, p["numDisparities"], seed)
        maps[key] = R.disparity(base, lookup, p, reverse)
        if not reverse:
            print("%-28s valid %.4f, near the truth %.4f" % ((key,) + R.shares(maps[key], truth, p["numDisparities"])))
    if "--check" in argv:
        with np.load(R.GOLDEN_PATH) as f:
            bad = [k for k in maps if k not in f.files or not np.array_equal(f[k], maps[k])] + [k for k in f.files if k not in maps]
        print("differ: %s" % bad if bad else "the file holds the loop reference's maps")
        return 1 if bad else 0
    np.savez_compressed(R.GOLDEN_PATH, **maps)
    print("wrote %s: %d maps, %d bytes" % (R.GOLDEN_PATH, len(maps), os.path.getsize(R.GOLDEN_PATH)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
