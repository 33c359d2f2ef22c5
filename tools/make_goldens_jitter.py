"""Writes tests/golden/pil_jitter.npz: Pillow's own results for the cases of tests/jitter_ref.py.

    python tools/make_goldens_jitter.py

Needs only Pillow (the installed one is the yardstick, as for K31): ``ImageEnhance.Brightness`` / ``Contrast`` / ``Color`` and the
``convert("HSV")``, add, ``convert("RGB")`` hue step, chained as torchvision 0.8.2's ColorJitter chains them on PIL images.  The
file holds expected outputs only (``<case>``: uint8 [B, 3, H, W]) and the Pillow version that made them; the inputs and the
transforms are regenerated from the seeds in tests/jitter_ref.py.

A tool: not run by the tests.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import jitter_ref as J          # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "pil_jitter.npz")


def main():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__)}
    for key, images, params in J.golden_cases():
        out[key] = J.pillow_batch(images, params)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes, Pillow %s)" % (OUT, os.path.getsize(OUT), PIL.__version__))


if __name__ == "__main__":
    main()
