"""Writes the two data files of K37 (ops.disp_colorize) from numpy and matplotlib only:

    depthmodelhardening_amd/data/magma_256.txt   the packaged colour table: (matplotlib's magma at 256 entries * 255).astype(uint8),
                                                 256 text lines "r g b" -- the package never imports matplotlib.
    tests/golden/disp_colorize.npz               for every case of tests/colorize_ref.py: the maps, (lo, hi, g) of numpy's virtual
                                                 index, np.percentile(., 95) per panel and the bytes of matplotlib's
                                                 ScalarMappable under every limit mode, for the maps and for their differences.

    python tools/make_goldens_colorize.py

The installed numpy and matplotlib are the yardstick (their versions are recorded).  A tool: not run by the tests.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import colorize_ref as R         # noqa: E402

TABLE = os.path.join(REPO, "depthmodelhardening_amd", "data", "magma_256.txt")
OUT = os.path.join(REPO, "tests", "golden", "disp_colorize.npz")


def numpy_plan(n, q=95):
    """(lo, hi, g) read out of numpy's own quantile helpers."""
    import numpy.lib._function_base_impl as F
    quant = np.asanyarray(np.true_divide(q, np.float32(100)))
    method = F._QuantileMethods["linear"]
    vi = np.asanyarray(method["get_virtual_index"](n, quant))
    prev, nxt = F._get_indexes(np.zeros(n, dtype=np.float32), vi, n)
    lo, hi = int(prev) % n, int(nxt) % n
    g = float(F._get_gamma(vi, np.floor(vi), method)) if hi != lo else 0.0
    return lo, hi, g


def main():
    import matplotlib
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    table = R.mpl_table()
    assert table.shape == (256, 3) and table.dtype == np.uint8
    with open(TABLE, "w") as f:
        f.write("# (matplotlib magma, 256 entries, * 255).astype(uint8): r g b per line; tools/make_goldens_colorize.py\n")
        f.writelines("%d %d %d\n" % tuple(row) for row in table)
    out = {"numpy_version": np.array(np.__version__), "matplotlib_version": np.array(matplotlib.__version__)}
    for name in R.CASES:
        maps = R.case_maps(name)
        out[name + "/maps"] = maps
        out[name + "/plan"] = np.array(numpy_plan(maps[0].size), dtype=np.float64)
        for diff in (False, True):
            src = R.panel_sources(maps, diff)
            tag = name + ("/diff" if diff else "/plain")
            out[tag + "/p95"] = np.array([np.percentile(s, 95) for s in src], dtype=np.float32)
            for mode in R.MODES:
                out[tag + "/" + mode] = np.stack([R.mpl_bytes(s, lo, hi) for s, (lo, hi) in zip(src, R.limits(src, mode))])
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes) and %s (%d bytes); numpy %s, matplotlib %s"
          % (TABLE, os.path.getsize(TABLE), OUT, os.path.getsize(OUT), np.__version__, matplotlib.__version__))


if __name__ == "__main__":
    main()
