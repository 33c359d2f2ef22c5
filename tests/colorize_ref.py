"""The cases of K37 (ops.disp_colorize): seeded float32 maps, the panels of every limit mode, and the two host expressions the
kernel is held to -- ``np.percentile(a, 95)`` and matplotlib's ``(ScalarMappable(Normalize(vmin, vmax), 'magma').to_rgba(a)[..., :3]
* 255).astype(uint8)``.  tools/make_goldens_colorize.py records their results in tests/golden/disp_colorize.npz;
tests/test_colorize_ref.py holds the numpy twin to them, tests/test_gpu_colorize.py the kernel to the twin.

Every case is a batch of three maps with different contents.  Image 0 is the one whose percentile is the shared ``vmax`` of the
"zero_ref" panels, so its percentile is positive in every case (matplotlib refuses vmin > vmax).
"""
import numpy as np

MODES = ("min_p95", "zero_ref", "min_max")
CASES = ("1x1", "3x7", "37x53", "constant", "eighths", "signed", "above")


def case_maps(name):
    """float32 [3, h, w]."""
    rng = np.random.RandomState(3700 + CASES.index(name))
    if name == "1x1":
        return np.array([[[0.625]], [[0.11]], [[1.7]]], dtype=np.float32)
    if name == "3x7":       # n = 21: 20 * 0.95 = 19, the virtual index lands on or next to an integer
        return rng.rand(3, 3, 7).astype(np.float32)
    if name == "37x53":
        return (rng.rand(3, 37, 53) * np.array([1.0, 0.3, 2.5])[:, None, None]).astype(np.float32)
    if name == "constant":  # vmin == vmax: every byte is TAB[0]
        return np.broadcast_to(np.array([0.25, 0.5, 3.0], dtype=np.float32)[:, None, None], (3, 5, 9)).copy()
    if name == "eighths":   # ties at the selected ranks
        return (np.floor(rng.rand(3, 37, 53) * 8) / 8).astype(np.float32)
    if name == "signed":    # negatives and both zeros
        m = (rng.rand(3, 11, 23) * 1.3 - 0.3).astype(np.float32)
        m[:, 0, :6] = np.float32(-0.0)
        m[:, 1, :6] = np.float32(0.0)
        m[1] = -np.abs(m[1])            # one map without a positive value: its percentile is negative or a zero
        m[1, 2, :4] = np.float32(-0.0)
        return m
    if name == "above":     # under image 0's limit: values above vmax and exactly at vmax (index 255)
        m = rng.rand(3, 19, 31).astype(np.float32)
        vmax = np.percentile(m[0], 95)
        m[1:] *= np.float32(2.0)
        m[1, 3, :5] = vmax
        m[2, 7, 10:14] = vmax
        m[2, 8, :3] = np.nextafter(vmax, np.float32(0))
        return m
    raise KeyError(name)


def panels(mode, diff=False):
    """The three panels of a case under ``mode``: the maps themselves, or |map i - map (i + 1) % 3| with ``diff`` (the limit of
    "zero_ref" is then the percentile of the first difference)."""
    return [(i, (i + 1) % 3 if diff else -1, mode, 0 if mode == "zero_ref" else i) for i in range(3)]


def panel_sources(maps, diff=False):
    return np.stack([np.abs(maps[i] - maps[(i + 1) % 3]) if diff else maps[i] for i in range(3)])


def limits(src, mode):
    """(vmin, vmax) float32 per panel, from numpy: what the reference passes to Normalize (test_simple.py:152-153, my_utils.py:55,
    61-67)."""
    p95 = [np.percentile(s, 95) for s in src]
    assert all(p.dtype == np.float32 for p in p95)
    if mode == "min_p95":
        return [(s.min(), p) for s, p in zip(src, p95)]
    if mode == "zero_ref":
        return [(np.float32(0), p95[0]) for _ in src]
    return [(s.min(), s.max()) for s in src]


def mpl_bytes(a, vmin, vmax):
    """The reference's colour expression (MD2/test_simple.py:153-155), live."""
    import matplotlib as mpl
    import matplotlib.cm as cm
    mapper = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=vmin, vmax=vmax), cmap="magma")
    return (mapper.to_rgba(a)[..., :3] * 255).astype(np.uint8)


def mpl_table():
    import matplotlib
    return (np.asarray(matplotlib.colormaps["magma"].resampled(256)(np.arange(256)))[:, :3] * 255).astype(np.uint8)
