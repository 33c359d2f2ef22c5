"""K37's host side, no GPU: ``ops.percentile_plan`` and the numpy twin ``ops.disp_colorize_host`` against numpy and matplotlib
themselves -- live where they are importable, and through tests/golden/disp_colorize.npz (tools/make_goldens_colorize.py) always --
the packaged colour table, the C ABI with its sanitizer driver, and the figures of my_utils.py on CPU tensors."""
import os
import subprocess

import numpy as np
import pytest
import torch

from depthmodelhardening_amd import ops
from tests import colorize_ref as R


def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return False
    return True


@pytest.fixture(scope="module")
def gold(golden):
    return golden("disp_colorize")


def _twin_percentile(a, q=95):
    """the plan's two order statistics and numpy's float32 lerp, as the twin and the kernel compute it"""
    lo, hi, g = ops.percentile_plan(a.size, q)
    s, g = np.sort(a, axis=None), np.float32(g)
    d = s[hi] - s[lo]
    return s[hi] - d * (1 - g) if g >= 0.5 else s[lo] + d * g


def test_percentile_plan_is_numpys_percentile_at_every_size():
    """Every n in 1 .. 4096 and the three workload sizes: random float32 data, and data quantised to 1/8 (ties).  Exact."""
    rng = np.random.RandomState(37)
    for n in list(range(1, 4097)) + [327680, 465750, 1048576]:
        for a in (rng.rand(n).astype(np.float32) * 3 - 1, (np.floor(rng.rand(n) * 8) / 8).astype(np.float32)):
            want = np.percentile(a, 95)
            got = _twin_percentile(a)
            assert want.dtype == np.float32 and got.dtype == np.float32
            assert got == want, (n, got, want)
        lo, hi, g = ops.percentile_plan(n)
        assert 0 <= lo <= hi <= min(lo + 1, n - 1) and 0.0 <= g < 1.0


def test_percentile_plan_other_quantiles_and_refusals():
    rng = np.random.RandomState(38)
    a = rng.rand(1000).astype(np.float32)
    for q in (0, 5, 50, 99, 100):
        assert _twin_percentile(a, q) == np.percentile(a, q)
    assert ops.percentile_plan(1) == (0, 0, 0.0) and ops.percentile_plan(7, 100) == (6, 6, 0.0)
    with pytest.raises(RuntimeError, match="positive"):
        ops.percentile_plan(0)
    with pytest.raises(RuntimeError, match=r"\[0, 100\]"):
        ops.percentile_plan(10, 101)


def test_golden_inputs_and_plans(gold):
    assert str(gold["numpy_version"]).split(".")[0] == np.__version__.split(".")[0]
    for name in R.CASES:
        maps = R.case_maps(name)
        assert np.array_equal(maps.view(np.uint32), gold[name + "/maps"].view(np.uint32)), name
        assert tuple(float(v) for v in ops.percentile_plan(maps[0].size)) == tuple(gold[name + "/plan"]), name
    # what the cases are there for
    assert ops.percentile_plan(21) == (19, 20, 0.0)
    assert np.unique(R.case_maps("eighths")).size <= 8
    signed = R.case_maps("signed")
    assert (signed < 0).any() and np.signbit(signed[signed == 0]).any() and not np.signbit(signed[signed == 0]).all()
    above = R.case_maps("above")
    vmax = np.percentile(above[0], 95)
    assert (above[1:] > vmax).any() and (above[1] == vmax).sum() >= 5 and (above[2] == vmax).sum() >= 4


@pytest.mark.parametrize("diff", [False, True], ids=["plain", "diff"])
@pytest.mark.parametrize("name", R.CASES)
def test_twin_equals_golden_and_live_matplotlib(gold, name, diff):
    """Zero differing bytes in every limit mode, and the percentile equal to np.percentile's."""
    maps = R.case_maps(name)
    src = R.panel_sources(maps, diff)
    tag = name + ("/diff" if diff else "/plain")
    for mode in R.MODES:
        out = ops.disp_colorize_host(torch.from_numpy(maps), R.panels(mode, diff), return_map=True)
        rgb, stats = out.rgb.numpy(), out.stats.numpy()
        assert rgb.shape == src.shape + (3,) and rgb.dtype == np.uint8
        assert np.array_equal(out.map.numpy().view(np.uint32), src.view(np.uint32))
        assert np.array_equal(rgb, gold[tag + "/" + mode]), (name, mode)
        assert np.array_equal(stats[:, 4], gold[tag + "/p95"]), (name, mode)
        assert np.array_equal(stats[:, 4], np.array([np.percentile(s, 95) for s in src]))
        assert np.array_equal(stats[:, 0], src.min((1, 2))) and np.array_equal(stats[:, 1], src.max((1, 2)))
        if _have_matplotlib():
            for i, (vmin, vmax) in enumerate(R.limits(src, mode)):
                assert np.array_equal(rgb[i], R.mpl_bytes(src[i], vmin, vmax)), (name, mode, i)
    if name == "constant":      # vmin == vmax: all TAB[0]
        flat = ops.disp_colorize_host(torch.from_numpy(maps), R.panels("min_p95", diff)).rgb.numpy()
        assert (flat == ops.magma_table()[0]).all()
    if name == "above" and not diff:
        top = ops.disp_colorize_host(torch.from_numpy(maps), R.panels("zero_ref")).rgb.numpy()
        vmax = np.percentile(maps[0], 95)
        assert (top[1][maps[1] >= vmax] == ops.magma_table()[255]).all() and (maps[1] == vmax).any()


def test_packaged_table():
    t = ops.magma_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8 and ops.COLORIZE_TABLE_PATH.endswith(".txt")
    assert tuple(t[0]) == (0, 0, 3) and tuple(t[255]) == (251, 252, 191)        # magma's ends
    if _have_matplotlib():
        assert np.array_equal(t, R.mpl_table())


def test_the_package_does_not_import_matplotlib():
    code = ("import sys, torch; from depthmodelhardening_amd import ops, my_utils; "
            "ops.disp_colorize_host(torch.rand(2, 4, 5)); my_utils.eval_depth_diff_jcl(torch.rand(3, 6, 7), torch.rand(3, 6, 7), None, "
            "disp1=torch.rand(4, 5), disp2=torch.rand(4, 5)); assert 'matplotlib' not in sys.modules")
    import sys
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_twin_mosaic_and_argument_checks():
    maps = torch.from_numpy(R.case_maps("37x53"))
    panels = R.panels("zero_ref") + [(0, 1, "min_max", 0)]
    single = ops.disp_colorize_host(maps, panels).rgb
    mosaic = torch.full((2 * 37 + 5, 2 * 53 + 7, 3), 77, dtype=torch.uint8)
    origins = [(0, 0), (1, 53 + 7), (37 + 5, 3), (37 + 4, 53 + 5)]
    out = ops.disp_colorize_host(maps, panels, out=mosaic, origins=origins)
    assert out.rgb is mosaic
    covered = torch.zeros(mosaic.shape[:2], dtype=torch.bool)
    for i, (y, x) in enumerate(origins):
        assert torch.equal(mosaic[y:y + 37, x:x + 53], single[i])
        covered[y:y + 37, x:x + 53] = True
    assert (mosaic[~covered] == 77).all()
    for bad, match in (((3, -1, "min_p95", 0), "outside the batch"), ((0, 3, "min_p95", 0), "outside the batch"),
                       ((0, -1, "p95", 0), "mode must be"), ((0, -1, "zero_ref", 4), "outside the"), ((0, -1, 7, 0), "mode must be")):
        with pytest.raises(RuntimeError, match=match):
            ops.disp_colorize_host(maps, [bad])
    with pytest.raises(RuntimeError, match="float32 tensor"):
        ops.disp_colorize_host(maps.double())
    with pytest.raises(RuntimeError, match="go together"):
        ops.disp_colorize_host(maps, out=mosaic)
    with pytest.raises(RuntimeError, match="leaves the"):
        ops.disp_colorize_host(maps, panels, out=mosaic, origins=[(0, 0), (0, 0), (0, 0), (50, 0)])
    with pytest.raises(RuntimeError, match="panels <="):
        ops.disp_colorize_host(maps, [(0, -1, "min_max", 0)] * 33)


def test_abi_names_sources_and_operator():
    import torch as _torch
    from depthmodelhardening_amd import _native as N, build, library
    assert {"dmh_disp_colorize", "dmh_disp_colorize_ws_size"} <= set(N.EXPORTS) and "disp_colorize.hip" in build.SOURCES
    assert "disp_colorize" in library.OPS and hasattr(_torch.ops.dmh, "disp_colorize")
    import ctypes
    assert ctypes.sizeof(N.ColorizePanel) == 24 and N.ColorizePanel.origin.offset == 16
    assert not any(f.startswith("-ffast-math") or f.startswith("-Ofast") or "unsafe-math" in f or "fp-contract=fast" in f
                   for f in build.FLAGS), "the colour stage needs the IEEE quotient"
    lib = N.lib()
    assert lib.dmh_disp_colorize_ws_size(2) == 2 * (3 * 2 * 2048 + 8) and lib.dmh_disp_colorize_ws_size(0) == -1
    p = (N.ColorizePanel * 1)(N.ColorizePanel(0, -1, 5, 0, 0))
    one = ctypes.c_void_p(64)
    assert lib.dmh_disp_colorize(one, 1, 4, 4, p, 1, 4, 4, 14, 15, 0.25, one, one, one, one, one, 48, 12, None) == 1
    assert b"bad mode word" in lib.dmh_last_error()


def test_fake_operator_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from depthmodelhardening_amd import library  # noqa: F401
    with FakeTensorMode():
        rgb, fmap, stats = torch.ops.dmh.disp_colorize(torch.empty(2, 6, 20), [0, -1, 0, 0, 0, 1, 2, 0, 1, -1, 1, 0], 12, 39)
    assert rgb.shape == (3, 12, 39, 3) and rgb.dtype == torch.uint8 and fmap.shape == (3, 12, 39) and stats.shape == (3, 5)


def test_colorize_host_side_under_address_sanitizer():
    """tests/asan/colorize_checks.c: a stand-alone program linked against the host-only sanitizer build of the library; every
    refusal of K37's entry points.  Nothing is launched and nothing is loaded into Python."""
    from depthmodelhardening_amd.build import ASAN_LIB_PATH, build_asan
    driver = build_asan(driver_name="colorize_checks")
    assert os.path.exists(ASAN_LIB_PATH)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([driver], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "colorize_checks: ok" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ figures
def _figure_inputs():
    g = torch.Generator().manual_seed(371)
    img1, img2 = torch.rand(1, 3, 20, 33, generator=g), torch.rand(1, 3, 20, 33, generator=g)
    disp1 = torch.rand(1, 1, 11, 29, generator=g)
    disp2 = (disp1 + 0.3 * torch.rand(1, 1, 11, 29, generator=g)).clamp(0, 1)
    return img1, img2, disp1, disp2


def test_eval_depth_diff_geometry_and_limits():
    """The 3 x 2 mosaic on CPU tensors: the image panels are ToPILImage's bytes, the colour panels the twin under the reference's
    limits (my_utils.py:55,61-67), the rest is background."""
    from depthmodelhardening_amd import my_utils as U
    img1, img2, disp1, disp2 = _figure_inputs()
    image, d1, d2 = U.eval_depth_diff(img1, img2, None, disp1=disp1, disp2=disp2)
    assert np.array_equal(d1, disp1[0, 0].numpy()) and np.array_equal(d2, disp2[0, 0].numpy())
    fig = np.array(image)
    height, width, img_at, colour_at = U.figure_layout((20, 33), (11, 29))
    assert fig.shape == (height, width, 3) and image.mode == "RGB"
    assert (height, width) == (8 + 20 + 8 + 2 * (11 + 8), 8 + 2 * (33 + 8))
    covered = np.zeros((height, width), dtype=bool)
    for im, (y, x) in zip((img1, img2), img_at):
        want = im[0].mul(255).byte().permute(1, 2, 0).numpy()        # ToPILImage: mul(255).byte()
        assert np.array_equal(fig[y:y + 20, x:x + 33], want)
        covered[y:y + 20, x:x + 33] = True
    a, b = disp1[0, 0].numpy(), disp2[0, 0].numpy()
    diff = np.abs(a - b)
    vmax = np.percentile(a, 95)
    want = [ops.colorize_bytes_host(a, 0, vmax), ops.colorize_bytes_host(b, 0, vmax), ops.colorize_bytes_host(diff, 0, vmax),
            ops.colorize_bytes_host(diff, diff.min(), diff.max())]
    for w, (y, x) in zip(want, colour_at):
        assert np.array_equal(fig[y:y + 11, x:x + 29], w)
        covered[y:y + 11, x:x + 29] = True
    assert (fig[~covered] == U.FIGURE_FILL).all() and covered.sum() == 2 * 20 * 33 + 4 * 11 * 29
    if _have_matplotlib():
        assert np.array_equal(want[2], R.mpl_bytes(diff, 0, vmax)) and np.array_equal(want[3], R.mpl_bytes(diff, None, None))


def test_eval_depth_diff_jcl_and_save_pic(tmp_path):
    from PIL import Image
    from depthmodelhardening_amd import my_utils as U
    img1, img2, disp1, disp2 = _figure_inputs()
    model = lambda x: disp1 if x is img1 else disp2         # noqa: E731  (the disparities come from the model when not given)
    image = U.eval_depth_diff_jcl(img1, img2, model)
    fig = np.array(image)
    height, width, img_at, colour_at = U.figure_layout((20, 33), (11, 29), jcl=True)
    assert fig.shape == (height, width, 3) == (8 + 20 + 8 + 2 * (11 + 8), 8 + 33 + 8, 3) and len(img_at) == 1 and len(colour_at) == 2
    a, b = disp1[0, 0].numpy(), disp2[0, 0].numpy()
    vmax = np.percentile(a, 95)
    (y, x), (y2, x2) = colour_at
    assert np.array_equal(fig[y:y + 11, x:x + 29], ops.colorize_bytes_host(a, 0, vmax))
    assert np.array_equal(fig[y2:y2 + 11, x2:x2 + 29], ops.colorize_bytes_host(np.abs(a - b), 0, vmax))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        U.eval_depth_diff_jcl(img1, img2, None, filename="fig", disp1=disp1, disp2=disp2)
        assert np.array_equal(np.array(Image.open("temp_fig.png")), fig)
        U.save_pic(img1, 3)
        U.save_pic(img1[0], "x", log_dir=str(tmp_path))
    finally:
        os.chdir(cwd)
    want = img1[0].mul(255).byte().permute(1, 2, 0).numpy()
    assert np.array_equal(np.array(Image.open(tmp_path / "3.png")), want) and np.array_equal(np.array(Image.open(tmp_path / "x.png")), want)
    with pytest.raises(RuntimeError, match="share a shape"):
        U.eval_depth_diff(img1, img2, None, disp1=disp1, disp2=disp2[..., :5])
