"""K39 on the host: ``ops.pseudo_lidar_host`` (the definition the kernel is held to, and the path CPU tensors take) against a
per-pixel loop in Python floats and against the reference's own clouds (tests/golden/pseudo_lidar.npz, tools/make_goldens_lidar.py),
bit for bit; the calibration parse; the file form of ``python -m depthmodelhardening_amd.generate_lidar``.  No GPU."""
import os

import numpy as np
import pytest
import torch

from depthmodelhardening_amd import ops
from tests import eigen_eval_ref as E
from tests import lidar_ref as L


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(L.GOLDEN))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_wiring():
    from depthmodelhardening_amd import _native as N, build, library
    assert "dmh_pseudo_lidar" in N.EXPORTS and "pseudo_lidar.hip" in build.SOURCES
    assert "pseudo_lidar" in library.OPS and hasattr(torch.ops.dmh, "pseudo_lidar")
    assert N.LIDAR_TILE % 256 == 0 and N.LIDAR_CALIB == 27


@pytest.mark.parametrize("case", L.GOLDEN_CASES, ids=[c[0] for c in L.GOLDEN_CASES])
def test_host_equals_the_reference_and_the_loop(golden, case):
    name, form, hw, kind, max_high, _ = case
    m, cal = L.case_map(case), ops.lidar_calib(L.calib_text(kind, hw))
    pts, off = ops.pseudo_lidar_host(m.reshape(-1), form, [hw], cal[None], max_high)
    assert pts.dtype == np.float32 and off.dtype == np.int64 and off.tolist() == [0, pts.shape[0]]
    assert _same(pts, golden[name + "_cloud"])                              # the reference's np.dot chain, after its float32 cast
    assert _same(pts, L.frame_loop(form, m, cal, hw[0], hw[1], max_high))    # Python floats, one pixel at a time
    assert (pts[:, 3] == 1).all()


def test_the_goldens_cover_the_edge_cases(golden):
    assert golden["depth_5x7_none_cloud"].shape == (0, 4) and golden["depth_37x124_all_cloud"].shape == (37 * 124, 4)
    m = L.disp_map("disp_37x124_rot_mh3", (37, 124))
    assert (m == 0).sum() > 100 and (m < 0).sum() > 100
    assert 0 < golden["disp_37x124_rot_mh3_cloud"].shape[0] < (m > 0).sum()


def test_lidar_calib_equals_the_reference_and_crop_moves_the_principal_point(golden, tmp_path):
    from depthmodelhardening_amd.datasets.kitti_object import Calibration
    for name, _, hw, kind, _, _ in L.GOLDEN_CASES:
        text = L.calib_text(kind, hw)
        cal = ops.lidar_calib(text)
        assert cal.dtype == np.float64 and cal.shape == (27,) and np.array_equal(cal, golden[name + "_calib"])
    path = tmp_path / "000001.txt"
    path.write_text(text)
    assert np.array_equal(ops.lidar_calib(str(path)), cal) and np.array_equal(ops.lidar_calib(path), cal)
    shifted = ops.lidar_calib(text, crop=(3, 11))
    want = cal.copy()
    want[2] -= 3.0
    want[3] -= 11.0
    assert np.array_equal(shifted, want)
    c = Calibration(text)
    assert np.array_equal(c.C2V[:, :3], c.V2C[:, :3].T) and c.P.shape == (3, 4) and c.R0.shape == (3, 3)
    with pytest.raises(RuntimeError, match="no calibration file"):
        ops.lidar_calib(str(tmp_path / "missing.txt"))
    with pytest.raises(RuntimeError, match="R0_rect"):
        ops.lidar_calib("P2: " + " ".join(["1"] * 12) + "\nTr_velo_to_cam: " + " ".join(["1"] * 12) + "\n")


def test_rows_keep_the_row_major_pixel_order():
    """An identity-like rig: velodyne y = -camera x and z = -camera y, so within a frame kept at constant depth the rows must
    come out row by row (z falling), and left to right inside a row (y falling)."""
    hw = (6, 9)
    cal = ops.lidar_calib(L.calib_text("identity", hw))
    pts, _ = ops.pseudo_lidar_host(np.full(54, 4.0, dtype=np.float32), "depth", [hw], cal[None], max_high=100)
    assert pts.shape == (54, 4)
    grid = pts.reshape(6, 9, 4)
    assert (np.diff(grid[:, :, 1], axis=1) < 0).all() and (np.diff(grid[:, :, 2], axis=0) < 0).all()
    assert np.ptp(grid[:, :, 2], axis=1).max() == 0 and np.ptp(grid[:, :, 1], axis=0).max() == 0


@pytest.mark.parametrize("quantise", [False, True])
def test_net_form_is_the_resize_of_the_scaled_disparity(quantise):
    from depthmodelhardening_amd.layers import disp_to_depth
    disp = L.net_map("net/a", (12, 40))
    H, W = 17, 53
    scaled = disp_to_depth(torch.from_numpy(disp), 0.1, 100)[0].numpy()
    assert scaled.dtype == np.float32
    resized = E.resize(scaled, H, W, dtype=np.float32)                       # K25's arithmetic, fp32 products and sums
    with np.errstate(all="ignore"):
        depth = np.clip((np.float32(1) / resized) * np.float32(5.4), np.float32(1e-3), np.float32(80))
        if quantise:
            depth = (depth * np.float32(256)).astype(np.uint16).astype(np.float32) / np.float32(256)
    got = ops.lidar_net_depth_host(disp, H, W, quantise)
    assert _same(got, depth.astype(np.float32))
    assert _same(got, L.net_depth_loop(disp, H, W, quantise))
    cal = ops.lidar_calib(L.calib_text("rotated", (H, W)))
    pts, off = ops.pseudo_lidar_host(disp[None], "net", [(H, W)], cal[None], 3, quantise)
    want, _ = ops.pseudo_lidar_host(got.reshape(-1), "depth", [(H, W)], cal[None], 3)
    assert _same(pts, want) and _same(pts, L.frame_loop("depth", got, cal, H, W, 3)) and 0 < off[-1] < H * W


def test_batches_offsets_and_the_cpu_tensor_path(golden):
    cases = [c for c in L.GOLDEN_CASES if c[1] == "depth" and c[4] == 1][:4]
    maps = [L.case_map(c) for c in cases]
    cal = np.stack([golden[c[0] + "_calib"] for c in cases])
    shapes = [c[2] for c in cases]
    flat = np.concatenate([np.full(3, np.nan, dtype=np.float32)] + [np.concatenate([m.reshape(-1), [np.float32(7)]]) for m in maps])
    starts = [3 + sum(h * w + 1 for h, w in shapes[:i]) for i in range(len(shapes))]
    out = ops.pseudo_lidar(torch.from_numpy(flat), "depth", shapes, torch.from_numpy(cal), 1, offsets=starts)
    off = out.offsets.numpy()
    assert out.points.shape == (sum(h * w for h, w in shapes), 4) and out.offsets.dtype == torch.int64
    for i, c in enumerate(cases):
        assert _same(out.points[off[i]:off[i + 1]].numpy(), golden[c[0] + "_cloud"])
    assert [c.shape[0] for c in ops.lidar_clouds(out)] == np.diff(off).tolist()
    # a frame without pixels between two others
    packed = np.concatenate([maps[0].reshape(-1), maps[1].reshape(-1)])
    pts, off = ops.pseudo_lidar_host(packed, "depth", [shapes[0], (0, 5), shapes[1]], cal[[0, 0, 1]], 1)
    assert off[1] == off[2] and _same(pts, np.concatenate([golden[cases[0][0] + "_cloud"], golden[cases[1][0] + "_cloud"]]))


def test_errors():
    cal = torch.from_numpy(ops.lidar_calib(L.calib_text("rotated", (5, 7))))[None]
    m = torch.zeros(35)
    with pytest.raises(RuntimeError, match="form must be"):
        ops.pseudo_lidar(m, "points", [(5, 7)], cal)
    with pytest.raises(RuntimeError, match="float32"):
        ops.pseudo_lidar(m.double(), "depth", [(5, 7)], cal)
    with pytest.raises(RuntimeError, match="shapes must be"):
        ops.pseudo_lidar(m, "depth", [(5, -7)], cal)
    with pytest.raises(RuntimeError, match="shapes must be"):
        ops.pseudo_lidar(torch.zeros(2, 4, 4), "net", [(5, 7)], torch.cat([cal, cal]))
    with pytest.raises(RuntimeError, match="packed flat"):
        ops.pseudo_lidar(m.view(5, 7), "depth", [(5, 7)], cal)
    with pytest.raises(RuntimeError, match="offsets must place"):
        ops.pseudo_lidar(m, "depth", [(5, 8)], cal)
    with pytest.raises(RuntimeError, match="offsets must place"):
        ops.pseudo_lidar(m, "disp", [(5, 7)], cal, offsets=[1])
    with pytest.raises(RuntimeError, match="offsets must place"):
        ops.pseudo_lidar(m, "disp", [(5, 7)], cal, offsets=[-1])
    with pytest.raises(RuntimeError, match="offsets belong"):
        ops.pseudo_lidar(torch.zeros(1, 4, 4), "net", [(5, 7)], cal, offsets=[0])
    with pytest.raises(RuntimeError, match="calib must be"):
        ops.pseudo_lidar(m, "depth", [(5, 7)], cal.float())
    with pytest.raises(RuntimeError, match="calib must be"):
        ops.pseudo_lidar(m, "depth", [(5, 7)], cal[:, :26])
    with pytest.raises(RuntimeError, match="quantise"):
        ops.pseudo_lidar(m, "depth", [(5, 7)], cal, quantise=True)
    with pytest.raises(RuntimeError, match="share a device"):
        ops.pseudo_lidar(m, "depth", [(5, 7)], cal.to("meta"))
    with pytest.raises(RuntimeError, match="CUDA"):
        torch.ops.dmh.pseudo_lidar(m, "depth", [5, 7], cal)


def test_entry_point_rejects_bad_arguments_without_gpu():
    """Host-side argument checks of dmh_pseudo_lidar: every call fails before any launch."""
    import ctypes
    from depthmodelhardening_amd import _native as N
    lib, one, odd = N.lib(), ctypes.c_void_p(64), ctypes.c_void_p(68)

    def call(src_len=35, form=N.LIDAR_DEPTH, h=0, w=0, quantise=0, n=1, n_tiles=1, max_high=1.0, cap=35, out=one, calib=one):
        return lib.dmh_pseudo_lidar(one, src_len, form, h, w, quantise, calib, one, one, n, n_tiles, max_high, one, out, cap, one, None)
    assert call(form=7) != 0 and b"form" in lib.dmh_last_error()
    assert call(calib=None) != 0 and b"null pointer" in lib.dmh_last_error()
    assert call(n=0) != 0 and call(n_tiles=-1) != 0
    assert call(cap=N.LIDAR_TILE + 1) != 0 and b"cap" in lib.dmh_last_error()
    assert call(src_len=2 ** 31) != 0
    assert call(form=N.LIDAR_NET, h=5, w=8) != 0 and b"n h w" in lib.dmh_last_error()
    assert call(quantise=1) != 0 and call(h=5, w=7) != 0
    assert call(max_high=float("nan")) != 0
    assert call(out=odd) != 0 and b"aligned" in lib.dmh_last_error()
    assert call(out=None) != 0


@pytest.mark.parametrize("is_depth", [False, True])
def test_command_line_file_form(golden, tmp_path, is_depth):
    """One .npy and one 16-bit .png, as a user runs it: the .bin files are the reference's clouds for those files."""
    from PIL import Image
    from depthmodelhardening_amd import generate_lidar as G
    calib_dir, maps_dir = L.write_cli_tree(tmp_path, is_depth)
    with Image.open(os.path.join(maps_dir, L.CLI_FILES[1])) as img:
        assert img.mode.startswith("I;16")
    (tmp_path / "maps" / "notes.txt").write_text("not a map")
    save = tmp_path / "out" / "velodyne"

    def argv(batch):
        return ["--calib_dir", calib_dir, "--disparity_dir", maps_dir, "--save_dir", str(save), "--max_high", str(L.CLI_MAX_HIGH),
                "--batch_size", str(batch)] + (["--is_depth"] if is_depth else [])
    written = G.main(argv(2))
    assert [os.path.basename(p) for p in written] == [fn[:-4] + ".bin" for fn in L.CLI_FILES]
    assert sorted(os.listdir(save)) == [fn[:-4] + ".bin" for fn in L.CLI_FILES]
    for fn in L.CLI_FILES:
        got = np.fromfile(save / (fn[:-4] + ".bin"), dtype=np.float32).reshape(-1, 4)
        assert got.shape[0] > 100 and _same(got, golden["cli_%d_%s" % (int(is_depth), fn[:-4])])
    assert G.main(argv(1)) == written                       # one file per launch: the same bytes
    for fn in L.CLI_FILES:
        got = np.fromfile(save / (fn[:-4] + ".bin"), dtype=np.float32).reshape(-1, 4)
        assert _same(got, golden["cli_%d_%s" % (int(is_depth), fn[:-4])])
