"""What tools/make_goldens_velo.py and the K32 tests must agree on: the made-up calibrations and seeded point clouds of the
velodyne cases, the layout of the data-only tree tests/golden/kitti_velo_tree (calibration files and scans for the frames of
kitti_ref.SPLIT_LINES; no images, tests/golden/kitti_tree has those and must stay without scans), and the keys of
tests/golden/velo_depth.npz."""
import hashlib
import os

import numpy as np

from tests import kitti_ref as R

REPO = R.REPO
TREE = os.path.join(REPO, "tests", "golden", "kitti_velo_tree")
CAMS, VEL_DEPTHS = (2, 3), (False, True)
TREE_POINTS = 3000
# (name, (H, W), points, exact): the smallest images at which each rule can go wrong -- nearly every hit pixel is a duplicate and
# several edge pairs are occupied.  ``exact``: a calibration of exact axes (camera depth == x, focal length a power of two), so that
# a point at the origin has camera depth exactly 0 and chosen points land exactly on rounding ties.
SMALL_CASES = [("tiny_even", (12, 40), 3000, False), ("tiny_odd", (9, 17), 2000, True)]

# KITTI's published calibration of 2011_09_26 (rotations only; the intrinsics are scaled to the image)
R_RECT = [9.999239e-01, 9.837760e-03, -7.445048e-03, -9.869795e-03, 9.999421e-01, -4.278459e-03, 7.402527e-03, 4.351614e-03, 9.999631e-01]
R_VELO = [7.533745e-03, -9.999714e-01, -6.166020e-04, 1.480249e-02, 7.280733e-04, -9.998902e-01, 9.998621e-01, 7.523790e-03, 1.480755e-02]
T_VELO = [-4.069766e-03, -7.631618e-02, -2.717806e-01]


def _row(values):
    return " ".join("%.6e" % v for v in values)


def intrinsics(hw, exact):
    H, W = hw
    if exact:
        return 8.0, W / 2.0, H / 2.0
    return 0.58 * W, W / 2.0 + 0.3, H / 2.0 - 0.2


def calib_texts(hw, exact=False):
    """(calib_cam_to_cam.txt, calib_velo_to_cam.txt) of a made-up rig whose rectified image is hw."""
    H, W = hw
    f, cx, cy = intrinsics(hw, exact)
    tz = 0.0 if exact else 2.745884e-03
    p2 = [f, 0, cx, 0.0 if exact else 0.0622 * f, 0, f, cy, 0.0 if exact else 2.9e-04 * f, 0, 0, 1, tz]
    p3 = [f, 0, cx, -0.4709 * f, 0, f, cy, 0.0 if exact else 3.4e-03 * f, 0, 0, 1, 0.0 if exact else 4.981016e-03]
    r_rect = [1, 0, 0, 0, 1, 0, 0, 0, 1] if exact else R_RECT
    r_velo = [0, -1, 0, 0, 0, -1, 1, 0, 0] if exact else R_VELO
    t_velo = [0, -0.0625, 0] if exact else T_VELO
    cam = "\n".join(["calib_time: 09-Jan-2012 13:57:47", "corner_dist: 9.950000e-02", "S_rect_02: " + _row([W, H]),
                     "R_rect_00: " + _row(r_rect), "P_rect_02: " + _row(p2), "S_rect_03: " + _row([W, H]), "P_rect_03: " + _row(p3)]) + "\n"
    velo = "\n".join(["calib_time: 15-Mar-2012 11:37:16", "R: " + _row(r_velo), "T: " + _row(t_velo), "delta_f: 0.000000e+00 0.000000e+00"]) + "\n"
    return cam, velo


def cloud(name, hw, n, exact=False):
    """float32 [n, 4]: points aimed at the image and a margin of three pixels around it, behind them the rows every rule needs."""
    H, W = hw
    f, cx, cy = intrinsics(hw, exact)
    rng = np.random.RandomState(int(hashlib.sha256(("velo/" + name).encode()).hexdigest()[:8], 16))
    d = rng.uniform(1.5, 60.0, n)
    u, v = rng.uniform(-3.0, W + 4.0, n), rng.uniform(-3.0, H + 4.0, n)
    pts = np.stack([d, -(u - cx) * d / f, -(v - cy) * d / f, rng.uniform(0, 1, n)], 1).astype(np.float32)
    k = n // 25
    pts[0:k, 0] *= -1.0                                   # behind the scanner: x < 0
    pts[k:2 * k, 0] = 0.0                                 # x == 0 passes x >= 0; its camera depth is negative or zero
    pts[2 * k] = [np.nan, 1.0, 1.0, 0.0]                  # a NaN fails x >= 0
    pts[2 * k + 1] = [5.0, np.nan, 0.1, 0.0]              # kept by x >= 0; its projection is NaN
    pts[2 * k + 2] = [0.0, 0.0, 0.0, 0.0]                 # the origin: camera depth exactly 0 under the exact calibration
    pts[2 * k + 3] = [np.inf, 0.0, 0.0, 0.0]
    if exact:
        # q0 / q2 = (cx x - f y) / x: 9.5 and 8.5 at W = 17 -- half to even gives u = 9 and 7, half away from zero 9 and 8
        pts[2 * k + 4] = [2.0, -0.25, 0.125, 0.0]
        pts[2 * k + 5] = [2.0, 0.0, 0.125, 0.0]
    return pts


def tree_cases():
    """(line index, folder, frame, (H, W)) of the frames the tree holds scans for."""
    shapes = dict(R.DRIVES)
    return [(li, ln.split()[0], int(ln.split()[1]), shapes[ln.split()[0]]) for li, ln in enumerate(R.SPLIT_LINES)]


def tree_calib_dir(folder):
    return os.path.join(TREE, folder.split("/")[0])


def tree_velo_path(folder, frame):
    return os.path.join(TREE, folder, "velodyne_points", "data", "%010d.bin" % frame)


def all_cases(g):
    """name -> (points float32 [n, 4], (H, W), {cam: proj}, {(cam, vel_depth): the reference's float32 map}) from the golden ``g``:
    the small cases' points lie in the golden, the tree's in its .bin files."""
    out = {}
    names = [("case_" + nm, None) for nm, _, _, _ in SMALL_CASES] + [("line_%d" % li, (folder, frame)) for li, folder, frame, _ in tree_cases()]
    for key, where in names:
        pts = g[key + "_points"] if where is None else np.fromfile(tree_velo_path(*where), dtype=np.float32).reshape(-1, 4)
        hw = tuple(int(v) for v in g[key + "_shape"])
        out[key] = (pts, hw, {c: g["%s_proj_%d" % (key, c)] for c in CAMS},
                    {(c, vd): g["%s_map_%d_%d" % (key, c, int(vd))] for c in CAMS for vd in VEL_DEPTHS})
    return out
