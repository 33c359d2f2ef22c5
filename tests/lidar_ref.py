"""What tools/make_goldens_lidar.py and the K39 tests must agree on: the made-up KITTI-object calibrations, the seeded maps of the
pseudo-LiDAR cases, the keys of tests/golden/pseudo_lidar.npz -- and the per-pixel loop reference in Python floats that
``ops.pseudo_lidar_host`` is held to."""
import hashlib
import math
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "pseudo_lidar.npz")

# KITTI's published calibration rotations (the intrinsics are scaled to the image)
R_RECT = [9.999239e-01, 9.837760e-03, -7.445048e-03, -9.869795e-03, 9.999421e-01, -4.278459e-03, 7.402527e-03, 4.351614e-03, 9.999631e-01]
TR_VELO = [7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03, 1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02,
           9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01]
CALIBS = ("rotated", "identity")


def _row(values):
    return " ".join("%.12e" % v for v in values)


def calib_text(kind, hw):
    """A KITTI-object calibration file for an image of ``hw``: "rotated" has KITTI's rectifying rotation and velodyne pose,
    "identity" an identity R0 and exact axes.  Lines the parser must skip are part of it."""
    H, W = hw
    f = 721.5377 * max(W, 8) / 1242.0
    cu, cv = 609.5593 * W / 1242.0, 172.854 * H / 375.0
    p2 = [f, 0, cu, 4.485728e+01 * f / 721.5377, 0, f, cv, 2.163791e-01 * f / 721.5377, 0, 0, 1, 2.745884e-03]
    if kind == "identity":
        r0, tr = [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, -1, 0, 0.0, 0, 0, -1, -0.08, 1, 0, 0, -0.27]
    else:
        r0, tr = R_RECT, TR_VELO
    return "\n".join(["calib_time: 09-Jan-2012 13:57:47", "P0: " + _row([f, 0, cu, 0, 0, f, cv, 0, 0, 0, 1, 0]), "P2: " + _row(p2), "",
                      "R0_rect: " + _row(r0), "Tr_velo_to_cam: " + _row(tr), "Tr_imu_to_velo: " + _row(range(12))]) + "\n"


def _rng(name):
    return np.random.RandomState(int(hashlib.sha256(("lidar/" + name).encode()).hexdigest()[:8], 16))


def depth_map(name, hw, kind="mixed"):
    """float32 [H, W] metric depth.  "mixed": 2 .. 70 m, so that rows above the horizon pass and fail max_high by their depth;
    "none": 40 .. 80 m on a frame that lies above the horizon at that range and a band behind the camera (nothing is kept);
    "all": 3 .. 6 m (everything is kept at max_high 3)."""
    H, W = hw
    rng = _rng(name)
    if kind == "all":
        return rng.uniform(3.0, 6.0, (H, W)).astype(np.float32)
    if kind == "none":
        m = rng.uniform(40.0, 80.0, (H, W))
        m[H // 2:] = -m[H // 2:]
        return m.astype(np.float32)
    return rng.uniform(2.0, 70.0, (H, W)).astype(np.float32)


def disp_map(name, hw):
    """float32 [H, W] disparity in pixels with exact zeros, negatives and sub-pixel values."""
    H, W = hw
    rng = _rng(name)
    m = rng.uniform(0.3, 96.0, (H, W))
    kind = rng.randint(0, 6, (H, W))
    m[kind == 0] = 0.0
    m[kind == 1] = -m[kind == 1]
    return m.astype(np.float32)


def net_map(name, hw):
    """float32 [h, w] in (0, 1): a sigmoid output, smooth with noise."""
    h, w = hw
    rng = _rng(name)
    yy, xx = np.mgrid[0:h, 0:w]
    z = 1.5 * np.sin(xx / 7.0) + 2.0 * (yy / max(h - 1, 1) - 0.5) + rng.normal(0, 0.7, (h, w))
    return (1.0 / (1.0 + np.exp(-z))).astype(np.float32)


# (name, form, (H, W), calibration, max_high, map kind): what tests/golden/pseudo_lidar.npz holds a reference cloud for
GOLDEN_CASES = [(("%s_%dx%d_%s_mh%d" % (form, hw[0], hw[1], cal[:3], mh)), form, hw, cal, mh, "mixed")
                for hw in ((5, 7), (1, 1)) for form in ("depth", "disp") for cal in CALIBS for mh in (1, 3)]
GOLDEN_CASES += [("depth_37x124_rot_mh1", "depth", (37, 124), "rotated", 1, "mixed"),
                 ("depth_37x124_ide_mh3", "depth", (37, 124), "identity", 3, "mixed"),
                 ("disp_37x124_rot_mh3", "disp", (37, 124), "rotated", 3, "mixed"),
                 ("disp_37x124_ide_mh1", "disp", (37, 124), "identity", 1, "mixed"),
                 ("depth_64x200_rot_mh1", "depth", (64, 200), "rotated", 1, "mixed"),
                 ("depth_5x7_none", "depth", (5, 7), "rotated", 1, "none"),
                 ("depth_37x124_all", "depth", (37, 124), "identity", 3, "all")]
# the file form of the command: (name, is_depth, (H, W), calibration, max_high); the inputs are ``cli_inputs``
CLI_SHAPE, CLI_CALIB, CLI_MAX_HIGH = (20, 50), "rotated", 1
CLI_FILES = ("000003.npy", "000007.png")


def case_map(case):
    name, form, hw, _, _, kind = case
    return depth_map(name, hw, kind) if form == "depth" else disp_map(name, hw)


def cli_inputs(is_depth):
    """{file name: array} of one run of the file form.  With --is_depth the files hold 256 x depth (float32 .npy, 16-bit .png);
    without it disparities in pixels (.npy with fractions and zeros, .png whole pixels below 256)."""
    rng = _rng("cli/%d" % int(is_depth))
    if is_depth:
        a = (rng.uniform(2.0, 70.0, CLI_SHAPE) * 256.0).astype(np.float32)
        b = (rng.uniform(2.0, 70.0, CLI_SHAPE) * 256.0).astype(np.uint16)
    else:
        a = rng.uniform(0.3, 96.0, CLI_SHAPE).astype(np.float32)
        a[rng.randint(0, 5, CLI_SHAPE) == 0] = 0.0
        b = rng.randint(0, 97, CLI_SHAPE).astype(np.uint16)
    return {CLI_FILES[0]: a, CLI_FILES[1]: b}


def write_cli_tree(root, is_depth):
    """<root>/calib/<name>.txt and <root>/maps/<name>.npy|png; returns (calib_dir, maps_dir)."""
    from PIL import Image
    calib_dir, maps_dir = os.path.join(str(root), "calib"), os.path.join(str(root), "maps")
    os.makedirs(calib_dir, exist_ok=True)
    os.makedirs(maps_dir, exist_ok=True)
    for fn, arr in cli_inputs(is_depth).items():
        with open(os.path.join(calib_dir, fn[:-4] + ".txt"), "w") as f:
            f.write(calib_text(CLI_CALIB, CLI_SHAPE))
        if fn.endswith(".npy"):
            np.save(os.path.join(maps_dir, fn), arr)
        else:
            Image.fromarray(arr).save(os.path.join(maps_dir, fn))      # a 16-bit greyscale PNG
    return calib_dir, maps_dir


# ------------------------------------------------------------------------------------------------- the loop reference
def _f32(x):
    return np.float32(x)


def net_depth_loop(disp, H, W, quantise):
    """The net form's depth, pixel by pixel: every fp32 operation rounded on its own (numpy float32 scalars)."""
    h, w = disp.shape
    out = np.zeros((H, W), dtype=np.float32)

    def axis(d, dst, src):
        ff = _f32((d + 0.5) * (float(src) / float(dst)) - 0.5)
        s = int(math.floor(float(ff)))
        ff = _f32(ff - _f32(s))
        if s < 0:
            s, ff = 0, _f32(0)
        if s >= src - 1:
            s, ff = src - 1, _f32(0)
        return s, min(s + 1, src - 1), ff

    def tap(y, x):
        return _f32(_f32(1.0 / 100.0) + _f32(_f32(1.0 / 0.1 - 1.0 / 100.0) * disp[y, x]))

    with np.errstate(all="ignore"):
        for y in range(H):
            ya, yb, fy = axis(y, H, h)
            for x in range(W):
                xa, xb, fx = axis(x, W, w)
                a0, a1, b0, b1 = _f32(_f32(1) - fx), fx, _f32(_f32(1) - fy), fy
                r0 = _f32(_f32(a0 * tap(ya, xa)) + _f32(a1 * tap(ya, xb)))
                r1 = _f32(_f32(a0 * tap(yb, xa)) + _f32(a1 * tap(yb, xb)))
                d = _f32(_f32(b0 * r0) + _f32(b1 * r1))
                depth = _f32(_f32(_f32(1) / d) * _f32(5.4))
                if depth < _f32(1e-3):
                    depth = _f32(1e-3)
                if depth > _f32(80):
                    depth = _f32(80)
                if quantise:
                    q = _f32(depth * _f32(256))
                    depth = _f32(_f32(0 if math.isnan(float(q)) else int(q) & 0xffff) / _f32(256))
                out[y, x] = depth
    return out


def frame_loop(form, m, cal, H, W, max_high):
    """One frame's kept rows, float32 [M, 4]: Python floats (IEEE double), one pixel at a time, in the stated association.
    ``m``: float32 [H, W], the depth or disparity map (the net form passes its depth as "depth")."""
    f_u, f_v, c_u, c_v, b_x, b_y = (float(v) for v in cal[:6])
    Ri = [[float(cal[6 + 3 * i + j]) for j in range(3)] for i in range(3)]
    Cm = [[float(cal[15 + 4 * i + j]) for j in range(4)] for i in range(3)]
    rows = []
    for v in range(H):
        for u in range(W):
            s = float(m[v, u])
            if form == "disp":
                if s < 0:
                    s = 0.0
                if not s > 0:
                    continue
                d = (f_u * 0.54) / ((s + 1.) - 1.0)
            else:
                d = s
            x = ((u - c_u) * d) / f_u + b_x
            y = ((v - c_v) * d) / f_v + b_y
            z = d
            r = [(Ri[i][0] * x + Ri[i][1] * y) + Ri[i][2] * z for i in range(3)]
            o = [((Cm[i][0] * r[0] + Cm[i][1] * r[1]) + Cm[i][2] * r[2]) + Cm[i][3] for i in range(3)]
            if o[0] >= 0 and o[2] < max_high:
                rows.append([o[0], o[1], o[2], 1.0])
    with np.errstate(all="ignore"):
        return np.array(rows, dtype=np.float64).reshape(-1, 4).astype(np.float32)
