"""The odometry evaluation's yardstick (K40, ``ops.pose_ate`` / ``ops.pose_ate_host`` / ``ops.gt_local_poses``): the cases of
tests/golden/pose_ate.npz, the float64 anchor and the gate.

The cases.  A made-up drive: per step a rotation from a small random axis-angle (|angle| about 0.02 rad) and a translation with a
forward motion of about 1 unit; the global poses ``gt_global`` [N + 1, 3, 4] chain the steps.  The predictions ``pred`` [N, 4, 4]
float32 are the ground truth's local poses with the translation scaled by 0.03 (a monocular network's scale is arbitrary) plus
noise of 1 % of a step, which puts the snippet errors at the order of 1e-2.  N in {1, 3, 4, 5, 37, 65, 257}: 1, 3, 4 and 5 are the
truncated snippets (the last snippets of every sequence have 4, 3, 2 and 1 poses), 65 and 257 step over a wave and a workgroup
of K40.  ``zero`` (N = 9): predictions 3 and 8 have an all-zero translation, so every snippet that consists of one of them alone
has sum(pred^2) = 0 and is NaN, as in numpy: snippet 8 at track_length 5, snippets 3 and 8 at track_length 2 (both are stored).

What the fixture holds per run ``<case>_t<track_length>`` (tools/make_goldens_pose_eval.py): the inputs (``<case>_gt_global``,
``<case>_pred``), the reference's own local poses (``<case>_gt_local``, MD2/evaluate_pose.py:104-114) and its own ``ates``, mean
and std (its ``dump_xyz`` / ``compute_ate`` and its loop :116-125 with that track_length); the ANCHOR: the same loop on the same
pred and gt_local carried out in ``np.longdouble`` (80-bit on the machine that wrote it) and rounded to float64 at the end; and
``e_ref``, the largest relative distance of the reference's ates, mean and std from the anchor's.  For the local poses the anchor
is a longdouble Gauss-Jordan inverse of the longdouble product, and ``<case>_e_ref_local`` the reference's distance from it
(the cases of ``LOCAL_CASES``: the fixture stays under 100 KB).  ``gt_global`` holds float32 values and is stored as float32.

The gate (the project's usual form, tests/test_gpu_l2.py): a result passes when its largest relative distance from the anchor is
at most 20 e_ref, with a floor of 4 x 2^-52 where e_ref is 0.  Bit equality with numpy cannot be the gate: numpy forms the 4x4
products through BLAS, and a float64 loop in index order differs from it in the last bit while both are equally far from the
anchor; the factor 20 covers a different ORDER of the same float64 operations, not a lower precision.  NaNs must sit at the
same indices, and mean and std must be NaN where the reference's are.  Distances: element-wise |x - a| / |a| for the errors and
the two statistics (all positive); for a 4x4 pose max|x - a| / max|a| over the matrix, since its bottom row holds exact zeros.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_ate.npz")
TRACK_LENGTH = 5
FLOOR = 4.0 * 2.0 ** -52
MARGIN = 20.0
PRED_SCALE = 0.03
NOISE = 0.01
# (name, N, seed, indices whose predicted translation is exactly zero, track lengths stored)
CASES = (("n1", 1, 1, (), (5,)), ("n3", 3, 3, (), (5,)), ("n4", 4, 4, (), (5,)), ("n5", 5, 5, (), (5,)), ("n37", 37, 37, (), (5,)),
         ("n65", 65, 65, (), (5,)), ("n257", 257, 257, (), (5,)), ("zero", 9, 9, (3, 8), (5, 2)))
LOCAL_CASES = tuple(c[0] for c in CASES if c[1] <= 9)       # the cases that also hold the anchor of the local poses (file size)
RUNS = tuple((c[0], t) for c in CASES for t in c[4])
RUN_IDS = ["%s_t%d" % r for r in RUNS]
# what odom_image_path / odom_test_lines are compared with: (data_path, sequence, frame, side, extension)
PATH_QUERIES = (("/data/odom", 9, 0, "l", ".jpg"), ("/data/odom", 10, 1199, "l", ".png"), ("odom", 9, 123456, "r", ".jpg"),
                ("/d", 3, 7, "2", ".png"), ("/d", 10, 42, "3", ".jpg"))


def _rot(axisangle):
    """Rodrigues' formula, float64."""
    a = np.asarray(axisangle, dtype=np.float64)
    angle = np.sqrt((a * a).sum())
    if angle == 0:
        return np.eye(3)
    n = a / angle
    K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def make_case(name):
    """(gt_global float64 [N + 1, 3, 4], pred float32 [N, 4, 4]) of case ``name``.  Used by the golden tool only: the tests read
    the inputs from the fixture, so a libm that rounds a sine differently cannot move them."""
    _, n, seed, zeros, _ = next(c for c in CASES if c[0] == name)
    rng = np.random.RandomState(1000 + seed)
    G = [np.eye(4)]
    pred = np.zeros((n, 4, 4), dtype=np.float64)
    for i in range(n):
        R = _rot(rng.normal(size=3) * 0.02)
        t = np.array([0.0, 0.0, 1.0]) + rng.normal(size=3) * np.array([0.05, 0.02, 0.2])
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = R, t
        G.append((G[-1] @ M).astype(np.float32).astype(np.float64))      # float32 values: the file stays small, a drive all the same
        # the local pose the reference forms is inv(M) = [R^T | -R^T t]; the prediction is a scaled, noisy copy of it
        Rn = _rot(rng.normal(size=3) * 0.002) @ R.T
        tn = PRED_SCALE * (-R.T @ t + rng.normal(size=3) * NOISE)
        pred[i] = np.eye(4)
        pred[i, :3, :3], pred[i, :3, 3] = Rn, (0.0 if i in zeros else tn)
    return np.stack(G)[:, :3, :].copy(), pred.astype(np.float32)


def inv_longdouble(m):
    """Gauss-Jordan with partial pivoting in np.longdouble."""
    n = m.shape[0]
    a = np.concatenate([np.array(m, dtype=np.longdouble), np.eye(n, dtype=np.longdouble)], 1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        if p != c:
            a[[c, p]] = a[[p, c]]
        a[c] = a[c] / a[c, c]
        for r in range(n):
            if r != c:
                a[r] = a[r] - a[r, c] * a[c]
    return a[:, n:]


def anchor_local(gt_global):
    """MD2/evaluate_pose.py:104-114 in longdouble, rounded to float64 at the end."""
    g = np.concatenate((np.asarray(gt_global, dtype=np.float64), np.zeros((len(gt_global), 1, 4))), 1)
    g[:, 3, 3] = 1
    g = g.astype(np.longdouble)
    return np.stack([inv_longdouble(np.dot(inv_longdouble(g[i - 1]), g[i])) for i in range(1, len(g))]).astype(np.float64)


def anchor_run(pred, gt_local, track_length):
    """The reference's loop (MD2/evaluate_pose.py:23-46, :116-125) in longdouble on float32 pred / float64 gt_local, rounded to
    float64 at the end: (ates [N], mean, std)."""
    ld = np.longdouble
    pred, gt = np.asarray(pred).astype(ld), np.asarray(gt_local).astype(ld)

    def dump_xyz(ts):
        c = np.eye(4, dtype=ld)
        out = [c[:3, 3]]
        for t in ts:
            c = np.dot(c, t)
            out.append(c[:3, 3])
        return np.array(out, dtype=ld)

    ates = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(len(pred)):
            p, g = dump_xyz(pred[i:i + track_length - 1]), dump_xyz(gt[i:i + track_length - 1])
            p = p + (g[0] - p[0])[None, :]
            scale = np.sum(g * p) / np.sum(p ** 2)
            ates.append(np.sqrt(np.sum((p * scale - g) ** 2)) / ld(g.shape[0]))
        ates = np.array(ates, dtype=ld)
        mean = np.sum(ates) / ld(len(ates))
        std = np.sqrt(np.sum((ates - mean) ** 2) / ld(len(ates)))
    return ates.astype(np.float64), float(mean), float(std)


def rel_dist(x, anchor):
    """Largest |x - a| / |a| over the entries where the anchor is a number; 0 for none.  The NaN pattern is checked apart."""
    x, a = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(anchor, dtype=np.float64))
    ok = ~np.isnan(a)
    if not ok.any():
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(x[ok] - a[ok]) / np.abs(a[ok])
    return float(np.max(d))


def rel_dist_poses(x, anchor):
    """Largest max|x - a| / max|a| over the 4x4 matrices."""
    x, a = np.asarray(x, dtype=np.float64), np.asarray(anchor, dtype=np.float64)
    return float(np.max(np.abs(x - a).reshape(len(a), -1).max(1) / np.abs(a).reshape(len(a), -1).max(1)))


def bound(e_ref):
    e_ref = float(e_ref)
    return MARGIN * e_ref if e_ref > 0 else FLOOR


def run_distance(ates, mean, std, anchor_ates, anchor_mean, anchor_std):
    """The distance of a run (errors and the two statistics) from the anchor."""
    return max(rel_dist(ates, anchor_ates), rel_dist(mean, anchor_mean), rel_dist(std, anchor_std))


def check_run(g, run, ates, mean, std, what):
    """A run (``ates`` float64 [N], ``mean``, ``std``) against the fixture ``g``: the NaN pattern is the reference's, the distance
    from the anchor is within the gate.  Returns (distance, e_ref) for printing."""
    tag = "%s_t%d_" % run
    ates = np.asarray(ates, dtype=np.float64)
    ref, anchor = g[tag + "ates"], g[tag + "anchor_ates"]
    assert ates.shape == ref.shape and ates.dtype == np.float64, (what, run, ates.shape, ates.dtype)
    assert np.array_equal(np.isnan(ates), np.isnan(ref)), (what, run, "NaN at other indices than the reference's")
    assert np.isnan(mean) == np.isnan(float(g[tag + "mean"])) and np.isnan(std) == np.isnan(float(g[tag + "std"])), (what, run, mean, std)
    e_ref = float(g[tag + "e_ref"])
    d = run_distance(ates, mean, std, anchor, float(g[tag + "anchor_mean"]), float(g[tag + "anchor_std"]))
    print("%-14s %-10s distance from the anchor %.3g  e_ref %.3g  bound %.3g" % (what, tag[:-1], d, e_ref, bound(e_ref)))
    assert d <= bound(e_ref), (what, run, d, e_ref)
    return d, e_ref
