"""Writes tests/golden/pose_ate.npz (tests/pose_eval_ref.py has its cases, keys and gate).

    python tools/make_goldens_pose_eval.py [--reference DIR]

The reference's ``evaluate_pose`` module is imported the way tools/make_goldens_pose.py imports its siblings
(oracle/make_goldens.install_shims stands in for torchvision and the other packages the reference's ``datasets`` and ``networks``
pull in; nothing of the trajectory arithmetic is stubbed).  Per case it runs, on the made-up drives of tests/pose_eval_ref.py, the
reference's own expression for the local poses (MD2/evaluate_pose.py:104-114) and its own ``dump_xyz`` and ``compute_ate`` inside
its loop (:116-125), and beside them the same loop in ``np.longdouble`` -- the anchor -- and the distance between the two, e_ref.
It refuses to run where ``np.longdouble`` is not wider than float64.

Also stored: ``KITTIOdomDataset.get_image_path`` for the queries of tests/pose_eval_ref.PATH_QUERIES, and the line counts and
sha256 digests of the reference's ``splits/odom/test_files_09.txt`` / ``_10.txt`` -- after asserting once more that the two lists
are exactly what ``datasets.kitti_odom.odom_test_lines`` generates, which is why no list file ships with this repository.

Data only, well under 100 KB.  A tool: not run by the tests.
"""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as mg                                          # noqa: E402
from tests import pose_eval_ref as R                                           # noqa: E402
from depthmodelhardening_amd.datasets.kitti_odom import ODOM_TEST_PAIRS, odom_test_lines      # noqa: E402

ARGV = list(sys.argv)        # (install_shims resets sys.argv for the reference's option parser)


def reference_modules(ref_dir):
    mg.install_shims()
    from PIL import Image
    if not hasattr(Image, "ANTIALIAS"):     # removed in Pillow 10; LANCZOS is its later name (the dataset's constructor reads it)
        Image.ANTIALIAS = Image.LANCZOS
    md2 = os.path.join(ref_dir, "DepthNetworks", "monodepth2")
    sys.path.insert(0, ref_dir)         # (the reference's datasets import its torchattacks package from the tree's root)
    sys.path.insert(0, md2)
    import evaluate_pose
    from datasets import KITTIOdomDataset
    return evaluate_pose, KITTIOdomDataset, md2


def reference_run(E, pred, gt_global, track_length):
    """MD2/evaluate_pose.py:104-125 around the reference's own functions: (gt_local [N, 4, 4], ates [N], mean, std)."""
    g = np.concatenate((gt_global, np.zeros((gt_global.shape[0], 1, 4))), 1)
    g[:, 3, 3] = 1
    local = [np.linalg.inv(np.dot(np.linalg.inv(g[i - 1]), g[i])) for i in range(1, len(g))]
    ates = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(0, g.shape[0] - 1):
            local_xyzs = np.array(E.dump_xyz(pred[i:i + track_length - 1]))
            gt_local_xyzs = np.array(E.dump_xyz(local[i:i + track_length - 1]))
            ates.append(E.compute_ate(gt_local_xyzs, local_xyzs))
        return np.stack(local), np.array(ates, dtype=np.float64), float(np.mean(ates)), float(np.std(ates))


def main():
    if np.finfo(np.longdouble).nmant <= np.finfo(np.float64).nmant:
        raise SystemExit("np.longdouble is float64 here: the anchor needs a wider format")
    ref_dir = ARGV[ARGV.index("--reference") + 1] if "--reference" in ARGV else mg.REF
    E, KITTIOdomDataset, md2 = reference_modules(ref_dir)
    out = {}
    for name, n, _, _, track_lengths in R.CASES:
        gt_global, pred = R.make_case(name)
        assert np.array_equal(gt_global.astype(np.float32).astype(np.float64), gt_global)
        out[name + "_gt_global"], out[name + "_pred"] = gt_global.astype(np.float32), pred      # float32 values, stored as such
        for t in track_lengths:
            local, ates, mean, std = reference_run(E, pred, gt_global, t)
            a_ates, a_mean, a_std = R.anchor_run(pred, local, t)
            assert np.array_equal(np.isnan(ates), np.isnan(a_ates)), (name, t)
            tag = "%s_t%d_" % (name, t)
            out[tag + "ates"], out[tag + "mean"], out[tag + "std"] = ates, np.float64(mean), np.float64(std)
            out[tag + "anchor_ates"], out[tag + "anchor_mean"], out[tag + "anchor_std"] = a_ates, np.float64(a_mean), np.float64(a_std)
            out[tag + "e_ref"] = np.float64(R.run_distance(ates, mean, std, a_ates, a_mean, a_std))
            print("%-10s N %3d  mean %.6f std %.6f  NaN %d  e_ref %.3g" % (tag[:-1], n, mean, std, int(np.isnan(ates).sum()), out[tag + "e_ref"]))
        out[name + "_gt_local"] = local
        if name in R.LOCAL_CASES:
            out[name + "_anchor_local"] = R.anchor_local(gt_global)
            out[name + "_e_ref_local"] = np.float64(R.rel_dist_poses(local, out[name + "_anchor_local"]))
            print("%-10s local poses e_ref %.3g" % (name, out[name + "_e_ref_local"]))
    # the file names and the two lists
    paths = []
    for data_path, seq, frame, side, ext in R.PATH_QUERIES:
        ds = KITTIOdomDataset(data_path, ["%d 0 l" % seq], 192, 640, [0, 1], 4, is_train=False, img_ext=ext)
        paths.append(ds.get_image_path(seq, frame, side))
    out["paths"] = np.array(paths)
    counts, digests = [], []
    for seq in sorted(ODOM_TEST_PAIRS):
        with open(os.path.join(md2, "splits", "odom", "test_files_{:02d}.txt".format(seq))) as f:
            lines = f.read().splitlines()
        assert lines == odom_test_lines(seq, ODOM_TEST_PAIRS[seq]), "test_files_%02d.txt is not the generated list" % seq
        counts.append(len(lines))
        digests.append(hashlib.sha256("\n".join(lines).encode()).hexdigest())
    out["test_sequences"], out["test_counts"], out["test_digests"] = np.array(sorted(ODOM_TEST_PAIRS)), np.array(counts), np.array(digests)
    np.savez_compressed(R.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (R.GOLDEN, os.path.getsize(R.GOLDEN)))


if __name__ == "__main__":
    main()
