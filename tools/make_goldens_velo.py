"""Writes tests/golden/velo_depth.npz and the data-only tree tests/golden/kitti_velo_tree/ (tests/velo_ref.py has their layout).

    python tools/make_goldens_velo.py [--reference DIR]

Needs the reference tree: its own ``generate_depth_map`` (MD2/kitti_utils.py:46-98) runs on the made-up calibrations and seeded
clouds of tests/velo_ref.py, for both cameras and both ``vel_depth`` values, and its float64 result is cast to float32 as its
callers cast it (mono_dataset.py:365, export_gt_depth.py:55).  Stand-in: ``np.int = int`` (NumPy 1.24 removed the alias the
function uses).  ``<key>_proj_<cam>`` is P_velo2im as the function forms it (:50-62: ``read_calib_file`` and two ``np.dot``).

If a regenerated fixture disagrees with ops.velo_depth_map_host in float32 (BLAS's summation order inside ``np.dot`` differs from
the kernel's fixed order in the last bits of float64), change the seed in tests/velo_ref.py; do not loosen the test.

A tool: not run by the tests.
"""
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as mg      # noqa: E402
from tests import velo_ref as V            # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "velo_depth.npz")


def write_calib(calib_dir, hw, exact):
    os.makedirs(calib_dir, exist_ok=True)
    cam, velo = V.calib_texts(hw, exact)
    with open(os.path.join(calib_dir, "calib_cam_to_cam.txt"), "w") as f:
        f.write(cam)
    with open(os.path.join(calib_dir, "calib_velo_to_cam.txt"), "w") as f:
        f.write(velo)


def projection(ku, calib_dir, cam):
    cam2cam = ku.read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    velo2cam = ku.read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    velo2cam = np.hstack((velo2cam["R"].reshape(3, 3), velo2cam["T"][..., np.newaxis]))
    velo2cam = np.vstack((velo2cam, np.array([0, 0, 0, 1.0])))
    R_cam2rect = np.eye(4)
    R_cam2rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    P_rect = cam2cam["P_rect_0" + str(cam)].reshape(3, 4)
    return np.dot(np.dot(P_rect, R_cam2rect), velo2cam)


def record(out, ku, key, calib_dir, velo_file, hw):
    out[key + "_shape"] = np.array(hw, dtype=np.int32)
    for cam in V.CAMS:
        out["%s_proj_%d" % (key, cam)] = projection(ku, calib_dir, cam)
        for vd in V.VEL_DEPTHS:
            with np.errstate(all="ignore"):
                m = ku.generate_depth_map(calib_dir, velo_file, cam, vd)
            assert m.shape == tuple(hw), (m.shape, hw)
            out["%s_map_%d_%d" % (key, cam, int(vd))] = m.astype(np.float32)


def main():
    argv = list(sys.argv)
    ref_dir = argv[argv.index("--reference") + 1] if "--reference" in argv else mg.REF
    sys.path.insert(0, os.path.join(ref_dir, "DepthNetworks", "monodepth2"))
    if not hasattr(np, "int"):
        np.int = int
    import kitti_utils as ku
    out = {"stand_ins": np.array(["np.int = int"])}
    with tempfile.TemporaryDirectory() as tmp:
        for name, hw, n, exact in V.SMALL_CASES:
            calib_dir = os.path.join(tmp, name)
            write_calib(calib_dir, hw, exact)
            pts = V.cloud(name, hw, n, exact)
            velo_file = os.path.join(calib_dir, "cloud.bin")
            pts.tofile(velo_file)
            out["case_%s_points" % name] = pts
            record(out, ku, "case_" + name, calib_dir, velo_file, hw)
    for li, folder, frame, hw in V.tree_cases():
        write_calib(V.tree_calib_dir(folder), hw, False)
        path = V.tree_velo_path(folder, frame)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        V.cloud("%s/%d" % (folder, frame), hw, V.TREE_POINTS).tofile(path)
        record(out, ku, "line_%d" % li, V.tree_calib_dir(folder), path, hw)
    np.savez_compressed(OUT, **out)
    print("wrote %s %.1f KiB, %d arrays" % (OUT, os.path.getsize(OUT) / 1024.0, len(out)))


if __name__ == "__main__":
    main()
