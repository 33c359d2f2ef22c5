"""What the velodyne ground truth costs, for 32 frames of about 120 k points at 375 x 1242 (writes profiles/velo_depth.txt).

    python tools/velo_depth_bench.py [--batch 32] [--points 120000] [--steps 6] [--out profiles/velo_depth.txt] [--no_train]

Calibration and clouds are made up and seeded (tests/velo_ref.py); nothing is read from the reference tree.  Reported:
  1. K32 alone (HIP events): the loader's form (375 x 1242, half of the frames flipped) and the export's (own sizes, vel_depth);
  2. the numpy restatement ``ops.velo_depth_map_host``, one thread, per frame;
  3. a loop-form restatement -- projection and scatter in numpy, then a Python loop over the duplicate keys, which is how the
     reference resolves them -- per frame on one thread, and the 32 frames on 16 threads;
  4. reading and uploading the scans of one batch (the prefetcher's own work, 16 threads);
  5. a train step with --dataset kitti on the same tree without and with the velodyne files: wall time per step, the step with the
     loader's output held fixed, the main thread's waits.
Needs PIL and a GPU.
"""
import argparse
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import kitti_loader_bench as LB                                             # noqa: E402
from depthmodelhardening_amd import ops                                      # noqa: E402
from depthmodelhardening_amd.datasets import kitti as K                      # noqa: E402
from depthmodelhardening_amd.datasets import kitti_velo as KV                # noqa: E402
from tests import velo_ref as V                                              # noqa: E402

HW = (375, 1242)


def loop_form(pts, P, hw, vel_depth=False):
    """The map by the reference's method: a Python loop over the keys that occur more than once."""
    H, W = hw
    pts = pts[pts[:, 0] >= 0]
    x, y, z = (pts[:, c].astype(np.float64) for c in range(3))
    with np.errstate(all="ignore"):
        q = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]
        u, v = np.rint(q[0] / q[2]) - 1, np.rint(q[1] / q[2]) - 1
    ok = (u >= 0) & (v >= 0) & (u < W) & (v < H)
    u, v, d = u[ok].astype(np.int64), v[ok].astype(np.int64), (x if vel_depth else q[2])[ok]
    depth = np.zeros(hw)
    depth[v, u] = d
    keys = v * (W - 1) + u - 1
    uniq, counts = np.unique(keys, return_counts=True)
    for key in uniq[counts > 1]:
        members = np.nonzero(keys == key)[0]
        depth[v[members[0]], u[members[0]]] = d[members].min()
    depth[depth < 0] = 0
    return depth.astype(np.float32)


def add_velodyne(root, n, points):
    date = LB.DRIVE.split("/")[0]
    cam, velo = V.calib_texts(HW)
    with open(os.path.join(root, date, "calib_cam_to_cam.txt"), "w") as f:
        f.write(cam)
    with open(os.path.join(root, date, "calib_velo_to_cam.txt"), "w") as f:
        f.write(velo)
    os.makedirs(os.path.join(root, LB.DRIVE, "velodyne_points", "data"))
    for i in range(n):
        V.cloud("bench/%d" % i, HW, points + 997 * (i % 5)).tofile(KV.velo_path(root, LB.DRIVE, i))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "velo_depth.txt"))
    ap.add_argument("--no_train", action="store_true")
    a = ap.parse_args()
    dev, B = torch.device("cuda"), a.batch
    root = tempfile.mkdtemp(prefix="velo_bench_")
    lines = []
    try:
        LB.make_tree(root, B)
        common = ["--frame_ids", "0", "--use_stereo", "--height", str(LB.H), "--width", str(LB.W), "--batch_size", str(B), "--weights_init",
                  "scratch", "--log_dir", os.path.join(root, "log"), "--adv_train", "--norm_type", "l_inf", "--atk_batch_size", "12",
                  "--num_workers", "16", "--dataset", "kitti", "--data_path", root, "--png", "--split_dir", os.path.join(root, "splits"),
                  "--scene_root", os.path.join(root, "scenes")]
        if not a.no_train:
            r = LB.step_times(common, a.steps)
            lines.append("5. train step, batch %d, no velodyne files (the parent commit's step): wall %.1f ms / step; loader's output held fixed "
                         "%.1f ms; waiting for the prefetched batch %.1f ms / step; next_batch on the device %.2f ms"
                         % (B, r["wall"], r["held"], r["take_wait"], r["batch_ms"]))
        add_velodyne(root, B, a.points)
        P, hw = KV.velo_projection(KV.calib_dir(root, LB.DRIVE), 2)
        clouds = [np.fromfile(KV.velo_path(root, LB.DRIVE, i), dtype=np.float32).reshape(-1, 4) for i in range(B)]
        offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
        pts_d, off_d = torch.from_numpy(np.concatenate(clouds)).to(dev), torch.from_numpy(offsets).to(dev)
        proj_d = torch.from_numpy(np.stack([P] * B)).to(dev)
        flip_d = torch.tensor([i % 2 for i in range(B)], dtype=torch.int32, device=dev)
        first = ops.velo_depth_map_host(clouds[0], [0, len(clouds[0])], P[None], [hw])[0]
        got = ops.velo_depth_map(pts_d, off_d, proj_d, [hw] * B, False, HW)[0].cpu().numpy()
        assert np.array_equal(got, first) and np.array_equal(loop_form(clouds[0], P, hw), first)
        hits = int((first > 0).sum())
        lines.append("0. %d frames of %d .. %d points at %d x %d; frame 0: %d hit pixels; kernel, restatement and loop form agree on it"
                     % (B, min(map(len, clouds)), max(map(len, clouds)), hw[0], hw[1], hits))
        lines.append("1. K32, loader's form (375 x 1242, half flipped), 3 launches: %.3f ms; export's form (own sizes, vel_depth): %.3f ms"
                     % (LB.gpu_ms(lambda: ops.velo_depth_map(pts_d, off_d, proj_d, [hw] * B, False, HW, flip_d)),
                        LB.gpu_ms(lambda: ops.velo_depth_map(pts_d, off_d, proj_d, [hw] * B, True))))
        t0 = time.perf_counter()
        for c in clouds[:4]:
            ops.velo_depth_map_host(c, [0, len(c)], P[None], [hw])
        t_host = (time.perf_counter() - t0) / 4
        t0 = time.perf_counter()
        for c in clouds[:2]:
            loop_form(c, P, hw)
        t_loop = (time.perf_counter() - t0) / 2
        with ThreadPoolExecutor(16) as ex:
            t0 = time.perf_counter()
            list(ex.map(lambda c: loop_form(c, P, hw), clouds))
            t_loop16 = time.perf_counter() - t0
            t0 = time.perf_counter()
            list(ex.map(lambda c: ops.velo_depth_map_host(c, [0, len(c)], P[None], [hw]), clouds))
            t_host16 = time.perf_counter() - t0
        lines.append("2. numpy restatement, one thread: %.1f ms / frame; the %d frames on 16 threads: %.1f ms" % (t_host * 1e3, B, t_host16 * 1e3))
        lines.append("3. loop form, one thread: %.1f ms / frame; the %d frames on 16 threads: %.1f ms" % (t_loop * 1e3, B, t_loop16 * 1e3))
        split = K.read_split(os.path.join(root, "splits", "eigen_zhou", "train_files.txt"))
        ds = K.KITTIRAWDataset(root, split, LB.H, LB.W, [0], 4, dev, is_train=True, img_ext=".png", num_workers=16)
        pre = K._Prefetcher(B, dev, 16)
        for k in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pre._load_clouds(k % 2, [ds.velo_path(i) for i in range(B)])
            t1 = time.perf_counter()
        pre.close()
        ds.close()
        lines.append("4. reading the %d scans into the pinned buffer (%.1f MB, np.fromfile, 16 threads): %.1f ms"
                     % (B, offsets[-1] * 16 / 1e6, (t1 - t0) * 1e3))
        if not a.no_train:
            r = LB.step_times(common, a.steps)
            lines.append("5. train step, batch %d, with velodyne files (depth_gt built every step):  wall %.1f ms / step; loader's output held fixed "
                         "%.1f ms; waiting for the prefetched batch %.1f ms / step; next_batch on the device %.2f ms"
                         % (B, r["wall"], r["held"], r["take_wait"], r["batch_ms"]))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/velo_depth_bench.py, batch %d, %d points\n" % (B, a.points) + text)


if __name__ == "__main__":
    main()
