"""The ground truth of the KITTI evaluation (MD2/export_gt_depth.py): ``gt_depths.npz``, which ``evaluate_depth`` reads through
``--eval_gt_path``.

    python -m depthmodelhardening_amd.export_gt_depth --data_path D --split_dir S --split eigen|eigen_benchmark [--out PATH]

``eigen``: the velodyne scans of <split_dir>/eigen/test_files.txt through K32 (``ops.velo_depth_map``) with camera 2 and
``vel_depth`` -- the reference's ``generate_depth_map(calib_dir, velo_filename, 2, True)`` -- each map at its frame's own size, in
batches.  ``eigen_benchmark``: the reference's PNG branch on the host, ``float32(png) / 256``.  The file is written as the
reference writes it, ``np.savez_compressed(path, data=np.array(maps, dtype=object))``; the default path is
<split_dir>/<split>/gt_depths.npz.  ``--device cpu`` runs the numpy restatement of K32 instead of the kernel (the same bits).
"""
import argparse
import os

import numpy as np
import torch

from . import ops
from .datasets import kitti_velo
from .datasets.kitti import read_split
from .my_utils import to_device_async

EXPORT_BATCH = 16


def velodyne_maps(data_path, lines, device, batch_size=EXPORT_BATCH):
    """float32 maps [H, W] of the split lines, at each frame's own size: camera 2, ``vel_depth`` (export_gt_depth.py:45-49)."""
    device = torch.device(device)
    maps = []
    for first in range(0, len(lines), batch_size):
        clouds, proj, shapes = [], [], []
        for line in lines[first:first + batch_size]:
            folder, frame_id = line.split()[:2]
            path = kitti_velo.velo_path(data_path, folder, int(frame_id))
            pts = np.empty((kitti_velo.cloud_points(path), 4), dtype=np.float32)
            kitti_velo.read_cloud_into(path, pts)
            P, hw = kitti_velo.velo_projection(kitti_velo.calib_dir(data_path, folder), 2)
            clouds.append(pts), proj.append(P), shapes.append(hw)
        offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
        flat, cell_off = ops.velo_depth_map(to_device_async(np.concatenate(clouds), device), to_device_async(offsets, device),
                                            to_device_async(np.stack(proj), device), shapes, vel_depth=True)
        flat = flat.cpu().numpy()
        maps.extend(flat[cell_off[i]:cell_off[i + 1]].reshape(hw).copy() for i, hw in enumerate(shapes))
    return maps


def benchmark_maps(data_path, lines):
    """export_gt_depth.py:50-53: the improved ground truth's 16-bit PNGs over 256."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("--split eigen_benchmark reads PNG files with PIL (Pillow), which is not installed: %s" % e)
    maps = []
    for line in lines:
        folder, frame_id = line.split()[:2]
        path = os.path.join(data_path, folder, "proj_depth", "groundtruth", "image_02", "{:010d}.png".format(int(frame_id)))
        with Image.open(path) as img:
            maps.append(np.array(img).astype(np.float32) / 256)
    return maps


def save_gt_depths(path, maps):
    data = np.empty(len(maps), dtype=object)        # np.array(maps, dtype=object) for maps of one size would be 3-D
    for i, m in enumerate(maps):
        data[i] = m.astype(np.float32)
    np.savez_compressed(path, data=data)


def main(argv=None):
    parser = argparse.ArgumentParser(description="export_gt_depth")
    parser.add_argument("--data_path", type=str, required=True, help="path to the root of the KITTI data")
    parser.add_argument("--split_dir", type=str, required=True, help="folder of Monodepth2's split lists")
    parser.add_argument("--split", type=str, required=True, choices=["eigen", "eigen_benchmark"])
    parser.add_argument("--out", type=str, default=None, help="default: <split_dir>/<split>/gt_depths.npz")
    parser.add_argument("--device", type=str, default="cuda")
    opt = parser.parse_args(argv)
    lines = read_split(os.path.join(opt.split_dir, opt.split, "test_files.txt"))
    print("Exporting ground truth depths for {}".format(opt.split))
    maps = velodyne_maps(opt.data_path, lines, opt.device) if opt.split == "eigen" else benchmark_maps(opt.data_path, lines)
    out = opt.out or os.path.join(opt.split_dir, opt.split, "gt_depths.npz")
    save_gt_depths(out, maps)
    print("Saving to {}".format(out))
    return out


if __name__ == "__main__":
    main()
