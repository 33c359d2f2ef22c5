"""Host side of the velodyne ground truth (K32): KITTI's calibration files, the velodyne->image projection of
``generate_depth_map`` (MD2/kitti_utils.py:17-36,49-62) and the paths of the scans (MD2/datasets/kitti_dataset.py:37-47,70-76).
The projection of the points themselves is ``ops.velo_depth_map``."""
import os

import numpy as np

_FLOAT_CHARS = set("0123456789.e+- ")
_projection_cache = {}


def read_calib_file(path):
    """A KITTI calibration file as {key: float64 array, or the string where the value is not a row of numbers}."""
    if not os.path.isfile(path):
        raise RuntimeError("calibration file %s not found: depth_gt needs <date>/calib_cam_to_cam.txt and "
                           "<date>/calib_velo_to_cam.txt beside the drives" % path)
    data = {}
    with open(path) as f:
        for line in f.read().splitlines():
            if ":" not in line:
                continue
            key, value = line.split(":", 1)
            value = value.strip()
            data[key] = value
            if _FLOAT_CHARS.issuperset(value):
                try:
                    data[key] = np.array([float(v) for v in value.split(" ")])
                except ValueError:
                    pass
    return data


def velo_projection(calib_dir, cam=2):
    """(P_velo2im float64 [3, 4], (H, W)) of camera ``cam``: P_rect_0{cam} . R_cam2rect . velo2cam, the products taken as the
    reference takes them (two ``np.dot``); the image size is S_rect_02's for both cameras (kitti_utils.py:56).  Cached per
    (calib_dir, cam)."""
    key = (os.path.abspath(calib_dir), int(cam))
    hit = _projection_cache.get(key)
    if hit is None:
        cam2cam = read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
        velo = read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
        velo2cam = np.hstack((velo["R"].reshape(3, 3), velo["T"][..., np.newaxis]))
        velo2cam = np.vstack((velo2cam, np.array([0, 0, 0, 1.0])))
        shape = cam2cam["S_rect_02"][::-1].astype(np.int32)
        R_cam2rect = np.eye(4)
        R_cam2rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
        P_rect = cam2cam["P_rect_0" + str(int(cam))].reshape(3, 4)
        P = np.dot(np.dot(P_rect, R_cam2rect), velo2cam)
        P.setflags(write=False)
        hit = _projection_cache[key] = (P, (int(shape[0]), int(shape[1])))
    return hit


def velo_path(data_path, folder, frame_index):
    return os.path.join(data_path, folder, "velodyne_points/data/{:010d}.bin".format(int(frame_index)))


def calib_dir(data_path, folder):
    return os.path.join(data_path, folder.split("/")[0])


def check_depth(data_path, filenames):
    """Whether the scan of the first split line exists (kitti_dataset.py:37-47); a line without a frame index has none."""
    parts = filenames[0].split()
    return len(parts) >= 2 and os.path.isfile(velo_path(data_path, parts[0], int(parts[1])))


def cloud_points(path):
    """The number of points of a scan, from the file's size: float32 [n, 4] records of 16 bytes."""
    size = os.path.getsize(path)
    if size % 16:
        raise RuntimeError("%s holds %d bytes, which is not a multiple of 16: a velodyne scan is float32 [n, 4]" % (path, size))
    return size // 16


def read_cloud_into(path, dst):
    """np.fromfile of a scan into ``dst``, a float32 [n, 4] numpy view of the pinned buffer."""
    a = np.fromfile(path, dtype=np.float32)
    if a.size != dst.size:
        raise RuntimeError("%s changed while it was read: %d floats, expected %d" % (path, a.size, dst.size))
    dst[...] = a.reshape(-1, 4)
