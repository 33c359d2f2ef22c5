"""A KITTI-object calibration file as the reference's ``preprocessing/kitti_util.Calibration`` reads it (:57-96, :178-185): the parse,
``C2V`` and the intrinsics of camera 2.  Only the image -> velodyne direction is restated (``project_image_to_velo``, :159-175); its
arithmetic per pixel is K39 (``ops.pseudo_lidar``), which takes the 27 doubles of ``packed()``.  Everything here is host work done
once per frame: the kernel never inverts anything."""
import os

import numpy as np

CALIB_DOUBLES = 27      # DMH_LIDAR_CALIB: f_u f_v c_u c_v b_x b_y, inv(R0)[9], C2V[12]


def read_calib_text(text):
    """``Calibration.read_calib_file`` (:79-96) on the file's text: key -> float64 array; lines whose values are not floats are
    skipped."""
    data = {}
    for line in text.splitlines():
        line = line.rstrip()
        if len(line) == 0:
            continue
        key, value = line.split(":", 1)
        try:
            data[key] = np.array([float(x) for x in value.split()])
        except ValueError:
            pass
    return data


def inverse_rigid_trans(Tr):
    """[R' | -R' t] of a 3 x 4 [R | t] (:178-185), with the reference's own ``np.dot`` for the three translation entries."""
    inv_Tr = np.zeros_like(Tr)
    inv_Tr[0:3, 0:3] = np.transpose(Tr[0:3, 0:3])
    inv_Tr[0:3, 3] = np.dot(-np.transpose(Tr[0:3, 0:3]), Tr[0:3, 3])
    return inv_Tr


class Calibration(object):
    """``P`` (3 x 4, P2), ``V2C``, ``C2V`` (3 x 4), ``R0`` (3 x 3), ``c_u c_v f_u f_v b_x b_y``: the reference's attributes with the
    reference's values.  ``source``: a path, or the text of a calibration file (anything with a newline or a colon in it that is not
    an existing file).  ``crop=(left, top)``: the scene was cropped by that many pixels, so the principal point moves with it."""

    def __init__(self, source, crop=None):
        source = os.fspath(source) if hasattr(source, "__fspath__") else source
        if "\n" not in source and os.path.isfile(os.path.expanduser(source)):
            with open(os.path.expanduser(source), "r") as f:
                source = f.read()
        elif "\n" not in source and ":" not in source:
            raise RuntimeError("no calibration file %s" % source)
        calibs = read_calib_text(source)
        for key, count in (("P2", 12), ("Tr_velo_to_cam", 12), ("R0_rect", 9)):
            if key not in calibs or calibs[key].size != count:
                raise RuntimeError("calibration: need %d values under %s" % (count, key))
        self.P = np.reshape(calibs["P2"], [3, 4])
        self.V2C = np.reshape(calibs["Tr_velo_to_cam"], [3, 4])
        self.C2V = inverse_rigid_trans(self.V2C)
        self.R0 = np.reshape(calibs["R0_rect"], [3, 3])
        self.c_u = self.P[0, 2]
        self.c_v = self.P[1, 2]
        self.f_u = self.P[0, 0]
        self.f_v = self.P[1, 1]
        self.b_x = self.P[0, 3] / (-self.f_u)
        self.b_y = self.P[1, 3] / (-self.f_v)
        if crop is not None:
            left, top = crop
            self.c_u = self.c_u - float(left)
            self.c_v = self.c_v - float(top)

    def packed(self):
        """float64 [27]: f_u f_v c_u c_v b_x b_y, ``np.linalg.inv(R0)`` (as project_rect_to_ref forms it, :119) and C2V, row-major."""
        return np.concatenate([np.array([self.f_u, self.f_v, self.c_u, self.c_v, self.b_x, self.b_y], dtype=np.float64),
                               np.linalg.inv(self.R0).reshape(-1), self.C2V.reshape(-1)]).astype(np.float64)
