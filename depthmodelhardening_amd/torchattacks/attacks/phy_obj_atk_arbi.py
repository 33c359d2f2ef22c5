"""Random-patch baseline on the object: the no-search row of the reference's ``evaluate_attacks``
(``MD2/evaluate_depth.py:146-147``, ``norm_type == "arbi"``).

Same class name, constructor, call signature and return tuple as the reference's ``torchattacks/attacks/phy_obj_atk_arbi.py``
(forward :56-108).  Every call fills the rectangle [90:170, 100:200] of the object from a generator the instance keeps
(``RandomState(17)``, :54): with probability one half per-pixel noise, else one constant colour.  The poses are not drawn from
Python's generator: distances ``linspace(5, 30, batch_size)``, angles from a fresh ``RandomState(17)`` (:91-92).  There is no
search and no hot path: the fill is made on the host as the reference makes it, the rectangle uploaded, and the two pastes are
K3 launches.
"""
import numpy as np
import torch

from ... import ops
from ...my_utils import object_dataset_root
from .phy_obj_atk import Phy_obj_atk


class Phy_obj_atk_arbi(Phy_obj_atk):
    r"""
    Arguments:
        model (nn.Module): the model (not called: the paste needs its device only).
        obj_img (1x3xHxW), obj_mask (1x1xHxW): the clean object patch and its paint mask.
        region (r0, r1, c0, c1): the rectangle that is filled, clipped as the slices clip. (Default: (90, 170, 100, 200))
    """

    def __init__(self, model, obj_img, obj_mask, dist_range=list(range(5, 31, 2)), region=ops.GAUSS_REGION):
        super().__init__(model, obj_img, obj_mask, dist_range=dist_range)
        self.region = tuple(int(v) for v in region)
        self.rs = np.random.RandomState(17)
        self.fills = []         # test hook: which fill every call drew, "noise" or "colour"

    def draw_fill(self, shape):
        """fp32 [b, c, rh, rw]: the rectangle of the next pattern, from ``self.rs`` in the order of :77-82 -- one ``rand()`` for the
        branch; then ``rand(b, c, h, w)`` for the WHOLE patch (the generator moves as the reference's does), or one ``rand()``
        per channel."""
        b, c, h, w = shape
        r0, r1, c0, c1 = ops._gauss_region(self.region, h, w, "Phy_obj_atk_arbi")
        if self.rs.rand() > 0.5:
            self.fills.append("noise")
            return np.ascontiguousarray(self.rs.rand(b, c, h, w)[:, :, r0:r1, c0:c1].astype(np.float32))
        self.fills.append("colour")
        fill = np.ones((b, c, r1 - r0, c1 - c0), dtype=np.float32)
        for c_ind in range(c):
            fill[:, c_ind] *= np.float32(self.rs.rand())        # a fp32 tensor times a Python float: the factor rounded to fp32
        return fill

    def forward(self, images, batch_size, cfg_path=f'{object_dataset_root}/training/calib/003086.txt', eval=False):
        r"""
        images: scene image, 1*3*375*1242 (tiled over the batch) or batch_size*3*375*1242.
        In eval mode the first object position / angle is fixed (7 m, 0 deg).
        """
        images = images.detach().to(self.device)
        self._check_batch(images, batch_size)
        obj = self.obj_img.detach().to(self.device).contiguous()
        r0, r1, c0, c1 = ops._gauss_region(self.region, int(obj.shape[-2]), int(obj.shape[-1]), "Phy_obj_atk_arbi")
        obj_img_adv = obj.clone()
        obj_img_adv[:, :, r0:r1, c0:c1] = torch.from_numpy(self.draw_fill(tuple(obj.shape))).to(self.device)

        z0_sample = np.linspace(5, 30, num=batch_size)
        alpha_sample = np.random.RandomState(17).choice(list(range(-30, 31, 2)), batch_size, replace=True)
        self._eval_pose(z0_sample, alpha_sample, eval)
        coeffs = self._coeffs([(z0_sample, alpha_sample)])
        return self._return_scenes(images, obj_img_adv, obj, self.obj_mask.to(self.device), coeffs[0])
