"""The no-op paste of the reference's evaluation protocol for the tube-light attack (``MD2/evaluate_depth.py:178-182``): after
the first scene batch has run the search, every later batch pastes the patch it found.

Same class name, constructor, call signature and return tuple as the reference's ``torchattacks/attacks/phy_obj_atk_vanila.py``
(forward :58-94): the given patch and the clean object at ONE shared pose draw, two K3 launches.
"""
from ...my_utils import object_dataset_root
from .phy_obj_atk import Phy_obj_atk


class Phy_obj_atk_vanila(Phy_obj_atk):
    r"""
    Arguments:
        model (nn.Module): the model (not called: the paste needs its device only).
        obj_img (1x3xHxW), obj_mask (1x1xHxW): the clean object patch and its paint mask.
    """

    def __init__(self, model, obj_img, obj_mask, dist_range=list(range(5, 31, 2))):
        super().__init__(model, obj_img, obj_mask, dist_range=dist_range)
        self._clean_img = obj_img       # what phy_trans_ben keeps pasting after forward() has replaced self.obj_img (:73)

    def forward(self, images, obj_img, batch_size, cfg_path=f'{object_dataset_root}/training/calib/003086.txt', eval=False):
        r"""
        images: scene image, 1*3*375*1242 (tiled over the batch) or batch_size*3*375*1242;  obj_img: the patch to paste.
        In eval mode the first object position / angle is fixed (7 m, 0 deg).
        """
        images = images.detach().to(self.device)
        self._check_batch(images, batch_size)
        self.obj_img = obj_img
        obj_img_adv = obj_img.clone().detach().to(self.device)
        z0_sample, alpha_sample = self._draw(batch_size, explicit=True)
        self._eval_pose(z0_sample, alpha_sample, eval)
        coeffs = self._coeffs([(z0_sample, alpha_sample)])
        return self._return_scenes(images, obj_img_adv, self._clean_img.to(self.device), self.obj_mask.to(self.device), coeffs[0])
