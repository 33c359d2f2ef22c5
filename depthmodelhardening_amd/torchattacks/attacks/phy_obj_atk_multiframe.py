"""PGD-L_inf object attack on a multi-frame depth model (ManyDepth run with a lookup frame).  This project's addition: the
reference attacks ManyDepth in the degenerate single-frame call only, and computes the matching volume under ``no_grad``.

The object stands in the scene, so it is visible in the current AND in the previous frame: every step pastes the patch into
the current scenes with that step's (z0, alpha) and into the lookup scenes with the same draw seen from the lookup camera
(``PhysicalTrans.coeffs_for(z0, alpha, None, T_lookup)``, the way the stereo twin of the training data is pasted), runs
``ManyDepthModelWrapper`` with ``poses = T_lookup`` and takes the cost, the gradient and the sign step of ``Phy_obj_atk``.

``matching_grad`` says how much of the gradient is taken:
    "none"      the matching volume is a constant (the reference's ``no_grad``): the baseline, and a case of gradient masking;
    "current"   the gradient flows through the volume to the current frame's features only (K38's ``d_current``);
    "full"      also through the lookup features into the patch pasted on the lookup frame (K38's ``d_lookup``).  The default.

``pose_translation_scale`` multiplies the translation of ``T_lookup`` before it is handed to the encoder: the ratio of the
network's depth units to metres.  The paste works in metres (the calibration file), the cost volume in the units of the depth
bins (0.1 .. 20 for KITTI_HR, learnt up to scale by a monocular model).  Nobody has measured that ratio for KITTI_HR; 1.0 is a
placeholder, not a claim.

L_inf, eager, whole frame: ``shard``, ``use_graph`` and windows raise NotImplementedError.  The (z0, alpha) draws and their
order are the parent's; the return tuple is the parent's, and ``last_lookup_scenes`` / ``last_lookup_scenes_ben`` /
``last_lookup_masks`` hold the lookup frames of the returned scenes.
"""
import numpy as np
import torch

from ... import ops
from ...my_utils import object_dataset_root, to_device_async
from .phy_obj_atk import Phy_obj_atk

MATCHING_GRAD_MODES = ("none", "current", "full")


class Phy_obj_atk_mf(Phy_obj_atk):
    def __init__(self, model, obj_img, obj_mask, eps=0.3, alpha=2 / 255, steps=40, random_start=True,
                 dist_range=list(range(5, 31, 2)), matching_grad="full", pose_translation_scale=1.0):
        super().__init__(model, obj_img, obj_mask, eps=eps, alpha=alpha, steps=steps, random_start=random_start,
                         dist_range=dist_range)
        if matching_grad not in MATCHING_GRAD_MODES:
            raise ValueError("Phy_obj_atk_mf: matching_grad must be one of %s; got %r" % (MATCHING_GRAD_MODES, matching_grad))
        self.matching_grad = matching_grad
        self.pose_translation_scale = float(pose_translation_scale)
        self.use_roi = False            # whole frames: the windowed path (K19) is not extended to the cost-volume encoder
        self.last_lookup_scenes = None
        self.last_lookup_scenes_ben = None
        self.last_lookup_masks = None

    def network_pose(self, T_lookup, n):
        """[n,1,4,4] on the attack's device: ``T_lookup`` with its translation in the network's units."""
        T = np.array(T_lookup, dtype=np.float64).reshape(4, 4)
        T[:3, 3] *= self.pose_translation_scale
        return to_device_async(np.ascontiguousarray(np.broadcast_to(T.astype(np.float32), (n, 1, 4, 4))), self.device)

    def _encoder(self):
        enc = getattr(self.model, "encoder", None)
        if enc is None or not hasattr(enc, "matching_grad"):
            raise RuntimeError("Phy_obj_atk_mf needs a multi-frame depth model (depth_model.ManyDepthModelWrapper)")
        return enc

    def forward(self, images, batch_size, lookup_images=None, T_lookup=None,
                cfg_path=f'{object_dataset_root}/training/calib/003086.txt', eval=False):
        r"""
        images, lookup_images: the current scenes and the previous frame of each, 1*3*375*1242 or batch_size*3*375*1242.
        T_lookup: 4x4, current-camera to lookup-camera coordinates, in metres (a forward drive of tz: T[2, 3] = tz).
        """
        if self.shard is not None:
            raise NotImplementedError("Phy_obj_atk_mf: shard (the data-parallel shared-patch mode) is not served")
        if self.use_graph:
            raise NotImplementedError("Phy_obj_atk_mf: use_graph is not served (the attack runs eagerly)")
        if self.use_roi or self.common_windows:
            raise NotImplementedError("Phy_obj_atk_mf: windows (K19) are not extended to the cost-volume encoder")
        if lookup_images is None or T_lookup is None:
            raise RuntimeError("Phy_obj_atk_mf: lookup_images and T_lookup are required")
        enc = self._encoder()
        images = images.detach().to(self.device)
        lookups = lookup_images.detach().to(self.device)
        self._check_batch(images, batch_size)
        if lookups.shape != images.shape:
            raise RuntimeError("Phy_obj_atk_mf: lookup_images %s must have the shape of images %s" % (
                tuple(lookups.shape), tuple(images.shape)))

        obj_img_adv = self.obj_img.clone().detach()
        if self.random_start:
            obj_img_adv = torch.clamp(obj_img_adv + self._random_start(obj_img_adv), min=0, max=1).detach()

        # the parent's draws in the parent's order; each is projected into both cameras
        pt = self.phy_trans_ben
        draws = [self._draw(batch_size) for _ in range(self.steps)]
        z0_sample, alpha_sample = self._draw(batch_size, explicit=True)
        self._eval_pose(z0_sample, alpha_sample, eval)
        samples = draws + [(z0_sample, alpha_sample)]
        T_host = np.array(T_lookup, dtype=np.float64).reshape(4, 4)
        coeffs = self._coeffs(samples)
        coeffs_look = to_device_async(np.stack([pt.coeffs_for(z0, al, None, T_host) for z0, al in samples], 0), self.device)
        poses = self.network_pose(T_host, batch_size)
        l_pad, t_pad = pt.l_pad, pt.t_pad
        mask = self.obj_mask.to(self.device)
        self._one = torch.ones((), device=self.device, dtype=torch.float32)
        through_lookup = self.matching_grad == "full"

        saved = enc.matching_grad
        enc.matching_grad = {"none": False, "current": "current", "full": True}[self.matching_grad]
        try:
            for s in range(self.steps):
                obj_img_adv.requires_grad_()
                adv_scenes, obj_masks_out = ops.eot_paste(images, obj_img_adv, mask, coeffs[s], l_pad, t_pad, self.scene_size)
                with torch.set_grad_enabled(through_lookup):
                    look_scenes, _ = ops.eot_paste(lookups, obj_img_adv if through_lookup else obj_img_adv.detach(), mask,
                                                   coeffs_look[s], l_pad, t_pad, self.scene_size)
                cost = self.model.masked_sq_mean(adv_scenes, obj_masks_out, negate=True, lookup_images=look_scenes.unsqueeze(1),
                                                 poses=poses)
                grad = torch.autograd.grad(cost, obj_img_adv, grad_outputs=self._grad_seed(cost), retain_graph=False,
                                           create_graph=False)[0]
                if self.trace is not None:
                    self.trace.append((float(cost.detach()), grad.detach().clone()))
                obj_img_adv = self._step(obj_img_adv, grad)
        finally:
            enc.matching_grad = saved

        with torch.no_grad():
            self.last_lookup_scenes, self.last_lookup_masks = ops.eot_paste(lookups, obj_img_adv, mask, coeffs_look[-1], l_pad,
                                                                            t_pad, self.scene_size)
            self.last_lookup_scenes_ben, _ = ops.eot_paste(lookups, self.obj_img, mask, coeffs_look[-1], l_pad, t_pad,
                                                           self.scene_size)
        return self._return_scenes(images, obj_img_adv, self.obj_img, mask, coeffs[-1])
