"""Gaussian-blur attack on the object patch: the gradient-free search over growing sigmas of the reference's
``evaluate_attacks`` (``MD2/evaluate_depth.py:148-149``, ``norm_type == "guassian"``, the reference's spelling).

Same class name, constructor, call signature and return tuple as the reference's ``torchattacks/attacks/phy_obj_atk_guassian.py``
(forward :61-141).  For ``steps`` growing sigmas the reference blurs the whole object with ``scipy.ndimage.gaussian_filter`` on
the host, writes the blurred rectangle [90:170, 100:200] into the object, pastes it at fresh random poses and keeps the step the
model answers with the smallest masked disparity.  Nothing in it depends on the model's answers -- the mask is 0 / 1, so the
accumulated patch is always "this step's blur inside the rectangle, the original outside" -- so every blurred rectangle is made
by K26 before the search (two launches for all steps, bit-equal to scipy), every pose is drawn on the host up front in the
reference's order, and the loop reads nothing back:

    per step    K26 gauss_blur_compose (the window the device cursor points at, into the object)
                -> K3 eot_paste -> model / K19 windowed cost -> K24 tube_light_commit (cost array, best cost, best step, cursor)

After the loop the best patch is recomposed from the best step's window by the same kernel.
"""
import contextlib

import numpy as np
import torch

from ... import ops
from ...my_utils import object_dataset_root, to_device_async
from ...roi import RoiPlan
from .phy_obj_atk import Phy_obj_atk


class Phy_obj_atk_guassian(Phy_obj_atk):
    r"""
    Arguments:
        model (nn.Module): model to attack.
        obj_img (1x3xHxW), obj_mask (1x1xHxW): object patch and its paint mask.
        steps (int): number of sigmas tried; step i blurs with sigma (i / steps) (max(H, W) // 2). (Default: 40)
        eps, alpha, random_start: accepted as the reference accepts them; the search does not use them.
        region (r0, r1, c0, c1): the rectangle of the object that is repainted, clipped as the slices clip.
            (Default: the reference's (90, 170, 100, 200))
        host_chain (bool): run the reference's shape instead -- the blur in numpy on the host, an upload and a host
            comparison per step -- on the same paste / cost kernels (the benchmark's baseline and the tests' eager twin).
    """

    def __init__(self, model, obj_img, obj_mask, eps=1, alpha=0.2, steps=40, random_start=True,
                 dist_range=list(range(5, 31, 2)), region=ops.GAUSS_REGION, host_chain=False):
        super().__init__(model, obj_img, obj_mask, eps=eps, alpha=alpha, steps=steps, random_start=random_start,
                         dist_range=dist_range)
        if int(steps) < 1:
            raise RuntimeError("Phy_obj_atk_guassian: steps must be positive")
        self.alpha = 2.5 * eps / steps      # :45
        self.region, self.host_chain = tuple(int(v) for v in region), bool(host_chain)
        # test hooks
        self.trace = None       # set to a list: after the search it receives one dict per step (cost, sigma, z0, alpha), read
        #                         from the ONE copy of the cost array
        # loop_context: a context-manager factory entered around the whole step loop (tests: torch.cuda.set_sync_debug_mode)
        self.loop_context = contextlib.nullcontext
        self.best_index = None  # what that one copy held: the best step ...
        self.costs = None       # ... and the cost of every step (numpy)

    def forward(self, images, batch_size, cfg_path=f'{object_dataset_root}/training/calib/003086.txt', eval=False):
        r"""
        images: scene image, 1*3*375*1242 (tiled over the batch) or batch_size*3*375*1242.
        In eval mode the first object position / angle of the returned scenes is fixed (7 m, 0 deg).
        """
        if self.shard is not None:
            raise NotImplementedError("Phy_obj_atk_guassian: shard is not built (evaluation runs on one rank)")
        images = images.detach().to(self.device)
        if images.size()[0] != 1 and images.size()[0] != batch_size:
            raise RuntimeError('Batch size doesn\'t match!')
        scene_imgs = images
        dev = self.device
        obj = self.obj_img.detach().to(dev).contiguous()
        mask = self.obj_mask.to(dev)
        pt = self.phy_trans_ben
        l_pad, t_pad = pt.l_pad, pt.t_pad
        n = int(self.steps)
        h, w = int(obj.shape[-2]), int(obj.shape[-1])
        sigmas = ops.gauss_sigmas(n, h, w)
        ops._gauss_region(self.region, h, w, "Phy_obj_atk_guassian")       # an empty rectangle: refused before any draw

        # every pose up front, in the reference's order: one project() per step, then the two samples of the returned scenes
        # (:128-129)
        draws = [self._draw(batch_size) for _ in range(n)]
        z0_sample, alpha_sample = self._draw(batch_size, explicit=True)
        if eval:
            z0_sample[0] = 7
            alpha_sample[0] = 0
        coeffs = self._coeffs(draws + [(z0_sample, alpha_sample)])

        plans = tabs = clean = None
        if ops.ROI_ENABLED and self.use_roi and hasattr(self.model, "masked_sq_mean") and dev.type == "cuda":
            plans = [RoiPlan(pt.mask_boxes(z0, al, self.scene_size), *self.scene_size, depth=ops.ROI_DEPTH) for z0, al in draws]
            tabs = to_device_async(np.stack([p.table() for p in plans], 0), dev)
            for p_, t_ in zip(plans, tabs):
                p_.bind_table(t_)
            with torch.no_grad():       # the frames without the object (see Phy_obj_atk.forward)
                clean, _ = ops.eot_paste(scene_imgs, obj, torch.zeros_like(mask), coeffs[0], l_pad, t_pad, self.scene_size)

        def cost_of(patch, q):
            adv, m = ops.eot_paste(scene_imgs, patch, mask, coeffs[q], l_pad, t_pad, self.scene_size)
            if plans is not None:
                return self.model.masked_sq_mean(adv, m, plans[q], tabs[q], clean)
            return ops.masked_sq_mean(self.model(adv), m)        # MSE(adv_depth * mask, 0) (:119): minimised

        adv_patch = torch.zeros_like(obj)
        if self.host_chain:
            costs, best = self._host_search(sigmas, obj, cost_of, adv_patch)
        else:
            weights_host, radii_host = ops.gauss_blur_table(sigmas)
            weights, radii = to_device_async(weights_host, dev), to_device_async(radii_host, dev)
            state, best_cost, cost_arr = ops.tube_light_state(n, dev)
            patch = torch.zeros_like(obj)
            with torch.no_grad():
                windows = ops.gauss_blur_windows(obj, weights, radii, self.region)     # every step's rectangle: two launches
                # a throwaway cost of the clean object at step 0's poses: the first model call of a frozen-weights scope fills
                # its caches (transformed filters, BatchNorm affines), one-time host work that is no part of any step
                cost_of(obj, 0)
                with self.loop_context():
                    for q in range(n):
                        ops.gauss_blur_compose(windows, state, obj, self.region, out=patch)
                        ops.tube_light_commit(cost_of(patch, q).reshape(1), cost_arr, best_cost, state)
                ops.gauss_blur_compose(windows, state[1:], obj, self.region, out=adv_patch)    # the best step's patch, bit for bit
            costs, best = cost_arr.cpu().numpy(), int(state.cpu()[1])       # the reads of the search: after it
        self.costs, self.best_index = costs, best
        if best < 0:
            raise RuntimeError("Phy_obj_atk_guassian: no step had a cost below 1e10 (non-finite model output?)")
        if self.trace is not None:
            for q in range(n):
                self.trace.append(dict(cost=float(costs[q]), sigma=sigmas[q], z0=list(draws[q][0]), alpha=list(draws[q][1])))

        self.phy_trans_adv.reset_img(adv_patch, self.obj_mask)
        with torch.no_grad():
            adv_scenes, obj_masks_out = ops.eot_paste(scene_imgs, adv_patch, mask, coeffs[-1], l_pad, t_pad, self.scene_size)
            ben_scenes, _ = ops.eot_paste(scene_imgs, obj, mask, coeffs[-1], l_pad, t_pad, self.scene_size)
        return adv_scenes, ben_scenes, obj_masks_out, adv_patch

    def _host_search(self, sigmas, obj, cost_of, adv_patch):
        """The reference's loop shape on this project's paste and cost: the blur on the host (numpy in scipy's order, the
        rectangle only), one upload and one host comparison per step.  Returns (costs, best step); ``adv_patch`` receives the
        winner."""
        r0, r1, c0, c1 = ops._gauss_region(self.region, int(obj.shape[-2]), int(obj.shape[-1]), "Phy_obj_atk_guassian")
        x0 = obj.cpu().numpy()      # :81
        costs = np.zeros(len(sigmas), dtype=np.float32)
        best_cost, best = 1e10, -1
        with torch.no_grad():
            cost_of(obj, 0)         # the same warm-up as the device loop's
        with torch.no_grad(), self.loop_context():
            for q, sigma in enumerate(sigmas):
                window = torch.from_numpy(ops.gauss_blur_host(x0, sigma, self.region)).to(self.device)     # the upload
                patch = obj.clone()
                patch[:, :, r0:r1, c0:c1] = window
                cost = cost_of(patch, q)
                if cost < best_cost:        # the host read of :121
                    best_cost, best = cost, q
                    adv_patch.copy_(patch)
                costs[q] = float(cost)
        return costs, best
