"""Tube-light attack on the object patch: the black-box random search of the reference's ``evaluate_attacks``
(``MD2/evaluate_depth.py:150-151,178-182``, ``norm_type == "light"``).

Same class name, constructor, call signature and return tuple as the reference's ``torchattacks/attacks/phy_obj_atk_light.py``
(forward :64-188); the literals 200 and 20 of :113 and :88 are the keywords ``n_init`` and ``n_search``.  The search casts
n_init x n_search x 2 coloured light beams on the object, pastes each lit object at fresh random poses, and keeps the one the
model answers with the smallest masked disparity.  Nothing in it depends on the model's answers -- ``init_v`` is never updated
(:117-128), the only feedback is the running minimum (:165-167) -- so every parameter set (numpy's generator) and every pose
(Python's) is drawn on the host before the first launch, in the reference's order, and the loop reads nothing back:

    per query   K24 tube_light_compose (the lit patch, from the record the device cursor points at)
                -> K3 eot_paste -> model / K19 windowed cost -> K24 tube_light_commit (cost array, best cost, best query, cursor)

where the reference fills a 260 x 300 x 3 array in a Python double loop, adds it with OpenCV, rounds through a PIL uint8 image,
uploads it and compares ``cost < best_cost`` on the host, 8000 times.  After the loop the best patch is regenerated from the
best query's record by the same kernel (deterministic: the very bits that won).
"""
import contextlib

import numpy as np
import torch

from ... import ops
from ...my_utils import object_dataset_root, to_device_async
from ...roi import RoiPlan
from .phy_obj_atk import Phy_obj_atk

Q = np.asarray([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 1], [0, 1, 1, 0],
                [0, 1, 0, 1], [0, 0, 1, 1]])        # the search directions of :90-100: wavelength, angle, b, beta
LO, HI = [380, 0, 0, 10], [750, 180, 400, 1600]     # :128


class Phy_obj_atk_light(Phy_obj_atk):
    r"""
    Arguments:
        model (nn.Module): model to attack.
        obj_img (1x3xHxW), obj_mask (1x1xHxW): object patch and its paint mask.
        eps, alpha, steps, random_start: accepted as the reference accepts them; the search does not use them.
        n_init (int): start points of the search. (Default: 200)
        n_search (int): random directions per start point, each tried both ways. (Default: 20)
        host_chain (bool): run the reference's shape instead -- the pattern in numpy on the host, an upload and a host
            comparison per query -- on the same paste / cost kernels (the benchmark's baseline and the tests' eager twin).
    """

    def __init__(self, model, obj_img, obj_mask, eps=1, alpha=0.2, steps=40, random_start=True,
                 dist_range=list(range(5, 31, 2)), n_init=200, n_search=20, host_chain=False):
        super().__init__(model, obj_img, obj_mask, eps=eps, alpha=alpha, steps=steps, random_start=random_start,
                         dist_range=dist_range)
        if int(n_init) < 1 or int(n_search) < 1:
            raise ValueError("Phy_obj_atk_light: n_init and n_search must be positive")
        self.n_init, self.n_search, self.host_chain = int(n_init), int(n_search), bool(host_chain)
        # test hooks
        self.trace = None       # set to a list: after the search it receives one dict per query (cost, params = (wavelength,
        #                         angle, b, beta), z0, alpha), read from the ONE copy of the cost array
        # loop_context: a context-manager factory entered around the whole query loop (tests: torch.cuda.set_sync_debug_mode)
        self.loop_context = contextlib.nullcontext
        self.best_index = None  # what that one copy held: the best query ...
        self.costs = None       # ... and the cost of every query (numpy)

    def draw_params(self):
        """int64 [n_init * n_search * 2, 4]: every parameter set of the search from numpy's global generator in the order of
        :113-128 (all start points first; per direction one ``randint(len(Q))`` and one ``randint(1, 20)``, used for a = -1, +1)."""
        inits = [[np.random.randint(380, 750), np.random.randint(0, 180), np.random.randint(0, 400), np.random.randint(10, 1600)]
                 for _ in range(self.n_init)]
        out = np.zeros((self.n_init, self.n_search, 2, 4), dtype=np.int64)
        for i, init_v in enumerate(inits):
            for s in range(self.n_search):
                q = Q[np.random.randint(len(Q))] * np.random.randint(1, 20)
                for j, a in enumerate((-1, 1)):
                    out[i, s, j] = np.clip(np.asarray(init_v) + a * q, LO, HI)
        return out.reshape(-1, 4)

    def forward(self, images, batch_size, cfg_path=f'{object_dataset_root}/training/calib/003086.txt', eval=False):
        r"""
        images: scene image, 1*3*375*1242 (tiled over the batch) or batch_size*3*375*1242.
        In eval mode the first object position / angle of the returned scenes is fixed (7 m, 0 deg).
        """
        if self.shard is not None:
            raise NotImplementedError("Phy_obj_atk_light: shard is not built (evaluation runs on one rank)")
        images = images.detach().to(self.device)
        if images.size()[0] != 1 and images.size()[0] != batch_size:
            raise RuntimeError('Batch size doesn\'t match!')
        scene_imgs = images
        dev = self.device
        obj = self.obj_img.detach().to(dev).contiguous()
        mask = self.obj_mask.to(dev)
        pt = self.phy_trans_ben
        l_pad, t_pad = pt.l_pad, pt.t_pad

        # both streams up front, in the reference's order: numpy's for the parameters, Python's for one project() per query and
        # the two samples of the returned scenes (:173-174)
        params = self.draw_params()
        n = len(params)
        draws = [self._draw(batch_size) for _ in range(n)]
        z0_sample, alpha_sample = self._draw(batch_size, explicit=True)
        if eval:
            z0_sample[0] = 7
            alpha_sample[0] = 0
        coeffs = self._coeffs(draws + [(z0_sample, alpha_sample)])
        table_host = ops.tube_light_table(params)
        base = obj.mul(255).to(torch.uint8).contiguous()        # ToPILImage (:111): truncation

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
            return ops.masked_sq_mean(self.model(adv), m)        # MSE(adv_depth * mask, 0) (:163): minimised

        adv_patch = torch.zeros_like(obj)
        if self.host_chain:
            costs, best = self._host_search(table_host, base, cost_of, adv_patch)
        else:
            table = to_device_async(table_host, dev)
            state, best_cost, cost_arr = ops.tube_light_state(n, dev)
            patch = torch.zeros_like(obj)
            with torch.no_grad():
                # a throwaway cost of the clean object at query 0's poses: the first model call of a frozen-weights scope fills
                # its caches (transformed filters, BatchNorm affines), one-time host work that is no part of any query
                cost_of(obj, 0)
                with self.loop_context():
                    for q in range(n):
                        ops.tube_light_compose(table, state, base, out=patch)
                        ops.tube_light_commit(cost_of(patch, q).reshape(1), cost_arr, best_cost, state)
                ops.tube_light_compose(table, state[1:], base, out=adv_patch)       # the best query's patch, bit for bit
            costs, best = cost_arr.cpu().numpy(), int(state.cpu()[1])       # the reads of the search: after it
        self.costs, self.best_index = costs, best
        if best < 0:
            raise RuntimeError("Phy_obj_atk_light: no query had a cost below 1e10 (non-finite model output?)")
        if self.trace is not None:
            for q in range(n):
                self.trace.append(dict(cost=float(costs[q]), params=tuple(int(v) for v in params[q]), z0=list(draws[q][0]),
                                       alpha=list(draws[q][1])))

        self.phy_trans_adv.reset_img(adv_patch, self.obj_mask)
        with torch.no_grad():
            adv_scenes, obj_masks_out = ops.eot_paste(scene_imgs, adv_patch, mask, coeffs[-1], l_pad, t_pad, self.scene_size)
            ben_scenes, _ = ops.eot_paste(scene_imgs, obj, mask, coeffs[-1], l_pad, t_pad, self.scene_size)
        return adv_scenes, ben_scenes, obj_masks_out, adv_patch

    def _host_search(self, table_host, base, cost_of, adv_patch):
        """The reference's loop shape on this project's paste and cost: pattern on the host (numpy, where the reference loops in
        Python), one upload and one host comparison per query.  Returns (costs, best query); ``adv_patch`` receives the winner."""
        base_hwc = base[0].permute(1, 2, 0).contiguous().cpu().numpy()
        n = len(table_host)
        costs = np.zeros(n, dtype=np.float32)
        best_cost, best = 1e10, -1
        with torch.no_grad():
            cost_of(self.obj_img.detach().to(self.device).contiguous(), 0)      # the same warm-up as the device loop's
        with torch.no_grad(), self.loop_context():
            for q in range(n):
                u8 = ops.tube_light_host(base_hwc, table_host[q])
                patch = torch.from_numpy(u8).permute(2, 0, 1).float().div(255).unsqueeze(0).to(self.device)   # ToTensor, upload
                cost = cost_of(patch.contiguous(), q)
                if cost < best_cost:        # the host read of :165
                    best_cost, best = cost, q
                    adv_patch.copy_(patch)
                costs[q] = float(cost)
        return costs, best
