"""The gradient-free rows of the evaluation (tube light, Gaussian blur) as one search: ``n`` candidate patches, none of which
depends on the model's answers, each pasted at fresh random poses; the one the model answers with the smallest masked disparity
wins.  Every draw is made on the host before the first launch, in the reference's order, and the loop reads nothing back:

    per query   compose (the candidate the device cursor points at) -> K3 eot_paste -> model / K19 windowed cost
                -> K24 tube_light_commit (cost array, best cost, best query, cursor)

After the loop the best patch is recomposed from the best query's index by the same kernel (deterministic: the very bits that
won), and the cost array and the best index are read once.
"""
import contextlib

import numpy as np
import torch

from ... import ops
from ...my_utils import object_dataset_root
from .phy_obj_atk import Phy_obj_atk


class _ObjectSearch(Phy_obj_atk):
    """``host_chain=True`` runs the reference's shape instead -- the candidate made on the host, an upload and a host comparison
    per query -- on the same paste / cost kernels (the benchmarks' baseline and the tests' eager twin).  A subclass supplies

        noun                            what it calls a query, in messages
        _prepare(obj)                   (n, ctx): the number of queries and whatever its other hooks need; every host draw and
                                        every refusal that has to come before the pose draws happens here
        _device_search(obj, n, ctx)     (ops.tube_light_state(n, device), compose): the uploads and the device work before the
                                        loop, in its own order; compose(cursor, out) writes the patch of query cursor[0] to out
        _host_patches(obj, ctx)         make(q): the patch of query q, made on the host and uploaded
        _trace_fields(ctx, q)           its part of query q's trace dict

    and may replace what a search whose candidates depend on the model's answers (Phy_obj_atk_Square) does differently:

        shared_poses                    True: ONE pose set, window plan and coefficient row for all queries (_pose_draws returns
                                        one draw) instead of one per query
        _pose_draws(batch_size, n)      the pose draws of the search (default: one _draw() per query)
        _pasted(q, patch)               the buffer query q pastes (default: the composed patch)
        _run_queries(n, query)          the loop over query(q) (default: q = 0 .. n - 1, eagerly)
        _finish(compose, state, patch, adv_patch)    the best patch into adv_patch (default: recomposed from the best index)
        _record(costs, best)            bookkeeping of its own from the one copy of the cost array
    """

    noun = "query"
    shared_poses = False

    def __init__(self, model, obj_img, obj_mask, host_chain=False, **kw):
        super().__init__(model, obj_img, obj_mask, **kw)
        self.host_chain = bool(host_chain)
        # test hooks
        self.trace = None       # set to a list: after the search it receives one dict per query (cost, the subclass's fields,
        #                         z0, alpha), read from the ONE copy of the cost array
        # loop_context: a context-manager factory entered around the whole query loop (tests: torch.cuda.set_sync_debug_mode)
        self.loop_context = contextlib.nullcontext
        self.best_index = None  # what that one copy held: the best query ...
        self.costs = None       # ... and the cost of every query (numpy)

    def forward(self, images, batch_size, cfg_path=f'{object_dataset_root}/training/calib/003086.txt', eval=False):
        r"""
        images: scene image, 1*3*375*1242 (tiled over the batch) or batch_size*3*375*1242.
        In eval mode the first object position / angle of the returned scenes is fixed (7 m, 0 deg).
        """
        name = type(self).__name__
        if self.shard is not None:
            raise NotImplementedError("%s: shard is not built (evaluation runs on one rank)" % name)
        images = images.detach().to(self.device)
        self._check_batch(images, batch_size)
        scene_imgs = images
        dev = self.device
        obj = self.obj_img.detach().to(dev).contiguous()
        mask = self.obj_mask.to(dev)
        pt = self.phy_trans_ben
        l_pad, t_pad = pt.l_pad, pt.t_pad

        # every draw up front, in the reference's order: the subclass's own, one project() per query, the two samples of the
        # returned scenes
        n, ctx = self._prepare(obj)
        draws = self._pose_draws(batch_size, n)
        pose = (lambda q: 0) if self.shared_poses else (lambda q: q)
        z0_sample, alpha_sample = self._draw(batch_size, explicit=True)
        self._eval_pose(z0_sample, alpha_sample, eval)
        coeffs = self._coeffs(draws + [(z0_sample, alpha_sample)])
        plans, tabs, clean = self._window_plans(draws, scene_imgs, mask, coeffs[0])

        def cost_of(patch, q):
            p = pose(q)
            adv, m = ops.eot_paste(scene_imgs, patch, mask, coeffs[p], l_pad, t_pad, self.scene_size)
            if plans is not None:
                return self.model.masked_sq_mean(adv, m, plans[p], tabs[p], clean)
            return ops.masked_sq_mean(self.model(adv), m)        # MSE(adv_depth * mask, 0): minimised

        adv_patch = torch.zeros_like(obj)
        if self.host_chain:
            costs, best = self._host_search(obj, n, ctx, cost_of, adv_patch)
        else:
            (state, best_cost, cost_arr), compose = self._device_search(obj, n, ctx)
            patch = torch.zeros_like(obj)
            with torch.no_grad():
                # a throwaway cost of the clean object at query 0's poses: the first model call of a frozen-weights scope fills
                # its caches (transformed filters, BatchNorm affines), one-time host work that is no part of any query
                cost_of(obj, 0)

                def query(q):
                    compose(state, patch)
                    ops.tube_light_commit(cost_of(self._pasted(q, patch), q).reshape(1), cost_arr, best_cost, state)

                with self.loop_context():
                    self._run_queries(n, query)
                self._finish(compose, state, patch, adv_patch)
            costs, best = cost_arr.cpu().numpy(), int(state.cpu()[1])       # the reads of the search: after it
        self.costs, self.best_index = costs, best
        self._record(costs, best)
        if best < 0:
            raise RuntimeError("%s: no %s had a cost below 1e10 (non-finite model output?)" % (name, self.noun))
        if self.trace is not None:
            for q in range(n):
                self.trace.append(dict(cost=float(costs[q]), **self._trace_fields(ctx, q), z0=list(draws[pose(q)][0]),
                                       alpha=list(draws[pose(q)][1])))
        return self._return_scenes(scene_imgs, adv_patch, obj, mask, coeffs[-1])

    # ------------------------------------------------------------------------------ hooks: the defaults are the searches above
    def _pose_draws(self, batch_size, n):
        return [self._draw(batch_size) for _ in range(n)]

    def _pasted(self, q, patch):
        return patch

    def _run_queries(self, n, query):
        for q in range(n):
            query(q)

    def _finish(self, compose, state, patch, adv_patch):
        compose(state[1:], adv_patch)       # the best query's patch, bit for bit

    def _record(self, costs, best):
        pass

    def _host_search(self, obj, n, ctx, cost_of, adv_patch):
        """The reference's loop shape on this project's paste and cost: one upload and one host comparison per query.
        Returns (costs, best query); ``adv_patch`` receives the winner."""
        make = self._host_patches(obj, ctx)
        costs = np.zeros(n, dtype=np.float32)
        best_cost, best = 1e10, -1
        with torch.no_grad():
            cost_of(obj, 0)         # the same warm-up as the device loop's
        with torch.no_grad(), self.loop_context():
            for q in range(n):
                patch = make(q)
                cost = cost_of(patch, q)
                if cost < best_cost:        # the reference's host read
                    best_cost, best = cost, q
                    adv_patch.copy_(patch)
                costs[q] = float(cost)
        return costs, best
