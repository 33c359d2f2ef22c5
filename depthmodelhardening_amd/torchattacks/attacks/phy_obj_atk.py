"""PGD-L_inf attack on one shared object patch under expectation over physical transformations.

Same class name, constructor, call signature, return tuple and error behaviour as the reference's
``torchattacks/attacks/phy_obj_atk.py:13-123``.  The inner loop (:83-101) is re-built on the HIP kernels:

    per step   K3 eot_paste (pad + perspective + composite + resize, one launch for all B samples)
               -> model (PyTorch/MIOpen) -> K6 masked_sq_mean -> autograd (K6 bwd, model bwd, K3 bwd)
               -> K4 pgd_linf_step

instead of B x 2 ``perspective`` calls, a composite, two ``Resize`` and five element-wise kernels.
The (z0, alpha) draws use ``random.sample`` in the reference's order; the per-step homography
coefficients for the whole attack are computed on the host up front and shipped in ONE H2D copy.
"""
import torch

from ... import ops
from ...my_utils import object_dataset_root
from .object_attack import ObjectAttack


class Phy_obj_atk(ObjectAttack):
    r"""
    Distance Measure : Linf

    Arguments:
        model (nn.Module): model to attack.
        obj_img (1x3xHxW), obj_mask (1x1xHxW): object patch and its paint mask.
        eps (float): maximum perturbation. (Default: 0.3)
        alpha (float): step size. (Default: 2/255)
        steps (int): number of steps. (Default: 40)
        random_start (bool): using random initialization of delta. (Default: True)
    """

    def __init__(self, model, obj_img, obj_mask, eps=0.3,
                 alpha=2 / 255, steps=40, random_start=True, dist_range=list(range(5, 31, 2))):
        super().__init__("PGD", model, obj_img, obj_mask, dist_range)
        self.eps = eps
        self.alpha = alpha
        self.steps = steps
        self.random_start = random_start
        self._supported_mode = ['default', 'targeted']
        self._targeted = True
        self.random_start_noise = None  # test hook: a tensor here replaces the uniform_(-eps, eps) draw
        self.trace = None       # test hook: set to a list to record (cost, patch gradient) of every step
        # (z0, alpha) are drawn WITHOUT replacement from 25 distances / 13 angles (physicalTrans.py:150,155), so the
        # reference raises ValueError beyond 13 scenes.  pose_group = g (<= 13) lifts that for larger batches: every run
        # of g consecutive scenes gets its own draw without replacement (physical_adv_training at batch 32: 13 + 13 + 6).
        # None = the reference's behaviour.
        self.pose_group = None
        # use_graph, common_windows, shard, use_roi: see ObjectAttack.  _capture_fault makes the capture of _graph_steps fail
        # after its first launch.

    # the two pieces a subclass with another norm swaps (Phy_obj_atk_l2)
    def _random_start(self, obj_img_adv):
        """The noise added to the clean patch before the first step (:83-85), on the attack's device."""
        noise = self.random_start_noise
        if noise is None:
            noise = torch.empty_like(obj_img_adv).uniform_(-self.eps, self.eps)
        return noise.to(self.device)

    def _step(self, x, grad, out=None):
        """The patch after one update (:98-101): K4."""
        return ops.pgd_linf_step(x, self.obj_img, grad, self.alpha, self.eps, out=out)

    def forward(self, images, batch_size, cfg_path=f'{object_dataset_root}/training/calib/003086.txt', eval=False):
        r"""
        images: scene image, 1*3*375*1242 (tiled over the batch) or batch_size*3*375*1242.
        In eval mode the first object position / angle of the returned scenes is fixed (7 m, 0 deg).
        """
        images = images.detach().to(self.device)
        mine, share = None, 1.0
        if self.shard is not None:
            import torch.distributed as dist
            rank, world, group = self.shard
            mine = list(range(rank, batch_size, world))         # this rank's scenes of the global batch
            share = len(mine) / float(batch_size)               # its part of the global mean of the cost
        n_local = batch_size if mine is None else len(mine)
        self._check_batch(images, n_local)
        scene_imgs = images

        obj_img_adv = self.obj_img.clone().detach()
        if self.random_start:
            noise = self._random_start(obj_img_adv)
            if mine is not None:
                dist.broadcast(noise, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            obj_img_adv = torch.clamp(obj_img_adv + noise, min=0, max=1).detach()

        # every (z0, alpha) draw of the attack, in the reference's order: one project() per step
        # (physicalTrans.py:150,155), then the two explicit draws for the returned scenes (:108-109)
        pt = self.phy_trans_ben
        draws = [self._draw(batch_size) for _ in range(self.steps)]
        z0_sample, alpha_sample = self._draw(batch_size, explicit=True)
        self._eval_pose(z0_sample, alpha_sample, eval)
        if mine is not None:        # rank 0's draws for the whole batch; every rank keeps the poses of its own scenes
            box = [draws + [(z0_sample, alpha_sample)]]
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            allp = [([z[i] for i in mine], [a[i] for i in mine]) for z, a in box[0]]
            draws, (z0_sample, alpha_sample) = allp[:-1], allp[-1]
            if n_local == 0:        # more ranks than scenes: this rank only takes part in the exchange
                return self._shard_without_scenes(obj_img_adv, dist, group)
            batch_size = n_local
        coeffs = self._coeffs(draws + [(z0_sample, alpha_sample)])
        l_pad, t_pad = pt.l_pad, pt.t_pad
        mask = self.obj_mask.to(self.device)

        # a graph holds no collective (shard), no host read (trace), and needs a step to replay
        want_graph = bool(self.use_graph and mine is None and self.trace is None and self.steps >= 3
                          and not ops.profiling_every_launch())
        plans, tabs, clean = self._window_plans(draws, scene_imgs, mask, coeffs[0], common=self.use_graph or self.common_windows,
                                                bind=not want_graph)
        self._one = torch.ones((), device=self.device, dtype=torch.float32)
        first = 0
        if want_graph and plans is not None:
            if self._one_size(plans):
                obj_img_adv, first = self._graph_steps(scene_imgs, obj_img_adv, mask, coeffs, plans[0], tabs, clean, l_pad, t_pad)
            if first < self.steps:      # no common size, or the capture failed: the eager loop takes over on the same plans
                self._bind_tables(plans, tabs)
        for s in range(first, self.steps):
            obj_img_adv.requires_grad_()
            adv_scenes, obj_masks_out = ops.eot_paste(scene_imgs, obj_img_adv, mask, coeffs[s], l_pad, t_pad,
                                                      self.scene_size)
            if plans is not None:
                cost = self._neg_cost(adv_scenes, obj_masks_out, plans[s], tabs[s], clean)
            else:
                adv_depth = self.model(adv_scenes)
                cost = -ops.masked_sq_mean(adv_depth, obj_masks_out)  # -MSE(adv_depth * mask, 0)
            if mine is not None:
                cost = cost * share     # the local mean's part of the mean over the global batch
            grad = torch.autograd.grad(cost, obj_img_adv, grad_outputs=self._grad_seed(cost), retain_graph=False,
                                       create_graph=False)[0]
            if mine is not None:        # 0.94 MB: the one exchange of the shared-patch attack, before the sign
                dist.all_reduce(grad, op=dist.ReduceOp.SUM, group=group)
            if self.trace is not None:
                self.trace.append((float(cost), grad.detach().clone()))
            obj_img_adv = self._step(obj_img_adv, grad)

        return self._return_scenes(scene_imgs, obj_img_adv, self.obj_img, mask, coeffs[-1])

    def _graph_steps(self, scene_imgs, obj_img_adv, mask, coeffs, plan, tabs, clean, l_pad, t_pad):
        """All steps of the attack with ONE captured step.  The step reads its pose (homography coefficients, window origins)
        and its patch from fixed device buffers, so a replay after two small device copies IS the next step; every window plan
        of the attack has the sizes of ``plan`` (roi.common_size_plans).  Step 0 runs eagerly: it fills the caches of the
        frozen-weights scope (transformed filters, the clean frames' features), which must not be captured and replayed.
        The capture itself, and what a failed one leaves behind: ObjectAttack._capture_graph."""
        patch_in, patch_out = obj_img_adv.detach().clone(), torch.empty_like(obj_img_adv)
        coeff_cur, tab_cur = coeffs[0].clone(), tabs[0].clone()
        plan.bind_table(tab_cur)
        plan.table_rewritten = True     # consumers that keep origins for a later step must copy them (ops.CleanHead.mark)

        def step():
            p = patch_in.detach().requires_grad_(True)
            adv, m = ops.eot_paste(scene_imgs, p, mask, coeff_cur, l_pad, t_pad, self.scene_size)
            cost = self._neg_cost(adv, m, plan, tab_cur, clean)
            (grad,) = torch.autograd.grad(cost, p, grad_outputs=self._one)
            self._step(p, grad, out=patch_out)
            patch_in.copy_(patch_out)

        step()                                              # step 0, eager
        coeff_cur.copy_(coeffs[1])
        tab_cur.copy_(tabs[1])

        def traced():
            if self._capture_fault:                         # test hook: a capture that dies half way
                ops.eot_paste(scene_imgs, patch_in, mask, coeff_cur, l_pad, t_pad, self.scene_size)
                raise RuntimeError("injected capture fault")
            step()

        g = self._capture_graph(traced, what="the attack step")
        if g is None:
            # Nothing of the captured step has executed: the device holds the state step 0 left (patch_in = the patch after
            # step 0, the encoder head's bookkeeping copies of step 0's origins).  Hand the attack back to the eager loop.
            return patch_in.clone(), 1
        g.replay()                                          # step 1 (capturing executes nothing)
        for s in range(2, self.steps):
            coeff_cur.copy_(coeffs[s])
            tab_cur.copy_(tabs[s])
            g.replay()
        out = patch_in.clone()
        self._keep_graph(g)
        return out, self.steps

    def _shard_without_scenes(self, obj_img_adv, dist, group):
        """A rank whose share of the attack batch is empty (world > batch_size): it contributes a zero gradient to every
        step's sum and follows the patch."""
        for _ in range(self.steps):
            grad = torch.zeros_like(obj_img_adv)
            dist.all_reduce(grad, op=dist.ReduceOp.SUM, group=group)
            obj_img_adv = self._step(obj_img_adv, grad)
        self.phy_trans_adv.reset_img(obj_img_adv, self.obj_mask)
        empty = obj_img_adv.new_zeros((0, 3) + tuple(self.scene_size))
        return empty, empty.clone(), obj_img_adv.new_zeros((0, 1) + tuple(self.scene_size)), obj_img_adv
