"""Auto-PGD (L_inf) on one shared object patch: the evaluation attack of the reference's ``evaluate_attacks``
(``MD2/evaluate_depth.py:138-141``).

Same class name, constructor, call signature, return tuple and error behaviour as the reference's
``torchattacks/attacks/phy_obj_atk_apgd.py`` (forward :75-115, attack_single_run :133-292, perturb(cheap=True) :295-330), for the
one configuration its evaluation uses: norm 'Linf', one restart, one EOT iteration.  Built on ``Phy_obj_atk``'s machinery:

    per iteration   K22 apgd_step (momentum step; step size and momentum weight read from the controller record on the device)
                    -> K3 eot_paste -> model / K19 windowed cost -> autograd (cost bwd, model bwd, K3 bwd)
                    -> K22 apgd_commit (best point, loss history, checkpoint, step halving, restart, next record)

The reference draws its poses with ``project(batch_size, rs=RandomState(seed))`` (:169, :236): a fresh generator with the same
seed at every call, so every iteration of one attack sees the SAME (z0, alpha) set -- one coefficient table, one window plan and
one set of clean-frame features serve the whole attack.  Where the reference ends every iteration in host reads
(``loss_steps[i] = y1.cpu()``, ``.nonzero()``, the numpy checkpoint logic of :273-290), this loop reads nothing back and branches
on nothing the device computed: the controller lives in device memory, which also makes one iteration
replayable from a HIP graph.
"""
from random import sample

import numpy as np
import torch

from ... import ops
from ...my_utils import object_dataset_root
from .phy_obj_atk import Phy_obj_atk


class Phy_obj_atk_APGD(Phy_obj_atk):
    r"""
    APGD in the paper 'Reliable evaluation of adversarial robustness with an ensemble of diverse parameter-free attacks'
    [https://arxiv.org/abs/2003.01690]

    Distance Measure : Linf

    Arguments:
        model (nn.Module): model to attack.
        obj_img (1x3xHxW), obj_mask (1x1xHxW): object patch and its paint mask.
        norm (str): 'Linf' (the reference's 'L2' branch is not built).
        eps (float): maximum perturbation. (Default: 8/255)
        steps (int): number of iterations. (Default: 100)
        n_restarts (int): 1.
        seed (int): seed of the pose draw, the same at every iteration. (Default: 17)
        eot_iter (int): 1.
        rho (float): parameter for the step-size update. (Default: 0.75)
    """

    def __init__(self, model, obj_img, obj_mask, norm='Linf', eps=8 / 255, steps=100, n_restarts=1,
                 seed=17, loss='ce', eot_iter=1, rho=.75, verbose=False,
                 dist_range=list(range(5, 31, 2))):
        for name, value, only in (("norm", norm, 'Linf'), ("n_restarts", n_restarts, 1), ("eot_iter", eot_iter, 1)):
            if value != only:
                raise NotImplementedError("Phy_obj_atk_APGD: %s=%r is not built (the reference's evaluation uses %s=%r only)"
                                          % (name, value, name, only))
        super().__init__(model, obj_img, obj_mask, eps=eps, steps=steps, dist_range=dist_range)
        self.attack = "APGD"
        self.norm = norm
        self.n_restarts = n_restarts
        self.seed = seed
        self.loss = loss
        self.eot_iter = eot_iter
        self.thr_decr = rho
        self.verbose = verbose
        self._supported_mode = ['default']
        # test hooks.  random_start_noise: a tensor here stands in for the ``2 * rand - 1`` of :142.  trace: set to a list to get,
        # after the attack, one dict per iteration read from the controller records in ONE copy (loss, loss_best, step_size, k,
        # checkpoint, reduced, moved, n_rose) plus ``patch``, a device copy of the iterate before a possible restart.

    def perturb(self, scene_imgs, best_loss=False, cheap=True):
        """The reference's entry below forward(); its ``best_loss=True`` branch (restarts ranked by loss) is never reached by the
        reference's evaluation and is not built, and ``cheap=False`` is 'not implemented yet' there too."""
        if best_loss:
            raise NotImplementedError("Phy_obj_atk_APGD: best_loss=True is not built (the reference's evaluation never uses it)")
        if not cheap:
            raise ValueError('not implemented yet')
        raise NotImplementedError("Phy_obj_atk_APGD: call the attack object; forward() holds perturb(cheap=True) and "
                                  "attack_single_run in one device-side loop")

    def forward(self, images, batch_size, cfg_path=f'{object_dataset_root}/training/calib/003086.txt', eval=False):
        r"""
        images: scene image, 1*3*375*1242 (tiled over the batch) or batch_size*3*375*1242.
        In eval mode the first object position / angle of the returned scenes is fixed (7 m, 0 deg).
        """
        if self.shard is not None:
            raise NotImplementedError("Phy_obj_atk_APGD: shard is not built (evaluation runs on one rank)")
        images = images.detach().to(self.device)
        self._check_batch(images, batch_size)
        scene_imgs = images
        dev, steps = self.device, int(self.steps)
        x0 = self.obj_img.detach().to(dev).contiguous()
        mask = self.obj_mask.to(dev)

        # start point (:142-147)
        t = self.random_start_noise
        if t is None:
            t = 2 * torch.rand(x0.shape).to(dev) - 1
        t = t.to(dev)
        eps_t = torch.full((1, 1, 1, 1), self.eps, device=dev, dtype=torch.float32)
        x_adv = (x0 + eps_t * t / t.abs().max()).clamp(0., 1.).contiguous()

        # the ONE pose set of the attack (:169, :236), then the two draws for the returned scenes (:98-99)
        pt = self.phy_trans_ben
        z0_it, al_it = pt.draw_samples(batch_size, rs=np.random.RandomState(self.seed))
        z0_sample, alpha_sample = sample(pt.dist_range, batch_size), sample(pt.angle_range, batch_size)
        self._eval_pose(z0_sample, alpha_sample, eval)
        coeffs = self._coeffs([(z0_it, al_it), (z0_sample, alpha_sample)])
        l_pad, t_pad = pt.l_pad, pt.t_pad

        plans, tabs, clean = self._window_plans([(z0_it, al_it)], scene_imgs, mask, coeffs[0])
        self._one = torch.ones((), device=dev, dtype=torch.float32)

        def cost_and_grad(x):
            p = x.detach().requires_grad_(True)
            adv, m = ops.eot_paste(scene_imgs, p, mask, coeffs[0], l_pad, t_pad, self.scene_size)
            if plans is not None:
                cost = self._neg_cost(adv, m, plans[0], tabs[0], clean)
            else:
                cost = -ops.masked_sq_mean(self.model(adv), m)      # -MSE(adv_depth * mask, 0) (:176)
            (g,) = torch.autograd.grad(cost, p, grad_outputs=self._grad_seed(cost))
            return cost.detach().reshape(1), g

        # the state of attack_single_run (:148-200), all of it on the device
        loss0, g0 = cost_and_grad(x_adv)
        grad = g0.contiguous().clone()
        x_best, grad_best, x_old, x_ret = x_adv.clone(), grad.clone(), x_adv.clone(), x_adv.clone()
        ctl, hist, cursor, size_decr, steps_min = ops.apgd_controller(steps, self.eps, loss0, self.thr_decr)
        patches = [] if self.trace is not None else None

        def iteration():
            ops.apgd_step(x_adv, x_old, x0, grad, ctl, cursor, steps, self.eps)
            loss, g = cost_and_grad(x_adv)
            ops.apgd_commit(x_adv, g.contiguous(), grad, x_best, grad_best, x_ret, loss, ctl, hist, cursor, steps, size_decr,
                            steps_min, self.thr_decr)

        done = 0
        if self.use_graph and steps >= 2 and dev.type == "cuda" and not ops.profiling_every_launch():
            iteration()                 # eager: with the start point's pass it has filled every cache of the frozen-weights scope
            done = 1
            if patches is not None:
                patches.append(x_ret.clone())

            def traced():
                if self._capture_fault:     # test hook: a capture that dies before its first launch
                    raise RuntimeError("injected capture fault")
                iteration()

            # Every buffer the iteration updates is updated in place by the two K22 launches, so after a failed capture the
            # eager loop goes on from the state of the eager iteration.  The windows of this attack never move: the cells of
            # the cached clean features that a half-traced iteration left marked are exactly the cells the next paste
            # overwrites (no restore_head).
            g = self._capture_graph(traced, what="the attack iteration")
            if g is not None:
                for _ in range(1, steps):
                    g.replay()
                    if patches is not None:
                        patches.append(x_ret.clone())
                done = steps
                self._keep_graph(g)
        for _ in range(done, steps):
            iteration()
            if patches is not None:
                patches.append(x_ret.clone())

        if self.trace is not None:      # the record array IS the trace: one device-to-host copy, after the last iteration
            rec = ctl.cpu().numpy()
            for i in range(steps):
                now, nxt = rec[i], rec[i + 1]
                self.trace.append(dict(loss=float(nxt[8]), loss_best=float(nxt[2]), step_size=float(now[0]), k=int(now[4]),
                                       checkpoint=bool(nxt[9]), reduced=bool(nxt[10]), moved=bool(nxt[11]), n_rose=int(nxt[12]),
                                       patch=patches[i]))

        # x_best_adv of :255: the last iterate as it was before a possible restart
        return self._return_scenes(scene_imgs, x_ret, self.obj_img, mask, coeffs[1])
