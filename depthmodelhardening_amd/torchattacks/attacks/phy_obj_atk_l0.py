"""L0 physical-object attack: two non-negative pattern tensors optimised with Adam under a tanh
sparsity penalty that an L0-ratio threshold switches on and off.

Same surface as the reference's ``torchattacks/attacks/phy_obj_atk_l0.py:16-174``.  Per iteration:
K5 l0_compose (pattern clamp/compose + thresholded L0 count, one launch) -> K3 eot_paste -> model ->
K6 masked_sq_mean + K5 l0_mask_cost -> autograd -> Adam.  The reference reads the L0 ratio on the host
every iteration (:105-111, a device sync); here the mask weight is selected ON DEVICE and the host only
looks at the ratio when it can end the loop (stp >= steps).
"""
import random
from random import sample

import numpy as np
import torch
import torch.nn.functional as F

from ... import color_jitter, ops
from ...my_utils import object_dataset_root, ori_H, ori_W, to_device_async
from .object_attack import ObjectAttack


def host_below(counts, stp, thresh):
    """The fused attack's decision for iteration ``stp`` from a host copy of its count array, in float32 exactly as K23
    evaluates it on the device (csrc/l0_fused.hip, l0_below): count[stp] / count[0] <= thresh."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(np.float32(counts[stp]) / np.float32(counts[0]) <= np.float32(thresh))


class Phy_obj_atk_l0(ObjectAttack):
    r"""
    Distance Measure : L_0
    """

    def __init__(self, model, obj_img, obj_mask, adam_lr=0.5, steps=10, mask_wt=0.1, l0_thresh=1 / 10,
                 dist_range=list(range(5, 31, 2))):
        super().__init__("PGD", model, obj_img.clone().detach(), obj_mask.clone().detach(), dist_range)
        self.steps = steps
        self.clip_max = 1
        self.learning_rate = adam_lr
        self.mask_weight_init = mask_wt
        self.mask_weight = self.mask_weight_init
        self.l0_thresh = l0_thresh
        self.l0_clip = self.clip_max / 255.
        # ONE random colour transform per attack object, drawn here as the reference does (:41; four random.uniform + one
        # random.shuffle of the global ``random`` generator), applied by forward(..., color_jit=True)
        self.color_aug = color_jitter.get_params((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1))
        self.trace = None  # set to a list to record (l0, mask_weight, adv_cost, mask_cost) per iteration
        self.grad_trace = None  # set to a list to record the two pattern gradients Adam is handed, per iteration (tests)
        # fused: everything between the model's gradient and the next composed patch is ONE launch (K23, csrc/l0_fused.hip) that
        # reads its decisions from device memory -- no torch.optim.Adam, no torch.where, no autograd node for the mask cost; the
        # trace is read once after the loop from K23's record array (kept in ``records``).  Off by default.
        self.fused = False
        # use_graph / common_windows (ObjectAttack): one set of window sizes for all 2 * steps draws, iteration 0 eager,
        # iteration 1 captured in a HIP graph, later iterations two small device copies + a replay.  Implies ``fused``.
        # _capture_fault makes that capture fail after the whole iteration has been traced.
        self.records = None             # K23's record array [2 * steps, ops.L0_REC] of the last fused attack (device)
        self.graph_replays = 0          # how many iterations of the last attack were graph replays

    def cal_l0(self):
        """Number of pixels whose thresholded pattern is non-zero (:43-52), as a device tensor."""
        _, count = ops.l0_compose(self.obj_img, self.pattern_pos_tensor.detach(), self.pattern_neg_tensor.detach(),
                                  self.l0_clip)
        return count[0]

    def forward(self, images, batch_size, cfg_path=f'{object_dataset_root}/training/calib/003086.txt', eval=False,
                color_jit=False):
        img_B, img_C, img_H, img_W = images.size()
        if img_H != ori_H or img_W != ori_W:
            images = F.interpolate(images, size=[ori_H, ori_W], mode="bilinear", align_corners=False)
            print("image size inconsistent in l0 attack")
        images = images.detach().to(self.device)
        # data-parallel "shared patch" mode (see Phy_obj_atk.shard): this rank holds scenes rank, rank + world, ... of the
        # batch; rank 0's initial patterns and pose draws are the job's; the two pattern gradients are summed over the ranks
        mine, share, world, group, src = None, 1.0, 1, None, 0
        if self.shard is not None:
            import torch.distributed as dist
            rank, world, group = self.shard
            src = dist.get_global_rank(group, 0) if group is not None else 0
            mine = list(range(rank, batch_size, world))
            if not mine:
                raise RuntimeError("Phy_obj_atk_l0.shard: more ranks than attack scenes is not supported")
            share = len(mine) / float(batch_size)
        if self.shard is not None and (self.fused or self.use_graph):
            raise NotImplementedError("Phy_obj_atk_l0: shard together with fused / use_graph is not built (the sharded attack's "
                                      "two all-reduces sit between the backward kernels the fused update replaces)")
        if color_jit and self.use_graph:
            raise NotImplementedError("Phy_obj_atk_l0: color_jit=True together with use_graph is not built (the colour "
                                      "augmentation takes the whole-frame path; fused alone works with it)")
        if self.grad_trace is not None and (self.fused or self.use_graph):
            raise NotImplementedError("Phy_obj_atk_l0: grad_trace belongs to the unfused path (the fused update never "
                                      "materialises the pattern gradients)")
        n_local = batch_size if mine is None else len(mine)
        self._check_batch(images, n_local)
        scene_imgs = images

        # numpy RNG on the host, exactly as the reference (:73-83)
        pats = []
        for _ in range(2):
            init_pattern = np.random.random(self.obj_img.size()) * self.clip_max
            init_pattern = np.clip(init_pattern, 0.0, self.clip_max) / self.clip_max
            t = torch.Tensor(init_pattern).to(self.device)
            if mine is not None:
                dist.broadcast(t, src=src, group=group)
            t.requires_grad = True
            pats.append(t)
        self.pattern_pos_tensor, self.pattern_neg_tensor = pats
        optimizer = torch.optim.Adam([self.pattern_pos_tensor, self.pattern_neg_tensor], lr=self.learning_rate,
                                     betas=(0.5, 0.9))

        pt = self.phy_trans_ben
        max_iter = self.steps * 2
        # All (z0, alpha) draws up front -> one H2D copy of the homographies.  The reference only consumes
        # a project() draw for iterations it actually runs, so the RNG state after each iteration's draws
        # is kept and restored if the loop ends early: later draws then match the reference draw for draw.
        draws, rng_states = [], [random.getstate()]
        for _ in range(max_iter):
            draws.append(pt.draw_samples(batch_size))
            rng_states.append(random.getstate())
        # The poses of the returned scenes (:161-163) are drawn AFTER the loop, i.e. from the RNG state that follows the draws
        # of the iterations that really ran (steps ... 2 steps of them, known only at the end).  One candidate per possible
        # count, each with the state it leaves behind: the loop's exit picks its own, and later draws continue from there --
        # in the one-process attack and, with rank 0's candidates broadcast, in the sharded one alike.
        finals, states_after = {}, {}
        for r in range(self.steps, max_iter + 1):
            random.setstate(rng_states[r])
            z0_f, al_f = sample(pt.dist_range, batch_size), sample(pt.angle_range, batch_size)
            self._eval_pose(z0_f, al_f, eval, dist=6.1)     # GLOBAL scene 0's (:165-167): before the scenes are dealt out
            finals[r], states_after[r] = (z0_f, al_f), random.getstate()
        if mine is not None:        # the job's draws are rank 0's (the final pose draws included); keep the own scenes' poses
            box = [(draws, finals)]
            dist.broadcast_object_list(box, src=src, group=group)
            draws = [([z[i] for i in mine], [a[i] for i in mine]) for z, a in box[0][0]]
            finals = {r: ([z[i] for i in mine], [a[i] for i in mine]) for r, (z, a) in box[0][1].items()}
            batch_size = n_local
        coeffs = self._coeffs(draws)
        l_pad, t_pad = pt.l_pad, pt.t_pad
        mask = self.obj_mask.to(self.device)
        # the adversarial cost on windows around the object (ObjectAttack._window_plans), one set of sizes for all 2 * steps
        # draws where a graph or its eager twin asks for it.  Not with color_jit: the whole frame changes with the patch -- the
        # contrast step blends with the pasted image's mean -- so neither the windows' "unchanged outside the box" nor the
        # cached clean-frame features hold: whole-frame path
        plans = tabs = clean = None
        if not color_jit:
            plans, tabs, clean = self._window_plans(draws, scene_imgs, mask, coeffs[0],
                                                    common=self.use_graph or self.common_windows)
        if self.fused or self.use_graph:
            ran, mw = self._fused_loop(scene_imgs, mask, coeffs, l_pad, t_pad, plans, tabs, clean, color_jit, max_iter)
        else:
            thresh = torch.full((), float(self.l0_thresh), device=self.device)      # fill kernels: no host sync
            w_on = torch.full((), float(self.mask_weight_init), device=self.device)
            w_off = torch.zeros((), device=self.device)
            l0_norm_init = None
            mw = w_on
            ran = 0
            for stp in range(max_iter):
                obj_img_adv, l0_norm = ops.l0_compose(self.obj_img, self.pattern_pos_tensor, self.pattern_neg_tensor,
                                                      self.l0_clip)
                if stp == 0:
                    l0_norm_init = l0_norm
                below = (l0_norm.float() / l0_norm_init.float())[0] <= thresh
                if stp >= self.steps and bool(below):  # the only host read of the ratio (:106-109)
                    mw = w_off
                    break
                mw = torch.where(below, w_off, w_on)
                adv_scenes, adv_obj_mask = ops.eot_paste(scene_imgs, obj_img_adv, mask, coeffs[stp], l_pad, t_pad,
                                                         self.scene_size)
                if plans is not None:
                    adv_cost = self.model.masked_sq_mean(adv_scenes, adv_obj_mask, plans[stp], tabs[stp], clean)
                else:
                    if color_jit:       # :122-124 (off the hot path: composed from tensor operations, see color_jitter.py)
                        adv_scenes = self.color_aug(adv_scenes)
                    adv_depth = self.model(adv_scenes)
                    adv_cost = ops.masked_sq_mean(adv_depth, adv_obj_mask)
                mask_cost = ops.l0_mask_cost(self.pattern_pos_tensor, self.pattern_neg_tensor)
                total_cost = adv_cost + mw * mask_cost
                if mine is not None:    # this rank's part of the job's cost: the sum over the ranks below is the one-process gradient
                    total_cost = adv_cost * share + mw * mask_cost * (1.0 / world)
                # same update as zero_grad(); total_cost.backward(); step() (:136-138), but only the two
                # pattern tensors get gradients: the reference's backward() also fills (and later discards)
                # weight gradients of the attacked model -- a third of the conv backward work
                g_pos, g_neg = torch.autograd.grad(total_cost, [self.pattern_pos_tensor, self.pattern_neg_tensor])
                if mine is not None:
                    dist.all_reduce(g_pos, op=dist.ReduceOp.SUM, group=group)
                    dist.all_reduce(g_neg, op=dist.ReduceOp.SUM, group=group)
                if self.grad_trace is not None:
                    self.grad_trace.append((g_pos.detach().clone(), g_neg.detach().clone()))
                self.pattern_pos_tensor.grad, self.pattern_neg_tensor.grad = g_pos, g_neg
                optimizer.step()
                ran += 1
                if self.trace is not None:
                    self.trace.append((int(l0_norm), float(mw), float(adv_cost), float(mask_cost)))
        random.setstate(states_after[ran])     # as if only the iterations that ran, and then the final poses, had drawn
        # the loop runs ``steps`` ... 2 ``steps`` iterations, by the patch's L0 ratio (:105-109): callers that time the attack
        # (bench.py) report how many it ran
        self.total_iterations = getattr(self, "total_iterations", 0) + ran
        self.total_calls = getattr(self, "total_calls", 0) + 1

        with torch.no_grad():
            obj_img_adv, _ = ops.l0_compose(self.obj_img, self.pattern_pos_tensor.detach(),
                                            self.pattern_neg_tensor.detach(), self.l0_clip, finalize=True)
        self.mask_weight = float(mw)
        cf = to_device_async(pt.coeffs_for(*finals[ran]), self.device)
        return self._return_scenes(scene_imgs, obj_img_adv, self.obj_img, mask, cf)

    # ------------------------------------------------------------------------------------------------ fused path (K23)
    def _fused_loop(self, scene_imgs, mask, coeffs, l_pad, t_pad, plans, tabs, clean, color_jit, max_iter):
        """Iterations of the attack with K23 as the update: eot_paste -> cost -> autograd.grad(adv_cost, patch) -> l0_fused_step.
        Iterations below ``steps`` read nothing back; from ``steps`` on the host reads the count array before each iteration
        and ends the loop as the reference does (:105-109).  Returns (iterations run, last mask weight)."""
        dev = self.device
        obj = self.obj_img.to(dev).contiguous()
        st = ops.L0FusedState(self.pattern_pos_tensor, self.pattern_neg_tensor, self.steps, self.learning_rate)
        self.pattern_pos_tensor, self.pattern_neg_tensor = st.pos, st.neg     # plain device buffers, updated in place
        with torch.no_grad():           # iteration 0's patch and count[0] (K5); every later one comes out of K23
            adv0, c0 = ops.l0_compose(obj, st.pos, st.neg, self.l0_clip)
            st.adv.copy_(adv0)
            st.count[:1].copy_(c0)
        self._one = torch.ones((), device=dev, dtype=torch.float32)
        tracing = self.trace is not None
        mask_wt, thresh = float(self.mask_weight_init), float(self.l0_thresh)

        def iteration(coeff, plan, tab):
            p = st.adv.detach().requires_grad_(True)
            adv_scenes, adv_obj_mask = ops.eot_paste(scene_imgs, p, mask, coeff, l_pad, t_pad, self.scene_size)
            if plan is not None:
                adv_cost = self.model.masked_sq_mean(adv_scenes, adv_obj_mask, plan, tab, clean)
            else:
                if color_jit:
                    adv_scenes = self.color_aug(adv_scenes)
                adv_cost = ops.masked_sq_mean(self.model(adv_scenes), adv_obj_mask)
            (g,) = torch.autograd.grad(adv_cost, p, grad_outputs=self._grad_seed(adv_cost))
            mask_cost = None
            if tracing:
                with torch.no_grad():
                    mask_cost = ops.l0_mask_cost(st.pos, st.neg)
            st.step(obj, g.contiguous(), adv_cost.detach(), mask_cost, mask_wt, thresh, self.l0_clip)

        def traced():
            iteration(coeff_cur, plans[0], tab_cur)
            if self._capture_fault:     # test hook: a capture that dies after the whole iteration has been traced
                raise RuntimeError("injected capture fault")

        graph_mode = bool(self.use_graph and plans is not None and dev.type == "cuda" and not ops.profiling_every_launch())
        coeff_cur = tab_cur = g = None
        if graph_mode:      # the captured iteration reads its pose from fixed buffers (see Phy_obj_atk._graph_steps)
            coeff_cur, tab_cur = coeffs[0].clone(), tabs[0].clone()
            plans[0].bind_table(tab_cur)
            plans[0].table_rewritten = True
        self.graph_replays = 0
        ran, exited, counts = 0, False, None
        for stp in range(max_iter):
            if stp >= self.steps:       # the only host read of the loop (:106-109)
                counts = st.count.cpu().numpy()
                if host_below(counts, stp, self.l0_thresh):
                    exited = True
                    break
            if graph_mode and stp > 0:
                coeff_cur.copy_(coeffs[stp])
                tab_cur.copy_(tabs[stp])
                if g is None:
                    # restore_head: tracing the iteration runs the Python-side bookkeeping of the incremental encoder head,
                    # and these windows move from iteration to iteration
                    g = self._capture_graph(traced, what="the attack iteration", restore_head=True)
                    if g is None:       # the capture failed: the eager loop takes over on the same common-size plans
                        graph_mode = False
                        self._bind_tables(plans, tabs)
            if graph_mode and stp > 0:
                g.replay()
                self.graph_replays += 1
            elif graph_mode:
                iteration(coeff_cur, plans[0], tab_cur)     # iteration 0, eager: it fills the caches of the frozen-weights scope
            elif plans is not None:
                iteration(coeffs[stp], plans[stp], tabs[stp])
            else:
                iteration(coeffs[stp], None, None)
            ran += 1
        if g is not None:
            self._keep_graph(g)
        self.records = st.rec
        rec = st.rec[:ran].cpu().numpy() if (tracing or not exited) and ran else None
        if tracing and rec is not None:
            for r in rec:
                self.trace.append((int(r[0]), float(r[1]), float(r[2]), float(r[3])))
        mw = 0.0 if exited or rec is None else float(rec[ran - 1][1])
        return ran, mw
