"""What every attack on the object patch shares: the pair of PhysicalTrans, the pose draws in the reference's RNG order, the
window plans of the cost, the HIP-graph capture of one step, the two pastes of the returned scenes -- and, for the gradient-free
rows of the evaluation, the search loop.  An attack class adds its constructor, its draws and its per-step body (a search: how
one query's patch is composed on the device, and its host twin).
"""
import warnings
from random import sample

import numpy as np
import torch

from ... import ops
from ...my_utils import object_dataset_root, ori_H, ori_W, to_device_async
from ...physicalTrans import PhysicalTrans
from ...roi import RoiPlan, common_size_plans
from ..attack import Attack


class ObjectAttack(Attack):
    """Base of Phy_obj_atk (and, through it, of the evaluation rows) and of Phy_obj_atk_l0.  ``obj_img`` / ``obj_mask`` are kept
    as given: a subclass that wants its own copies clones them before it calls this constructor."""

    pose_group = None       # see Phy_obj_atk: _draw reads it

    def __init__(self, name, model, obj_img, obj_mask, dist_range):
        super().__init__(name, model)
        self.obj_img = obj_img
        self.obj_mask = obj_mask
        self.scene_size = [320, 1024]
        self.use_roi = True     # evaluate the cost on windows around the object when the model offers masked_sq_mean
        # Data-parallel "shared patch" mode: shard = (rank, world, process group or None).  The
        # reference attacks ONE patch on batch_size scenes per iteration (MD2/trainer.py:300-307, mono_dataset.py:178-184);
        # with a shard every rank holds scenes rank, rank + world, ... of that batch (``images`` = its own scenes), the pose
        # draws and the random start come from rank 0, and the patch gradient is summed over the ranks before the update:
        # all ranks end with the same patch -- the patch of the one-process attack on the concatenated scenes.
        self.shard = None
        # use_graph: give all steps of the attack the same window sizes (roi.common_size_plans), run step 0 eagerly, capture
        # step 1 in a HIP graph and replay it for the others -- ~130 kernel launches per step leave the host as ONE graph
        # launch (the step's Python + ctypes enqueue, ~2.5 ms, is what bounds a rank whose GPU share is small: DESIGN.md
        # section 7).  Same arithmetic as the eager loop on the same windows, bit for bit.  Off by default: at the headline
        # batch the GPU is the limiter and the common windows are a few per cent larger than each step's own.
        self.use_graph = False
        self.common_windows = False     # the common-size window plans without the graph (tests: the eager twin of use_graph)
        self.graph_failure = None       # why use_graph switched itself off (a failed capture), else None
        self._graph = None      # (graph of the previous attack, event behind its last replay): destroyed once it has run
        self._graph_pool = None
        self._capture_fault = False     # test hook: the subclass makes the capture of its step fail (where: see its ``traced``)
        self._model_negates = None      # does model.masked_sq_mean take negate=...?  (asked once)
        self._one = None                # the constant 1 handed to autograd.grad as d cost / d cost (made once per attack)
        conf = {'path': f'{object_dataset_root}/training/calib/003086.txt'}
        self.phy_trans_adv = PhysicalTrans(self.obj_img.clone(), self.obj_mask, conf, (1, 3, ori_H, ori_W),
                                           dist_range=dist_range)
        self.phy_trans_ben = PhysicalTrans(self.obj_img, self.obj_mask, conf, (1, 3, ori_H, ori_W),
                                           dist_range=dist_range)

    # --------------------------------------------------------------------------------------------------- prologue pieces
    @staticmethod
    def _check_batch(images, n_scenes):
        """One scene (broadcast inside the paste kernel, no torch.cat copy) or one per pose."""
        if images.size()[0] != 1 and images.size()[0] != n_scenes:
            raise RuntimeError('Batch size doesn\'t match!')

    @staticmethod
    def _eval_pose(z0_sample, alpha_sample, eval, dist=7):
        """In eval mode the first object of the returned scenes stands at a fixed distance, straight on."""
        if eval:
            z0_sample[0] = dist
            alpha_sample[0] = 0

    def _draw(self, batch_size, explicit=False):
        """One set of (z0, alpha) for ``batch_size`` scenes in the reference's RNG order: project()'s draw
        (physicalTrans.py:146-155), or with ``explicit`` the two ``sample`` calls of phy_obj_atk.py:108-109."""
        pt, g = self.phy_trans_ben, self.pose_group
        sizes = [batch_size] if not g or batch_size <= g else [min(g, batch_size - lo) for lo in range(0, batch_size, g)]
        z0s, als = [], []
        for n in sizes:
            z0, al = (sample(pt.dist_range, n), sample(pt.angle_range, n)) if explicit else pt.draw_samples(n)
            z0s += list(z0)
            als += list(al)
        return z0s, als

    def _coeffs(self, samples):
        """One device tensor [len(samples), B, 8] for a list of (z0, alpha) sample lists."""
        host = np.stack([self.phy_trans_ben.coeffs_for(z0, al) for z0, al in samples], 0)
        return to_device_async(host, self.device)

    # ------------------------------------------------------------------------------------------------------------- cost
    def _window_plans(self, draws, scene_imgs, mask, coeffs0, *, common=False, bind=True):
        """(plans, tabs, clean) for the pose sets ``draws``, or three Nones.  The cost reads the disparity under the object
        only: a model that can evaluate mean((disp * mask)^2) on windows around the object (DepthModelWrapper.masked_sq_mean:
        exact) gets one RoiPlan per pose set -- with ``common`` all of one size (roi.common_size_plans) where that is possible
        --, every origin table in ONE H2D copy, each plan tied to ITS slice of it (RoiPlan.bind_table; ``bind=False`` leaves
        that to a caller that replays one table buffer from a graph), and ``clean``: the frames without the object (a paste
        with an all-zero mask: scene (1 - 0) + patch 0, then the same Resize).  Every step's pasted frames equal them outside
        the step's boxes, so the model may start from their features."""
        if not (ops.ROI_ENABLED and self.use_roi and hasattr(self.model, "masked_sq_mean") and self.device.type == "cuda"):
            return None, None, None
        pt = self.phy_trans_ben
        boxes = [pt.mask_boxes(z0, al, self.scene_size) for z0, al in draws]
        plans = common_size_plans(boxes, *self.scene_size, depth=ops.ROI_DEPTH) if common else None
        if plans is None:
            plans = [RoiPlan(b, *self.scene_size, depth=ops.ROI_DEPTH) for b in boxes]
        tabs = to_device_async(np.stack([p.table() for p in plans], 0), self.device)
        if bind:
            self._bind_tables(plans, tabs)
        with torch.no_grad():
            clean, _ = ops.eot_paste(scene_imgs, self.obj_img, torch.zeros_like(mask), coeffs0, pt.l_pad, pt.t_pad,
                                     self.scene_size)
        return plans, tabs, clean

    @staticmethod
    def _one_size(plans):
        """Do all plans launch the same kernels on tensors of the same shapes (what roi.common_size_plans hands out)?"""
        return len({(tuple(sorted(p.size.items())), p.layer2_incremental_ok, p.head_incremental_ok) for p in plans}) == 1

    @staticmethod
    def _bind_tables(plans, tabs):
        """Every plan reads its own slice of the stacked table (again, after a graph that rewrote plans[0]'s buffer in place)."""
        plans[0].table_rewritten = False
        for p_, t_ in zip(plans, tabs):
            p_.bind_table(t_)

    def _neg_cost(self, adv, m, plan, tab, clean):
        """-mean((disp * mask)^2) on the plan's windows (phy_obj_atk.py:94-95); a model whose masked_sq_mean takes ``negate``
        applies the sign inside its cost kernel (no element-wise launch for it, forward or backward)."""
        if self._model_negates is None:
            import inspect
            try:
                self._model_negates = "negate" in inspect.signature(self.model.masked_sq_mean).parameters
            except (TypeError, ValueError):
                self._model_negates = False
        if self._model_negates:
            return self.model.masked_sq_mean(adv, m, plan, tab, clean, negate=True)
        return -self.model.masked_sq_mean(adv, m, plan, tab, clean)

    def _grad_seed(self, cost):
        """d cost / d cost = 1 for autograd.grad as the tensor made once per attack (``self._one``; autograd otherwise fills a
        fresh one-element tensor per step: one more launch in a chain of ~120 short dependent ones)."""
        return self._one if cost.dim() == 0 and cost.dtype == torch.float32 else None

    # ------------------------------------------------------------------------------------------------------ graph capture
    def _capture_graph(self, traced, *, what, restore_head=False):
        """``traced()`` -- one step of the attack, reading its pose and its patch from fixed device buffers -- as a HIP graph,
        or None after a failed capture, with ``graph_failure`` set, ``use_graph`` switched off (a stack that cannot capture
        this step will not capture the next attack's either) and a warning that names ``what``.  Capture goes through
        CUDAGraph.capture_begin / capture_end on a side stream -- ``with torch.cuda.graph()`` synchronises the device and
        empties the allocator's cache on entry, once per attack here -- into a memory pool this attack object keeps, so that
        the graph of the next attack reuses the blocks of this one.  A capture executes nothing: after a failure the device
        holds the state the last eager step left, and the caller's eager loop goes on from there.  What tracing changes on the
        Python side is the bookkeeping of the incremental encoder head (ops.CleanHead: which window is dirty, its generation,
        its private origin copies) and the frozen-weights cache, which may gain entries that point at pool memory no kernel
        ever wrote: ``restore_head`` snapshots both before the capture and puts them back after a failed one."""
        dev = self.device
        if self._graph is not None:         # the previous attack's graph: let its last replay finish before it is destroyed
            self._graph[1].synchronize()
            self._graph = None
        main = torch.cuda.current_stream(dev)
        pool, side = self._capture_pool(main)
        side.wait_stream(main)
        g = torch.cuda.CUDAGraph()
        snap = ops.clean_head_snapshot() if restore_head else None
        try:
            with torch.cuda.stream(side):
                ops._sk_workspace(dev)                      # this stream's stream-K workspace: allocated outside the capture
                # thread_local: a HIP call of ANOTHER thread (the process group's watchdog, the all-reduce still in flight on the
                # bucket's stream in the trainer's overlap mode) must not invalidate this thread's capture
                g.capture_begin(pool=pool, capture_error_mode="thread_local")
                try:
                    traced()
                except BaseException:
                    try:
                        g.capture_end()                     # ends the (invalidated) capture; its own error adds nothing
                    except Exception:
                        pass
                    raise
                g.capture_end()
        except RuntimeError as e:
            main.wait_stream(side)
            if restore_head:
                ops.clean_head_restore(snap)
            self.use_graph = False
            self.graph_failure = "%s: %s" % (type(e).__name__, str(e).splitlines()[0] if str(e) else "")
            warnings.warn("%s: HIP-graph capture of %s failed (%s); continuing with eager launches"
                          % (type(self).__name__, what, self.graph_failure))
            return None
        main.wait_stream(side)
        return g

    def _keep_graph(self, g):
        """After the last replay: the graph lives until the next capture (or the attack object) retires it behind this event."""
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.device))
        self._graph = (g, done)

    def _capture_pool(self, main):
        """(memory pool, side stream) this attack object captures its graphs into, made at the first capture."""
        if self._graph_pool is None:
            dev = self.device
            # the allocator drops a pool with its last graph: a one-kernel graph that is never destroyed keeps this one
            pool, side, keeper = torch.cuda.graph_pool_handle(), torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                keeper.capture_begin(pool=pool)
                try:
                    torch.zeros(8, device=dev)
                finally:
                    keeper.capture_end()
            self._graph_pool = (pool, side, keeper)
        return self._graph_pool[0], self._graph_pool[1]

    # ------------------------------------------------------------------------------------------------------------ epilogue
    def _return_scenes(self, scene_imgs, adv_patch, clean_obj, mask, coeff):
        """The attack's return tuple: the scenes with ``adv_patch`` and with ``clean_obj`` pasted at the poses of ``coeff``
        (two K3 launches), the pasted masks, the patch -- which phy_trans_adv pastes from now on."""
        pt = self.phy_trans_ben
        self.phy_trans_adv.reset_img(adv_patch, self.obj_mask)
        with torch.no_grad():
            adv_scenes, obj_masks_out = ops.eot_paste(scene_imgs, adv_patch, mask, coeff, pt.l_pad, pt.t_pad, self.scene_size)
            ben_scenes, _ = ops.eot_paste(scene_imgs, clean_obj, mask, coeff, pt.l_pad, pt.t_pad, self.scene_size)
        return adv_scenes, ben_scenes, obj_masks_out, adv_patch
