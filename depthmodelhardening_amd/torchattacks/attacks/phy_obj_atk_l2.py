"""PGD-L2 attack on one shared object patch: the ``norm_type == "l_2"`` row of the reference's ``evaluate_attacks``
(``MD2/evaluate_depth.py:133-137``).

Same class name, constructor, call signature and return tuple as the reference's ``torchattacks/attacks/phy_obj_atk_l2.py``.
Its pose draws, paste, cost and returned scenes are ``Phy_obj_atk``'s line for line (:94-138 against phy_obj_atk.py:83-121), so
this class is ``Phy_obj_atk`` with two pieces swapped:

    the random start   :83-90    a normal draw scaled to the norm  r eps,  r ~ U(0, 1), then the clamp to [0, 1]
    the update         :110-120  K28 pgd_l2_step (two launches) instead of K4

The shared-patch form.  The reference views the gradient of the ONE patch [1,3,H,W] as ``batch_size`` rows (:110) and divides by
[B,1,1,1] norms (:111): with B > 1 the "patch" is [B,3,H,W] after the first step and the next paste no longer fits its masks, so
the class as written runs at ``batch_size == 1`` (or ``steps == 1``) only -- tests/golden/atk_l2.npz records what happens at
B = 2.  At B = 1 it is an ordinary L2 PGD on the shared patch, and that is what is built here for every B: one patch, one norm over
the whole patch, the cost averaged over the B scenes.

Quirks kept: the constructor takes ``alpha`` and ignores it (``self.alpha = 2.5 * eps / steps``, :44); ``eps_for_division`` is
added to the gradient norm only; ``eps / ||delta||`` divides by an unguarded norm (``eps / 0 = inf`` gives the factor 1).  The
``print`` of the step loop (:100) is not reproduced.  Evaluation only: ``shard`` is refused.
"""
import torch

from ... import ops
from ...my_utils import object_dataset_root
from .phy_obj_atk import Phy_obj_atk


class Phy_obj_atk_l2(Phy_obj_atk):
    r"""
    Distance Measure : L2

    Arguments:
        model (nn.Module): model to attack.
        obj_img (1x3xHxW), obj_mask (1x1xHxW): object patch and its paint mask.
        eps (float): maximum perturbation, the L2 norm over the whole patch. (Default: 1)
        alpha (float): ignored, as in the reference: the step size is 2.5 * eps / steps.
        steps (int): number of steps. (Default: 40)
        random_start (bool): using random initialization of delta. (Default: True)
    """

    def __init__(self, model, obj_img, obj_mask, eps=1,
                 alpha=0.2, steps=40, random_start=True, dist_range=list(range(5, 31, 2))):
        super().__init__(model, obj_img, obj_mask, eps=eps, alpha=2.5 * eps / steps, steps=steps, random_start=random_start,
                         dist_range=dist_range)
        self.eps_for_division = 1e-10
        # test hook: a pair (normal tensor shaped like the patch, r) here replaces the normal_() and uniform_(0, 1) draws
        self.random_start_noise = None
        # measurement hook (tools/l2_eval_bench.py): the update as the reference's chain of torch expressions instead of K28
        self.torch_step = False
        self._workspace = None      # K28's partial sums: allocated once per attack object, outside any graph capture

    def _random_start(self, obj_img_adv):
        """:83-88: delta = normal * (r / ||normal||_2 * eps)."""
        if self.random_start_noise is not None:
            delta, r = self.random_start_noise
            delta = delta.to(self.device).clone()
            r = torch.as_tensor(r, dtype=delta.dtype).reshape(obj_img_adv.size(0), 1, 1, 1).to(self.device)
        else:
            delta = torch.empty_like(obj_img_adv).normal_()
            r = None
        d_flat = delta.view(obj_img_adv.size(0), -1)
        n = d_flat.norm(p=2, dim=1).view(obj_img_adv.size(0), 1, 1, 1)
        if r is None:
            r = torch.zeros_like(n).uniform_(0, 1)
        delta *= r / n * self.eps
        return delta

    def _step(self, x, grad, out=None):
        if self.torch_step:
            res = self._torch_step(x.detach(), grad)
            return res if out is None else out.copy_(res)
        return ops.pgd_l2_step(x, self.obj_img, grad, self.alpha, self.eps, out=out, workspace=self._workspace)

    def _torch_step(self, x, grad):
        """:110-120 with one row: the reference's expressions at batch_size = 1."""
        grad_norms = torch.norm(grad.view(1, -1), p=2, dim=1) + self.eps_for_division
        grad = grad / grad_norms.view(1, 1, 1, 1)
        x = x + self.alpha * grad
        delta = x - self.obj_img
        delta_norms = torch.norm(delta.view(1, -1), p=2, dim=1)
        factor = self.eps / delta_norms
        factor = torch.min(factor, torch.ones_like(delta_norms))
        delta = delta * factor.view(-1, 1, 1, 1)
        return torch.clamp(self.obj_img + delta, min=0, max=1).detach()

    def forward(self, images, batch_size, cfg_path=f'{object_dataset_root}/training/calib/003086.txt', eval=False):
        if self.shard is not None:
            raise NotImplementedError("Phy_obj_atk_l2 is an evaluation attack: shard (the data-parallel shared-patch mode of "
                                      "training) is not built for it")
        if self._workspace is None and self.obj_img.is_cuda:
            self._workspace = ops.pgd_l2_workspace(self.obj_img.numel(), self.obj_img.device)
        return super().forward(images, batch_size, cfg_path, eval)
