"""CPU restatement of the reference's L2 physical-object attack in its shared-patch form, a test helper.

Reference: torchattacks/attacks/phy_obj_atk_l2.py -- the random start :83-90, the step loop :94-120, the returned scenes :123-140
-- under Attack.__call__'s eval()/train() bracket.  Plain torch with the reference's own expressions, in the dtype of the inputs:
called on fp32 tensors it is the fp32 form, on float64 tensors the float64 form that the 20 e_ref rule is anchored to.  Written
on the pieces of oracle/attack_ref (PhysicalTransRef, paste) and the toy model, seeds and scenes that tests/square_ref.py uses.

The shared-patch form: ONE patch [1, 3, H, W], one norm over the whole patch (the reference's ``view(batch_size, -1)`` at
batch_size = 1), the cost averaged over the B scenes.  At B = 1 this is the reference's code expression for expression;
tests/golden/atk_l2.npz (tools/make_goldens_l2.py) holds the reference's own run at B = 1 and what it does at B = 2.

Also here, because the fixture generator and the tests must agree on them: the fixture's inputs (``CASE``).
"""
import random

import numpy as np
import torch
import torch.nn as nn

from oracle import attack_ref, synth, tv082
from tests.square_ref import REGION, depth_cost, make_model, seed_all  # noqa: F401

# inputs of the fixture: the reference at B = 1 (and the probe at B = 2) on the 260 x 300 object; eps as in the reference's own
# l_2 rows (MD2/evaluate_depth.py:467-486: 8, 16, 24); 3 steps make alpha = 2.5 eps / 3 > eps / 2, so the projection acts
CASE = dict(model_seed=5, gain=6.0, scene_seed=47, steps=3, eps=8.0, rng_seed=67)
EPS_FOR_DIVISION = 1e-10


def case_inputs(batch, case=CASE):
    obj, mask = synth.make_object()
    scenes = synth.kitti_like(batch, 3, 375, 1242, torch.Generator().manual_seed(case["scene_seed"]))
    return obj, mask, scenes


def draw_start(obj):
    """(normal, r) from torch's CPU generator in the reference's order (:83, :86)."""
    normal = torch.empty_like(obj).normal_()
    r = torch.zeros(obj.size(0), 1, 1, 1, dtype=obj.dtype).uniform_(0, 1)
    return normal, r


def random_start(obj, normal, r, eps):
    """:83-90 on draws made earlier: the start patch."""
    delta = normal.clone().to(obj.dtype)
    d_flat = delta.view(obj.size(0), -1)
    n = d_flat.norm(p=2, dim=1).view(obj.size(0), 1, 1, 1)
    delta *= r.to(obj.dtype).view(obj.size(0), 1, 1, 1) / n * eps
    return torch.clamp(obj + delta, min=0, max=1).detach()


def step(x, x0, grad, alpha, eps):
    """:110-120 with one row (batch_size = 1), any shape: the tensors are flattened to one row for the two norms."""
    rows = 1
    grad_norms = torch.norm(grad.reshape(rows, -1), p=2, dim=1) + EPS_FOR_DIVISION
    grad = grad / grad_norms.view([rows] + [1] * (grad.dim() - 1))
    x = x.detach() + alpha * grad
    delta = x - x0
    delta_norms = torch.norm(delta.reshape(rows, -1), p=2, dim=1)
    factor = eps / delta_norms
    factor = torch.min(factor, torch.ones_like(delta_norms))
    delta = delta * factor.view([-1] + [1] * (delta.dim() - 1))
    return torch.clamp(x0 + delta, min=0, max=1).detach()


def step_alpha(eps, steps):
    return 2.5 * eps / steps        # :44: the constructor's alpha is ignored


def phy_obj_atk_l2(model, obj_img, obj_mask, images, batch_size, eps=1, steps=40, random_start_draw=None, dist_range=None,
                   eval=False, P2=attack_ref.KITTI_P2, trace=None, draws=None, final_draw=None):
    """Returns (adv_scenes, ben_scenes, obj_masks_out, adv_patch) in the dtype of ``obj_img``.  ``random_start_draw``: (normal,
    r) made earlier, None draws them here, False starts from the clean patch.  ``trace``: a list that receives per step a dict
    with ``cost`` (the reference's, negative), ``grad`` and ``patch`` (after the step).  ``draws`` / ``final_draw``: poses made
    earlier instead of project()'s ``random.sample``."""
    dist_range = list(range(5, 31, 2)) if dist_range is None else dist_range
    alpha = step_alpha(eps, steps)
    given_training = model.training
    model.eval()
    trans_adv = attack_ref.PhysicalTransRef(obj_img.clone(), obj_mask, P2, dist_range=dist_range)
    trans_ben = attack_ref.PhysicalTransRef(obj_img, obj_mask, P2, dist_range=dist_range)
    scene_imgs = attack_ref._tile_scene(images.detach(), batch_size)
    loss = nn.MSELoss()
    adv = obj_img.clone().detach()
    if random_start_draw is not False:
        normal, r = draw_start(obj_img) if random_start_draw is None else random_start_draw
        adv = random_start(obj_img, normal, r, eps)
    target = torch.zeros((batch_size, 1) + tuple(attack_ref.SCENE_SIZE), dtype=obj_img.dtype)
    for s in range(steps):
        adv.requires_grad_()
        trans_adv.reset_img(adv, obj_mask)
        z0_i, al_i = draws[s] if draws is not None else (None, None)
        adv_scenes, masks, _, _, _ = attack_ref.paste(scene_imgs, trans_adv, batch_size, z0_i, al_i)
        cost = -loss(model(adv_scenes) * masks, target)
        grad = torch.autograd.grad(cost, adv, retain_graph=False, create_graph=False)[0]
        adv = step(adv, obj_img, grad, alpha, eps)
        if trace is not None:
            trace.append(dict(cost=float(cost.detach()), grad=grad.detach().clone(), patch=adv.clone()))
    trans_adv.reset_img(adv, obj_mask)
    if final_draw is not None:
        z0, al = list(final_draw[0]), list(final_draw[1])
    else:
        z0 = random.sample(trans_ben.dist_range, batch_size)
        al = random.sample(trans_ben.angle_range, batch_size)
    if eval:
        z0[0], al[0] = 7, 0
    adv_scenes, _, full_mask, _, _ = attack_ref.paste(scene_imgs, trans_adv, batch_size, z0, al)
    obj_ben, _, _, _ = trans_ben.project(batch_size=batch_size, z0_sample=z0, alpha_sample=al)
    ben_scenes = tv082.resize(scene_imgs * (1 - full_mask) + obj_ben * full_mask, attack_ref.SCENE_SIZE)
    masks_out = tv082.resize(full_mask, attack_ref.SCENE_SIZE)
    if given_training:
        model.train()
    return adv_scenes, ben_scenes, masks_out, adv


def draw_poses(dist_range, angle_range, steps, batch_size):
    """steps + 1 (z0, alpha) sets from Python's global generator in the reference's order: one project() per step
    (physicalTrans.py:150,155), then the two samples of :125-126."""
    return [(random.sample(dist_range, batch_size), random.sample(angle_range, batch_size)) for _ in range(steps + 1)]


def norms_of(trace, obj):
    return np.asarray([float((t["patch"].double() - obj.double()).norm()) for t in trace])


# --------------------------------------------------------------------------- the kernel's input cases (tests/test_gpu_l2.py)
KERNEL_SIZES = (1, 3, 5, 255, 256, 257, 1023, 3 * 260 * 300, (1 << 20) + 3)
KERNEL_CASES = ("inside", "outside", "zero_grad", "zero_grad_at_x0", "clamps")


def kernel_case(name, n, seed=0):
    """(x, x0, g, alpha, eps) fp32 on the CPU for one of KERNEL_CASES.  eps scales with sqrt(n), so that every size meets the
    case's regime: "inside" keeps ||y - x0|| below eps (factor 1), "outside" lands beyond it (factor < 1), "clamps" pushes values
    of x0 near 0 and near 1 across both bounds of [0, 1]."""
    g_ = torch.Generator().manual_seed(1000 * seed + n % 997 + 17 * KERNEL_CASES.index(name))
    root = float(n) ** 0.5
    x0 = torch.rand(n, generator=g_) * 0.8 + 0.1
    grad = torch.randn(n, generator=g_) * 1e-3
    if name == "inside":
        eps, alpha = 0.05 * root, 0.01 * root
        x = x0 + (torch.rand(n, generator=g_) * 2 - 1) * 0.02
    elif name == "outside":
        eps, alpha = 0.05 * root, 0.04 * root
        x = x0 + torch.sign(grad) * 0.03 * (1 + torch.rand(n, generator=g_))     # along the step: the two add up at every n
    elif name == "zero_grad":
        eps, alpha = 0.05 * root, 0.02 * root
        x = x0 + (torch.rand(n, generator=g_) * 2 - 1) * 0.03
        grad = torch.zeros(n)
    elif name == "zero_grad_at_x0":
        eps, alpha = 0.05 * root, 0.02 * root
        x = x0.clone()
        grad = torch.zeros(n)
    elif name == "clamps":
        eps, alpha = 0.5 * root, 0.3 * root
        x0 = torch.where(torch.rand(n, generator=g_) < 0.5, torch.rand(n, generator=g_) * 0.05, 1 - torch.rand(n, generator=g_) * 0.05)
        x = torch.clamp(x0 + (torch.rand(n, generator=g_) * 2 - 1) * 0.2, 0, 1)
        grad = torch.randn(n, generator=g_)
    else:
        raise KeyError(name)
    return x.float().contiguous(), x0.float().contiguous(), grad.float().contiguous(), alpha, eps
