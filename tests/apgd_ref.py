"""CPU restatement of the reference's Auto-PGD physical-object attack (Linf), a test helper.

Reference: torchattacks/attacks/phy_obj_atk_apgd.py -- forward :75-115, check_oscillation :117-122, attack_single_run :133-292,
perturb(cheap=True) :295-330, under Attack.__call__'s eval()/train() bracket (attack.py:296-312).  Written in the style of
oracle/attack_ref.phy_obj_atk and on its pieces (PhysicalTransRef, paste).  It runs in the dtype of its inputs (float32: the
reference's arithmetic, op for op; float64: the anchor the decision margins are measured in) and can record every iteration.

Also here, because the fixture generator (tools/make_goldens_apgd.py) and the tests must agree on them: the inputs of the fixture
(``CASE``, ``make_model``, ``case_inputs``) and the decision margins (``margins``, ``safe_prefix``).
"""
import random

import numpy as np
import torch
import torch.nn as nn

from oracle import attack_ref, synth, tv082

# The fixture's inputs.  TinyDepthNet(seed=5) as it stands answers the patch with loss changes of 1e-5 relative and less (the
# decisions of the algorithm then hang on the last bits of an fp32 sum), so the last convolution is scaled by ``gain``: the
# sigmoid leaves its flat region and the cost responds to the patch.
CASE = dict(model_seed=5, gain=6.0, eps=0.2, steps=10, batch=2, scene_seed=31, noise_seed=1234, seed=17, rng_seed=41)


def make_model(model_seed=CASE["model_seed"], gain=CASE["gain"]):
    model = synth.TinyDepthNet(seed=model_seed)
    with torch.no_grad():
        model.c3.weight.mul_(gain)
        model.c3.bias.mul_(gain)
    return model


def case_inputs(case=CASE):
    """(obj, mask, scenes, start noise t) of the fixture, all float32 on the CPU."""
    obj, mask = synth.make_object()
    scenes = synth.kitti_like(case["batch"], 3, 375, 1242, torch.Generator().manual_seed(case["scene_seed"]))
    t = 2 * torch.rand(obj.shape, generator=torch.Generator().manual_seed(case["noise_seed"])) - 1
    return obj, mask, scenes, t


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def schedule(steps):
    """(k at the start, steps_min, size_decr) of :137."""
    return max(int(0.22 * steps), 1), max(int(0.06 * steps), 1), max(int(0.03 * steps), 1)


def phy_obj_atk_apgd(model, obj_img, obj_mask, images, batch_size, eps=8 / 255, steps=100, seed=17, rho=.75, dist_range=None,
                     eval=False, P2=attack_ref.KITTI_P2, start_noise=None, trace=None):
    """Returns (adv_scenes, ben_scenes, obj_masks_out, adv_patch).  ``start_noise`` stands in for the ``2 * rand - 1`` of :142;
    ``trace``: a list that receives one dict per iteration (loss, loss_best after it, the step size and k it used, whether it was a
    checkpoint / reduced / moved loss_best, the count of rising losses, the iterate before a possible restart, and ``cmp``: every
    pair of numbers the iteration compared, as (a, b, structural) -- see ``margins``)."""
    dist_range = list(range(5, 31, 2)) if dist_range is None else dist_range
    dt = obj_img.dtype
    given_training = model.training
    model.eval()
    trans_adv = attack_ref.PhysicalTransRef(obj_img.clone(), obj_mask, P2, dist_range=dist_range)
    trans_ben = attack_ref.PhysicalTransRef(obj_img, obj_mask, P2, dist_range=dist_range)
    scene_imgs = attack_ref._tile_scene(images.detach(), batch_size)
    target = torch.zeros((batch_size, 1) + tuple(attack_ref.SCENE_SIZE), dtype=dt)
    criterion = nn.MSELoss()

    def poses():        # project(batch_size, rs=RandomState(seed)), physicalTrans.py:146-155: the same set at every call
        rs = np.random.RandomState(seed)
        z0 = rs.choice(trans_adv.dist_range, batch_size, replace=False)
        return z0, rs.choice(trans_adv.angle_range, batch_size, replace=False)

    def loss_and_grad(x_adv):
        x_adv.requires_grad_()
        with torch.enable_grad():
            trans_adv.reset_img(x_adv, obj_mask)
            z0, al = poses()
            adv_scenes, masks, _, _, _ = attack_ref.paste(scene_imgs, trans_adv, batch_size, z0, al)
            loss_indiv = -1. * criterion(model(adv_scenes) * masks, target).unsqueeze(0)
            loss = loss_indiv.sum()
        return loss_indiv.detach(), torch.autograd.grad(loss, [x_adv])[0].detach()

    x = obj_img.clone()
    k, steps_min, size_decr = schedule(steps)
    t = (2 * torch.rand(x.shape) - 1).to(dt) if start_noise is None else start_noise.to(dt)
    eps_t = torch.full((1, 1, 1, 1), eps, dtype=dt)
    x_adv = x.detach() + eps_t * t / t.reshape([1, -1]).abs().max(dim=1, keepdim=True)[0].reshape([-1, 1, 1, 1])
    x_adv = x_adv.clamp(0., 1.)
    x_best, x_best_adv = x_adv.clone(), x_adv.clone()
    loss_steps = np.zeros([steps, 1], dtype=np.float64 if dt == torch.float64 else np.float32)
    loss_indiv, grad = loss_and_grad(x_adv)
    grad_best = grad.clone()
    loss_best = loss_indiv.clone()
    step_size = eps_t * torch.tensor([2.0], dtype=dt).reshape([1, 1, 1, 1])
    x_adv_old = x_adv.clone()
    counter3 = 0
    loss_best_last_check = loss_best.clone()
    reduced_last_check = True
    moved_since_check = False
    for i in range(steps):
        with torch.no_grad():
            x_adv = x_adv.detach()
            grad2 = x_adv - x_adv_old
            x_adv_old = x_adv.clone()
            a = 0.75 if i > 0 else 1.0
            x_adv_1 = x_adv + step_size * torch.sign(grad)
            x_adv_1 = torch.clamp(torch.min(torch.max(x_adv_1, x - eps), x + eps), 0.0, 1.0)
            x_adv_1 = torch.clamp(torch.min(torch.max(x_adv + (x_adv_1 - x_adv) * a + grad2 * (1 - a), x - eps), x + eps), 0.0, 1.0)
            x_adv = x_adv_1 + 0.
        loss_indiv, grad = loss_and_grad(x_adv)
        x_best_adv = x_adv.detach() + 0.            # :255, before this iteration's checkpoint
        rec = dict(step_size=float(step_size), k=int(k), checkpoint=False, reduced=False, n_rose=0, cmp=[])
        with torch.no_grad():
            y1 = loss_indiv.clone()
            loss_steps[i] = y1.numpy()
            rec["cmp"].append((float(y1), float(loss_best), False))
            moved = bool(y1 > loss_best)            # strictly (:263)
            if moved:
                x_best, grad_best, loss_best = x_adv.detach().clone(), grad.clone(), y1.clone()
                moved_since_check = True
            counter3 += 1
            if counter3 == k:
                rose = 0
                for c in range(k):                  # check_oscillation: row i - c - 1 may be -1 = the last row, still zero
                    va, vb = loss_steps[i - c, 0], loss_steps[i - c - 1, 0]
                    rec["cmp"].append((float(va), float(vb), False))
                    rose += int(va > vb)
                oscillation = rose <= k * rho
                # loss_best_last_check is a copy of an earlier loss_best and loss_best only grows: while it has not moved since
                # that checkpoint the two operands are the SAME stored number in any implementation (structural, no margin)
                rec["cmp"].append((float(loss_best_last_check), float(loss_best), not moved_since_check))
                no_impr = (not reduced_last_check) and bool(loss_best_last_check >= loss_best)
                reduce = bool(oscillation or no_impr)
                reduced_last_check = reduce
                loss_best_last_check = loss_best.clone()
                moved_since_check = False
                if reduce:
                    step_size = step_size / 2.0
                    x_adv = x_best.clone()
                    grad = grad_best.clone()
                counter3 = 0
                k = max(k - size_decr, steps_min)
                rec.update(checkpoint=True, reduced=reduce, n_rose=rose)
        rec.update(loss=float(y1), loss_best=float(loss_best), moved=moved, patch=x_best_adv.clone())
        if trace is not None:
            trace.append(rec)
    adv = x_best_adv.detach()
    trans_adv.reset_img(adv, obj_mask)
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


def run64(model_fn, obj, mask, scenes, batch, t, **kw):
    """The restatement in float64 on the same inputs; returns its trace."""
    tr = []
    state = random.getstate()
    phy_obj_atk_apgd(model_fn().double(), obj.double(), mask.double(), scenes.double(), batch, start_noise=t.double(), trace=tr, **kw)
    random.setstate(state)
    return tr


def margins(trace64):
    """Per iteration the smallest relative margin |a - b| / max(|a|, |b|) over the comparisons the algorithm made in it (each
    ``loss > loss_best``, each rose/fell comparison of a checkpoint, the ``>=`` of the no-improvement test); structural ties
    (see the restatement) carry no margin."""
    out = []
    for rec in trace64:
        m = np.inf
        for a, b, structural in rec["cmp"]:
            if structural:
                continue
            d = max(abs(a), abs(b))
            m = min(m, abs(a - b) / d if d > 0 else 0.0)
        out.append(m)
    return np.array(out)


def decisions(trace):
    """int [n, 5]: (moved, checkpoint, reduced, n_rose, k) per iteration."""
    return np.array([[int(r["moved"]), int(r["checkpoint"]), int(r["reduced"]), int(r["n_rose"]), int(r["k"])] for r in trace])


def safe_prefix(losses32, trace32_decisions, trace64):
    """(n_safe, e_ref, margin per iteration, threshold).  e_ref: the largest relative distance between the fp32 run's losses and
    the float64 ones over the leading iterations on which both runs took the same decisions (beyond a split the two runs are on
    different trajectories and their distance says nothing about rounding).  An iteration is safe when its margin is at least
    max(20 e_ref, 1e-4); n_safe counts the leading safe iterations and never exceeds the common prefix."""
    l64 = np.array([r["loss"] for r in trace64])
    d64 = decisions(trace64)
    same = 0
    while same < len(l64) and np.array_equal(d64[same], np.asarray(trace32_decisions)[same]):
        same += 1
    rel = np.abs(np.asarray(losses32, dtype=np.float64)[:same] - l64[:same]) / np.abs(l64[:same])
    e_ref = float(rel.max()) if same else float("inf")
    thr = max(20.0 * e_ref, 1e-4)
    m = margins(trace64)
    n_safe = 0
    while n_safe < same and m[n_safe] >= thr:
        n_safe += 1
    return n_safe, e_ref, m, thr


def coverage(dec, n_safe, steps):
    """The conditions of the fixture on its safe prefix: a checkpoint that halves and restarts, one that does not, the wrapped
    read (the first checkpoint), an iteration where loss_best moves and one where it does not."""
    d = np.asarray(dec)[:n_safe]
    chk = d[:, 1] == 1
    k0 = schedule(steps)[0]
    return dict(reducing_checkpoint=bool((chk & (d[:, 2] == 1)).any()), plain_checkpoint=bool((chk & (d[:, 2] == 0)).any()),
                wrapped_read=bool(n_safe >= k0 and chk[k0 - 1]), moved=bool((d[:, 0] == 1).any()), stayed=bool((d[:, 0] == 0).any()))
