"""CPU restatement of the reference's Square physical-object attack, a test helper.

Reference: torchattacks/attacks/phy_obj_atk_square.py -- p_selection :222-249, random_choice / random_int :173-179,
attack_single_run's Linf branch :258-329, depth_loss :123-133, forward :83-121 -- under Attack.__call__'s eval()/train() bracket.
Written in numpy float32 (one rounded operation per step, as ATen's element-wise kernels round) on the pieces of
oracle/attack_ref (PhysicalTransRef, paste) and tests/light_ref (the model, the seeds, the scenes at one shared pose set); the
package's own host pieces (ops.square_sides, ops.square_table, ops.square_host) are written in torch and are held to this file
by tests/test_square_ref.py, and both to the reference's own run stored in tests/golden/atk_square.npz.

The accept rule is K24's: strictly below the running minimum, which starts at 1e10, so a tie and a NaN are rejected.  The
reference differs after a NaN only: its ``loss_min`` turns NaN (0 * nan, :300-301) and nothing is accepted any more; the
fixture's scripts therefore hold no improvement after their NaN.

Also here, because the fixture generator (tools/make_goldens_square.py) and the tests must agree on them: the fixture's inputs
(``CASE``, ``SCRIPT_CASES``, ``script_object``) and the schedule cases.
"""
import math
import random

import numpy as np
import torch

from oracle import attack_ref, synth
from tests.light_ref import argmin_gap, make_model, seed_all, vanila_scenes  # noqa: F401

# inputs of the fixture's end-to-end part
CASE = dict(model_seed=5, gain=6.0, batch=2, scene_seed=43, n_queries=6, eps=0.1, rng_seed=61, pose_seed=0)
# the scripted trajectories: (C, H, W), p_init (0.5 keeps the largest square inside these small objects), eps, torch seed and the
# loss the stand-in depth_loss returns per call: start, accept, exact tie, reject, accept, reject, accept, NaN, reject, reject.
# Case "a" follows the rescaled schedule (sides 11, 2, 1, ...), case "b" the plain one (side 10 throughout).
SCRIPT = [5.0, 4.0, 4.0, 6.0, 3.5, 3.75, 3.25, float("nan"), 3.5, 9.0]
SCRIPT_CASES = {"a": dict(shape=(3, 13, 19), p_init=0.5, eps=0.1, seed=71, resc=True),
                "b": dict(shape=(3, 12, 16), p_init=0.5, eps=0.3, seed=72, resc=False)}
SCHEDULE_CASES = [(n, resc, hw) for n in (10, 60, 5000) for resc in (True, False) for hw in ((13, 19), (260, 300))]
REGION = (90, 170, 100, 200)        # the sub-rectangle of the patch the fixture stores (the siblings' rectangle)


def script_object(shape):
    """fp32 [1, C, H, W] in [0, 1] with values near 0 and 1, so that both clips and both eps bounds are met."""
    c, h, w = shape
    x = np.random.RandomState(100 * h + w).rand(1, c, h, w).astype(np.float32)
    x[:, :, ::3, ::4] = 0.0
    x[:, :, 1::3, 1::4] = 1.0
    x[:, :, 2::5, ::3] *= np.float32(0.05)
    return x


def case_inputs(case=CASE):
    obj, mask = synth.make_object()
    scenes = synth.kitti_like(case["batch"], 3, 375, 1242, torch.Generator().manual_seed(case["scene_seed"]))
    return obj, mask, scenes


# --------------------------------------------------------------------------- the schedule
def p_selection(it, n_queries, p_init=0.8, resc_schedule=True):
    if resc_schedule:
        it = int(it / n_queries * 10000)
    if 10 < it <= 50:
        return p_init / 2
    elif 50 < it <= 200:
        return p_init / 4
    elif 200 < it <= 500:
        return p_init / 8
    elif 500 < it <= 1000:
        return p_init / 16
    elif 1000 < it <= 2000:
        return p_init / 32
    elif 2000 < it <= 4000:
        return p_init / 64
    elif 4000 < it <= 6000:
        return p_init / 128
    elif 6000 < it <= 8000:
        return p_init / 256
    elif 8000 < it:
        return p_init / 512
    return p_init


def sides(n_queries, c, h, w, p_init=0.8, resc_schedule=True):
    n_features = c * h * w
    return [max(int(round(math.sqrt(p_selection(i, n_queries, p_init, resc_schedule) * n_features / c))), 1)
            for i in range(n_queries)]


# --------------------------------------------------------------------------- the draws
def draw(n_queries, c, h, w, p_init=0.8, resc_schedule=True):
    """(stripes fp32 [c, w], vh [n], vw [n], s [n], signs [n, c]) from the CPU torch global generator in the reference's order."""
    stripes = torch.sign(2 * torch.rand([1, c, 1, w]) - 1).numpy().reshape(c, w)
    vh, vw, sg = [], [], []
    ss = sides(n_queries, c, h, w, p_init, resc_schedule)
    for s in ss:
        vh.append(int((0 + (h - s - 0) * torch.rand([1])).long()))
        vw.append(int((0 + (w - s - 0) * torch.rand([1])).long()))
        sg.append(torch.sign(2 * torch.rand([c, 1, 1]) - 1).numpy().reshape(c))
    return stripes, np.asarray(vh), np.asarray(vw), np.asarray(ss), np.asarray(sg, dtype=np.float32).reshape(len(ss), c)


def table_of(vh, vw, s, signs):
    """int32 [n + 1, 3 + c]: row q = the square of iteration q - 1, row 0 zero (query 0 is the stripes)."""
    n, c = signs.shape
    t = np.zeros((n + 1, 3 + c), dtype=np.int32)
    t[1:, 0], t[1:, 1], t[1:, 2], t[1:, 3:] = vh, vw, s, signs
    return t


# --------------------------------------------------------------------------- propose
def propose(x0, x_best, x_new, table, stripes, q, best, eps):
    """K27's contract in numpy: (x_best, x_new) after the launch with cursor ``q`` and best query ``best``.  fp32 [1, C, H, W]."""
    n = len(table)
    eps = np.float32(eps)
    x_best, x_new = x_best.copy(), x_new.copy()
    if q < 0 or q > n:
        return x_best, x_new
    if q > 0 and best == q - 1:
        x_best = x_new.copy()
    if q == n:
        return x_best, x_new
    if q == 0:
        x_new = np.clip(x0 + eps * stripes[None, :, None, :].astype(np.float32), np.float32(0), np.float32(1))
        return x_best, x_new
    vh, vw, s = (int(v) for v in table[q][:3])
    x_new = x_best.copy()
    d = (np.float32(2) * eps) * table[q][3:].astype(np.float32)[None, :, None, None]
    win = (slice(None), slice(None), slice(vh, vh + s), slice(vw, vw + s))
    v = x_best[win] + d
    v = np.minimum(np.maximum(v, x0[win] - eps), x0[win] + eps)
    x_new[win] = np.clip(v, np.float32(0), np.float32(1))
    return x_best, x_new


def search(x0, table, stripes, eps, cost_fn, query_patch="candidate"):
    """The search loop with a cost callback ``cost_fn(patch, q)``.  Returns (x_best after every query [n, 1, C, H, W], costs
    fp32 [n], accepted queries, final x_best)."""
    n = len(table)
    x_best, x_new = x0.copy(), np.zeros_like(x0)
    low, best, costs, after, accepted = np.float32(1e10), -1, np.zeros(n, dtype=np.float32), [], []
    for q in range(n):
        x_best, x_new = propose(x0, x_best, x_new, table, stripes, q, best, eps)
        c = np.float32(cost_fn(x_best if query_patch == "best" and q > 0 else x_new, q))
        costs[q] = c
        if c < low:
            low, best = c, q
            accepted.append(q)
        after.append(x_new.copy() if best == q else x_best.copy())
    x_best, _ = propose(x0, x_best, x_new, table, stripes, n, best, eps)
    return np.stack(after, 0), costs, accepted, x_best


def accepted_of(costs):
    """The accepted queries of a cost array: its running strict minimum from 1e10."""
    low, out = np.float32(1e10), []
    for q, c in enumerate(np.asarray(costs, dtype=np.float32)):
        if c < low:
            low = c
            out.append(q)
    return out


# --------------------------------------------------------------------------- the cost (depth_loss :123-133)
def rs_poses(dist_range, angle_range, batch_size, seed):
    """The pose set of every depth_loss call: project(rs=np.random.RandomState(seed)) (physicalTrans.py:146-155)."""
    rs = np.random.RandomState(seed)
    return rs.choice(dist_range, batch_size, replace=False), rs.choice(angle_range, batch_size, replace=False)


def final_poses(dist_range, angle_range, batch_size, eval=False):
    z0, al = random.sample(dist_range, batch_size), random.sample(angle_range, batch_size)      # :106-107
    if eval:
        z0[0], al[0] = 7, 0
    return z0, al


def depth_cost(model, patch, obj_mask, scene_imgs, batch_size, z0, al, dist_range, P2=attack_ref.KITTI_P2):
    """MSE(model(pasted scenes) * mask, 0) in the dtype of ``patch``; the model is used as it stands (eval() by the caller)."""
    trans = attack_ref.PhysicalTransRef(patch, obj_mask, P2, dist_range=dist_range)
    adv_scenes, masks, _, _, _ = attack_ref.paste(scene_imgs, trans, batch_size, list(z0), list(al))
    with torch.no_grad():
        return torch.nn.MSELoss()(model(adv_scenes) * masks, torch.zeros_like(masks))
