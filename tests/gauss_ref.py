"""CPU restatement of the reference's Gaussian-blur and random-patch physical-object attacks, a test helper.

Reference: torchattacks/attacks/phy_obj_atk_guassian.py (forward :61-141) and phy_obj_atk_arbi.py (forward :56-108), under
Attack.__call__'s eval()/train() bracket; scipy.ndimage.gaussian_filter as the former calls it.  Written on the pieces of
oracle/attack_ref (PhysicalTransRef, paste) and tests/light_ref (the model, the seeds, the scenes at one shared pose set).

``blur`` restates ``np.clip(gaussian_filter(x, [0, 0, s, s]), 0, 1)`` (mode 'reflect', truncate 4.0) in numpy in scipy's own
order -- correlate1d's symmetric branch: per output and axis, in float64, ``tmp = a[i] p[lw]``, then for ``ll = -lw .. -1``
``tmp = tmp + (a[r(i + ll)] + a[r(i - ll)]) p[lw + ll]``, rounded to fp32; axis H first, the intermediate an fp32 array -- so
that tests without scipy have the exact values; tests/test_gauss_ref.py holds it to scipy itself where scipy is installed and
to the windows scipy wrote into tests/golden/atk_gauss.npz everywhere.

Also here, because the fixture generator (tools/make_goldens_gauss.py) and the tests must agree on them: the fixture's inputs
(``CASE``, ``case_inputs``), the shapes, sigmas and rectangles of the kernel test (``KERNEL_CASES``, ``kernel_input``).
"""
import random

import numpy as np
import torch
import torch.nn as nn

from oracle import attack_ref, synth
from tests.light_ref import argmin_gap, make_model, seed_all, vanila_scenes  # noqa: F401

# inputs of the fixture's attack part; ``rng_seeds``: the seeds the generator tries in turn until the argmin is decidable
CASE = dict(model_seed=5, gain=6.0, batch=2, scene_seed=37, steps=10, rng_seeds=(51, 52, 53, 54, 55))
REGION = (90, 170, 100, 200)        # phy_obj_atk_guassian.py:88, phy_obj_atk_arbi.py:75
ARBI_ANGLES = list(range(-30, 31, 2))

# (h, w, an interior rectangle): a radius below n, a radius above 2 n (sigma = 2 max(h, w)), H != W both ways
SMALL_SHAPES = [(7, 9, (2, 6, 1, 7)), (12, 10, (3, 9, 2, 8)), (33, 65, (5, 30, 7, 50))]


def small_sigmas(h, w):
    return [0.4, 3.0, 2.0 * max(h, w)]


BIG_STEPS = (1, 5, 10)      # of the 10-step schedule on 260 x 300: sigma 15, 75, 149.99999999999997


def kernel_input(h, w):
    """fp32 [1, 3, h, w] of the kernel test: the fixture's object at 260 x 300, seeded noise at the small shapes."""
    if (h, w) == (260, 300):
        return synth.make_object()[0].numpy()
    return np.random.RandomState(1000 * h + w).rand(1, 3, h, w).astype(np.float32)


def case_inputs(case=CASE):
    """(obj, mask, scenes) of the fixture, float32 on the CPU."""
    obj, mask = synth.make_object()
    scenes = synth.kitti_like(case["batch"], 3, 375, 1242, torch.Generator().manual_seed(case["scene_seed"]))
    return obj, mask, scenes


# --------------------------------------------------------------------------- the filter
def sigmas(steps, h, w):
    """The schedule of :76-95 in Python floats: 149.99999999999997, not 150, at step 10 of 10 on 260 x 300."""
    epsilon, stepsize, max_sigma, out = 0.0, 1.0 / steps, max(h, w) // 2, []
    for _ in range(steps):
        epsilon += stepsize
        out.append(epsilon * max_sigma)
    return out


def kernel1d(sigma, truncate=4.0):
    """(p float64 [2 lw + 1], lw): scipy's _gaussian_kernel1d of order 0 at the radius gaussian_filter1d gives it."""
    sd = float(sigma)
    lw = int(truncate * sd + 0.5)
    x = np.arange(-lw, lw + 1)
    p = np.exp(-0.5 / (sd * sd) * x ** 2)
    return p / p.sum(), lw


def correlate_last(a, idx, p, lw):
    """correlate1d (symmetric weights, mode 'reflect') along the last axis of fp32 ``a`` at the positions ``idx``."""
    n = a.shape[-1]
    a = a.astype(np.float64)

    def r(j):
        m = np.mod(j, 2 * n)
        return np.where(m >= n, 2 * n - 1 - m, m)
    tmp = a[..., idx] * p[lw]
    for ll in range(-lw, 0):
        tmp = tmp + (a[..., r(idx + ll)] + a[..., r(idx - ll)]) * p[lw + ll]
    return tmp.astype(np.float32)


def blur(x, sigma, region=None):
    """np.clip(gaussian_filter(x, [0, .., 0, s, s]), 0, 1) of fp32 ``x`` [..., H, W] on ``region`` = (r0, r1, c0, c1) (the whole
    patch by default): only the rectangle's rows go through the first pass, which changes no value."""
    x = np.asarray(x, dtype=np.float32)
    H, W = x.shape[-2:]
    r0, r1, c0, c1 = (0, H, 0, W) if region is None else region
    p, lw = kernel1d(sigma)
    rows = correlate_last(np.swapaxes(x, -1, -2), np.arange(r0, r1), p, lw)
    return np.clip(correlate_last(np.swapaxes(rows, -1, -2), np.arange(c0, c1), p, lw), 0, 1)


# --------------------------------------------------------------------------- the draws
def draw_poses(dist_range, angle_range, steps, batch_size):
    """steps + 1 (z0, alpha) sets from Python's global generator: one project() per step (physicalTrans.py:150,155), then the
    two samples of :128-129."""
    return [(random.sample(dist_range, batch_size), random.sample(angle_range, batch_size)) for _ in range(steps + 1)]


def arbi_fill(rs, shape, region=REGION):
    """(fp32 [b, c, rh, rw], "noise" | "colour"): the rectangle of the next pattern of Phy_obj_atk_arbi from its generator ``rs``
    (:77-82): one rand() for the branch, then rand(b, c, h, w) or one rand() per channel."""
    b, c, h, w = shape
    r0, r1, c0, c1 = region
    if rs.rand() > 0.5:
        return rs.rand(b, c, h, w)[:, :, r0:r1, c0:c1].astype(np.float32), "noise"
    fill = np.ones((b, c, r1 - r0, c1 - c0), dtype=np.float32)
    for c_ind in range(c):
        fill[:, c_ind] *= np.float32(rs.rand())
    return fill, "colour"


def arbi_poses(batch_size, eval=False):
    """(z0, alpha) of :91-96."""
    z0 = np.linspace(5, 30, num=batch_size)
    al = np.random.RandomState(17).choice(ARBI_ANGLES, batch_size, replace=True)
    if eval:
        z0[0], al[0] = 7, 0
    return z0, al


# --------------------------------------------------------------------------- the attacks
def with_window(obj_img, window, region=REGION):
    r0, r1, c0, c1 = region
    out = obj_img.clone()
    out[:, :, r0:r1, c0:c1] = torch.as_tensor(window).to(obj_img.dtype)
    return out


def phy_obj_atk_guassian(model, obj_img, obj_mask, images, batch_size, steps=CASE["steps"], dist_range=None, eval=False,
                         region=REGION, P2=attack_ref.KITTI_P2, trace=None, poses=None, windows=None):
    """Returns (adv_scenes, ben_scenes, obj_masks_out, adv_patch).  Runs in the dtype of ``obj_img`` (the blurred rectangle is
    the fp32 filter's in either).  ``trace``: a dict that receives ``sigma`` [steps], ``z0`` / ``alpha`` [steps + 1, B], ``cost``
    [steps], ``best`` and ``windows`` [steps, 3, rh, rw].  ``poses`` / ``windows``: made earlier instead of afresh."""
    dist_range = list(range(5, 31, 2)) if dist_range is None else dist_range
    dt = obj_img.dtype
    given_training = model.training
    model.eval()
    trans_adv = attack_ref.PhysicalTransRef(obj_img.clone(), obj_mask, P2, dist_range=dist_range)
    trans_ben = attack_ref.PhysicalTransRef(obj_img, obj_mask, P2, dist_range=dist_range)
    scene_imgs = attack_ref._tile_scene(images.detach(), batch_size)
    target = torch.zeros((batch_size, 1) + tuple(attack_ref.SCENE_SIZE), dtype=dt)
    criterion = nn.MSELoss()
    h, w = obj_img.shape[-2:]
    sig = sigmas(steps, h, w)
    if poses is None:
        poses = draw_poses(trans_ben.dist_range, trans_ben.angle_range, steps, batch_size)
    if windows is None:
        x0 = obj_img.float().numpy()
        windows = np.concatenate([blur(x0, s, region) for s in sig], 0)
    cost = np.zeros(steps, dtype=np.float64)
    best_cost, best = 1e10, -1
    with torch.no_grad():
        for i in range(steps):
            trans_adv.reset_img(with_window(obj_img, windows[i], region), obj_mask)
            adv_scenes, masks, _, _, _ = attack_ref.paste(scene_imgs, trans_adv, batch_size, poses[i][0], poses[i][1])
            c = criterion(model(adv_scenes) * masks, target)
            cost[i] = float(c)
            if c < best_cost:       # strictly (:121)
                best_cost, best = c, i
    if trace is not None:
        trace.update(sigma=np.asarray(sig), z0=np.asarray([p[0] for p in poses], dtype=np.float64),
                     alpha=np.asarray([p[1] for p in poses], dtype=np.int64), cost=cost, best=best, windows=windows)
    if given_training:
        model.train()
    if best < 0:
        return None, None, None, None
    adv = with_window(obj_img, windows[best], region)
    trans_adv.reset_img(adv, obj_mask)
    z0, al = list(poses[steps][0]), list(poses[steps][1])
    if eval:
        z0[0], al[0] = 7, 0
    return vanila_scenes(scene_imgs, trans_adv, trans_ben, batch_size, z0, al) + (adv,)


def phy_obj_atk_arbi(rs, obj_img, obj_mask, images, batch_size, dist_range=None, eval=False, region=REGION,
                     P2=attack_ref.KITTI_P2):
    """One call of Phy_obj_atk_arbi.forward with the instance's generator ``rs``: (adv_scenes, ben_scenes, masks, patch, fill)."""
    dist_range = list(range(5, 31, 2)) if dist_range is None else dist_range
    fill, kind = arbi_fill(rs, tuple(obj_img.shape), region)
    adv = with_window(obj_img, fill, region)
    trans_adv = attack_ref.PhysicalTransRef(adv, obj_mask, P2, dist_range=dist_range)
    trans_ben = attack_ref.PhysicalTransRef(obj_img, obj_mask, P2, dist_range=dist_range)
    scene_imgs = attack_ref._tile_scene(images.detach(), batch_size)
    z0, al = arbi_poses(batch_size, eval)
    return vanila_scenes(scene_imgs, trans_adv, trans_ben, batch_size, z0, al) + (adv, kind)


def costs64(model_fn, obj, mask, scenes, batch, steps, poses, dist_range, windows, region=REGION):
    """Costs of the restatement in float64 on poses and fp32 windows made earlier."""
    tr = {}
    phy_obj_atk_guassian(model_fn().double(), obj.double(), mask.double(), scenes.double(), batch, steps=steps,
                         dist_range=dist_range, region=region, trace=tr, poses=poses, windows=windows)
    return tr["cost"]
