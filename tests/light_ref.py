"""CPU restatement of the reference's tube-light physical-object attack, a test helper.

Reference: torchattacks/attacks/phy_obj_atk_light.py (forward :64-188) and light_simulation.py (simple_add :23-28,
wavelength_to_rgb :40-84, tube_light_generation_by_func :124-163), under Attack.__call__'s eval()/train() bracket; the no-op
paste of phy_obj_atk_vanila.py :58-94.  Written on the pieces of oracle/attack_ref (PhysicalTransRef, paste).

The attack is a random search whose draws never depend on the model: ``draw_params`` and ``draw_poses`` reproduce both streams
(numpy's for the light parameters, Python's for the poses) in the reference's order.  ``pattern_u8`` is the reference's chain
tube_light_generation_by_func -> * 255.0 -> simple_add -> clip -> uint8, vectorised in float64/float32 with every operation
rounded where the reference's scalar Python rounds it.

Also here, because the fixture generator (tools/make_goldens_light.py) and the tests must agree on them: the fixture's inputs
(``CASE``, ``make_model``, ``case_inputs``) and the parameter sets of its ``patterns`` part (``PATTERN_SETS``).
"""
import math
import random

import numpy as np
import torch
import torch.nn as nn

from oracle import attack_ref, synth, tv082

# inputs of the fixture's ``attack`` part (the model and the gain of tests/apgd_ref.py); ``rng_seeds``: the seeds the generator
# tries in turn until the argmin of the 8000 costs is decidable
CASE = dict(model_seed=5, gain=6.0, batch=2, scene_seed=31, rng_seeds=(41, 42, 43, 44, 45))
N_INIT, N_SEARCH = 200, 20                      # the literals of :113 and :88
LO, HI = (380, 0, 0, 10), (750, 180, 400, 1600)  # the clip of :128: wavelength, angle, b, beta
Q = np.asarray([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 1], [0, 1, 1, 0],
                [0, 1, 0, 1], [0, 0, 1, 1]])

# (wavelength, angle, b, beta) of the fixture's ``patterns`` part: every branch of wavelength_to_rgb and its boundaries,
# angles 0 / 89 / 90 / 91 / 179, both clip edges of every parameter, beta 10 and 1600
PATTERN_SETS = [(380, 90, 0, 10), (440, 0, 400, 1600), (490, 89, 200, 300), (510, 91, 100, 900), (580, 179, 200, 55),
                (645, 45, 1, 1599), (750, 180, 250, 700), (410, 135, 130, 10), (465, 30, 0, 1600), (500, 0, 0, 400),
                (545, 60, 0, 120), (612, 150, 260, 36), (700, 1, 77, 1000), (749, 120, 300, 11)]


def make_model(model_seed=CASE["model_seed"], gain=CASE["gain"]):
    model = synth.TinyDepthNet(seed=model_seed)
    with torch.no_grad():
        model.c3.weight.mul_(gain)
        model.c3.bias.mul_(gain)
    return model


def case_inputs(case=CASE):
    """(obj, mask, scenes) of the fixture, float32 on the CPU."""
    obj, mask = synth.make_object()
    scenes = synth.kitti_like(case["batch"], 3, 375, 1242, torch.Generator().manual_seed(case["scene_seed"]))
    return obj, mask, scenes


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


# --------------------------------------------------------------------------- the light pattern
def colour(wavelength, gamma=0.8):
    """wavelength_to_rgb (:40-84): the first matching band wins at a shared boundary."""
    w = float(wavelength)
    if 380 <= w <= 440:
        att = 0.3 + 0.7 * (w - 380) / (440 - 380)
        return (((-(w - 440) / (440 - 380)) * att) ** gamma, 0.0, (1.0 * att) ** gamma)
    if 440 <= w <= 490:
        return (0.0, ((w - 440) / (490 - 440)) ** gamma, 1.0)
    if 490 <= w <= 510:
        return (0.0, 1.0, (-(w - 510) / (510 - 490)) ** gamma)
    if 510 <= w <= 580:
        return (((w - 510) / (580 - 510)) ** gamma, 1.0, 0.0)
    if 580 <= w <= 645:
        return (1.0, (-(w - 645) / (645 - 580)) ** gamma, 0.0)
    if 645 <= w <= 750:
        att = 0.3 + 0.7 * (750 - w) / (750 - 645)
        return ((1.0 * att) ** gamma, 0.0, 0.0)
    return (0.0, 0.0, 0.0)


def record(params, alpha=1.0):
    """(k, b, beta, full_end, light_end, sqrt(1 + k k), c0 alpha, c1 alpha, c2 alpha) in float64 for one (wavelength, angle, b,
    beta): the scalars :130-133 and tube_light_generation_by_func :143-146 make before the pixel loop."""
    wl, angle, b, beta = (int(v) for v in params)
    k = round(math.tan(math.radians(angle)), 2)
    c = colour(wl)
    return np.array([k, b, beta, int(math.sqrt(beta) + 0.5), int(math.sqrt(beta * 20) + 0.5), math.sqrt(1 + k * k),
                     c[0] * alpha, c[1] * alpha, c[2] * alpha], dtype=np.float64)


def light(rec, h, w):
    """tube_light_generation_by_func's [h, w, 3] float64 array."""
    k, b, beta, full, end, s = (rec[i] for i in range(6))
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    d = np.abs(k * x - y + b) / s
    with np.errstate(divide="ignore", invalid="ignore"):
        att = np.where(d <= full, 1.0, np.where(d <= end, beta / (d * d), 0.0))
    return np.stack([rec[6 + i] * att for i in range(3)], -1)


def pattern_u8(base_u8, rec):
    """The lit object as uint8 [h, w, 3]: (light * 255.0) rounded to fp32, added to the fp32 base in fp32, clipped, truncated."""
    h, w, _ = base_u8.shape
    lit = (light(rec, h, w) * 255.0).astype(np.float32)
    return np.clip(base_u8.astype(np.float32) + lit, 0.0, 255.0).astype(np.uint8)


def base_u8(obj_img):
    """ToPILImage on a float tensor: mul(255).byte(), as [h, w, 3]."""
    return obj_img.detach().squeeze(0).float().cpu().mul(255).byte().permute(1, 2, 0).contiguous().numpy()


def to_patch(u8, dtype=torch.float32):
    """ToTensor: [h, w, 3] uint8 -> [1, 3, h, w], divided by 255 in fp32."""
    return torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).float().div(255).unsqueeze(0).to(dtype).contiguous()


# --------------------------------------------------------------------------- the draws
def draw_params(n_init=N_INIT, n_search=N_SEARCH):
    """int64 [n_init * n_search * 2, 4] from numpy's global generator in the order of :113-128."""
    inits = [[np.random.randint(380, 750), np.random.randint(0, 180), np.random.randint(0, 400), np.random.randint(10, 1600)]
             for _ in range(n_init)]
    out = []
    for init_v in inits:
        for _ in range(n_search):
            q = Q[np.random.randint(len(Q))] * np.random.randint(1, 20)
            for a in (-1, 1):
                out.append(np.clip(init_v + a * q, LO, HI))
    return np.asarray(out, dtype=np.int64).reshape(-1, 4)


def draw_poses(dist_range, angle_range, n, batch_size):
    """n + 1 (z0, alpha) sets from Python's global generator: one project() per query (physicalTrans.py:150,155), then the
    two samples of :173-174."""
    return [(random.sample(dist_range, batch_size), random.sample(angle_range, batch_size)) for _ in range(n + 1)]


# --------------------------------------------------------------------------- the search
def phy_obj_atk_light(model, obj_img, obj_mask, images, batch_size, n_init=N_INIT, n_search=N_SEARCH, dist_range=None,
                      eval=False, P2=attack_ref.KITTI_P2, trace=None, draws=None, only=None):
    """Returns (adv_scenes, ben_scenes, obj_masks_out, adv_patch).  Runs in the dtype of ``obj_img`` (the patch itself is the
    fp32 ``uint8 / 255`` in either).  ``trace``: a dict that receives ``params`` [n, 4], ``poses`` (z0 [n + 1, B], alpha
    [n + 1, B]), ``cost`` [n] and ``best``.  ``draws``: (params, poses) drawn earlier instead of a fresh draw.  ``only``: an
    iterable of query numbers: the others are skipped (their cost is nan; the draws are made all the same)."""
    dist_range = list(range(5, 31, 2)) if dist_range is None else dist_range
    dt = obj_img.dtype
    given_training = model.training
    model.eval()
    trans_adv = attack_ref.PhysicalTransRef(obj_img.clone(), obj_mask, P2, dist_range=dist_range)
    trans_ben = attack_ref.PhysicalTransRef(obj_img, obj_mask, P2, dist_range=dist_range)
    scene_imgs = attack_ref._tile_scene(images.detach(), batch_size)
    target = torch.zeros((batch_size, 1) + tuple(attack_ref.SCENE_SIZE), dtype=dt)
    criterion = nn.MSELoss()
    base = base_u8(obj_img)
    if draws is None:
        params = draw_params(n_init, n_search)
        poses = draw_poses(trans_ben.dist_range, trans_ben.angle_range, len(params), batch_size)
    else:
        params, poses = draws
    n = len(params)
    cost = np.full(n, np.nan, dtype=np.float64)
    best_cost, best, best_u8 = 1e10, -1, None
    todo = range(n) if only is None else only
    with torch.no_grad():
        for i in todo:
            u8 = pattern_u8(base, record(params[i]))
            trans_adv.reset_img(to_patch(u8, dt), obj_mask)
            adv_scenes, masks, _, _, _ = attack_ref.paste(scene_imgs, trans_adv, batch_size, poses[i][0], poses[i][1])
            c = criterion(model(adv_scenes) * masks, target)
            cost[i] = float(c)
            if c < best_cost:       # strictly (:165)
                best_cost, best, best_u8 = c, i, u8
    if trace is not None:
        trace.update(params=params, z0=np.asarray([p[0] for p in poses], dtype=np.float64),
                     alpha=np.asarray([p[1] for p in poses], dtype=np.int64), cost=cost, best=best)
    if best_u8 is None:
        if given_training:
            model.train()
        return None, None, None, None
    adv = to_patch(best_u8, dt)
    trans_adv.reset_img(adv, obj_mask)
    z0, al = list(poses[n][0]), list(poses[n][1])
    if eval:
        z0[0], al[0] = 7, 0
    out = vanila_scenes(scene_imgs, trans_adv, trans_ben, batch_size, z0, al)
    if given_training:
        model.train()
    return out + (adv,)


def vanila_scenes(scene_imgs, trans_adv, trans_ben, batch_size, z0, al):
    """(adv_scenes, ben_scenes, masks) at one shared pose set (:179-186; phy_obj_atk_vanila.py:85-92)."""
    adv_scenes, _, full_mask, _, _ = attack_ref.paste(scene_imgs, trans_adv, batch_size, z0, al)
    obj_ben, _, _, _ = trans_ben.project(batch_size=batch_size, z0_sample=z0, alpha_sample=al)
    ben_scenes = tv082.resize(scene_imgs * (1 - full_mask) + obj_ben * full_mask, attack_ref.SCENE_SIZE)
    return adv_scenes, ben_scenes, tv082.resize(full_mask, attack_ref.SCENE_SIZE)


def phy_obj_atk_vanila(obj_img0, obj_mask, images, obj_img, batch_size, dist_range=None, eval=False, P2=attack_ref.KITTI_P2):
    """Phy_obj_atk_vanila.forward: ``obj_img`` pasted as the adversarial patch, ``obj_img0`` (the constructor's) as the clean."""
    dist_range = list(range(5, 31, 2)) if dist_range is None else dist_range
    trans_adv = attack_ref.PhysicalTransRef(obj_img.clone().detach(), obj_mask, P2, dist_range=dist_range)
    trans_ben = attack_ref.PhysicalTransRef(obj_img0, obj_mask, P2, dist_range=dist_range)
    scene_imgs = attack_ref._tile_scene(images.detach(), batch_size)
    z0 = random.sample(trans_ben.dist_range, batch_size)
    al = random.sample(trans_ben.angle_range, batch_size)
    if eval:
        z0[0], al[0] = 7, 0
    return vanila_scenes(scene_imgs, trans_adv, trans_ben, batch_size, z0, al) + (obj_img.clone().detach(),)


def costs64(model_fn, obj, mask, scenes, batch, draws, dist_range, only=None):
    """Costs of the restatement in float64 for the queries ``only`` (all of them by default) on draws made earlier."""
    tr = {}
    phy_obj_atk_light(model_fn().double(), obj.double(), mask.double(), scenes.double(), batch, dist_range=dist_range,
                      trace=tr, draws=draws, only=only)
    return tr["cost"]


def argmin_gap(costs):
    """(index of the smallest cost -- the first one at a tie, as the strict ``<`` keeps it --, relative gap to the second
    smallest)."""
    c = np.asarray(costs, dtype=np.float64)
    order = np.argsort(c, kind="stable")
    lo, nxt = c[order[0]], c[order[1]]
    return int(order[0]), float((nxt - lo) / abs(nxt)) if nxt != 0 else 0.0
