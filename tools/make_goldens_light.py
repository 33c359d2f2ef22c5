"""Writes tests/golden/atk_light.npz: the reference's own ``Phy_obj_atk_light`` and light_simulation functions on the seeded
inputs of tests/light_ref.py.

    python tools/make_goldens_light.py [--reference DIR] [--workers 6] [--raw FILE]
    python tools/make_goldens_light.py --patterns-only        (rewrites the ``patterns`` part of an existing fixture: seconds)

The reference package is imported the way tools/make_goldens_apgd.py imports it (oracle/make_goldens.install_shims, a temporary
calibration file).  Its ``forward`` is observed with ``sys.settrace`` -- cost and parameters at the line of ``if cost <
best_cost``, the pose draw at the return of PhysicalTrans.project -- and is not edited.  cv2 and torchvision are not installed
where this runs, so the tool installs stand-ins of its own (``STAND_INS`` below, copied into the fixture's metadata).

Two parts.  ``patterns``: tests/light_ref.PATTERN_SETS through the reference's tube_light_generation_by_func -> * 255.0 ->
simple_add -> clip -> uint8.  ``attack``: all 200 x 20 x 2 queries of the reference class; this part is written only if the final
argmin is decidable: the relative gap between the smallest and the second smallest reference cost is at least
max(20 e_ref, 1e-4), e_ref = the largest relative distance between the reference's fp32 costs and a float64 run of the
restatement (which runs in worker processes beside the reference).  Otherwise the next seed of light_ref.CASE["rng_seeds"] is
tried; with none left the tool exits and writes nothing.  The reference's pixel loop is Python: expect the better part of an
hour per seed.
"""
import inspect
import multiprocessing
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as mg      # noqa: E402
from oracle import synth                   # noqa: E402
from tests import light_ref as R           # noqa: E402

ROWS = (slice(None), slice(None), slice(120, 300, 9), slice(300, 800, 5))      # the row sample of atk_linf / atk_apgd
DIST_RANGE = list(np.arange(5, 10, 0.2))
STAND_INS = ["cv2.resize: identity (source and target sizes are equal)",
             "cv2.addWeighted: fp32 a * alpha + b * beta + gamma (alpha = beta = 1, gamma = 0: fl32(a + b) in any order)",
             "torchvision ToPILImage: PIL.Image.fromarray(t.mul(255).byte() as HWC)",
             "torchvision ToTensor: uint8 HWC -> CHW float32 .div(255)",
             "torchvision Normalize / CenterCrop / Compose: inert (built by forward, never applied)",
             "torchvision Resize / Pad / functional.perspective: oracle/tv082.py (oracle/make_goldens.install_shims)"]


def install_light_stand_ins():
    import PIL.Image as Image
    cv2 = sys.modules["cv2"]
    cv2.resize = lambda a, size: a
    cv2.addWeighted = lambda a, alpha, b, beta, gamma: (a * np.float32(alpha) + b * np.float32(beta)
                                                        + np.float32(gamma)).astype(np.float32)
    tvt = sys.modules["torchvision.transforms"]

    class ToPILImage(object):
        def __call__(self, t):
            return Image.fromarray(t.mul(255).byte().permute(1, 2, 0).contiguous().numpy())

    class ToTensor(object):
        def __call__(self, img):
            return torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous().float().div(255)

    class Inert(object):
        def __init__(self, *a, **k):
            pass

        def __call__(self, x):
            return x
    tvt.ToPILImage, tvt.ToTensor = ToPILImage, ToTensor
    tvt.Normalize = tvt.CenterCrop = tvt.Compose = Inert


def reference_modules(ref_dir):
    import matplotlib
    matplotlib.use("Agg")
    mg.install_shims()
    install_light_stand_ins()
    tmp = tempfile.mkdtemp(prefix="kitti_obj_")
    os.makedirs(os.path.join(tmp, "training", "calib"))
    with open(os.path.join(tmp, "training", "calib", "003086.txt"), "w") as f:
        f.write(synth.KITTI_CALIB_TEXT)
    sys.path.insert(0, os.path.join(ref_dir, "DepthNetworks", "monodepth2"))
    sys.path.append(ref_dir)
    import my_utils
    my_utils.object_dataset_root = tmp
    import torchattacks as ta
    import physicalTrans
    from torchattacks.attacks import light_simulation
    return ta.Phy_obj_atk_light, physicalTrans.PhysicalTrans, light_simulation


def observe(atk, project_code, call):
    """Runs ``call()``; returns (its result, costs, parameters, pose draws): the cost and ``temp_q`` of every query read at the
    line of ``if cost < best_cost``, and (z0_sample, alpha_sample) of every PhysicalTrans.project made without samples."""
    fwd = type(atk).forward
    code = fwd.__code__
    src = inspect.getsource(fwd).splitlines()
    (line,) = [code.co_firstlineno + i for i, s in enumerate(src) if s.strip().startswith("if cost < best_cost")]
    costs, params, poses = [], [], []
    t0 = time.time()

    def in_forward(frame, event, arg):
        if event == "line" and frame.f_lineno == line:
            loc = frame.f_locals
            costs.append(loc["cost"].detach().clone())
            params.append(np.array(loc["temp_q"], dtype=np.int64))
            if len(costs) % 200 == 0:
                print("  query %5d  %.0f s" % (len(costs), time.time() - t0), flush=True)
        return in_forward

    def in_project(frame, event, arg):
        if event == "return":
            loc = frame.f_locals
            poses.append(([float(v) for v in loc["z0_sample"]], [int(v) for v in loc["alpha_sample"]]))
        return in_project

    def tracer(frame, event, arg):
        if frame.f_code is code:
            return in_forward
        if frame.f_code is project_code:
            return in_project
        return None
    sys.settrace(tracer)
    try:
        out = call()
    finally:
        sys.settrace(None)
    return out, costs, np.stack(params, 0), poses


def gold_patterns(light_simulation):
    obj, _ = synth.make_object()
    base = R.base_u8(obj)
    h, w, _ = base.shape
    import math
    keep = dict(pattern_sets=np.asarray(R.PATTERN_SETS, dtype=np.int64))
    sums, subs, lit, changed = [], [], [], []
    for wl, angle, b, beta in R.PATTERN_SETS:
        k = round(math.tan(math.radians(angle)), 2)
        tube = light_simulation.tube_light_generation_by_func(k, b, alpha=1.0, beta=beta, wavelength=wl, w=w, h=h)
        img = np.clip(light_simulation.simple_add(base, tube * 255.0, 1.0), 0.0, 255.0).astype("uint8")
        sums.append(img.astype(np.int64).sum((0, 1)))
        subs.append(img[::4, ::4])
        lit.append(int((tube.max(-1) > 0).sum()))
        changed.append(int((img != base).any(-1).sum()))
        mine = R.pattern_u8(base, R.record((wl, angle, b, beta)))
        print("pattern %s  lit %6d  changed %6d  restatement differs in %d values" % ((wl, angle, b, beta), lit[-1], changed[-1],
                                                                                       int((mine != img).sum())))
    keep.update(pattern_sum=np.stack(sums, 0), pattern_sub=np.stack(subs, 0), pattern_lit=np.asarray(lit, dtype=np.int64),
                pattern_changed=np.asarray(changed, dtype=np.int64))
    return keep


def _worker(job):
    seed, only = job
    torch.set_num_threads(1)
    obj, mask, scenes = R.case_inputs()
    R.seed_all(seed)
    params = R.draw_params()
    poses = R.draw_poses(DIST_RANGE, attack_ref_angles(), len(params), R.CASE["batch"])
    return only, R.costs64(R.make_model, obj, mask, scenes, R.CASE["batch"], (params, poses), DIST_RANGE, only=only)[only]


def attack_ref_angles():
    from oracle import attack_ref
    return list(attack_ref.ANGLE_RANGE)


def main():
    ref_dir = sys.argv[sys.argv.index("--reference") + 1] if "--reference" in sys.argv else mg.REF
    workers = int(sys.argv[sys.argv.index("--workers") + 1]) if "--workers" in sys.argv else 6
    B = R.CASE["batch"]
    n = R.N_INIT * R.N_SEARCH * 2
    if "--patterns-only" in sys.argv:
        path = os.path.join(mg.OUT, "atk_light.npz")
        old = dict(np.load(path))
        old.update(gold_patterns(reference_modules(ref_dir)[2]))
        mg.save("atk_light", **old)
        return
    pool = multiprocessing.get_context("fork").Pool(workers)        # forked before the reference and its stand-ins come in
    Light, PhysicalTrans, light_simulation = reference_modules(ref_dir)
    keep = gold_patterns(light_simulation)
    obj, mask, scenes = R.case_inputs()
    torch.set_num_threads(2)

    for seed in R.CASE["rng_seeds"]:
        print("seed %d" % seed, flush=True)
        chunks = [list(range(lo, min(lo + 100, n))) for lo in range(0, n, 100)]
        pending = pool.map_async(_worker, [(seed, c) for c in chunks], chunksize=1)
        model = R.make_model()
        model.train()
        atk = Light(model, obj, mask, dist_range=DIST_RANGE)
        R.seed_all(seed)
        (adv_s, ben_s, m_out, patch), costs, params, poses = observe(atk, PhysicalTrans.project.__code__,
                                                                     lambda: atk(scenes, B, eval=True))
        cost32 = torch.stack(costs).numpy().astype(np.float32)
        if "--raw" in sys.argv:         # the observations as they came, before any check (a run is long)
            np.savez_compressed(sys.argv[sys.argv.index("--raw") + 1], cost=cost32, params=params, patch=patch.numpy(),
                                z0=np.asarray([p[0] for p in poses]), alpha=np.asarray([p[1] for p in poses]),
                                adv=adv_s.numpy(), ben=ben_s.numpy(), mask=m_out.numpy())
        assert model.training and len(costs) == n and len(poses) == n + 2, (len(costs), len(poses))
        # the restatement's draw order against what the reference drew
        R.seed_all(seed)
        my_params = R.draw_params()
        my_poses = R.draw_poses(DIST_RANGE, attack_ref_angles(), n, B)
        assert np.array_equal(my_params, params), "parameter draws differ from the reference's"
        # the first n projects are the queries'; the last two (adv, ben) carry the explicit samples, eval's (7, 0) in front
        assert [p for p in my_poses[:n]] == poses[:n], "pose draws differ from the reference's"
        assert poses[n] == poses[n + 1] and poses[n][0][1:] == my_poses[n][0][1:] and poses[n][1][1:] == my_poses[n][1][1:]
        cost64 = np.full(n, np.nan)
        for only, c in pending.get():
            cost64[only] = c
        e_ref = float((np.abs(cost32.astype(np.float64) - cost64) / np.abs(cost64)).max())
        best, gap = R.argmin_gap(cost32)
        thr = max(20.0 * e_ref, 1e-4)
        print("e_ref %.3g  threshold %.3g  best %d  gap %.3g  (float64 argmin %d)" % (e_ref, thr, best, gap,
                                                                                       R.argmin_gap(cost64)[0]), flush=True)
        if gap < thr:
            print("the argmin is not decidable with this seed")
            continue
        u8 = patch.squeeze(0).mul(255).round().byte().permute(1, 2, 0).contiguous().numpy()     # uint8 / 255 back to uint8: exact
        assert np.array_equal(R.to_patch(u8).numpy(), patch.numpy())
        assert np.array_equal(u8, R.pattern_u8(R.base_u8(obj), R.record(params[best]))), "the best patch is not query `best`'s"
        zi = np.asarray([[DIST_RANGE.index(v) for v in p[0]] for p in my_poses], dtype=np.int8)
        ai = np.asarray([[attack_ref_angles().index(v) for v in p[1]] for p in my_poses], dtype=np.int8)
        mg.save("atk_light", shape=np.array([B, R.N_INIT, R.N_SEARCH, seed]), stand_ins=np.array(STAND_INS), cost=cost32,
                params=params.astype(np.int16), z0_index=zi, alpha_index=ai, dist_range=np.asarray(DIST_RANGE, dtype=np.float64),
                best=np.int64(best), e_ref=np.float64(e_ref), gap=np.float64(gap), seed=np.int64(seed),
                patch_u8_sub=u8[::2, ::2], patch_u8_sum=u8.astype(np.int64).sum((0, 1)),
                adv_rows=adv_s[ROWS], ben_rows=ben_s[ROWS], mask_rows=m_out[ROWS], adv_sum=adv_s.double().sum((2, 3)),
                ben_sum=ben_s.double().sum((2, 3)), mask_out_sum=m_out.double().sum((1, 2, 3)), **keep)
        pool.terminate()
        return
    pool.terminate()
    sys.exit("no seed of light_ref.CASE['rng_seeds'] makes a decidable fixture: nothing written")


if __name__ == "__main__":
    main()
