"""Writes tests/golden/atk_gauss.npz: the reference's own ``Phy_obj_atk_guassian`` and ``Phy_obj_atk_arbi`` and scipy's
``gaussian_filter`` on the seeded inputs of tests/gauss_ref.py.

    python tools/make_goldens_gauss.py [--reference DIR]

The reference package is imported the way tools/make_goldens_light.py imports it (oracle/make_goldens.install_shims, a temporary
calibration file).  ``forward`` is observed with ``sys.settrace`` -- cost and sigma at the line of ``if cost < best_cost``, the
pose draw at the return of PhysicalTrans.project -- and is not edited.  The reference imports ``gaussian_filter`` from
``scipy.ndimage.filters``, a module name newer scipy releases drop: the tool installs a stand-in of its own that binds it to the
real ``scipy.ndimage.gaussian_filter`` (``STAND_INS`` below, copied into the fixture's metadata).

Three parts.  ``windows``: np.clip(gaussian_filter(x, [0, 0, s, s]), 0, 1) by scipy at the shapes and sigmas of the kernel test
(gauss_ref.SMALL_SHAPES whole, 260 x 300 on the default rectangle), so that GPU tests need no scipy.  ``attack``: a 10-step run
of the reference class; written only if the argmin is decidable: the relative gap between the two smallest reference costs is at
least max(20 e_ref, 1e-4), e_ref = the largest relative distance between the reference's fp32 costs and a float64 run of the
restatement.  Otherwise the next seed of gauss_ref.CASE["rng_seeds"] is tried; with none left the tool exits and writes nothing.
``arbi``: two consecutive calls of one ``Phy_obj_atk_arbi`` instance, with the fill branch each of them drew.
"""
import inspect
import os
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import attack_ref              # noqa: E402
from oracle import make_goldens as mg      # noqa: E402
from oracle import synth                   # noqa: E402
from tests import gauss_ref as R           # noqa: E402

ROWS = (slice(None), slice(None), slice(120, 300, 9), slice(300, 800, 5))      # the row sample of atk_linf / atk_apgd / atk_light
DIST_RANGE = list(np.arange(5, 10, 0.2))
STAND_INS = ["scipy.ndimage.filters: a module whose gaussian_filter is scipy.ndimage.gaussian_filter",
             "torchvision Resize / Pad / functional.perspective: oracle/tv082.py (oracle/make_goldens.install_shims)"]


def reference_classes(ref_dir):
    import matplotlib
    matplotlib.use("Agg")
    mg.install_shims()
    import scipy.ndimage
    filters = types.ModuleType("scipy.ndimage.filters")
    filters.gaussian_filter = scipy.ndimage.gaussian_filter
    sys.modules["scipy.ndimage.filters"] = filters
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
    return ta.Phy_obj_atk_guassian, ta.Phy_obj_atk_arbi, physicalTrans.PhysicalTrans


def observe(atk, project_code, call):
    """Runs ``call()``; returns (its result, costs, sigmas, pose draws): the cost and the sigma of every step read at the line of
    ``if cost < best_cost`` (none for a forward without that line), and (z0_sample, alpha_sample) at the return of every
    PhysicalTrans.project."""
    fwd = type(atk).forward
    code = fwd.__code__
    src = inspect.getsource(fwd).splitlines()
    lines = [code.co_firstlineno + i for i, s in enumerate(src) if s.strip().startswith("if cost < best_cost")]
    costs, sig, poses = [], [], []

    def in_forward(frame, event, arg):
        if event == "line" and frame.f_lineno in lines:
            loc = frame.f_locals
            costs.append(loc["cost"].detach().clone())
            sig.append(float(loc["sigmas"][-1]))
            assert list(loc["sigmas"][:2]) == [0, 0] and loc["sigmas"][-2] == loc["sigmas"][-1]
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
    return out, costs, sig, poses


def gold_windows():
    """scipy on the kernel test's inputs; the restatement is held to it here too."""
    from scipy.ndimage import gaussian_filter
    keep = {}
    for h, w, _ in R.SMALL_SHAPES:
        x = R.kernel_input(h, w)
        for k, s in enumerate(R.small_sigmas(h, w)):
            ref = np.clip(gaussian_filter(x, [0, 0, s, s]), 0, 1)
            assert ref.dtype == np.float32 and np.array_equal(ref, R.blur(x, s)), (h, w, s)
            keep["win_%dx%d_%d" % (h, w, k)] = ref
    x = R.kernel_input(260, 300)
    sig = R.sigmas(10, 260, 300)
    r0, r1, c0, c1 = R.REGION
    big = np.concatenate([np.clip(gaussian_filter(x, [0, 0, sig[i - 1], sig[i - 1]]), 0, 1)[:, :, r0:r1, c0:c1] for i in R.BIG_STEPS], 0)
    for j, i in enumerate(R.BIG_STEPS):
        differs = int((R.blur(x, sig[i - 1], R.REGION) != big[j:j + 1]).sum())
        print("260 x 300, sigma %r: the restatement differs from scipy in %d values" % (sig[i - 1], differs))
        assert differs == 0
    keep.update(win_big=big, win_big_sigma=np.asarray([sig[i - 1] for i in R.BIG_STEPS], dtype=np.float64))
    return keep


def gold_arbi(Arbi, PhysicalTrans, obj, mask, scenes, B):
    model = R.make_model()
    atk = Arbi(model, obj, mask, dist_range=DIST_RANGE)
    rs = np.random.RandomState(17)
    r0, r1, c0, c1 = R.REGION
    keep, kinds = {}, []
    for call in range(2):
        (adv_s, ben_s, m_out, patch), _, _, poses = observe(atk, PhysicalTrans.project.__code__, lambda: atk(scenes, B, eval=True))
        fill, kind = R.arbi_fill(rs, tuple(obj.shape))
        assert np.array_equal(R.with_window(obj, fill).numpy(), patch.numpy()), "the restatement's fill is not the reference's"
        z0, al = R.arbi_poses(B, eval=True)
        assert poses[0] == poses[1] == ([float(v) for v in z0], [int(v) for v in al]), poses
        kinds.append(kind)
        keep.update({"arbi%d_rect" % call: patch[:, :, r0:r1, c0:c1], "arbi%d_adv_rows" % call: adv_s[ROWS],
                     "arbi%d_ben_rows" % call: ben_s[ROWS], "arbi%d_mask_rows" % call: m_out[ROWS],
                     "arbi%d_adv_sum" % call: adv_s.double().sum((2, 3)), "arbi%d_z0" % call: np.asarray(poses[0][0]),
                     "arbi%d_alpha" % call: np.asarray(poses[0][1], dtype=np.int64)})
    print("arbi: the two calls drew %s" % kinds)
    keep["arbi_fills"] = np.array(kinds)
    return keep


def main():
    ref_dir = sys.argv[sys.argv.index("--reference") + 1] if "--reference" in sys.argv else mg.REF
    Gauss, Arbi, PhysicalTrans = reference_classes(ref_dir)
    B, steps = R.CASE["batch"], R.CASE["steps"]
    keep = gold_windows()
    obj, mask, scenes = R.case_inputs()
    keep.update(gold_arbi(Arbi, PhysicalTrans, obj, mask, scenes, B))
    angles = list(attack_ref.ANGLE_RANGE)
    r0, r1, c0, c1 = R.REGION
    for seed in R.CASE["rng_seeds"]:
        print("seed %d" % seed, flush=True)
        model = R.make_model()
        model.train()
        atk = Gauss(model, obj, mask, steps=steps, dist_range=DIST_RANGE)
        R.seed_all(seed)
        (adv_s, ben_s, m_out, patch), costs, sig, poses = observe(atk, PhysicalTrans.project.__code__,
                                                                  lambda: atk(scenes, B, eval=True))
        cost32 = torch.stack(costs).numpy().astype(np.float32)
        assert model.training and len(costs) == steps and len(poses) == steps + 2, (len(costs), len(poses))
        assert sig == R.sigmas(steps, *obj.shape[-2:]), "the sigma schedule differs from the reference's"
        R.seed_all(seed)
        my_poses = R.draw_poses(DIST_RANGE, angles, steps, B)
        assert my_poses[:steps] == poses[:steps], "pose draws differ from the reference's"
        # the last two projects (adv, ben) carry the explicit samples, eval's (7, 0) in front
        assert poses[steps] == poses[steps + 1] and poses[steps][0][1:] == my_poses[steps][0][1:] \
            and poses[steps][1][1:] == my_poses[steps][1][1:]
        tr = {}
        R.phy_obj_atk_guassian(R.make_model(), obj, mask, scenes, B, steps=steps, dist_range=DIST_RANGE, eval=True, trace=tr,
                               poses=my_poses)
        cost64 = R.costs64(R.make_model, obj, mask, scenes, B, steps, my_poses, DIST_RANGE, tr["windows"])
        e_ref = float((np.abs(cost32.astype(np.float64) - cost64) / np.abs(cost64)).max())
        best, gap = R.argmin_gap(cost32)
        thr = max(20.0 * e_ref, 1e-4)
        print("costs %s\ne_ref %.3g  threshold %.3g  best %d  gap %.3g  (float64 argmin %d)" % (
            cost32, e_ref, thr, best, gap, R.argmin_gap(cost64)[0]), flush=True)
        if gap < thr:
            print("the argmin is not decidable with this seed")
            continue
        rect = patch[:, :, r0:r1, c0:c1].numpy()
        assert np.array_equal(rect, tr["windows"][best:best + 1]), "the best patch is not step `best`'s"
        assert np.array_equal(R.with_window(obj, rect).numpy(), patch.numpy()), "the patch differs from the object outside the rectangle"
        zi = np.asarray([[DIST_RANGE.index(v) for v in p[0]] for p in my_poses], dtype=np.int8)
        ai = np.asarray([[angles.index(v) for v in p[1]] for p in my_poses], dtype=np.int8)
        mg.save("atk_gauss", shape=np.array([B, steps, seed]), stand_ins=np.array(STAND_INS), cost=cost32,
                sigma=np.asarray(sig, dtype=np.float64), z0_index=zi, alpha_index=ai,
                dist_range=np.asarray(DIST_RANGE, dtype=np.float64), best=np.int64(best), e_ref=np.float64(e_ref),
                gap=np.float64(gap), seed=np.int64(seed), region=np.asarray(R.REGION), patch_rect=rect,
                adv_rows=adv_s[ROWS], ben_rows=ben_s[ROWS], mask_rows=m_out[ROWS], adv_sum=adv_s.double().sum((2, 3)),
                ben_sum=ben_s.double().sum((2, 3)), mask_out_sum=m_out.double().sum((1, 2, 3)), **keep)
        return
    sys.exit("no seed of gauss_ref.CASE['rng_seeds'] makes a decidable fixture: nothing written")


if __name__ == "__main__":
    main()
