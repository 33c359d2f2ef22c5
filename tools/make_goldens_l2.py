"""Writes tests/golden/atk_l2.npz: the reference's own ``Phy_obj_atk_l2`` on the seeded inputs of tests/l2_ref.py.

    python tools/make_goldens_l2.py [--reference DIR]

The reference package is imported the way tools/make_goldens_square.py imports it (oracle/make_goldens.install_shims, a temporary
calibration file).  CPU only, seeded with tests/l2_ref.seed_all (``torch.manual_seed`` for the start draws, ``random.seed`` for the
poses).  Two parts.

``b1_*``: the unmodified class at batch_size = 1, eval=True, l2_ref.CASE["steps"] steps, the 260 x 300 object and the siblings'
toy model.  It is observed from outside: ``phy_trans_adv.reset_img`` sees the patch before every step and the final one,
``phy_trans_adv.project`` the poses, and an ``nn.MSELoss`` that remembers its results the costs.  Stored: the start draws (r whole,
the normal tensor as the siblings' REGION and its float64 sum -- the tests redraw it from the seed and check both), per-step costs
and ||patch - obj||_2, the REGION of the final patch, the sampled ROWS of the returned scenes, and e_ref: the distance of the
reference's fp32 run from tests/l2_ref.py's float64 form on the same draws.

``b2_*``: the probe at batch_size = 2, 2 steps: does the class as written run with more than one scene?  Stored: whether it
raised, the exception's type and first line, and the shapes ``reset_img`` saw until then.

A tool: not run by the tests.
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import attack_ref              # noqa: E402
from oracle import make_goldens as mg      # noqa: E402
from oracle import synth                   # noqa: E402
from tests import l2_ref as R              # noqa: E402

ROWS = (slice(None), slice(None), slice(120, 300, 9), slice(300, 800, 5))      # the row sample of the sibling fixtures
DIST_RANGE = list(np.arange(5, 10, 0.2))
STAND_INS = ["torchvision Resize / Pad / functional.perspective: oracle/tv082.py (oracle/make_goldens.install_shims)"]


def reference_class(ref_dir):
    import matplotlib
    matplotlib.use("Agg")
    mg.install_shims()
    tmp = tempfile.mkdtemp(prefix="kitti_obj_")
    os.makedirs(os.path.join(tmp, "training", "calib"))
    with open(os.path.join(tmp, "training", "calib", "003086.txt"), "w") as f:
        f.write(synth.KITTI_CALIB_TEXT)
    sys.path.insert(0, os.path.join(ref_dir, "DepthNetworks", "monodepth2"))
    sys.path.append(ref_dir)
    import my_utils
    my_utils.object_dataset_root = tmp
    import torchattacks as ta
    return ta.Phy_obj_atk_l2


class _RecordingMSE(nn.MSELoss):
    seen = []

    def forward(self, a, b):
        out = super().forward(a, b)
        _RecordingMSE.seen.append(out.detach().clone())
        return out


@contextlib.contextmanager
def observed(atk):
    """(patches reset_img saw, poses project drew, MSE results) while the block runs; the step loop's print is swallowed."""
    patches, poses = [], []
    reset_img, project = atk.phy_trans_adv.reset_img, atk.phy_trans_adv.project

    def seen_reset(obj_img, obj_mask):
        patches.append(obj_img.detach().clone())
        return reset_img(obj_img, obj_mask)

    def seen_project(*a, **k):
        out = project(*a, **k)
        poses.append(([float(v) for v in out[2]], [int(v) for v in out[3]]))
        return out
    atk.phy_trans_adv.reset_img, atk.phy_trans_adv.project = seen_reset, seen_project
    _RecordingMSE.seen = []
    plain = nn.MSELoss
    nn.MSELoss = _RecordingMSE
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            yield patches, poses, _RecordingMSE.seen
    finally:
        nn.MSELoss = plain
        atk.phy_trans_adv.reset_img, atk.phy_trans_adv.project = reset_img, project


def gold_b1(L2):
    case = R.CASE
    steps, eps, seed = case["steps"], case["eps"], case["rng_seed"]
    obj, mask, scenes = R.case_inputs(1)
    model = R.make_model()
    model.train()
    atk = L2(model, obj, mask, eps=eps, alpha=123.0, steps=steps, dist_range=DIST_RANGE)
    assert atk.alpha == R.step_alpha(eps, steps), "the constructor's alpha is not ignored"
    R.seed_all(seed)
    with observed(atk) as (patches, poses, mse):
        adv_s, ben_s, m_out, patch = atk(scenes, 1, eval=True)
    assert model.training and len(patches) == steps + 1 and len(mse) == steps and len(poses) == steps + 1, (len(patches), len(mse))
    assert tuple(patch.shape) == tuple(obj.shape) and torch.equal(patch, patches[-1])
    cost32 = -torch.stack(mse).numpy().astype(np.float32)
    norms = np.asarray([float((p.double() - obj.double()).norm()) for p in patches[1:]])
    # the same draws again, for the restatement: the start from torch's generator, the poses from Python's
    R.seed_all(seed)
    normal, r = R.draw_start(obj)
    assert torch.equal(R.random_start(obj, normal, r, eps), patches[0]), "the restatement's random start is not the reference's"
    R.seed_all(seed)
    drawn = R.draw_poses(DIST_RANGE, list(attack_ref.ANGLE_RANGE), steps, 1)
    fz, fa = list(drawn[-1][0]), list(drawn[-1][1])
    fz[0], fa[0] = 7, 0
    assert poses[:steps] == [([float(v) for v in z], [int(v) for v in a]) for z, a in drawn[:steps]], "step poses differ"
    assert poses[steps] == ([float(v) for v in fz], [int(v) for v in fa]), "final poses differ"
    tr32, tr64 = [], []
    R.phy_obj_atk_l2(R.make_model(), obj, mask, scenes, 1, eps=eps, steps=steps, random_start_draw=(normal, r),
                     dist_range=DIST_RANGE, eval=True, trace=tr32, draws=drawn[:steps], final_draw=drawn[-1])
    _, _, _, p64 = R.phy_obj_atk_l2(R.make_model().double(), obj.double(), mask.double(), scenes.double(), 1, eps=eps, steps=steps,
                                    random_start_draw=(normal.double(), r.double()), dist_range=DIST_RANGE, eval=True, trace=tr64,
                                    draws=drawn[:steps], final_draw=drawn[-1])
    c64 = np.asarray([t["cost"] for t in tr64])
    c32 = np.asarray([t["cost"] for t in tr32])
    e_cost = float((np.abs(cost32 - c64) / np.abs(c64)).max())
    e_patch = float((patch.double() - p64).abs().max())
    print("reference costs %s  norms %s" % (cost32, norms))
    print("restatement fp32 costs %s (largest distance to the reference %.3g), patch distance %.3g" % (
        c32, np.abs(c32 - cost32).max(), float((tr32[-1]["patch"] - patch).abs().max())))
    print("float64 costs %s  e_ref cost %.3g  e_ref patch %.3g  clamped texels %d" % (
        c64, e_cost, e_patch, int(((patch == 0) | (patch == 1)).sum())))
    r0, r1, c0, c1 = R.REGION
    return dict(b1_shape=np.array([1, steps, seed]), b1_eps=np.float64(eps), b1_alpha=np.float64(atk.alpha),
                b1_r=r.numpy().reshape(-1), b1_normal_rect=normal[:, :, r0:r1, c0:c1], b1_normal_sum=np.float64(normal.double().sum()),
                b1_start_rect=patches[0][:, :, r0:r1, c0:c1], b1_cost=cost32, b1_norm=norms,
                b1_z0=np.asarray([p[0] for p in poses], dtype=np.float64), b1_alpha_deg=np.asarray([p[1] for p in poses], dtype=np.int64),
                b1_dist_range=np.asarray(DIST_RANGE, dtype=np.float64), b1_region=np.asarray(R.REGION),
                b1_patch_rect=patch[:, :, r0:r1, c0:c1], b1_patch_sum=patch.double().sum((0, 2, 3)),
                b1_e_ref_cost=np.float64(e_cost), b1_e_ref_patch=np.float64(e_patch),
                b1_adv_rows=adv_s[ROWS], b1_ben_rows=ben_s[ROWS], b1_mask_rows=m_out[ROWS],
                b1_adv_sum=adv_s.double().sum((2, 3)), b1_ben_sum=ben_s.double().sum((2, 3)),
                b1_mask_out_sum=m_out.double().sum((1, 2, 3)))


def gold_b2(L2):
    case = R.CASE
    obj, mask, scenes = R.case_inputs(2)
    atk = L2(R.make_model(), obj, mask, eps=case["eps"], steps=2, dist_range=DIST_RANGE)
    R.seed_all(case["rng_seed"])
    raised, kind, text, out_shapes = False, "", "", []
    with observed(atk) as (patches, poses, mse):
        try:
            out = atk(scenes, 2, eval=True)
            out_shapes = [list(t.shape) for t in out]
        except Exception as e:      # whatever it is, it is the finding
            raised, kind, text = True, type(e).__name__, (str(e).splitlines() or [""])[0]
    shapes = [list(p.shape) for p in patches]
    print("B = 2: raised %s %s %r; reset_img saw %s; %d costs; returned %s" % (raised, kind, text, shapes, len(mse), out_shapes))
    pad = lambda rows: np.asarray(rows, dtype=np.int64).reshape(-1, 4)      # noqa: E731
    return dict(b2_raised=np.bool_(raised), b2_exception=np.array(kind), b2_message=np.array(text), b2_patch_shapes=pad(shapes),
                b2_costs_seen=np.int64(len(mse)), b2_returned_shapes=pad(out_shapes), b2_steps=np.int64(2))


def main():
    ref_dir = sys.argv[sys.argv.index("--reference") + 1] if "--reference" in sys.argv else mg.REF
    L2 = reference_class(ref_dir)
    keep = gold_b1(L2)
    keep.update(gold_b2(L2))
    mg.save("atk_l2", stand_ins=np.array(STAND_INS), **keep)


if __name__ == "__main__":
    main()
