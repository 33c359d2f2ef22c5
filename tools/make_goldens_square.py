"""Writes tests/golden/atk_square.npz: the reference's own ``Phy_obj_atk_Square`` on the seeded inputs of tests/square_ref.py.

    python tools/make_goldens_square.py [--reference DIR]

The reference package is imported the way tools/make_goldens_gauss.py imports it (oracle/make_goldens.install_shims, a temporary
calibration file).  Three parts.

``sched_*``: the side of the square per iteration from the reference's own ``p_selection`` and side formula (:281), for
square_ref.SCHEDULE_CASES.

``script_*``: the reference's own search loop on small objects, driven by a scripted loss.  A subclass made here overrides only
``depth_loss``: it records its argument and returns the next value of square_ref.SCRIPT (accepts, rejects, an exact tie, a NaN);
``random_int`` / ``random_choice`` are wrapped on the instance to record every draw.  Line :295 hands ``x_best`` to depth_loss,
so the recorded arguments ARE x_best after every query (the value perturb() returns closes the list): this pins the draw stream,
the strict accept rule, and the candidate ``x_new`` -- seen after each accept as the next argument.

``e2e_*``: the unmodified class (observed through wrappers set on the instance) on the 260 x 300 object with the siblings' toy
model, B = 2, n_queries = 6, eval=True.  Written only if all 7 reference costs are bit-identical and the returned patch equals
the start stripes -- what line :295 implies with fixed poses and a deterministic model.
"""
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import attack_ref              # noqa: E402
from oracle import make_goldens as mg      # noqa: E402
from oracle import synth                   # noqa: E402
from tests import square_ref as R          # noqa: E402

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
    return ta.Phy_obj_atk_Square


def record_draws(atk):
    """Wraps random_int / random_choice on the instance; returns the list that receives (kind, high or shape, tensor)."""
    log = []
    r_int, r_choice = atk.random_int, atk.random_choice

    def random_int(low=0, high=1, shape=[1]):
        t = r_int(low, high, shape)
        log.append(("int", high, t.clone()))
        return t

    def random_choice(shape):
        t = r_choice(shape)
        log.append(("choice", tuple(shape), t.clone()))
        return t
    atk.random_int, atk.random_choice = random_int, random_choice
    return log


def gold_schedule(Square):
    keep = {}
    for n, resc, (h, w) in R.SCHEDULE_CASES:
        atk = Square(R.make_model(), torch.zeros(1, 3, h, w), torch.ones(1, 1, h, w), n_queries=n, resc_schedule=resc)
        import math
        s = [max(int(round(math.sqrt(atk.p_selection(i) * (3 * h * w) / 3))), 1) for i in range(n)]
        assert s == R.sides(n, 3, h, w, 0.8, resc), (n, resc, h, w)
        keep["sched_%d_%d_%dx%d" % (n, int(resc), h, w)] = np.asarray(s, dtype=np.int32)
    return keep


def gold_script(Square, name, case):
    c, h, w = case["shape"]
    x0 = torch.from_numpy(R.script_object(case["shape"]))
    n = len(R.SCRIPT) - 1
    seen = []

    class Scripted(Square):
        def depth_loss(self, x_adv, scene_imgs):
            seen.append(x_adv.clone())
            return torch.ones(x_adv.shape[0]), torch.tensor([R.SCRIPT[len(seen) - 1]], dtype=torch.float32)

    atk = Scripted(R.make_model(), x0, torch.ones(1, 1, h, w), eps=case["eps"], n_queries=n, p_init=case["p_init"],
                   resc_schedule=case["resc"])
    log = record_draws(atk)
    torch.manual_seed(case["seed"])
    final = atk.perturb(None)
    assert len(seen) == n + 1 and len(log) == 1 + 3 * n, (len(seen), len(log))
    after = torch.stack(seen[1:] + [final], 0).numpy()
    stripes = log[0][2].numpy().reshape(c, w)
    vh = np.asarray([int(log[1 + 3 * i][2]) for i in range(n)])
    vw = np.asarray([int(log[2 + 3 * i][2]) for i in range(n)])
    s = np.asarray([h - log[1 + 3 * i][1] for i in range(n)])
    assert np.array_equal(s, [w - log[2 + 3 * i][1] for i in range(n)])
    signs = np.stack([log[3 + 3 * i][2].numpy().reshape(c) for i in range(n)], 0)
    # the restatement on the same stream and script
    torch.manual_seed(case["seed"])
    st2, vh2, vw2, s2, sg2 = R.draw(n, c, h, w, case["p_init"], case["resc"])
    assert np.array_equal(st2, stripes) and np.array_equal(vh2, vh) and np.array_equal(vw2, vw) and np.array_equal(s2, s) \
        and np.array_equal(sg2, signs), "the restatement's draws differ from the reference's"
    mine, _, accepted, last = R.search(x0.numpy(), R.table_of(vh, vw, s, signs), stripes, case["eps"], lambda p, q: R.SCRIPT[q], "best")
    assert np.array_equal(mine, after) and np.array_equal(last, after[-1]), "the restatement's x_best differs from the reference's"
    print("script %s: %s, squares %s, accepted %s" % (name, case["shape"], s.tolist(), accepted))
    assert len(accepted) >= 4
    pre = "script_%s_" % name
    return {pre + "x0": x0.numpy(), pre + "stripes": stripes, pre + "vh": vh, pre + "vw": vw, pre + "s": s, pre + "signs": signs,
            pre + "x_best": after, pre + "loss": np.asarray(R.SCRIPT, dtype=np.float32), pre + "accepted": np.asarray(accepted)}


def gold_e2e(Square):
    case = R.CASE
    B, n, seed = case["batch"], case["n_queries"], case["rng_seed"]
    obj, mask, scenes = R.case_inputs()
    model = R.make_model()
    model.train()
    atk = Square(model, obj, mask, eps=case["eps"], n_queries=n, seed=case["pose_seed"], dist_range=DIST_RANGE)
    log = record_draws(atk)
    costs, poses = [], []
    depth_loss, project = atk.depth_loss, atk.phy_trans_adv.project

    def observed_loss(x_adv, scene_imgs):
        out = depth_loss(x_adv, scene_imgs)
        costs.append(out[1].detach().clone())
        return out

    def observed_project(*a, **k):
        out = project(*a, **k)
        poses.append(([float(v) for v in out[2]], [int(v) for v in out[3]]))
        return out
    atk.depth_loss, atk.phy_trans_adv.project = observed_loss, observed_project
    R.seed_all(seed)
    adv_s, ben_s, m_out, patch = atk(scenes, B, eval=True)
    assert model.training and len(costs) == n + 1 and len(poses) == n + 2, (len(costs), len(poses))
    cost32 = torch.cat(costs).numpy().astype(np.float32)
    print("reference costs %s" % cost32)
    assert len(set(cost32.tobytes()[4 * i:4 * i + 4] for i in range(n + 1))) == 1, "the reference's costs are not bit-identical"
    stripes = log[0][2].numpy().reshape(3, -1)
    start = torch.clamp(obj + case["eps"] * log[0][2], 0., 1.)
    assert torch.equal(patch, start), "the reference's patch is not the start stripes"
    angles = list(attack_ref.ANGLE_RANGE)
    z0, al = R.rs_poses(DIST_RANGE, angles, B, case["pose_seed"])
    assert all(p == ([float(v) for v in z0], [int(v) for v in al]) for p in poses[:n + 1]), "RandomState poses differ"
    R.seed_all(seed)
    fz, fa = R.final_poses(DIST_RANGE, angles, B, eval=True)
    assert poses[n + 1] == ([float(v) for v in fz], [int(v) for v in fa]), "final poses differ"
    # e_ref: the reference's fp32 cost against a float64 run of the restatement on the same patch and poses
    model.eval()
    c32 = float(R.depth_cost(model, patch, mask, scenes, B, z0, al, DIST_RANGE))
    c64 = float(R.depth_cost(R.make_model().double().eval(), patch.double(), mask.double(), scenes.double(), B, z0, al, DIST_RANGE))
    e_ref = max(abs(float(cost32[0]) - c64), abs(c32 - c64)) / abs(c64)
    _, gap = R.argmin_gap(cost32)
    print("restated cost fp32 %.9g  float64 %.12g  e_ref %.3g  gap %.3g" % (c32, c64, e_ref, gap))
    r0, r1, c0, c1 = R.REGION
    return dict(e2e_shape=np.array([B, n, seed, case["pose_seed"]]), e2e_eps=np.float64(case["eps"]), e2e_cost=cost32,
                e2e_rs_z0=np.asarray(z0, dtype=np.float64), e2e_rs_alpha=np.asarray(al, dtype=np.int64),
                e2e_final_z0=np.asarray(fz, dtype=np.float64), e2e_final_alpha=np.asarray(fa, dtype=np.int64),
                e2e_dist_range=np.asarray(DIST_RANGE, dtype=np.float64), e2e_stripes=stripes,
                e2e_patch_rect=patch[:, :, r0:r1, c0:c1], e2e_patch_sum=patch.double().sum((0, 2, 3)),
                e2e_region=np.asarray(R.REGION), e2e_e_ref=np.float64(e_ref), e2e_gap=np.float64(gap),
                e2e_adv_rows=adv_s[ROWS], e2e_ben_rows=ben_s[ROWS], e2e_mask_rows=m_out[ROWS],
                e2e_adv_sum=adv_s.double().sum((2, 3)), e2e_ben_sum=ben_s.double().sum((2, 3)),
                e2e_mask_out_sum=m_out.double().sum((1, 2, 3)))


def main():
    ref_dir = sys.argv[sys.argv.index("--reference") + 1] if "--reference" in sys.argv else mg.REF
    Square = reference_class(ref_dir)
    keep = gold_schedule(Square)
    for name, case in R.SCRIPT_CASES.items():
        keep.update(gold_script(Square, name, case))
    keep.update(gold_e2e(Square))
    mg.save("atk_square", stand_ins=np.array(STAND_INS), **keep)


if __name__ == "__main__":
    main()
