"""K38 (the backward of ManyDepth's matching cost volume, csrc/cost_volume_bwd.hip) timed on the GPU at the workload's shape.

    python tools/cost_volume_bwd_bench.py [--batch 12] [--reps 20] [--out profiles/cost_volume_bwd.txt]

(a) ``ops.cost_volume_bwd_launch`` (both gradients, ``d_current`` alone) beside K30's forward into reduce_conv's buffer, at
    80 x 256, C = 64, D = 96, batch 12, L = 1 and 2.  The poses are small enough that a good part of the grid sees all 96 bins:
    only confident columns carry gradient, and their share is printed.
(b) The same against torch-eager autograd through ``ops.cost_volume_module`` (the expression behind ``_match_features_module``, which
    allocates [D, C, H, W] per sample and lookup) on the device, forward + backward, at batch 2.
(c) One step of ``Phy_obj_atk_mf`` (paste into both frames, the wrapper, the gradient, the sign step) on 12 scenes, in the three
    gradient modes, with ``pose_translation_scale = 0.03`` (not the default 1.0), chosen so that a good part of the columns is
    confident and K38 has work.  The line says so.

Times are HIP events around ``reps`` back-to-back calls after warm-up, the median of 5 such windows with the smallest and the
largest beside it (one box, one process: read differences of a few per cent as noise).  Needs the GPU.
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from depthmodelhardening_amd import depth_model as DM, ops                  # noqa: E402
from tools.cost_volume_bench import C, D, H, W, poses_for, timed            # noqa: E402


def inputs(B, L, dev):
    torch.manual_seed(0)
    K1, invK1 = DM.manydepth_intrinsics(4 * W, 4 * H)
    K, invK = K1.to(dev).repeat(B, 1, 1), invK1.to(dev).repeat(B, 1, 1)
    bins = torch.from_numpy(np.linspace(0.1, 20.0, D)).float().to(dev)
    cur = torch.relu(torch.randn(B, C, H, W, device=dev))
    look = torch.relu(torch.randn(B, L, C, H, W, device=dev))
    poses = poses_for(B, L, dev)
    poses[:, :, :3, 3] *= 0.03
    return cur, look, poses, K, invK, bins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cost_volume_bwd_bench: needs the GPU")
    dev = torch.device("cuda")
    B = a.batch
    lines = ["tools/cost_volume_bwd_bench.py: %s, torch %s, %d x %d, C %d, D %d, %d calls per window, median [min .. max] of 5 windows"
             % (torch.cuda.get_device_name(0), torch.__version__, H, W, C, D, a.reps)]
    for L in (1, 2):
        t = inputs(B, L, dev)
        buf = torch.empty(B, C + D, H, W, device=dev)
        g = torch.randn(B, C + D, H, W, device=dev)
        conf = ops.cost_volume(*t, into=buf)[2]
        forms = [("K30 forward into the buffer", lambda: ops.cost_volume(*t, into=buf)),
                 ("K38 d_current + d_lookup", lambda: ops.cost_volume_bwd_launch(*t, g[:, C:])),
                 ("K38 d_current only", lambda: ops.cost_volume_bwd_launch(*t, g[:, C:], need_lookup=False))]
        for name, fn in forms:
            lines.append("batch %2d  L = %d  %-30s %9.3f ms  [%.3f .. %.3f]" % ((B, L, name) + timed(fn, a.reps)))
        lines.append("batch %2d  L = %d  confident columns: %.3f of all" % (B, L, float(conf.mean())))
        del buf, g, t

    Be = 2
    for L in (1, 2):
        cur, look, poses, K, invK, bins = inputs(Be, L, dev)
        g = torch.randn(Be, C + D, H, W, device=dev)

        def eager():
            c, l_ = cur.clone().requires_grad_(True), look.clone().requires_grad_(True)
            stacked = ops.cost_volume_stack_host(c, l_, poses, K, invK, bins)[0]
            return torch.autograd.grad(stacked, (c, l_), g)

        def fused():
            c, l_ = cur.clone().requires_grad_(True), look.clone().requires_grad_(True)
            stacked = ops.cost_volume_stack(c, l_, poses, K, invK, bins)[0]
            return torch.autograd.grad(stacked, (c, l_), g)

        te, tf = timed(eager, max(2, a.reps // 10)), timed(fused, a.reps)
        ge, gf = eager(), fused()
        lines.append("batch %2d  L = %d  torch eager autograd, forward + backward   %9.3f ms  [%.3f .. %.3f]" % ((Be, L) + te))
        lines.append("batch %2d  L = %d  K30 + K38 node, forward + backward         %9.3f ms  [%.3f .. %.3f]   eager / node = %.1f x" % (
            (Be, L) + tf + (te[0] / tf[0],)))
        lines.append("batch %2d  L = %d  rel-L2 to eager: d_current %.3g, d_lookup %.3g" % (
            Be, L, float((gf[0] - ge[0]).norm() / ge[0].norm()), float((gf[1] - ge[1]).norm() / ge[1].norm())))
        del cur, look, g, ge, gf

    from depthmodelhardening_amd.datasets import SyntheticKITTIDataset, make_object
    from depthmodelhardening_amd.torchattacks import Phy_obj_atk_mf
    torch.manual_seed(1)
    model = DM.import_depth_model((1024, 320), 'manydepth', matching=True).to(dev).eval()
    data = SyntheticKITTIDataset(320, 1024, [0, "s"], 4, 1 << 30, dev, seed=17, pool=max(8, B))
    scenes, lookups = data.next_scene_pairs(B)
    obj, mask = make_object(dev)
    T = np.eye(4)
    T[2, 3] = 0.8
    PTS = 0.03
    for mode in ("none", "current", "full"):
        atk = Phy_obj_atk_mf(model, obj, mask, eps=0.1, alpha=0.02, steps=1, matching_grad=mode, pose_translation_scale=PTS)
        random.seed(7)
        t = timed(lambda: atk(scenes, B, lookup_images=lookups, T_lookup=T), max(2, a.reps // 4))
        lines.append("Phy_obj_atk_mf, %2d scenes, 1 step + the returned scenes, pose_translation_scale %g, matching_grad = %-8s %9.3f ms  [%.3f .. %.3f]" % (
            (B, PTS, repr(mode)) + t))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
