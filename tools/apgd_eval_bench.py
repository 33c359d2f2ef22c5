"""Device and wall time of one 10-iteration Auto-PGD object attack on 12 scenes with the ResNet-18 U-Net, three ways:

    (a) Phy_obj_atk_APGD, eager                    K22 step / commit, controller on the device, no host read per iteration
    (b) Phy_obj_atk_APGD, use_graph                one captured iteration replayed steps - 1 times
    (c) ``aten_attack`` below                      the same paste / cost / gradient, but step and controller as the reference
                                                   writes them: its ATen element-wise chain and its ``.cpu()`` reads per iteration

    python tools/apgd_eval_bench.py [--attacks 7] [--out profiles/apgd_eval.txt]

(c) is a function of this tool, not a switch of the product.  The three alternate inside one process after a warm-up; the report
is the median and the spread (min .. max) of ``--attacks`` attacks each, device time from HIP events around the attack and wall
time from perf_counter around the same region with a synchronisation at its end.
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from depthmodelhardening_amd import ops                                      # noqa: E402
from depthmodelhardening_amd.depth_model import import_depth_model           # noqa: E402
from depthmodelhardening_amd.datasets import make_object                     # noqa: E402
from depthmodelhardening_amd.roi import RoiPlan                              # noqa: E402
from depthmodelhardening_amd.torchattacks import Phy_obj_atk_APGD            # noqa: E402


def aten_attack(atk, images, batch_size):
    """attack_single_run of the reference (phy_obj_atk_apgd.py:133-292) on this project's paste / cost / gradient: the update and
    the controller are the reference's own op chain, host reads included.  Returns the patch (x_best_adv)."""
    dev, steps, eps = atk.device, int(atk.steps), atk.eps
    x = atk.obj_img.detach().to(dev)
    mask = atk.obj_mask.to(dev)
    pt = atk.phy_trans_ben
    t = atk.random_start_noise.to(dev)
    x_adv = x + eps * torch.ones([1, 1, 1, 1], device=dev) * t / t.reshape([1, -1]).abs().max(dim=1, keepdim=True)[0].reshape([-1, 1, 1, 1])
    x_adv = x_adv.clamp(0., 1.)
    z0, al = pt.draw_samples(batch_size, rs=np.random.RandomState(atk.seed))
    coeffs = atk._coeffs([(z0, al)])
    plan = RoiPlan(pt.mask_boxes(z0, al, atk.scene_size), *atk.scene_size, depth=ops.ROI_DEPTH)
    tab = plan.device_table(dev)
    with torch.no_grad():
        clean, _ = ops.eot_paste(images, atk.obj_img, torch.zeros_like(mask), coeffs[0], pt.l_pad, pt.t_pad, atk.scene_size)
    one = torch.ones((), device=dev)

    def cost_and_grad(xa):
        p = xa.detach().requires_grad_(True)
        adv, m = ops.eot_paste(images, p, mask, coeffs[0], pt.l_pad, pt.t_pad, atk.scene_size)
        cost = atk._neg_cost(adv, m, plan, tab, clean)
        (g,) = torch.autograd.grad(cost, p, grad_outputs=one)
        return cost.detach().reshape(1), g

    steps_2, steps_min, size_decr = max(int(0.22 * steps), 1), max(int(0.06 * steps), 1), max(int(0.03 * steps), 1)
    x_best, x_best_adv = x_adv.clone(), x_adv.clone()
    loss_steps = torch.zeros([steps, 1])
    loss_indiv, grad = cost_and_grad(x_adv)
    grad_best, loss_best = grad.clone(), loss_indiv.clone()
    step_size = eps * torch.ones([1, 1, 1, 1], device=dev) * torch.tensor([2.0], device=dev).reshape([1, 1, 1, 1])
    x_adv_old = x_adv.clone()
    k, counter3 = steps_2, 0
    loss_best_last_check = loss_best.clone()
    reduced_last_check = np.ones(1, dtype=bool)
    u = np.arange(1)
    for i in range(steps):
        with torch.no_grad():
            grad2 = x_adv - x_adv_old
            x_adv_old = x_adv.clone()
            a = 0.75 if i > 0 else 1.0
            x_adv_1 = x_adv + step_size * torch.sign(grad)
            x_adv_1 = torch.clamp(torch.min(torch.max(x_adv_1, x - eps), x + eps), 0.0, 1.0)
            x_adv_1 = torch.clamp(torch.min(torch.max(x_adv + (x_adv_1 - x_adv) * a + grad2 * (1 - a), x - eps), x + eps), 0.0, 1.0)
            x_adv = x_adv_1 + 0.
        loss_indiv, grad = cost_and_grad(x_adv)
        x_best_adv = x_adv + 0.
        with torch.no_grad():
            y1 = loss_indiv.clone()
            loss_steps[i] = y1.cpu() + 0
            ind = (y1 > loss_best).nonzero(as_tuple=False).squeeze()
            x_best[ind] = x_adv[ind].clone()
            grad_best[ind] = grad[ind].clone()
            loss_best[ind] = y1[ind] + 0
            counter3 += 1
            if counter3 == k:
                hist = loss_steps.numpy()
                rose = np.zeros(1)
                for c in range(k):
                    rose += hist[i - c] > hist[i - c - 1]
                fl = rose <= k * atk.thr_decr * np.ones(1)
                no_impr = (~reduced_last_check) * (loss_best_last_check.cpu().numpy() >= loss_best.cpu().numpy())
                fl = ~(~fl * ~no_impr)
                reduced_last_check = np.copy(fl)
                loss_best_last_check = loss_best.clone()
                if np.sum(fl) > 0:
                    step_size[u[fl]] /= 2.0
                    w = np.where(fl)
                    x_adv[w] = x_best[w].clone()
                    grad[w] = grad_best[w].clone()
                counter3 = 0
                k = max(k - size_decr, steps_min)
    return x_best_adv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attacks", type=int, default=7)
    ap.add_argument("--scenes", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = import_depth_model((1024, 320)).to(dev).eval()
    obj, mask = make_object(dev)
    B = args.scenes
    scenes = torch.rand(B, 3, 375, 1242, generator=torch.Generator().manual_seed(3)).to(dev)
    noise = 2 * torch.rand(obj.shape, generator=torch.Generator().manual_seed(9)) - 1

    def make(graph):
        atk = Phy_obj_atk_APGD(model, obj, mask, eps=0.1, steps=args.steps, dist_range=list(np.arange(5, 10, 0.2)))
        atk.random_start_noise = noise
        atk.use_graph = graph
        return atk
    eager, graph, chain = make(False), make(True), make(False)

    def run_chain():
        model.eval()
        with ops.frozen_weights():
            return aten_attack(chain, scenes, B)
    forms = [("a: K22, eager", lambda: eager(scenes, B)[3]), ("b: K22, HIP graph", lambda: graph(scenes, B)[3]),
             ("c: ATen chain + host reads", run_chain)]
    patches = {}
    for _ in range(2):                      # warm-up: kernel caches, the graph's memory pool
        for name, fn in forms:
            random.seed(1)
            patches[name] = fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(args.attacks):
        for name, fn in forms:
            random.seed(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append((e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3))
    names = [n for n, _ in forms]
    lines = ["Auto-PGD object attack: %d iterations, %d scenes, ResNet-18 U-Net 320x1024, %d attacks per form, alternating"
             % (args.steps, B, args.attacks),
             "graph_failure of (b): %r" % (graph.graph_failure,),
             "patch texels of (b) equal to (a): %.6f   of (c) equal to (a): %.6f" % (
                 (patches[names[1]] == patches[names[0]]).float().mean().item(),
                 (patches[names[2]] == patches[names[0]]).float().mean().item()),
             "%-30s %28s %28s" % ("form", "device ms  median (min..max)", "wall ms  median (min..max)")]
    for name in names:
        d, w = [t[0] for t in times[name]], [t[1] for t in times[name]]
        lines.append("%-30s %10.2f (%7.2f ..%7.2f) %12.2f (%7.2f ..%7.2f)" % (name, statistics.median(d), min(d), max(d),
                                                                             statistics.median(w), min(w), max(w)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
