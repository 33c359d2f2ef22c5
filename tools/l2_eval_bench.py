"""Wall and device time of the L2 object attack (40 steps by default) on 12 scenes of 375 x 1242 with the ResNet-18 U-Net, three
ways:

    (a) Phy_obj_atk_l2                       the update as K28 (two launches)
    (b) Phy_obj_atk_l2(torch_step=True)      the update as the reference's chain of torch expressions (phy_obj_atk_l2.py:110-120):
                                             the baseline, since no earlier revision serves this row
    (c) Phy_obj_atk_l2(use_graph=True)       (a) with the step replayed from a HIP graph

    python tools/l2_eval_bench.py [--attacks 5] [--steps 40] [--scenes 12] [--out profiles/l2_eval.txt]

The forms alternate inside one process after a warm-up (a short attack of each); the report is the median and the spread of
``--attacks`` attacks each: wall time from perf_counter around the whole call with a synchronisation at its end, device time from
HIP events around the same region.  The update alone, (a) against (b), is also timed with HIP events on the patch's 234,000
elements.  Kernel launches per step are counted with the profiler as the slope between two short attacks of each eager form.
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

from depthmodelhardening_amd.depth_model import import_depth_model           # noqa: E402
from depthmodelhardening_amd.datasets import make_object                     # noqa: E402
from depthmodelhardening_amd.torchattacks import Phy_obj_atk_l2              # noqa: E402


def launches_per_step(make, scenes, B, steps=3):
    """What one more step launches: the slope between two short attacks (set-up and the two final pastes cancel)."""
    from torch.profiler import ProfilerActivity, profile
    random.seed(1)
    make(steps)(scenes, B)          # warm
    torch.cuda.synchronize()
    counts = []
    for q in (steps, steps * 3):
        atk = make(q)
        random.seed(1)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            atk(scenes, B)
            torch.cuda.synchronize()
        counts.append((q, sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                                             and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())))
    (n0, k0), (n1, k1) = counts
    return (k1 - k0) / float(n1 - n0)


def update_us(atk, repeats=200):
    """Median HIP-event time of one update on the patch, in microseconds: ``repeats`` updates between two events, five times."""
    x = torch.clamp(atk.obj_img + 0.01 * torch.randn_like(atk.obj_img), 0, 1)
    grad = torch.randn_like(x)
    out = torch.empty_like(x)
    for _ in range(10):
        atk._step(x, grad, out=out)
    res = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(repeats):
            atk._step(x, grad, out=out)
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / repeats)
    return statistics.median(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attacks", type=int, default=5)
    ap.add_argument("--scenes", type=int, default=12)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--eps", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = import_depth_model((1024, 320)).to(dev).eval()
    obj, mask = make_object(dev)
    B, n = args.scenes, args.steps
    scenes = torch.rand(B, 3, 375, 1242, generator=torch.Generator().manual_seed(3)).to(dev)
    normal = torch.randn(obj.shape, generator=torch.Generator().manual_seed(4))

    def make(form, steps=n):
        atk = Phy_obj_atk_l2(model, obj, mask, eps=args.eps, steps=steps, dist_range=list(np.arange(5, 10, 0.2)))
        atk.random_start_noise = (normal, 0.5)
        atk.torch_step, atk.use_graph = form == "torch", form == "graph"
        return atk
    forms = [("a: K28", "k28"), ("b: torch expressions", "torch"), ("c: K28, HIP graph", "graph")]
    per_step = {name: launches_per_step(lambda k, f=form: make(f, k), scenes, B) for name, form in forms[:2]}
    for _, form in forms:           # warm-up: a short attack of each
        random.seed(1)
        make(form, 4)(scenes, B)
    torch.cuda.synchronize()
    attackers = {name: make(form) for name, form in forms}      # (c) keeps its pool and workspace from attack to attack
    times, patches = {name: [] for name, _ in forms}, {}
    for r in range(args.attacks):
        for name, _ in forms:
            atk = attackers[name]
            random.seed(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            patch = atk(scenes, B)[3]
            e1.record()
            torch.cuda.synchronize()
            times[name].append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)))
            patches[name] = patch.clone()
    (na, _), (nb, _), (nc, _) = forms
    ua, ub = update_us(attackers[na]), update_us(attackers[nb])
    lines = ["L2 object attack: %d steps, eps %g, %d scenes of 375x1242, ResNet-18 U-Net 320x1024, %d attacks per form, alternating"
             % (n, args.eps, B, args.attacks),
             "the update alone on %d elements (HIP events, 200 back to back): K28 %.1f us, torch expressions %.1f us" % (
                 obj.numel(), ua, ub),
             "graph failure: %s;  largest |patch(a) - patch(b)| %.3g;  ||patch(a) - obj|| %.4f" % (
                 attackers[nc].graph_failure, float((patches[na] - patches[nb]).abs().max()), float((patches[na] - obj).norm())),
             "%-24s %30s %16s %14s %14s" % ("form", "wall ms  median (min..max)", "device-span ms", "ms per step", "launches/step")]
    for name, _ in forms:
        w, d = [t[0] for t in times[name]], [t[1] for t in times[name]]
        lines.append("%-24s %10.1f (%8.1f ..%8.1f) %16.1f %14.4f %14s" % (
            name, statistics.median(w), min(w), max(w), statistics.median(d), statistics.median(w) / n,
            "%.1f" % per_step[name] if name in per_step else "1 graph"))
    med = {name: statistics.median([t[0] for t in times[name]]) for name, _ in forms}
    spread = max(max(t[0] for t in times[name]) - min(t[0] for t in times[name]) for name in (na, nb))
    lines.append("(a) - (b) wall time: %.1f ms (%.3f of (b)); run-to-run spread of the two forms: %.1f ms;  (c) / (a): %.3f" % (
        med[na] - med[nb], med[na] / med[nb], spread, med[nc] / med[na]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
