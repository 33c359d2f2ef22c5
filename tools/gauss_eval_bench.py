"""Wall and device time of the Gaussian-blur object attack (40 steps by default) on 12 scenes of 375 x 1242 with the ResNet-18
U-Net, two ways:

    (a) Phy_obj_atk_guassian                     K26 windows for all steps before the loop, compose / K24 commit per step, every
                                                 draw made up front, no host read per step
    (b) Phy_obj_atk_guassian(host_chain=True)    the reference's loop shape on the same paste / cost kernels: the blur in numpy on
                                                 the host (the rectangle only), an upload and a host comparison per step

    python tools/gauss_eval_bench.py [--attacks 7] [--steps 40] [--scenes 12] [--out profiles/gauss_eval.txt]

(b) stands for the reference's loop with scipy's C filter over the whole 3 x 260 x 300 patch replaced by a numpy loop over the
rectangle: the two are not the same host cost, so the report also times scipy's own call per step where scipy is installed.  The
two forms alternate inside one process after a warm-up (a short attack of each); the report is the median and the spread of
``--attacks`` attacks each: wall time from perf_counter around the whole call with a synchronisation at its end, device time from
HIP events around the same region, and the part of the wall time the host spent enqueuing the step loop.  K26's two launches are
timed on their own with HIP events.  Kernel launches per step are counted with the profiler on a separate short attack of each
form.
"""
import argparse
import contextlib
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from depthmodelhardening_amd.depth_model import import_depth_model           # noqa: E402
from depthmodelhardening_amd.datasets import make_object                     # noqa: E402
from depthmodelhardening_amd import ops                                       # noqa: E402
from depthmodelhardening_amd.torchattacks import Phy_obj_atk_guassian        # noqa: E402


def seed_all(seed):
    import random
    random.seed(seed)
    np.random.seed(seed)


def launches_per_step(make, scenes, B, steps=2):
    """What one more step launches: the slope between two short attacks (set-up and the two final pastes cancel)."""
    from torch.profiler import ProfilerActivity, profile
    atk = make(steps)
    seed_all(1)
    atk(scenes, B)          # warm
    torch.cuda.synchronize()
    counts = []
    for q in (steps, steps * 3):
        atk = make(q)
        seed_all(1)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            atk(scenes, B)
            torch.cuda.synchronize()
        counts.append((q, sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                                             and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())))
    (n0, k0), (n1, k1) = counts
    return (k1 - k0) / float(n1 - n0)


def windows_ms(obj, steps, repeats=5):
    """Median HIP-event time of K26's two launches for all ``steps`` windows of the default rectangle."""
    dev = obj.device
    weights, radii = (torch.from_numpy(v).to(dev) for v in ops.gauss_blur_table(ops.gauss_sigmas(steps, *obj.shape[-2:])))
    ops.gauss_blur_windows(obj, weights, radii)
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.gauss_blur_windows(obj, weights, radii)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def scipy_ms(obj, steps):
    """Host time of the reference's own filter call per step (whole patch), or None without scipy."""
    try:
        from scipy.ndimage import gaussian_filter
    except ImportError:
        return None
    x0 = obj.cpu().numpy()
    t = time.perf_counter()
    for s in ops.gauss_sigmas(steps, *obj.shape[-2:]):
        np.clip(gaussian_filter(x0, [0, 0, s, s]), 0, 1)
    return (time.perf_counter() - t) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attacks", type=int, default=7)
    ap.add_argument("--scenes", type=int, default=12)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = import_depth_model((1024, 320)).to(dev).eval()
    obj, mask = make_object(dev)
    B = args.scenes
    scenes = torch.rand(B, 3, 375, 1242, generator=torch.Generator().manual_seed(3)).to(dev)
    n = args.steps
    enqueue = []

    @contextlib.contextmanager
    def stamp():
        t = time.perf_counter()
        yield
        enqueue.append(time.perf_counter() - t)

    def make(host, steps=args.steps):
        atk = Phy_obj_atk_guassian(model, obj, mask, dist_range=list(np.arange(5, 10, 0.2)), steps=steps, host_chain=host)
        atk.loop_context = stamp
        return atk
    forms = [("a: K26, device loop", False), ("b: host chain", True)]
    per_step = {name: launches_per_step(lambda k, h=host: make(h, k), scenes, B) for name, host in forms}
    results, times = {}, {name: [] for name, _ in forms}
    for r in range(args.attacks):
        for name, host in forms:
            atk = make(host)
            del enqueue[:]
            seed_all(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            patch = atk(scenes, B)[3]
            e1.record()
            torch.cuda.synchronize()
            times[name].append(((time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), enqueue[0] * 1e3 if enqueue else float("nan")))
            results[name] = (atk.best_index, atk.costs.copy(), patch.clone())
    (na, _), (nb, _) = forms
    k26, sp = windows_ms(obj, n), scipy_ms(obj, n)
    lines = ["Gaussian-blur object attack: %d steps, %d scenes of 375x1242, ResNet-18 U-Net 320x1024, %d attacks per form, alternating"
             % (n, B, args.attacks),
             "K26 gauss_blur_windows, all %d steps (two launches): %.3f ms;  scipy gaussian_filter + clip on the host: %s" % (
                 n, k26, "not installed" if sp is None else "%.1f ms per step" % sp),
             "best step (a) %d  (b) %d;  costs bit-equal: %s;  patches bit-equal: %s" % (
                 results[na][0], results[nb][0], bool(np.array_equal(results[na][1], results[nb][1])),
                 bool(torch.equal(results[na][2], results[nb][2]))),
             "%-22s %30s %16s %14s %18s %14s" % ("form", "wall ms  median (min..max)", "device-span ms", "ms per step",
                                                 "loop enqueue ms", "launches/step")]
    for name, _ in forms:
        w, d, q = [t[0] for t in times[name]], [t[1] for t in times[name]], [t[2] for t in times[name]]
        lines.append("%-22s %10.1f (%8.1f ..%8.1f) %16.1f %14.4f %18.1f %14.1f" % (
            name, statistics.median(w), min(w), max(w), statistics.median(d), statistics.median(w) / n, statistics.median(q),
            per_step[name]))
    wa, qa = statistics.median([t[0] for t in times[na]]), statistics.median([t[2] for t in times[na]])
    lines.append("(a): the host spent %.1f %% of the wall time enqueuing the step loop; the draws, window plans, tables and K26 before it "
                 "and the wait after it are the rest" % (100.0 * qa / wa))
    lines.append("(a) / (b) wall time: %.3f" % (wa / statistics.median([t[0] for t in times[nb]])))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
