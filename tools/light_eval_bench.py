"""Wall and device time of the tube-light object attack (200 x 20 x 2 = 8000 queries by default) on 12 scenes with the ResNet-18
U-Net, two ways:

    (a) Phy_obj_atk_light                      K24 compose / commit, every draw made up front, no host read per query
    (b) Phy_obj_atk_light(host_chain=True)     the reference's loop shape on the same paste / cost kernels: the pattern in numpy on
                                               the host, an upload and a host comparison per query

    python tools/light_eval_bench.py [--attacks 7] [--n-init 200] [--n-search 20] [--out profiles/light_eval.txt]

(b) stands for the reference's loop with its Python pixel loop already replaced by numpy: it flatters the baseline.  The two forms
alternate inside one process after a warm-up (a short attack of each); the report is the median and the spread of ``--attacks``
attacks each: wall time from perf_counter around the whole call with a synchronisation at its end, device time from HIP events
around the same region, and for (a) the part of the wall time the host spent enqueuing the query loop -- when it is close to the
whole, the device waited for the host; the rest is how far the host ran ahead.  Kernel launches per query are counted with the
profiler on a separate short attack of each form.
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
from depthmodelhardening_amd.torchattacks import Phy_obj_atk_light           # noqa: E402


def seed_all(seed):
    import random
    random.seed(seed)
    np.random.seed(seed)


def launches_per_query(make, scenes, B, queries=(2, 2)):
    """Kernel launches of a whole short attack divided by its queries, minus nothing: set-up and the two final pastes are in."""
    from torch.profiler import ProfilerActivity, profile
    atk = make(*queries)
    seed_all(1)
    atk(scenes, B)          # warm
    torch.cuda.synchronize()
    counts = []
    for q in (queries, (queries[0] * 3, queries[1])):
        atk = make(*q)
        seed_all(1)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            atk(scenes, B)
            torch.cuda.synchronize()
        counts.append((q[0] * q[1] * 2, sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                                             and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())))
    (n0, k0), (n1, k1) = counts
    return (k1 - k0) / float(n1 - n0)       # the slope: what one more query launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attacks", type=int, default=7)
    ap.add_argument("--scenes", type=int, default=12)
    ap.add_argument("--n-init", type=int, default=200)
    ap.add_argument("--n-search", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = import_depth_model((1024, 320)).to(dev).eval()
    obj, mask = make_object(dev)
    B = args.scenes
    scenes = torch.rand(B, 3, 375, 1242, generator=torch.Generator().manual_seed(3)).to(dev)
    n = args.n_init * args.n_search * 2
    enqueue = []

    @contextlib.contextmanager
    def stamp():
        t = time.perf_counter()
        yield
        enqueue.append(time.perf_counter() - t)

    def make(host, n_init=args.n_init, n_search=args.n_search):
        atk = Phy_obj_atk_light(model, obj, mask, dist_range=list(np.arange(5, 10, 0.2)), n_init=n_init, n_search=n_search,
                                host_chain=host)
        atk.loop_context = stamp
        return atk
    forms = [("a: K24, device loop", False), ("b: host chain", True)]
    per_query = {name: launches_per_query(lambda i, s, h=host: make(h, i, s), scenes, B) for name, host in forms}
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
    lines = ["Tube-light object attack: %d x %d x 2 = %d queries, %d scenes, ResNet-18 U-Net 320x1024, %d attacks per form, alternating"
             % (args.n_init, args.n_search, n, B, args.attacks),
             "best query (a) %d  (b) %d;  costs bit-equal: %s;  patches bit-equal: %s" % (
                 results[na][0], results[nb][0], bool(np.array_equal(results[na][1], results[nb][1])),
                 bool(torch.equal(results[na][2], results[nb][2]))),
             "%-22s %30s %16s %14s %18s %14s" % ("form", "wall ms  median (min..max)", "device-span ms", "ms per query",
                                                 "loop enqueue ms", "launches/query")]
    for name, _ in forms:
        w, d, q = [t[0] for t in times[name]], [t[1] for t in times[name]], [t[2] for t in times[name]]
        lines.append("%-22s %10.1f (%8.1f ..%8.1f) %16.1f %14.4f %18.1f %14.1f" % (
            name, statistics.median(w), min(w), max(w), statistics.median(d), statistics.median(w) / n, statistics.median(q),
            per_query[name]))
    wa, qa = statistics.median([t[0] for t in times[na]]), statistics.median([t[2] for t in times[na]])
    lines.append("(a): the host spent %.1f %% of the wall time enqueuing the query loop; the draws, window plans and tables before it "
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
