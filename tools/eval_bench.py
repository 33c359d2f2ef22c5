"""K25 against the numpy loop: the benign evaluation of 697 synthetic ground-truth maps at KITTI sizes.

    python tools/eval_bench.py [--images 697] [--repeats 5] [--post-process] [--out profiles/eigen_eval.txt]

Device: ops.eigen_depth_errors over batches of 16 predictions at 192 x 640, HIP events around the whole chain (the ground truth
is packed before, once per test set; its time is reported on its own).  Host: the float32 loop of tests/eigen_eval_ref.py
(resize, mask, two medians, eight reductions per image) on the same machine, wall clock.  Report only: nothing is asserted
beyond the two agreeing."""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from depthmodelhardening_amd import ops  # noqa: E402
from depthmodelhardening_amd.datasets import SyntheticEvalSet  # noqa: E402
from tests import eigen_eval_ref as R  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    n, repeats, out = arg("--images", 697), arg("--repeats", 5), arg("--out", "")
    pp = "--post-process" in sys.argv
    h, w, batch = 192, 640, 16
    dev = torch.device("cuda")
    data = SyntheticEvalSet(n, 8, 8, dev, seed=3)        # the frames are not used: the predictions below stand in for a model
    rng = np.random.RandomState(5)
    disp = np.concatenate([R.smooth_disp(rng, min(batch, n - i), h, w) for i in range(0, n, batch)])
    flip = disp[:, :, ::-1].copy() if pp else None
    d_dev = torch.from_numpy(disp).to(dev)
    f_dev = torch.from_numpy(flip).to(dev) if pp else None
    t0 = time.perf_counter()
    pack = ops.eigen_gt_pack(data.gt_depths, "eigen", dev)
    torch.cuda.synchronize()
    t_pack = time.perf_counter() - t0

    def chain():
        rows = []
        for i in range(0, n, batch):
            e, r = ops.eigen_depth_errors(d_dev[i:i + batch], pack, i, pred_disp_flip=None if f_dev is None else f_dev[i:i + batch])
            rows.append(torch.cat([e, r[:, None]], 1))
        return torch.cat(rows)
    chain()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        table = chain()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    got = table.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    taps = R.post_process_taps(disp, flip).astype(np.float32) if pp else disp
    errors, ratios = R.evaluate_loop(taps, data.gt_depths, "eigen", dtype=np.float32)
    t_host = time.perf_counter() - t0
    px = int(pack.offsets[-1])
    valid = int(pack.counts.sum())
    lines = ["K25 benign evaluation: %d maps, %d packed pixels (%.1f %% valid), predictions %d x %d, batches of %d%s" % (
                 n, px, 100.0 * valid / px, h, w, batch, ", post-processed" if pp else ""),
             "device chain (HIP events, %d repeats): median %.3f ms, min %.3f, max %.3f" % (
                 repeats, float(np.median(times)), min(times), max(times)),
             "numpy loop on this host (float32, wall): %.1f ms" % (1e3 * t_host),
             "packing the ground truth (upload + counts + medians, once per test set, wall): %.1f ms" % (1e3 * t_pack),
             "bytes per pass over the packed pixels: depth 8 B/px = %.1f MB, histogram passes 1 and 2 4 B/px = %.1f MB each, "
             "metrics 8 B/px = %.1f MB; total %.1f MB per evaluation" % (8e-6 * px, 4e-6 * px, 8e-6 * px, 24e-6 * px),
             "mean errors device %s" % np.array2string(np.nanmean(got[:, :8], 0), precision=5),
             "mean errors numpy  %s" % np.array2string(np.nanmean(errors, 0), precision=5),
             "largest relative difference of a per-image ratio: %.3g" % np.nanmax(np.abs(got[:, 8] / ratios - 1))]
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
