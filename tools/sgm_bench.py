"""What the device stereo matcher costs (writes profiles/sgm_stereo.txt).

    python tools/sgm_bench.py [--height 320] [--width 1024] [--batch 8] [--reps 5] [--workspace_cap BYTES] [--out FILE]

K35 (``ops.sgm_disparity``) with the twelve parameter sets of the reference on ``batch`` synthetic stereo pairs (tests/sgm_ref.py
``make_pair``), by HIP events after warm-up.  The phases are attributed by running the prefixes cost, cost + paths, cost + paths +
select and the whole call (``phases=``) and taking differences; the bytes of a phase are counted from its loads and stores of the
workspace and the output.  For scale: the host twin (``ops.sgm_disparity_host``) on one pair, wall clock; and the precompute tool
end to end with ``--matcher device`` on a synthetic tree of ``batch`` PNG pairs, wall clock (decode, resize, matchers, fusion and the
``.npy`` files), after one run that warmed the library up.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from depthmodelhardening_amd import _native as N, ops, precompute_depth_hints as P     # noqa: E402
from tests import sgm_ref as R                                                          # noqa: E402


def gpu_ms(fn, reps):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workspace_cap", type=int, default=ops.SGM_WORKSPACE_CAP)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sgm_stereo.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    H, W, B = a.height, a.width, a.batch
    params = P.stereo_matcher_params()
    pairs = [R.make_pair(H, W, 64, 80 + i) for i in range(B)]
    rev = [i % 2 == 1 for i in range(B)]
    pairs = [(p[0][:, :, ::-1], p[1][:, :, ::-1]) if r else p[:2] for p, r in zip(pairs, rev)]
    base = torch.from_numpy(np.ascontiguousarray(np.stack([p[0] for p in pairs])))
    lookup = torch.from_numpy(np.ascontiguousarray(np.stack([p[1] for p in pairs])))
    b_d, l_d = base.to(dev), lookup.to(dev)
    flags = torch.tensor([int(v) for v in rev], dtype=torch.int32, device=dev)
    nbytes, chunks = ops.sgm_plan(B, H, W, params, a.workspace_cap)

    def run(phases):
        return ops.sgm_disparity(b_d, l_d, params, reverse=flags, workspace_cap=a.workspace_cap, phases=phases)

    out = run(N.SGM_ALL)
    valid = float((out >= 0).float().mean())
    prefixes = [N.SGM_COST, N.SGM_COST | N.SGM_PATHS, N.SGM_COST | N.SGM_PATHS | N.SGM_SELECT, N.SGM_ALL]
    times = [gpu_ms(lambda ph=ph: run(ph), a.reps) for ph in prefixes]
    phase_ms = [times[0]] + [times[i] - times[i - 1] for i in range(1, 4)]
    # elements of the distinct jobs: blockSize 2 and 3 share a radius
    vol = B * 2 * sum(H * max(W - D, 0) * D for D in P.NUM_DISPARITIES)
    maps = B * 2 * len(P.NUM_DISPARITIES)
    moved = [2 * vol + maps * 6 * H * W,                         # C stored; both views read
             vol * (5 * 2 + 2 + 4 * 4),                          # C read five times; S stored once, then loaded and stored four times
             2 * vol + B * len(params) * H * W * 2,              # S read; every output slot stored
             maps * H * W * (2 + 8 + 2 * 2 + 8 + 4 + 4) + B * len(params) * H * W * 2]   # map reads, labels and sizes, the masked store
    t0 = time.perf_counter()
    ops.sgm_disparity_host(base[:1], lookup[:1], params, rev[:1])
    t_host = time.perf_counter() - t0
    with tempfile.TemporaryDirectory() as tmp:
        lines = R.write_tree(os.path.join(tmp, "tree"), (H, W), 80, "lr" * (B // 2) + "l" * (B % 2))
        with open(os.path.join(tmp, "list.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        argv = ["--data_path", os.path.join(tmp, "tree"), "--filenames", os.path.join(tmp, "list.txt"), "--height", str(H), "--width", str(W),
                "--batch_size", str(B), "--matcher", "device", "--overwrite_saved_depths"]
        P.main(argv + ["--save_path", os.path.join(tmp, "warm")])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P.main(argv + ["--save_path", os.path.join(tmp, "hints")])
        t_tool = time.perf_counter() - t0
    names = ("cost", "paths", "select", "speckle")
    lines = ["tools/sgm_bench.py: %d stereo pairs of %d x %d, the reference's 12 parameter sets (8 distinct), device time by HIP events"
             % (B, H, W),
             "0. workspace %.0f MB under a cap of %.0f MB: %d sequences of launches; %.1f %% of the output is valid"
             % (nbytes / 1e6, a.workspace_cap / 1e6, chunks, 100 * valid),
             "1. K35 ops.sgm_disparity, the whole call: %.2f ms (%.2f ms / pair)" % (times[3], times[3] / B)]
    for i in range(4):
        lines.append("   %-8s %8.2f ms   %8.1f MB   %6.0f GB/s" % (names[i], phase_ms[i], moved[i] / 1e6, moved[i] / max(phase_ms[i], 1e-6) / 1e6))
    lines += ["2. the host twin (numpy) on one pair, wall clock: %.1f s" % t_host,
              "3. precompute_depth_hints --matcher device on a synthetic tree of %d PNG pairs, wall clock, second run: %.2f s (%.3f s / pair)"
              % (B, t_tool, t_tool / B)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
