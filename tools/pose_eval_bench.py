"""What the odometry evaluation costs above the image files, on the device chain and on the reference's shape (writes
profiles/pose_eval.txt).

    python tools/pose_eval_bench.py [--frames 1591] [--reps 3] [--out profiles/pose_eval.txt]

A synthetic sequence of ``--frames`` frames at 192 x 640 (sequence 09 has 1591), handed to ``evaluate_pose.evaluate`` through its
``frames`` / ``gt_global_poses`` keywords, so that no file is decoded: what is timed is the pose encoder with K41 as its first
layer, K29, and K40 with one copy at the end (the device chain), against ``host_chain=True`` -- ``forward(torch.cat(...))``, a
``.cpu()`` per batch and the numpy loop -- on the same random-initialised weights.  Host clock around the whole call after a
warm-up call, best of ``--reps``.  Also: K41 and the library's normalise + convolution on one [16, 3, 192, 640] pair batch by HIP
events, and the largest error of either per unit of |w| (*) |xn| against a float64 convolution (tests/test_gpu_pose_eval.py).
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from depthmodelhardening_amd import evaluate_pose as EP, networks, ops      # noqa: E402
from depthmodelhardening_amd.options import MonodepthOptions              # noqa: E402

H, W, BATCH = 192, 640, 16


def drive(n_frames, seed=0):
    """gt_global [n_frames, 3, 4]: about one unit forward per frame with a slow random yaw."""
    rng = np.random.RandomState(seed)
    G, out = np.eye(4), []
    for _ in range(n_frames):
        out.append(G[:3].copy())
        yaw = rng.normal() * 0.01
        M = np.eye(4)
        M[0, 0], M[0, 2], M[2, 0], M[2, 2] = np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)
        M[:3, 3] = [rng.normal() * 0.02, rng.normal() * 0.01, 1.0 + rng.normal() * 0.1]
        G = G @ M
    return np.stack(out)


def blocks(pool, n_frames):
    """Blocks of BATCH pairs from a pool of random frames; the last frame of a block is the first of the next."""
    first = 0
    while first < n_frames - 1:
        n = min(BATCH, n_frames - 1 - first)
        idx = torch.arange(first, first + n + 1, device=pool.device) % pool.shape[0]
        yield pool[idx]
        first += n


def gpu_ms(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1591)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pose_eval.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    pool = torch.rand(64, 3, H, W, device=dev)
    gt = drive(a.frames)
    lines = []
    with tempfile.TemporaryDirectory() as folder:
        enc = networks.ResnetEncoder(18, False, 2)
        torch.save(enc.state_dict(), os.path.join(folder, "pose_encoder.pth"))
        torch.save(networks.PoseDecoder(enc.num_ch_enc, 1, 2).state_dict(), os.path.join(folder, "pose.pth"))
        opt = MonodepthOptions().parse(["--eval_split", "odom_9", "--load_weights_folder", folder, "--height", str(H), "--width", str(W),
                                        "--batch_size", str(BATCH)])
        times, res = {}, {}
        for host in (False, True):
            best = None
            for rep in range(a.reps + 1):       # the first call warms up (kernel selection, allocator)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    res[host] = EP.evaluate(opt, frames=blocks(pool, a.frames), gt_global_poses=gt, host_chain=host)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep > 0:
                    best = dt if best is None else min(best, dt)
            times[host] = best
        rel = np.abs(res[False]["ates"] - res[True]["ates"]) / np.abs(res[True]["ates"])
        lines.append("1. evaluate on %d synthetic frames of %d x %d (%d pairs, batches of %d, random-weight ResNet-18 pose networks, no file "
                     "decoded), host clock, best of %d after a warm-up call: device chain (K41 stem, K29, K40, one copy) %.1f ms; "
                     "host_chain=True (cat + normalise + library convolution, a copy per batch, numpy loop) %.1f ms; ratio %.2f x.  "
                     "Trajectory error %.4f / %.4f, std %.4f / %.4f; largest relative difference of a snippet error %.2g."
                     % (a.frames, H, W, a.frames - 1, BATCH, a.reps, 1e3 * times[False], 1e3 * times[True], times[True] / times[False],
                        res[False]["ate_mean"], res[True]["ate_mean"], res[False]["ate_std"], res[True]["ate_std"], float(rel.max())))
    # the first layer alone
    f = pool[:BATCH + 1]
    w = ((torch.rand(64, 6, 7, 7, device=dev) - 0.5) * 0.2)
    with torch.no_grad():
        t_k41 = gpu_ms(lambda: ops.stem_pair_norm(f[:-1], f[1:], w))
        t_lib = gpu_ms(lambda: F.conv2d((torch.cat([f[:-1], f[1:]], 1) - 0.45) / 0.225, w, None, 2, 3))
        y, lib = ops.stem_pair_norm(f[:-1], f[1:], w), F.conv2d((torch.cat([f[:-1], f[1:]], 1) - 0.45) / 0.225, w, None, 2, 3)
    xn = (torch.cat([f[:-1], f[1:]], 1).cpu().double() - 0.45) / 0.225
    want = F.conv2d(xn, w.cpu().double(), None, 2, 3)
    mass = F.conv2d(xn.abs(), w.cpu().double().abs(), None, 2, 3)
    r_k41 = float(((y.cpu().double() - want).abs() / mass).max())
    r_lib = float(((lib.cpu().double() - want).abs() / mass).max())
    lines.append("2. the first layer on one batch of %d pairs of %d x %d, HIP events: K41 (two launches, no temporaries) %.3f ms; "
                 "torch.cat + (x - 0.45) / 0.225 + the library's convolution %.3f ms; ratio %.2f x.  Largest |error| / (|w| (*) |xn|) "
                 "against a float64 convolution: K41 %.3g, the library's path %.3g." % (BATCH, H, W, t_k41, t_lib, t_lib / t_k41, r_k41, r_lib))
    n = a.frames - 1
    pred = torch.from_numpy(res[False]["pred_poses"]).to(dev)
    local = torch.from_numpy(ops.gt_local_poses(gt)).to(dev)
    t_k40 = gpu_ms(lambda: ops.pose_ate(pred, local))
    t0 = time.perf_counter()
    ops.pose_ate_host(res[False]["pred_poses"], ops.gt_local_poses(gt)[:n])
    t_host = time.perf_counter() - t0
    lines.append("3. the trajectory arithmetic on %d poses: K40 (two launches) %.3f ms by HIP events; the numpy loop %.1f ms by the host clock."
                 % (n, t_k40, 1e3 * t_host))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("tools/pose_eval_bench.py on one MI355X, one run.\n" + text)


if __name__ == "__main__":
    main()
