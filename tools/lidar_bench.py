"""What turning depth into pseudo-LiDAR clouds costs on the device and on the host (writes profiles/pseudo_lidar.txt).

    python tools/lidar_bench.py [--frames 16] [--reps 500] [--images 32] [--threads 16] [--out FILE]

1. K39 (``ops.pseudo_lidar``): ``--frames`` frames of 375 x 1242 in each of the three forms (the net form from 320 x 1024, plain and
   quantised), one call, by device time: HIP events around 20 replays of a HIP graph that holds 50 calls (no host work between
   the launches), and around ``--reps`` eager calls after a warm-up.  Every call reads the same maps.
2. The host chain it replaces -- the numpy restatement of the reference's ``project_depth_to_points`` /
   ``project_disp_to_points`` over ``Calibration.project_image_to_velo`` (meshgrid, [3, N] stack, two ``np.dot``, boolean gather,
   the ones column and the float32 cast), one frame per task on a pool of ``--threads`` threads, by the host clock.  The copy of
   the maps to the host, which that chain also needs, is not counted.
3. ``python -m depthmodelhardening_amd.generate_lidar --image_dir`` on a folder of ``--images`` synthetic 375 x 1242 PNGs with a
   random-weight network fed 320 x 1024, end to end by the host clock (decode, K31, network, K39, the copies and the .bin
   writes), after one warm-up pass.

Needs a GPU.  The maps and images are seeded; nothing is read from outside the tree.
"""
import argparse
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from depthmodelhardening_amd import generate_lidar as G        # noqa: E402
from depthmodelhardening_amd import ops                         # noqa: E402
from depthmodelhardening_amd.datasets.kitti_object import Calibration  # noqa: E402
from tests import lidar_ref as L                                # noqa: E402

FEED, FULL = (320, 1024), (375, 1242)


def gpu_ms(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def graph_ms(fn, calls=50, replays=20):
    """Device time of one call: ``calls`` of them captured into one HIP graph, replayed back to back (no host work between launches)."""
    fn()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            fn()
    graph.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (calls * replays)


def reference_chain(calib, m, max_high, is_disp):
    """generate_lidar.py:10-33 and :75-76 with kitti_util.py:159-175, 113-130 restated in numpy as the reference writes them."""
    if is_disp:
        m = m.astype(np.float64)
        m[m < 0] = 0
        mask = m > 0
        depth = calib.f_u * 0.54 / (m + 1. - mask)
    else:
        depth = m
    rows, cols = depth.shape
    c, r = np.meshgrid(np.arange(cols), np.arange(rows))
    points = np.stack([c, r, depth]).reshape((3, -1)).T
    if is_disp:
        points = points[mask.reshape(-1)]
    x = ((points[:, 0] - calib.c_u) * points[:, 2]) / calib.f_u + calib.b_x
    y = ((points[:, 1] - calib.c_v) * points[:, 2]) / calib.f_v + calib.b_y
    rect = np.zeros((points.shape[0], 3))
    rect[:, 0], rect[:, 1], rect[:, 2] = x, y, points[:, 2]
    ref = np.transpose(np.dot(np.linalg.inv(calib.R0), np.transpose(rect)))
    cloud = np.dot(np.hstack((ref, np.ones((ref.shape[0], 1)))), np.transpose(calib.C2V))
    cloud = cloud[(cloud[:, 0] >= 0) & (cloud[:, 2] < max_high)]
    return np.concatenate([cloud, np.ones((cloud.shape[0], 1))], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pseudo_lidar.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/lidar_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda")
    n, px = a.frames, FULL[0] * FULL[1]
    text = L.calib_text("rotated", FULL)
    calib = Calibration(text)
    cal = torch.from_numpy(np.repeat(calib.packed()[None], n, 0)).to(dev)
    depth = [L.depth_map("bench/depth/%d" % i, FULL) for i in range(n)]
    disp = [L.disp_map("bench/disp/%d" % i, FULL) for i in range(n)]
    net = np.stack([L.net_map("bench/net/%d" % i, FEED) for i in range(n)])
    src = {"depth": torch.from_numpy(np.concatenate([m.reshape(-1) for m in depth])).to(dev),
           "disp": torch.from_numpy(np.concatenate([m.reshape(-1) for m in disp])).to(dev), "net": torch.from_numpy(net).to(dev)}
    lines = ["tools/lidar_bench.py: %d frames of %d x %d, max_high 1" % ((n,) + FULL)]
    with ThreadPoolExecutor(max_workers=a.threads) as pool:
        for form, quantise in (("depth", False), ("disp", False), ("net", False), ("net", True)):
            out = ops.pseudo_lidar(src[form], form, [FULL] * n, cal, 1, quantise)
            kept = int(out.offsets[-1])
            t_e = gpu_ms(lambda: ops.pseudo_lidar(src[form], form, [FULL] * n, cal, 1, quantise), a.reps)
            t_k = graph_ms(lambda: ops.pseudo_lidar(src[form], form, [FULL] * n, cal, 1, quantise))
            moved = 4 * src[form].numel() * 2 + 16 * kept                     # the source is read by both passes; the rows
            line = ("1. K39 %-5s%s one call (3 launches): %.3f ms device time replayed from a HIP graph (%.4f ms / frame), %.3f ms per eager "
                    "call; %d of %d pixels kept; %.0f GB/s of %.1f MB (the same maps every call: reads may come from cache)") % (
                form, " quantised," if quantise else ",", t_k, t_k / n, t_e, kept, n * px, moved / t_k / 1e6, moved / 1e6)
            if form != "net":
                maps = depth if form == "depth" else disp
                first = reference_chain(calib, maps[0], 1, form == "disp")
                mine = out.points[:int(out.offsets[1])].cpu().numpy()
                same = first.shape == mine.shape and np.array_equal(first.view(np.uint32), mine.view(np.uint32))
                list(pool.map(lambda m: reference_chain(calib, m, 1, form == "disp"), maps))
                t0 = time.perf_counter()
                for _ in range(2):
                    list(pool.map(lambda m: reference_chain(calib, m, 1, form == "disp"), maps))
                t_h = (time.perf_counter() - t0) / 2 * 1e3
                line += "\n2. the reference's numpy chain, %s form, on %d threads: %.1f ms wall (%.1f ms / frame); ratio %.0f x; frame 0 bit-equal to K39: %s" % (
                    form, a.threads, t_h, t_h / n, t_h / t_k, same)
            lines.append(line)

    from PIL import Image
    from oracle import synth
    model = synth.TinyDepthNet(seed=11).to(dev).eval()
    rng = np.random.RandomState(39)
    with tempfile.TemporaryDirectory() as folder:
        images, calibs, save = (os.path.join(folder, d) for d in ("image_2", "calib", "velodyne"))
        os.makedirs(images)
        os.makedirs(calibs)
        for i in range(a.images):
            Image.fromarray(rng.randint(0, 256, FULL + (3,), dtype=np.uint8)).save(os.path.join(images, "%06d.png" % i))
            with open(os.path.join(calibs, "%06d.txt" % i), "w") as f:
                f.write(text)
        args = G.parse_args(["--calib_dir", calibs, "--image_dir", images, "--save_dir", save, "--batch_size", str(n)])
        args.feed_height, args.feed_width = FEED
        with open(os.devnull, "w") as null:
            stdout, sys.stdout = sys.stdout, null
            try:
                with torch.backends.cudnn.flags(enabled=False):
                    G.main(args, model=model)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    written = G.main(args, model=model)
                    torch.cuda.synchronize()
                    t_s = time.perf_counter() - t0
            finally:
                sys.stdout = stdout
        size = sum(os.path.getsize(p) for p in written)
    lines += ["3. generate_lidar --image_dir on %d synthetic %d x %d PNGs, random-weight 3-layer network fed %d x %d, batches of %d, end to end: "
              "%.2f s wall (%.1f ms / image), %.1f MB of .bin written" % ((a.images,) + FULL + FEED + (n, t_s, 1e3 * t_s / a.images, size / 1e6)),
              "   (PNG decode of incompressible noise, the copy of the kept rows and the file writes are host work; the network here is a stand-in)"]
    out_text = "\n".join(lines) + "\n"
    print(out_text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out_text)


if __name__ == "__main__":
    main()
