"""What colouring disparity maps costs on the device and on the host (writes profiles/disp_colorize.txt).

    python tools/colorize_bench.py [--maps 16] [--reps 20] [--images 64] [--threads 16] [--out FILE]

1. K37 (``ops.disp_colorize``): ``--maps`` disparities of 192 x 640 resized to 375 x 1242, minimum, 95th percentile and magma
   bytes, one call, by device time (HIP events around ``--reps`` calls after a warm-up).
2. The host chain it replaces (MD2/test_simple.py:136-155), per map: F.interpolate on the device, the copy to the host,
   ``np.percentile``, matplotlib's ``Normalize`` + ``ScalarMappable``, ``* 255``, ``astype(uint8)`` -- on a pool of ``--threads``
   threads, by the host clock around work that ends with every result in hand.  Needs matplotlib (the package does not).
3. ``python -m depthmodelhardening_amd.test_simple`` on a folder of ``--images`` synthetic 375 x 1242 PNGs with a random-weight
   network fed 192 x 640, end to end by the host clock (decode, K31, network, K37, JPEG and .npy writes), after one warm-up pass.

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
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from depthmodelhardening_amd import ops                         # noqa: E402
from depthmodelhardening_amd import test_simple as TS           # noqa: E402

FEED, FULL = (192, 640), (375, 1242)


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


def host_chain(disp, pool):
    """test_simple.py:136-155 for every map of ``disp`` [n, h, w] on the device; returns the byte images."""
    import matplotlib as mpl
    import matplotlib.cm as cm

    def one(i):
        a = F.interpolate(disp[i][None, None], FULL, mode="bilinear", align_corners=False).squeeze().cpu().numpy()
        vmax = np.percentile(a, 95)
        mapper = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=a.min(), vmax=vmax), cmap='magma')
        return (mapper.to_rgba(a)[:, :, :3] * 255).astype(np.uint8)
    return list(pool.map(one, range(disp.shape[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "disp_colorize.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/colorize_bench.py measures on the GPU; there is none")
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(37)
    # smooth maps in (0, 1), as a disparity is: a coarse field upsampled
    disp = torch.sigmoid(4 * F.interpolate(torch.randn(a.maps, 1, 12, 40, generator=g), FEED, mode="bicubic", align_corners=False))
    disp = disp[:, 0].contiguous().to(dev)

    got = ops.disp_colorize(disp, out_size=FULL, return_map=True)
    want = ops.disp_colorize_host(got.map.cpu())
    differs = int((got.rgb.cpu() != want.rgb).sum())
    t_k = gpu_ms(lambda: ops.disp_colorize(disp, out_size=FULL), a.reps)
    n_out = a.maps * FULL[0] * FULL[1]
    moved = 4 * a.maps * FEED[0] * FEED[1] + n_out * (4 + 3 * 4 + 3)      # read src; map written once and read three times; bytes

    with ThreadPoolExecutor(max_workers=a.threads) as pool:
        host_chain(disp, pool)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            ref = host_chain(disp, pool)
        t_h = (time.perf_counter() - t0) / 3 * 1e3
    against = int(sum((r != w.numpy()).sum() for r, w in zip(ref, got.rgb.cpu())))

    from PIL import Image
    from oracle import synth
    model = synth.TinyDepthNet(seed=11).to(dev).eval()
    rng = np.random.RandomState(37)
    with tempfile.TemporaryDirectory() as folder:
        for i in range(a.images):
            Image.fromarray(rng.randint(0, 256, FULL + (3,), dtype=np.uint8)).save(os.path.join(folder, "%04d.png" % i))
        args = argparse.Namespace(image_path=folder, ext="png", pred_metric_depth=False, no_cuda=False, model_name=None,
                                  load_weights_folder=None, feed_height=FEED[0], feed_width=FEED[1])
        with open(os.devnull, "w") as null:
            stdout, sys.stdout = sys.stdout, null
            try:
                with torch.backends.cudnn.flags(enabled=False):
                    TS.test_simple(args, model=model)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    TS.test_simple(args, model=model)
                    torch.cuda.synchronize()
                    t_s = time.perf_counter() - t0
            finally:
                sys.stdout = stdout

    lines = ["tools/colorize_bench.py: %d disparities of %d x %d -> %d x %d" % ((a.maps,) + FEED + FULL),
             "0. bytes that differ from the numpy twin on the returned map: %d; from the host chain (its resize is torch's): %d of %d"
             % (differs, against, 3 * n_out),
             "1. K37 ops.disp_colorize, one call (memset + 7 launches): %.3f ms device time (%.3f ms / map); %.1f MB moved, %.0f GB/s of them"
             % (t_k, t_k / a.maps, moved / 1e6, moved / t_k / 1e6),
             "2. the host chain (resize on the device, D2H, np.percentile, matplotlib) on %d threads: %.1f ms wall (%.2f ms / map); ratio %.0f x"
             % (a.threads, t_h, t_h / a.maps, t_h / t_k),
             "3. test_simple on %d synthetic %d x %d PNGs, random-weight 3-layer network fed %d x %d, end to end: %.2f s wall (%.1f ms / image)"
             % ((a.images,) + FULL + FEED + (t_s, 1e3 * t_s / a.images)),
             "   (PNG decode of incompressible noise and the JPEG encode are host work on one thread each; the network here is a stand-in)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
