"""What the fusion of depth-hint candidates costs on the device (writes profiles/depth_hint_fuse.txt).

    python tools/depth_hint_bench.py [--height 320] [--width 1024] [--candidates 12] [--batch 8] [--reps 10] [--out FILE]

K34 (``ops.depth_hint_fuse``, one launch for the batch, int16 candidates) against the torch-eager expression of the same lines of
depth-hints/precompute_depth_hints.py (:151, :247-252) on the device, one image after the other as the reference runs them, by
device time (HIP events).  Inputs are the seeded recipe of tests/hint_ref.py; nothing is read from the reference tree.  The two
are compared on item 0 first (the share of pixels whose depth differs is printed; exact ties and float32 rounding make it > 0).

This times the device half only.  With OpenCV the whole precompute stage is bound by the host matchers (twelve SGBM runs per
stereo pair), which neither form touches.  Needs a GPU.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from depthmodelhardening_amd import ops            # noqa: E402
from tests import hint_ref as R                    # noqa: E402


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


class Eager(object):
    """The reference's device half for one image: its modules' buffers are built once, as ``run`` builds them."""

    def __init__(self, n, H, W, dev):
        self.n, self.H, self.W = n, H, W
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
        self.ones = torch.ones(n, 1, H * W, device=dev)
        self.pix = torch.cat([torch.stack([xs.reshape(-1), ys.reshape(-1)], 0).unsqueeze(0).repeat(n, 1, 1), self.ones], 1)

    def __call__(self, base, lookup, raw, K, inv_K, T):
        n, H, W = self.n, self.H, self.W
        disps = raw.float() / 16
        depths = K[0, 0] * 0.1 / (disps + 1e-7) * (disps > 0).float()
        Kn, iKn = K.unsqueeze(0).expand(n, -1, -1), inv_K.unsqueeze(0).expand(n, -1, -1)
        cam = torch.matmul(iKn[:, :3, :3], self.pix)
        cam = torch.cat([depths.view(n, 1, -1) * cam, self.ones], 1)
        P = torch.matmul(Kn, T.unsqueeze(0))[:, :3, :]
        cp = torch.matmul(P, cam)
        pc = cp[:, :2, :] / (cp[:, 2, :].unsqueeze(1) + 1e-7)
        pc = pc.view(n, 2, H, W).permute(0, 2, 3, 1)
        pc[..., 0] /= W - 1
        pc[..., 1] /= H - 1
        pc = (pc - 0.5) * 2
        img_l = (lookup.float() / 255).unsqueeze(0).expand(n, -1, -1, -1)
        img_b = (base.float() / 255).unsqueeze(0).expand(n, -1, -1, -1)
        sample = F.grid_sample(img_l, pc, padding_mode="border", align_corners=False)
        loss = 0.85 * ops._hint_ssim(sample, img_b).mean(1, True) + 0.15 * torch.abs(img_b - sample).mean(1, True)
        return torch.gather(depths, 0, torch.argmin(loss, dim=0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--candidates", type=int, default=12)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_hint_fuse.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    H, W, n, B = a.height, a.width, a.candidates, a.batch
    case = R.cat_cases([R.make_case(H, W, n, "lr"[i % 2], 50 + i) for i in range(B)])
    args = [case[k].to(dev) for k in R.ARGS]
    eager = Eager(n, H, W, dev)

    def run_eager():
        return [eager(*[t[i] for t in args]) for i in range(B)]

    got, want = ops.depth_hint_fuse(*args), run_eager()
    differs = float((got[0] != want[0]).float().mean())
    t_k = gpu_ms(lambda: ops.depth_hint_fuse(*args), a.reps)
    t_e = gpu_ms(run_eager, max(2, a.reps // 2))
    moved = B * H * W * (6 + 2 * n + 4)
    lines = ["tools/depth_hint_bench.py: %d stereo pairs of %d x %d, %d candidates (int16), device time by HIP events" % (B, H, W, n),
             "0. item 0: the kernel's depth differs from the eager expression's at %.2f %% of the pixels (ties, float32 rounding)" % (100 * differs),
             "1. K34 ops.depth_hint_fuse, one launch for the batch: %.3f ms (%.3f ms / image); %.1f MB in and out, %.0f GB/s of them"
             % (t_k, t_k / B, moved / 1e6, moved / t_k / 1e6),
             "2. torch eager, the same lines, image by image: %.3f ms (%.3f ms / image); ratio %.1f x" % (t_e, t_e / B, t_e / t_k),
             "The device half only: with OpenCV the precompute stage is bound by the host matchers (12 SGBM runs per pair)."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
