"""What tools/make_goldens_hints.py and the depth-hint tests (K34) must agree on: the seeded stereo pairs and candidate disparities,
the camera of depth-hints/precompute_depth_hints.py:107-123, the layout of the tiny hint tree tests/golden/kitti_hints, and the
regret criterion.  ``reference`` runs the package's host twins only; nothing here needs a GPU.

The input recipe.  Lookup image: 4 x 4 blocky random bytes blended with per-pixel noise.  Base image: the lookup shifted by a
smooth disparity field of 2 .. ~60 px (towards the side the other camera sees it).  Candidate n: the true disparity + Gaussian
noise of sigma 0.3 (n % 4) + 10 % outliers, rounded to 1/16 and stored as StereoSGBM does (int16, disparity x 16); then 15 % of
the pixels are -16 (no match), values >= 16 [64, 96, 128, 160][n % 4] are -16 (beyond the matcher's numDisparities), and columns
0 .. 4 are all -16.
"""
import functools
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HINT_TREE = os.path.join(REPO, "tests", "golden", "kitti_hints")
NUM_DISPARITIES = (64, 96, 128, 160)
GOLDEN_CASE = dict(H=24, W=80, N=12, side="l", seed=34)          # tests/golden/depth_hint_fuse.npz
TREE_HINT_SIZE = (16, 48)       # every file of the hint tree: half of kitti_ref.TRAIN_SIZE, so that the loader at 32 x 96 resizes


def camera(H, W, side):
    """K, inv_K, T float32 [1, 4, 4] as DepthHintDataset builds them (pinv in float32; T[0, 3] = -0.1 left, +0.1 right)."""
    K = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    K[0] *= W
    K[1] *= H
    inv_K = np.linalg.pinv(K)
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = -0.1 if side == "l" else 0.1
    return tuple(torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).unsqueeze(0) for m in (K, inv_K, T))


def make_case(H, W, N=12, side="l", seed=0, all_invalid=False):
    """One stereo pair: dict(base, lookup uint8 [1, 3, H, W], cand int16 [1, N, H, W], K, inv_K, T float32 [1, 4, 4])."""
    rng = np.random.RandomState(seed)
    blocks = rng.randint(0, 256, size=(3, (H + 3) // 4, (W + 3) // 4)).astype(np.float64)
    blocky = np.kron(blocks, np.ones((4, 4)))[:, :H, :W]
    noise = rng.randint(0, 256, size=(3, H, W)).astype(np.float64)
    lookup = np.clip(np.rint(0.7 * blocky + 0.3 * noise), 0, 255).astype(np.uint8)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    truth = 2.0 + 58.0 * (0.5 + 0.5 * np.sin(2.0 * np.pi * xx / max(W, 1) + 0.7) * np.cos(np.pi * yy / max(H, 1)))
    sign = -1.0 if side == "l" else 1.0            # a left base pixel x shows what the right view has at x - d
    sx = np.clip(np.rint(xx + sign * truth), 0, W - 1).astype(np.int64)
    base = np.take_along_axis(lookup, np.broadcast_to(sx, (3, H, W)), axis=2)
    cand = np.empty((N, H, W), dtype=np.int16)
    for n in range(N):
        d = truth + rng.normal(0.0, 1.0, size=(H, W)) * (0.3 * (n % 4))
        outlier = rng.uniform(size=(H, W)) < 0.10
        d = np.where(outlier, rng.uniform(0.0, 170.0, size=(H, W)), d)
        raw = np.rint(d * 16.0)
        raw[rng.uniform(size=(H, W)) < 0.15] = -16
        raw[raw >= 16 * NUM_DISPARITIES[n % 4]] = -16
        raw[raw < 0] = -16
        raw[:, :5] = -16
        cand[n] = raw.astype(np.int16)
    if all_invalid:
        cand[:] = -16
    K, inv_K, T = camera(H, W, side)
    return dict(base=torch.from_numpy(np.ascontiguousarray(base)).unsqueeze(0), lookup=torch.from_numpy(lookup).unsqueeze(0),
                cand=torch.from_numpy(cand).unsqueeze(0), K=K, inv_K=inv_K, T=T)


def cat_cases(cases):
    return {k: torch.cat([c[k] for c in cases], 0) for k in cases[0]}


ARGS = ("base", "lookup", "cand", "K", "inv_K", "T")


@functools.lru_cache(maxsize=None)
def reference(H, W, N=12, side="l", seed=0):
    """The case with its float32 reference (the host twin: the reference's torch expressions) and its float64 anchor, computed
    once per process: dict(case, depths, loss32, best32, loss64, dev = max |loss32 - loss64|).  Shared; do not modify."""
    from depthmodelhardening_amd import ops
    case = make_case(H, W, N, side, seed)
    args = [case[k] for k in ARGS]
    best32, loss32 = ops.depth_hint_fuse_host(*args, want_losses=True)
    _, loss64 = ops.depth_hint_fuse_host(*args, want_losses=True, dtype=torch.float64)
    dev = float((loss32.double() - loss64).abs().max())
    return dict(case=case, depths=ops.hint_candidate_depths(case["cand"], case["K"]), loss32=loss32, best32=best32, loss64=loss64, dev=dev)


def regret(loss64, index):
    """The float64 loss of the picked candidate minus the float64 minimum, per pixel: [B, H, W]."""
    picked = torch.gather(loss64, 1, index.unsqueeze(1))[:, 0]
    return picked - loss64.min(dim=1).values


def hint_path(folder, side, frame):
    return os.path.join(HINT_TREE, folder, "image_0%d" % (2 if side == "l" else 3), "%010d.npy" % frame)


def tree_hint(folder, side, frame, hw):
    """The made-up hint of a frame of tests/golden/kitti_tree: float32 [1, h, w], seeded by its name; about a quarter of the pixels
    are 0 (no hint), a few are -0.0."""
    import hashlib
    seed = int(hashlib.sha256(("hint/%s/%s/%d" % (folder, side, frame)).encode()).hexdigest()[:8], 16)
    rng = np.random.RandomState(seed)
    a = rng.uniform(1.0, 80.0, size=(1,) + tuple(hw)).astype(np.float32)
    a[rng.uniform(size=a.shape) < 0.25] = 0.0
    a[rng.uniform(size=a.shape) < 0.02] = -0.0
    return a
