"""Writes tests/golden/depth_hint_fuse.npz and the data-only hint tree tests/golden/kitti_hints/ (tests/hint_ref.py has the input
recipe and the tree's layout).

    python tools/make_goldens_hints.py [--reference DIR]

The reference's own ``BackprojectDepth``, ``Project3D`` and ``SSIM`` (depth-hints/layers.py) and ``compute_reprojection_loss``
(depth-hints/precompute_depth_hints.py:66-77) run on hint_ref.GOLDEN_CASE, imported the way the sibling tools import the reference
(oracle/make_goldens.install_shims; ``cv2`` is a stub with ``setNumThreads`` -- the script imports it at the top and the matchers
are not run -- and ``six.moves.urllib`` when six is absent).  The lines :151 (disparity -> depth) and :247-252 (warp, loss, argmin,
gather) are the script's, on the CPU, in float32; the float64 losses are the same modules fed float64 tensors.

Stored: the inputs (base, lookup, cand, K, inv_K, T), ``depths`` (the reference's line :151), ``loss32`` [N, H, W], ``best_depth``
[1, H, W], ``loss64``, ``ref_dev`` = max |loss32 - loss64|, and ``twin_dev`` = max |twin float32 losses - loss32|, the observed
distance of ops.depth_hint_fuse_host from the reference (the same torch expressions: 0 is expected), which the CPU test holds it to.

A tool: not run by the tests.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as mg      # noqa: E402
from tests import hint_ref as R            # noqa: E402
from tests import kitti_ref as KR          # noqa: E402

ARGV = list(sys.argv)
OUT = os.path.join(REPO, "tests", "golden", "depth_hint_fuse.npz")


def install(ref_dir):
    import types
    mg.install_shims()
    sys.modules["cv2"].setNumThreads = lambda n: None
    try:
        import six  # noqa: F401
    except ImportError:
        import urllib
        moves = types.ModuleType("six.moves")
        moves.urllib = urllib
        six = types.ModuleType("six")
        six.moves = moves
        sys.modules["six"], sys.modules["six.moves"] = six, moves
    import PIL.Image as Image
    if not hasattr(Image, "ANTIALIAS"):
        Image.ANTIALIAS = Image.LANCZOS
    sys.path.insert(0, os.path.join(ref_dir, "DepthNetworks", "depth-hints"))


def reference_run(case, pre, dtype):
    """precompute_depth_hints.py:151 and :247-252 on one stereo pair."""
    import torch
    import torch.nn.functional as F
    n, H, W = case["cand"].shape[1:]
    disps = torch.from_numpy(case["cand"][0].numpy() / 16).float()
    K = case["K"].expand(n, -1, -1).float()
    depths = K[0, 0, 0] * 0.1 / (disps + 1e-7) * (disps > 0).float()          # :151 (self.baseline = 0.1)
    data = {"depths": depths.unsqueeze(1).to(dtype), "K": K.to(dtype), "invK": case["inv_K"].expand(n, -1, -1).to(dtype),
            "T": case["T"].to(dtype),
            "base_image": case["base"].to(dtype).expand(n, -1, -1, -1) / 255, "lookup_image": case["lookup"].to(dtype).expand(n, -1, -1, -1) / 255}
    cam_to_world = pre.BackprojectDepth(n, H, W).to(dtype)
    world_to_cam = pre.Project3D(n, H, W)
    world_points = cam_to_world(data["depths"], data["invK"])
    cam_pix = world_to_cam(world_points, data["K"], data["T"])
    sample = F.grid_sample(data["lookup_image"], cam_pix, padding_mode="border")
    losses = pre.compute_reprojection_loss(sample, data["base_image"])
    best_index = torch.argmin(losses, dim=0)
    best_depth = torch.gather(depths, dim=0, index=best_index)
    return depths, losses[:, 0], best_depth.reshape(1, H, W)


def write_hint_tree():
    for drive, _ in KR.DRIVES:
        for side in ("l", "r"):
            for frame in KR.FRAMES:
                path = R.hint_path(drive, side, frame)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                np.save(path, R.tree_hint(drive, side, frame, R.TREE_HINT_SIZE))


def main():
    import torch
    ref_dir = ARGV[ARGV.index("--reference") + 1] if "--reference" in ARGV else mg.REF
    install(ref_dir)
    import precompute_depth_hints as pre
    from depthmodelhardening_amd import ops
    case = R.make_case(**R.GOLDEN_CASE)
    depths, loss32, best = reference_run(case, pre, torch.float32)
    _, loss64, _ = reference_run(case, pre, torch.float64)
    twin_best, twin_loss = ops.depth_hint_fuse_host(*[case[k] for k in R.ARGS], want_losses=True)
    twin_dev = float((twin_loss[0].double() - loss32.double()).abs().max())
    ref_dev = float((loss32.double() - loss64).abs().max())
    print("ref_dev %.3e twin_dev %.3e depths equal %s best equal %s" % (
        ref_dev, twin_dev, torch.equal(ops.hint_candidate_depths(case["cand"], case["K"])[0], depths), torch.equal(twin_best[0], best)))
    np.savez_compressed(OUT, depths=depths.numpy(), loss32=loss32.numpy(), best_depth=best.numpy(), loss64=loss64.numpy(),
                        ref_dev=np.float64(ref_dev), twin_dev=np.float64(twin_dev), torch_version=np.array(torch.__version__),
                        **{k: case[k].numpy() for k in R.ARGS})
    print("wrote %s %.1f KiB" % (OUT, os.path.getsize(OUT) / 1024.0))
    write_hint_tree()


if __name__ == "__main__":
    main()
