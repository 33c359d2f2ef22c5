"""What tools/make_goldens_kitti.py and the KITTI-loader / K31 tests must agree on: the seeded images of the resample cases, the
layout of the tiny PNG tree tests/golden/kitti_tree, its made-up split lines, and the digests of the synthetic set's batches.
Nothing here imports PIL."""
import hashlib
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.join(REPO, "tests", "golden", "kitti_tree")

# (name, source (h, w), output (h, w)): odd / even sources whose tap windows are cut at both borders, to the training size, to
# half size, to a larger size (filterscale clamps to 1: KITTI's 370 -> 375), one axis unchanged (that pass is skipped), and a
# tiny up-scaling
RESIZE_CASES = [("odd_train", (37, 123), (32, 96)), ("even_train", (38, 124), (32, 96)), ("odd_half", (37, 123), (18, 61)),
                ("even_half", (38, 124), (19, 62)), ("larger", (37, 123), (38, 124)), ("rows_only", (37, 123), (32, 123)),
                ("cols_only", (38, 124), (38, 96)), ("tiny_up", (5, 7), (9, 13))]
FILTERS = ("lanczos", "bilinear")
KINDS = ("rand", "noise")       # uniform bytes; 0 / 255 noise, which drives both clips
CHAIN_SIZE = (32, 96)           # the four-level chain 37 x 123 -> 32 x 96 -> 16 x 48 -> 8 x 24 -> 4 x 12


def case_image(name, hw, kind):
    """uint8 [h, w, 3], seeded by the case's name and kind."""
    seed = int(hashlib.sha256(("%s/%s" % (name, kind)).encode()).hexdigest()[:8], 16)
    rng = np.random.RandomState(seed)
    if kind == "noise":
        return (rng.randint(0, 2, size=hw + (3,)) * 255).astype(np.uint8)
    return rng.randint(0, 256, size=hw + (3,)).astype(np.uint8)


# ---- the tree: two drives of different frame sizes, three frames each, both cameras
DRIVES = [("2011_09_26/2011_09_26_drive_0001_sync", (38, 124)), ("2011_09_28/2011_09_28_drive_0002_sync", (37, 123))]
FRAMES = (0, 1, 2)
# made-up split lines: both sides, both drives; frame 1 has both temporal neighbours in the tree
SPLIT_LINES = ["2011_09_26/2011_09_26_drive_0001_sync 1 l", "2011_09_28/2011_09_28_drive_0002_sync 1 r",
               "2011_09_28/2011_09_28_drive_0002_sync 0 l", "2011_09_26/2011_09_26_drive_0001_sync 2 r"]
TRAIN_SIZE = (32, 96)
GETITEM_SEED = 5                # random.seed() before the reference's __getitem__(0 .. 3) with is_train: mixes flipped and plain items
SCENE_CROP = (36, 120)          # KittiLoader's bottom-centre crop (h, w) on the tree's frames


def tree_image(drive, camera, frame, hw):
    return case_image("%s/%d/%d" % (drive, camera, frame), hw, "rand")


def tree_path(drive, camera, frame):
    return os.path.join(TREE, drive, "image_0%d" % camera, "data", "%010d.png" % frame)


# ---- the synthetic set's batches must stay what they are: digests of CPU batches for three seeds
SYNTH_SEEDS = (3, 1234, 99)


def synthetic_digests(dataset_cls):
    out = []
    for seed in SYNTH_SEEDS:
        ds = dataset_cls(64, 192, [0, "s"], 4, 8, "cpu", seed=seed, pool=4)
        for bi in range(2):
            batch = ds.next_batch(3)
            for key in sorted(batch, key=str):
                t = batch[key].detach().cpu().contiguous()
                out.append("%d/%d/%s=%s" % (seed, bi, key, hashlib.sha256(t.numpy().tobytes()).hexdigest()))
    return out
