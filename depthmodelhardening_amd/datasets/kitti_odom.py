"""KITTI odometry frames for the pose evaluation (``python -m depthmodelhardening_amd.evaluate_pose``).

The reference's ``KITTIOdomDataset`` (MD2/datasets/kitti_dataset.py:88-101) differs from the raw dataset in its file names only:
``<data_path>/sequences/<seq:02d>/image_<2|3>/<frame:06d><ext>``.  Its evaluation (MD2/evaluate_pose.py:58-67) reads
``splits/odom/test_files_<seq:02d>.txt`` with frame ids [0, 1], so item i is the pair (frame i, frame i + 1) and every frame
but the first and the last is decoded twice, once as frame 0 of pair i and once as frame 1 of pair i - 1.  The two lists are
exactly ``"<seq> <i> l"`` for i in range(pairs) -- 1590 lines for sequence 09 and 1200 for sequence 10 -- so ``odom_test_lines``
generates them and no list file ships here.

``odom_pair_frames`` decodes every file ONCE: it yields blocks of consecutive frames, float [n + 1, 3, height, width], whose
pairs are (block[:-1], block[1:]); the last frame of a block is carried over on the device as the first of the next.  It is built
on the raw loader's prefetcher and K31 exactly as ``datasets.kitti.eval_frames`` is: with ``is_train=False`` the reference's
``color_aug`` is ``color`` (mono_dataset.py:148-149, 193-196) and nothing is flipped.

Training on the odometry split is out of scope: ``datasets.kitti.from_options`` and the Trainer refuse ``--dataset kitti_odom``.
"""
import os

import torch

from .. import ops
from .kitti import SIDE_MAP, _Prefetcher, pool_workers

ODOM_TEST_PAIRS = {9: 1590, 10: 1200}        # the lengths of the reference's splits/odom/test_files_09.txt / _10.txt


def odom_image_path(data_path, sequence, frame_index, side, img_ext=".jpg"):
    """kitti_dataset.py:94-101."""
    return os.path.join(data_path, "sequences/{:02d}".format(int(sequence)), "image_{}".format(SIDE_MAP[side]),
                        "{:06d}{}".format(frame_index, img_ext))


def odom_test_lines(sequence, n_pairs):
    """The reference's ``splits/odom/test_files_<sequence:02d>.txt`` when ``n_pairs`` is its length: one line per frame pair."""
    return ["{} {} l".format(int(sequence), i) for i in range(int(n_pairs))]


def odom_pair_frames(data_path, sequence, n_pairs, height, width, device, img_ext=".jpg", batch_size=16, num_workers=12):
    """Blocks of consecutive frames of one sequence, left camera: float [n + 1, 3, height, width] with n <= ``batch_size`` pairs
    each, ``n_pairs`` pairs (``n_pairs + 1`` files) in all.  Every file is decoded once; the first frame of every block but the
    first is the previous block's last one, kept on the device."""
    n_pairs, batch_size = int(n_pairs), int(batch_size)
    if n_pairs < 1 or batch_size < 1:
        raise RuntimeError("odom_pair_frames: need at least one pair and a positive batch_size; got %d and %d" % (n_pairs, batch_size))
    paths = [odom_image_path(data_path, sequence, i, "l", img_ext) for i in range(n_pairs + 1)]
    # the first block decodes batch_size + 1 files, every later one batch_size: each block then holds batch_size pairs
    chunks = [paths[:batch_size + 1]] + [paths[i:i + batch_size] for i in range(batch_size + 1, len(paths), batch_size)]
    pre = _Prefetcher(batch_size + 1, device, pool_workers(num_workers))
    carry = None
    try:
        pre.submit(0, chunks[0])
        for k, chunk in enumerate(chunks):
            raw, sizes = pre.take(k)
            if k + 1 < len(chunks):
                pre.submit(k + 1, chunks[k + 1])
            out = ops.pil_resize(raw, (height, width), "lanczos", None, tuple(sizes), want_u8=False).f32
            pre.release(k)
            block = out if carry is None else torch.cat([carry, out], 0)
            carry = block[-1:].clone()          # its own storage: the consumer may drop the block
            yield block
    finally:
        pre.close()
