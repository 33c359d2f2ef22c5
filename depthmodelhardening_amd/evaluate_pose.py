"""Pose evaluation on KITTI odometry: the reference's ``MD2/evaluate_pose.py``.

    python -m depthmodelhardening_amd.evaluate_pose --eval_split odom_9 --data_path ODOM --load_weights_folder W [--png]

The standard protocol: the pose network (``pose_encoder.pth`` + ``pose.pth``, the separate-resnet form, as a ``--pose_net``
training run saves them) runs on every consecutive frame pair of sequence 09 or 10; five-frame snippets are built from the
predicted and the ground-truth relative poses; each snippet is aligned by one scale factor; the mean and the standard deviation of
the absolute trajectory error are printed and ``poses.npy`` is saved into the weights folder.

Everything above the image files runs on the device.  ``datasets.kitti_odom.odom_pair_frames`` decodes each file once and K31
resizes it; the pose encoder's first layer takes the two frames of a pair as two views of one block (K41,
``ResnetEncoder.forward_pair``: no concatenation, no normalised copy); K29 is the head; the predicted poses stay on the device and
K40 (``ops.pose_ate``) chains and aligns the snippets and reduces the errors there.  The loop reads nothing back: one
device-to-host copy of the errors, the two statistics and the poses follows the last block.

``evaluate(..., host_chain=True)`` is the reference's shape on the same weights -- ``forward(torch.cat(...))``, a ``.cpu()`` per
batch, the numpy loop (``ops.pose_ate_host``) -- kept as the twin for the tests and for tools/pose_eval_bench.py.
"""
import os

import numpy as np
import torch

from . import networks, ops
from .datasets.kitti_odom import odom_pair_frames

POSE_EVAL_BATCH = 16


def load_pose_networks(opt, device):
    """MD2/evaluate_pose.py:69-81: ``ResnetEncoder(num_layers, False, 2)`` and ``PoseDecoder(num_ch_enc, 1, 2)`` from
    pose_encoder.pth and pose.pth, in eval mode."""
    folder = os.path.expanduser(opt.load_weights_folder)
    pose_encoder = networks.ResnetEncoder(opt.num_layers, False, 2)
    pose_encoder.load_state_dict(torch.load(os.path.join(folder, "pose_encoder.pth"), map_location="cpu"))
    pose_decoder = networks.PoseDecoder(pose_encoder.num_ch_enc, 1, 2)
    pose_decoder.load_state_dict(torch.load(os.path.join(folder, "pose.pth"), map_location="cpu"))
    return pose_encoder.to(device).eval(), pose_decoder.to(device).eval()


def evaluate(opt, frames=None, gt_global_poses=None, host_chain=False):
    """Evaluate odometry on the KITTI dataset (MD2/evaluate_pose.py:49-129).

    ``frames``: an iterable of float [n + 1, 3, h, w] device blocks of consecutive frames in place of ``odom_pair_frames``;
    ``gt_global_poses``: [N + 1, 3, 4] in place of ``<data_path>/poses/<seq>.txt``.  Returns {"ate_mean", "ate_std", "ates"
    float64 [N], "pred_poses" float32 [N, 4, 4]} (numpy)."""
    assert os.path.isdir(opt.load_weights_folder), \
        "Cannot find a folder at {}".format(opt.load_weights_folder)
    assert opt.eval_split == "odom_9" or opt.eval_split == "odom_10", \
        "eval_split should be either odom_9 or odom_10"
    sequence_id = int(opt.eval_split.split("_")[1])
    device = torch.device("cuda")
    ops._need_cuda(device)
    pose_encoder, pose_decoder = load_pose_networks(opt, device)

    if gt_global_poses is None:
        gt_global_poses = np.loadtxt(os.path.join(opt.data_path, "poses", "{:02d}.txt".format(sequence_id))).reshape(-1, 3, 4)
    gt_local = ops.gt_local_poses(gt_global_poses)
    n_pairs = len(gt_local)
    batch = max(1, int(opt.batch_size))
    if frames is None:
        frames = odom_pair_frames(opt.data_path, sequence_id, n_pairs, opt.height, opt.width, device, ".png" if opt.png else ".jpg",
                                  batch, opt.num_workers)
    gt_dev = None if host_chain else torch.from_numpy(gt_local).to(device, non_blocking=True)

    print("-> Computing pose predictions")
    pred, count = [], 0
    with torch.no_grad():
        for block in frames:
            if block.dim() != 4 or block.shape[0] < 2 or block.shape[1] != 3:
                raise RuntimeError("evaluate: a block of frames must be [n + 1, 3, h, w] with n >= 1; got %s" % (tuple(block.shape),))
            for i in range(0, block.shape[0] - 1, batch):
                f = block[i:i + batch + 1]
                if host_chain:      # the reference's shape: the concatenation, the encoder's own stem, a copy per batch
                    pose_decoder([pose_encoder(torch.cat([f[:-1], f[1:]], 1))])
                    pred.append(pose_decoder.T[:, 0].cpu().numpy())
                else:
                    pose_decoder([pose_encoder.forward_pair(f[:-1], f[1:])])
                    pred.append(pose_decoder.T[:, 0])
                count += f.shape[0] - 1
    if count != n_pairs:
        raise RuntimeError("evaluate: %d frame pairs but %d ground-truth local poses" % (count, n_pairs))

    if host_chain:
        pred_poses = np.ascontiguousarray(np.concatenate(pred), dtype=np.float32)
        ates, mean, std = ops.pose_ate_host(pred_poses, gt_local, ops.POSE_TRACK_LENGTH)
    else:
        pred_dev = torch.cat(pred).contiguous()
        out = ops.pose_ate(pred_dev, gt_dev, ops.POSE_TRACK_LENGTH)
        # the one copy: [N] errors, the two statistics and the [N, 16] poses as float64 (float32 widens exactly)
        table = torch.cat([out.ates, out.stats, pred_dev.reshape(-1).double()]).cpu().numpy()
        ates, (mean, std) = table[:n_pairs], table[n_pairs:n_pairs + 2]
        pred_poses = table[n_pairs + 2:].astype(np.float32).reshape(n_pairs, 4, 4)

    print("\n   Trajectory error: {:0.3f}, std: {:0.3f}\n".format(mean, std))
    save_path = os.path.join(opt.load_weights_folder, "poses.npy")
    np.save(save_path, pred_poses)
    print("-> Predictions saved to", save_path)
    return {"ate_mean": float(mean), "ate_std": float(std), "ates": np.array(ates, dtype=np.float64), "pred_poses": pred_poses}


def main(argv=None):
    import sys
    from .options import MonodepthOptions
    args = list(sys.argv[1:] if argv is None else argv)
    if not any(a == "--batch_size" or a.startswith("--batch_size=") for a in args):
        args += ["--batch_size", str(POSE_EVAL_BATCH)]
    return evaluate(MonodepthOptions().parse(args))


if __name__ == "__main__":
    main()
