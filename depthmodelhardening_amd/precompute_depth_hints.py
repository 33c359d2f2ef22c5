"""Precompute depth hints by the 'fused SGM' method: depth-hints/precompute_depth_hints.py with its device half as one launch (K34)
and, with ``--matcher device``, its stereo matchers on the device too (K35).

    python -m depthmodelhardening_amd.precompute_depth_hints --data_path DIR --filenames LIST [--save_path DIR]
        [--height 320] [--width 1024] [--overwrite_saved_depths] [--matcher auto|opencv|device|files] [--candidates_dir DIR]
        [--save_candidates DIR] [--batch_size 8] [--num_workers 12]

For every line "sequence frame side" of the list: both views are decoded by the KITTI loader's pool (at most 16 threads) and
resized by ``ops.pil_resize(..., "lanczos", want_u8=True)`` (the reference's ANTIALIAS is LANCZOS); twelve candidate disparity
maps come from the matchers of ``generate_stereo_matchers`` (blockSize 1 / 2 / 3 x numDisparities 64 / 96 / 128 / 160);
``ops.depth_hint_fuse`` picks the candidate with the lowest reprojection loss per pixel, a batch of pairs per launch; the result is
saved as ``save_path/<sequence>/image_0{2,3}/<frame:010d>.npy``, float32 [1, H, W].  Files that exist are skipped unless
``--overwrite_saved_depths``.  The files of a batch are written after the next batch has been enqueued, so the device never waits
for the disk.

Where the candidates come from (``--matcher``):

    device   ``ops.sgm_disparity`` (K35) on the resized bytes already on the device, with the same twelve parameter sets and the
             reference's left-right reversal for a right base image as a per-item flag; the int16 tensor goes straight into the
             fusion, and nothing comes back to the host before the hints do.  PNG files in, hints out, with this package alone.
             K35 is this package's own matcher, modelled on StereoSGBM's structure; its maps are not OpenCV's.
             With ``--device cpu`` its host twin runs.
    opencv   OpenCV's StereoSGBM on host threads (the resized bytes come back for it): bound by twelve SGBM runs per pair.
    files    ``--candidates_dir``: one int16 [N, H, W] ``.npy`` per line laid out as the output is (disparity x 16, -16 = no match).
    auto     (default) opencv **if cv2 can be imported** and no ``--candidates_dir`` is given, files if it is given; without either
             the tool stops and says so.

``--save_candidates DIR`` also writes the candidates of every line in the ``--candidates_dir`` layout.
"""
import argparse
import os

import numpy as np
import torch

from . import ops
from .datasets import kitti
from .my_utils import to_device_async

BASELINE = 0.1                      # precompute_depth_hints.py:121, the baseline of datasets/mono_dataset.py
NUM_DISPARITIES = (64, 96, 128, 160)
BLOCK_SIZES = (1, 2, 3)


def import_cv2():
    """OpenCV, or None when it cannot be imported."""
    try:
        import cv2
    except ImportError:
        return None
    return cv2


def stereo_matcher_params():
    """The twelve parameter sets of generate_stereo_matchers (precompute_depth_hints.py:42-63), in its order."""
    sad_window_size = 3
    return [dict(preFilterCap=63, P1=sad_window_size * sad_window_size * 4, P2=sad_window_size * sad_window_size * 32, minDisparity=0,
                 numDisparities=num, uniquenessRatio=10, speckleWindowSize=100, speckleRange=16, blockSize=block)
            for block in BLOCK_SIZES for num in NUM_DISPARITIES]


def generate_stereo_matchers(cv2):
    return [cv2.StereoSGBM_create(**params) for params in stereo_matcher_params()]


def compute_candidates(matchers, base_image, lookup_image, reverse=False):
    """compute_depths (precompute_depth_hints.py:128-147) up to the raw disparities: int16 [N, H, W], disparity x 16.  ``reverse``:
    the base image is the right one (OpenCV matches for the left image): both are mirrored, and every result mirrored back."""
    if reverse:
        base_image, lookup_image = base_image[:, ::-1], lookup_image[:, ::-1]
    base_image, lookup_image = np.ascontiguousarray(base_image), np.ascontiguousarray(lookup_image)
    disps = []
    for matcher in matchers:
        disp = np.asarray(matcher.compute(base_image, lookup_image))
        disps.append(disp[:, ::-1] if reverse else disp)
    return np.stack(disps).astype(np.int16)


def camera(height, width, sides, device):
    """K, inv_K, T float32 [B, 4, 4] (precompute_depth_hints.py:107-123, :160-176): T[0, 3] = -0.1 for 'l', +0.1 otherwise."""
    K = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    K[0] *= width
    K[1] *= height
    inv_K = np.linalg.pinv(K)
    B = len(sides)
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T[:, 0, 3] = [(-1.0 if sd == "l" else 1.0) * BASELINE for sd in sides]
    mats = np.stack([np.tile(K, (B, 1, 1)), np.tile(inv_K.astype(np.float32), (B, 1, 1)), T])
    dev = to_device_async(mats, device, torch.float32)
    return dev[0], dev[1], dev[2]


def output_path(save_path, sequence, frame, side):
    return os.path.join(save_path, sequence, "image_02" if side == "l" else "image_03", "{}.npy".format(str(frame).zfill(10)))


def run(opt):
    """Computes depth hints for all files of opt.filenames; returns the number of files written."""
    print("Computing depth hints...")
    if opt.save_path is None:
        opt.save_path = os.path.join(opt.data_path, "depth_hints")
    print("Saving depth hints to {}".format(opt.save_path))
    device = torch.device(opt.device)
    H, W = int(opt.height), int(opt.width)
    mode = getattr(opt, "matcher", "auto")
    cv2 = import_cv2() if mode in ("auto", "opencv") else None
    if mode == "auto":
        if cv2 is None and not opt.candidates_dir:
            raise RuntimeError("precompute_depth_hints: no source of candidate disparities: OpenCV (cv2) cannot be imported for the "
                               "stereo matchers, and no --candidates_dir with precomputed int16 [N, H, W] .npy files was given")
        mode = "files" if opt.candidates_dir else "opencv"
    if mode == "opencv" and cv2 is None:
        raise RuntimeError("precompute_depth_hints: --matcher opencv, but OpenCV (cv2) cannot be imported")
    if mode == "files" and not opt.candidates_dir:
        raise RuntimeError("precompute_depth_hints: --matcher files needs --candidates_dir")
    matchers = None
    if mode == "opencv":
        cv2.setNumThreads(0)
        matchers = generate_stereo_matchers(cv2)
    save_candidates = getattr(opt, "save_candidates", None)
    lines = [tuple(ln.split()) for ln in kitti.read_split(opt.filenames) if ln.strip()]
    todo = [ln for ln in lines if opt.overwrite_saved_depths or not os.path.isfile(output_path(opt.save_path, *ln))]
    batch = max(1, int(opt.batch_size))
    chunks = [todo[i:i + batch] for i in range(0, len(todo), batch)]
    workers = kitti.pool_workers(opt.num_workers)
    pre = kitti._Prefetcher(2 * batch, device, workers)
    pool = pre.workers              # one pool of at most 16 threads for decoding, reading candidates and the matchers

    def paths_of(chunk):
        """view-major: the base images, then the lookup images"""
        def one(seq, frame, sd):
            return kitti.image_path(opt.data_path, seq, int(frame), sd, opt.img_ext)
        return [one(s, f, sd) for s, f, sd in chunk] + [one(s, f, "r" if sd == "l" else "l") for s, f, sd in chunk]

    def candidates(chunk, base_u8, lookup_u8):
        if mode == "device":
            # K35: from the bytes on the device to the fusion on the device (the flags go up through pinned memory)
            return ops.sgm_disparity(base_u8, lookup_u8, stereo_matcher_params(), reverse=[ln[2] != "l" for ln in chunk])
        if matchers is None:
            arrs = list(pool.map(lambda ln: np.load(output_path(opt.candidates_dir, *ln)), chunk))
        else:
            # the matchers run on the host: the resized bytes come back (a host read; this stage is bound by the matchers)
            b, l = base_u8.permute(0, 2, 3, 1).cpu().numpy(), lookup_u8.permute(0, 2, 3, 1).cpu().numpy()
            arrs = list(pool.map(lambda i: compute_candidates(matchers, b[i], l[i], reverse=chunk[i][2] != "l"), range(len(chunk))))
        for ln, a in zip(chunk, arrs):
            if a.dtype != np.int16 or a.ndim != 3 or a.shape[1:] != (H, W):
                raise RuntimeError("precompute_depth_hints: the candidates of %s must be int16 [N, %d, %d]; got %s %s"
                                   % (" ".join(ln), H, W, a.dtype, a.shape))
        return to_device_async(np.stack(arrs), device)

    def flush(pending):
        """write the files of a batch whose result has reached the host"""
        chunk, host, event, cand_host = pending
        if event is not None:
            event.synchronize()
        for i, (ln, depth) in enumerate(zip(chunk, host.numpy())):
            for root, array in ((opt.save_path, depth),) + (((save_candidates, cand_host[i].numpy()),) if cand_host is not None else ()):
                path = output_path(root, *ln)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                np.save(path, array)
        return len(chunk)

    written, pending = 0, None
    try:
        if chunks:
            pre.submit(0, paths_of(chunks[0]))
        for k, chunk in enumerate(chunks):
            raw, sizes = pre.take(k)
            if k + 1 < len(chunks):
                pre.submit(k + 1, paths_of(chunks[k + 1]))
            u8 = ops.pil_resize(raw, (H, W), "lanczos", None, tuple(sizes), want_float=False, want_u8=True).u8
            pre.release(k)
            n = len(chunk)
            base_u8, lookup_u8 = u8[:n], u8[n:]
            K, inv_K, T = camera(H, W, [ln[2] for ln in chunk], device)
            cand = candidates(chunk, base_u8, lookup_u8)
            best = ops.depth_hint_fuse(base_u8, lookup_u8, cand, K, inv_K, T)
            cand_host = None
            if save_candidates:
                cand_host = torch.empty(cand.shape, dtype=cand.dtype, pin_memory=device.type == "cuda")
                cand_host.copy_(cand, non_blocking=True)
            if device.type == "cuda":
                host = torch.empty(best.shape[:1] + best.shape[2:], dtype=torch.float32, pin_memory=True)
                host.copy_(best[:, 0], non_blocking=True)
                event = torch.cuda.Event()
                event.record(torch.cuda.current_stream(device))
            else:
                host, event = best[:, 0].contiguous(), None
            # this batch is enqueued: now the previous one's files are written
            if pending is not None:
                written += flush(pending)
            pending = (chunk, host.unsqueeze(1), event, cand_host)
        if pending is not None:
            written += flush(pending)
    finally:
        pre.close()
    print("wrote {} depth hints, skipped {}".format(written, len(lines) - len(todo)))
    return written


def get_opts(argv=None):
    """The reference's command line (precompute_depth_hints.py:265-293) and this package's additions."""
    parser = argparse.ArgumentParser()
    parser.add_argument("--data_path", help="path to images", type=str)
    parser.add_argument("--filenames", type=str, default="splits/eigen_full/all_files.txt",
                        help='path to textfile containing list of images. Each line is expected to be of the form '
                             '"sequence_name frame_number side"')
    parser.add_argument("--save_path", type=str,
                        help="path to save resulting depth hints to. If not set will save to datapath/depth_hints")
    parser.add_argument("--height", help="height of computed depth hints", default=320, type=int)
    parser.add_argument("--width", help="width of computed depth hints", default=1024, type=int)
    parser.add_argument("--overwrite_saved_depths", action="store_true",
                        help="if set, will overwrite any existing depth hints rather than skipping")
    parser.add_argument("--candidates_dir", type=str, default=None,
                        help="read the candidate disparities from here instead of running OpenCV's matchers: one int16 [N, H, W] "
                             ".npy per line (disparity x 16, -16 = no match), laid out as the output is")
    parser.add_argument("--matcher", type=str, default="auto", choices=["auto", "opencv", "device", "files"],
                        help="where the candidate disparities come from: this package's matcher on the device (K35; its host twin "
                             "with --device cpu), OpenCV's StereoSGBM on the host, --candidates_dir, or (auto) OpenCV if it can be "
                             "imported and no --candidates_dir is given, else the files")
    parser.add_argument("--save_candidates", type=str, default=None,
                        help="also write every line's candidates here, int16 [N, H, W] .npy in the --candidates_dir layout")
    parser.add_argument("--batch_size", type=int, default=8, help="stereo pairs per launch of the fusion")
    parser.add_argument("--num_workers", type=int, default=12, help="decode / matcher threads (at most 16)")
    parser.add_argument("--img_ext", type=str, default=".png", help="the reference reads data/<frame>.png")
    parser.add_argument("--device", type=str, default="cuda", help="cpu runs the host twins (tests)")
    return parser.parse_args(argv)


def main(argv=None):
    return run(get_opts(argv))


if __name__ == "__main__":
    main()
