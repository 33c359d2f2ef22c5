"""KITTI raw from disk: ``KITTIRAWDataset`` (MD2/datasets/kitti_dataset.py:18-68 + mono_dataset.py:42-375) and the attack's
scene feed ``KittiSceneFeed`` (dataLoader.py:107-209), with the reference's image pyramid on the device (K31).

Host side: the files of a batch are decoded by PIL in a pool of ``min(num_workers, 16)`` threads straight into a pinned uint8
buffer [views x batch, 376, 1242, 3] (KITTI raw frames are 370..376 x 1224..1242; each lies in the top-left corner of its slot),
and a loader thread uploads the buffer on a side stream while the current step runs: two buffers, an event before first use.
``KittiSceneFeed`` decodes the next call's scenes in the background the same way (the attack asks for the same number every
iteration); its generator draws them one call ahead, in the same order.

Device side, ``preprocess="reference"``: what ``MonoDataset.preprocess`` does with PIL, bit for bit, by ``ops.pil_pyramid``:
  benign       the raw bytes, the per-sample ``do_flip`` as K31's mirrored read -> ("color", f, 0..3), ("color_aug", f, 0).
  adversarial  ``prep_adv_data`` (mono_dataset.py:186-265): the frames become float (``to_tensor``), are resized to 375 x 1242 with
               F.interpolate(bilinear, align_corners=False) when their size differs (:196-199, torchvision 0.8.2's tensor Resize),
               get the object by the three K3 pastes of ``SyntheticKITTIDataset.synthesize`` at out_size (375, 1242) -- at the
               frame's own size K3's resize taps are (y, x) with weight exactly 1, so the output is the plain composite -- and
               K31's float-in mode then does ``ToPILImage``'s truncating 8-bit round trip and the LANCZOS chain.  The object mask
               goes through as one channel and is expanded.  Only what the Trainer reads is built: the opposite view's coarse
               levels only with ``right_pyramid``.
``preprocess="fast"``: the synthetic set's path fed from files -- K3 resizes bilinearly inside the paste, benign frames are
resized by F.interpolate, the coarse levels are 2^s box means.  Not the reference's pixels; half the launches.

ColorJitter (only with ``color_aug``, for half of the samples, mono_dataset.py:297,344-348): ``jitter="pil"`` keeps K31's level-0
bytes of the keys that are jittered and runs torchvision 0.8.2's ColorJitter on them as Pillow computes it on the 8-bit image --
a byte after each of the four operations, the grey of the saturation step as Pillow's integer L, the contrast mean of every
image, the hue shifted on the H byte -- by ``ops.pil_color_jitter`` (K33): one call for every key of the batch, two launches, none
when no coin fell.  ``jitter="float"`` (the default) applies color_jitter.py's tensor operations to the float level 0 in a loop
over items and keys.

Departures, stated: with ``jitter="float"`` the jittered pixels are not the reference's (``jitter="pil"`` removes this one); the
coarser ``color_aug`` levels are not built (nothing reads them).  Under
``half_no_synthesis`` the samples without an object take the float round trip of the others, which returns every byte
((v / 255.f) * 255.f truncates to v for all 256 values: tests/test_pil_resample_ref.py).  The reference pins Pillow
5.4.1; K31 and K33 are held to the Pillow that is installed (12.x), whose 8-bit resample, blend and HSV conversions are believed,
not checked, to round the same way.

``depth_gt`` (kitti_dataset.py:70-85): when the scan of the first split line exists (``check_depth``), the scans of a batch are read
by the same pool with ``np.fromfile`` into a pinned float32 buffer [points, 4], ragged, the offsets from the file sizes, uploaded with
the frames; ``ops.velo_depth_map`` (K32) projects them with the camera of the split line's side, resizes to ``full_res_shape`` and
mirrors the flipped samples -> inputs["depth_gt"] [B, 1, 375, 1242].  The resize is K32's integer nearest rule, not
scikit-image 0.17.2's fitted affine map.

``depth_hint`` / ``depth_hint_mask`` (depth-hints/datasets/mono_dataset.py:368-388, with ``use_depth_hints``): the ``.npy`` hint of every
item (``<depth_hint_path>/<folder>/image_0{2,3}/<frame:010d>.npy``, float32 [1, Hs, Ws], written by precompute_depth_hints.py) is read
by the same pool into a pinned float32 buffer and uploaded with the frames; ``ops.depth_hint_prepare`` (K34's second kernel)
mirrors the flipped items, resizes to (height, width) by OpenCV's INTER_NEAREST rule and forms the mask (hint > 0), one launch.
A missing file raises the reference's ``FileNotFoundError``.  The hints of one batch must share a size (the precompute tool writes
one size); the adversarial paste leaves hints untouched, as in the reference.

PIL is imported here (and by export_gt_depth's PNG branch) and nowhere else in the package, when a file is first decoded.
"""
import os
import random
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

from .. import color_jitter, ops
from . import kitti_velo
from ..my_utils import ori_H, ori_W, to_device_async
from .synthetic import SyntheticKITTIDataset

MAX_WORKERS = 16            # a GPU machine gives a command 16 CPUs; never sized by os.cpu_count()
SLOT_H, SLOT_W = 376, 1242  # the largest KITTI raw frame
SIDE_MAP = {"2": 2, "3": 3, "l": 2, "r": 3}      # kitti_dataset.py:35
OTHER_SIDE = {"r": "l", "l": "r"}


def _pil():
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("--dataset kitti decodes its files with PIL (Pillow), which is not installed: %s" % e)
    return Image


def pool_workers(num_workers):
    return max(1, min(int(num_workers), MAX_WORKERS))


def read_split(path):
    """The lines of a Monodepth2 split file (MD2/utils.py readlines)."""
    if not os.path.isfile(path):
        raise RuntimeError("split file %s not found: --split_dir must hold <split>/train_files.txt, val_files.txt and "
                           "<eval_split>/test_files.txt (Monodepth2's lists; none ships with this repository)" % path)
    with open(path) as f:
        return f.read().splitlines()


def parse_line(line):
    """(folder, frame_index, side) of a split line (mono_dataset.py:301-312): three fields, or a folder alone (frame 0, no side)."""
    parts = line.split()
    folder = parts[0]
    if len(parts) == 3:
        return folder, int(parts[1]), parts[2]
    return folder, 0, None


def image_path(data_path, folder, frame_index, side, img_ext=".jpg"):
    """kitti_dataset.py:64-68."""
    return os.path.join(data_path, folder, "image_0{}/data".format(SIDE_MAP[side]), "{:010d}{}".format(frame_index, img_ext))


def decode_into(path, slot):
    """pil_loader (mono_dataset.py:34-39) into a uint8 [SLOT_H, SLOT_W, 3] slot, a numpy view (a torch copy from sixteen threads
    at once starts sixteen intra-op thread teams that spin against each other); returns the image's (h, w)."""
    Image = _pil()
    with open(path, "rb") as f:
        with Image.open(f) as img:
            a = np.array(img.convert("RGB"))
    h, w = a.shape[:2]
    if h > slot.shape[0] or w > slot.shape[1]:
        raise RuntimeError("%s is %d x %d; frames larger than %d x %d are not KITTI raw" % (path, h, w, slot.shape[0], slot.shape[1]))
    slot[:h, :w] = a
    return h, w


def hint_path(depth_hint_path, folder, frame_index, side):
    """depth-hints/datasets/mono_dataset.py:369-371."""
    return os.path.join(depth_hint_path, folder, "image_02" if side == "l" else "image_03", str(frame_index).zfill(10) + ".npy")


def load_hint(item):
    """``np.load(path)[0]`` of (depth_hint_path, folder, frame_index, side) as float32 [Hs, Ws]; a missing file raises with the
    reference's wording (mono_dataset.py:373-380)."""
    root, folder, frame_index, side = item
    try:
        depth = np.load(hint_path(root, folder, frame_index, side))[0]
    except FileNotFoundError:
        raise FileNotFoundError("Warning - cannot find depth hint for {} {} {}! "
                                "Either specify the correct path in option "
                                "--depth_hint_path, or run precompute_depth_hints.py to"
                                "train with depth hints".format(folder, "image_02" if side == "l" else "image_03", frame_index))
    if depth.ndim != 2:
        raise RuntimeError("depth hint %s must be an array [1, H, W]; got %s" % (hint_path(root, folder, frame_index, side), (1,) + depth.shape))
    return np.asarray(depth, dtype=np.float32)


class _Prefetcher(object):
    """Two pinned uint8 buffers and their device twins.  ``submit(k, paths)`` decodes batch k into buffer k % 2 on the worker pool
    and uploads it on a side stream from a loader thread; ``take(k)`` returns (device buffer, sizes) once the current stream has
    been told to wait for the upload's event."""

    def __init__(self, slots, device, workers, slot_hw=(SLOT_H, SLOT_W)):
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        self.workers = ThreadPoolExecutor(max_workers=workers)
        self.loader = ThreadPoolExecutor(max_workers=1)
        slot_h, slot_w = int(slot_hw[0]), int(slot_hw[1])       # the KITTI raw slot; test_simple sizes it by its folder's files
        self.host = [torch.empty((slots, slot_h, slot_w, 3), dtype=torch.uint8, pin_memory=self.cuda) for _ in range(2)]
        self.host_np = [t.numpy() for t in self.host]          # the workers write through numpy views of the pinned buffers
        self.dev = [torch.empty((slots, slot_h, slot_w, 3), dtype=torch.uint8, device=self.device) for _ in range(2)] if self.cuda else self.host
        self.side = torch.cuda.Stream(self.device) if self.cuda else None
        self.uploaded = [None, None]     # event: the upload of the buffer has finished
        self.consumed = [None, None]     # event: the kernels that read the device buffer have been queued before it
        self.pending = {}
        self.wait_s = 0.0                # time the consuming thread spent waiting for a batch that was not ready
        # velodyne scans: per buffer a pinned float32 [capacity, 4] and int32 offsets, their device twins; grown on demand
        self.cloud_host, self.cloud_dev = [None, None], [None, None]
        self.clouds = [None, None]       # (device points [total, 4], device offsets int32 [n + 1]) of the buffer's batch
        # depth hints: per buffer a pinned float32 [n, 1, Hs, Ws] and its device twin; (re)allocated when the shape changes
        self.hint_host, self.hint_dev = [None, None], [None, None]

    def _load_hints(self, b, items):
        """The hints ``items`` into buffer b.  Runs after the buffer's last upload finished."""
        arrs = list(self.workers.map(load_hint, items))
        if len({a.shape for a in arrs}) != 1:
            raise RuntimeError("KITTIRAWDataset: the depth hints of one batch must share a size; got %s" % sorted({a.shape for a in arrs}))
        shape = (len(arrs), 1) + arrs[0].shape
        if self.hint_host[b] is None or tuple(self.hint_host[b].shape) != shape:
            if self.cuda and self.consumed[b] is not None:
                self.consumed[b].synchronize()      # the kernels that read the old device buffer have run
            self.hint_host[b] = torch.empty(shape, dtype=torch.float32, pin_memory=self.cuda)
            if self.cuda:
                self.hint_dev[b] = torch.empty(shape, dtype=torch.float32, device=self.device)
                fresh = torch.cuda.Event()      # the allocator may hand out memory that queued work still reads
                fresh.record(torch.cuda.current_stream(self.device))
                self.side.wait_event(fresh)
            else:
                self.hint_dev[b] = self.hint_host[b]
        view = self.hint_host[b].numpy()
        for i, a in enumerate(arrs):
            view[i, 0] = a

    def _load_clouds(self, b, velo):
        """The scans ``velo`` into buffer b: ragged, offsets from the file sizes.  Runs after the buffer's last upload finished."""
        counts = [kitti_velo.cloud_points(p) for p in velo]
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        total, n = int(offsets[-1]), len(velo)
        host = self.cloud_host[b]
        if host is None or host[0].shape[0] < total or host[1].numel() < n + 1:
            if self.cuda and self.consumed[b] is not None:
                self.consumed[b].synchronize()      # the kernels that read the old device buffer have run
            cap = max(total + total // 4, 1)
            host = self.cloud_host[b] = (torch.empty((cap, 4), dtype=torch.float32, pin_memory=self.cuda),
                                         torch.empty(n + 1, dtype=torch.int32, pin_memory=self.cuda))
            if self.cuda:
                self.cloud_dev[b] = tuple(torch.empty(t.shape, dtype=t.dtype, device=self.device) for t in host)
                fresh = torch.cuda.Event()      # the allocator may hand out memory that queued work still reads
                fresh.record(torch.cuda.current_stream(self.device))
                self.side.wait_event(fresh)
            else:
                self.cloud_dev[b] = host
        pts, off = host[0].numpy(), host[1].numpy()
        off[:n + 1] = offsets
        list(self.workers.map(lambda ip: kitti_velo.read_cloud_into(ip[1], pts[offsets[ip[0]]:offsets[ip[0] + 1]]), enumerate(velo)))
        return total, n

    def _load(self, k, paths, velo=None, hints=None):
        b = k % 2
        if self.cuda and self.uploaded[b] is not None:
            self.uploaded[b].synchronize()          # the pinned buffers are free once their last upload is done
        sizes = list(self.workers.map(lambda ip: decode_into(ip[1], self.host_np[b][ip[0]]), enumerate(paths)))
        total, n = self._load_clouds(b, velo) if velo else (0, 0)
        if velo:
            self.clouds[b] = (self.cloud_dev[b][0][:total], self.cloud_dev[b][1][:n + 1])
        if hints:
            self._load_hints(b, hints)
        if self.cuda:
            with torch.cuda.stream(self.side):
                if self.consumed[b] is not None:
                    self.side.wait_event(self.consumed[b])
                self.dev[b][:len(paths)].copy_(self.host[b][:len(paths)], non_blocking=True)
                if velo:
                    self.clouds[b][0].copy_(self.cloud_host[b][0][:total], non_blocking=True)
                    self.clouds[b][1].copy_(self.cloud_host[b][1][:n + 1], non_blocking=True)
                if hints:
                    self.hint_dev[b].copy_(self.hint_host[b], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.side)
            self.uploaded[b] = ev
        return sizes

    def submit(self, k, paths, velo=None, hints=None):
        if k not in self.pending:
            self.pending[k] = (self.loader.submit(self._load, k, list(paths), None if velo is None else list(velo),
                                                  None if hints is None else list(hints)), len(paths))

    def take(self, k):
        fut, n = self.pending.pop(k)
        t0 = time.perf_counter()
        sizes = fut.result()
        self.wait_s += time.perf_counter() - t0
        b = k % 2
        if self.cuda:
            torch.cuda.current_stream(self.device).wait_event(self.uploaded[b])
        return self.dev[b][:n], sizes

    def take_clouds(self, k):
        """(points [total, 4], offsets int32 [n + 1]) of batch k on the device, after ``take(k)``."""
        return self.clouds[k % 2]

    def take_hints(self, k):
        """float32 [n, 1, Hs, Ws] of batch k on the device, after ``take(k)``."""
        return self.hint_dev[k % 2]

    def release(self, k):
        """The current stream has queued every read of batch k's device buffer."""
        if self.cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self.consumed[k % 2] = ev

    def close(self):
        self.loader.shutdown(wait=True)
        self.workers.shutdown(wait=True)


class KITTIRAWDataset(SyntheticKITTIDataset):
    """``next_batch(batch_size)`` returns the keys of ``SyntheticKITTIDataset.next_batch``; the adversarial hooks
    (``set_adv_train``, ``update_adv_obj``, ``begin_epoch``), ``synthesize`` and ``_camera`` are the base class's code."""

    def __init__(self, data_path, filenames, height, width, frame_idxs, num_scales, device, is_train=False, img_ext=".jpg",
                 seed=1234, num_workers=12, preprocess="reference", color_aug=False, full_res_shape=(ori_H, ori_W), jitter="float",
                 use_depth_hints=False, depth_hint_path=None):
        if preprocess not in ("reference", "fast"):
            raise RuntimeError("kitti_preprocess must be 'reference' or 'fast'; got %r" % (preprocess,))
        if jitter not in ("float", "pil"):
            raise RuntimeError("kitti_jitter must be 'float' or 'pil'; got %r" % (jitter,))
        if jitter == "pil" and preprocess != "reference":
            raise RuntimeError("kitti_jitter 'pil' jitters the 8-bit level 0 that kitti_preprocess 'reference' builds; "
                               "kitti_preprocess %r has no PIL bytes" % (preprocess,))
        if not filenames:
            raise RuntimeError("KITTIRAWDataset: the split list is empty")
        self.data_path, self.filenames = data_path, list(filenames)
        # the base class's state (sizes, self.rng: the per-sample draws in __getitem__'s order, switches, camera); no pool of frames
        self._init_common(height, width, list(frame_idxs), num_scales, len(self.filenames), device, seed)
        self.is_train, self.img_ext = bool(is_train), img_ext
        self.preprocess, self.color_aug, self.jitter = preprocess, bool(color_aug), jitter
        self.order_rng = random.Random(seed + 1)     # the DataLoader's shuffle: apart, so that it never moves a draw
        self.flip_augmentation = self.is_train       # mono_dataset.py:298
        self.full_res_shape = (int(full_res_shape[0]), int(full_res_shape[1]))      # depth_gt's size (kitti_dataset.py:34)
        self.load_depth = self.check_depth()
        self.use_depth_hints = bool(use_depth_hints)
        self.depth_hint_path = depth_hint_path if depth_hint_path is not None else os.path.join(data_path, "depth_hints")
        if self.use_depth_hints and "s" not in self.frame_idxs:
            raise RuntimeError("KITTIRAWDataset: depth hints are loaded with the stereo frame (mono_dataset.py:359-368); "
                               "frame_idxs must hold 's' (--use_stereo)")
        self.views = [0] + (["s"] if "s" in self.frame_idxs else []) + self.neighbour_ids
        self.pool_workers = pool_workers(num_workers)
        self._prefetch = None
        self._order, self._cursor, self._step = [], 0, 0
        self.scene_feed = None                       # a KittiSceneFeed: the attack's scenes (Trainer sets it from --scene_root)

    # ------------------------------------------------------------------ host side
    def paths_of(self, index):
        """The files of item ``index``, one per view of ``self.views`` (mono_dataset.py:314-319)."""
        folder, frame_index, side = parse_line(self.filenames[index])
        out = []
        for f in self.views:
            if f == "s":
                out.append(image_path(self.data_path, folder, frame_index, OTHER_SIDE[side], self.img_ext))
            else:
                out.append(image_path(self.data_path, folder, frame_index + f, side, self.img_ext))
        return out

    def check_depth(self):
        return kitti_velo.check_depth(self.data_path, self.filenames)

    def velo_path(self, index):
        folder, frame_index, _ = parse_line(self.filenames[index])
        return kitti_velo.velo_path(self.data_path, folder, frame_index)

    def _next_indices(self, n):
        idx = []
        while len(idx) < n:
            if self._cursor >= len(self._order):
                self._order = list(range(self.length))
                if self.is_train:
                    self.order_rng.shuffle(self._order)
                self._cursor = 0
            idx.append(self._order[self._cursor])
            self._cursor += 1
        return idx

    def _submit(self, k, batch_size):
        idx = self._next_indices(batch_size)
        # view-major: slot v * batch + i
        paths = [p for v in range(len(self.views)) for p in (self.paths_of(i)[v] for i in idx)]
        hints = None
        if self.use_depth_hints:
            hints = [(self.depth_hint_path,) + parse_line(self.filenames[i]) for i in idx]
        self._prefetch.submit(k, paths, [self.velo_path(i) for i in idx] if self.load_depth else None, hints)
        return idx

    def _depth_gt(self, k, idx, sides, flip):
        """get_depth (kitti_dataset.py:70-85) for the batch: K32 with each line's camera, at full_res_shape, flipped samples mirrored."""
        points, offsets = self._prefetch.take_clouds(k)
        calib = [kitti_velo.velo_projection(kitti_velo.calib_dir(self.data_path, parse_line(self.filenames[i])[0]), SIDE_MAP[sd])
                 for i, sd in zip(idx, sides)]
        proj = to_device_async(np.stack([P for P, _ in calib]), self.device)
        return ops.velo_depth_map(points, offsets, proj, [hw for _, hw in calib], False, self.full_res_shape, flip).unsqueeze(1)

    def _draw_first(self, geo):
        """do_color_aug's coin (mono_dataset.py:297: one ``random()`` whenever is_train, whether or not colour is augmented) comes
        before do_flip (:298); the rest of ``draw_batch_geometry`` -- flip, the synthesis coin (:324), (z0, alpha) inside
        prep_adv_data -- is the base class's, with the side taken from the split line."""
        coin = self.rng.random() > 0.5 if self.is_train else False
        geo.setdefault("jitter", []).append(coin and self.color_aug)

    def _draw_last(self, geo):
        """ColorJitter.get_params of an item whose coin fell comes last in ``__getitem__`` (mono_dataset.py:344-346), before the
        next item's coin."""
        geo.setdefault("jitter_params", []).append(self._jitter_params() if geo["jitter"][-1] else None)

    def _jitter_params(self):
        """ColorJitter.get_params (mono_dataset.py:345-346; torchvision 0.8.2: four uniforms, then the shuffle of the four
        operations) drawn from this dataset's generator."""
        b, c, s, h = (self.rng.uniform(lo, hi) for lo, hi in ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1)))
        order = ["brightness", "contrast", "saturation", "hue"]
        self.rng.shuffle(order)
        return color_jitter.JitterParams(b, c, s, h, order)

    # ------------------------------------------------------------------ device side
    def _float_frames(self, raw, sizes):
        """``to_tensor`` of the raw frames and mono_dataset.py:196-199: [n, 3, 375, 1242] float, resized where the size differs."""
        out = torch.empty((raw.shape[0], 3, ori_H, ori_W), device=raw.device, dtype=torch.float32)
        groups = {}
        for i, hw in enumerate(sizes):
            groups.setdefault(hw, []).append(i)
        for (h, w), members in groups.items():
            sel = raw if len(members) == raw.shape[0] else raw[to_device_async(members, raw.device, torch.int64)]
            x = sel[:, :h, :w].permute(0, 3, 1, 2).float().div(255)
            if (h, w) != (ori_H, ori_W):
                x = F.interpolate(x, [ori_H, ori_W], mode="bilinear", align_corners=False)
            if len(members) == raw.shape[0]:
                return x.contiguous()
            out[to_device_async(members, raw.device, torch.int64)] = x
        return out

    def _levels(self, inputs, view, src, flip=None, sizes=None, full=True, keep_u8=False):
        """("color", view, s) by K31 from ``src`` (raw uint8 HWC with sizes and flip, or a float frame); returns the level-0 bytes
        with ``keep_u8`` (K33 jitters them)."""
        H, W = self.height, self.width
        if full:
            levels = ops.pil_pyramid(src, H, W, self.num_scales, "lanczos", flip, sizes)
            for s, lvl in enumerate(levels):
                inputs[("color", view, s)] = lvl.f32
            return levels[0].u8
        lvl = ops.pil_resize(src, (H, W), "lanczos", flip, sizes, want_u8=keep_u8)
        inputs[("color", view, 0)] = lvl.f32
        return lvl.u8

    def _box_levels(self, inputs, view, img):
        inputs[("color", view, 0)] = img
        if view != 0 and not self.right_pyramid:
            return
        fused = img.is_cuda and self.num_scales == 4 and self.height % 8 == 0 and self.width % 8 == 0
        levels = ops.avg_pyramid(img) if fused else [F.avg_pool2d(img, 2 ** s) for s in range(1, self.num_scales)]
        for s in range(1, self.num_scales):
            inputs[("color", view, s)] = levels[s - 1]

    def next_batch(self, batch_size):
        dev, H, W = self.device, self.height, self.width
        if self._prefetch is None:
            self._prefetch = _Prefetcher(len(self.views) * batch_size, dev, self.pool_workers)
            self._batch = batch_size
            self._queued = self._submit(self._step, batch_size)
        if batch_size != self._batch:
            raise RuntimeError("KITTIRAWDataset: the batch size is fixed by the first batch (%d); got %d" % (self._batch, batch_size))
        k, idx = self._step, self._queued
        raw, sizes = self._prefetch.take(k)
        self._step += 1
        self._queued = self._submit(self._step, batch_size)      # the next batch decodes and uploads while this one is used
        sides = [parse_line(self.filenames[i])[2] for i in idx]
        if "s" in self.frame_idxs and any(sd is None for sd in sides):
            raise RuntimeError("KITTIRAWDataset: a split line without a camera side cannot serve frame id 's'")
        if self.is_adv_train and "s" not in self.frame_idxs:
            raise RuntimeError("KITTIRAWDataset: adversarial training pastes into frame 0 and its stereo partner "
                               "(mono_dataset.py:186-261); frame_idxs must hold 's' (--use_stereo)")
        geo = self.draw_batch_geometry(batch_size, sides)
        B = batch_size
        view_raw = {v: raw[j * B:(j + 1) * B] for j, v in enumerate(self.views)}
        view_sizes = {v: tuple(sizes[j * B:(j + 1) * B]) for j, v in enumerate(self.views)}
        flip = to_device_async([int(f) for f in geo["flip"]], dev, torch.int32) if any(geo["flip"]) else None
        reference = self.preprocess == "reference"
        inputs = {}
        pil_jitter = self.jitter == "pil" and any(geo["jitter"])
        u8 = {}         # the level-0 bytes of the keys K33 jitters
        if self.is_adv_train:
            # frame 0 / the opposite view as a pool of float frames that K3 reads by index, as the synthetic set's pool is read
            self.raw = torch.cat([self._float_frames(view_raw[0], view_sizes[0]), self._float_frames(view_raw["s"], view_sizes["s"])], 0)
            both = to_device_async([list(range(B)), list(range(B, 2 * B))], dev, torch.int32)
            out_size = (ori_H, ori_W) if reference else (H, W)
            aug0, aug_s, ben0, mask0 = self.synthesize(None, None, geo, out_size, pool_index=(both[0], both[1]))
            if reference:
                lvl = ops.pil_resize(aug0, (H, W), want_u8=pil_jitter)
                inputs[("color_aug", 0, 0)], u8[("color_aug", 0, 0)] = lvl.f32, lvl.u8
                u8[("color_ben", 0, 0)] = self._levels(inputs, 0, ben0)         # ("color", 0, -1) = color_ben, :257
                u8[("color_aug", "s", 0)] = self._levels(inputs, "s", aug_s, full=self.right_pyramid, keep_u8=pil_jitter)   # :258
                inputs[("color_ben", 0, 0)] = inputs[("color", 0, 0)]
                mask0 = ops.pil_resize(mask0, (H, W), want_u8=False).f32
            else:
                inputs[("color_aug", 0, 0)] = aug0
                self._box_levels(inputs, 0, ben0)
                self._box_levels(inputs, "s", aug_s)
                inputs[("color_ben", 0, 0)] = ben0
            if not self.half_no_synthesis:
                inputs[("color_objmask", 0, 0)] = mask0.expand(-1, 3, -1, -1)
                inputs[("objdepth", 0, 0)] = to_device_async(geo["z0"], dev, torch.float32).view(B, 1)
            plain = self.neighbour_ids
            if self.neighbour_ids:
                inputs[("color_aug", "s", 0)] = inputs[("color", "s", 0)]
        else:
            plain = self.views
        for v in plain:
            if reference:
                u8[("color_aug", v, 0)] = self._levels(inputs, v, view_raw[v], flip, view_sizes[v],
                                                       full=(v == 0 or self.right_pyramid), keep_u8=pil_jitter)
            else:
                img = F.interpolate(self._float_frames(view_raw[v], view_sizes[v]), [H, W], mode="bilinear", align_corners=False)
                if flip is not None:
                    img = torch.where(flip.view(B, 1, 1, 1) != 0, img.flip(3), img)
                self._box_levels(inputs, v, img)
            if v != "s" or self.neighbour_ids:
                inputs[("color_aug", v, 0)] = inputs[("color", v, 0)]
        if self.load_depth:
            if any(sd is None for sd in sides):
                raise RuntimeError("KITTIRAWDataset: depth_gt needs the camera side of every split line")
            inputs["depth_gt"] = self._depth_gt(k, idx, sides, flip)
        if self.use_depth_hints:
            # mono_dataset.py:382-388: fliplr, INTER_NEAREST to the training size, the mask; the pasted object never touches it
            inputs["depth_hint"], inputs["depth_hint_mask"] = ops.depth_hint_prepare(self._prefetch.take_hints(k), flip, (H, W))
        self._prefetch.release(k)
        if pil_jitter:
            # mono_dataset.py:344-348 on the 8-bit level 0: one transform per item, the same for every frame of the item; every
            # key of the batch in one call of K33, the items whose coin did not fall are only converted
            keys = [q for q in inputs if q[0] in ("color_aug", "color_ben")]
            for key, res in zip(keys, ops.pil_color_jitter([u8[q] for q in keys], geo["jitter_params"])):
                inputs[key] = res.f32
        elif any(geo["jitter"]):
            # the same on the float level 0 by tensor operations: not the reference's pixels
            for i, aug in enumerate(geo["jitter_params"]):
                if aug is None:
                    continue
                for key in [q for q in inputs if q[0] in ("color_aug", "color_ben")]:
                    if inputs[key] is inputs.get(("color", key[1], key[2])):
                        inputs[key] = inputs[key].clone()
                    inputs[key][i] = aug(inputs[key][i])
        inputs.update(self._camera(B))
        if "s" in self.frame_idxs:
            sign = [(-1.0 if sd == "l" else 1.0) * (-1.0 if fl else 1.0) for sd, fl in zip(geo["side"], geo["flip"])]
            if any(v != -1.0 for v in sign):
                T = inputs["stereo_T"].clone()
                T[:, 0, 3] = to_device_async([0.1 * v for v in sign], dev, torch.float32)
                inputs["stereo_T"] = T
        return inputs

    def next_scenes(self, n):
        if self.scene_feed is None:
            raise RuntimeError("KITTIRAWDataset serves training items; the attack's scenes come from a KittiSceneFeed "
                               "(give --scene_root)")
        return self.scene_feed.next_scenes(n)

    def close(self):
        if self._prefetch is not None:
            self._prefetch.close()
            self._prefetch = None
        if self.scene_feed is not None:
            self.scene_feed.close()


class KittiSceneFeed(object):
    """The attack's scenes (dataLoader.py:107-209, KittiLoader in train mode at size (1242, 375)): the files of the list
    ``<scene_root>/<list_name>`` under ``<scene_root>/training/image_2`` (:75-88), cropped bottom-centre to 375 x 1242 (:185-189)
    and scaled as ``float32 / 256`` (:200 -- 256, not 255).  ``next_scenes(n)`` -> [n, 3, 375, 1242] on the device.  ``crop``: another (h, w), for tests on small frames."""

    def __init__(self, scene_root, device, list_name="vehicle_detection/training.txt", seed=1234, num_workers=12,
                 crop=(ori_H, ori_W)):
        self.root, self.device, self.crop = scene_root, torch.device(device), (int(crop[0]), int(crop[1]))
        path = os.path.join(scene_root, list_name)
        if not os.path.isfile(path):
            raise RuntimeError("scene list %s not found (--scene_root must hold %s and training/image_2)" % (path, list_name))
        with open(path) as f:
            names = [ln.split(" ")[0].rstrip() for ln in f.read().splitlines() if ln.strip()]
        if not names:
            raise RuntimeError("scene list %s is empty" % path)
        self.files = [os.path.join(scene_root, "training", "image_2", nm + ".png") for nm in names]
        self.rng = random.Random(seed)
        self.pool_workers = pool_workers(num_workers)
        self.workers = ThreadPoolExecutor(max_workers=self.pool_workers)
        self.loader = ThreadPoolExecutor(max_workers=1)
        self._pending = None             # (n, future of the next call's decoded scenes)
        self.wait_s = 0.0                # time the caller spent inside next_scenes

    def __len__(self):
        return len(self.files)

    def _decode(self, picks):
        return np.stack(list(self.workers.map(self.load, picks)))

    def _draw(self, n):
        return [self.files[self.rng.randrange(len(self.files))] for _ in range(n)]

    def close(self):
        self.loader.shutdown(wait=True)
        self.workers.shutdown(wait=True)

    def load(self, path):
        Image = _pil()
        with open(path, "rb") as f:
            with Image.open(f) as img:
                a = np.asarray(img.convert("RGB"))
        h, w = a.shape[:2]
        ch, cw = self.crop
        if h < ch or w < cw:
            raise RuntimeError("%s is %d x %d: smaller than the %d x %d crop" % (path, h, w, ch, cw))
        left, top = (w - cw) // 2, h - ch
        return np.ascontiguousarray(a[top:top + ch, left:left + cw])

    def next_scenes(self, n):
        t0 = time.perf_counter()
        if self._pending is not None and self._pending[0] == n:
            frames = self._pending[1].result()
        else:
            frames = self._decode(self._draw(n))
        # the next call's scenes are drawn now and decoded while the step runs (the attack asks for the same n every iteration)
        self._pending = (n, self.loader.submit(self._decode, self._draw(n)))
        u8 = to_device_async(frames, self.device)
        self.wait_s += time.perf_counter() - t0
        return (u8.permute(0, 3, 1, 2).float() / 256.0).contiguous()


def eval_frames(data_path, lines, height, width, device, img_ext=".jpg", batch_size=16, num_workers=12):
    """The test frames of ``evaluate_depth.evaluate`` (MD2/evaluate_depth.py:242-251: KITTIRAWDataset with frame id 0, four
    scales, is_train False): batches of ``batch_size`` files through K31, level 0 only, no flip -> float [n, 3, height, width]."""
    paths = [image_path(data_path, *parse_line(ln), img_ext=img_ext) for ln in lines]
    if any(parse_line(ln)[2] is None for ln in lines):
        raise RuntimeError("eval_frames: every test line needs a camera side")
    chunks = [paths[i:i + batch_size] for i in range(0, len(paths), batch_size)]
    pre = _Prefetcher(batch_size, device, pool_workers(num_workers))
    try:
        if chunks:
            pre.submit(0, chunks[0])
        for k, chunk in enumerate(chunks):
            raw, sizes = pre.take(k)
            if k + 1 < len(chunks):
                pre.submit(k + 1, chunks[k + 1])
            out = ops.pil_resize(raw, (height, width), "lanczos", None, tuple(sizes), want_u8=False).f32
            pre.release(k)
            yield out
    finally:
        pre.close()


def from_options(opt, device, rank=0):
    """The training set of ``--dataset kitti`` (MD2/trainer.py:162-181) and, under --adv_train, its scene feed.  What is not
    built raises here, where a user meets it."""
    if opt.dataset != "kitti":
        raise NotImplementedError("--dataset %s: only KITTI raw (kitti) is read from disk; kitti_odom, kitti_depth and "
                                  "kitti_test have no loader here" % opt.dataset)
    if opt.gt_depth:
        raise NotImplementedError("--gt_depth with --dataset kitti: the pseudo-depth term on depth_gt from velodyne points is "
                                  "not wired to this loader (depth_gt itself is built when the scans exist: load_depth)")
    lines = read_split(os.path.join(opt.split_dir, opt.split, "train_files.txt"))
    dataset = KITTIRAWDataset(opt.data_path, lines, opt.height, opt.width, opt.frame_ids, 4, device, is_train=True,
                              img_ext=".png" if opt.png else ".jpg", seed=opt.seed + rank, num_workers=opt.num_workers,
                              preprocess=opt.kitti_preprocess, color_aug=opt.contrastive_learning,
                              jitter=opt.kitti_jitter, use_depth_hints=opt.use_depth_hints, depth_hint_path=opt.depth_hint_path)
    if opt.adv_train:
        if not opt.scene_root:
            raise RuntimeError("--dataset kitti with --adv_train reads the attack's scenes from --scene_root")
        dataset.scene_feed = KittiSceneFeed(opt.scene_root, device, seed=opt.seed + rank, num_workers=opt.num_workers)
    return dataset
