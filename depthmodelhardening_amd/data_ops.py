"""The loader and preprocessing operators: the PIL-exact resize (K31), the velodyne depth maps (K32), the colour jitter (K33), the
depth hints (K34), the stereo matcher (K35) and the pseudo-LiDAR clouds (K39).  ops.py re-exports every name, and callers reach
them as ``ops.<name>``.

Each operator comes with a ``*_host`` function, the numpy restatement its kernel is held to bit for bit.  CPU tensors run that
restatement; tensors on the device launch the kernel.  The upload caches below are only ever mutated in place.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _native as N
from ._launch import _UploadCache, _c, _flip_operand, _need_i32, _timed


def _host_list(x):
    """A per-item host argument (sizes, shapes, offsets, flips) given as a tensor or an array: as the list it stands for."""
    return x.tolist() if hasattr(x, "tolist") else x


def _host_pairs(x):
    return tuple((int(h), int(w)) for h, w in _host_list(x))


def _host_flips(flip, n):
    """The per-item flips of a host restatement as a list of bools (None: nothing is flipped); the caller checks its length."""
    return [False] * n if flip is None else [bool(v) for v in np.asarray(_host_list(flip)).reshape(-1)]


# ----------------------------------------------------------------------------------------------------------------- K31
PIL_FILTERS = {"lanczos": (N.PIL_LANCZOS, 3.0), "bilinear": (N.PIL_BILINEAR, 1.0)}      # name -> (PIL's number, support)
PIL_PRECISION_BITS = 22
PIL_DESC_CACHE = 64         # descriptor sets kept per process (a few hundred bytes each); the tables themselves are never repeated
PilLevel = namedtuple("PilLevel", ["u8", "f32"])
_pil_axis_cache = {}
# (device, sizes, out, filter) -> descriptors on the device
_pil_device_cache = _UploadCache(PIL_DESC_CACHE, "pil_resize: the first call with these source sizes uploads their descriptors; "
                                                 "make it once before capturing a graph")
_pil_graph_keys = _pil_device_cache.held


def _pil_filter(filter):
    try:
        return PIL_FILTERS[str(filter).lower()]
    except KeyError:
        raise RuntimeError("pil_resize: filter must be one of %s; got %r" % (sorted(PIL_FILTERS), filter))


def _pil_weight(x, support):
    """Pillow's filter functions (Resample.c: bilinear_filter; lanczos_filter = sinc(x) sinc(x / 3) on [-3, 3)) on Python
    floats: ``math.sin`` is the C library's, as Pillow's is."""
    import math
    if support == 1.0:
        x = -x if x < 0.0 else x
        return 1.0 - x if x < 1.0 else 0.0
    if not -3.0 <= x < 3.0:
        return 0.0

    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / 3)


def pil_axis_table(in_size, out_size, filter="lanczos"):
    """Host: Pillow's coefficients of one axis (Resample.c precompute_coeffs + normalize_coeffs_8bpc) for ``in_size`` ->
    ``out_size``: (xmin int32 [out], count int32 [out], k int32 [out, ksize]).  float64 in Pillow's order -- the taps
    ``filter((x + xmin - center + 0.5) * (1 / filterscale))`` summed by index, each divided by the sum -- then integers with 22
    fraction bits, rounded half away from zero.  Equal sizes give the pass Pillow skips as the table (x, 1, 2^22).  Cached."""
    in_size, out_size = int(in_size), int(out_size)
    number, support0 = _pil_filter(filter)
    if not (0 < in_size < (1 << 20) and 0 < out_size < (1 << 20)):
        raise RuntimeError("pil_axis_table: sizes must be in [1, 2^20); got %d -> %d" % (in_size, out_size))
    key = (in_size, out_size, number)
    hit = _pil_axis_cache.get(key)
    if hit is not None:
        return hit
    if in_size == out_size:
        tab = (np.arange(out_size, dtype=np.int32), np.ones(out_size, dtype=np.int32),
               np.full((out_size, 1), 1 << PIL_PRECISION_BITS, dtype=np.int32))
    else:
        import math
        scale = in_size / out_size
        filterscale = max(scale, 1.0)
        support = support0 * filterscale
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / filterscale
        xmins, counts = np.zeros(out_size, dtype=np.int32), np.zeros(out_size, dtype=np.int32)
        k = np.zeros((out_size, ksize), dtype=np.int32)
        one = float(1 << PIL_PRECISION_BITS)
        for xx in range(out_size):
            center = (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), in_size) - xmin
            w = [_pil_weight((x + xmin - center + 0.5) * ss, support0) for x in range(xmax)]
            ww = 0.0
            for v in w:
                ww += v
            if ww != 0.0:
                w = [v / ww for v in w]
            xmins[xx], counts[xx] = xmin, xmax
            k[xx, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        tab = (xmins, counts, k)
    for a in tab:
        a.setflags(write=False)
    _pil_axis_cache[key] = tab
    return tab


def _pil_pass_host(a, table, sums=None):
    """One pass of Pillow's 8-bit resample along the last axis of uint8 ``a``: clip((2^21 + sum(p k)) >> 22, 0, 255) in int32.
    ``sums`` (a list) receives the sums before the shift and the clip."""
    xmin, count, k = table
    idx = np.minimum(xmin[:, None] + np.arange(k.shape[1])[None, :], a.shape[-1] - 1)      # taps past ``count`` weigh 0
    acc = (a[..., idx].astype(np.int32) * k).sum(-1, dtype=np.int32) + np.int32(1 << (PIL_PRECISION_BITS - 1))
    if sums is not None:
        sums.append(acc)
    return np.clip(acc >> PIL_PRECISION_BITS, 0, 255).astype(np.uint8)


def pil_quantize_host(x):
    """torchvision's ``ToPILImage`` on a float tensor: ``pic.mul(255).byte()``, a truncation in fp32."""
    return (np.asarray(x, dtype=np.float32) * np.float32(255.0)).astype(np.uint8)


def pil_resize_host(img, out_size, filter="lanczos", flip=False, sums=None):
    """Host twin of K31 in numpy: ``PIL.Image.fromarray(img).resize((out_w, out_h), filter)`` of uint8 ``img`` [..., H, W]
    (planar: leading axes are channels or a batch), bit-equal to Pillow's.  ``flip``: transpose(FLIP_LEFT_RIGHT) first.  The
    horizontal pass runs first into an 8-bit intermediate; a pass whose size does not change is skipped."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim < 2:
        raise RuntimeError("pil_resize_host: need a uint8 array [..., H, W]; got %s %s" % (img.dtype, img.shape))
    oh, ow = (int(v) for v in out_size)
    if flip:
        img = img[..., ::-1]
    H, W = img.shape[-2:]
    if W != ow:
        img = _pil_pass_host(img, pil_axis_table(W, ow, filter), sums)
    if H != oh:
        img = np.swapaxes(_pil_pass_host(np.swapaxes(img, -1, -2), pil_axis_table(H, oh, filter), sums), -1, -2)
    return np.ascontiguousarray(img)


class _PilArena(object):
    """The axis tables of one device: one int32 tensor that holds every distinct (in, out, filter) table once, at a word offset
    that never changes.  KITTI raw has about five frame sizes, so the arena stops growing after the first batches; when a new
    table arrives the whole arena is uploaded again (pinned, asynchronous) and the upload is waited for once, so that any stream
    may read it afterwards."""

    def __init__(self, device):
        self.device, self.entries, self.words, self.tables = device, {}, [], None
        self.tile_rows = {}

    def place(self, n_in, n_out, number, filter):
        """(word offset, ksize) of the table; ``self.tables`` is stale until ``sync`` when this added one."""
        key = (n_in, n_out, number)
        if key not in self.entries:
            xmin, count, k = pil_axis_table(n_in, n_out, filter)
            flat = np.concatenate([xmin, count, np.ascontiguousarray(k.T).reshape(-1)])
            want = N.lib().dmh_pil_resample_tables_size(n_in, n_out, number)
            if want != flat.size:
                raise RuntimeError("pil_resize: the table of %d -> %d has %d words, the library expects %d" % (n_in, n_out, flat.size, want))
            self.entries[key] = (sum(w.size for w in self.words), k.shape[1])
            self.words.append(flat)
            self.tables = None
        return self.entries[key]

    def rows(self, h, oh, filter, number):
        """The most source rows one tile of PIL_TILE_ROWS output rows needs on the vertical axis h -> oh."""
        key = (h, oh, number)
        if key not in self.tile_rows:
            tile = N.PIL_TILE_ROWS
            ymin, count, _ = pil_axis_table(h, oh, filter)
            last_i = np.minimum(np.arange(tile - 1, oh + tile - 1, tile), oh - 1)
            self.tile_rows[key] = int((ymin[last_i] + count[last_i] - ymin[::tile]).max())
        return self.tile_rows[key]

    def sync(self):
        if self.tables is None:
            host = torch.from_numpy(np.concatenate(self.words)).pin_memory()
            self.tables = host.to(self.device, non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.device))
            done.synchronize()          # once per new table: later calls, on any stream, read a finished upload
        return self.tables


_pil_arenas = {}


def _pil_tables_device(device, sizes, oh, ow, number, filter):
    """(tables int32 [words], desc int32 [N, 8], lds_rows) on ``device`` for a batch whose images have the source sizes
    ``sizes`` (a tuple of (h, w)).  The tables live once per distinct (in, out, filter) in the device's arena; what depends on
    the batch is the descriptor set alone (32 bytes per image), kept in ``_pil_device_cache``: a repeated batch shape -- a
    captured graph's, a pyramid's coarser levels -- launches with the same device buffer and no copy."""
    arena = _pil_arenas.get(str(device))
    if arena is None:
        arena = _pil_arenas[str(device)] = _PilArena(device)

    def make():
        desc, lds_rows = np.zeros((len(sizes), 8), dtype=np.int32), 1
        for i, (h, w) in enumerate(sizes):
            (ho, hk), (vo, vk) = arena.place(w, ow, number, filter), arena.place(h, oh, number, filter)
            desc[i, :6] = (h, w, ho, hk, vo, vk)
            lds_rows = max(lds_rows, arena.rows(h, oh, filter, number))
        if lds_rows * ow > 65536:
            raise RuntimeError("pil_resize: %d source rows of %d output columns per tile exceed the 64 KiB LDS tile; resize in two "
                               "steps" % (lds_rows, ow))
        return [torch.from_numpy(desc)], lds_rows
    (desc_d,), lds_rows = _pil_device_cache.get((str(device), sizes, oh, ow, number), device, make)
    return arena.sync(), desc_d, lds_rows


def _pil_sizes(sizes, n, H, W):
    if sizes is None:
        return ((H, W),) * n
    sizes = _host_pairs(sizes)
    if len(sizes) != n or not all(0 < h <= H and 0 < w <= W for h, w in sizes):
        raise RuntimeError("pil_resize: sizes must be %d pairs (h, w) within the buffer's %d x %d; got %s" % (n, H, W, sizes))
    return sizes


def pil_resize(src, out_size, filter="lanczos", flip=None, sizes=None, want_float=True, layout=None, want_u8=True):
    """K31: ``PIL.Image.resize((out_w, out_h), filter)`` of a batch of 8-bit images, bit for bit, in one launch.

    src      uint8 [N, H, W, C] (``layout="hwc"``, the default for uint8: decoded files), uint8 [N, C, H, W]
             (``layout="chw"``: a previous level), or float32 [N, C, H, W] in [0, 1], quantised on read as ToPILImage does.
    sizes    per image (h, w) <= (H, W): the image lies in the top-left corner of its slot (host values: they choose the tables).
    flip     per image, a device int32 [N] (or a host sequence of bools): != 0 resizes transpose(FLIP_LEFT_RIGHT) of the image.
    Returns  PilLevel(u8 uint8 [N, C, out_h, out_w] or None, f32 = u8.float() / 255 or None).

    CPU tensors run the numpy restatement of the same integers (``pil_resize_host``)."""
    number, _ = _pil_filter(filter)
    oh, ow = (int(v) for v in out_size)
    if oh < 1 or ow < 1:
        raise RuntimeError("pil_resize: out_size must be positive; got %s" % (tuple(out_size),))
    if src.dim() != 4 or src.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError("pil_resize: src must be uint8 or float32 with 4 dimensions; got %s %s" % (src.dtype, tuple(src.shape)))
    if not (want_float or want_u8):
        raise RuntimeError("pil_resize: nothing to return (want_float and want_u8 are both off)")
    layout = layout or ("hwc" if src.dtype == torch.uint8 else "chw")
    if layout not in ("hwc", "chw") or (src.dtype == torch.float32 and layout != "chw"):
        raise RuntimeError("pil_resize: layout must be 'hwc' or 'chw' (float32 sources are 'chw'); got %r" % (layout,))
    n, (H, W, C_) = int(src.shape[0]), ((int(v) for v in src.shape[1:]) if layout == "hwc" else (int(src.shape[2]), int(src.shape[3]), int(src.shape[1])))
    sizes = _pil_sizes(sizes, n, H, W)
    if src.device.type != "cuda":
        planar = src.permute(0, 3, 1, 2) if layout == "hwc" else src
        planar = planar.numpy() if src.dtype == torch.uint8 else pil_quantize_host(planar.numpy())
        flips = _host_flips(flip, n)
        if len(flips) != n:
            raise RuntimeError("pil_resize: flip must have one entry per image")
        u8 = torch.from_numpy(np.stack([pil_resize_host(planar[i, :, :h, :w], (oh, ow), filter, flips[i])
                                        for i, (h, w) in enumerate(sizes)]))
        return PilLevel(u8 if want_u8 else None, u8.float().div(255) if want_float else None)
    src = _c(src)
    dev = src.device
    flip = _flip_operand("pil_resize", flip, n, dev)
    tables, desc, lds_rows = _pil_tables_device(dev, sizes, oh, ow, number, filter)
    u8 = torch.empty((n, C_, oh, ow), device=dev, dtype=torch.uint8) if want_u8 else None
    f32 = torch.empty((n, C_, oh, ow), device=dev, dtype=torch.float32) if want_float else None
    strides = (H * W * C_, 1, W * C_, C_) if layout == "hwc" else (C_ * H * W, H * W, W, 1)
    N.check(_timed("pil_resample", lambda: N.lib().dmh_pil_resample(
        N.ptr(src), int(src.dtype == torch.float32), *strides, H, W, N.ptr(tables), int(tables.numel()), N.ptr(desc),
        N.ptr(flip), n, C_, oh, ow, lds_rows, N.ptr(u8), N.ptr(f32), N.stream()),
        src.numel() * src.element_size() + n * C_ * oh * ow * (int(want_u8) + 4 * int(want_float))))
    return PilLevel(u8, f32)


def pil_pyramid(src, height, width, num_scales=4, filter="lanczos", flip=None, sizes=None, want_float=True, layout=None):
    """The loader's image pyramid (MD2/datasets/mono_dataset.py:100-104,119-144): level 0 is ``src`` resized to height x width,
    level i the 8-bit level i - 1 resized to (height // 2^i) x (width // 2^i) -- one launch of K31 per level.  ``flip`` applies to
    level 0 (the reference flips the loaded image).  Returns ``num_scales`` PilLevel(u8, f32)."""
    levels = []
    for i in range(int(num_scales)):
        s = 2 ** i
        if height // s < 1 or width // s < 1:
            raise RuntimeError("pil_pyramid: level %d of %d x %d is empty" % (i, height, width))
        if i == 0:
            levels.append(pil_resize(src, (height, width), filter, flip, sizes, want_float, layout))
        else:
            levels.append(pil_resize(levels[-1].u8, (height // s, width // s), filter, None, None, want_float, "chw"))
    return levels


# ---------------------------------------------------------------------------------------------------------------- K32
VELO_EMPTY, VELO_DESC_CACHE = 0xFFFFFFFF, 16
_velo_desc_cache = _UploadCache(VELO_DESC_CACHE, "velo_depth_map: the first call with these shapes uploads their descriptors; make "
                                                 "it once before capturing a graph")     # (device, shapes) -> descriptors


def nearest_index(n_in, n_out):
    """Source index of every output index of K32's nearest resize: ((2 o + 1) n_in) // (2 n_out), the exact-arithmetic value of
    the pixel-centre mapping round((o + 0.5) n_in / n_out - 0.5); the identity when the sizes agree."""
    o = np.arange(int(n_out), dtype=np.int64)
    return ((2 * o + 1) * int(n_in)) // (2 * int(n_out))


def _velo_shapes(shapes, n):
    shapes = _host_pairs(shapes)
    if len(shapes) != n or not all(h >= 1 and w >= 2 for h, w in shapes):
        raise RuntimeError("velo_depth_map: shapes must be %d pairs (H, W) with H >= 1 and W >= 2; got %s" % (n, shapes))
    return shapes


def _velo_frame_host(pts, P, H, W, vel_depth):
    """One frame of K32 in numpy -> float32 [H, W]: the kernel's arithmetic in the kernel's order (csrc/velo_depth.hip)."""
    idx = np.nonzero(pts[:, 0] >= 0)[0]                     # a NaN fails the test
    x, y, z = (pts[idx, c].astype(np.float64) for c in range(3))
    with np.errstate(all="ignore"):
        q = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]
        u, v = np.rint(q[0] / q[2]) - 1.0, np.rint(q[1] / q[2]) - 1.0
        keep = (u >= 0) & (v >= 0) & (u < W) & (v < H)      # NaN and inf fall out
        d = (x if vel_depth else q[2])[keep]
        val = np.where(d > 0, d, 0.0).astype(np.float32)    # float32(max(d, 0)); rounding and the clamp are monotone
    idx, ui, vi = idx[keep], u[keep].astype(np.int64), v[keep].astype(np.int64)
    if idx.size == 0:
        return np.zeros((H, W), dtype=np.float32)
    bits = val.view(np.uint32)                             # non-negative floats order as their bits do
    cells = np.full(H * W, VELO_EMPTY, dtype=np.uint32)
    np.minimum.at(cells, vi * W + ui, bits)
    out = np.where(cells == VELO_EMPTY, np.uint32(0), cells).reshape(H, W)
    if H > 1:
        # the reference's sub2ind gives A = (y, W - 1) and B = (y + 1, 0) one key: where both hold points, the one that holds the
        # pair's earliest point gets the minimum over both, the other keeps its last point's value
        first = np.full((H, 2), np.iinfo(np.int64).max, dtype=np.int64)
        last = np.full((H, 2), -1, dtype=np.int64)
        for side, col in ((0, 0), (1, W - 1)):
            on = ui == col
            np.minimum.at(first[:, side], vi[on], idx[on])
            np.maximum.at(last[:, side], vi[on], idx[on])
        cells = cells.reshape(H, W)
        a, b = cells[:-1, W - 1], cells[1:, 0]
        both = (a != VELO_EMPTY) & (b != VELO_EMPTY)
        a_first = first[:-1, 1] < first[1:, 0]
        low = np.minimum(a, b)
        pos = np.full(pts.shape[0], -1, dtype=np.int64)
        pos[idx] = np.arange(idx.size)
        last_a, last_b = bits[pos[np.maximum(last[:-1, 1], 0)]], bits[pos[np.maximum(last[1:, 0], 0)]]
        out[:-1, W - 1] = np.where(both, np.where(a_first, low, last_a), out[:-1, W - 1])
        out[1:, 0] = np.where(both, np.where(a_first, last_b, low), out[1:, 0])
    return out.view(np.float32)


def velo_depth_map_host(points, offsets, proj, shapes, vel_depth=False, out_size=None, flip=None):
    """K32 in numpy, the definition the kernel is held to (and the path CPU tensors take): vectorised, no loop per duplicate.
    points float32 [npts, 4], offsets [n + 1], proj float64 [n, 3, 4] or [n, 12], shapes n pairs (H, W).  Returns float32
    [n, out_h, out_w] with ``out_size``, else the list of the n maps at their own sizes."""
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
    offsets = [int(v) for v in np.asarray(offsets).reshape(-1)]
    n = len(offsets) - 1
    proj = np.asarray(proj, dtype=np.float64).reshape(n, 3, 4)
    shapes = _velo_shapes(shapes, n)
    flips = _host_flips(flip, n)
    if len(flips) != n:
        raise RuntimeError("velo_depth_map: flip must have one entry per frame")
    if offsets[0] < 0 or offsets[-1] > points.shape[0] or any(a > b for a, b in zip(offsets[:-1], offsets[1:])):
        raise RuntimeError("velo_depth_map: offsets must ascend within the %d points; got %s" % (points.shape[0], offsets))
    maps = []
    for f, (H, W) in enumerate(shapes):
        m = _velo_frame_host(points[offsets[f]:offsets[f + 1]], proj[f], H, W, bool(vel_depth))
        if out_size is not None:
            m = m[nearest_index(H, out_size[0])][:, nearest_index(W, out_size[1])]
        maps.append(np.ascontiguousarray(m[:, ::-1] if flips[f] else m))
    return np.stack(maps) if out_size is not None else maps


def _velo_desc_device(device, shapes):
    def make():
        cells = np.cumsum([0] + [h * w for h, w in shapes])
        rows = np.cumsum([0] + [h for h, _ in shapes])
        return [torch.tensor([[h, w, int(cells[i]), int(rows[i])] for i, (h, w) in enumerate(shapes)], dtype=torch.int32)], None
    return _velo_desc_cache.get((str(device), shapes), device, make)[0][0]


def velo_depth_map(points, offsets, proj, shapes, vel_depth=False, out_size=None, flip=None):
    """K32: the sparse depth maps of a batch of velodyne scans (MD2/kitti_utils.py:46-98, generate_depth_map, float32-equal),
    with the loader's nearest resize and flip (MD2/datasets/kitti_dataset.py:70-85).

    points   float32 [npts, 4], the frames' points packed in file order; offsets int32 [n + 1] on the same device.
    proj     float64 [n, 3, 4] (or [n, 12]): P_velo2im of each frame (datasets.kitti_velo.velo_projection).
    shapes   n pairs (H, W): each frame's image size.  Host values: they size the workspace and the output.
    flip     per frame, an int32 tensor [n] on the device (or a host sequence of bools): != 0 mirrors the columns.
    Returns  float32 [n, out_h, out_w] with ``out_size``; without it (flat float32 [sum H W], cell offsets as a list of n + 1
             ints): frame f is flat[off[f]:off[f + 1]].view(H, W).

    CPU tensors run ``velo_depth_map_host``, the numpy restatement the kernel is bit-equal to."""
    if not torch.is_tensor(points) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 4:
        raise RuntimeError("velo_depth_map: points must be a float32 tensor [npts, 4]; got %s %s"
                           % (getattr(points, "dtype", type(points)), tuple(getattr(points, "shape", ()))))
    _need_i32(offsets, "offsets")
    n = offsets.numel() - 1
    if offsets.dim() != 1 or n < 1:
        raise RuntimeError("velo_depth_map: offsets must hold n + 1 >= 2 entries; got %s" % (tuple(offsets.shape),))
    if not torch.is_tensor(proj) or proj.dtype != torch.float64 or proj.numel() != 12 * n:
        raise RuntimeError("velo_depth_map: proj must be a float64 tensor of %d x 12 entries; got %s %s"
                           % (n, getattr(proj, "dtype", type(proj)), tuple(getattr(proj, "shape", ()))))
    shapes = _velo_shapes(shapes, n)
    if out_size is not None:
        out_size = tuple(int(v) for v in out_size)
        if len(out_size) != 2 or out_size[0] < 1 or out_size[1] < 1:
            raise RuntimeError("velo_depth_map: out_size must be a positive (h, w); got %s" % (out_size,))
    cell_off = [int(v) for v in np.cumsum([0] + [h * w for h, w in shapes])]
    dev = points.device
    if offsets.device != dev or proj.device != dev:
        raise RuntimeError("velo_depth_map: points, offsets and proj must share a device")
    if dev.type != "cuda":
        res = velo_depth_map_host(points.numpy(), offsets.numpy(), proj.numpy(), shapes, vel_depth, out_size, flip)
        if out_size is not None:
            return torch.from_numpy(res)
        return torch.from_numpy(np.concatenate([m.reshape(-1) for m in res])), cell_off
    flip = _flip_operand("velo_depth_map", flip, n, dev)
    lib = N.lib()
    total_cells, total_rows = cell_off[-1], sum(h for h, _ in shapes)
    words = lib.dmh_velo_depth_ws_size(total_cells, total_rows)
    if words < 0:
        raise RuntimeError("velo_depth_map: %d cells and %d rows do not fit a 2^31-word workspace" % (total_cells, total_rows))
    desc = _velo_desc_device(dev, shapes)
    ws = torch.empty(words, device=dev, dtype=torch.int32)
    out = torch.empty((n,) + out_size if out_size is not None else (total_cells,), device=dev, dtype=torch.float32)
    points, proj = _c(points), _c(proj)
    oh, ow = out_size if out_size is not None else (0, 0)
    N.check(_timed("velo_depth_map", lambda: lib.dmh_velo_depth_map(
        N.ptr(points) if points.numel() else None, int(points.shape[0]), N.ptr(_c(offsets)), N.ptr_f64(proj), N.ptr(desc),
        N.ptr(flip), n, int(bool(vel_depth)), total_cells, total_rows, oh, ow, N.ptr(ws), N.ptr(out),
        N.stream()), points.numel() * 4 + 8 * words + out.numel() * 4))
    return out if out_size is not None else (out, cell_off)


# ---------------------------------------------------------------------------------------------------------------- K33
JITTER_MAX_TENSORS = 8                  # DMH_JITTER_MAX_TENSORS
JITTER_MAX_PIXELS = (2 ** 32 - 1) // 255  # 255 H W must fit the 32-bit sum of L


def _jitter_L(img):
    """Pillow's ``convert("L")`` of uint8 [3, H, W] -> int32 [H, W]."""
    r, g, b = (img[c].astype(np.int32) for c in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16


def _jitter_blend(deg, img, f):
    """``Image.blend(degenerate, image, f)`` per channel: float32, the product and the sum rounded separately; truncated to a byte
    for 0 <= f <= 1, clipped outside."""
    f = np.float32(f)
    d = np.asarray(deg).astype(np.float32)
    t = d + f * (img.astype(np.float32) - d)
    if np.float32(0) <= f <= np.float32(1):
        return t.astype(np.int32).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def _jitter_hue(img, shift):
    """``convert("HSV")``, the shift added to the H byte modulo 256, ``convert("RGB")`` (Pillow's Convert.c rgb2hsv / hsv2rgb)."""
    r, g, b = (img[c].astype(np.int32) for c in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    flat = mx == mn
    cr = np.where(flat, 1, mx - mn).astype(np.float32)
    s = cr / np.where(flat, 1, mx).astype(np.float32)
    rc, gc, bc = ((mx - c).astype(np.float32) / cr for c in (r, g, b))
    rc64, gc64, bc64 = (c.astype(np.float64) for c in (rc, gc, bc))
    h = np.where(r == mx, bc64 - gc64, np.where(g == mx, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(np.float32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    H = np.where(flat, 0, np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255))
    S = np.where(flat, 0, np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255))
    V = mx
    H = (H + int(shift)) & 255
    fs = S / 255.0
    x = H * 6.0 / 255.0
    i = np.floor(x)
    fr = x - i

    def byte(z):        # C's round (half away from zero; z >= 0 here), then CLIP8
        return np.clip(np.floor(z + 0.5), 0, 255).astype(np.int32)
    p, q, t = byte(V * (1.0 - fs)), byte(V * (1.0 - fs * fr)), byte(V * (1.0 - fs * (1.0 - fr)))
    k = i.astype(np.int32) % 6
    grey = S == 0
    out = [np.where(grey, V, np.choose(k, table)) for table in ((V, q, p, p, t, V), (t, V, V, q, p, p), (p, p, t, V, V, q))]
    return np.stack(out).astype(np.uint8)


def pil_color_jitter_host(images, records, sums=None):
    """Host twin of K33 in numpy, bit-equal to Pillow: torchvision 0.8.2's ColorJitter on 8-bit PIL images.  ``images``: uint8
    arrays [B, 3, H, W]; ``records``: int32 [B, 8] (color_jitter.pil_records).  Every operation ends in a byte: brightness =
    blend(0, img, f), saturation = blend(L(img), img, f), contrast = blend(m, img, f) with m = int(mean of L over this image as the
    operations before left it + 0.5), hue = the HSV round trip with the shifted H byte.  Returns the uint8 results; ``sums`` (a
    list) receives the integer sum of L of every image that took a contrast step."""
    records = np.asarray(records, dtype=np.int32).reshape(-1, 8)
    out = []
    for img in images:
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 4 or img.shape[1] != 3 or img.shape[0] != records.shape[0]:
            raise RuntimeError("pil_color_jitter_host: need uint8 arrays [%d, 3, H, W]; got %s %s" % (records.shape[0], img.dtype, img.shape))
        res = np.empty_like(img)
        for i, rec in enumerate(records):
            x = img[i]
            factors = rec[2:5].view(np.float32)
            seen_contrast = False
            for k in range(min(max(int(rec[0]), 0), 4)):
                op = (int(rec[1]) >> (8 * k)) & 255
                if op == 0:
                    x = _jitter_blend(0, x, factors[0])
                elif op == 1:
                    L = _jitter_L(x)
                    S = int(L.sum(dtype=np.int64))
                    if sums is not None and not seen_contrast:
                        sums.append(S)
                    seen_contrast = True
                    x = _jitter_blend(int(S / float(L.size) + 0.5), x, factors[1])
                elif op == 2:
                    x = _jitter_blend(_jitter_L(x)[None], x, factors[2])
                elif op == 3:
                    x = _jitter_hue(x, int(rec[5]) & 255)
            res[i] = x
        out.append(res)
    return out


def pil_color_jitter(images, params, want_u8=False):
    """K33: torchvision 0.8.2's ``ColorJitter`` on 8-bit PIL images (MD2/datasets/mono_dataset.py:344-348, :133, :144), Pillow's
    bytes, for a whole batch and all its keys in two launches (one when no item has a contrast step).

    images   a list of at most 8 uint8 tensors [B, 3, H, W] on one device (K31's level-0 ``u8``): item i of every tensor takes
             transform i; every image has its own contrast mean.
    params   a list of B ``color_jitter.JitterParams`` or None (None: the item is only converted), or the prepared int32 record
             [B, 8] on the images' device (``color_jitter.pil_records``; a captured graph reads it at every replay).
    Returns  a list of PilLevel(u8 or None, f32 = u8.float() / 255), one per tensor.

    CPU tensors run ``pil_color_jitter_host``, the numpy restatement the kernel is bit-equal to."""
    from . import color_jitter
    from .my_utils import to_device_async
    images = list(images)
    if not 1 <= len(images) <= JITTER_MAX_TENSORS:
        raise RuntimeError("pil_color_jitter: one call takes 1 .. %d tensors; got %d" % (JITTER_MAX_TENSORS, len(images)))
    first = images[0]
    for t in images:
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[1] != 3 or t.shape != first.shape or t.device != first.device:
            raise RuntimeError("pil_color_jitter: images must be uint8 tensors [B, 3, H, W] of one shape on one device; got %s %s"
                               % (getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
    B, _, H, W = (int(v) for v in first.shape)
    if B < 1 or H < 1 or W < 1 or H * W > JITTER_MAX_PIXELS:
        raise RuntimeError("pil_color_jitter: need a non-empty batch of images of at most %d pixels (255 H W must fit 32 bits); "
                           "got %d x %d x %d" % (JITTER_MAX_PIXELS, B, H, W))
    dev = first.device
    if torch.is_tensor(params):
        if params.dtype != torch.int32 or params.numel() != 8 * B or params.device != dev:
            raise RuntimeError("pil_color_jitter: a prepared record is an int32 tensor [%d, 8] on %s" % (B, dev))
        rec, with_contrast = params, True
    else:
        host = color_jitter.pil_records(params)
        if host.shape[0] != B:
            raise RuntimeError("pil_color_jitter: params must hold one entry per item (%d); got %d" % (B, host.shape[0]))
        with_contrast = bool(color_jitter.records_have_contrast(host))
        rec = host if dev.type != "cuda" else to_device_async(host, dev)
    if dev.type != "cuda":
        res = [torch.from_numpy(a) for a in pil_color_jitter_host([t.numpy() for t in images], rec.numpy() if torch.is_tensor(rec) else rec)]
        return [PilLevel(u8 if want_u8 else None, u8.float().div(255)) for u8 in res]
    images = [_c(t) for t in images]
    rec = _c(rec)
    f32 = [torch.empty((B, 3, H, W), device=dev, dtype=torch.float32) for _ in images]
    u8 = [torch.empty((B, 3, H, W), device=dev, dtype=torch.uint8) for _ in images] if want_u8 else None
    T = len(images)
    words = N.lib().dmh_color_jitter_ws_size(T, B, H, W)
    if words < 0:
        raise RuntimeError("pil_color_jitter: %d tensors of %d x 3 x %d x %d are more than one call takes (T B <= 65535, "
                           "B 3 H W < 2^31)" % (T, B, H, W))
    ws = torch.empty(words, device=dev, dtype=torch.int32) if with_contrast else None
    N.check(_timed("color_jitter", lambda: N.lib().dmh_color_jitter(
        N.ptr_array(images, JITTER_MAX_TENSORS), N.ptr_array(f32, JITTER_MAX_TENSORS),
        N.ptr_array(u8, JITTER_MAX_TENSORS) if want_u8 else None, T, B, H, W, N.ptr(rec), int(with_contrast), N.ptr(ws), N.stream()),
        T * B * H * W * 3 * (1 + 4 + int(want_u8)) + (T * B * H * W * 3 if with_contrast else 0)))
    return [PilLevel(u8[i] if want_u8 else None, f32[i]) for i in range(T)]


# ---------------------------------------------------------------------------------------------------------------- K34
HINT_MAX_CANDIDATES = 16
HINT_TABLE_CACHE = 8
_hint_table_cache = _UploadCache(HINT_TABLE_CACHE, "depth_hint_prepare: the first call with these sizes uploads their index tables; "
                                                   "make it once before capturing a graph")     # (device, Hs, Ws, H, W) -> (ytab, xtab)


def hint_candidate_depths(cand, K):
    """depth-hints/precompute_depth_hints.py:142,151 for a batch: StereoSGBM's int16 output [B, N, H, W] (disparity x 16, -16 where
    nothing matched) -> float32 depths, fx 0.1 / (disp + 1e-7) * (disp > 0) with fx = K[b, 0, 0], as torch computes it on the CPU."""
    disps = torch.from_numpy(cand.cpu().numpy() / 16).float()
    fx = K.detach().cpu().float()[:, 0, 0].view(-1, 1, 1, 1)
    return fx * 0.1 / (disps + 1e-7) * (disps > 0).float()


def _hint_check(base, lookup, cand, K, inv_K, T):
    if not (torch.is_tensor(base) and base.dtype == torch.uint8 and base.dim() == 4 and base.shape[1] == 3):
        raise RuntimeError("depth_hint_fuse: base must be a uint8 tensor [B, 3, H, W]; got %s %s"
                           % (getattr(base, "dtype", type(base)), tuple(getattr(base, "shape", ()))))
    B, _, H, W = (int(v) for v in base.shape)
    if not (torch.is_tensor(lookup) and lookup.dtype == torch.uint8 and lookup.shape == base.shape):
        raise RuntimeError("depth_hint_fuse: lookup must be a uint8 tensor of base's shape %s; got %s %s"
                           % (tuple(base.shape), getattr(lookup, "dtype", type(lookup)), tuple(getattr(lookup, "shape", ()))))
    if not (torch.is_tensor(cand) and cand.dtype in (torch.int16, torch.float32) and cand.dim() == 4 and cand.shape[0] == B
            and tuple(cand.shape[2:]) == (H, W)):
        raise RuntimeError("depth_hint_fuse: cand must be int16 (disparity x 16) or float32 (depths) [%d, N, %d, %d]; got %s %s"
                           % (B, H, W, getattr(cand, "dtype", type(cand)), tuple(getattr(cand, "shape", ()))))
    n = int(cand.shape[1])
    if not 1 <= n <= HINT_MAX_CANDIDATES:
        raise RuntimeError("depth_hint_fuse: 1 <= N <= %d candidates; got %d" % (HINT_MAX_CANDIDATES, n))
    if B < 1 or H < 2 or W < 2:
        raise RuntimeError("depth_hint_fuse: need B >= 1 and H, W >= 2; got %d x %d x %d" % (B, H, W))
    for name, m in (("K", K), ("inv_K", inv_K), ("T", T)):
        if not (torch.is_tensor(m) and m.dtype == torch.float32 and tuple(m.shape) == (B, 4, 4)):
            raise RuntimeError("depth_hint_fuse: %s must be a float32 tensor [%d, 4, 4]; got %s %s"
                               % (name, B, getattr(m, "dtype", type(m)), tuple(getattr(m, "shape", ()))))
    for t in (lookup, cand, K, inv_K, T):
        if t.device != base.device:
            raise RuntimeError("depth_hint_fuse: every operand must be on base's device %s; got %s" % (base.device, t.device))
    return B, n, H, W


def _hint_ssim(x, y):
    """depth-hints/layers.py SSIM.forward."""
    import torch.nn.functional as F
    x, y = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    mu_x, mu_y = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
    sigma_x = F.avg_pool2d(x ** 2, 3, 1) - mu_x ** 2
    sigma_y = F.avg_pool2d(y ** 2, 3, 1) - mu_y ** 2
    sigma_xy = F.avg_pool2d(x * y, 3, 1) - mu_x * mu_y
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    n = (2 * mu_x * mu_y + C1) * (2 * sigma_xy + C2)
    d = (mu_x ** 2 + mu_y ** 2 + C1) * (sigma_x + sigma_y + C2)
    return torch.clamp((1 - n / d) / 2, 0, 1)


def depth_hint_fuse_host(base, lookup, cand, K, inv_K, T, want_losses=False, dtype=torch.float32):
    """K34 in plain torch on the CPU, the definition the kernel is held to (and the path CPU tensors take): the lines
    precompute_depth_hints.py:247-252 with BackprojectDepth, Project3D and SSIM of depth-hints/layers.py, item by item with the
    candidates as the batch.  The candidate depths are float32 in every form (they are inputs: ``hint_candidate_depths`` for
    int16); ``dtype=torch.float64`` computes everything after them in float64: the anchor.  Returns best_depth float32
    [B, 1, H, W], with ``want_losses`` (best_depth, losses ``dtype`` [B, N, H, W])."""
    import torch.nn.functional as F
    B, n, H, W = _hint_check(base, lookup, cand, K, inv_K, T)
    depths = hint_candidate_depths(cand, K) if cand.dtype == torch.int16 else cand.detach().cpu()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=dtype)], 0).unsqueeze(0)     # [1, 3, HW]
    ones = torch.ones(n, 1, H * W, dtype=dtype)
    best, losses = [], []
    for b in range(B):
        Kb, iKb, Tb = (m[b:b + 1].detach().cpu().to(dtype) for m in (K, inv_K, T))
        d = depths[b].to(dtype)
        cam = torch.matmul(iKb[:, :3, :3], pix)
        cam = torch.cat([d.reshape(n, 1, -1) * cam, ones], 1)
        P = torch.matmul(Kb, Tb)[:, :3, :]
        cp = torch.matmul(P, cam)
        pc = cp[:, :2, :] / (cp[:, 2, :].unsqueeze(1) + 1e-7)
        pc = pc.view(n, 2, H, W).permute(0, 2, 3, 1)
        pc[..., 0] /= W - 1
        pc[..., 1] /= H - 1
        pc = (pc - 0.5) * 2
        img_l = (lookup[b:b + 1].cpu().to(dtype) / 255).expand(n, -1, -1, -1)
        img_b = (base[b:b + 1].cpu().to(dtype) / 255).expand(n, -1, -1, -1)
        sample = F.grid_sample(img_l, pc, padding_mode="border", align_corners=False)
        l1 = torch.abs(img_b - sample).mean(1, True)
        loss = 0.85 * _hint_ssim(sample, img_b).mean(1, True) + 0.15 * l1
        index = torch.argmin(loss, dim=0)
        best.append(torch.gather(depths[b].unsqueeze(1), 0, index.unsqueeze(0))[0])
        losses.append(loss[:, 0])
    best = torch.stack(best).float()
    return (best, torch.stack(losses)) if want_losses else best


def depth_hint_fuse(base, lookup, cand, K, inv_K, T, want_losses=False):
    """K34: DepthHints' fused hint selection (depth-hints/precompute_depth_hints.py:247-252) for a batch of stereo pairs in one
    launch: per candidate depth map the other view warped into the base view (grid_sample's defaults, border padding), SSIM + L1
    against the base image, the lowest loss per pixel (the lowest index among equal float32 losses), its depth.

    base, lookup  uint8 [B, 3, H, W] (``pil_resize(..., want_u8=True).u8``): the view the hint is for, and the other one.
    cand          int16 [B, N, H, W]: StereoSGBM's raw output (disparity x 16, -16 = no match), converted as the reference does;
                  or float32 [B, N, H, W]: depths.  1 <= N <= 16.
    K, inv_K, T   float32 [B, 4, 4]; T[b, 0, 3] = -0.1 for a left base image, +0.1 for a right one.
    Returns       best_depth float32 [B, 1, H, W]; with ``want_losses`` (best_depth, losses float32 [B, N, H, W]).

    CPU tensors run ``depth_hint_fuse_host``."""
    B, n, H, W = _hint_check(base, lookup, cand, K, inv_K, T)
    if base.device.type != "cuda":
        return depth_hint_fuse_host(base, lookup, cand, K, inv_K, T, want_losses)
    if B * n * H * W >= 2 ** 31 or B > 65535:
        raise RuntimeError("depth_hint_fuse: B N H W must stay below 2^31 and B below 65536; got %d x %d x %d x %d" % (B, n, H, W))
    base, lookup, cand, K, inv_K, T = (_c(t) for t in (base, lookup, cand, K, inv_K, T))
    best = torch.empty((B, 1, H, W), device=base.device, dtype=torch.float32)
    losses = torch.empty((B, n, H, W), device=base.device, dtype=torch.float32) if want_losses else None
    raw = cand.dtype == torch.int16
    N.check(_timed("depth_hint_fuse", lambda: N.lib().dmh_depth_hint_fuse(
        N.ptr(base), N.ptr(lookup), C.c_void_p(cand.data_ptr()), int(raw), N.ptr(K), N.ptr(inv_K), N.ptr(T), B, n, H, W, N.ptr(best),
        N.ptr(losses), N.stream()), B * H * W * (6 + n * (2 if raw else 4) + 4 + (4 * n if want_losses else 0))))
    return (best, losses) if want_losses else best


def cv_nearest_index(n_src, n_dst):
    """Source index of every destination index of OpenCV's INTER_NEAREST along one axis, as its source states it (resizeNN:
    min(floor(dst * (double)src / dst_size), src - 1)); the identity when the sizes agree."""
    scale = float(int(n_src)) / float(int(n_dst))
    return np.minimum(np.floor(np.arange(int(n_dst), dtype=np.float64) * scale).astype(np.int64), int(n_src) - 1)


def _hint_prepare_check(hints, flip, out_size):
    if not (torch.is_tensor(hints) and hints.dtype == torch.float32 and hints.dim() == 4 and hints.shape[1] == 1 and hints.numel() > 0):
        raise RuntimeError("depth_hint_prepare: hints must be a non-empty float32 tensor [B, 1, Hs, Ws]; got %s %s"
                           % (getattr(hints, "dtype", type(hints)), tuple(getattr(hints, "shape", ()))))
    out_size = tuple(int(v) for v in out_size)
    if len(out_size) != 2 or out_size[0] < 1 or out_size[1] < 1:
        raise RuntimeError("depth_hint_prepare: out_size must be a positive (h, w); got %s" % (out_size,))
    B = int(hints.shape[0])
    if flip is not None:
        n = flip.numel() if torch.is_tensor(flip) else len(flip)
        if n != B:
            raise RuntimeError("depth_hint_prepare: flip must have one entry per item (%d); got %d" % (B, n))
    return B, int(hints.shape[2]), int(hints.shape[3]), out_size[0], out_size[1]


def depth_hint_prepare_host(hints, flip, out_size):
    """depth-hints/datasets/mono_dataset.py:382-388 for a batch in numpy: np.fliplr of the flipped items, OpenCV's INTER_NEAREST
    to ``out_size`` (``cv_nearest_index``), the mask (hint > 0).  Returns (depth_hint, depth_hint_mask) float32 [B, 1, H, W]."""
    B, Hs, Ws, H, W = _hint_prepare_check(hints, flip, out_size)
    src = hints.detach().cpu().numpy()
    flips = _host_flips(flip, B)
    yi, xi = cv_nearest_index(Hs, H), cv_nearest_index(Ws, W)
    out = np.empty((B, 1, H, W), dtype=np.float32)
    for b in range(B):
        a = np.fliplr(src[b, 0]) if flips[b] else src[b, 0]
        out[b, 0] = a[yi][:, xi]
    hint = torch.from_numpy(out)
    return hint, (hint > 0).float()


def _hint_tables_device(device, Hs, Ws, H, W):
    def make():
        return [torch.from_numpy(cv_nearest_index(a, b).astype(np.int32)) for a, b in ((Hs, H), (Ws, W))], None
    return _hint_table_cache.get((str(device), Hs, Ws, H, W), device, make)[0]


def depth_hint_prepare(hints, flip, out_size):
    """The loader's side of a stored depth hint (depth-hints/datasets/mono_dataset.py:382-388) for a batch in one launch.

    hints     float32 [B, 1, Hs, Ws]: the loaded ``.npy`` files.
    flip      None, an int32 tensor [B] on the hints' device, or a host sequence of bools: != 0 is np.fliplr before the resize.
    out_size  (H, W): cv2.resize(..., INTER_NEAREST) to it; at Hs, Ws == H, W a (mirrored) copy.
    Returns   (depth_hint, depth_hint_mask = (depth_hint > 0).float()), float32 [B, 1, H, W].

    CPU tensors run ``depth_hint_prepare_host``."""
    B, Hs, Ws, H, W = _hint_prepare_check(hints, flip, out_size)
    dev = hints.device
    if dev.type != "cuda":
        return depth_hint_prepare_host(hints, flip, out_size)
    flip = _flip_operand("depth_hint_prepare", flip, B, dev)
    ytab, xtab = _hint_tables_device(dev, Hs, Ws, H, W)
    hints = _c(hints)
    hint = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    mask = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    N.check(_timed("depth_hint_prepare", lambda: N.lib().dmh_depth_hint_prepare(
        N.ptr(hints), N.ptr(flip), N.ptr(ytab), N.ptr(xtab), H, W, B, Hs, Ws, H, W, N.ptr(hint),
        N.ptr(mask), N.stream()), B * H * W * 12))
    return hint, mask


# ---------------------------------------------------------------------------------------------------------------- K35
SGM_MAX_MATCHERS = 16
SGM_MAX_WIDTH = 4096
SGM_WORKSPACE_CAP = 2 << 30
SGM_PC_MAX = 567                    # 3 channels x (126 prefiltered + 255 >> 2 raw): the largest pixel cost
_SGM_KEYS = ("numDisparities", "blockSize", "P1", "P2", "preFilterCap", "uniquenessRatio", "disp12MaxDiff", "speckleWindowSize",
             "speckleRange", "minDisparity")
_SGM_DEFAULTS = dict(disp12MaxDiff=0, minDisparity=0)


def _sgm_params(params):
    """The parameter sets as tuples in ``_SGM_KEYS`` order, each refused where the matcher does not serve it."""
    if isinstance(params, dict):
        params = [params]
    params = list(params)
    if not 1 <= len(params) <= SGM_MAX_MATCHERS:
        raise RuntimeError("sgm_disparity: 1 <= N <= %d parameter sets; got %d" % (SGM_MAX_MATCHERS, len(params)))
    out = []
    for p in params:
        unknown = set(p) - set(_SGM_KEYS)
        if unknown:
            raise RuntimeError("sgm_disparity: unknown parameter(s) %s; the keys are %s" % (sorted(unknown), list(_SGM_KEYS)))
        missing = [k for k in _SGM_KEYS if k not in p and k not in _SGM_DEFAULTS]
        if missing:
            raise RuntimeError("sgm_disparity: a parameter set lacks %s" % missing)
        D, b, P1, P2, cap, uniq, d12, spw, spr, mind = t = tuple(int(p.get(k, _SGM_DEFAULTS.get(k, 0))) for k in _SGM_KEYS)
        if mind != 0:
            raise RuntimeError("sgm_disparity: minDisparity must be 0; got %d" % mind)
        if D % 16 != 0 or not 16 <= D <= 256:
            raise RuntimeError("sgm_disparity: numDisparities must be a multiple of 16 in [16, 256]; got %d" % D)
        if not 1 <= b <= 3:
            raise RuntimeError("sgm_disparity: blockSize must be 1, 2 or 3 (radius <= 1, for which int16 sums are exact); got %d" % b)
        side = 2 * (b // 2) + 1
        if P1 < 0 or P2 < 0 or 5 * (side * side * SGM_PC_MAX + P2) >= 32767:
            raise RuntimeError("sgm_disparity: P1, P2 >= 0 and 5 ((2r+1)^2 %d + P2) < 32767 (int16 sums); got P1 %d, P2 %d at "
                               "blockSize %d" % (SGM_PC_MAX, P1, P2, b))
        if not 1 <= cap <= 63 or not 0 <= uniq <= 100 or not 0 <= d12 <= 32767 or spw < 0 or not 0 <= spr <= 4096:
            raise RuntimeError("sgm_disparity: need preFilterCap in [1, 63], uniquenessRatio in [0, 100], disp12MaxDiff in [0, 32767], "
                               "speckleWindowSize >= 0 and speckleRange in [0, 4096]; got %s" % (dict(zip(_SGM_KEYS, t)),))
        out.append(t)
    return out


def _sgm_check(base, lookup, params, reverse):
    if not (torch.is_tensor(base) and base.dtype == torch.uint8 and base.dim() == 4 and base.shape[1] == 3 and base.numel() > 0):
        raise RuntimeError("sgm_disparity: base must be a non-empty uint8 tensor [B, 3, H, W]; got %s %s"
                           % (getattr(base, "dtype", type(base)), tuple(getattr(base, "shape", ()))))
    if not (torch.is_tensor(lookup) and lookup.dtype == torch.uint8 and lookup.shape == base.shape and lookup.device == base.device):
        raise RuntimeError("sgm_disparity: lookup must be a uint8 tensor of base's shape %s on its device; got %s %s"
                           % (tuple(base.shape), getattr(lookup, "dtype", type(lookup)), tuple(getattr(lookup, "shape", ()))))
    B, _, H, W = (int(v) for v in base.shape)
    plist = _sgm_params(params)
    if W > SGM_MAX_WIDTH or H > 65535 or B * len(plist) * H * W >= 2 ** 31:
        raise RuntimeError("sgm_disparity: need W <= %d, H <= 65535 and B N H W < 2^31; got %d x %d x %d x %d"
                           % (SGM_MAX_WIDTH, B, len(plist), H, W))
    if reverse is not None:
        n = reverse.numel() if torch.is_tensor(reverse) else len(reverse)
        if n != B:
            raise RuntimeError("sgm_disparity: reverse must have one entry per item (%d); got %d" % (B, n))
    return B, H, W, plist


def _sgm_lo_hi(A):
    left = np.concatenate([A[..., :1], A[..., :-1]], -1)
    right = np.concatenate([A[..., 1:], A[..., -1:]], -1)
    hl, hr = (A + left) >> 1, (A + right) >> 1
    return np.minimum(A, np.minimum(hl, hr)), np.maximum(A, np.maximum(hl, hr))


def _sgm_block_cost(base, lookup, D, r, cap):
    """Steps 1-3 for one pair: C int32 [H, Wv, D]."""
    _, H, W = base.shape
    kinds = []
    for img in (base.astype(np.int32), lookup.astype(np.int32)):
        rows = np.pad(img, ((0, 0), (1, 1), (0, 0)), mode="edge")
        dx = rows[:, :, 2:] - rows[:, :, :-2]                           # [3, H + 2, W - 2]
        g = np.full(img.shape, cap, dtype=np.int32)
        g[:, :, 1:W - 1] = np.clip(dx[:, :-2] + 2 * dx[:, 1:-1] + dx[:, 2:], -cap, cap) + cap
        A = np.concatenate([g, img], 0)                                 # [6, H, W]
        kinds.append((A,) + _sgm_lo_hi(A))
    (u, lo_u, hi_u), (v, lo_v, hi_v) = kinds
    cols = np.arange(D, W)[:, None] - np.arange(D)[None, :]             # [Wv, D]: the lookup column of (x, d)
    pc = np.zeros((H, W - D, D), dtype=np.int32)
    for k in range(6):                                                  # g of the three channels, then their bytes
        a, lo_a, hi_a = (t[k][:, D:, None] for t in (u, lo_u, hi_u))
        b, lo_b, hi_b = (t[k][:, cols] for t in (v, lo_v, hi_v))
        bt = np.minimum(np.maximum(0, np.maximum(a - hi_b, lo_b - a)), np.maximum(0, np.maximum(b - hi_a, lo_a - b)))
        pc += bt if k < 3 else bt >> 2
    if r == 0:
        return pc
    pad = np.pad(pc, ((r, r), (r, r), (0, 0)), mode="edge")
    Wv = W - D
    return sum(pad[dy:dy + H, dx:dx + Wv] for dy in range(2 * r + 1) for dx in range(2 * r + 1))


def _sgm_step(C, q, P1, P2):
    """One step of a path for a whole front: C, q [..., D] -> L."""
    big = np.int32(1 << 28)
    m = q.min(-1, keepdims=True)
    down = np.concatenate([np.full_like(q[..., :1], big), q[..., :-1]], -1)
    up = np.concatenate([q[..., 1:], np.full_like(q[..., :1], big)], -1)
    return C + np.minimum(np.minimum(q, np.minimum(down, up) + P1), m + P2) - m


def _sgm_aggregate(C, P1, P2):
    H, Wv, D = C.shape
    S = np.zeros_like(C)
    for cols in (range(Wv), range(Wv - 1, -1, -1)):                     # from the left, from the right: all rows at once
        L = None
        for x in cols:
            L = C[:, x] if L is None else _sgm_step(C[:, x], L, P1, P2)
            S[:, x] += L
    for dx in (-1, 0, 1):                                               # from above: all columns at once
        L = C[0]
        S[0] += L
        for y in range(1, H):
            q = L if dx == 0 else np.roll(L, -dx, axis=0)               # q[x] = L[x + dx]
            new = _sgm_step(C[y], q, P1, P2)
            if dx == -1:
                new[0] = C[y, 0]
            elif dx == 1:
                new[Wv - 1] = C[y, Wv - 1]
            L = new
            S[y] += L
    return S


def _sgm_select(S, W, uniq, d12):
    """Steps 5 and 6: S [H, Wv, D] -> int32 [H, W]."""
    H, Wv, D = S.shape
    out = np.full((H, W), -16, dtype=np.int32)
    d_star = S.argmin(-1)
    min_s = np.take_along_axis(S, d_star[..., None], -1)[..., 0]
    far = np.abs(np.arange(D)[None, None, :] - d_star[..., None]) > 1
    unique = ~((S * (100 - uniq) < 100 * min_s[..., None]) & far).any(-1)
    sm = np.take_along_axis(S, np.maximum(d_star - 1, 0)[..., None], -1)[..., 0]
    sp = np.take_along_axis(S, np.minimum(d_star + 1, D - 1)[..., None], -1)[..., 0]
    den = np.maximum(sm + sp - 2 * min_s, 1)
    num = (sm - sp) * 16 + den
    frac = np.sign(num) * (np.abs(num) // (2 * den))                    # C's division
    value = 16 * d_star + np.where((d_star == 0) | (d_star == D - 1), 0, frac)
    out[:, D:] = np.where(unique, value, -16)
    xs = np.broadcast_to(np.arange(D, W)[None, :], (H, Wv))
    ys = np.broadcast_to(np.arange(H)[:, None], (H, Wv))
    none = np.int64(1) << 40
    keys = np.full((H, W), none, dtype=np.int64)
    np.minimum.at(keys, (ys[unique], (xs - d_star)[unique]), (min_s.astype(np.int64)[unique] << 16) | xs[unique])
    owner = np.where(keys == none, D, keys & 0xffff).astype(np.int64)   # the proposer's column (D where nobody proposed)
    disp2 = np.take_along_axis(d_star, owner - D, 1)
    is_set = keys != none
    xa = np.broadcast_to(np.arange(W)[None, :], (H, W))
    bad = np.zeros((H, W), dtype=np.int32)
    for k in (0, 15):
        dd = (out + k) >> 4
        x2 = xa - dd
        inside = (x2 >= 0) & (x2 < W)
        x2c = np.clip(x2, 0, W - 1)
        hit = inside & np.take_along_axis(is_set, x2c, 1) & (np.abs(np.take_along_axis(disp2, x2c, 1) - dd) > d12)
        bad += hit
    out[(out >= 0) & (bad == 2)] = -16
    return out


def _sgm_speckle(disp, window, rng16):
    """Step 7 by label propagation with pointer jumping; components do not depend on the order."""
    H, W = disp.shape
    valid = disp >= 0
    lab = np.arange(H * W, dtype=np.int64).reshape(H, W)
    right = valid[:, :-1] & valid[:, 1:] & (np.abs(disp[:, :-1] - disp[:, 1:]) <= rng16)
    down = valid[:-1] & valid[1:] & (np.abs(disp[:-1] - disp[1:]) <= rng16)
    while True:
        new = lab.copy()
        np.minimum(new[:, :-1], np.where(right, lab[:, 1:], new[:, :-1]), out=new[:, :-1])
        np.minimum(new[:, 1:], np.where(right, lab[:, :-1], new[:, 1:]), out=new[:, 1:])
        np.minimum(new[:-1], np.where(down, lab[1:], new[:-1]), out=new[:-1])
        np.minimum(new[1:], np.where(down, lab[:-1], new[1:]), out=new[1:])
        flat = new.reshape(-1)
        for _ in range(4):
            flat = flat[flat]
        new = flat.reshape(H, W)
        if np.array_equal(new, lab):
            break
        lab = new
    sizes = np.bincount(lab[valid], minlength=H * W)
    out = disp.copy()
    out[valid & (sizes[lab] <= window)] = -16
    return out


def sgm_disparity_host(base, lookup, params, reverse=None):
    """K35 in whole-image numpy on the CPU (the path CPU tensors take), bit-equal to the pixel-by-pixel statement of the matcher
    in tests/sgm_ref.py.  Returns int16 [B, N, H, W]."""
    B, H, W, plist = _sgm_check(base, lookup, params, reverse)
    flips = _host_flips(reverse, B)
    b_np, l_np = base.detach().cpu().numpy(), lookup.detach().cpu().numpy()
    out = np.full((B, len(plist), H, W), -16, dtype=np.int16)
    for b in range(B):
        ib, il = (a[b, :, :, ::-1] if flips[b] else a[b] for a in (b_np, l_np))
        done = {}
        for n, (D, blk, P1, P2, cap, uniq, d12, spw, spr, _) in enumerate(plist):
            key = (D, blk // 2, P1, P2, cap, uniq, d12, spw, spr)
            if key not in done:
                disp = np.full((H, W), -16, dtype=np.int32)
                if W > D:
                    S = _sgm_aggregate(_sgm_block_cost(ib, il, D, blk // 2, cap), P1, P2)
                    disp = _sgm_select(S, W, uniq, d12)
                if spw > 0:
                    disp = _sgm_speckle(disp, spw, 16 * spr)
                done[key] = disp[:, ::-1] if flips[b] else disp
            out[b, n] = done[key]
    return torch.from_numpy(out)


def _sgm_native_params(plist):
    arr = (N.SgmParams * len(plist))()
    for i, (D, blk, P1, P2, cap, uniq, d12, spw, spr, mind) in enumerate(plist):
        arr[i] = N.SgmParams(D, blk, P1, P2, cap, uniq, d12, spw, spr, mind)
    return arr


def sgm_plan(B, H, W, params, workspace_cap=SGM_WORKSPACE_CAP):
    """(workspace bytes, sequences of launches) of ``sgm_disparity`` for a batch under ``workspace_cap`` bytes; host only."""
    plist = _sgm_params(params)
    chunks = C.c_int(0)
    nbytes = N.lib().dmh_sgm_plan(int(B), int(H), int(W), _sgm_native_params(plist), len(plist), int(workspace_cap), C.byref(chunks))
    if nbytes < 0:
        raise RuntimeError("libdmh_hip: " + N.lib().dmh_last_error().decode())
    return int(nbytes), int(chunks.value)


def sgm_disparity(base, lookup, params, reverse=None, workspace_cap=SGM_WORKSPACE_CAP, phases=N.SGM_ALL):
    """K35: the integer semi-global stereo matcher of DESIGN.md section 3 (K35) for a batch of stereo pairs on the device; every
    parameter set of ``params`` gives one map.

    base, lookup   uint8 [B, 3, H, W] (``pil_resize(..., want_u8=True).u8``): the view the disparity is for, and the other one.
    params         a list of at most 16 dicts with the keys of ``precompute_depth_hints.stereo_matcher_params()`` (and optionally
                   ``disp12MaxDiff``, 0 by default).  numDisparities a multiple of 16 in [16, 256], blockSize <= 3, minDisparity 0.
    reverse        None, an int32 tensor [B] on base's device, or a host sequence of bools: != 0 where the base image is the right
                   view (the pair is matched mirrored and the result mirrored back).
    workspace_cap  bytes the workspace may take (2 GiB by default); the batch is split into sequences of launches that fit.
    phases         ``N.SGM_ALL``; a subset launches only those phases, for tools/sgm_bench.py (the result is then undefined).
    Returns        int16 [B, N, H, W]: disparity x 16, -16 where nothing matched -- what ``depth_hint_fuse`` takes.

    CPU tensors run ``sgm_disparity_host``."""
    B, H, W, plist = _sgm_check(base, lookup, params, reverse)
    dev = base.device
    if dev.type != "cuda":
        return sgm_disparity_host(base, lookup, params, reverse)
    if reverse is not None and not torch.is_tensor(reverse):
        reverse = torch.tensor([int(bool(v)) for v in reverse], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    if reverse is not None and (reverse.dtype != torch.int32 or reverse.device != dev):
        raise RuntimeError("sgm_disparity: reverse must be an int32 tensor of %d entries on %s" % (B, dev))
    native = _sgm_native_params(plist)
    nbytes = N.lib().dmh_sgm_plan(B, H, W, native, len(plist), int(workspace_cap), None)
    if nbytes < 0:
        raise RuntimeError("libdmh_hip: " + N.lib().dmh_last_error().decode())
    base, lookup = _c(base), _c(lookup)
    out = torch.empty((B, len(plist), H, W), device=dev, dtype=torch.int16)
    ws = torch.empty(int(nbytes), device=dev, dtype=torch.uint8)
    N.check(_timed("sgm_disparity", lambda: N.lib().dmh_sgm_disparity(
        N.ptr(base), N.ptr(lookup), N.ptr(None if reverse is None else _c(reverse)), B, H, W, native, len(plist),
        C.c_void_p(out.data_ptr()), N.ptr(ws), int(nbytes), int(phases), N.stream()), B * H * W * (6 + 2 * len(plist))))
    return out


# ---------------------------------------------------------------------------------------------------------------- K39
PseudoLidarOut = namedtuple("PseudoLidarOut", ["points", "offsets"])
LIDAR_FORMS = {"depth": N.LIDAR_DEPTH, "disp": N.LIDAR_DISP, "net": N.LIDAR_NET}
LIDAR_BASELINE = 0.54                   # generate_lidar.py:12
LIDAR_DESC_CACHE = 16
_lidar_desc_cache = _UploadCache(LIDAR_DESC_CACHE, "pseudo_lidar: the first call with these shapes uploads their descriptors; make it "
                                                   "once before capturing a graph")      # (device, form, shapes, offsets) -> tables


def lidar_calib(path_or_text, crop=None):
    """The 27 float64 values K39 takes for one frame -- f_u f_v c_u c_v b_x b_y, inv(R0), C2V -- from a KITTI-object calibration
    file (or its text), made as the reference's ``Calibration.__init__`` makes them (datasets/kitti_object.py).
    ``crop=(left, top)``: the scene was cropped by that many pixels; c_u and c_v move with it, nothing else does."""
    from .datasets.kitti_object import Calibration
    return Calibration(path_or_text, crop).packed()


def _lidar_shapes(shapes, n):
    shapes = _host_pairs(shapes)
    if n < 1 or len(shapes) != n or not all(h >= 0 and w >= 0 and h * w < 2 ** 31 for h, w in shapes):
        raise RuntimeError("pseudo_lidar: shapes must be n >= 1 pairs (H, W) with H, W >= 0, one per frame (%d); got %s" % (n, shapes))
    return shapes


def _lidar_offsets(form, shapes, offsets, src_len):
    """The first element of every frame of a packed depth / disp input (K32's cell offsets); default: one map after the other."""
    if form == "net":
        if offsets is not None:
            raise RuntimeError("pseudo_lidar: offsets belong to the packed depth / disp forms")
        return None
    if offsets is None:
        offsets = np.cumsum([0] + [h * w for h, w in shapes])
    offsets = tuple(int(v) for v in _host_list(offsets))
    if len(offsets) not in (len(shapes), len(shapes) + 1) or any(o < 0 or o + h * w > src_len for o, (h, w) in zip(offsets, shapes)):
        raise RuntimeError("pseudo_lidar: offsets must place every frame's H W values inside the %d values given; got %s for %s"
                           % (src_len, offsets, shapes))
    return offsets[:len(shapes)]


def _lidar_lin_axis(dst, src):
    """K25's lin_axis for every destination index of one axis: (s0, s1, f), f float32 (OpenCV's INTER_LINEAR coordinates)."""
    scale = float(src) / float(dst)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    return s, np.minimum(s + 1, src - 1), f


def lidar_net_depth_host(disp, H, W, quantise=False):
    """The net form's depth of one frame, float32 [H, W], from the sigmoid output [h, w]: disp_to_depth's scaling in fp32, the
    bilinear resize, 5.4 / disp, evaluate's clamp and with ``quantise`` the 16-bit PNG round trip -- every operation a rounded
    float32 one, in the kernel's order."""
    disp = np.asarray(disp, dtype=np.float32)
    h, w = disp.shape
    with np.errstate(all="ignore"):
        taps = np.float32(1.0 / 100.0) + np.float32(1.0 / 0.1 - 1.0 / 100.0) * disp
        sx, sx1, fx = _lidar_lin_axis(W, w)
        sy, sy1, fy = _lidar_lin_axis(H, h)
        a0, a1 = np.float32(1) - fx, fx
        b0, b1 = (np.float32(1) - fy)[:, None], fy[:, None]
        rows = a0 * taps[:, sx] + a1 * taps[:, sx1]
        small = b0 * rows[sy] + b1 * rows[sy1]
        depth = (np.float32(1) / small) * np.float32(5.4)
        depth = np.where(depth < np.float32(1e-3), np.float32(1e-3), depth)
        depth = np.where(depth > np.float32(80), np.float32(80), depth)
        if quantise:
            q = depth * np.float32(256)
            k = np.where(np.isnan(q), np.float32(0), q).astype(np.uint16)
            depth = k.astype(np.float32) / np.float32(256)
    return depth.astype(np.float32)


def _lidar_frame_host(cal, H, W, d, keep, max_high):
    """project_image_to_velo and the validity test on the candidates of one frame: ``d`` float64 [H W] in pixel order, ``keep`` the
    candidate mask (None: all).  Element-wise float64 in the kernel's association; never ``np.dot``."""
    p = np.arange(H * W, dtype=np.int64) if keep is None else np.nonzero(keep)[0]
    v, u = (p // max(W, 1)).astype(np.float64), (p % max(W, 1)).astype(np.float64)
    d = d[p]
    f_u, f_v, c_u, c_v, b_x, b_y = (float(c) for c in cal[:6])
    Ri, Cm = cal[6:15].reshape(3, 3), cal[15:27].reshape(3, 4)
    with np.errstate(all="ignore"):
        x = ((u - c_u) * d) / f_u + b_x
        y = ((v - c_v) * d) / f_v + b_y
        z = d
        r = [(Ri[i, 0] * x + Ri[i, 1] * y) + Ri[i, 2] * z for i in range(3)]
        o = [((Cm[i, 0] * r[0] + Cm[i, 1] * r[1]) + Cm[i, 2] * r[2]) + Cm[i, 3] for i in range(3)]
        valid = (o[0] >= 0) & (o[2] < max_high)                 # a NaN fails either comparison
        rows = np.stack([o[0][valid], o[1][valid], o[2][valid], np.ones(int(valid.sum()))], axis=1).astype(np.float32)
    return rows


def pseudo_lidar_host(src, form, shapes, calib, max_high=1, quantise=False, offsets=None):
    """K39 in numpy, the definition the kernel is held to (and the path CPU tensors take).  ``src``: float32, the packed maps of
    the depth / disp forms (frame f at ``offsets[f]``) or the network's output [n, h, w] of the net form.  ``calib``: float64
    [n, 27].  Returns (float32 [M, 4], int64 [n + 1]): the kept rows of all frames in batch order and pixel order, and where each
    frame's rows start."""
    if form not in LIDAR_FORMS:
        raise RuntimeError("pseudo_lidar: form must be one of %s; got %r" % (sorted(LIDAR_FORMS), form))
    src = np.asarray(src, dtype=np.float32)
    n = src.shape[0] if form == "net" else len(shapes)
    if form == "net" and src.ndim != 3:
        raise RuntimeError("pseudo_lidar: the net form takes [n, h, w]; got %s" % (src.shape,))
    if quantise and form != "net":
        raise RuntimeError("pseudo_lidar: quantise belongs to the net form")
    shapes = _lidar_shapes(shapes, n)
    calib = np.asarray(calib, dtype=np.float64).reshape(n, N.LIDAR_CALIB)
    starts = _lidar_offsets(form, shapes, offsets, src.size)
    flat = src.reshape(-1)
    max_high = float(max_high)
    clouds = []
    for f, (H, W) in enumerate(shapes):
        cal, keep = calib[f], None
        if H * W == 0:
            clouds.append(np.zeros((0, 4), dtype=np.float32))
            continue
        if form == "net":
            d = lidar_net_depth_host(src[f], H, W, quantise).reshape(-1).astype(np.float64)
        else:
            m = flat[starts[f]:starts[f] + H * W]
            if form == "depth":
                d = m.astype(np.float64)
            else:
                with np.errstate(all="ignore"):
                    s = np.where(m < 0, np.float32(0), m)       # a NaN stays and fails the mask
                    keep = s > 0
                    d = (cal[0] * LIDAR_BASELINE) / ((s.astype(np.float64) + 1.) - keep.astype(np.float64))
        clouds.append(_lidar_frame_host(cal, H, W, d, keep, max_high))
    counts = np.array([0] + [c.shape[0] for c in clouds], dtype=np.int64)
    return np.concatenate(clouds).reshape(-1, 4), np.cumsum(counts)


def _lidar_tables_device(device, form, shapes, starts):
    def make():
        tiles = [(h * w + N.LIDAR_TILE - 1) // N.LIDAR_TILE for h, w in shapes]
        first = np.cumsum([0] + tiles)
        desc = [[h, w, 0 if starts is None else starts[i], int(first[i])] for i, (h, w) in enumerate(shapes)]
        tile_frame = np.repeat(np.arange(len(shapes)), tiles)
        if tile_frame.size == 0:
            tile_frame = np.array([-1])                         # never read: a launch has n_tiles = 0
        return [torch.tensor(desc, dtype=torch.int32), torch.from_numpy(tile_frame.astype(np.int32))], int(first[-1])
    (desc, tile_frame), n_tiles = _lidar_desc_cache.get((str(device), form, shapes, starts), device, make)
    return desc, tile_frame, n_tiles


def pseudo_lidar(src, form, shapes, calib, max_high=1, quantise=False, offsets=None):
    """K39: maps of a batch of frames to velodyne-frame point clouds, as the reference's preprocessing/generate_lidar.py makes them
    on the host (``project_depth_to_points`` / ``project_disp_to_points`` over ``Calibration.project_image_to_velo``), float32-equal,
    in three launches with no host read.

    src      float32.  ``form`` "depth": metric depth maps packed flat, frame f's H W values at ``offsets[f]`` (K32's layout; default
             one map after the other); every pixel is a candidate.  "disp": the same layout of disparities in pixels; negatives
             count as 0 and only pixels with a positive disparity are candidates.  "net": the network's sigmoid output [n, h, w]
             (or [n, 1, h, w]); per frame it is scaled (disp_to_depth(., 0.1, 100)), resized to (H, W) as evaluate resizes it,
             turned into 5.4 / disp, clamped to [1e-3, 80], and with ``quantise`` rounded down to 1 / 256 as a 16-bit PNG stores it.
    shapes   n pairs (H, W): each frame's own size.  Host values: they size the launch.
    calib    float64 [n, 27] on src's device: ``lidar_calib`` of every frame.
    max_high a point is kept if its velodyne x >= 0 and z < max_high.
    Returns  PseudoLidarOut(points, offsets): float32 [sum H W, 4], the kept rows (x, y, z, 1) of all frames in batch order, each
             frame's in row-major pixel order, and int64 [n + 1] on the device: frame f is points[offsets[f]:offsets[f + 1]].
             Rows from offsets[n] on are unspecified.

    CPU tensors run ``pseudo_lidar_host``, the numpy restatement the kernel is bit-equal to."""
    if form not in LIDAR_FORMS:
        raise RuntimeError("pseudo_lidar: form must be one of %s; got %r" % (sorted(LIDAR_FORMS), form))
    if not torch.is_tensor(src) or src.dtype != torch.float32:
        raise RuntimeError("pseudo_lidar: src must be a float32 tensor; got %s" % (getattr(src, "dtype", type(src)),))
    if form == "net":
        if src.dim() == 4 and src.shape[1] == 1:
            src = src[:, 0]
        if src.dim() != 3 or src.shape[1] < 1 or src.shape[2] < 1:
            raise RuntimeError("pseudo_lidar: the net form takes [n, h, w] or [n, 1, h, w]; got %s" % (tuple(src.shape),))
        n, h, w = (int(v) for v in src.shape)
    else:
        if quantise:
            raise RuntimeError("pseudo_lidar: quantise belongs to the net form")
        if src.dim() != 1:
            raise RuntimeError("pseudo_lidar: the %s form takes the maps packed flat; got %s" % (form, tuple(src.shape)))
        n, h, w = len(shapes), 0, 0
    shapes = _lidar_shapes(shapes, n)
    if not torch.is_tensor(calib) or calib.dtype != torch.float64 or calib.numel() != N.LIDAR_CALIB * n:
        raise RuntimeError("pseudo_lidar: calib must be a float64 tensor of %d x %d entries; got %s %s"
                           % (n, N.LIDAR_CALIB, getattr(calib, "dtype", type(calib)), tuple(getattr(calib, "shape", ()))))
    dev = src.device
    if calib.device != dev:
        raise RuntimeError("pseudo_lidar: src and calib must share a device; got %s and %s" % (dev, calib.device))
    starts = _lidar_offsets(form, shapes, offsets, src.numel())
    cap = sum(hh * ww for hh, ww in shapes)
    if cap >= 2 ** 31 or src.numel() >= 2 ** 31:
        raise RuntimeError("pseudo_lidar: the batch must hold fewer than 2^31 pixels; got %d" % cap)
    if dev.type != "cuda":
        pts, off = pseudo_lidar_host(src.numpy(), form, shapes, calib.numpy(), max_high, quantise, starts)
        points = torch.zeros((cap, 4), dtype=torch.float32)
        points[:pts.shape[0]] = torch.from_numpy(pts)
        return PseudoLidarOut(points, torch.from_numpy(off))
    desc, tile_frame, n_tiles = _lidar_tables_device(dev, form, shapes, starts)
    src, calib = _c(src), _c(calib)
    ws = torch.empty(2 * max(n_tiles, 1), device=dev, dtype=torch.int32)
    points = torch.empty((cap, 4), device=dev, dtype=torch.float32)
    off = torch.empty(n + 1, device=dev, dtype=torch.int64)
    N.check(_timed("pseudo_lidar", lambda: N.lib().dmh_pseudo_lidar(
        N.ptr(src) if src.numel() else None, src.numel(), LIDAR_FORMS[form], h, w, int(bool(quantise)), N.ptr_f64(calib), N.ptr(desc),
        N.ptr(tile_frame), n, n_tiles, float(max_high), N.ptr(ws), N.ptr(points) if cap else None, cap, C.c_void_p(off.data_ptr()),
        N.stream()), 2 * 4 * src.numel() + 16 * cap))
    return PseudoLidarOut(points, off)


def lidar_clouds(out):
    """The clouds of a ``PseudoLidarOut`` on the host, one float32 [M_f, 4] array per frame: the n + 1 offsets are read first (they
    say how many rows are in use), then only those rows are copied."""
    off = out.offsets.cpu().numpy()
    used = out.points[:int(off[-1])].cpu().numpy()
    return [used[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
