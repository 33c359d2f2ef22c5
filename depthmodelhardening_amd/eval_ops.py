"""The evaluation operators: the masked depth errors, the benign KITTI evaluation (K25), the fused percentile + colour map (K37)
and the odometry evaluation's trajectory error (K40) and pair stem (K41).
ops.py re-exports every name, and callers reach them as ``ops.<name>``.

The depth errors, K25 and K41 launch on the device only.  K37 and K40 take CPU tensors too: they run ``disp_colorize_host`` /
``pose_ate_host``, the numpy restatements the kernels are held to.
"""
import functools
import os
from collections import namedtuple

import numpy as np
import torch

from . import _native as N
from ._launch import _UploadCache, _c, _need_cuda, _need_f32, _need_i32, _timed


def masked_depth_errors(disp_gt, disp_pred, mask=None, min_depth=0.1, max_depth=100.0, scale=5.4, clamp_lo=1e-3,
                        clamp_hi=80.0):
    """The eight attack-evaluation metrics of MD2/evaluate_depth.py:57-99 computed from two disparity maps in one
    pass on the device: returns a tensor [abs_err, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3]."""
    lib = N.lib()
    disp_gt, disp_pred = _c(disp_gt.detach()), _c(disp_pred.detach())
    n = disp_gt.numel()
    if disp_pred.numel() != n or (mask is not None and mask.numel() != n):
        raise RuntimeError("masked_depth_errors: size mismatch")
    part = torch.empty(lib.dmh_depth_errors_partials_size(n), device=disp_gt.device, dtype=torch.float32)
    out = torch.empty(8, device=disp_gt.device, dtype=torch.float32)
    N.check(lib.dmh_masked_depth_errors(N.ptr(disp_gt), N.ptr(disp_pred), N.ptr(None if mask is None else _c(mask)), n,
                                        min_depth, max_depth, scale, clamp_lo, clamp_hi, N.ptr(part), N.ptr(out),
                                        N.stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------- K25
EIGEN_REC, EIGEN_CHUNK, EIGEN_MAX_BATCH = 8, 8192, 64       # DMH_EIGEN_* of include/dmh_hip.h


def eigen_crop(gt_h, gt_w):
    """The Eigen crop (y0, y1, x0, x1) of a gt_h x gt_w map, in double and truncated as MD2/evaluate_depth.py:363-364 does."""
    return np.array([0.40810811 * gt_h, 0.99189189 * gt_h, 0.03594771 * gt_w, 0.96405229 * gt_w]).astype(np.int32)


def _eigen_ws(n, device):
    return torch.empty(N.lib().dmh_eigen_select_ws_size(n), device=device, dtype=torch.int32)


def eigen_gt_stats(gt, table, blk_img, first, n, b0, grid, eigen):
    """K25 on the ground truth alone: (medians fp32 [n], valid counts int32 [n]) of the images first .. first + n - 1 of a pack
    (np.median of the valid values; NaN and 0 for a map without a valid pixel).  Three histogram passes, no sort."""
    lib = N.lib()
    _need_f32(gt, "gt"), _need_i32(table, "table"), _need_i32(blk_img, "blk_img")
    if not 0 < n <= EIGEN_MAX_BATCH:
        raise RuntimeError("eigen_gt_stats: 1 .. %d images per call; got %d" % (EIGEN_MAX_BATCH, n))
    med = torch.empty(n, device=gt.device, dtype=torch.float32)
    cnt = torch.empty(n, device=gt.device, dtype=torch.int32)
    ws = _eigen_ws(n, gt.device)
    N.check(lib.dmh_eigen_gt_stats(N.ptr(gt), gt.numel(), N.ptr(table), N.ptr(blk_img), int(table.shape[0]), blk_img.numel(),
                                   int(first), int(n), int(b0), int(grid), int(bool(eigen)), N.ptr(ws), N.ptr(med), N.ptr(cnt),
                                   N.stream()))
    return med, cnt


def eigen_depth_errors_launch(pred_disp, pred_disp_flip, gt, table, blk_img, med_gt, first, b0, grid, px0, npx, eigen,
                              scale_factor=1.0, median_scaling=True):
    """K25's launches for one batch on plain tensors (what ``eigen_depth_errors`` and ``torch.ops.dmh.eigen_depth_errors`` share):
    (errors [n, 8], ratios [n], depth [npx], medians of the valid depths [n]).  ``px0`` / ``npx``: offset and pixel count of the
    batch inside ``gt``; ``b0`` / ``grid``: its work blocks.  Without median scaling the medians are not computed: they and
    ``ratios`` are NaN."""
    lib = N.lib()
    _need_f32(pred_disp, "pred_disp"), _need_f32(gt, "gt"), _need_f32(med_gt, "med_gt")
    _need_i32(table, "table"), _need_i32(blk_img, "blk_img")
    if pred_disp.dim() != 3:
        raise RuntimeError("eigen_depth_errors: pred_disp must be [n, h, w]")
    n, h, w = [int(v) for v in pred_disp.shape]
    if not 0 < n <= EIGEN_MAX_BATCH:
        raise RuntimeError("eigen_depth_errors: 1 .. %d predictions per call; got %d" % (EIGEN_MAX_BATCH, n))
    if pred_disp_flip is not None and (_need_f32(pred_disp_flip, "pred_disp_flip").shape != pred_disp.shape):
        raise RuntimeError("eigen_depth_errors: pred_disp_flip must have pred_disp's shape")
    if med_gt.numel() != table.shape[0] or table.dim() != 2 or table.shape[1] != EIGEN_REC:
        raise RuntimeError("eigen_depth_errors: table must be [N, %d] and med_gt [N]" % EIGEN_REC)
    if px0 < 0 or npx <= 0 or px0 + npx > gt.numel():
        raise RuntimeError("eigen_depth_errors: the batch's pixels must lie in gt")
    dev = pred_disp.device
    pred_disp = _c(pred_disp.detach())
    flip = None if pred_disp_flip is None else _c(pred_disp_flip.detach())
    depth = torch.empty(int(npx), device=dev, dtype=torch.float32)
    errors = torch.empty((n, 8), device=dev, dtype=torch.float32)
    part = torch.empty(lib.dmh_eigen_partials_size(int(grid)), device=dev, dtype=torch.float32)
    ws = _eigen_ws(n, dev) if median_scaling else None
    sizes = (int(table.shape[0]), blk_img.numel(), int(first), n, int(b0), int(grid))
    N.check(lib.dmh_eigen_pred_depth(N.ptr(pred_disp), N.ptr(flip), h, w, N.ptr(gt), gt.numel(), N.ptr(table), N.ptr(blk_img),
                                     *sizes, int(bool(eigen)), float(scale_factor), int(px0), N.ptr(depth), depth.numel(),
                                     N.ptr(ws), N.stream()))
    if median_scaling:
        med = torch.empty(n, device=dev, dtype=torch.float32)
        ratios = torch.empty(n, device=dev, dtype=torch.float32)
        N.check(lib.dmh_eigen_pred_ratio(N.ptr(depth), depth.numel(), int(px0), gt.numel(), N.ptr(table), N.ptr(blk_img), *sizes,
                                         N.ptr(ws), N.ptr(med_gt), N.ptr(med), N.ptr(ratios), N.stream()))
    else:
        ratios = torch.full((n,), float("nan"), device=dev, dtype=torch.float32)
        med = ratios.clone()
    N.check(lib.dmh_eigen_metrics(N.ptr(gt), gt.numel(), N.ptr(depth), depth.numel(), int(px0), N.ptr(table), N.ptr(blk_img),
                                  *sizes, N.ptr(ratios if median_scaling else None), N.ptr(part), N.ptr(errors), N.stream()))
    return errors, ratios, depth, med


class EigenGtPack(object):
    """The ground truth of an evaluation set on the device (``eigen_gt_pack``): ``gt`` the maps one after the other (fp32),
    ``table`` / ``blk_img`` K25's tables, ``counts`` / ``medians`` the valid pixels and np.median of the valid values of every map
    (they depend on the ground truth only: computed once, here).  Host copies: ``shapes``, ``crops`` (y0, y1, x0, x1),
    ``offsets`` [N + 1] and ``blk_first`` [N + 1]."""

    def __init__(self, gt, table, blk_img, shapes, crops, offsets, blk_first, eval_split):
        self.gt, self.table, self.blk_img = gt, table, blk_img
        self.shapes, self.crops, self.offsets, self.blk_first = shapes, crops, offsets, blk_first
        self.eval_split, self.eigen = eval_split, eval_split == "eigen"
        self.counts = self.medians = None

    def __len__(self):
        return len(self.shapes)

    def view(self, flat, first, i):
        """Image ``first + i`` of a batch's flat buffer (``return_pred``) as [gt_h, gt_w]."""
        o = int(self.offsets[first + i] - self.offsets[first])
        gh, gw = self.shapes[first + i]
        return flat[o:o + gh * gw].view(gh, gw)


def eigen_gt_pack(gt_list, eval_split, device):
    """Packs the 2-D ground-truth maps ``gt_list`` (their own, different sizes) for K25: one flat fp32 buffer, the record table
    (crop bounds of MD2/evaluate_depth.py:363-364 for split ``eigen``, the whole map otherwise), and per map the number of valid
    pixels and the median of the valid values."""
    device = torch.device(device)
    _need_cuda(device)
    maps = [np.ascontiguousarray(np.asarray(g), dtype=np.float32) for g in gt_list]
    if not maps or any(m.ndim != 2 or m.size == 0 for m in maps):
        raise RuntimeError("eigen_gt_pack: need at least one ground-truth map, all of them 2-D and not empty")
    shapes = [tuple(int(v) for v in m.shape) for m in maps]
    sizes = np.array([h * w for h, w in shapes], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    blocks = (sizes + EIGEN_CHUNK - 1) // EIGEN_CHUNK
    blk_first = np.concatenate([[0], np.cumsum(blocks)])
    if offsets[-1] >= 2 ** 31:
        raise RuntimeError("eigen_gt_pack: %d pixels; a pack holds fewer than 2^31" % offsets[-1])
    eigen = eval_split == "eigen"
    crops = np.stack([eigen_crop(h, w) if eigen else np.array([0, h, 0, w], dtype=np.int32) for h, w in shapes])
    table = np.zeros((len(maps), EIGEN_REC), dtype=np.int32)
    table[:, 0], table[:, 1], table[:, 2] = offsets[:-1], [s[0] for s in shapes], [s[1] for s in shapes]
    table[:, 3:7], table[:, 7] = crops, blk_first[:-1]
    blk_img = np.repeat(np.arange(len(maps), dtype=np.int32), blocks)
    flat = np.concatenate([m.ravel() for m in maps])
    pack = EigenGtPack(torch.from_numpy(flat).to(device), torch.from_numpy(table).to(device), torch.from_numpy(blk_img).to(device),
                       shapes, crops, offsets, blk_first, eval_split)
    med, cnt = [], []
    for first in range(0, len(maps), EIGEN_MAX_BATCH):
        n = min(EIGEN_MAX_BATCH, len(maps) - first)
        m, c = eigen_gt_stats(pack.gt, pack.table, pack.blk_img, first, n, int(blk_first[first]),
                              int(blk_first[first + n] - blk_first[first]), eigen)
        med.append(m)
        cnt.append(c)
    pack.medians, pack.counts = torch.cat(med), torch.cat(cnt)
    return pack


def eigen_depth_errors(pred_disp, pack, first, *, pred_disp_flip=None, scale_factor=1.0, median_scaling=True, return_pred=False):
    """MD2/evaluate_depth.py:351-384 for the predictions ``pred_disp`` [n, h, w] (disparities at network resolution) of the images
    ``first`` .. ``first + n - 1`` of ``pack``: (errors [n, 8], ratios [n]) on the device, nothing read by the host.
    ``pred_disp_flip``: the predictions of the mirrored frames (not mirrored back): --post_process.  ``scale_factor``:
    --pred_depth_scale_factor.  ``median_scaling`` off: no medians, ``ratios`` is NaN.  ``return_pred``: also the scratch buffer,
    laid out like the batch's ground truth (``pack.view``): the depth before median scaling at the valid pixels, NaN (all bits
    set) at the others; and the medians [n] of its valid values."""
    if not isinstance(pack, EigenGtPack):
        raise RuntimeError("eigen_depth_errors: pack must come from eigen_gt_pack")
    if not torch.is_tensor(pred_disp) or pred_disp.dim() != 3:
        raise RuntimeError("eigen_depth_errors: pred_disp must be [n, h, w]")
    n, first = int(pred_disp.shape[0]), int(first)
    if first < 0 or n == 0 or first + n > len(pack):
        raise RuntimeError("eigen_depth_errors: predictions %d .. %d, but the pack holds %d ground-truth maps" % (
            first, first + n - 1, len(pack)))
    px0, b0 = int(pack.offsets[first]), int(pack.blk_first[first])
    errors, ratios, depth, med = eigen_depth_errors_launch(
        pred_disp, pred_disp_flip, pack.gt, pack.table, pack.blk_img, pack.medians, first, b0, int(pack.blk_first[first + n]) - b0,
        px0, int(pack.offsets[first + n]) - px0, pack.eigen, scale_factor, median_scaling)
    return (errors, ratios, depth, med) if return_pred else (errors, ratios)


# ---------------------------------------------------------------------------------------------------------------- K37
COLORIZE_MODES = {"min_p95": N.COLORIZE_MIN_P95, "zero_ref": N.COLORIZE_ZERO_REF, "min_max": N.COLORIZE_MIN_MAX}
COLORIZE_TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "magma_256.txt")
ColorizeOut = namedtuple("ColorizeOut", ["rgb", "map", "stats"])
_colorize_table_cache = _UploadCache(8, "disp_colorize: the first call on a device uploads the colour table; make it once before "
                                        "capturing a graph")


@functools.lru_cache(maxsize=None)
def magma_table():
    """(matplotlib's magma at 256 entries * 255).astype(uint8) as uint8 [256, 3]: data/magma_256.txt (256 lines "r g b"), written once by
    tools/make_goldens_colorize.py and read once per process.  matplotlib is not imported."""
    with open(COLORIZE_TABLE_PATH) as f:
        rows = [[int(v) for v in line.split()] for line in f if line.strip() and not line.startswith("#")]
    if len(rows) != 256 or any(len(r) != 3 or min(r) < 0 or max(r) > 255 for r in rows):
        raise RuntimeError("%s must hold 256 lines of three bytes" % COLORIZE_TABLE_PATH)
    return np.array(rows, dtype=np.uint8)


def percentile_plan(n, q=95):
    """(lo, hi, g) of ``np.percentile(a, q)`` for a float32 ``a`` of n elements (numpy 2: float32 throughout): the result is
    ``lerp(sorted[lo], sorted[hi], g)``.  numpy's own expressions (the "linear" method's virtual index ``(n - 1) * quantiles`` and
    the bounds of ``_get_indexes``), evaluated in float32 as numpy evaluates them -- they depend on n and q only."""
    n = int(n)
    if n < 1:
        raise RuntimeError("percentile_plan: n must be positive; got %d" % n)
    quant = np.asanyarray(np.true_divide(q, np.float32(100)), dtype=np.float32)
    if not 0 <= float(quant) <= 1:
        raise RuntimeError("percentile_plan: q must lie in [0, 100]; got %r" % (q,))
    vi = np.asanyarray((n - 1) * quant)
    if vi.dtype != np.float32:
        raise RuntimeError("percentile_plan: the virtual index left float32 (%s)" % vi.dtype)
    if vi >= n - 1:
        return n - 1, n - 1, 0.0
    if vi < 0:
        return 0, 0, 0.0
    lo = np.floor(vi)
    return int(lo), int(lo) + 1, float(np.float32(vi - lo))


def _colorize_panels(panels, n_src):
    """Panels as (a, b, mode number, ref) tuples; the default is one ``min_p95`` panel per map."""
    if panels is None:
        panels = [(i, -1, "min_p95", i) for i in range(n_src)]
    out = []
    for i, pn in enumerate(panels):
        if len(pn) != 4:
            raise RuntimeError("disp_colorize: a panel is (a, b, mode, ref); got %r" % (pn,))
        a, b, mode, ref = pn
        mode = COLORIZE_MODES.get(mode, mode)
        if mode not in COLORIZE_MODES.values():
            raise RuntimeError("disp_colorize: mode must be one of %s; got %r" % (sorted(COLORIZE_MODES), pn[2]))
        a, b, ref = int(a), int(b), int(ref)
        if not (0 <= a < n_src and -1 <= b < n_src):
            raise RuntimeError("disp_colorize: panel %d names a map outside the batch of %d: a = %d, b = %d" % (i, n_src, a, b))
        out.append((a, b, int(mode), ref))
    if not 1 <= len(out) <= N.COLORIZE_MAX_PANELS:
        raise RuntimeError("disp_colorize: 1 <= panels <= %d; got %d" % (N.COLORIZE_MAX_PANELS, len(out)))
    for i, (a, b, mode, ref) in enumerate(out):
        if mode == N.COLORIZE_ZERO_REF and not 0 <= ref < len(out):
            raise RuntimeError("disp_colorize: panel %d takes its limit from panel %d, outside the %d panels" % (i, ref, len(out)))
    return out


def _colorize_check(maps, panels, out_size, out, origins):
    if not (torch.is_tensor(maps) and maps.dtype == torch.float32 and maps.dim() == 3 and maps.numel() > 0):
        raise RuntimeError("disp_colorize: maps must be a non-empty float32 tensor [B, h, w]; got %s %s"
                           % (getattr(maps, "dtype", type(maps)), tuple(getattr(maps, "shape", ()))))
    B, h, w = (int(v) for v in maps.shape)
    H, W = (h, w) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if H < 1 or W < 1:
        raise RuntimeError("disp_colorize: out_size must be a positive (H, W); got %s" % (out_size,))
    panels = _colorize_panels(panels, B)
    if (out is None) != (origins is None):
        raise RuntimeError("disp_colorize: out (a uint8 mosaic [Hm, Wm, 3]) and origins (one (y, x) per panel) go together")
    offsets, pitch = [i * H * W * 3 for i in range(len(panels))], W * 3
    if out is not None:
        if not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.dim() == 3 and out.shape[2] == 3 and out.is_contiguous()
                and out.device == maps.device):
            raise RuntimeError("disp_colorize: out must be a contiguous uint8 tensor [Hm, Wm, 3] on the maps' device")
        Hm, Wm = int(out.shape[0]), int(out.shape[1])
        if len(origins) != len(panels):
            raise RuntimeError("disp_colorize: one origin per panel (%d); got %d" % (len(panels), len(origins)))
        offsets, pitch = [], Wm * 3
        for y, x in origins:
            y, x = int(y), int(x)
            if not (0 <= y and y + H <= Hm and 0 <= x and x + W <= Wm):
                raise RuntimeError("disp_colorize: a %d x %d panel at (%d, %d) leaves the %d x %d mosaic" % (H, W, y, x, Hm, Wm))
            offsets.append((y * Wm + x) * 3)
    return B, h, w, H, W, panels, offsets, pitch


def colorize_bytes_host(a, vmin, vmax):
    """The bytes of ``(ScalarMappable(Normalize(vmin, vmax), 'magma').to_rgba(a)[..., :3] * 255).astype(uint8)`` for a float32
    array: float32 throughout, the index 0 where 256 x < 0, 255 where 256 x >= 256, trunc(256 x) otherwise."""
    a, vmin, vmax = np.asarray(a, dtype=np.float32), np.float32(vmin), np.float32(vmax)
    with np.errstate(all="ignore"):
        x = np.zeros_like(a) if vmin == vmax else (a - vmin) / (vmax - vmin)
        xa = x * np.float32(256)
        idx = np.where(xa < 0, 0, np.where(xa >= 256, 255, np.trunc(xa))).astype(np.int64)
    return magma_table()[idx]


def disp_colorize_host(maps, panels=None, out_size=None, out=None, origins=None, return_map=False, q=95):
    """K37's numpy twin, the arithmetic stated in csrc/disp_colorize.hip: sort instead of the radix select, numpy's float32 lerp,
    float32 limits and index, the packaged table.  With ``out_size`` the map is resized by torch's own float32 CPU
    ``F.interpolate(bilinear, align_corners=False)``, which is NOT bit-equal to the kernel's resize (torch's back ends differ among
    themselves): colour the kernel's returned map (no ``out_size``) to compare bytes."""
    B, h, w, H, W, panels, offsets, pitch = _colorize_check(maps, panels, out_size, out, origins)
    src = maps.detach().cpu().numpy()
    lo, hi, g = percentile_plan(H * W, q)
    g = np.float32(g)
    made, stats = [], np.zeros((len(panels), N.COLORIZE_STATS), dtype=np.float32)
    for i, (a, b, mode, ref) in enumerate(panels):
        m = src[a] if b < 0 else np.abs(src[a] - src[b])
        if (H, W) != (h, w):
            m = torch.nn.functional.interpolate(torch.from_numpy(np.ascontiguousarray(m))[None, None], (H, W), mode="bilinear",
                                                align_corners=False)[0, 0].numpy()
        s = np.sort(m, axis=None)
        a_lo, a_hi = s[lo], s[hi]
        d = a_hi - a_lo
        p = a_hi - d * (1 - g) if g >= 0.5 else a_lo + d * g
        stats[i] = (s[0], s[-1], a_lo, a_hi, p)
        made.append(m)
    rgb = np.empty((len(panels), H, W, 3), dtype=np.uint8)
    for i, (a, b, mode, ref) in enumerate(panels):
        vmin, vmax = ((stats[i, 0], stats[i, 4]) if mode == N.COLORIZE_MIN_P95 else
                      (np.float32(0), stats[ref, 4]) if mode == N.COLORIZE_ZERO_REF else (stats[i, 0], stats[i, 1]))
        rgb[i] = colorize_bytes_host(made[i], vmin, vmax)
    if out is not None:
        view = out.numpy()
        for i, (y, x) in enumerate(origins):
            view[int(y):int(y) + H, int(x):int(x) + W] = rgb[i]
    return ColorizeOut(out if out is not None else torch.from_numpy(rgb), torch.from_numpy(np.stack(made)) if return_map else None,
                       torch.from_numpy(stats))


def disp_colorize(maps, panels=None, out_size=None, out=None, origins=None, return_map=False, q=95):
    """K37: float maps to magma-coloured bytes, as MD2/test_simple.py:136-156 and the figures of my_utils.py:43-105 make them on
    the host, in one fixed chain of launches with no host read.

    maps      float32 [B, h, w], finite (disparities).
    panels    what is coloured: a sequence of (a, b, mode, ref) -- maps[a], or |maps[a] - maps[b]| when b >= 0, with the limits
              "min_p95" (the panel's own minimum and q-th percentile), "zero_ref" (0 and the percentile of panel ``ref``) or
              "min_max" (the panel's minimum and maximum).  Default: every map, "min_p95".
    out_size  (H, W): the source is resized first (bilinear, align_corners=False semantics); default (h, w), the input bits.
    out, origins  a uint8 mosaic [Hm, Wm, 3] and one (y, x) per panel: the panels are written into their places, nothing else
              is touched.  Without them a new uint8 [P, H, W, 3].
    Returns   ColorizeOut(rgb, map, stats): the bytes (``out`` when given), the coloured float maps [P, H, W] with ``return_map``
              (None otherwise), and float32 [P, 5] = min, max, sorted[lo], sorted[hi], the percentile as ``np.percentile`` gives it.

    CPU tensors run ``disp_colorize_host``."""
    B, h, w, H, W, panels, offsets, pitch = _colorize_check(maps, panels, out_size, out, origins)
    dev = maps.device
    if dev.type != "cuda":
        return disp_colorize_host(maps, panels, out_size, out, origins, return_map, q)
    P = len(panels)
    if P * H * W >= 2 ** 31 or B * h * w >= 2 ** 31:
        raise RuntimeError("disp_colorize: B h w and panels H W must stay below 2^31; got %d x %d x %d -> %d x %d x %d"
                           % (B, h, w, P, H, W))
    lo, hi, g = percentile_plan(H * W, q)
    table = _colorize_table_cache.get(str(dev), dev, lambda: ([torch.from_numpy(magma_table().copy())], None))[0][0]
    maps = _c(maps)
    native = (N.ColorizePanel * P)(*[N.ColorizePanel(a, b, mode, ref, off) for (a, b, mode, ref), off in zip(panels, offsets)])
    rgb = out if out is not None else torch.empty((P, H, W, 3), device=dev, dtype=torch.uint8)
    fmap = torch.empty((P, H, W), device=dev, dtype=torch.float32)
    stats = torch.empty((P, N.COLORIZE_STATS), device=dev, dtype=torch.float32)
    ws = torch.empty(N.lib().dmh_disp_colorize_ws_size(P), device=dev, dtype=torch.int32)
    N.check(_timed("disp_colorize", lambda: N.lib().dmh_disp_colorize(
        N.ptr(maps), B, h, w, native, P, H, W, lo, hi, g, N.ptr(table), N.ptr(fmap), N.ptr(ws), N.ptr(stats), N.ptr(rgb),
        rgb.numel(), pitch, N.stream()), 4 * P * (4 * H * W + h * w) + 3 * P * H * W))
    return ColorizeOut(rgb, fmap if return_map else None, stats)


# ---------------------------------------------------------------------------------------------------------------- K40
POSE_TRACK_LENGTH = 5       # MD2/evaluate_pose.py:118
PoseAteOut = namedtuple("PoseAteOut", ["ates", "stats"])


def gt_local_poses(gt_global):
    """MD2/evaluate_pose.py:104-114: the KITTI odometry ground truth ``gt_global`` [N + 1, 3, 4] (the rows of ``poses/<seq>.txt``)
    to the N local poses ``inv(dot(inv(G[i - 1]), G[i]))`` of its 4x4 forms, float64 [N, 4, 4], in the reference's own expression.
    Once per sequence, on the host: ground-truth preparation, not per-model work."""
    g = np.asarray(gt_global, dtype=np.float64)
    if g.ndim != 3 or g.shape[1:] != (3, 4) or g.shape[0] < 2:
        raise RuntimeError("gt_local_poses: gt_global must be [N + 1, 3, 4] with N >= 1; got %s" % (g.shape,))
    g = np.concatenate((g, np.zeros((g.shape[0], 1, 4))), 1)
    g[:, 3, 3] = 1
    return np.stack([np.linalg.inv(np.dot(np.linalg.inv(g[i - 1]), g[i])) for i in range(1, len(g))])


def _pose_ate_check(pred_poses, gt_local, track_length):
    """The refusals ``pose_ate`` and ``pose_ate_host`` share; returns N.  Arrays and tensors alike."""
    for name, t, dtype in (("pred_poses", pred_poses, "float32"), ("gt_local", gt_local, "float64")):
        is_t = torch.is_tensor(t)
        if not (is_t or isinstance(t, np.ndarray)):
            raise RuntimeError("pose_ate: %s must be a tensor or an array; got %s" % (name, type(t)))
        if str(t.dtype).split(".")[-1] != dtype:
            raise RuntimeError("pose_ate: %s must be %s; got %s" % (name, dtype, t.dtype))
        if t.ndim != 3 or tuple(t.shape[1:]) != (4, 4):
            raise RuntimeError("pose_ate: %s must be [N, 4, 4]; got %s" % (name, tuple(t.shape)))
        if not (t.is_contiguous() if is_t else t.flags["C_CONTIGUOUS"]):
            raise RuntimeError("pose_ate: %s must be contiguous" % name)
    if len(pred_poses) != len(gt_local):
        raise RuntimeError("pose_ate: %d predicted poses but %d ground-truth local poses" % (len(pred_poses), len(gt_local)))
    if len(pred_poses) == 0:
        raise RuntimeError("pose_ate: no poses")
    if isinstance(track_length, bool) or int(track_length) != track_length or track_length < 2:
        raise RuntimeError("pose_ate: track_length must be an integer >= 2; got %r" % (track_length,))
    return len(pred_poses)


def pose_ate_host(pred_poses, gt_local, track_length=POSE_TRACK_LENGTH):
    """K40's numpy twin, the reference's loop restated (MD2/evaluate_pose.py:23-46, :116-125): ``dump_xyz`` chains ``np.dot`` from
    the identity over ``poses[i:i + track_length - 1]`` -- slices that get shorter at the end of the sequence -- and ``compute_ate``
    aligns by one scale factor and divides the root of the squared error by the point count.  Returns (ates float64 [N], mean,
    np.std).  No guard on an all-zero prediction: 0 / 0 is NaN here as there."""
    _pose_ate_check(pred_poses, gt_local, track_length)
    pred = pred_poses.detach().cpu().numpy() if torch.is_tensor(pred_poses) else pred_poses
    gt = gt_local.detach().cpu().numpy() if torch.is_tensor(gt_local) else gt_local

    def dump_xyz(transformations):
        cam_to_world = np.eye(4)
        xyzs = [cam_to_world[:3, 3]]
        for t in transformations:
            cam_to_world = np.dot(cam_to_world, t)
            xyzs.append(cam_to_world[:3, 3])
        return np.array(xyzs)

    ates = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(len(pred)):
            pred_xyz = dump_xyz(pred[i:i + track_length - 1])
            gt_xyz = dump_xyz(gt[i:i + track_length - 1])
            pred_xyz = pred_xyz + (gt_xyz[0] - pred_xyz[0])[None, :]
            scale = np.sum(gt_xyz * pred_xyz) / np.sum(pred_xyz ** 2)
            ates.append(np.sqrt(np.sum((pred_xyz * scale - gt_xyz) ** 2)) / gt_xyz.shape[0])
    ates = np.array(ates, dtype=np.float64)
    return ates, float(np.mean(ates)), float(np.std(ates))


def pose_ate_launch(pred_poses, gt_local, track_length):
    """K40's two launches on plain device tensors (what ``pose_ate`` and ``torch.ops.dmh.pose_ate`` share)."""
    n = _pose_ate_check(pred_poses, gt_local, track_length)
    _need_cuda(pred_poses)
    if not torch.is_tensor(gt_local) or gt_local.device != pred_poses.device:
        raise RuntimeError("pose_ate: pred_poses and gt_local must share a device")
    if n > 2 ** 24 or track_length > 2 ** 16:
        raise RuntimeError("pose_ate: at most 2^24 poses and a track_length of 2^16; got %d and %d" % (n, track_length))
    ates = torch.empty(n, device=pred_poses.device, dtype=torch.float64)
    stats = torch.empty(2, device=pred_poses.device, dtype=torch.float64)
    N.check(_timed("pose_ate", lambda: N.lib().dmh_pose_ate(N.ptr(pred_poses), N.ptr_f64(gt_local), n, int(track_length), N.ptr_f64(ates),
                                                           N.ptr_f64(stats), N.stream()), 192 * n))
    return ates, stats


def pose_ate(pred_poses, gt_local, track_length=POSE_TRACK_LENGTH):
    """K40: the absolute trajectory error of the KITTI odometry protocol (MD2/evaluate_pose.py:23-46, :116-125) without leaving the
    device.

    pred_poses   float32 [N, 4, 4]: the predicted relative poses, K29's ``T[:, 0]`` of every frame pair, concatenated.
    gt_local     float64 [N, 4, 4]: ``gt_local_poses`` of the sequence; a numpy array is uploaded to pred_poses' device.
    Returns      PoseAteOut(ates float64 [N], stats float64 [2] = mean and np.std of ates), both on the device: nothing is read
                 back until the caller asks.  Snippets at the end of the sequence are shorter, as the reference's slices are.

    Refused with RuntimeError: lengths that differ, N = 0, track_length < 2, a wrong dtype or a non-contiguous operand.
    CPU tensors run ``pose_ate_host``, the reference's loop."""
    _pose_ate_check(pred_poses, gt_local, track_length)
    if not torch.is_tensor(pred_poses):
        raise RuntimeError("pose_ate: pred_poses must be a tensor (pose_ate_host takes arrays)")
    if pred_poses.device.type != "cuda":
        ates, mean, std = pose_ate_host(pred_poses, gt_local, track_length)
        return PoseAteOut(torch.from_numpy(ates), torch.tensor([mean, std], dtype=torch.float64))
    if not torch.is_tensor(gt_local):
        gt_local = torch.from_numpy(gt_local).to(pred_poses.device, non_blocking=True)
    return PoseAteOut(*pose_ate_launch(pred_poses, gt_local, int(track_length)))


# ---------------------------------------------------------------------------------------------------------------- K41
def stem_pair_norm(a, b, weight, mean=0.45, std=0.225):
    """K41: ``conv1((cat([a, b], 1) - mean) / std)`` for the pose encoder's first layer (MD2/evaluate_pose.py:94-96 into
    MD2/networks/resnet_encoder.py:89-90 with num_input_images = 2: 6 -> 64 channels, 7x7, stride 2, padding 3, no bias) without
    the concatenation and without the normalised copy.  ``a`` and ``b`` are [B, 3, H, W] with even H and W; they may be overlapping
    views of one tensor (``f[:-1]`` and ``f[1:]``).  Forward only: a call that would need a gradient is refused."""
    for name, t in (("a", a), ("b", b), ("weight", weight)):
        _need_f32(t, name)
    _need_cuda(a)
    if (a.dim() != 4 or a.shape[1] != 3 or a.shape != b.shape or a.shape[2] % 2 or a.shape[3] % 2 or a.shape[0] == 0
            or tuple(weight.shape) != (64, 6, 7, 7)):
        raise RuntimeError("stem_pair_norm: a and b must be [B,3,H,W] with B >= 1 and even H, W, and weight [64,6,7,7]; got %s, %s, %s"
                           % (tuple(a.shape), tuple(b.shape), tuple(weight.shape)))
    if b.device != a.device or weight.device != a.device:
        raise RuntimeError("stem_pair_norm: a, b and weight must share a device")
    if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad or weight.requires_grad):
        raise RuntimeError("stem_pair_norm is forward only (K41 has no backward): call it under torch.no_grad(), or take "
                           "ResnetEncoder.forward(torch.cat([a, b], 1)), which differentiates")
    if not std > 0:
        raise RuntimeError("stem_pair_norm: std must be positive; got %r" % (std,))
    a, b, weight = _c(a.detach()), _c(b.detach()), _c(weight.detach())
    B, _, H, W = a.shape
    y = torch.empty((B, 64, H // 2, W // 2), device=a.device, dtype=torch.float32)
    N.check(_timed("stem_pair_fwd", lambda: N.lib().dmh_stem_pair_norm_fwd(N.ptr(a), N.ptr(b), N.ptr(weight), B, H, W, float(mean),
                                                                          float(std), N.ptr(y), N.stream()),
                   4 * (2 * a.numel() + 3 * y.numel()), 2 * 294 * y.numel()))
    return y
