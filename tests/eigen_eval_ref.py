"""CPU restatement of the reference's benign evaluation protocol, a test helper.

Reference: MD2/evaluate_depth.py -- ``compute_errors`` (unmasked branch :61-76), ``batch_post_process_disparity`` :102-110, and
the per-image loop of ``evaluate`` :351-391.  ``cv2.resize`` (INTER_LINEAR, no antialiasing) is restated from OpenCV's source
(modules/imgproc/src/resize.cpp, the float path), because OpenCV is not a dependency of this project:

    per axis   scale = src / dst in double,  f = float32((d + 0.5) * scale - 0.5),  s = floor(f),  f -= s  (fp32)
               s < 0: s = 0, f = 0;   s >= src - 1: s = src - 1, f = 0;   the second tap is min(s + 1, src - 1)
    weights    (1 - f, f) in fp32
    value      horizontal pass first: S = a0 src[sx] + a1 src[sx + 1] on both rows, then dst = b0 S0 + b1 S1

``resize`` evaluates this in the dtype asked for (float32: what the kernel does, up to fused multiply-adds; float64: the exact
value of the formula for the same fp32-rounded weights); ``resize_direct`` is a second, scalar evaluation of the same formula in
float64 that shares no code with it beyond the axis rule being stated twice.

Also here, because the fixture generator (tools/make_goldens_eval.py) and the tests must agree on them: the fixture's inputs
(``pp_pairs``, ``metric_vectors``).
"""
import math

import numpy as np

MIN_DEPTH, MAX_DEPTH = 1e-3, 80
STEREO_SCALE_FACTOR = 5.4
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)


# ------------------------------------------------------------------------------------------------------------ the reference's pieces
def compute_errors(gt, pred):
    """:61-76 (mask=None) in the arrays' own dtype: abs_err, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3."""
    thresh = np.maximum(gt / pred, pred / gt)
    a1, a2, a3 = [(thresh < t).mean() for t in THRESHOLDS]
    d = gt - pred
    return (np.mean(np.abs(d)), np.mean(np.abs(d) / gt), np.mean(d ** 2 / gt), np.sqrt((d ** 2).mean()),
            np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean()), a1, a2, a3)


def left_mask(w):
    """:107-108: 1 - clip(20 (l - 0.05), 0, 1) over l = linspace(0, 1, w), float64."""
    return 1.0 - np.clip(20 * (np.linspace(0, 1, w) - 0.05), 0, 1)


def post_process(l_disp, r_disp):
    """:102-110 on [n, h, w] arrays; ``r_disp`` is already mirrored back.  float64, as numpy's promotion makes it."""
    w = l_disp.shape[-1]
    l_mask = left_mask(w)[None, None, :]
    r_mask = l_mask[:, :, ::-1]
    return r_mask * l_disp + l_mask * r_disp + (1.0 - l_mask - r_mask) * (0.5 * (l_disp + r_disp))


def crop_bounds(gt_h, gt_w):
    """:363-364."""
    return np.array([0.40810811 * gt_h, 0.99189189 * gt_h, 0.03594771 * gt_w, 0.96405229 * gt_w]).astype(np.int32)


def valid_mask(gt, split):
    """:360-370."""
    if split != "eigen":
        return gt > 0
    mask = np.logical_and(gt > np.float32(MIN_DEPTH), gt < MAX_DEPTH)
    c = crop_bounds(*gt.shape)
    crop = np.zeros(gt.shape, dtype=bool)
    crop[c[0]:c[1], c[2]:c[3]] = True
    return np.logical_and(mask, crop)


# ------------------------------------------------------------------------------------------------------------ cv2.resize, restated
def lin_axis(dst, src):
    """(s0, s1, f) of every destination index of one axis; f is float32."""
    scale = float(src) / float(dst)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    return s, np.minimum(s + 1, src - 1), f


def resize(src, gt_h, gt_w, dtype=np.float64):
    """``src`` [h, w] at gt_h x gt_w.  The weights are fp32 values in every dtype; the products and sums are in ``dtype``."""
    h, w = src.shape
    sx, sx1, fx = lin_axis(gt_w, w)
    sy, sy1, fy = lin_axis(gt_h, h)
    a0, a1 = (np.float32(1) - fx).astype(dtype), fx.astype(dtype)
    b0, b1 = (np.float32(1) - fy).astype(dtype)[:, None], fy.astype(dtype)[:, None]
    s = src.astype(dtype)
    rows = s[:, sx] * a0 + s[:, sx1] * a1
    return (rows[sy] * b0 + rows[sy1] * b1).astype(dtype)


def resize_direct(src, gt_h, gt_w, ys=None, xs=None):
    """The stated formula pixel by pixel in Python floats (float64), weights rounded to float32 first."""
    h, w = src.shape

    def axis(d, n_src, n_dst):
        f = float(np.float32((d + 0.5) * (float(n_src) / float(n_dst)) - 0.5))
        s = math.floor(f)
        f = float(np.float32(np.float32(f) - np.float32(s)))
        if s < 0:
            s, f = 0, 0.0
        if s >= n_src - 1:
            s, f = n_src - 1, 0.0
        return s, min(s + 1, n_src - 1), f
    ys = range(gt_h) if ys is None else ys
    xs = range(gt_w) if xs is None else xs
    out = np.zeros((len(ys), len(xs)))
    for i, y in enumerate(ys):
        y0, y1, fy = axis(y, h, gt_h)
        b0, b1 = float(np.float32(1) - np.float32(fy)), fy
        for j, x in enumerate(xs):
            x0, x1, fx = axis(x, w, gt_w)
            a0, a1 = float(np.float32(1) - np.float32(fx)), fx
            top = a0 * float(src[y0, x0]) + a1 * float(src[y0, x1])
            bot = a0 * float(src[y1, x0]) + a1 * float(src[y1, x1])
            out[i, j] = b0 * top + b1 * bot
    return out


def post_process_taps(l_disp, flip_disp):
    """What K25 resizes under --post_process: the blend of :102-110 at network resolution with the masks rounded to float32
    (the kernel's weights), float64 otherwise.  ``flip_disp`` is the prediction of the mirrored frame, not mirrored back."""
    w = l_disp.shape[-1]
    lm = left_mask_exact(w).astype(np.float32)
    rm = lm[::-1]
    l, r = l_disp.astype(np.float64), flip_disp[..., ::-1].astype(np.float64)
    mid = (np.float32(1) - lm - rm).astype(np.float64)
    return rm.astype(np.float64) * l + lm.astype(np.float64) * r + mid * (0.5 * (l + r))


def left_mask_exact(w):
    """The left mask over x / (w - 1) (what linspace states, without its multiplication by a rounded step)."""
    t = np.arange(w, dtype=np.float64) / (w - 1) if w > 1 else np.zeros(1)
    return 1.0 - np.clip(20 * (t - 0.05), 0, 1)


# ------------------------------------------------------------------------------------------------------------ the loop :351-391
def evaluate_loop(pred_disps, gt_depths, split, scale_factor=1.0, median_scaling=True, dtype=np.float64):
    """(errors [N, 8], ratios [N]) of the reference's loop in ``dtype``; an image without a valid pixel gives NaN."""
    errors, ratios = [], []
    for disp, gt in zip(pred_disps, gt_depths):
        gt = np.asarray(gt)
        depth = 1 / resize(np.asarray(disp), gt.shape[0], gt.shape[1], dtype)
        mask = valid_mask(gt, split)
        e, r = image_errors(gt[mask].astype(dtype), depth[mask] * dtype(scale_factor), median_scaling)
        errors.append(e)
        ratios.append(r)
    return np.array(errors, dtype=np.float64), np.array(ratios, dtype=np.float64)


def image_errors(gt, pred, median_scaling=True, ratio=None):
    """:375-384 on the valid values; ``ratio``: use this one instead of the medians'."""
    if gt.size == 0:
        return (np.nan,) * 8, np.nan
    if median_scaling and ratio is None:
        ratio = np.median(gt) / np.median(pred)
    if median_scaling:
        pred = pred * ratio
    pred = np.clip(pred, pred.dtype.type(MIN_DEPTH), pred.dtype.type(MAX_DEPTH))
    return compute_errors(gt, pred), (ratio if median_scaling else np.nan)


def near_threshold(gt, pred, rel=1e-5):
    """Per threshold, the number of elements whose max(gt / pred, pred / gt) lies within ``rel`` (relative) of it."""
    th = np.maximum(gt / pred, pred / gt).astype(np.float64)
    return [int((np.abs(th - t) <= rel * t).sum()) for t in THRESHOLDS]


# ------------------------------------------------------------------------------------------------------------ fixture inputs
PP_SHAPE = (24, 80)


def pp_pairs(seed=5, n=3):
    """(l_disp, r_disp) [n, 24, 80] float32: smooth disparities in (0.01, 1) and an independent second view."""
    rng = np.random.RandomState(seed)
    h, w = PP_SHAPE
    ys, xs = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    out = []
    for _ in range(2):
        base = 0.02 + 0.5 * ys[None] * (1 + 0.3 * np.sin(5 * xs[None] + 6.3 * rng.rand(n, 1, 1)))
        out.append((base * (1 + 0.2 * rng.rand(n, h, w))).astype(np.float32))
    return out[0], out[1]


def metric_vectors(seed=9, sizes=(1, 2, 777, 4096)):
    """(gt, disp) pairs of float32 vectors; pred = float32(1) / disp lies in [1e-3, 80] and no max(gt / pred, pred / gt) lies
    within 1e-4 (relative) of a threshold, so that a1..a3 do not depend on the last bits of a division."""
    rng = np.random.RandomState(seed)
    out = []
    for n in sizes:
        gt = np.exp(rng.uniform(np.log(1.0), np.log(79.0), 4 * n + 16)).astype(np.float32)
        pred = np.clip(gt.astype(np.float64) * np.exp(rng.normal(0, 0.35, gt.size)), 0.5, 79.5)
        disp = (1.0 / pred).astype(np.float32)
        pred = (np.float32(1) / disp).astype(np.float64)
        th = np.maximum(gt / pred, pred / gt)
        keep = np.all([np.abs(th - t) > 1e-4 * t for t in THRESHOLDS], 0)
        out.append((gt[keep][:n].copy(), disp[keep][:n].copy()))
        assert out[-1][0].size == n
    return out


# ------------------------------------------------------------------------------------------------------------ the GPU tests' cases
def smooth_disp(rng, n, h, w):
    """[n, h, w] float32 disparities in about (0.02, 0.7): a ramp towards the bottom row, a lateral wave, 10 % texture."""
    ys, xs = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    base = 0.02 + 0.5 * ys[None] * (1 + 0.3 * np.sin(5 * xs[None] + 6.3 * rng.rand(n, 1, 1)))
    return (base * (1 + 0.1 * rng.rand(n, h, w))).astype(np.float32)


def lidar_gt(rng, gh, gw, density, parity=None):
    """fp32 map: ``density`` of the pixels carry 0.0005 .. 90 m (log-uniform: both ends of the range mask bite), the rest 0.
    ``parity``: the number of valid pixels under split eigen is made even (0) or odd (1) by clearing one of them."""
    gt = np.where(rng.rand(gh, gw) < density, np.exp(rng.uniform(np.log(5e-4), np.log(90.0), (gh, gw))), 0.0).astype(np.float32)
    if parity is not None and int(valid_mask(gt, "eigen").sum()) % 2 != parity:
        y, x = np.argwhere(valid_mask(gt, "eigen"))[0]
        gt[y, x] = 0
    return gt


def batch_cases(seed=3):
    """name -> (split, pred_disp [n, h, w], flip_disp [n, h, w], [gt maps]): the shapes of the GPU tests."""
    rng = np.random.RandomState(seed)
    cases = {}
    # up-scaling by non-integer factors, ragged sizes, an odd width; even and odd counts; one map whose valid values are all equal
    gts = [lidar_gt(rng, 37, 122, 0.6, parity=0), lidar_gt(rng, 38, 121, 0.05, parity=1), None, lidar_gt(rng, 37, 122, 0.3)]
    gts[2] = np.where(rng.rand(36, 124) < 0.4, np.float32(12.5), np.float32(0)).astype(np.float32)
    cases["up"] = ("eigen", smooth_disp(rng, 4, 24, 80), smooth_disp(rng, 4, 24, 80), gts)
    # down-scaling
    cases["down"] = ("eigen", smooth_disp(rng, 1, 48, 160), smooth_disp(rng, 1, 48, 160), [lidar_gt(rng, 37, 122, 0.5)])
    # a crop that leaves one valid pixel (the others lie outside it or outside the range), and a map without a valid pixel
    one = np.zeros((37, 122), dtype=np.float32)
    one[:15] = 20.0                     # in range, above the crop
    one[:, :4] = 30.0                   # in range, left of the crop
    one[20:30, 50:60] = 85.0            # inside the crop, out of range
    one[25, 70] = 17.0
    none = np.zeros((38, 121), dtype=np.float32)
    none[:15] = 20.0
    assert int(valid_mask(one, "eigen").sum()) == 1 and int(valid_mask(none, "eigen").sum()) == 0
    cases["edge"] = ("eigen", smooth_disp(rng, 3, 24, 80), smooth_disp(rng, 3, 24, 80), [one, none, lidar_gt(rng, 37, 122, 0.3)])
    # every pixel valid (another split): the first and last rows and columns, where the clamps of the resize act
    dense = np.exp(rng.uniform(np.log(0.5), np.log(90.0), (37, 122))).astype(np.float32)
    cases["border"] = ("eigen_benchmark", smooth_disp(rng, 1, 24, 80), smooth_disp(rng, 1, 24, 80), [dense])
    return cases


def straddle_values():
    """Three (lo, hi) pairs of neighbouring float32 values in [2, 4) whose integer keys differ first in the digit of pass 0
    (the top 11 bits), of pass 1 (the next 11) and of pass 2 (the last 10)."""
    two = int(np.float32(2.0).view(np.uint32))
    pairs = []
    for hi_bits in (int(np.float32(2.5).view(np.uint32)), two + 0x400, two + 2):
        lo, hi = np.uint32(hi_bits - 1).view(np.float32), np.uint32(hi_bits).view(np.float32)
        pairs.append((lo, hi))
    key = lambda v: int(np.float32(v).view(np.uint32)) | 0x80000000     # noqa: E731
    (a, b), (c, d), (e, f) = pairs
    assert key(a) >> 21 != key(b) >> 21
    assert key(c) >> 21 == key(d) >> 21 and key(c) >> 10 != key(d) >> 10
    assert key(e) >> 10 == key(f) >> 10 and key(e) != key(f)
    return pairs


def disp_for_depth(target):
    """A float32 disparity whose fp32 reciprocal is exactly ``target`` (in [2, 4): every value there is one)."""
    guess = int((np.float32(1) / np.float32(target)).view(np.uint32))
    for bits in range(guess - 4, guess + 5):
        d = np.uint32(bits).view(np.float32)
        if np.float32(1) / d == np.float32(target):
            return d
    raise AssertionError("no disparity gives depth %r" % target)


def straddle_case(seed=13, shape=(6, 40)):
    """(pred_disp [3, 6, 40], [gt maps]) for split None with pred and gt of one size (the resize is the identity): in image k
    100 depths are the lo and 100 the hi value of pair k, 20 are smaller and 20 larger, shuffled -- the two middle ranks are
    duplicated values in neighbouring bins of pass k.  The ground-truth maps hold the same arrangement of the values."""
    rng = np.random.RandomState(seed)
    n = shape[0] * shape[1]
    assert n == 240
    disps, gts = [], []
    for lo, hi in straddle_values():
        disp = np.concatenate([np.full(100, disp_for_depth(lo)), np.full(100, disp_for_depth(hi)),
                               np.linspace(0.55, 0.9, 20), np.linspace(0.26, 0.3, 20)]).astype(np.float32)    # 1.1 .. 1.8, 3.3 .. 3.8 m
        disp = disp[rng.permutation(n)]
        values = np.float32(1) / disp
        disps.append(disp.reshape(shape))
        gts.append(values[::-1].copy().reshape(shape))
    return np.stack(disps), gts


def reference_run(case, post_process=False, scale_factor=1.0, median_scaling=True):
    """The float64 loop on one of ``batch_cases``: (errors, ratios, [depth maps before the factor], [valid masks])."""
    split, disp, flip, gts = case
    taps = post_process_taps(disp, flip) if post_process else disp.astype(np.float64)
    depths = [1 / resize(taps[i], g.shape[0], g.shape[1]) for i, g in enumerate(gts)]
    masks = [valid_mask(g, split) for g in gts]
    out = [image_errors(g[m].astype(np.float64), d[m] * scale_factor, median_scaling) for g, d, m in zip(gts, depths, masks)]
    return np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.float64), depths, masks
