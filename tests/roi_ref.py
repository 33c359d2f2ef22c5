"""K19 in plain float64 numpy, written from DESIGN.md section K19 and not from the kernels: the windowed decoder glue and its
exact adjoint BY SCATTER (the kernels gather), the windowed cost, the crops, the paste and the windowed stem backward -- and
the geometries, source forms and inputs of tests/test_gpu_roi_anchor.py, so that tests/test_roi_ref.py can hold both the
reference and the cases' input conditions without a GPU.

    glue   out[b, :, i, j] = pad1_reflect(cat(up2_nearest(ELU(y)), skip))[b, :, oy_b + i, ox_b + j]       (padded coordinates)
    cost   sum_b sum_window (sigmoid(d) * mask_window)^2 / (B H W)
    stem   g_z = scale[c] [feat > 0] (g_feat + adjoint of MaxPool2d(3, 2, 1) through the argmax byte ky * 3 + kx)
"""
import numpy as np


# ---- the glue ---------------------------------------------------------------------------------------------------------------------

def elu(y):
    return np.where(y > 0, y, np.expm1(np.minimum(y, 0)))


def elu_grad(y):
    return np.where(y > 0, 1.0, np.exp(np.minimum(y, 0)))


def padded_frame(y, skip, up, apply_elu):
    """pad1_reflect(cat(up2_nearest(ELU(y)), skip)) of whole frames: [B, C1 + C2, FH + 2, FW + 2]."""
    e = elu(y) if apply_elu else y
    if up:
        e = e.repeat(2, axis=2).repeat(2, axis=3)
    p = e if skip is None else np.concatenate([e, skip], axis=1)
    return np.pad(p, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect")


def cut(full, org, size):
    """The per-sample windows ``full[b, :, oy_b : oy_b + h, ox_b : ox_b + w]`` stacked."""
    h, w = size
    return np.stack([full[b, :, oy:oy + h, ox:ox + w] for b, (oy, ox) in enumerate(np.asarray(org))])


def embed(win, org, shape, fill=0.0):
    """The inverse of cut(): windows written into a frame of ``shape`` that holds ``fill`` elsewhere."""
    full = np.full(shape, fill, dtype=win.dtype)
    h, w = win.shape[2:]
    for b, (oy, ox) in enumerate(np.asarray(org)):
        full[b, :, oy:oy + h, ox:ox + w] = win[b]
    return full


def glue_fwd(y, skip, up, apply_elu, dst_org, size):
    """``y`` / ``skip``: whole frames in float64.  The window at padded position dst_org of hc + 2 rows, wc + 2 columns."""
    return cut(padded_frame(np.asarray(y, np.float64), None if skip is None else np.asarray(skip, np.float64), up, apply_elu),
               dst_org, (size[0] + 2, size[1] + 2))


def pad_source(n):
    """Frame index that each of the n + 2 padded indices reads (ReflectionPad2d(1))."""
    i = np.abs(np.arange(-1, n + 1))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def window_sources(oy, ox, size, frame):
    """Index map of one window: frame row of each window row, frame column of each window column."""
    return pad_source(frame[0])[oy:oy + size[0] + 2], pad_source(frame[1])[ox:ox + size[1] + 2]


def glue_bwd(g_out, y, n_skip, up, apply_elu, dst_org, size, frame):
    """The adjoint of glue_fwd by scatter: every window entry adds its gradient to the source element it read.

    Returns whole-frame float64 g_y (times elu'(y)) and g_skip, the same scatter over |g_out| (S_y, S_skip: the S of
    tests/util.py assert_round_bound) and the number of window entries that read each element (n_y [B, sh, sw], n_skip
    [B, FH, FW]): where that is 0 the gradient is an exact zero."""
    g_out, y = np.asarray(g_out, np.float64), np.asarray(y, np.float64)
    B, C1 = y.shape[:2]
    FH, FW = frame
    assert y.shape[2:] == ((FH // 2, FW // 2) if up else (FH, FW)) and g_out.shape == (B, C1 + n_skip, size[0] + 2, size[1] + 2)
    g_y, S_y, n_y = np.zeros(y.shape), np.zeros(y.shape), np.zeros((B,) + y.shape[2:], np.int64)
    g_k, S_k, n_k = np.zeros((B, n_skip, FH, FW)), np.zeros((B, n_skip, FH, FW)), np.zeros((B, FH, FW), np.int64)
    for b, (oy, ox) in enumerate(np.asarray(dst_org)):
        rows, cols = window_sources(oy, ox, size, frame)
        Y, X = np.meshgrid(rows, cols, indexing="ij")
        ys, xs = (Y >> 1, X >> 1) if up else (Y, X)
        c = np.arange(C1)[:, None, None]
        np.add.at(g_y[b], (c, ys[None], xs[None]), g_out[b, :C1])
        np.add.at(S_y[b], (c, ys[None], xs[None]), np.abs(g_out[b, :C1]))
        np.add.at(n_y[b], (ys, xs), 1)
        if n_skip:
            c = np.arange(n_skip)[:, None, None]
            np.add.at(g_k[b], (c, Y[None], X[None]), g_out[b, C1:])
            np.add.at(S_k[b], (c, Y[None], X[None]), np.abs(g_out[b, C1:]))
        np.add.at(n_k[b], (Y, X), 1)
    if apply_elu:
        d = elu_grad(y)
        g_y, S_y = g_y * d, S_y * d
    return dict(g_y=g_y, g_skip=g_k, S_y=S_y, S_skip=S_k, n_y=n_y, n_skip=n_k)


def source_boxes(dst_org, size, frame, up):
    """Per sample the tight box [lo, hi) of the source elements its destination window reads: two [B, 2] arrays."""
    lo, hi = [], []
    for oy, ox in np.asarray(dst_org):
        rows, cols = window_sources(oy, ox, size, frame)
        if up:
            rows, cols = rows >> 1, cols >> 1
        lo.append((rows.min(), cols.min()))
        hi.append((rows.max() + 1, cols.max() + 1))
    return np.array(lo), np.array(hi)


def covering_boxes(dst_org, size, frame, up, even):
    """One rectangle size for all samples and an origin per sample such that each rectangle lies in its plane and holds the
    sample's source_boxes() box; ``even``: origins and width even (the two-wide kernel's alignment), otherwise the width is
    odd (the one-element kernel).  The y_region / skip_region of dmh_roi_glue_bwd."""
    lo, hi = source_boxes(dst_org, size, frame, up)
    plane = (frame[0] >> 1, frame[1] >> 1) if up else tuple(frame)
    if even:
        lo = lo.copy()
        lo[:, 1] &= ~1
    ext = (hi - lo).max(axis=0)
    ext[1] += (ext[1] & 1) if even else 1 - (ext[1] & 1)
    org = np.minimum(lo, np.array(plane) - ext)
    if even:
        org[:, 1] &= ~1
    assert (org >= 0).all() and (org <= lo).all() and (org + ext >= hi).all() and (org + ext <= np.array(plane)).all()
    return org.astype(np.int32), (int(ext[0]), int(ext[1]))


# ---- split_rc of csrc/roi_glue.hip in Python integers ----------------------------------------------------------------------------------

def split_magic(w2):
    """The launchers' ``(unsigned)((1 << 32) / w2) + 1u``."""
    return ((1 << 32) // w2 + 1) & 0xFFFFFFFF


def split_rc(t, w2, magic, correct=True):
    """(row, column, took the correction branch) of the flat index ``t`` at ``w2`` columns; numpy uint64 arrays or ints."""
    t = np.asarray(t, dtype=np.uint64)
    if w2 == 1:
        return t.astype(np.int64), np.zeros(t.shape, np.int64), np.zeros(t.shape, bool)
    r = ((t * np.uint64(magic)) >> np.uint64(32)).astype(np.int64)          # __umulhi: t < 2^30, magic < 2^32
    t = t.astype(np.int64)
    over = r * w2 > t
    if correct:
        r = r - over
    return r, t - r * w2, over


# ---- cost ---------------------------------------------------------------------------------------------------------------------------------

def sigmoid(d):
    return 1.0 / (1.0 + np.exp(-np.asarray(d, np.float64)))


def cost_fwd(d, mask, org):
    """``d`` [B, hd, wd] pre-activations of the windows, ``mask`` [B, H, W], ``org`` [B, 2]: (cost, sigmoid(d))."""
    B, hd, wd = d.shape
    s = sigmoid(d)
    m = cut(np.asarray(mask, np.float64)[:, None], org, (hd, wd))[:, 0]
    return float(((s * m) ** 2).sum() / (B * mask.shape[1] * mask.shape[2])), s


def cost_bwd(sig, mask, org, gscale):
    """d (gscale * cost) / d d from the stored sigmoid: gscale * 2 s m^2 s (1 - s) / (B H W)."""
    s = np.asarray(sig, np.float64)
    B, hd, wd = s.shape
    m = cut(np.asarray(mask, np.float64)[:, None], org, (hd, wd))[:, 0]
    return gscale * 2.0 * s * m * m * s * (1.0 - s) / (B * mask.shape[1] * mask.shape[2])


# ---- crop, paste, the windowed stem backward ----------------------------------------------------------------------------------------------

def crop(src, org, size, gate=None, gate_compact=False, src_compact=False):
    """src's windows (``src_compact``: src is the windows already, the kernel's mode 2), zeroed where the gate (whole-frame, or
    compact like the output) is <= 0."""
    out = src if src_compact else cut(src, org, size)
    if gate is not None:
        out = np.where((gate if gate_compact else cut(gate, org, size)) > 0, out, 0)
    return out


def paste(dst, src, win_org, size, src_org=None):
    """dst with the window ``size`` at win_org taken from src: a compact window at frame origin src_org, or a whole frame."""
    out = dst.copy()
    h, w = size
    for b, (oy, ox) in enumerate(np.asarray(win_org)):
        sy, sx = (oy, ox) if src_org is None else (oy - src_org[b][0], ox - src_org[b][1])
        out[b, :, oy:oy + h, ox:ox + w] = src[b, :, sy:sy + h, sx:sx + w]
    return out


def pool_adjoint(g_pool, argmax, H, W):
    """Adjoint of MaxPool2d(3, 2, 1) on an H x W map: every pooled cell adds its gradient to the element its argmax byte
    (ky * 3 + kx) names, (2 i - 1 + ky, 2 j - 1 + kx)."""
    B, C, PH, PW = g_pool.shape
    assert (PH, PW) == (H // 2, W // 2) and argmax.shape == g_pool.shape
    a = argmax.astype(np.int64)
    b, c, i, j = np.meshgrid(np.arange(B), np.arange(C), np.arange(PH), np.arange(PW), indexing="ij")
    ty, tx = 2 * i - 1 + a // 3, 2 * j - 1 + a % 3
    assert (a < 9).all() and (ty >= 0).all() and (ty < H).all() and (tx >= 0).all() and (tx < W).all()
    out = np.zeros((B, C, H, W))
    np.add.at(out, (b, c, ty, tx), np.asarray(g_pool, np.float64))
    return out


def stem_bwd_win(feat, argmax, g_feat, g_pool_win, scale, org, pool_org, size):
    """(g_z, S) on the ``size`` window at ``org`` of the 1/2 map; g_pool_win is the compact window at pool_org of the 1/4
    map's gradient and counts as zero outside it.  S: the same with every term's magnitude."""
    B, C, H, W = feat.shape
    g_pool_win = np.asarray(g_pool_win, np.float64)
    full = embed(g_pool_win, pool_org, (B, C, H // 2, W // 2))
    gate = (feat > 0) * np.asarray(scale, np.float64)[None, :, None, None]
    g = pool_adjoint(full, argmax, H, W)
    S = pool_adjoint(np.abs(full), argmax, H, W)
    if g_feat is not None:
        g, S = g + g_feat, S + np.abs(g_feat)
    return cut(g * gate, org, size), cut(S * np.abs(gate), org, size)


# ---- the geometries and source forms of tests/test_gpu_roi_anchor.py -------------------------------------------------------------------

def _corners(frame, size, inner):
    (FH, FW), (hc, wc) = frame, size
    return [(0, 0), (FH - hc, FW - wc), (0, FW - wc), inner, (FH - hc, 0)]


GEOMETRIES = {
    # name: (destination frame, window, origins); every origin even
    "G1": ((24, 40), (10, 12), _corners((24, 40), (10, 12), (6, 14))),
    "G1e": ((24, 40), (10, 12), [(0, 14), (14, 14), (6, 0), (6, 28)]),   # one border each: tight windows of even width at top / bottom
    "G2a": ((4, 4), (2, 2), [(0, 0), (2, 2), (0, 2), (2, 0)]),
    "G2b": ((4, 4), (4, 4), [(0, 0)]),                                   # the window is the frame
    "G3a": ((40, 64), (30, 46), _corners((40, 64), (30, 46), (4, 8))),   # PW / 2 = 24: three blocks
    "G3b": ((40, 64), (38, 62), [(0, 0), (2, 2), (0, 2), (2, 0)]),       # PW / 2 = 32
    "G4a": ((23, 41), (11, 12), [(0, 0), (12, 0), (6, 14), (12, 28), (0, 28)]),      # odd frame: up = 0 only
    "G4b": ((24, 42), (10, 12), _corners((24, 42), (10, 12), (6, 14))),              # up = 1: the source is 12 x 21
    "G5": ((1100, 4096), (1098, 4094), [(0, 0), (2, 2)]),                # one sample per launch (see glue_groups)
}

# (geometry, C1, C2, up, elu, y windowed, skip: None / "whole" / "win")
GLUE_CASES = [
    ("G1", 6, 4, 1, 1, False, "whole"),
    ("G1", 8, 4, 1, 1, True, "win"),
    ("G1", 8, 16, 1, 0, False, "win"),
    ("G1", 16, 0, 0, 1, True, None),
    ("G1", 3, 5, 0, 0, False, "whole"),
    ("G1", 8, 16, 0, 1, True, "whole"),
    ("G1", 8, 4, 0, 0, False, "win"),
    ("G1e", 8, 16, 1, 1, True, "win"),
    ("G1e", 8, 4, 0, 1, True, "win"),
    ("G3a", 8, 16, 1, 1, True, "win"),
    ("G3a", 6, 4, 0, 1, False, "whole"),
    ("G3a", 8, 4, 1, 0, False, "win"),
    ("G3a", 16, 0, 0, 0, True, None),
    ("G3b", 16, 0, 1, 1, True, None),
    ("G3b", 3, 5, 1, 1, True, "win"),
    ("G3b", 8, 16, 0, 0, False, "whole"),
    ("G2a", 6, 4, 1, 1, False, "whole"),
    ("G2a", 3, 5, 0, 1, True, "win"),
    ("G2b", 8, 16, 1, 0, False, "whole"),
    ("G2b", 8, 4, 0, 1, False, "whole"),
    ("G4a", 6, 4, 0, 1, False, "whole"),
    ("G4a", 16, 0, 0, 0, False, None),
    ("G4b", 8, 4, 1, 1, False, "whole"),
    ("G4b", 3, 5, 1, 0, True, "win"),
]
G5_CASE = ("G5", 1, 0, 0, 0, False, None)

# whole-frame sources with y_region / skip_region: (geometry, C1, C2, up, elu, even rectangles)
RECT_CASES = [
    ("R1", 8, 4, 1, 1, True),
    ("R1", 6, 4, 0, 1, True),
    ("R1", 6, 4, 1, 0, False),        # an odd rectangle width: the one-element kernel
]
RECT_GEOMETRY = ((40, 64), (10, 12), [(0, 0), (30, 52), (14, 20), (30, 0), (8, 52)])     # (30, 52): flush bottom-right


# cost: (window hd x wd, mask frame H x W, origins -- the last one flush with the frame's bottom-right corner)
COST_CASES = [
    ((6, 10), (16, 24), [(0, 0), (3, 5), (10, 14)]),                  # one block
    ((40, 64), (48, 80), [(1, 2), (0, 7), (8, 16)]),                  # three blocks
    ((130, 520), (140, 540), [(0, 0), (7, 13), (10, 20)]),            # 67,600 elements: the 64-block cap, the grid-stride loop
]

# crop: windows in a 32 x 64 frame at the four corners and inside (even origins and widths)
CROP_FRAME = (32, 64)
CROP_WINDOWS = [(6, 8), (24, 44)]
CROP_CHANNELS = [6, 8, 16]

# paste: windows (odd sizes and origins allowed) in a 24 x 40 frame
PASTE_FRAME = (24, 40)
PASTE_WINDOWS = [(5, 7), (20, 30)]
PASTE_CHANNELS = [6, 16]

# windowed stem backward: (1/2-map H x W, window hs x ws)
STEM_CASES = [((16, 24), (6, 8)), ((40, 64), (20, 36))]


def corner_origins(frame, size, inner):
    (H, W), (h, w) = frame, size
    return np.array([(0, 0), (0, W - w), (H - h, 0), (H - h, W - w), inner], np.int32)


def stem_windows(frame, size):
    """Origins of the 1/2-map windows (every corner, one inside) and the 1/4-map windows of g_pool: hs / 2 x ws / 2 cells, the
    cells of the window's own quads -- so the cells below and right of the window that its last quads read lie outside it --
    and, for the inner sample, shifted by (1, 1) so that its first row and column of cells lie outside as well."""
    (H, W), (hs, ws) = frame, size
    org = corner_origins(frame, size, (4, 6))
    hq, wq = hs // 2, ws // 2
    pool_org = org // 2
    pool_org[4] += 1
    assert (org % 2 == 0).all() and (pool_org >= 0).all() and (pool_org + (hq, wq) <= (H // 2, W // 2)).all()
    return org, pool_org, (hq, wq)


def stem_cells_outside(frame, size):
    """Per sample: the pooled cells its window's quads read (cells i and i + 1 of quad row i, inside the 1/4 map) that lie
    outside its g_pool window."""
    org, pool_org, (hq, wq) = stem_windows(frame, size)
    out = []
    for (oy, ox), (py, px) in zip(org, pool_org):
        ci = np.arange(oy // 2, min(oy // 2 + size[0] // 2 + 1, frame[0] // 2))
        cj = np.arange(ox // 2, min(ox // 2 + size[1] // 2 + 1, frame[1] // 2))
        oi, oj = (ci < py) | (ci >= py + hq), (cj < px) | (cj >= px + wq)
        out.append(int(oi.sum() * len(cj) + oj.sum() * len(ci) - oi.sum() * oj.sum()))
    return out


def case_id(case):
    geo, C1, C2, up, el, ywin, skip = case
    return "%s-%dx%d-up%d-elu%d-y%s-skip%s" % (geo, C1, C2, up, el, "win" if ywin else "whole", skip or "none")


def fwd_group(C1, C2):
    """Channel planes per thread of roi_glue_fwd_kernel, as dmh_roi_glue_fwd chooses them."""
    return 8 if C1 % 8 == 0 and C2 % 8 == 0 else (4 if C1 % 4 == 0 and C2 % 4 == 0 else 1)


def borders(origin, size, frame):
    """Which of the frame's borders the window at ``origin`` touches; ("interior",) if none."""
    (oy, ox), (hc, wc), (FH, FW) = origin, size, frame
    b = [n for n, on in (("top", oy == 0), ("bottom", oy + hc == FH), ("left", ox == 0), ("right", ox + wc == FW)) if on]
    return tuple(b) or ("interior",)


def glue_inputs(case, seed=0):
    """Whole-frame fp32 inputs of a case: y [B, C1, sh, sw], skip [B, C2, FH, FW] or None, g_out [B, C, hc + 2, wc + 2], dst_org."""
    geo, C1, C2, up, el, ywin, skip = case
    frame, size, origins = GEOMETRIES[geo] if geo in GEOMETRIES else RECT_GEOMETRY
    rng = np.random.RandomState(1000 + seed)
    B = len(origins)
    FH, FW = frame
    sh, sw = (FH // 2, FW // 2) if up else (FH, FW)
    y = rng.standard_normal((B, C1, sh, sw)).astype(np.float32)
    sk = rng.standard_normal((B, C2, FH, FW)).astype(np.float32) if C2 else None
    g = rng.standard_normal((B, C1 + C2, size[0] + 2, size[1] + 2)).astype(np.float32)
    return dict(y=y, skip=sk, g_out=g, dst_org=np.array(origins, np.int32), frame=frame, size=size, up=up, elu=el)


def glue_groups(case):
    """The launches of a case.  The kernels take ONE source-window size per launch, and a tight window of a sample at a
    border is a row / column shorter than an interior one's: the samples are grouped by the extents of their tight windows
    (a whole-frame source does not split the batch; G5 runs one sample per launch).  Each group: (sample indices, y_org,
    y size, skip_org, skip size) with None for a whole-frame source."""
    geo, C1, C2, up, el, ywin, skip = case
    frame, size, origins = GEOMETRIES[geo]
    ylo, yhi = source_boxes(origins, size, frame, up)
    klo, khi = source_boxes(origins, size, frame, 0)
    groups = {}
    for b in range(len(origins)):
        key = (tuple(int(v) for v in yhi[b] - ylo[b]) if ywin else None,
               tuple(int(v) for v in khi[b] - klo[b]) if skip == "win" else None,
               b if geo == "G5" else None)
        groups.setdefault(key, []).append(b)
    out = []
    for (yext, kext, _), idx in groups.items():
        out.append((idx, ylo[idx].astype(np.int32) if ywin else None, yext, klo[idx].astype(np.int32) if skip == "win" else None,
                    kext))
    return out


def bwd_kernel(sw, yw, kw=None, rkw=None):
    """Which backward kernel dmh_roi_glue_bwd launches for 8-byte aligned bases: "two-wide" when the y plane's width ``sw``,
    its region's width ``yw`` and (with a skip gradient) the skip plane's and region's widths are all even."""
    odd = (sw | yw | (0 if kw is None else kw | rkw)) & 1
    return "one-element" if odd else "two-wide"
