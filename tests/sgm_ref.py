"""K35's yardstick: the semi-global matcher of DESIGN.md section 3 (K35) restated pixel by pixel from its text, and the seeded
inputs that tools/make_goldens_sgm.py and the tests share.  Integers only (Python ints and int64 arrays over the disparity axis):
nothing here is shared with ``ops.sgm_disparity_host`` (whole-image numpy) or with the kernel, which are both held to it bit for bit.

``disparity(base, lookup, params, reverse)``: base, lookup uint8 [3, H, W]; returns int16 [H, W], disparity x 16, -16 = no match.
"""
import functools
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(REPO, "tests", "golden", "sgm_disparity.npz")
SHAPES = ((9, 70, 16, 1), (16, 100, 32, 3), (24, 136, 64, 2), (8, 200, 160, 1))       # (H, W, numDisparities, blockSize)
BIG = 1 << 30


WINDOWS = (100, 0, 12)          # speckleWindowSize: the reference's, none, and one that splits the small maps' components


def params(D, block, window=100, **kw):
    """One parameter set with the reference's constants (``precompute_depth_hints.stereo_matcher_params``)."""
    p = dict(preFilterCap=63, P1=36, P2=288, minDisparity=0, numDisparities=D, uniquenessRatio=10,
             speckleWindowSize=int(window), speckleRange=16, blockSize=block)
    p.update(kw)
    return p


def tdiv(a, b):
    """C's integer division: the quotient truncated toward zero (b > 0)."""
    return -((-a) // b) if a < 0 else a // b


def prefilter(I, cap):
    C, H, W = I.shape
    g = [[[cap] * W for _ in range(H)] for _ in range(C)]
    for c in range(C):
        for y in range(H):
            up, dn = I[c][max(y - 1, 0)], I[c][min(y + 1, H - 1)]
            mid = I[c][y]
            for x in range(1, W - 1):
                s = (int(up[x + 1]) - int(up[x - 1])) + 2 * (int(mid[x + 1]) - int(mid[x - 1])) + (int(dn[x + 1]) - int(dn[x - 1]))
                g[c][y][x] = min(max(s, -cap), cap) + cap
    return np.array(g, dtype=np.int64).reshape(C, H, W)


def lo_hi(A):
    """lo, hi of every row of A [..., W]: the extremes of A(x) and its two half-way points, columns replicated at the ends."""
    W = A.shape[-1]
    lo, hi = np.empty_like(A), np.empty_like(A)
    for x in range(W):
        a, l, r = A[..., x], A[..., max(x - 1, 0)], A[..., min(x + 1, W - 1)]
        hl, hr = (a + l) // 2, (a + r) // 2            # non-negative: the quotient needs no sign rule
        lo[..., x] = np.minimum(a, np.minimum(hl, hr))
        hi[..., x] = np.maximum(a, np.maximum(hl, hr))
    return lo, hi


def pixel_costs(base, lookup, D, cap):
    """pc [H, W, D] (columns x < D stay 0 and are never read)."""
    _, H, W = base.shape
    rows = []
    for img in (base.astype(np.int64), lookup.astype(np.int64)):
        g = prefilter(img, cap)
        rows.append((g,) + lo_hi(g) + (img,) + lo_hi(img))
    (gb, gb_lo, gb_hi, ib, ib_lo, ib_hi), (gl, gl_lo, gl_hi, il, il_lo, il_hi) = rows
    pc = np.zeros((H, W, D), dtype=np.int64)
    zero = np.zeros(D, dtype=np.int64)

    def bt(u, lo_u, hi_u, v, lo_v, hi_v):
        return np.minimum(np.maximum(zero, np.maximum(u - hi_v, lo_v - u)), np.maximum(zero, np.maximum(v - hi_u, lo_u - v)))
    for y in range(H):
        for x in range(D, W):
            cols = x - np.arange(D)
            acc = zero.copy()
            for c in range(3):
                acc += bt(gb[c, y, x], gb_lo[c, y, x], gb_hi[c, y, x], gl[c, y, cols], gl_lo[c, y, cols], gl_hi[c, y, cols])
                acc += bt(ib[c, y, x], ib_lo[c, y, x], ib_hi[c, y, x], il[c, y, cols], il_lo[c, y, cols], il_hi[c, y, cols]) >> 2
            pc[y, x] = acc
    return pc


def block_costs(pc, D, r):
    """C [H, Wv, D]: matched column x is index x - D."""
    H, W, _ = pc.shape
    C = np.zeros((H, W - D, D), dtype=np.int64)
    for y in range(H):
        for x in range(D, W):
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    C[y, x - D] += pc[min(max(y + dy, 0), H - 1), min(max(x + dx, D), W - 1)]
    return C


PATHS = ((-1, 0), (1, 0), (-1, -1), (0, -1), (1, -1))       # the predecessor is p + (dx, dy)


def aggregate(C, P1, P2):
    H, Wv, D = C.shape
    S = np.zeros_like(C)
    for dx, dy in PATHS:
        L = np.zeros_like(C)
        xs = range(Wv - 1, -1, -1) if (dx, dy) == (1, 0) else range(Wv)
        for y in range(H):
            for x in xs:
                qx, qy = x + dx, y + dy
                if qx < 0 or qx >= Wv or qy < 0:
                    L[y, x] = C[y, x]
                    continue
                q = L[qy, qx]
                m = int(q.min())
                down = np.concatenate(([BIG], q[:-1])) + P1         # L(q, d - 1); d - 1 < 0 takes no part
                up = np.concatenate((q[1:], [BIG])) + P1            # L(q, d + 1)
                L[y, x] = C[y, x] + np.minimum(np.minimum(q, down), np.minimum(up, m + P2)) - m
        S += L
    return S


def select_row(S, D, W, uniq, d12, counts=None):
    """Steps 5 and 6 for one row: S [Wv, D] -> list of W values.  ``counts``: a dict whose "not_unique" and "lr_removed" grow by the
    pixels the uniqueness test dropped and by those the left-right check removed after it had kept them."""
    out = [-16] * W
    best = {}                       # lookup column -> (minS, x, d*) of the proposer that holds it
    for x in range(D, W):
        s = [int(v) for v in S[x - D]]
        min_s = min(s)
        d_star = s.index(min_s)
        if any(s[d] * (100 - uniq) < 100 * min_s for d in range(D) if abs(d - d_star) > 1):
            if counts is not None:
                counts["not_unique"] = counts.get("not_unique", 0) + 1
            continue
        x2 = x - d_star
        if x2 not in best or (min_s, x) < best[x2][:2]:
            best[x2] = (min_s, x, d_star)
        if d_star == 0 or d_star == D - 1:
            out[x] = 16 * d_star
        else:
            den = max(s[d_star - 1] + s[d_star + 1] - 2 * min_s, 1)
            out[x] = 16 * d_star + tdiv((s[d_star - 1] - s[d_star + 1]) * 16 + den, 2 * den)
    for x in range(D, W):
        v = out[x]
        if v < 0:
            continue
        bad = 0
        for dd in (v >> 4, (v + 15) >> 4):
            x2 = x - dd
            if 0 <= x2 < W and x2 in best and abs(best[x2][2] - dd) > d12:
                bad += 1
        if bad == 2:
            out[x] = -16
            if counts is not None:
                counts["lr_removed"] = counts.get("lr_removed", 0) + 1
    return out


def speckle(disp, window, rng16):
    H, W = disp.shape
    out = disp.copy()
    seen = np.zeros((H, W), dtype=bool)
    for y0 in range(H):
        for x0 in range(W):
            if seen[y0, x0] or disp[y0, x0] < 0:
                continue
            seen[y0, x0] = True
            comp, stack = [], [(y0, x0)]
            while stack:
                y, x = stack.pop()
                comp.append((y, x))
                for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= ny < H and 0 <= nx < W and not seen[ny, nx] and disp[ny, nx] >= 0 \
                            and abs(int(disp[ny, nx]) - int(disp[y, x])) <= rng16:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
            if len(comp) <= window:
                for y, x in comp:
                    out[y, x] = -16
    return out


def disparity(base, lookup, p, reverse=False, stages=None):
    """The whole matcher for one pair.  ``stages``: a dict that receives "raw", the map after step 6 (before the speckle filter), and
    ``select_row``'s counts."""
    base, lookup = np.asarray(base), np.asarray(lookup)
    if reverse:
        base, lookup = base[:, :, ::-1], lookup[:, :, ::-1]
    _, H, W = base.shape
    D, r = int(p["numDisparities"]), int(p["blockSize"]) // 2
    out = np.full((H, W), -16, dtype=np.int64)
    if W > D:
        pc = pixel_costs(base, lookup, D, int(p["preFilterCap"]))
        S = aggregate(block_costs(pc, D, r), int(p["P1"]), int(p["P2"]))
        for y in range(H):
            out[y] = select_row(S[y], D, W, int(p["uniquenessRatio"]), int(p.get("disp12MaxDiff", 0)), stages)
    if stages is not None:
        stages["raw"] = (out[:, ::-1] if reverse else out).astype(np.int16)
    if int(p["speckleWindowSize"]) > 0:
        out = speckle(out, int(p["speckleWindowSize"]), 16 * int(p["speckleRange"]))
    if reverse:
        out = out[:, ::-1]
    return np.ascontiguousarray(out).astype(np.int16)


# ------------------------------------------------------------------------------------------------ the inputs
def _texture(rng, H, W):
    """Random bytes, lightly smoothed (1 2 1 / 4 along both axes, in integers), 3 channels."""
    t = rng.randint(0, 256, size=(3, H + 2, W + 2)).astype(np.int64)
    t = (t[:, :, :-2] + 2 * t[:, :, 1:-1] + t[:, :, 2:] + 2) // 4
    t = (t[:, :-2] + 2 * t[:, 1:-1] + t[:, 2:] + 2) // 4
    return t.astype(np.uint8)


def make_pair(H, W, D, seed=0):
    """(base, lookup uint8 [3, H, W], truth int [H, W]).  The lookup view is the texture; the base view shows at x what the
    lookup has at x - truth: a background, a bottom band and a box in the middle at three disparities below D; where x - truth
    leaves the image (the strip the other camera does not see) the base is filled from spare texture."""
    rng = np.random.RandomState(1000 + seed)
    lookup, spare = _texture(rng, H, W), _texture(rng, H, W)
    truth = np.full((H, W), max(1, D // 5), dtype=np.int64)
    truth[(2 * H) // 3:] = (9 * D) // 20
    truth[H // 4:(2 * H) // 3, W // 2:(5 * W) // 6] = (7 * D) // 10
    src = np.arange(W)[None, :] - truth
    base = np.take_along_axis(lookup, np.broadcast_to(np.clip(src, 0, W - 1), (3, H, W)), axis=2)
    base = np.where(src[None] < 0, spare, base)
    return np.ascontiguousarray(base), lookup, truth


def golden_cases():
    """(key, H, W, params, reverse, seed) of every map in tests/golden/sgm_disparity.npz."""
    out = []
    for i, (H, W, D, b) in enumerate(SHAPES):
        for reverse in (False, True):
            for window in WINDOWS:
                out.append(("h%d_w%d_d%d_b%d_r%d_s%d" % (H, W, D, b, reverse, window), H, W, params(D, b, window), reverse, i))
    return out


@functools.lru_cache(maxsize=None)
def reference(H, W, D, block, reverse=False, window=100, seed=0):
    """The loop reference's map for ``make_pair(H, W, D, seed)``, computed once per process.  Shared; do not modify."""
    base, lookup, _ = make_pair(H, W, D, seed)
    out = disparity(base, lookup, params(D, block, window), reverse)
    out.setflags(write=False)
    return out


def shares(disp, truth, D):
    """(valid share of the matched columns, share of the valid pixels within 16 units of 16 truth)."""
    m = disp[:, D:]
    valid = m >= 0
    near = np.abs(m.astype(np.int64) - 16 * truth[:, D:]) <= 16
    return float(valid.mean()), float((near & valid).sum()) / max(int(valid.sum()), 1)


def write_tree(root, size=(16, 208), seed=70, sides="lrl"):
    """A KITTI-shaped tree of PNG files at ``size`` whose pairs are ``make_pair(H, W, 64, seed + i)`` (true disparities below 64, so
    that every matcher of the reference sees them): a left base image for an "l" line; for an "r" line both views are stored
    mirrored, so that the tool's reversal matches the same pair.  Returns the split lines."""
    from PIL import Image
    lines = []
    for i, side in enumerate(sides):
        base, lookup, _ = make_pair(size[0], size[1], 64, seed + i)
        left, right = (base, lookup) if side == "l" else (lookup[:, :, ::-1], base[:, :, ::-1])
        seq = "2011_09_26/2011_09_26_drive_%04d_sync" % (i + 1)
        for cam, img in (("image_02", left), ("image_03", right)):
            path = os.path.join(root, seq, cam, "data", "%010d.png" % i)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0))).save(path)
        lines.append("%s %d %s" % (seq, i, side))
    return lines
