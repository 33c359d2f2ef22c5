"""ManyDepth's matching cost volume restated in numpy, at float32 and at float64: what K30 (csrc/cost_volume.hip) is held to.

Written from the arithmetic of manydepth2/networks/resnet_encoder.py:157-236 (match_features), :258-265 (compute_confidence_mask)
and :294-296 (the argmin of forward), and manydepth2/layers.py:164-195 (BackprojectDepth / Project3D), operation by operation; every
matrix product is written out with its terms added in index order.  ``forward(case, np.float64)`` also returns, per pixel column
(b, h, w), the smallest distance -- in pixels of the matching grid -- of any of its (bin, lookup) sample positions to the nearest
of the four thresholds of the edge mask: a flag can only differ between two precisions where that distance is tiny, and one
flipped flag changes the column's count, maximum and confidence.  The GPU tests exclude the columns whose distance is below
``EXCLUDE`` and assert that they are few.

The cases (``case(name)``) are the ones tests/golden/cost_volume.npz records the reference for (tools/make_goldens_manydepth.py).
"""
import hashlib

import numpy as np

C = 64
EXCLUDE = 1e-3              # pixels
NORMALISED_K = ((0.58, 0.0, 0.5), (0.0, 1.92, 0.5), (0.0, 0.0, 1.0))
SHAPES = {"A": dict(H=12, W=24, D=8, B=2, L=2), "B": dict(H=16, W=40, D=96, B=2, L=2), "odd": dict(H=9, W=37, D=19, B=1, L=1)}


def intrinsics(W, H):
    K = np.eye(4)
    K[:3, :3] = np.array(NORMALISED_K)
    K[0, :] *= W
    K[1, :] *= H
    return K.astype(np.float32), np.linalg.pinv(K).astype(np.float32)


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def generic_poses(B, L):
    """Poses with no axis-aligned component: a pure x-translation puts whole rows of samples exactly on a threshold."""
    T = np.zeros((B, L, 4, 4))
    for b in range(B):
        for l in range(L):
            T[b, l, :3, :3] = _rot("z", 0.007 * (b + l + 1)) @ _rot("y", -0.023 * (l + 1)) @ _rot("x", 0.011 * (b + 1))
            T[b, l, :3, 3] = (0.31 if l == 0 else -0.31, 0.043 * (b + 1), -0.37 + 0.5 * l)
            T[b, l, 3, 3] = 1.0
    return T.astype(np.float32)


def case(name):
    """Inputs of a named case: features relu(randn) from seed 0, K the normalised intrinsics times (W, H), bins
    linspace(0.5, 10, D), generic poses with the last lookup of the last sample all zero.  Variants of case A: "A_bp1" (poses
    [1,L,4,4] at B = 2: the second sample has no lookups) and "A_zero" (all poses zero)."""
    base = name.split("_")[0]
    s = SHAPES[base]
    B, L, H, W, D = s["B"], s["L"], s["H"], s["W"], s["D"]
    rng = np.random.RandomState(0)
    cur = np.maximum(rng.standard_normal((B, C, H, W)), 0).astype(np.float32)
    look = np.maximum(rng.standard_normal((B, L, C, H, W)), 0).astype(np.float32)
    K, invK = intrinsics(W, H)
    poses = generic_poses(B, L)
    if B > 1:
        poses[B - 1, L - 1] = 0
    if name.endswith("_bp1"):
        poses = poses[:1].copy()
    elif name.endswith("_zero"):
        poses = np.zeros_like(poses)
    return dict(current=cur, lookup=look, poses=poses, K=np.repeat(K[None], B, 0), invK=np.repeat(invK[None], B, 0),
                bins=np.linspace(0.5, 10, D).astype(np.float32))


def digest(c):
    h = hashlib.sha256()
    for k in sorted(c):
        h.update(k.encode())
        h.update(np.ascontiguousarray(c[k]).tobytes())
    return h.hexdigest()


def _sample(feat, ix, iy):
    """grid_sample(bilinear, zeros, align_corners=True) of feat [C,H,W] at pixel positions ix, iy [...]."""
    Cc, H, W = feat.shape
    x0, y0 = np.floor(ix), np.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    wx0, wy0 = (x0 + 1) - ix, (y0 + 1) - iy
    out = np.zeros((Cc,) + ix.shape, dtype=feat.dtype)
    for dy, dx, wgt in ((0, 0, wx0 * wy0), (0, 1, wx1 * wy0), (1, 0, wx0 * wy1), (1, 1, wx1 * wy1)):
        xs, ys = x0 + dx, y0 + dy
        ok = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        xi = np.where(ok, xs, 0).astype(np.int64)
        yi = np.where(ok, ys, 0).astype(np.int64)
        out = out + feat[:, yi, xi] * np.where(ok, wgt, 0).astype(feat.dtype)[None]
    return out


def forward(c, dtype=np.float32, set_missing_to_max=True):
    """dict(cost, missing, confidence, argmin, margin [B,H,W], gap_ok [B,H,W]) of a case in ``dtype``.  ``margin``: see the module
    docstring (inf where no sample of the column counts).  ``gap_ok``: the two smallest costs of the column (zeros read as 100)
    differ by less than 4 * 2^-24 * cost, so that either index is a legitimate argmin in float32.  An exact tie is not such a
    column: it comes from one value written twice (zeros read as 100, missing entries set to the column's maximum), is a tie in
    every precision, and the first index has to win."""
    cur, look, poses, K, invK, bins = (np.asarray(c[k]).astype(dtype) for k in ("current", "lookup", "poses", "K", "invK", "bins"))
    B, Cc, H, W = cur.shape
    L, D, Bp = look.shape[1], bins.shape[0], poses.shape[0]
    one, half, two, eps = dtype(1), dtype(0.5), dtype(2), dtype(1e-7)
    wm1, hm1 = dtype(W - 1), dtype(H - 1)
    ys, xs = np.meshgrid(np.arange(H).astype(dtype), np.arange(W).astype(dtype), indexing="ij")
    cur_mask = np.zeros((H, W), dtype=dtype)
    cur_mask[2:-2, 2:-2] = 1
    cost_all, miss_all = np.zeros((B, D, H, W), dtype), np.zeros((B, D, H, W), dtype)
    margin = np.full((B, H, W), np.inf)
    for b in range(B):
        iK = invK[b]
        cam = [iK[r, 0] * xs + iK[r, 1] * ys + iK[r, 2] for r in range(3)]                  # invK[:3,:3] @ (x, y, 1)
        pts = [bins[:, None, None] * cam[r][None] for r in range(3)]                        # [D,H,W] each
        total, counts = np.zeros((D, H, W), dtype), np.zeros((D, H, W), dtype)
        for l in range(L):
            if b >= Bp:
                continue
            T = poses[b, l]
            s = dtype(0)
            for v in T.reshape(-1):
                s = s + v
            if s == 0:
                continue
            P = np.zeros((3, 4), dtype)
            for r in range(3):
                for cc in range(4):
                    a = K[b, r, 0] * T[0, cc]
                    for k in (1, 2, 3):
                        a = a + K[b, r, k] * T[k, cc]
                    P[r, cc] = a
            proj = [((P[r, 0] * pts[0] + P[r, 1] * pts[1]) + P[r, 2] * pts[2]) + P[r, 3] for r in range(3)]
            den = proj[2] + eps
            with np.errstate(divide="ignore", invalid="ignore"):
                gx = ((proj[0] / den) / wm1 - half) * two
                gy = ((proj[1] / den) / hm1 - half) * two
            xv, yv = (gx / two + half) * wm1, (gy / two + half) * hm1
            edge = ((xv >= 2) & (xv <= W - 2) & (yv >= 2) & (yv <= H - 2)).astype(dtype) * cur_mask[None]
            dist = np.minimum(np.minimum(np.abs(xv - 2), np.abs(xv - (W - 2))), np.minimum(np.abs(yv - 2), np.abs(yv - (H - 2))))
            dist = np.where(cur_mask[None] > 0, np.nan_to_num(dist.astype(np.float64), nan=0.0), np.inf)
            margin[b] = np.minimum(margin[b], dist.min(0))
            ix, iy = ((gx + one) / two) * wm1, ((gy + one) / two) * hm1
            ix, iy = np.nan_to_num(ix, nan=-5.0, posinf=-5.0, neginf=-5.0), np.nan_to_num(iy, nan=-5.0, posinf=-5.0, neginf=-5.0)
            warped = _sample(look[b, l], ix, iy)                                            # [C,D,H,W]
            diffs = (np.abs(warped - cur[b][:, None]).sum(0, dtype=dtype) / dtype(Cc)) * edge
            total = total + diffs
            counts = counts + (diffs > 0).astype(dtype)
        cost = total / (counts + eps)
        miss = (cost == 0).astype(dtype)
        if set_missing_to_max:
            cost = cost * (one - miss) + cost.max(0)[None] * miss
        cost_all[b], miss_all[b] = cost, miss
    confidence = (((cost_all * (1 - miss_all)) > 0).sum(1) == D).astype(dtype)
    viz = np.where(cost_all == 0, dtype(100), cost_all)
    argmin = viz.argmin(1)
    two_smallest = np.sort(viz, 1)[:, :2] if D > 1 else np.concatenate([viz, viz + 1], 1)
    gap = two_smallest[:, 1] - two_smallest[:, 0]
    gap_ok = (gap > 0) & (gap < 4 * 2.0 ** -24 * two_smallest[:, 0])
    return dict(cost=cost_all, missing=miss_all, confidence=confidence, argmin=argmin, margin=margin, gap_ok=gap_ok)


# ------------------------------------------------------------------------------------------------- the encoder fixture
def formula_state_dict(shapes, seed=11):
    """Weights of an encoder from a formula (one seeded generator, keys in sorted order), so that the fixture need not store
    them (load with strict=False: the ``backprojector`` pixel grid is left as constructed): convolutions N(0, 1) * 0.05, BatchNorm weight 1 + 0.1 n, bias and running mean 0.1 n, running variance 0.5 + |n|."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for k in sorted(shapes):
        if k.startswith("backprojector."):      # the pixel grid: constants, not weights
            continue
        shape = tuple(shapes[k])
        if k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(3, dtype=torch.long)
            continue
        n = torch.randn(shape, generator=gen)
        if k.endswith("running_var"):
            out[k] = 0.5 + n.abs()
        elif k.endswith("running_mean") or (len(shape) == 1 and k.endswith("bias")):
            out[k] = 0.1 * n
        elif len(shape) == 1:
            out[k] = 1 + 0.1 * n
        else:
            out[k] = 0.05 * n
    return out


def encoder_inputs(H=48, W=96):
    """A 2-sample H x W (48 x 96) frame pair with one lookup frame (the current frame shifted and dimmed: matching features exist), generic
    relative poses with a small translation, and the intrinsics of the H/4 x W/4 matching grid."""
    rng = np.random.RandomState(5)
    yy, xx = np.meshgrid(np.arange(H) / float(H), np.arange(W) / float(W), indexing="ij")
    base = np.stack([0.5 + 0.3 * np.sin(7 * xx + 3 * yy + ph) + 0.15 * np.cos(11 * yy * (1 + xx) + ph) for ph in (0.0, 0.7, 1.9)], 0)
    cur = np.stack([base, base[::-1]], 0) + 0.05 * rng.standard_normal((2, 3, H, W))
    look = np.roll(cur, 3, axis=3) * 0.95 + 0.03 * rng.standard_normal((2, 3, H, W))
    K, invK = intrinsics(W // 4, H // 4)
    poses = generic_poses(2, 1)
    poses[:, :, :3, 3] *= 0.03          # bins 0.1 .. 20: a translation small enough that part of the grid sees all 96 bins
    return dict(current=np.clip(cur, 0, 1).astype(np.float32), lookup=np.clip(look, 0, 1).astype(np.float32)[:, None],
                poses=poses, K=np.repeat(K[None], 2, 0), invK=np.repeat(invK[None], 2, 0))
