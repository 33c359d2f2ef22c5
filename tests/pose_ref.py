"""The pose head restated in numpy, in float32 and in float64, forward and analytic backward: what K29 (csrc/pose_head.hip) is
held to.

Forward, per (sample, frame) of x [B, 6 nf, h, w]:
  v = 0.01 * x.mean(3).mean(2)                     MD2/networks/pose_decoder.py:47-49
  axisangle, translation = v[:3], v[3:]            MD2/networks/pose_decoder.py:51-52
  angle = |axisangle|, axis = axisangle / (angle + 1e-7), the nine entries of the rotation      MD2/layers.py:69-100
  T = Trans(t) Rot, or with ``invert`` Rot^T Trans(-t)                                          MD2/layers.py:31-43
Every operation is carried out in ``dtype`` in the reference's order, so the float32 form differs from the reference's fp32 run
only by the library functions (sqrt, sin, cos) and the order of the mean's additions.

Backward: d sum(g_T * T) (+ g_axisangle, g_translation) / d x, by the chain rule on R = n n^T C + ca I + sa [n]_x; at a zero
axis-angle the gradient of the norm is 0 (torch's norm backward).  tests/test_pose_ref.py checks it against autograd in float64.
"""
import numpy as np

SCALE = 0.01
SHAPES = ((1, 1, 1, 1), (2, 1, 3, 5), (2, 2, 6, 20), (3, 1, 10, 32), (2, 1, 24, 80))      # (B, nf, h, w)


def case(shape, seed):
    """Input of one case: per-channel constants plus 10 % noise, so that the rotation angles span 1e-3 .. 1.5 rad (log-uniform)
    and the translations reach O(1); invert flags mixed across the frames.  Returns (x float32, invert flags)."""
    B, nf, h, w = shape
    rng = np.random.RandomState(seed)
    angles = np.exp(rng.uniform(np.log(1e-3), np.log(1.5), size=(B, nf)))
    axis = rng.normal(size=(B, nf, 3))
    axis /= np.linalg.norm(axis, axis=2, keepdims=True)
    const = np.concatenate([axis * angles[..., None], rng.uniform(-1.0, 1.0, size=(B, nf, 3))], 2) / SCALE     # [B, nf, 6]
    x = const.reshape(B, nf * 6, 1, 1) + 0.1 * np.abs(const).reshape(B, nf * 6, 1, 1) * rng.normal(size=(B, nf * 6, h, w))
    invert = [bool((f + seed) % 2) for f in range(nf)]
    return x.astype(np.float32), invert


def zero_case():
    """(2, 2, 6, 20) with (sample 1, frame 1) all zero: means exactly zero, T the identity."""
    x, _ = case((2, 2, 6, 20), 99)
    x[1, 6:12] = 0.0
    return x, [True, False]


def cases():
    out = [case(s, i) for i, s in enumerate(SHAPES)]
    out.append(zero_case())
    x, _ = zero_case()
    out.append((x, [False, True]))      # the zero frame inverted as well
    return out


def _rot(a, dtype):
    """a [..., 3] -> dict of the intermediates of rot_from_axisangle (MD2/layers.py:64-103)."""
    one, eps = dtype(1.0), dtype(1e-7)
    angle = np.sqrt(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2]).astype(dtype)
    d = angle + eps
    n = (a / d[..., None]).astype(dtype)
    ca, sa = np.cos(angle).astype(dtype), np.sin(angle).astype(dtype)
    C = one - ca
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    xs, ys, zs = x * sa, y * sa, z * sa
    xC, yC, zC = x * C, y * C, z * C
    xyC, yzC, zxC = x * yC, y * zC, z * xC
    R = np.zeros(a.shape[:-1] + (3, 3), dtype=dtype)
    R[..., 0, 0] = x * xC + ca
    R[..., 0, 1] = xyC - zs
    R[..., 0, 2] = zxC + ys
    R[..., 1, 0] = xyC + zs
    R[..., 1, 1] = y * yC + ca
    R[..., 1, 2] = yzC - xs
    R[..., 2, 0] = zxC - ys
    R[..., 2, 1] = yzC + xs
    R[..., 2, 2] = z * zC + ca
    return dict(angle=angle, d=d, n=n, ca=ca, sa=sa, C=C, R=R)


def forward(x, invert, dtype=np.float64, scale=SCALE):
    """(axisangle [B,nf,1,3], translation [B,nf,1,3], T [B,nf,4,4]) in ``dtype``."""
    x = np.asarray(x).astype(dtype)
    B, c6, h, w = x.shape
    nf = c6 // 6
    v = (dtype(scale) * x.mean(3, dtype=dtype).mean(2, dtype=dtype)).reshape(B, nf, 6).astype(dtype)
    a, t = v[..., :3], v[..., 3:]
    r = _rot(a, dtype)
    T = np.zeros((B, nf, 4, 4), dtype=dtype)
    T[..., 3, 3] = 1
    for f in range(nf):
        R = r["R"][:, f]
        if invert[f]:
            T[:, f, :3, :3] = R.transpose(0, 2, 1)
            tn = -t[:, f]
            for i in range(3):
                T[:, f, i, 3] = (R[:, 0, i] * tn[:, 0] + R[:, 1, i] * tn[:, 1]) + R[:, 2, i] * tn[:, 2]
        else:
            T[:, f, :3, :3] = R
            T[:, f, :3, 3] = t[:, f]
    return a.reshape(B, nf, 1, 3).copy(), t.reshape(B, nf, 1, 3).copy(), T


def backward(x, invert, g_T, g_axisangle=None, g_translation=None, dtype=np.float64, scale=SCALE):
    """g_x [B, 6 nf, h, w] in ``dtype``."""
    x = np.asarray(x).astype(dtype)
    B, c6, h, w = x.shape
    nf = c6 // 6
    aa, tr, _ = forward(x, invert, dtype, scale)
    a, t = aa.reshape(B, nf, 3), tr.reshape(B, nf, 3)
    r = _rot(a, dtype)
    G = np.zeros((B, nf, 4, 4), dtype=dtype) if g_T is None else np.asarray(g_T).astype(dtype)
    gR = np.zeros((B, nf, 3, 3), dtype=dtype)
    gt = np.zeros((B, nf, 3), dtype=dtype)
    for f in range(nf):
        R = r["R"][:, f]
        if invert[f]:
            # M[i][j] = R[j][i];  M[i][3] = -sum_k R[k][i] t[k]
            for k in range(3):
                for i in range(3):
                    gR[:, f, k, i] = G[:, f, i, k] - G[:, f, i, 3] * t[:, f, k]
                gt[:, f, k] = -((G[:, f, 0, 3] * R[:, k, 0] + G[:, f, 1, 3] * R[:, k, 1]) + G[:, f, 2, 3] * R[:, k, 2])
        else:
            gR[:, f] = G[:, f, :3, :3]
            gt[:, f] = G[:, f, :3, 3]
    n, ca, sa, C, angle, d = r["n"], r["ca"], r["sa"], r["C"], r["angle"], r["d"]
    ax = np.stack([gR[..., 2, 1] - gR[..., 1, 2], gR[..., 0, 2] - gR[..., 2, 0], gR[..., 1, 0] - gR[..., 0, 1]], -1)
    sym = gR + gR.swapaxes(-1, -2)
    gn = C[..., None] * np.einsum("bfkj,bfj->bfk", sym, n) + sa[..., None] * ax
    gC = np.einsum("bfkj,bfk,bfj->bf", gR, n, n)
    g_ca = (gR[..., 0, 0] + gR[..., 1, 1] + gR[..., 2, 2]) - gC
    g_sa = (n * ax).sum(-1)
    g_angle = (g_sa * ca - g_ca * sa) - (gn * a).sum(-1) / (d * d)
    safe = np.where(angle > 0, angle, dtype(1.0))
    via_norm = np.where((angle > 0)[..., None], g_angle[..., None] * (a / safe[..., None]), dtype(0.0))
    ga = gn / d[..., None] + via_norm
    if g_axisangle is not None:
        ga = ga + np.asarray(g_axisangle).astype(dtype).reshape(B, nf, 3)
    if g_translation is not None:
        gt = gt + np.asarray(g_translation).astype(dtype).reshape(B, nf, 3)
    s6 = (np.concatenate([ga, gt], -1) * (dtype(scale) / dtype(h * w))).astype(dtype)          # [B, nf, 6]
    return np.broadcast_to(s6.reshape(B, c6, 1, 1), (B, c6, h, w)).copy()


def weights(shape, seed, dtype=np.float64):
    """Fixed output-gradient weights of a case: g_T [B,nf,4,4], g_axisangle, g_translation [B,nf,1,3]."""
    B, nf = shape[0], shape[1] // 6
    rng = np.random.RandomState(1000 + seed)
    return (rng.normal(size=(B, nf, 4, 4)).astype(np.float32).astype(dtype),
            rng.normal(size=(B, nf, 1, 3)).astype(np.float32).astype(dtype),
            rng.normal(size=(B, nf, 1, 3)).astype(np.float32).astype(dtype))


# ---- the formula weights of the golden fixture (tools/make_goldens_pose.py and the tests rebuild them; they are not stored)
GOLDEN_SEED, GOLDEN_SCALE = 20250, 0.05


def formula_state_dict(shapes):
    """{key: tensor} for ``shapes`` = {key: shape}: one seeded torch generator, keys in sorted order, N(0, 1) * GOLDEN_SCALE."""
    import torch
    g = torch.Generator().manual_seed(GOLDEN_SEED)
    return {k: torch.randn(tuple(shapes[k]), generator=g) * GOLDEN_SCALE for k in sorted(shapes)}


def golden_features():
    import torch
    g = torch.Generator().manual_seed(GOLDEN_SEED + 1)
    return torch.randn(2, 512, 3, 5, generator=g) * 20.0      # (scaled so that the rotation angles reach a few tenths of a radian)


# ---- digests of the synthetic dataset's batches (the fixture holds the parent commit's; frame_idxs [0, "s"] must keep them)
DATASET_CONFIGS = ({"hints": False, "seed": 1234}, {"hints": True, "seed": 77})


def dataset_digests(dataset_cls):
    """["<config>/<batch>/<key>=<sha256 of the tensor's bytes>", ...] for two CPU batches of each config."""
    import hashlib
    out = []
    for ci, cfg in enumerate(DATASET_CONFIGS):
        ds = dataset_cls(64, 192, [0, "s"], 4, 8, "cpu", seed=cfg["seed"], pool=4)
        ds.make_depth_hints = cfg["hints"]
        for bi in range(2):
            batch = ds.next_batch(3)
            for key in sorted(batch, key=str):
                t = batch[key].detach().cpu().contiguous()
                out.append("%d/%d/%s=%s" % (ci, bi, key, hashlib.sha256(t.numpy().tobytes()).hexdigest()))
    return out
