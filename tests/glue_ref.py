"""K7 (csrc/decoder_glue.hip) and the eval forms of K9 (csrc/encoder_glue.hip) again, in plain float64 numpy, written from the
definition: index arrays and loops, no torch, nothing shared with ops.py or the kernels.

    up_cat_pad(y, skip)   = pad1_reflect(cat(up2_nearest(elu(y)), skip))            elu(x) = x > 0 ? x : expm1(x)
    elu_pad(z, apply_elu) = pad1_reflect(elu(z))                                     (apply_elu = 0: the pad alone)
    bn_act(x, ...)        = act(x * scale[c] + shift[c] (+ res))                     act = ReLU or the identity
    stem(x, scale, shift) = feat = relu(x * scale[c] + shift[c]), MaxPool2d(3, 2, 1) of feat, and the pool's argmax

The adjoint of the reflection pad is a SCATTER-ADD over the padded plane (g[reflect(py - 1), reflect(px - 1)] += g_out[py, px]) where
the kernels gather (fold rows 0 / H + 1 onto rows 1 / H - 2): the two formulations check each other.  The max-pool adjoint is a
scatter-add through the argmax where the kernels look their <= 4 covering windows up.

tests/test_glue_ref.py holds this file to torch's float64 operators and autograd on the CPU; tests/test_gpu_glue_anchor.py holds the
kernels to it."""
import numpy as np


# ---- inputs -------------------------------------------------------------------------------------------------------------------

DYADIC_SCALES = (-1.0, -0.5, 0.25, 0.5, 1.0, 2.0)


def _signed_channels(v, rng):
    """Random signs, at least one of them negative, for per-channel factors of magnitude |v|."""
    sign = np.where(rng.uniform(size=v.shape) < 0.5, -1.0, 1.0)
    sign[rng.randint(v.size)] = -1.0
    return np.abs(v) * sign


def dyadic(shape, rng, kind="value"):
    """fp32 inputs on a coarse binary grid.  value: multiples of 2^-4 in [-4, 4]; shift, grad: multiples of 2^-4 in [-2, 2];
    scale: one of DYADIC_SCALES per entry, at least one negative.  A product value * scale is a multiple of 2^-6 below 8, a sum of
    <= 16 such terms (or of 16 gradients) needs at most 7 + 6 bits: everything is exact in fp32, so an fp32 kernel must reproduce
    the float64 result bit for bit -- except through expf.  The grid also makes positive values tie exactly in many pooling
    windows."""
    if kind == "value":
        return (rng.randint(-64, 65, size=shape) / 16.0).astype(np.float32)
    if kind in ("shift", "grad"):
        return (rng.randint(-32, 33, size=shape) / 16.0).astype(np.float32)
    assert kind == "scale", kind
    s = np.asarray(DYADIC_SCALES)[rng.randint(len(DYADIC_SCALES), size=shape)]
    if not (s < 0).any():
        s.flat[rng.randint(s.size)] = DYADIC_SCALES[rng.randint(2)]
    return s.astype(np.float32)


def generic(shape, rng, kind="value"):
    """fp32 inputs without structure.  value, grad: standard normal; scale: +-[0.3, 1.5], at least one negative; shift: [-0.5, 0.5]."""
    if kind in ("value", "grad"):
        return rng.standard_normal(shape).astype(np.float32)
    if kind == "shift":
        return rng.uniform(-0.5, 0.5, size=shape).astype(np.float32)
    assert kind == "scale", kind
    return _signed_channels(rng.uniform(0.3, 1.5, size=shape), rng).astype(np.float32)


# ---- the pieces ---------------------------------------------------------------------------------------------------------------

def reflect(i, n):
    """ReflectionPad2d(1): -1 -> 1, n -> n - 2 (the border itself is not repeated)."""
    if i < 0:
        return -i
    if i >= n:
        return 2 * (n - 1) - i
    return i


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def elu(x):
    x = _f64(x)
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def elu_grad(x):
    x = _f64(x)
    return np.where(x > 0, 1.0, np.exp(np.minimum(x, 0)))


def pad1_reflect(t):
    H, W = t.shape[-2:]
    ry = np.array([reflect(p - 1, H) for p in range(H + 2)])
    rx = np.array([reflect(p - 1, W) for p in range(W + 2)])
    return t[..., ry[:, None], rx[None, :]]


def pad1_reflect_adjoint(g):
    """Scatter-add over the padded plane."""
    H, W = g.shape[-2] - 2, g.shape[-1] - 2
    out = np.zeros(g.shape[:-2] + (H, W))
    for py in range(H + 2):
        for px in range(W + 2):
            out[..., reflect(py - 1, H), reflect(px - 1, W)] += g[..., py, px]
    return out


def up2_nearest(e):
    h, w = e.shape[-2:]
    return e[..., (np.arange(2 * h) // 2)[:, None], (np.arange(2 * w) // 2)[None, :]]


def up2_nearest_adjoint(g):
    H, W = g.shape[-2:]
    out = np.zeros(g.shape[:-2] + (H // 2, W // 2))
    for Y in range(H):
        for X in range(W):
            out[..., Y // 2, X // 2] += g[..., Y, X]
    return out


def _per_channel(v, ndim=4):
    return _f64(v).reshape((1, -1) + (1,) * (ndim - 2))


# ---- K7 -----------------------------------------------------------------------------------------------------------------------

def up_cat_pad(y, skip=None):
    t = up2_nearest(elu(y))
    if skip is not None:
        t = np.concatenate([t, _f64(skip)], axis=1)
    return pad1_reflect(t)


def up_cat_pad_bwd(y, g_out, want_skip=True):
    """(g_y, g_skip, S_y, S_skip): the gradients and the same adjoint applied to |g_out| (times elu'(y) for g_y), the magnitude
    tests.util.assert_round_bound takes.  g_skip / S_skip are None without skip planes or with want_skip false."""
    y, g_out = _f64(y), _f64(g_out)
    C1 = y.shape[1]
    res = []
    for g in (g_out, np.abs(g_out)):
        t = pad1_reflect_adjoint(g)
        res.append((up2_nearest_adjoint(t[:, :C1]) * elu_grad(y), t[:, C1:] if want_skip and t.shape[1] > C1 else None))
    (g_y, g_skip), (S_y, S_skip) = res
    return g_y, g_skip, S_y, S_skip


def elu_pad(z, apply_elu=True):
    return pad1_reflect(elu(z) if apply_elu else _f64(z))


def elu_pad_bwd(z, g_out, apply_elu=True):
    """(g_z, S)."""
    d = elu_grad(z) if apply_elu else 1.0
    return pad1_reflect_adjoint(_f64(g_out)) * d, pad1_reflect_adjoint(np.abs(_f64(g_out))) * d


# ---- K9, eval forms -----------------------------------------------------------------------------------------------------------

def affine(x, scale, shift, res=None):
    """x * scale[c] + shift[c] (+ res) in float64: the pre-activation."""
    pre = _f64(x) * _per_channel(scale, np.ndim(x)) + _per_channel(shift, np.ndim(x))
    return pre if res is None else pre + _f64(res)


def affine_S(x, scale, shift, res=None):
    """|x * scale[c]| + |shift[c]| (+ |res|): what the roundings of the forward act on."""
    S = np.abs(_f64(x) * _per_channel(scale, np.ndim(x))) + np.abs(_per_channel(shift, np.ndim(x)))
    return S if res is None else S + np.abs(_f64(res))


def bn_act(x, scale, shift, res=None, relu=True):
    pre = affine(x, scale, shift, res)
    return np.maximum(pre, 0.0) if relu else pre


def bn_act_bwd(out, g, scale, relu=True):
    """(g_x, g_res): g_res = relu ? g [out > 0] : g, g_x = g_res * scale[c]."""
    g = _f64(g)
    g_res = np.where(_f64(out) > 0, g, 0.0) if relu else g
    return g_res * _per_channel(scale, g.ndim), g_res


def stem(x, scale, shift, better=np.greater):
    """(feat, pooled, argmax) of MaxPool2d(3, 2, 1) over feat = relu(x * scale[c] + shift[c]); H and W even.  argmax is ky * 3 + kx
    of the UNCLIPPED window rows 2i - 1 .. 2i + 1, columns 2j - 1 .. 2j + 1.  The scan runs ky, then kx, ascending over the
    positions inside the image and replaces only on strictly greater: the first maximum wins, in a window of zeros too.
    ``better`` exists for tests/test_glue_ref.py, which seeds the other tie rule."""
    feat = np.maximum(affine(x, scale, shift), 0.0)
    B, C, H, W = feat.shape
    PH, PW = H // 2, W // 2
    pooled = np.empty((B, C, PH, PW))
    argmax = np.empty((B, C, PH, PW), np.uint8)
    for i in range(PH):
        for j in range(PW):
            m = np.full((B, C), -np.inf)
            a = np.full((B, C), 255, np.uint8)
            for ky in range(3):
                yy = 2 * i - 1 + ky
                if yy < 0 or yy >= H:
                    continue
                for kx in range(3):
                    xx = 2 * j - 1 + kx
                    if xx < 0 or xx >= W:
                        continue
                    v = feat[:, :, yy, xx]
                    take = better(v, m)
                    m = np.where(take, v, m)
                    a = np.where(take, np.uint8(ky * 3 + kx), a)
            pooled[:, :, i, j], argmax[:, :, i, j] = m, a
    return feat, pooled, argmax


def stem_bwd(feat, argmax, g_feat, g_pool, scale, decode=lambda a: (a // 3, a % 3)):
    """(g_x, S): scatter-add of g_pool through the argmax, plus g_feat, masked by feat > 0, times scale[c]; either gradient may be
    None.  S is the same with |g_pool|, |g_feat|, |scale|.  ``decode`` exists for tests/test_glue_ref.py (a transposed decoding)."""
    feat = _f64(feat)
    B, C, H, W = feat.shape
    acc, S = np.zeros(feat.shape), np.zeros(feat.shape)
    if g_pool is not None:
        g_pool = _f64(g_pool)
        for b in range(B):
            for c in range(C):
                for i in range(H // 2):
                    for j in range(W // 2):
                        ky, kx = decode(int(argmax[b, c, i, j]))
                        yy, xx = 2 * i - 1 + ky, 2 * j - 1 + kx
                        if 0 <= yy < H and 0 <= xx < W:         # (a correct argmax is always inside)
                            acc[b, c, yy, xx] += g_pool[b, c, i, j]
                            S[b, c, yy, xx] += abs(g_pool[b, c, i, j])
    if g_feat is not None:
        acc += _f64(g_feat)
        S += np.abs(_f64(g_feat))
    live = feat > 0
    s = _per_channel(scale)
    return np.where(live, acc * s, 0.0), np.where(live, S * np.abs(s), 0.0)
