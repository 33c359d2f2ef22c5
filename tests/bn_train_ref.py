"""K9's train forms (csrc/encoder_glue.hip: dmh_bn_train_stats_tracked, dmh_bn_train_bwd) again, in plain float64 numpy, written from
the definition: two-pass statistics, the closed form of the backward, python loops over the slabs.  No torch, nothing shared with
ops.py or the kernels.

    stats     mean = E[x], var = E[(x - mean)^2] over (B, H, W) per channel (two passes), invstd = 1 / sqrt(var + eps),
              scale = weight * invstd, shift = bias - mean * scale, unbiased var = sum (x - mean)^2 / max(n - 1, 1)
    running   new = (1 - momentum) * old + momentum * batch value                       (nn.BatchNorm2d; the variance unbiased)
    backward  g' = g * [out > 0] (or g), xc = x - mean, n = B * HW:
              db = sum g',  dw = invstd * sum g' xc,  dx = w invstd (g' - db / n - xc invstd^2 (sum g' xc) / n),  g_pre = g'

The three reductions of the kernels (statistics, backward sums, dmh_channel_sum) deal the SLAB-element slabs of one plane to
S = min(S_CAP, ceil(HW / SLAB)) blocks: block s owns slabs s, s + S, s + 2 S, ...  slab_sets() restates that deal the way the scalar
loops walk it ("for (r0 = s * SLAB; r0 < HW; r0 += S * SLAB)"), slabs_of() is the closed form the vector loops use; the two must
select the same sets (tests/test_bn_train_ref.py).

Tensors are [B, C, HW] (or [B, C, H, W]: flattened here).  tests/test_bn_train_ref.py holds this file to torch's float64 operators on
the CPU; tests/test_gpu_bn_train_anchor.py holds the kernels to it."""
import numpy as np

NT = 256                # threads of a block
SLAB = 4 * NT           # elements of a plane one block takes per step
S_CAP = 64              # most blocks per plane


# ---- the deal of slabs to blocks ----------------------------------------------------------------------------------------------

def launch_form(HW):
    return "vector" if HW % 4 == 0 else "scalar"


def slabs_of(HW, s, S):
    """Closed form: how many slabs of an HW-element plane fall to block s of S."""
    nslab = (HW + SLAB - 1) // SLAB
    return (nslab - 1 - s) // S + 1 if s < nslab else 0


def slab_sets(HW):
    """(S, sets): sets[s] is the list of element ranges (lo, hi) of block s, in the order the block visits them."""
    S = min(S_CAP, (HW + SLAB - 1) // SLAB)
    sets = []
    for s in range(S):
        ranges, r0 = [], s * SLAB
        while r0 < HW:
            ranges.append((r0, min(r0 + SLAB, HW)))
            r0 += S * SLAB
        sets.append(ranges)
    return S, sets


def block_pairs(B, HW):
    """(S, pairs): pairs[s] is the list of (image, lo, hi) triples of block s in the order of the flattened (image, slab) loop,
    i = b * nk + j."""
    S, sets = slab_sets(HW)
    return S, [[(b, lo, hi) for b in range(B) for (lo, hi) in ranges] for ranges in sets]


# ---- inputs -------------------------------------------------------------------------------------------------------------------

def _flat(a):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _ch(v):
    return np.asarray(v, dtype=np.float64).reshape(1, -1, 1)


def dyadic(shape, rng, kind="x", mean=None):
    """fp32 inputs on a coarse binary grid, such that every product and every partial sum of the backward's two reductions is exact
    in fp32 whatever the order: grad in {-1, -1/2, 0, 1/2, 1}; mean (per channel) a multiple of 1/4 in [-2, 2]; x = mean[c] + a
    multiple of 1/4 in [-2, 2]; invstd and weight powers of two (weight of either sign); out: exact zeros on about half the elements,
    multiples of 1/4 in (0, 2] elsewhere; bias a multiple of 1/4.  A term g' (x - mean) is a multiple of 1/8 of magnitude <= 2, so a
    sum of n terms needs log2(16 n) bits: exact below n = 2^20 elements per channel."""
    if kind == "grad":
        return (rng.randint(-2, 3, size=shape) / 2.0).astype(np.float32)
    if kind in ("mean", "bias"):
        return (rng.randint(-8, 9, size=shape) / 4.0).astype(np.float32)
    if kind == "x":
        x = rng.randint(-8, 9, size=shape) / 4.0
        return (x + (0.0 if mean is None else np.asarray(mean, np.float64).reshape((1, -1) + (1,) * (len(shape) - 2)))).astype(np.float32)
    if kind == "invstd":
        return (2.0 ** rng.randint(-2, 3, size=shape)).astype(np.float32)
    if kind == "weight":
        return (2.0 ** rng.randint(-1, 2, size=shape) * np.where(rng.uniform(size=shape) < 0.5, -1.0, 1.0)).astype(np.float32)
    assert kind == "out", kind
    return (rng.randint(1, 9, size=shape) / 4.0 * (rng.uniform(size=shape) < 0.5)).astype(np.float32)


def generic(shape, rng, kind="x", pivot=None):
    """fp32 inputs without structure.  x [B, C, ...]: per-channel sigma log-uniform in [0.1, 10], per-channel mean uniform in
    [-4, 4] sigma, normal around it; ``pivot`` = p sets x[0, c, 0...] = mean + p sigma (the element the statistics kernel shifts its
    sums by).  grad, out: standard normal (out > 0 on about half the elements); weight: +-[0.5, 1.5]; bias: [-0.5, 0.5]."""
    if kind in ("grad", "out"):
        return rng.standard_normal(shape).astype(np.float32)
    if kind == "bias":
        return rng.uniform(-0.5, 0.5, size=shape).astype(np.float32)
    if kind == "weight":
        return (rng.uniform(0.5, 1.5, size=shape) * np.where(rng.uniform(size=shape) < 0.5, -1.0, 1.0)).astype(np.float32)
    assert kind == "x", kind
    C = shape[1]
    bc = (1, C) + (1,) * (len(shape) - 2)
    sigma = np.exp(rng.uniform(np.log(0.1), np.log(10.0), size=C))
    mean = rng.uniform(-4.0, 4.0, size=C) * sigma
    x = mean.reshape(bc) + sigma.reshape(bc) * rng.standard_normal(shape)
    if pivot is not None:
        x.reshape(shape[0], C, -1)[0, :, 0] = mean + pivot * sigma
    return x.astype(np.float32)


# ---- forward statistics -------------------------------------------------------------------------------------------------------

def stats(x, weight=None, bias=None, eps=1e-5, pairs=None):
    """(mean, biased var, invstd, scale, shift, unbiased var) per channel, by the two-pass definition.  ``pairs``: a list of
    (image, lo, hi) triples to take the statistics over instead of the whole tensor (tests/test_bn_train_ref.py seeds lost and doubled
    slabs with it)."""
    x = _flat(x)
    if pairs is not None:
        x = np.concatenate([x[b, :, lo:hi] for (b, lo, hi) in pairs], axis=1)[None]
    n = x.shape[0] * x.shape[2]
    mean = x.sum(axis=(0, 2)) / n
    m2 = ((x - _ch(mean)) ** 2).sum(axis=(0, 2))
    var = m2 / n
    invstd = 1.0 / np.sqrt(var + eps)
    scale = invstd if weight is None else np.asarray(weight, np.float64) * invstd
    shift = (0.0 if bias is None else np.asarray(bias, np.float64)) - mean * scale
    return mean, var, invstd, scale, shift, m2 / max(n - 1, 1)


def running_update(rm, rv, mean, unbiased_var, momentum):
    m = float(momentum)
    return ((1.0 - m) * np.asarray(rm, np.float64) + m * np.asarray(mean, np.float64),
            (1.0 - m) * np.asarray(rv, np.float64) + m * np.asarray(unbiased_var, np.float64))


def partial_counts(B, HW, pairs=None):
    """[S]: elements per channel that block s reduces."""
    if pairs is None:
        _, pairs = block_pairs(B, HW)
    return np.array([sum(hi - lo for (_, lo, hi) in p) for p in pairs], dtype=np.int64)


# ---- backward -----------------------------------------------------------------------------------------------------------------

def masked(g, out):
    g = _flat(g)
    return g if out is None else np.where(_flat(out) > 0, g, 0.0)


def bwd_sums(x, g, out, mean, pairs=None, absolute=False):
    """[C, S, 2]: per channel and block, sum g' and sum g' (x - mean) over the block's (image, slab) pairs; ``absolute``: the same
    sums of |g'| and |g'| |x - mean| (the magnitude tests.util.assert_round_bound takes)."""
    x, gp = _flat(x), masked(g, out)
    t = gp * (x - _ch(mean))
    if absolute:
        gp, t = np.abs(gp), np.abs(t)
    if pairs is None:
        _, pairs = block_pairs(x.shape[0], x.shape[2])
    res = np.zeros((x.shape[1], len(pairs), 2))
    for s, p in enumerate(pairs):
        for (b, lo, hi) in p:
            res[:, s, 0] += gp[b, :, lo:hi].sum(axis=1)
            res[:, s, 1] += t[b, :, lo:hi].sum(axis=1)
    return res


def bwd(x, g, out, weight, mean, invstd):
    """(g_x, g_weight, g_bias, g_pre) by the closed form, in float64 from the mean and invstd it is handed."""
    x, gp = _flat(x), masked(g, out)
    n = x.shape[0] * x.shape[2]
    mean, invstd = np.asarray(mean, np.float64), np.asarray(invstd, np.float64)
    w = np.ones_like(invstd) if weight is None else np.asarray(weight, np.float64)
    xc = x - _ch(mean)
    db = gp.sum(axis=(0, 2))
    sxc = (gp * xc).sum(axis=(0, 2))
    g_x = _ch(w * invstd) * (gp - _ch(db / n) - xc * _ch(invstd * invstd * sxc / n))
    return g_x, invstd * sxc, db, gp


def apply_from_coef(x, g, out, coef):
    """(g_x, S) of the element-wise pass  k.x * ((g' - k.y) - (x - k.w) * k.z)  with k = coef[c] ([C, 4]); S is the magnitude sum
    |k.x| (|g'| + |k.y| + |x - k.w| |k.z|)."""
    x, gp = _flat(x), masked(g, out)
    k = np.asarray(coef, np.float64)
    kx, ky, kz, kw = (_ch(k[:, i]) for i in range(4))
    return kx * ((gp - ky) - (x - kw) * kz), np.abs(kx) * (np.abs(gp) + np.abs(ky) + np.abs(x - kw) * np.abs(kz))
