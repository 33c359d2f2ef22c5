"""numpy restatement of K23 (csrc/l0_fused.hip): one fused iteration of the L0 object attack for a given dtype, op by op in the
kernel's order, plus the controller (mask-weight selection and the host's exit) replayed from a count array.

In float32 every numpy operation rounds once, as the kernel's un-contracted operations do (its division and square root are the
correctly rounded forms), so with the mask weight at zero the kernel has to reproduce this bit for bit; with the mask term on,
numpy's tanh and the device's differ in the last place.  In float64 it is the anchor of the update."""
import math

import numpy as np

B1, B2, EPS = 0.5, 0.9, 1e-8
REC = 8


def adam_table(steps, lr):
    """float64 [2 * steps, 2]: (lr / (1 - b1^t), sqrt(1 - b2^t)) for t = 1 .. 2 * steps."""
    return np.asarray([(lr / (1.0 - B1 ** t), math.sqrt(1.0 - B2 ** t)) for t in range(1, 2 * steps + 1)], dtype=np.float64)


def below(c_i, c_0, thresh, dtype=np.float32):
    """count[i] / count[0] <= thresh in ``dtype`` (0 / 0 = nan compares false: the mask weight stays on)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return bool(dtype(c_i) / dtype(c_0) <= dtype(thresh))


def replay_controller(counts, steps, mask_wt, thresh, dtype=np.float32):
    """The attack's decisions from its count array: ([mask weight of every iteration that ran], did the loop exit early)."""
    mws = []
    for stp in range(2 * steps):
        bl = below(counts[stp], counts[0], thresh, dtype)
        if stp >= steps and bl:
            return mws, True
        mws.append(dtype(0) if bl else dtype(mask_wt))
    return mws, False


def make_state(pos, neg, steps, count0, dtype=np.float32):
    """pos, neg: [C, HW].  count: int64 [2 * steps + 1] with count[0] given, rec [2 * steps, REC], cursor 0."""
    z = lambda: np.zeros_like(pos, dtype=dtype)     # noqa: E731
    count = np.zeros(2 * steps + 1, dtype=np.int64)
    count[0] = count0
    return dict(pos=pos.astype(dtype).copy(), neg=neg.astype(dtype).copy(), m_pos=z(), v_pos=z(), m_neg=z(), v_neg=z(), adv=z(),
                count=count, rec=np.zeros((2 * steps, REC), dtype=dtype), cursor=0, steps=steps)


def compose(obj, pos, neg, l0_clip, dtype=np.float32):
    """clamp(obj + (clamp(pos,0,1) - clamp(neg,0,1)), 0, 1) and the number of pixels of the thresholded pattern (K5's forward)."""
    f = dtype
    pp, pn = np.clip(pos, f(0), f(1)), -np.clip(neg, f(0), f(1))
    t1, t2 = np.where(pp < f(l0_clip), f(0), pp), np.where(pn > -f(l0_clip), f(0), pn)
    acc = np.zeros(pos.shape[1], dtype=f)
    for c in range(pos.shape[0]):
        acc = acc + np.abs(t1[c] + t2[c])
    return np.clip(obj + (pp + pn), f(0), f(1)), int(np.count_nonzero(acc != 0))


def mask_grad(p, mw, dtype):
    """mw * d mask_cost / d p: (1 - th^2) / 10 / (2 - 1e-7) / HW at the first maximal channel of every pixel, zero elsewhere."""
    f = dtype
    hw = p.shape[1]
    th = np.tanh(p / f(10))
    val = th / f(2.0 - 1e-7) + f(0.5)
    best = np.argmax(val, axis=0)       # the first maximal channel, as torch.max(dim=1)
    up = f(mw) / f(hw)
    g = up * (f(1) - th * th) / f(10) / f(2.0 - 1e-7)
    out = np.zeros_like(p)
    cols = np.arange(hw)
    out[best, cols] = g[best, cols]
    return out


def adam(p, m, v, g, ss, bc2s, dtype):
    f = dtype
    m = m * f(B1) + g * f(1.0 - B1)
    v = v * f(B2) + (g * g) * f(1.0 - B2)
    den = np.sqrt(v) / bc2s + f(EPS)
    p = p + (-ss) * (m / den)
    return p, m, v


def fused_step(st, obj, g_adv, tab, mask_wt, thresh, l0_clip, adv_cost=0.0, mask_cost=0.0, dtype=np.float32):
    """One launch of K23 on the state ``st`` (in place).  ``tab``: adam_table() in float64, rounded to ``dtype`` here."""
    f = dtype
    it, steps = st["cursor"], st["steps"]
    if it < 0 or it >= 2 * steps:
        return st
    c_i, c_0 = st["count"][it], st["count"][0]
    bl = below(c_i, c_0, thresh, dtype)
    mw = f(0) if bl else f(mask_wt)
    ss, bc2s = f(tab[it, 0]), f(tab[it, 1])
    obj, g_adv = obj.astype(f), g_adv.astype(f)
    p, q = st["pos"], st["neg"]
    v = obj + (np.clip(p, f(0), f(1)) - np.clip(q, f(0), f(1)))
    g = np.where((v >= 0) & (v <= 1), g_adv, f(0))
    zero = np.zeros_like(p)
    gp = np.where((p >= 0) & (p <= 1), g, f(0)) + (mask_grad(p, mw, f) if mw != 0 else zero)
    gn = np.where((q >= 0) & (q <= 1), -g, f(0)) + (mask_grad(q, mw, f) if mw != 0 else zero)
    st["pos"], st["m_pos"], st["v_pos"] = adam(p, st["m_pos"], st["v_pos"], gp, ss, bc2s, f)
    st["neg"], st["m_neg"], st["v_neg"] = adam(q, st["m_neg"], st["v_neg"], gn, ss, bc2s, f)
    st["adv"], n = compose(obj, st["pos"], st["neg"], l0_clip, f)
    st["count"][it + 1] += n
    st["rec"][it] = [f(c_i), mw, f(adv_cost), f(mask_cost), f(it + 1), f(1 if bl else 0), f(0), f(0)]
    st["cursor"] = it + 1
    return st
