"""The element-wise rounding bound of tests/util.py (round_bound_violations) is not vacuous: on the CPU, a correct fp32
accumulation in a kernel's order passes it with room, and each of the faults a strip kernel can have -- a tap one column off,
a strip's last row without its ky = 2 taps, an unwritten strip column, a bias added twice, two channels' taps swapped, a strip
row missing from a weight-gradient sum -- is flagged on the outputs it touches.

The emulated chain is one fused multiply-add per tap (float64 product and sum of fp32 operands, rounded to fp32: a product of
two fp32 numbers is exact in float64), so n_round = 9 C for the taps + 1 for the bias, as for K13's tile kernel."""
import numpy as np
import pytest
import torch

from tests.util import round_bound_violations

HO, WO = 43, 66             # outputs: two strip rows (40 + 3) and two strip columns (62 + 4)
FR, FCOLS = 40, 62          # the strip geometry of csrc/head_conv.hip


def _fma(acc, a, b):
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def _data(C, seed=3):
    r = np.random.RandomState(seed)
    x = r.randn(C, HO + 2, WO + 2).astype(np.float32)
    w = (r.randn(C, 3, 3) * (2.0 / (9 * C)) ** 0.5).astype(np.float32)
    b = np.float32(0.3)
    return x, w, b


def _conv32(x, w, b, tap=None, bias_twice=False):
    """fp32 tap-by-tap accumulation; ``tap(c, ky, kx, patch, acc)`` may replace a tap's [HO, WO] input patch."""
    acc = np.zeros((HO, WO), np.float32)
    for c in range(x.shape[0]):
        for ky in range(3):
            for kx in range(3):
                patch = x[c, ky:ky + HO, kx:kx + WO]
                if tap is not None:
                    patch = tap(c, ky, kx, patch)
                acc = _fma(acc, patch, np.full_like(patch, w[c, ky, kx]))
    acc = (acc + b).astype(np.float32)
    return (acc + b).astype(np.float32) if bias_twice else acc


def _ref64(x, w, b):
    x64, w64 = np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64))
    ref, S = np.full((HO, WO), float(b)), np.full((HO, WO), abs(float(b)))
    for c in range(x.shape[0]):
        for ky in range(3):
            for kx in range(3):
                ref += x[c, ky:ky + HO, kx:kx + WO].astype(np.float64) * float(w[c, ky, kx])
                S += x64[c, ky:ky + HO, kx:kx + WO] * w64[c, ky, kx]
    return torch.from_numpy(ref), torch.from_numpy(S)


def _bad(got, ref, S, n):
    return round_bound_violations(torch.from_numpy(got), ref, S, n).numpy()


@pytest.mark.parametrize("C", [4, 16, 128])
def test_forward_bound_passes_a_clean_chain_and_flags_every_seeded_fault(C):
    x, w, b = _data(C)
    ref, S = _ref64(x, w, b)
    n = 9 * C + 1
    clean = _conv32(x, w, b)
    assert not _bad(clean, ref, S, n).any()
    used = float((np.abs(clean - ref.numpy()) / (n * 2.0 ** -24 * S.numpy())).max())
    print("C = %d: the clean fp32 chain uses %.3f of the bound" % (C, used))
    assert used < 0.5        # room on both sides: the count is an upper bound, not a fit

    # one tap reads the neighbouring column: a change of ONE of the 9 C products of every output
    def shifted(c, ky, kx, patch):
        return x[c, ky:ky + HO, kx + 1:kx + 1 + WO] if (c, ky, kx) == (C - 1, 1, 0) else patch
    bad = _bad(_conv32(x, w, b, tap=shifted), ref, S, n)
    print("C = %d: one tap a column off is flagged on %.3f of the outputs" % (C, bad.mean()))
    assert bad.mean() > (0.85 if C == 128 else 0.99)

    # the last row of a 40-row strip loses its ky = 2 taps
    def seam(c, ky, kx, patch):
        if ky != 2:
            return patch
        p = patch.copy()
        p[FR - 1] = 0
        return p
    bad = _bad(_conv32(x, w, b, tap=seam), ref, S, n)
    assert bad[FR - 1].mean() > 0.99 and not np.delete(bad, FR - 1, 0).any()

    # column 61 of a 62-column strip is left unwritten (the output buffer is pre-filled with NaN)
    got = clean.copy()
    got[:, FCOLS - 1] = np.nan
    bad = _bad(got, ref, S, n)
    assert bad[:, FCOLS - 1].all() and not np.delete(bad, FCOLS - 1, 1).any()

    # the bias is added twice
    assert _bad(_conv32(x, w, b, bias_twice=True), ref, S, n).all()

    # two channels' taps are swapped
    w2 = w.copy()
    w2[[0, 1]] = w2[[1, 0]]
    assert _bad(_conv32(x, w2, b), ref, S, n).mean() > 0.99


@pytest.mark.parametrize("C", [4, 16, 128])
def test_weight_gradient_bound_passes_a_strip_ordered_sum_and_flags_a_dropped_strip_row(C):
    """dW[c, ky, kx] = sum g * x summed as K13 does: a lane runs down the 40 rows of its strip column (40 FMAs), the 64 lanes
    meet in a tree of depth 6, the strips are added in order.  n_round = 40 + 6 + strips."""
    x, _, _ = _data(C, 5)
    g = (np.random.RandomState(6).randn(HO, WO) / (HO * WO) ** 0.5).astype(np.float32)
    strips = [(y0, x0) for y0 in range(0, HO, FR) for x0 in range(0, WO, FCOLS)]
    n = FR + 6 + len(strips)

    def wgrad32(drop=None):
        out = np.zeros((C, 3, 3), np.float32)
        for (y0, x0) in strips:
            gs = np.zeros((FR, 64), np.float32)
            blk = g[y0:y0 + FR, x0:x0 + FCOLS]
            gs[:blk.shape[0], :blk.shape[1]] = blk
            if drop == (y0, x0):
                gs[FR // 2] = 0                     # one strip row never reaches the sum
            for c in range(C):
                for ky in range(3):
                    for kx in range(3):
                        xs = np.zeros((FR, 64), np.float32)
                        xb = x[c, y0 + ky:y0 + ky + blk.shape[0], x0 + kx:x0 + kx + blk.shape[1]]
                        xs[:xb.shape[0], :xb.shape[1]] = xb
                        lane = np.zeros(64, np.float32)
                        for r in range(FR):
                            lane = _fma(lane, gs[r], xs[r])
                        while lane.size > 1:
                            lane = (lane[0::2] + lane[1::2]).astype(np.float32)
                        out[c, ky, kx] = np.float32(out[c, ky, kx] + lane[0])
        return out

    ref, S = np.zeros((C, 3, 3)), np.zeros((C, 3, 3))
    for ky in range(3):
        for kx in range(3):
            p = g.astype(np.float64)[None] * x[:, ky:ky + HO, kx:kx + WO].astype(np.float64)
            ref[:, ky, kx], S[:, ky, kx] = p.sum((1, 2)), np.abs(p).sum((1, 2))
    ref, S = torch.from_numpy(ref), torch.from_numpy(S)
    clean = wgrad32()
    assert not _bad(clean, ref, S, n).any()
    assert float((np.abs(clean - ref.numpy()) / (n * 2.0 ** -24 * S.numpy())).max()) < 0.5
    assert _bad(wgrad32(drop=strips[0]), ref, S, n).mean() > 0.95
