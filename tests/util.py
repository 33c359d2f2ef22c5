import numpy as np
import torch


def to_dev(x, dev="cuda"):
    if torch.is_tensor(x):
        return x.to(dev).contiguous()
    if isinstance(x, dict):
        return {k: to_dev(v, dev) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(to_dev(v, dev) for v in x)
    return x


def rel_l2(got, want):
    """||got - want|| / ||want|| over ALL elements, in float64."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    d = want.norm().item()
    return (got - want).norm().item() / d if d > 0 else (got - want).norm().item()


def bad_frac(got, want, rtol, atol):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).abs() > (atol + rtol * want.abs())).double().mean().item()


def assert_close_frac(got, want, rtol=1e-4, atol=1e-6, max_bad_frac=0.0, name="", max_rel_l2=None):
    """|got-want| <= atol + rtol*|want| for all but ``max_bad_frac`` of the elements, and the
    relative L2 error is below 10*rtol.  The outlier allowance exists for quantities whose
    derivative is discontinuous in the inputs (bilinear floor(), min/argmin ties)."""
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.isfinite(got).all(), name + ": non-finite values"
    err = (got - want).abs()
    bad = err > (atol + rtol * want.abs())
    frac = bad.double().mean().item()
    denom = want.norm().item()
    rel_l2 = (got - want).norm().item() / denom if denom > 0 else (got - want).norm().item()
    assert frac <= max_bad_frac, "%s: %.3g of elements out of tolerance (max err %.3g, rel-L2 %.3g)" % (
        name, frac, err.max().item(), rel_l2)
    if max_rel_l2 is not None:     # untrimmed: every element counts, outliers included
        assert rel_l2 <= max_rel_l2, "%s: rel-L2 over all elements %.3g > %.3g" % (name, rel_l2, max_rel_l2)
    # rel-L2 over the elements that are in tolerance (all of them when no outliers are allowed)
    good = ~bad
    dg = want[good].norm().item()
    trimmed = (got[good] - want[good]).norm().item() / dg if dg > 0 else 0.0
    assert trimmed <= 10 * rtol or err[good].max().item() <= atol, "%s: trimmed rel-L2 %.3g" % (name, trimmed)
    return frac, rel_l2


def np_t(a):
    return torch.from_numpy(np.asarray(a))


class GradPool(object):
    """fp64-anchored gradient bound, pooled over cases (seeds) and kept per scale.

    For every case add(s, got, ref32, g64): ``got`` is the HIP gradient, ``ref32`` an fp32 run of the reference
    algorithm (the oracle in fp32, or a golden of the reference itself), ``g64`` the oracle in float64.  check() asserts,
    per scale and over ALL elements of all pooled cases,

        rel-L2(got vs g64)  <= 1.5 * rel-L2(ref32 vs g64) + 1e-6
        #bad(got)           <= 1.5 * #bad(ref32) + 1e-3 * numel        (bad: |err| > 1e-4 * (max|g64| + |g64|))

    i.e. HIP may not be further from exact arithmetic than 1.5x the reference's own fp32 conditioning noise.  No
    additive slack beyond 1e-6 / 1e-3: a gradient that is a few per cent wrong fails.

    And the absolute gate of north_star (1e-4 relative) where the reference is well conditioned: on the elements where the
    fp32 reference itself is within 1e-4 * (max|g64| + |g64|) of fp64 (no floor() / argmin flip in its neighbourhood), HIP
    must be too, for all but 1e-3 of them (its own, independent flips) -- per scale, for every case that goes through a pool:

        #{ |got - g64| > tol  and  |ref32 - g64| <= tol }  <=  1e-3 * #{ |ref32 - g64| <= tol }  +  #{ |ref32 - g64| > tol }

    ``count_floor``: the DepthHints normalisation divides a masked sum by the mask's pixel count (DH/trainer.py:700-708), so
    ONE argmin flip anywhere rescales every gradient element of that scale by 1/count -- 2.6e-4 on a 48 x 80 image, more
    than the 1e-4 gate.  Pools of that variant pass count_floor = 2 / (pixels per image): HIP's element-wise bound for the
    gate is widened by two such flips (the same allowance the dh loss scalar has); 1.6e-5 at 192 x 640."""

    def __init__(self, scales=4, count_floor=0.0):
        self.count_floor = float(count_floor)
        z = lambda: np.zeros(scales)   # noqa: E731
        self.num_h, self.num_r, self.den, self.bad_h, self.bad_r, self.cnt = z(), z(), z(), z(), z(), z()
        self.ok_r, self.bad_h_on_ok = z(), z()

    def add(self, s, got, ref32, g64):
        got, ref32, g64 = (t.detach().double().cpu() for t in (got, ref32, g64))
        assert got.shape == g64.shape == ref32.shape, (got.shape, ref32.shape, g64.shape)
        assert torch.isfinite(got).all()
        self.num_h[s] += float((got - g64).pow(2).sum())
        self.num_r[s] += float((ref32 - g64).pow(2).sum())
        self.den[s] += float(g64.pow(2).sum())
        tol = 1e-4 * g64.abs().max().item() + 1e-4 * g64.abs()
        bad_h, ok_r = (got - g64).abs() > tol, (ref32 - g64).abs() <= tol
        self.bad_h[s] += float(bad_h.sum())
        self.bad_r[s] += float((~ok_r).sum())
        self.ok_r[s] += float(ok_r.sum())
        self.bad_h_on_ok[s] += float((((got - g64).abs() > tol + self.count_floor * g64.abs()) & ok_r).sum())
        self.cnt[s] += g64.numel()

    def check(self, name=""):
        for s in range(len(self.cnt)):
            if self.cnt[s] == 0:
                continue
            e_h, e_r = (self.num_h[s] / self.den[s]) ** 0.5, (self.num_r[s] / self.den[s]) ** 0.5
            print("%s scale %d: rel-L2 vs fp64  hip %.3g  ref32 %.3g | bad elements hip %d ref32 %d of %d" % (
                name, s, e_h, e_r, self.bad_h[s], self.bad_r[s], self.cnt[s]))
            assert e_h <= 1.5 * e_r + 1e-6, "%s scale %d: HIP rel-L2 %.3g vs fp32 reference %.3g (both against fp64)" % (
                name, s, e_h, e_r)
            assert self.bad_h[s] <= 1.5 * self.bad_r[s] + 1e-3 * self.cnt[s], (name, s, self.bad_h[s], self.bad_r[s],
                                                                             self.cnt[s])
            print("%s scale %d: well-conditioned elements %d of %d, HIP beyond 1e-4 on them: %d" % (
                name, s, self.ok_r[s], self.cnt[s], self.bad_h_on_ok[s]))
            # HIP's flips are independent of the reference's: it may have as many of its own, on other elements, as the
            # reference has (on 48 x 80 images a flipped pixel is 1 % of a coarse scale's texels in ANY fp32 implementation)
            assert self.bad_h_on_ok[s] <= max(1e-3 * self.ok_r[s], 1.0) + self.bad_r[s], (
                "%s scale %d: HIP beyond 1e-4 on %d of the %d elements where the fp32 reference is within 1e-4 of fp64" % (
                    name, s, self.bad_h_on_ok[s], self.ok_r[s]))


def no_miopen(fn):
    """Decorator for tests whose only library convolutions belong to the SCAFFOLDING network (oracle.synth.TinyDepthNet through
    nn.Conv2d): run them on ATen's own GPU convolution.  On a fresh box MIOpen compiles a kernel per new (shape, direction) --
    3-5 s each, 45 s for the fifteen configurations of one harness test -- for arithmetic no assertion is about."""
    import functools

    import torch

    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with torch.backends.cudnn.flags(enabled=False):
            return fn(*a, **kw)
    return wrapped


# ---- float64 anchors of the convolution kernels (tests/test_gpu_conv_anchor.py, tests/test_gpu_conv_epilogue.py) ----------------

def rel_fp64(a, ref64):
    """rel-L2 of ``a`` against a float64 reference on the same device."""
    return float((a.detach().double() - ref64).norm() / ref64.norm())


def fp64_bound(name, e_hip, e_lib, chain=0, factor=1.5, chain_margin=1.0):
    """rel-L2(HIP vs fp64) <= factor x rel-L2(library fp32 vs fp64) + 1e-7.

    ``chain``: length of the kernel's single fp32 accumulation chain per output (the direct MFMA kernels K11 / K15 / K16
    sum all C x 9 products of an output into ONE accumulator; the library's implicit GEMMs split that sum): a chain of n
    rounded additions carries ~ 0.5 sqrt(n) 2^-24 of relative error (random-walk estimate), which is allowed beside the
    library-relative bound -- 1.4e-6 for layer4.0's 2,304 products, two orders below north_star's 1e-4.
    ``factor``: 2 for a chain of two launches measured as one (a block node), each held to 1.5 on its own.
    ``chain_margin``: a multiple of the chain estimate (the same 1.5 the library gets, where the estimate is the kernel's
    measured error itself)."""
    print("%-44s rel-L2 vs fp64: hip %.3g  library fp32 %.3g  (ratio %.2f)" % (name, e_hip, e_lib, e_hip / e_lib if e_lib else 0.0))
    assert e_hip <= max(factor * e_lib + 1e-7, chain_margin * 0.5 * chain ** 0.5 * 2.0 ** -24), (name, e_hip, e_lib)


def conv_data(B, C, K, H, W, seed):
    """x ~ N(0, 1) [B, C, H, W] and a He-scaled 3x3 filter [K, C, 3, 3] on the GPU (outputs of the order of x)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g).cuda()
    w = (torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).cuda()
    return x, w


# ---- element-wise rounding bound (tests/test_round_bound.py, tests/test_gpu_stem_head_anchor.py) ---------------------------------

U32 = 2.0 ** -24        # unit roundoff of fp32 (round to nearest)


def round_bound_violations(got, ref64, S, n_round, extra=None):
    """Boolean mask of the elements that break  |got - ref64| <= n_round * 2^-24 * S (+ extra).

    ``ref64``: the operation in float64.  ``S``: the same operation on absolute values in float64 (conv(|x|, |w|) + |b|, or
    sum |g * x| per tap): the sum of the magnitudes every rounding acts on.  ``n_round``: the number of fp32 roundings on the
    longest path one product takes to the output, read from the kernel -- each rounding of a partial sum p errs by at most
    2^-24 |p| <= 2^-24 S, so n of them by n 2^-24 S to first order (the second-order term is n 2^-24 / 2 of that).
    ``extra``: a separately derived float64 term of the same shape (K14's input normalisation), never a measured number.
    An element that is NaN or infinite is a violation: nothing here is an outlier share or an additive slack."""
    got, ref64, S = got.detach().double(), ref64.detach().double(), S.detach().double()
    assert got.shape == ref64.shape == S.shape, (got.shape, ref64.shape, S.shape)
    bound = float(n_round) * U32 * S
    if extra is not None:
        bound = bound + extra.detach().double()
    return ~((got - ref64).abs() <= bound)


def assert_round_bound(name, got, ref64, S, n_round, extra=None):
    """Every element inside the derived bound of round_bound_violations; prints and returns the largest share of it used."""
    bad = round_bound_violations(got, ref64, S, n_round, extra)
    bound = float(n_round) * U32 * S.detach().double() + (0 if extra is None else extra.detach().double())
    err = (got.detach().double() - ref64.detach().double()).abs()
    used = float(torch.nan_to_num(err / bound.clamp_min(1e-300), nan=float("inf")).max()) if err.numel() else 0.0
    print("%-52s n_round %6d  worst |err| / bound %.3f" % (name, n_round, used))
    assert not bool(bad.any()), "%s: %d of %d elements beyond n_round * 2^-24 * S (n_round %d, worst share %.3g)" % (
        name, int(bad.sum()), bad.numel(), n_round, used)
    return used
