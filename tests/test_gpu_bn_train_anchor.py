"""Float64 anchors of K9's train forms (csrc/encoder_glue.hip): dmh_bn_train_stats_tracked (bn_stats_partial_kernel +
bn_stats_finalize_kernel) and dmh_bn_train_bwd (bn_bwd_partial_kernel + bn_bwd_finalize_kernel + bn_bwd_apply_vec / _scalar), through
the C ABI -- and dmh_channel_sum, the third reduction that deals slabs to blocks -- against tests/bn_train_ref.py (plain numpy
float64; tests/test_bn_train_ref.py holds that reference to torch's float64
operators, feeds every check of this file the reference rounded to fp32 and seeded faults, and asserts the input conditions on the
CPU).  One operator-level test goes through ops.bn_act_train and ops.stem_bn_relu_pool_train.

Launch forms, from the host code -- the case list is written against these rules, every case asserts the form it is meant to reach,
and a change of a rule makes the list visibly stale:

    slab        4 * NT = 1024 elements of one (image, channel) plane
    S           min(64, ceil(HW / 1024)) blocks per channel; block s owns slabs s, s + S, ...: slabs_of(HW, s, S) of them per image
    statistics  (HW & 3) == 0: vector -- the block's B * nk (image, slab) pairs as ONE loop, four pairs per step, the tail clamped;
                else scalar -- image by image, slab by slab, four strided elements per thread
    backward    the same rule; the vector loop takes two pairs per step.  <RELU> from out != NULL
    apply       (HW & 3) == 0: bn_bwd_apply_vec, else _scalar; <RELU, RES> from out != NULL, g_pre != NULL
    channel sum (HW & 3) == 0: the backward's column 0; else rows of NT floats dealt to the blocks, one chain per thread
    workspaces  statistics C * S * 3 floats (n, mean, M2); backward 4 C (coef) + C * S * 2; channel sum C * S

No assertion rests on a hand-derived worst case for Welford / Chan arithmetic:

  A  exact, on both kinds of input: the n of every statistics partial; num_batches_tracked; g_pre == g * [out > 0] (``out`` is an
     INPUT of the backward, so the mask is never in doubt and no element is excluded anywhere in this file); g_bias, g_weight and
     the four coefficients rebuilt from the fp32 partials read back from the workspace (the finalize kernel adds in double, in
     block order, and casts once: equality).
  B  dyadic input (tests/bn_train_ref.py): every product and partial sum of the backward's reductions is exact in fp32 whatever the
     order, so each of the C * S * 2 partials equals the float64 sum over its slab set BIT FOR BIT, and so do g_bias and g_weight.
     A lost or doubled slab has no tolerance to hide in.
  C  generic input, element by element:  |got - ref64| <= n_round * 2^-24 * S  (tests/util.py: assert_round_bound), n_round read
     from the kernel (constants below): the backward partials; the apply pass against the float64 evaluation FROM THE fp32
     COEFFICIENTS READ BACK (this sees a wrong channel index on ragged planes); the running-mean update from the kernel's own
     save_mean.
  D  generic input, C = 64: statistics, the normalised output and the gradients against float64, relative to what the fp32 library
     (ATen's native_batch_norm / native_batch_norm_backward on the device) achieves on the same data -- tests/util.py: fp64_bound,

         e_hip <= max(1.5 * e_lib + 1e-7, cond * 0.5 * sqrt(n_round) * 2^-24)

     cond = 1 for mean-type quantities; for variance-type quantities (invstd, scale, shift, running_var, the normalised output)
     cond = 1 + max_c ((x[0, c, 0] - mean_c) / sigma_c)^2 from the float64 reference: the kernel shifts its sums by the channel's
     first element k, and M2 = sum (x - k)^2 - (sum (x - k))^2 / n loses the factor (sigma^2 + (mean - k)^2) / sigma^2.  The shift
     bias - mean * scale carries the relative error of scale on its second term, so it is variance-type.  A second variant puts
     that element 8 sigma off the mean: it prices the pivot.
  E  the operator level: output, gradients and running buffers of the autograd nodes under rule D with factor 2 (two launches
     measured as one); the float64 backward masks with the HIP forward's own output.

Every launch runs twice and must reproduce itself bit for bit.  Every output and workspace handed to the C ABI is NaN before the
call and has a NaN guard behind it, which must be intact afterwards."""
import zlib

import numpy as np
import pytest
import torch

from tests import bn_train_ref as R
from tests.util import assert_round_bound as _rb, fp64_bound as _bound

pytestmark = pytest.mark.gpu

GUARD = 4096                        # floats of NaN behind every output and workspace
EPS = float(np.float32(1e-5))       # the C ABI takes eps and momentum as float: the references take the same values
MOMENTUM = float(np.float32(0.1))

# ---- n_round, in units of 2^-24, read from the kernels ------------------------------------------------------------------------------
WAVES = R.NT // 64                  # waves of 64 lanes per block
SHUFFLES = 6                        # log2(WAVE) __shfl_down steps


def n_part(B, nk, column):
    """bn_bwd_partial_kernel, one partial: a thread's chain takes one addition (column 1: one fmaf) per (image, slab) pair, B * nk;
    "(a[0] + a[1]) + (a[2] + a[3])": 2; six shuffle steps; "t += red[i]" for the three other waves; column 1 rounds x - mean
    before the fmaf: 1 more."""
    return B * nk + 2 + SHUFFLES + (WAVES - 1) + (1 if column else 0)


def n_channel_sum(B, HW):
    """channel_sum_partial_kernel + the double finish: the vector form is the backward's column 0; the scalar form walks the plane in
    steps of S * NT floats on ONE chain per thread (and deals the plane by rows of NT floats, not by slabs: only its total is held);
    + 1 for the cast of the double sum."""
    S, sets = R.slab_sets(HW)
    chain = B * max(len(r) for r in sets) if HW % 4 == 0 else B * -(-HW // (S * R.NT))
    return chain + 2 + SHUFFLES + (WAVES - 1) + 1


N_APPLY = 5         # k.x * ((g' - k.y) - (x - k.w) * k.z): two differences, a product, a difference, a product; an FMA only lowers it
N_RUNNING = 4       # (1.f - momentum) * old + momentum * mean: a difference, two products, a sum
# wf_merge(a, b): d = b.mean - a.mean (1), f = b.n / n (1), mean = a.mean + d * f (2): 4 roundings meet in the mean;
# M2 = a.m2 + b.m2 + d * d * a.n * f: three products and two sums on top of d and f: 7.  n = a.n + b.n is an integer below 2^24: exact.
MERGE_MEAN, MERGE_M2 = 4, 7


def n_merges(S):
    """wf_merge calls on the longest path: six shuffle steps, three wave joins, and the finalize kernel's S - 1 (its first merge onto
    n = 0 returns the partial unchanged)."""
    return SHUFFLES + (WAVES - 1) + (S - 1)


def n_mean(B, nk, S):
    """d = v - k (1), B * nk additions of a chain, 2 to join the four chains, k + s1 / n (2), then the merges."""
    return 1 + B * nk + 2 + 2 + MERGE_MEAN * n_merges(S)


def n_m2(B, nk, S):
    """d = v - k (1), B * nk fmaf of a chain, 2 to join, s2 - s1 * s1 / n (3), then the merges."""
    return 1 + B * nk + 2 + 3 + MERGE_M2 * n_merges(S)


RSQRT = 2                           # rsqrtf: one ulp, two units


def n_invstd(B, nk, S):
    return n_m2(B, nk, S) + 2 + RSQRT       # m2 / n, + eps, rsqrtf


def n_stats(B, HW):
    """n_round of every line of rule D for a [B, C, HW] tensor, on the block with the most slabs."""
    S, sets = R.slab_sets(HW)
    nk = max(len(r) for r in sets)
    inv = n_invstd(B, nk, S)
    return {"save_mean": n_mean(B, nk, S), "running_mean": n_mean(B, nk, S) + N_RUNNING, "save_invstd": inv, "scale": inv + 1,
            "shift": inv + 1 + 2, "running_var": n_m2(B, nk, S) + 1 + N_RUNNING, "out": inv + 1 + 2 + 1,
            "g_bias": n_part(B, nk, 0) + 1, "g_weight": n_part(B, nk, 1) + 1, "g_x": n_part(B, nk, 1) + 1 + N_APPLY}


# ---- cases: the smallest shapes at which each form and edge exists ------------------------------------------------------------------
# (B, HW, form, S, blocks that own two slabs, elements of the plane's last slab); C = 3.  B * nk per block: 1, 2, 3, 5 and 6 / 3 -- 1,
# odd, and no multiple of 4: the clamped tails of the four-wide and of the two-wide loop are both live.
CASES = [
    (2, 1, "scalar", 1, 0, 1),              # one element per image: 255 threads hold n = 0, the n == 0 branches of wf_merge decide
    (2, 4, "vector", 1, 0, 4),              # one word per image
    (1, 63, "scalar", 1, 0, 63),            # the ragged end inside wave 0
    (3, 252, "vector", 1, 0, 252),          # 63 words: the ragged last word inside wave 0 of the vector form ...
    (1, 252, "vector", 1, 0, 252),          # ... and B * nk = 1
    (3, 1028, "vector", 2, 0, 4),           # the second slab holds one word
    (5, 1028, "vector", 2, 0, 4),           # B * nk = 5: one full step of four (two of two) and a tail of one
    (2, 1030, "scalar", 2, 0, 6),           # the second slab holds six floats
    (3, 66564, "vector", 64, 2, 4),         # 66 slabs on 64 blocks: blocks 0 and 1 own two; the last slab is one word
    (1, 66563, "scalar", 64, 2, 3),         # the same, the last slab three floats
]
C_STRUCT = 3
DATA = ("dyadic", "generic")
# backward modes: (relu: out handed, g_pre wanted, weight handed, g_weight / g_bias wanted) -- all four <RELU, RES> instantiations
BWD_MODES = [(True, True, True, True), (True, False, False, True), (False, True, True, False), (False, False, True, True)]
# statistics modes: (weight, bias, running buffers, num_batches_tracked) handed
STATS_MODES = [(True, True, True, True), (False, True, True, False), (True, False, False, True), (False, False, False, False)]
# rule D: (B, HW), C = 64; both forms at S = 1, S = 2 and 66 slabs on 64 blocks
C_STAT = 64
D_CASES = [(2, 1), (2, 4), (3, 63), (3, 252), (3, 1028), (3, 1030), (2, 66564), (2, 66563)]
D_VARIANTS = (None, 8.0)            # the pivot element as drawn, and 8 sigma off the mean
# rule E: (H, W): one vector and one scalar plane of the case table, B = 3
E_SHAPES = [(2, 514), (10, 103)]


def case_form(B, HW):
    S, sets = R.slab_sets(HW)
    assert all(len(r) in (1, 2) for r in sets)
    last = HW - ((HW + R.SLAB - 1) // R.SLAB - 1) * R.SLAB
    return (R.launch_form(HW), S, sum(len(r) == 2 for r in sets), last)


def _id(case):
    return "%dx%d-%s" % (case[0], case[1], case[2]) if len(case) > 2 else "%dx%d" % case


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) % (2 ** 31))


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


_REF = {}


def _cached(fn):
    def wrapped(*key):
        k = (fn.__name__,) + key
        if k not in _REF:
            _REF[k] = _freeze(fn(*key))
        return _REF[k]
    return wrapped


# ---- references: inputs and float64 results of a case, computed once, shared read-only ----------------------------------------------

def _inputs(B, C, HW, data, rng, pivot=None):
    if data == "dyadic":
        mean = R.dyadic((C,), rng, "mean")
        return {"x": R.dyadic((B, C, HW), rng, "x", mean), "mean": mean, "invstd": R.dyadic((C,), rng, "invstd"),
                "weight": R.dyadic((C,), rng, "weight"), "bias": R.dyadic((C,), rng, "bias"),
                "g": R.dyadic((B, C, HW), rng, "grad"), "out": R.dyadic((B, C, HW), rng, "out")}
    d = {"x": R.generic((B, C, HW), rng, "x", pivot), "weight": R.generic((C,), rng, "weight"), "bias": R.generic((C,), rng, "bias"),
         "g": R.generic((B, C, HW), rng, "grad"), "out": R.generic((B, C, HW), rng, "out")}
    st = R.stats(d["x"], None, None, EPS)
    d["mean"], d["invstd"] = st[0].astype(np.float32), st[2].astype(np.float32)    # what the forward would hand the backward
    return d


@_cached
def stats_reference(case, data):
    B, HW = case[:2]
    d = _inputs(B, C_STRUCT, HW, data, _rng("stats", case, data))
    rng = _rng("buffers", case, data)
    d.update(B=B, HW=HW, C=C_STRUCT, exact=data == "dyadic", S=R.slab_sets(HW)[0], counts=R.partial_counts(B, HW),
             rm0=rng.uniform(-1, 1, C_STRUCT).astype(np.float32), rv0=rng.uniform(0.5, 2, C_STRUCT).astype(np.float32))
    return d


@_cached
def bwd_reference(case, data, mode):
    B, HW = case[:2]
    relu, want_pre, with_weight, want_wb = mode
    d = dict(_inputs(B, C_STRUCT, HW, data, _rng("bwd", case, data)))
    d.update(B=B, HW=HW, C=C_STRUCT, exact=data == "dyadic", S=R.slab_sets(HW)[0], nk=[len(r) for r in R.slab_sets(HW)[1]], mode=mode)
    if not relu:
        d["out"] = None
    if not with_weight:
        d["weight"] = None
    d["part"] = R.bwd_sums(d["x"], d["g"], d["out"], d["mean"])
    d["part_S"] = R.bwd_sums(d["x"], d["g"], d["out"], d["mean"], absolute=True)
    _, d["g_weight"], d["g_bias"], d["g_pre"] = R.bwd(d["x"], d["g"], d["out"], d["weight"], d["mean"], d["invstd"])
    return d


def d_reference(case, pivot):
    """Rule D's inputs and float64 results (not cached: up to 34 MB per tensor, used by one test)."""
    B, HW = case
    d = _inputs(B, C_STAT, HW, "generic", _rng("D", case, pivot), pivot)
    d.update(B=B, HW=HW, C=C_STAT, pivot=pivot)
    mean, var, invstd, scale, shift, unbiased = R.stats(d["x"], d["weight"], d["bias"], EPS)
    d["ref"] = {"save_mean": mean, "save_invstd": invstd, "scale": scale, "shift": shift, "var": var, "unbiased": unbiased}
    d["ref"]["running_mean"], d["ref"]["running_var"] = R.running_update(0.0, 0.0, mean, unbiased, 1.0)
    d["cond"] = float(1.0 + (((d["x"][:, :, 0][0].astype(np.float64) - mean) ** 2) / var).max())
    return d


# ---- checks: ``got`` are fp32 CPU tensors, from the GPU here and from seeded faults in tests/test_bn_train_ref.py -------------------

def _np(a):
    return None if a is None else (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a))


def _t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _is32(name, a, shape):
    a = _np(a)
    assert a.dtype == np.float32 and tuple(a.shape) == tuple(shape), (name, a.dtype, a.shape, shape)
    return a


def _equal(name, got, want64):
    """Bit equality with the float64 value cast to fp32 (NaN nowhere; +0 == -0 does not occur in a sum)."""
    want = np.asarray(want64, np.float64).astype(np.float32)
    got = _is32(name, got, want.shape)
    bad = ~(got == want)
    assert not bad.any(), "%s: %d of %d entries differ from the float64 value cast to fp32 (first: got %r, want %r)" % (
        name, int(bad.sum()), bad.size, got[bad].flat[0], want[bad].flat[0])


def check_stats_partials(name, d, part):
    """A: the n of every partial is the size of its slab set times B -- an integer below 2^24, exact in fp32 -- and they add up to
    B * HW."""
    part = _is32(name + " partials", part, (d["C"], d["S"], 3))
    n = part[:, :, 0].astype(np.float64)
    assert np.array_equal(n, np.broadcast_to(d["counts"].astype(np.float64), n.shape)), (name, "n of the partials", n[0], d["counts"])
    assert (n.sum(axis=1) == d["B"] * d["HW"]).all(), (name, "sum of n", n.sum(axis=1), d["B"] * d["HW"])
    assert np.isfinite(part).all(), name + ": a partial is not finite"


def check_counter(name, before, after, handed):
    """A: num_batches_tracked goes up by exactly 1 per call, and is untouched when NULL is passed."""
    assert int(after) == int(before) + (1 if handed else 0), (name, int(before), int(after), handed)


def check_running_mean(name, d, rm, save_mean, momentum=MOMENTUM):
    """C: running_mean against (1 - m) * old + m * save_mean in float64 from the kernel's own save_mean."""
    save_mean = _is32(name + " save_mean", save_mean, (d["C"],)).astype(np.float64)
    ref, _ = R.running_update(d["rm0"], 0.0, save_mean, 0.0, momentum)
    S = np.abs((1.0 - momentum) * d["rm0"].astype(np.float64)) + np.abs(momentum * save_mean)
    return _rb(name + " running_mean", torch.from_numpy(_is32(name, rm, (d["C"],))), _t64(ref), _t64(S), N_RUNNING)


def check_bwd_exact(name, d, coef, part, g_weight, g_bias, g_pre):
    """A: g_pre is the masked gradient; g_bias, g_weight and the coefficients are the finalize kernel's double sums, in block
    order, of the fp32 partials it was handed."""
    C, S, B, HW = d["C"], d["S"], d["B"], d["HW"]
    relu, want_pre, with_weight, want_wb = d["mode"]
    assert (g_pre is None) == (not want_pre) and (g_weight is None) == (not want_wb) and (g_bias is None) == (not want_wb), name
    if want_pre:
        want = d["g"] if d["out"] is None else d["g"] * (d["out"] > 0)
        got = torch.from_numpy(_is32(name + " g_pre", g_pre, want.shape))
        assert torch.equal(got, torch.from_numpy(np.array(want, np.float32))), "%s: g_pre is not g * [out > 0] (%d elements)" % (
            name, int((got != torch.from_numpy(np.array(want, np.float32))).sum()))
    part = _is32(name + " partials", part, (C, S, 2)).astype(np.float64)
    s1, s2 = np.zeros(C), np.zeros(C)
    for s in range(S):
        s1, s2 = s1 + part[:, s, 0], s2 + part[:, s, 1]
    inv_n = 1.0 / (float(B) * float(HW))
    isd = d["invstd"].astype(np.float64)
    w = np.ones(C) if d["weight"] is None else d["weight"].astype(np.float64)
    if want_wb:
        _equal(name + " g_bias = float(sum of the partials)", g_bias, s1)
        _equal(name + " g_weight = float(sum of the partials * invstd)", g_weight, s2 * isd)
    coef = _is32(name + " coef", coef, (C, 4))
    _equal(name + " coef.x = float(w * invstd)", coef[:, 0], w * isd)
    _equal(name + " coef.y = float(s1 / n)", coef[:, 1], s1 * inv_n)
    _equal(name + " coef.z = float(s2 * invstd^2 / n)", coef[:, 2], s2 * isd * isd * inv_n)
    assert np.array_equal(coef[:, 3], d["mean"]), name + ": coef.w is not the mean"


def check_bwd_dyadic(name, d, part, g_weight, g_bias):
    """B: on dyadic input every partial, and g_bias and g_weight, equal the float64 sums bit for bit."""
    assert d["exact"]
    _equal(name + " partials", part, d["part"])
    if g_bias is not None:
        _equal(name + " g_bias", g_bias, d["g_bias"])
        _equal(name + " g_weight", g_weight, d["g_weight"])


def check_bwd_partials(name, d, part):
    """C: every partial within n_part * 2^-24 * (sum |g'|, sum |g'| |x - mean|) over its slab set."""
    part = _is32(name + " partials", part, (d["C"], d["S"], 2))
    used, nk = [], np.array(d["nk"])
    for k in sorted(set(d["nk"])):          # the blocks that own k slabs per image share an n_round
        for col in (0, 1):
            used.append(_rb("%s partials, %d slab(s), column %d" % (name, k, col), torch.from_numpy(part[:, nk == k, col].copy()),
                            _t64(d["part"][:, nk == k, col]), _t64(d["part_S"][:, nk == k, col]), n_part(d["B"], k, col)))
    return max(used)


def check_apply(name, d, coef, g_x):
    """C: g_x against the element-wise pass in float64 from the fp32 coefficients the apply kernel read."""
    coef = _is32(name + " coef", coef, (d["C"], 4))
    ref, S = R.apply_from_coef(d["x"], d["g"], d["out"], coef)
    return _rb(name + " g_x", torch.from_numpy(_is32(name + " g_x", g_x, ref.shape)), _t64(ref), _t64(S), N_APPLY)


def check_channel_sum(name, d, part, out):
    """dmh_channel_sum on the case's gradient: A (out is the double sum of the fp32 partials, in block order, cast once), B (dyadic:
    equal to the float64 sum bit for bit; in the vector form every partial too: its slab sets are the backward's) and C."""
    assert d["out"] is None
    part = _is32(name + " partials", part, (d["C"], d["S"])).astype(np.float64)
    acc = np.zeros(d["C"])
    for s in range(d["S"]):
        acc = acc + part[:, s]
    _equal(name + " out = float(sum of the partials)", out, acc)
    if d["exact"]:
        _equal(name + " out", out, d["g_bias"])
        if R.launch_form(d["HW"]) == "vector":
            _equal(name + " partials", part.astype(np.float32), d["part"][:, :, 0])
    return _rb(name + " out", torch.from_numpy(_np(out)), _t64(d["g_bias"]), _t64(d["part_S"][:, :, 0].sum(1)),
               n_channel_sum(d["B"], d["HW"]))


def _chan_err(got, ref, scale):
    """rel-L2 over the channels, every channel in units of its own scale."""
    return float(np.sqrt(np.mean(((np.asarray(got, np.float64) - ref) / scale) ** 2)))


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def stats_errors(d, r):
    """{line: error against float64} of one implementation's fp32 results ``r`` (the kernel's, or the library's)."""
    ref = d["ref"]
    spread = np.sqrt(ref["save_mean"] ** 2 + ref["var"])
    bias = np.zeros(d["C"]) if d["bias"] is None else d["bias"].astype(np.float64)
    e = {"save_mean": _chan_err(r["save_mean"], ref["save_mean"], spread),
         "running_mean": _chan_err(r["running_mean"], ref["running_mean"], spread),
         "save_invstd": _chan_err(r["save_invstd"], ref["save_invstd"], ref["save_invstd"]),
         "scale": _chan_err(r["scale"], ref["scale"], np.abs(ref["scale"])),
         "shift": _chan_err(r["shift"], ref["shift"], np.abs(bias) + np.abs(ref["save_mean"] * ref["scale"])),
         "running_var": _chan_err(r["running_var"], ref["running_var"], ref["running_var"])}
    if r.get("out") is not None:
        x = d["x"].astype(np.float64)
        e["out"] = _rel(r["out"], x * ref["scale"].reshape(1, -1, 1) + ref["shift"].reshape(1, -1, 1))
    return e


VARIANCE_TYPE = ("save_invstd", "scale", "shift", "running_var", "out")


def check_stats_fp64(name, d, got, lib):
    """D, statistics: every line under fp64_bound with chain = n_round and chain_margin = cond.  Returns [(line, e_hip, e_lib)]."""
    for k in ("save_mean", "save_invstd", "scale", "shift", "running_mean", "running_var"):
        _is32(name + " " + k, got[k], (d["C"],))
    e_hip, e_lib, n = stats_errors(d, got), stats_errors(d, lib), n_stats(d["B"], d["HW"])
    table, failed = [], []
    for k in e_hip:
        cond = d["cond"] if k in VARIANCE_TYPE else 1.0
        assert np.isfinite(e_hip[k]), (name, k)
        try:
            _bound("%s %s (n_round %d, cond %.1f)" % (name, k, n[k], cond), e_hip[k], e_lib[k], chain=n[k], chain_margin=cond)
        except AssertionError as e:
            failed.append(str(e))
        table.append((k, e_hip[k], e_lib[k]))
    assert not failed, failed
    return table


def check_invstd_consistency(name, d, save_invstd, running_var_m1):
    """D: save_invstd is within 4 ulp of rsqrt(running_var(momentum 1, zero buffers) * (n - 1) / n + eps) in float64: the biased and
    the unbiased variance come from one M2."""
    n = d["B"] * d["HW"]
    want = 1.0 / np.sqrt(_np(running_var_m1).astype(np.float64) * (n - 1) / n + EPS)
    got = _np(save_invstd)
    ulps = np.abs(got.astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
    print("%-52s worst distance %.2f ulp" % (name + " invstd vs running_var", float(ulps.max())))
    assert not (~(ulps <= 4.0)).any(), (name, float(ulps.max()))


def check_bwd_fp64(name, d, got, lib):
    """D, the whole backward: g_x, g_weight, g_bias against bwd() in float64 from the fp32 mean and invstd both were handed."""
    g_x, g_w, g_b, _ = R.bwd(d["x"], d["g"], d["out"], d["weight"], d["mean"], d["invstd"])
    n, table, failed = n_stats(d["B"], d["HW"]), [], []
    for k, ref in (("g_x", g_x), ("g_weight", g_w), ("g_bias", g_b)):
        _is32(name + " " + k, got[k], ref.shape)
        e_hip, e_lib = _rel(_np(got[k]), ref), _rel(_np(lib[k]), ref)
        assert np.isfinite(e_hip), (name, k)
        try:
            _bound("%s %s (n_round %d)" % (name, k, n[k]), e_hip, e_lib, chain=n[k])
        except AssertionError as e:
            failed.append(str(e))
        table.append((k, e_hip, e_lib))
    assert not failed, failed
    return table


# ---- launches -----------------------------------------------------------------------------------------------------------------------

def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


class _Out(object):
    """A NaN-filled fp32 output of the given shape with a NaN guard behind it."""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + GUARD,), float("nan"), device="cuda")
        self.t = self.buf[:self.n].view(*shape)

    def intact(self):
        return bool(torch.isnan(self.buf[self.n:]).all())


def _twice(launch):
    """Run a launch twice; the results must be bit-identical (compared as integers: NaN-safe).  Returns the first, on the CPU."""
    a, b = launch(), launch()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            bits = torch.int32 if u.dtype == torch.float32 else u.dtype
            assert torch.equal(u.detach().view(bits), v.detach().view(bits)), "a launch does not reproduce itself"
    return [None if u is None else u.detach().cpu() for u in a]


def run_stats(x, weight, bias, momentum, rm0, rv0, nbt0):
    """dmh_bn_train_stats_tracked, twice.  -> partials [C, S, 3], scale, shift, save_mean, save_invstd, running_mean, running_var,
    num_batches_tracked (the last three None where not handed)."""
    import ctypes
    from depthmodelhardening_amd import _native as N
    lib = N.lib()
    B, C, HW = x.shape
    S = R.slab_sets(HW)[0]
    n = lib.dmh_bn_stats_partials_size(B, C, HW)
    assert n == C * S * 3, (n, C, S)

    def launch():
        part, outs = _Out(C, S, 3), [_Out(C) for _ in range(4)]
        rm, rv = (None if t is None else _Out(C) for t in (rm0, rv0))
        if rm is not None:
            rm.t.copy_(rm0)
            rv.t.copy_(rv0)
        nbt = None if nbt0 is None else nbt0.clone()
        N.check(lib.dmh_bn_train_stats_tracked(
            N.ptr(x), B, C, HW, N.ptr(weight), N.ptr(bias), float(momentum), EPS, None if rm is None else N.ptr(rm.t),
            None if rv is None else N.ptr(rv.t), None if nbt is None else ctypes.c_void_p(nbt.data_ptr()), N.ptr(part.t),
            N.ptr(outs[0].t), N.ptr(outs[1].t), N.ptr(outs[2].t), N.ptr(outs[3].t), N.stream()))
        torch.cuda.synchronize()
        assert all(o.intact() for o in [part] + outs + [o for o in (rm, rv) if o is not None]), "a NaN guard was written"
        return [part.t] + [o.t for o in outs] + [None if rm is None else rm.t, None if rv is None else rv.t, nbt]
    return _twice(launch)


def run_bwd(x, g, out, weight, mean, invstd, want_pre, want_wb):
    """dmh_bn_train_bwd, twice.  -> coef [C, 4], partials [C, S, 2], g_x, g_weight, g_bias, g_pre."""
    from depthmodelhardening_amd import _native as N
    lib = N.lib()
    B, C, HW = x.shape
    S = R.slab_sets(HW)[0]
    n = lib.dmh_bn_train_bwd_workspace_size(B, C, HW)
    assert n == 4 * C + C * S * 2, (n, C, S)

    def launch():
        ws, gx = _Out(n), _Out(B, C, HW)
        gw, gb = (_Out(C) if want_wb else None for _ in range(2))
        gp = _Out(B, C, HW) if want_pre else None
        t = lambda o: None if o is None else N.ptr(o.t)      # noqa: E731
        N.check(lib.dmh_bn_train_bwd(N.ptr(x), N.ptr(g), N.ptr(out), N.ptr(weight), N.ptr(mean), N.ptr(invstd), B, C, HW, N.ptr(ws.t),
                                     N.ptr(gx.t), t(gw), t(gb), t(gp), N.stream()))
        torch.cuda.synchronize()
        assert all(o.intact() for o in (ws, gx, gw, gb, gp) if o is not None), "a NaN guard was written"
        assert not bool(torch.isnan(ws.t).any()), "a workspace entry was not written"
        return [ws.t[:4 * C].view(C, 4), ws.t[4 * C:].view(C, S, 2), gx.t] + [None if o is None else o.t for o in (gw, gb, gp)]
    return _twice(launch)


def run_channel_sum(g):
    """dmh_channel_sum, twice.  -> partials [C, S], out [C]."""
    from depthmodelhardening_amd import _native as N
    lib = N.lib()
    B, C, HW = g.shape
    S = R.slab_sets(HW)[0]
    assert lib.dmh_channel_sum_partials_size(B, C, HW) == C * S

    def launch():
        part, out = _Out(C, S), _Out(C)
        N.check(lib.dmh_channel_sum(N.ptr(g), B, C, HW, N.ptr(part.t), N.ptr(out.t), N.stream()))
        torch.cuda.synchronize()
        assert part.intact() and out.intact(), "a NaN guard was written"
        return part.t, out.t
    return _twice(launch)


# ---- the tests ----------------------------------------------------------------------------------------------------------------------

def test_case_list_reaches_the_forms_it_names():
    """Needs no GPU (tests/test_bn_train_ref.py runs it too)."""
    for case in CASES:
        assert case_form(*case[:2]) == case[2:], (case, case_form(*case[:2]))
    assert {c[2:4] for c in CASES} == {(f, S) for f in ("vector", "scalar") for S in (1, 2, 64)}
    totals = set()
    for B, HW, form in (c[:3] for c in CASES):
        if form == "vector":
            totals |= {B * len(r) for r in R.slab_sets(HW)[1]}
    assert 1 in totals and any(t % 2 for t in totals if t > 1) and any(t % 4 == 2 for t in totals) and any(t > 4 and t % 4 for t in totals)
    assert {R.launch_form(HW) for _, HW in D_CASES} == {"vector", "scalar"} and {R.launch_form(h * w) for h, w in E_SHAPES} == {
        "vector", "scalar"}
    assert all(h * w in {c[1] for c in CASES} for h, w in E_SHAPES) and all(HW in {c[1] for c in CASES} for _, HW in D_CASES)
    assert {m[:2] for m in BWD_MODES} == {(r, p) for r in (True, False) for p in (True, False)}


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_statistics_structure(case, data):
    """A on the statistics, C on the running mean; weight, bias, the running buffers and the counter NULL in turn."""
    d = stats_reference(case, data)
    assert case_form(*case[:2]) == case[2:]
    x = _dev(d["x"])
    first = None
    for (w, b, run, cnt) in STATS_MODES:
        name = "stats %s %s w%d b%d run%d cnt%d" % (_id(case), data, w, b, run, cnt)
        nbt0 = torch.tensor(41, dtype=torch.int64, device="cuda") if cnt else None
        weight, bias = _dev(d["weight"] if w else None), _dev(d["bias"] if b else None)
        part, scale, shift, mean, invstd, rm, rv, nbt = run_stats(x, weight, bias, MOMENTUM, _dev(d["rm0"]) if run else None,
                                                                  _dev(d["rv0"]) if run else None, nbt0)
        check_stats_partials(name, d, part)
        check_counter(name, 41, 41 if nbt is None else nbt, cnt)
        for t in (scale, shift, mean, invstd):
            assert bool(torch.isfinite(t).all()), name
        if run:
            check_running_mean(name, d, rm, mean)
            assert bool(torch.isfinite(rv).all()), name
        # the affine: scale = float(w * invstd), shift = float(b - mean * scale) up to the contraction of the last line
        assert torch.equal(scale, invstd * torch.from_numpy(np.array(d["weight"])) if w else invstd), name + ": scale is not weight * invstd"
        if first is None:
            first = (part, mean, invstd)
        else:       # the batch statistics do not depend on what else is handed
            assert all(torch.equal(u, v) for u, v in zip(first, (part, mean, invstd))), name


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_backward_structure(case, data):
    """A, B (dyadic) and C (partials, apply pass) on the backward, in all four <RELU, RES> instantiations."""
    assert case_form(*case[:2]) == case[2:]
    for mode in BWD_MODES:
        d = bwd_reference(case, data, mode)
        name = "bwd %s %s relu%d pre%d w%d wb%d" % ((_id(case), data) + tuple(int(m) for m in mode))
        coef, part, g_x, g_w, g_b, g_pre = run_bwd(_dev(d["x"]), _dev(d["g"]), _dev(d["out"]), _dev(d["weight"]), _dev(d["mean"]),
                                                   _dev(d["invstd"]), mode[1], mode[3])
        check_bwd_exact(name, d, coef, part, g_w, g_b, g_pre)
        if d["exact"]:
            check_bwd_dyadic(name, d, part, g_w, g_b)
        check_bwd_partials(name, d, part)
        check_apply(name, d, coef, g_x)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_channel_sum_structure(case, data):
    """The third reduction that deals slabs to blocks, on the backward's gradient (no mask: its sum is the reference's g_bias)."""
    d = bwd_reference(case, data, BWD_MODES[3])
    part, out = run_channel_sum(_dev(d["g"]))
    check_channel_sum("channel_sum %s %s" % (_id(case), data), d, part, out)


def _library_stats(x, weight, bias):
    """ATen's fp32 native_batch_norm on the device (no MIOpen: no kernel compilation for arithmetic of the same class)."""
    import torch.nn.functional as F
    C = x.shape[1]
    with torch.backends.cudnn.flags(enabled=False):
        rm, rv = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        out = F.batch_norm(x, rm, rv, weight, bias, True, 1.0, EPS)
        _, mean, invstd = torch.native_batch_norm(x, weight, bias, None, None, True, 1.0, EPS)
    scale = weight * invstd
    r = {"save_mean": mean, "save_invstd": invstd, "scale": scale, "shift": bias - mean * scale, "running_mean": rm, "running_var": rv,
         "out": out}
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("pivot", D_VARIANTS, ids=["drawn", "pivot8"])
@pytest.mark.parametrize("case", D_CASES, ids=_id)
def test_statistics_and_gradients_vs_fp64_and_library(case, pivot):
    """D.  The backward (whose kernels do not shift by the pivot) runs on the first variant only."""
    from depthmodelhardening_amd import _native as N
    d = d_reference(case, pivot)
    B, HW, C = d["B"], d["HW"], d["C"]
    name = "D %s %s" % (_id(case), "pivot 8 sigma" if pivot else "as drawn")
    x, weight, bias = _dev(d["x"]), _dev(d["weight"]), _dev(d["bias"])
    zeros = torch.zeros(C, device="cuda")
    part, scale, shift, mean, invstd, rm, rv, _ = run_stats(x, weight, bias, 1.0, zeros, zeros, None)

    def normalise():
        out = _Out(B, C, HW)
        N.check(N.lib().dmh_bn_act_fwd(N.ptr(x), N.ptr(scale_d), N.ptr(shift_d), None, B, C, HW, 0, N.ptr(out.t), N.stream()))
        torch.cuda.synchronize()
        assert out.intact()
        return (out.t,)
    scale_d, shift_d = scale.cuda(), shift.cuda()
    got = {"save_mean": mean, "save_invstd": invstd, "scale": scale, "shift": shift, "running_mean": rm, "running_var": rv,
           "out": _twice(normalise)[0]}
    got = {k: v.numpy() for k, v in got.items()}
    print("%s: cond %.1f" % (name, d["cond"]))
    check_stats_fp64(name, d, got, _library_stats(x, weight, bias))
    check_invstd_consistency(name, d, invstd, rv)
    if pivot is not None:
        return
    g, out, m32, i32 = _dev(d["g"]), _dev(d["out"]), _dev(d["mean"]), _dev(d["invstd"])
    _, _, g_x, g_w, g_b, g_pre = run_bwd(x, g, out, weight, m32, i32, True, True)
    g_masked = torch.where(out > 0, g, torch.zeros_like(g))
    assert torch.equal(g_pre, g_masked.cpu())
    lx, lw, lb = torch.ops.aten.native_batch_norm_backward(g_masked.view(B, C, HW, 1), x.view(B, C, HW, 1), weight, None, None, m32, i32,
                                                           True, EPS, [True, True, True])
    check_bwd_fp64(name, d, {"g_x": g_x.numpy(), "g_weight": g_w.numpy(), "g_bias": g_b.numpy()},
                   {"g_x": lx.reshape(B, C, HW).cpu().numpy(), "g_weight": lw.cpu().numpy(), "g_bias": lb.cpu().numpy()})


def _err_t(a, ref64, unit=None):
    """rel-L2 against a float64 tensor on the device; with ``unit``: over the channels, each in units of its own scale."""
    diff = a.detach().double() - ref64
    return float((diff / unit).pow(2).mean().sqrt()) if unit is not None else float(diff.norm() / ref64.norm())


def _hold_e(name, hip, lib, ref, n, cond, unit=None):
    assert bool(torch.isfinite(hip).all()), name
    _bound("%s (n_round %d, cond %.1f)" % (name, n, cond), _err_t(hip, ref, unit), _err_t(lib, ref, unit), chain=n, factor=2.0,
           chain_margin=cond)


@pytest.mark.parametrize("shape", E_SHAPES, ids=lambda s: "%dx%d" % s)
def test_train_nodes_vs_fp64_module(shape):
    """E: ops.bn_act_train over relu x residual (none, constant, requiring grad) x affine on / off, and
    ops.stem_bn_relu_pool_train, against nn.BatchNorm2d in float64; the library is the same module in fp32.  Without the affine the
    backward leaves the fused kernel for ATen's: the gradients must still be right."""
    import torch.nn as nn
    import torch.nn.functional as F
    from depthmodelhardening_amd import ops
    H, W = shape
    B, C, HW = 3, C_STAT, H * W
    rng = _rng("E", shape)
    x = torch.from_numpy(R.generic((B, C, H, W), rng, "x")).cuda()
    res = torch.from_numpy(R.generic((B, C, H, W), rng, "grad")).cuda()
    g = torch.from_numpy(R.generic((B, C, H, W), rng, "grad")).cuda()
    gp = torch.from_numpy(R.generic((B, C, H // 2, W // 2), rng, "grad")).cuda()
    wt, bs = (torch.from_numpy(R.generic((C,), rng, k)).cuda() for k in ("weight", "bias"))
    mean, var = R.stats(x.cpu().numpy())[:2]
    cond = float(1.0 + ((x[0, :, 0, 0].double().cpu().numpy() - mean) ** 2 / var).max())
    n = n_stats(B, HW)
    n_out, n_grad = n["out"] + 1, n["save_invstd"] + n["g_x"]          # (+ 1: the residual add)

    def module(affine, dtype):
        bn = nn.BatchNorm2d(C, affine=affine).cuda().train()
        if affine:
            with torch.no_grad():
                bn.weight.copy_(wt)
                bn.bias.copy_(bs)
        return bn.to(dtype)

    def leaves(dtype, res_mode):
        xs = x.to(dtype).requires_grad_(True)
        rs = None if res_mode is None else res.to(dtype).requires_grad_(res_mode == "grad")
        return xs, rs

    def grads(outs, gouts, bn, xs, rs):
        ins = [xs] + ([rs] if rs is not None and rs.requires_grad else []) + list(bn.parameters())
        gr = torch.autograd.grad(outs, ins, gouts)
        names = ["g_x"] + (["g_res"] if rs is not None and rs.requires_grad else []) + (["g_weight", "g_bias"] if bn.affine else [])
        return dict(zip(names, gr))

    def hold_all(name, hip, lib, ref):
        # the two buffers per channel in units of the quantity's scale, as in rule D (an average near 0 is no scale: the spread,
        # times the momentum it entered the zero buffer with)
        units = {"running_mean": torch.from_numpy(np.sqrt(mean ** 2 + var) * MOMENTUM).cuda(), "running_var": ref["running_var"]}
        rounds = {"out": n_out, "feat": n_out, "pooled": n_out, "running_mean": n["running_mean"], "running_var": n["running_var"]}
        for k in hip:
            c = cond if k in ("out", "feat", "pooled", "g_x", "g_weight", "running_var") else 1.0
            _hold_e("%s %s" % (name, k), hip[k], lib[k], ref[k], rounds.get(k, n_grad), c, units.get(k))

    with torch.backends.cudnn.flags(enabled=False):
        for affine in (True, False):
            for relu in (True, False):
                for res_mode in (None, "const", "grad"):
                    name = "E %dx%d affine%d relu%d res-%s" % (H, W, affine, relu, res_mode)
                    runs = []
                    for _ in range(2):
                        bn = module(affine, torch.float32)
                        xs, rs = leaves(torch.float32, res_mode)
                        out = ops.bn_act_train(bn, xs, residual=rs, relu=relu)
                        r = dict(grads([out], [g], bn, xs, rs), out=out.detach(), running_mean=bn.running_mean.clone(),
                                 running_var=bn.running_var.clone())
                        assert int(bn.num_batches_tracked) == 1
                        runs.append(r)
                    assert all(torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)) for k in runs[0]), name
                    hip = runs[0]
                    mask = (hip["out"] > 0) if relu else None
                    both = []
                    for dtype in (torch.float32, torch.float64):
                        bn = module(affine, dtype)
                        xs, rs = leaves(dtype, res_mode)
                        y = bn(xs) if rs is None else bn(xs) + rs
                        if relu:        # float64: the HIP forward's own mask; the library: its own ReLU
                            y = y * mask.to(dtype) if dtype == torch.float64 else F.relu(y)
                        both.append(dict(grads([y], [g.to(dtype)], bn, xs, rs), out=y.detach(), running_mean=bn.running_mean.clone(),
                                         running_var=bn.running_var.clone()))
                    assert set(both[0]) == set(hip) and set(both[1]) == set(hip), name
                    hold_all(name, hip, both[0], both[1])
        if HW % 4:
            return          # the stem's pool needs even H and W: a vector plane
        for affine in (True, False):
            name = "E %dx%d stem affine%d" % (H, W, affine)
            runs = []
            for _ in range(2):
                bn = module(affine, torch.float32)
                xs, _ = leaves(torch.float32, None)
                feat, pooled = ops.stem_bn_relu_pool_train(bn, xs)
                runs.append(dict(grads([feat, pooled], [g, gp], bn, xs, None), feat=feat.detach(), pooled=pooled.detach(),
                                 running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone()))
            assert all(torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)) for k in runs[0]), name
            hip = runs[0]
            mask = hip["feat"] > 0
            both = []
            for dtype in (torch.float32, torch.float64):
                bn = module(affine, dtype)
                xs, _ = leaves(dtype, None)
                feat = bn(xs) * mask.to(dtype) if dtype == torch.float64 else F.relu(bn(xs))
                pooled = F.max_pool2d(feat, 3, 2, 1)
                both.append(dict(grads([feat, pooled], [g.to(dtype), gp.to(dtype)], bn, xs, None), feat=feat.detach(),
                                 pooled=pooled.detach(), running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone()))
            hold_all(name, hip, both[0], both[1])
