"""tests/bn_train_ref.py -- the float64 reference of K9's train forms -- against torch's float64 operators and autograd on the CPU, the
input conditions the GPU cases rely on, and the checks of tests/test_gpu_bn_train_anchor.py against the reference rounded to fp32
(which must pass) and against seeded faults (each of which must be flagged), at the GPU test's own shapes.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import bn_train_ref as R
from tests import test_gpu_bn_train_anchor as A

TOL = 1e-12
D_SMALL = [c for c in A.D_CASES if c[1] <= 1030]


def _close(name, got, want, tol=TOL):
    want = want.detach().numpy() if torch.is_tensor(want) else np.asarray(want)
    got = np.asarray(got)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= tol * max(1.0, float(np.abs(want).max()) if want.size else 0.0), (name, err)


def _t(a, grad=False):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64)).requires_grad_(grad)


# ---- the deal of slabs ----------------------------------------------------------------------------------------------------------------

def test_slab_sets_partition_the_plane_and_agree_with_the_closed_form():
    sizes = sorted({c[1] for c in A.CASES} | {1023, 1024, 1025, 2048, 65535, 65536, 65537, 66560, 81920, 131071, 131073, 200000})
    for HW in sizes:
        S, sets = R.slab_sets(HW)
        nslab = -(-HW // R.SLAB)
        assert S == min(R.S_CAP, nslab) and len(sets) == S
        seen = np.zeros(HW, np.int64)
        for s, ranges in enumerate(sets):
            assert len(ranges) == R.slabs_of(HW, s, S), (HW, s)
            for j, (lo, hi) in enumerate(ranges):
                assert lo == (s + j * S) * R.SLAB and lo < hi <= HW and hi - lo <= R.SLAB
                seen[lo:hi] += 1
        assert (seen == 1).all(), HW
        assert all(R.slabs_of(HW, s, S + 3) == 0 for s in range(nslab, nslab + 3))
    S, pairs = R.block_pairs(3, 66564)
    assert [len(p) for p in pairs] == [6, 6] + [3] * 62 and pairs[0][:3] == [(0, 0, 1024), (0, 65536, 66560), (1, 0, 1024)]
    assert pairs[1][1] == (0, 66560, 66564) and R.partial_counts(3, 66564).sum() == 3 * 66564


def test_case_list_reaches_the_forms_it_names():
    A.test_case_list_reaches_the_forms_it_names()


# ---- the reference against torch float64 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("relu,res", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("case", [c for c in A.CASES if c[0] * c[1] > 1], ids=A._id)
def test_reference_vs_torch(case, relu, res):
    """F.batch_norm(training=True) under autograd, with ReLU and a residual; nn.BatchNorm2d's running-statistics update."""
    B, HW = case[:2]
    rng = A._rng("torch", case, relu, res)
    d = A._inputs(B, 3, HW, "generic", rng)
    r = R.generic((B, 3, HW), rng, "grad") if res else None
    x, w, b, rt = _t(d["x"], True), _t(d["weight"], True), _t(d["bias"], True), _t(r, True)
    y = F.batch_norm(x, None, None, w, b, True, 0.1, A.EPS)
    y = y if rt is None else y + rt
    out = F.relu(y) if relu else y
    mean, var, invstd, scale, shift, unbiased = R.stats(d["x"], d["weight"], d["bias"], A.EPS)
    _close("mean", mean, x.detach().mean((0, 2)))
    _close("var", var, x.detach().var((0, 2), unbiased=False))
    _close("unbiased", unbiased, x.detach().var((0, 2), unbiased=True))
    _close("invstd", invstd, (x.detach().var((0, 2), unbiased=False) + A.EPS).rsqrt())
    pre = d["x"].astype(np.float64) * scale.reshape(1, -1, 1) + shift.reshape(1, -1, 1) + (0.0 if r is None else r)
    _close("forward", np.maximum(pre, 0.0) if relu else pre, out, 1e-11)
    bn = nn.BatchNorm2d(3, eps=A.EPS, momentum=0.1).double().train()
    rm0, rv0 = rng.uniform(-1, 1, 3), rng.uniform(0.5, 2, 3)
    with torch.no_grad():
        bn.running_mean.copy_(_t(rm0))
        bn.running_var.copy_(_t(rv0))
        bn(x.detach().view(B, 3, HW, 1))
    rm, rv = R.running_update(rm0, rv0, mean, unbiased, 0.1)
    _close("running_mean", rm, bn.running_mean)
    _close("running_var", rv, bn.running_var)
    g = torch.autograd.grad(out, [x, w, b] + ([rt] if res else []), _t(d["g"]))
    o = out.detach().numpy() if relu else None
    g_x, g_w, g_b, g_pre = R.bwd(d["x"], d["g"], o, d["weight"], mean, invstd)
    scale_g = 1e-9 * max(1.0, float(invstd.max()) ** 2)
    _close("g_x", g_x, g[0], scale_g)
    _close("g_weight", g_w, g[1], scale_g)
    _close("g_bias", g_b, g[2])
    if res:
        _close("g_pre", g_pre, g[3])
    sums = R.bwd_sums(d["x"], d["g"], o, mean)
    _close("partials add up to g_bias", sums[:, :, 0].sum(1), g_b)
    _close("partials add up to g_weight", sums[:, :, 1].sum(1) * invstd, g_w, scale_g)
    n = B * HW
    coef = np.stack([d["weight"] * invstd, g_b / n, g_w * invstd / n, mean], 1)
    ax, S = R.apply_from_coef(d["x"], d["g"], o, coef)
    _close("apply_from_coef", ax, g_x, scale_g)
    assert (S >= np.abs(ax) * (1 - 1e-12)).all()
    assert (R.bwd_sums(d["x"], d["g"], o, mean, absolute=True) >= np.abs(sums) * (1 - 1e-12)).all()
    g_x1, g_w1, _, _ = R.bwd(d["x"], d["g"], o, None, mean, invstd)         # weight = NULL is weight = 1
    _close("g_x without weight", g_x1 * d["weight"].astype(np.float64).reshape(1, -1, 1), g_x, scale_g)
    _close("g_weight without weight", g_w1, g_w)


# ---- the input conditions -------------------------------------------------------------------------------------------------------------

def test_input_generators_are_what_they_claim():
    rng = np.random.RandomState(0)
    g, m, o = R.dyadic((4000,), rng, "grad"), R.dyadic((64,), rng, "mean"), R.dyadic((2, 3, 2000), rng, "out")
    assert set(g.tolist()) == {-1.0, -0.5, 0.0, 0.5, 1.0}
    assert np.array_equal(m * 4, np.round(m * 4)) and np.abs(m).max() <= 2
    x = R.dyadic((2, 64, 100), rng, "x", m)
    xc = x.astype(np.float64) - m.astype(np.float64).reshape(1, -1, 1)
    assert np.array_equal(xc * 4, np.round(xc * 4)) and xc.min() == -2 and xc.max() == 2
    assert set(np.log2(R.dyadic((200,), rng, "invstd")).tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    wt = R.dyadic((200,), rng, "weight")
    assert set(np.abs(wt).tolist()) == {0.5, 1.0, 2.0} and (wt < 0).any() and (wt > 0).any()
    assert 0.4 < (o == 0).mean() < 0.6 and o.min() == 0 and np.array_equal(o * 4, np.round(o * 4))
    x = R.generic((64, 64, 400), rng, "x").astype(np.float64)
    sigma, mean = x.std((0, 2)), x.mean((0, 2))
    assert 0.09 < sigma.min() < 0.2 and 5 < sigma.max() < 11 and np.abs(mean / sigma).max() < 4.1 and np.abs(mean / sigma).max() > 3
    for case in D_SMALL[2:]:
        for pivot, lo, hi in ((None, 1.0, 30.0), (8.0, 50.0, 80.0)):      # 1 + 8^2 = 65 up to the sampling noise of mean and sigma
            d = A.d_reference(case, pivot)
            assert lo <= d["cond"] <= hi, (case, pivot, d["cond"])
    assert 0.4 < (R.generic((10000,), rng, "out") > 0).mean() < 0.6


@pytest.mark.parametrize("case", A.CASES, ids=A._id)
def test_dyadic_sums_are_exact_in_fp32(case):
    """The premise of check B: a SEQUENTIAL fp32 sum of the generated terms equals their float64 sum, per block and in total (so
    does every other order: all partial sums are multiples of 1/8 below 2^21)."""
    B, HW = case[:2]
    _, pairs = R.block_pairs(B, HW)
    for mode in A.BWD_MODES[:1] + A.BWD_MODES[3:]:
        d = A.bwd_reference(case, "dyadic", mode)
        gp = R.masked(d["g"], d["out"])
        t = gp * (d["x"].astype(np.float64) - d["mean"].astype(np.float64).reshape(1, -1, 1))
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t) and np.array_equal(t * 8, np.round(t * 8))
        for col, terms in enumerate((gp, t)):
            for c in range(d["C"]):
                for s, p in enumerate(pairs):
                    v = np.concatenate([terms[b, c, lo:hi] for (b, lo, hi) in p])
                    assert float(np.cumsum(v.astype(np.float32), dtype=np.float32)[-1]) == d["part"][c, s, col] == v.sum()
                v = terms[:, c].ravel()
                assert float(np.cumsum(v.astype(np.float32), dtype=np.float32)[-1]) == v.sum() == d["part"][c, :, col].sum()
        assert np.abs(d["part_S"]).max() * 8 < 2 ** 21
        assert np.array_equal(d["g_weight"].astype(np.float32).astype(np.float64), d["g_weight"])


# ---- what a correct fp32 implementation would hand the checks ---------------------------------------------------------------------

def _f32(a):
    return None if a is None else torch.from_numpy(np.asarray(a).astype(np.float32))


def _finalize(d, part32):
    """bn_bwd_finalize_kernel restated: double sums of the fp32 partials in block order, one cast.  -> coef, g_weight, g_bias."""
    p = np.asarray(part32, np.float32).astype(np.float64)
    s1, s2 = np.zeros(d["C"]), np.zeros(d["C"])
    for s in range(d["S"]):
        s1, s2 = s1 + p[:, s, 0], s2 + p[:, s, 1]
    isd = d["invstd"].astype(np.float64)
    w = np.ones(d["C"]) if d["weight"] is None else d["weight"].astype(np.float64)
    inv_n = 1.0 / (float(d["B"]) * float(d["HW"]))
    coef = np.stack([w * isd, s1 * inv_n, s2 * isd * isd * inv_n, d["mean"].astype(np.float64)], 1).astype(np.float32)
    return coef, (s2 * isd).astype(np.float32), s1.astype(np.float32)


def _bwd_outputs(d, pairs=None, mask_from=None, unmasked_pre=False, coef_shift=0):
    """The backward's six outputs as fp32 arithmetic would leave them, from the float64 reference -- or with a seeded fault."""
    relu, want_pre, _, want_wb = d["mode"]
    out = d["out"] if mask_from is None else mask_from
    part = _f32(R.bwd_sums(d["x"], d["g"], out, d["mean"], pairs=pairs))
    coef, g_w, g_b = _finalize(d, part.numpy())
    g_x, _ = R.apply_from_coef(d["x"], d["g"], out, np.roll(coef, -coef_shift, axis=0))
    g_pre = d["g"] if (out is None or unmasked_pre) else R.masked(d["g"], out)
    return (torch.from_numpy(coef), part, _f32(g_x), _f32(g_w) if want_wb else None, _f32(g_b) if want_wb else None,
            _f32(g_pre.reshape(d["g"].shape)) if want_pre else None)


def _run_bwd_checks(name, d, outs):
    coef, part, g_x, g_w, g_b, g_pre = outs
    A.check_bwd_exact(name, d, coef, part, g_w, g_b, g_pre)
    if d["exact"]:
        A.check_bwd_dyadic(name, d, part, g_w, g_b)
    A.check_bwd_partials(name, d, part)
    A.check_apply(name, d, coef, g_x)


def _stats_outputs(d, **fault):
    """Rule D's quantities rounded to fp32 from the float64 reference, or with a seeded fault."""
    ref = dict(d["ref"])
    if fault.get("pairs") is not None:
        mean, var, invstd, scale, shift, unbiased = R.stats(d["x"], d["weight"], d["bias"], A.EPS, pairs=fault["pairs"])
        ref.update(save_mean=mean, save_invstd=invstd, scale=scale, shift=shift, running_mean=mean, running_var=unbiased)
    if fault.get("biased_running_var"):
        ref["running_var"] = ref["var"]
    if fault.get("eps_outside"):
        ref["save_invstd"] = 1.0 / (np.sqrt(ref["var"]) + A.EPS)
        ref["scale"] = d["weight"] * ref["save_invstd"]
        ref["shift"] = d["bias"] - ref["save_mean"] * ref["scale"]
    r = {k: np.asarray(ref[k]).astype(np.float32) for k in ("save_mean", "save_invstd", "scale", "shift", "running_mean", "running_var")}
    r["out"] = (d["x"].astype(np.float64) * ref["scale"].reshape(1, -1, 1) + ref["shift"].reshape(1, -1, 1)).astype(np.float32)
    return r


def _flags(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _report(name, found, altered):
    print("%s: flagged at %d of the %d cases it alters" % (name, len(found), altered))
    assert found, name + ": flagged nowhere"


def test_checks_pass_the_reference_rounded_to_fp32():
    """Not vacuous the other way round: at every GPU case, both kinds of data, every mode."""
    for data in A.DATA:
        for case in A.CASES:
            d = A.stats_reference(case, data)
            part = np.zeros((d["C"], d["S"], 3), np.float32)
            part[:, :, 0] = d["counts"]
            A.check_stats_partials("clean", d, part)
            A.check_counter("clean", 41, 42, True)
            A.check_counter("clean", 41, 41, False)
            mean32 = R.stats(d["x"])[0].astype(np.float32)
            A.check_running_mean("clean", d, _f32(R.running_update(d["rm0"], 0.0, mean32, 0.0, A.MOMENTUM)[0]), mean32)
            for mode in A.BWD_MODES:
                d = A.bwd_reference(case, data, mode)
                _run_bwd_checks("clean", d, _bwd_outputs(d))
            part = _f32(d["part"][:, :, 0])         # (relu off in the last mode: the plain sum of g)
            A.check_channel_sum("clean", d, part, _f32(part.double().sum(1)))


@pytest.mark.parametrize("pivot", A.D_VARIANTS, ids=["drawn", "pivot8"])
@pytest.mark.parametrize("case", A.D_CASES, ids=A._id)
def test_rule_d_passes_the_reference_rounded_to_fp32(case, pivot):
    d = A.d_reference(case, pivot)
    r = _stats_outputs(d)
    A.check_stats_fp64("clean", d, r, r)
    A.check_invstd_consistency("clean", d, r["save_invstd"], r["running_var"])
    if pivot is None:
        g_x, g_w, g_b, _ = R.bwd(d["x"], d["g"], d["out"], d["weight"], d["mean"], d["invstd"])
        r = {"g_x": g_x.astype(np.float32), "g_weight": g_w.astype(np.float32), "g_bias": g_b.astype(np.float32)}
        A.check_bwd_fp64("clean", d, r, r)


# ---- sensitivity: seeded faults -------------------------------------------------------------------------------------------------------

def _drop(pairs):
    """One slab lost: the last (image, slab) pair of block 0."""
    return [pairs[0][:-1]] + [list(p) for p in pairs[1:]]


def _double(pairs):
    """One slab counted twice: the last pair of the last block."""
    return [list(p) for p in pairs[:-1]] + [pairs[-1] + pairs[-1][-1:]]


def _no_tail(step):
    """The clamped tail of the flattened (image, slab) loop dropped: steps of ``step`` pairs, the incomplete last step lost."""
    return lambda pairs: [p[:len(p) - len(p) % step] for p in pairs]


SLAB_FAULTS = [("one slab dropped", _drop, _drop), ("one slab counted twice", _double, _double),
               ("tail pair / quad dropped", _no_tail(2), _no_tail(4))]


@pytest.mark.parametrize("fault", SLAB_FAULTS, ids=lambda f: f[0].replace(" ", "-"))
def test_lost_and_doubled_slabs_are_flagged(fault):
    label, bwd_fault, stats_fault = fault
    found, altered, found_n, altered_n = [], 0, [], 0
    for case in A.CASES:
        B, HW = case[:2]
        _, pairs = R.block_pairs(B, HW)
        bad = stats_fault(pairs)
        if bad != pairs:            # the statistics: the n of the partials (the tail fault needs the vector form's flattened loop)
            if not (label.startswith("tail") and case[2] == "scalar"):
                d = A.stats_reference(case, "generic")
                part = np.zeros((d["C"], d["S"], 3), np.float32)
                part[:, :, 0] = R.partial_counts(B, HW, bad)
                altered_n += 1
                if _flags(A.check_stats_partials, label, d, part):
                    found_n.append(case)
        bad = bwd_fault(pairs)
        if bad == pairs or (label.startswith("tail") and case[2] == "scalar"):
            continue
        for data in A.DATA:
            for mode in A.BWD_MODES[:2]:
                d = A.bwd_reference(case, data, mode)
                outs = _bwd_outputs(d, pairs=bad)
                if not (outs[1].double().numpy() != d["part"].astype(np.float32)).any():
                    continue        # (a lost slab of zeros)
                altered += 1
                if _flags(_run_bwd_checks, label, d, outs):
                    found.append((case, data, mode))
            d = A.bwd_reference(case, data, A.BWD_MODES[3])
            part = _f32(R.bwd_sums(d["x"], d["g"], None, d["mean"], pairs=bad)[:, :, 0])
            assert (part.double().numpy() == d["part"][:, :, 0].astype(np.float32)).all() or _flags(
                A.check_channel_sum, label, d, part, _f32(part.double().sum(1))), (label, case, data, "channel_sum")
    _report(label + " (backward sums)", found, altered)
    _report(label + " (statistics, n)", found_n, altered_n)
    assert len(found) == altered and len(found_n) == altered_n
    assert any(c[0][1] >= 66563 for c in found) and any(c[1] >= 66563 for c in found_n)
    # and through rule D: the statistics of a plane with that fault
    d = A.d_reference((3, 1030), None)
    _, pairs = R.block_pairs(3, 1030)
    bad = [q for p in _no_tail(2)(pairs) for q in p] if label.startswith("tail") else [q for p in stats_fault(pairs) for q in p]
    good = _stats_outputs(d)
    assert _flags(A.check_stats_fp64, label, d, _stats_outputs(d, pairs=bad), good), label + ": rule D does not see it"


def test_wrong_running_updates_are_flagged():
    found = []
    for case in D_SMALL:
        d = A.d_reference(case, None)
        good = _stats_outputs(d)
        assert _flags(A.check_stats_fp64, "n for n - 1", d, _stats_outputs(d, biased_running_var=True), good), case
        found.append(case)
    _report("n for n - 1 in the running variance", found, len(D_SMALL))
    found = []
    for case in A.CASES:
        d = A.stats_reference(case, "generic")
        mean32 = R.stats(d["x"])[0].astype(np.float32)
        swapped = _f32(A.MOMENTUM * d["rm0"].astype(np.float64) + (1 - A.MOMENTUM) * mean32.astype(np.float64))
        assert _flags(A.check_running_mean, "momentum on the old value", d, swapped, mean32), case
        found.append(case)
    _report("momentum applied to the wrong operand", found, len(A.CASES))


def test_eps_outside_the_square_root_is_flagged():
    found = []
    for case in A.D_CASES[:6]:
        d = A.d_reference(case, None)
        if _flags(A.check_stats_fp64, "eps outside", d, _stats_outputs(d, eps_outside=True), _stats_outputs(d)):
            found.append(case)
    _report("1 / (sqrt(var) + eps)", found, 6)
    assert len(found) == 6


def test_wrong_channel_mask_and_g_pre_are_flagged():
    ch, mask, pre = [], [], []
    n_ch = n_mask = n_pre = 0
    for case in A.CASES:
        for data in A.DATA:
            for mode in A.BWD_MODES:
                d = A.bwd_reference(case, data, mode)
                n_ch += 1
                if _flags(_run_bwd_checks, "coef of channel c + 1", d, _bwd_outputs(d, coef_shift=1)):
                    ch.append((case, data, mode))
                if not mode[0]:
                    continue
                n_mask += 1
                if _flags(_run_bwd_checks, "mask from g", d, _bwd_outputs(d, mask_from=d["g"])):
                    mask.append((case, data, mode))
                if mode[1]:
                    n_pre += 1
                    if _flags(_run_bwd_checks, "g_pre unmasked", d, _bwd_outputs(d, unmasked_pre=True)):
                        pre.append((case, data, mode))
    _report("the coefficient of channel c + 1", ch, n_ch)
    _report("the mask taken from g instead of out", mask, n_mask)
    _report("g_pre unmasked", pre, n_pre)
    assert len(ch) == n_ch and len(mask) == n_mask
    # (g_pre unmasked: invisible only where every masked element holds g = 0 -- the one-element planes)
    assert {c[0] for c in pre} >= {c for c in A.CASES if c[1] >= 63}
    assert {c[0][2] for c in ch} == {"vector", "scalar"}
