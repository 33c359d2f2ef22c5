"""tests/glue_ref.py -- the float64 reference of K7 and K9's eval forms -- against torch's float64 operators and autograd on the CPU,
and the checks of tests/test_gpu_glue_anchor.py against seeded faults: they pass the reference itself (cast to fp32) at every GPU
case and flag each of the index mistakes such kernels can have, at the GPU test's own shapes.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import glue_ref as R
from tests import test_gpu_glue_anchor as A

TOL = 1e-14


def _close(name, got, want):
    want = want.detach().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= TOL * max(1.0, float(np.abs(want).max()) if want.size else 0.0), (name, err)


def _t(a, grad=False):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64)).requires_grad_(grad)


def _ch(v):
    return _t(v).view(1, -1, 1, 1)


# ---- the reference against torch float64 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", A.UP_CASES, ids=A._id)
def test_up_cat_pad_reference_vs_torch(case):
    d = A.up_reference(case, "generic")
    y, skip = _t(d["y"], True), _t(d["skip"], True)
    t = F.interpolate(F.elu(y), scale_factor=2, mode="nearest")
    out = F.pad(t if skip is None else torch.cat([t, skip], 1), (1, 1, 1, 1), mode="reflect")
    _close("forward", d["out"], out)
    g = torch.autograd.grad(out, [y] + ([skip] if skip is not None else []), _t(d["g"]))
    g_y, g_skip, S_y, S_skip = R.up_cat_pad_bwd(d["y"], d["g"], True)
    _close("g_y", g_y, g[0])
    assert (g_skip is None) == (skip is None)
    if skip is not None:
        _close("g_skip", g_skip, g[1])
        assert (S_skip >= np.abs(g_skip)).all()
    assert (S_y >= np.abs(g_y)).all()
    if not d["skip_grad"]:
        assert d["g_skip"] is None and d["S_skip"] is None


@pytest.mark.parametrize("apply_elu", [0, 1])
@pytest.mark.parametrize("case", A.PAD_CASES, ids=A._id)
def test_elu_pad_reference_vs_torch(case, apply_elu):
    d = A.pad_reference(case, apply_elu, "generic")
    z = _t(d["z"], True)
    out = F.pad(F.elu(z) if apply_elu else z, (1, 1, 1, 1), mode="reflect")
    _close("forward", d["out"], out)
    _close("g_z", d["g_z"], torch.autograd.grad(out, z, _t(d["g"]))[0])
    assert (d["S"] >= np.abs(d["g_z"])).all()


@pytest.mark.parametrize("mode", A.BN_MODES, ids=lambda m: "relu%d-res%s" % (m[0], m[1]))
@pytest.mark.parametrize("case", A.BN_CASES, ids=A._id)
def test_bn_act_reference_vs_torch(case, mode):
    d = A.bn_reference(case, mode, "generic")
    x, res = _t(d["x"], True), _t(d["res"], True)
    pre = x * _ch(d["scale"]) + _ch(d["shift"])
    pre = pre if res is None else pre + res
    out = F.relu(pre) if d["relu"] else pre
    _close("forward", d["out"], out)
    g = torch.autograd.grad(out, [x] + ([res] if res is not None else []), _t(d["g"]))
    _close("g_x", d["g_x"], g[0])
    if res is not None:
        _close("g_res", d["g_res"], g[1])


def _window_code(idx, H, W):
    """max_pool2d's flat plane index -> ky * 3 + kx of the unclipped window of its pooled cell."""
    PH, PW = H // 2, W // 2
    i, j = np.arange(PH)[:, None], np.arange(PW)[None, :]
    yy, xx = idx // W, idx % W
    ky, kx = yy - (2 * i - 1), xx - (2 * j - 1)
    assert ((ky >= 0) & (ky < 3) & (kx >= 0) & (kx < 3)).all()
    return (ky * 3 + kx).astype(np.uint8)


@pytest.mark.parametrize("case", A.STEM_CASES, ids=A._id)
def test_stem_reference_vs_torch(case):
    """Generic data only: ATen's choice among exact ties is not part of its contract.  Windows of zeros (every candidate clamped)
    tie even here, so the argmax is compared where the maximum is positive -- unique on this data, which the empty excluded set
    asserts -- and the gradient through a zero maximum is masked whichever candidate carries it."""
    (H, W), _ = case
    d = A.stem_reference(case, "generic")
    x = _t(d["x"], True)
    feat = F.relu(x * _ch(d["scale"]) + _ch(d["shift"]))
    pooled, idx = F.max_pool2d(feat, 3, 2, 1, return_indices=True)
    _close("feat", d["feat"], feat)
    _close("pooled", d["pooled"], pooled)
    A.assert_nothing_excluded("stem", d, A.N_STEM_FWD, pool=True)
    live = d["pooled"] > 0
    assert live.any() and np.array_equal(_window_code(idx.numpy(), H, W)[live], d["arg"][live])
    assert d["arg"].max() <= 8
    for gf, gp in A.STEM_GRADS:
        cost = (feat * _t(d["g_feat"])).sum() * float(gf) + (pooled * _t(d["g_pool"])).sum() * float(gp)
        _close("g_x %d %d" % (gf, gp), d["g_x", gf, gp], torch.autograd.grad(cost, x, retain_graph=True)[0])
        assert (d["S", gf, gp] >= np.abs(d["g_x", gf, gp])).all()


def test_first_maximum_wins_in_the_reference():
    """The definition, on a plane built by hand: equal positive values, and a window of zeros."""
    x = np.zeros((1, 1, 4, 4), np.float32)
    x[0, 0, 1, 1] = x[0, 0, 1, 2] = x[0, 0, 2, 1] = 3.0         # window (1, 1) covers rows 1..3, columns 1..3
    one, zero = np.ones(1, np.float32), np.zeros(1, np.float32)
    feat, pooled, arg = R.stem(x, one, zero)
    assert arg[0, 0].tolist() == [[8, 6], [2, 0]] and pooled[0, 0].tolist() == [[3.0, 3.0], [3.0, 3.0]]
    feat, pooled, arg = R.stem(-np.abs(x) - 1, one, zero)       # every candidate clamps to zero: the first in-image position
    assert arg[0, 0].tolist() == [[4, 3], [1, 0]] and not pooled.any()
    _, _, last = R.stem(x, one, zero, better=np.greater_equal)
    assert last[0, 0].tolist() == [[8, 7], [5, 3]]


def test_input_generators_are_what_they_claim():
    rng = np.random.RandomState(0)
    v, g, s = R.dyadic((4000,), rng), R.dyadic((4000,), rng, "grad"), R.dyadic((64,), rng, "scale")
    assert np.array_equal(v * 16, np.round(v * 16)) and v.min() == -4 and v.max() == 4 and (v == 0).any()
    assert np.array_equal(g * 16, np.round(g * 16)) and g.min() == -2 and g.max() == 2
    assert set(s.tolist()) == set(R.DYADIC_SCALES)
    for C in (1, 3):
        for k in range(50):
            assert (R.dyadic((C,), rng, "scale") < 0).any() and (R.generic((C,), rng, "scale") < 0).any()
    s = R.generic((1000,), rng, "scale")
    assert (np.abs(s) >= 0.3).all() and (np.abs(s) <= 1.5).all() and (s > 0).any()
    assert np.abs(R.generic((1000,), rng, "shift")).max() <= 0.5


# ---- exact adjoint identities on dyadic data ------------------------------------------------------------------------------------------

def _dot(a, b):
    return float((np.asarray(a, np.float64) * np.asarray(b, np.float64)).sum())


@pytest.mark.parametrize("case", A.PAD_CASES, ids=A._id)
def test_pad_only_operator_and_its_adjoint_exactly(case):
    d = A.pad_reference(case, 0, "dyadic")
    assert _dot(d["out"], d["g"]) == _dot(d["z"], d["g_z"])


@pytest.mark.parametrize("case", [c for c in A.UP_CASES if c[0][2] and c[1]], ids=A._id)
def test_skip_branch_and_its_adjoint_exactly(case):
    d = A.up_reference(case, "dyadic")
    C1 = d["C1"]
    assert _dot(d["out"][:, C1:], d["g"][:, C1:]) == _dot(d["skip"], d["g_skip"])


# ---- the GPU cases' input conditions --------------------------------------------------------------------------------------------

def test_case_lists_reach_the_forms_they_name():
    A.test_case_lists_reach_the_forms_they_name()


def test_generic_seeds_leave_the_excluded_sets_empty():
    for case in A.BN_CASES:
        for mode in A.BN_MODES:
            if mode[0]:
                d = A.bn_reference(case, mode, "generic")
                A.assert_nothing_excluded("bn_act %s %s" % (case, mode), d, A.N_BN_FWD if d["res"] is None else A.N_BN_FWD_RES)
    for case in A.STEM_CASES:
        d = A.stem_reference(case, "generic")
        A.assert_nothing_excluded("stem %s" % (case,), d, A.N_STEM_FWD, pool=True)
        assert (d["feat"] > 0).any() and (d["feat"] == 0).any()


def test_dyadic_stem_cases_tie_at_positive_maxima():
    """What the coarse grid is for: in the dyadic cases many windows hold their positive maximum twice, and the other tie rule would
    route a live gradient elsewhere."""
    tied = 0
    for case in A.STEM_CASES:
        d = A.stem_reference(case, "dyadic")
        _, _, last = R.stem(d["x"], d["scale"], d["shift"], better=np.greater_equal)
        tied += int(((last != d["arg"]) & (d["pooled"] > 0)).sum())
    assert tied >= 100, tied


# ---- sensitivity: the checks of the GPU file against seeded faults ----------------------------------------------------------------

def _f32(a):
    return None if a is None else torch.from_numpy(np.asarray(a).astype(np.float32))


def _flags(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _differs(a, b):
    """Beyond a different order of float64 additions."""
    return bool((np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) > 1e-9).any())


def _clean(d, kind):
    if kind == "up":
        A.check_up_forward("clean", d, _f32(d["out"]))
        A.check_up_backward("clean", d, _f32(d["g_y"]), _f32(d["g_skip"]))
    elif kind == "pad":
        A.check_pad_forward("clean", d, _f32(d["out"]))
        A.check_pad_backward("clean", d, _f32(d["g_z"]))
    elif kind == "bn":
        A.check_bn_forward("clean", d, _f32(d["out"]))
        A.check_bn_backward("clean", d, _f32(d["g_x"]), _f32(d["g_res"]) if d["res_grad"] else None)
    else:
        A.check_stem_forward("clean", d, _f32(d["feat"]), _f32(d["pooled"]), torch.from_numpy(d["arg"].copy()))
        for gf, gp in A.STEM_GRADS:
            A.check_stem_backward("clean", d, _f32(d["g_x", gf, gp]), gf, gp)


def test_checks_pass_the_reference_rounded_to_fp32():
    """Not vacuous the other way round: at every GPU case, both kinds of data, the float64 result cast to fp32 passes."""
    for data in A.DATA:
        for case in A.UP_CASES:
            _clean(A.up_reference(case, data), "up")
        for case in A.PAD_CASES:
            for e in (0, 1):
                _clean(A.pad_reference(case, e, data), "pad")
        for case in A.BN_CASES:
            for mode in A.BN_MODES:
                _clean(A.bn_reference(case, mode, data), "bn")
        for case in A.STEM_CASES:
            _clean(A.stem_reference(case, data), "stem")
    _clean(A.up_reference(A.UP_ONES, "dyadic", True), "up")
    _clean(A.pad_reference(A.PAD_ONES, 1, "dyadic", True), "pad")
    _clean(A.bn_reference(A.BN_ONES, (True, "grad"), "dyadic", True), "bn")
    _clean(A.stem_reference(A.STEM_ONES, "dyadic", True), "stem")


def _fold(g, bottom=2):
    """The reflection pad's adjoint the way the kernels write it -- a gather: padded rows 0 / H + 1 are added onto interior rows
    1 / H - 2, then padded columns 0 / W + 1 onto interior columns 1 / W - 2.  ``bottom`` = 1 seeds the fault "row H + 1 onto row
    H - 1"."""
    g = np.asarray(g, np.float64)
    H, W = g.shape[-2] - 2, g.shape[-1] - 2
    t = g[..., 1:-1, :].copy()
    t[..., 1, :] += g[..., 0, :]
    t[..., H - bottom, :] += g[..., H + 1, :]
    o = t[..., 1:-1].copy()
    o[..., 1] += t[..., 0]
    o[..., W - 2] += t[..., W + 1]
    return o


def _report(name, found, altered):
    print("%s: flagged at %d of the %d cases it alters" % (name, len(found), altered))
    assert found, name + ": flagged nowhere"


def test_fold_formulation_equals_the_scatter_and_a_misplaced_bottom_row_is_flagged():
    found, altered = [], 0
    for data in A.DATA:
        for case in A.PAD_CASES:
            for e in (0, 1):
                d = A.pad_reference(case, e, data)
                dz = R.elu_grad(d["z"]) if e else 1.0
                _close("fold == scatter", _fold(d["g"]) * dz, d["g_z"])
                bad = _fold(d["g"], bottom=1) * dz
                assert _differs(bad, d["g_z"])
                altered += 1
                if _flags(A.check_pad_backward, "row H+1 onto H-1", d, _f32(bad)):
                    found.append(("elu_pad", case, e, data))
        for case in A.UP_CASES:
            d = A.up_reference(case, data)
            C1 = d["C1"]
            _close("fold == scatter", R.up2_nearest_adjoint(_fold(d["g"])[:, :C1]) * R.elu_grad(d["y"]), d["g_y"])
            t = _fold(d["g"], bottom=1)
            g_y = R.up2_nearest_adjoint(t[:, :C1]) * R.elu_grad(d["y"])
            # the y branch sums rows 2i and 2i + 1 into one source row: a fold moved from row H - 2 to row H - 1 stays inside it, and
            # only a skip gradient shows the fault
            assert not _differs(g_y, d["g_y"])
            if not d["skip_grad"]:
                continue
            assert _differs(t[:, C1:], d["g_skip"])
            altered += 1
            if _flags(A.check_up_backward, "row H+1 onto H-1", d, _f32(g_y), _f32(t[:, C1:])):
                found.append(("up_cat_pad", case, data))
    _report("fold onto row H - 1", found, altered)
    assert len(found) == altered


def test_left_column_reflected_from_column_0_is_flagged():
    found, altered = [], 0
    for data in A.DATA:
        for case in A.PAD_CASES:
            for e in (0, 1):
                d = A.pad_reference(case, e, data)
                bad = d["out"].copy()
                bad[..., 0] = bad[..., 1]           # padded column 1 is interior column 0
                altered += 1
                if _flags(A.check_pad_forward, "left column", d, _f32(bad)):
                    found.append(("elu_pad", case, e, data))
        for case in A.UP_CASES:
            d = A.up_reference(case, data)
            bad = d["out"].copy()
            bad[..., 0] = bad[..., 1]
            assert not _differs(bad[:, :d["C1"]], d["out"][:, :d["C1"]])      # up-sampled columns 0 and 1 are copies of each other
            if not case[0][2]:
                continue                            # so only skip planes show the fault
            altered += 1
            if _flags(A.check_up_forward, "left column", d, _f32(bad)):
                found.append(("up_cat_pad", case, data))
    _report("left column from column 0", found, altered)
    assert len(found) == altered


def test_last_maximum_tie_rule_is_flagged():
    found, altered = [], 0
    for data in A.DATA:
        for case in A.STEM_CASES:
            d = A.stem_reference(case, data)
            feat, pooled, arg = R.stem(d["x"], d["scale"], d["shift"], better=np.greater_equal)
            if np.array_equal(arg, d["arg"]):
                continue
            altered += 1
            assert np.array_equal(pooled, d["pooled"])
            if _flags(A.check_stem_forward, "tie rule", d, _f32(feat), _f32(pooled), torch.from_numpy(arg)):
                found.append((case, data, "argmax"))
            g_x, _ = R.stem_bwd(d["feat"], arg, d["g_feat"], d["g_pool"], d["scale"])
            if _differs(g_x, d["g_x", True, True]) and _flags(A.check_stem_backward, "tie rule", d, _f32(g_x), True, True):
                found.append((case, data, "g_x"))
    _report("last maximum wins (argmax bytes)", [f for f in found if f[2] == "argmax"], altered)
    assert len([f for f in found if f[2] == "argmax"]) == altered
    assert any(f[1] == "dyadic" and f[2] == "g_x" for f in found)       # on dyadic data the rule moves live gradients


def test_channel_index_without_the_modulo_is_flagged():
    """c = i / hw instead of (i / hw) % C: images after the first read past the end of scale / shift (emulated as zeros)."""
    found, altered = [], 0
    for data in A.DATA:
        for case in A.BN_CASES:
            B, C = case[0][:2]
            if B < 2:
                continue
            for mode in A.BN_MODES:
                d = A.bn_reference(case, mode, data)
                x = d["x"].reshape(1, B * C, *case[0][2:])
                res = None if d["res"] is None else d["res"].reshape(x.shape)
                pad = np.zeros((B - 1) * C, np.float32)
                sc, sh = np.concatenate([d["scale"], pad]), np.concatenate([d["shift"], pad])
                out = R.bn_act(x, sc, sh, res, d["relu"])
                g_x, g_res = R.bn_act_bwd(d["out"].reshape(x.shape), d["g"].reshape(x.shape), sc, d["relu"])
                altered += 1
                hit = _flags(A.check_bn_forward, "no % C", d, _f32(out.reshape(d["out"].shape)))
                hit_b = _flags(A.check_bn_backward, "no % C", d, _f32(g_x.reshape(d["out"].shape)),
                               _f32(g_res.reshape(d["out"].shape)) if d["res_grad"] else None)
                assert hit and hit_b, (case, mode, data)
                found.append((case, mode, data))
    _report("channel index without % C", found, altered)
    assert any(f[0][0][0] == 2 for f in found)


def test_elu_of_the_neighbouring_column_is_flagged():
    found, altered = [], 0
    for data in A.DATA:
        for case in A.UP_CASES:
            d = A.up_reference(case, data)
            C1, h, w = d["C1"], case[0][3], case[0][4]
            e = R.elu(d["y"])
            cols = np.minimum((np.arange(2 * w) + 1) // 2, w - 1)
            bad = d["out"].copy()
            bad[:, :C1] = R.pad1_reflect(e[..., (np.arange(2 * h) // 2)[:, None], cols[None, :]])
            if not _differs(bad, d["out"]):
                assert w == 1
                continue
            altered += 1
            if _flags(A.check_up_forward, "column shift", d, _f32(bad)):
                found.append((case, data))
    _report("ELU of the neighbouring column", found, altered)
    assert len(found) == altered


def test_transposed_argmax_decoding_is_flagged():
    found, altered = [], 0
    for data in A.DATA:
        for case in A.STEM_CASES:
            d = A.stem_reference(case, data)
            for gf in (True, False):
                g_x, _ = R.stem_bwd(d["feat"], d["arg"], d["g_feat"] if gf else None, d["g_pool"], d["scale"],
                                    decode=lambda a: (a % 3, a // 3))
                if not _differs(g_x, d["g_x", gf, True]):
                    continue
                altered += 1
                if _flags(A.check_stem_backward, "kx * 3 + ky", d, _f32(g_x), gf, True):
                    found.append((case, data, gf))
    _report("argmax decoded as kx * 3 + ky", found, altered)
    assert len(found) == altered
    assert {f[0] for f in found} >= {c for c in A.STEM_CASES if c[0] != (2, 2)}
