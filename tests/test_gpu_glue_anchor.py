"""Float64 anchors of K7 (csrc/decoder_glue.hip: up_cat_pad, elu_pad) and of K9's eval forms (csrc/encoder_glue.hip: bn_act, stem),
forward and backward, in every launch form, against tests/glue_ref.py (plain numpy float64, the adjoints by SCATTER where the
kernels gather; tests/test_glue_ref.py holds that reference to torch's float64 operators, feeds the checks of this file seeded
faults, and checks the input conditions of the generic cases on the CPU).

Launch forms, from the host code of the two .hip files -- the case lists below are written against these rules, every case asserts
the form it is meant to reach, and a change of a rule makes the lists visibly stale:

    up_cat_pad   (w & 1) == 0          four-wide (up_cat_pad_fwd4 / bwd4_kernel), else pair (up_cat_pad_fwd / bwd_kernel<true>)
    elu_pad      (W & 3) == 0          four-wide (elu_pad_fwd4 / bwd4_kernel); else (W & 1) == 0: pair (<true>); else scalar (<false>)
    bn_act       (HW & 3) == 0         vector (bn_act_fwd / bwd_vec), else scalar; <RELU, RES> from relu / residual (backward: RES from
                                       "the residual requires grad")
    stem         (W & 3) == 0          backward stem_bwd4_kernel, else stem_bwd_kernel (pair); the forward has one form

Two kinds of input (tests/glue_ref.py).  ``dyadic``: every product and sum is exact in fp32, so the kernel must equal the float64
reference cast to fp32 BIT FOR BIT wherever no expf is involved -- an off-by-one on one border row cannot hide in a tolerance --
and positive values tie exactly in many pooling windows, so the tie rule decides live gradients.  ``generic``: normal data, held
element by element to

        |got - ref64|  <=  n_round * 2^-24 * S                              (tests/util.py: assert_round_bound)

with S from the float64 reference and n_round READ FROM THE KERNEL (constants below), no outlier share, no additive slack.  A copy
(a skip plane, a pad-only plane, ELU of a positive number, g_res) is torch.equal on both kinds of input.

ELU forward on x <= 0: |got - expm1(x)| <= 2 * 2^-24, absolute.  expf(x) lies in (0, 1], where one ulp is at most 2^-24 (EXPF_ULP
= 1, measured over every fp32 argument of [-20, 0]: DESIGN.md, K19); "expf(x) - 1.f" is exact for expf(x) >= 0.5 (Sterbenz) and
rounds by at most half an ulp of a number in (-1, -0.5), 2^-25, below that: less than 2 * 2^-24 together.

Masks and argmax on generic data: the float64 reference decides them.  An element whose float64 pre-activation lies within the
forward bound of 0 could take either side of the ReLU in fp32; a window whose two largest candidates (at different positions, the
larger one positive) lie within twice the forward bound of each other could take either argmax.  Such elements would have to be
excluded; instead the seeds are such that there are NONE, and that is asserted (here and, for the same seeds, on the CPU).  A
window whose candidates are all zero is no such window: with no pre-activation near 0 every candidate is exactly 0.0 in fp32 as
well, and the tie rule of the definition (first position wins) decides both -- that rule is part of what is tested.

Every launch runs twice and must reproduce itself bit for bit.  Outputs handed to the C ABI are pre-filled with NaN (argmax: 255)."""
import zlib

import numpy as np
import pytest
import torch

from tests import glue_ref as R
from tests.util import U32, assert_round_bound as _rb

pytestmark = pytest.mark.gpu

# ---- n_round, in units of 2^-24 (one ulp of a result is two of them), read from the kernels ---------------------------------------
EXPF_ULP = 1                # tests/test_gpu_roi_anchor.py, DESIGN.md K19: 0.857 ulp measured, rounded up
# up_cat_pad, y branch.  Pair form: fold2d adds <= 2 x 2 entries onto 0.f (H, W even: a row is 1 or H - 2, never both, unless H = 2,
# where row 0 takes only H + 1 and row 1 only 0): 3 rounded additions; the four children's folds are summed: + 3; "acc *
# elu_grad(y)": + 1 for the product, + 2 EXPF_ULP for the expf inside.  Four-wide form: row_quad 1, the second row 1, "r0.x + r0.y
# + r1.x + r1.y" 3: fewer.  6 + 2 + 1.
N_UP_Y = 6 + 2 * EXPF_ULP + 1
# up_cat_pad, skip branch: the same fold of <= 2 x 2 entries and nothing else -- no product, no expf: 3, not the 3 + 3 of elu_pad.
N_UP_SKIP = 3
# elu_pad.  H and W are free here: for H = 3 row 1 is both "Y == 1" and "Y == H - 2" (three rows meet), for W = 3 likewise (the
# scalar form), so fold2d adds up to 3 x 3 entries onto 0.f: 8 rounded additions, not 3 (at this file's shapes at most 3 x 2 = 6
# entries, 5 additions; the count is the kernel's, not the shapes').  With ELU + 1 product + 2 EXPF_ULP.
N_PAD = 8
N_PAD_ELU = N_PAD + 2 * EXPF_ULP + 1
N_BN_FWD, N_BN_FWD_RES = 1, 2       # fmaf(x, s, b): one rounding; "+= res": one more.  ReLU is exact.
N_BN_BWD = 1                        # g * scale[c]; g_res is a masked copy (torch.equal)
N_STEM_FWD = 1                      # relu(fmaf(x, s, b)); the maximum is exact
# stem backward: a pixel in an odd row and column is a candidate of four windows: up to four g_pool are added onto 0.f (the first
# exactly: 3 rounded additions), "+= g_feat": 1 -- 4 additions; "* s": 1 product.
N_STEM_BWD = 4 + 1
ELU_FWD_ABS = 2 * U32


def up_form(h, w):
    return "four-wide" if (w & 1) == 0 else "pair"


def pad_form(H, W):
    return "four-wide" if (W & 3) == 0 else ("pair" if (W & 1) == 0 else "scalar")


def bn_form(H, W):
    return "vector" if ((H * W) & 3) == 0 else "scalar"


def stem_form(H, W):
    return "bwd4" if (W & 3) == 0 else "pair"


# ---- cases: the smallest shapes at which each form and edge exists ----------------------------------------------------------------
# ((B, C1, C2, h, w), skip requires grad, form)
UP_CASES = [
    ((1, 2, 1, 1, 2), True, "four-wide"),       # H = 2, W = 4: one quad is first and last of its row, rows 0 and 1 both take a fold
    ((2, 3, 2, 3, 4), True, "four-wide"),
    ((2, 3, 2, 9, 66), True, "four-wide"),      # blocks per plane: 2 (y part, 297 threads), 3 (skip part, 594): ragged last blocks
    ((1, 2, 0, 4, 6), True, "four-wide"),       # skip = None
    ((2, 2, 3, 5, 8), False, "four-wide"),      # g_skip = NULL with C2 > 0
    ((2, 3, 2, 1, 1), True, "pair"),            # W = 2: columns 0 and 1 both take a fold
    ((1, 2, 1, 5, 3), True, "pair"),
    ((2, 1, 2, 9, 33), True, "pair"),           # several blocks per plane in both parts
    ((1, 2, 0, 3, 5), True, "pair"),            # skip = None
    ((2, 1, 2, 3, 7), False, "pair"),           # g_skip = NULL with C2 > 0
]
UP_ONES = ((2, 3, 2, 3, 4), True, "four-wide")
# ((H, W), form), B, C = 2, 3, apply_elu 0 and 1
PAD_CASES = [
    ((2, 4), "four-wide"), ((3, 8), "four-wide"), ((9, 260), "four-wide"),      # (3, 8): row 1 is both Y == 1 and Y == H - 2
    ((2, 2), "pair"), ((5, 6), "pair"), ((17, 66), "pair"),
    ((2, 3), "scalar"), ((4, 5), "scalar"), ((7, 37), "scalar"),
]
PAD_ONES = ((5, 6), "pair")
# ((B, C, H, W), form); (relu, residual) in all four combinations, the residual with and without requires_grad
BN_CASES = [
    ((1, 1, 1, 1), "scalar"), ((2, 5, 3, 4), "vector"), ((3, 7, 3, 5), "scalar"), ((2, 3, 20, 52), "vector"), ((2, 3, 7, 37), "scalar"),
]
BN_MODES = [(relu, res) for relu in (True, False) for res in (None, "grad", "nograd")]
BN_ONES = ((2, 5, 3, 4), "vector")
# ((H, W), backward form), B, C = 2, 3
STEM_CASES = [
    ((2, 2), "pair"), ((2, 4), "bwd4"), ((4, 6), "pair"), ((10, 2), "pair"), ((6, 8), "bwd4"), ((34, 38), "pair"), ((36, 64), "bwd4"),
]
STEM_GRADS = [(True, True), (True, False), (False, True)]       # (g_feat, g_pool) present
STEM_ONES = ((6, 8), "bwd4")
DATA = ("dyadic", "generic")

# generic-data seeds are offset by this; bump an entry if a case ever lands an element in the excluded set (never happened: the
# chance is ~1e-7 per element)
SEED_BUMP = {}


def _rng(*key):
    return np.random.RandomState((zlib.crc32(repr(key).encode()) + SEED_BUMP.get(key, 0)) % (2 ** 31))


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


# ---- references: inputs and float64 results of a case, computed once, shared read-only --------------------------------------------

@_cached
def up_reference(case, data, ones=False):
    (B, C1, C2, h, w), skip_grad, form = case
    rng, gen = _rng("up", case, data), getattr(R, data)
    d = {"y": gen((B, C1, h, w), rng), "skip": gen((B, C2, 2 * h, 2 * w), rng) if C2 else None,
         "g": np.ones((B, C1 + C2, 2 * h + 2, 2 * w + 2), np.float32) if ones else gen((B, C1 + C2, 2 * h + 2, 2 * w + 2), rng, "grad"),
         "ones": ones, "skip_grad": bool(skip_grad and C2), "C1": C1, "exact": data == "dyadic"}
    d["out"] = R.up_cat_pad(d["y"], d["skip"])
    d["g_y"], d["g_skip"], d["S_y"], d["S_skip"] = R.up_cat_pad_bwd(d["y"], d["g"], d["skip_grad"])
    return d


@_cached
def pad_reference(case, apply_elu, data, ones=False):
    (H, W), form = case
    rng, gen = _rng("pad", case, apply_elu, data), getattr(R, data)
    d = {"z": gen((2, 3, H, W), rng), "g": np.ones((2, 3, H + 2, W + 2), np.float32) if ones else gen((2, 3, H + 2, W + 2), rng, "grad"),
         "ones": ones, "apply_elu": apply_elu, "exact": data == "dyadic"}
    d["out"] = R.elu_pad(d["z"], apply_elu)
    d["g_z"], d["S"] = R.elu_pad_bwd(d["z"], d["g"], apply_elu)
    return d


@_cached
def bn_reference(case, mode, data, ones=False):
    shape, form = case
    relu, res = mode
    rng, gen = _rng("bn", case, mode, data), getattr(R, data)
    C = shape[1]
    d = {"x": gen(shape, rng), "scale": gen((C,), rng, "scale"), "shift": gen((C,), rng, "shift"),
         "res": gen(shape, rng) if res else None, "g": np.ones(shape, np.float32) if ones else gen(shape, rng, "grad"),
         "ones": ones, "relu": relu, "res_grad": res == "grad", "exact": data == "dyadic"}
    d["pre"] = R.affine(d["x"], d["scale"], d["shift"], d["res"])
    d["S_fwd"] = R.affine_S(d["x"], d["scale"], d["shift"], d["res"])
    d["out"] = R.bn_act(d["x"], d["scale"], d["shift"], d["res"], relu)
    d["g_x"], d["g_res"] = R.bn_act_bwd(d["out"], d["g"], d["scale"], relu)
    return d


@_cached
def stem_reference(case, data, ones=False):
    (H, W), form = case
    rng, gen = _rng("stem", case, data), getattr(R, data)
    d = {"x": gen((2, 3, H, W), rng), "scale": gen((3,), rng, "scale"), "shift": gen((3,), rng, "shift"),
         "g_feat": np.ones((2, 3, H, W), np.float32) if ones else gen((2, 3, H, W), rng, "grad"),
         "g_pool": np.ones((2, 3, H // 2, W // 2), np.float32) if ones else gen((2, 3, H // 2, W // 2), rng, "grad"),
         "ones": ones, "exact": data == "dyadic"}
    assert (d["scale"] < 0).sum() >= 1
    d["pre"] = R.affine(d["x"], d["scale"], d["shift"])
    d["S_fwd"] = R.affine_S(d["x"], d["scale"], d["shift"])
    d["feat"], d["pooled"], d["arg"] = R.stem(d["x"], d["scale"], d["shift"])
    for gf, gp in STEM_GRADS:
        d["g_x", gf, gp], d["S", gf, gp] = R.stem_bwd(d["feat"], d["arg"], d["g_feat"] if gf else None, d["g_pool"] if gp else None,
                                                     d["scale"])
    return d


# ---- the excluded sets (generic data): must be empty ------------------------------------------------------------------------------

def relu_excluded(d, n_round):
    """Elements whose float64 pre-activation lies within the forward bound of 0."""
    return np.abs(d["pre"]) <= n_round * U32 * d["S_fwd"]


def pool_windows(a, fill):
    """[B, C, H, W] -> [B, C, H / 2, W / 2, 9]: the 3 x 3 / 2 windows with padding 1, ``fill`` outside the image."""
    B, C, H, W = a.shape
    p = np.full((B, C, H + 2, W + 2), fill, np.float64)
    p[:, :, 1:-1, 1:-1] = a
    return np.stack([p[:, :, ky:ky + H:2, kx:kx + W:2] for ky in range(3) for kx in range(3)], -1)


def argmax_excluded(d):
    """Windows whose two largest candidates (two positions; the larger one positive) lie within twice the forward bound of each other."""
    cand = pool_windows(d["feat"], -np.inf)
    bound = pool_windows(N_STEM_FWD * U32 * d["S_fwd"], 0.0)
    order = np.argsort(-cand, axis=-1, kind="stable")
    v = np.take_along_axis(cand, order[..., :2], -1)
    b = np.take_along_axis(bound, order[..., :2], -1)
    assert np.array_equal(v[..., 0], d["pooled"])               # (the two formulations of the maximum agree)
    return (v[..., 0] > 0) & (v[..., 0] - v[..., 1] <= 2 * b.max(-1))


def assert_nothing_excluded(name, d, n_round, pool=False):
    if d["exact"]:
        return      # dyadic: fp32 arithmetic is exact, so masks and argmax are the float64 ones by construction
    ex = relu_excluded(d, n_round)
    assert not ex.any(), "%s: %d pre-activations within the forward bound of 0 -- choose another seed (SEED_BUMP)" % (name, ex.sum())
    if pool:
        ex = argmax_excluded(d)
        assert not ex.any(), "%s: %d windows with two candidates within twice the forward bound -- choose another seed" % (name, ex.sum())


# ---- checks: ``got`` are fp32 CPU tensors, from the GPU here and from seeded faults in tests/test_glue_ref.py ---------------------

def _t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _t32(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32))


def _equal(name, got, want64, where=None):
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want64.shape), (name, got.dtype, got.shape, want64.shape)
    want = _t32(want64)
    if where is not None:
        where = torch.from_numpy(np.array(where))
        got, want = got[where], want[where]
    assert torch.equal(got, want), "%s: %d of %d elements differ from the float64 reference cast to fp32" % (
        name, int((got != want).sum()), got.numel())


def check_elu_forward(name, got, want64):
    """An ELU plane: a copy (torch.equal) where the value is positive, within 2 * 2^-24 of expm1 elsewhere.  Returns the worst
    share of that bound."""
    _equal(name + " (x > 0: a copy)", got, want64, want64 > 0)
    neg = torch.from_numpy(np.array(want64 <= 0))
    err = (got.double() - _t64(want64)).abs()[neg]
    used = float(torch.nan_to_num(err, nan=float("inf")).max() / ELU_FWD_ABS) if err.numel() else 0.0
    print("%-52s ELU(x <= 0): worst |got - expm1(x)| / (2 * 2^-24) %.3f" % (name, used))
    assert not bool((~(err <= ELU_FWD_ABS)).any()), "%s: %d ELU values beyond 2 * 2^-24 of expm1 (worst share %.3g)" % (
        name, int((~(err <= ELU_FWD_ABS)).sum()), used)
    return used


def check_up_forward(name, d, out):
    C1 = d["C1"]
    used = check_elu_forward(name + " y planes", out[:, :C1], d["out"][:, :C1])
    _equal(name + " skip planes", out[:, C1:], d["out"][:, C1:])
    return used


def check_up_backward(name, d, g_y, g_skip):
    if d["exact"]:
        _equal(name + " g_y (y > 0: no expf)", g_y, d["g_y"], d["y"] > 0)
    used = [_rb(name + " g_y", g_y, _t64(d["g_y"]), _t64(d["S_y"]), N_UP_Y)]
    assert (g_skip is None) == (d["g_skip"] is None), name + ": g_skip present / absent"
    if g_skip is not None:
        if d["exact"]:
            _equal(name + " g_skip", g_skip, d["g_skip"])
        used.append(_rb(name + " g_skip", g_skip, _t64(d["g_skip"]), _t64(d["S_skip"]), N_UP_SKIP))
    return max(used)


def check_pad_forward(name, d, out):
    if d["apply_elu"]:
        return check_elu_forward(name, out, d["out"])
    _equal(name + " (pad only: a copy)", out, d["out"])
    return 0.0


def check_pad_backward(name, d, g_z):
    if d["exact"]:
        _equal(name + " g_z (no expf)", g_z, d["g_z"], (d["z"] > 0) if d["apply_elu"] else None)
    return _rb(name + " g_z", g_z, _t64(d["g_z"]), _t64(d["S"]), N_PAD_ELU if d["apply_elu"] else N_PAD)


def check_bn_forward(name, d, out):
    if d["exact"]:
        _equal(name + " out", out, d["out"])
    return _rb(name + " out", out, _t64(d["out"]), _t64(d["S_fwd"]), N_BN_FWD if d["res"] is None else N_BN_FWD_RES)


def check_bn_backward(name, d, g_x, g_res):
    if d["relu"]:
        assert_nothing_excluded(name, d, N_BN_FWD if d["res"] is None else N_BN_FWD_RES)
    assert (g_res is None) == (not d["res_grad"]), name + ": g_res present / absent"
    if g_res is not None:
        _equal(name + " g_res (a masked copy)", g_res, d["g_res"])
    if d["exact"]:
        _equal(name + " g_x", g_x, d["g_x"])
    return _rb(name + " g_x", g_x, _t64(d["g_x"]), _t64(np.abs(d["g_x"])), N_BN_BWD)


def check_stem_forward(name, d, feat, pooled, arg):
    assert_nothing_excluded(name, d, N_STEM_FWD, pool=True)
    assert arg.dtype == torch.uint8 and tuple(arg.shape) == d["arg"].shape
    bad = arg != torch.from_numpy(np.array(d["arg"]))
    assert not bool(bad.any()), "%s: %d of %d argmax bytes differ (first-maximum rule, ky * 3 + kx of the unclipped window)" % (
        name, int(bad.sum()), bad.numel())
    if d["exact"]:
        _equal(name + " feat", feat, d["feat"])
        _equal(name + " pooled", pooled, d["pooled"])
    S_pool = np.take_along_axis(pool_windows(d["S_fwd"], 0.0), d["arg"][..., None].astype(np.int64), -1)[..., 0]
    return max(_rb(name + " feat", feat, _t64(d["feat"]), _t64(d["S_fwd"]), N_STEM_FWD),
               _rb(name + " pooled", pooled, _t64(d["pooled"]), _t64(S_pool), N_STEM_FWD))


def check_stem_backward(name, d, g_x, gf, gp):
    if d["exact"]:
        _equal(name + " g_x", g_x, d["g_x", gf, gp])
    return _rb(name + " g_x", g_x, _t64(d["g_x", gf, gp]), _t64(d["S", gf, gp]), N_STEM_BWD)


# ---- launches ---------------------------------------------------------------------------------------------------------------------

def _dev(a, grad=False):
    return None if a is None else torch.from_numpy(np.array(a)).cuda().requires_grad_(grad)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


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


def _grads(out, inputs, d):
    """Gradients of the op's output: for an explicit g_out, or of out.sum() -- an expanded, stride-0 incoming gradient."""
    if d["ones"]:
        return torch.autograd.grad(out.sum(), inputs)
    return torch.autograd.grad(out, inputs, _dev(d["g"]))


def run_up(d):
    from depthmodelhardening_amd import ops

    def launch():
        y, skip = _dev(d["y"], True), _dev(d["skip"], d["skip_grad"])
        out = ops.up_cat_pad(y, skip)
        g = _grads(out, [y] + ([skip] if d["skip_grad"] else []), d)
        return out, g[0], (g[1] if d["skip_grad"] else None)
    return _twice(launch)


def run_pad(d):
    from depthmodelhardening_amd import ops

    def launch():
        z = _dev(d["z"], True)
        out = ops.elu_pad(z, d["apply_elu"])
        return out, _grads(out, [z], d)[0]
    return _twice(launch)


def run_bn(d):
    from depthmodelhardening_amd import ops

    def launch():
        x, res = _dev(d["x"], True), _dev(d["res"], d["res_grad"])
        out = ops.bn_act(x, _dev(d["scale"]), _dev(d["shift"]), res, d["relu"])
        g = _grads(out, [x] + ([res] if d["res_grad"] else []), d)
        return out, g[0], (g[1] if d["res_grad"] else None)
    return _twice(launch)


def run_stem_forward(d):
    from depthmodelhardening_amd import _native as N
    x, sc, sh = _dev(d["x"]), _dev(d["scale"]), _dev(d["shift"])
    B, C, H, W = x.shape

    def launch():
        feat, pooled = _nan(B, C, H, W), _nan(B, C, H // 2, W // 2)
        arg = torch.full((B, C, H // 2, W // 2), 255, dtype=torch.uint8, device="cuda")
        N.check(N.lib().dmh_stem_bn_relu_pool_fwd(N.ptr(x), N.ptr(sc), N.ptr(sh), B, C, H, W, N.ptr(feat), N.ptr(pooled), N.ptr(arg),
                                                  N.stream()))
        return feat, pooled, arg
    return _twice(launch)


def run_stem_backward(d, gf, gp):
    """From the REFERENCE's feat (cast to fp32) and argmax, not the forward kernel's: the two directions are held separately."""
    from depthmodelhardening_amd import _native as N
    feat, arg, sc = _dev(d["feat"].astype(np.float32)), _dev(d["arg"]), _dev(d["scale"])
    g_feat, g_pool = _dev(d["g_feat"] if gf else None), _dev(d["g_pool"] if gp else None)
    B, C, H, W = feat.shape

    def launch():
        g_x = _nan(B, C, H, W)
        N.check(N.lib().dmh_stem_bn_relu_pool_bwd(N.ptr(feat), N.ptr(arg), N.ptr(g_feat), N.ptr(g_pool), N.ptr(sc), B, C, H, W,
                                                  N.ptr(g_x), N.stream()))
        return (g_x,)
    return _twice(launch)[0]


def _aten_elu_share(x32):
    """ATen's own fp32 F.elu (CPU) against expm1 on the non-positive inputs, as a share of the same bound: for information only."""
    x = torch.from_numpy(np.array(x32))
    neg = x <= 0
    if not bool(neg.any()):
        return 0.0
    err = (torch.nn.functional.elu(x).double() - torch.expm1(x.double())).abs()[neg]
    return float(err.max() / ELU_FWD_ABS)


# ---- the tests ----------------------------------------------------------------------------------------------------------------------

def _id(case):
    return "x".join(str(v) for v in case[0]) + "-" + case[-1]


def test_case_lists_reach_the_forms_they_name():
    """Needs no GPU (tests/test_glue_ref.py runs it too): every case reaches the launch form written beside it, by the rules of the
    host code quoted in this file's docstring, and every form of every kernel is reached."""
    assert all(up_form(*c[0][3:]) == c[2] for c in UP_CASES + [UP_ONES])
    assert all(pad_form(*c[0]) == c[1] for c in PAD_CASES + [PAD_ONES])
    assert all(bn_form(*c[0][2:]) == c[1] for c in BN_CASES + [BN_ONES])
    assert all(stem_form(*c[0]) == c[1] for c in STEM_CASES + [STEM_ONES])
    assert {c[2] for c in UP_CASES} == {"four-wide", "pair"} and {c[1] for c in PAD_CASES} == {"four-wide", "pair", "scalar"}
    assert {c[1] for c in BN_CASES} == {"vector", "scalar"} and {c[1] for c in STEM_CASES} == {"bwd4", "pair"}
    for form in ("four-wide", "pair"):      # per form: no skip, and a skip without gradient
        mine = [c for c in UP_CASES if c[2] == form]
        assert any(c[0][2] == 0 for c in mine) and any(c[0][2] > 0 and not c[1] for c in mine)
    (B, C1, C2, h, w) = UP_CASES[2][0]      # blocks of 256 threads per plane: 2 in the y part, 3 in the skip part, both ragged
    assert (-(-(h * (w // 2)) // 256), -(-(h * w) // 256)) == (2, 3) and (h * (w // 2)) % 256 and (h * w) % 256


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", UP_CASES, ids=_id)
def test_up_cat_pad_vs_fp64(case, data):
    d = up_reference(case, data)
    assert up_form(*case[0][3:]) == case[2]
    name = "up_cat_pad %s %s" % (_id(case), data)
    out, g_y, g_skip = run_up(d)
    check_up_forward(name, d, out)
    print("%-52s ATen fp32 F.elu on the same inputs: %.3f of the bound" % (name, _aten_elu_share(d["y"])))
    check_up_backward(name, d, g_y, g_skip)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("apply_elu", [0, 1], ids=["pad", "elu"])
@pytest.mark.parametrize("case", PAD_CASES, ids=_id)
def test_elu_pad_vs_fp64(case, apply_elu, data):
    d = pad_reference(case, apply_elu, data)
    assert pad_form(*case[0]) == case[1]
    name = "elu_pad %s elu%d %s" % (_id(case), apply_elu, data)
    out, g_z = run_pad(d)
    check_pad_forward(name, d, out)
    if apply_elu:
        print("%-52s ATen fp32 F.elu on the same inputs: %.3f of the bound" % (name, _aten_elu_share(d["z"])))
    check_pad_backward(name, d, g_z)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", BN_CASES, ids=_id)
def test_bn_act_vs_fp64(case, data):
    assert bn_form(*case[0][2:]) == case[1]
    for mode in BN_MODES:
        d = bn_reference(case, mode, data)
        name = "bn_act %s relu%d res-%s %s" % (_id(case), mode[0], mode[1], data)
        out, g_x, g_res = run_bn(d)
        check_bn_forward(name, d, out)
        check_bn_backward(name, d, g_x, g_res)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("case", STEM_CASES, ids=_id)
def test_stem_vs_fp64(case, data):
    d = stem_reference(case, data)
    assert stem_form(*case[0]) == case[1]
    name = "stem %s %s" % (_id(case), data)
    feat, pooled, arg = run_stem_forward(d)
    check_stem_forward(name, d, feat, pooled, arg)
    for gf, gp in STEM_GRADS:
        check_stem_backward("%s g_feat%d g_pool%d" % (name, gf, gp), d, run_stem_backward(d, gf, gp), gf, gp)


def test_sum_cost_hands_every_op_a_stride_0_gradient():
    """cost = out.sum(): the incoming gradient is an expanded scalar (every stride 0), which the backward launchers must copy to a
    contiguous tensor before they take its pointer (ops._c)."""
    from depthmodelhardening_amd import ops
    d = up_reference(UP_ONES, "dyadic", True)
    out, g_y, g_skip = run_up(d)
    check_up_forward("sum cost up_cat_pad", d, out)
    check_up_backward("sum cost up_cat_pad", d, g_y, g_skip)
    d = pad_reference(PAD_ONES, 1, "dyadic", True)
    out, g_z = run_pad(d)
    check_pad_forward("sum cost elu_pad", d, out)
    check_pad_backward("sum cost elu_pad", d, g_z)
    d = bn_reference(BN_ONES, (True, "grad"), "dyadic", True)
    out, g_x, g_res = run_bn(d)
    check_bn_forward("sum cost bn_act", d, out)
    check_bn_backward("sum cost bn_act", d, g_x, g_res)
    d = stem_reference(STEM_ONES, "dyadic", True)

    def launch():       # the stem through its autograd node: feat.sum() + pooled.sum()
        x = _dev(d["x"], True)
        feat, pooled = ops.stem_bn_relu_pool(x, _dev(d["scale"]), _dev(d["shift"]))
        return feat, pooled, torch.autograd.grad(feat.sum() + pooled.sum(), x)[0]
    feat, pooled, g_x = _twice(launch)
    _equal("sum cost stem feat", feat, d["feat"])
    _equal("sum cost stem pooled", pooled, d["pooled"])
    check_stem_backward("sum cost stem", d, g_x, True, True)
