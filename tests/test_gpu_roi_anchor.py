"""Float64 anchors of K19 -- the windowed glue, cost, crops, paste and stem backward of csrc/roi_glue.hip and csrc/roi_encoder.hip --
in every launch form, against tests/roi_ref.py (plain numpy float64, the adjoint by SCATTER where the kernels gather;
tests/test_roi_ref.py holds that reference to torch's float64 operators and checks the cases' input conditions on the CPU).

Every bound here is an exact-equality claim or, element by element,

        |got - ref64|  <=  n_round * 2^-24 * S                              (tests/util.py: assert_round_bound)

with S from the float64 reference and n_round READ FROM THE KERNEL, in units of 2^-24 (one ulp of a result is two of them):

  expf                 EXPF_ULP = 1 ulp = 2 units (see EXPF_ULP below for where the number comes from)
  glue forward, ELU    elu_f = expf(x) - 1.f: 2 EXPF_ULP for expf, acting on exp(x), + 1 for the subtraction, acting on at most
                       exp(x) + 1: 2 EXPF_ULP + 1 with S = exp(min(y, 0)) + 1.  Without ELU, and on the skip planes: a copy, torch.equal.
  glue backward        gather_pad starts from 0.f and adds at most 3 x 3 readers: 8 rounded additions; an up-sampled source adds
                       its 2 x 2 children's sums: + 3; with ELU "acc * elu_grad(y)": + 1 for the product, + 2 EXPF_ULP for the expf
                       inside: 8 (+ 3) (+ 1 + 2 EXPF_ULP).  S = the scatter of |g_out| (times elu').  The fast paths add fewer.
  cost                 s = 1 / (1 + expf(-d)): 2 EXPF_ULP + 1 (the addition) + 1 (the division); v = s m: + 1; v v doubles v's
                       error, + 1 for the product: 4 EXPF_ULP + 7 per term.  Then ceil(n / (blocks x 256)) additions per thread,
                       block_sum<256> (6 shuffle adds + the 4 wave totals), the finalize kernel's sum and division in double (none)
                       and its cast of the quotient to float (1).  Every term is positive: S is the reference itself.
  sigmoid output       2 EXPF_ULP + 2 (above), S = sigmoid(d).
  cost backward        g * 2 (exact) * inv_n * s * m * m * s * (1 - s): 6 rounded products, the rounding of inv_n to fp32, the
                       subtraction: 8, S = |reference| (one product, no sum).
  windowed stem        at most four pooled gradients meet in an element (the first onto 0.f: 3 rounded additions, counted as 4),
                       + g_feat: 1, * scale: 1: 6.  S = scale [feat > 0] (adjoint of |g_pool| + |g_feat|).
"""
import numpy as np
import pytest
import torch

from tests import roi_ref as R
from tests.util import assert_round_bound as _rb

pytestmark = pytest.mark.gpu

# Largest error of the device's expf, in ulps.  ROCm's math-accuracy table is not among the documentation installed with the
# toolchain, so the number is measured: expf against float64 exp on the device over EVERY fp32 argument of [-20, 0] (1.1e9 of
# them; and of [0, 20], which the cost's sigmoid reaches), the maximum rounded up to a whole ulp.  DESIGN.md, section K19, has
# the measured maxima.
EXPF_ULP = 1
N_ELU_FWD = 2 * EXPF_ULP + 1
N_SIGMOID = 2 * EXPF_ULP + 2
N_COST_TERM = 4 * EXPF_ULP + 7
N_COST_BWD = 8
N_STEM_WIN = 6
BLOCK_SUM_256 = 6 + 4           # common.hpp block_sum<256>: wave_sum's 6 shuffle adds, then the 4 wave totals in order
COST_NT, COST_PER_BLOCK, COST_MAX_BLOCKS = 256, 1024, 64        # csrc/roi_glue.hip: NT, cost_blocks()


def n_glue_bwd(up, elu):
    return 8 + (3 if up else 0) + (1 + 2 * EXPF_ULP if elu else 0)


def n_cost(n):
    blocks = min(max(-(-n // COST_PER_BLOCK), 1), COST_MAX_BLOCKS)
    return N_COST_TERM + -(-n // (blocks * COST_NT)) + BLOCK_SUM_256 + 1


def _lib():
    from depthmodelhardening_amd import _native as N
    return N, N.lib()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _nan(*shape, misalign=False):
    """A NaN-filled fp32 output; ``misalign``: a view that starts one float into its buffer (4 bytes off 8-byte alignment)."""
    n = int(np.prod(shape))
    if not misalign:
        return torch.full((n,), float("nan"), device="cuda").view(*shape)
    t = torch.full((n + 1,), float("nan"), device="cuda")[1:].view(*shape)
    assert t.data_ptr() % 8 == 4 and t.is_contiguous()
    return t


SENTINEL = 12345.678        # finite guard value
GUARD = 256

_REF = {}


def _reference(case):
    """Inputs and float64 results of a case, computed once and shared (read-only) by the tests that need them."""
    if case not in _REF:
        d = R.glue_inputs(case)
        geo, C1, C2, up, el = case[:5]
        d["fwd"] = R.glue_fwd(d["y"], d["skip"], up, el, d["dst_org"], d["size"])
        d["fwd_S"] = R.glue_fwd(np.exp(np.minimum(d["y"].astype(np.float64), 0)) + 1, None, up, 0, d["dst_org"], d["size"])
        d["bwd"] = R.glue_bwd(d["g_out"], d["y"], C2, up, el, d["dst_org"], d["size"], d["frame"])
        for v in list(d.values()) + list(d["bwd"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[case] = d
    return _REF[case]


class _Launch(object):
    """One group of samples of a case on the device: the argument struct and every tensor it points to, kept alive."""

    def __init__(self, case, d, group, misalign_y=False):
        from depthmodelhardening_amd import ops
        geo, C1, C2, up, el, ywin, skip = case
        idx, y_org, yext, k_org, kext = group
        self.idx, self.y_org, self.yext, self.k_org, self.kext, self.C1, self.C2 = idx, y_org, yext, k_org, kext, C1, C2
        y = d["y"][idx]
        y = R.cut(y, y_org, yext) if y_org is not None else y
        if misalign_y:
            buf = torch.empty(y.size + 1, device="cuda")
            self.y = buf[1:].view(*y.shape)
            self.y.copy_(torch.from_numpy(np.ascontiguousarray(y)))
            assert self.y.data_ptr() % 8 == 4
        else:
            self.y = _dev(y)
        sk = None if not C2 else (R.cut(d["skip"][idx], k_org, kext) if k_org is not None else d["skip"][idx])
        self.skip, self.org = _dev(sk), _dev(d["dst_org"][idx])
        self.y_org_d, self.k_org_d = _dev(y_org), _dev(k_org)
        g = d["g_out"][idx]             # between two guards of 256 floats
        self.g_buf = torch.full((g.size + 2 * GUARD,), SENTINEL, device="cuda")
        self.g_out = self.g_buf[GUARD:GUARD + g.size].view(*g.shape)
        self.g_out.copy_(torch.from_numpy(np.ascontiguousarray(g)))
        self.a = ops._roi_glue_args(self.y, self.y_org_d, self.skip, self.k_org_d, self.org, d["size"], d["frame"], up, el)

    def forward(self):
        """dmh_roi_glue_fwd through the C ABI into a NaN-filled output between two guards of one sample's size each: nothing
        may stay unwritten, nothing may be written outside."""
        import ctypes as C
        N, lib = _lib()
        a = self.a
        shape = (a.B, a.C1 + a.C2, a.hc + 2, a.wc + 2)
        n, guard = int(np.prod(shape)), int(np.prod(shape[1:]))
        buf = torch.full((n + 2 * guard,), SENTINEL, device="cuda")
        out = buf[guard:guard + n].view(*shape)
        out.fill_(float("nan"))
        N.check(lib.dmh_roi_glue_fwd(C.byref(a), N.ptr(out), N.stream()))
        torch.cuda.synchronize()
        assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all()), "written outside the output"
        return out.cpu()

    def backward(self, misalign_out=False, y_region=None, skip_region=None, g_y=None, g_skip=None):
        """dmh_roi_glue_bwd through the C ABI into NaN-filled outputs (whole planes: nothing may stay unwritten)."""
        import ctypes as C
        N, lib = _lib()
        g_y = _nan(*self.y.shape, misalign=misalign_out) if g_y is None else g_y
        if self.C2 and g_skip is None:
            g_skip = _nan(*self.skip.shape)
        yo, (yh, yw) = y_region if y_region is not None else (None, (0, 0))
        ko, (kh, kw) = skip_region if skip_region is not None else (None, (0, 0))
        N.check(lib.dmh_roi_glue_bwd(C.byref(self.a), N.ptr(self.g_out), N.ptr(g_y), N.ptr(g_skip), N.ptr(yo), yh, yw, N.ptr(ko),
                                     kh, kw, N.stream()))
        torch.cuda.synchronize()
        return g_y.cpu(), (None if g_skip is None else g_skip.cpu())

    def kernel(self):
        """The backward kernel this group reaches with aligned bases (csrc/roi_glue.hip: dmh_roi_glue_bwd's ``wide``)."""
        sw = self.y.shape[3]
        return R.bwd_kernel(sw, sw, *((self.skip.shape[3],) * 2 if self.C2 else ()))


def _window(full, org, ext):
    return full if org is None else R.cut(full, org, ext)


def _check_backward(name, case, d, L, g_y, g_skip):
    geo, C1, C2, up, el = case[:5]
    r, idx = d["bwd"], L.idx
    n = n_glue_bwd(up, el)
    want, S = _window(r["g_y"][idx], L.y_org, L.yext), _window(r["S_y"][idx], L.y_org, L.yext)
    unread = np.broadcast_to(_window(r["n_y"][idx][:, None], L.y_org, L.yext) == 0, want.shape)
    used = [_rb(name + " g_y", g_y, _t64(want), _t64(S), n)]
    assert bool((g_y[torch.from_numpy(unread.copy())] == 0).all()), name + ": an element no window entry reads is not 0.0"
    if C2:
        want, S = _window(r["g_skip"][idx], L.k_org, L.kext), _window(r["S_skip"][idx], L.k_org, L.kext)
        unread = np.broadcast_to(_window(r["n_skip"][idx][:, None], L.k_org, L.kext) == 0, want.shape)
        used.append(_rb(name + " g_skip", g_skip, _t64(want), _t64(S), 8))
        assert bool((g_skip[torch.from_numpy(unread.copy())] == 0).all()), name + ": an unread skip element is not 0.0"
    return max(used)


def _check_forward(name, case, d, L, out):
    geo, C1, C2, up, el = case[:5]
    want = d["fwd"][L.idx]
    assert out.shape == want.shape
    if el:
        _rb(name + " ELU(y) planes", out[:, :C1], _t64(want[:, :C1]), _t64(d["fwd_S"][L.idx]), N_ELU_FWD)
        pos = torch.from_numpy(want[:, :C1] > 0)        # ELU is the identity there: a copy
        assert torch.equal(out[:, :C1][pos], torch.from_numpy(want[:, :C1].astype(np.float32))[pos])
    else:
        assert torch.equal(out[:, :C1], torch.from_numpy(want[:, :C1].astype(np.float32))), name + ": y planes are a pure copy"
    assert torch.equal(out[:, C1:], torch.from_numpy(want[:, C1:].astype(np.float32))), name + ": skip planes are a pure copy"


# ---- which launch forms the case list reaches -------------------------------------------------------------------------------------

def _case_cells(case):
    """The launch forms one case reaches, from its geometry alone (no launch): flat cells of the issue's list, and one
    (geometry, forward group, backward kernels, up, elu, y form, skip form) tuple."""
    geo, C1, C2, up, el, ywin, skip = case
    frame, size, origins = R.GEOMETRIES[geo]
    plane = (frame[0] >> 1, frame[1] >> 1) if up else frame
    kernels = set()
    for idx, y_org, yext, k_org, kext in R.glue_groups(case):
        sw = yext[1] if ywin else plane[1]
        kw = None if not C2 else (kext[1] if skip == "win" else frame[1])
        kernels.add(R.bwd_kernel(sw, sw, kw, kw))
    cells = {("fwd group", R.fwd_group(C1, C2)), ("up", up), ("elu", el), ("y", "win" if ywin else "whole"), ("skip", skip)}
    cells |= {("bwd", k) for k in kernels}
    for o in origins:
        cells |= {("border", b) for b in R.borders(o, size, frame)}
    return cells, (geo, R.fwd_group(C1, C2), tuple(sorted(kernels)), up, el, "win" if ywin else "whole", skip)


FLAT_CELLS = ({("fwd group", g) for g in (1, 4, 8)} | {("bwd", "two-wide"), ("bwd", "one-element")} | {("up", 0), ("up", 1)} |
              {("elu", 0), ("elu", 1)} | {("y", "win"), ("y", "whole")} | {("skip", None), ("skip", "whole"), ("skip", "win")} |
              {("border", b) for b in ("top", "bottom", "left", "right", "interior")})

# the list of forms, written out: removing (or changing) any case of roi_ref.GLUE_CASES makes the comparison below fail
B12 = ("one-element", "two-wide")
FORMS = {
    ("G1", 1, ("two-wide",), 1, 1, "whole", "whole"),
    ("G1", 4, B12, 1, 1, "win", "win"),
    ("G1", 8, B12, 1, 0, "whole", "win"),
    ("G1", 8, B12, 0, 1, "win", None),
    ("G1", 1, ("two-wide",), 0, 0, "whole", "whole"),
    ("G1", 8, B12, 0, 1, "win", "whole"),
    ("G1", 4, B12, 0, 0, "whole", "win"),
    ("G1e", 8, B12, 1, 1, "win", "win"),
    ("G1e", 4, B12, 0, 1, "win", "win"),
    ("G3a", 8, ("one-element",), 1, 1, "win", "win"),          # 46 / 2 + 1 (+ 1 inside) columns of y, 47 / 48 of skip
    ("G3a", 1, ("two-wide",), 0, 1, "whole", "whole"),
    ("G3a", 4, B12, 1, 0, "whole", "win"),
    ("G3a", 8, B12, 0, 0, "win", None),
    ("G3b", 8, ("two-wide",), 1, 1, "win", None),              # 32 columns of y
    ("G3b", 1, ("one-element",), 1, 1, "win", "win"),          # 63 columns of skip
    ("G3b", 8, ("two-wide",), 0, 0, "whole", "whole"),
    ("G2a", 1, ("two-wide",), 1, 1, "whole", "whole"),
    ("G2a", 1, ("one-element",), 0, 1, "win", "win"),
    ("G2b", 8, ("two-wide",), 1, 0, "whole", "whole"),
    ("G2b", 4, ("two-wide",), 0, 1, "whole", "whole"),
    ("G4a", 1, ("one-element",), 0, 1, "whole", "whole"),
    ("G4a", 8, ("one-element",), 0, 0, "whole", None),
    ("G4b", 4, ("one-element",), 1, 1, "whole", "whole"),
    ("G4b", 1, B12, 1, 0, "win", "win"),
}


def test_case_list_covers_every_epilogue_cell():
    cells, forms = set(), []
    for case in R.GLUE_CASES:
        c, f = _case_cells(case)
        cells |= c
        forms.append(f)
    assert FLAT_CELLS <= cells, sorted(FLAT_CELLS - cells, key=str)
    assert len(set(forms)) == len(forms) and set(forms) == FORMS, (sorted(set(forms) ^ FORMS, key=str))
    # the cells the issue names one by one, against the list: forward groups by channel counts, G4 on the one-element kernel,
    # the w2 == 1 branch of split_rc (a region two elements wide) in G2 with an up-sampled source
    assert [R.fwd_group(*c) for c in ((6, 4), (8, 4), (8, 16), (16, 0), (3, 5))] == [1, 4, 8, 8, 1]
    assert all(f[2] == ("one-element",) for f in forms if f[0] in ("G4a", "G4b") and f[5] == "whole")
    assert any(f[0] in ("G2a", "G2b") and f[3] == 1 and "two-wide" in f[2] for f in forms) and R.GEOMETRIES["G2a"][0][1] // 2 == 2
    # without any one case, the forms are no longer the list
    for k in range(len(forms)):
        assert set(forms[:k] + forms[k + 1:]) != FORMS


# ---- glue, forward and backward -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.GLUE_CASES, ids=R.case_id)
def test_glue_forward_and_backward_vs_fp64(case):
    d = _reference(case)
    forms = set()
    for group in R.glue_groups(case):
        L = _Launch(case, d, group)
        name = "%s samples %s" % (R.case_id(case), group[0])
        _check_forward(name, case, d, L, L.forward())
        g_y, g_skip = L.backward()
        _check_backward(name + " " + L.kernel(), case, d, L, g_y, g_skip)
        forms.add(L.kernel())
    assert tuple(sorted(forms)) == _case_cells(case)[1][2]


@pytest.mark.parametrize("sample", [0, 1])
def test_glue_large_plane_reaches_the_row_split_correction(sample):
    """G5: PW / 2 = sw / 2 = 2,048 over 1,100 rows: flat pair indices beyond 2^21 + 2047, where the reciprocal product is one
    row too large and split_rc's ``--r`` must put it right.  Pure copies and folds: up = 0, elu = 0, one plane."""
    case = R.G5_CASE
    d = _reference(case)
    L = _Launch(case, d, R.glue_groups(case)[sample])
    assert L.idx == [sample] and L.kernel() == "two-wide"
    out = L.forward()
    assert torch.equal(out, torch.from_numpy(d["fwd"][L.idx].astype(np.float32)))
    g_y, _ = L.backward()
    _check_backward("G5 origin %s" % (tuple(d["dst_org"][sample]),), case, d, L, g_y, None)


# ---- rectangles -----------------------------------------------------------------------------------------------------------------------

def _rect_setup(case):
    geo, C1, C2, up, el, even = case
    frame, size, origins = R.RECT_GEOMETRY
    full = case[:5] + (False, "whole")
    if full not in _REF:
        d = R.glue_inputs(full)
        d["bwd"] = R.glue_bwd(d["g_out"], d["y"], C2, up, el, d["dst_org"], size, frame)
        _REF[full] = d
    d = _REF[full]
    B = len(origins)
    L = _Launch(full, d, (list(range(B)), None, None, None, None))
    y_reg, k_reg = R.covering_boxes(origins, size, frame, up, even), R.covering_boxes(origins, size, frame, 0, even)
    return d, L, y_reg, k_reg


@pytest.mark.parametrize("case", R.RECT_CASES, ids=lambda c: "%dx%d-up%d-elu%d-%s" % (c[1:5] + ("even" if c[5] else "odd",)))
def test_glue_backward_rectangles(case):
    """y_region / skip_region through the C ABI into sentinel-filled planes: inside the rectangle the bound, outside the sentinel
    untouched (the kernel writes the rectangle only; the zero fill around it is the caller's, see the next test)."""
    geo, C1, C2, up, el, even = case
    d, L, (yo, yext), (ko, kext) = _rect_setup(case)
    g_y = torch.full(L.y.shape, SENTINEL, device="cuda")
    g_skip = torch.full(L.skip.shape, SENTINEL, device="cuda")
    keep = (_dev(yo), _dev(ko))
    g_y, g_skip = L.backward(y_region=(keep[0], yext), skip_region=(keep[1], kext), g_y=g_y, g_skip=g_skip)
    assert R.bwd_kernel(L.y.shape[3], yext[1], L.skip.shape[3], kext[1]) == ("two-wide" if even else "one-element")
    r = d["bwd"]
    for name, got, want, S, org, ext, n in (("g_y", g_y, r["g_y"], r["S_y"], yo, yext, n_glue_bwd(up, el)),
                                            ("g_skip", g_skip, r["g_skip"], r["S_skip"], ko, kext, 8)):
        inside = torch.from_numpy(R.cut(got.numpy(), org, ext))
        _rb("rectangle %s %s" % (name, "two-wide" if even else "one-element"), inside, _t64(R.cut(want, org, ext)),
            _t64(R.cut(S, org, ext)), n)
        outside = R.embed(np.zeros_like(inside.numpy()), org, got.shape, fill=1.0) == 1.0
        assert bool((got[torch.from_numpy(outside)] == float(np.float32(SENTINEL))).all()), name + ": written outside its rectangle"
        assert outside.sum() == got.numel() - inside.numel()


@pytest.mark.parametrize("prezero", [True, False])
def test_glue_backward_rectangles_zero_fill_contract(prezero):
    """ops._roi_glue_bwd with rectangles (the planes are more than 3 x the rectangles, so it keeps them): g_y exactly zero outside
    its rectangle, and so g_skip -- unless skip_prezero is False: then only the inside is defined."""
    from depthmodelhardening_amd import ops
    case = R.RECT_CASES[0]
    geo, C1, C2, up, el, even = case
    d, L, (yo, yext), (ko, kext) = _rect_setup(case)
    assert L.y.shape[2] * L.y.shape[3] >= 3 * yext[0] * yext[1] and L.skip.shape[2] * L.skip.shape[3] >= 3 * kext[0] * kext[1]
    g_y, g_skip = ops._roi_glue_bwd(L.a, L.g_out, L.y.device, True, y_region=(_dev(yo), yext), skip_region=(_dev(ko), kext),
                                    skip_prezero=prezero)
    torch.cuda.synchronize()
    r = d["bwd"]
    n = n_glue_bwd(up, el)
    if prezero:
        _rb("rectangles via ops g_y", g_y.cpu(), _t64(r["g_y"]), _t64(r["S_y"]), n)
        _rb("rectangles via ops g_skip", g_skip.cpu(), _t64(r["g_skip"]), _t64(r["S_skip"]), 8)
        outside = torch.from_numpy(R.embed(np.zeros((len(yo), C1) + yext), yo, tuple(g_y.shape), fill=1.0) == 1.0)
        assert bool((g_y.cpu()[outside] == 0).all())
        outside = torch.from_numpy(R.embed(np.zeros((len(ko), C2) + kext), ko, tuple(g_skip.shape), fill=1.0) == 1.0)
        assert bool((g_skip.cpu()[outside] == 0).all())
    else:
        _rb("rectangles via ops g_y (skip not pre-zeroed)", g_y.cpu(), _t64(r["g_y"]), _t64(r["S_y"]), n)
        _rb("rectangles via ops g_skip inside", torch.from_numpy(R.cut(g_skip.cpu().numpy(), ko, kext)),
            _t64(R.cut(r["g_skip"], ko, kext)), _t64(R.cut(r["S_skip"], ko, kext)), 8)


# ---- the two backward kernels, bit for bit ----------------------------------------------------------------------------------------------------

TWIN_CASES = [c for c in R.GLUE_CASES if c[0] in ("G1", "G1e", "G3a", "G3b")]


@pytest.mark.parametrize("case", TWIN_CASES, ids=R.case_id)
def test_one_element_backward_is_bitwise_the_two_wide_backward(case):
    """"the same additions in the same order per element".  The same launch twice in one process: once
    as it is (two-wide, where the widths allow it), once with g_y -- and y, which the two-wide kernel reads as float2 -- starting
    one float into their buffers, which fails the launcher's 8-byte test and selects roi_glue_bwd_kernel."""
    d = _reference(case)
    compared = 0
    for group in R.glue_groups(case):
        L = _Launch(case, d, group)
        if L.kernel() != "two-wide":
            continue
        wide_y, wide_k = L.backward()
        M = _Launch(case, d, group, misalign_y=True)
        one_y, one_k = M.backward(misalign_out=True)
        assert torch.equal(one_y, wide_y), "g_y differs between the kernels"
        assert one_k is None or torch.equal(one_k, wide_k), "g_skip differs between the kernels"
        compared += 1
    assert compared or "two-wide" not in _case_cells(case)[1][2]


# ---- cost -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(R.COST_CASES)), ids=["%dx%d" % c[0] for c in R.COST_CASES])
def test_cost_forward_and_backward_vs_fp64(k):
    N, lib = _lib()
    (hd, wd), (H, W), org = R.COST_CASES[k]
    B, n = len(org), hd * wd
    rng = np.random.RandomState(50 + k)
    d = (2.0 * rng.standard_normal((B, hd, wd))).astype(np.float32)
    mask = rng.uniform(0, 1, (B, H, W)).astype(np.float32)
    org = np.array(org, np.int32)
    dd, md, od = _dev(d), _dev(mask), _dev(org)
    nblk = int(lib.dmh_roi_cost_partials_size(B, hd, wd))
    assert nblk == B * min(-(-n // COST_PER_BLOCK), COST_MAX_BLOCKS)
    res = {}
    for scale in (1.0, -1.0):
        sig, partials, cost = _nan(B, hd, wd), _nan(nblk), _nan(1)
        N.check(lib.dmh_roi_cost_fwd_scaled(N.ptr(dd), N.ptr(md), N.ptr(od), B, hd, wd, H, W, scale, N.ptr(sig), N.ptr(partials),
                                            N.ptr(cost), N.stream()))
        torch.cuda.synchronize()
        res[scale] = (cost.cpu(), sig.cpu())
    want, s64 = R.cost_fwd(d.astype(np.float64), mask, org)
    _rb("cost %d x %d (%d blocks / sample)" % (hd, wd, nblk // B), res[1.0][0], _t64([want]), _t64([want]), n_cost(n))
    _rb("sigmoid %d x %d" % (hd, wd), res[1.0][1], _t64(s64), _t64(s64), N_SIGMOID)
    assert torch.equal(res[-1.0][0].view(torch.int32), (-res[1.0][0]).view(torch.int32)) and float(res[-1.0][0]) < 0
    assert torch.equal(res[-1.0][1], res[1.0][1])
    # backward from a sigmoid that does not come from the kernel above: the float64 one rounded to fp32
    s32 = s64.astype(np.float32)
    sd, gs = _dev(s32), torch.tensor([0.7], device="cuda")
    g = {}
    for scale in (1.0, -1.0):
        g_pre = _nan(B, hd, wd)
        N.check(lib.dmh_roi_cost_bwd_scaled(N.ptr(sd), N.ptr(md), N.ptr(od), B, hd, wd, H, W, scale, N.ptr(gs), N.ptr(g_pre),
                                            N.stream()))
        torch.cuda.synchronize()
        g[scale] = g_pre.cpu()
    want = R.cost_bwd(s32.astype(np.float64), mask, org, float(np.float32(0.7)))
    _rb("cost backward %d x %d" % (hd, wd), g[1.0], _t64(want), _t64(np.abs(want)), N_COST_BWD)
    assert torch.equal(g[-1.0].view(torch.int32), (-g[1.0]).view(torch.int32))


# ---- crop, paste ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", R.CROP_WINDOWS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("C", R.CROP_CHANNELS)
def test_crop_modes_are_slicing(C, size):
    N, lib = _lib()
    H, W = R.CROP_FRAME
    org = R.corner_origins(R.CROP_FRAME, size, (2, 6))
    B = len(org)
    rng = np.random.RandomState(60 + C)
    src = rng.standard_normal((B, C, H, W)).astype(np.float32)
    gate = rng.standard_normal((B, C, H, W)).astype(np.float32)
    gate[rng.uniform(size=gate.shape) < 0.1] = 0.0                     # "> 0": a zero gate closes
    g = rng.standard_normal((B, C) + size).astype(np.float32)
    gate_c = R.cut(gate, org, size)
    sd, gd, cd, gcd, od = _dev(src), _dev(gate), _dev(g), _dev(gate_c), _dev(org)
    forms = {
        "mode 0": ((sd, None, None, 0), R.crop(src, org, size)),
        "mode 1": ((sd, gd, None, 0), R.crop(src, org, size, gate)),
        "mode 2": ((None, gd, cd, 0), R.crop(g, org, size, gate, src_compact=True)),
        "mode 1 + 4": ((sd, gcd, None, 1), R.crop(src, org, size, gate_c, gate_compact=True)),
        "mode 2 + 4": ((None, gcd, cd, 1), R.crop(g, org, size, gate_c, gate_compact=True, src_compact=True)),
    }
    for name, ((s_, q_, g_, compact), want) in forms.items():
        out = _nan(B, C, *size)
        N.check(lib.dmh_roi_crop(N.ptr(s_), N.ptr(q_), N.ptr(g_), N.ptr(od), B, C, H, W, size[0], size[1], compact, N.ptr(out),
                                 N.stream()))
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.from_numpy(np.ascontiguousarray(want))), name


@pytest.mark.parametrize("size", R.PASTE_WINDOWS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("C", R.PASTE_CHANNELS)
@pytest.mark.parametrize("windowed", [True, False], ids=["windowsrc", "framesrc"])
def test_paste_writes_its_window_and_nothing_else(windowed, C, size):
    N, lib = _lib()
    H, W = R.PASTE_FRAME
    h, w = size
    org = R.corner_origins(R.PASTE_FRAME, size, (3, 5))
    B = len(org)
    rng = np.random.RandomState(70 + C)
    frame = rng.standard_normal((B, C, H, W)).astype(np.float32)
    if windowed:        # a source window larger than the pasted one, at its own origin
        sh, sw = h + 3, w + 2
        src_org = np.minimum(np.maximum(org - 1, 0), np.array([H - sh, W - sw])).astype(np.int32)
        assert (src_org <= org).all() and (src_org + (sh, sw) >= org + size).all()
        src = R.cut(frame, src_org, (sh, sw))
    else:
        (sh, sw), src_org, src = (H, W), None, frame
    dst = np.full((B, C, H, W), SENTINEL, np.float32)
    dd, sd, od, so = _dev(dst), _dev(src), _dev(org), _dev(src_org)
    N.check(lib.dmh_roi_paste(N.ptr(sd), N.ptr(so), sh, sw, N.ptr(od), B, C, H, W, h, w, N.ptr(dd), N.stream()))
    torch.cuda.synchronize()
    want = R.paste(dst, src, org, size, src_org)
    assert np.array_equal(R.cut(want, org, size), R.cut(frame, org, size)) and (want == np.float32(SENTINEL)).sum() == dst.size - B * C * h * w
    assert torch.equal(dd.cpu(), torch.from_numpy(want))


# ---- the windowed stem backward -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_g_feat", [True, False], ids=["gfeat", "nogfeat"])
@pytest.mark.parametrize("k", range(len(R.STEM_CASES)), ids=["%dx%d" % c[0] for c in R.STEM_CASES])
def test_stem_window_backward_vs_fp64_and_the_whole_frame_kernel(k, with_g_feat):
    N, lib = _lib()
    (H, W), (hs, ws) = R.STEM_CASES[k]
    org, pool_org, (hq, wq) = R.stem_windows((H, W), (hs, ws))
    B, C = len(org), 3
    rng = np.random.RandomState(80 + k)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    scale, shift = np.array([0.7, -1.3, 0.4], np.float32), np.array([0.1, 0.0, -0.2], np.float32)
    xd, sc, sf = _dev(x), _dev(scale), _dev(shift)
    feat, pooled = _nan(B, C, H, W), _nan(B, C, H // 2, W // 2)
    arg = torch.full((B, C, H // 2, W // 2), 255, dtype=torch.uint8, device="cuda")
    N.check(lib.dmh_stem_bn_relu_pool_fwd(N.ptr(xd), N.ptr(sc), N.ptr(sf), B, C, H, W, N.ptr(feat), N.ptr(pooled), N.ptr(arg),
                                          N.stream()))
    g_pool = rng.standard_normal((B, C, hq, wq)).astype(np.float32)
    g_feat = rng.standard_normal((B, C, H, W)).astype(np.float32) if with_g_feat else None
    gp, gf, od, po = _dev(g_pool), _dev(g_feat), _dev(org), _dev(pool_org)
    g_z = _nan(B, C, hs, ws)
    N.check(lib.dmh_stem_bn_relu_pool_bwd_win(N.ptr(feat), N.ptr(arg), N.ptr(gf), N.ptr(gp), N.ptr(sc), N.ptr(od), N.ptr(po), B, C, H,
                                              W, hs, ws, hq, wq, N.ptr(g_z), N.stream()))
    torch.cuda.synchronize()
    want, S = R.stem_bwd_win(feat.cpu().numpy().astype(np.float64), arg.cpu().numpy(), g_feat, g_pool, scale, org, pool_org,
                             (hs, ws))
    assert (S > 0).mean() > 0.05            # (the inputs: a fair share of the window takes a gradient at all)
    _rb("stem window %d x %d in %d x %d" % (hs, ws, H, W), g_z.cpu(), _t64(want), _t64(S), N_STEM_WIN)
    # bit-identical to the whole-frame kernel fed the embedded g_pool, cut to the window
    gp_full = _dev(R.embed(g_pool, pool_org, (B, C, H // 2, W // 2)))
    g_full = _nan(B, C, H, W)
    N.check(lib.dmh_stem_bn_relu_pool_bwd(N.ptr(feat), N.ptr(arg), N.ptr(gf), N.ptr(gp_full), N.ptr(sc), B, C, H, W, N.ptr(g_full),
                                          N.stream()))
    torch.cuda.synchronize()
    assert torch.equal(g_z.cpu(), torch.from_numpy(R.cut(g_full.cpu().numpy(), org, (hs, ws))))
