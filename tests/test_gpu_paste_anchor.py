"""Float64 anchors of K3 -- paste_fwd_kernel, paste_fwd4_kernel, paste_fwd_tile_kernel and paste_bwd_kernel of csrc/eot_paste.hip --
in every launch form, against tests/paste_ref.py (plain numpy float64, the adjoint by SCATTER where the kernel gathers;
tests/test_paste_ref.py pins that reference on the float64 chain of oracle/tv082.py and checks every case's input conditions).

(a) Exact-coordinate sweeps through the C ABI.  Power-of-two frames and dyadic affine coefficients: the fp32 sample coordinate of
every composite pixel is EXACT (test_paste_ref.py), so the kernels' index logic has no conditioning to hide behind and the gate is,
element by element, with no outlier share and no additive slack,

        |got - ref64|  <=  n_round * 2^-24 * S                              (tests/util.py: assert_round_bound)

S: the same operation on absolute values (1 - mk becomes 1 + mk), n_round READ FROM THE KERNEL, in roundings of 2^-24 each:

  patch_sample         gx = 1 - fx and gy = 1 - fy (2), the weight gx gy (1), v w (1), three additions (3):     N_SAMPLE = 7
  resize               hx = 1 - lx (1), hx comp (1), the row's sum (1), hy = 1 - ly (1), hy (..) (1), the sum (1):  N_RESIZE = 6
  forward, composite   o mk: N_SAMPLE for each factor and 1 for the product, the composite's sum 1 (the other term,
                       scene (1 - mk), is shorter: N_SAMPLE + 1 + 1 + 1), then the resize: N_FWD_COMPOSITE = 2 * 7 + 2 + 6 = 22
  forward, warp-only   o, then the resize; and mask_out in both modes:                     N_FWD_WARP = 7 + 6 = 13
  backward             wyy and wxx (1 - l, and the sum of the two matches: 2 each), ww = wyy wxx (1): 5;  fmaf into G, one rounding
                       per resize tap of the scene pixel: T;  wu wv (1 - f: 1 each, the product 1): 3;  composite mode:
                       w *= patch_sample(mask): N_SAMPLE + 1;  fmaf into acc, one rounding per candidate pixel that reads the
                       texel, for the ceil(N / 16) samples of a lane: K ceil(N / 16);  the xor-butterfly: 4.
                       n = 5 + T + 3 + (8) + K ceil(N / 16) + 4, with T and K the maxima over the case FROM THE REFERENCE'S INDEX
                       MAP (paste_ref.n_bwd), never from the kernel's output.

hipcc contracts a * b + c into one fused operation: fewer roundings than counted, never more.  The resize fractions of the two
non-dyadic output sizes (60 x 192, 32 x 63) are formed in fp32 exactly as the kernel and ATen form them ('fp32' weights of
paste_ref.resize_matrix), so that they are inputs of the bound, not part of the error.

Outputs are slices of larger buffers, NaN inside, 256 sentinel floats before and after: nothing may stay unwritten, nothing may be
written outside.  Patch-gradient texels that no pixel reads must be exactly 0.0.

(b) Perspective cases through ops.eot_paste / ops.perspective_warp and autograd against the float64 oracle chain (float64 resize
weights: fully independent of the kernel), the same chain in fp32 beside it as the only comparator.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import paste_ref as R
from tests.util import U32, assert_round_bound as _rb, fp64_bound, rel_l2

pytestmark = pytest.mark.gpu

SENTINEL = 12345.678
GUARD = 256


def _lib():
    from depthmodelhardening_amd import _native as N
    return N, N.lib()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


class _Guarded(object):
    """An fp32 output of ``shape`` inside a larger buffer: NaN inside, SENTINEL in the 256 floats before and after.  ``misalign``:
    the output starts one float later (4 bytes off 16-byte alignment)."""

    def __init__(self, shape, misalign=False):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD + 4,), SENTINEL, device="cuda")
        self.lo = GUARD + (1 if misalign else 0)
        self.out = self.buf[self.lo:self.lo + n].view(*shape)
        self.out.fill_(float("nan"))
        assert self.out.data_ptr() % 16 == (4 if misalign else 0) and self.out.is_contiguous()

    def result(self, name):
        n = self.out.numel()
        buf = self.buf.cpu()
        assert bool((buf[:self.lo] == np.float32(SENTINEL)).all()) and bool((buf[self.lo + n:] == np.float32(SENTINEL)).all()), (
            name + ": written outside the output")
        out = buf[self.lo:self.lo + n].view(*self.out.shape)
        assert not bool(torch.isnan(out).any()), name + ": %d elements left unwritten" % int(torch.isnan(out).sum())
        return out


def _args(d, mode, scene, flip, index):
    """The argument struct of a launch, and the device tensors it points to (kept alive by the caller)."""
    from depthmodelhardening_amd import ops
    P = d["P"]
    keep = [_dev(scene) if scene is not None else torch.empty((1, 3, P.SH, P.SW), device="cuda"), _dev(d["patch"]), _dev(d["mask"]),
            _dev(d["coeffs"]), _dev(flip), _dev(index)]
    a = ops._paste_args(keep[0], keep[1], keep[2], keep[3], P.l_pad, P.t_pad, P.OH, P.OW, mode, keep[4], keep[5])
    return a, keep


SHARES = {}         # worst share of the bound per (kernel, case): printed for DESIGN.md's table


# ---- (a) forward ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", [c[0] for c in R.FWD_CASES])
def test_forward_forms_vs_fp64(cid):
    N, lib = _lib()
    d = R.fwd_case(cid)
    P = d["P"]
    worst = 0.0
    for name, mode, kind, flip, outs in R.FWD_VARIANTS:
        scene = {"per": d["scenes"], "bcast": d["scenes"][:1], "pool": d["pool"], None: None}[kind]
        a, keep = _args(d, mode, scene, d["flip"] if flip else None, d["index"] if kind == "pool" else None)
        assert a.scene_bstride == (0 if kind in ("bcast", None) else 3 * P.SH * P.SW) and a.N == P.N == 8
        # the misaligned case moves whichever output comes first off 16-byte alignment
        adv = _Guarded((P.N, 3, P.OH, P.OW), misalign=d["misalign"]) if outs != "mask" else None
        mo = _Guarded((P.N, 1, P.OH, P.OW), misalign=d["misalign"] and adv is None) if outs != "adv" else None
        pa, pm = N.ptr(adv.out) if adv else None, N.ptr(mo.out) if mo else None
        assert lib.dmh_eot_paste_fwd_form(C.byref(a), pa, pm) == d["form"], (cid, name)
        N.check(lib.dmh_eot_paste_fwd(C.byref(a), pa, pm, N.stream()))
        torch.cuda.synchronize()
        want_adv, want_mo, S_adv, S_mo = d[name]
        tag = "%s | %s" % (cid, name)
        if adv:
            worst = max(worst, _rb(tag + " adv", adv.result(tag + " adv"), _t64(want_adv), _t64(S_adv),
                                   R.N_FWD_COMPOSITE if mode == R.COMPOSITE else R.N_FWD_WARP))
        if mo:
            got = mo.result(tag + " mask_out")
            worst = max(worst, _rb(tag + " mask_out", got, _t64(want_mo), _t64(S_mo), R.N_FWD_WARP))
            assert bool((got[_t64(want_mo) == 0] == 0).all()), tag + ": mask_out is not 0.0 where no footprint meets the patch"
    SHARES[("fwd", cid)] = worst
    print("SHARE fwd %-28s form %d  worst share of the bound %.3f" % (cid, d["form"], worst))


def test_forms_agree_bitwise_on_one_shape():
    """32 x 64 -> 32 x 64 is tiled with aligned outputs and generic one float off: the same per-pixel arithmetic."""
    N, lib = _lib()
    d = R.fwd_case("A-32x64-generic-misaligned")
    P = d["P"]
    a, keep = _args(d, R.COMPOSITE, d["scenes"], d["flip"], None)
    res = []
    for mis, form in ((False, R.TILED), (True, R.GENERIC)):
        adv, mo = _Guarded((P.N, 3, P.OH, P.OW), mis), _Guarded((P.N, 1, P.OH, P.OW))
        assert lib.dmh_eot_paste_fwd_form(C.byref(a), N.ptr(adv.out), N.ptr(mo.out)) == form
        N.check(lib.dmh_eot_paste_fwd(C.byref(a), N.ptr(adv.out), N.ptr(mo.out), N.stream()))
        torch.cuda.synchronize()
        res.append((adv.result("adv"), mo.result("mask_out")))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---- (a) backward -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [R.COMPOSITE, R.WARP_ONLY], ids=["composite", "warp-only"])
@pytest.mark.parametrize("cid", [c[0] for c in R.BWD_CASES])
def test_backward_vs_fp64(cid, mode):
    N, lib = _lib()
    d = R.bwd_case(cid)
    P = d["P"]
    r = d[mode]
    # one broadcast scene (the backward never reads it: the gradient passes through mk alone)
    a, keep = _args(d, mode, d["scenes"][:1] if mode == R.COMPOSITE else None, d["flip"], None)
    assert a.N == len(d["names"]) and a.scene_bstride == 0
    g_adv = _dev(d["g_adv"])
    gp = _Guarded((1, 3, P.PH, P.PW))
    N.check(lib.dmh_eot_paste_bwd(C.byref(a), N.ptr(g_adv), N.ptr(gp.out), N.stream()))
    torch.cuda.synchronize()
    tag = "bwd %s %s N %d" % (cid, "composite" if mode == R.COMPOSITE else "warp-only", P.N)
    got = gp.result(tag)[0]
    share = _rb(tag, got, _t64(r["g"]), _t64(r["S"]), r["n_round"])
    unread = torch.from_numpy(np.broadcast_to(r["unread"], (3,) + r["unread"].shape).copy())
    assert bool((got[unread] == 0).all()), tag + ": a texel no pixel reads is not exactly 0.0"
    print("SHARE %-44s n_round %3d  worst share of the bound %.3f  (exact-zero texels %d)" % (tag, r["n_round"], share,
                                                                                               int(r["unread"].sum())))
    # without flip: the same launch against the reference's un-mirrored adjoint
    if cid in ("A-N3", "A-N17"):
        a.flip = None
        gq = _Guarded((1, 3, P.PH, P.PW))
        N.check(lib.dmh_eot_paste_bwd(C.byref(a), N.ptr(g_adv), N.ptr(gq.out), N.stream()))
        torch.cuda.synchronize()
        _rb(tag + " no flip", gq.result(tag)[0], _t64(P.backward(d["g_adv"], d["mask"], mode)),
            _t64(P.backward(d["g_adv"], d["mask"], mode, absolute=True)), r["n_round"])


# ---- (b) perspective cases through the ops and autograd ---------------------------------------------------------------------------------

SEEDS = (0, 1, 2)
_ORACLE = {}


def _persp(geo_name, out, mask_kind, N, seed, warp_only=False):
    """Inputs, the float64 oracle chain and the same chain in fp32, computed once per key."""
    key = (geo_name, out, mask_kind, N, seed, warp_only)
    if key not in _ORACLE:
        g = R.persp_geometry(geo_name)
        gen = torch.Generator().manual_seed(1000 * seed + N)
        frame, hw = g["frame"], g["patch"]
        d = {"scene": torch.rand((N, 3) + frame, generator=gen), "patch": torch.rand((1, 3) + hw, generator=gen),
             "mask": torch.ones((1, 1) + hw) if mask_kind == "ones" else (torch.rand((1, 1) + hw, generator=gen) > 0.3).float(),
             "g_adv": torch.rand((N, 3) + (frame if warp_only else out), generator=gen) - 0.5,
             "coeffs": R.persp_coeffs(g, N)}
        for dt, nm in ((torch.float64, "f64"), (torch.float32, "f32")):
            d[nm] = R.oracle_chain(dt, d["scene"], d["patch"], d["mask"], d["coeffs"], g["pad"], out, d["g_adv"], warp_only)
        _ORACLE[key] = d
    return _ORACLE[key]


def _gates(name, results):
    """results: per seed, a list of (quantity, hip, f32 oracle, f64 oracle).  Primary: fp64_bound per seed and quantity.  Max-abs:
    pooled over the seeds, HIP's largest deviation at most twice the fp32 oracle's, plus 8 x 2^-24 x max |ref64|."""
    pooled = {}
    for per_seed in results:
        for q, hip, o32, o64 in per_seed:
            fp64_bound("%s %s" % (name, q), rel_l2(hip, o64), rel_l2(o32, o64))
            p = pooled.setdefault(q, [0.0, 0.0, 0.0])
            p[0] = max(p[0], float((hip.double().cpu() - o64).abs().max()))
            p[1] = max(p[1], float((o32.double() - o64).abs().max()))
            p[2] = max(p[2], float(o64.abs().max()))
    for q, (e_hip, e_o32, scale) in pooled.items():
        print("%-44s max-abs vs fp64: hip %.3g  fp32 oracle %.3g  (floor %.3g)" % ("%s %s" % (name, q), e_hip, e_o32, 8 * U32 * scale))
        assert e_hip <= 2.0 * e_o32 + 8 * U32 * scale, (name, q, e_hip, e_o32)


@pytest.mark.parametrize("N", [4, 18])
@pytest.mark.parametrize("mask_kind", ["ones", "binary"])
@pytest.mark.parametrize("geo_name,out", R.PERSP_CASES, ids=["%s-%dx%d" % ((g,) + o) for g, o in R.PERSP_CASES])
def test_perspective_paste_vs_fp64_oracle(geo_name, out, mask_kind, N):
    from depthmodelhardening_amd import ops
    g = R.persp_geometry(geo_name)
    results = []
    for seed in SEEDS:
        d = _persp(geo_name, out, mask_kind, N, seed)
        patch = d["patch"].cuda().requires_grad_(True)
        adv, mo = ops.eot_paste(d["scene"].cuda(), patch, d["mask"].cuda(), torch.from_numpy(d["coeffs"]).float().cuda(),
                                g["pad"][0], g["pad"][1], out)
        (gp,) = torch.autograd.grad(adv, patch, d["g_adv"].cuda())
        results.append([(q, h.cpu(), d["f32"][i], d["f64"][i]) for i, (q, h) in enumerate((("adv", adv.detach()), ("mask_out", mo),
                                                                                           ("g_patch", gp)))])
    _gates("%s %dx%d %s N %d" % ((geo_name,) + out + (mask_kind, N)), results)


@pytest.mark.parametrize("geo_name", ["small", "large"])
def test_perspective_warp_only_vs_fp64_oracle(geo_name):
    """ops.perspective_warp (warp-only mode, no resize) and its patch gradient, which no other test checks."""
    from depthmodelhardening_amd import ops
    g = R.persp_geometry(geo_name)
    for mask_kind in ("ones", "binary"):
        results = []
        for seed in SEEDS:
            d = _persp(geo_name, g["frame"], mask_kind, 4, seed, warp_only=True)
            patch = d["patch"].cuda().requires_grad_(True)
            obj, mo = ops.perspective_warp(patch, d["mask"].cuda(), torch.from_numpy(d["coeffs"]).float().cuda(), g["pad"][0],
                                           g["pad"][1], g["frame"])
            (gp,) = torch.autograd.grad(obj, patch, d["g_adv"].cuda())
            results.append([(q, h.cpu(), d["f32"][i], d["f64"][i]) for i, (q, h) in enumerate((("obj", obj.detach()), ("mask_out", mo),
                                                                                               ("g_patch", gp)))])
        _gates("warp-only %s %s" % (geo_name, mask_kind), results)


def test_rmax_boundary_case_is_tiled():
    """40 -> 30 rows: floor(rh * 7) + 3 is exactly RMAX = 12, the last ratio the tiled kernel takes."""
    N, lib = _lib()
    a = N.PasteArgs()
    one = C.c_void_p(64)
    a.scene, a.patch, a.pmask, a.coeffs = one, one, one, one
    a.N, a.SH, a.SW, a.PH, a.PW, a.l_pad, a.t_pad = 4, 40, 64, 12, 16, 24, 10
    forms = {}
    for out in R.PERSP_SMALL["outs"]:
        a.OH, a.OW = out
        forms[out] = lib.dmh_eot_paste_fwd_form(C.byref(a), one, one)
    assert int(np.floor(np.float32(40) / np.float32(30) * 7)) + 3 == 12
    assert forms == {(32, 64): R.TILED, (30, 52): R.TILED, (24, 36): R.FOUR_WIDE, (33, 53): R.GENERIC, (48, 96): R.TILED}, forms
