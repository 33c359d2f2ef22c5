"""tests/paste_ref.py (K3 in float64 numpy, adjoint by scatter) pinned on the float64 torch chain of oracle/tv082.py, and the input
conditions of every case of tests/test_gpu_paste_anchor.py checked on the CPU, so that no GPU case can pass emptily: exact fp32
coordinates, a mask that is nonzero on the patch border, objects over all four frame edges and across the tile seams, the launch
forms and sample counts the case list reaches -- and five broken references that the rounding bound must catch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import paste_ref as R
from tests.util import U32, round_bound_violations

C, W = R.COMPOSITE, R.WARP_ONLY


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _close(name, got, want, tol=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= tol * max(1.0, np.abs(want).max()), (name, err)


# ---- the reference against the float64 oracle chain ---------------------------------------------------------------------------------

PIN_CASES = [
    # (id, geometry | exact frame, out, N, flip, scene kind, mode)
    ("perspective-per-sample", "small", (30, 52), 4, False, "per", C),
    ("perspective-flip-broadcast", "small", (33, 53), 6, True, "bcast", C),
    ("perspective-pool-upsize", "small", (48, 96), 5, True, "pool", C),
    ("perspective-large", "large", (84, 200), 4, True, "per", C),
    ("perspective-warp-only", "small", (40, 64), 4, False, None, W),
    ("affine-flip", "affine", (32, 63), 8, True, "per", C),
    ("affine-warp-only-flip", "affine", (32, 64), 8, True, None, W),
]


@pytest.mark.parametrize("case", PIN_CASES, ids=[c[0] for c in PIN_CASES])
def test_reference_is_the_float64_oracle_chain(case):
    cid, geo, out, N, flip, kind, mode = case
    rng = np.random.RandomState(len(cid))
    if geo == "affine":
        frame, hw, pad, coeffs = R.FRAME_A, (11, 15), (24, 10), R.coeffs_of(R.SETS_A[:N])
    else:
        g = R.persp_geometry(geo)
        frame, hw, pad, coeffs = g["frame"], g["patch"], g["pad"], R.persp_coeffs(g, N)
    patch, mask = rng.uniform(0, 1, (1, 3) + hw), (rng.uniform(0, 1, (1, 1) + hw) > 0.3) * rng.uniform(0.2, 1, (1, 1) + hw)
    pool = rng.uniform(0, 1, ({"per": N, "bcast": 1, "pool": 3, None: 1}[kind], 3) + frame)
    index = rng.randint(0, 3, N) if kind == "pool" else None
    flips = R.flips_of(N) if flip else None
    g_adv = rng.uniform(-0.5, 0.5, (N, 3) + out)
    P = R.Paste(coeffs, frame, hw, pad, out)
    adv, mo = P.forward(pool, patch, mask, mode, flips, index)
    gp = P.backward(g_adv, mask, mode, flips)
    # the oracle: torch in float64, sample by sample; the mirror applied to the finished sample and to the gradient fed back
    mirror = lambda a: np.stack([a[n][..., ::-1] if flips is not None and flips[n] else a[n] for n in range(N)])     # noqa: E731
    scenes = pool[index] if index is not None else pool
    a64, m64, g64 = R.oracle_chain(torch.float64, scenes, patch, mask, coeffs, pad, out, g_adv=mirror(g_adv), warp_only=mode == W)
    _close(cid + " adv", adv, mirror(a64.numpy()))
    _close(cid + " mask_out", mo, mirror(m64.numpy()))
    _close(cid + " g_patch", gp, g64.numpy()[0])
    assert np.abs(gp).max() > 0.1 and mo.max() > 0.5


def test_adjoint_is_the_transpose_of_the_forward():
    """<g, forward(p)> - <g, forward(0)> == <backward(g), p>: the scatter is the forward's own transpose (the map is affine in p)."""
    d = R.bwd_case("A-N3")
    P = d["P"]
    for mode in (C, W):
        f1 = P.forward(d["scenes"][:3], d["patch"], d["mask"], mode, d["flip"])[0]
        f0 = P.forward(d["scenes"][:3], 0 * d["patch"], d["mask"], mode, d["flip"])[0]
        lhs, rhs = ((f1 - f0) * d["g_adv"]).sum(), (d[mode]["g"] * d["patch"][0]).sum()
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (mode, lhs, rhs)


@pytest.mark.parametrize("S,O", [(64, 63), (64, 60), (256, 192), (40, 33), (64, 53), (32, 64), (64, 16)])
def test_fp32_resize_weights_are_atens(S, O):
    """The 'fp32' weights against fp32 F.interpolate of a float64 composite rounded to fp32: the same taps and fractions, so the two
    differ by the roundings of ATen's own lerps alone (N_RESIZE of them, each on at most the sum S = the resize itself: the data
    is positive) -- one wrong index or a fraction off by an ulp of the COORDINATE is orders above that.  And with a dyadic ratio
    the two weight modes are the same matrix."""
    rng = np.random.RandomState(S + O)
    comp = rng.uniform(0, 1, (1, 1, 7, S)).astype(np.float32)
    got = F.interpolate(torch.from_numpy(comp), size=[7, O], mode="bilinear", align_corners=False).double()
    Rx = R.resize_matrix(S, O, "fp32")
    want = _t(comp.astype(np.float64) @ Rx.T)
    assert not round_bound_violations(got, want, want, R.N_RESIZE).any()
    if (S, O) == (64, 63):      # the coordinate with a separately rounded product is NOT ATen's: one column is an ulp of 62 off
        f = np.float32
        src = np.maximum(f(S) / f(O) * (np.arange(O, dtype=f) + f(0.5)) - f(0.5), f(0))
        lam = (src - np.floor(src)).astype(np.float64)
        Ru = np.zeros((O, S))
        np.add.at(Ru, (np.arange(O), src.astype(int)), 1 - lam)
        np.add.at(Ru, (np.arange(O), np.minimum(src.astype(int) + 1, S - 1)), lam)
        unfused = _t(comp.astype(np.float64) @ Ru.T)
        assert round_bound_violations(got, unfused, unfused, R.N_RESIZE).any()
    assert np.allclose(Rx.sum(1), 1.0, atol=1e-15) and (Rx >= 0).all()
    if S % O == 0 or O % S == 0:
        assert np.array_equal(Rx, R.resize_matrix(S, O, "float64"))
    else:
        assert np.abs(Rx - R.resize_matrix(S, O, "float64")).max() < 64 * S * U32


# ---- input conditions of the exact cases ---------------------------------------------------------------------------------------------

ALL_EXACT = [("fwd", c[0]) for c in R.FWD_CASES] + [("bwd", c[0]) for c in R.BWD_CASES]


def _case(kind, cid):
    return R.fwd_case(cid) if kind == "fwd" else R.bwd_case(cid)


@pytest.mark.parametrize("kind,cid", ALL_EXACT, ids=["%s-%s" % k for k in ALL_EXACT])
def test_exact_cases_have_exact_fp32_coordinates_and_a_live_border(kind, cid):
    d = _case(kind, cid)
    P = d["P"]
    x64, y64 = R.sample_coords(P.coeffs, P.SH, P.SW)
    x32, y32 = R.sample_coords_fp32(P.coeffs, P.SH, P.SW)
    assert np.array_equal(x32.astype(np.float64), x64) and np.array_equal(y32.astype(np.float64), y64)
    assert (P.coeffs[:, 6:] == 0).all() and P.SH in (32, 64) and P.SW in (64, 256)
    m = d["mask"][0, 0]
    assert (m[0] > 0).all() and (m[-1] > 0).all() and (m[:, 0] > 0).all() and (m[:, -1] > 0).all()
    assert d["patch"].min() >= 0 and d["patch"].max() <= 1 and P.SH * P.SW <= 96 * 320
    # the padded patch lies inside the frame; no texel's candidate box comes near the 64 pixels at which the backward gives up
    assert P.l_pad + P.PW <= P.SW and P.t_pad + P.PH <= P.SH
    lin = P.coeffs[:, [0, 1, 3, 4]].reshape(-1, 2, 2)
    assert (2 * np.abs(np.linalg.inv(lin)).sum(-1) + 2 < 64).all()


def test_objects_cross_every_frame_edge_and_the_tile_seams():
    for sets, frame, patch in ((R.SETS_A, R.FRAME_A, "p11x15"), (R.SETS_A, R.FRAME_A, "p12x16"), (R.SETS_B, R.FRAME_B, "p20x28")):
        hw, pad = R.PATCHES[patch]
        ext = R.object_extent(R.coeffs_of(sets), frame, hw, pad)
        assert all(e is not None for e in ext)
        assert set().union(*(R.edges_crossed(e, frame) for e in ext)) == {"top", "bottom", "left", "right"}
        assert any(not R.edges_crossed(e, frame) for e in ext)
    col128 = False
    for cid, frame, patch, out, form, mis, wts, mk, sets in R.FWD_CASES:
        d = R.fwd_case(cid)
        live = d["composite, broadcast scene, adv only"][1][:, 0] != 0          # un-mirrored mask_out [N, OH, OW]
        assert live.any(axis=(1, 2)).all()
        if form == R.TILED:
            assert (live[:, 7:-1:8] & live[:, 8::8]).any(), cid + ": no object across a tile's row seam"
            col128 = col128 or (out[1] > 128 and bool((live[:, :, 127] & live[:, :, 128]).any()))
        if form in (R.TILED, R.FOUR_WIDE):
            groups = live.reshape(live.shape[0], out[0], out[1] // 4, 4).sum(-1)
            assert (groups == 0).any() and ((groups > 0) & (groups < 4)).any() and (groups == 4).any(), cid
    assert col128, "no tiled case puts an object across output column 128"


def test_gradient_coverage_of_the_backward_cases():
    zeros = 0
    for c in R.BWD_CASES:
        d = R.bwd_case(c[0])
        for mode in (C, W):
            g, unread = d[mode]["g"], d[mode]["unread"]
            assert ((g == 0).all(0) == unread).all(), (c[0], "a texel is exactly 0.0 exactly where no pixel reads it")
            if c[0] in R.FULL_COVERAGE:
                assert not unread.any() and (g != 0).all(), c[0]
            assert (d[mode]["S"][:, ~unread] > 0).all()
        if c[0] == "A-N1-s25":
            zeros = int(d[C]["unread"].sum())
            assert 0 < zeros < g[0].size // 2 and "s25" in c[6]
    assert zeros > 0
    assert (11 * 15) % R.LPT != 0 and any(c[2] == "p11x15" for c in R.BWD_CASES)        # a ragged last group of 16 lanes


def test_perspective_cases_lie_in_front_of_the_horizon_and_reach_their_cells():
    """(b): paste_bwd_kernel leaves out a sample for a texel when c6 x + c7 y + 1 is not positive at a corner of its candidate
    box, or when the box is wider than 64 pixels (a limit of the kernel; the forward pastes there all the same).
    No case of (b) may come near either: the denominator is positive on the whole object and around it, the boxes are small."""
    for name in ("small", "large"):
        g = R.persp_geometry(name)
        (SH, SW), hw, pad = g["frame"], g["patch"], g["pad"]
        coeffs = R.persp_coeffs(g, 18)
        tex, w = R.index_map(coeffs, SH, SW, hw[0], hw[1], pad[0], pad[1])
        xn, yn = np.arange(SW)[None, None, :] + 0.5, np.arange(SH)[None, :, None] + 0.5
        den = coeffs[:, 6, None, None] * xn + coeffs[:, 7, None, None] * yn + 1.0
        hit = ((tex >= 0) & (w != 0)).any(-1).reshape(18, SH, SW)
        assert hit.any(axis=(1, 2)).all() and den[hit].min() > 0.25
        x, y = R.sample_coords(coeffs, SH, SW)
        for n in range(18):      # scene pixels per texel along both axes, on the object: far below 64 / 2
            gx, gy = np.gradient(x[n]), np.gradient(y[n])
            jac = np.abs(gx[1] * gy[0] - gx[0] * gy[1])[hit[n]]
            assert jac.min() > 1.0 / 16 ** 2, (name, n, jac.min())
        edges = [R.edges_crossed(e, g["frame"]) for e in R.object_extent(coeffs[:4], g["frame"], hw, pad)]
        assert set().union(*edges) >= {"left", "right", "bottom"}, edges
    # the larger frame: an object across output column 128 of (80, 256); (30, 52) of the smaller one sits exactly at RMAX
    g = R.PERSP_LARGE
    P = R.Paste(R.persp_coeffs(g, 4), g["frame"], g["patch"], g["pad"], (80, 256))
    live = P.forward(np.zeros((1, 3) + g["frame"]), np.zeros((1, 3) + g["patch"]), np.ones((1, 1) + g["patch"]))[1][:, 0] != 0
    assert (live[:, :, 127] & live[:, :, 128]).any()
    assert int(np.floor(np.float32(40) / np.float32(30) * np.float32(7))) + 3 == 12


# ---- the case list, written out ----------------------------------------------------------------------------------------------------------

def _n_class(N):
    return "1" if N == 1 else ("<16" if N < R.LPT else ("16" if N == R.LPT else ("17..32" if N <= 2 * R.LPT else ">32")))


def _cells():
    cells = []
    for cid, frame, patch, out, form, mis, wts, mk, sets in R.FWD_CASES:
        hw, pad = R.PATCHES[patch]
        edges = set().union(*(R.edges_crossed(e, frame) for e in R.object_extent(R.coeffs_of(sets), frame, hw, pad)))
        ratio = "up" if out[0] > frame[0] else ("same" if out == frame else "down")
        cells.append(("fwd", form, "%dx%d" % frame, patch, ratio, "misaligned" if mis else "aligned", wts, mk, _n_class(len(sets)),
                      tuple(sorted(edges))))
    for cid, frame, patch, out, wts, mk, names in R.BWD_CASES:
        hw, pad = R.PATCHES[patch]
        edges = set().union(*(R.edges_crossed(e, frame) for e in R.object_extent(R.coeffs_of(names), frame, hw, pad)))
        ratio = "up" if out[0] > frame[0] else ("same" if out == frame else "down")
        cells.append(("bwd", "%dx%d" % frame, patch, ratio, wts, mk, _n_class(len(names)), tuple(sorted(edges))))
    return cells


ALL_EDGES = ("bottom", "left", "right", "top")
CELLS = {
    ("fwd", R.TILED, "32x64", "p11x15", "same", "aligned", "float64", "ones", "<16", ALL_EDGES),
    ("fwd", R.TILED, "32x64", "p12x16", "up", "aligned", "float64", "uniform", "<16", ALL_EDGES),
    ("fwd", R.TILED, "64x256", "p20x28", "same", "aligned", "float64", "uniform", "<16", ALL_EDGES),
    ("fwd", R.TILED, "64x256", "p20x28", "down", "aligned", "fp32", "ones", "<16", ALL_EDGES),
    ("fwd", R.FOUR_WIDE, "64x256", "p20x28", "down", "aligned", "fp32", "uniform", "<16", ALL_EDGES),
    ("fwd", R.FOUR_WIDE, "32x64", "p12x16", "down", "aligned", "float64", "ones", "<16", ALL_EDGES),
    ("fwd", R.GENERIC, "32x64", "p11x15", "down", "aligned", "fp32", "uniform", "<16", ALL_EDGES),
    ("fwd", R.GENERIC, "32x64", "p12x16", "same", "misaligned", "float64", "uniform", "<16", ALL_EDGES),
    ("bwd", "32x64", "p12x16", "same", "float64", "ones", "1", ()),
    ("bwd", "32x64", "p11x15", "down", "float64", "uniform", "1", ("left", "top")),
    ("bwd", "32x64", "p12x16", "down", "fp32", "uniform", "<16", ("bottom", "right")),
    ("bwd", "32x64", "p11x15", "up", "float64", "ones", "16", ALL_EDGES),
    ("bwd", "32x64", "p12x16", "same", "float64", "ones", "17..32", ALL_EDGES),
    ("bwd", "64x256", "p20x28", "same", "float64", "uniform", "<16", ("left", "top")),
    ("bwd", "64x256", "p20x28", "down", "fp32", "uniform", ">32", ALL_EDGES),
}


def test_case_list_reaches_every_listed_cell():
    cells = _cells()
    assert len(set(cells)) == len(cells) and set(cells) == CELLS, sorted(set(cells) ^ CELLS, key=str)
    for k in range(len(cells)):                 # without any one case, the cells are no longer the list
        assert set(cells[:k] + cells[k + 1:]) != CELLS
    assert {c[1] for c in cells if c[0] == "fwd"} == {R.TILED, R.FOUR_WIDE, R.GENERIC}
    assert [len(c[6]) for c in R.BWD_CASES] == [1, 1, 3, 16, 17, 3, 33]
    # every forward case runs composite and warp-only, with and without flip, with adv or mask_out missing, and the three scene kinds
    v = R.FWD_VARIANTS
    assert {x[1] for x in v} == {C, W} and {x[3] for x in v} == {True, False} and {x[4] for x in v} == {"both", "adv", "mask"}
    assert {x[2] for x in v} == {"per", "bcast", "pool", None} and R.SCENE_POOL == (2, 0, 2, 1)


# ---- the bound bites: five broken references -----------------------------------------------------------------------------------------

def _bwd_violations(d, mode, got):
    r = d[mode]
    return int(round_bound_violations(_t(got), _t(r["g"]), _t(r["S"]), r["n_round"]).sum())


def _with_taps(d, tex, w):
    P = d["P"]
    return R.Paste(P.coeffs, (P.SH, P.SW), (P.PH, P.PW), (P.l_pad, P.t_pad), (P.OH, P.OW), taps=(tex, w))


def test_bound_catches_a_dropped_border_tap():
    """Forward and backward without the taps onto the patch's last column."""
    d = R.fwd_case("A-32x64-tiled")
    P = d["P"]
    tex, w = (a.copy() for a in P.taps)
    tex[(tex >= 0) & (tex % P.PW == P.PW - 1)] = -1         # (every forward case has N = 8: one of each coefficient set)
    Q = _with_taps(d, tex, w)
    name = "composite, per-sample scenes, flip"
    adv, mo, S_adv, S_mo = d[name]
    got_adv, got_mo = Q.forward(d["scenes"], d["patch"], d["mask"], C, d["flip"])
    assert round_bound_violations(_t(got_adv), _t(adv), _t(S_adv), R.N_FWD_COMPOSITE).any()
    assert round_bound_violations(_t(got_mo), _t(mo), _t(S_mo), R.N_FWD_WARP).any()
    b = R.bwd_case("A-N17")
    tex, w = (a.copy() for a in b["P"].taps)
    tex[(tex >= 0) & (tex % b["P"].PW == b["P"].PW - 1)] = -1
    for mode in (C, W):
        assert _bwd_violations(b, mode, _with_taps(b, tex, w).backward(b["g_adv"], b["mask"], mode, b["flip"])) > 0


@pytest.mark.parametrize("cid", ["A-N1-magl", "A-N3", "B-N3"])
def test_bound_catches_a_candidate_box_shrunk_by_one_pixel(cid):
    """Per sample and texel, the readers in the rightmost pixel column of the texel's readers are lost (Xhi less one)."""
    d = R.bwd_case(cid)
    P = d["P"]
    tex, w = (a.copy() for a in P.taps)
    X = np.broadcast_to((np.arange(P.SH * P.SW) % P.SW)[None, :, None], tex.shape)
    for n in range(P.N):
        hit = (tex[n] >= 0) & (w[n] != 0)
        xmax = np.full(P.PH * P.PW, -1)
        np.maximum.at(xmax, tex[n][hit], X[n][hit])
        w[n][hit & (X[n] == xmax[np.maximum(tex[n], 0)])] = 0.0
    for mode in (C, W):
        assert _bwd_violations(d, mode, _with_taps(d, tex, w).backward(d["g_adv"], d["mask"], mode, d["flip"])) > 0


def test_bound_catches_an_ignored_x0_minus_one_tap():
    """Pixels whose footprint starts one texel left of the patch (x0 == -1) still read column 0 with weight fx."""
    for cid in ("A-N3", "A-N17"):
        d = R.bwd_case(cid)
        P = d["P"]
        tex, w = (a.copy() for a in P.taps)
        x0 =np.floor(R.sample_coords(P.coeffs, P.SH, P.SW)[0]).reshape(P.N, -1) - P.l_pad
        assert (x0 == -1).any()
        tex[np.broadcast_to((x0 == -1)[:, :, None], tex.shape)] = -1
        for mode in (C, W):
            assert _bwd_violations(d, mode, _with_taps(d, tex, w).backward(d["g_adv"], d["mask"], mode, d["flip"])) > 0
    d = R.fwd_case("A-16x32-fourwide")
    P = d["P"]
    tex, w = (a.copy() for a in P.taps)
    x0 = np.floor(R.sample_coords(P.coeffs, P.SH, P.SW)[0]).reshape(P.N, -1) - P.l_pad
    tex[np.broadcast_to((x0 == -1)[:, :, None], tex.shape)] = -1
    adv, mo, S_adv, S_mo = d["warp-only, flip"]
    got = _with_taps(d, tex, w).forward(None, d["patch"], d["mask"], W, d["flip"])[0]
    assert round_bound_violations(_t(got), _t(adv), _t(S_adv), R.N_FWD_WARP).any()


def test_bound_catches_a_skipped_sample_and_a_misplaced_flip():
    d = R.bwd_case("A-N17")
    P = d["P"]
    for mode in (C, W):
        assert _bwd_violations(d, mode, P.backward(d["g_adv"], d["mask"], mode, d["flip"], skip_samples=(16,))) > 0
        assert _bwd_violations(d, mode, P.backward(d["g_adv"], d["mask"], mode, np.roll(d["flip"], 1))) > 0
        assert _bwd_violations(d, mode, P.backward(d["g_adv"], d["mask"], mode, d["flip"])) == 0
    f = R.fwd_case("A-32x63-generic")
    adv, mo, S_adv, S_mo = f["composite, per-sample scenes, flip"]
    got = f["P"].forward(f["scenes"], f["patch"], f["mask"], C, np.roll(f["flip"], 1))
    assert round_bound_violations(_t(got[0]), _t(adv), _t(S_adv), R.N_FWD_COMPOSITE).any()
    assert round_bound_violations(_t(got[1]), _t(mo), _t(S_mo), R.N_FWD_WARP).any()


def test_reference_of_the_largest_frame_is_quick():
    import time
    c = [c for c in R.BWD_CASES if c[0] == "B-N3"][0]
    hw, pad = R.PATCHES[c[2]]
    d = R.case_inputs(c[0], c[1], c[2], 3, c[5], c[3])
    t0 = time.time()
    P = R.Paste(R.coeffs_of(c[6]), c[1], hw, pad, c[3], c[4])
    P.forward(d["scenes"], d["patch"], d["mask"])
    P.backward(d["g_adv"], d["mask"])
    assert time.time() - t0 < 1.0
