"""tests/roi_ref.py (K19 in float64 numpy: scatter adjoint, cost, crops, windowed stem backward) held against torch's own
float64 operators on the CPU, the reciprocal row split of csrc/roi_glue.hip in Python integers over its whole domain, and the
input conditions of every case of tests/test_gpu_roi_anchor.py -- so that what that file compares the kernels with is itself
checked, and checked without a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import roi_ref as R


def _torch_frame(y, skip, up, elu):
    e = F.elu(y) if elu else y
    if up:
        e = F.interpolate(e, scale_factor=2, mode="nearest")
    return F.pad(e if skip is None else torch.cat([e, skip], 1), (1, 1, 1, 1), mode="reflect")


def _data(frame, up, B, C1, C2, seed):
    rng = np.random.RandomState(seed)
    FH, FW = frame
    y = rng.standard_normal((B, C1) + ((FH // 2, FW // 2) if up else (FH, FW)))
    skip = rng.standard_normal((B, C2, FH, FW)) if C2 else None
    return rng, y, skip


GEOS = [((24, 40), (10, 12), [(0, 0), (14, 28), (6, 14)]), ((4, 4), (2, 2), [(0, 0), (2, 2), (0, 2)]), ((4, 4), (4, 4), [(0, 0)]),
        ((23, 41), (11, 12), [(0, 0), (12, 28), (6, 14)])]


@pytest.mark.parametrize("up", [0, 1])
@pytest.mark.parametrize("elu", [0, 1])
@pytest.mark.parametrize("C2", [0, 3])
def test_glue_forward_is_the_torch_operators_in_float64(up, elu, C2):
    for frame, size, org in GEOS:
        if up and (frame[0] & 1 or frame[1] & 1):
            continue
        _, y, skip = _data(frame, up, len(org), 4, C2, 1)
        want = _torch_frame(torch.from_numpy(y), None if skip is None else torch.from_numpy(skip), up, elu).numpy()
        got = R.glue_fwd(y, skip, up, elu, org, size)
        for b, (oy, ox) in enumerate(org):
            assert np.abs(got[b] - want[b, :, oy:oy + size[0] + 2, ox:ox + size[1] + 2]).max() <= 1e-12


@pytest.mark.parametrize("up", [0, 1])
def test_glue_backward_is_the_adjoint_of_the_forward(up):
    """<glue_fwd(y, skip), g> == <y, g_y> + <skip, g_skip> with elu = 0 (the forward is linear then)."""
    for frame, size, org in GEOS:
        if up and (frame[0] & 1 or frame[1] & 1):
            continue
        rng, y, skip = _data(frame, up, len(org), 3, 2, 2)
        g = rng.standard_normal((len(org), 5, size[0] + 2, size[1] + 2))
        r = R.glue_bwd(g, y, 2, up, 0, org, size, frame)
        lhs = (R.glue_fwd(y, skip, up, 0, org, size) * g).sum()
        rhs = (y * r["g_y"]).sum() + (skip * r["g_skip"]).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
        # every window entry reads exactly one y element and one skip element
        n = (size[0] + 2) * (size[1] + 2)
        assert (r["n_y"].sum(axis=(1, 2)) == n).all() and (r["n_skip"].sum(axis=(1, 2)) == n).all()


@pytest.mark.parametrize("up", [0, 1])
@pytest.mark.parametrize("elu", [0, 1])
def test_glue_backward_is_float64_autograd(up, elu):
    for frame, size, org in GEOS:
        if up and (frame[0] & 1 or frame[1] & 1):
            continue
        rng, y, skip = _data(frame, up, len(org), 3, 2, 3)
        g = rng.standard_normal((len(org), 5, size[0] + 2, size[1] + 2))
        ty, ts = torch.from_numpy(y).requires_grad_(True), torch.from_numpy(skip).requires_grad_(True)
        P = _torch_frame(ty, ts, up, elu)
        gP = torch.from_numpy(R.embed(g, org, tuple(P.shape)))
        # (embed overwrites; the samples' windows are in different batch rows, so nothing overlaps)
        P.backward(gP)
        r = R.glue_bwd(g, y, 2, up, elu, org, size, frame)
        assert np.abs(r["g_y"] - ty.grad.numpy()).max() <= 1e-12
        assert np.abs(r["g_skip"] - ts.grad.numpy()).max() <= 1e-12
        assert ((r["S_y"] == 0) == (np.broadcast_to(r["n_y"][:, None], y.shape) == 0)).all()
        assert (np.abs(r["g_y"]) <= r["S_y"] * (1 + 1e-15)).all() and (np.abs(r["g_skip"]) <= r["S_skip"] * (1 + 1e-15)).all()


def test_cut_embed_and_boxes():
    rng = np.random.RandomState(4)
    full = rng.standard_normal((3, 2, 9, 11))
    org = np.array([(0, 0), (4, 5), (2, 6)])
    w = R.cut(full, org, (5, 5))
    assert w.shape == (3, 2, 5, 5) and np.array_equal(w[1], full[1, :, 4:9, 5:10])
    e = R.embed(w, org, full.shape, fill=7.0)
    assert np.array_equal(R.cut(e, org, (5, 5)), w) and (e == 7.0).sum() == full.size - w.size
    # the tight boxes: top-left corner of G1 reads rows 0..10 (row -1 reflects to 1), the interior rows 5..16
    lo, hi = R.source_boxes([(0, 0), (6, 14), (14, 28)], (10, 12), (24, 40), 0)
    assert lo.tolist() == [[0, 0], [5, 13], [13, 27]] and hi.tolist() == [[11, 13], [17, 27], [24, 40]]
    lo, hi = R.source_boxes([(0, 0), (6, 14)], (10, 12), (24, 40), 1)
    assert lo.tolist() == [[0, 0], [2, 6]] and hi.tolist() == [[6, 7], [9, 14]]


def test_stem_reference_is_float64_autograd_through_max_pool():
    rng = np.random.RandomState(5)
    B, C, H, W = 2, 3, 12, 16
    z = rng.standard_normal((B, C, H, W))
    scale, shift = np.array([0.7, -1.3, 0.2]), np.array([0.1, 0.0, -0.2])
    tz = torch.from_numpy(z).requires_grad_(True)
    feat = F.relu(tz * torch.from_numpy(scale)[None, :, None, None] + torch.from_numpy(shift)[None, :, None, None])
    pooled, idx = F.max_pool2d(feat, 3, 2, 1, return_indices=True)
    # no ties that matter: a positive pooled maximum is attained once in its 3 x 3 cell (a maximum of 0 is a tie of elements
    # that the ReLU gate zeroes whichever of them the pool names)
    unf = F.unfold(F.pad(feat.detach(), (1, 1, 1, 1), value=-1.0).reshape(B * C, 1, H + 2, W + 2), 3, stride=2)
    unf = unf.reshape(B, C, 9, H // 2, W // 2)
    once = (unf == pooled.detach()[:, :, None]).sum(2) == 1
    assert bool((once | (pooled.detach() == 0)).all()) and bool((pooled > 0).float().mean() > 0.9)
    iy, ix = idx // W, idx % W
    i, j = torch.meshgrid(torch.arange(H // 2), torch.arange(W // 2), indexing="ij")
    arg = ((iy - (2 * i - 1)) * 3 + (ix - (2 * j - 1))).numpy().astype(np.uint8)
    g_pool_full, g_feat = rng.standard_normal((B, C, H // 2, W // 2)), rng.standard_normal((B, C, H, W))
    org, pool_org = np.array([(2, 4), (6, 8)]), np.array([(1, 2), (2, 3)])
    size, psize = (6, 8), (4, 5)
    g_pool_win = R.cut(g_pool_full, pool_org, psize)
    (pooled * torch.from_numpy(R.embed(g_pool_win, pool_org, g_pool_full.shape))).sum().backward(retain_graph=True)
    want_pool_only = R.cut(tz.grad.numpy(), org, size)
    got, S = R.stem_bwd_win(feat.detach().numpy(), arg, None, g_pool_win, scale, org, pool_org, size)
    assert np.abs(got - want_pool_only).max() <= 1e-12 and (np.abs(got) <= S * (1 + 1e-15)).all()
    tz.grad = None
    ((pooled * torch.from_numpy(R.embed(g_pool_win, pool_org, g_pool_full.shape))).sum() + (feat * torch.from_numpy(g_feat)).sum()).backward()
    got, S = R.stem_bwd_win(feat.detach().numpy(), arg, g_feat, g_pool_win, scale, org, pool_org, size)
    assert np.abs(got - R.cut(tz.grad.numpy(), org, size)).max() <= 1e-12 and (np.abs(got) <= S * (1 + 1e-15)).all()


def test_cost_reference_is_float64_autograd():
    rng = np.random.RandomState(6)
    (hd, wd), (H, W), org = R.COST_CASES[0]
    d, mask = rng.standard_normal((3, hd, wd)), rng.uniform(0, 1, (3, H, W))
    td = torch.from_numpy(d).requires_grad_(True)
    m = torch.from_numpy(R.cut(mask[:, None], org, (hd, wd))[:, 0])
    cost = ((torch.sigmoid(td) * m) ** 2).sum() / (3 * H * W)
    (0.7 * cost).backward()
    c, s = R.cost_fwd(d, mask, org)
    assert abs(c - float(cost.detach())) <= 1e-15 and np.abs(s - torch.sigmoid(td).detach().numpy()).max() <= 1e-15
    assert np.abs(R.cost_bwd(s, mask, org, 0.7) - td.grad.numpy()).max() <= 1e-15


def test_crop_and_paste_are_slicing():
    rng = np.random.RandomState(7)
    src, gate = rng.standard_normal((2, 3, 10, 12)), rng.standard_normal((2, 3, 10, 12))
    org = np.array([(0, 2), (4, 4)])
    c = R.crop(src, org, (4, 6), gate)
    assert np.array_equal(c[1], np.where(gate[1, :, 4:8, 4:10] > 0, src[1, :, 4:8, 4:10], 0))
    assert np.array_equal(R.crop(c, org, (4, 6), R.cut(gate, org, (4, 6)), gate_compact=True, src_compact=True), c)
    dst = np.full(src.shape, 9.0)
    p = R.paste(dst, R.cut(src, org - 1 + (org == 0), (6, 8)), org, (4, 6), src_org=org - 1 + (org == 0))
    assert np.array_equal(R.cut(p, org, (4, 6)), R.cut(src, org, (4, 6))) and (p == 9.0).sum() == dst.size - 2 * 3 * 24
    assert np.array_equal(R.paste(dst, src, org, (4, 6)), p)


# ---- split_rc --------------------------------------------------------------------------------------------------------------------------

def _split_samples(w2):
    n = ((1 << 30) - 1) // w2 * w2                 # rows * w2 < 2^30 with the most rows
    magic = R.split_magic(w2)
    parts = [np.arange(0, min(n, 4096), dtype=np.int64)]
    k = np.unique(np.concatenate([np.linspace(0, n // w2, 257).astype(np.int64), n // w2 - np.arange(0, 4)]))
    parts.append((k[:, None] * w2 + np.arange(-2, 3)[None]).ravel())
    e = (((1 << 32) // w2 + 1) * w2 - (1 << 32))          # e w2, e = magic - 2^32 / w2 before magic is cut to 32 bits
    t0 = (1 << 32) // e                                   # 2^32 / (w2 e): where t * e first reaches one row
    parts.append(np.arange(t0 - 2 * w2, t0 + 2 * w2 + 1, dtype=np.int64))
    m0 = t0 // w2 * w2
    parts.append((m0 + np.arange(-3, 4)[:, None] * w2 + np.arange(-2, 3)[None]).ravel())
    t = np.unique(np.concatenate(parts))
    return t[(t >= 0) & (t < n)], magic


def test_split_rc_is_exact_over_its_domain():
    """row = t // w2 and column = t % w2 for every pair width 1..2,100 (region widths to 4,200) over planes of just under 2^30
    elements -- dmh_roi_glue_* refuse larger ones -- sampled around every seam; the correction branch must be what makes it so."""
    hits = {}
    for w2 in range(1, 2101):
        t, magic = _split_samples(w2)
        r, c, over = R.split_rc(t, w2, magic)
        assert np.array_equal(r, t // w2) and np.array_equal(c, t % w2), w2
        hits[w2] = int(over.sum())
    assert hits[1] == 0 and hits[2048] > 0
    # w2 = 2048: magic = 2^21 + 1, the first corrected index is 2^21 + 2047 -- row 1,024 of a 4,096-wide plane
    t = np.arange((1 << 21), (1 << 21) + 4096, dtype=np.int64)
    r, c, over = R.split_rc(t, 2048, R.split_magic(2048))
    assert R.split_magic(2048) == (1 << 21) + 1 and int(t[over][0]) == (1 << 21) + 2047
    wrong, _, _ = R.split_rc(t, 2048, R.split_magic(2048), correct=False)
    assert not np.array_equal(wrong, t // 2048)
    # G5 of the GPU test reaches it: forward and backward run PW / 2 = sw / 2 = 2,048 over 1,100 rows
    frame, size, _ = R.GEOMETRIES["G5"]
    assert (size[1] + 2) // 2 == 2048 and frame[1] // 2 == 2048 and frame[0] * 2048 > (1 << 21) + 2047
    assert (size[0] + 2) * 2048 > (1 << 21) + 2047


# ---- input conditions of the GPU cases -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.GLUE_CASES, ids=R.case_id)
def test_gpu_glue_case_conditions(case):
    geo, C1, C2, up, el, ywin, skip = case
    frame, size, origins = R.GEOMETRIES[geo]
    FH, FW = frame
    assert (C2 == 0) == (skip is None) and size[1] % 2 == 0 and all(oy % 2 == 0 and ox % 2 == 0 for oy, ox in origins)
    assert all(0 <= oy and oy + size[0] <= FH and 0 <= ox and ox + size[1] <= FW for oy, ox in origins)
    assert not up or (FH % 2 == 0 and FW % 2 == 0)
    d = R.glue_inputs(case)
    r = R.glue_bwd(d["g_out"], d["y"], C2, up, el, d["dst_org"], size, frame)
    seen = []
    for idx, y_org, yext, k_org, kext in R.glue_groups(case):
        seen += idx
        org = d["dst_org"][idx]
        if ywin:        # tight: the box of what the window reads, and the reference gradient is exactly zero outside it
            lo, hi = R.source_boxes(org, size, frame, up)
            assert np.array_equal(lo, y_org) and (hi - lo == yext).all()
            inside = R.embed(R.cut(r["g_y"][idx], y_org, yext), y_org, r["g_y"][idx].shape)
            assert np.array_equal(inside, r["g_y"][idx])
            n_in = R.cut(r["n_y"][idx][:, None], y_org, yext)
            assert n_in.sum() == (size[0] + 2) * (size[1] + 2) * len(idx)
            assert (n_in.max(axis=3) > 0).all() and (n_in.max(axis=2) > 0).all()        # every row and column is read
        if skip == "win":
            lo, hi = R.source_boxes(org, size, frame, 0)
            assert np.array_equal(lo, k_org) and (hi - lo == kext).all()
            inside = R.embed(R.cut(r["g_skip"][idx], k_org, kext), k_org, r["g_skip"][idx].shape)
            assert np.array_equal(inside, r["g_skip"][idx])
            n_in = R.cut(r["n_skip"][idx][:, None], k_org, kext)
            assert (n_in.max(axis=3) > 0).all() and (n_in.max(axis=2) > 0).all()
    assert sorted(seen) == list(range(len(origins)))
    # a random gradient has no zero entry, so "no window entry reads it" is what S == 0 says
    assert (d["g_out"] != 0).all()


@pytest.mark.parametrize("case", R.RECT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_gpu_rectangle_case_conditions(case):
    geo, C1, C2, up, el, even = case
    frame, size, origins = R.RECT_GEOMETRY
    assert origins[1] == (frame[0] - size[0], frame[1] - size[1])          # one window flush with the bottom-right corner
    d = R.glue_inputs(case + (None,))
    r = R.glue_bwd(d["g_out"], d["y"], C2, up, el, d["dst_org"], size, frame)
    for which, u in (("g_y", up), ("g_skip", 0)):
        org, ext = R.covering_boxes(origins, size, frame, u, even)
        plane = r[which].shape[2:]
        assert plane[0] * plane[1] >= 3 * ext[0] * ext[1]               # ops._roi_glue_bwd keeps such a rectangle
        assert (ext[1] % 2 == 0 and (org[:, 1] % 2 == 0).all()) if even else ext[1] % 2 == 1
        # the reference gradient is exactly zero outside the rectangles, and the flush one ends with the plane
        assert np.array_equal(R.embed(R.cut(r[which], org, ext), org, r[which].shape), r[which])
        assert (org[1] + ext == plane).all()


def test_gpu_g5_and_side_case_conditions():
    frame, size, origins = R.GEOMETRIES["G5"]
    assert R.G5_CASE[1:] == (1, 0, 0, 0, False, None) and frame[0] * frame[1] * 4 < 19e6 and len(R.glue_groups(R.G5_CASE)) == 2
    for (hd, wd), (H, W), org in R.COST_CASES:
        assert len(org) == 3 and org[-1] == (H - hd, W - wd) and len(set(org)) == 3
        assert all(0 <= oy <= H - hd and 0 <= ox <= W - wd for oy, ox in org)
    assert [-(-hd * wd // 1024) for (hd, wd), _, _ in R.COST_CASES] == [1, 3, 67] and 130 * 520 > 64 * 1024
    for size in R.CROP_WINDOWS:
        org = R.corner_origins(R.CROP_FRAME, size, (2, 6))
        assert (org % 2 == 0).all() and size[1] % 2 == 0 and (org + size <= R.CROP_FRAME).all()
    assert [-(-h * w // 512) for h, w in R.CROP_WINDOWS] == [1, 3] and [-(-h * w // 256) for h, w in R.PASTE_WINDOWS] == [1, 3]
    for frame, size in R.STEM_CASES:
        out = R.stem_cells_outside(frame, size)
        # the four corners' last quads read cells below / right of the window unless the map ends there; the inner sample
        # has cells outside on all four sides
        assert out[0] > 0 and out[1] > 0 and out[2] > 0 and out[3] == 0 and out[4] > 0


def test_gpu_case_list_reaches_every_launch_form():
    """The coverage assertion of tests/test_gpu_roi_anchor.py needs no GPU: it runs here as well."""
    from tests import test_gpu_roi_anchor as G
    G.test_case_list_covers_every_epilogue_cell()
