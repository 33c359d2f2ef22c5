"""The tail of the weight-gradient kernels: the slice reductions of K16, K18, K20 and K21, and K16 / K20 as a whole.

Every kernel of this family leaves one partial per workgroup (or wave) in a workspace the caller owns and a second launch adds
the partials of each output in a documented, fixed order.  The reduce kernels issue their loads in register batches of 32
(16 in K20: csrc/common.hpp, chain_sum) with tails of 16, 8, ... 1; the shapes here are the smallest whose chains are at
least nine partials long, are no multiple of the batch, reach the full batch once, and end in a ragged tile.

  * pure sums (K20 dmh_down_wrw, K16 dmh_conv3x3_small_wrw at C = 16 and 32, K21 dmh_stem_wrw): every output is rebuilt from
    the workspace with fp32 tensor additions in the kernel's order.  An elementwise fp32 addition is correctly rounded, so the
    rebuilt filter must be EQUAL, bit for bit.  The workspace is NaN before the call: a partial the producer did not write would
    poison the outputs, and the NaN guard behind dmh_*_workspace_size must survive.
  * K18 (dmh_wino_wrw) applies G^T . G after the sum: float64 anchor at the bound of tests/test_gpu_conv_anchor.py, twice bit
    for bit.
  * K16 and K20 as a whole: the same float64 anchors, twice bit for bit.
"""
import pytest
import torch

from tests.util import fp64_bound as _bound, rel_fp64 as _rel

pytestmark = pytest.mark.gpu

GUARD = 4096            # floats of NaN behind the workspace


def _N():
    from depthmodelhardening_amd import _native as N
    return N, N.lib()


def _workspace(n):
    """n floats of workspace and a guard behind them, all NaN."""
    buf = torch.full((n + GUARD,), float("nan"), device="cuda")
    return buf, buf[:n]


def _guard_intact(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def _seq_sum(parts):
    """0 + parts[0] + parts[1] + ... in that order, in fp32 (parts: [n, ...])."""
    acc = torch.zeros_like(parts[0]) if len(parts) else None
    for p in parts:
        acc = acc + p
    return acc


# ---- K20 ----------------------------------------------------------------------------------------------------------------------

def _k20_case(B, C, K, H, W, with_d):
    N, lib = _N()
    g0 = torch.Generator().manual_seed(5 + C + W)
    x = torch.randn(B, C, H, W, generator=g0).cuda()
    px = (H // 2) * (W // 2)
    g3 = (torch.randn(B, K, H // 2, W // 2, generator=g0) / px ** 0.5).cuda()
    gd = (torch.randn(B, K, H // 2, W // 2, generator=g0) / px ** 0.5).cuda() if with_d else None
    n = lib.dmh_down_wrw_workspace_size(B, C, K, H, W)
    assert n > 0
    outs = []
    for _ in range(2):
        buf, ws = _workspace(n)
        dw3 = torch.full((K, C, 3, 3), float("nan"), device="cuda")
        dwd = torch.full((K, C), float("nan"), device="cuda") if with_d else None
        N.check(lib.dmh_down_wrw(N.ptr(x), N.ptr(g3), N.ptr(gd) if with_d else None, B, C, K, H, W, N.ptr(ws), N.ptr(dw3),
                                 N.ptr(dwd) if with_d else None, N.stream()))
        torch.cuda.synchronize()
        assert _guard_intact(buf, n)
        outs.append((dw3, dwd, ws))
    return x, g3, gd, outs


K20_SHAPES = [(3, 64, 64, 6, 72), (4, 128, 128, 6, 40)]    # 18 slices of one pair (16 + 2); 12 slices of each of four pairs


@pytest.mark.parametrize("with_d", [True, False], ids=["shortcut", "3x3-only"])
@pytest.mark.parametrize("shape", K20_SHAPES, ids=["64x64", "128x128"])
def test_k20_reduce_is_the_ordered_sum_of_its_partials(shape, with_d):
    B, C, K, H, W = shape
    x, g3, gd, outs = _k20_case(B, C, K, H, W, with_d)
    dw3, dwd, ws = outs[0]
    nk, nc = K // 64, C // 64
    ntiles = B * (H // 2) * ((W // 2 + 31) // 32)
    S = min(512 // (nk * nc), ntiles)
    assert S >= 9 and S % 16 != 0 and (W // 2) % 32 != 0
    part = ws.view(nk, nc, S, 10, 64, 64)                       # [pair][slice][tap][k][c]
    tot = _seq_sum(part.permute(2, 0, 1, 3, 4, 5))               # slices in order
    tot = tot.permute(2, 0, 3, 1, 4).reshape(10, K, C)           # [tap][k][c]
    assert torch.isfinite(dw3).all()
    assert torch.equal(dw3, tot[:9].permute(1, 2, 0).reshape(K, C, 3, 3))
    if with_d:
        assert torch.equal(dwd, tot[9])
    assert torch.equal(outs[1][0], dw3) and (not with_d or torch.equal(outs[1][1], dwd)), "a second call must agree bit for bit"


@pytest.mark.parametrize("with_d", [True, False], ids=["shortcut", "3x3-only"])
def test_k20_small_shape_vs_fp64(with_d):
    B, C, K, H, W = K20_SHAPES[0]
    x, g3, gd, outs = _k20_case(B, C, K, H, W, with_d)
    dw3, dwd, _ = outs[0]
    px = (H // 2) * (W // 2)
    chain = B * px / 18 + 18                                    # tests/test_gpu_conv_anchor.py: _wrw_chain(pixels, parts)
    w3 = torch.zeros(K, C, 3, 3, device="cuda")
    ref3 = torch.nn.grad.conv2d_weight(x.double(), (K, C, 3, 3), g3.double(), 2, 1)
    lib3 = torch.ops.aten.convolution_backward(g3, x, w3, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1]
    _bound("K20 small 3x3/2 weight gradient", _rel(dw3, ref3), _rel(lib3, ref3), chain=chain)
    if with_d:
        wd = torch.zeros(K, C, 1, 1, device="cuda")
        refd = torch.nn.grad.conv2d_weight(x.double(), (K, C, 1, 1), gd.double(), 2, 0)
        libd = torch.ops.aten.convolution_backward(gd, x, wd, None, [2, 2], [0, 0], [1, 1], False, [0, 0], 1, [False, True, False])[1]
        _bound("K20 small 1x1/2 weight gradient", _rel(dwd.view(K, C, 1, 1), refd), _rel(libd, refd), chain=chain)


# ---- K16 ----------------------------------------------------------------------------------------------------------------------

# (B, H, W, pad), tiles at C = 16 / 32, all with a ragged last row and column of tiles: 18 / 36 (chains of 4-5 / 9 per group);
# 168 / 312 (chains of 42 / 78)
K16_SHAPES = [(2, 21, 130, 1), (6, 51, 250, 0)]


def _k16_case(B, C, H, W, pad):
    N, lib = _N()
    g0 = torch.Generator().manual_seed(7 + C + W)
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    x = torch.randn(B, C, H, W, generator=g0).cuda()
    g = (torch.randn(B, 16, Ho, Wo, generator=g0) / (Ho * Wo) ** 0.5).cuda()
    n = lib.dmh_conv3x3_small_wrw_partials_size(C)
    assert n > 0
    outs = []
    for _ in range(2):
        buf, ws = _workspace(n)
        gw = torch.full((16, C, 3, 3), float("nan"), device="cuda")
        gb = torch.full((16,), float("nan"), device="cuda")
        N.check(lib.dmh_conv3x3_small_wrw(N.ptr(x), N.ptr(g), B, C, H, W, pad, N.ptr(ws), N.ptr(gw), N.ptr(gb), N.stream()))
        torch.cuda.synchronize()
        assert _guard_intact(buf, n)
        outs.append((gw, gb, ws))
    return x, g, outs


@pytest.mark.parametrize("C", [16, 32])
@pytest.mark.parametrize("shape", K16_SHAPES, ids=["small", "full-batch"])
def test_k16_reduce_is_the_ordered_sum_of_its_partials(shape, C):
    B, H, W, pad = shape
    x, g, outs = _k16_case(B, C, H, W, pad)
    gw, gb, ws = outs[0]
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    TR = 8 if C == 16 else 4                                    # csrc/small_wrw.hip: launch<1, 8> / launch<2, 4>, TW = 64
    nwg = min(B * ((Ho + TR - 1) // TR) * ((Wo + 63) // 64), 512)
    assert nwg >= 9 and (nwg // 4) % 32 != 0 and Ho % TR != 0 and Wo % 64 != 0
    P = (C // 16) * 2304 + 64
    part = ws.view(512, P)[:nwg]
    assert torch.isfinite(part).all() and torch.isnan(ws.view(512, P)[nwg:]).all()
    bias = part[:, P - 64:]
    bias = (bias[:, 0:16] + bias[:, 16:32]) + (bias[:, 32:48] + bias[:, 48:64])
    r = [_seq_sum(part[grp::4, :P - 64]) for grp in range(4)]   # group g: partials g, g + 4, ...
    rb = [_seq_sum(bias[grp::4]) for grp in range(4)]
    v = (r[0] + r[1]) + (r[2] + r[3])
    vb = (rb[0] + rb[1]) + (rb[2] + rb[3])
    # element ((cb * 9 + tap) * 4 + (k & 3)) * 64 + 16 * (k >> 2) + (c & 15)
    want = v.view(C // 16, 9, 4, 4, 16).permute(3, 2, 0, 4, 1).reshape(16, C, 3, 3)
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all()
    assert torch.equal(gw, want)
    assert torch.equal(gb, vb)
    assert torch.equal(outs[1][0], gw) and torch.equal(outs[1][1], gb), "a second call must agree bit for bit"


@pytest.mark.parametrize("C", [16, 32])
def test_k16_small_shape_vs_fp64(C):
    B, H, W, pad = K16_SHAPES[0]
    x, g, outs = _k16_case(B, C, H, W, pad)
    gw, gb, _ = outs[0]
    ref = torch.nn.grad.conv2d_weight(x.double(), (16, C, 3, 3), g.double(), 1, pad)
    w = torch.zeros(16, C, 3, 3, device="cuda")
    lib = torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [pad, pad], [1, 1], False, [0, 0], 1, [False, True, False])[1]
    _bound("K16 small %d->16 weight gradient" % C, _rel(gw, ref), _rel(lib, ref))
    refb = g.double().sum((0, 2, 3))
    _bound("K16 small %d->16 bias gradient" % C, _rel(gb, refb), _rel(g.sum((0, 2, 3)), refb))


# ---- K21 ----------------------------------------------------------------------------------------------------------------------

# 30 / 70 tiles of 4 x 32 output pixels, ragged in both directions: 120 / 280 partials, eight ranges of 15 / 35
@pytest.mark.parametrize("shape", [(3, 38, 72), (7, 38, 72)], ids=["ranges-of-15", "ranges-of-35"])
def test_k21_reduce_is_the_ordered_sum_of_its_partials(shape):
    N, lib = _N()
    B, H, W = shape
    g0 = torch.Generator().manual_seed(9 + B)
    x = torch.rand(B, 3, H, W, generator=g0).cuda()
    Ho, Wo = H // 2, W // 2
    g = (torch.randn(B, 64, Ho, Wo, generator=g0) / (Ho * Wo) ** 0.5).cuda()
    n = lib.dmh_stem_wrw_workspace_size(B, H, W)
    ntiles = B * ((Ho + 3) // 4) * ((Wo + 31) // 32)            # csrc/stem_wrw.hip: TR = 4, TC = 32
    nparts = 4 * min(ntiles, 512)
    assert n == nparts * 10240 and nparts // 8 >= 9 and (nparts // 8) % 32 != 0 and Ho % 4 != 0 and Wo % 32 != 0
    outs = []
    for _ in range(2):
        buf, ws = _workspace(n)
        dw = torch.full((64, 3, 7, 7), float("nan"), device="cuda")
        N.check(lib.dmh_stem_wrw(N.ptr(x), N.ptr(g), B, H, W, 0.45, 0.225, N.ptr(ws), N.ptr(dw), N.stream()))
        torch.cuda.synchronize()
        assert _guard_intact(buf, n)
        outs.append((dw, ws))
    dw, ws = outs[0]
    part = ws.view(nparts, 2, 5, 32, 32)                        # [partial][k half][tap block][k & 31][tap & 31]
    tot = None
    for ch in range(8):                                         # the eight ranges, then their sums in order
        r = _seq_sum(part[nparts * ch // 8:nparts * (ch + 1) // 8])
        tot = r if tot is None else tot + r
    want = tot.permute(0, 2, 1, 3).reshape(64, 160)[:, :147].reshape(64, 3, 7, 7)
    assert torch.isfinite(dw).all()
    assert torch.equal(dw, want)
    assert torch.equal(outs[1][0], dw), "a second call must agree bit for bit"


# ---- K18 ----------------------------------------------------------------------------------------------------------------------

# (B, C, K, H, W): 20 slices (16 + 4) of a 64 x 64 and a 32 x 96 block; two pairs side by side; 60 slices (32 + 16 + 8 + 4)
K18_SHAPES = [(2, 64, 64, 12, 20), (2, 96, 32, 12, 20), (2, 128, 64, 12, 20), (4, 64, 64, 12, 36)]


@pytest.mark.parametrize("shape", K18_SHAPES, ids=["64-64", "96-32", "128-64", "64-64-60-slices"])
def test_k18_vs_fp64_and_twice(shape):
    N, lib = _N()
    B, C, K, H, W = shape
    g0 = torch.Generator().manual_seed(11 + C + W)
    x = torch.randn(B, C, H, W, generator=g0).cuda()
    Ho, Wo = H - 2, W - 2
    dy = (torch.randn(B, K, Ho, Wo, generator=g0) / (Ho * Wo) ** 0.5).cuda()
    n = lib.dmh_wino_wrw_workspace_size(B, C, K, H, W, 0)
    assert n > 0
    outs = []
    for _ in range(2):
        buf, ws = _workspace(n)
        dw = torch.full((K, C, 3, 3), float("nan"), device="cuda")
        N.check(lib.dmh_wino_wrw(N.ptr(x), N.ptr(dy), B, C, K, H, W, 0, N.ptr(ws), N.ptr(dw), N.stream()))
        torch.cuda.synchronize()
        assert _guard_intact(buf, n)
        outs.append(dw)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), "a second call must agree bit for bit"
    ref = torch.nn.grad.conv2d_weight(x.double(), (K, C, 3, 3), dy.double(), 1, 0)
    w = torch.zeros(K, C, 3, 3, device="cuda")
    gl = torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [False, True, False])[1]
    _bound("K18 %d->%d @%dx%d weight gradient" % (C, K, H, W), _rel(outs[0], ref), _rel(gl, ref))
