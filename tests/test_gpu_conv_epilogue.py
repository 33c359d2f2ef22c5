"""fp64-anchored checks of K10's fused epilogue (csrc/wino_conv.hip: wino_conv_kernel<TRW, FLAT, EPI = true, SK> and, under
stream-K, wino_sk_fixup_kernel), which the encoder's eval-mode block nodes (ops._BasicBlockEval, ops._DownBlockEval) run on
every attack step: BatchNorm shift (the bias), identity addend, ReLU, and in the backward pass a ReLU MASK read from a saved
activation (relu flag bit 1).

The reference is float64 (the same bound as tests/test_gpu_conv_anchor.py), with no ReLU-kink allowance:
  * forward: ReLU is 1-Lipschitz, |relu(a) - relu(b)| <= |a - b|: the plain float64 chain is a valid reference;
  * backward: the mask is a tensor both sides are given (in the block tests: the HIP forward's own activations), so the float64
    chain masks exactly the same elements.

Beside the tolerance, the epilogue is isolated bit for bit: the plain K10 launch of the same filter image and shift, followed by
the epilogue in torch fp32 ops, must equal the fused launch wherever the library reports the same decomposition for both.  Each
case pins the path it takes (tile form, stream-K) through dmh_wino_conv3x3_plan, so that a later change of thresholds or of the
cost model cannot move a case onto another path unnoticed.

One known gap (see WHOLE_ITEM_CHAIN below): a whole-item launch sums each transformed output's C products in ONE MFMA
accumulator.  At C = 512 and batch 2 (the no-workspace launches of "4x16 stream-K" and "FLAT stream-K pad2") that chain's
rounding, 0.5 sqrt(C) 2^-24 = 6.7e-7, is about 3x what the library measures there (2.2e-7: at this small batch it does not take
its F(2,3) Winograd, which measures 6.6e-7 at batch 12).  The network takes these shapes in the stream-K form (ratio 1.2); the
whole-item form of a 512-channel layer runs only under the DMH_WINO_SK=0 switch.  Such launches are held to the chain estimate
and reported; every other launch meets the library bound.

The file runs in about 9 s on one MI355X.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.util import fp64_bound, rel_fp64

pytestmark = pytest.mark.gpu

FORMS = {0: "2x32", 1: "4x16", 2: "FLAT"}
SK_SLOT = 16384         # floats of one partial item (csrc/wino_conv.hip SK_SLOT)
WS_FLOATS = 2 * 256 * SK_SLOT       # the plan queries below assume 256 CUs (MI355X); test_case_list_covers_every_epilogue_cell checks

# (name, B, C, K, H, W, pad, tile form, stream-K with a workspace): INPUT sizes of the launch.  Without a workspace every case runs
# whole items of the same form.  Ragged rows / columns of the tile regions and pads 0 / 1 / 2 are spread over the forms; C = 40 / 56
# (an odd number of 8-channel chunks) keeps the PLAIN launch of a whole-item case unsplit, so that it can be compared bit for bit.
CASES = [("2x32 whole", 12, 64, 64, 16, 64, 1, 0, False),
         ("2x32 whole ragged pad2", 4, 40, 64, 16, 58, 2, 0, False),
         ("2x32 stream-K K96 ragged", 2, 128, 96, 16, 40, 1, 0, True),
         ("2x32 stream-K ragged pad0", 2, 256, 128, 20, 62, 0, 0, True),
         ("4x16 whole", 12, 64, 64, 8, 32, 1, 1, False),
         ("4x16 whole ragged pad2", 3, 40, 64, 12, 20, 2, 1, False),
         ("4x16 stream-K", 2, 512, 512, 8, 32, 1, 1, True),
         ("4x16 stream-K ragged", 1, 256, 256, 8, 66, 1, 1, True),
         ("FLAT stream-K layer4 attack", 12, 512, 512, 10, 32, 1, 2, True),
         ("FLAT stream-K ragged rows", 3, 128, 128, 10, 32, 1, 2, True),
         ("FLAT stream-K ragged pad0", 6, 256, 256, 6, 24, 0, 2, True),
         ("FLAT stream-K pad2", 2, 512, 512, 8, 30, 2, 2, True),
         ("FLAT whole ragged rows", 5, 56, 64, 10, 32, 1, 2, False)]

# epilogue modes: (relu flag, bias, tensor kind, filter direction)
MODES = {"a shift+relu": (1, True, None, False),          # conv1 of a block
         "b shift+res+relu": (1, True, "res", False),     # conv2 of a block
         "c mask": (2, False, "mask", True),              # conv2's backward-data, masked by the saved out1
         "d res": (0, False, "res", True)}                # conv1's backward-data + the identity branch's gradient


def _lib():
    from depthmodelhardening_amd import _native as N
    return N, N.lib()


def _plan(B, C, K, H, W, pad, epilogue, ws_floats):
    _, lib = _lib()
    p = lib.dmh_wino_conv3x3_plan(B, C, K, H, W, pad, epilogue, ws_floats)
    assert p >= 0, ("the kernel does not take", B, C, K, H, W, pad)
    return {"sk": bool(p & 1), "split": bool(p & 2), "form": (p >> 2) & 3, "items": p >> 8}


def _same_decomposition(p_epi, p_plain):
    """The fused and the plain launch sum every output in the same order: whole items without channel split, or stream-K both
    (same units, same workgroup count: the grid depends on the shape alone)."""
    return not p_plain["split"] and p_epi["sk"] == p_plain["sk"] and p_epi["form"] == p_plain["form"]


def test_case_list_covers_every_epilogue_cell():
    """All six EPI cells -- tile form {2x32, 4x16, FLAT} x {whole items, stream-K} -- are reached, each with at least one
    bit-for-bit comparison with the plain launch.  (Every case runs all four epilogue modes: the mode loop of
    test_fused_epilogue_vs_fp64 over MODES.)"""
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256, "case paths were chosen for 256 CUs"
    cells = {}
    for name, B, C, K, H, W, pad, form, sk in CASES:
        for ws in (WS_FLOATS, 0):
            p = _plan(B, C, K, H, W, pad, 1, ws)
            q = _plan(B, C, K, H, W, pad, 0, ws)
            cell = cells.setdefault((p["form"], p["sk"]), {"cases": [], "bitwise": 0})
            cell["cases"].append("%s%s" % (name, "" if ws else " (no workspace)"))
            cell["bitwise"] += _same_decomposition(p, q)
    print("\nEPI cell           bitwise  cases")
    for (form, sk), c in sorted(cells.items()):
        print("%-5s %-12s %7d  %s" % (FORMS[form], "stream-K" if sk else "whole items", c["bitwise"], "; ".join(c["cases"])))
    for form in FORMS:
        for sk in (False, True):
            c = cells.get((form, sk))
            assert c is not None, ("EPI cell not reached", FORMS[form], sk)
            assert c["bitwise"] >= 1, (FORMS[form], sk, c)


def _launch(fn_ws, x, U, bias, res, relu, B, C, K, H, W, pad, ws):
    """One launch into a NaN-filled output (an element the kernel does not write stays NaN)."""
    N, lib = _lib()
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    y = torch.full((B, K, Ho, Wo), float("nan"), device="cuda")
    if fn_ws == "act":
        args = (N.ptr(x), N.ptr(U), N.ptr(bias), N.ptr(res), relu, B, C, K, H, W, pad, N.ptr(y))
        rc = (lib.dmh_wino_conv3x3_act_ws(*args, N.ptr(ws), ws.numel(), N.stream()) if ws is not None
              else lib.dmh_wino_conv3x3_act(*args, N.stream()))
    else:
        args = (N.ptr(x), N.ptr(U), N.ptr(bias), B, C, K, H, W, pad, N.ptr(y))
        rc = (lib.dmh_wino_conv3x3_ws(*args, N.ptr(ws), ws.numel(), N.stream()) if ws is not None
              else lib.dmh_wino_conv3x3(*args, N.stream()))
    N.check(rc)
    return y


def _epilogue(y, bias, res, relu):
    """The epilogue in torch fp32 ops, in the kernel's order: (+ shift was added by the plain launch), addend or mask, ReLU."""
    if res is not None:
        y = torch.where(res > 0, y, torch.zeros_like(y)) if relu & 2 else y + res
    return y.clamp_min(0) if relu & 1 else y


def _epilogue64(y64, shift, res, relu):
    if shift is not None:
        y64 = y64 + shift.double().view(1, -1, 1, 1)
    if res is not None:
        y64 = torch.where(res > 0, y64, torch.zeros_like(y64)) if relu & 2 else y64 + res.double()
    return y64.clamp_min(0) if relu & 1 else y64


# The known gap of whole items (module docstring): where a whole-item launch exceeds the library bound it is held to its single
# accumulation chain's random-walk estimate 0.5 sqrt(C) 2^-24 instead, with a margin of 1.2 (measured at C = 512: 0.64-1.04 of the
# estimate, the mask mode highest; a residual dilutes the relative error), and printed as such.  Only launches with C >= WHOLE_ITEM_CHAIN may use it: at C <= 256 whole items meet the library
# bound (ratios 0.99-1.59 with the 1e-7 floor), and a regression there fails.
WHOLE_ITEM_CHAIN = 512


def _whole_item_bound(name, e_hip, e_lib, C):
    if e_hip <= 1.5 * e_lib + 1e-7 or C < WHOLE_ITEM_CHAIN:
        fp64_bound(name, e_hip, e_lib)
        return
    print("KNOWN GAP %s: %.2f x the library; chain estimate %.3g" % (name, e_hip / e_lib, 0.5 * C ** 0.5 * 2.0 ** -24))
    fp64_bound(name, e_hip, e_lib, chain=C, chain_margin=1.2)


@pytest.mark.parametrize("case", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_fused_epilogue_vs_fp64(case):
    """Every epilogue mode through dmh_wino_conv3x3_act_ws (the case's path, pinned) and dmh_wino_conv3x3_act (whole items):
    float64 bound, bit for bit against the plain launch + torch epilogue, stream-K run twice bit for bit."""
    N, lib = _lib()
    name, B, C, K, H, W, pad, form, sk = case
    p_ws, p_0 = _plan(B, C, K, H, W, pad, 1, WS_FLOATS), _plan(B, C, K, H, W, pad, 1, 0)
    assert (p_ws["form"], p_ws["sk"]) == (form, sk), (name, p_ws)
    assert (p_0["form"], p_0["sk"], p_0["split"], p_ws["split"]) == (form, False, False, False), (name, p_0)
    same_ws = _same_decomposition(p_ws, _plan(B, C, K, H, W, pad, 0, WS_FLOATS))
    same_0 = _same_decomposition(p_0, _plan(B, C, K, H, W, pad, 0, 0))
    ws = torch.empty(WS_FLOATS, device="cuda")
    g = torch.Generator().manual_seed(B * 1000 + C + H)
    x = torch.randn(B, C, H, W, generator=g).cuda()
    w = (torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).cuda()           # forward filter [K, C]
    wb = (torch.randn(C, K, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).cuda()          # a forward K -> C filter, run backward
    sc_f = (torch.rand(K, generator=g) + 0.5).cuda()            # BatchNorm scale of the forward output channels
    sc_b = (torch.rand(C, generator=g) + 0.5).cuda()            # of wb's output channels: the INPUT channels of its backward pass
    shift = (torch.randn(K, generator=g) * 0.5).cuda()
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    res = (torch.randn(B, K, Ho, Wo, generator=g) * 1.5).cuda()         # the order of the convolution output
    mask = torch.relu(torch.randn(B, K, Ho, Wo, generator=g)).cuda()    # a saved ReLU output: half of it exactly zero
    filt = {}
    for backward in (False, True):
        wsrc, scale = (wb, sc_b) if backward else (w, sc_f)
        U = torch.empty(lib.dmh_wino_weight_size(K, C), device="cuda")
        N.check(lib.dmh_wino_weight_transform_scaled(N.ptr(wsrc), wsrc.shape[0], wsrc.shape[1], int(backward), N.ptr(scale),
                                                     N.ptr(U), N.stream()))
        # the effective filter of the pass [K, C, 3, 3]: forward w * scale[k]; backward flipped, transposed, scale[c]
        weff = ((wb * sc_b.view(-1, 1, 1, 1)).flip(2, 3).transpose(0, 1) if backward else w * sc_f.view(-1, 1, 1, 1)).contiguous()
        y64 = F.conv2d(x.double(), (wb.double() * sc_b.double().view(-1, 1, 1, 1)).flip(2, 3).transpose(0, 1) if backward
                       else w.double() * sc_f.double().view(-1, 1, 1, 1), None, 1, pad)
        filt[backward] = (U, weff.contiguous(), y64)
    for mode, (relu, use_bias, kind, backward) in MODES.items():
        U, weff, y64 = filt[backward]
        bias = shift if use_bias else None
        t = {"res": res, "mask": mask, None: None}[kind]
        ref64 = _epilogue64(y64, bias, t, relu)
        lib32 = _epilogue(torch.conv2d(x, weff, bias, 1, pad), None, t, relu)
        e_lib = rel_fp64(lib32, ref64)
        y_sk = _launch("act", x, U, bias, t, relu, B, C, K, H, W, pad, ws)
        y_whole = _launch("act", x, U, bias, t, relu, B, C, K, H, W, pad, None)
        tag = "%s [%s]" % (name, mode)
        if sk:
            fp64_bound(tag + " stream-K", rel_fp64(y_sk, ref64), e_lib)
        else:
            _whole_item_bound(tag + " ws", rel_fp64(y_sk, ref64), e_lib, C)
        _whole_item_bound(tag + " whole items", rel_fp64(y_whole, ref64), e_lib, C)
        if sk:
            assert torch.equal(y_sk, _launch("act", x, U, bias, t, relu, B, C, K, H, W, pad, ws)), (tag, "stream-K run twice")
        else:
            assert torch.equal(y_sk, y_whole), (tag, "the same whole-item launch with and without a workspace")
        # the epilogue isolated: the plain launch (bias = shift) + the epilogue in torch fp32 ops
        if same_ws:
            plain = _epilogue(_launch("plain", x, U, bias, None, 0, B, C, K, H, W, pad, ws), None, t, relu)
            assert torch.equal(plain, y_sk), (tag, "fused vs plain + epilogue (workspace)", float((plain - y_sk).abs().max()))
        if same_0:
            plain = _epilogue(_launch("plain", x, U, bias, None, 0, B, C, K, H, W, pad, None), None, t, relu)
            assert torch.equal(plain, y_whole), (tag, "fused vs plain + epilogue (whole items)", float((plain - y_whole).abs().max()))


@pytest.mark.parametrize("shape", [(12, 512, 10, 32), (2, 256, 20, 64)], ids=["layer4_attack", "layer3_two_scenes"])
def test_conv3x3_bn_act_forward_and_backward_data_vs_fp64(shape):
    """ops.conv3x3_bn_act (the op-level entry: _ConvBnAct) with a residual and ReLU: forward, and the backward-data pass (K9 mask
    by the op's own output, then K10 on the scaled flipped filter) against float64 conditioned on that output."""
    from depthmodelhardening_amd import ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(C + B)
    x = torch.randn(B, C, H, W, generator=g).cuda()
    w = (torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).cuda()
    scale, shift = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.5).cuda()
    res = (torch.randn(B, C, H, W, generator=g) * 1.5).cuda()
    gy = torch.randn(B, C, H, W, generator=g).cuda()
    assert ops._wino_ok(B, C, C, H, W, allow_split=False, allow_sk=True), "the shape must take the fused K10 launch"
    xg = x.clone().requires_grad_(True)
    with ops.frozen_weights():
        y = ops.conv3x3_bn_act(xg, w, scale, shift, res, True, 1)
        assert type(y.grad_fn).__name__.startswith("_ConvBnAct")
        (gx,) = torch.autograd.grad(y, xg, gy)
    w64 = w.double() * scale.double().view(-1, 1, 1, 1)
    y64 = (F.conv2d(x.double(), w64, None, 1, 1) + shift.double().view(1, -1, 1, 1) + res.double()).clamp_min(0)
    ws = w * scale.view(-1, 1, 1, 1)
    y_lib = (torch.conv2d(x, ws, shift, 1, 1) + res).clamp_min(0)
    fp64_bound("conv3x3_bn_act %s forward" % (shape,), rel_fp64(y, y64), rel_fp64(y_lib, y64))
    g_pre = gy * (y > 0)                                    # the op's own mask: the same on every side
    gx64 = F.conv_transpose2d(g_pre.double(), w64, None, 1, 1)
    gx_lib = torch.ops.aten.convolution_backward(g_pre, x, ws, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                 [True, False, False])[0]
    fp64_bound("conv3x3_bn_act %s backward-data" % (shape,), rel_fp64(gx, gx64), rel_fp64(gx_lib, gx64))


# ---- the block nodes against float64 ---------------------------------------------------------------------------------------------

def _bn_params(bns):
    with torch.no_grad():
        for bn in bns:
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)


def _aff(bn):
    sc = (bn.weight * torch.rsqrt(bn.running_var + bn.eps)).detach()
    return sc, (bn.bias - bn.running_mean * sc).detach()


def _block_pre(blk, x, dtype):
    """The module path of a BasicBlock in eval() as plain ATen ops in ``dtype`` (the encoder's own module path runs ops.conv3x3 /
    K15): the pre-activations (pre1, pre2) of its two ReLUs."""
    def bn(t, m):
        c = lambda p: p.detach().to(dtype)      # noqa: E731
        return F.batch_norm(t, c(m.running_mean), c(m.running_var), c(m.weight), c(m.bias), False, 0.0, m.eps)

    def conv(m, t):
        return F.conv2d(t, m.weight.detach().to(dtype), None, m.stride, m.padding)
    x = x.detach().to(dtype)
    pre1 = bn(conv(blk.conv1, x), blk.bn1)
    idt = x if blk.downsample is None else bn(conv(blk.downsample[0], x), blk.downsample[1])
    return pre1, bn(conv(blk.conv2, pre1.clamp_min(0)), blk.bn2) + idt


def _masks_agree(name, act_hip, pre64, ulps=4):
    """[act_hip > 0] == [pre64 > 0] except where |pre64| is within ``ulps`` fp32 ulps of the layer's scale (max |pre64|, ~5): a
    forward that clamps the wrong element fails here.  Measured: the farthest flip lies 0.41 ulps from zero (8 flips in all
    the block shapes); the block forwards' rel-L2 <= 2.5e-7 bounds an element's error at a few ulps of the scale."""
    scale = float(pre64.abs().max())
    ulp = 2.0 ** -23 * scale
    near = pre64.abs() <= ulps * ulp
    differ = (act_hip > 0) != (pre64 > 0)
    worst = float(pre64.abs()[differ].max()) / ulp if bool(differ.any()) else 0.0
    print("%-44s mask flips %d, the farthest at %.2f ulps of %.3g (allowed %d; %d elements that close)" % (
        name, int(differ.sum()), worst, scale, ulps, int(near.sum())))
    assert not bool((differ & ~near).any()), (name, int((differ & ~near).sum()))


# (B, C, H, W): the shapes of test_gpu_trainer.py::test_basic_block_eval_node_vs_module_path that take the node
BASIC = [(12, 64, 80, 256), (12, 128, 40, 128), (12, 512, 10, 32), (2, 256, 20, 64), (2, 512, 10, 32)]


@pytest.mark.parametrize("shape", BASIC, ids=["x".join(map(str, s)) for s in BASIC])
def test_basic_block_node_vs_fp64(shape):
    """ops._BasicBlockEval (BasicBlock.forward_fused inside an attack): forward against the float64 module path; backward
    against a float64 chain that takes its ReLU masks from the HIP forward (y, and out1 from the node's saved tensors -- the
    same K10 launch recomputed, bit for bit)."""
    from depthmodelhardening_amd import ops
    from depthmodelhardening_amd.networks.resnet_encoder import BasicBlock
    B, C, H, W = shape
    torch.manual_seed(B * 7 + C)
    blk = BasicBlock(C, C).cuda().eval()
    _bn_params((blk.bn1, blk.bn2))
    x = torch.randn(B, C, H, W, device="cuda").requires_grad_(True)
    gy = torch.randn(B, C, H, W, device="cuda")
    aff = {bn: _aff(bn) for bn in (blk.bn1, blk.bn2)}
    with ops.frozen_weights():
        y = blk.forward_fused(x, aff)
        assert type(y.grad_fn).__name__.startswith("_BasicBlockEval")
        out1 = y.grad_fn.saved_tensors[0]
        with torch.no_grad():
            assert torch.equal(out1, ops.conv3x3_bn_act(x.detach(), blk.conv1.weight, *aff[blk.bn1], None, True, 1))
        (gx,) = torch.autograd.grad(y, x, gy)
    pre1, pre2 = _block_pre(blk, x, torch.float64)
    y64, y_lib = pre2.clamp_min(0), _block_pre(blk, x, torch.float32)[1].clamp_min(0)
    fp64_bound("basic block %s forward" % (shape,), rel_fp64(y, y64), rel_fp64(y_lib, y64), factor=2.0)
    _masks_agree("basic block %s out1" % (shape,), out1, pre1)
    _masks_agree("basic block %s y" % (shape,), y, pre2)
    # backward with the HIP forward's masks
    s1, s2 = aff[blk.bn1][0], aff[blk.bn2][0]
    g2 = gy * (y > 0)
    w1s, w2s = blk.conv1.weight.detach() * s1.view(-1, 1, 1, 1), blk.conv2.weight.detach() * s2.view(-1, 1, 1, 1)
    g1_64 = F.conv_transpose2d(g2.double(), w2s.double(), None, 1, 1) * (out1 > 0)
    gx64 = F.conv_transpose2d(g1_64, w1s.double(), None, 1, 1) + g2.double()
    g1_lib = F.conv_transpose2d(g2, w2s, None, 1, 1) * (out1 > 0)
    gx_lib = F.conv_transpose2d(g1_lib, w1s, None, 1, 1) + g2
    fp64_bound("basic block %s backward" % (shape,), rel_fp64(gx, gx64), rel_fp64(gx_lib, gx64), factor=2.0)


DOWN = [(12, 64, 128, 80, 256), (12, 128, 256, 40, 128)]


@pytest.mark.parametrize("shape", DOWN, ids=["x".join(map(str, s)) for s in DOWN])
def test_down_block_node_vs_fp64(shape):
    """ops._DownBlockEval: K15 (3x3 / 2 and 1x1 / 2 with BatchNorm, ReLU) + K10 (shift, identity, ReLU; backward: mask flag 2)
    against float64 the same way."""
    from depthmodelhardening_amd import ops
    from depthmodelhardening_amd.networks.resnet_encoder import BasicBlock
    import torch.nn as nn
    B, Ci, Co, H, W = shape
    torch.manual_seed(Ci + 3)
    down = nn.Sequential(nn.Conv2d(Ci, Co, 1, 2, bias=False), nn.BatchNorm2d(Co))
    blk = BasicBlock(Ci, Co, 2, down).cuda().eval()
    bnd = blk.downsample[1]
    _bn_params((blk.bn1, blk.bn2, bnd))
    x = torch.randn(B, Ci, H, W, device="cuda").requires_grad_(True)
    gy = torch.randn(B, Co, H // 2, W // 2, device="cuda")
    aff = {bn: _aff(bn) for bn in (blk.bn1, blk.bn2, bnd)}
    with ops.frozen_weights():
        y = blk.forward_fused(x, aff)
        assert type(y.grad_fn).__name__.startswith("_DownBlockEval")
        out1 = y.grad_fn.saved_tensors[0]
        (gx,) = torch.autograd.grad(y, x, gy)
    w3, wd, w2 = (m.weight.detach() for m in (blk.conv1, blk.downsample[0], blk.conv2))
    pre1, pre2 = _block_pre(blk, x, torch.float64)
    y64, y_lib = pre2.clamp_min(0), _block_pre(blk, x, torch.float32)[1].clamp_min(0)
    # out1 comes from K15, a direct MFMA kernel with one accumulation chain of 9 x Ci products per output (as in
    # tests/test_gpu_conv_anchor.py test_strided_block_entry_vs_fp64): that chain's rounding is allowed beside the bound
    fp64_bound("down block %s forward" % (shape,), rel_fp64(y, y64), rel_fp64(y_lib, y64), chain=9 * Ci, factor=2.0)
    _masks_agree("down block %s out1" % (shape,), out1, pre1)
    _masks_agree("down block %s y" % (shape,), y, pre2)
    s1, sd, s2 = aff[blk.bn1][0], aff[bnd][0], aff[blk.bn2][0]
    w3s, wds, w2s = (w * s.view(-1, 1, 1, 1) for w, s in ((w3, s1), (wd, sd), (w2, s2)))
    g2 = gy * (y > 0)

    def chain(g2_, w3s_, wds_, w2s_):
        g1 = F.conv_transpose2d(g2_, w2s_, None, 1, 1) * (out1 > 0)
        return (F.conv_transpose2d(g1, w3s_, None, 2, 1, output_padding=1) +
                F.conv_transpose2d(g2_, wds_, None, 2, 0, output_padding=1))
    gx64 = chain(g2.double(), w3s.double(), wds.double(), w2s.double())
    gx_lib = chain(g2, w3s, wds, w2s)
    # K15's backward is a direct MFMA kernel: one accumulation chain of 9 x Co / 4 + Co / 4 products per input element (see
    # tests/test_gpu_conv_anchor.py test_strided_block_entry_vs_fp64), allowed beside the library-relative bound
    fp64_bound("down block %s backward" % (shape,), rel_fp64(gx, gx64), rel_fp64(gx_lib, gx64), chain=10 * Co // 4, factor=2.0)
