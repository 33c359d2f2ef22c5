"""ManyDepth hardening on the GPU: K36 (``ops.reduce_conv_degenerate``), the fused train path of ``ResnetEncoderMatching`` and
``Trainer`` with ``--depth_net manydepth``.

Yardsticks: float64 (the definition ``ops.reduce_conv_degenerate_host`` / the CPU module path in float64), with an fp32 library
evaluation of the same arithmetic as the measure of what fp32 can do (tests/util.fp64_bound, the factors of
tests/test_gpu_conv_anchor.py), and for the bias gradient the element-wise rounding bound of tests/util.assert_round_bound with
the number of roundings csrc/reduce_node.hip's header derives."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

from tests import cost_volume_ref as R
from tests import manydepth_train_ref as T
from tests.util import assert_close_frac, assert_round_bound, fp64_bound, rel_fp64, rel_l2

pytestmark = pytest.mark.gpu

D = 96


def _smallest(ok, batches=(1, 2, 3), limit=128):
    """The (B, H, W) of fewest elements (then fewest images, rows) for which ok(B, 64, 64, H, W) holds."""
    cands = sorted((B * H * W, B, H, W) for B in batches for H in range(2, limit + 1, 2) for W in range(2, limit + 1, 2))
    for _, B, H, W in cands:
        if ok(B, 64, 64, H, W):
            return B, 64, H, W
    raise AssertionError("no shape up to %d x %d is taken" % (limit, limit))


NODE_SHAPES = {"2x64x12x24": (2, 64, 12, 24), "1x64x6x10": (1, 64, 6, 10), "3x64x7x9": (3, 64, 7, 9),
               "smallest_wino_ok": "_wino_ok", "smallest_epilogue_ok": "_reduce_act_ok"}      # the last two: found by calling the rule


def _node_shape(name):
    from depthmodelhardening_amd import ops
    shape = NODE_SHAPES[name]
    return _smallest(getattr(ops, shape)) if isinstance(shape, str) else shape


def _wgrad64(x, g):
    xp = F.pad(x.double(), (1, 1, 1, 1))
    g64 = g.double()
    H, W = g.shape[2], g.shape[3]
    out = torch.empty(g.shape[1], x.shape[1], 3, 3, dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            out[:, :, ky, kx] = torch.einsum("bkyx,bcyx->kc", g64, xp[:, :, ky:ky + H, kx:kx + W])
    return out


def _node_case(shape, seed=5):
    B, Cc, H, W = shape
    gen = torch.Generator().manual_seed(seed + B * H * W)
    x = torch.randn(B, Cc, H, W, generator=gen).cuda()
    w = (torch.randn(64, Cc + D, 3, 3, generator=gen) * (2.0 / (9 * Cc)) ** 0.5).cuda()
    b = (torch.randn(64, generator=gen) * 0.1).cuda()
    g = torch.randn(B, 64, H, W, generator=gen).cuda()
    return x, w, b, g


def _run_node(x, w, b, g):
    from depthmodelhardening_amd import ops
    xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = ops.reduce_conv_degenerate(xs, ws, bs)
    return (y.detach(),) + torch.autograd.grad(y, (xs, ws, bs), g)


def test_node_shapes_cover_both_forward_forms():
    from depthmodelhardening_amd import ops
    shapes = [_node_shape(n) for n in NODE_SHAPES]
    print("K36 node shapes:", shapes)
    assert ops._wino_ok(*shapes[3][:2], 64, *shapes[3][2:]) and ops._reduce_act_ok(*shapes[4][:2], 64, *shapes[4][2:])
    assert not any(ops._wino_ok(B, C, 64, H, W) for B, C, H, W in shapes[:3])


@pytest.mark.parametrize("name", list(NODE_SHAPES))
def test_reduce_node_against_float64(name):
    from depthmodelhardening_amd import ops
    shape = _node_shape(name)
    B, Cc, H, W = shape
    x, w, b, g = _node_case(shape)
    wc = w[:, :Cc].contiguous()
    y, gx, gw, gb = _run_node(x, w, b, g)
    tag = "K36 %s%s " % (shape, " K10" if ops._wino_ok(*shape[:2], 64, H, W) else "")
    # forward
    y64 = ops.reduce_conv_degenerate_host(x.double(), w.double(), b.double())
    y_lib = torch.relu(torch.conv2d(x, wc, b, 1, 1))
    fp64_bound(tag + "forward", rel_fp64(y, y64), rel_fp64(y_lib, y64))
    # the mask pass: bit-equal to g * (y > 0) on the node's own output
    g_pre, part = ops.reduce_bwd_mask(g, y)
    assert torch.equal(g_pre, g * (y > 0)) and float((y > 0).float().mean()) > 0.2
    # bias gradient: element-wise, n_round roundings of partial sums bounded by S = sum |g_pre|
    n_round = ops.reduce_bwd_rounds(B, 64, H * W)
    S1 = 1 if H * W <= 1024 else -(-H * W // 1024)
    assert n_round == (B * -(-H * W // (min(S1, 64) * 1024)) + 12 if (H * W) % 4 == 0 else B * -(-H * W // (min(S1, 64) * 256)) + 10)
    assert_round_bound(tag + "bias gradient", gb, g_pre.double().sum((0, 2, 3)), g_pre.double().abs().sum((0, 2, 3)), n_round)
    # input gradient and weight gradient of the convolution on g_pre (K10 backward-data / K18 where they take the shape)
    gx64 = F.conv_transpose2d(g_pre.double(), wc.double(), None, 1, 1)
    gx_lib, gw_lib, _ = torch.ops.aten.convolution_backward(g_pre, x, wc, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [True, True, False])
    fp64_bound(tag + "backward-data", rel_fp64(gx, gx64), rel_fp64(gx_lib, gx64))
    gw64 = _wgrad64(x, g_pre)
    assert tuple(gw.shape) == (64, Cc + D, 3, 3) and gw.is_contiguous()
    fp64_bound(tag + "weight gradient", rel_fp64(gw[:, :Cc], gw64), rel_fp64(gw_lib, gw64))
    assert float(gw[:, Cc:].abs().max()) == 0.0 and not bool(torch.signbit(gw[:, Cc:]).any())
    # two runs: identical bits
    again = _run_node(x, w, b, g)
    for name, a, c in zip(("y", "g_x", "g_weight", "g_bias"), (y, gx, gw, gb), again):
        assert torch.equal(a, c), "%s differs between two runs (max %.3g)" % (name, float((a - c).abs().max()))
    # inside frozen_weights() no parameter gradient appears
    xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
    with ops.frozen_weights():
        yf = ops.reduce_conv_degenerate(xs, ws, bs)
        yf.backward(g)
    assert torch.equal(yf.detach(), y) and torch.equal(xs.grad, gx) and ws.grad is None and bs.grad is None


def test_reduce_node_refuses_what_it_does_not_take():
    from depthmodelhardening_amd import ops
    x, w, b, _ = _node_case((1, 64, 6, 10))
    for bad in ((x[:, :60], w, b), (x, w[:60], b[:60]), (x, w[:, :32], b), (x, w, None), (x.double(), w.double(), b.double())):
        with pytest.raises(RuntimeError):
            ops.reduce_conv_degenerate(*bad)


def test_registered_operator_passes_opcheck():
    from depthmodelhardening_amd import library, ops    # noqa: F401
    x, w, b, g = _node_case((1, 64, 6, 10))
    args = tuple(t.clone().requires_grad_(True) for t in (x, w, b))
    torch.library.opcheck(torch.ops.dmh.reduce_conv_degenerate, args)
    y = torch.ops.dmh.reduce_conv_degenerate(*args)
    ref = _run_node(x, w, b, g)
    assert all(torch.equal(a, c) for a, c in zip((y.detach(),) + torch.autograd.grad(y, args, g), ref))
    with ops.frozen_weights():
        y = torch.ops.dmh.reduce_conv_degenerate(*args)
        y.backward(g)
    assert torch.equal(args[0].grad, ref[1]) and args[1].grad is None and args[2].grad is None


# --------------------------------------------------------------------------------------------------------------- encoder
def _k10_frame(batch=2):
    """The smallest frame (multiples of 32, fewest pixels first) whose 1/4-size feature puts reduce_conv on K10."""
    from depthmodelhardening_amd import ops
    for _, H, W in sorted((H * W, H, W) for H in range(32, 513, 32) for W in range(32, 513, 32)):
        if ops._wino_ok(batch, 64, 64, H // 4, W // 4):
            return H, W
    raise AssertionError("no frame up to 512 x 512 puts reduce_conv on K10")


def _frames(B, H, W):
    gen = torch.Generator().manual_seed(H + W)
    yy, xx = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, indexing="ij")
    base = torch.stack([0.5 + 0.3 * torch.sin(7 * xx + 3 * yy + ph) + 0.15 * torch.cos(11 * yy * (1 + xx) + ph) for ph in (0.0, 0.7, 1.9)], 0)
    return (base.unsqueeze(0) + 0.05 * torch.randn(B, 3, H, W, generator=gen)).clamp(0, 1)


def _module_run(enc, x, dtype):
    """The CPU module path in ``dtype``: (features, the four gradients, layer0.1 statistics)."""
    enc = copy.deepcopy(enc).to(dtype)
    xin = {k: v.to(dtype) for k, v in x.items()}
    feats, grads = T.run(enc, xin, "none")
    bn = enc.layer0[1]
    return [f.detach() for f in feats], grads, (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))


@pytest.mark.parametrize("frame", ["64x128", "k10"])
def test_fused_train_path_against_the_cpu_module_path_in_float64(frame):
    from depthmodelhardening_amd import networks, ops
    H, W = (64, 128) if frame == "64x128" else _k10_frame()
    print("frame %d x %d, reduce_conv on K10: %s" % (H, W, ops._wino_ok(2, 64, 64, H // 4, W // 4)))
    assert ops._wino_ok(2, 64, 64, H // 4, W // 4) == (frame == "k10")
    enc = networks.ResnetEncoderMatching(18, False, input_height=H, input_width=W)
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict(R.formula_state_dict(shapes), strict=False)
    K, invK = R.intrinsics(W // 4, H // 4)
    x = dict(current=_frames(2, H, W), K=torch.from_numpy(K).expand(2, 4, 4), invK=torch.from_numpy(invK).expand(2, 4, 4))
    f64, g64, s64 = _module_run(enc, x, torch.float64)
    f32, g32, _ = _module_run(enc, x, torch.float32)
    dev = copy.deepcopy(enc).cuda()
    xd = {k: v.cuda() for k, v in x.items()}
    seen = []
    node = ops.reduce_conv_degenerate
    ops.reduce_conv_degenerate = lambda *a: (seen.append(1), node(*a))[1]       # the fused path is the one that ran
    # At these frame sizes layers 2 - 4 run the library's convolutions (the maps are too small for K10 / K15 / K18), whose default
    # solvers for such maps add with atomics: features 3 and 4 of two runs differ in the last bits on this path and on the module
    # path alike.  The library is therefore put in its deterministic mode for all device runs of this test; "identical bits"
    # below then says that nothing of this package's adds an order of its own.
    det = torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)
    det.__enter__()
    try:
        feats, grads = T.run(dev, xd, "none")
    finally:
        ops.reduce_conv_degenerate = node
        det.__exit__(None, None, None)
    assert seen == [1]
    feats, grads = [f.detach().clone() for f in feats], {k: g.clone() for k, g in grads.items()}
    for i in range(5):
        fp64_bound("%s feature %d" % (frame, i), rel_l2(feats[i], f64[i]), rel_l2(f32[i], f64[i]))
    for k in T.GRADS:
        a, b, c = grads[k], g32[k], g64[k]
        if k == "reduce_conv.0.weight":
            assert float(a[:, 64:].abs().max()) == 0.0
            a, b, c = a[:, :64], b[:, :64], c[:, :64]
        fp64_bound("%s gradient %s" % (frame, k), rel_l2(a, c), rel_l2(b, c))
    bn = dev.layer0[1]
    assert_close_frac(bn.running_mean, s64[0], rtol=1e-4, atol=1e-5, name="running_mean")
    assert_close_frac(bn.running_var, s64[1], rtol=1e-4, atol=1e-5, name="running_var")
    assert int(bn.num_batches_tracked) == s64[2] == 4
    # a second forward / backward from the same state: identical bits
    dev2 = copy.deepcopy(enc).cuda()
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        feats2, grads2 = T.run(dev2, xd, "none")
    differ = ["feature %d" % i for i, (a, b) in enumerate(zip(feats, feats2)) if not torch.equal(a, b)]
    differ += [k for k in T.GRADS if not torch.equal(grads[k], grads2[k])]
    assert not differ and torch.equal(bn.running_var, dev2.layer0[1].running_var), differ
    # the multi-frame call (real lookups) keeps the module path in train mode; so does fuse_train = False
    ops.reduce_conv_degenerate = lambda *a: (seen.append(2), node(*a))[1]
    try:
        look = torch.roll(xd["current"], 3, 3).unsqueeze(1) * 0.95
        poses = torch.from_numpy(R.generic_poses(2, 1)).cuda()
        poses[:, :, :3, 3] *= 0.03
        dev2.train()
        feats3, _, conf = dev2(xd["current"], look, poses, xd["K"], xd["invK"])
        sum(f.sum() for f in feats3).backward()
        assert len(feats3) == 5 and conf.shape == (2, H // 4, W // 4) and dev2.reduce_conv[0].weight.grad is not None
        dev2.fuse_train = False
        T.run(dev2, xd, "none")
    finally:
        ops.reduce_conv_degenerate = node
    assert seen == [1]


# --------------------------------------------------------------------------------------------------------------- trainer
ARGV = ("--depth_net manydepth --dataset synthetic --frame_ids 0 --use_stereo --height 64 --width 128 --batch_size 2 --adv_train "
        "--norm_type l_inf --atk_steps 2 --max_steps 2")


def _trainer(tmp_path, argv=ARGV, extra="", seed=3):
    from depthmodelhardening_amd.options import MonodepthOptions
    from depthmodelhardening_amd.trainer import Trainer
    torch.manual_seed(seed)
    import random
    random.seed(seed)
    opt = MonodepthOptions().parse((argv + " --synthetic_len 8 --atk_batch_size 2 --model_name t --seed %d --log_dir %s %s" % (
        seed, tmp_path, extra)).split())
    tr = Trainer(opt, device=torch.device("cuda"))
    tr.val_eval_count = 0       # the logging step's evaluation under attack is not what these tests are about
    return tr


def _float64_head(enc):
    """In train() mode the two layers the fused train path replaces -- the stem convolution on the normalised frame, and
    reduce_conv -- computed in float64 from the fp32 weights and rounded to fp32 once (autograd differentiates them in float64):
    the module path with those two layers as exact as the number format allows.  Everything else, and eval() mode, is untouched."""
    extract, reduce = enc.feature_extraction, enc._reduce

    def feature_extraction(image, return_all_feats=False):
        if not enc.training:
            return extract(image, return_all_feats)
        z = F.conv2d((image.double() - 0.45) / 0.225, enc.layer0[0].weight.double(), None, 2, 3).float()
        f0 = enc.layer0[2](enc.layer0[1](z))
        feats = [f0, enc.layer1(f0)]
        return feats if return_all_feats else feats[1]

    def _reduce(x, weight):
        if not enc.training:
            return reduce(x, weight)
        return torch.relu(F.conv2d(x.double(), weight.double(), enc.reduce_conv[0].bias.double(), 1, 1)).float()
    enc.feature_extraction, enc._reduce = feature_extraction, _reduce


def _two_steps(tmp_path, mode):
    """The command's two steps (Adam, each run's own attacks).  ``mode``: "fused"; "module" (the encoder's fuse_train off: what the
    commit before K36 runs); "float64" (the module path with _float64_head).  Returns (trainer, losses, parameter deltas after
    step 1 and after step 2)."""
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):      # (__init__ runs the first attack)
        tr = _trainer(tmp_path / mode)
    enc = tr.models["encoder"]
    enc.fuse_train = mode == "fused"
    if mode == "float64":
        _float64_head(enc)
    before = [p.detach().clone() for p in tr.bucket.params]
    tr.set_train()
    tr.epoch = tr.step = 0
    losses, deltas = [], []
    # the library in its deterministic mode (see the encoder test): a run of a mode then does not depend on the order in which
    # the library's atomics landed
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        for _ in range(2):
            losses.append(tr.train_step())
            tr.step += 1
            tr._apply_pending_update()
            deltas.append(torch.cat([(p.detach() - q).reshape(-1) for p, q in zip(tr.bucket.params, before)]))
    return tr, losses, deltas


def test_trainer_two_adversarial_steps(tmp_path):
    """The command's two steps: finite losses, every disparity = decoder output / 8.6437, the two-step weights against the same
    run on the encoder's module path, the checkpoint round trip.

    The weights.  Three runs of the command as it stands (Adam, own attacks): this path, the module path, and the module path
    with the two layers this path replaces (stem, reduce_conv) computed in float64 -- a yardstick whose stem is independent of
    both.  This path's parameter deltas may be no further from that run's than 1.5 x (fp64_bound's factor) the module path's are:
    the fused stem and K36 train the weights the module path trains, as far as fp32 can tell.  Adam's first steps are
    -lr * sign(g), so the distance between two fp32 runs counts the elements whose gradient is at rounding level (8 % rel-L2
    between any two runs here) -- many elements, hence a figure that is stable from run to run, which the distances of SGD
    steps (a handful of flipped pixels of the loss's per-pixel minimum) are not."""
    from depthmodelhardening_amd import depth_model as DM
    tr, losses, d_fused = _two_steps(tmp_path, "fused")
    assert all(torch.isfinite(l["loss"]).all() for l in losses) and float(d_fused[1].abs().max()) > 0
    enc = tr.models["encoder"]
    assert enc.prematching_conv[0].weight.grad is None and all(p.grad is None for p in enc.backprojector.parameters())
    assert float(enc.reduce_conv[0].weight.grad[:, 64:].abs().max()) == 0.0
    # every ("disp", s) is the decoder's output / 8.6437
    inputs = tr.dataset.next_batch(2)
    raw = {}
    hook = tr.models["depth"].register_forward_hook(lambda mod, args, out: raw.update({k: v.clone() for k, v in out.items()}))
    with torch.no_grad():
        outputs, _ = tr.process_batch(inputs)
    hook.remove()
    for s in range(4):
        assert torch.equal(outputs[("disp", s)], raw[("disp", s)] / 8.6437) and float(raw[("disp", s)].max()) > 0
    _, _, d_module = _two_steps(tmp_path, "module")
    _, _, d_f64 = _two_steps(tmp_path, "float64")
    for i in range(2):
        print("step %d parameter deltas, rel-L2: fused vs module %.3g, fused vs float64 head %.3g, module vs float64 head %.3g" % (
            i + 1, rel_l2(d_fused[i], d_module[i]), rel_l2(d_fused[i], d_f64[i]), rel_l2(d_module[i], d_f64[i])))
    # the two-step weights against the module-path run's, within fp64_bound's factor of that run's own distance from the yardstick
    fp64_bound("two-step parameter deltas vs module path", rel_l2(d_fused[1], d_module[1]), rel_l2(d_module[1], d_f64[1]))
    # ... and so (triangle inequality) no further from the yardstick than the module path is, by more than the same factor
    fp64_bound("two-step parameter deltas vs float64 head", rel_l2(d_fused[1], d_f64[1]), rel_l2(d_module[1], d_f64[1]))
    # save_model -> import_depth_model(..., matching=True): the eval disparity, bit for bit
    tr.set_eval()
    x = inputs[("color", 0, 0)]
    tr.save_model()
    folder = os.path.join(tr.log_path, "models", "weights_0")
    back = DM.import_depth_model((1024, 320), 'manydepth', pre_model_path=folder, matching=True).cuda().eval()
    # (the library in its deterministic mode: at this frame size the deep layers run its convolutions, see the encoder test)
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        want = tr.models["DepthModelWrapper"](x)
        again = tr.models["DepthModelWrapper"](x)
        got = back(x)
    assert torch.equal(want, again), "the wrapper itself gives two answers: max %.3g" % float((want - again).abs().max())
    assert torch.equal(got, want) and float(want.abs().max()) > 0, float((got - want).abs().max())


def test_trainer_one_step_with_a_pose_network(tmp_path):
    argv = ARGV.replace("--frame_ids 0 --use_stereo", "--pose_net --frame_ids 0 -1 1 --use_stereo").replace("--max_steps 2", "--max_steps 1")
    tr = _trainer(tmp_path, argv)
    assert "pose_encoder" in tr.models
    tr.set_train()
    tr.epoch = tr.step = 0
    losses = tr.train_step()
    tr._apply_pending_update()
    assert torch.isfinite(losses["loss"]).all()
    g = tr.models["encoder"].reduce_conv[0].weight.grad
    assert g is not None and float(g[:, :64].abs().max()) > 0 and float(g[:, 64:].abs().max()) == 0.0
