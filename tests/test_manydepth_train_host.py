"""ManyDepth hardening off the GPU: the encoder's module path in train() mode against tests/golden/manydepth_train.npz (the
reference's own class, tools/make_goldens_manydepth_train.py), ``ops.reduce_conv_degenerate_host`` against the reference's
expression in float64, ``Trainer(host_only=True)`` with ``--depth_net manydepth``, and the argument checks of K36's C entry points."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cost_volume_ref as R
from tests import manydepth_train_ref as T


def _encoder():
    from depthmodelhardening_amd import networks
    enc = networks.ResnetEncoderMatching(18, False, input_height=48, input_width=96)
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict(R.formula_state_dict(shapes), strict=False)
    return enc


def _close(got, want, rtol, atol, name):
    np.testing.assert_allclose(got.detach().numpy(), want, rtol=rtol, atol=atol, err_msg=name)


@pytest.fixture(scope="module")
def module_runs():
    """The module path in train() mode, once per form: (features, gradients, layer0.1 statistics)."""
    x = {k: torch.from_numpy(v) for k, v in R.encoder_inputs().items()}
    out = {}
    for form in ("zero", "none"):
        enc = _encoder()
        feats, grads = T.run(enc, x, form)
        bn = enc.layer0[1]
        out[form] = ([f.detach() for f in feats], {k: g.clone() for k, g in grads.items()},
                     (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)))
    return out


@pytest.mark.parametrize("form", ["zero", "none"])
def test_train_mode_module_path_reproduces_the_reference(golden, module_runs, form):
    """Features 0 and 1 at the tolerances test_manydepth_host.py::test_cpu_module_path_reproduces_the_reference uses for them, what
    lies behind reduce_conv at the ones it uses for reduce_conv's output; the gradients at that rtol (1e-4) with atol = 1e-5 of
    the largest entry (the same arithmetic in the same library: only the order of a few additions may differ)."""
    g = golden("manydepth_train")
    feats, grads, (mean, var, batches) = module_runs[form]
    assert len(feats) == 5
    for i, f in enumerate(feats):
        rtol, atol = (1e-5, 1e-6) if i < 2 else (1e-4, 1e-5)
        _close(T.FEATURE_SAMPLE[i](f), g["features%d" % i], rtol, atol, "features%d" % i)
    gr = grads["reduce_conv.0.weight"]
    for got, key in ((grads["layer0.0.weight"], "grad_layer0_0_weight"), (gr[:, :64][T.REDUCE_SAMPLE], "grad_reduce_weight"),
                     (grads["reduce_conv.0.bias"], "grad_reduce_bias"),
                     (grads["layer2.0.conv1.weight"][T.LAYER2_SAMPLE], "grad_layer2_0_conv1_weight")):
        _close(got, g[key], 1e-4, 1e-5 * float(np.abs(g[key]).max()), key)
    assert int(g["reduce_tail_nonzero"]) == 0 and int((gr[:, 64:] != 0).sum()) == 0 and tuple(gr.shape) == (64, 160, 3, 3)
    # layer0.1's running statistics.  The reference's forward sends the all-zero lookup frame through layer0 / layer1 in train()
    # mode as well: two updates per forward, which the "zero" form repeats; the "none" form makes the current frame's update only
    tag = "" if form == "zero" else "_first"
    _close(mean, g["bn0_mean" + tag], 1e-5, 1e-6, "running_mean")
    _close(var, g["bn0_var" + tag], 1e-5, 1e-6, "running_var")
    assert int(g["bn0_batches"]) == 5 and batches == (5 if form == "zero" else 4)


def test_none_form_and_zero_lookup_form_give_identical_gradients(module_runs):
    fz, gz, _ = module_runs["zero"]
    fn, gn, _ = module_runs["none"]
    assert all(torch.equal(a, b) for a, b in zip(fz, fn))
    assert set(gz) == set(T.GRADS) and all(torch.equal(gz[k], gn[k]) for k in gz)


@pytest.mark.parametrize("shape", [(2, 64, 12, 24), (1, 64, 5, 7)], ids=["2x64x12x24", "1x64x5x7"])
def test_reduce_conv_degenerate_host_is_the_reference_expression(shape):
    from depthmodelhardening_amd import ops
    B, Cc, H, W = shape
    D = 96
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B, Cc, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(64, Cc + D, 3, 3, generator=gen, dtype=torch.float64) * 0.05
    b = torch.randn(64, generator=gen, dtype=torch.float64) * 0.1
    gy = torch.randn(B, 64, H, W, generator=gen, dtype=torch.float64)
    res = []
    for fn in (lambda x_, w_, b_: ops.reduce_conv_degenerate(x_, w_, b_),      # CPU tensors: the host definition
               lambda x_, w_, b_: ops.reduce_conv_degenerate_host(x_, w_, b_),
               lambda x_, w_, b_: F.conv2d(torch.cat([x_, torch.zeros(B, D, H, W, dtype=x_.dtype)], 1), w_, b_, 1, 1).relu()):
        xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
        y = fn(xs, ws, bs)
        res.append((y.detach(),) + torch.autograd.grad(y, (xs, ws, bs), gy))
    for got in res[:2]:
        for a, ref, name in zip(got, res[2], ("y", "g_x", "g_weight", "g_bias")):
            assert a.shape == ref.shape and float((a - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), name
        assert float(got[2][:, Cc:].abs().max()) == 0.0
    assert float(res[2][2][:, Cc:].abs().max()) == 0.0 and float((res[0][0] > 0).double().mean()) > 0.2
    with pytest.raises(RuntimeError, match="reduce_conv_degenerate"):
        ops.reduce_conv_degenerate_host(x, w[:, :32], b)


def _options(tmp_path, extra=""):
    from depthmodelhardening_amd.options import MonodepthOptions
    base = "--dataset synthetic --frame_ids 0 --use_stereo --height 64 --width 128 --batch_size 2 --log_dir %s " % tmp_path
    return MonodepthOptions().parse((base + extra).split())


def _trainer(tmp_path, extra=""):
    from depthmodelhardening_amd.trainer import Trainer
    return Trainer(_options(tmp_path, extra), host_only=True, device=torch.device("cpu"))


def test_trainer_builds_saves_and_reloads_manydepth(tmp_path):
    from depthmodelhardening_amd import depth_model as DM, networks
    torch.manual_seed(5)
    t = _trainer(tmp_path, "--depth_net manydepth")
    enc, wrap = t.models["encoder"], t.models["DepthModelWrapper"]
    assert isinstance(enc, networks.ResnetEncoderMatching) and isinstance(wrap, DM.ManyDepthModelWrapper)
    assert wrap.encoder is enc and wrap.decoder is t.models["depth"] and enc.roi_backward is False
    # parameters_to_train follows the reference (encoder + depth); the bucket leaves out what never receives a gradient
    want = list(enc.parameters()) + list(t.models["depth"].parameters())
    assert len(t.parameters_to_train) == len(want) and all(a is b for a, b in zip(t.parameters_to_train, want))
    skipped = {id(p) for n, p in enc.named_parameters() if n.startswith(("prematching_conv.", "backprojector."))}
    assert len(skipped) == 5
    in_bucket = {id(p) for p in t.bucket.params}
    assert not (in_bucket & skipped) and in_bucket == {id(p) for p in want} - skipped
    assert all(p.requires_grad for p in t.bucket.params)
    # save_model: the two extra keys, and a folder that loads back through import_depth_model(..., matching=True)
    t.epoch = 0
    t.save_model()
    folder = os.path.join(t.log_path, "models", "weights_0")
    saved = torch.load(os.path.join(folder, "encoder.pth"))
    extra = set(saved) - set(enc.state_dict())
    assert extra == {"height", "width", "use_stereo", "min_depth_bin", "max_depth_bin"}
    assert (saved["min_depth_bin"], saved["max_depth_bin"]) == (wrap.min_depth_bin, wrap.max_depth_bin) == (0.1, 20.0)
    b = DM.import_depth_model((1024, 320), 'manydepth', pre_model_path=folder, matching=True)
    sa, sb = wrap.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert (b.min_depth_bin, b.max_depth_bin) == (0.1, 20.0)
    # ... and as --load_weights_folder of a second Trainer (--fine_tune selects the same call)
    for flag in ("", " --fine_tune"):
        t2 = _trainer(tmp_path / ("again" + flag.strip(" -")), "--depth_net manydepth --load_weights_folder %s%s" % (folder, flag))
        s2 = t2.models["DepthModelWrapper"].state_dict()
        assert all(torch.equal(sa[k], s2[k]) for k in sa)


@pytest.mark.parametrize("extra,word", [("--adv_train --norm_type l_inf --contrastive_learning", "contrastive_learning"),
                                        ("--pose_net --frame_ids 0 -1 1 --pose_model_type shared", "shared"),
                                        ("--adv_train --norm_type l_inf --graph_attack", "graph_attack"),
                                        ("--num_layers 34", "num_layers")])
def test_trainer_refuses_what_manydepth_does_not_serve(tmp_path, extra, word):
    with pytest.raises(NotImplementedError, match=word):
        _trainer(tmp_path, "--depth_net manydepth " + extra)


def test_resnet_checkpoints_keep_their_keys(tmp_path):
    from depthmodelhardening_amd import networks
    from depthmodelhardening_amd.options import MonodepthOptions
    assert MonodepthOptions().parse([]).depth_net == "resnet"
    t = _trainer(tmp_path)
    assert isinstance(t.models["encoder"], networks.ResnetEncoder) and not t.manydepth
    t.epoch = 0
    t.save_model()
    saved = torch.load(os.path.join(t.log_path, "models", "weights_0", "encoder.pth"))
    assert list(saved) == list(t.models["encoder"].state_dict()) + ["height", "width", "use_stereo"]
    assert (saved["height"], saved["width"], saved["use_stereo"]) == (64, 128, True)


def test_k36_entry_points_refuse_bad_arguments():
    """Null pointers, C or K not a multiple of 8, sizes beyond the 32-bit index range: 1 and a message, before any launch."""
    from depthmodelhardening_amd import _native as N, build
    assert "reduce_node.hip" in build.SOURCES
    lib = N.lib()
    p = C.c_void_p(256)     # never dereferenced: every call below is refused on the host
    err = lambda: lib.dmh_last_error().decode()     # noqa: E731
    assert lib.dmh_reduce_bias_relu(None, p, 2, 64, 64, 288, p, None) == 1 and "null" in err()
    assert lib.dmh_reduce_bwd_mask(p, p, 2, 64, 64, 288, p, None, None) == 1 and "null" in err()
    assert lib.dmh_reduce_bwd_finish(p, None, 2, 64, 64, 96, 288, p, p, None) == 1 and "null" in err()
    for fn, args in ((lib.dmh_reduce_bias_relu, lambda c, k, hw, b=2: (p, p, b, c, k, hw, p, None)),
                     (lib.dmh_reduce_bwd_mask, lambda c, k, hw, b=2: (p, p, b, c, k, hw, p, p, None)),
                     (lib.dmh_reduce_bwd_finish, lambda c, k, hw, b=2: (p, p, b, c, k, 96, hw, p, p, None))):
        assert fn(*args(60, 64, 288)) == 1 and "C must be a multiple of 8" in err()
        assert fn(*args(64, 60, 288)) == 1 and "K must be a multiple of 8" in err()
        assert fn(*args(64, 64, 1 << 20, 32)) == 1 and "32-bit" in err()
        assert fn(*args(64, 64, 0)) == 1 and "positive" in err()
    assert lib.dmh_reduce_bwd_finish(p, p, 2, 64, 64, 1 << 22, 288, p, p, None) == 1 and "32-bit" in err()
    assert lib.dmh_reduce_bwd_partials_size(2, 60, 64, 288) == -1 and lib.dmh_reduce_bwd_rounds(2, 64, 60, 288) == -1
    # the sizes and the rounding count the kernel header derives: S = min(64, ceil(HW / 1024)) slabs
    assert lib.dmh_reduce_bwd_partials_size(2, 64, 64, 288) == 64 and lib.dmh_reduce_bwd_partials_size(12, 64, 64, 80 * 256) == 64 * 20
    assert lib.dmh_reduce_bwd_rounds(2, 64, 64, 288) == 2 * 1 + 12 and lib.dmh_reduce_bwd_rounds(3, 64, 64, 63) == 3 * 1 + 10
    assert lib.dmh_reduce_bwd_rounds(12, 64, 64, 80 * 256) == 12 * 1 + 12 and lib.dmh_reduce_bwd_rounds(1, 64, 64, 1 << 20) == 16 + 12
    assert {"dmh_reduce_bias_relu", "dmh_reduce_bwd_mask", "dmh_reduce_bwd_finish"} <= set(N.EXPORTS)


def test_operator_is_registered():
    from depthmodelhardening_amd import library
    assert {"reduce_conv_degenerate", "reduce_conv_degenerate_bwd"} <= set(library.OPS)
    assert hasattr(torch.ops.dmh, "reduce_conv_degenerate")
