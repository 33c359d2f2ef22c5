"""The pose networks on the CPU: this project's ``PoseDecoder`` / ``transformation_from_parameters`` (module path: the reference's
expressions) and tests/pose_ref.py's float32 restatement against the reference's own run in tests/golden/pose_net.npz
(tools/make_goldens_pose.py); the restatement's analytic backward against autograd in float64; the host side of K29
(``dmh_pose_head_*`` argument checks), ``--pose_net`` and the constructor's refusals; and the synthetic dataset's batches for
``frame_idxs [0, "s"]`` against the digests recorded from the parent commit.

Tolerance of the fixture comparison: rtol 1e-5 (fp32 rounding; the project's usual CPU-vs-reference tolerance) with an atol of
1e-6 of the tensor's largest entry for the entries that cancel.
"""
import ctypes
import json
import tempfile

import numpy as np
import pytest
import torch

from tests import pose_ref as R

NUM_CH_ENC = [64, 64, 128, 256, 512]


def _close(got, want, name, rtol=1e-5):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want).max()
    print("%s: max abs err %.3g (scale %.3g)" % (name, err, np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-6 * np.abs(want).max(), err_msg=name)


def _decoder(g, prefix, ctor, dtype=torch.float32):
    from depthmodelhardening_amd import networks
    dec = networks.PoseDecoder(*ctor)
    shapes = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
    assert list(shapes) == [str(k) for k in g[prefix + "keys"]]                 # the reference's state_dict keys, in its order
    assert [list(shapes[k]) for k in shapes] == [json.loads(str(s)) for s in g[prefix + "shapes"]]
    dec.load_state_dict(R.formula_state_dict(shapes))
    return dec.to(dtype)


@pytest.mark.parametrize("prefix,ctor", [("a_", (NUM_CH_ENC, 1, 2)), ("b_", (NUM_CH_ENC, 2))])
def test_pose_decoder_module_path_reproduces_the_reference_fixture(golden, prefix, ctor):
    g = golden("pose_net")
    feats = R.golden_features()
    assert np.array_equal(feats.numpy(), g["features"])
    dec = _decoder(g, prefix, ctor)
    inputs = [feats] if ctor[1] == 1 else [feats, feats.flip(1)]
    nf = dec.num_frames_to_predict_for
    for invert, tag in ((False, prefix + "fwd_"), (True, prefix + "inv_")):
        leaves = [f.clone().requires_grad_(True) for f in inputs]
        axisangle, translation = dec([[f] for f in leaves], invert=invert)
        T = dec.T
        assert T.shape == (2, nf, 4, 4) and axisangle.shape == (2, nf, 1, 3) and translation.shape == (2, nf, 1, 3)
        _close(axisangle.detach(), g[tag + "axisangle"], tag + "axisangle")
        _close(translation.detach(), g[tag + "translation"], tag + "translation")
        _close(T.detach(), g[tag + "T"], tag + "T")
        wt = torch.from_numpy(R.weights((2, 6 * nf), 7)[0]).float()
        grads = torch.autograd.grad((T * wt).sum(), leaves)
        for i, gr in enumerate(grads):
            _close(gr[:, ::8], g[tag + "g_feat%d" % i], tag + "g_feat%d" % i, rtol=1e-4)
        # the float32 restatement of the head on the last convolution's output matches too
        with torch.no_grad():
            out = torch.cat([dec.relu(dec.convs["squeeze"](f)) for f in inputs], 1)
            out = dec.relu(dec.convs[("pose", 0)](out))
            out = dec.relu(dec.convs[("pose", 1)](out))
            out = dec.convs[("pose", 2)](out)
        aa, tr, T32 = R.forward(out.numpy(), [invert] * nf, np.float32)
        assert T32.dtype == np.float32
        _close(aa, g[tag + "axisangle"], tag + "axisangle (restatement)")
        _close(tr, g[tag + "translation"], tag + "translation (restatement)")
        _close(T32, g[tag + "T"], tag + "T (restatement)")


def test_restatement_backward_is_autograd_in_float64():
    from depthmodelhardening_amd.layers import transformation_from_parameters
    for ci, (x, invert) in enumerate(R.cases()):
        B, c6, h, w = x.shape
        nf = c6 // 6
        g_T, g_aa, g_tr = R.weights(x.shape, ci)
        xt = torch.from_numpy(x).double().requires_grad_(True)
        v = 0.01 * xt.mean(3).mean(2).view(-1, nf, 1, 6)
        aa, tr = v[..., :3], v[..., 3:]
        T = torch.stack([transformation_from_parameters(aa[:, f], tr[:, f], invert=invert[f]) for f in range(nf)], 1)
        a64, t64, T64 = R.forward(x, invert, np.float64)
        np.testing.assert_allclose(T.detach().numpy(), T64, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(aa.detach().numpy(), a64, rtol=1e-13, atol=0)
        loss = (T * torch.from_numpy(g_T)).sum() + (aa * torch.from_numpy(g_aa)).sum() + (tr * torch.from_numpy(g_tr)).sum()
        want, = torch.autograd.grad(loss, xt)
        got = R.backward(x, invert, g_T, g_aa, g_tr, np.float64)
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-9, atol=1e-12 * np.abs(want.numpy()).max())
    # the all-zero frame: the identity forward, a finite backward
    x, invert = R.zero_case()
    _, _, T = R.forward(x, invert, np.float32)
    assert np.array_equal(T[1, 1], np.eye(4, dtype=np.float32))


def test_layers_functions_keep_the_reference_surface():
    from depthmodelhardening_amd import layers
    a = torch.tensor([[[0.3, -0.2, 0.1]], [[0.0, 0.0, 0.0]]])
    t = torch.tensor([[[1.0, 2.0, 3.0]], [[-1.0, 0.5, 0.25]]])
    R4, Tm = layers.rot_from_axisangle(a), layers.get_translation_matrix(t)
    assert R4.shape == (2, 4, 4) and torch.equal(R4[1], torch.eye(4)) and torch.equal(Tm[:, :3, 3], t[:, 0])
    M, Mi = layers.transformation_from_parameters(a, t), layers.transformation_from_parameters(a, t, invert=True)
    assert torch.equal(M, Tm @ R4)
    assert torch.allclose(M @ Mi, torch.eye(4).expand(2, 4, 4), atol=1e-6)       # the inverted form is the inverse
    assert torch.equal(t, torch.tensor([[[1.0, 2.0, 3.0]], [[-1.0, 0.5, 0.25]]]))  # (the argument is not negated in place)


def test_pose_head_entry_points_reject_bad_shapes_without_gpu():
    from depthmodelhardening_amd import _native as N
    lib = N.lib()
    one = ctypes.c_void_p(16)
    ok = (2, 2, 3, 5, 0.01, 1)
    assert lib.dmh_pose_head_fwd(None, *ok, one, one, one, None) != 0 and b"null pointer" in lib.dmh_last_error()
    assert lib.dmh_pose_head_fwd(one, *ok, one, one, None, None) != 0 and b"null pointer" in lib.dmh_last_error()
    for bad in ((0, 2, 3, 5, 0.01, 0), (2, 0, 3, 5, 0.01, 0), (2, 2, 0, 5, 0.01, 0), (2, 2, 3, -1, 0.01, 0), (65536, 1, 1, 1, 0.01, 0),
                (2, 33, 3, 5, 0.01, 0), (2, 2, 4096, 4096, 0.01, 0), (2, 2, 3, 5, float("nan"), 0), (2, 2, 3, 5, float("inf"), 0),
                (2, 2, 3, 5, 0.01, 4)):
        assert lib.dmh_pose_head_fwd(one, *bad, one, one, one, None) == 1, bad
        assert b"dmh_pose_head_fwd" in lib.dmh_last_error()
        assert lib.dmh_pose_head_bwd(one, None, None, one, one, *bad, one, None) == 1, bad
    assert b"invert_mask" in lib.dmh_last_error()
    assert lib.dmh_pose_head_bwd(None, None, None, one, one, *ok, one, None) == 1 and b"no output gradient" in lib.dmh_last_error()
    assert lib.dmh_pose_head_bwd(one, None, None, None, one, *ok, one, None) == 1
    assert lib.dmh_pose_head_bwd(one, None, None, one, one, *ok, None, None) == 1
    assert {"dmh_pose_head_fwd", "dmh_pose_head_bwd"} <= set(N.EXPORTS)


def test_pose_head_python_face_rejects_bad_arguments():
    from depthmodelhardening_amd import build, library, ops
    assert "pose_head.hip" in build.SOURCES and {"pose_head", "pose_head_bwd"} <= set(library.OPS)
    assert hasattr(torch.ops.dmh, "pose_head") and hasattr(torch.ops.dmh, "pose_head_bwd")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pose_head(torch.zeros(1, 6, 2, 2))
    assert ops.pose_invert_mask(True, 2) == 3 and ops.pose_invert_mask([False, True, True], 3) == 6
    with pytest.raises(RuntimeError, match="invert flags"):
        ops.pose_invert_mask([True], 2)
    with pytest.raises(RuntimeError, match="not a tensor"):
        ops.pose_invert_mask(torch.tensor([True]), 1)
    aa, tr, T = torch.ops.dmh.pose_head(torch.empty(3, 12, 4, 5, device="meta"), 0, 0.01)        # the fake implementation
    assert aa.shape == (3, 2, 1, 3) and tr.shape == (3, 2, 1, 3) and T.shape == (3, 2, 4, 4)


def _opts(extra):
    from depthmodelhardening_amd.options import MonodepthOptions
    return MonodepthOptions().parse(["--dataset", "synthetic", "--log_dir", tempfile.mkdtemp(), "--weights_init", "scratch"] + extra)


def test_pose_net_flag_and_constructor_refusals():
    from depthmodelhardening_amd.trainer import Trainer
    assert _opts([]).pose_net is False and _opts(["--pose_net"]).pose_net is True
    assert _opts([]).frame_ids == [0, -1, 1]
    with pytest.raises(NotImplementedError, match="--pose_net"):
        Trainer(_opts([]), device="cpu", host_only=True)
    with pytest.raises(NotImplementedError, match="posecnn"):
        Trainer(_opts(["--pose_net", "--pose_model_type", "posecnn"]), device="cpu", host_only=True)
    with pytest.raises(RuntimeError, match="--use_stereo"):
        Trainer(_opts(["--pose_net", "--adv_train", "--norm_type", "l_inf"]), device="cpu", host_only=True)


@pytest.mark.parametrize("extra,encoder_in,decoder_in,nf", [
    ([], 6, 256, 2), (["--pose_model_input", "all"], 9, 256, 2), (["--pose_model_type", "shared"], None, 512, 1),
    (["--pose_model_type", "shared", "--pose_model_input", "all", "--use_stereo"], None, 768, 2)])
def test_pose_models_are_built_trained_and_checkpointed(extra, encoder_in, decoder_in, nf):
    """Host side (no GPU): the models of MD2/trainer.py:97-121, their parameters in the optimiser and the gradient bucket (without
    the unused ``fc``), pose_encoder.pth / pose.pth written and read back bit for bit."""
    import os
    from depthmodelhardening_amd.trainer import Trainer
    opt = _opts(["--pose_net", "--height", "64", "--width", "96", "--synthetic_len", "4"] + extra)
    orig = SyntheticPools.swap(2)
    try:
        tr = Trainer(opt, device="cpu", host_only=True)
    finally:
        SyntheticPools.restore(orig)
    assert ("pose_encoder" in tr.models) == (encoder_in is not None)
    if encoder_in is not None:
        assert tr.models["pose_encoder"].encoder.conv1.weight.shape[1] == encoder_in
    pose = tr.models["pose"]
    assert pose.net[1].weight.shape[1] == decoder_in and pose.num_frames_to_predict_for == nf
    trained = {id(p) for p in tr.parameters_to_train}
    bucketed = {id(p) for p in tr.bucket.params}
    for name in ("pose", "pose_encoder"):
        if name not in tr.models:
            continue
        for pname, p in tr.models[name].named_parameters():
            assert id(p) in trained, (name, pname)
            assert (id(p) in bucketed) == (".fc." not in pname), (name, pname)
    tr.epoch = 0
    tr.save_model()
    folder = os.path.join(tr.log_path, "models", "weights_0")
    want = {n: {k: v.clone() for k, v in tr.models[n].state_dict().items()} for n in ("pose", "pose_encoder") if n in tr.models}
    assert all(os.path.isfile(os.path.join(folder, n + ".pth")) for n in want)
    with torch.no_grad():
        for n in want:
            for p in tr.models[n].parameters():
                p.add_(1.0)
    tr.opt.load_weights_folder = folder
    tr.load_model()
    for n in want:
        got = tr.models[n].state_dict()
        assert list(got) == list(want[n]) and all(torch.equal(got[k], want[n][k]) for k in got)


class SyntheticPools:
    """The trainer builds its dataset with the default pool of 48 full-resolution frames per view: 2 are plenty on the host."""

    @staticmethod
    def swap(pool):
        from depthmodelhardening_amd.datasets import synthetic
        orig = synthetic.SyntheticKITTIDataset.__init__

        def small(self, *a, **kw):
            kw["pool"] = pool
            orig(self, *a, **kw)
        synthetic.SyntheticKITTIDataset.__init__ = small
        return orig

    @staticmethod
    def restore(orig):
        from depthmodelhardening_amd.datasets import synthetic
        synthetic.SyntheticKITTIDataset.__init__ = orig


def test_stereo_batches_are_the_parent_commits(golden):
    """frame_idxs [0, "s"]: every tensor of the batches is bit-identical to the parent commit's (digests in the fixture)."""
    from depthmodelhardening_amd.datasets import SyntheticKITTIDataset
    want = [str(s) for s in golden("pose_net")["dataset_digests"]]
    got = R.dataset_digests(SyntheticKITTIDataset)
    assert len(want) == 64 and got == want


def test_neighbour_frames_of_the_synthetic_dataset():
    from depthmodelhardening_amd.datasets import SyntheticKITTIDataset
    plain = SyntheticKITTIDataset(64, 192, [0, "s"], 4, 8, "cpu", seed=5, pool=3)
    assert plain.neighbour_ids == [] and plain.raw_neighbours == {}
    ds = SyntheticKITTIDataset(64, 192, [0, -1, 1, "s"], 4, 8, "cpu", seed=5, pool=3)
    assert ds.neighbour_ids == [-1, 1] and torch.equal(ds.raw, plain.raw)           # drawn after every existing draw
    assert all(ds.raw_neighbours[f].shape == ds.raw.shape for f in (-1, 1))
    step = max(1, int(round(4 * ds.ori_W / 1024.0)))
    for f in (-1, 1):       # 90 % the pool rolled in the direction of the sign, 10 % texture in [0, 1)
        resid = (ds.raw_neighbours[f] - 0.9 * torch.roll(ds.raw, step * f, 3)) / 0.1
        assert float(resid.min()) > -1e-5 and float(resid.max()) < 1 + 1e-5 and float(resid.std()) > 0.01
    assert not torch.equal(ds.raw_neighbours[-1], ds.raw_neighbours[1])
    b = ds.next_batch(4)
    b0 = plain.next_batch(4)
    assert all(torch.equal(b[k], b0[k]) for k in b0)                                 # the stereo keys are untouched
    assert set(b) - set(b0) == {("color", -1, 0), ("color", 1, 0), ("color_aug", -1, 0), ("color_aug", 1, 0), ("color_aug", "s", 0)}
    assert b[("color", -1, 0)] is b[("color_aug", -1, 0)] and b[("color_aug", "s", 0)] is b[("color", "s", 0)]
    assert b[("color", 1, 0)].shape == b[("color", 0, 0)].shape
    # side and flip: with every sample on the right camera and flipped, the neighbours come from the right pool's neighbours
    ds.rng.seed(3)
    picks_rng = ds.rng.getstate()
    ds.both_sides = ds.flip_augmentation = False
    left = ds.next_batch(2)
    ds.rng.setstate(picks_rng)
    ds.draw_batch_geometry = lambda n: {"side": ["r"] * n, "flip": [True] * n, "synth": [True] * n, "z0": [0.0] * n, "alpha": [0] * n}
    right = ds.next_batch(2)
    ds.rng.setstate(picks_rng)
    picks = [ds.rng.randrange(ds.pool_size) for _ in range(2)]
    idx = torch.tensor(picks) + ds.pool_size
    want = torch.nn.functional.interpolate(ds.raw_neighbours[-1].index_select(0, idx), [64, 192], mode="bilinear",
                                           align_corners=False).flip(3)
    assert torch.equal(right[("color", -1, 0)], want) and not torch.equal(right[("color", -1, 0)], left[("color", -1, 0)])


def test_filter_table_survives_a_second_encoder_inside_a_pass():
    """ops.wino_pass(): only the first ``fresh`` prefetch of a pass empties the table of ready filters; outside a pass every
    ``fresh`` prefetch does, as before."""
    from depthmodelhardening_amd import ops
    saved = dict(ops._wino_ready)
    try:
        ops._wino_ready.clear()
        ops._wino_ready[(1, True)] = (0, None, None)
        ops.wino_prefetch([], fresh=False)
        assert (1, True) in ops._wino_ready
        ops.wino_prefetch([], fresh=True)                   # one encoder per pass: emptied
        assert not ops._wino_ready
        with ops.wino_pass():
            ops._wino_ready[(2, True)] = (0, None, None)    # (left by the previous pass)
            ops.wino_prefetch([], fresh=True)               # the first encoder of the pass empties the table ...
            assert not ops._wino_ready
            ops._wino_ready[(3, True)] = (0, None, None)    # ... its backward-data forms ...
            ops.wino_prefetch([], fresh=True)               # ... survive the second encoder's prefetch
            assert list(ops._wino_ready) == [(3, True)]
            with ops.frozen_weights():
                ops.wino_prefetch([], fresh=True)           # a frozen scope never touches the table
            assert list(ops._wino_ready) == [(3, True)]
        assert ops._wino_pass is None
        ops.wino_prefetch([], fresh=True)
        assert not ops._wino_ready
    finally:
        ops._wino_ready.clear()
        ops._wino_ready.update(saved)
