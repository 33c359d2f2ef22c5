"""The odometry evaluation on the GPU: K40 (``ops.pose_ate``) against the float64 anchor of tests/golden/pose_ate.npz, K41
(``ops.stem_pair_norm``, ``ResnetEncoder.forward_pair``) against a float64 convolution, and ``evaluate_pose.evaluate`` end to end
against its host twin.

K41's bound, per output element: |y - y64| <= c * (|w| (*) |xn|), both sides from a float64 convolution of the concatenated,
normalised input on the CPU, with c = max(1.5e-7, 4 c_ATen): 1.5e-7 is the error of a k-ordered fp32 fma chain per unit of
sum |a b| (the fp32 MFMA), and c_ATen is the largest such ratio the library's own fp32 path -- ``conv2d((cat - 0.45) / 0.225)`` -- reaches on
the same inputs in the same test; both normalise in fp32, which is part of either error.  Measured on one MI355X, largest ratio
per shape (K41 / ATen; also in profiles/pose_eval.txt): (1,2,2) 1.04e-07 / 6.09e-08; (2,46,130) 1.89e-07 / 1.60e-07; (3,64,96 as
views of one tensor) 1.37e-07 / 2.00e-07.  K40: at most 1.13 e_ref from the anchor over the nine runs (bound 20 e_ref).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import pose_eval_ref as R  # noqa: E402
from tests.util import assert_close_frac  # noqa: E402

DEV = torch.device("cuda")
CHAIN_C = 1.5e-7


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(R.GOLDEN))


# ------------------------------------------------------------------------------------------------------------------- K40
@pytest.mark.parametrize("run", R.RUNS, ids=R.RUN_IDS)
def test_pose_ate_against_the_anchor(golden, run):
    from depthmodelhardening_amd import library, ops  # noqa: F401  (library registers torch.ops.dmh)
    name, t = run
    pred = torch.from_numpy(golden[name + "_pred"]).to(DEV)
    local = torch.from_numpy(golden[name + "_gt_local"]).to(DEV)
    out = ops.pose_ate(pred, local, t)
    assert out.ates.is_cuda and out.stats.is_cuda and out.ates.dtype == out.stats.dtype == torch.float64
    ates, stats = out.ates.cpu().numpy(), out.stats.cpu().numpy()
    R.check_run(golden, run, ates, float(stats[0]), float(stats[1]), "K40")
    again = ops.pose_ate(pred, golden[name + "_gt_local"], t)           # a numpy ground truth is uploaded
    assert torch.equal(again.ates.view(torch.int64), out.ates.view(torch.int64))
    assert torch.equal(again.stats.view(torch.int64), out.stats.view(torch.int64))
    a3, s3 = torch.ops.dmh.pose_ate(pred, local, t)
    assert torch.equal(a3.view(torch.int64), out.ates.view(torch.int64)) and torch.equal(s3.view(torch.int64), out.stats.view(torch.int64))


def test_pose_ate_refuses_on_the_device(golden):
    from depthmodelhardening_amd import ops
    pred = torch.from_numpy(golden["n5_pred"]).to(DEV)
    local = torch.from_numpy(golden["n5_gt_local"])
    with pytest.raises(RuntimeError, match="share a device"):
        ops.pose_ate_launch(pred, local, 5)
    with pytest.raises(RuntimeError, match="track_length"):
        ops.pose_ate(pred, local.to(DEV), 1)


# ------------------------------------------------------------------------------------------------------------------- K41
def _pair_inputs(B, H, W, seed, overlapping):
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(64, 6, 7, 7, generator=g) - 0.5) * 0.2
    if overlapping:
        f = torch.rand(B + 1, 3, H, W, generator=g)
        fd = f.to(DEV)
        return f[:-1], f[1:], w, fd[:-1], fd[1:]
    a, b = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    return a, b, w, a.to(DEV), b.to(DEV)


@pytest.mark.parametrize("shape,overlapping", [((1, 2, 2), False), ((2, 46, 130), False), ((3, 64, 96), True)],
                         ids=["1x2x2", "2x46x130", "3x64x96-views"])
def test_stem_pair_norm_against_float64(shape, overlapping):
    from depthmodelhardening_amd import library, ops  # noqa: F401  (library registers torch.ops.dmh)
    B, H, W = shape
    a, b, w, ad, bd = _pair_inputs(B, H, W, 7 * B + H, overlapping)
    wd = w.to(DEV)
    xn = (torch.cat([a, b], 1).double() - 0.45) / 0.225
    want = F.conv2d(xn, w.double(), None, 2, 3)
    mass = F.conv2d(xn.abs(), w.double().abs(), None, 2, 3)
    assert float(mass.min()) > 0
    with torch.no_grad():
        y = ops.stem_pair_norm(ad, bd, wd)
        y2 = ops.stem_pair_norm(ad, bd, wd)
        y3 = torch.ops.dmh.stem_pair_norm(ad, bd, wd, 0.45, 0.225)
        aten = F.conv2d((torch.cat([ad, bd], 1) - 0.45) / 0.225, wd, None, 2, 3)
    assert y.shape == (B, 64, H // 2, W // 2) and y.dtype == torch.float32
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32)) and torch.equal(y.view(torch.int32), y3.view(torch.int32))
    r_k41 = float(((y.cpu().double() - want).abs() / mass).max())
    c_aten = float(((aten.cpu().double() - want).abs() / mass).max())
    c = max(CHAIN_C, 4.0 * c_aten)
    print("stem_pair_norm %s: largest |err| / (|w| (*) |xn|): K41 %.3g  ATen %.3g  bound c %.3g" % (shape, r_k41, c_aten, c))
    assert r_k41 <= c, (shape, r_k41, c_aten)


def test_stem_pair_norm_refuses_a_gradient():
    from depthmodelhardening_amd import ops
    a, b, w, ad, bd = _pair_inputs(1, 8, 8, 1, False)
    wd = w.to(DEV)
    for leaf in range(3):
        args = [ad.clone(), bd.clone(), wd.clone()]
        args[leaf].requires_grad_(True)
        with pytest.raises(RuntimeError, match="forward only"):
            ops.stem_pair_norm(*args)
        with torch.no_grad():
            ops.stem_pair_norm(*args)
    with pytest.raises(RuntimeError, match="even H, W"):
        ops.stem_pair_norm(ad[:, :, :7], bd[:, :, :7], wd)
    with pytest.raises(RuntimeError, match="even H, W"):
        ops.stem_pair_norm(ad, bd[:, :, :6], wd)


def test_forward_pair_against_forward_of_the_concatenation():
    from depthmodelhardening_amd import networks
    torch.manual_seed(5)
    enc = networks.ResnetEncoder(18, False, 2).to(DEV).eval()
    g = torch.Generator().manual_seed(6)
    a, b = torch.rand(2, 3, 64, 96, generator=g).to(DEV), torch.rand(2, 3, 64, 96, generator=g).to(DEV)
    with torch.no_grad():
        assert enc._pair_stem_ok(a, b)
        pair = [f.clone() for f in enc.forward_pair(a, b)]
        cat = enc.forward(torch.cat([a, b], 1))
    assert len(pair) == len(cat) == 5 and all(p.shape == c.shape for p, c in zip(pair, cat))
    assert_close_frac(pair[0], cat[0], rtol=1e-5, atol=2e-6 * cat[0].abs().max().item(), name="forward_pair feature 0")
    for i in range(1, 5):
        assert_close_frac(pair[i], cat[i], rtol=1e-3, atol=1e-4 * cat[i].abs().max().item(), name="forward_pair feature %d" % i)
    # with grad enabled the filter is owed a gradient: the fallback, which IS the cat call
    assert not enc._pair_stem_ok(a, b)


def test_a_train_mode_encoder_takes_the_fallback(monkeypatch):
    """In train mode ``forward_pair`` IS ``forward(torch.cat([a, b], 1))``: one call of ``forward`` on the concatenation, whose
    result it hands back, and torch.equal to a cat call of one's own.

    The second comparison sets two executions of the train-mode forward side by side, so it can only hold where that forward
    repeats itself.  Through the library's convolutions it does not at this shape: measured on one MI355X, two identical
    ``forward(cat)`` calls differ in features 2, 3 and 4 (layer2 on: the 128-channel and stride-2 configurations), with no
    ``forward_pair`` involved.  So the comparison runs on ATen's own convolutions (``torch.backends.cudnn.flags(enabled=False)``,
    as tests/util.no_miopen does), where the forward repeats itself, and the test asserts that it does."""
    from depthmodelhardening_amd import networks
    torch.manual_seed(5)
    enc = networks.ResnetEncoder(18, False, 2).to(DEV).train()
    g = torch.Generator().manual_seed(6)
    a, b = torch.rand(2, 3, 64, 96, generator=g).to(DEV), torch.rand(2, 3, 64, 96, generator=g).to(DEV)
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    with torch.no_grad():
        assert not enc._pair_stem_ok(a, b)
    # 1. the fallback is the call itself
    calls, real = [], enc.forward

    def recording(x, *args, **kw):
        out = real(x, *args, **kw)
        calls.append((x, args, kw, out))
        return out
    monkeypatch.setattr(enc, "forward", recording)
    with torch.no_grad():
        got = enc.forward_pair(a, b)
    monkeypatch.undo()
    assert len(calls) == 1 and calls[0][1] == () and calls[0][2] == {}
    assert torch.equal(calls[0][0], torch.cat([a, b], 1)) and got is calls[0][3] and len(got) == 5

    # 2. and equal to a cat call of one's own
    def fresh(call):
        enc.load_state_dict(state)          # a train-mode forward moves the running statistics: every call starts from the same
        with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
            return [f.clone() for f in call()]
    fresh(lambda: enc.forward(torch.cat([a, b], 1)))        # kernels are chosen at the first call of a configuration
    cat = fresh(lambda: enc.forward(torch.cat([a, b], 1)))
    pair = fresh(lambda: enc.forward_pair(a, b))
    again = fresh(lambda: enc.forward(torch.cat([a, b], 1)))
    print("train-mode fallback: features equal to the cat call %s; the cat call equal to itself %s; largest difference of the cat "
          "call from itself %s" % ([torch.equal(p, c) for p, c in zip(pair, cat)], [torch.equal(p, c) for p, c in zip(again, cat)],
                                   ["%.3g" % float((p - c).abs().max()) for p, c in zip(again, cat)]))
    assert all(torch.isfinite(c).all() for c in cat)
    assert all(torch.equal(p, c) for p, c in zip(again, cat)), "the train-mode forward does not repeat itself on ATen's convolutions"
    assert all(torch.equal(p, c) for p, c in zip(pair, cat))


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def odom_tree(tmp_path_factory, golden):
    """A sequence 09 of 6 PNG frames of 370 x 1226, poses/09.txt with 6 lines, random-initialised pose networks."""
    from PIL import Image
    from depthmodelhardening_amd import networks
    root = tmp_path_factory.mktemp("odom")
    img_dir = root / "sequences" / "09" / "image_2"
    img_dir.mkdir(parents=True)
    rng = np.random.RandomState(9)
    for i in range(6):
        Image.fromarray(rng.randint(0, 256, size=(370, 1226, 3), dtype=np.uint8)).save(str(img_dir / ("%06d.png" % i)))
    (root / "poses").mkdir()
    np.savetxt(str(root / "poses" / "09.txt"), golden["n5_gt_global"].astype(np.float64).reshape(6, 12))
    weights = root / "weights"
    weights.mkdir()
    torch.manual_seed(11)
    enc = networks.ResnetEncoder(18, False, 2)
    torch.save(enc.state_dict(), str(weights / "pose_encoder.pth"))
    torch.save(networks.PoseDecoder(enc.num_ch_enc, 1, 2).state_dict(), str(weights / "pose.pth"))
    return root


def _options(root):
    from depthmodelhardening_amd.options import MonodepthOptions
    return MonodepthOptions().parse(["--eval_split", "odom_9", "--data_path", str(root), "--load_weights_folder", str(root / "weights"),
                                     "--height", "64", "--width", "96", "--png", "--batch_size", "4", "--num_workers", "4"])


def test_evaluate_end_to_end_against_the_host_chain(odom_tree, capsys):
    from depthmodelhardening_amd import evaluate_pose as EP
    poses_npy = odom_tree / "weights" / "poses.npy"
    dev = EP.evaluate(_options(odom_tree))
    printed = capsys.readouterr().out
    assert "\n   Trajectory error: {:0.3f}, std: {:0.3f}\n".format(dev["ate_mean"], dev["ate_std"]) in printed
    saved = np.load(str(poses_npy))
    assert saved.shape == (5, 4, 4) and saved.dtype == np.float32 and np.array_equal(saved, dev["pred_poses"])
    os.remove(str(poses_npy))
    host = EP.evaluate(_options(odom_tree), host_chain=True)
    assert np.load(str(poses_npy)).shape == (5, 4, 4)
    assert dev["ates"].shape == host["ates"].shape == (5,) and dev["ates"].dtype == np.float64
    np.testing.assert_allclose(dev["pred_poses"], host["pred_poses"], rtol=1e-4, atol=1e-5)      # K29's tolerance, tests/test_gpu_pose.py
    rel = np.abs(dev["ates"] - host["ates"]) / np.abs(host["ates"])
    print("evaluate: ates %s  relative distance from the host chain %s" % (dev["ates"], rel))
    assert np.isfinite(host["ates"]).all() and rel.max() <= 1e-4
    assert abs(dev["ate_mean"] - host["ate_mean"]) <= 1e-4 * abs(host["ate_mean"])
    assert abs(dev["ate_std"] - host["ate_std"]) <= 1e-4 * abs(host["ate_mean"])
    assert dev["ate_mean"] == pytest.approx(dev["ates"].mean(), rel=1e-12) and dev["ate_std"] == pytest.approx(dev["ates"].std(), rel=1e-9)


def test_odom_pair_frames_decodes_every_file_once(odom_tree, monkeypatch):
    from depthmodelhardening_amd import ops
    from depthmodelhardening_amd.datasets import kitti, kitti_odom
    seen = []
    real = kitti.decode_into

    def counting(path, slot):
        seen.append(path)
        return real(path, slot)
    monkeypatch.setattr(kitti, "decode_into", counting)
    blocks = [b.clone() for b in kitti_odom.odom_pair_frames(str(odom_tree), 9, 5, 64, 96, DEV, ".png", 4, 4)]
    paths = [kitti_odom.odom_image_path(str(odom_tree), 9, i, "l", ".png") for i in range(6)]
    assert sorted(seen) == paths                                        # six decodes for six files
    assert [tuple(b.shape) for b in blocks] == [(5, 3, 64, 96), (2, 3, 64, 96)]
    assert torch.equal(blocks[1][0], blocks[0][-1])                     # the carried frame
    # the frames eval_frames makes of the same files: decode, K31 lanczos to the feed size, level 0, no flip
    raw = np.zeros((6, 370, 1226, 3), dtype=np.uint8)
    sizes = tuple(real(p, raw[i]) for i, p in enumerate(paths))
    want = ops.pil_resize(torch.from_numpy(raw).to(DEV), (64, 96), "lanczos", None, sizes, want_u8=False).f32
    assert torch.equal(torch.cat([blocks[0], blocks[1][1:]], 0), want)
