"""The odometry evaluation on the host: ``ops.pose_ate_host`` (K40's numpy twin, the reference's loop) and ``ops.gt_local_poses``
against the reference's own run and the float64 anchor of tests/golden/pose_ate.npz (tools/make_goldens_pose_eval.py; the gate is
stated in tests/pose_eval_ref.py), the file names and the generated test lists of ``datasets.kitti_odom``, and the refusals of
``ops.pose_ate*`` and of ``evaluate_pose.evaluate``.  No GPU."""
import hashlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from depthmodelhardening_amd import ops
from tests import pose_eval_ref as R


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(R.GOLDEN))


def test_wiring():
    from depthmodelhardening_amd import _native as N, build, library
    assert {"dmh_pose_ate", "dmh_stem_pair_norm_fwd"} <= set(N.EXPORTS)
    assert {"pose_traj.hip", "pose_stem.hip"} <= set(build.SOURCES)
    assert {"pose_ate", "stem_pair_norm"} <= set(library.OPS)
    assert hasattr(torch.ops.dmh, "pose_ate") and hasattr(torch.ops.dmh, "stem_pair_norm")
    assert ops.POSE_TRACK_LENGTH == R.TRACK_LENGTH == 5


def test_the_fixture_holds_what_the_gate_needs(golden):
    assert os.path.getsize(R.GOLDEN) < 100 * 1000
    assert sorted({c[1] for c in R.CASES}) == [1, 3, 4, 5, 9, 37, 65, 257]
    for name, n, _, zeros, track_lengths in R.CASES:
        assert golden[name + "_gt_global"].shape == (n + 1, 3, 4) and golden[name + "_pred"].shape == (n, 4, 4)
        assert golden[name + "_pred"].dtype == np.float32 and golden[name + "_gt_local"].dtype == np.float64
        for i in zeros:
            assert not golden[name + "_pred"][i, :3, 3].any()
        for t in track_lengths:
            tag = "%s_t%d_" % (name, t)
            assert golden[tag + "ates"].shape == golden[tag + "anchor_ates"].shape == (n,)
            assert 0 <= float(golden[tag + "e_ref"]) < 1e-12          # the reference's own run is a float64 run
    # the zero case: the snippets that consist of one zero-translation prediction alone, and nothing else
    assert np.flatnonzero(np.isnan(golden["zero_t5_ates"])).tolist() == [8]
    assert np.flatnonzero(np.isnan(golden["zero_t2_ates"])).tolist() == [3, 8]
    assert np.isnan(golden["zero_t5_mean"]) and np.isnan(golden["zero_t5_std"]) and np.isnan(golden["zero_t5_anchor_mean"])
    finite = golden["n257_t5_ates"]
    assert 1e-3 < finite.mean() < 1e-1                               # errors of the order 1e-2


@pytest.mark.parametrize("run", R.RUNS, ids=R.RUN_IDS)
def test_pose_ate_host_against_the_anchor(golden, run):
    name, t = run
    pred, local = golden[name + "_pred"], golden[name + "_gt_local"]
    ates, mean, std = ops.pose_ate_host(pred, local, t)
    R.check_run(golden, run, ates, mean, std, "pose_ate_host")
    # CPU tensors take the same path through ops.pose_ate
    out = ops.pose_ate(torch.from_numpy(pred), torch.from_numpy(local), t)
    assert out.ates.dtype == torch.float64 and out.stats.shape == (2,)
    assert np.array_equal(out.ates.numpy(), ates, equal_nan=True)
    assert np.array_equal(out.stats.numpy(), np.array([mean, std]), equal_nan=True)


def test_truncated_snippets_use_the_point_count(golden):
    """The last snippet has one pose, two points: the error is the root of the squared error over 2, not over sqrt(2)."""
    pred, local = golden["n5_pred"], golden["n5_gt_local"]
    ates, _, _ = ops.pose_ate_host(pred, local, 5)
    p, g = pred[4, :3, 3].astype(np.float64), local[4, :3, 3]
    s = (g * p).sum() / (p * p).sum()
    assert abs(ates[4] - np.sqrt(((p * s - g) ** 2).sum()) / 2) <= 1e-15
    # a shorter track_length only shortens the snippets
    a2, _, _ = ops.pose_ate_host(pred, local, 2)
    assert abs(a2[4] - ates[4]) == 0 and a2.shape == (5,)


@pytest.mark.parametrize("name", R.LOCAL_CASES)
def test_gt_local_poses_against_the_anchor(golden, name):
    gt_global = golden[name + "_gt_global"].astype(np.float64)
    local = ops.gt_local_poses(gt_global)
    assert local.dtype == np.float64 and local.shape == golden[name + "_gt_local"].shape
    d, e_ref = R.rel_dist_poses(local, golden[name + "_anchor_local"]), float(golden[name + "_e_ref_local"])
    print("gt_local_poses %-5s distance from the anchor %.3g  e_ref %.3g  bound %.3g" % (name, d, e_ref, R.bound(e_ref)))
    assert d <= R.bound(e_ref)
    assert R.rel_dist_poses(local, golden[name + "_gt_local"]) <= R.bound(e_ref)        # and that close to the reference's own


def test_odom_paths_and_lists(golden):
    from depthmodelhardening_amd.datasets import kitti_odom as K
    got = [K.odom_image_path(*q) for q in R.PATH_QUERIES]
    assert got == [str(s) for s in golden["paths"]]
    assert K.odom_image_path("/data/odom", 9, 0, "l") == "/data/odom/sequences/09/image_2/000000.jpg"      # the default: .jpg
    for seq, count, digest in zip(golden["test_sequences"], golden["test_counts"], golden["test_digests"]):
        lines = K.odom_test_lines(int(seq), K.ODOM_TEST_PAIRS[int(seq)])
        assert len(lines) == int(count) == K.ODOM_TEST_PAIRS[int(seq)]
        assert hashlib.sha256("\n".join(lines).encode()).hexdigest() == str(digest)
    assert K.odom_test_lines(9, 3) == ["9 0 l", "9 1 l", "9 2 l"] and K.odom_test_lines(10, 0) == []


def test_kitti_odom_stays_out_of_training():
    from depthmodelhardening_amd.datasets import kitti
    with pytest.raises(NotImplementedError, match="kitti_odom"):
        kitti.from_options(SimpleNamespace(dataset="kitti_odom"), "cpu")


@pytest.mark.parametrize("fn", ["pose_ate", "pose_ate_host"])
def test_refusals_of_pose_ate(golden, fn):
    f = getattr(ops, fn)
    pred, local = torch.from_numpy(golden["n5_pred"]), torch.from_numpy(golden["n5_gt_local"])
    f(pred, local, 5)
    with pytest.raises(RuntimeError, match="5 predicted poses but 4"):
        f(pred, local[:4].contiguous(), 5)
    with pytest.raises(RuntimeError, match="no poses"):
        f(pred[:0], local[:0], 5)
    for t in (1, 0, -3, 2.5, True):
        with pytest.raises(RuntimeError, match="track_length"):
            f(pred, local, t)
    with pytest.raises(RuntimeError, match="pred_poses must be float32"):
        f(pred.double(), local, 5)
    with pytest.raises(RuntimeError, match="gt_local must be float64"):
        f(pred, local.float(), 5)
    with pytest.raises(RuntimeError, match="contiguous"):
        f(pred.transpose(1, 2), local, 5)
    with pytest.raises(RuntimeError, match="contiguous"):
        f(pred, torch.from_numpy(golden["n37_gt_local"])[::2][:5], 5)
    with pytest.raises(RuntimeError, match=r"\[N, 4, 4\]"):
        f(pred[:, :3].contiguous(), local, 5)
    with pytest.raises(RuntimeError, match="tensor or an array"):
        f(pred.tolist(), local, 5)


def test_refusals_of_the_c_entry_points():
    """Host-side argument checks of dmh_pose_ate and dmh_stem_pair_norm_fwd: every call fails before any launch."""
    import ctypes
    from depthmodelhardening_amd import _native as N
    lib = N.lib()
    one, two, three, four = (ctypes.c_void_p(v) for v in (64, 128, 192, 256))
    for args in ((None, two, 5, 5, three, four), (one, two, 0, 5, three, four), (one, two, 5, 1, three, four),
                 (one, two, 5, 5, two, four), (one, two, 5, 5, three, three), (one, ctypes.c_void_p(132), 5, 5, three, four),
                 (one, two, (1 << 24) + 1, 5, three, four)):
        assert lib.dmh_pose_ate(*args, None) == 1, args
        assert b"dmh_pose_ate" in lib.dmh_last_error()
    for args in ((None, two, three, 1, 4, 4, 0.45, 0.225, four), (one, two, three, 0, 4, 4, 0.45, 0.225, four),
                 (one, two, three, 1, 3, 4, 0.45, 0.225, four), (one, two, three, 1, 4, 6 + 1, 0.45, 0.225, four),
                 (one, two, three, 1, 4, 4, 0.45, 0.0, four), (one, two, three, 1, 4, 4, 0.45, 0.225, one),
                 (one, two, three, 1, 4, 4, 0.45, 0.225, two)):
        assert lib.dmh_stem_pair_norm_fwd(*args, None) == 1, args
        assert b"dmh_stem_pair_norm_fwd" in lib.dmh_last_error()


def test_stem_pair_norm_and_forward_pair_without_a_gpu():
    """CPU tensors are refused by the operator, and ``forward_pair`` IS ``forward(cat)`` for them."""
    from depthmodelhardening_amd import networks
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(1, 3, 32, 32, generator=g), torch.rand(1, 3, 32, 32, generator=g)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.stem_pair_norm(a, b, torch.zeros(64, 6, 7, 7))
    with pytest.raises(RuntimeError, match="fp32"):
        ops.stem_pair_norm(a.double(), b, torch.zeros(64, 6, 7, 7))
    enc = networks.ResnetEncoder(18, False, 2).eval()
    with torch.no_grad():
        pair, cat = enc.forward_pair(a, b), enc.forward(torch.cat([a, b], 1))
    assert len(pair) == 5 and all(torch.equal(p, c) for p, c in zip(pair, cat))


def test_refusals_of_evaluate(tmp_path):
    from depthmodelhardening_amd import evaluate_pose as EP
    from depthmodelhardening_amd.options import MonodepthOptions
    opt = MonodepthOptions().parse(["--eval_split", "odom_9", "--load_weights_folder", str(tmp_path / "missing")])
    with pytest.raises(AssertionError, match="Cannot find a folder at"):
        EP.evaluate(opt)
    opt = MonodepthOptions().parse(["--eval_split", "eigen", "--load_weights_folder", str(tmp_path)])
    with pytest.raises(AssertionError, match="eval_split should be either odom_9 or odom_10"):
        EP.evaluate(opt)
