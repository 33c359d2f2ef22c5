"""K26 and Phy_obj_atk_guassian / Phy_obj_atk_arbi on the GPU: the blur kernel bit for bit against the windows scipy wrote into
tests/golden/atk_gauss.npz (tests/test_gauss_ref.py holds the numpy restatement to the same windows, and to scipy itself), the
compose kernel, the device loop against its host-chain twin, the attack against the reference's own 10-step run, windows against
full frames, the absence of host reads, the random-patch baseline, the evaluation entry, the refusals, the registered operators.

Cost bound (per step): |cost_hip - cost_ref| <= 20 e_ref |cost_ref| (tests/test_gpu_light._check_costs), e_ref = the reference's
own fp32-versus-float64 spread on the same inputs, stored in the fixture.
"""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gauss_ref as R  # noqa: E402
from tests.util import assert_close_frac, no_miopen, np_t  # noqa: E402

ROWS = (slice(None), slice(None), slice(120, 300, 9), slice(300, 800, 5))
TRAIN_DIST = list(np.arange(5, 10, 0.2))


def _mods():
    from depthmodelhardening_amd import library, ops  # noqa: F401
    from depthmodelhardening_amd import torchattacks as ta
    return ops, ta


def _windows(ops, x, sigmas, region):
    dev = torch.device("cuda")
    weights, radii = ops.gauss_blur_table(sigmas)
    return ops.gauss_blur_windows(torch.from_numpy(x).to(dev), torch.from_numpy(weights).to(dev), torch.from_numpy(radii).to(dev),
                                  region)


def _report(got, want, what):
    """Asserts got == want bit for bit; on a mismatch names the count, the largest difference and the first differing value."""
    got, want = got.cpu(), torch.as_tensor(want)
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    diff = got != want
    n_bad = int(diff.sum())
    print("%s: %d values, %d differ" % (what, got.numel(), n_bad))
    if n_bad:
        at = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError("%s: %d of %d values differ, largest |difference| %.3g; first at %s: kernel %r, scipy %r" % (
            what, n_bad, got.numel(), float((got.double() - want.double()).abs().max()), at, float(got[at]), float(want[at])))


# ------------------------------------------------------------------------------------------------------------------- 1. kernel
@pytest.mark.parametrize("h,w,rect", R.SMALL_SHAPES)
def test_windows_equal_scipy_on_small_shapes(golden, h, w, rect):
    """Whole patch and an interior rectangle; sigma 0.4 (radius 2), 3.0 (radius 12 >= n at 7 x 9) and 2 max(h, w) (radius 8 n:
    the reflected index wraps several periods on both axes)."""
    ops, _ = _mods()
    g = golden("atk_gauss")
    x, sig = R.kernel_input(h, w), R.small_sigmas(h, w)
    want = np.concatenate([g["win_%dx%d_%d" % (h, w, k)] for k in range(len(sig))], 0)
    _report(_windows(ops, x, sig, (0, h, 0, w)), want, "%d x %d, whole" % (h, w))
    _report(_windows(ops, x, sig, rect), want[:, :, rect[0]:rect[1], rect[2]:rect[3]], "%d x %d, %s" % (h, w, rect))


def test_windows_equal_scipy_on_the_object(golden):
    """260 x 300, the default rectangle, sigmas 15, 75 and 149.99999999999997 (radii 60, 300, 600) in one launch pair."""
    ops, _ = _mods()
    g = golden("atk_gauss")
    sig = [float(s) for s in g["win_big_sigma"]]
    assert sig == [15.0, 75.0, 149.99999999999997]
    _report(_windows(ops, R.kernel_input(260, 300), sig, ops.GAUSS_REGION), g["win_big"], "260 x 300, %s" % (ops.GAUSS_REGION,))


# ------------------------------------------------------------------------------------------------------------------ 2. compose
def test_compose_writes_the_window_and_keeps_the_object():
    ops, _ = _mods()
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(4)
    obj = torch.rand(1, 3, 37, 50, generator=gen).to(dev)
    region = (5, 30, 7, 41)
    windows = torch.rand(3, 3, 25, 34, generator=gen).to(dev) + 2.0        # no value of the object
    for q in range(3):
        out = ops.gauss_blur_compose(windows, torch.tensor([q, 7], dtype=torch.int32, device=dev), obj, region)
        want = obj.clone()
        want[:, :, 5:30, 7:41] = windows[q]
        assert torch.equal(out, want), q
    # the rectangle clips as slices clip
    small = windows[:, :, :7, :10].contiguous()
    out = ops.gauss_blur_compose(small, torch.zeros(1, dtype=torch.int32, device=dev), obj, (30, 170, 40, 200))
    want = obj.clone()
    want[:, :, 30:, 40:] = small[0]
    assert torch.equal(out, want)
    for idx in (3, 4, -1, -7, 1 << 30):      # outside [0, steps): ``out`` stays as it is
        out = torch.full_like(obj, 0.25)
        ops.gauss_blur_compose(windows, torch.tensor([idx], dtype=torch.int32, device=dev), obj, region, out=out)
        assert bool((out == 0.25).all()), idx


# ------------------------------------------------------------------------------------------------------------------- 3. attack
def _run(model, B, seed=13, scene_seed=8, eval=False, **attrs):
    _, ta = _mods()
    from oracle import synth
    dev = torch.device("cuda")
    obj, pmask = synth.make_object()
    scenes = synth.kitti_like(B, 3, 375, 1242, torch.Generator().manual_seed(scene_seed)).to(dev)
    ctor = {k: attrs.pop(k) for k in ("steps", "host_chain", "region") if k in attrs}
    atk = ta.Phy_obj_atk_guassian(model, obj.to(dev), pmask.to(dev), dist_range=TRAIN_DIST, **ctor)
    atk.trace = []
    for k, v in attrs.items():
        setattr(atk, k, v)
    R.seed_all(seed)
    adv, ben, m, patch = atk(scenes, B, eval=eval)
    return atk, adv, m, patch


@no_miopen
def test_device_loop_equals_the_host_chain():
    model = R.make_model().cuda().eval()
    d, a0, m0, p0 = _run(model, 3, steps=4)
    h, a1, m1, p1 = _run(model, 3, steps=4, host_chain=True)
    assert d.best_index == h.best_index and 0 <= d.best_index < 4
    assert torch.equal(p0, p1) and torch.equal(a0, a1) and torch.equal(m0, m1)
    assert np.array_equal(d.costs, h.costs), np.abs(d.costs - h.costs).max()
    assert d.trace == h.trace and len(d.trace) == 4


@no_miopen
def test_attack_matches_the_reference_fixture(golden):
    """The 10 steps of the reference's own run."""
    from tests.test_gpu_light import _check_costs
    _, ta = _mods()
    g = golden("atk_gauss")
    B, steps, seed = [int(v) for v in g["shape"]]
    obj, mask, scenes = R.case_inputs()
    model = R.make_model().cuda()
    model.train()
    rm = model.bn.running_mean.clone()
    atk = ta.Phy_obj_atk_guassian(model, obj.cuda(), mask.cuda(), steps=steps, dist_range=TRAIN_DIST)
    atk.trace = []
    R.seed_all(seed)
    adv_s, ben_s, m_out, patch = atk(scenes.cuda(), B, eval=True)
    assert model.training and torch.equal(model.bn.running_mean, rm)
    assert len(atk.trace) == steps == len(g["cost"])
    assert np.array_equal(np.array([t["sigma"] for t in atk.trace]), g["sigma"])
    dist, angles = g["dist_range"], np.arange(-30, 31, 5)
    assert np.array_equal(np.array([t["z0"] for t in atk.trace]), dist[g["z0_index"][:steps]])
    assert np.array_equal(np.array([t["alpha"] for t in atk.trace]), angles[g["alpha_index"][:steps]])
    e_ref, gap = float(g["e_ref"]), float(g["gap"])
    _check_costs([t["cost"] for t in atk.trace], g["cost"], e_ref, "fixture")
    if gap >= max(20 * e_ref, 1e-4):        # the fixture's decidability rule (the generator writes no other fixture)
        assert atk.best_index == int(g["best"]), (atk.best_index, int(g["best"]))
    r0, r1, c0, c1 = [int(v) for v in g["region"]]
    _report(patch[:, :, r0:r1, c0:c1], g["patch_rect"], "the winning rectangle")
    assert torch.equal(patch.cpu(), R.with_window(obj, g["patch_rect"]))
    assert_close_frac(m_out[ROWS], np_t(g["mask_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="mask rows")
    assert_close_frac(ben_s[ROWS], np_t(g["ben_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="ben rows")
    torch.testing.assert_close(m_out.double().sum((1, 2, 3)).cpu(), np_t(g["mask_out_sum"]), rtol=1e-5, atol=0)
    assert_close_frac(adv_s[ROWS], np_t(g["adv_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=0.01, name="adv rows")


def _unet(dev, seed=0):
    from depthmodelhardening_amd.depth_model import import_depth_model
    torch.manual_seed(seed)
    model = import_depth_model((1024, 320)).to(dev).eval()
    g = torch.Generator().manual_seed(seed + 1)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(0.1 * torch.randn(m.num_features, generator=g))
            m.running_var.copy_(1 + 0.2 * torch.rand(m.num_features, generator=g))
    return model


def test_windowed_cost_equals_full_frame_cost():
    model = _unet(torch.device("cuda"), seed=2)
    full, _, m0, p0 = _run(model, 12, steps=4, use_roi=False)
    win, _, m1, p1 = _run(model, 12, steps=4)
    rel = np.abs(full.costs - win.costs) / np.abs(full.costs)
    print("windowed vs full-frame cost: largest relative difference %.3g over %d steps" % (rel.max(), len(rel)))
    assert full.best_index == win.best_index, (full.costs, win.costs)
    assert torch.equal(m0, m1) and torch.equal(p0, p1)


@contextlib.contextmanager
def _sync_is_an_error():
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode(before)


def test_no_host_reads_in_the_loop():
    dev = torch.device("cuda")
    with _sync_is_an_error():           # the guard itself works: a host read raises
        with pytest.raises(RuntimeError):
            torch.ones(1, device=dev).item()
    assert torch.cuda.get_sync_debug_mode() == 0
    with torch.backends.cudnn.flags(enabled=False):
        tiny, _, _, _ = _run(R.make_model().cuda().eval(), 2, steps=3, loop_context=_sync_is_an_error)
    unet, _, _, _ = _run(_unet(dev, seed=2), 4, steps=3, loop_context=_sync_is_an_error)
    assert tiny.best_index >= 0 and unet.best_index >= 0 and torch.cuda.get_sync_debug_mode() == 0
    with pytest.raises(RuntimeError):   # the guard sees the loop: the host chain, which reads every cost back, trips it
        with torch.backends.cudnn.flags(enabled=False):
            _run(R.make_model().cuda().eval(), 2, steps=1, host_chain=True, loop_context=_sync_is_an_error)
    assert torch.cuda.get_sync_debug_mode() == 0


# --------------------------------------------------------------------------------------------------------------------- 4. arbi
@no_miopen
def test_arbi_matches_two_consecutive_reference_calls(golden):
    _, ta = _mods()
    g = golden("atk_gauss")
    B = int(g["shape"][0])
    obj, mask, scenes = R.case_inputs()
    atk = ta.Phy_obj_atk_arbi(R.make_model().cuda(), obj.cuda(), mask.cuda(), dist_range=TRAIN_DIST)
    for call in range(2):
        adv_s, ben_s, m_out, patch = atk(scenes.cuda(), B, eval=True)
        assert atk.fills[call] == str(g["arbi_fills"][call])
        assert torch.equal(patch.cpu(), R.with_window(obj, g["arbi%d_rect" % call])), "call %d: the patch" % call
        assert_close_frac(m_out[ROWS], np_t(g["arbi%d_mask_rows" % call]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="mask rows")
        assert_close_frac(ben_s[ROWS], np_t(g["arbi%d_ben_rows" % call]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="ben rows")
        assert_close_frac(adv_s[ROWS], np_t(g["arbi%d_adv_rows" % call]), rtol=1e-4, atol=2e-5, max_bad_frac=0.01, name="adv rows")


# --------------------------------------------------------------------------------------------------------------- 5. evaluation
@no_miopen
def test_evaluate_attacks_runs_the_gaussian_and_the_arbitrary_rows():
    from depthmodelhardening_amd.evaluate_depth import evaluate_attacks
    model = R.make_model().cuda().eval()
    on = {"gradient_free_attacks": True, "batch_size": 2}
    out = evaluate_attacks(model, dict(on, norm_type="guassian", step=3), eval_count=2)
    assert out.shape == (8,) and np.isfinite(out).all()
    out = evaluate_attacks(model, dict(on, norm_type="arbi"), eval_count=2)
    assert out.shape == (8,) and np.isfinite(out).all()
    with pytest.raises(NotImplementedError, match="out of scope"):      # the key serves these two rows only
        evaluate_attacks(model, dict(on, norm_type="Square", epsilon=0.05, n_queries=10), eval_count=1)
    with pytest.raises(NotImplementedError, match="out of scope"):
        evaluate_attacks(model, {"norm_type": "l_2", "epsilon": 0.05, "step": 10, "batch_size": 2}, eval_count=1)


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    ops, ta = _mods()
    from oracle import synth
    dev = torch.device("cuda")
    obj, mask = synth.make_object()
    model = R.make_model().cuda()
    atk = ta.Phy_obj_atk_guassian(model, obj.cuda(), mask.cuda(), dist_range=TRAIN_DIST, steps=1)
    with pytest.raises(RuntimeError, match="Batch size doesn't match"):
        atk(torch.zeros(2, 3, 375, 1242).cuda(), 3)
    atk.shard = (0, 2, None)
    with pytest.raises(NotImplementedError, match="shard"):
        atk(torch.zeros(1, 3, 375, 1242).cuda(), 2)
    with pytest.raises(RuntimeError, match="positive"):
        ta.Phy_obj_atk_guassian(model, obj.cuda(), mask.cuda(), steps=0)
    with pytest.raises(RuntimeError, match="empty"):
        ta.Phy_obj_atk_guassian(model, obj.cuda(), mask.cuda(), steps=1, region=(300, 400, 0, 10))(
            torch.zeros(1, 3, 375, 1242).cuda(), 2)
    arbi = ta.Phy_obj_atk_arbi(model, obj.cuda(), mask.cuda(), dist_range=TRAIN_DIST)
    with pytest.raises(RuntimeError, match="Batch size doesn't match"):
        arbi(torch.zeros(2, 3, 375, 1242).cuda(), 3)
    weights, radii = (torch.from_numpy(v) for v in ops.gauss_blur_table([1.0, 2.0]))
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.gauss_blur_windows(x, weights, radii, (0, 8, 0, 8))
    xd, wd, rd = x.to(dev), weights.to(dev), radii.to(dev)
    with pytest.raises(RuntimeError, match="float64"):
        ops.gauss_blur_windows(xd, wd.float(), rd, (0, 8, 0, 8))
    with pytest.raises(RuntimeError, match="int32"):
        ops.gauss_blur_windows(xd, wd, rd.long(), (0, 8, 0, 8))
    with pytest.raises(RuntimeError, match="int32"):
        ops.gauss_blur_windows(xd, wd, rd[:1], (0, 8, 0, 8))
    with pytest.raises(RuntimeError, match="fp32"):
        ops.gauss_blur_windows(xd.double(), wd, rd, (0, 8, 0, 8))
    with pytest.raises(RuntimeError, match="fp32"):
        ops.gauss_blur_windows(torch.rand(2, 3, 8, 8, device=dev), wd, rd, (0, 8, 0, 8))
    with pytest.raises(RuntimeError, match="empty"):
        ops.gauss_blur_windows(xd, wd, rd, (8, 12, 0, 8))
    with pytest.raises(RuntimeError, match="empty"):
        ops.gauss_blur_windows(xd, wd, rd, (4, 4, 0, 8))
    with pytest.raises(RuntimeError, match="at least one step"):
        ops.gauss_blur_windows(xd, wd[:0], rd[:0], (0, 8, 0, 8))
    with pytest.raises(RuntimeError, match="positive"):
        ops.gauss_blur_table([1.0, 0.0])
    with pytest.raises(RuntimeError, match="at least one step"):
        ops.gauss_sigmas(0, 8, 8)
    win = ops.gauss_blur_windows(xd, wd, rd, (1, 7, 2, 8))
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="windows"):
        ops.gauss_blur_compose(win, idx, xd, (0, 8, 0, 8))
    with pytest.raises(RuntimeError, match="int32"):
        ops.gauss_blur_compose(win, idx.long(), xd, (1, 7, 2, 8))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.gauss_blur_compose(win, idx, xd, (1, 7, 2, 8), out=torch.zeros(1, 3, 8, 9, device=dev))
    with pytest.raises(RuntimeError, match="empty"):
        ops.gauss_blur_compose(win, idx, xd, (9, 7, 2, 8))


# ------------------------------------------------------------------------------------------------------------------- 7. opcheck
def test_opcheck_of_the_gauss_operators():
    ops, _ = _mods()
    dev = torch.device("cuda")
    tests = ("test_schema", "test_faketensor")
    weights, radii = (torch.from_numpy(v).to(dev) for v in ops.gauss_blur_table([0.7, 2.5]))
    obj = torch.rand(1, 3, 16, 24, device=dev)
    torch.library.opcheck(torch.ops.dmh.gauss_blur_windows, (obj, weights, radii, 3, 170, -20, 20), test_utils=tests)
    w1 = torch.ops.dmh.gauss_blur_windows(obj, weights, radii, 3, 170, -20, 20)
    w2 = ops.gauss_blur_windows(obj, weights, radii, (3, 16, 4, 20))
    assert w1.shape == (2, 3, 13, 16) and torch.equal(w1, w2)
    idx = torch.tensor([1], dtype=torch.int32, device=dev)
    out = torch.zeros_like(obj)
    torch.library.opcheck(torch.ops.dmh.gauss_blur_compose, (w1, idx, obj, out, 3, 170, -20, 20), test_utils=tests)
    # the registered ops launch the same kernels as ops.py's wrappers
    o1, o2 = torch.zeros_like(obj), torch.zeros_like(obj)
    torch.ops.dmh.gauss_blur_compose(w1, idx, obj, o1, 3, 170, -20, 20)
    ops.gauss_blur_compose(w2, idx, obj, (3, 16, 4, 20), out=o2)
    assert torch.equal(o1, o2) and torch.equal(o1[:, :, 3:16, 4:20], w1[1:2]) and not torch.equal(o1, obj)
