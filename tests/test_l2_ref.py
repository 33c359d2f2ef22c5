"""The L2 object attack on the CPU: tests/l2_ref.py's fp32 form against the reference's own run at batch_size = 1 in
tests/golden/atk_l2.npz (tools/make_goldens_l2.py), the fixture's record of the reference at batch_size = 2 against what DESIGN.md
section 8 says about it, and the host side of ``Phy_obj_atk_l2``: the ignored ``alpha``, the refused ``shard``, the wiring.

Tolerances of the fixture comparison: the ones tests/test_gpu_attacks.py holds the L_inf golden to -- patch texels within 1e-5 for
more than 99.5 % of them, rows and scalars to rtol 1e-4 / atol 2e-5.
"""
import os

import numpy as np
import pytest
import torch

from oracle import attack_ref
from tests import l2_ref as R
from tests.util import assert_close_frac, np_t

ROWS = (slice(None), slice(None), slice(120, 300, 9), slice(300, 800, 5))
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fp32_form_reproduces_the_reference_fixture(golden):
    g = golden("atk_l2")
    B, steps, seed = [int(v) for v in g["b1_shape"]]
    eps = float(g["b1_eps"])
    assert (B, steps, seed, eps) == (1, R.CASE["steps"], R.CASE["rng_seed"], R.CASE["eps"])
    assert float(g["b1_alpha"]) == R.step_alpha(eps, steps)
    obj, mask, scenes = R.case_inputs(1)
    r0, r1, c0, c1 = [int(v) for v in g["b1_region"]]
    R.seed_all(seed)
    normal, r = R.draw_start(obj)                           # the reference's first two draws from torch's generator
    assert torch.equal(normal[:, :, r0:r1, c0:c1], np_t(g["b1_normal_rect"])) and np.array_equal(r.numpy().reshape(-1), g["b1_r"])
    assert float(normal.double().sum()) == float(g["b1_normal_sum"])
    assert torch.equal(R.random_start(obj, normal, r, eps)[:, :, r0:r1, c0:c1], np_t(g["b1_start_rect"]))
    R.seed_all(seed)                                        # the poses come from Python's generator
    trace = []
    adv_s, ben_s, m_out, patch = R.phy_obj_atk_l2(R.make_model(), obj, mask, scenes, 1, eps=eps, steps=steps,
                                                  random_start_draw=(normal, r), dist_range=list(g["b1_dist_range"]), eval=True,
                                                  trace=trace)
    costs = np.asarray([t["cost"] for t in trace])
    norms = R.norms_of(trace, obj)
    print("costs %s (fixture %s)  norms %s (fixture %s)" % (costs, g["b1_cost"], norms, g["b1_norm"]))
    np.testing.assert_allclose(costs, g["b1_cost"], rtol=1e-4, atol=0)
    np.testing.assert_allclose(norms, g["b1_norm"], rtol=1e-4, atol=2e-5)
    assert (norms <= eps * (1 + 1e-6)).all() and float(patch.min()) >= 0 and float(patch.max()) <= 1
    agree = ((patch[:, :, r0:r1, c0:c1] - np_t(g["b1_patch_rect"])).abs() <= 1e-5).float().mean().item()
    assert agree > 0.995, agree
    np.testing.assert_allclose(patch.double().sum((0, 2, 3)).numpy(), g["b1_patch_sum"], rtol=1e-5)
    assert_close_frac(m_out[ROWS], np_t(g["b1_mask_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="mask rows")
    assert_close_frac(ben_s[ROWS], np_t(g["b1_ben_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="ben rows")
    assert_close_frac(adv_s[ROWS], np_t(g["b1_adv_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=0.01, name="adv rows")
    assert 0 < float(g["b1_e_ref_cost"]) < 1e-3 and 0 < float(g["b1_e_ref_patch"]) < 1e-2


def test_the_reference_at_batch_two_is_what_the_design_says(golden):
    """The class as written does not run with two scenes: after the first step the patch has one row per scene, and the second
    step's paste has B * B images for B masks."""
    g = golden("atk_l2")
    assert bool(g["b2_raised"]) and str(g["b2_exception"]) == "RuntimeError"
    assert g["b2_patch_shapes"].tolist() == [[1, 3, 260, 300], [2, 3, 260, 300]]
    assert int(g["b2_costs_seen"]) == 1 and int(g["b2_steps"]) == 2 and g["b2_returned_shapes"].size == 0
    assert "(4)" in str(g["b2_message"]) and "(2)" in str(g["b2_message"])
    text = " ".join(open(os.path.join(REPO, "DESIGN.md")).read().split())
    assert "raises `RuntimeError` in the second step's composite (4 pasted images against 2 masks)" in text
    assert "broadcasting accident" not in text


def test_step_with_one_row_is_the_reference_expression_at_batch_one():
    """l2_ref.step against the reference's lines written out with batch_size = 1 views, and the quirks: eps / 0 gives factor 1,
    a zero gradient leaves the patch where it is."""
    x, x0, grad, alpha, eps = R.kernel_case("outside", 257)
    want = x + alpha * (grad / (torch.norm(grad.view(1, -1), p=2, dim=1) + 1e-10).view(1))
    d = want - x0
    want = torch.clamp(x0 + d * torch.min(eps / torch.norm(d.view(1, -1), p=2, dim=1), torch.ones(1)).view(-1), 0, 1)
    assert torch.equal(R.step(x, x0, grad, alpha, eps), want)
    x, x0, grad, alpha, eps = R.kernel_case("zero_grad_at_x0", 5)
    out = R.step(x, x0, grad, alpha, eps)
    assert torch.equal(out, x0) and torch.isfinite(out).all()
    x, x0, grad, alpha, eps = R.kernel_case("zero_grad", 1023)
    assert torch.equal(R.step(x, x0, grad, alpha, eps), x)


def test_alpha_is_ignored_shard_is_refused_and_the_row_is_wired():
    from depthmodelhardening_amd import _native, build, library
    from depthmodelhardening_amd import torchattacks as ta
    from depthmodelhardening_amd.torchattacks import attacks
    from oracle import synth
    obj, mask = synth.make_object()
    model = synth.TinyDepthNet()
    atk = ta.Phy_obj_atk_l2(model, obj, mask, eps=8, alpha=123.0, steps=10, dist_range=attack_ref.TRAIN_DIST_RANGE)
    assert isinstance(atk, ta.Phy_obj_atk) and attacks.Phy_obj_atk_l2 is ta.Phy_obj_atk_l2 and "Phy_obj_atk_l2" in ta.__all__
    assert atk.alpha == 2.5 * 8 / 10 and atk.eps == 8 and atk.steps == 10 and atk.eps_for_division == 1e-10
    assert (atk.use_graph, atk.common_windows, atk.use_roi, atk.trace, atk.torch_step, atk.random_start_noise) == (
        False, False, True, None, False, None)
    default = ta.Phy_obj_atk_l2(model, obj, mask)
    assert (default.eps, default.steps, default.alpha, default.random_start) == (1, 40, 2.5 / 40, True)
    atk.shard = (0, 2, None)
    with pytest.raises(NotImplementedError, match="shard"):
        atk(torch.zeros(1, 3, 375, 1242), 2)
    # the start noise from the hook: the reference's expression on the same draws
    torch.manual_seed(3)
    normal, r = R.draw_start(obj)
    atk.random_start_noise = (normal, r)
    assert torch.equal(torch.clamp(obj + atk._random_start(obj), 0, 1), R.random_start(obj, normal, r, 8))
    assert torch.equal(atk.random_start_noise[0], normal)          # the hook's tensor is not written
    # the torch form of the step (the benchmark's baseline) is the twin's
    x, x0, grad, alpha, eps = R.kernel_case("outside", obj.numel())
    t = ta.Phy_obj_atk_l2(model, x0.view_as(obj), mask, eps=eps, steps=5)
    assert torch.equal(t._torch_step(x.view_as(obj), grad.view_as(obj)), R.step(x, x0, grad, t.alpha, eps).view_as(obj))
    assert "dmh_pgd_l2_step" in _native._SIGNATURES and "dmh_pgd_l2_workspace_size" in _native._SIGNATURES
    assert "l2_step.hip" in build.SOURCES and "pgd_l2_step" in library.OPS and hasattr(torch.ops.dmh, "pgd_l2_step")
    lib = _native.lib()
    assert lib.dmh_pgd_l2_workspace_size(0) == 0 and lib.dmh_pgd_l2_workspace_size(1) == 24
    sizes = [lib.dmh_pgd_l2_workspace_size(n) for n in R.KERNEL_SIZES]
    assert sizes == sorted(sizes) and max(sizes) <= 24 * 256 and lib.dmh_pgd_l2_workspace_size(3 * 260 * 300) // 24 <= 256
    assert lib.dmh_pgd_l2_step(None, None, None, 0.1, 0.1, None, 0, None, 0, None) == 1
    from depthmodelhardening_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pgd_l2_step(x, x0, grad, 0.1, 0.1, workspace=torch.zeros(768, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.pgd_l2_step(x, x0[:-1], grad, 0.1, 0.1)
