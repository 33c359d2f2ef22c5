"""tests/l0_fused_ref (the numpy restatement of K23, the fused L0 update) against torch.optim.Adam driven through autograd in
float64, the bias-correction table, and the host-side plumbing of the fused attack."""
import math

import numpy as np
import torch

from tests import l0_fused_ref as R


def test_restatement_in_float64_is_adam_on_the_autograd_gradients():
    """Formula equivalence: five iterations with the mask weight toggling, to rtol 1e-12 (four orders above double rounding of
    the dozen operations of one update)."""
    from oracle import attack_ref
    rng = np.random.RandomState(5)
    C, H, W, steps, lr, mask_wt, thresh, clip = 3, 8, 12, 3, 0.5, 0.06, 0.1, 1.0 / 255.0
    hw = H * W
    obj = rng.rand(C, hw)
    pos, neg = rng.rand(C, hw) * 1.6 - 0.3, rng.rand(C, hw) * 1.6 - 0.3      # values outside [0, 1] too
    pos[0, :4], pos[1, 4:8], neg[0, 8:12], neg[2, 12:16] = 0.0, 1.0, 0.0, 1.0   # on the gates' edges
    obj[0, :2], obj[1, 16:18] = 0.0, 1.0
    st = R.make_state(pos, neg, steps, 100, dtype=np.float64)
    tab = R.adam_table(steps, lr)
    tp = torch.tensor(pos.reshape(1, C, H, W), dtype=torch.float64, requires_grad=True)
    tn = torch.tensor(neg.reshape(1, C, H, W), dtype=torch.float64, requires_grad=True)
    to = torch.tensor(obj.reshape(1, C, H, W), dtype=torch.float64)
    opt = torch.optim.Adam([tp, tn], lr=lr, betas=(0.5, 0.9))
    seen = set()
    for i in range(5):
        st["count"][i] = 100 if i % 2 == 0 else 7        # ratio 1 / 0.07 against thresh 0.1: the mask weight toggles
        g_adv = rng.randn(C, hw)
        R.fused_step(st, obj, g_adv, tab, mask_wt, thresh, clip, dtype=np.float64)
        mw = float(st["rec"][i][1])
        seen.add(mw)
        adv = torch.clamp(to + (torch.clamp(tp, 0.0, 1.0) - torch.clamp(tn, 0.0, 1.0)), 0.0, 1.0)
        total = (adv * torch.tensor(g_adv.reshape(1, C, H, W))).sum() + mw * attack_ref.l0_mask_cost(tp, tn)
        opt.zero_grad()
        total.backward()
        opt.step()
        np.testing.assert_allclose(st["pos"], tp.detach().numpy().reshape(C, hw), rtol=1e-12, atol=0)
        np.testing.assert_allclose(st["neg"], tn.detach().numpy().reshape(C, hw), rtol=1e-12, atol=0)
        want_adv = torch.clamp(to + (torch.clamp(tp, 0.0, 1.0) - torch.clamp(tn, 0.0, 1.0)), 0.0, 1.0).detach()
        np.testing.assert_allclose(st["adv"], want_adv.numpy().reshape(C, hw), rtol=1e-12, atol=0)
        assert st["count"][i + 1] == int(attack_ref.cal_l0(torch.clamp(tp, 0.0, 1.0), -torch.clamp(tn, 0.0, 1.0), clip))
        st["count"][i + 1] = 0
    assert seen == {0.0, mask_wt} and st["cursor"] == 5
    assert [int(r[4]) for r in st["rec"][:5]] == [1, 2, 3, 4, 5]


def test_bias_correction_table():
    from depthmodelhardening_amd import ops
    for steps, lr in ((1, 0.5), (10, 0.5), (3, 0.1)):
        tab = ops.l0_adam_table(steps, lr)
        assert tab.dtype == torch.float32 and tuple(tab.shape) == (2 * steps, 2)
        want = np.asarray([(lr / (1 - 0.5 ** t), math.sqrt(1 - 0.9 ** t)) for t in range(1, 2 * steps + 1)])
        assert np.array_equal(tab.numpy(), want.astype(np.float32))
        assert np.array_equal(R.adam_table(steps, lr), want)


def test_controller_replay_and_host_decision_agree():
    from depthmodelhardening_amd.torchattacks.attacks.phy_obj_atk_l0 import host_below
    counts = np.array([1000, 1000, 100, 101, 99, 0, 100, 5000, 3], dtype=np.int32)
    for thresh in (0.1, 0.5, 1.0, 0.0):
        for i in range(len(counts)):
            assert host_below(counts, i, thresh) == R.below(counts[i], counts[0], thresh)
    assert host_below(np.array([0, 0]), 1, 0.1) is False                     # 0 / 0: the mask weight stays on
    mws, exited = R.replay_controller(counts, 4, 0.06, 0.1)
    assert exited and [float(m) for m in mws] == [np.float32(0.06)] * 2 + [0.0, np.float32(0.06)]
    mws, exited = R.replay_controller(np.full(9, 50), 4, 0.06, 0.1)
    assert not exited and len(mws) == 8


def test_native_lists_the_fused_step_and_the_library_the_operator():
    from depthmodelhardening_amd import _native, build, library
    assert "dmh_l0_fused_step" in _native._SIGNATURES and "l0_fused.hip" in build.SOURCES
    assert "l0_fused_step" in library.OPS and hasattr(torch.ops.dmh, "l0_fused_step")


def test_graph_attack_with_l0_parses_and_passes_the_option_check():
    from depthmodelhardening_amd.options import MonodepthOptions
    from depthmodelhardening_amd.trainer import attack_switches
    base = ["--dataset", "synthetic", "--adv_train"]
    o = MonodepthOptions().parse(base + ["--norm_type", "l_0", "--graph_attack"])
    assert attack_switches(o) == {"fused": True, "use_graph": True}
    o = MonodepthOptions().parse(base + ["--norm_type", "l_0", "--atk_fused_l0"])
    assert o.atk_fused_l0 and attack_switches(o) == {"fused": True}
    o = MonodepthOptions().parse(base + ["--norm_type", "l_inf", "--graph_attack"])
    assert attack_switches(o) == {"use_graph": True}
    assert attack_switches(MonodepthOptions().parse(base + ["--norm_type", "l_0"])) == {}
    import pytest
    with pytest.raises(NotImplementedError, match="atk_fused_l0"):
        attack_switches(MonodepthOptions().parse(base + ["--norm_type", "l_inf", "--atk_fused_l0"]))


def test_attack_object_defaults_are_off():
    from depthmodelhardening_amd.torchattacks import Phy_obj_atk_l0
    from oracle import synth
    obj, mask = synth.make_object()
    atk = Phy_obj_atk_l0(synth.TinyDepthNet(seed=5), obj, mask, steps=2, dist_range=list(np.arange(5, 10, 0.2)))
    assert atk.fused is False and atk.use_graph is False and atk.common_windows is False and atk.graph_failure is None
