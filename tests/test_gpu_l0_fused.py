"""K23 (csrc/l0_fused.hip) and Phy_obj_atk_l0's ``fused`` / ``use_graph`` on the GPU: the kernel bit for bit against the fp32
numpy restatement (tests/l0_fused_ref.py) and, with the mask term, against its float64 form; the controller against a Python
replay; the fused attack against the reference's fixture and the CPU oracle; graph replay against the eager loop; the early
exit and the RNG bookkeeping; the trainer's switches; the refusals and the registered operator."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import l0_fused_ref as R  # noqa: E402
from tests.util import no_miopen, np_t  # noqa: E402

TRAIN_DIST = list(np.arange(5, 10, 0.2))
CLIP = 1.0 / 255.0


def _mods():
    from depthmodelhardening_amd import library, ops  # noqa: F401
    from depthmodelhardening_amd import torchattacks as ta
    return ops, ta


def _seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def _inputs(C, HW, seed):
    """obj, pos, neg [C, HW] fp32 with pattern values outside [0, 1] and exactly on the gates' edges."""
    rng = np.random.RandomState(seed)
    obj = rng.rand(C, HW).astype(np.float32)
    pos = (rng.rand(C, HW) * 1.6 - 0.3).astype(np.float32)
    neg = (rng.rand(C, HW) * 1.6 - 0.3).astype(np.float32)
    q = max(HW // 8, 1)
    pos[0, :q], pos[1, q:2 * q], neg[0, 2 * q:3 * q], neg[2 % C, 3 * q:4 * q] = 0.0, 1.0, 0.0, 1.0
    obj[0, ::7], obj[1, 3::11] = 0.0, 1.0
    return obj, pos, neg


class _Dev(object):
    """Device buffers of one K23 state; ``offset``: which of the nine patch-sized tensors sits 4 bytes off 16-byte alignment."""
    NAMES = ("obj", "pos", "neg", "m_pos", "v_pos", "m_neg", "v_neg", "g_adv", "adv")

    def __init__(self, ops, obj, pos, neg, steps, count0, lr, offset=None):
        dev = torch.device("cuda")
        C, HW = obj.shape
        shape = (1, C, 1, HW)
        self.ops, self.steps = ops, steps
        for name in self.NAMES:
            buf = torch.zeros(C * HW + 4, device=dev)
            lo = 1 if name == offset else 0
            setattr(self, name, buf[lo:lo + C * HW].view(shape))
        self.obj.copy_(torch.from_numpy(obj).view(shape))
        self.pos.copy_(torch.from_numpy(pos).view(shape))
        self.neg.copy_(torch.from_numpy(neg).view(shape))
        self.count = torch.zeros(2 * steps + 1, device=dev, dtype=torch.int32)
        self.count[0] = count0
        self.rec = torch.zeros(2 * steps, ops.L0_REC, device=dev)
        self.cursor = torch.zeros(2, device=dev, dtype=torch.int32)
        self.tab = ops.l0_adam_table(steps, lr).to(dev)

    def step(self, g_adv, adv_cost, mask_cost, mask_wt, thresh):
        self.g_adv.copy_(torch.from_numpy(g_adv).view(self.g_adv.shape))
        self.ops.l0_fused_step(self.obj, self.pos, self.neg, self.m_pos, self.v_pos, self.m_neg, self.v_neg, self.g_adv, self.adv,
                               self.count, self.rec, self.cursor, self.tab, adv_cost, mask_cost, self.steps, mask_wt, thresh, CLIP)

    def host(self, name):
        t = getattr(self, name)
        return t.cpu().numpy().reshape(self.obj.shape[1], -1) if name in self.NAMES else t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------- 1. kernel, bit-exact
@pytest.mark.parametrize("C,HW,offset", [(3, 78000, None), (3, 4099, None), (3, 7, None), (3, 78000, "pos"), (3, 4100, "g_adv")])
def test_kernel_without_the_mask_term_is_bit_exact(C, HW, offset):
    ops, _ = _mods()
    dev = torch.device("cuda")
    steps, lr, thresh = 2, 0.5, 0.1
    obj, pos, neg = _inputs(C, HW, HW + (1 if offset else 0))
    _, count0 = R.compose(obj, pos, neg, CLIP)
    assert count0 > 0
    st = R.make_state(pos, neg, steps, count0)
    d = _Dev(ops, obj, pos, neg, steps, count0, lr, offset)
    tab = R.adam_table(steps, lr)
    rng = np.random.RandomState(HW)
    for i in range(3):
        g = rng.randn(C, HW).astype(np.float32)
        g[:, ::5] = 0.0                             # zero gradients
        g[:, 1::9] *= 1e-6                          # and tiny ones: Adam's eps matters there
        cost = np.float32(0.25 + i)
        R.fused_step(st, obj, g, tab, 0.0, thresh, CLIP, adv_cost=cost, mask_cost=np.float32(0.5))
        d.step(g, torch.tensor([cost], device=dev), torch.tensor([0.5], device=dev), 0.0, thresh)
        for name in ("pos", "neg", "m_pos", "v_pos", "m_neg", "v_neg", "adv"):
            got, want = d.host(name), st[name]
            assert np.array_equal(got, want), (name, i, int((got != want).sum()), float(np.abs(got - want).max()))
        assert np.array_equal(d.host("count"), st["count"]) and np.array_equal(d.host("rec"), st["rec"])
        assert d.cursor.tolist() == [i + 1, 0]
    # the comparison is not vacuous: the update moved what the gates let through (outer gate ~0.7 x pattern gate ~0.6 x non-zero
    # gradients 0.8 of the texels)
    assert float(np.mean(st["pos"] != pos)) > 0.2


# ------------------------------------------------------------------------------------------------------- 2. kernel, mask term
def test_kernel_with_the_mask_term_is_as_close_to_float64_as_the_unfused_path():
    """Share of texels farther than 1e-6 from the float64 restatement after three steps: at most 1.5 x the same share of the
    unfused device path (K5 compose, K5 mask cost backward, torch.optim.Adam on the GPU) on the same inputs, plus 1e-4 of the
    texels.  1.5 is tests/util.py's convention for distances measured against a float64 anchor."""
    ops, _ = _mods()
    dev = torch.device("cuda")
    C, H, W, steps, lr, mask_wt, thresh = 3, 260, 300, 2, 0.5, 0.06, 0.1
    HW = H * W
    obj, pos, neg = _inputs(C, HW, 17)
    _, count0 = R.compose(obj, pos, neg, CLIP)
    rng = np.random.RandomState(3)
    grads = [(10.0 ** rng.uniform(-3, 0, (C, HW)) * rng.choice([-1.0, 1.0], (C, HW))).astype(np.float32) for _ in range(3)]
    st64 = R.make_state(pos, neg, steps, count0, dtype=np.float64)
    tab = R.adam_table(steps, lr)
    d = _Dev(ops, obj, pos, neg, steps, count0, lr)
    shape = (1, C, H, W)
    tp = torch.from_numpy(pos).view(shape).to(dev).requires_grad_(True)
    tn = torch.from_numpy(neg).view(shape).to(dev).requires_grad_(True)
    to = torch.from_numpy(obj).view(shape).to(dev)
    opt = torch.optim.Adam([tp, tn], lr=lr, betas=(0.5, 0.9))
    cost = torch.tensor([0.5], device=dev)
    for i, g in enumerate(grads):
        R.fused_step(st64, obj.astype(np.float64), g.astype(np.float64), tab, mask_wt, thresh, CLIP, dtype=np.float64)
        assert float(st64["rec"][i][1]) == mask_wt          # the mask term is on in every step
        d.step(g, cost, None, mask_wt, thresh)
        adv, _ = ops.l0_compose(to, tp, tn, CLIP)
        mc = ops.l0_mask_cost(tp, tn)
        g_pos, g_neg = torch.autograd.grad([adv, mc], [tp, tn],
                                           grad_outputs=[torch.from_numpy(g).view(shape).to(dev), torch.tensor(mask_wt, device=dev)])
        tp.grad, tn.grad = g_pos, g_neg
        opt.step()
    assert np.array_equal(d.host("rec")[:3, 1], np.full(3, np.float32(mask_wt)))
    far = {}
    for label, got_p, got_n in (("fused", d.host("pos"), d.host("neg")),
                                ("unfused", tp.detach().cpu().numpy().reshape(C, HW), tn.detach().cpu().numpy().reshape(C, HW))):
        diff = np.concatenate([np.abs(got_p.astype(np.float64) - st64["pos"]), np.abs(got_n.astype(np.float64) - st64["neg"])])
        far[label] = float(np.mean(diff > 1e-6))
        print("%s: share of texels farther than 1e-6 from float64: %.6g (max distance %.3g)" % (label, far[label], diff.max()))
    assert far["fused"] <= 1.5 * far["unfused"] + 1e-4, far


# ------------------------------------------------------------------------------------------------------------ 3. controller
def _controller_case(HW):
    """Patterns and per-iteration gradients that take the count below thresh * count[0] and back above it: group A (40 % of
    the pixels) starts on and is switched off by iteration 0, group B (30 %) starts on and gets no gradient, group C (30 %)
    starts just below the 1/255 threshold and is switched on by iteration 1.  The negative pattern sits outside its gate."""
    C = 3
    a, b = int(0.4 * HW), int(0.7 * HW)
    obj = np.full((C, HW), 0.2, dtype=np.float32)
    pos = np.full((C, HW), 0.45, dtype=np.float32)
    pos[:, b:] = 0.001
    neg = np.full((C, HW), -0.5, dtype=np.float32)
    g0, g1 = np.zeros((C, HW), dtype=np.float32), np.zeros((C, HW), dtype=np.float32)
    g0[:, :a] = 1.0
    g1[:, b:] = -1.0
    return obj, pos, neg, [g0, g1]


@pytest.mark.parametrize("steps", [1, 3, 10])
def test_controller_matches_a_python_replay(steps):
    ops, _ = _mods()
    from depthmodelhardening_amd.torchattacks.attacks.phy_obj_atk_l0 import host_below
    dev = torch.device("cuda")
    HW, mask_wt, thresh, lr = 1031, 0.06, 0.5, 0.5
    obj, pos, neg, grads = _controller_case(HW)
    _, count0 = R.compose(obj, pos, neg, CLIP)
    d = _Dev(ops, obj, pos, neg, steps, count0, lr)
    zero = np.zeros_like(obj)
    ran, exited = 0, False
    for stp in range(2 * steps):
        if stp >= steps and host_below(d.host("count"), stp, thresh):       # the attack's host-side exit
            exited = True
            break
        d.step(grads[stp] if stp < len(grads) else zero, torch.tensor([float(stp)], device=dev), None, mask_wt, thresh)
        ran += 1
    counts, rec = d.host("count"), d.host("rec")
    print("steps %d: counts %s, ran %d, exited %s" % (steps, counts.tolist(), ran, exited))
    mws, want_exit = R.replay_controller(counts, steps, mask_wt, thresh)
    assert (len(mws), want_exit) == (ran, exited)
    assert np.array_equal(rec[:ran, 1], np.asarray(mws, dtype=np.float32))
    assert np.array_equal(rec[:ran, 0], counts[:ran].astype(np.float32)) and rec[:ran, 4].tolist() == list(range(1, ran + 1))
    assert np.array_equal(rec[:ran, 2], np.arange(ran, dtype=np.float32)) and not rec[ran:].any()
    assert d.cursor.tolist() == [ran, 0]
    # the case does what it is for: on at iteration 0, below the threshold at iteration 1 and, where it runs, above it again
    assert counts[0] == int(0.7 * HW) and rec[0, 1] == np.float32(mask_wt) and counts[1] * 2 <= counts[0]
    if steps == 1:
        assert exited and ran == 1
    else:
        assert rec[1, 1] == 0.0 and counts[2] * 2 > counts[0] and rec[2, 1] == np.float32(mask_wt)


def test_cursor_outside_the_attack_changes_nothing():
    ops, _ = _mods()
    dev = torch.device("cuda")
    steps = 3
    obj, pos, neg = _inputs(3, 1000, 4)
    d = _Dev(ops, obj, pos, neg, steps, 900, 0.5)
    g = np.ones_like(obj)
    for cur in (2 * steps, -1, 1 << 20):
        d.cursor.copy_(torch.tensor([cur, 0], dtype=torch.int32))
        before = {n: getattr(d, n).clone() for n in _Dev.NAMES + ("count", "rec")}
        d.step(g, torch.tensor([1.0], device=dev), None, 0.06, 0.1)
        before["g_adv"] = d.g_adv.clone()
        assert all(torch.equal(getattr(d, n), v) for n, v in before.items()) and d.cursor.tolist() == [cur, 0]


# ------------------------------------------------------------------------------------- 4. the attack vs the reference's fixture
def _setup():
    _, ta = _mods()
    from oracle import attack_ref, synth
    obj, mask = synth.make_object()
    return ta, attack_ref, synth, obj, mask


def test_fused_attack_matches_reference_golden(golden):
    """The gates of tests/test_gpu_attacks.py::test_phy_obj_atk_l0_matches_reference_golden, with ``fused`` on."""
    ta, attack_ref, synth, obj, mask = _setup()
    g = golden("atk_l0")
    Ba, steps, seed = [int(v) for v in g["shape"]]
    scenes = synth.kitti_like(Ba, 3, 375, 1242, torch.Generator().manual_seed(31))
    model = synth.TinyDepthNet(seed=5).cuda()
    atk = ta.Phy_obj_atk_l0(model, obj.cuda(), mask.cuda(), adam_lr=0.5, steps=steps, mask_wt=0.06, l0_thresh=0.1,
                            dist_range=TRAIN_DIST)
    atk.fused = True
    atk.trace = []
    _seed_all(seed)
    adv_s, ben_s, m_out, patch = atk(scenes.cuda(), Ba)
    assert len(atk.trace) >= steps and atk.records is not None
    assert abs(atk.mask_weight - float(g["final_mask_weight"])) < 1e-7
    assert abs(int(atk.cal_l0()) - int(g["l0_final"])) <= 5
    for name, t in (("pattern_pos_sub", atk.pattern_pos_tensor), ("pattern_neg_sub", atk.pattern_neg_tensor)):
        ref = np_t(g[name])
        agree = ((t[:, :, ::2, ::2].detach().cpu() - ref).abs() <= 2e-3).float().mean().item()
        print("%s: share of texels within 2e-3 of the reference: %.5f" % (name, agree))
        assert agree > 0.99, (name, agree)
    ref = np_t(g["patch_sub"])
    assert ((patch[:, :, ::2, ::2].cpu() - ref).abs() <= 2e-3).float().mean().item() > 0.99
    torch.testing.assert_close(m_out.double().sum((1, 2, 3)).cpu(), np_t(g["mask_out_sum"]), rtol=1e-5, atol=0)
    torch.testing.assert_close(ben_s.double().sum((2, 3)).cpu(), np_t(g["ben_sum"]), rtol=1e-5, atol=0)
    torch.testing.assert_close(adv_s.double().sum((2, 3)).cpu(), np_t(g["adv_sum"]), rtol=1e-3, atol=0)


def test_fused_attack_trace_vs_oracle():
    """The gates of tests/test_gpu_attacks.py::test_l0_attack_trace_vs_oracle, the trace read from K23's record array."""
    ta, attack_ref, synth, obj, mask = _setup()
    scenes = synth.kitti_like(2, 3, 375, 1242, torch.Generator().manual_seed(8))
    rec = []
    _seed_all(21)
    attack_ref.phy_obj_atk_l0(synth.TinyDepthNet(seed=5), obj, mask, scenes, 2, adam_lr=0.5, steps=2, mask_wt=0.06,
                              l0_thresh=0.1, dist_range=attack_ref.TRAIN_DIST_RANGE, record=rec)
    atk = ta.Phy_obj_atk_l0(synth.TinyDepthNet(seed=5).cuda(), obj.cuda(), mask.cuda(), adam_lr=0.5, steps=2,
                            mask_wt=0.06, l0_thresh=0.1, dist_range=TRAIN_DIST)
    atk.fused = True
    atk.trace = []
    _seed_all(21)
    atk(scenes.cuda(), 2)
    assert len(atk.trace) == len(rec)
    for (l0, mw, ac, mc), (l0r, mwr, acr, mcr) in zip(atk.trace, rec):
        assert abs(l0 - l0r) <= max(3, 1e-3 * l0r) and abs(mw - mwr) < 1e-7
        assert abs(ac - acr) <= 1e-3 * abs(acr) + 1e-7 and abs(mc - mcr) <= 1e-4 * abs(mcr)


# ------------------------------------------------------------------------------------------------------- 5. graph = eager
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


def _unet_attack(model, steps, B=4, **attrs):
    _, ta = _mods()
    from oracle import synth
    dev = torch.device("cuda")
    obj, pmask = synth.make_object()
    scenes = synth.kitti_like(B, 3, 375, 1242, torch.Generator().manual_seed(8)).to(dev)
    atk = ta.Phy_obj_atk_l0(model, obj.to(dev), pmask.to(dev), adam_lr=0.5, steps=steps, mask_wt=0.06, l0_thresh=0.1,
                            dist_range=TRAIN_DIST)
    for k, v in attrs.items():
        setattr(atk, k, v)
    _seed_all(13)
    out = atk(scenes, B)
    return atk, out


def test_graph_replay_equals_the_eager_loop():
    model = _unet(torch.device("cuda"), seed=2)
    eager, out0 = _unet_attack(model, 3, fused=True, common_windows=True)
    graph, out1 = _unet_attack(model, 3, use_graph=True)
    assert graph.graph_failure is None and graph.use_graph and graph.graph_replays == graph.total_iterations - 1 >= 2
    assert eager.graph_replays == 0 and eager.total_iterations == graph.total_iterations

    def same(a, oa, b, ob):
        assert torch.equal(a.pattern_pos_tensor, b.pattern_pos_tensor) and torch.equal(a.pattern_neg_tensor, b.pattern_neg_tensor)
        assert all(torch.equal(x, y) for x, y in zip(oa, ob))
        assert torch.equal(a.records, b.records)
    same(eager, out0, graph, out1)
    assert float(eager.records[:eager.total_iterations, 2].abs().min()) > 0        # the records hold the costs
    # a capture that fails after the whole iteration was traced hands the attack back to the eager loop, with the reason kept
    failed, out2 = _unet_attack(model, 3, use_graph=True, _capture_fault=True)
    assert failed.graph_failure is not None and "injected" in failed.graph_failure and not failed.use_graph
    assert failed.graph_replays == 0
    same(eager, out0, failed, out2)


# ---------------------------------------------------------------------------------------------------- 6. early exit and RNG
@no_miopen
def test_early_exit_and_rng_bookkeeping():
    """l0_thresh = 1: the ratio 1 <= 1 holds from iteration 0 on, the mask weight is 0 throughout and the loop ends at
    stp == steps; ``random`` continues exactly where the unfused attack leaves it."""
    ta, attack_ref, synth, obj, mask = _setup()
    scenes = synth.kitti_like(2, 3, 375, 1242, torch.Generator().manual_seed(8)).cuda()
    after = {}
    for fused in (False, True):
        atk = ta.Phy_obj_atk_l0(synth.TinyDepthNet(seed=5).cuda(), obj.cuda(), mask.cuda(), adam_lr=0.5, steps=3, mask_wt=0.06,
                                l0_thresh=1.0, dist_range=TRAIN_DIST)
        atk.fused = fused
        atk.trace = []
        _seed_all(29)
        atk(scenes, 2)
        after[fused] = (random.random(), atk.total_iterations, [t[1] for t in atk.trace], atk.mask_weight)
    assert after[True][1] == 3 and after[True][2] == [0.0, 0.0, 0.0] and after[True][3] == 0.0
    assert after[True] == after[False]


# ----------------------------------------------------------------------------------------------------------- 7. trainer, opcheck
def test_trainer_graph_attack_with_l0(tmp_path):
    """One step of --adv_train --norm_type l_0 --graph_attack: finite loss; and the attack's patch equals the --atk_fused_l0
    run's bit for bit.  The graph needs one set of window sizes for all iterations, so its eager twin is the fused attack on
    the same common-size windows (``common_windows``, as in test_graph_replay_equals_the_eager_loop): the trainers' own first
    attacks run on different windows, and the compared attack is one more on both, from the same seeds."""
    from depthmodelhardening_amd.options import MonodepthOptions
    from depthmodelhardening_amd.trainer import Trainer
    patches = {}
    for flag in ("--graph_attack", "--atk_fused_l0"):
        argv = ["--dataset", "synthetic", "--frame_ids", "0", "--use_stereo", "--height", "64", "--width", "192",
                "--batch_size", "2", "--weights_init", "scratch", "--log_dir", str(tmp_path), "--model_name", "t",
                "--synthetic_len", "8", "--atk_steps", "2", "--atk_batch_size", "2", "--adv_train", "--norm_type", "l_0", flag]
        _seed_all(3)
        tr = Trainer(MonodepthOptions().parse(argv), device=torch.device("cuda"))
        atk = tr.dataset.depth_atk
        assert atk.fused and atk.use_graph == (flag == "--graph_attack") and atk.graph_failure is None
        atk.common_windows = True
        tr.dataset.rng.seed(5)
        _seed_all(7)
        tr.update_adv_obj()
        patches[flag] = tr.dataset.obj_img_adv.clone()
        if flag == "--graph_attack":
            assert atk.graph_failure is None and atk.graph_replays >= 1
            tr.set_train()
            losses = tr.train_step()
            assert torch.isfinite(losses["loss"]) and float(losses["loss"]) > 0
    assert torch.equal(patches["--graph_attack"], patches["--atk_fused_l0"])
    assert float((patches["--graph_attack"] - tr.dataset.obj_img_ben).abs().max()) > 0


def test_opcheck_of_the_fused_operator():
    ops, _ = _mods()
    dev = torch.device("cuda")
    obj, pos, neg = _inputs(3, 516, 2)
    d = _Dev(ops, obj, pos, neg, 2, 400, 0.5)
    d.g_adv.copy_(torch.randn(d.g_adv.shape, generator=torch.Generator().manual_seed(1)))
    args = lambda s: (s.obj, s.pos, s.neg, s.m_pos, s.v_pos, s.m_neg, s.v_neg, s.g_adv, s.adv, s.count, s.rec, s.cursor,      # noqa: E731
                      s.tab, torch.tensor([0.5], device=dev), None, 2, 0.06, 0.1, CLIP)
    torch.library.opcheck(torch.ops.dmh.l0_fused_step, args(d), test_utils=("test_schema", "test_faketensor"))
    # the registered op launches the same kernel as ops.py's wrapper
    a, b = _Dev(ops, obj, pos, neg, 2, 400, 0.5), _Dev(ops, obj, pos, neg, 2, 400, 0.5)
    a.g_adv.copy_(d.g_adv)
    b.g_adv.copy_(d.g_adv)
    torch.ops.dmh.l0_fused_step(*args(a))
    ops.l0_fused_step(*args(b))
    assert all(torch.equal(getattr(a, n), getattr(b, n)) for n in _Dev.NAMES + ("count", "rec", "cursor"))
    assert a.cursor.tolist() == [1, 0] and not torch.equal(a.pos.cpu().view(3, -1), torch.from_numpy(pos))


# ------------------------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals():
    ops, ta = _mods()
    from oracle import synth
    dev = torch.device("cuda")
    obj, mask = synth.make_object()
    model = synth.TinyDepthNet(seed=5).cuda()
    scenes = torch.zeros(1, 3, 375, 1242, device=dev)

    def make(**attrs):
        atk = ta.Phy_obj_atk_l0(model, obj.cuda(), mask.cuda(), steps=2, dist_range=TRAIN_DIST)
        for k, v in attrs.items():
            setattr(atk, k, v)
        return atk
    for attrs in ({"fused": True}, {"use_graph": True}):
        with pytest.raises(NotImplementedError, match="shard"):
            make(shard=(0, 2, None), **attrs)(scenes, 2)
    with pytest.raises(NotImplementedError, match="color_jit"):
        make(use_graph=True)(scenes, 2, color_jit=True)
    with pytest.raises(NotImplementedError, match="grad_trace"):
        make(fused=True, grad_trace=[])(scenes, 2)
    _seed_all(1)
    out = make(fused=True)(scenes, 2, color_jit=True)       # fused alone works with the colour augmentation
    assert tuple(out[0].shape) == (2, 3, 320, 1024) and float((out[3] - obj.cuda()).abs().max()) > 0
    # the wrapper's own checks
    o, p, n = _inputs(3, 64, 1)
    d = _Dev(ops, o, p, n, 2, 50, 0.5)
    cost = torch.tensor([0.5], device=dev)
    base = [d.obj, d.pos, d.neg, d.m_pos, d.v_pos, d.m_neg, d.v_neg, d.g_adv, d.adv, d.count, d.rec, d.cursor, d.tab, cost, None, 2,
            0.06, 0.1, CLIP]

    def call(**change):
        a = list(base)
        names = ["obj", "pos", "neg", "m_pos", "v_pos", "m_neg", "v_neg", "g_adv", "adv", "count", "rec", "cursor", "tab", "adv_cost",
                 "mask_cost", "steps"]
        for k, v in change.items():
            a[names.index(k)] = v
        return ops.l0_fused_step(*a)
    with pytest.raises(RuntimeError, match="different buffers"):
        call(m_pos=d.pos)
    with pytest.raises(RuntimeError, match="records"):
        call(steps=5, count=torch.zeros(11, device=dev, dtype=torch.int32), tab=torch.zeros(10, 2, device=dev))
    with pytest.raises(RuntimeError, match="count"):
        call(steps=5)
    with pytest.raises(RuntimeError, match="steps"):
        call(steps=0)
    with pytest.raises(RuntimeError, match="CUDA"):
        call(obj=d.obj.cpu())
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(rec=torch.zeros(2 * 2 * ops.L0_REC + 1, device=dev)[1:])
    assert d.cursor.tolist() == [0, 0]
