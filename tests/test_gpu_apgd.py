"""K22 and Phy_obj_atk_APGD on the GPU: the step kernel bit for bit, the controller alone against a Python replay, the whole
attack against the reference's fixture (tests/golden/atk_apgd.npz) and against the CPU restatement (tests/apgd_ref.py), the
HIP-graph form, the refusals and the evaluation entry."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import apgd_ref as R  # noqa: E402
from tests.util import assert_close_frac, no_miopen, np_t  # noqa: E402

ROWS = (slice(None), slice(None), slice(120, 300, 9), slice(300, 800, 5))
TRAIN_DIST = list(np.arange(5, 10, 0.2))
# the losses of a 10-step run on TinyDepthNet(seed=5) at eps = 0.1: successive values differ by 1e-5 relative and less
FLAT_RUN = [-0.00363451, -0.00363172, -0.0036308, -0.00363049, -0.00363039, -0.00363034, -0.00363033, -0.00363033, -0.00363031,
            -0.0036303]


def _mods():
    from depthmodelhardening_amd import library, ops  # noqa: F401
    from depthmodelhardening_amd import torchattacks as ta
    return ops, ta


# ---------------------------------------------------------------------------------------------------------------- 1. step kernel
def _step_expr(x, xo, x0, g, ss, a, eps):
    """phy_obj_atk_apgd.py:207-215, op by op, on the tensors' device."""
    grad2 = x - xo
    x1 = x + ss * torch.sign(g)
    x1 = torch.clamp(torch.min(torch.max(x1, x0 - eps), x0 + eps), 0.0, 1.0)
    return torch.clamp(torch.min(torch.max(x + (x1 - x) * a + grad2 * (1 - a), x0 - eps), x0 + eps), 0.0, 1.0)


@pytest.mark.parametrize("n,offset", [(3 * 260 * 300, 0), (4099, 0), (4099, 1), (7, 3)])
@pytest.mark.parametrize("a", [1.0, 0.75])
def test_step_kernel_is_bit_exact(n, offset, a):
    ops, _ = _mods()
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(n + offset)
    for eps, ss in ((0.1, 0.2), (0.05, 0.025), (8 / 255, 8 / 255 / 4), (0.2, 0.4)):
        x0 = torch.rand(n + offset, generator=gen)
        x = (x0 + (torch.rand(n + offset, generator=gen) * 2 - 1) * eps).clamp(0, 1)
        xo = (x0 + (torch.rand(n + offset, generator=gen) * 2 - 1) * eps).clamp(0, 1)
        g = torch.randn(n + offset, generator=gen)
        q = (n + offset) // 8
        x[:q] = (x0[:q] + eps).clamp(0, 1)              # on the clamp edges: x0 + eps, x0 - eps, 0, 1
        x[q:2 * q] = (x0[q:2 * q] - eps).clamp(0, 1)
        x0[2 * q:2 * q + q // 2], x[2 * q:2 * q + q // 2] = 0.0, 0.0
        x0[2 * q + q // 2:3 * q], x[2 * q + q // 2:3 * q] = 1.0, 1.0
        g[::5] = 0.0                                    # zero gradients: sign() = 0
        x0, x, xo, g = (v.to(dev)[offset:] for v in (x0, x, xo, g))     # offset != 0: a mis-aligned view, scalar form
        ss32 = float(torch.tensor(ss, dtype=torch.float32))
        want = _step_expr(x, xo, x0, g, torch.full((1,), ss32, device=dev), a, eps)
        ctl = torch.zeros(4, ops.APGD_REC, device=dev)
        ctl[2, 0], ctl[2, 1] = ss32, a
        cursor = torch.tensor([2, -1], device=dev, dtype=torch.int32)
        x_in = x.clone()
        ops.apgd_step(x, xo, x0, g, ctl, cursor, 3, eps)        # in place, on the (possibly mis-aligned) views themselves
        assert torch.equal(x, want), (n, offset, a, eps, float((x - want).abs().max()))
        assert torch.equal(xo, x_in) and cursor.tolist() == [2, 2]
        assert float((x != x_in).float().mean()) > 0.3      # the step moved the patch: the comparison above is not vacuous


def test_step_and_commit_outside_the_attack_do_nothing():
    """A cursor beyond the last iteration (a graph replayed once too often) must not index anything."""
    ops, _ = _mods()
    dev = torch.device("cuda")
    x = torch.rand(1000, device=dev)
    bufs = [x.clone() for _ in range(6)]
    ctl, hist, cursor, sd, sm = ops.apgd_controller(3, 0.1, torch.tensor([-1.0], device=dev))
    for cur in ([3, 3], [-1, -1], [1 << 20, 1 << 20]):
        cursor.copy_(torch.tensor(cur, dtype=torch.int32))
        before = ctl.clone()
        ops.apgd_step(bufs[0], bufs[1], bufs[2], bufs[3], ctl, cursor, 3, 0.1)
        ops.apgd_commit(bufs[0], bufs[3], bufs[4], bufs[5], bufs[1], bufs[2], torch.tensor([0.5], device=dev), ctl, hist, cursor, 3,
                        sd, sm)
        assert all(torch.equal(b, x) for b in bufs) and torch.equal(ctl, before) and cursor.tolist() == cur


# ------------------------------------------------------------------------------------------------------------------ 2. controller
def _replay(losses, steps, eps, loss0, rho=0.75):
    """Points 5-7 of the attack's controller in plain Python on fp32 numbers: per iteration (step size used, k used, moved,
    checkpoint, reduced, rose, loss_best after) and which iteration's x / grad the buffers hold afterwards."""
    f = np.float32
    k, steps_min, size_decr = max(int(0.22 * steps), 1), max(int(0.06 * steps), 1), max(int(0.03 * steps), 1)
    hist = np.zeros(steps, dtype=f)
    step, best, best_chk, red_last, cnt = f(f(eps) * f(2)), f(loss0), f(loss0), True, 0
    x_id, g_id, xb_id, gb_id = -1, -1, -1, -1       # -1 = the start point
    out = []
    for i in range(steps):
        x_id, g_id = i, i                           # the step wrote iterate i, the backward pass gradient i
        loss = f(losses[i])
        hist[i] = loss
        moved = bool(loss > best)
        if moved:
            best, xb_id, gb_id = loss, i, i
        cnt += 1
        chk, red, rose = cnt == k, False, 0
        row = (step, k)
        if chk:
            for c in range(k):
                rose += int(hist[i - c] > hist[i - c - 1])      # numpy wraps row -1 to the last row
            red = bool(rose <= k * rho) or ((not red_last) and bool(best_chk >= best))
            red_last, best_chk = red, best
            if red:
                step = f(step / f(2))
                x_id, g_id = xb_id, gb_id
            cnt, k = 0, max(k - size_decr, steps_min)
        out.append(dict(step=row[0], k=row[1], moved=moved, chk=chk, red=red, rose=rose, best=best, ret=i, x=x_id, g=g_id,
                        xb=xb_id, gb=gb_id))
    return out


def _sequences(steps, golden):
    rng = np.random.RandomState(steps)
    seqs = {"rising": np.linspace(-1.0, -0.1, steps), "falling": np.linspace(-0.1, -1.0, steps),
            "alternating": np.array([-0.5 + 0.1 * (-1) ** i - 0.001 * i for i in range(steps)]),
            "flat with ties": np.full(steps, -0.25), "ties then a rise": np.array([-0.25] * (steps - 1) + [-0.2]),
            "random": -rng.rand(steps), "positive": rng.rand(steps) - 0.3}
    if steps == 10:
        seqs["fixture"] = golden("atk_apgd")["loss_steps"]
        seqs["flat run"] = np.array(FLAT_RUN)
    return seqs


@pytest.mark.parametrize("steps", [1, 3, 10, 100])
def test_controller_alone_matches_a_python_replay(steps, golden):
    ops, _ = _mods()
    dev = torch.device("cuda")
    n, eps = 1031, 0.1
    for name, seq in _sequences(steps, golden).items():
        seq = np.asarray(seq, dtype=np.float32)
        for loss0 in (float(seq[0]) - 0.05, float(seq[0]), float(seq.max()) + 1.0):
            want = _replay(seq, steps, eps, loss0)
            ctl, hist, cursor, sd, sm = ops.apgd_controller(steps, eps, torch.tensor([loss0], device=dev))
            # tensors whose values name the iteration that wrote them (-1: the start point)
            x0 = torch.full((n,), 0.5, device=dev)
            x_adv, x_old, grad = torch.full((n,), -1.0, device=dev), torch.full((n,), -1.0, device=dev), torch.full((n,), -1.0, device=dev)
            x_best, grad_best, x_ret = x_adv.clone(), grad.clone(), x_adv.clone()
            for i in range(steps):
                ops.apgd_step(x_adv, x_old, x0, grad, ctl, cursor, steps, eps)     # advances the cursor's second word
                x_adv.fill_(float(i))                                               # "iterate i"
                g_new = torch.full((n,), float(i), device=dev)
                ops.apgd_commit(x_adv, g_new, grad, x_best, grad_best, x_ret, torch.tensor([seq[i]], device=dev), ctl, hist, cursor,
                                steps, sd, sm)
                w = want[i]
                both = torch.stack([x_adv, grad, x_best, grad_best, x_ret])
                lo, got = both.min(1)[0].tolist(), both.max(1)[0].tolist()
                assert lo == got, (name, i)
                assert got == [w["x"], w["g"], w["xb"], w["gb"], w["ret"]], (name, loss0, i, got, w)
            rec = ctl.cpu().numpy()
            assert cursor.tolist() == [steps, steps - 1]
            assert np.array_equal(hist.cpu().numpy(), seq)
            for i, w in enumerate(want):
                now, nxt = rec[i], rec[i + 1]
                got = (now[0], int(now[4]), bool(nxt[11]), bool(nxt[9]), bool(nxt[10]), int(nxt[12]), nxt[2], nxt[8], int(nxt[6]))
                exp = (w["step"], w["k"], w["moved"], w["chk"], w["red"], w["rose"], w["best"], seq[i], i + 1)
                assert got == exp, (name, loss0, i, got, exp)
                assert now[1] == (1.0 if i == 0 else 0.75)


# ------------------------------------------------------------------------------------------------- 3. / 4. the whole attack
def _check_against(trace, patch, obj, eps, ref_dec, ref_step, ref_loss, ref_patch, n_safe, e_ref, margin, d_ref, sub, label):
    steps = len(trace)
    dec = R.decisions(trace)
    assert np.array_equal(dec[:n_safe], np.asarray(ref_dec)[:n_safe]), (dec.T, np.asarray(ref_dec).T)
    assert np.array_equal(np.array([r["step_size"] for r in trace], dtype=np.float32)[:n_safe],
                          np.asarray(ref_step, dtype=np.float32)[:n_safe])
    upto = steps if n_safe == steps else n_safe
    mine, ref = np.array([r["loss"] for r in trace], dtype=np.float64)[:upto], np.asarray(ref_loss, dtype=np.float64)[:upto]
    e_hip = float((np.abs(mine - ref) / np.abs(ref)).max())
    print("%s: e_ref %.3g  HIP distance to the fp32 reference's losses %.3g  smallest margin of the safe prefix %.3g  n_safe %d"
          % (label, e_ref, e_hip, float(np.min(margin[:n_safe])), n_safe))
    assert e_hip <= 1.5 * e_ref + 1e-4
    got = (patch if n_safe == steps else trace[n_safe - 1]["patch"]).cpu()
    assert float((got - obj).abs().max()) <= eps + 1e-6
    got = got[:, :, ::2, ::2] if sub else got
    diff = (got - ref_patch).abs()
    share = float((diff > 1e-5).float().mean())
    print("%s: d_ref %.4g  share of HIP texels beyond 1e-5 of the reference patch %.4g" % (label, d_ref, share))
    assert d_ref <= 0.05
    assert share <= 1.5 * d_ref + 0.005
    assert float(diff.max()) <= 2 * eps + 1e-6


@no_miopen
def test_attack_matches_the_reference_fixture(golden):
    _, ta = _mods()
    g = golden("atk_apgd")
    B, steps, rng_seed = [int(v) for v in g["shape"]]
    eps, n_safe = float(g["eps"]), int(g["n_safe"])
    obj, mask, scenes, t = R.case_inputs()
    model = R.make_model().cuda()
    model.train()
    rm = model.bn.running_mean.clone()
    atk = ta.Phy_obj_atk_APGD(model, obj.cuda(), mask.cuda(), eps=eps, steps=steps, seed=R.CASE["seed"], dist_range=TRAIN_DIST)
    atk.random_start_noise = t
    atk.trace = []
    R.seed_all(rng_seed)
    adv_s, ben_s, m_out, patch = atk(scenes.cuda(), B, eval=True)
    assert model.training and torch.equal(model.bn.running_mean, rm)
    ref_patch = np_t(g["patch_sub"] if n_safe == steps else g["patch_safe_sub"])
    _check_against(atk.trace, patch, obj, eps, g["decisions"], g["step_size"], g["loss_steps"], ref_patch, n_safe, float(g["e_ref"]),
                   g["margins"], float(g["d_ref"]), True, "fixture")
    assert_close_frac(m_out[ROWS], np_t(g["mask_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="mask rows")
    assert_close_frac(ben_s[ROWS], np_t(g["ben_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="ben rows")
    torch.testing.assert_close(m_out.double().sum((1, 2, 3)).cpu(), np_t(g["mask_out_sum"]), rtol=1e-5, atol=0)
    if n_safe == steps:
        assert_close_frac(adv_s[ROWS], np_t(g["adv_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=0.01, name="adv rows")


@no_miopen
def test_attack_matches_the_restatement_on_other_inputs():
    """One broadcast scene, eval=True, 4 iterations, another eps; margins and the safe prefix computed here."""
    _, ta = _mods()
    from oracle import synth
    obj, mask = synth.make_object()
    scene = synth.kitti_like(1, 3, 375, 1242, torch.Generator().manual_seed(77))
    t = 2 * torch.rand(obj.shape, generator=torch.Generator().manual_seed(9)) - 1
    B, steps, eps = 3, 4, 0.1
    kw = dict(eps=eps, steps=steps, seed=5, dist_range=TRAIN_DIST, eval=True)
    make = lambda: R.make_model(model_seed=6, gain=6.0)     # noqa: E731
    tr32 = []
    random.seed(5)
    a_ref, b_ref, m_ref, p_ref = R.phy_obj_atk_apgd(make(), obj, mask, scene, B, start_noise=t, trace=tr32, **kw)
    tr64 = R.run64(make, obj, mask, scene, B, t, **kw)
    dec32 = R.decisions(tr32)
    n_safe, e_ref, margin, thr = R.safe_prefix([r["loss"] for r in tr32], dec32, tr64)
    assert n_safe >= 1, (margin, thr)
    d_ref = float(((tr32[n_safe - 1]["patch"].double() - tr64[n_safe - 1]["patch"]).abs() > 1e-5).double().mean())
    atk = ta.Phy_obj_atk_APGD(make().cuda(), obj.cuda(), mask.cuda(), eps=eps, steps=steps, seed=5, dist_range=TRAIN_DIST)
    atk.random_start_noise = t
    atk.trace = []
    random.seed(5)
    a, b, m, p = atk(scene.cuda(), B, eval=True)
    ref_patch = p_ref if n_safe == steps else tr32[n_safe - 1]["patch"]
    _check_against(atk.trace, p, obj, eps, dec32, [r["step_size"] for r in tr32], [r["loss"] for r in tr32], ref_patch, n_safe, e_ref,
                   margin, d_ref, False, "restatement")
    assert_close_frac(m, m_ref, rtol=1e-4, atol=2e-5, max_bad_frac=1e-4, name="mask")
    assert_close_frac(b, b_ref, rtol=1e-4, atol=2e-5, max_bad_frac=1e-4, name="benign scenes")
    if n_safe == steps:
        assert_close_frac(a, a_ref, rtol=1e-4, atol=2e-5, max_bad_frac=0.01, name="adv scenes")


# ------------------------------------------------------------------------------------------------------ 5. graph, windows
def _unet(dev, seed=0):
    from depthmodelhardening_amd.depth_model import import_depth_model
    torch.manual_seed(seed)
    model = import_depth_model((1024, 320)).to(dev).eval()
    # random-init BatchNorm statistics are (0, 1): perturb them so that the eval-mode affine is not the identity
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
    atk = ta.Phy_obj_atk_APGD(model, obj.to(dev), pmask.to(dev), eps=0.1, steps=steps, dist_range=TRAIN_DIST)
    atk.random_start_noise = 2 * torch.rand(obj.shape, generator=torch.Generator().manual_seed(9)) - 1
    atk.trace = []
    for k, v in attrs.items():
        setattr(atk, k, v)
    random.seed(13)
    adv, ben, m, patch = atk(scenes, B)
    return atk, adv, m, patch


def _strip(trace):
    return [{k: v for k, v in r.items() if k != "patch"} for r in trace]


def test_graph_replay_equals_the_eager_loop():
    """A capture does not survive a host read: graph_failure None IS the proof that the iteration reads nothing back."""
    model = _unet(torch.device("cuda"), seed=2)
    eager, _, m0, p0 = _unet_attack(model, 5)
    graph, _, m1, p1 = _unet_attack(model, 5, use_graph=True)
    assert graph.graph_failure is None and graph.use_graph
    assert torch.equal(p0, p1) and torch.equal(m0, m1)
    assert _strip(eager.trace) == _strip(graph.trace)
    assert all(torch.equal(a["patch"], b["patch"]) for a, b in zip(eager.trace, graph.trace))
    # a capture that fails hands the attack back to the eager loop, with the reason kept
    failed, _, _, p2 = _unet_attack(model, 5, use_graph=True, _capture_fault=True)
    assert failed.graph_failure is not None and "injected" in failed.graph_failure and not failed.use_graph
    assert torch.equal(p0, p2)


def test_windowed_cost_equals_full_frame_cost():
    model = _unet(torch.device("cuda"), seed=2)
    full, _, m0, p0 = _unet_attack(model, 3, B=12, use_roi=False)
    win, _, m1, p1 = _unet_attack(model, 3, B=12)
    assert np.array_equal(R.decisions(full.trace), R.decisions(win.trace)), (R.decisions(full.trace).T, R.decisions(win.trace).T)
    assert torch.equal(m0, m1)
    agree = (p0 == p1).float().mean().item()
    print("patch texels identical with / without windows: %.5f" % agree)
    assert agree > 0.999


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    ops, ta = _mods()
    from oracle import synth
    dev = torch.device("cuda")
    obj, mask = synth.make_object()
    model = R.make_model().cuda()
    for kw, word in (({"norm": "L2"}, "norm"), ({"n_restarts": 2}, "n_restarts"), ({"eot_iter": 2}, "eot_iter")):
        with pytest.raises(NotImplementedError, match=word):
            ta.Phy_obj_atk_APGD(model, obj.cuda(), mask.cuda(), **kw)
    atk = ta.Phy_obj_atk_APGD(model, obj.cuda(), mask.cuda(), eps=0.1, steps=2, dist_range=TRAIN_DIST)
    with pytest.raises(NotImplementedError, match="best_loss"):
        atk.perturb(None, best_loss=True)
    with pytest.raises(RuntimeError, match="Batch size doesn't match"):
        atk(torch.zeros(2, 3, 375, 1242).cuda(), 3)
    atk.shard = (0, 2, None)
    with pytest.raises(NotImplementedError, match="shard"):
        atk(torch.zeros(1, 3, 375, 1242).cuda(), 2)
    x = torch.rand(64)
    ctl, cur = torch.zeros(3, ops.APGD_REC), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.apgd_step(x, x.clone(), x.clone(), x.clone(), ctl, cur, 2, 0.1)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.apgd_commit(x, x.clone(), x.clone(), x.clone(), x.clone(), x.clone(), torch.zeros(1), ctl, torch.zeros(2), cur, 2, 1, 1)
    xc = x.to(dev)
    with pytest.raises(RuntimeError, match="records"):         # a record array too short for ``steps``
        ops.apgd_step(xc, xc.clone(), xc.clone(), xc.clone(), ctl.to(dev), cur.to(dev), 5, 0.1)
    with pytest.raises(RuntimeError, match="different buffers"):
        ops.apgd_step(xc, xc, xc.clone(), xc.clone(), ctl.to(dev), cur.to(dev), 2, 0.1)


# --------------------------------------------------------------------------------------------------------------- 7. evaluation
@no_miopen
def test_evaluate_attacks_runs_apgd():
    from depthmodelhardening_amd.evaluate_depth import evaluate_attacks
    model = R.make_model().cuda().eval()
    out = evaluate_attacks(model, {"norm_type": "APGD", "epsilon": 0.05, "step": 10, "batch_size": 2}, eval_count=2)
    assert out.shape == (8,) and np.isfinite(out).all()
    with pytest.raises(NotImplementedError, match="out of scope"):
        evaluate_attacks(model, {"norm_type": "Square", "epsilon": 0.05, "step": 10, "batch_size": 2}, eval_count=1)


# ------------------------------------------------------------------------------------------------------------------ 8. opcheck
def test_opcheck_of_the_apgd_operators():
    ops, _ = _mods()
    dev = torch.device("cuda")
    tests = ("test_schema", "test_faketensor")
    x = [torch.rand(515, device=dev) for _ in range(7)]
    ctl, hist, cursor, sd, sm = ops.apgd_controller(3, 0.1, torch.tensor([-1.0], device=dev))
    torch.library.opcheck(torch.ops.dmh.apgd_step, (x[0], x[1], x[2], x[3], ctl, cursor, 3, 0.1), test_utils=tests)
    torch.library.opcheck(torch.ops.dmh.apgd_commit, (x[0], x[3], x[4], x[5], x[6], x[1].clone(), torch.tensor([-0.5], device=dev), ctl,
                                                     hist, cursor, 3, sd, sm, 0.75), test_utils=tests)
    # the registered ops launch the same kernels as ops.py's wrappers
    a, b = [v.clone() for v in x[:4]], [v.clone() for v in x[:4]]
    c1, c2 = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    torch.ops.dmh.apgd_step(a[0], a[1], a[2], a[3], ctl, c1, 3, 0.1)
    ops.apgd_step(b[0], b[1], b[2], b[3], ctl, c2, 3, 0.1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(c1, c2)
