"""K28 and Phy_obj_atk_l2 on the GPU: the kernel against the float64 form of tests/l2_ref.py, the attack against that form and
against the reference's own run at batch_size = 1 (tests/golden/atk_l2.npz), graph replay against the eager loop, the evaluation
row and the registered operator.

The bound everywhere: with e_ref = the distance of the fp32 form of the reference's expressions from their float64 form on the
same inputs, the HIP result may be 20 e_ref away from the float64 form (the margin of the sibling attack tests); where e_ref is 0
(the fp32 form is exact: a zero gradient), one fp32 rounding of a value of [0, 1]: 2^-24.

Measured on one MI355X (largest over the five input cases): n = 234,000: e_ref 1.6e-06, kernel 3.0e-08; n = 2^20 + 3: e_ref
1.0e-05, kernel 3.0e-08 -- the kernel's error is the final rounding to fp32 at every size.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import l2_ref as R  # noqa: E402
from tests.util import assert_close_frac, no_miopen, np_t  # noqa: E402

ROWS = (slice(None), slice(None), slice(120, 300, 9), slice(300, 800, 5))
TRAIN_DIST = list(np.arange(5, 10, 0.2))
ONE_ROUNDING = 2.0 ** -24


def _mods():
    from depthmodelhardening_amd import library, ops  # noqa: F401
    from depthmodelhardening_amd import torchattacks as ta
    return ops, ta


def _bound(e_ref):
    return 20.0 * e_ref if e_ref > 0 else ONE_ROUNDING


# ------------------------------------------------------------------------------------------------------------------- 1. kernel
def _kernel_case(ops, name, n, offset):
    dev = torch.device("cuda")
    x, x0, g, alpha, eps = R.kernel_case(name, n)
    want64 = R.step(x.double(), x0.double(), g.double(), alpha, eps)
    e_ref = float((R.step(x, x0, g, alpha, eps).double() - want64).abs().max())

    def on_device(t):       # ``offset`` elements into a larger buffer: offset 1 makes the pointer 4- but not 16-byte aligned
        buf = torch.zeros(n + offset, device=dev)
        buf[offset:] = t.to(dev)
        return buf[offset:]
    dx, dx0, dg = on_device(x), on_device(x0), on_device(g)
    assert dx.data_ptr() % 16 == (4 * offset) % 16
    ws = ops.pgd_l2_workspace(n, dev)
    out_buf = torch.full((n + offset + 1,), -7.0, device=dev)       # one guard element on either side of the result
    out = out_buf[offset:offset + n] if offset else out_buf[:n]
    got = ops.pgd_l2_step(dx, dx0, dg, alpha, eps, out=out, workspace=ws)
    assert got.data_ptr() == out.data_ptr()
    again = ops.pgd_l2_step(dx, dx0, dg, alpha, eps, out=torch.empty_like(out), workspace=ws)
    fresh = ops.pgd_l2_step(dx, dx0, dg, alpha, eps)                # out=None, workspace=None
    assert torch.equal(got, again) and torch.equal(got, fresh), "%s n %d: two calls differ" % (name, n)
    assert float(out_buf[n + offset]) == -7.0 and (offset == 0 or float(out_buf[0]) == -7.0), "written outside the result"
    assert torch.equal(dx.cpu(), x) and torch.equal(dx0.cpu(), x0) and torch.equal(dg.cpu(), g)      # inputs untouched
    res = got.cpu()
    assert torch.isfinite(res).all() and float(res.min()) >= 0 and float(res.max()) <= 1
    err = float((res.double() - want64).abs().max())
    print("%-16s n %8d offset %d: e_ref %.3g  kernel %.3g  bound %.3g" % (name, n, offset, e_ref, err, _bound(e_ref)))
    assert err <= _bound(e_ref), (name, n, offset, err, e_ref)
    # the case is the case it claims to be (float64 form)
    y = x.double() + alpha * g.double() / (g.double().norm() + R.EPS_FOR_DIVISION)
    dn = float((y - x0.double()).norm())
    if name in ("inside", "zero_grad", "clamps"):
        assert 0 < dn < eps
    elif name == "outside":
        assert dn > eps
        assert float((res.double() - x0.double()).norm()) <= eps * (1 + 1e-6)
    elif name == "zero_grad_at_x0":
        assert dn == 0 and torch.equal(res, x0)
    if name == "zero_grad":
        assert torch.equal(res, x)
    if name == "clamps" and n >= 255:
        assert bool((res == 0).any()) and bool((res == 1).any())
    return e_ref, err


@pytest.mark.parametrize("n", R.KERNEL_SIZES)
def test_kernel_against_the_float64_form(n):
    """Every input case at every size; at n = 257 also with all four tensors one element off the 16-byte alignment (the scalar
    form).  n <= 1023 with aligned pointers take the 16-byte form in one partial workgroup, 234,000 in 229, 2^20 + 3 in the
    capped 256 with a grid-stride loop; 1, 3, 5, 255, 257, 1023 and 2^20 + 3 have a tail after the last whole float4."""
    ops, _ = _mods()
    worst = (0.0, 0.0)
    for name in R.KERNEL_CASES:
        for offset in ((0, 1) if n == 257 else (0,)):
            e_ref, err = _kernel_case(ops, name, n, offset)
            worst = max(worst, (e_ref, err), key=lambda p: p[1])
    print("n %d: largest kernel error %.3g (e_ref there %.3g)" % (n, worst[1], worst[0]))


def test_kernel_refusals():
    ops, _ = _mods()
    dev = torch.device("cuda")
    x = torch.rand(64, device=dev)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.pgd_l2_step(x, x[:-1], x, 0.1, 0.1)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.pgd_l2_step(x, x.clone(), x.clone(), 0.1, 0.1, out=torch.empty(63, device=dev))
    with pytest.raises(RuntimeError, match="negative"):
        ops.pgd_l2_step(x, x.clone(), x.clone(), 0.1, -0.1)
    with pytest.raises(RuntimeError, match="of its own"):
        ops.pgd_l2_step(x, x.clone(), x.clone(), 0.1, 0.1, out=x)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.pgd_l2_step(x, x.clone(), x.clone(), 0.1, 0.1, workspace=torch.zeros(2, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match="float64"):
        ops.pgd_l2_step(x, x.clone(), x.clone(), 0.1, 0.1, workspace=torch.zeros(768, device=dev))


# ------------------------------------------------------------------------------------------------------------------- 2. attack
@pytest.fixture(scope="module")
def twins():
    """Per batch size: the draws and the fp32 / float64 forms of the attack on the CPU, computed once and not written again."""
    out = {}
    case = R.CASE
    for B in (1, 2):
        obj, mask, scenes = R.case_inputs(B)
        R.seed_all(case["rng_seed"])
        normal, r = R.draw_start(obj)
        R.seed_all(case["rng_seed"])
        drawn = R.draw_poses(TRAIN_DIST, list(R.attack_ref.ANGLE_RANGE), case["steps"], B)
        runs = {}
        for dt in (torch.float32, torch.float64):
            tr = []
            res = R.phy_obj_atk_l2(R.make_model().to(dt), obj.to(dt), mask.to(dt), scenes.to(dt), B, eps=case["eps"],
                                   steps=case["steps"], random_start_draw=(normal.to(dt), r.to(dt)), dist_range=TRAIN_DIST,
                                   eval=True, trace=tr, draws=drawn[:-1], final_draw=drawn[-1])
            runs[dt] = (np.asarray([t["cost"] for t in tr]), res[3])
        (c32, p32), (c64, p64) = runs[torch.float32], runs[torch.float64]
        out[B] = dict(normal=normal, r=r, c64=c64, p64=p64, e_cost=float((np.abs(c32 - c64) / np.abs(c64)).max()),
                      e_patch=float((p32.double() - p64).abs().max()))
    return out


def _attack(B, start, model=None, torch_seed=None, **attrs):
    _, ta = _mods()
    case = R.CASE
    obj, mask, scenes = R.case_inputs(B)
    model = R.make_model().cuda() if model is None else model
    atk = ta.Phy_obj_atk_l2(model, obj.cuda(), mask.cuda(), eps=case["eps"], alpha=123.0, steps=attrs.pop("steps", case["steps"]),
                            dist_range=TRAIN_DIST)
    atk.random_start_noise = start
    for k, v in attrs.items():
        setattr(atk, k, v)
    R.seed_all(case["rng_seed"])
    if torch_seed is not None:
        torch.manual_seed(torch_seed)       # the start's generator alone; the poses keep their seed
    return (atk,) + tuple(atk(scenes.cuda(), B, eval=True))


@no_miopen
@pytest.mark.parametrize("B", [2, 1])
def test_attack_against_the_float64_form(twins, golden, B):
    t = twins[B]
    case = R.CASE
    obj = R.case_inputs(B)[0]
    model = R.make_model().cuda()
    model.train()
    rm = model.bn.running_mean.clone()
    atk, adv_s, ben_s, m_out, patch = _attack(B, (t["normal"], t["r"]), model=model, trace=[])
    assert model.training and torch.equal(model.bn.running_mean, rm)        # eval() during the attack, restored after
    assert atk.alpha == R.step_alpha(case["eps"], case["steps"]) and len(atk.trace) == case["steps"]
    costs = np.asarray([c for c, _ in atk.trace])
    e_cost = float((np.abs(costs - t["c64"]) / np.abs(t["c64"])).max())
    e_patch = float((patch.cpu().double() - t["p64"]).abs().max())
    print("B %d: costs %s  float64 %s" % (B, costs, t["c64"]))
    print("B %d: cost e_ref %.3g HIP %.3g   patch e_ref %.3g HIP %.3g" % (B, t["e_cost"], e_cost, t["e_patch"], e_patch))
    assert e_cost <= _bound(t["e_cost"]) and e_patch <= _bound(t["e_patch"])
    norm = float((patch.cpu().double() - obj.double()).norm())
    print("B %d: ||patch - obj|| %.6f of eps %g; %d texels at a bound of [0, 1]" % (B, norm, case["eps"],
                                                                                  int(((patch == 0) | (patch == 1)).sum())))
    assert norm <= case["eps"] * (1 + 1e-6) and float(patch.min()) >= 0 and float(patch.max()) <= 1
    assert tuple(patch.shape) == tuple(obj.shape) and adv_s.shape[0] == ben_s.shape[0] == m_out.shape[0] == B
    if B == 1:      # the reference's own run
        g = golden("atk_l2")
        ref = g["b1_cost"].astype(np.float64)
        e_fix = float((np.abs(costs - ref) / np.abs(ref)).max())
        r0, r1, c0, c1 = [int(v) for v in g["b1_region"]]
        e_rect = float((patch[:, :, r0:r1, c0:c1].cpu() - np_t(g["b1_patch_rect"])).abs().max())
        print("fixture: cost e_ref %.3g HIP %.3g   patch region e_ref %.3g HIP %.3g" % (
            float(g["b1_e_ref_cost"]), e_fix, float(g["b1_e_ref_patch"]), e_rect))
        assert e_fix <= _bound(float(g["b1_e_ref_cost"])) and e_rect <= _bound(float(g["b1_e_ref_patch"]))
        assert abs(norm - float(g["b1_norm"][-1])) <= 1e-4 * norm
        assert_close_frac(m_out[ROWS], np_t(g["b1_mask_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="mask rows")
        assert_close_frac(ben_s[ROWS], np_t(g["b1_ben_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="ben rows")
        assert_close_frac(adv_s[ROWS], np_t(g["b1_adv_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=0.01, name="adv rows")
        torch.testing.assert_close(m_out.double().sum((1, 2, 3)).cpu(), np_t(g["b1_mask_out_sum"]), rtol=1e-5, atol=0)


@no_miopen
def test_own_random_start_and_torch_step(twins):
    """Without the hook the start is drawn on the device from torch's generator: inside the ball, the same for the same seed,
    another one for another seed.  ``torch_step`` (the benchmark's baseline) follows the kernel to the fp32 form's own error."""
    t = twins[2]
    obj = R.case_inputs(2)[0]
    _, _, _, _, p0 = _attack(2, None, torch_seed=5, steps=1)
    _, _, _, _, p1 = _attack(2, None, torch_seed=6, steps=1)
    _, _, _, _, p2 = _attack(2, None, torch_seed=5, steps=1)
    assert not torch.equal(p0, p1) and torch.equal(p0, p2)
    assert float((p0.cpu().double() - obj.double()).norm()) <= R.CASE["eps"] * (1 + 1e-6)
    _, _, _, _, pk = _attack(2, (t["normal"], t["r"]))
    _, _, _, _, pt = _attack(2, (t["normal"], t["r"]), torch_step=True)
    e = float((pk - pt).abs().max())
    print("K28 against the torch form of the step after %d steps: %.3g (e_ref %.3g)" % (R.CASE["steps"], e, t["e_patch"]))
    assert e <= _bound(t["e_patch"])


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


def test_graph_replay_equals_the_eager_loop(twins):
    """The graph needs the windowed cost, which the U-Net offers: the eager loop on the common-size windows and the replayed
    step end with the same bits, twice (a second attack of the same object reuses the pool and the workspace)."""
    t = twins[2]
    model = _unet(torch.device("cuda"), seed=2)
    start = (t["normal"], t["r"])
    eager, a0, _, m0, p0 = _attack(2, start, model=model, steps=4, common_windows=True)
    graph, a1, _, m1, p1 = _attack(2, start, model=model, steps=4, use_graph=True)
    assert graph.graph_failure is None and graph.use_graph and graph._graph is not None and eager._graph is None
    assert torch.equal(p0, p1) and torch.equal(a0, a1) and torch.equal(m0, m1)
    obj = R.case_inputs(2)[0]
    assert float((p1.cpu().double() - obj.double()).norm()) <= R.CASE["eps"] * (1 + 1e-6)
    ws = graph._workspace
    R.seed_all(R.CASE["rng_seed"])
    _, _, _, p2 = graph(R.case_inputs(2)[2].cuda(), 2, eval=True)
    assert torch.equal(p2, p1) and graph._workspace is ws and graph.graph_failure is None


# --------------------------------------------------------------------------------------------------------------- 3. evaluation
@no_miopen
def test_evaluate_attacks_runs_the_l2_row():
    from depthmodelhardening_amd.evaluate_depth import evaluate_attacks
    model = R.make_model().cuda().eval()
    args = {"norm_type": "l_2", "epsilon": 8, "alpha": 0.02, "step": 3, "batch_size": 2}
    out = evaluate_attacks(model, dict(args, l2_attack=True), eval_count=2)
    assert out.shape == (8,) and np.isfinite(out).all()
    with pytest.raises(NotImplementedError, match="out of scope"):
        evaluate_attacks(model, args, eval_count=1)
    with pytest.raises(NotImplementedError, match="out of scope"):      # another row's key does not serve this one
        evaluate_attacks(model, dict(args, square_attack=True), eval_count=1)


def test_evaluate_attacks_honours_graph_attack():
    from depthmodelhardening_amd.evaluate_depth import evaluate_attacks
    model = _unet(torch.device("cuda"), seed=2)
    args = {"norm_type": "l_2", "epsilon": 8, "alpha": 0.02, "step": 3, "batch_size": 2, "l2_attack": True, "graph_attack": True}
    out = evaluate_attacks(model, args, eval_count=1)
    assert out.shape == (8,) and np.isfinite(out).all()


def test_registered_operator():
    ops, _ = _mods()
    dev = torch.device("cuda")
    x, x0, g, alpha, eps = (t.to(dev) if torch.is_tensor(t) else t for t in R.kernel_case("outside", 1023))
    torch.library.opcheck(torch.ops.dmh.pgd_l2_step, (x, x0, g, alpha, eps), test_utils=("test_schema", "test_faketensor"))
    a = torch.ops.dmh.pgd_l2_step(x, x0, g, alpha, eps)
    b = ops.pgd_l2_step(x, x0, g, alpha, eps)
    assert torch.equal(a, b) and not torch.equal(a, x) and a.data_ptr() != x.data_ptr()
    x3 = x[:1020].view(1, 3, 17, 20)
    a = torch.ops.dmh.pgd_l2_step(x3, x0[:1020].view(1, 3, 17, 20), g[:1020].view(1, 3, 17, 20), alpha, eps)
    assert a.shape == x3.shape and torch.equal(a.view(-1), ops.pgd_l2_step(x[:1020], x0[:1020], g[:1020], alpha, eps))
