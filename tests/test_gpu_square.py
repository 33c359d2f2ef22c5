"""K27 and Phy_obj_atk_Square on the GPU: the propose kernel bit for bit (tolerance 0: there is no transcendental in it) against
the numpy restatement of tests/square_ref.py, propose + K24's commit along the reference's own scripted trajectories
(tests/golden/atk_square.npz), the device loop against its host-chain twin, the attack against the reference's own 6-query run,
the absence of host reads, windows against full frames, graph replay against the eager loop, the evaluation entry, the refusals
and the registered operator.

Cost bound of the fixture test: |cost_hip - cost_ref| <= 20 e_ref |cost_ref| (tests/test_gpu_light._check_costs), e_ref = the
reference's own fp32-versus-float64 spread on the same inputs, stored in the fixture.
"""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import square_ref as R  # noqa: E402
from tests.util import assert_close_frac, no_miopen, np_t  # noqa: E402

ROWS = (slice(None), slice(None), slice(120, 300, 9), slice(300, 800, 5))
TRAIN_DIST = list(np.arange(5, 10, 0.2))


def _mods():
    from depthmodelhardening_amd import library, ops  # noqa: F401
    from depthmodelhardening_amd import torchattacks as ta
    return ops, ta


def _same(got, want, what):
    """got (device tensor) == want (numpy) bit for bit; on a mismatch names the count and the first differing value."""
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d values differ; first at %s: kernel %r, restatement %r" % (
            what, len(bad), got.size, at, float(got[at]), float(want[at])))


# ------------------------------------------------------------------------------------------------------------------- 1. kernel
def _records(c, h, w, rs):
    """Rows 1 ..: side 1 and min(h, w), a middle side flush with every corner and border, an interior square; mixed signs."""
    m, mid = min(h, w), max(min(h, w) // 2, 1)
    rows = [(0, 0, 1), (h - 1, w - 1, 1), (h // 2, w // 3, 1), (0, 0, m), (h - m, w - m, m),
            (0, 0, mid), (0, w - mid, mid), (h - mid, 0, mid), (h - mid, w - mid, mid),
            (0, (w - mid) // 2, mid), ((h - mid) // 2, 0, mid), (h - mid, (w - mid) // 2, mid), ((h - mid) // 2, w - mid, mid),
            ((h - mid) // 2, (w - mid) // 2 + (1 if w - mid > 1 else 0), mid)]
    table = np.zeros((len(rows) + 1, 3 + c), dtype=np.int32)
    for row, (vh, vw, s) in zip(table[1:], rows):
        row[:3] = vh, vw, s
        row[3:] = rs.choice([-1, 1], c)
    table[4, 3:] = 1        # the two whole-side squares push every texel they cover against a bound: up ...
    table[5, 3:] = -1       # ... and down
    return table


@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 13, 19), (3, 64, 65), (3, 32, 64), (3, 260, 300)])
def test_propose_equals_the_restatement(shape):
    """Every record with both decisions, the stripes, the absorb-only call at q = n, and cursors outside [0, n].  (3, 32, 64)
    and (3, 260, 300) take the 16-byte form, the others the scalar one; at 260 x 300 the launch has 77 workgroups."""
    ops, _ = _mods()
    dev = torch.device("cuda")
    c, h, w = shape
    rs = np.random.RandomState(1000 * h + w)
    eps = 0.1
    x0 = R.script_object(shape)
    table = _records(c, h, w, rs)
    stripes = rs.choice([-1.0, 1.0], (c, w)).astype(np.float32)
    n = len(table)
    e32 = np.float32(eps)
    # two different points of the feasible set, as a search would hold them
    xb = np.clip(np.minimum(np.maximum(x0 + rs.uniform(-0.2, 0.2, x0.shape).astype(np.float32), x0 - e32), x0 + e32), 0, 1)
    xn = np.clip(np.minimum(np.maximum(x0 + rs.uniform(-0.2, 0.2, x0.shape).astype(np.float32), x0 - e32), x0 + e32), 0, 1)
    d0, dt, ds = torch.from_numpy(x0).to(dev), torch.from_numpy(table).to(dev), torch.from_numpy(stripes).to(dev)
    seen = {"0": False, "1": False, "lo": False, "hi": False}
    for q in list(range(n + 1)) + [-1, -5, n + 1, 1 << 30]:
        for accept in (False, True):
            best = q - 1 if accept else (q - 2 if q > 1 else -1)
            state = torch.tensor([q, best], dtype=torch.int32, device=dev)
            gb, gn = torch.from_numpy(xb).to(dev), torch.from_numpy(xn).to(dev)
            ops.square_propose(d0, gb, gn, dt, ds, state, eps)
            wb, wn = R.propose(x0, xb, xn, table, stripes, q, best, eps)
            _same(gb, wb, "%s q %d accept %d: x_best" % (shape, q, accept))
            _same(gn, wn, "%s q %d accept %d: x_new" % (shape, q, accept))
            assert state.tolist() == [q, best]
            if q < 0 or q > n:
                assert np.array_equal(wb, xb) and np.array_equal(wn, xn)
            elif q == n:
                assert np.array_equal(wn, xn) and np.array_equal(wb, xn if accept else xb)
            elif q > 0:
                vh, vw, sd = (int(v) for v in table[q][:3])
                sq = (slice(None), slice(None), slice(vh, vh + sd), slice(vw, vw + sd))
                seen["0"] |= bool((wn[sq] == 0).any())
                seen["1"] |= bool((wn[sq] == 1).any())
                seen["lo"] |= bool(((wn[sq] == (x0 - e32)[sq]) & (wn[sq] > 0)).any())
                seen["hi"] |= bool(((wn[sq] == (x0 + e32)[sq]) & (wn[sq] < 1)).any())
    assert all(seen.values()), seen      # the clips at 0, at 1 and at x0 -+ eps were all met


# --------------------------------------------------------------------------------------------------------- 2. scripted trajectory
@pytest.mark.parametrize("name", sorted(R.SCRIPT_CASES))
def test_propose_and_commit_follow_the_reference_trajectory(golden, name):
    """K27 + K24 driven by the fixture's loss script, no model: x_best equals the reference's after every query.  The device
    takes a query's decision in at the next propose, so x_best after query q is read after launch q + 1."""
    ops, _ = _mods()
    dev = torch.device("cuda")
    g, case = golden("atk_square"), R.SCRIPT_CASES[name]
    s = {k[len("script_%s_" % name):]: g[k] for k in g.files if k.startswith("script_%s_" % name)}
    table = torch.from_numpy(R.table_of(s["vh"], s["vw"], s["s"], s["signs"])).to(dev)
    n = int(table.shape[0])
    x0, stripes = torch.from_numpy(s["x0"]).to(dev), torch.from_numpy(s["stripes"]).to(dev)
    x_best, x_new = x0.clone(), torch.zeros_like(x0)
    state, best, cost = ops.tube_light_state(n, dev)
    loss = torch.from_numpy(s["loss"]).to(dev)
    for q in range(n + 1):
        ops.square_propose(x0, x_best, x_new, table, stripes, state, case["eps"])
        if q > 0:
            _same(x_best, s["x_best"][q - 1], "script %s: x_best after query %d" % (name, q - 1))
        if q < n:
            ops.tube_light_commit(loss[q:q + 1], cost, best, state)
    assert state.tolist() == [n, int(s["accepted"][-1])]
    assert np.array_equal(cost.cpu().numpy(), s["loss"], equal_nan=True)
    assert R.accepted_of(cost.cpu().numpy()) == s["accepted"].tolist()


# ------------------------------------------------------------------------------------------------------------------- 3. attack
def _run(model, B, seed=13, scene_seed=8, eval=False, **attrs):
    _, ta = _mods()
    from oracle import synth
    dev = torch.device("cuda")
    obj, pmask = synth.make_object()
    scenes = synth.kitti_like(B, 3, 375, 1242, torch.Generator().manual_seed(scene_seed)).to(dev)
    ctor = {k: attrs.pop(k) for k in ("n_queries", "host_chain", "query_patch", "eps") if k in attrs}
    atk = ta.Phy_obj_atk_Square(model, obj.to(dev), pmask.to(dev), dist_range=TRAIN_DIST, **ctor)
    atk.trace = []
    for k, v in attrs.items():
        setattr(atk, k, v)
    R.seed_all(seed)
    adv, ben, m, patch = atk(scenes, B, eval=eval)
    return atk, adv, m, patch


@no_miopen
@pytest.mark.parametrize("query_patch", ["candidate", "best"])
def test_device_loop_equals_the_host_chain(query_patch):
    model = R.make_model().cuda().eval()
    d, a0, m0, p0 = _run(model, 3, n_queries=6, query_patch=query_patch)
    h, a1, m1, p1 = _run(model, 3, n_queries=6, query_patch=query_patch, host_chain=True)
    print("%s: costs %s accepted %s" % (query_patch, d.costs, d.accepted))
    assert d.best_index == h.best_index and 0 <= d.best_index < 7 and d.accepted == h.accepted and d.accepted[0] == 0
    assert torch.equal(p0, p1) and torch.equal(a0, a1) and torch.equal(m0, m1)
    assert np.array_equal(d.costs, h.costs), np.abs(d.costs - h.costs).max()
    assert d.trace == h.trace and len(d.trace) == 7 and d.trace[0]["square"] is None and d.trace[1]["square"][2] == 250
    if query_patch == "best":       # the reference's line :295: every query asks about the stripes again
        assert d.accepted == [0] and len(set(d.costs.tolist())) == 1


@no_miopen
def test_attack_matches_the_reference_fixture(golden):
    """The reference's own run: 7 evaluations of the start stripes at the RandomState poses (query_patch="best")."""
    from tests.test_gpu_light import _check_costs
    _, ta = _mods()
    g = golden("atk_square")
    B, n, seed, pose_seed = [int(v) for v in g["e2e_shape"]]
    obj, mask, scenes = R.case_inputs()
    model = R.make_model().cuda()
    model.train()
    rm = model.bn.running_mean.clone()
    atk = ta.Phy_obj_atk_Square(model, obj.cuda(), mask.cuda(), eps=float(g["e2e_eps"]), n_queries=n, seed=pose_seed,
                                dist_range=TRAIN_DIST, query_patch="best")
    atk.trace = []
    R.seed_all(seed)
    adv_s, ben_s, m_out, patch = atk(scenes.cuda(), B, eval=True)
    assert model.training and torch.equal(model.bn.running_mean, rm)
    assert len(atk.trace) == n + 1 == len(g["e2e_cost"])
    for t in atk.trace:
        assert np.array_equal(np.asarray(t["z0"], dtype=np.float64), g["e2e_rs_z0"]) and \
            np.array_equal(np.asarray(t["alpha"], dtype=np.int64), g["e2e_rs_alpha"])
    _check_costs(atk.costs, g["e2e_cost"], float(g["e2e_e_ref"]), "fixture")
    assert atk.accepted == [0] and atk.best_index == 0
    stripes = torch.from_numpy(g["e2e_stripes"]).reshape(1, 3, 1, -1)
    assert torch.equal(patch.cpu(), torch.clamp(obj + float(g["e2e_eps"]) * stripes, 0., 1.)), "the patch is not the stripes"
    r0, r1, c0, c1 = [int(v) for v in g["e2e_region"]]
    assert torch.equal(patch[:, :, r0:r1, c0:c1].cpu(), np_t(g["e2e_patch_rect"]))
    assert_close_frac(m_out[ROWS], np_t(g["e2e_mask_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="mask rows")
    assert_close_frac(ben_s[ROWS], np_t(g["e2e_ben_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=1e-3, name="ben rows")
    torch.testing.assert_close(m_out.double().sum((1, 2, 3)).cpu(), np_t(g["e2e_mask_out_sum"]), rtol=1e-5, atol=0)
    assert_close_frac(adv_s[ROWS], np_t(g["e2e_adv_rows"]), rtol=1e-4, atol=2e-5, max_bad_frac=0.01, name="adv rows")


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
        tiny, _, _, _ = _run(R.make_model().cuda().eval(), 2, n_queries=3, loop_context=_sync_is_an_error)
    unet, _, _, _ = _run(_unet(dev, seed=2), 4, n_queries=3, loop_context=_sync_is_an_error)
    assert tiny.best_index >= 0 and unet.best_index >= 0 and torch.cuda.get_sync_debug_mode() == 0
    with pytest.raises(RuntimeError):   # the guard sees the loop: the host chain, which reads every cost back, trips it
        with torch.backends.cudnn.flags(enabled=False):
            _run(R.make_model().cuda().eval(), 2, n_queries=1, host_chain=True, loop_context=_sync_is_an_error)
    assert torch.cuda.get_sync_debug_mode() == 0


WINDOW_SEED = 13        # the siblings' seed; to be replaced on a GPU run if fewer than 3 of its 5 full-frame margins decide


def test_windowed_cost_against_full_frame_cost():
    """A decision counts only where the full-frame margin to the running best exceeds 20 x the largest relative difference
    measured between the two costs (the fixtures' decidability rule); at least 3 of the 5 evaluations must be decidable."""
    model = _unet(torch.device("cuda"), seed=2)
    full, _, m0, _ = _run(model, 12, seed=WINDOW_SEED, n_queries=4, use_roi=False)
    win, _, m1, _ = _run(model, 12, seed=WINDOW_SEED, n_queries=4)
    assert torch.equal(m0, m1)
    rel = float((np.abs(full.costs - win.costs) / np.abs(full.costs)).max())
    print("windowed vs full-frame cost: largest relative difference %.3g over %d evaluations" % (rel, len(full.costs)))
    print("full-frame costs %s accepted %s; windowed accepted %s" % (full.costs, full.accepted, win.accepted))
    low, decidable = None, 0
    for q, c in enumerate(full.costs.astype(np.float64)):
        margin = np.inf if low is None else abs(c - low) / abs(low)
        if margin > 20.0 * rel:
            decidable += 1
            assert (q in full.accepted) == (q in win.accepted), (q, margin, rel)
        if low is None or c < low:
            low = c
    print("decidable evaluations: %d of %d" % (decidable, len(full.costs)))
    assert decidable >= 3


# -------------------------------------------------------------------------------------------------------------------- 4. graph
def _graph_case(model, B):
    eager, a0, m0, p0 = _run(model, B, n_queries=5)
    graph, a1, m1, p1 = _run(model, B, n_queries=5, use_graph=True)
    assert graph.graph_failure is None and graph.use_graph and graph.graph_replays == 4
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(a0, a1)
    assert np.array_equal(eager.costs, graph.costs) and eager.accepted == graph.accepted and eager.trace == graph.trace
    # a capture that fails hands the search back to the eager loop, with the reason kept
    with pytest.warns(UserWarning, match="capture"):
        failed, _, _, p2 = _run(model, B, n_queries=5, use_graph=True, _capture_fault=True)
    assert failed.graph_failure is not None and "injected" in failed.graph_failure and not failed.use_graph
    assert failed.graph_replays == 0 and torch.equal(p0, p2) and np.array_equal(eager.costs, failed.costs)


@no_miopen
def test_graph_replay_equals_the_eager_loop_toy_model():
    _graph_case(R.make_model().cuda().eval(), 3)


def test_graph_replay_equals_the_eager_loop_unet():
    """A capture does not survive a host read: graph_failure None is one more proof that the query reads nothing back."""
    _graph_case(_unet(torch.device("cuda"), seed=2), 2)


# --------------------------------------------------------------------------------------------------------------- 5. evaluation
@no_miopen
def test_evaluate_attacks_runs_the_square_row():
    from depthmodelhardening_amd.evaluate_depth import evaluate_attacks
    model = R.make_model().cuda().eval()
    args = {"norm_type": "Square", "epsilon": 0.05, "n_queries": 3, "batch_size": 2}
    out = evaluate_attacks(model, dict(args, square_attack=True), eval_count=2)
    assert out.shape == (8,) and np.isfinite(out).all()
    out = evaluate_attacks(model, dict(args, square_attack=True, query_patch="best"), eval_count=1)
    assert out.shape == (8,) and np.isfinite(out).all()
    with pytest.raises(NotImplementedError, match="out of scope"):
        evaluate_attacks(model, args, eval_count=1)
    with pytest.raises(NotImplementedError, match="out of scope"):      # that key serves the guassian and arbi rows only
        evaluate_attacks(model, dict(args, gradient_free_attacks=True), eval_count=1)


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    ops, ta = _mods()
    from oracle import synth
    dev = torch.device("cuda")
    obj, mask = synth.make_object()
    model = R.make_model().cuda()
    atk = ta.Phy_obj_atk_Square(model, obj.cuda(), mask.cuda(), dist_range=TRAIN_DIST, n_queries=1)
    with pytest.raises(RuntimeError, match="Batch size doesn't match"):
        atk(torch.zeros(2, 3, 375, 1242).cuda(), 3)
    atk.shard = (0, 2, None)
    with pytest.raises(NotImplementedError, match="shard"):
        atk(torch.zeros(1, 3, 375, 1242).cuda(), 2)
    small = ta.Phy_obj_atk_Square(model, obj[:, :, :13, :19].contiguous().cuda(), mask[:, :, :13, :19].contiguous().cuda(),
                                  dist_range=TRAIN_DIST, n_queries=2)
    with pytest.raises(ValueError, match="exceeds"):
        small(torch.zeros(1, 3, 375, 1242).cuda(), 2)
    table, stripes = ops.square_table(3, 3, 8, 12, p_init=0.5)
    x = torch.rand(1, 3, 8, 12, device=dev)
    t, s = torch.from_numpy(table).to(dev), stripes.to(dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="different buffers"):
        ops.square_propose(x, x, x.clone(), t, s, state, 0.1)
    y = x.clone()
    with pytest.raises(RuntimeError, match="different buffers"):
        ops.square_propose(x, y, y, t, s, state, 0.1)
    with pytest.raises(RuntimeError, match="table"):
        ops.square_propose(x, x.clone(), x.clone(), t.long(), s, state, 0.1)
    with pytest.raises(RuntimeError, match="table"):
        ops.square_propose(x, x.clone(), x.clone(), t[:, :5].contiguous(), s, state, 0.1)
    with pytest.raises(RuntimeError, match="stripes"):
        ops.square_propose(x, x.clone(), x.clone(), t, s[:, :11].contiguous(), state, 0.1)
    with pytest.raises(RuntimeError, match="int32"):
        ops.square_propose(x, x.clone(), x.clone(), t, s, state.long(), 0.1)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.square_propose(x, x.clone().double(), x.clone(), t, s, state, 0.1)
    with pytest.raises(RuntimeError, match="negative"):
        ops.square_propose(x, x.clone(), x.clone(), t, s, state, -0.1)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.square_propose(x, x.clone(), x.clone(), t, s.cpu(), state, 0.1)


# ------------------------------------------------------------------------------------------------------------------- 7. opcheck
def test_opcheck_of_the_square_operator():
    ops, _ = _mods()
    dev = torch.device("cuda")
    tests = ("test_schema", "test_faketensor")
    table, stripes = ops.square_table(3, 3, 16, 24, p_init=0.3)
    t, s = torch.from_numpy(table).to(dev), stripes.to(dev)
    x0 = torch.rand(1, 3, 16, 24, device=dev)
    state = torch.tensor([2, 1], dtype=torch.int32, device=dev)
    torch.library.opcheck(torch.ops.dmh.square_propose, (x0, x0.clone(), torch.rand_like(x0), t, s, state, 0.1), test_utils=tests)
    # the registered op launches the same kernel as ops.py's wrapper
    b1, n1 = x0.clone(), torch.rand(x0.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    b2, n2 = b1.clone(), n1.clone()
    torch.ops.dmh.square_propose(x0, b1, n1, t, s, state, 0.1)
    ops.square_propose(x0, b2, n2, t, s, state, 0.1)
    assert torch.equal(b1, b2) and torch.equal(n1, n2) and torch.equal(b1, torch.rand(x0.shape, generator=torch.Generator().manual_seed(3)).to(dev))
    assert not torch.equal(n1, b1)
