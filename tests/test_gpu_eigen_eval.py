"""K25 (ops.eigen_gt_pack / ops.eigen_depth_errors) and evaluate_depth.evaluate on the GPU, against tests/eigen_eval_ref.py (the
CPU restatement that tests/test_eigen_eval_ref.py holds to the reference's fixture) and the fixture itself.

Bounds.  Depth buffer against the float64 value of the stated resize formula with the same fp32-rounded weights: rtol 2e-6
plain (about 10 fp32 roundings of positive terms with non-negative weights, 6e-7, times 3 for fused multiply-adds), 4e-6
post-processed (about 20).  Medians: bit-equal to np.median of the values the kernel itself wrote.  Metrics against the
restatement in float64 fed the kernel's own depths and ratio: rtol 2e-5 for the five continuous ones (K8's bound,
tests/test_gpu_attacks.py); a1..a3 may differ by k / n + 2e-5, k = the valid pixels whose float64 max(gt / pred, pred / gt) lies
within 1e-5 (relative) of the threshold; k <= 0.005 n is a condition on the inputs (asserted here on the kernel's values and in
the CPU test on the restatement's).

One exception, with its reason: the map with a single valid pixel under median scaling.  The ratio maps the one prediction onto
the one ground-truth value, so abs_err, abs_rel, sq_rel and rmse are the rounding of one fp32 product (the kernel rounds
depth * ratio to fp32, the float64 restatement does not) and rmse_log that plus the error of two logarithms (one ulp each of a
value in [2, 4): 2^-22 each, 5 x 2^-23 in all): no relative bound means anything for a difference of two equal numbers.  There the four are held to the absolute size of that rounding, 2^-23 of the ground-truth
value (2^-23 for the relative ones), and a1..a3 must be 1; the same map without median scaling (the stereo run) goes through
the relative bounds like every other."""
import contextlib
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import eigen_eval_ref as R  # noqa: E402
from tests.util import no_miopen  # noqa: E402

RTOL_METRIC = 2e-5
DEV = "cuda"


def _ops():
    from depthmodelhardening_amd import library, ops  # noqa: F401
    return ops


@pytest.fixture(scope="module")
def cases():
    return R.batch_cases()


@pytest.fixture(scope="module")
def runs(cases):
    """name, post_process -> what the kernel gave for the case (median scaling, factor 1) and the float64 reference of it."""
    ops = _ops()
    out = {}
    for name, case in cases.items():
        split, disp, flip, gts = case
        pack = ops.eigen_gt_pack(gts, split, DEV)
        for pp in (False, True):
            errors, ratios, depth, med = ops.eigen_depth_errors(torch.from_numpy(disp).to(DEV), pack, 0,
                                                                pred_disp_flip=torch.from_numpy(flip).to(DEV) if pp else None,
                                                                return_pred=True)
            maps = [pack.view(depth, 0, i).cpu().numpy() for i in range(len(gts))]
            out[name, pp] = dict(pack=pack, errors=errors.cpu().numpy(), ratios=ratios.cpu().numpy(), med=med.cpu().numpy(),
                                 maps=maps, ref=R.reference_run(case, pp))
    return out


def _check_metrics(got, gt, pred64, name, scaled=True):
    """``got`` [8] fp32 against compute_errors in float64 on (gt, pred64), with the threshold allowance."""
    want = np.array(R.compute_errors(gt, pred64), dtype=np.float64)
    n = gt.size
    if n == 1 and scaled:       # see the module's docstring
        u = 2.0 ** -23
        print("%s: single pixel under median scaling: got %s, want %s" % (name, got.tolist(), want.tolist()))
        assert got[0] <= u * gt[0] and got[1] <= u and got[2] <= u * u * gt[0] and got[3] <= u * gt[0] and got[4] <= 5 * u
        assert got[5:].tolist() == [1.0, 1.0, 1.0]
        return [0, 0, 0]
    k = R.near_threshold(gt, pred64)
    print("%s: n %d, near-threshold %s, got %s, want %s" % (name, n, k, got.tolist(), want.tolist()))
    assert max(k) <= 0.005 * n, (name, k, n)
    np.testing.assert_allclose(got[:5], want[:5], rtol=RTOL_METRIC, atol=0, err_msg=name)
    for j in range(3):
        assert abs(got[5 + j] - want[5 + j]) <= k[j] / n + 2e-5, (name, j, got[5 + j], want[5 + j], k[j], n)
    return k


# ------------------------------------------------------------------------------------------------------------------ 1. depth buffer
@pytest.mark.parametrize("pp", (False, True), ids=("plain", "post_process"))
@pytest.mark.parametrize("name", ("up", "down", "edge", "border"))
def test_depth_buffer(cases, runs, name, pp):
    split, disp, flip, gts = cases[name]
    run = runs[name, pp]
    _, _, depths, masks = run["ref"]
    rtol = 4e-6 if pp else 2e-6
    for i, (got, want, m) in enumerate(zip(run["maps"], depths, masks)):
        assert got.shape == gts[i].shape
        assert np.array_equal(~np.isnan(got), m), (name, i, "validity flags")
        assert np.array_equal(got.view(np.uint32)[~m], np.full(int((~m).sum()), 0xffffffff, dtype=np.uint32))
        if split == "eigen":
            assert run["pack"].crops[i].tolist() == R.crop_bounds(*gts[i].shape).tolist()
        else:
            assert run["pack"].crops[i].tolist() == [0, gts[i].shape[0], 0, gts[i].shape[1]]
        if m.any():
            rel = np.abs(got[m] / want[m] - 1).max()
            print("%s image %d %s: %d valid, largest relative difference %.3g (bound %.1g)" % (name, i, "pp" if pp else "plain",
                                                                                               int(m.sum()), rel, rtol))
            np.testing.assert_allclose(got[m], want[m], rtol=rtol, atol=0)
    if name == "border":        # every pixel valid: the rows and columns where the clamps of the resize act, on their own
        got, want = run["maps"][0], depths[0]
        assert masks[0].all()
        for sel in ((0,), (-1,), (slice(None), 0), (slice(None), -1)):
            np.testing.assert_allclose(got[sel], want[sel], rtol=rtol, atol=0)
        if not pp:              # both clamps give weight 0 to the second tap: the corners are the source's corners, exactly
            assert got[0, 0] == np.float32(1) / disp[0, 0, 0] and got[-1, -1] == np.float32(1) / disp[0, -1, -1]


# ------------------------------------------------------------------------------------------------------------------ 2. medians
def test_medians_equal_numpy_on_the_kernels_own_values(cases, runs):
    seen = set()
    for (name, pp), run in runs.items():
        split, _, _, gts = cases[name]
        med_gt, cnt = run["pack"].medians.cpu().numpy(), run["pack"].counts.cpu().numpy()
        for i, (got, gt) in enumerate(zip(run["maps"], gts)):
            m = R.valid_mask(gt, split)
            n = int(m.sum())
            assert cnt[i] == n
            if n == 0:
                assert np.isnan(med_gt[i]) and np.isnan(run["med"][i]) and np.isnan(run["ratios"][i])
                continue
            want_gt, want_pred = np.median(gt[m]), np.median(got[m])
            assert want_gt.dtype == np.float32 and want_pred.dtype == np.float32
            assert med_gt[i].view(np.uint32) == want_gt.view(np.uint32), (name, i, med_gt[i], want_gt)
            assert run["med"][i].view(np.uint32) == want_pred.view(np.uint32), (name, pp, i, run["med"][i], want_pred)
            assert run["ratios"][i].view(np.uint32) == (want_gt / want_pred).view(np.uint32)
            seen.add((n % 2, min(n, 2)))
    assert {(0, 2), (1, 2), (1, 1)} <= seen         # even, odd, and a single value


def test_medians_of_duplicates_across_the_bin_boundaries_of_every_pass():
    ops = _ops()
    disp, gts = R.straddle_case()
    pack = ops.eigen_gt_pack(gts, None, DEV)
    _, ratios, depth, med = ops.eigen_depth_errors(torch.from_numpy(disp).to(DEV), pack, 0, return_pred=True)
    med, med_gt, ratios = med.cpu().numpy(), pack.medians.cpu().numpy(), ratios.cpu().numpy()
    assert pack.counts.tolist() == [240] * 3
    for k, (lo, hi) in enumerate(R.straddle_values()):
        got = pack.view(depth, 0, k).cpu().numpy()
        assert np.array_equal(got, np.float32(1) / disp[k])             # the resize between equal sizes is the identity
        want = np.median(got)
        assert want == (lo + hi) / np.float32(2)
        assert med[k].view(np.uint32) == want.view(np.uint32), (k, med[k], want)
        assert med_gt[k].view(np.uint32) == np.median(gts[k]).view(np.uint32) and med_gt[k] == want
        assert ratios[k] == 1.0


# ------------------------------------------------------------------------------------------------------------------ 3. metrics
@pytest.mark.parametrize("pp", (False, True), ids=("plain", "post_process"))
@pytest.mark.parametrize("name", ("up", "down", "edge", "border"))
def test_metrics_against_the_restatement_on_the_kernels_depths(cases, runs, name, pp):
    split, _, _, gts = cases[name]
    run = runs[name, pp]
    for i, (depth, gt) in enumerate(zip(run["maps"], gts)):
        m = R.valid_mask(gt, split)
        if not m.any():
            assert np.isnan(run["errors"][i]).all()
            continue
        raw = depth[m].astype(np.float64) * float(run["ratios"][i])
        assert name != "border" or 0 < (raw > R.MAX_DEPTH).sum() < raw.size                    # the upper clamp bites
        pred = np.clip(raw, np.float32(R.MIN_DEPTH), R.MAX_DEPTH)
        _check_metrics(run["errors"][i], gt[m].astype(np.float64), pred, "%s image %d" % (name, i))
    ref_errors = run["ref"][0]      # and the whole float64 loop, its own medians included
    ok = np.array([R.valid_mask(gt, split).sum() > 1 for gt in gts])
    np.testing.assert_allclose(run["errors"][ok][:, :5], ref_errors[ok][:, :5], rtol=RTOL_METRIC, atol=0)


@pytest.mark.parametrize("name,factor", (("up", R.STEREO_SCALE_FACTOR), ("edge", R.STEREO_SCALE_FACTOR), ("border", 2e-4)))
def test_scale_factor_without_median_scaling(cases, name, factor):
    """The stereo protocol; and a factor that puts part of the depths under the lower clamp."""
    ops = _ops()
    split, disp, flip, gts = cases[name]
    pack = ops.eigen_gt_pack(gts, split, DEV)
    errors, ratios, depth, _ = ops.eigen_depth_errors(torch.from_numpy(disp).to(DEV), pack, 0, scale_factor=factor,
                                                      median_scaling=False, return_pred=True)
    assert torch.isnan(ratios).all()
    errors = errors.cpu().numpy()
    for i, gt in enumerate(gts):
        m = R.valid_mask(gt, split)
        if not m.any():
            assert np.isnan(errors[i]).all()
            continue
        got = pack.view(depth, 0, i).cpu().numpy()
        pred = np.clip(got[m].astype(np.float64), np.float32(R.MIN_DEPTH), R.MAX_DEPTH)
        assert name != "border" or 0 < (got[m] < np.float32(R.MIN_DEPTH)).sum() < m.sum()      # the lower clamp bites
        _check_metrics(errors[i], gt[m].astype(np.float64), pred, "factor %g image %d" % (factor, i), scaled=False)


def test_metric_launch_reproduces_the_reference_numbers(golden):
    """The fixture's (gt, pred) vectors as one-row maps of another split: every pixel valid, the resize the identity."""
    ops = _ops()
    g = golden("eigen_eval")
    n_cases = g["err_out"].shape[0]
    for i in range(n_cases):
        gt, disp = g["err_gt_%d" % i], g["err_disp_%d" % i]
        pack = ops.eigen_gt_pack([gt[None, :]], None, DEV)
        errors, _, depth, _ = ops.eigen_depth_errors(torch.from_numpy(disp[None, None, :]).to(DEV), pack, 0, median_scaling=False,
                                                     return_pred=True)
        assert np.array_equal(depth.cpu().numpy(), np.float32(1) / disp)
        got = errors.cpu().numpy()[0]
        print("vector %d (n %d): %s" % (i, gt.size, got.tolist()))
        np.testing.assert_allclose(got, g["err_out"][i], rtol=RTOL_METRIC, atol=0)


# ------------------------------------------------------------------------------------------------------------------ 4. end to end
N_IMAGES, BATCH, NET_H, NET_W = 5, 2, 64, 192


def _opt(args, tmp_path):
    from depthmodelhardening_amd.options import MonodepthOptions
    return MonodepthOptions().parse(args.split() + ["--load_weights_folder", str(tmp_path)])


def _e2e_parts():
    from depthmodelhardening_amd.datasets import SyntheticEvalSet
    from oracle import synth
    net = synth.TinyDepthNet(seed=5).to(DEV).eval()
    data = SyntheticEvalSet(N_IMAGES, NET_H, NET_W, DEV, seed=7, batch_size=BATCH)
    return data, (lambda x: x), (lambda x: {("disp", 0): net(x)}), {"height": NET_H, "width": NET_W}


def _check_mean(got, disps, gts, factor, med, name):
    """Mean errors against the restatement's whole loop in float64 on the same disparities."""
    errors, ratios = R.evaluate_loop(disps, gts, "eigen", factor, med)
    want = errors.mean(0)
    allow = np.zeros(3)
    for disp, gt, ratio in zip(disps, gts, ratios):
        m = R.valid_mask(gt, "eigen")
        pred = (1 / R.resize(disp, *gt.shape))[m] * factor * (ratio if med else 1.0)
        k = R.near_threshold(gt[m].astype(np.float64), np.clip(pred, R.MIN_DEPTH, R.MAX_DEPTH))
        assert max(k) <= 0.005 * m.sum(), (name, k, m.sum())
        allow += np.array(k) / m.sum() / len(gts)
    print("%s: got %s want %s threshold allowance %s" % (name, got.tolist(), want.tolist(), allow.tolist()))
    np.testing.assert_allclose(got[:5], want[:5], rtol=RTOL_METRIC, atol=0, err_msg=name)
    assert (np.abs(got[5:] - want[5:]) <= allow + 2e-5).all(), (name, got[5:], want[5:], allow)
    return ratios


@no_miopen
def test_evaluate_end_to_end(tmp_path, capsys):
    from depthmodelhardening_amd.evaluate_depth import evaluate
    data, enc, dec, enc_dict = _e2e_parts()
    gts = data.gt_depths
    assert len({g.shape for g in gts}) > 1 and N_IMAGES % BATCH != 0
    header = "\n  " + ("{:>8} | " * 8).format("abs_err", "abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
    row = re.compile(r"^(&\s*-?\d+\.\d{3}  ){8}\\\\$", re.M)
    path = str(tmp_path / "disps_eigen_split.npy")

    mono = evaluate(_opt("--eval_mono --save_pred_disps", tmp_path), enc, dec, enc_dict, frames=data.frames(), gt_depths=gts)
    out = capsys.readouterr().out
    disps = np.load(path)
    assert disps.shape == (N_IMAGES, NET_H, NET_W) and disps.dtype == np.float32
    ratios = _check_mean(mono, disps, gts, 1.0, True, "mono")
    med = np.median(ratios)
    assert " Scaling ratios | med: {:0.3f} | std: {:0.3f}".format(med, np.std(ratios / med)) in out
    assert "   Mono evaluation - using median scaling" in out and header in out and row.search(out) and "-> Done!" in out
    assert ("&{: 8.3f}  " * 8).format(*mono.tolist()) + "\\\\" in out

    ext = evaluate(_opt("--eval_mono --ext_disp_to_eval " + path, tmp_path), None, None, enc_dict, gt_depths=gts)
    assert np.array_equal(ext, mono), "the saved predictions give other numbers than the model run"
    assert "-> Loading predictions from " + path in capsys.readouterr().out

    opt = _opt("--eval_stereo", tmp_path)
    stereo = evaluate(opt, enc, dec, enc_dict, frames=data.frames(), gt_depths=gts)
    out = capsys.readouterr().out
    _check_mean(stereo, disps, gts, R.STEREO_SCALE_FACTOR, False, "stereo")
    assert "   Stereo evaluation - disabling median scaling, scaling by 5.4" in out and "Scaling ratios" not in out
    assert opt.disable_median_scaling is True and opt.pred_depth_scale_factor == 5.4 and row.search(out)

    post = evaluate(_opt("--eval_mono --post_process --save_pred_disps", tmp_path), enc, dec, enc_dict, frames=data.frames(),
                    gt_depths=gts)
    blended = np.load(path)
    assert blended.shape == disps.shape and blended.dtype == np.float64 and not np.array_equal(blended, disps)
    _check_mean(post, blended, gts, 1.0, True, "post_process")
    assert not np.array_equal(post, mono)

    assert evaluate(_opt("--eval_mono --no_eval --save_pred_disps", tmp_path), enc, dec, enc_dict, frames=data.frames()) is None
    assert "-> Evaluation disabled. Done." in capsys.readouterr().out and np.array_equal(np.load(path), disps)


# ------------------------------------------------------------------------------------------------------------------ 5. no host reads
@contextlib.contextmanager
def _sync_is_an_error():
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode(before)


@no_miopen
def test_no_host_reads_in_the_loop(tmp_path):
    from depthmodelhardening_amd.evaluate_depth import evaluate
    with _sync_is_an_error():           # the guard itself works: a host read raises
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()
    assert torch.cuda.get_sync_debug_mode() == 0
    data, enc, dec, enc_dict = _e2e_parts()
    state = {"batches": 0, "inside": False}

    def guarded(frames):
        """Guard on from the first batch handed out (the pack is on the device by then) until the loop asks for one more
        after the last: everything the loop enqueues, and nothing of the final copy."""
        with _sync_is_an_error():
            state["inside"] = True
            for f in frames:
                state["batches"] += 1
                yield f
            state["inside"] = False

    for args in ("--eval_mono", "--eval_mono --post_process", "--eval_stereo"):
        state["batches"] = 0
        out = evaluate(_opt(args, tmp_path), enc, dec, enc_dict, frames=guarded(data.frames()), gt_depths=data.gt_depths)
        assert state["batches"] == 3 and not state["inside"] and np.isfinite(out).all()
        assert torch.cuda.get_sync_debug_mode() == 0

    def reads(frames):                   # the guard sees the loop: a host read between two batches trips it
        for f in guarded(frames):
            yield f
            f.sum().item()
    with pytest.raises(RuntimeError):
        evaluate(_opt("--eval_mono", tmp_path), enc, dec, enc_dict, frames=reads(data.frames()), gt_depths=data.gt_depths)
    torch.cuda.set_sync_debug_mode(0)


# ------------------------------------------------------------------------------------------------------------------ 6. reproducible
def test_two_runs_give_the_same_bits(cases):
    ops = _ops()
    split, disp, flip, gts = cases["up"]
    got = []
    for _ in range(2):
        pack = ops.eigen_gt_pack(gts, split, DEV)
        e, r = ops.eigen_depth_errors(torch.from_numpy(disp).to(DEV), pack, 0, pred_disp_flip=torch.from_numpy(flip).to(DEV))
        got.append((e.cpu().numpy().view(np.uint32), r.cpu().numpy().view(np.uint32), pack.medians.cpu().numpy().view(np.uint32)))
    assert all(np.array_equal(a, b) for a, b in zip(*got))
    # a batch in the middle of a pack gives what it gives alone
    pack = ops.eigen_gt_pack(gts, split, DEV)
    e, r = ops.eigen_depth_errors(torch.from_numpy(disp[1:3]).to(DEV), pack, 1, pred_disp_flip=torch.from_numpy(flip[1:3]).to(DEV))
    assert np.array_equal(e.cpu().numpy().view(np.uint32), got[0][0][1:3]) and np.array_equal(r.cpu().numpy().view(np.uint32), got[0][1][1:3])


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(cases, tmp_path):
    from depthmodelhardening_amd.evaluate_depth import evaluate
    ops = _ops()
    split, disp, flip, gts = cases["up"]
    enc_dict = {"height": 24, "width": 80}
    np.save(str(tmp_path / "d.npy"), disp)
    ext = " --ext_disp_to_eval " + str(tmp_path / "d.npy")
    for flags in ("", "--eval_mono --eval_stereo"):
        with pytest.raises(AssertionError, match="Please choose mono or stereo"):
            evaluate(_opt(flags + ext, tmp_path), None, None, enc_dict, gt_depths=gts)
    with pytest.raises(NotImplementedError, match="benchmark"):
        evaluate(_opt("--eval_mono --eval_split benchmark" + ext, tmp_path), None, None, enc_dict, gt_depths=gts)
    with pytest.raises(NotImplementedError, match="eval_eigen_to_benchmark"):
        evaluate(_opt("--eval_mono --eval_eigen_to_benchmark" + ext, tmp_path), None, None, enc_dict, gt_depths=gts)
    with pytest.raises(RuntimeError, match="4 predictions but 3 ground-truth maps"):
        evaluate(_opt("--eval_mono" + ext, tmp_path), None, None, enc_dict, gt_depths=gts[:3])
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.eigen_gt_pack(gts, split, "cpu")
    pack = ops.eigen_gt_pack(gts, split, DEV)
    d = torch.from_numpy(disp)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.eigen_depth_errors(d, pack, 0)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.eigen_depth_errors(d.to(DEV), pack, 0, pred_disp_flip=torch.from_numpy(flip))
    with pytest.raises(RuntimeError, match="fp32"):
        ops.eigen_depth_errors(d.double().to(DEV), pack, 0)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.eigen_depth_errors(d.to(DEV), pack, 0, pred_disp_flip=torch.from_numpy(flip).to(DEV).half())
    with pytest.raises(RuntimeError, match="fp32"):
        ops.eigen_gt_stats(pack.gt.double(), pack.table, pack.blk_img, 0, 4, 0, 4, True)
    with pytest.raises(RuntimeError, match="int32"):
        ops.eigen_gt_stats(pack.gt, pack.table.long(), pack.blk_img, 0, 4, 0, 4, True)
    with pytest.raises(RuntimeError, match="holds 4 ground-truth maps"):
        ops.eigen_depth_errors(d.to(DEV), pack, 1)
    with pytest.raises(RuntimeError, match="must lie in the pack"):      # the library's own check of a batch against the tables
        ops.eigen_gt_stats(pack.gt, pack.table, pack.blk_img, 2, 4, 0, 4, True)


# ------------------------------------------------------------------------------------------------------------------ 8. opcheck
def test_opcheck_of_the_eval_operators(cases):
    ops = _ops()
    split, disp, flip, gts = cases["up"]
    pack = ops.eigen_gt_pack(gts, split, DEV)
    tests = ("test_schema", "test_faketensor")
    d, f = torch.from_numpy(disp).to(DEV), torch.from_numpy(flip).to(DEV)
    grid, npx = int(pack.blk_first[-1]), int(pack.offsets[-1])
    torch.library.opcheck(torch.ops.dmh.eigen_gt_stats, (pack.gt, pack.table, pack.blk_img, 0, 4, 0, grid, True), test_utils=tests)
    for fl in (None, f):
        torch.library.opcheck(torch.ops.dmh.eigen_depth_errors,
                              (d, fl, pack.gt, pack.table, pack.blk_img, pack.medians, 0, 0, grid, 0, npx, True, 1.0, True),
                              test_utils=tests)
    # the registered ops launch the same kernels as ops.py's wrappers
    med, cnt = torch.ops.dmh.eigen_gt_stats(pack.gt, pack.table, pack.blk_img, 0, 4, 0, grid, True)
    assert torch.equal(med, pack.medians) and torch.equal(cnt, pack.counts)
    e1, r1, p1, m1 = torch.ops.dmh.eigen_depth_errors(d, f, pack.gt, pack.table, pack.blk_img, pack.medians, 0, 0, grid, 0, npx, True,
                                                      1.0, True)
    e2, r2, p2, m2 = ops.eigen_depth_errors(d, pack, 0, pred_disp_flip=f, return_pred=True)
    assert torch.equal(e1, e2) and torch.equal(r1, r2) and torch.equal(m1, m2) and bool(torch.isfinite(e1).all())
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32))
