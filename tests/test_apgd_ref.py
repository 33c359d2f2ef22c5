"""tests/apgd_ref.phy_obj_atk_apgd (the CPU restatement of the reference's Auto-PGD object attack) against
tests/golden/atk_apgd.npz, which tools/make_goldens_apgd.py wrote from the reference's own ``Phy_obj_atk_APGD``; and the
conditions that make that fixture decidable, re-checked from what it stores."""
import numpy as np
import pytest
import torch

from tests import apgd_ref as R
from tests.util import np_t

ROWS = (slice(None), slice(None), slice(120, 300, 9), slice(300, 800, 5))


@pytest.fixture(scope="module")
def runs(golden):
    g = golden("atk_apgd")
    B, steps, rng_seed = [int(v) for v in g["shape"]]
    assert (B, steps, rng_seed) == (R.CASE["batch"], R.CASE["steps"], R.CASE["rng_seed"])
    obj, mask, scenes, t = R.case_inputs()
    kw = dict(eps=float(g["eps"]), steps=steps, seed=R.CASE["seed"], dist_range=list(np.arange(5, 10, 0.2)), eval=True)
    model = R.make_model()
    model.train()
    tr32 = []
    R.seed_all(rng_seed)
    out32 = R.phy_obj_atk_apgd(model, obj, mask, scenes, B, start_noise=t, trace=tr32, **kw)
    assert model.training
    R.seed_all(rng_seed)
    tr64 = R.run64(R.make_model, obj, mask, scenes, B, t, **kw)
    return g, obj, t, out32, tr32, tr64


def test_restatement_matches_the_reference_fixture(runs):
    """Same library, same arithmetic: the tolerances of test_oracle_golden.test_phy_obj_atk_linf; discrete state exactly."""
    g, obj, t, (adv_s, ben_s, m_out, patch), tr32, _ = runs
    n_safe, steps = int(g["n_safe"]), len(tr32)
    torch.testing.assert_close(t[:, :, ::8, ::8], np_t(g["start_noise_sub"]), rtol=0, atol=0)
    dec = R.decisions(tr32)
    assert np.array_equal(dec[:n_safe], g["decisions"][:n_safe])
    assert np.array_equal(np.array([r["step_size"] for r in tr32], dtype=np.float32)[:n_safe], g["step_size"][:n_safe])
    upto = steps if n_safe == steps else n_safe
    torch.testing.assert_close(torch.tensor([r["loss"] for r in tr32])[:upto], np_t(g["loss_steps"])[:upto], rtol=1e-6, atol=0)
    torch.testing.assert_close(torch.tensor([r["loss_best"] for r in tr32])[:upto], np_t(g["loss_best_steps"])[1:upto + 1],
                               rtol=1e-6, atol=0)
    if n_safe == steps:
        torch.testing.assert_close(patch[:, :, ::2, ::2], np_t(g["patch_sub"]), rtol=0, atol=1e-6)
        torch.testing.assert_close(patch.double().sum(), np_t(g["patch_sum"]), rtol=1e-7, atol=0)
        torch.testing.assert_close(adv_s[ROWS], np_t(g["adv_rows"]), rtol=1e-5, atol=1e-6)
    else:
        torch.testing.assert_close(tr32[n_safe - 1]["patch"][:, :, ::2, ::2], np_t(g["patch_safe_sub"]), rtol=0, atol=1e-6)
    torch.testing.assert_close(ben_s[ROWS], np_t(g["ben_rows"]), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m_out[ROWS], np_t(g["mask_rows"]), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m_out.double().sum((1, 2, 3)), np_t(g["mask_out_sum"]), rtol=1e-7, atol=0)
    assert float((patch - obj).abs().max()) <= float(g["eps"]) + 1e-6


def test_fixture_is_decidable(runs):
    """Decision margin, coverage and cap (the three conditions the generator checks), from the stored numbers and afresh."""
    g, _, _, _, _, tr64 = runs
    steps = int(g["shape"][1])
    n_safe, e_ref, margin, thr = R.safe_prefix(g["loss_steps"], g["decisions"], tr64)
    print("e_ref %.3g  threshold %.3g  smallest margin of the safe prefix %.3g  n_safe %d" % (e_ref, thr, margin[:n_safe].min(), n_safe))
    assert n_safe == int(g["n_safe"]) and n_safe >= 6
    assert abs(e_ref - float(g["e_ref"])) <= 1e-9 + 1e-6 * e_ref
    np.testing.assert_allclose(margin, g["margins"], rtol=1e-9)
    assert (g["margins"][:n_safe] >= max(20 * float(g["e_ref"]), 1e-4)).all()
    cov = R.coverage(g["decisions"], n_safe, steps)
    assert all(cov.values()), cov
    assert float(g["d_ref"]) <= 0.05


def test_wrapped_history_read_and_schedule():
    """Points 5 and 7 on numbers: k's schedule, and the first checkpoint reading the last, still zero, history row."""
    assert R.schedule(10) == (2, 1, 1) and R.schedule(100) == (22, 6, 3) and R.schedule(1) == (1, 1, 1)
    g = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "atk_apgd.npz"))
    dec, loss = g["decisions"], g["loss_steps"]
    first = int(np.argmax(dec[:, 1]))
    assert first == R.schedule(len(loss))[0] - 1
    # all losses are negative: read against the zero row every one of them "fell", read against nothing none would count
    rose = sum(int(loss[first - c] > (loss[first - c - 1] if first - c - 1 >= 0 else 0.0)) for c in range(dec[first, 4]))
    assert rose == dec[first, 3]
