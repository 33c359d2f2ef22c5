"""The float64 fixtures of the training-path attacks (tests/golden/atk_{linf,l0,pgd}_f64.npz, tools/make_goldens_f64.py) on the CPU:

  * the fp32 leg of the pair of runs behind them IS the reference's run: it equals tests/golden/atk_linf.npz, atk_l0.npz and
    atk_pgd_*.npz bit for bit, which ties the float64 twin to the reference;
  * every cap tests/test_gpu_attacks.py holds the HIP attacks to (20 x e_ref) holds for the fp32 oracle alone with margin 1, on
    the recorded data: the recorded e_ref are what a fresh fp32 run measures against the stored float64 trajectory;
  * a one-step float64 re-run reproduces the first step of each stored trajectory: the fixtures are not stale.

The runs are made with the CPU thread count of the recording (oracle/f64_anchor.recorded_threads): the last bits of an fp32 cost
follow it, and margin 1 leaves no room for that.  The float64 re-run is held within reordering of float64 sums (_near64).
Like tests/test_oracle_golden.py, the bit-for-bit half holds on the CPU family the reference's fixtures were recorded on:
another CPU's vector paths round the fp32 convolutions differently.

Measured (CPU, 16 threads): 21 s for the file on an idle machine, 46 s on a busy one -- the four fp32 runs, once per module,
are two thirds of it, the three float64 first steps the rest.
"""
import numpy as np
import pytest
import torch

from oracle import f64_anchor as A

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def legs():
    """The fp32 runs of the tool, once, and not written again."""
    return dict(linf=A.run_linf(F32), l0=A.run_l0(F32), pgd={t: A.run_pgd(F32, t) for t in (True, False)})


def _same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.shape == np.asarray(b).shape and np.array_equal(a, np.asarray(b))


def _near64(a, b):
    """Two float64 runs of the same step.  They are the same arithmetic, but the CPU convolutions and sums may split their work
    differently under another thread count or BLAS path, so the re-run is held to the stored one within reordering of float64
    sums, not bit for bit: 1e-12 relative on a cost (reordering the sums behind it moves it by some 1e-14), and for a
    gradient stored rounded to fp32, two fp32 roundings of each value plus 1e-10 of the largest (texels that cancel to ~0).  A
    stale fixture is off by far more: the fp32 and float64 forms of one step already differ by 5e-8 / 3e-5."""
    a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 0:
        return abs(a - b) <= 1e-12 * abs(b)
    return a.shape == b.shape and bool((np.abs(a - b) <= 2.0 ** -22 * np.abs(b) + 1e-10 * np.abs(b).max()).all())


ROWS = (slice(None), slice(None), slice(120, 300, 9), slice(300, 800, 5))


def test_fp32_leg_is_the_reference_run(legs, golden):
    r, g = legs["linf"], golden("atk_linf")
    assert _same(A.sub(r["patch"]), g["patch_sub"]) and float(r["patch"].double().sum()) == float(g["patch_sum"])
    for k, t in (("adv_rows", r["adv_s"]), ("ben_rows", r["ben_s"]), ("mask_rows", r["m_out"])):
        assert _same(t[ROWS], g[k]), k
    assert _same(r["adv_s"].double().sum((2, 3)), g["adv_sum"]) and _same(r["m_out"].double().sum((1, 2, 3)), g["mask_out_sum"])
    r, g = legs["l0"], golden("atk_l0")
    for k, t in (("patch_sub", r["patch"]), ("pattern_pos_sub", r["pos"]), ("pattern_neg_sub", r["neg"])):
        assert _same(A.sub(t), g[k]), k
    assert r["l0_final"] == int(g["l0_final"]) and np.float32(r["trace"][-1][1]) == np.float32(float(g["final_mask_weight"]))
    for k, t in (("adv_sum", r["adv_s"]), ("ben_sum", r["ben_s"])):
        assert _same(t.double().sum((2, 3)), g[k]), k
    assert float(r["pos"].double().sum()) == float(g["pattern_pos_sum"])
    for targeted, name in ((True, "targeted"), (False, "untargeted")):
        r, g = legs["pgd"][targeted], golden("atk_pgd_" + name)
        assert _same(A.pgd_rows(r["adv"]), g["adv_rows"]) and _same(r["adv"].double().sum((2, 3)), g["adv_sum"]), name
        assert float((r["adv"] - r["clean"]).abs().max()) == float(g["delta_absmax"])


def _grads_with_margin_1(au, name, d, f):
    au.per_step(name + " rel-L2", d["e_%s_rel" % name], f["e_%s_rel" % name])
    au.per_step(name + " max-abs", d["e_%s_maxabs" % name], f["e_%s_maxabs" % name])
    for s, n in enumerate(d["n_%s_sign_offend" % name]):
        au.none("%s[%d] sign offenders" % (name, s), n)     # cap = the recorded max|g32 - g64|: none by construction
    assert np.array_equal(d["n_%s_sign_differ" % name], f["n_%s_sign_differ" % name])
    assert np.array_equal(d["n_%s_zero_breach" % name], f["n_%s_zero_breach" % name])


def test_fp32_oracle_meets_every_cap_with_margin_1(legs, golden):
    f = golden("atk_linf_f64")
    d = A.linf_distances(legs["linf"], f, caps=f["e_grad_maxabs"])
    au = A.Audit("L_inf fp32 oracle", margin=1.0)
    au.per_step("cost", d["e_cost"], f["e_cost"], fp32_scalar=True)
    _grads_with_margin_1(au, "grad", d, f)
    au.texels("patch", d["n_patch_beyond"], f["n_patch_beyond"], f["tau"])
    for k in ("adv_sum", "ben_sum", "mask_out_sum"):
        au.scalar(k, d["e_" + k], f["e_" + k])
    au.finish()

    f = golden("atk_l0_f64")
    d = A.l0_distances(legs["l0"], f, caps={k: f["e_%s_maxabs" % k] for k in ("gpos", "gneg")})
    au = A.Audit("L0 fp32 oracle", margin=1.0)
    assert np.array_equal(np.asarray(legs["l0"]["trace"], dtype=np.float64), f["trace32"])
    assert np.array_equal(f["trace32"][:, 1], f["trace64"][:, 1])           # mask_weight: exact
    au.count("l0", d["e_l0"], f["e_l0"])
    au.per_step("adv_cost", d["e_adv_cost"], f["e_adv_cost"], fp32_scalar=True)
    au.per_step("mask_cost", d["e_mask_cost"], f["e_mask_cost"], fp32_scalar=True)
    _grads_with_margin_1(au, "gpos", d, f)
    _grads_with_margin_1(au, "gneg", d, f)
    for name in ("pos", "neg", "patch"):
        au.texels(name, d["n_%s_beyond" % name], f["n_%s_beyond" % name], f["tau"])
    au.count("l0 of the final patch", d["e_l0_final"], f["e_l0_final"])
    for k in ("adv_sum", "ben_sum", "mask_out_sum"):
        au.scalar(k, d["e_" + k], f["e_" + k])
    # the second, scalars-only case: its fp32 record is stored beside the float64 one
    t = A.l0_trace_distances(f["t_trace32"], f["t_trace64"])
    assert np.array_equal(f["t_trace32"][:, 1], f["t_trace64"][:, 1]) and t["e_l0"] == float(f["t_e_l0"])
    au.per_step("t adv_cost", t["e_adv_cost"], f["t_e_adv_cost"], fp32_scalar=True)
    au.per_step("t mask_cost", t["e_mask_cost"], f["t_e_mask_cost"], fp32_scalar=True)
    au.finish()

    f = golden("atk_pgd_f64")
    for targeted, tag in ((True, "targeted_"), (False, "untargeted_")):
        d = A.pgd_distances(legs["pgd"][targeted], f, tag)
        au = A.Audit("PGD fp32 oracle " + tag[:-1], margin=1.0)
        au.per_step("cost", d["e_cost"], f[tag + "e_cost"], fp32_scalar=True)
        au.texels("adv rows", d["n_adv_beyond"], f[tag + "n_adv_beyond"], f["tau"])
        au.scalar("adv_sum", d["e_adv_sum"], f[tag + "e_adv_sum"])
        au.scalar("delta_absmax", d["e_delta_absmax"], f[tag + "e_delta_absmax"])
        au.finish()


@pytest.fixture(scope="module")
def linf64_first():
    return A.run_linf(F64, steps=1)


def test_zero_sets_of_the_two_oracle_forms(legs, linf64_first, golden):
    """The GPU tests assert "HIP's gradient is exactly zero where both oracle forms' is" for a step only if the two forms' zero
    sets of that step are identical (``zero_only32_*`` = ``zero_only64_*`` = 0): they are for the first step of both object
    attacks -- the one whose gradient is asserted.  Recounted here for the first L_inf step."""
    f = golden("atk_linf_f64")
    g32, g64 = legs["linf"]["grads"][0], linf64_first["grads"][0]
    only32, only64 = int(((g32 == 0) & (g64 != 0)).sum()), int(((g32 != 0) & (g64 == 0)).sum())
    print("first L_inf step: zero in fp32 only %d, in float64 only %d, in both %d of %d" % (
        only32, only64, int(((g32 == 0) & (g64 == 0)).sum()), g32.numel()))
    assert only32 == int(f["zero_only32_grad"][0]) == 0 and only64 == int(f["zero_only64_grad"][0]) == 0
    assert float((g64 == 0).double().mean()) == float(f["zero_frac"]) > 0.3      # outside the object mask: 37 % of the texels
    f = golden("atk_l0_f64")
    for name in ("gpos", "gneg"):
        assert int(f["zero_only32_" + name][0]) == 0 and int(f["zero_only64_" + name][0]) == 0, name


def test_float64_first_step_is_reproduced(linf64_first, golden):
    """steps = 1 in float64: the first step of every stored trajectory (same start, same first pose draw)."""
    f = golden("atk_linf_f64")
    r = linf64_first
    assert _near64(r["costs"][0], f["cost64"][0]) and _near64(A.sub(r["grads"][0]), f["grad64_sub"][0])
    f = golden("atk_l0_f64")
    r = A.run_l0(F64, steps=1)
    assert tuple(r["trace"][0][:2]) == tuple(f["trace64"][0][:2])                  # l0 and mask_weight
    assert _near64(r["trace"][0][2], f["trace64"][0][2]) and _near64(r["trace"][0][3], f["trace64"][0][3])
    for name in ("gpos", "gneg"):
        assert _near64(A.sub(r[name][0], A.GRAD_SUB_L0_FIRST), f[name + "64_first"]), name
    f = golden("atk_pgd_f64")
    r = A.run_pgd(F64, True, steps=1)
    assert _near64(r["costs"][0], f["targeted_cost64"][0])
