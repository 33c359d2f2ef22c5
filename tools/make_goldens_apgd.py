"""Writes tests/golden/atk_apgd.npz: the reference's own ``Phy_obj_atk_APGD`` on the seeded inputs of tests/apgd_ref.py.

    python tools/make_goldens_apgd.py [--reference DIR]

The reference package is imported the way oracle/make_goldens.py imports it (its stand-ins for the absent torchvision, a
temporary calibration file); its attack_single_run is observed with ``sys.settrace`` -- the state of its locals at the head of
every iteration -- and is not edited.  Before anything is written the script checks, on the CPU, that the inputs make the
fixture decidable (tests/apgd_ref.py: ``safe_prefix``, ``coverage``): every comparison of the leading ``n_safe`` iterations has
a relative margin of at least max(20 e_ref, 1e-4) in a float64 run, the safe prefix covers both kinds of checkpoint, the wrapped
history read and both outcomes of the best-loss test, and n_safe >= 6.
"""
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as mg      # noqa: E402
from oracle import synth                   # noqa: E402
from tests import apgd_ref as R            # noqa: E402

ROWS = (slice(None), slice(None), slice(120, 300, 9), slice(300, 800, 5))      # the row sample of atk_linf


def reference_attack_class(ref_dir):
    mg.install_shims()
    tmp = tempfile.mkdtemp(prefix="kitti_obj_")
    os.makedirs(os.path.join(tmp, "training", "calib"))
    with open(os.path.join(tmp, "training", "calib", "003086.txt"), "w") as f:
        f.write(synth.KITTI_CALIB_TEXT)
    sys.path.insert(0, os.path.join(ref_dir, "DepthNetworks", "monodepth2"))
    sys.path.append(ref_dir)
    import my_utils
    my_utils.object_dataset_root = tmp
    import torchattacks as ta
    return ta.Phy_obj_atk_APGD


def observe(atk, call):
    """Runs ``call()`` and returns (its result, states): states[i] = the locals of attack_single_run after iteration i, read at
    the head of the loop (the line of ``for i in range(self.steps)``) and at the final ``return``."""
    code = type(atk).attack_single_run.__code__
    head, ret = code.co_firstlineno + 70, code.co_firstlineno + 159     # ``for i in range(self.steps):`` and the final ``return``
    states = {}

    def local(frame, event, arg):
        if event == "line" and frame.f_lineno in (head, ret):
            loc = frame.f_locals
            if "i" in loc:
                states[int(loc["i"])] = dict(step_size=float(loc["step_size"]), k=int(loc["k"]), counter3=int(loc["counter3"]),
                                             loss_steps=loc["loss_steps"].clone(), loss_best_steps=loc["loss_best_steps"].clone(),
                                             patch=loc["x_best_adv"].detach().clone())
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is code else None
    sys.settrace(tracer)
    try:
        out = call()
    finally:
        sys.settrace(None)
    return out, states


def main():
    ref_dir = sys.argv[sys.argv.index("--reference") + 1] if "--reference" in sys.argv else mg.REF
    case = R.CASE
    steps, B, eps = case["steps"], case["batch"], case["eps"]
    APGD = reference_attack_class(ref_dir)
    obj, mask, scenes, t = R.case_inputs(case)
    dist_range = list(np.arange(5, 10, 0.2))

    model = R.make_model()
    model.train()
    atk = APGD(model, obj, mask, eps=eps, steps=steps, seed=case["seed"], dist_range=dist_range)
    real_rand = torch.rand

    def fake_rand(*a, **k):             # the one torch.rand of attack_single_run (:142): the draw behind the start noise t
        return real_rand(obj.shape, generator=torch.Generator().manual_seed(case["noise_seed"]))
    R.seed_all(case["rng_seed"])
    torch.rand = fake_rand
    try:
        (adv_s, ben_s, m_out, patch), states = observe(atk, lambda: atk(scenes, B, eval=True))
    finally:
        torch.rand = real_rand
    assert model.training and sorted(states) == list(range(steps)), sorted(states)

    last = states[steps - 1]
    loss_steps = last["loss_steps"][:, 0].numpy()
    loss_best_steps = last["loss_best_steps"][:, 0].numpy()
    k0 = R.schedule(steps)[0]
    dec, step_used = [], []
    for i in range(steps):
        before = states[i - 1] if i else dict(step_size=float(np.float32(eps) * 2), k=k0)
        chk = states[i]["counter3"] == 0
        rose = 0
        if chk:
            for c in range(before["k"]):
                rose += int(loss_steps[i - c] > loss_steps[i - c - 1])      # row -1 wraps, as in check_oscillation
        dec.append([int(loss_best_steps[i + 1] > loss_best_steps[i]), int(chk), int(states[i]["step_size"] < before["step_size"]),
                    rose, before["k"]])
        step_used.append(before["step_size"])
    dec = np.array(dec)

    # ---- is the fixture decidable?  (float64 restatement on the same inputs)
    kw = dict(eps=eps, steps=steps, seed=case["seed"], dist_range=dist_range, eval=True)
    R.seed_all(case["rng_seed"])
    tr64 = R.run64(R.make_model, obj, mask, scenes, B, t, **kw)
    n_safe, e_ref, margin, thr = R.safe_prefix(loss_steps, dec, tr64)
    cov = R.coverage(dec, n_safe, steps)
    print("losses       ", loss_steps)
    print("decisions (moved, checkpoint, reduced, rose, k):\n", dec.T)
    print("margins      ", margin)
    print("e_ref %.3g  threshold %.3g  n_safe %d  coverage %s" % (e_ref, thr, n_safe, cov))
    if n_safe < 6 or not all(cov.values()):
        sys.exit("these inputs do not make a decidable fixture: nothing written")
    ref_patch = states[n_safe - 1]["patch"]
    d_ref = float(((ref_patch.double() - tr64[n_safe - 1]["patch"]).abs() > 1e-5).double().mean())
    print("d_ref %.4g (share of texels where fp32 reference and float64 restatement differ after iteration %d)" % (d_ref, n_safe - 1))
    if d_ref > 0.05:
        sys.exit("d_ref > 0.05: the patch comparison would not discriminate: nothing written")

    rs = np.random.RandomState(case["seed"])
    z0 = rs.choice(dist_range, B, replace=False)
    al = rs.choice(list(range(-30, 31, 5)), B, replace=False)
    extra = {} if n_safe == steps else {"patch_safe_sub": ref_patch[:, :, ::2, ::2]}
    mg.save("atk_apgd", shape=np.array([B, steps, case["rng_seed"]]), eps=np.float64(eps), start_noise_sub=t[:, :, ::8, ::8], start_noise_sum=t.double().sum(), loss_steps=loss_steps,
            loss_best_steps=loss_best_steps, step_size=np.array(step_used, dtype=np.float32), decisions=dec.astype(np.int32),
            n_safe=np.int32(n_safe), e_ref=np.float64(e_ref), d_ref=np.float64(d_ref), margins=margin,
            patch_sub=patch[:, :, ::2, ::2], patch_sum=patch.double().sum(), z0=np.asarray(z0, dtype=np.float64),
            alpha=np.asarray(al, dtype=np.int64), adv_rows=adv_s[ROWS], ben_rows=ben_s[ROWS], mask_rows=m_out[ROWS],
            adv_sum=adv_s.double().sum((2, 3)), ben_sum=ben_s.double().sum((2, 3)), mask_out_sum=m_out.double().sum((1, 2, 3)),
            **extra)


if __name__ == "__main__":
    main()
