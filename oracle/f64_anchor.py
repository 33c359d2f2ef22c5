"""How far a run of Phy_obj_atk, Phy_obj_atk_l0 or PGD_depth is from its recorded float64 trajectory.

tools/make_goldens_f64.py runs the attacks of oracle/attack_ref.py in fp32 and in float64 on the inputs below and writes
tests/golden/atk_{linf,l0,pgd}_f64.npz: the float64 trajectory, and ``e_*`` / ``n_*`` = the distances of the fp32 oracle from it,
measured by the functions of this file.  The tests measure a HIP run (tests/test_gpu_attacks.py) or a second fp32 oracle run
(tests/test_attack_f64_ref.py) with the same functions and hold it to ``margin`` times the recorded figures: 20 for HIP (the rule
of tests/test_gpu_l2.py), 1 for the oracle itself.  Test infrastructure only (see oracle/__init__.py).

Every tensor comparison is made on the subsample the fixture stores, for the run under test and for the recorded e_ref alike.
"""
import functools
import random

import numpy as np
import torch

from . import attack_ref, synth

MARGIN = 20.0                   # HIP may be this many times as far from float64 as the fp32 oracle is
ONE_ROUNDING = 2.0 ** -24       # the bound where the fp32 oracle's own distance is 0: one fp32 rounding of the quantity
TEXEL_FLOOR = 5                 # texels allowed beyond tau where the fp32 oracle has none
L0_FLOOR = 3                    # pixels on the 1/255 threshold: the count may differ by max(3, margin * recorded difference)

LINF = dict(scene_seed=31, seed=41, steps=3, eps=0.1, alpha=0.02, tau=(1e-5,))
L0 = dict(scene_seed=31, seed=43, steps=3, adam_lr=0.5, mask_wt=0.06, l0_thresh=0.1, tau=(2e-3, 1e-2))
L0_TRACE = dict(L0, scene_seed=8, seed=21, steps=2)       # the inputs of test_l0_attack_trace_vs_oracle: scalars only
PGD = dict(image_seed=33, seed=47, steps=3, eps=0.03, alpha=2 / 255, tau=(1e-6,))
GRAD_SUB_L0_FIRST, GRAD_SUB_L0_LATER = 4, 8     # the L0 gradients are stored coarser than [::2, ::2] (fixture size)
THREADS = 8                     # the CPU threads the fixtures were recorded with, see recorded_threads


def recorded_threads(run):
    """The oracle runs split their convolutions and sums among the CPU threads, so a cost's last bits follow the thread count
    (measured: the fp32 L_inf costs of steps 2 and 3 move by 1e-7 relative between 8 threads and 3, as much as e_ref itself;
    8 and 16 agree).  A run that is compared with recorded figures at margin 1, or bit for bit, is therefore made with the thread
    count of the recording, whatever the environment says; the caller's setting is put back."""
    @functools.wraps(run)
    def pinned(*args, **kwargs):
        before = torch.get_num_threads()
        torch.set_num_threads(THREADS)
        try:
            return run(*args, **kwargs)
        finally:
            torch.set_num_threads(before)
    return pinned


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def make_model(dtype=torch.float32):
    """TinyDepthNet(seed=5): built in fp32 and converted, so that both forms have the same weights (a model constructed under a
    float64 default dtype draws others)."""
    return synth.TinyDepthNet(seed=5).to(dtype)


def sub(t, k=2):
    return t[..., ::k, ::k]


def pgd_rows(t):
    return t[..., ::16, ::8]


def _t64(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).detach().cpu().double()


# ------------------------------------------------------------------------------------------------------------------ the runs
@recorded_threads
def run_linf(dtype, steps=None):
    c = LINF
    obj, mask = synth.make_object()
    scenes = synth.kitti_like(2, 3, 375, 1242, torch.Generator().manual_seed(c["scene_seed"]))
    model = make_model(dtype)
    model.train()
    seed_all(c["seed"])
    noise = torch.empty_like(obj).uniform_(-c["eps"], c["eps"])      # the reference's first draw, in fp32 for both forms
    tr = []
    adv_s, ben_s, m_out, patch = attack_ref.phy_obj_atk(
        model, obj.to(dtype), mask.to(dtype), scenes.to(dtype), 2, eps=c["eps"], alpha=c["alpha"],
        steps=c["steps"] if steps is None else steps, dist_range=attack_ref.TRAIN_DIST_RANGE, start_noise=noise.to(dtype), trace=tr)
    assert model.training
    return dict(costs=[t[0] for t in tr], grads=[t[1] for t in tr], patch=patch, adv_s=adv_s, ben_s=ben_s, m_out=m_out)


@recorded_threads
def run_l0(dtype, case=L0, steps=None):
    obj, mask = synth.make_object()
    scenes = synth.kitti_like(2, 3, 375, 1242, torch.Generator().manual_seed(case["scene_seed"]))
    rec, grads, pats = [], [], []
    seed_all(case["seed"])
    adv_s, ben_s, m_out, patch = attack_ref.phy_obj_atk_l0(
        make_model(dtype), obj.to(dtype), mask.to(dtype), scenes.to(dtype), 2, adam_lr=case["adam_lr"],
        steps=case["steps"] if steps is None else steps, mask_wt=case["mask_wt"], l0_thresh=case["l0_thresh"],
        dist_range=attack_ref.TRAIN_DIST_RANGE, record=rec, grad_record=grads, patterns=pats)
    pos, neg = pats[0]
    return dict(trace=rec, gpos=[g[0] for g in grads], gneg=[g[1] for g in grads], pos=pos, neg=neg, patch=patch,
                adv_s=adv_s, ben_s=ben_s, m_out=m_out, l0_final=int(attack_ref.cal_l0(pos.clamp(0, 1), -neg.clamp(0, 1), 1 / 255.0)))


@recorded_threads
def run_pgd(dtype, targeted, steps=None):
    c = PGD
    imgs = synth.kitti_like(2, 3, 320, 1024, torch.Generator().manual_seed(c["image_seed"]))
    seed_all(c["seed"])
    noise = torch.empty_like(imgs).uniform_(-c["eps"], c["eps"])
    tr = []
    adv, clean = attack_ref.pgd_depth(make_model(dtype), imgs.to(dtype), eps=c["eps"], alpha=c["alpha"],
                                      steps=c["steps"] if steps is None else steps, targeted=targeted, start_noise=noise.to(dtype),
                                      trace=tr)
    return dict(costs=[t[0] for t in tr], grads=[t[1] for t in tr], adv=adv, clean=clean)


# ------------------------------------------------------------------------------------------------------------- the distances
def rel_scalar(got, want64):
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    return np.abs(got - want64) / np.abs(want64)


def tensor_distance(g, g64):
    """(rel-L2, max-abs) of ``g`` against the stored float64 tensor."""
    g, g64 = _t64(g), _t64(g64)
    assert g.shape == g64.shape, (g.shape, g64.shape)
    den = float(g64.norm())
    return float((g - g64).norm()) / (den if den > 0 else 1.0), float((g - g64).abs().max())


def sign_report(g, g64, cap):
    """(texels whose sign differs from float64's, those of them where |g64| > cap).  A sign may differ only where the float64
    gradient is within rounding of zero: with cap = max|g32 - g64| the fp32 oracle has none of the second kind by construction."""
    g, g64 = _t64(g), _t64(g64)
    differ = torch.sign(g) != torch.sign(g64)
    return int(differ.sum()), int((differ & (g64.abs() > cap)).sum())


def zero_breaches(g, g64):
    """Texels with an exactly zero float64 gradient and a non-zero ``g``."""
    g, g64 = _t64(g), _t64(g64)
    return int(((g64 == 0) & (g != 0)).sum())


def count_beyond(x, x64, taus):
    d = (_t64(x) - _t64(x64)).abs()
    return np.asarray([int((d > float(t)).sum()) for t in taus], dtype=np.int64)


def sums(run):
    return dict(adv_sum=_t64(run["adv_s"]).sum((2, 3)).numpy(), ben_sum=_t64(run["ben_s"]).sum((2, 3)).numpy(),
                mask_out_sum=_t64(run["m_out"]).sum((1, 2, 3)).numpy())


def _grad_block(out, name, grads, stored, caps=None):
    """Per step: rel-L2, max-abs, sign differences / offenders (against ``caps``, or the step's own max-abs), zero-set breaches.
    ``stored(s)``: (the float64 gradient of step s as the fixture holds it, the stride it is held at), or None past the last."""
    rows = []
    for s, g in enumerate(grads):
        held = stored(s)
        if held is None:
            break
        g64, stride = held
        gs = sub(g, stride)
        r, m = tensor_distance(gs, g64)
        differ, offend = sign_report(gs, g64, m if caps is None else float(caps[s]))
        rows.append((r, m, differ, offend, zero_breaches(gs, g64)))
    a = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    out["e_%s_rel" % name], out["e_%s_maxabs" % name] = a[:, 0], a[:, 1]
    out["n_%s_sign_differ" % name], out["n_%s_sign_offend" % name] = a[:, 2].astype(np.int64), a[:, 3].astype(np.int64)
    out["n_%s_zero_breach" % name] = a[:, 4].astype(np.int64)


def linf_distances(run, fix, caps=None):
    """``run``: costs, grads (whole tensors), patch and the returned scenes of one attack; ``fix``: atk_linf_f64.  ``caps``: per
    step, the |g64| above which a differing sign counts as an offender (None: the run's own max|g - g64|)."""
    out = {"e_cost": rel_scalar(run["costs"], fix["cost64"][:len(run["costs"])])}
    _grad_block(out, "grad", run["grads"], lambda s: (fix["grad64_sub"][s], 2) if s < len(fix["grad64_sub"]) else None, caps)
    out["n_patch_beyond"] = count_beyond(sub(run["patch"]), fix["patch64_sub"], fix["tau"])
    for k, v in sums(run).items():
        out["e_" + k] = float(rel_scalar(v, fix[k + "64"]).max())
    return out


def _l0_stored_grad(fix, name):
    def stored(s):
        if s == 0:
            return fix[name + "64_first"], GRAD_SUB_L0_FIRST
        return (fix[name + "64_later"][s - 1], GRAD_SUB_L0_LATER) if s - 1 < len(fix[name + "64_later"]) else None
    return stored


def l0_trace_distances(trace, t64):
    t, t64 = np.asarray(trace, dtype=np.float64).reshape(-1, 4), np.asarray(t64, dtype=np.float64)
    assert len(t) == len(t64), "the run took %d iterations, the float64 form %d" % (len(t), len(t64))
    return {"e_l0": float(np.abs(t[:, 0] - t64[:, 0]).max()), "e_adv_cost": rel_scalar(t[:, 2], t64[:, 2]),
            "e_mask_cost": rel_scalar(t[:, 3], t64[:, 3])}


def l0_distances(run, fix, caps=None):
    """``run``: trace, patterns, patch, returned scenes, and (or None: the fused path has none) the pattern gradients."""
    out = l0_trace_distances(run["trace"], fix["trace64"])
    if run.get("gpos") is not None:
        for name in ("gpos", "gneg"):
            _grad_block(out, name, run[name], _l0_stored_grad(fix, name), None if caps is None else caps[name])
    for name in ("pos", "neg", "patch"):
        out["n_%s_beyond" % name] = count_beyond(sub(run[name]), fix[name + "64_sub"], fix["tau"])
    out["e_l0_final"] = float(abs(int(run["l0_final"]) - int(fix["l0_final64"])))
    for k, v in sums(run).items():
        out["e_" + k] = float(rel_scalar(v, fix[k + "64"]).max())
    return out


def pgd_distances(run, fix, tag):
    out = {"n_adv_beyond": count_beyond(pgd_rows(run["adv"]), fix[tag + "adv64_rows"], fix["tau"]),
           "e_adv_sum": float(rel_scalar(_t64(run["adv"]).sum((2, 3)).numpy(), fix[tag + "adv_sum64"]).max()),
           "e_delta_absmax": abs(float((run["adv"] - run["clean"]).abs().max()) - float(fix[tag + "delta_absmax64"]))}
    if run.get("costs"):
        out["e_cost"] = rel_scalar(run["costs"], fix[tag + "cost64"][:len(run["costs"])])
    return out


# ----------------------------------------------------------------------------------------------------------------- the bounds
def bound(e_ref, margin=MARGIN, fp32_scalar=False):
    """margin x e_ref; where e_ref is 0, one fp32 rounding of the quantity.

    ``fp32_scalar``: the quantity is ONE fp32 number read back from the run (a per-step cost).  The fp32 oracle's value of it is
    itself a rounded fp32 number, so its distance from float64 lies anywhere in [0, 2^-24] relative even where its arithmetic is
    exact: an e_ref below 2^-24 is the chance of that step's rounding, not an accuracy another fp32 evaluation can be held to
    twenty times over (20 x 1.9e-9 = 3.9e-8 is less than one rounding of any fp32 result).  Such a step's e_ref counts as one
    rounding.  Measured on one MI355X, L0 attack, iteration 4: mask_cost e_ref 1.94e-9, HIP 2.39e-7 -- two ulps of the 1.07 it
    is, from K5's all-fp32 two-stage tree sum over 78,000 texels and the device's Adam and tanhf, where the same quantity's
    e_ref is 3.6e-7 at iteration 3 and 2.6e-7 at iteration 5 (HIP there: 7.1e-7, 1.0e-7).  Every other step of every attack
    meets 20 x its own e_ref without this."""
    e_ref = float(e_ref)
    if e_ref <= 0:
        return ONE_ROUNDING
    return margin * (max(e_ref, ONE_ROUNDING) if fp32_scalar else e_ref)


def texel_cap(n_ref, margin=MARGIN):
    return margin * int(n_ref) if int(n_ref) > 0 else TEXEL_FLOOR


def l0_cap(e_ref, margin=MARGIN):
    return max(L0_FLOOR, margin * float(e_ref))


class Audit(object):
    """Prints every figure beside its e_ref and its bound, collects the misses, and raises them together at the end: one run
    shows all of them."""

    def __init__(self, name, margin=MARGIN):
        self.name, self.margin, self.missed = name, margin, []

    def _row(self, what, got, ref, cap, asserted):
        ok = got <= cap
        print("%-22s %-26s e_ref %-10.4g got %-10.4g bound %-10.4g %s" % (
            self.name, what, ref, got, cap, ("ok" if ok else "MISS") if asserted else "(printed only)"))
        if asserted and not ok:
            self.missed.append("%s: %.6g > %.6g (e_ref %.6g)" % (what, got, cap, ref))

    def scalar(self, what, got, ref, asserted=True, fp32_scalar=False):
        self._row(what, float(got), float(ref), bound(ref, self.margin, fp32_scalar), asserted)

    def per_step(self, what, got, ref, asserted=None, fp32_scalar=False):
        """``fp32_scalar``: per-step costs, each one fp32 number (see bound); not for distances of whole tensors."""
        for s, (a, b) in enumerate(zip(np.atleast_1d(got), np.atleast_1d(ref))):
            self.scalar("%s[%d]" % (what, s), a, b, asserted is None or s in asserted, fp32_scalar)

    def texels(self, what, got, ref, taus, asserted=True):
        for t, a, b in zip(taus, got, ref):
            self._row("%s beyond %g" % (what, t), int(a), int(b), texel_cap(b, self.margin), asserted)

    def count(self, what, got, ref):
        self._row(what, float(got), float(ref), l0_cap(ref, self.margin), True)

    def none(self, what, got, asserted=True):
        self._row(what, int(got), 0, 0, asserted)

    def finish(self):
        assert not self.missed, "%s: %s" % (self.name, "; ".join(self.missed))
