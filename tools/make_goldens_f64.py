"""Writes tests/golden/atk_linf_f64.npz, atk_l0_f64.npz and atk_pgd_f64.npz: one float64 trajectory per training-path attack.

    python tools/make_goldens_f64.py            (writes the three files)
    python tools/make_goldens_f64.py --check    (runs the same and compares with the committed files instead)

CPU only; imports oracle/ alone.  Each attack of oracle/attack_ref.py runs twice -- in fp32 and in float64 -- on the inputs of the
GPU tests in tests/test_gpu_attacks.py (oracle/f64_anchor.py: TinyDepthNet(seed=5) built in fp32 and converted, two scenes, 3 steps,
the fixtures' seeds; the start draws are the fp32 ones in both runs, the poses come from the same ``random`` state).  The fp32 run
is the one tests/golden/atk_{linf,l0,pgd_*}.npz record of the reference; tests/test_attack_f64_ref.py checks that bit for bit.

Stored per attack:
  * the float64 trajectory: per-step costs as float64; per-step gradients, the final patch, the L0 patterns and the PGD rows as the
    float64 values ROUNDED TO fp32, at the subsampling of the sibling fixtures ([::2, ::2]; PGD [::16, ::8]; the L0 pattern
    gradients at [::4, ::4] for the first iteration and [::8, ::8] for the later ones, which are only printed).  That rounding is
    6e-8 relative: far below every tolerance that is held against these tensors (the smallest: tau = 1e-6 on values of [0, 1],
    and gradient distances of 1e-5 relative);
  * for the L0 attack the per-iteration (l0, mask_weight, adv_cost, mask_cost), also for the second, scalars-only case of
    test_l0_attack_trace_vs_oracle (keys ``t_*``);
  * adv_sum, ben_sum, mask_out_sum of the returned scenes;
  * e_ref -- keys ``e_*`` (errors) and ``n_*`` (texel counts): the fp32 run's own distance from that trajectory, one value for
    every quantity the GPU tests assert, measured by oracle/f64_anchor.py on the stored (subsampled, rounded) tensors exactly as
    the tests measure the HIP run;
  * ``zero_only32_<gradient>`` / ``zero_only64_<gradient>``: per step, the texels where one form's gradient is exactly zero
    and the other's is not.  Where both are 0 for a step the two zero sets are identical, and the GPU tests hold HIP to that set
    (the first step of every attack; later the forms clamp different texels at 0 or 1).

A tool: not run by the tests (the runs and the distances they share with it are in oracle/f64_anchor.py).
"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import f64_anchor as A          # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
F32, F64 = torch.float32, torch.float64


def r32(t):
    """A float64 tensor as stored: rounded to fp32."""
    return t.detach().to(F32).numpy()


def zero_sets(name, g32, g64):
    """Per step, on the whole tensors: texels that are exactly zero in the fp32 gradient alone / in the float64 one alone."""
    only32 = np.asarray([int(((a == 0) & (b != 0)).sum()) for a, b in zip(g32, g64)], dtype=np.int64)
    only64 = np.asarray([int(((a != 0) & (b == 0)).sum()) for a, b in zip(g32, g64)], dtype=np.int64)
    return {"zero_only32_" + name: only32, "zero_only64_" + name: only64}


def build_linf():
    c = A.LINF
    r_32, r_64 = A.run_linf(F32), A.run_linf(F64)
    fix = dict(shape=np.array([2, c["steps"], c["seed"]]), tau=np.asarray(c["tau"]), cost64=np.asarray(r_64["costs"]),
               cost32=np.asarray(r_32["costs"]), grad64_sub=np.stack([r32(A.sub(g)) for g in r_64["grads"]]),
               patch64_sub=r32(A.sub(r_64["patch"])), n_sub=np.int64(A.sub(r_64["patch"]).numel()),
               zero_frac=np.float64(float((r_64["grads"][0] == 0).double().mean())))
    fix.update(zero_sets("grad", r_32["grads"], r_64["grads"]))
    fix.update({k + "64": v for k, v in A.sums(r_64).items()})
    fix.update(A.linf_distances(r_32, fix))
    return fix, r_32


def build_l0():
    c = A.L0
    r_32, r_64 = A.run_l0(F32), A.run_l0(F64)
    assert len(r_32["trace"]) == len(r_64["trace"]), "fp32 and float64 ran different numbers of iterations"
    k1, k2 = A.GRAD_SUB_L0_FIRST, A.GRAD_SUB_L0_LATER
    fix = dict(shape=np.array([2, c["steps"], c["seed"]]), tau=np.asarray(c["tau"]),
               trace64=np.asarray(r_64["trace"], dtype=np.float64), trace32=np.asarray(r_32["trace"], dtype=np.float64),
               n_sub=np.int64(A.sub(r_64["patch"]).numel()), l0_final64=np.int64(r_64["l0_final"]))
    for name in ("gpos", "gneg"):
        fix.update(zero_sets(name, r_32[name], r_64[name]))
    for name in ("gpos", "gneg"):
        fix[name + "64_first"] = r32(A.sub(r_64[name][0], k1))
        fix[name + "64_later"] = np.stack([r32(A.sub(g, k2)) for g in r_64[name][1:]])
    for name in ("pos", "neg", "patch"):
        fix[name + "64_sub"] = r32(A.sub(r_64[name]))
    fix.update({k + "64": v for k, v in A.sums(r_64).items()})
    fix.update(A.l0_distances(r_32, fix))
    # the scalars-only second case
    t_32, t_64 = A.run_l0(F32, A.L0_TRACE), A.run_l0(F64, A.L0_TRACE)
    fix["t_shape"] = np.array([2, A.L0_TRACE["steps"], A.L0_TRACE["seed"], A.L0_TRACE["scene_seed"]])
    fix["t_trace64"] = np.asarray(t_64["trace"], dtype=np.float64)
    fix["t_trace32"] = np.asarray(t_32["trace"], dtype=np.float64)
    fix.update({"t_" + k: v for k, v in A.l0_trace_distances(t_32["trace"], fix["t_trace64"]).items()})
    return fix, r_32, t_32


def build_pgd():
    c = A.PGD
    fix, runs = dict(shape=np.array([2, c["steps"], c["seed"]]), tau=np.asarray(c["tau"])), {}
    for targeted in (True, False):
        tag = "targeted_" if targeted else "untargeted_"
        r_32, r_64 = A.run_pgd(F32, targeted), A.run_pgd(F64, targeted)
        fix[tag + "cost64"] = np.asarray(r_64["costs"])
        fix[tag + "adv64_rows"] = r32(A.pgd_rows(r_64["adv"]))
        fix[tag + "adv_sum64"] = r_64["adv"].sum((2, 3)).numpy()
        fix[tag + "delta_absmax64"] = np.float64(float((r_64["adv"] - r_64["clean"]).abs().max()))
        fix[tag + "n_rows"] = np.int64(A.pgd_rows(r_64["adv"]).numel())
        g32, g64 = r_32["grads"], r_64["grads"]
        fix[tag + "e_grad_rel"] = np.asarray([A.tensor_distance(a, b)[0] for a, b in zip(g32, g64)])
        fix.update({tag + k: v for k, v in A.pgd_distances(r_32, fix, tag).items()})
        runs[targeted] = r_32
    return fix, runs


def show(name, fix):
    for k in sorted(fix):
        if k.startswith(("e_", "n_", "t_e_", "zero", "cost", "trace64", "targeted_e_", "targeted_n_", "untargeted_e_", "untargeted_n_")):
            print("  %-12s %-34s %s" % (name, k, np.array2string(np.asarray(fix[k]), precision=3)))


def save_or_check(name, fix, check):
    path = os.path.join(OUT, name + ".npz")
    fix = {k: np.asarray(v) for k, v in fix.items()}
    if check:
        old = np.load(path)
        diff = [k for k in sorted(set(fix) | set(old.files)) if k not in fix or k not in old.files
                or not np.array_equal(fix[k], old[k])]
        print("%-20s %s" % (name + ".npz", "reproduced" if not diff else "DIFFERS in %s" % diff))
        return not diff
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(path, **fix)
    print("wrote %-24s %7.1f KiB" % (name + ".npz", os.path.getsize(path) / 1024.0))
    return True


def main():
    check = "--check" in sys.argv
    ok = True
    for name, build in (("atk_linf_f64", build_linf), ("atk_l0_f64", build_l0), ("atk_pgd_f64", build_pgd)):
        t0 = time.time()
        fix = build()[0]
        print("%s: %.0f s" % (name, time.time() - t0))
        show(name, fix)
        ok = save_or_check(name, fix, check) and ok
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
