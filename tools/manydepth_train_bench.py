"""What hardening ManyDepth costs; writes profiles/manydepth_train.txt.

    python tools/manydepth_train_bench.py [--steps 10] [--warmup 3] [--batch 12] [--only a,b,c] [--commit TEXT] [--out FILE] [--append]

(a) ``ResnetEncoderMatching`` forward + backward in train() mode with ``lookup_images=None`` at 320 x 1024: the fused train path
    (K14 / K9 stem, K36 reduce_conv, K10 filter prefetch).  This part uses nothing newer than the encoder class itself, so the same
    script run on the commit before K36 measures the module path there (``--only a --append`` adds it to the same file); on a commit that has the switch it also
    times ``fuse_train = False`` in the same process, alternating with the fused path.
(b) The K36 node ``ops.reduce_conv_degenerate`` against the composition ``relu(ops.conv3x3(x, w[:, :64].contiguous(), b))`` at
    [batch, 64, 80, 256], forward + backward with parameter gradients (the composition's weight gradient is the [64, 64, 3, 3]
    slice's; autograd's scatter into the [64, 160, 3, 3] parameter is part of what it costs).
(c) The adversarial train step (``--adv_train --norm_type l_inf``, stereo) with ``--depth_net manydepth`` beside ``--depth_net
    resnet``, same batch; and each step's attack (``Trainer.update_adv_obj``) timed on its own, which says where the difference is.

Device time from HIP events around work that is already warm (every timed shape has run ``--warmup`` times), the two forms of a
comparison alternating in one process, median (min .. max) over ``--steps`` repeats.  No threshold is set anywhere: the file
records what was measured and the commit it was measured on (``--commit``, default: ``git rev-parse`` of the tree the tool runs
in, "unknown" outside a checkout).

A tool: not run by the tests.
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from depthmodelhardening_amd import networks, ops                    # noqa: E402
from depthmodelhardening_amd.depth_model import manydepth_intrinsics  # noqa: E402

torch.backends.cudnn.benchmark = False


def timed(fns, steps, warmup, inner=1):
    """{name: [ms per call]}: the callables alternate, one HIP-event pair around ``inner`` calls (more than one where a call is
    short beside the events' own resolution)."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / inner)
    return out


def fmt(ms):
    return "%9.3f (%.3f .. %.3f)" % (statistics.median(ms), min(ms), max(ms))


def part_a(a):
    dev = torch.device("cuda")
    torch.manual_seed(1)
    enc = networks.ResnetEncoderMatching(18, False, input_height=320, input_width=1024).to(dev).train()
    x = torch.rand(a.batch, 3, 320, 1024, device=dev)
    K, invK = (t.to(dev).expand(a.batch, 4, 4) for t in manydepth_intrinsics(1024, 320))
    pose = torch.zeros(1, 1, 4, 4, device=dev)
    wts = None

    def run(fused):
        nonlocal wts
        if hasattr(enc, "fuse_train"):
            enc.fuse_train = fused
        enc.zero_grad(set_to_none=True)
        feats, _, _ = enc(x, None, pose, K, invK)
        if wts is None:
            wts = [torch.rand_like(f) for f in feats]
        sum((f * w).sum() for f, w in zip(feats, wts)).backward()
    fns = {"fused train path": lambda: run(True), "module path (fuse_train = False)": lambda: run(False)} if hasattr(enc, "fuse_train") \
        else {"module path (this commit has no fused train path)": lambda: run(False)}
    res = timed(fns, a.steps, a.warmup)
    lines = ["(a) ResnetEncoderMatching forward + backward, train(), lookup_images=None, [%d, 3, 320, 1024]: ms median (min .. max)" % a.batch]
    lines += ["    %-52s %s" % (k, fmt(v)) for k, v in res.items()]
    return lines


def part_b(a):
    dev = torch.device("cuda")
    g0 = torch.Generator().manual_seed(2)
    x = torch.randn(a.batch, 64, 80, 256, generator=g0).to(dev).requires_grad_(True)
    w = (torch.randn(64, 160, 3, 3, generator=g0) * 0.05).to(dev).requires_grad_(True)
    b = (torch.randn(64, generator=g0) * 0.1).to(dev).requires_grad_(True)
    g = torch.randn(a.batch, 64, 80, 256, generator=g0).to(dev)

    def node():
        x.grad = w.grad = b.grad = None
        ops.reduce_conv_degenerate(x, w, b).backward(g)

    def composed():
        x.grad = w.grad = b.grad = None
        torch.relu(ops.conv3x3(x, w[:, :64].contiguous(), b)).backward(g)
    res = timed({"K36 node (ops.reduce_conv_degenerate)": node, "relu(ops.conv3x3(x, w[:, :64].contiguous(), b))": composed},
                max(a.steps, 20), max(a.warmup, 10), inner=50)
    lines = ["(b) reduce_conv, degenerate call, forward + backward, x [%d, 64, 80, 256], weight [64, 160, 3, 3], 50 calls per event pair: ms per call, median (min .. max)" % a.batch]
    lines += ["    %-52s %s" % (k, fmt(v)) for k, v in res.items()]
    return lines


def part_c(a):
    from depthmodelhardening_amd.options import MonodepthOptions
    from depthmodelhardening_amd.trainer import Trainer
    trainers = {}
    for net in ("manydepth", "resnet"):
        argv = ["--dataset", "synthetic", "--height", "320", "--width", "1024", "--batch_size", str(a.batch), "--weights_init", "scratch",
                "--frame_ids", "0", "--use_stereo", "--adv_train", "--norm_type", "l_inf", "--depth_net", net,
                "--log_dir", tempfile.mkdtemp(), "--synthetic_len", str(a.batch * (a.steps + a.warmup + 2))]
        torch.manual_seed(1)
        tr = Trainer(MonodepthOptions().parse(argv), device=torch.device("cuda"))
        tr.set_train()
        trainers["--depth_net " + net] = tr
    res = timed({k: tr.train_step for k, tr in trainers.items()}, a.steps, a.warmup)
    lines = ["(c) adversarial train step (--adv_train --norm_type l_inf, --frame_ids 0 --use_stereo), 320 x 1024, batch %d: ms median (min .. max)" % a.batch]
    lines += ["    %-52s %s" % (k, fmt(v)) for k, v in res.items()]
    # where a step's time goes: its attack (update_adv_obj: the PGD steps through the eval-mode wrapper) timed on its own
    res = timed({k: tr.update_adv_obj for k, tr in trainers.items()}, a.steps, 1)
    lines += ["    of which the attack alone (Trainer.update_adv_obj):"]
    lines += ["    %-52s %s" % (k, fmt(v)) for k, v in res.items()]
    return lines


def commit_of_tree():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                              text=True, check=True).stdout.strip() or "unknown"
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "manydepth_train.txt"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (part (a) of an earlier commit)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("manydepth_train_bench: needs the GPU (a CPU run measures nothing)")
    lines = ["ManyDepth hardening, device time from HIP events, %s, measured on commit: %s" % (
        torch.cuda.get_device_name(0), a.commit or commit_of_tree()), ""]
    for name, part in (("a", part_a), ("b", part_b), ("c", part_c)):
        if name in a.only.split(","):
            lines += part(a) + [""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
