"""Times the pose head and the monocular train step; writes profiles/mono_step.txt.

    python tools/mono_step_bench.py [--steps 10] [--warmup 3] [--batch 12] [--out profiles/mono_step.txt]

(a) The head: K29 forward + backward (``ops.pose_head``) beside the torch expressions of the same head -- the module path of
    ``networks.PoseDecoder`` / ``layers.transformation_from_parameters``, i.e. the reference's arithmetic (MD2/networks/
    pose_decoder.py:47-52, MD2/layers.py:28-103), run on the same CUDA tensor -- at the workload's shape [B, 12, 10, 32], per source
    frame: kernel launches from the profiler, milliseconds from HIP events (200 calls between two events, median of five).
(b) The step: ``--frame_ids 0 -1 1 --use_stereo --pose_net`` at 320 x 1024 beside the stereo-only step (``--frame_ids 0
    --use_stereo``, what the trainer served before the pose networks), same batch, HIP events around ``train_step``.

A tool: not run by the tests.  No timing is claimed anywhere until this file's output exists.
"""
import argparse
import os
import statistics
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from depthmodelhardening_amd import layers, ops                      # noqa: E402
from depthmodelhardening_amd.options import MonodepthOptions         # noqa: E402
from depthmodelhardening_amd.trainer import Trainer                  # noqa: E402

torch.backends.cudnn.benchmark = False


def torch_head(x, invert, nf=2):
    """The reference's expressions on a CUDA tensor (layers' own fall-back forms, K29 switched off)."""
    saved = layers._pose_head_ok
    layers._pose_head_ok = lambda *a: False
    try:
        out = 0.01 * x.mean(3).mean(2).view(-1, nf, 1, 6)
        axisangle, translation = out[..., :3], out[..., 3:]
        return axisangle, translation, layers.transformation_from_parameters(axisangle[:, 0], translation[:, 0], invert=invert)
    finally:
        layers._pose_head_ok = saved


def hip_head(x, invert, nf=2):
    axisangle, translation, T = ops.pose_head(x, invert)
    return axisangle, translation, T[:, 0]


def fwd_bwd(head, x, w, invert):
    x.grad = None
    (head(x, invert)[2] * w).sum().backward()


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def event_ms(fn, repeats=200):
    for _ in range(10):
        fn()
    res = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(repeats):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / repeats)
    return statistics.median(res)


def step_ms(extra, batch, steps, warmup):
    argv = ["--dataset", "synthetic", "--height", "320", "--width", "1024", "--batch_size", str(batch), "--weights_init", "scratch",
            "--log_dir", tempfile.mkdtemp(), "--synthetic_len", str(batch * (steps + warmup + 1))] + extra
    torch.manual_seed(1)
    tr = Trainer(MonodepthOptions().parse(argv), device=torch.device("cuda"))
    tr.set_train()
    for _ in range(warmup):
        tr.train_step()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.train_step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mono_step.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    x = (torch.randn(a.batch, 12, 10, 32, device=dev) * 10).requires_grad_(True)
    w = torch.randn(a.batch, 4, 4, device=dev)
    lines = ["pose head, x [%d, 12, 10, 32], forward + backward of sum(T[:, 0] * w)" % a.batch,
             "%-34s %10s %14s" % ("form", "launches", "ms (HIP events)")]
    for name, head in (("K29 (ops.pose_head)", hip_head), ("torch expressions (module path)", torch_head)):
        for invert in (False, True):
            fn = lambda head=head, invert=invert: fwd_bwd(head, x, w, invert)      # noqa: E731
            lines.append("%-34s %10d %14.4f" % (name + (", invert" if invert else ""), launches(fn), event_ms(fn)))
    lines += ["", "train step, 320 x 1024, batch %d, %d steps after %d warm-up: ms median (min .. max)" % (a.batch, a.steps, a.warmup)]
    for name, extra in (("stereo only (--frame_ids 0 --use_stereo)", ["--frame_ids", "0", "--use_stereo"]),
                        ("mono + stereo (--frame_ids 0 -1 1 --use_stereo --pose_net)", ["--frame_ids", "0", "-1", "1", "--use_stereo", "--pose_net"])):
        med, lo, hi = step_ms(extra, a.batch, a.steps, a.warmup)
        lines.append("%-62s %8.2f (%.2f .. %.2f)" % (name, med, lo, hi))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
