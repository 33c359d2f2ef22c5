"""bench.py's N > 1 branch on the ONE GPU this suite has: two ranks share GPU 0 over gloo (RCCL needs a GPU per rank; the
driver runs the real 8-GPU bench).  What runs here is everything of that branch but the ring itself: the launcher, the
rank-0-first warm-up, shorten_timeout, the timed region with the side-stream all-reduce overlapped with the next attack, the
second timing in the other attack / all-reduce order, the all-reduce's HIP-event durations in the JSON line, and a rank that
stops taking part.  The ranks are started by the launcher BEFORE anything touches the GPU (bench.launch_ranks).  The per-kernel
and per-order figures are --full's; a plain single-rank run and its --dump-outputs are checked at the end."""
import json
import os
import subprocess
import sys
import time

import pytest

# one xdist group: these tests start rank processes of their own, and the box allows six processes on the GPU
pytestmark = [pytest.mark.gpu, pytest.mark.xdist_group("ranks")]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--gpus", "2", "--steps", "2", "--warmup", "1", "--batch_size", "4", "--atk_scenes", "2", "--no_cpu_baseline", "--full"]


def _bench(extra=(), env=None, timeout=600, flags=FLAGS):
    e = dict(os.environ, DMH_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "DMH_BENCH_CHILD"):
        e.pop(k, None)
    e.update(env or {})
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + flags + list(extra), cwd=REPO, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    return r, time.time() - t0


def _line(r):
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[0])


@pytest.mark.parametrize("shared", [False, True])
def test_two_ranks_on_one_gpu(shared):
    r, _ = _bench(["--shared_patch"] if shared else [])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "rank 0 warmed the kernel cache" in r.stderr
    d = _line(r)
    cfg = d["config"]
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert cfg["global_batch"] == 8 and cfg["parallelism"] == "dp2" and cfg["attack_overlap"] is True
    assert cfg["shared_patch"] is shared and cfg["attack_scenes"] == 2
    assert cfg["final_loss"] == cfg["final_loss"] and abs(cfg["final_loss"]) < 1e3          # finite
    other = cfg["other_order"]
    assert other["mode"] == "sync_attack" and other["value"] > 0 and other["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] / 8e3 - 1) < 1e-3
    # the gradient exchange of every timed step, by HIP events on the side stream
    ar = cfg["all_reduce"]
    assert ar["launches"] == 2 and ar["bucket_mb"] == pytest.approx(57.3, abs=0.05) and ar["backend"] == "gloo"
    assert 0 < ar["all_reduce_ms_per_step"] <= ar["all_reduce_ms_max"] * (1 + 1e-6)
    assert 0 <= ar["optimizer_wait_ms_per_step"] <= ar["optimizer_wait_ms_max"] + 1e-6
    assert d["roofline"]["kernel"] == "photo_bwd_kernel" and "cpu_baseline" not in d


def test_a_rank_that_stops_fails_the_job_within_the_shortened_timeout():
    """Rank 1 stops taking part after the warm-up: rank 0 sits in the next step's gradient all-reduce until the process group's
    steady-state timeout (DMH_DIST_STEADY_TIMEOUT_MIN, here 0.1 min) fails it; the launcher then stops rank 1 and exits
    non-zero -- minutes earlier than the 60-minute start-up timeout would."""
    r, took = _bench(env={"DMH_BENCH_AFTER_WARMUP": "hang:1", "DMH_DIST_STEADY_TIMEOUT_MIN": "0.1"}, timeout=420)
    assert r.returncode != 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "stopping the other ranks" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert took < 400


def test_a_rank_that_dies_fails_the_job_at_once():
    r, _ = _bench(env={"DMH_BENCH_AFTER_WARMUP": "exit:1"}, timeout=420)
    assert r.returncode != 0 and "rank 1 exited with 3" in r.stderr


def test_plain_single_rank_run_and_its_dumped_outputs(tmp_path):
    """Without --full the line carries the contract fields and nothing that takes work of its own (no roofline, no CPU
    baseline); --steps sets the timed steps; --dump-outputs writes the last timed step's losses, a fixed sample of the gradient
    and weights, and the attack's patch, as finite float32 arrays."""
    import numpy as np
    flags = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch_size", "4", "--atk_scenes", "2"]
    r, _ = _bench(["--dump-outputs", str(tmp_path)], flags=flags)
    assert r.returncode == 0, r.stderr[-4000:]
    d = _line(r)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["unit"] == "images/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["value"] > 0 and d["metric"].startswith("adv-train images/sec @1024x320")
    assert abs(d["value"] * d["ms_per_step"] / 4e3 - 1) < 1e-3
    assert "roofline" not in d and "cpu_baseline" not in d and "other_order" not in d["config"]
    files = {f[:-4]: np.load(str(tmp_path / f)) for f in os.listdir(str(tmp_path))}
    assert {"loss", "loss_0", "grad_sample", "weights_sample", "adv_patch"} <= set(files), sorted(files)
    assert files["grad_sample"].shape == files["weights_sample"].shape == (1 << 20,)
    assert files["adv_patch"].shape[-3:] == (3, 260, 300)
    for name, x in files.items():
        assert x.dtype == np.float32 and np.isfinite(x).all(), name
    assert abs(float(files["loss"]) - d["config"]["final_loss"]) <= 1e-6
    assert np.abs(files["grad_sample"]).max() > 0
