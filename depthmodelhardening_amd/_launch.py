"""What every operator module launches through: the per-launch profile, the Philox draw, the operand checks and the
upload cache of the small device tables.  ops.py, attack_ops.py, eval_ops.py and data_ops.py import it; it imports none of them.
"""
from collections import OrderedDict

import torch

# Optional per-launch HIP-event timing of the K1 kernels (bench.py's roofline figure): a dict
# name -> list of (start, end) torch.cuda.Event pairs recorded on the launch stream, or None (off).
_profile = None
_profile_only = None


def enable_profile(on=True, only=None):
    """HIP-event timing of the instrumented launches.  ``only``: tuple of name prefixes to time (the others launch
    untouched) -- an event pair adds ~10 us of dispatch latency around a launch, so a timed region should carry events
    on the kernels it reports and nothing else."""
    global _profile, _profile_only
    _profile = {} if on else None
    _profile_only = tuple(only) if (on and only) else None


def profile_ms():
    """Average launch duration in ms per instrumented kernel (synchronises)."""
    if not _profile:
        return {}
    torch.cuda.synchronize()
    return {k: sum(e[0].elapsed_time(e[1]) for e in v) / len(v) for k, v in _profile.items() if v}


def profile_bytes():
    """Per instrumented kernel: (launches, total ms, total algorithmic bytes, total direct-convolution flops) -- for
    kernels whose shape varies from launch to launch."""
    if not _profile:
        return {}
    torch.cuda.synchronize()
    return {k: (len(v), sum(e[0].elapsed_time(e[1]) for e in v), sum(e[2] for e in v), sum(e[3] for e in v))
            for k, v in _profile.items() if v}


def profiling_every_launch():
    """True while enable_profile(True) without ``only`` is in force: every instrumented launch carries an event pair (bench.py's
    one fully instrumented step).  Events cannot be read back from a captured HIP graph, so the attack runs that step eagerly."""
    return _profile is not None and _profile_only is None


def _timed(name, launch, nbytes=0, flops=0):
    if _profile is None or (_profile_only is not None and not name.startswith(_profile_only)):
        return launch()
    if torch.cuda.is_current_stream_capturing():      # an event recorded into a graph has no time stamp to read
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = launch()
    e1.record()
    _profile.setdefault(name, []).append((e0, e1, nbytes, flops))
    return rc


def _philox(device, count):
    """(seed, offset) for the in-kernel tie-break noise, drawn from torch's CUDA generator state so
    that torch.manual_seed() makes runs reproducible; the generator offset is advanced past the
    ``count`` counters this call consumes."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    seed, off = gen.initial_seed(), gen.get_offset()
    gen.set_offset(off + ((count + 3) // 4) * 4)
    return seed & 0xFFFFFFFFFFFFFFFF, off


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _need_cuda(t):
    """A CPU operand (``t``: a tensor or a torch.device) is an error, never another code path."""
    device = t if isinstance(t, torch.device) else t.device
    if device.type != "cuda":
        raise RuntimeError("libdmh_hip ops need CUDA (ROCm) tensors; got device %s -- there is no CPU path" % device)


def _need_f32(t, name):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise RuntimeError("libdmh_hip ops compute in fp32; got %s for %s" % (getattr(t, "dtype", type(t)), name))
    return t


def _need_i32(t, name):
    if not torch.is_tensor(t) or t.dtype != torch.int32:
        raise RuntimeError("%s must be int32; got %s" % (name, getattr(t, "dtype", type(t))))
    return t


class _UploadCache(object):
    """The last ``cap`` sets of small tables a loader operator has uploaded, by key, so that a repeated batch shape launches with
    the same device buffers and no copy.  An entry keeps the event of its upload -- a hit on another stream a moment later waits
    for it -- and the pinned host copies, which live as long as the upload may.  A key a captured graph has launched with is
    ``held``: a replay reads its buffers, so it is never evicted.  ``what``: the error a miss raises inside a capture."""

    def __init__(self, cap, what):
        self.cap, self.what, self.entries, self.held = cap, what, OrderedDict(), set()

    def __len__(self):
        return len(self.entries)

    def __contains__(self, key):
        return key in self.entries

    def get(self, key, device, make):
        """(device tensors, payload) of ``key``; at a miss ``make()`` gives (host tensors, payload): the tensors are pinned and
        uploaded without a wait, the payload (host values that go with them) is kept as it is."""
        hit = self.entries.get(key)
        if hit is not None:
            self.entries.move_to_end(key)
            if torch.cuda.is_current_stream_capturing():
                self.held.add(key)
            elif not hit[1].query():
                torch.cuda.current_stream(device).wait_event(hit[1])        # uploaded on another stream a moment ago
            return hit[0], hit[3]
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(self.what)
        host, payload = make()
        host = [h.pin_memory() for h in host]
        on_device = [h.to(device, non_blocking=True) for h in host]
        uploaded = torch.cuda.Event()
        uploaded.record(torch.cuda.current_stream(device))
        self.entries[key] = (on_device, uploaded, host, payload)
        for old in [k for k in self.entries if k not in self.held][:max(0, len(self.entries) - self.cap)]:
            del self.entries[old]
        return on_device, payload


def _flip_operand(name, flip, n, dev):
    """The per-item ``flip`` of a loader operator as the kernel reads it: None, or a contiguous int32 tensor of ``n`` entries on
    ``dev`` (a host sequence of bools is uploaded from pinned memory)."""
    if flip is None:
        return None
    if not torch.is_tensor(flip):
        flip = torch.tensor([int(bool(v)) for v in flip], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    if flip.dtype != torch.int32 or flip.numel() != n or flip.device != dev:
        raise RuntimeError("%s: flip must be an int32 tensor of %d entries on %s" % (name, n, dev))
    return _c(flip)
