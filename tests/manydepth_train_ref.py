"""What tests/golden/manydepth_train.npz records and how (shared by tools/make_goldens_manydepth_train.py, which runs the reference's
own ``ResnetEncoderMatching`` in train() mode, and by the tests that hold this package's encoder to it).

The objective is ``sum_i <features_i, pattern_i>`` with a fixed pattern per feature; its gradients with respect to four parameters
are kept (whole, or a strided sample).  ``run`` is the one procedure both sides follow: zero the gradients, one forward in train()
mode on tests/cost_volume_ref.encoder_inputs(), one backward.
"""
import numpy as np
import torch

FEATURE_SAMPLE = (lambda f: f[:, ::8, ::2, ::2], lambda f: f[:, ::4], lambda f: f[:, ::4], lambda f: f[:, ::4], lambda f: f[:, ::8])
REDUCE_SAMPLE = (slice(None, None, 2), slice(None, 64, 2))      # of reduce_conv.0.weight.grad[:, :64]
LAYER2_SAMPLE = (slice(None, None, 4), slice(None, None, 4))    # of layer2.0.conv1.weight.grad
GRADS = ("layer0.0.weight", "reduce_conv.0.weight", "reduce_conv.0.bias", "layer2.0.conv1.weight")


def pattern(shape, i, dtype=torch.float32):
    """A fixed, sign-changing weight per feature element: cos(0.37 n + 1.3 i) over the flattened index n."""
    n = int(np.prod(shape))
    return torch.cos(torch.arange(n, dtype=torch.float64) * 0.37 + 1.3 * i).reshape(shape).to(dtype)


def objective(feats):
    return sum((f * pattern(f.shape, i, f.dtype).to(f.device)).sum() for i, f in enumerate(feats))


def run(enc, x, form):
    """One train-mode forward + backward of ``enc`` (this package's class or the reference's).  ``form``: "zero" = the reference
    trainer's degenerate call (lookup_images * 0, a [1,1,4,4] zero pose), "none" = lookup_images=None (this package only).
    Returns (features, {parameter name: gradient})."""
    enc.train()
    enc.zero_grad(set_to_none=True)
    cur = x["current"]
    look = cur.unsqueeze(1) * 0 if form == "zero" else None
    feats, _, _ = enc(cur, look, torch.zeros(1, 1, 4, 4, dtype=cur.dtype, device=cur.device), x["K"], x["invK"])
    objective(feats).backward()
    params = dict(enc.named_parameters())
    return feats, {k: params[k].grad for k in GRADS}
