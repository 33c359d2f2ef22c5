"""Writes tests/golden/manydepth_train.npz by running the reference's own ``ResnetEncoderMatching``
(manydepth2/networks/resnet_encoder.py) in train() mode on the CPU, in the call its trainer makes (manydepth2/trainer.py:371-385:
``lookup_images * 0`` and a [1,1,4,4] zero pose).

    python tools/make_goldens_manydepth_train.py [--reference DIR]

The reference class is imported exactly as tools/make_goldens_manydepth.py imports it (``reference_class``).  Inputs:
tests/cost_volume_ref.encoder_inputs() (2 x 3 x 48 x 96) and the formula state dict; the procedure is
tests/manydepth_train_ref.run.  Recorded (data only):

  features0 .. features4   the five features, subsampled (manydepth_train_ref.FEATURE_SAMPLE)
  bn0_mean / bn0_var / bn0_batches             ``layer0.1`` running statistics and num_batches_tracked after the forward.  The
                           reference also sends the all-zero lookup frame through layer0 / layer1 in train() mode, so these have
                           been updated TWICE (bn0_batches = 3 + 2);
  bn0_mean_first / bn0_var_first               the same after the current frame's pass alone (a forward hook on the reference's own
                           BatchNorm module copies them out after its first call)
  grad_layer0_0_weight, grad_reduce_weight (strided sample of [:, :64]), grad_reduce_bias, grad_layer2_0_conv1_weight (strided
                           sample): the gradients of sum_i <features_i, pattern_i>
  reduce_tail_nonzero      the number of non-zero entries of reduce_conv.0.weight.grad[:, 64:]

A tool: not run by the tests.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from oracle import make_goldens as mg          # noqa: E402
from tests import cost_volume_ref as R         # noqa: E402
from tests import manydepth_train_ref as T     # noqa: E402
from make_goldens_manydepth import reference_class      # noqa: E402

ARGV = list(sys.argv)
OUT = os.path.join(REPO, "tests", "golden", "manydepth_train.npz")


def main():
    ref_dir = ARGV[ARGV.index("--reference") + 1] if "--reference" in ARGV else mg.REF
    Ref = reference_class(ref_dir)
    enc = Ref(18, False, input_height=48, input_width=96)
    shapes = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict(R.formula_state_dict(shapes), strict=False)
    bn0 = enc.layer0[1]
    first = {}

    def after_first(mod, _inp, _out):
        if not first:
            first["mean"], first["var"] = mod.running_mean.clone(), mod.running_var.clone()
    handle = bn0.register_forward_hook(after_first)
    x = {k: torch.from_numpy(v) for k, v in R.encoder_inputs().items()}
    feats, grads = T.run(enc, x, "zero")
    handle.remove()
    out = {"features%d" % i: T.FEATURE_SAMPLE[i](f.detach()).contiguous().numpy() for i, f in enumerate(feats)}
    out.update(bn0_mean=bn0.running_mean.numpy(), bn0_var=bn0.running_var.numpy(), bn0_batches=np.array(int(bn0.num_batches_tracked)),
               bn0_mean_first=first["mean"].numpy(), bn0_var_first=first["var"].numpy())
    gr = grads["reduce_conv.0.weight"]
    out["grad_layer0_0_weight"] = grads["layer0.0.weight"].numpy()
    out["grad_reduce_weight"] = gr[:, :64][T.REDUCE_SAMPLE].contiguous().numpy()
    out["grad_reduce_bias"] = grads["reduce_conv.0.bias"].numpy()
    out["grad_layer2_0_conv1_weight"] = grads["layer2.0.conv1.weight"][T.LAYER2_SAMPLE].contiguous().numpy()
    out["reduce_tail_nonzero"] = np.array(int((gr[:, 64:] != 0).sum()))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes); batches tracked %d, non-zero entries of weight.grad[:, 64:]: %d, |grad bias| %.3f" % (
        OUT, os.path.getsize(OUT), int(out["bn0_batches"]), int(out["reduce_tail_nonzero"]), float(np.abs(out["grad_reduce_bias"]).mean())))


if __name__ == "__main__":
    main()
