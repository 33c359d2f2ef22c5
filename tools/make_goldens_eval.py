"""Writes tests/golden/eigen_eval.npz: the reference's own ``batch_post_process_disparity`` and ``compute_errors`` (unmasked
branch) on the seeded inputs of tests/eigen_eval_ref.py.

    python tools/make_goldens_eval.py [--reference DIR]

Needs the reference tree; run where it is available.  Its MD2/evaluate_depth.py cannot be imported without OpenCV and
torchvision, and neither function needs them: the two function definitions are taken out of the file's syntax tree at run time
and compiled on their own with numpy as their only global.  Nothing of them is written anywhere.

Contents: ``pp_l`` / ``pp_r`` [3, 24, 80] float32 and ``pp_out`` float64, the post-processed pairs (``pp_r`` is already mirrored
back, as the reference passes it); ``err_gt_<i>`` / ``err_disp_<i>`` float32 vectors and ``err_out`` [cases, 8] float64, the
eight numbers for gt and pred = float32(1) / disp, both handed over as float64."""
import ast
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import make_goldens as mg  # noqa: E402
from tests import eigen_eval_ref as R  # noqa: E402

WANTED = ("batch_post_process_disparity", "compute_errors")


def reference_functions(ref_md2):
    path = os.path.join(ref_md2, "evaluate_depth.py")
    tree = ast.parse(open(path).read(), filename=path)
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED]
    assert sorted(d.name for d in defs) == sorted(WANTED), [d.name for d in defs]
    space = {"np": np}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), space)
    return space["batch_post_process_disparity"], space["compute_errors"]


def main():
    ref = sys.argv[sys.argv.index("--reference") + 1] if "--reference" in sys.argv else mg.MD2
    post_process, compute_errors = reference_functions(ref)
    out = {}
    l, r = R.pp_pairs()
    out["pp_l"], out["pp_r"], out["pp_out"] = l, r, np.asarray(post_process(l, r), dtype=np.float64)
    rows = []
    for i, (gt, disp) in enumerate(R.metric_vectors()):
        pred = (np.float32(1) / disp).astype(np.float64)
        out["err_gt_%d" % i], out["err_disp_%d" % i] = gt, disp
        rows.append([float(v) for v in compute_errors(gt.astype(np.float64), pred)])
    out["err_out"] = np.array(rows, dtype=np.float64)
    path = os.path.join(REPO, "tests", "golden", "eigen_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
