"""K30 (csrc/cost_volume.hip, ``ops.cost_volume``) on the GPU against the float64 restatement of tests/cost_volume_ref.py.

The gate is the project's (tests/test_gpu_pose.py): pooled over the cases, on ``cost_volume``,
    e_hip = ||HIP - float64||  <=  1.5 * e_ref + 2^-24 * ||float64||,    e_ref = ||float32 restatement - float64||.
A pixel column (b, h, w) is excluded when any of its sample positions lies within 1e-3 pixel of a threshold of the edge mask in
float64 (one flipped flag changes the column's count, maximum and confidence); at most 10 % of a case's columns may be excluded.
On the kept columns ``missing_mask``, ``confidence_mask`` and ``argmin`` equal the float64 form's; where the two smallest float64
costs of a column differ by less than 4 * 2^-24 * cost either index is accepted, and at most 1 % of the columns may be such.
"""
import numpy as np
import pytest
import torch

from tests import cost_volume_ref as R
from tests.test_gpu_pose import Pool

pytestmark = pytest.mark.gpu

_ref = {}


def _forms(name):
    if name not in _ref:
        c = R.case(name)
        _ref[name] = (c, R.forward(c, np.float32), R.forward(c, np.float64))
    return _ref[name]


def _run(c, **kw):
    from depthmodelhardening_amd import ops
    t = [torch.from_numpy(c[k]).cuda() for k in ("current", "lookup", "poses", "K", "invK", "bins")]
    return ops.cost_volume(*t, **kw)


def _check_flags(name, out, f64):
    cost, missing, conf, idx = (o.cpu().numpy() for o in out)
    keep = f64["margin"] >= R.EXCLUDE
    amb = f64["gap_ok"]
    excluded, ambiguous = 1.0 - keep.mean(), float((amb & keep).mean())
    k4 = np.broadcast_to(keep[:, None], cost.shape)
    n_miss = int((missing[k4] != f64["missing"][k4]).sum())
    n_conf = int((conf[keep] != f64["confidence"][keep]).sum())
    n_arg = int((idx[keep & ~amb] != f64["argmin"][keep & ~amb]).sum())
    either = idx[keep & amb]
    print("%s: excluded columns %.4f, ambiguous argmin columns %.4f; differing on kept columns: missing %d, confidence %d, argmin %d; "
          "max |cost - f64| %.3g on costs up to %.3g; missing share %.2f, confidence share %.2f" % (
              name, excluded, ambiguous, n_miss, n_conf, n_arg, np.abs(cost - f64["cost"])[k4].max(initial=0.0), f64["cost"].max(),
              f64["missing"].mean(), f64["confidence"].mean()))
    assert excluded <= 0.10 and ambiguous <= 0.01
    assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < cost.shape[1] and np.isfinite(cost).all()
    assert n_miss == 0 and n_conf == 0 and n_arg == 0
    if either.size:         # an ambiguous column: the index is one of the two smallest float64 costs
        viz = np.where(f64["cost"] == 0, 100.0, f64["cost"])
        two = np.argsort(viz, 1, kind="stable")[:, :2]
        sel = keep & amb
        assert np.all((either == two[:, 0][sel]) | (either == two[:, 1][sel]))
    return k4


def test_k30_against_the_float64_restatement():
    pool = Pool("cost_volume")
    for name in ("A", "B"):
        c, f32, f64 = _forms(name)
        out = _run(c)
        k4 = _check_flags(name, out, f64)
        pool.add(out[0].cpu().numpy()[k4], f32["cost"][k4], f64["cost"][k4])
        assert 0.1 < f64["missing"].mean() < 0.9 and 0.1 < f64["confidence"].mean() < 0.9        # every branch is populated
    pool.check()


@pytest.mark.parametrize("name", ["A_bp1", "odd"])
def test_k30_short_pose_batch_and_odd_shape(name):
    """poses [1,L,4,4] at B = 2 (the second sample has no lookups); 9 x 37 with 19 bins: two tiles of 32 pixels, the second with
    5, and a second block of bins with 3."""
    c, f32, f64 = _forms(name)
    out = _run(c)
    k4 = _check_flags(name, out, f64)
    pool = Pool(name)
    pool.add(out[0].cpu().numpy()[k4], f32["cost"][k4], f64["cost"][k4])
    pool.check()
    if name == "A_bp1":
        assert not out[0][1].any() and out[1][1].all() and not out[2][1].any() and not out[3][1].any()


def test_k30_all_poses_zero_is_empty():
    c, _, _ = _forms("A_zero")
    cost, missing, conf, idx = _run(c)
    assert not cost.any() and missing.all() and not conf.any() and not idx.any()


def test_k30_is_bitwise_repeatable_and_the_tile_order_changes_no_bit():
    from depthmodelhardening_amd import ops
    c, _, _ = _forms("B")
    a, b = _run(c), _run(c)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    saved = ops.COST_VOLUME_BANDED
    try:
        ops.COST_VOLUME_BANDED = not saved
        d = _run(c)
    finally:
        ops.COST_VOLUME_BANDED = saved
    assert all(torch.equal(u, v) for u, v in zip(a, d))
    e = _run(c, set_missing_to_max=False)       # the missing entries stay 0; everything else is the same
    assert torch.equal(e[1], a[1]) and torch.equal(e[2], a[2]) and torch.equal(e[0], a[0] * (1 - a[1]))
    assert torch.equal(e[0] == 0, a[1] == 1)


def test_k30_buffer_form_and_library_op():
    from depthmodelhardening_amd import library, ops  # noqa: F401
    c, _, _ = _forms("B")
    t = [torch.from_numpy(c[k]).cuda() for k in ("current", "lookup", "poses", "K", "invK", "bins")]
    cost, missing, conf, idx = ops.cost_volume(*t)
    D = cost.shape[1]
    buf = torch.full((2, 64 + D, 16, 40), -7.0, device="cuda")
    none_c, none_m, conf2, idx2 = ops.cost_volume(*t, into=buf)
    assert none_c is None and none_m is None and torch.equal(conf2, conf) and torch.equal(idx2, idx)
    assert torch.equal(buf[:, 64:], cost * conf.unsqueeze(1)) and bool((buf[:, :64] == -7.0).all())
    out = torch.ops.dmh.cost_volume(*t)
    assert all(torch.equal(u, v) for u, v in zip(out, (cost, missing, conf, idx)))
    buf2 = torch.zeros_like(buf)
    conf3, idx3 = torch.ops.dmh.cost_volume_into(*t, buf2)
    assert torch.equal(buf2[:, 64:], buf[:, 64:]) and torch.equal(conf3, conf) and torch.equal(idx3, idx)
    torch.library.opcheck(torch.ops.dmh.cost_volume, tuple(t), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(RuntimeError, match="rows"):
        ops.cost_volume(t[0], t[1], torch.zeros(3, 2, 4, 4, device="cuda"), *t[3:])
    # the outputs carry no gradient, whatever the inputs ask for
    cur = t[0].clone().requires_grad_(True)
    assert not any(o.requires_grad for o in ops.cost_volume(cur, *t[1:]))
