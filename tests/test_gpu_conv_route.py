"""The route is what gets launched: ops.conv3x3 forward and backward at the smallest shapes that still reach each kernel of the
3x3 convolution family, with the launches read back from the profile.  The kernels ops._conv3x3_route (forward, backward-data)
and ops._wrw_route (weight gradient) name are the ones that ran, and no others of the family.  No numbers are compared here:
tests/test_gpu_conv_anchor.py and tests/test_gpu_stem_head_anchor.py hold every one of these kernels to float64."""
import pytest
import torch

from depthmodelhardening_amd import ops

pytestmark = pytest.mark.gpu

_CONV = {"k10": "wino_conv3x3", "k17": "wino32_conv3x3", "k11": "conv3x3_small"}      # K13: by direction, below
_WRW = {"k13": "conv3x3_head_wrw", "k16": "conv3x3_small_wrw", "k18": "wino_wrw"}
_FAMILY = set(_CONV.values()) | set(_WRW.values()) | {"conv3x3_head", "conv3x3_head_bwd"}


@pytest.mark.parametrize("B,Cc,K,H,W,pad,fwd,bwd,wrw", [
    (4, 64, 64, 64, 128, 1, "k10", "k10", "k18"),           # (K18 from batch 4 on: 1024 chunk blocks)
    (4, 96, 32, 104, 512, 1, "k17", "k17", "k18"),          # K18 in its 32 x 96 form
    (2, 16, 1, 34, 66, 0, "k13", "k13", "k13"),
    (2, 16, 16, 32, 64, 1, "k11", "k11", "k16"),
    (2, 48, 48, 16, 32, 1, None, None, None),               # the library's
])
def test_conv3x3_launches_the_routed_kernels(B, Cc, K, H, W, pad, fwd, bwd, wrw):
    g = torch.Generator().manual_seed(B + Cc + K)
    x = (torch.rand(B, Cc, H, W, generator=g) - 0.5).cuda().requires_grad_(True)
    w = ((torch.rand(K, Cc, 3, 3, generator=g) - 0.5) * 0.1).cuda().requires_grad_(True)
    b = (torch.rand(K, generator=g) - 0.5).cuda().requires_grad_(True)
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    assert ops._conv3x3_route(B, Cc, K, H, W, pad, False) == fwd
    assert ops._conv3x3_route(B, K, Cc, Ho, Wo, 2 - pad, True) == bwd
    ops.enable_profile(True)
    try:
        y = ops.conv3x3(x, w, b, pad)
        assert ops._wrw_route(x, y, K, Cc) == wrw           # (the output gradient has the output's shape)
        y.backward(torch.ones_like(y))
        ran = {name: n[0] for name, n in ops.profile_bytes().items() if name in _FAMILY}
    finally:
        ops.enable_profile(False)
    assert tuple(y.shape) == (B, K, Ho, Wo) and x.grad is not None and w.grad is not None and b.grad is not None
    want = {}
    for name in (("conv3x3_head" if fwd == "k13" else _CONV.get(fwd)), ("conv3x3_head_bwd" if bwd == "k13" else _CONV.get(bwd)),
                 _WRW.get(wrw)):
        if name is not None:
            want[name] = want.get(name, 0) + 1
    assert ran == want
