"""torch.ops.dmh.* (depthmodelhardening_amd/library.py): the registered operators give the bits of ops.py's autograd
Functions, pass torch.library.opcheck (schema, fake tensors, autograd registration), trace under fake tensors, and back the
stand-alone layers surface (MD2/layers.py SSIM / get_smooth_loss) with kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _lib():
    from depthmodelhardening_amd import _native as N, library, ops  # noqa: F401
    return N, ops, library


def _paste_case(dev, n=3):
    from depthmodelhardening_amd.my_utils import ori_H, ori_W
    from depthmodelhardening_amd.physicalTrans import PhysicalTrans
    from oracle import synth
    obj, pmask = synth.make_object()
    pt = PhysicalTrans(obj, pmask, None, (1, 3, ori_H, ori_W), dist_range=list(np.arange(5, 10, 0.2)))
    coeffs = torch.from_numpy(pt.coeffs_for([5.0, 7.2, 9.8][:n], [0, 15, -30][:n])).to(dev)
    scenes = synth.kitti_like(n, 3, 375, 1242, torch.Generator().manual_seed(3)).to(dev)
    return scenes, obj.to(dev), pmask.to(dev), coeffs, pt.l_pad, pt.t_pad


def test_registered_attack_ops_equal_the_autograd_functions():
    N, ops, library = _lib()
    dev = torch.device("cuda")
    scenes, obj, pmask, coeffs, l_pad, t_pad = _paste_case(dev)
    res = []
    for use_lib in (False, True):
        patch = obj.clone().requires_grad_(True)
        if use_lib:
            adv, m = torch.ops.dmh.eot_paste(scenes, patch, pmask, coeffs, l_pad, t_pad, 320, 1024, None)
            cost = torch.ops.dmh.masked_sq_mean(adv[:, :1] * 0.5, m)
        else:
            adv, m = ops.eot_paste(scenes, patch, pmask, coeffs, l_pad, t_pad, (320, 1024))
            cost = ops.masked_sq_mean(adv[:, :1] * 0.5, m)
        (g,) = torch.autograd.grad(cost, patch)
        step = (torch.ops.dmh.pgd_linf_step if use_lib else ops.pgd_linf_step)(patch.detach(), obj, g, 0.02, 0.1)
        res.append((adv.detach(), m, cost.detach(), g, step))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][3].abs().max()) > 0
    # L0 operators
    g0 = torch.Generator().manual_seed(5)
    pos = torch.rand(obj.shape, generator=g0).to(dev).requires_grad_(True)
    neg = torch.rand(obj.shape, generator=g0).to(dev).requires_grad_(True)
    a1, c1 = ops.l0_compose(obj, pos, neg, 1 / 255.0)
    a2, c2 = torch.ops.dmh.l0_compose(obj, pos, neg, 1 / 255.0, False)
    assert torch.equal(a1, a2) and torch.equal(c1, c2)
    m1, m2 = ops.l0_mask_cost(pos, neg), torch.ops.dmh.l0_mask_cost(pos, neg)
    g1 = torch.autograd.grad(a1.sum() + m1, [pos, neg])
    g2 = torch.autograd.grad(a2.sum() + m2, [pos, neg])
    assert torch.equal(m1, m2) and all(torch.equal(x, y) for x, y in zip(g1, g2))


def test_registered_fused_loss_equals_ops_and_traces_under_fake_tensors():
    N, ops, library = _lib()
    from oracle import synth
    from tests.util import to_dev
    B, H, W = 2, 64, 192
    inputs, disps = synth.make_loss_case(B, H, W, 5)
    d_in = to_dev(inputs)
    res = []
    for use_lib in (False, True):
        dd = [d.cuda().requires_grad_(True) for d in disps]
        args = (d_in[("color", 0, 0)], [d_in[("color", "s", 0)]], [d_in["stereo_T"]], d_in[("K", 0)], d_in[("inv_K", 0)], dd,
                [d_in[("color", 0, s)] for s in range(4)])
        if use_lib:
            fin, sel, _ = torch.ops.dmh.photo_smooth_loss(*args, 0.1, 100.0, N.VARIANT_MD2, True, False, 1e-3, N.NOISE_NONE, 0, 0)
            sel0 = ops.SelectionMaps(sel, 4)[0]
        else:
            out = ops.photometric_smooth_loss(*args, noise=None)
            fin, sel0 = out.fin, out.sel[0]
        fin[N.FIN_LOSS].backward()
        res.append((fin.detach(), sel0, [d.grad for d in dd]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert all(torch.equal(a, b) for a, b in zip(res[0][2], res[1][2]))
    # fake-tensor propagation: shapes and dtypes without touching the device
    from torch._subclasses.fake_tensor import FakeTensorMode
    mode = FakeTensorMode()
    fk = lambda t: mode.from_tensor(t)      # noqa: E731
    fargs = (fk(args[0]), [fk(t) for t in args[1]], [fk(t) for t in args[2]], fk(args[3]), fk(args[4]),
             [fk(d.detach()) for d in args[5]], [fk(t) for t in args[6]])
    with mode:
        f_fin, f_sel, f_st = torch.ops.dmh.photo_smooth_loss(*fargs, 0.1, 100.0, N.VARIANT_MD2, True, False, 1e-3,
                                                             N.NOISE_NONE, 0, 0)
        assert tuple(f_fin.shape) == (N.FIN_SIZE,) and tuple(f_sel.shape) == (B, H, W) and f_sel.dtype == torch.uint8
        assert tuple(f_st.shape) == (4, B, 2)


def test_opcheck_of_the_small_operators():
    """torch.library.opcheck: schema, fake implementation against the real one, autograd registration and the AOT dispatch path."""
    N, ops, library = _lib()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, 16, 24, generator=g).to(dev)
    y = torch.rand(2, 3, 16, 24, generator=g).to(dev)
    tests = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.dmh.ssim_map, (x.clone().requires_grad_(True), y.clone().requires_grad_(True)), test_utils=tests)
    d = torch.rand(2, 1, 16, 24, generator=g).to(dev)
    torch.library.opcheck(torch.ops.dmh.smooth_loss, (d.clone().requires_grad_(True), x), test_utils=tests)
    torch.library.opcheck(torch.ops.dmh.masked_sq_mean, (d.clone().requires_grad_(True), (d > 0.5).float()), test_utils=tests)
    torch.library.opcheck(torch.ops.dmh.pgd_linf_step, (x, y, x - y, 0.02, 0.1), test_utils=tests)
    # --gt_depth term (K6b): same bits as ops.gt_depth_mse, mask passed as the dataset passes it (one channel expanded to three)
    m3 = (torch.rand(2, 1, 16, 24, generator=g) > 0.6).float().to(dev).expand(-1, 3, -1, -1)
    od = torch.tensor([[6.2], [8.4]], device=dev)
    d2 = (d * 0.3 + 0.01)
    torch.library.opcheck(torch.ops.dmh.gt_depth_mse, (d2.clone().requires_grad_(True), (d2 * 0.9).contiguous(), m3, od, 0.1, 100.0),
                          test_utils=tests)
    a, b = d2.clone().requires_grad_(True), d2.clone().requires_grad_(True)
    la, lb = torch.ops.dmh.gt_depth_mse(a, (d2 * 0.9).contiguous(), m3, od, 0.1, 100.0), ops.gt_depth_mse(b, d2 * 0.9, m3, od, 0.1, 100.0)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    assert set(library.OPS) <= set(dir(torch.ops.dmh)) or all(hasattr(torch.ops.dmh, n) for n in library.OPS)


@pytest.mark.parametrize("shape", [(2, 3, 32, 96), (1, 3, 5, 7), (2, 1, 2, 2)])
def test_layers_ssim_goes_through_the_kernel_and_matches_the_formula(shape):
    """depthmodelhardening_amd.layers.SSIM on CUDA tensors = torch.ops.dmh.ssim_map: values and both input gradients against
    the reference's formula (MD2/layers.py:223-253) evaluated in float64 -- including 2-pixel-wide planes, where every
    window reads reflected pixels twice."""
    from depthmodelhardening_amd import layers
    g = torch.Generator().manual_seed(shape[2])
    x = torch.rand(shape, generator=g)
    y = (0.7 * x + 0.3 * torch.rand(shape, generator=g))
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    out = layers.SSIM()(xd, yd)
    w = torch.rand(shape, generator=g)
    (out * w.cuda()).sum().backward()
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    xp, yp = F.pad(x64, (1, 1, 1, 1), mode="reflect"), F.pad(y64, (1, 1, 1, 1), mode="reflect")
    mu_x, mu_y = F.avg_pool2d(xp, 3, 1), F.avg_pool2d(yp, 3, 1)
    sx, sy = F.avg_pool2d(xp ** 2, 3, 1) - mu_x ** 2, F.avg_pool2d(yp ** 2, 3, 1) - mu_y ** 2
    sxy = F.avg_pool2d(xp * yp, 3, 1) - mu_x * mu_y
    ref = torch.clamp((1 - (2 * mu_x * mu_y + 1e-4) * (2 * sxy + 9e-4) / ((mu_x ** 2 + mu_y ** 2 + 1e-4) * (sx + sy + 9e-4))) / 2, 0, 1)
    (ref * w.double()).sum().backward()
    assert float((out.detach().cpu().double() - ref.detach()).abs().max()) <= 5e-5      # sigma = E[x^2] - mu^2 cancels to ~1e-3
    for got, want in ((xd.grad, x64.grad), (yd.grad, y64.grad)):
        err = float((got.cpu().double() - want).norm() / want.norm())
        assert err <= 2e-3, err                                                         # the same cancellation, differentiated


@pytest.mark.parametrize("shape", [(2, 3, 32, 96), (1, 3, 2, 5)])
def test_layers_smooth_loss_goes_through_the_kernel(shape):
    from depthmodelhardening_amd import layers
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(W)
    disp, img = torch.rand(B, 1, H, W, generator=g), torch.rand(B, Cc, H, W, generator=g)
    dd = disp.cuda().requires_grad_(True)
    out = layers.get_smooth_loss(dd, img.cuda())
    out.backward()
    d64, i64 = disp.double().requires_grad_(True), img.double()
    gdx, gdy = (d64[:, :, :, :-1] - d64[:, :, :, 1:]).abs(), (d64[:, :, :-1, :] - d64[:, :, 1:, :]).abs()
    gix = (i64[:, :, :, :-1] - i64[:, :, :, 1:]).abs().mean(1, keepdim=True)
    giy = (i64[:, :, :-1, :] - i64[:, :, 1:, :]).abs().mean(1, keepdim=True)
    ref = (gdx * torch.exp(-gix)).mean() + (gdy * torch.exp(-giy)).mean()
    ref.backward()
    assert abs(float(out) - float(ref)) <= 2e-6 * abs(float(ref))
    assert float((dd.grad.cpu().double() - d64.grad).abs().max()) <= 1e-5 * float(d64.grad.abs().max())


# ---- both surfaces run the launchers of ops.py: what is left to hold is the plumbing around them -- argument order, saved tensors
# and gradient slots of the autograd.Function and custom_op wrappers -- in the forms the tests above do not reach
@pytest.mark.parametrize("flip,broadcast", [(True, False), (False, True), (True, True)])
def test_paste_surfaces_agree_with_flip_and_a_broadcast_scene(flip, broadcast):
    N, ops, library = _lib()
    dev = torch.device("cuda")
    scenes, obj, pmask, coeffs, l_pad, t_pad = _paste_case(dev, 2)
    scenes = scenes[:1] if broadcast else scenes
    fl = torch.tensor([1, 0], dtype=torch.int32, device=dev) if flip else None
    w = torch.rand(2, 3, 40, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    res = []
    for use_lib in (False, True):
        patch = obj.clone().requires_grad_(True)
        if use_lib:
            adv, m = torch.ops.dmh.eot_paste(scenes, patch, pmask, coeffs, l_pad, t_pad, 40, 128, fl)
        else:
            adv, m = ops.eot_paste(scenes, patch, pmask, coeffs, l_pad, t_pad, (40, 128), flip=fl)
        (g,) = torch.autograd.grad((adv * w).sum(), patch)
        res.append((adv.detach(), m, g))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    assert float(res[0][2].abs().max()) > 0 and float(res[0][1].max()) > 0
    if flip:        # the flag reaches the kernel on both surfaces: sample 0 differs from its un-flipped paste, sample 1 does not
        plain, _ = ops.eot_paste(scenes, obj, pmask, coeffs, l_pad, t_pad, (40, 128))
        assert not torch.equal(plain[0], res[0][0][0]) and torch.equal(plain[1], res[0][0][1])


def test_small_operator_surfaces_agree_without_a_mask_and_with_finalize():
    N, ops, library = _lib()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(6)
    d = torch.rand(2, 1, 16, 24, generator=g).to(dev)
    res = []
    for fn in (ops.masked_sq_mean, torch.ops.dmh.masked_sq_mean):
        x = d.clone().requires_grad_(True)
        cost = fn(x, None)
        (gx,) = torch.autograd.grad(cost * 3.0, x)
        res.append((cost.detach(), gx))
    assert all(torch.equal(a, b) for a, b in zip(*res)) and float(res[0][1].abs().max()) > 0
    obj = torch.rand(1, 3, 16, 24, generator=g).to(dev)
    pos0, neg0 = torch.rand(1, 3, 16, 24, generator=g).to(dev) * 1.5 - 0.25, torch.rand(1, 3, 16, 24, generator=g).to(dev) * 1.5 - 0.25
    w = torch.rand(1, 3, 16, 24, generator=g).to(dev)
    res = []
    for use_lib in (False, True):
        pos, neg = pos0.clone().requires_grad_(True), neg0.clone().requires_grad_(True)
        adv, count = torch.ops.dmh.l0_compose(obj, pos, neg, 0.3, True) if use_lib else ops.l0_compose(obj, pos, neg, 0.3, finalize=True)
        res.append((adv.detach(), count) + torch.autograd.grad((adv * w).sum(), [pos, neg]))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    plain, _ = ops.l0_compose(obj, pos0, neg0, 0.3, finalize=False)
    assert not torch.equal(plain, res[0][0])        # ``finalize`` reaches the kernel


@pytest.mark.parametrize("variant,philox", [("dh", False), ("md2", True), ("dh", True)])
def test_fused_loss_surfaces_agree_in_variant_dh_and_with_philox(variant, philox):
    N, ops, library = _lib()
    from oracle import synth
    from tests.util import to_dev
    B, H, W = 2, 64, 192
    inputs, disps = synth.make_loss_case(B, H, W, 5)
    d_in = to_dev(inputs)
    wfin = torch.rand(N.FIN_SIZE, generator=torch.Generator().manual_seed(8)).cuda()
    res = []
    for use_lib in (False, True):
        dd = [d.cuda().requires_grad_(True) for d in disps]
        args = (d_in[("color", 0, 0)], [d_in[("color", "s", 0)]], [d_in["stereo_T"]], d_in[("K", 0)], d_in[("inv_K", 0)], dd,
                [d_in[("color", 0, s)] for s in range(4)])
        torch.manual_seed(77)
        gen = torch.cuda.default_generators[torch.cuda.current_device()]
        gen.set_offset(40)
        seed, offset = gen.initial_seed() & 0xFFFFFFFFFFFFFFFF, gen.get_offset()       # what ops._philox hands the kernel
        if use_lib:
            fin, sel, _ = torch.ops.dmh.photo_smooth_loss(*args, 0.1, 100.0, N.VARIANT_DH if variant == "dh" else N.VARIANT_MD2, True,
                                                          False, 1e-3, N.NOISE_PHILOX if philox else N.NOISE_NONE, seed, offset)
        else:
            out = ops.photometric_smooth_loss(*args, variant=variant, noise="philox" if philox else None)
            fin, sel = out.fin, out.sel.packed
        res.append((fin.detach(), sel) + torch.autograd.grad((fin * wfin).sum(), dd))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    assert all(float(g.abs().max()) > 0 for g in res[0][2:])


# ---- the upload cache of the loader operators (ops._UploadCache): K32's descriptors and K34's index tables follow K31's rules
def _velo_case(i, dev):
    """One frame of (4 + i) x 6 cells with a dozen points in front of it: (points, offsets, proj, shapes)."""
    H, W = 4 + i, 6
    g = torch.Generator().manual_seed(100 + i)
    pts = torch.rand(12, 4, generator=g)
    pts[:, 2] += 1.0                                       # u = rint(W x / z + 1) - 1, v = rint(H y / z + 1) - 1: mostly inside
    proj = torch.tensor([[[W, 0, 1, 0], [0, H, 1, 0], [0, 0, 1, 0]]], dtype=torch.float64)
    return pts.to(dev), torch.tensor([0, 12], dtype=torch.int32).to(dev), proj.to(dev), ((H, W),)


def _hint_case(i):
    """(hints [2, 1, Hs, Ws] on the CPU, flip, out_size): a few pixels each, every i another (Hs, Ws) -> (H, W)."""
    hints = torch.rand(2, 1, 3 + i, 5, generator=torch.Generator().manual_seed(200 + i)) - 0.3
    return hints, [True, False], (4 + i, 7)


def test_upload_caches_stay_bounded_and_right_after_eviction():
    N, ops, library = _lib()
    dev, cpu = torch.device("cuda"), torch.device("cpu")
    for i in list(range(ops.VELO_DESC_CACHE + 3)) + [0]:         # the first key once more, after its eviction
        got, off = ops.velo_depth_map(*_velo_case(i, dev))
        want, want_off = ops.velo_depth_map(*_velo_case(i, cpu))
        assert torch.equal(got.cpu(), want) and off == want_off and float(want.max()) > 0, i
        assert len(ops._velo_desc_cache) <= ops.VELO_DESC_CACHE + len(ops._velo_desc_cache.held)
    for i in list(range(ops.HINT_TABLE_CACHE + 3)) + [0]:
        hints, flip, out_size = _hint_case(i)
        got, want = ops.depth_hint_prepare(hints.to(dev), flip, out_size), ops.depth_hint_prepare_host(hints, flip, out_size)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]) and float(want[1].sum()) > 0, i
        assert len(ops._hint_table_cache) <= ops.HINT_TABLE_CACHE + len(ops._hint_table_cache.held)


def test_a_second_stream_waits_for_the_first_upload():
    N, ops, library = _lib()
    dev = torch.device("cuda")
    side = torch.cuda.Stream()
    velo = _velo_case(40, dev)
    hints, flip, out_size = _hint_case(40)
    hints_d, flip_d = hints.to(dev), torch.tensor([1, 0], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()                                # the inputs are there: what is left to wait for is the tables' upload
    first_v = ops.velo_depth_map(*velo)[0]
    with torch.cuda.stream(side):
        second_v = ops.velo_depth_map(*velo)[0]
    first_h = ops.depth_hint_prepare(hints_d, flip_d, out_size)
    with torch.cuda.stream(side):
        second_h = ops.depth_hint_prepare(hints_d, flip_d, out_size)
    torch.cuda.synchronize()
    want_v = ops.velo_depth_map(*_velo_case(40, torch.device("cpu")))[0]
    want_h = ops.depth_hint_prepare_host(hints, flip, out_size)
    assert torch.equal(first_v.cpu(), want_v) and torch.equal(second_v.cpu(), want_v)
    for got in (first_h, second_h):
        assert torch.equal(got[0].cpu(), want_h[0]) and torch.equal(got[1].cpu(), want_h[1])


def test_tables_a_captured_graph_holds_are_not_evicted():
    N, ops, library = _lib()
    dev = torch.device("cuda")
    hints, _, out_size = _hint_case(60)
    hints_d = hints.to(dev)
    eager = ops.depth_hint_prepare(hints_d, None, out_size)             # warms the key
    key = (str(hints_d.device), hints.shape[2], hints.shape[3]) + out_size
    assert key in ops._hint_table_cache
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):                    # one launch: no parallel branches
            held = ops.depth_hint_prepare(hints_d, None, out_size)
    torch.cuda.current_stream().wait_stream(stream)
    for i in range(61, 61 + ops.HINT_TABLE_CACHE + 1):
        other, flip, size = _hint_case(i)
        ops.depth_hint_prepare(other.to(dev), flip, size)
    for t in held:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(held[0], eager[0]) and torch.equal(held[1], eager[1]) and float(eager[1].sum()) > 0
    assert key in ops._hint_table_cache and key in ops._hint_table_cache.held
