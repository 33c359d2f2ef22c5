"""ops.pil_resize_host / ops.pil_axis_table (the numpy restatement of Pillow's 8-bit separable resample that K31 is held to, and
the path ``ops.pil_resize`` takes for CPU tensors) against Pillow itself where it is installed and against what Pillow wrote into
tests/golden/kitti_loader.npz (tools/make_goldens_kitti.py).  Every comparison is array_equal: the arithmetic is 8-bit fixed
point, there is no tolerance to give."""
import numpy as np
import pytest
import torch

from depthmodelhardening_amd import ops
from tests import kitti_ref as R


@pytest.fixture(scope="module")
def g(golden):
    return golden("kitti_loader")


def planar(img):
    return np.ascontiguousarray(img.transpose(2, 0, 1))


def hwc(img):
    return img.transpose(1, 2, 0)


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=[c[0] for c in R.RESIZE_CASES])
def test_restatement_equals_the_fixture(g, case):
    name, hw, out = case
    for kind in R.KINDS:
        img = R.case_image(name, hw, kind)
        for f in R.FILTERS:
            got = hwc(ops.pil_resize_host(planar(img), out, f))
            assert np.array_equal(got, g["resize_%s_%s_%s" % (name, kind, f)]), (name, kind, f)


@pytest.mark.parametrize("case", R.RESIZE_CASES + [("kitti_up", (370, 1224), (375, 1242)), ("kitti_train", (375, 1242), (320, 1024))],
                         ids=[c[0] for c in R.RESIZE_CASES] + ["kitti_up", "kitti_train"])
def test_restatement_equals_live_pillow(case):
    Image = pytest.importorskip("PIL.Image")
    number = {"lanczos": Image.LANCZOS, "bilinear": Image.BILINEAR}
    name, hw, (oh, ow) = case
    for kind in R.KINDS:
        img = R.case_image(name, hw, kind)
        for f in R.FILTERS:
            want = np.asarray(Image.fromarray(img).resize((ow, oh), number[f]))
            assert np.array_equal(hwc(ops.pil_resize_host(planar(img), (oh, ow), f)), want), (name, kind, f)
        gray = np.ascontiguousarray(img[..., 0])
        assert np.array_equal(ops.pil_resize_host(gray, (oh, ow)), np.asarray(Image.fromarray(gray, "L").resize((ow, oh), Image.LANCZOS)))


def test_both_clips_fire_on_the_noise_image():
    """On the 0 / 255 image the sums before the shift leave [0, 255] on both sides, so the clip is what the comparison holds."""
    sums = []
    ops.pil_resize_host(planar(R.case_image("odd_train", (37, 123), "noise")), (32, 96), "lanczos", sums=sums)
    assert len(sums) == 2       # the horizontal pass, then the vertical
    for acc in sums:
        v = acc >> ops.PIL_PRECISION_BITS
        assert v.min() < 0 and v.max() > 255, (v.min(), v.max())


def test_skipped_pass_and_the_identity():
    img = planar(R.case_image("rows_only", (37, 123), "rand"))
    sums = []
    ops.pil_resize_host(img, (32, 123), sums=sums)
    assert len(sums) == 1
    assert np.array_equal(ops.pil_resize_host(img, (37, 123)), img)
    xmin, count, k = ops.pil_axis_table(9, 9)
    assert xmin.tolist() == list(range(9)) and count.tolist() == [1] * 9 and k.tolist() == [[1 << 22]] * 9


def test_table_geometry():
    """The window of Pillow's precompute_coeffs: cut at both borders, ksize = 2 ceil(support) + 1, taps summing to about 2^22."""
    xmin, count, k = ops.pil_axis_table(123, 96, "lanczos")
    assert k.shape == (96, 2 * int(np.ceil(3.0 * 123 / 96)) + 1)
    assert xmin[0] == 0 and xmin[-1] + count[-1] == 123 and count[0] < count[48] and count[-1] < count[48]
    assert np.all(np.abs(k.sum(1) - (1 << 22)) <= k.shape[1])
    assert (k < 0).any()                    # LANCZOS has negative lobes
    xmin, count, k = ops.pil_axis_table(370, 375, "lanczos")     # up-scaling: filterscale clamps to 1
    assert k.shape[1] == 7
    xmin, count, k = ops.pil_axis_table(7, 13, "bilinear")
    assert k.shape[1] == 3 and (k >= 0).all()
    with pytest.raises(RuntimeError):
        ops.pil_axis_table(0, 4)
    with pytest.raises(RuntimeError):
        ops.pil_axis_table(8, 4, "bicubic")


def test_the_four_level_chain(g):
    for kind in R.KINDS:
        src = torch.from_numpy(R.case_image("odd_train", (37, 123), kind))[None]
        levels = ops.pil_pyramid(src, R.CHAIN_SIZE[0], R.CHAIN_SIZE[1], 4)
        assert len(levels) == 4
        for s, lvl in enumerate(levels):
            want = g["chain_%s_%d" % (kind, s)]
            assert np.array_equal(hwc(lvl.u8[0].numpy()), want), (kind, s)
            assert torch.equal(lvl.f32[0], torch.from_numpy(want).permute(2, 0, 1).float().div(255))


def test_flip_is_transpose_then_resize(g):
    Image = pytest.importorskip("PIL.Image")
    for kind in R.KINDS:
        img = R.case_image("odd_train", (37, 123), kind)
        got = hwc(ops.pil_resize_host(planar(img), R.CHAIN_SIZE, flip=True))
        assert np.array_equal(got, g["flip_%s" % kind])
        want = np.asarray(Image.fromarray(img).transpose(Image.FLIP_LEFT_RIGHT).resize(R.CHAIN_SIZE[::-1], Image.LANCZOS))
        assert np.array_equal(got, want)
        # (the result is not flipped instead: the rounded taps are not guaranteed to be mirror-symmetric)
    batch = torch.from_numpy(np.stack([R.case_image("odd_train", (37, 123), k) for k in R.KINDS]))
    out = ops.pil_resize(batch, R.CHAIN_SIZE, flip=[True, False])
    assert np.array_equal(hwc(out.u8[0].numpy()), g["flip_rand"]) and np.array_equal(hwc(out.u8[1].numpy()), g["chain_noise_0"])


def test_float_sources_truncate_as_topilimage_does():
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 37, 123, generator=gen)
    x[0, 0, 0, :4] = torch.tensor([0.0, 1.0, 254.5 / 255, 1.0 / 255])
    q = x.mul(255).byte()                                   # torchvision's ToPILImage on a float tensor
    assert np.array_equal(ops.pil_quantize_host(x.numpy()), q.numpy())
    got = ops.pil_resize(x, (32, 96))
    want = ops.pil_resize(q, (32, 96), layout="chw")
    assert torch.equal(got.u8, want.u8) and torch.equal(got.f32, want.f32)
    # a decoded byte survives to_tensor -> ToPILImage: the pixels of a pasted frame outside the object are the file's
    back = (torch.arange(256, dtype=torch.float32) / 255).mul(255).byte()
    assert torch.equal(back, torch.arange(256, dtype=torch.uint8))


def test_division_by_255_is_torchs():
    ramp = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16)
    out = ops.pil_resize(ramp, (16, 16), layout="chw")
    assert torch.equal(out.u8, ramp) and torch.equal(out.f32, ramp.float().div(255))


def test_mixed_source_sizes_in_one_batch(g):
    buf = np.zeros((2, 38, 124, 3), dtype=np.uint8)
    buf[0, :37, :123] = R.case_image("odd_train", (37, 123), "rand")
    buf[1] = R.case_image("even_train", (38, 124), "rand")
    out = ops.pil_resize(torch.from_numpy(buf), (32, 96), sizes=[(37, 123), (38, 124)])
    assert np.array_equal(hwc(out.u8[0].numpy()), g["resize_odd_train_rand_lanczos"])
    assert np.array_equal(hwc(out.u8[1].numpy()), g["resize_even_train_rand_lanczos"])
    with pytest.raises(RuntimeError):
        ops.pil_resize(torch.from_numpy(buf), (32, 96), sizes=[(39, 123), (38, 124)])
    with pytest.raises(RuntimeError):
        ops.pil_resize(torch.from_numpy(buf).double(), (32, 96))


def test_registration():
    from depthmodelhardening_amd import _native as N, build, library
    assert {"dmh_pil_resample", "dmh_pil_resample_tables_size"} <= set(N.EXPORTS) and "pil_resample.hip" in build.SOURCES
    assert "pil_resample" in library.OPS and hasattr(torch.ops.dmh, "pil_resample")
    lib = N.lib()
    for n_in, n_out, f in ((123, 96, "lanczos"), (370, 375, "lanczos"), (7, 13, "bilinear"), (96, 96, "lanczos"), (1242, 1024, "lanczos")):
        xmin, count, k = ops.pil_axis_table(n_in, n_out, f)
        assert lib.dmh_pil_resample_tables_size(n_in, n_out, ops.PIL_FILTERS[f][0]) == xmin.size + count.size + k.size
    assert lib.dmh_pil_resample_tables_size(0, 4, 1) == -1 and lib.dmh_pil_resample_tables_size(8, 4, 3) == -1
