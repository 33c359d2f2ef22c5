"""K31 (csrc/pil_resample.hip) against what Pillow wrote into tests/golden/kitti_loader.npz and against the numpy restatement
(tests/test_pil_resample_ref.py holds that to Pillow itself): torch.equal on the uint8 result and on the float one, no tolerance.
The shapes are the smallest at which the kernel takes every path: odd / even sources whose tap windows are cut at both borders,
half size, a larger size, one axis unchanged, 5 x 7 -> 9 x 13, more than one tile of 8 output rows, a batch that mixes two source
sizes and flips, both input modes, the chain, cached tables, a captured graph."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from depthmodelhardening_amd import ops  # noqa: E402
from tests import kitti_ref as R  # noqa: E402

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def g(golden):
    return golden("kitti_loader")


def chw(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=[c[0] for c in R.RESIZE_CASES])
def test_kernel_equals_pillow_and_the_restatement(g, case):
    name, hw, out = case
    src = torch.from_numpy(np.stack([R.case_image(name, hw, kind) for kind in R.KINDS]))
    for f in R.FILTERS:
        got = ops.pil_resize(src.to(DEV), out, f)
        host = ops.pil_resize(src, out, f)
        assert got.u8.dtype == torch.uint8 and got.f32.dtype == torch.float32
        assert torch.equal(got.u8.cpu(), host.u8) and torch.equal(got.f32.cpu(), host.f32), (name, f)
        for i, kind in enumerate(R.KINDS):
            want = chw(g["resize_%s_%s_%s" % (name, kind, f)])
            assert torch.equal(got.u8[i].cpu(), want), (name, kind, f)
            assert torch.equal(got.f32[i].cpu(), want.float().div(255)), (name, kind, f)


def test_mixed_sizes_and_flips_in_one_batch(g):
    buf = np.zeros((4, 38, 124, 3), dtype=np.uint8)
    sizes = [(37, 123), (38, 124), (37, 123), (38, 124)]
    names = ["odd_train", "even_train", "odd_train", "even_train"]
    for i, (nm, (h, w)) in enumerate(zip(names, sizes)):
        buf[i, :h, :w] = R.case_image(nm, (h, w), "rand")
    flips = [1, 0, 0, 1]
    src = torch.from_numpy(buf)
    got = ops.pil_resize(src.to(DEV), (32, 96), flip=torch.tensor(flips, dtype=torch.int32, device=DEV), sizes=sizes)
    host = ops.pil_resize(src, (32, 96), flip=flips, sizes=sizes)
    assert torch.equal(got.u8.cpu(), host.u8) and torch.equal(got.f32.cpu(), host.f32)
    assert torch.equal(got.u8[0].cpu(), chw(g["flip_rand"]))                             # transpose(FLIP_LEFT_RIGHT), then resize
    assert torch.equal(got.u8[1].cpu(), chw(g["resize_even_train_rand_lanczos"]))
    assert torch.equal(got.u8[2].cpu(), chw(g["resize_odd_train_rand_lanczos"]))


def test_float_sources_and_planar_sources():
    gen = torch.Generator().manual_seed(11)
    x = torch.rand(2, 3, 37, 123, generator=gen)
    x[0, 0, 0, :4] = torch.tensor([0.0, 1.0, 254.5 / 255, 1.0 / 255])
    got = ops.pil_resize(x.to(DEV), (32, 96), flip=[0, 1])
    host = ops.pil_resize(x, (32, 96), flip=[0, 1])
    assert torch.equal(got.u8.cpu(), host.u8) and torch.equal(got.f32.cpu(), host.f32)
    q = x.mul(255).byte()                                   # ToPILImage's truncation, then the uint8 planar mode
    planar = ops.pil_resize(q.to(DEV), (32, 96), flip=[0, 1], layout="chw")
    assert torch.equal(planar.u8, got.u8) and torch.equal(planar.f32, got.f32)
    mask = torch.rand(3, 1, 37, 123, generator=gen)         # one channel, as the object mask goes through
    one = ops.pil_resize(mask.to(DEV), (32, 96), want_u8=False)
    assert one.u8 is None and torch.equal(one.f32.cpu(), ops.pil_resize(mask, (32, 96)).f32)
    only_u8 = ops.pil_resize(mask.to(DEV), (32, 96), want_float=False)
    assert only_u8.f32 is None and torch.equal(only_u8.u8.cpu(), ops.pil_resize(mask, (32, 96)).u8)


def test_the_training_shape():
    """One 375 x 1242 frame -> 320 x 1024 -> 160 x 512: 1024 columns are four trips of a workgroup's 256 threads through the
    horizontal loop and 32 through the vertical one, and the LDS tile is 17 and 28 rows of 1024 bytes."""
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, size=(1, 375, 1242, 3)).astype(np.uint8)
    img[0, 100:200] = (rng.randint(0, 2, size=(100, 1242, 3)) * 255).astype(np.uint8)      # a band that drives the clips
    src = torch.from_numpy(img)
    got = ops.pil_pyramid(src.to(DEV), 320, 1024, 2, flip=[1])
    host = ops.pil_pyramid(src, 320, 1024, 2, flip=[1])
    for a, b in zip(got, host):
        assert torch.equal(a.u8.cpu(), b.u8) and torch.equal(a.f32.cpu(), b.f32)


def test_many_batch_shapes_share_the_tables():
    """A shuffled list mixes the frame sizes anew in every batch: the tables are kept once per (in, out, filter) -- the arena
    stops growing after the first batch -- and the per-batch descriptor sets are a bounded cache."""
    rng = np.random.RandomState(9)
    kinds = [(37, 123), (38, 124), (36, 120)]
    buf = torch.from_numpy(rng.randint(0, 256, size=(6, 38, 124, 3)).astype(np.uint8))
    dev_buf = buf.to(DEV)
    ops.pil_resize(dev_buf, (32, 96), sizes=[kinds[i % 3] for i in range(6)])
    arena = ops._pil_arenas[str(dev_buf.device)]
    words, tables = sum(w.size for w in arena.words), arena.tables
    seen = set()
    for trial in range(ops.PIL_DESC_CACHE + 40):
        sizes = tuple(kinds[int(v)] for v in rng.randint(0, 3, size=6))
        seen.add(sizes)
        got = ops.pil_resize(dev_buf, (32, 96), sizes=sizes)
        if trial % 25 == 0:
            assert torch.equal(got.u8.cpu(), ops.pil_resize(buf, (32, 96), sizes=sizes).u8), sizes
    assert len(seen) > ops.PIL_DESC_CACHE, "the trial must bring more batch shapes than the cache keeps"
    assert sum(w.size for w in arena.words) == words and arena.tables is tables       # no table was made or uploaded again
    assert len(ops._pil_device_cache) <= ops.PIL_DESC_CACHE + len(ops._pil_graph_keys)


def test_every_byte_divides_as_torch_divides():
    ramp = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16)
    out = ops.pil_resize(ramp.to(DEV), (16, 16), layout="chw")
    assert torch.equal(out.u8.cpu(), ramp) and torch.equal(out.f32.cpu(), ramp.float().div(255))


def test_the_chain_cached_tables_and_a_graph(g):
    src = torch.from_numpy(np.stack([R.case_image("odd_train", (37, 123), kind) for kind in R.KINDS])).to(DEV)
    first = ops.pil_pyramid(src, 32, 96, 4)
    for i, kind in enumerate(R.KINDS):
        for s in range(4):
            want = chw(g["chain_%s_%d" % (kind, s)])
            assert torch.equal(first[s].u8[i].cpu(), want) and torch.equal(first[s].f32[i].cpu(), want.float().div(255)), (kind, s)
    cached = len(ops._pil_device_cache)
    second = ops.pil_pyramid(src, 32, 96, 4)                # the tables are on the device already
    assert len(ops._pil_device_cache) == cached
    for a, b in zip(first, second):
        assert torch.equal(a.u8, b.u8) and torch.equal(a.f32, b.f32)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):        # four launches in a row: no parallel branches
            held = ops.pil_pyramid(src, 32, 96, 4)
    for lvl in held:
        lvl.u8.zero_()
        lvl.f32.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, held):
        assert torch.equal(a.u8, b.u8) and torch.equal(a.f32, b.f32)


def test_the_operator_and_its_argument_checks():
    from depthmodelhardening_amd import library  # noqa: F401
    src = torch.from_numpy(R.case_image("odd_train", (37, 123), "rand"))[None].to(DEV)
    want = ops.pil_resize(src, (32, 96))
    u8, f32 = torch.ops.dmh.pil_resample(src, 32, 96, "lanczos", None, [37, 123], True)
    assert torch.equal(u8, want.u8) and torch.equal(f32, want.f32)
    torch.library.opcheck(torch.ops.dmh.pil_resample, (src, 32, 96, "lanczos", None, [37, 123], True),
                          test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(RuntimeError):
        ops.pil_resize(src, (0, 96))
    with pytest.raises(RuntimeError):
        ops.pil_resize(src, (32, 96), "bicubic")
    with pytest.raises(RuntimeError):
        ops.pil_resize(src, (32, 96), flip=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.pil_resize(src.float(), (32, 96), layout="hwc")
    with pytest.raises(RuntimeError):
        ops.pil_resize(src, (32, 96), want_float=False, want_u8=False)
    with pytest.raises(RuntimeError, match="LDS"):          # 3000 -> 8 rows: a tile would need ~4800 source rows of 1024 bytes
        ops.pil_resize(torch.zeros(1, 1, 3000, 8, dtype=torch.uint8, device=DEV), (8, 1024), layout="chw")
