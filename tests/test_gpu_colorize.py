"""K37 (ops.disp_colorize) on the GPU against its numpy twin (which tests/test_colorize_ref.py holds to numpy and matplotlib),
``python -m depthmodelhardening_amd.test_simple`` end to end, and the figure of ``evaluate_attacks``.

Exact where the arithmetic is exact: the bytes of the plain and |a - b| forms, the percentile, the bytes of the resize form given
the map the kernel returned.  The resize itself is held to float64 within a bound, because F.interpolate(bilinear,
align_corners=False) is not bit-reproducible between torch's own back ends.

The resize bound.  max |torch float32 CPU F.interpolate - float64 F.interpolate| on [0, 1) data, measured at the four shape pairs
(the largest of five seeds):
    (6, 20) -> (12, 39)          1.19e-6
    (5, 7) -> (3, 4)             1.42e-7
    (8, 8) -> (8, 8)             0 (the kernel must return the input bits)
    (192, 640) -> (375, 1242)    5.21e-5   (the float32 source coordinate near x = 1242 is 4e-5 off; the data's slope is ~1 per pixel)
The kernel may be 4 x that far from float64: its float32 scale and product order differ from the CPU kernel's while rounding the
same quantities."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import colorize_ref as R  # noqa: E402
from tests.util import no_miopen  # noqa: E402

DEV = torch.device("cuda")
RESIZE_CASES = [((6, 20), (12, 39), 1.19e-6), ((5, 7), (3, 4), 1.42e-7), ((8, 8), (8, 8), 0.0), ((192, 640), (375, 1242), 5.21e-5)]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("diff", [False, True], ids=["plain", "diff"])
@pytest.mark.parametrize("name", R.CASES)
def test_bytes_and_percentile_equal_the_twin(name, diff):
    """B = 3, different contents per image, every limit mode: zero differing bytes; the percentile is np.percentile's."""
    from depthmodelhardening_amd import ops
    maps = torch.from_numpy(R.case_maps(name))
    src = R.panel_sources(maps.numpy(), diff)
    for mode in R.MODES:
        panels = R.panels(mode, diff)
        want = ops.disp_colorize_host(maps, panels)
        got = ops.disp_colorize(maps.to(DEV), panels, return_map=True)
        assert got.rgb.shape == want.rgb.shape and got.rgb.dtype == torch.uint8
        nbad = int((got.rgb.cpu() != want.rgb).sum())
        assert nbad == 0, "%s %s: %d differing bytes" % (name, mode, nbad)
        stats = got.stats.cpu().numpy()
        p95 = np.array([np.percentile(s, 95) for s in src])
        print(name, mode, "percentile", stats[:, 4], p95)
        assert np.array_equal(stats[:, 4], p95)
        assert np.array_equal(stats, want.stats.numpy())
        assert _same_bits(got.map.cpu().numpy(), src)


@pytest.fixture(scope="module")
def resize_inputs():
    out = {}
    for (h, w), (H, W), _ in RESIZE_CASES:
        g = torch.Generator().manual_seed(h * 1000 + w)
        x = torch.rand(3, h, w, generator=g)
        out[(h, w)] = (x, F.interpolate(x[:, None].double(), (H, W), mode="bilinear", align_corners=False)[:, 0])
    return out


@pytest.mark.parametrize("hw,HW,measured", RESIZE_CASES)
def test_resize_form(resize_inputs, hw, HW, measured):
    """(a) the returned map within 4 x the CPU kernel's own distance from float64; (b) the bytes equal the twin applied to the
    returned map, zero differences; the percentile equals np.percentile of the returned map."""
    from depthmodelhardening_amd import ops
    x, ref64 = resize_inputs[hw]
    got = ops.disp_colorize(x.to(DEV), out_size=HW, return_map=True)
    fmap = got.map.cpu()
    assert fmap.shape == (3,) + HW
    err = float((fmap.double() - ref64).abs().max())
    print(hw, HW, "max |map - float64| = %.3e, bound %.3e" % (err, 4 * measured))
    assert err <= 4 * measured
    if hw == HW:
        assert _same_bits(fmap.numpy(), x.numpy())
    want = ops.disp_colorize_host(fmap)
    nbad = int((got.rgb.cpu() != want.rgb).sum())
    assert nbad == 0, "%d differing bytes" % nbad
    assert np.array_equal(got.stats.cpu().numpy()[:, 4], np.array([np.percentile(m, 95) for m in fmap.numpy()]))
    # per-panel forms through the resize: the difference of two maps under a shared limit
    panels = [(0, -1, "zero_ref", 0), (0, 1, "zero_ref", 0), (2, 1, "min_max", 0)]
    got = ops.disp_colorize(x.to(DEV), panels, out_size=HW, return_map=True)
    want = ops.disp_colorize_host(got.map.cpu(), [(0, -1, "zero_ref", 0), (1, -1, "zero_ref", 0), (2, -1, "min_max", 0)])
    assert int((got.rgb.cpu() != want.rgb).sum()) == 0


def test_mosaic_form():
    """Panels written with pitch and origin into one buffer (odd origins: the byte-store path and the 32-bit path): each panel's
    bytes equal the single-panel call's, bytes outside the panels are untouched."""
    from depthmodelhardening_amd import ops
    maps = torch.from_numpy(R.case_maps("37x53")).to(DEV)
    panels = R.panels("zero_ref") + [(0, 1, "min_max", 0)]
    single = ops.disp_colorize(maps, panels).rgb
    mosaic = torch.full((2 * 37 + 5, 2 * 53 + 7, 3), 77, dtype=torch.uint8, device=DEV)
    origins = [(0, 0), (1, 53 + 7), (37 + 5, 3), (37 + 4, 53 + 5)]
    out = ops.disp_colorize(maps, panels, out=mosaic, origins=origins)
    assert out.rgb is mosaic
    covered = torch.zeros(mosaic.shape[:2], dtype=torch.bool, device=DEV)
    for i, (y, x) in enumerate(origins):
        assert torch.equal(mosaic[y:y + 37, x:x + 53], single[i]), i
        covered[y:y + 37, x:x + 53] = True
    assert bool((mosaic[~covered] == 77).all())
    host = torch.full(mosaic.shape, 77, dtype=torch.uint8)
    ops.disp_colorize_host(maps.cpu(), panels, out=host, origins=origins)
    assert torch.equal(mosaic.cpu(), host)


def test_reproducible_and_graph_replay():
    from depthmodelhardening_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4, 48, 160, generator=g).to(DEV)
    panels = [(0, -1, "min_p95", 0), (1, 2, "zero_ref", 0), (3, -1, "min_max", 0)]
    a = ops.disp_colorize(x, panels, out_size=(93, 310), return_map=True)
    b = ops.disp_colorize(x, panels, out_size=(93, 310), return_map=True)
    assert torch.equal(a.rgb, b.rgb) and torch.equal(a.map.view(torch.int32), b.map.view(torch.int32)) and torch.equal(a.stats, b.stats)
    static = x.clone()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            c = ops.disp_colorize(static, panels, out_size=(93, 310), return_map=True)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c.rgb, a.rgb) and torch.equal(c.stats, a.stats)
    static.copy_(x.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    d = ops.disp_colorize(x.flip(0).contiguous(), panels, out_size=(93, 310))
    assert torch.equal(c.rgb, d.rgb) and not torch.equal(c.rgb, a.rgb)


def test_registered_operator_and_refusals():
    from depthmodelhardening_amd import library, ops  # noqa: F401
    x = torch.from_numpy(R.case_maps("signed")).to(DEV)
    rgb, fmap, stats = torch.ops.dmh.disp_colorize(x, [0, -1, 0, 0, 1, 2, 1, 0], 11, 23)
    want = ops.disp_colorize(x, [(0, -1, "min_p95", 0), (1, 2, "zero_ref", 0)], return_map=True)
    assert torch.equal(rgb, want.rgb) and torch.equal(stats, want.stats) and _same_bits(fmap.cpu().numpy(), want.map.cpu().numpy())
    with pytest.raises(RuntimeError, match="CUDA"):
        torch.ops.dmh.disp_colorize(x.cpu(), [0, -1, 0, 0], 11, 23)
    with pytest.raises(RuntimeError, match="on the maps' device"):
        ops.disp_colorize(x, out=torch.zeros(40, 80, 3, dtype=torch.uint8), origins=[(0, 0)] * 3)


@no_miopen
def test_test_simple_end_to_end(tmp_path):
    """Two PNGs of different sizes, a random-weight model fed 32 x 64: the .npy is disp_to_depth of the network's output on K31's
    resized input, the JPEG is PIL's encoding of the twin's bytes for the returned map, a *_disp.jpg in the folder is skipped."""
    import argparse
    from PIL import Image
    from depthmodelhardening_amd import ops, test_simple as TS
    from depthmodelhardening_amd.layers import disp_to_depth
    from oracle import synth
    rng = np.random.RandomState(7)
    sizes = {"a": (40, 64), "b": (75, 130)}
    for name, (h, w) in sizes.items():
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / (name + ".png"))
    Image.fromarray(rng.randint(0, 256, (20, 30, 3), dtype=np.uint8)).save(tmp_path / "c_disp.jpg")
    Image.fromarray(rng.randint(0, 256, (20, 30, 3), dtype=np.uint8)).save(tmp_path / "a_disp.jpg")
    model = synth.TinyDepthNet(seed=11).to(DEV).eval()
    args = argparse.Namespace(image_path=str(tmp_path), ext="png", pred_metric_depth=False, no_cuda=False, model_name=None,
                              load_weights_folder=None, feed_height=32, feed_width=64)
    results = TS.test_simple(args, model=model, return_maps=True)
    assert [os.path.basename(r["image"]) for r in results] == ["a.png", "b.png"]
    for r, (name, (h, w)) in zip(results, sorted(sizes.items())):
        with Image.open(tmp_path / (name + ".png")) as img:
            fed = np.asarray(img.convert("RGB").resize((64, 32), Image.LANCZOS), dtype=np.float32) / 255        # ToTensor
        with torch.no_grad():
            disp = model(torch.from_numpy(fed).permute(2, 0, 1)[None].to(DEV))
        npy = np.load(r["npy"])
        assert r["npy"] == str(tmp_path / (name + "_disp.npy")) and npy.shape == (1, 1, 32, 64) and npy.dtype == np.float32
        assert np.array_equal(npy, disp_to_depth(disp, 0.1, 100)[0].cpu().numpy())
        assert r["map"].shape == (h, w)
        ref64 = F.interpolate(disp.double().cpu(), (h, w), mode="bilinear", align_corners=False)[0, 0].numpy()
        # torch's float32 CPU resize is 1.11e-6 (40 x 64) and 2.35e-6 (75 x 130) from float64 at these shapes on [0, 1) data
        assert np.abs(r["map"] - ref64).max() <= 4 * (1.11e-6 if name == "a" else 2.35e-6)
        want = ops.disp_colorize_host(torch.from_numpy(r["map"])[None]).rgb[0].numpy()
        Image.fromarray(want).save(tmp_path / "want.jpeg")
        with open(tmp_path / "want.jpeg", "rb") as f1, open(r["jpeg"], "rb") as f2:
            assert f1.read() == f2.read()
        assert r["jpeg"] == str(tmp_path / (name + "_disp.jpeg"))
    assert not os.path.exists(tmp_path / "c_disp_disp.jpeg") and not os.path.exists(tmp_path / "a_disp_disp.npy")
    # a single file, metric depth; a jpg folder whose only files are disparity images
    args.image_path, args.pred_metric_depth = str(tmp_path / "b.png"), True
    (r,) = TS.test_simple(args, model=model)
    assert r["npy"].endswith("b_depth.npy") and np.load(r["npy"]).shape == (1, 1, 32, 64)
    assert np.allclose(np.load(r["npy"]), 5.4 / np.load(tmp_path / "b_disp.npy"), rtol=1e-6)      # 5.4 x 1 / the scaled disparity
    args.image_path, args.ext = str(tmp_path), "jpg"
    assert TS.test_simple(args, model=model) == []
    args.no_cuda = True
    with pytest.raises(RuntimeError, match="no CPU path"):
        TS.test_simple(args, model=model)


@no_miopen
def test_evaluate_attacks_figure(tmp_path, monkeypatch):
    """figure_path: the first scene of the first batch as the three-row figure; its colour panels are the twin's bytes for the
    disparities the evaluation computed.  Without figure_path the metrics are those of the same call with it."""
    from PIL import Image
    from depthmodelhardening_amd import evaluate_depth as E, my_utils as U, ops
    from tests import light_ref
    model = light_ref.make_model().to(DEV).eval()
    args = {"norm_type": "l_inf", "epsilon": 0.1, "alpha": 0.1, "step": 1, "batch_size": 2}
    seen = []
    errors = ops.masked_depth_errors

    def spy(disp_gt, disp_atk, *a, **k):
        seen.append((disp_gt.detach().clone(), disp_atk.detach().clone()))
        return errors(disp_gt, disp_atk, *a, **k)
    monkeypatch.setattr(E.ops, "masked_depth_errors", spy)
    path = tmp_path / "atk.png"
    light_ref.seed_all(3)
    with_figure = E.evaluate_attacks(model, args, eval_count=1, figure_path=str(path))
    light_ref.seed_all(3)
    without = E.evaluate_attacks(model, args, eval_count=1)
    assert np.array_equal(with_figure, without) and np.isfinite(without).all() and len(seen) == 2
    disp_gt, disp_atk = seen[0]
    fig = np.array(Image.open(path))
    h, w = disp_gt.shape[2:]
    height, width, img_at, colour_at = U.figure_layout((h, w), (h, w), jcl=True)
    assert fig.shape == (height, width, 3)
    a, b = disp_atk[0, 0].cpu().numpy(), disp_gt[0, 0].cpu().numpy()
    vmax = np.percentile(a, 95)
    (y, x), (y2, x2) = colour_at
    assert np.array_equal(fig[y:y + h, x:x + w], ops.colorize_bytes_host(a, 0, vmax))
    assert np.array_equal(fig[y2:y2 + h, x2:x2 + w], ops.colorize_bytes_host(np.abs(a - b), 0, vmax))
    assert (a != b).any() and fig[img_at[0][0]:img_at[0][0] + h, img_at[0][1]:img_at[0][1] + w].std() > 0


def test_test_simple_command_line_with_a_weights_folder(tmp_path):
    """The command as a user runs it: --load_weights_folder with encoder.pth (its height / width set the feed size) and
    depth.pth, random weights, one KITTI-sized PNG.  The .npy is disp_to_depth of the loaded network on K31's input."""
    from PIL import Image
    from depthmodelhardening_amd import networks, ops, test_simple as TS
    from depthmodelhardening_amd.layers import disp_to_depth
    torch.manual_seed(37)
    encoder = networks.ResnetEncoder(18, False)
    decoder = networks.DepthDecoder(num_ch_enc=encoder.num_ch_enc, scales=range(4))
    weights = tmp_path / "weights"
    weights.mkdir()
    torch.save(dict(encoder.state_dict(), height=320, width=1024, use_stereo=True), weights / "encoder.pth")
    torch.save(decoder.state_dict(), weights / "depth.pth")
    frames = tmp_path / "frames"
    frames.mkdir()
    rgb = np.random.RandomState(3).randint(0, 256, (375, 1242, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(frames / "f.png")
    args = TS.parse_args(["--image_path", str(frames), "--ext", "png", "--load_weights_folder", str(weights)])
    (r,) = TS.test_simple(args, return_maps=True)
    model, fh, fw = TS.load_model(str(weights), DEV)
    assert (fh, fw) == (320, 1024)
    fed = ops.pil_resize(torch.from_numpy(rgb)[None].to(DEV), (320, 1024), "lanczos", want_u8=False).f32
    with torch.no_grad():
        disp = model(fed)
    npy = np.load(r["npy"])
    assert npy.shape == (1, 1, 320, 1024) and np.array_equal(npy, disp_to_depth(disp, 0.1, 100)[0].cpu().numpy())
    with Image.open(r["jpeg"]) as im:
        assert im.size == (1242, 375) and im.mode == "RGB"
    want = ops.disp_colorize_host(torch.from_numpy(r["map"])[None]).rgb[0].numpy()
    Image.fromarray(want).save(tmp_path / "want.jpeg")
    with open(tmp_path / "want.jpeg", "rb") as f1, open(r["jpeg"], "rb") as f2:
        assert f1.read() == f2.read()
