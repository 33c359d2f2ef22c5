"""K34 on the host: ops.depth_hint_fuse_host against the reference's own layers as tools/make_goldens_hints.py recorded them in
tests/golden/depth_hint_fuse.npz, the candidate depths, ops.depth_hint_prepare_host against a direct numpy expression, the KITTI
loader's hint keys on "cpu" over tests/golden/kitti_tree + tests/golden/kitti_hints, and the precompute tool on CPU tensors (with
--candidates_dir, and with a stub cv2 module for the matcher plumbing).  No test needs a GPU or the real OpenCV."""
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

from depthmodelhardening_amd import ops
from depthmodelhardening_amd.datasets import kitti as K
from depthmodelhardening_amd.options import MonodepthOptions
from tests import hint_ref as R
from tests import kitti_ref as KR


@pytest.fixture(scope="module")
def g(golden):
    return golden("depth_hint_fuse")


def _case(g):
    return {k: torch.from_numpy(g[k]) for k in R.ARGS}


def test_the_recipe_is_the_fixtures(g):
    case = R.make_case(**R.GOLDEN_CASE)
    for k in R.ARGS:
        assert torch.equal(case[k], torch.from_numpy(g[k])), k
    cand = case["cand"][0]
    assert bool((cand[:, :, :5] == -16).all()) and 0.1 < float((cand == -16).float().mean()) < 0.5
    for n in range(cand.shape[0]):
        assert int(cand[n].max()) < 16 * R.NUM_DISPARITIES[n % 4]


def test_candidate_depths_equal_the_references(g):
    case = _case(g)
    got = ops.hint_candidate_depths(case["cand"], case["K"])
    want = torch.from_numpy(g["depths"])
    assert got.dtype == torch.float32 and torch.equal(got[0], want)
    invalid = case["cand"][0] <= 0
    assert bool((got[0][invalid] == 0).all()) and bool((got[0][~invalid] > 0).all())


def test_twin_reproduces_the_references_losses_and_pick(g):
    """The twin is the reference's torch expressions: the tool observed max |twin - reference| = twin_dev (0) when it made the
    fixture, and the twin is held to that.  best_depth by value wherever the reference's two lowest losses differ."""
    case = _case(g)
    best, losses = ops.depth_hint_fuse_host(*[case[k] for k in R.ARGS], want_losses=True)
    want = torch.from_numpy(g["loss32"])
    twin_dev = float(g["twin_dev"])
    assert twin_dev <= float(np.finfo(np.float32).eps), "the fixture records more than one ulp of a loss <= 1"
    dev = float((losses[0].double() - want.double()).abs().max())
    assert dev <= twin_dev, (dev, twin_dev)
    two = torch.topk(want, 2, dim=0, largest=False).values
    decided = two[0] != two[1]
    assert float(decided.float().mean()) > 0.9
    want_best = torch.from_numpy(g["best_depth"])
    assert tuple(best.shape) == (1, 1) + tuple(want.shape[1:]) and best.dtype == torch.float32
    assert torch.equal(best[0][decided.unsqueeze(0)], want_best[decided.unsqueeze(0)])
    # the anchor: the float64 form against the reference's modules fed float64
    _, l64 = ops.depth_hint_fuse_host(*[case[k] for k in R.ARGS], want_losses=True, dtype=torch.float64)
    assert l64.dtype == torch.float64 and float((l64[0] - torch.from_numpy(g["loss64"])).abs().max()) <= 1e-12
    assert float((want.double() - l64[0]).abs().max()) == pytest.approx(float(g["ref_dev"]), rel=1e-6)


def test_float_depths_and_int16_agree_and_cpu_tensors_take_the_twin(g):
    case = _case(g)
    args = [case[k] for k in R.ARGS]
    depths = ops.hint_candidate_depths(case["cand"], case["K"])
    a = ops.depth_hint_fuse(*args)
    b, lb = ops.depth_hint_fuse(case["base"], case["lookup"], depths, case["K"], case["inv_K"], case["T"], want_losses=True)
    assert torch.equal(a, b) and tuple(lb.shape) == tuple(depths.shape)
    with pytest.raises(RuntimeError, match="candidates"):
        ops.depth_hint_fuse(case["base"], case["lookup"], depths.repeat(1, 2, 1, 1), case["K"], case["inv_K"], case["T"])
    with pytest.raises(RuntimeError, match="lookup"):
        ops.depth_hint_fuse(case["base"], case["lookup"][:, :, :-1], depths, case["K"], case["inv_K"], case["T"])
    with pytest.raises(RuntimeError, match="int16"):
        ops.depth_hint_fuse(case["base"], case["lookup"], depths.double(), case["K"], case["inv_K"], case["T"])
    with pytest.raises(RuntimeError, match="4, 4"):
        ops.depth_hint_fuse(case["base"], case["lookup"], depths, case["K"][:, :3], case["inv_K"], case["T"])


def test_all_invalid_candidates_give_zero_and_one_candidate_is_itself():
    case = R.make_case(10, 20, N=3, seed=2, all_invalid=True)
    best = ops.depth_hint_fuse_host(*[case[k] for k in R.ARGS])
    assert bool((best == 0).all())
    case = R.make_case(10, 20, N=1, seed=3)
    best = ops.depth_hint_fuse_host(*[case[k] for k in R.ARGS])
    assert torch.equal(best, ops.hint_candidate_depths(case["cand"], case["K"]))


def test_the_layers_above_exist():
    from depthmodelhardening_amd import _native as N, build, library
    assert {"dmh_depth_hint_fuse", "dmh_depth_hint_prepare"} <= set(N.EXPORTS) and "depth_hints.hip" in build.SOURCES
    assert "depth_hint_fuse" in library.OPS and hasattr(torch.ops.dmh, "depth_hint_fuse")
    with pytest.raises(RuntimeError, match="no CPU path"):
        case = R.make_case(10, 20, N=2)
        torch.ops.dmh.depth_hint_fuse(*[case[k] for k in R.ARGS])


# ------------------------------------------------------------------------------------------------ depth_hint_prepare
def _direct(src, flips, H, W):
    Hs, Ws = src.shape[2:]
    yi = np.minimum(np.floor(np.arange(H) * (float(Hs) / H)).astype(np.int64), Hs - 1)
    xi = np.minimum(np.floor(np.arange(W) * (float(Ws) / W)).astype(np.int64), Ws - 1)
    out = np.stack([(np.fliplr(a[0]) if f else a[0])[yi][:, xi][None] for a, f in zip(src, flips)])
    return out, (out > 0).astype(np.float32)


def prepare_input(B, Hs, Ws, seed):
    rng = np.random.RandomState(seed)
    a = rng.uniform(0.5, 80.0, size=(B, 1, Hs, Ws)).astype(np.float32)
    a[rng.uniform(size=a.shape) < 0.3] = 0.0
    a[:, :, 0, 1] = -0.0
    a[:, :, 1, 0] = -1.5
    return a


PREPARE_CASES = [((32, 96), (32, 96), [False, True, False]), ((37, 123), (32, 96), [True, False, True]),
                 ((16, 48), (32, 96), [True, True, False]), ((5, 7), (9, 4), None)]


@pytest.mark.parametrize("src_hw,out_hw,flips", PREPARE_CASES)
def test_prepare_host_against_a_direct_expression(src_hw, out_hw, flips):
    src = prepare_input(3, src_hw[0], src_hw[1], 11)
    hint, mask = ops.depth_hint_prepare_host(torch.from_numpy(src), flips, out_hw)
    want, want_mask = _direct(src, flips or [False] * 3, *out_hw)
    assert hint.dtype == torch.float32 and mask.dtype == torch.float32 and tuple(hint.shape) == (3, 1) + out_hw
    assert np.array_equal(hint.numpy(), want) and np.array_equal(mask.numpy(), want_mask)
    assert float(mask[:, :, 0, :].min()) == 0.0             # -0.0 and negatives are not hints
    if src_hw == out_hw:                                     # the normal case: a (mirrored) copy
        for b, f in enumerate(flips):
            assert np.array_equal(hint[b, 0].numpy(), src[b, 0, :, ::-1] if f else src[b, 0])
    got = ops.depth_hint_prepare(torch.from_numpy(src), None if flips is None else torch.tensor(flips, dtype=torch.int32), out_hw)
    assert torch.equal(got[0], hint) and torch.equal(got[1], mask)      # CPU tensors take the twin
    assert ops.cv_nearest_index(7, 7).tolist() == list(range(7)) and ops.cv_nearest_index(3, 7).max() == 2


def test_prepare_refuses_what_it_cannot_do():
    with pytest.raises(RuntimeError, match="float32"):
        ops.depth_hint_prepare(torch.zeros(2, 1, 4, 4, dtype=torch.float64), None, (4, 4))
    with pytest.raises(RuntimeError, match="one entry per item"):
        ops.depth_hint_prepare(torch.zeros(2, 1, 4, 4), [True], (4, 4))
    with pytest.raises(RuntimeError, match="out_size"):
        ops.depth_hint_prepare(torch.zeros(2, 1, 4, 4), None, (0, 4))


# ------------------------------------------------------------------------------------------------ the loader on "cpu"
def _dataset(hw=KR.TRAIN_SIZE, **kw):
    args = dict(is_train=False, img_ext=".png", num_workers=2, use_depth_hints=True, depth_hint_path=R.HINT_TREE)
    args.update(kw)
    return K.KITTIRAWDataset(KR.TREE, KR.SPLIT_LINES, hw[0], hw[1], [0, "s"], 4, "cpu", **args)


def _tree_hints(lines):
    out = []
    for ln in lines:
        folder, frame, side = K.parse_line(ln)
        out.append(R.tree_hint(folder, side, frame, R.TREE_HINT_SIZE))
    return np.stack(out)


def test_the_hint_tree_is_the_recipes():
    for ln in KR.SPLIT_LINES:
        folder, frame, side = K.parse_line(ln)
        a = np.load(R.hint_path(folder, side, frame))
        assert a.dtype == np.float32 and a.shape == (1,) + R.TREE_HINT_SIZE
        assert np.array_equal(a, R.tree_hint(folder, side, frame, R.TREE_HINT_SIZE))
        assert K.hint_path(R.HINT_TREE, folder, frame, side) == R.hint_path(folder, side, frame)


@pytest.mark.parametrize("hw", [KR.TRAIN_SIZE, R.TREE_HINT_SIZE])
def test_loader_delivers_the_hints(hw):
    pytest.importorskip("PIL")
    ds = _dataset(hw)
    try:
        batch = ds.next_batch(4)
    finally:
        ds.close()
    src = _tree_hints(KR.SPLIT_LINES)
    want, want_mask = _direct(src, [False] * 4, *hw)
    assert tuple(batch["depth_hint"].shape) == (4, 1) + tuple(hw) and batch["depth_hint"].dtype == torch.float32
    assert np.array_equal(batch["depth_hint"].numpy(), want) and np.array_equal(batch["depth_hint_mask"].numpy(), want_mask)
    if tuple(hw) == R.TREE_HINT_SIZE:
        assert np.array_equal(batch["depth_hint"].numpy(), src)
    plain = K.KITTIRAWDataset(KR.TREE, KR.SPLIT_LINES, hw[0], hw[1], [0, "s"], 4, "cpu", img_ext=".png", num_workers=2)
    try:
        other = plain.next_batch(4)
    finally:
        plain.close()
    assert set(batch) - set(other) == {"depth_hint", "depth_hint_mask"}
    for k in other:
        assert torch.equal(batch[k], other[k]), k


def test_loader_flips_the_hints_of_flipped_items():
    pytest.importorskip("PIL")
    ds = _dataset(is_train=True, seed=5)
    ds.order_rng.shuffle = lambda order: None
    ref, flips = random.Random(5), []
    for _ in range(4):
        ref.random()
        flips.append(ref.random() > 0.5)
    assert 0 < sum(flips) < 4
    try:
        batch = ds.next_batch(4)
    finally:
        ds.close()
    want, want_mask = _direct(_tree_hints(KR.SPLIT_LINES), flips, *KR.TRAIN_SIZE)
    assert np.array_equal(batch["depth_hint"].numpy(), want) and np.array_equal(batch["depth_hint_mask"].numpy(), want_mask)


def test_a_missing_hint_raises_the_references_error(tmp_path):
    pytest.importorskip("PIL")
    ds = _dataset(depth_hint_path=str(tmp_path))
    try:
        with pytest.raises(FileNotFoundError, match="cannot find depth hint for .* image_0[23] [0-9]+! Either specify the correct path "
                                                    "in option --depth_hint_path, or run precompute_depth_hints.py"):
            ds.next_batch(2)
    finally:
        ds.close()
    with pytest.raises(RuntimeError, match="use_stereo"):
        K.KITTIRAWDataset(KR.TREE, KR.SPLIT_LINES, 32, 96, [0], 4, "cpu", use_depth_hints=True)


def test_from_options_accepts_depth_hints(tmp_path):
    split = tmp_path / "eigen_zhou"
    split.mkdir()
    (split / "train_files.txt").write_text("\n".join(KR.SPLIT_LINES) + "\n")
    base = ["--data_path", KR.TREE, "--split_dir", str(tmp_path), "--png", "--frame_ids", "0", "--use_stereo", "--height", "32",
            "--width", "96", "--loss_variant", "dh", "--use_depth_hints"]
    def parse(argv):
        opt = MonodepthOptions().parse(argv)
        opt.frame_ids.append("s")               # as the Trainer does for --use_stereo before it builds the dataset
        return opt
    opt = parse(base)
    assert opt.depth_hint_path == os.path.join(KR.TREE, "depth_hints")
    ds = K.from_options(opt, "cpu")
    assert ds.use_depth_hints and ds.depth_hint_path == os.path.join(KR.TREE, "depth_hints")
    ds = K.from_options(parse(base + ["--depth_hint_path", R.HINT_TREE]), "cpu")
    assert ds.use_depth_hints and ds.depth_hint_path == R.HINT_TREE
    ds = K.from_options(parse(base[:-1]), "cpu")
    assert not ds.use_depth_hints


# ------------------------------------------------------------------------------------------------ the tool
TOOL_SIZE = (24, 64)


def _tool_inputs(tmp_path, lines=KR.SPLIT_LINES, n=12):
    """The list file and a candidates tree for ``lines``; returns (argv, {line: candidates})."""
    from depthmodelhardening_amd import precompute_depth_hints as P
    listing = tmp_path / "all_files.txt"
    listing.write_text("\n".join(lines) + "\n")
    cands = {}
    for i, ln in enumerate(lines):
        seq, frame, side = ln.split()
        cand = R.make_case(TOOL_SIZE[0], TOOL_SIZE[1], N=n, side=side, seed=100 + i)["cand"][0].numpy()
        path = P.output_path(str(tmp_path / "cands"), seq, frame, side)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, cand)
        cands[ln] = cand
    argv = ["--data_path", KR.TREE, "--filenames", str(listing), "--save_path", str(tmp_path / "hints"), "--height", str(TOOL_SIZE[0]),
            "--width", str(TOOL_SIZE[1]), "--batch_size", "3", "--num_workers", "64", "--device", "cpu"]
    return argv, cands


def tool_twin(line, cand):
    """What the tool must write for ``line``: PIL-exact LANCZOS of both views (K31's host restatement), the twin's fusion."""
    from depthmodelhardening_amd import precompute_depth_hints as P
    pytest.importorskip("PIL")
    from PIL import Image
    seq, frame, side = line.split()
    views = []
    for sd in (side, "r" if side == "l" else "l"):
        a = np.array(Image.open(K.image_path(KR.TREE, seq, int(frame), sd, ".png")).convert("RGB"))
        u8 = ops.pil_resize(torch.from_numpy(a).unsqueeze(0), TOOL_SIZE, "lanczos", want_float=False).u8
        views.append(u8)
    Km, iK, T = P.camera(TOOL_SIZE[0], TOOL_SIZE[1], [side], "cpu")
    return views, ops.depth_hint_fuse_host(views[0], views[1], torch.from_numpy(cand).unsqueeze(0), Km, iK, T)[0].numpy()


def test_tool_on_cpu_with_candidates_dir(tmp_path):
    pytest.importorskip("PIL")
    from depthmodelhardening_amd import precompute_depth_hints as P
    argv, cands = _tool_inputs(tmp_path)
    assert P.main(argv + ["--candidates_dir", str(tmp_path / "cands")]) == 4
    files = {}
    for ln in KR.SPLIT_LINES:
        seq, frame, side = ln.split()
        path = tmp_path / "hints" / seq / ("image_02" if side == "l" else "image_03") / ("%010d.npy" % int(frame))
        a = np.load(str(path))
        assert a.dtype == np.float32 and a.shape == (1,) + TOOL_SIZE
        assert np.array_equal(a, tool_twin(ln, cands[ln])[1]), ln
        files[ln] = path
    # existing files are skipped ...
    first = files[KR.SPLIT_LINES[0]]
    np.save(str(first), np.zeros((1,) + TOOL_SIZE, dtype=np.float32))
    files[KR.SPLIT_LINES[1]].unlink()
    assert P.main(argv + ["--candidates_dir", str(tmp_path / "cands")]) == 1
    assert not np.load(str(first)).any() and files[KR.SPLIT_LINES[1]].exists()
    # ... unless told to overwrite
    assert P.main(argv + ["--candidates_dir", str(tmp_path / "cands"), "--overwrite_saved_depths"]) == 4
    assert np.array_equal(np.load(str(first)), tool_twin(KR.SPLIT_LINES[0], cands[KR.SPLIT_LINES[0]])[1])
    # the default save path is <data_path>/depth_hints
    assert P.get_opts(["--data_path", "/d"]).save_path is None and P.output_path("/d/depth_hints", "a/b", "7", "r") == "/d/depth_hints/a/b/image_03/0000000007.npy"


def test_tool_without_a_source_of_candidates_says_so(tmp_path, monkeypatch):
    from depthmodelhardening_amd import precompute_depth_hints as P
    monkeypatch.setattr(P, "import_cv2", lambda: None)
    argv, _ = _tool_inputs(tmp_path, KR.SPLIT_LINES[:1], n=2)
    with pytest.raises(RuntimeError, match="cv2.*--candidates_dir"):
        P.main(argv)
    assert not (tmp_path / "hints").exists()


def test_tool_matcher_plumbing_with_a_stub_cv2(tmp_path, monkeypatch):
    """A stub cv2 in sys.modules records StereoSGBM_create's keyword arguments and returns canned int16 arrays: the twelve
    parameter sets in the reference's order, the reversal and un-reversal for a right base image, and what the matchers returned
    reaching the fusion."""
    pytest.importorskip("PIL")
    from depthmodelhardening_amd import precompute_depth_hints as P
    lines = KR.SPLIT_LINES[:2]                  # one left, one right base image
    assert [ln.split()[2] for ln in lines] == ["l", "r"]
    argv, cands = _tool_inputs(tmp_path, lines)
    twins = {ln: tool_twin(ln, cands[ln]) for ln in lines}
    created, calls = [], []

    class Matcher(object):
        def __init__(self, index):
            self.index = index

        def compute(self, left, right):
            assert left.flags["C_CONTIGUOUS"] and left.dtype == np.uint8 and left.shape == TOOL_SIZE + (3,)
            for ln in lines:
                (base, lookup), rev = twins[ln][0], ln.split()[2] != "l"
                b, l = base[0].permute(1, 2, 0).numpy(), lookup[0].permute(1, 2, 0).numpy()
                if np.array_equal(left, b[:, ::-1] if rev else b) and np.array_equal(right, l[:, ::-1] if rev else l):
                    calls.append((ln, self.index))
                    out = cands[ln][self.index]
                    return np.ascontiguousarray(out[:, ::-1]) if rev else out       # canned in the matcher's (mirrored) frame
            raise AssertionError("the matcher was fed images that are no pair of the list (reversed for a right base image)")

    stub = types.ModuleType("cv2")
    stub.setNumThreads = lambda n: created.append(("threads", n))

    def create(**kw):
        created.append(kw)
        return Matcher(len([c for c in created if isinstance(c, dict)]) - 1)
    stub.StereoSGBM_create = create
    monkeypatch.setitem(sys.modules, "cv2", stub)
    assert P.main(argv) == 2
    assert created[0] == ("threads", 0)
    want = [dict(preFilterCap=63, P1=36, P2=288, minDisparity=0, numDisparities=nd, uniquenessRatio=10, speckleWindowSize=100,
                 speckleRange=16, blockSize=bs) for bs in (1, 2, 3) for nd in (64, 96, 128, 160)]
    assert created[1:] == want
    assert sorted(calls) == sorted((ln, i) for ln in lines for i in range(12))
    for ln in lines:
        seq, frame, side = ln.split()
        got = np.load(P.output_path(str(tmp_path / "hints"), seq, frame, side))
        assert np.array_equal(got, twins[ln][1]), ln
