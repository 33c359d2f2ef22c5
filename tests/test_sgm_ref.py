"""K35 on the host: ``ops.sgm_disparity_host`` (whole-image numpy) against the pixel-by-pixel statement of the matcher in
tests/sgm_ref.py, both against the maps tools/make_goldens_sgm.py recorded in tests/golden/sgm_disparity.npz, the properties DESIGN.md
(section 3, K35) states, the sanity of the specification itself on pairs with a known disparity, the parameter refusals, and the
precompute tool with ``--matcher``.  No test needs a GPU or OpenCV; the kernel is held to the same loop reference, bit for bit, in
tests/test_gpu_sgm.py."""
import os

import numpy as np
import pytest
import torch

from depthmodelhardening_amd import ops
from tests import kitti_ref as KR
from tests import sgm_ref as R

# recorded from the loop reference on make_pair(H, W, D, seed = index) without the speckle filter (its window of 100 pixels is
# sized for 320 x 1024 maps): (valid share of the matched columns, share of the valid pixels within 16 units of the truth)
RECORDED_SHARES = {(9, 70, 16, 1): (0.870, 0.938), (16, 100, 32, 3): (0.890, 0.981), (24, 136, 64, 2): (0.950, 0.979),
                   (8, 200, 160, 1): (0.934, 0.949)}
TOOL_SIZE = (16, 208)


@pytest.fixture(scope="module")
def g(golden):
    return golden("sgm_disparity")


def _twin(base, lookup, p, reverse=False):
    out = ops.sgm_disparity_host(torch.from_numpy(base).unsqueeze(0), torch.from_numpy(lookup).unsqueeze(0), [p], [reverse])
    assert out.dtype == torch.int16 and tuple(out.shape) == (1, 1) + base.shape[1:]
    return out[0, 0].numpy()


@pytest.mark.parametrize("case", range(len(R.SHAPES)))
def test_twin_equals_the_loop_reference_and_both_the_golden_file(g, case):
    H, W, D, block = R.SHAPES[case]
    base, lookup, _ = R.make_pair(H, W, D, case)
    seen = 0
    for key, h, w, p, reverse, seed in R.golden_cases():
        if (h, w, p["numDisparities"], p["blockSize"]) != (H, W, D, block):
            continue
        assert seed == case
        want = R.reference(H, W, D, block, reverse, p["speckleWindowSize"], case)
        assert want.dtype == np.int16 and np.array_equal(want, g[key]), key
        assert np.array_equal(_twin(base, lookup, p, reverse), want), key
        seen += 1
    assert seen == 2 * len(R.WINDOWS)


def test_the_golden_file_holds_exactly_the_cases():
    with np.load(R.GOLDEN_PATH) as f:
        assert sorted(f.files) == sorted(c[0] for c in R.golden_cases())
    assert os.path.getsize(R.GOLDEN_PATH) < 100 * 1024


def test_unmatched_columns_and_images_no_wider_than_the_range():
    for case, (H, W, D, block) in enumerate(R.SHAPES):
        for reverse in (False, True):
            out = R.reference(H, W, D, block, reverse, 0, case)
            assert bool((out[:, -D:] == -16).all() if reverse else (out[:, :D] == -16).all())
            assert int((out >= 0).sum()) > 0 and int(out.max()) <= 16 * (D - 1) and int(out.min()) == -16
    base, lookup, _ = R.make_pair(6, 32, 32, 3)
    for D in (32, 48):                      # W == D and W < D
        p = R.params(D, 3)
        assert bool((R.disparity(base, lookup, p) == -16).all()) and bool((_twin(base, lookup, p) == -16).all())


def test_block_sizes_of_one_radius_agree():
    base, lookup, _ = R.make_pair(10, 60, 16, 5)
    two, three, one = (R.disparity(base, lookup, R.params(16, b, 12)) for b in (2, 3, 1))
    assert np.array_equal(two, three) and not np.array_equal(one, three)
    both = ops.sgm_disparity_host(torch.from_numpy(base)[None], torch.from_numpy(lookup)[None], [R.params(16, 3, 12), R.params(16, 2, 12)])
    assert np.array_equal(both[0, 0].numpy(), three) and np.array_equal(both[0, 1].numpy(), three)


def test_reverse_is_flipping_the_inputs_and_the_output():
    H, W, D, block = R.SHAPES[1]
    base, lookup, _ = R.make_pair(H, W, D, 1)
    flipped = np.ascontiguousarray(base[:, :, ::-1]), np.ascontiguousarray(lookup[:, :, ::-1])
    for window in (0, 12):
        p = R.params(D, block, window)
        want = R.disparity(flipped[0], flipped[1], p)[:, ::-1]
        assert np.array_equal(R.reference(H, W, D, block, True, window, 1), want)
        assert np.array_equal(_twin(base, lookup, p, True), want)
        assert not np.array_equal(R.reference(H, W, D, block, False, window, 1), want)


def test_a_constant_pair_matches_everywhere_at_disparity_zero():
    """Every cost is 0, so every S is equal: the lowest d of minimal S is 0, the uniqueness test compares 0 < 0 and keeps the pixel,
    every proposer of a lookup column proposes 0, so the left-right check keeps it too: 0 in every matched column.  The whole map
    is then one component, which the speckle filter removes when it is no larger than the window."""
    for value in (0, 90, 255):
        img = np.full((3, 9, 70), value, dtype=np.uint8)
        for reverse in (False, True):
            out = R.disparity(img, img, R.params(16, 3, 0), reverse)
            matched = out[:, :-16] if reverse else out[:, 16:]
            assert bool((matched == 0).all()) and int((out == -16).sum()) == 9 * 16
            assert np.array_equal(_twin(img, img, R.params(16, 3, 0), reverse), out)
        assert bool((R.disparity(img, img, R.params(16, 3, 9 * 54)) == -16).all())
        assert np.array_equal(R.disparity(img, img, R.params(16, 3, 9 * 54 - 1)), R.disparity(img, img, R.params(16, 3, 0)))
        assert bool((_twin(img, img, R.params(16, 3, 9 * 54)) == -16).all())


def test_the_speckle_filter_removes_some_components_and_keeps_others():
    seen = 0
    for case, (H, W, D, block) in enumerate(R.SHAPES):
        for reverse in (False, True):
            raw = R.reference(H, W, D, block, reverse, 0, case)
            for window in (100, 12):
                out = R.reference(H, W, D, block, reverse, window, case)
                kept, removed = int((out >= 0).sum()), int(((raw >= 0) & (out < 0)).sum())
                assert bool((out[out >= 0] == raw[out >= 0]).all()) and bool((out[raw < 0] == -16).all())
                seen += kept > 0 and removed > 0
    assert seen >= 4
    # at the reference's window: (8, 200, 160, 1) loses 102 of its 299 valid pixels and keeps 197
    raw, out = R.reference(8, 200, 160, 1, False, 0, 3), R.reference(8, 200, 160, 1, False, 100, 3)
    assert (int((raw >= 0).sum()), int((out >= 0).sum())) == (299, 197)


def test_uniqueness_and_left_right_check_both_remove_pixels():
    """Neither branch is dead: per case the pixels the uniqueness test drops, and those it kept that the left-right check removes."""
    total = {"not_unique": 0, "lr_removed": 0}
    for case, (H, W, D, block) in enumerate(R.SHAPES[:3]):
        base, lookup, _ = R.make_pair(H, W, D, case)
        stages = {}
        out = R.disparity(base, lookup, R.params(D, block, 0), False, stages)
        assert stages.get("not_unique", 0) > 0 and stages.get("lr_removed", 0) > 0, (case, stages.keys())
        assert np.array_equal(out, stages["raw"])
        loose = R.disparity(base, lookup, R.params(D, block, 0, disp12MaxDiff=D), False)         # a check that can never fire
        assert int((loose >= 0).sum()) - int((out >= 0).sum()) == stages["lr_removed"]
        assert np.array_equal(_twin(base, lookup, R.params(D, block, 0, disp12MaxDiff=D)), loose)
        for k in total:
            total[k] += stages[k]
    assert total == {"not_unique": 22 + 23 + 37, "lr_removed": 41 + 96 + 48}


@pytest.mark.parametrize("case", range(len(R.SHAPES)))
def test_the_specification_finds_the_true_disparity(case):
    H, W, D, block = R.SHAPES[case]
    _, _, truth = R.make_pair(H, W, D, case)
    valid, near = R.shares(R.reference(H, W, D, block, False, 0, case), truth, D)
    want_valid, want_near = RECORDED_SHARES[R.SHAPES[case]]
    print("%s: valid %.3f (recorded %.3f), within one disparity of the truth %.3f (recorded %.3f)" % (R.SHAPES[case], valid, want_valid, near, want_near))
    assert valid >= want_valid - 0.03 and near >= want_near - 0.03
    assert int(truth.max()) < D and len(np.unique(truth)) == 3


def test_sub_pixel_division_truncates_toward_zero():
    assert [R.tdiv(a, 8) for a in (-15, -9, -8, -7, -1, 0, 7, 8, 15)] == [-1, -1, -1, 0, 0, 0, 0, 1, 1]
    S = np.full((1, 1, 16), 500, dtype=np.int64)
    S[0, 0, 5:8] = (100, 40, 43)            # den = 63, (100 - 43) 16 + 63 = 975 -> 975 / 126 = 7
    assert R.select_row(S[0], 16, 17, 10, 0)[16] == 16 * 6 + 7
    assert int(ops._sgm_select(S.astype(np.int32), 17, 10, 0)[0, 16]) == 16 * 6 + 7
    S[0, 0, 5:8] = (43, 40, 100)            # (43 - 100) 16 + 63 = -849 -> -849 / 126 = -6 in C (floor would give -7)
    assert R.select_row(S[0], 16, 17, 10, 0)[16] == 16 * 6 - 6
    assert int(ops._sgm_select(S.astype(np.int32), 17, 10, 0)[0, 16]) == 16 * 6 - 6


def test_parameter_refusals():
    base = torch.zeros(1, 3, 8, 40, dtype=torch.uint8)
    ok = R.params(16, 3)
    for bad, match in ((dict(ok, blockSize=5), "blockSize"), (dict(ok, blockSize=0), "blockSize"), (dict(ok, numDisparities=24), "multiple of 16"),
                       (dict(ok, numDisparities=0), "multiple of 16"), (dict(ok, numDisparities=272), "multiple of 16"),
                       (dict(ok, minDisparity=1), "minDisparity"), (dict(ok, P2=1500), "int16"), (dict(ok, P1=-1), "P1"),
                       (dict(ok, preFilterCap=64), "preFilterCap"), (dict(ok, uniquenessRatio=101), "uniquenessRatio"),
                       (dict(ok, disp12MaxDiff=-1), "disp12MaxDiff"), (dict(ok, mode=1), "unknown"),
                       ({k: v for k, v in ok.items() if k != "P1"}, "lacks")):
        with pytest.raises(RuntimeError, match=match):
            ops.sgm_disparity(base, base, [bad])
        with pytest.raises(RuntimeError, match=match):
            ops.sgm_plan(1, 8, 40, [bad])
    assert ops.sgm_disparity(base, base, [dict(ok, P2=1447)]).shape == (1, 1, 8, 40)        # 5 (9 x 567 + 1447) = 32750
    with pytest.raises(RuntimeError, match="N <= 16"):
        ops.sgm_disparity(base, base, [ok] * 17)
    with pytest.raises(RuntimeError, match="N <= 16"):
        ops.sgm_disparity(base, base, [])
    with pytest.raises(RuntimeError, match="uint8"):
        ops.sgm_disparity(base.float(), base.float(), [ok])
    with pytest.raises(RuntimeError, match="lookup"):
        ops.sgm_disparity(base, base[:, :, :, :-1], [ok])
    with pytest.raises(RuntimeError, match="one entry per item"):
        ops.sgm_disparity(base, base, [ok], reverse=[True, False])
    with pytest.raises(RuntimeError, match="W <= 4096"):
        ops.sgm_disparity(torch.zeros(1, 3, 1, 4097, dtype=torch.uint8), torch.zeros(1, 3, 1, 4097, dtype=torch.uint8), [ok])


def test_plan_reports_bytes_and_chunks():
    """Host only: per item and distinct parameter set two int16 volumes [H][W - D][D] and 8 H W bytes of labels, each rounded up to
    256 bytes; blockSize 2 and 3 are one set; at most 32 sets per sequence of launches."""
    from depthmodelhardening_amd.precompute_depth_hints import stereo_matcher_params
    def up(v):
        return (v + 255) // 256 * 256
    per_item = 2 * sum(2 * up(2 * 16 * (208 - D) * D) + up(8 * 16 * 208) for D in (64, 96, 128, 160))
    assert ops.sgm_plan(3, 16, 208, stereo_matcher_params()) == (3 * per_item, 1)
    assert ops.sgm_plan(5, 16, 208, stereo_matcher_params()) == (4 * per_item, 2)              # 40 jobs: 32 + 8
    nbytes, chunks = ops.sgm_plan(3, 16, 208, stereo_matcher_params(), 3 << 20)
    assert nbytes <= 3 << 20 and chunks == 6
    assert ops.sgm_plan(1, 16, 208, [R.params(256, 1, 0)]) == (256, 1)                          # W <= D, no speckle filter: nothing to hold
    with pytest.raises(RuntimeError, match="cap"):
        ops.sgm_plan(3, 16, 208, stereo_matcher_params(), 1 << 16)
    nbytes, chunks = ops.sgm_plan(8, 320, 1024, stereo_matcher_params())
    assert nbytes <= 2 << 30 and chunks == 4


def test_the_layers_above_exist():
    from depthmodelhardening_amd import _native as N, build, library
    assert {"dmh_sgm_plan", "dmh_sgm_disparity"} <= set(N.EXPORTS) and "sgm_stereo.hip" in build.SOURCES
    assert "sgm_disparity" in library.OPS and hasattr(torch.ops.dmh, "sgm_disparity")
    flat = library.sgm_params_flat([R.params(64, 3), R.params(16, 1, 0, disp12MaxDiff=2)])
    assert len(flat) == 20 and library.sgm_params_unflat(flat)[1]["disp12MaxDiff"] == 2
    base = torch.zeros(1, 3, 8, 40, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.dmh.sgm_disparity(base, base, flat)


# ------------------------------------------------------------------------------------------------ the tool
def _argv(tmp_path, root, lines, *more):
    listing = tmp_path / "all_files.txt"
    listing.write_text("\n".join(lines) + "\n")
    return ["--data_path", root, "--filenames", str(listing), "--save_path", str(tmp_path / "hints"), "--height", str(TOOL_SIZE[0]),
            "--width", str(TOOL_SIZE[1]), "--batch_size", "3", "--num_workers", "4", "--device", "cpu"] + list(more)


def test_tool_with_the_device_matcher_on_cpu_tensors_writes_every_file(tmp_path):
    pytest.importorskip("PIL")
    from depthmodelhardening_amd import precompute_depth_hints as P
    assert P.main(_argv(tmp_path, KR.TREE, KR.SPLIT_LINES, "--matcher", "device")) == len(KR.SPLIT_LINES)
    for ln in KR.SPLIT_LINES:
        a = np.load(P.output_path(str(tmp_path / "hints"), *ln.split()))
        assert a.dtype == np.float32 and a.shape == (1,) + TOOL_SIZE and bool(np.isfinite(a).all())
    assert not (tmp_path / "cands").exists()


def test_tool_saved_candidates_reproduce_the_hints_through_files(tmp_path):
    """On a tree of synthetic pairs: ``--matcher device --save_candidates`` writes the twin's maps for the resized bytes, with the
    line's side as ``reverse``; ``--matcher files`` on them gives the same hints."""
    pytest.importorskip("PIL")
    from depthmodelhardening_amd import precompute_depth_hints as P
    from depthmodelhardening_amd.datasets import kitti as K
    from PIL import Image
    root = str(tmp_path / "tree")
    lines = R.write_tree(root, TOOL_SIZE)
    assert [ln.split()[2] for ln in lines] == ["l", "r", "l"]
    argv = _argv(tmp_path, root, lines)
    assert P.main(argv + ["--matcher", "device", "--save_candidates", str(tmp_path / "cands")]) == 3
    first = {}
    for ln in lines:
        seq, frame, side = ln.split()
        cand, hint = np.load(P.output_path(str(tmp_path / "cands"), seq, frame, side)), np.load(P.output_path(str(tmp_path / "hints"), seq, frame, side))
        assert cand.dtype == np.int16 and cand.shape == (12,) + TOOL_SIZE
        views = []
        for sd in (side, "r" if side == "l" else "l"):
            a = np.array(Image.open(K.image_path(root, seq, int(frame), sd, ".png")).convert("RGB"))
            views.append(ops.pil_resize(torch.from_numpy(a).unsqueeze(0), TOOL_SIZE, "lanczos", want_float=False).u8)
        want = ops.sgm_disparity_host(views[0], views[1], P.stereo_matcher_params(), [side != "l"])
        assert np.array_equal(cand, want[0].numpy()), ln
        seen = cand[:, :, 160:] if side == "l" else cand[:, :, :-160]
        assert float((seen >= 0).mean()) > 0.5 and float((hint > 0).mean()) > 0.5, ln
        first[ln] = hint
    again = argv[:argv.index("--save_path") + 1] + [str(tmp_path / "again")] + argv[argv.index("--save_path") + 2:]
    assert P.main(again + ["--matcher", "files", "--candidates_dir", str(tmp_path / "cands")]) == 3
    for ln in lines:
        assert np.array_equal(np.load(P.output_path(str(tmp_path / "again"), *ln.split())), first[ln]), ln


def test_tool_matcher_choices(tmp_path, monkeypatch):
    from depthmodelhardening_amd import precompute_depth_hints as P
    monkeypatch.setattr(P, "import_cv2", lambda: None)
    argv = _argv(tmp_path, KR.TREE, KR.SPLIT_LINES[:1])
    assert P.get_opts(argv).matcher == "auto" and P.get_opts(argv).save_candidates is None
    with pytest.raises(RuntimeError, match="no source of candidate disparities.*cv2.*--candidates_dir"):
        P.main(argv)                                # auto without cv2 and without files: as before
    with pytest.raises(RuntimeError, match="no source of candidate disparities"):
        P.main(argv + ["--matcher", "auto"])
    with pytest.raises(RuntimeError, match="--matcher opencv"):
        P.main(argv + ["--matcher", "opencv"])
    with pytest.raises(RuntimeError, match="--matcher files needs --candidates_dir"):
        P.main(argv + ["--matcher", "files"])
    with pytest.raises(SystemExit):
        P.get_opts(argv + ["--matcher", "sgbm"])
    assert not (tmp_path / "hints").exists()
