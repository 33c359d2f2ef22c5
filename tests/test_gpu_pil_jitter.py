"""K33 (csrc/color_jitter.hip) on the GPU: ``ops.pil_color_jitter`` against its host twin (which tests/test_pil_jitter_ref.py holds
to Pillow itself) and against Pillow's recorded results in tests/golden/pil_jitter.npz, ``torch.equal`` on the bytes and on the
floats; the KITTI loader's ``jitter="pil"`` and two train steps with ``--kitti_jitter pil``.

K33's workgroup is 256 threads; it takes 1024 pixels a round when H W is a multiple of 4 and 256 otherwise, and a launch has about
2048 workgroups, at least 4 per image.  67 x 259 = 17353 pixels is odd (68 rounds of 256, the last one partial); three tensors of
24 items leave an image 28 workgroups, so each of them strides."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from depthmodelhardening_amd import color_jitter, ops  # noqa: E402
from tests import jitter_ref as J  # noqa: E402
from tests import kitti_ref as R  # noqa: E402

DEV = torch.device("cuda")


def host(images, params):
    """The host twin on [B, 3, H, W] arrays -> uint8 tensors, one per array."""
    rec = params if isinstance(params, np.ndarray) else color_jitter.pil_records(params)
    return [torch.from_numpy(a) for a in ops.pil_color_jitter_host(images, rec)]


def device(images, params, want_u8=True):
    if isinstance(params, np.ndarray):
        params = torch.from_numpy(params).to(DEV)
    return ops.pil_color_jitter([torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in images], params, want_u8)


def check(got, want):
    assert len(got) == len(want)
    for res, w in zip(got, want):
        assert res.u8.dtype == torch.uint8 and res.f32.dtype == torch.float32 and res.f32.is_contiguous()
        assert torch.equal(res.u8.cpu(), w)
        assert torch.equal(res.f32.cpu(), w.float().div(255))


@pytest.fixture(scope="module")
def g(golden):
    return golden("pil_jitter")


@pytest.mark.parametrize("key", [k for k, _, _ in J.golden_cases()])
def test_golden_cases(g, key):
    """5 x 7, 37 x 53 (odd width), 32 x 96 (four pixels per thread), 67 x 259 (several workgroups, a partial last round), the 24
    orders, a batch that mixes plain and jittered items, the contrast tie, the 255 clip, a flat image, the hue shift 0."""
    images, params = next((im, p) for k, im, p in J.golden_cases() if k == key)
    got = device([images], params)
    check(got, host([images], params))
    check(got, [torch.from_numpy(g[key])])


def test_plain_items_are_only_converted():
    _, images, params = next(c for c in J.golden_cases() if c[0] == "mixed")
    assert [p is None for p in params] == [False, True, False, True, False]
    res = device([images], params, want_u8=False)[0]
    assert res.u8 is None
    src = torch.from_numpy(images)
    plain = src.float().div(255)        # on the host: to_tensor's IEEE division (on the device torch multiplies by 1 / 255)
    for i, p in enumerate(params):
        assert torch.equal(res.f32[i].cpu(), plain[i]) == (p is None), i
    none = device([images], [None] * 5)[0]                       # no contrast anywhere: the second pass alone
    assert torch.equal(none.u8.cpu(), src) and torch.equal(none.f32.cpu(), plain)


def test_three_tensors_24_orders_strided():
    """Three tensors with different content in one call: item i of each takes order i, every image its own mean."""
    params = J.order_params("three")
    images = [J.batch("three/%d" % t, 24, (67, 259)) for t in range(3)]
    sums = []
    want = [torch.from_numpy(a) for a in ops.pil_color_jitter_host(images, color_jitter.pil_records(params), sums)]
    assert len(sums) == 72 and len(set(sums)) > 60                # the means differ across the tensors
    check(device(images, params), want)


def test_lattice_tie_and_clip_images():
    lat = J.lattice()[None]
    for shift in J.LATTICE_SHIFTS:
        check(device([lat], J.hue_record(shift)), host([lat], J.hue_record(shift)))
    for f in J.LATTICE_SATURATIONS:
        check(device([lat], [J.only("saturation", f)]), host([lat], [J.only("saturation", f)]))
    for f in (0.9, 0.0):
        check(device([J.TIE[None]], [J.only("contrast", f)]), host([J.TIE[None]], [J.only("contrast", f)]))
    assert set(device([J.TIE[None]], [J.only("contrast", 0.0)])[0].u8.reshape(-1).tolist()) == {11}
    img, p = J.clip_case()
    check(device([img[None]], [p]), host([img[None]], [p]))
    check(device([img[None]], [J.only("brightness", 1.2)]), host([img[None]], [J.only("brightness", 1.2)]))


def test_training_shape_and_reproducibility():
    images = J.batch("train", 1, (320, 1024))
    params = [J.draw(random.Random(11))]
    first = device([images], params)
    check(first, host([images], params))
    again = device([images], params)
    assert torch.equal(first[0].u8, again[0].u8) and torch.equal(first[0].f32, again[0].f32)
    many = [J.batch("many/%d" % t, 6, (37, 53)) for t in range(2)]
    p6 = J.order_params("many")[5:11]
    a, b = device(many, p6), device(many, p6)
    for x, y in zip(a, b):
        assert torch.equal(x.u8, y.u8) and torch.equal(x.f32, y.f32)


def test_graph_replay_reads_the_record_on_the_device():
    images = J.batch("graph", 4, (32, 96))
    pa, pb = J.order_params("graph/a")[:4], J.order_params("graph/b")[8:12]
    src = torch.from_numpy(images).to(DEV)
    rec = torch.from_numpy(color_jitter.pil_records(pa)).to(DEV)
    ops.pil_color_jitter([src], rec, want_u8=True)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):            # pass 1, pass 2 in a row: no parallel branches
            held = ops.pil_color_jitter([src], rec, want_u8=True)
    held[0].u8.zero_()
    held[0].f32.zero_()
    graph.replay()
    torch.cuda.synchronize()
    check(held, host([images], pa))
    rec.copy_(torch.from_numpy(color_jitter.pil_records(pb)).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    check(held, host([images], pb))
    assert not torch.equal(host([images], pa)[0], host([images], pb)[0])


def test_the_operator_and_its_argument_checks():
    from depthmodelhardening_amd import library  # noqa: F401
    images = J.batch("op", 2, (32, 96))
    params = J.order_params("op")[:2]
    src = torch.from_numpy(images).to(DEV)
    rec = torch.from_numpy(color_jitter.pil_records(params)).to(DEV)
    out = torch.ops.dmh.color_jitter([src, src.flip(0).contiguous()], rec, True)
    assert len(out) == 4 and torch.equal(out[2].cpu(), host([images], params)[0]) and torch.equal(out[0].cpu(), out[2].cpu().float().div(255))
    torch.library.opcheck(torch.ops.dmh.color_jitter, ([src], rec, True), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(RuntimeError, match="prepared record"):
        ops.pil_color_jitter([src], rec[:1])
    with pytest.raises(RuntimeError, match="prepared record"):
        ops.pil_color_jitter([src], rec.cpu())
    with pytest.raises(RuntimeError, match="uint8"):
        ops.pil_color_jitter([src.float()], rec)


# ---------------------------------------------------------------------------------------------------------------- the loader
def _spy(monkeypatch):
    """Records every call of ops.pil_color_jitter: (the byte tensors, the transforms, the results)."""
    calls, real = [], ops.pil_color_jitter

    def recorder(images, params, want_u8=False):
        res = real(images, params, want_u8)
        calls.append(([t.cpu().numpy() for t in images], list(params), [r.f32.cpu() for r in res]))
        return res
    monkeypatch.setattr(ops, "pil_color_jitter", recorder)
    return calls


def _batch(device, **kw):
    from depthmodelhardening_amd.datasets import KITTIRAWDataset
    pytest.importorskip("PIL")
    args = dict(is_train=True, img_ext=".png", num_workers=4, seed=6, color_aug=True, jitter="pil")
    args.update(kw)
    ds = KITTIRAWDataset(R.TREE, R.SPLIT_LINES, R.TRAIN_SIZE[0], R.TRAIN_SIZE[1], [0, "s"], 4, device, **args)
    ds.order_rng.shuffle = lambda order: None
    try:
        return ds.next_batch(4)
    finally:
        ds.close()


def test_loader_batch_equals_the_cpu_batch(monkeypatch):
    calls = _spy(monkeypatch)
    gpu = _batch(DEV)
    assert len(calls) == 1 and len(calls[0][0]) == 1              # one call for the batch: ("color_aug", 0, 0) is its only key
    cpu = _batch("cpu")
    assert sorted(gpu, key=str) == sorted(cpu, key=str)
    for k in cpu:
        assert torch.equal(gpu[k].cpu(), cpu[k]), k
    coins = [p is not None for p in calls[0][1]]
    assert 0 < sum(coins) < 4, "the seed must mix jittered and plain items"
    floats = _batch(DEV, jitter="float")                          # the same draws: every ("color", ...) key is untouched
    for k in gpu:
        if k[0] != "color_aug":
            assert torch.equal(gpu[k], floats[k]), k
    for i, c in enumerate(coins):
        assert torch.equal(gpu[("color_aug", 0, 0)][i], gpu[("color", 0, 0)][i]) == (not c), i
    want = host(calls[0][0], calls[0][1])[0]
    assert torch.equal(gpu[("color_aug", 0, 0)].cpu(), want.float().div(255))


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """(split_dir, scene_root) as tests/test_gpu_kitti_trainer.py builds them: the made-up split lists and one 375 x 1242 scene."""
    import os
    from PIL import Image
    base = tmp_path_factory.mktemp("kitti_jitter")
    for split in ("eigen_zhou", "eigen"):
        os.makedirs(str(base / "splits" / split))
    for name in ("train_files.txt", "val_files.txt"):
        (base / "splits" / "eigen_zhou" / name).write_text("\n".join(R.SPLIT_LINES) + "\n")
    (base / "splits" / "eigen" / "test_files.txt").write_text("\n".join(R.SPLIT_LINES) + "\n")
    os.makedirs(str(base / "scenes" / "vehicle_detection"))
    os.makedirs(str(base / "scenes" / "training" / "image_2"))
    ys, xs = np.meshgrid(np.arange(376), np.arange(1244), indexing="ij")
    scene = np.stack([(xs // 5) % 256, (ys * 3) % 256, ((xs + ys) // 7) % 256], -1).astype(np.uint8)
    Image.fromarray(scene).save(str(base / "scenes" / "training" / "image_2" / "000000.png"))
    (base / "scenes" / "vehicle_detection" / "training.txt").write_text("000000 1\n")
    return str(base / "splits"), str(base / "scenes")


def _trainer(tmp_path, roots, seed, hw, batch=4):
    from depthmodelhardening_amd.options import MonodepthOptions
    from depthmodelhardening_amd.trainer import Trainer
    argv = ["--dataset", "kitti", "--data_path", R.TREE, "--split_dir", roots[0], "--scene_root", roots[1], "--png",
            "--frame_ids", "0", "--use_stereo", "--height", str(hw[0]), "--width", str(hw[1]), "--batch_size", str(batch), "--weights_init", "scratch",
            "--log_dir", str(tmp_path), "--model_name", "t", "--atk_steps", "2", "--atk_batch_size", "2", "--num_workers", "4",
            "--kitti_jitter", "pil", "--contrastive_learning", "--adv_train", "--norm_type", "l_inf"]
    random.seed(seed)               # the attack's EOT pose draws use the random module (physicalTrans.py:150-155)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return Trainer(MonodepthOptions().parse(argv), device=DEV)


def test_adversarial_batch_jitters_color_ben_with_the_items_transform(tmp_path, roots, monkeypatch):
    pytest.importorskip("PIL")
    calls = _spy(monkeypatch)
    tr = _trainer(tmp_path, roots, 6, R.TRAIN_SIZE)
    try:
        assert tr.dataset.jitter == "pil" and tr.dataset.color_aug
        for seed in range(64):                                    # the first seed whose four coins are mixed
            tr.dataset.rng = random.Random(seed)
            if 0 < sum(tr.dataset.draw_batch_geometry(4, ["l"] * 4)["jitter"]) < 4:
                break
        tr.dataset.rng = random.Random(seed)
        batch = tr.dataset.next_batch(4)
    finally:
        tr.dataset.close()
    keys = [q for q in batch if q[0] in ("color_aug", "color_ben")]
    assert ("color_ben", 0, 0) in keys and ("color_aug", 0, 0) in keys
    assert len(calls) == 1 and len(calls[0][0]) == len(keys)      # one call for all of them
    images, params, results = calls[0]
    coins = [p is not None for p in params]
    assert 0 < sum(coins) < 4
    want = host(images, params)
    for key, res, w, src in zip(keys, results, want, images):
        assert torch.equal(batch[key].cpu(), res) and torch.equal(res, w.float().div(255)), key
        for i, c in enumerate(coins):
            assert torch.equal(res[i], torch.from_numpy(src[i]).float().div(255)) == (not c), (key, i)
    ben = keys.index(("color_ben", 0, 0))
    assert torch.equal(torch.from_numpy(images[ben]).float().div(255), batch[("color", 0, 0)].cpu())      # the benign level 0's bytes
    assert not np.array_equal(images[ben], images[keys.index(("color_aug", 0, 0))])                       # the object


def test_two_train_steps_with_kitti_jitter_pil(tmp_path, roots, monkeypatch):
    """Batch 2 at 64 x 192, the shapes of tests/test_gpu_kitti_trainer.py's own two steps, under the same seeds and the library's
    repeatable algorithms; the steps must have jittered (K33 ran in them)."""
    pytest.importorskip("PIL")
    runs, launches, real = [], [], ops.pil_color_jitter
    monkeypatch.setattr(ops, "pil_color_jitter", lambda *a, **kw: launches.append(len(a[0])) or real(*a, **kw))
    for _ in range(2):                  # the same seed twice
        with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            tr = _trainer(tmp_path, roots, 3, (64, 192), batch=2)
            try:
                tr.set_train()
                runs.append([float(tr.train_step()["loss"]) for _ in range(2)])
                torch.cuda.synchronize()
            finally:
                tr.dataset.close()
    print("two runs from one seed (loss, loss):", runs, "tensors per K33 call:", launches)
    assert launches and launches[:len(launches) // 2] == launches[len(launches) // 2:], launches      # the steps did jitter
    assert all(np.isfinite(v) for v in runs[0]), runs
    assert runs[0] == runs[1], runs
