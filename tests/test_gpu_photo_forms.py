"""K1 (csrc/photo_loss.hip) held to the float64 oracle in every launch form the other files leave to "finite and non-zero":
three source frames, two frames in the DepthHints variant, tie-break noise with more than one frame (tensor and Philox), the
generic one-frame kernel behind --no_ssim / --disable_automasking with its backward, the pose gradient with one and with
three frames, and the strip heights pick_rows gives the workload (16 / 32 rows forward, 18 / 33 backward).

Every numeric case asserts, with the rules tests/test_gpu_kernels.py already uses and no other: the loss scalars; the
selection codes EXACTLY (0 identity, 1 + f frame f) against the argmin the test forms itself from the oracle's candidate stack,
on every pixel whose two smallest candidates are further apart than the tie width; to_opt; the disparity gradients through
GradPool (HIP no further from float64 than 1.5 x the fp32 oracle); and bitwise repeatability.  The conditions on the inputs --
under 1 % of the pixels inside the tie band, every candidate the winner on at least 1 % -- are checked on the oracle alone:
every selection code and every noise slot is then exercised.  DESIGN.md, "Launch forms and float64 anchors of K1", has the
table of instantiations and the measured figures."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.photo_cases import (L1_ATOL, PIX_ATOL, candidate_stack, frames_case, oracle_pass, selection_reference,  # noqa: E402
                               tie_noise)
from tests.util import GradPool, assert_close_frac, to_dev  # noqa: E402

MS = (0, -1, 1, "s")        # Monodepth2's "MS": --frame_ids 0 -1 1 --use_stereo
FW_OUT, BW_OUT = 62, 60     # output columns of a forward / backward strip (csrc/photo_loss.hip)


def _mods():
    from depthmodelhardening_amd import _native as N, ops
    return N, ops


def _hip(case, inputs_d, disps, poses_d, noise, backward):
    N, ops = _mods()
    fids = case["fids"]
    dd = [d.cuda().requires_grad_(backward) for d in disps]
    nz = None
    if noise is not None and case.get("automask", True):
        nz = [noise[s].cuda() for s in range(4)]
    out = ops.photometric_smooth_loss(
        inputs_d[("color", 0, 0)], [inputs_d[("color", f, 0)] for f in fids[1:]],
        [inputs_d["stereo_T"] if f == "s" else poses_d[f] for f in fids[1:]], inputs_d[("K", 0)], inputs_d[("inv_K", 0)], dd,
        [inputs_d[("color", 0, s)] for s in range(4)], variant=case.get("variant", "md2"), automask=case.get("automask", True),
        no_ssim=case.get("no_ssim", False), noise=nz, want_to_opt=True)
    if backward:
        out.fin[N.FIN_LOSS].backward()
    return out, [d.grad for d in dd]


def _pin_rows(case, B, H, W, inputs_d, disps, poses_d):
    """The strip heights the case must run at, read back from the sizes of the partial-sum buffers: a later change of pick_rows's
    thresholds then fails here and does not silently move the case back to 8 / 9 rows."""
    N, ops = _mods()
    fw, bw = case["rows"]
    lib = N.lib()
    assert lib.dmh_photo_partials_size(B, H, W, 4) == 16 * B * (-(-W // FW_OUT)) * (-(-H // fw)), ("forward strip height", fw)
    fids = case["fids"]
    cfg = dict(min_depth=0.1, max_depth=100.0, variant=case.get("variant", "md2"), automask=True, no_ssim=False,
               noise_mode=N.NOISE_NONE)
    dd = [d.cuda() for d in disps]
    a = ops._photo_args(cfg, inputs_d[("color", 0, 0)], [inputs_d[("color", f, 0)] for f in fids[1:]],
                        [inputs_d["stereo_T"] if f == "s" else poses_d[f] for f in fids[1:]], inputs_d[("K", 0)],
                        inputs_d[("inv_K", 0)], dd, ())
    nf = len(fids) - 1
    assert lib.dmh_photo_pose_partials_size(C.byref(a)) == 4 * B * (-(-W // BW_OUT)) * (-(-H // bw)) * nf * 12, (
        "backward strip height", bw)


def run_case(case, B, H, W, seeds, oracle_device="cpu", backward=True):
    """One row of the form matrix: every seed against the fp32 and the float64 oracle."""
    N, _ = _mods()
    fids, variant = case["fids"], case.get("variant", "md2")
    automask, no_ssim = case.get("automask", True), case.get("no_ssim", False)
    nf = len(fids) - 1
    width = 2 * (L1_ATOL if no_ssim else PIX_ATOL)
    pool = GradPool(count_floor=2.0 / (H * W) if variant == "dh" else 0.0)
    for seed in seeds:
        inputs, disps, poses = frames_case(B, H, W, seed, fids, case.get("coarsest", 8))
        noise = None
        if automask and case.get("sigma", 1e-5):
            noise = tie_noise(B, nf if variant == "md2" else 1, H, W, seed, case.get("sigma", 1e-5))
        kw = dict(variant=variant, automask=automask, no_ssim=no_ssim, device=oracle_device, backward=backward)
        o32 = oracle_pass(inputs, disps, poses, fids, noise, dtype=torch.float32, **kw)
        o64 = oracle_pass(inputs, disps, poses, fids, noise, dtype=torch.float64, **kw)
        losses, losses64 = o32["losses"], o64["losses"]
        inputs_d, poses_d = to_dev(inputs), to_dev(poses)
        if "rows" in case:
            _pin_rows(case, B, H, W, inputs_d, disps, poses_d)
        out, grads = _hip(case, inputs_d, disps, poses_d, noise, backward)
        out2, grads2 = _hip(case, inputs_d, disps, poses_d, noise, backward)
        torch.cuda.synchronize()
        # ---- a second identical call gives the same bits
        assert torch.equal(out.fin, out2.fin) and torch.equal(out.sel.packed, out2.sel.packed), "fin / packed selection bits"
        if backward:
            assert all(torch.equal(a_, b_) for a_, b_ in zip(grads, grads2)), "gradient bits"
        f = out.fin.detach().cpu()

        # ---- scalars: scalar_ok of test_photo_smooth_loss_vs_oracle (md2's mean(min(.)) is continuous in the inputs: 2e-5 against
        # the fp32 oracle; dh's masked-sum / mask-count jumps at every flipped near-tie, in the fp32 oracle as much as in the
        # kernel: 1.5 x the fp32 oracle's distance from float64, plus two flips)
        def scalar_ok(got, key):
            if variant == "md2":
                return abs(got - losses[key].item()) <= 2e-5 * abs(losses[key].item())
            ref64 = losses64[key].item()
            return abs(got - ref64) <= 1.5 * abs(losses[key].item() - ref64) + max(2e-5, 2.0 / (B * H * W)) * abs(ref64)
        keys = [(N.FIN_LOSS, "loss")] + [(N.FIN_LOSS_S + s, "loss/%d" % s) for s in range(4)]
        if variant == "dh":
            keys += [(N.FIN_REPROJ_S + s, "reproj_loss/%d" % s) for s in range(4)]
        for slot, key in keys:
            print("%s seed %d %-14s hip %.9g  oracle fp32 %.9g  fp64 %.12g" % (case["id"], seed, key, f[slot].item(),
                                                                           losses[key].item(), losses64[key].item()))
            assert scalar_ok(f[slot].item(), key), (key, f[slot].item(), losses[key].item(), losses64[key].item())
        for s in range(4):
            # ---- conditions on the inputs, on the oracle alone
            stack, codes = candidate_stack(o32, fids, s, variant, automask, no_ssim)
            code, tie, wins = selection_reference(stack, codes, width)
            print("%s seed %d scale %d: tie band %.4f of the pixels, candidates win %s" % (
                case["id"], seed, s, tie.float().mean().item(), " ".join("%.3f" % w for w in wins.tolist())))
            assert tie.float().mean().item() < 0.01, "tie band"
            assert wins.min().item() >= 0.01, ("a candidate never wins: this case cannot see its index", wins.tolist())
            # ---- selection codes, exactly, away from ties
            sel = out.sel[s].to(code.device)
            off = ~tie
            n_bad = int(((sel != code) & off).sum())
            assert n_bad == 0, "scale %d: %d selection codes differ away from ties (%d pixels compared)" % (s, n_bad, int(off.sum()))
            if automask:    # and as the trainer decodes them into identity_selection/s (trainer.py, compute_losses)
                dec = (sel > 0).float()
                if variant == "dh":
                    dec = 1 - dec
                ref_sel = o32["outs"]["identity_selection/%d" % s].reshape(B, H, W)
                assert int(((dec != ref_sel) & off).sum()) == 0
            # ---- to_opt
            ref_map = o32["maps"][s].reshape(B, H, W)
            got_map = out.to_opt[s].to(ref_map.device)
            if variant == "dh":   # masked map: a flipped tie moves the value by the whole loss, compare off-tie only
                got_map, ref_map = got_map[off], ref_map[off]
            assert_close_frac(got_map, ref_map, rtol=1e-4, atol=PIX_ATOL, name="to_opt[%d]" % s)
            if no_ssim:           # the plain L1 map at the tolerance the project holds it to
                assert_close_frac(got_map, ref_map, rtol=1e-4, atol=L1_ATOL, max_bad_frac=1e-4, name="l1[%d]" % s)
            if backward:
                pool.add(s, grads[s], o32["grads"][s], o64["grads"][s])
    if backward:
        pool.check(case["id"])


# ---------------------------------------------------------------------------------------------- part 1: the form matrix
# 6 x 40 x 136, the shape of test_photo_loss_two_frames_and_options: three forward strips (62 + 62 + 12 columns), three backward
# strips (60 + 60 + 16), ragged last strips in y in both directions; four seeds pooled = 1.3e5 pixels, the floor of _pool_seeds.
SHAPE = (6, 40, 136)
SEEDS = (77, 177, 277, 377)

FORMS = [
    # photo_fwd_kernel<3,1,false> + photo_bwd_kernel<3>: noise [B,3,H,W], read as noise[s][((b*NF+f)*H+y)*W+x]
    dict(id="ms-md2", fids=MS),
    # the same kernels in the DepthHints variant: minimum over the frames first, then ONE noise plane
    dict(id="ms-dh", fids=MS, variant="dh"),
    # photo_fwd_kernel<2,2,false> + photo_bwd_kernel<2> with the tie-break noise (the existing two-frame test has none)
    dict(id="two-md2", fids=(0, -1, 1)),
    dict(id="two-dh", fids=(0, -1, 1), variant="dh"),
    # the generic one-frame kernel photo_fwd_kernel<1,2,false> and photo_bwd_kernel<1> / <1,false,true> under the options
    dict(id="one-noautomask", fids=(0, "s"), automask=False),
    dict(id="one-nossim", fids=(0, "s"), no_ssim=True),
    dict(id="one-noautomask-nossim", fids=(0, "s"), automask=False, no_ssim=True),
    dict(id="ms-noautomask", fids=MS, automask=False),
    dict(id="ms-nossim", fids=MS, no_ssim=True),
    dict(id="ms-dh-noautomask", fids=MS, variant="dh", automask=False),    # every pixel counts in the mask
    # noise planes: LARGE noise, an independent N(0, 0.05^2) field per (scale, frame) plane.  The usual randn * 1e-5 moves the
    # selection only inside the excluded tie band; with this one the selection depends on the noise at most pixels, so a wrong
    # plane, frame or scale index is a mass of mismatches away from ties
    dict(id="ms-md2-planes", fids=MS, sigma=0.05),
    dict(id="two-dh-planes", fids=(0, -1, 1), variant="dh", sigma=0.05),
    # a disparity at 1/16 of the frame (6 x 48 x 144; pyramid 1, 2, 4, 16).  A backward strip of R rows touches
    # floor(u + (R - 1) / f) - floor(u) + 2 low-resolution rows, u = (Y0 + 0.5) / f - 0.5: that is R / f + 2 whenever f divides
    # R - 1 -- every f <= 8 at R = 9 and R = 33 -- and at R = 18 the strip origins 18 k never have the residue that needs one more
    # (Y0 mod 4 = 1, Y0 mod 8 = 3).  The (R % f) increment of stage_slots therefore only ever acts at f = 16, R = 9, where a strip
    # at Y0 = 18 spans three rows against 9 / 16 + 2 = 2: this case is what holds it
    dict(id="one-md2-f16", fids=(0, "s"), coarsest=16, shape=(6, 48, 144)),
]


@pytest.mark.parametrize("case", FORMS, ids=[c["id"] for c in FORMS])
def test_form_vs_oracle(case):
    run_case(case, *case.get("shape", SHAPE), SEEDS)


def test_philox_noise_with_three_frames():
    """The in-kernel tie-break noise with three frames (slot (j * NF + f) & 3 of the pixel's draw): seeded; and each frame's
    term is N(0, 1) * 1e-5 of its own.  Only the winning identity frame's draw shows in to_opt, so the three source frames are
    rotated through the three slots under one seed: the same pixels then show slot 0, 1 and 2 in turn."""
    N, ops = _mods()
    B, H, W = SHAPE
    inputs, disps, poses = frames_case(B, H, W, SEEDS[0], MS)
    from oracle import loss_ref
    tgt = inputs[("color", 0, 0)]
    ident = torch.cat([loss_ref.compute_reprojection_loss(inputs[("color", f, 0)], tgt) for f in MS[1:]], 1)
    two, idx = ident.topk(2, dim=1, largest=False)
    # the identity frame that wins by more than the tie width: 6 sigma of the noise (6e-5) cannot change it
    clear = ((two[:, 1] - two[:, 0]) > 2 * PIX_ATOL).cuda()
    winner = idx[:, 0].cuda()
    d_in, d_poses = to_dev(inputs), to_dev(poses)
    dd = [d.cuda() for d in disps]

    def run(order, noise):
        return ops.photometric_smooth_loss(
            d_in[("color", 0, 0)], [d_in[("color", f, 0)] for f in order],
            [d_in["stereo_T"] if f == "s" else d_poses[f] for f in order], d_in[("K", 0)], d_in[("inv_K", 0)], dd,
            [d_in[("color", 0, s)] for s in range(4)], noise=noise, want_to_opt=True)
    frames = list(MS[1:])
    z = {}      # (frame index in MS[1:], slot) -> its draws / 1e-5 on the pixels where that frame's identity term wins
    keep = [clear.clone() for _ in range(3)]
    runs = []
    for r in range(3):
        order = frames[r:] + frames[:r]         # frame i sits in slot (i - r) % 3
        base = run(order, None)
        torch.manual_seed(123)
        a = run(order, "philox")
        torch.manual_seed(123)
        b = run(order, "philox")
        assert torch.equal(a.fin, b.fin) and torch.equal(a.sel.packed, b.sel.packed) and torch.equal(a.to_opt[0], b.to_opt[0])
        if r == 0:
            c = run(order, "philox")            # the next draw differs
            assert not torch.equal(a.to_opt[0], c.to_opt[0])
            assert abs(a.fin[N.FIN_LOSS].item() - base.fin[N.FIN_LOSS].item()) < 1e-5 * abs(base.fin[N.FIN_LOSS].item())
        runs.append((a, base))
        for i in range(3):
            keep[i] &= (a.sel[0] == 0) & (base.sel[0] == 0) & (winner == i)
    for r, (a, base) in enumerate(runs):
        for i in range(3):
            z[(i, (i - r) % 3)] = ((a.to_opt[0] - base.to_opt[0])[keep[i]] / 1e-5).double().cpu()
    for i in range(3):
        assert keep[i].sum().item() >= 300, ("too few pixels where identity frame %d wins" % i, keep[i].sum().item())
        for slot in range(3):
            v = z[(i, slot)]
            print("identity frame %d in slot %d: %d pixels, mean %.3f std %.3f max %.2f" % (i, slot, v.numel(), v.mean(), v.std(),
                                                                                       v.abs().max()))
            # the moment bounds of test_philox_noise_is_tiny_and_seeded, per frame
            assert abs(v.mean().item()) < 0.2 and 0.7 < v.std().item() < 1.3 and v.abs().max().item() < 6
        # the three frames' draws at a pixel are three different numbers (one draw read three times would give equal ones).
        # They are seen as differences of fp32 maps whose values are below 1, i.e. on a grid of at most 2^-24 / 1e-5 = 6e-3
        # sigma: two independent normals fall on the same grid point with probability <= 6e-3 / (2 sqrt(pi)) = 1.7e-3 ...
        for s0, s1 in ((0, 1), (0, 2), (1, 2)):
            v0, v1 = z[(i, s0)], z[(i, s1)]
            assert (v0 != v1).double().mean().item() > 0.99
            # ... and independent ones: |correlation| of n pairs of independent normals is below 5 / sqrt(n) (5 sigma)
            corr = float(((v0 - v0.mean()) * (v1 - v1.mean())).mean() / (v0.std() * v1.std()))
            assert abs(corr) < 5.0 / v0.numel() ** 0.5, (i, s0, s1, corr)


POSE_FORMS = [
    dict(id="ms-all", fids=MS, pose=(-1, 1, "s")),            # photo_bwd_kernel<3,true>: cam_T_cam of -1 and +1, and stereo_T
    dict(id="ms-all-dh", fids=MS, pose=(-1, 1, "s"), variant="dh"),
    dict(id="one-mono", fids=(0, -1), pose=(-1,)),            # photo_bwd_kernel<1,true>
    dict(id="ms-mono-only", fids=MS, pose=(-1, 1)),           # stereo_T needs no gradient: its sums are formed and dropped
]


@pytest.mark.parametrize("case", POSE_FORMS, ids=[c["id"] for c in POSE_FORMS])
def test_pose_gradient_forms_vs_fp64_oracle(case):
    """d loss / d T of every source frame with one and with three frames, with the statistic and the bound of
    test_pose_gradient_vs_fp64_oracle: pooled over six seeds, e_h <= 1.5 e_o + 1e-4 |g64|; disparity gradients unchanged against
    the launch without pose sums; bitwise reproducible."""
    N, ops = _mods()
    B, H, W = 2, 40, 136
    fids, variant, want = case["fids"], case.get("variant", "md2"), case["pose"]
    e_h = e_o = n64 = 0.0
    for seed in (31, 131, 231, 331, 431, 531):
        inputs, disps, poses = frames_case(B, H, W, seed, fids)
        kw = dict(variant=variant, pose_grad=want)
        g32 = oracle_pass(inputs, disps, poses, fids, None, dtype=torch.float32, **kw)["pose_grads"]
        g64 = oracle_pass(inputs, disps, poses, fids, None, dtype=torch.float64, **kw)["pose_grads"]
        d_in, d_poses = to_dev(inputs), to_dev(poses)

        def hip(pose):
            Ts = {f: (d_in["stereo_T"] if f == "s" else d_poses[f]).detach().clone().requires_grad_(pose and f in want)
                  for f in fids[1:]}
            dd = [d.cuda().requires_grad_(True) for d in disps]
            out = ops.photometric_smooth_loss(d_in[("color", 0, 0)], [d_in[("color", f, 0)] for f in fids[1:]],
                                              [Ts[f] for f in fids[1:]], d_in[("K", 0)], d_in[("inv_K", 0)], dd,
                                              [d_in[("color", 0, s)] for s in range(4)], noise=None, variant=variant)
            out.fin[N.FIN_LOSS].backward()
            return {f: Ts[f].grad for f in fids[1:]}, [d.grad for d in dd]
        gT, gd = hip(True)
        gT2, gd2 = hip(True)
        assert all(torch.equal(gT[f], gT2[f]) for f in want) and all(torch.equal(a_, b_) for a_, b_ in zip(gd, gd2))
        assert all(gT[f] is None for f in fids[1:] if f not in want)
        none, gd0 = hip(False)
        assert all(v is None for v in none.values())
        for a_, b_ in zip(gd, gd0):        # the pose variant of the kernel computes the same disparity gradients
            torch.testing.assert_close(a_, b_, rtol=1e-4, atol=1e-6 * float(b_.abs().max()))    # (another instruction order)
        for f in want:
            got, r32, r64 = gT[f], g32[f], g64[f]
            assert float(got[:, 3].abs().max()) == 0.0            # (K T)[:3,:] does not depend on T's last row
            assert float(r64.abs().max()) > 0
            e_h += float((got.cpu().double() - r64).pow(2).sum())
            e_o += float((r32.double() - r64).pow(2).sum())
            n64 += float(r64.pow(2).sum())
    e_h, e_o, n64 = e_h ** 0.5, e_o ** 0.5, n64 ** 0.5
    print("%s: pose gradient rel-L2 vs fp64  hip %.3g  oracle fp32 %.3g" % (case["id"], e_h / n64, e_o / n64))
    assert n64 > 0 and e_h <= 1.5 * e_o + 1e-4 * n64, (e_h / n64, e_o / n64)


# ------------------------------------------------------------------------------- part 2: the strip heights the workload runs
# 40 x 64, one stereo frame, tensor noise: two strips in x (62 + 2 forward, 60 + 4 backward), so photo_combine_kernel adds
# overlapping staging blocks on both axes, and every strip column ends in a ragged strip.  pick_rows leaves 8 / 9 rows only once a
# launch has 8192 forward / 4096 backward strips, hence the batches; rows = (forward R, backward R), pinned by _pin_rows.
# The oracle of these 1.8 to 5.2 million pixels runs on the device, float32 and float64: the same oracle/loss_ref.py code,
# held to its CPU float64 run by test_device_fp64_oracle_matches_the_cpu_fp64_oracle.
ROWS = [
    dict(id="B688-fw8-bw18", fids=(0, "s"), B=688, rows=(8, 18), backward=True),       # backward strips of 18, 18, 4 rows
    dict(id="B1368-fw16-bw33", fids=(0, "s"), B=1368, rows=(16, 33), backward=True),   # forward 16, 16, 8; backward 33, 7
    dict(id="B1368-fw16-bw33-dh", fids=(0, "s"), B=1368, rows=(16, 33), backward=True, variant="dh"),
    dict(id="B2048-fw32", fids=(0, "s"), B=2048, rows=(32, 33), backward=False),       # forward 32, 8
]


@pytest.mark.parametrize("case", ROWS, ids=[c["id"] for c in ROWS])
def test_strip_heights_vs_oracle(case):
    run_case(case, case["B"], 40, 64, (91,), oracle_device="cuda", backward=case["backward"])


@pytest.mark.parametrize("variant", ["md2", "dh"])
def test_device_fp64_oracle_matches_the_cpu_fp64_oracle(variant):
    """The float64 oracle on the device -- the anchor of test_strip_heights_vs_oracle -- against the same code on the CPU, on
    the three-frame cases of part 1, both variants (part 2 leans on both): losses, maps and disparity gradients to 1e-12 x max
    (float64 rounds at 1.1e-16; the gate is eight orders below anything fp32 can show and does not involve the kernel under
    test)."""
    B, H, W = SHAPE
    inputs, disps, poses = frames_case(B, H, W, SEEDS[0], MS)
    noise = tie_noise(B, 3 if variant == "md2" else 1, H, W, SEEDS[0])
    cpu = oracle_pass(inputs, disps, poses, MS, noise, variant=variant, dtype=torch.float64)
    dev = oracle_pass(inputs, disps, poses, MS, noise, variant=variant, dtype=torch.float64, device="cuda")
    for key, ref in cpu["losses"].items():
        assert abs(dev["losses"][key].item() - ref.item()) <= 1e-12 * abs(ref.item()), key
    for s in range(4):
        for name, got, ref in (("to_opt", dev["maps"][s], cpu["maps"][s]), ("grad", dev["grads"][s], cpu["grads"][s])):
            err = float((got.cpu() - ref).abs().max())
            print("%s scale %d %s: max |device - cpu| %.3g of max %.3g" % (variant, s, name, err, float(ref.abs().max())))
            assert err <= 1e-12 * float(ref.abs().max()), (s, name, err)
