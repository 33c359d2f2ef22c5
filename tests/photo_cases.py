"""Inputs and oracle passes of K1's launch forms (tests/test_gpu_photo_forms.py, tests/test_gpu_kernels.py): source frames, poses,
tie-break noise, one pass of oracle/loss_ref.py in a given dtype on a given device, and the selection codes the test forms
itself from the oracle's candidate stack.  Nothing here touches the HIP library, so the conditions a case puts on its inputs
(tie band, every candidate wins somewhere) can be checked without a GPU."""
import torch
import torch.nn.functional as F

from oracle import loss_ref, synth

# Per-pixel SSIM values carry fp32 conditioning noise: sigma = E[x^2] - mu^2 cancels ~0.25 - 0.25 down to
# ~1e-3, so one ulp of the window sums moves (1 - SSIM)/2 by ~1e-5.  Scalars (means over >= 6k pixels) are
# held to 2e-5 relative; per-pixel maps to 5e-5 absolute.
PIX_ATOL = 5e-5
L1_ATOL = 5e-6      # --no_ssim: the plain L1 map has no such cancellation (test_photo_loss_two_frames_and_options)


def general_pose(B, seed):
    """A different rigid transform per sample: rotations of up to ~1 degree about all three axes + a translation."""
    g = torch.Generator().manual_seed(seed)
    ang = (torch.rand(B, 3, generator=g, dtype=torch.float64) - 0.5) * 0.03
    T = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    for b in range(B):
        cx, cy, cz = torch.cos(ang[b])
        sx, sy, sz = torch.sin(ang[b])
        Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
        Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
        Rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
        T[b, :3, :3] = Rz @ Ry @ Rx
    T[:, 0, 3], T[:, 1, 3], T[:, 2, 3] = 0.05, 0.01, -0.02
    T[:, :3, 3] += (torch.rand(B, 3, generator=g, dtype=torch.float64) - 0.5) * 0.02
    return T


def frames_case(B, H, W, seed, fids, coarsest=8):
    """synth.make_loss_case + the monocular frames of ``fids``: a rolled target (frame -1 two pixels one way, frame +1 the other)
    blended with fresh texture, each with a general pose rounded to float32.  ``coarsest`` = 16: the last scale's disparity and
    colour at 1/16 of the frame, the coarsest the kernel accepts (a disparity pyramid of 1, 2, 4, 16).
    Returns (inputs, disps, {frame: pose})."""
    inputs, disps = synth.make_loss_case(B, H, W, seed)
    if coarsest != 8:
        g16 = torch.Generator().manual_seed(seed + 16)
        inputs[("color", 0, 3)] = F.avg_pool2d(inputs[("color", 0, 0)], coarsest).contiguous()
        disps[3] = synth.smooth_field(B, H // coarsest, W // coarsest, g16, 0.01, 0.35, k=3)
    g = torch.Generator().manual_seed(seed + 1)
    poses = {}
    for f in fids[1:]:
        if f == "s":
            continue
        inputs[("color", f, 0)] = (0.8 * torch.roll(inputs[("color", 0, 0)], 2 * f, 3) +
                                   0.2 * synth.kitti_like(B, 3, H, W, g)).contiguous()
        poses[f] = general_pose(B, seed + (2 if f == -1 else 3)).float()
    return inputs, disps, poses


def tie_noise(B, planes, H, W, seed, sigma=1e-5):
    """{scale: [B, planes, H, W]}: an independent N(0, sigma^2) field per (scale, frame) plane, already scaled (the reference:
    randn * 1e-5, MD2/trainer.py:642-645)."""
    g = torch.Generator().manual_seed(seed + 100)
    return {s: torch.randn(B, planes, H, W, generator=g) * sigma for s in range(4)}


def oracle_pass(inputs, disps, poses, fids, noise, variant="md2", automask=True, no_ssim=False, dtype=torch.float32,
                device="cpu", backward=True, pose_grad=()):
    """One pass of oracle/loss_ref.py: compute_losses for the plain form, compute_losses_options(_dh) for the option branches.
    ``pose_grad``: frames ("s" included) whose transform is a leaf.  Returns a dict: losses, maps, ins, outs, grads (one per
    scale, or None), pose_grads {frame: grad}."""
    ins = {k: v.to(device=device, dtype=dtype) for k, v in inputs.items()}
    outs, leaves, pose_leaves = {}, [], {}
    for f in fids[1:]:
        T = ins["stereo_T"] if f == "s" else poses[f].to(device=device, dtype=dtype)
        if f in pose_grad:
            T = T.detach().clone().requires_grad_(True)
            pose_leaves[f] = T
        if f == "s":
            ins["stereo_T"] = T
        else:
            outs[("cam_T_cam", 0, f)] = T
    for s, d in enumerate(disps):
        d = d.detach().clone().to(device=device, dtype=dtype).requires_grad_(backward and not pose_grad)
        leaves.append(d)
        outs[("disp", s)] = d
    nz = None if noise is None or not automask else {s: z.to(device=device, dtype=dtype) for s, z in noise.items()}
    loss_ref.generate_images_pred(ins, outs, frame_ids=fids)
    if automask and not no_ssim:
        losses, maps = loss_ref.compute_losses(ins, outs, frame_ids=fids, noise=nz, variant=variant)
    elif variant == "md2":
        losses, maps = loss_ref.compute_losses_options(ins, outs, frame_ids=fids, noise=nz, automask=automask, no_ssim=no_ssim)
    else:
        assert not no_ssim, "DepthHints has no --no_ssim"
        losses, maps = loss_ref.compute_losses_options_dh(ins, outs, frame_ids=fids, noise=nz, automask=automask)
    if backward:
        losses["loss"].backward()
    return dict(losses=losses, maps=maps, ins=ins, outs=outs, noise=nz, grads=[l.grad for l in leaves],
                pose_grads={f: t.grad for f, t in pose_leaves.items()})


def candidate_stack(o, fids, s, variant="md2", automask=True, no_ssim=False):
    """The candidates the per-pixel minimum of scale ``s`` runs over, in the order of the reference's torch.cat, from the pass
    ``o`` of oracle_pass, and the selection code of each (0: an identity term, 1 + f: the reprojection of source frame f).
    md2: [identity_f + noise_f ..., reprojection_f ...] (MD2/trainer.py:642-654); dh: [reprojection_f ..., min_f identity_f +
    noise] -- its argmin is over [min reprojection, identity] with the reprojection first (DH/trainer.py:693-703), and the first
    of equal frames wins either minimum; without auto-masking the reprojections alone."""
    ins, outs = o["ins"], o["outs"]
    tgt = ins[("color", 0, 0)]
    nf = len(fids) - 1
    with torch.no_grad():
        reproj = torch.cat([loss_ref.compute_reprojection_loss(outs[("color", f, s)], tgt, no_ssim) for f in fids[1:]], 1)
        if not automask:
            return reproj, list(range(1, nf + 1))
        ident = torch.cat([loss_ref.compute_reprojection_loss(ins[("color", f, 0)], tgt, no_ssim) for f in fids[1:]], 1)
        if variant == "md2":
            if o["noise"] is not None:
                ident = ident + o["noise"][s]
            return torch.cat([ident, reproj], 1), [0] * nf + list(range(1, nf + 1))
        ident = ident.min(1, keepdim=True)[0]
        if o["noise"] is not None:
            ident = ident + o["noise"][s]
        return torch.cat([reproj, ident], 1), list(range(1, nf + 1)) + [0]


def selection_reference(stack, codes, width):
    """(code [B,H,W]: the code of the first smallest candidate, as torch.min picks it; tie [B,H,W]: the two smallest candidates
    are closer than ``width``; wins: the share of the pixels each candidate wins)."""
    C = stack.shape[1]
    idx = stack.min(1)[1]
    code = torch.tensor(codes, device=stack.device, dtype=torch.float32)[idx]
    if C == 1:
        tie = torch.zeros_like(idx, dtype=torch.bool)
    else:
        two = stack.topk(2, dim=1, largest=False)[0]
        tie = (two[:, 1] - two[:, 0]) < width
    wins = torch.bincount(idx.reshape(-1), minlength=C).double() / idx.numel()
    return code, tie, wins
