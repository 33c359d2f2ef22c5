"""Autograd-aware Python faces of the HIP kernels in libdmh_hip.so.

PyTorch is plumbing here: it owns device memory, streams and the autograd graph; every op
below is one or a few launches of hand-written gfx950 kernels through the C ABI
(include/dmh_hip.h).  There is no eager/CPU fallback: CPU tensors raise RuntimeError.
"""
import contextlib
import ctypes as C
import functools
import os
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _native as N

LossOut = namedtuple("LossOut", ["fin", "sel", "to_opt"])

# Optional per-launch HIP-event timing of the K1 kernels (bench.py's roofline figure): a dict
# name -> list of (start, end) torch.cuda.Event pairs recorded on the launch stream, or None (off).
_profile = None
_profile_only = None


def enable_profile(on=True, only=None):
    """HIP-event timing of the instrumented launches.  ``only``: tuple of name prefixes to time (the others launch
    untouched) -- an event pair adds ~10 us of dispatch latency around a launch, so a timed region should carry events
    on the kernels it reports and nothing else."""
    global _profile, _profile_only
    _profile = {} if on else None
    _profile_only = tuple(only) if (on and only) else None


def profile_ms():
    """Average launch duration in ms per instrumented kernel (synchronises)."""
    if not _profile:
        return {}
    torch.cuda.synchronize()
    return {k: sum(e[0].elapsed_time(e[1]) for e in v) / len(v) for k, v in _profile.items() if v}


def profile_bytes():
    """Per instrumented kernel: (launches, total ms, total algorithmic bytes, total direct-convolution flops) -- for
    kernels whose shape varies from launch to launch."""
    if not _profile:
        return {}
    torch.cuda.synchronize()
    return {k: (len(v), sum(e[0].elapsed_time(e[1]) for e in v), sum(e[2] for e in v), sum(e[3] for e in v))
            for k, v in _profile.items() if v}


def profiling_every_launch():
    """True while enable_profile(True) without ``only`` is in force: every instrumented launch carries an event pair (bench.py's
    one fully instrumented step).  Events cannot be read back from a captured HIP graph, so the attack runs that step eagerly."""
    return _profile is not None and _profile_only is None


def _timed(name, launch, nbytes=0, flops=0):
    if _profile is None or (_profile_only is not None and not name.startswith(_profile_only)):
        return launch()
    if torch.cuda.is_current_stream_capturing():      # an event recorded into a graph has no time stamp to read
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = launch()
    e1.record()
    _profile.setdefault(name, []).append((e0, e1, nbytes, flops))
    return rc


def _philox(device, count):
    """(seed, offset) for the in-kernel tie-break noise, drawn from torch's CUDA generator state so
    that torch.manual_seed() makes runs reproducible; the generator offset is advanced past the
    ``count`` counters this call consumes."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    seed, off = gen.initial_seed(), gen.get_offset()
    gen.set_offset(off + ((count + 3) // 4) * 4)
    return seed & 0xFFFFFFFFFFFFFFFF, off


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _need_cuda(t):
    """A CPU operand (``t``: a tensor or a torch.device) is an error, never another code path."""
    device = t if isinstance(t, torch.device) else t.device
    if device.type != "cuda":
        raise RuntimeError("libdmh_hip ops need CUDA (ROCm) tensors; got device %s -- there is no CPU path" % device)


def _photo_args(cfg, target, sources, Ts, K, inv_K, disps, noises, hint=None):
    a = N.PhotoArgs()
    B, _, H, W = target.shape
    if hint is not None:
        for t_ in hint:
            if tuple(t_.shape) != (B, 1, H, W):
                raise RuntimeError("photometric loss: depth_hint / depth_hint_mask must be [B,1,H,W]")
        a.depth_hint, a.depth_hint_mask = N.ptr(hint[0]), N.ptr(hint[1])
    a.target = N.ptr(target)
    for f, (s_, t_) in enumerate(zip(sources, Ts)):
        if tuple(s_.shape) != (B, 3, H, W) or tuple(t_.shape) != (B, 4, 4):
            raise RuntimeError("photometric loss: source/T shape mismatch %s %s" % (tuple(s_.shape), tuple(t_.shape)))
        a.source[f] = N.ptr(s_)
        a.T[f] = N.ptr(t_)
    if tuple(K.shape) != (B, 4, 4) or tuple(inv_K.shape) != (B, 4, 4):
        raise RuntimeError("photometric loss: K / inv_K must be [B,4,4]")
    a.K, a.inv_K = N.ptr(K), N.ptr(inv_K)
    for s, d in enumerate(disps):
        if d.dim() != 4 or d.shape[0] != B or d.shape[1] != 1:
            raise RuntimeError("photometric loss: disp[%d] must be [B,1,Hs,Ws]" % s)
        a.disp[s] = N.ptr(d)
        a.Hs[s], a.Ws[s] = d.shape[2], d.shape[3]
    a.B, a.H, a.W = B, H, W
    a.num_frames, a.num_scales = len(sources), len(disps)
    a.min_depth, a.max_depth = cfg["min_depth"], cfg["max_depth"]
    a.variant = N.VARIANT_MD2 if cfg["variant"] == "md2" else N.VARIANT_DH
    a.automask, a.no_ssim = int(cfg["automask"]), int(cfg["no_ssim"])
    a.noise_mode = cfg["noise_mode"]
    if cfg["noise_mode"] == N.NOISE_TENSOR:
        nf = len(sources) if cfg["variant"] == "md2" else 1
        for s, z in enumerate(noises):
            if tuple(z.shape) != (B, nf, H, W):
                raise RuntimeError("photometric loss: noise[%d] must be [B,%d,H,W]" % (s, nf))
            a.noise[s] = N.ptr(z)
    a.seed, a.offset = cfg.get("seed", 0), cfg.get("offset", 0)
    return a


def _smooth_args(disps, colors):
    a = N.SmoothArgs()
    B = disps[0].shape[0]
    for s, (d, c) in enumerate(zip(disps, colors)):
        if tuple(c.shape) != (B, 3, d.shape[2], d.shape[3]):
            raise RuntimeError("smoothness: color[%d] %s does not match disp %s" % (s, tuple(c.shape), tuple(d.shape)))
        a.disp[s], a.color[s] = N.ptr(d), N.ptr(c)
        a.Hs[s], a.Ws[s] = d.shape[2], d.shape[3]
    a.B, a.num_scales = B, len(disps)
    return a


def photo_smooth_fwd_launch(cfg, target, sources, Ts, K, inv_K, disps, colors, noises=(), hint=None):
    """K1 + K2 + finalise on checked, contiguous tensors: (fin [FIN_SIZE], packed selection bytes [B,H,W], smoothness statistics
    [NS,B,2], to_opt: NS tensors [B,H,W] with cfg["want_to_opt"], else NS times None)."""
    lib = N.lib()
    B, _, H, W = target.shape
    dev = target.device
    NS = len(disps)
    a = _photo_args(cfg, target, sources, Ts, K, inv_K, disps, noises, hint)
    sm = _smooth_args(disps, colors)
    sel = torch.empty((B, H, W), device=dev, dtype=torch.uint8)    # 2 bits per scale: 0 identity, 1+f frame f
    to_opt = [torch.empty((B, H, W), device=dev, dtype=torch.float32) if cfg["want_to_opt"] else None
              for _ in range(NS)]
    pp = torch.empty(lib.dmh_photo_partials_size(B, H, W, NS), device=dev, dtype=torch.float32)
    sp = torch.empty(lib.dmh_smooth_partials_size(C.byref(sm)), device=dev, dtype=torch.float32)
    fin = torch.empty(N.FIN_SIZE, device=dev, dtype=torch.float32)
    sstats = torch.empty((NS, B, 2), device=dev, dtype=torch.float32)
    st = N.stream()
    optp = N.ptr_array(to_opt)
    N.check(_timed("photo_fwd", lambda: lib.dmh_photo_loss_fwd(C.byref(a), N.ptr(sel), optp, N.ptr(pp), st)))
    N.check(lib.dmh_smooth_loss_fwd(C.byref(sm), N.ptr(sp), st))
    N.check(lib.dmh_loss_finalize(N.ptr(pp), N.ptr(sp), B, H, W, C.byref(sm), a.variant, cfg["smooth_wt"],
                                  N.ptr(fin), N.ptr(sstats), st))
    return fin, sel, sstats, to_opt


def photo_smooth_bwd_launch(cfg, target, sources, Ts, K, inv_K, disps, colors, hint, fin, sel, sstats, g_fin, want_pose):
    """The backward of photo_smooth_fwd_launch: (g_disp: one per scale, g_T: per source frame [B,4,4] where ``want_pose[f]``,
    else None)."""
    lib = N.lib()
    dev = target.device
    F, NS = len(sources), len(disps)
    gvec = _c(g_fin.to(torch.float32))
    a = _photo_args(dict(cfg, noise_mode=N.NOISE_NONE), target, sources, Ts, K, inv_K, disps, (), hint)
    sm = _smooth_args(disps, colors)
    st = N.stream()
    g_disp = [torch.empty_like(d) for d in disps]
    stage = torch.empty(lib.dmh_photo_stage_size(C.byref(a)), device=dev, dtype=torch.float32)
    gp = N.ptr_array(g_disp)
    g_T = [None] * F
    if any(want_pose):
        # monocular frames: K1's backward also leaves twelve sums per (scale, strip, frame), from which
        # d loss / d P_f (P_f = (K T_f)[:3,:]) and d loss / d T_f = K[:3,:]^T dP_f follow (include/dmh_hip.h)
        B = target.shape[0]
        part = torch.empty(lib.dmh_photo_pose_partials_size(C.byref(a)), device=dev, dtype=torch.float32)
        N.check(_timed("photo_bwd", lambda: lib.dmh_photo_loss_bwd_pose(C.byref(a), N.ptr(sel), N.ptr(gvec), N.ptr(fin),
                                                                       N.ptr(stage), gp, N.ptr(part), st)))
        sums = part.view(NS, B, -1, F, 3, 4).double().sum((0, 2))               # [B, F, 3, (S_i0, S_i1, S_i2, s_i)]
        Kd, iKd = K.double(), inv_K.double()
        for f in range(F):
            if not want_pose[f]:
                continue
            dP = torch.cat([torch.matmul(sums[:, f, :, :3], iKd[:, :3, :3].transpose(1, 2)), sums[:, f, :, 3:4]], 2)
            g_T[f] = torch.matmul(Kd[:, :3, :].transpose(1, 2), dP).to(Ts[f].dtype)     # [B, 4, 4]
    else:
        N.check(_timed("photo_bwd", lambda: lib.dmh_photo_loss_bwd(C.byref(a), N.ptr(sel), N.ptr(gvec), N.ptr(fin),
                                                                  N.ptr(stage), gp, st)))
    N.check(lib.dmh_smooth_loss_bwd(C.byref(sm), N.ptr(gvec), N.ptr(sstats), cfg["smooth_wt"], gp, 1, st))
    return g_disp, g_T


class _PhotoSmoothLoss(torch.autograd.Function):
    """K1 + K2 + finalise.  Tensor args: target, K, inv_K, then F sources, F Ts, NS colors,
    (NS noises), NS disps."""

    @staticmethod
    def forward(ctx, cfg, target, K, inv_K, *rest):
        F, NS = cfg["F"], cfg["NS"]
        sources, Ts = rest[:F], rest[F:2 * F]
        colors = rest[2 * F:2 * F + NS]
        pos = 2 * F + NS
        noises = ()
        if cfg["noise_mode"] == N.NOISE_TENSOR:
            noises = rest[pos:pos + NS]
            pos += NS
        disps = rest[pos:pos + NS]
        hint = tuple(rest[pos + NS:pos + NS + 2]) if cfg["hints"] else None
        fin, sel, sstats, to_opt = photo_smooth_fwd_launch(cfg, target, sources, Ts, K, inv_K, disps, colors, noises, hint)
        ctx.cfg = cfg
        ctx.save_for_backward(target, K, inv_K, fin, sstats, sel, *sources, *Ts, *colors, *disps, *(hint or ()))
        outs = [fin, sel] + [t for t in to_opt if t is not None]
        ctx.mark_non_differentiable(*outs[1:])
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_fin, *unused):
        cfg = ctx.cfg
        F, NS = cfg["F"], cfg["NS"]
        sv = ctx.saved_tensors
        target, K, inv_K, fin, sstats, sel = sv[:6]
        sources, Ts = sv[6:6 + F], sv[6 + F:6 + 2 * F]
        colors = sv[6 + 2 * F:6 + 2 * F + NS]
        disps = sv[6 + 2 * F + NS:6 + 2 * F + 2 * NS]
        hint = tuple(sv[6 + 2 * F + 2 * NS:6 + 2 * F + 2 * NS + 2]) if cfg["hints"] else None
        want_pose = [bool(ctx.needs_input_grad[4 + F + f]) for f in range(F)]      # cam_T_cam of source frame f
        g_disp, g_T = photo_smooth_bwd_launch(cfg, target, sources, Ts, K, inv_K, disps, colors, hint, fin, sel, sstats, g_fin,
                                              want_pose)
        n_tail = NS + (NS if cfg["noise_mode"] == N.NOISE_TENSOR else 0)
        return ((None, None, None, None) + (None,) * F + tuple(g_T) + (None,) * n_tail + tuple(g_disp)
                + ((None, None) if cfg["hints"] else ()))


class SelectionMaps(object):
    """The per-scale selection maps of the fused loss, unpacked on demand from the packed byte map the kernel writes
    (2 bits per scale): ``maps[s]`` is a float [B,H,W] tensor, 0 where the identity term was chosen, 1 + f where the
    reprojection of source frame f was (== outputs["identity_selection/s"] for one source frame,
    MD2/trainer.py:656-658).  Nothing is materialised until a scale is asked for."""

    def __init__(self, packed, num_scales):
        self.packed, self.num_scales, self._cache = packed, num_scales, {}

    def __len__(self):
        return self.num_scales

    def __getitem__(self, s):
        if not 0 <= s < self.num_scales:
            raise IndexError(s)
        if s not in self._cache:
            out = torch.empty(self.packed.shape, device=self.packed.device, dtype=torch.float32)
            N.check(N.lib().dmh_unpack_selection(N.ptr(self.packed), self.packed.numel(), int(s), N.ptr(out), N.stream()))
            self._cache[s] = out
        return self._cache[s]

    def __iter__(self):
        return (self[s] for s in range(self.num_scales))


def photometric_smooth_loss(target, sources, Ts, K, inv_K, disps, colors, min_depth=0.1, max_depth=100.0,
                            variant="md2", automask=True, no_ssim=False, smooth_wt=1e-3, noise="philox",
                            want_to_opt=False, depth_hint=None, depth_hint_mask=None):
    """Fused photometric-reprojection + SSIM + auto-mask + smoothness loss over all scales.

    target [B,3,H,W]; sources / Ts: one per non-target frame; disps[s] [B,1,H/2^s,W/2^s];
    colors[s] = inputs[("color",0,s)].  ``noise``: "philox" (in-kernel randn*1e-5, the reference's
    tie-break of MD2/trainer.py:642-645), None, or a list of NS already-scaled tensors.
    ``depth_hint`` / ``depth_hint_mask`` [B,1,H,W]: DepthHints' --use_depth_hints (DH/trainer.py:510-525,629-636,
    700-725; variant "dh", one source frame): fin[FIN_HINT_S+s] is depth_hint_loss/s (already part of loss/s) and
    sel[s] == 3 marks the pixels where the hint won the argmin (outputs["depth_hint_pixels/s"]).
    Returns LossOut(fin, sel, to_opt): fin[FIN_*] is differentiable w.r.t. the disparities; sel is a SelectionMaps
    (sel[s] unpacks scale s on demand).
    """
    F, NS = len(sources), len(disps)
    N.ptr(target)   # rejects CPU tensors up front ("no CPU path") before any CUDA-only call below
    if not (1 <= F <= 3 and 1 <= NS <= N.MAX_SCALES):
        raise RuntimeError("photometric loss supports 1..3 source frames and 1..4 scales")
    if variant not in ("md2", "dh"):
        raise RuntimeError("variant must be 'md2' or 'dh'")
    B, _, H, W = target.shape
    if (depth_hint is None) != (depth_hint_mask is None):
        raise RuntimeError("depth_hint and depth_hint_mask go together")
    cfg = dict(F=F, NS=NS, min_depth=float(min_depth), max_depth=float(max_depth), variant=variant,
               automask=bool(automask), no_ssim=bool(no_ssim), smooth_wt=float(smooth_wt), want_to_opt=want_to_opt,
               hints=depth_hint is not None)
    noises = ()
    if noise is None or not automask:
        cfg["noise_mode"] = N.NOISE_NONE
    elif isinstance(noise, str):
        cfg["noise_mode"] = N.NOISE_PHILOX
        cfg["seed"], cfg["offset"] = _philox(target.device, NS * B * F * H * W)
    else:
        cfg["noise_mode"] = N.NOISE_TENSOR
        noises = tuple(_c(z) for z in noise)
    args = (_c(target), _c(K), _c(inv_K)) + tuple(_c(s) for s in sources) + tuple(_c(t) for t in Ts) + \
        tuple(_c(c) for c in colors) + noises + tuple(_c(d) for d in disps)
    if depth_hint is not None:
        args += (_c(depth_hint), _c(depth_hint_mask))
    outs = _PhotoSmoothLoss.apply(cfg, *args)
    fin, sel = outs[0], SelectionMaps(outs[1], NS)
    to_opt = list(outs[2:]) if want_to_opt else [None] * NS
    return LossOut(fin, sel, to_opt)


class _WarpView(torch.autograd.Function):
    @staticmethod
    def forward(ctx, source, disp, K, inv_K, T, H, W, min_depth, max_depth):
        lib = N.lib()
        B = source.shape[0]
        Hs, Ws = disp.shape[2], disp.shape[3]
        dev = source.device
        depth = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
        sample = torch.empty((B, H, W, 2), device=dev, dtype=torch.float32)
        color = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
        N.check(lib.dmh_warp_view_fwd(N.ptr(source), N.ptr(disp), N.ptr(K), N.ptr(inv_K), N.ptr(T), B, H, W, Hs, Ws,
                                      min_depth, max_depth, N.ptr(depth), N.ptr(sample), N.ptr(color), N.stream()))
        ctx.save_for_backward(source, disp, K, inv_K, T)
        ctx.geo = (H, W, min_depth, max_depth)
        ctx.mark_non_differentiable(sample)
        return depth, sample, color

    @staticmethod
    def backward(ctx, g_depth, g_sample, g_color):
        source, disp, K, inv_K, T = ctx.saved_tensors
        H, W, min_depth, max_depth = ctx.geo
        lib = N.lib()
        B = source.shape[0]
        Hs, Ws = disp.shape[2], disp.shape[3]
        g_up = torch.empty((B, H, W), device=source.device, dtype=torch.float32)
        gc = _c(g_color) if g_color is not None else None
        gd = _c(g_depth) if g_depth is not None else None
        st = N.stream()
        N.check(lib.dmh_warp_view_bwd(N.ptr(source), N.ptr(disp), N.ptr(K), N.ptr(inv_K), N.ptr(T), B, H, W, Hs, Ws,
                                      min_depth, max_depth, N.ptr(gc), N.ptr(gd), N.ptr(g_up), st))
        if (Hs, Ws) == (H, W):
            g = g_up.view(B, 1, H, W)
        else:
            g = torch.empty_like(disp)
            N.check(lib.dmh_upsample_bilinear_adjoint(N.ptr(g_up), N.ptr(g), B, H, W, Hs, Ws, 0, st))
        return None, g, None, None, None, None, None, None, None


def warp_view(source, disp, K, inv_K, T, H, W, min_depth=0.1, max_depth=100.0):
    """One (scale, frame) body of generate_images_pred (MD2/trainer.py:481-519):
    returns (depth [B,1,H,W], sample grid [B,H,W,2], warped colour [B,3,H,W])."""
    return _WarpView.apply(_c(source), _c(disp), _c(K), _c(inv_K), _c(T), int(H), int(W), float(min_depth),
                           float(max_depth))


def ssim_map_fwd_launch(x, y):
    """clamp((1 - SSIM(x, y)) / 2, 0, 1) per channel with 3x3 reflection-padded means (MD2/layers.py:223-253): K1's window sums
    stand-alone, on contiguous tensors."""
    if x.dim() != 4 or x.shape != y.shape:
        raise RuntimeError("ssim_map: x and y must be [B,C,H,W] of the same shape")
    B, Cc, H, W = x.shape
    out = torch.empty_like(x)
    N.check(N.lib().dmh_ssim_map(N.ptr(x), N.ptr(y), B * Cc, H, W, N.ptr(out), N.stream()))
    return out


def ssim_map_bwd_launch(x, y, g_out):
    B, Cc, H, W = x.shape
    ws = torch.empty(5 * x.numel(), device=x.device, dtype=torch.float32)
    g_x, g_y = torch.empty_like(x), torch.empty_like(y)
    N.check(N.lib().dmh_ssim_map_bwd(N.ptr(x), N.ptr(y), N.ptr(g_out), B * Cc, H, W, N.ptr(ws), N.ptr(g_x), N.ptr(g_y),
                                     N.stream()))
    return g_x, g_y


def edge_smooth_fwd_launch(disp, img):
    """mean(|d_x disp| exp(-mean_c |d_x img|)) + mean(|d_y disp| exp(-mean_c |d_y img|)) (MD2/layers.py:207-220): K2 on one scale,
    on contiguous tensors."""
    if disp.dim() != 4 or disp.shape[1] != 1 or img.dim() != 4 or img.shape[0] != disp.shape[0] or img.shape[2:] != disp.shape[2:]:
        raise RuntimeError("smooth_loss: disp [B,1,H,W] and img [B,C,H,W] expected")
    B, Cc, H, W = img.shape
    lib = N.lib()
    part = torch.empty(lib.dmh_edge_smooth_partials_size(B, H, W), device=disp.device, dtype=torch.float32)
    out = torch.empty((), device=disp.device, dtype=torch.float32)
    N.check(lib.dmh_edge_smooth(N.ptr(disp), N.ptr(img), B, Cc, H, W, N.ptr(part), N.ptr(out), N.stream()))
    return out


def edge_smooth_bwd_launch(disp, img, g):
    B, Cc, H, W = img.shape
    g_disp = torch.empty_like(disp)
    N.check(N.lib().dmh_edge_smooth_bwd(N.ptr(disp), N.ptr(img), B, Cc, H, W, N.ptr(_c(g.to(torch.float32))), N.ptr(g_disp),
                                        N.stream()))
    return g_disp


def _paste_args(scene, patch, pmask, coeffs, l_pad, t_pad, OH, OW, mode=N.PASTE_COMPOSITE, flip=None, scene_index=None):
    a = N.PasteArgs()
    if flip is not None:
        if flip.dtype != torch.int32 or flip.numel() != coeffs.shape[0]:
            raise RuntimeError("eot_paste: flip must be an int32 tensor with one entry per sample")
        a.flip = N.ptr(flip)
    n = coeffs.shape[0]
    a.mode = mode
    if scene_index is not None:     # `scene` is a pool of frames; sample i reads frame scene_index[i] (range-checked by the caller)
        if scene_index.dtype != torch.int32 or scene_index.numel() != n or scene.shape[1] != 3:
            raise RuntimeError("eot_paste: scene_index must be an int32 tensor with one frame index per sample")
        a.scene_index = N.ptr(scene_index)
    elif scene.shape[0] not in (1, n) or scene.shape[1] != 3:
        raise RuntimeError("Batch size doesn't match!")
    if patch.dim() != 4 or patch.shape[0] != 1 or patch.shape[1] != 3 or tuple(pmask.shape) != (1, 1) + tuple(patch.shape[2:]):
        raise RuntimeError("eot_paste: patch must be [1,3,PH,PW] and mask [1,1,PH,PW]")
    if tuple(coeffs.shape) != (n, 8):
        raise RuntimeError("eot_paste: coeffs must be [N,8]")
    a.scene = N.ptr(scene) if mode == N.PASTE_COMPOSITE else None
    a.patch, a.pmask, a.coeffs = N.ptr(patch), N.ptr(pmask), N.ptr(coeffs)
    a.scene_bstride = 0 if (scene.shape[0] == 1 and scene_index is None) else scene.shape[1] * scene.shape[2] * scene.shape[3]
    a.N, a.SH, a.SW = n, scene.shape[2], scene.shape[3]
    a.PH, a.PW, a.OH, a.OW = patch.shape[2], patch.shape[3], OH, OW
    a.l_pad, a.t_pad = l_pad, t_pad
    return a


def eot_paste_fwd_launch(scene, patch, pmask, coeffs, l_pad, t_pad, OH, OW, mode=N.PASTE_COMPOSITE, flip=None, scene_index=None):
    """K3 on contiguous tensors: (adv [N,3,OH,OW], mask_out [N,1,OH,OW])."""
    a = _paste_args(scene, patch, pmask, coeffs, l_pad, t_pad, OH, OW, mode, flip, scene_index)
    adv = torch.empty((a.N, 3, OH, OW), device=scene.device, dtype=torch.float32)
    mask_out = torch.empty((a.N, 1, OH, OW), device=scene.device, dtype=torch.float32)
    # algorithmic bytes: the scene read once (one copy when it is broadcast) + patch and mask + the two outputs
    n_scene = scene.numel() if scene_index is None else a.N * 3 * a.SH * a.SW      # frames read, not the pool's size
    nb = 4 * (n_scene + patch.numel() + pmask.numel() + adv.numel() + mask_out.numel()) if mode == N.PASTE_COMPOSITE \
        else 4 * (patch.numel() + pmask.numel() + adv.numel() + mask_out.numel())
    N.check(_timed("paste_fwd", lambda: N.lib().dmh_eot_paste_fwd(C.byref(a), N.ptr(adv), N.ptr(mask_out), N.stream()), nb))
    return adv, mask_out


def eot_paste_bwd_launch(scene, patch, pmask, coeffs, l_pad, t_pad, OH, OW, mode, flip, scene_index, g_adv):
    """K3's adjoint: the gradient w.r.t. ``patch`` for ``g_adv`` (contiguous)."""
    a = _paste_args(scene, patch, pmask, coeffs, l_pad, t_pad, OH, OW, mode, flip, scene_index)
    g_patch = torch.empty_like(patch)
    N.check(_timed("paste_bwd", lambda: N.lib().dmh_eot_paste_bwd(C.byref(a), N.ptr(g_adv), N.ptr(g_patch), N.stream()),
                   4 * (g_adv.numel() + g_patch.numel())))
    return g_patch


class _EotPaste(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scene, patch, pmask, coeffs, l_pad, t_pad, OH, OW, mode, flip=None, scene_index=None):
        adv, mask_out = eot_paste_fwd_launch(scene, patch, pmask, coeffs, l_pad, t_pad, OH, OW, mode, flip, scene_index)
        ctx.save_for_backward(scene, patch, pmask, coeffs)
        ctx.geo = (l_pad, t_pad, OH, OW, mode)
        ctx.flip = flip
        ctx.scene_index = scene_index
        ctx.mark_non_differentiable(mask_out)
        return adv, mask_out

    @staticmethod
    def backward(ctx, g_adv, g_mask):
        scene, patch, pmask, coeffs = ctx.saved_tensors
        g_patch = eot_paste_bwd_launch(scene, patch, pmask, coeffs, *ctx.geo, ctx.flip, ctx.scene_index, _c(g_adv))
        return None, g_patch, None, None, None, None, None, None, None, None, None


def eot_paste(scene, patch, pmask, coeffs, l_pad, t_pad, out_size, flip=None, scene_index=None):
    """Pad -> perspective(patch, mask) -> composite -> Resize, fused (physicalTrans.py:107-166 +
    phy_obj_atk.py:87-90).  Returns (adv [N,3,OH,OW], mask_out [N,1,OH,OW]); differentiable w.r.t. patch.
    ``flip`` (int32 [N], optional): samples to mirror horizontally (mono_dataset.py:222-225 on an un-flipped scene).
    ``scene_index`` (int32 [N], optional): ``scene`` is a POOL of frames [P,3,SH,SW] and sample i reads frame scene_index[i]
    -- the loader's choice of frames and camera sides without copying them (the caller guarantees 0 <= index < P)."""
    return _EotPaste.apply(_c(scene), _c(patch), _c(pmask), _c(coeffs), int(l_pad), int(t_pad), int(out_size[0]),
                           int(out_size[1]), N.PASTE_COMPOSITE, flip, scene_index)


def perspective_warp(patch, pmask, coeffs, l_pad, t_pad, frame_size):
    """Pad + torchvision-0.8.2 perspective of patch and mask into [N,3,SH,SW] / [N,1,SH,SW] frames
    (physicalTrans.py:156-165), no compositing; differentiable w.r.t. patch."""
    SH, SW = int(frame_size[0]), int(frame_size[1])
    dummy = patch.new_empty((1, 3, SH, SW))   # shape carrier only; never read in warp-only mode
    return _EotPaste.apply(dummy, _c(patch), _c(pmask), _c(coeffs), int(l_pad), int(t_pad), SH, SW,
                           N.PASTE_WARP_ONLY)


def masked_sq_mean_fwd_launch(disp, mask):
    """K6 on contiguous tensors (``mask`` may be None): the cost, a float32 scalar on the device."""
    lib = N.lib()
    n = disp.numel()
    if mask is not None and mask.numel() != n:
        raise RuntimeError("masked_sq_mean: mask and disp sizes differ")
    part = torch.empty(lib.dmh_sq_mean_partials_size(n), device=disp.device, dtype=torch.float32)
    cost = torch.empty((), device=disp.device, dtype=torch.float32)
    N.check(lib.dmh_masked_sq_mean_fwd(N.ptr(disp), N.ptr(mask), n, N.ptr(part), N.ptr(cost), N.stream()))
    return cost


def masked_sq_mean_bwd_launch(disp, mask, g):
    g_disp = torch.empty_like(disp)
    N.check(N.lib().dmh_masked_sq_mean_bwd(N.ptr(disp), N.ptr(mask), disp.numel(), N.ptr(_c(g.to(torch.float32))),
                                           N.ptr(g_disp), N.stream()))
    return g_disp


class _MaskedSqMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, mask):
        cost = masked_sq_mean_fwd_launch(disp, mask)
        ctx.save_for_backward(disp, mask)
        return cost

    @staticmethod
    def backward(ctx, g):
        disp, mask = ctx.saved_tensors
        return masked_sq_mean_bwd_launch(disp, mask, g), None


def masked_sq_mean(disp, mask=None):
    """mean((disp*mask)^2) == nn.MSELoss()(disp*mask, zeros) (phy_obj_atk.py:94)."""
    return _MaskedSqMean.apply(_c(disp), None if mask is None else _c(mask))


def _gt_depth_operands(disp, disp_gt, objmask, objdepth):
    """Checked operands of the --gt_depth term: (disp, disp_gt, mask tensor, mask batch stride, objdepth[B], B, HW).
    ``objmask`` is inputs[("color_objmask",0,0)] ([B,3,H,W] or [B,1,H,W]; channel 0 is read in place through its batch stride),
    ``objdepth`` inputs[("objdepth",0,0)] (one distance per sample, any shape with B elements)."""
    disp, disp_gt = _c(disp), _c(disp_gt)
    if disp.dim() != 4 or disp.shape[1] != 1 or disp_gt.shape != disp.shape:
        raise RuntimeError("gt_depth_mse: disp and disp_gt must both be [B,1,H,W]")
    B, _, H, W = disp.shape
    if objmask.dim() != 4 or objmask.shape[0] != B or tuple(objmask.shape[2:]) != (H, W):
        raise RuntimeError("gt_depth_mse: color_objmask must be [B,C,H,W] at the disparity's size")
    if objmask.stride(3) != 1 or objmask.stride(2) != W or objmask.stride(0) < H * W:
        objmask = objmask[:, :1].contiguous()      # e.g. the dataset's expand(-1, 3, -1, -1) view of a one-channel mask
    if objmask.dtype != torch.float32 or objmask.device != disp.device or not objmask.is_cuda:
        raise RuntimeError("gt_depth_mse: color_objmask must be float32 on the disparity's (ROCm) device")
    objdepth = _c(objdepth.reshape(-1))
    if objdepth.numel() != B:
        raise RuntimeError("gt_depth_mse: objdepth needs one distance per sample")
    return disp, disp_gt, objmask, int(objmask.stride(0)), objdepth, B, H * W


def gt_depth_mse_fwd_launch(disp, disp_gt, objmask, bstride, objdepth, B, HW, min_depth, max_depth):
    """K6b on the output of _gt_depth_operands: the cost, a float32 scalar on the device."""
    lib = N.lib()
    part = torch.empty(lib.dmh_sq_mean_partials_size(B * HW), device=disp.device, dtype=torch.float32)
    cost = torch.empty((), device=disp.device, dtype=torch.float32)
    # channel 0 of the mask is read in place through its batch stride (layout validated by _gt_depth_operands)
    N.check(lib.dmh_gt_depth_mse_fwd(N.ptr(disp), N.ptr(disp_gt), C.c_void_p(objmask.data_ptr()), bstride, N.ptr(objdepth), B, HW,
                                     float(min_depth), float(max_depth), N.ptr(part), N.ptr(cost), N.stream()))
    return cost


def gt_depth_mse_bwd_launch(disp, disp_gt, objmask, bstride, objdepth, B, HW, min_depth, max_depth, g):
    g_disp = torch.empty_like(disp)
    N.check(N.lib().dmh_gt_depth_mse_bwd(N.ptr(disp), N.ptr(disp_gt), C.c_void_p(objmask.data_ptr()), bstride, N.ptr(objdepth), B, HW,
                                         float(min_depth), float(max_depth), N.ptr(_c(g.to(torch.float32))), N.ptr(g_disp),
                                         N.stream()))
    return g_disp


class _GtDepthMse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, disp_gt, objmask, objdepth, min_depth, max_depth):
        disp, disp_gt, objmask, bstride, objdepth, B, HW = _gt_depth_operands(disp, disp_gt, objmask, objdepth)
        ctx.save_for_backward(disp, disp_gt, objmask, objdepth)
        ctx.geo = (bstride, B, HW, float(min_depth), float(max_depth))
        return gt_depth_mse_fwd_launch(disp, disp_gt, objmask, bstride, objdepth, B, HW, min_depth, max_depth)

    @staticmethod
    def backward(ctx, g):
        disp, disp_gt, objmask, objdepth = ctx.saved_tensors
        bstride, B, HW, min_depth, max_depth = ctx.geo
        return gt_depth_mse_bwd_launch(disp, disp_gt, objmask, bstride, objdepth, B, HW, min_depth, max_depth, g), None, None, None, None, None


def gt_depth_mse(disp, disp_gt, objmask, objdepth, min_depth=0.1, max_depth=100.0):
    """--gt_depth supervised term (MD2/trainer.py:551-557): MSELoss(gt_depth, pred_depth) with
    pred / pseudo depth = clamp(disp_to_depth(.)[1] * 5.4, 1e-3, 80) and gt_depth = m objdepth + pseudo (1 - m), m = channel 0
    of color_objmask.  One fused pass forward, one backward (gradient w.r.t. ``disp`` only: disp_gt is the frozen teacher's)."""
    return _GtDepthMse.apply(disp, disp_gt.detach(), objmask, objdepth, min_depth, max_depth)


def avg_pyramid(x):
    """[F.avg_pool2d(x, 2), F.avg_pool2d(x, 4), F.avg_pool2d(x, 8)] of a [B,C,H,W] frame (H, W multiples of 8) in ONE launch,
    bit-identical to the three ATen calls: the colour pyramid inputs[("color", f, s)] of the GPU-side sample synthesis (no
    gradient: the frames are data)."""
    x = _c(x.detach())
    B, Cc, H, W = x.shape
    outs = [torch.empty((B, Cc, H >> s, W >> s), device=x.device, dtype=torch.float32) for s in (1, 2, 3)]
    N.check(_timed("avg_pyramid", lambda: N.lib().dmh_avg_pyramid(N.ptr(x), B * Cc, H, W, N.ptr(outs[0]), N.ptr(outs[1]),
                                                                  N.ptr(outs[2]), N.stream()), 4 * (x.numel() * 85 // 64)))
    return outs


def pgd_linf_step(x, x0, grad, alpha, eps, out=None):
    """x <- clamp(x0 + clamp(x + alpha*sign(grad) - x0, -eps, eps), 0, 1) (phy_obj_atk.py:98-101)."""
    x, x0, grad = _c(x.detach()), _c(x0), _c(grad)
    if x.shape != x0.shape or x.shape != grad.shape:
        raise RuntimeError("pgd_linf_step: shape mismatch")
    if out is None:
        out = torch.empty_like(x)
    N.check(N.lib().dmh_pgd_linf_step(N.ptr(x), N.ptr(x0), N.ptr(grad), float(alpha), float(eps), N.ptr(out),
                                      x.numel(), N.stream()))
    return out


def pgd_l2_workspace(n, device):
    """The float64 workspace of pgd_l2_step for tensors of ``n`` elements: K28's per-workgroup partial sums."""
    return torch.empty(int(N.lib().dmh_pgd_l2_workspace_size(int(n))) // 8, device=device, dtype=torch.float64)


def pgd_l2_step(x, x0, grad, alpha, eps, out=None, workspace=None):
    """K28: y = x + alpha grad / (||grad||_2 + 1e-10); out = clamp(x0 + (y - x0) min(eps / ||y - x0||_2, 1), 0, 1), with ONE norm
    over the whole tensor (phy_obj_atk_l2.py:110-120, shared-patch form).  Two launches, no host read.  ``workspace``:
    pgd_l2_workspace(x.numel(), x.device), written by every call (one is allocated when none is given: not inside a graph capture
    that is to be replayed).  ``out`` must be a tensor of its own."""
    x, x0, grad = _c(x.detach()), _c(x0), _c(grad)
    if x.shape != x0.shape or x.shape != grad.shape:
        raise RuntimeError("pgd_l2_step: shape mismatch")
    if not float(eps) >= 0.0:
        raise RuntimeError("pgd_l2_step: eps must not be negative")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape:
        raise RuntimeError("pgd_l2_step: shape mismatch")
    if workspace is None:
        workspace = pgd_l2_workspace(x.numel(), x.device)
    N.check(N.lib().dmh_pgd_l2_step(N.ptr(x), N.ptr(x0), N.ptr(grad), float(alpha), float(eps), N.ptr(out), x.numel(),
                                    N.ptr_f64(workspace), workspace.numel() * 8, N.stream()))
    return out


APGD_REC = 16       # floats per controller record (DMH_APGD_REC)


def apgd_controller(steps, eps, loss0, rho=0.75):
    """Device state of the Auto-PGD controller (K22) for one attack of ``steps`` iterations: (ctl [steps + 1, 16] with record 0
    filled from phy_obj_atk_apgd.py:137,190-200, hist [steps] zeros, cursor int32 [2] zeros, size_decr, steps_min).  ``loss0``:
    the device scalar holding the loss at the start point (loss_best and loss_best_last_check start there); nothing is read back."""
    steps = int(steps)
    if steps < 1 or steps >= 1 << 24:
        raise RuntimeError("apgd_controller: steps must lie in [1, 2^24)")
    _need_cuda(loss0)
    k0, steps_min, size_decr = max(int(0.22 * steps), 1), max(int(0.06 * steps), 1), max(int(0.03 * steps), 1)
    host = torch.zeros((steps + 1, APGD_REC), dtype=torch.float32)
    host[0, 0], host[0, 1], host[0, 4], host[0, 7] = 2.0 * float(torch.tensor(eps, dtype=torch.float32)), 1.0, k0, 1.0
    ctl = host.to(loss0.device, non_blocking=True)
    ctl[0, 2:4] = loss0.detach().reshape(1).to(torch.float32)
    hist = torch.zeros(steps, device=loss0.device, dtype=torch.float32)
    cursor = torch.zeros(2, device=loss0.device, dtype=torch.int32)
    return ctl, hist, cursor, size_decr, steps_min


def _apgd_check(name, steps, ctl, hist, cursor, tensors):
    n = tensors[0].numel()
    for t in tensors:
        if t.numel() != n or t.dtype != torch.float32:
            raise RuntimeError("%s: the patch-sized tensors must be fp32 and of one size" % name)
    if int(steps) < 1 or ctl.dtype != torch.float32 or ctl.numel() < (int(steps) + 1) * APGD_REC:
        raise RuntimeError("%s: ctl must hold steps + 1 records of %d floats" % (name, APGD_REC))
    if hist is not None and (hist.dtype != torch.float32 or hist.numel() < int(steps)):
        raise RuntimeError("%s: hist must hold steps floats" % name)
    if cursor.dtype != torch.int32 or cursor.numel() < 2:
        raise RuntimeError("%s: cursor must be int32[2]" % name)
    return n


def apgd_step(x_adv, x_old, x0, grad, ctl, cursor, steps, eps):
    """In place: x_old <- x_adv, x_adv <- Auto-PGD's momentum step (phy_obj_atk_apgd.py:207-215) with the step size and the
    momentum weight of the controller record the device cursor points at.  No host value of the iteration enters."""
    n = _apgd_check("apgd_step", steps, ctl, None, cursor, (x_adv, x_old, x0, grad))
    N.check(N.lib().dmh_apgd_step(N.ptr(x_adv), N.ptr(x_old), N.ptr(x0), N.ptr(grad), N.ptr(ctl), N.ptr(cursor), int(steps),
                                  float(eps), n, N.stream()))
    return x_adv


def apgd_commit(x_adv, g_new, grad, x_best, grad_best, x_ret, loss, ctl, hist, cursor, steps, size_decr, steps_min, rho=0.75):
    """In place, decided on the device from ``loss`` (device scalar: the cost at the new x_adv, ``g_new`` its gradient) and the
    controller record: best point, loss history, checkpoint, step halving, restart (phy_obj_atk_apgd.py:255-290); writes the
    next record and advances the cursor."""
    n = _apgd_check("apgd_commit", steps, ctl, hist, cursor, (x_adv, g_new, grad, x_best, grad_best, x_ret))
    if loss.numel() != 1 or loss.dtype != torch.float32:
        raise RuntimeError("apgd_commit: loss must be one fp32 value")
    N.check(N.lib().dmh_apgd_commit(N.ptr(x_adv), N.ptr(g_new), N.ptr(grad), N.ptr(x_best), N.ptr(grad_best), N.ptr(x_ret),
                                    N.ptr(loss), N.ptr(ctl), N.ptr(hist), N.ptr(cursor), int(steps), int(size_decr),
                                    int(steps_min), float(rho), n, N.stream()))
    return x_adv


LIGHT_REC = 10      # doubles per query record (DMH_LIGHT_REC)


def tube_light_table(params, alpha=1.0):
    """Host: the record array [n, 10] float64 of K24 for ``params`` [n, 4] = (wavelength, angle, b, beta) per query.  Every scalar
    is made in float64 the way the reference's Python makes it: k = round(tan(radians(angle)), 2) (phy_obj_atk_light.py:130-131),
    full_end = int(sqrt(beta) + 0.5), light_end = int(sqrt(beta * 20) + 0.5), the divisor sqrt(1 + k k) and the colour of
    wavelength_to_rgb with its ``** 0.8`` times alpha (light_simulation.py:40-84,143-146,150)."""
    import math
    params = np.asarray(params).reshape(-1, 4)
    out = np.zeros((len(params), LIGHT_REC), dtype=np.float64)
    for row, (wl, angle, b, beta) in zip(out, params.tolist()):
        k = round(math.tan(math.radians(angle)), 2)
        w, g = float(wl), 0.8
        if 380 <= w <= 440:         # the first matching band wins at a shared boundary
            att = 0.3 + 0.7 * (w - 380) / (440 - 380)
            c = (((-(w - 440) / (440 - 380)) * att) ** g, 0.0, (1.0 * att) ** g)
        elif 440 <= w <= 490:
            c = (0.0, ((w - 440) / (490 - 440)) ** g, 1.0)
        elif 490 <= w <= 510:
            c = (0.0, 1.0, (-(w - 510) / (510 - 490)) ** g)
        elif 510 <= w <= 580:
            c = (((w - 510) / (580 - 510)) ** g, 1.0, 0.0)
        elif 580 <= w <= 645:
            c = (1.0, (-(w - 645) / (645 - 580)) ** g, 0.0)
        elif 645 <= w <= 750:
            c = ((1.0 * (0.3 + 0.7 * (750 - w) / (750 - 645))) ** g, 0.0, 0.0)
        else:
            c = (0.0, 0.0, 0.0)
        row[:9] = (k, b, beta, int(math.sqrt(beta) + 0.5), int(math.sqrt(beta * 20) + 0.5), math.sqrt(1 + k * k),
                   c[0] * alpha, c[1] * alpha, c[2] * alpha)
    return out


def tube_light_host(base_hwc, rec):
    """Host twin of K24's compose in numpy (``Phy_obj_atk_light(host_chain=True)``): uint8 [H, W, 3] base and one record ->
    the lit uint8 [H, W, 3], float64 / fp32 with the roundings of the reference's chain."""
    h, w, _ = base_hwc.shape
    k, b, beta, full, end, s = (rec[i] for i in range(6))
    d = np.abs(k * np.arange(w, dtype=np.float64)[None, :] - np.arange(h, dtype=np.float64)[:, None] + b) / s
    with np.errstate(divide="ignore", invalid="ignore"):
        att = np.where(d <= full, 1.0, np.where(d <= end, beta / (d * d), 0.0))
    lit = (np.stack([rec[6 + i] * att for i in range(3)], -1) * 255.0).astype(np.float32)
    return np.clip(base_hwc.astype(np.float32) + lit, 0.0, 255.0).astype(np.uint8)


def tube_light_state(n_queries, device):
    """Device state of one tube-light search (K24): (state int32 [2] = (cursor 0, best query -1), best float [1] = 1e10,
    cost float [n_queries] zeros)."""
    if int(n_queries) < 1:
        raise RuntimeError("tube_light_state: need at least one query")
    state = torch.tensor([0, -1], dtype=torch.int32).to(device, non_blocking=True)
    best = torch.full((1,), 1e10, device=device, dtype=torch.float32)
    return state, best, torch.zeros(int(n_queries), device=device, dtype=torch.float32)


def tube_light_compose(table, index, base_u8, out=None):
    """The object lit by the tube light of record ``index[0]`` (a device int32: nothing of the query comes from the host) of
    ``table`` [n, 10] float64: ``base_u8`` [1 or no batch, 3, H, W] uint8 -> fp32 [1, 3, H, W], bit-equal to the reference's
    numpy / OpenCV / PIL chain.  An index outside [0, n) leaves ``out`` as it is."""
    if table.dim() != 2 or table.shape[1] != LIGHT_REC:
        raise RuntimeError("tube_light_compose: table must be [n, %d] float64" % LIGHT_REC)
    if index.dtype != torch.int32 or index.numel() < 1:
        raise RuntimeError("tube_light_compose: index must be int32")
    if base_u8.dtype != torch.uint8 or base_u8.numel() % 3 or base_u8.dim() < 3 or base_u8.shape[-3] != 3 \
            or base_u8.numel() != 3 * base_u8.shape[-2] * base_u8.shape[-1]:
        raise RuntimeError("tube_light_compose: base must be uint8 [3, H, W]")
    H, W = int(base_u8.shape[-2]), int(base_u8.shape[-1])
    if out is None:
        out = torch.zeros((1, 3, H, W), device=base_u8.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.numel() != base_u8.numel():
        raise RuntimeError("tube_light_compose: out must be fp32 of the base's size")
    N.check(N.lib().dmh_tube_light_compose(N.ptr_f64(table), N.ptr(index), N.ptr(base_u8), N.ptr(out), int(table.shape[0]), H, W,
                                           N.stream()))
    return out


def tube_light_commit(cost_in, cost, best, state):
    """In place, on the device (phy_obj_atk_light.py:165-167): the query the cursor state[0] points at gets ``cost_in`` (device
    scalar) into ``cost``; a strictly smaller cost than ``best`` becomes the best and its query state[1]; the cursor advances."""
    if cost_in.numel() != 1 or cost_in.dtype != torch.float32 or best.numel() != 1 or best.dtype != torch.float32 \
            or cost.dtype != torch.float32:
        raise RuntimeError("tube_light_commit: cost_in and best must be one fp32 value each, cost fp32")
    if state.dtype != torch.int32 or state.numel() < 2:
        raise RuntimeError("tube_light_commit: state must be int32[2]")
    N.check(N.lib().dmh_tube_light_commit(N.ptr(cost_in), N.ptr(cost), N.ptr(best), N.ptr(state), int(cost.numel()), N.stream()))
    return state


GAUSS_REGION = (90, 170, 100, 200)      # rows 90:170, columns 100:200 of the object (phy_obj_atk_guassian.py:88)


def gauss_sigmas(steps, h, w):
    """Host: the sigmas of a ``steps``-step Gaussian-blur attack on an h x w object, in Python floats as the reference
    accumulates them (phy_obj_atk_guassian.py:76-95): ``epsilon += 1.0 / steps``, ``sigma = epsilon * (max(h, w) // 2)``."""
    if int(steps) < 1:
        raise RuntimeError("gauss_sigmas: need at least one step")
    epsilon, stepsize, max_sigma, out = 0.0, 1.0 / int(steps), max(int(h), int(w)) // 2, []
    for _ in range(int(steps)):
        epsilon += stepsize
        out.append(epsilon * max_sigma)
    return out


def gauss_blur_table(sigmas):
    """Host: (weights float64 [n, max lw + 1], radii int32 [n]) of K26.  Row s holds p[0 .. lw] -- the left half and the centre
    of the symmetric kernel -- of scipy's ``_gaussian_kernel1d`` for sigma s with truncate 4.0, in float64 and in its order:
    lw = int(4.0 * s + 0.5), p = exp(-0.5 / (s * s) * x ** 2) for x = -lw .. lw, p / p.sum(); zero padded."""
    sigmas = [float(s) for s in sigmas]
    if not sigmas:
        raise RuntimeError("gauss_blur_table: need at least one sigma")
    if not all(s > 0.0 and np.isfinite(s) for s in sigmas):
        raise RuntimeError("gauss_blur_table: every sigma must be positive and finite")
    radii = np.asarray([int(4.0 * s + 0.5) for s in sigmas], dtype=np.int32)
    weights = np.zeros((len(sigmas), int(radii.max()) + 1), dtype=np.float64)
    for row, s, lw in zip(weights, sigmas, radii.tolist()):
        x = np.arange(-lw, lw + 1)
        p = np.exp(-0.5 / (s * s) * x ** 2)
        row[:lw + 1] = (p / p.sum())[:lw + 1]
    return weights, radii


def _gauss_region(region, H, W, name):
    """``region`` = (r0, r1, c0, c1) clipped to an H x W patch the way the slices [r0:r1, c0:c1] clip."""
    if len(region) != 4:
        raise RuntimeError("%s: region must be (r0, r1, c0, c1)" % name)
    r0, r1, _ = slice(int(region[0]), int(region[1])).indices(H)
    c0, c1, _ = slice(int(region[2]), int(region[3])).indices(W)
    if r1 <= r0 or c1 <= c0:
        raise RuntimeError("%s: the rectangle %s clips to empty on a %d x %d patch" % (name, tuple(region), H, W))
    return r0, r1, c0, c1


def _gauss_axis_host(a, idx, p, lw):
    """correlate1d of scipy (symmetric branch, mode 'reflect') along the last axis of ``a`` at the positions ``idx``: float64,
    the taps in scipy's order, every operation rounded on its own; the result rounded to fp32."""
    n = a.shape[-1]
    a = a.astype(np.float64)

    def r(j):
        m = np.mod(j, 2 * n)
        return np.where(m >= n, 2 * n - 1 - m, m)
    tmp = a[..., idx] * p[lw]
    for ll in range(-lw, 0):
        tmp = tmp + (a[..., r(idx + ll)] + a[..., r(idx - ll)]) * p[lw + ll]
    return tmp.astype(np.float32)


def gauss_blur_host(x, sigma, region=None):
    """Host twin of K26 in numpy (``Phy_obj_atk_guassian(host_chain=True)``): np.clip(gaussian_filter(x, [0, .., 0, s, s]), 0, 1) of
    fp32 ``x`` [..., H, W] on the rectangle ``region`` (the whole patch by default), bit-equal to scipy's."""
    x = np.asarray(x, dtype=np.float32)
    H, W = x.shape[-2:]
    r0, r1, c0, c1 = _gauss_region((0, H, 0, W) if region is None else region, H, W, "gauss_blur_host")
    weights, radii = gauss_blur_table([sigma])
    p, lw = weights[0], int(radii[0])
    rows = _gauss_axis_host(np.swapaxes(x, -1, -2), np.arange(r0, r1), p, lw)        # axis H first: [..., W, rh]
    out = _gauss_axis_host(np.swapaxes(rows, -1, -2), np.arange(c0, c1), p, lw)      # then axis W: [..., rh, rw]
    return np.clip(out, 0, 1)


def _gauss_obj(obj, name):
    if obj.dtype != torch.float32 or obj.dim() not in (3, 4) or (obj.dim() == 4 and obj.shape[0] != 1):
        raise RuntimeError("%s: obj must be fp32 [1, C, H, W] or [C, H, W]" % name)
    return tuple(int(v) for v in obj.shape[-3:])


def gauss_blur_windows(obj, weights, radii, region=GAUSS_REGION):
    """K26: np.clip(scipy.ndimage.gaussian_filter(obj, [0, 0, s, s]), 0, 1) on the rectangle ``region`` = (r0, r1, c0, c1) of
    fp32 ``obj`` [1, C, H, W] for every row of ``(weights, radii) = gauss_blur_table(sigmas)`` (device float64 [n, k] / int32
    [n]) -> fp32 [n, C, r1 - r0, c1 - c0], bit-equal to scipy's; two launches for all n."""
    C_, H, W = _gauss_obj(obj, "gauss_blur_windows")
    if weights.dim() != 2 or weights.dtype != torch.float64:
        raise RuntimeError("gauss_blur_windows: weights must be float64 [steps, k]")
    n = int(weights.shape[0])
    if n < 1 or int(weights.shape[1]) < 1:
        raise RuntimeError("gauss_blur_windows: need at least one step")
    if radii.dtype != torch.int32 or radii.dim() != 1 or int(radii.shape[0]) != n:
        raise RuntimeError("gauss_blur_windows: radii must be int32 [steps]")
    r0, r1, c0, c1 = _gauss_region(region, H, W, "gauss_blur_windows")
    tmp = torch.empty((n, C_, r1 - r0, W), device=obj.device, dtype=torch.float32)
    windows = torch.empty((n, C_, r1 - r0, c1 - c0), device=obj.device, dtype=torch.float32)
    N.check(N.lib().dmh_gauss_blur_windows(N.ptr(obj), N.ptr_f64(weights), N.ptr(radii), N.ptr(tmp), N.ptr(windows), n,
                                           int(weights.shape[1]), C_, H, W, r0, r1, c0, c1, N.stream()))
    return windows


def gauss_blur_compose(windows, index, obj, region=GAUSS_REGION, out=None):
    """The object with window ``index[0]`` (a device int32: nothing of the step comes from the host) of ``windows``
    [n, C, rh, rw] in the rectangle ``region`` and ``obj`` elsewhere -> fp32 [1, C, H, W].  An index outside [0, n) leaves
    ``out`` as it is."""
    C_, H, W = _gauss_obj(obj, "gauss_blur_compose")
    r0, r1, c0, c1 = _gauss_region(region, H, W, "gauss_blur_compose")
    if windows.dtype != torch.float32 or windows.dim() != 4 or int(windows.shape[0]) < 1 \
            or tuple(windows.shape[1:]) != (C_, r1 - r0, c1 - c0):
        raise RuntimeError("gauss_blur_compose: windows must be fp32 [steps, %d, %d, %d] for this rectangle" % (C_, r1 - r0, c1 - c0))
    if index.dtype != torch.int32 or index.numel() < 1:
        raise RuntimeError("gauss_blur_compose: index must be int32")
    if out is None:
        out = torch.zeros((1, C_, H, W), device=obj.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.numel() != obj.numel():
        raise RuntimeError("gauss_blur_compose: out must be fp32 of the object's size")
    N.check(N.lib().dmh_gauss_blur_compose(N.ptr(windows), N.ptr(index), N.ptr(obj), N.ptr(out), int(windows.shape[0]), C_, H, W,
                                           r0, r1, c0, c1, N.stream()))
    return out


def square_sides(n_queries, c, h, w, p_init=0.8, resc_schedule=True):
    """Host: the side of the square of every iteration of a Square attack of ``n_queries`` iterations on a c x h x w object, in
    Python floats as the reference makes it: ``p_selection`` (phy_obj_atk_square.py:222-249, with ``int(it / n_queries *
    10000)`` under ``resc_schedule``) and ``s = max(int(round(sqrt(p * n_features / c))), 1)`` (:281)."""
    import math
    n_queries = int(n_queries)
    if n_queries < 1:
        raise RuntimeError("square_sides: need at least one query")
    n_features, out = c * h * w, []
    for it in range(n_queries):
        if resc_schedule:
            it = int(it / n_queries * 10000)
        p = p_init
        for above, div in ((10, 2), (50, 4), (200, 8), (500, 16), (1000, 32), (2000, 64), (4000, 128), (6000, 256), (8000, 512)):
            if it > above:
                p = p_init / div
        out.append(max(int(round(math.sqrt(p * n_features / c))), 1))
    return out


def square_table(n_queries, c, h, w, p_init=0.8, resc_schedule=True):
    """Host: every draw of a Square attack, from the CPU torch global generator with the reference's expressions in its call
    order -- the start stripes ``sign(2 rand([1, c, 1, w]) - 1)`` (:259-260, :173-175), then per iteration ``vh``, ``vw`` =
    ``(0 + (h - s - 0) rand([1])).long()`` (:177-179, :282-283) and the signs ``sign(2 rand([c, 1, 1]) - 1)`` (:286).
    Returns (table int32 [n_queries + 1, 3 + c] = (vh, vw, s, signs) with row q the square of iteration q - 1 and row 0 zero:
    query 0 is the stripes; stripes fp32 [c, w]).  A side larger than min(h, w) -- where the reference would slice with a negative
    bound -- is refused before any draw."""
    sides = square_sides(n_queries, c, h, w, p_init, resc_schedule)
    if max(sides) > min(h, w):
        raise RuntimeError("square_table: the schedule's largest square (%d) exceeds the %d x %d object; lower p_init"
                           % (max(sides), h, w))
    stripes = torch.sign(2 * torch.rand([1, c, 1, w]) - 1).reshape(c, w).contiguous()
    table = np.zeros((len(sides) + 1, 3 + c), dtype=np.int32)
    for row, s in zip(table[1:], sides):
        vh = (0 + (h - s - 0) * torch.rand([1])).long()
        vw = (0 + (w - s - 0) * torch.rand([1])).long()
        sign = torch.sign(2 * torch.rand([c, 1, 1]) - 1)
        row[0], row[1], row[2] = int(vh), int(vw), s
        row[3:] = sign.reshape(c).numpy()
    return table, stripes


def _square_operands(name, x0, x_best, x_new, table, stripes):
    if x0.dtype != torch.float32 or x0.dim() not in (3, 4) or (x0.dim() == 4 and x0.shape[0] != 1):
        raise RuntimeError("%s: x0 must be fp32 [1, C, H, W] or [C, H, W]" % name)
    C_, H, W = (int(v) for v in x0.shape[-3:])
    for t in (x_best, x_new):
        if t.dtype != torch.float32 or t.numel() != x0.numel() or tuple(t.shape[-3:]) != (C_, H, W):
            raise RuntimeError("%s: x_best and x_new must be fp32 of x0's size" % name)
    ptrs = {x0.data_ptr(), x_best.data_ptr(), x_new.data_ptr()}
    if len(ptrs) != 3:
        raise RuntimeError("%s: x0, x_best and x_new must be three different buffers" % name)
    if table.dtype != torch.int32 or table.dim() != 2 or int(table.shape[0]) < 1 or int(table.shape[1]) != 3 + C_:
        raise RuntimeError("%s: table must be int32 [n, %d]" % (name, 3 + C_))
    if stripes.dtype != torch.float32 or tuple(stripes.shape) != (C_, W):
        raise RuntimeError("%s: stripes must be fp32 [%d, %d]" % (name, C_, W))
    return C_, H, W


def square_propose(x0, x_best, x_new, table, stripes, state, eps):
    """K27, in place, driven by K24's ``state`` = (cursor q, best query) on the device: if query q - 1 became the best,
    ``x_best`` <- ``x_new``; then ``x_new`` <- the candidate of query q -- the stripes for q = 0, else ``x_best`` with the square
    of ``table`` row q pushed by 2 eps sign_c and projected onto [x0 - eps, x0 + eps] and [0, 1] (phy_obj_atk_square.py:284-291),
    bit-equal to the torch expression.  q = n only absorbs; any other q outside [0, n) does nothing."""
    C_, H, W = _square_operands("square_propose", x0, x_best, x_new, table, stripes)
    if state.dtype != torch.int32 or state.numel() < 2:
        raise RuntimeError("square_propose: state must be int32[2]")
    if not float(eps) >= 0.0:
        raise RuntimeError("square_propose: eps must not be negative")
    N.check(N.lib().dmh_square_propose(N.ptr(x0), N.ptr(x_best), N.ptr(x_new), N.ptr(table), N.ptr(stripes), N.ptr(state),
                                       int(table.shape[0]), C_, H, W, float(eps), N.stream()))
    return x_new


def square_host(x0, x_best, x_new, table, stripes, q, accept, eps):
    """Host twin of K27 in torch on the CPU (``Phy_obj_atk_Square(host_chain=True)``): returns the new (x_best, x_new) for query
    ``q`` after the decision ``accept`` about query q - 1, with the reference's own expressions (:259-260, :284-291)."""
    C_, H, W = _square_operands("square_host", x0, x_best, x_new, torch.as_tensor(table), stripes)
    n = len(table)
    if accept and 0 < q <= n:
        x_best = x_new.clone()
    if q == 0:
        x_new = torch.clamp(x0 + eps * stripes.reshape(1, C_, 1, W), 0., 1.).reshape(x0.shape)
    elif 0 < q < n:
        vh, vw, s = (int(v) for v in table[q][:3])
        new_deltas = torch.zeros([C_, H, W])
        new_deltas[:, vh:vh + s, vw:vw + s] = 2. * eps * torch.as_tensor(table[q][3:]).float().reshape(C_, 1, 1)
        x_new = x_best.reshape(C_, H, W) + new_deltas
        x_new = torch.min(torch.max(x_new, x0.reshape(C_, H, W) - eps), x0.reshape(C_, H, W) + eps)
        x_new = torch.clamp(x_new, 0., 1.).reshape(x0.shape)
    return x_best, x_new


def l0_compose_fwd_launch(obj, pos, neg, l0_clip, finalize):
    """K5 on contiguous tensors: (adv, count int32 [1])."""
    if obj.dim() != 4 or obj.shape[0] != 1 or obj.shape != pos.shape or obj.shape != neg.shape:
        raise RuntimeError("l0_compose: obj/pos/neg must all be [1,C,H,W]")
    adv = torch.empty_like(obj)
    count = torch.zeros(1, device=obj.device, dtype=torch.int32)
    N.check(N.lib().dmh_l0_compose_fwd(N.ptr(obj), N.ptr(pos), N.ptr(neg), obj.shape[1], obj.shape[2] * obj.shape[3],
                                       float(l0_clip), int(finalize), N.ptr(adv), N.ptr(count), N.stream()))
    return adv, count


def l0_compose_bwd_launch(obj, pos, neg, g_adv):
    g_pos, g_neg = torch.empty_like(pos), torch.empty_like(neg)
    N.check(N.lib().dmh_l0_compose_bwd(N.ptr(obj), N.ptr(pos), N.ptr(neg), N.ptr(g_adv), obj.shape[1], obj.shape[2] * obj.shape[3],
                                       N.ptr(g_pos), N.ptr(g_neg), 0, N.stream()))
    return g_pos, g_neg


class _L0Compose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obj, pos, neg, l0_clip, finalize):
        adv, count = l0_compose_fwd_launch(obj, pos, neg, l0_clip, finalize)
        ctx.save_for_backward(obj, pos, neg)
        ctx.mark_non_differentiable(count)
        return adv, count

    @staticmethod
    def backward(ctx, g_adv, g_count):
        obj, pos, neg = ctx.saved_tensors
        g_pos, g_neg = l0_compose_bwd_launch(obj, pos, neg, _c(g_adv))
        return None, g_pos, g_neg, None, None


def l0_compose(obj, pos, neg, l0_clip=1.0 / 255.0, finalize=False):
    """adv = clamp(obj + clamp(pos,0,1) - clamp(neg,0,1), 0, 1) and the L0 count of the thresholded
    pattern (phy_obj_atk_l0.py:94-99, 43-52; finalize=True applies :143-150).  Returns (adv, count[int32,1])."""
    return _L0Compose.apply(_c(obj), _c(pos), _c(neg), float(l0_clip), bool(finalize))


def l0_mask_cost_fwd_launch(pos, neg):
    if pos.dim() != 4 or pos.shape[0] != 1 or pos.shape != neg.shape:
        raise RuntimeError("l0_mask_cost: pos/neg must be [1,C,H,W]")
    lib = N.lib()
    Cc, HW = pos.shape[1], pos.shape[2] * pos.shape[3]
    part = torch.empty(lib.dmh_l0_mask_partials_size(HW), device=pos.device, dtype=torch.float32)
    cost = torch.empty((), device=pos.device, dtype=torch.float32)
    N.check(lib.dmh_l0_mask_cost_fwd(N.ptr(pos), N.ptr(neg), Cc, HW, N.ptr(part), N.ptr(cost), N.stream()))
    return cost


def l0_mask_cost_bwd_launch(pos, neg, g):
    g_pos, g_neg = torch.empty_like(pos), torch.empty_like(neg)
    N.check(N.lib().dmh_l0_mask_cost_bwd(N.ptr(pos), N.ptr(neg), pos.shape[1], pos.shape[2] * pos.shape[3],
                                         N.ptr(_c(g.to(torch.float32))), None, N.ptr(g_pos), N.ptr(g_neg), 0, N.stream()))
    return g_pos, g_neg


class _L0MaskCost(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, neg):
        ctx.save_for_backward(pos, neg)
        return l0_mask_cost_fwd_launch(pos, neg)

    @staticmethod
    def backward(ctx, g):
        return l0_mask_cost_bwd_launch(*ctx.saved_tensors, g)


def l0_mask_cost(pos, neg):
    """mean(max_c(tanh(pos/10)/(2-1e-7)+0.5)) + same for neg (phy_obj_atk_l0.py:130-132)."""
    return _L0MaskCost.apply(_c(pos), _c(neg))


L0_REC = 8          # floats per record of the fused L0 update (DMH_L0_REC)
L0_BETAS = (0.5, 0.9)   # phy_obj_atk_l0.py:85; K23 holds them as constants


def l0_adam_table(steps, lr):
    """Adam's bias corrections for t = 1 .. 2 * steps as K23 reads them: a host fp32 tensor [2 * steps, 2] of
    (lr / (1 - b1^t), sqrt(1 - b2^t)), computed in double and rounded once."""
    import math
    b1, b2 = L0_BETAS
    rows = [(float(lr) / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)) for t in range(1, 2 * int(steps) + 1)]
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


class L0FusedState(object):
    """The device buffers of one fused L0 attack of ``steps`` (2 * steps iterations at the most): the two patterns (taken over,
    updated in place), Adam's m / v for both, the composed patch, and the controller's words -- count int32 [2 steps + 1], rec
    [2 steps, L0_REC], cursor int32 [2], tab [2 steps, 2].  Nothing here is read by the host while the attack runs."""

    def __init__(self, pos, neg, steps, lr):
        steps = int(steps)
        if steps < 1 or steps >= 1 << 24:
            raise RuntimeError("L0FusedState: steps must lie in [1, 2^24)")
        _need_cuda(pos)
        dev = pos.device
        self.steps = steps
        self.pos, self.neg = _c(pos.detach()), _c(neg.detach())
        state = torch.zeros((4,) + tuple(pos.shape), device=dev, dtype=torch.float32)
        self.m_pos, self.v_pos, self.m_neg, self.v_neg = state[0], state[1], state[2], state[3]
        self.adv = torch.empty_like(self.pos)
        self.count = torch.zeros(2 * steps + 1, device=dev, dtype=torch.int32)
        self.rec = torch.zeros((2 * steps, L0_REC), device=dev, dtype=torch.float32)
        self.cursor = torch.zeros(2, device=dev, dtype=torch.int32)
        self.tab = l0_adam_table(steps, lr).to(dev, non_blocking=True)

    def step(self, obj, g_adv, adv_cost, mask_cost, mask_wt, thresh, l0_clip):
        return l0_fused_step(obj, self.pos, self.neg, self.m_pos, self.v_pos, self.m_neg, self.v_neg, g_adv, self.adv,
                             self.count, self.rec, self.cursor, self.tab, adv_cost, mask_cost, self.steps, mask_wt, thresh,
                             l0_clip)


def l0_fused_step(obj, pos, neg, m_pos, v_pos, m_neg, v_neg, g_adv, adv, count, rec, cursor, tab, adv_cost, mask_cost, steps,
                  mask_wt, thresh, l0_clip=1.0 / 255.0):
    """K23, in place: iteration i = cursor[0] of the L0 attack from ``g_adv`` = d adv_cost / d composed patch to the next composed
    patch ``adv`` -- mask weight from count[i] / count[0] <= thresh, both clamps' gates, the mask cost's gradient, Adam on both
    patterns, compose, count[i + 1], record i, cursor + 1 (phy_obj_atk_l0.py:92-138).  No host value of the iteration enters."""
    steps = int(steps)
    if obj.dim() != 4 or obj.shape[0] != 1:
        raise RuntimeError("l0_fused_step: obj must be [1,C,H,W]")
    n = obj.numel()
    for t in (obj, pos, neg, m_pos, v_pos, m_neg, v_neg, g_adv, adv):
        if t.numel() != n or t.dtype != torch.float32:
            raise RuntimeError("l0_fused_step: the patch-sized tensors must be fp32 and of one size")
    if steps < 1 or steps >= 1 << 24:
        raise RuntimeError("l0_fused_step: steps must lie in [1, 2^24)")
    if count.dtype != torch.int32 or count.numel() < 2 * steps + 1:
        raise RuntimeError("l0_fused_step: count must be int32[2 * steps + 1]")
    if rec.dtype != torch.float32 or rec.numel() < 2 * steps * L0_REC:
        raise RuntimeError("l0_fused_step: rec must hold 2 * steps records of %d floats" % L0_REC)
    if tab.dtype != torch.float32 or tab.numel() < 4 * steps:
        raise RuntimeError("l0_fused_step: tab must hold 2 * steps pairs of floats")
    if cursor.dtype != torch.int32 or cursor.numel() < 2:
        raise RuntimeError("l0_fused_step: cursor must be int32[2]")
    for name, t in (("adv_cost", adv_cost), ("mask_cost", mask_cost)):
        if t is not None and (t.numel() != 1 or t.dtype != torch.float32):
            raise RuntimeError("l0_fused_step: %s must be one fp32 value" % name)
    N.check(N.lib().dmh_l0_fused_step(N.ptr(obj), N.ptr(pos), N.ptr(neg), N.ptr(m_pos), N.ptr(v_pos), N.ptr(m_neg), N.ptr(v_neg),
                                      N.ptr(g_adv), N.ptr(adv), N.ptr(count), N.ptr(rec), N.ptr(cursor), N.ptr(tab),
                                      N.ptr(adv_cost), N.ptr(mask_cost), steps, obj.shape[1], obj.shape[2] * obj.shape[3],
                                      float(mask_wt), float(thresh), float(l0_clip), N.stream()))
    return adv


class _UpCatPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, skip):
        lib = N.lib()
        B, C1, h, w = y.shape
        C2 = 0 if skip is None else skip.shape[1]
        if skip is not None and tuple(skip.shape) != (B, C2, 2 * h, 2 * w):
            raise RuntimeError("up_cat_pad: skip must be [B,C2,2h,2w], got %s for y %s" % (tuple(skip.shape), tuple(y.shape)))
        out = torch.empty((B, C1 + C2, 2 * h + 2, 2 * w + 2), device=y.device, dtype=torch.float32)
        nb = 4 * (y.numel() + (0 if skip is None else skip.numel()) + out.numel())
        N.check(_timed("up_cat_pad_fwd", lambda: lib.dmh_dec_up_cat_pad_fwd(N.ptr(y), N.ptr(skip), B, C1, C2, h, w,
                                                                           N.ptr(out), N.stream()), nb))
        ctx.save_for_backward(y)
        ctx.c2 = C2
        ctx.skip_grad = skip is not None and skip.requires_grad
        return out

    @staticmethod
    def backward(ctx, g_out):
        (y,) = ctx.saved_tensors
        lib = N.lib()
        B, C1, h, w = y.shape
        g_y = torch.empty_like(y)
        g_skip = torch.empty((B, ctx.c2, 2 * h, 2 * w), device=y.device, dtype=torch.float32) if ctx.skip_grad else None
        g_out = _c(g_out)
        nb = 4 * (2 * y.numel() + g_out.numel() + (0 if g_skip is None else g_skip.numel()))
        N.check(_timed("up_cat_pad_bwd", lambda: lib.dmh_dec_up_cat_pad_bwd(N.ptr(y), N.ptr(g_out), B, C1, ctx.c2, h, w,
                                                                           N.ptr(g_y), N.ptr(g_skip), N.stream()), nb))
        return g_y, g_skip


def up_cat_pad(y, skip=None):
    """pad1_reflect(cat(up2_nearest(ELU(y)), skip)) in one pass (MD2/networks/depth_decoder.py:54-60 + the
    ReflectionPad2d of the next Conv3x3)."""
    return _UpCatPad.apply(_c(y), None if skip is None else _c(skip))


class _EluPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, apply_elu):
        lib = N.lib()
        B, Cc, H, W = z.shape
        out = torch.empty((B, Cc, H + 2, W + 2), device=z.device, dtype=torch.float32)
        N.check(_timed("elu_pad_fwd", lambda: lib.dmh_elu_pad_fwd(N.ptr(z), B, Cc, H, W, int(apply_elu), N.ptr(out),
                                                                 N.stream()), 4 * (z.numel() + out.numel())))
        ctx.save_for_backward(z)
        ctx.apply_elu = int(apply_elu)
        return out

    @staticmethod
    def backward(ctx, g_out):
        (z,) = ctx.saved_tensors
        lib = N.lib()
        B, Cc, H, W = z.shape
        g_z = torch.empty_like(z)
        g_out = _c(g_out)
        N.check(_timed("elu_pad_bwd", lambda: lib.dmh_elu_pad_bwd(N.ptr(z), N.ptr(g_out), B, Cc, H, W, ctx.apply_elu,
                                                                 N.ptr(g_z), N.stream()), 4 * (2 * z.numel() + g_out.numel())))
        return g_z, None


def elu_pad(z, apply_elu=True):
    """pad1_reflect(ELU(z)) in one pass (apply_elu=False: ReflectionPad2d(1) only)."""
    return _EluPad.apply(_c(z), bool(apply_elu))


class _BnAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, shift, residual, relu):
        lib = N.lib()
        B, Cc = x.shape[0], x.shape[1]
        HW = x.numel() // (B * Cc)
        if scale.numel() != Cc or shift.numel() != Cc:
            raise RuntimeError("bn_act: scale/shift must have %d entries" % Cc)
        if residual is not None and residual.shape != x.shape:
            raise RuntimeError("bn_act: residual %s does not match x %s" % (tuple(residual.shape), tuple(x.shape)))
        out = torch.empty_like(x)
        nb = 4 * (x.numel() * (2 if residual is None else 3))
        N.check(_timed("bn_act_fwd", lambda: lib.dmh_bn_act_fwd(N.ptr(x), N.ptr(scale), N.ptr(shift), N.ptr(residual), B,
                                                               Cc, HW, int(relu), N.ptr(out), N.stream()), nb))
        ctx.save_for_backward(out if relu else None, scale)
        ctx.relu = int(relu)
        ctx.res_grad = residual is not None and residual.requires_grad
        ctx.x_grad = x.requires_grad
        return out

    @staticmethod
    def backward(ctx, g_out):
        out, scale = ctx.saved_tensors
        lib = N.lib()
        g_out = _c(g_out)
        B, Cc = g_out.shape[0], g_out.shape[1]
        HW = g_out.numel() // (B * Cc)
        g_x = torch.empty_like(g_out)
        g_res = torch.empty_like(g_out) if ctx.res_grad else None
        nb = 4 * g_out.numel() * (2 + (1 if ctx.relu else 0) + (1 if ctx.res_grad else 0))
        N.check(_timed("bn_act_bwd", lambda: lib.dmh_bn_act_bwd(N.ptr(out), N.ptr(g_out), N.ptr(scale), B, Cc, HW, ctx.relu,
                                                               N.ptr(g_x), N.ptr(g_res), N.stream()), nb))
        return g_x, None, None, g_res, None


def _reject_affine_grad(name, scale, shift):
    """scale / shift are constants of these ops (their backward returns None for them): refuse, loudly, a call that
    expects a gradient through them instead of silently dropping it."""
    if torch.is_grad_enabled() and not _wino_frozen and (scale.requires_grad or shift.requires_grad):
        raise RuntimeError("%s: scale/shift require grad, but this op treats them as constants (eval-mode BatchNorm "
                           "inside an attack); use the nn.BatchNorm2d module path, ops.frozen_weights() or detach()" % name)


def bn_act(x, scale, shift, residual=None, relu=True):
    """act(x * scale[c] + shift[c] (+ residual)) in one pass: BatchNorm2d in eval() mode folded to its per-channel
    affine, the BasicBlock's identity add and the ReLU (torchvision BasicBlock.forward as used by
    MD2/networks/resnet_encoder.py:85-98).  No gradient flows to scale/shift (eval-mode statistics and affine
    parameters are constants of the attack; phy_obj_atk.py:96 differentiates w.r.t. the patch only)."""
    _reject_affine_grad("bn_act", scale, shift)
    return _BnAct.apply(_c(x), _c(scale.detach()), _c(shift.detach()), None if residual is None else _c(residual),
                        bool(relu))


def _bn_train_stats(x, bn):
    """Batch statistics of x for the BatchNorm2d module `bn` in train mode: (scale, shift, save_mean, save_invstd);
    updates bn.running_mean / running_var / num_batches_tracked as nn.BatchNorm2d.forward does."""
    lib = N.lib()
    B, Cc = x.shape[0], x.shape[1]
    HW = x.numel() // (B * Cc)
    dev = x.device
    part = torch.empty(lib.dmh_bn_stats_partials_size(B, Cc, HW), device=dev, dtype=torch.float32)
    scale, shift, mean, invstd = (torch.empty(Cc, device=dev, dtype=torch.float32) for _ in range(4))
    if bn.momentum is None:
        raise RuntimeError("bn_act_train: cumulative-average BatchNorm (momentum=None) is not supported")
    track = bn.track_running_stats and bn.running_mean is not None
    nbt = bn.num_batches_tracked if (track and bn.num_batches_tracked is not None) else None
    if nbt is not None and not (nbt.is_cuda and nbt.dtype == torch.int64 and nbt.numel() == 1):
        raise RuntimeError("bn_act_train: num_batches_tracked must be a CUDA int64 scalar")
    N.check(_timed("bn_train_stats", lambda: lib.dmh_bn_train_stats_tracked(
        N.ptr(x), B, Cc, HW, N.ptr(None if bn.weight is None else _c(bn.weight.detach())),
        N.ptr(None if bn.bias is None else _c(bn.bias.detach())), float(bn.momentum), float(bn.eps),
        N.ptr(bn.running_mean if track else None), N.ptr(bn.running_var if track else None),
        None if nbt is None else C.c_void_p(nbt.data_ptr()), N.ptr(part), N.ptr(scale),
        N.ptr(shift), N.ptr(mean), N.ptr(invstd), N.stream()), 4 * x.numel()))
    return scale, shift, mean, invstd


def _bn_backward(g_pre, x, weight, bn, mean, invstd, eps, mask):
    """BatchNorm2d backward (train mode) from the saved batch statistics.  MIOpen's kernel when all three gradients
    are wanted (the train pass: 157 us average against 258 us for ATen's native kernel on these shapes)."""
    if all(mask) and weight is not None and hasattr(torch.ops.aten, "miopen_batch_norm_backward"):
        return torch.ops.aten.miopen_batch_norm_backward(x, g_pre, weight, bn.running_mean, bn.running_var, mean, invstd, eps)
    return torch.ops.aten.native_batch_norm_backward(g_pre, x, weight, bn.running_mean, bn.running_var, mean, invstd, True,
                                                     eps, mask)


def channel_sum(g):
    """sum of a contiguous fp32 CUDA [B, C, H, W] tensor over (0, 2, 3): a convolution's bias gradient, one streaming read."""
    lib = N.lib()
    B, Cc = g.shape[0], g.shape[1]
    HW = g.numel() // (B * Cc)
    part = torch.empty(lib.dmh_channel_sum_partials_size(B, Cc, HW), device=g.device, dtype=torch.float32)
    out = torch.empty(Cc, device=g.device, dtype=torch.float32)
    N.check(_timed("channel_sum", lambda: lib.dmh_channel_sum(N.ptr(g), B, Cc, HW, N.ptr(part), N.ptr(out), N.stream()),
                   4 * g.numel()))
    return out


def _bn_backward_fused(g, x, out, weight, mean, invstd, want_pre):
    """K9 train-mode BatchNorm backward (dmh_bn_train_bwd): ReLU mask (``out`` = the saved ReLU output, or None) + the
    three gradients in three launches.  Returns (g_x, g_weight, g_bias, g_pre or None)."""
    lib = N.lib()
    B, Cc = g.shape[0], g.shape[1]
    HW = g.numel() // (B * Cc)
    ws = torch.empty(lib.dmh_bn_train_bwd_workspace_size(B, Cc, HW), device=g.device, dtype=torch.float32)
    gx = torch.empty_like(g)
    gw = torch.empty(Cc, device=g.device, dtype=torch.float32)
    gb = torch.empty(Cc, device=g.device, dtype=torch.float32)
    g_pre = torch.empty_like(g) if want_pre else None
    nb = 4 * g.numel() * ((6 if out is not None else 4) + 1 + (1 if want_pre else 0))
    N.check(_timed("bn_train_bwd", lambda: lib.dmh_bn_train_bwd(
        N.ptr(x), N.ptr(g), N.ptr(out), N.ptr(weight), N.ptr(mean), N.ptr(invstd), B, Cc, HW, N.ptr(ws), N.ptr(gx), N.ptr(gw),
        N.ptr(gb), N.ptr(g_pre), N.stream()), nb))
    return gx, gw, gb, g_pre


class _BnActTrain(torch.autograd.Function):
    """Train-mode BatchNorm2d -> (+ residual) -> ReLU: K9 statistics + one bn_act pass forward; backward = ReLU mask
    (one K9 pass) + aten::native_batch_norm_backward (MIOpen) with the saved batch statistics."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, relu, bn):
        lib = N.lib()
        scale, shift, mean, invstd = _bn_train_stats(x, bn)
        B, Cc = x.shape[0], x.shape[1]
        HW = x.numel() // (B * Cc)
        out = torch.empty_like(x)
        nb = 4 * (x.numel() * (2 if residual is None else 3))
        N.check(_timed("bn_act_fwd", lambda: lib.dmh_bn_act_fwd(N.ptr(x), N.ptr(scale), N.ptr(shift), N.ptr(residual), B, Cc,
                                                               HW, int(relu), N.ptr(out), N.stream()), nb))
        ctx.save_for_backward(x, weight, mean, invstd, out if relu else None)
        ctx.relu, ctx.eps, ctx.bn = bool(relu), float(bn.eps), bn
        ctx.res_grad = residual is not None and residual.requires_grad
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, mean, invstd, out = ctx.saved_tensors
        lib = N.lib()
        g = _c(g)
        B, Cc = g.shape[0], g.shape[1]
        if weight is not None and g.numel() < (1 << 31) and Cc <= 65535:
            gx, gw, gb, g_pre = _bn_backward_fused(g, x, out if ctx.relu else None, weight, mean, invstd,
                                                   ctx.res_grad and ctx.relu)
            if ctx.res_grad and not ctx.relu:
                g_pre = g
            return gx, gw, gb, (g_pre if ctx.res_grad else None), None, None
        if ctx.relu:
            ones = frozen_memo(("ones", Cc, g.device), lambda: torch.ones(Cc, device=g.device, dtype=torch.float32))
            g_pre = torch.empty_like(g)
            N.check(_timed("bn_act_bwd", lambda: lib.dmh_bn_act_bwd(N.ptr(out), N.ptr(g), N.ptr(ones), B, Cc,
                                                                   g.numel() // (B * Cc), 1, N.ptr(g_pre), None, N.stream()),
                           12 * g.numel()))
        else:
            g_pre = g
        gx, gw, gb = _bn_backward(g_pre, x, weight, ctx.bn, mean, invstd, ctx.eps,
                                  [ctx.needs_input_grad[0], weight is not None and ctx.needs_input_grad[1],
                                   weight is not None and ctx.needs_input_grad[2]])
        return gx, gw, gb, (g_pre if ctx.res_grad else None), None, None


def bn_act_train(bn, x, residual=None, relu=True):
    """act(bn(x) (+ residual)) for an nn.BatchNorm2d in train mode (batch statistics, running statistics updated):
    torchvision BasicBlock under model.train() (MD2/networks/resnet_encoder.py:85-98, the training pass)."""
    return _BnActTrain.apply(_c(x), bn.weight, bn.bias, None if residual is None else _c(residual), bool(relu), bn)


def _stem_pool_fwd(x, scale, shift):
    """K9 stem: (feat = relu(x * scale + shift), maxpool3x3/2(feat), the pool's argmax bytes) in one launch."""
    B, Cc, H, W = x.shape
    feat = torch.empty_like(x)
    pooled = torch.empty((B, Cc, H // 2, W // 2), device=x.device, dtype=torch.float32)
    arg = torch.empty((B, Cc, H // 2, W // 2), device=x.device, dtype=torch.uint8)
    nb = 4 * (2 * x.numel() + pooled.numel()) + arg.numel()
    N.check(_timed("stem_fwd", lambda: N.lib().dmh_stem_bn_relu_pool_fwd(N.ptr(x), N.ptr(scale), N.ptr(shift), B, Cc, H, W,
                                                                        N.ptr(feat), N.ptr(pooled), N.ptr(arg), N.stream()), nb))
    return feat, pooled, arg


class _StemBnReluPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, shift):
        feat, pooled, arg = _stem_pool_fwd(x, scale, shift)
        ctx.save_for_backward(feat, arg, scale)
        ctx.mark_non_differentiable(arg)
        ctx.set_materialize_grads(False)    # an unused output hands None to backward: the kernel skips that read
        return feat, pooled, arg

    @staticmethod
    def backward(ctx, g_feat, g_pooled, _g_arg):
        feat, arg, scale = ctx.saved_tensors
        if g_feat is None and g_pooled is None:
            return None, None, None
        lib = N.lib()
        B, Cc, H, W = feat.shape
        g_feat = None if g_feat is None else _c(g_feat)
        g_pooled = None if g_pooled is None else _c(g_pooled)
        g_x = torch.empty_like(feat)
        nb = 4 * (2 * feat.numel() + (0 if g_feat is None else feat.numel()) +
                  (0 if g_pooled is None else g_pooled.numel())) + arg.numel()
        N.check(_timed("stem_bwd", lambda: lib.dmh_stem_bn_relu_pool_bwd(N.ptr(feat), N.ptr(arg), N.ptr(g_feat),
                                                                        N.ptr(g_pooled), N.ptr(scale), B, Cc, H, W,
                                                                        N.ptr(g_x), N.stream()), nb))
        return g_x, None, None


class _StemTrain(torch.autograd.Function):
    """Train-mode stem: BatchNorm2d (batch statistics) -> ReLU -> MaxPool2d(3, 2, 1) with the K9 kernels; backward =
    max-pool adjoint + skip gradient + ReLU mask in one K9 pass, then aten::native_batch_norm_backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn):
        scale, shift, mean, invstd = _bn_train_stats(x, bn)
        feat, pooled, arg = _stem_pool_fwd(x, scale, shift)
        ctx.save_for_backward(x, weight, mean, invstd, feat, arg)
        ctx.eps, ctx.bn = float(bn.eps), bn
        ctx.mark_non_differentiable(arg)
        ctx.set_materialize_grads(False)
        return feat, pooled, arg

    @staticmethod
    def backward(ctx, g_feat, g_pooled, _g_arg):
        x, weight, mean, invstd, feat, arg = ctx.saved_tensors
        if g_feat is None and g_pooled is None:
            return None, None, None, None
        lib = N.lib()
        B, Cc, H, W = feat.shape
        g_feat = None if g_feat is None else _c(g_feat)
        g_pooled = None if g_pooled is None else _c(g_pooled)
        ones = frozen_memo(("ones", Cc, feat.device), lambda: torch.ones(Cc, device=feat.device, dtype=torch.float32))
        g_pre = torch.empty_like(feat)
        N.check(_timed("stem_bwd", lambda: lib.dmh_stem_bn_relu_pool_bwd(N.ptr(feat), N.ptr(arg), N.ptr(g_feat),
                                                                        N.ptr(g_pooled), N.ptr(ones), B, Cc, H, W,
                                                                        N.ptr(g_pre), N.stream()), 12 * feat.numel()))
        if weight is not None and g_pre.numel() < (1 << 31) and Cc <= 65535:
            gx, gw, gb, _ = _bn_backward_fused(g_pre, x, None, weight, mean, invstd, False)
            return gx, gw, gb, None
        gx, gw, gb = _bn_backward(g_pre, x, weight, ctx.bn, mean, invstd, ctx.eps,
                                  [ctx.needs_input_grad[0], weight is not None and ctx.needs_input_grad[1],
                                   weight is not None and ctx.needs_input_grad[2]])
        return gx, gw, gb, None


def stem_bn_relu_pool_train(bn, x):
    """(relu(bn(x)), maxpool3x3/2(relu(bn(x)))) for an nn.BatchNorm2d in train mode; H and W even."""
    feat, pooled, _ = _StemTrain.apply(_c(x), bn.weight, bn.bias, bn)
    return feat, pooled


def stem_bn_relu_pool(x, scale, shift):
    """(ReLU(BN_eval(x)), MaxPool2d(3, 2, 1) of it) in one pass -- the encoder stem of
    MD2/networks/resnet_encoder.py:88-91 (features[0] and the input of layer1).  H and W must be even."""
    _reject_affine_grad("stem_bn_relu_pool", scale, shift)
    feat, pooled, _ = _StemBnReluPool.apply(_c(x), _c(scale.detach()), _c(shift.detach()))
    return feat, pooled


# ---------------------------------------------------------------------------------------------------------------
# K10: 3x3 stride-1 convolution, Winograd F(2x2,3x3) on the fp32 matrix cores (forward and backward-data); weight gradients:
# K13 / K16 / K18 by channel counts.  Dispatch is by shape: the kernel wins where a launch fills the chip with >= 64 output
# channels (tools/wino_bench.py, profiles/); everything else is the ATen/MIOpen convolution.
# ---------------------------------------------------------------------------------------------------------------
WINO_ENABLED = os.environ.get("DMH_WINO", "1") != "0"
_wino_frozen = 0
_wino_cache = {}


@contextlib.contextmanager
def frozen_weights():
    """Scope in which the network parameters are constants (an attack: torchattacks/attack.py brackets it with
    model.eval() and differentiates w.r.t. the perturbation only -- phy_obj_atk.py:96, phy_obj_atk_l0.py:134,
    pgd_depth.py:72).  Inside, the Winograd-transformed filters are computed once per weight tensor instead of once
    per call (the cache is dropped on exit) and ops.conv3x3 produces no weight/bias gradients: a custom autograd
    Function cannot see that torch.autograd.grad() was asked for the input gradient only, and the weight-gradient
    convolutions would otherwise run in every attack step just to be thrown away."""
    global _wino_frozen
    _wino_frozen += 1
    try:
        yield
    finally:
        _wino_frozen -= 1
        if _wino_frozen == 0:
            _wino_cache.clear()


def weights_frozen():
    """True inside a frozen_weights() scope (network parameters are constants there)."""
    return _wino_frozen > 0


def frozen_memo(key, fn):
    """fn() memoised for the lifetime of the enclosing frozen_weights() scope (parameters are constants there);
    outside a scope fn() is simply evaluated."""
    if not _wino_frozen:
        return fn()
    if key not in _wino_cache:
        _wino_cache[key] = fn()
    return _wino_cache[key]


def _wino_filter(weight, backward, scale=None, k17=False):
    """Winograd-transformed filter of the forward (backward=False) or backward-data pass, in K10's layout or (``k17``) K17's;
    `scale` (K10) folds a per-channel factor of the forward OUTPUT (an eval-mode BatchNorm) into it."""
    lib = N.lib()
    K, Cc = weight.shape[0], weight.shape[1]
    key = (weight.data_ptr(), weight._version, bool(backward), "k17" if k17 else None if scale is None else scale.data_ptr())
    if _wino_frozen and key in _wino_cache:
        return _wino_cache[key]
    if key[3] is None and not _wino_frozen:
        ready = _wino_ready.get((key[0], key[2]))      # transformed ahead of its use by wino_prefetch()
        if ready is not None and ready[0] == key[1] and ready[1].device == weight.device:
            return ready[1]
    n_out, n_in = (Cc, K) if backward else (K, Cc)
    size = lib.dmh_wino32_weight_size(n_out, n_in) if k17 else lib.dmh_wino_weight_size(n_out, n_in)
    U = torch.empty(size, device=weight.device, dtype=torch.float32)
    if k17:
        N.check(lib.dmh_wino32_weight_transform(N.ptr(_c(weight.detach())), K, Cc, int(backward), N.ptr(U), N.stream()))
    else:
        N.check(lib.dmh_wino_weight_transform_scaled(N.ptr(_c(weight.detach())), K, Cc, int(backward), N.ptr(scale), N.ptr(U),
                                                     N.stream()))
    if _wino_frozen:
        _wino_cache[key] = U
    return U


WINO_PREFETCH = os.environ.get("DMH_WINO_PREFETCH", "1") != "0"     # A/B switch: 0 = every filter transformed at its first use
_wino_ready = {}        # (weight pointer, backward) -> (weight version, U, weight): the filters of ONE pass outside a
                        # frozen_weights() scope (the train pass: forward forms now, backward-data forms for its backward); an
                        # entry keeps its weight tensor alive, so the pointer cannot come to name another tensor's data


_wino_pass = None       # inside wino_pass(): [has this pass emptied the table yet]


@contextlib.contextmanager
def wino_pass():
    """One train pass with several encoders (the depth and the pose encoder): inside, only the FIRST ``fresh`` prefetch empties
    the table of ready filters, so that the second encoder's prefetch leaves the first one's backward-data forms where the
    backward will look for them.  Outside such a scope every ``fresh`` prefetch empties it, as one encoder per pass wants."""
    global _wino_pass
    prev, _wino_pass = _wino_pass, [False]
    try:
        yield
    finally:
        _wino_pass = prev


def wino_prefetch(jobs, fresh=False):
    """Transform many K10 filters in ONE launch (dmh_wino_weight_transform_batch) ahead of their use: ``jobs`` = iterable of
    (weight [K, C, 3, 3], backward, scale or None) -- what _wino_filter() will be asked for.  A step needs every filter in its
    forward and its backward-data form, for the attack's frozen weights (BatchNorm scale folded in) and again for the train
    pass: 76 launches of 5-20 us when each is made at its first use.  Forms the kernel does not take (input channels of the pass
    not a multiple of 8) are skipped; whatever is not prefetched is still transformed on demand.  Inside frozen_weights() the
    results join that scope's cache (scaled forms included); outside it only unscaled forms are taken, into a table that the
    first prefetch of the next pass (``fresh``: the encoder's) empties.  Returns the number of filters transformed."""
    if not (WINO_ENABLED and WINO_PREFETCH):
        return 0
    lib = N.lib()
    todo, keep = [], []
    if fresh and not _wino_frozen:
        if _wino_pass is None or not _wino_pass[0]:
            _wino_ready.clear()
        if _wino_pass is not None:
            _wino_pass[0] = True
    for weight, backward, scale in jobs:
        if not (weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3)):
            continue
        K, Cc = weight.shape[0], weight.shape[1]
        n_out, n_in = (Cc, K) if backward else (K, Cc)
        if not _k10_channels(n_in, n_out):             # not a K10 shape in this direction
            continue
        if scale is not None and not _wino_frozen:     # a scale is a temporary: only a frozen scope's cache may key on it
            continue
        sc = None if scale is None else _c(scale.detach())
        key = (weight.data_ptr(), weight._version, bool(backward), None if sc is None else sc.data_ptr())
        if _wino_frozen and key in _wino_cache:
            continue
        # (outside a frozen scope a job is always done: an entry of an earlier call may predate a change of the weight that
        #  did not bump its version counter -- p.data.copy_(...))
        U = torch.empty(lib.dmh_wino_weight_size(n_out, n_in), device=weight.device, dtype=torch.float32)
        w = _c(weight.detach())
        keep.append((w, sc))
        todo.append((N.ptr(w), N.ptr(sc), N.ptr(U), K, Cc, int(bool(backward))))
        if _wino_frozen:
            _wino_cache[key] = U
        else:
            _wino_ready[(key[0], key[2])] = (key[1], U, weight)
    if todo:
        arr = (N.WinoWtJob * len(todo))()
        for j, (w, sc, U, K, Cc, bw) in enumerate(todo):
            arr[j].w, arr[j].scale, arr[j].U, arr[j].K, arr[j].C, arr[j].backward = w, sc, U, K, Cc, bw
        N.check(lib.dmh_wino_weight_transform_batch(arr, len(todo), N.stream()))
    return len(todo)


WINO_SK = os.environ.get("DMH_WINO_SK", "1") != "0"       # A/B switch: stream-K decomposition of the plain K10 launches
# work items below which MIOpen is level or ahead.  200 until round 5: measured with whole items only.  With the
# stream-K forms a launch of 64 items (or 512 (item, chunk) units) already beats the library's fixed costs: the strong-scaling
# share (train batch 4, 2 attack scenes) 50.2 -> 38.5 ms per step at 75 / 50 / 35 alike, batch 4 + 12 scenes and the headline
# batch unchanged (round 6, with a switch since removed)
_WINO_MIN_ITEMS = 64
_WINO_MIN_FILL = 0.5        # real tiles / tiles of the regions below which MIOpen is ahead


def _k10_channels(n_in, n_out):
    """Channel counts of a pass that K10 (64 output channels per work item, 8 input channels per chunk) takes."""
    return n_in % 8 == 0 and n_in >= 24 and n_out >= 64


def _k17_channels(n_in, n_out):
    """Channel counts of a pass that K17 takes: 32 or 96 output channels, which K10's 64-channel items would half-fill."""
    return n_in % 8 == 0 and n_in >= 24 and n_out % 32 == 0 and n_out % 64 != 0 and n_out <= 96


def _wino_ok(B, n_in, n_out, Ho, Wo, allow_split=True, allow_sk=False):
    """Shapes the Winograd-MFMA kernel takes: channel counts it tiles without waste and enough 64-channel x 64-tile
    work items to fill the chip (measured crossover, tools/wino_bench.py).  The thresholds are this rule's; the geometry of the
    launch they are applied to -- tile form, regions, the two-way channel split, stream-K -- is the library's own answer
    (dmh_wino_conv3x3_plan: what the launcher would do), not restated here."""
    if not WINO_ENABLED or not _k10_channels(n_in, n_out) or Ho % 2 or Wo % 2 or Ho < 2 or Wo < 2:
        return False
    if B * n_in * (Ho + 2) * (Wo + 2) >= (1 << 30):     # 32-bit byte offsets of the kernel's buffer loads: ATen beyond
        return False
    if n_in < 64 and n_out % 64:        # few chunks per item and a half-empty channel group: MIOpen is level or ahead
        return False
    ws_floats = 0       # no workspace, no stream-K: the switch is off, or a fused epilogue whose caller does not allow it
    if WINO_SK and (allow_split or allow_sk):
        try:
            ws_floats = _sk_ws_floats(torch.cuda.current_device()) if torch.cuda.is_available() else 2 * 256 * _SK_SLOT_FLOATS
        except Exception:
            ws_floats = 2 * 256 * _SK_SLOT_FLOATS
    return _wino_fills(B, n_in, n_out, Ho, Wo, 0 if allow_split else 1, ws_floats, WINO_SK)


@functools.lru_cache(maxsize=4096)
def _wino_fills(B, n_in, n_out, Ho, Wo, epilogue, ws_floats, sk):
    """_wino_ok's thresholds on the launch plan of a shape, remembered: a step asks for the same few dozen shapes again and
    again.  Every input of the decision is an argument (``sk``: WINO_SK, which tests flip at run time, like WINO_ENABLED, which
    _wino_ok looks at before it comes here)."""
    plan = N.lib().dmh_wino_conv3x3_plan(B, n_in, n_out, Ho, Wo, 1, epilogue, ws_floats)
    if plan < 0:
        return False
    items = plan >> 8                                   # whole work items: regions x the channel split (bit 1)
    regions = items // (2 if plan & 2 else 1)
    # ragged image: too many empty tiles (e.g. 17 tile columns in a 32-wide region); a region has 64 tiles in every form
    if B * (Ho // 2) * (Wo // 2) < _WINO_MIN_FILL * (regions // -(-n_out // 64)) * 64:
        return False
    if plan & 1:        # the library would take the stream-K form: enough (item, chunk) units for it?
        if regions * (n_in // 8) >= 8 * _WINO_MIN_ITEMS:
            return True
        items = N.lib().dmh_wino_conv3x3_plan(B, n_in, n_out, Ho, Wo, 1, epilogue, 0) >> 8      # ... no: as whole items
    return items >= (_WINO_MIN_ITEMS if sk else max(_WINO_MIN_ITEMS, 200))     # whole items only: round 4's threshold


def _wrw_ok(x, g, K, Cc):
    """Shapes of K18 (Winograd-domain weight gradient): both channel counts multiples of 64 (64 x 64 blocks), or 32 k output
    channels with 96 k' / 64 k' input channels (32 x 96 / 32 x 64 blocks: upconv(1,1), upconv(1,0)); even output size, enough
    tile chunks (8 tiles) to give every workgroup of a (k-block, c-block) pair a few, tensors below 4 GB."""
    if not WINO_ENABLED or g.shape[2] % 2 or g.shape[3] % 2:
        return False
    if K % 64 == 0 and Cc % 64 == 0:
        kch, cch = 64, 64
    elif K % 32 == 0 and Cc % 96 == 0:
        kch, cch = 32, 96
    elif K % 32 == 0 and Cc % 64 == 0:
        kch, cch = 32, 64
    else:
        return False
    pad = (g.shape[2] + 2 - x.shape[2]) // 2
    if pad not in (0, 1) or (pad == 1 and x.shape[3] % 16):
        return False
    if x.numel() * 4 > 0xFFFFFF00 or g.numel() >= (1 << 30):      # the kernel's own limits (DMH_REQUIRE in csrc/wino_wrw.hip)
        return False
    chunks = g.shape[0] * (g.shape[2] // 2) * -(-(g.shape[3] // 2) // 8)
    return chunks * (K // kch) * (Cc // cch) >= 1024


def _wino32_ok(B, n_in, n_out, Ho, Wo):
    """Shapes of K17, the 32-output-channel form of K10 (work item 32 channels x 4 x 32 tiles): output channels a multiple
    of 32 that K10's 64-channel items would half-fill, enough items to cover the chip and few empty tiles."""
    if (not WINO_ENABLED or not _k17_channels(n_in, n_out) or n_in < 32 or Ho % 2 or Wo % 2
            or B * n_in * (Ho + 2) * (Wo + 2) >= (1 << 30)):
        return False        # (32 -> 96, the backward-data pass of upconv(1,1): 509 us against MIOpen's 566, tools/wino32_bench.py)
    ht, wt = Ho // 2, Wo // 2
    rows, cols = -(-ht // 4) * 4, -(-wt // 32) * 32
    if ht * wt < 0.8 * rows * cols:
        return False
    return B * (rows // 4) * (cols // 32) * (n_out // 32) >= 400


_sk_ws = {}         # (device, stream) -> workspace of the stream-K launches (caller-owned: the library keeps nothing)
_SK_SLOT_FLOATS = 16384         # one partial work item: 16 output channels x 256 threads x float4


def _sk_ws_floats(device):
    """2 slots per workgroup, one workgroup per CU (MI355X: 256 CUs = 32 MB): sized from the device, not assumed."""
    return 2 * torch.cuda.get_device_properties(device).multi_processor_count * _SK_SLOT_FLOATS


def _sk_workspace(device):
    """The library decides per launch (dmh_wino_conv3x3_ws / dmh_wino32_conv3x3_ws): stream-K where whole work items would leave
    the chip idle for part of a round.  ONE buffer per device AND stream -- the launches of a stream are ordered, and the fix-up
    kernel that reads the partial items is enqueued right behind the kernel that wrote them; two streams that run convolutions
    side by side must not share the slots."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    ws = _sk_ws.get(key)
    if ws is None:
        ws = _sk_ws[key] = torch.empty(_sk_ws_floats(device), device=device, dtype=torch.float32)
    return ws


def _k10_act(lib, x, U, bias, res, relu, B, Cc, K, H, W, pad, y, stream, workspace=True):
    """K10 with the fused epilogue.  ``workspace``: hand the library the stream-K workspace of the current device (it takes the
    decomposed form only for launches of few tile regions: layer4 at the attack batch); without one it runs whole items."""
    if not (workspace and WINO_SK):
        return lib.dmh_wino_conv3x3_act(x, U, bias, res, relu, B, Cc, K, H, W, pad, y, stream)
    ws = _sk_workspace(torch.device("cuda", torch.cuda.current_device()))
    return lib.dmh_wino_conv3x3_act_ws(x, U, bias, res, relu, B, Cc, K, H, W, pad, y, N.ptr(ws), ws.numel(), stream)


def _k10(x, w, scale, *, backward, bias=None, res=None, flag, workspace, pad=1, count_filter=False):
    """One K10 launch with the fused epilogue: conv3x3(x) with the filter ``w`` (``backward``: its backward-data pass on a
    gradient x), ``scale`` folded into the filter, + ``bias``, then by ``flag``: 0 = + res, 1 = ReLU(. + res), 2 = masked by
    [res > 0].  ``workspace``: see _k10_act -- the block nodes pass True; the encoder heads' window launches pass False, since a
    workspace lets the library choose the stream-K form, which sums in another order.  ``count_filter``: the profile's byte
    count includes the filter image."""
    B, Cc, H, W = x.shape
    K = w.shape[1] if backward else w.shape[0]
    y = torch.empty((B, K, H + 2 * pad - 2, W + 2 * pad - 2), device=x.device, dtype=torch.float32)
    U = _wino_filter(w, backward, scale)
    nb = 4 * (x.numel() + y.numel() * (1 if res is None else 2)) + (4 * U.numel() if count_filter else 0)
    N.check(_timed("wino_conv3x3", lambda: _k10_act(N.lib(), N.ptr(x), N.ptr(U), N.ptr(bias), N.ptr(res), int(flag), B, Cc, K, H, W,
                                                    pad, N.ptr(y), N.stream(), workspace), nb, 18 * Cc * y.numel()))
    return y


def _relu_mask_bwd(y, g):
    """g * [y > 0] on whole tensors: the K9 backward kernel with a unit scale."""
    B, Cc = g.shape[0], g.shape[1]
    ones = frozen_memo(("ones", Cc, g.device), lambda: torch.ones(Cc, device=g.device, dtype=torch.float32))
    g_pre = torch.empty_like(g)
    N.check(_timed("bn_act_bwd", lambda: N.lib().dmh_bn_act_bwd(N.ptr(y), N.ptr(g), N.ptr(ones), B, Cc, g.numel() // (B * Cc), 1,
                                                               N.ptr(g_pre), None, N.stream()), 12 * g.numel()))
    return g_pre


def _wino_conv(x, U, bias, K, pad, k17=False):
    """The plain K10 launch, or (``k17``) K17's, on a transformed filter U."""
    lib = N.lib()
    B, Cc, H, W = x.shape
    y = torch.empty((B, K, H + 2 * pad - 2, W + 2 * pad - 2), device=x.device, dtype=torch.float32)
    nb = 4 * (x.numel() + y.numel()) + 4 * U.numel()
    ws = _sk_workspace(x.device) if WINO_SK else None
    args = (N.ptr(x), N.ptr(U), N.ptr(bias), B, Cc, K, H, W, pad, N.ptr(y), N.ptr(ws), 0 if ws is None else ws.numel(), N.stream())
    if k17:
        N.check(_timed("wino32_conv3x3", lambda: lib.dmh_wino32_conv3x3_ws(*args), nb, 18 * Cc * y.numel()))
    else:
        N.check(_timed("wino_conv3x3", lambda: lib.dmh_wino_conv3x3_ws(*args), nb, 18 * Cc * y.numel()))
    return y


def _small_ok(n_in, n_out):
    """Channel counts of the K11 direct-MFMA kernel (last decoder stage, disparity heads)."""
    return WINO_ENABLED and ((n_in in (1, 2, 3, 4, 16) and n_out <= 32) or (n_in == 32 and n_out <= 16))


def _small_conv(x, weight, bias, pad, backward):
    lib = N.lib()
    if x.numel() >= (1 << 30):      # beyond the 32-bit byte offsets of the kernel's buffer loads: ATen, as for K15 / K18
        if backward:
            return torch.nn.functional.conv_transpose2d(x, weight, None, 1, 2 - pad)
        return torch.conv2d(x, weight, bias, 1, pad)
    B, _, H, W = x.shape
    Kw, Cw = weight.shape[0], weight.shape[1]
    n_out = Cw if backward else Kw
    y = torch.empty((B, n_out, H + 2 * pad - 2, W + 2 * pad - 2), device=x.device, dtype=torch.float32)
    nb = 4 * (x.numel() + y.numel())
    N.check(_timed("conv3x3_small", lambda: lib.dmh_conv3x3_small(N.ptr(x), N.ptr(_c(weight.detach())), N.ptr(bias), B, Kw,
                                                                 Cw, H, W, pad, int(backward), N.ptr(y), N.stream()), nb,
                   18 * x.shape[1] * y.numel()))
    return y


def _head_conv(x, weight, bias, pad):
    """K13: the 3x3 convolution to ONE output channel (the disparity heads)."""
    B, Cc, H, W = x.shape
    y = torch.empty((B, 1, H + 2 * pad - 2, W + 2 * pad - 2), device=x.device, dtype=torch.float32)
    N.check(_timed("conv3x3_head", lambda: N.lib().dmh_conv3x3_head(N.ptr(x), N.ptr(_c(weight.detach())), N.ptr(bias), B, Cc, H, W,
                                                                   pad, N.ptr(y), N.stream()), 4 * (x.numel() + y.numel())))
    return y


def _head_conv_bwd(g, weight):
    """K13's backward-data pass at forward padding 0: one gradient plane in registers, C planes streamed out."""
    B, Cc, H, W = g.shape[0], weight.shape[1], g.shape[2] + 2, g.shape[3] + 2
    g_x = torch.empty((B, Cc, H, W), device=g.device, dtype=torch.float32)
    N.check(_timed("conv3x3_head_bwd", lambda: N.lib().dmh_conv3x3_head_bwd_data(
        N.ptr(g), N.ptr(_c(weight.detach())), B, Cc, H, W, N.ptr(g_x), N.stream()), 4 * (g_x.numel() + g.numel())))
    return g_x


def _direct_wrw(x, g, weight, pad, need_b):
    """(g_w, g_b or None) of a convolution to ONE output channel (K13: a strip reduction, the disparity heads) or to 16 (K16:
    pixel axis on the MFMA, persistent workgroups, the last decoder stage) in place of MIOpen's implicit GEMMs."""
    lib = N.lib()
    B, Cc, H, W = x.shape
    K, nb = weight.shape[0], 4 * (x.numel() + g.numel())
    n_part = lib.dmh_conv3x3_head_wrw_partials_size(B, Cc, H, W, pad) if K == 1 else lib.dmh_conv3x3_small_wrw_partials_size(Cc)
    part = torch.empty(n_part, device=g.device, dtype=torch.float32)
    g_w = torch.empty_like(weight)
    g_b = torch.empty(K, device=g.device, dtype=torch.float32) if need_b else None
    args = (N.ptr(x), N.ptr(g), B, Cc, H, W, pad, N.ptr(part), N.ptr(g_w), N.ptr(g_b), N.stream())
    if K == 1:
        N.check(_timed("conv3x3_head_wrw", lambda: lib.dmh_conv3x3_head_wrw(*args), nb))
    else:
        N.check(_timed("conv3x3_small_wrw", lambda: lib.dmh_conv3x3_small_wrw(*args), nb, 18 * Cc * g.numel()))
    return g_w, g_b


def _wino_wrw(x, g, K, pad):
    """K18, the [K, C, 3, 3] weight gradient in the Winograd domain on the fp32 MFMA (MIOpen: NHWC implicit GEMMs between layout
    transposes, with atomics).  The bias gradient is a plain reduction of g and the caller's."""
    lib = N.lib()
    B, Cc, H, W = x.shape
    ws = torch.empty(lib.dmh_wino_wrw_workspace_size(B, Cc, K, H, W, pad), device=g.device, dtype=torch.float32)
    g_w = torch.empty((K, Cc, 3, 3), device=g.device, dtype=torch.float32)
    N.check(_timed("wino_wrw", lambda: lib.dmh_wino_wrw(N.ptr(x), N.ptr(g), B, Cc, K, H, W, pad, N.ptr(ws), N.ptr(g_w), N.stream()),
                   4 * (x.numel() + g.numel()), 18 * Cc * g.numel()))
    return g_w


def _wrw_route(x, g, K, Cc):
    """Which kernel takes the weight gradient of a [K, C, 3, 3] convolution of x with output gradient g: "k13" (one output
    channel), "k16" (16 output channels from 16 or 32), "k18" (_wrw_ok) or None (ATen)."""
    if WINO_ENABLED and K == 1 and Cc * x.shape[2] * x.shape[3] < (1 << 29):
        return "k13"
    if WINO_ENABLED and K == 16 and Cc in (16, 32) and Cc * x.shape[2] * x.shape[3] < (1 << 28):
        return "k16"
    return "k18" if _wrw_ok(x, g, K, Cc) else None


def _conv3x3_route(B, n_in, n_out, H, W, pad, backward, capable_only=False):
    """THE rule of which kernel takes a 3x3 convolution pass: "k10", "k17", "k13", "k11" or None (the caller's fall-back).  Host
    logic only, in the terms of the pass: n_in -> n_out channels on a [B, n_in, H, W] input with zero padding ``pad``;
    ``backward``: it is a backward-data pass -- the same convolution on the output gradient with pad = 2 - the forward padding.
    A kernel is named where it WINS (the thresholds of _wino_ok / _wino32_ok, K13's tile count); with ``capable_only`` wherever
    it CAN run (channel and size limits): the attack's window launches, smaller than the shapes the thresholds were measured on."""
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    if capable_only:
        if not WINO_ENABLED or B * n_in * H * W >= (1 << 30):
            return None
        if Ho % 2 == 0 and Wo % 2 == 0 and Ho >= 2 and Wo >= 2:
            if _k17_channels(n_in, n_out):          # (96 output channels: K17's here, K10's by throughput where it fills the chip)
                return "k17"
            if _k10_channels(n_in, n_out):
                return "k10"
    elif _wino_ok(B, n_in, n_out, Ho, Wo):
        return "k10"
    elif _wino32_ok(B, n_in, n_out, Ho, Wo):
        return "k17"
    if backward:        # disparity head, backward-data at forward padding 0: one gradient plane in, <= 64 planes out
        head = n_in == 1 and pad == 2 and n_out % 4 == 0 and n_out <= 64 and Ho >= 3 and Wo >= 3
    else:               # disparity head: the strip kernel at padding 0, the tiled one where its 8 x 64 tiles fill the chip
        head = n_out == 1 and ((pad == 0 and n_in % 4 == 0) or (
            not capable_only and n_in % 16 == 0 and n_in >= 32 and B * -(-Ho // 8) * -(-Wo // 64) >= 512))
    if WINO_ENABLED and head:
        return "k13"
    return "k11" if _small_ok(n_in, n_out) else None


def _conv3x3_routed(x, weight, bias, pad, backward=False, scale=None, k10_only=False, capable_only=False):
    """conv2d(x, weight, bias, padding=pad) -- with ``backward`` the backward-data pass of ``weight`` on a gradient x, pad = 2 -
    the forward padding -- on the kernel _conv3x3_route() names, or None: the fall-back is the caller's.  ``k10_only``: the
    sites around K10's fused epilogue, which take K10 or their library path; their ``scale`` is folded into K10's filter."""
    B, n_in, H, W = x.shape
    n_out = weight.shape[1] if backward else weight.shape[0]
    route = _conv3x3_route(B, n_in, n_out, H, W, pad, backward, capable_only)
    if route == "k10":
        return _wino_conv(x, _wino_filter(weight, backward, scale), bias, n_out, pad)
    if route is None or k10_only:
        return None
    if route == "k17":
        return _wino_conv(x, _wino_filter(weight, backward, k17=True), bias, n_out, pad, k17=True)
    if route == "k13":
        return _head_conv_bwd(x, weight) if backward else _head_conv(x, weight, bias, pad)
    return _small_conv(x, weight, bias, pad, backward)


class _Conv3x3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, pad):
        ctx.pad = pad
        ctx.has_bias = bias is not None
        ctx.params_const = _wino_frozen > 0
        ctx.save_for_backward(x, weight)
        y = _conv3x3_routed(x, weight, None if bias is None else _c(bias.detach()), pad)
        return torch.conv2d(x, weight, bias, 1, pad) if y is None else y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        K, Cc = weight.shape[0], weight.shape[1]
        pad = ctx.pad
        g = _c(g)
        need_x = ctx.needs_input_grad[0]
        need_w = ctx.needs_input_grad[1] and not ctx.params_const
        need_b = ctx.has_bias and ctx.needs_input_grad[2] and not ctx.params_const
        g_x = g_w = g_b = None
        if need_x:
            g_x = _conv3x3_routed(g, weight, None, 2 - pad, backward=True)
            need_x = g_x is None
        route = _wrw_route(x, g, K, Cc) if need_w else None
        if route in ("k13", "k16"):
            g_w, g_b = _direct_wrw(x, g, weight, pad, need_b)
        elif route == "k18":
            g_w = _wino_wrw(x, g, K, pad)
            if need_b:
                g_b = channel_sum(g) if K <= 65535 else g.sum((0, 2, 3))
        if route is not None:
            need_w = need_b = False
        if need_x or need_w or need_b:
            r = torch.ops.aten.convolution_backward(g, x, weight, [K] if ctx.has_bias else None, [1, 1], [pad, pad], [1, 1],
                                                    False, [0, 0], 1, [need_x, need_w, need_b])
            g_x = r[0] if need_x else g_x
            g_w = r[1] if need_w else g_w
            g_b = r[2] if need_b else g_b
        return g_x, g_w, g_b, None


class _ConvBnAct(torch.autograd.Function):
    """conv3x3 -> eval-mode BatchNorm -> (+ residual) -> ReLU as ONE K10 launch (scale folded into the filter, shift as
    the bias, residual and ReLU in the output transform).  Backward: ReLU mask (one K9 pass), then the backward-data
    K10 launch on the filter with the scale folded in."""

    @staticmethod
    def forward(ctx, x, weight, scale, shift, residual, relu, pad):
        y = _k10(x, weight, scale, backward=False, bias=shift, res=residual, flag=int(relu), workspace=True, pad=pad,
                 count_filter=True)
        ctx.save_for_backward(x, weight, scale, y if relu else None)
        ctx.pad, ctx.relu = pad, bool(relu)
        ctx.res_grad = residual is not None and residual.requires_grad
        ctx.params_const = _wino_frozen > 0
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, scale, y = ctx.saved_tensors
        g = _c(g)
        g_pre = _relu_mask_bwd(y, g) if ctx.relu else g         # it is also the residual's gradient
        g_x = g_w = None
        need_w = ctx.needs_input_grad[1] and not ctx.params_const
        if ctx.needs_input_grad[0]:
            g_x = _conv3x3_routed(g_pre, weight, None, 2 - ctx.pad, backward=True, scale=scale, k10_only=True)
            if g_x is None:
                g_conv = g_pre * scale.view(1, -1, 1, 1)
                g_x = torch.ops.aten.convolution_backward(g_conv, x, weight, None, [1, 1], [ctx.pad] * 2, [1, 1], False,
                                                          [0, 0], 1, [True, False, False])[0]
        if need_w:
            g_conv = g_pre * scale.view(1, -1, 1, 1)
            g_w = torch.ops.aten.convolution_backward(g_conv, x, weight, None, [1, 1], [ctx.pad] * 2, [1, 1], False, [0, 0],
                                                      1, [False, True, False])[1]
        return g_x, g_w, None, None, (g_pre if ctx.res_grad else None), None, None


def conv3x3_bn_act(x, weight, scale, shift, residual=None, relu=True, padding=1):
    """act(BatchNorm_eval(conv3x3(x, weight)) (+ residual)) with BatchNorm given as its per-channel (scale, shift): the
    BasicBlock pattern of the encoder in eval() (MD2/networks/resnet_encoder.py:85-98).  One K10 launch where the shape
    fills the chip, otherwise conv3x3 followed by the K9 bn_act pass.  No gradient flows to scale / shift."""
    B, Cc, H, W = x.shape
    _reject_affine_grad("conv3x3_bn_act", scale, shift)
    if x.is_cuda and _wino_ok(B, Cc, weight.shape[0], H + 2 * padding - 2, W + 2 * padding - 2, allow_split=False, allow_sk=True):
        return _ConvBnAct.apply(_c(x), weight, _c(scale.detach()), _c(shift.detach()),
                                None if residual is None else _c(residual), bool(relu), int(padding))
    return bn_act(conv3x3(x, weight, None, padding), scale, shift, residual, relu)


def conv3x3(x, weight, bias=None, padding=1):
    """nn.Conv2d(C, K, 3, stride=1, padding=padding) with zero padding 0, 1 or 2 -- the 3x3 convolutions of the ResNet
    encoder (torchvision BasicBlock under MD2/networks/resnet_encoder.py:85-98) and of the depth decoder
    (MD2/layers.py:127-141 Conv3x3).  Forward and the gradient w.r.t. x run the K10 / K17 / K11 / K13 kernels by shape (K10
    where >= 64 output channels fill the chip), the weight gradient K13 / K16 / K18 by channel counts (fixed-order sums); the
    remaining shapes are ATen/MIOpen."""
    if padding not in (0, 1, 2) or weight.shape[2:] != (3, 3):
        raise RuntimeError("conv3x3: 3x3 kernel with padding 0, 1 or 2 expected")
    _need_cuda(x)
    return _Conv3x3.apply(_c(x), weight, bias, int(padding))


# ---------------------------------------------------------------------------------------------------------------
# K36: ManyDepth's reduce_conv in the degenerate call (no lookup frames: the D cost-volume channels are exact zeros)
# ---------------------------------------------------------------------------------------------------------------
_reduce_slices = {}     # weight pointer -> (weight version, weight[:, :C] contiguous, weight): kept like the Winograd filters


def _reduce_slice(weight, Cc, fresh=False):
    """The contiguous ``weight[:, :C]`` of a [K, C + D, 3, 3] filter, cached on (data_ptr, _version) so that a pass slices it
    once (forward; the backward finds it).  ``fresh``: slice again whatever the cache says -- the train pass's prefetch asks for
    that on every forward, as wino_prefetch re-transforms every filter, because a write through ``p.data`` (ddp.broadcast_parameters,
    a weight swap) changes the weight without changing its version.  An entry keeps its weight tensor alive, so the pointer cannot
    come to name another tensor's data; at most 8 entries."""
    key = (weight.data_ptr(), Cc)
    hit = _reduce_slices.get(key)
    if not fresh and hit is not None and hit[0] == weight._version and hit[1].device == weight.device:
        return hit[1]
    if len(_reduce_slices) >= 8:
        _reduce_slices.clear()
    wc = weight.detach()[:, :Cc].contiguous()
    _reduce_slices[key] = (weight._version, wc, weight)
    return wc


def _reduce_act_ok(B, Cc, K, H, W):
    """K10 with its fused bias + ReLU epilogue takes the shape (the rule of conv3x3_bn_act)."""
    return _wino_ok(B, Cc, K, H, W, allow_split=False, allow_sk=True)


def reduce_bwd_mask(g, y, Cc=None):
    """(g * [y > 0], per-(channel, slab) partial sums of it): K36's first backward launch.  ``Cc``: the node's input channels
    (the C of the entry points' checks; K when the pass is used on its own)."""
    lib = N.lib()
    B, K = g.shape[0], g.shape[1]
    Cc = K if Cc is None else Cc
    HW = g.numel() // (B * K)
    n = lib.dmh_reduce_bwd_partials_size(B, Cc, K, HW)
    if n < 0:
        N.check(1)
    part = torch.empty(n, device=g.device, dtype=torch.float32)
    g_pre = torch.empty_like(g)
    N.check(_timed("reduce_bwd_mask", lambda: lib.dmh_reduce_bwd_mask(N.ptr(g), N.ptr(y), B, Cc, K, HW, N.ptr(g_pre), N.ptr(part),
                                                                      N.stream()), 12 * g.numel()))
    return g_pre, part


def reduce_bwd_rounds(B, K, HW):
    """fp32 roundings on the longest path of one bias-gradient sum of K36 (csrc/reduce_node.hip's header derives it)."""
    return int(N.lib().dmh_reduce_bwd_rounds(B, K, K, HW))


def _lib_deterministic():
    """Scope for K36's library fall-backs (shapes K10 / K18 do not take): the library's deterministic algorithms only -- its
    default weight-gradient and backward-data solvers for small maps add with atomics, and the node promises the same bits twice."""
    cd = torch.backends.cudnn
    return cd.flags(enabled=cd.enabled, benchmark=cd.benchmark, deterministic=True, allow_tf32=cd.allow_tf32)


def reduce_conv_fwd_launch(x, weight, bias):
    """K36 forward on contiguous fp32 CUDA tensors: one K10 launch with the bias + ReLU epilogue where the shape fills the chip,
    else the convolution ops.conv3x3 would pick + K36's bias_relu pass (in place)."""
    B, Cc, H, W = x.shape
    K = weight.shape[0]
    wc = _reduce_slice(weight, Cc)
    b = _c(bias.detach())
    if _reduce_act_ok(B, Cc, K, H, W):
        return _k10(x, wc, None, backward=False, bias=b, flag=1, workspace=True, count_filter=True)
    z = _conv3x3_routed(x, wc, None, 1, k10_only=True)
    if z is None:
        with _lib_deterministic():
            z = torch.conv2d(x, wc, None, 1, 1)
    N.check(_timed("reduce_bias_relu", lambda: N.lib().dmh_reduce_bias_relu(N.ptr(z), N.ptr(b), B, Cc, K, H * W, N.ptr(z), N.stream()),
                   8 * z.numel()))
    return z


def reduce_conv_bwd_launch(g, x, weight, y, need_x=True, need_params=True):
    """K36 backward: (g_x, g_weight, g_bias).  The mask pass (g_pre and the bias gradient's partial sums in one read of g and y),
    K10 backward-data and K18 on g_pre (the library's kernels for shapes they do not take), and the finish launch: the bias
    gradient, and the [K, C, 3, 3] gradient laid into the [K, C + D, 3, 3] layout with exact zeros behind it.  Without
    ``need_params`` (inside frozen_weights()) the mask pass alone precedes backward-data; g_weight and g_bias are None."""
    B, Cc, H, W = x.shape
    K, D = weight.shape[0], weight.shape[1] - Cc
    lib = N.lib()
    if need_params:
        g_pre, part = reduce_bwd_mask(g, y, Cc)
    else:
        g_pre = _relu_mask_bwd(y, g)
    wc = _reduce_slice(weight, Cc)
    g_x = g_w = g_b = None
    if need_x:
        g_x = _conv3x3_routed(g_pre, wc, None, 1, backward=True, k10_only=True)
        if g_x is None:
            with _lib_deterministic():
                g_x = torch.ops.aten.convolution_backward(g_pre, x, wc, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                          [True, False, False])[0]
    if need_params:
        if _wrw_ok(x, g_pre, K, Cc):        # the node considers K18 only (not _wrw_route's K13 / K16)
            dw = _wino_wrw(x, g_pre, K, 1)
        else:
            with _lib_deterministic():
                dw = _c(torch.ops.aten.convolution_backward(g_pre, x, wc, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                            [False, True, False])[1])
        g_w = torch.empty(tuple(weight.shape), device=g.device, dtype=torch.float32)
        g_b = torch.empty(K, device=g.device, dtype=torch.float32)
        N.check(_timed("reduce_bwd_finish", lambda: lib.dmh_reduce_bwd_finish(N.ptr(part), N.ptr(dw), B, Cc, K, D, H * W, N.ptr(g_b),
                                                                              N.ptr(g_w), N.stream()),
                       4 * (g_w.numel() + dw.numel())))
    return g_x, g_w, g_b


class _ReduceConvDegenerate(torch.autograd.Function):
    """relu(conv3x3(x, weight[:, :C]) + bias) as one node (reduce_conv_fwd_launch / reduce_conv_bwd_launch).  Neither x with D
    zero channels nor a zero-padded filter ever exists."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        y = reduce_conv_fwd_launch(x, weight, bias)
        ctx.save_for_backward(x, weight, y)
        ctx.params_const = _wino_frozen > 0
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        need_params = (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) and not ctx.params_const
        g_x, g_w, g_b = reduce_conv_bwd_launch(_c(g), x, weight, y, ctx.needs_input_grad[0], need_params)
        return g_x, (g_w if ctx.needs_input_grad[1] else None), (g_b if ctx.needs_input_grad[2] else None)


def reduce_conv_degenerate_host(x, weight, bias):
    """The definition in torch, any device and dtype: relu(conv3x3(x, weight[:, :C]) + bias) == the reference's
    ``reduce_conv(cat([x, zeros(B, D, H, W)], 1))`` (manydepth2/networks/resnet_encoder.py:321 in the degenerate call).  The path
    of CPU tensors and the yardstick of the fused node."""
    Cc = x.shape[1]
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[1] < Cc:
        raise RuntimeError("reduce_conv_degenerate: weight must be [K, C + D, 3, 3] with C = x.shape[1]; got %s for %s"
                           % (tuple(weight.shape), tuple(x.shape)))
    return torch.relu(torch.nn.functional.conv2d(x, weight[:, :Cc], bias, 1, 1))


def _reduce_operands(x, weight, bias):
    """What K36 takes, checked once for ops.reduce_conv_degenerate and torch.ops.dmh.reduce_conv_degenerate alike."""
    _need_cuda(x)
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[1] < x.shape[1] or bias is None \
            or tuple(bias.shape) != (weight.shape[0],):
        raise RuntimeError("reduce_conv_degenerate: x [B,C,H,W], weight [K,C+D,3,3], bias [K] expected; got %s, %s, %s" % (
            tuple(x.shape), tuple(weight.shape), None if bias is None else tuple(bias.shape)))
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or bias.dtype != torch.float32:
        raise RuntimeError("libdmh_hip ops compute in fp32; got %s, %s, %s" % (x.dtype, weight.dtype, bias.dtype))
    if not (weight.is_cuda and bias.is_cuda):
        raise RuntimeError("libdmh_hip ops need CUDA (ROCm) tensors; got weight on %s, bias on %s" % (weight.device, bias.device))
    if x.shape[1] % 8 or weight.shape[0] % 8:
        raise RuntimeError("reduce_conv_degenerate: C and K must be multiples of 8; got C = %d, K = %d" % (x.shape[1], weight.shape[0]))


def reduce_conv_degenerate(x, weight, bias):
    """ManyDepth's ``reduce_conv`` when every lookup frame is missing -- the call the reference's trainer, wrapper and evaluation
    make: x [B, C, H, W], weight [K, C + D, 3, 3], bias [K] -> relu(conv3x3(x, weight[:, :C]) + bias) [B, K, H, W].  CUDA fp32
    tensors take K36 (one autograd node; weight.grad has the full [K, C + D, 3, 3] layout with exact zeros in [:, C:], sums in a
    fixed order); CPU tensors take reduce_conv_degenerate_host.  Inside frozen_weights() no parameter gradient is produced."""
    if not x.is_cuda:
        return reduce_conv_degenerate_host(x, weight, bias)
    _reduce_operands(x, weight, bias)
    return _ReduceConvDegenerate.apply(_c(x), weight, bias)


def _stem_wrw(x, g, weight, mean, std):
    """K21: dW of the 7x7/2 first convolution on (x - mean) / std, fixed-order sums on the fp32 MFMA; None when the shape is
    not the kernel's (3 -> 64 channels, even H, W a multiple of 8): the caller then takes ATen's."""
    B, Cin, H, W = x.shape
    if not WINO_ENABLED or tuple(weight.shape) != (64, 3, 7, 7) or Cin != 3 or x.numel() * 4 > 0xFFFFFF00:
        return None
    lib = N.lib()
    n = lib.dmh_stem_wrw_workspace_size(B, H, W)
    if n < 0:
        return None
    ws = torch.empty(n, device=x.device, dtype=torch.float32)
    g_w = torch.empty_like(weight, memory_format=torch.contiguous_format)
    N.check(_timed("stem_wrw", lambda: lib.dmh_stem_wrw(N.ptr(x), N.ptr(g), B, H, W, mean, std, N.ptr(ws), N.ptr(g_w),
                                                        N.stream()), 4 * (x.numel() + g.numel()), 2 * 147 * g.numel()))
    return g_w


class _StemConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        ctx.params_const = _wino_frozen > 0
        return torch.conv2d(x, weight, None, 2, 3)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        lib = N.lib()
        g = _c(g)
        B, Cin, H, W = x.shape
        K = weight.shape[0]
        g_x = g_w = None
        need_w = ctx.needs_input_grad[1] and not ctx.params_const
        if ctx.needs_input_grad[0]:
            g_x = torch.empty_like(x)
            nb = 4 * (g.numel() + g_x.numel())
            N.check(_timed("stem_conv_bwd", lambda: lib.dmh_conv7x7s2_bwd_data(N.ptr(g), N.ptr(_c(weight.detach())), B, K,
                                                                              Cin, H, W, N.ptr(g_x), N.stream()), nb,
                           2 * 49 * Cin * g.numel()))
        if need_w:
            g_w = _stem_wrw(x, g, weight, 0.0, 1.0)
            if g_w is None:
                g_w = torch.ops.aten.convolution_backward(g, x, weight, None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1,
                                                          [False, True, False])[1]
        return g_x, g_w


def stem_conv(x, weight):
    """nn.Conv2d(Cin, K, 7, stride=2, padding=3, bias=False) -- the encoder's first convolution
    (MD2/networks/resnet_encoder.py:88).  Forward is MIOpen, the weight gradient K21 (3 -> 64 channels; MIOpen otherwise); the gradient w.r.t. the image (what
    every attack step back-propagates to the patch) is the K12 gather kernel."""
    B, Cin, H, W = x.shape
    if (not x.is_cuda or not WINO_ENABLED or weight.shape[1:] != (Cin, 7, 7) or Cin > 4 or weight.shape[0] % 8 or H % 2
            or W % 2 or not x.requires_grad):
        return torch.conv2d(x, weight, None, 2, 3)
    return _StemConv.apply(_c(x), weight)


def _stem_conv_norm_fwd(x, weight, mean, std):
    """K14 on the whole frame: conv1((x - mean) / std), 3 -> 64 channels."""
    B, _, H, W = x.shape
    y = torch.empty((B, 64, H // 2, W // 2), device=x.device, dtype=torch.float32)
    N.check(_timed("stem_conv_fwd", lambda: N.lib().dmh_stem_conv_norm_fwd(N.ptr(x), N.ptr(_c(weight.detach())), B, H, W, mean, std,
                                                                          N.ptr(y), N.stream()), 4 * (x.numel() + y.numel()),
                   2 * 147 * y.numel()))
    return y


def _stem_w_over_std(weight, std):
    """d/dx of conv((x - mean) / std, w) = conv_bwd_data(g, w / std): the 1/std goes into the 9,408 filter taps (once per attack
    inside frozen_weights()) instead of a pass over the image gradient."""
    return frozen_memo(("stem_w_over_std", weight.data_ptr(), weight._version, std), lambda: _c(weight.detach() * (1.0 / std)))


def _stem_window_bwd(g_z, w_stem, org_z, org_d, size_d, H, W):
    """K12's window form, the tail of the windowed encoder heads' backward: d / d image [B,3,H,W] of conv1((x - 0.45) / 0.225)
    from the gradient ``g_z`` of a compact window of its output (origins ``org_z`` on the 1/2 map), written inside the image
    window (``org_d``, ``size_d``) and zero elsewhere."""
    B, _, hs, ws = g_z.shape
    hd, wd = size_d
    w_s = _stem_w_over_std(w_stem, 0.225)
    g_x = torch.zeros((B, 3, H, W), device=g_z.device, dtype=torch.float32)
    N.check(_timed("stem_conv_bwd_win", lambda: N.lib().dmh_conv7x7s2_bwd_data_win(
        N.ptr(g_z), N.ptr(w_s), N.ptr(org_d), N.ptr(org_z), B, 64, 3, H, W, hd, wd, hs, ws, N.ptr(g_x), N.stream()),
        4 * (g_z.numel() + B * 3 * hd * wd), 2 * 147 * 64 * B * (hd // 2) * (wd // 2)))
    return g_x


class _StemConvNorm(torch.autograd.Function):
    """K14 forward (normalisation + 7x7/2 convolution on the fp32 MFMA); backward: image gradient by K12 (scaled by 1/std),
    weight gradient by K21 (train pass only; ATen on the re-normalised image for widths that are not multiples of 8)."""

    @staticmethod
    def forward(ctx, x, weight, mean, std):
        y = _stem_conv_norm_fwd(x, weight, mean, std)
        ctx.save_for_backward(x, weight)
        ctx.norm = (mean, std)
        ctx.params_const = _wino_frozen > 0
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        mean, std = ctx.norm
        lib = N.lib()
        g = _c(g)
        B, Cin, H, W = x.shape
        g_x = g_w = None
        if ctx.needs_input_grad[0]:
            g_x = torch.empty_like(x)
            nb = 4 * (g.numel() + g_x.numel())
            w_s = _stem_w_over_std(weight, std)
            N.check(_timed("stem_conv_bwd", lambda: lib.dmh_conv7x7s2_bwd_data(N.ptr(g), N.ptr(w_s), B, 64, Cin, H, W,
                                                                              N.ptr(g_x), N.stream()), nb, 2 * 147 * g.numel()))
        if ctx.needs_input_grad[1] and not ctx.params_const:
            g_w = _stem_wrw(x, g, weight, mean, std)
            if g_w is None:
                xn = (x - mean) / std
                g_w = torch.ops.aten.convolution_backward(g, xn, weight, None, [2, 2], [3, 3], [1, 1], False, [0, 0], 1,
                                                          [False, True, False])[1]
        return g_x, g_w, None, None


def stem_conv_norm(x, weight, mean=0.45, std=0.225):
    """conv1((x - mean) / std) for the encoder's first layer -- MD2/networks/resnet_encoder.py:89-90 with torchvision's
    ResNet.conv1 (3 -> 64 channels, 7x7, stride 2, padding 3, no bias) -- as ONE launch of the K14 MFMA kernel: the
    normalisation is applied while the input tile is staged, so neither the normalised image nor a layout transpose
    ever exists in memory."""
    _need_cuda(x)
    if tuple(weight.shape) != (64, 3, 7, 7) or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 2 or x.shape[3] % 2:
        raise RuntimeError("stem_conv_norm: x must be [B,3,H,W] with even H, W and weight [64,3,7,7]")
    return _StemConvNorm.apply(_c(x), weight, float(mean), float(std))




def _down_image(w3, wd):
    """The filter pair of K15 as an image of the kernels' LDS layout (csrc/down_conv.hip, "round 5"): [rows / 32][inner / 8][2560]
    floats from w3 [rows, inner, 3, 3] and wd [rows, inner(, 1, 1)] or None.  Once per weight tensor inside frozen_weights()."""
    lib = N.lib()
    rows, inner = w3.shape[0], w3.shape[1]

    def make():
        img = torch.empty(lib.dmh_down_conv_image_size(rows, inner), device=w3.device, dtype=torch.float32)
        N.check(lib.dmh_down_conv_weight_image(N.ptr(w3), N.ptr(wd), rows, inner, N.ptr(img), N.stream()))
        # the entry keeps its source tensors: a caller may hand in a temporary (a contiguous copy of a channels_last parameter),
        # and a freed temporary's address could come to name another layer's data with the same version inside one scope
        return img, w3, wd
    return frozen_memo(("down_img", w3.data_ptr(), w3._version, None if wd is None else (wd.data_ptr(), wd._version)), make)[0]


def _k15_fwd(lib, x, w3, wd, shift3, shiftd, relu3, B, Cin, Cout, H, W, y3, yd, stream):
    """dmh_down_conv_fwd_act, in its image form (16-byte loaders; bit-identical) where the rows are whole 16-byte words."""
    if W % 4 == 0 and Cout % 32 == 0:
        return lib.dmh_down_conv_fwd_img(N.ptr(x), N.ptr(_down_image(w3, wd)), int(wd is not None), N.ptr(shift3), N.ptr(shiftd),
                                         int(relu3), B, Cin, Cout, H, W, N.ptr(y3), N.ptr(yd), stream)
    return lib.dmh_down_conv_fwd_act(N.ptr(x), N.ptr(w3), N.ptr(wd), N.ptr(shift3), N.ptr(shiftd), int(relu3), B, Cin, Cout, H, W,
                                     N.ptr(y3), N.ptr(yd), stream)


def _k15_bwd(lib, g3, gd, w3t, wdt, g_add, B, Cin, Cout, H, W, g_x, stream):
    """dmh_down_conv_bwd_data_acc (filters transposed: w3t [Cin, Cout, 3, 3], wdt [Cin, Cout]), image form where W % 8 == 0."""
    if W % 8 == 0 and Cin % 32 == 0:
        return lib.dmh_down_conv_bwd_data_img(N.ptr(g3), N.ptr(gd), N.ptr(_down_image(w3t, wdt)), N.ptr(g_add), B, Cin, Cout, H, W,
                                              N.ptr(g_x), stream)
    return lib.dmh_down_conv_bwd_data_acc(N.ptr(g3), N.ptr(gd), N.ptr(w3t), N.ptr(wdt), N.ptr(g_add), B, Cin, Cout, H, W, N.ptr(g_x),
                                          stream)


class _DownConvs(torch.autograd.Function):
    """K15: conv3x3 stride 2 and the 1x1 stride-2 shortcut convolution of a down-sampling BasicBlock, one launch; backward:
    both input gradients in one launch (no separate accumulation pass), both weight gradients in one K20 launch (train pass
    only; ATen for input widths that are not multiples of 8)."""

    @staticmethod
    def forward(ctx, x, w3, wd):
        lib = N.lib()
        B, Cin, H, W = x.shape
        Cout = w3.shape[0]
        y3 = torch.empty((B, Cout, H // 2, W // 2), device=x.device, dtype=torch.float32)
        yd = torch.empty_like(y3)
        nb = 4 * (x.numel() + 2 * y3.numel() + w3.numel() + wd.numel())
        N.check(_timed("down_conv_fwd", lambda: _k15_fwd(lib, x, _c(w3.detach()), _c(wd.detach()), None, None, 0, B, Cin, Cout, H, W,
                                                         y3, yd, N.stream()), nb, 20 * Cin * y3.numel()))
        ctx.save_for_backward(x, w3, wd)
        ctx.params_const = _wino_frozen > 0
        return y3, yd

    @staticmethod
    def backward(ctx, g3, gd):
        x, w3, wd = ctx.saved_tensors
        lib = N.lib()
        B, Cin, H, W = x.shape
        Cout = w3.shape[0]
        g3, gd = _c(g3), _c(gd)
        g_x = g_w3 = g_wd = None
        if ctx.needs_input_grad[0]:
            # the kernel takes the filters transposed ([C_in][C_out][...]): once per attack inside frozen_weights()
            w3t = frozen_memo(("down_w3t", w3.data_ptr(), w3._version), lambda: _c(w3.detach().transpose(0, 1)))
            wdt = frozen_memo(("down_wdt", wd.data_ptr(), wd._version), lambda: _c(wd.detach().reshape(Cout, Cin).t()))
            g_x = torch.empty_like(x)
            nb = 4 * (g_x.numel() + 2 * g3.numel() + w3.numel() + wd.numel())
            N.check(_timed("down_conv_bwd", lambda: _k15_bwd(lib, g3, gd, w3t, wdt, None, B, Cin, Cout, H, W, g_x, N.stream()),
                           nb, 20 * Cin * g3.numel()))
        if not ctx.params_const and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            n = lib.dmh_down_wrw_workspace_size(B, Cin, Cout, H, W) if x.numel() * 4 <= 0xFFFFFF00 else -1
            if n >= 0 and ctx.needs_input_grad[1]:
                ws = torch.empty(n, device=x.device, dtype=torch.float32)
                g_w3 = torch.empty_like(w3, memory_format=torch.contiguous_format)
                with_d = bool(ctx.needs_input_grad[2])
                g_wd = torch.empty_like(wd, memory_format=torch.contiguous_format) if with_d else None
                N.check(_timed("down_wrw", lambda: lib.dmh_down_wrw(
                    N.ptr(x), N.ptr(g3), N.ptr(gd) if with_d else None, B, Cin, Cout, H, W, N.ptr(ws), N.ptr(g_w3),
                    N.ptr(g_wd) if with_d else None, N.stream()), 4 * (x.numel() + 2 * g3.numel()), 20 * Cin * g3.numel()))
                return g_x, g_w3, g_wd
            if ctx.needs_input_grad[1]:
                g_w3 = torch.ops.aten.convolution_backward(g3, x, w3, None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1,
                                                           [False, True, False])[1]
            if ctx.needs_input_grad[2]:
                g_wd = torch.ops.aten.convolution_backward(gd, x, wd, None, [2, 2], [0, 0], [1, 1], False, [0, 0], 1,
                                                           [False, True, False])[1]
        return g_x, g_w3, g_wd


def down_convs_ok(x, w3, wd):
    """Shapes K15 takes: fp32 CUDA, [C_out, C_in, 3, 3] + [C_out, C_in, 1, 1] with both channel counts multiples of 64,
    even input size."""
    return (WINO_ENABLED and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and w3.dim() == 4 and wd.dim() == 4
            and tuple(w3.shape[2:]) == (3, 3) and tuple(wd.shape[2:]) == (1, 1) and w3.shape[:2] == wd.shape[:2]
            and w3.shape[1] == x.shape[1] and x.shape[1] % 64 == 0 and w3.shape[0] % 64 == 0
            and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and x.shape[2] >= 2 and x.shape[3] >= 2
            # the kernel's own 32-bit index limits (DMH_REQUIRE in csrc/down_conv.hip): beyond them the caller falls back
            and x.shape[0] * max(x.shape[1], w3.shape[0]) * x.shape[2] * x.shape[3] < (1 << 29)
            and x.shape[1] * w3.shape[0] < (1 << 24))


def down_convs(x, w3, wd):
    """(conv2d(x, w3, stride=2, padding=1), conv2d(x, wd, stride=2)): the first 3x3 convolution and the 1x1 shortcut of a
    down-sampling torchvision BasicBlock (layer2.0 / layer3.0 / layer4.0 under MD2/networks/resnet_encoder.py:94-98), which
    read the same input -- one K15 MFMA launch forward, one for the summed input gradient."""
    _need_cuda(x)
    if not down_convs_ok(x, w3, wd):
        raise RuntimeError("down_convs: x [B,C,H,W] (C %% 64 == 0, even H, W), w3 [K,C,3,3], wd [K,C,1,1] (K %% 64 == 0) expected")
    return _DownConvs.apply(_c(x), w3, wd)


def _block_fwd(x, w1, s1, b1, w2, s2, b2, workspace):
    """A stride-1 BasicBlock in eval() as two K10 launches: (out1, y) = (relu(bn1(conv1(x))), relu(bn2(conv2(out1)) + x))."""
    out1 = _k10(x, w1, s1, backward=False, bias=b1, flag=1, workspace=workspace)
    return out1, _k10(out1, w2, s2, backward=False, bias=b2, res=x, flag=1, workspace=workspace)


def _block_bwd(g2, out1, w1, s1, w2, s2, workspace):
    """The block's input gradient from ``g2`` = g * [y > 0] (the caller's masking pass), as two K10 launches."""
    g1 = _k10(g2, w2, s2, backward=True, res=out1, flag=2, workspace=workspace)        # conv2's backward-data * [out1 > 0]
    return _k10(g1, w1, s1, backward=True, res=g2, flag=0, workspace=workspace)        # conv1's + the identity branch's gradient


class _BasicBlockEval(torch.autograd.Function):
    """A stride-1 torchvision BasicBlock in eval() with constant parameters (inside an attack), as one autograd node:
        out1 = relu(bn1(conv1(x)));   y = relu(bn2(conv2(out1)) + x)          MD2/networks/resnet_encoder.py:85-98
    forward = the two K10 launches of conv3x3_bn_act; backward = one K9 pass (mask by y) + two K10 launches whose
    epilogues apply the ReLU mask of out1 and add the identity branch's gradient -- instead of two K9 passes, two K10
    launches and autograd's accumulation add."""

    @staticmethod
    def forward(ctx, x, w1, s1, b1, w2, s2, b2):
        out1, y = _block_fwd(x, w1, s1, b1, w2, s2, b2, True)
        ctx.save_for_backward(out1, y, w1, s1, w2, s2)
        return y

    @staticmethod
    def backward(ctx, g):
        out1, y, w1, s1, w2, s2 = ctx.saved_tensors
        g2 = _relu_mask_bwd(y, _c(g))       # gradient of conv2's BatchNorm output and of the identity branch
        return _block_bwd(g2, out1, w1, s1, w2, s2, True), None, None, None, None, None, None


def basic_block_eval_ok(x, w1, w2):
    """Shapes and state the one-node BasicBlock takes: inside frozen_weights() (no parameter gradients exist there), fp32
    CUDA, equal channel counts, both convolutions on the K10 epilogue kernel (no channel split)."""
    if not (_wino_frozen > 0 and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    B, Cc, H, W = x.shape
    return (tuple(w1.shape) == (Cc, Cc, 3, 3) and tuple(w2.shape) == (Cc, Cc, 3, 3)
            and _wino_ok(B, Cc, Cc, H, W, allow_split=False, allow_sk=True))


def basic_block_eval(x, w1, scale1, shift1, w2, scale2, shift2):
    """relu(bn2(conv2(relu(bn1(conv1(x))))) + x) with the BatchNorms given as (scale, shift): a stride-1 BasicBlock of the
    encoder during an attack (model in eval(), parameters constant), as one autograd node (see _BasicBlockEval)."""
    if not basic_block_eval_ok(x, w1, w2):
        raise RuntimeError("basic_block_eval: needs ops.frozen_weights(), an fp32 CUDA [B,C,H,W] input and [C,C,3,3] filters "
                           "of a shape the Winograd kernel takes (ops.basic_block_eval_ok)")
    _reject_affine_grad("basic_block_eval", scale1, shift1)
    _reject_affine_grad("basic_block_eval", scale2, shift2)
    if not x.requires_grad:         # nothing to differentiate: the two fused launches
        y = conv3x3_bn_act(x, w1, scale1, shift1, None, True, 1)
        return conv3x3_bn_act(y, w2, scale2, shift2, x, True, 1)
    return _BasicBlockEval.apply(_c(x), w1.detach(), _c(scale1.detach()), _c(shift1.detach()), w2.detach(),
                                 _c(scale2.detach()), _c(shift2.detach()))


def _down_block_fwd(x, w3, s1, b1, wd, sd, bd, w2, s2, b2, workspace, count_filters):
    """A down-sampling BasicBlock in eval(): (out1, y) = (relu(bn1(conv1_s2(x))), relu(bn2(conv2(out1)) + bn_d(conv1x1_s2(x)))) as
    ONE K15 launch (both BatchNorm scales folded into the filters, shifts and the ReLU in its epilogue) + one K10 launch.
    ``count_filters``: the profile's byte count of the K15 launch includes the two filters."""
    B, Cin, H, W = x.shape
    Co = w3.shape[0]
    w3s = frozen_memo(("down_w3s", w3.data_ptr(), w3._version, s1.data_ptr()), lambda: _c(w3 * s1.view(-1, 1, 1, 1)))
    wds = frozen_memo(("down_wds", wd.data_ptr(), wd._version, sd.data_ptr()), lambda: _c(wd * sd.view(-1, 1, 1, 1)))
    out1 = torch.empty((B, Co, H // 2, W // 2), device=x.device, dtype=torch.float32)
    idt = torch.empty_like(out1)
    nb = 4 * (x.numel() + 2 * out1.numel() + (w3.numel() + wd.numel() if count_filters else 0))
    N.check(_timed("down_conv_fwd", lambda: _k15_fwd(N.lib(), x, w3s, wds, b1, bd, 1, B, Cin, Co, H, W, out1, idt, N.stream()),
                   nb, 20 * Cin * out1.numel()))
    return out1, _k10(out1, w2, s2, backward=False, bias=b2, res=idt, flag=1, workspace=workspace)


def _down_block_bwd(g1, g2, g_skip, in_shape, w3, s1, wd, sd):
    """The block's input gradient [``in_shape``] as one K15 launch on the transposed, scaled filters: from ``g1`` (bn1's output:
    conv2's masked backward-data, the caller's K10 launch), ``g2`` = g * [y > 0] (the shortcut's BatchNorm output) and
    ``g_skip`` (optional: the gradient of the input's other consumer, added in the epilogue)."""
    B, Cin, H, W = in_shape
    Co = w3.shape[0]
    w3ts = frozen_memo(("down_w3ts", w3.data_ptr(), w3._version, s1.data_ptr()),
                       lambda: _c((w3 * s1.view(-1, 1, 1, 1)).transpose(0, 1)))
    wdts = frozen_memo(("down_wdts", wd.data_ptr(), wd._version, sd.data_ptr()),
                       lambda: _c((wd * sd.view(-1, 1, 1, 1)).reshape(Co, Cin).t()))
    g_x = torch.empty((B, Cin, H, W), device=g1.device, dtype=torch.float32)
    N.check(_timed("down_conv_bwd", lambda: _k15_bwd(N.lib(), g1, g2, w3ts, wdts, g_skip, B, Cin, Co, H, W, g_x, N.stream()),
                   4 * (g_x.numel() * (1 if g_skip is None else 2) + 2 * g1.numel()), 20 * Cin * g1.numel()))
    return g_x


class _DownBlockEval(torch.autograd.Function):
    """A down-sampling torchvision BasicBlock in eval() with constant parameters (inside an attack), as one autograd node:
        out1 = relu(bn1(conv1_s2(x)));  idt = bn_d(conv1x1_s2(x));  y = relu(bn2(conv2(out1)) + idt)
    forward = ONE K15 launch + one K10 launch (_down_block_fwd); backward = one K9 pass (mask by y), one K10 launch (conv2's
    backward-data masked by [out1 > 0] in the epilogue) and one K15 launch on the transposed, scaled filters -- no separate
    BatchNorm / ReLU passes."""

    @staticmethod
    def forward(ctx, x, w3, s1, b1, wd, sd, bd, w2, s2, b2, want_skip):
        out1, y = _down_block_fwd(x, w3, s1, b1, wd, sd, bd, w2, s2, b2, True, True)
        ctx.save_for_backward(out1, y, w3, s1, wd, sd, w2, s2)
        ctx.in_shape = tuple(x.shape)
        ctx.set_materialize_grads(False)
        # want_skip: x is handed back as a second output (an alias).  A caller that feeds THAT tensor to x's other consumer
        # (the decoder's skip connection) makes its gradient an input of this node's backward, where K15's epilogue adds it:
        # autograd's separate accumulation pass over the feature map disappears.
        return (y, x) if want_skip else (y, None)

    @staticmethod
    def backward(ctx, g, g_skip=None):
        out1, y, w3, s1, wd, sd, w2, s2 = ctx.saved_tensors
        if g is None:           # only the alias was used
            return (g_skip,) + (None,) * 10
        g = _c(g)
        g_skip = None if g_skip is None else _c(g_skip)
        g2 = _relu_mask_bwd(y, g)           # gradient of bn2's output and of the shortcut's BatchNorm output
        g1 = _k10(g2, w2, s2, backward=True, res=out1, flag=2, workspace=True)      # of bn1's output
        return (_down_block_bwd(g1, g2, g_skip, ctx.in_shape, w3, s1, wd, sd),) + (None,) * 10




def down_block_eval_ok(x, w3, wd, w2):
    """Inside frozen_weights(), K15 shapes, and the block's second convolution on the K10 epilogue kernel."""
    if not (_wino_frozen > 0 and down_convs_ok(x, w3, wd)):
        return False
    Co = w3.shape[0]
    return tuple(w2.shape) == (Co, Co, 3, 3) and _wino_ok(x.shape[0], Co, Co, x.shape[2] // 2, x.shape[3] // 2, allow_split=False,
                                                         allow_sk=True)


def down_block_eval(x, w3, scale1, shift1, wd, scale_d, shift_d, w2, scale2, shift2, return_skip=False):
    """relu(bn2(conv2(relu(bn1(conv1_s2(x))))) + bn_d(conv1x1_s2(x))) with the BatchNorms given as (scale, shift): a
    down-sampling BasicBlock of the encoder during an attack, as one autograd node (see _DownBlockEval).
    ``return_skip``: returns (y, x') with x' an alias of x to be used by x's OTHER consumer (the decoder's skip connection,
    MD2/networks/depth_decoder.py:53-57): its gradient then enters this node and is added in K15's epilogue."""
    if not down_block_eval_ok(x, w3, wd, w2):
        raise RuntimeError("down_block_eval: needs ops.frozen_weights() and shapes K15 / K10 take (ops.down_block_eval_ok)")
    for sc, sh in ((scale1, shift1), (scale_d, shift_d), (scale2, shift2)):
        _reject_affine_grad("down_block_eval", sc, sh)
    d = lambda t: _c(t.detach())        # noqa: E731
    x = _c(x)
    args = (x, w3.detach(), d(scale1), d(shift1), wd.detach(), d(scale_d), d(shift_d), w2.detach(), d(scale2), d(shift2))
    if not x.requires_grad:
        with torch.no_grad():
            y, _ = _DownBlockEval.apply(*args, False)
        return (y, x) if return_skip else y
    y, skip = _DownBlockEval.apply(*args, bool(return_skip))
    return (y, skip) if return_skip else y


# ---------------------------------------------------------------------------------------------------------------
# K19: the attack's cost evaluated on one window per scene (roi.py plans the windows, csrc/roi_glue.hip is the pass
# between the convolutions).  The convolution kernels are the ones above, chosen here by what a kernel CAN take: a window
# launch is smaller than the shapes the throughput thresholds of _wino_ok / _wino32_ok were measured on.
# ---------------------------------------------------------------------------------------------------------------
ROI_ENABLED = os.environ.get("DMH_ROI", "1") != "0"      # A/B switch: 0 = the attack runs the whole frame


def _conv_any(x, weight, bias, pad, backward=False):
    """conv2d(x, weight, padding=pad) -- or, with ``backward``, the same filter's backward-data pass on a gradient x with
    pad' = 2 - pad_forward -- on whichever hand-written kernel takes the channel counts (_conv3x3_route's ``capable_only``);
    ATen otherwise."""
    y = _conv3x3_routed(x, weight, bias, pad, backward, capable_only=True)
    if y is not None:
        return y
    if backward:
        return torch.nn.functional.conv_transpose2d(x, weight, None, 1, 2 - pad)
    return torch.conv2d(x, weight, bias, 1, pad)


def _roi_glue_args(y, y_org, skip, skip_org, dst_org, size, frame, up, elu):
    a = N.RoiGlueArgs()
    a.y, a.skip = N.ptr(y), N.ptr(skip)
    a.y_org, a.skip_org, a.dst_org = N.ptr(y_org), N.ptr(skip_org), N.ptr(dst_org)
    a.B, a.C1, a.C2 = y.shape[0], y.shape[1], (0 if skip is None else skip.shape[1])
    a.sh, a.sw = y.shape[2], y.shape[3]
    a.kh, a.kw = (0, 0) if skip is None else (skip.shape[2], skip.shape[3])
    a.hc, a.wc = size
    a.H, a.W = frame
    a.up, a.elu = int(up), int(elu)
    return a


def _roi_glue_fwd(a, device):
    out = torch.empty((a.B, a.C1 + a.C2, a.hc + 2, a.wc + 2), device=device, dtype=torch.float32)
    N.check(_timed("roi_glue_fwd", lambda: N.lib().dmh_roi_glue_fwd(C.byref(a), N.ptr(out), N.stream()), 8 * out.numel()))
    return out


def _roi_glue_bwd(a, g_out, device, want_skip, y_region=None, skip_region=None, skip_prezero=True):
    """``y_region`` / ``skip_region`` = (org table [B,2], (rows, cols)): for a whole-frame source only that rectangle is
    computed; the rest of g_y is zero-filled, and so is the rest of g_skip unless ``skip_prezero`` is False (its consumer
    reads inside the rectangle only)."""
    # A rectangle needs the rest of its plane zero-filled first (one more launch, and every byte of the plane written once more):
    # where the plane is less than three times the rectangle the kernel takes the WHOLE plane instead and writes the zeros of
    # the elements no window entry reads itself (round 6: upconv(depth,0)'s output and encoder feature 3 at the attack's sizes)
    if y_region is not None and a.sh * a.sw < 3 * y_region[1][0] * y_region[1][1]:
        y_region = None
    if skip_region is not None and skip_prezero and a.kh * a.kw < 3 * skip_region[1][0] * skip_region[1][1]:
        skip_region = None
    new = torch.zeros if y_region is not None else torch.empty
    g_y = new((a.B, a.C1, a.sh, a.sw), device=device, dtype=torch.float32)
    g_skip = None
    if want_skip:
        new = torch.zeros if (skip_region is not None and skip_prezero) else torch.empty
        g_skip = new((a.B, a.C2, a.kh, a.kw), device=device, dtype=torch.float32)
    yo, (yh, yw) = y_region if y_region is not None else (None, (0, 0))
    ko, (kh, kw) = skip_region if (skip_region is not None and want_skip) else (None, (0, 0))
    nb = 4 * (g_out.numel() + 2 * a.B * a.C1 * (yh * yw if yo is not None else a.sh * a.sw) +
              (0 if g_skip is None else a.B * a.C2 * (kh * kw if ko is not None else a.kh * a.kw)))
    N.check(_timed("roi_glue_bwd", lambda: N.lib().dmh_roi_glue_bwd(C.byref(a), N.ptr(g_out), N.ptr(g_y), N.ptr(g_skip),
                                                                   N.ptr(yo), yh, yw, N.ptr(ko), kh, kw, N.stream()), nb))
    return g_y, g_skip


from .roi import STAGES as _ROI_STAGES, TABLE as _ROI_NAMES     # noqa: E402  (row order of the device table of origins)

ROI_DEPTH = 4       # level of the deepest windowed decoder stage (2, 3 or 4)
# channel plan of the reference decoder's stages (MD2/networks/depth_decoder.py:22-37), by window name: (out, in)
_ROI_CHANNELS = {"d": (1, 16), "z01": (16, 16), "y00": (16, 32), "z11": (32, 96), "y10": (32, 64), "z21": (64, 128),
                 "y20": (64, 128), "z31": (128, 256), "y30": (128, 256), "z41": (256, 512)}


def _roi_chain(depth):
    """The windowed stages from z{depth}1 down to the disparity head, in execution order: (name, level, up, skip index)."""
    names = [st[0] for st in _ROI_STAGES]
    return list(reversed(_ROI_STAGES[:names.index("z%d1" % depth) + 1]))


class _RoiTail(torch.autograd.Function):
    """mean((disp0 * mask)^2) from upconv(depth,0)'s whole-frame output and the encoder features below it, through
    upconv(depth,1) ... dispconv(0) (MD2/networks/depth_decoder.py:51-63) evaluated on one window per scene.  Hand-written
    backward (parameters are constants: inside ops.frozen_weights() only): gradients w.r.t. that output and the features,
    zero outside the rectangles the windows reach.  Tensor arguments: x_top, feat_0 .. feat_{depth-1}, mask, tab, then
    (weight, bias) per stage in execution order."""

    @staticmethod
    def _glue(chain, k, src, feats, org, sz, H0, W0, f0_compact):
        name, lvl, up, skip = chain[k]
        src_org = None if k == 0 else org[chain[k - 1][0]]
        skip_org = org["hz"] if (skip == 0 and f0_compact) else None      # feature 0 handed on as its "hz" window only
        return _roi_glue_args(src, src_org, None if skip is None else feats[skip], skip_org, org[name], sz[name],
                              (H0 >> lvl, W0 >> lvl), up, 1)

    @staticmethod
    def forward(ctx, plan, depth, x_top, *rest):
        lib = N.lib()
        dev = x_top.device
        depth, sign = (depth if isinstance(depth, tuple) else (depth, 1.0))       # (depth, -1.0): the negated cost
        feats, mask, tab = rest[:depth], rest[depth], rest[depth + 1]
        wb = rest[depth + 2:]
        chain = _roi_chain(depth)
        B = x_top.shape[0]
        H0, W0 = x_top.shape[2] << (depth + 1), x_top.shape[3] << (depth + 1)
        f0c = bool(plan.f0_compact)
        if (any(tuple(f.shape[2:]) != ((H0 >> (k + 1), W0 >> (k + 1)) if (k or not f0c) else plan.size["hz"])
                for k, f in enumerate(feats))
                or tuple(mask.shape) != (B, 1, H0, W0) or plan.B != B or (plan.H, plan.W) != (H0, W0)):
            raise RuntimeError("roi tail: feature / mask / plan shapes do not match")
        org = {n: tab[k] for k, n in enumerate(_ROI_NAMES)}
        sz = plan.size
        outs, src = [], x_top
        for k in range(len(chain)):
            a = _RoiTail._glue(chain, k, src, feats, org, sz, H0, W0, f0c)
            src = _conv_any(_roi_glue_fwd(a, dev), wb[2 * k], wb[2 * k + 1], 0)
            outs.append(src)
        d_pre = outs.pop()
        hd, wd_ = sz["d"]
        sig = torch.empty_like(d_pre)
        part = torch.empty(lib.dmh_roi_cost_partials_size(B, hd, wd_), device=dev, dtype=torch.float32)
        cost = torch.empty((), device=dev, dtype=torch.float32)
        N.check(lib.dmh_roi_cost_fwd_scaled(N.ptr(d_pre), N.ptr(mask), N.ptr(org["d"]), B, hd, wd_, H0, W0, sign, N.ptr(sig),
                                            N.ptr(part), N.ptr(cost), N.stream()))
        ctx.save_for_backward(x_top, mask, tab, sig, *feats, *outs, *wb[0::2])
        ctx.plan, ctx.depth, ctx.f0c, ctx.sign = plan, depth, f0c, sign
        return cost

    @staticmethod
    def backward(ctx, g):
        plan, depth = ctx.plan, ctx.depth
        sv = ctx.saved_tensors
        x_top, mask, tab, sig = sv[:4]
        chain = _roi_chain(depth)
        n = len(chain)
        feats, outs, ws = sv[4:4 + depth], sv[4 + depth:4 + depth + n - 1], sv[4 + depth + n - 1:]
        lib = N.lib()
        dev = x_top.device
        B = x_top.shape[0]
        H0, W0 = plan.H, plan.W
        org = {nm: tab[k] for k, nm in enumerate(_ROI_NAMES)}
        sz = plan.size
        hd, wd_ = sz["d"]
        g_cur = torch.empty_like(sig)
        N.check(lib.dmh_roi_cost_bwd_scaled(N.ptr(sig), N.ptr(mask), N.ptr(org["d"]), B, hd, wd_, H0, W0, ctx.sign,
                                            N.ptr(_c(g.to(torch.float32))), N.ptr(g_cur), N.stream()))
        g_feats = [None] * depth
        for k in range(n - 1, -1, -1):
            name, lvl, up, skip = chain[k]
            src = x_top if k == 0 else outs[k - 1]
            a = _RoiTail._glue(chain, k, src, feats, org, sz, H0, W0, ctx.f0c)
            want_skip = skip is not None and ctx.needs_input_grad[3 + skip]
            y_reg = ("r_y%d0" % lvl) if k == 0 else None
            s_reg = None if (skip is None or (skip == 0 and ctx.f0c)) else "r_f%d" % skip      # a compact feature: all of it
            # feature 0's gradient is zero outside "r_f0"; an encoder head that runs its backward on the plan's windows reads
            # it inside that rectangle only, so the rest of the 252 MB tensor is not even zero-filled then
            g_cur, g_skip = _roi_glue_bwd(a, _conv_any(g_cur, ws[k], None, 2, True), dev, want_skip,
                                          y_region=None if y_reg is None else (org[y_reg], sz[y_reg]),
                                          skip_region=None if s_reg is None else (org[s_reg], sz[s_reg]),
                                          skip_prezero=not (skip == 0 and plan.head_windowed))
            if skip is not None:
                g_feats[skip] = g_skip
        return (None, None, g_cur) + tuple(g_feats) + (None,) * (2 + 2 * n)


def roi_tail_ok(x_top, feats, convs, depth):
    """The cropped tail applies: inside frozen_weights() (its backward has no parameter gradients), fp32 CUDA tensors, the
    reference decoder's channel plan for the stages upconv(depth,1) ... dispconv(0)."""
    if depth not in (2, 3, 4) or len(feats) != depth:
        return False
    chain = _roi_chain(depth)
    shapes = [tuple(c.weight.shape) for c in convs]
    return (ROI_ENABLED and _wino_frozen > 0 and x_top.is_cuda and all(t.dtype == torch.float32 for t in (x_top,) + tuple(feats))
            and shapes == [_ROI_CHANNELS[st[0]] + (3, 3) for st in chain]
            and x_top.shape[1] == _ROI_CHANNELS["z%d1" % depth][0]
            and all(f.shape[1] == _ROI_CHANNELS["z%d1" % (k + 1)][1] - _ROI_CHANNELS["z%d1" % (k + 1)][0] for k, f in enumerate(feats))
            and x_top.shape[2] >= 2 and x_top.shape[3] >= 2)


def roi_tail_cost(x_top, feats, mask, plan, tab, convs, negate=False):
    """mean((sigmoid(dispconv0(...)) * mask)^2) of the decoder tail on the windows of ``plan`` (roi.RoiPlan; ``tab`` is
    its origin table on the device, int32 [len(roi.TABLE), B, 2]).  ``x_top``: upconv(depth,0)'s whole-frame output (before
    its ELU), depth = plan.depth; ``feats``: encoder features 0 .. depth-1; ``convs``: the nn.Conv2d modules of upconv(depth,1)
    ... upconv(0,1), dispconv(0) in execution order.  Equals ops.masked_sq_mean(decoder(...)[("disp", 0)], mask) when the
    mask is zero outside the plan's boxes; ``negate``: minus that (what an attack hands to autograd), the sign applied inside
    the cost kernels."""
    depth = plan.depth
    feats = tuple(feats)
    if not roi_tail_ok(x_top, feats, convs, depth):
        raise RuntimeError("roi_tail_cost: needs ops.frozen_weights(), fp32 CUDA tensors and the Monodepth2 decoder tail")
    if tab.dtype != torch.int32 or tuple(tab.shape) != (len(_ROI_NAMES), x_top.shape[0], 2):
        raise RuntimeError("roi_tail_cost: origin table must be int32 [%d, B, 2] (roi.TABLE)" % len(_ROI_NAMES))
    wb = []
    for c in convs:
        wb += [c.weight.detach(), None if c.bias is None else _c(c.bias.detach())]
    return _RoiTail.apply(plan, (depth, -1.0) if negate else depth, _c(x_top), *[_c(f) for f in feats], _c(mask), _c(tab), *wb)


def _roi_crop(src, gate, g, org, size, frame=None, gate_compact=False):
    """Compact [B, C, h, w] window (origins ``org``, ``size``) of ``src``, a tensor on a frame of ``frame`` = (H, W) (default: its
    own size), times [gate > 0] where a gate is given (whole-frame, or ``gate_compact``: itself that window); or, with ``g``
    (compact) instead of src, g * [gate window > 0]  (roi_crop / roi_mask of csrc/roi_encoder.hip)."""
    ref = src if src is not None else gate
    B, Cc = ref.shape[:2]
    H, W = frame if frame is not None else ref.shape[2:]
    out = torch.empty((B, Cc) + tuple(size), device=ref.device, dtype=torch.float32)
    N.check(_timed("roi_crop", lambda: N.lib().dmh_roi_crop(N.ptr(src), N.ptr(gate), N.ptr(g), N.ptr(org), B, Cc, H, W, size[0],
                                                           size[1], int(gate_compact), N.ptr(out), N.stream()),
                   4 * out.numel() * (2 + (gate is not None))))
    return out


class _EncHeadEval(torch.autograd.Function):
    """conv1((x - 0.45) / 0.225) -> bn1 -> relu -> maxpool -> layer1 (two stride-1 BasicBlocks) of the ResNet encoder in
    eval() with constant parameters (MD2/networks/resnet_encoder.py:85-98), as ONE autograd node whose backward runs on the
    windows of a roi.RoiPlan: the attack reads d cost / d image under the pasted object only.  Forward = the same launches as
    the separate nodes (K14, K9 stem, four K10 launches).  Backward: layer1 on the "l1" window of the 1/4 map (four K10
    launches on compact tensors; each spoils one ring of the window, which is four rings larger than what is read of it),
    the stem's max-pool / ReLU / BatchNorm adjoint on the "gz" window of the 1/2 map, K12 on the image window "d"."""

    @staticmethod
    def forward(ctx, x, plan, tab, w_stem, s0, b0, w1a, s1a, b1a, w2a, s2a, b2a, w1b, s1b, b1b, w2b, s2b, b2b):
        f0, pooled, arg = _stem_pool_fwd(_stem_conv_norm_fwd(x, w_stem, 0.45, 0.225), s0, b0)
        o1a, ya = _block_fwd(pooled, w1a, s1a, b1a, w2a, s2a, b2a, False)
        o1b, f1 = _block_fwd(ya, w1b, s1b, b1b, w2b, s2b, b2b, False)
        ctx.save_for_backward(f0, arg, s0, o1a, ya, o1b, f1, tab, w_stem, w1a, s1a, w2a, s2a, w1b, s1b, w2b, s2b)
        ctx.plan, ctx.img = plan, tuple(x.shape[2:])
        ctx.set_materialize_grads(False)
        return f0, f1

    @staticmethod
    def backward(ctx, g_f0, g_f1):
        f0, arg, s0, o1a, ya, o1b, f1, tab, w_stem, w1a, s1a, w2a, s2a, w1b, s1b, w2b, s2b = ctx.saved_tensors
        plan, (H, W) = ctx.plan, ctx.img
        B = f0.shape[0]
        org = {n: tab[k] for k, n in enumerate(_ROI_NAMES)}
        sz = plan.size
        hq, wq = sz["l1"]
        if g_f1 is None:
            g_pool = torch.zeros((B, 64, hq, wq), device=f0.device, dtype=torch.float32)
        else:
            g2b = _roi_crop(_c(g_f1), f1, None, org["l1"], (hq, wq))                    # g * [y_b > 0] on the window
            g_ya = _block_bwd(g2b, _roi_crop(o1b, None, None, org["l1"], (hq, wq)), w1b, s1b, w2b, s2b, False)
            g2a = _roi_crop(None, ya, g_ya, org["l1"], (hq, wq))                        # * [y_a > 0]
            g_pool = _block_bwd(g2a, _roi_crop(o1a, None, None, org["l1"], (hq, wq)), w1a, s1a, w2a, s2a, False)
        hs, ws = sz["gz"]
        g_z = torch.empty((B, 64, hs, ws), device=f0.device, dtype=torch.float32)
        N.check(_timed("stem_bwd_win", lambda: N.lib().dmh_stem_bn_relu_pool_bwd_win(
            N.ptr(f0), N.ptr(arg), N.ptr(None if g_f0 is None else _c(g_f0)), N.ptr(g_pool), N.ptr(s0), N.ptr(org["gz"]),
            N.ptr(org["l1"]), B, 64, H // 2, W // 2, hs, ws, hq, wq, N.ptr(g_z), N.stream()), 4 * 4 * g_z.numel()))
        return (_stem_window_bwd(g_z, w_stem, org["gz"], org["d"], sz["d"], H, W),) + (None,) * 17


def encoder_head_ok(x, conv1_weight, blocks):
    """The windowed encoder head applies: inside frozen_weights(), an fp32 CUDA image [B,3,H,W] with H, W multiples of 8, the
    standard 3 -> 64 7x7 first layer and a layer1 of two stride-1 64-channel BasicBlocks whose convolutions K10 takes."""
    if not (ROI_ENABLED and _wino_frozen > 0 and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3
            and x.shape[2] % 8 == 0 and x.shape[3] % 8 == 0 and x.requires_grad and tuple(conv1_weight.shape) == (64, 3, 7, 7)):
        return False
    B, _, H, W = x.shape
    return (len(blocks) == 2 and all(tuple(w.shape) == (64, 64, 3, 3) for blk in blocks for w in blk)
            and _wino_ok(B, 64, 64, H // 4, W // 4, allow_split=False) and B * 64 * (H // 4) * (W // 4) < (1 << 30))


def _head_plan_ok(x, plan, tab):
    """The plan and its device table of origins (int32 [len(roi.TABLE), B, 2]) belong to the image batch x."""
    return (tab.dtype == torch.int32 and tuple(tab.shape) == (len(_ROI_NAMES), x.shape[0], 2) and plan.B == x.shape[0]
            and (plan.H, plan.W) == tuple(x.shape[2:]))


def _head_args(conv1_weight, aff0, *blocks):
    """The tensor arguments of the head nodes: the stem's (weight, scale, shift), then (weight, scale, shift) per convolution of
    the blocks, each given as (w, (scale, shift), w, (scale, shift), ...)."""
    d = lambda t: _c(t.detach())        # noqa: E731
    args = [d(conv1_weight), d(aff0[0]), d(aff0[1])]
    for blk in blocks:
        for w, aff in zip(blk[0::2], blk[1::2]):
            args += [w.detach(), d(aff[0]), d(aff[1])]
    return args


def encoder_head_eval(x, plan, tab, conv1_weight, aff0, blocks):
    """(feature 0, feature 1) of the ResNet-18 encoder in eval() -- MD2/networks/resnet_encoder.py:88-95: relu(bn1(conv1((x -
    0.45) / 0.225))) and layer1(maxpool(.)) -- as one node whose backward runs on the windows of ``plan`` (see _EncHeadEval):
    d / d x is exact inside the plan's image window "d" and ZERO outside it, which is all an object attack reads
    (physicalTrans.py:156-165).  ``blocks``: per BasicBlock (w1, (scale1, shift1), w2, (scale2, shift2)); ``aff0``: bn1's
    (scale, shift).  Marks the plan as head_windowed (the decoder tail then writes feature 0's gradient inside "r_f0" only)."""
    ws = [(b[0], b[2]) for b in blocks]
    if not encoder_head_ok(x, conv1_weight, ws):
        raise RuntimeError("encoder_head_eval: needs ops.frozen_weights() and the ResNet-18 head (ops.encoder_head_ok)")
    if not _head_plan_ok(x, plan, tab):
        raise RuntimeError("encoder_head_eval: plan / origin table do not match the image batch")
    plan.head_windowed = True
    return _EncHeadEval.apply(_c(x), plan, _c(tab), *_head_args(conv1_weight, aff0, *blocks))


class CleanHead(object):
    """What the incremental encoder head keeps of the CLEAN scenes for the length of one attack: encoder feature 1 (layer1's
    output) of the un-pasted frames, twice -- ``pristine`` is never written; ``work`` is the tensor handed to the rest of the
    network, into which each attack step writes the cells the pasted object changes ("f1s") and puts the clean values back
    before the next step."""

    def __init__(self, f1, f2=None, frames=None):
        self.frames = frames        # the clean frames themselves: kept alive, so that their address cannot name other data
        self.generation = 0         # bumped by every step that writes into `work`: a backward of an older step must not run
        self.pristine, self.work = f1, f1.clone()
        self.dirty = None           # (origin table [B,2], (rows, cols)) of the window written by the last step
        self.pristine2, self.work2 = f2, (None if f2 is None else f2.clone())     # the same for feature 2 (layer2's output)
        self.dirty2 = None
        self._own = {}              # private copies of the origins of `dirty` / `dirty2` (mark(..., keep=True))

    def mark(self, which, org, size, keep):
        """Record the window step ``which`` (1: feature 1, 2: feature 2) has just written.  ``keep``: the origin table will be
        OVERWRITTEN before restore() reads it (an attack replayed from a HIP graph keeps one table buffer and copies every
        step's origins into it: torchattacks/attacks/phy_obj_atk.py, _graph_steps) -- the origins are then copied into a
        buffer of this object, by a device copy that is part of the step."""
        if keep:
            own = self._own.get(which)
            if own is None or own.shape != org.shape:
                own = self._own[which] = torch.empty_like(org)
            own.copy_(org)
            org = own
        if which == 1:
            self.dirty = (org, size)
        else:
            self.dirty2 = (org, size)

    @staticmethod
    def _put_back(pristine, work, dirty):
        org, (h, w) = dirty
        B, Cc, H, W = work.shape
        N.check(N.lib().dmh_roi_paste(N.ptr(pristine), None, H, W, N.ptr(org), B, Cc, H, W, h, w, N.ptr(work), N.stream()))

    def restore(self):
        if self.dirty is not None:
            self._put_back(self.pristine, self.work, self.dirty)
            self.dirty = None
        if self.dirty2 is not None:
            self._put_back(self.pristine2, self.work2, self.dirty2)
            self.dirty2 = None


def clean_head_snapshot():
    """The Python-side state a traced-but-never-executed attack iteration changes (a HIP-graph capture): the keys of the
    frozen-weights cache and, of every CleanHead in it, the dirty windows, the generation and the private origin copies."""
    heads = [(h, h.dirty, h.dirty2, h.generation, dict(h._own)) for h in _wino_cache.values() if isinstance(h, CleanHead)]
    return set(_wino_cache), heads


def clean_head_restore(snap):
    """Put back what clean_head_snapshot() saw: entries made since are dropped (after a failed capture they point at pool memory
    that no kernel wrote), and every CleanHead names the window the last EXECUTED iteration left dirty."""
    keys, heads = snap
    for k in [k for k in _wino_cache if k not in keys]:
        del _wino_cache[k]
    for h, dirty, dirty2, generation, own in heads:
        h.dirty, h.dirty2, h.generation, h._own = dirty, dirty2, generation, own


class _EncHeadInc(torch.autograd.Function):
    """The encoder head of an attack step, incrementally: the pasted scene differs from the clean scene inside the object's
    box only (physicalTrans.py:156-165), so conv1 -> bn1 -> relu -> maxpool -> layer1 (MD2/networks/resnet_encoder.py:85-98)
    are evaluated on ONE compact window per scene ("hz" on the 1/2 map, "hl" on the 1/4 map: K14's window form, then the
    whole-tensor kernels on the compact tensors; zero padding / pooling padding at the window's edge spoil one ring per stage
    and the plan makes the window that much larger than what is read of it).  Outputs: feature 0 as its "hz" window (its only
    consumers, the decoder tail and this node's backward, read inside it) and feature 1 as the cached clean feature with the
    changed cells ("f1s") written in.  Backward: the same compact tensors through layer1's four backward-data launches, the
    stem's adjoint and K12's window form -- d / d image inside the plan's image window "d", zero elsewhere."""

    @staticmethod
    def forward(ctx, x, plan, tab, clean, w_stem, s0, b0, w1a, s1a, b1a, w2a, s2a, b2a, w1b, s1b, b1b, w2b, s2b, b2b, *l2):
        """``l2`` (optional, 15 tensors): layer2 = a down-sampling block (w3, s1, b1, wd, sd, bd, w2, s2, b2) and a stride-1
        block (w1, s1, b1, w2, s2, b2) -- evaluated on the plan's "h3" window and returned as a third output."""
        lib = N.lib()
        B, _, H, W = x.shape
        st = N.stream()
        org = {n: tab[k] for k, n in enumerate(_ROI_NAMES)}
        hl, wl = plan.size["hl"]
        hz, wz = 2 * hl, 2 * wl
        z = torch.empty((B, 64, hz, wz), device=x.device, dtype=torch.float32)
        N.check(_timed("stem_conv_fwd", lambda: lib.dmh_stem_conv_norm_fwd_win(
            N.ptr(x), N.ptr(_c(w_stem)), N.ptr(org["hz"]), B, H, W, hz, wz, 0.45, 0.225, N.ptr(z), st),
            4 * (z.numel() + 12 * B * hz * wz), 2 * 147 * z.numel()))
        f0, pooled, arg = _stem_pool_fwd(z, s0, b0)
        del z
        o1a, ya = _block_fwd(pooled, w1a, s1a, b1a, w2a, s2a, b2a, False)
        o1b, f1c = _block_fwd(ya, w1b, s1b, b1b, w2b, s2b, b2b, False)
        # feature 1 = the clean scenes' feature with the changed cells written in (the clean values return before the next step)
        clean.restore()
        clean.generation += 1
        ctx.clean, ctx.generation = clean, clean.generation
        hs_, ws_ = plan.size["f1s"]
        N.check(_timed("roi_paste", lambda: lib.dmh_roi_paste(N.ptr(f1c), N.ptr(org["hl"]), hl, wl, N.ptr(org["f1s"]), B, 64,
                                                             H // 4, W // 4, hs_, ws_, N.ptr(clean.work), st),
                       8 * B * 64 * hs_ * ws_))
        clean.mark(1, org["f1s"], (hs_, ws_), getattr(plan, "table_rewritten", False))
        saved = [f0, arg, s0, o1a, ya, o1b, f1c, tab, w_stem, w1a, s1a, w2a, s2a, w1b, s1b, w2b, s2b]
        ctx.plan, ctx.img, ctx.l2 = plan, (H, W), bool(l2)
        ctx.set_materialize_grads(False)
        if not l2:
            ctx.save_for_backward(*saved)
            return f0, clean.work.detach()  # a fresh alias per step: the cached tensor itself never enters an autograd graph
        # ---- layer2 on the "h3" window of the 1/8 map: its input is the "h3in" window of feature 1 as just assembled
        w3, sc1, sh1, wd, scd, shd, w2, sc2, sh2, v1, t1, u1, v2, t2, u2 = l2
        h3, w3_ = plan.size["h3"]
        Co = w3.shape[0]
        x2 = _roi_crop(clean.work, None, None, org["h3in"], (2 * h3, 2 * w3_), frame=(H // 4, W // 4))
        q1, y2a = _down_block_fwd(x2, w3, sc1, sh1, wd, scd, shd, w2, sc2, sh2, False, False)
        q2, f2c = _block_fwd(y2a, v1, t1, u1, v2, t2, u2, False)
        hf, wf = plan.size["f2s"]
        N.check(_timed("roi_paste", lambda: lib.dmh_roi_paste(N.ptr(f2c), N.ptr(org["h3"]), h3, w3_, N.ptr(org["f2s"]), B, Co,
                                                             H // 8, W // 8, hf, wf, N.ptr(clean.work2), st), 8 * B * Co * hf * wf))
        clean.mark(2, org["f2s"], (hf, wf), getattr(plan, "table_rewritten", False))
        ctx.save_for_backward(*saved, q1, y2a, q2, f2c, w3, sc1, wd, scd, w2, sc2, v1, t1, v2, t2)
        return f0, clean.work.detach(), clean.work2.detach()

    @staticmethod
    def backward(ctx, g_f0, g_f1, g_f2=None):
        if ctx.clean.generation != ctx.generation:
            raise RuntimeError("encoder_head_incremental: a later forward has re-written the cached clean features this graph's "
                               "feature 1 / 2 alias; run each step's backward before the next step's forward")
        sv = ctx.saved_tensors
        f0, arg, s0, o1a, ya, o1b, f1c, tab, w_stem, w1a, s1a, w2a, s2a, w1b, s1b, w2b, s2b = sv[:17]
        plan, (H, W) = ctx.plan, ctx.img
        B, _, hz, wz = f0.shape
        org = {n: tab[k] for k, n in enumerate(_ROI_NAMES)}
        hl, wl = plan.size["hl"]
        g_pool = None
        f1_frame, f1_org = (H // 4, W // 4), org["hl"]          # where feature 1's gradient lives: the whole 1/4 map ...
        if ctx.l2 and g_f2 is not None:
            # ---- layer2's backward on "h3": feature 1's gradient comes out as the "h3in" window (which holds "hl")
            q1, y2a, q2, f2c, w3, sc1, wd, scd, w2, sc2, v1, t1, v2, t2 = sv[17:]
            h3, w3_ = plan.size["h3"]
            gb = _roi_crop(_c(g_f2), f2c, None, org["h3"], (h3, w3_), frame=(H // 8, W // 8), gate_compact=True)  # g * [f2 > 0]
            g_y2a = _block_bwd(gb, q2, v1, t1, v2, t2, False)
            # * [y2a > 0]: bn2's output and the shortcut's
            g2 = _roi_crop(None, y2a, g_y2a, org["h3"], (h3, w3_), frame=(H // 8, W // 8), gate_compact=True)
            g1 = _k10(g2, w2, sc2, backward=True, res=q1, flag=2, workspace=False)
            gskip = None
            if g_f1 is not None:            # the decoder's skip gradient, on the same window: added in K15's epilogue
                gskip = _roi_crop(_c(g_f1), None, None, org["h3in"], (2 * h3, 2 * w3_), frame=(H // 4, W // 4))
            g_f1 = _down_block_bwd(g1, g2, gskip, (B, 64, 2 * h3, 2 * w3_), w3, sc1, wd, scd)
            f1_frame, f1_org = (2 * h3, 2 * w3_), org["hl_rel"]             # ... or that window, "hl" at its relative origin
        if g_f1 is not None:
            g2b = _roi_crop(_c(g_f1), f1c, None, f1_org, (hl, wl), frame=f1_frame, gate_compact=True)   # g * [y_b > 0]
            g_ya = _block_bwd(g2b, o1b, w1b, s1b, w2b, s2b, False)
            g2a = _roi_crop(None, ya, g_ya, org["hl"], (hl, wl), frame=(H // 4, W // 4), gate_compact=True)     # * [y_a > 0]
            g_pool = _block_bwd(g2a, o1a, w1a, s1a, w2a, s2a, False)
        n_in = 19 + (15 if ctx.l2 else 0)
        if g_pool is None and g_f0 is None:
            return (None,) * n_in
        g_z = torch.empty_like(f0)
        N.check(_timed("stem_bwd", lambda: N.lib().dmh_stem_bn_relu_pool_bwd(
            N.ptr(f0), N.ptr(arg), N.ptr(None if g_f0 is None else _c(g_f0)), N.ptr(g_pool), N.ptr(s0), B, 64, hz, wz, N.ptr(g_z),
            N.stream()), 4 * 4 * g_z.numel()))
        return (_stem_window_bwd(g_z, w_stem, org["hz"], org["d"], plan.size["d"], H, W),) + (None,) * (n_in - 1)


def clean_head(x_clean, conv1_weight, aff0, blocks, layer2=None):
    """CleanHead of the clean frames ``x_clean`` [B,3,H,W]: feature 1 (and, with ``layer2`` = (down block, block) as in
    encoder_head_incremental, feature 2) through the whole-frame kernels, no gradient."""
    with torch.no_grad():
        z = stem_conv_norm(x_clean, conv1_weight, 0.45, 0.225)
        _, y = stem_bn_relu_pool(z, aff0[0], aff0[1])
        for w1, a1, w2, a2 in blocks:
            o = conv3x3_bn_act(y, w1, a1[0], a1[1], None, True, 1)
            y = conv3x3_bn_act(o, w2, a2[0], a2[1], y, True, 1)
        f2 = None
        if layer2 is not None:
            (w3, a1, wd, ad, w2, a2), (v1, c1, v2, c2) = layer2
            f2 = down_block_eval(y, w3, a1[0], a1[1], wd, ad[0], ad[1], w2, a2[0], a2[1])
            o = conv3x3_bn_act(f2, v1, c1[0], c1[1], None, True, 1)
            f2 = conv3x3_bn_act(o, v2, c2[0], c2[1], f2, True, 1)
    return CleanHead(y, f2, x_clean)


def layer2_incremental_ok(x, layer2):
    """layer2 = a 64 -> 128 down-sampling block + a stride-1 block whose kernels (K15, K10) take the whole-frame shape."""
    if layer2 is None:
        return False
    (w3, _, wd, _, w2, _), (v1, _, v2, _) = layer2
    B, _, H, W = x.shape
    probe = x.new_empty((B, 64, H // 4, W // 4))
    return (tuple(w3.shape) == (128, 64, 3, 3) and tuple(wd.shape) == (128, 64, 1, 1) and down_convs_ok(probe, w3, wd)
            and all(tuple(w.shape) == (128, 128, 3, 3) for w in (w2, v1, v2))
            and _wino_ok(B, 128, 128, H // 8, W // 8, allow_split=False))


def encoder_head_incremental(x, plan, tab, clean, conv1_weight, aff0, blocks, layer2=None):
    """(feature 0 on its "hz" window, feature 1[, feature 2]) of the ResNet-18 encoder for an attack step whose image ``x``
    differs from the clean frames behind ``clean`` (ops.clean_head) inside the plan's boxes only -- see _EncHeadInc.  Marks the
    plan: head_windowed (feature 0's gradient is read inside the window) and f0_compact (feature 0 IS the window).  ``layer2``:
    ((w3, aff1, wd, aff_d, w2, aff2), (w1, aff1, w2, aff2)) -- then layer2 runs on the plan's "h3" window as well."""
    ws = [(b[0], b[2]) for b in blocks]
    if not encoder_head_ok(x, conv1_weight, ws) or not plan.head_incremental_ok:
        raise RuntimeError("encoder_head_incremental: needs ops.frozen_weights(), the ResNet-18 head and a plan whose \"hz\" "
                           "window holds what is read of feature 0")
    if not _head_plan_ok(x, plan, tab) or tuple(clean.work.shape) != (x.shape[0], 64, x.shape[2] // 4, x.shape[3] // 4):
        raise RuntimeError("encoder_head_incremental: plan / origin table / clean feature do not match the image batch")
    if layer2 is not None and not (layer2_incremental_ok(x, layer2) and plan.layer2_incremental_ok and clean.work2 is not None):
        raise RuntimeError("encoder_head_incremental: layer2 given, but its shapes / the plan's \"h3\" window / the clean "
                           "feature 2 do not allow the incremental form")
    plan.head_windowed = plan.f0_compact = True
    return _EncHeadInc.apply(_c(x), plan, _c(tab), clean, *_head_args(conv1_weight, aff0, *blocks, *(layer2 or ())))


def masked_depth_errors(disp_gt, disp_pred, mask=None, min_depth=0.1, max_depth=100.0, scale=5.4, clamp_lo=1e-3,
                        clamp_hi=80.0):
    """The eight attack-evaluation metrics of MD2/evaluate_depth.py:57-99 computed from two disparity maps in one
    pass on the device: returns a tensor [abs_err, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3]."""
    lib = N.lib()
    disp_gt, disp_pred = _c(disp_gt.detach()), _c(disp_pred.detach())
    n = disp_gt.numel()
    if disp_pred.numel() != n or (mask is not None and mask.numel() != n):
        raise RuntimeError("masked_depth_errors: size mismatch")
    part = torch.empty(lib.dmh_depth_errors_partials_size(n), device=disp_gt.device, dtype=torch.float32)
    out = torch.empty(8, device=disp_gt.device, dtype=torch.float32)
    N.check(lib.dmh_masked_depth_errors(N.ptr(disp_gt), N.ptr(disp_pred), N.ptr(None if mask is None else _c(mask)), n,
                                        min_depth, max_depth, scale, clamp_lo, clamp_hi, N.ptr(part), N.ptr(out),
                                        N.stream()))
    return out


# ---------------------------------------------------------------------------------------------------------------- K25
EIGEN_REC, EIGEN_CHUNK, EIGEN_MAX_BATCH = 8, 8192, 64       # DMH_EIGEN_* of include/dmh_hip.h


def eigen_crop(gt_h, gt_w):
    """The Eigen crop (y0, y1, x0, x1) of a gt_h x gt_w map, in double and truncated as MD2/evaluate_depth.py:363-364 does."""
    return np.array([0.40810811 * gt_h, 0.99189189 * gt_h, 0.03594771 * gt_w, 0.96405229 * gt_w]).astype(np.int32)


def _eigen_f32(t, name):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise RuntimeError("libdmh_hip ops compute in fp32; got %s for %s" % (getattr(t, "dtype", type(t)), name))
    return t


def _eigen_i32(t, name):
    if not torch.is_tensor(t) or t.dtype != torch.int32:
        raise RuntimeError("%s must be int32; got %s" % (name, getattr(t, "dtype", type(t))))
    return t


def _eigen_ws(n, device):
    return torch.empty(N.lib().dmh_eigen_select_ws_size(n), device=device, dtype=torch.int32)


def eigen_gt_stats(gt, table, blk_img, first, n, b0, grid, eigen):
    """K25 on the ground truth alone: (medians fp32 [n], valid counts int32 [n]) of the images first .. first + n - 1 of a pack
    (np.median of the valid values; NaN and 0 for a map without a valid pixel).  Three histogram passes, no sort."""
    lib = N.lib()
    _eigen_f32(gt, "gt"), _eigen_i32(table, "table"), _eigen_i32(blk_img, "blk_img")
    if not 0 < n <= EIGEN_MAX_BATCH:
        raise RuntimeError("eigen_gt_stats: 1 .. %d images per call; got %d" % (EIGEN_MAX_BATCH, n))
    med = torch.empty(n, device=gt.device, dtype=torch.float32)
    cnt = torch.empty(n, device=gt.device, dtype=torch.int32)
    ws = _eigen_ws(n, gt.device)
    N.check(lib.dmh_eigen_gt_stats(N.ptr(gt), gt.numel(), N.ptr(table), N.ptr(blk_img), int(table.shape[0]), blk_img.numel(),
                                   int(first), int(n), int(b0), int(grid), int(bool(eigen)), N.ptr(ws), N.ptr(med), N.ptr(cnt),
                                   N.stream()))
    return med, cnt


def eigen_depth_errors_launch(pred_disp, pred_disp_flip, gt, table, blk_img, med_gt, first, b0, grid, px0, npx, eigen,
                              scale_factor=1.0, median_scaling=True):
    """K25's launches for one batch on plain tensors (what ``eigen_depth_errors`` and ``torch.ops.dmh.eigen_depth_errors`` share):
    (errors [n, 8], ratios [n], depth [npx], medians of the valid depths [n]).  ``px0`` / ``npx``: offset and pixel count of the
    batch inside ``gt``; ``b0`` / ``grid``: its work blocks.  Without median scaling the medians are not computed: they and
    ``ratios`` are NaN."""
    lib = N.lib()
    _eigen_f32(pred_disp, "pred_disp"), _eigen_f32(gt, "gt"), _eigen_f32(med_gt, "med_gt")
    _eigen_i32(table, "table"), _eigen_i32(blk_img, "blk_img")
    if pred_disp.dim() != 3:
        raise RuntimeError("eigen_depth_errors: pred_disp must be [n, h, w]")
    n, h, w = [int(v) for v in pred_disp.shape]
    if not 0 < n <= EIGEN_MAX_BATCH:
        raise RuntimeError("eigen_depth_errors: 1 .. %d predictions per call; got %d" % (EIGEN_MAX_BATCH, n))
    if pred_disp_flip is not None and (_eigen_f32(pred_disp_flip, "pred_disp_flip").shape != pred_disp.shape):
        raise RuntimeError("eigen_depth_errors: pred_disp_flip must have pred_disp's shape")
    if med_gt.numel() != table.shape[0] or table.dim() != 2 or table.shape[1] != EIGEN_REC:
        raise RuntimeError("eigen_depth_errors: table must be [N, %d] and med_gt [N]" % EIGEN_REC)
    if px0 < 0 or npx <= 0 or px0 + npx > gt.numel():
        raise RuntimeError("eigen_depth_errors: the batch's pixels must lie in gt")
    dev = pred_disp.device
    pred_disp = _c(pred_disp.detach())
    flip = None if pred_disp_flip is None else _c(pred_disp_flip.detach())
    depth = torch.empty(int(npx), device=dev, dtype=torch.float32)
    errors = torch.empty((n, 8), device=dev, dtype=torch.float32)
    part = torch.empty(lib.dmh_eigen_partials_size(int(grid)), device=dev, dtype=torch.float32)
    ws = _eigen_ws(n, dev) if median_scaling else None
    sizes = (int(table.shape[0]), blk_img.numel(), int(first), n, int(b0), int(grid))
    N.check(lib.dmh_eigen_pred_depth(N.ptr(pred_disp), N.ptr(flip), h, w, N.ptr(gt), gt.numel(), N.ptr(table), N.ptr(blk_img),
                                     *sizes, int(bool(eigen)), float(scale_factor), int(px0), N.ptr(depth), depth.numel(),
                                     N.ptr(ws), N.stream()))
    if median_scaling:
        med = torch.empty(n, device=dev, dtype=torch.float32)
        ratios = torch.empty(n, device=dev, dtype=torch.float32)
        N.check(lib.dmh_eigen_pred_ratio(N.ptr(depth), depth.numel(), int(px0), gt.numel(), N.ptr(table), N.ptr(blk_img), *sizes,
                                         N.ptr(ws), N.ptr(med_gt), N.ptr(med), N.ptr(ratios), N.stream()))
    else:
        ratios = torch.full((n,), float("nan"), device=dev, dtype=torch.float32)
        med = ratios.clone()
    N.check(lib.dmh_eigen_metrics(N.ptr(gt), gt.numel(), N.ptr(depth), depth.numel(), int(px0), N.ptr(table), N.ptr(blk_img),
                                  *sizes, N.ptr(ratios if median_scaling else None), N.ptr(part), N.ptr(errors), N.stream()))
    return errors, ratios, depth, med


class EigenGtPack(object):
    """The ground truth of an evaluation set on the device (``eigen_gt_pack``): ``gt`` the maps one after the other (fp32),
    ``table`` / ``blk_img`` K25's tables, ``counts`` / ``medians`` the valid pixels and np.median of the valid values of every map
    (they depend on the ground truth only: computed once, here).  Host copies: ``shapes``, ``crops`` (y0, y1, x0, x1),
    ``offsets`` [N + 1] and ``blk_first`` [N + 1]."""

    def __init__(self, gt, table, blk_img, shapes, crops, offsets, blk_first, eval_split):
        self.gt, self.table, self.blk_img = gt, table, blk_img
        self.shapes, self.crops, self.offsets, self.blk_first = shapes, crops, offsets, blk_first
        self.eval_split, self.eigen = eval_split, eval_split == "eigen"
        self.counts = self.medians = None

    def __len__(self):
        return len(self.shapes)

    def view(self, flat, first, i):
        """Image ``first + i`` of a batch's flat buffer (``return_pred``) as [gt_h, gt_w]."""
        o = int(self.offsets[first + i] - self.offsets[first])
        gh, gw = self.shapes[first + i]
        return flat[o:o + gh * gw].view(gh, gw)


def eigen_gt_pack(gt_list, eval_split, device):
    """Packs the 2-D ground-truth maps ``gt_list`` (their own, different sizes) for K25: one flat fp32 buffer, the record table
    (crop bounds of MD2/evaluate_depth.py:363-364 for split ``eigen``, the whole map otherwise), and per map the number of valid
    pixels and the median of the valid values."""
    device = torch.device(device)
    _need_cuda(device)
    maps = [np.ascontiguousarray(np.asarray(g), dtype=np.float32) for g in gt_list]
    if not maps or any(m.ndim != 2 or m.size == 0 for m in maps):
        raise RuntimeError("eigen_gt_pack: need at least one ground-truth map, all of them 2-D and not empty")
    shapes = [tuple(int(v) for v in m.shape) for m in maps]
    sizes = np.array([h * w for h, w in shapes], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    blocks = (sizes + EIGEN_CHUNK - 1) // EIGEN_CHUNK
    blk_first = np.concatenate([[0], np.cumsum(blocks)])
    if offsets[-1] >= 2 ** 31:
        raise RuntimeError("eigen_gt_pack: %d pixels; a pack holds fewer than 2^31" % offsets[-1])
    eigen = eval_split == "eigen"
    crops = np.stack([eigen_crop(h, w) if eigen else np.array([0, h, 0, w], dtype=np.int32) for h, w in shapes])
    table = np.zeros((len(maps), EIGEN_REC), dtype=np.int32)
    table[:, 0], table[:, 1], table[:, 2] = offsets[:-1], [s[0] for s in shapes], [s[1] for s in shapes]
    table[:, 3:7], table[:, 7] = crops, blk_first[:-1]
    blk_img = np.repeat(np.arange(len(maps), dtype=np.int32), blocks)
    flat = np.concatenate([m.ravel() for m in maps])
    pack = EigenGtPack(torch.from_numpy(flat).to(device), torch.from_numpy(table).to(device), torch.from_numpy(blk_img).to(device),
                       shapes, crops, offsets, blk_first, eval_split)
    med, cnt = [], []
    for first in range(0, len(maps), EIGEN_MAX_BATCH):
        n = min(EIGEN_MAX_BATCH, len(maps) - first)
        m, c = eigen_gt_stats(pack.gt, pack.table, pack.blk_img, first, n, int(blk_first[first]),
                              int(blk_first[first + n] - blk_first[first]), eigen)
        med.append(m)
        cnt.append(c)
    pack.medians, pack.counts = torch.cat(med), torch.cat(cnt)
    return pack


def eigen_depth_errors(pred_disp, pack, first, *, pred_disp_flip=None, scale_factor=1.0, median_scaling=True, return_pred=False):
    """MD2/evaluate_depth.py:351-384 for the predictions ``pred_disp`` [n, h, w] (disparities at network resolution) of the images
    ``first`` .. ``first + n - 1`` of ``pack``: (errors [n, 8], ratios [n]) on the device, nothing read by the host.
    ``pred_disp_flip``: the predictions of the mirrored frames (not mirrored back): --post_process.  ``scale_factor``:
    --pred_depth_scale_factor.  ``median_scaling`` off: no medians, ``ratios`` is NaN.  ``return_pred``: also the scratch buffer,
    laid out like the batch's ground truth (``pack.view``): the depth before median scaling at the valid pixels, NaN (all bits
    set) at the others; and the medians [n] of its valid values."""
    if not isinstance(pack, EigenGtPack):
        raise RuntimeError("eigen_depth_errors: pack must come from eigen_gt_pack")
    if not torch.is_tensor(pred_disp) or pred_disp.dim() != 3:
        raise RuntimeError("eigen_depth_errors: pred_disp must be [n, h, w]")
    n, first = int(pred_disp.shape[0]), int(first)
    if first < 0 or n == 0 or first + n > len(pack):
        raise RuntimeError("eigen_depth_errors: predictions %d .. %d, but the pack holds %d ground-truth maps" % (
            first, first + n - 1, len(pack)))
    px0, b0 = int(pack.offsets[first]), int(pack.blk_first[first])
    errors, ratios, depth, med = eigen_depth_errors_launch(
        pred_disp, pred_disp_flip, pack.gt, pack.table, pack.blk_img, pack.medians, first, b0, int(pack.blk_first[first + n]) - b0,
        px0, int(pack.offsets[first + n]) - px0, pack.eigen, scale_factor, median_scaling)
    return (errors, ratios, depth, med) if return_pred else (errors, ratios)


# ----------------------------------------------------------------------------------------------------------------- K29
POSE_SCALE = 0.01       # MD2/networks/pose_decoder.py:49


def pose_invert_mask(invert, nf):
    """Bit f set = frame f of the head is inverted (Rot^T Trans(-t): a negative frame id, MD2/trainer.py:408-410).  ``invert``: a
    bool for all frames or one bool per frame -- host values, they travel to the kernel as an argument."""
    if torch.is_tensor(invert):
        raise RuntimeError("pose_head: invert is a bool or a sequence of bools (a kernel argument), not a tensor")
    flags = [bool(invert)] * nf if isinstance(invert, (bool, int, np.bool_)) else [bool(v) for v in invert]
    if len(flags) != nf:
        raise RuntimeError("pose_head: %d invert flags for %d frames" % (len(flags), nf))
    return sum(1 << f for f, v in enumerate(flags) if v)


def _pose_head_shape(x):
    if x.dim() != 4 or x.shape[1] % 6 or x.shape[1] == 0:
        raise RuntimeError("pose_head: x must be [B, 6 * nf, h, w]; got %s" % (tuple(x.shape),))
    B, c6, h, w = x.shape
    return B, c6 // 6, h, w


def pose_head_fwd_launch(x, mask, scale):
    B, nf, h, w = _pose_head_shape(x)
    aa = torch.empty((B, nf, 1, 3), device=x.device, dtype=torch.float32)
    tr = torch.empty((B, nf, 1, 3), device=x.device, dtype=torch.float32)
    T = torch.empty((B, nf, 4, 4), device=x.device, dtype=torch.float32)
    N.check(_timed("pose_head_fwd", lambda: N.lib().dmh_pose_head_fwd(N.ptr(x), B, nf, h, w, scale, mask, N.ptr(aa), N.ptr(tr),
                                                                      N.ptr(T), N.stream())))
    return aa, tr, T


def pose_head_bwd_launch(g_T, g_aa, g_tr, aa, tr, shape, mask, scale):
    B, c6, h, w = shape
    g_x = torch.empty(tuple(shape), device=aa.device, dtype=torch.float32)
    gs = [None if g is None else _c(g.to(torch.float32)) for g in (g_T, g_aa, g_tr)]
    N.check(_timed("pose_head_bwd", lambda: N.lib().dmh_pose_head_bwd(N.ptr(gs[0]), N.ptr(gs[1]), N.ptr(gs[2]), N.ptr(aa),
                                                                      N.ptr(tr), B, c6 // 6, h, w, scale, mask, N.ptr(g_x),
                                                                      N.stream())))
    return g_x


class _PoseHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, scale):
        aa, tr, T = pose_head_fwd_launch(x, mask, scale)
        ctx.save_for_backward(aa, tr)
        ctx.cfg = (tuple(x.shape), mask, scale)
        return aa, tr, T

    @staticmethod
    def backward(ctx, g_aa, g_tr, g_T):
        aa, tr = ctx.saved_tensors
        shape, mask, scale = ctx.cfg
        if g_aa is None and g_tr is None and g_T is None:
            return None, None, None
        return pose_head_bwd_launch(g_T, g_aa, g_tr, aa, tr, shape, mask, scale), None, None


def pose_head(x, invert=False, scale=POSE_SCALE):
    """K29: the pose decoder's tail and transformation_from_parameters in one launch (MD2/networks/pose_decoder.py:47-52,
    MD2/layers.py:28-103).  x [B, 6 nf, h, w] -> (axisangle [B, nf, 1, 3], translation [B, nf, 1, 3], T [B, nf, 4, 4]);
    ``invert``: a bool, or one per frame.  Differentiable w.r.t. x through all three results (one launch)."""
    _need_cuda(x)
    _, nf, _, _ = _pose_head_shape(x)
    return _PoseHead.apply(_c(x), pose_invert_mask(invert, nf), float(scale))


# ----------------------------------------------------------------------------------------------------------------- K30
COST_VOLUME_BANDED = True       # workgroups that share an XCD take a contiguous band of tiles (speed only: same bits either way)


def _cost_volume_shapes(current_feats, lookup_feats, poses, K, invK, depth_bins, into=None):
    """(B, L, Bp, C, H, W, D) of a cost-volume call; every shape mistake is a RuntimeError here, on the host (the reference raises
    IndexError from its batch loop for the pose ones)."""
    if current_feats.dim() != 4 or lookup_feats.dim() != 5:
        raise RuntimeError("cost_volume: current_feats must be [B,C,H,W] and lookup_feats [B,L,C,H,W]; got %s and %s" % (
            tuple(current_feats.shape), tuple(lookup_feats.shape)))
    B, C, H, W = current_feats.shape
    L = lookup_feats.shape[1]
    if tuple(lookup_feats.shape) != (B, L, C, H, W) or L < 1:
        raise RuntimeError("cost_volume: lookup_feats %s does not match current_feats %s" % (
            tuple(lookup_feats.shape), tuple(current_feats.shape)))
    if poses.dim() != 4 or tuple(poses.shape[2:]) != (4, 4):
        raise RuntimeError("cost_volume: poses must be [Bp,L,4,4]; got %s" % (tuple(poses.shape),))
    Bp = poses.shape[0]
    if poses.shape[1] != L:
        raise RuntimeError("cost_volume: poses name %d lookup frames, lookup_feats holds %d" % (poses.shape[1], L))
    if not 1 <= Bp <= B:
        raise RuntimeError("cost_volume: poses has %d rows for a batch of %d (1 .. B rows; samples beyond them have no lookups)" % (Bp, B))
    for name, t in (("K", K), ("invK", invK)):
        if tuple(t.shape) != (B, 4, 4):
            raise RuntimeError("cost_volume: %s must be [%d,4,4]; got %s" % (name, B, tuple(t.shape)))
    if depth_bins.dim() != 1 or not 1 <= depth_bins.numel() <= 128:
        raise RuntimeError("cost_volume: depth_bins must be a vector of 1 .. 128 depths; got %s" % (tuple(depth_bins.shape),))
    D = depth_bins.numel()
    if C != 64:
        raise RuntimeError("cost_volume: %d feature channels; the kernel takes 64 (the layer-1 width of ResNet-18/34)" % C)
    if H < 5 or W < 5:
        raise RuntimeError("cost_volume: the matching grid must be at least 5 x 5; got %d x %d" % (H, W))
    if into is not None and (tuple(into.shape) != (B, C + D, H, W) or not into.is_contiguous() or into.dtype != torch.float32):
        raise RuntimeError("cost_volume: the buffer must be a contiguous fp32 [%d,%d,%d,%d]" % (B, C + D, H, W))
    return B, L, Bp, C, H, W, D


def cost_volume_launch(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max=True, into=None, volume=True):
    B, L, Bp, C, H, W, D = _cost_volume_shapes(current_feats, lookup_feats, poses, K, invK, depth_bins, into)
    dev = current_feats.device
    cur, look, poses, K, invK, bins = (_c(t.detach().to(torch.float32)) for t in (current_feats, lookup_feats, poses, K, invK,
                                                                                   depth_bins))
    nhwc = torch.empty((B, L, H, W, C), device=dev, dtype=torch.float32)
    cost = torch.empty((B, D, H, W), device=dev, dtype=torch.float32) if volume else None
    miss = torch.empty((B, D, H, W), device=dev, dtype=torch.float32) if volume else None
    conf = torch.empty((B, H, W), device=dev, dtype=torch.float32)
    idx = torch.empty((B, H, W), device=dev, dtype=torch.int32)
    nbytes = 4 * (cur.numel() + 3 * look.numel() + (2 * B * D * H * W if volume else 0) + (B * D * H * W if into is not None else 0))
    N.check(_timed("cost_volume", lambda: N.lib().dmh_cost_volume_fwd(
        N.ptr(cur), N.ptr(look), N.ptr(poses), N.ptr(K), N.ptr(invK), N.ptr(bins), B, L, Bp, C, H, W, D, int(bool(set_missing_to_max)),
        int(COST_VOLUME_BANDED), N.ptr(nhwc), N.ptr(cost), N.ptr(miss), N.ptr(conf), N.ptr(idx), N.ptr(into), N.stream()), nbytes))
    return cost, miss, conf, idx


def cost_volume(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max=True, into=None):
    """K30: ManyDepth's plane-sweep matching cost volume (manydepth2/networks/resnet_encoder.py:157-236, :258-265, :294-296) as
    one transposing pass plus one launch, forward only -- the reference computes it under no_grad, and so the results carry no
    gradient.  current_feats [B,64,H,W], lookup_feats [B,L,64,H,W], poses [Bp,L,4,4] with 1 <= Bp <= B, K / invK [B,4,4],
    depth_bins [D] (a device vector, D <= 128).  A lookup whose pose sums to exactly 0, and every lookup of a sample b >= Bp, is
    missing; that is read on the device.  Returns (cost_volume [B,D,H,W], missing_mask [B,D,H,W], confidence_mask [B,H,W],
    argmin [B,H,W] int32).  ``into`` [B,64+D,H,W]: its channels 64 .. 64+D-1 receive cost_volume * confidence (reduce_conv's
    input, without the cat and the in-place multiply); the volume and the mask are then not written and come back as None."""
    for t in (current_feats, lookup_feats, poses, K, invK, depth_bins) + (() if into is None else (into,)):
        _need_cuda(t)
    return cost_volume_launch(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max, into, volume=into is None)


# ----------------------------------------------------------------------------------------------------------------- K38
def cost_volume_bwd_launch(current_feats, lookup_feats, poses, K, invK, depth_bins, g, need_current=True, need_lookup=True):
    """K38: (d_current [B,64,H,W] or None, d_lookup [B,L,64,H,W] or None) of V = cost_volume * confidence for the upstream gradient
    ``g`` [B,D,H,W].  ``g`` may be a channel slice of a contiguous [B,64+D,H,W] tensor: it is read in place through its batch
    stride.  The gradient that is not needed is not computed.  No host read."""
    B, L, Bp, Cc, H, W, D = _cost_volume_shapes(current_feats, lookup_feats, poses, K, invK, depth_bins)
    if not (need_current or need_lookup):
        return None, None
    dev = current_feats.device
    if tuple(g.shape) != (B, D, H, W) or g.dtype != torch.float32 or not g.is_cuda:
        raise RuntimeError("cost_volume_bwd: g must be a CUDA fp32 [%d,%d,%d,%d]; got %s %s on %s" % (
            B, D, H, W, g.dtype, tuple(g.shape), g.device))
    if B > 1 and g.stride(0) < D * H * W or g.stride()[1:] != (H * W, W, 1):
        g = g.contiguous()
    cur, look, poses, K, invK, bins = (_c(t.detach().to(torch.float32)) for t in (current_feats, lookup_feats, poses, K, invK,
                                                                                   depth_bins))
    nhwc = torch.empty((B, L, H, W, Cc), device=dev, dtype=torch.float32)
    dtotal = torch.empty((B, D, H, W), device=dev, dtype=torch.float32)
    acc = torch.empty((B * L * H * W * Cc + 1,), device=dev, dtype=torch.int64) if need_lookup else None
    d_cur = torch.empty((B, Cc, H, W), device=dev, dtype=torch.float32) if need_current else None
    d_look = torch.empty((B, L, Cc, H, W), device=dev, dtype=torch.float32) if need_lookup else None
    nbytes = 4 * (2 * cur.numel() + 3 * look.numel() + 3 * B * D * H * W) + (20 * look.numel() if need_lookup else 0)
    N.check(_timed("cost_volume_bwd", lambda: N.lib().dmh_cost_volume_bwd(
        N.ptr(cur), N.ptr(look), N.ptr(poses), N.ptr(K), N.ptr(invK), N.ptr(bins), B, L, Bp, Cc, H, W, D, C.c_void_p(g.data_ptr()),
        g.stride(0) if B > 1 else D * H * W, N.ptr(nhwc), N.ptr(dtotal), None if acc is None else C.c_void_p(acc.data_ptr()),
        N.ptr(d_cur), N.ptr(d_look), N.stream()), nbytes))
    return d_cur, d_look


def cost_volume_stack_fwd_launch(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max=True):
    """(stacked [B,64+D,H,W], confidence, argmin): K30 into the buffer plus the copy of the current features."""
    B, _, _, C, H, W, D = _cost_volume_shapes(current_feats, lookup_feats, poses, K, invK, depth_bins)
    stacked = torch.empty((B, C + D, H, W), device=current_feats.device, dtype=torch.float32)
    _, _, conf, idx = cost_volume_launch(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max, stacked,
                                         volume=False)
    stacked[:, :C] = current_feats.detach()
    return stacked, conf, idx


class _CostVolumeStack(torch.autograd.Function):
    """cat([current_feats, cost_volume * confidence], 1) as one node: K30 forward, K38 backward."""

    @staticmethod
    def forward(ctx, current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max):
        stacked, conf, idx = cost_volume_stack_fwd_launch(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max)
        ctx.save_for_backward(current_feats, lookup_feats, poses, K, invK, depth_bins)
        ctx.mark_non_differentiable(conf, idx)
        return stacked, conf, idx

    @staticmethod
    def backward(ctx, g, _g_conf, _g_idx):
        cur, look, poses, K, invK, bins = ctx.saved_tensors
        Cc = cur.shape[1]
        g = _c(g)
        d_cur, d_look = cost_volume_bwd_launch(cur, look, poses, K, invK, bins, g[:, Cc:], ctx.needs_input_grad[0],
                                               ctx.needs_input_grad[1])
        if d_cur is not None:
            d_cur += g[:, :Cc]
        return d_cur, d_look, None, None, None, None, None


def cost_volume_module(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max=True):
    """(cost_volume, missing_mask), both [B,D,H,W], in torch, any device and dtype, differentiable: match_features
    (manydepth2/networks/resnet_encoder.py:157-236) as plain expressions of the reference's arithmetic -- the module path of
    ``ResnetEncoderMatching`` and the CPU restatement the GPU tests compare with."""
    F = torch.nn.functional
    B, Cc, H, W = current_feats.shape
    D = depth_bins.numel()
    dev, dt = current_feats.device, current_feats.dtype
    depths = depth_bins.to(device=dev, dtype=dt).view(D, 1, 1)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W)], 0).unsqueeze(0).to(device=dev, dtype=dt)
    ones = torch.ones(D, 1, H * W, device=dev, dtype=dt)
    current_mask = torch.zeros(D, H, W, device=dev, dtype=dt)
    current_mask[:, 2:-2, 2:-2] = 1.0
    volumes, masks = [], []
    for b in range(B):
        cost = torch.zeros(D, H, W, device=dev, dtype=dt)
        counts = torch.zeros(D, H, W, device=dev, dtype=dt)
        points = torch.cat([depths * torch.matmul(invK[b:b + 1, :3, :3], pix), ones], 1)
        for l in range(lookup_feats.shape[1]):
            pose = poses[b:b + 1, l]
            if pose.sum() == 0:
                continue
            P = torch.matmul(K[b:b + 1], pose)[:, :3, :]
            cam = torch.matmul(P, points)
            grid = cam[:, :2, :] / (cam[:, 2, :].unsqueeze(1) + 1e-7)
            grid = grid.view(D, 2, H, W).permute(0, 2, 3, 1).clone()
            grid[..., 0] /= W - 1
            grid[..., 1] /= H - 1
            grid = (grid - 0.5) * 2
            warped = F.grid_sample(lookup_feats[b:b + 1, l].expand(D, Cc, H, W), grid, padding_mode='zeros', mode='bilinear',
                                   align_corners=True)
            x_vals = (grid[..., 0] / 2 + 0.5) * (W - 1)
            y_vals = (grid[..., 1] / 2 + 0.5) * (H - 1)
            edge = ((x_vals >= 2.0) * (x_vals <= W - 2) * (y_vals >= 2.0) * (y_vals <= H - 2)).to(dt) * current_mask
            diffs = torch.abs(warped - current_feats[b:b + 1]).mean(1) * edge
            cost = cost + diffs
            counts = counts + (diffs > 0).to(dt)
        cost = cost / (counts + 1e-7)
        miss = (cost == 0).to(dt)
        if set_missing_to_max:
            cost = cost * (1 - miss) + cost.max(0)[0].unsqueeze(0) * miss
        volumes.append(cost)
        masks.append(miss)
    return torch.stack(volumes, 0), torch.stack(masks, 0)


def cost_volume_stack_host(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max=True):
    """The definition in torch (any device and dtype; autograd differentiates it): the path of CPU tensors."""
    cost, miss = cost_volume_module(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max)
    conf = ((cost * (1 - miss) > 0).sum(1) == depth_bins.numel()).to(cost.dtype).detach()
    viz = torch.where(cost == 0, torch.full_like(cost, 100.0), cost)
    argmin = torch.min(viz.detach(), 1)[1].to(torch.int32)
    return torch.cat([current_feats, cost * conf.unsqueeze(1)], 1), conf, argmin


def cost_volume_stack(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max=True):
    """reduce_conv's input of the multi-frame call WITH gradient: (stacked [B,64+D,H,W], confidence [B,H,W], argmin [B,H,W] int32),
    ``stacked[:, :64] = current_feats`` and ``stacked[:, 64:] = cost_volume * confidence``.  One autograd node on CUDA fp32 tensors
    (K30 forward, K38 backward): d current = g[:, :64] + K38's d_current, d lookup = K38's d_lookup, and the one that is not
    required is not computed.  The sample positions, masks, counts and the confidence are constants, as torch autograd treats them
    in the module expression; the reference itself computes the volume under no_grad -- this gradient is this project's addition.
    CPU tensors take ``cost_volume_stack_host``."""
    if not current_feats.is_cuda:
        return cost_volume_stack_host(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max)
    for t in (current_feats, lookup_feats, poses, K, invK, depth_bins):
        _need_cuda(t)
    if current_feats.dtype != torch.float32 or lookup_feats.dtype != torch.float32:
        raise RuntimeError("libdmh_hip ops compute in fp32; got %s, %s" % (current_feats.dtype, lookup_feats.dtype))
    _cost_volume_shapes(current_feats, lookup_feats, poses, K, invK, depth_bins)
    return _CostVolumeStack.apply(_c(current_feats), _c(lookup_feats), poses, K, invK, depth_bins, bool(set_missing_to_max))


def cost_volume_bwd_host(current_feats, lookup_feats, poses, K, invK, depth_bins, g):
    """K38's formulas in numpy, in the dtype of ``current_feats`` (float32 or float64): (d_current [B,C,H,W], d_lookup
    [B,L,C,H,W]) of V = cost_volume * confidence for the upstream gradient ``g`` [B,D,H,W].  Positions, masks, counts and the
    confidence are constants; sgn(0) = 0; taps outside the map and non-finite positions get nothing; a lookup whose pose sums to
    exactly 0, or of a sample b >= Bp, is skipped."""
    cur = np.asarray(current_feats)
    dtype = cur.dtype.type
    if dtype not in (np.float32, np.float64):
        raise RuntimeError("cost_volume_bwd_host: float32 or float64 arrays; got %s" % cur.dtype)
    look, poses, K, invK, bins, g = (np.asarray(t).astype(dtype) for t in (lookup_feats, poses, K, invK, depth_bins, g))
    B, Cc, H, W = cur.shape
    L, D, Bp = look.shape[1], bins.shape[0], poses.shape[0]
    one, half, two, eps = dtype(1), dtype(0.5), dtype(2), dtype(1e-7)
    wm1, hm1 = dtype(W - 1), dtype(H - 1)
    ys, xs = np.meshgrid(np.arange(H).astype(dtype), np.arange(W).astype(dtype), indexing="ij")
    cur_mask = np.zeros((H, W), dtype=dtype)
    cur_mask[2:-2, 2:-2] = 1
    d_cur, d_look = np.zeros_like(cur), np.zeros_like(look)
    for b in range(B):
        iK = invK[b]
        cam = [iK[r, 0] * xs + iK[r, 1] * ys + iK[r, 2] for r in range(3)]
        pts = [bins[:, None, None] * cam[r][None] for r in range(3)]
        total, counts = np.zeros((D, H, W), dtype), np.zeros((D, H, W), dtype)
        kept = []           # per lookup that counts: (l, sign * edge [C,D,H,W], taps [(flat index, weight)])
        for l in range(L):
            if b >= Bp:
                continue
            T = poses[b, l]
            s = dtype(0)
            for v in T.reshape(-1):
                s = s + v
            if s == 0:
                continue
            P = np.zeros((3, 4), dtype)
            for r in range(3):
                for cc in range(4):
                    a = K[b, r, 0] * T[0, cc]
                    for k in (1, 2, 3):
                        a = a + K[b, r, k] * T[k, cc]
                    P[r, cc] = a
            proj = [((P[r, 0] * pts[0] + P[r, 1] * pts[1]) + P[r, 2] * pts[2]) + P[r, 3] for r in range(3)]
            den = proj[2] + eps
            with np.errstate(divide="ignore", invalid="ignore"):
                gx = ((proj[0] / den) / wm1 - half) * two
                gy = ((proj[1] / den) / hm1 - half) * two
                xv, yv = (gx / two + half) * wm1, (gy / two + half) * hm1
                edge = ((xv >= 2) & (xv <= W - 2) & (yv >= 2) & (yv <= H - 2)).astype(dtype) * cur_mask[None]
                ix, iy = ((gx + one) / two) * wm1, ((gy + one) / two) * hm1
            ix = np.nan_to_num(ix, nan=-5.0, posinf=-5.0, neginf=-5.0)
            iy = np.nan_to_num(iy, nan=-5.0, posinf=-5.0, neginf=-5.0)
            x0, y0 = np.floor(ix), np.floor(iy)
            wx1, wy1, wx0, wy0 = ix - x0, iy - y0, (x0 + 1) - ix, (y0 + 1) - iy
            feat = look[b, l].reshape(Cc, H * W)
            warped = np.zeros((Cc, D, H, W), dtype)
            taps = []
            for dy, dx, wgt in ((0, 0, wx0 * wy0), (0, 1, wx1 * wy0), (1, 0, wx0 * wy1), (1, 1, wx1 * wy1)):
                xt, yt = x0 + dx, y0 + dy
                ok = (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)
                flat = (np.where(ok, yt, 0) * W + np.where(ok, xt, 0)).astype(np.int64)
                wgt = np.where(ok, wgt, 0).astype(dtype)
                warped = warped + feat[:, flat] * wgt[None]
                taps.append((flat, wgt))
            delta = warped - cur[b][:, None]
            diffs = (np.abs(delta).sum(0, dtype=dtype) / dtype(Cc)) * edge
            total = total + diffs
            counts = counts + (diffs > 0).astype(dtype)
            kept.append((l, np.sign(delta) * edge[None], taps))
        cost = total / (counts + eps)
        conf = ((cost > 0).sum(0) == D).astype(dtype)
        dtotal = (g[b] / (counts + eps)) * conf[None]
        for l, sg, taps in kept:
            dw = sg * (dtotal[None] / dtype(Cc))                      # d warped_l [C,D,H,W]
            d_cur[b] -= dw.sum(1, dtype=dtype)
            out = np.zeros((H * W, Cc), dtype)
            dwt = np.ascontiguousarray(dw.reshape(Cc, -1).T)
            for flat, wgt in taps:
                np.add.at(out, flat.reshape(-1), dwt * wgt.reshape(-1, 1))
            d_look[b, l] = out.T.reshape(Cc, H, W)
    return d_cur, d_look


# ------------------------------------------------------------------------------------ the loader operators (K31, K32, K34)
class _UploadCache(object):
    """The last ``cap`` sets of small tables a loader operator has uploaded, by key, so that a repeated batch shape launches with
    the same device buffers and no copy.  An entry keeps the event of its upload -- a hit on another stream a moment later waits
    for it -- and the pinned host copies, which live as long as the upload may.  A key a captured graph has launched with is
    ``held``: a replay reads its buffers, so it is never evicted.  ``what``: the error a miss raises inside a capture."""

    def __init__(self, cap, what):
        self.cap, self.what, self.entries, self.held = cap, what, OrderedDict(), set()

    def __len__(self):
        return len(self.entries)

    def __contains__(self, key):
        return key in self.entries

    def get(self, key, device, make):
        """(device tensors, payload) of ``key``; at a miss ``make()`` gives (host tensors, payload): the tensors are pinned and
        uploaded without a wait, the payload (host values that go with them) is kept as it is."""
        hit = self.entries.get(key)
        if hit is not None:
            self.entries.move_to_end(key)
            if torch.cuda.is_current_stream_capturing():
                self.held.add(key)
            elif not hit[1].query():
                torch.cuda.current_stream(device).wait_event(hit[1])        # uploaded on another stream a moment ago
            return hit[0], hit[3]
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(self.what)
        host, payload = make()
        host = [h.pin_memory() for h in host]
        on_device = [h.to(device, non_blocking=True) for h in host]
        uploaded = torch.cuda.Event()
        uploaded.record(torch.cuda.current_stream(device))
        self.entries[key] = (on_device, uploaded, host, payload)
        for old in [k for k in self.entries if k not in self.held][:max(0, len(self.entries) - self.cap)]:
            del self.entries[old]
        return on_device, payload


def _flip_operand(name, flip, n, dev):
    """The per-item ``flip`` of a loader operator as the kernel reads it: None, or a contiguous int32 tensor of ``n`` entries on
    ``dev`` (a host sequence of bools is uploaded from pinned memory)."""
    if flip is None:
        return None
    if not torch.is_tensor(flip):
        flip = torch.tensor([int(bool(v)) for v in flip], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    if flip.dtype != torch.int32 or flip.numel() != n or flip.device != dev:
        raise RuntimeError("%s: flip must be an int32 tensor of %d entries on %s" % (name, n, dev))
    return _c(flip)


# ----------------------------------------------------------------------------------------------------------------- K31
PIL_FILTERS = {"lanczos": (N.PIL_LANCZOS, 3.0), "bilinear": (N.PIL_BILINEAR, 1.0)}      # name -> (PIL's number, support)
PIL_PRECISION_BITS = 22
PIL_DESC_CACHE = 64         # descriptor sets kept per process (a few hundred bytes each); the tables themselves are never repeated
PilLevel = namedtuple("PilLevel", ["u8", "f32"])
_pil_axis_cache = {}
# (device, sizes, out, filter) -> descriptors on the device
_pil_device_cache = _UploadCache(PIL_DESC_CACHE, "pil_resize: the first call with these source sizes uploads their descriptors; "
                                                 "make it once before capturing a graph")
_pil_graph_keys = _pil_device_cache.held


def _pil_filter(filter):
    try:
        return PIL_FILTERS[str(filter).lower()]
    except KeyError:
        raise RuntimeError("pil_resize: filter must be one of %s; got %r" % (sorted(PIL_FILTERS), filter))


def _pil_weight(x, support):
    """Pillow's filter functions (Resample.c: bilinear_filter; lanczos_filter = sinc(x) sinc(x / 3) on [-3, 3)) on Python
    floats: ``math.sin`` is the C library's, as Pillow's is."""
    import math
    if support == 1.0:
        x = -x if x < 0.0 else x
        return 1.0 - x if x < 1.0 else 0.0
    if not -3.0 <= x < 3.0:
        return 0.0

    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / 3)


def pil_axis_table(in_size, out_size, filter="lanczos"):
    """Host: Pillow's coefficients of one axis (Resample.c precompute_coeffs + normalize_coeffs_8bpc) for ``in_size`` ->
    ``out_size``: (xmin int32 [out], count int32 [out], k int32 [out, ksize]).  float64 in Pillow's order -- the taps
    ``filter((x + xmin - center + 0.5) * (1 / filterscale))`` summed by index, each divided by the sum -- then integers with 22
    fraction bits, rounded half away from zero.  Equal sizes give the pass Pillow skips as the table (x, 1, 2^22).  Cached."""
    in_size, out_size = int(in_size), int(out_size)
    number, support0 = _pil_filter(filter)
    if not (0 < in_size < (1 << 20) and 0 < out_size < (1 << 20)):
        raise RuntimeError("pil_axis_table: sizes must be in [1, 2^20); got %d -> %d" % (in_size, out_size))
    key = (in_size, out_size, number)
    hit = _pil_axis_cache.get(key)
    if hit is not None:
        return hit
    if in_size == out_size:
        tab = (np.arange(out_size, dtype=np.int32), np.ones(out_size, dtype=np.int32),
               np.full((out_size, 1), 1 << PIL_PRECISION_BITS, dtype=np.int32))
    else:
        import math
        scale = in_size / out_size
        filterscale = max(scale, 1.0)
        support = support0 * filterscale
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / filterscale
        xmins, counts = np.zeros(out_size, dtype=np.int32), np.zeros(out_size, dtype=np.int32)
        k = np.zeros((out_size, ksize), dtype=np.int32)
        one = float(1 << PIL_PRECISION_BITS)
        for xx in range(out_size):
            center = (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), in_size) - xmin
            w = [_pil_weight((x + xmin - center + 0.5) * ss, support0) for x in range(xmax)]
            ww = 0.0
            for v in w:
                ww += v
            if ww != 0.0:
                w = [v / ww for v in w]
            xmins[xx], counts[xx] = xmin, xmax
            k[xx, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        tab = (xmins, counts, k)
    for a in tab:
        a.setflags(write=False)
    _pil_axis_cache[key] = tab
    return tab


def _pil_pass_host(a, table, sums=None):
    """One pass of Pillow's 8-bit resample along the last axis of uint8 ``a``: clip((2^21 + sum(p k)) >> 22, 0, 255) in int32.
    ``sums`` (a list) receives the sums before the shift and the clip."""
    xmin, count, k = table
    idx = np.minimum(xmin[:, None] + np.arange(k.shape[1])[None, :], a.shape[-1] - 1)      # taps past ``count`` weigh 0
    acc = (a[..., idx].astype(np.int32) * k).sum(-1, dtype=np.int32) + np.int32(1 << (PIL_PRECISION_BITS - 1))
    if sums is not None:
        sums.append(acc)
    return np.clip(acc >> PIL_PRECISION_BITS, 0, 255).astype(np.uint8)


def pil_quantize_host(x):
    """torchvision's ``ToPILImage`` on a float tensor: ``pic.mul(255).byte()``, a truncation in fp32."""
    return (np.asarray(x, dtype=np.float32) * np.float32(255.0)).astype(np.uint8)


def pil_resize_host(img, out_size, filter="lanczos", flip=False, sums=None):
    """Host twin of K31 in numpy: ``PIL.Image.fromarray(img).resize((out_w, out_h), filter)`` of uint8 ``img`` [..., H, W]
    (planar: leading axes are channels or a batch), bit-equal to Pillow's.  ``flip``: transpose(FLIP_LEFT_RIGHT) first.  The
    horizontal pass runs first into an 8-bit intermediate; a pass whose size does not change is skipped."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim < 2:
        raise RuntimeError("pil_resize_host: need a uint8 array [..., H, W]; got %s %s" % (img.dtype, img.shape))
    oh, ow = (int(v) for v in out_size)
    if flip:
        img = img[..., ::-1]
    H, W = img.shape[-2:]
    if W != ow:
        img = _pil_pass_host(img, pil_axis_table(W, ow, filter), sums)
    if H != oh:
        img = np.swapaxes(_pil_pass_host(np.swapaxes(img, -1, -2), pil_axis_table(H, oh, filter), sums), -1, -2)
    return np.ascontiguousarray(img)


class _PilArena(object):
    """The axis tables of one device: one int32 tensor that holds every distinct (in, out, filter) table once, at a word offset
    that never changes.  KITTI raw has about five frame sizes, so the arena stops growing after the first batches; when a new
    table arrives the whole arena is uploaded again (pinned, asynchronous) and the upload is waited for once, so that any stream
    may read it afterwards."""

    def __init__(self, device):
        self.device, self.entries, self.words, self.tables = device, {}, [], None
        self.tile_rows = {}

    def place(self, n_in, n_out, number, filter):
        """(word offset, ksize) of the table; ``self.tables`` is stale until ``sync`` when this added one."""
        key = (n_in, n_out, number)
        if key not in self.entries:
            xmin, count, k = pil_axis_table(n_in, n_out, filter)
            flat = np.concatenate([xmin, count, np.ascontiguousarray(k.T).reshape(-1)])
            want = N.lib().dmh_pil_resample_tables_size(n_in, n_out, number)
            if want != flat.size:
                raise RuntimeError("pil_resize: the table of %d -> %d has %d words, the library expects %d" % (n_in, n_out, flat.size, want))
            self.entries[key] = (sum(w.size for w in self.words), k.shape[1])
            self.words.append(flat)
            self.tables = None
        return self.entries[key]

    def rows(self, h, oh, filter, number):
        """The most source rows one tile of PIL_TILE_ROWS output rows needs on the vertical axis h -> oh."""
        key = (h, oh, number)
        if key not in self.tile_rows:
            tile = N.PIL_TILE_ROWS
            ymin, count, _ = pil_axis_table(h, oh, filter)
            last_i = np.minimum(np.arange(tile - 1, oh + tile - 1, tile), oh - 1)
            self.tile_rows[key] = int((ymin[last_i] + count[last_i] - ymin[::tile]).max())
        return self.tile_rows[key]

    def sync(self):
        if self.tables is None:
            host = torch.from_numpy(np.concatenate(self.words)).pin_memory()
            self.tables = host.to(self.device, non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.device))
            done.synchronize()          # once per new table: later calls, on any stream, read a finished upload
        return self.tables


_pil_arenas = {}


def _pil_tables_device(device, sizes, oh, ow, number, filter):
    """(tables int32 [words], desc int32 [N, 8], lds_rows) on ``device`` for a batch whose images have the source sizes
    ``sizes`` (a tuple of (h, w)).  The tables live once per distinct (in, out, filter) in the device's arena; what depends on
    the batch is the descriptor set alone (32 bytes per image), kept in ``_pil_device_cache``: a repeated batch shape -- a
    captured graph's, a pyramid's coarser levels -- launches with the same device buffer and no copy."""
    arena = _pil_arenas.get(str(device))
    if arena is None:
        arena = _pil_arenas[str(device)] = _PilArena(device)

    def make():
        desc, lds_rows = np.zeros((len(sizes), 8), dtype=np.int32), 1
        for i, (h, w) in enumerate(sizes):
            (ho, hk), (vo, vk) = arena.place(w, ow, number, filter), arena.place(h, oh, number, filter)
            desc[i, :6] = (h, w, ho, hk, vo, vk)
            lds_rows = max(lds_rows, arena.rows(h, oh, filter, number))
        if lds_rows * ow > 65536:
            raise RuntimeError("pil_resize: %d source rows of %d output columns per tile exceed the 64 KiB LDS tile; resize in two "
                               "steps" % (lds_rows, ow))
        return [torch.from_numpy(desc)], lds_rows
    (desc_d,), lds_rows = _pil_device_cache.get((str(device), sizes, oh, ow, number), device, make)
    return arena.sync(), desc_d, lds_rows


def _pil_sizes(sizes, n, H, W):
    if sizes is None:
        return ((H, W),) * n
    sizes = tuple((int(h), int(w)) for h, w in (sizes.tolist() if hasattr(sizes, "tolist") else sizes))
    if len(sizes) != n or not all(0 < h <= H and 0 < w <= W for h, w in sizes):
        raise RuntimeError("pil_resize: sizes must be %d pairs (h, w) within the buffer's %d x %d; got %s" % (n, H, W, sizes))
    return sizes


def pil_resize(src, out_size, filter="lanczos", flip=None, sizes=None, want_float=True, layout=None, want_u8=True):
    """K31: ``PIL.Image.resize((out_w, out_h), filter)`` of a batch of 8-bit images, bit for bit, in one launch.

    src      uint8 [N, H, W, C] (``layout="hwc"``, the default for uint8: decoded files), uint8 [N, C, H, W]
             (``layout="chw"``: a previous level), or float32 [N, C, H, W] in [0, 1], quantised on read as ToPILImage does.
    sizes    per image (h, w) <= (H, W): the image lies in the top-left corner of its slot (host values: they choose the tables).
    flip     per image, a device int32 [N] (or a host sequence of bools): != 0 resizes transpose(FLIP_LEFT_RIGHT) of the image.
    Returns  PilLevel(u8 uint8 [N, C, out_h, out_w] or None, f32 = u8.float() / 255 or None).

    CPU tensors run the numpy restatement of the same integers (``pil_resize_host``)."""
    number, _ = _pil_filter(filter)
    oh, ow = (int(v) for v in out_size)
    if oh < 1 or ow < 1:
        raise RuntimeError("pil_resize: out_size must be positive; got %s" % (tuple(out_size),))
    if src.dim() != 4 or src.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError("pil_resize: src must be uint8 or float32 with 4 dimensions; got %s %s" % (src.dtype, tuple(src.shape)))
    if not (want_float or want_u8):
        raise RuntimeError("pil_resize: nothing to return (want_float and want_u8 are both off)")
    layout = layout or ("hwc" if src.dtype == torch.uint8 else "chw")
    if layout not in ("hwc", "chw") or (src.dtype == torch.float32 and layout != "chw"):
        raise RuntimeError("pil_resize: layout must be 'hwc' or 'chw' (float32 sources are 'chw'); got %r" % (layout,))
    n, (H, W, C_) = int(src.shape[0]), ((int(v) for v in src.shape[1:]) if layout == "hwc" else (int(src.shape[2]), int(src.shape[3]), int(src.shape[1])))
    sizes = _pil_sizes(sizes, n, H, W)
    if src.device.type != "cuda":
        planar = src.permute(0, 3, 1, 2) if layout == "hwc" else src
        planar = planar.numpy() if src.dtype == torch.uint8 else pil_quantize_host(planar.numpy())
        flips = [False] * n if flip is None else [bool(v) for v in (flip.tolist() if hasattr(flip, "tolist") else flip)]
        if len(flips) != n:
            raise RuntimeError("pil_resize: flip must have one entry per image")
        u8 = torch.from_numpy(np.stack([pil_resize_host(planar[i, :, :h, :w], (oh, ow), filter, flips[i])
                                        for i, (h, w) in enumerate(sizes)]))
        return PilLevel(u8 if want_u8 else None, u8.float().div(255) if want_float else None)
    src = _c(src)
    dev = src.device
    flip = _flip_operand("pil_resize", flip, n, dev)
    tables, desc, lds_rows = _pil_tables_device(dev, sizes, oh, ow, number, filter)
    u8 = torch.empty((n, C_, oh, ow), device=dev, dtype=torch.uint8) if want_u8 else None
    f32 = torch.empty((n, C_, oh, ow), device=dev, dtype=torch.float32) if want_float else None
    strides = (H * W * C_, 1, W * C_, C_) if layout == "hwc" else (C_ * H * W, H * W, W, 1)
    N.check(_timed("pil_resample", lambda: N.lib().dmh_pil_resample(
        N.ptr(src), int(src.dtype == torch.float32), *strides, H, W, N.ptr(tables), int(tables.numel()), N.ptr(desc),
        N.ptr(flip), n, C_, oh, ow, lds_rows, N.ptr(u8), N.ptr(f32), N.stream()),
        src.numel() * src.element_size() + n * C_ * oh * ow * (int(want_u8) + 4 * int(want_float))))
    return PilLevel(u8, f32)


def pil_pyramid(src, height, width, num_scales=4, filter="lanczos", flip=None, sizes=None, want_float=True, layout=None):
    """The loader's image pyramid (MD2/datasets/mono_dataset.py:100-104,119-144): level 0 is ``src`` resized to height x width,
    level i the 8-bit level i - 1 resized to (height // 2^i) x (width // 2^i) -- one launch of K31 per level.  ``flip`` applies to
    level 0 (the reference flips the loaded image).  Returns ``num_scales`` PilLevel(u8, f32)."""
    levels = []
    for i in range(int(num_scales)):
        s = 2 ** i
        if height // s < 1 or width // s < 1:
            raise RuntimeError("pil_pyramid: level %d of %d x %d is empty" % (i, height, width))
        if i == 0:
            levels.append(pil_resize(src, (height, width), filter, flip, sizes, want_float, layout))
        else:
            levels.append(pil_resize(levels[-1].u8, (height // s, width // s), filter, None, None, want_float, "chw"))
    return levels


# ---------------------------------------------------------------------------------------------------------------- K32
VELO_EMPTY, VELO_DESC_CACHE = 0xFFFFFFFF, 16
_velo_desc_cache = _UploadCache(VELO_DESC_CACHE, "velo_depth_map: the first call with these shapes uploads their descriptors; make "
                                                 "it once before capturing a graph")     # (device, shapes) -> descriptors


def nearest_index(n_in, n_out):
    """Source index of every output index of K32's nearest resize: ((2 o + 1) n_in) // (2 n_out), the exact-arithmetic value of
    the pixel-centre mapping round((o + 0.5) n_in / n_out - 0.5); the identity when the sizes agree."""
    o = np.arange(int(n_out), dtype=np.int64)
    return ((2 * o + 1) * int(n_in)) // (2 * int(n_out))


def _velo_shapes(shapes, n):
    shapes = tuple((int(h), int(w)) for h, w in (shapes.tolist() if hasattr(shapes, "tolist") else shapes))
    if len(shapes) != n or not all(h >= 1 and w >= 2 for h, w in shapes):
        raise RuntimeError("velo_depth_map: shapes must be %d pairs (H, W) with H >= 1 and W >= 2; got %s" % (n, shapes))
    return shapes


def _velo_frame_host(pts, P, H, W, vel_depth):
    """One frame of K32 in numpy -> float32 [H, W]: the kernel's arithmetic in the kernel's order (csrc/velo_depth.hip)."""
    idx = np.nonzero(pts[:, 0] >= 0)[0]                     # a NaN fails the test
    x, y, z = (pts[idx, c].astype(np.float64) for c in range(3))
    with np.errstate(all="ignore"):
        q = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]
        u, v = np.rint(q[0] / q[2]) - 1.0, np.rint(q[1] / q[2]) - 1.0
        keep = (u >= 0) & (v >= 0) & (u < W) & (v < H)      # NaN and inf fall out
        d = (x if vel_depth else q[2])[keep]
        val = np.where(d > 0, d, 0.0).astype(np.float32)    # float32(max(d, 0)); rounding and the clamp are monotone
    idx, ui, vi = idx[keep], u[keep].astype(np.int64), v[keep].astype(np.int64)
    if idx.size == 0:
        return np.zeros((H, W), dtype=np.float32)
    bits = val.view(np.uint32)                             # non-negative floats order as their bits do
    cells = np.full(H * W, VELO_EMPTY, dtype=np.uint32)
    np.minimum.at(cells, vi * W + ui, bits)
    out = np.where(cells == VELO_EMPTY, np.uint32(0), cells).reshape(H, W)
    if H > 1:
        # the reference's sub2ind gives A = (y, W - 1) and B = (y + 1, 0) one key: where both hold points, the one that holds the
        # pair's earliest point gets the minimum over both, the other keeps its last point's value
        first = np.full((H, 2), np.iinfo(np.int64).max, dtype=np.int64)
        last = np.full((H, 2), -1, dtype=np.int64)
        for side, col in ((0, 0), (1, W - 1)):
            on = ui == col
            np.minimum.at(first[:, side], vi[on], idx[on])
            np.maximum.at(last[:, side], vi[on], idx[on])
        cells = cells.reshape(H, W)
        a, b = cells[:-1, W - 1], cells[1:, 0]
        both = (a != VELO_EMPTY) & (b != VELO_EMPTY)
        a_first = first[:-1, 1] < first[1:, 0]
        low = np.minimum(a, b)
        pos = np.full(pts.shape[0], -1, dtype=np.int64)
        pos[idx] = np.arange(idx.size)
        last_a, last_b = bits[pos[np.maximum(last[:-1, 1], 0)]], bits[pos[np.maximum(last[1:, 0], 0)]]
        out[:-1, W - 1] = np.where(both, np.where(a_first, low, last_a), out[:-1, W - 1])
        out[1:, 0] = np.where(both, np.where(a_first, last_b, low), out[1:, 0])
    return out.view(np.float32)


def velo_depth_map_host(points, offsets, proj, shapes, vel_depth=False, out_size=None, flip=None):
    """K32 in numpy, the definition the kernel is held to (and the path CPU tensors take): vectorised, no loop per duplicate.
    points float32 [npts, 4], offsets [n + 1], proj float64 [n, 3, 4] or [n, 12], shapes n pairs (H, W).  Returns float32
    [n, out_h, out_w] with ``out_size``, else the list of the n maps at their own sizes."""
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
    offsets = [int(v) for v in np.asarray(offsets).reshape(-1)]
    n = len(offsets) - 1
    proj = np.asarray(proj, dtype=np.float64).reshape(n, 3, 4)
    shapes = _velo_shapes(shapes, n)
    flips = [False] * n if flip is None else [bool(v) for v in np.asarray(flip).reshape(-1)]
    if len(flips) != n:
        raise RuntimeError("velo_depth_map: flip must have one entry per frame")
    if offsets[0] < 0 or offsets[-1] > points.shape[0] or any(a > b for a, b in zip(offsets[:-1], offsets[1:])):
        raise RuntimeError("velo_depth_map: offsets must ascend within the %d points; got %s" % (points.shape[0], offsets))
    maps = []
    for f, (H, W) in enumerate(shapes):
        m = _velo_frame_host(points[offsets[f]:offsets[f + 1]], proj[f], H, W, bool(vel_depth))
        if out_size is not None:
            m = m[nearest_index(H, out_size[0])][:, nearest_index(W, out_size[1])]
        maps.append(np.ascontiguousarray(m[:, ::-1] if flips[f] else m))
    return np.stack(maps) if out_size is not None else maps


def _velo_desc_device(device, shapes):
    def make():
        cells = np.cumsum([0] + [h * w for h, w in shapes])
        rows = np.cumsum([0] + [h for h, _ in shapes])
        return [torch.tensor([[h, w, int(cells[i]), int(rows[i])] for i, (h, w) in enumerate(shapes)], dtype=torch.int32)], None
    return _velo_desc_cache.get((str(device), shapes), device, make)[0][0]


def velo_depth_map(points, offsets, proj, shapes, vel_depth=False, out_size=None, flip=None):
    """K32: the sparse depth maps of a batch of velodyne scans (MD2/kitti_utils.py:46-98, generate_depth_map, float32-equal),
    with the loader's nearest resize and flip (MD2/datasets/kitti_dataset.py:70-85).

    points   float32 [npts, 4], the frames' points packed in file order; offsets int32 [n + 1] on the same device.
    proj     float64 [n, 3, 4] (or [n, 12]): P_velo2im of each frame (datasets.kitti_velo.velo_projection).
    shapes   n pairs (H, W): each frame's image size.  Host values: they size the workspace and the output.
    flip     per frame, an int32 tensor [n] on the device (or a host sequence of bools): != 0 mirrors the columns.
    Returns  float32 [n, out_h, out_w] with ``out_size``; without it (flat float32 [sum H W], cell offsets as a list of n + 1
             ints): frame f is flat[off[f]:off[f + 1]].view(H, W).

    CPU tensors run ``velo_depth_map_host``, the numpy restatement the kernel is bit-equal to."""
    if not torch.is_tensor(points) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 4:
        raise RuntimeError("velo_depth_map: points must be a float32 tensor [npts, 4]; got %s %s"
                           % (getattr(points, "dtype", type(points)), tuple(getattr(points, "shape", ()))))
    _eigen_i32(offsets, "offsets")
    n = offsets.numel() - 1
    if offsets.dim() != 1 or n < 1:
        raise RuntimeError("velo_depth_map: offsets must hold n + 1 >= 2 entries; got %s" % (tuple(offsets.shape),))
    if not torch.is_tensor(proj) or proj.dtype != torch.float64 or proj.numel() != 12 * n:
        raise RuntimeError("velo_depth_map: proj must be a float64 tensor of %d x 12 entries; got %s %s"
                           % (n, getattr(proj, "dtype", type(proj)), tuple(getattr(proj, "shape", ()))))
    shapes = _velo_shapes(shapes, n)
    if out_size is not None:
        out_size = tuple(int(v) for v in out_size)
        if len(out_size) != 2 or out_size[0] < 1 or out_size[1] < 1:
            raise RuntimeError("velo_depth_map: out_size must be a positive (h, w); got %s" % (out_size,))
    cell_off = [int(v) for v in np.cumsum([0] + [h * w for h, w in shapes])]
    dev = points.device
    if offsets.device != dev or proj.device != dev:
        raise RuntimeError("velo_depth_map: points, offsets and proj must share a device")
    if dev.type != "cuda":
        res = velo_depth_map_host(points.numpy(), offsets.numpy(), proj.numpy(), shapes, vel_depth, out_size,
                                  None if flip is None else (flip.tolist() if hasattr(flip, "tolist") else flip))
        if out_size is not None:
            return torch.from_numpy(res)
        return torch.from_numpy(np.concatenate([m.reshape(-1) for m in res])), cell_off
    flip = _flip_operand("velo_depth_map", flip, n, dev)
    lib = N.lib()
    total_cells, total_rows = cell_off[-1], sum(h for h, _ in shapes)
    words = lib.dmh_velo_depth_ws_size(total_cells, total_rows)
    if words < 0:
        raise RuntimeError("velo_depth_map: %d cells and %d rows do not fit a 2^31-word workspace" % (total_cells, total_rows))
    desc = _velo_desc_device(dev, shapes)
    ws = torch.empty(words, device=dev, dtype=torch.int32)
    out = torch.empty((n,) + out_size if out_size is not None else (total_cells,), device=dev, dtype=torch.float32)
    points, proj = _c(points), _c(proj)
    oh, ow = out_size if out_size is not None else (0, 0)
    N.check(_timed("velo_depth_map", lambda: lib.dmh_velo_depth_map(
        N.ptr(points) if points.numel() else None, int(points.shape[0]), N.ptr(_c(offsets)), N.ptr_f64(proj), N.ptr(desc),
        N.ptr(flip), n, int(bool(vel_depth)), total_cells, total_rows, oh, ow, N.ptr(ws), N.ptr(out),
        N.stream()), points.numel() * 4 + 8 * words + out.numel() * 4))
    return out if out_size is not None else (out, cell_off)


# ---------------------------------------------------------------------------------------------------------------- K33
JITTER_MAX_TENSORS = 8                  # DMH_JITTER_MAX_TENSORS
JITTER_MAX_PIXELS = (2 ** 32 - 1) // 255  # 255 H W must fit the 32-bit sum of L


def _jitter_L(img):
    """Pillow's ``convert("L")`` of uint8 [3, H, W] -> int32 [H, W]."""
    r, g, b = (img[c].astype(np.int32) for c in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16


def _jitter_blend(deg, img, f):
    """``Image.blend(degenerate, image, f)`` per channel: float32, the product and the sum rounded separately; truncated to a byte
    for 0 <= f <= 1, clipped outside."""
    f = np.float32(f)
    d = np.asarray(deg).astype(np.float32)
    t = d + f * (img.astype(np.float32) - d)
    if np.float32(0) <= f <= np.float32(1):
        return t.astype(np.int32).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def _jitter_hue(img, shift):
    """``convert("HSV")``, the shift added to the H byte modulo 256, ``convert("RGB")`` (Pillow's Convert.c rgb2hsv / hsv2rgb)."""
    r, g, b = (img[c].astype(np.int32) for c in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    flat = mx == mn
    cr = np.where(flat, 1, mx - mn).astype(np.float32)
    s = cr / np.where(flat, 1, mx).astype(np.float32)
    rc, gc, bc = ((mx - c).astype(np.float32) / cr for c in (r, g, b))
    rc64, gc64, bc64 = (c.astype(np.float64) for c in (rc, gc, bc))
    h = np.where(r == mx, bc64 - gc64, np.where(g == mx, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(np.float32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    H = np.where(flat, 0, np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255))
    S = np.where(flat, 0, np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255))
    V = mx
    H = (H + int(shift)) & 255
    fs = S / 255.0
    x = H * 6.0 / 255.0
    i = np.floor(x)
    fr = x - i

    def byte(z):        # C's round (half away from zero; z >= 0 here), then CLIP8
        return np.clip(np.floor(z + 0.5), 0, 255).astype(np.int32)
    p, q, t = byte(V * (1.0 - fs)), byte(V * (1.0 - fs * fr)), byte(V * (1.0 - fs * (1.0 - fr)))
    k = i.astype(np.int32) % 6
    grey = S == 0
    out = [np.where(grey, V, np.choose(k, table)) for table in ((V, q, p, p, t, V), (t, V, V, q, p, p), (p, p, t, V, V, q))]
    return np.stack(out).astype(np.uint8)


def pil_color_jitter_host(images, records, sums=None):
    """Host twin of K33 in numpy, bit-equal to Pillow: torchvision 0.8.2's ColorJitter on 8-bit PIL images.  ``images``: uint8
    arrays [B, 3, H, W]; ``records``: int32 [B, 8] (color_jitter.pil_records).  Every operation ends in a byte: brightness =
    blend(0, img, f), saturation = blend(L(img), img, f), contrast = blend(m, img, f) with m = int(mean of L over this image as the
    operations before left it + 0.5), hue = the HSV round trip with the shifted H byte.  Returns the uint8 results; ``sums`` (a
    list) receives the integer sum of L of every image that took a contrast step."""
    records = np.asarray(records, dtype=np.int32).reshape(-1, 8)
    out = []
    for img in images:
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 4 or img.shape[1] != 3 or img.shape[0] != records.shape[0]:
            raise RuntimeError("pil_color_jitter_host: need uint8 arrays [%d, 3, H, W]; got %s %s" % (records.shape[0], img.dtype, img.shape))
        res = np.empty_like(img)
        for i, rec in enumerate(records):
            x = img[i]
            factors = rec[2:5].view(np.float32)
            seen_contrast = False
            for k in range(min(max(int(rec[0]), 0), 4)):
                op = (int(rec[1]) >> (8 * k)) & 255
                if op == 0:
                    x = _jitter_blend(0, x, factors[0])
                elif op == 1:
                    L = _jitter_L(x)
                    S = int(L.sum(dtype=np.int64))
                    if sums is not None and not seen_contrast:
                        sums.append(S)
                    seen_contrast = True
                    x = _jitter_blend(int(S / float(L.size) + 0.5), x, factors[1])
                elif op == 2:
                    x = _jitter_blend(_jitter_L(x)[None], x, factors[2])
                elif op == 3:
                    x = _jitter_hue(x, int(rec[5]) & 255)
            res[i] = x
        out.append(res)
    return out


def pil_color_jitter(images, params, want_u8=False):
    """K33: torchvision 0.8.2's ``ColorJitter`` on 8-bit PIL images (MD2/datasets/mono_dataset.py:344-348, :133, :144), Pillow's
    bytes, for a whole batch and all its keys in two launches (one when no item has a contrast step).

    images   a list of at most 8 uint8 tensors [B, 3, H, W] on one device (K31's level-0 ``u8``): item i of every tensor takes
             transform i; every image has its own contrast mean.
    params   a list of B ``color_jitter.JitterParams`` or None (None: the item is only converted), or the prepared int32 record
             [B, 8] on the images' device (``color_jitter.pil_records``; a captured graph reads it at every replay).
    Returns  a list of PilLevel(u8 or None, f32 = u8.float() / 255), one per tensor.

    CPU tensors run ``pil_color_jitter_host``, the numpy restatement the kernel is bit-equal to."""
    from . import color_jitter
    from .my_utils import to_device_async
    images = list(images)
    if not 1 <= len(images) <= JITTER_MAX_TENSORS:
        raise RuntimeError("pil_color_jitter: one call takes 1 .. %d tensors; got %d" % (JITTER_MAX_TENSORS, len(images)))
    first = images[0]
    for t in images:
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[1] != 3 or t.shape != first.shape or t.device != first.device:
            raise RuntimeError("pil_color_jitter: images must be uint8 tensors [B, 3, H, W] of one shape on one device; got %s %s"
                               % (getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
    B, _, H, W = (int(v) for v in first.shape)
    if B < 1 or H < 1 or W < 1 or H * W > JITTER_MAX_PIXELS:
        raise RuntimeError("pil_color_jitter: need a non-empty batch of images of at most %d pixels (255 H W must fit 32 bits); "
                           "got %d x %d x %d" % (JITTER_MAX_PIXELS, B, H, W))
    dev = first.device
    if torch.is_tensor(params):
        if params.dtype != torch.int32 or params.numel() != 8 * B or params.device != dev:
            raise RuntimeError("pil_color_jitter: a prepared record is an int32 tensor [%d, 8] on %s" % (B, dev))
        rec, with_contrast = params, True
    else:
        host = color_jitter.pil_records(params)
        if host.shape[0] != B:
            raise RuntimeError("pil_color_jitter: params must hold one entry per item (%d); got %d" % (B, host.shape[0]))
        with_contrast = bool(color_jitter.records_have_contrast(host))
        rec = host if dev.type != "cuda" else to_device_async(host, dev)
    if dev.type != "cuda":
        res = [torch.from_numpy(a) for a in pil_color_jitter_host([t.numpy() for t in images], rec.numpy() if torch.is_tensor(rec) else rec)]
        return [PilLevel(u8 if want_u8 else None, u8.float().div(255)) for u8 in res]
    images = [_c(t) for t in images]
    rec = _c(rec)
    f32 = [torch.empty((B, 3, H, W), device=dev, dtype=torch.float32) for _ in images]
    u8 = [torch.empty((B, 3, H, W), device=dev, dtype=torch.uint8) for _ in images] if want_u8 else None
    T = len(images)
    words = N.lib().dmh_color_jitter_ws_size(T, B, H, W)
    if words < 0:
        raise RuntimeError("pil_color_jitter: %d tensors of %d x 3 x %d x %d are more than one call takes (T B <= 65535, "
                           "B 3 H W < 2^31)" % (T, B, H, W))
    ws = torch.empty(words, device=dev, dtype=torch.int32) if with_contrast else None
    N.check(_timed("color_jitter", lambda: N.lib().dmh_color_jitter(
        N.ptr_array(images, JITTER_MAX_TENSORS), N.ptr_array(f32, JITTER_MAX_TENSORS),
        N.ptr_array(u8, JITTER_MAX_TENSORS) if want_u8 else None, T, B, H, W, N.ptr(rec), int(with_contrast), N.ptr(ws), N.stream()),
        T * B * H * W * 3 * (1 + 4 + int(want_u8)) + (T * B * H * W * 3 if with_contrast else 0)))
    return [PilLevel(u8[i] if want_u8 else None, f32[i]) for i in range(T)]


# ---------------------------------------------------------------------------------------------------------------- K34
HINT_MAX_CANDIDATES = 16
HINT_TABLE_CACHE = 8
_hint_table_cache = _UploadCache(HINT_TABLE_CACHE, "depth_hint_prepare: the first call with these sizes uploads their index tables; "
                                                   "make it once before capturing a graph")     # (device, Hs, Ws, H, W) -> (ytab, xtab)


def hint_candidate_depths(cand, K):
    """depth-hints/precompute_depth_hints.py:142,151 for a batch: StereoSGBM's int16 output [B, N, H, W] (disparity x 16, -16 where
    nothing matched) -> float32 depths, fx 0.1 / (disp + 1e-7) * (disp > 0) with fx = K[b, 0, 0], as torch computes it on the CPU."""
    disps = torch.from_numpy(cand.cpu().numpy() / 16).float()
    fx = K.detach().cpu().float()[:, 0, 0].view(-1, 1, 1, 1)
    return fx * 0.1 / (disps + 1e-7) * (disps > 0).float()


def _hint_check(base, lookup, cand, K, inv_K, T):
    if not (torch.is_tensor(base) and base.dtype == torch.uint8 and base.dim() == 4 and base.shape[1] == 3):
        raise RuntimeError("depth_hint_fuse: base must be a uint8 tensor [B, 3, H, W]; got %s %s"
                           % (getattr(base, "dtype", type(base)), tuple(getattr(base, "shape", ()))))
    B, _, H, W = (int(v) for v in base.shape)
    if not (torch.is_tensor(lookup) and lookup.dtype == torch.uint8 and lookup.shape == base.shape):
        raise RuntimeError("depth_hint_fuse: lookup must be a uint8 tensor of base's shape %s; got %s %s"
                           % (tuple(base.shape), getattr(lookup, "dtype", type(lookup)), tuple(getattr(lookup, "shape", ()))))
    if not (torch.is_tensor(cand) and cand.dtype in (torch.int16, torch.float32) and cand.dim() == 4 and cand.shape[0] == B
            and tuple(cand.shape[2:]) == (H, W)):
        raise RuntimeError("depth_hint_fuse: cand must be int16 (disparity x 16) or float32 (depths) [%d, N, %d, %d]; got %s %s"
                           % (B, H, W, getattr(cand, "dtype", type(cand)), tuple(getattr(cand, "shape", ()))))
    n = int(cand.shape[1])
    if not 1 <= n <= HINT_MAX_CANDIDATES:
        raise RuntimeError("depth_hint_fuse: 1 <= N <= %d candidates; got %d" % (HINT_MAX_CANDIDATES, n))
    if B < 1 or H < 2 or W < 2:
        raise RuntimeError("depth_hint_fuse: need B >= 1 and H, W >= 2; got %d x %d x %d" % (B, H, W))
    for name, m in (("K", K), ("inv_K", inv_K), ("T", T)):
        if not (torch.is_tensor(m) and m.dtype == torch.float32 and tuple(m.shape) == (B, 4, 4)):
            raise RuntimeError("depth_hint_fuse: %s must be a float32 tensor [%d, 4, 4]; got %s %s"
                               % (name, B, getattr(m, "dtype", type(m)), tuple(getattr(m, "shape", ()))))
    for t in (lookup, cand, K, inv_K, T):
        if t.device != base.device:
            raise RuntimeError("depth_hint_fuse: every operand must be on base's device %s; got %s" % (base.device, t.device))
    return B, n, H, W


def _hint_ssim(x, y):
    """depth-hints/layers.py SSIM.forward."""
    import torch.nn.functional as F
    x, y = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
    mu_x, mu_y = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
    sigma_x = F.avg_pool2d(x ** 2, 3, 1) - mu_x ** 2
    sigma_y = F.avg_pool2d(y ** 2, 3, 1) - mu_y ** 2
    sigma_xy = F.avg_pool2d(x * y, 3, 1) - mu_x * mu_y
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    n = (2 * mu_x * mu_y + C1) * (2 * sigma_xy + C2)
    d = (mu_x ** 2 + mu_y ** 2 + C1) * (sigma_x + sigma_y + C2)
    return torch.clamp((1 - n / d) / 2, 0, 1)


def depth_hint_fuse_host(base, lookup, cand, K, inv_K, T, want_losses=False, dtype=torch.float32):
    """K34 in plain torch on the CPU, the definition the kernel is held to (and the path CPU tensors take): the lines
    precompute_depth_hints.py:247-252 with BackprojectDepth, Project3D and SSIM of depth-hints/layers.py, item by item with the
    candidates as the batch.  The candidate depths are float32 in every form (they are inputs: ``hint_candidate_depths`` for
    int16); ``dtype=torch.float64`` computes everything after them in float64: the anchor.  Returns best_depth float32
    [B, 1, H, W], with ``want_losses`` (best_depth, losses ``dtype`` [B, N, H, W])."""
    import torch.nn.functional as F
    B, n, H, W = _hint_check(base, lookup, cand, K, inv_K, T)
    depths = hint_candidate_depths(cand, K) if cand.dtype == torch.int16 else cand.detach().cpu()
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=dtype)], 0).unsqueeze(0)     # [1, 3, HW]
    ones = torch.ones(n, 1, H * W, dtype=dtype)
    best, losses = [], []
    for b in range(B):
        Kb, iKb, Tb = (m[b:b + 1].detach().cpu().to(dtype) for m in (K, inv_K, T))
        d = depths[b].to(dtype)
        cam = torch.matmul(iKb[:, :3, :3], pix)
        cam = torch.cat([d.reshape(n, 1, -1) * cam, ones], 1)
        P = torch.matmul(Kb, Tb)[:, :3, :]
        cp = torch.matmul(P, cam)
        pc = cp[:, :2, :] / (cp[:, 2, :].unsqueeze(1) + 1e-7)
        pc = pc.view(n, 2, H, W).permute(0, 2, 3, 1)
        pc[..., 0] /= W - 1
        pc[..., 1] /= H - 1
        pc = (pc - 0.5) * 2
        img_l = (lookup[b:b + 1].cpu().to(dtype) / 255).expand(n, -1, -1, -1)
        img_b = (base[b:b + 1].cpu().to(dtype) / 255).expand(n, -1, -1, -1)
        sample = F.grid_sample(img_l, pc, padding_mode="border", align_corners=False)
        l1 = torch.abs(img_b - sample).mean(1, True)
        loss = 0.85 * _hint_ssim(sample, img_b).mean(1, True) + 0.15 * l1
        index = torch.argmin(loss, dim=0)
        best.append(torch.gather(depths[b].unsqueeze(1), 0, index.unsqueeze(0))[0])
        losses.append(loss[:, 0])
    best = torch.stack(best).float()
    return (best, torch.stack(losses)) if want_losses else best


def depth_hint_fuse(base, lookup, cand, K, inv_K, T, want_losses=False):
    """K34: DepthHints' fused hint selection (depth-hints/precompute_depth_hints.py:247-252) for a batch of stereo pairs in one
    launch: per candidate depth map the other view warped into the base view (grid_sample's defaults, border padding), SSIM + L1
    against the base image, the lowest loss per pixel (the lowest index among equal float32 losses), its depth.

    base, lookup  uint8 [B, 3, H, W] (``pil_resize(..., want_u8=True).u8``): the view the hint is for, and the other one.
    cand          int16 [B, N, H, W]: StereoSGBM's raw output (disparity x 16, -16 = no match), converted as the reference does;
                  or float32 [B, N, H, W]: depths.  1 <= N <= 16.
    K, inv_K, T   float32 [B, 4, 4]; T[b, 0, 3] = -0.1 for a left base image, +0.1 for a right one.
    Returns       best_depth float32 [B, 1, H, W]; with ``want_losses`` (best_depth, losses float32 [B, N, H, W]).

    CPU tensors run ``depth_hint_fuse_host``."""
    B, n, H, W = _hint_check(base, lookup, cand, K, inv_K, T)
    if base.device.type != "cuda":
        return depth_hint_fuse_host(base, lookup, cand, K, inv_K, T, want_losses)
    if B * n * H * W >= 2 ** 31 or B > 65535:
        raise RuntimeError("depth_hint_fuse: B N H W must stay below 2^31 and B below 65536; got %d x %d x %d x %d" % (B, n, H, W))
    base, lookup, cand, K, inv_K, T = (_c(t) for t in (base, lookup, cand, K, inv_K, T))
    best = torch.empty((B, 1, H, W), device=base.device, dtype=torch.float32)
    losses = torch.empty((B, n, H, W), device=base.device, dtype=torch.float32) if want_losses else None
    raw = cand.dtype == torch.int16
    N.check(_timed("depth_hint_fuse", lambda: N.lib().dmh_depth_hint_fuse(
        N.ptr(base), N.ptr(lookup), C.c_void_p(cand.data_ptr()), int(raw), N.ptr(K), N.ptr(inv_K), N.ptr(T), B, n, H, W, N.ptr(best),
        N.ptr(losses), N.stream()), B * H * W * (6 + n * (2 if raw else 4) + 4 + (4 * n if want_losses else 0))))
    return (best, losses) if want_losses else best


def cv_nearest_index(n_src, n_dst):
    """Source index of every destination index of OpenCV's INTER_NEAREST along one axis, as its source states it (resizeNN:
    min(floor(dst * (double)src / dst_size), src - 1)); the identity when the sizes agree."""
    scale = float(int(n_src)) / float(int(n_dst))
    return np.minimum(np.floor(np.arange(int(n_dst), dtype=np.float64) * scale).astype(np.int64), int(n_src) - 1)


def _hint_prepare_check(hints, flip, out_size):
    if not (torch.is_tensor(hints) and hints.dtype == torch.float32 and hints.dim() == 4 and hints.shape[1] == 1 and hints.numel() > 0):
        raise RuntimeError("depth_hint_prepare: hints must be a non-empty float32 tensor [B, 1, Hs, Ws]; got %s %s"
                           % (getattr(hints, "dtype", type(hints)), tuple(getattr(hints, "shape", ()))))
    out_size = tuple(int(v) for v in out_size)
    if len(out_size) != 2 or out_size[0] < 1 or out_size[1] < 1:
        raise RuntimeError("depth_hint_prepare: out_size must be a positive (h, w); got %s" % (out_size,))
    B = int(hints.shape[0])
    if flip is not None:
        n = flip.numel() if torch.is_tensor(flip) else len(flip)
        if n != B:
            raise RuntimeError("depth_hint_prepare: flip must have one entry per item (%d); got %d" % (B, n))
    return B, int(hints.shape[2]), int(hints.shape[3]), out_size[0], out_size[1]


def depth_hint_prepare_host(hints, flip, out_size):
    """depth-hints/datasets/mono_dataset.py:382-388 for a batch in numpy: np.fliplr of the flipped items, OpenCV's INTER_NEAREST
    to ``out_size`` (``cv_nearest_index``), the mask (hint > 0).  Returns (depth_hint, depth_hint_mask) float32 [B, 1, H, W]."""
    B, Hs, Ws, H, W = _hint_prepare_check(hints, flip, out_size)
    src = hints.detach().cpu().numpy()
    flips = [False] * B if flip is None else [bool(v) for v in (flip.tolist() if hasattr(flip, "tolist") else flip)]
    yi, xi = cv_nearest_index(Hs, H), cv_nearest_index(Ws, W)
    out = np.empty((B, 1, H, W), dtype=np.float32)
    for b in range(B):
        a = np.fliplr(src[b, 0]) if flips[b] else src[b, 0]
        out[b, 0] = a[yi][:, xi]
    hint = torch.from_numpy(out)
    return hint, (hint > 0).float()


def _hint_tables_device(device, Hs, Ws, H, W):
    def make():
        return [torch.from_numpy(cv_nearest_index(a, b).astype(np.int32)) for a, b in ((Hs, H), (Ws, W))], None
    return _hint_table_cache.get((str(device), Hs, Ws, H, W), device, make)[0]


def depth_hint_prepare(hints, flip, out_size):
    """The loader's side of a stored depth hint (depth-hints/datasets/mono_dataset.py:382-388) for a batch in one launch.

    hints     float32 [B, 1, Hs, Ws]: the loaded ``.npy`` files.
    flip      None, an int32 tensor [B] on the hints' device, or a host sequence of bools: != 0 is np.fliplr before the resize.
    out_size  (H, W): cv2.resize(..., INTER_NEAREST) to it; at Hs, Ws == H, W a (mirrored) copy.
    Returns   (depth_hint, depth_hint_mask = (depth_hint > 0).float()), float32 [B, 1, H, W].

    CPU tensors run ``depth_hint_prepare_host``."""
    B, Hs, Ws, H, W = _hint_prepare_check(hints, flip, out_size)
    dev = hints.device
    if dev.type != "cuda":
        return depth_hint_prepare_host(hints, flip, out_size)
    flip = _flip_operand("depth_hint_prepare", flip, B, dev)
    ytab, xtab = _hint_tables_device(dev, Hs, Ws, H, W)
    hints = _c(hints)
    hint = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    mask = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    N.check(_timed("depth_hint_prepare", lambda: N.lib().dmh_depth_hint_prepare(
        N.ptr(hints), N.ptr(flip), N.ptr(ytab), N.ptr(xtab), H, W, B, Hs, Ws, H, W, N.ptr(hint),
        N.ptr(mask), N.stream()), B * H * W * 12))
    return hint, mask


# ---------------------------------------------------------------------------------------------------------------- K35
SGM_MAX_MATCHERS = 16
SGM_MAX_WIDTH = 4096
SGM_WORKSPACE_CAP = 2 << 30
SGM_PC_MAX = 567                    # 3 channels x (126 prefiltered + 255 >> 2 raw): the largest pixel cost
_SGM_KEYS = ("numDisparities", "blockSize", "P1", "P2", "preFilterCap", "uniquenessRatio", "disp12MaxDiff", "speckleWindowSize",
             "speckleRange", "minDisparity")
_SGM_DEFAULTS = dict(disp12MaxDiff=0, minDisparity=0)


def _sgm_params(params):
    """The parameter sets as tuples in ``_SGM_KEYS`` order, each refused where the matcher does not serve it."""
    if isinstance(params, dict):
        params = [params]
    params = list(params)
    if not 1 <= len(params) <= SGM_MAX_MATCHERS:
        raise RuntimeError("sgm_disparity: 1 <= N <= %d parameter sets; got %d" % (SGM_MAX_MATCHERS, len(params)))
    out = []
    for p in params:
        unknown = set(p) - set(_SGM_KEYS)
        if unknown:
            raise RuntimeError("sgm_disparity: unknown parameter(s) %s; the keys are %s" % (sorted(unknown), list(_SGM_KEYS)))
        missing = [k for k in _SGM_KEYS if k not in p and k not in _SGM_DEFAULTS]
        if missing:
            raise RuntimeError("sgm_disparity: a parameter set lacks %s" % missing)
        D, b, P1, P2, cap, uniq, d12, spw, spr, mind = t = tuple(int(p.get(k, _SGM_DEFAULTS.get(k, 0))) for k in _SGM_KEYS)
        if mind != 0:
            raise RuntimeError("sgm_disparity: minDisparity must be 0; got %d" % mind)
        if D % 16 != 0 or not 16 <= D <= 256:
            raise RuntimeError("sgm_disparity: numDisparities must be a multiple of 16 in [16, 256]; got %d" % D)
        if not 1 <= b <= 3:
            raise RuntimeError("sgm_disparity: blockSize must be 1, 2 or 3 (radius <= 1, for which int16 sums are exact); got %d" % b)
        side = 2 * (b // 2) + 1
        if P1 < 0 or P2 < 0 or 5 * (side * side * SGM_PC_MAX + P2) >= 32767:
            raise RuntimeError("sgm_disparity: P1, P2 >= 0 and 5 ((2r+1)^2 %d + P2) < 32767 (int16 sums); got P1 %d, P2 %d at "
                               "blockSize %d" % (SGM_PC_MAX, P1, P2, b))
        if not 1 <= cap <= 63 or not 0 <= uniq <= 100 or not 0 <= d12 <= 32767 or spw < 0 or not 0 <= spr <= 4096:
            raise RuntimeError("sgm_disparity: need preFilterCap in [1, 63], uniquenessRatio in [0, 100], disp12MaxDiff in [0, 32767], "
                               "speckleWindowSize >= 0 and speckleRange in [0, 4096]; got %s" % (dict(zip(_SGM_KEYS, t)),))
        out.append(t)
    return out


def _sgm_check(base, lookup, params, reverse):
    if not (torch.is_tensor(base) and base.dtype == torch.uint8 and base.dim() == 4 and base.shape[1] == 3 and base.numel() > 0):
        raise RuntimeError("sgm_disparity: base must be a non-empty uint8 tensor [B, 3, H, W]; got %s %s"
                           % (getattr(base, "dtype", type(base)), tuple(getattr(base, "shape", ()))))
    if not (torch.is_tensor(lookup) and lookup.dtype == torch.uint8 and lookup.shape == base.shape and lookup.device == base.device):
        raise RuntimeError("sgm_disparity: lookup must be a uint8 tensor of base's shape %s on its device; got %s %s"
                           % (tuple(base.shape), getattr(lookup, "dtype", type(lookup)), tuple(getattr(lookup, "shape", ()))))
    B, _, H, W = (int(v) for v in base.shape)
    plist = _sgm_params(params)
    if W > SGM_MAX_WIDTH or H > 65535 or B * len(plist) * H * W >= 2 ** 31:
        raise RuntimeError("sgm_disparity: need W <= %d, H <= 65535 and B N H W < 2^31; got %d x %d x %d x %d"
                           % (SGM_MAX_WIDTH, B, len(plist), H, W))
    if reverse is not None:
        n = reverse.numel() if torch.is_tensor(reverse) else len(reverse)
        if n != B:
            raise RuntimeError("sgm_disparity: reverse must have one entry per item (%d); got %d" % (B, n))
    return B, H, W, plist


def _sgm_lo_hi(A):
    left = np.concatenate([A[..., :1], A[..., :-1]], -1)
    right = np.concatenate([A[..., 1:], A[..., -1:]], -1)
    hl, hr = (A + left) >> 1, (A + right) >> 1
    return np.minimum(A, np.minimum(hl, hr)), np.maximum(A, np.maximum(hl, hr))


def _sgm_block_cost(base, lookup, D, r, cap):
    """Steps 1-3 for one pair: C int32 [H, Wv, D]."""
    _, H, W = base.shape
    kinds = []
    for img in (base.astype(np.int32), lookup.astype(np.int32)):
        rows = np.pad(img, ((0, 0), (1, 1), (0, 0)), mode="edge")
        dx = rows[:, :, 2:] - rows[:, :, :-2]                           # [3, H + 2, W - 2]
        g = np.full(img.shape, cap, dtype=np.int32)
        g[:, :, 1:W - 1] = np.clip(dx[:, :-2] + 2 * dx[:, 1:-1] + dx[:, 2:], -cap, cap) + cap
        A = np.concatenate([g, img], 0)                                 # [6, H, W]
        kinds.append((A,) + _sgm_lo_hi(A))
    (u, lo_u, hi_u), (v, lo_v, hi_v) = kinds
    cols = np.arange(D, W)[:, None] - np.arange(D)[None, :]             # [Wv, D]: the lookup column of (x, d)
    pc = np.zeros((H, W - D, D), dtype=np.int32)
    for k in range(6):                                                  # g of the three channels, then their bytes
        a, lo_a, hi_a = (t[k][:, D:, None] for t in (u, lo_u, hi_u))
        b, lo_b, hi_b = (t[k][:, cols] for t in (v, lo_v, hi_v))
        bt = np.minimum(np.maximum(0, np.maximum(a - hi_b, lo_b - a)), np.maximum(0, np.maximum(b - hi_a, lo_a - b)))
        pc += bt if k < 3 else bt >> 2
    if r == 0:
        return pc
    pad = np.pad(pc, ((r, r), (r, r), (0, 0)), mode="edge")
    Wv = W - D
    return sum(pad[dy:dy + H, dx:dx + Wv] for dy in range(2 * r + 1) for dx in range(2 * r + 1))


def _sgm_step(C, q, P1, P2):
    """One step of a path for a whole front: C, q [..., D] -> L."""
    big = np.int32(1 << 28)
    m = q.min(-1, keepdims=True)
    down = np.concatenate([np.full_like(q[..., :1], big), q[..., :-1]], -1)
    up = np.concatenate([q[..., 1:], np.full_like(q[..., :1], big)], -1)
    return C + np.minimum(np.minimum(q, np.minimum(down, up) + P1), m + P2) - m


def _sgm_aggregate(C, P1, P2):
    H, Wv, D = C.shape
    S = np.zeros_like(C)
    for cols in (range(Wv), range(Wv - 1, -1, -1)):                     # from the left, from the right: all rows at once
        L = None
        for x in cols:
            L = C[:, x] if L is None else _sgm_step(C[:, x], L, P1, P2)
            S[:, x] += L
    for dx in (-1, 0, 1):                                               # from above: all columns at once
        L = C[0]
        S[0] += L
        for y in range(1, H):
            q = L if dx == 0 else np.roll(L, -dx, axis=0)               # q[x] = L[x + dx]
            new = _sgm_step(C[y], q, P1, P2)
            if dx == -1:
                new[0] = C[y, 0]
            elif dx == 1:
                new[Wv - 1] = C[y, Wv - 1]
            L = new
            S[y] += L
    return S


def _sgm_select(S, W, uniq, d12):
    """Steps 5 and 6: S [H, Wv, D] -> int32 [H, W]."""
    H, Wv, D = S.shape
    out = np.full((H, W), -16, dtype=np.int32)
    d_star = S.argmin(-1)
    min_s = np.take_along_axis(S, d_star[..., None], -1)[..., 0]
    far = np.abs(np.arange(D)[None, None, :] - d_star[..., None]) > 1
    unique = ~((S * (100 - uniq) < 100 * min_s[..., None]) & far).any(-1)
    sm = np.take_along_axis(S, np.maximum(d_star - 1, 0)[..., None], -1)[..., 0]
    sp = np.take_along_axis(S, np.minimum(d_star + 1, D - 1)[..., None], -1)[..., 0]
    den = np.maximum(sm + sp - 2 * min_s, 1)
    num = (sm - sp) * 16 + den
    frac = np.sign(num) * (np.abs(num) // (2 * den))                    # C's division
    value = 16 * d_star + np.where((d_star == 0) | (d_star == D - 1), 0, frac)
    out[:, D:] = np.where(unique, value, -16)
    xs = np.broadcast_to(np.arange(D, W)[None, :], (H, Wv))
    ys = np.broadcast_to(np.arange(H)[:, None], (H, Wv))
    none = np.int64(1) << 40
    keys = np.full((H, W), none, dtype=np.int64)
    np.minimum.at(keys, (ys[unique], (xs - d_star)[unique]), (min_s.astype(np.int64)[unique] << 16) | xs[unique])
    owner = np.where(keys == none, D, keys & 0xffff).astype(np.int64)   # the proposer's column (D where nobody proposed)
    disp2 = np.take_along_axis(d_star, owner - D, 1)
    is_set = keys != none
    xa = np.broadcast_to(np.arange(W)[None, :], (H, W))
    bad = np.zeros((H, W), dtype=np.int32)
    for k in (0, 15):
        dd = (out + k) >> 4
        x2 = xa - dd
        inside = (x2 >= 0) & (x2 < W)
        x2c = np.clip(x2, 0, W - 1)
        hit = inside & np.take_along_axis(is_set, x2c, 1) & (np.abs(np.take_along_axis(disp2, x2c, 1) - dd) > d12)
        bad += hit
    out[(out >= 0) & (bad == 2)] = -16
    return out


def _sgm_speckle(disp, window, rng16):
    """Step 7 by label propagation with pointer jumping; components do not depend on the order."""
    H, W = disp.shape
    valid = disp >= 0
    lab = np.arange(H * W, dtype=np.int64).reshape(H, W)
    right = valid[:, :-1] & valid[:, 1:] & (np.abs(disp[:, :-1] - disp[:, 1:]) <= rng16)
    down = valid[:-1] & valid[1:] & (np.abs(disp[:-1] - disp[1:]) <= rng16)
    while True:
        new = lab.copy()
        np.minimum(new[:, :-1], np.where(right, lab[:, 1:], new[:, :-1]), out=new[:, :-1])
        np.minimum(new[:, 1:], np.where(right, lab[:, :-1], new[:, 1:]), out=new[:, 1:])
        np.minimum(new[:-1], np.where(down, lab[1:], new[:-1]), out=new[:-1])
        np.minimum(new[1:], np.where(down, lab[:-1], new[1:]), out=new[1:])
        flat = new.reshape(-1)
        for _ in range(4):
            flat = flat[flat]
        new = flat.reshape(H, W)
        if np.array_equal(new, lab):
            break
        lab = new
    sizes = np.bincount(lab[valid], minlength=H * W)
    out = disp.copy()
    out[valid & (sizes[lab] <= window)] = -16
    return out


def sgm_disparity_host(base, lookup, params, reverse=None):
    """K35 in whole-image numpy on the CPU (the path CPU tensors take), bit-equal to the pixel-by-pixel statement of the matcher
    in tests/sgm_ref.py.  Returns int16 [B, N, H, W]."""
    B, H, W, plist = _sgm_check(base, lookup, params, reverse)
    flips = [False] * B if reverse is None else [bool(v) for v in (reverse.tolist() if hasattr(reverse, "tolist") else reverse)]
    b_np, l_np = base.detach().cpu().numpy(), lookup.detach().cpu().numpy()
    out = np.full((B, len(plist), H, W), -16, dtype=np.int16)
    for b in range(B):
        ib, il = (a[b, :, :, ::-1] if flips[b] else a[b] for a in (b_np, l_np))
        done = {}
        for n, (D, blk, P1, P2, cap, uniq, d12, spw, spr, _) in enumerate(plist):
            key = (D, blk // 2, P1, P2, cap, uniq, d12, spw, spr)
            if key not in done:
                disp = np.full((H, W), -16, dtype=np.int32)
                if W > D:
                    S = _sgm_aggregate(_sgm_block_cost(ib, il, D, blk // 2, cap), P1, P2)
                    disp = _sgm_select(S, W, uniq, d12)
                if spw > 0:
                    disp = _sgm_speckle(disp, spw, 16 * spr)
                done[key] = disp[:, ::-1] if flips[b] else disp
            out[b, n] = done[key]
    return torch.from_numpy(out)


def _sgm_native_params(plist):
    arr = (N.SgmParams * len(plist))()
    for i, (D, blk, P1, P2, cap, uniq, d12, spw, spr, mind) in enumerate(plist):
        arr[i] = N.SgmParams(D, blk, P1, P2, cap, uniq, d12, spw, spr, mind)
    return arr


def sgm_plan(B, H, W, params, workspace_cap=SGM_WORKSPACE_CAP):
    """(workspace bytes, sequences of launches) of ``sgm_disparity`` for a batch under ``workspace_cap`` bytes; host only."""
    plist = _sgm_params(params)
    chunks = C.c_int(0)
    nbytes = N.lib().dmh_sgm_plan(int(B), int(H), int(W), _sgm_native_params(plist), len(plist), int(workspace_cap), C.byref(chunks))
    if nbytes < 0:
        raise RuntimeError("libdmh_hip: " + N.lib().dmh_last_error().decode())
    return int(nbytes), int(chunks.value)


def sgm_disparity(base, lookup, params, reverse=None, workspace_cap=SGM_WORKSPACE_CAP, phases=N.SGM_ALL):
    """K35: the integer semi-global stereo matcher of DESIGN.md section 3 (K35) for a batch of stereo pairs on the device; every
    parameter set of ``params`` gives one map.

    base, lookup   uint8 [B, 3, H, W] (``pil_resize(..., want_u8=True).u8``): the view the disparity is for, and the other one.
    params         a list of at most 16 dicts with the keys of ``precompute_depth_hints.stereo_matcher_params()`` (and optionally
                   ``disp12MaxDiff``, 0 by default).  numDisparities a multiple of 16 in [16, 256], blockSize <= 3, minDisparity 0.
    reverse        None, an int32 tensor [B] on base's device, or a host sequence of bools: != 0 where the base image is the right
                   view (the pair is matched mirrored and the result mirrored back).
    workspace_cap  bytes the workspace may take (2 GiB by default); the batch is split into sequences of launches that fit.
    phases         ``N.SGM_ALL``; a subset launches only those phases, for tools/sgm_bench.py (the result is then undefined).
    Returns        int16 [B, N, H, W]: disparity x 16, -16 where nothing matched -- what ``depth_hint_fuse`` takes.

    CPU tensors run ``sgm_disparity_host``."""
    B, H, W, plist = _sgm_check(base, lookup, params, reverse)
    dev = base.device
    if dev.type != "cuda":
        return sgm_disparity_host(base, lookup, params, reverse)
    if reverse is not None and not torch.is_tensor(reverse):
        reverse = torch.tensor([int(bool(v)) for v in reverse], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    if reverse is not None and (reverse.dtype != torch.int32 or reverse.device != dev):
        raise RuntimeError("sgm_disparity: reverse must be an int32 tensor of %d entries on %s" % (B, dev))
    native = _sgm_native_params(plist)
    nbytes = N.lib().dmh_sgm_plan(B, H, W, native, len(plist), int(workspace_cap), None)
    if nbytes < 0:
        raise RuntimeError("libdmh_hip: " + N.lib().dmh_last_error().decode())
    base, lookup = _c(base), _c(lookup)
    out = torch.empty((B, len(plist), H, W), device=dev, dtype=torch.int16)
    ws = torch.empty(int(nbytes), device=dev, dtype=torch.uint8)
    N.check(_timed("sgm_disparity", lambda: N.lib().dmh_sgm_disparity(
        N.ptr(base), N.ptr(lookup), N.ptr(None if reverse is None else _c(reverse)), B, H, W, native, len(plist),
        C.c_void_p(out.data_ptr()), N.ptr(ws), int(nbytes), int(phases), N.stream()), B * H * W * (6 + 2 * len(plist))))
    return out


# ---------------------------------------------------------------------------------------------------------------- K37
COLORIZE_MODES = {"min_p95": N.COLORIZE_MIN_P95, "zero_ref": N.COLORIZE_ZERO_REF, "min_max": N.COLORIZE_MIN_MAX}
COLORIZE_TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "magma_256.txt")
ColorizeOut = namedtuple("ColorizeOut", ["rgb", "map", "stats"])
_colorize_table_host = None
_colorize_table_cache = _UploadCache(8, "disp_colorize: the first call on a device uploads the colour table; make it once before "
                                        "capturing a graph")


def magma_table():
    """(matplotlib's magma at 256 entries * 255).astype(uint8) as uint8 [256, 3]: data/magma_256.txt (256 lines "r g b"), written once by
    tools/make_goldens_colorize.py.  matplotlib is not imported."""
    global _colorize_table_host
    if _colorize_table_host is None:
        with open(COLORIZE_TABLE_PATH) as f:
            rows = [[int(v) for v in line.split()] for line in f if line.strip() and not line.startswith("#")]
        if len(rows) != 256 or any(len(r) != 3 or min(r) < 0 or max(r) > 255 for r in rows):
            raise RuntimeError("%s must hold 256 lines of three bytes" % COLORIZE_TABLE_PATH)
        _colorize_table_host = np.array(rows, dtype=np.uint8)
    return _colorize_table_host


def percentile_plan(n, q=95):
    """(lo, hi, g) of ``np.percentile(a, q)`` for a float32 ``a`` of n elements (numpy 2: float32 throughout): the result is
    ``lerp(sorted[lo], sorted[hi], g)``.  numpy's own expressions (the "linear" method's virtual index ``(n - 1) * quantiles`` and
    the bounds of ``_get_indexes``), evaluated in float32 as numpy evaluates them -- they depend on n and q only."""
    n = int(n)
    if n < 1:
        raise RuntimeError("percentile_plan: n must be positive; got %d" % n)
    quant = np.asanyarray(np.true_divide(q, np.float32(100)), dtype=np.float32)
    if not 0 <= float(quant) <= 1:
        raise RuntimeError("percentile_plan: q must lie in [0, 100]; got %r" % (q,))
    vi = np.asanyarray((n - 1) * quant)
    if vi.dtype != np.float32:
        raise RuntimeError("percentile_plan: the virtual index left float32 (%s)" % vi.dtype)
    if vi >= n - 1:
        return n - 1, n - 1, 0.0
    if vi < 0:
        return 0, 0, 0.0
    lo = np.floor(vi)
    return int(lo), int(lo) + 1, float(np.float32(vi - lo))


def _colorize_panels(panels, n_src):
    """Panels as (a, b, mode number, ref) tuples; the default is one ``min_p95`` panel per map."""
    if panels is None:
        panels = [(i, -1, "min_p95", i) for i in range(n_src)]
    out = []
    for i, pn in enumerate(panels):
        if len(pn) != 4:
            raise RuntimeError("disp_colorize: a panel is (a, b, mode, ref); got %r" % (pn,))
        a, b, mode, ref = pn
        mode = COLORIZE_MODES.get(mode, mode)
        if mode not in COLORIZE_MODES.values():
            raise RuntimeError("disp_colorize: mode must be one of %s; got %r" % (sorted(COLORIZE_MODES), pn[2]))
        a, b, ref = int(a), int(b), int(ref)
        if not (0 <= a < n_src and -1 <= b < n_src):
            raise RuntimeError("disp_colorize: panel %d names a map outside the batch of %d: a = %d, b = %d" % (i, n_src, a, b))
        out.append((a, b, int(mode), ref))
    if not 1 <= len(out) <= N.COLORIZE_MAX_PANELS:
        raise RuntimeError("disp_colorize: 1 <= panels <= %d; got %d" % (N.COLORIZE_MAX_PANELS, len(out)))
    for i, (a, b, mode, ref) in enumerate(out):
        if mode == N.COLORIZE_ZERO_REF and not 0 <= ref < len(out):
            raise RuntimeError("disp_colorize: panel %d takes its limit from panel %d, outside the %d panels" % (i, ref, len(out)))
    return out


def _colorize_check(maps, panels, out_size, out, origins):
    if not (torch.is_tensor(maps) and maps.dtype == torch.float32 and maps.dim() == 3 and maps.numel() > 0):
        raise RuntimeError("disp_colorize: maps must be a non-empty float32 tensor [B, h, w]; got %s %s"
                           % (getattr(maps, "dtype", type(maps)), tuple(getattr(maps, "shape", ()))))
    B, h, w = (int(v) for v in maps.shape)
    H, W = (h, w) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if H < 1 or W < 1:
        raise RuntimeError("disp_colorize: out_size must be a positive (H, W); got %s" % (out_size,))
    panels = _colorize_panels(panels, B)
    if (out is None) != (origins is None):
        raise RuntimeError("disp_colorize: out (a uint8 mosaic [Hm, Wm, 3]) and origins (one (y, x) per panel) go together")
    offsets, pitch = [i * H * W * 3 for i in range(len(panels))], W * 3
    if out is not None:
        if not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.dim() == 3 and out.shape[2] == 3 and out.is_contiguous()
                and out.device == maps.device):
            raise RuntimeError("disp_colorize: out must be a contiguous uint8 tensor [Hm, Wm, 3] on the maps' device")
        Hm, Wm = int(out.shape[0]), int(out.shape[1])
        if len(origins) != len(panels):
            raise RuntimeError("disp_colorize: one origin per panel (%d); got %d" % (len(panels), len(origins)))
        offsets, pitch = [], Wm * 3
        for y, x in origins:
            y, x = int(y), int(x)
            if not (0 <= y and y + H <= Hm and 0 <= x and x + W <= Wm):
                raise RuntimeError("disp_colorize: a %d x %d panel at (%d, %d) leaves the %d x %d mosaic" % (H, W, y, x, Hm, Wm))
            offsets.append((y * Wm + x) * 3)
    return B, h, w, H, W, panels, offsets, pitch


def colorize_bytes_host(a, vmin, vmax):
    """The bytes of ``(ScalarMappable(Normalize(vmin, vmax), 'magma').to_rgba(a)[..., :3] * 255).astype(uint8)`` for a float32
    array: float32 throughout, the index 0 where 256 x < 0, 255 where 256 x >= 256, trunc(256 x) otherwise."""
    a, vmin, vmax = np.asarray(a, dtype=np.float32), np.float32(vmin), np.float32(vmax)
    with np.errstate(all="ignore"):
        x = np.zeros_like(a) if vmin == vmax else (a - vmin) / (vmax - vmin)
        xa = x * np.float32(256)
        idx = np.where(xa < 0, 0, np.where(xa >= 256, 255, np.trunc(xa))).astype(np.int64)
    return magma_table()[idx]


def disp_colorize_host(maps, panels=None, out_size=None, out=None, origins=None, return_map=False, q=95):
    """K37's numpy twin, the arithmetic stated in csrc/disp_colorize.hip: sort instead of the radix select, numpy's float32 lerp,
    float32 limits and index, the packaged table.  With ``out_size`` the map is resized by torch's own float32 CPU
    ``F.interpolate(bilinear, align_corners=False)``, which is NOT bit-equal to the kernel's resize (torch's back ends differ among
    themselves): colour the kernel's returned map (no ``out_size``) to compare bytes."""
    B, h, w, H, W, panels, offsets, pitch = _colorize_check(maps, panels, out_size, out, origins)
    src = maps.detach().cpu().numpy()
    lo, hi, g = percentile_plan(H * W, q)
    g = np.float32(g)
    made, stats = [], np.zeros((len(panels), N.COLORIZE_STATS), dtype=np.float32)
    for i, (a, b, mode, ref) in enumerate(panels):
        m = src[a] if b < 0 else np.abs(src[a] - src[b])
        if (H, W) != (h, w):
            m = torch.nn.functional.interpolate(torch.from_numpy(np.ascontiguousarray(m))[None, None], (H, W), mode="bilinear",
                                                align_corners=False)[0, 0].numpy()
        s = np.sort(m, axis=None)
        a_lo, a_hi = s[lo], s[hi]
        d = a_hi - a_lo
        p = a_hi - d * (1 - g) if g >= 0.5 else a_lo + d * g
        stats[i] = (s[0], s[-1], a_lo, a_hi, p)
        made.append(m)
    rgb = np.empty((len(panels), H, W, 3), dtype=np.uint8)
    for i, (a, b, mode, ref) in enumerate(panels):
        vmin, vmax = ((stats[i, 0], stats[i, 4]) if mode == N.COLORIZE_MIN_P95 else
                      (np.float32(0), stats[ref, 4]) if mode == N.COLORIZE_ZERO_REF else (stats[i, 0], stats[i, 1]))
        rgb[i] = colorize_bytes_host(made[i], vmin, vmax)
    if out is not None:
        view = out.numpy()
        for i, (y, x) in enumerate(origins):
            view[int(y):int(y) + H, int(x):int(x) + W] = rgb[i]
    return ColorizeOut(out if out is not None else torch.from_numpy(rgb), torch.from_numpy(np.stack(made)) if return_map else None,
                       torch.from_numpy(stats))


def disp_colorize(maps, panels=None, out_size=None, out=None, origins=None, return_map=False, q=95):
    """K37: float maps to magma-coloured bytes, as MD2/test_simple.py:136-156 and the figures of my_utils.py:43-105 make them on
    the host, in one fixed chain of launches with no host read.

    maps      float32 [B, h, w], finite (disparities).
    panels    what is coloured: a sequence of (a, b, mode, ref) -- maps[a], or |maps[a] - maps[b]| when b >= 0, with the limits
              "min_p95" (the panel's own minimum and q-th percentile), "zero_ref" (0 and the percentile of panel ``ref``) or
              "min_max" (the panel's minimum and maximum).  Default: every map, "min_p95".
    out_size  (H, W): the source is resized first (bilinear, align_corners=False semantics); default (h, w), the input bits.
    out, origins  a uint8 mosaic [Hm, Wm, 3] and one (y, x) per panel: the panels are written into their places, nothing else
              is touched.  Without them a new uint8 [P, H, W, 3].
    Returns   ColorizeOut(rgb, map, stats): the bytes (``out`` when given), the coloured float maps [P, H, W] with ``return_map``
              (None otherwise), and float32 [P, 5] = min, max, sorted[lo], sorted[hi], the percentile as ``np.percentile`` gives it.

    CPU tensors run ``disp_colorize_host``."""
    B, h, w, H, W, panels, offsets, pitch = _colorize_check(maps, panels, out_size, out, origins)
    dev = maps.device
    if dev.type != "cuda":
        return disp_colorize_host(maps, panels, out_size, out, origins, return_map, q)
    P = len(panels)
    if P * H * W >= 2 ** 31 or B * h * w >= 2 ** 31:
        raise RuntimeError("disp_colorize: B h w and panels H W must stay below 2^31; got %d x %d x %d -> %d x %d x %d"
                           % (B, h, w, P, H, W))
    lo, hi, g = percentile_plan(H * W, q)
    table = _colorize_table_cache.get(str(dev), dev, lambda: ([torch.from_numpy(magma_table().copy())], None))[0][0]
    maps = _c(maps)
    native = (N.ColorizePanel * P)(*[N.ColorizePanel(a, b, mode, ref, off) for (a, b, mode, ref), off in zip(panels, offsets)])
    rgb = out if out is not None else torch.empty((P, H, W, 3), device=dev, dtype=torch.uint8)
    fmap = torch.empty((P, H, W), device=dev, dtype=torch.float32)
    stats = torch.empty((P, N.COLORIZE_STATS), device=dev, dtype=torch.float32)
    ws = torch.empty(N.lib().dmh_disp_colorize_ws_size(P), device=dev, dtype=torch.int32)
    N.check(_timed("disp_colorize", lambda: N.lib().dmh_disp_colorize(
        N.ptr(maps), B, h, w, native, P, H, W, lo, hi, g, N.ptr(table), N.ptr(fmap), N.ptr(ws), N.ptr(stats), N.ptr(rgb),
        rgb.numel(), pitch, N.stream()), 4 * P * (4 * H * W + h * w) + 3 * P * H * W))
    return ColorizeOut(rgb, fmap if return_map else None, stats)


# ---------------------------------------------------------------------------------------------------------------- K39
PseudoLidarOut = namedtuple("PseudoLidarOut", ["points", "offsets"])
LIDAR_FORMS = {"depth": N.LIDAR_DEPTH, "disp": N.LIDAR_DISP, "net": N.LIDAR_NET}
LIDAR_BASELINE = 0.54                   # generate_lidar.py:12
LIDAR_DESC_CACHE = 16
_lidar_desc_cache = _UploadCache(LIDAR_DESC_CACHE, "pseudo_lidar: the first call with these shapes uploads their descriptors; make it "
                                                   "once before capturing a graph")      # (device, form, shapes, offsets) -> tables


def lidar_calib(path_or_text, crop=None):
    """The 27 float64 values K39 takes for one frame -- f_u f_v c_u c_v b_x b_y, inv(R0), C2V -- from a KITTI-object calibration
    file (or its text), made as the reference's ``Calibration.__init__`` makes them (datasets/kitti_object.py).
    ``crop=(left, top)``: the scene was cropped by that many pixels; c_u and c_v move with it, nothing else does."""
    from .datasets.kitti_object import Calibration
    return Calibration(path_or_text, crop).packed()


def _lidar_shapes(shapes, n):
    shapes = tuple((int(h), int(w)) for h, w in (shapes.tolist() if hasattr(shapes, "tolist") else shapes))
    if n < 1 or len(shapes) != n or not all(h >= 0 and w >= 0 and h * w < 2 ** 31 for h, w in shapes):
        raise RuntimeError("pseudo_lidar: shapes must be n >= 1 pairs (H, W) with H, W >= 0, one per frame (%d); got %s" % (n, shapes))
    return shapes


def _lidar_offsets(form, shapes, offsets, src_len):
    """The first element of every frame of a packed depth / disp input (K32's cell offsets); default: one map after the other."""
    if form == "net":
        if offsets is not None:
            raise RuntimeError("pseudo_lidar: offsets belong to the packed depth / disp forms")
        return None
    if offsets is None:
        offsets = np.cumsum([0] + [h * w for h, w in shapes])
    offsets = tuple(int(v) for v in (offsets.tolist() if hasattr(offsets, "tolist") else offsets))
    if len(offsets) not in (len(shapes), len(shapes) + 1) or any(o < 0 or o + h * w > src_len for o, (h, w) in zip(offsets, shapes)):
        raise RuntimeError("pseudo_lidar: offsets must place every frame's H W values inside the %d values given; got %s for %s"
                           % (src_len, offsets, shapes))
    return offsets[:len(shapes)]


def _lidar_lin_axis(dst, src):
    """K25's lin_axis for every destination index of one axis: (s0, s1, f), f float32 (OpenCV's INTER_LINEAR coordinates)."""
    scale = float(src) / float(dst)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    return s, np.minimum(s + 1, src - 1), f


def lidar_net_depth_host(disp, H, W, quantise=False):
    """The net form's depth of one frame, float32 [H, W], from the sigmoid output [h, w]: disp_to_depth's scaling in fp32, the
    bilinear resize, 5.4 / disp, evaluate's clamp and with ``quantise`` the 16-bit PNG round trip -- every operation a rounded
    float32 one, in the kernel's order."""
    disp = np.asarray(disp, dtype=np.float32)
    h, w = disp.shape
    with np.errstate(all="ignore"):
        taps = np.float32(1.0 / 100.0) + np.float32(1.0 / 0.1 - 1.0 / 100.0) * disp
        sx, sx1, fx = _lidar_lin_axis(W, w)
        sy, sy1, fy = _lidar_lin_axis(H, h)
        a0, a1 = np.float32(1) - fx, fx
        b0, b1 = (np.float32(1) - fy)[:, None], fy[:, None]
        rows = a0 * taps[:, sx] + a1 * taps[:, sx1]
        small = b0 * rows[sy] + b1 * rows[sy1]
        depth = (np.float32(1) / small) * np.float32(5.4)
        depth = np.where(depth < np.float32(1e-3), np.float32(1e-3), depth)
        depth = np.where(depth > np.float32(80), np.float32(80), depth)
        if quantise:
            q = depth * np.float32(256)
            k = np.where(np.isnan(q), np.float32(0), q).astype(np.uint16)
            depth = k.astype(np.float32) / np.float32(256)
    return depth.astype(np.float32)


def _lidar_frame_host(cal, H, W, d, keep, max_high):
    """project_image_to_velo and the validity test on the candidates of one frame: ``d`` float64 [H W] in pixel order, ``keep`` the
    candidate mask (None: all).  Element-wise float64 in the kernel's association; never ``np.dot``."""
    p = np.arange(H * W, dtype=np.int64) if keep is None else np.nonzero(keep)[0]
    v, u = (p // max(W, 1)).astype(np.float64), (p % max(W, 1)).astype(np.float64)
    d = d[p]
    f_u, f_v, c_u, c_v, b_x, b_y = (float(c) for c in cal[:6])
    Ri, Cm = cal[6:15].reshape(3, 3), cal[15:27].reshape(3, 4)
    with np.errstate(all="ignore"):
        x = ((u - c_u) * d) / f_u + b_x
        y = ((v - c_v) * d) / f_v + b_y
        z = d
        r = [(Ri[i, 0] * x + Ri[i, 1] * y) + Ri[i, 2] * z for i in range(3)]
        o = [((Cm[i, 0] * r[0] + Cm[i, 1] * r[1]) + Cm[i, 2] * r[2]) + Cm[i, 3] for i in range(3)]
        valid = (o[0] >= 0) & (o[2] < max_high)                 # a NaN fails either comparison
        rows = np.stack([o[0][valid], o[1][valid], o[2][valid], np.ones(int(valid.sum()))], axis=1).astype(np.float32)
    return rows


def pseudo_lidar_host(src, form, shapes, calib, max_high=1, quantise=False, offsets=None):
    """K39 in numpy, the definition the kernel is held to (and the path CPU tensors take).  ``src``: float32, the packed maps of
    the depth / disp forms (frame f at ``offsets[f]``) or the network's output [n, h, w] of the net form.  ``calib``: float64
    [n, 27].  Returns (float32 [M, 4], int64 [n + 1]): the kept rows of all frames in batch order and pixel order, and where each
    frame's rows start."""
    if form not in LIDAR_FORMS:
        raise RuntimeError("pseudo_lidar: form must be one of %s; got %r" % (sorted(LIDAR_FORMS), form))
    src = np.asarray(src, dtype=np.float32)
    n = src.shape[0] if form == "net" else len(shapes)
    if form == "net" and src.ndim != 3:
        raise RuntimeError("pseudo_lidar: the net form takes [n, h, w]; got %s" % (src.shape,))
    if quantise and form != "net":
        raise RuntimeError("pseudo_lidar: quantise belongs to the net form")
    shapes = _lidar_shapes(shapes, n)
    calib = np.asarray(calib, dtype=np.float64).reshape(n, N.LIDAR_CALIB)
    starts = _lidar_offsets(form, shapes, offsets, src.size)
    flat = src.reshape(-1)
    max_high = float(max_high)
    clouds = []
    for f, (H, W) in enumerate(shapes):
        cal, keep = calib[f], None
        if H * W == 0:
            clouds.append(np.zeros((0, 4), dtype=np.float32))
            continue
        if form == "net":
            d = lidar_net_depth_host(src[f], H, W, quantise).reshape(-1).astype(np.float64)
        else:
            m = flat[starts[f]:starts[f] + H * W]
            if form == "depth":
                d = m.astype(np.float64)
            else:
                with np.errstate(all="ignore"):
                    s = np.where(m < 0, np.float32(0), m)       # a NaN stays and fails the mask
                    keep = s > 0
                    d = (cal[0] * LIDAR_BASELINE) / ((s.astype(np.float64) + 1.) - keep.astype(np.float64))
        clouds.append(_lidar_frame_host(cal, H, W, d, keep, max_high))
    counts = np.array([0] + [c.shape[0] for c in clouds], dtype=np.int64)
    return np.concatenate(clouds).reshape(-1, 4), np.cumsum(counts)


def _lidar_tables_device(device, form, shapes, starts):
    def make():
        tiles = [(h * w + N.LIDAR_TILE - 1) // N.LIDAR_TILE for h, w in shapes]
        first = np.cumsum([0] + tiles)
        desc = [[h, w, 0 if starts is None else starts[i], int(first[i])] for i, (h, w) in enumerate(shapes)]
        tile_frame = np.repeat(np.arange(len(shapes)), tiles)
        if tile_frame.size == 0:
            tile_frame = np.array([-1])                         # never read: a launch has n_tiles = 0
        return [torch.tensor(desc, dtype=torch.int32), torch.from_numpy(tile_frame.astype(np.int32))], int(first[-1])
    (desc, tile_frame), n_tiles = _lidar_desc_cache.get((str(device), form, shapes, starts), device, make)
    return desc, tile_frame, n_tiles


def pseudo_lidar(src, form, shapes, calib, max_high=1, quantise=False, offsets=None):
    """K39: maps of a batch of frames to velodyne-frame point clouds, as the reference's preprocessing/generate_lidar.py makes them
    on the host (``project_depth_to_points`` / ``project_disp_to_points`` over ``Calibration.project_image_to_velo``), float32-equal,
    in three launches with no host read.

    src      float32.  ``form`` "depth": metric depth maps packed flat, frame f's H W values at ``offsets[f]`` (K32's layout; default
             one map after the other); every pixel is a candidate.  "disp": the same layout of disparities in pixels; negatives
             count as 0 and only pixels with a positive disparity are candidates.  "net": the network's sigmoid output [n, h, w]
             (or [n, 1, h, w]); per frame it is scaled (disp_to_depth(., 0.1, 100)), resized to (H, W) as evaluate resizes it,
             turned into 5.4 / disp, clamped to [1e-3, 80], and with ``quantise`` rounded down to 1 / 256 as a 16-bit PNG stores it.
    shapes   n pairs (H, W): each frame's own size.  Host values: they size the launch.
    calib    float64 [n, 27] on src's device: ``lidar_calib`` of every frame.
    max_high a point is kept if its velodyne x >= 0 and z < max_high.
    Returns  PseudoLidarOut(points, offsets): float32 [sum H W, 4], the kept rows (x, y, z, 1) of all frames in batch order, each
             frame's in row-major pixel order, and int64 [n + 1] on the device: frame f is points[offsets[f]:offsets[f + 1]].
             Rows from offsets[n] on are unspecified.

    CPU tensors run ``pseudo_lidar_host``, the numpy restatement the kernel is bit-equal to."""
    if form not in LIDAR_FORMS:
        raise RuntimeError("pseudo_lidar: form must be one of %s; got %r" % (sorted(LIDAR_FORMS), form))
    if not torch.is_tensor(src) or src.dtype != torch.float32:
        raise RuntimeError("pseudo_lidar: src must be a float32 tensor; got %s" % (getattr(src, "dtype", type(src)),))
    if form == "net":
        if src.dim() == 4 and src.shape[1] == 1:
            src = src[:, 0]
        if src.dim() != 3 or src.shape[1] < 1 or src.shape[2] < 1:
            raise RuntimeError("pseudo_lidar: the net form takes [n, h, w] or [n, 1, h, w]; got %s" % (tuple(src.shape),))
        n, h, w = (int(v) for v in src.shape)
    else:
        if quantise:
            raise RuntimeError("pseudo_lidar: quantise belongs to the net form")
        if src.dim() != 1:
            raise RuntimeError("pseudo_lidar: the %s form takes the maps packed flat; got %s" % (form, tuple(src.shape)))
        n, h, w = len(shapes), 0, 0
    shapes = _lidar_shapes(shapes, n)
    if not torch.is_tensor(calib) or calib.dtype != torch.float64 or calib.numel() != N.LIDAR_CALIB * n:
        raise RuntimeError("pseudo_lidar: calib must be a float64 tensor of %d x %d entries; got %s %s"
                           % (n, N.LIDAR_CALIB, getattr(calib, "dtype", type(calib)), tuple(getattr(calib, "shape", ()))))
    dev = src.device
    if calib.device != dev:
        raise RuntimeError("pseudo_lidar: src and calib must share a device; got %s and %s" % (dev, calib.device))
    starts = _lidar_offsets(form, shapes, offsets, src.numel())
    cap = sum(hh * ww for hh, ww in shapes)
    if cap >= 2 ** 31 or src.numel() >= 2 ** 31:
        raise RuntimeError("pseudo_lidar: the batch must hold fewer than 2^31 pixels; got %d" % cap)
    if dev.type != "cuda":
        pts, off = pseudo_lidar_host(src.numpy(), form, shapes, calib.numpy(), max_high, quantise, starts)
        points = torch.zeros((cap, 4), dtype=torch.float32)
        points[:pts.shape[0]] = torch.from_numpy(pts)
        return PseudoLidarOut(points, torch.from_numpy(off))
    desc, tile_frame, n_tiles = _lidar_tables_device(dev, form, shapes, starts)
    src, calib = _c(src), _c(calib)
    ws = torch.empty(2 * max(n_tiles, 1), device=dev, dtype=torch.int32)
    points = torch.empty((cap, 4), device=dev, dtype=torch.float32)
    off = torch.empty(n + 1, device=dev, dtype=torch.int64)
    N.check(_timed("pseudo_lidar", lambda: N.lib().dmh_pseudo_lidar(
        N.ptr(src) if src.numel() else None, src.numel(), LIDAR_FORMS[form], h, w, int(bool(quantise)), N.ptr_f64(calib), N.ptr(desc),
        N.ptr(tile_frame), n, n_tiles, float(max_high), N.ptr(ws), N.ptr(points) if cap else None, cap, C.c_void_p(off.data_ptr()),
        N.stream()), 2 * 4 * src.numel() + 16 * cap))
    return PseudoLidarOut(points, off)


def lidar_clouds(out):
    """The clouds of a ``PseudoLidarOut`` on the host, one float32 [M_f, 4] array per frame: the n + 1 offsets are read first (they
    say how many rows are in use), then only those rows are copied."""
    off = out.offsets.cpu().numpy()
    used = out.points[:int(off[-1])].cpu().numpy()
    return [used[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
