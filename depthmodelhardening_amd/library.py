"""``torch.ops.dmh.*`` -- the hot-path kernels registered with ``torch.library`` on top of the unchanged C ABI.

SURVEY.md section 8b asks for "PyTorch-ROCm custom ops": operators the dispatcher knows, with a fake-tensor (meta)
implementation, so that they can be traced, exported and compiled (``torch.compile`` / ``torch.export`` see an opaque
``dmh::...`` call with known output shapes instead of a ctypes call they cannot look into) and an autograd formula that is
itself a registered op.  Each operator below is a schema, a fake implementation and an autograd formula around a launcher of
``ops.py`` (``ops.*_fwd_launch`` / ``ops.*_bwd_launch``, or the ``ops.*`` function itself): this module makes no call into
``libdmh_hip.so`` of its own, so the two surfaces cannot drift.  ``ops.py``'s ``torch.autograd.Function`` wrappers, around the
same launchers, remain the path the Trainer and the attacks use (they carry the per-attack caches and the fused multi-launch
nodes); tests/test_gpu_library.py holds the wrappers of both surfaces -- argument order, saved tensors, gradient slots -- to
the same bits.  There is no CPU kernel behind any of them: CPU tensors are rejected as ``ops.py`` rejects them.

    dmh::eot_paste            physicalTrans.py:156-165 + phy_obj_atk.py:88-90   (K3)   + dmh::eot_paste_bwd
    dmh::masked_sq_mean       phy_obj_atk.py:94, pgd_depth.py:68-70             (K6)   + dmh::masked_sq_mean_bwd
    dmh::gt_depth_mse         MD2/trainer.py:551-557 (--supervised_adv --gt_depth) (K6b)  + dmh::gt_depth_mse_bwd
    dmh::pgd_linf_step        phy_obj_atk.py:98-101, pgd_depth.py:76-78         (K4)
    dmh::apgd_step            phy_obj_atk_apgd.py:207-215                       (K22, in place)
    dmh::apgd_commit          phy_obj_atk_apgd.py:255-290                       (K22, in place)
    dmh::tube_light_compose   phy_obj_atk_light.py:130-138, light_simulation.py  (K24, writes ``out``)
    dmh::tube_light_commit    phy_obj_atk_light.py:165-167                      (K24, in place)
    dmh::gauss_blur_windows   phy_obj_atk_guassian.py:96-101 (scipy gaussian_filter + clip, all steps)   (K26)
    dmh::gauss_blur_compose   phy_obj_atk_guassian.py:103                       (K26, writes ``out``)
    dmh::square_propose       phy_obj_atk_square.py:259-260,284-291,312-313     (K27, in place)
    dmh::pgd_l2_step          phy_obj_atk_l2.py:110-120, shared-patch form      (K28)
    dmh::l0_fused_step        phy_obj_atk_l0.py:105-111,136-138,94-99           (K23, in place)
    dmh::eigen_gt_stats       MD2/evaluate_depth.py:360-373,377 (ground truth)  (K25)
    dmh::eigen_depth_errors   MD2/evaluate_depth.py:351-384, :102-110, :61-76   (K25)
    dmh::l0_compose           phy_obj_atk_l0.py:94-99,43-52                     (K5)   + dmh::l0_compose_bwd
    dmh::l0_mask_cost         phy_obj_atk_l0.py:130-132                         (K5)   + dmh::l0_mask_cost_bwd
    dmh::photo_smooth_loss    MD2/trainer.py:472-523,539-674 (DH/trainer.py:638-741 with variant 1)   (K1 + K2 + finalise)
                                                                                       + dmh::photo_smooth_loss_bwd
    dmh::ssim_map             MD2/layers.py:223-253 SSIM.forward                (K1's window sums, stand-alone)
    dmh::smooth_loss          MD2/layers.py:207-220 get_smooth_loss             (K2 on one scale)
    dmh::pose_head            MD2/networks/pose_decoder.py:47-52 + MD2/layers.py:28-103   (K29) + dmh::pose_head_bwd
    dmh::cost_volume          manydepth2/networks/resnet_encoder.py:157-236,258-265,294-296   (K30, forward only)
    dmh::cost_volume_into     the same, cost_volume * confidence written into channels 64 .. of ``buffer``   (K30, in place)
    dmh::cost_volume_stack    cat([features, cost_volume * confidence], 1) with gradient; no counterpart in the reference   (K30 + K38)
    dmh::pil_resample         MD2/datasets/mono_dataset.py:100-104,119-144 (PIL.Image.resize, 8-bit, bit for bit)   (K31, no autograd)
    dmh::velo_depth_map       MD2/kitti_utils.py:46-98 + datasets/kitti_dataset.py:70-85 (generate_depth_map, float32-equal) (K32, no autograd)
    dmh::color_jitter         MD2/datasets/mono_dataset.py:344-348,133,144 (torchvision 0.8.2 ColorJitter on 8-bit PIL images, Pillow's bytes) (K33, no autograd)
    dmh::depth_hint_fuse      depth-hints/precompute_depth_hints.py:151,247-252 (warp, SSIM + L1, argmin, gather per candidate) (K34, no autograd)
    dmh::reduce_conv_degenerate   manydepth2/networks/resnet_encoder.py:124-129,321 in the degenerate call of manydepth2/trainer.py:371-385
                              (reduce_conv over 64 features + D zero channels: conv3x3 with weight[:, :C], bias, ReLU)   (K36)
                                                                                       + dmh::reduce_conv_degenerate_bwd
    dmh::sgm_disparity        the stereo matchers of depth-hints/precompute_depth_hints.py:42-63,128-147 as this package's own integer
                              semi-global matcher (not OpenCV's output)   (K35, no autograd)
    dmh::disp_colorize        MD2/test_simple.py:136-156, my_utils.py:54-67 (bilinear resize, np.percentile, Normalize + magma, uint8)
                              (K37, no autograd)
    dmh::pseudo_lidar         preprocessing/generate_lidar.py:10-33 + kitti_util.py:159-175 (maps to velodyne-frame clouds, float32-equal)
                              (K39, no autograd)
    dmh::pose_ate             MD2/evaluate_pose.py:23-46,116-125 (dump_xyz, compute_ate, np.mean, np.std in float64)   (K40, no autograd)
    dmh::stem_pair_norm       MD2/evaluate_pose.py:94-96 + MD2/networks/resnet_encoder.py:89-90 (cat, normalise, the 6 -> 64 conv1)
                              (K41, forward only)
"""
from typing import List, Optional, Tuple

import torch
from torch.library import custom_op

from . import _native as N
from . import ops


def _cu(t):
    return t if t.is_contiguous() else t.contiguous()


def _cul(ts):
    return [_cu(t) for t in ts]


# ----------------------------------------------------------------------------------------------------------------- K3
@custom_op("dmh::eot_paste", mutates_args=())
def eot_paste(scene: torch.Tensor, patch: torch.Tensor, pmask: torch.Tensor, coeffs: torch.Tensor, l_pad: int, t_pad: int,
              oh: int, ow: int, flip: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.eot_paste_fwd_launch(_cu(scene), _cu(patch), _cu(pmask), _cu(coeffs), l_pad, t_pad, oh, ow, N.PASTE_COMPOSITE, flip)


@eot_paste.register_fake
def _(scene, patch, pmask, coeffs, l_pad, t_pad, oh, ow, flip=None):
    n = coeffs.shape[0]
    return scene.new_empty((n, 3, oh, ow)), scene.new_empty((n, 1, oh, ow))


@custom_op("dmh::eot_paste_bwd", mutates_args=())
def eot_paste_bwd(scene: torch.Tensor, patch: torch.Tensor, pmask: torch.Tensor, coeffs: torch.Tensor, l_pad: int, t_pad: int,
                  oh: int, ow: int, flip: Optional[torch.Tensor], g_adv: torch.Tensor) -> torch.Tensor:
    return ops.eot_paste_bwd_launch(_cu(scene), _cu(patch), _cu(pmask), _cu(coeffs), l_pad, t_pad, oh, ow, N.PASTE_COMPOSITE, flip,
                                    None, _cu(g_adv))


@eot_paste_bwd.register_fake
def _(scene, patch, pmask, coeffs, l_pad, t_pad, oh, ow, flip, g_adv):
    return torch.empty_like(patch)


def _paste_setup(ctx, inputs, output):
    scene, patch, pmask, coeffs, l_pad, t_pad, oh, ow, flip = inputs
    ctx.save_for_backward(scene, patch, pmask, coeffs, *([flip] if flip is not None else []))
    ctx.geo = (l_pad, t_pad, oh, ow, flip is not None)


def _paste_backward(ctx, g_adv, g_mask):
    sv = ctx.saved_tensors
    l_pad, t_pad, oh, ow, has_flip = ctx.geo
    g_patch = torch.ops.dmh.eot_paste_bwd(sv[0], sv[1], sv[2], sv[3], l_pad, t_pad, oh, ow, sv[4] if has_flip else None, g_adv)
    return None, g_patch, None, None, None, None, None, None, None


eot_paste.register_autograd(_paste_backward, setup_context=_paste_setup)


# ----------------------------------------------------------------------------------------------------------------- K6
@custom_op("dmh::masked_sq_mean", mutates_args=())
def masked_sq_mean(disp: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    return ops.masked_sq_mean_fwd_launch(_cu(disp), None if mask is None else _cu(mask))


@masked_sq_mean.register_fake
def _(disp, mask=None):
    return disp.new_empty(())


@custom_op("dmh::masked_sq_mean_bwd", mutates_args=())
def masked_sq_mean_bwd(disp: torch.Tensor, mask: Optional[torch.Tensor], g: torch.Tensor) -> torch.Tensor:
    return ops.masked_sq_mean_bwd_launch(_cu(disp), None if mask is None else _cu(mask), g)


@masked_sq_mean_bwd.register_fake
def _(disp, mask, g):
    return torch.empty_like(disp)


def _msm_setup(ctx, inputs, output):
    disp, mask = inputs
    ctx.save_for_backward(disp, *([mask] if mask is not None else []))
    ctx.has_mask = mask is not None


def _msm_backward(ctx, g):
    sv = ctx.saved_tensors
    return torch.ops.dmh.masked_sq_mean_bwd(sv[0], sv[1] if ctx.has_mask else None, g), None


masked_sq_mean.register_autograd(_msm_backward, setup_context=_msm_setup)


# ---------------------------------------------------------------------------------------------------------------- K6b
@custom_op("dmh::gt_depth_mse", mutates_args=())
def gt_depth_mse(disp: torch.Tensor, disp_gt: torch.Tensor, objmask: torch.Tensor, objdepth: torch.Tensor, min_depth: float,
                 max_depth: float) -> torch.Tensor:
    return ops.gt_depth_mse_fwd_launch(*ops._gt_depth_operands(disp, disp_gt, objmask, objdepth), min_depth, max_depth)


@gt_depth_mse.register_fake
def _(disp, disp_gt, objmask, objdepth, min_depth, max_depth):
    return disp.new_empty(())


@custom_op("dmh::gt_depth_mse_bwd", mutates_args=())
def gt_depth_mse_bwd(disp: torch.Tensor, disp_gt: torch.Tensor, objmask: torch.Tensor, objdepth: torch.Tensor, min_depth: float,
                     max_depth: float, g: torch.Tensor) -> torch.Tensor:
    return ops.gt_depth_mse_bwd_launch(*ops._gt_depth_operands(disp, disp_gt, objmask, objdepth), min_depth, max_depth, g)


@gt_depth_mse_bwd.register_fake
def _(disp, disp_gt, objmask, objdepth, min_depth, max_depth, g):
    return torch.empty_like(disp)


def _gtd_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], inputs[2], inputs[3])
    ctx.depths = (inputs[4], inputs[5])


def _gtd_backward(ctx, g):
    disp, disp_gt, objmask, objdepth = ctx.saved_tensors
    return torch.ops.dmh.gt_depth_mse_bwd(disp, disp_gt, objmask, objdepth, ctx.depths[0], ctx.depths[1], g), None, None, None, None, None


gt_depth_mse.register_autograd(_gtd_backward, setup_context=_gtd_setup)


# ----------------------------------------------------------------------------------------------------------------- K4
@custom_op("dmh::pgd_linf_step", mutates_args=())
def pgd_linf_step(x: torch.Tensor, x0: torch.Tensor, grad: torch.Tensor, alpha: float, eps: float) -> torch.Tensor:
    return ops.pgd_linf_step(x, x0, grad, alpha, eps)


@pgd_linf_step.register_fake
def _(x, x0, grad, alpha, eps):
    return torch.empty_like(x)


# ---------------------------------------------------------------------------------------------------------------- K28
@custom_op("dmh::pgd_l2_step", mutates_args=())
def pgd_l2_step(x: torch.Tensor, x0: torch.Tensor, grad: torch.Tensor, alpha: float, eps: float) -> torch.Tensor:
    return ops.pgd_l2_step(_cu(x), _cu(x0), _cu(grad), alpha, eps)


@pgd_l2_step.register_fake
def _(x, x0, grad, alpha, eps):
    return torch.empty_like(x)


# ---------------------------------------------------------------------------------------------------------------- K22
@custom_op("dmh::apgd_step", mutates_args=("x_adv", "x_old", "cursor"))
def apgd_step(x_adv: torch.Tensor, x_old: torch.Tensor, x0: torch.Tensor, grad: torch.Tensor, ctl: torch.Tensor,
              cursor: torch.Tensor, steps: int, eps: float) -> None:
    ops.apgd_step(x_adv, x_old, x0, grad, ctl, cursor, steps, eps)


@apgd_step.register_fake
def _(x_adv, x_old, x0, grad, ctl, cursor, steps, eps):
    return None


@custom_op("dmh::apgd_commit", mutates_args=("x_adv", "grad", "x_best", "grad_best", "x_ret", "ctl", "hist", "cursor"))
def apgd_commit(x_adv: torch.Tensor, g_new: torch.Tensor, grad: torch.Tensor, x_best: torch.Tensor, grad_best: torch.Tensor,
                x_ret: torch.Tensor, loss: torch.Tensor, ctl: torch.Tensor, hist: torch.Tensor, cursor: torch.Tensor,
                steps: int, size_decr: int, steps_min: int, rho: float) -> None:
    ops.apgd_commit(x_adv, g_new, grad, x_best, grad_best, x_ret, loss, ctl, hist, cursor, steps, size_decr, steps_min, rho)


@apgd_commit.register_fake
def _(x_adv, g_new, grad, x_best, grad_best, x_ret, loss, ctl, hist, cursor, steps, size_decr, steps_min, rho):
    return None


# ---------------------------------------------------------------------------------------------------------------- K23
@custom_op("dmh::l0_fused_step", mutates_args=("pos", "neg", "m_pos", "v_pos", "m_neg", "v_neg", "adv", "count", "rec", "cursor"))
def l0_fused_step(obj: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, m_pos: torch.Tensor, v_pos: torch.Tensor,
                  m_neg: torch.Tensor, v_neg: torch.Tensor, g_adv: torch.Tensor, adv: torch.Tensor, count: torch.Tensor,
                  rec: torch.Tensor, cursor: torch.Tensor, tab: torch.Tensor, adv_cost: torch.Tensor,
                  mask_cost: Optional[torch.Tensor], steps: int, mask_wt: float, thresh: float, l0_clip: float) -> None:
    ops.l0_fused_step(obj, pos, neg, m_pos, v_pos, m_neg, v_neg, g_adv, adv, count, rec, cursor, tab, adv_cost, mask_cost, steps,
                      mask_wt, thresh, l0_clip)


@l0_fused_step.register_fake
def _(obj, pos, neg, m_pos, v_pos, m_neg, v_neg, g_adv, adv, count, rec, cursor, tab, adv_cost, mask_cost, steps, mask_wt, thresh,
      l0_clip):
    return None


# ---------------------------------------------------------------------------------------------------------------- K24
@custom_op("dmh::tube_light_compose", mutates_args=("out",))
def tube_light_compose(table: torch.Tensor, index: torch.Tensor, base_u8: torch.Tensor, out: torch.Tensor) -> None:
    ops.tube_light_compose(table, index, base_u8, out)


@tube_light_compose.register_fake
def _(table, index, base_u8, out):
    return None


@custom_op("dmh::tube_light_commit", mutates_args=("cost", "best", "state"))
def tube_light_commit(cost_in: torch.Tensor, cost: torch.Tensor, best: torch.Tensor, state: torch.Tensor) -> None:
    ops.tube_light_commit(cost_in, cost, best, state)


@tube_light_commit.register_fake
def _(cost_in, cost, best, state):
    return None


# ---------------------------------------------------------------------------------------------------------------- K25
@custom_op("dmh::eigen_gt_stats", mutates_args=())
def eigen_gt_stats(gt: torch.Tensor, table: torch.Tensor, blk_img: torch.Tensor, first: int, n: int, b0: int, grid: int,
                   eigen: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.eigen_gt_stats(_cu(gt), _cu(table), _cu(blk_img), first, n, b0, grid, eigen)


@eigen_gt_stats.register_fake
def _(gt, table, blk_img, first, n, b0, grid, eigen):
    return gt.new_empty((n,)), table.new_empty((n,))


@custom_op("dmh::eigen_depth_errors", mutates_args=())
def eigen_depth_errors(pred_disp: torch.Tensor, pred_disp_flip: Optional[torch.Tensor], gt: torch.Tensor, table: torch.Tensor,
                       blk_img: torch.Tensor, med_gt: torch.Tensor, first: int, b0: int, grid: int, px0: int, npx: int,
                       eigen: bool, scale_factor: float,
                       median_scaling: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.eigen_depth_errors_launch(pred_disp, pred_disp_flip, _cu(gt), _cu(table), _cu(blk_img), _cu(med_gt), first, b0, grid,
                                         px0, npx, eigen, scale_factor, median_scaling)


@eigen_depth_errors.register_fake
def _(pred_disp, pred_disp_flip, gt, table, blk_img, med_gt, first, b0, grid, px0, npx, eigen, scale_factor, median_scaling):
    n = pred_disp.shape[0]
    return pred_disp.new_empty((n, 8)), pred_disp.new_empty((n,)), pred_disp.new_empty((npx,)), pred_disp.new_empty((n,))


# ---------------------------------------------------------------------------------------------------------------- K26
@custom_op("dmh::gauss_blur_windows", mutates_args=())
def gauss_blur_windows(obj: torch.Tensor, weights: torch.Tensor, radii: torch.Tensor, r0: int, r1: int, c0: int, c1: int) -> torch.Tensor:
    return ops.gauss_blur_windows(obj, weights, radii, (r0, r1, c0, c1))


@gauss_blur_windows.register_fake
def _(obj, weights, radii, r0, r1, c0, c1):
    H, W = obj.shape[-2], obj.shape[-1]
    (a, b, _), (c, d, _) = slice(r0, r1).indices(H), slice(c0, c1).indices(W)
    return obj.new_empty((weights.shape[0], obj.shape[-3], max(b - a, 0), max(d - c, 0)))


@custom_op("dmh::gauss_blur_compose", mutates_args=("out",))
def gauss_blur_compose(windows: torch.Tensor, index: torch.Tensor, obj: torch.Tensor, out: torch.Tensor, r0: int, r1: int, c0: int,
                       c1: int) -> None:
    ops.gauss_blur_compose(windows, index, obj, (r0, r1, c0, c1), out)


@gauss_blur_compose.register_fake
def _(windows, index, obj, out, r0, r1, c0, c1):
    return None


# ---------------------------------------------------------------------------------------------------------------- K27
@custom_op("dmh::square_propose", mutates_args=("x_best", "x_new"))
def square_propose(x0: torch.Tensor, x_best: torch.Tensor, x_new: torch.Tensor, table: torch.Tensor, stripes: torch.Tensor,
                   state: torch.Tensor, eps: float) -> None:
    ops.square_propose(x0, x_best, x_new, table, stripes, state, eps)


@square_propose.register_fake
def _(x0, x_best, x_new, table, stripes, state, eps):
    return None


# ----------------------------------------------------------------------------------------------------------------- K5
@custom_op("dmh::l0_compose", mutates_args=())
def l0_compose(obj: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, l0_clip: float, finalize: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.l0_compose_fwd_launch(_cu(obj), _cu(pos), _cu(neg), l0_clip, finalize)


@l0_compose.register_fake
def _(obj, pos, neg, l0_clip, finalize):
    return torch.empty_like(obj), obj.new_empty((1,), dtype=torch.int32)


@custom_op("dmh::l0_compose_bwd", mutates_args=())
def l0_compose_bwd(obj: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, g_adv: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.l0_compose_bwd_launch(_cu(obj), _cu(pos), _cu(neg), _cu(g_adv))


@l0_compose_bwd.register_fake
def _(obj, pos, neg, g_adv):
    return torch.empty_like(pos), torch.empty_like(neg)


def _l0c_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], inputs[2])


def _l0c_backward(ctx, g_adv, g_count):
    obj, pos, neg = ctx.saved_tensors
    g_pos, g_neg = torch.ops.dmh.l0_compose_bwd(obj, pos, neg, g_adv)
    return None, g_pos, g_neg, None, None


l0_compose.register_autograd(_l0c_backward, setup_context=_l0c_setup)


@custom_op("dmh::l0_mask_cost", mutates_args=())
def l0_mask_cost(pos: torch.Tensor, neg: torch.Tensor) -> torch.Tensor:
    return ops.l0_mask_cost_fwd_launch(_cu(pos), _cu(neg))


@l0_mask_cost.register_fake
def _(pos, neg):
    return pos.new_empty(())


@custom_op("dmh::l0_mask_cost_bwd", mutates_args=())
def l0_mask_cost_bwd(pos: torch.Tensor, neg: torch.Tensor, g: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.l0_mask_cost_bwd_launch(_cu(pos), _cu(neg), g)


@l0_mask_cost_bwd.register_fake
def _(pos, neg, g):
    return torch.empty_like(pos), torch.empty_like(neg)


def _l0m_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])


def _l0m_backward(ctx, g):
    pos, neg = ctx.saved_tensors
    return torch.ops.dmh.l0_mask_cost_bwd(pos, neg, g)


l0_mask_cost.register_autograd(_l0m_backward, setup_context=_l0m_setup)


# ------------------------------------------------------------------------------------------------------- K1 + K2 + finalise
def _loss_cfg(sources, disps, min_depth, max_depth, variant, automask, no_ssim, smooth_wt, noise_mode, seed, offset):
    return dict(F=len(sources), NS=len(disps), min_depth=float(min_depth), max_depth=float(max_depth),
                variant="dh" if variant == N.VARIANT_DH else "md2", automask=bool(automask), no_ssim=bool(no_ssim),
                smooth_wt=float(smooth_wt), want_to_opt=False, hints=False, noise_mode=int(noise_mode), seed=int(seed),
                offset=int(offset))


@custom_op("dmh::photo_smooth_loss", mutates_args=())
def photo_smooth_loss(target: torch.Tensor, sources: List[torch.Tensor], Ts: List[torch.Tensor], K: torch.Tensor,
                      inv_K: torch.Tensor, disps: List[torch.Tensor], colors: List[torch.Tensor], min_depth: float,
                      max_depth: float, variant: int, automask: bool, no_ssim: bool, smooth_wt: float, noise_mode: int,
                      seed: int, offset: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(fin [FIN_SIZE], packed selection bytes [B,H,W], smoothness statistics): fin[FIN_LOSS] = losses["loss"],
    fin[FIN_LOSS_S + s] = losses["loss/s"] (include/dmh_hip.h).  noise_mode: 0 none, 2 in-kernel Philox (seed, offset)."""
    if noise_mode not in (N.NOISE_NONE, N.NOISE_PHILOX):
        raise RuntimeError("dmh::photo_smooth_loss: noise_mode must be 0 (none) or 2 (Philox)")
    cfg = _loss_cfg(sources, disps, min_depth, max_depth, variant, automask, no_ssim, smooth_wt, noise_mode, seed, offset)
    return ops.photo_smooth_fwd_launch(cfg, _cu(target), _cul(sources), _cul(Ts), _cu(K), _cu(inv_K), _cul(disps), _cul(colors))[:3]


@photo_smooth_loss.register_fake
def _(target, sources, Ts, K, inv_K, disps, colors, min_depth, max_depth, variant, automask, no_ssim, smooth_wt, noise_mode,
      seed, offset):
    B, _, H, W = target.shape
    return (target.new_empty((N.FIN_SIZE,)), target.new_empty((B, H, W), dtype=torch.uint8),
            target.new_empty((len(disps), B, 2)))


@custom_op("dmh::photo_smooth_loss_bwd", mutates_args=())
def photo_smooth_loss_bwd(target: torch.Tensor, sources: List[torch.Tensor], Ts: List[torch.Tensor], K: torch.Tensor,
                          inv_K: torch.Tensor, disps: List[torch.Tensor], colors: List[torch.Tensor], min_depth: float,
                          max_depth: float, variant: int, automask: bool, no_ssim: bool, smooth_wt: float, fin: torch.Tensor,
                          sel: torch.Tensor, sstats: torch.Tensor, g_fin: torch.Tensor) -> List[torch.Tensor]:
    cfg = _loss_cfg(sources, disps, min_depth, max_depth, variant, automask, no_ssim, smooth_wt, N.NOISE_NONE, 0, 0)
    return ops.photo_smooth_bwd_launch(cfg, _cu(target), _cul(sources), _cul(Ts), _cu(K), _cu(inv_K), _cul(disps), _cul(colors), None,
                                       _cu(fin), _cu(sel), _cu(sstats), g_fin, [False] * len(sources))[0]


@photo_smooth_loss_bwd.register_fake
def _(target, sources, Ts, K, inv_K, disps, colors, min_depth, max_depth, variant, automask, no_ssim, smooth_wt, fin, sel, sstats,
      g_fin):
    return [torch.empty_like(d) for d in disps]


def _psl_setup(ctx, inputs, output):
    (target, sources, Ts, K, inv_K, disps, colors, min_depth, max_depth, variant, automask, no_ssim, smooth_wt, _nm, _seed,
     _off) = inputs
    fin, sel, sstats = output
    ctx.nf, ctx.ns = len(sources), len(disps)
    ctx.save_for_backward(target, K, inv_K, fin, sel, sstats, *sources, *Ts, *disps, *colors)
    ctx.scalars = (min_depth, max_depth, variant, automask, no_ssim, smooth_wt)


def _psl_backward(ctx, g_fin, g_sel, g_sstats):
    sv = ctx.saved_tensors
    target, K, inv_K, fin, sel, sstats = sv[:6]
    nf, ns = ctx.nf, ctx.ns
    sources, Ts = list(sv[6:6 + nf]), list(sv[6 + nf:6 + 2 * nf])
    disps, colors = list(sv[6 + 2 * nf:6 + 2 * nf + ns]), list(sv[6 + 2 * nf + ns:6 + 2 * nf + 2 * ns])
    g_disp = torch.ops.dmh.photo_smooth_loss_bwd(target, sources, Ts, K, inv_K, disps, colors, *ctx.scalars, fin, sel, sstats,
                                                 g_fin)
    # one entry per input, list inputs as lists of the same length
    return (None, [None] * nf, [None] * nf, None, None, list(g_disp), [None] * ns) + (None,) * 9


photo_smooth_loss.register_autograd(_psl_backward, setup_context=_psl_setup)


# ------------------------------------------------------------------------- the stand-alone layers surface (MD2/layers.py)
@custom_op("dmh::ssim_map", mutates_args=())
def ssim_map(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """clamp((1 - SSIM(x, y)) / 2, 0, 1) per channel with 3x3 reflection-padded means: MD2/layers.py:223-253."""
    return ops.ssim_map_fwd_launch(_cu(x), _cu(y))


@ssim_map.register_fake
def _(x, y):
    return torch.empty_like(x)


@custom_op("dmh::ssim_map_bwd", mutates_args=())
def ssim_map_bwd(x: torch.Tensor, y: torch.Tensor, g_out: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.ssim_map_bwd_launch(_cu(x), _cu(y), _cu(g_out))


@ssim_map_bwd.register_fake
def _(x, y, g_out):
    return torch.empty_like(x), torch.empty_like(y)


def _ssim_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])


def _ssim_backward(ctx, g):
    x, y = ctx.saved_tensors
    g_x, g_y = torch.ops.dmh.ssim_map_bwd(x, y, g)
    return g_x, g_y


ssim_map.register_autograd(_ssim_backward, setup_context=_ssim_setup)


@custom_op("dmh::smooth_loss", mutates_args=())
def smooth_loss(disp: torch.Tensor, img: torch.Tensor) -> torch.Tensor:
    """mean(|d_x disp| exp(-mean_c |d_x img|)) + mean(|d_y disp| exp(-mean_c |d_y img|)): MD2/layers.py:207-220 on the
    disparity as given (the caller applies the mean normalisation of MD2/trainer.py:662-664)."""
    return ops.edge_smooth_fwd_launch(_cu(disp), _cu(img))


@smooth_loss.register_fake
def _(disp, img):
    return disp.new_empty(())


@custom_op("dmh::smooth_loss_bwd", mutates_args=())
def smooth_loss_bwd(disp: torch.Tensor, img: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    return ops.edge_smooth_bwd_launch(_cu(disp), _cu(img), g)


@smooth_loss_bwd.register_fake
def _(disp, img, g):
    return torch.empty_like(disp)


def _smooth_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])


def _smooth_backward(ctx, g):
    disp, img = ctx.saved_tensors
    return torch.ops.dmh.smooth_loss_bwd(disp, img, g), None      # the image is data: no gradient flows to it here


smooth_loss.register_autograd(_smooth_backward, setup_context=_smooth_setup)


# ----------------------------------------------------------------------------------------------------------------- K29
@custom_op("dmh::pose_head", mutates_args=())
def pose_head(x: torch.Tensor, invert_mask: int, scale: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.pose_head_fwd_launch(_cu(x), invert_mask, scale)


@pose_head.register_fake
def _(x, invert_mask, scale):
    B, nf = x.shape[0], x.shape[1] // 6
    return x.new_empty((B, nf, 1, 3)), x.new_empty((B, nf, 1, 3)), x.new_empty((B, nf, 4, 4))


@custom_op("dmh::pose_head_bwd", mutates_args=())
def pose_head_bwd(g_T: Optional[torch.Tensor], g_axisangle: Optional[torch.Tensor], g_translation: Optional[torch.Tensor],
                  axisangle: torch.Tensor, translation: torch.Tensor, shape: List[int], invert_mask: int,
                  scale: float) -> torch.Tensor:
    return ops.pose_head_bwd_launch(g_T, g_axisangle, g_translation, _cu(axisangle), _cu(translation), shape, invert_mask, scale)


@pose_head_bwd.register_fake
def _(g_T, g_axisangle, g_translation, axisangle, translation, shape, invert_mask, scale):
    return axisangle.new_empty(shape)


def _pose_setup(ctx, inputs, output):
    x, invert_mask, scale = inputs
    ctx.save_for_backward(output[0], output[1])
    ctx.cfg = (list(x.shape), invert_mask, scale)


def _pose_backward(ctx, g_aa, g_tr, g_T):
    aa, tr = ctx.saved_tensors
    shape, invert_mask, scale = ctx.cfg
    return torch.ops.dmh.pose_head_bwd(g_T, g_aa, g_tr, aa, tr, shape, invert_mask, scale), None, None


pose_head.register_autograd(_pose_backward, setup_context=_pose_setup)


# ----------------------------------------------------------------------------------------------------------------- K30
# No autograd formula: the reference computes the volume under torch.no_grad(); the outputs carry no gradient.
@custom_op("dmh::cost_volume", mutates_args=())
def cost_volume(current_feats: torch.Tensor, lookup_feats: torch.Tensor, poses: torch.Tensor, K: torch.Tensor, invK: torch.Tensor,
                depth_bins: torch.Tensor, set_missing_to_max: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.cost_volume(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max)


@cost_volume.register_fake
def _(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max=True):
    B, _, H, W = current_feats.shape
    D = depth_bins.shape[0]
    return (current_feats.new_empty((B, D, H, W)), current_feats.new_empty((B, D, H, W)), current_feats.new_empty((B, H, W)),
            current_feats.new_empty((B, H, W), dtype=torch.int32))


@custom_op("dmh::cost_volume_into", mutates_args=("buffer",))
def cost_volume_into(current_feats: torch.Tensor, lookup_feats: torch.Tensor, poses: torch.Tensor, K: torch.Tensor,
                     invK: torch.Tensor, depth_bins: torch.Tensor, buffer: torch.Tensor,
                     set_missing_to_max: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.cost_volume(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max, into=buffer)[2:]


@cost_volume_into.register_fake
def _(current_feats, lookup_feats, poses, K, invK, depth_bins, buffer, set_missing_to_max=True):
    B, _, H, W = current_feats.shape
    return current_feats.new_empty((B, H, W)), current_feats.new_empty((B, H, W), dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------- K38
@custom_op("dmh::cost_volume_stack", mutates_args=())
def cost_volume_stack(current_feats: torch.Tensor, lookup_feats: torch.Tensor, poses: torch.Tensor, K: torch.Tensor, invK: torch.Tensor,
                      depth_bins: torch.Tensor, set_missing_to_max: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(stacked [B, 64 + D, H, W], confidence, argmin); differentiable w.r.t. the two feature tensors through ``stacked`` (K38)."""
    for t in (current_feats, lookup_feats, poses, K, invK, depth_bins):
        ops._need_cuda(t)
    return ops.cost_volume_stack_fwd_launch(_cu(current_feats), _cu(lookup_feats), poses, K, invK, depth_bins, set_missing_to_max)


@cost_volume_stack.register_fake
def _(current_feats, lookup_feats, poses, K, invK, depth_bins, set_missing_to_max=True):
    B, Cc, H, W = current_feats.shape
    return (current_feats.new_empty((B, Cc + depth_bins.shape[0], H, W)), current_feats.new_empty((B, H, W)),
            current_feats.new_empty((B, H, W), dtype=torch.int32))


@custom_op("dmh::cost_volume_stack_bwd", mutates_args=())
def cost_volume_stack_bwd(g: torch.Tensor, current_feats: torch.Tensor, lookup_feats: torch.Tensor, poses: torch.Tensor,
                          K: torch.Tensor, invK: torch.Tensor, depth_bins: torch.Tensor, need_current: bool,
                          need_lookup: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d current_feats, d lookup_feats) for the gradient ``g`` of ``stacked``; the one that is not needed is an empty tensor (and
    is not computed)."""
    Cc = current_feats.shape[1]
    g = _cu(g)
    d_cur, d_look = ops.cost_volume_bwd_launch(current_feats, lookup_feats, poses, K, invK, depth_bins, g[:, Cc:], need_current,
                                               need_lookup)
    if d_cur is not None:
        d_cur += g[:, :Cc]
    return (d_cur if need_current else g.new_empty(0)), (d_look if need_lookup else g.new_empty(0))


@cost_volume_stack_bwd.register_fake
def _(g, current_feats, lookup_feats, poses, K, invK, depth_bins, need_current, need_lookup):
    return (torch.empty_like(current_feats) if need_current else g.new_empty(0),
            torch.empty_like(lookup_feats) if need_lookup else g.new_empty(0))


def _cvs_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:6])


def _cvs_backward(ctx, g, _g_conf, _g_idx):
    need_cur, need_look = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if not (need_cur or need_look):
        return (None,) * 7
    d_cur, d_look = torch.ops.dmh.cost_volume_stack_bwd(g, *ctx.saved_tensors, need_cur, need_look)
    return (d_cur if need_cur else None), (d_look if need_look else None), None, None, None, None, None


cost_volume_stack.register_autograd(_cvs_backward, setup_context=_cvs_setup)


# ---------------------------------------------------------------------------------------------------------------- K36
@custom_op("dmh::reduce_conv_degenerate", mutates_args=())
def reduce_conv_degenerate(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    ops._reduce_operands(x, weight, bias)       # the checks of ops.reduce_conv_degenerate; the launches below are its launches too
    return ops.reduce_conv_fwd_launch(_cu(x), weight, bias)


@reduce_conv_degenerate.register_fake
def _(x, weight, bias):
    return x.new_empty((x.shape[0], weight.shape[0], x.shape[2], x.shape[3]))


@custom_op("dmh::reduce_conv_degenerate_bwd", mutates_args=())
def reduce_conv_degenerate_bwd(g: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, y: torch.Tensor,
                               need_params: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(g_x, g_weight, g_bias); without ``need_params`` the last two are empty tensors (no launch made for them)."""
    g_x, g_w, g_b = ops.reduce_conv_bwd_launch(_cu(g), _cu(x), weight, _cu(y), True, need_params)
    return g_x, (g_w if need_params else g.new_empty(0)), (g_b if need_params else g.new_empty(0))


@reduce_conv_degenerate_bwd.register_fake
def _(g, x, weight, y, need_params):
    if need_params:
        return torch.empty_like(x), weight.new_empty(weight.shape), weight.new_empty((weight.shape[0],))
    return torch.empty_like(x), g.new_empty(0), g.new_empty(0)


def _reduce_setup(ctx, inputs, output):
    x, weight, bias = inputs
    ctx.save_for_backward(x, weight, output)
    ctx.need_params = not ops.weights_frozen()      # as ops.conv3x3: parameters are constants of an attack


def _reduce_backward(ctx, g):
    x, weight, y = ctx.saved_tensors
    need_params = ctx.need_params and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
    g_x, g_w, g_b = torch.ops.dmh.reduce_conv_degenerate_bwd(g, x, weight, y, need_params)
    return g_x, (g_w if need_params and ctx.needs_input_grad[1] else None), (g_b if need_params and ctx.needs_input_grad[2] else None)


reduce_conv_degenerate.register_autograd(_reduce_backward, setup_context=_reduce_setup)


# ---------------------------------------------------------------------------------------------------------------- K31
@custom_op("dmh::pil_resample", mutates_args=())
def pil_resample(src: torch.Tensor, out_h: int, out_w: int, filter: str = "lanczos", flip: Optional[torch.Tensor] = None,
                 sizes: Optional[List[int]] = None, hwc: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(uint8 [N, C, out_h, out_w], the same as float32 / 255).  ``sizes``: h0, w0, h1, w1, ... of the images in their slots;
    ``hwc``: a uint8 source is [N, H, W, C].  Images carry no gradient: there is no autograd formula."""
    pairs = None if sizes is None else list(zip(sizes[0::2], sizes[1::2]))
    ops._need_cuda(src)
    return tuple(ops.pil_resize(src, (out_h, out_w), filter, flip, pairs, True, "hwc" if hwc else "chw"))


@pil_resample.register_fake
def _(src, out_h, out_w, filter="lanczos", flip=None, sizes=None, hwc=False):
    shape = (src.shape[0], src.shape[3] if hwc else src.shape[1], out_h, out_w)
    return src.new_empty(shape, dtype=torch.uint8), src.new_empty(shape, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------- K32
@custom_op("dmh::velo_depth_map", mutates_args=())
def velo_depth_map(points: torch.Tensor, offsets: torch.Tensor, proj: torch.Tensor, shapes: List[int], vel_depth: bool = False,
                   out_size: Optional[List[int]] = None, flip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``shapes``: H0, W0, H1, W1, ... of the frames.  With ``out_size`` float32 [n, out_h, out_w]; without it the maps at their own
    sizes in one flat float32 buffer, frame f at sum(H W of the frames before it).  Ground truth carries no gradient."""
    ops._need_cuda(points)
    out = ops.velo_depth_map(points, offsets, proj, list(zip(shapes[0::2], shapes[1::2])), vel_depth, out_size, flip)
    return out if out_size is not None else out[0]


@velo_depth_map.register_fake
def _(points, offsets, proj, shapes, vel_depth=False, out_size=None, flip=None):
    if out_size is not None:
        return points.new_empty((offsets.shape[0] - 1, out_size[0], out_size[1]))
    return points.new_empty((sum(h * w for h, w in zip(shapes[0::2], shapes[1::2])),))


# ---------------------------------------------------------------------------------------------------------------- K33
@custom_op("dmh::color_jitter", mutates_args=())
def color_jitter(images: List[torch.Tensor], record: torch.Tensor, want_u8: bool = False) -> List[torch.Tensor]:
    """``images``: up to 8 uint8 [B, 3, H, W]; ``record``: int32 [B, 8] on their device (color_jitter.pil_records).  Returns the
    float32 results (byte / 255), one per tensor, followed with ``want_u8`` by the uint8 results.  Images carry no gradient."""
    for t in images:
        ops._need_cuda(t)
    res = ops.pil_color_jitter(images, record, want_u8)
    return [r.f32 for r in res] + ([r.u8 for r in res] if want_u8 else [])


@color_jitter.register_fake
def _(images, record, want_u8=False):
    return [t.new_empty(t.shape, dtype=torch.float32) for t in images] + ([t.new_empty(t.shape) for t in images] if want_u8 else [])


# ---------------------------------------------------------------------------------------------------------------- K34
@custom_op("dmh::depth_hint_fuse", mutates_args=())
def depth_hint_fuse(base: torch.Tensor, lookup: torch.Tensor, cand: torch.Tensor, K: torch.Tensor, inv_K: torch.Tensor, T: torch.Tensor,
                    want_losses: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(best_depth float32 [B, 1, H, W], losses float32 [B, N, H, W]; an empty tensor without ``want_losses``).  ``cand``: int16
    [B, N, H, W] (disparity x 16) or float32 depths.  Hints are data: there is no autograd formula."""
    ops._need_cuda(base)
    out = ops.depth_hint_fuse(base, lookup, cand, K, inv_K, T, want_losses)
    return (out[0], out[1]) if want_losses else (out, out.new_empty((0,)))


@depth_hint_fuse.register_fake
def _(base, lookup, cand, K, inv_K, T, want_losses=False):
    B, _, H, W = base.shape
    return (base.new_empty((B, 1, H, W), dtype=torch.float32),
            base.new_empty((B, cand.shape[1], H, W) if want_losses else (0,), dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------- K35
@custom_op("dmh::sgm_disparity", mutates_args=())
def sgm_disparity(base: torch.Tensor, lookup: torch.Tensor, params: List[int], reverse: Optional[torch.Tensor] = None,
                  workspace_cap: int = ops.SGM_WORKSPACE_CAP) -> torch.Tensor:
    """int16 [B, N, H, W], disparity x 16, -16 = no match.  ``params``: the N parameter sets flattened, ten integers each in the order
    of ``ops._SGM_KEYS`` (``sgm_params_flat`` makes them from the dicts).  Disparities are data: there is no autograd formula."""
    ops._need_cuda(base)
    return ops.sgm_disparity(base, lookup, sgm_params_unflat(params), reverse, workspace_cap)


@sgm_disparity.register_fake
def _(base, lookup, params, reverse=None, workspace_cap=ops.SGM_WORKSPACE_CAP):
    B, _, H, W = base.shape
    return base.new_empty((B, len(params) // len(ops._SGM_KEYS), H, W), dtype=torch.int16)


# ---------------------------------------------------------------------------------------------------------------- K37
@custom_op("dmh::disp_colorize", mutates_args=())
def disp_colorize(maps: torch.Tensor, panels: List[int], out_h: int, out_w: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(uint8 [P, out_h, out_w, 3], the coloured float maps [P, out_h, out_w], float32 [P, 5] statistics).  ``panels``: a, b, mode
    number, ref of every panel, flattened (``ops.COLORIZE_MODES``).  Figures carry no gradient: there is no autograd formula."""
    ops._need_cuda(maps)
    if len(panels) == 0 or len(panels) % 4 != 0:
        raise RuntimeError("disp_colorize: panels must hold four integers per panel; got %d" % len(panels))
    out = ops.disp_colorize(maps, [tuple(panels[i:i + 4]) for i in range(0, len(panels), 4)], (out_h, out_w), return_map=True)
    return out.rgb, out.map, out.stats


@disp_colorize.register_fake
def _(maps, panels, out_h, out_w):
    P = len(panels) // 4
    return (maps.new_empty((P, out_h, out_w, 3), dtype=torch.uint8), maps.new_empty((P, out_h, out_w)),
            maps.new_empty((P, ops.N.COLORIZE_STATS)))


# ---------------------------------------------------------------------------------------------------------------- K39
@custom_op("dmh::pseudo_lidar", mutates_args=())
def pseudo_lidar(src: torch.Tensor, form: str, shapes: List[int], calib: torch.Tensor, max_high: float = 1.0, quantise: bool = False,
                 offsets: Optional[List[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(points float32 [sum H W, 4], offsets int64 [n + 1]).  ``shapes``: H0, W0, H1, W1, ... of the frames; ``form``: "depth", "disp"
    or "net" (``ops.pseudo_lidar``).  Clouds carry no gradient: there is no autograd formula."""
    ops._need_cuda(src)
    out = ops.pseudo_lidar(src, form, list(zip(shapes[0::2], shapes[1::2])), calib, max_high, quantise, offsets)
    return out.points, out.offsets


@pseudo_lidar.register_fake
def _(src, form, shapes, calib, max_high=1.0, quantise=False, offsets=None):
    return (src.new_empty((sum(h * w for h, w in zip(shapes[0::2], shapes[1::2])), 4)),
            src.new_empty((len(shapes) // 2 + 1,), dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------- K40
@custom_op("dmh::pose_ate", mutates_args=())
def pose_ate(pred_poses: torch.Tensor, gt_local: torch.Tensor, track_length: int = 5) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ates float64 [N], stats float64 [2] = mean, np.std) of MD2/evaluate_pose.py:116-125 (``ops.pose_ate``).  Errors carry no
    gradient: there is no autograd formula."""
    ops._need_cuda(pred_poses)
    return ops.pose_ate_launch(pred_poses, gt_local, track_length)


@pose_ate.register_fake
def _(pred_poses, gt_local, track_length=5):
    return gt_local.new_empty((pred_poses.shape[0],)), gt_local.new_empty((2,))


# ---------------------------------------------------------------------------------------------------------------- K41
@custom_op("dmh::stem_pair_norm", mutates_args=())
def stem_pair_norm(a: torch.Tensor, b: torch.Tensor, weight: torch.Tensor, mean: float = 0.45, std: float = 0.225) -> torch.Tensor:
    """conv1((cat([a, b], 1) - mean) / std) of the pose encoder (``ops.stem_pair_norm``).  Forward only: there is no autograd
    formula, and a backward through it raises."""
    return ops.stem_pair_norm(a, b, weight, mean, std)


@stem_pair_norm.register_fake
def _(a, b, weight, mean=0.45, std=0.225):
    return a.new_empty((a.shape[0], 64, a.shape[2] // 2, a.shape[3] // 2))


def sgm_params_flat(params):
    """A list of parameter dicts as the flat integer list ``torch.ops.dmh.sgm_disparity`` takes."""
    return [int(v) for t in ops._sgm_params(params) for v in t]


def sgm_params_unflat(flat):
    k = len(ops._SGM_KEYS)
    if len(flat) == 0 or len(flat) % k != 0:
        raise RuntimeError("sgm_disparity: params must hold %d integers per parameter set; got %d" % (k, len(flat)))
    return [dict(zip(ops._SGM_KEYS, flat[i:i + k])) for i in range(0, len(flat), k)]


OPS = ("eot_paste", "eot_paste_bwd", "masked_sq_mean", "masked_sq_mean_bwd", "gt_depth_mse", "gt_depth_mse_bwd", "pgd_linf_step", "l0_compose", "l0_compose_bwd",
       "l0_mask_cost", "l0_mask_cost_bwd", "photo_smooth_loss", "photo_smooth_loss_bwd", "ssim_map", "ssim_map_bwd", "smooth_loss", "smooth_loss_bwd",
       "apgd_step", "apgd_commit", "l0_fused_step", "tube_light_compose", "tube_light_commit",
       "gauss_blur_windows", "gauss_blur_compose", "square_propose", "pgd_l2_step", "eigen_gt_stats", "eigen_depth_errors", "pose_head", "pose_head_bwd",
       "cost_volume", "cost_volume_into", "cost_volume_stack", "cost_volume_stack_bwd", "pil_resample", "velo_depth_map", "color_jitter", "depth_hint_fuse", "sgm_disparity",
       "reduce_conv_degenerate", "reduce_conv_degenerate_bwd", "disp_colorize", "pseudo_lidar", "pose_ate",
       "stem_pair_norm")
