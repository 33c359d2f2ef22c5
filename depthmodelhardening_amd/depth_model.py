"""The callable the attacks differentiate through (reference ``depth_model.py:10-20,89-161``)."""
import os

import numpy as np
import torch
import torch.nn

from . import networks


class DepthModelWrapper(torch.nn.Module):
    """encoder -> decoder -> outputs[("disp", 0)]."""

    def __init__(self, encoder, decoder) -> None:
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder

    def forward(self, input_image):
        feats = self.encoder(input_image)
        if feats[-1].is_cuda and hasattr(self.decoder, "_forward_fused"):
            return self.decoder(feats, only_scales=(0,))[("disp", 0)]     # the heads nobody reads are not computed
        return self.decoder(feats)[("disp", 0)]


    def masked_sq_mean(self, input_image, mask, plan=None, tab=None, clean=None, negate=False):
        """mean((disp_0(input_image) * mask)^2): the cost every object attack maximises (phy_obj_atk.py:92-94,
        phy_obj_atk_l0.py:125-127).  With a window plan (roi.RoiPlan + its device table) around the pasted object, and a
        decoder that supports it, the decoder below its first stage and the encoder head's backward run on the windows only;
        with ``clean`` (the same frames without the object: input_image equals it outside the plan's boxes) the encoder
        head's forward does too.  ``negate``: returns -mean(.), what the L_inf attack differentiates (phy_obj_atk.py:95)."""
        from . import ops
        # the decoder's static capability is asked BEFORE the encoder may hand back window-shaped features
        roi_dec = plan is not None and hasattr(self.decoder, "roi_ok") and self.decoder.roi_static_ok(plan)
        if plan is not None:        # what THIS call's encoder does with the plan (a plan may be used for more than one call)
            plan.head_windowed = plan.f0_compact = False
            tab = plan.device_table(input_image.device, tab)    # the plan's own table; one of another plan raises
        if roi_dec and getattr(self.encoder, "roi_backward", False):
            feats = self.encoder(input_image, roi=(plan, tab), clean=clean)
        else:
            feats = self.encoder(input_image)
        if roi_dec and self.decoder.roi_ok(feats, plan):
            return self.decoder.masked_sq_mean(feats, mask, plan, tab, negate=negate)
        if plan is not None and (plan.head_windowed or plan.f0_compact):
            # the decoder turned the plan down on the features' sizes after all: the whole-frame path serves the call
            plan.head_windowed = plan.f0_compact = False
            feats = self.encoder(input_image)
        if feats[-1].is_cuda and hasattr(self.decoder, "_forward_fused"):
            disp = self.decoder(feats, only_scales=(0,))[("disp", 0)]
        else:
            disp = self.decoder(feats)[("disp", 0)]
        cost = ops.masked_sq_mean(disp, mask)
        return -cost if negate else cost


# KITTI's normalised intrinsics, the values of the reference's manydepth2/assets/test_sequence_intrinsics.json
MANYDEPTH_INTRINSICS = ((0.58, 0.0, 0.5), (0.0, 1.92, 0.5), (0.0, 0.0, 1.0))
MANYDEPTH_DISP_SCALE = 8.6437


def manydepth_intrinsics(width, height):
    """(K, invK), both [1,4,4]: the normalised intrinsics scaled to the 1/4-size matching grid, and their pseudo-inverse
    (depth_model.py:60-75 load_and_preprocess_intrinsics)."""
    K = np.eye(4)
    K[:3, :3] = np.array(MANYDEPTH_INTRINSICS)
    K[0, :] *= width // 4
    K[1, :] *= height // 4
    return torch.Tensor(K).unsqueeze(0), torch.Tensor(np.linalg.pinv(K)).unsqueeze(0)


class ManyDepthModelWrapper(DepthModelWrapper):
    """ManyDepth as the attacks see it (depth_model.py:22-58): a single frame in, ``disp_0 / 8.6437`` out.  The reference hands
    the encoder ``input_image * 0`` as the lookup frame and a [1,1,4,4] zero pose, which makes every lookup "missing"; here the
    wrapper states that there are no lookups (``lookup_images=None``), so neither lookup features nor a cost volume are computed.
    ``encoder_dict``: the loaded ``encoder.pth`` (its ``width`` / ``height`` / ``min_depth_bin`` / ``max_depth_bin``)."""

    def __init__(self, encoder, decoder, encoder_dict=None):
        super().__init__(encoder, decoder)
        d = encoder_dict or {}
        self.width, self.height = int(d.get("width", 1024)), int(d.get("height", 320))
        self.min_depth_bin, self.max_depth_bin = float(d.get("min_depth_bin", 0.1)), float(d.get("max_depth_bin", 20.0))
        K, invK = manydepth_intrinsics(self.width, self.height)
        self.register_buffer("K", K, persistent=False)
        self.register_buffer("invK", invK, persistent=False)
        self.register_buffer("zero_pose", torch.zeros([1, 1, 4, 4]), persistent=False)

    def forward(self, input_image, lookup_images=None, poses=None):
        """One argument: the single-frame call above.  With ``lookup_images`` [B,L,3,H,W] and ``poses`` [Bp,L,4,4] (current camera
        -> lookup camera, translation in the network's units) the encoder's multi-frame form runs; whether a gradient flows through
        the matching volume is the encoder's ``matching_grad``."""
        bs = input_image.shape[0]
        if lookup_images is not None and poses is None:
            raise RuntimeError("ManyDepthModelWrapper: lookup_images need poses [Bp,L,4,4]")
        feats, _, _ = self.encoder(input_image, lookup_images, self.zero_pose if lookup_images is None else poses,
                                   self.K.expand(bs, 4, 4), self.invK.expand(bs, 4, 4), self.min_depth_bin, self.max_depth_bin)
        if feats[-1].is_cuda and hasattr(self.decoder, "_forward_fused"):
            disp = self.decoder(feats, only_scales=(0,))[("disp", 0)]
        else:
            disp = self.decoder(feats)[("disp", 0)]
        return disp / MANYDEPTH_DISP_SCALE

    def masked_sq_mean(self, input_image, mask, plan=None, tab=None, clean=None, negate=False, lookup_images=None, poses=None):
        """mean((disp_0 / 8.6437 * mask)^2) on the whole frame: the windowed path (K19) is not extended to the cost-volume
        encoder, so ``plan`` / ``tab`` / ``clean`` are accepted and ignored.  ``lookup_images`` / ``poses``: as forward."""
        disp = self.forward(input_image) if lookup_images is None else self.forward(input_image, lookup_images, poses)
        if disp.is_cuda:
            from . import ops
            cost = ops.masked_sq_mean(disp, mask)
        else:
            cost = ((disp * mask) ** 2).mean()
        return -cost if negate else cost


def _import_manydepth(pre_model_path):
    model_path = pre_model_path
    if model_path is None and os.environ.get("DMH_MODELS_DIR"):
        cand = os.path.join(os.environ["DMH_MODELS_DIR"], "KITTI_HR")
        model_path = cand if os.path.isdir(cand) else None
    enc = torch.load(os.path.join(model_path, "encoder.pth"), map_location="cpu") if model_path is not None else {}
    encoder = networks.ResnetEncoderMatching(18, False, input_width=int(enc.get("width", 1024)), input_height=int(enc.get("height", 320)),
                                             adaptive_bins=True, min_depth_bin=float(enc.get("min_depth_bin", 0.1)),
                                             max_depth_bin=float(enc.get("max_depth_bin", 20.0)), depth_binning='linear',
                                             num_depth_bins=96)
    decoder = networks.DepthDecoder(num_ch_enc=encoder.num_ch_enc, scales=range(4))
    if model_path is not None:
        encoder.load_state_dict({k: v for k, v in enc.items() if k in encoder.state_dict()})
        decoder.load_state_dict(torch.load(os.path.join(model_path, "depth.pth"), map_location="cpu"))
    model = ManyDepthModelWrapper(encoder, decoder, enc)
    model.model_type, model.model_name = 'manydepth', 'KITTI_HR'
    return model


def import_depth_model(scene_size, model_type='monodepth2', pre_model_path=None, matching=False):
    """Build the ResNet-18 depth model of ``model_type`` and load ``encoder.pth`` / ``depth.pth`` (depth_model.py:89-161, which
    filters the encoder dict by key the same way).  'monodepth2' (``mono+stereo_1024x320``) and 'depthhints'
    (``DH_MS_320_1024``, BASELINE config 4) are the same architecture -- DepthHints' networks/ is Monodepth2's -- and differ in
    the weights folder only; 'manydepth' (cost-volume encoder) is outside the hot path.  The reference reads
    ``DepthNetworks/<fork>/models/<name>``; here the folder is ``pre_model_path`` or ``$DMH_MODELS_DIR/<name>``; without
    weights on disk the model is randomly initialised (no network in this environment).

    scene_size: (width, height)."""
    names = {'monodepth2': 'mono+stereo_1024x320', 'depthhints': 'DH_MS_320_1024'}
    if tuple(scene_size) not in ((1024, 320),):
        raise RuntimeError("scene size undefined!")
    if model_type == 'manydepth' and matching:
        return _import_manydepth(pre_model_path)
    if model_type == 'manydepth':
        raise RuntimeError("the manydepth depth model (cost-volume encoder) is outside the hot-path scope")
    if model_type not in names:
        raise RuntimeError("depth model unfound")
    model_path = pre_model_path
    if model_path is None and os.environ.get("DMH_MODELS_DIR"):
        cand = os.path.join(os.environ["DMH_MODELS_DIR"], names[model_type])
        model_path = cand if os.path.isdir(cand) else None
    encoder = networks.ResnetEncoder(18, False)
    decoder = networks.DepthDecoder(num_ch_enc=encoder.num_ch_enc, scales=range(4))
    if model_path is not None:
        enc = torch.load(os.path.join(model_path, "encoder.pth"), map_location="cpu")
        encoder.load_state_dict({k: v for k, v in enc.items() if k in encoder.state_dict()})
        decoder.load_state_dict(torch.load(os.path.join(model_path, "depth.pth"), map_location="cpu"))
    model = DepthModelWrapper(encoder, decoder)
    model.model_type, model.model_name = model_type, names[model_type]
    return model
