"""ManyDepth's cost-volume encoder (reference: manydepth2/networks/resnet_encoder.py:68-331, ``ResnetEncoderMatching``).

The first two ResNet stages run on the current frame and on every lookup frame; a plane-sweep cost volume over
``num_depth_bins`` depth hypotheses is built at 1/4 resolution; ``reduce_conv`` (3x3 over 64 + D channels) follows, then layers
2-4.  The state-dict keys are the reference's (``layer0.0``, ``layer0.1``, ``layer1.1.{0,1}``, ``layer2`` .. ``layer4``,
``backprojector``'s pixel grid, ``prematching_conv.0`` -- declared and unused there too -- and ``reduce_conv.0``), so its ``encoder.pth`` files load unchanged.

In eval() mode on CUDA fp32 tensors the stages run the fused paths ``ResnetEncoder`` uses for whole frames (K14, K9, K10 / K15),
the cost volume is K30 (``ops.cost_volume``: one transposing pass and one launch, no host read, so the forward can be captured
into a graph) and ``reduce_conv`` goes through ``ops.conv3x3``.  CPU tensors take the module path: plain PyTorch expressions of
the reference's arithmetic, which also serve as the CPU restatement the GPU tests compare with.

In train() mode with gradients enabled, on CUDA fp32 tensors, the degenerate call -- the one the reference trains
(manydepth2/trainer.py:371-385) -- runs the fused train path of ``ResnetEncoder.forward``: K14 for the stem (weight gradient K21),
``ops.stem_bn_relu_pool_train`` on ``layer0.1``, the BasicBlocks' train-fused branch, the K10 filter prefetch, and ``reduce_conv`` as
one autograd node (K36, ``ops.reduce_conv_degenerate``).  ``fuse_train = False`` switches that off (the module path; the blocks keep
their own train-fused branch).  The multi-frame call keeps the module path in train mode: the reference does not train it.

Two call forms.  Multi-frame: real lookup frames and relative poses.  Degenerate: the reference's wrapper, trainer and evaluation
call the encoder with ``lookup_images * 0`` and a [1,1,4,4] zero pose, so every lookup is "missing", the volume and the confidence
are zero; a caller that KNOWS there are no lookups passes ``lookup_images=None`` and pays for neither lookup features nor a cost
volume (``reduce_conv`` then runs on the 64 feature channels with ``weight[:, :64]``: the zero channels contribute exact zeros).
The general path given all-zero poses computes the same tensors; nothing on the device is special-cased.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .resnet_encoder import _CONFIGS, ResNet, _plain3x3, _train_fused


class _PixelGrid(nn.Module):
    """The reference's ``BackprojectDepth`` (manydepth2/layers.py:139-162) keeps its pixel grid as three frozen parameters, which
    therefore are keys of every ``encoder.pth``: ``id_coords`` [2,H,W], ``ones`` [D,1,HW], ``pix_coords`` [D,3,HW] = (x, y, 1)
    repeated per depth bin.  Declared here with the same names, shapes and values so that those files load strictly; the module
    path reads ``pix_coords[:1]``, K30 computes the grid itself."""

    def __init__(self, bins, height, width):
        super().__init__()
        ys, xs = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32), indexing="ij")
        self.id_coords = nn.Parameter(torch.stack([xs, ys], 0), requires_grad=False)
        self.ones = nn.Parameter(torch.ones(bins, 1, height * width), requires_grad=False)
        pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(height * width)], 0)
        self.pix_coords = nn.Parameter(pix.unsqueeze(0).repeat(bins, 1, 1), requires_grad=False)


class ResnetEncoderMatching(nn.Module):
    """Setting ``adaptive_bins=True`` recomputes the depth bins from ``min_depth_bin`` / ``max_depth_bin`` of each forward (they
    are cached per value, so unchanged limits upload nothing)."""

    def __init__(self, num_layers, pretrained, input_height, input_width, min_depth_bin=0.1, max_depth_bin=20.0,
                 num_depth_bins=96, adaptive_bins=False, depth_binning='linear'):
        super().__init__()
        if num_layers not in _CONFIGS:
            raise ValueError("{} is not a valid number of resnet layers".format(num_layers))
        if pretrained:
            print("ResnetEncoderMatching: ImageNet weights are not available offline -- using random initialisation")
        self.adaptive_bins = adaptive_bins
        self.depth_binning = depth_binning
        self.set_missing_to_max = True
        self.num_ch_enc = np.array([64, 64, 128, 256, 512])
        self.num_depth_bins = num_depth_bins
        self.matching_height, self.matching_width = input_height // 4, input_width // 4     # the volume is built at 1/4 resolution
        self.roi_backward = False       # the windowed attack path (K19) is not extended to this encoder
        self.fuse_train = True          # train(): the fused stem / reduce_conv path of the degenerate call (False: module path)
        # True: with lookup frames, the lookup features and the volume are built WITH gradient (K38; this project's addition --
        # the reference computes both under no_grad, which False keeps: the volume is then a constant of every gradient).
        # "current": the volume with gradient, the lookup features without -- the gradient reaches the current frame only
        self.matching_grad = False

        block, layers = _CONFIGS[num_layers]
        trunk = ResNet(block, layers)
        self.layer0 = nn.Sequential(trunk.conv1, trunk.bn1, trunk.relu)
        self.layer1 = nn.Sequential(trunk.maxpool, trunk.layer1)
        self.layer2 = trunk.layer2
        self.layer3 = trunk.layer3
        self.layer4 = trunk.layer4
        # the ResNet object itself (its eval_affine / fused_eval_ok helpers) is kept outside the module tree: its modules are
        # the ones registered above, and the state dict has the reference's keys only
        self.__dict__["_trunk"] = trunk
        if num_layers > 34:
            self.num_ch_enc[1:] *= 4

        self.backprojector = _PixelGrid(self.num_depth_bins, self.matching_height, self.matching_width)

        self._bins = {}             # (min, max, D, binning) -> {"cpu": tensor, device: tensor}
        self.depth_bins = None
        self.compute_depth_bins(min_depth_bin, max_depth_bin)

        self.prematching_conv = nn.Sequential(nn.Conv2d(64, out_channels=16, kernel_size=1, stride=1, padding=0),
                                              nn.ReLU(inplace=True))
        self.reduce_conv = nn.Sequential(nn.Conv2d(int(self.num_ch_enc[1]) + self.num_depth_bins, out_channels=int(self.num_ch_enc[1]),
                                                   kernel_size=3, stride=1, padding=1),
                                         nn.ReLU(inplace=True))

    # ------------------------------------------------------------------------------------------------------ depth bins
    def compute_depth_bins(self, min_depth_bin, max_depth_bin):
        """The depth hypotheses, linear in depth ('linear') or in inverse depth ('inverse'), made on the host in float64 and
        rounded to float32 as the reference does (resnet_encoder.py:133-147)."""
        key = (float(min_depth_bin), float(max_depth_bin), int(self.num_depth_bins), self.depth_binning)
        entry = self._bins.get(key)
        if entry is None:
            if self.depth_binning == 'inverse':
                bins = 1 / np.linspace(1 / max_depth_bin, 1 / min_depth_bin, self.num_depth_bins)[::-1]
            elif self.depth_binning == 'linear':
                bins = np.linspace(min_depth_bin, max_depth_bin, self.num_depth_bins)
            else:
                raise NotImplementedError
            if len(self._bins) >= 16:       # a caller that tracks running limits would otherwise grow the cache without bound
                self._bins.clear()
            entry = self._bins[key] = {"cpu": torch.from_numpy(np.ascontiguousarray(bins)).float()}
        self._bins_entry = entry
        self.depth_bins = entry["cpu"]

    def _bins_on(self, device):
        device = torch.device(device)
        if device.type == "cpu":
            return self.depth_bins
        if device not in self._bins_entry:
            self._bins_entry[device] = self.depth_bins.to(device)
        return self._bins_entry[device]

    def indices_to_disparity(self, indices):
        """1 / depth of cost-volume indices [B,H,W], gathered on the indices' device."""
        return 1 / self._bins_on(indices.device)[indices.long()]

    def compute_confidence_mask(self, cost_volume, num_bins_threshold=None):
        if num_bins_threshold is None:
            num_bins_threshold = self.num_depth_bins
        return ((cost_volume > 0).sum(1) == num_bins_threshold).float()

    # ----------------------------------------------------------------------------------------------------- cost volume
    def _check_lookups(self, batch, lookups, poses):
        if poses.dim() != 4 or tuple(poses.shape[2:]) != (4, 4):
            raise RuntimeError("ResnetEncoderMatching: poses must be [Bp,L,4,4]; got %s" % (tuple(poses.shape),))
        if poses.shape[1] != lookups:
            raise RuntimeError("ResnetEncoderMatching: poses name %d lookup frames, there are %d" % (poses.shape[1], lookups))
        if not 1 <= poses.shape[0] <= batch:
            raise RuntimeError("ResnetEncoderMatching: poses has %d rows for a batch of %d" % (poses.shape[0], batch))

    def match_features(self, current_feats, lookup_feats, relative_poses, K, invK):
        """(cost_volume, missing_mask), both [B,D,H,W]: the mean absolute difference between the current features and the lookup
        features warped to each depth hypothesis, averaged over the lookups that are present (a lookup whose pose sums to 0 is
        missing), border samples masked out (resnet_encoder.py:157-236)."""
        self._check_lookups(current_feats.shape[0], lookup_feats.shape[1], relative_poses)
        if current_feats.is_cuda and current_feats.dtype == torch.float32:
            return ops.cost_volume(current_feats, lookup_feats, relative_poses, K, invK, self._bins_on(current_feats.device),
                                   self.set_missing_to_max)[:2]
        return self._match_features_module(current_feats, lookup_feats, relative_poses, K, invK)

    def _match_features_module(self, current_feats, lookup_feats, relative_poses, K, invK):
        """The reference's arithmetic as plain PyTorch expressions, any device and dtype (``ops.cost_volume_module``: the one copy,
        which ``ops.cost_volume_stack`` differentiates for CPU tensors)."""
        H, W = current_feats.shape[2:]
        if (H, W) != (self.matching_height, self.matching_width):
            raise RuntimeError("ResnetEncoderMatching: features of %d x %d, the matching grid is %d x %d" % (
                H, W, self.matching_height, self.matching_width))
        return ops.cost_volume_module(current_feats, lookup_feats, relative_poses, K, invK, self.depth_bins, self.set_missing_to_max)

    # ------------------------------------------------------------------------------------------------------------ stages
    def _fused_ok(self, image):
        c = self.layer0[0]
        return (self._trunk.fused_eval_ok(image) and image.dim() == 4 and image.shape[1] == 3 and image.shape[2] % 4 == 0
                and image.shape[3] % 4 == 0 and tuple(c.weight.shape) == (64, 3, 7, 7) and c.stride == (2, 2)
                and c.padding == (3, 3) and c.dilation == (1, 1) and c.groups == 1 and c.bias is None)

    def _head_fused(self, image, aff):
        """[features 0, features 1] of ``image`` on the fused eval path (K14, K9's stem pass, the layer-1 blocks)."""
        z = ops.stem_conv_norm(image, self.layer0[0].weight, 0.45, 0.225)
        f0, y = ops.stem_bn_relu_pool(z, *aff[self.layer0[1]])
        for blk in self.layer1[1]:
            y = blk.forward_fused(y, aff)
        return [f0, y]

    def _stem_is_standard(self, image):
        c = self.layer0[0]
        return (image.dim() == 4 and image.shape[1] == 3 and image.shape[2] % 4 == 0 and image.shape[3] % 4 == 0
                and tuple(c.weight.shape) == (64, 3, 7, 7) and c.stride == (2, 2) and c.padding == (3, 3) and c.dilation == (1, 1)
                and c.groups == 1 and c.bias is None)

    def _train_fused_ok(self, image):
        """The conditions of ResnetEncoder.forward's train branch (its _stem and _train_fused), and reduce_conv as declared."""
        r = self.reduce_conv[0]
        return (self.fuse_train and _train_fused(self.layer0[1], image) and self._stem_is_standard(image)
                and r.kernel_size == (3, 3) and r.stride == (1, 1) and r.padding == (1, 1) and r.dilation == (1, 1) and r.groups == 1
                and r.bias is not None and r.out_channels % 8 == 0)

    def _k10_convs(self):
        """The 3x3 stride-1 convolutions of the residual blocks: the filters K10 may be asked for (ResnetEncoder._k10_convs)."""
        if self.__dict__.get("_k10_list") is None:
            out = []
            for layer in (self.layer1[1], self.layer2, self.layer3, self.layer4):
                for blk in layer:
                    for conv in (getattr(blk, "conv1", None), getattr(blk, "conv2", None)):
                        if conv is not None and conv.kernel_size == (3, 3) and _plain3x3(conv):
                            out.append(conv)
            self.__dict__["_k10_list"] = out
        return self.__dict__["_k10_list"]

    def _prefetch_filters(self):
        """All K10 filters of the train pass in one launch, as ResnetEncoder._prefetch_filters does (inside ops.wino_pass() a pose
        encoder's prefetch leaves them in place): the blocks' and reduce_conv's ``weight[:, :64]``."""
        dirs = (False, True) if torch.is_grad_enabled() else (False,)
        jobs = [(c.weight, bw, None) for c in self._k10_convs() for bw in dirs]
        w = self.reduce_conv[0].weight
        if w.is_cuda and w.dtype == torch.float32:
            wc = ops._reduce_slice(w, int(self.num_ch_enc[1]), fresh=True)      # every forward, like the transforms below
            jobs += [(wc, bw, None) for bw in dirs]
        ops.wino_prefetch(jobs, fresh=True)

    def _head_train(self, image):
        """[features 0, features 1] on the fused train path: K14, K9's train-mode stem pass, the layer-1 blocks."""
        z = ops.stem_conv_norm(image, self.layer0[0].weight, 0.45, 0.225)
        f0, p = ops.stem_bn_relu_pool_train(self.layer0[1], z)
        return [f0, self.layer1[1](p)]

    def feature_extraction(self, image, return_all_feats=False):
        """The first two ResNet stages on ``(image - 0.45) / 0.225``."""
        if self._fused_ok(image):
            feats = self._head_fused(image, self._trunk.eval_affine())
        else:
            f0 = self.layer0((image - 0.45) / 0.225)
            feats = [f0, self.layer1(f0)]
        return feats if return_all_feats else feats[1]

    def _reduce(self, x, weight):
        conv = self.reduce_conv[0]
        if x.is_cuda and x.dtype == torch.float32:
            return torch.relu(ops.conv3x3(x, weight, conv.bias, 1))
        return torch.relu(F.conv2d(x, weight, conv.bias, 1, 1))

    def _tail(self, post, fused):
        """features 2 .. 4 from reduce_conv's output; the list so far is self.features."""
        feats = self.features
        if not fused:
            for layer in (self.layer2, self.layer3, self.layer4):
                post = layer(post)
                feats.append(post)
            return feats
        aff = self._trunk.eval_affine()
        y = post
        for li, layer in enumerate((self.layer2, self.layer3, self.layer4)):
            for bi, blk in enumerate(layer):
                if li > 0 and bi == 0 and hasattr(blk, "_is_down_pair"):
                    y, feats[-1] = blk.forward_fused(y, aff, want_skip=True)    # y: a pyramid feature with two consumers
                else:
                    y = blk.forward_fused(y, aff)
            feats.append(y)
        return feats

    def _forward_matching_grad(self, current_feats, lookup_images, poses, K, invK, bins, weight, fused):
        """The multi-frame tail of forward with the matching path differentiable.  CUDA fp32 features take ``ops.cost_volume_stack``
        (K30 + K38, one node) whether or not the stages around it run fused -- ``match_features`` would hand them to K30, which is
        forward only and would make the volume a constant again; everything else takes the module expression, the lines of forward
        without no_grad / detach.  The same values as forward's."""
        B, C, H, W = current_feats.shape
        L = lookup_images.shape[1]
        with torch.set_grad_enabled(self.matching_grad != "current" and torch.is_grad_enabled()):
            lookup_feats = self.feature_extraction(lookup_images.reshape(B * L, *lookup_images.shape[2:]))
        lookup_feats = lookup_feats.reshape(B, L, C, H, W)
        if current_feats.is_cuda and current_feats.dtype == torch.float32:
            stacked, confidence_mask, argmin = ops.cost_volume_stack(current_feats, lookup_feats, poses, K, invK, bins,
                                                                     self.set_missing_to_max)
        else:
            cost_volume, missing_mask = self._match_features_module(current_feats, lookup_feats, poses, K, invK)
            with torch.no_grad():
                confidence_mask = self.compute_confidence_mask(cost_volume * (1 - missing_mask))
                viz = torch.where(cost_volume == 0, torch.full_like(cost_volume, 100.0), cost_volume)
                argmin = torch.min(viz, 1)[1]
            cost_volume = cost_volume * confidence_mask.unsqueeze(1)
            stacked = torch.cat([current_feats, cost_volume], 1)
        with torch.no_grad():
            lowest_cost = self.indices_to_disparity(argmin)
        post = self._reduce(stacked, weight)
        return self._tail(post, fused), lowest_cost, confidence_mask

    def forward(self, current_image, lookup_images, poses, K, invK, min_depth_bin=None, max_depth_bin=None):
        """(features, lowest_cost, confidence_mask).  ``lookup_images`` [B,L,3,H,W], or None: the caller states that there are no
        lookup frames (the degenerate call; ``poses`` is then not read)."""
        fused = self._fused_ok(current_image)
        train_fused = not fused and lookup_images is None and self._train_fused_ok(current_image)
        if self.adaptive_bins and min_depth_bin is not None and max_depth_bin is not None:
            self.compute_depth_bins(min_depth_bin, max_depth_bin)
        if train_fused:
            self._prefetch_filters()
            self.features = self._head_train(current_image)
        else:
            self.features = self.feature_extraction(current_image, return_all_feats=True)
        current_feats = self.features[-1]
        B, C, H, W = current_feats.shape
        D = self.num_depth_bins
        weight = self.reduce_conv[0].weight
        bins = self._bins_on(current_feats.device)

        if lookup_images is None:
            confidence_mask = current_feats.new_zeros((B, H, W))
            lowest_cost = (1 / bins[:1]).to(current_feats.dtype).expand(B, H * W).reshape(B, H, W)
            if train_fused:
                post = ops.reduce_conv_degenerate(current_feats, weight, self.reduce_conv[0].bias)       # K36: one autograd node
            else:
                post = self._reduce(current_feats, weight[:, :C].contiguous())
            return self._tail(post, fused), lowest_cost, confidence_mask

        if lookup_images.dim() != 5 or lookup_images.shape[0] != B or lookup_images.shape[2:] != current_image.shape[1:]:
            raise RuntimeError("ResnetEncoderMatching: lookup_images must be [B,L,3,H,W] at the current frame's size; got %s for %s"
                               % (tuple(lookup_images.shape), tuple(current_image.shape)))
        L = lookup_images.shape[1]
        self._check_lookups(B, L, poses)
        if self.matching_grad:
            return self._forward_matching_grad(current_feats, lookup_images, poses, K, invK, bins, weight, fused)
        with torch.no_grad():
            lookup_feats = self.feature_extraction(lookup_images.reshape(B * L, *lookup_images.shape[2:]))
            lookup_feats = lookup_feats.reshape(B, L, C, H, W)
            if fused:
                stacked = torch.empty((B, C + D, H, W), device=current_feats.device, dtype=torch.float32)
                _, _, confidence_mask, argmin = ops.cost_volume(current_feats, lookup_feats, poses, K, invK, bins,
                                                                self.set_missing_to_max, into=stacked)
            else:
                cost_volume, missing_mask = self.match_features(current_feats.detach(), lookup_feats, poses, K, invK)
                confidence_mask = self.compute_confidence_mask(cost_volume * (1 - missing_mask))
                viz = torch.where(cost_volume == 0, torch.full_like(cost_volume, 100.0), cost_volume)
                argmin = torch.min(viz, 1)[1]
                cost_volume = cost_volume * confidence_mask.unsqueeze(1)
            lowest_cost = self.indices_to_disparity(argmin)
        if fused:
            stacked[:, :C] = current_feats
        else:
            stacked = torch.cat([current_feats, cost_volume], 1)
        post = self._reduce(stacked, weight)
        return self._tail(post, fused), lowest_cost, confidence_mask
