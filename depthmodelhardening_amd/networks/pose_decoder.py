"""Pose decoder (MD2/networks/pose_decoder.py): same constructor, same state_dict keys (net.0 squeeze 1x1, net.1 / net.2 the
3x3 convolutions, net.3 the 1x1 that ends in 6 numbers per predicted frame), same return value (axisangle, translation).

On CUDA fp32 tensors the two 3x3 convolutions go through ``ops.conv3x3`` (K10 / K18 where their shapes allow, ATen / MIOpen
otherwise), the 1x1 convolutions stay with ATen / MIOpen, and the tail -- mean over the feature map, 0.01 *, the split and
``transformation_from_parameters`` (MD2/layers.py:28-103) -- is one K29 launch, ``ops.pose_head``.  The matrices it computed on
the way are kept in ``self.T`` [B, num_frames_to_predict_for, 4, 4], so that ``Trainer.predict_poses`` does not launch again;
``forward(..., invert=...)`` says which frames are inverted (negative frame ids).  Any other tensor (CPU, float64) takes the
reference's expressions: that path is test infrastructure and what the golden fixture is checked against.
"""
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import ops
from ..layers import transformation_from_parameters


class PoseDecoder(nn.Module):
    def __init__(self, num_ch_enc, num_input_features, num_frames_to_predict_for=None, stride=1):
        super().__init__()
        self.num_ch_enc = num_ch_enc
        self.num_input_features = num_input_features
        if num_frames_to_predict_for is None:
            num_frames_to_predict_for = num_input_features - 1
        self.num_frames_to_predict_for = num_frames_to_predict_for
        self.convs = OrderedDict()
        self.convs[("squeeze")] = nn.Conv2d(int(self.num_ch_enc[-1]), 256, 1)
        self.convs[("pose", 0)] = nn.Conv2d(num_input_features * 256, 256, 3, stride, 1)
        self.convs[("pose", 1)] = nn.Conv2d(256, 256, 3, stride, 1)
        self.convs[("pose", 2)] = nn.Conv2d(256, 6 * num_frames_to_predict_for, 1)
        self.relu = nn.ReLU()
        self.net = nn.ModuleList(list(self.convs.values()))
        self.T = None

    def _conv3x3(self, conv, x):
        if x.is_cuda and x.dtype == torch.float32 and conv.stride == (1, 1):
            return ops.conv3x3(x, conv.weight, conv.bias, 1)
        return conv(x)

    def forward(self, input_features, invert=False):
        last_features = [f[-1] for f in input_features]
        cat_features = [self.relu(self.convs["squeeze"](f)) for f in last_features]
        out = torch.cat(cat_features, 1)
        out = self.relu(self._conv3x3(self.convs[("pose", 0)], out))
        out = self.relu(self._conv3x3(self.convs[("pose", 1)], out))
        out = self.convs[("pose", 2)](out)
        nf = self.num_frames_to_predict_for
        if out.is_cuda and out.dtype == torch.float32:
            axisangle, translation, self.T = ops.pose_head(out, invert)
            return axisangle, translation
        out = out.mean(3).mean(2)
        out = 0.01 * out.view(-1, nf, 1, 6)
        axisangle = out[..., :3]
        translation = out[..., 3:]
        flags = [bool(invert)] * nf if isinstance(invert, (bool, int)) else [bool(v) for v in invert]
        self.T = torch.stack([transformation_from_parameters(axisangle[:, f], translation[:, f], invert=flags[f])
                              for f in range(nf)], 1)
        return axisangle, translation
