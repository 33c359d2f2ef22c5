from .depth_decoder import DepthDecoder
from .pose_decoder import PoseDecoder
from .resnet_encoder import ResnetEncoder

__all__ = ["ResnetEncoder", "DepthDecoder", "PoseDecoder"]
