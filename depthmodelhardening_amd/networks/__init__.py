from .depth_decoder import DepthDecoder
from .matching_encoder import ResnetEncoderMatching
from .pose_decoder import PoseDecoder
from .resnet_encoder import ResnetEncoder

__all__ = ["ResnetEncoder", "ResnetEncoderMatching", "DepthDecoder", "PoseDecoder"]
