from .kitti import KITTIRAWDataset, KittiSceneFeed
from .synthetic import SyntheticEvalSet, SyntheticKITTIDataset, kitti_like, make_object

__all__ = ["KITTIRAWDataset", "KittiSceneFeed", "SyntheticEvalSet", "SyntheticKITTIDataset", "kitti_like", "make_object"]
