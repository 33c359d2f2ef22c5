from .synthetic import SyntheticEvalSet, SyntheticKITTIDataset, kitti_like, make_object

__all__ = ["SyntheticEvalSet", "SyntheticKITTIDataset", "kitti_like", "make_object"]
