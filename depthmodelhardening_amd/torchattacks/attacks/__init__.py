from .phy_obj_atk_apgd import Phy_obj_atk_APGD  # noqa: F401
