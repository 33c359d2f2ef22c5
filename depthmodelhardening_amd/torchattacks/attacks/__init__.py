from .phy_obj_atk_apgd import Phy_obj_atk_APGD  # noqa: F401
from .phy_obj_atk_arbi import Phy_obj_atk_arbi  # noqa: F401
from .phy_obj_atk_guassian import Phy_obj_atk_guassian  # noqa: F401
from .phy_obj_atk_l2 import Phy_obj_atk_l2  # noqa: F401
from .phy_obj_atk_multiframe import Phy_obj_atk_mf  # noqa: F401
from .phy_obj_atk_light import Phy_obj_atk_light  # noqa: F401
from .phy_obj_atk_square import Phy_obj_atk_Square  # noqa: F401
from .phy_obj_atk_vanila import Phy_obj_atk_vanila  # noqa: F401
