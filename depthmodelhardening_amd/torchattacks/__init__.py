"""The depth attacks of the reference's patched ``torchattacks`` package that the training path uses
(torchattacks/__init__.py:6-8), and the evaluation attacks built so far: Auto-PGD on the object patch
(MD2/evaluate_depth.py:138-141), the tube-light random search with its no-op paste (:150-151, :178-182), the Gaussian-blur search
(:148-149), the random-patch baseline (:146-147), the Square attack (:142-145) and L2 PGD on the object patch in its shared-patch
form (:133-137).  That is every ``norm_type`` row of the reference's ``evaluate_attacks``.  The stock classification attacks
 are out of scope."""
from .attack import Attack
from .attacks.pgd_depth import PGD_depth
from .attacks.phy_obj_atk import Phy_obj_atk
from .attacks.phy_obj_atk_apgd import Phy_obj_atk_APGD
from .attacks.phy_obj_atk_arbi import Phy_obj_atk_arbi
from .attacks.phy_obj_atk_guassian import Phy_obj_atk_guassian
from .attacks.phy_obj_atk_l0 import Phy_obj_atk_l0
from .attacks.phy_obj_atk_l2 import Phy_obj_atk_l2
from .attacks.phy_obj_atk_multiframe import Phy_obj_atk_mf
from .attacks.phy_obj_atk_light import Phy_obj_atk_light
from .attacks.phy_obj_atk_square import Phy_obj_atk_Square
from .attacks.phy_obj_atk_vanila import Phy_obj_atk_vanila

__all__ = ["Attack", "PGD_depth", "Phy_obj_atk", "Phy_obj_atk_APGD", "Phy_obj_atk_arbi", "Phy_obj_atk_guassian", "Phy_obj_atk_l0", "Phy_obj_atk_l2", "Phy_obj_atk_mf", "Phy_obj_atk_light", "Phy_obj_atk_Square", "Phy_obj_atk_vanila"]
