from .oriented_head import OrientedHead  # noqa: F401
from .oriented_rpn_head import OrientedRPNHead  # noqa: F401
from .s2anet_head import AlignConv, S2ANetHead, bbox_decode  # noqa: F401
from .rotated_retina_head import RotatedRetinaHead  # noqa: F401
from .kfiou_rotated_retina_head import KFIoURRetinaHead  # noqa: F401
from .rotated_atss_head import RotatedATSSHead  # noqa: F401
from .rbbox_head import BBoxHeadRbbox  # noqa: F401
from .convfc_rbbox_head import ConvFCBBoxHeadRbbox, SharedFCBBoxHeadRbbox  # noqa: F401
from .fasterrcnn_head import AnchorHead, FasterrcnnHead  # noqa: F401
from .gliding_rpn_head import GlidingRPNHead  # noqa: F401
from .gliding_head import GlidingHead  # noqa: F401
from .fcos_head import FCOSHead  # noqa: F401
from .h2rbox_head import H2RBoxHead  # noqa: F401
from .rotated_reppoints_head import MlvlPointGenerator, RotatedRepPointsHead  # noqa: F401
from .rotated_retina_distribution_head import RotatedRetinaDistributionHead  # noqa: F401
from .ld_rotated_retina_head import RotatedRetinaLocalizationDistillationHead  # noqa: F401
from .retina_head import RetinaHead  # noqa: F401
from .csl_rretina_head import CSLRRetinaHead  # noqa: F401
from .strip_head import StripHead  # noqa: F401
