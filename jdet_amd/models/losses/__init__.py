from .focal_loss import FocalLoss, sigmoid_focal_loss  # noqa: F401
from .smooth_l1_loss import L1Loss, SmoothL1Loss, smooth_l1_loss  # noqa: F401
from .cross_entropy_loss import CrossEntropyLoss, CrossEntropyLossForRcnn  # noqa: F401
from .gaussian_dist_loss import GDLoss, GDLoss_v1  # noqa: F401
from .kf_iou_loss import KFLoss  # noqa: F401
from .poly_iou_loss import PolyIoULoss, poly_iou_loss  # noqa: F401
from .convex_giou_loss import ConvexGIoULoss  # noqa: F401
from .iou_loss import IoULoss, iou_loss  # noqa: F401
from .h2rbox_loss import H2RBoxLoss  # noqa: F401
from .kd_loss import IMLoss, KnowledgeDistillationKLDivLoss  # noqa: F401
from .smooth_focal_loss import SmoothFocalLoss  # noqa: F401
