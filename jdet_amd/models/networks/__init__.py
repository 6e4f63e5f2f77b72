from .rcnn import RCNN, OrientedRCNN, StripRCNN  # noqa: F401
from .s2anet import S2ANet  # noqa: F401
from .rotated_retinanet import RotatedRetinaNet  # noqa: F401
from .roi_transformer import RoITransformer  # noqa: F401
from .gliding_vertex import GlidingVertex  # noqa: F401
from .fcos import FCOS, SingleStageDetector  # noqa: F401
from .h2rbox import H2RBox  # noqa: F401
from .kd_one_stage import KnowledgeDistillationSingleStageDetector  # noqa: F401
from .retinanet import RetinaNet  # noqa: F401
