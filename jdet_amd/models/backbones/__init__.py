from .resnet import ResNet, Resnet50, Resnet101  # noqa: F401
from .lsknet import LSKNet, LSKNet_s, LSKNet_t  # noqa: F401
from .stripnet import StripNet, StripNet_S, StripNet_T  # noqa: F401
