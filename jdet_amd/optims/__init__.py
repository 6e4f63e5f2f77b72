from .lr_scheduler import StepLR, WarmUpLR  # noqa: F401
from .optimizer import SGD, AdamW  # noqa: F401
