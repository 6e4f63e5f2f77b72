"""Gliding Vertex detector.  Mirrors python/jdet/models/networks/gliding_vertex.py:L5-12 (`GlidingVertex(RCNN)`:
backbone -> neck -> GlidingRPNHead -> GlidingHead; train mode returns the head losses + the rpn losses)."""
from jdet_amd.utils.registry import MODELS

from .rcnn import RCNN


@MODELS.register_module()
class GlidingVertex(RCNN):
    """https://arxiv.org/pdf/1911.09358.pdf"""
