"""Single-stage detector trained against a frozen teacher.  Mirrors python/jdet/models/networks/kd_one_stage.py:L12-98.

The teacher is built from the `model` section of `teacher_config` and kept OUT of the module tree -- the reference's
`dfs` skips it -- so it is in no `parameters()`, `state_dict()`, optimizer or checkpoint.  It still follows `.to()` /
`.cuda()` / `.float()` (`_apply`) and the Runner's channels-last conversion (`frozen_parameters`), stays in eval mode
under `.train()` when `eval_teacher` is set, and runs under `torch.no_grad()`.

`teacher_ckpt` is a LOCAL file in one of the layouts `Runner.load` reads.  The reference config holds an https link
there; nothing here fetches anything: a string that looks like a URL raises ValueError at construction."""
import os
import pickle
import re

import numpy as np
import torch

from jdet_amd.models.utils.level_pack import run_levels
from jdet_amd.utils.registry import MODELS, build_from_cfg

from .rotated_retinanet import RotatedRetinaNet

_URL = re.compile(r"^\s*[A-Za-z][A-Za-z0-9+.\-]*://")


def _load_teacher(model, path):
    if not isinstance(path, (str, os.PathLike)):
        raise TypeError("teacher_ckpt must be a local path, got %r" % type(path).__name__)
    if isinstance(path, str) and _URL.match(path):
        raise ValueError("teacher_ckpt %r looks like a URL: download the checkpoint yourself and pass the local file"
                         % path)
    with open(path, "rb") as f:
        data = pickle.load(f)
    if isinstance(data, dict) and "model" in data:
        data = data["model"]
    elif isinstance(data, dict) and "state_dict" in data:
        data = data["state_dict"]
    own = model.state_dict()
    good = {}
    for k, v in data.items():
        t = torch.as_tensor(np.asarray(v))
        if k in own and tuple(t.shape) == tuple(own[k].shape):
            good[k] = t.to(own[k].dtype)
    model.load_state_dict(good, strict=False)
    return sorted(set(own) - set(good))


@MODELS.register_module()
class KnowledgeDistillationSingleStageDetector(RotatedRetinaNet):
    def __init__(self, teacher_config, backbone, neck=None, bbox_head=None, teacher_ckpt=None, eval_teacher=True):
        if isinstance(teacher_ckpt, str) and _URL.match(teacher_ckpt):   # before anything is built
            raise ValueError("teacher_ckpt %r looks like a URL: download the checkpoint yourself and pass the local file"
                             % teacher_ckpt)
        super().__init__(backbone=backbone, neck=neck, bbox_head=bbox_head)
        self.eval_teacher = eval_teacher
        if isinstance(teacher_config, (str, os.PathLike)):
            if isinstance(teacher_config, str) and _URL.match(teacher_config):
                raise ValueError("teacher_config %r looks like a URL; pass a dict, a Config or a local path"
                                 % teacher_config)
            from jdet_amd.config import Config
            teacher_config = Config(os.fspath(teacher_config)).dump()
        teacher = build_from_cfg(teacher_config["model"], MODELS)
        for p in teacher.parameters():
            p.requires_grad_(False)
        # not a registered submodule (see the module docstring)
        object.__setattr__(self, "teacher_model", teacher)
        self.teacher_missing = _load_teacher(teacher, teacher_ckpt) if teacher_ckpt is not None else []
        self.train(self.training)

    def frozen_parameters(self):
        """the teacher's parameters: what follows the model's layout conversions without being trained or saved"""
        return list(self.teacher_model.parameters())

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self.teacher_model._apply(fn, *args, **kwargs)
        return self

    def train(self, mode=True):
        super().train(mode)
        if "teacher_model" in self.__dict__:
            self.teacher_model.train(mode and not self.eval_teacher)
        return self

    def execute_train(self, images, targets):
        features = self.backbone(images)
        if self.neck:
            features = self.neck(features)
        teacher = self.teacher_model
        with torch.no_grad():
            feats_teacher = teacher.neck(teacher.backbone(images))
            per_level = run_levels(list(feats_teacher), lambda x, mask: teacher.bbox_head.forward_single(x, mask=mask))
            logits_teacher = tuple(map(list, zip(*per_level)))
        return self.bbox_head.execute_train(features, feats_teacher, logits_teacher, targets)

    def forward(self, images, targets):
        if self.training:
            return self.execute_train(images, targets)
        return super().forward(images, targets)

    execute = forward
