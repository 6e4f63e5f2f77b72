"""CPU: the ATSS pieces that need no device -- the fixtures of tests/atss_ref.py hold the conditions under which the
restatement (literal float64 inside test, stable-sort tie order) and the kernel (algebraic fp32 inside test) must agree;
closed forms of the restatement; the names in SIGNATURES and the workspace query; the argument checks of
jdet_atss_assign; the registry names and the config; points_in_rotated_boxes."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import atss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_fixture_holds_the_conditions(name):
    anchors, num_level, gts, labels, ref = R.fixture(name)
    size, K, _ = R.FIXTURES[name]
    assert anchors.shape[0] == {256: 1364, 512: 5456}[size] and ref["cand"].shape == (K, {256: 40, 512: 45}[size])
    print("%s: margin %.2e, boundary ties %d, positives per gt %s, anchors claimed twice %d"
          % (name, ref["margin"], ref["boundary_ties"], ref["positives_per_gt"].tolist(), ref["multi_claimed"]))
    assert ref["margin"] >= 1e-5
    assert ref["boundary_ties"] == 0
    assert (ref["positives_per_gt"] >= 1).all()
    assert ref["multi_claimed"] >= 1
    if size == 256:
        assert num_level == [1024, 256, 64, 16, 4]          # the last level is below topk: min(topk, n)


def test_gt_identical_to_an_anchor_takes_it_with_iou_one():
    anchors, num_level = R.lattice(256)
    j = 1024 + 256 + 27                                      # an anchor of level 2
    ref = R.assign(anchors, num_level, anchors[j:j + 1].copy(), R.TOPK)
    assert ref["gt_inds"][j] == 1 and ref["max_overlaps"][j] == np.float32(1.0)


def test_no_positive_lies_outside_its_gt_and_a_tiny_gt_gets_none():
    anchors, num_level, gts, _, ref = R.fixture("256b")
    flags, _ = R.inside_literal64(anchors[:, :2], gts)
    pos = np.flatnonzero(ref["gt_inds"] > 0)
    assert pos.size and flags[pos, ref["gt_inds"][pos] - 1].all()
    assert (ref["max_overlaps"][ref["gt_inds"] == 0] == R.NEG_INF).all()
    # a gt between four lattice points of the finest level, too small to contain any anchor centre
    tiny = np.asarray([[7.5, 7.5, 3.0, 3.0, 0.3]], np.float32)
    out = R.assign(anchors, num_level, tiny, R.TOPK)
    assert (out["gt_inds"] == 0).all() and out["positives_per_gt"].tolist() == [0]


@pytest.fixture(scope="module")
def built_lib():
    from jdet_amd import _lib
    _lib.build()
    return _lib


def test_header_signatures_and_exports_agree(built_lib):
    assert {"jdet_atss_assign", "jdet_atss_assign_workspace"} <= set(built_lib.SIGNATURES)
    lib = built_lib.lib()
    assert lib.jdet_atss_assign_workspace(1364, 8, 5, 9) == 1364 * 8 + 8 * 45 * 4
    assert lib.jdet_atss_assign_workspace(10, 3, 1, 3) == 10 * 8 + 40            # 36 bytes of indices, rounded up to 8
    assert lib.jdet_atss_assign_workspace(10, 3, 8, 9) == 0                      # 72 candidates: unsupported


def test_argument_checks_return_before_any_launch(built_lib):
    lib = built_lib.lib()
    N, X = None, 4096                                        # X: a non-null, 8-byte aligned address nobody reads
    offs = (ctypes.c_int32 * 3)(0, 6, 10)
    need = lib.jdet_atss_assign_workspace(10, 2, 2, 3)

    def call(anchors=X, A=10, stride=5, lo=offs, L=2, gt=X, K=2, gl=N, ov=N, topk=3, gi=X, mo=X, lab=N, ws=X, wsb=need):
        return lib.jdet_atss_assign(anchors, A, stride, lo, L, gt, K, gl, ov, topk, 0, gi, mo, lab, ws, wsb, N)
    for null in ("anchors", "lo", "gt", "gi", "mo", "ws"):
        assert call(**{null: N}) == -1, null
    assert call(lab=X) == -1                                 # labels without gt_labels
    assert call(ws=X + 4) == -1                              # workspace not 8-byte aligned
    assert call(K=0) == -1 and call(A=0) == -1 and call(K=-3) == -1
    assert call(stride=4) == -1 and call(topk=0) == -1 and call(L=0) == -1
    assert call(lo=(ctypes.c_int32 * 3)(0, 6, 9)) == -1      # does not end at A
    assert call(lo=(ctypes.c_int32 * 3)(1, 6, 10)) == -1     # does not start at 0
    assert call(lo=(ctypes.c_int32 * 3)(0, 11, 10)) == -1    # decreasing
    assert call(wsb=need - 1) == -3
    assert call(topk=33) == -2                               # L * topk = 66 > JDET_ATSS_MAX_CANDIDATES
    assert call(A=1, lo=(ctypes.c_int32 * 3)(0, 0, 1)) == -2  # C = 1: the variance divides by C - 1
    assert call(lo=(ctypes.c_int32 * 3)(0, 0, 10), wsb=need - 1) == -3     # an empty level is allowed


def test_registry_builds_the_assigner_the_head_and_the_model():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.config import Config
    from jdet_amd.config.named import ATSS_RETINANET_CFG
    from jdet_amd.utils import registry as Reg
    a = Reg.build_from_cfg(dict(type="ATSSAssignerRbbox", topk=9, iou_calculator=dict(type="BboxOverlaps2D_rotated")),
                           Reg.BOXES)
    assert a.topk == 9 and a.assigned_labels_filled == 0 and type(a.iou_calculator).__name__ == "BboxOverlaps2D_rotated"
    with pytest.raises(ValueError, match="No gt or bboxes"):
        a.assign(torch.zeros((0, 5)), [0], torch.zeros((3, 5)))
    h = Reg.build_from_cfg(dict(type="RotatedATSSHead", num_classes=16, in_channels=256), Reg.HEADS)
    assert h.num_anchors == 1 and h.train_cfg.assigner.type == "ATSSAssignerRbbox"
    m = Reg.build_from_cfg(ATSS_RETINANET_CFG["model"], Reg.MODELS)
    assert type(m).__name__ == "RotatedRetinaNet" and type(m.bbox_head).__name__ == "RotatedATSSHead"
    assert m.bbox_head.retina_cls.weight.shape == (15, 256, 1, 1) and m.bbox_head.retina_reg.weight.shape[0] == 5
    # the reference's file, as `Config` reads it, is the named twin
    c = Config(os.path.join(ROOT, "tests", "golden", "configs", "rotated_retinanet_obb_r50_fpn_1x_dota_atss.yaml")).dump()

    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        return [plain(x) for x in v] if isinstance(v, (list, tuple)) else v
    for k in ("model", "optimizer", "scheduler"):
        assert plain(c[k]) == plain(ATSS_RETINANET_CFG[k]), k


def test_assigner_refuses_host_tensors():
    import jdet_amd.models  # noqa: F401
    from jdet_amd._lib import JDetHipError
    from jdet_amd.models.boxes.assigner import ATSSAssignerRbbox
    with pytest.raises(JDetHipError):
        ATSSAssignerRbbox(9).assign(torch.zeros((20, 5)), [20], torch.ones((2, 5)))


def test_points_in_rotated_boxes_matches_the_float64_flags():
    from jdet_amd.models.boxes.box_ops import points_in_rotated_boxes
    anchors, _, gts, _, ref = R.fixture("256a")
    want, margin = R.inside_literal64(anchors[:, :2], gts)
    got = points_in_rotated_boxes(torch.from_numpy(anchors.copy()), torch.from_numpy(gts.copy())).numpy()
    assert got.shape == want.shape == (1364, 8) and got.dtype == np.bool_
    far = margin > 1e-5                                      # fp32 against float64: away from the edges
    assert far.mean() > 0.99 and np.array_equal(got[far], want[far]) and want.any() and not want.all()
