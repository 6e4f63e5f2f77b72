"""CPU: the Rotated RepPoints pieces that need no device -- closed forms of the assignment restatement
(tests/reppoints_ref.py) and its fixtures' conditions; the names in SIGNATURES and the header's limits; the argument
checks of both entry points (they return before any launch); REPPOINTS_CFG against the reference's file as `Config` reads it; the
model through the registries; MlvlPointGenerator against hand values; use_reassign."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import reppoints_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ the restatement
def test_lg_is_exact_on_powers_of_two_and_log2_elsewhere():
    for e in range(-20, 21):
        assert R.lg(np.float32(2.0 ** e)) == np.float32(e)
    x = np.asarray([3.0, 5.5, 100.0, 1e-6], np.float32)
    np.testing.assert_allclose(R.lg(x), np.log2(x.astype(np.float64)), rtol=0, atol=4e-6)


def test_level_of_exact_power_of_two_boxes():
    # w / scale, h / scale in {8, 16, 32}: level = trunc((a + b) / 2) with a, b in {3, 4, 5}
    for a in (3, 4, 5):
        for b in (3, 4, 5):
            g = R.rect(100.0, 100.0, R.SCALE * 2 ** a, R.SCALE * 2 ** b)
            assert R.level_value(g)[0] == np.float32((a + b) / 2)
            assert R.levels_of(g)[0] == (a + b) // 2
    # the clamp: a 4 x 4 box has the value 0, a 4096 x 4096 box the value 10
    assert R.levels_of(R.rect(10.0, 10.0, 4.0, 4.0))[0] == 3 and R.levels_of(R.rect(0.0, 0.0, 4096.0, 4096.0))[0] == 7


def test_loop_closed_forms():
    points, sizes = R.grid(64, 64)
    assert sizes == [64, 16, 4, 1, 1] and points.shape == (86, 2)
    ids = list(R.LEVEL_IDS)
    # a 32 x 32 square centred on the grid point (16, 24) of level 3 (stride 8): that point and nothing else
    r = R.assign_loop(points, sizes, ids, R.square(16.0, 24.0, 32.0)[None], [7], pos_num=1, labels_filled=-1)
    want = np.zeros(86, np.int32)
    want[3 * 8 + 2] = 1
    assert np.array_equal(r["gt_inds"], want) and r["labels"][3 * 8 + 2] == 7 and (r["labels"][want == 0] == -1).all()
    # centred exactly between (8, 8) and (16, 8): the lower point index
    r = R.assign_loop(points, sizes, ids, R.square(12.0, 8.0, 32.0)[None], pos_num=1)
    assert r["rank_ties"] == 1 and np.flatnonzero(r["gt_inds"]).tolist() == [1 * 8 + 1]
    # two identical gts: the strict < keeps the first
    g = np.stack([R.square(20.0, 20.0, 32.0)] * 2)
    r = R.assign_loop(points, sizes, ids, g, [3, 9], pos_num=3)
    assert r["equal_claims"] == 3 and set(r["gt_inds"].tolist()) == {0, 1} and (r["gt_inds"] == 1).sum() == 3
    assert set(r["labels"][r["gt_inds"] == 1].tolist()) == {3}
    # a nearer later gt takes the point over
    g = np.stack([R.square(20.0, 20.0, 32.0), R.square(17.0, 17.0, 32.0)])
    r = R.assign_loop(points, sizes, ids, g, pos_num=1)
    assert r["gt_inds"][2 * 8 + 2] == 2 and (r["gt_inds"] > 0).sum() == 1
    # a level of one point with pos_num 3: the clamp (a 512 x 512 box: value 7)
    r = R.assign_loop(points, sizes, ids, R.square(32.0, 32.0, 512.0)[None], pos_num=3)
    assert np.flatnonzero(r["gt_inds"]).tolist() == [85]
    # a gap in level_ids: the gt of the missing level claims nothing
    r = R.assign_loop(points[:85], sizes[:4], [3, 4, 6, 7], R.square(32.0, 32.0, 128.0)[None], pos_num=1)
    assert not r["gt_inds"].any()
    # no gts
    r = R.assign_loop(points, sizes, ids, np.zeros((0, 8), np.float32), np.zeros(0, np.int32), labels_filled=-1)
    assert not r["gt_inds"].any() and (r["labels"] == -1).all()


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_fixture_holds_the_conditions(name):
    fx = R.fixture(name)
    (h, w) = fx["hw"]
    assert sum(fx["sizes"]) == len(fx["points"])
    if name == "b2_256":
        assert fx["sizes"] == [1024, 256, 64, 16, 4] and len(fx["points"]) == 1364
    if name == "hw_256x192":
        assert fx["sizes"][0] == 24 * 32 and h != w
    if name == "s64":
        assert fx["sizes"][-2:] == [1, 1]
    if name == "k70_k0":
        assert fx["counts"] == [70, 0] and fx["gt"].shape[1] == 70 > 64
    for b, k in enumerate(fx["counts"]):
        g = fx["gt"][b, :k]
        if k == 0:
            continue
        margin = R.level_margin(g)
        lv = R.levels_of(g)
        for pos_num in (1, 3):
            r = R.assign_loop(fx["points"], fx["sizes"], fx["level_ids"], g, fx["labels"][b, :k], pos_num=pos_num,
                              labels_filled=-1)
            print("%s image %d K %d pos_num %d: level margin min %.2e, gts per level %s, positives %d, rank ties %d, "
                  "equal claims %d" % (name, b, k, pos_num, margin.min(), np.bincount(lv - 3, minlength=5).tolist(),
                                       int((r["gt_inds"] > 0).sum()), r["rank_ties"], r["equal_claims"]))
            assert 1 <= (r["gt_inds"] > 0).sum() <= k * pos_num
        assert (margin >= R.MARGIN).all()
        assert len(np.unique(lv)) >= 2                     # more than one level decides something
        if name == "s64":
            assert (lv >= 6).any()                             # a gt on a one-point level: pos_num = 3 meets the clamp
    if name == "k70_k0":
        # 70 gts on 1364 points: some point is claimed by more than one gt, so the conflict rule decides
        g = fx["gt"][0]
        singles = [np.flatnonzero(R.assign_loop(fx["points"], fx["sizes"], fx["level_ids"], g[i:i + 1], pos_num=3)["gt_inds"])
                   for i in range(70)]
        assert len(np.unique(np.concatenate(singles))) < sum(len(s) for s in singles)


# --------------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def built_lib():
    from jdet_amd import _lib
    _lib.build()
    return _lib


def test_header_signatures_and_exports_agree(built_lib):
    assert {"jdet_convex_point_assign_workspace", "jdet_convex_point_assign",
            "jdet_convex_giou_loss"} <= set(built_lib.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "jdet_hip.h")).read()
    assert int(re.search(r"#define JDET_CONVEX_ASSIGN_MAX_POS (\d+)", hdr).group(1)) == 16
    assert int(re.search(r"#define JDET_CONVEX_ASSIGN_MAX_LEVELS (\d+)", hdr).group(1)) == 8


def test_argument_checks_return_before_any_launch(built_lib):
    lib = built_lib.lib()
    N, X = None, 4096                                        # X: a non-null, 8-byte aligned address nobody reads
    lo = (ctypes.c_int32 * 3)(0, 6, 10)
    ids = (ctypes.c_int32 * 2)(3, 4)
    need = lib.jdet_convex_point_assign_workspace(2, 10)
    assert need == 2 * 10 * 8
    assert lib.jdet_convex_point_assign_workspace(0, 10) == 0 and lib.jdet_convex_point_assign_workspace(2, 0) == 0

    def pa(points=X, n=10, stride=2, lo=lo, ids=ids, L=2, gt=X, gl=X, gc=X, B=2, K=3, scale=4.0, pos=1, gi=X, lab=X,
           ws=X, wsb=need):
        return lib.jdet_convex_point_assign(points, n, stride, lo, ids, L, gt, gl, gc, B, K, scale, pos, 0, gi, lab, ws,
                                            wsb, N)
    for null in ("points", "lo", "ids", "gt", "gc", "gi", "ws"):
        assert pa(**{null: N}) == -1, null
    assert pa(gl=N) == -1                                    # labels without gt_labels
    assert pa(ws=X + 4) == -1                                # not 8-byte aligned
    assert pa(n=0) == -1 and pa(B=0) == -1 and pa(K=-1) == -1 and pa(L=0) == -1 and pa(stride=1) == -1
    assert pa(pos=0) == -1
    for bad in (0.0, -4.0, float("nan"), float("inf")):
        assert pa(scale=bad) == -1, bad
    assert pa(lo=(ctypes.c_int32 * 3)(1, 6, 10)) == -1       # [0] != 0
    assert pa(lo=(ctypes.c_int32 * 3)(0, 6, 9)) == -1        # [L] != N
    assert pa(lo=(ctypes.c_int32 * 3)(0, 11, 10)) == -1      # decreasing
    assert pa(ids=(ctypes.c_int32 * 2)(3, 3)) == -1          # two equal level ids
    assert pa(L=9, lo=(ctypes.c_int32 * 10)(0, 1, 2, 3, 4, 5, 6, 7, 8, 10), ids=(ctypes.c_int32 * 9)(*range(9))) == -2
    assert pa(pos=17) == -2
    assert pa(B=65536, wsb=1 << 40) == -2
    assert pa(n=1 << 30, B=4, lo=(ctypes.c_int32 * 3)(0, 6, 1 << 30), wsb=1 << 40) == -2     # B * N beyond 2^31 - 1
    assert pa(wsb=need - 1) == -3
    assert pa(lo=(ctypes.c_int32 * 3)(0, 0, 10), wsb=need - 1) == -3                          # an empty level is allowed

    def gl(pred=X, target=X, w=X, norm=X, P=5, loss=X, grad=X):
        return lib.jdet_convex_giou_loss(pred, target, w, norm, P, loss, grad, N)
    for null in ("pred", "target", "w", "norm", "loss", "grad"):
        assert gl(**{null: N}) == -1, null
    assert gl(P=-1) == -1
    assert gl(P=(1 << 32) - 1) == -2
    assert gl(P=0, pred=N, target=N, w=N, norm=N, loss=N, grad=N) == 0     # nothing to do, nothing launched


# ---------------------------------------------------------------------------------------------- config, registry, model
def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return [_plain(x) for x in v] if isinstance(v, (list, tuple)) else v


def test_named_config_equals_the_reference_file():
    from jdet_amd.config import Config
    from jdet_amd.config.named import REPPOINTS_CFG
    c = Config(os.path.join(ROOT, "tests", "golden", "configs", "rotated_reppoints_obb_r50_fpn_1x_dota.yaml")).dump()
    for k in ("model", "optimizer", "scheduler"):
        assert _plain(c[k]) == _plain(REPPOINTS_CFG[k]), k
    assert REPPOINTS_CFG["optimizer"]["lr"] == 0.008


def test_registry_builds_the_assigners_the_loss_the_head_and_the_model():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.config.named import REPPOINTS_CFG
    from jdet_amd.ops.dcn_v1 import DeformConv
    from jdet_amd.utils import registry as Reg
    a = Reg.build_from_cfg(dict(type="ConvexAssigner", scale=4, pos_num=1, assigned_labels_filled=-1), Reg.BOXES)
    assert (a.scale, a.pos_num, a.assigned_labels_filled) == (4, 1, -1)
    m = Reg.build_from_cfg(REPPOINTS_CFG["model"]["bbox_head"]["train_cfg"]["refine"]["assigner"], Reg.BOXES)
    assert type(m).__name__ == "MaxConvexIoUAssigner" and type(m.iou_calculator).__name__ == "ConvexOverlaps"
    assert (m.pos_iou_thr, m.neg_iou_thr, m.min_pos_iou, m.assigned_labels_filled) == (0.4, 0.3, 0, -1)
    with pytest.raises(ValueError, match="No gt or bboxes"):
        m.assign(torch.zeros((0, 18)), torch.zeros((3, 8)))
    with pytest.raises(AssertionError):
        m.iou_calculator(torch.zeros((3, 8)), torch.zeros((4, 18)), mode="iof")
    loss = Reg.build_from_cfg(dict(type="ConvexGIoULoss", loss_weight=0.375), Reg.LOSSES)
    assert loss.loss_weight == 0.375 and loss.reduction == "mean"
    cfg = dict(REPPOINTS_CFG["model"])
    cfg["backbone"] = dict(cfg["backbone"], pretrained=False)
    model = Reg.build_from_cfg(cfg, Reg.MODELS)
    assert type(model).__name__ == "RotatedRetinaNet" and type(model.bbox_head).__name__ == "RotatedRepPointsHead"
    # FPN convs carry GroupNorm
    for convs in (model.neck.lateral_convs, model.neck.fpn_convs):
        for cm in convs:
            assert isinstance(cm.gn, torch.nn.GroupNorm) and cm.gn.num_groups == 32 and cm.conv.bias is None
    h = model.bbox_head
    dcn = [n for n, mod in h.named_modules() if isinstance(mod, DeformConv)]
    assert sorted(dcn) == ["reppoints_cls_conv", "reppoints_pts_refine_conv"] and h.num_points == 9
    assert h.dcn_kernel == 3 and h.dcn_pad == 1 and h.cls_out_channels == 15 and h.point_base_scale == 2
    assert h.gradient_mul == 0.3 and h.use_reassign is False and not h.sampling
    # dcn_base_offset: (y, x) of the 3 x 3 kernel taps, row-major, y first
    want = [v for y in (-1, 0, 1) for x in (-1, 0, 1) for v in (y, x)]
    assert h.dcn_base_offset.shape == (1, 18, 1, 1) and h.dcn_base_offset.flatten().tolist() == want
    assert "dcn_base_offset" not in h.state_dict()
    names = {n for n, _ in h.named_parameters()}
    for n in ("cls_convs.2.conv.weight", "reg_convs.2.gn.bias", "reppoints_cls_conv.weight", "reppoints_cls_out.bias",
              "reppoints_pts_init_conv.weight", "reppoints_pts_init_out.bias", "reppoints_pts_refine_conv.weight",
              "reppoints_pts_refine_out.weight"):
        assert n in names, n
    assert "cls_convs.0.conv.bias" not in names and "cls_convs.3.conv.weight" not in names
    assert h.reppoints_pts_init_out.weight.shape == (18, 256, 1, 1) and h.reppoints_cls_out.weight.shape == (15, 256, 1, 1)
    assert type(h.init_assigner).__name__ == "ConvexAssigner" and type(h.refine_assigner).__name__ == "MaxConvexIoUAssigner"
    assert type(h.sampler).__name__ == "PseudoSampler"
    assert type(h.loss_bbox_init).__name__ == "ConvexGIoULoss" and h.loss_bbox_init.loss_weight == 0.375


def test_use_reassign_raises():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.config.named import REPPOINTS_CFG
    from jdet_amd.utils import registry as Reg
    cfg = dict(REPPOINTS_CFG["model"]["bbox_head"], use_reassign=True)
    with pytest.raises(NotImplementedError, match="use_reassign"):
        Reg.build_from_cfg(cfg, Reg.HEADS)


def test_point_generator_grid_and_valid_flags_by_hand():
    from jdet_amd.models.roi_heads.rotated_reppoints_head import MlvlPointGenerator
    g = MlvlPointGenerator([8, 16], offset=0.)
    assert g.num_levels == 2 and g.num_base_priors == [1, 1]
    # a 4 x 3 (h x w) map at stride 8: x runs fastest
    p = g.single_level_grid_priors((4, 3), 0, with_stride=True)
    want = [[x * 8.0, y * 8.0, 8.0, 8.0] for y in range(4) for x in range(3)]
    assert p.dtype == torch.float32 and p.tolist() == want
    assert g.single_level_grid_priors((4, 3), 0).tolist() == [r[:2] for r in want]
    half = MlvlPointGenerator([8], offset=0.5).single_level_grid_priors((1, 2), 0)
    assert half.tolist() == [[4.0, 4.0], [12.0, 4.0]]
    # a padded image of 20 x 17 (h x w) pixels: ceil(20 / 8) = 3 valid rows, ceil(17 / 8) = 3 valid columns of the 4 x 3
    # map; at stride 16 a 2 x 2 map has 2 valid rows and 2 valid columns
    flags = g.valid_flags([(4, 3), (2, 2)], (20, 17))
    assert flags[0].tolist() == [True] * 9 + [False] * 3 and flags[1].tolist() == [True] * 4
    flags = g.valid_flags([(4, 3), (2, 2)], (20, 9))
    assert flags[0].tolist() == [True, True, False] * 3 + [False] * 3 and flags[1].tolist() == [True, False, True, False]
    assert g.sparse_priors(torch.tensor([0, 4, 11]), (4, 3), 0).tolist() == [[0.0, 0.0], [8.0, 8.0], [16.0, 24.0]]


def test_device_only_paths_refuse_host_tensors():
    import jdet_amd.models  # noqa: F401
    from jdet_amd._lib import JDetHipError
    from jdet_amd.models.boxes.assigner import ConvexAssigner
    from jdet_amd.models.losses.convex_giou_loss import ConvexGIoULoss
    pts = torch.tensor([[0.0, 0.0, 8.0, 8.0], [8.0, 0.0, 8.0, 8.0]])
    with pytest.raises(JDetHipError):
        ConvexAssigner(4, 1).assign(pts, torch.from_numpy(R.square(4.0, 0.0, 32.0))[None])
    with pytest.raises(JDetHipError):
        ConvexGIoULoss().dense(torch.zeros((2, 18)), torch.zeros((2, 8)), torch.ones(2), torch.ones(2))
    with pytest.raises(AssertionError):
        ConvexAssigner._levels(torch.tensor([[0.0, 0.0, 12.0, 12.0]]))       # a stride that is no power of two
