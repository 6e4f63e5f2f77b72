"""GPU: RetinaNet-v1d -- every row of tests/retina_cases.py through the buffer-contract protocol (hostile buffers, B == A),
the fused targets against the composed fp32 route (labels bit for bit) and the float64 restatement, the detection front
and the whole get_bboxes fused against composed, the bilinear merge against float64 / autograd / its adjoint, the FPN and
the detector fused against composed, and a Runner on the named config.

Bounds.  Encode, decode and gt preparation are float64 arithmetic rounded once: one fp32 spacing of the float64 value.
The bilinear bounds k * 2^-24 * max|input| are derived in retina_cases.bilinear_k (forward k = 12, backward
k = n (n + 7) for a pre-image of n addends).  The detector's fused-against-composed bound is measured, not fixed: the
composed fp32 route against its own float64 run on the same inputs gives the error E of fp32 arithmetic on this model;
the fused route may be 2 E from that float64 run and 2 E from the composed route (the figures are printed;
profiles/retinanet_notes.md records them and why the two routes share one forward pass)."""
import copy

import numpy as np
import pytest
import torch

from tests import guarded, retina_cases
from tests import retina_ref as R

pytestmark = pytest.mark.gpu

CASES = retina_cases.all_cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_buffer_contract_and_reference(case, dev):
    print(guarded.run_case(case.entry_points[0], case.label, case.fn, dev))


def _head(dev, **kw):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.config import named
    from jdet_amd.utils.registry import HEADS, build_from_cfg
    cfg = dict(copy.deepcopy(named.RETINANET_V1D_DOTA_CFG["model"]["rpn_net"]), **kw)
    return build_from_cfg(cfg, HEADS).to(dev)


# ------------------------------------------------------------------------------------------------------------ targets
@pytest.mark.parametrize("tie", [False, True])
def test_fused_targets_equal_the_composed_route_and_the_restatement(tie, dev):
    from jdet_amd.ops import retina
    f = R.batch(tie)
    head = _head(dev)
    anchors = torch.from_numpy(R.anchors()).to(dev)
    targets = [dict(rboxes=torch.from_numpy(r).to(dev), labels=torch.from_numpy(l).to(dev))
               for r, l in zip(f["raws"], f["labels"])]
    rb, rh = retina.gt_prepare(torch.cat([t["rboxes"] for t in targets]))
    assert (np.abs(rb.cpu().double().numpy() - np.concatenate([R.gt_prepare(r)[0] for r in f["raws"]])) <=
            R.spacing(f["rboxes"])).all()
    t = retina.targets(anchors, rb, rh, torch.cat([x["labels"] for x in targets]),
                       torch.from_numpy(f["offsets"]).to(dev), R.POS, R.NEG_HI, R.NEG_LO)
    composed = head.composed_targets(anchors, targets)                  # fp32 tensor program on the device
    raw = t["raw_labels"].cpu().numpy()
    for i, (loc, lab) in enumerate(composed):
        assert np.array_equal(raw[i], lab.cpu().numpy()), "image %d: fused labels differ from the composed route" % i
        assert np.array_equal(raw[i], f["raw_labels"][i])
        for got in (t["loc_targets"][i], loc):
            assert (np.abs(got.cpu().double().numpy() - f["loc"][i]) <= R.spacing(f["loc"][i])).all(), i
    assert np.array_equal(t["normalizer"].cpu().numpy(), f["normalizer"].astype(np.float32))
    assert np.array_equal(t["labels"].cpu().numpy(), np.maximum(raw, 0))
    assert np.array_equal(t["label_weights"].cpu().numpy(), (raw >= 0).astype(np.float32))
    assert np.array_equal(t["loc_weights"].cpu().numpy(), np.repeat((raw > 0).astype(np.float32)[..., None], 5, -1))
    assert (raw[0] == 0).all() and t["normalizer"][0] == 1                       # the image without gts
    if tie:
        assert np.array_equal(raw, R.batch(False)["raw_labels"])                # the duplicate (gt 70) never wins gt 5


# ------------------------------------------------------------------------------------------------------------- detect
@pytest.mark.parametrize("nms_pre,max_dets", [(1000, 10000), (20, 10000), (1000, 50)])
def test_get_bboxes_fused_equals_composed(nms_pre, max_dets, dev, monkeypatch):
    f = R.detect_fixture()
    head = _head(dev, nms_pre=nms_pre, max_dets=max_dets).eval()
    anchors = torch.from_numpy(R.anchors()).to(dev)
    loc, logits = torch.from_numpy(f["loc"]).to(dev)[None], torch.from_numpy(f["logits"]).to(dev)[None]
    meta = [dict(img_size=(128, 128), ori_img_size=(256, 256))]
    d = R.detect(R.anchors(), f["loc"], f["logits"], f["thr"])
    assert (d["counts"] > 20).all()                                     # nms_pre = 20 cuts every class
    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("JDET_RETINA_FUSED", fused)
        out[fused] = head.get_bboxes(anchors, loc, logits, meta)[0]
    (pf, sf, lf), (pc, sc, lc) = out["1"], out["0"]
    assert pf.shape == pc.shape and pf.shape[1] == 8 and 0 < pf.shape[0] <= max_dets
    assert torch.equal(lf, lc) and lf.dtype == torch.int32
    assert (sf - sc).abs().max() <= float(R.spacing(1.0)) and bool((sf > f["thr"]).all())
    # polygons are fp32 functions of boxes that agree within one spacing: a few spacings of the largest coordinate
    assert float((pf - pc).abs().max()) <= 8 * float(R.spacing(float(pc.abs().max())))


# ---------------------------------------------------------------------------------------------------- bilinear merge
@pytest.mark.parametrize("shape", retina_cases.BILINEAR_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_bilinear_backward_against_autograd_and_the_adjoint(shape, dev):
    from jdet_amd.ops import upsample_add as UA
    N, C, H, W, Ht, Wt, div = shape
    torch.manual_seed(H * 100 + W)
    cl = torch.channels_last
    lat = torch.randn(N, C, H, W, device=dev).contiguous(memory_format=cl).requires_grad_(True)
    top = torch.randn(N, C, Ht, Wt, device=dev).contiguous(memory_format=cl).requires_grad_(True)
    g = torch.randn(N, C, H, W, device=dev).contiguous(memory_format=cl)
    assert UA.fusable(lat, top)
    out = UA.upsample_add_bilinear(lat, top, div)
    out.backward(g)
    lat64, top64 = lat.detach().double().requires_grad_(True), top.detach().double().requires_grad_(True)
    out64 = UA.upsample_add_bilinear_composed(lat64, top64, div)
    out64.backward(g.double())
    m = max(float(lat.abs().max()), float(top.abs().max()))
    u = 2.0 ** -24
    kf, kb = retina_cases.bilinear_k(shape, False), retina_cases.bilinear_k(shape, True)
    assert float((out.double() - out64).abs().max()) <= kf * u * m
    assert float((top.grad.double() - top64.grad).abs().max()) <= kb * u * float(g.abs().max())
    assert torch.equal(lat.grad, g / div)
    # <resize(t), g> = <t, resize^T(g)>, in float64 from the kernel's two outputs (lateral 0, div 1)
    t2 = top.detach().clone().requires_grad_(True)
    fwd = UA.upsample_add_bilinear(torch.zeros_like(lat), t2, 1.0)
    fwd.backward(g)
    lhs, rhs = float((fwd.double() * g.double()).sum()), float((t2.detach().double() * t2.grad.double()).sum())
    terms = N * C * H * W
    assert abs(lhs - rhs) <= (kf + kb) * u * terms * m * float(g.abs().max())


def _r18_model(dev):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.config import named
    from jdet_amd.utils.registry import MODELS, build_from_cfg
    cfg = copy.deepcopy(named.RETINANET_V1D_DOTA_CFG["model"])
    cfg["backbone"]["type"] = "Resnet18_v1d"
    cfg["neck"]["in_channels"] = [64, 128, 256, 512]
    torch.manual_seed(0)
    model = build_from_cfg(cfg, MODELS).to(dev)
    for p in model.parameters():
        if p.dim() == 4 and p.shape[2] * p.shape[3] > 1:
            p.data = p.data.contiguous(memory_format=torch.channels_last)
    return model


def test_fpn_fused_equals_composed_on_backbone_features(dev, monkeypatch):
    from jdet_amd.ops import upsample_add as UA
    model = _r18_model(dev).train()
    # (the v1d downsample is an average pool of the stride: every stage halves exactly, so the merges here are exact 2x;
    # other ratios are rows of retina_cases)
    x = torch.randn(2, 3, 128, 96, device=dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        feats = model.backbone(x)
        assert [tuple(f.shape[2:]) for f in feats] == [(32, 24), (16, 12), (8, 6), (4, 3)]
        neck = model.neck
        laterals = [conv(feats[neck.start_level + k]) for k, conv in enumerate(neck.lateral_convs)]
        assert all(UA.fusable(a, b) for a, b in zip(laterals, laterals[1:]))
        fused = neck._top_down(laterals)
        monkeypatch.setattr(UA, "fusable", lambda a, b: False)
        composed = neck._top_down(laterals)
        outs = neck(feats)
    assert [tuple(o.shape[2:]) for o in outs] == [(16, 12), (8, 6), (4, 3), (2, 2), (1, 1)]
    # one merge is within 12 u m of float64 (retina_cases.bilinear_k), so two routes differ by at most 24 u m; the level
    # below takes the merged map (halved) and adds a merge of its own: 36 u m covers both levels
    m = max(float(x.abs().max()) for x in laterals)
    assert torch.equal(fused[-1], composed[-1])
    for a, b in zip(fused[:-1], composed[:-1]):
        assert float((a - b).abs().max()) <= 36 * 2.0 ** -24 * m


def test_resnet50_v1d_on_the_device_against_float64(dev):
    """the bottleneck net: a stage's first block (pooled downsample) runs per layer, the others on the fused conv family;
    the forward against the same net in float64, and a backward that reaches every parameter.  Bound: 53 layers, each within a few fp32
    roundings of its input's scale -- 53 * 16 * 2^-24 of the largest value"""
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils.registry import BACKBONES, build_from_cfg
    torch.manual_seed(0)
    net = build_from_cfg(dict(type="Resnet50_v1d", return_stages=["layer1", "layer2", "layer3", "layer4"]),
                         BACKBONES).to(dev).train()
    for p in net.parameters():
        if p.dim() == 4 and p.shape[2] * p.shape[3] > 1:
            p.data = p.data.contiguous(memory_format=torch.channels_last)
    net64 = copy.deepcopy(net).double()
    x = torch.randn(2, 3, 64, 64, device=dev).contiguous(memory_format=torch.channels_last)
    outs, outs64 = net(x), net64(x.double())
    bound = 53 * 16 * 2.0 ** -24
    assert [tuple(o.shape[1:]) for o in outs] == [(256, 16, 16), (512, 8, 8), (1024, 4, 4), (2048, 2, 2)]
    for a, b in zip(outs, outs64):
        assert float((a.double() - b).abs().max()) <= bound * float(b.abs().max())
    sum(o.square().mean() for o in outs).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


# ----------------------------------------------------------------------------------------------------------- detector
def _step(model, images, targets):
    model.zero_grad(set_to_none=True)
    losses = model(images, targets)
    (losses["roi_cls_loss"] + losses["roi_loc_loss"]).backward()
    grads = {n: p.grad.detach().double().clone() for n, p in model.named_parameters() if p.grad is not None}
    return {k: float(v) for k, v in losses.items()}, grads


def _rel_err(a, b):
    """max over parameters of max|a - b| / max|b|"""
    return max(float((a[n] - b[n]).abs().max()) / max(float(b[n].abs().max()), 1e-30) for n in b)


def _grads(model, losses):
    model.zero_grad(set_to_none=True)
    (losses["roi_cls_loss"] + losses["roi_loc_loss"]).backward(retain_graph=True)
    return ({k: float(v.detach()) for k, v in losses.items()},
            {n: p.grad.detach().double().clone() for n, p in model.named_parameters() if p.grad is not None})


def test_detector_train_step_fused_equals_composed(dev, monkeypatch):
    """A train step of the detector from the same weights on both head routes: equal losses and gradients.

    Bound (no number is fixed): E = the composed fp32 route against its own float64 run, as the max over parameters of
    max|difference| / max|gradient|; the fused route may be 2 E from that float64 run and 2 E from the composed route,
    and likewise for the two losses (a loss within one fp32 spacing of float64 has no error to double: 2^-23 is the
    floor).

    Both routes are evaluated on ONE forward pass (`RetinaHead.predict`, then `RetinaHead.loss` per route, each with
    its own backward through the whole model).  The reason is measured: the forward of this model differs from run to
    run in its last bits (the library convolutions of the backbone), and on these inputs one ReLU input of the
    regression tower lies within that rounding of zero.  Whether its mask comes out 0 or 1 moves that channel's
    gradient, and every gradient below it, by 1.4e-3 of its largest element -- on either route, and float64 takes the
    one side.  Two separate forwards therefore compare the routes across a discontinuity that belongs to neither
    (profiles/retinanet_notes.md); one forward gives both routes the same masks."""
    from jdet_amd.runner import synthetic_batch
    model = _r18_model(dev).train()
    images, targets = synthetic_batch(2, 128, dev, seed=3, num_gts=8)
    images = images.contiguous(memory_format=torch.channels_last)
    model64 = copy.deepcopy(model).double()
    head = model.rpn_net
    pred = head.predict(model.neck(model.backbone(images)))
    monkeypatch.setenv("JDET_RETINA_FUSED", "1")
    assert head._fused_route(pred[1])
    lf, gf = _grads(model, head.loss(*pred, targets))
    monkeypatch.setenv("JDET_RETINA_FUSED", "0")
    assert not head._fused_route(pred[1])
    lc, gc = _grads(model, head.loss(*pred, targets))
    l64, g64 = _step(model64, images.double(), targets)
    assert set(gf) == set(gc) == set(g64) == {n for n, p in model.named_parameters() if p.requires_grad}
    e_comp, e_fused, e_routes = _rel_err(gc, g64), _rel_err(gf, g64), _rel_err(gf, gc)
    l_comp = max(abs(lc[k] - l64[k]) / abs(l64[k]) for k in l64)
    l_fused = max(abs(lf[k] - l64[k]) / abs(l64[k]) for k in l64)
    print("detector 2x128x128 Resnet18_v1d against its float64 run: composed grad %.3e loss %.3e; fused grad %.3e "
          "loss %.3e; fused against composed grad %.3e" % (e_comp, l_comp, e_fused, l_fused, e_routes))
    assert all(np.isfinite(v) and v > 0 for v in lf.values())
    assert e_fused <= 2 * e_comp and e_routes <= 2 * e_comp
    assert l_fused <= 2 * max(l_comp, 2.0 ** -23)


def test_runner_takes_two_steps_on_the_named_config(dev):
    from jdet_amd.config import named
    from jdet_amd.runner import Runner, synthetic_batch
    cfg = copy.deepcopy(named.RETINANET_V1D_DOTA_CFG)
    cfg["model"]["backbone"]["type"] = "Resnet18_v1d"
    cfg["model"]["neck"]["in_channels"] = [64, 128, 256, 512]
    torch.manual_seed(0)
    runner = Runner(cfg, device=dev, conv_autotune=False)
    assert type(runner.optimizer).__name__ == "GradMutilpySGD"
    images, targets = synthetic_batch(2, 128, dev, seed=1, num_gts=8)
    l1, parts = runner.train_step(images, targets)
    l2, _ = runner.train_step(images, targets)
    assert set(parts) == {"roi_cls_loss", "roi_loc_loss"}
    assert torch.isfinite(l1) and torch.isfinite(l2) and float(l1) != float(l2)
