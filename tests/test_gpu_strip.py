"""GPU: the rolling-window strip-convolution kernel (csrc/strip_conv.hip) on the buffer-contract harness
(tests/guarded.py: guard bands, poisoned outputs, inputs unchanged, run B == run A bit for bit) against the float32
restatement of its stated order, and bit for bit against the generic depthwise kernel it shares that order with; the
autograd node against the direct ABI calls; the fallbacks; the StripNet_T backbone against float64; STRIP_RCNN_S_CFG
(StripNet_T widths) through Runner.

Every kernel bound is equality (tests/strip_cases.py).  Backbone: per stage output, the HIP routes may show 4 x the max
error against float64 that the library float32 route alone shows on the same input and weights; both are printed."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import strip_cases as C

pytestmark = pytest.mark.gpu

CASES = C.strip_cases()


def _dev(a, dev):
    return torch.tensor(np.ascontiguousarray(a), device=dev)


def _nchw(a, dev):
    """(N, H, W, C) array -> channels-last (N, C, H, W) device tensor over the same memory order"""
    return _dev(a, dev).permute(0, 3, 1, 2)


def _weight(f, dev):
    """the fixture's (K, C) taps as a depthwise nn.Conv2d weight (C, 1, K, 1) or (C, 1, 1, K)"""
    K, C_ = f["w"].shape
    return _dev(f["w"], dev).t().reshape((C_, 1, K, 1) if f["axis"] == 0 else (C_, 1, 1, K)).contiguous()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_strip_conv_contract(dev, case):
    from tests import guarded
    guarded.run_case(case.entry_points[0], case.label, case.fn, dev)


@pytest.mark.parametrize("axis", C.AXES)
@pytest.mark.parametrize("shape", [(2, 64, 40, 44, 19), (1, 320, 24, 24, 19)], ids=["2x64x40x44", "1x320x24x24"])
def test_bit_equal_to_the_generic_depthwise_kernel(dev, shape, axis):
    """many workgroups, interior and border windows, with a bias: jdet_strip_conv_forward == jdet_dwconv_nhwc_forward"""
    from jdet_amd.ops import dwconv as D, strip_conv as S
    N, C_, H, W, K = shape
    g = torch.Generator().manual_seed(N * C_ + axis)
    x = torch.randn((N, H, W, C_), generator=g).to(dev).permute(0, 3, 1, 2)
    w = (torch.randn((K, C_), generator=g) * 0.5).to(dev)
    b = torch.randn((C_,), generator=g).to(dev)
    geom = (N, H, W, C_, K)
    got = S.strip_conv_nhwc(x, w, b, geom, axis)
    want = D.dwconv_nhwc(x, w.reshape((K, 1, C_) if axis == 0 else (1, K, C_)), b, S._dw_geometry(geom, axis), 0)
    assert got.is_contiguous(memory_format=torch.channels_last) and torch.equal(got, want)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 1.0


# ------------------------------------------------------------------------------------------------------------- the node
@pytest.mark.parametrize("key,axis", [("a", 1), ("a", 0), ("g", 1), ("d", 0), ("e", 1)])
def test_strip_node_equals_the_direct_calls(dev, key, axis, monkeypatch):
    from jdet_amd.ops import dwconv as D, strip_conv as S
    monkeypatch.setattr(S, "ENABLED", True)
    monkeypatch.setattr(S, "preferred", lambda x, w: True)
    f = C.strip_fixture(key, axis)
    x = _nchw(f["x"], dev).requires_grad_(True)
    g = _nchw(f["g"], dev)
    weight = _weight(f, dev).requires_grad_(True)
    bias = None if f["bias"] is None else _dev(f["bias"], dev).requires_grad_(True)
    assert S.fusable(x, weight, bias, f["pad"])
    y = S.strip_conv(x, weight, bias, f["pad"])
    assert y.is_contiguous(memory_format=torch.channels_last) and type(y.grad_fn).__name__ == "_StripConvBackward"
    y.backward(g)
    # the same through the ABI, call by call
    xd = x.detach()
    y2 = S.strip_conv_nhwc(xd, _dev(f["w"], dev), None if bias is None else bias.detach(), f["geom"], axis)
    gx2 = S.strip_conv_nhwc(g, _dev(C.flip_taps(f["w"]), dev), None, f["geom"], axis)
    gw2, gb2 = D.dwconv_wgrad_nhwc(xd, g, S._dw_geometry(f["geom"], axis), bias is not None)
    assert torch.equal(y, y2) and torch.equal(x.grad, gx2)
    assert np.array_equal(y.detach().permute(0, 2, 3, 1).cpu().numpy(), C.expected(f))
    assert np.array_equal(x.grad.permute(0, 2, 3, 1).cpu().numpy(), C.expected(f, flipped=True))
    assert torch.equal(weight.grad[:, 0].permute(1, 2, 0), gw2)
    assert bias is None or torch.equal(bias.grad, gb2)
    # and against float64 autograd of the composed form, loosely: the routes wire the right tensors together
    x64, w64 = x.detach().double().cpu().requires_grad_(True), weight.detach().double().cpu().requires_grad_(True)
    b64 = None if bias is None else bias.detach().double().cpu().requires_grad_(True)
    D.dwconv_composed(x64, w64, b64, f["pad"], 1).backward(g.double().cpu())
    for got, want in ((x.grad, x64.grad), (weight.grad, w64.grad)) + (() if bias is None else ((bias.grad, b64.grad),)):
        assert float((got.double().cpu() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))


def test_strip_conv_falls_back_to_dwconv(dev, monkeypatch):
    """not fusable (C = 6, not channels-last, an even K, dilation 2) or not enabled: exactly what ops.dwconv.dwconv gives"""
    from jdet_amd.ops import dwconv as D, strip_conv as S
    monkeypatch.setattr(S, "ENABLED", True)
    monkeypatch.setattr(S, "preferred", lambda x, w: True)
    nodes = []
    real = S._StripConv.apply
    monkeypatch.setattr(S._StripConv, "apply", lambda *a: (nodes.append(1), real(*a))[1])
    torch.manual_seed(0)

    def cl(t):
        return t.contiguous(memory_format=torch.channels_last)
    x6, w6 = cl(torch.randn(2, 6, 5, 21, device=dev)), torch.randn(6, 1, 1, 19, device=dev)
    assert not S.fusable(x6, w6, None, (0, 9))                                                   # C = 6
    assert torch.equal(S.strip_conv(x6, w6, None, (0, 9)), D.dwconv(x6, w6, None, (0, 9), 1))
    x8, w8, b8 = torch.randn(2, 8, 5, 21, device=dev), torch.randn(8, 1, 1, 19, device=dev), torch.randn(8, device=dev)
    assert not S.fusable(x8, w8, b8, (0, 9)) and S.fusable(cl(x8), w8, b8, (0, 9))              # not channels-last
    assert torch.equal(S.strip_conv(x8, w8, b8, (0, 9)), D.dwconv(x8, w8, b8, (0, 9), 1))
    we = torch.randn(8, 1, 1, 4, device=dev)
    assert not S.fusable(cl(x8), we, b8, (0, 2))                                                 # an even K
    assert torch.equal(S.strip_conv(cl(x8), we, b8, (0, 2)), F.conv2d(cl(x8), we, b8, 1, (0, 2), 1, groups=8))
    wd = torch.randn(8, 1, 7, 1, device=dev)
    assert D.fusable(cl(x8), wd, b8, (6, 0), 2) and not S.fusable(cl(x8), wd, b8, (6, 0), 2)    # dilation 2
    assert not S.fusable(cl(x8), torch.randn(8, 1, 3, 3, device=dev), b8, 1)                     # no strip
    assert not S.fusable(cl(x8), w8, b8, (0, 8)) and not S.fusable(cl(x8), w8, b8, (0, 9), stride=2)
    assert nodes == []
    y_on = S.strip_conv(cl(x8), w8, b8, (0, 9))
    assert nodes == [1]
    monkeypatch.setattr(S, "ENABLED", False)
    y_off = S.strip_conv(cl(x8), w8, b8, (0, 9))
    assert nodes == [1] and torch.equal(y_off, D.dwconv(cl(x8), w8, b8, (0, 9), 1))
    assert torch.equal(y_on, y_off)                                    # the two kernels share one order
    # the shipped rule (profiles/strip.md): small maps and 1 x K layers stay on the generic kernel, with the same result
    monkeypatch.undo()
    monkeypatch.setattr(S, "ENABLED", True)
    monkeypatch.setattr(S._StripConv, "apply", lambda *a: (nodes.append(2), real(*a))[1])
    assert not S.preferred(cl(x8), w8) and torch.equal(S.strip_conv(cl(x8), w8, b8, (0, 9)), y_on) and nodes == [1]
    xb, wb = cl(torch.randn(2, 8, 256, 256, device=dev)), torch.randn(8, 1, 19, 1, device=dev)
    assert S.preferred(xb, wb) and not S.preferred(xb, wb.permute(0, 1, 3, 2))
    yb = S.strip_conv(xb, wb, b8, (9, 0))
    assert nodes == [1, 2] and torch.equal(yb, D.dwconv(xb, wb, b8, (9, 0), 1))


# ------------------------------------------------------------------------------------------------------------- backbone
def _stage_errors(outs, ref):
    return [float((o.double().cpu() - r).abs().max()) for o, r in zip(outs, ref)]


def test_backbone_against_float64(dev, monkeypatch):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.ops import dwconv as D, strip_conv as S
    from jdet_amd.utils.registry import BACKBONES, build_from_cfg
    torch.manual_seed(0)
    m = build_from_cfg(dict(type="StripNet_T", out_indices=(0, 1, 2, 3)), BACKBONES).train()
    x = torch.randn(2, 3, 64, 64)
    m64 = copy.deepcopy(m).double()
    ref = [o.detach() for o in m64(x.double())]
    m = m.to(dev)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    monkeypatch.setattr(S, "preferred", lambda x, w: True)      # every route on: the strip kernel on these small maps too
    routes = []
    real_dw, real_st = D._DWConv.apply, S._StripConv.apply
    errs = {}
    for on in (False, True):
        monkeypatch.setattr(D, "ENABLED", on)
        monkeypatch.setattr(S, "ENABLED", on)
        if on:
            monkeypatch.setattr(D._DWConv, "apply", lambda *a: (routes.append("dw"), real_dw(*a))[1])
            monkeypatch.setattr(S._StripConv, "apply", lambda *a: (routes.append("strip"), real_st(*a))[1])
        m.zero_grad(set_to_none=True)
        outs = m(xd)
        errs[on] = _stage_errors(outs, ref)
        assert all(o.is_contiguous(memory_format=torch.channels_last) for o in outs)
        if on:
            sum((o * o).sum() for o in outs).backward()
    blocks = 3 + 3 + 5 + 2
    assert routes.count("strip") == 2 * blocks and routes.count("dw") == 2 * blocks
    for i, (lib_e, hip_e) in enumerate(zip(errs[False], errs[True])):
        print("StripNet_T stage %d: max error against float64, library float32 route %.3e, HIP routes %.3e (bound %.3e)"
              % (i + 1, lib_e, hip_e, 4 * lib_e))
        assert hip_e <= 4 * lib_e, i
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


# ------------------------------------------------------------------------------------------------------------- detector
def test_detector_trains_and_infers_through_runner(dev, monkeypatch):
    from jdet_amd.config.named import STRIP_RCNN_S_CFG
    from jdet_amd.ops import dwconv as D, strip_conv as S
    from jdet_amd.runner import Runner, synthetic_batch
    monkeypatch.setattr(D, "ENABLED", True)
    monkeypatch.setattr(S, "ENABLED", True)
    monkeypatch.setattr(S, "preferred", lambda x, w: True)
    cfg = copy.deepcopy(STRIP_RCNN_S_CFG)
    cfg["model"]["backbone"]["type"] = "StripNet_T"
    cfg["model"]["neck"]["in_channels"] = [32, 64, 160, 256]
    images, targets = synthetic_batch(1, 128, dev, seed=3, num_gts=6)
    torch.manual_seed(0)
    r = Runner(cfg, device=dev, conv_autotune=False, graph=False)
    assert type(r.model).__name__ == "StripRCNN" and type(r.model.backbone).__name__ == "StripNet"
    assert type(r.model.bbox_head).__name__ == "StripHead" and cfg["optimizer"]["type"] == "AdamW"
    before = r.model.backbone.block1[0].layer_scale_1.detach().clone()
    loss, parts = r.train_step(images, targets)
    assert bool(torch.isfinite(loss)) and set(parts) == {"loss_cls", "orcnn_bbox_loss", "loss_rpn_cls", "loss_rpn_bbox"}
    loss2, _ = r.train_step(images, targets)
    assert bool(torch.isfinite(loss2))
    assert not torch.equal(r.model.backbone.block1[0].layer_scale_1.detach(), before)
    m = r.model.eval()
    with torch.no_grad():
        res = m(images.contiguous(memory_format=torch.channels_last), targets)
    assert len(res) == 1
    polys, scores, labels = res[0]
    assert polys.shape[1] == 8 and polys.shape[0] == scores.shape[0] == labels.shape[0]
    assert bool(torch.isfinite(polys).all()) and bool(torch.isfinite(scores).all())
    assert labels.numel() == 0 or (int(labels.min()) >= 0 and int(labels.max()) < 15)
