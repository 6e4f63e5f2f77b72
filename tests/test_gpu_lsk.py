"""GPU: the depthwise-convolution and kernel-selection kernels (csrc/dwconv.hip, csrc/lsk_select.hip) against the
restatements of tests/lsk_ref.py on the buffer-contract harness (tests/guarded.py: guard bands, poisoned outputs and
workspace, inputs unchanged, run B == run A bit for bit, a short workspace refused); the autograd nodes against the direct
ABI calls; the LSKNet_t backbone against float64; LSKNET_S_ORCNN_CFG (LSKNet_t widths) through Runner.

Bounds are those of tests/lsk_cases.py.  act 0 forward and the data gradient are bit-exact pins.

GELU allowance.  No documented ulp error of the device erff is on the machines, so the allowance is 4 x the error of the
framework's own float32 GELU against float64 on the same pre-activations, measured when the reference is evaluated and
printed by the test (profiles/lsk.md records the figures of one run).  Measured on an MI355X (shapes d / a / c): the
framework's forward error 4.27e-7 / 1.51e-7 / 4.25e-7, its backward error 1.29e-7 / 1.06e-7 / 1.18e-7; the largest
bound any element was given 7.6e-6 / 1.9e-5 / 3.0e-5 forward and 1.7e-5 / 3.7e-5 / 6.9e-5 backward; the kernels' own
errors 6.4e-7 / 3.3e-7 / 1.0e-6 forward and 1.1e-7 / 3.8e-8 / 6.2e-7 backward.

Backbone.  Per stage output, the HIP routes may show 4 x the max error against float64 that the library float32 route
alone shows on the same input and weights; both are printed."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lsk_cases as C
from tests import lsk_ref as R

pytestmark = pytest.mark.gpu

DW_CASES = C.dw_cases()
SELECT_CASES = C.select_cases()


def _dev(a, dev):
    return torch.tensor(np.asarray(a), device=dev)


def _nchw(a, dev):
    """(N, H, W, C) array -> channels-last (N, C, H, W) device tensor over the same memory order"""
    return _dev(a, dev).permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", DW_CASES, ids=[c.id for c in DW_CASES])
def test_dwconv_contract(dev, case):
    from tests import guarded
    C.MEASURED.clear()
    guarded.run_case(case.entry_points[-1], case.label, case.fn, dev)
    for k, v in C.MEASURED.items():
        if k[2] == "cuda":
            print("%s %s: framework float32 GELU error %.3e, largest bound %.3e" % (k[0], k[1], v[0], v[1]))


@pytest.mark.parametrize("case", SELECT_CASES, ids=[c.id for c in SELECT_CASES])
def test_selection_contract(dev, case):
    from tests import guarded
    guarded.run_case(case.entry_points[0], case.label, case.fn, dev)


# ------------------------------------------------------------------------------------------------------------ the nodes
@pytest.mark.parametrize("key,act", [("e", None), ("d", "gelu"), ("a", "gelu"), ("f", None)])
def test_dwconv_node_equals_the_direct_calls(dev, key, act, monkeypatch):
    from jdet_amd.ops import dwconv as D
    monkeypatch.setattr(D, "ENABLED", True)
    monkeypatch.setattr(D, "LARGE_TAPS_MIN_POSITIONS", 0)      # the 7x7 on these small maps too
    f = C.dw_fixture(key, with_bias=act is not None)
    x = _nchw(f["x"], dev).requires_grad_(True)
    g = _nchw(f["g"], dev)
    weight = _dev(f["w"], dev).permute(2, 0, 1).unsqueeze(1).contiguous().requires_grad_(True)
    bias = None if f["bias"] is None else _dev(f["bias"], dev).requires_grad_(True)
    assert D.fusable(x, weight, bias, f["pad"], f["dil"])
    y = D.dwconv(x, weight, bias, f["pad"], f["dil"], act)
    assert y.is_contiguous(memory_format=torch.channels_last) and type(y.grad_fn).__name__ == "_DWConvBackward"
    y.backward(g)
    # the same through the ABI, call by call
    wp, wf = _dev(f["w"], dev), _dev(R.flip_taps(f["w"]), dev)
    xd = x.detach()
    y2 = D.dwconv_nhwc(xd, wp, None if bias is None else bias.detach(), f["geom"], 1 if act else 0)
    gz = D.dwconv_gelu_backward_nhwc(xd, wp, bias.detach(), g, f["geom"]) if act else g
    gx2 = D.dwconv_nhwc(gz, wf, None, f["geom"], 0)
    gw2, gb2 = D.dwconv_wgrad_nhwc(xd, gz, f["geom"], bias is not None)
    assert torch.equal(y, y2) and torch.equal(x.grad, gx2)
    assert torch.equal(weight.grad[:, 0].permute(1, 2, 0), gw2)
    assert bias is None or torch.equal(bias.grad, gb2)
    # and against float64 autograd of the composed form, loosely: the routes wire the right tensors together
    x64, w64 = x.detach().double().cpu().requires_grad_(True), weight.detach().double().cpu().requires_grad_(True)
    b64 = None if bias is None else bias.detach().double().cpu().requires_grad_(True)
    D.dwconv_composed(x64, w64, b64, f["pad"], f["dil"], act).backward(g.double().cpu())
    for got, want in ((x.grad, x64.grad), (weight.grad, w64.grad)) + (() if bias is None else ((bias.grad, b64.grad),)):
        assert float((got.double().cpu() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))


def test_dwconv_takes_the_composed_form_where_it_is_not_fusable(dev, monkeypatch):
    from jdet_amd.ops import dwconv as D
    monkeypatch.setattr(D, "ENABLED", True)
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(6, 6, 5, padding=2, groups=6).to(dev)
    x = torch.randn(2, 6, 9, 11, device=dev).contiguous(memory_format=torch.channels_last)
    assert not D.fusable(x, conv.weight, conv.bias, conv.padding, conv.dilation)             # C = 6
    assert torch.equal(D.dwconv(x, conv.weight, conv.bias, conv.padding, conv.dilation), conv(x))
    conv8 = torch.nn.Conv2d(8, 8, 5, padding=2, groups=8).to(dev)
    x8 = torch.randn(2, 8, 9, 11, device=dev)
    assert not D.fusable(x8, conv8.weight, conv8.bias, 2, 1)                                 # not channels-last
    assert D.fusable(x8.contiguous(memory_format=torch.channels_last), conv8.weight, conv8.bias, 2, 1)
    assert not D.fusable(x8.contiguous(memory_format=torch.channels_last), conv8.weight, conv8.bias, 1, 1)    # not "same"
    assert not D.fusable(x8.contiguous(memory_format=torch.channels_last), conv8.weight, conv8.bias, 2, 1, stride=2)
    # more than 25 taps on a small map: the library is the measured faster choice (profiles/lsk.md)
    w7 = torch.randn(8, 1, 7, 7, device=dev)
    xc = x8.contiguous(memory_format=torch.channels_last)
    assert D.fusable(xc, w7, None, 9, 3) and not D.preferred(xc, w7) and D.preferred(xc, conv8.weight)
    assert D.preferred(torch.empty(2, 8, 64, 32, device=dev), w7) and D.LARGE_TAPS_MIN_POSITIONS == 4096
    assert torch.equal(D.dwconv(xc, w7, None, 9, 3), F.conv2d(xc, w7, None, 1, 9, 3, groups=8))
    monkeypatch.setattr(D, "ENABLED", False)
    assert torch.equal(D.dwconv(xc, conv8.weight, conv8.bias, 2, 1, "gelu"), F.gelu(conv8(xc)))


@pytest.mark.parametrize("ch,tied", [(16, False), (160, False), (16, True)])
def test_selection_nodes_equal_the_direct_calls_and_torch_max(dev, ch, tied, monkeypatch):
    """autograd through lsk_squeeze / lsk_select equals the ABI calls bit for bit; on tied maxima the gradient goes to the
    FIRST index, as torch.max(dim=1) autograd sends it (float64 on the CPU)"""
    from jdet_amd import _lib as L
    from jdet_amd.ops import lsk_select as S
    monkeypatch.setattr(S, "ENABLED", True)
    f = C.select_fixture(ch, tied)
    N, H, W = C.SELECT_MAP
    a1, a2 = (_nchw(f[k], dev).requires_grad_(True) for k in ("a1", "a2"))
    sig = _nchw(f["sig"], dev).requires_grad_(True)
    g_agg, g = _nchw(f["g_agg"], dev), _nchw(f["g"], dev)
    assert S.fusable(a1, a2) and S.fusable(a1, a2, sig)
    agg = S.lsk_squeeze(a1, a2)
    assert type(agg.grad_fn).__name__ == "_LskSqueezeBackward" and agg.shape == (N, 2, H, W)
    agg.backward(g_agg)
    mean, mag, mx, idx = R.squeeze(f["a1"], f["a2"])
    assert np.array_equal(agg.detach()[:, 1].cpu().numpy(), mx)
    assert (np.abs(agg.detach()[:, 0].double().cpu().numpy() - mean) <= R.gamma(2 * ch + 1) * mag).all()
    # direct: forward, then the accumulating backward onto zeros
    agg2 = torch.empty_like(agg)
    am = torch.empty((N * H * W,), dtype=torch.int32, device=dev)
    L.check(L.lib().jdet_lsk_squeeze_forward(L.ptr(a1), L.ptr(a2), N, H, W, ch, L.ptr(agg2), L.ptr(am), L.stream_ptr(a1)), "")
    z1, z2 = (torch.zeros_like(a1, memory_format=torch.channels_last) for _ in range(2))
    L.check(L.lib().jdet_lsk_squeeze_backward(L.ptr(g_agg.contiguous(memory_format=torch.channels_last)), L.ptr(am), N, H, W,
                                              ch, L.ptr(z1), L.ptr(z2), L.stream_ptr(a1)), "")
    assert torch.equal(agg, agg2) and np.array_equal(am.cpu().numpy(), idx.reshape(-1))
    assert torch.equal(a1.grad, z1) and torch.equal(a2.grad, z2)
    # torch.max(dim=1) autograd in float64: the first index takes g_max
    c1, c2 = (torch.tensor(f[k]).double().permute(0, 3, 1, 2).requires_grad_(True) for k in ("a1", "a2"))
    S.lsk_squeeze_composed(c1, c2).backward(torch.tensor(f["g_agg"]).double().permute(0, 3, 1, 2))
    assert R.has_ties(f["a1"], f["a2"]).any() == tied
    _, _, m1, m2 = R.squeeze_backward64(f["g_agg"], idx, ch)          # |g_mean| / (2 Ch) + |g_max| at the argmax
    for got, want, mag in ((a1.grad, c1.grad, m1), (a2.grad, c2.grad, m2)):
        err = (got.double().cpu() - want).abs().permute(0, 2, 3, 1).numpy()
        assert (err <= 3 * R.U32 * mag).all()
    # select
    a1.grad = a2.grad = None
    out = S.lsk_select(a1, a2, sig)
    assert type(out.grad_fn).__name__ == "_LskSelectBackward"
    out.backward(g)
    assert np.array_equal(out.detach().permute(0, 2, 3, 1).cpu().numpy(), R.select_f32(f["a1"], f["a2"], f["sig"]))
    r1, r2, rs, smag = R.select_backward(f["g"], f["a1"], f["a2"], f["sig"])
    assert np.array_equal(a1.grad.permute(0, 2, 3, 1).cpu().numpy(), r1)
    assert np.array_equal(a2.grad.permute(0, 2, 3, 1).cpu().numpy(), r2)
    assert (np.abs(sig.grad.permute(0, 2, 3, 1).double().cpu().numpy() - rs) <= R.gamma(ch + 1) * smag).all()
    # not fusable: Ch = 6, and the composed result exactly
    b1, b2, s6 = (torch.randn(2, c, 3, 5, device=dev).contiguous(memory_format=torch.channels_last) for c in (6, 6, 2))
    assert not S.fusable(b1, b2) and torch.equal(S.lsk_select(b1, b2, s6), S.lsk_select_composed(b1, b2, s6))
    assert torch.equal(S.lsk_squeeze(b1, b2), S.lsk_squeeze_composed(b1, b2))


# ------------------------------------------------------------------------------------------------------------- backbone
def _stage_errors(outs, ref):
    return [float((o.double().cpu() - r).abs().max()) for o, r in zip(outs, ref)]


def test_backbone_against_float64(dev, monkeypatch):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.ops import dwconv as D, lsk_select as S
    from jdet_amd.utils.registry import BACKBONES, build_from_cfg
    torch.manual_seed(0)
    m = build_from_cfg(dict(type="LSKNet_t", out_indices=(0, 1, 2, 3)), BACKBONES).train()
    x = torch.randn(2, 3, 64, 64)
    m64 = copy.deepcopy(m).double()
    ref = [o.detach() for o in m64(x.double())]
    m = m.to(dev)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    monkeypatch.setattr(D, "LARGE_TAPS_MIN_POSITIONS", 0)      # every route on: the 7x7 dilation-3 on these small maps too
    routes = []
    real_dw, real_sq, real_sel = D._DWConv.apply, S._LskSqueeze.apply, S._LskSelect.apply
    errs = {}
    for on in (False, True):
        monkeypatch.setattr(D, "ENABLED", on)
        monkeypatch.setattr(S, "ENABLED", on)
        if on:
            monkeypatch.setattr(D._DWConv, "apply", lambda *a: (routes.append("dw"), real_dw(*a))[1])
            monkeypatch.setattr(S._LskSqueeze, "apply", lambda *a: (routes.append("sq"), real_sq(*a))[1])
            monkeypatch.setattr(S._LskSelect, "apply", lambda *a: (routes.append("sel"), real_sel(*a))[1])
        m.zero_grad(set_to_none=True)
        outs = m(xd)
        errs[on] = _stage_errors(outs, ref)
        assert all(o.is_contiguous(memory_format=torch.channels_last) for o in outs)
        if on:
            sum((o * o).sum() for o in outs).backward()
    blocks = 3 + 3 + 5 + 2
    assert routes.count("dw") == 3 * blocks and routes.count("sq") == blocks and routes.count("sel") == blocks
    for i, (lib_e, hip_e) in enumerate(zip(errs[False], errs[True])):
        print("LSKNet_t stage %d: max error against float64, library float32 route %.3e, HIP routes %.3e (bound %.3e)"
              % (i + 1, lib_e, hip_e, 4 * lib_e))
        assert hip_e <= 4 * lib_e, i
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


# ------------------------------------------------------------------------------------------------------------- detector
def test_detector_trains_and_infers_through_runner(dev, monkeypatch):
    from jdet_amd.config.named import LSKNET_S_ORCNN_CFG
    from jdet_amd.ops import dwconv as D, lsk_select as S
    from jdet_amd.runner import Runner, synthetic_batch
    monkeypatch.setattr(D, "ENABLED", True)
    monkeypatch.setattr(S, "ENABLED", True)
    cfg = copy.deepcopy(LSKNET_S_ORCNN_CFG)
    cfg["model"]["backbone"]["type"] = "LSKNet_t"
    cfg["model"]["neck"]["in_channels"] = [32, 64, 160, 256]
    images, targets = synthetic_batch(1, 128, dev, seed=3, num_gts=6)
    torch.manual_seed(0)
    r = Runner(cfg, device=dev, conv_autotune=False, graph=False)
    assert type(r.model.backbone).__name__ == "LSKNet"and cfg["optimizer"]["type"] == "AdamW"
    before = r.model.backbone.block1[0].layer_scale_1.detach().clone()
    loss, parts = r.train_step(images, targets)
    assert bool(torch.isfinite(loss)) and set(parts) == {"loss_cls", "orcnn_bbox_loss", "loss_rpn_cls", "loss_rpn_bbox"}
    loss2, _ = r.train_step(images, targets)
    assert bool(torch.isfinite(loss2))
    assert not torch.equal(r.model.backbone.block1[0].layer_scale_1.detach(), before)
    m = r.model.eval()
    with torch.no_grad():
        feats = m.neck(m.backbone(images.contiguous(memory_format=torch.channels_last)))
        tables, losses = m.rpn(feats, targets)
        res = m(images.contiguous(memory_format=torch.channels_last), targets)
    nms_post = cfg["model"]["rpn"]["nms_post"]
    assert losses == {} and len(tables) == 1
    for tab in tables:                                       # the proposal-table contract of OrientedRPNHead
        assert tab.shape == (nms_post, 6)
        s = tab[:, 5]
        n = int((s >= 0).sum())
        assert 0 < n <= nms_post and bool((s[:n] >= 0).all()) and not bool((s[n:] >= 0).any())
        assert bool((s[:n - 1] >= s[1:n]).all()) and bool(torch.isfinite(tab[:n]).all())
    assert len(res) == 1
    polys, scores, labels = res[0]
    assert polys.shape[1] == 8 and polys.shape[0] == scores.shape[0] == labels.shape[0]
    assert bool(torch.isfinite(polys).all()) and bool(torch.isfinite(scores).all())
