"""CPU: the Strip R-CNN feature without a device -- the side header against STRIP_SIGNATURES and the exports; every
argument rule refused before any launch; the strip order of include/jdet_hip_strip.h restated as a windowed loop in
numpy float32 against tests/lsk_ref.dwconv_f32 (equality) and float64 F.conv2d(groups=C) (gamma(K + 1) * sum |terms|);
the dry run of the smallest cases; the composed route of the op; StripNet_T / StripNet_S parameter names and shapes
against the committed list, output shapes and strides, gradients to every parameter; StripHead's layers, its trunk
against a plain restatement of the reference's forward_single, and the class grouping of its regression output; the
named config against its golden YAML and the detector it builds."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lsk_ref as R
from tests import strip_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"jdet_strip_conv_forward"}


# ---------------------------------------------------------------------------------------------------------------- ABI
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|size_t)\s+(jdet_\w+)\s*\(([^)]*)\)\s*;", src):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
    return out


@pytest.fixture(scope="module")
def built():
    from jdet_amd import _lib
    _lib.build()
    return _lib


def test_header_table_and_exports_agree(built):
    d = _declared("jdet_hip_strip.h")
    assert set(d) == set(built.STRIP_SIGNATURES) == NAMES
    for other in (built.SIGNATURES, built.RETINA_SIGNATURES, built.CSL_SIGNATURES, built.LSK_SIGNATURES):
        assert not set(d) & set(other)
    # the other headers keep their symbol sets: nothing of the strip entry point went into them
    assert set(_declared("jdet_hip.h")) == set(built.SIGNATURES)
    assert set(_declared("jdet_hip_lsk.h")) == set(built.LSK_SIGNATURES) and len(built.LSK_SIGNATURES) == 8
    for header in ("jdet_hip.h", "jdet_hip_lsk.h"):
        assert "strip_conv" not in open(os.path.join(ROOT, "include", header)).read()
    raw = ctypes.CDLL(built.LIB_PATH)
    lib = built.lib()
    for name, nargs in d.items():
        res, args = built.STRIP_SIGNATURES[name]
        assert len(args) == nargs, name
        assert hasattr(raw, name), "missing export " + name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name


def test_argument_validation_returns_before_any_launch(built):
    """every answer comes from the host-side checks: no device here, and a launch on these addresses would not return"""
    lib = built.lib()
    N, X = None, 4096                                        # X: a 16-byte aligned non-null address nobody reads
    BAD, UNS = -1, -2

    def f(x=X, wp=X, b=N, n=2, h=8, w=8, c=8, k=19, axis=1, y=X):
        return lib.jdet_strip_conv_forward(x, wp, b, n, h, w, c, k, axis, y, N)

    for dim in ("n", "h", "w", "c", "k"):
        assert f(**{dim: 0}) == BAD and f(**{dim: -1}) == BAD, dim
    assert f(axis=2) == BAD and f(axis=-1) == BAD
    assert f(c=6) == UNS and f(c=2) == UNS and f(c=321) == UNS                           # C % 4
    assert f(k=2) == UNS and f(k=18) == UNS and f(k=1024) == UNS                         # an even K
    assert f(k=1025) == UNS and f(k=1023, x=N) == BAD                                    # K > 1023; 1023 passes to the next rule
    for axis in (0, 1):
        assert f(n=2 ** 13, h=2 ** 8, w=2 ** 8, c=4, x=X + 4, axis=axis) == UNS          # 2^31 elements
        assert f(n=2 ** 13 - 1, h=2 ** 8, w=2 ** 8, c=4, x=X + 4, axis=axis) == BAD      # one image fewer: the next rule
    assert f(x=N) == BAD and f(wp=N) == BAD and f(y=N) == BAD                            # null
    for off in (4, 8, 12):                                                               # not 16-byte aligned
        assert f(x=X + off) == BAD and f(wp=X + off) == BAD and f(b=X + off) == BAD and f(y=X + off) == BAD
    # the geometries of the cases are accepted up to the first pointer check
    for key in C.STRIP_SHAPES:
        for axis in C.AXES:
            g = C.strip_fixture(key, axis)["geom"]
            assert lib.jdet_strip_conv_forward(None, X, None, *g, axis, X, None) == BAD


# ------------------------------------------------------------------------------------------------------- restatements
def _windowed_f32(x, w, bias, axis):
    """the header's order, restated as the kernel's access pattern states it: four consecutive outputs of the strip axis
    walk their shared window of K + 3 inputs once; the value at window position j goes to output p through tap j - p"""
    x = np.moveaxis(np.asarray(x, np.float32), 1 + axis, 0)             # strip axis first: (L, ..., C)
    L, K = x.shape[0], w.shape[0]
    pad = (K - 1) // 2
    y = np.empty_like(x)
    for o0 in range(0, L, 4):
        acc = [np.zeros(x.shape[1:], np.float32) + (np.float32(0) if bias is None else bias) for _ in range(4)]
        for j in range(K + 3):
            i = o0 + j - pad
            if i < 0 or i >= L:
                continue                                                # skipped as a whole
            for p in range(4):
                k = j - p
                if 0 <= k < K:
                    acc[p] = (acc[p] + (w[k] * x[i]).astype(np.float32)).astype(np.float32)
        for p in range(4):
            if o0 + p < L:
                y[o0 + p] = acc[p]
    return np.moveaxis(y, 0, 1 + axis)


@pytest.mark.parametrize("axis", C.AXES)
@pytest.mark.parametrize("key", sorted(C.STRIP_SHAPES))
def test_windowed_order_equals_the_tap_order_and_agrees_with_float64(key, axis):
    f = C.strip_fixture(key, axis)
    K = f["geom"][4]
    y = _windowed_f32(f["x"], f["w"], f["bias"], axis)
    assert y.dtype == np.float32 and np.array_equal(y, C.expected(f))
    d = _windowed_f32(f["g"], C.flip_taps(f["w"]), None, axis)
    assert np.array_equal(d, C.expected(f, flipped=True))
    z, mag = R.dwconv_f64(f["x"], f["w"].reshape(f["kshape"]), f["bias"], f["pad"], f["dil"])
    err = np.abs(y.astype(np.float64) - z)
    assert (err <= R.gamma(K + 1) * mag).all()
    # the data gradient is the same rule on the flipped taps: against float64 autograd
    x64 = torch.tensor(f["x"]).double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = torch.tensor(f["w"].reshape(f["kshape"])).double().permute(2, 0, 1).unsqueeze(1)
    g64 = torch.tensor(f["g"]).double().permute(0, 3, 1, 2)
    (gx,) = torch.autograd.grad(F.conv2d(x64, w64, None, 1, f["pad"], 1, groups=x64.shape[1]), x64, g64)
    _, gmag = R.dwconv_f64(f["g"], C.flip_taps(f["w"]).reshape(f["kshape"]), None, f["pad"], f["dil"])
    assert (np.abs(d - gx.permute(0, 2, 3, 1).numpy()) <= R.gamma(K + 1) * gmag).all()


def test_the_smallest_cases_dry_run(built, monkeypatch):
    """the protocol of tests/test_guarded_cpu.py's dry run: argument lists fit the ctypes signature, each row calls
    exactly what it names, the references evaluate with the outputs' sizes"""
    from tests import abi_cases, guarded as G
    from tests.test_guarded_cpu import _DryLib
    for case in C.smallest_cases():
        called = set()
        real = built.lib()
        monkeypatch.setattr(abi_cases, "lib", lambda called=called: _DryLib(real, built.STRIP_SIGNATURES, called))
        run = G.Run("cpu", "A")
        res = case.fn(run)
        assert called == set(case.entry_points) == NAMES, (case.id, sorted(called))
        refs = res.ref()
        assert set(refs) == set(res.outs), case.id
        for k, (ref, bound) in refs.items():
            assert bound == 0.0 and np.asarray(ref).size == res.outs[k].numel(), (case.id, k)
            assert np.asarray(ref).dtype == np.float32 and np.isfinite(np.asarray(ref)).all(), (case.id, k)
    assert len(C.strip_cases()) == 7 * 2 * 2


# ------------------------------------------------------------------------------------------------------- composed op
def test_strip_conv_composes_on_cpu_tensors():
    from jdet_amd.ops import strip_conv as S
    x = torch.randn(2, 8, 5, 23).contiguous(memory_format=torch.channels_last)
    for shape, pad in (((8, 1, 1, 19), (0, 9)), ((8, 1, 19, 1), (9, 0))):
        w, b = torch.randn(shape), torch.randn(8)
        assert not S.fusable(x, w, b, pad)                                               # not a device tensor
        assert torch.equal(S.strip_conv(x, w, b, pad), F.conv2d(x, w, b, 1, pad, 1, groups=8))
        assert torch.equal(S.strip_conv(x, w, None, pad), F.conv2d(x, w, None, 1, pad, 1, groups=8))
    assert S.strip_axis(torch.zeros(8, 1, 1, 19)) == 1 and S.strip_axis(torch.zeros(8, 1, 19, 1)) == 0
    assert S.strip_axis(torch.zeros(8, 1, 3, 3)) is None and S.strip_axis(torch.zeros(8, 1, 1, 1)) == 1
    f = C.strip_fixture("e", 0)
    w = torch.tensor(f["w"]).t().reshape(12, 1, 3, 1)
    assert np.array_equal(S.pack_weight(w).numpy(), f["w"])
    assert np.array_equal(S.pack_weight(w, flip=True).numpy(), C.flip_taps(f["w"]))
    assert S._dw_geometry((2, 5, 7, 8, 19), 0) == (2, 5, 7, 8, 19, 1, 9, 0, 1, 1)
    assert S._dw_geometry((2, 5, 7, 8, 19), 1) == (2, 5, 7, 8, 1, 19, 0, 9, 1, 1)
    assert isinstance(S.ENABLED, bool)
    # the measured rule (profiles/strip.md): the K x 1 layers on maps of 2 x 256^2 positions and more
    big, small = torch.empty(2, 4, 256, 256), torch.empty(2, 4, 256, 255)
    assert S.COLUMN_MIN_POSITIONS == 131072
    assert S.preferred(big, torch.zeros(4, 1, 19, 1)) and not S.preferred(small, torch.zeros(4, 1, 19, 1))
    assert not S.preferred(big, torch.zeros(4, 1, 1, 19)) and not S.preferred(big, torch.zeros(4, 1, 1, 1))


# -------------------------------------------------------------------------------------------------------------- model
DIMS = {"StripNet_T": [32, 64, 160, 256], "StripNet_S": [64, 128, 320, 512]}
DEPTHS = {"StripNet_T": [3, 3, 5, 2], "StripNet_S": [2, 2, 4, 2]}


@pytest.fixture(scope="module")
def backbones():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils.registry import BACKBONES, build_from_cfg
    torch.manual_seed(0)
    return {n: build_from_cfg(dict(type=n, out_indices=(0, 1, 2, 3), pretrained="weights/not_there.pkl"), BACKBONES)
            for n in ("StripNet_T", "StripNet_S")}


def _state_names(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")]


@pytest.mark.parametrize("name", ["StripNet_T", "StripNet_S"])
def test_parameter_names_and_shapes_match_the_committed_list(backbones, name):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "stripnet_param_names.json")))[name]
    m = backbones[name]
    assert _state_names(m) == want
    keys = {k for k, _ in want}
    for k in ("patch_embed1.proj.weight", "patch_embed4.norm.running_var", "block1.0.norm1.weight", "block1.0.attn.proj_1.bias",
              "block3.1.attn.spatial_gating_unit.conv0.weight", "block3.1.attn.spatial_gating_unit.conv_spatial1.weight",
              "block3.1.attn.spatial_gating_unit.conv_spatial2.bias", "block3.1.attn.spatial_gating_unit.conv1.weight",
              "block2.0.attn.proj_2.weight", "block2.0.norm2.bias", "block2.0.mlp.fc1.weight",
              "block2.0.mlp.dwconv.dwconv.weight", "block2.0.mlp.fc2.bias", "block4.1.layer_scale_1", "block4.1.layer_scale_2",
              "norm1.weight", "norm4.bias"):
        assert k in keys, k
    assert not any("conv_squeeze" in k or k.endswith("conv_spatial.weight") or ".conv2." in k for k in keys)
    params = dict(m.named_parameters())
    assert params["block1.0.layer_scale_1"].requires_grad and float(params["block1.0.layer_scale_2"].detach()[0]) == float(np.float32(1e-2))
    for i, (d, n, r) in enumerate(zip(DIMS[name], DEPTHS[name], (8, 8, 4, 4))):
        assert len(getattr(m, "block%d" % (i + 1))) == n
        assert tuple(params["block%d.0.mlp.dwconv.dwconv.weight" % (i + 1)].shape) == (d * r, 1, 3, 3)
        sgu = getattr(m, "block%d" % (i + 1))[0].attn.spatial_gating_unit
        s1, s2 = sgu.conv_spatial1, sgu.conv_spatial2
        assert (s1.kernel_size, s1.padding, s1.groups, s1.dilation) == ((1, 19), (0, 9), d, (1, 1))
        assert (s2.kernel_size, s2.padding, s2.groups, s2.dilation) == ((19, 1), (9, 0), d, (1, 1))
        assert tuple(s1.weight.shape) == (d, 1, 1, 19) and tuple(s2.weight.shape) == (d, 1, 19, 1)
        assert tuple(sgu.conv0.weight.shape) == (d, 1, 5, 5) and tuple(sgu.conv1.weight.shape) == (d, d, 1, 1)
        assert getattr(m, "norm%d" % (i + 1)).eps == 1e-5
    # fan-out normal init: std sqrt(2 / (k k out / groups)); biases zero
    w = params["block1.0.mlp.fc1.weight"]
    assert abs(float(w.std()) - (2.0 / w.shape[0]) ** 0.5) < 0.1 * (2.0 / w.shape[0]) ** 0.5
    w = params["block3.0.attn.spatial_gating_unit.conv_spatial1.weight"]
    assert abs(float(w.std()) - (2.0 / 19) ** 0.5) < 0.1 * (2.0 / 19) ** 0.5
    assert float(params["block1.0.mlp.fc1.bias"].abs().max()) == 0.0
    m.train()
    assert all(b.training for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))


@pytest.mark.parametrize("name", ["StripNet_T", "StripNet_S"])
def test_outputs_are_channels_last_and_gradients_reach_every_parameter(backbones, name):
    m = backbones[name]
    m.train()
    m.zero_grad(set_to_none=True)
    outs = m(torch.randn(2, 3, 64, 64))
    assert [tuple(o.shape) for o in outs] == [(2, d, 64 // s, 64 // s) for d, s in zip(DIMS[name], (4, 8, 16, 32))]
    for o, d in zip(outs, DIMS[name]):
        assert o.is_contiguous(memory_format=torch.channels_last)
        assert o.stride()[1] == 1 and o.stride()[3] == d
    sum((o * torch.randn_like(o)).sum() for o in outs).backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k


def test_out_indices_drop_path_and_constructor_arguments():
    from jdet_amd.models.backbones.stripnet import StripNet
    torch.manual_seed(1)
    m = StripNet(embed_dims=[8, 8, 8, 8], depths=[1, 1, 1, 1], drop_path_rate=0.3, out_indices=(1, 3))
    assert [type(getattr(m, "block%d" % i)[0].drop_path).__name__ for i in (1, 2, 3, 4)] == ["Identity"] + ["DropPath"] * 3
    assert abs(m.block4[0].drop_path.p - 0.3) < 1e-6 and abs(m.block3[0].drop_path.p - 0.2) < 1e-6
    assert [tuple(o.shape) for o in m(torch.randn(2, 3, 64, 64))] == [(2, 8, 8, 8), (2, 8, 2, 2)]
    # k1s / k2s are taken as given: a 3 x 7 then a 7 x 3 kernel is no strip and still a "same" convolution
    m = StripNet(embed_dims=[8, 8], depths=[1, 1], num_stages=2, k1s=[3, 1], k2s=[7, 5], out_indices=(0, 1))
    sgu = m.block1[0].attn.spatial_gating_unit
    assert (sgu.conv_spatial1.kernel_size, sgu.conv_spatial1.padding) == ((3, 7), (1, 3))
    assert (sgu.conv_spatial2.kernel_size, sgu.conv_spatial2.padding) == ((7, 3), (3, 1))
    assert m.block2[0].attn.spatial_gating_unit.conv_spatial2.kernel_size == (5, 1)
    assert [tuple(o.shape) for o in m(torch.randn(1, 3, 32, 32))] == [(1, 8, 8, 8), (1, 8, 4, 4)]
    with pytest.raises(ValueError):
        StripNet(norm_cfg=dict(type="BN"))


# --------------------------------------------------------------------------------------------------------------- head
@pytest.fixture(scope="module")
def head():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.config import named
    from jdet_amd.utils.registry import HEADS, build_from_cfg
    torch.manual_seed(2)
    return build_from_cfg(named.STRIP_RCNN_S_CFG["model"]["bbox_head"], HEADS)


def test_head_layers_have_the_reference_names_and_the_class_specific_shapes(head):
    sd = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    want = {"cls_fcs.0.weight": (1024, 12544), "cls_fcs.0.bias": (1024,), "cls_fcs.1.weight": (1024, 1024),
            "cls_fcs.1.bias": (1024,), "reg_theta_fcs.0.weight": (1024, 12544), "reg_theta_fcs.0.bias": (1024,),
            "reg_theta_fcs.1.weight": (1024, 1024), "reg_theta_fcs.1.bias": (1024,),
            "reg_xy_wh_convs.0.conv.weight": (256, 256, 3, 3), "reg_xy_wh_convs.0.conv.bias": (256,),
            "reg_xy_wh_convs.1.conv.weight": (256, 256, 3, 3), "reg_xy_wh_convs.1.conv.bias": (256,),
            "reg_xy_wh_convs.1.bn.weight": (256,), "reg_xy_wh_convs.1.bn.bias": (256,),
            "reg_xy_wh_convs.1.bn.running_mean": (256,), "reg_xy_wh_convs.1.bn.running_var": (256,),
            "reg_xy_wh_convs.1.bn.num_batches_tracked": (),
            "fc_cls.weight": (16, 1024), "fc_cls.bias": (16,), "fc_reg_xy_wh.weight": (60, 12544),
            "fc_reg_xy_wh.bias": (60,), "fc_reg_theta.weight": (15, 1024), "fc_reg_theta.bias": (15,)}
    assert sd == want
    assert not any(k.startswith(("fc_reg.", "reg_fcs", "reg_convs", "shared")) for k in sd)
    assert not hasattr(head, "fc_reg") and not hasattr(head, "reg_fcs")
    for name in ("shared_convs", "shared_fcs", "cls_convs", "reg_xy_wh_fcs", "reg_theta_convs"):
        assert len(getattr(head, name)) == 0, name
    assert head.reg_class_agnostic is False and head.num_classes == 15 and head.reg_dim == 5
    assert not hasattr(head.reg_xy_wh_convs[0], "bn") and type(head.reg_xy_wh_convs[1].bn).__name__ == "BatchNorm2d"
    # the init: N(0, 0.01), N(0, 0.001), Xavier-uniform (bound sqrt(6 / (fan_in + fan_out))), zero biases
    assert abs(float(head.fc_cls.weight.std()) - 0.01) < 0.002
    assert abs(float(head.fc_reg_xy_wh.weight.std()) - 0.001) < 0.0001 and abs(float(head.fc_reg_theta.weight.std()) - 0.001) < 0.0002
    for m, fan in ((head.cls_fcs[0], 12544 + 1024), (head.reg_theta_fcs[1], 2048)):
        a = (6.0 / fan) ** 0.5
        assert 0.99 * a < float(m.weight.detach().abs().max()) <= a * (1 + 2.0 ** -22)      # the bound itself is float32
    assert all(float(v.abs().max()) == 0.0 for k, v in head.state_dict().items() if k.endswith(".bias"))


def _reference_forward_single(sd, x, dtype):
    """the reference's forward_single after the extractor (strip_head.py:L391-429), restated with plain torch on an NCHW
    map, flatten(1) in (c, ph, pw) order, the weights as the state dict holds them; BatchNorm in training mode"""
    p = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype).contiguous()
    x_cls = x.flatten(1)
    for i in range(2):
        x_cls = F.relu(F.linear(x_cls, p["cls_fcs.%d.weight" % i], p["cls_fcs.%d.bias" % i]))
    r = F.relu(F.conv2d(x, p["reg_xy_wh_convs.0.conv.weight"], p["reg_xy_wh_convs.0.conv.bias"], padding=1))
    r = F.conv2d(r, p["reg_xy_wh_convs.1.conv.weight"], p["reg_xy_wh_convs.1.conv.bias"], padding=1)
    r = F.relu(F.batch_norm(r, None, None, p["reg_xy_wh_convs.1.bn.weight"], p["reg_xy_wh_convs.1.bn.bias"], True, 0.1, 1e-5))
    x_theta = x.flatten(1)
    for i in range(2):
        x_theta = F.relu(F.linear(x_theta, p["reg_theta_fcs.%d.weight" % i], p["reg_theta_fcs.%d.bias" % i]))
    cls_score = F.linear(x_cls, p["fc_cls.weight"], p["fc_cls.bias"])
    xy_wh = F.linear(r.flatten(1), p["fc_reg_xy_wh.weight"], p["fc_reg_xy_wh.bias"])
    theta = F.linear(x_theta, p["fc_reg_theta.weight"], p["fc_reg_theta.bias"])
    return cls_score, torch.cat([xy_wh, theta], dim=1)


class _StubExtractor(torch.nn.Module):
    num_inputs = 4

    def forward(self, feats, rois):
        return feats[0]


def test_head_trunk_equals_the_reference_forward_single(head):
    import copy
    torch.manual_seed(3)
    h = copy.deepcopy(head).train()
    # every layer away from its init, the output layers large enough to be read
    with torch.no_grad():
        for k, p in h.named_parameters():
            p.copy_(torch.randn_like(p) * (0.05 if k.startswith("fc_") else (0.02 if p.dim() > 1 else 0.1)))
    h.bbox_roi_extractor = _StubExtractor()
    x = torch.randn(12, 256, 7, 7).contiguous(memory_format=torch.channels_last)
    sd = {k: v.clone() for k, v in h.state_dict().items()}           # the reference's column order (the save hook)
    cls32, box32 = h._trunk([x], None)
    assert cls32.shape == (12, 16) and box32.shape == (12, 75)
    h64 = copy.deepcopy(h).double()
    cls64h, box64h = h64._trunk([x.double()], None)
    rc32, rb32 = _reference_forward_single(sd, x, torch.float32)
    rc64, rb64 = _reference_forward_single(sd, x, torch.float64)
    # in float64 the two are the same function
    assert float((cls64h - rc64).abs().max()) <= 1e-12 * float(rc64.abs().max())
    assert float((box64h - rb64).abs().max()) <= 1e-12 * float(rb64.abs().max())
    for what, got, ref32, ref64 in (("cls_score", cls32, rc32, rc64), ("bbox_pred", box32, rb32, rb64)):
        own = float((ref32.double() - ref64).abs().max())
        err = float((got.double() - ref64).abs().max())
        print("StripHead %s: max error against the float64 restatement, float32 restatement %.3e, head %.3e (bound %.3e)"
              % (what, own, err, 4 * own))
        assert own > 0 and err <= 4 * own, what
    # a loaded reference-order state dict gives the same function back
    h2 = copy.deepcopy(head).train()
    h2.load_state_dict(sd)
    h2.bbox_roi_extractor = _StubExtractor()
    c2, b2 = h2._trunk([x], None)
    assert torch.equal(c2, cls32) and torch.equal(b2, box32)


@pytest.mark.parametrize("c", [0, 7, 12, 14])
def test_class_c_owns_entries_5c_of_the_concatenation(head, c):
    """a prediction whose only non-zero entries are 5c .. 5c + 4 of cat([xy_wh, theta]) moves the box of class c only"""
    from jdet_amd.models.boxes.fixed_shape import class_rows
    rois = torch.tensor([[50.0, 40.0, 30.0, 12.0, 0.3], [20.0, 25.0, 8.0, 16.0, -0.5]])
    xy_wh, theta = torch.zeros(2, 60), torch.zeros(2, 15)
    delta = torch.tensor([0.5, -0.25, 0.3, -0.2, 0.4])
    for e in range(5 * c, 5 * c + 5):                                   # entry e of the concatenation
        (xy_wh if e < 60 else theta)[:, e if e < 60 else e - 60] = delta[e - 5 * c]
    pred = torch.cat([xy_wh, theta], dim=1)
    decoded = head.bbox_coder.decode(rois, pred, max_shape=None).view(2, 15, 5)
    still = head.bbox_coder.decode(rois, torch.zeros(2, 75), max_shape=None).view(2, 15, 5)
    for k in range(15):
        moved = not torch.allclose(decoded[:, k], still[:, k], atol=1e-6)
        assert moved == (k == c), k
    assert (decoded[:, c, :2] - still[:, c, :2]).abs().min() > 0.1 and (decoded[:, c, 4] - still[:, c, 4]).abs().min() > 1e-3
    # the loss reads the same five entries for a row labelled c
    rows = class_rows(pred, torch.tensor([c, c]), 5, head.reg_class_agnostic, head.num_classes)
    assert torch.equal(rows, delta[None].repeat(2, 1))
    other = class_rows(pred, torch.tensor([(c + 1) % 15] * 2), 5, head.reg_class_agnostic, head.num_classes)
    assert float(other.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------- config
def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return [_plain(x) for x in v] if isinstance(v, (list, tuple)) else v


def test_named_config_equals_the_reference_file_and_builds():
    import jdet_amd.models  # noqa: F401
    import jdet_amd.optims  # noqa: F401
    from jdet_amd.config import Config, named
    from jdet_amd.utils import registry as Reg
    cfg = named.STRIP_RCNN_S_CFG
    c = Config(os.path.join(ROOT, "tests", "golden", "configs", "strip_rcnn_s_fpn_1x_dota_with_flip.yaml")).dump()
    for k in ("model", "optimizer", "scheduler"):
        assert _plain(cfg[k]) == _plain(c[k]), k
    assert cfg["optimizer"]["type"] == "AdamW" and cfg["optimizer"]["lr"] == 0.0001 and cfg["optimizer"]["weight_decay"] == 0.05
    assert cfg["model"]["neck"]["in_channels"] == [64, 128, 320, 512] and cfg["model"]["bbox_head"]["reg_class_agnostic"] is True
    for name in ("StripNet", "StripNet_T", "StripNet_S"):
        assert name in Reg.BACKBONES, name
    assert "StripHead" in Reg.HEADS and "StripRCNN" in Reg.MODELS
    m = Reg.build_from_cfg(cfg["model"], Reg.MODELS)          # the pretrained file is absent: the init stays
    assert type(m).__name__ == "StripRCNN" and type(m.backbone).__name__ == "StripNet"
    assert type(m.bbox_head).__name__ == "StripHead" and type(m.rpn).__name__ == "OrientedRPNHead"
    assert m.backbone.out_indices == (0, 1, 2, 3) and m.neck.lateral_convs[2].conv.in_channels == 320
    assert [len(getattr(m.backbone, "block%d" % i)) for i in (1, 2, 3, 4)] == [2, 2, 4, 2]
    opt = Reg.build_from_cfg(dict(cfg["optimizer"]), Reg.OPTIMS, params=list(m.parameters()))
    assert Reg.build_from_cfg(dict(cfg["scheduler"]), Reg.SCHEDULERS, optimizer=opt) is not None
    feats = m.neck(m.backbone(torch.randn(1, 3, 64, 64)))
    assert [tuple(f.shape) for f in feats] == [(1, 256, s, s) for s in (16, 8, 4, 2, 1)]
