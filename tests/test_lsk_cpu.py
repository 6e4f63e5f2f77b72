"""CPU: the LSKNet feature without a device -- the side header against LSK_SIGNATURES and the exports; every argument
rule refused before any launch; the float32 restatement of the tap order (tests/lsk_ref.py) against float64
F.conv2d(groups=C), forward and (on flipped taps) data gradient, within gamma(KH KW + 1) * sum |terms|; the dry run of
the smallest case of every entry point; the composed routes of the ops; LSKNet_t / LSKNet_s parameter names and shapes
against the committed list, output shapes and strides, gradients to every parameter; the named config against its
golden YAML and the detector it builds."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lsk_cases as C
from tests import lsk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"jdet_dwconv_nhwc_forward", "jdet_dwconv_nhwc_wgrad_workspace", "jdet_dwconv_nhwc_wgrad",
         "jdet_dwconv_gelu_backward", "jdet_lsk_squeeze_forward", "jdet_lsk_squeeze_backward", "jdet_lsk_select_forward",
         "jdet_lsk_select_backward"}


# ---------------------------------------------------------------------------------------------------------------- ABI
def _declared():
    src = open(os.path.join(ROOT, "include", "jdet_hip_lsk.h")).read()
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
    d = _declared()
    assert set(d) == set(built.LSK_SIGNATURES) == NAMES
    for other in (built.SIGNATURES, built.RETINA_SIGNATURES, built.CSL_SIGNATURES):
        assert not set(d) & set(other)
    main = open(os.path.join(ROOT, "include", "jdet_hip.h")).read()
    assert "dwconv" not in main and "lsk" not in main
    raw = ctypes.CDLL(built.LIB_PATH)
    lib = built.lib()
    for name, nargs in d.items():
        res, args = built.LSK_SIGNATURES[name]
        assert len(args) == nargs, name
        assert hasattr(raw, name), "missing export " + name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res, name


def test_argument_validation_returns_before_any_launch(built):
    """every answer comes from the host-side checks: no device here, and a launch on these addresses would not return"""
    lib = built.lib()
    N, X = None, 4096                                        # X: a 16-byte aligned non-null address nobody reads
    BAD, UNS, WS = -1, -2, -3

    def geom(n=2, h=8, w=8, c=8, kh=7, kw=7, ph=9, pw=9, dh=3, dw=3):
        return (n, h, w, c, kh, kw, ph, pw, dh, dw)

    def fwd(x=X, wp=X, b=N, act=0, y=X, **g):
        return lib.jdet_dwconv_nhwc_forward(x, wp, b, *geom(**g), act, y, N)

    def gelu(x=X, wp=X, b=X, gy=X, gz=X, **g):
        return lib.jdet_dwconv_gelu_backward(x, wp, b, gy, *geom(**g), gz, N)

    def need(**g):
        return lib.jdet_dwconv_nhwc_wgrad_workspace(*geom(**g)[:6])

    def wgrad(x=X, g_=X, gw=X, gb=N, ws=X, wsb=None, **g):
        return lib.jdet_dwconv_nhwc_wgrad(x, g_, *geom(**g), gw, gb, ws, need(**g) if wsb is None else wsb, N)

    for f in (fwd, gelu, wgrad):
        for dim in ("n", "h", "w", "c", "kh", "kw"):
            assert f(**{dim: 0}) == BAD and f(**{dim: -1}) == BAD, dim
        assert f(ph=-1) == BAD and f(dh=0) == BAD and f(dw=-3) == BAD
        assert f(c=6) == UNS and f(c=2) == UNS and f(c=321) == UNS                       # C % 4
        assert f(ph=8) == UNS and f(pw=10) == UNS and f(ph=3, pw=3) == UNS               # 2 pad != dil (K - 1)
        assert f(kh=4, ph=4) == UNS                                                      # an even kernel under dilation 3
        assert f(n=2 ** 13, h=2 ** 8, w=2 ** 8, c=4, x=X + 4) == UNS                     # 2^31 elements
        assert f(n=2 ** 13 - 1, h=2 ** 8, w=2 ** 8, c=4, x=X + 4) == BAD                 # one image fewer: the next rule
        assert f(kh=1025, ph=3 * 512) == UNS and f(dh=1026, ph=3 * 1026) == UNS
        assert f(x=N) == BAD and f(x=X + 4) == BAD and f(x=X + 8) == BAD                 # null, not 16-byte aligned
    assert fwd(wp=N) == BAD and fwd(y=N) == BAD and fwd(act=2) == BAD and fwd(act=-1) == BAD
    assert fwd(wp=X + 4) == BAD and fwd(b=X + 4) == BAD and fwd(y=X + 12) == BAD
    assert gelu(wp=N) == BAD and gelu(gy=N) == BAD and gelu(gz=N) == BAD and gelu(gy=X + 4) == BAD
    assert wgrad(g_=N) == BAD and wgrad(gw=N) == BAD and wgrad(ws=N) == BAD and wgrad(ws=X + 8) == BAD
    assert wgrad(gb=X + 4) == BAD
    # the workspace: S * (KH KW + 1) * C floats, S = min(N H, 512); one byte less is refused, as is none at all
    assert need() == 16 * 50 * 8 * 4 and need(n=2, h=1024) == 512 * 50 * 8 * 4 and need(c=6) == 0 and need(h=0) == 0
    assert wgrad(wsb=need() - 1) == WS and wgrad(wsb=0) == WS
    # the selection entry points take any Ch >= 1
    def sq(a1=X, a2=X, n=2, h=3, w=5, ch=16, agg=X, am=X):
        return lib.jdet_lsk_squeeze_forward(a1, a2, n, h, w, ch, agg, am, N)

    def sqb(g=X, am=X, n=2, h=3, w=5, ch=16, g1=X, g2=X):
        return lib.jdet_lsk_squeeze_backward(g, am, n, h, w, ch, g1, g2, N)

    def sel(a1=X, a2=X, sig=X, n=2, h=3, w=5, ch=16, out=X):
        return lib.jdet_lsk_select_forward(a1, a2, sig, n, h, w, ch, out, N)

    def selb(g=X, a1=X, a2=X, sig=X, n=2, h=3, w=5, ch=16, g1=X, g2=X, gs=X):
        return lib.jdet_lsk_select_backward(g, a1, a2, sig, n, h, w, ch, g1, g2, gs, N)
    for f in (sq, sqb, sel, selb):
        for dim in ("n", "h", "w", "ch"):
            assert f(**{dim: 0}) == BAD and f(**{dim: -2}) == BAD, dim
        assert f(n=2 ** 10, h=2 ** 10, w=2 ** 6, ch=8) == UNS                            # 2^31 elements of the concatenation
        assert f(n=2 ** 5, h=2 ** 10, w=2 ** 10, ch=1) == UNS                            # 2^25 pixels
    for f, ptrs in ((sq, ("a1", "a2", "agg", "am")), (sqb, ("g", "am", "g1", "g2")), (sel, ("a1", "a2", "sig", "out")),
                    (selb, ("g", "a1", "a2", "sig", "g1", "g2", "gs"))):
        for p in ptrs:
            assert f(**{p: N}) == BAD, p


def test_strip_and_square_geometries_pass_the_rules(built):
    """the geometries of the feature are accepted up to the first pointer check (a null x is the next rule)"""
    lib = built.lib()
    for key in C.DW_SHAPES:
        f = C.dw_fixture(key)
        assert lib.jdet_dwconv_nhwc_forward(None, 4096, None, *f["geom"], 0, 4096, None) == -1
        n, h, w, c, kh, kw = f["geom"][:6]
        assert lib.jdet_dwconv_nhwc_wgrad_workspace(n, h, w, c, kh, kw) == min(n * h, 512) * (kh * kw + 1) * c * 4


# ------------------------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("key", sorted(C.DW_SHAPES))
def test_float32_tap_order_agrees_with_float64_conv2d(key):
    f = C.dw_fixture(key)
    kh, kw = f["w"].shape[:2]
    y32 = R.dwconv_f32(f["x"], f["w"], f["bias"], f["pad"], f["dil"])
    z, mag = R.dwconv_f64(f["x"], f["w"], f["bias"], f["pad"], f["dil"])
    err = np.abs(y32.astype(np.float64) - z)
    assert (err <= R.conv_bound(mag, kh, kw)).all() and err.max() > 0
    # the data gradient is the same rule on the flipped taps: against float64 autograd
    x64 = torch.tensor(f["x"]).double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = torch.tensor(f["w"]).double().permute(2, 0, 1).unsqueeze(1)
    g64 = torch.tensor(f["g"]).double().permute(0, 3, 1, 2)
    (gx,) = torch.autograd.grad(F.conv2d(x64, w64, None, 1, f["pad"], f["dil"], groups=x64.shape[1]), x64, g64)
    d32 = R.dwconv_f32(f["g"], R.flip_taps(f["w"]), None, f["pad"], f["dil"])
    _, gmag = R.dwconv_f64(f["g"], R.flip_taps(f["w"]), None, f["pad"], f["dil"])
    assert (np.abs(d32 - gx.permute(0, 2, 3, 1).numpy()) <= R.conv_bound(gmag, kh, kw)).all()


def test_skipped_taps_and_order_are_what_the_restatement_says():
    """a single pixel sees the centre tap only; a hand-worked 1 x 3 row in float32"""
    f = C.dw_fixture("b")
    y = R.dwconv_f32(f["x"], f["w"], None, f["pad"], f["dil"])
    assert np.array_equal(y[0, 0, 0], (f["w"][2, 2] * f["x"][0, 0, 0]).astype(np.float32))
    x = np.float32([1e8, 1.0, -1e8]).reshape(1, 1, 3, 1).repeat(4, 3)
    w = np.ones((1, 3, 4), np.float32)
    y = R.dwconv_f32(x, w, np.float32([0.5] * 4), (0, 1), (1, 1))
    # w = 1: ((0.5 + 1e8) + 1) + -1e8 in float32 = 0; the ends skip their outside tap
    assert y[0, 0, 1, 0] == 0.0 and y[0, 0, 0, 0] == np.float32(np.float32(0.5 + 1e8) + 1.0) and y[0, 0, 2, 0] == np.float32(
        np.float32(np.float32(0.5) + np.float32(1.0)) + np.float32(-1e8))


def test_selection_restatements_against_torch():
    for ch in C.SELECT_CH:
        for tied in (False, True):
            f = C.select_fixture(ch, tied)
            a1, a2 = (torch.tensor(f[k]).permute(0, 3, 1, 2).double().requires_grad_(True) for k in ("a1", "a2"))
            cat = torch.cat([a1, a2], 1)
            mx, idx = cat.max(dim=1)
            mean, _, rmax, ridx = R.squeeze(f["a1"], f["a2"])
            assert np.array_equal(idx.numpy(), ridx) and np.array_equal(mx.detach().numpy(), rmax.astype(np.float64))
            assert np.abs(cat.mean(1).detach().numpy() - mean).max() <= 1e-15
            assert R.has_ties(f["a1"], f["a2"]).any() == tied
            g = torch.tensor(f["g_agg"]).double()
            (cat.mean(1) * g[..., 0] + mx * g[..., 1]).sum().backward()
            r1, r2, _, _ = R.squeeze_backward64(f["g_agg"], ridx, ch)       # first index: what autograd differentiates through
            assert np.abs(a1.grad.permute(0, 2, 3, 1).numpy() - r1).max() <= 1e-15
            assert np.abs(a2.grad.permute(0, 2, 3, 1).numpy() - r2).max() <= 1e-15


def test_every_entry_point_dry_runs(built, monkeypatch):
    """the protocol of tests/test_guarded_cpu.py's dry run on the smallest cases: argument lists fit the ctypes
    signatures, each row calls exactly what it names, the references evaluate with the outputs' sizes"""
    from tests import abi_cases, guarded as G
    from tests.test_guarded_cpu import _DryLib
    covered = set()
    for case in C.smallest_cases():
        called = set()
        real = built.lib()
        monkeypatch.setattr(abi_cases, "lib", lambda called=called: _DryLib(real, built.LSK_SIGNATURES, called))
        run = G.Run("cpu", "A")
        res = case.fn(run)
        launching = {n for n in case.entry_points if not n.endswith("_workspace")}
        assert called == launching, (case.id, sorted(called))
        covered |= set(case.entry_points)
        refs = res.ref()
        assert set(refs) == set(res.outs), case.id
        for k, (ref, bound) in refs.items():
            b = np.asarray(bound, np.float64)
            assert np.isfinite(b).all() and (b >= 0).all(), (case.id, k)
            assert np.asarray(ref).size == res.outs[k].numel() and (b.ndim == 0 or b.size == res.outs[k].numel())
            assert np.isfinite(np.asarray(ref, np.float64)).all(), (case.id, k)
    assert covered == set(built.LSK_SIGNATURES)
    assert len(C.dw_cases()) == 7 * 3 + 2 * len(C.GELU_KEYS) and len(C.select_cases()) == 4 * 3 + 2


# ------------------------------------------------------------------------------------------------------- composed ops
def test_ops_compose_on_cpu_tensors():
    from jdet_amd.ops import dwconv as D, lsk_select as S
    x = torch.randn(2, 8, 5, 7).contiguous(memory_format=torch.channels_last)
    w, b = torch.randn(8, 1, 7, 7), torch.randn(8)
    assert not D.fusable(x, w, b, 9, 3) and D.same_padded(w, 9, 3) and not D.same_padded(w, 3, 3)
    assert not D.same_padded(w, 9, 3, stride=2) and D.same_padded(torch.zeros(8, 1, 1, 19), (0, 9), 1)
    y = D.dwconv(x, w, b, 9, 3, act="gelu")
    assert torch.equal(y, F.gelu(F.conv2d(x, w, b, 1, 9, 3, groups=8)))
    assert torch.equal(D.dwconv(x, w, None, 9, 3), F.conv2d(x, w, None, 1, 9, 3, groups=8))
    with pytest.raises(ValueError):
        D.dwconv(x, w, b, 9, 3, act="relu")
    f = C.dw_fixture("c")
    assert np.array_equal(D.pack_weight(torch.tensor(f["w"]).permute(2, 0, 1).unsqueeze(1)).numpy(), f["w"])
    assert np.array_equal(D.pack_weight(torch.tensor(f["w"]).permute(2, 0, 1).unsqueeze(1), flip=True).numpy(),
                          R.flip_taps(f["w"]))
    a1, a2, sig = torch.randn(2, 16, 3, 5), torch.randn(2, 16, 3, 5), torch.rand(2, 2, 3, 5)
    assert not S.fusable(a1, a2) and not S.fusable(a1, a2, sig)
    agg = S.lsk_squeeze(a1, a2)
    cat = torch.cat([a1, a2], 1)
    assert torch.equal(agg[:, 0], cat.mean(1)) and torch.equal(agg[:, 1], cat.max(1)[0])
    assert torch.equal(S.lsk_select(a1, a2, sig), a1 * sig[:, :1] + a2 * sig[:, 1:])
    assert isinstance(D.ENABLED, bool) and isinstance(S.ENABLED, bool)


# -------------------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def backbones():
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils.registry import BACKBONES, build_from_cfg
    torch.manual_seed(0)
    return {n: build_from_cfg(dict(type=n, out_indices=(0, 1, 2, 3), pretrained="weights/not_there.pkl"), BACKBONES)
            for n in ("LSKNet_t", "LSKNet_s")}


def _state_names(m):
    return [[k, list(v.shape)] for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")]


@pytest.mark.parametrize("name", ["LSKNet_t", "LSKNet_s"])
def test_parameter_names_and_shapes_match_the_committed_list(backbones, name):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "lsknet_param_names.json")))[name]
    m = backbones[name]
    assert _state_names(m) == want
    keys = {k for k, _ in want}
    for k in ("patch_embed1.proj.weight", "patch_embed4.norm.running_var", "block1.0.norm1.weight", "block1.0.attn.proj_1.bias",
              "block3.1.attn.spatial_gating_unit.conv0.weight", "block3.1.attn.spatial_gating_unit.conv_spatial.weight",
              "block3.1.attn.spatial_gating_unit.conv1.weight", "block3.1.attn.spatial_gating_unit.conv2.bias",
              "block3.1.attn.spatial_gating_unit.conv_squeeze.weight", "block3.1.attn.spatial_gating_unit.conv.weight",
              "block2.0.attn.proj_2.weight", "block2.0.norm2.bias", "block2.0.mlp.fc1.weight",
              "block2.0.mlp.dwconv.dwconv.weight", "block2.0.mlp.fc2.bias", "block4.1.layer_scale_1", "block4.1.layer_scale_2",
              "norm1.weight", "norm4.bias"):
        assert k in keys, k
    params = dict(m.named_parameters())
    assert params["block1.0.layer_scale_1"].requires_grad and float(params["block1.0.layer_scale_2"].detach()[0]) == float(np.float32(1e-2))
    dims = {"LSKNet_t": [32, 64, 160, 256], "LSKNet_s": [64, 128, 320, 512]}[name]
    depths = {"LSKNet_t": [3, 3, 5, 2], "LSKNet_s": [2, 2, 4, 2]}[name]
    for i, (d, n, r) in enumerate(zip(dims, depths, (8, 8, 4, 4))):
        assert len(getattr(m, "block%d" % (i + 1))) == n
        assert tuple(params["block%d.0.mlp.dwconv.dwconv.weight" % (i + 1)].shape) == (d * r, 1, 3, 3)
        sgu = getattr(m, "block%d" % (i + 1))[0].attn.spatial_gating_unit
        assert (sgu.conv_spatial.kernel_size, sgu.conv_spatial.dilation, sgu.conv_spatial.padding) == ((7, 7), (3, 3), (9, 9))
        assert tuple(sgu.conv_squeeze.weight.shape) == (2, 2, 7, 7) and tuple(sgu.conv1.weight.shape) == (d // 2, d, 1, 1)
    # fan-out normal init: std sqrt(2 / (k k out / groups)); biases zero
    w = params["block1.0.mlp.fc1.weight"]
    assert abs(float(w.std()) - (2.0 / w.shape[0]) ** 0.5) < 0.1 * (2.0 / w.shape[0]) ** 0.5
    assert float(params["block1.0.mlp.fc1.bias"].abs().max()) == 0.0
    m.train()
    assert all(b.training for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))


@pytest.mark.parametrize("name", ["LSKNet_t", "LSKNet_s"])
def test_outputs_are_channels_last_and_gradients_reach_every_parameter(backbones, name):
    m = backbones[name]
    m.train()
    m.zero_grad(set_to_none=True)
    outs = m(torch.randn(2, 3, 64, 64))
    dims = {"LSKNet_t": [32, 64, 160, 256], "LSKNet_s": [64, 128, 320, 512]}[name]
    assert [tuple(o.shape) for o in outs] == [(2, d, 64 // s, 64 // s) for d, s in zip(dims, (4, 8, 16, 32))]
    for o, d in zip(outs, dims):
        assert o.is_contiguous(memory_format=torch.channels_last)
        assert o.stride()[1] == 1 and o.stride()[3] == d
    sum((o * torch.randn_like(o)).sum() for o in outs).backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k


def test_out_indices_and_drop_path():
    from jdet_amd.models.backbones.lsknet import DropPath, LSKNet
    torch.manual_seed(1)
    m = LSKNet(embed_dims=[8, 8, 8, 8], depths=[1, 1, 1, 1], drop_path_rate=0.3, out_indices=(1, 3))
    assert [type(getattr(m, "block%d" % i)[0].drop_path).__name__ for i in (1, 2, 3, 4)] == ["Identity"] + ["DropPath"] * 3
    assert abs(m.block4[0].drop_path.p - 0.3) < 1e-6
    assert [tuple(o.shape) for o in m(torch.randn(2, 3, 64, 64))] == [(2, 8, 8, 8), (2, 8, 2, 2)]
    d = DropPath(0.5)
    x = torch.ones(64, 3, 2, 2)
    y = d.train()(x)
    per = y.flatten(1)
    assert ((per == 0).all(1) | (per == 2).all(1)).all() and 0 < int((per[:, 0] == 0).sum()) < 64
    assert torch.equal(d.eval()(x), x)


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return [_plain(x) for x in v] if isinstance(v, (list, tuple)) else v


def test_named_config_equals_the_reference_file_and_builds():
    import jdet_amd.models  # noqa: F401
    import jdet_amd.optims  # noqa: F401
    from jdet_amd.config import Config, named
    from jdet_amd.utils import registry as Reg
    cfg = named.LSKNET_S_ORCNN_CFG
    c = Config(os.path.join(ROOT, "tests", "golden", "configs", "lsknet-s_fpn_1x_dota_with_flip.yaml")).dump()
    for k in ("model", "optimizer", "scheduler"):
        assert _plain(cfg[k]) == _plain(c[k]), k
    assert cfg["optimizer"]["type"] == "AdamW" and cfg["optimizer"]["lr"] == 0.0001 and cfg["optimizer"]["weight_decay"] == 0.05
    assert cfg["model"]["neck"]["in_channels"] == [64, 128, 320, 512]
    for name in ("LSKNet", "LSKNet_t", "LSKNet_s"):
        assert name in Reg.BACKBONES, name
    m = Reg.build_from_cfg(cfg["model"], Reg.MODELS)          # the pretrained file is absent: the init stays
    assert type(m).__name__ == "OrientedRCNN" and type(m.backbone).__name__ == "LSKNet"
    assert m.backbone.out_indices == (0, 1, 2, 3) and m.neck.lateral_convs[2].conv.in_channels == 320
    opt = Reg.build_from_cfg(dict(cfg["optimizer"]), Reg.OPTIMS, params=list(m.parameters()))
    assert Reg.build_from_cfg(dict(cfg["scheduler"]), Reg.SCHEDULERS, optimizer=opt) is not None
    feats = m.neck(m.backbone(torch.randn(1, 3, 64, 64)))
    assert [tuple(f.shape) for f in feats] == [(1, 256, s, s) for s in (16, 8, 4, 2, 1)]
