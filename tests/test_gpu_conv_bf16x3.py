"""GPU: the 3x3 convolution on bf16 MFMA through the exact three-way fp32 split (csrc/conv_bf16x3.hip), called
through its entry point: against float64 conv2d at the bound of tests/test_gpu_conv_igemm.py, against the fp32 kernel's own error, the bit-exact probes of tests/bf16x3_cases.py, the
buffer contract, and the ConvModule route against JDET_CONV_BF16X3=0."""
import numpy as np
import pytest
import torch

from tests import bf16x3_cases as BC

pytestmark = pytest.mark.gpu


def _run(x, w, bias=None, relu=False, mask=None, entry="bf16x3"):
    """numpy / tensor inputs -> y (N,H,W,Cout) device tensor through the C entry point"""
    from jdet_amd import _lib as L
    t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))).cuda()
    x, w, bias, mask = t(x), t(w), t(bias), t(mask)
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    y = torch.full((N, H, W, Cout), float("nan"), device="cuda")
    if entry == "bf16x3":
        rc = L.lib().jdet_conv3x3_bf16x3_forward(L.ptr(x), N, H, W, Cin, L.ptr(w), Cout, L.ptr(bias), int(relu), L.ptr(mask),
                                                 L.ptr(y), L.stream_ptr(x))
    else:
        rc = L.lib().jdet_conv3x3_igemm_forward(L.ptr(x), N, H, W, Cin, L.ptr(w), Cout, L.ptr(bias), int(relu), L.ptr(mask),
                                                None, 0, L.ptr(y), None, 0, L.stream_ptr(x))
    assert rc == 0, rc
    return y


def _finish(ref, relu, mask):
    ref = np.maximum(ref, 0.0) if relu else ref
    return ref * mask.astype(np.float64).reshape(ref.shape[:3] + (1,)) if mask is not None else ref


def _max_err(y, ref):
    return float((y.double().cpu() - torch.from_numpy(np.array(ref))).abs().max())


@pytest.mark.parametrize("case", sorted(BC.CASES))
def test_matches_float64_with_and_without_bias_relu_and_rowmask(case):
    x, w, b, mask = BC.inputs(case)
    for bias in (False, True):
        for relu in (False, True):
            for masked in (False, True):
                ref = _finish(BC.reference(case, bias), relu, mask if masked else None)
                y = _run(x, w, b if bias else None, relu, mask if masked else None)
                err, bound = _max_err(y, ref), BC.BOUND[0] * np.abs(ref).max() + BC.BOUND[1]
                print("case %s bias %d relu %d mask %d: max err %.3e bound %.3e" % (case, bias, relu, masked, err, bound))
                assert err <= bound


def test_unsupported_channels_are_reported():
    from jdet_amd import _lib as L
    assert L.lib().jdet_conv3x3_bf16x3_supported(48, 64) == 0
    x, w = torch.zeros(1, 4, 4, 48, device="cuda"), torch.zeros(64, 3, 3, 48, device="cuda")
    y = torch.zeros(1, 4, 4, 64, device="cuda")
    assert L.lib().jdet_conv3x3_bf16x3_forward(L.ptr(x), 1, 4, 4, 48, L.ptr(w), 64, None, 0, None, L.ptr(y),
                                               L.stream_ptr(x)) == -2


@pytest.mark.parametrize("log2_scale", [-60, 40])
def test_range_of_the_split_at_the_tower_channels(log2_scale):
    """case (f) with the inputs scaled by a power of two: the split parts keep fp32's exponent range, so the error
    scales with the data (the absolute term of the bound is scaled along: at 2^-60 it would otherwise hide everything)"""
    x, w, _, _ = BC.inputs("f")
    s = 2.0 ** log2_scale
    ref = BC.reference("f", False) * s
    y = _run((x * np.float32(s)).astype(np.float32), w)
    err, bound = _max_err(y, ref), BC.BOUND[0] * np.abs(ref).max() + BC.BOUND[1] * s
    print("case f x 2^%d: max err %.3e bound %.3e" % (log2_scale, err, bound))
    assert err <= bound


@pytest.mark.parametrize("case", ["d", "f"])
def test_error_against_float64_is_at_most_twice_the_fp32_kernels(case):
    x, w, _, _ = BC.inputs(case)
    ref = BC.reference(case, False)
    err_new, err_f32 = _max_err(_run(x, w), ref), _max_err(_run(x, w, entry="igemm"), ref)
    print("case %s: max err against float64: bf16x3 %.3e, fp32 kernel %.3e, ratio %.2f" % (case, err_new, err_f32,
                                                                                         err_new / err_f32))
    assert err_new <= 2 * err_f32


@pytest.mark.parametrize("which", ["i", "ii", "iii"])
def test_exactness_probe(which):
    """one non-zero, fp32-exact product per output: y equals the float64 reference bit for bit"""
    x, w, ref = BC.probe(which)
    y = _run(x, w).double().cpu().numpy()
    wrong = int((y != ref).sum())
    print("probe %s: %d of %d outputs differ, %d non-zero" % (which, wrong, ref.size, int((ref != 0).sum())))
    assert wrong == 0
    assert (ref != 0).sum() > (1000 if which == "ii" else ref.size // 2)


def test_rowmask_multiplies_the_finished_rows_and_runs_are_bit_equal():
    x, w, b, mask = BC.inputs("d")
    y = _run(x, w, b, True)
    ym = _run(x, w, b, True, mask)
    assert torch.equal(ym, y * torch.from_numpy(np.array(mask)).cuda().view(y.shape[:3] + (1,)))
    assert torch.equal(_run(x, w, b, True).view(torch.int32), y.view(torch.int32))
    assert (ym == 0).all(dim=3).sum().item() >= int((mask == 0).sum())


def test_batch_of_zero_returns_at_once():
    from jdet_amd import _lib as L
    assert L.lib().jdet_conv3x3_bf16x3_forward(None, 0, 8, 8, 64, None, 64, None, 1, None, None, None) == 0


@pytest.mark.parametrize("case", ["b", "c", "d"])
def test_buffer_contract(dev, case):
    """the guard-band / poison protocol of tests/guarded.py: nothing outside y is written, no guard is read"""
    from tests import guarded
    from tests.abi_cases import bf16x3_case
    c = bf16x3_case(case)
    guarded.run_case(c.entry_points[0], c.label, c.fn, dev)


def test_conv_module_route_matches_the_fp32_route():
    """ConvModule(256, 256, 3) on 2 x 128 x 128 -- the shape that takes the big route: output, grad_x, weight and bias
    gradients of the split route (forward and data gradient) against JDET_CONV_BF16X3=0, at the bound of
    test_conv_module_fused_path_matches_library_path"""
    from jdet_amd.models.utils.modules import ConvModule
    from jdet_amd.ops import conv_igemm as CI
    torch.manual_seed(5)
    m = ConvModule(256, 256, 3, padding=1, act_cfg=dict(type="ReLU")).cuda()
    torch.nn.init.normal_(m.conv.bias, std=0.1)
    x = torch.randn(2, 256, 128, 128, device="cuda").contiguous(memory_format=torch.channels_last)
    assert CI.preferred(x, m.conv.weight) and CI.bf16x3_big(2 * 128 * 128, 256, 256)
    g = torch.randn(2, 256, 128, 128, device="cuda")
    saved = (CI.BF16X3, CI.BF16X3_DGRAD)
    calls = []
    real = CI.conv3x3_bf16x3_nhwc
    CI.conv3x3_bf16x3_nhwc = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        CI.BF16X3 = CI.BF16X3_DGRAD = False
        with torch.no_grad():      # outputs within rounding of the ReLU threshold may land on either side of it
            g = g * (m(x).abs() > 1e-4)
        assert not calls
        outs = []
        for on in (True, False):
            CI.BF16X3 = CI.BF16X3_DGRAD = on
            xi = x.clone().requires_grad_(True)
            m.zero_grad()
            y = m(xi)
            y.backward(g)
            outs.append((y.detach(), xi.grad, m.conv.weight.grad.clone(), m.conv.bias.grad.clone()))
            assert len(calls) == 2, calls          # the route's forward + data gradient; the fp32 pass adds none
        for name, a, b in zip(("y", "grad_x", "grad_w", "grad_b"), *outs):
            err, bound = (a - b).abs().max().item(), 2e-4 * b.abs().max().item() + 1e-6
            print("%s: max difference %.3e bound %.3e" % (name, err, bound))
            assert err <= bound
        CI.BF16X3 = True
        with torch.no_grad():
            assert torch.equal(m(x), outs[0][0])          # the no-grad route is the same kernel
        assert len(calls) == 3
        assert (outs[0][0] == 0).float().mean().item() > 0.2     # the ReLU is active
        # the weight updated behind its version counter (as the fused multi-tensor SGD step does): the flipped weights of
        # the split data gradient follow (tests/test_gpu_conv_rows.py makes the same check for the rows route)
        v = m.conv.weight._version
        m.conv.weight.data.mul_(-1.5)
        assert m.conv.weight._version == v
        CI.BF16X3 = CI.BF16X3_DGRAD = False
        with torch.no_grad():      # (the outputs near the ReLU threshold are other ones now)
            g = g * (m(x).abs() > 1e-4)
        outs = []
        for on in (True, False):
            CI.BF16X3 = CI.BF16X3_DGRAD = on
            xi = x.clone().requires_grad_(True)
            m.zero_grad()
            m(xi).backward(g)
            outs.append((xi.grad, m.conv.weight.grad.clone(), m.conv.bias.grad.clone()))
        assert len(calls) == 5
        for name, a, b in zip(("grad_x", "grad_w", "grad_b"), *outs):
            err, bound = (a - b).abs().max().item(), 2e-4 * b.abs().max().item() + 1e-6
            print("after the update, %s: max difference %.3e bound %.3e" % (name, err, bound))
            assert err <= bound
    finally:
        CI.BF16X3, CI.BF16X3_DGRAD = saved
        CI.conv3x3_bf16x3_nhwc = real
