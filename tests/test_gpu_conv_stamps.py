"""The profiling build of the conv_bn kernel (csrc/experimental/conv_bn_stamps.hip, libjdet_experimental.so -- not a product
path): outside the 16 stamp words of every (M tile, N tile) its output is bit-equal to the product's same kernel
(conv_bn_nhwc(..., tile=66) = the 64 x 64 tile, 32-deep K steps, one wave group, operand tiles two steps ahead: the same
operation order), and the stamp words hold what scripts/r6_conv_stamps.py reads."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _stamps(x, w, bn, relu):
    from jdet_amd import _experimental as X
    from jdet_amd import _lib as L
    from jdet_amd.ops import conv_bn as CB
    N, H, W, Cin = x.shape
    Cout, R = w.shape[0], w.shape[1]
    y = torch.empty((N, CB.out_size(H, R, 1), CB.out_size(W, R, 1), Cout), dtype=torch.float32, device=x.device)
    ep = CB.epilogue(L.EPI_FORWARD, bn, relu)
    status = X.lib().jdet_conv_bn_forward_stamps(L.ptr(x), N, H, W, Cin, L.ptr(w), Cout, R, 1, ctypes.byref(ep), L.ptr(y),
                                                 L.stream_ptr(x))
    torch.cuda.synchronize()
    return status, y


def test_stamps_build_equals_the_product_kernel_outside_its_stamp_words(dev):
    from jdet_amd.ops import conv_bn as CB
    g = torch.Generator().manual_seed(7)
    N, H, W, Cin, Cout, R = 1, 9, 15, 64, 128, 3           # M = 135: three M tiles, the last ragged; two N tiles
    x = torch.randn(N, H, W, Cin, generator=g).to(dev)
    w = (torch.randn(Cout, R, R, Cin, generator=g) / (R * Cin ** 0.5)).to(dev)
    bn = torch.nn.BatchNorm2d(Cout)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(Cout, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(Cout, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(Cout, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(Cout, generator=g) + 0.5)
    bn = bn.to(dev).eval()
    ref = CB.conv_bn_nhwc(x, w, 1, bn, None, True, tile=66)
    status, y = _stamps(x, w, bn, True)
    assert status == 0
    M = N * H * W
    y2, ref2 = y.reshape(M, Cout), ref.reshape(M, Cout)
    stamped = torch.zeros((M, Cout), dtype=torch.bool, device=dev)
    words = []
    for m0 in range(0, M, 64):
        for n0 in range(0, Cout, 64):
            stamped[m0, n0:n0 + 16] = True
            words.append(y2[m0, n0:n0 + 16].contiguous().view(torch.int32).cpu().numpy().astype(np.int64))
    assert torch.equal(y2[~stamped], ref2[~stamped])
    words = np.stack(words)
    assert len(words) == 6
    assert (words[:, 11] == 0x5741).all()
    assert sorted(words[:, 10]) == list(range(6))                     # distinct workgroup ids below 6
    t = np.stack([(words[:, 2 * k] & 0xffffffff) | (words[:, 2 * k + 1] << 32) for k in range(4)], 1)
    assert (np.diff(t, axis=1) >= 0).all(), t                          # start <= K loop entered <= K loop left <= end

    status, _ = _stamps(torch.randn(N, H, W, 48, device=dev), torch.randn(Cout, R, R, 48, device=dev), bn, True)
    assert status == -2                                                # JDET_E_UNSUPPORTED: Cin % 32 != 0
