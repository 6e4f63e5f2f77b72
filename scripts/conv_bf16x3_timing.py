"""usage (GPU box): python scripts/conv_bf16x3_timing.py  -- the bf16 three-way-split 3x3 convolution
(csrc/conv_bf16x3.hip) beside the fp32-MFMA kernel and the library's data gradient, per shape of the `big` rule
(256 -> 256 channels, batch 2 and 4 at 128^2, batch 2 at 256^2) plus one packed-level shape below the rule for reference.
Random data (never zeros: the clock a bf16 MFMA loop holds depends on its operands)."""
import json
import sys

import torch

sys.path.insert(0, ".")
from jdet_amd.ops import conv_igemm as CI   # noqa: E402


def timeit(fn, iters=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


for N, hw, C in ((2, 128, 256), (4, 128, 256), (2, 256, 256), (2, 64, 256)):
    x = torch.randn(N, C, hw, hw, device="cuda").contiguous(memory_format=torch.channels_last)
    w = (torch.randn(C, C, 3, 3, device="cuda") * 0.02).contiguous(memory_format=torch.channels_last)
    b = torch.randn(C, device="cuda")
    g = torch.randn(N, C, hw, hw, device="cuda").contiguous(memory_format=torch.channels_last)
    xn, wk = x.permute(0, 2, 3, 1), CI.weight_krsc(w)
    flop = 2.0 * N * hw * hw * C * C * 9
    row = dict(N=N, hw=hw, C=C, big=bool(CI.bf16x3_big(N * hw * hw, C, C)))
    row["fp32_us"] = t32 = round(timeit(lambda: CI.conv3x3_nhwc(xn, wk, b, True, bf16x3=False)), 1)
    row["bf16x3_us"] = t16 = round(timeit(lambda: CI.conv3x3_bf16x3_nhwc(xn, wk, b, True)), 1)
    row["fp32_tflops"], row["bf16x3_tflops"] = round(flop / t32 / 1e6, 1), round(flop / t16 / 1e6, 1)
    row["lib_dgrad_us"] = round(timeit(lambda: torch.ops.aten.convolution_backward(
        g, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False])), 1)
    y32 = CI.conv3x3_nhwc(xn, wk, b, True, bf16x3=False)
    y16 = CI.conv3x3_bf16x3_nhwc(xn, wk, b, True)
    row["max_diff_over_max"] = float((y32 - y16).abs().max() / y32.abs().max())
    print(json.dumps(row), flush=True)
