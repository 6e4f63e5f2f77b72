"""usage (GPU box): python scripts/conv_rows_timing.py [--iters 20] -- HIP-event times of the three entry points of
csrc/conv_rows.hip (jdet_rows_nonzero, jdet_conv3x3_wgrad_rows, jdet_conv3x3_dgrad_rows incl. its zero fill) at the
S2ANet regression towers' shapes (P3: 2 x 128 x 128, the packed P4..P7 canvas: 2 x 64 x 97; 256 -> 256 channels), beside
the dense data gradient (the library's, autotuned) and the dense weight gradient (csrc/conv_wgrad.hip) in the same
process on the same device.  Gradients: a few seed rows per map dilated 0 / 1 / 2 times (the row sets the tower layers see,
profiles/conv_rows.md), random rows at 5 .. 50 %, and a fully dense gradient -- the density at which the rows path
crosses the dense kernels is read off these lines.  One JSON line per (shape, gradient)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jdet_amd.ops import conv_igemm as CI  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
torch.backends.cudnn.benchmark = True


def timeit(fn, iters=args.iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters * 1e3, 1)


def row_mask(n, h, w, kind, arg, gen):
    """(n, h, w) bool: `seeds` random rows dilated `arg[1]` times, or random rows at density `arg`"""
    if kind == "seeds":
        m = torch.zeros(n * h * w, dtype=torch.bool)
        m[torch.randperm(n * h * w, generator=gen)[:arg[0]]] = True
        m = m.view(n, 1, h, w).float()
        for _ in range(arg[1]):
            m = F.max_pool2d(m, 3, 1, 1)
        return m.view(n, h, w) > 0
    return torch.rand(n, h, w, generator=gen) < arg


# (name, N, H, W, seed rows of both images: the positive anchors of profiles/conv_rows.md)
SHAPES = (("P3", 2, 128, 128, 78), ("pack P4..P7", 2, 64, 97, 221))
C = 256
for name, n, h, w, seeds in SHAPES:
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(n, C, h, w, device="cuda").contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(C, C, 3, 3, device="cuda") * 0.02).contiguous(memory_format=torch.channels_last)
    wd = wt.flip(2, 3).permute(1, 2, 3, 0).contiguous()
    xn = x.permute(0, 2, 3, 1)
    gw = torch.zeros(C, 3, 3, C, device="cuda")
    cases = [("seeds x%d dilated %d" % (seeds, d), "seeds", (seeds, d)) for d in (0, 1, 2)]
    cases += [("random %d %%" % round(100 * f), "random", f) for f in (0.05, 0.1, 0.25, 0.5)] + [("dense", "random", 2.0)]
    for label, kind, arg in cases:
        mask = row_mask(n, h, w, kind, arg, gen).cuda()
        g = (torch.randn(n, h, w, C, device="cuda") * mask[..., None]).permute(0, 3, 1, 2)       # channels-last memory
        gn = g.permute(0, 2, 3, 1)
        _, rows, drows, counts = CI.rows_nonzero(gn)
        c0, c1 = (int(v) for v in counts.cpu())
        dense_dgrad = lambda: torch.ops.aten.convolution_backward(g, x, wt, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                                  [True, False, False])
        ref = dense_dgrad()[0].permute(0, 2, 3, 1)
        got = CI.conv3x3_dgrad_rows_nhwc(gn, wd, drows, counts.data_ptr() + 4)
        err = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
        line = dict(shape=name, positions=n * h * w, gradient=label, rows=c0, rows_dilated=c1,
                    rows_nonzero_us=timeit(lambda: CI.rows_nonzero(gn)),
                    wgrad_rows_us=timeit(lambda: CI.conv3x3_wgrad_nhwc(xn, gn, out=gw, rows=(rows, counts.data_ptr()))),
                    dgrad_rows_us=timeit(lambda: CI.conv3x3_dgrad_rows_nhwc(gn, wd, drows, counts.data_ptr() + 4)),
                    dense_wgrad_us=timeit(lambda: CI.conv3x3_wgrad_nhwc(xn, gn, out=gw)),
                    dense_dgrad_us=timeit(dense_dgrad), dgrad_rel_err=float("%.2e" % err))
        line["rows_path_us"] = round(line["rows_nonzero_us"] + line["wgrad_rows_us"] + line["dgrad_rows_us"], 1)
        line["dense_path_us"] = round(line["dense_wgrad_us"] + line["dense_dgrad_us"], 1)
        print(json.dumps(line), flush=True)
