"""usage (GPU box): python scripts/conv_rows_fwd_timing.py [--iters 20] -- HIP-event times of the entry points of
include/jdet_hip.h (jdet_rows_from_flags; jdet_conv3x3_rows_forward incl. its zero fill) at the S2ANet ODM
regression tower's shapes (P3: 2 x 128 x 128, the packed P4..P7 canvas: 2 x 64 x 97; 256 -> 256 channels, bias + ReLU),
beside the dense forward (csrc/conv_igemm.hip) in the same process on the same device.  Flags: a few seed rows per map
(the positive anchors of profiles/conv_rows.md) -- the tower's second layer then runs on their first dilation, its
first layer on the second -- random rows at 5 .. 50 %, and every row: the density at which the gathered forward crosses
the dense kernel is read off these lines.  One JSON line per (shape, flags)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jdet_amd.ops import conv_igemm as CI  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()


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


# (name, N, H, W, seed rows of both images: the positive anchors of profiles/conv_rows.md)
SHAPES = (("P3", 2, 128, 128, 78), ("pack P4..P7", 2, 64, 97, 221))
C = 256
for name, n, h, w, seeds in SHAPES:
    P = n * h * w
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(n, h, w, C, device="cuda")
    wt = (torch.randn(C, 3, 3, C, device="cuda") * 0.02).contiguous()
    b = torch.randn(C, device="cuda") * 0.1
    dense = lambda: CI.conv3x3_nhwc(x, wt, b, True)  # noqa: E731
    ref = dense()
    dense_us = timeit(dense)
    cases = [("seeds x%d" % seeds, seeds)] + [("random %d %%" % round(100 * f), f) for f in (0.05, 0.25, 0.5)] + [("all rows", 2.0)]
    for label, arg in cases:
        flags = torch.zeros(P, dtype=torch.bool)
        if isinstance(arg, int):
            flags[torch.randperm(P, generator=gen)[:arg]] = True
        else:
            flags = torch.rand(P, generator=gen) < arg
        flags = flags.cuda()
        lists = CI.rows_from_flags(flags, n, h, w)
        counts = [int(v) for v in lists[3].cpu()]
        line = dict(shape=name, positions=P, flags=label, rows=counts, dense_forward_us=dense_us,
                    rows_from_flags_us=timeit(lambda: CI.rows_from_flags(flags, n, h, w)))
        for k in (0, 1, 2):        # the gathered forward on the list after k dilations
            fwd = lambda: CI.conv3x3_rows_forward_nhwc(x, wt, b, True, None, lists[k], lists[3].data_ptr() + 4 * k)  # noqa: E731
            got = fwd()
            listed = torch.zeros(P, dtype=torch.bool, device="cuda")
            listed[lists[k][:counts[k]].long()] = True
            err = float(((got - ref).reshape(P, C)[listed]).abs().max() / ref.abs().max()) if counts[k] else 0.0
            assert err < 1e-4 and not got.reshape(P, C)[~listed].any(), (label, k, err)
            line["rows_forward_d%d_us" % k] = timeit(fwd)
        # what the tower pays: the lists once, layer 1 on the second dilation, layer 2 on the first -- against two dense layers
        line["tower_rows_us"] = round(line["rows_from_flags_us"] + line["rows_forward_d2_us"] + line["rows_forward_d1_us"], 1)
        line["tower_dense_us"] = round(2 * dense_us, 1)
        print(json.dumps(line), flush=True)
