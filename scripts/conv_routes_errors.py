"""The framework route's own error against float64 at the shapes of tests/conv_route_cases.py: every case of the table,
tolerance tier, as F.conv2d [+ relu] [* mask] and its autograd on the device in fp32 (no code of ops/conv_igemm.py runs).
The largest |err| / max|ref| per output kind is LIBRARY_ERR of the case module, from which the bound for the outputs a
route leaves to the library, a GEMM or the framework is formed (profiles/conv_routes.md).

    python scripts/conv_routes_errors.py"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import conv_route_cases as K  # noqa: E402


def rel_err(got, ref):
    if got is None or not ref.size:
        return 0.0
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - ref).max())
    return err / float(np.abs(ref).max()) if err else 0.0


def framework(dev, c, inp):
    fmt = lambda t, f: t.contiguous(memory_format=torch.channels_last) if f == "cl" else t.contiguous()
    dv = lambda a: torch.from_numpy(np.array(a)).to(dev)
    w = fmt(dv(inp.w), c.wfmt).requires_grad_(c.need[1])
    b = dv(inp.b).requires_grad_(c.need[2]) if c.bias else None
    xs = [fmt(dv(x), c.xfmt).requires_grad_(c.need[0]) for x in inp.x]
    ys = []
    for p in range(c.passes):
        row = []
        for u, x in enumerate(xs):
            y = F.conv2d(x, w, b, c.stride, c.pad, c.dil, c.groups)
            y = torch.relu(y) if c.relu else y
            if inp.mask[u] is not None:
                y = y * dv(inp.mask[u]).view(x.shape[0], 1, x.shape[2], x.shape[3])
            row.append(y)
        torch.autograd.backward(row, [fmt(dv(g), "nchw" if f == "nchw" else "cl") for g, f in zip(inp.g, c.grad)])
        ys.append([y.detach() for y in row])
        if p + 1 < c.passes:
            w.data.mul_(c.rescale)
    return ys, xs, w, b


def main():
    dev = torch.device("cuda:0")
    worst = {k: 0.0 for k in K.KINDS}
    seen = set()
    for c in K.CASES:
        if (c.data, c.passes) in seen or c.data != c.name:
            continue                                     # (the switch cases share their base's inputs)
        seen.add((c.data, c.passes))
        inp, ref = K.inputs_of(c, "tolerance"), K.reference(c, "tolerance")
        ys, xs, w, b = framework(dev, c, inp)
        err = {"y": max(rel_err(ys[p][u], ref.y[p][u]) for p in range(c.passes) for u in range(len(xs))),
               "grad_x": max(rel_err(x.grad, ref.grad_x[u]) for u, x in enumerate(xs)) if c.need[0] else 0.0,
               "grad_w": rel_err(w.grad, ref.grad_w) if c.need[1] else 0.0,
               "grad_b": rel_err(b.grad, ref.grad_b) if c.bias and c.need[2] else 0.0}
        print("conv_routes | framework | %s | %s" % (c.name, " | ".join("%s %.3e" % (k, err[k]) for k in K.KINDS)), flush=True)
        worst = {k: max(worst[k], err[k]) for k in K.KINDS}
    print("conv_routes | framework | LIBRARY_ERR = {%s}" % ", ".join('"%s": %.1e' % (k, worst[k]) for k in K.KINDS))


if __name__ == "__main__":
    main()
