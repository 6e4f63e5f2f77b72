"""GPU: the buffer promises of include/jdet_hip_rows.h by the guard-band / poison protocol of tests/guarded.py, in the
manner of tests/test_gpu_abi_buffers.py: a clean run A, a hostile run B (canaries in the outputs and around every
buffer, a 0xFF workspace, NaN next to every float input, position 0 next to every list), B == A bit for bit where the
kernel is deterministic, both within the bound of the kernels' own test (tests/test_gpu_conv_rows.py), nothing written
outside the documented extents, and a workspace claim one byte short refused with JDET_E_WORKSPACE."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = (2e-5, 1e-6)          # tests/test_gpu_conv_rows.py (= tests/test_gpu_conv_igemm.py:45, test_gpu_conv_wgrad.py:48)
SHAPES = [(2, 13, 17, 64, 64), (1, 8, 8, 256, 256), (2, 20, 24, 32, 256)]


def _inputs(shape, frac):
    N, H, W, Cin, Cout = shape
    P = N * H * W
    rng = np.random.default_rng(N * 1000 + H * 100 + W + Cin + int(frac * 64))
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * (2.0 / (9 * Cin)) ** 0.5).astype(np.float32)
    rows = np.sort(rng.choice(P, max(1, int(round(frac * P))), replace=False))
    rows = np.unique(np.concatenate([rows, [0, W - 1, H * W - 1, P - 1]]))        # corners and the image boundary
    g = np.zeros((P, Cout), np.float32)
    g[rows] = rng.standard_normal((len(rows), Cout)).astype(np.float32)
    nz = np.zeros(P, bool)
    nz[rows] = True
    pad = np.pad(nz.reshape(N, H, W), ((0, 0), (1, 1), (1, 1)))
    dil = np.zeros((N, H, W), bool)
    for dy in range(3):
        for dx in range(3):
            dil |= pad[:, dy:dy + H, dx:dx + W]
    return x, w, g.reshape(N, H, W, Cout), rows.astype(np.int32), np.flatnonzero(dil.reshape(-1)).astype(np.int32)


def _reference(x, w, g):
    x64 = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = torch.from_numpy(w).double().requires_grad_(True)
    gx, gw = torch.autograd.grad(F.conv2d(x64, w64, None, 1, 1), (x64, w64), torch.from_numpy(g).double().permute(0, 3, 1, 2))
    return gx.permute(0, 2, 3, 1).contiguous(), gw.permute(0, 2, 3, 1).contiguous()


def _padded(a, n):
    out = np.full(n, -1, np.int32)
    out[:len(a)] = a
    return out


def _case(entry, shape, frac):
    from tests.abi_cases import I32, U8, P as PTR, ST, Case, Res, exact, rel
    from jdet_amd import _lib as L
    N, H, W, Cin, Cout = shape
    P = N * H * W
    x0, w0, g0, rows0, drows0 = _inputs(shape, frac)

    def nonzero(run):
        lib = L.lib()
        g = run.inp("g", g0)
        flags, rows, drows = run.out("flags", (P,), U8), run.out("rows", (P,), I32), run.out("rows_dilated", (P,), I32)
        counts = run.out("counts", (2,), I32)
        ws, wsb = run.ws("workspace", lib.jdet_rows_nonzero_workspace(N, H, W))
        run.ok(lib.jdet_rows_nonzero(PTR(g), N, H, W, Cout, PTR(flags), PTR(rows), PTR(drows), PTR(counts), PTR(ws), wsb,
                                     ST(g)), entry)
        want = np.zeros(P, np.uint8)
        want[rows0] = 1
        return Res({"flags": flags, "rows": rows, "rows_dilated": drows, "counts": counts},
                   lambda: {"flags": exact(want), "rows": exact(_padded(rows0, P)),
                            "rows_dilated": exact(_padded(drows0, P)),
                            "counts": exact(np.asarray([len(rows0), len(drows0)], np.int32))})

    def wgrad(run):
        x, g = run.inp("x", x0), run.inp("gy", g0)
        rows, count = run.inp("rows", rows0), run.inp("count", np.asarray([len(rows0)], np.int32))     # no entry past the count
        base = np.random.default_rng(5).standard_normal((Cout, 3, 3, Cin)).astype(np.float32)
        gw = run.acc("gw", base)
        run.ok(L.lib().jdet_conv3x3_wgrad_rows(PTR(x), PTR(g), PTR(rows), PTR(count), N, H, W, Cin, Cout, PTR(gw), ST(x)),
               entry)

        def ref():
            # the value is out - base in float64, so the fp32 roundings of adding onto the base count as error: at most
            # jdet_conv3x3_wgrad_rows_workers() workgroups add to an element, each addition rounds by at most 2^-24 of the
            # running value
            r, bound = rel(_reference(x0, w0, g0)[1], *BOUND)
            return {"gw": (r, bound + L.lib().jdet_conv3x3_wgrad_rows_workers(Cin, Cout) * 2.0 ** -24 * float(np.abs(base).max() + np.abs(r).max()))}
        return Res({"gw": gw}, ref, atomic=True)

    def dgrad(run):
        g = run.inp("gy", g0)
        wd = run.inp("wd", np.ascontiguousarray(w0[:, :, ::-1, ::-1].transpose(1, 2, 3, 0)))
        rows, count = run.inp("rows", drows0), run.inp("count", np.asarray([len(drows0)], np.int32))
        gx = run.out("gx", (N, H, W, Cin))
        run.ok(L.lib().jdet_conv3x3_dgrad_rows(PTR(g), PTR(wd), PTR(rows), PTR(count), N, H, W, Cin, Cout, 1, PTR(gx),
                                               ST(g)), entry)
        return Res({"gx": gx}, lambda: {"gx": rel(_reference(x0, w0, g0)[0], *BOUND)})

    fn = {"jdet_rows_nonzero": nonzero, "jdet_conv3x3_wgrad_rows": wgrad, "jdet_conv3x3_dgrad_rows": dgrad}[entry]
    return Case((entry,), "x(%d,%d,%d,%d) Cout %d rows %.0f%%" % (N, H, W, Cin, Cout, 100 * frac), fn)


@pytest.mark.parametrize("frac", [0.03, 1.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("entry", ["jdet_rows_nonzero", "jdet_conv3x3_wgrad_rows", "jdet_conv3x3_dgrad_rows"])
def test_buffer_contract(dev, entry, shape, frac):
    from tests import guarded
    case = _case(entry, shape, frac)
    guarded.run_case(case.entry_points[0], case.label, case.fn, dev)


def test_dgrad_without_zero_fill_writes_the_listed_rows_only(dev):
    """zero_first = 0: rows of gx outside the list keep what they held, bit for bit"""
    from jdet_amd import _lib as L
    shape = SHAPES[0]
    N, H, W, Cin, Cout = shape
    x0, w0, g0, rows0, drows0 = _inputs(shape, 0.03)
    g = torch.from_numpy(g0).to(dev)
    wd = torch.from_numpy(np.ascontiguousarray(w0[:, :, ::-1, ::-1].transpose(1, 2, 3, 0))).to(dev)
    rows, count = torch.from_numpy(drows0).to(dev), torch.tensor([len(drows0)], dtype=torch.int32, device=dev)
    gx = torch.full((N * H * W, Cin), 3.25, device=dev)
    L.check(L.lib().jdet_conv3x3_dgrad_rows(g.data_ptr(), wd.data_ptr(), rows.data_ptr(), count.data_ptr(), N, H, W, Cin,
                                            Cout, 0, gx.data_ptr(), L.stream_ptr(g)), "jdet_conv3x3_dgrad_rows")
    keep = torch.ones(N * H * W, dtype=torch.bool, device=dev)
    keep[rows.long()] = False
    assert bool((gx[keep] == 3.25).all()) and not bool((gx[~keep] == 3.25).all(1).any())
