"""GPU: the buffer promises of include/jdet_hip_rows_fwd.h by the guard-band / poison protocol of tests/guarded.py, as
tests/test_gpu_conv_rows_abi.py has them for jdet_hip_rows.h: a clean run A, a hostile run B (canaries in the outputs and
around every buffer, a 0xFF workspace, NaN next to every float input, position 0 next to every list), B == A bit for
bit, both within the bound of the kernels' own test (tests/test_gpu_conv_rows_fwd.py), nothing written outside the
documented extents, and a workspace claim one byte short refused with JDET_E_WORKSPACE."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = (2e-5, 1e-6)          # tests/test_gpu_conv_rows_fwd.py (= tests/test_gpu_conv_igemm.py:45)
SHAPES = [(2, 13, 17, 64, 64), (1, 8, 8, 256, 256), (2, 20, 24, 32, 256)]


def _dilate(nz):
    N, H, W = nz.shape
    pad = np.pad(nz, ((0, 0), (1, 1), (1, 1)))
    out = np.zeros_like(nz)
    for dy in range(3):
        for dx in range(3):
            out |= pad[:, dy:dy + H, dx:dx + W]
    return out


def _inputs(shape, frac):
    N, H, W, Cin, Cout = shape
    P = N * H * W
    rng = np.random.default_rng(N * 1000 + H * 100 + W + Cin + int(frac * 64) + 1)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * (2.0 / (9 * Cin)) ** 0.5).astype(np.float32)
    b = (0.3 * rng.standard_normal(Cout)).astype(np.float32)
    rows = np.sort(rng.choice(P, max(1, int(round(frac * P))), replace=False))
    rows = np.unique(np.concatenate([rows, [0, W - 1, H * W - 1, P - 1]]))        # corners and the image boundary
    mask = (rng.random(P) > 0.2).astype(np.float32)
    return x, w, b, rows.astype(np.int32), mask


def _padded(a, n):
    out = np.full(n, -1, np.int32)
    out[:len(a)] = a
    return out


def _case(entry, shape, frac):
    from tests.abi_cases import I32, P as PTR, ST, Case, Res, exact, rel
    from jdet_amd import _lib as L
    N, H, W, Cin, Cout = shape
    P = N * H * W
    x0, w0, b0, rows0, mask0 = _inputs(shape, frac)

    def from_flags(run):
        lib = L.lib()
        f0 = np.zeros(P, np.uint8)
        f0[rows0] = 1 + (rows0 % 200).astype(np.uint8)          # any non-zero byte is a flag
        flags = run.inp("flags", f0)
        outs = [run.out(n, (P,), I32) for n in ("rows", "rows_dilated", "rows_dilated2")]
        counts = run.out("counts", (3,), I32)
        ws, wsb = run.ws("workspace", lib.jdet_rows_from_flags_workspace(N, H, W))
        run.ok(lib.jdet_rows_from_flags(PTR(flags), N, H, W, PTR(outs[0]), PTR(outs[1]), PTR(outs[2]), PTR(counts),
                                        PTR(ws), wsb, ST(flags)), entry)
        nz = (f0 != 0).reshape(N, H, W)
        want = [np.flatnonzero(nz), np.flatnonzero(_dilate(nz)), np.flatnonzero(_dilate(_dilate(nz)))]
        return Res({"rows": outs[0], "rows_dilated": outs[1], "rows_dilated2": outs[2], "counts": counts},
                   lambda: {"rows": exact(_padded(want[0], P)), "rows_dilated": exact(_padded(want[1], P)),
                            "rows_dilated2": exact(_padded(want[2], P)),
                            "counts": exact(np.asarray([len(v) for v in want], np.int32))})

    def forward(run):
        x = run.inp("x", x0)
        w = run.inp("w", np.ascontiguousarray(w0.transpose(0, 2, 3, 1)))
        b, mask = run.inp("bias", b0), run.inp("rowmask", mask0)
        rows, count = run.inp("rows", rows0), run.inp("count", np.asarray([len(rows0)], np.int32))   # no entry past the count
        y = run.out("y", (N, H, W, Cout))
        run.ok(L.lib().jdet_conv3x3_rows_forward(PTR(x), PTR(w), PTR(b), 1, PTR(mask), PTR(rows), PTR(count), N, H, W,
                                                 Cin, Cout, 1, PTR(y), ST(x)), entry)

        def ref():
            pre = F.conv2d(torch.from_numpy(x0).double().permute(0, 3, 1, 2), torch.from_numpy(w0).double(),
                           torch.from_numpy(b0).double(), 1, 1).permute(0, 2, 3, 1).reshape(P, Cout).numpy()
            keep = np.zeros(P)
            keep[rows0] = mask0[rows0]
            full = np.maximum(pre, 0.0)
            r, bound = rel(full, *BOUND)               # the bound of the whole map's scale; unlisted / masked rows are 0
            return {"y": ((full * keep[:, None]).reshape(N, H, W, Cout), bound)}
        return Res({"y": y}, ref)

    fn = {"jdet_rows_from_flags": from_flags, "jdet_conv3x3_rows_forward": forward}[entry]
    return Case((entry,), "x(%d,%d,%d,%d) Cout %d rows %.0f%%" % (N, H, W, Cin, Cout, 100 * frac), fn)


@pytest.mark.parametrize("frac", [0.03, 1.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("entry", ["jdet_rows_from_flags", "jdet_conv3x3_rows_forward"])
def test_buffer_contract(dev, entry, shape, frac):
    from tests import guarded
    case = _case(entry, shape, frac)
    guarded.run_case(case.entry_points[0], case.label, case.fn, dev)
