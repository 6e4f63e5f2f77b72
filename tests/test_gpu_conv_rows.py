"""GPU: the row-sparse backward of the regression towers' 3x3 convolutions (csrc/conv_rows.hip):
the device-side row lists against numpy, both gradients against float64 conv2d autograd on the CPU at the bound of the
igemm / weight-gradient tests (|err| <= 2e-5 max|ref| + 1e-6), exact zeros outside the dilated list, accumulation,
count 0, a data gradient without the zero fill, the ConvModule route against the dense route, and a captured backward
replayed with other gradients."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(2, 13, 17, 64, 64),        # odd sizes and an image boundary
          (1, 8, 8, 256, 256),        # single image, full channel count
          (2, 20, 24, 32, 256)]       # narrow Cin
PATTERNS = ["zero", "borders", "random3", "dense", "negzero_nan"]
REL, ABS = 2e-5, 1e-6                 # tests/test_gpu_conv_igemm.py:45, tests/test_gpu_conv_wgrad.py:48


def _rows_of(pattern, N, H, W, rng):
    P = N * H * W
    if pattern == "zero":
        return np.zeros(0, np.int64)
    if pattern == "borders":       # the four corners, one row on each edge, the last row of image 0 / the first of image 1
        yx = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)]
        rows = [y * W + x for y, x in yx]
        if N > 1:
            rows += [H * W - 1, H * W]
        return np.unique(np.asarray(rows, np.int64))
    if pattern == "random3":
        return np.sort(rng.choice(P, max(1, int(round(0.03 * P))), replace=False))
    if pattern == "dense":
        return np.arange(P)
    raise KeyError(pattern)


@functools.lru_cache(maxsize=None)
def _case(shape, pattern):
    """inputs and the float64 CPU reference of one (shape, pattern), computed once and shared"""
    N, H, W, Cin, Cout = shape
    P = N * H * W
    rng = np.random.default_rng(1000 * SHAPES.index(shape) + PATTERNS.index(pattern))
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * (2.0 / (9 * Cin)) ** 0.5).astype(np.float32)
    g = np.zeros((P, Cout), np.float32)
    if pattern == "negzero_nan":
        rows = np.sort(rng.choice(P, 6, replace=False))
        g[rows] = rng.standard_normal((6, Cout)).astype(np.float32)
        interior = [p for p in range(P) if 0 < (p % (H * W)) // W < H - 1 and 0 < p % W < W - 1 and p not in set(rows)]
        neg, nan = interior[len(interior) // 3], interior[2 * len(interior) // 3]
        g[neg] = -0.0                                   # a row of -0.0 only: dropped
        g[nan, Cout // 2] = np.nan                      # a row of zeros and one NaN: kept
    else:
        rows = _rows_of(pattern, N, H, W, rng)
        g[rows] = rng.standard_normal((len(rows), Cout)).astype(np.float32)
    g = g.reshape(N, H, W, Cout)
    x64 = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = torch.from_numpy(w).double().requires_grad_(True)
    y = F.conv2d(x64, w64, None, 1, 1)
    gx, gw = torch.autograd.grad(y, (x64, w64), torch.from_numpy(g).double().permute(0, 3, 1, 2))
    ref = dict(gx=gx.permute(0, 2, 3, 1).contiguous().numpy(), gw=gw.permute(0, 2, 3, 1).contiguous().numpy())
    nz = ((g.view(np.uint32) & 0x7FFFFFFF) != 0).any(-1)                       # (N, H, W)
    pad = np.pad(nz, ((0, 0), (1, 1), (1, 1)))
    dil = np.zeros_like(nz)
    for dy in range(3):
        for dx in range(3):
            dil |= pad[:, dy:dy + H, dx:dx + W]
    ref["rows"], ref["drows"] = np.flatnonzero(nz.reshape(-1)), np.flatnonzero(dil.reshape(-1))
    return x, w, g, ref


def _close(val, ref, scale=1.0, extra=0.0):
    """|val - ref| <= scale * (REL max|ref| + ABS) + extra over the finite entries; NaN exactly where the reference has it"""
    val = val.detach().cpu().double().numpy() if isinstance(val, torch.Tensor) else np.asarray(val, np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(val), nan), "NaN in %d places, reference in %d" % (np.isnan(val).sum(), nan.sum())
    fin = ~nan
    top = float(np.abs(ref[fin]).max()) if fin.any() else 0.0
    err = float(np.abs(val[fin] - ref[fin]).max()) if fin.any() else 0.0
    bound = scale * (REL * top + ABS) + extra
    print("max err %.3e bound %.3e (max|ref| %.3e)" % (err, bound, top))
    assert err <= bound, (err, bound)


def _wd(w):
    """(Cout, Cin, 3, 3) -> the flipped (Cin, 3, 3, Cout) data-gradient weights"""
    return w.flip(2, 3).permute(1, 2, 3, 0).contiguous()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rows_lists_and_gradients(dev, shape, pattern):
    from jdet_amd.ops import conv_igemm as CI
    N, H, W, Cin, Cout = shape
    P = N * H * W
    x0, w0, g0, ref = _case(shape, pattern)
    x, w, g = (torch.from_numpy(a).to(dev) for a in (x0, w0, g0))
    scratch = torch.full((8 * P + 16 + CI.L.lib().jdet_rows_nonzero_workspace(N, H, W) + P,), 0xA5, dtype=torch.uint8,
                         device=dev)
    flags, rows, drows, counts = CI.rows_nonzero(g, scratch)
    c0, c1 = (int(v) for v in counts.cpu())
    # ---- lists and counts: numpy.nonzero of the row test and of its dilation, ascending, -1 behind ----
    assert c0 == len(ref["rows"]) and c1 == len(ref["drows"])
    assert np.array_equal(rows.cpu().numpy()[:c0], ref["rows"]) and bool((rows[c0:] == -1).all())
    assert np.array_equal(drows.cpu().numpy()[:c1], ref["drows"]) and bool((drows[c1:] == -1).all())
    want_flags = np.zeros(P, np.uint8)
    want_flags[ref["rows"]] = 1
    assert np.array_equal(flags.cpu().numpy(), want_flags)
    if pattern == "negzero_nan":
        nan_row = int(np.flatnonzero(np.isnan(g0.reshape(P, Cout)).any(1))[0])
        neg_row = int(np.flatnonzero(np.signbit(g0.reshape(P, Cout)).all(1))[0])
        assert nan_row in ref["rows"] and neg_row not in ref["rows"] and c0 == 7
    # ---- gx: the listed rows against float64, every other row exactly zero ----
    gx = CI.conv3x3_dgrad_rows_nhwc(g, _wd(w), drows, counts.data_ptr() + 4)
    _close(gx, ref["gx"])
    if pattern != "negzero_nan":
        outside = np.ones(P, bool)
        outside[ref["drows"]] = False
        assert not gx.reshape(P, Cin).cpu().numpy()[outside].any()
    # ---- gW: from a zero buffer, then accumulated twice onto a base ----
    gw = CI.conv3x3_wgrad_nhwc(x, g, rows=(rows, counts.data_ptr()))
    _close(gw, ref["gw"])
    fin = ref["gw"][~np.isnan(ref["gw"])]
    top = float(np.abs(fin).max()) if fin.size else 0.0
    base = (torch.randn(Cout, 3, 3, Cin, device=dev) * (0.5 * top if top else 1.0)).contiguous()
    acc = base.clone()
    for _ in range(2):
        CI.conv3x3_wgrad_nhwc(x, g, out=acc, rows=(rows, counts.data_ptr()))
    if c0 == 0:
        assert torch.equal(acc, base) and not gx.any() and not gw.any()      # count 0: nothing added, bit for bit
    else:
        # two calls' own error, plus the fp32 roundings of adding onto the base: per call at most
        # jdet_conv3x3_wgrad_rows_workers() workgroups add a partial sum to an element, each addition rounds by at most
        # 2^-24 of the running value (<= max|base| + 2 max|ref|)
        roundings = 2 * CI.wgrad_rows_workers(Cin, Cout) * 2.0 ** -24 * (float(base.abs().max()) + 2 * top)
        _close(acc, base.double().cpu().numpy() + 2 * ref["gw"], scale=2.0, extra=roundings)


def _tower(dev, ch=64):
    from jdet_amd.models.utils.modules import ConvModule
    torch.manual_seed(7)
    tower = torch.nn.ModuleList([ConvModule(ch, ch, 3, padding=1) for _ in range(2)]).to(dev)
    for m in tower:
        torch.nn.init.normal_(m.conv.bias, std=0.1)
        m.conv.weight.data = m.conv.weight.data.contiguous(memory_format=torch.channels_last)
    return tower


def _run_tower(tower, x, g, sparse):
    for m in tower:
        m.row_sparse_grad = sparse
        m.zero_grad()
    xi = x.clone().requires_grad_(True)
    y = xi
    for m in tower:
        y = m(y)
    y.backward(g)
    return [xi.grad] + [p.grad.clone() for m in tower for p in (m.conv.weight, m.conv.bias)]


def _sparse_grad(shape, nrows, dev, seed):
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    g = torch.zeros(N * H * W, C)
    if nrows:
        g[torch.randperm(N * H * W, generator=gen)[:nrows]] = torch.randn(nrows, C, generator=gen)
    return g.view(N, H, W, C).permute(0, 3, 1, 2).to(dev)


def test_conv_module_rows_route_matches_dense_route(dev, monkeypatch):
    """a two-layer ConvModule tower with row_sparse_grad set and not set: input, weight and bias gradients agree at
    2e-4 max + 1e-6 (tests/test_gpu_conv_igemm.py: test_conv_module_fused_path_matches_library_path); the flag routes
    both layers through the rows path and JDET_CONV_ROWS=0 (the module switch) routes none"""
    from jdet_amd.ops import conv_igemm as CI
    tower = _tower(dev)
    x = torch.randn(2, 64, 13, 17, device=dev).contiguous(memory_format=torch.channels_last)
    g = _sparse_grad((2, 64, 13, 17), 13, dev, 3)
    calls = []
    real = CI._rows_backward
    monkeypatch.setattr(CI, "_rows_backward", lambda *a: (calls.append(1), real(*a))[1])
    sparse = _run_tower(tower, x, g, True)
    assert len(calls) == 2
    dense = _run_tower(tower, x, g, False)
    assert len(calls) == 2
    monkeypatch.setattr(CI, "ROWS", False)
    off = _run_tower(tower, x, g, True)
    assert len(calls) == 2
    for a, b, c in zip(sparse, dense, off):
        assert (a - b).abs().max().item() <= 2e-4 * b.abs().max().item() + 1e-6
        assert (c - b).abs().max().item() <= 2e-4 * b.abs().max().item() + 1e-6
    assert dense[0].abs().max().item() > 0
    # weights updated behind the version counters (as the fused multi-tensor SGD step does): the flipped weights of the
    # rows data gradient follow
    monkeypatch.setattr(CI, "ROWS", True)
    for m in tower:
        v = m.conv.weight._version
        m.conv.weight.data.mul_(-1.5)
        assert m.conv.weight._version == v
    sparse, dense = _run_tower(tower, x, g, True), _run_tower(tower, x, g, False)
    assert len(calls) == 4
    for a, b in zip(sparse, dense):
        assert (a - b).abs().max().item() <= 2e-4 * b.abs().max().item() + 1e-6


def test_captured_backward_reads_the_count_at_replay(dev):
    """one forward + backward of the tower captured in a HIP graph, replayed with gradients of 3, 40 and 0 non-zero rows
    copied into the static input: every replay equals the eager dense route -- no list length, grid or loop bound was
    fixed at capture time"""
    from jdet_amd import _lib as L
    tower = _tower(dev)
    shape = (2, 64, 13, 17)
    x = torch.randn(*shape, device=dev).contiguous(memory_format=torch.channels_last)
    grads = [_sparse_grad(shape, n, dev, 10 + n) for n in (3, 40, 0)]
    want = [_run_tower(tower, x, g, False) for g in grads]
    for m in tower:
        m.row_sparse_grad = True
        m.zero_grad(set_to_none=True)
    params = [p for m in tower for p in (m.conv.weight, m.conv.bias)]
    gs = _sparse_grad(shape, 25, dev, 99).clone()
    xi = x.clone().requires_grad_(True)

    def step():
        y = xi
        for m in tower:
            y = m(y)
        return torch.autograd.grad(y, [xi] + params, gs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = L.new_graph()
    with torch.cuda.graph(graph):
        out = step()
    L.harden_graph(graph)
    for g, ref in zip(grads, want):
        gs.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, ref):
            assert (a - b).abs().max().item() <= 2e-4 * b.abs().max().item() + 1e-6
    assert not any(o.any() for o in out[:1] + out[1::2])       # the last replay had no rows: zero input / weight gradients


def test_dgrad_without_zero_fill_writes_the_listed_rows_only(dev):
    """zero_first = 0: rows of gx outside the list keep what they held, bit for bit"""
    from jdet_amd import _lib as L
    from tests.abi_cases import ROWS_SHAPES, rows_inputs
    N, H, W, Cin, Cout = ROWS_SHAPES[0]
    x0, w0, g0, rows0, drows0 = rows_inputs(ROWS_SHAPES[0], 0.03)
    g = torch.from_numpy(g0).to(dev)
    wd = torch.from_numpy(np.ascontiguousarray(w0[:, :, ::-1, ::-1].transpose(1, 2, 3, 0))).to(dev)
    rows, count = torch.from_numpy(drows0).to(dev), torch.tensor([len(drows0)], dtype=torch.int32, device=dev)
    gx = torch.full((N * H * W, Cin), 3.25, device=dev)
    L.check(L.lib().jdet_conv3x3_dgrad_rows(g.data_ptr(), wd.data_ptr(), rows.data_ptr(), count.data_ptr(), N, H, W, Cin,
                                            Cout, 0, gx.data_ptr(), L.stream_ptr(g)), "jdet_conv3x3_dgrad_rows")
    keep = torch.ones(N * H * W, dtype=torch.bool, device=dev)
    keep[rows.long()] = False
    assert bool((gx[keep] == 3.25).all()) and not bool((gx[~keep] == 3.25).all(1).any())
