"""GPU: the row-sparse forward of a regression tower's 3x3 convolutions (csrc/conv_rows.hip):
the three device-side row lists from a flag byte per position against numpy, the gathered forward against float64
conv2d + bias [+ relu] on the CPU at the bound of the igemm test (|err| <= 2e-5 max|ref| + 1e-6), untouched / zero rows
outside the list, the row mask, count 0, a dense list, the two-layer tower + prediction layer against the dense route,
and a captured forward + backward replayed with other flags."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(2, 13, 17, 64, 64),        # odd sizes and an image boundary; 442 rows = six full M tiles and a partial seventh
          (1, 8, 8, 256, 256),        # single image, full channel count
          (2, 20, 24, 32, 256)]       # narrow Cin
PATTERNS = ["zero", "borders", "random3", "dense"]
REL, ABS = 2e-5, 1e-6                 # tests/test_gpu_conv_igemm.py:45
IDS = lambda s: "x".join(map(str, s))  # noqa: E731


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
        rows = rng.choice(P, max(1, int(round(0.03 * P))), replace=False)
        if N > 1:                  # a dilation across the image boundary would show
            rows = np.concatenate([rows, [H * W - 1, H * W]])
        return np.unique(rows)
    if pattern == "dense":
        return np.arange(P)
    raise KeyError(pattern)


def _dilate(nz):
    """3x3 dilation of (N, H, W) booleans inside each image"""
    N, H, W = nz.shape
    pad = np.pad(nz, ((0, 0), (1, 1), (1, 1)))
    out = np.zeros_like(nz)
    for dy in range(3):
        for dx in range(3):
            out |= pad[:, dy:dy + H, dx:dx + W]
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_lists_from_flags(dev, shape, pattern):
    """the three lists and counts equal numpy's flatnonzero of the flags, of their dilation and of the second dilation;
    -1 behind every count; any non-zero byte is a flag"""
    from jdet_amd.ops import conv_igemm as CI
    N, H, W = shape[:3]
    P = N * H * W
    rng = np.random.default_rng(100 * SHAPES.index(shape) + PATTERNS.index(pattern))
    rows0 = _rows_of(pattern, N, H, W, rng)
    f = np.zeros(P, np.uint8)
    f[rows0] = rng.integers(1, 256, len(rows0))
    nz = f.reshape(N, H, W) != 0
    want = [np.flatnonzero(nz), np.flatnonzero(_dilate(nz)), np.flatnonzero(_dilate(_dilate(nz)))]
    if N > 1 and pattern in ("borders", "random3"):
        assert H * W - 1 in want[0] and H * W in want[0]
    r0, r1, r2, counts = CI.rows_from_flags(torch.from_numpy(f).to(dev), N, H, W)
    got_counts = [int(v) for v in counts.cpu()]
    assert got_counts == [len(w) for w in want]
    for got, ref, c in zip((r0, r1, r2), want, got_counts):
        got = got.cpu().numpy()
        assert got.shape == (P,) and np.array_equal(got[:c], ref) and (got[c:] == -1).all()
    # a bool tensor is the same bytes
    b0, b1, b2, bc = CI.rows_from_flags(torch.from_numpy(nz.reshape(-1)).to(dev), N, H, W)
    assert torch.equal(bc, counts) and torch.equal(b0, r0) and torch.equal(b1, r1) and torch.equal(b2, r2)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs and the float64 CPU reference of one shape, computed once and shared: x, w, bias, the pre-activation"""
    N, H, W, Cin, Cout = shape
    rng = np.random.default_rng(7000 + SHAPES.index(shape))
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * (2.0 / (9 * Cin)) ** 0.5).astype(np.float32)
    b = (0.3 * rng.standard_normal(Cout)).astype(np.float32)
    y = F.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), torch.from_numpy(w).double(),
                 torch.from_numpy(b).double(), 1, 1).permute(0, 2, 3, 1).contiguous().numpy()
    rows = _rows_of("random3", N, H, W, rng)
    rows = np.unique(np.concatenate([rows, _rows_of("borders", N, H, W, rng)]))
    return x, w, b, y.reshape(N * H * W, Cout), rows


def _close(val, ref):
    val = val.detach().cpu().double().numpy()
    top = float(np.abs(ref).max()) if ref.size else 0.0
    err = float(np.abs(val - ref).max()) if ref.size else 0.0
    bound = REL * top + ABS
    print("max err %.3e bound %.3e (max|ref| %.3e)" % (err, bound, top))
    assert err <= bound, (err, bound)


def _forward(dev, shape, rows, relu, out=None, rowmask=None, count=None):
    from jdet_amd.ops import conv_igemm as CI
    N, H, W, Cin, Cout = shape
    P = N * H * W
    x0, w0, b0, _, _ = _case(shape)
    x, b = torch.from_numpy(x0).to(dev), torch.from_numpy(b0).to(dev)
    w = torch.from_numpy(w0).to(dev).permute(0, 2, 3, 1).contiguous()
    lst = torch.full((P,), -1, dtype=torch.int32, device=dev)
    lst[:len(rows)] = torch.from_numpy(np.asarray(rows, np.int32)).to(dev)
    cnt = torch.tensor([len(rows) if count is None else count], dtype=torch.int32, device=dev)
    y = CI.conv3x3_rows_forward_nhwc(x, w, b, relu, rowmask, lst, cnt.data_ptr(), out)
    torch.cuda.synchronize()
    return y.reshape(P, Cout)


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gathered_forward(dev, shape, relu):
    N, H, W, Cin, Cout = shape
    P = N * H * W
    _, _, _, pre, rows = _case(shape)
    ref = np.maximum(pre, 0.0) if relu else pre
    listed = np.zeros(P, bool)
    listed[rows] = True
    # ---- zero fill: the listed rows within the bound, every other row exactly 0 ----
    y = _forward(dev, shape, rows, relu)
    _close(y[torch.from_numpy(listed).to(dev)], ref[listed])
    assert not y.cpu().numpy()[~listed].any()
    # ---- a poisoned output and no zero fill: every unlisted row unchanged bit for bit, the listed rows as before ----
    poison = torch.full((N, H, W, Cout), float("nan"), device=dev)
    poison.view(torch.int32).fill_(0x7FC5A5A5)
    got = _forward(dev, shape, rows, relu, out=poison)
    bits = got.view(torch.int32).cpu().numpy()
    assert (bits[~listed] == 0x7FC5A5A5).all()
    assert torch.equal(got[torch.from_numpy(listed).to(dev)], y[torch.from_numpy(listed).to(dev)])
    # ---- rows with rowmask 0 exactly 0 (as a dilated row in a gap of a LevelPack), the others unchanged ----
    mask = np.ones(P, np.float32)
    mask[rows[::3]] = 0.0
    ym = _forward(dev, shape, rows, relu, rowmask=torch.from_numpy(mask).to(dev))
    keep = torch.from_numpy(listed & (mask != 0)).to(dev)
    assert not ym.cpu().numpy()[mask == 0].any()
    assert torch.equal(ym[keep], y[keep])
    # ---- count 0 writes nothing ----
    poison.view(torch.int32).fill_(0x7FC5A5A5)
    none = _forward(dev, shape, rows, relu, out=poison, count=0)
    assert (none.view(torch.int32).cpu().numpy() == 0x7FC5A5A5).all()
    assert not _forward(dev, shape, rows, relu, count=0).any()          # ... and its zero fill is the whole result


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dense_list_reproduces_the_whole_map(dev, shape):
    N, H, W, Cin, Cout = shape
    _, _, _, pre, _ = _case(shape)
    _close(_forward(dev, shape, np.arange(N * H * W), True), np.maximum(pre, 0.0))
    _close(_forward(dev, shape, np.arange(N * H * W), False), pre)


# ---- the tower: two ConvModules + a 3x3 five-channel prediction layer --------------------------------------------------
TSHAPE = (2, 64, 13, 17)


def _tower(dev, ch=64):
    from jdet_amd.models.utils.modules import ConvModule
    torch.manual_seed(7)
    tower = torch.nn.ModuleList([ConvModule(ch, ch, 3, padding=1) for _ in range(2)]).to(dev)
    for m in tower:
        torch.nn.init.normal_(m.conv.bias, std=0.1)
        m.conv.weight.data = m.conv.weight.data.contiguous(memory_format=torch.channels_last)
        m.row_sparse_grad = True
    pred = torch.nn.Conv2d(ch, 5, 3, padding=1).to(dev)
    return tower, pred


def _params(tower, pred):
    return [p for m in tower for p in (m.conv.weight, m.conv.bias)] + [pred.weight, pred.bias]


def _flags_and_grad(nrows, dev, seed):
    """flags of `nrows` positions and a prediction gradient that is non-zero on exactly those rows"""
    N, _, H, W = TSHAPE
    gen = torch.Generator().manual_seed(seed)
    flags = torch.zeros(N * H * W, dtype=torch.bool)
    g = torch.zeros(N * H * W, 5)
    if nrows:
        idx = torch.randperm(N * H * W, generator=gen)[:nrows]
        flags[idx] = True
        g[idx] = torch.randn(nrows, 5, generator=gen)
    return flags.to(dev), g.view(N, H, W, 5).permute(0, 3, 1, 2).contiguous().to(dev)


def _forward_tower(tower, pred, xi, flags, rows_route):
    from jdet_amd.ops import conv_igemm as CI
    if rows_route:
        y = CI.rows_tower([m.conv for m in tower], xi, flags)
    else:
        y = xi
        for m in tower:
            y = m(y)
    return CI.conv_module(pred, y)


def _run_tower(tower, pred, x, flags, g, rows_route):
    xi = x.clone().requires_grad_(True)
    out = _forward_tower(tower, pred, xi, flags, rows_route)
    grads = torch.autograd.grad(out, [xi] + _params(tower, pred), g)
    at_flags = out.detach().permute(0, 2, 3, 1).reshape(-1, 5) * flags[:, None]
    return [at_flags] + [t.clone() for t in grads]


def _agree(got, want):
    for a, b in zip(got, want):
        assert a.shape == b.shape
        assert (a - b).abs().max().item() <= 2e-4 * b.abs().max().item() + 1e-6


def test_tower_rows_route_matches_dense_route(dev, monkeypatch):
    """the prediction at the flagged rows, the input gradient and every weight / bias gradient agree with the dense
    route at 2e-4 max + 1e-6 (test_conv_module_rows_route_matches_dense_route), also after the weights moved behind their
    version counters; both layers take the gathered forward, on the twice / once dilated list"""
    from jdet_amd.ops import conv_igemm as CI
    tower, pred = _tower(dev)
    x = torch.randn(*TSHAPE, device=dev).contiguous(memory_format=torch.channels_last)
    flags, g = _flags_and_grad(13, dev, 3)
    assert CI.rows_tower_applicable([m.conv for m in tower], x)
    calls = []
    real = CI.conv3x3_rows_forward_nhwc
    monkeypatch.setattr(CI, "conv3x3_rows_forward_nhwc", lambda *a: (calls.append(a[5]), real(*a))[1])
    rows = _run_tower(tower, pred, x, flags, g, True)
    assert len(calls) == 2
    nz = flags.view(TSHAPE[0], TSHAPE[2], TSHAPE[3]).cpu().numpy()
    d1 = np.flatnonzero(_dilate(nz))
    d2 = np.flatnonzero(_dilate(_dilate(nz)))
    assert np.array_equal(calls[0].cpu().numpy()[:len(d2)], d2) and np.array_equal(calls[1].cpu().numpy()[:len(d1)], d1)
    dense = _run_tower(tower, pred, x, flags, g, False)
    assert len(calls) == 2
    _agree(rows, dense)
    assert all(t.abs().max().item() > 0 for t in dense)
    for m in tower:
        v = m.conv.weight._version
        m.conv.weight.data.mul_(-1.5)
        assert m.conv.weight._version == v
    _agree(_run_tower(tower, pred, x, flags, g, True), _run_tower(tower, pred, x, flags, g, False))
    assert len(calls) == 4


def test_captured_tower_reads_flags_and_counts_at_replay(dev):
    """one forward + backward of the tower captured in a HIP graph, replayed with flags of 3, 40 and 0 rows (and their
    gradients) copied into the static inputs: every replay equals the eager dense route -- no list length, grid or loop
    bound was fixed at capture time; the last replay has zero tower gradients"""
    from jdet_amd import _lib as L
    tower, pred = _tower(dev)
    x = torch.randn(*TSHAPE, device=dev).contiguous(memory_format=torch.channels_last)
    cases = [_flags_and_grad(n, dev, 10 + n) for n in (3, 40, 0)]
    want = [_run_tower(tower, pred, x, f, g, False) for f, g in cases]
    fs, gs = (t.clone() for t in _flags_and_grad(25, dev, 99))
    xi = x.clone().requires_grad_(True)

    def step():
        out = _forward_tower(tower, pred, xi, fs, True)
        return (out,) + torch.autograd.grad(out, [xi] + _params(tower, pred), gs)

    step()                        # warm-up: library workspaces, the scratch caches
    torch.cuda.synchronize()
    graph = L.new_graph()
    with torch.cuda.graph(graph):
        out = step()
    L.harden_graph(graph)
    for (f, g), ref in zip(cases, want):
        fs.copy_(f)
        gs.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        got = [out[0].detach().permute(0, 2, 3, 1).reshape(-1, 5) * f[:, None]] + list(out[1:])
        _agree(got, ref)
    assert not any(o.any() for o in out[1:6])       # no rows: zero input gradient and zero tower weight / bias gradients
