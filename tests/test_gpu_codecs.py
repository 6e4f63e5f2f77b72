"""GPU: the seven elementwise rotated-box codec kernels (csrc/box_codec_assign.hip, csrc/box_codec_oriented.hip) through
the Python wrappers the heads call, against the float64 restatements and fixtures of tests/codec_ref.py
(tests/test_codec_cpu.py holds the fixtures to their contract and shows that the bounds below tell a wrong codec from
the right one).

Retained boxes against float64.  Error measures: encodes |err| / max(1, |ref|) per column; decodes the position / size
columns relative to the box's largest |x|, |y|, w, h and the angle in radians, compared directly (not modulo pi).
Bound = 4 x e32, e32 = the worst error of the float32 restatement against the float64 one in the same measure over the
same boxes -- computed here from the two restatements, never from the kernel (factor 4 as in tests/test_gpu_fcos.py:
a different legal operation order plus a device libm within 2 ulp).  Integer-like outputs are compared exactly: which
of (w, h) came out first, which dtheta the oriented encode took, the angle of obb2hbb2obb.

Edge rows (ties, values exactly on a clamp or a wrap point, n = 0 and n = 1) are compared with the float32 torch
composition on the device: in float64 these fp32 ties are no ties.  The kernels are built with -ffp-contract=off and
perform the composition's IEEE operations in its order: identical branch, values within 2 ulp.

Grid-stride loops: each of the six looped kernels runs on its 4096-row fixture tiled to just past the capacity of its
capped grid (65 536 x 256 elements for the oriented kernels, 262 144 x 256 for the assign kernels); every tile of the
output must equal the first, and the first the small launch, bit for bit.

Measured on an MI355X (this module's own printout; e32 is a property of the fixtures, the last column is the kernel):

  fixture       group  retained  e32        bound      kernel          fixture       group  e32        bound      kernel
  b2d           col0   1.0000    4.303e-07  1.721e-06  4.303e-07       d2b_hi3       xywh   1.155e-07  4.621e-07  1.101e-07
  b2d           col1             3.411e-07  1.364e-06  3.411e-07       d2b_hi3       angle  9.265e-07  3.706e-06  1.165e-06
  b2d           col2             4.316e-07  1.726e-06  3.136e-07       d2b_lo1       xywh   2.097e-07  8.388e-07  1.265e-07
  b2d           col3             2.818e-07  1.127e-06  2.547e-07       d2b_lo1       angle  7.954e-07  3.182e-06  9.197e-07
  b2d           col4             1.802e-06  7.206e-06  1.802e-06       d2b_lo15      xywh   1.769e-07  7.074e-07  1.324e-07
  ori_enc       col0   0.9998    4.072e-07  1.629e-06  4.072e-07       d2b_lo15      angle  9.944e-07  3.978e-06  1.199e-06
  ori_enc       col1             3.651e-07  1.460e-06  3.651e-07       ori_dec_hi3   xywh   1.197e-07  4.787e-07  1.153e-07
  ori_enc       col2             3.515e-07  1.406e-06  3.496e-07       ori_dec_hi3   angle  7.272e-07  2.909e-06  7.272e-07
  ori_enc       col3             3.159e-07  1.263e-06  2.539e-07       ori_dec_lo1   xywh   1.322e-07  5.286e-07  8.059e-08
  ori_enc       col4             5.421e-06  2.168e-05  5.421e-06       ori_dec_lo1   angle  7.272e-07  2.909e-06  7.272e-07
  mid_enc       col0   0.9976    4.594e-05  1.838e-04  4.594e-05       ori_dec_lo15  xywh   1.837e-07  7.350e-07  1.357e-07
  mid_enc       col1             2.731e-05  1.092e-04  2.731e-05       ori_dec_lo15  angle  7.272e-07  2.909e-06  7.272e-07
  mid_enc       col2             3.103e-05  1.241e-04  3.103e-05       mid_dec_hi    xywh   8.789e-06  3.516e-05  8.789e-06
  mid_enc       col3             2.335e-05  9.341e-05  2.335e-05       mid_dec_hi    angle  8.770e-06  3.508e-05  8.770e-06
  mid_enc       col4             1.252e-05  5.007e-05  1.252e-05       mid_dec_lo    xywh   3.365e-06  1.346e-05  2.722e-06
  mid_enc       col5             1.295e-05  5.181e-05  1.295e-05       mid_dec_lo    angle  7.065e-06  2.826e-05  7.065e-06
  hbb           xywh   0.9998    1.785e-07  7.140e-07  1.901e-07       hbb           angle  4.371e-08  1.748e-07  4.371e-08

(retained: d2b_hi3 1.0000, d2b_lo1 0.9998, d2b_lo15 1.0000, ori_dec_hi3 0.9997, ori_dec_lo1 1.0000, ori_dec_lo15 0.9998,
mid_dec_hi 1.0000, mid_dec_lo 0.9998.)  Where the kernel's figure equals e32 the worst box is the same box with the same
rounding: the kernels perform the restatement's float32 operations; every encode column is at most e32.  The midpoint encode's columns are large because
(gx - px) / pw / std cancels two coordinates of several hundred px; that is the codec, in either precision.
Edge rows: every case bit-equal to the composition except the midpoint decode (1 ulp, in the columns behind atan2f /
sincosf).  Grid-stride: b2d 67 112 961 rows (3.75 GB), d2b 4 474 198 x 15 (2.58 GB), the four oriented kernels
16 781 313 rows (0.94 GB): every tile equal to the first; none skipped.
"""
import math

import numpy as np
import pytest
import torch

from tests import codec_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
HALF_PI32 = F32(math.pi / 2)


def _dev(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(device=dev, dtype=dtype)       # a copy: the fixtures are read-only


def _wrapper(codec, kw):
    """the call the heads make: fn(*device tensors) -> device tensor"""
    from jdet_amd.models.boxes import coder
    from jdet_amd.models.boxes.iou_calculator import fake_rotated_boxes
    if codec == "b2d":
        return lambda p, g: coder.DeltaXYWHABBoxCoder(kw["means"], kw["stds"]).encode(p, g)
    if codec == "d2b":
        return lambda r, d: coder.DeltaXYWHABBoxCoder(kw["means"], kw["stds"]).decode(r, d, wh_ratio_clip=kw["wh_ratio_clip"])
    if codec == "hbb":
        return fake_rotated_boxes
    c = (coder.MidpointOffsetCoder if codec.startswith("mid") else coder.OrientedDeltaXYWHTCoder)(kw["means"], kw["stds"])
    if codec.endswith("enc"):
        return c.encode
    return lambda a, d: c.decode(a, d, wh_ratio_clip=kw["wh_ratio_clip"])


def _composition(codec, kw, tensors):
    """the torch general route in the tensors' dtype on their device: asking for a gradient keeps the fused launch out"""
    if codec == "hbb":
        from jdet_amd.ops.bbox_transforms import hbb2obb, obb2hbb
        return hbb2obb(obb2hbb(tensors[0][:, :5]))
    last = tensors[-1].clone().requires_grad_(True)
    with torch.enable_grad():
        out = _wrapper(codec, kw)(*tensors[:-1], last)
    assert out.requires_grad or out.numel() == 0
    return out.detach()


def _direct(codec, kw, tensors):
    """the entry point itself, on float32 device tensors"""
    from jdet_amd import _lib as L
    a = tensors[0]
    n = a.shape[0]
    st = L.stream_ptr(a)
    if codec == "hbb":
        out = torch.empty((n, 5), dtype=torch.float32, device=a.device)
        rc = L.lib().jdet_obb2hbb2obb(L.ptr(a), n, a.shape[1], L.ptr(out), st)
        L.check(rc, codec)
        return out
    b = tensors[1]
    k = 6 if codec.startswith("mid") else 5
    m, s = L.vecn(kw["means"], k), L.vecn(kw["stds"], k)
    if codec == "b2d":
        out = torch.empty_like(a)
        rc = L.lib().jdet_bbox2delta_rotated(L.ptr(a), L.ptr(b), n, m, s, L.ptr(out), st)
    elif codec == "d2b":
        out = torch.empty_like(b)
        rc = L.lib().jdet_delta2bbox_rotated(L.ptr(a), L.ptr(b), n, b.shape[1] // 5, m, s, kw["wh_ratio_clip"], L.ptr(out), st)
    elif codec == "mid_enc":
        out = torch.empty((n, 6), dtype=torch.float32, device=a.device)
        rc = L.lib().jdet_midpoint_offset_encode(L.ptr(a), L.ptr(b), n, m, s, L.ptr(out), st)
    elif codec == "mid_dec":
        out = torch.empty((n, 5), dtype=torch.float32, device=a.device)
        rc = L.lib().jdet_midpoint_offset_decode(L.ptr(a), L.ptr(b), n, m, s, kw["wh_ratio_clip"], L.ptr(out), st)
    elif codec == "ori_enc":
        out = torch.empty_like(a)
        rc = L.lib().jdet_oriented_delta_encode(L.ptr(a), L.ptr(b), n, m, s, L.ptr(out), st)
    else:
        out = torch.empty_like(b)
        rc = L.lib().jdet_oriented_delta_decode(L.ptr(a), L.ptr(b), n, b.shape[1] // 5, m, s, kw["wh_ratio_clip"], L.ptr(out), st)
    L.check(rc, codec)
    return out


def _angle_range(codec):
    """the closed fp32 image of the decoder's angle interval: r = x - floor(x / pi) * pi lies in [0, pi] in fp32 (a tiny
    negative x gives pi itself), so start + r reaches the upper end; the reference's fp32 program does the same"""
    start = F32(-math.pi / 4) if codec == "d2b" else F32(-math.pi / 2)
    return float(start), float(F32(start + F32(math.pi)))


# ---------------------------------------------------------------------------------------------- retained boxes vs float64
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_retained_boxes_against_float64(dev, name):
    f = R.fixture(name)
    n = R.N_ROWS
    got_t = _wrapper(f.codec, f.kw)(*(_dev(a, dev) for a in f.args))
    assert got_t.dtype == torch.float32 and tuple(got_t.shape) == f.ref.shape
    got = got_t.cpu().numpy()
    assert np.isfinite(got).all()
    err, bound = R.worst(R.errors(f.codec, got, f.ref), f.keep), f.bound()
    for k in sorted(bound):
        print("%-13s %-6s retained %.4f  e32 %.3e  bound %.3e  kernel %.3e"
              % (name, k, float(f.keep.mean()), f.e32[k], bound[k], err[k]))
    for k in bound:
        assert err[k] <= bound[k], (name, k, err[k], bound[k])
    g = got.astype(F64).reshape(n, -1, f.ref.shape[1] // f.keep.shape[1])
    r = f.ref.reshape(g.shape)
    if f.codec in ("ori_dec", "mid_dec"):
        # which of (w, h) came out first: the pre-swap pair is (h, w) of the reference where it swapped
        sw = f.flags["swapped"]
        first, second = np.where(sw, r[..., 3], r[..., 2]), np.where(sw, r[..., 2], r[..., 3])
        got_swapped = np.abs(g[..., 2] - second) < np.abs(g[..., 2] - first)
        assert np.array_equal(got_swapped[f.keep], sw[f.keep])
        assert (got[:, 2::5] >= got[:, 3::5]).all()                              # every box, retained or not
    if f.codec == "ori_enc":
        # which dtheta: the two candidates lie pi/2 apart, the output names one of them
        p, gt = (a.astype(F64) for a in f.args)
        d1 = R._regular_theta(gt[:, 4] - p[:, 4], F64, None)[0]
        d2 = R._regular_theta(gt[:, 4] - p[:, 4] + math.pi / 2, F64, None)[0]
        dth = g[:, 0, 4] * f.kw["stds"][4] + f.kw["means"][4]
        got_second = np.abs(dth - d2) < np.abs(dth - d1)
        assert np.array_equal(got_second[f.keep[:, 0]], f.flags["second"][f.keep])
    if f.codec == "hbb":
        ang = got[:, 4]
        assert np.isin(ang, [F32(0), F32(0) - HALF_PI32]).all()
        assert np.array_equal((ang == 0)[f.keep[:, 0]], f.flags["wide"][f.keep])
        assert (got[:, 2] >= got[:, 3]).all()
    if f.codec in ("d2b", "ori_dec", "mid_dec"):
        lo, hi = _angle_range(f.codec)
        a = got[:, 4::5]
        assert a.min() >= lo and a.max() <= hi, (float(a.min()), float(a.max()), lo, hi)


# ---------------------------------------------------------------------------------------------- edge rows vs the composition
def _ulps(a, b):
    """|a - b| in units of the fp32 spacing at b (0 where equal)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    d = np.abs(a.astype(F64) - b.astype(F64)) / np.spacing(np.maximum(np.abs(b), np.finfo(F32).tiny)).astype(F64)
    return np.where(a == b, 0.0, d)


@pytest.mark.parametrize("name", sorted(R.edge_cases()))
def test_edge_rows_equal_the_float32_composition(dev, name):
    codec, args, kw = R.edge_cases()[name]
    t = [_dev(a, dev) for a in args]
    fused = _wrapper(codec, kw)(*t)
    comp = _composition(codec, kw, t)
    assert fused.dtype == torch.float32 and fused.shape == comp.shape and fused.shape[0] == args[0].shape[0]
    if fused.numel() == 0:
        return
    a, c = fused.cpu().numpy(), comp.cpu().numpy()
    u = _ulps(a, c)
    print("edge %-15s rows %2d  bit-equal %-5s  max distance %.1f ulp" % (name, a.shape[0], bool((a == c).all()), u.max()))
    assert np.isfinite(a).all()
    if codec in R.DECODES:      # branch: the same side first, the same fold of the angle
        assert (np.abs(a[:, 4::5] - c[:, 4::5]) < 1e-3).all(), (a[:, 4::5], c[:, 4::5])
    assert u.max() <= 2, (name, np.argwhere(u > 2)[:4], a[u.max(1) > 2][:4], c[u.max(1) > 2][:4])
    # closed forms
    if name == "mid_enc_axis":
        axis = args[1][:, 4] == 0
        assert (a[axis, 4:] == 0.5).all()
    if name == "hbb_squares":
        assert (a[[0, 1, 4], 4] == 0).all() and (a[[0, 1, 4], 2] == a[[0, 1, 4], 3]).all()
        assert a[6, 4] == F32(0) - HALF_PI32 and a[6, 2] == 40 and a[6, 3] == 20
    if name == "mid_dec_edges":      # da and db both beyond the clamp: the axis-aligned box, 64 x 32 on either anchor
        assert (a[[14, 16], 4] == 0).all() and (np.abs(a[[15, 17], 4]) == HALF_PI32).all()
        assert (np.abs(a[14:18, 2] - 64) < 1e-4).all() and (np.abs(a[14:18, 3] - 32) < 1e-4).all()
    if name == "ori_dec_edges":
        assert (a[:4, 2] == a[:4, 3]).all()                      # the squares: the tie branch, sides equal


# ---------------------------------------------------------------------------------------------- grid-stride loops
# the block caps of the two `grid_for` functions, as their sources state them: (file, the text of the cap, blocks)
CAPS = {"oriented": ("box_codec_oriented.hip", "g > 65536 ? 65536", 65536),
        "assign": ("box_codec_assign.hip", "g > 262144 ? 262144", 262144)}
LOOPED = {           # codec -> (fixture, which cap its launch is under)
    "mid_dec": ("mid_dec_lo", "oriented"), "mid_enc": ("mid_enc", "oriented"),
    "ori_dec": ("ori_dec_lo1", "oriented"), "ori_enc": ("ori_enc", "oriented"),
    "d2b": ("d2b_lo15", "assign"), "b2d": ("b2d", "assign"),
}


def _capacity(which):
    """elements one grid of the capped size covers (256 lanes a block).  The cap is read off the kernel's source: if it
    is raised there, this fails instead of quietly no longer reaching the loop's second iteration"""
    import os
    from jdet_amd import _lib as L
    fname, text, blocks = CAPS[which]
    with open(os.path.join(os.path.dirname(L.LIB_PATH), fname)) as fh:
        src = fh.read()
    assert text in src and "__launch_bounds__(256)" in src, "%s: grid_for no longer caps at %d blocks of 256" % (fname, blocks)
    return blocks * 256


@pytest.mark.parametrize("codec", sorted(LOOPED))
def test_grid_stride_loop_repeats_the_first_tile(dev, codec):
    """n * ncls = capacity + 4097 elements (delta2bbox_rotated with 15 classes: the smallest n that reaches it, since
    that number is no multiple of 15): the loop runs a second time for the first 4097 lanes.  No host reference at this
    size: the tiled input must give the tiled output"""
    name, which = LOOPED[codec]
    capacity = _capacity(which)
    f = R.fixture(name)
    rows = R.N_ROWS
    n = -(-(capacity + 4097) // f.ncls)
    widths = [a.shape[1] for a in f.args] + [f.ref.shape[1]]
    need = 4 * n * sum(widths)
    free = torch.cuda.mem_get_info(dev)[0]
    if free < 2 * need:
        pytest.skip("%s at n = %d needs %.2f GB twice over, the device has %.2f GB free" % (codec, n, need / 2 ** 30, free / 2 ** 30))
    small = [_dev(a, dev) for a in f.args]
    fn = _wrapper(codec, f.kw)
    first = fn(*small)
    reps = -(-n // rows)
    big = [t.repeat(reps, 1)[:n].contiguous() for t in small]
    out = fn(*big)
    del big
    assert out.shape[0] == n and n * f.ncls > capacity
    full = n // rows
    tiles = out[:full * rows].view(full, rows * out.shape[1])
    assert torch.equal(tiles[0], first.view(-1)), "the first tile differs from the 4096-row launch"
    assert torch.equal(tiles, tiles[0].expand_as(tiles)), "a tile differs from the first"
    rest = n - full * rows
    assert torch.equal(out[full * rows:], first[:rest]), "the rows past the last whole tile differ"
    print("grid-stride %-8s n %d x ncls %d = %d elements (capacity %d), %.2f GB, %d tiles equal"
          % (codec, n, f.ncls, n * f.ncls, capacity, need / 2 ** 30, full))


# ---------------------------------------------------------------------------------------------- dtype routing
@pytest.mark.parametrize("name", ["b2d", "d2b_lo15", "hbb", "mid_enc", "mid_dec_lo", "ori_enc", "ori_dec_hi3"])
def test_float64_gets_the_float64_composition_and_float32_the_fused_launch(dev, name):
    """the kernels are fp32: float64 tensors on the device are not cast down; float32 tensors still take the launch --
    their output is bit-equal to a direct call of the entry point (which tells the launch from the composition only
    where the two differ in a bit, the midpoint decode; the launch counts of the heads are pinned by the sync-free tests)"""
    f = R.fixture(name)
    k = 256
    args = [a[:k] for a in f.args]
    fn = _wrapper(f.codec, f.kw)
    out64 = fn(*(_dev(a, dev, torch.float64) for a in args))
    assert out64.dtype == torch.float64
    cols = f.ref.shape[1] // f.keep.shape[1]
    keep = np.repeat(f.keep[:k], cols, axis=1)
    np.testing.assert_allclose(out64.cpu().numpy()[keep], f.ref[:k][keep], rtol=1e-12, atol=1e-12)
    t32 = [_dev(a, dev) for a in args]
    out32 = fn(*t32)
    assert out32.dtype == torch.float32
    assert torch.equal(out32, _direct(f.codec, f.kw, t32))
    # half precision (a head under autocast) is up-cast to the same launch, not sent to the composition
    t16 = [t.to(torch.float16) for t in t32]
    out16 = fn(*t16)
    assert out16.dtype == torch.float32
    want16 = _direct(f.codec, f.kw, [t.float() for t in t16])
    assert torch.equal(out16.view(torch.int32), want16.view(torch.int32))          # bit for bit, whatever the values
