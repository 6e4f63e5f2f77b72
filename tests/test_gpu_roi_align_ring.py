"""GPU parity: the rolling-window tap loop of the RoIAlign forward (round 6) against the per-bin loop it replaced."""
import numpy as np
import pytest
import torch

from tests import inputs as I

pytestmark = pytest.mark.gpu

PER_BIN = 6   # forward mode of jdet_roi_align_forward_cl_mode (csrc/experimental/roi_align_modes.hip)


def cases():
    out = []
    # (variant, n_orient, C, N, H, W, hw, R)
    shapes = [(0, 1, 256, 1, 256, 256, (7, 7), 2000), (0, 1, 64, 3, 40, 56, (7, 7), 203), (1, 1, 128, 2, 40, 56, (4, 4), 150),
              (0, 1, 192, 2, 33, 47, (5, 8), 180), (3, 1, 64, 3, 40, 56, (8, 3), 120), (4, 1, 256, 2, 64, 64, (7, 7), 300),
              (2, 8, 256, 2, 64, 64, (7, 7), 300), (2, 4, 128, 2, 40, 56, (7, 7), 200), (0, 1, 256, 1, 16, 16, (7, 7), 64),
              (0, 1, 256, 1, 256, 256, (7, 7), 3), (0, 1, 256, 1, 256, 256, (2, 2), 50), (0, 1, 256, 1, 256, 256, (1, 1), 50)]
    for k, (variant, no, C, N, H, W, hw, R) in enumerate(shapes):
        rng = np.random.default_rng(900 + k)
        feat = rng.standard_normal((N, C, H, W)).astype(np.float32)
        scale = 0.25
        rois = np.concatenate([I.rois_from_obbs(I.random_obbs(rng, R, extent=W / scale, wh=(2.0, 300.0)),
                                                rng.integers(0, N, R)), I.edge_rois(H, W, scale)], 0)
        rois[:, 0] = np.minimum(rois[:, 0], N - 1)              # (edge_rois name image 1)
        rois[rng.random(rois.shape[0]) < 0.15, 0] = -1.0        # masked RoIs (another pyramid level's)
        if variant in (3, 4):
            rois = I.obb_to_hbb_rois(rois)
        out.append((variant, no, feat, rois.astype(np.float32), hw, scale))
    return out


def test_rolling_window_equals_the_per_bin_loop(dev):
    """Round 6: the product tap loop of the channels-last merged forward is a rolling window of 4 groups of 4 rows
    (hand-counted vmcnt, csrc/roi_align_fwd.h); the per-bin loop of rounds 1-5 is forward mode 6 of
    jdet_roi_align_forward_cl_mode in libjdet_experimental.so.  Both fold the same entries in the same order with the same
    fmaf: every output word must be EQUAL -- 12 shapes x dialects (north-star size, masked RoIs, RoIs across and beyond the
    border: empty bins, every channel count class, 1x1 .. 8x3 grids, RiRoIAlign with 4 / 8 orientations).  The per-bin
    launch gets the schedule the product computes for itself (jdet_roi_spatial_order for R >= 64, none below), so the two
    launches differ in the loop only; outputs start at 7.0, so the untouched rows of masked RoIs are compared too."""
    from jdet_amd import _experimental as X
    from jdet_amd import _lib as L
    from jdet_amd.ops._roi_common import spatial_order
    lib, xlib = L.lib(), X.lib()   # (a missing libjdet_experimental.so raises: the test fails, it does not skip)
    report, ok = [], True
    for k, (variant, no, feat, rois, hw, scale) in enumerate(cases()):
        x = torch.from_numpy(feat).to(dev).contiguous(memory_format=torch.channels_last)
        r = torch.from_numpy(rois).to(dev)
        N, C, H, W = x.shape
        R = r.shape[0]
        a = torch.full((R, C) + tuple(hw), 7.0, device=dev).contiguous(memory_format=torch.channels_last)
        b = torch.full((R, C) + tuple(hw), 7.0, device=dev).contiguous(memory_format=torch.channels_last)
        wsb = lib.jdet_roi_align_forward_cl_workspace(R, hw[0], hw[1])
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        L.check(lib.jdet_roi_align_forward_cl(variant, x.data_ptr(), N, C, H, W, r.data_ptr(), R, hw[0], hw[1], scale, 2, no,
                                              a.data_ptr(), ws.data_ptr(), wsb, L.stream_ptr(x)), "fwd_cl")
        order = spatial_order(r, scale, N, H, W) if R >= 64 else None
        L.check(xlib.jdet_roi_align_forward_cl_mode(PER_BIN, variant, x.data_ptr(), N, C, H, W, r.data_ptr(), R, hw[0], hw[1],
                                                    scale, 2, no, order.data_ptr() if order is not None else None,
                                                    b.data_ptr(), None, 0, L.stream_ptr(x)), "fwd_cl_mode 6")
        torch.cuda.synchronize()
        same = torch.equal(a.view(torch.int32), b.view(torch.int32))
        report.append("case %2d  shape %-22s bit-equal %s  max|diff| %.3e  nan %s" %
                      (k, tuple(a.shape), same, float((a - b).abs().max()), bool(torch.isnan(a).any())))
        ok = ok and same
    print("\n".join(report))
    assert ok, "\n".join(report)
