"""GPU: S2ANetHead's training forward with the ODM regression tower computed on the rows its loss reads
(`_forward_train_rows`: csrc/conv_rows.hip's gathered forward) against the dense route: the three losses the route does
not touch are bit-equal, loss_odm_bbox and every gradient agree at the bound of the tower test, the step has no host
synchronisation, and each switch routes as documented."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(40, 40), (20, 20), (10, 10), (5, 5), (3, 3)]          # 1600 positions: stays per level; 4 packed
STRIDES = [8, 16, 32, 64, 128]
IMG = 320


def _gts():
    """per image: boxes the size of the stride-8 anchors (32) for the per-level path, of the stride-16 / -32 anchors
    (64, 128) for the packed path"""
    a = np.asarray([[60.0, 70.0, 34.0, 30.0, 0.1], [200.0, 90.0, 30.0, 36.0, -0.2], [120.0, 220.0, 70.0, 60.0, 0.3],
                    [230.0, 230.0, 120.0, 130.0, 0.0]], np.float32)
    b = np.asarray([[100.0, 100.0, 32.0, 32.0, 0.0], [250.0, 60.0, 60.0, 66.0, 0.4], [150.0, 200.0, 140.0, 120.0, -0.1]],
                   np.float32)
    return [a, b]


def _targets(dev):
    out = []
    for k, g in enumerate(_gts()):
        out.append(dict(rboxes=torch.from_numpy(g).to(dev),
                        labels=torch.from_numpy((1 + np.arange(len(g)) + k).astype(np.int32)).to(dev),
                        rboxes_ignore=torch.zeros((0, 5), device=dev), img_size=(IMG, IMG), scale_factor=1.0,
                        pad_shape=(IMG, IMG)))
    return out


def test_the_gts_give_positives_on_both_paths():
    """the restatement of anchor_target_single on the initial anchors (CPU): positives on the per-level level AND on the
    packed levels, in every image"""
    from oracle import box_oracle as B
    anchors = [B.grid_anchors_s2anet(s, [4], [1.0], hw, s) for hw, s in zip(SIZES, STRIDES)]
    first = len(anchors[0])
    for g in _gts():
        pos = B.anchor_target_single(np.concatenate(anchors), g, np.arange(1, len(g) + 1, dtype=np.int32))[4]
        assert (pos < first).sum() > 0 and (pos >= first).sum() > 0


def _agree(got, want):
    for a, b in zip(got, want):
        assert a.shape == b.shape
        assert (a - b).abs().max().item() <= 2e-4 * b.abs().max().item() + 1e-6


def test_rows_forward_route_matches_dense_route(dev, monkeypatch):
    import jdet_amd.models  # noqa: F401
    from jdet_amd.models.roi_heads import s2anet_head as SH
    from jdet_amd.ops import conv_igemm as CI
    from jdet_amd.utils.general import parse_losses
    test_the_gts_give_positives_on_both_paths()
    torch.manual_seed(0)
    head = SH.S2ANetHead(num_classes=16, in_channels=32, feat_channels=32, stacked_convs=2, with_orconv=True,
                         anchor_strides=STRIDES).to(dev)
    head.train()
    head.pack_max_positions = 1024
    feats = [torch.randn(2, 32, h, w, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
             for h, w in SIZES]
    targets = _targets(dev)
    towers, backs = [], []
    real_tower, real_back = CI.rows_tower, CI._rows_backward
    monkeypatch.setattr(CI, "rows_tower", lambda *a: (towers.append(a[3] if len(a) > 3 else None), real_tower(*a))[1])
    monkeypatch.setattr(CI, "_rows_backward", lambda *a: (backs.append(1), real_back(*a))[1])

    def run():
        for f in feats:
            f.grad = None
        head.zero_grad()
        del towers[:], backs[:]
        losses = head(feats, targets)
        total, parsed = parse_losses(losses)
        total.backward()
        grads = [f.grad.clone() for f in feats] + [p.grad.clone() for p in head.parameters() if p.grad is not None]
        return {k: v.detach().clone() for k, v in parsed.items()}, grads, (len(towers), len(backs))

    monkeypatch.setattr(CI, "ROWS", True)
    monkeypatch.setattr(CI, "ROWS_FWD", True)
    on, on_grads, on_calls = run()
    # one tower call for the per-level level, one with the pack's row mask for the packed levels; the backward of the
    # four regression-tower layers on both paths stays the rows backward
    assert on_calls == (2, 8) and sum(m is not None for m in towers) == 1
    monkeypatch.setattr(CI, "ROWS_FWD", False)
    off, off_grads, off_calls = run()
    assert off_calls == (0, 8)
    for k in ("loss_fam_cls", "loss_fam_bbox", "loss_odm_cls"):
        assert torch.equal(on[k], off[k]), k
    assert off["loss_odm_bbox"].item() > 0
    _agree([on["loss_odm_bbox"]], [off["loss_odm_bbox"]])
    assert len(on_grads) == len(off_grads) == len(feats) + sum(p.requires_grad for p in head.parameters())
    _agree(on_grads, off_grads)
    # JDET_CONV_ROWS=0 switches the forward route off together with the rows backward
    monkeypatch.setattr(CI, "ROWS", False)
    monkeypatch.setattr(CI, "ROWS_FWD", True)
    none, none_grads, none_calls = run()
    assert none_calls == (0, 0)
    _agree(none_grads, off_grads)
    # ---- the route-on step has no host synchronisation (caches are warm) ----
    monkeypatch.setattr(CI, "ROWS", True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for f in feats:
            f.grad = None
        head.zero_grad()
        del towers[:]
        total, _ = parse_losses(head(feats, targets))
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert len(towers) == 2 and torch.isfinite(total)
    # eval mode is untouched: no tower call
    head.eval()
    del towers[:]
    with torch.no_grad():
        head(feats, targets)
    assert not towers
