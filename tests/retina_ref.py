"""float64 numpy restatements of the RetinaNet-v1d rules (include/jdet_hip_retina.h, models/roi_heads/retina_head.py) and
the fixtures of tests/retina_cases.py, tests/test_retinanet_cpu.py and tests/test_gpu_retinanet.py.

Restated once here: ground-truth preparation, the fp32 IoU of bbox_iou in its operation order, assignment + bbox2loc_r
targets, the head's loss, the decode / threshold selection in front of the NMS, and the bilinear tf_mode resize with its
transpose.  Everything a tolerance is measured against is float64 evaluated from the fp32 inputs; only the IoU (a
bit-for-bit claim) and the resize coordinates (the rule says fp32) are float32 on purpose."""
import functools

import numpy as np

PI = np.pi
POS, NEG_HI, NEG_LO = 0.5, 0.4, 0.0
FEATMAPS = [(5, 7), (3, 4), (2, 2), (1, 1), (1, 1)]
GT_CHUNK = 256                      # JDET_RETINA_GT_CHUNK
ANCHOR_CFG = dict(type="AnchorGeneratorRotated", strides=[8, 16, 32, 64, 128],
                  ratios=[1, 0.5, 2.0, 0.3333333333333333, 3.0, 5.0, 0.2],
                  scales=[1, 1.2599210498948732, 1.5874010519681994], base_sizes=[32, 64, 128, 256, 512],
                  angles=[-90, -75, -60, -45, -30, -15], mode="H")


def spacing(x):
    """one fp32 spacing at |x| (the bound of a float64 value rounded once to fp32, with room for the last digit of the
    device's exp / log / sin / cos)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------- gt preparation
def gt_prepare(gts):
    """(K, 5) fp32 -> (rboxes (K, 5), rboxes_h (K, 4)) float64"""
    g = np.asarray(gts, np.float32).astype(np.float64).reshape(-1, 5)
    x, y, w, h, a = g.T.copy()
    a = np.where(a >= 0, a - PI, a)
    swap = a < -PI / 2
    a = np.where(swap, a + PI / 2, a)
    w, h = np.where(swap, h, w), np.where(swap, w, h)
    wide = w > h
    ow, oh, oa = np.where(wide, w, h), np.where(wide, h, w), np.where(wide, a - PI / 2, a)
    c, s = np.cos(oa + PI / 2), np.sin(oa + PI / 2)
    xs = np.stack([-ow / 2, ow / 2, ow / 2, -ow / 2], 1)
    ys = np.stack([-oh / 2, -oh / 2, oh / 2, oh / 2], 1)
    px, py = c[:, None] * xs - s[:, None] * ys + x[:, None], s[:, None] * xs + c[:, None] * ys + y[:, None]
    return np.stack([x, y, ow, oh, oa], 1), np.stack([px.min(1), py.min(1), px.max(1), py.max(1)], 1) if len(g) else \
        np.zeros((0, 4))


# ---------------------------------------------------------------------------------------------------------------- IoU
def iou32(anchors, boxes_h):
    """(A, 4) x (K, 4) -> (A, K) float32, every operation a single fp32 operation in bbox_iou's order"""
    a, b = np.asarray(anchors, np.float32), np.asarray(boxes_h, np.float32)
    tl = np.maximum(a[:, None, :2], b[None, :, :2])
    br = np.minimum(a[:, None, 2:], b[None, :, 2:])
    inside = (tl < br).all(axis=2).astype(np.float32)
    area_i = ((br[..., 0] - tl[..., 0]) * (br[..., 1] - tl[..., 1])) * inside
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return area_i / ((area_a[:, None] + area_b[None, :]) - area_i)


def anchor_sources(anchors):
    """the anchor as cvt2_w_greater_than_h(boxes_x0y0x1y1_to_xywh([anchor, -pi/2])): (x, y, h, w, -pi) when h > w, else
    (x, y, w, h, -pi/2); float64"""
    a = np.asarray(anchors, np.float32).astype(np.float64)
    x, y, w, h = (a[:, 0] + a[:, 2]) / 2, (a[:, 1] + a[:, 3]) / 2, a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    tall = h > w
    return np.stack([x, y, np.where(tall, h, w), np.where(tall, w, h), np.where(tall, -PI, -PI / 2)], 1)


def bbox2loc_r(src, dst):
    eps = 1e-5
    return np.stack([(dst[:, 0] - src[:, 0]) / (src[:, 2] + 1), (dst[:, 1] - src[:, 1]) / (src[:, 3] + 1),
                     np.log(dst[:, 2] / (src[:, 2] + 1) + eps), np.log(dst[:, 3] / (src[:, 3] + 1) + eps),
                     dst[:, 4] - src[:, 4]], 1)


def targets(anchors, rboxes, rboxes_h, labels, pos=POS, neg_hi=NEG_HI, neg_lo=NEG_LO):
    """one image: prepared fp32 gts -> (raw_labels (A) int32 with -1 = ignored, loc targets (A, 5) float64, normalizer,
    max IoU (A) fp32, argmax (A))"""
    A = len(anchors)
    if len(rboxes) == 0:
        return np.zeros(A, np.int32), np.zeros((A, 5)), 1.0, np.zeros(A, np.float32), np.zeros(A, np.int64)
    iou = iou32(anchors, rboxes_h)
    arg = iou.argmax(1)                                   # numpy: the first among equal maxima
    mx = iou[np.arange(A), arg]
    raw = np.full(A, -1, np.int32)
    raw[(mx < np.float32(neg_hi)) & (mx >= np.float32(neg_lo))] = 0
    hit = mx >= np.float32(pos)
    raw[hit] = np.asarray(labels, np.int32)[arg[hit]]
    loc = np.zeros((A, 5))
    loc[hit] = bbox2loc_r(anchor_sources(anchors)[hit], np.asarray(rboxes, np.float32).astype(np.float64)[arg[hit]])
    return raw, loc, float(max(int((raw > 0).sum()), 1)), mx, arg


# --------------------------------------------------------------------------------------------------------------- loss
def focal_sum(logits, labels, alpha=0.25, gamma=2.0):
    """models/losses/focal_loss.py: sum over the rows with label >= 0 and every class; float64"""
    x = np.asarray(logits, np.float64)
    lab = np.asarray(labels)
    t = (np.arange(1, x.shape[1] + 1)[None, :] == lab[:, None]).astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-x))
    mv = np.maximum(-x, 0)
    ce = (1 - t) * x + mv + np.log(np.maximum(np.exp(-mv) + np.exp(-x - mv), 1e-10))
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * (1 - p_t) ** gamma * (alpha * t + (1 - alpha) * (1 - t))
    return float(loss[lab >= 0].sum())


def smooth_l1_sum(pred, target, beta):
    d = np.abs(np.asarray(pred, np.float64) - np.asarray(target, np.float64))
    return float((np.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta) if beta != 0 else d).sum())


def head_loss(bbox_pred, cls_score, locs, raws, beta, cls_w=1.0, loc_w=0.2):
    """per image (sum / max(#positives, 1)), then * weight / N: (roi_cls_loss, roi_loc_loss) float64"""
    N = len(raws)
    cls = loc = 0.0
    for i in range(N):
        pos = raws[i] > 0
        norm = max(int(pos.sum()), 1)
        cls += focal_sum(cls_score[i], raws[i]) / norm
        loc += smooth_l1_sum(np.asarray(bbox_pred[i])[pos], locs[i][pos], beta) / norm
    return cls * cls_w / N, loc * loc_w / N


# ------------------------------------------------------------------------------------------------------------- detect
def decode(anchors, loc):
    """loc2bbox_r from the proposals (x, y, h, w, -pi/2) | (x, y, w, h, 0), with the (x1+x2)/2, x2-x1 round trip; float64"""
    s = anchor_sources(anchors)
    s[:, 4] = np.where(s[:, 4] < -0.75 * PI, -PI / 2, 0.0)
    l = np.asarray(loc, np.float32).astype(np.float64)
    cx, cy = l[:, 0] * s[:, 2] + s[:, 0], l[:, 1] * s[:, 3] + s[:, 1]
    w, h = np.exp(l[:, 2]) * s[:, 2], np.exp(l[:, 3]) * s[:, 3]
    x1, y1, x2, y2 = cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h
    return np.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, l[:, 4] + s[:, 4]], 1)


def detect(anchors, loc, logits, thr, sx=1.0, sy=1.0):
    """-> dict(boxes (M, 5) float64 with the two size ratios applied, scores (M) float64, labels (M), anchor (M), counts
    (C), margins: the smallest distance of a score from thr and of an angle from +-pi/2) in class-major,
    anchor-ascending order"""
    box = decode(anchors, loc)
    p = 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float32).astype(np.float64)))
    ok = (box[:, 4] < PI / 2) & (box[:, 4] > -PI / 2)
    sel = ((p > thr) & ok[:, None]).T
    cls, anc = np.nonzero(sel)
    scaled = box * np.asarray([np.float32(sx), np.float32(sy), np.float32(sx), np.float32(sy), 1.0], np.float64)
    return dict(boxes=scaled[anc], scores=p.T[sel], labels=cls.astype(np.int32), anchor=anc, counts=sel.sum(1),
                score_margin=float(np.abs(p - thr).min()), angle_margin=float(np.abs(np.abs(box[:, 4]) - PI / 2).min()))


# ----------------------------------------------------------------------------------------------------- bilinear resize
def tf_taps(out_size, in_size):
    """(i0, i1, d) per destination index; the coordinate in fp32: x = float(i) * (float(in) / float(out)), clamped to
    [0, in - 1] when out > in"""
    s = np.float32(in_size) / np.float32(out_size)
    x = np.arange(out_size, dtype=np.float32) * s
    if out_size > in_size:
        x = np.clip(x, np.float32(0), np.float32(in_size - 1))
    i0 = np.floor(x)
    d = (x - i0).astype(np.float64)
    i0 = i0.astype(np.int64)
    return i0, np.minimum(i0 + 1, in_size - 1), d


def resize(top, H, W):
    """(N, Ht, Wt, C) -> (N, H, W, C), float64"""
    t = np.asarray(top, np.float64)
    i0, i1, dx = tf_taps(H, t.shape[1])
    j0, j1, dy = tf_taps(W, t.shape[2])
    dx, dy = dx[None, :, None, None], dy[None, None, :, None]
    a, b, c, d = t[:, i0][:, :, j0], t[:, i1][:, :, j0], t[:, i0][:, :, j1], t[:, i1][:, :, j1]
    return (dx * b + (1 - dx) * a) * (1 - dy) + (dx * d + (1 - dx) * c) * dy


def resize_weights(out_size, in_size):
    """(out, in) matrix of the 1-D rule: row i holds 1 - d at i0 and d at i1 (summed when they coincide)"""
    i0, i1, d = tf_taps(out_size, in_size)
    m = np.zeros((out_size, in_size))
    np.add.at(m, (np.arange(out_size), i0), 1 - d)
    np.add.at(m, (np.arange(out_size), i1), d)
    return m


def resize_t(g, Ht, Wt):
    """the transpose of `resize`: (N, H, W, C) -> (N, Ht, Wt, C), float64"""
    g = np.asarray(g, np.float64)
    return np.einsum("ip,jq,nijc->npqc", resize_weights(g.shape[1], Ht), resize_weights(g.shape[2], Wt), g)


def preimage_addends(H, W, Ht, Wt):
    """the largest number of fine pixels one coarse pixel collects from"""
    return int((resize_weights(H, Ht) != 0).sum(0).max() * (resize_weights(W, Wt) != 0).sum(0).max())


# ----------------------------------------------------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def anchors():
    """the config's five-level generator on FEATMAPS: (1113, 4) fp32 -- 17 waves of 64 and 25 more, five workgroups of
    256 with the last one partly empty"""
    import jdet_amd.models  # noqa: F401
    from jdet_amd.utils.registry import BOXES, build_from_cfg
    gen = build_from_cfg(dict(ANCHOR_CFG), BOXES)
    a = np.concatenate([x.numpy() for x in gen.grid_anchors(FEATMAPS)], 0).astype(np.float32)
    assert a.shape == (1113, 4)
    return a


def _raw_gts(K, seed):
    """K raw gts [x, y, w, h, a], each a randomly chosen anchor with its centre shifted by +-12 % of its size and its
    sides scaled by 0.8 .. 1.25, stated as a box at -pi/2 (horizontal extents (h, w)); every third one with pi added to
    its angle (the a >= 0 branch, the same box)"""
    rng = np.random.default_rng(seed)
    a = anchors()[rng.integers(0, len(anchors()), K)].astype(np.float64)
    w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    x = (a[:, 0] + a[:, 2]) / 2 + rng.uniform(-0.12, 0.12, K) * w
    y = (a[:, 1] + a[:, 3]) / 2 + rng.uniform(-0.12, 0.12, K) * h
    w, h = w * rng.uniform(0.8, 1.25, K), h * rng.uniform(0.8, 1.25, K)
    ang = np.where(np.arange(K) % 3 == 2, PI / 2, -PI / 2)
    return np.stack([x, y, h, w, ang], 1).astype(np.float32), rng.integers(1, 16, K).astype(np.int32)


def margins(mx, iou):
    """(distance of every anchor's max IoU from both thresholds, top-two gap), each the minimum over all anchors"""
    m = np.minimum(np.abs(mx.astype(np.float64) - NEG_HI), np.abs(mx.astype(np.float64) - POS)).min()
    if iou.shape[1] < 2:
        return float(m), np.inf
    top = np.sort(iou.astype(np.float64), axis=1)[:, -2:]
    return float(m), float((top[:, 1] - top[:, 0]).min())


@functools.lru_cache(maxsize=None)
def image(K, seed):
    """one image's gts: the first seed of seed, seed + 5, ... whose every anchor keeps its max IoU >= 1e-6 away from both
    thresholds and its two best gts >= 1e-6 apart, with positives, ignored and negatives all present.  No anchor is
    left out of the conditions: a seed that fails is replaced."""
    if K == 0:
        return dict(raw=np.zeros((0, 5), np.float32), labels=np.zeros((0,), np.int32), seed=seed)
    for s in range(seed, seed + 5 * 40, 5):
        raw, labels = _raw_gts(K, s)
        rb, rh = gt_prepare(raw)
        rb32, rh32 = rb.astype(np.float32), rh.astype(np.float32)
        iou = iou32(anchors(), rh32)
        lab, _, _, mx, _ = targets(anchors(), rb32, rh32, labels)
        m, gap = margins(mx, iou)
        kinds = ((lab > 0).any() and (lab == 0).any() and (lab < 0).any())
        if m >= 1e-6 and gap >= 1e-6 and kinds:
            return dict(raw=raw, labels=labels, seed=s)
    raise AssertionError("no seed gives K = %d a fixture with margins" % K)


KS = (0, 1, 70, GT_CHUNK + 1)


@functools.lru_cache(maxsize=None)
def batch(tie=False):
    """the gt fixture: images with K = 0, 1, 70 and GT_CHUNK + 1 gts (seeds 0 .. 3 onwards), packed.  tie: the K = 70
    image gets its gt 5 appended again with another label -- an exact tie that must resolve to gt 5."""
    imgs = [image(K, i) for i, K in enumerate(KS)]
    raws, labels = [im["raw"] for im in imgs], [im["labels"] for im in imgs]
    if tie:
        raws[2] = np.concatenate([raws[2], raws[2][5:6]], 0)
        labels[2] = np.concatenate([labels[2], np.asarray([labels[2][5] % 15 + 1], np.int32)], 0)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.int32)
    prepared = [gt_prepare(r) for r in raws]
    rb32 = np.concatenate([p[0] for p in prepared], 0).astype(np.float32)
    rh32 = np.concatenate([p[1] for p in prepared], 0).astype(np.float32)
    per = [targets(anchors(), rb32[offsets[i]:offsets[i + 1]], rh32[offsets[i]:offsets[i + 1]], labels[i])
           for i in range(len(imgs))]
    if tie:
        hit = (per[2][4] == 5) & (per[2][0] > 0)
        assert hit.any(), "the tie fixture needs positives of gt 5"
    return dict(raws=raws, labels=labels, offsets=offsets, rboxes=rb32, rboxes_h=rh32,
                gt_labels=np.concatenate(labels).astype(np.int32), raw_labels=np.stack([p[0] for p in per]),
                loc=np.stack([p[1] for p in per]), normalizer=np.asarray([p[2] for p in per], np.float64))


@functools.lru_cache(maxsize=None)
def detect_fixture(C=15, thr=0.05, seed=0):
    """loc / logits for the 1113 anchors: about 4 % of the scores pass, some angles leave (-pi/2, pi/2); every sigmoid
    is >= 1e-5 away from thr and every decoded angle >= 1e-5 away from +-pi/2 (asserted, nothing dropped)"""
    for s in range(seed, seed + 200):
        rng = np.random.default_rng(1000 + s)
        A = len(anchors())
        loc = (rng.standard_normal((A, 5)) * np.asarray([0.2, 0.2, 0.3, 0.3, 1.2])).astype(np.float32)
        logits = (rng.standard_normal((A, C)) * 1.2 - 5.0).astype(np.float32)
        d = detect(anchors(), loc, logits, thr)
        if d["score_margin"] >= 1e-5 and d["angle_margin"] >= 1e-5 and d["counts"].min() > 0:
            return dict(loc=loc, logits=logits, thr=thr, C=C)
    raise AssertionError("no seed gives a detect fixture with margins")
