"""Host references and input recipes for the tests of the shared NMS scan (csrc/nms_scan.h) at the sizes where it
changes regime.  numpy only: no GPU, no torch device.

The scan treats a 64-row block in one of two ways: while the block reaches at most kPrefetchCols = 128 column blocks
to its right (64 * ncols <= 8 * 1024) its words are prefetched into registers, wider blocks take the
fetch-after-resolve path.  `wide_row_blocks` restates which blocks are wide from the sizes and labels alone,
`wide_path_witnesses` counts the boxes that only the second path can suppress.

Everything here works in VISITING order: row / column i of `hit` is the i-th box visited, `greedy_keep` returns flags
by position.  `to_original` maps them back to the input order.
"""
import functools

import numpy as np

from tests import inputs as I

kPrefetchCols = 128          # nms_scan.h: kPre * kScanBlock / 64
LEVEL_SIZES = (8400, 0, 1, 333)   # label layout of the per-label cases: label 1 absent, a one-box label


def greedy_keep(hit):
    """hit (n, n) bool in visiting order, only i < j is read -> keep flags by position: visit i, keep it unless it is
    removed, a kept box removes every later box it hits (one row OR per kept box)"""
    n = hit.shape[0]
    assert hit.shape == (n, n) and hit.dtype == np.bool_
    removed = np.zeros(n, bool)
    keep = np.zeros(n, bool)
    for i in range(n):
        if removed[i]:
            continue
        keep[i] = True
        removed[i + 1:] |= hit[i, i + 1:]
    return keep


def to_original(keep_by_position, order):
    out = np.zeros(keep_by_position.shape[0], bool)
    out[np.asarray(order)] = keep_by_position
    return out


def same_label(labels_visit):
    l = np.asarray(labels_visit)
    return l[:, None] == l[None, :]


# ------------------------------------------------------------------------------------------------ horizontal boxes
def _is_dyadic16(thr):
    return float(thr) * 16.0 == float(int(float(thr) * 16.0)) and 0.0 <= float(thr) < 1.0


def hbb_hits_exact(boxes_xyxy_sorted, thr, chunk=512):
    """the exact decision `inter > thr * union` for every pair, (n, n) bool.

    Valid only under the horizontal recipe (asserted): integer corners, even widths and heights of at most 80, thr a
    multiple of 1/16 in [0, 1).  Then inter, both areas and the union are integers <= 12800, `thr * union` is exact in
    float64, and the kernel's fp32 `inter / uni > thr` takes the same decision: centre and size are exact in fp32
    (half-integers / even integers far below 2^24), so are inter and uni, and a quotient that is not exactly thr is
    at least 1 / (16 * 12800) = 4.9e-6 away from it against an fp32 ulp of 6e-8 below 1.  A threshold like 0.7 is
    NOT allowed: inter / uni == 7/10 ties differently against the fp32 and the float64 nearest of 0.7."""
    b = np.asarray(boxes_xyxy_sorted)
    assert b.ndim == 2 and b.shape[1] == 4
    bi = b.astype(np.int64)
    assert np.array_equal(bi.astype(b.dtype), b), "integer corners"
    w, h = bi[:, 2] - bi[:, 0], bi[:, 3] - bi[:, 1]
    assert (w > 0).all() and (h > 0).all() and (w <= 80).all() and (h <= 80).all() and not (w & 1).any() \
        and not (h & 1).any(), "even widths / heights in 2 .. 80"
    assert np.abs(bi).max() < 1 << 20
    assert _is_dyadic16(thr), "threshold must be a multiple of 1/16 in [0, 1)"
    n = b.shape[0]
    bi, area = bi.astype(np.int32), (w * h).astype(np.int32)     # every intermediate is far below 2^31
    hit = np.zeros((n, n), bool)
    for r0 in range(0, n, chunk):
        r = bi[r0:r0 + chunk, None, :]
        iw = np.minimum(r[..., 2], bi[None, :, 2]) - np.maximum(r[..., 0], bi[None, :, 0])
        ih = np.minimum(r[..., 3], bi[None, :, 3]) - np.maximum(r[..., 1], bi[None, :, 1])
        inter = np.maximum(iw, 0) * np.maximum(ih, 0)
        union = area[r0:r0 + chunk, None] + area[None, :] - inter
        hit[r0:r0 + chunk] = inter.astype(np.float64) > float(thr) * union.astype(np.float64)
    return hit


def hbb_hits_fp32_kernel_formula(boxes_xyxy_sorted, thr, chunk=512):
    """the horizontal path restated in numpy fp32, operation by operation: ops/nms.py turns corners into centre / size,
    nms_mask_kernel<true> rebuilds the corners, `uni > 0 ? inter / uni : 0` and `> thr`"""
    f = np.float32
    b = np.asarray(boxes_xyxy_sorted, f)
    xc, yc = (b[:, 0] + b[:, 2]) * f(0.5), (b[:, 1] + b[:, 3]) * f(0.5)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    x1, x2, y1, y2 = xc - f(0.5) * w, xc + f(0.5) * w, yc - f(0.5) * h, yc + f(0.5) * h
    area = w * h
    n = b.shape[0]
    hit = np.zeros((n, n), bool)
    for r0 in range(0, n, chunk):
        s = slice(r0, r0 + chunk)
        iw = np.minimum(x2[s, None], x2[None, :]) - np.maximum(x1[s, None], x1[None, :])
        ih = np.minimum(y2[s, None], y2[None, :]) - np.maximum(y1[s, None], y1[None, :])
        inter = np.maximum(iw, f(0)) * np.maximum(ih, f(0))
        uni = area[s, None] + area[None, :] - inter
        assert inter.dtype == f and uni.dtype == f
        ovr = np.where(uni > 0, inter / np.where(uni > 0, uni, f(1)), f(0))
        hit[s] = ovr > f(thr)
    return hit


@functools.lru_cache(maxsize=None)
def hbb_case(n):
    """the horizontal recipe: (boxes (n, 4) xyxy fp32, scores (n,) fp32, order (n,) int32 by descending score).
    24 cluster centres, jittered integer centres, integer half sizes 4 .. 40: heavy overlap inside a cluster, exact
    arithmetic everywhere (see hbb_hits_exact)"""
    rng = np.random.default_rng(7)
    centres = rng.integers(40, 1000, size=(24, 2))
    c = centres[rng.integers(0, 24, size=n)] + rng.integers(-12, 13, size=(n, 2))
    half = rng.integers(4, 41, size=(n, 2))
    boxes = np.concatenate([c - half, c + half], 1).astype(np.float32)
    scores = (rng.uniform(0, 1, n) + np.arange(n) * 1e-7).astype(np.float32)
    for a in (boxes, scores):
        a.setflags(write=False)
    return boxes, scores, score_order(scores)


# --------------------------------------------------------------------------------------------------- rotated boxes
@functools.lru_cache(maxsize=None)
def rotated_case(n):
    """the recipe of test_gpu_iou_nms.test_nms_vs_oracle: half random, half clustered OBBs, tie-free scores, then 15
    random labels -> (dets (n, 5), scores, order by descending score, labels (n,) fp32)"""
    rng = np.random.default_rng(n)
    dets = np.concatenate([I.random_obbs(rng, n // 2), I.clustered_obbs(rng, n - n // 2, 24, 1024.0)], 0)
    scores = (rng.uniform(0, 1, n) + np.arange(n) * 1e-7).astype(np.float32)
    labels = rng.integers(0, 15, n).astype(np.float32)
    for a in (dets, scores, labels):
        a.setflags(write=False)
    return dets, scores, score_order(scores), labels


def score_order(scores):
    o = np.argsort(-np.asarray(scores), kind="stable").astype(np.int32)
    o.setflags(write=False)
    return o


def label_order(scores, labels):
    """the visiting order of ml_nms_rotated / nms_keep_mask(labels=): label by label, descending score inside"""
    o = score_order(scores)
    o = o[np.argsort(np.asarray(labels)[o], kind="stable")].astype(np.int32)
    o.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def level_labels(seed=8734):
    """labels 0 .. 3 with LEVEL_SIZES boxes each, shuffled over the n = 8734 input positions"""
    rng = np.random.default_rng(seed)
    l = np.concatenate([np.full(s, i) for i, s in enumerate(LEVEL_SIZES)]).astype(np.float32)
    l = l[rng.permutation(l.size)]
    l.setflags(write=False)
    return l


def rotated_hits_of_kept_rows(dets_sorted, keep_by_position, thr, cmp_ge, labels_visit=None):
    """(n, n) bool with the rows of the KEPT boxes filled from the CPU oracle's IoU (the rows of suppressed boxes never
    take part in a greedy pass and stay False): what wide_path_witnesses needs, at k * n instead of n * n IoUs"""
    from oracle import oracle as O
    d = np.ascontiguousarray(np.asarray(dets_sorted)[:, :5], np.float32)
    n = d.shape[0]
    rows = np.flatnonzero(keep_by_position)
    hit = np.zeros((n, n), bool)
    for r0 in range(0, rows.size, 1024):
        r = rows[r0:r0 + 1024]
        iou = O.box_iou_rotated(d[r], d)
        h = (iou >= np.float32(thr)) if cmp_ge else (iou > np.float32(thr))
        if labels_visit is not None:
            l = np.asarray(labels_visit)
            h &= l[r][:, None] == l[None, :]
        hit[r] = h
    return hit


# ------------------------------------------------------------------------------------------------ the scan's regimes
def wide_row_blocks(n, labels_visit=None, n_labels=1):
    """bool per 64-row block: does the scan take the fetch-after-resolve path for it?  Restates the tile kernels'
    tile_jmax (unlabelled: always the last column block; labelled: the last column block whose label range meets the
    row block's) and the scan's `min(tile_jmax[c], c_hi - 1) - c` (c_hi: the end of the workgroup's label segment, the
    end of everything when n_labels == 1).  A block shared by several labels counts as wide if it is for any of them."""
    cb = (n + 63) >> 6
    jmax = np.full(cb, cb - 1)
    if labels_visit is not None:
        l = np.asarray(labels_visit, np.float64)
        lo = np.array([l[c * 64:(c + 1) * 64].min() for c in range(cb)])
        hi = np.array([l[c * 64:(c + 1) * 64].max() for c in range(cb)])
        for r in range(cb):
            meets = ~((hi[r] < lo[r:]) | (hi[r:] < lo[r]))
            jmax[r] = r + np.flatnonzero(meets).max()
    wide = np.zeros(cb, bool)
    if n_labels == 1 or labels_visit is None:
        segs = [(0, n)]
    else:
        l = np.asarray(labels_visit)
        assert (np.diff(l) >= 0).all()
        segs = [(int(np.searchsorted(l, g, "left")), int(np.searchsorted(l, g, "right"))) for g in range(n_labels)]
    for lo_, hi_ in segs:
        if lo_ >= hi_:
            continue
        c_lo, c_hi = lo_ >> 6, (hi_ + 63) >> 6
        for c in range(c_lo, c_hi):
            if max(min(jmax[c], c_hi - 1) - c, 0) > kPrefetchCols:
                wide[c] = True
    return wide


def wide_path_witnesses(keep, hit, n, wide=None):
    """how many boxes are suppressed ONLY through the scan's second path: boxes hit by at least one earlier kept box,
    where every such kept box lies in a wide row block (default: the first col_blocks - 129 blocks, the unlabelled
    case; pass wide_row_blocks(...) for labelled inputs) and in another block than the box itself (the diagonal tile
    is resolved by the readlane chain whatever the path).  A scan that drops or mis-addresses the ORs of the wide
    blocks keeps at least the first of them.  keep / hit by visiting position; only the kept rows of hit are read."""
    cb = (n + 63) >> 6
    if wide is None:
        wide = np.arange(cb) < cb - (kPrefetchCols + 1)
    assert keep.shape == (n,) and hit.shape == (n, n) and wide.shape == (cb,)
    kept = np.flatnonzero(keep)
    blk = np.arange(n) >> 6
    h = hit[kept] & (np.arange(n)[None, :] > kept[:, None])
    other_way = (~wide[blk[kept]])[:, None] | (blk[kept][:, None] == blk[None, :])
    any_hit = h.any(0)
    assert not (any_hit & keep).any(), "keep is not the greedy solution of hit"
    return int((any_hit & ~(h & other_way).any(0)).sum())
