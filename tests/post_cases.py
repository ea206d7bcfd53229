"""Seeded YOLO heads for the device-only post-processing paths (NumPy only): tied confidences, tied class maxima, degenerate boxes,
and the oracle with one tie rule changed.  tests/test_post_cases_cpu.py shows on the CPU that every case is sound and not vacuous;
tests/test_gpu_post_edges.py runs the same cases through the HIP kernels.

All values are float32-exact (dyadic grids) unless said otherwise, so a confidence that is meant to tie does tie, bit for bit."""
import types

import numpy as np

from oracle import yolo_post

BOX_SCORE, IOU = 0.4, 0.45          # the chain cases
SCAN_SCORE = 0.9                    # the scan cases: above every grid value, so only the planted handful become candidates
LB = yolo_post.letterbox_params((720, 1280), (640, 640))
MODEL = {0: "yolov8", 1: "yolov5"}
MODES = {0: "reference", 1: "greedy"}

# Candidate counts at the edges of the NMS size classes (64 candidates per register slot, one wave up to 512, the block loop above);
# an empty and a one-candidate frame sit in between.
CHAIN_N = (2, 3, 63, 64, 0, 65, 127, 128, 129, 255, 1, 256, 257, 511, 512, 513, 514)
CHAIN_SHAPE = {0: (3549, 3), 1: (10647, 17)}       # layout -> (A, nc)

SCAN_V8 = ((21, 1), (84, 2), (1029, 3), (3549, 5), (3549, 80), (2100, 91), (8400, 80))
SCAN_V5 = ((63, 80), (1029, 33), (10647, 1), (10647, 3), (10647, 17), (10647, 80))
SCAN_FRAMES = 3


def _cluster_boxes(rng, n_hot):
    """[n_hot, 4] cx, cy, w, h on integers: about n_hot / 5 clusters whose members are shifted by up to a third of the cluster's size, so
    the IoU inside a cluster falls on both sides of the threshold and which of two tied members survives depends on their order."""
    n_cl = max(1, n_hot // 5)
    ccx, ccy = rng.integers(80, 560, n_cl), rng.integers(200, 440, n_cl)
    cw, ch = rng.integers(24, 120, n_cl), rng.integers(24, 100, n_cl)
    k = rng.integers(0, n_cl, n_hot)
    dx = rng.integers(-(cw[k] // 3), cw[k] // 3 + 1)
    dy = rng.integers(-(ch[k] // 3), ch[k] // 3 + 1)
    return np.stack([ccx[k] + dx, ccy[k] + dy, cw[k] + rng.integers(-4, 5, n_hot), ch[k] + rng.integers(-4, 5, n_hot)], 1).astype(np.float32)


def _background_boxes(rng, A):
    return np.stack([rng.integers(50, 590, A), rng.integers(180, 460, A), rng.integers(20, 120, A), rng.integers(20, 100, A)], 1).astype(np.float32)


def _other_class(rng, nc, c, same):
    """A class that the scan keeps apart from class c (same(c, d) is False), or -1 if there is none."""
    others = [d for d in range(nc) if not same(c, d)]
    return int(rng.choice(others)) if others else -1


def tie_head_v8(seed, A, nc, n_hot):
    """[4+nc][A]: exactly n_hot anchors above BOX_SCORE.  Hot scores are 8/16 .. 15/16 (8 levels), the background k/64 <= 0.25; on a third
    of the hot anchors a class of ANOTHER class group of yolo_scan_v8 (groups of ceil(nc/4) classes) holds the hot value too."""
    rng = np.random.default_rng(seed)
    out = np.zeros((4 + nc, A), np.float32)
    out[0:4] = _background_boxes(rng, A).T
    out[4:] = rng.integers(0, 17, (nc, A)) / 64.0
    hot = np.sort(rng.choice(A, n_hot, replace=False))
    if n_hot:
        out[0:4, hot] = _cluster_boxes(rng, n_hot).T
    cpg = (nc + 3) // 4
    for a in hot:
        v, c = rng.integers(8, 16) / 16.0, int(rng.integers(nc))
        out[4 + c, a] = v
        if rng.integers(3) == 0:
            d = _other_class(rng, nc, c, lambda p, q: p // cpg == q // cpg)
            if d >= 0:
                out[4 + d, a] = v
    return out


def tie_head_v5(seed, A, nc, n_hot):
    """[A][5+nc]: exactly n_hot anchors above BOX_SCORE.  Hot rows have obj and one class in {12, 14, 16}/16 (6 distinct products, exact
    in fp32); the background has obj <= 0.5 and classes <= 0.5, so its products are <= 0.25.  On a third of the hot rows a class of ANOTHER
    lane of yolo_scan_v5 (class % 16) holds the hot value too."""
    rng = np.random.default_rng(seed)
    out = np.zeros((A, 5 + nc), np.float32)
    out[:, 0:4] = _background_boxes(rng, A)
    out[:, 4] = rng.integers(0, 9, A) / 16.0
    out[:, 5:] = rng.integers(0, 9, (A, nc)) / 16.0
    hot = np.sort(rng.choice(A, n_hot, replace=False))
    if n_hot:
        out[hot, 0:4] = _cluster_boxes(rng, n_hot)
    for a in hot:
        out[a, 4] = rng.choice((12, 14, 16)) / 16.0
        v, c = rng.choice((12, 14, 16)) / 16.0, int(rng.integers(nc))
        out[a, 5 + c] = v
        if rng.integers(3) == 0:
            d = _other_class(rng, nc, c, lambda p, q: p % 16 == q % 16)
            if d >= 0:
                out[a, 5 + d] = v
    return out


def tie_head(layout, seed, A, nc, n_hot):
    return (tie_head_v8 if layout == 0 else tie_head_v5)(seed, A, nc, n_hot)


def chain_frames(layout):
    """The frames of one chain launch, in CHAIN_N order: [(N, head)]."""
    A, nc = CHAIN_SHAPE[layout]
    return [(n, tie_head(layout, 1000 * (layout + 1) + n, A, nc, n)) for n in CHAIN_N]


def _special_anchors(rng, A):
    """Disjoint anchor sets: all-zero, maximum in the last class, planted candidates (a handful), and for v5 obj = 0."""
    perm = rng.permutation(A)
    n = max(1, A // 20)
    n_cand = min(5, max(1, A // 8))
    return perm[:n], perm[n:2 * n], perm[2 * n:2 * n + n_cand], perm[2 * n + n_cand:3 * n + n_cand], perm[3 * n + n_cand:]


def scan_head_v8(seed, A, nc, frames=SCAN_FRAMES):
    """[frames][4+nc][A], every frame distinct: class values k/8, k < 7, so the maximum ties within a class group, across groups, or not at
    all; a twentieth of the anchors all zero (class 0, confidence 0), a twentieth with a single maximum 7/8 in the last class, and a
    handful at 15/16, the only anchors above SCAN_SCORE."""
    rng = np.random.default_rng(seed)
    out = np.zeros((frames, 4 + nc, A), np.float32)
    for f in range(frames):
        out[f, 0:4] = _background_boxes(rng, A).T
        out[f, 4:] = rng.integers(0, 7, (nc, A)) / 8.0
        zero, last, cand, _, _ = _special_anchors(rng, A)
        out[f, 4:, zero] = 0
        out[f, 4 + nc - 1, last] = 0.875
        out[f, 4 + rng.integers(0, nc, len(cand)), cand] = 0.9375
    return out


def scan_head_v5(seed, A, nc, frames=SCAN_FRAMES):
    """[frames][A][5+nc], every frame distinct: obj in {1..4}/4 and classes k/8, k < 7 (products exact, ties within and across the 16
    lanes); a twentieth of the rows all zero, a twentieth with obj = 0, a twentieth with a single maximum 7/8 in the last class, a handful
    with obj = 1 and one class 15/16, the only rows above SCAN_SCORE; and a quarter of the rest uniform(0, 0.9) float32 values, where
    cls * obj rounds in fp32."""
    rng = np.random.default_rng(seed)
    out = np.zeros((frames, A, 5 + nc), np.float32)
    for f in range(frames):
        out[f, :, 0:4] = _background_boxes(rng, A)
        out[f, :, 4] = rng.integers(1, 5, A) / 4.0
        out[f, :, 5:] = rng.integers(0, 7, (A, nc)) / 8.0
        zero, last, cand, obj0, rest = _special_anchors(rng, A)
        rough = rest[:len(rest) // 4]
        out[f, rough, 4:] = rng.uniform(0, 0.9, (len(rough), 1 + nc)).astype(np.float32)
        out[f, zero, 4:] = 0
        out[f, obj0, 4] = 0
        out[f, last, 4] = 1.0
        out[f, last, 5 + nc - 1] = 0.875
        out[f, cand, 4] = 1.0
        out[f, cand, 5 + rng.integers(0, nc, len(cand))] = 0.9375
    return out


def scan_probs(layout, head):
    """One frame's class scores [A][nc] as the reference forms them (yoloDetector.py:122-124): float32, for v5 cls * obj rounded in fp32."""
    return head[4:].T if layout == 0 else head[:, 5:] * head[:, 4:5]


def degenerate_head(seed):
    """v8 [4+2][2100] (more than 2048 anchors, so that a spill arena can be asked for): four groups of exact duplicate boxes (IoU exactly 1) with tied and distinct scores, and on one centre boxes of zero
    width, zero height and both.  In greedy mode (no "+1" in the areas) two zero-area boxes give 0/0: the reference drops the later one
    because `NaN <= thr` is false.  Call the oracle inside np.errstate(all="ignore")."""
    rng = np.random.default_rng(seed)
    A, nc = 2100, 2
    out = np.zeros((4 + nc, A), np.float32)
    out[0:4] = _background_boxes(rng, A).T
    out[4:] = rng.integers(0, 17, (nc, A)) / 64.0
    hot = np.sort(rng.choice(A, 28, replace=False))
    box = _cluster_boxes(rng, 4)
    for i, a in enumerate(hot[:16]):
        out[0:4, a] = box[i % 4]
    flat = ((0, 0), (0, 0), (0, 7), (0, 7), (9, 0), (9, 0), (0, 0), (5, 0), (0, 3), (6, 6), (6, 6), (0, 0))
    for a, (w, h) in zip(hot[16:], flat):
        out[0:4, a] = (300, 320, w, h)
    out[4 + rng.integers(0, nc, 28), hot] = rng.integers(8, 12, 28) / 16.0
    return out


class _NumpyWith:
    """numpy with some functions replaced; everything else is numpy's."""

    def __init__(self, **changed):
        self.__dict__.update(changed)

    def __getattr__(self, name):
        return getattr(np, name)


def _last_argmax(a, *args, **kw):
    a = np.asarray(a)
    return len(a) - 1 - np.argmax(a[::-1], *args, **kw)


def _argsort_low_index_first(a, kind=None):
    return np.argsort(-np.asarray(a), kind="stable")[::-1]          # reversed by the caller: descending, ties -> LOWER index first


def _recompiled(fn, **changed):
    """fn's own code, run with a numpy in which `changed` is changed: the oracle's function with exactly one rule different."""
    return types.FunctionType(fn.__code__, dict(vars(yolo_post), np=_NumpyWith(**changed)), fn.__name__, fn.__defaults__)


_MUTANT_NMS = {"last-max": _recompiled(yolo_post.fast_soft_nms, argmax=_last_argmax),
               "low-index-first": _recompiled(yolo_post.fast_nms, argsort=_argsort_low_index_first)}


def mutant_detect_post(kind, output, lb, model_type="yolov8", box_score=0.4, iou_thr=0.45):
    """oracle.yolo_post.detect_post with one tie rule changed.  "last-max": reference mode whose selection takes the LAST maximum of the
    remaining scores (the packed key of the wave NMS with j in place of ~j).  "low-index-first": greedy mode whose order puts the LOWER
    index first among equal scores."""
    boxes, cls, conf, aidx = yolo_post.process_output(output, model_type, box_score)
    xywh = yolo_post.convert_boxes_coordinate(boxes, lb)
    keep = _MUTANT_NMS[kind](xywh, conf, iou_thr)
    r = yolo_post.rect_infos(xywh, conf, cls, keep)
    r.update(keep=np.asarray(keep, np.int64), cand_xywh=xywh, cand_conf=conf, cand_cls=cls, cand_anchor=aidx)
    return r
