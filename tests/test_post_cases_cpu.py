"""CPU: the cases of tests/post_cases.py, which tests/test_gpu_post_edges.py runs through the HIP kernels, are sound and not vacuous.

Sound: the host emulation of csrc/post_core.h equals the oracle under parity_checks.check_yolo in both NMS modes, and the candidate
count is the intended N.  Not vacuous (conditions stated here, met by the oracle alone, for the seeds post_cases.py fixes):
  tie cases, N >= 63   at most N / 4 distinct confidences; two survivors share a confidence; the keep list of an oracle that takes the
                       LAST maximum (reference mode) or puts the LOWER index first on ties (greedy mode) differs from the oracle's
  scan heads           at least 5 % of the anchors have a tied maximum (nc >= 2: one class cannot tie); for v8 at nc >= 5 at least 1 %
                       tie across two class groups of yolo_scan_v8; at least one anchor is all zero, one has its maximum in the last
                       class alone, and for v5 one row has obj = 0 and one product cls * obj is inexact in float64 (it rounds in fp32)
  degenerate head      boxes with IoU exactly 1 and zero-area boxes are among the candidates, and greedy mode meets 0/0
Each test prints one line per case, past pytest's capture."""
import functools

import numpy as np
import pytest

import emu_api, parity_checks as pc, post_cases as P
from oracle import yolo_post


CHAIN_AT_129 = P.CHAIN_N.index(129)


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


@functools.lru_cache(maxsize=None)
def _frames(layout):
    return P.chain_frames(layout)


@pytest.mark.parametrize("layout", [0, 1], ids=["v8", "v5"])
def test_mutant_builders_change_one_rule_only(layout):
    """With numpy's own argmax / argsort put back, the rebuilt functions are the oracle's: the mutants differ in the tie rule alone."""
    same_ref = P._recompiled(yolo_post.fast_soft_nms, argmax=np.argmax)
    same_greedy = P._recompiled(yolo_post.fast_nms, argsort=np.argsort)
    n, head = _frames(layout)[CHAIN_AT_129]
    boxes, cls, conf, _ = yolo_post.process_output(head, P.MODEL[layout], P.BOX_SCORE)
    xywh = yolo_post.convert_boxes_coordinate(boxes, P.LB)
    np.testing.assert_array_equal(same_ref(xywh, conf, P.IOU), yolo_post.fast_soft_nms(xywh, conf, P.IOU))
    np.testing.assert_array_equal(same_greedy(xywh, conf, P.IOU), yolo_post.fast_nms(xywh, conf, P.IOU))
    # and on distinct scores no tie rule decides
    distinct = np.linspace(0.5, 0.9, len(conf))
    for kind, fn in (("last-max", yolo_post.fast_soft_nms), ("low-index-first", yolo_post.fast_nms)):
        np.testing.assert_array_equal(P._MUTANT_NMS[kind](xywh, distinct, P.IOU), fn(xywh, distinct, P.IOU))


@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "greedy"])
@pytest.mark.parametrize("layout", [0, 1], ids=["v8", "v5"])
def test_tie_chain_cases(layout, mode, capsys):
    for n, head in _frames(layout):
        want = yolo_post.detect_post(head, P.LB, P.MODEL[layout], P.BOX_SCORE, P.IOU, P.MODES[mode])
        got = emu_api.yolo_post(head, layout, P.LB, P.BOX_SCORE, P.IOU, mode)
        assert got["n_found"] == len(want["cand_conf"]) == n and not got["overflow"], n
        pc.check_yolo(got, want)
        kind = "last-max" if mode == 0 else "low-index-first"
        mut = P.mutant_detect_post(kind, head, P.LB, P.MODEL[layout], P.BOX_SCORE, P.IOU)
        differs = mut["keep"].tolist() != want["keep"].tolist()
        n_conf = len(np.unique(want["cand_conf"]))
        shared = len(want["conf"]) - len(np.unique(want["conf"]))
        # on a third of the hot anchors two classes tie: the candidate's class must be the lower one
        probs = P.scan_probs(layout, head)[want["cand_anchor"]]
        n_cls_tie = int(((probs == probs.max(1, keepdims=True)).sum(1) > 1).sum()) if n else 0
        _say(capsys, "tie %s %-9s N=%3d  distinct confidences %2d  survivors %3d (%3d share a confidence)  class ties %3d  %s differs: %s"
              % (P.MODEL[layout], P.MODES[mode], n, n_conf, len(want["keep"]), shared, n_cls_tie, kind, differs))
        if n >= 63:
            assert n_conf <= n / 4, n
            assert shared >= 1, n
            assert differs, (n, kind)
            assert n_cls_tie >= n // 8, n


@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "greedy"])
def test_degenerate_head(mode, capsys):
    head = P.degenerate_head(7)
    with np.errstate(all="ignore"):
        want = yolo_post.detect_post(head, P.LB, "yolov8", P.BOX_SCORE, P.IOU, P.MODES[mode])
    got = emu_api.yolo_post(head, 0, P.LB, P.BOX_SCORE, P.IOU, mode)
    assert got["n_found"] == 28
    pc.check_yolo(got, want)
    b = want["cand_xywh"]
    n_dup = len(b) - len(np.unique(b, axis=0))
    n_flat = int(((b[:, 2] == 0) | (b[:, 3] == 0)).sum())
    n_point = int(((b[:, 2] == 0) & (b[:, 3] == 0)).sum())
    _say(capsys, "degenerate %-9s N=%d  duplicate boxes %d  zero-area boxes %d (%d points)  survivors %d" % (P.MODES[mode], len(b), n_dup, n_flat, n_point, len(want["keep"])))
    assert n_dup >= 12 and n_flat == 10 and n_point >= 3       # three points on one centre: two of them meet as 0/0 in greedy mode
    assert 0 < len(want["keep"]) < 28


def _scan_case_stats(layout, heads, nc):
    tied = cross = zero = last = 0
    cpg = (nc + 3) // 4
    for head in heads:
        p = P.scan_probs(layout, head)
        at_max = p == p.max(1, keepdims=True)
        tied += int((at_max.sum(1) > 1).sum())
        grp = np.arange(nc) // cpg
        cross += int((np.stack([(at_max & (grp == g)).any(1) for g in range(4)]).sum(0) > 1).sum())
        zero += int((~p.any(1)).sum())
        last += int((at_max[:, nc - 1] & (at_max.sum(1) == 1)).sum())
    return tied, cross, zero, last


@pytest.mark.parametrize("A,nc", P.SCAN_V8, ids=lambda v: str(v))
def test_scan_heads_v8(A, nc, capsys):
    heads = P.scan_head_v8(A * 100 + nc, A, nc)
    assert heads.shape == (P.SCAN_FRAMES, 4 + nc, A) and not np.array_equal(heads[0], heads[1])
    tied, cross, zero, last = _scan_case_stats(0, heads, nc)
    n_cand = []
    for head in heads:
        want = yolo_post.detect_post(head, P.LB, "yolov8", P.SCAN_SCORE, P.IOU)
        pc.check_yolo(emu_api.yolo_post(head, 0, P.LB, P.SCAN_SCORE, P.IOU, 0), want)
        n_cand.append(len(want["cand_conf"]))
    total = A * P.SCAN_FRAMES
    _say(capsys, "scan v8 A=%5d nc=%2d  tied maximum %5.1f %%  across groups %5.1f %%  all-zero %d  last class %d  candidates %s"
          % (A, nc, 100 * tied / total, 100 * cross / total, zero, last, n_cand))
    assert zero >= P.SCAN_FRAMES and last >= P.SCAN_FRAMES and all(1 <= n <= 5 for n in n_cand)
    if nc >= 2:
        assert tied >= 0.05 * total
    if nc >= 5:
        assert cross >= 0.01 * total


@pytest.mark.parametrize("A,nc", P.SCAN_V5, ids=lambda v: str(v))
def test_scan_heads_v5(A, nc, capsys):
    heads = P.scan_head_v5(A * 100 + nc, A, nc)
    assert heads.shape == (P.SCAN_FRAMES, A, 5 + nc) and not np.array_equal(heads[0], heads[1])
    tied, _, zero, last = _scan_case_stats(1, heads, nc)
    n_cand, obj0, inexact, lanes = [], 0, 0, 0
    for head in heads:
        want = yolo_post.detect_post(head, P.LB, "yolov5", P.SCAN_SCORE, P.IOU)
        pc.check_yolo(emu_api.yolo_post(head, 1, P.LB, P.SCAN_SCORE, P.IOU, 0), want)
        n_cand.append(len(want["cand_conf"]))
        obj0 += int(((head[:, 4] == 0) & head[:, 5:].any(1)).sum())
        p64 = head[:, 5:].astype(np.float64) * head[:, 4:5].astype(np.float64)
        inexact += int((p64 != P.scan_probs(1, head)).any(1).sum())
        p = P.scan_probs(1, head)
        at_max = p == p.max(1, keepdims=True)
        lanes += int((np.stack([at_max[:, s::16].any(1) for s in range(16)]).sum(0) > 1).sum())
    total = A * P.SCAN_FRAMES
    _say(capsys, "scan v5 A=%5d nc=%2d  tied maximum %5.1f %%  across lanes %5.1f %%  all-zero %d  obj=0 %d  last class %d  inexact rows %d  candidates %s"
          % (A, nc, 100 * tied / total, 100 * lanes / total, zero, obj0, last, inexact, n_cand))
    assert zero >= P.SCAN_FRAMES and obj0 >= P.SCAN_FRAMES and last >= P.SCAN_FRAMES and inexact >= P.SCAN_FRAMES
    assert all(1 <= n <= 5 for n in n_cand)
    if nc >= 2:
        assert tied >= 0.05 * total and lanes >= 0.05 * total
