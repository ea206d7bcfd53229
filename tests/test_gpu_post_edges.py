"""GPU: the YOLO post-processing code that only hipcc compiles, on the inputs where it can go wrong without tests/test_gpu_post.py
noticing: tied confidences, tied class maxima, candidate counts at the edges of the NMS size classes, odd head shapes, the HBM spill
arena under the wave NMS, and the pre-scanned entry of the fused Detect sink.  tests/hostemu compiles the #else branches of
csrc/post_core.h and has a scan of its own, so the CPU suite cannot reach any of this.  Every comparison is equality: the reference is
oracle/yolo_post.py under parity_checks.check_yolo, and for the scan kernels NumPy's float32 argmax / maximum on every anchor.  The
cases come from tests/post_cases.py; tests/test_post_cases_cpu.py shows that each is sound and would tell a changed tie rule apart.

device path -> cases
  yolo_scan_v8, float4 path (A % 4 == 0)      scan-v8 (84, 2)  (2100, 91: nc no multiple of 4)  (8400, 80)
  yolo_scan_v8, scalar path (A % 4 != 0)      scan-v8 (21, 1: fewer anchors than one wave holds)  (1029, 3)  (3549, 5)  (3549, 80);  every chain-v8
                                              and prescanned-v8 launch (3549, 3);  three frames per launch, so the frame stride is odd too
  yolo_scan_v8, empty class groups            (21, 1): groups 1..3;  (84, 2): groups 2, 3;  (1029, 3) and (3549, 5): group 3
  yolo_scan_v8, first maximum across groups   every scan-v8 case with nc >= 2 (17 % .. 95 % of the anchors tie across two groups);  chain-v8
  yolo_scan_v5, idle lanes (nc < 16)          scan-v5 (10647, 1)  (10647, 3)
  yolo_scan_v5, two classes in one lane       (10647, 17: lane 0 only)  (1029, 33)  (63, 80)  (10647, 80);  every chain-v5 launch (10647, 17)
  yolo_scan_v5, partial last row group        every A here: 63, 1029 and 10647 are all 3 mod 4
  yolo_scan_v5, lower class wins across lanes every scan-v5 case with nc >= 2 (23 % .. 74 % of the rows);  chain-v5
  phase A of yolo_post_frame (ballot compaction, four sub-passes per trip)
                                              every case: n_found and cand_anchor;  A = 21 and 63 end inside the first sub-pass, 3549 and 10647
                                              inside a trip;  chain frames with 0, 1 and up to 514 flags
  yolo_nms_reference_wave<1>                  chain, reference mode, N = 2, 3, 63, 64;  scan cases (2 or 5 candidates);  degenerate (28)
  yolo_nms_reference_wave<2>                  chain N = 65, 127, 128;  prescanned (65 and 66)
  yolo_nms_reference_wave<4>                  chain N = 129, 255, 256
  yolo_nms_reference_wave<8>                  chain N = 257, 511, 512
  block loop + block_argmax_first (shuffles)  chain N = 513, 514
  greedy mode (rank sort, ties to the higher index; the shared code as hipcc compiles it)
                                              chain, greedy mode, every N;  degenerate (0/0 between zero-area boxes)
  LDS arena                                   max_candidates = 1024:  chain-*-lds, degenerate-lds, scan cases, prescanned-v8
  HBM spill arena (max_candidates > 2048)     max_candidates = A:  chain-*-spill (the wave NMS keeps lc0..lc3, larea, lidx in HBM: lane 0 writes a
                                              row, the wave reads it on the next step), degenerate-spill (2100), prescanned-v5
  adas_yolo_post_scan_views                   every scan case;  prescanned
  adas_yolo_post_run_prescanned               prescanned-v8, prescanned-v5;  the lite layout is refused
A chain launch holds the fifteen edge counts of post_cases.CHAIN_N plus an empty and a one-candidate frame as seventeen frames of one
(layout, mode, arena): v8 at A = 3549, nc = 3 and v5 at A = 10647, nc = 17."""
import functools

import numpy as np
import pytest

import parity_checks as pc, post_cases as P
from oracle import yolo_post

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gpu_api
    assert gpu_api.L.lib().adas_device_count() > 0, "no HIP device"
    return gpu_api


# ------------------------------------------------------------------------------------------------ a. scan kernels, per anchor
def _check_scan(G, layout, heads):
    conf, cls, res = G.yolo_scan(heads, layout, P.LB, P.SCAN_SCORE, P.IOU)
    for f, head in enumerate(heads):
        probs = P.scan_probs(layout, head)
        want_cls = np.argmax(probs, 1)
        want_conf = probs[np.arange(len(probs)), want_cls]
        bad = np.nonzero(cls[f] != want_cls)[0]
        assert bad.size == 0, "frame %d: best_cls differs on %d anchors, first %d: got %d, want %d (row maximum %r at classes %s)" % (
            f, bad.size, bad[0], cls[f, bad[0]], want_cls[bad[0]], want_conf[bad[0]], np.nonzero(probs[bad[0]] == want_conf[bad[0]])[0][:8])
        np.testing.assert_array_equal(conf[f].view(np.uint32), want_conf.view(np.uint32), err_msg="frame %d best_conf bits" % f)
        want = yolo_post.detect_post(head, P.LB, P.MODEL[layout], P.SCAN_SCORE, P.IOU)
        assert res[f]["rc"] == 0 and not res[f]["overflow"] and 1 <= res[f]["n_found"] == len(want["cand_conf"]) <= 5
        pc.check_yolo(res[f], want)


@pytest.mark.parametrize("A,nc", P.SCAN_V8, ids=lambda v: str(v))
def test_scan_v8_every_anchor(G, A, nc):
    _check_scan(G, 0, P.scan_head_v8(A * 100 + nc, A, nc))


@pytest.mark.parametrize("A,nc", P.SCAN_V5, ids=lambda v: str(v))
def test_scan_v5_every_anchor(G, A, nc):
    _check_scan(G, 1, P.scan_head_v5(A * 100 + nc, A, nc))


# ------------------------------------------------------------------------------------------------ b. the chain on tied scores
@functools.lru_cache(maxsize=None)
def _chain(layout):
    frames = P.chain_frames(layout)
    return [n for n, _ in frames], np.stack([h for _, h in frames])


@functools.lru_cache(maxsize=None)
def _chain_want(layout, mode):
    return [yolo_post.detect_post(h, P.LB, P.MODEL[layout], P.BOX_SCORE, P.IOU, P.MODES[mode]) for h in _chain(layout)[1]]


def _cap(arena, A):
    return 1024 if arena == "lds" else A          # above 2048: the frame's working set is an HBM workspace


@pytest.mark.parametrize("arena", ["lds", "spill"])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "greedy"])
@pytest.mark.parametrize("layout", [0, 1], ids=["v8", "v5"])
def test_tied_chain_at_size_class_edges(G, layout, mode, arena):
    ns, heads = _chain(layout)
    A, nc = P.CHAIN_SHAPE[layout]
    assert _cap(arena, A) > 2048 or arena == "lds"
    yp = G.PP.YoloPost(layout, A, nc, P.BOX_SCORE, P.IOU, P.LB, mode, _cap(arena, A), max_batch=len(ns))
    try:
        res = yp.run_host(heads)
    finally:
        yp.close()
    for n, got, want in zip(ns, res, _chain_want(layout, mode)):
        assert got["rc"] == 0 and not got["overflow"] and got["n_found"] == n == len(want["cand_conf"]), "frame with N = %d: %r" % (
            n, (got["rc"], got["overflow"], got["n_found"]))
        try:
            pc.check_yolo(got, want)
        except AssertionError as e:
            raise AssertionError("frame with N = %d (%s, %s, %s arena): %s" % (n, P.MODEL[layout], P.MODES[mode], arena, e)) from None


# ------------------------------------------------------------------------------------------------ c. degenerate boxes
@pytest.mark.parametrize("arena", ["lds", "spill"])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "greedy"])
def test_degenerate_boxes(G, mode, arena):
    head = P.degenerate_head(7)
    with np.errstate(all="ignore"):
        want = yolo_post.detect_post(head, P.LB, "yolov8", P.BOX_SCORE, P.IOU, P.MODES[mode])
    got = G.yolo_post(head, 0, P.LB, P.BOX_SCORE, P.IOU, mode, cap=_cap(arena, head.shape[1]))
    assert got["rc"] == 0 and not got["overflow"] and got["n_found"] == len(want["cand_conf"]) == 28
    pc.check_yolo(got, want)


# ------------------------------------------------------------------------------------------------ d. pre-scanned entry
def _oracle_scan(layout, head):
    probs = P.scan_probs(layout, head)
    cls = np.argmax(probs, 1)
    return np.ascontiguousarray(probs[np.arange(len(probs)), cls], np.float32), cls.astype(np.int32)


@pytest.mark.parametrize("layout", [0, 1], ids=["v8", "v5"])
def test_run_prescanned_reads_the_scan_views(G, layout):
    """run() -> overwrite the views with the oracle's scan -> run_prescanned(): the same frame.  Then one more anchor raised above the
    threshold in the views alone (the head in HBM keeps its box and its low class values): the candidates gain exactly that anchor and the
    results are the oracle's on a head whose scores say the same -- the entry reads the views, not the head and not a stale scan."""
    A, nc = P.CHAIN_SHAPE[layout]
    head = P.tie_head(layout, 77 + layout, A, nc, 65)
    want = yolo_post.detect_post(head, P.LB, P.MODEL[layout], P.BOX_SCORE, P.IOU)
    lib = G.L.lib()
    yp = G.PP.YoloPost(layout, A, nc, P.BOX_SCORE, P.IOU, P.LB, 0, 1024 if layout == 0 else A, max_batch=1)
    buf = G.L.DeviceBuffer.from_array(head[None])
    try:
        yp.run_device(buf.ptr, 1)
        first = yp.fetch(0)
        assert first["rc"] == 0 and first["n_found"] == 65
        pc.check_yolo(first, want)
        d_conf, d_cls = G.scan_views(yp)

        def prescanned(conf, cls):
            G.L.check(lib.adas_memcpy_h2d(d_conf, G.L.ptr(conf), conf.nbytes))
            G.L.check(lib.adas_memcpy_h2d(d_cls, G.L.ptr(cls), cls.nbytes))
            G.L.check(lib.adas_yolo_post_run_prescanned(yp.h, buf.ptr, 1, None))
            return yp.fetch(0)

        conf, cls = _oracle_scan(layout, head)
        again = prescanned(conf, cls)
        assert again["rc"] == 0 and again["n_found"] == 65
        pc.check_yolo(again, want)
        pc.check_yolo(again, first)

        cand = set(want["cand_anchor"].tolist())
        a = next(x for x in range(int(want["cand_anchor"][32]), A) if x not in cand)       # lands in the middle of the list
        c = nc - 1
        conf[a], cls[a] = 0.96875, c
        raised = head.copy()
        if layout == 0:
            raised[4 + c, a] = 0.96875
        else:
            raised[a, 4], raised[a, 5 + c] = 1.0, 0.96875
        want2 = yolo_post.detect_post(raised, P.LB, P.MODEL[layout], P.BOX_SCORE, P.IOU)
        assert want2["cand_anchor"].tolist() == sorted(cand | {a})
        more = prescanned(conf, cls)
        assert more["rc"] == 0 and more["n_found"] == 66
        pc.check_yolo(more, want2)
    finally:
        buf.free(); yp.close()


def test_run_prescanned_refuses_the_lite_layout(G):
    yp = G.PP.YoloPost(2, 25200, 80, P.BOX_SCORE, P.IOU, P.LB, input_hw=(640, 640))
    buf = G.L.DeviceBuffer(64)
    try:
        with pytest.raises(Exception, match="v8- and v5-layout heads only"):
            G.L.check(G.L.lib().adas_yolo_post_run_prescanned(yp.h, buf.ptr, 1, None))
    finally:
        buf.free(); yp.close()
