"""Adapters that give the HIP library the same call shape as tests/emu_api.py."""
import ctypes as C
import numpy as np
from conftest import load_pkg
import importlib

load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")


def yolo_post(head, layout, lb, box_score, iou, nms_mode=0, cap=1024, batch_copies=1, input_hw=None):
    head = np.ascontiguousarray(head, np.float32)
    if layout == 0:
        nc, A = head.shape[0] - 4, head.shape[1]
    else:
        A, nc = head.shape[0], head.shape[1] - 5
    yp = PP.YoloPost(layout, A, nc, box_score, iou, lb, nms_mode, cap, max_batch=batch_copies, input_hw=input_hw)
    try:
        res = yp.run_host(np.stack([head] * batch_copies))
    finally:
        yp.close()
    return res if batch_copies > 1 else res[0]


def scan_views(yp):
    """Device addresses of a YoloPost's per-anchor scan results: best_conf float32 [max_batch][A], best_cls int32 [max_batch][A]."""
    conf, cls = C.c_void_p(), C.c_void_p()
    L.check(L.lib().adas_yolo_post_scan_views(yp.h, C.byref(conf), C.byref(cls)))
    return conf.value, cls.value


def yolo_scan(heads, layout, lb, box_score, iou, nms_mode=0, cap=1024):
    """heads [frames, ...]: one launch over all frames -> (best_conf [frames, A] float32, best_cls [frames, A] int32 as the scan kernel
    left them for EVERY anchor, the per-frame results of fetch())."""
    heads = np.ascontiguousarray(heads, np.float32)
    F = heads.shape[0]
    if layout == 0:
        nc, A = heads.shape[1] - 4, heads.shape[2]
    else:
        A, nc = heads.shape[1], heads.shape[2] - 5
    yp = PP.YoloPost(layout, A, nc, box_score, iou, lb, nms_mode, cap, max_batch=F)
    try:
        res = yp.run_host(heads)                                   # fetch() waits for the launch
        d_conf, d_cls = scan_views(yp)
        conf, cls = np.empty((F, A), np.float32), np.empty((F, A), np.int32)
        L.check(L.lib().adas_memcpy_d2h(L.ptr(conf), d_conf, conf.nbytes))
        L.check(L.lib().adas_memcpy_d2h(L.ptr(cls), d_cls, cls.nbytes))
    finally:
        yp.close()
    return conf, cls, res


def ufld(outs, cfg, W, H, lw=1):
    lr, lc = outs[0], outs[1]
    ud = PP.UfldDecode(lr.shape[1], lr.shape[2], lc.shape[1], lc.shape[2], W, H, cfg.row_anchor, cfg.col_anchor, lw, num_lanes=lr.shape[3])
    try:
        return ud.run_host(outs)[0]
    finally:
        ud.close()


def ufld1(head, cfg, input_wh, src_wh):
    ud = PP.Ufld1Decode(cfg.griding_num, cfg.cls_num_per_lane, cfg.img_w, cfg.img_h, input_wh[0], input_wh[1], src_wh[0], src_wh[1],
                        cfg.row_anchor)
    try:
        return ud.run_host(np.asarray(head, np.float32).reshape(1, cfg.griding_num + 1, cfg.cls_num_per_lane, 4))[0]
    finally:
        ud.close()


def lane_fetch(lg, frame=0):
    """LaneGeometry.fetch(frame) plus raw = (curvature, offset) as the kernel left them: fetch() hides both when there is no estimate."""
    out = lg.fetch(frame)
    res = L.LaneGeometryResult()
    L.check(L.lib().adas_lane_geometry_fetch(lg.h, frame, C.byref(res), None, None))
    out["raw"] = (float(res.curvature), float(res.offset))
    return out


def track_snapshot(hdr, tracked, lost):
    def rec(r):
        return dict(track_id=int(r["track_id"]), state=int(r["state"]), is_activated=bool(r["is_activated"]),
                    score=float(r["score"]), class_id=int(r["class_id"]), start_frame=int(r["start_frame"]),
                    frame_id=int(r["frame_id"]), tracklet_len=int(r["tracklet_len"]),
                    tlwh=[float(v) for v in r["tlwh"]])
    return dict(frame_id=int(hdr.frame_id), count=int(hdr.id_count), tracked=[rec(r) for r in tracked],
                lost=[rec(r) for r in lost])


ERR_CAPACITY = -5      # ADAS_ERR_CAPACITY: what a fetch returns, after filling its outputs, once BtHeader.err is set


def track_fetch(trk, stream, frame=None):
    """(snapshot, err) of a stream, or of frame `frame` of the last update_device_frames launch.  Unlike DeviceTracker.fetch this
    reads a stream whose err bits are set: the C call fills header and tracks and then returns the capacity error."""
    hdr = L.TrackHeader()
    recs = np.zeros(2 * trk.max_tracks, L.TRACK_DTYPE)
    if frame is None:
        rc = L.lib().adas_bytetrack_fetch(trk.h, stream, C.byref(hdr), L.ptr(recs), len(recs))
    else:
        rc = L.lib().adas_bytetrack_fetch_frame(trk.h, stream, frame, C.byref(hdr), L.ptr(recs), len(recs))
    if rc not in (0, ERR_CAPACITY):
        L.check(rc)
    assert (rc == ERR_CAPACITY) == (hdr.err != 0), (rc, hdr.err)
    nt, nl = hdr.n_tracked, hdr.n_lost
    return track_snapshot(hdr, recs[:nt], recs[nt:nt + nl]), int(hdr.err)


def upload_det_slabs(frames, det_stride, count_stride=1, count_index=0, counts=None):
    """Per-slab detection frames dict(boxes, scores, ids) in the layout adas_bytetrack_update_device[_frames] reads: slab q holds its
    rows at xyxy[q][det_stride][4] / score[q][det_stride] / cls[q][det_stride] and its count at counts[q * count_stride + count_index].
    Rows past a slab's count hold a decoy (a large box of score 0.99) and the other count words -1, so a kernel that read either
    would show it.  Returns (views for DeviceTracker.update_device*, the buffers to free)."""
    n = len(frames)
    xyxy = np.tile(np.asarray([10.0, 10.0, 900.0, 700.0]), (n, det_stride, 1))
    score = np.full((n, det_stride), 0.99)
    cls = np.full((n, det_stride), 77, np.int32)
    cnt = np.full(n * count_stride, -1, np.int32)
    for q, fr in enumerate(frames):
        k = len(fr["scores"])
        assert k <= det_stride
        if k:
            xyxy[q, :k] = np.asarray(fr["boxes"], np.float64).reshape(-1, 4)
            score[q, :k] = np.asarray(fr["scores"], np.float64)
            cls[q, :k] = np.asarray(fr["ids"], np.int32)
        cnt[q * count_stride + count_index] = k if counts is None else counts[q]
    bufs = [L.DeviceBuffer.from_array(a) for a in (xyxy, score, cls, cnt)]
    return dict(xyxy=bufs[0].ptr, score=bufs[1].ptr, cls=bufs[2].ptr, counts=bufs[3].ptr), bufs
