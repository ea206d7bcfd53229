"""NumPy restatement of the overlay's object layer, rules D6-D9 of csrc/overlay_core.h: the boxes of ObjectDetectBase.cornerRect and the
box part of ObjectTrackBase.plot_bbox.  Written from the STEPPING definitions -- a thick segment is walked as its body plus the two
midpoint-walk discs, pixel by pixel, thin edges by the error-term loop of the line, and the fold is a loop of whole-image operations in
the reference's call order -- not from the closed forms the device uses.  Modelled on OpenCV 4.5; the definitions are the authority and
parity with a real cv2 build is unpinned.  Text, the label background, key points, trajectories and arrows are not drawn.
Test scaffolding."""
import numpy as np

import overlay_ref as ref

DETECTIONS, TRACKS = 16, 32
RECT_T, ARM_T, TRACK_T = 1, 5, 2          # cornerRect's rt and t, plot_bbox's thickness
MIN_BOX_AREA = 10.0
UNKNOWN = (0, 0, 0)


# ------------------------------------------------------------------------------------------------------------- D6
def thick_segment_mask(ax, ay, bx, by, t, H, W):
    """Body (the segment's pixels along its axis by -R .. +R across it) plus a disc of radius R on each endpoint; t == 1: the D3 line."""
    ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
    assert ax == bx or ay == by
    if t == 1:
        return ref.line_mask(ax, ay, bx, by, H, W)
    R = (t + 1) >> 1
    m = np.zeros((H, W), bool)
    if (ax, ay) != (bx, by):              # a zero-length segment is its two coinciding discs
        for x in range(max(min(ax, bx) - (R if ax == bx else 0), 0), min(max(ax, bx) + (R if ax == bx else 0), W - 1) + 1):
            for y in range(max(min(ay, by) - (R if ay == by else 0), 0), min(max(ay, by) + (R if ay == by else 0), H - 1) + 1):
                m[y, x] = True
    return m | ref.disc_mask(ax, ay, R, H, W) | ref.disc_mask(bx, by, R, H, W)


# ------------------------------------------------------------------------------------------------------------- D7
def rect_mask(x1, y1, x2, y2, t, H, W):
    m = np.zeros((H, W), bool)
    for a, b in (((x1, y1), (x2, y1)), ((x2, y1), (x2, y2)), ((x2, y2), (x1, y2)), ((x1, y2), (x1, y1))):
        m |= thick_segment_mask(a[0], a[1], b[0], b[1], t, H, W)
    return m


def corner_rect_mask(xmin, ymin, xmax, ymax, H, W, t=ARM_T, rt=RECT_T):
    """ObjectDetectBase.cornerRect: the outline and the eight arms, in its order."""
    xmin, ymin, xmax, ymax = int(xmin), int(ymin), int(xmax), int(ymax)
    l = max(1, int(min(ymax - ymin, xmax - xmin) * 0.2))
    m = rect_mask(xmin, ymin, xmax, ymax, rt, H, W)
    for a, b in (((xmin, ymin), (xmin + l, ymin)), ((xmin, ymin), (xmin, ymin + l)), ((xmax, ymin), (xmax - l, ymin)), ((xmax, ymin), (xmax, ymin + l)),
                 ((xmin, ymax), (xmin + l, ymax)), ((xmin, ymax), (xmin, ymax - l)), ((xmax, ymax), (xmax - l, ymax)), ((xmax, ymax), (xmax, ymax - l))):
        m |= thick_segment_mask(a[0], a[1], b[0], b[1], t, H, W)
    return m


# ------------------------------------------------------------------------------------------------------------- D8
def tint(a, b):
    """addWeighted(a, 0.6, b, 0.4, 1.0) on u8: two fp32 products rounded separately, two fp32 adds in that order, ties to even, saturated."""
    pa = np.asarray(a).astype(np.float32) * np.float32(0.6)
    pb = np.asarray(b).astype(np.float32) * np.float32(0.4)
    s = (pa + pb).astype(np.float32)
    s = (s + np.float32(1.0)).astype(np.float32)
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- D9
def class_colour(cls, table):
    return tuple(int(c) for c in table[cls]) if table is not None and 0 <= int(cls) < len(table) else UNKNOWN


def draw_detections(img, boxes, classes, table=None, t=ARM_T, rt=RECT_T):
    """DrawDetectedOnFrame's boxes, in _object_info order: (xmin, ymin, xmax, ymax) ints, written."""
    H, W = img.shape[:2]
    out = img.copy()
    for box, cls in zip(np.asarray(boxes, np.int64).reshape(-1, 4), classes):
        out[corner_rect_mask(*box, H, W, t, rt)] = class_colour(cls, table)
    return out


def track_box(tlwh, H, W, min_box_area=MIN_BOX_AREA):
    """plot_bbox's corners, or None when the area gate fails."""
    tlwh = np.asarray(tlwh, np.float64)
    if not tlwh[2] * tlwh[3] > min_box_area:
        return None
    tx1, ty1, tw, th = (int(v) for v in tlwh.astype(np.int64))
    return max(0, tx1), max(0, ty1), min(W, tx1 + tw), min(H, ty1 + th)


def draw_tracks(img, tlwhs, classes, table=None, min_box_area=MIN_BOX_AREA, t=TRACK_T):
    """The box part of DrawTrackedOnFrame for activated tracked tracks, in list order: the outline written, then the region tinted."""
    H, W = img.shape[:2]
    out = img.copy()
    for tlwh, cls in zip(np.asarray(tlwhs, np.float64).reshape(-1, 4), classes):
        box = track_box(tlwh, H, W, min_box_area)
        if box is None:
            continue
        x1, y1, x2, y2 = box
        col = class_colour(cls, table)
        out[rect_mask(x1, y1, x2, y2, t, H, W)] = col
        if x2 > x1 and y2 > y1:           # the stated divergence: an empty region tints nothing
            out[y1:y2, x1:x2] = tint(out[y1:y2, x1:x2], np.array(col, np.uint8)[None, None, :])
    return out


def compose(img, lanes=None, poly=None, area_status=False, dist=None, offset_type=ref.OFFSET_UNKNOWN, area_color=ref.AREA_COLOR, stages=7,
            dets=None, det_cls=None, det_table=None, trks=None, trk_cls=None, trk_table=None, min_box_area=MIN_BOX_AREA,
            thickness=(RECT_T, ARM_T, TRACK_T), **kw):
    """One frame through the Draw block's order: lanes, area, detections, tracks, distance discs.  (frame_show, flags)."""
    out, flags = ref.compose(img, lanes, poly, area_status, None, offset_type, area_color, stages & 3, **kw)
    if stages & DETECTIONS and dets is not None:
        out = draw_detections(out, dets, det_cls, det_table, thickness[1], thickness[0])
    if stages & TRACKS and trks is not None:
        out = draw_tracks(out, trks, trk_cls, trk_table, min_box_area, thickness[2])
    if stages & ref.DISTANCE and dist is not None:
        out = ref.draw_distance(out, dist, kw.get("radii", (3, 4))[1])
    return out, flags
