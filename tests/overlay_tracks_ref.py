"""NumPy restatement of the overlay's trajectories stage (csrc/overlay_track_core.h): the per-track arithmetic of
BYTETracker.DrawTrackedOnFrame's show_traject part (plot_trajectories' circles, plot_directions' lock-on rectangle or shadowed arrow) in
the reference's own expressions, and the pixel rules D10-D12 and the fold written from their SET definitions by brute force over pixels
-- a circle is the union of discs on the midpoint walk's outline, a segment's body the pixels with 0 <= v.d <= d.d and
cross^2 <= R^2 d.d (the squared form, in exact integers: no Tq, no row intervals), the fold a loop of whole-image writes in the
reference's call order.  Modelled on OpenCV 4.5; the definitions are the authority and parity with a real cv2 build is unpinned.
Text is not drawn.  Test scaffolding."""
import numpy as np

import overlay_ref as ref
import overlay_objects_ref as oref

TRAJECTORIES = 128
TRACK_RANGE = 2
RING = 30
CIRCLE, RECT, ARROW = 1, 2, 3
SQRT_HALF = 0.70710678118654752440


def trunc(v):
    """int() for what an image can hold: toward zero, saturated to int32, NaN -> 0 (overlay_trunc_i32)."""
    v = float(v)
    if v != v:
        return 0
    if v >= 2147483647.0:
        return 2147483647
    if v <= -2147483648.0:
        return -2147483648
    return int(v)


def mark_table():
    """(radius, thickness) of circle i, plot_trajectories' own expressions."""
    return [(int(np.sqrt(float(i + 1)) * 0.5), int(np.sqrt(float(i + 1)) * 1.2)) for i in range(RING)]


def seg_radius(t):
    return (t + 1) >> 1 if t >= 2 else 0


# ------------------------------------------------------------------------------------------------------------- the per-track arithmetic
def compute_directions(boxes, limit_shift=2):
    out = []
    for i in range(len(boxes) - 1):
        cur, nxt = np.asarray(boxes[i], np.float64), np.asarray(boxes[i + 1], np.float64)
        shift = abs(min(nxt - cur))
        cc = np.array([(cur[0] + cur[2]) / 2, (cur[1] + cur[3]) / 2])
        nc = np.array([(nxt[0] + nxt[2]) / 2, (nxt[1] + nxt[3]) / 2])
        out.append(nc - cc if shift >= limit_shift else np.array([0.0, 0.0]))
    return out


def arrow_tips(p1, p2, tip):
    """D12: qa, qb."""
    k = np.float64(tip) * np.float64(SQRT_HALF)
    ux, uy = int(p1[0]) - int(p2[0]), int(p1[1]) - int(p2[1])
    qa = (trunc(np.rint(np.float64(p2[0]) + k * np.float64(ux - uy))), trunc(np.rint(np.float64(p2[1]) + k * np.float64(ux + uy))))
    qb = (trunc(np.rint(np.float64(p2[0]) + k * np.float64(ux + uy))), trunc(np.rint(np.float64(p2[1]) + k * np.float64(uy - ux))))
    return qa, qb


def track_marks(tlwh, trajectory, colour, H, W, min_box_area=oref.MIN_BOX_AREA, activated=True, track=0):
    """One track's marks in drawing order: dicts with kind, track, x1, y1, x2, y2, radius, thickness, color, tip (the tip length of an
    arrow), tips (its two tip points)."""
    tlwh = np.asarray(tlwh, np.float64)
    if not activated or not tlwh[2] * tlwh[3] > min_box_area:
        return []
    T = [np.asarray(b, np.float64) for b in trajectory][-RING:]
    colour = tuple(int(c) for c in colour)
    marks = []
    tab = mark_table()
    if len(T) > 1:
        for i, box in enumerate(T):
            marks.append(dict(kind=CIRCLE, track=track, x1=trunc((box[0] + box[2]) / 2), y1=trunc(box[3]), x2=trunc((box[0] + box[2]) / 2),
                              y2=trunc(box[3]), radius=tab[i][0], thickness=tab[i][1], color=colour, tip=0.0, tips=(0, 0, 0, 0)))
    O = [b for b in T if b[0] >= 10 and b[1] >= 10 and b[2] <= W - 10 and b[3] <= H - 10]
    dirs = compute_directions(O)
    if len(O) > 1:
        cx, cy = tlwh[0] + tlwh[2] / 2, tlwh[1] + tlwh[3] / 2
        rate, h = tlwh[2] / tlwh[3], tlwh[3]
        w = h * rate
        n = len(dirs)
        if n < 5:
            rate_w = (cx - (cx - w // 2)) / 5
            rate_h = (cy - (cy - h // 2)) / 5
            sx, sy = trunc(cx - w // 2 + rate_w * n), trunc(cy - h // 2 + rate_h * n)
            ex, ey = trunc(cx + w // 2 - rate_w * n), trunc(cy + h // 2 - rate_h * n)
            marks.append(dict(kind=RECT, track=track, x1=sx, y1=sy, x2=ex, y2=ey, radius=0, thickness=2, color=tuple(max(0, c - 10) for c in colour),
                              tip=0.0, tips=(0, 0, 0, 0)))
        else:
            L = 1000 * min((h * w) / (H * W), 0.02)
            md = np.median(np.asarray(dirs, np.float64), axis=0)
            start = (trunc(cx), trunc(cy))
            end = (trunc(cx + md[0] * L), trunc(cy + md[1] * L))
            for p1, p2, col, t, tip in (((start[0] - 2, start[1] + 2), (end[0] - 2, end[1] + 2), (100, 100, 100), 5, 0.3),
                                        (start, (end[0] - 1, end[1] - 1), (255, 255, 255), 2, 0.3 - 0.1),
                                        (start, end, (255, 255, 255), 3, 0.3)):
                qa, qb = arrow_tips(p1, p2, tip)
                marks.append(dict(kind=ARROW, track=track, x1=p1[0], y1=p1[1], x2=p2[0], y2=p2[1], radius=0, thickness=t, color=col, tip=tip,
                                  tips=(qa[0], qa[1], qb[0], qb[1])))
    return marks


# ------------------------------------------------------------------------------------------------------------- D10
def circle_outline(r):
    """The offsets the midpoint walk visits, with their eight reflections."""
    pts = set()
    dx, dy, err, plus, minus = r, 0, 0, 1, 2 * r - 1
    while dx >= dy:
        for a, b in ((dx, dy), (dy, dx)):
            for sa in (1, -1):
                for sb in (1, -1):
                    pts.add((sa * a, sb * b))
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return sorted(pts)


def circle_mask(cx, cy, r, t, H, W):
    m = np.zeros((H, W), bool)
    R = seg_radius(t)
    for ox, oy in circle_outline(r):
        m |= ref.disc_mask(cx + ox, cy + oy, R, H, W)      # R = 0: the pixel itself
    return m


# ------------------------------------------------------------------------------------------------------------- D11
def in_range(*v):
    return all(abs(int(c)) <= ref.COORD_MAX for c in v)


def segment_mask(ax, ay, bx, by, t, H, W):
    ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
    if t == 1:
        return ref.line_mask(ax, ay, bx, by, H, W)
    R = seg_radius(t)
    m = ref.disc_mask(ax, ay, R, H, W) | ref.disc_mask(bx, by, R, H, W)
    dx, dy = bx - ax, by - ay
    dd = dx * dx + dy * dy
    if dd == 0:
        return m
    x0, x1 = max(min(ax, bx) - R - 1, 0), min(max(ax, bx) + R + 1, W - 1)
    y0, y1 = max(min(ay, by) - R - 1, 0), min(max(ay, by) + R + 1, H - 1)
    if x0 > x1 or y0 > y1:
        return m
    big = max(abs(dx), abs(dy), abs(ax) + W, abs(ay) + H) >= (1 << 14)      # exact integers either way: objects when int64 could overflow
    dt = object if big else np.int64
    vy, vx = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64).astype(dt) - ay, np.arange(x0, x1 + 1, dtype=np.int64).astype(dt) - ax, indexing="ij")
    dot = vx * dx + vy * dy
    cr = vx * dy - vy * dx
    body = (dot >= 0) & (dot <= dd) & (cr * cr <= R * R * dd)
    m[y0:y1 + 1, x0:x1 + 1] |= np.asarray(body, bool)
    return m


def mark_segments(mk):
    """The D11 segments of a rectangle (D7's edges) or an arrow (shaft, two tips), each (ax, ay, bx, by)."""
    x1, y1, x2, y2 = mk["x1"], mk["y1"], mk["x2"], mk["y2"]
    if mk["kind"] == RECT:
        return [(x1, y1, x2, y1), (x2, y1, x2, y2), (x2, y2, x1, y2), (x1, y2, x1, y1)]
    q = mk["tips"]
    return [(x1, y1, x2, y2), (q[0], q[1], x2, y2), (q[2], q[3], x2, y2)]


def mark_mask(mk, H, W):
    """(mask, range flag) of one mark."""
    if mk["kind"] == CIRCLE:
        return circle_mask(mk["x1"], mk["y1"], mk["radius"], mk["thickness"], H, W), 0
    m, flag = np.zeros((H, W), bool), 0
    for s in mark_segments(mk):
        if not in_range(*s):
            flag = TRACK_RANGE
            continue
        m |= segment_mask(*s, mk["thickness"], H, W)
    return m, flag


# ------------------------------------------------------------------------------------------------------------- the fold
def draw_tracks(img, tlwhs, classes, trajectories, table=None, min_box_area=oref.MIN_BOX_AREA, t=oref.TRACK_T, boxes=True, marks=True):
    """DrawTrackedOnFrame(frame, show_box=boxes, show_traject=marks) without its text, for rows of activated tracked tracks in list order.
    trajectories: per row its list of tlbr boxes, oldest first.  (image, flags, marks)."""
    H, W = img.shape[:2]
    out, flags, all_marks = img.copy(), 0, []
    for k, (tlwh, cls) in enumerate(zip(np.asarray(tlwhs, np.float64).reshape(-1, 4), classes)):
        if boxes:
            out = oref.draw_tracks(out, [tlwh], [cls], table, min_box_area, t)
        if marks:
            for mk in track_marks(tlwh, trajectories[k], oref.class_colour(cls, table), H, W, min_box_area, track=k):
                m, f = mark_mask(mk, H, W)
                out[m] = mk["color"]
                flags |= f
                all_marks.append(mk)
    return out, flags, all_marks


def compose(img, lanes=None, poly=None, area_status=False, dist=None, offset_type=ref.OFFSET_UNKNOWN, area_color=ref.AREA_COLOR, stages=7,
            dets=None, det_cls=None, det_table=None, trks=None, trk_cls=None, trk_table=None, trajectories=None, min_box_area=oref.MIN_BOX_AREA,
            thickness=(oref.RECT_T, oref.ARM_T, oref.TRACK_T), **kw):
    """One frame through the Draw block's order: lanes, area, detections, per track its box and its marks, distance discs.
    (frame_show, flags, marks)."""
    out, flags = ref.compose(img, lanes, poly, area_status, None, offset_type, area_color, stages & 3, **kw)
    marks = []
    if stages & oref.DETECTIONS and dets is not None:
        out = oref.draw_detections(out, dets, det_cls, det_table, thickness[1], thickness[0])
    if stages & (oref.TRACKS | TRAJECTORIES) and trks is not None:
        out, f, marks = draw_tracks(out, trks, trk_cls, trajectories if trajectories is not None else [[]] * len(trk_cls), trk_table, min_box_area,
                                    thickness[2], bool(stages & oref.TRACKS), bool(stages & TRAJECTORIES))
        flags |= f
    if stages & ref.DISTANCE and dist is not None:
        out = ref.draw_distance(out, dist, kw.get("radii", (3, 4))[1])
    return out, flags, marks


def marks_table(marks):
    """Marks as comparable tuples: (kind, track, x1, y1, x2, y2, radius, thickness, color, tips)."""
    return [(m["kind"], m["track"], m["x1"], m["y1"], m["x2"], m["y2"], m["radius"], m["thickness"], tuple(m["color"]), tuple(m["tips"])) for m in marks]


def device_marks_table(arr):
    """The same tuples from LaneOverlay.track_marks() / the emulation's structured array."""
    return [(int(m["kind"]), int(m["track"]), int(m["x1"]), int(m["y1"]), int(m["x2"]), int(m["y2"]), int(m["radius"]), int(m["thickness"]),
             tuple(int(c) for c in m["color"]), tuple(int(v) for v in m["tip"])) for m in arr]
