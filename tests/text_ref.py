"""NumPy / plain Python restatement of the overlay text's rules T1-T7 (csrc/overlay_text_core.h), written from the reference's lines and the
rules' wording, not from the C++: Python's own '%.2f', a loop per item, a loop per glyph, one pixel at a time.  The CPU suite compares the
host build of the core with it, the GPU suite the device.

A font is a dict: atlas (cell_h, atlas_w) uint8, glyph_x / glyph_w / bearing_x / advance (95,) ints for characters 32..126 (advance in
16.16), baseline_row, size_h, size_w_extra (16.16), scale.  A scene is a dict of one frame's sources (see layout)."""
import numpy as np

DETECTIONS, TRACKS, TRACK_IDS, DISTANCE, PANELS, LINES = 1, 2, 4, 8, 16, 32
RANGE, OVERFLOW = 1, 2
RECT, RUN = 1, 2
OFFSET = ("To Be Determined ...", "Please Keep Right", "Please Keep Left", "Good Lane Keeping")                      # ufldDetector/utils.py:10-14
CURVATURE = ("To Be Determined ...", "Keep Straight Ahead", "Gentle Left Curve Ahead", "Hard Left Curve Ahead",
             "Gentle Right Curve Ahead", "Hard Right Curve Ahead")                                                     # :16-22
COLLISION = ("Determined ...", "Normal Risk", "Prompt Risk", "Warning Risk")                                          # ObjectDetector/utils.py:8-12
YELLOW, RED, GREEN, ORANGE = (0, 255, 255), (0, 0, 255), (0, 255, 0), (0, 102, 255)
LIMIT = 2 ** 30


def default_style():
    return dict(show_ratio=0.25, min_box_area=10.0, max_text_items=256, det_size_slot=0, det_label_slot=1, det_label_dx=2, det_label_dy=-7,
                det_box_pad=3, track_slot=2, track_dy=-10, id_first=3, id_count=1, id_shadow_first=4, id_shadow_count=1, dist_size_first=5,
                dist_size_count=1, dist_first=6, dist_count=1, dist_shadow_first=7, dist_shadow_count=1, shadow_dx=2, shadow_dy=2, ldws_slot=8,
                lkas_slot=8, fcws_slot=9, ldws_x=10, ldws_y=240, lkas_x=10, lkas_y=280, fcws_dx=100, fcws_y=240, id_shadow_sub=30,
                label_color=(255, 255, 255), dist_color=(255, 255, 255), dist_shadow_color=(150, 150, 150),
                offset_colors=(YELLOW, RED, RED, GREEN), curvature_colors=(YELLOW, GREEN, ORANGE, RED, ORANGE, RED),
                collision_colors=(YELLOW, GREEN, ORANGE, RED))


def glyph(ch):
    o = ch if isinstance(ch, int) else ord(ch)
    return (o if 32 <= o <= 126 else ord("?")) - 32


def text_size(font, s):
    """T2 -> (w, h)"""
    total = sum(int(font["advance"][glyph(c)]) for c in s.encode("latin-1"))
    return (total + int(font["size_w_extra"]) + 0x8000) >> 16, int(font["size_h"])


def ladder(fonts, first, count, v):
    best = first
    for k in range(first + 1, first + count):
        dk, db = abs(fonts[k]["scale"] - v), abs(fonts[best]["scale"] - v)
        if dk < db or (dk == db and fonts[k]["scale"] < fonts[best]["scale"]):
            best = k
    return best


def run_box(font, s, x, y, W, H):
    pen, lo, hi = x << 16, None, None
    for c in s.encode("latin-1"):
        g = glyph(c)
        gx0, gw = (pen >> 16) + int(font["bearing_x"][g]), int(font["glyph_w"][g])
        if gw > 0:
            lo = gx0 if lo is None else min(lo, gx0)
            hi = gx0 + gw if hi is None else max(hi, gx0 + gw)
        pen += int(font["advance"][g])
    if lo is None:
        return (0, 0, 0, 0)
    return clip(lo, y - font["baseline_row"], hi, y - font["baseline_row"] + font["atlas"].shape[0], W, H)


def clip(x0, y0, x1, y1, W, H):
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
    return (0, 0, 0, 0) if x0 >= x1 or y0 >= y1 else (x0, y0, x1, y1)


def _run(fonts, source, slot, x, y, color, s, W, H):
    s = s[:47]
    return dict(kind=RUN, source=source, x=x, y=y, x1=0, y1=0, box=run_box(fonts[slot], s, x, y, W, H), slot=slot, color=tuple(int(c) for c in color), text=s)


def _rect(source, c1, c2, color, W, H):
    box = clip(min(c1[0], c2[0]), min(c1[1], c2[1]), max(c1[0], c2[0]) + 1, max(c1[1], c2[1]) + 1, W, H)
    return dict(kind=RECT, source=source, x=c1[0], y=c1[1], x1=c2[0], y1=c2[1], box=box, slot=-1, color=tuple(int(c) for c in color), text="")


def _name(names, cls):
    return names[cls] if names is not None and 0 <= cls < len(names) else "unknown"


def _colour(colors, cls):
    return tuple(colors[cls]) if colors is not None and 0 <= cls < len(colors) else (0, 0, 0)


def _ok(v):
    return abs(v) < LIMIT   # False for nan


def layout(scene, fonts, W, H, mask, style=None):
    """One frame's items in paint order -> (items, flags).  scene keys (all optional): det_xyxy (n, 4) ints, det_cls; trk_tlwh (n, 4)
    floats, trk_cls, trk_ids, trk_last (n, 4) floats, traj_len; dist_points (n, 2) ints, dist_d; offset, curvature, collision;
    det_names, trk_names, det_colors, trk_colors; lines: [(x, y, slot, colour, text)]."""
    st = dict(default_style(), **(style or {}))
    items, flags = [], 0
    if mask & DETECTIONS:      # yoloDetector.py:180-191
        for (xmin, ymin, _, _), cls in zip(scene["det_xyxy"], scene["det_cls"]):
            xmin, ymin, cls = int(xmin), int(ymin), int(cls)
            if not (_ok(xmin) and _ok(ymin)):
                flags |= RANGE
                continue
            label = _name(scene.get("det_names"), cls)
            tw, th = text_size(fonts[st["det_size_slot"]], label)
            known = scene.get("det_names") is not None and 0 <= cls < len(scene["det_names"])     # an id outside the table is 'unknown', black
            colour = _colour(scene.get("det_colors"), cls) if known else (0, 0, 0)
            items.append(_rect(DETECTIONS, (xmin, ymin), (xmin + tw, ymin - th - st["det_box_pad"]), colour, W, H))
            items.append(_run(fonts, DETECTIONS, st["det_label_slot"], xmin + st["det_label_dx"], ymin + st["det_label_dy"], st["label_color"], label, W, H))
    for kind in (TRACKS, TRACK_IDS):
        if not mask & kind:
            continue
        for i, tlwh in enumerate(scene["trk_tlwh"]):
            if not float(tlwh[2]) * float(tlwh[3]) > st["min_box_area"]:       # byteTracker.py:210
                continue
            cls, tid = int(scene["trk_cls"][i]), int(scene["trk_ids"][i])
            colour = _colour(scene.get("trk_colors"), cls)
            if kind == TRACKS:  # core.py:235-239
                if not (_ok(tlwh[0]) and _ok(tlwh[1])):
                    flags |= RANGE
                    continue
                items.append(_run(fonts, TRACKS, st["track_slot"], int(tlwh[0]), int(tlwh[1]) + st["track_dy"], colour,
                                  "%s : %d" % (_name(scene.get("trk_names"), cls), tid), W, H))
                continue
            if int(scene["traj_len"][i]) <= 1:                                   # core.py:188
                continue
            box = [float(v) for v in scene["trk_last"][i]]
            v = (box[2] + box[3]) * 6e-4
            fs = v if v < 1 else 1                                               # min(1, v)
            ox, oy = box[0] + 10 * fs, box[1] + 30 * fs
            if not (_ok(ox) and _ok(oy)):
                flags |= RANGE
                continue
            x, y, s = int(ox), int(oy), "ID: %d" % tid
            shadow = tuple(max(0, min(255, c - st["id_shadow_sub"])) for c in colour)
            items.append(_run(fonts, TRACK_IDS, ladder(fonts, st["id_shadow_first"], st["id_shadow_count"], fs), x + st["shadow_dx"], y + st["shadow_dy"],
                              shadow, s, W, H))
            items.append(_run(fonts, TRACK_IDS, ladder(fonts, st["id_first"], st["id_count"], fs), x, y, colour, s, W, H))
    if mask & DISTANCE:        # distanceMeasure.py:97-115
        for (x, y), d in zip(scene["dist_points"], scene["dist_d"]):
            x, y, d = int(x), int(y), float(d)
            if (not d < 0 and d == d and abs(d) >= LIMIT) or not (_ok(x) and _ok(y)):     # a negative d prints no number
                flags |= RANGE
                continue
            text = " unknown m" if d < 0 else " %.2f m" % d
            fs = 1.0 if (d == 0 or d != d) else max(0.4, min(1, 1 / d))
            tw, th = text_size(fonts[ladder(fonts, st["dist_size_first"], st["dist_size_count"], fs)], text)
            tx, ty = int(x - tw / 2) + 1, int(y + th) + 5
            items.append(_run(fonts, DISTANCE, ladder(fonts, st["dist_shadow_first"], st["dist_shadow_count"], fs), tx + st["shadow_dx"], ty + st["shadow_dy"],
                              st["dist_shadow_color"], text, W, H))
            items.append(_run(fonts, DISTANCE, ladder(fonts, st["dist_first"], st["dist_count"], fs), tx, ty, st["dist_color"], text, W, H))
    if mask & PANELS:          # demo.py:173-174, 212
        o, c, k = (int(scene[n]) for n in ("offset", "curvature", "collision"))
        o, c, k = (o if 0 <= o < 4 else 0), (c if 0 <= c < 6 else 0), (k if 0 <= k < 4 else 0)
        items.append(_run(fonts, PANELS, st["ldws_slot"], st["ldws_x"], st["ldws_y"], st["offset_colors"][o], "LDWS : " + OFFSET[o], W, H))
        items.append(_run(fonts, PANELS, st["lkas_slot"], st["lkas_x"], st["lkas_y"], st["curvature_colors"][c], "LKAS : " + CURVATURE[c], W, H))
        items.append(_run(fonts, PANELS, st["fcws_slot"], W - int(W * st["show_ratio"]) + st["fcws_dx"], st["fcws_y"], st["collision_colors"][k],
                          "FCWS : " + COLLISION[k], W, H))
    if mask & LINES:
        for x, y, slot, colour, text in scene.get("lines", ()):
            items.append(_run(fonts, LINES, slot, x, y, colour, text, W, H))
    if len(items) > st["max_text_items"]:      # T6
        flags |= OVERFLOW
        items = items[:st["max_text_items"]]
    return items, flags


def paint(img, items, fonts):
    """T7 in place on img (H, W, 3) uint8: the items one after another, a run's glyphs one after another."""
    H, W = img.shape[:2]
    for it in items:
        if it["kind"] == RECT:
            x0, y0, x1, y1 = it["box"]
            img[y0:y1, x0:x1] = it["color"]
            continue
        f = fonts[it["slot"]]
        pen, top = it["x"] << 16, it["y"] - f["baseline_row"]
        for c in it["text"].encode("latin-1"):
            g = glyph(c)
            gx0, gw, ax = (pen >> 16) + int(f["bearing_x"][g]), int(f["glyph_w"][g]), int(f["glyph_x"][g])
            pen += int(f["advance"][g])
            for r in range(f["atlas"].shape[0]):
                y = top + r
                if not 0 <= y < H:
                    continue
                for k in range(gw):
                    x, cov = gx0 + k, int(f["atlas"][r, ax + k])
                    if not 0 <= x < W or cov == 0:
                        continue
                    for ch in range(3):          # T4
                        img[y, x, ch] = (int(img[y, x, ch]) * (255 - cov) + it["color"][ch] * cov + 127) // 255
    return img
