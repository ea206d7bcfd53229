"""NumPy / plain Python restatement of the bird view's readouts, rules R0-R6 (csrc/overlay_readout_core.h), written from the reference's
lines (PerspectiveTransformation.calcCurveAndOffset, perspectiveTransformation.py:205-213) and the rules' wording, not from the C++: Python's
own '%.1f', the arrows as marks of tests/overlay_tracks_ref.py (D11 / D12 from their set definitions, brute force over pixels), the
strings glyph by glyph, glyph pixel by glyph pixel, real pixel by real pixel with text_ref's T2-T4.  It does not import the emulation.
Modelled on OpenCV 4.5; the definitions are the authority and parity with a real cv2 build is unpinned.  Test scaffolding.

A font is text_ref's dict.  A record is dict(drawn, flags, arrows: [mark, mark] (overlay_tracks_ref's mark dicts, track 0 at veh_pos and
track 1 at the centre), strings: [dict(x, y, box, text, skipped)] * 2: the offset, the radius)."""
import numpy as np

import overlay_ref as ref
import overlay_tracks_ref as tref
import text_ref as R

READOUTS = 256
RANGE = 1
DIR_NONE = 0
LIMIT = 2 ** 30


def default_style():
    return dict(slot=10, zoom=2, offset_x=20, offset_y=80, radius_x=20, radius_y=180, text_color=(0, 0, 255), arrow_a_color=(255, 255, 255),
                arrow_b_color=(150, 150, 150))


def synthetic_font(seed=12345, cell_h=9, baseline_row=6):
    """A 9-row font of random coverage with glyphs of every width 1 .. 9, side bearings of either sign and fractional advances (the
    generator of the text's bounds program)."""
    g = np.arange(95)
    gw = np.where(g > 0, 1 + (g * 7) % 9, 0)
    gx = 1 + np.concatenate([[0], np.cumsum(gw + 1)[:-1]])
    aw = int(1 + np.sum(gw + 1))
    rng = np.random.default_rng(seed)
    atlas = rng.integers(0, 256, (cell_h, aw), dtype=np.uint8)
    atlas[rng.random((cell_h, aw)) < 0.3] = 0          # holes: a coverage of 0 writes nothing
    return dict(atlas=atlas, glyph_x=gx, glyph_w=gw, bearing_x=(g * 5) % 5 - 2, advance=((gw + 1) << 16) + (g * 4099) % 65536,
                baseline_row=baseline_row, size_h=cell_h - 2, size_w_extra=0x18000, scale=1.0)


def fmt1(v):
    """T1's '%.1f': Python's own, or None: finite and |v| >= 2^30."""
    v = float(v)
    if v == v and abs(v) != float("inf") and abs(v) >= LIMIT:
        return None
    return "%.1f" % v


def _arrow(track, p1, p2, colour, t, tip):
    qa, qb = tref.arrow_tips(p1, p2, tip)
    return dict(kind=tref.ARROW, track=track, x1=p1[0], y1=p1[1], x2=p2[0], y2=p2[1], radius=0, thickness=t, color=tuple(int(c) for c in colour), tip=tip,
                tips=(qa[0], qa[1], qb[0], qb[1]))


def run_extent(font, s):
    """The columns [lo, hi) the run's glyphs cover at zoom 1 relative to its origin, or None."""
    pen, lo, hi = 0, None, None
    for c in s.encode("latin-1"):
        g = R.glyph(c)
        gx0, gw = (pen >> 16) + int(font["bearing_x"][g]), int(font["glyph_w"][g])
        if gw > 0:
            lo = gx0 if lo is None else min(lo, gx0)
            hi = gx0 + gw if hi is None else max(hi, gx0 + gw)
        pen += int(font["advance"][g])
    return None if lo is None else (lo, hi)


def layout(direction, veh_pos, curvature, offset, Wb, Hb, font, style=None):
    """R0-R3 and the boxes of R4 for one frame -> record."""
    st = dict(default_style(), **(style or {}))
    if int(direction) == DIR_NONE:                                              # R0
        return dict(drawn=False, flags=0, arrows=[], strings=[])
    flags = 0
    xa = tref.trunc(veh_pos)
    arrows = [_arrow(0, (xa, Hb - 1), (xa, tref.trunc(float(Wb) / 3)), st["arrow_a_color"], 5, 0.2),             # R1: img.shape[1] / 3
              _arrow(1, (tref.trunc(Wb / 2.), Hb - 1), (tref.trunc(Wb / 2.), tref.trunc(float(Hb) / 1.3)), st["arrow_b_color"], 10, 0.5)]   # R2
    for mk in arrows:
        if not all(tref.in_range(*s) for s in tref.mark_segments(mk)):
            flags |= RANGE
    z, strings = int(st["zoom"]), []
    for head, v, (x, y) in (("Offset: ", offset, (st["offset_x"], st["offset_y"])), ("R : ", curvature, (st["radius_x"], st["radius_y"]))):   # R3
        num = fmt1(v)
        if num is None:
            flags |= RANGE
            strings.append(dict(x=x, y=y, box=(0, 0, 0, 0), text="", skipped=True))
            continue
        text = head + num + " m"
        ext = run_extent(font, text)
        top = -int(font["baseline_row"])
        box = (0, 0, 0, 0) if ext is None else R.clip(x + z * ext[0], y + z * top, x + z * ext[1], y + z * (top + font["atlas"].shape[0]), Wb, Hb)
        strings.append(dict(x=x, y=y, box=box, text=text, skipped=False))
    return dict(drawn=True, flags=flags, arrows=arrows, strings=strings)


def paint_string(img, s, font, colour, zoom):
    """R4 in place: glyph pixel (u, v) of the zoom-1 run covers the zoom x zoom real pixels at (x + z u, y + z v), blended per T4."""
    H, W = img.shape[:2]
    pen, z = 0, int(zoom)
    for c in s["text"].encode("latin-1"):
        g = R.glyph(c)
        gx0, gw, ax = (pen >> 16) + int(font["bearing_x"][g]), int(font["glyph_w"][g]), int(font["glyph_x"][g])
        pen += int(font["advance"][g])
        for r in range(font["atlas"].shape[0]):
            v = r - int(font["baseline_row"])
            for k in range(gw):
                cov = int(font["atlas"][r, ax + k])
                if cov == 0:
                    continue
                u = gx0 + k
                for j in range(z):
                    for i in range(z):
                        px, py = s["x"] + z * u + i, s["y"] + z * v + j
                        if 0 <= px < W and 0 <= py < H:
                            for ch in range(3):
                                img[py, px, ch] = (int(img[py, px, ch]) * (255 - cov) + int(colour[ch]) * cov + 127) // 255
    return img


def paint(img, rec, font, style=None):
    """R5 in place on img (Hb, Wb, 3) uint8: arrow A, arrow B, string 1, string 2, one after another."""
    st = dict(default_style(), **(style or {}))
    if not rec["drawn"]:
        return img
    H, W = img.shape[:2]
    for mk in rec["arrows"]:
        m, _ = tref.mark_mask(mk, H, W)
        img[m] = mk["color"]
    for s in rec["strings"]:
        if not s["skipped"]:
            paint_string(img, s, font, st["text_color"], st["zoom"])
    return img


def draw(bird, direction, veh_pos, curvature, offset, font, style=None, lanes=None, radius=10, offset_type=ref.OFFSET_UNKNOWN):
    """One bird image (a copy) through the readouts and, with lanes (4 lists of bird-view points), DrawDetectedOnBirdView's discs on top.
    -> (image, record)"""
    out = np.ascontiguousarray(bird, np.uint8).copy()
    rec = layout(direction, veh_pos, curvature, offset, out.shape[1], out.shape[0], font, style)
    paint(out, rec, font, style)
    if lanes is not None:
        out = ref.draw_lanes(out, lanes, offset_type, radius=radius, direct=True)
    return out, rec


def record_table(rec):
    """A record as comparable values."""
    return (bool(rec["drawn"]), int(rec["flags"]), tref.marks_table(rec["arrows"]),
            [(s["x"], s["y"], tuple(s["box"]), s["text"], bool(s["skipped"])) for s in rec["strings"]])


def device_record_table(rec):
    """The same from LaneOverlay.readout_record() / the emulation's public record."""
    if not rec["drawn"]:
        return (False, int(rec["flags"]), [], [])
    return (True, int(rec["flags"]), tref.device_marks_table(rec["arrows"]),
            [(s["x"], s["y"], tuple(s["box"]), s["text"], bool(s["skipped"])) for s in rec["strings"]])
