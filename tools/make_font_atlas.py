#!/usr/bin/env python3
"""Write a glyph atlas (.npz) for the overlay's text (LaneOverlay.set_fonts, AdasPipeline(overlay=dict(fonts=...))): the arrays of
adas_overlay_font -- atlas (cell_h, atlas_w) uint8 coverage, glyph_x / glyph_w / bearing_x / advance (95,) for characters 32..126 (advance
in 16.16), baseline_row, size_h, size_w_extra (16.16), scale.  The repository ships no font: the atlas is the caller's data.

    python tools/make_font_atlas.py --ttf /path/to/font.ttf --px 20 --scale 0.7 out.npz          # PIL: coverage of the anti-aliased glyph
    python tools/make_font_atlas.py --cv2 --face 0 --scale 0.7 --thickness 2 out.npz              # one cv2.putText per glyph

The --cv2 branch needs `import cv2` and renders each character alone with cv2.putText at the face, scale and thickness the reference
passes (e.g. face 0, tl / 3, tf for the label's size slot; FONT_HERSHEY_TRIPLEX, thickness 1 for the distance), takes the advance from
cv2.getTextSize of the character doubled minus once, and size_h / size_w_extra from getTextSize.  cv2 is not installed on the machines this
project is developed and tested on, so that branch ships UNEXERCISED; the PIL branch is what tests/test_font_atlas_tool.py runs.
"""
import argparse
import sys

import numpy as np

CHARS = [chr(c) for c in range(32, 127)]


def pack(cells, bearings, advances, baseline_row, size_h, size_w_extra, scale):
    """cells: 95 (cell_h, w) uint8 arrays (w may be 0) -> the atlas dict."""
    cell_h = max(c.shape[0] for c in cells)
    gw = np.array([c.shape[1] for c in cells], np.int32)
    if cell_h > 64 or gw.max() > 64:
        raise SystemExit("a glyph cell of %d rows x %d columns: the overlay takes at most 64 x 64 (render smaller)" % (cell_h, gw.max()))
    gx = np.zeros(95, np.int32)
    x = 1
    for g in range(95):
        gx[g] = x
        x += gw[g] + 1
    atlas = np.zeros((cell_h, x), np.uint8)
    for g, c in enumerate(cells):
        atlas[:c.shape[0], gx[g]:gx[g] + gw[g]] = c
    return dict(atlas=atlas, glyph_x=gx, glyph_w=gw, bearing_x=np.asarray(bearings, np.int32), advance=np.asarray(advances, np.int32),
                baseline_row=np.int32(baseline_row), size_h=np.int32(size_h), size_w_extra=np.int32(size_w_extra), scale=np.float64(scale))


def _trim(cov):
    """Drop empty columns on both sides -> (cells, first column)."""
    cols = np.flatnonzero(cov.any(axis=0))
    if not len(cols):
        return cov[:, :0], 0
    return cov[:, cols[0]:cols[-1] + 1], int(cols[0])


def from_ttf(path, px, scale):
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.truetype(path, px)
    ascent, descent = font.getmetrics()
    cell_h, pad = ascent + descent, px
    cells, bearings, advances = [], [], []
    for ch in CHARS:
        img = Image.new("L", (3 * px + 2 * pad, cell_h), 0)
        ImageDraw.Draw(img).text((pad, 0), ch, fill=255, font=font)
        cov, x0 = _trim(np.asarray(img, np.uint8))
        cells.append(cov)
        bearings.append(x0 - pad if cov.shape[1] else 0)
        advances.append(int(round(font.getlength(ch) * 65536)))
    return pack(cells, bearings, advances, baseline_row=ascent, size_h=ascent, size_w_extra=0, scale=scale)


def from_cv2(face, scale, thickness):   # UNEXERCISED here: cv2 is not on the project's machines
    import cv2
    (_, h), base = cv2.getTextSize("Ag", face, scale, thickness)
    pad = 2 * thickness + 4
    cell_h = h + base + 2 * pad
    cells, bearings, advances = [], [], []
    for ch in CHARS:
        (w1, _), _ = cv2.getTextSize(ch, face, scale, thickness)
        (w2, _), _ = cv2.getTextSize(ch + ch, face, scale, thickness)
        img = np.zeros((cell_h, w1 + 2 * pad + 4), np.uint8)
        cv2.putText(img, ch, (pad, pad + h), face, scale, 255, thickness)
        cov, x0 = _trim(img)
        cells.append(cov)
        bearings.append(x0 - pad if cov.shape[1] else 0)
        advances.append((w2 - w1) << 16)
    (wa, _), _ = cv2.getTextSize("A", face, scale, thickness)
    (waa, _), _ = cv2.getTextSize("AA", face, scale, thickness)
    return pack(cells, bearings, advances, baseline_row=pad + h, size_h=h, size_w_extra=(2 * wa - waa) << 16, scale=scale)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out")
    ap.add_argument("--ttf")
    ap.add_argument("--px", type=int, default=20, help="TTF pixel size")
    ap.add_argument("--cv2", action="store_true")
    ap.add_argument("--face", type=int, default=0)
    ap.add_argument("--thickness", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0,
                    help="the fontScale this atlas stands for (ladders pick by it).  The bird view's readouts ('Offset: ...', 'R : ...') are "
                         "fontScale 3, thickness 5, drawn at an integer zoom: render their atlas at 3 / zoom -- --scale 1.5 for the default zoom 2 "
                         "(with --cv2: --face 0 --thickness 3 or so; a cell is at most 64 rows)")
    a = ap.parse_args(argv)
    if bool(a.ttf) == bool(a.cv2):
        ap.error("give --ttf FILE or --cv2")
    f = from_cv2(a.face, a.scale, a.thickness) if a.cv2 else from_ttf(a.ttf, a.px, a.scale)
    np.savez(a.out, **f)
    print("%s: %d x %d atlas, baseline row %d, size_h %d" % (a.out, f["atlas"].shape[1], f["atlas"].shape[0], f["baseline_row"], f["size_h"]))


if __name__ == "__main__":
    sys.exit(main())
