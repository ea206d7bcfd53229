"""NumPy restatement of the demo's three UI panels (ControlPanel.DisplayBirdViewPanel / DisplaySignsPanel / DisplayCollisionPanel,
demo.py:101-214) without their putText lines: what csrc/overlay_panel_core.h (rules P1-P6) is checked against, painted the way the
reference paints -- one panel after the other, whole slices at a time -- and not the way the device folds it per byte.
The signs and collision panels and the bird panel's placement are pinned to the reference's own code by tests/golden/panels.json.gz; the
resize inside the bird panel is oracle.preprocess.cv_resize_linear_u8, the project's restatement of OpenCV's INTER_LINEAR: UNPINNED.
Types and latches are the integers of ADAS_OFFSET_* / ADAS_CURVATURE_* / ADAS_COLLISION_* / ADAS_PANEL_LATCH_*."""
import hashlib

import numpy as np

from oracle.preprocess import cv_resize_linear_u8

BIRD, SIGNS, COLLISION = 1, 2, 4
OFF_UNKNOWN, OFF_RIGHT, OFF_LEFT, OFF_CENTER = 0, 1, 2, 3
CUR_UNKNOWN, CUR_STRAIGHT, CUR_EASY_LEFT, CUR_HARD_LEFT, CUR_EASY_RIGHT, CUR_HARD_RIGHT = 0, 1, 2, 3, 4, 5
COL_UNKNOWN, COL_NORMAL, COL_PROMPT, COL_WARNING = 0, 1, 2, 3
LATCH_NONE, LATCH_LEFT, LATCH_RIGHT, LATCH_STRAIGHT = 0, 1, 2, 3
DEFAULTS = dict(show_ratio=0.25, border=10, signs_w=400, signs_h=365, signs_sprite_row=10, collision_sprite_row=50, collision_sprite_col=5,
                border_color=(0, 0, 255))


def sha(img):
    return hashlib.sha256(np.ascontiguousarray(img, np.uint8).tobytes()).hexdigest()


def choose_signs(latch, off, cur):
    """([sprite names in paint order, None where a chain paints nothing], latch after)."""
    off = off if 0 <= off < 4 else 0
    cur = cur if 0 <= cur < 6 else 0
    a = b = None
    if cur == CUR_UNKNOWN and off in (OFF_UNKNOWN, OFF_CENTER):
        a, latch = "warn", LATCH_NONE
    elif (cur == CUR_HARD_LEFT or latch == LATCH_LEFT) and cur not in (CUR_EASY_RIGHT, CUR_HARD_RIGHT):
        a, latch = "left", LATCH_LEFT
    elif (cur == CUR_HARD_RIGHT or latch == LATCH_RIGHT) and cur not in (CUR_EASY_LEFT, CUR_HARD_LEFT):
        a, latch = "right", LATCH_RIGHT
    if off == OFF_RIGHT:
        b = "lta_left"
    elif off == OFF_LEFT:
        b = "lta_right"
    elif cur == CUR_STRAIGHT or latch == LATCH_STRAIGHT:
        b, latch = "straight", LATCH_STRAIGHT
    return [a, b], latch


def choose_collision(col):
    return {COL_WARNING: "fcws_warning", COL_PROMPT: "fcws_prompt", COL_NORMAL: "fcws_normal"}.get(col)


def _widget(img, r0, r1, c0, c1, colour):
    w = np.copy(img[r0:r1, c0:c1])
    w //= 2
    w[0:3, :] = colour
    w[-3:-1, :] = colour
    w[:, 0:3] = colour
    w[:, -3:-1] = colour
    img[r0:r1, c0:c1] = w


def _sprite(img, spr, y0, x0, mask_channel):
    if spr is None:
        return
    y, x = spr[:, :, mask_channel].nonzero()
    img[y + y0, x + x0] = spr[y, x, :3]


def geometry(hw, p):
    W, H = int(hw[1] * p["show_ratio"]), int(hw[0] * p["show_ratio"])
    return W, H


def bird_panel(img, bird_img, **params):
    p = dict(DEFAULTS, **params)
    W, H = geometry(img.shape, p)
    b = p["border"]
    small = cv_resize_linear_u8(np.ascontiguousarray(bird_img), (W, H))
    panel = np.zeros((H + 2 * b, W + 2 * b, 3), np.uint8)
    panel[b:b + H, b:b + W] = small
    img[0:panel.shape[0], img.shape[1] - panel.shape[1]:] = panel


def signs_panel(img, sprites, latch, off, cur, **params):
    """Paints; returns ([names], latch after)."""
    p = dict(DEFAULTS, **params)
    sw, sh = p["signs_w"], p["signs_h"]
    _widget(img, 0, sh, 0, sw, p["border_color"])
    names, latch = choose_signs(latch, off, cur)
    for n in names:
        if n is not None and sprites.get(n) is not None:
            s = sprites[n]
            _sprite(img, s, p["signs_sprite_row"], sw // 2 - s.shape[1] // 2, 2 if n.startswith("lta_") else 3)
    return names, latch


def collision_panel(img, sprites, col, **params):
    p = dict(DEFAULTS, **params)
    W, H = geometry(img.shape, p)
    b, sw = p["border"], img.shape[1]
    _widget(img, H + 2 * b, 2 * H, sw - W - 2 * b, sw, p["border_color"])
    n = choose_collision(col if 0 <= col < 4 else 0)
    if n is not None:
        _sprite(img, sprites.get(n), H + p["collision_sprite_row"], sw - W - p["collision_sprite_col"], 3)
    return n


def compose(img, sprites, latch, off, cur, col, bird_img=None, panels=7, **params):
    """One frame through the three calls in the demo's order.  -> (image, record): record = dict(signs=[names painted], collision=name or
    None, latch=the latch after the frame)."""
    out = np.ascontiguousarray(img, np.uint8).copy()
    names, cn = [None, None], None
    if panels & BIRD:
        bird_panel(out, bird_img, **params)
    if panels & SIGNS:
        names, latch = signs_panel(out, sprites, latch, off, cur, **params)
    if panels & COLLISION:
        cn = collision_panel(out, sprites, col, **params)
    return out, dict(signs=[n for n in names if n is not None], collision=cn, latch=latch)


def panel_pixels(hw, sprites, panels=7, **params):
    """Boolean (h, w): the pixels some panel rectangle of the mask covers (sprites outside their widget not included)."""
    p = dict(DEFAULTS, **params)
    W, H = geometry(hw, p)
    b = p["border"]
    m = np.zeros(hw[:2], bool)
    if panels & BIRD:
        m[0:H + 2 * b, hw[1] - W - 2 * b:] = True
    if panels & SIGNS:
        m[0:p["signs_h"], 0:p["signs_w"]] = True
    if panels & COLLISION:
        m[H + 2 * b:2 * H, hw[1] - W - 2 * b:] = True
    return m
