"""Independent statement of the scaling stage's rules S2-S6 (csrc/scale_core.h states them; this file shares no code with it): BGR frames ->
the canvases of tiles, in NumPy and Python integers.  S5 (`area`) is taken straight from the weight formula over every source index; S4
(`linear`) is oracle.preprocess.cv_resize_linear_u8, the project's restatement of OpenCV's 8-bit INTER_LINEAR: UNPINNED against a real cv2."""
import numpy as np

from oracle.preprocess import cv_resize_linear_u8

DEFAULT_COLORS = ((0, 255, 255), (0, 255, 0), (0, 102, 255), (0, 0, 255))   # UNKNOWN, NORMAL, PROMPT, WARNING as BGR


def area_weights(dn, sn):
    """int64 [dn][sn]: S5's weight of source index s for destination index d, 0 where s lies outside d's span"""
    W = np.zeros((dn, sn), np.int64)
    for d in range(dn):
        for s in range(sn):
            if s * dn < (d + 1) * sn and (s + 1) * dn > d * sn:
                W[d, s] = min((s + 1) * dn, (d + 1) * sn) - max(s * dn, d * sn)
    return W


def resize_area(img, size):
    """img [h][w][3] u8 -> [dst_h][dst_w][3] u8 by S5"""
    sh, sw = img.shape[:2]
    dw, dh = size
    assert dw <= sw and dh <= sh and sw * sh <= 1 << 23
    Wx, Wy = area_weights(dw, sw), area_weights(dh, sh)
    D = sw * sh
    num = np.einsum("ys,xt,stc->yxc", Wy, Wx, img.astype(np.int64))
    return ((num + D // 2) // D).astype(np.uint8)


def resize(img, size, mode):
    return resize_area(img, size) if mode == "area" else cv_resize_linear_u8(np.ascontiguousarray(img), size)


def canvases(batch, mosaic):
    T = mosaic[0] * mosaic[1]
    return -(-batch // T)


def scale(bgr, size, mode="area", mosaic=(1, 1), border=0, background=(0, 0, 0), border_colors=DEFAULT_COLORS, states=None):
    """bgr [batch][h][w][3] -> uint8 [canvases][rows * dst_h][cols * dst_w][3] by S2-S6"""
    bgr = np.asarray(bgr, np.uint8)
    batch = bgr.shape[0]
    dw, dh = size
    cols, rows = mosaic
    T = cols * rows
    out = np.empty((canvases(batch, mosaic), rows * dh, cols * dw, 3), np.uint8)
    out[:] = np.asarray(background, np.uint8)
    for f in range(batch):
        tile = resize(bgr[f], size, mode)
        if border > 0 and states is not None:
            st = int(states[f])
            colour = np.asarray(border_colors[st if 0 <= st <= 3 else 0], np.uint8)
            ring = np.ones((dh, dw), bool)
            ring[border:dh - border, border:dw - border] = False
            tile = tile.copy()
            tile[ring] = colour
        k, cell = divmod(f, T)
        r, c = divmod(cell, cols)
        out[k, r * dh:(r + 1) * dh, c * dw:(c + 1) * dw] = tile
    return out
