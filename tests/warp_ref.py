"""NumPy restatement of cv2.warpPerspective(img, M, (w, h), flags=INTER_LINEAR [| WARP_INVERSE_MAP], BORDER_CONSTANT 0) on 8-bit
images: the yardstick of csrc/warp_core.h / warp_kernels.hip (PerspectiveTransformation.transformToBirdView /
transformToFrontalView, perspectiveTransformation.py:89-117).

cv2 is not installed and the reference holds no warped image, so -- as oracle/preprocess.py did for cv2.resize -- this restates
OpenCV 4.5's reference arithmetic (imgproc/src/imgwarp.cpp: WarpPerspectiveInvoker, remapBilinear with 15-bit integer weights).
PARITY UNPINNED against a real cv2 build; the restatement is the yardstick.

    matrix   without the inverse-map flag the 3x3 double matrix is inverted first: adjugate times 1/det, the cofactors written out
             in double, det by first-row expansion, det == 0 an error
    coords   per destination pixel, in double, no FMA: bx = (x // BW) * BW, x1 = x - bx, BW = min(1024 // min(16, dst_h), dst_w);
             X0 = M0*bx + M1*y + M2 (Y0, W0 alike); W = W0 + M6*x1; W = 32/W if W != 0 else 0;
             fX = max(INT_MIN, min(INT_MAX, (X0 + M0*x1)*W)); X = rint(fX) (ties to even); sx = sat_s16(X >> 5), ax = X & 31
    taps     integer weights (32-ax)*(32-ay)*32, ax*(32-ay)*32, (32-ax)*ay*32, ax*ay*32 (sum 2^15) on (sx, sy), (sx+1, sy),
             (sx, sy+1), (sx+1, sy+1); a tap outside the source reads 0; dst = (sum + 2^14) >> 15 in int32
Whether OpenCV's 16-bit weight table stores its (0, 0) entry differently is not known here; this definition makes the identity warp
exact.
"""
import numpy as np

INT_MAX, INT_MIN = 2147483647.0, -2147483648.0


def invert3x3(M):
    m = np.asarray(M, np.float64).reshape(9)
    c0 = m[4] * m[8] - m[5] * m[7]
    c1 = m[3] * m[8] - m[5] * m[6]
    c2 = m[3] * m[7] - m[4] * m[6]
    d = m[0] * c0 - m[1] * c1 + m[2] * c2
    if d == 0.0:
        raise ValueError("singular matrix")
    d = 1.0 / d
    return np.array([c0 * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
                     (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
                     c2 * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d], np.float64)


def block_width(dst_h, dst_w):
    return min(1024 // min(16, dst_h), dst_w)


def _clamp_int(v):
    """std::max((double)INT_MIN, std::min((double)INT_MAX, v)) with <algorithm>'s comparisons (a NaN becomes INT_MAX)."""
    t = np.where(v < INT_MAX, v, INT_MAX)
    return np.where(INT_MIN < t, t, INT_MIN)


def coords(M, dst_hw, inverse=False):
    """-> sx, sy, ax, ay, each (dst_h, dst_w) int64."""
    m = np.asarray(M, np.float64).reshape(9) if inverse else invert3x3(M)
    dh, dw = int(dst_hw[0]), int(dst_hw[1])
    bw = block_width(dh, dw)
    x = np.arange(dw, dtype=np.int64)[None, :]
    y = np.arange(dh, dtype=np.int64)[:, None].astype(np.float64)
    bx = ((x // bw) * bw).astype(np.float64)
    x1 = x.astype(np.float64) - bx
    with np.errstate(all="ignore"):
        X0 = m[0] * bx + m[1] * y + m[2]
        Y0 = m[3] * bx + m[4] * y + m[5]
        W0 = m[6] * bx + m[7] * y + m[8]
        W = W0 + m[6] * x1
        W = np.where(W != 0.0, 32.0 / np.where(W != 0.0, W, 1.0), 0.0)
        fX = _clamp_int((X0 + m[0] * x1) * W)
        fY = _clamp_int((Y0 + m[3] * x1) * W)
    X = np.rint(fX).astype(np.int64)
    Y = np.rint(fY).astype(np.int64)
    sat = lambda v: np.clip(v, -32768, 32767)
    return sat(X >> 5), sat(Y >> 5), X & 31, Y & 31


def warp_perspective(img, M, dst_wh, inverse=False):
    """img (H, W, C) uint8; dst_wh = (width, height) as cv2's dsize -> (height, width, C) uint8."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    sh, sw = img.shape[:2]
    dw, dh = int(dst_wh[0]), int(dst_wh[1])
    sx, sy, ax, ay = coords(M, (dh, dw), inverse)
    src = img.astype(np.int64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
        v = src[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)]
        return np.where(ok[..., None], v, 0)

    w00 = ((32 - ax) * (32 - ay) * 32)[..., None]
    w01 = (ax * (32 - ay) * 32)[..., None]
    w10 = ((32 - ax) * ay * 32)[..., None]
    w11 = (ax * ay * 32)[..., None]
    acc = tap(sy, sx) * w00 + tap(sy, sx + 1) * w01 + tap(sy + 1, sx) * w10 + tap(sy + 1, sx + 1) * w11
    out = (acc + (1 << 14)) >> 15
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)
