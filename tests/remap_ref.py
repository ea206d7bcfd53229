"""NumPy restatement of cv2.initUndistortRectifyMap(K, D, R, new_K, (w, h), cv2.CV_16SC2) and cv2.remap(img, map1, map2, INTER_LINEAR,
BORDER_CONSTANT 0) on 8-bit images -- together cv2.undistort: the yardstick of csrc/remap_core.h / remap_kernels.hip, rules U1-U6 in the
header's association.

cv2 is not installed, so -- as tests/warp_ref.py did for cv2.warpPerspective -- this restates OpenCV 4.5's reference arithmetic.  PARITY
UNPINNED against a real cv2 build; the restatement is the yardstick.  OpenCV accumulates X, Y, W along a row; here, as in the header,
they are evaluated per pixel, which can move a map entry only when it sits on a 1/32 tie.

    model   A = new_K * R (A[0][j] = fx'*R[0][j] + cx'*R[2][j], ...), iR = adjugate / determinant (warp_ref.invert3x3)
            X = iR0*x + (iR1*y + iR2) (Y, W alike); w = 1/W; xn = X*w; yn = Y*w; x2, y2, r2 = x2 + y2, _2xy = 2*xn*yn
            kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)
            xd = xn*kr + p1*_2xy + p2*(r2 + 2*x2); yd = yn*kr + p1*(r2 + 2*y2) + p2*_2xy; u = fx*xd + cx; v = fy*yd + cy
            iu = rint(clamp_int(u * 32)); sx = sat_s16(iu >> 5); ax = iu & 31 (iv, sy, ay alike)
    map     xy (h, w, 2) int16 = (sx, sy), frac (h, w) uint16 = ay * 32 + ax; the top 6 bits of frac are ignored on read
    taps    warp_ref's: integer weights that sum to 2^15, a tap outside the source reads 0, dst = (sum + 2^14) >> 15
"""
import numpy as np

from warp_ref import invert3x3, _clamp_int

LENSES = {"identity": (0, 0, 0, 0), "barrel": (-0.2, 0.05, 0.001, -0.001), "rational": (-0.2, 0.05, 0.001, -0.001, 0.01, 0.1, 0.02, 0.003),
          "pincushion": (0.15, 0.02, 0.001, -0.001)}


def camera(K, D=(), new_K=None, R=None):
    """The four parameter lists padded and defaulted: K (4), D (8), new_K (4), R (9) float64."""
    K = np.asarray(K, np.float64).reshape(4)
    D = np.asarray(D, np.float64).reshape(-1)
    assert D.size in (0, 4, 5, 8)
    D = np.concatenate([D, np.zeros(8 - D.size)])
    new_K = K.copy() if new_K is None else np.asarray(new_K, np.float64).reshape(4)
    R = np.eye(3).reshape(9) if R is None else np.asarray(R, np.float64).reshape(9)
    return K, D, new_K, R


def inverse_rectification(new_K, R):
    A = np.empty(9)
    for j in range(3):
        A[j] = new_K[0] * R[j] + new_K[2] * R[6 + j]
        A[3 + j] = new_K[1] * R[3 + j] + new_K[3] * R[6 + j]
        A[6 + j] = R[6 + j]
    return invert3x3(A)


def model_coords(K, D, new_K, R, dst_hw):
    """-> iu, iv (dst_h, dst_w) int64: the rounded 1/32-pixel source coordinates of every destination pixel, steps 1-6."""
    K, D, new_K, R = camera(K, D, new_K, R)
    iR = inverse_rectification(new_K, R)
    k1, k2, p1, p2, k3, k4, k5, k6 = D
    x = np.arange(int(dst_hw[1]), dtype=np.float64)[None, :]
    y = np.arange(int(dst_hw[0]), dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X = iR[0] * x + (iR[1] * y + iR[2])
        Y = iR[3] * x + (iR[4] * y + iR[5])
        W = iR[6] * x + (iR[7] * y + iR[8])
        w = 1.0 / W
        xn, yn = X * w, Y * w
        x2, y2 = xn * xn, yn * yn
        r2, _2xy = x2 + y2, 2 * xn * yn
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = xn * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
        yd = yn * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
        u, v = K[0] * xd + K[2], K[1] * yd + K[3]
        iu = np.rint(_clamp_int(u * 32)).astype(np.int64)
        iv = np.rint(_clamp_int(v * 32)).astype(np.int64)
    return iu, iv


def build_map(K, D=(), new_K=None, R=None, dst_hw=None):
    """-> xy (h, w, 2) int16, frac (h, w) uint16: cv2's map1, map2 of initUndistortRectifyMap(..., CV_16SC2)."""
    iu, iv = model_coords(K, D, new_K, R, dst_hw)
    xy = np.stack([np.clip(iu >> 5, -32768, 32767), np.clip(iv >> 5, -32768, 32767)], -1).astype(np.int16)
    return xy, ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)


def remap(img, xy, frac):
    """img (H, W, C) uint8 through the map -> (h, w, C) uint8."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    sh, sw = img.shape[:2]
    sx, sy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    ax, ay = (frac & 31).astype(np.int64), ((frac >> 5) & 31).astype(np.int64)
    src = img.astype(np.int64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < sh) & (xx >= 0) & (xx < sw)
        return np.where(ok[..., None], src[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)], 0)

    w00, w01 = ((32 - ax) * (32 - ay) * 32)[..., None], (ax * (32 - ay) * 32)[..., None]
    w10, w11 = ((32 - ax) * ay * 32)[..., None], (ax * ay * 32)[..., None]
    out = (tap(sy, sx) * w00 + tap(sy, sx + 1) * w01 + tap(sy + 1, sx) * w10 + tap(sy + 1, sx + 1) * w11 + (1 << 14)) >> 15
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def remap_batch(frames, maps, stream_map, n_streams):
    """U5: frame f belongs to stream f % n_streams and reads maps[stream_map[stream]]."""
    return np.stack([remap(fr, *maps[stream_map[f % n_streams]]) for f, fr in enumerate(frames)])


def crafted_map(src_hw, dst_hw, shift=0):
    """The table of saturated and edge entries: sx, sy out of {-32768, -2, -1, 0, n-3, n-2, n-1, n, 32767}, fractions out of {0, 1, 16, 31};
    at 36x36 every combination once.  Every other entry carries junk in the ignored top 6 bits of its fraction word."""
    sh, sw = src_hw
    j = np.arange(dst_hw[0] * dst_hw[1], dtype=np.int64) + shift
    SX = np.array([-32768, -2, -1, 0, sw - 3, sw - 2, sw - 1, sw, 32767])
    SY = np.array([-32768, -2, -1, 0, sh - 3, sh - 2, sh - 1, sh, 32767])
    F = np.array([0, 1, 16, 31])
    xy = np.stack([SX[j % 9], SY[(j // 9) % 9]], -1).astype(np.int16).reshape(dst_hw[0], dst_hw[1], 2)
    frac = (F[(j // 324) % 4] * 32 + F[(j // 81) % 4] + np.where(j & 1, 0xfc00, 0)).astype(np.uint16).reshape(dst_hw)
    return xy, frac


def lcg_bytes(n, seed=12345):
    """The bounds program's frame generator."""
    out, s = np.empty(n, np.uint8), seed
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xffffffff
        out[i] = s >> 24
    return out
