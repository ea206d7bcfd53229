"""Independent NumPy statement of the YUV output's rules E1-E6 (csrc/yuvout_core.h states them; this file shares no code with it): BGR frames
-> the bytes of NV12 / NV21 / I420 / YUYV / UYVY frames at any byte layout, whole arrays in int64.  Where a byte lies inside a frame is
tests/yuv_ref.py's statement of the layout rule C2 (NumPy as well); the layouts the tests run are here."""
import numpy as np

import yuv_ref

FORMATS = yuv_ref.FORMATS
MATRICES = yuv_ref.MATRICES
CHROMA = ("mean", "first")
FIELDS = yuv_ref.FIELDS
KINDS = ("tight", "odd", "wide", "tall", "gap")
is420 = yuv_ref.is420
frame_bytes = yuv_ref.frame_bytes


def layout(fmt, w, h, kind="tight"):
    """yuv_ref's layouts -- "tight"; "odd": pitches = row bytes + 1 and an odd frame stride; "wide": pitches + 16; "tall": every chroma plane
    behind a plane padded by 6 rows -- and "gap": the tight planes 32 bytes into a frame whose stride leaves 48 more behind them."""
    if kind != "gap":
        return yuv_ref.layout(fmt, w, h, kind)
    L = yuv_ref.layout(fmt, w, h, "tight")
    L["y_offset"] += 32
    if fmt not in ("yuyv", "uyvy"):
        L["u_offset"] += 32
    if fmt == "i420":
        L["v_offset"] += 32
    L["frame_stride"] += 80
    return L


def batch_bytes(fmt, w, h, L, batch):
    return (batch - 1) * L["frame_stride"] + frame_bytes(fmt, w, h, L)


def colour(bgr, matrix="video"):
    """E3 / E4 on (..., 3) BGR -> (..., 3) int64 Y, U, V"""
    bgr = np.asarray(bgr).astype(np.int64)
    B, G, R = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    if matrix == "video":
        half = 1 << 19
        Y = (269484 * R + 528482 * G + 102760 * B + half + (16 << 20)) >> 20
        U = (-155188 * R - 305135 * G + 460324 * B + half + (128 << 20)) >> 20
        V = (460324 * R - 385875 * G - 74448 * B + half + (128 << 20)) >> 20
    elif matrix == "full":          # jpeg_core.h J2
        Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
        U = (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32768) >> 16
        V = (32768 * R - 27439 * G - 5329 * B + 8388608 + 32768) >> 16
    else:
        raise ValueError(matrix)
    return np.clip(np.stack([Y, U, V], -1), 0, 255)


def planes(bgr, fmt, matrix="video", chroma="mean"):
    """[n][h][w][3] BGR -> Y [n][h][w], U and V [n][h or h / 2][w / 2] (E5)"""
    yuv = colour(bgr, matrix)
    n, h, w, _ = yuv.shape
    Y, U, V = yuv[..., 0], yuv[..., 1], yuv[..., 2]
    if is420(fmt):
        if chroma == "first":
            return Y, U[:, ::2, ::2], V[:, ::2, ::2]
        cell = lambda a: (a.reshape(n, h // 2, 2, w // 2, 2).sum((2, 4)) + 2) >> 2
        return Y, cell(U), cell(V)
    if chroma == "first":
        return Y, U[:, :, ::2], V[:, :, ::2]
    cell = lambda a: (a.reshape(n, h, w // 2, 2).sum(3) + 1) >> 1
    return Y, cell(U), cell(V)


def to_yuv(bgr, fmt, L=None, matrix="video", chroma="mean", fill=0xA5):
    """[n][h][w][3] BGR -> uint8 [batch_bytes]: the frames at layout L (default tight), every byte no plane row owns = fill."""
    bgr = np.asarray(bgr)
    if bgr.ndim == 3:
        bgr = bgr[None]
    n, h, w, _ = bgr.shape
    L = L or layout(fmt, w, h)
    Y, U, V = planes(bgr, fmt, matrix, chroma)
    iy, iu, iv = yuv_ref._index(fmt, w, h, L)          # per pixel; a cell's pixels share iu and iv
    step = (slice(None, None, 2), slice(None, None, 2)) if is420(fmt) else (slice(None), slice(None, None, 2))
    iu, iv = iu[step], iv[step]
    buf = np.full(batch_bytes(fmt, w, h, L, n), fill, np.uint8)
    for f in range(n):
        o = f * L["frame_stride"]
        buf[o + iy], buf[o + iu], buf[o + iv] = Y[f], U[f], V[f]
    return buf


def plane_mask(fmt, w, h, L, batch):
    """bool [batch_bytes]: the bytes plane rows own"""
    iy, iu, iv = yuv_ref._index(fmt, w, h, L)
    m = np.zeros(batch_bytes(fmt, w, h, L, batch), bool)
    for f in range(batch):
        o = f * L["frame_stride"]
        m[o + iy] = m[o + iu] = m[o + iv] = True
    return m
