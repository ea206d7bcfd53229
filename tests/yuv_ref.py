"""Independent NumPy statement of the YUV conversion's rules C1-C6 (csrc/yuv_core.h states them; this file shares no code with it): frames
in NV12 / NV21 / I420 / YUYV / UYVY at any byte layout -> BGR, in int64, every plane indexed by (x >> 1, y >> 1) or (x >> 1, y).  Also the
inverse the tests need -- BGR -> the bytes of a frame in each format (BT.601, any consistent rounding: only the bytes matter) -- and the
layouts the tests run."""
import numpy as np

FORMATS = ("nv12", "nv21", "i420", "yuyv", "uyvy")
MATRICES = ("video", "full")
FIELDS = ("frame_stride", "y_offset", "y_pitch", "u_offset", "u_pitch", "v_offset", "v_pitch")


def is420(fmt):
    return fmt in ("nv12", "nv21", "i420")


def row_bytes(fmt, w):
    """(bytes of a row of the Y or packed plane, of a chroma plane)"""
    if fmt in ("yuyv", "uyvy"):
        return 2 * w, 0
    return w, (w // 2 if fmt == "i420" else w)


def layout(fmt, w, h, kind="tight"):
    """C2 layouts: "tight"; "odd": pitches = row bytes + 1; "wide": pitches + 16; "tall": tight pitches, each chroma plane behind a plane padded
    by 6 rows (NV12's chroma offset is y_pitch * (h + 6))."""
    ry, rc = row_bytes(fmt, w)
    add = {"tight": 0, "odd": 1, "wide": 16, "tall": 0}[kind]
    pad = 6 if kind == "tall" else 0
    L = dict.fromkeys(FIELDS, 0)
    L["y_pitch"] = ry + add
    end = L["y_pitch"] * (h + pad)
    if rc:
        L["u_offset"], L["u_pitch"] = end, rc + add
        end += L["u_pitch"] * (h // 2 + pad)
    if fmt == "i420":
        L["v_offset"], L["v_pitch"] = end, rc + add
        end += L["v_pitch"] * (h // 2 + pad)
    L["frame_stride"] = end + (1 if kind == "odd" else 0)
    if kind == "odd" and L["frame_stride"] % 2 == 0:
        L["frame_stride"] += 1
    return L


def frame_bytes(fmt, w, h, L):
    """bytes of a frame that belong to its planes' rows: up to the end of the last plane"""
    ry, rc = row_bytes(fmt, w)
    end = L["y_offset"] + (h - 1) * L["y_pitch"] + ry
    if rc:
        end = max(end, L["u_offset"] + (h // 2 - 1) * L["u_pitch"] + rc)
    if fmt == "i420":
        end = max(end, L["v_offset"] + (h // 2 - 1) * L["v_pitch"] + rc)
    return end


def source_bytes(fmt, w, h, L, batch):
    return (batch - 1) * L["frame_stride"] + frame_bytes(fmt, w, h, L)


def _index(fmt, w, h, L):
    """byte index inside a frame of every pixel's Y, U and V: three int64 [h][w]"""
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    cx = x >> 1
    if fmt in ("yuyv", "uyvy"):
        base = L["y_offset"] + y * L["y_pitch"]
        if fmt == "yuyv":
            return base + 2 * x, base + 4 * cx + 1, base + 4 * cx + 3
        return base + 2 * x + 1, base + 4 * cx, base + 4 * cx + 2
    cy = y >> 1
    iy = L["y_offset"] + y * L["y_pitch"] + x
    if fmt == "i420":
        return iy, L["u_offset"] + cy * L["u_pitch"] + cx, L["v_offset"] + cy * L["v_pitch"] + cx
    pair = L["u_offset"] + cy * L["u_pitch"] + 2 * cx
    return (iy, pair, pair + 1) if fmt == "nv12" else (iy, pair + 1, pair)


def colour(Y, U, V, matrix="video"):
    """C4 / C5 on int64 arrays -> (..., 3) uint8 BGR"""
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    u, v = U - 128, V - 128
    if matrix == "video":
        y = np.maximum(0, Y - 16) * 1220542 + (1 << 19)
        b = (y + 2116026 * u) >> 20
        g = (y - 852492 * v - 409993 * u) >> 20
        r = (y + 1673527 * v) >> 20
    elif matrix == "full":          # jpegdec_core.h D8
        r = Y + ((91881 * v + 32768) >> 16)
        b = Y + ((116130 * u + 32768) >> 16)
        g = Y + ((-22554 * u - 46802 * v + 32768) >> 16)
    else:
        raise ValueError(matrix)
    return np.clip(np.stack(np.broadcast_arrays(b, g, r), -1), 0, 255).astype(np.uint8)


def to_bgr(buf, fmt, w, h, L, matrix="video", batch=1):
    """buf: uint8 bytes of `batch` frames at L -> [batch][h][w][3]"""
    buf = np.asarray(buf, np.uint8)
    iy, iu, iv = _index(fmt, w, h, L)
    out = np.empty((batch, h, w, 3), np.uint8)
    for f in range(batch):
        o = f * L["frame_stride"]
        out[f] = colour(buf[o + iy], buf[o + iu], buf[o + iv], matrix)
    return out


def from_bgr(bgr, fmt, L=None, fill=0):
    """[batch][h][w][3] BGR -> the bytes of the frames at layout L (default tight), bytes outside the planes' rows = fill.  BT.601 limited
    range, chroma averaged over a sample's cell."""
    bgr = np.asarray(bgr, np.float64)
    if bgr.ndim == 3:
        bgr = bgr[None]
    n, h, w, _ = bgr.shape
    L = L or layout(fmt, w, h)
    B, G, R = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    Y = 16 + (65.481 * R + 128.553 * G + 24.966 * B) / 255
    U = 128 + (-37.797 * R - 74.203 * G + 112.0 * B) / 255
    V = 128 + (112.0 * R - 93.786 * G - 18.214 * B) / 255
    if is420(fmt):
        U = U.reshape(n, h // 2, 2, w // 2, 2).mean((2, 4))
        V = V.reshape(n, h // 2, 2, w // 2, 2).mean((2, 4))
        U, V = (np.repeat(np.repeat(a, 2, 1), 2, 2) for a in (U, V))
    else:
        U = np.repeat(U.reshape(n, h, w // 2, 2).mean(3), 2, 2)
        V = np.repeat(V.reshape(n, h, w // 2, 2).mean(3), 2, 2)
    q = lambda a: np.clip(np.floor(a + 0.5), 0, 255).astype(np.uint8)
    iy, iu, iv = _index(fmt, w, h, L)
    buf = np.full(source_bytes(fmt, w, h, L, n), fill, np.uint8)
    for f in range(n):
        o = f * L["frame_stride"]
        buf[o + iy], buf[o + iu], buf[o + iv] = q(Y[f]), q(U[f]), q(V[f])
    return buf
