"""NumPy / Python-integer restatement of the JPEG decoder's rules D1-D9 (csrc/jpegdec_core.h), written from ITU-T T.81 on its own: a general
marker parser, an entropy decoder over strings of bits with dictionaries of code words (the header uses maxcode / valptr and a look-up), a
float64 inverse DCT next to the integer one as a full matrix product (the header evaluates mirrored sums and differences), and D7 / D8 on
whole planes (the header computes single pixels)."""
import math

import numpy as np

from jpeg_ref import ZIGZAG, huffman_codes

UNSUPPORTED, FORMAT, SIZE, CORRUPT = 1, 2, 4, 8
REJECT = UNSUPPORTED | FORMAT | SIZE
IDCT_ERR_BASE, IDCT_ERR_SLOPE, IDCT_ERR = 0.2337, 1.06e-4, 0.451

M = np.array([[(1.0 if u == 0 else math.sqrt(2) * math.cos((2 * x + 1) * u * math.pi / 16)) for x in range(8)] for u in range(8)])
K = np.rint(8192 * M).astype(np.int64)


class Reject(Exception):
    def __init__(self, flag):
        self.flag = flag


def parse(stream, w, h, capacity=None, length=None):
    """D1, D2: the header of `stream` -> dict(ncomp, hs, vs, dri, q {id: [64] zigzag}, huff {(class, id): (bits, vals)}, tq, td, ta, scan);
    raises Reject(flag)."""
    n = len(stream) if length is None else length
    cap = capacity if capacity else max(len(stream), 1)
    if n <= 0 or n > cap:
        raise Reject(FORMAT)
    s = bytes(stream[:n])
    if s[:2] != b"\xff\xd8":
        raise Reject(FORMAT)
    info = dict(q={}, huff={}, dri=0, adobe=None, sof=False)
    pos = 2
    while True:
        if pos >= n or s[pos] != 0xFF:
            raise Reject(FORMAT)
        while pos < n and s[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise Reject(FORMAT)
        m = s[pos]
        pos += 1
        if m in (0x00, 0xD8, 0xD9):
            raise Reject(FORMAT)
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if pos + 2 > n:
            raise Reject(FORMAT)
        L = int.from_bytes(s[pos:pos + 2], "big")
        if L < 2 or pos + L > n:
            raise Reject(FORMAT)
        body = s[pos + 2:pos + L]
        if m == 0xC0:
            if info["sof"] or L < 8 or L != 8 + 3 * body[5]:
                raise Reject(FORMAT)
            nf = body[5]
            if body[0] != 8 or nf not in (1, 3):
                raise Reject(UNSUPPORTED)
            info["tq"] = []
            for c in range(nf):
                hv, t = body[6 + 3 * c + 1], body[6 + 3 * c + 2]
                if t > 3:
                    raise Reject(FORMAT)
                info["tq"].append(t)
                if nf == 3 and hv not in ((0x22, 0x21, 0x11) if c == 0 else (0x11,)):
                    raise Reject(UNSUPPORTED)
                if c == 0:
                    info["hs"], info["vs"] = (hv >> 4, hv & 15) if nf == 3 else (1, 1)
            if (int.from_bytes(body[3:5], "big"), int.from_bytes(body[1:3], "big")) != (w, h):
                raise Reject(SIZE)
            info["ncomp"], info["sof"] = nf, True
        elif m == 0xDB:
            p = 0
            while p < len(body):
                pq, t = body[p] >> 4, body[p] & 15
                if pq > 1 or t > 3:
                    raise Reject(FORMAT)
                if pq == 1:
                    raise Reject(UNSUPPORTED)
                if p + 65 > len(body):
                    raise Reject(FORMAT)
                info["q"][t] = list(body[p + 1:p + 65])
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(body):
                tc, th = body[p] >> 4, body[p] & 15
                if tc > 1 or th > 3:
                    raise Reject(FORMAT)
                if th > 1:
                    raise Reject(UNSUPPORTED)
                if p + 17 > len(body):
                    raise Reject(FORMAT)
                bits = list(body[p + 1:p + 17])
                if sum(bits) > 256 or p + 17 + sum(bits) > len(body):
                    raise Reject(FORMAT)
                used = 0
                for l in range(1, 17):          # Kraft: code words of length l used up so far, in units of 2^-l
                    used = used * 2 + bits[l - 1]
                    if used > 1 << l:
                        raise Reject(FORMAT)
                info["huff"][(tc, th)] = (bits, list(body[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        elif m == 0xDD:
            if L != 4:
                raise Reject(FORMAT)
            info["dri"] = int.from_bytes(body, "big")
        elif m == 0xDA:
            if not info["sof"] or L < 3 or L != 6 + 2 * body[0]:
                raise Reject(FORMAT)
            ns = body[0]
            if ns != info["ncomp"]:
                raise Reject(UNSUPPORTED)
            info["td"], info["ta"] = [], []
            for c in range(ns):
                t = body[2 + 2 * c]
                if (t >> 4) > 3 or (t & 15) > 3:
                    raise Reject(FORMAT)
                if (t >> 4) > 1 or (t & 15) > 1:
                    raise Reject(UNSUPPORTED)
                info["td"].append(t >> 4)
                info["ta"].append(t & 15)
            if tuple(body[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0):
                raise Reject(UNSUPPORTED)
            if ns == 3 and info["adobe"] == 0:
                raise Reject(UNSUPPORTED)
            for c in range(ns):
                if info["tq"][c] not in info["q"] or (0, info["td"][c]) not in info["huff"] or (1, info["ta"][c]) not in info["huff"]:
                    raise Reject(FORMAT)
            info["scan"] = pos + L
            info["stream"] = s
            return info
        elif 0xE0 <= m <= 0xEF:
            if m == 0xEE and L >= 14 and body[:5] == b"Adobe":
                info["adobe"] = body[11]
        elif m != 0xFE:
            raise Reject(UNSUPPORTED)
        pos += L


def segments(info):
    """D3: (list of the segments' bytes, CORRUPT or 0 for the marker order and count, expected count)."""
    s, i = info["stream"], info["scan"]
    n = len(s)
    segs, start, bad = [], i, 0
    while i < n:
        if s[i] == 0xFF and i + 1 < n and s[i + 1] not in (0x00, 0xFF):
            if 0xD0 <= s[i + 1] <= 0xD7:
                if s[i + 1] - 0xD0 != len(segs) % 8:
                    bad = CORRUPT
                segs.append(s[start:i])
                start = i + 2
                i += 2
                continue
            break
        i += 1
    segs.append(s[start:i])
    info["scan_end"] = i
    hs, vs = info["hs"], info["vs"]
    return segs, bad, hs, vs


def second_scan(s, pos):
    """D2: is there an SOS among the marker segments from `pos` (the scan's end) on?  They are stepped over by their lengths up to EOI, the
    stream's end or the first thing that is no marker segment."""
    n = len(s)
    while pos < n and s[pos] == 0xFF:
        rest = s[pos:].lstrip(b"\xff")          # fill bytes and the marker's own 0xFF
        if not rest:
            return False
        m, pos = rest[0], n - len(rest) + 1
        if m == 0xDA:
            return True
        if m in (0x00, 0xD8, 0xD9):
            return False
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if pos + 2 > n:
            return False
        L = int.from_bytes(s[pos:pos + 2], "big")
        if L < 2 or pos + L > n:
            return False
        pos += L
    return False


def geometry(info, w, h):
    hs, vs = info["hs"], info["vs"]
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    nseg = -(-mcux * mcuy // info["dri"]) if info["dri"] else 1
    return mcux, mcuy, nseg


class _Bits:
    """A segment's data as a string of bits: 0xFF 0x00 is 0xFF, any other 0xFF ends it."""

    def __init__(self, seg):
        out, i = bytearray(), 0
        while i < len(seg):
            if seg[i] == 0xFF:
                if i + 1 < len(seg) and seg[i + 1] == 0:
                    out.append(0xFF)
                    i += 2
                    continue
                break
            out.append(seg[i])
            i += 1
        self.s = format(int.from_bytes(out, "big"), "0%db" % (8 * len(out))) if out else ""
        self.pos = 0

    def symbol(self, table):
        for l in range(1, 17):
            v = table.get(self.s[self.pos:self.pos + l]) if self.pos + l <= len(self.s) else None
            if v is not None:
                self.pos += l
                return v
        return None

    def value(self, size):
        if self.pos + size > len(self.s):
            return None
        x = int(self.s[self.pos:self.pos + size], 2)
        self.pos += size
        return x if x >> (size - 1) else x - (1 << size) + 1


def _block(bits, dc, ac, q, pred):
    """D4, D5 on one block -> ([64] natural order, new predictor), or None on an error."""
    t = bits.symbol(dc)
    if t is None or t > 11:
        return None
    d = 0
    if t:
        d = bits.value(t)
        if d is None:
            return None
    pred = max(-32768, min(32767, pred + d))
    out = [0] * 64
    out[0] = max(-2048, min(2047, pred * q[0]))
    k = 1
    while k < 64:
        rs = bits.symbol(ac)
        if rs is None:
            return None
        run, size = rs >> 4, rs & 15
        if size == 0:
            if run == 0:
                break
            if run != 15 or k > 48:
                return None
            k += 16
            continue
        k += run
        if size > 10 or k > 63:
            return None
        v = bits.value(size)
        if v is None:
            return None
        out[ZIGZAG[k]] = max(-2048, min(2047, v * q[k]))
        k += 1
    return out, pred


def coefficients(info, w, h):
    """D3-D5: (per component [bh][bw][64] int64 natural order, CORRUPT or 0)."""
    mcux, mcuy, nseg = geometry(info, w, h)
    segs, flag, hs, vs = segments(info)
    if len(segs) != nseg:
        flag = CORRUPT
    inv = {k: {c: s for s, c in huffman_codes(*v).items()} for k, v in info["huff"].items()}
    samp = [(hs, vs)] + [(1, 1)] * (info["ncomp"] - 1)
    coef = [np.zeros((mcuy * v, mcux * hh, 64), np.int64) for hh, v in samp]
    dri = info["dri"] or mcux * mcuy
    for k, seg in enumerate(segs[:nseg]):
        bits, pred, ok = _Bits(seg), [0] * info["ncomp"], True
        for m in range(k * dri, min((k + 1) * dri, mcux * mcuy)):
            mx, my = m % mcux, m // mcux
            for c, (hh, v) in enumerate(samp):
                for by in range(v):
                    for bx in range(hh):
                        r = _block(bits, inv[(0, info["td"][c])], inv[(1, info["ta"][c])], info["q"][info["tq"][c]], pred[c]) if ok else None
                        if r is None:
                            ok, flag = False, CORRUPT
                            continue
                        coef[c][my * v + by, mx * hh + bx], pred[c] = r
    return coef, flag


def idct_exact(F):
    """[n][64] -> f [n][8][8] float64, the orthonormal inverse DCT (without the level shift)."""
    F = np.asarray(F, np.float64).reshape(-1, 8, 8)
    return np.einsum("vy,nvu,ux->nyx", M, F, M) / 8


def idct_int(F):
    """D6: [n][64] -> (acc [n][8][8], the sums in front of the last shift; samples [n][8][8] in 0..255)."""
    F = np.asarray(F, np.int64).reshape(-1, 8, 8)
    T = (np.einsum("nvu,ux->nvx", F, K) + 2048) >> 12
    acc = np.einsum("vy,nvx->nyx", K, T)
    return acc, np.clip(((acc + 65536) >> 17) + 128, 0, 255)


def plane_of(blocks):
    """[bh][bw][8][8] -> [bh * 8][bw * 8]"""
    bh, bw = blocks.shape[:2]
    return blocks.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def planes(coef, exact=False):
    out = []
    for c in coef:
        bh, bw = c.shape[:2]
        if exact:
            px = np.clip(np.rint(idct_exact(c.reshape(-1, 64))) + 128, 0, 255).astype(np.int64)
        else:
            px = idct_int(c.reshape(-1, 64))[1]
        out.append(plane_of(px.reshape(bh, bw, 8, 8)))
    return out


def upsample(c, hs, vs, w, h):
    """D7: a chroma plane (MCU-padded) -> [h][w]."""
    c = np.asarray(c, np.int64)
    if hs == 1:
        return c[:h, :w]
    cw = (w + 1) // 2
    if vs == 1:
        c = c[:h, :cw]
        left, right = np.concatenate([c[:, :1], c[:, :-1]], 1), np.concatenate([c[:, 1:], c[:, -1:]], 1)
        out = np.zeros((h, 2 * cw), np.int64)
        out[:, 0::2] = (3 * c + left + 1) >> 2
        out[:, 1::2] = (3 * c + right + 2) >> 2
        out[:, 0], out[:, 2 * cw - 1] = c[:, 0], c[:, -1]
        return out[:, :w]
    ch = (h + 1) // 2
    c = c[:ch, :cw]
    up, down = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    s = np.zeros((2 * ch, cw), np.int64)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + down
    left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.zeros((2 * ch, 2 * cw), np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out[:h, :w]


def colour(y, cb, cr):
    """D8 -> BGR u8 [h][w][3]."""
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], 2), 0, 255).astype(np.uint8)


def pixels(pl, info, w, h):
    y = np.asarray(pl[0], np.int64)[:h, :w]
    if info["ncomp"] == 1:
        return np.stack([y, y, y], 2).astype(np.uint8)
    return colour(y, upsample(pl[1], info["hs"], info["vs"], w, h), upsample(pl[2], info["hs"], info["vs"], w, h))


class Decoded:
    pass


def decode(stream, w, h, capacity=None, length=None, exact=False):
    """One stream -> Decoded(flags, info, coef, planes, bgr).  exact=True: the float64 inverse DCT rounded to nearest in place of D6."""
    d = Decoded()
    d.coef, d.planes, d.info = [], [], None
    try:
        d.info = parse(stream, w, h, capacity, length)
    except Reject as r:
        d.flags, d.bgr = r.flag, np.zeros((h, w, 3), np.uint8)
        return d
    segments(d.info)
    if second_scan(d.info["stream"], d.info["scan_end"]):
        d.flags, d.bgr = UNSUPPORTED, np.zeros((h, w, 3), np.uint8)
        return d
    d.coef, d.flags = coefficients(d.info, w, h)
    d.planes = planes(d.coef, exact)
    d.bgr = pixels(d.planes, d.info, w, h)
    return d

