"""NumPy / Python-integer restatement of the JPEG encoder's rules J1-J9 (csrc/jpeg_core.h), written from ITU-T T.81 on its own: the tables
are typed in again, the DCT matrix is rounded here from its formula and applied as a full matrix (the header evaluates mirrored sums and
differences), the entropy coder builds strings of bits.  decode() is a small baseline Huffman decoder that turns a stream back into the
quantised levels, without any inverse transform."""
import math

import numpy as np

HEADER_BYTES = 611
FDCT_ERR = 1.75
OVERFLOW = 1

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
assert sorted(ZIGZAG) == list(range(64))

BASE = np.array([        # Annex K.1, K.2, natural order
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32], np.int64)

_AC_TAIL = [r * 16 + s for r in range(16) for s in range(1, 11)]
BITS = {         # Annex K.3: (Tc, Th) -> (codes per length 1..16, values)
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
             [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
              0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
              0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
              0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
              0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
              0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
              0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
              0xfa]),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
              0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
              0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
              0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
              0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
              0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
              0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
              0xfa]),
}
for _k, (_b, _v) in BITS.items():      # every table lists each symbol once; the AC tables hold EOB, ZRL and every (run, size 1..10)
    assert sum(_b) == len(_v) == len(set(_v))
    assert _k[0] == 0 or sorted(_v) == sorted(_AC_TAIL + [0x00, 0xF0])


def huffman_codes(bits, vals):
    """Annex C: symbol -> string of bits."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = format(code, "0%db" % length)
            code += 1
            k += 1
        code <<= 1
    return out


CODES = {k: huffman_codes(*v) for k, v in BITS.items()}


def qtables(quality):
    """J5: the two divisor tables, natural order, [2][64]."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((BASE * s + 50) // 100, 1, 255)


def dct_matrix():
    """K = round(8192 M), M[u][x] = c(u) sqrt(2) cos((2x + 1) u pi / 16)."""
    return np.array([[round(8192 * (1.0 if u == 0 else math.sqrt(2) * math.cos((2 * x + 1) * u * math.pi / 16))) for x in range(8)] for u in range(8)],
                    np.int64)


K = dct_matrix()


def fdct(f):
    """[n][8][8] level-shifted samples -> F' [n][8][8] (J4)."""
    f = np.asarray(f, np.int64).reshape(-1, 8, 8)
    t = (np.einsum("nyx,ux->nyu", f, K) + 256) >> 9
    return (np.einsum("vy,nyu->nvu", K, t) + 65536) >> 17


def fdct_exact(f):
    """8 F in float64, F the orthonormal DCT."""
    f = np.asarray(f, np.float64).reshape(-1, 8, 8)
    M = np.array([[(1.0 if u == 0 else math.sqrt(2) * math.cos((2 * x + 1) * u * math.pi / 16)) for x in range(8)] for u in range(8)])
    return np.einsum("vy,nyx,ux->nvu", M, f, M)


def quantise(F, d):
    """[n][8][8] F' and [8][8] divisors -> levels (J5)."""
    F = np.asarray(F, np.int64)
    a = (np.abs(F) + 4 * d) // (8 * d)
    ac = np.ones((8, 8), bool)
    ac[0, 0] = False
    a = np.where(ac & (a > 1023), 1023, a)
    return np.where(F < 0, -a, a)


def components(img):
    """J1-J3: BGR u8 [h][w][3] -> (Y [H][W], Cb [H/2][W/2], Cr), H and W the sizes padded to 16 by edge replication, values 0..255."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    p = np.pad(img, ((0, -h % 16), (0, -w % 16), (0, 0)), mode="edge").astype(np.int64)
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    y = np.clip((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, 0, 255)
    cb = np.clip((-11059 * r - 21709 * g + 32768 * b + 8388608 + 32768) >> 16, 0, 255)
    cr = np.clip((32768 * r - 27439 * g - 5329 * b + 8388608 + 32768) >> 16, 0, 255)
    half = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    return y, half(cb), half(cr)


def blocks_of(plane):
    """[H][W] -> [H/8][W/8][8][8]"""
    H, W = plane.shape
    return plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)


def levels(img, quality):
    """The quantised levels in coding order: [mcu_h][6 * mcu_w][64], zigzag."""
    y, cb, cr = components(img)
    q = qtables(quality).reshape(2, 8, 8)
    ly = quantise(fdct(blocks_of(y - 128).reshape(-1, 8, 8)), q[0]).reshape(y.shape[0] // 8, y.shape[1] // 8, 64)
    lc = [quantise(fdct(blocks_of(c - 128).reshape(-1, 8, 8)), q[1]).reshape(c.shape[0] // 8, c.shape[1] // 8, 64) for c in (cb, cr)]
    mh, mw = cb.shape[0] // 8, cb.shape[1] // 8
    out = np.zeros((mh, mw, 6, 64), np.int64)
    for k in range(4):
        out[:, :, k] = ly[k >> 1::2, k & 1::2]
    out[:, :, 4], out[:, :, 5] = lc
    return out[..., ZIGZAG].reshape(mh, mw * 6, 64)


def _value_bits(v):
    s = abs(v).bit_length()
    return s, (format(v if v >= 0 else v + (1 << s) - 1, "0%db" % s) if s else "")


def code_block(lev, pred, cls):
    """One block's levels (zigzag) with DC predictor `pred` -> its string of bits (J6)."""
    s, vb = _value_bits(int(lev[0]) - pred)
    out = [CODES[(0, cls)][s], vb]
    ac, run = CODES[(1, cls)], 0
    for k in range(1, 64):
        v = int(lev[k])
        if v == 0:
            run += 1
            continue
        while run >= 16:
            out.append(ac[0xF0])
            run -= 16
        s, vb = _value_bits(v)
        out += [ac[(run << 4) | s], vb]
        run = 0
    if run:
        out.append(ac[0x00])
    return "".join(out)


def header(w, h, quality):
    q = qtables(quality)
    o = bytearray(b"\xff\xd8")
    for c in range(2):
        o += b"\xff\xdb" + (67).to_bytes(2, "big") + bytes([c]) + bytes(int(q[c][z]) for z in ZIGZAG)
    o += b"\xff\xc0" + (17).to_bytes(2, "big") + bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc, th in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = BITS[(tc, th)]
        o += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([tc << 4 | th]) + bytes(bits) + bytes(vals)
    o += b"\xff\xdd" + (4).to_bytes(2, "big") + ((w + 15) // 16).to_bytes(2, "big")
    o += b"\xff\xda" + (12).to_bytes(2, "big") + bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(o) == HEADER_BYTES
    return bytes(o)


def bound(w, h):
    mw, mh = (w + 15) // 16, (h + 15) // 16
    return HEADER_BYTES + 6 * mw * mh * 416 + 2 * (mh - 1) + 2


def encode(img, quality, lev=None):
    """One frame -> its stream (J1-J7)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    lev = levels(img, quality) if lev is None else lev
    out = bytearray(header(w, h, quality))
    for row in range(lev.shape[0]):
        pred, bits = [0, 0, 0], []
        for b in range(lev.shape[1]):
            comp = max(0, b % 6 - 3)
            bits.append(code_block(lev[row, b], pred[comp], comp > 0))
            pred[comp] = int(lev[row, b, 0])
        s = "".join(bits)
        s += "1" * (-len(s) % 8)
        raw = int(s, 2).to_bytes(len(s) // 8, "big")
        out += raw.replace(b"\xff", b"\xff\x00")
        if row + 1 < lev.shape[0]:
            out += bytes([0xFF, 0xD0 + row % 8])
    return bytes(out + b"\xff\xd9")


def encode_batch(frames, quality, capacity, fill=0):
    """J8 on a batch: (out [n][capacity] pre-filled with `fill`, lengths, flags)."""
    out = np.full((len(frames), capacity), fill, np.uint8)
    lengths, flags = np.zeros(len(frames), np.int64), np.zeros(len(frames), np.int32)
    for f, img in enumerate(frames):
        s = encode(img, quality)
        if len(s) > capacity:
            flags[f] = OVERFLOW
        else:
            out[f, :len(s)] = np.frombuffer(s, np.uint8)
            lengths[f] = len(s)
    return out, lengths, flags


# ------------------------------------------------------------------------------------------------ what the CPU and the GPU tests encode
# (width, height, frames): one MCU; whole MCUs; partial MCUs in both directions, twice; 10 segments (the RST index wraps); one full-width
# segment (two rounds of 256 blocks in the entropy kernel); three frames of three segments
SHAPES = ((16, 16, 1), (48, 32, 1), (40, 24, 1), (17, 9, 1), (16, 160, 1), (1280, 16, 1), (1280, 48, 3))
QUALITIES = (1, 50, 90, 100)
CONTENTS = ("noise", "binary", "flat0", "flat255", "flat128", "gradient")


def gradient(w, h, seed=0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = 0.7 * seed
    img = np.stack([127.5 + 120 * np.sin(x / max(w, 8) * 2.1 + ph) * np.cos(y / max(h, 8) * 1.3),
                    127.5 + 110 * np.cos(x / max(w, 8) * 1.2 - y / max(h, 8) * 1.7 + ph),
                    40 + 170 * (x + 2 * y) / (w + 2 * h)], axis=2)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def content(name, w, h, n=1, seed=0):
    """[n][h][w][3] u8: uniform noise; a random 0 / 255 pattern (the longest codes, many stuffed bytes); flat frames (EOB-only blocks, DC
    difference 0); a smooth gradient.  Frame f differs from frame 0 where the content is not flat."""
    rng = np.random.default_rng([seed, w, h, CONTENTS.index(name)])
    if name == "noise":
        return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if name == "binary":
        return (rng.integers(0, 2, (n, h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    if name.startswith("flat"):
        return np.full((n, h, w, 3), int(name[4:]), np.uint8)
    return np.stack([gradient(w, h, seed + f) for f in range(n)])


def smooth(w, h):
    """A low-frequency gradient plus a few flat rectangles: what the PSNR comparison with another encoder runs on."""
    img = gradient(w, h, 3).copy()
    for k, (y0, x0, y1, x1, c) in enumerate(((0.1, 0.1, 0.4, 0.35, (200, 40, 40)), (0.5, 0.55, 0.9, 0.8, (30, 180, 220)), (0.3, 0.6, 0.45, 0.95, (128, 128, 128)))):
        img[int(y0 * h):int(y1 * h), int(x0 * w):int(x1 * w)] = c
    return img


# ------------------------------------------------------------------------------------------------ the decoder of the entropy layer
def parse(stream):
    """The marker segments in front of the first restart segment: dict(w, h, dri, q [2][64] zigzag, huff {(tc, th): (bits, vals)}, markers, scan)."""
    assert stream[:2] == b"\xff\xd8" and stream[-2:] == b"\xff\xd9"
    info, i = dict(q={}, huff={}, markers=["SOI"]), 2
    while True:
        assert stream[i] == 0xFF, i
        m, n = stream[i + 1], int.from_bytes(stream[i + 2:i + 4], "big")
        body = stream[i + 4:i + 2 + n]
        if m == 0xDB:
            assert body[0] >> 4 == 0 and len(body) == 65
            info["q"][body[0] & 15] = list(body[1:])
            info["markers"].append("DQT")
        elif m == 0xC0:
            assert body[0] == 8 and body[5] == 3 and bytes(body[6:]) == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
            info["h"], info["w"] = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            info["markers"].append("SOF0")
        elif m == 0xC4:
            bits = list(body[1:17])
            info["huff"][(body[0] >> 4, body[0] & 15)] = (bits, list(body[17:]))
            assert len(body) == 17 + sum(bits)
            info["markers"].append("DHT")
        elif m == 0xDD:
            info["dri"] = int.from_bytes(body, "big")
            info["markers"].append("DRI")
        elif m == 0xDA:
            assert bytes(body) == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
            info["markers"].append("SOS")
            info["scan"] = i + 2 + n
            return info
        else:
            raise AssertionError("marker 0x%02x" % m)
        i += 2 + n


def decode(stream):
    """A stream -> (info, levels [mcu_h][6 * mcu_w][64] in zigzag order): marker order, restart markers, stuffing, padding and every code checked
    on the way."""
    info = parse(stream)
    assert info["markers"] == ["SOI", "DQT", "DQT", "SOF0", "DHT", "DHT", "DHT", "DHT", "DRI", "SOS"], info["markers"]
    mw, mh = (info["w"] + 15) // 16, (info["h"] + 15) // 16
    assert info["dri"] == mw
    inv = {k: {c: s for s, c in huffman_codes(*v).items()} for k, v in info["huff"].items()}
    body = stream[info["scan"]:-2]
    segs, start, i = [], 0, 0
    while i < len(body):           # inside a segment 0xFF is followed by 0x00; anything else is the next restart marker
        if body[i] == 0xFF:
            if body[i + 1] == 0:
                i += 2
                continue
            assert body[i + 1] == 0xD0 + len(segs) % 8, (len(segs), body[i + 1])
            segs.append(body[start:i])
            start = i = i + 2
            continue
        i += 1
    segs.append(body[start:])
    assert len(segs) == mh
    out = np.zeros((mh, 6 * mw, 64), np.int64)

    def symbol(s, pos, table):
        for n in range(1, 17):
            v = table.get(s[pos:pos + n])
            if v is not None:
                return v, pos + n
        raise AssertionError("no code at bit %d" % pos)

    def value(s, pos, n):
        if n == 0:
            return 0, pos
        v = int(s[pos:pos + n], 2)
        return (v if v >> (n - 1) else v - (1 << n) + 1), pos + n

    for row, seg in enumerate(segs):
        raw = bytes(seg).replace(b"\xff\x00", b"\xff")
        s = format(int.from_bytes(raw, "big"), "0%db" % (8 * len(raw))) if raw else ""
        pos, pred = 0, [0, 0, 0]
        for b in range(6 * mw):
            comp = max(0, b % 6 - 3)
            cls = int(comp > 0)
            n, pos = symbol(s, pos, inv[(0, cls)])
            d, pos = value(s, pos, n)
            pred[comp] += d
            out[row, b, 0] = pred[comp]
            k = 1
            while k < 64:
                rs, pos = symbol(s, pos, inv[(1, cls)])
                if rs == 0:
                    break
                if rs == 0xF0:
                    k += 16
                    continue
                k += rs >> 4
                assert k < 64
                out[row, b, k], pos = value(s, pos, rs & 15)
                k += 1
        assert len(s) - pos < 8 and set(s[pos:]) <= {"1"}, (row, len(s) - pos)      # padded with 1-bits to the byte, nothing behind
    return info, out
