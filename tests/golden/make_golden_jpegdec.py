"""Writes tests/golden/jpegdec_streams.npz: baseline JPEG streams from libjpeg (through Pillow) with libjpeg's own decoding of each, for
tests/test_jpegdec_cpu.py and tests/test_gpu_jpegdec.py -- an encoder other than ours (other tables, samplings, restart intervals, APP0) and
an outside decoder to compare with, on machines without Pillow.

    python tests/golden/make_golden_jpegdec.py

Per case i: stream_i (u8), pixels_i (BGR u8 [h][w][3], what Pillow decodes; absent for a reject); names, sizes [n][2] = (w, h), kinds
("444" "422" "420" "grey", or "reject:<flag name>")."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref as ref

SUB = {"444": 0, "422": 1, "420": 2}


def image(content, w, h, seed=0):
    if content == "smooth":
        return ref.smooth(w, h) if seed == 0 else np.ascontiguousarray(ref.smooth(w, h)[::-1, ::-1])
    return ref.content(content, w, h, 1, seed)[0]


def encode(bgr, kind, **kw):
    buf = io.BytesIO()
    if kind == "grey":
        Image.fromarray(bgr[..., 1]).save(buf, "JPEG", **kw)
    else:
        Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", subsampling=SUB[kind], **kw)
    return buf.getvalue()


def decode(stream):
    """libjpeg's pixels as BGR u8."""
    im = Image.open(io.BytesIO(stream))
    a = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(a[..., ::-1])


def cases():
    out = []
    for w, h in ((16, 16), (17, 9), (40, 24), (1, 1)):
        for kind in ("444", "422", "420", "grey"):
            out.append(("base_%dx%d_%s" % (w, h, kind), kind, image("gradient", w, h), dict(quality=90)))
    rst = dict(rb1=dict(restart_marker_blocks=1), rb2=dict(restart_marker_blocks=2), rr1=dict(restart_marker_rows=1))
    for w, h, kind, tags in ((40, 24, "444", ("rb1",)), (40, 24, "422", ("rb2",)), (40, 24, "420", ("rr1",)), (40, 24, "grey", ("rb2",)),
                             (17, 9, "420", ("rb1", "rb2", "rr1")), (17, 9, "422", ("rb1",))):
        for tag in tags:
            out.append(("rst_%dx%d_%s_%s" % (w, h, kind, tag), kind, image("gradient", w, h, 1), dict(quality=85, **rst[tag])))
    for kind in ("444", "422", "420", "grey"):
        out.append(("opt_40x24_%s" % kind, kind, image("noise", 40, 24, 2), dict(quality=75, optimize=True)))
    for q in (30, 90, 100):
        for kind in ("444", "420"):
            out.append(("noise_40x24_%s_q%d" % (kind, q), kind, image("noise", 40, 24, 3), dict(quality=q, restart_marker_rows=1 if kind == "420" else 0)))
    out.append(("binary_17x9_422_q100", "422", image("binary", 17, 9), dict(quality=100)))
    for f in range(2):
        out.append(("frame%d_200x120_420" % f, "420", image("smooth", 200, 120, f), dict(quality=85, restart_marker_rows=1)))
    return out


def main():
    data, names, sizes, kinds = {}, [], [], []
    for name, kind, bgr, kw in cases():
        s = encode(bgr, kind, **kw)
        i = len(names)
        data["stream_%d" % i] = np.frombuffer(s, np.uint8)
        data["pixels_%d" % i] = decode(s)
        names.append(name); sizes.append(bgr.shape[1::-1]); kinds.append(kind)
    g = image("gradient", 16, 16)
    rgb = Image.fromarray(np.ascontiguousarray(g[..., ::-1]))
    rejects = []
    buf = io.BytesIO(); rgb.save(buf, "JPEG", progressive=True); rejects.append(("reject_progressive", buf.getvalue()))
    buf = io.BytesIO(); rgb.save(buf, "JPEG", keep_rgb=True); rejects.append(("reject_keep_rgb", buf.getvalue()))
    buf = io.BytesIO(); rgb.convert("CMYK").save(buf, "JPEG"); rejects.append(("reject_cmyk", buf.getvalue()))
    for name, s in rejects:
        data["stream_%d" % len(names)] = np.frombuffer(s, np.uint8)
        names.append(name); sizes.append((16, 16)); kinds.append("reject:UNSUPPORTED")
    out = os.path.join(HERE, "jpegdec_streams.npz")
    np.savez_compressed(out, names=np.array(names), sizes=np.array(sizes, np.int32), kinds=np.array(kinds), **data)
    print(out, len(names), "cases", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
